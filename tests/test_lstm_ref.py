"""tests/lstm_ref.py (float64 numpy) against torch.nn.LSTM(16, 16, L,
batch_first=True).double() + gather + autograd on the CPU, on every input set
of lstm_ref.SETS: outputs and every gradient within 1e-12 of each tensor's
largest magnitude.

The same test measures torch's float32 CPU LSTM against lstm_ref on the same
inputs: what an independent float32 implementation of the encoder gives, the
figures the bounds of tests/test_gpu_lstm.py are judged against.  Recorded
(torch 2.x CPU; out: max abs error, the others: max abs error / max |ref|):

    set   out      d_vocab  dW_ih    dW_hh    db
    a     1.4e-08  2.4e-07  1.9e-07  0        1.9e-07
    b     6.8e-08  2.2e-07  2.0e-07  1.5e-07  1.0e-07
    c     3.5e-08  1.9e-07  3.1e-07  2.4e-07  2.9e-07
    d     5.8e-08  2.9e-07  5.0e-07  3.9e-07  2.6e-06
    e     1.3e-07  4.4e-07  5.2e-07  3.6e-07  2.3e-06
    f     5.1e-08  3.4e-07  3.4e-07  4.1e-07  4.9e-06
    g15   3.7e-08  2.4e-07  3.6e-07  3.3e-07  1.8e-07
    g16   2.7e-08  1.5e-07  2.4e-07  5.5e-07  4.2e-07

(db: the worse of torch's bias_ih and bias_hh gradients, which it sums
separately.)  The test prints the figures of the torch at hand.
"""
import numpy as np
import pytest
import torch

import lstm_ref

EXTRA = 9  # token-table rows beyond n: ridx is drawn with repetition from a larger table


def torch_lstm(c, ridx, d_out, dtype):
    """(out, d_vocab, [(dW_ih, dW_hh, db)]) of torch.nn.LSTM in `dtype` under autograd."""
    L = c["L"]
    rnn = torch.nn.LSTM(16, 16, L, batch_first=True).to(dtype)
    with torch.no_grad():
        for l, layer in enumerate(c["layers"]):
            for name, p in zip(("weight_ih", "weight_hh", "bias_ih", "bias_hh"), layer):
                getattr(rnn, "%s_l%d" % (name, l)).copy_(torch.from_numpy(p).to(dtype))
    vocab = torch.from_numpy(c["vocab"]).to(dtype).requires_grad_(True)
    tok = torch.from_numpy(c["tokens"].astype(np.int64))[torch.from_numpy(ridx)]
    seq, _ = rnn(vocab[tok])
    idx = (tok != c["pad"]).sum(-1) - 1
    out = seq.gather(1, idx.view(-1, 1, 1).expand(-1, 1, 16)).squeeze(1)
    (out * torch.from_numpy(d_out).to(dtype)).sum().backward()
    g = lambda name, l: getattr(rnn, "%s_l%d" % (name, l)).grad.numpy()  # noqa: E731
    # (torch sums the two biases' gradients separately: equal to rounding only)
    return out.detach().numpy(), vocab.grad.numpy(), [(g("weight_ih", l), g("weight_hh", l), g("bias_ih", l),
                                                         g("bias_hh", l)) for l in range(L)]


def errors(got, want):
    """{quantity: max abs error (out) or max abs error / max |want| (gradients), worst layer}."""
    rel = lambda a, b: float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))  # noqa: E731
    return {"out": float(np.abs(got[0] - want[0]).max()), "d_vocab": rel(got[1], want[1]),
            "dW_ih": max(rel(a[0], b[0]) for a, b in zip(got[2], want[2])),
            "dW_hh": max((rel(a[1], b[1]) for a, b in zip(got[2], want[2]) if np.abs(b[1]).max() > 0), default=0.0),
            "db": max(rel(a[k], b[2]) for a, b in zip(got[2], want[2]) for k in range(2, len(a)))}


@pytest.mark.parametrize("name", sorted(lstm_ref.SETS))
def test_lstm_ref_matches_torch_float64(name):
    c = lstm_ref.case(name, extra=EXTRA)
    ridx = lstm_ref.ridx_for(c)
    d_out = np.random.default_rng(7).standard_normal((len(ridx), 16)).astype(np.float32)
    want = lstm_ref.grads(c["vocab"], c["layers"], c["tokens"], c["pad"], ridx, d_out)
    assert np.array_equal(want[0], lstm_ref.encode(c["vocab"], c["layers"], c["tokens"][ridx], c["pad"]))
    assert np.all(want[1][c["pad"]] == 0)
    if c["T"] > 1:
        assert all(np.abs(w[1]).max() > 0 for w in want[2])
    t64 = torch_lstm(c, ridx, d_out, torch.float64)
    for (a, b, what) in [(want[0], t64[0], "out"), (want[1], t64[1], "d_vocab")] + \
            [(want[2][l][min(k, 2)], t64[2][l][k], "%s_l%d" % (("dW_ih", "dW_hh", "db_ih", "db_hh")[k], l))
             for l in range(c["L"]) for k in range(4)]:
        assert a.shape == b.shape and a.dtype == np.float64, what
        assert np.abs(a - b).max() <= 1e-12 * max(np.abs(b).max(), 1e-300), (name, what)
    e = errors(torch_lstm(c, ridx, d_out, torch.float32), want)
    print("float32 CPU torch vs lstm_ref, set %-3s: out %.2e  d_vocab %.2e  dW_ih %.2e  dW_hh %.2e  db %.2e"
          % (name, e["out"], e["d_vocab"], e["dW_ih"], e["dW_hh"], e["db"]))


def test_head_only_rows_have_no_recurrent_gradient():
    """Rows of one token: h_prev is zero at the only step, so dW_hh is exactly 0."""
    c = lstm_ref.case("c")
    tok = np.full_like(c["tokens"], c["pad"])
    tok[:, 0] = c["tokens"][:, 0]
    ridx = np.arange(len(tok), dtype=np.int64)
    d_out = np.random.default_rng(8).standard_normal((len(ridx), 16))
    _, d_vocab, wg = lstm_ref.grads(c["vocab"], c["layers"], tok, c["pad"], ridx, d_out)
    assert all(np.all(w[1] == 0) and np.abs(w[0]).max() > 0 for w in wg)
    assert np.all(d_vocab[c["pad"]] == 0)
