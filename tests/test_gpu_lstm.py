"""The LSTM rule encoder's kernels (rnnlogic_amd/csrc/encode.hip) against the
float64 reference of tests/lstm_ref.py, called through the C ABI so that the
shapes, ld_out, ridx and the scratch contents are the test's own, and the
model path (PredictorPlus) on a small synthetic graph.

Input sets: lstm_ref.SETS (1-3 layers, 1-8 tokens, 1 .. 16,391 rows); the
training runs draw ridx with repetition from a token table of n + 9 rows, and
hand the kernels act / da / xh / dvx / part / weight-gradient / d_vocab
buffers filled with NaN, so that an element the kernels should have written
and did not, or read and should not have, shows.

Bounds (against float64, no rtol): outputs max |out - ref| <= 2e-6; every
gradient tensor max |g - ref| <= 1e-5 max |ref| + 1e-6.  tests/test_lstm_ref.py
records what torch's float32 CPU LSTM gives on the same inputs.

Observed on an MI355X (out: max abs error; gradients: max abs error / max
|ref|, the worst layer), no bound raised; test_zz_print_figures prints the table:

    case         out      d_vocab  dW_ih    dW_hh    db
    encode a-g   <= 7.4e-08 (set e, saturated gates: 2.1e-07)
    trie i  L=1/2/3   1.3e-07 / 4.0e-08 / 3.7e-08
    trie ii L=1/3     1.9e-07 / 7.1e-08
    train a      3.6e-08  2.3e-07  1.1e-07  0        8.5e-08
    train b      6.7e-08  1.8e-07  2.6e-07  2.5e-07  2.2e-07
    train c      5.2e-08  1.6e-07  3.8e-07  3.0e-07  1.8e-07
    train d      6.2e-08  5.2e-07  6.2e-07  5.8e-07  1.2e-06
    train e      2.1e-07  4.1e-07  6.9e-07  9.2e-07  9.1e-07
    train f      5.8e-08  4.8e-07  4.9e-07  5.5e-07  6.7e-07
    train g15    3.5e-08  1.7e-07  2.6e-07  4.6e-07  2.2e-07
    train g16    2.7e-08  2.2e-07  2.8e-07  4.1e-07  2.4e-07
    half-zero    <= 2.1e-07  5.6e-07  6.8e-07  6.3e-07  6.0e-07   (worst set)
    head-only    <= 7.1e-08  3.8e-07  5.7e-07  0        9.1e-07   (worst set)
    model L=1/2 (train)  7.2e-08 / 3.1e-08; gradients <= 3.5e-07
    model L=4    3.3e-08 (torch's LSTM), scores 2.4e-07 from the numpy model
    model 9 tokens       <= 7.2e-08

rnnl_lstm_train_forward's rows are bitwise rnnl_lstm_encode's on every set.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import lstm_ref
import synth_graphs as sg
from oracle import reference_np as ref
from rnnlogic_amd import _native

pytestmark = pytest.mark.gpu

OUT_TOL = 2e-6
EXTRA = 9  # token-table rows beyond n in the training runs
SET_NAMES = sorted(lstm_ref.SETS)
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class DevWeights(object):
    """One model's parameters on the device: stacked (rnnl_lstm_encode) and
    as arrays of per-layer pointers (the trie and the training entry points)."""

    def __init__(self, vocab, layers, dev):
        self.L = len(layers)
        self.vocab = up(vocab, dev)
        self.per_layer = [[up(p, dev) for p in layer] for layer in layers]
        self.stacked = [up(np.stack([layer[k] for layer in layers]), dev) for k in range(4)]
        self.arrs = [(ctypes.c_void_p * 3)(*[self.per_layer[l][k].data_ptr() for l in range(self.L)])
                     for k in range(4)]

    def stacked_ptrs(self):
        return [t.data_ptr() for t in self.stacked]


def hip_encode(w, tok, pad, dev, ld_out=16, guard=0, fill=NAN):
    """rnnl_lstm_encode over the host rows tok (n, T): the whole (n + guard, ld_out) buffer."""
    n, T = tok.shape
    out = torch.full((n + guard, ld_out), fill, dtype=torch.float32, device=dev)
    tk = up(tok.astype(np.int32), dev)
    _native.call("rnnl_lstm_encode", w.vocab.data_ptr(), *w.stacked_ptrs(), w.L, 16, tk.data_ptr(), n, T, pad,
                 out.data_ptr(), ld_out, stream(dev))
    torch.cuda.synchronize()
    return out


_figures = {}


def note(case, what, value):
    _figures.setdefault(case, {})[what] = max(_figures.get(case, {}).get(what, 0.0), value)


def check_out(got, want, case, what="out"):
    assert got.shape == want.shape and np.isfinite(got).all(), (case, what)
    err = float(np.abs(got.astype(np.float64) - want).max())
    note(case, what, err)
    print("%s %s: max |got - f64| = %.3g (bound %.1g)" % (case, what, err, OUT_TOL))
    assert err <= OUT_TOL, (case, what, err)


def check_grad(got, want, case, what):
    assert got.shape == want.shape, (case, what, got.shape, want.shape)
    assert np.isfinite(got).all(), (case, what, "non-finite gradient")
    scale = float(np.abs(want).max())
    err = float(np.abs(got.astype(np.float64) - want).max())
    bound = 1e-5 * scale + 1e-6
    note(case, what.split("_l")[0], err / scale if scale else err)
    print("%s %s: max |got - f64| = %.3g = %.3g max|ref| (bound %.3g)" % (case, what, err, err / scale if scale else 0,
                                                                         bound))
    assert err <= bound, (case, what, err, bound)


# --------------------------------------------------------------------------- rnnl_lstm_encode
_cases = {}


def case_of(name):
    """The input set and its float64 outputs, computed once."""
    if name not in _cases:
        c = lstm_ref.case(name)
        c["out"] = lstm_ref.encode(c["vocab"], c["layers"], c["tokens"], c["pad"])
        _cases[name] = c
    return _cases[name]


@pytest.mark.parametrize("name", SET_NAMES)
def test_encode_matches_float64(name, dev):
    """rnnl_lstm_encode of every input set, into rows of 24 floats with two
    guard rows: the 16 columns match the reference, everything else keeps its
    bits."""
    c = case_of(name)
    n = c["n"]
    w = DevWeights(c["vocab"], c["layers"], dev)
    sentinel = -12345.678
    out = hip_encode(w, c["tokens"], c["pad"], dev, ld_out=24, guard=2, fill=sentinel)
    check_out(out[:n, :16].cpu().numpy(), c["out"], "encode " + name)
    untouched = torch.full_like(out, sentinel).view(torch.int32)
    bits = out.view(torch.int32)
    assert torch.equal(bits[:n, 16:], untouched[:n, 16:]), "columns 16-23 were written"
    assert torch.equal(bits[n:], untouched[n:]), "the guard rows were written"
    # the plain layout gives the same rows, bitwise
    assert torch.equal(hip_encode(w, c["tokens"], c["pad"], dev), out[:n, :16])


def test_encode_argument_errors(dev):
    """Shapes the kernels do not support: RNNL_ERR_INVALID, rnnl_last_error set, out untouched."""
    c = case_of("b")
    w = DevWeights(c["vocab"], c["layers"], dev)
    tk = up(np.concatenate([c["tokens"], c["tokens"]], axis=1).astype(np.int32), dev)  # wide enough for seq_len 9
    out = torch.full((c["n"], 24), 77.0, dtype=torch.float32, device=dev)
    lib = _native.lib()
    good = dict(layers=1, hidden=16, seq_len=8, ld_out=24)
    for bad in (dict(seq_len=9), dict(layers=0), dict(layers=4), dict(hidden=8), dict(ld_out=15)):
        a = dict(good, **bad)
        # another entry point's message first: the one read below is this call's
        assert lib.rnnl_lstm_weight_grads_scratch(0, 1, ctypes.byref(ctypes.c_size_t())) == _native.RNNL_ERR_INVALID
        assert b"weight_grads_scratch" in lib.rnnl_last_error()
        rc = lib.rnnl_lstm_encode(w.vocab.data_ptr(), *w.stacked_ptrs(), a["layers"], a["hidden"], tk.data_ptr(),
                                  c["n"], a["seq_len"], c["pad"], out.data_ptr(), a["ld_out"], stream(dev))
        assert rc == _native.RNNL_ERR_INVALID, bad
        assert b"rnnl_lstm_encode:" in lib.rnnl_last_error(), bad
    torch.cuda.synchronize()
    assert bool((out == 77.0).all())


# --------------------------------------------------------------------------- the trie forms
R_I, R_II = 6, 24


def rules_i():
    """Bodies of length 1-7 over 6 tokens, three heads: a chain of strict
    prefixes (rules ending at interior nodes), identical rules (one node, two
    output rows), a repeated token."""
    chain = [1, 2, 3, 4, 5, 0, 1]
    rules = [(0, chain[:k]) for k in range(1, 8)]
    rules += [(0, [2, 2, 2]), (0, [1, 2]), (0, [3, 0]), (0, [5]), (1, [0, 0]), (1, [0, 0, 4]), (1, [4, 3, 2, 1]),
              (1, [4, 3, 2, 1]), (1, [2]), (3, [3] * 7), (3, [1, 5]), (0, [3, 0, 3])]
    return rules


def rules_ii():
    """One head, all 24^3 bodies of length 3 but the last three (13,821 nodes
    on the deepest full level: the wide kernel, one live node in its last
    group) and a few bodies of length 4 under them."""
    bodies = [list(b) for b in itertools.product(range(R_II), repeat=3)][:-3]
    assert len(bodies) == 13821 and len(bodies) % 4 == 1
    bodies += [[0, 0, 0, 5], [23, 23, 20, 1], [7, 11, 13, 17], [7, 11, 13, 18]]
    return [(0, b) for b in bodies]


def padded(rules, pad, T=None):
    T = T or 1 + max(len(b) for _, b in rules)
    return np.asarray([[h] + list(b) + [pad] * (T - 1 - len(b)) for h, b in rules], dtype=np.int32)


class NativeRules(object):
    """An rnnl_rules handle for a rule list; the graph supplies only the relation count."""

    def __init__(self, rules, R, dev):
        from rnnlogic_amd.data import _DeviceHandle
        hrt = np.asarray([[0, 0, 1]], dtype=np.int32)
        g = ctypes.c_void_p()
        with torch.cuda.device(dev):
            _native.call("rnnl_graph_create", hrt.ctypes.data_as(ctypes.c_void_p), 1, 2, R, ctypes.byref(g))
            self.graph = _DeviceHandle(g, "rnnl_graph_destroy")
            flat, ptr = [], [0]
            for h, b in rules:
                flat += [h] + list(b)
                ptr.append(len(flat))
            tok = np.ascontiguousarray(flat, dtype=np.int32)
            ptr = np.ascontiguousarray(ptr, dtype=np.int64)
            h = ctypes.c_void_p()
            _native.call("rnnl_rules_create", g, tok.ctypes.data_as(ctypes.c_void_p),
                         ptr.ctypes.data_as(ctypes.c_void_p), len(rules), ctypes.byref(h))
            self.rules = _DeviceHandle(h, "rnnl_rules_destroy")
        info = (ctypes.c_int32 * 5)()
        _native.call("rnnl_rules_info", h, info)
        assert info[0] == len(rules)
        self.n_nodes, self.record = info[1], info[3]
        self.ptr = h


_lists = {}


def rule_list(which):
    """(rules, relation count, padded tokens) of list 'i' or 'ii'."""
    if which not in _lists:
        rules, R = (rules_i(), R_I) if which == "i" else (rules_ii(), R_II)
        _lists[which] = (rules, R, padded(rules, R))
    return _lists[which]


@pytest.mark.parametrize("which,L", [("i", 1), ("i", 2), ("i", 3), ("ii", 1), ("ii", 3)])
def test_trie_encoder(which, L, dev):
    """rnnl_lstm_encode_trie is bitwise rnnl_lstm_encode of the same padded
    rules (the header's contract) and matches the reference; the node records
    rnnl_lstm_encode_trie_sum forms are bitwise rnnl_node_weights' of those
    rows; scratch one byte short is refused."""
    rules, R, tok = rule_list(which)
    n = len(rules)
    rng = np.random.default_rng(50 + L)
    vocab = rng.standard_normal((R + 1, 16)).astype(np.float32)
    vocab[R] = 0
    layers = lstm_ref.weights(L, seed=L)
    w = DevWeights(vocab, layers, dev)
    nr = NativeRules(rules, R, dev)
    nbytes = ctypes.c_size_t()
    _native.call("rnnl_lstm_encode_trie_scratch", nr.ptr, L, ctypes.byref(nbytes))
    assert nbytes.value == nr.n_nodes * L * 32 * 4
    # the per-node states start as NaN: a state read before it is written shows
    state = torch.full((nbytes.value,), 0xFF, dtype=torch.uint8, device=dev)
    out = torch.full((n, 16), NAN, dtype=torch.float32, device=dev)
    _native.call("rnnl_lstm_encode_trie", nr.ptr, w.vocab.data_ptr(), *w.arrs, L, 16, out.data_ptr(), 16,
                 state.data_ptr(), state.numel(), stream(dev))
    per_rule = hip_encode(w, tok, R, dev)
    assert torch.equal(out, per_rule), float((out - per_rule).abs().max())
    check_out(out.cpu().numpy(), lstm_ref.encode(vocab, layers, tok, R), "trie %s L=%d" % (which, L))
    # one byte short
    before = out.clone()
    lib = _native.lib()
    rc = lib.rnnl_lstm_encode_trie(nr.ptr, w.vocab.data_ptr(), *w.arrs, L, 16, out.data_ptr(), 16, state.data_ptr(),
                                   state.numel() - 1, stream(dev))
    assert rc == _native.RNNL_ERR_INVALID and b"rnnl_lstm_encode_trie" in lib.rnnl_last_error()
    assert torch.equal(out, before)
    # the SUM records, with the rows in a wider buffer
    add_w = up(rng.uniform(-0.25, 0.25, (16, 16)).astype(np.float32), dev)
    wbytes = ctypes.c_size_t()
    _native.call("rnnl_node_weights_size", nr.ptr, _native.AGG_SUM, ctypes.byref(wbytes))
    n_rec = nr.n_nodes * nr.record
    assert wbytes.value == n_rec + 64
    fused = torch.full((wbytes.value,), 0xAB, dtype=torch.uint8, device=dev)
    state.fill_(0xFF)
    rows = torch.full((n, 24), NAN, dtype=torch.float32, device=dev)
    _native.call("rnnl_lstm_encode_trie_sum", nr.ptr, w.vocab.data_ptr(), *w.arrs, L, 16, rows.data_ptr(), 24,
                 state.data_ptr(), state.numel(), add_w.data_ptr(), fused.data_ptr(), stream(dev))
    assert torch.equal(rows[:, :16], out)
    assert bool(torch.isnan(rows[:, 16:]).all())
    sep = torch.full_like(fused, 0xCD)
    _native.call("rnnl_node_weights", nr.ptr, out.data_ptr(), 16, _native.AGG_SUM, add_w.data_ptr(), sep.data_ptr(),
                 stream(dev))
    torch.cuda.synchronize()
    assert torch.equal(fused[:n_rec + 32], sep[:n_rec + 32])


# --------------------------------------------------------------------------- training kernels
def run_train(c, tokens, ridx, d_out, dev):
    """rnnl_lstm_train_forward / _backward / rnnl_lstm_weight_grads on NaN-filled
    buffers -> dict of host arrays (out, d_vocab, dW_ih, dW_hh, db (L, ...))
    and the device tensors da / xh / dvx."""
    L, T, pad = c["L"], tokens.shape[1], c["pad"]
    n = len(ridx)
    w = DevWeights(c["vocab"], c["layers"], dev)
    sizes = [ctypes.c_size_t() for _ in range(4)]
    _native.call("rnnl_lstm_train_sizes", L, 16, T, n, *[ctypes.byref(x) for x in sizes])
    assert [x.value for x in sizes] == [L * T * 6 * n * 16, L * n * T * 64, L * n * T * 32, n * T * 16]
    nan = lambda k: torch.full((k,), NAN, dtype=torch.float32, device=dev)  # noqa: E731
    act, da, xh, dvx = [nan(x.value) for x in sizes]
    out = nan(n * 16).view(n, 16)
    tk, rd = up(tokens.astype(np.int32), dev), up(ridx.astype(np.int64), dev)
    assert 0 <= ridx.min() and ridx.max() < len(tokens)
    st = stream(dev)
    _native.call("rnnl_lstm_train_forward", w.vocab.data_ptr(), *w.arrs, L, 16, tk.data_ptr(), T, pad, rd.data_ptr(),
                 n, out.data_ptr(), act.data_ptr(), st)
    tok_id, ptr, pos = lstm_ref.token_csr(tokens[ridx], pad)
    assert pos.size == 0 or (pos.max() < n * T and tok_id.max() < len(c["vocab"]))
    t_id, t_ptr, t_pos = up(tok_id, dev), up(ptr, dev), up(pos, dev)
    d_vocab = nan(c["vocab"].size).view(c["vocab"].shape)
    g = up(d_out.astype(np.float32), dev)
    _native.call("rnnl_lstm_train_backward", w.vocab.data_ptr(), *w.arrs, L, 16, tk.data_ptr(), T, pad, rd.data_ptr(),
                 n, act.data_ptr(), g.data_ptr(), da.data_ptr(), xh.data_ptr(), dvx.data_ptr(), t_id.data_ptr(),
                 t_ptr.data_ptr(), t_pos.data_ptr(), len(tok_id), d_vocab.data_ptr(), len(c["vocab"]), st)
    rows = n * T
    n_part = ctypes.c_size_t()
    _native.call("rnnl_lstm_weight_grads_scratch", L, rows, ctypes.byref(n_part))
    assert n_part.value == (rows + 127) // 128 * L * 33 * 64
    part, wg = nan(n_part.value), nan(L * 64 * 33)
    _native.call("rnnl_lstm_weight_grads", da.data_ptr(), xh.data_ptr(), L, rows, part.data_ptr(), n_part.value,
                 wg.data_ptr(), st)
    torch.cuda.synchronize()
    h = wg.cpu().numpy()
    return dict(out=out.cpu().numpy(), d_vocab=d_vocab.cpu().numpy(), dW_ih=h[:L * 1024].reshape(L, 64, 16),
                dW_hh=h[L * 1024:L * 2048].reshape(L, 64, 16), db=h[L * 2048:].reshape(L, 64), da=da, xh=xh, dvx=dvx,
                w=w)


def check_train(got, want, c, tokens, ridx, case):
    out, d_vocab, wg = want
    check_out(got["out"], out, case)
    # the pad steps' rows are written (as zeros): nothing of the NaN fill is left
    for k in ("da", "xh", "dvx"):
        assert bool(torch.isfinite(got[k]).all()), (case, k)
    check_grad(got["d_vocab"], d_vocab, case, "d_vocab")
    for l in range(c["L"]):
        for k, name in enumerate(("dW_ih", "dW_hh", "db")):
            check_grad(got[name][l], wg[l][k], case, "%s_l%d" % (name, l))
    assert np.all(got["d_vocab"][c["pad"]] == 0), "the pad row has a gradient"
    unused = np.setdiff1d(np.arange(len(c["vocab"])), np.unique(tokens[ridx]))
    assert len(unused) >= 1 and np.all(got["d_vocab"][unused] == 0), "an unused vocab row has a gradient"


_train = {}


def train_case(name):
    """The input set with a token table of n + EXTRA rows, ridx drawn with
    repetition, an upstream gradient and the float64 results, computed once."""
    if name not in _train:
        c = lstm_ref.case(name, extra=EXTRA)
        ridx = lstm_ref.ridx_for(c)
        if c["n"] > c["T"]:
            assert len(np.unique(ridx)) < len(ridx)
        d_out = np.random.default_rng(7).standard_normal((len(ridx), 16)).astype(np.float32)
        want = lstm_ref.grads(c["vocab"], c["layers"], c["tokens"], c["pad"], ridx, d_out)
        _train[name] = (c, ridx, d_out, want)
    return _train[name]


@pytest.mark.parametrize("name", SET_NAMES)
def test_train_matches_float64(name, dev):
    """Outputs and every gradient against the reference; the forward's rows
    are bitwise rnnl_lstm_encode's; a second run gives bitwise the same
    gradients (the fixed summation order)."""
    c, ridx, d_out, want = train_case(name)
    got = run_train(c, c["tokens"], ridx, d_out, dev)
    check_train(got, want, c, c["tokens"], ridx, "train " + name)
    enc = hip_encode(got["w"], c["tokens"][ridx], c["pad"], dev).cpu().numpy()
    assert np.array_equal(enc.view(np.int32), got["out"].view(np.int32)), \
        "rnnl_lstm_train_forward's rows are not bitwise rnnl_lstm_encode's"
    again = run_train(c, c["tokens"], ridx, d_out, dev)
    for k in ("out", "d_vocab", "dW_ih", "dW_hh", "db"):
        assert np.array_equal(got[k].view(np.int32), again[k].view(np.int32)), (name, k)


@pytest.mark.parametrize("name", SET_NAMES)
def test_train_zero_upstream_on_half_the_rows(name, dev):
    c, ridx, d_out, _ = train_case(name)
    d_out = d_out.copy()
    d_out[::2] = 0
    want = lstm_ref.grads(c["vocab"], c["layers"], c["tokens"], c["pad"], ridx, d_out)
    check_train(run_train(c, c["tokens"], ridx, d_out, dev), want, c, c["tokens"], ridx, "half-zero " + name)


@pytest.mark.parametrize("name", SET_NAMES)
def test_train_head_only_rows(name, dev):
    """Every row is its head token alone: h_prev is zero at the only step, dW_hh exactly 0."""
    c, ridx, d_out, _ = train_case(name)
    tokens = np.full_like(c["tokens"], c["pad"])
    tokens[:, 0] = c["tokens"][:, 0]
    want = lstm_ref.grads(c["vocab"], c["layers"], tokens, c["pad"], ridx, d_out)
    got = run_train(c, tokens, ridx, d_out, dev)
    check_train(got, want, c, tokens, ridx, "head-only " + name)
    assert np.all(got["dW_hh"] == 0)


# --------------------------------------------------------------------------- the model path
def model_spec():
    """30 entities, 6 relations, 170 distinct random facts; the queries are facts of relation 0."""
    rng = np.random.default_rng(21)
    E, facts, seen = 30, [], set()
    while len(facts) < 170:
        f = (int(rng.integers(E)), int(rng.integers(R_I)), int(rng.integers(E)))
        if f not in seen:
            seen.add(f)
            facts.append(f)
    queries = {"q%d" % k: (h, t) for k, (h, r, t) in enumerate([f for f in facts if f[1] == 0][:6])}
    return sg.Spec("lstm", E, R_I, facts, queries, [(h, list(b)) for h, b in rules_i()])


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    from rnnlogic_amd.data import KnowledgeGraph
    spec = model_spec()
    path, _ = sg.write(spec, tmp_path_factory.mktemp("lstm") / spec.name)
    return spec, path, KnowledgeGraph(path)


def build_model(env, rules, L, dev, seed=0):
    from rnnlogic_amd.predictors import PredictorPlus
    torch.manual_seed(seed)
    m = PredictorPlus(env[2], type="lstm", num_layers=L, hidden_dim=16, entity_feature="bias", aggregator="sum")
    m.set_rules([[h] + list(b) for h, b in rules])
    with torch.no_grad():
        m.bias.normal_()
    return m.to(dev)


def state_of(model, L):
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    layers = [tuple(sd["rnn.%s_l%d" % (n, l)] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
              for l in range(L)]
    return sd, layers


def both_forms(model):
    with torch.no_grad():
        model.encoder_trie = True
        a = model.all_rule_embeddings().clone()
        model.encoder_trie = False
        b = model.all_rule_embeddings().clone()
    model.encoder_trie = True
    return a, b


@pytest.mark.parametrize("L", [1, 2])
def test_model_eval_and_train(L, env, dev):
    """PredictorPlus with 1 and 2 layers: all_rule_embeddings over the trie
    and per rule (bitwise equal) against the reference, and the training
    path's parameter gradients."""
    rules = rules_i()
    model = build_model(env, rules, L, dev).eval()
    sd, layers = state_of(model, L)
    tok = model.rule_features.numpy()
    assert tok.shape == (len(rules), 8)
    want = lstm_ref.encode(sd["vocab_emb.weight"], layers, tok, R_I)
    a, b = both_forms(model)
    assert torch.equal(a, b)
    check_out(a.cpu().numpy(), want, "model L=%d" % L)
    model.train()
    rels = [0, 1, 3]
    ridx = model._rule_ids(rels, dev)
    assert model._lstm_hip(dev) and ridx.numel() == len(rules)
    d_out = np.random.default_rng(9).standard_normal((ridx.numel(), 16)).astype(np.float32)
    model.zero_grad()
    out = model._encode_rules_padded(ridx, dev, rels)
    (out * up(d_out, dev)).sum().backward()
    r_out, d_vocab, wg = lstm_ref.grads(sd["vocab_emb.weight"], layers, tok, R_I, ridx.cpu().numpy(), d_out)
    case = "model train L=%d" % L
    check_out(out.detach().cpu().numpy(), r_out, case)
    p = dict(model.named_parameters())
    check_grad(p["vocab_emb.weight"].grad.cpu().numpy(), d_vocab, case, "d_vocab")
    for l in range(L):
        for name, k in (("weight_ih", 0), ("weight_hh", 1), ("bias_ih", 2), ("bias_hh", 2)):
            check_grad(p["rnn.%s_l%d" % (name, l)].grad.cpu().numpy(), wg[l][k], case,
                       "%s_l%d" % (("dW_ih", "dW_hh", "db")[k], l))


def test_model_four_layers(env, dev):
    """num_layers = 4 (the reference accepts any): no kernel has that shape, the
    model runs torch's LSTM and rnnl_node_weights; embeddings against the
    reference, scores against the numpy restatement of the reference model."""
    spec, path, _ = env
    rules = rules_i()
    model = build_model(env, rules, 4, dev).eval()
    sd, layers = state_of(model, 4)
    a, b = both_forms(model)
    want = lstm_ref.encode(sd["vocab_emb.weight"], layers, model.rule_features.numpy(), R_I)
    check_out(a.cpu().numpy(), want, "model L=4")
    check_out(b.cpu().numpy(), want, "model L=4 per rule")
    h = np.asarray([q[0] for q in spec.queries.values()], dtype=np.int64)
    r = np.zeros_like(h)
    with torch.no_grad():
        score, mask = model(up(h, dev), up(r, dev), None)
    g = ref.Graph(path)
    rr = ref.Rules([[hd] + list(bd) for hd, bd in rules], g.relation_size)
    cfg = dict(type="lstm", aggregator="sum", entity_feature="bias", num_layers=4)
    w_score, w_mask = ref.predictorplus_forward(sd, cfg, g, rr, h, r, None)
    assert np.array_equal(mask.cpu().numpy(), w_mask)
    assert np.abs(w_score - sd["bias"][None]).max() > 1e-2, "no rule reaches a candidate"
    err = float(np.abs(score.cpu().numpy() - w_score).max())
    print("model L=4: max |score - oracle| = %.3g" % err)
    assert err <= 1e-4, err


@pytest.mark.parametrize("L", [1, 3])
def test_model_nine_token_rules(L, env, dev):
    """A body of 8 relations (9 tokens): the trie form encodes it (one launch
    per depth), the per-rule form has no such shape and runs torch's LSTM."""
    rules = rules_i() + [(1, [5, 4, 3, 2, 1, 0, 5, 4])]
    model = build_model(env, rules, L, dev).eval()
    assert model.rule_features.size(1) == 9
    sd, layers = state_of(model, L)
    want = lstm_ref.encode(sd["vocab_emb.weight"], layers, model.rule_features.numpy(), R_I)
    a, b = both_forms(model)
    check_out(a.cpu().numpy(), want, "model 9 tokens L=%d trie" % L)
    check_out(b.cpu().numpy(), want, "model 9 tokens L=%d per rule" % L)
    # the node records of either form are built from those rows
    model.node_weights(dev)
    model.encoder_trie = False
    model.invalidate_cache()
    model.node_weights(dev)


def test_zz_print_figures(dev):
    """The observed maxima per case (the module docstring's table)."""
    cols = ("out", "d_vocab", "dW_ih", "dW_hh", "db")
    for case in sorted(_figures):
        print("%-28s %s" % (case, "  ".join("%s %.2e" % (k, _figures[case][k]) for k in cols if k in _figures[case])))
