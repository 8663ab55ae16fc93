"""Yardstick of the LSTM rule encoder (rnnlogic_amd/csrc/encode.hip): plain
numpy, float64 throughout, no torch and no GPU.

encode():  PredictorPlus.encode_rules for type 'lstm' — torch.nn.LSTM(16, 16,
           L) over the padded token rows, the top layer's h at each row's last
           non-pad position (gate order i, f, g, o; bias b_ih + b_hh).
grads():   its backward through time for the rows tokens[ridx] and an upstream
           gradient d_out: the vocab rows' gradient and every layer's dW_ih,
           dW_hh and db (= d b_ih = d b_hh).  Pad steps contribute nothing.
case():    the seeded input sets (SETS) the CPU and the GPU tests share, with
           ridx_for() and token_csr() for the training runs.

vocab (V + 1, H) with row `pad` the padding row; layers: a list of
(w_ih (4H, H), w_hh (4H, H), b_ih (4H), b_hh (4H)); tokens (n, T) integers
padded with `pad` after each row's tokens.  Independent of
oracle/reference_np.lstm_encode (float32, forward only).
"""
import numpy as np


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _f64(layers):
    return [tuple(np.asarray(p, dtype=np.float64) for p in layer) for layer in layers]


def _forward(vocab, layers, tokens, pad):
    """out (n, H), per-layer saved steps, lengths."""
    vocab = np.asarray(vocab, dtype=np.float64)
    tokens = np.asarray(tokens, dtype=np.int64)
    n, T = tokens.shape
    H = vocab.shape[1]
    live = tokens != pad
    length = live.sum(1)
    assert (length >= 1).all() and (live == (np.arange(T)[None] < length[:, None])).all(), "pads follow the tokens"
    x = vocab[tokens]  # (n, T, H); pad steps are computed and never read
    saved = []
    for w_ih, w_hh, b_ih, b_hh in _f64(layers):
        b = b_ih + b_hh
        h = np.zeros((n, H))
        c = np.zeros((n, H))
        steps, outs = [], []
        for t in range(T):
            z = x[:, t] @ w_ih.T + h @ w_hh.T + b
            i, f, g, o = _sigmoid(z[:, :H]), _sigmoid(z[:, H:2 * H]), np.tanh(z[:, 2 * H:3 * H]), _sigmoid(z[:, 3 * H:])
            c_new = f * c + i * g
            h_new = o * np.tanh(c_new)
            steps.append((x[:, t], h, c, i, f, g, o, c_new))
            h, c = h_new, c_new
            outs.append(h)
        saved.append(steps)
        x = np.stack(outs, 1)
    return x[np.arange(n), length - 1], saved, length


def encode(vocab, layers, tokens, pad):
    """(n, H): the top layer's h at each row's last non-pad position."""
    return _forward(vocab, layers, tokens, pad)[0]


def grads(vocab, layers, tokens, pad, ridx, d_out):
    """(out (m, H), d_vocab (V + 1, H), [(dW_ih, dW_hh, db) per layer]) for
    the rows tokens[ridx] (m = len(ridx), repetition allowed) and the
    upstream gradient d_out (m, H)."""
    vocab = np.asarray(vocab, dtype=np.float64)
    tok = np.asarray(tokens, dtype=np.int64)[np.asarray(ridx, dtype=np.int64)]
    d_out = np.asarray(d_out, dtype=np.float64)
    out, saved, length = _forward(vocab, layers, tok, pad)
    m, T = tok.shape
    H = vocab.shape[1]
    # dL/d(the current layer's output h_t): the gather puts d_out at t = len - 1
    dseq = np.zeros((m, T, H))
    dseq[np.arange(m), length - 1] = d_out
    wgrads = [None] * len(layers)
    for l in range(len(layers) - 1, -1, -1):
        w_ih, w_hh = _f64(layers)[l][:2]
        dW_ih, dW_hh, db = np.zeros_like(w_ih), np.zeros_like(w_hh), np.zeros(4 * H)
        dh_next = np.zeros((m, H))
        dc_next = np.zeros((m, H))
        dx_all = np.zeros((m, T, H))
        for t in range(T - 1, -1, -1):
            x, h_prev, c_prev, i, f, g, o, c = saved[l][t]
            on = (t < length)[:, None]  # a pad step has no gradient and passes none on
            dh = np.where(on, dseq[:, t] + dh_next, 0.0)
            tc = np.tanh(c)
            dc = np.where(on, dh * o * (1.0 - tc * tc) + dc_next, 0.0)
            dz = np.concatenate([dc * g * i * (1.0 - i), dc * c_prev * f * (1.0 - f), dc * i * (1.0 - g * g),
                                 dh * tc * o * (1.0 - o)], axis=1)
            dW_ih += dz.T @ x
            dW_hh += dz.T @ h_prev
            db += dz.sum(0)
            dx_all[:, t] = dz @ w_ih
            dh_next = dz @ w_hh
            dc_next = dc * f
        wgrads[l] = (dW_ih, dW_hh, db)
        dseq = dx_all
    d_vocab = np.zeros_like(vocab)
    live = tok != pad
    np.add.at(d_vocab, tok[live], dseq[live])
    return out, d_vocab, wgrads


# --------------------------------------------------------------------------- shared input sets
# name: (layers L, seq_len T, token-table rows n, vocabulary V, weight scale)
SETS = {
    "a": (1, 1, 1, 5, 1.0),        # smallest possible launch
    "b": (1, 8, 17, 7, 1.0),       # full-length rows; 16 + 1 rules; 136 = 128 + 8 gradient rows
    "c": (2, 5, 129, 24, 1.0),     # two layers; 645 gradient rows (ragged last segment)
    "d": (3, 8, 2000, 93, 1.0),    # the kernels' maximum shape
    "e": (3, 8, 2000, 93, 3.0),    # set d with the weights x 3 (saturated gates)
    "f": (2, 3, 16391, 475, 1.0),  # second grid-stride pass, 7 valid rules in its first row group
    "g15": (3, 6, 15, 24, 1.0),    # the miner's five-relation bodies; one short of a row group
    "g16": (3, 6, 16, 24, 1.0),    # ... and exactly one row group
}


def weights(L, H=16, scale=1.0, seed=0):
    """[(w_ih, w_hh, b_ih, b_hh)] float32, U(-1/sqrt(H), 1/sqrt(H)) x scale (torch's init)."""
    rng = np.random.default_rng(1000 + seed)
    k = scale / np.sqrt(H)
    shapes = ((4 * H, H), (4 * H, H), (4 * H,), (4 * H,))
    return [tuple(rng.uniform(-k, k, shape).astype(np.float32) for shape in shapes) for _ in range(L)]


def token_table(T, n, V, seed=0):
    """(n, T) int32 rows padded with V over the tokens 0 .. V - 2 (token V - 1
    is in no row): rows 0 .. T - 1 have lengths 1 .. T (the last has no pad);
    row 1 repeats one token in every position; the last row repeats the one
    before it (n >= 4); the others have random lengths and tokens."""
    rng = np.random.default_rng(2000 + seed)
    used = max(V - 1, 1)
    length = rng.integers(1, T + 1, n)
    length[:min(T, n)] = np.arange(1, T + 1)[:n]
    tok = rng.integers(0, used, (n, T))
    if n > 1:
        tok[1] = tok[1, 0]
    if n >= 4:
        tok[n - 1], length[n - 1] = tok[n - 2], length[n - 2]
    tok[np.arange(T)[None] >= length[:, None]] = V
    return tok.astype(np.int32)


def case(name, extra=0, seed=0):
    """dict(L, T, n, V, pad, vocab (V + 1, 16) float32 with a zero pad row,
    layers, tokens) of input set `name`; the token table has n + extra rows."""
    L, T, n, V, scale = SETS[name]
    rng = np.random.default_rng(3000 + seed)
    vocab = rng.standard_normal((V + 1, 16)).astype(np.float32)
    vocab[V] = 0
    return dict(name=name, L=L, T=T, n=n, V=V, pad=V, vocab=vocab, layers=weights(L, 16, scale, seed),
                tokens=token_table(T, n + extra, V, seed))


def ridx_for(c, seed=0):
    """n int64 row ids into case c's token table, drawn with repetition; the
    first min(T, n) are rows 0 .. T - 1 (every length), and row 0 is drawn
    twice when n > T."""
    rng = np.random.default_rng(4000 + seed)
    m, rows = c["n"], len(c["tokens"])
    r = rng.integers(0, rows, m)
    k = min(c["T"], m)
    r[:k] = np.arange(k)
    if m > k:
        r[k] = 0
    return r.astype(np.int64)


def token_csr(tok, pad):
    """(tok_id, ptr, pos) int32 of the non-pad tokens of the rows `tok`
    (m, T): positions row T + t grouped by token id, in position order — the
    lists PredictorPlus._token_csr hands rnnl_lstm_train_backward."""
    flat = np.asarray(tok).reshape(-1)
    pos = np.nonzero(flat != pad)[0]
    pos = pos[np.argsort(flat[pos], kind="stable")]
    tok_id, counts = np.unique(flat[pos], return_counts=True)
    ptr = np.concatenate([[0], np.cumsum(counts)])
    return tok_id.astype(np.int32), ptr.astype(np.int32), pos.astype(np.int32)
