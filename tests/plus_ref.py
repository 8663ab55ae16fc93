"""Yardstick of PredictorPlus's rule part in training (rnnlogic_amd/csrc/
backward.hip, pna_grad.hip): torch.float64 on the CPU, the grounding from
oracle/reference_np (dense int64 path counts), no product code and no GPU.

coo():                   the candidates and (candidate, rule, count) entries of
                         a batch of rows of any relations, each row's rules
                         grounded by reference_np.grounding with its own edge
                         removed (data.py:136-173).
sum_forward_backward():  FuncToNodeSum + score_model (layers.py:9-77,
                         predictors.py:238-271) and, by autograd under the
                         upstream gradient G (nq x |E|), every gradient.
pna_stats() / pna_stats_backward():  FuncToNode's statistics (layers.py:89-101)
                         and their backward under the project's tie convention.
pna_forward_backward():  the whole PNA model (FuncToNode.finish's formulas).
margins():               every ReLU input of the candidates with a gradient and
                         its a-priori fp32 rounding bound (admissibility).
small_graph():           the synthetic dataset the CPU and the GPU tests share;
params(): its seeded model parameters; SETS / batch(): the shared input sets.

Every function takes `dtype`: torch.float64 is the reference, torch.float32
the same formulas as an independent fp32 implementation (tests/test_plus_ref.py
measures one against the other: the GPU tests' bounds).

Tie convention.  The reference's dense .min(1) / .max(1)
route a candidate's min / max gradient to one index among the tied ones.  Here:
whole to the smallest trie node among the candidate's entries tied at the
value — nodes are the distinct (head, body) pairs, numbered breadth-first with
children in relation order, i.e. ordered by (head, body length, body) — split
evenly among that node's member rules (the rules listed with that body) tied at
the value.
"""
import os

import numpy as np
import torch

from oracle import reference_np as ref

H = 16
U32 = 64.0 * 2.0 ** -24  # rounding bound of an fp32 dot product of <= 33 terms, per unit of sum |w x| + |b|

# --------------------------------------------------------------------------- the graph
STARS = (1, 23, 24, 25, 63, 64, 65, 129)  # r1 neighbours of head B's star centres
NBODY = 9                                 # body relations 0 .. 8 of head A
REL = dict(A=9, B=10, r1=11, r2=12, C=13, D=14, r4=15)
NREL = 16
CORE = 40                                 # entities of the dense random neighbourhood
CORE_EDGES = 44                           # edges per body relation among them


def small_graph(root, seed=0, stars=STARS):
    """Writes the dataset (entities.dict, relations.dict, train / valid /
    test.txt) and rules.txt under `root`/plus_small<seed> (another `stars`
    tuple: plus_small<seed>_s<its sizes>; the random part is drawn before the
    stars are laid out, so it is the same); no parallel edges.

    A <- every body of length 1..3 over the relations 0..8 (819 rules = trie
            nodes) on 40 core entities with 44 random edges per relation.
    B <- r1 | r1 r2 | r1 (again: one node, two member rules) | B r2 | r2 |
            r1 r2 r2: star centres with 1, 23, ..., 129 r1 leaves, the leaves of
            a star on an r2 cycle, the fact (centre, B, leaf 0): a centre's row
            has exactly its leaves as candidates.
    C    facts on the core, no rule.
    D <- r4 | r4 r4 | D r4 on chains of three: rows with 0 - 3 candidates.
    Returns dict(path, rules, facts={head name: [(h, r, t)]}, n_entities)."""
    rng = np.random.default_rng(100 + seed)
    trip = []

    def pairs(n, lo, hi):
        out = set()
        while len(out) < n:
            a, b = (int(x) for x in rng.integers(lo, hi, 2))
            if a != b:
                out.add((a, b))
        return sorted(out)

    for b in range(NBODY):
        trip += [(h, b, t) for h, t in pairs(CORE_EDGES, 0, CORE)]
    facts = {"A": [(h, REL["A"], t) for h, t in pairs(40, 0, CORE)],
             "C": [(h, REL["C"], t) for h, t in pairs(10, 0, CORE)], "B": [], "D": []}
    n = CORE
    for k in stars:
        centre, leaves = n, list(range(n + 1, n + 1 + k))
        n += 1 + k
        trip += [(centre, REL["r1"], x) for x in leaves]
        if k > 1:
            trip += [(leaves[i], REL["r2"], leaves[(i + 1) % k]) for i in range(k)]
        facts["B"].append((centre, REL["B"], leaves[0]))
    d0 = n
    n += 30
    for i in range(29):
        if i % 3 != 2:
            trip.append((d0 + i, REL["r4"], d0 + i + 1))
        facts["D"].append((d0 + i, REL["D"], d0 + i + 1))
    facts["D"] += [(d0, REL["D"], d0 + 3), (d0 + 6, REL["D"], d0 + 9)]
    for k in ("A", "B", "C", "D"):
        trip += facts[k]
    assert len(set(trip)) == len(trip) and (n <= 512 or tuple(stars) != STARS)
    tag = "" if tuple(stars) == STARS else "_s" + "_".join(map(str, stars))
    d = os.path.join(str(root), "plus_small%d%s" % (seed, tag))
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "entities.dict"), "w") as f:
        f.write("".join("%d\te%d\n" % (i, i) for i in range(n)))
    with open(os.path.join(d, "relations.dict"), "w") as f:
        f.write("".join("%d\tr%d\n" % (i, i) for i in range(NREL)))
    with open(os.path.join(d, "train.txt"), "w") as f:
        f.write("".join("e%d\tr%d\te%d\n" % (h, r, t) for h, r, t in trip))
    for fn in ("valid.txt", "test.txt"):
        with open(os.path.join(d, fn), "w") as f:
            f.write("e%d\tr%d\te%d\n" % facts["A"][0])
    rules = []
    for a in range(NBODY):
        rules.append([REL["A"], a])
    for a in range(NBODY):
        for b in range(NBODY):
            rules.append([REL["A"], a, b])
            for c in range(NBODY):
                rules.append([REL["A"], a, b, c])
    B, D, r1, r2, r4 = REL["B"], REL["D"], REL["r1"], REL["r2"], REL["r4"]
    rules += [[B, r1], [B, r1, r2], [D, r4], [B, r1], [B, B, r2], [D, r4, r4], [B, r2], [B, r1, r2, r2], [D, D, r4]]
    rp = os.path.join(d, "rules.txt")
    with open(rp, "w") as f:
        f.write("".join(" ".join(map(str, r)) + "\n" for r in rules))
    return dict(path=d, rules=rp, facts=facts, n_entities=n)


def node_of_rule(rules):
    """Trie-node rank of every rule: distinct (head, body) in the order (head,
    body length, body) — the order of the breadth-first numbering among the
    rule-bearing nodes."""
    keys = [(hd, len(b), tuple(b)) for hd, b in rules.rules]
    rank = {k: i for i, k in enumerate(sorted(set(keys)))}
    return np.asarray([rank[k] for k in keys], dtype=np.int64)


# --------------------------------------------------------------------------- parameters and input sets
def params(sg, type_, aggregator, seed=0):
    """The state dict (float32 numpy) of PredictorPlus(hidden_dim 16) on the
    small graph: torch's default initial ranges, each perturbed by randn x 0.3."""
    rng = np.random.default_rng(500 + seed)
    n_rules = sum(1 for _ in open(sg["rules"]))

    def lin(out, inp, prefix, sd):
        k = 1.0 / np.sqrt(inp)
        sd[prefix + ".weight"] = rng.uniform(-k, k, (out, inp)) + 0.3 * rng.standard_normal((out, inp))
        sd[prefix + ".bias"] = rng.uniform(-k, k, out) + 0.3 * rng.standard_normal(out)

    sd = {}
    sd["vocab_emb.weight"] = rng.standard_normal((NREL + 1, H))
    sd["vocab_emb.weight"][NREL] = 0
    if type_ == "lstm":
        k = 1.0 / np.sqrt(H)
        for l in range(3):
            for name, shape in (("weight_ih", (4 * H, H)), ("weight_hh", (4 * H, H)), ("bias_ih", (4 * H,)),
                                ("bias_hh", (4 * H,))):
                sd["rnn.%s_l%d" % (name, l)] = rng.uniform(-k, k, shape) + 0.3 * rng.standard_normal(shape)
    else:
        sd["rule_emb"] = rng.uniform(-0.25, 0.25, (n_rules, H)) + 0.3 * rng.standard_normal((n_rules, H))
    lin(H, H if aggregator == "sum" else 12 * H, "rule_to_entity.add_model.layers.0", sd)
    sd["rule_to_entity.layer_norm.weight"] = 1 + 0.3 * rng.standard_normal(H)
    sd["rule_to_entity.layer_norm.bias"] = 0.3 * rng.standard_normal(H)
    sd["relation_emb.weight"] = rng.standard_normal((NREL, H)) + 0.3 * rng.standard_normal((NREL, H))
    lin(128, 2 * H, "score_model.layers.0", sd)
    lin(1, 128, "score_model.layers.1", sd)
    sd["bias"] = 0.3 * rng.standard_normal(sg["n_entities"])
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in sd.items()}


# params()' seed per (type, aggregator): one for which every set below is
# admissible (margins(); tests/test_plus_ref.py checks)
PARAM_SEED = {("emb", "sum"): 0, ("emb", "pna"): 1, ("lstm", "sum"): 6, ("lstm", "pna"): 0}

# name: (heads the rows are drawn from in turn, rows, seed)
SETS = {
    "A1": ("A", 1, 0),
    "A5": ("A", 5, 0),
    "A33": ("A", 33, 0),
    "B1": ("B", 1, 0),
    "B5": ("B", 5, 0),
    "B33": ("B", 33, 0),
    "stars": ("B", 8, 0),       # every star centre once
    "mixed": ("ABCD", 24, 0),   # interleaved, unsorted
    "tile": ("BD", 44, 0),      # tiled 25 times by the GPU test: 1,100 rows
}


def batch(sg, g, name, seed=None):
    """(h, r, t, etr) int64 of set `name`: row k is a fact of head
    heads[k % len(heads)], facts in file order first, then drawn with
    repetition; etr is the fact's index among its relation's train edges."""
    heads, n, s = SETS[name]
    rng = np.random.default_rng(900 + (s if seed is None else seed))
    rows, used = [], {k: 0 for k in heads}
    for k in range(n):
        hd = heads[k % len(heads)]
        f = sg["facts"][hd]
        rows.append(f[used[hd]] if used[hd] < len(f) else f[int(rng.integers(0, len(f)))])
        used[hd] += 1
    return rows_of(g, rows)


def rows_of(g, facts):
    a = np.asarray(facts, dtype=np.int64).reshape(-1, 3)
    etr = np.asarray([g.ht2index[r][t * g.entity_size + h] for h, r, t in a.tolist()], dtype=np.int64)
    return a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy(), etr


def upstream(nq, E, seed, mean=0.5):
    """The upstream gradient G (nq, E) float32: randn + mean (a non-zero mean,
    so that no gradient is a near-cancelling sum)."""
    return (np.random.default_rng(7000 + seed).standard_normal((nq, E)) + mean).astype(np.float32)


# --------------------------------------------------------------------------- the grounding COO
def coo(g, rules, h, r, etr):
    """dict(nq, E, row, ent (C,), ce, rule, count (nnz,)): candidates in
    row-major order (entity ascending), one entry per (candidate, rule) with a
    non-zero path count.  Rows of any relations."""
    h, r = np.asarray(h, dtype=np.int64), np.asarray(r, dtype=np.int64)
    nq, E = len(h), g.entity_size
    ent_rows, rule_rows, cnt_rows, q_rows = [], [], [], []
    for q in np.unique(r):
        sel = np.nonzero(r == q)[0]
        for i, (hd, body) in rules.relation2rules[int(q)]:
            x = ref.grounding(g, h[sel], hd, body, None if etr is None else np.asarray(etr)[sel])
            qq, ee = np.nonzero(x)
            q_rows.append(sel[qq])
            ent_rows.append(ee)
            rule_rows.append(np.full(len(qq), i, dtype=np.int64))
            cnt_rows.append(x[qq, ee])
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, dtype=np.int64)  # noqa: E731
    key = cat(q_rows) * E + cat(ent_rows)
    cand, ce = np.unique(key, return_inverse=True)
    return dict(nq=nq, E=E, row=cand // E, ent=cand % E, ce=ce.astype(np.int64), rule=cat(rule_rows),
                count=cat(cnt_rows).astype(np.int64))


def _t(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype)


def leaves(sd, names, dtype):
    return {n: _t(sd[n], dtype).requires_grad_(True) for n in names}


def lstm_table(p, rules, dtype):
    """encode_rules (predictors.py:201-208) of every rule: torch.nn.LSTM(16,
    16, 3) in `dtype` on the leaves p (vocab_emb.weight, rnn.*)."""
    tok = torch.from_numpy(rules.features)
    x = p["vocab_emb.weight"][tok]
    n, T = tok.shape
    for l in range(3):
        wi, wh = p["rnn.weight_ih_l%d" % l], p["rnn.weight_hh_l%d" % l]
        b = p["rnn.bias_ih_l%d" % l] + p["rnn.bias_hh_l%d" % l]
        hh = torch.zeros((n, H), dtype=dtype)
        c = torch.zeros((n, H), dtype=dtype)
        outs = []
        for t in range(T):
            z = x[:, t] @ wi.t() + hh @ wh.t() + b
            i, f, gg, o = z.split(H, 1)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
            hh = torch.sigmoid(o) * torch.tanh(c)
            outs.append(hh)
        x = torch.stack(outs, 1)
    idx = (tok != NREL).sum(-1) - 1
    return x[torch.arange(n), idx]


LSTM_NAMES = ["vocab_emb.weight"] + ["rnn.%s_l%d" % (n, l) for l in range(3)
                                      for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
DENSE_NAMES = ["rule_to_entity.add_model.layers.0.weight", "rule_to_entity.add_model.layers.0.bias",
               "rule_to_entity.layer_norm.weight", "rule_to_entity.layer_norm.bias", "score_model.layers.0.weight",
               "score_model.layers.0.bias", "score_model.layers.1.weight", "score_model.layers.1.bias",
               "relation_emb.weight"]


def rule_table(sd, rules, dtype):
    """(x (n_rules, 16) with its graph, the leaves it depends on)."""
    if "rule_emb" in sd:
        p = leaves(sd, ["rule_emb"], dtype)
        return p["rule_emb"], p
    p = leaves(sd, LSTM_NAMES, dtype)
    return lstm_table(p, rules, dtype), p


def _layer_norm(y, w, b):
    mu = y.mean(-1, keepdim=True)
    var = ((y - mu) ** 2).mean(-1, keepdim=True)
    xh = (y - mu) / torch.sqrt(var + 1e-5)
    return xh * w + b, xh, torch.sqrt(var + 1e-5)


def _score(p, z, rel_rows):
    """score_model on cat(z, relation_emb[rel]) -> (scores (C,), hidden pre-activations (C, 128))."""
    inp = torch.cat([z, p["relation_emb.weight"][rel_rows]], -1)
    a = inp @ p["score_model.layers.0.weight"].t() + p["score_model.layers.0.bias"]
    out = torch.relu(a) @ p["score_model.layers.1.weight"].t() + p["score_model.layers.1.bias"]
    return out.squeeze(-1), a, inp


def _finish(out, c, G, p, extra, dtype):
    """Gradients of sum(score x G) over the candidates: {name: float64/32 numpy}."""
    Gt = _t(np.asarray(G), dtype)
    gc = Gt[torch.from_numpy(c["row"]), torch.from_numpy(c["ent"])]
    names = list(p) + list(extra)
    ts = [p[n] for n in p] + [extra[n] for n in extra]
    if len(gc):
        gs = torch.autograd.grad((out * gc).sum(), ts, allow_unused=True)
    else:
        gs = [None] * len(ts)
    grads = {n: (g if g is not None else torch.zeros_like(t)).detach().numpy() for n, g, t in zip(names, gs, ts)}
    grads["bias"] = Gt.sum(0).numpy()
    return grads


def sum_forward(sd, c, x, rel_of_row, dtype=torch.float64, p=None):
    p = p if p is not None else leaves(sd, DENSE_NAMES, dtype)
    ce, rule, cnt = (torch.from_numpy(c[k]) for k in ("ce", "rule", "count"))
    C = len(c["ent"])
    feat = torch.zeros((C, H), dtype=dtype).index_add(0, ce, cnt.to(dtype).unsqueeze(-1) * x[rule])
    y = feat @ p["rule_to_entity.add_model.layers.0.weight"].t() + p["rule_to_entity.add_model.layers.0.bias"]
    a_ln, xh, sd_ = _layer_norm(y, p["rule_to_entity.layer_norm.weight"], p["rule_to_entity.layer_norm.bias"])
    rel_rows = torch.from_numpy(np.asarray(rel_of_row, dtype=np.int64)[c["row"]])
    out, a_h, inp = _score(p, torch.relu(a_ln), rel_rows)
    return out, dict(p=p, feat=feat, y=y, a_ln=a_ln, xh=xh, std=sd_, a_h=a_h, inp=inp, x=x, c=c)


def sum_forward_backward(sd, c, rules, rel_of_row, base, G, dtype=torch.float64):
    """FuncToNodeSum + score_model on the COO c under the upstream gradient G
    (nq, E).  base: the bias vector (E,) or None (entity_feature none).
    Returns (scores at the candidates (C,) — with base[ent] added —, the
    gradients {state-dict name: array} of every rule-part parameter and of
    'bias' (G's column sums), and the saved forward for margins())."""
    x, px = rule_table(sd, rules, dtype)
    out, saved = sum_forward(sd, c, x, rel_of_row, dtype)
    grads = _finish(out, c, G, saved["p"], px, dtype)
    score = out.detach().numpy().copy()
    if base is not None:
        score = score + np.asarray(base, dtype=score.dtype)[c["ent"]]
    return score, grads, saved


# --------------------------------------------------------------------------- PNA
def pna_stats(c, x, dtype=torch.float64):
    """FuncToNode's statistics of the rule table x (n_rules, 16) per candidate
    (layers.py:89-101): dict(wsum, wsq, mn, mx (C, 16), deg (C,), row, ent (C,),
    row_scale (nq,): the rows' mean log(deg), 0 for a row without candidates)."""
    x = x if torch.is_tensor(x) else _t(x, dtype)
    ce, rule, cnt = (torch.from_numpy(c[k]) for k in ("ce", "rule", "count"))
    C = len(c["ent"])
    k = cnt.to(dtype).unsqueeze(-1)
    xe = x[rule]
    idx = ce.unsqueeze(-1).expand(-1, H)
    wsum = torch.zeros((C, H), dtype=dtype).index_add(0, ce, k * xe)
    wsq = torch.zeros((C, H), dtype=dtype).index_add(0, ce, k * xe * xe)
    mn = torch.full((C, H), float("inf"), dtype=dtype).scatter_reduce(0, idx, xe.detach(), "amin")
    mx = torch.full((C, H), float("-inf"), dtype=dtype).scatter_reduce(0, idx, xe.detach(), "amax")
    deg = torch.zeros(C, dtype=dtype).index_add(0, ce, cnt.to(dtype)) + 1
    row = torch.from_numpy(c["row"])
    s_sum = torch.zeros(c["nq"], dtype=dtype).index_add(0, row, deg.log())
    s_cnt = torch.zeros(c["nq"], dtype=dtype).index_add(0, row, torch.ones(C, dtype=dtype))
    return dict(wsum=wsum, wsq=wsq, mn=mn, mx=mx, deg=deg, row=c["row"], ent=c["ent"],
                row_scale=s_sum / s_cnt.clamp(min=1))


def pna_stats_backward(c, x, node, g_wsum, g_wsq, g_mn, g_mx, dtype=torch.float64):
    """d_x (n_rules, 16) of pna_stats under the four upstream gradients (C, 16)
    and the tie convention of the module docstring; node = node_of_rule()."""
    x = _t(np.asarray(x), dtype)
    ce, rule, cnt = (torch.from_numpy(c[k]) for k in ("ce", "rule", "count"))
    node = torch.from_numpy(np.asarray(node, dtype=np.int64))[rule]
    g_wsum, g_wsq, g_mn, g_mx = (_t(np.asarray(a), dtype) for a in (g_wsum, g_wsq, g_mn, g_mx))
    C = len(c["ent"])
    k = cnt.to(dtype).unsqueeze(-1)
    xe = x[rule]
    idx = ce.unsqueeze(-1).expand(-1, H)
    d = k * g_wsum[ce] + 2 * xe * k * g_wsq[ce]
    big = torch.iinfo(torch.int64).max
    for red, init, g in (("amin", float("inf"), g_mn), ("amax", float("-inf"), g_mx)):
        v = torch.full((C, H), init, dtype=dtype).scatter_reduce(0, idx, xe, red)
        tied = xe == v[ce]
        cand_node = torch.full((C, H), big, dtype=torch.int64).scatter_reduce(
            0, idx, torch.where(tied, node.unsqueeze(-1).expand(-1, H), torch.full_like(idx, big)), "amin")
        take = tied & (node.unsqueeze(-1) == cand_node[ce])
        n_take = torch.zeros((C, H), dtype=dtype).index_add(0, ce, take.to(dtype))
        d = d + torch.where(take, g[ce] / n_take[ce].clamp(min=1), torch.zeros_like(xe))
    return torch.zeros_like(x).index_add(0, rule, d).numpy()


def pna_finish(p, st, rel_rows, dtype):
    """FuncToNode.finish (layers.py:102-126) + score_model from the statistics."""
    eps = 1e-6
    deg = st["deg"].unsqueeze(-1)
    mean = st["wsum"] / deg.clamp(min=eps)
    sq_mean = st["wsq"] / deg.clamp(min=eps)
    var = sq_mean - mean * mean
    std = var.clamp(min=eps).sqrt()
    feats = torch.cat([mean, st["mn"], st["mx"], std], -1)
    s = deg.log() / st["row_scale"][torch.from_numpy(st["row"])].unsqueeze(-1).clamp(min=eps)
    scales = torch.cat([torch.ones_like(s), s, 1 / s.clamp(min=eps)], -1)
    upd = (feats.unsqueeze(-1) * scales.unsqueeze(-2)).flatten(-2)
    y = upd @ p["rule_to_entity.add_model.layers.0.weight"].t() + p["rule_to_entity.add_model.layers.0.bias"]
    a_ln, xh, sd_ = _layer_norm(y, p["rule_to_entity.layer_norm.weight"], p["rule_to_entity.layer_norm.bias"])
    out, a_h, inp = _score(p, torch.relu(a_ln), rel_rows)
    return out, dict(p=p, feat=upd, y=y, a_ln=a_ln, xh=xh, std=sd_, a_h=a_h, inp=inp,
                     var=var, var_m=U32 * (sq_mean + mean * mean))


def pna_forward_backward(sd, c, rules, rel_of_row, base, G, dtype=torch.float64):
    """The whole PNA model; returns as sum_forward_backward.  The statistics'
    backward is pna_stats_backward (the tie convention), the rest autograd."""
    x, px = rule_table(sd, rules, dtype)
    st = pna_stats(c, x.detach(), dtype)
    for k in ("wsum", "wsq", "mn", "mx"):
        st[k] = st[k].detach().requires_grad_(True)
    p = leaves(sd, DENSE_NAMES, dtype)
    rel_rows = torch.from_numpy(np.asarray(rel_of_row, dtype=np.int64)[c["row"]])
    out, saved = pna_finish(p, st, rel_rows, dtype)
    stat_leaves = {"stat." + k: st[k] for k in ("wsum", "wsq", "mn", "mx")}
    grads = _finish(out, c, G, p, stat_leaves, dtype)
    gs = [grads.pop("stat." + k) for k in ("wsum", "wsq", "mn", "mx")]
    d_x = pna_stats_backward(c, x.detach().numpy(), node_of_rule(rules), *gs, dtype=dtype)
    names = list(px)
    if len(c["ent"]):
        gx = torch.autograd.grad(x, [px[n] for n in names], grad_outputs=_t(d_x, dtype), allow_unused=True) \
            if names != ["rule_emb"] else [_t(d_x, dtype)]
    else:
        gx = [None] * len(names)
    for n, gr in zip(names, gx):
        grads[n] = (gr if gr is not None else torch.zeros_like(px[n])).detach().numpy()
    score = out.detach().numpy().copy()
    if base is not None:
        score = score + np.asarray(base, dtype=score.dtype)[c["ent"]]
    saved["c"], saved["x"] = c, x
    return score, grads, saved


# --------------------------------------------------------------------------- admissibility
def margins(saved, G):
    """Every ReLU input of the candidates with a non-zero upstream gradient:
    (a, m) flat float64 arrays — the pre-activation and the a-priori bound of
    its fp32 evaluation, m = 64 x 2^-24 x (sum |w_i x_i| + |b|):

      LayerNorm out d  a = w_d xh_d + b_d (one term and the bias);
      hidden unit o    a = W0[o] . [z, rel] + b0[o] (32 terms and the bias);
      PNA's std clamp  a = var - 1e-6 with var = E[x^2] - mean^2: the two terms
                       (`var`, `var_m` saved by pna_finish).

    A set is admissible iff every |a| > m."""
    c, p = saved["c"], saved["p"]
    on = torch.from_numpy(np.asarray(G)[c["row"], c["ent"]] != 0)
    det = lambda t: t.detach().to(torch.float64)  # noqa: E731
    lnw, lnb = det(p["rule_to_entity.layer_norm.weight"]), det(p["rule_to_entity.layer_norm.bias"])
    m_ln = U32 * ((lnw * det(saved["xh"])).abs() + lnb.abs())
    W0 = det(p["score_model.layers.0.weight"])
    m_h = U32 * (det(saved["inp"]).abs() @ W0.abs().t() + det(p["score_model.layers.0.bias"]).abs())
    a = [det(saved["a_ln"])[on].reshape(-1), det(saved["a_h"])[on].reshape(-1)]
    m = [m_ln[on].reshape(-1), m_h[on].reshape(-1)]
    if "var" in saved:
        a.append((det(saved["var"]) - 1e-6)[on].reshape(-1))
        m.append(det(saved["var_m"])[on].reshape(-1))
    return torch.cat(a).numpy(), torch.cat(m).numpy()


def rel_err(got, want):
    """max |got - want| / max |want| over the entries where want is finite (0 / 0 = 0)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    ok = np.isfinite(want)
    if not ok.any():
        return 0.0
    scale = float(np.abs(want[ok]).max())
    err = float(np.abs(got[ok] - want[ok]).max())
    return err / scale if scale > 0 else err


def score_split_bound(saved):
    """A-priori bound (C,) of what the eval scorer's first layer leaves out of
    a score.  It multiplies W0[:, :16] and z as two fp16 parts each (v = hi +
    lo + r, |r| <= 2^-22 |v|) and drops lo x lo (<= 2^-22 |w z|): each of the
    16 products of an active hidden unit o is off by at most 3 x 2^-22 |w z|,
    which reaches the score times |W1[o]|."""
    p = saved["p"]
    det = lambda t: t.detach().to(torch.float64)  # noqa: E731
    z = det(saved["inp"])[:, :H]
    per_unit = z @ det(p["score_model.layers.0.weight"])[:, :H].abs().t()  # z >= 0
    active = (det(saved["a_h"]) > 0).to(torch.float64)
    return (3 * 2.0 ** -22 * (per_unit * active) @ det(p["score_model.layers.1.weight"]).abs().t()).squeeze(-1).numpy()
