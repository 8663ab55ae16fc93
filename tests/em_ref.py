"""Yardstick of the EM loop's training step (rnnlogic_amd/csrc/predictor.hip,
loss.hip, batch.hip): numpy / torch.float64 on the CPU oracle's grounding
(plus_ref.coo, which grounds each rule with oracle/reference_np.grounding), no
product code and no GPU.

graph():       plus_ref.small_graph with a ninth star of 300 leaves: one row
               with 300 candidates (5 chunks of 64, more than one 256-thread
               pass, an hr2o list longer than a workgroup), |E| = 773.
wide_rules():  a second rules file for the same graph whose head A has the
               first n bodies in (length, lexicographic) order over the
               relations 0..8, lengths up to 5: n rule-bearing trie nodes.
weights() / bias():  the seeded float32 parameters of every case.
scores() / rule_grads() / rule_stats() / H() / nll() / step() / ranks():
               the formulas of the reference's Predictor.forward, its
               gradient, compute_H (src/predictors.py:53-119), the training
               loss (src/trainer.py:84-90) and the filtered ranks
               (src/trainer.py:191-203).
table_shift() / score_bound() / rule_grad_bound() / bias_grad_bound():
               the a-priori bounds of the kernels' stated arithmetic, computed
               in float64 from the reference's own quantities.

Every formula takes `dtype`: torch.float64 is the reference, torch.float32 the
same formulas as an independent fp32 implementation (tests/test_em_ref.py
measures one against the other: the GPU tests' bounds of H, the loss, its
gradient and the chained step).

The a-priori bounds (each times ROUND = 1.01 for its own rounding):

* Score at a candidate.  lin_node_kernel sums a node's rule weights in fp64
  and rounds to fp32 (2^-24 |nw|); lin_fix_kernel rounds that to the table's
  grid 2^-shift (half a step), shift = min(30 - e, 60) with frexp(max
  |float32(nw)|) = (., e), 30 for an all-zero table; score_linear_kernel sums
  count x fix exactly and rounds once to fp32, and once more when the bias is
  added:  sum_e count_e (|nw_e| 2^-24 + 2^-(shift+1)) + 2^-24 |S|
  (+ 2^-24 |S + b|).
* Rule gradient.  predictor_backward_kernel rounds each candidate's gradient
  to the grid 2^-sc, sc = 61 - floor(log2(K max |G|)), K the sum of the
  counts at candidates with G != 0, multiplies by the integer count and sums
  exactly; the result is rounded to fp32:  half_ulp32(g64) + k_node 2^-(sc+1)
  with k_node the node's share of K.  half_ulp32(g) is 2^-24 |g|, and 2^-150
  below the smallest normal fp32 (half the spacing of the denormals: what
  fp32 can hold of a gradient under an upstream gradient x 2^-130).
* Bias gradient.  A sum of nq fp32 terms per entity in any order:
  (nq - 1) 2^-24 sum_q |G[q, e]|.
"""
import itertools
import os

import numpy as np
import torch

import plus_ref as pr
from oracle import reference_np as ref

STARS = pr.STARS + (300,)
ROUND = 1.01
WIDE_LEN = 5


def graph(root):
    return pr.small_graph(root, 0, stars=STARS)


def wide_bodies(n):
    """The first n bodies in (length, lexicographic) order over the relations 0 .. NBODY-1."""
    out = []
    for length in range(1, WIDE_LEN + 1):
        for body in itertools.product(range(pr.NBODY), repeat=length):
            if len(out) == n:
                return out
            out.append(list(body))
    assert len(out) == n, "no more than %d bodies of length <= %d" % (len(out), WIDE_LEN)
    return out


def wide_rules(sg, n):
    """Writes rules_wide<n>.txt beside the graph's rules.txt: head A <- the
    first n bodies of wide_bodies, heads B and D as in rules.txt.  Returns its path."""
    with open(sg["rules"]) as f:
        old = [[int(x) for x in line.split()] for line in f]
    rules = [[pr.REL["A"]] + b for b in wide_bodies(n)] + [r for r in old if r[0] != pr.REL["A"]]
    path = os.path.join(sg["path"], "rules_wide%d.txt" % n)
    with open(path, "w") as f:
        f.write("".join(" ".join(map(str, r)) + "\n" for r in rules))
    return path


# --------------------------------------------------------------------------- parameters
KINDS = ("normal", "zero", "tiny", "skew", "cancel")


def weights(rules, kind, seed=0):
    """rule_weights (n_rules,) float32 of `rules` (reference_np.Rules)."""
    n = len(rules.rules)
    w = (0.5 * np.random.default_rng(300 + seed).standard_normal(n)).astype(np.float32)
    if kind == "zero":
        w[:] = 0
    elif kind == "tiny":
        w = (w.astype(np.float64) * 2.0 ** -40).astype(np.float32)
    elif kind == "skew":
        A = [i for i, (hd, _) in enumerate(rules.rules) if hd == pr.REL["A"]]
        w[A] *= np.float32(2.0 ** 12)
    elif kind == "cancel":
        dup = [i for i, (hd, b) in enumerate(rules.rules) if hd == pr.REL["B"] and b == [pr.REL["r1"]]]
        assert len(dup) == 2
        w[dup[0]], w[dup[1]] = np.float32(1.5), np.float32(-1.5 + 2.0 ** -20)
    else:
        assert kind == "normal", kind
    return w


def bias(n_entities, seed=0):
    return (0.3 * np.random.default_rng(400 + seed).standard_normal(n_entities)).astype(np.float32)


def tile_coo(c, times):
    """The COO of c's rows repeated `times` times (row k x nq + q is row q), by offsetting."""
    C, nq = len(c["ent"]), c["nq"]
    rep = lambda a, step: (np.tile(a, times) + np.repeat(np.arange(times, dtype=np.int64) * step, len(a)))  # noqa: E731
    return dict(nq=nq * times, E=c["E"], row=rep(c["row"], nq), ent=np.tile(c["ent"], times), ce=rep(c["ce"], C),
                rule=np.tile(c["rule"], times), count=np.tile(c["count"], times))


def select_rows(c, rows):
    """The COO of the rows `rows` (ascending) of c, renumbered."""
    rows = np.asarray(rows, dtype=np.int64)
    new_row = np.full(c["nq"], -1, dtype=np.int64)
    new_row[rows] = np.arange(len(rows))
    keep_c = new_row[c["row"]] >= 0
    new_c = np.cumsum(keep_c) - 1
    keep_e = keep_c[c["ce"]]
    return dict(nq=len(rows), E=c["E"], row=new_row[c["row"][keep_c]], ent=c["ent"][keep_c],
                ce=new_c[c["ce"][keep_e]], rule=c["rule"][keep_e], count=c["count"][keep_e])


def node_entries(c, node):
    """One entry per (candidate, trie node): (ce, node, count) — the member
    rules of a node share its count, so the first member's entries stand for it."""
    node = np.asarray(node, dtype=np.int64)
    first = np.full(int(node.max()) + 1, len(node), dtype=np.int64)
    np.minimum.at(first, node, np.arange(len(node)))
    keep = first[node[c["rule"]]] == c["rule"]
    return c["ce"][keep], node[c["rule"][keep]], c["count"][keep]


def _t(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype)


# --------------------------------------------------------------------------- Predictor.forward and its gradient
def scores(c, w, b=None, dtype=torch.float64):
    """(C,) score at every candidate: sum over its entries of count x w[rule] (+ b[ent])."""
    ce, rule, cnt = (torch.from_numpy(c[k]) for k in ("ce", "rule", "count"))
    s = torch.zeros(len(c["ent"]), dtype=dtype).index_add(0, ce, cnt.to(dtype) * _t(w, dtype)[rule])
    if b is not None:
        s = s + _t(b, dtype)[torch.from_numpy(c["ent"])]
    return s.numpy()


def rule_grads(c, G, n_rules, dtype=torch.float64):
    """(d rule_weights (n_rules,), d bias (E,)) under the upstream gradient G
    (nq, E): per rule sum of count x G[row, ent] over its entries; G.sum(0)."""
    Gt = _t(np.asarray(G), dtype)
    ce, rule, cnt = (torch.from_numpy(c[k]) for k in ("ce", "rule", "count"))
    g_e = Gt[torch.from_numpy(c["row"]), torch.from_numpy(c["ent"])][ce]
    gw = torch.zeros(n_rules, dtype=dtype).index_add(0, rule, cnt.to(dtype) * g_e)
    return gw.numpy(), Gt.sum(0).numpy()


# --------------------------------------------------------------------------- compute_H
def rule_stats(c, n_rules, t):
    """(pos, tot (nq, n_rules) int64, n_cand (nq,) int64): per (row, rule) the
    path count at the row's true tail and the sum over the row's candidates."""
    nq = c["nq"]
    pos = np.zeros((nq, n_rules), dtype=np.int64)
    tot = np.zeros((nq, n_rules), dtype=np.int64)
    rr = c["row"][c["ce"]]
    np.add.at(tot, (rr, c["rule"]), c["count"])
    at_t = c["ent"][c["ce"]] == np.asarray(t, dtype=np.int64)[rr]
    np.add.at(pos, (rr[at_t], c["rule"][at_t]), c["count"][at_t])
    return pos, tot, np.bincount(c["row"], minlength=nq).astype(np.int64)


def H(c, w, rules, r, t, dtype=torch.float64):
    """(n_rules,) sum over the rows of predictors.py:82-119's per-row softmax
    over the rules of the row's relation of w x pos - w x tot / max(n_cand, 1)
    (uniform for a row without candidates); a relation without rules adds
    nothing.  None when no row's relation has a rule (the reference's (None,
    None))."""
    r = np.asarray(r, dtype=np.int64)
    n_rules = len(rules.rules)
    pos, tot, ncand = rule_stats(c, n_rules, t)
    out = torch.zeros(n_rules, dtype=dtype)
    any_rule = False
    wt = _t(w, dtype)
    for q in np.unique(r):
        idx = np.asarray([i for i, _ in rules.relation2rules[int(q)]], dtype=np.int64)
        if not len(idx):
            continue
        any_rule = True
        sel = np.nonzero(r == q)[0]
        wq = wt[torch.from_numpy(idx)]
        p = _t(pos[np.ix_(sel, idx)], dtype) * wq
        n = _t(tot[np.ix_(sel, idx)], dtype) * wq / _t(np.maximum(ncand[sel], 1), dtype).unsqueeze(1)
        out[torch.from_numpy(idx)] += torch.softmax(p - n, dim=-1).sum(0)
    return out.numpy() if any_rule else None


# --------------------------------------------------------------------------- the loss
def smoothed_target(target, all_t, smoothing, dtype):
    tt = _t(np.asarray(target), dtype)
    one = torch.zeros_like(tt).scatter_(1, torch.from_numpy(np.asarray(all_t, dtype=np.int64)).view(-1, 1), 1.0)
    return tt * smoothing + one * (1 - smoothing)


def _nll(logits, tt):
    lp = (torch.softmax(logits, dim=1) + 1e-8).log()
    return -(lp * tt).sum() / torch.clamp(tt.sum(), min=1)


def nll(logits, target, all_t, smoothing, c=1.0, dtype=torch.float64):
    """trainer.py:84-90 with an all-True mask -> (loss, d (loss x c) / d logits (B, E))."""
    x = _t(np.asarray(logits), dtype).requires_grad_(True)
    loss = _nll(x, smoothed_target(target, all_t, smoothing, dtype))
    (loss * c).backward()
    return loss.item(), x.grad.numpy()


def step(c, w, b, target, all_t, smoothing, dtype=torch.float64):
    """scores -> loss -> (loss, d rule_weights, d bias): the chain of
    TrainerPredictor.train_step for the bias feature (every entity scored)."""
    wt, bt = _t(w, dtype).requires_grad_(True), _t(b, dtype).requires_grad_(True)
    ce, rule, cnt = (torch.from_numpy(c[k]) for k in ("ce", "rule", "count"))
    val = torch.zeros(len(c["ent"]), dtype=dtype).index_add(0, ce, cnt.to(dtype) * wt[rule])
    flat = torch.from_numpy(c["row"] * c["E"] + c["ent"])
    score = torch.zeros(c["nq"] * c["E"], dtype=dtype).scatter(0, flat, val).view(c["nq"], c["E"]) + bt.unsqueeze(0)
    loss = _nll(score, smoothed_target(target, all_t, smoothing, dtype))
    loss.backward()
    return loss.item(), wt.grad.numpy(), bt.grad.numpy()


# --------------------------------------------------------------------------- filtered ranks
def ranks(score, mask, flag, all_t):
    """(L, H) int64 per row, trainer.py:191-203: L = #(flagged scores > s_t) +
    1, H = #(flagged scores >= s_t) + 2; (1, |E| + 1) where mask[k, t] is False."""
    score, mask, flag = np.asarray(score), np.asarray(mask, dtype=bool), np.asarray(flag, dtype=bool)
    t = np.asarray(all_t, dtype=np.int64)
    rows = np.arange(len(t))
    val = score[rows, t][:, None]
    with np.errstate(invalid="ignore"):
        L = ((score > val) & flag).sum(1) + 1
        Hh = ((score >= val) & flag).sum(1) + 2
    hit = mask[rows, t]
    return np.where(hit, L, 1).astype(np.int64), np.where(hit, Hh, score.shape[1] + 1).astype(np.int64)


# --------------------------------------------------------------------------- a-priori bounds
def node_sums(w, node):
    """float64 sum of the member rules' float32 weights per node rank."""
    node = np.asarray(node, dtype=np.int64)
    nw = np.zeros(int(node.max()) + 1, dtype=np.float64)
    np.add.at(nw, node, np.asarray(w, dtype=np.float64))
    return nw


def table_shift(w, node):
    """The fixed-point shift of the whole node table: min(30 - e, 60) with
    frexp(max |float32(nw)|) = (., e); 30 for an all-zero table."""
    m = float(np.abs(node_sums(w, node).astype(np.float32)).max())
    return 30 if m == 0 else min(30 - int(np.frexp(m)[1]), 60)


def score_bound(c, w, b, node):
    """(C,) bound of |kernel score - scores(float64)| at every candidate."""
    nw = node_sums(w, node)
    shift = table_shift(w, node)
    ce, nd, cnt = node_entries(c, node)
    per = np.zeros(len(c["ent"]), dtype=np.float64)
    np.add.at(per, ce, cnt * (np.abs(nw[nd]) * 2.0 ** -24 + 2.0 ** -(shift + 1)))
    S = scores(c, w, None)
    per += 2.0 ** -24 * np.abs(S)
    if b is not None:
        per += 2.0 ** -24 * np.abs(S + np.asarray(b, dtype=np.float64)[c["ent"]])
    return ROUND * per


def half_ulp32(x):
    """What rounding x to fp32 may lose: 2^-24 |x|, 2^-150 in the denormal range."""
    return np.maximum(2.0 ** -24 * np.abs(np.asarray(x, dtype=np.float64)), 2.0 ** -150)


def backward_scale(c, G, node):
    """(sc, k_node (n_nodes,)): the launch's fixed-point scale and each node's sum of counts, over the
    candidates whose upstream gradient is finite and not 0; sc = None where there is none."""
    g = np.asarray(G, dtype=np.float64)[c["row"], c["ent"]]
    ce, nd, cnt = node_entries(c, node)
    on = (g != 0) & np.isfinite(g)
    k_node = np.zeros(int(np.asarray(node).max()) + 1, dtype=np.float64)
    np.add.at(k_node, nd[on[ce]], cnt[on[ce]].astype(np.float64))
    K = k_node.sum()
    if not K > 0:
        return None, k_node
    return 61 - int(np.floor(np.log2(K * np.abs(g[on]).max()))), k_node


def rule_grad_bound(c, G, node, g64):
    """(n_rules,) bound of |kernel d rule_weights - g64|."""
    sc, k_node = backward_scale(c, G, node)
    fix = 0.0 if sc is None else k_node[np.asarray(node, dtype=np.int64)] * 2.0 ** -(sc + 1)
    return ROUND * (half_ulp32(g64) + fix)


def bias_grad_bound(G):
    G = np.asarray(G, dtype=np.float64)
    return ROUND * (len(G) - 1) * 2.0 ** -24 * np.abs(G).sum(0)
