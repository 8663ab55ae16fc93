"""tests/plus_ref.py (torch.float64 on the CPU grounding) checked, and the
bounds of tests/test_gpu_plus_grad.py measured.

* Forward: plus_ref's scores equal oracle/reference_np.predictorplus_forward
  (fp32 numpy) on the small graph, sum and pna, emb and lstm, within that
  oracle's own 1e-4.
* The tie convention of pna_stats_backward: without ties it is float64
  autograd of the dense .min(1) / .max(1) formulation (1e-12); with planted
  ties the per-dimension sum over the rules is autograd's, and the routing is
  the hand-computed one of a three-rule example.
* Every input set of plus_ref.SETS is admissible for every model variant
  (plus_ref.margins: no ReLU input, and no std clamp, within its a-priori fp32
  rounding bound of the kink).
* measure(): the same formulas in float32 on the CPU against float64, per
  input and per tensor: e32 = max |fp32 - f64| / max |f64| (scores: max
  |fp32 - f64|).  The GPU tests' bounds are 16 x e32 — the kernels sum in
  another order, round node records once to their fixed-point grid, and the
  eval scorer's first layer drops the lo x lo fp16 part of each product — a
  gradient tensor's never below 2^-20 max |f64|, a score's never above 1e-4.
  The SUM scores' bound adds plus_ref.score_split_bound, the a-priori size of
  the dropped lo x lo part (3 x 2^-22 per product of an active hidden unit,
  about 2e-5 of a score here): 16 x e32 alone is a sample of the float32
  rounding only, 8e-7 on the one-candidate set B1, where the scorer's 1.0e-6
  is that truncation.
  E32 keeps what was measured; test_gpu_plus_grad.py imports measure().

Recorded e32 (torch 2.x CPU, upstream gradient randn + 0.5, entity feature
bias; `rule`: rule_emb, or the worst of vocab_emb and the LSTM's tensors):

    set    variant   score   rule    add_w   add_b   ln_w    ln_b    s0_w    s0_b    s1_w    s1_b    rel
    A1     emb/sum   9.0e-07 2.4e-07 2.1e-07 7.7e-08 1.3e-07 9.0e-08 2.0e-07 7.9e-08 1.5e-07 7.9e-08 2.4e-07
    A1     emb/pna   1.8e-06 1.8e-07 4.3e-07 2.2e-07 2.3e-07 1.4e-07 1.4e-07 1.1e-07 9.5e-08 7.9e-08 9.8e-08
    A1     lstm/sum  7.5e-07 4.3e-07 2.0e-07 2.4e-07 8.5e-08 7.6e-08 2.4e-07 9.8e-08 2.3e-07 7.9e-08 2.0e-07
    A1     lstm/pna  4.2e-06 4.2e-07 5.5e-07 1.2e-07 1.1e-07 1.2e-07 1.8e-07 1.3e-07 2.8e-07 7.9e-08 1.7e-07
    A33    emb/sum   2.3e-06 3.6e-07 2.0e-07 5.5e-08 2.3e-08 4.7e-08 1.3e-07 7.7e-08 1.4e-07 1.8e-07 8.3e-07
    A33    emb/pna   2.5e-06 2.8e-07 3.6e-07 8.8e-08 1.0e-07 3.0e-08 3.2e-07 8.8e-08 1.5e-07 1.8e-07 8.5e-07
    A33    lstm/sum  1.3e-06 8.7e-07 3.6e-07 6.1e-08 4.2e-08 7.3e-08 3.0e-07 8.8e-08 1.7e-07 1.8e-07 7.6e-07
    A33    lstm/pna  4.3e-06 5.8e-07 3.6e-07 9.0e-08 6.3e-08 9.8e-08 2.2e-07 5.8e-08 1.4e-07 1.8e-07 4.6e-07
    A5     emb/sum   2.0e-06 1.7e-07 3.2e-07 3.7e-08 6.2e-08 7.3e-08 3.6e-07 1.3e-07 2.5e-07 4.1e-08 1.6e-07
    A5     emb/pna   2.1e-06 1.8e-07 5.0e-07 1.6e-07 1.6e-07 1.1e-07 3.2e-07 7.4e-08 3.3e-07 4.1e-08 2.5e-07
    A5     lstm/sum  9.0e-07 8.5e-07 2.6e-07 6.8e-08 1.9e-08 3.1e-08 7.1e-07 6.2e-08 2.0e-07 4.1e-08 3.4e-07
    A5     lstm/pna  4.2e-06 3.5e-07 5.4e-07 5.9e-08 6.8e-08 2.0e-08 2.4e-07 8.0e-08 2.0e-07 4.1e-08 1.9e-07
    B1     emb/sum   1.1e-07 2.2e-07 2.4e-07 1.7e-07 1.2e-07 1.9e-07 8.9e-08 3.0e-08 1.5e-07 0.0e+00 1.6e-07
    B1     emb/pna   7.1e-07 2.5e-07 2.8e-07 2.7e-07 6.0e-08 1.4e-07 3.0e-07 2.6e-08 3.0e-07 0.0e+00 1.8e-07
    B1     lstm/sum  2.6e-08 7.6e-07 2.9e-07 1.9e-07 5.4e-08 1.4e-07 1.3e-07 5.2e-08 1.2e-07 0.0e+00 4.9e-08
    B1     lstm/pna  6.9e-07 4.1e-07 1.7e-07 1.3e-07 3.0e-07 1.0e-07 3.9e-07 3.7e-08 1.4e-07 0.0e+00 1.6e-07
    B33    emb/sum   6.4e-07 1.3e-06 2.3e-07 5.5e-08 1.6e-07 4.6e-08 2.1e-07 1.1e-07 8.4e-08 7.8e-09 5.1e-07
    B33    emb/pna   2.6e-06 7.6e-07 1.1e-06 3.6e-07 7.8e-07 5.7e-08 1.2e-06 5.8e-08 8.9e-07 7.8e-09 8.0e-07
    B33    lstm/sum  5.7e-07 5.1e-07 1.9e-07 1.1e-07 5.0e-08 1.1e-07 2.7e-07 9.3e-08 2.5e-07 7.8e-09 5.7e-07
    B33    lstm/pna  2.8e-06 9.4e-07 1.2e-06 3.1e-07 8.4e-07 3.7e-08 5.1e-07 4.6e-08 4.5e-07 7.8e-09 5.6e-07
    B5     emb/sum   6.4e-07 4.2e-07 2.0e-07 4.7e-08 2.2e-07 5.6e-08 3.6e-07 7.9e-08 1.6e-07 5.9e-08 2.0e-07
    B5     emb/pna   2.3e-06 4.9e-07 8.1e-07 2.8e-07 5.6e-07 5.8e-08 1.1e-06 8.7e-08 7.0e-07 5.9e-08 2.9e-07
    B5     lstm/sum  5.4e-07 2.5e-07 3.3e-07 6.0e-08 4.6e-08 8.7e-08 2.9e-07 1.1e-07 2.6e-07 5.9e-08 1.2e-07
    B5     lstm/pna  2.8e-06 6.0e-07 7.6e-07 1.7e-07 4.1e-07 2.4e-08 4.6e-07 6.3e-08 3.9e-07 5.9e-08 1.7e-07
    mixed  emb/sum   2.0e-06 2.5e-07 2.7e-07 9.1e-08 1.6e-07 3.9e-08 1.9e-07 5.7e-08 2.5e-07 1.6e-08 2.7e-07
    mixed  emb/pna   2.6e-06 5.7e-07 8.5e-07 2.1e-07 3.7e-07 6.3e-08 6.0e-07 4.0e-08 3.9e-07 1.6e-08 2.2e-07
    mixed  lstm/sum  1.0e-06 4.7e-07 2.9e-07 7.8e-08 6.8e-08 6.7e-08 2.3e-07 8.5e-08 2.0e-07 1.6e-08 2.4e-07
    mixed  lstm/pna  4.2e-06 8.1e-07 8.2e-07 1.9e-07 4.5e-07 9.1e-08 4.3e-07 6.3e-08 4.2e-07 1.6e-08 2.5e-07
    stars  emb/sum   6.4e-07 4.8e-07 1.5e-07 8.6e-08 2.3e-07 6.5e-08 3.7e-07 6.5e-08 2.1e-07 5.6e-08 4.1e-07
    stars  emb/pna   2.6e-06 6.7e-07 1.1e-06 3.8e-07 8.2e-07 4.1e-08 1.2e-06 1.0e-07 8.6e-07 5.6e-08 2.5e-07
    stars  lstm/sum  5.7e-07 8.3e-07 2.4e-07 7.4e-08 4.6e-08 4.1e-08 3.2e-07 7.9e-08 6.0e-07 5.6e-08 3.0e-07
    stars  lstm/pna  2.8e-06 5.9e-07 1.3e-06 2.9e-07 9.8e-07 4.4e-08 5.8e-07 6.2e-08 4.9e-07 5.6e-08 3.6e-07
    tile   emb/sum   1.0e-06 7.3e-07 1.7e-07 3.8e-08 3.0e-07 3.7e-08 2.1e-07 5.8e-08 1.1e-07 4.7e-08 5.7e-07
    tile   emb/pna   2.6e-06 7.8e-07 1.2e-06 3.8e-07 8.4e-07 3.1e-08 1.2e-06 9.9e-08 9.2e-07 4.7e-08 7.4e-07
    tile   lstm/sum  5.7e-07 4.7e-07 3.4e-07 5.2e-08 4.3e-08 7.9e-08 2.4e-07 8.5e-08 3.6e-07 4.7e-08 3.6e-07
    tile   lstm/pna  2.8e-06 6.5e-07 1.1e-06 2.5e-07 9.8e-07 4.2e-08 5.6e-07 1.1e-07 4.7e-07 4.7e-08 5.2e-07

(test_sets_are_admissible_and_measured prints the rows of the torch at hand.)
"""
import numpy as np
import pytest
import torch

import plus_ref as pr
from oracle import reference_np as ref

VARIANTS = [("emb", "sum"), ("emb", "pna"), ("lstm", "sum"), ("lstm", "pna")]
SHORT = {"rule_to_entity.add_model.layers.0.weight": "add_w", "rule_to_entity.add_model.layers.0.bias": "add_b",
         "rule_to_entity.layer_norm.weight": "ln_w", "rule_to_entity.layer_norm.bias": "ln_b",
         "score_model.layers.0.weight": "s0_w", "score_model.layers.0.bias": "s0_b",
         "score_model.layers.1.weight": "s1_w", "score_model.layers.1.bias": "s1_b", "relation_emb.weight": "rel",
         "bias": "bias", "rule_emb": "rule"}
GRAD_FACTOR, GRAD_FLOOR, SCORE_CAP = 16.0, 2.0 ** -20, 1e-4
E32 = {}  # label -> {tensor: e32}, filled by measure()


def model_fn(agg):
    return pr.sum_forward_backward if agg == "sum" else pr.pna_forward_backward


def measure(label, agg, sd, c, rules, rel_of_row, base, G):
    """(score64, grads64, saved64, bounds): the float64 reference of one input
    and, from the float32 run of the same formulas, the GPU bounds {tensor:
    absolute bound} ('score': on the scores at the candidates)."""
    f = model_fn(agg)
    s64, g64, saved = f(sd, c, rules, rel_of_row, base, G, dtype=torch.float64)
    s32, g32, _ = f(sd, c, rules, rel_of_row, base, G, dtype=torch.float32)
    e = {"score": float(np.abs(s32.astype(np.float64) - s64).max()) if s64.size else 0.0}
    # SUM: the scorer's fp16-split first layer on top (plus_ref.score_split_bound, a priori)
    split = float(pr.score_split_bound(saved).max()) if agg == "sum" and s64.size else 0.0
    bounds = {"score": min(GRAD_FACTOR * e["score"] + split, SCORE_CAP)}
    for n in g64:
        e[n] = pr.rel_err(g32[n], g64[n])
        bounds[n] = max(GRAD_FACTOR * e[n], GRAD_FLOOR) * finite_max(g64[n])
    E32[label] = e
    return s64, g64, saved, bounds


def finite_max(a):
    a = np.abs(np.asarray(a, dtype=np.float64))
    a = a[np.isfinite(a)]
    return float(a.max()) if a.size else 0.0


def measure_stats(label, c, x):
    """(float64 pna_stats, bounds {wsum, wsq, row_scale: absolute}) of the rule table x (float32)."""
    s64 = {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in pr.pna_stats(c, x, torch.float64).items()}
    s32 = {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in pr.pna_stats(c, x, torch.float32).items()}
    e = {k: pr.rel_err(s32[k], s64[k]) for k in ("wsum", "wsq", "row_scale")}
    E32[label] = e
    return s64, {k: max(GRAD_FACTOR * e[k], GRAD_FLOOR) * finite_max(s64[k]) for k in e}


def measure_stats_backward(label, c, x, node, gs):
    """(float64 d_x, its absolute bound) of pna_stats_backward under the four upstream gradients gs."""
    d64 = pr.pna_stats_backward(c, x, node, *gs, dtype=torch.float64)
    d32 = pr.pna_stats_backward(c, x, node, *gs, dtype=torch.float32)
    e = pr.rel_err(d32, d64)
    E32[label] = {"d_x": e}
    return d64, max(GRAD_FACTOR * e, GRAD_FLOOR) * finite_max(d64)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    sg = pr.small_graph(tmp_path_factory.mktemp("plus"), 0)
    g = ref.Graph(sg["path"])
    rules = ref.Rules(sg["rules"], g.relation_size)
    coos = {}

    def coo_of(name):
        if name not in coos:
            h, r, t, etr = pr.batch(sg, g, name)
            coos[name] = (h, r, etr, pr.coo(g, rules, h, r, etr))
        return coos[name]
    return sg, g, rules, coo_of


def test_small_graph_shape(world):
    sg, g, rules, coo_of = world
    assert g.entity_size <= 512 and len(set(g.train_facts)) == len(g.train_facts)
    node = pr.node_of_rule(rules)
    A = [i for i, (hd, _) in enumerate(rules.rules) if hd == pr.REL["A"]]
    assert len(A) == 819 and len(set(node[A].tolist())) == 819
    B = [i for i, (hd, _) in enumerate(rules.rules) if hd == pr.REL["B"]]
    assert len(B) == 6 and len(set(node[B].tolist())) == 5 and not rules.relation2rules[pr.REL["C"]]
    h, r, etr, c = coo_of("stars")
    assert sorted(np.bincount(c["row"], minlength=len(h)).tolist()) == sorted(pr.STARS)
    h, r, etr, c = coo_of("A33")
    lens = np.bincount(c["ce"])
    assert (lens == 24).any() and (lens == 25).any() and lens.max() > 64  # lists at and past the whole-wave walk
    h, r, etr, c = coo_of("mixed")
    assert set(np.bincount(c["row"], minlength=len(h)).tolist()) >= {0, 1, 2, 3}
    assert len(set(r.tolist())) == 4 and (np.diff(r) < 0).any()


@pytest.mark.parametrize("typ,agg", VARIANTS)
@pytest.mark.parametrize("name", ["A5", "B5"])
@pytest.mark.parametrize("feature", ["bias", "none"])
def test_forward_matches_oracle(world, name, typ, agg, feature):
    sg, g, rules, coo_of = world
    h, r, etr, c = coo_of(name)
    sd = pr.params(sg, typ, agg, pr.PARAM_SEED[typ, agg])
    base = sd["bias"] if feature == "bias" else None
    score, _, _ = model_fn(agg)(sd, c, rules, r, base, np.zeros((len(h), g.entity_size), np.float32))
    want, mask = ref.predictorplus_forward(sd, dict(type=typ, aggregator=agg, entity_feature=feature), g, rules, h, r,
                                           etr)
    cand = np.zeros_like(mask)
    cand[c["row"], c["ent"]] = True
    if feature == "none":
        assert np.array_equal(mask, cand)
    else:
        assert mask.all() and np.array_equal(want[~cand], np.broadcast_to(sd["bias"], want.shape)[~cand])
    assert np.abs(want[c["row"], c["ent"]] - score).max() <= 1e-4


def dense_stats_autograd(c, x, rule_ids, gs):
    """d_x by float64 autograd of the dense formulation (layers.py:89-101) on
    the rules rule_ids; returns (n_rules, 16)."""
    A = np.zeros((len(rule_ids), len(c["ent"])))
    pos = {int(i): k for k, i in enumerate(rule_ids)}
    A[[pos[int(i)] for i in c["rule"]], c["ce"]] = c["count"]
    At = torch.from_numpy(A).t()
    xt = torch.from_numpy(np.asarray(x, dtype=np.float64)).requires_grad_(True)
    xf = xt[torch.from_numpy(np.asarray(rule_ids))]
    active = (At != 0).unsqueeze(-1)
    xb = xf.unsqueeze(0)
    mn = torch.where(active, xb, torch.full_like(xb, float("inf"))).min(1)[0]
    mx = torch.where(active, xb, torch.full_like(xb, float("-inf"))).max(1)[0]
    stats = [At.matmul(xf), At.matmul(xf * xf), mn, mx]
    sum((s * torch.from_numpy(np.asarray(g_, dtype=np.float64))).sum() for s, g_ in zip(stats, gs)).backward()
    return xt.grad.numpy()


@pytest.mark.parametrize("name", ["A5", "B5"])
def test_pna_backward_without_ties_is_autograd(world, name):
    sg, g, rules, coo_of = world
    h, r, etr, c = coo_of(name)
    x = pr.params(sg, "emb", "pna", 1)["rule_emb"]
    gs = [np.random.default_rng(k).standard_normal((len(c["ent"]), 16)) + 0.5 for k in range(4)]
    ids = [i for i, _ in rules.relation2rules[int(r[0])]]
    want = dense_stats_autograd(c, x, ids, gs)
    got = pr.pna_stats_backward(c, x, pr.node_of_rule(rules), *gs)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    for k in range(4):  # each upstream gradient alone
        one = [g_ if j == k else np.zeros_like(g_) for j, g_ in enumerate(gs)]
        assert np.abs(pr.pna_stats_backward(c, x, pr.node_of_rule(rules), *one)
                      - dense_stats_autograd(c, x, ids, one)).max() <= 1e-12 * np.abs(want).max()


def planted_ties(sg, rules, seed=1):
    """The emb table with equal rows planted: the twice-listed rule of head B
    (two members of one node) equal in every dimension, B <- r1 r2 (another
    node, reaching the same leaves) equal to it in dimensions 0-7, pairs of
    length-3 bodies of head A equal in dimensions 4-11, and every A <- a b
    (b > 0) equal in dimensions 12-15 to A <- a 0 0, which the rule file lists
    before it and the trie numbers after it."""
    x = pr.params(sg, "emb", "pna", seed)["rule_emb"].copy()
    B = [i for i, (hd, b) in enumerate(rules.rules) if hd == pr.REL["B"]]
    dup = [i for i in B if rules.rules[i][1] == [pr.REL["r1"]]]
    two = [i for i in B if rules.rules[i][1] == [pr.REL["r1"], pr.REL["r2"]]][0]
    x[dup[1]] = x[dup[0]]
    x[two, :8] = x[dup[0], :8]
    A3 = [i for i, (hd, b) in enumerate(rules.rules) if hd == pr.REL["A"] and len(b) == 3]
    x[A3[1::2], 4:12] = x[A3[0::2][:len(A3[1::2])], 4:12]
    at = {tuple(b): i for i, (hd, b) in enumerate(rules.rules) if hd == pr.REL["A"]}
    for (a, b) in [k for k in at if len(k) == 2 and k[1] > 0]:
        x[at[a, b], 12:] = x[at[a, 0, 0], 12:]
    return x


@pytest.mark.parametrize("name", ["A5", "B5"])
def test_pna_backward_with_ties_conserves_the_sum(world, name):
    sg, g, rules, coo_of = world
    h, r, etr, c = coo_of(name)
    x = planted_ties(sg, rules)
    gs = [np.random.default_rng(k).standard_normal((len(c["ent"]), 16)) + 0.5 for k in range(4)]
    ids = [i for i, _ in rules.relation2rules[int(r[0])]]
    want = dense_stats_autograd(c, x, ids, gs)
    got = pr.pna_stats_backward(c, x, pr.node_of_rule(rules), *gs)
    assert np.abs(got - want).max() > 1e-3  # the routings differ ...
    assert np.abs(got.sum(0) - want.sum(0)).max() <= 1e-12 * np.abs(want).max()  # ... and conserve the sum


def test_pna_tie_routing_by_hand():
    """One candidate reached by rule 0 (node 0), rule 1 (node 1) and rule 2
    (node 0 again: the same body listed twice), min / max gradient 1:
      dim 0  x = 1, 1, 1  all tied: node 0, its two members half each (min and max)
      dim 1  x = 2, 1, 3  no tie: min to rule 1, max to rule 2
      dim 2  x = 1, 1, 5  min tied across nodes: node 0, of whose members only rule 0 is at 1
      dim 3  x = 4, 7, 7  max tied across nodes: node 0, of whose members only rule 2 is at 7"""
    c = dict(nq=1, E=1, row=np.zeros(1, np.int64), ent=np.zeros(1, np.int64), ce=np.zeros(3, np.int64),
             rule=np.arange(3), count=np.asarray([1, 2, 1]))
    x = np.arange(48, dtype=np.float64).reshape(3, 16)
    x[:, :4] = [[1, 2, 1, 4], [1, 1, 1, 7], [1, 3, 5, 7]]
    z, one = np.zeros((1, 16)), np.ones((1, 16))
    d_mn = pr.pna_stats_backward(c, x, [0, 1, 0], z, z, one, z)
    d_mx = pr.pna_stats_backward(c, x, [0, 1, 0], z, z, z, one)
    assert d_mn[:, :4].tolist() == [[0.5, 0, 1, 1], [0, 1, 0, 0], [0.5, 0, 0, 0]]
    assert d_mx[:, :4].tolist() == [[0.5, 0, 0, 0], [0, 0, 0, 0], [0.5, 1, 1, 1]]
    assert d_mn[:, 4:].tolist() == [[1] * 12, [0] * 12, [0] * 12] and d_mx[:, 4:].tolist() == [[0] * 12] * 2 + [[1] * 12]
    d_s = pr.pna_stats_backward(c, x, [0, 1, 0], one, one, z, z)
    assert np.array_equal(d_s, np.asarray([[1], [2], [1]]) * (1 + 2 * x))


@pytest.mark.parametrize("typ,agg", VARIANTS)
@pytest.mark.parametrize("name", sorted(pr.SETS))
def test_sets_are_admissible_and_measured(world, name, typ, agg):
    """Admissibility of every (set, variant) the GPU tests use, with every
    candidate carrying a gradient; prints the set's e32 row."""
    sg, g, rules, coo_of = world
    h, r, etr, c = coo_of(name)
    sd = pr.params(sg, typ, agg, pr.PARAM_SEED[typ, agg])
    G = pr.upstream(len(h), g.entity_size, 0)
    label = "%s %s/%s" % (name, typ, agg)
    s64, g64, saved, bounds = measure(label, agg, sd, c, rules, r, sd["bias"], G)
    a, m = pr.margins(saved, G)
    assert len(a) == len(c["ent"]) * (144 + (16 if agg == "pna" else 0))
    assert (np.abs(a) > m).all(), (label, float((np.abs(a) / m).min()))
    e = E32[label]
    rule = e["rule_emb"] if typ == "emb" else max(e[n] for n in pr.LSTM_NAMES)
    print("%-16s %.1e  %.1e " % (label, e["score"], rule)
          + " ".join("%.1e" % e[n] for n in pr.DENSE_NAMES) + "  |a|/m >= %.2f" % float((np.abs(a) / m).min()))
    # the float32 run is itself a sane implementation of the same function
    assert e["score"] <= 1e-4 and all(v <= 1e-3 for v in e.values())
    # rows without a rule (head C) and absent relations get no relation_emb gradient
    got_rel = np.abs(g64["relation_emb.weight"]).max(1) > 0
    assert set(np.nonzero(got_rel)[0].tolist()) == set(r[c["row"]].tolist())
