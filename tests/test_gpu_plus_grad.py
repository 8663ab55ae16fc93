"""The SUM and PNA training kernels (rnnlogic_amd/csrc/backward.hip,
pna_grad.hip) against the float64 reference of tests/plus_ref.py, whose
grounding is the CPU oracle's (not ground_kernel's export), on the small graph
of plus_ref.small_graph: PredictorPlus(hidden_dim=16) with plus_ref.params,
driven through forward_autograd + score.backward(gradient=G) with the test's
own upstream gradient G, and _PnaStats.apply with the test's own four.

Bounds: tests/test_plus_ref.measure runs the same formulas in float32 on the
CPU for the very input of each case; a tensor's bound is 16 x that float32
error (gradients: never below 2^-20 of the tensor's largest float64 magnitude;
scores: never above 1e-4; the SUM scores add plus_ref.score_split_bound, the
a-priori size of the eval scorer's dropped lo x lo fp16 part).  Every input set is admissible
(test_plus_ref.test_sets_are_admissible_and_measured); no case is skipped or
masked.  Exact where the operation is a selection or an integer: masks, deg,
row, ent, mn, mx, and every gradient of a launch without a score gradient.

Cases: one-relation batches of head A (819 trie nodes: past BW_LDS_NODES and
PG_LDS_NODES, bucket lists at and past BW_BIG) and head B (stars of 1 - 129
candidates) with 1 / 5 / 33 rows, entity feature none / bias, emb / lstm; the
stars together and alone; mixed relations (head = -1) unsorted, sorted and as
four one-relation batches; 1,100 rows (more than BW_GRID x 4 chunks and
PG_GRID x 4 candidates); an upstream gradient at one candidate per row, at
non-candidates only, all zero, x 2^-60, x 2^40, with one NaN and with one
+inf; _PnaStats forward and backward with the four gradients together, alone,
zero, scaled and NaN; planted ties; the whole PNA model.

Observed on an MI355X (scores: max abs error at the candidates; gradients:
max abs error / max |ref|; the worst of each group's cases — 1 / 5 / 33 rows:
over type and entity feature — and no bound raised; test_zz_print_figures
prints the table of the run at hand):

    case        score   rule    add_w   add_b   ln_w    ln_b    s0_w    s0_b    s1_w    s1_b    rel     bias
    pna A1      3.9e-06 3.8e-07 2.8e-07 1.2e-07 1.7e-07 1.9e-07 2.0e-07 5.6e-08 1.5e-07 1.1e-08 1.3e-07 0.0e+00
    pna A33     2.8e-06 7.2e-07 3.6e-07 1.4e-07 2.9e-08 9.3e-08 7.7e-07 7.6e-08 1.7e-07 5.1e-08 6.5e-08 8.2e-08
    pna A5      3.9e-06 3.7e-07 7.3e-07 1.3e-07 7.9e-08 8.9e-08 3.6e-07 8.9e-08 4.3e-07 2.1e-08 2.8e-07 6.0e-08
    pna B1      2.1e-07 4.1e-07 2.0e-07 1.0e-07 3.2e-07 7.1e-08 2.3e-07 4.7e-08 1.9e-07 0.0e+00 1.7e-07 0.0e+00
    pna B33     1.1e-06 4.4e-07 3.3e-07 1.1e-07 1.0e-07 9.7e-08 1.1e-06 6.5e-08 3.1e-07 6.4e-08 3.4e-08 8.2e-08
    pna B5      1.4e-06 4.9e-07 4.8e-07 2.2e-07 7.0e-07 1.4e-07 3.4e-07 9.2e-08 3.5e-07 6.7e-08 8.9e-08 6.0e-08
    pna mixed   2.6e-06 2.7e-07 7.9e-07 1.0e-07 6.6e-08 8.0e-08 6.2e-07 9.7e-08 4.9e-07 3.2e-08 8.4e-08 8.6e-08
    pna tiled   9.1e-07 1.1e-07 1.4e-06 1.7e-07 1.5e-07 6.5e-08 3.7e-06 1.0e-07 1.0e-06 2.2e-08 1.8e-07 1.2e-07
    sum A1      1.3e-06 2.5e-07 1.1e-07 1.4e-07 1.1e-07 1.4e-07 2.7e-07 2.6e-07 1.6e-07 1.1e-08 1.4e-07 0.0e+00
    sum A33     2.1e-06 4.3e-07 1.4e-07 4.4e-08 9.0e-08 3.9e-08 7.6e-08 5.3e-08 1.6e-07 3.7e-08 1.9e-07 8.2e-08
    sum A5      1.9e-06 6.6e-07 3.0e-07 2.4e-07 1.4e-07 3.0e-07 8.6e-08 1.1e-07 1.7e-07 4.8e-08 3.3e-07 6.5e-08
    sum B1      1.1e-06 4.3e-07 2.3e-07 1.7e-07 1.6e-07 1.4e-07 1.0e-07 5.4e-08 1.8e-07 0.0e+00 2.0e-07 0.0e+00
    sum B33     1.1e-06 2.9e-07 9.9e-08 8.0e-08 1.8e-07 8.6e-08 1.2e-07 6.9e-08 1.7e-07 2.6e-08 2.5e-07 8.2e-08
    sum B5      1.1e-06 7.4e-07 1.1e-07 1.5e-07 1.7e-07 7.9e-08 2.4e-07 1.2e-07 1.7e-07 6.7e-08 2.7e-07 6.0e-08
    sum mixed   1.9e-06 9.6e-07 1.5e-07 5.9e-08 1.2e-07 5.6e-08 1.5e-07 1.2e-07 1.2e-07 3.2e-08 9.8e-08 1.2e-07
    sum star    1.1e-06 1.4e-07 2.0e-07 1.8e-07 2.8e-07 1.4e-07 2.9e-07 2.7e-07 1.7e-07 7.2e-08 2.6e-07 0.0e+00
    sum stars   1.1e-06 6.2e-08 7.8e-08 4.7e-08 2.2e-07 4.5e-08 1.0e-07 8.8e-08 9.6e-08 5.7e-08 4.2e-07 7.0e-08
    sum tiled   1.1e-06 1.2e-07 1.2e-07 4.0e-08 2.1e-07 3.1e-08 1.1e-07 8.5e-08 8.3e-08 2.2e-08 4.2e-08 1.2e-07
    stats       wsum 3.7e-08  wsq 5.6e-08  row_scale 1.2e-07  d_x 6.4e-08
    ties        d_x 4.8e-08

Found by these tests, and fixed: with a NaN or an inf in G, sum_backward_kernel
left score_model.layers.1.weight's gradient finite at the hidden units that
are inactive at that candidate (55 of 128 non-finite), where the reference's
product g x relu(h) = g x 0 is NaN (128 of 128).  Found, and documented (DESIGN
§3.11): the training forward's node records carry the head's own fixed-point
shift, so its scores are the eval path's bit for bit only where the head's
largest record shares the whole table's binade; the lstm model's head A (shift
30 against 29) differs from the eval scores by up to 7.2e-7, both within the
bound of float64.

Self-check on scratch builds (not committed): without the xh x m2 term of the
LayerNorm backward 36 of these tests fail (and 8 of the 12 cases of
test_fused_backward_matches_autograd); with PNA's min gradient routed to the
largest tied node the four test_pna_ties cases fail (the older test: none);
without flush_rel at a relation change test_tiled_rows[sum] fails (the older
test: none).
"""
import ctypes

import numpy as np
import pytest
import torch

import plus_ref as pr
import test_plus_ref as tpr
from oracle import reference_np as ref

pytestmark = pytest.mark.gpu

FIG = {}  # label -> {tensor: observed error / bound scale}, printed by test_zz_print_figures


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


class World:
    def __init__(self, root):
        from rnnlogic_amd.data import KnowledgeGraph
        self.sg = pr.small_graph(root, 0)
        self.g = ref.Graph(self.sg["path"])
        self.rules = ref.Rules(self.sg["rules"], self.g.relation_size)
        self.graph = KnowledgeGraph(self.sg["path"])
        self.E = self.g.entity_size
        self.node = pr.node_of_rule(self.rules)
        self._coo, self._model = {}, {}

    def rows(self, name):
        return pr.batch(self.sg, self.g, name)

    def coo(self, key, h, r, etr):
        if key not in self._coo:
            self._coo[key] = pr.coo(self.g, self.rules, h, r, etr)
        return self._coo[key]

    def model(self, typ, agg, feature, dev):
        """(model in train mode, its float32 state dict as numpy)."""
        from rnnlogic_amd.predictors import PredictorPlus
        key = (typ, agg, feature)
        if key not in self._model:
            sd = pr.params(self.sg, typ, agg, pr.PARAM_SEED[typ, agg])
            m = PredictorPlus(self.graph, type=typ, num_layers=3, hidden_dim=16, entity_feature=feature,
                              aggregator=agg)
            m.set_rules(self.sg["rules"])
            with torch.no_grad():
                for n, prm in m.named_parameters():
                    prm.copy_(torch.from_numpy(sd[n]))
            self._model[key] = (m.to(dev).train(), sd)
        return self._model[key]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return World(tmp_path_factory.mktemp("plus_gpu"))


def dev_rows(h, r, etr, dev):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (h, r, etr)]


def run_model(model, h, r, etr, G, dev, query_r=None):
    """(score, mask, {parameter name: gradient or None}) of forward_autograd + backward(gradient=G)."""
    model.zero_grad(set_to_none=True)
    th, tr, te = dev_rows(h, r, etr, dev)
    score, mask = model.forward_autograd(th, tr, te, query_r=query_r)
    score.backward(gradient=torch.from_numpy(np.ascontiguousarray(G)).to(dev))
    torch.cuda.synchronize()
    grads = {n: (p.grad.detach().cpu().numpy().copy() if p.grad is not None else None)
             for n, p in model.named_parameters()}
    return score.detach().cpu().numpy(), mask.cpu().numpy(), grads


def check(label, got, want, c, sd, feature):
    """Scores at the candidates, the mask, the rest of the score rows, and
    every gradient the reference has, against `want` = measure()'s result."""
    score, mask, grads = got
    s64, g64, _, bounds = want
    cand = np.zeros(score.shape, dtype=bool)
    cand[c["row"], c["ent"]] = True
    fig = FIG.setdefault(label, {})
    if feature == "none":
        assert np.array_equal(mask, cand), label
        assert np.all(score[~cand] == -np.inf), label
    else:
        assert mask.all(), label
        assert np.array_equal(score[~cand], np.broadcast_to(sd["bias"], score.shape)[~cand]), label
    if s64.size:
        fig["score"] = float(np.abs(score[c["row"], c["ent"]] - s64).max())
        print("%-28s score %.2e (bound %.2e)" % (label, fig["score"], bounds["score"]))
    for n, w in g64.items():
        if n == "bias" and feature == "none":
            continue
        g = grads[n]
        assert g is not None or not np.any(w), (label, n)
        g = np.zeros_like(w) if g is None else g
        assert np.isfinite(g).all(), (label, n)
        err, top = float(np.abs(g - w).max()), float(np.abs(w).max())
        fig[n] = err / top if top > 0 else err
        print("%-28s %-42s %.2e of max |ref| (bound %.2e)" % (label, n, fig[n], bounds[n] / top if top > 0 else 0))
    assert "score" not in fig or fig["score"] <= bounds["score"], (label, fig["score"], bounds["score"])
    for n, w in g64.items():
        if n in fig:
            top = float(np.abs(w).max())
            assert fig[n] * (top if top > 0 else 1) <= bounds[n], (label, n, fig[n], bounds[n])


def reference(world, label, agg, sd, feature, key, h, r, etr, G):
    c = world.coo(key, h, r, etr)
    return c, tpr.measure(label, agg, sd, c, world.rules, r, sd["bias"] if feature == "bias" else None, G)


def sum_table_shift(model, dev, head=None):
    """The fixed-point shift of the SUM node records (trailer word 1): of the
    whole table (rnnl_node_weights: the eval path's), or of `head`'s trie alone
    (rnnl_node_weights_head: the training forward's)."""
    from rnnlogic_amd import _native
    nr = model.native_rules(dev)
    with torch.no_grad():
        emb = model.all_rule_embeddings().detach().float().contiguous()
    add_w = model.rule_to_entity.add_model.layers[0].weight.detach().float().contiguous()
    n = ctypes.c_size_t()
    _native.call("rnnl_node_weights_size", nr.ptr, _native.AGG_SUM, ctypes.byref(n))
    w = torch.zeros(n.value, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    if head is None:
        _native.call("rnnl_node_weights", nr.ptr, emb.data_ptr(), 16, _native.AGG_SUM, add_w.data_ptr(), w.data_ptr(),
                     stream)
    else:
        _native.call("rnnl_node_weights_head", nr.ptr, head, emb.data_ptr(), 16, _native.AGG_SUM, add_w.data_ptr(),
                     w.data_ptr(), stream)
    torch.cuda.synchronize()
    return int(w[n.value - 64:n.value - 48].cpu().numpy().view(np.int32)[1])


# --------------------------------------------------------------------------- SUM
@pytest.mark.parametrize("typ", ["emb", "lstm"])
@pytest.mark.parametrize("feature", ["none", "bias"])
@pytest.mark.parametrize("name", ["A1", "A5", "A33", "B1", "B5", "B33"])
def test_sum_one_relation(world, dev, name, feature, typ):
    """Case 1: scores, mask and every gradient of a one-relation batch; the
    training scores are the eval path's bit for bit."""
    model, sd = world.model(typ, "sum", feature, dev)
    h, r, t, etr = world.rows(name)
    G = pr.upstream(len(h), world.E, 1)
    label = "sum %s %s/%s" % (name, typ, feature)
    c, want = reference(world, label, "sum", sd, feature, name, h, r, etr, G)
    got = run_model(model, h, r, etr, G, dev, query_r=int(r[0]))
    check(label, got, want, c, sd, feature)
    model.eval()
    with torch.no_grad():
        es, em = model.forward_rows(*dev_rows(h, r, etr, dev))
    model.train()
    es = es.cpu().numpy()
    assert np.array_equal(em.cpu().numpy(), got[1]), label
    # the training forward folds the batch relation's trie only: its records
    # are the eval table's — and the scores the eval path's bit for bit —
    # when the head's largest record is in the binade of the whole table's
    # (one fixed-point shift per table); else they sit on a finer grid
    shifts = sum_table_shift(model, dev), sum_table_shift(model, dev, int(r[0]))
    if shifts[0] == shifts[1]:
        assert np.array_equal(es, got[0]), label
    else:
        diff = float(np.abs(es[c["row"], c["ent"]] - got[0][c["row"], c["ent"]]).max())
        print("%-28s eval shift %d, training shift %d: scores differ by %.2e" % (label, shifts[0], shifts[1], diff))
        assert shifts[1] > shifts[0] and np.array_equal(es[~got[1]], got[0][~got[1]]), label
        assert float(np.abs(es[c["row"], c["ent"]] - want[0]).max()) <= want[3]["score"], label


def test_sum_stars(world, dev):
    """Case 2: the star centres with 1 / 23 / 24 / 25 / 63 / 64 / 65 / 129
    candidates in one batch and each alone."""
    model, sd = world.model("emb", "sum", "bias", dev)
    h, r, t, etr = world.rows("stars")
    G = pr.upstream(len(h), world.E, 2)
    c, want = reference(world, "sum stars", "sum", sd, "bias", "stars", h, r, etr, G)
    assert sorted(np.bincount(c["row"]).tolist()) == sorted(pr.STARS)
    check("sum stars", run_model(model, h, r, etr, G, dev, query_r=int(r[0])), want, c, sd, "bias")
    for k in range(len(h)):
        label = "sum star %d" % pr.STARS[k]
        hk, rk, ek, Gk = h[k:k + 1], r[k:k + 1], etr[k:k + 1], G[k:k + 1]
        c, want = reference(world, label, "sum", sd, "bias", label, hk, rk, ek, Gk)
        assert len(c["ent"]) == pr.STARS[k]
        check(label, run_model(model, hk, rk, ek, Gk, dev, query_r=int(rk[0])), want, c, sd, "bias")


def add_grads(parts):
    out = {}
    for g in parts:
        for n, v in g.items():
            if v is not None:
                out[n] = out.get(n, 0) + v.astype(np.float64)
    return out


@pytest.mark.parametrize("agg", ["sum", "pna"])
@pytest.mark.parametrize("typ", ["emb", "lstm"])
def test_mixed_relations(world, dev, typ, agg):
    """Cases 3 and 11: rows of heads A, B, C, D interleaved (query_r None:
    head = -1), unsorted and sorted by relation; relation_emb's gradient is zero
    for head C (no rule) and every absent relation; the same rows as four
    one-relation batches sum to the same gradients within the bound."""
    model, sd = world.model(typ, agg, "bias", dev)
    h, r, t, etr = world.rows("mixed")
    G = pr.upstream(len(h), world.E, 3)
    label = "%s mixed %s" % (agg, typ)
    c, want = reference(world, label, agg, sd, "bias", "mixed", h, r, etr, G)
    got = run_model(model, h, r, etr, G, dev)
    check(label, got, want, c, sd, "bias")
    live = set(r[c["row"]].tolist())
    assert pr.REL["C"] not in live and len(live) == 3
    for q in range(pr.NREL):
        if q not in live:
            assert not got[2]["relation_emb.weight"][q].any(), (label, q)
    order = np.argsort(r, kind="stable")
    hs, rs, es, Gs = h[order], r[order], etr[order], G[order]
    cs, wants = reference(world, label + " sorted", agg, sd, "bias", "mixed sorted", hs, rs, es, Gs)
    check(label + " sorted", run_model(model, hs, rs, es, Gs, dev), wants, cs, sd, "bias")
    parts = []
    for q in np.unique(r):
        sel = r == q
        parts.append(run_model(model, h[sel], r[sel], etr[sel], G[sel], dev, query_r=int(q))[2])
    total = add_grads(parts)
    for n, w in want[1].items():
        assert np.abs(total[n] - w).max() <= want[3][n], (label, "four batches", n)


@pytest.mark.parametrize("agg", ["sum", "pna"])
def test_tiled_rows(world, dev, agg):
    """Cases 4 and 11: 1,100 rows tiled from heads B and D in one mixed
    launch — more chunks than BW_GRID x 4 waves (a wave walks several and
    flushes at the relation changes) and more candidates than PG_GRID x 4:
    against float64, and against the tile count times the untiled gradients."""
    model, sd = world.model("emb", agg, "bias", dev)
    h, r, t, etr = world.rows("tile")
    G = pr.upstream(len(h), world.E, 4)
    tiles = 25
    ht, rt, et, Gt = (np.concatenate([a] * tiles) for a in (h, r, etr, G))
    label = "%s tiled" % agg
    c, want = reference(world, label, agg, sd, "bias", "tile x25", ht, rt, et, Gt)
    assert len(ht) == 1100 and len(c["ent"]) > 960
    got = run_model(model, ht, rt, et, Gt, dev)
    check(label, got, want, c, sd, "bias")
    one = run_model(model, h, r, etr, G, dev)[2]
    for n, w in want[1].items():
        assert np.abs(tiles * one[n].astype(np.float64) - w).max() <= want[3][n], (label, "tiles", n)


@pytest.mark.parametrize("name", ["A5", "B5"])
def test_sum_sparse_and_zero_gradient(world, dev, name):
    """Case 5: an upstream gradient at one candidate per row; at
    non-candidates only (every rule-part gradient exactly 0, the bias gradient
    G's column sums); all zero (every gradient exactly 0, nothing non-finite)."""
    model, sd = world.model("emb", "sum", "bias", dev)
    h, r, t, etr = world.rows(name)
    c = world.coo(name, h, r, etr)
    full = pr.upstream(len(h), world.E, 5)
    G = np.zeros_like(full)
    for q in np.unique(c["row"]):  # the row's third candidate, or its last
        ks = np.nonzero(c["row"] == q)[0]
        k = ks[min(2, len(ks) - 1)]
        G[q, c["ent"][k]] = full[q, c["ent"][k]]
    label = "sum %s one candidate" % name
    _, want = reference(world, label, "sum", sd, "bias", name, h, r, etr, G)
    check(label, run_model(model, h, r, etr, G, dev, query_r=int(r[0])), want, c, sd, "bias")
    G = full.copy()
    G[c["row"], c["ent"]] = 0
    for lab, Gz in (("non-candidates", G), ("zero", np.zeros_like(full))):
        score, mask, grads = run_model(model, h, r, etr, Gz, dev, query_r=int(r[0]))
        for n, g in grads.items():
            if n == "bias":  # a float32 sum of len(h) terms in any order
                tol = len(h) * 2.0 ** -24 * np.abs(Gz).sum(0, dtype=np.float64)
                assert np.all(np.abs(g - Gz.sum(0, dtype=np.float64)) <= tol), (name, lab)
            elif g is not None:
                assert not g.any(), (name, lab, n)  # exactly 0.0 (and finite)


@pytest.mark.parametrize("exp", [-60, 40])
@pytest.mark.parametrize("name", ["A5", "B5", "mixed"])
def test_sum_scaled_gradient(world, dev, name, exp):
    """Case 6: G x 2^-60 and G x 2^40 — the fixed-point scale follows the
    magnitude: the same relative bounds against float64."""
    model, sd = world.model("emb", "sum", "bias", dev)
    h, r, t, etr = world.rows(name)
    G = np.ldexp(pr.upstream(len(h), world.E, 6), exp).astype(np.float32)
    label = "sum %s x 2^%d" % (name, exp)
    c, want = reference(world, label, "sum", sd, "bias", name, h, r, etr, G)
    got = run_model(model, h, r, etr, G, dev, query_r=int(r[0]) if name != "mixed" else None)
    check(label, got, want, c, sd, "bias")


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_sum_nonfinite_gradient(world, dev, bad):
    """Case 7: one NaN / +inf in G at a candidate of head B.  The non-finite
    gradient entries are those of torch's fp32 autograd on the grounding COO
    (fused_backward False: the reference formulation, where 0 x NaN of an
    inactive hidden unit is NaN in score_model.layers.1.weight), every finite
    entry within the bound."""
    model, sd = world.model("emb", "sum", "bias", dev)
    h, r, t, etr = world.rows("B5")
    c = world.coo("B5", h, r, etr)
    G = pr.upstream(len(h), world.E, 7)
    k = int(np.nonzero(c["row"] == 2)[0][5])
    G[c["row"][k], c["ent"][k]] = bad
    label = "sum B5 %s" % bad
    _, want = reference(world, label, "sum", sd, "bias", "B5", h, r, etr, G)
    fused = run_model(model, h, r, etr, G, dev, query_r=int(r[0]))[2]
    model.fused_backward = False
    try:
        torch_ = run_model(model, h, r, etr, G, dev, query_r=int(r[0]))[2]
    finally:
        model.fused_backward = True
    for n, w in want[1].items():
        a, b = fused[n], torch_[n]
        assert np.array_equal(np.isfinite(a), np.isfinite(b)), (label, n, int((~np.isfinite(a)).sum()),
                                                                int((~np.isfinite(b)).sum()))
        ok = np.isfinite(a)
        assert np.isfinite(w[ok]).all(), (label, n)
        if ok.any():
            err = float(np.abs(a[ok] - w[ok]).max())
            print("%-28s %-42s %d non-finite, finite entries %.2e (bound %.2e)" % (label, n, (~ok).sum(), err,
                                                                                 want[3][n]))
            assert err <= want[3][n], (label, n, err, want[3][n])
    assert not np.isfinite(fused["rule_emb"]).all() and np.isfinite(fused["rule_emb"]).any()


# --------------------------------------------------------------------------- PNA statistics
def run_stats(model, x, h, r, etr, head, dev, gs=None):
    """_PnaStats.apply on the table x: the eight outputs sorted by (row,
    entity) as numpy, and d_x under the four upstream gradients gs (given in
    that sorted order)."""
    from rnnlogic_amd.predictors import _PnaStats
    emb = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev).requires_grad_(True)
    th, tr, te = dev_rows(h, r, etr, dev)
    out = _PnaStats.apply(model, emb, th, tr, te, head)
    row, ent = out[5].cpu().numpy(), out[6].cpu().numpy()
    order = np.argsort(row * model.num_entities + ent, kind="stable")
    res = dict(zip(("wsum", "wsq", "mn", "mx", "deg", "row", "ent"), (o.detach().cpu().numpy()[order] for o in out[:7])))
    res["row_scale"] = out[7].cpu().numpy()
    d_x = None
    if gs is not None:
        inv = torch.from_numpy(np.argsort(order)).to(dev)
        ups = [torch.from_numpy(np.ascontiguousarray(g, dtype=np.float32)).to(dev)[inv] for g in gs]
        torch.autograd.backward(list(out[:4]), ups)
        torch.cuda.synchronize()
        d_x = emb.grad.cpu().numpy()
    return res, d_x


STAT_SETS = ["A5", "A33", "B33", "mixed", "tile x25"]


def stat_rows(world, name):
    if name == "tile x25":
        h, r, t, etr = world.rows("tile")
        return [np.concatenate([a] * 25) for a in (h, r, etr)]
    h, r, t, etr = world.rows(name)
    return h, r, etr


@pytest.mark.parametrize("mixed_launch", [False, True])
@pytest.mark.parametrize("name", STAT_SETS)
def test_pna_stats_forward(world, dev, name, mixed_launch):
    """Case 8: deg / row / ent exact, mn / mx exact (selections of fp32
    inputs), wsum / wsq / row_scale within the bound; one-relation launches and
    head = -1; more than 960 candidates (A33, B33, the 1,100 rows); head A past
    PG_LDS_NODES."""
    model, sd = world.model("emb", "pna", "bias", dev)
    h, r, etr = stat_rows(world, name)
    one = len(set(r.tolist())) == 1
    if not one and not mixed_launch:
        h, r, etr = h[r == pr.REL["D"]], r[r == pr.REL["D"]], etr[r == pr.REL["D"]]  # head D alone
        name = name + " D"
        one = True
    head = int(r[0]) if one and not mixed_launch else -1
    label = "stats %s head %d" % (name, head)
    c = world.coo(name, h, r, etr)
    x = sd["rule_emb"]
    s64, bounds = tpr.measure_stats(label, c, x)
    got, _ = run_stats(model, x, h, r, etr, head, dev)
    assert np.array_equal(got["row"], c["row"]) and np.array_equal(got["ent"], c["ent"]), label
    assert np.array_equal(got["deg"].astype(np.float64), s64["deg"]), label
    assert np.array_equal(got["mn"].astype(np.float64), s64["mn"]), label
    assert np.array_equal(got["mx"].astype(np.float64), s64["mx"]), label
    fig = FIG.setdefault(label, {})
    for k in ("wsum", "wsq", "row_scale"):
        err, top = float(np.abs(got[k] - s64[k]).max()), float(np.abs(s64[k]).max())
        fig[k] = err / top
        print("%-28s %-10s %.2e of max |ref| (bound %.2e)" % (label, k, fig[k], bounds[k] / top))
        assert err <= bounds[k], (label, k, err, bounds[k])


def upstream4(C, seed):
    rng = np.random.default_rng(8000 + seed)
    return [(rng.standard_normal((C, 16)) + 0.5).astype(np.float32) for _ in range(4)]


def check_dx(label, d_x, d64, bound):
    top = float(np.abs(d64).max())
    err = float(np.abs(d_x - d64).max())
    FIG.setdefault(label, {})["d_x"] = err / top if top > 0 else err
    print("%-36s d_x %.2e of max |ref| (bound %.2e)" % (label, err / top if top > 0 else err,
                                                       bound / top if top > 0 else 0))
    assert np.isfinite(d_x).all() and err <= bound, (label, err, bound)


@pytest.mark.parametrize("name,mixed_launch", [("A5", False), ("A5", True), ("B33", False), ("B33", True),
                                               ("mixed", True)])
def test_pna_stats_backward(world, dev, name, mixed_launch):
    """Case 9: d_x under the four upstream gradients together, each alone,
    all zero (exactly 0), x 2^-60 and x 2^40, and with one NaN (every d_x of
    the launch's nodes NaN, as pna_grad_rules_kernel documents; the next
    launch is undisturbed: bitwise the result before it)."""
    model, sd = world.model("emb", "pna", "bias", dev)
    h, r, etr = stat_rows(world, name)
    head = -1 if mixed_launch else int(r[0])
    c = world.coo(name, h, r, etr)
    x = sd["rule_emb"]
    gs = upstream4(len(c["ent"]), 0)
    variants = [("all four", gs)]
    for k, what in enumerate(("wsum", "wsq", "mn", "mx")):
        variants.append((what + " alone", [g if j == k else np.zeros_like(g) for j, g in enumerate(gs)]))
    variants += [("x 2^-60", [np.ldexp(g, -60).astype(np.float32) for g in gs]),
                 ("x 2^40", [np.ldexp(g, 40).astype(np.float32) for g in gs])]
    first = None
    for what, ups in variants:
        label = "stats bwd %s head %d %s" % (name, head, what)
        d64, bound = tpr.measure_stats_backward(label, c, x, world.node, ups)
        d_x = run_stats(model, x, h, r, etr, head, dev, ups)[1]
        first = d_x if first is None else first
        check_dx(label, d_x, d64, bound)
    zero = run_stats(model, x, h, r, etr, head, dev, [np.zeros_like(g) for g in gs])[1]
    assert not zero.any()
    bad = [g.copy() for g in gs]
    bad[1][len(bad[1]) // 2, 3] = float("nan")
    d_nan = run_stats(model, x, h, r, etr, head, dev, bad)[1]
    ids = [i for q in np.unique(r) for i, _ in world.rules.relation2rules[int(q)]] if head >= 0 else \
        list(range(len(world.rules.rules)))
    assert np.isnan(d_nan[ids]).all()
    rest = np.setdiff1d(np.arange(len(d_nan)), ids)
    assert not d_nan[rest].any()
    again = run_stats(model, x, h, r, etr, head, dev, gs)[1]
    assert np.array_equal(again, first)


@pytest.mark.parametrize("mixed_launch", [False, True])
@pytest.mark.parametrize("name", ["A5", "B5"])
def test_pna_ties(world, dev, name, mixed_launch):
    """Case 10: planted equal rows (test_plus_ref.planted_ties: two members of
    one node; two nodes reaching the same candidates; a tie whose rule-file
    order and trie order disagree): d_x entry by entry against
    pna_stats_backward's stated convention, min and max gradients alone too."""
    model, sd = world.model("emb", "pna", "bias", dev)
    h, r, etr = stat_rows(world, name)
    head = -1 if mixed_launch else int(r[0])
    c = world.coo(name, h, r, etr)
    x = tpr.planted_ties(world.sg, world.rules)
    # the reference's node order is the library's
    nr = model.native_rules(dev)
    lib_node = nr.node_of_rule.cpu().numpy()
    assert np.array_equal(np.unique(lib_node, return_inverse=True)[1], np.unique(world.node, return_inverse=True)[1])
    gs = upstream4(len(c["ent"]), 1)
    z = np.zeros_like(gs[0])
    for what, ups in (("all four", gs), ("mn alone", [z, z, gs[2], z]), ("mx alone", [z, z, z, gs[3]])):
        label = "ties %s head %d %s" % (name, head, what)
        d64, bound = tpr.measure_stats_backward(label, c, x, world.node, ups)
        got, d_x = run_stats(model, x, h, r, etr, head, dev, ups)
        check_dx(label, d_x, d64, bound)
    # the ties are live: some candidate's min is shared by two entries
    tied = x[c["rule"]] == got["mn"][c["ce"]]
    assert max(np.bincount(c["ce"], weights=tied[:, d].astype(float)).max() for d in range(16)) > 1


# --------------------------------------------------------------------------- the whole PNA model
@pytest.mark.parametrize("typ", ["emb", "lstm"])
@pytest.mark.parametrize("feature", ["none", "bias"])
@pytest.mark.parametrize("name", ["A1", "A5", "A33", "B1", "B5", "B33"])
def test_pna_one_relation(world, dev, name, feature, typ):
    """Case 11 on case 1's batches: _PnaStats, FuncToNode.finish and
    score_model under autograd against pna_forward_backward."""
    model, sd = world.model(typ, "pna", feature, dev)
    h, r, t, etr = world.rows(name)
    G = pr.upstream(len(h), world.E, 1)
    label = "pna %s %s/%s" % (name, typ, feature)
    c, want = reference(world, label, "pna", sd, feature, name, h, r, etr, G)
    check(label, run_model(model, h, r, etr, G, dev, query_r=int(r[0])), want, c, sd, feature)


def test_zz_print_figures():
    """The observed figures of this run, the worst over each group of cases
    (the table of the module docstring)."""
    groups = {}
    for label, fig in FIG.items():
        key = " ".join(label.split()[:2]) if label.split()[0] in ("sum", "pna") else label.split()[0]
        g = groups.setdefault(key, {})
        for n, v in fig.items():
            n = tpr.SHORT.get(n, "rule" if n.startswith(("rnn.", "vocab")) else n)
            g[n] = max(g.get(n, 0.0), v)
    for key in sorted(groups):
        print("%-14s " % key + "  ".join("%s %.1e" % (n, v) for n, v in groups[key].items()))
