"""The EM loop's training step — rnnlogic_amd/csrc/predictor.hip (node table,
scores, rule statistics, backward), loss.hip (the smoothed NLL and its
backward) and the small exact kernels of batch.hip — against the float64
reference of tests/em_ref.py, whose grounding is the CPU oracle's, on the
graph of em_ref.graph (plus_ref.small_graph with a 300-leaf star, |E| = 773):
Predictor(graph, entity_feature) with em_ref.weights / em_ref.bias copied in,
driven through forward_rows, forward (eval and, in train mode,
_PredictorLinear with the test's own upstream gradient G), forward_autograd,
compute_H, compute_H_rows, _rule_stats and _SmoothedNLL.

Bounds.  Scores, rule gradients and bias gradients: the a-priori formulas of
em_ref's docstring (the kernels' stated arithmetic, in float64 from the
reference's own quantities).  H, the loss, its gradient and the chained step:
16 x the float32-against-float64 error of the same formulas on the very input
(tests/test_em_ref.py measures and tables them), never looser than what the
older tests assert.  Exact where the operation is a selection or an integer:
masks, candidate counts, pos / tot, ranks, batches, the scores of an all-zero
table, every gradient under an all-zero G.  No case is skipped or masked.

Cases: see each test's docstring.  test_zz_print_figures prints the observed
maxima of the run at hand; DESIGN.md §5 records those of an MI355X.

Found by these tests, and fixed: the LDS-table check of
rnnl_predictor_rule_stats / rnnl_predictor_backward counted a head's root and
refused 8,192 bodies in one head, which the table can hold; forward_autograd
summed in fp32 (a rule gradient 7.7e-7 off where one rounding allows 5.2e-7);
compute_H_rows added the rows' softmax with fp32 atomics (4.6e-3 off at 345
over 4,136 rows, bound 6.5e-4).
"""
import random

import numpy as np
import pytest
import torch

import em_ref as em
import plus_ref as pr
import test_em_ref as ter

pytestmark = pytest.mark.gpu

FIG = {}  # group -> {quantity: (observed max, its bound)}, printed by test_zz_print_figures


def note(group, quantity, err, bound):
    old = FIG.setdefault(group, {}).get(quantity, (-1.0, 0.0))
    if err > old[0]:
        FIG[group][quantity] = (float(err), float(bound))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


class GpuWorld(ter.World):
    def __init__(self, root):
        super().__init__(root)
        from rnnlogic_amd.data import KnowledgeGraph
        self.graph = KnowledgeGraph(self.sg["path"])
        self._model = {}

    def model(self, feature, kind, dev, wide=None):
        """(Predictor on dev, rule_weights, bias as float32 numpy): one model
        per (feature, rules file), the weights of `kind` copied in."""
        from rnnlogic_amd.predictors import Predictor
        key = (feature, wide)
        if key not in self._model:
            m = Predictor(self.graph, entity_feature=feature)
            m.set_rules(self.sg["rules"] if wide is None else self.wide(wide)[0])
            self._model[key] = m.to(dev)
        m = self._model[key]
        rules = self.rules if wide is None else self.wide(wide)[1]
        w, b = em.weights(rules, kind), em.bias(self.E)
        with torch.no_grad():
            m.rule_weights.copy_(torch.from_numpy(w))
            if feature == "bias":
                m.bias.copy_(torch.from_numpy(b))
        return m, w, b

    def nodes(self, wide=None):
        return self.node if wide is None else self.wide(wide)[2]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return GpuWorld(tmp_path_factory.mktemp("em_gpu"))


def to_dev(dev, *arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def table_shift(model, dev):
    """The fixed-point shift of the Predictor's node table (trailer word 1)."""
    tab = model.node_weights(dev)
    off = (model.native_rules(dev).n_nodes * 4 + 15) & ~15
    torch.cuda.synchronize()
    return int(tab[off:off + 16].cpu().numpy().view(np.int32)[1])


def cand_mask(c):
    cand = np.zeros((c["nq"], c["E"]), dtype=bool)
    cand[c["row"], c["ent"]] = True
    return cand


# --------------------------------------------------------------------------- forward
FWD_SETS = ["A1", "A33", "B33", "stars", "star300", "star300x2", "mixed", "tile94"]


def check_forward(world, dev, model, w, b, feature, kind, name, removed, wide=None):
    h, r, t, etr = world.rows(name)
    c = world.coo(name, removed, wide)
    th, tr, te = to_dev(dev, h, r, etr if removed else None)
    label = "%s %s %s%s" % (name, feature, kind, "" if removed else " kept")
    with torch.no_grad():
        score, mask, n_cand = model.forward_rows(th, tr, te, return_ncand=True)
        if len(set(r.tolist())) == 1:  # Predictor.forward: one relation per batch
            s1, m1 = model(th, tr, te)
            assert torch.equal(s1, score) and torch.equal(m1, mask), label
    score, mask, n_cand = score.cpu().numpy(), mask.cpu().numpy(), n_cand.cpu().numpy()
    cand = cand_mask(c)
    assert np.array_equal(n_cand, np.bincount(c["row"], minlength=len(h))), label
    if feature == "none":
        assert np.array_equal(mask, cand), label
        assert np.all(score[~cand] == -np.inf), label
    else:
        assert mask.all(), label
        assert np.array_equal(score[~cand], np.broadcast_to(b, score.shape)[~cand]), label
    base = b if feature == "bias" else None
    got = score[c["row"], c["ent"]]
    if kind == "zero":
        assert np.array_equal(got, b[c["ent"]] if feature == "bias" else np.zeros(len(got), np.float32)), label
    want, bound = em.scores(c, w, base), em.score_bound(c, w, base, world.nodes(wide))
    err = np.abs(got.astype(np.float64) - want)
    k, top = int(np.argmax(err)), float(np.abs(want).max())
    note("forward %s %s" % (kind, feature), "score", err[k] / (top or 1.0), bound[k] / (top or 1.0))
    k = int(np.argmax(err - bound))
    assert (err <= bound).all(), (label, float(err[k]), float(bound[k]))


@pytest.mark.parametrize("kind", em.KINDS)
@pytest.mark.parametrize("feature", ["bias", "none"])
def test_forward(world, dev, feature, kind):
    """lin_node_kernel, lin_fix_kernel and score_linear_kernel: the mask,
    n_cand, the non-candidates (exactly the bias, or -inf) and the candidates'
    scores within the a-priori bound, with and without the removed edge, for
    one to 300 candidates per row (five chunks), mixed relations and 4,136
    rows (more chunks than 4 x the grid's waves); the table's one shift for an
    all-zero table, weights x 2^-40 (the shift caps at 60), head A x 2^12
    against the other heads, and a node whose two member rules cancel."""
    model, w, b = world.model(feature, kind, dev)
    model.eval()
    assert table_shift(model, dev) == em.table_shift(w, world.node)
    if kind == "tiny":
        assert em.table_shift(w, world.node) == 60
    if kind == "zero":
        assert em.table_shift(w, world.node) == 30
    if kind == "cancel":
        dup = [i for i, (hd, body) in enumerate(world.rules.rules) if hd == pr.REL["B"] and body == [pr.REL["r1"]]]
        assert em.node_sums(w, world.node)[world.node[dup[0]]] == 2.0 ** -20
    for name in FWD_SETS:
        for removed in (True, False):
            check_forward(world, dev, model, w, b, feature, kind, name, removed)


# --------------------------------------------------------------------------- backward
BW_SETS = ["A1", "A33", "B33", "stars", "star300", "tile94B", "tile94D"]
G_KINDS = ["dense", "one", "noncand", "zero", "x2^-60", "x2^-130", "x2^40"]


def upstream(kind, c, seed):
    """The test's upstream gradient (nq, E) float32: plus_ref.upstream dense;
    at one candidate per row; at non-candidates only; all zero; dense x 2^-60,
    x 2^-130 (fp32 denormals), x 2^40."""
    G = pr.upstream(c["nq"], c["E"], seed).astype(np.float64)
    cand = cand_mask(c)
    if kind == "one":
        first = np.unique(c["row"], return_index=True)[1]
        keep = np.zeros_like(cand)
        keep[c["row"][first], c["ent"][first]] = True
        G[~keep] = 0
    elif kind == "noncand":
        G[cand] = 0
    elif kind == "zero":
        G[:] = 0
    elif kind.startswith("x2^"):
        G *= 2.0 ** int(kind[3:])
    else:
        assert kind == "dense", kind
    return G.astype(np.float32)


def run_backward(model, dev, rows, G, between=None, coo_path=False):
    """(d rule_weights or None, d bias) as numpy of forward() in train mode
    (_PredictorLinear) — or forward_autograd — and score.backward(gradient=G);
    between: rows of an unrelated forward run before the backward."""
    h, r, t, etr = rows
    th, tr, te, tG = to_dev(dev, h, r, etr, G)
    model.train()
    model.zero_grad(set_to_none=True)
    score, mask = model.forward_autograd(th, tr, te) if coo_path else model(th, tr, te)
    if between is not None:
        with torch.no_grad():
            model.forward_rows(*to_dev(dev, between[0], between[1], between[3]))
    score.backward(gradient=tG)
    torch.cuda.synchronize()
    gw = model.rule_weights.grad
    return (None if gw is None else gw.detach().cpu().numpy().copy()), model.bias.grad.detach().cpu().numpy().copy()


def check_grads(label, group, got, c, G, rules, node, finite_rules=None, finite_cols=None):
    """Rule and bias gradients against float64 within the a-priori bounds;
    the rules of other heads exactly 0.  finite_*: the entries the reference
    keeps finite (all by default)."""
    gw, gb = got
    n_rules = len(rules.rules)
    with np.errstate(invalid="ignore"):
        w64, b64 = em.rule_grads(c, G, n_rules)
    heads = np.asarray([hd for hd, _ in rules.rules])
    live = np.isin(heads, np.unique(heads[c["rule"]]))
    assert not gw[~live].any(), label
    fr = np.ones(n_rules, bool) if finite_rules is None else finite_rules
    fc = np.ones(len(gb), bool) if finite_cols is None else finite_cols
    Gf = np.where(np.isfinite(G), G, 0).astype(np.float32)
    wb = em.rule_grad_bound(c, G, node, np.where(fr, w64, 0))
    with np.errstate(invalid="ignore"):  # inf - inf where both are non-finite: not among the compared entries
        err = np.abs(gw.astype(np.float64) - w64)
        errb = np.abs(gb.astype(np.float64) - b64)
    top = (float(np.abs(w64[fr]).max()) if fr.any() else 0.0) or 1.0
    k = int(np.argmax(np.where(fr, err, -np.inf)))
    note(group, "rule", err[k] / top, wb[k] / top)
    k = int(np.argmax(np.where(fr, err - wb, -np.inf)))
    assert np.isfinite(gw[fr]).all() and (err[fr] <= wb[fr]).all(), (label, float(err[k]), float(wb[k]))
    bb = em.bias_grad_bound(Gf)
    topb = float(np.abs(b64[fc]).max()) or 1.0
    k = int(np.argmax(np.where(fc, errb, -np.inf)))
    note(group, "bias", errb[k] / topb, bb[k] / topb)
    k = int(np.argmax(np.where(fc, errb - bb, -np.inf)))
    assert np.isfinite(gb[fc]).all() and (errb[fc] <= bb[fc]).all(), (label, float(errb[k]), float(bb[k]))
    return w64, b64


@pytest.mark.parametrize("gkind", G_KINDS)
@pytest.mark.parametrize("name", BW_SETS)
def test_backward(world, dev, name, gkind):
    """predictor_bw_stats_kernel, predictor_backward_kernel and
    predictor_bw_fix_kernel under the test's own upstream gradient: rule and
    bias gradients within the a-priori bounds of float64, exact zeros for the
    other heads' rules, for a zero G and for a G at non-candidates only; the
    same bytes from a second run and from a run whose workspace an unrelated
    forward reused before the backward (ground again); forward_autograd (the
    COO path) within the same bounds.  One to 2,068 rows, one to 300
    candidates per row (two 256-thread passes)."""
    model, w, b = world.model("bias", "normal", dev)
    rows, c = world.rows(name), world.coo(name)
    G = upstream(gkind, c, 11)
    label = "%s %s" % (name, gkind)
    got = run_backward(model, dev, rows, G)
    assert got[0] is not None, label  # the batch has candidates: a tensor, also under a zero G
    check_grads(label, "backward " + gkind, got, c, G, world.rules, world.node)
    if gkind in ("zero", "noncand"):
        assert not got[0].any(), label
    if gkind == "zero":
        assert not got[1].any(), label
    again = run_backward(model, dev, rows, G)
    assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes(), label
    reground = run_backward(model, dev, rows, G, between=world.rows("A1"))
    assert reground[0].tobytes() == got[0].tobytes() and reground[1].tobytes() == got[1].tobytes(), label
    auto = run_backward(model, dev, rows, G, coo_path=True)
    check_grads(label + " coo", "coo path " + gkind, auto, c, G, world.rules, world.node)


@pytest.mark.parametrize("value", [np.nan, np.inf])
@pytest.mark.parametrize("name", ["A33", "stars"])
def test_backward_nonfinite(world, dev, name, value):
    """One NaN, one +inf in G at a candidate: a rule's gradient
    is non-finite exactly where the rule has a non-zero count at that
    candidate — what torch autograd on the COO yields —, the other rules keep
    their float64 value within the bound, the entity's bias column is
    non-finite; the fused kernel and forward_autograd agree."""
    model, w, b = world.model("bias", "normal", dev)
    rows, c = world.rows(name), world.coo(name)
    G = upstream("dense", c, 12)
    k = len(c["ent"]) // 2
    G[c["row"][k], c["ent"][k]] = value
    hit = np.zeros(len(w), bool)
    hit[c["rule"][c["ce"] == k]] = True
    assert hit.any() and not hit.all()
    cols = np.ones(world.E, bool)
    cols[c["ent"][k]] = False
    for coo_path in (False, True):
        label = "%s %s %s" % (name, value, "coo" if coo_path else "fused")
        gw, gb = run_backward(model, dev, rows, G, coo_path=coo_path)
        assert np.array_equal(~np.isfinite(gw), hit), (label, int((~np.isfinite(gw)).sum()), int(hit.sum()))
        assert np.array_equal(~np.isfinite(gb), ~cols), label
        if np.isnan(value):
            assert np.isnan(gw[hit]).all() and np.isnan(gb[~cols]).all(), label
        else:
            assert (gw[hit] == np.inf).all() and (gb[~cols] == np.inf).all(), label
        check_grads(label, "backward non-finite", (gw, gb), c, G, world.rules, world.node, ~hit, cols)


# --------------------------------------------------------------------------- E-step
def check_rule_stats(label, world, dev, model, name, wide=None):
    h, r, t, etr = world.rows(name)
    c = world.coo(name, True, wide)
    rules = world.rules if wide is None else world.wide(wide)[1]
    roots, ld = model.head_roots(dev)
    pos, tot, n_cand = model._rule_stats(*to_dev(dev, h, r, t, etr), ld)
    torch.cuda.synchronize()
    assert pos.dtype == torch.int64 and tot.dtype == torch.int64
    pos, tot, n_cand = pos.cpu().numpy(), tot.cpu().numpy(), n_cand.cpu().numpy()
    wpos, wtot, wn = em.rule_stats(c, len(rules.rules), t)
    assert np.array_equal(n_cand, wn), label
    n2r = model.native_rules(dev).node_of_rule.cpu().numpy()
    for q in np.unique(r):
        idx = np.asarray([i for i, _ in rules.relation2rules[int(q)]], dtype=np.int64)
        sel = np.nonzero(r == q)[0]
        if len(idx):
            k = n2r[idx] - roots[int(q)]
            assert np.array_equal(pos[np.ix_(sel, k)], wpos[np.ix_(sel, idx)]), (label, int(q))
            assert np.array_equal(tot[np.ix_(sel, k)], wtot[np.ix_(sel, idx)]), (label, int(q))
        else:
            assert not pos[sel].any() and not tot[sel].any(), (label, int(q))


@pytest.mark.parametrize("kind", ter.H_KINDS)
@pytest.mark.parametrize("name", ter.H_SETS)
def test_e_step(world, dev, name, kind):
    """rule_stats_kernel: pos / tot as int64 exactly em_ref.rule_stats, and
    n_cand; then compute_H per one-relation batch and compute_H_rows (one
    launch, and chunk=7) against float64 within 16 x e32.  Rows with 1 - 300
    candidates (two 256-thread passes), without any, with the tail outside
    the candidates (8 of mixed's 24), a head without rules ((None, None)),
    4,136 rows (a second trip of the 4,096-workgroup grid), one row three
    times, all_t given on the CPU, 8,192 nodes in one head.  Zero weights:
    every row adds exactly 1 / n_rules to each of its relation's rules."""
    wide = 8192 if name == "wide" else None
    model, w, b = world.model("bias", kind, dev, wide)
    model.eval()
    rules = world.rules if wide is None else world.wide(wide)[1]
    h, r, t, etr = world.rows(name)
    c = world.coo(name, True, wide)
    label = "H %s %s" % (name, kind)
    check_rule_stats(label, world, dev, model, name, wide)
    want, bound = ter.measure_H(label, c, w, rules, r, t)
    th, tr, tt, te = to_dev(dev, h, r, t, etr)
    got_rows = model.compute_H_rows(th, tr, tt, te).cpu().numpy()
    chunked = model.compute_H_rows(th, tr, tt, te, chunk=7).cpu().numpy() if len(h) <= 64 else None
    if want is None:
        assert model.compute_H(th, tr, tt, te) == (None, None), label
        assert model.compute_H(th, tr, tt.cpu(), te) == (None, None), label
        assert not got_rows.any() and not chunked.any(), label
        return
    results = [("rows", got_rows)] + ([("chunk 7", chunked)] if chunked is not None else [])
    if len(set(r.tolist())) == 1:
        for tag, t_in in (("batch", tt), ("batch, all_t on the CPU", tt.cpu())):
            Hq, index = model.compute_H(th, tr, t_in, te)
            assert index.cpu().tolist() == [i for i, _ in rules.relation2rules[int(r[0])]], label
            full = np.zeros(len(w), np.float32)
            full[index.cpu().numpy()] = Hq.cpu().numpy()
            results.append((tag, full))
    for tag, got in results:
        err = float(np.abs(got.astype(np.float64) - want).max())
        note("H " + kind, name, err, bound)
        assert err <= bound, (label, tag, err, bound)
        if kind == "zero":
            for q in np.unique(r):
                idx = [i for i, _ in rules.relation2rules[int(q)]]
                if idx:
                    assert len(set(got[idx].tolist())) == 1, (label, tag)
                    if (r == q).sum() == 1:
                        assert got[idx[0]] == np.float32(1.0 / len(idx)), (label, tag)


# --------------------------------------------------------------------------- the table limit
def test_table_limit(world, dev):
    """8,192 rule-bearing nodes in one head (64 KB of LDS slots: the root,
    where no rule ends, has none): forward, backward and compute_H run and
    pass the bounds (compute_H: test_e_step[wide]).  One node more: compute_H
    and the backward raise the library's error before any launch."""
    from rnnlogic_amd import _native
    model, w, b = world.model("bias", "normal", dev, 8192)
    assert model.head_roots(dev)[1] == 8193  # with the root
    model.eval()
    assert table_shift(model, dev) == em.table_shift(w, world.nodes(8192))
    check_forward(world, dev, model, w, b, "bias", "normal", "wide", True, 8192)
    rows, c = world.rows("wide"), world.coo("wide", True, 8192)
    G = upstream("dense", c, 13)
    rules, node = world.wide(8192)[1], world.nodes(8192)
    got = run_backward(model, dev, rows, G)
    check_grads("wide dense", "backward wide", got, c, G, rules, node)
    check_grads("wide dense coo", "backward wide", run_backward(model, dev, rows, G, coo_path=True), c, G, rules, node)
    big, w_big, b_big = world.model("bias", "normal", dev, 8193)
    assert big.head_roots(dev)[1] == 8194
    th, tr, tt, te, tG = to_dev(dev, *rows, G)
    big.eval()
    with pytest.raises(_native.NativeError, match="head trie too large for the LDS table"):
        big.compute_H(th, tr, tt, te)
    with pytest.raises(_native.NativeError, match="head trie too large for the LDS table"):
        big.compute_H_rows(th, tr, tt, te)
    big.train()
    score, mask = big(th, tr, te)
    with pytest.raises(_native.NativeError, match="head trie too large for the LDS table"):
        score.backward(gradient=tG)
    torch.cuda.synchronize()
    # the forward has no such table: it still scores the 8,193 bodies
    check_forward(world, dev, big.eval(), w_big, b_big, "bias", "normal", "wide", True, 8193)


# --------------------------------------------------------------------------- the loss
def run_nll(dev, x, target, all_t, smoothing, c):
    from rnnlogic_amd.trainer import _SmoothedNLL
    tx, tt, ta = to_dev(dev, x, target, all_t)
    tx.requires_grad_(True)
    loss = _SmoothedNLL.apply(tx, tt, ta, smoothing)
    (loss * c).backward()
    torch.cuda.synchronize()
    return loss.item(), tx.grad.cpu().numpy()


def check_nll(label, group, got, want):
    loss, grad = got
    l64, g64, lb, gb = want
    if np.isfinite(l64):
        note(group, "loss", abs(loss - l64), lb)
        assert abs(loss - l64) <= lb, (label, loss, l64, lb)
    else:
        assert np.isnan(loss) and np.isnan(l64), (label, loss, l64)
    ok = np.isfinite(gb)
    assert np.isfinite(grad[ok]).all(), label
    err = np.where(ok, np.abs(grad.astype(np.float64) - np.where(ok, g64, 0)), 0)
    top = ter.finite_max(g64[ok]) or 1.0
    k = np.unravel_index(int(np.argmax(err)), err.shape)
    note(group, "gradient", err[k] / top, gb[k] / top)
    k = np.unravel_index(int(np.argmax(np.where(ok, err - gb, -np.inf))), err.shape)
    assert (err[ok] <= gb[ok]).all(), (label, k, float(err[k]), float(gb[k]))


@pytest.mark.parametrize("smoothing", ter.LOSS_SMOOTHING)
@pytest.mark.parametrize("B,E", ter.LOSS_SHAPES)
def test_loss(dev, B, E, smoothing):
    """nll_forward_kernel / nll_backward_kernel against trainer.py:84-90 in
    float64 with autograd: E below, at and past the 64-lane wave and the
    1,024-lane workgroup, smoothing 0 / 0.2 / 1, a row with its mass on five
    entities, a row spread over +-100, -inf logits, an empty target row, a row
    whose only target is all_t; the upstream factor 1.5, 2^-40, 2^30 and 0."""
    x, target, all_t = ter.loss_input(B, E)
    for c in ter.LOSS_C:
        label = "loss %dx%d s%g c%g" % (B, E, smoothing, c)
        want = ter.measure_nll(label, x, target, all_t, smoothing, c)
        got = run_nll(dev, x, target, all_t, smoothing, c)
        check_nll(label, "loss %dx%d" % (B, E), got, want)
        if c == 0:
            assert not got[1].any(), label


@pytest.mark.parametrize("name", ["clamp", "zero1", "zero3"])
def test_loss_small_target_sum(dev, name):
    """T = max(sum target', 1) in its clamped branch (B = 1, smoothing 0.5, an
    empty target: T = 0.5 -> 1); smoothing 1 and empty targets: the loss and
    every gradient entry exactly 0."""
    x, target, all_t, s = ter.loss_special(name)
    want = ter.measure_nll("loss " + name, x, target, all_t, s, 1.5)
    got = run_nll(dev, x, target, all_t, s, 1.5)
    check_nll("loss " + name, "loss " + name, got, want)
    if name == "clamp":
        # the unclamped T = 0.5 would double the loss
        assert abs(got[0] - want[0]) < 0.25 * abs(want[0])
    else:
        assert got[0] == 0 and not got[1].any()


@pytest.mark.parametrize("poison", ["nan", "inf"])
@pytest.mark.parametrize("B,E", ter.LOSS_POISON)
def test_loss_nonfinite_logit(dev, B, E, poison):
    """One NaN, one +inf logit: the loss is NaN, that row's gradient is NaN,
    the other rows' gradients equal float64 torch's within the bound."""
    x, target, all_t = ter.loss_input(B, E, poison)
    others = [0] + list(range(2, B))
    label = "loss %dx%d %s" % (B, E, poison)
    want = ter.measure_nll(label, x, target, all_t, 0.2, 1.5, rows=others)
    assert np.isnan(want[0]) and np.isnan(want[1][1]).all() and np.isfinite(want[1][others]).all()
    got = run_nll(dev, x, target, all_t, 0.2, 1.5)
    assert np.isnan(got[0]) and np.isnan(got[1][1]).all(), label
    check_nll(label, "loss non-finite", got, want)


def test_loss_counter_across_batch_sizes(dev):
    """The `done` counter of nll_forward_kernel across launches of B = 5, 3, 5
    on one device: each result is its isolated launch's (a fresh counter) bit
    for bit."""
    from rnnlogic_amd.trainer import _SmoothedNLL
    inputs = [ter.loss_input(B, 135 + k) for k, B in enumerate((5, 3, 5))]
    alone = []
    for x, target, all_t in inputs:
        _SmoothedNLL._counters.clear()
        alone.append(run_nll(dev, x, target, all_t, 0.2, 1.5))
    _SmoothedNLL._counters.clear()
    for (x, target, all_t), (l0, g0) in zip(inputs, alone):
        loss, grad = run_nll(dev, x, target, all_t, 0.2, 1.5)
        assert np.float32(loss).tobytes() == np.float32(l0).tobytes() and grad.tobytes() == g0.tobytes()
    assert len(_SmoothedNLL._counters) == 1 and int(next(iter(_SmoothedNLL._counters.values())).item()) == 0


# --------------------------------------------------------------------------- the whole step
@pytest.mark.parametrize("name", ter.STEP_SETS)
def test_whole_step(world, dev, name):
    """forward() in train mode -> _SmoothedNLL -> backward, as
    TrainerPredictor.train_step runs it: the loss, rule_weights.grad and
    bias.grad against em_ref.step in float64 within 16 x the chain's e32."""
    from rnnlogic_amd.trainer import _SmoothedNLL
    model, w, b = world.model("bias", "normal", dev)
    h, r, t, etr = world.rows(name)
    target = world.target(name)
    (l64, gw64, gb64), (lb, wb, bb) = ter.measure_step("step " + name, world.coo(name), w, b, target, t,
                                                       ter.STEP_SMOOTHING)
    th, tr, tt, te, ttarget = to_dev(dev, h, r, t, etr, target)
    model.train()
    model.zero_grad(set_to_none=True)
    logits, mask = model(th, tr, te)
    loss = _SmoothedNLL.apply(logits, ttarget, tt, ter.STEP_SMOOTHING)
    loss.backward()
    torch.cuda.synchronize()
    gw, gb = model.rule_weights.grad.cpu().numpy(), model.bias.grad.cpu().numpy()
    errs = (abs(loss.item() - l64), float(np.abs(gw - gw64).max()), float(np.abs(gb - gb64).max()))
    note("step " + name, "loss", errs[0], lb)
    note("step " + name, "rule", errs[1] / np.abs(gw64).max(), wb / np.abs(gw64).max())
    note("step " + name, "bias", errs[2] / np.abs(gb64).max(), bb / np.abs(gb64).max())
    assert errs[0] <= lb and errs[1] <= wb and errs[2] <= bb, (name, errs, (lb, wb, bb))
    heads = np.asarray([hd for hd, _ in world.rules.rules])
    assert not gw[heads != int(r[0])].any()


# --------------------------------------------------------------------------- the exact kernels
@pytest.mark.parametrize("n", [1, 7])
@pytest.mark.parametrize("E", [1, 2, 255, 256, 257, 1025])
def test_filtered_ranks(dev, E, n):
    """filtered_ranks_kernel against em_ref.ranks (trainer.py:191-203): widths
    around the 256-lane workgroup; randn, 8 distinct values, all equal, +-0,
    +-inf, NaN at the target, NaN at competitors, flag all False, flag False
    at the target, mask False at the target ((1, E + 1))."""
    from rnnlogic_amd.trainer import TrainerPredictor
    for k, kind in enumerate(ter.RANK_KINDS):
        s, mask, flag, all_t = ter.rank_input(kind, n, E, 1000 + 16 * E + k)
        L, H = TrainerPredictor.filtered_ranks(*to_dev(dev, s, mask, flag, all_t), E)
        wL, wH = em.ranks(s, mask, flag, all_t)
        assert L.dtype == torch.int64 and np.array_equal(L.cpu().numpy(), wL), (kind, E, n)
        assert np.array_equal(H.cpu().numpy(), wH), (kind, E, n)
        if kind == "mask_t":
            assert wL.tolist() == [1] * n and wH.tolist() == [E + 1] * n


@pytest.mark.parametrize("batch_size", [1, 32])
def test_device_batches(world, dev, batch_size):
    """train_batch_kernel and multi_hot_kernel through DeviceTrainBatches /
    DeviceEvalBatches on em_ref.graph (a 300-entry hr2o list: longer than a
    workgroup; the first and the last key of the table; |E| = 773): every
    batch equals Train / Valid / TestDataset.__getitem__, rows() over all
    batches their concatenation."""
    from rnnlogic_amd.data import (DeviceEvalBatches, DeviceTrainBatches, TestDataset, TrainDataset, ValidDataset)
    g = world.graph
    keys = sorted(g.hr2o)
    assert max(len(v) for v in g.hr2o.values()) == 300 and g.entity_size == 773
    random.seed(5)
    ts = TrainDataset(g, batch_size)
    seen = {int(r) * g.entity_size + int(h) for b in ts.batches for h, r, _ in b}
    assert keys[0] in seen and keys[-1] in seen
    dtb = DeviceTrainBatches(ts, dev)
    assert len(dtb) == len(ts)
    parts = []
    for i in range(len(ts)):
        want, got = ts[i], dtb[i]
        for a, b in zip(want, got):
            assert a.dtype == b.dtype and torch.equal(a, b.cpu()), (batch_size, i)
        parts.append(want)
    h, r, t, etr = dtb.rows(range(len(ts)))
    for k, x in zip((0, 1, 2, 4), (h, r, t, etr)):
        assert torch.equal(torch.cat([p[k] for p in parts]), x.cpu()), (batch_size, k)
    for cls in (ValidDataset, TestDataset):
        es = cls(g, batch_size)
        deb = DeviceEvalBatches(es, dev)
        assert len(deb) == len(es) > 0
        for i in range(len(es)):
            for a, b in zip(es[i], deb[i]):
                assert a.dtype == b.dtype and torch.equal(a, b.cpu()), (cls.__name__, i)
        for a, b in zip([torch.cat([es[i][k] for i in range(len(es))]) for k in range(4)],
                        deb.rows(range(len(es)))):
            assert torch.equal(a, b.cpu()), cls.__name__


@pytest.mark.parametrize("width", [1, 255, 257])
def test_multi_hot_lists(dev, width):
    """rnnl_multi_hot / rnnl_filter_flags on a hand-made CSR against a numpy
    loop: a missing key (between two keys, before the first, past the last),
    an empty list, a list with a repeated value, a list longer than a
    workgroup, a key repeated in two rows."""
    from rnnlogic_amd import _native
    rng = np.random.default_rng(width)
    lists = {3: [0], 10: [], 11: [width - 1, 0, width - 1, width // 2, 0],
             40: rng.integers(0, width, 700).tolist(), 41: list(range(width))}
    keys = np.asarray(sorted(lists), dtype=np.int64)
    offs = np.zeros(len(keys) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(lists[int(k)]) for k in keys])
    vals = np.asarray([v for k in keys for v in lists[int(k)]], dtype=np.int32)
    row_keys = np.asarray([11, 3, 5, 10, 40, 11, 0, 99, 41, 40], dtype=np.int64)
    tk, to, tv, tr = to_dev(dev, keys, offs, vals, row_keys)
    stream = torch.cuda.current_stream(dev).cuda_stream
    hot = torch.full((len(row_keys), width), 7.0, dtype=torch.float32, device=dev)
    flags = torch.full((len(row_keys), width), 7, dtype=torch.uint8, device=dev)
    for fn, out in (("rnnl_multi_hot", hot), ("rnnl_filter_flags", flags)):
        _native.call(fn, tk.data_ptr(), to.data_ptr(), tv.data_ptr(), len(keys), tr.data_ptr(), len(row_keys), width,
                     out.data_ptr(), stream)
    torch.cuda.synchronize()
    want = np.zeros((len(row_keys), width), dtype=np.float32)
    for i, k in enumerate(row_keys.tolist()):
        for v in lists.get(k, []):
            want[i, v] = 1
    assert np.array_equal(hot.cpu().numpy(), want)
    assert np.array_equal(flags.cpu().numpy(), (1 - want).astype(np.uint8))


# --------------------------------------------------------------------------- figures
def test_zz_print_figures():
    """The observed maxima of this run per case group (the table of DESIGN.md
    §5's bullet): error / max |ref| for scores and gradients, absolute for H
    and the loss, each beside the bound of the entry where it was observed."""
    for group in sorted(FIG):
        print("    %-28s " % group + "  ".join("%s %.1e (%.1e)" % (q, e, bnd) for q, (e, bnd) in FIG[group].items()))
    assert FIG
