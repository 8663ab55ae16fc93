"""tests/em_ref.py (numpy / torch.float64 on the CPU grounding) checked, and the
measured bounds of tests/test_gpu_em_step.py.

* em_ref's scores and H in float64 equal oracle/reference_np.predictor_forward
  / predictor_compute_H (fp32 numpy, the dense restatement pinned to the
  reference's fixtures) on the small graph within that oracle's own 1e-5:
  sets A5, B5, stars and D rows, bias and none, with and without the removed
  edge.
* em_ref.ranks equals a literal loop transcription of trainer.py:191-203 on
  200 random small rows (ties, NaN, +-inf, +-0, flags and masks included).
* plus_ref.small_graph's default output is byte for byte what it was before it
  took `stars`; the 300-star row has exactly 300 candidates; the wide_rules
  files have 8,192 and 8,193 distinct (head A, body) nodes.
* measure_H / measure_nll / measure_step: the float32 formulas against float64
  for the very input of each GPU case.  A GPU bound of these quantities is
  FACTOR = 16 x that measurement (the project's margin in
  test_gpu_plus_grad.py: four bits for the GPU's libm and summation order
  against the CPU's), never looser than what the older tests assert
  (H 1e-5 per 32 rows; loss 2e-6 relative; loss gradient rtol 1e-4, atol 1e-6 max |g|), a
  gradient tensor's never below 2^-20 of its float64 maximum.  The loss's
  relative cap is taken of max(|loss|, sum target' / T): log(p + 1e-8) is off
  by 2^-24 in absolute terms whatever its size (the fp32 rounding of p +
  1e-8), so a loss far below one nat per unit of target — B = E = 1, where
  p = 1 and the float64 loss is -1e-8 — has no relative fp32 accuracy.

Recorded e32 (torch 2.x CPU; H: max |f32 - f64|; loss: |f32 - f64|; loss
gradient, d rule_weights, d bias: max |f32 - f64| / max |f64|; the worst of a
group's cases; test_measured_table prints the rows of the torch at hand):

    H A33 normal           H 2.1e-08
    H A33 zero             H 1.3e-09
    H A3same normal        H 8.9e-10
    H A3same zero          H 2.5e-10
    H mixed normal         H 1.3e-07
    H mixed zero           H 2.9e-11
    H star300 normal       H 5.0e-09
    H star300 zero         H 5.0e-09
    H stars normal         H 7.9e-08
    H stars zero           H 7.9e-08
    H tile94 normal        H 5.1e-05
    H tile94 zero          H 4.1e-05
    H wide normal          H 6.5e-10
    H wide zero            H 0.0e+00
    loss 1x1               loss 1.0e-08  loss_grad 0.0e+00
    loss 1x2               loss 5.0e-08  loss_grad 7.8e-08
    loss 2x1023            loss 9.5e-07  loss_grad 1.6e-07
    loss 2x1024            loss 2.6e-07  loss_grad 1.5e-06
    loss 2x1025            loss 2.6e-07  loss_grad 9.3e-07
    loss 300x135           loss 1.2e-06  loss_grad 2.8e-07
    loss 33x2049           loss 9.3e-07  loss_grad 2.9e-07
    loss 3x63              loss 8.6e-07  loss_grad 1.0e-06
    loss 3x64              loss 6.5e-07  loss_grad 8.3e-07
    loss 3x65              loss 1.0e-06  loss_grad 1.0e-07
    loss clamp             loss 1.3e-07  loss_grad 9.1e-07
    loss zero1             loss 0.0e+00  loss_grad 0.0e+00
    loss zero3             loss 0.0e+00  loss_grad 0.0e+00
    step A33               loss 4.0e-07  rule_weights 2.5e-07  bias 2.4e-07
    step star300           loss 2.7e-08  rule_weights 5.2e-07  bias 3.2e-08
    step stars             loss 2.6e-07  rule_weights 4.1e-07  bias 1.5e-07

(H C5: (None, None), nothing to measure.  A loss group is a shape over the
three smoothings, the four upstream factors and, for 3x65 and 33x2049, the NaN
and +inf logits, whose poisoned row is left out.  `H wide zero` is exact in
fp32 too: one row adds 2^-13 to each of 8,192 rules.)
"""
import hashlib
import os

import numpy as np
import pytest
import torch

import em_ref as em
import plus_ref as pr
from oracle import reference_np as ref

FACTOR, GRAD_FLOOR = 16.0, 2.0 ** -20
H_CAP, LOSS_CAP, GRAD_RTOL, GRAD_ATOL = 1e-5, 2e-6, 1e-4, 1e-6
E32 = {}  # label -> {quantity: e32}, filled by the measure functions

SMALL_GRAPH_SHA256 = {
    "entities.dict": "7783d346241df4505cece03839a5bd5eb97032666881100de1190fca54fd11a9",
    "relations.dict": "e5c4d2df7f8d3c66872a461ee240154a06c4ccb2fecd5806c319f922a1b489d8",
    "rules.txt": "d59d72e542286fb9b556ba90d0524031ef7de051b4956710a13599f9070fb4f8",
    "test.txt": "440c215759cbf4f315a6384613f0b56349c0457782a1d6e8c3f5ae688379595a",
    "train.txt": "9a544a7a88d5ffd4b315b4f2b96dc948ba833e354027e11f91f0efa335a9ce9c",
    "valid.txt": "440c215759cbf4f315a6384613f0b56349c0457782a1d6e8c3f5ae688379595a",
}


# --------------------------------------------------------------------------- the shared world and its input sets
class World:
    """The graph of em_ref.graph, its rules, and the input sets of the CPU and
    the GPU tests with their reference COOs (grounded once, shared, never changed)."""
    TILE = 94

    def __init__(self, root):
        self.sg = em.graph(root)
        self.g = ref.Graph(self.sg["path"])
        self.E = self.g.entity_size
        self.rules = ref.Rules(self.sg["rules"], self.g.relation_size)
        self.node = pr.node_of_rule(self.rules)
        self._coo, self._wide = {}, {}

    def wide(self, n):
        """(rules file, reference_np.Rules, node_of_rule) of em_ref.wide_rules(n)."""
        if n not in self._wide:
            path = em.wide_rules(self.sg, n)
            rules = ref.Rules(path, self.g.relation_size)
            self._wide[n] = (path, rules, pr.node_of_rule(rules))
        return self._wide[n]

    def rows(self, name):
        """(h, r, t, etr) int64 of a set: plus_ref.SETS and
        star300 / star300x2   the 300-leaf centre once / twice
        D5 / C5               the first five facts of head D / C (C has no rule)
        A3same                one head-A row three times
        tile94                `tile` 94 times: 4,136 rows; tile94B / tile94D: its B / D rows
        wide                  one head-A row (for the wide_rules files)."""
        f = self.sg["facts"]
        if name in pr.SETS:
            return pr.batch(self.sg, self.g, name)
        if name in ("star300", "star300x2"):
            return pr.rows_of(self.g, [f["B"][len(em.STARS) - 1]] * (2 if name.endswith("x2") else 1))
        if name in ("D5", "C5"):
            return pr.rows_of(self.g, f[name[0]][:5])
        if name == "A3same":
            return pr.rows_of(self.g, [f["A"][2]] * 3)
        if name == "wide":
            return pr.rows_of(self.g, [f["A"][0]])
        base = self.rows("tile")
        if name in ("tileB", "tileD"):
            sel = base[1] == pr.REL[name[-1]]
            return tuple(a[sel] for a in base)
        if name.startswith("tile94"):
            return tuple(np.tile(a, self.TILE) for a in self.rows("tile" + name[6:]))
        raise KeyError(name)

    def coo(self, name, removed=True, wide=None):
        key = (name, removed, wide)
        if key not in self._coo:
            if name.startswith("tile94"):  # by offsetting the 44 rows' COO, not grounded again
                c = em.tile_coo(self.coo("tile" + name[6:], removed), self.TILE)
            elif name in ("tileB", "tileD"):
                c = em.select_rows(self.coo("tile", removed), np.nonzero(self.rows("tile")[1] == pr.REL[name[-1]])[0])
            else:
                h, r, t, etr = self.rows(name)
                rules = self.rules if wide is None else self.wide(wide)[1]
                c = pr.coo(self.g, rules, h, r, etr if removed else None)
            self._coo[key] = c
        return self._coo[key]

    def target(self, name):
        """TrainDataset.__getitem__'s multi-hot rows of hr2o (data.py:206-209), float32."""
        h, r, t, _ = self.rows(name)
        out = np.zeros((len(h), self.E), dtype=np.float32)
        for k in range(len(h)):
            out[k, self.g.hr2o[int(r[k]) * self.E + int(h[k])]] = 1
        return out


# the GPU cases of H, of the loss and of the whole step (the measured bounds)
H_SETS = ["A33", "stars", "star300", "mixed", "C5", "tile94", "A3same", "wide"]
H_KINDS = ["normal", "zero"]
STEP_SETS = ["A33", "stars", "star300"]
STEP_SMOOTHING = 0.2
LOSS_SHAPES = [(1, 1), (1, 2), (3, 63), (3, 64), (3, 65), (2, 1023), (2, 1024), (2, 1025), (33, 2049), (300, 135)]
LOSS_SMOOTHING = [0.0, 0.2, 1.0]
LOSS_C = [1.5, 2.0 ** -40, 2.0 ** 30, 0.0]
LOSS_POISON = [(3, 65), (33, 2049)]


def loss_input(B, E, poison=None):
    """(logits, target (B, E) float32, all_t (B,) int64) of a loss case.
    logits  randn x 6; row 0 has its mass on five entities (+40); row 1 is
            spread over +-100 (expf underflows); row 2 has -inf at a tenth of
            its entries, none of them all_t or a target.
    target  random multi-hot; row 0's only target is all_t; the last row of a
            batch of two or more is empty.
    poison  'nan' / 'inf': that value at logits[1, E // 3]."""
    rng = np.random.default_rng(B * 7 + E)
    x = (6 * rng.standard_normal((B, E))).astype(np.float32)
    x[0, :5] += 40
    all_t = rng.integers(0, E, B).astype(np.int64)
    target = (rng.random((B, E)) < max(0.001, 2.0 / E)).astype(np.float32)
    target[0] = 0
    target[0, all_t[0]] = 1
    if B >= 2:
        x[1] = rng.uniform(-100, 100, E).astype(np.float32)
        target[B - 1] = 0
    if B >= 3:
        off = (rng.random(E) < 0.1) & (target[2] == 0)
        off[all_t[2]] = False
        x[2, off] = -np.inf
    if poison:
        x[1, E // 3] = dict(nan=np.nan, inf=np.inf)[poison]
    return x, target, all_t


def loss_special(name):
    """(logits, target, all_t, smoothing): 'clamp' — B = 1, smoothing 0.5 and an
    empty target: T = 0.5 is clamped to 1; 'zero1' / 'zero3' — smoothing 1 and
    empty targets: the loss and every gradient entry are exactly 0."""
    B = 3 if name == "zero3" else 1
    x, target, all_t = loss_input(B, 65)
    return x, np.zeros_like(target), all_t, (0.5 if name == "clamp" else 1.0)


# --------------------------------------------------------------------------- measured bounds
def finite_max(a):
    a = np.abs(np.asarray(a, dtype=np.float64))
    a = a[np.isfinite(a)]
    return float(a.max()) if a.size else 0.0


def grad_bound(e32_rel, g64):
    return max(FACTOR * e32_rel, GRAD_FLOOR) * finite_max(g64)


def measure_H(label, c, w, rules, r, t):
    """(float64 H or None, the absolute bound min(16 e32, 1e-5 per 32 rows)):
    the older tests assert 1e-5 of batches of up to 32 rows, each row adding a
    softmax of sum 1; H over the 4,136 rows of tile94 reaches 1,034, where
    half an fp32 step alone is 6e-5."""
    h64 = em.H(c, w, rules, r, t, torch.float64)
    if h64 is None:
        return None, 0.0
    h32 = em.H(c, w, rules, r, t, torch.float32)
    e = float(np.abs(h32.astype(np.float64) - h64).max())
    E32[label] = {"H": e}
    return h64, min(FACTOR * e, H_CAP * max(1.0, c["nq"] / 32.0))


def loss_bound(e32_abs, loss64, target, all_t, smoothing):
    tt = float(em.smoothed_target(target, all_t, smoothing, torch.float64).sum())
    return min(FACTOR * e32_abs, LOSS_CAP * max(abs(loss64), tt / max(tt, 1.0)))


def measure_nll(label, logits, target, all_t, smoothing, c, rows=None):
    """(float64 loss, float64 gradient (B, E), loss bound, elementwise gradient
    bound (B, E)) of em_ref.nll; rows: the rows whose gradient is measured and
    bounded (all by default; the others get an infinite bound)."""
    l64, g64 = em.nll(logits, target, all_t, smoothing, c, torch.float64)
    l32, g32 = em.nll(logits, target, all_t, smoothing, c, torch.float32)
    sel = np.arange(len(g64)) if rows is None else np.asarray(rows, dtype=np.int64)
    top = finite_max(g64[sel])
    e_l = abs(l32 - l64) if np.isfinite(l64) else 0.0
    e_g = float(np.abs(g32[sel].astype(np.float64) - g64[sel]).max()) / top if top > 0 else 0.0
    E32[label] = {"loss": e_l, "loss_grad": e_g}
    gb = np.full(g64.shape, np.inf)
    gb[sel] = np.minimum(grad_bound(e_g, g64[sel]), GRAD_ATOL * top + GRAD_RTOL * np.abs(g64[sel]))
    lb = loss_bound(e_l, l64, target, all_t, smoothing) if np.isfinite(l64) else 0.0
    return l64, g64, lb, gb


def measure_step(label, c, w, b, target, all_t, smoothing):
    """(float64 (loss, d rule_weights, d bias), bounds (loss, d rule_weights, d bias: absolute))."""
    l64, gw64, gb64 = em.step(c, w, b, target, all_t, smoothing, torch.float64)
    l32, gw32, gb32 = em.step(c, w, b, target, all_t, smoothing, torch.float32)
    e = {"loss": abs(l32 - l64), "rule_weights": pr.rel_err(gw32, gw64), "bias": pr.rel_err(gb32, gb64)}
    E32[label] = e
    return (l64, gw64, gb64), (loss_bound(e["loss"], l64, target, all_t, smoothing),
                               grad_bound(e["rule_weights"], gw64), grad_bound(e["bias"], gb64))


# --------------------------------------------------------------------------- tests
@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return World(tmp_path_factory.mktemp("em"))


def test_graph_and_wide_rules(world, tmp_path):
    sg = pr.small_graph(tmp_path, 0)
    assert sorted(os.listdir(sg["path"])) == sorted(SMALL_GRAPH_SHA256)
    for fn, want in SMALL_GRAPH_SHA256.items():
        with open(os.path.join(sg["path"], fn), "rb") as f:
            assert hashlib.sha256(f.read()).hexdigest() == want, fn
    assert os.path.basename(world.sg["path"]) != os.path.basename(sg["path"])
    assert world.E == 773
    # the same random part: the old graph's facts of heads A and C, its core edges
    assert world.sg["facts"]["A"] == sg["facts"]["A"] and world.sg["facts"]["C"] == sg["facts"]["C"]
    c = world.coo("star300")
    assert c["nq"] == 1 and len(c["ent"]) == 300
    h, r, t, etr = world.rows("star300")
    assert len(world.g.hr2o[pr.REL["r1"] * world.E + int(h[0])]) == 300  # the centre's r1 leaves
    assert np.bincount(world.coo("star300x2")["row"]).tolist() == [300, 300]
    assert sorted(np.bincount(world.coo("stars")["row"]).tolist()) == sorted(pr.STARS)
    for n in (8192, 8193):
        path, rules, node = world.wide(n)
        A = [i for i, (hd, _) in enumerate(rules.rules) if hd == pr.REL["A"]]
        assert len(A) == n and len(set(node[A].tolist())) == n and len({tuple(rules.rules[i][1]) for i in A}) == n
        assert max(len(rules.rules[i][1]) for i in A) == 5 and len(rules.rules) == n + 9
        # every prefix of a body is a body: the trie has no node without a rule but the root
        bodies = {tuple(rules.rules[i][1]) for i in A}
        assert all(b[:-1] in bodies for b in bodies if len(b) > 1)
    mixed = world.coo("mixed")
    h, r, t, _ = world.rows("mixed")
    hit = set(zip(mixed["row"].tolist(), mixed["ent"].tolist()))
    assert sum((q, int(t[q])) not in hit for q in range(len(t))) == 8
    assert (np.bincount(mixed["row"], minlength=len(h)) == 0).any()
    c94 = world.coo("tile94")
    assert c94["nq"] == 4136 and len(c94["ent"]) == 94 * len(world.coo("tile")["ent"])
    # the offset COO is the grounding of the tiled rows (checked on the first two tiles)
    h, r, t, etr = world.rows("tile94")
    two = pr.coo(world.g, world.rules, h[:88], r[:88], etr[:88])
    sub = em.select_rows(c94, np.arange(88))
    assert np.array_equal(two["row"], sub["row"]) and np.array_equal(two["ent"], sub["ent"])
    entries = lambda c: sorted(zip(c["ce"].tolist(), c["rule"].tolist(), c["count"].tolist()))  # noqa: E731
    assert entries(two) == entries(sub)


@pytest.mark.parametrize("removed", [True, False])
@pytest.mark.parametrize("feature", ["bias", "none"])
@pytest.mark.parametrize("name", ["A5", "B5", "stars", "D5"])
def test_matches_oracle(world, name, feature, removed):
    h, r, t, etr = world.rows(name)
    c = world.coo(name, removed)
    w, b = em.weights(world.rules, "normal"), em.bias(world.E)
    sd = {"rule_weights": w, "bias": b}
    want, mask = ref.predictor_forward(sd, feature, world.g, world.rules, h, r, etr if removed else None)
    cand = np.zeros_like(mask)
    cand[c["row"], c["ent"]] = True
    if feature == "none":
        assert np.array_equal(mask, cand) and np.all(want[~cand] == -np.inf)
    else:
        assert mask.all() and np.array_equal(want[~cand], np.broadcast_to(b, want.shape)[~cand])
    got = em.scores(c, w, b if feature == "bias" else None)
    assert np.abs(want[c["row"], c["ent"]] - got).max() <= 1e-5
    Hw, idx = ref.predictor_compute_H(sd, world.g, world.rules, h, r, t, etr if removed else None)
    Hg = em.H(c, w, world.rules, r, t)
    assert np.abs(Hg[idx] - Hw).max() <= 1e-5
    assert not np.any(np.delete(Hg, idx))
    pos, tot, ncand = em.rule_stats(c, len(w), t)
    assert np.array_equal(ncand, cand.sum(1)) and (pos <= tot).all()


def test_H_without_rules_or_candidates(world):
    h, r, t, etr = world.rows("C5")
    assert em.H(world.coo("C5"), em.weights(world.rules, "normal"), world.rules, r, t) is None
    # a row without candidates: the uniform softmax over its relation's rules
    h, r, t, etr = world.rows("mixed")
    c = world.coo("mixed")
    empty = np.nonzero((np.bincount(c["row"], minlength=len(h)) == 0) & (r != pr.REL["C"]))[0]
    assert len(empty)
    one = em.select_rows(c, empty[:1])
    Hq = em.H(one, em.weights(world.rules, "normal"), world.rules, r[empty[:1]], t[empty[:1]])
    idx = [i for i, _ in world.rules.relation2rules[int(r[empty[0]])]]
    assert np.allclose(Hq[idx], 1.0 / len(idx), rtol=1e-15) and Hq.sum() == pytest.approx(1.0)


def loop_ranks(logits, mask, flag, all_t, entity_size):
    """trainer.py:191-203, line for line, on torch CPU tensors."""
    out = []
    for k in range(all_t.size(0)):
        t = all_t[k]
        if mask[k, t].item() == True:  # noqa: E712
            val = logits[k, t]
            L = (logits[k][flag[k]] > val).sum().item() + 1
            H = (logits[k][flag[k]] >= val).sum().item() + 2
        else:
            L = 1
            H = entity_size + 1
        out += [[L, H]]
    return np.asarray(out, dtype=np.int64).reshape(-1, 2)


RANK_KINDS = ["randn", "eight", "equal", "zeros", "inf", "nan_t", "nan_other", "flag_none", "flag_t", "mask_t"]


def rank_input(kind, n, E, seed):
    """(score (n, E) float32, mask, flag (n, E) bool, all_t (n,)) of a ranks case:
    randn; 8 distinct values; all equal; +-0 mixed; +-inf mixed in; NaN at the
    target; NaN at competitors; flag all False; flag False at the target; mask
    False at the target."""
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((n, E)).astype(np.float32)
    all_t = rng.integers(0, E, n).astype(np.int64)
    mask = np.ones((n, E), dtype=bool)
    flag = rng.random((n, E)) < 0.8
    rows = np.arange(n)
    if kind == "eight":
        s = rng.integers(0, 8, (n, E)).astype(np.float32)
    elif kind == "equal":
        s[:] = 0.25
    elif kind == "zeros":
        s = np.where(rng.random((n, E)) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    elif kind == "inf":
        u = rng.random((n, E))
        s[u < 0.2], s[u > 0.8] = -np.inf, np.inf
    elif kind == "nan_t":
        s[rows, all_t] = np.nan
    elif kind == "nan_other":
        s[rng.random((n, E)) < 0.3] = np.nan
        s[rows, all_t] = 0.1
    elif kind == "flag_none":
        flag[:] = False
    elif kind == "flag_t":
        flag[rows, all_t] = False
    elif kind == "mask_t":
        mask[rows, all_t] = False
    return s, mask, flag, all_t


def test_ranks_matches_loop():
    n_rows = 0
    for k in range(40):
        kind = RANK_KINDS[k % len(RANK_KINDS)]
        E = [1, 2, 3, 7, 16][k % 5]
        s, mask, flag, all_t = rank_input(kind, 5, E, k)
        L, H = em.ranks(s, mask, flag, all_t)
        want = loop_ranks(torch.from_numpy(s), torch.from_numpy(mask), torch.from_numpy(flag),
                          torch.from_numpy(all_t), E)
        assert np.array_equal(np.stack([L, H], 1), want), (kind, E)
        n_rows += 5
    assert n_rows == 200


def test_measured_table(world):
    """Every measured GPU case once, the float32 run itself a sane
    implementation; prints the table of the module docstring."""
    b = em.bias(world.E)
    for name in H_SETS:
        for kind in H_KINDS:
            wide = 8192 if name == "wide" else None
            rules = world.rules if wide is None else world.wide(wide)[1]
            h, r, t, _ = world.rows(name)
            measure_H("H %s %s" % (name, kind), world.coo(name, True, wide), em.weights(rules, kind), rules, r, t)
    for name in STEP_SETS:
        h, r, t, _ = world.rows(name)
        measure_step("step %s" % name, world.coo(name), em.weights(world.rules, "normal"), b, world.target(name), t,
                     STEP_SMOOTHING)
    for B, E in LOSS_SHAPES:
        for s in LOSS_SMOOTHING:
            for c in LOSS_C:
                measure_nll("loss %dx%d s%g c%g" % (B, E, s, c), *loss_input(B, E), s, c)
    for B, E in LOSS_POISON:
        for p in ("nan", "inf"):
            measure_nll("loss %dx%d %s" % (B, E, p), *loss_input(B, E, p), 0.2, 1.5, rows=[0] + list(range(2, B)))
    for name in ("clamp", "zero1", "zero3"):
        x, target, all_t, s = loss_special(name)
        l64, g64, lb, gb = measure_nll("loss %s" % name, x, target, all_t, s, 1.5)
        if name != "clamp":
            assert l64 == 0 and not g64.any()
    groups = {}
    for label, e in sorted(E32.items()):
        key = " ".join(label.split()[:2]) if not label.startswith("H ") else label
        for q, v in e.items():
            groups.setdefault(key, {})[q] = max(groups.get(key, {}).get(q, 0.0), v)
            assert v <= 1e-3, (label, q, v)
    for key, e in groups.items():
        print("    %-22s " % key + "  ".join("%s %.1e" % (q, v) for q, v in e.items()))
