"""explain_paths of both predictors (rnnl_paths_rows) and
TrainerPredictor.predict(paths=...) on the GPU.

Every comparison is integer and exact.  The yardstick is the brute-force
enumeration of tests/mine_paths_ref.py on its tail side (every path walked and
written down, then sorted by x_{L-1}, x_{L-2}, ...): `t = -1` removes nothing,
a closed (h, r, t) removes the row's own edge — on graphs without doubled
triples that is the edge with the row's edges_to_remove id.

 1. three models (UMLS PredictorPlus lstm/sum/bias, kinship PredictorPlus
    emb/pna/none, UMLS EM Predictor): test rows of several relations, the first
    3 places of predict_topk, per slot the top 3 rules of explain_rows, a rule
    of the relation that does not reach the entity, a -1 entry, a -1 slot;
    P = 1, 3, 64.
 2. count equals explain_rows' count; a duplicated rule lists the same paths
    under both ids.
 3. a training batch with its edges_to_remove; rows chosen on the CPU so that
    a listed path would walk the removed edge if it stayed; the inverse twin
    is walked (a small graph that has one).
 4. 512 / 513 / 2,100 entities: below and above the bound where the levels
    leave LDS for the caller's scratch; a frontier of 100 entities; lists cut
    at 3 and at 64.
 5. a seeded dense graph with bodies of four and five relations.
 6. more than 2^32 paths: the closed form and the first paths by hand.
 7. one triple given twice, through the C-ABI directly.
 8. the invalid entries raise ValueError.
 9. two calls are byte-equal in both regimes.
10. TrainerPredictor.predict(paths=2) and (paths=0).
"""
import ctypes
import random

import numpy as np
import pytest
import torch

import synth_graphs
import test_gpu_predict as tp
from mine_paths_ref import PATH_LEN, MinePathsRef

pytestmark = pytest.mark.gpu

LDS_E = 512  # csrc/paths.hip PATHS_LDS_E: up to here the levels live in LDS


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ---------------------------------------------------------------- helpers
_REF = {}


def _ref_of(data):
    if data not in _REF:
        graph = tp._env(data)[0]
        _REF[data] = MinePathsRef(graph.train_facts, graph.entity_size, graph.relation_size)
    return _REF[data]


def _expected(refm, rules, h, r, t, ents, named, P):
    """The three arrays from the reference: rows (h[i], r[i]) with the closed
    tail t[i] (-1: nothing removed), ents (n, m), named (n, m, c) global rule
    ids into rules = [(head, body)]."""
    n, m, c = named.shape
    listed = np.zeros((n, m, c), np.int32)
    count = np.zeros((n, m, c), np.int64)
    path = np.full((n, m, c, P, PATH_LEN), -1, np.int32)
    for i in range(n):
        for j in range(m):
            for s in range(c):
                k, e = int(named[i, j, s]), int(ents[i, j])
                if k < 0 or e < 0:
                    continue
                assert rules[k][0] == int(r[i])
                got = refm.explain_paths(int(h[i]), int(r[i]), int(t[i]), e, rules[k][1], P)
                listed[i, j, s], count[i, j, s], path[i, j, s] = got[0], got[1], np.asarray(got[2], np.int32)
    return listed, count, path


def _assert_equal(got, want, what):
    listed, count, path = [x.cpu().numpy() for x in got]
    assert listed.dtype == np.int32 and count.dtype == np.int64 and path.dtype == np.int32
    assert np.array_equal(count, want[1]), (what, "count")
    assert np.array_equal(listed, want[0]), (what, "listed")
    assert np.array_equal(path, want[2]), (what, "path")


def _rules_of(model):
    return [(int(hd), [int(b) for b in body]) for hd, body in model.rules]


def _top_rules(off, rule, count, slot, c):
    """The first c rules of a slot of explain_rows' CSR by (count descending, rule id ascending), on the host."""
    a, b = int(off[slot]), int(off[slot + 1])
    pairs = sorted(zip(count[a:b].tolist(), rule[a:b].tolist()), key=lambda cr: (-cr[0], cr[1]))[:c]
    return [k for _, k in pairs]


def _synthetic(tmp_path, name, E, R, facts, rules, dev, queries=None):
    """An EM Predictor on a graph written as a dataset directory: (model, reference)."""
    from rnnlogic_amd.data import KnowledgeGraph
    from rnnlogic_amd.predictors import Predictor
    h0, _, t0 = facts[0]
    spec = synth_graphs.Spec(name, E, R, list(facts), queries or {"q": (h0, t0)}, [(hd, list(b)) for hd, b in rules])
    path, _ = synth_graphs.write(spec, tmp_path / name)
    graph = KnowledgeGraph(path)
    model = Predictor(graph, entity_feature="bias")
    model.set_rules([[hd] + list(b) for hd, b in rules])
    return model.to(dev).eval(), MinePathsRef(facts, E, R), graph


def _walks(path_row, src, rel_at, body, dst):
    """Does the path x_0 .. x_L walk an edge src -rel-> dst on a hop of relation rel_at?"""
    return any(body[j] == rel_at and path_row[j] == src and path_row[j + 1] == dst for j in range(len(body)))


# ---------------------------------------------------------------- 1, 2: the shipped models
def _model_case(name, dev, duplicate=False):
    """Rows of three relations, the first 3 places of predict_topk and one -1
    slot; per slot the top 3 rules of explain_rows, one rule of the relation
    that does not reach the entity, one -1 entry: (model, h, r, ents, named, csr)."""
    model = tp._model(name, dev, duplicate)[0]
    data = tp.MODELS[name][0]
    rules = _rules_of(model)
    hs, rs = [], []
    for q, h, _ in tp._relation_rows(data, n_rel=3, per=4):
        hs += h.tolist()
        rs += [q] * len(h)
    th, tr = torch.tensor(hs, device=dev), torch.tensor(rs, device=dev)
    top = model.predict_topk(th, tr, 10)[0][:, :3]
    ents = torch.cat([top, torch.full_like(top[:, :1], -1)], 1).contiguous()
    off, rule, count = [x.cpu().numpy() for x in model.explain_rows(th, tr, ents)]
    n, m = ents.shape
    named = np.full((n, m, 5), -1, np.int32)
    e_host = ents.cpu().numpy()
    for i in range(n):
        of_rel = [k for k, (hd, body) in enumerate(rules) if hd == rs[i] and 1 <= len(body) <= 5]
        for j in range(m):
            if e_host[i, j] < 0:
                continue
            a, b = int(off[i * m + j]), int(off[i * m + j + 1])
            firing = set(rule[a:b].tolist())
            best = _top_rules(off, rule, count, i * m + j, 3)
            named[i, j, :len(best)] = best
            silent = [k for k in of_rel if k not in firing]
            if silent:
                named[i, j, 3] = silent[0]
    return model, th, tr, ents, named, (off, rule, count)


@pytest.mark.parametrize("name", sorted(tp.MODELS))
def test_paths_equal_the_reference(name, dev):
    model, th, tr, ents, named, _ = _model_case(name, dev)
    refm, rules = _ref_of(tp.MODELS[name][0]), _rules_of(model)
    h, r, e = th.cpu().numpy(), tr.cpu().numpy(), ents.cpu().numpy()
    assert len(set(r.tolist())) >= 2 and (named[:, :3, :3] >= 0).any() and (named[:, :3, 3] >= 0).any()
    assert (e[:, 3] == -1).all() and (named[:, :, 4] == -1).all()
    cut = 0
    for P in (1, 3, 64):
        want = _expected(refm, rules, h, r, np.full(len(h), -1), e, named, P)
        _assert_equal(model.explain_paths(th, tr, ents, torch.from_numpy(named), P), want, (name, P))
        cut += int((want[1] > P).sum())
        assert (want[0][:, :, 3] == 0).all() and (want[1][:, :, 3] == 0).all()  # the rule that does not reach
    assert cut, "no entry has more paths than are listed"


@pytest.mark.parametrize("name", ["plus_lstm_sum_bias", "em_bias"])
def test_counts_are_explain_rows_counts_and_a_duplicated_rule_lists_the_same(name, dev):
    model, th, tr, ents, named, (off, rule, count) = _model_case(name, dev, duplicate=True)
    rules = _rules_of(model)
    dup = len(rules) - 1
    orig = rules.index(rules[dup])
    assert orig < dup
    n, m, _ = named.shape
    # the last two entries of every slot of the duplicated rule's relation name both copies
    both = named.copy()
    e_host = ents.cpu().numpy()
    for i in range(n):
        if int(tr[i]) == rules[dup][0]:
            both[i, :, 3] = np.where(e_host[i] >= 0, orig, -1)
            both[i, :, 4] = np.where(e_host[i] >= 0, dup, -1)
    listed, cnt, path = [x.cpu().numpy() for x in model.explain_paths(th, tr, ents, torch.from_numpy(both), 5)]
    seen = fired = 0
    for i in range(n):
        for j in range(m):
            a, b = int(off[i * m + j]), int(off[i * m + j + 1])
            by_rule = dict(zip(rule[a:b].tolist(), count[a:b].tolist()))
            for s in range(5):
                if both[i, j, s] >= 0 and e_host[i, j] >= 0:
                    assert cnt[i, j, s] == by_rule.get(int(both[i, j, s]), 0), (i, j, s)
                    seen += 1
            if both[i, j, 3] == orig and both[i, j, 4] == dup:
                assert cnt[i, j, 3] == cnt[i, j, 4] and listed[i, j, 3] == listed[i, j, 4]
                assert np.array_equal(path[i, j, 3], path[i, j, 4])
                fired += int(cnt[i, j, 3] > 0)
    assert seen and fired, "no slot where the duplicated rule has a path"


# ---------------------------------------------------------------- 3: edge removal
def test_edge_removal_on_a_training_batch(dev):
    name, P = "em_bias", 3
    model = tp._model(name, dev)[0]
    graph, train_set, _, _ = tp._env("umls")
    refm, rules = _ref_of("umls"), _rules_of(model)
    E = graph.entity_size
    # on the CPU reference alone: rows of a batch where, with nothing removed, one of the first P paths of a rule at
    # an entity walks the row's own edge
    picked = None
    for b in range(min(len(train_set), 40)):
        all_h, all_r, all_t, _, etr = train_set[b]
        q = int(all_r[0])
        of_rel = [k for k, (hd, body) in enumerate(rules) if hd == q and q in body][:3]
        cases = []
        for i, (h, t) in enumerate(zip(all_h.tolist(), all_t.tolist())):
            for k in of_rel:
                for e in range(E):
                    first = refm.paths(h, q, -1, e, rules[k][1])[:P]
                    if any(_walks(p, h, q, rules[k][1], t) for p in first):
                        cases.append((i, e, k))
        if cases:
            picked = (all_h, all_r, all_t, etr, of_rel, cases)
            break
    assert picked is not None, "no training batch where a listed path would walk the removed edge"
    all_h, all_r, all_t, etr, of_rel, cases = picked
    rows = sorted({i for i, _, _ in cases})[:6]
    m = 3
    ents = np.full((len(rows), m), -1, np.int32)
    for a, i in enumerate(rows):
        es = sorted({e for i2, e, _ in cases if i2 == i})[:m]
        ents[a, :len(es)] = es
    named = np.full((len(rows), m, 3), -1, np.int32)
    named[:, :, :len(of_rel)] = of_rel
    sel = torch.tensor(rows)
    h, r, t, te = all_h[sel], all_r[sel], all_t[sel], etr[sel]
    open_want = _expected(refm, rules, h.numpy(), r.numpy(), np.full(len(rows), -1), ents, named, P)
    walked = sum(_walks(open_want[2][a, j, s, p], int(h[a]), int(r[a]), rules[int(named[a, j, s])][1], int(t[a]))
                 for a in range(len(rows)) for j in range(m) for s in range(len(of_rel))
                 for p in range(open_want[0][a, j, s]))
    assert walked >= 1
    want = _expected(refm, rules, h.numpy(), r.numpy(), t.numpy(), ents, named, P)
    got = model.explain_paths(h.to(dev), r.to(dev), torch.from_numpy(ents), torch.from_numpy(named), P,
                              edges_to_remove=te.to(dev))
    _assert_equal(got, want, "removed")
    path, listed = got[2].cpu().numpy(), got[0].cpu().numpy()
    for a in range(len(rows)):
        for j in range(m):
            for s in range(len(of_rel)):
                for p in range(listed[a, j, s]):
                    assert not _walks(path[a, j, s, p], int(h[a]), int(r[a]), rules[int(named[a, j, s])][1], int(t[a]))
    # and without edges_to_remove nothing is skipped
    _assert_equal(model.explain_paths(h.to(dev), r.to(dev), torch.from_numpy(ents), torch.from_numpy(named), P),
                  open_want, "kept")
    assert not np.array_equal(open_want[1], want[1])


def test_the_inverse_twin_of_the_removed_edge_is_walked(dev, tmp_path):
    """r1 is r0's inverse here: (1, r1, 0) is the twin of the row's own edge (0, r0, 1).  r0 <- r0 r0 r1 r0 from 0:
    0 > 2 > 1 > 0 > {1, 2}; the removed edge takes 0 > 1 away at the first and the last hop, the twin 1 > 0 stays."""
    from rnnlogic_amd.data import TrainDataset
    facts = [(0, 0, 1), (1, 1, 0), (0, 0, 2), (2, 0, 1)]
    rules = [(0, [0, 0, 1, 0]), (0, [0])]
    model, refm, graph = _synthetic(tmp_path, "twin", 4, 2, facts, rules, dev)
    etr = None
    train_set = TrainDataset(graph, 8)
    for b in range(len(train_set)):
        all_h, all_r, all_t, _, ids = train_set[b]
        for i in range(len(all_h)):
            if (int(all_h[i]), int(all_r[i]), int(all_t[i])) == facts[0]:
                etr = ids[i:i + 1]
    assert etr is not None
    h, r = torch.tensor([0], device=dev), torch.tensor([0], device=dev)
    ents, named = np.asarray([[1, 2, 3]], np.int32), np.zeros((1, 3, 2), np.int32)
    named[:, :, 1] = 1
    kept = _expected(refm, rules, [0], [0], [-1], ents, named, 4)
    assert kept[1][0].tolist() == [[1, 1], [1, 1], [0, 0]] and kept[2][0, 0, 0, 0].tolist() == [0, 2, 1, 0, 1, -1]
    want = _expected(refm, rules, [0], [0], [1], ents, named, 4)
    assert want[1][0].tolist() == [[0, 0], [1, 1], [0, 0]]
    got = model.explain_paths(h, r, torch.from_numpy(ents), torch.from_numpy(named), 4, edges_to_remove=etr.to(dev))
    _assert_equal(got, want, "twin")
    twin = got[2][0, 1, 0, 0].tolist()
    assert twin == [0, 2, 1, 0, 2, -1] and _walks(twin, 1, 1, rules[0][1], 0)
    _assert_equal(model.explain_paths(h, r, torch.from_numpy(ents), torch.from_numpy(named), 4), kept, "twin kept")


# ---------------------------------------------------------------- 4, 9: regimes
def _fan_graph(E):
    """0 -r1-> 100 middle entities spread over the id range -r2-> the last entity and each a private one; a third hop
    r3 from those back to E - 2.  Entities without an edge stay between."""
    mids = [1 + (i * (E - 210)) // 100 for i in range(100)]
    assert len(set(mids)) == 100 and max(mids) < E - 205
    last, priv = E - 1, [E - 205 + i for i in range(100)]
    facts = [(0, 0, last)]
    facts += [(0, 1, x) for x in mids]
    facts += [(x, 2, last) for x in mids] + [(x, 2, p) for x, p in zip(mids, priv)]
    facts += [(x, 2, priv[0]) for x in mids[1::2]]
    facts += [(p, 3, E - 2) for p in priv] + [(last, 3, E - 2)]
    rules = [(0, [1, 2]), (0, [1, 2, 3]), (0, [1]), (0, [2, 3])]
    return facts, rules, mids, priv


@pytest.mark.parametrize("E", [LDS_E, LDS_E + 1, 2100])
def test_both_regimes_against_the_reference_and_twice(E, dev, tmp_path):
    facts, rules, mids, priv = _fan_graph(E)
    model, refm, _ = _synthetic(tmp_path, "fan%d" % E, E, 4, facts, rules, dev)
    need = ctypes.c_size_t()
    from rnnlogic_amd import _native
    _native.call("rnnl_paths_rows_scratch", model.graph.device_graph(dev), 2, ctypes.byref(need))
    assert (need.value == 0) == (E <= LDS_E) and need.value in (0, 2 * 72 * E)
    h, r = torch.tensor([0, mids[3]], device=dev), torch.tensor([0, 0], device=dev)
    ents = np.asarray([[E - 1, priv[0], E - 2, mids[99]], [E - 2, E - 1, -1, 0]], np.int32)
    named = np.tile(np.asarray([0, 1, 2, 3], np.int32), (2, 4, 1))
    for P in (3, 64):
        want = _expected(refm, rules, [0, mids[3]], [0, 0], [-1, -1], ents, named, P)
        if P == 3:
            assert want[1][0, 0, 0] == 100 and want[1][0, 1, 0] == 51 and want[1][0, 2, 1] == 250
            assert want[1][0, 3, 2] == 1 and want[1][1, 0, 3] == 3
        got = model.explain_paths(h, r, torch.from_numpy(ents), torch.from_numpy(named), P)
        _assert_equal(got, want, (E, P))
        assert got[0][0, 0, 0] == P and got[0][0, 1, 0] == min(P, 51)
        again = model.explain_paths(h, r, torch.from_numpy(ents), torch.from_numpy(named), P)
        for a, b in zip(got, again):
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


# ---------------------------------------------------------------- 5: long bodies
def _dense(seed, E=14, R=3, n=70):
    rng = random.Random(seed)
    facts = sorted({(rng.randrange(E), rng.randrange(R), rng.randrange(E)) for _ in range(n)})
    rng.shuffle(facts)
    rules = [(0, [rng.randrange(R) for _ in range(L)]) for L in (4, 5, 4, 5, 5)]
    return E, R, facts, rules


def test_bodies_of_four_and_five(dev, tmp_path):
    P = 4
    for seed in range(50):
        E, R, facts, rules = _dense(seed)
        refm = MinePathsRef(facts, E, R)
        hs = list(range(6))
        ents = np.tile(np.arange(E, dtype=np.int32), (len(hs), 1))
        named = np.tile(np.arange(len(rules), dtype=np.int32), (len(hs), E, 1))
        want = _expected(refm, rules, hs, [0] * len(hs), [-1] * len(hs), ents, named, P)
        many, few = int((want[1] > P).sum()), int(((want[1] >= 1) & (want[1] <= 3)).sum())
        if many >= 20 and few >= 20:
            break
    assert many >= 20 and few >= 20, "no seed below 50 gives 20 entries above P and 20 with 1..3 paths"
    print("seed %d: %d entries with more than %d paths, %d with 1..3" % (seed, many, P, few))
    model, _, _ = _synthetic(tmp_path, "dense", E, R, facts, rules, dev)
    got = model.explain_paths(torch.tensor(hs, device=dev), torch.zeros(len(hs), dtype=torch.int64, device=dev),
                              torch.from_numpy(ents), torch.from_numpy(named), P)
    _assert_equal(got, want, "long bodies")


# ---------------------------------------------------------------- 6: past 2^32
def test_counts_past_2_32(dev, tmp_path):
    """e0 -r1-> L1 -r1-> L2 -r1-> L3 -r1-> L4 -r1-> e5, 257 entities per layer wired complete bipartite, and the rule
    r0 <- r1^5: 257^4 = 4,362,470,401 > 2^32 paths from e0 to e5.  In the order (x_4, x_3, x_2, x_1 ascending) the
    first paths hold the first entity of L4, L3 and L2 and run through L1."""
    w = 257
    layers = [[0]] + [list(range(1 + k * w, 1 + (k + 1) * w)) for k in range(4)] + [[1 + 4 * w]]
    E = 2 + 4 * w
    facts = [(0, 0, E - 1)] + [(x, 1, y) for a, b in zip(layers[:-1], layers[1:]) for x in a for y in b]
    rules = [(0, [1, 1, 1, 1, 1]), (0, [1, 1, 1, 1]), (0, [1, 1, 1])]
    from rnnlogic_amd.data import KnowledgeGraph
    from rnnlogic_amd.predictors import Predictor
    spec = synth_graphs.Spec("layers257", E, 2, facts, {"q": (0, E - 1)}, [(hd, list(b)) for hd, b in rules])
    graph = KnowledgeGraph(synth_graphs.write(spec, tmp_path / "layers257")[0])
    model = Predictor(graph, entity_feature="bias")
    model.set_rules([[hd] + b for hd, b in rules])
    model = model.to(dev).eval()
    P = 5
    ents = torch.tensor([[E - 1, layers[4][7], layers[3][0]]], dtype=torch.int32)
    named = torch.tensor([[[0, 1, 2]] * 3], dtype=torch.int32)
    listed, count, path = [x.cpu().numpy() for x in model.explain_paths(
        torch.tensor([0], device=dev), torch.tensor([0], device=dev), ents, named, P)]
    assert w ** 4 > 2 ** 32
    assert count[0].tolist() == [[w ** 4, 0, 0], [0, w ** 3, 0], [0, 0, w ** 2]]
    assert listed[0].tolist() == [[P, 0, 0], [0, P, 0], [0, 0, P]]
    first = [layer[0] for layer in layers]
    assert path[0, 0, 0].tolist() == [[0, layers[1][p], first[2], first[3], first[4], E - 1] for p in range(P)]
    assert path[0, 1, 1].tolist() == [[0, layers[1][p], first[2], first[3], layers[4][7], -1] for p in range(P)]
    assert path[0, 2, 2].tolist() == [[0, layers[1][p], first[2], first[3], -1, -1] for p in range(P)]
    assert (path[0, 0, 1:] == -1).all() and (path[0, 1, 0] == -1).all()


# ---------------------------------------------------------------- 7: a doubled edge, through the C-ABI
def test_a_triple_given_twice_is_two_edges(dev):
    from rnnlogic_amd import _native
    # 0 -r1-> {1, 2}, 1 -r1-> 3 twice, 2 -r1-> 3, 3 -r1-> 4: below the doubled edge every path appears twice in a row
    facts = [(0, 1, 1), (0, 1, 2), (1, 1, 3), (2, 1, 3), (1, 1, 3), (3, 1, 4), (0, 0, 4), (5, 1, 1)]
    rules = [(0, [1, 1, 1]), (0, [1, 1]), (0, [1])]
    E, R, P = 6, 2, 6
    refm = MinePathsRef(facts, E, R)
    hrt = np.ascontiguousarray(facts, dtype=np.int32)
    tok = np.ascontiguousarray([x for hd, b in rules for x in [hd] + b], dtype=np.int32)
    ptr = np.ascontiguousarray(np.cumsum([0] + [1 + len(b) for _, b in rules]), dtype=np.int64)
    g, rl = ctypes.c_void_p(), ctypes.c_void_p()
    with torch.cuda.device(dev):
        _native.call("rnnl_graph_create", hrt.ctypes.data_as(ctypes.c_void_p), len(facts), E, R, ctypes.byref(g))
        try:
            _native.call("rnnl_rules_create", g, tok.ctypes.data_as(ctypes.c_void_p),
                         ptr.ctypes.data_as(ctypes.c_void_p), len(rules), ctypes.byref(rl))
            h = torch.tensor([0, 5], dtype=torch.int64, device=dev)
            r = torch.zeros(2, dtype=torch.int64, device=dev)
            ents = np.asarray([[4, 3, 1], [4, 3, 1]], np.int32)
            named = np.tile(np.asarray([0, 1, 2], np.int32), (2, 3, 1))
            d_ent, d_rule = torch.from_numpy(ents).to(dev), torch.from_numpy(named).to(dev)
            listed = torch.empty((2, 3, 3), dtype=torch.int32, device=dev)
            count = torch.empty((2, 3, 3), dtype=torch.int64, device=dev)
            path = torch.empty((2, 3, 3, P, PATH_LEN), dtype=torch.int32, device=dev)
            counters = torch.empty(4, dtype=torch.int64, device=dev)
            need = ctypes.c_size_t(1)
            _native.call("rnnl_paths_rows_scratch", g, 2, ctypes.byref(need))
            assert need.value == 0
            _native.call("rnnl_paths_rows", g, rl, h.data_ptr(), r.data_ptr(), None, 2, d_ent.data_ptr(), 3,
                         d_rule.data_ptr(), 3, P, listed.data_ptr(), count.data_ptr(), path.data_ptr(), None, 0,
                         counters.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
            assert counters.cpu().tolist() == [0, 0, 0, 0]
        finally:
            if rl:
                _native.call("rnnl_rules_destroy", rl)
            _native.call("rnnl_graph_destroy", g)
    want = _expected(refm, rules, [0, 5], [0, 0], [-1, -1], ents, named, P)
    assert want[1][0].tolist() == [[3, 0, 0], [0, 3, 0], [0, 0, 1]] and want[1][1, 0, 0] == 2
    assert want[2][0, 0, 0, :3].tolist() == [[0, 1, 3, 4, -1, -1], [0, 1, 3, 4, -1, -1], [0, 2, 3, 4, -1, -1]]
    _assert_equal((listed, count, path), want, "doubled")


# ---------------------------------------------------------------- 8: invalid entries
def test_invalid_entries_raise(dev, tmp_path):
    facts = [(0, 0, 1), (0, 1, 1), (1, 1, 2), (2, 1, 0)]
    rules = [(0, [1]), (1, [0]), (0, [1] * 6), (0, [1, 1])]
    model, _, _ = _synthetic(tmp_path, "invalid", 3, 2, facts, rules, dev)
    h, r = torch.tensor([0], device=dev), torch.tensor([0], device=dev)

    def call(ent, rule, **kw):
        return model.explain_paths(h, r, torch.tensor([[ent]], dtype=torch.int32),
                                   torch.tensor([[[rule]]], dtype=torch.int32), 2, **kw)
    listed, count, path = call(1, 0)
    assert (int(listed), int(count), path[0, 0, 0, 0].tolist()) == (1, 1, [0, 1, -1, -1, -1, -1])
    for ent, rule in ((1, 1), (1, 4), (1, -2), (3, 0), (-2, 0), (1, 2)):  # other relation, ids out of range, body of six
        with pytest.raises(ValueError, match="explain_paths"):
            call(ent, rule)
    with pytest.raises(ValueError, match="explain_paths"):
        call(1, 0, edges_to_remove=torch.tensor([7], device=dev))  # relation 0 has one edge
    # unused slots and entries are no error
    listed, count, path = call(-1, 0)
    assert int(listed) == 0 and int(count) == 0 and (path == -1).all()
    listed, count, path = call(1, -1)
    assert int(listed) == 0 and int(count) == 0 and (path == -1).all()
    # what predict(paths=) does with a listed rule that has no walkable body: it names it -1
    assert model.listable(torch.tensor([0, 2, 3], dtype=torch.int32)).tolist() == [0, -1, 3]
    listed, count, path = call(1, int(model.listable(torch.tensor([2], dtype=torch.int32))[0]))
    assert int(listed) == 0 and int(count) == 0 and (path == -1).all()
    # argument errors, as the miner's explain_paths raises them
    with pytest.raises(ValueError, match="rules must be"):
        model.explain_paths(h, r, torch.zeros((1, 2), dtype=torch.int32), torch.zeros((1, 2, 17), dtype=torch.int32))
    with pytest.raises(ValueError, match="entities must be"):
        model.explain_paths(h, r, torch.zeros((2, 2), dtype=torch.int32), torch.zeros((2, 2, 1), dtype=torch.int32))
    from rnnlogic_amd import _native
    buf = torch.zeros(64, dtype=torch.int64, device=dev)
    rc = _native.lib().rnnl_paths_rows(model.graph.device_graph(dev), model.native_rules(dev).ptr, buf.data_ptr(),
                                       buf.data_ptr(), None, 1 << 20, buf.data_ptr(), 64, buf.data_ptr(), 16, 64,
                                       buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), None, 0, buf.data_ptr(), None)
    assert rc == _native.RNNL_ERR_INVALID and "2^31" in _native.lib().rnnl_last_error().decode()


def test_a_scratch_that_is_too_small_is_refused(dev, tmp_path):
    from rnnlogic_amd import _native
    facts, rules, _, _ = _fan_graph(LDS_E + 1)
    model, _, _ = _synthetic(tmp_path, "small_scratch", LDS_E + 1, 4, facts, rules, dev)
    buf = torch.zeros(64, dtype=torch.int64, device=dev)
    p = buf.data_ptr()
    for scratch, size in ((None, 0), (p, 72 * (LDS_E + 1) - 1)):
        rc = _native.lib().rnnl_paths_rows(model.graph.device_graph(dev), model.native_rules(dev).ptr, p, p, None, 1,
                                           p, 1, p, 1, 1, p, p, p, scratch, size, p, None)
        assert rc == _native.RNNL_ERR_INVALID and "scratch" in _native.lib().rnnl_last_error().decode()


# ---------------------------------------------------------------- 10: TrainerPredictor.predict
def test_trainer_predict_with_paths(dev, tmp_path):
    from rnnlogic_amd.data import ValidDataset
    from rnnlogic_amd.miner import path_text
    from rnnlogic_amd.trainer import TrainerPredictor
    model = tp._model("plus_lstm_sum_bias", dev)[0]
    graph, train_set, test_set, _ = tp._env("umls")
    solver = TrainerPredictor(model, train_set, ValidDataset(graph, 32), test_set,
                              torch.optim.Adam(model.parameters(), lr=0.005), gpus=[0])
    before = solver.evaluate("test")
    m, P = 2, 2
    plain_file, zero_file, paths_file = [str(tmp_path / f) for f in ("plain.tsv", "zero.tsv", "paths.tsv")]
    plain = solver.predict("test", k=5, explain=m, output=plain_file)
    zero = solver.predict("test", k=5, explain=m, output=zero_file, paths=0)
    assert sorted(plain) == sorted(zero) and all(np.array_equal(plain[key], zero[key]) for key in plain)
    assert open(plain_file).read() == open(zero_file).read()
    out = solver.predict("test", k=5, explain=m, output=paths_file, paths=P)
    assert solver.evaluate("test") == before
    assert all(np.array_equal(plain[key], out[key]) for key in plain)
    n = len(out["h"])
    assert out["explain_paths_rule"].shape == (n, m, m) and out["explain_paths_rule"].dtype == np.int32
    assert out["explain_paths_listed"].shape == (n, m, m) and out["explain_paths_count"].shape == (n, m, m)
    assert out["explain_path"].shape == (n, m, m, P, PATH_LEN)
    # the named rules: the first m of each slot by (count descending, rule id ascending)
    for slot in range(n * m):
        best = _top_rules(out["explain_off"], out["explain_rule"], out["explain_count"], slot, m)
        assert out["explain_paths_rule"][slot // m, slot % m].tolist() == best + [-1] * (m - len(best))
    # the arrays are explain_paths' on the same slots
    th, tr = torch.from_numpy(out["h"]).to(dev), torch.from_numpy(out["r"]).to(dev)
    got = model.explain_paths(th, tr, torch.from_numpy(out["index"][:, :m].copy()),
                              torch.from_numpy(out["explain_paths_rule"]), P)
    for key, x in zip(("explain_paths_listed", "explain_paths_count", "explain_path"), got):
        assert np.array_equal(out[key], x.cpu().numpy()), key
    assert (out["explain_paths_count"] > out["explain_paths_listed"]).any()
    # every bracket of the file reads back to the array row; ` | ...` exactly where count > listed
    lines = [line.rstrip("\n").split("\t") for line in open(paths_file)]
    plain_lines = [line.rstrip("\n").split("\t") for line in open(plain_file)]
    assert len(lines) == len(plain_lines) == int(out["valid"].sum())
    at = 0
    for i in range(n):
        for j in range(int(out["valid"][i])):
            c, c0 = lines[at], plain_lines[at]
            at += 1
            assert c[:6] == c0[:6] and len(c) == len(c0)
            if j >= m:
                assert len(c) == 6
                continue
            named = [int(k) for k in out["explain_paths_rule"][i, j] if k >= 0]
            assert len(c) == 6 + len(named)
            for s, (col, col0) in enumerate(zip(c[6:], c0[6:])):
                text, bracket = col.split(" [", 1)
                assert text == col0 and bracket.endswith("]")
                assert text == "%s:%d" % (solver.rule_text(model.rules[named[s]]), out["explain_paths_count"][i, j, s])
                parts = bracket[:-1].split(" | ")
                listed = int(out["explain_paths_listed"][i, j, s])
                more = out["explain_paths_count"][i, j, s] > listed
                assert (parts[-1] == "...") == bool(more)
                parts = parts[:-1] if more else parts
                assert parts == [path_text(row, graph) for row in out["explain_path"][i, j, s][:listed]]
    with pytest.raises(ValueError, match="explain > 0"):
        solver.predict("test", k=5, paths=2)
