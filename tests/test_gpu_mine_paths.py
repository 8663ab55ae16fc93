"""The grounding paths behind a predicted answer on the GPU —
RuleMiner.explain_paths, predict(paths=...) and the command line's -paths
(rnnl_miner_paths_side, csrc/mine_paths.hip) — against the
brute-force restatement tests/mine_paths_ref.py and against explain's counts.

Everything is an integer and is compared exactly.  The graphs are those of
test_gpu_mine_eval.py, two small ones for the query's own edge, and a seeded
dense one for long bodies whose lists are cut inside a run of edges.
"""
import numpy as np
import pytest
import torch

from mine_paths_ref import PATH_LEN, MinePathsRef
from test_gpu_mine_eval import TINY, TINY_RULES, TINY_WEIGHTS, fake_graph, real_graph, run_cli, spread_graph
from test_gpu_mine_predict import TINY_Q

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def make(dev, triples, E, R, rules, weights=None, max_body=3):
    from rnnlogic_amd.miner import RuleMiner
    miner = RuleMiner(fake_graph(triples, E, R), dev, max_body=max_body)
    miner.set_logic_rules(rules)
    miner.set_weights(weights if weights is not None else [[0.5] * len(rs) for rs in rules])
    return miner, MinePathsRef(triples, E, R)


def head_form(queries):
    """The tail-side queries (h, r[, t]) as head-side ones: the open ones are open at h."""
    return [(h, r, t[0]) if t and t[0] >= 0 else (-1, r, h) for h, r, *t in queries]


def closed(queries):
    return [(h, r, t[0] if t else -1) for h, r, *t in queries]


def all_rules(queries, rules, m, extra=1):
    """(n, m, c): per slot every rule index of the query's relation, then -1 (c = the longest list + extra)."""
    c = max(len(rs) for rs in rules) + extra
    rule = np.full((len(queries), m, c), -1, dtype=np.int32)
    for i, (_, r, _) in enumerate(queries):
        rule[i, :, :len(rules[r])] = np.arange(len(rules[r]))
    return rule


def check(miner, ref, rules, queries, index, rule, P, side):
    """explain_paths against the restatement; returns the three numpy arrays."""
    queries = closed(queries)
    index, rule = np.asarray(index, dtype=np.int32), np.asarray(rule, dtype=np.int32)
    listed, count, path = (x.cpu().numpy() for x in miner.explain_paths(queries, index, rule, P, side))
    assert (listed.dtype, count.dtype, path.dtype) == (np.int32, np.int64, np.int32)
    assert listed.shape == count.shape == rule.shape and path.shape == rule.shape + (P, PATH_LEN)
    wl, wc, wp = ref.expected(queries, index.tolist(), rule.tolist(), rules, P, side)
    assert np.array_equal(count, np.asarray(wc, dtype=np.int64).reshape(count.shape))
    assert np.array_equal(listed, np.asarray(wl, dtype=np.int32).reshape(listed.shape))
    assert np.array_equal(path, np.asarray(wp, dtype=np.int32).reshape(path.shape))
    assert np.array_equal(listed, np.minimum(count, P))
    return listed, count, path


def slots_of(miner, queries, k, side, more):
    """predict_topk's first k entities per query, then the columns `more` (entities, or -1)."""
    index = miner.predict_topk(queries, k, side=side)[0].cpu().numpy()
    return np.concatenate([index] + [np.full((len(queries), 1), e, dtype=np.int32) for e in more], 1)


def counts_equal_explain(miner, queries, index, rule, count, side):
    """Under the sum: explain's fired is the number of rules with paths, its counts are these counts."""
    c = rule.shape[2]
    fired, _, erule, ecount = (x.cpu().numpy() for x in miner.explain(queries, index, c, side))
    for i, j in np.ndindex(*index.shape):
        named = rule[i, j] >= 0
        assert fired[i, j] == int((count[i, j][named] > 0).sum())
        for kk, n in zip(erule[i, j].tolist(), ecount[i, j].tolist()):
            if kk >= 0:
                assert count[i, j, kk] == n  # (rule[i, j, kk] == kk: all_rules lists the indices in order)


def walks_own_edge(row, body, h, r, t):
    ents = [x for x in row if x >= 0]
    return any(b == r and (a, z) == (h, t) for a, b, z in zip(ents, body, ents[1:]))


# --------------------------------------------------------------- 1. tiny graph
@pytest.mark.parametrize("side", ["tail", "head"])
def test_tiny_graph(dev, side):
    miner, ref = make(dev, TINY, 8, 4, TINY_RULES, TINY_WEIGHTS)
    queries = closed(TINY_Q) if side == "tail" else head_form(TINY_Q)
    index = slots_of(miner, queries, 3, side, (-1, 7 if side == "tail" else 6))
    rule = all_rules(queries, TINY_RULES, index.shape[1])
    assert rule.shape[2] == 10 and TINY_RULES[0][0] == (0, ()) and TINY_RULES[0][8] == (0, (3,))
    for P in (1, 3, 64):
        listed, count, path = check(miner, ref, TINY_RULES, queries, index, rule, P, side)
        assert count.max() >= 2 and (count > 0).sum() >= 20
        assert not count[:, 3].any() and np.all(path[:, 3] == -1)     # the -1 slot
        rel0 = np.asarray([r == 0 for _, r, _ in queries])
        assert not count[:, :, 8].any() and not count[rel0][:, :, 0].any()  # a rule that never fires, one without a body
        assert not count[:, :, 9].any() and np.all(path[:, :, 9] == -1)  # the -1 entry
        counts_equal_explain(miner, queries, index, rule, count, side)
        for i, (h, r, t) in enumerate(queries):
            for j, k in np.ndindex(*rule.shape[1:]):
                for row in path[i, j, k][:listed[i, j, k]]:
                    assert not walks_own_edge(row.tolist(), TINY_RULES[r][k][1], h, r, t)
    # (0, 0, 1) is in train twice: 0 -0-> 1 -1-> 5 is two paths, side by side
    q = [(0, 0, -1)] if side == "tail" else [(-1, 0, 5)]
    e = 5 if side == "tail" else 0
    listed, count, path = (x.cpu().numpy() for x in miner.explain_paths(q, [[e]], [[[6]]], 3, side))
    assert TINY_RULES[0][6] == (0, (0, 1)) and (listed.item(), count.item()) == (2, 2)
    assert path[0, 0, 0].tolist() == [[0, 1, 5, -1, -1, -1]] * 2 + [[-1] * 6]


# ------------------------------------------------------ 2. the query's own edge
def test_own_edge_is_skipped_on_every_hop(dev):
    """0 -> 2 -> 0 -> 1 -> 3, all of the head relation: the body (0, 0, 0, 0) passes (0, 0, 1) on its third hop."""
    tri = [(0, 0, 1), (0, 0, 2), (2, 0, 0), (1, 0, 3)]
    rules = [[(0, (0,)), (0, (0, 0, 0, 0)), (0, (0, 0, 0))]]
    miner, ref = make(dev, tri, 4, 1, rules, max_body=5)
    index = [[1, 3, 0, 2]] * 2
    rule = all_rules([(0, 0, 1)] * 2, rules, 4)
    listed, count, path = check(miner, ref, rules, [(0, 0, 1), (0, 0, -1)], index, rule, 3, "tail")
    assert count[0, 0, 0] == 0 and count[1, 0, 0] == 1 and path[1, 0, 0, 0].tolist() == [0, 1, -1, -1, -1, -1]
    assert count[0, 1, 1] == 0 and count[1, 1, 1] == 1 and path[1, 1, 1, 0].tolist() == [0, 2, 0, 1, 3, -1]
    assert not count[0, :2].any() and count[1, :2].sum() == 3  # 1 and 3 lie behind the own edge
    listed, count, path = check(miner, ref, rules, [(0, 0, 1), (-1, 0, 1)], index, rule, 3, "head")
    assert count[0, 2, 2] == 0 and count[1, 2, 2] == 1 and path[1, 2, 2, 0].tolist() == [0, 2, 0, 1, -1, -1]
    assert count[0, 2, 0] == 0 and count[1, 2, 0] == 1 and path[1, 2, 0, 0].tolist() == [0, 1, -1, -1, -1, -1]
    # the doubled own edge of the tiny graph: closed, no path of 0 <- 0 or 0 <- 0 1 over it; open, two of each
    miner, ref = make(dev, TINY, 8, 4, TINY_RULES, TINY_WEIGHTS)
    rule = [[[4, 6]] * 2] * 2
    assert TINY_RULES[0][4] == (0, (0,))
    listed, count, path = check(miner, ref, TINY_RULES, [(0, 0, 1), (0, 0, -1)], [[1, 5]] * 2, rule, 4, "tail")
    assert count[0].tolist() == [[0, 0], [1, 0]] and count[1].tolist() == [[2, 0], [1, 2]]


# ------------------------------------- 3. both regimes and the boundary, 7. twice
@pytest.mark.parametrize("E", [512, 513, 2100])
def test_entities_in_lds_and_in_global_memory(dev, E):
    """512 entities are the most the LDS levels hold; from 513 on they are per-workgroup global memory."""
    tri, E, R, rules, mids = spread_graph(E)
    miner, ref = make(dev, tri, E, R, rules)
    tails = [(0, 0, 5), (0, 0, E - 1), (0, 0, -1), (7, 0, 5), (0, 1, E - 1), (E - 1, 2, 0), (5, 2, -1), (0, 0, 5)]
    for side, queries, more in (("tail", tails, (5, E - 4, -1)), ("head", head_form(tails), (0, mids[50], E - 3))):
        index = slots_of(miner, queries, 3, side, more)
        rule = all_rules(queries, rules, index.shape[1])
        for P in (3, 64):
            listed, count, path = check(miner, ref, rules, queries, index, rule, P, side)
            assert count.max() == len(mids) == 100 and (count > 0).sum() >= 12  # cut at 3 and at 64
            assert np.array_equal(count[0], count[-1]) and np.array_equal(path[0], path[-1])  # the same query
            if side == "tail":  # 0 -1-> the 100 middle entities -2-> 5, the middles ascending
                assert path[0, 3, 1, :, 1].tolist() == mids[:P] and np.all(path[0, 3, 1, :, 2] == 5)
        counts_equal_explain(miner, queries, index, rule, count, side)


@pytest.mark.parametrize("E", [512, 2100])
def test_two_calls_are_byte_equal(dev, E):
    tri, E, R, rules, mids = spread_graph(E)
    miner, _ = make(dev, tri, E, R, rules)
    for side, queries in (("tail", [(0, 0, 5), (0, 0, -1), (0, 1, E - 1)] * 20),
                          ("head", [(0, 0, 5), (-1, 0, 5), (0, 1, E - 1)] * 20)):
        index = miner.predict_topk(queries, 4, side=side)[0]
        rule = all_rules(queries, rules, 4)
        a = miner.explain_paths(queries, index, rule, 8, side)
        b = miner.explain_paths(queries, index, rule, 8, side)
        assert all(torch.equal(x, y) for x, y in zip(a, b)) and int(a[0].sum()) > 0


# ------------------------- 4. lists cut inside a run of edges, bodies of 4 and 5
DENSE_SEED, DENSE_TRIPLES, DENSE_P = 3, 330, 4
DENSE_RULES = [[(0, (1, 2, 0, 1)), (0, (0, 0, 1, 2, 0)), (0, (2,)), (0, (1, 1, 2, 2, 1)), (0, (2, 1, 0, 0))],
               [(1, (0, 1, 2, 0, 1)), (1, (2, 2, 2, 2))], [(2, (0, 1, 0, 1, 0))]]


def dense_graph():
    """40 entities, 3 relations, seeded; triples drawn with repeats, so some edges are doubled."""
    rng = np.random.default_rng(DENSE_SEED)
    E, R, n = 40, 3, DENSE_TRIPLES
    tri = [(int(h), int(r), int(t)) for h, r, t in zip(rng.integers(0, E, n), rng.integers(0, R, n),
                                                       rng.integers(0, E, n))]
    return tri, E, R


@pytest.mark.parametrize("side", ["tail", "head"])
def test_truncation_inside_a_run_and_long_bodies(dev, side):
    tri, E, R = dense_graph()
    miner, ref = make(dev, tri, E, R, DENSE_RULES, max_body=5)
    tails = tri[:12] + [(h, r, -1) for h in range(3) for r in range(R)]
    queries = closed(tails) if side == "tail" else head_form(tails)
    index = slots_of(miner, queries, 4, side, ())
    rule = all_rules(queries, DENSE_RULES, index.shape[1], extra=0)
    _, wc, _ = ref.expected(queries, index.tolist(), rule.tolist(), DENSE_RULES, DENSE_P, side)
    wc = np.asarray(wc, dtype=np.int64)
    long_body = np.asarray([[len(DENSE_RULES[r][k][1]) >= 4 if k >= 0 else False for k in rule[i, 0]]
                            for i, (_, r, _) in enumerate(queries)])[:, None, :] & (wc > 0)
    print("dense %s: %d entries with count > P, %d with 0 < count < P, %d of them with bodies of 4 or 5, max %d"
          % (side, (wc > DENSE_P).sum(), ((wc > 0) & (wc < DENSE_P)).sum(), long_body.sum(), wc.max()))
    assert (wc > DENSE_P).sum() >= 20 and ((wc > 0) & (wc < DENSE_P)).sum() >= 5 and wc.max() < 2 ** 32
    assert long_body.sum() >= 20 and len(set(tri)) < len(tri)
    listed, count, path = check(miner, ref, DENSE_RULES, queries, index, rule, DENSE_P, side)
    counts_equal_explain(miner, queries, index, rule, count, side)


# ------------------------------------------------------------ 5. aggregations
def test_aggregations_change_nothing(dev):
    weights = [[0.3, 0.5, 0.5, 0.25, 0.0, 0.5, 0.1, 0.3, 1.0], [1.0, 0.25, 0.5, 0.5], [], [0.7, 0.7]]
    miner, ref = make(dev, TINY, 8, 4, TINY_RULES, weights)
    queries = closed(TINY_Q)
    index = slots_of(miner, queries, 3, "tail", (-1,))
    rule = all_rules(queries, TINY_RULES, 4)
    want = miner.explain_paths(queries, index, rule, 3)
    assert int(want[1].max()) >= 2  # more than reachability
    for agg in (("noisy_or", 1), ("max", 2)):
        miner.set_aggregation(agg[0], depth=agg[1])
        for side in ("tail", "head"):
            q = queries if side == "tail" else head_form(TINY_Q)
            check(miner, ref, TINY_RULES, q, index, rule, 3, side)
        assert all(torch.equal(a, b) for a, b in zip(want, miner.explain_paths(queries, index, rule, 3)))
        assert miner.aggregation == agg
        assert int(miner.explain(queries, index, 3)[3].max()) == 1  # explain itself reports reachability there


# ------------------------------------------------------------------ 6. range
def test_path_count_past_32_bits_is_reported(dev):
    from rnnlogic_amd import _native
    from rnnlogic_amd.miner import RuleMiner
    tri = [(0, 0, 3)] + [(0, 1, 1)] * 1700 + [(1, 1, 2)] * 1700 + [(2, 1, 3)] * 1700
    miner = RuleMiner(fake_graph(tri, 4, 2), dev)
    miner.set_logic_rules([[(0, (1, 1, 1))], []])
    miner.set_weights([[0.5], []])
    for side in ("tail", "head"):
        with pytest.raises(_native.NativeError) as err:
            miner.explain_paths([(0, 0, 3)], [[3, 0]], [[[0], [0]]], 2, side)
        assert err.value.code == _native.RNNL_ERR_RANGE
    miner.set_logic_rules([[(0, (1, 1))], []])  # 1,700^2 fits
    miner.set_weights([[0.5], []])
    listed, count, path = miner.explain_paths([(0, 0, 3)], [[2, 3]], [[[0], [0]]], 3)
    assert listed.tolist() == [[[3], [0]]] and count.tolist() == [[[1700 * 1700], [0]]]
    assert path[0, 0, 0].tolist() == [[0, 1, 2, -1, -1, -1]] * 3 and bool((path[0, 1] == -1).all())


# ---------------------------------------------------------------- 8. kinship
@pytest.mark.parametrize("side", ["tail", "head"])
def test_kinship_with_the_shipped_rules(dev, side):
    from rnnlogic_amd import datasets
    from rnnlogic_amd.miner import RuleMiner, read_rule_file
    graph = real_graph("kinship")
    miner = RuleMiner(graph, dev)
    miner.read_rules(datasets.rule_file("kinship"))
    rules, _ = read_rule_file(datasets.rule_file("kinship"), graph.relation_size)
    ref = MinePathsRef(graph.train_facts, graph.entity_size, graph.relation_size)
    queries = [tuple(q) for q in graph.test_facts[:64]]
    index = miner.predict_topk(queries, 3, side=side)[0]
    fired, _, rule, ecount = miner.explain(queries, index, 3, side)
    listed, count, path = check(miner, ref, rules, queries, index.cpu().numpy(), rule.cpu().numpy(), 4, side)
    assert np.array_equal(count, ecount.cpu().numpy())
    print("kinship %s: %d entries with count > 4, %d with 0 < count < 4" % (side, (count > 4).sum(),
                                                                           ((count > 0) & (count < 4)).sum()))
    assert (count > 4).sum() >= 5 and ((count > 0) & (count < 4)).sum() >= 100  # some lists are cut, most are whole


# --------------------------- 9. predict(paths=..., output=...) and the command line
def bracket_checks(lines, P):
    """Each rule column `rule:count:weight [a > x > b | ...]`: min(P, count) paths between the line's ends."""
    seen = 0
    for ln in lines:
        cols = ln.split("\t")
        for col in cols[6:]:
            text, inner = col[:-1].rsplit(" [", 1)
            assert col.endswith("]") and " <- " in text
            count = int(text.rsplit(":", 2)[1])
            parts = inner.split(" | ")
            assert (parts[-1] == "...") == (count > P)
            parts = parts[:-1] if parts[-1] == "..." else parts
            assert len(parts) == min(P, count) and count >= 1
            for p in parts:
                ents = p.split(" > ")
                assert ents[0] == cols[0] and ents[-1] == cols[3] and 2 <= len(ents) <= PATH_LEN
            seen += len(parts)
    return seen


def test_predict_file_and_command_line(dev, tmp_path):
    from rnnlogic_amd import datasets
    from rnnlogic_amd.miner import RuleMiner
    graph = real_graph("kinship")
    miner = RuleMiner(graph, dev, max_body=5)  # as the command line holds a rule file
    miner.read_rules(datasets.rule_file("kinship"))
    base = ["-data-path", graph.data_path, "-rule-file", datasets.rule_file("kinship"), "-k", "3", "-explain", "2"]
    out = miner.predict("test", k=3, explain=2, paths=2, output=str(tmp_path / "api.tsv"))
    n = len(graph.test_facts)
    assert out["explain_path"].shape == (n, 2, 3, 2, PATH_LEN) and out["explain_path"].dtype == np.int32
    assert out["explain_paths_listed"].shape == out["explain_paths_count"].shape == (n, 2, 3)
    assert np.array_equal(out["explain_paths_count"], out["explain_count"])
    got = run_cli(base + ["-predict", "test", "-paths", "2", "-predictions-file", str(tmp_path / "cli.tsv")], tmp_path)
    assert (tmp_path / "cli.tsv").read_bytes() == (tmp_path / "api.tsv").read_bytes()
    assert got[-1] == "#Predictions written: %d" % int(out["valid"].sum())
    lines = (tmp_path / "api.tsv").read_text().splitlines()
    assert bracket_checks(lines, 2) == int(out["explain_paths_listed"].sum()) > n
    # the head side, through a queries file: one closed and one open line
    h, r, t = graph.test_facts[0]
    (tmp_path / "q.tsv").write_text("%s\t%s\t%s\n\t%s\t%s\n" % (graph.id2entity[h], graph.id2relation[r],
                                                               graph.id2entity[t], graph.id2relation[r],
                                                               graph.id2entity[t]))
    hout = miner.predict(triples=[(h, r, t), (-1, r, t)], k=3, explain=2, paths=2, side="head",
                         output=str(tmp_path / "h_api.tsv"))
    run_cli(base + ["-queries-file", str(tmp_path / "q.tsv"), "-side", "head", "-paths", "2", "-predictions-file",
                    str(tmp_path / "h_cli.tsv")], tmp_path)
    assert (tmp_path / "h_cli.tsv").read_bytes() == (tmp_path / "h_api.tsv").read_bytes()
    assert bracket_checks((tmp_path / "h_api.tsv").read_text().splitlines(), 2) == \
        int(hout["explain_paths_listed"].sum()) > 0
    # without -paths: the file of predict(paths=0), no bracket anywhere
    miner.predict("test", k=3, explain=2, output=str(tmp_path / "plain_api.tsv"))
    run_cli(base + ["-predict", "test", "-predictions-file", str(tmp_path / "plain_cli.tsv")], tmp_path)
    plain = (tmp_path / "plain_api.tsv").read_bytes()
    assert (tmp_path / "plain_cli.tsv").read_bytes() == plain and b"[" not in plain
    assert [ln.split(" [")[0] for col in lines for ln in col.split("\t")[6:]] == \
        [c for ln in plain.decode().splitlines() for c in ln.split("\t")[6:]]


# ------------------------------------------------------------ 10. bad arguments
def test_bad_arguments_raise(dev):
    miner, _ = make(dev, TINY, 8, 4, TINY_RULES, TINY_WEIGHTS)
    q, index, rule = [(0, 0, 1)], [[1, 5]], [[[1, 2], [1, -1]]]
    assert int(miner.explain_paths(q, index, rule, 3)[1].sum()) > 0
    for P in (0, 65):
        with pytest.raises(ValueError):
            miner.explain_paths(q, index, rule, P)
    for bad in ([[[1, 2]]], [[1, 2], [1, -1]], [[[1, 2], [1, -1]]] * 2, [[[1] * 17, [1] * 17]]):
        with pytest.raises(ValueError):
            miner.explain_paths(q, index, bad, 3)
    with pytest.raises(ValueError):
        miner.explain_paths(q, index, rule, 3, side="both")
    with pytest.raises(ValueError):
        miner.explain_paths([(8, 0, 1)], index, rule, 3)
    with pytest.raises(ValueError):
        miner.predict(triples=q, k=3, paths=2)
    with pytest.raises(ValueError):
        miner.predict(triples=q, k=3, explain=2, paths=65)
    from rnnlogic_amd import _native
    for index_bad, rule_bad in (([[1, 8]], rule), (index, [[[1, 9], [1, -1]]])):  # an entity / a rule index out of range
        with pytest.raises(_native.NativeError) as err:
            miner.explain_paths(q, index_bad, rule_bad, 3)
        assert err.value.code == _native.RNNL_ERR_INTERNAL  # (counters[2], as explain reports it)
