"""The miner's noisy-or and max aggregations on the GPU (RuleMiner.
set_aggregation; rnnl_miner_set_aggregation) in scores /
eval_ranks / predict_topk / explain on both sides, against the plain Python
restatement tests/mine_agg_ref.py.

No tolerances: scores and totals are compared bitwise; pairs, index, valid,
position, fired, rule and count exactly.  tests/test_mine_agg_ref.py shows, on
the restatement alone, that these inputs tell the modes and depths apart.
"""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import mine_agg_ref as A
import mine_eval_ref
from conftest import GOLDEN, REPO

pytestmark = pytest.mark.gpu

SIDES = ("tail", "head")
NEW_MODES = A.MODES[1:]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


_graphs, _fixtures = {}, {}


def real_graph(data):
    if data not in _graphs:
        from rnnlogic_amd import datasets
        from rnnlogic_amd.data import KnowledgeGraph
        _graphs[data] = KnowledgeGraph(datasets.materialize(data))
    return _graphs[data]


def fixture(data):
    if data not in _fixtures:
        _fixtures[data] = mine_eval_ref.load_fixture(os.path.join(GOLDEN, "_mine_eval_%s.npz" % data))
    return _fixtures[data]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def fake_graph(triples, E, R, **more):
    return types.SimpleNamespace(train_facts=[tuple(t) for t in triples], entity_size=E, relation_size=R, **more)


def make(dev, triples, E, R, rules, weights, max_body=3):
    """(a miner, {side: restatement}) with the same rules and weights."""
    from rnnlogic_amd.miner import RuleMiner
    miner = RuleMiner(fake_graph(triples, E, R), dev, max_body=max_body)
    miner.set_logic_rules(rules)
    miner.set_weights(weights)
    refs = {side: A.make_ref(side, triples, E, R) for side in SIDES}
    for ref in refs.values():
        ref.set_rules(rules, weights)
    return miner, refs


def check_scores_and_pairs(miner, ref, queries, E, side):
    want = np.asarray([ref.scores(*q) for q in queries], dtype=np.float64).reshape(len(queries), E)
    got = miner.scores(queries, side=side).cpu().numpy()
    assert got.dtype == np.float64 and same_bits(got, want)
    out = {}
    for filtered in (True, False):
        pairs = miner.eval_ranks(queries, filtered=filtered, side=side)
        assert np.array_equal(pairs, np.asarray(ref.pairs(queries, filtered), dtype=np.int64).reshape(-1, 2))
        out[filtered] = pairs
    return got, out


def check_topk(miner, ref, queries, k, filtered, candidates, side):
    index, score, valid, position = (x.cpu().numpy()
                                     for x in miner.predict_topk(queries, k, filtered, candidates, side=side))
    want = [ref.topk(h, r, t, k, filtered, candidates) for h, r, t in queries]
    assert np.array_equal(index, np.asarray([w[0] for w in want], dtype=np.int32).reshape(-1, k))
    assert same_bits(score, np.asarray([w[1] for w in want], dtype=np.float64).reshape(-1, k))
    assert valid.tolist() == [w[2] for w in want] and position.tolist() == [w[3] for w in want]
    return index, score, valid, position


def check_explain(miner, ref, queries, index, c, side):
    fired, total, rule, count = (x.cpu().numpy() for x in miner.explain(queries, index, c, side=side))
    assert rule.shape == count.shape == index.shape + (c,)
    for i, (h, r, t) in enumerate(queries):
        for j, e in enumerate(np.asarray(index)[i].tolist()):
            w = ref.explain(h, r, t, e, c)
            assert (int(fired[i, j]), rule[i, j].tolist(), count[i, j].tolist()) == (w[0], w[2], w[3])
            assert same_bits(total[i, j], w[1])
    return fired, total, rule, count


def check_everything(miner, refs, queries, E, modes=A.MODES, k=4, c=3):
    """All of a query's outputs in every mode on both sides; returns {(mode, depth, side): scores}."""
    out = {}
    for mode, depth in modes:
        miner.set_aggregation(mode, depth)
        assert miner.aggregation == (mode, depth)
        for side in SIDES:
            ref = refs[side].set_mode(mode, depth)
            out[(mode, depth, side)] = check_scores_and_pairs(miner, ref, queries, E, side)[0]
            for filtered, candidates in ((True, "reached"), (False, "all")):
                index = check_topk(miner, ref, queries, k, filtered, candidates, side)[0]
            fired, total, _, count = check_explain(miner, ref, queries, index[:, :3].copy(), c, side)
            if mode != "sum":
                assert set(count.reshape(-1).tolist()) <= {0, 1}
    return out


# --------------------------------------------------------------- 1. tiny graph
def test_tiny_graph_in_every_mode_on_both_sides(dev):
    miner, refs = make(dev, A.TINY, 8, 4, A.TINY_RULES, A.TINY_WEIGHTS)
    val = check_everything(miner, refs, A.TINY_QUERIES, 8)
    # the modes differ on the device as they do in the restatement (not one mode under three names)
    assert not np.array_equal(val[("sum", 1, "tail")], val[("noisy_or", 1, "tail")])
    assert not np.array_equal(val[("max", 1, "tail")], val[("max", 2, "tail")])
    assert not np.array_equal(val[("max", 2, "tail")], val[("max", 3, "tail")])
    assert not np.array_equal(val[("max", 2, "head")], val[("max", 3, "head")])
    miner.set_aggregation("max", 2)
    assert miner.eval_ranks([(0, 0, 1), (0, 0, 5)], filtered=False).tolist() == [[0, 1], [2, 3]]
    miner.set_aggregation("max", 1)
    assert miner.eval_ranks([(0, 0, 1), (0, 0, 5)], filtered=False).tolist() == [[0, 2], [2, 5]]
    # the display values: the probability, the strongest firing rule's weight
    s = miner.scores([(0, 3, 3)]).cpu().numpy()
    assert miner.score_value(s, 3).tolist() == [[0.0, .7, 0.0, .7, .7, .7, 0.0, 0.0]]
    miner.set_aggregation("noisy_or")
    p = miner.score_value(miner.scores([(0, 3, 3)]).cpu().numpy(), 3)[0]
    assert abs(p[5] - (1 - .3 ** 3)) < 1e-15 and abs(p[3] - (1 - .3 ** 2)) < 1e-15 and p[0] == 0.0


def test_long_bodies_on_both_sides(dev):
    """Bodies of four and five relations (max_body=5), the lists of the head-side tests, with confidences."""
    import mine_head_ref
    weights = [[1.0, .5, .5, .25, 0, .5, .125, .75, 1.0, .75, .25], [1.0, .25, .5, .5], [], [.7, .7]]
    miner, refs = make(dev, A.TINY, 8, 4, mine_head_ref.TINY_RULES, weights, max_body=5)
    check_everything(miner, refs, mine_head_ref.TINY_QUERIES, 8, modes=NEW_MODES)


# ------------------------------------- 2. rounds of four, more rules than lanes
def test_more_rules_than_a_round(dev):
    tri, E, R, rules = A.many_rules_graph()
    assert len(rules[0]) == 1110
    weights = A.confidence_like_weights(rules, 1)
    miner, refs = make(dev, tri, E, R, rules, weights)
    queries = tri[::5] + [(h, 0, t) for h in range(E) for t in (0, 5)]
    val = check_everything(miner, refs, queries, E, c=16)
    # max: the key is a function of the set of firing rules — a permuted list gives the same bits
    perm = np.random.default_rng(11).permutation(len(rules[0])).tolist()
    shuffled = [[rules[0][i] for i in perm]] + rules[1:]
    miner.set_logic_rules(shuffled)
    miner.set_weights([[weights[0][i] for i in perm]] + weights[1:])
    assert miner.aggregation == ("max", 3)
    for side in SIDES:
        assert same_bits(miner.scores(queries, side=side).cpu().numpy(), val[("max", 3, side)])
    keys = val[("max", 3, "tail")].astype(np.int64)
    assert np.any((keys >> 34) == ((keys >> 17) & 0x1FFFF)) and len(np.unique(keys >> 34)) > 2


# ---------------------------- 3. the regimes of the dense arrays (LDS / global)
@pytest.mark.parametrize("E", [512, 513, 2100])
def test_entities_in_lds_and_in_global_memory(dev, E):
    from rnnlogic_amd.miner import RuleMiner
    tri, E, R, rules, mids = A.spread_graph(E)
    queries = A.spread_queries(E, mids)
    miner, refs = make(dev, tri, E, R, rules, A.SPREAD_W)
    for mode, depth in NEW_MODES:
        miner.set_aggregation(mode, depth)
        for side in SIDES:
            ref = refs[side].set_mode(mode, depth)
            check_scores_and_pairs(miner, ref, queries, E, side)
            index = check_topk(miner, ref, queries, 10, True, "all", side)[0]
            check_explain(miner, ref, queries, index[:, :3].copy(), 3, side)
    # the scratch was left zeroed: the sum on this miner is a fresh miner's
    miner.set_aggregation("sum")
    fresh = RuleMiner(fake_graph(tri, E, R), dev)
    fresh.set_logic_rules(rules)
    fresh.set_weights(A.SPREAD_W)
    for side in SIDES:
        assert same_bits(miner.scores(queries, side=side).cpu().numpy(),
                         fresh.scores(queries, side=side).cpu().numpy())
        got, want = miner.predict_topk(queries, 10, side=side), fresh.predict_topk(queries, 10, side=side)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
        ex = [m.explain(queries, want[0][:, :3].contiguous(), 3, side=side) for m in (miner, fresh)]
        assert all(torch.equal(a, b) for a, b in zip(*ex))
    refs["tail"].set_mode("sum")
    assert same_bits(miner.scores(queries).cpu().numpy(), np.asarray([refs["tail"].scores(*q) for q in queries]))


# ------------------------------------------- 4. no path count, no range error
def test_reachability_has_no_range_error(dev):
    """1,700 parallel edges on each of three hops: 1,700^3 > 2^32 paths is an
    error code of the sum (as before) and nothing to the modes that do not count."""
    import math
    from rnnlogic_amd import _native
    from rnnlogic_amd.miner import RuleMiner
    tri = [(0, 0, 3)] + [(0, 1, 1)] * 1700 + [(1, 1, 2)] * 1700 + [(2, 1, 3)] * 1700
    miner = RuleMiner(fake_graph(tri, 4, 2), dev)
    miner.set_logic_rules([[(0, (1, 1, 1))], []])
    miner.set_weights([[0.5], []])
    with pytest.raises(_native.NativeError) as err:
        miner.eval_ranks([(0, 0, 3)])
    assert err.value.code == _native.RNNL_ERR_RANGE
    for (mode, depth), want in zip(NEW_MODES, (-math.log1p(-0.5), float(1 << 34), float(1 << 34), float(1 << 34))):
        miner.set_aggregation(mode, depth)
        for side, at in (("tail", 3), ("head", 0)):
            row = [0.0] * 4
            row[at] = want
            assert miner.scores([(0, 0, 3)], side=side).cpu().numpy().tolist() == [row]
            assert miner.eval_ranks([(0, 0, 3)], filtered=False, side=side).tolist() == [[0, 1]]
            index, score, valid, _ = miner.predict_topk([(0, 0, 3)], 2, side=side)
            assert index.tolist() == [[at, -1]] and score.tolist()[0][0] == want and valid.tolist() == [1]
            fired, total, rule, count = miner.explain([(0, 0, 3)], [[at, 1]], 2, side=side)
            assert fired.tolist() == [[1, 0]] and total.tolist() == [[want, 0.0]]
            assert rule.tolist() == [[[0, -1], [-1, -1]]] and count.tolist() == [[[1, 0], [0, 0]]]
    miner.set_aggregation("sum")
    with pytest.raises(_native.NativeError) as err:
        miner.eval_ranks([(0, 0, 3)])
    assert err.value.code == _native.RNNL_ERR_RANGE


# ------------------------------------------------- 5. stickiness and refresh
def test_the_mode_is_sticky_and_follows_the_weights(dev):
    from rnnlogic_amd import _native
    miner, refs = make(dev, A.TINY, 8, 4, A.TINY_RULES, A.TINY_WEIGHTS)
    ref, q = refs["tail"], A.TINY_QUERIES
    want_sum = miner.scores(q).cpu().numpy()
    miner.set_aggregation("noisy_or")
    first = miner.scores(q).cpu().numpy()
    assert same_bits(first, [ref.set_mode("noisy_or").scores(*x) for x in q])
    other = [[.25, 1.0, .125, .5, .5, 0, .75, .5, .0625], [.5, .5, 1.0, .25], [], [.1, .2, .3, .4]]
    miner.set_weights(other)  # other values: the operand is derived again
    ref.set_rules(A.TINY_RULES, other)
    second = miner.scores(q).cpu().numpy()
    assert same_bits(second, [ref.set_mode("noisy_or").scores(*x) for x in q]) and not np.array_equal(first, second)
    miner.set_logic_rules(A.TINY_RULES)  # new rules, weights 0: the mode stays, every u is 0
    assert miner.aggregation == ("noisy_or", 1)
    assert not miner.scores(q).cpu().numpy().any()
    miner.set_weights([[.25, 1.5, .125, .5, .5, 0, .75, .5, .0625]] + other[1:])
    with pytest.raises(ValueError, match="rule 1 of relation 0"):
        miner.scores(q)
    with pytest.raises(ValueError, match="rule 1 of relation 0"):  # and again: nothing was launched, nothing kept
        miner.predict_topk(q, 3)
    miner.set_aggregation("max", 2)  # max admits 1.5
    ref.set_rules(A.TINY_RULES, [[.25, 1.5, .125, .5, .5, 0, .75, .5, .0625]] + other[1:])
    assert same_bits(miner.scores(q).cpu().numpy(), [ref.set_mode("max", 2).scores(*x) for x in q])
    miner.set_weights([[.25, -1.5, .125, .5, .5, 0, .75, .5, .0625]] + other[1:])
    with pytest.raises(ValueError, match="rule 1 of relation 0"):
        miner.explain(q, [[0]] * len(q))
    miner.set_weights(A.TINY_WEIGHTS)
    miner.set_aggregation("sum")
    assert same_bits(miner.scores(q).cpu().numpy(), want_sum)
    # the native call checks its operand itself
    bad = torch.tensor([0.5] * 16 + [131072.0], dtype=torch.float64, device=dev)
    with pytest.raises(_native.NativeError) as err:
        _native.call("rnnl_miner_set_aggregation", miner._handle, _native.MINER_AGG_MAX, 1, bad.data_ptr(), None)
    assert err.value.code == _native.RNNL_ERR_INVALID
    bad[:] = 1.0
    bad[3] = float("nan")
    with pytest.raises(_native.NativeError):
        _native.call("rnnl_miner_set_aggregation", miner._handle, _native.MINER_AGG_NOISY_OR, 1, bad.data_ptr(), None)
    assert same_bits(miner.scores(q).cpu().numpy(), want_sum)  # a refused operand leaves the handle as it was


# ------------------------------------------------ 6. kinship, confidences
STRIDE = 8  # every 8th test triple: a cap on the pure-Python restatement's time, not a tolerance


def test_kinship_with_pca_confidences(dev):
    from rnnlogic_amd.miner import RuleMiner
    graph, fx = real_graph("kinship"), fixture("kinship")
    miner = RuleMiner(graph, dev)
    miner.set_logic_rules(fx["rules"])
    conf = miner.confidence("pca")
    miner.set_weights(conf)
    assert all(np.all((c >= 0) & (c <= 1)) for c in conf) and any(np.any(c > 0) for c in conf)
    triples = graph.test_facts[::STRIDE]
    known = graph.train_facts + graph.valid_facts + graph.test_facts
    got = {}
    for side in SIDES:
        ref = A.make_ref(side, graph.train_facts, graph.entity_size, graph.relation_size, known=known)
        ref.set_rules(fx["rules"], conf)
        for mode, depth in A.MODES:
            miner.set_aggregation(mode, depth)
            pairs = miner.eval_ranks(triples, side=side)
            assert np.array_equal(pairs, np.asarray(ref.set_mode(mode, depth).pairs(triples), dtype=np.int64))
            got[(mode, depth, side)] = pairs
    assert not np.array_equal(got[("sum", 1, "tail")], got[("noisy_or", 1, "tail")])
    assert not np.array_equal(got[("max", 1, "tail")], got[("max", 2, "tail")])
    miner.set_aggregation("noisy_or")
    assert miner.evaluate("test", side="both")["n"] == 2 * len(graph.test_facts)


# ------------------------------------------------------ 7. repeatability
@pytest.mark.parametrize("mode, depth", NEW_MODES[::3] + A.MODES[:1])
def test_two_calls_are_bitwise_equal(mode, depth, dev):
    from rnnlogic_amd.miner import RuleMiner
    graph, fx = real_graph("kinship"), fixture("kinship")
    miner = RuleMiner(graph, dev)
    miner.set_logic_rules(fx["rules"])
    miner.set_weights(miner.confidence("std"))
    miner.set_aggregation(mode, depth)
    q = graph.test_facts[:256]
    s = [miner.scores(q).cpu().numpy() for _ in range(2)]
    p = [miner.eval_ranks(graph.test_facts) for _ in range(2)]
    k = [miner.predict_topk(q, 10, True, "all") for _ in range(2)]
    assert s[0].any() and same_bits(s[0], s[1]) and np.array_equal(p[0], p[1])
    assert all(torch.equal(a, b) for a, b in zip(*k))


# ------------------------------------------------------- 8. command line
def test_command_line_with_confidences_and_max(dev, tmp_path):
    from rnnlogic_amd.miner import RuleMiner, metrics_line
    graph, fx = real_graph("umls"), fixture("umls")
    rule_file = tmp_path / "rules.txt"
    with open(str(rule_file), "w") as fo:
        for rules, ws in zip(fx["rules"], fx["weights"]):
            for (hd, body), w in zip(rules, ws):
                fo.write("%d%s %r\n" % (hd, "".join(" %d" % b for b in body), float(w)))
    miner = RuleMiner(graph, dev, max_body=5)
    miner.read_rules(str(rule_file))
    miner.set_weights(miner.confidence("pca"))
    miner.set_aggregation("max", 2)
    want = metrics_line("Test", miner.evaluate("test"))
    out = miner.predict("test", k=5, explain=2, output=str(tmp_path / "api.tsv"))
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = [sys.executable, "-m", "rnnlogic_amd.miner", "-data-path", graph.data_path, "-rule-file", str(rule_file)]
    got = subprocess.run(base + ["-weights", "conf", "-agg", "max", "-agg-depth", "2", "-evaluate", "test", "-predict",
                                 "test", "-k", "5", "-explain", "2", "-predictions-file", str(tmp_path / "cli.tsv")],
                         check=True, env=env, cwd=str(tmp_path), timeout=300, capture_output=True,
                         text=True).stdout.splitlines()
    assert got[-2:] == [want, "#Predictions written: %d" % int(np.sum(out["valid"]))]
    assert (tmp_path / "cli.tsv").read_bytes() == (tmp_path / "api.tsv").read_bytes()
    # the score column is the strongest firing rule's weight, the rule's own weight stays behind its count
    line = (tmp_path / "api.tsv").read_text().splitlines()[0].split("\t")
    assert 0.0 < float(line[4]) <= 1.0 and line[6].endswith(":1:" + line[4])
    # the file's learned weights are no confidences: the error names the rule and says what to do
    bad = subprocess.run(base + ["-agg", "noisy-or", "-evaluate", "test"], env=env, cwd=str(tmp_path), timeout=300,
                         capture_output=True, text=True)
    assert bad.returncode == 2 and "of relation" in bad.stderr and "-weights conf" in bad.stderr
