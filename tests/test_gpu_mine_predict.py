"""The miner's predictions on the GPU — RuleMiner.predict_topk / explain /
predict and the command line (rnnl_miner_predict / rnnl_miner_explain,
csrc/mine_predict.hip) — against the restatement tests/mine_predict_ref.py and
against the calls that were there before (scores, eval_ranks).

Everything is compared exactly: index, valid, position, fired, rule and count
as integers, score and total bit for bit.  The graphs are those of
test_gpu_mine_eval.py.
"""
import math

import numpy as np
import pytest
import torch

import mine_predict_ref
from test_gpu_mine_eval import (TINY, TINY_RULES, TINY_WEIGHTS, fake_graph, fixture, many_rules_graph,
                                quantised_weights, real_graph, run_cli, spread_graph, write_rule_file)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def make(dev, triples, E, R, rules, weights, known=None, max_body=3, **more):
    from rnnlogic_amd.miner import RuleMiner
    miner = RuleMiner(fake_graph(triples, E, R, **more), dev, max_body=max_body)
    miner.set_logic_rules(rules)
    miner.set_weights(weights)
    ref = mine_predict_ref.MinePredictRef(triples, E, R, known=known)
    ref.set_rules(rules, weights)
    return miner, ref


def closed(q):
    return [(h, r, t[0] if t else -1) for h, r, *t in q]


def check_topk(miner, ref, queries, k, filtered, candidates):
    """predict_topk against the restatement; returns the four arrays."""
    index, score, valid, position = (x.cpu().numpy() for x in miner.predict_topk(queries, k, filtered, candidates))
    want = [ref.topk(h, r, t, k, filtered, candidates) for h, r, t in closed(queries)]
    assert index.dtype == np.int32 and score.dtype == np.float64 and index.shape == score.shape == (len(want), k)
    assert np.array_equal(index, np.asarray([w[0] for w in want], dtype=np.int32).reshape(-1, k))
    assert same_bits(score, np.asarray([w[1] for w in want], dtype=np.float64).reshape(-1, k))
    assert valid.tolist() == [w[2] for w in want] and position.tolist() == [w[3] for w in want]
    return index, score, valid, position


def check_explain(miner, ref, queries, index, c):
    fired, total, rule, count = (x.cpu().numpy() for x in miner.explain(queries, index, c))
    assert rule.dtype == np.int32 and count.dtype == np.int64 and rule.shape == count.shape == index.shape + (c,)
    for i, (h, r, t) in enumerate(closed(queries)):
        for j, e in enumerate(np.asarray(index)[i].tolist()):
            w = ref.explain(h, r, t, e, c)
            assert (int(fired[i, j]), rule[i, j].tolist(), count[i, j].tolist()) == (w[0], w[2], w[3])
            assert same_bits(total[i, j], w[1])
    return fired, total, rule, count


# --------------------------------------------------------------- 1. tiny graph
TINY_Q = [
    (0, 0, 1),   # a train triple that is there twice
    (5, 2, 0),   # a relation without rules
    (6, 0, 7),   # a head that nothing leaves but the removed edge
    (0, 0, 5), (3, 0, 6), (0, 0, 7), (2, 0, 2), (0, 1, 5), (0, 3, 3),
    (0, 0, 1),   # the first query again
    (0, 0, -1), (5, 2, -1), (6, 0, -1),  # open: t = -1
]


@pytest.mark.parametrize("k", [1, 3, 8, 20])
def test_tiny_graph(dev, k):
    miner, ref = make(dev, TINY, 8, 4, TINY_RULES, TINY_WEIGHTS)
    assert 0.0 in TINY_WEIGHTS[0] and TINY_WEIGHTS[0].count(0.5) == 2 and min(TINY_WEIGHTS[0]) < 0
    for filtered in (True, False):
        for candidates in ("reached", "all"):
            index, score, valid, position = check_topk(miner, ref, TINY_Q, k, filtered, candidates)
            assert np.array_equal(index[0], index[9]) and same_bits(score[0], score[9])  # a repeated query
            assert np.all(position[10:] == -1)
            for i in range(len(TINY_Q)):
                assert np.all(index[i, valid[i]:] == -1) and np.all(np.isneginf(score[i, valid[i]:]))
            if candidates == "reached":
                assert valid[1] == 0 and valid[2] == 0
            else:  # no rules: the first k unfiltered ids with 0.0
                ids = [e for e in range(8) if not (filtered and e in (1,))][:k]  # (5, 2, 1) is known, t = 0 stays
                assert index[1, :valid[1]].tolist() == ids and not score[1, :valid[1]].any()
            if k == 20:
                assert np.all(valid < k)  # k > |E|
            check_explain(miner, ref, TINY_Q, index[:, :min(k, 4)].copy(), 3)
    # the open forms of a head keep the query's edge: (h, r) and (h, r, -1) agree, the closed query differs
    open2 = miner.predict_topk([(0, 0), (5, 2), (6, 0)], 8, False, "all")
    open3 = miner.predict_topk(TINY_Q[10:], 8, False, "all")
    assert all(torch.equal(a, b) for a, b in zip(open2, open3))
    assert ref.ground(0, 0, -1)[0] != ref.ground(0, 0, 1)[0]
    assert not same_bits(miner.predict_topk([(0, 0, 1)], 8, False, "all")[1].cpu().numpy(), open3[1][:1].cpu().numpy())


# ------------------------- 2. tie runs across the k-th place, in both regimes
SPREAD_W = [[0.5, -0.25, 1.0, 0.0, 0.5, 0.125], [1.0, 0.5], [0.5, 0.5]]


@pytest.mark.parametrize("E", [512, 513, 2100])
def test_tie_runs_across_the_kth_place(dev, E):
    """512 entities are the most LDS holds; from 513 on val, the integer scratch
    and the flags are per-workgroup global memory."""
    tri, E, R, rules, mids = spread_graph(E)
    q = [(0, 0, 5)]
    miner, ref = make(dev, tri, E, R, rules, SPREAD_W)
    order, val = ref.order(0, 0, 5, False, "reached")
    v = [val[e] for e in order]
    assert sum(x > 0.5 for x in v) == 5 and v[5:104] == [0.5] * 99 and len(v) == 107 and sum(x < 0 for x in v) == 3
    everyone = ref.order(0, 0, 5, False, "all")[0]
    zeros = [val[e] for e in everyone]
    assert zeros[199] == zeros[200] == 0.0 and all(x < 0 for x in zeros[-3:])  # 200 falls inside the zero run
    for k in (10, 64):
        assert v[k - 1] == v[k] == 0.5  # inside the 0.5 run: the lowest ids win
    for k in (5, 10, 64, 104, 107, 200):
        got = {}
        for filtered in (False, True):
            got[filtered] = check_topk(miner, ref, q + [(0, 0, E - 1), (0, 0, -1)], k, filtered, "reached")
            check_topk(miner, ref, q + [(0, 1, E - 1), (E - 1, 2, -1)], k, filtered, "all")
        if k in (10, 64):
            assert got[False][0][0, 5:k].tolist() == sorted(order[5:104])[:k - 5]
        if k >= 107:  # everything, the negatives last; filtered, two known tails have left
            assert got[False][2][0] == 107 and all(val[e] < 0 for e in got[False][0][0, 104:107])
            assert got[True][2][0] == 105 and all(val[e] < 0 for e in got[True][0][0, 102:105])
    # the first rule at weight 0.0: the middle entities are reached with val +0.0
    w0 = [[0.0] + SPREAD_W[0][1:]] + SPREAD_W[1:]
    miner.set_weights(w0)
    ref.set_rules(rules, w0)
    order, val = ref.order(0, 0, 5, False, "reached")
    v = [val[e] for e in order]
    assert v.count(0.0) == 99 and len(v) == 107 and all(x < 0 for x in v[-3:])  # ahead of the negatives
    everyone = ref.order(0, 0, 5, False, "all")[0]
    run = [e for e in everyone if val[e] == 0.0]
    assert run == sorted(run) and len(run) == E - 8  # reached or not: by id alone
    for k in (64, 107, 200):
        check_topk(miner, ref, q, k, False, "reached")
        check_topk(miner, ref, q, k, False, "all")


# --------------------------- 3. more rules than a round or a wave holds
def test_explanations_of_many_rules(dev):
    tri, E, R, rules = many_rules_graph()
    assert len(rules[0]) == 1110
    queries = tri[:4] + [(h, 0, 5) for h in range(4)] + [(1, 0, -1)]
    miner, ref = make(dev, tri, E, R, rules, quantised_weights(rules, 1))
    index = check_topk(miner, ref, queries, 3, True, "reached")[0]
    tie = False
    for c in (1, 3, 16):
        fired, _, rule, _ = check_explain(miner, ref, queries, index, c)
        assert fired.max() >= 100
    for i, (h, r, t) in enumerate(queries):
        for e in index[i].tolist():
            if e >= 0:
                top = sorted(ref.contributions(h, r, t, e), reverse=True)[:16]
                tie |= any(a == b for a, b in zip(top, top[1:]))
    assert tie  # equal contributions among the first c: the list index decides


# ----------------------------------- 4. consistency with the existing calls
def test_consistent_with_scores_and_eval_ranks_on_kinship(dev):
    from rnnlogic_amd.miner import RuleMiner
    graph, fx = real_graph("kinship"), fixture("kinship")
    miner = RuleMiner(graph, dev)
    miner.set_logic_rules(fx["rules"])
    miner.set_weights(fx["weights"])
    q = graph.test_facts[:200]
    k = min(256, graph.entity_size)
    got = miner.predict_topk(q, k, True, "all")
    again = miner.predict_topk(q, k, True, "all")
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    index, score, valid, position = (x.cpu().numpy() for x in got)
    scores = miner.scores(q).cpu().numpy()
    pairs = miner.eval_ranks(q)
    for i in range(len(q)):
        n = int(valid[i])
        assert n > 0 and same_bits(score[i, :n], scores[i, index[i, :n]])
        assert pairs[i, 0] <= position[i] < pairs[i, 1]
    fired, total, rule, count = miner.explain(q, got[0][:, :8].contiguous(), 3)
    listed = index[:, :8] >= 0
    assert listed.any() and same_bits(total.cpu().numpy()[listed], score[:, :8][listed]) and int(fired.max()) > 0
    twice = miner.explain(q, got[0][:, :8].contiguous(), 3)
    assert all(torch.equal(a, b) for a, b in zip((fired, total, rule, count), twice))


# ------------------------------------------- 5. bodies of 4 and 5 relations
def test_bodies_of_four_and_five_relations(dev):
    rng = np.random.default_rng(11)
    E, R = 12, 3
    tri = sorted(set((int(h), int(r), int(t)) for h, r, t in
                     zip(rng.integers(0, E, 70), rng.integers(0, R, 70), rng.integers(0, E, 70))))
    rules = [[(0, (1, 2, 0, 1)), (0, (0, 0, 1, 2, 0)), (0, (2,)), (0, (1, 1, 2, 2, 1)), (0, (2, 1, 0, 0))],
             [(1, (0, 1, 2, 0, 1)), (1, (2, 2, 2, 2))], [(2, (0, 1, 0, 1, 0))]]
    weights = [[0.5, -0.25, 0.1, 0.5, 1e-3], [1.0, -1.7], [0.5]]
    miner, ref = make(dev, tri, E, R, rules, weights, max_body=5)
    queries = tri[:12] + [(h, r, -1) for h in range(3) for r in range(R)]
    for candidates in ("reached", "all"):
        index = check_topk(miner, ref, queries, 5, True, candidates)[0]
        fired = check_explain(miner, ref, queries, index, 4)[0]
    assert fired.max() >= 2


# ---------------------------------------------------------- 6. range error
def test_path_count_past_32_bits_is_reported(dev):
    from rnnlogic_amd import _native
    from rnnlogic_amd.miner import RuleMiner
    tri = [(0, 0, 3)] + [(0, 1, 1)] * 1700 + [(1, 1, 2)] * 1700 + [(2, 1, 3)] * 1700
    miner = RuleMiner(fake_graph(tri, 4, 2), dev)
    miner.set_logic_rules([[(0, (1, 1, 1))], []])
    miner.set_weights([[0.5], []])
    for call in (lambda: miner.predict_topk([(0, 0, 3)], 2), lambda: miner.explain([(0, 0, 3)], [[3, 2]], 1)):
        with pytest.raises(_native.NativeError) as err:
            call()
        assert err.value.code == _native.RNNL_ERR_RANGE
    miner.set_logic_rules([[(0, (1, 1))], []])  # 1,700^2 fits
    miner.set_weights([[0.5], []])
    index, score, valid, position = miner.predict_topk([(0, 0, 3)], 2)
    assert index.tolist() == [[2, -1]] and score.tolist() == [[0.5 * 1700 * 1700, -math.inf]]
    assert valid.tolist() == [1] and position.tolist() == [-1]
    fired, total, rule, count = miner.explain([(0, 0, 3)], index, 2)
    assert (fired.tolist(), total.tolist()) == ([[1, 0]], [[0.5 * 1700 * 1700, 0.0]])
    assert rule.tolist() == [[[0, -1], [-1, -1]]] and count.tolist() == [[[1700 * 1700, 0], [0, 0]]]


# -------------------------------------------------------- 7. Python errors
def test_bad_arguments_raise(dev):
    miner, _ = make(dev, TINY, 8, 4, TINY_RULES, TINY_WEIGHTS)
    for k in (0, 257, -3):
        with pytest.raises(ValueError):
            miner.predict_topk([(0, 0, 1)], k)
    with pytest.raises(ValueError):
        miner.predict_topk([(0, 0, 1)], 3, candidates="some")
    for q in ([(8, 0, 1)], [(0, 4, 1)], [(0, 0, 8)], [(0, 0, -2)], [(-1, 0, 1)], [(0, 0, 1, 2)]):
        with pytest.raises(ValueError):
            miner.predict_topk(q, 3)
        with pytest.raises(ValueError):
            miner.explain(q, [[1]], 3)
    for c in (0, 17):
        with pytest.raises(ValueError):
            miner.explain([(0, 0, 1)], [[1]], c)
    with pytest.raises(ValueError):
        miner.explain([(0, 0, 1)], [[1], [2]], 3)


# ---------------------------------- 8. predict(output=...) and the command line
def umls_rule_file(dev, tmp_path):
    """(graph, fixture, a miner that has read the rule file, the command line's first arguments)"""
    from rnnlogic_amd.miner import RuleMiner
    graph, fx = real_graph("umls"), fixture("umls")
    rule_file = str(tmp_path / "rules.txt")
    write_rule_file(rule_file, fx["rules"], fx["weights"])
    miner = RuleMiner(graph, dev)
    miner.read_rules(rule_file)
    return graph, fx, miner, ["-data-path", graph.data_path, "-rule-file", rule_file]


def test_predict_file_and_command_line(dev, tmp_path):
    graph, fx, miner, base = umls_rule_file(dev, tmp_path)
    out = miner.predict("test", k=5, explain=2, output=str(tmp_path / "api.tsv"))
    n = int(out["valid"].sum())
    assert out["explain_rule"].shape == (len(graph.test_facts), 2, 3) and n > len(graph.test_facts)
    lines = (tmp_path / "api.tsv").read_text().splitlines()
    assert len(lines) == n
    first = lines[0].split("\t")
    h, r, t = graph.test_facts[0]
    assert first[:3] == [graph.id2entity[h], graph.id2relation[r], "1"] and first[4] == repr(float(out["score"][0, 0]))
    assert first[6].startswith(graph.id2relation[r] + " <- ") and first[6].count(":") == 2
    assert sum(ln.split("\t")[5] == "*" for ln in lines) == int(((out["position"] >= 0) & (out["position"] < 5)).sum())
    got = run_cli(base + ["-predict", "test", "-k", "5", "-explain", "2", "-predictions-file",
                          str(tmp_path / "cli.tsv")], tmp_path)
    assert (tmp_path / "cli.tsv").read_bytes() == (tmp_path / "api.tsv").read_bytes()
    assert got[-1] == "#Predictions written: %d" % n


def test_command_line_answers_a_queries_file(dev, tmp_path):
    """One open and one closed line, in dictionary names."""
    graph, fx, miner, base = umls_rule_file(dev, tmp_path)
    h, r, t = graph.test_facts[0]
    (tmp_path / "q.tsv").write_text("%s\t%s\n%s\t%s\t%s\n" % (graph.id2entity[h], graph.id2relation[r],
                                                            graph.id2entity[h], graph.id2relation[r],
                                                            graph.id2entity[t]))
    want = miner.predict(triples=[(h, r, -1), (h, r, t)], k=10, output=str(tmp_path / "q_api.tsv"))
    got = run_cli(base + ["-queries-file", str(tmp_path / "q.tsv"), "-predictions-file", str(tmp_path / "q_cli.tsv")],
                  tmp_path)
    assert (tmp_path / "q_cli.tsv").read_bytes() == (tmp_path / "q_api.tsv").read_bytes()
    assert got[-1] == "#Predictions written: %d" % int(want["valid"].sum()) and want["position"][0] == -1
    assert want["valid"][0] > 0 and want["valid"][1] > 0


def test_evaluate_command_line_prints_what_it_printed_before(dev, tmp_path):
    import mine_eval_ref
    from rnnlogic_amd.miner import metrics_line
    graph, fx, miner, base = umls_rule_file(dev, tmp_path)
    got = run_cli(base + ["-evaluate", "both"], tmp_path)
    assert got[-3:] == ["#Rules read: %d" % sum(len(x) for x in fx["rules"])] + [
        metrics_line(name, dict(zip(mine_eval_ref.METRIC_NAMES, fx["metrics"][split])))
        for name, split in (("Valid", "valid"), ("Test", "test"))]
    assert not any("Predictions" in ln for ln in got)
