"""The miner's head queries (?, r, t) on the GPU — RuleMiner.scores / eval_ranks
/ evaluate / predict_topk / explain / predict with side="head" and the command
line's -side (rnnl_miner_evaluate_side / _predict_side / _explain_side,
csrc/mine_ground.h) — against the two restatements of tests/mine_head_ref.py
and against the tail side of the transposed graph on the GPU itself.

No tolerances: scores and totals are compared bit for bit; pairs, lists,
positions, fired, rule and count exactly.  The graphs are copies of those of
test_gpu_mine_eval.py (mine_head_ref.py holds them).
"""
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import mine_eval_ref
import mine_head_ref
from conftest import GOLDEN, REPO
from mine_head_ref import TINY, TINY_QUERIES, TINY_RULES, TINY_WEIGHTS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def fake_graph(triples, E, R, **more):
    return types.SimpleNamespace(train_facts=[tuple(t) for t in triples], entity_size=E, relation_size=R, **more)


def make(dev, triples, E, R, rules, weights, known=None, max_body=3, **more):
    """(a miner, restatement (b)) with the same rules and weights."""
    from rnnlogic_amd.miner import RuleMiner
    miner = RuleMiner(fake_graph(triples, E, R, **more), dev, max_body=max_body)
    miner.set_logic_rules(rules)
    miner.set_weights(weights)
    ref = mine_head_ref.HeadRef(triples, E, R, known=known)
    ref.set_rules(rules, weights)
    return miner, ref


def check_scores_and_pairs(miner, ref, queries, E):
    """scores bitwise, pairs exactly, filtered and unfiltered; returns (val, {filtered: pairs})."""
    want = np.asarray([ref.scores(*q) for q in queries], dtype=np.float64).reshape(len(queries), E)
    got = miner.scores(queries, side="head").cpu().numpy()
    assert got.dtype == np.float64 and same_bits(got, want)
    out = {}
    for filtered in (True, False):
        pairs = miner.eval_ranks(queries, filtered=filtered, side="head")
        assert pairs.dtype == np.int64
        assert np.array_equal(pairs, np.asarray(ref.pairs(queries, filtered), dtype=np.int64).reshape(-1, 2))
        assert np.all(pairs[:, 1] - pairs[:, 0] >= 1)
        out[filtered] = pairs
    return got, out


def check_topk(miner, ref, queries, k, filtered, candidates):
    index, score, valid, position = (x.cpu().numpy()
                                     for x in miner.predict_topk(queries, k, filtered, candidates, side="head"))
    want = [ref.topk(h, r, t, k, filtered, candidates) for h, r, t in queries]
    assert index.dtype == np.int32 and score.dtype == np.float64 and index.shape == score.shape == (len(want), k)
    assert np.array_equal(index, np.asarray([w[0] for w in want], dtype=np.int32).reshape(-1, k))
    assert same_bits(score, np.asarray([w[1] for w in want], dtype=np.float64).reshape(-1, k))
    assert valid.tolist() == [w[2] for w in want] and position.tolist() == [w[3] for w in want]
    return index, score, valid, position


def check_explain(miner, ref, queries, index, c):
    fired, total, rule, count = (x.cpu().numpy() for x in miner.explain(queries, index, c, side="head"))
    assert rule.dtype == np.int32 and count.dtype == np.int64 and rule.shape == count.shape == index.shape + (c,)
    for i, (h, r, t) in enumerate(queries):
        for j, e in enumerate(np.asarray(index)[i].tolist()):
            w = ref.explain(h, r, t, e, c)
            assert (int(fired[i, j]), rule[i, j].tolist(), count[i, j].tolist()) == (w[0], w[2], w[3])
            assert same_bits(total[i, j], w[1])
    return fired, total, rule, count


# --------------------------------------------------------------- 1. tiny graph
def test_tiny_graph_against_the_naive_definition(dev):
    """The duplicate train edge, the self-loop with h == t, an anchor whose only
    in-edge is the query's own, a relation without rules and one without
    triples; bodies of four and five relations."""
    miner, b = make(dev, TINY, 8, 4, TINY_RULES, TINY_WEIGHTS, max_body=5)
    a = mine_head_ref.NaiveHeadRef(TINY, 8, 4)
    a.set_rules(TINY_RULES, TINY_WEIGHTS)
    assert len(TINY_QUERIES) == 12 and max(len(body) for _, body in TINY_RULES[0]) == 5
    val, pairs = check_scores_and_pairs(miner, a, TINY_QUERIES, 8)
    check_scores_and_pairs(miner, b, TINY_QUERIES, 8)
    tail = miner.scores(TINY_QUERIES).cpu().numpy()
    assert sum(not same_bits(val[i], tail[i]) for i in range(12)) == 8  # the head side is another answer
    for i, (h, r, t) in enumerate(TINY_QUERIES):
        assert same_bits(val[i, h], tail[i, t])  # the same paths h -> t
    assert not val[3].any() and pairs[False][3].tolist() == [0, 8]  # no rules
    assert not val[5].any()  # (6, 0, 7): its own edge is all that enters 7
    assert val[6].tolist() == [0.0, 0.0, 0.5, 0.0, 0.0, 0.0, 0.0, 0.0]  # (2, 0, 2): 2 -1-> 2 stays, the loop is removed
    assert pairs[True][1].tolist() == [6, 7] and pairs[False][1].tolist() == [7, 8]  # (1, 0, 5) is known
    for k in (1, 3, 8, 20):
        for filtered in (True, False):
            for candidates in ("reached", "all"):
                index = check_topk(miner, b, TINY_QUERIES, k, filtered, candidates)[0]
                check_explain(miner, b, TINY_QUERIES, index[:, :min(k, 4)].copy(), 3)


def test_tiny_graph_filters_by_known_heads_of_valid_and_test_too(dev):
    valid, test = [(3, 0, 1), (4, 0, 5)], [(1, 0, 5), (3, 0, 6)]
    queries = TINY_QUERIES + valid + test
    miner, ref = make(dev, TINY, 8, 4, TINY_RULES, TINY_WEIGHTS, known=TINY + valid + test, max_body=5,
                      valid_facts=valid, test_facts=test)
    a = mine_head_ref.NaiveHeadRef(TINY, 8, 4, known=TINY + valid + test)
    a.set_rules(TINY_RULES, TINY_WEIGHTS)
    _, pairs = check_scores_and_pairs(miner, a, queries, 8)
    plain, plain_ref = make(dev, TINY, 8, 4, TINY_RULES, TINY_WEIGHTS, max_body=5)
    _, train_only = check_scores_and_pairs(plain, plain_ref, queries, 8)
    assert not np.array_equal(pairs[True], train_only[True]) and np.array_equal(pairs[False], train_only[False])
    assert pairs[True][1].tolist() == [5, 6]  # (0, 0, 5): the heads 1 and 4 have left
    check_topk(miner, ref, queries, 8, True, "all")


# ------------------------------- 2. transposition on the reference fixtures
_real = {}


def real(data, dev):
    """(graph, fixture, miner on G, miner on the transposed graph with reversed bodies), once per dataset."""
    if data not in _real:
        from rnnlogic_amd import datasets
        from rnnlogic_amd.data import KnowledgeGraph
        from rnnlogic_amd.miner import RuleMiner
        graph = KnowledgeGraph(datasets.materialize(data))
        fx = mine_eval_ref.load_fixture(os.path.join(GOLDEN, "_mine_eval_%s.npz" % data))
        miner = RuleMiner(graph, dev)
        miner.set_logic_rules(fx["rules"])
        miner.set_weights(fx["weights"])
        flipped = RuleMiner(fake_graph(mine_head_ref.transpose(graph.train_facts), graph.entity_size,
                                       graph.relation_size, valid_facts=mine_head_ref.transpose(graph.valid_facts),
                                       test_facts=mine_head_ref.transpose(graph.test_facts)), dev)
        flipped.set_logic_rules(mine_head_ref.reverse_rules(fx["rules"]))
        flipped.set_weights(fx["weights"])
        _real[data] = (graph, fx, miner, flipped)
    return _real[data]


@pytest.mark.parametrize("data", ["kinship", "umls"])
def test_head_side_is_the_tail_side_of_the_transposed_graph(data, dev):
    graph, fx, miner, flipped = real(data, dev)
    q = graph.test_facts
    qt = mine_head_ref.transpose(q)
    n = len(q)
    assert graph.entity_size <= 2100 and n > 500
    head = miner.scores(q, side="head")
    assert torch.equal(head.view(torch.int64), flipped.scores(qt).view(torch.int64)) and bool(head.any())
    tail = miner.scores(q)
    rows = torch.arange(n, device=head.device)
    hs = torch.as_tensor([h for h, _, _ in q], device=head.device)
    ts = torch.as_tensor([t for _, _, t in q], device=head.device)
    assert torch.equal(head[rows, hs].view(torch.int64), tail[rows, ts].view(torch.int64))  # on every triple
    differ = int((head.view(torch.int64) != tail.view(torch.int64)).any(1).sum())
    print("%s: %d of %d head rows differ from the tail rows" % (data, differ, n))
    assert differ > n // 2
    del head, tail
    differ = 0
    for filtered in (True, False):
        pairs = miner.eval_ranks(q, filtered=filtered, side="head")
        assert np.array_equal(pairs, flipped.eval_ranks(qt, filtered=filtered))
        differ += int((pairs != miner.eval_ranks(q, filtered=filtered)).any(1).sum())
    assert differ > n // 2
    # the tail side says what the reference said, with and without the argument
    assert np.array_equal(miner.eval_ranks(q), fx["pairs"]["test"])
    assert np.array_equal(miner.eval_ranks(q, side="tail"), fx["pairs"]["test"])
    for candidates in ("reached", "all"):
        got = miner.predict_topk(q, 10, True, candidates, side="head")
        want = flipped.predict_topk(qt, 10, True, candidates)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int64), want[1].view(torch.int64))
        assert torch.equal(got[2], want[2]) and torch.equal(got[3], want[3])
        assert int(got[2].max()) == 10 and int((got[3] >= 0).sum()) > 0
        first = got[0][:, :3].contiguous()
        ex, ex_want = miner.explain(q, first, 3, side="head"), flipped.explain(qt, first, 3)
        assert torch.equal(ex[1].view(torch.int64), ex_want[1].view(torch.int64)) and int(ex[0].max()) > 1
        assert all(torch.equal(x, y) for x, y in zip((ex[0], ex[2], ex[3]), (ex_want[0], ex_want[2], ex_want[3])))


# ------------------------------------------- 3. the LDS and the global regime
@pytest.mark.parametrize("E", [512, 513, 2100])
def test_entities_in_lds_and_in_global_memory(dev, E):
    """512 entities are the most the LDS arrays hold; from 513 on they are
    per-workgroup global memory.  Entity 5 has 100 in-edges of relation 2: the
    backward frontier of 0 <- 1 2 passes the 64 lanes of a wave."""
    tri, E, R, rules, mids = mine_head_ref.spread_graph(E)
    miner, ref = make(dev, tri, E, R, rules, mine_head_ref.SPREAD_W)
    assert len(mids) == 100 and sum(1 for h, r, t in tri if t == 5 and r == 2) == 100
    closed = [(0, 0, 5), (5, 0, E - 1), (E - 1, 2, 0), (0, 1, E - 1), (5, 2, E - 3), (mids[50], 0, 5), (0, 0, 5)]
    val, pairs = check_scores_and_pairs(miner, ref, closed, E)
    assert val[0][0] == -0.25 * 100 + 0.125 * 100  # 0 -1-> 100 mids -2-> 5, the rule listed twice
    assert val[0][mids[3]] == 0.5 and val[0][E - 1] == 0.0  # mids -2-> 5 by 0 <- 2
    queries = closed + [(-1, 0, 5), (-1, 0, E - 1), (-1, 2, 0), (-1, 1, E - 1), (-1, 2, E - 3)]
    for k in (10, 104, 200):
        for candidates in ("reached", "all"):
            index, score, valid, position = check_topk(miner, ref, queries, k, True, candidates)
            assert np.all(position[len(closed):] == -1)
        assert valid[0] == min(k, E)
    check_topk(miner, ref, queries, 64, False, "reached")
    check_explain(miner, ref, queries, index[:, :3].copy(), 3)


# -------------------------------------------- 4. more rules than a round holds
def test_more_rules_than_a_round(dev):
    tri, E, R, rules = mine_head_ref.many_rules_graph()
    assert len(rules[0]) == 1110
    queries = tri + [(h, 0, t) for h in range(E) for t in (0, 5)]
    miner, ref = make(dev, tri, E, R, rules, mine_head_ref.quantised_weights(rules, 1))
    _, pairs = check_scores_and_pairs(miner, ref, queries, E)
    assert np.any(pairs[True][:, 1] - pairs[True][:, 0] > 1) and np.any(pairs[True][:, 0] > 0)
    some = tri[:4] + [(h, 0, 5) for h in range(4)] + [(-1, 0, 1)]
    index = check_topk(miner, ref, some, 3, True, "reached")[0]
    for c in (1, 16):
        fired = check_explain(miner, ref, some, index, c)[0]
    assert fired.max() >= 100


# ---------------------------------------------------------------- 5. range
def test_path_count_past_32_bits_is_reported(dev):
    """1,700 parallel edges on each of three hops, walked backward from 3: 1,700^3 > 2^32 paths at 0."""
    from rnnlogic_amd import _native
    from rnnlogic_amd.miner import RuleMiner
    tri = [(0, 0, 3)] + [(0, 1, 1)] * 1700 + [(1, 1, 2)] * 1700 + [(2, 1, 3)] * 1700
    miner = RuleMiner(fake_graph(tri, 4, 2), dev)
    miner.set_logic_rules([[(0, (1, 1, 1))], []])
    miner.set_weights([[0.5], []])
    for call in (lambda: miner.eval_ranks([(0, 0, 3)], side="head"), lambda: miner.scores([(0, 0, 3)], side="head"),
                 lambda: miner.predict_topk([(0, 0, 3)], 2, side="head"),
                 lambda: miner.explain([(0, 0, 3)], [[0, 1]], 1, side="head")):
        with pytest.raises(_native.NativeError) as err:
            call()
        assert err.value.code == _native.RNNL_ERR_RANGE
    miner.set_logic_rules([[(0, (1, 1))], []])  # 1,700^2 fits: 1 -1-> 2 -1-> 3
    miner.set_weights([[0.5], []])
    assert miner.scores([(0, 0, 3)], side="head").cpu().numpy().tolist() == [[0.0, 0.5 * 1700 * 1700, 0.0, 0.0]]
    assert miner.eval_ranks([(0, 0, 3)], side="head").tolist() == [[1, 4]]
    index, score, valid, position = miner.predict_topk([(0, 0, 3)], 2, side="head")
    assert index.tolist() == [[1, -1]] and score.tolist() == [[0.5 * 1700 * 1700, -math.inf]]
    assert valid.tolist() == [1] and position.tolist() == [-1]
    fired, total, rule, count = miner.explain([(0, 0, 3)], index, 2, side="head")
    assert (fired.tolist(), total.tolist()) == ([[1, 0]], [[0.5 * 1700 * 1700, 0.0]])
    assert rule.tolist() == [[[0, -1], [-1, -1]]] and count.tolist() == [[[1700 * 1700, 0], [0, 0]]]


# ---------------------------------------------------- 6. open head queries
def test_open_head_queries(dev):
    miner, ref = make(dev, TINY, 8, 4, TINY_RULES, TINY_WEIGHTS, max_body=5)
    closed = [(0, 0, 1), (3, 0, 6), (0, 1, 5), (4, 1, 5), (2, 0, 2)]
    opened = [(-1, r, t) for _, r, t in closed]
    got = {}
    for name, q in (("closed", closed), ("open", opened)):
        got[name] = check_topk(miner, ref, q, 8, False, "all")
        check_explain(miner, ref, q, got[name][0][:, :4].copy(), 3)
    assert np.all(got["open"][3] == -1) and np.all(got["closed"][3] >= 0)
    # (3, 0, 6) and (0, 1, 5) are no train triples: no edge to remove, the lists are the open query's
    for i in (1, 2):
        assert np.array_equal(got["open"][0][i], got["closed"][0][i]) and same_bits(got["open"][1][i],
                                                                                   got["closed"][1][i])
    # (0, 0, 1) lies on paths into 1 (0 <- 0), (4, 1, 5) on paths into 5: removing them changes the scores
    for i in (0, 3):
        assert not same_bits(got["open"][1][i], got["closed"][1][i])
    # the open score row is the closed row of a triple that is not in the graph: no edge is removed
    assert (7, 0, 1) not in TINY
    row = miner.scores([(7, 0, 1)], side="head").cpu().numpy()[0]
    index, score, valid = got["open"][0][0], got["open"][1][0], got["open"][2][0]
    assert valid == 8 and same_bits(score, row[index])
    with pytest.raises(ValueError):
        miner.predict_topk([(0, 0)], 3, side="head")  # (h, r) is the tail side's open form
    with pytest.raises(ValueError):
        miner.predict_topk([(0, 0, -1)], 3, side="head")
    with pytest.raises(ValueError):
        miner.eval_ranks([(-1, 0, 1)], side="head")  # evaluation takes no open queries


# ------------------------------------------------- 7. evaluate(side="both")
def test_evaluate_both_sides(dev):
    from rnnlogic_amd.miner import expectation_metrics
    graph, fx, miner, _ = real("kinship", dev)
    E, n = graph.entity_size, len(graph.test_facts)
    tails, heads = miner.eval_ranks(graph.test_facts), miner.eval_ranks(graph.test_facts, side="head")
    both = miner.evaluate("test", side="both")
    assert both == expectation_metrics(np.concatenate([tails, heads]), E) and both["n"] == 2 * n
    assert miner.evaluate("test") == miner.evaluate("test", side="tail") == expectation_metrics(tails, E)
    ref = mine_head_ref.HeadRef(graph.train_facts, E, graph.relation_size,
                                known=graph.train_facts + graph.valid_facts + graph.test_facts)
    ref.set_rules(fx["rules"], fx["weights"])
    want = ref.pairs(graph.test_facts)
    assert np.array_equal(heads, np.asarray(want, dtype=np.int64))
    head = miner.evaluate("test", side="head")
    assert tuple(head[k] for k in mine_eval_ref.METRIC_NAMES) == mine_eval_ref.metrics(want, E) and head["n"] == n
    assert head["mrr"] != miner.evaluate("test")["mrr"]
    sub = graph.valid_facts[:50]
    assert miner.evaluate(triples=sub, filtered=False, side="both") == expectation_metrics(
        np.concatenate([miner.eval_ranks(sub, False), miner.eval_ranks(sub, False, "head")]), E)


# ----------------------------------------------- 8. after set_logic_rules
def test_head_queries_after_the_rules_are_set_again(dev):
    """set_logic_rules rebuilds the handle's rule state: the sorted in-edges are carried over."""
    miner, ref = make(dev, TINY, 8, 4, TINY_RULES, TINY_WEIGHTS, max_body=5)
    other = [[(0, b) for _, b in TINY_RULES[1]], [(1, b) for _, b in TINY_RULES[0][1:5]], [], []]
    miner.set_logic_rules(other)
    miner.set_logic_rules(TINY_RULES)
    assert not miner.scores(TINY_QUERIES, side="head").cpu().numpy().any()  # the weights were cleared
    miner.set_weights(TINY_WEIGHTS)
    check_scores_and_pairs(miner, ref, TINY_QUERIES, 8)
    check_topk(miner, ref, TINY_QUERIES + [(-1, 0, 5)], 8, True, "reached")
    weights = [[0.5, -1.0, 0.25, 2.0], [1.0, 0.5, -0.5, 0.125], [], []]
    miner.set_logic_rules(other)
    miner.set_weights(weights)
    ref.set_rules(other, weights)
    val, _ = check_scores_and_pairs(miner, ref, TINY_QUERIES, 8)
    assert val.any()


# --------------------------------------------------------- 9. repeatability
def test_two_calls_are_bitwise_equal(dev):
    graph, fx, miner, _ = real("kinship", dev)
    q = graph.test_facts
    s = [miner.scores(q, side="head").cpu().numpy() for _ in range(2)]
    p = [miner.eval_ranks(q, side="head") for _ in range(2)]
    assert s[0].any() and same_bits(s[0], s[1]) and np.array_equal(p[0], p[1])
    k = [miner.predict_topk(q, 10, True, "all", side="head") for _ in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(*k))
    e = [miner.explain(q, k[0][0][:, :4].contiguous(), 3, side="head") for _ in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(*e))


# ------------------------------------------------------- 10. command line
def run_cli(args, cwd):
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "rnnlogic_amd.miner"] + args, check=True, env=env, cwd=str(cwd),
                          timeout=300, capture_output=True, text=True).stdout.splitlines()


def umls_rule_file(dev, tmp_path):
    graph, fx, miner, _ = real("umls", dev)
    rule_file = str(tmp_path / "rules.txt")
    with open(rule_file, "w") as fo:
        for rules, ws in zip(fx["rules"], fx["weights"]):
            for (hd, body), w in zip(rules, ws):
                fo.write("%d%s %r\n" % (hd, "".join(" %d" % b for b in body), float(w)))  # repr round-trips
    return graph, fx, miner, ["-data-path", graph.data_path, "-rule-file", rule_file]


def test_command_line_evaluates_both_sides(dev, tmp_path):
    from rnnlogic_amd.miner import metrics_line
    graph, fx, miner, base = umls_rule_file(dev, tmp_path)
    got = run_cli(base + ["-evaluate", "test", "-side", "both"], tmp_path)
    want = [metrics_line("Test (%s)" % name, miner.evaluate("test", side=side))
            for name, side in (("tails", "tail"), ("heads", "head"), ("both", "both"))]
    assert got[-4:] == ["#Rules read: %d" % sum(len(x) for x in fx["rules"])] + want
    assert want[0] == metrics_line("Test (tails)", dict(zip(mine_eval_ref.METRIC_NAMES, fx["metrics"]["test"])))
    assert want[1].startswith("Test (heads) | MR ") and want[1].split("|")[1] != want[0].split("|")[1]


def test_command_line_without_side_says_what_it_said(dev, tmp_path):
    from rnnlogic_amd.miner import metrics_line
    graph, fx, miner, base = umls_rule_file(dev, tmp_path)
    out = miner.predict("test", k=5, explain=2, output=str(tmp_path / "api.tsv"))
    again = miner.predict("test", k=5, explain=2, output=str(tmp_path / "api_tail.tsv"), side="tail")
    assert (tmp_path / "api.tsv").read_bytes() == (tmp_path / "api_tail.tsv").read_bytes()
    first = (tmp_path / "api.tsv").read_text().splitlines()[0].split("\t")
    h, r, t = graph.test_facts[0]
    assert first[:3] == [graph.id2entity[h], graph.id2relation[r], "1"]  # head, relation, place: the tail format
    assert first[3] == graph.id2entity[int(out["index"][0, 0])] and np.array_equal(out["index"], again["index"])
    got = run_cli(base + ["-evaluate", "test", "-predict", "test", "-k", "5", "-explain", "2", "-predictions-file",
                          str(tmp_path / "cli.tsv")], tmp_path)
    assert (tmp_path / "cli.tsv").read_bytes() == (tmp_path / "api.tsv").read_bytes()
    assert got[-3:] == ["#Rules read: %d" % sum(len(x) for x in fx["rules"]),
                        metrics_line("Test", dict(zip(mine_eval_ref.METRIC_NAMES, fx["metrics"]["test"]))),
                        "#Predictions written: %d" % int(out["valid"].sum())]


def test_command_line_answers_head_queries_from_a_file(dev, tmp_path):
    """One open and one closed line, in dictionary names; the lines keep the triple's orientation."""
    graph, fx, miner, base = umls_rule_file(dev, tmp_path)
    h, r, t = graph.test_facts[0]
    (tmp_path / "q.tsv").write_text("\t%s\t%s\n%s\t%s\t%s\n" % (graph.id2relation[r], graph.id2entity[t],
                                                              graph.id2entity[h], graph.id2relation[r],
                                                              graph.id2entity[t]))
    want = miner.predict(triples=[(-1, r, t), (h, r, t)], k=10, explain=2, output=str(tmp_path / "q_api.tsv"),
                         side="head")
    got = run_cli(base + ["-side", "head", "-queries-file", str(tmp_path / "q.tsv"), "-explain", "2",
                          "-predictions-file", str(tmp_path / "q_cli.tsv")], tmp_path)
    assert (tmp_path / "q_cli.tsv").read_bytes() == (tmp_path / "q_api.tsv").read_bytes()
    assert got[-1] == "#Predictions written: %d" % int(want["valid"].sum())
    assert want["position"][0] == -1 and want["valid"][0] > 0 and want["valid"][1] > 0
    topk = miner.predict_topk([(-1, r, t), (h, r, t)], 10, side="head")
    assert np.array_equal(want["index"], topk[0].cpu().numpy()) and same_bits(want["score"], topk[1].cpu().numpy())
    lines = [ln.split("\t") for ln in (tmp_path / "q_cli.tsv").read_text().splitlines()]
    assert len(lines) == int(want["valid"].sum())
    n0 = int(want["valid"][0])
    for j, cols in enumerate(lines[:n0]):
        e = int(want["index"][0, j])
        assert cols[:6] == [graph.id2entity[e], graph.id2relation[r], "h%d" % (j + 1), graph.id2entity[t],
                            repr(float(want["score"][0, j])), ""]
    for j, cols in enumerate(lines[n0:]):
        e = int(want["index"][1, j])
        assert cols[:6] == [graph.id2entity[e], graph.id2relation[r], "h%d" % (j + 1), graph.id2entity[t],
                            repr(float(want["score"][1, j])), "*" if e == h else ""]
    assert lines[0][6].startswith(graph.id2relation[r] + " <- ") and lines[0][6].count(":") == 2
    assert sum(cols[5] == "*" for cols in lines) == int(0 <= want["position"][1] < 10)
