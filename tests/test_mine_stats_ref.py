"""The two restatements of the rule statistics (tests/mine_stats_ref.py) against
each other, and the host side of RuleMiner.rule_stats / confidence /
best_rules: grouping of the rules by body, the confidence arithmetic, the
filters.  No GPU."""
import types

import numpy as np
import pytest

import mine_stats_ref as ms

TINY = [(0, 0, 1), (0, 0, 1), (2, 0, 2), (0, 0, 5), (6, 0, 7), (0, 1, 3), (0, 1, 4), (3, 1, 5), (4, 1, 5), (1, 1, 5),
        (5, 2, 0), (5, 2, 1), (3, 2, 4), (0, 1, 1), (2, 1, 2), (1, 0, 5), (7, 2, 6), (5, 1, 3)]
TINY_RULES = [
    [(0, ()), (0, (1,)), (0, (1, 1)), (0, (1, 2, 1)), (0, (0,)), (0, (1, 1)), (0, (0, 1)), (0, (1, 1, 2)), (0, (3,))],
    [(1, (0,)), (1, (1, 1)), (1, (0, 1)), (1, (1, 2, 0)), (1, ())],
    [(2, (1, 1))],
    [(3, (1,)), (3, (0, 1)), (3, ())],
]


def same(a, b):
    return all(np.array_equal(x, y) for k in ("support", "body", "pca_body") for x, y in zip(a[k], b[k]))


def test_tiny_graph_by_hand_and_both_forms():
    dense, sets = ms.DenseStats(TINY, 8, 4), ms.SetStats(TINY, 8, 4)
    a, b = ms.stats_of(dense, TINY_RULES), ms.stats_of(sets, TINY_RULES)
    assert same(a, b)
    # 0 <- (): D(x) = {x}; (2, 0, 2) is the one self-loop of relation 0; heads with a 0-tail: 0, 1, 2, 6
    assert dense.stats(0, ()) == (1, 8, 4)
    # 0 <- 1: pairs of relation 1: (0,3) (0,4) (0,1) (3,5) (4,5) (1,5) (2,2) (5,3) = 8; known under 0: (0,1) (2,2)
    # (1,5); sources with a 0-tail among 0, 1, 2: 3 + 1 + 1 pairs
    assert dense.stats(0, (1,)) == (3, 8, 5)
    # the duplicate edge (0, 0, 1) counts once
    assert dense.stats(1, (0,)) == (3, 5, 4) and dense.head_pairs().tolist() == [5, 8, 4, 0]
    assert np.array_equal(dense.head_pairs(), sets.head_pairs())
    # relation 3 has rules and no triples: support and pca_body 0, body as any
    assert [int(a["support"][3][k]) for k in range(3)] == [0, 0, 0] and a["pca_body"][3].tolist() == [0, 0, 0]
    assert a["body"][3].tolist() == [8, dense.stats(0, (0, 1))[1], 8]
    assert a["support"][0][2] == a["support"][0][5]  # a copy
    assert a["body"][0][8] == 0  # a body of a relation without edges


@pytest.mark.parametrize("seed,E,R,n", [(1, 30, 3, 120), (2, 61, 5, 400), (3, 17, 2, 200), (4, 90, 6, 300)])
def test_dense_form_equals_set_form_on_random_graphs(seed, E, R, n):
    tri = ms.random_graph(seed, E, R, n)
    rules = ms.random_rules(seed + 10, R, 60, 5)
    a = ms.stats_of(ms.DenseStats(tri, E, R), rules)
    b = ms.stats_of(ms.SetStats(tri, E, R), rules)
    assert same(a, b)
    assert sum(int(x.sum()) for x in a["support"]) > 0
    assert all(np.all(s <= p) and np.all(p <= bd) for s, p, bd in zip(a["support"], a["pca_body"], a["body"]))


def test_rules_are_grouped_by_body_and_copies_share_a_slot():
    from rnnlogic_amd.miner import group_rules
    #        head, body                   the 9 in the second row lies past the body's end
    rules = [(2, (1, 1)), (0, (1, 1)), (1, ()), (2, (1, 1)), (0, (1,)), (1, (1, 1)), (1, (4, 3, 2, 1, 0))]
    head = [hd for hd, _ in rules]
    ln = [len(b) for _, b in rules]
    body = np.zeros((len(rules), 5), dtype=np.int32)
    for i, (_, b) in enumerate(rules):
        body[i, :len(b)] = b
    body[1, 3] = 9
    body_len, body_rel, head_off, head_rel, body_of, slot_of = group_rules(head, ln, body, 5)
    bodies = [tuple(body_rel[i, :body_len[i]].tolist()) for i in range(len(body_len))]
    assert sorted(bodies) == sorted(set(b for _, b in rules)) and len(bodies) == 4
    assert head_off[0] == 0 and np.all(np.diff(head_off) >= 1) and head_off[-1] == len(head_rel) == 6
    for i, (hd, b) in enumerate(rules):
        assert bodies[body_of[i]] == b
        assert head_off[body_of[i]] <= slot_of[i] < head_off[body_of[i] + 1] and head_rel[slot_of[i]] == hd
    k = bodies.index((1, 1))
    assert head_rel[head_off[k]:head_off[k + 1]].tolist() == [0, 1, 2]  # ascending, each once
    assert slot_of[0] == slot_of[3] and body_of[0] == body_of[1] == body_of[5]
    assert not body_rel[body_len[:, None] <= np.arange(5)[None, :]].any()
    # three-relation rows (the lists of a max_body = 3 miner) group the same way
    again = group_rules(head[:6], ln[:6], body[:6, :3], 5)
    assert np.array_equal(again[4], body_of[:6]) and again[1].shape[1] == 5


def test_confidence_arithmetic():
    from rnnlogic_amd.miner import confidence_of, confidences
    sup, bod, pca = [0, 3, 0, 7, 5], [0, 4, 9, 7, 10 ** 15], [0, 3, 0, 7, 3]
    assert confidences("std", sup, bod, pca, 5).tolist() == [0.0, 0.75, 0.0, 1.0, 5.0 / 10 ** 15]
    assert confidences("pca", sup, bod, pca, 5).tolist() == [0.0, 1.0, 0.0, 1.0, 5.0 / 3.0]
    assert confidences("head_coverage", sup, bod, pca, 5).tolist() == [0.0, 0.6, 0.0, 1.4, 1.0]
    assert confidences("head_coverage", [0, 0], [1, 2], [1, 1], 0).tolist() == [0.0, 0.0]  # 0 / 0
    assert confidences("std", sup, bod, pca, 5, pc=2.0).tolist() == [0.0, 0.5, 0.0, 7.0 / 9.0, 5.0 / (10 ** 15 + 2.0)]
    assert confidences("head_coverage", sup, bod, pca, 5, pc=2.0).tolist() == [0.0, 0.6, 0.0, 1.4, 1.0]  # no pc there
    for kind in ("std", "pca", "head_coverage"):
        for pc in (0.0, 0.5):
            got = confidences(kind, sup, bod, pca, 5, pc)
            assert got.dtype == np.float64
            assert np.array_equal(got, ms.confidence(kind, sup, bod, pca, 5, pc if kind != "head_coverage" else 0.0))
    assert confidence_of([1], [0], 0.0).tolist() == [0.0]  # x / 0 cannot come from counts; it is 0.0 too
    with pytest.raises(ValueError):
        confidences("amie", sup, bod, pca, 5)
    with pytest.raises(ValueError):
        confidences("std", sup, bod, pca, 5, pc=-1.0)


def hand_made_miner():
    """Two relations; pool, H and counts by hand, no device."""
    from rnnlogic_amd.miner import RuleMiner
    m = RuleMiner.__new__(RuleMiner)
    m.graph = types.SimpleNamespace(relation_size=2, entity_size=4)
    m.pool = [[(0, (1,)), (0, (1, 1)), (0, (0, 1)), (0, (1, 0))], [(1, (0,)), (1, (0, 0))]]
    m.pool_H = [np.asarray([0.1, 0.4, 0.4, 0.3]), np.asarray([0.9, 0.2])]
    m._searched = 2
    m._pool_arrays = (np.asarray([0, 0, 0, 0, 1, 1]), None, None)
    #                       support                 body                      pca_body
    m._pool_stats = (np.asarray([5, 0, 2, 1, 0, 4]), np.asarray([10, 7, 4, 50, 3, 8]), np.asarray([5, 7, 2, 10, 0, 4]))
    m._head_pairs = np.asarray([6, 4])
    return m


def test_best_rules_filters_before_top_n_out():
    m = hand_made_miner()
    name = lambda out: [(hd, body) for hd, body, _ in out]  # noqa: E731
    assert name(m.best_rules()) == [(0, (1, 1)), (0, (0, 1)), (0, (1, 0)), (0, (1,)), (1, (0,)), (1, (0, 0))]
    assert name(m.best_rules(2)) == [(0, (1, 1)), (0, (0, 1)), (1, (0,)), (1, (0, 0))]
    # support >= 1 drops (0, (1, 1)) and (1, (0,)) first; then the best two of what is left
    assert name(m.best_rules(2, min_support=1)) == [(0, (0, 1)), (0, (1, 0)), (1, (0, 0))]
    # pca: 1.0, 0, 1.0, 0.1, 0, 1.0; std: 0.5, 0, 0.5, 0.02, 0, 0.5
    assert name(m.best_rules(0, min_confidence=0.5)) == [(0, (0, 1)), (0, (1,)), (1, (0, 0))]
    assert name(m.best_rules(0, min_confidence=0.1)) == [(0, (0, 1)), (0, (1, 0)), (0, (1,)), (1, (0, 0))]
    assert name(m.best_rules(0, min_confidence=0.1, confidence="std")) == [(0, (0, 1)), (0, (1,)), (1, (0, 0))]
    assert name(m.best_rules(0, min_confidence=0.51, confidence="std")) == []
    # pc = 2: pca = 5/7, 0, 2/4, 1/12, 0, 4/6
    assert name(m.best_rules(0, min_confidence=0.6, pc=2.0)) == [(0, (1,)), (1, (0, 0))]
    # head coverage: 5/6, 0, 2/6, 1/6 | 0, 1
    assert name(m.best_rules(1, min_support=2, min_confidence=0.5, confidence="head_coverage")) == [(0, (1,)),
                                                                                                   (1, (0, 0))]
    assert [H for _, _, H in m.best_rules(1)] == [0.4, 0.9]


def test_stats_file_lines(tmp_path):
    m = hand_made_miner()
    assert m.out_rule_stats(str(tmp_path / "s.txt"), 1, min_support=1) == 2
    assert m.out_rules(str(tmp_path / "r.txt"), 1, min_support=1) == 2
    lines = (tmp_path / "s.txt").read_text().splitlines()
    assert lines == ["0 0 1 0.4000000000000000 2 4 2 0.5000000000000000 1.0000000000000000",
                     "1 0 0 0.2000000000000000 4 8 4 0.5000000000000000 1.0000000000000000"]
    assert [" ".join(ln.split()[:-5]) for ln in lines] == (tmp_path / "r.txt").read_text().splitlines()


def test_shipped_rule_files():
    """Every rule of a shipped mined_rules.txt was mined from a train triple, so
    its support is at least 1 — the lines are 'head body...' without an H
    column.  The prototype of the statistics counted 976 of 3,053 (UMLS) and
    1,592 of 2,500 (kinship) rules with support 0: it read the lines as
    out_rules writes them, 'head body... H', and so left the last body
    relation out.  Both readings are restated here."""
    from rnnlogic_amd import datasets
    from rnnlogic_amd.data import KnowledgeGraph
    from rnnlogic_amd.miner import read_rule_file
    for data, n_rules, prototype in (("umls", 3053, 976), ("kinship", 2500, 1592)):
        graph = KnowledgeGraph(datasets.materialize(data))
        rules, _ = read_rule_file(datasets.rule_file(data), graph.relation_size, 5)
        flat = [rule for per in rules for rule in per]
        assert len(flat) == n_rules
        ref = ms.DenseStats(graph.train_facts, graph.entity_size, graph.relation_size)
        assert sum(ref.stats(hd, body)[0] == 0 for hd, body in flat) == 0
        assert sum(ref.stats(hd, body[:-1])[0] == 0 for hd, body in flat) == prototype
