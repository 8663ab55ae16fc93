"""The restatement of the miner's aggregations (tests/mine_agg_ref.py) on its
own: its three modes on small cases worked by hand, the head side two ways,
and — non-vacuity — that the inputs of tests/test_gpu_mine_agg.py can tell the
modes and the depths apart, so a mode that silently fell back to the sum, or a
depth that was ignored, could not pass there.  Needs no GPU.
"""
import math

import mine_agg_ref as A
import mine_eval_ref


def tiny(side):
    ref = A.make_ref(side, A.TINY, 8, 4)
    ref.set_rules(A.TINY_RULES, A.TINY_WEIGHTS)
    return ref


def pairs_by_mode(ref, q, filtered):
    return {md: ref.set_mode(*md).pair(*q, filtered=filtered) for md in A.MODES}


def test_sum_mode_is_the_evaluation_restatement():
    ref = tiny("tail")
    plain = mine_eval_ref.MineEvalRef(A.TINY, 8, 4)
    plain.set_rules(A.TINY_RULES, A.TINY_WEIGHTS)
    for q in A.TINY_QUERIES:
        assert ref.scores(*q) == plain.scores(*q) and ref.pair(*q) == plain.pair(*q)


def test_noisy_or_and_max_by_hand():
    ref = tiny("tail")
    # (0, 3, 3), nothing removed: (1,) reaches 1, 3, 4; (0, 1) reaches 3 and 5; (1, 1) reaches 5; (1, 2, 1) reaches 5
    u = -math.log1p(-0.7)
    val = ref.set_mode("noisy_or").scores(0, 3, 3)
    assert val == [0.0, u, 0.0, u + u, u, 0.0 + u + u + u, 0.0, 0.0]
    assert [A.key_fields(v) for v in ref.set_mode("max", 3).scores(0, 3, 3)] == \
        [(0, 0, 0), (1, 0, 0), (0, 0, 0), (1, 1, 0), (1, 0, 0), (1, 1, 1), (0, 0, 0), (0, 0, 0)]
    assert [A.key_fields(v) for v in ref.set_mode("max", 2).scores(0, 3, 3)][5] == (1, 1, 0)
    assert [A.key_fields(v) for v in ref.set_mode("max", 1).scores(0, 3, 3)][5] == (1, 0, 0)
    # the clamp: a weight of 1 is the finite -log(2^-53)
    assert A.noisy_or_u(1.0) == 53 * math.log(2.0) and A.noisy_or_u(0.0) == 0.0
    # classes: equal weights share one, 0 has none
    assert A.classes_of([1.0, .5, .5, .25, 0, .5]) == ([3, 2, 2, 1, 0, 2], [.25, .5, 1.0])
    assert A.max_key([2, 0, 3, 2, 1], 3) == float((3 << 34) | (2 << 17) | 2) and A.max_key([0], 3) == 0.0
    # explain: the firing rules by operand, ties by list index, count 1, total = val
    ref.set_mode("max", 3)
    assert ref.explain(0, 3, 3, 5, 2) == (3, float((1 << 34) | (1 << 17) | 1), [1, 2], [1, 1])
    assert ref.explain(0, 3, 3, 0, 2) == (0, 0.0, [-1, -1], [0, 0])
    ref.set_mode("noisy_or")
    assert ref.explain(0, 0, 5, 1, 3)[1] == ref.scores(0, 0, 5)[1]


def test_max_key_does_not_depend_on_list_order():
    ref, rev = tiny("tail"), A.make_ref("tail", A.TINY, 8, 4)
    rev.set_rules([list(reversed(rs)) for rs in A.TINY_RULES], [list(reversed(ws)) for ws in A.TINY_WEIGHTS])
    for q in A.TINY_QUERIES:
        assert ref.set_mode("max", 3).scores(*q) == rev.set_mode("max", 3).scores(*q)


def test_head_side_is_the_naive_definition():
    """val[e] from the forward groundings of every candidate e, read at t."""
    ref = tiny("head")
    g = ref.T.g.__class__(A.TINY, 8, 4)  # mine_ref.MineRef on the graph as given
    for mode, depth in A.MODES[1:]:
        ref.set_mode(mode, depth)
        for h, r, t in A.TINY_QUERIES:
            want = []
            for e in range(8):
                ks = [k for k, (_, body) in enumerate(A.TINY_RULES[r])
                      if any(d == t and n > 0 for d, n in g.destinations(e, body, (h, r, t)))]
                want.append(ref.T.combine(r, ks) if ks else 0.0)
            assert ref.scores(h, r, t) == want


def test_the_gpu_inputs_tell_the_modes_apart():
    ref = tiny("tail")
    p = pairs_by_mode(ref, (0, 0, 1), False)
    assert p[("sum", 1)] == (1, 2) and p[("noisy_or", 1)] == (0, 1)       # sum against noisy-or
    assert p[("max", 1)] == (0, 2) and p[("max", 2)] == (0, 1)             # depth 1 against depth 2
    p = pairs_by_mode(ref, (0, 0, 5), False)
    assert p[("max", 1)] == (2, 5) and p[("max", 2)] == (2, 3)
    p = pairs_by_mode(ref, (0, 3, 3), False)
    assert p[("max", 2)] == (0, 2) and p[("max", 3)] == (1, 2)             # depth 2 against depth 3
    keys = [A.key_fields(v) for q in A.TINY_QUERIES for v in ref.set_mode("max", 3).scores(*q)]
    assert any(c1 == c2 > 0 for c1, c2, _ in keys) and any(c1 > c2 > c3 > 0 for c1, c2, c3 in keys)
    head = tiny("head")
    p = pairs_by_mode(head, (0, 1, 5), False)
    assert p[("max", 2)] == (0, 2) and p[("max", 3)] == (0, 1)
    p = pairs_by_mode(head, (1, 1, 5), False)
    assert p[("sum", 1)] != p[("noisy_or", 1)] and p[("noisy_or", 1)] != p[("max", 1)]
    # filtered and unfiltered differ somewhere in every mode
    for md in A.MODES:
        ref.set_mode(*md)
        assert ref.pairs(A.TINY_QUERIES, True) != ref.pairs(A.TINY_QUERIES, False)


def test_the_larger_gpu_inputs_tell_the_modes_apart():
    tri, E, R, rules = A.many_rules_graph()
    ref = A.make_ref("tail", tri, E, R)
    ref.set_rules(rules, A.confidence_like_weights(rules, 1))
    queries = [(h, 0, t) for h in range(E) for t in (0, 5)]
    got = {md: ref.set_mode(*md).pairs(queries, False) for md in A.MODES}
    assert len(set(map(tuple, got.values()))) == len(A.MODES)  # every mode and depth ranks differently somewhere
    tri, E, R, rules, mids = A.spread_graph(513)
    ref = A.make_ref("tail", tri, E, R)
    ref.set_rules(rules, A.SPREAD_W)
    got = {md: ref.set_mode(*md).pairs(A.spread_queries(E, mids), False) for md in A.MODES[:4]}
    assert got[("sum", 1)] != got[("noisy_or", 1)] and got[("noisy_or", 1)] != got[("max", 1)]
    assert got[("max", 1)] != got[("max", 2)]
