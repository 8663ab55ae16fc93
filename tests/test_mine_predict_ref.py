"""The restatement tests/mine_predict_ref.py itself, without a GPU: hand-worked
cases on the 8-entity TINY graph of test_gpu_mine_eval.py (restated here), and
the invariants that tie it to the evaluation's restatement mine_eval_ref.py.
"""
import math
import struct

import mine_eval_ref
import mine_predict_ref

# relation 2 has triples but no rules, relation 3 rules but no triples; (0,0,1) is there twice; (2,0,2) is a
# self-loop; 0 -1-> {3,4} -1-> 5 are two parallel paths; nothing but its own edge leaves 6
TINY = [(0, 0, 1), (0, 0, 1), (2, 0, 2), (0, 0, 5), (6, 0, 7), (0, 1, 3), (0, 1, 4), (3, 1, 5), (4, 1, 5), (1, 1, 5),
        (5, 2, 0), (5, 2, 1), (3, 2, 4), (0, 1, 1), (2, 1, 2), (1, 0, 5), (7, 2, 6), (5, 1, 3)]
TINY_RULES = [
    [(0, ()), (0, (1,)), (0, (1, 1)), (0, (1, 2, 1)), (0, (0,)), (0, (1, 1)), (0, (0, 1)), (0, (1, 1, 2)), (0, (3,))],
    [(1, (0,)), (1, (1, 1)), (1, (0, 1)), (1, (1, 2, 0))],
    [],
    [(3, (1,)), (3, (0, 1))],
]
TINY_WEIGHTS = [[3.0, 0.5, 0.5, -0.25, 0.0, -0.5, 0.1, 0.30000000000000004, 1.0], [1.0, -0.25, 0.5, 0.5], [],
                [0.7, -0.7]]
TINY_QUERIES = [(0, 0, 1), (0, 0, 5), (3, 0, 6), (5, 2, 0), (0, 0, 7), (0, 0, 1), (6, 0, 7), (2, 0, 2), (0, 1, 5),
                (0, 3, 3), (5, 2, 0)]


def bits(x):
    return struct.pack("<d", x)


def tiny():
    ref = mine_predict_ref.MinePredictRef(TINY, 8, 4)
    ref.set_rules(TINY_RULES, TINY_WEIGHTS)
    return ref


def test_hand_worked_closed_query():
    """(0, 0, 1), both copies of the edge removed.  By hand: 0 -1-> {1, 3, 4};
    (1, 1) arrives at 5 along three paths, (1, 2, 1) along one, (0,) reaches 5
    alone (weight 0.0), (0, 1) goes on to 3, (1, 1, 2) returns to 0 and 1 along
    three paths each."""
    ref = tiny()
    w7 = 0.30000000000000004
    val, reached, fired = ref.ground(0, 0, 1)
    want = [w7 * 3, 0.5 + w7 * 3, 0.0, 0.5 + 0.1, 0.5, ((1.5 + -0.25) + 0.0) + -1.5, 0.0, 0.0]
    assert [bits(v) for v in val] == [bits(v) for v in want]
    assert reached == [True, True, False, True, True, True, False, False]
    assert fired[5] == [(2, 3), (3, 1), (4, 1), (5, 3)]
    # known tails of (0, 0) are 1 and 5: filtered, 5 leaves; t = 1 stays and leads
    assert ref.topk(0, 0, 1, 8) == ([1, 0, 3, 4, -1, -1, -1, -1], want[1:2] + want[0:1] + [0.6, 0.5] + [-math.inf] * 4,
                                    4, 0)
    assert ref.topk(0, 0, 1, 3)[0] == [1, 0, 3]
    assert ref.topk(0, 0, 1, 8, filtered=False)[0] == [1, 0, 3, 4, 5, -1, -1, -1]
    # every entity: the unreached zeros by id, ahead of the negative score
    assert ref.topk(0, 0, 1, 8, filtered=False, candidates="all")[0] == [1, 0, 3, 4, 2, 6, 7, 5]
    assert ref.topk(0, 0, 1, 20, candidates="all")[2] == 7
    # the other tail of the row: t = 5 is reached, ranks last of the reached
    assert ref.topk(0, 0, 5, 8, filtered=False)[3] == len(ref.order(0, 0, 5, False)[0]) - 1


def test_hand_worked_explanation():
    ref = tiny()
    fired, total, rule, count = ref.explain(0, 0, 1, 5, 3)
    # contributions at 5: rule 2: +1.5, rule 3: -0.25, rule 4: 0.0 * 1, rule 5: -1.5
    assert (fired, bits(total), rule, count) == (4, bits(-0.25), [2, 4, 3], [3, 1, 1])
    assert ref.explain(0, 0, 1, 5, 16)[2][:5] == [2, 4, 3, 5, -1]
    assert ref.explain(0, 0, 1, 2, 2) == (0, 0.0, [-1, -1], [0, 0])  # nothing reaches 2
    assert ref.explain(0, 0, 1, -1, 1) == (0, 0.0, [-1], [0])
    # rules 0 and 1 both contribute +0.5 at the tail: the tie goes to the lower list index, behind rule 2's +1.0
    ref1 = mine_predict_ref.MinePredictRef([(0, 0, 1), (0, 1, 1)], 2, 3)
    ref1.set_rules([[], [], [(2, (1,)), (2, (0,)), (2, (1,))]], [[], [], [0.5, 0.5, 1.0]])
    assert ref1.explain(0, 2, 1, 1, 3) == (3, 2.0, [2, 0, 1], [1, 1, 1])


def test_open_queries_keep_the_edge_and_have_no_position():
    ref = tiny()
    closed, opened = ref.ground(0, 0, 1)[0], ref.ground(0, 0, -1)[0]
    assert closed != opened  # 0 -0-> 1 stays: (0, 1) arrives at 5 as well
    assert ref.g.destinations(0, (0,), (0, 0, -1)) == [(1, 2), (5, 1)]
    index, score, valid, position = ref.topk(0, 0, -1, 8)
    assert position == -1 and 1 not in index and 5 not in index  # no answer is kept: both known tails leave
    assert ref.topk(0, 0, -1, 8, filtered=False)[2] == 5


def test_weight_zero_reaches_and_no_rules_reach_nothing():
    ref = mine_predict_ref.MinePredictRef(TINY, 8, 4)
    ref.set_rules(TINY_RULES, [[0.0] * 9, [0.0] * 4, [], [0.0] * 2])
    assert ref.topk(0, 0, 1, 8)[0][:4] == [0, 1, 3, 4]  # all 0.0: reached, by id
    assert tiny().topk(5, 2, 0, 3) == ([-1] * 3, [-math.inf] * 3, 0, -1)  # relation 2 has no rules
    assert tiny().topk(5, 2, 0, 3, candidates="all") == ([0, 2, 3], [0.0] * 3, 3, 0)  # (5, 2, 1) is known
    assert tiny().topk(6, 0, 7, 3)[2] == 0  # nothing leaves 6 but the removed edge


def test_invariants_against_the_evaluation_restatement():
    """In `all` mode the eligible set is the evaluation's unskipped set, so the
    place of t lies inside its tie run; total is the entity's score bitwise."""
    ref = tiny()
    ev = mine_eval_ref.MineEvalRef(TINY, 8, 4)
    ev.set_rules(TINY_RULES, TINY_WEIGHTS)
    for h, r, t in TINY_QUERIES:
        for filtered in (True, False):
            num_g, num_ge = ev.pair(h, r, t, filtered)
            position = ref.topk(h, r, t, 8, filtered, "all")[3]
            assert num_g <= position < num_ge
        scores = ev.scores(h, r, t)
        assert [bits(v) for v in ref.ground(h, r, t)[0]] == [bits(v) for v in scores]
        for e in range(8):
            assert bits(ref.explain(h, r, t, e, 3)[1]) == bits(scores[e])
