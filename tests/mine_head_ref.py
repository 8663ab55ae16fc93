"""Plain Python restatement of the miner's head queries (?, r, t)
(RuleMiner.scores / eval_ranks / predict_topk / explain with side="head";
rnnl_miner_*_side), two ways.

Per query (h, r, t), h = -1 open (no edge removed, no answer kept):
  val[e] = sum over r's rules in list order of wt * #paths(e -> t along the
  body), every edge equal to (h, r, t) skipped on every hop; an entity e != h
  with (e, r, t) known is skipped in the filtered setting.

(a) naive: per candidate e, forward mine_ref.MineRef.destinations(e, body,
    (h, r, t)) read at t — the definition, |E| forward groundings per rule.
(b) transposed: the tail side of (t, r, h) on the graph of the triples
    (t, r, h) with every body reversed (mine_eval_ref / mine_predict_ref): the
    integer path counts are equal and the terms are added in the same order,
    so the two agree bit for bit.

A helper, like mine_predict_ref.py: the tests compare the GPU against it.
"""
import mine_eval_ref
import mine_predict_ref


def transpose(triples):
    return [(int(t), int(r), int(h)) for h, r, t in triples]


def reverse_rules(rel2rules):
    return [[(hd, tuple(reversed(tuple(body)))) for hd, body in rules] for rules in rel2rules]


class NaiveHeadRef(object):
    """(a).  train: [(h, r, t)]; known: every true triple for the filtered setting."""

    def __init__(self, train, n_entities, n_relations, known=None):
        self.ref = mine_eval_ref.MineEvalRef(train, n_entities, n_relations, known=known)
        self.E = int(n_entities)

    def set_rules(self, rel2rules, rel2weights):
        self.ref.set_rules(rel2rules, rel2weights)

    def scores(self, h, r, t):
        val = [0.0] * self.E
        for body, w in zip(self.ref.bodies[r], self.ref.wt[r]):
            for e in range(self.E):
                for dest, count in self.ref.g.destinations(e, body, (h, r, t)):
                    if dest == t:
                        val[e] += w * count
        return val

    def pair(self, h, r, t, filtered=True):
        val = self.scores(h, r, t)
        num_g = num_ge = 0
        for e in range(self.E):
            if filtered and e != h and (e, r, t) in self.ref.known:
                continue
            num_g += val[e] > val[h]
            num_ge += val[e] >= val[h]
        return num_g, num_ge

    def pairs(self, triples, filtered=True):
        return [self.pair(int(h), int(r), int(t), filtered) for h, r, t in triples]


class HeadRef(object):
    """(b).  Every method takes the query as (h, r, t) of the graph as given."""

    def __init__(self, train, n_entities, n_relations, known=None):
        self.T = mine_predict_ref.MinePredictRef(transpose(train), n_entities, n_relations,
                                                 known=transpose(known if known is not None else train))
        self.E = int(n_entities)

    def set_rules(self, rel2rules, rel2weights):
        self.T.set_rules(reverse_rules(rel2rules), rel2weights)

    def scores(self, h, r, t):
        return self.T.scores(t, r, h)

    def pair(self, h, r, t, filtered=True):
        return self.T.pair(t, r, h, filtered)

    def pairs(self, triples, filtered=True):
        return [self.pair(int(h), int(r), int(t), filtered) for h, r, t in triples]

    def topk(self, h, r, t, k, filtered=True, candidates="reached"):
        return self.T.topk(t, r, h, k, filtered, candidates)

    def explain(self, h, r, t, e, c):
        return self.T.explain(t, r, h, e, c)


# ---------------------------------------------------------------- the graphs
# Copies of the tiny graph, the hub graph and the 1,110-rule list of
# test_gpu_mine_eval.py (test files are not imported from), so that the CPU and
# the GPU tests of the head side read the same constants.
#
# Tiny: relation 2 has triples but no rules, relation 3 rules but no triples;
# (0,0,1) is there twice; (2,0,2) is a self-loop; 0 -1-> {3,4} -1-> 5 are two
# parallel paths; nothing enters 0 but relation 2's edge from 5 and nothing
# enters 6 but (7,2,6).
TINY = [(0, 0, 1), (0, 0, 1), (2, 0, 2), (0, 0, 5), (6, 0, 7), (0, 1, 3), (0, 1, 4), (3, 1, 5), (4, 1, 5), (1, 1, 5),
        (5, 2, 0), (5, 2, 1), (3, 2, 4), (0, 1, 1), (2, 1, 2), (1, 0, 5), (7, 2, 6), (5, 1, 3)]
TINY_RULES = [
    [(0, ()), (0, (1,)), (0, (1, 1)), (0, (1, 2, 1)), (0, (0,)), (0, (1, 1)), (0, (0, 1)), (0, (1, 1, 2)), (0, (3,)),
     (0, (1, 2, 0, 1, 1)), (0, (0, 1, 2, 1))],  # the last two: the head side's own, bodies of five and four
    [(1, (0,)), (1, (1, 1)), (1, (0, 1)), (1, (1, 2, 0))],
    [],
    [(3, (1,)), (3, (0, 1))],
]
TINY_WEIGHTS = [[3.0, 0.5, 0.5, -0.25, 0.0, -0.5, 0.1, 0.30000000000000004, 1.0, 0.7, -0.3], [1.0, -0.25, 0.5, 0.5],
                [], [0.7, -0.7]]
TINY_QUERIES = [
    (0, 0, 1),  # a train triple that occurs twice: both copies are removed
    (0, 0, 5),
    (3, 0, 6),  # not a train triple; only (7, 2, 6) enters 6
    (5, 2, 0),  # relation 2 has no rules: every val is 0
    (0, 0, 7),
    (6, 0, 7),  # its own edge is all that enters 7: nothing grounds
    (2, 0, 2),  # the self-loop, h == t, removed
    (0, 1, 5),
    (0, 3, 3),  # a relation with rules and no triples
    (1, 1, 5), (4, 1, 5), (5, 1, 3),
]


def many_rules_graph():
    """10 relations, every body of length 1..3 as relation 0's list: 1,110 rules."""
    import numpy as np
    rng = np.random.default_rng(5)
    R, E = 10, 8
    tri = sorted(set((int(h), int(r), int(t)) for h, r, t in
                     zip(rng.integers(0, E, 90), rng.integers(0, R, 90), rng.integers(0, E, 90))))
    bodies = [(a,) for a in range(R)] + [(a, b) for a in range(R) for b in range(R)] + \
        [(a, b, c) for a in range(R) for b in range(R) for c in range(R)]
    rules = [[(0, b) for b in bodies]] + [[(r, (r - 1,)), (r, (0, r))] for r in range(1, R)]
    return tri, E, R, rules


def quantised_weights(rules, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    return [[float(x) for x in rng.choice([0.0, 0.5, 0.5, -0.25, 0.1, 1e-3, -1.7], len(rs))] for rs in rules]


def spread_graph(E):
    """A hub over the whole index range: 0 -1-> 100 nodes -2-> 5, some of them on
    to the last entities.  Entity 5 has 100 in-edges of relation 2, so a
    backward frontier from 5 passes the 64 lanes of a wave, and (for E = 2,100)
    lies on both sides of index 2,048."""
    last = E - 1
    mids = sorted(set(3 + (i * (E - 10)) // 100 for i in range(1, 101)) - {5})
    tri = [(0, 0, 5), (0, 0, mids[7]), (7, 0, 5), (last, 0, 0), (5, 0, last), (0, 0, last - 1)]
    tri += [(0, 1, x) for x in mids] + [(x, 2, 5) for x in mids] + [(x, 2, last - 2) for x in mids[-30:]]
    tri += [(7, 1, mids[3]), (5, 1, last), (last, 2, 0), (last - 2, 0, last - 3), (5, 0, 1), (0, 1, last)]
    rules = [[(0, (1,)), (0, (1, 2)), (0, (1, 2, 0)), (0, (0, 1)), (0, (2,)), (0, (1, 2))],
             [(1, (0,)), (1, (1, 2, 1))], [(2, (0, 0)), (2, (2,))]]
    return tri, E, 3, rules, mids


SPREAD_W = [[0.5, -0.25, 1.0, 0.0, 0.5, 0.125], [1.0, 0.5], [0.5, 0.5]]
