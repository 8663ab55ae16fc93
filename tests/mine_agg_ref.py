"""Plain Python restatement of the miner's aggregations (RuleMiner.
set_aggregation; rnnl_miner_set_aggregation) on top of
mine_predict_ref.MinePredictRef / mine_ref.MineRef.destinations, and through
the transposed graph of mine_head_ref for the head side.

Relation r's rules k in list order, weights w_k; fires_k(e): rule k (with a
body) has at least one path to e, the query's own edge removed on every hop.
  sum       val[e] = sum_k w_k * #paths_k(e)                     (as MineEvalRef)
  noisy_or  u_k = -log1p(-min(w_k, 1 - 2^-53));  val[e] = the u_k of the firing
            rules added in list order
  max, d    the distinct positive weights ascending get classes 1..C, a weight
            of 0 class 0; c1 >= c2 >= c3 the d largest classes of the firing
            rules with multiplicity, 0 beyond; val[e] = float(c1 * 2^34 + c2 *
            2^17 + c3)
Everything after val — the pairs, eligibility, order, position — is the sum's.
Explanations in the new modes: fired as before, total = val[e], the listed
rules the firing ones by operand (u_k / class) descending then list index, each
with count 1.

A helper, like mine_predict_ref.py: the tests compare the GPU against it.  It
computes u_k and the classes itself, not through rnnlogic_amd.miner.
"""
import math

import mine_head_ref
import mine_predict_ref

MODES = (("sum", 1), ("noisy_or", 1), ("max", 1), ("max", 2), ("max", 3))


def noisy_or_u(w):
    return -math.log1p(-min(float(w), 1.0 - 2.0 ** -53))


def classes_of(ws):
    values = sorted(set(float(w) for w in ws if w > 0.0))
    return [values.index(float(w)) + 1 if w > 0.0 else 0 for w in ws], values


def max_key(classes, depth):
    top = (sorted((c for c in classes if c > 0), reverse=True) + [0, 0, 0])[:depth] + [0, 0, 0]
    return float((top[0] << 34) | (top[1] << 17) | top[2])


def key_fields(key):
    k = int(key)
    return k >> 34, (k >> 17) & 0x1FFFF, k & 0x1FFFF


class AggRef(mine_predict_ref.MinePredictRef):
    """The tail side.  mode 'sum', 'noisy_or' or 'max' (with depth 1..3)."""

    def __init__(self, train, n_entities, n_relations, known=None, mode="sum", depth=1):
        super().__init__(train, n_entities, n_relations, known=known)
        self.mode, self.depth, self.op = mode, depth, []

    def set_mode(self, mode, depth=1):
        self.__dict__.pop("_ground_memo", None)
        self.mode, self.depth = mode, depth
        return self

    def set_rules(self, rel2rules, rel2weights):
        self.__dict__.pop("_fires_memo", None)
        super().set_rules(rel2rules, rel2weights)
        self.u = [[noisy_or_u(w) if 0.0 <= w <= 1.0 else None for w in ws] for ws in self.wt]
        self.cls = [classes_of(ws)[0] if all(w >= 0.0 for w in ws) else None for ws in self.wt]

    def operand(self, r, k):
        return self.u[r][k] if self.mode == "noisy_or" else float(self.cls[r][k])

    def combine(self, r, ks):
        """val of an entity the rules ks (list order) of relation r reach."""
        if self.mode == "noisy_or":
            val = 0.0
            for k in ks:
                val += self.u[r][k]
            return val
        return max_key([self.cls[r][k] for k in ks], self.depth)

    def fires(self, h, r, t):
        """fired[e] = [(k, 1)] in list order: the rules with a path to e (the same in every mode but the sum's counts)."""
        memo = self.__dict__.setdefault("_fires_memo", {})  # (set_rules drops it)
        if (h, r, t) not in memo:
            fired = [[] for _ in range(self.E)]
            for k, body in enumerate(self.bodies[r]):
                for dest, count in self.g.destinations(h, body, (h, r, t)):
                    if count > 0:
                        fired[dest].append((k, 1))
            memo[(h, r, t)] = fired
        return memo[(h, r, t)]

    def ground(self, h, r, t):
        if self.mode == "sum":
            return super().ground(h, r, t)
        memo = self.__dict__.setdefault("_ground_memo", {})
        if (h, r, t) not in memo:
            fired = self.fires(h, r, t)
            val = [self.combine(r, [k for k, _ in f]) if f else 0.0 for f in fired]
            memo[(h, r, t)] = (val, [bool(f) for f in fired], fired)
        return memo[(h, r, t)]

    def scores(self, h, r, t):
        return list(self.ground(h, r, t)[0])

    def explain(self, h, r, t, e, c):
        if self.mode == "sum" or e < 0:
            return super().explain(h, r, t, e, c)
        val, _, fired = self.ground(h, r, t)
        best = sorted(fired[e], key=lambda kc: (-self.operand(r, kc[0]), kc[0]))[:c]
        pad = c - len(best)
        return len(fired[e]), val[e], [k for k, _ in best] + [-1] * pad, [1] * len(best) + [0] * pad


class HeadAggRef(object):
    """The head side: AggRef of (t, r, h) on the transposed graph with every body reversed."""

    def __init__(self, train, n_entities, n_relations, known=None, mode="sum", depth=1):
        self.T = AggRef(mine_head_ref.transpose(train), n_entities, n_relations,
                        known=mine_head_ref.transpose(known if known is not None else train), mode=mode, depth=depth)
        self.E = int(n_entities)

    def set_mode(self, mode, depth=1):
        self.T.set_mode(mode, depth)
        return self

    def set_rules(self, rel2rules, rel2weights):
        self.T.set_rules(mine_head_ref.reverse_rules(rel2rules), rel2weights)

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


def make_ref(side, train, n_entities, n_relations, known=None):
    return (HeadAggRef if side == "head" else AggRef)(train, n_entities, n_relations, known=known)


# ---------------------------------------------------------------- the inputs
# The tiny graph, rule lists and queries of test_gpu_mine_eval.py (test files are
# not imported from) with confidences as weights: repeated values, a zero, two
# rules at 1.0 (the noisy-or clamp).  The last two rules of relation 3 are this
# file's own: with them entity 5 of the query (0, 3, 3) has three firing rules
# of one class and entity 3 two, which only depth 3 tells apart.
TINY = mine_head_ref.TINY
TINY_RULES = [
    [(0, ()), (0, (1,)), (0, (1, 1)), (0, (1, 2, 1)), (0, (0,)), (0, (1, 1)), (0, (0, 1)), (0, (1, 1, 2)), (0, (3,))],
    [(1, (0,)), (1, (1, 1)), (1, (0, 1)), (1, (1, 2, 0))],
    [],
    [(3, (1,)), (3, (0, 1)), (3, (1, 1)), (3, (1, 2, 1))],
]
TINY_WEIGHTS = [[1.0, .5, .5, .25, 0, .5, .125, .75, 1.0], [1.0, .25, .5, .5], [], [.7, .7, .7, .7]]
TINY_QUERIES = [(0, 0, 1), (0, 0, 5), (3, 0, 6), (5, 2, 0), (0, 0, 7), (0, 0, 1), (6, 0, 7), (2, 0, 2), (0, 1, 5),
                (0, 3, 3), (5, 2, 0), (1, 1, 5), (4, 1, 5), (5, 1, 3)]

many_rules_graph = mine_head_ref.many_rules_graph
spread_graph = mine_head_ref.spread_graph
SPREAD_W = [[0.5, 0.25, 1.0, 0.0, 0.5, 0.125], [1.0, 0.5], [0.5, 0.5]]


def confidence_like_weights(rules, seed):
    """A handful of values in [0, 1], so classes repeat and many rules tie; the
    strong values are rare, so that among a thousand rules the strongest ones
    an entity is reached by still differ from entity to entity."""
    import numpy as np
    rng = np.random.default_rng(seed)
    values, p = [0.0, 1e-3, 0.1, 0.25, 0.5, 1.0], [0.5, 0.3, 0.15, 0.04, 0.008, 0.002]
    return [[float(x) for x in rng.choice(values, len(rs), p=p)] for rs in rules]


def spread_queries(E, mids):
    return [(0, 0, 5), (0, 0, E - 1), (0, 0, E - 2), (7, 0, 5), (0, 0, mids[50]), (0, 1, E - 1), (E - 1, 2, 0),
            (5, 2, E - 3), (0, 0, 5)]
