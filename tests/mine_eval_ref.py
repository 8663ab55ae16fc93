"""Plain Python fp64 restatement of the reference miner's evaluation
(ReasoningPredictor::evaluate_thread and ::evaluate, miner/rnnlogic.cpp:
968-1120) on top of mine_ref.MineRef.destinations.

Per query (h, r, t): val[e] = sum over r's rules in list order of
wt * path count (the query's own edge removed on every hop); an entity e != t
with (h, r, e) known is skipped; num_g / num_ge count the others with
val > / >= val[t].  The metrics are the expectation over the tie run
num_g + 1 .. num_ge from cumulative tables, summed in triple order.

tools/make_golden_mine_eval.py asserts, before it writes a fixture, that this
reproduces the reference's own pairs and metrics exactly (bitwise for the
metrics).  A helper, like mine_ref.py: the tests compare RuleMiner.scores /
eval_ranks / evaluate against it.
"""
import mine_ref


class MineEvalRef(object):
    """train: [(h, r, t)] the graph; known: every true triple (train, valid
    and test) for the filtered setting."""

    def __init__(self, train, n_entities, n_relations, known=None):
        self.g = mine_ref.MineRef(train, n_entities, n_relations)
        self.E, self.R = int(n_entities), int(n_relations)
        self.known = set((int(h), int(r), int(t)) for h, r, t in (known if known is not None else train))
        self.bodies = [[] for _ in range(self.R)]
        self.wt = [[] for _ in range(self.R)]

    def set_rules(self, rel2rules, rel2weights):
        self.bodies = [[tuple(int(x) for x in body) for _, body in rules] for rules in rel2rules]
        self.wt = [[float(w) for w in ws] for ws in rel2weights]
        assert [len(b) for b in self.bodies] == [len(w) for w in self.wt]

    def scores(self, h, r, t):
        """rank_list[.].val of evaluate_thread, :1001-1018."""
        val = [0.0] * self.E
        for body, w in zip(self.bodies[r], self.wt[r]):
            for dest, count in self.g.destinations(h, body, (h, r, t)):
                val[dest] += w * count
        return val

    def pair(self, h, r, t, filtered=True):
        """(num_g, num_ge), :1020-1034 (the sort only orders the scan)."""
        val = self.scores(h, r, t)
        t_val = val[t]
        num_g = num_ge = 0
        for e in range(self.E):
            if filtered and e != t and (h, r, e) in self.known:
                continue
            if val[e] > t_val:
                num_g += 1
            if val[e] >= t_val:
                num_ge += 1
        return num_g, num_ge

    def pairs(self, triples, filtered=True):
        return [self.pair(int(h), int(r), int(t), filtered) for h, r, t in triples]


def metrics(pairs, n_entities):
    """ReasoningPredictor::evaluate, :1070-1116: (mr, mrr, hit1, hit3, hit10)."""
    E = int(n_entities)
    tables = [[0.0] * (E + 1) for _ in range(5)]
    for rank in range(1, E + 1):
        tables[0][rank] = float(rank)
        tables[1][rank] = 1.0 / rank
        if rank <= 1:
            tables[2][rank] = 1.0
        if rank <= 3:
            tables[3][rank] = 1.0
        if rank <= 10:
            tables[4][rank] = 1.0
    for rank in range(1, E + 1):
        for tb in tables:
            tb[rank] += tb[rank - 1]
    out = [0.0] * 5
    for num_g, num_ge in pairs:
        for k, tb in enumerate(tables):
            out[k] += (tb[num_ge] - tb[num_g]) / (num_ge - num_g)
    return tuple(x / len(pairs) for x in out)


METRIC_NAMES = ("mr", "mrr", "hit1", "hit3", "hit10")


def load_fixture(path):
    """A tests/golden/_mine_eval_<data>.npz (tools/make_golden_mine_eval.py):
    rules [(head, body)] per relation, weights per relation, and per split the
    reference's pairs (n, 2) and metrics (5)."""
    import numpy as np
    z = np.load(path, allow_pickle=False)
    R = int(z["n_relations"])
    rel2rules = [[] for _ in range(R)]
    rel2weights = [[] for _ in range(R)]
    for hd, ln, body, w in zip(z["rule_head"].tolist(), z["rule_len"].tolist(), z["rule_body"].tolist(),
                               z["weights"].tolist()):
        rel2rules[hd].append((hd, tuple(body[:ln])))
        rel2weights[hd].append(w)
    return dict(data=str(z["data"]), rules=rel2rules, weights=rel2weights,
                pairs={s: z["pairs_" + s].astype(np.int64) for s in ("valid", "test")},
                metrics={s: z["metrics_" + s] for s in ("valid", "test")})
