"""Plain Python restatement of the miner's predictions and their explanations
(RuleMiner.predict_topk / explain; rnnl_miner_predict / rnnl_miner_explain,
csrc/mine_predict.hip) on top of mine_eval_ref.MineEvalRef and
mine_ref.MineRef.destinations.

Per query (h, r, t), t = -1 open (no edge removed, no answer kept):
  val[e]      as MineEvalRef.scores: rules in list order, val += wt * count;
  reached[e]  some rule with a body has a path count > 0 at e, whatever wt;
  eligible    ('all' or reached) and not (filtered and e != t and (h, r, e)
              known) and val[e] is not NaN;
  order       val descending, then e ascending (-0.0 == +0.0);
  position    the 0-based place of t in the whole order, -1 if not eligible.
Per (query, entity): the rules that fire there with their counts, the total
in list order and the c rules with the largest wt * count, ties by list index.

A helper, like mine_eval_ref.py: the tests compare the GPU against it.
"""
import math

import mine_eval_ref


class MinePredictRef(mine_eval_ref.MineEvalRef):
    def ground(self, h, r, t):
        """(val, reached, fired): fired[e] = [(k, count)] in list order."""
        memo = self.__dict__.setdefault("_ground_memo", {})  # (set_rules drops it)
        if (h, r, t) in memo:
            return memo[(h, r, t)]
        val = [0.0] * self.E
        reached = [False] * self.E
        fired = [[] for _ in range(self.E)]
        for k, (body, w) in enumerate(zip(self.bodies[r], self.wt[r])):
            for dest, count in self.g.destinations(h, body, (h, r, t)):
                val[dest] += w * count
                if count > 0:
                    reached[dest] = True
                    fired[dest].append((k, count))
        memo[(h, r, t)] = (val, reached, fired)
        return memo[(h, r, t)]

    def set_rules(self, rel2rules, rel2weights):
        self.__dict__.pop("_ground_memo", None)
        super().set_rules(rel2rules, rel2weights)

    def order(self, h, r, t, filtered=True, candidates="reached"):
        """(the eligible entities in order, val)."""
        val, reached, _ = self.ground(h, r, t)
        elig = [e for e in range(self.E)
                if (candidates == "all" or reached[e])
                and not (filtered and e != t and (h, r, e) in self.known)
                and not math.isnan(val[e])]
        elig.sort(key=lambda e: (-val[e], e))  # -0.0 == 0.0 compare equal: the id decides
        return elig, val

    def topk(self, h, r, t, k, filtered=True, candidates="reached"):
        """(index (k), score (k), valid, position) as rnnl_miner_predict writes them."""
        elig, val = self.order(h, r, t, filtered, candidates)
        valid = min(k, len(elig))
        index = elig[:valid] + [-1] * (k - valid)
        score = [val[e] for e in elig[:valid]] + [-math.inf] * (k - valid)
        position = elig.index(t) if t >= 0 and t in elig else -1
        return index, score, valid, position

    def explain(self, h, r, t, e, c):
        """(fired, total, rule (c), count (c)) of entity e (-1: an unused slot)."""
        if e < 0:
            return 0, 0.0, [-1] * c, [0] * c
        _, _, fired = self.ground(h, r, t)
        total = 0.0
        for k, count in fired[e]:
            total += self.wt[r][k] * count
        best = sorted(fired[e], key=lambda kc: (-(self.wt[r][kc[0]] * kc[1]), kc[0]))[:c]
        pad = c - len(best)
        return len(fired[e]), total, [k for k, _ in best] + [-1] * pad, [n for _, n in best] + [0] * pad

    def contributions(self, h, r, t, e):
        """[wt * count] of the rules that fire at e, in list order."""
        return [self.wt[r][k] * n for k, n in self.ground(h, r, t)[2][e]]
