"""Plain Python fp64 restatement of the reference miner after its search
(miner/main.cpp:27-49): rule subset per relation, ReasoningPredictor::learn
(online Adam, one weight per rule), H_score, RuleGenerator::update (running
mean over the pool) and out_rules' order — single-threaded, so a pure function
of the triple order.  It reproduces the H the reference CLI prints with
`-threads 1` to the rounding of its "%.16lf" (tools/make_golden_mine.py
asserts that before it writes a fixture).

Where the reference leaves an order to std::sort, ours is defined: top-k takes
val descending then position in the relation's rule list ascending; out_rules
takes H descending then pool order.

A helper, like topk_ref.py: the GPU tests compare RuleMiner.learn / h_score /
mine against it.
"""
import math

LOG_B1 = math.log(0.9)
LOG_B2 = math.log(0.999)


def c_shuffle(items, rand):
    """std::random_shuffle (libstdc++) with rand(): for i = 1..n-1,
    j = rand() % (i + 1), swap."""
    for i in range(1, len(items)):
        j = rand() % (i + 1)
        if i != j:
            items[i], items[j] = items[j], items[i]
    return items


class MineRef(object):
    """triples: [(h, r, t)] in train-file order; orders index into it."""

    def __init__(self, triples, n_entities, n_relations):
        self.triples = [(int(h), int(r), int(t)) for h, r, t in triples]
        self.E, self.R = int(n_entities), int(n_relations)
        self.adj = {}
        for h, r, t in self.triples:
            self.adj.setdefault((h, r), []).append(t)
        self.observed = set(self.triples)
        self._cache = {}
        self.set_logic_rules([[] for _ in range(self.R)])

    def set_logic_rules(self, rel2rules, priors=None):
        """rel2rules[r] = [(head, body)]; weights, Adam state and H cleared
        (ReasoningPredictor::set_logic_rules)."""
        self.bodies = [[tuple(int(x) for x in body) for _, body in rules] for rules in rel2rules]
        self.param = [[[0.0, 0.0, 0.0, 0.0] for _ in rules] for rules in self.bodies]  # data, m, v, t
        self.H = [[0.0] * len(rules) for rules in self.bodies]
        self.prior = [list(p) for p in priors] if priors is not None else [[0.0] * len(b) for b in self.bodies]

    def weights(self):
        return [[p[0] for p in rules] for rules in self.param]

    def destinations(self, h, body, removed):
        """KnowledgeGraph::rule_destination: [(dest, path count)], dest
        ascending; every edge equal to `removed` skipped on every hop."""
        if not body:
            return []
        rh, rr, rt = removed
        key = (h, body) if rr not in body else None  # the removed edge cannot lie on the path
        if key is not None and key in self._cache:
            return self._cache[key]
        cur = {h: 1}
        for rel in body:
            nxt = {}
            for e, n in cur.items():
                for x in self.adj.get((e, rel), ()):
                    if e == rh and rel == rr and x == rt:
                        continue
                    nxt[x] = nxt.get(x, 0) + n
            cur = nxt
        out = sorted(cur.items())
        if key is not None:
            self._cache[key] = out
        return out

    @staticmethod
    def update(p, grad, lr, wd):
        """Parameter::update."""
        g = grad - wd * p[0]
        p[3] += 1
        p[1] = 0.9 * p[1] + 0.1 * g
        p[2] = 0.999 * p[2] + 0.001 * g * g
        bias1 = 1 - math.exp(LOG_B1 * p[3])
        bias2 = 1 - math.exp(LOG_B2 * p[3])
        mt = p[1] / bias1
        vt = math.sqrt(p[2]) / math.sqrt(bias2) + 0.00000001
        p[0] += lr * mt / vt

    def learn(self, order, n_used, lr, wd, temp, fast=False):
        for T in range(n_used):
            tri = self.triples[order[T]]
            h, r, _ = tri
            params = self.param[r]
            lists = [self.destinations(h, body, tri) for body in self.bodies[r]]
            logit = {}
            for p, lst in zip(params, lists):
                for d, c in lst:
                    logit[d] = logit.get(d, 0.0) + p[0] * c / temp
            if not logit:
                continue
            dests = sorted(logit)
            mx = -1000000.0
            for d in dests:
                mx = max(mx, logit[d])
            s = 0.0
            for d in dests:
                s += math.exp(logit[d] - mx)
            grad = {}
            for d in dests:
                prob = math.exp(logit[d] - mx) / s
                target = 1.0 if (h, r, d) in self.observed else 0.0
                grad[d] = (target - prob) / temp
            for p, lst in zip(params, lists):
                for d, c in lst:
                    if fast:
                        self.update(p, grad[d] * c, lr, wd)
                    else:
                        for _ in range(c):
                            self.update(p, grad[d], lr, wd)

    def h_score(self, order, n_used, top_k, H_temperature=1.0, prior_weight=0.0):
        n_train = len(self.triples)
        for T in range(n_used):
            tri = self.triples[order[T]]
            h, r, t = tri
            nr = len(self.bodies[r])
            if nr == 0:
                continue
            lists = [self.destinations(h, body, tri) for body in self.bodies[r]]
            D = len(set(d for lst in lists for d, _ in lst))
            val = []
            for k, lst in enumerate(lists):
                w = self.param[r][k][0]
                v = self.prior[r][k] * prior_weight
                for d, c in lst:
                    if d == t:
                        v += w * c
                    v -= w * c / D
                val.append(v)
            H = self.H[r]
            if top_k == 0:
                val = [v / H_temperature for v in val]
                mx = -1000000.0
                for v in val:
                    mx = max(mx, v)
                s = 0.0
                for v in val:
                    s += math.exp(v - mx)
                for k, v in enumerate(val):
                    H[k] += math.exp(v - mx) / s / n_train
            else:
                for k in sorted(range(nr), key=lambda k: (-val[k], k))[:top_k]:
                    H[k] += 1.0 / top_k / n_train


def out_order(H, top_n_out=0):
    """out_rules' order of one relation's pool: H descending, then pool order."""
    idx = sorted(range(len(H)), key=lambda k: (-H[k], k))
    return idx[:top_n_out] if top_n_out else idx


def mine_replay(triples, n_entities, n_relations, pool, orders, selections, lr, wd, temp, top_k, portion=1.0,
                fast=False):
    """The loop of main.cpp:40-47 with the given triple order and selected
    pool indices per iteration.  pool[r] = [(head, body)].  Returns the pool's
    H per relation and the last iteration's weights per relation."""
    ref = MineRef(triples, n_entities, n_relations)
    n_used = int(len(triples) * portion)
    H = [[0.0] * len(p) for p in pool]
    cn = [[0] * len(p) for p in pool]
    for order, sel in zip(orders, selections):
        ref.set_logic_rules([[pool[r][i] for i in sel[r]] for r in range(n_relations)])
        ref.learn(order, n_used, lr, wd, temp, fast)
        ref.h_score(order, n_used, top_k, 1.0, 0.0)
        for r in range(n_relations):
            for k, i in enumerate(sel[r]):
                H[r][i] = (H[r][i] * cn[r][i] + ref.H[r][k]) / (cn[r][i] + 1)
                cn[r][i] += 1
    return H, ref.weights()


def load_fixture(path, n_relations):
    """A tests/golden/_mine_<case>.npz (tools/make_golden_mine.py): args,
    orders[it], selections[it][r] and the printed rules."""
    import json

    import numpy as np
    z = np.load(path, allow_pickle=False)
    args = json.loads(str(z["args"]))
    off, flat = z["sel_off"], z["sel_flat"]
    selections = [[flat[off[it * n_relations + r]:off[it * n_relations + r + 1]].tolist()
                   for r in range(n_relations)] for it in range(args["iterations"])]
    return dict(args=args, orders=[o.astype(np.int32) for o in z["orders"]], selections=selections,
                out_rel=z["out_rel"].astype(np.int64), out_idx=z["out_idx"].astype(np.int64), out_H=z["out_H"],
                out_len=z["out_len"])
