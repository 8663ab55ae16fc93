"""Two independent restatements of the rule statistics RuleMiner.rule_stats
computes (rnnl_miner_rule_stats, csrc/mine_stats.hip), on the train graph as
given: no inverses, no edge removed, duplicate edges counting once.

    D_b(x)         = entities reachable from x along the body b; {x} if b is empty
    T_r(x)         = {t : (x, r, t) in train}
    body(b)        = sum_x |D_b(x)|
    support(r, b)  = sum_x |D_b(x) & T_r(x)|
    pca_body(r, b) = sum over x with T_r(x) not empty of |D_b(x)|
    head_pairs(r)  = number of distinct (h, t) of relation r

(a) DenseStats: one boolean E x E matrix per relation, a body as a chain of
    fp32 matmuls thresholded at > 0 (prefixes cached), the counts as sums of
    masked matrices.  Shares nothing with a frontier walk.  (Every entry of a
    product of 0/1 matrices is an integer below 2^24 for E < 2^24, so fp32 is
    exact in telling zero from positive.)
(b) SetStats: a set walk per source, for graphs too large for E x E matrices.

A helper, like mine_ref.py: the tests compare the GPU counts against it.
"""
import numpy as np


class DenseStats(object):
    def __init__(self, triples, n_entities, n_relations):
        self.E, self.R = int(n_entities), int(n_relations)
        self.A = np.zeros((self.R, self.E, self.E), dtype=bool)
        for h, r, t in triples:
            self.A[int(r), int(h), int(t)] = True
        self.has_tail = self.A.any(2)  # (R, E)
        self._prefix = {(): np.eye(self.E, dtype=bool)}

    def reach(self, body):
        body = tuple(int(b) for b in body)
        if body not in self._prefix:
            m = self.reach(body[:-1]).astype(np.float32) @ self.A[body[-1]].astype(np.float32)
            self._prefix[body] = m > 0
        return self._prefix[body]

    def stats(self, head, body):
        """(support, body, pca_body) of the rule head <- body."""
        m = self.reach(body)
        return (int((m & self.A[head]).sum()), int(m.sum()), int(m[self.has_tail[head]].sum()))

    def head_pairs(self):
        return self.A.sum((1, 2)).astype(np.int64)


class SetStats(object):
    def __init__(self, triples, n_entities, n_relations):
        self.E, self.R = int(n_entities), int(n_relations)
        self.adj = {}
        for h, r, t in triples:
            self.adj.setdefault((int(h), int(r)), set()).add(int(t))
        self._cache = {}

    def reach(self, body):
        """{x: D_b(x)} over the sources x with D_b(x) not empty."""
        body = tuple(int(b) for b in body)
        if body not in self._cache:
            out = {}
            for x in range(self.E):
                cur = {x}
                for rel in body:
                    nxt = set()
                    for e in cur:
                        nxt |= self.adj.get((e, rel), set())
                    cur = nxt
                    if not cur:
                        break
                if cur:
                    out[x] = cur
            self._cache[body] = out
        return self._cache[body]

    def stats(self, head, body):
        sup = bod = pca = 0
        for x, dest in self.reach(body).items():
            tails = self.adj.get((x, int(head)))
            bod += len(dest)
            if tails:
                pca += len(dest)
                sup += len(dest & tails)
        return sup, bod, pca

    def head_pairs(self):
        out = np.zeros(self.R, dtype=np.int64)
        for (_, r), tails in self.adj.items():
            out[r] += len(tails)
        return out


def stats_of(ref, rel2rules):
    """dict(support, body, pca_body) of int64 arrays per relation, as RuleMiner.rule_stats."""
    out = dict(support=[], body=[], pca_body=[])
    for rules in rel2rules:
        rows = np.asarray([ref.stats(hd, body) for hd, body in rules], dtype=np.int64).reshape(-1, 3)
        out["support"].append(rows[:, 0])
        out["body"].append(rows[:, 1])
        out["pca_body"].append(rows[:, 2])
    return out


def confidence(kind, support, body, pca_body, head_pairs, pc=0.0):
    """The definition, rule by rule in Python floats: 0 / 0 is 0.0."""
    den = {"std": lambda i: body[i] + pc, "pca": lambda i: pca_body[i] + pc,
           "head_coverage": lambda i: head_pairs}[kind]
    return np.asarray([float(support[i]) / float(den(i)) if den(i) else 0.0 for i in range(len(support))],
                      dtype=np.float64)


def random_graph(seed, E, R, n):
    rng = np.random.default_rng(seed)
    return [(int(h), int(r), int(t)) for h, r, t in
            zip(rng.integers(0, E, n), rng.integers(0, R, n), rng.integers(0, E, n))]


def random_rules(seed, R, n, max_len):
    """n rules spread over the heads, bodies of length 0..max_len; some bodies under several heads."""
    rng = np.random.default_rng(seed)
    rel2rules = [[] for _ in range(R)]
    for _ in range(n):
        body = tuple(int(b) for b in rng.integers(0, R, int(rng.integers(0, max_len + 1))))
        for hd in set(int(x) for x in rng.integers(0, R, int(rng.integers(1, 3)))):
            rel2rules[hd].append((hd, body))
    return rel2rules
