"""Synthetic knowledge graphs that put one query into each regime of the
grounding kernel (csrc/ground.hip) that no shipped dataset reaches, and a
plain-Python audit that says in which regime a query lands.

Pure Python / numpy: no GPU, no product code.  The graphs are written in the
dataset layout of `chain_graph` in tests/test_gpu_ranges.py (entities.dict,
relations.dict, train / valid / test.txt and a rule file).  No graph holds a
parallel edge (the reference rejects them, data.py:68).

Relations: r0 (0) is the query relation, r1..r3 (1..3) occur in rule bodies,
r4 (4) has facts and no rules.  Rules, all with head r0:

    r0 <- r1      r0 <- r2      r0 <- r2 r3
    r0 <- r1 r1   r0 <- r0      r0 <- r0 r0

so the trie node of `r2` is a leaf (r0 <- r2) and an inner node (r0 <- r2 r3).
Every query is a train fact (h, r0, t): train mode has an edge to remove.
"""
import os
from collections import namedtuple

import numpy as np

WIN = 2048  # the audit's window: csrc/fwd.h WIN (tests/test_synth_audit.py checks that it still is)

R0, R1, R2, R3, R4 = range(5)
RULES = [(R0, [R1]), (R0, [R2]), (R0, [R2, R3]), (R0, [R1, R1]), (R0, [R0]), (R0, [R0, R0])]

MAIN_E = 200003   # > 196,608 = sort_words(1024) x 32, not a multiple of 2048
LIMIT_E = 1 << 19  # the largest graph the library accepts: 19 entity bits

Spec = namedtuple("Spec", "name E R facts queries rules")
# facts: [(h, r, t)] in train-file order; queries: {name: (h, t)}, each (h, R0, t) a fact


class _Builder(object):
    def __init__(self, name, E):
        self.name, self.E = name, E
        self.facts, self.seen, self.queries = [], set(), {}

    def add(self, h, r, t):
        assert 0 <= h < self.E and 0 <= t < self.E, (h, r, t)
        assert (h, r, t) not in self.seen, "parallel edge %r" % ((h, r, t),)
        self.seen.add((h, r, t))
        self.facts.append((h, r, t))

    def query(self, name, h, t, **neighbours):
        """The query (h, R0, t) and h's r1 / r2 neighbours."""
        assert name not in self.queries
        self.queries[name] = (h, t)
        self.add(h, R0, t)
        for rel, ts in neighbours.items():
            for x in ts:
                self.add(h, {"r1": R1, "r2": R2}[rel], int(x))

    def spec(self):
        return Spec(self.name, self.E, 5, list(self.facts), dict(self.queries), [(h, list(b)) for h, b in RULES])


def main_graph():
    """E = 200,003: one head per regime (module docstring of
    tests/test_gpu_synth_ground.py lists what each reaches).  Heads are the
    even ids from 10,240 (window 5), fresh tails the even ids from 12,288
    (window 6); no construction below places a neighbour there."""
    E = MAIN_E
    b = _Builder("main", E)
    heads = iter(range(10240, 12288, 2))
    tails = iter(range(12288, 14336, 2))
    last_lo = (E - 1) // WIN * WIN  # first entity of the last, partial window

    # few candidates on a big graph: k = 1..5 of these r1 neighbours
    corners = [E - 1, 196608, 98304, 49152, 0]
    for k in range(1, 6):
        b.query("few%d" % k, next(heads), next(tails), r1=corners[:k])
    # wide and sparse: 3,000 r1 neighbours, every 66th id (odd ids: never a head or a tail)
    b.query("sparse", next(heads), next(tails), r1=[13 + 66 * i for i in range(3000)])
    # dense window: 2,000 r1 neighbours inside [4096, 6144); the tail is one of them
    b.query("dense", next(heads), 4100, r1=range(4096, 6096))
    # last partial window: every entity of it, as an r1 and as an r2 neighbour
    # (E - last_lo = 1,347 entities: one relation alone would stay under HB_LOAD)
    b.query("last", next(heads), next(tails), r1=range(last_lo, E), r2=range(last_lo, E))
    # two adjacent windows (40, 41) with 768 + 768 = HB_LOAD and 768 + 769
    # contributions, ten more neighbours and the tail in window 80
    for name, nb in (("limit", 768), ("over", 769)):
        far = [80 * WIN + 2 * i for i in range(10)]
        b.query(name, next(heads), 80 * WIN + 100,
                r1=[40 * WIN + 2 * i for i in range(768)] + [41 * WIN + 2 * i for i in range(nb)] + far)
    # phase-A spill: 5,000 r2 neighbours, each with r3 edges to 7, 8, E - 1 and a private target
    mids = [120000 + i for i in range(5000)]
    b.query("spill", next(heads), 7, r2=mids)
    for i, m in enumerate(mids):
        for t in (7, 8, E - 1, 140000 + 3 * i):
            b.add(m, R3, t)
    # chunk edges: out-degree 63, 64, 65, 128, 129; the tail is the first neighbour
    fresh = iter(range(14336, 16384))
    for deg in (63, 64, 65, 128, 129):
        ns = [next(fresh) for _ in range(deg)]
        b.query("deg%d" % deg, next(heads), ns[0], r1=ns)
    # edge removal: the query's own edge is a self-loop that r0 <- r0 meets at
    # hop 1 and r0 <- r0 r0 at hops 1 and 2; a second r0 cycle and r1 edges
    # (a self-loop among them) stay.  r0 <- r1 r1 reaches h over two prefixes
    # (h -> h -> h, h -> d -> h): one candidate, the same rule-end node twice
    h = next(heads)
    a, c, d = next(tails), next(tails), next(tails)
    b.query("loop", h, h, r1=[h, d])
    for f in ((h, R0, a), (a, R0, h), (a, R0, c), (d, R1, a), (d, R1, h)):
        b.add(*f)
    # the relation without rules
    b.add(next(heads), R4, next(tails))
    return b.spec()


def limit_graph():
    """E = 2^19 exactly (19 entity bits in the grounding keys, 256 sort
    windows): two few-candidate queries touching both ends of the id range."""
    E = LIMIT_E
    b = _Builder("limit19", E)
    b.query("ends", 300000, 300002, r1=[0, E - 1, E // 2], r2=[E - 2])
    b.add(E - 2, R3, E - 1)
    b.add(E - 2, R3, 1)
    b.query("top", E - 1, 5, r1=[E - 3, 2])
    b.add(E - 3, R1, E - 4)
    b.add(300004, R4, 6)
    return b.spec()


def write(spec, directory):
    """Writes the dataset directory; returns (data path, rule file path)."""
    d = str(directory)
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "entities.dict"), "w") as f:
        f.write("".join("%d\te%d\n" % (i, i) for i in range(spec.E)))
    with open(os.path.join(d, "relations.dict"), "w") as f:
        f.write("".join("%d\tr%d\n" % (i, i) for i in range(spec.R)))
    line = "e%d\tr%d\te%d\n"
    with open(os.path.join(d, "train.txt"), "w") as f:
        f.write("".join(line % x for x in spec.facts))
    held = "".join(line % (h, R0, t) for h, t in spec.queries.values())
    for fn in ("valid.txt", "test.txt"):
        with open(os.path.join(d, fn), "w") as f:
            f.write(held)
    rules = os.path.join(d, "rules.txt")
    with open(rules, "w") as f:
        f.write("".join("%d %s\n" % (h, " ".join(str(x) for x in body)) for h, body in spec.rules))
    return d, rules


def rows(spec, names=None):
    """(names, h, r, t, etr) int64 arrays of the regime queries."""
    names = list(names if names is not None else spec.queries)
    ids = {}
    k = 0
    for f in spec.facts:
        if f[1] == R0:
            ids[f] = k
            k += 1
    h = np.array([spec.queries[n][0] for n in names], dtype=np.int64)
    t = np.array([spec.queries[n][1] for n in names], dtype=np.int64)
    etr = np.array([ids[(int(a), R0, int(c))] for a, c in zip(h, t)], dtype=np.int64)
    return names, h, np.full(len(h), R0, dtype=np.int64), t, etr


class Trie(object):
    """The prefix trie of one head relation's rule bodies: node 0 is the root,
    child[(node, rel)] the node of the prefix extended by rel, ends[node] the
    rules (indices into spec.rules) whose body is that prefix."""

    def __init__(self, rules, head):
        self.child, self.ends, self.depth = {}, {0: []}, {0: 0}
        for i, (hd, body) in enumerate(rules):
            if hd != head:
                continue
            node = 0
            for rel in body:
                nxt = self.child.get((node, rel))
                if nxt is None:
                    nxt = self.child[(node, rel)] = len(self.ends)
                    self.ends[nxt] = []
                    self.depth[nxt] = self.depth[node] + 1
                node = nxt
            self.ends[node].append(i)
        self.inner = {n for n, _ in self.child}
        self.children = {}
        for (n, rel), c in self.child.items():
            self.children.setdefault(n, []).append((rel, c))


_adjacency = {}


def adjacency(spec):
    key = (spec.name, len(spec.facts))
    if key not in _adjacency:
        adj = {}
        for h, r, t in spec.facts:
            adj.setdefault((h, r), []).append(t)
        _adjacency[key] = adj
    return _adjacency[key]


Audit = namedtuple("Audit", "keys_per_level P windows n_cand counts per_rule")


def audit(spec, name, remove=False):
    """Walks the rule trie of r0 over the fact list, level by level, as the
    grounding kernel's phase A does with every (node, entity) merged:

      keys_per_level  distinct (inner node, entity) keys entering each level's
                      hash (level 1 first): against HCAP / OCC_CAP
      P               contributions: one per (frontier key, edge) that ends a
                      rule — what phase B is given when phase A merged every
                      key (a spilled key adds more only if it is met twice)
      windows         contributions per window of WIN entities (numpy array)
      n_cand          distinct entities reached by some rule
      counts          {entity: paths summed over the rules}
      per_rule        {entity: {rule index: paths}}

    remove: the query's own edge (h, r0, t) is skipped on every r0 hop from h
    (data.py:164-169)."""
    h, t = spec.queries[name]
    trie = Trie(spec.rules, R0)
    adj = adjacency(spec)
    nwin = (spec.E + WIN - 1) // WIN
    windows = np.zeros(nwin, dtype=np.int64)
    per_node = {}
    frontier = {(0, h): 1}
    keys_per_level, P = [], 0
    while frontier:
        nxt = {}
        for (node, v), c in frontier.items():
            for rel, child in trie.children.get(node, ()):
                for x in adj.get((v, rel), ()):
                    if remove and rel == R0 and v == h and x == t:
                        continue
                    if trie.ends[child]:
                        P += 1
                        windows[x // WIN] += 1
                        per_node[(child, x)] = per_node.get((child, x), 0) + c
                    if child in trie.inner:
                        nxt[(child, x)] = nxt.get((child, x), 0) + c
        if nxt or not keys_per_level:
            keys_per_level.append(len(nxt))
        frontier = nxt
    counts, per_rule = {}, {}
    for (node, x), c in per_node.items():
        counts[x] = counts.get(x, 0) + c * len(trie.ends[node])
        for i in trie.ends[node]:
            per_rule.setdefault(x, {})[i] = per_rule.get(x, {}).get(i, 0) + c
    return Audit(keys_per_level, P, windows, len(counts), counts, per_rule)


Pass = namedtuple("Pass", "kind lo hi load")


def passes(windows, E, hb_load, win=WIN):
    """How phase B splits a query's contributions (candidates_phase,
    ground.hip): at most hb_load in all -> one hash pass over [0, E); else a
    window heavier than hb_load alone in the dense pass and runs of lighter
    consecutive windows in hash passes of at most hb_load contributions."""
    total = int(windows.sum())
    if total <= hb_load:
        return [Pass("hash", 0, E, total)] if total else []
    if len(windows) == 1:
        return [Pass("dense", 0, E, total)]
    out, w, n = [], 0, len(windows)
    while w < n:
        if windows[w] > hb_load:
            out.append(Pass("dense", w * win, min((w + 1) * win, E), int(windows[w])))
            w += 1
            continue
        w2, load = w + 1, int(windows[w])
        while w2 < n and load + windows[w2] <= hb_load:
            load += int(windows[w2])
            w2 += 1
        if load:
            out.append(Pass("hash", w * win, min(w2 * win, E), load))
        w = w2
    return out
