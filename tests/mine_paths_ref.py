"""Plain Python restatement of RuleMiner.explain_paths (rnnl_miner_paths_side,
DESIGN §3.19): the grounding paths behind a rule of a listed entity.

A path of rule r <- b_1..b_L for the query (h, r, t) is a sequence of train
edges x_0 -b_1-> x_1 ... -b_L-> x_L, x_0 = h and x_L = e on the tail side,
x_0 = e and x_L = t on the head side; every copy of the edge (h, r, t) is
skipped on every hop (an open query, t = -1 / h = -1, skips nothing).  A
triple that is in train twice is two edges.  Order: by the entities read from
e back toward the anchor — tail side (x_{L-1}, x_{L-2}, ...), head side
(x_1, x_2, ...), ascending.

The method has nothing of the device's: adjacency lists with duplicates, a
depth-first walk from the anchor that writes every path down, then a sort.  No
path is counted without being walked, so it is for small counts only.

A helper, like mine_predict_ref.py: the tests compare the GPU against it.
"""
PATH_LEN = 6


class MinePathsRef(object):
    """train: [(h, r, t)] in file order, duplicates kept."""

    def __init__(self, train, n_entities, n_relations):
        self.E, self.R = int(n_entities), int(n_relations)
        self.out, self.inc = {}, {}
        for h, r, t in train:
            self.out.setdefault((int(h), int(r)), []).append(int(t))
            self.inc.setdefault((int(t), int(r)), []).append(int(h))
        self._walks = {}

    def _walk(self, h, r, t, body, side):
        """Every path of the body from the anchor, in the triple's orientation, grouped by its far end."""
        key = (h, r, t, tuple(body), side)
        if key in self._walks:
            return self._walks[key]
        head = side == "head"
        adj = self.inc if head else self.out
        rels = list(reversed(body)) if head else list(body)
        found = {}

        def step(x, depth, walked):
            if depth == len(rels):
                found.setdefault(x, []).append(tuple(reversed(walked)) if head else tuple(walked))
                return
            rel = rels[depth]
            for y in adj.get((x, rel), ()):
                src, dst = (y, x) if head else (x, y)
                if (src, rel, dst) == (h, r, t):
                    continue
                step(y, depth + 1, walked + [y])

        if len(body):
            anchor = t if head else h
            step(anchor, 0, [anchor])
        self._walks[key] = found
        return found

    def paths(self, h, r, t, e, body, side="tail"):
        """All paths of the body between the anchor and e, in order: tuples x_0 .. x_L."""
        got = self._walk(int(h), int(r), int(t), tuple(int(b) for b in body), side).get(int(e), [])
        if side == "head":
            return sorted(got)
        return sorted(got, key=lambda p: p[::-1])

    def explain_paths(self, h, r, t, e, body, P, side="tail"):
        """(listed, count, rows): rows is P rows of PATH_LEN, -1 past x_L and in unlisted rows."""
        every = self.paths(h, r, t, e, body, side) if e >= 0 and body is not None else []
        listed = min(int(P), len(every))
        rows = [list(p) + [-1] * (PATH_LEN - len(p)) for p in every[:listed]]
        return listed, len(every), rows + [[-1] * PATH_LEN for _ in range(int(P) - listed)]

    def expected(self, queries, index, rule, rules, P, side="tail"):
        """The three arrays of explain_paths as nested lists: queries (n, 3) closed
        form, index (n, m), rule (n, m, c) indices into rules[r] (-1 unused)."""
        listed, count, path = [], [], []
        for (h, r, t), slots, per_slot in zip(queries, index, rule):
            listed.append([])
            count.append([])
            path.append([])
            for e, ks in zip(slots, per_slot):
                got = [self.explain_paths(h, r, t, e, rules[r][k][1] if k >= 0 else None, P, side) for k in ks]
                listed[-1].append([g[0] for g in got])
                count[-1].append([g[1] for g in got])
                path[-1].append([g[2] for g in got])
        return listed, count, path
