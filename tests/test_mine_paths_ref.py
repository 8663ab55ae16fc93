"""CPU side of the grounding paths: the brute-force restatement
tests/mine_paths_ref.py lists exactly as many paths as the path-count
restatements count (mine_ref.MineRef.destinations forward, and the same on the
transposed graph of mine_head_ref for the head side), and lists them in the
documented order.  Integers only, no tolerances."""
import mine_head_ref
import mine_ref
from mine_paths_ref import PATH_LEN, MinePathsRef
from test_mine_head_ref import read_split

TINY, TINY_RULES = mine_head_ref.TINY, mine_head_ref.TINY_RULES


def counts_agree(train, E, R, queries, bodies, entities):
    """len(paths) against the counting restatements, both sides; returns the number of paths seen."""
    ref = MinePathsRef(train, E, R)
    fwd = mine_ref.MineRef(train, E, R)
    bwd = mine_ref.MineRef(mine_head_ref.transpose(train), E, R)
    seen = 0
    for h, r, t in queries:
        for body in bodies[r]:
            if h >= 0:
                want = dict(fwd.destinations(h, tuple(body), (h, r, t)))
                for e in entities:
                    got = ref.paths(h, r, t, e, body, "tail")
                    assert len(got) == want.get(e, 0)
                    assert all(p[0] == h and p[-1] == e and len(p) == len(body) + 1 for p in got)
                    seen += len(got)
            if t >= 0:
                # paths e -> t along the body = paths t -> e along the reversed body on the transposed graph
                want = dict(bwd.destinations(t, tuple(reversed(body)), (t, r, h)))
                for e in entities:
                    got = ref.paths(h, r, t, e, body, "head")
                    assert len(got) == want.get(e, 0)
                    assert all(p[0] == e and p[-1] == t for p in got)
                    # the definition, forward from e, read at t
                    assert len(got) == dict(fwd.destinations(e, tuple(body), (h, r, t))).get(t, 0)
                    seen += len(got)
    return seen


def test_counts_on_the_tiny_graph():
    bodies = [[b for _, b in rules] for rules in TINY_RULES]
    queries = mine_head_ref.TINY_QUERIES + [(0, 0, -1), (6, 0, -1), (0, 1, -1), (-1, 0, 1), (-1, 0, 5), (-1, 1, 5)]
    assert counts_agree(TINY, 8, 4, queries, bodies, range(8)) > 100


def test_counts_on_kinship_samples():
    from rnnlogic_amd import datasets
    from rnnlogic_amd.miner import read_rule_file
    path = datasets.materialize("kinship")
    (train, E, R), (test, _, _) = (read_split(path, f) for f in ("train.txt", "test.txt"))
    rules, _ = read_rule_file(datasets.rule_file("kinship"), R)
    bodies = [[b for _, b in rs][:4] for rs in rules]
    queries = test[:6] + [(test[6][0], test[6][1], -1), (-1, test[7][1], test[7][2])]
    assert counts_agree(train, E, R, queries, bodies, range(0, E, 7)) > 50


def test_hand_written_lists_on_the_tiny_graph():
    ref = MinePathsRef(TINY, 8, 4)
    # 0 -1-> {1, 3, 4} -1-> 5
    assert ref.paths(0, 0, 5, 5, (1, 1), "tail") == [(0, 1, 5), (0, 3, 5), (0, 4, 5)]
    assert ref.paths(0, 0, 5, 0, (1, 1), "head") == [(0, 1, 5), (0, 3, 5), (0, 4, 5)]
    assert ref.paths(0, 0, 5, 5, (1, 1), "head") == [(5, 3, 5)]
    assert ref.paths(0, 0, -1, 5, (1, 2, 1), "tail") == [(0, 3, 4, 5)]
    # (0, 0, 1) is in train twice: two edges, the path through them twice, side by side
    assert ref.paths(0, 0, -1, 5, (0, 1), "tail") == [(0, 1, 5), (0, 1, 5)]
    assert ref.paths(-1, 0, 5, 0, (0, 1), "head") == [(0, 1, 5), (0, 1, 5)]
    assert ref.paths(0, 0, 5, 5, (0, 1), "tail") == [(0, 1, 5), (0, 1, 5)]  # (0, 0, 5) is another edge
    assert ref.paths(0, 0, 1, 5, (0, 1), "tail") == []                      # both copies are the query's own
    assert ref.paths(0, 0, 1, 0, (0, 1), "head") == []
    # the own edge on a one-relation body equal to the head relation
    assert ref.paths(0, 0, -1, 1, (0,), "tail") == [(0, 1), (0, 1)] and ref.paths(0, 0, 1, 1, (0,), "tail") == []
    assert ref.paths(0, 0, 5, 1, (0,), "tail") == [(0, 1), (0, 1)] and ref.paths(0, 0, 5, 5, (0,), "tail") == []
    assert ref.paths(0, 0, -1, 3, (0, 1), "tail") == [(0, 5, 3)] and ref.paths(0, 0, 5, 3, (0, 1), "tail") == []
    assert ref.paths(0, 0, 1, 1, (), "tail") == []  # a rule without a body has no path
    listed, count, rows = ref.explain_paths(0, 0, 5, 5, (1, 1), 2, "tail")
    assert (listed, count) == (2, 3) and rows == [[0, 1, 5, -1, -1, -1], [0, 3, 5, -1, -1, -1]]
    listed, count, rows = ref.explain_paths(0, 0, 5, 5, (1, 1), 4, "tail")
    assert (listed, count) == (3, 3) and rows[3] == [-1] * PATH_LEN and len(rows) == 4
    assert ref.explain_paths(0, 0, 5, -1, (1, 1), 2, "tail") == (0, 0, [[-1] * PATH_LEN] * 2)


def test_the_order_reads_from_the_listed_entity_toward_the_anchor():
    # 0 -> {1, 2} -> {3, 4} -> 5, all of relation 0
    train = [(0, 0, 1), (0, 0, 2), (1, 0, 3), (2, 0, 3), (1, 0, 4), (2, 0, 4), (3, 0, 5), (4, 0, 5)]
    ref = MinePathsRef(train, 6, 1)
    assert ref.paths(0, 0, -1, 5, (0, 0, 0), "tail") == [(0, 1, 3, 5), (0, 2, 3, 5), (0, 1, 4, 5), (0, 2, 4, 5)]
    assert ref.paths(-1, 0, 5, 0, (0, 0, 0), "head") == [(0, 1, 3, 5), (0, 1, 4, 5), (0, 2, 3, 5), (0, 2, 4, 5)]
    # the query's own edge on the last hop of the head side
    assert ref.paths(3, 0, 5, 0, (0, 0, 0), "head") == [(0, 1, 4, 5), (0, 2, 4, 5)]
    # the head relation on a middle hop: 0 -> 2 -> 0 -> 1 -> 3 passes (0, 0, 1) on its third
    loop = MinePathsRef([(0, 0, 1), (0, 0, 2), (2, 0, 0), (1, 0, 3)], 4, 1)
    assert loop.paths(0, 0, -1, 3, (0, 0, 0, 0), "tail") == [(0, 2, 0, 1, 3)]
    assert loop.paths(0, 0, 1, 3, (0, 0, 0, 0), "tail") == []
    assert loop.paths(-1, 0, 1, 0, (0, 0, 0), "head") == [(0, 2, 0, 1)] and loop.paths(0, 0, 1, 0, (0, 0, 0), "head") == []
    # a doubled edge below the top: each path under it twice, side by side
    ref = MinePathsRef(train + [(3, 0, 5)], 6, 1)
    assert ref.paths(0, 0, -1, 5, (0, 0, 0), "tail") == [(0, 1, 3, 5), (0, 1, 3, 5), (0, 2, 3, 5), (0, 2, 3, 5),
                                                         (0, 1, 4, 5), (0, 2, 4, 5)]
