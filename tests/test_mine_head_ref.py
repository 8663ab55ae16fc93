"""CPU side of the miner's head queries: the two restatements of
tests/mine_head_ref.py — (a) the naive per-candidate definition and (b) the
tail side of the transposed graph with reversed bodies — agree bit for bit, and
the head-side score of a triple's own head equals the tail-side score of its
own tail on the reference fixture's rules.  No tolerances."""
import os

import numpy as np

import mine_eval_ref
import mine_head_ref
from conftest import GOLDEN


def read_split(path, name):
    def rd(f):
        with open(os.path.join(path, f)) as fi:
            return {ln.split()[1]: int(ln.split()[0]) for ln in fi if ln.strip()}
    e2i, r2i = rd("entities.dict"), rd("relations.dict")
    with open(os.path.join(path, name)) as fi:
        return [(e2i[h], r2i[r], e2i[t]) for h, r, t in (ln.split() for ln in fi if ln.strip())], len(e2i), len(r2i)


def bits(v):
    return np.asarray(v, dtype=np.float64).view(np.int64).tolist()


def test_naive_definition_equals_transposition_on_the_tiny_graph():
    E, R = 8, 4
    valid, test = [(3, 0, 1), (4, 0, 5)], [(1, 0, 5), (3, 0, 6)]
    for known in (None, mine_head_ref.TINY + valid + test):
        a = mine_head_ref.NaiveHeadRef(mine_head_ref.TINY, E, R, known=known)
        b = mine_head_ref.HeadRef(mine_head_ref.TINY, E, R, known=known)
        tail = mine_eval_ref.MineEvalRef(mine_head_ref.TINY, E, R, known=known)
        for ref in (a, b, tail):
            ref.set_rules(mine_head_ref.TINY_RULES, mine_head_ref.TINY_WEIGHTS)
        differ = 0
        for h, r, t in mine_head_ref.TINY_QUERIES + [(-1, 0, 1), (-1, 0, 5), (-1, 1, 5)]:
            va, vb = a.scores(h, r, t), b.scores(h, r, t)
            assert bits(va) == bits(vb)
            if h < 0:  # open: no edge removed, so the closed query differs where the edge lay on a path
                continue
            for filtered in (True, False):
                assert a.pair(h, r, t, filtered) == b.pair(h, r, t, filtered)
            vt = tail.scores(h, r, t)
            assert bits(va[h]) == bits(vt[t])  # the same paths h -> t, added in the same order
            differ += bits(va) != bits(vt)
        assert differ == 8  # of 12: the head side is a different answer
    assert bits(a.scores(-1, 0, 1)) != bits(a.scores(0, 0, 1))
    # known heads of (0, 5) over train: 0 and 1; valid and test add 4 and (again) 1
    plain = mine_head_ref.NaiveHeadRef(mine_head_ref.TINY, E, R)
    plain.set_rules(mine_head_ref.TINY_RULES, mine_head_ref.TINY_WEIGHTS)
    assert plain.pair(0, 0, 5) == (6, 7) and a.pair(0, 0, 5) == (5, 6) and a.pair(0, 0, 5, False) == (7, 8)


def test_own_head_on_the_head_side_equals_own_tail_on_the_tail_side():
    from rnnlogic_amd import datasets
    fx = mine_eval_ref.load_fixture(os.path.join(GOLDEN, "_mine_eval_kinship.npz"))
    path = datasets.materialize("kinship")
    (train, E, R), (test, _, _) = (read_split(path, f) for f in ("train.txt", "test.txt"))
    head = mine_head_ref.HeadRef(train, E, R)
    tail = mine_eval_ref.MineEvalRef(train, E, R)
    head.set_rules(fx["rules"], fx["weights"])
    tail.set_rules(fx["rules"], fx["weights"])
    palindromes = sum(body == tuple(reversed(body)) for rules in fx["rules"] for _, body in rules)
    assert sum(len(x) for x in fx["rules"]) - palindromes > 900  # reversing the bodies matters
    differ = 0
    for h, r, t in test[:40]:
        vh, vt = head.scores(h, r, t), tail.scores(h, r, t)
        assert bits(vh[h]) == bits(vt[t])
        differ += head.pair(h, r, t) != tail.pair(h, r, t)
    assert differ >= 30  # the head-side pairs are another answer
