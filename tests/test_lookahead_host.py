"""The training lookahead's queue policy (rnnlogic_amd.lookahead.LookaheadQueue)
on the host: which queued grounding a forward takes, which it drops, what it
counts.  The expectations are those of the dict-and-tuple code this class
replaced (_HipGrounding._prefetched), recorded by driving that code with the
same cases."""
import types

import torch

from rnnlogic_amd.lookahead import Grounded, LookaheadQueue


def rows():
    return torch.tensor([1, 2]), torch.tensor([3, 3]), torch.tensor([0, 1])


def entry(scale=1, triple=None):
    """A queued grounding whose GPU fields the queue never touches."""
    return Grounded(triple or rows(), ws=object(), scale=scale, n_cand=object(), event=object(), keep=(),
                    header=object())


def queue_of(entries):
    counters = types.SimpleNamespace(prefetch_hits=0, prefetch_dropped=0)
    q = LookaheadQueue(counters)
    q.entries.extend(entries)
    return q, counters


def take(q, e, scale=1, peek=False):
    return q.take(e.rows, scale, peek)


def same(queue, entries):
    return len(queue.entries) == len(entries) and all(a is b for a, b in zip(queue.entries, entries))


def test_match_at_the_head_is_taken():
    es = [entry(), entry(), entry()]
    q, c = queue_of(es)
    assert take(q, es[0]) is es[0]
    assert (c.prefetch_hits, c.prefetch_dropped) == (1, 0)
    assert same(q, es[1:])


def test_match_behind_two_drops_them():
    es = [entry(), entry(), entry()]
    q, c = queue_of(es)
    assert take(q, es[2]) is es[2]
    assert (c.prefetch_hits, c.prefetch_dropped) == (1, 2)
    assert same(q, [])


def test_no_match_leaves_everything():
    es = [entry(), entry(), entry()]
    q, c = queue_of(es)
    assert take(q, entry()) is None
    assert (c.prefetch_hits, c.prefetch_dropped) == (0, 0)
    assert same(q, es)


def test_stale_scale_is_dropped_without_a_match():
    es = [entry(1), entry(2), entry(1)]
    q, c = queue_of(es)
    assert take(q, entry(2), scale=2) is None
    assert (c.prefetch_hits, c.prefetch_dropped) == (0, 2)
    assert same(q, [es[1]])


def test_stale_entry_of_the_same_rows_does_not_match():
    es = [entry(1), entry(2)]
    q, c = queue_of(es)
    assert take(q, es[0], scale=2) is None
    assert (c.prefetch_hits, c.prefetch_dropped) == (0, 1)
    assert same(q, [es[1]])


def test_peek_leaves_the_match_queued():
    es = [entry(), entry(), entry()]
    q, c = queue_of(es)
    got = take(q, es[1], peek=True)
    assert got is es[1]
    assert (c.prefetch_hits, c.prefetch_dropped) == (0, 1)
    assert same(q, es[1:])
    assert take(q, es[1]) is got
    assert (c.prefetch_hits, c.prefetch_dropped) == (1, 1)
    assert same(q, es[2:])


def test_rows_match_by_identity_not_value():
    e = entry()
    q, c = queue_of([e])
    clone = entry(triple=tuple(t.clone() for t in e.rows))
    assert take(q, clone) is None
    assert (c.prefetch_hits, c.prefetch_dropped) == (0, 0)
    assert same(q, [e])


def test_no_edges_to_remove_matches_none():
    e = entry(triple=(torch.tensor([1]), torch.tensor([2]), None))
    q, c = queue_of([e])
    assert q.take((e.rows[0], e.rows[1], None), 1) is e
    assert (c.prefetch_hits, c.prefetch_dropped) == (1, 0)


def test_retain_nothing_counts_what_was_queued():
    q, c = queue_of([entry(), entry()])
    q.retain([])
    q.retain([])
    assert (len(q.entries), c.prefetch_hits, c.prefetch_dropped) == (0, 0, 2)
