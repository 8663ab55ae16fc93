"""Host state of the training lookahead (_HipGrounding.prefetch).

A model grounds the next batches on a side stream while the current one scores,
steps back and updates.  Per (model, device) one Lookahead owns what that
takes: the queue of groundings launched ahead (LookaheadQueue of Grounded: the
part that needs no GPU), the side stream, a ring of workspaces, pinned header
copies with their events and the scoring statuses that are read two forwards
late.
"""
import collections
import ctypes
import logging
from typing import NamedTuple

import torch

from . import _native


class Grounded(NamedTuple):
    """One grounding launched ahead of the forward that will use it."""
    rows: tuple  # (all_h, all_r, edges_to_remove) as prefetch was called: a forward matches the objects
    ws: torch.Tensor
    scale: int  # the capacity_scale it was grounded at
    n_cand: torch.Tensor
    event: torch.cuda.Event  # on the side stream, behind the grounding and its header copy
    keep: tuple  # the contiguous row tensors the kernels read
    header: torch.Tensor  # pinned: the workspace header, then the first row's relation (int64)

    @property
    def relation(self):
        """The first row's relation (host read; the event has been waited on)."""
        return int(self.header[-8:].view(torch.int64)[0])


class LookaheadQueue(object):
    """The groundings queued ahead, oldest first, and the policy by which a
    forward takes its own: identity and integer comparisons only (no GPU).
    Counts into `model.prefetch_hits` / `.prefetch_dropped`."""

    def __init__(self, model):
        self.model = model
        self.entries = collections.deque()

    def take(self, rows, scale, peek=False):
        """The queued grounding of exactly these row objects (all_h, all_r,
        edges_to_remove: compared by identity), or None.  Entries
        grounded at another capacity_scale than `scale` (a retry raised it
        since) and those queued before the match (batches that ran without
        their lookahead) are dropped; entries after it are later batches and
        stay queued.  peek: leave the match queued."""
        live = [e for e in self.entries if e.scale == scale]
        self.retain(live)
        for i, e in enumerate(live):
            if all(a is b for a, b in zip(e.rows, rows)):
                self.retain(live[i:])
                if peek:
                    return e
                self.model.prefetch_hits += 1
                return self.entries.popleft()
        return None  # these rows were not grounded ahead; the queued ones are later batches

    def retain(self, entries):
        """Drop, and count, every queued grounding but `entries`."""
        # the side stream's work on dropped entries still ends before their
        # ring slots come round again (record_stream, the slots' order)
        c, n = self.model, len(self.entries) - len(entries)
        if n:
            c.prefetch_dropped += n
            logging.debug("%s: %d lookahead groundings dropped (%d so far)", type(c).__name__, n, c.prefetch_dropped)
            self.entries = collections.deque(entries)


class Lookahead(LookaheadQueue):
    """One model's lookahead on one device: the queue and the GPU resources
    behind it; follows model.prefetch_depth."""

    def __init__(self, model, device):
        super(Lookahead, self).__init__(model)
        n = ctypes.c_size_t()
        _native.call("rnnl_forward_header_bytes", ctypes.byref(n))
        self.header_bytes = n.value
        self.stream = torch.cuda.Stream(device)
        # depth + 1 workspaces: the forward in flight keeps one until its backward
        self.ring = {}
        self.next = 0
        self.grounded = self._host_ring(model.prefetch_depth + 1)  # one per workspace slot
        # the scoring passes' headers, read two forwards late: at most 2 are pending
        self.scored = self._host_ring(4)
        self.deferred = collections.deque()
        self.forwards = 0
        # PredictorPlus: the node records' range flag (int32), waited on within the forward
        self.node_flag = (torch.zeros(4, dtype=torch.uint8, pin_memory=True), torch.cuda.Event())

    def _host_ring(self, n):
        """n (pinned header buffer, event) pairs, reused instead of a pinned
        allocation and an event creation per step."""
        hb = self.header_bytes + 8  # + the first row's relation (int64)
        return [(torch.empty(hb, dtype=torch.uint8, pin_memory=True), torch.cuda.Event()) for _ in range(n)]

    def reset(self):
        """Forget the queued groundings and their workspaces (new rules).  The
        pending scoring statuses stay: check_deferred still reports them."""
        self.entries.clear()
        self.ring = {}

    def slot(self, nbytes, device):
        """The next ring slot: (workspace of at least nbytes, pinned header,
        event).  The slot's previous entry was consumed, or dropped behind the
        same side stream, before it comes round."""
        k = self.next % (self.model.prefetch_depth + 1)
        self.next += 1
        self.grounded += self._host_ring(k + 1 - len(self.grounded))  # (prefetch_depth was raised since)
        ws = self.ring.get(k)
        if ws is None or ws.numel() < nbytes:
            ws = self.ring[k] = torch.empty(nbytes, dtype=torch.uint8, device=device)
        return (ws,) + self.grounded[k]

    def defer(self, ws):
        """After a scoring pass on a grounding made ahead: its header copied
        behind it into a pinned ring slot, checked two forwards later
        (check_deferred) instead of waiting for the pass now."""
        hb = self.header_bytes
        self.forwards += 1
        dh, ev = self.scored[self.forwards % 4]
        dh[:hb].copy_(ws[:hb], non_blocking=True)
        ev.record(torch.cuda.current_stream(ws.device))
        self.deferred.append((dh, ev, self.forwards))

    def check_deferred(self, keep):
        q = self.deferred
        while len(q) > keep:
            dh, ev, n = q.popleft()
            ev.synchronize()
            rc = _native.lib().rnnl_forward_status_host(dh.data_ptr(), None)
            if rc != _native.RNNL_OK:
                q.clear()
                raise _native.NativeError(rc, "%s (scoring pass of lookahead forward #%d, read late: that step's "
                                              "backward and optimizer update have already been applied)" % (
                                                  _native.lib().rnnl_last_error().decode(errors="replace"), n))
