"""Time the rule statistics of a searched pool (RuleMiner.pool_stats ->
rnnl_miner_rule_stats, csrc/mine_stats.hip) against the strongest simple torch
composition of the same counts, in the same run on the same GPU.  Sibling of
tools/mine_timing.py, same protocol: one warm-up, then the median and min-max
of --runs (device events around the call, wall time beside them).  Not part of
bench.py.

The torch composition is dense: one E x E fp32 0/1 matrix per relation; level
by level one torch.bmm over the distinct body prefixes of that length,
thresholded at > 0; then per body support under every head as one matmul with
the flattened relation matrices, pca_body as the row sums times the "has a
tail" vectors, body as their total; gathered per rule.  Both sides get the
rules grouped on the host beforehand (distinct bodies / distinct prefixes);
both end with their counts on the host, and the two are compared.

    UMLS and kinship at length 3, UMLS at length 4
    a sparse synthetic graph above the LDS regime (E = 3,000, 4 relations, length 3)

FB15k-237 cannot be timed: its train.txt is not in the repository.

Usage: python tools/mine_stats_timing.py [--runs 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from rnnlogic_amd import datasets  # noqa: E402
from rnnlogic_amd.data import KnowledgeGraph  # noqa: E402
from rnnlogic_amd.miner import MAX_BODY, RuleMiner, group_rules  # noqa: E402


def timed(fn, runs):
    """median (min, max) of device-event and wall seconds over `runs` calls after one warm-up."""
    ev, wall = [], []
    for k in range(runs + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
        ev.append(a.elapsed_time(b) / 1e3)
    med = lambda v: dict(median=statistics.median(v[1:]), min=min(v[1:]), max=max(v[1:]))  # noqa: E731
    return dict(events_s=med(ev), wall_s=med(wall)), out


class DenseComposition(object):
    """The prefix tables on the host once; run() is the timed device part."""

    def __init__(self, triples, E, R, body_len, body_rel, dev, batch_bytes=1 << 30):
        self.E, self.R, self.dev = E, R, dev
        A = torch.zeros((R, E, E), dtype=torch.float32)
        t = torch.as_tensor(np.asarray(triples, dtype=np.int64).reshape(-1, 3))
        A[t[:, 1], t[:, 0], t[:, 2]] = 1.0
        self.A = A.to(dev)
        self.A_flat_t = self.A.reshape(R, E * E).t().contiguous()
        self.has_tail_t = (self.A.sum(2) > 0).float().t().contiguous()  # (E, R)
        self.batch = max(1, batch_bytes // (4 * E * E))
        # level k: the distinct prefixes of length k, each with its parent at level k - 1 and last relation;
        # body_at[k] = (indices of the bodies of length k, their prefix at level k)
        empty = np.flatnonzero(body_len == 0)
        self.levels, self.body_at = [], [(empty, np.zeros(len(empty), np.int64))]
        prev_of_body = np.zeros(len(body_len), dtype=np.int64)
        for k in range(1, MAX_BODY + 1):
            live = np.flatnonzero(body_len >= k)
            if len(live) == 0:
                break
            key = prev_of_body[live] * R + body_rel[live, k - 1]
            ukey, inv = np.unique(key, return_inverse=True)
            self.levels.append((torch.as_tensor(ukey // R).to(dev), torch.as_tensor(ukey % R).to(dev)))
            prev_of_body[live] = inv.reshape(-1)
            ends = body_len[live] == k
            self.body_at.append((live[ends], inv.reshape(-1)[ends]))
        self.n_bodies = len(body_len)

    def _counts(self, M):
        rows = M.sum(2)
        return M.reshape(len(M), -1) @ self.A_flat_t, rows @ self.has_tail_t, rows.sum(1)

    @torch.no_grad()
    def run(self):
        """(support (bodies, R), pca_body (bodies, R), body (bodies,)) as int64 numpy."""
        E, R, dev = self.E, self.R, self.dev
        sup = torch.zeros((self.n_bodies, R), dtype=torch.float32, device=dev)
        pca = torch.zeros((self.n_bodies, R), dtype=torch.float32, device=dev)
        bod = torch.zeros(self.n_bodies, dtype=torch.float32, device=dev)
        prev = torch.eye(E, dtype=torch.float32, device=dev)[None]
        idx, _ = self.body_at[0]
        if len(idx):
            s, p, b = self._counts(prev)
            sup[idx], pca[idx], bod[idx] = s, p, b
        for k, (parent, rel) in enumerate(self.levels, 1):
            last = k == len(self.levels)
            cur = None if last else torch.empty((len(parent), E, E), dtype=torch.float32, device=dev)
            idx, at = self.body_at[k]
            order = np.argsort(at, kind="stable")
            idx, at = torch.as_tensor(idx[order]).to(dev), at[order]
            for b0 in range(0, len(parent), self.batch):
                b1 = min(len(parent), b0 + self.batch)
                M = (torch.bmm(prev[parent[b0:b1]], self.A[rel[b0:b1]]) > 0).float()
                if cur is not None:
                    cur[b0:b1] = M
                lo, hi = np.searchsorted(at, [b0, b1])
                if hi > lo:
                    s, p, b = self._counts(M[torch.as_tensor(at[lo:hi] - b0).to(dev)])
                    sup[idx[lo:hi]], pca[idx[lo:hi]], bod[idx[lo:hi]] = s, p, b
            prev = cur
        return (sup.cpu().numpy().astype(np.int64), pca.cpu().numpy().astype(np.int64),
                bod.cpu().numpy().astype(np.int64))


def sparse_graph(E=3000, R=4, per_entity=5, seed=1):
    rng = np.random.default_rng(seed)
    n = E * per_entity
    return [(int(h), int(r), int(t)) for h, r, t in zip(rng.integers(0, E, n), rng.integers(0, R, n),
                                                        rng.integers(0, E, n))], E, R


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = []
    cases = [("umls", 3), ("kinship", 3), ("umls", 4), ("sparse3000", 3)]
    for data, L in cases:
        if data == "sparse3000":
            tri, E, R = sparse_graph()
            graph = types.SimpleNamespace(train_facts=tri, entity_size=E, relation_size=R)
        else:
            graph = KnowledgeGraph(datasets.materialize(data))
            tri, E, R = graph.train_facts, graph.entity_size, graph.relation_size
        miner = RuleMiner(graph, dev, max_body=5)
        miner.search(L)
        head, ln, body = miner._pool_arrays
        t0 = time.perf_counter()
        grouped = group_rules(head, ln, body, R)
        group_s = time.perf_counter() - t0
        body_len, body_rel, head_off, head_rel, body_of, slot_of = grouped
        ours, got = timed(lambda: miner._stats_grouped(grouped), a.runs)

        def whole():
            miner._pool_stats = None
            return miner.pool_stats()
        whole_t, _ = timed(whole, a.runs)
        dense = DenseComposition(tri, E, R, body_len, body_rel, dev)
        theirs, (sup, pca, bod) = timed(dense.run, a.runs)
        same = (np.array_equal(got[0], sup[body_of, head]) and np.array_equal(got[1], bod[body_of]) and
                np.array_equal(got[2], pca[body_of, head]))
        row = dict(data=data, max_length=L, entities=E, relations=R, rules=len(head), bodies=len(body_len),
                   slots=len(head_rel), rules_with_support_0=int((got[0] == 0).sum()), host_grouping_s=group_s,
                   rule_stats=ours, pool_stats_with_grouping=whole_t, torch_dense=theirs,
                   ratio_torch_over_ours_events=theirs["events_s"]["median"] / ours["events_s"]["median"],
                   counts_equal=bool(same))
        res.append(row)
        print(json.dumps(row), flush=True)
        del dense, miner
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fo:
            json.dump(res, fo, indent=1)
    if not all(r["counts_equal"] for r in res):
        sys.exit("the two sides disagree")


if __name__ == "__main__":
    main()
