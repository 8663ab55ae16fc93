"""Time RuleMiner.eval_ranks over the whole test split on the head side next
to the tail side, with all length-3 rules and weights from one
learn(), on kinship and UMLS.  Not part of bench.py; a record, not a test.

Method: one process; one warm-up call per side, then `--runs` calls per side,
alternating tail, head, tail, ...; device-event time around eval_ranks (upload
of the queries, the kernel, the counter and rank read-backs); median, minimum
and maximum per side, in seconds.  The pairs of the two sides are checked to
differ and to be equal between the runs.

Usage: python tools/mine_heads_timing.py [--data kinship umls] [--runs 20] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from rnnlogic_amd import datasets  # noqa: E402
from rnnlogic_amd.data import KnowledgeGraph  # noqa: E402
from rnnlogic_amd.miner import RuleMiner  # noqa: E402

LR, WD, TEMP, L = 0.01, 0.0005, 100.0, 3


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", nargs="+", default=["kinship", "umls"])
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []
    for data in a.data:
        graph = KnowledgeGraph(datasets.materialize(data))
        miner = RuleMiner(graph, dev)
        rules = miner.search(L)
        miner.set_logic_rules(miner.get_logic_rules())
        miner.learn(LR, WD, TEMP)
        secs, pairs = {"tail": [], "head": []}, {}
        for run in range(a.runs + 1):
            for side in ("tail", "head"):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                torch.cuda.synchronize()
                ev[0].record()
                got = miner.eval_ranks(graph.test_facts, side=side)
                ev[1].record()
                torch.cuda.synchronize()
                if run:  # the first call of a side is its warm-up
                    secs[side].append(ev[0].elapsed_time(ev[1]) / 1e3)
                assert side not in pairs or np.array_equal(pairs[side], got)
                pairs[side] = got
        assert not np.array_equal(pairs["tail"], pairs["head"])
        res = dict(data=data, max_length=L, rules=len(rules), test_triples=len(graph.test_facts), runs=a.runs,
                   tail_eval_ranks_events_s=spread(secs["tail"]), head_eval_ranks_events_s=spread(secs["head"]),
                   head_over_tail=statistics.median(secs["head"]) / statistics.median(secs["tail"]),
                   metrics={side: miner.evaluate("test", side=side) for side in ("tail", "head", "both")})
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
