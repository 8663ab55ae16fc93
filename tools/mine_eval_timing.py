"""Time RuleMiner.evaluate("test") (GPU) with all length-3 rules, weights from
one learn(), on kinship and UMLS; next to it the reference miner's out_test
over the same split and rules with 16 threads, through the oracle/_ref shim
(oracle.ground_c.RefMiner.out_test_timed) on the same box.  Not part of
bench.py; a record, not a test.

Method: one warm-up, then 5 runs; median, minimum and maximum.  The GPU time
is device-event time around eval_ranks (upload of the queries, the kernel, the
counter and rank read-backs) and, separately, the wall time of evaluate()
including the host's metric sums.  out_test is the reference's grounding pass
only (no scores, no ranking), so the comparison flatters the reference.

Usage: python tools/mine_eval_timing.py [--data kinship umls] [--runs 5] [--no-ref]
"""
import argparse
import json
import os
import statistics
import sys
import time

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
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-ref", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for data in a.data:
        path = datasets.materialize(data)
        graph = KnowledgeGraph(path)
        miner = RuleMiner(graph, dev)
        rules = miner.search(L)
        miner.set_logic_rules(miner.get_logic_rules())
        miner.learn(LR, WD, TEMP)
        ranks_s, wall_s, metrics = [], [], None
        for _ in range(a.runs + 1):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            ev[0].record()
            miner.eval_ranks(graph.test_facts)
            ev[1].record()
            torch.cuda.synchronize()
            ranks_s.append(ev[0].elapsed_time(ev[1]) / 1e3)
            t0 = time.perf_counter()
            metrics = miner.evaluate("test")
            wall_s.append(time.perf_counter() - t0)
        res = dict(data=data, max_length=L, rules=len(rules), test_triples=len(graph.test_facts), runs=a.runs,
                   gpu_eval_ranks_events_s=spread(ranks_s[1:]), gpu_evaluate_wall_s=spread(wall_s[1:]),
                   metrics=metrics)
        if not a.no_ref:
            from oracle import ground_c
            if os.path.exists(ground_c.REF_LIB):
                ref = ground_c.RefMiner(path)
                secs = [ref.out_test_timed(rules, 16, -1)[0] for _ in range(a.runs + 1)]
                ref.close()
                res["reference_out_test_16_threads_s"] = spread(secs[1:])
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
