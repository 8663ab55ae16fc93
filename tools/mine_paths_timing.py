"""Times RuleMiner.explain_paths next to RuleMiner.explain on the same queries
and slots, in one process, on the workloads of §3.16's table:
  - the kinship and UMLS fixture rules (tests/golden/_mine_eval_*.npz) over
    their test splits: the LDS regime (|E| <= 512);
  - datasets.rule_file("wn18rr") over WN18RR's test split with weights drawn
    once from a seeded normal generator: the global-memory regime.

Slots: the first 3 places of predict_topk(k=10) per test query; rules: the 3
that explain lists per slot; P = 3 paths per rule.  Warm-up, then the two
calls alternate, each bracketed by device events (both end with the read of
their error counters, so the host side is inside); median, minimum and maximum
over the repeats, in milliseconds.  explain grounds every rule of the query's
relation, explain_paths the distinct rules among the 9 named ones, one at a
time with all levels kept; `distinct_rules_per_query` is their mean number.
The counts of the two calls are checked to be equal.

    python tools/mine_paths_timing.py [--repeats 20] [--data kinship,umls,wn18rr] [--side tail] [--out FILE]
prints one JSON line.  Needs a GPU.  Not part of bench.py; a record, not a test.
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
sys.path.insert(0, os.path.join(REPO, "tools"))
from mine_predict_timing import load, stats, timed  # noqa: E402  (the same workloads, the same clock)

SLOTS, RULES, P = 3, 3, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--data", default="kinship,umls,wn18rr")
    ap.add_argument("--side", default="tail", choices=["tail", "head"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mine_paths_timing needs a GPU")
    dev = torch.device("cuda:0")
    result = dict(tool="mine_paths_timing", repeats=args.repeats, side=args.side, slots=SLOTS, rules_per_slot=RULES,
                  paths_per_rule=P, runs={})
    for data in args.data.split(","):
        graph, miner = load(data, dev)
        q = np.asarray(graph.test_facts, dtype=np.int64).reshape(-1, 3)
        n, E = len(q), graph.entity_size
        index = miner.predict_topk(q, 10, side=args.side)[0][:, :SLOTS].contiguous()
        rule = miner.explain(q, index, RULES, args.side)[2]
        calls = dict(explain=lambda: miner.explain(q, index, RULES, args.side),
                     explain_paths=lambda: miner.explain_paths(q, index, rule, P, args.side))
        for _ in range(args.warmup):
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        ms, out = {name: [] for name in calls}, {}
        for _ in range(args.repeats):  # alternating: both calls see the same neighbours on the machine
            for name, fn in calls.items():
                t, out[name] = timed(fn)
                ms[name].append(t)
        listed, count, path = out["explain_paths"]
        assert torch.equal(count, out["explain"][3]) and torch.equal(rule, out["explain"][2])
        named = rule.reshape(n, -1).cpu().numpy()
        distinct = float(np.mean([len(set(row[row >= 0].tolist())) for row in named]))
        med = {name: statistics.median(v) for name, v in ms.items()}
        result["runs"][data] = dict(
            queries=n, entities=E, rules=int(miner._rule_off[-1]), regime="lds" if E <= 512 else "global",
            distinct_rules_per_query=distinct, entries_with_paths=int((count > 0).sum()),
            entries_cut=int((count > P).sum()), paths_listed=int(listed.sum()), max_count=int(count.max()),
            explain_ms=stats(ms["explain"]), explain_paths_ms=stats(ms["explain_paths"]),
            paths_over_explain=med["explain_paths"] / med["explain"])
        print("%s: done" % data, file=sys.stderr, flush=True)
        del miner
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
