"""Time RuleMiner.mine (GPU) against the reference miner CLI with 16 threads
(oracle/_ref/rnnlogic, built by `make -C oracle ref`) on the same box:
UMLS and kinship at length 3, -top-n 0 -top-k 0 -iterations 1,
-lr 0.01 -wd 0.0005 -temp 100.  Not part of bench.py.

Method: one warm-up, then the median of 5.  The GPU run reports the search
and learn + H_score separately, each as device-event time (the events enclose
the host's chunk loop and its counter read-backs, which are part of the cost)
and the whole run as wall time including reading the dataset and writing the
rule file — the CLI's wall time includes both too, so the wall times are the
ones to compare.  The reference's 16-thread run is a lock-free race on the
weights; its time is comparable, its output is not.

Also printed: the relation whose chain bounds the learn kernel (one workgroup
walks a relation's triples in order): its triples, rules, (triple, rule) pairs
and grounding entries.

Usage: python tools/mine_timing.py [--data umls kinship] [--runs 5] [--no-ref]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from rnnlogic_amd import datasets  # noqa: E402
from rnnlogic_amd.data import KnowledgeGraph  # noqa: E402
from rnnlogic_amd.miner import RuleMiner  # noqa: E402

CLI = os.path.join(REPO, "oracle", "_ref", "rnnlogic")
LR, WD, TEMP, L = 0.01, 0.0005, 100.0, 3


def gpu_run(path, out_file):
    dev = torch.device("cuda:0")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    t0 = time.perf_counter()
    graph = KnowledgeGraph(path)
    miner = RuleMiner(graph, dev)
    ev[0].record()
    miner.search(L)
    ev[1].record()
    miner.mine(L, 1, 0, 0, LR, WD, TEMP, 0, seed=0)
    ev[2].record()
    torch.cuda.synchronize()
    miner.out_rules(out_file, 0)
    wall = time.perf_counter() - t0
    return dict(wall_s=wall, search_s=ev[0].elapsed_time(ev[1]) / 1e3, learn_h_s=ev[1].elapsed_time(ev[2]) / 1e3), miner


def chain_bound(miner):
    """The relation with the most grounding entries over its triples."""
    R = miner.graph.relation_size
    miner.set_logic_rules(miner.get_logic_rules())
    miner.learn(LR, WD, TEMP, order=np.arange(len(miner._hrt), dtype=np.int32))
    if miner._grounded is None:
        return None
    _, count, pb, _, pair_off, _, _, _ = miner._grounded[1]
    per_triple = (pair_off[pb[1:]] - pair_off[pb[:-1]]).cpu().numpy()
    rel = miner._hrt[:count, 1]
    entries = np.bincount(rel, weights=per_triple, minlength=R)
    r = int(np.argmax(entries))
    nr = int(miner._rule_off[r + 1] - miner._rule_off[r])
    nt = int(np.sum(rel == r))
    return dict(relation=r, triples=nt, rules=nr, pairs=nt * nr, entries=int(entries[r]),
                all_entries=int(entries.sum()), all_rules=int(miner._rule_off[-1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", nargs="+", default=["umls", "kinship"])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-ref", action="store_true")
    a = ap.parse_args()
    for data in a.data:
        path = datasets.materialize(data)
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, "rules.txt")
            runs = [gpu_run(path, out)[0] for _ in range(a.runs + 1)][1:]
            res = dict(data=data, max_length=L, runs=a.runs,
                       gpu={k: statistics.median(r[k] for r in runs) for k in runs[0]})
            _, miner = gpu_run(path, out)
            res["chain_bound"] = chain_bound(miner)
            if not a.no_ref and os.path.exists(CLI):
                walls = []
                for _ in range(a.runs + 1):
                    t0 = time.perf_counter()
                    subprocess.run([CLI, "-data-path", path, "-output-file", out, "-max-length", str(L), "-threads",
                                    "16", "-iterations", "1", "-lr", str(LR), "-wd", str(WD), "-temp", str(TEMP),
                                    "-top-k", "0", "-top-n", "0", "-top-n-out", "0"], check=True,
                                   stdout=subprocess.DEVNULL)
                    walls.append(time.perf_counter() - t0)
                res["reference_16_threads_wall_s"] = statistics.median(walls[1:])
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
