"""Time the rule search with bodies of up to five relations (rnnl_rule_search_long)
and learn + H score at length 4 against the reference miner on the same box
(its search through oracle/_ref/libref_miner.so, its CLI oracle/_ref/rnnlogic,
both with 16 threads).  Sibling of tools/mine_timing.py, same protocol: one
warm-up, then the median of --runs (device events around the call, wall time
beside them).  Not part of bench.py.

    search(4) on UMLS                       keys only (search_keys) and with the decode to tuples (search)
    search(5) on the E = 300 synthetic graph of tests/golden/_rules_long_sparse300.npz
    search(3) on UMLS and kinship           the untouched kernel, re-measured
    learn + H score at length 4 on UMLS     mine(4, one iteration, top_n 100), the search timed apart

Usage: python tools/mine_long_timing.py [--runs 5] [--ref-runs 3] [--no-ref] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from rnnlogic_amd import datasets  # noqa: E402
from rnnlogic_amd.data import KnowledgeGraph  # noqa: E402
from rnnlogic_amd.miner import RuleMiner  # noqa: E402

CLI = os.path.join(REPO, "oracle", "_ref", "rnnlogic")
LR, WD, TEMP = 0.01, 0.0005, 100.0


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


def write_dataset(path, tri, E, R):
    with open(os.path.join(path, "entities.dict"), "w") as fo:
        fo.writelines("%d\te%d\n" % (e, e) for e in range(E))
    with open(os.path.join(path, "relations.dict"), "w") as fo:
        fo.writelines("%d\tr%d\n" % (r, r) for r in range(R))
    for name, triples in (("train.txt", tri), ("valid.txt", tri[:1]), ("test.txt", tri[:1])):
        with open(os.path.join(path, name), "w") as fo:
            fo.writelines("e%d\tr%d\te%d\n" % tuple(t) for t in triples)


def reference_search(path, L, runs):
    from oracle import ground_c
    secs, n = [], 0
    for _ in range(runs + 1):
        m = ground_c.RefMiner(path)
        rules, sec = m.rule_search(L, threads=16)
        m.close()
        secs.append(sec)
        n = len(rules)
    return dict(rules=n, seconds=dict(median=statistics.median(secs[1:]), min=min(secs[1:]), max=max(secs[1:])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--ref-runs", type=int, default=3)
    ap.add_argument("--no-ref", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ref = not a.no_ref and os.path.exists(os.path.join(REPO, "oracle", "_ref", "libref_miner.so"))
    res = []

    def emit(row):
        res.append(row)
        print(json.dumps(row), flush=True)

    umls = datasets.materialize("umls")
    for data, L in (("umls", 3), ("kinship", 3), ("umls", 4)):
        path = datasets.materialize(data)
        miner = RuleMiner(KnowledgeGraph(path), dev, max_body=5)
        keys, out = timed(lambda: miner.search_keys(L), a.runs)
        full, rules = timed(lambda: miner.search(L), a.runs)
        row = dict(what="search", data=data, max_length=L, rules=len(out), gpu_keys=keys, gpu_with_decode=full)
        if ref and L == 4:
            row["reference_16_threads"] = reference_search(path, L, a.ref_runs)
        emit(row)

    z = np.load(os.path.join(REPO, "tests", "golden", "_rules_long_sparse300.npz"))
    tri, E, R = [tuple(int(x) for x in t) for t in z["triples"]], int(z["E"]), int(z["R"])
    miner = RuleMiner(types.SimpleNamespace(train_facts=tri, entity_size=E, relation_size=R), dev, max_body=5)
    keys, out = timed(lambda: miner.search_keys(5), a.runs)
    row = dict(what="search", data="sparse300", max_length=5, rules=len(out), gpu_keys=keys)
    if ref:
        with tempfile.TemporaryDirectory() as tmp:
            write_dataset(tmp, tri, E, R)
            row["reference_16_threads"] = reference_search(tmp, 5, a.ref_runs)
    emit(row)

    # learn + H score at length 4, 100 rules per relation drawn from the pool
    graph = KnowledgeGraph(umls)
    miner = RuleMiner(graph, dev, max_body=4)
    miner.search(4)
    learn, _ = timed(lambda: miner.mine(4, 1, 100, 0, LR, WD, TEMP, 100, seed=0), a.runs)
    row = dict(what="learn + H score", data="umls", max_length=4, top_n=100, pool=len(miner.rules), gpu=learn)
    if ref and os.path.exists(CLI):
        walls = []
        with tempfile.TemporaryDirectory() as tmp:
            for _ in range(a.ref_runs + 1):
                t0 = time.perf_counter()
                subprocess.run([CLI, "-data-path", umls, "-output-file", os.path.join(tmp, "r.txt"), "-max-length",
                                "4", "-threads", "16", "-iterations", "1", "-lr", str(LR), "-wd", str(WD), "-temp",
                                str(TEMP), "-top-k", "0", "-top-n", "100", "-top-n-out", "100"], check=True,
                               stdout=subprocess.DEVNULL)
                walls.append(time.perf_counter() - t0)
        row["reference_cli_16_threads_wall_s_with_its_search"] = dict(median=statistics.median(walls[1:]),
                                                                      min=min(walls[1:]), max=max(walls[1:]))
    emit(row)
    if a.out:
        with open(a.out, "w") as fo:
            json.dump(res, fo, indent=1)


if __name__ == "__main__":
    main()
