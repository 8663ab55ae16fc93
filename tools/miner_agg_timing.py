"""Time RuleMiner.eval_ranks over the whole test split under the three
aggregations (sum, noisy-or, max at depth 1 and 3), with the
fixture rules of tests/golden/_mine_eval_<data>.npz and their PCA confidences
as weights, on kinship and UMLS.  Not part of bench.py; a record, not a test.

Method: one process; one warm-up call per mode, then `--runs` calls per mode,
alternating sum, noisy-or, max, sum, ...; device-event time around eval_ranks
(upload of the queries, the kernel, the counter and rank read-backs); median,
minimum and maximum per mode, in seconds.  The pairs of a mode are checked to
be equal between the runs.  The yardstick of a new mode is the sum of the same
run.  `--modes sum` runs on a tree without set_aggregation as well, so the
same file times the sum of an earlier commit on the same input.

Usage: python tools/miner_agg_timing.py [--data kinship umls] [--runs 20] [--modes sum noisy_or max1 max3]
                                        [--out FILE]
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

MODES = {"sum": ("sum", 1), "noisy_or": ("noisy_or", 1), "max1": ("max", 1), "max3": ("max", 3)}


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


def fixture_rules(data):
    z = np.load(os.path.join(REPO, "tests", "golden", "_mine_eval_%s.npz" % data), allow_pickle=False)
    rel2rules = [[] for _ in range(int(z["n_relations"]))]
    for hd, ln, body in zip(z["rule_head"].tolist(), z["rule_len"].tolist(), z["rule_body"].tolist()):
        rel2rules[hd].append((hd, tuple(body[:ln])))
    return rel2rules


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", nargs="+", default=["kinship", "umls"])
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--modes", nargs="+", choices=sorted(MODES), default=["sum", "noisy_or", "max1", "max3"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []
    for data in a.data:
        graph = KnowledgeGraph(datasets.materialize(data))
        miner = RuleMiner(graph, dev)
        rules = fixture_rules(data)
        miner.set_logic_rules(rules)
        miner.set_weights(miner.confidence("pca"))
        secs, pairs = {m: [] for m in a.modes}, {}
        for run in range(a.runs + 1):
            for m in a.modes:
                if a.modes != ["sum"]:
                    miner.set_aggregation(*MODES[m])
                    miner.scores(graph.test_facts[:1])  # the operand goes up outside the timed call
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                torch.cuda.synchronize()
                ev[0].record()
                got = miner.eval_ranks(graph.test_facts)
                ev[1].record()
                torch.cuda.synchronize()
                if run:  # the first call of a mode is its warm-up
                    secs[m].append(ev[0].elapsed_time(ev[1]) / 1e3)
                assert m not in pairs or np.array_equal(pairs[m], got)
                pairs[m] = got
        res = dict(data=data, rules=sum(len(x) for x in rules), test_triples=len(graph.test_facts), runs=a.runs,
                   eval_ranks_events_s={m: spread(secs[m]) for m in a.modes},
                   over_sum={m: statistics.median(secs[m]) / statistics.median(secs["sum"]) for m in a.modes
                             if "sum" in a.modes},
                   pairs_differ_from_sum={m: bool(not np.array_equal(pairs[m], pairs["sum"])) for m in a.modes
                                          if "sum" in a.modes and m != "sum"})
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
