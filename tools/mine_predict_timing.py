"""Times RuleMiner.predict_topk against the composition it replaces,
    val  = miner.scores(queries)                                  # (n, |E|) float64
    mask = the filter flags of the known-tail lists, t re-admitted
    torch.topk(torch.where(mask, val, -inf), k),
in the same process, on
  - the kinship and UMLS fixture rules (tests/golden/_mine_eval_*.npz) over
    their test splits: the LDS regime (|E| <= 512);
  - datasets.rule_file("wn18rr") over WN18RR's test split: the global-memory
    regime.  That file carries no weights; they are drawn once from a seeded
    normal generator (all-zero weights would make every score a tie).

Per workload and k (10 and 100), filtered: warm-up, then the paths alternate,
each call bracketed by device events (the calls end with the read of their
error counters, so the host side is inside); median, minimum and maximum over
the repeats.  The composition's mask admits every entity, so the like-for-like
path is candidates='all'; the default candidates='reached' is timed beside it.
eval_ranks on the same queries grounds the same rules and counts instead of
selecting: predict_topk minus eval_ranks is what the selection costs.

    python tools/mine_predict_timing.py [--repeats 20] [--data kinship,umls,wn18rr] [--out FILE]
prints one JSON line.  Needs a GPU.
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
sys.path.insert(0, os.path.join(REPO, "tests"))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def stats(ms):
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms))


def load(data, dev):
    from rnnlogic_amd import datasets
    from rnnlogic_amd.data import KnowledgeGraph
    from rnnlogic_amd.miner import RuleMiner
    graph = KnowledgeGraph(datasets.materialize(data))
    if data == "wn18rr":
        miner = RuleMiner(graph, dev, max_body=5)
        miner.read_rules(datasets.rule_file(data))
        rng = np.random.default_rng(0)
        miner.set_weights([rng.standard_normal(int(b - a)) for a, b in zip(miner._rule_off[:-1], miner._rule_off[1:])])
    else:
        import mine_eval_ref
        fx = mine_eval_ref.load_fixture(os.path.join(REPO, "tests", "golden", "_mine_eval_%s.npz" % data))
        miner = RuleMiner(graph, dev)
        miner.set_logic_rules(fx["rules"])
        miner.set_weights(fx["weights"])
    return graph, miner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--data", default="kinship,umls,wn18rr")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mine_predict_timing needs a GPU")
    dev = torch.device("cuda:0")
    neg_inf = torch.full((), float("-inf"), device=dev, dtype=torch.float64)
    result = dict(tool="mine_predict_timing", repeats=args.repeats, runs={})
    for data in args.data.split(","):
        graph, miner = load(data, dev)
        q = np.asarray(graph.test_facts, dtype=np.int64).reshape(-1, 3)
        n, E = len(q), graph.entity_size
        known = miner._known_tails()
        qd = torch.from_numpy(q).to(dev)
        row_keys = (qd[:, 1] * E + qd[:, 0]).contiguous()
        rows = torch.arange(n, device=dev)

        def composition(k):
            val = miner.scores(q)
            flag = known.rows("rnnl_filter_flags", row_keys, E, torch.empty((n, E), dtype=torch.uint8, device=dev))
            flag[rows, qd[:, 2]] = 1
            return torch.topk(torch.where(flag.bool(), val, neg_inf), k)

        entry = dict(queries=n, entities=E, rules=int(miner._rule_off[-1]), regime="lds" if E <= 512 else "global",
                     matrix_bytes=8 * n * E)
        for k in (10, 100):
            k = min(k, E)
            paths = dict(predict_all=lambda: miner.predict_topk(q, k, True, "all"),
                         predict_reached=lambda: miner.predict_topk(q, k, True, "reached"),
                         composition=lambda: composition(k),
                         eval_ranks=lambda: miner.eval_ranks(q))
            for _ in range(args.warmup):
                for fn in paths.values():
                    fn()
            torch.cuda.synchronize()
            ms = {name: [] for name in paths}
            out = {}
            for _ in range(args.repeats):  # alternating: every path sees the same neighbours on the machine
                for name, fn in paths.items():
                    t, out[name] = timed(fn)
                    ms[name].append(t)
            # the two agree on the values wherever the row has k eligible entities (torch's tie order is its own)
            full = out["predict_all"][2] == k
            same = bool(torch.equal(out["predict_all"][1][full], out["composition"][0][full]))
            med = {name: statistics.median(v) for name, v in ms.items()}
            entry["k%d" % k] = dict({name + "_ms": stats(v) for name, v in ms.items()},
                                    predict_over_composition=med["predict_all"] / med["composition"],
                                    not_slower=bool(med["predict_all"] <= med["composition"]),
                                    selection_ms=med["predict_all"] - med["eval_ranks"],
                                    selection_share=(med["predict_all"] - med["eval_ranks"]) / med["predict_all"],
                                    values_equal=same)
        result["runs"][data] = entry
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
