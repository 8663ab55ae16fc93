"""Times rnnl_topk_rows against the torch composition it replaces,
    torch.topk(torch.where(mask & flag, score, -inf), k),
at the headline shape: the FB15k-237 test split, 40,932 rows x 14,541 entities.

Inputs: random scores, a random mask at the split's candidate density
(tests/golden/fb15k237_work.json: candidates / (rows x entities)) and the
split's real filter flags (DeviceEvalBatches).  Per k (10 and 100): warm-up,
then the two paths alternate, each launch bracketed by device events; the
median, minimum and maximum over the repeats are reported, with the one-read
floor (6 n |E| bytes: a float, a mask byte and a flag byte per entry) at the
8 TB/s HBM peak and at the 6.3 TB/s a streaming kernel achieves.

`--scores ties` draws the scores from 8 values, the `bias` / `none` models'
case: every row's k-th place then falls inside a long tie run.

    python tools/topk_timing.py [--repeats 20] [--scores random|ties] [--out FILE]
prints one JSON line.  Needs a GPU.
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_PEAK, HBM_STREAM = 8.0e12, 6.3e12


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scores", choices=["random", "ties"], default="random")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("topk_timing needs a GPU")
    from rnnlogic_amd import datasets
    from rnnlogic_amd.data import DeviceEvalBatches, KnowledgeGraph, TestDataset
    from rnnlogic_amd.predictors import topk_rows
    from rnnlogic_amd.utils import set_seed

    dev = torch.device("cuda:0")
    set_seed(1)
    graph = KnowledgeGraph(datasets.materialize("FB15k-237"))
    test_set = TestDataset(graph, 32)
    _, _, _, flag = DeviceEvalBatches(test_set, dev).rows(list(range(len(test_set))))
    n, E = flag.shape
    with open(os.path.join(REPO, "tests", "golden", "fb15k237_work.json")) as f:
        work = json.load(f)
    density = work["C"] / (work["queries"] * float(E))
    gen = torch.Generator(device=dev).manual_seed(1)
    if args.scores == "random":
        score = torch.randn((n, E), device=dev, generator=gen)
    else:
        score = torch.randint(0, 8, (n, E), device=dev, generator=gen).float() * 0.5 - 2.0
    mask = torch.rand((n, E), device=dev, generator=gen) < density
    neg_inf = torch.full((), float("-inf"), device=dev)
    result = dict(tool="topk_timing", rows=n, entities=E, scores=args.scores, mask_density=round(density, 4),
                  flag_density=round(float(flag.float().mean()), 6), repeats=args.repeats,
                  floor_ms_at_8TBs=6.0 * n * E / HBM_PEAK * 1e3, floor_ms_at_6p3TBs=6.0 * n * E / HBM_STREAM * 1e3,
                  runs={})
    for k in (10, 100):
        ours = lambda: topk_rows(score, mask, flag, None, k)  # noqa: E731
        ref = lambda: torch.topk(torch.where(mask & flag, score, neg_inf), k)  # noqa: E731
        for _ in range(args.warmup):
            ours()
            ref()
        torch.cuda.synchronize()
        t_ours, t_ref = [], []
        for _ in range(args.repeats):  # alternating: both paths see the same neighbours on the machine
            ms, (index, value, valid) = timed(ours)
            t_ours.append(ms)
            ms, (rv, ri) = timed(ref)
            t_ref.append(ms)
        # the two agree on the values wherever the row has k eligible entries (torch's tie order is its own)
        full = valid == k
        same = bool(torch.equal(value[full], rv[full]))
        med_o, med_r = statistics.median(t_ours), statistics.median(t_ref)
        result["runs"]["k%d" % k] = dict(
            hip_ms=dict(median=med_o, min=min(t_ours), max=max(t_ours)),
            torch_ms=dict(median=med_r, min=min(t_ref), max=max(t_ref)),
            hip_over_torch=med_o / med_r, values_equal=same,
            fraction_of_floor_8TBs=result["floor_ms_at_8TBs"] / med_o,
            fraction_of_floor_6p3TBs=result["floor_ms_at_6p3TBs"] / med_o,
            not_slower=bool(med_o <= med_r))
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
