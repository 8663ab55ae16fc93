"""Times the RotatE training step on the HIP path — rnnl_kge_sample_negatives
plus rnnl_kge_rotate_step, without Adam — against the torch-eager composition
of the same step (tests/kge_ref.py step(): float32 forward and autograd
backward), with the same negatives, on the same GPU in the same run.

Shapes: the shipped UMLS configuration (data/umls/RotatE_50/config.json: the
trainer's first batch, B = N = 128, E = 135, D = 50), the same graph at
B = 1024, N = 256 (about 2,000 samples per entity), and B = 1024, N = 256,
E = 14,541, D = 1000 (seeded tables, random positives over 237 relations).
Per shape: warm-up, then the two paths alternate, each call bracketed by
device events; median, minimum and maximum over the repeats, and the largest
difference between the two paths' loss, d_eemb and d_remb.  The step is also
given as a fraction of its gather floor: the kernel's three passes (the
candidate rows twice, the query rows once) x B N 2D 4 bytes at the 5.5 and
5.8 TB/s of gathered whole rows.

    python tools/kge_timing.py [--repeats 20] [--out FILE]
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

GATHER_LO, GATHER_HI = 5.5e12, 5.8e12
PASSES = 3


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def umls_case(dev, name="umls_RotatE_50", **change):
    import kge_ref
    from rnnlogic_amd import datasets, kge
    from rnnlogic_amd.data import KnowledgeGraph
    cfg = dict(kge_ref.UMLS_50, **change)
    tr = kge.RotatETrainer(KnowledgeGraph(datasets.materialize("umls")), seed=0, device=dev, **cfg)
    idx = tr._next_batch()
    return dict(name=name, eemb=tr.eemb.detach(), remb=tr.remb.detach(), gamma=tr.gamma,
                alpha=tr.alpha, positives=tr.triples.index_select(0, idx), weights=tr.weights.index_select(0, idx),
                lists=tr.true["tail"], N=tr.negative_sample_size)


def umls_long_lists_case(dev):
    """A large batch on a small graph: about 2,000 items per entity, the regime
    where the entity kernel's rank sort (quadratic in the list) weighs most."""
    return umls_case(dev, name="umls_B1024_N256_D50", batch_size=1024, negative_sample_size=256)


def large_case(dev, B=1024, N=256, E=14541, D=1000, R=237, gamma=9.0):
    from rnnlogic_amd import kge
    from rnnlogic_amd.data import _DeviceLists
    rng = np.random.default_rng(0)
    rho = (gamma + 2.0) / D
    eemb = torch.from_numpy(rng.uniform(-rho, rho, (E, 2 * D)).astype(np.float32)).to(dev)
    remb = torch.from_numpy(rng.uniform(-rho, rho, (R, D)).astype(np.float32)).to(dev)
    pos = np.stack([rng.integers(0, E, B), rng.integers(0, R, B), rng.integers(0, E, B)], axis=1).astype(np.int64)
    weights = torch.from_numpy(rng.uniform(0.1, 0.5, B).astype(np.float32)).to(dev)
    return dict(name="B%d_N%d_E%d_D%d" % (B, N, E, D), eemb=eemb, remb=remb, gamma=gamma, alpha=1.0,
                positives=torch.from_numpy(pos).to(dev), weights=weights,
                lists=_DeviceLists(kge.true_answers(pos, E, "tail"), dev), N=N)


def run_case(c, repeats, warmup):
    import kge_ref
    from rnnlogic_amd import kge
    dev = c["eemb"].device
    (E, D2), (B, N) = c["eemb"].shape, (c["positives"].size(0), c["N"])
    D = D2 // 2
    scratch = kge.step_scratch(B, N, E, D, dev)
    d_eemb, d_remb = torch.empty_like(c["eemb"]), torch.empty_like(c["remb"])
    capped = torch.zeros(1, dtype=torch.int32, device=dev)
    state = {"step": 0}

    def hip():
        state["step"] += 1
        neg = kge.sample_negatives(c["lists"], c["positives"], 0, E, N, 0, state["step"], capped)
        return neg, kge.rotate_step(c["eemb"], c["remb"], c["gamma"], c["positives"], neg, c["weights"], 0, c["alpha"],
                                    scratch, d_eemb, d_remb)

    def hip_step_only(neg):
        return kge.rotate_step(c["eemb"], c["remb"], c["gamma"], c["positives"], neg, c["weights"], 0, c["alpha"],
                               scratch, d_eemb, d_remb)

    def eager(neg):
        e = c["eemb"].clone().requires_grad_(True)
        r = c["remb"].clone().requires_grad_(True)
        _, _, losses = kge_ref.step(e, r, c["gamma"], c["positives"], neg, c["weights"], 0, c["alpha"])
        losses[2].backward()
        return losses[2].detach(), e.grad, r.grad

    for _ in range(warmup):
        neg, _ = hip()
        hip_step_only(neg)
        eager(neg)
    torch.cuda.synchronize()
    t_hip, t_step, t_ref, worst = [], [], [], 0.0
    for _ in range(repeats):  # alternating: both paths see the same neighbours on the machine
        ms, (neg, out) = timed(hip)
        t_hip.append(ms)
        loss, ge, gr = out[2][2].clone(), out[3].clone(), out[4].clone()
        ms, _ = timed(lambda: hip_step_only(neg))
        t_step.append(ms)
        ms, (rl, rge, rgr) = timed(lambda: eager(neg))
        t_ref.append(ms)
        worst = max(worst, float((loss - rl).abs()), float((ge - rge).abs().max()), float((gr - rgr).abs().max()))
    gather = PASSES * B * N * D2 * 4.0
    med = statistics.median
    stat = lambda t: dict(median=med(t), min=min(t), max=max(t))  # noqa: E731
    return dict(B=B, N=N, E=E, D=D, capped=int(capped.item()), hip_ms=stat(t_hip), hip_step_only_ms=stat(t_step),
                torch_ms=stat(t_ref), hip_over_torch=med(t_hip) / med(t_ref), not_slower=bool(med(t_hip) <= med(t_ref)),
                max_abs_difference=worst, gather_bytes=gather,
                floor_ms_at_5p5TBs=gather / GATHER_LO * 1e3, floor_ms_at_5p8TBs=gather / GATHER_HI * 1e3,
                step_fraction_of_floor_5p5TBs=gather / GATHER_LO * 1e3 / med(t_step),
                step_fraction_of_floor_5p8TBs=gather / GATHER_HI * 1e3 / med(t_step))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kge_timing needs a GPU")
    dev = torch.device("cuda:0")
    result = dict(tool="kge_timing", repeats=args.repeats, passes=PASSES, runs={})
    for make in (umls_case, umls_long_lists_case, large_case):
        c = make(dev)
        result["runs"][c["name"]] = run_case(c, args.repeats, args.warmup)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
