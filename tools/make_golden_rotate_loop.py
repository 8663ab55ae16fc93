"""Records what the RotatE DIRECT scorer computes on the small shapes of
tests/test_gpu_rotate_loop.py into tests/golden/_rotate_loop_parent.npz.

The fixture pins the scorer's bits across a rewrite of its inner loop: it is
generated on the GPU in a checkout of the commit BEFORE the rewrite (only
this file is added there) and the test compares the rewritten kernels with
it, so the expected values never come from the code under test.  Only the
public RotatE API is used.

  python tools/make_golden_rotate_loop.py [OUT.npz]

Per case: sha/<key> = sha256 of the float32 output bytes; out/<key> = the
output itself for the one-chunk cases (D <= 32).  The file name starts with
an underscore because tests/conftest.py lists every other tests/golden/*.npz
as a forward-fixture case.
"""
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

GOLDEN = os.path.join(REPO, "tests", "golden", "_rotate_loop_parent.npz")
GAMMA = 9.0
NREL = 3
SMALL_D = (1, 2, 3, 4, 5, 7, 31, 32)  # one DCH chunk: always the one-pass kernel
SMALL_E = (1, 257)
SMALL_ROWS = (1, 21)
BIG_D = (33, 34, 35, 36, 37, 63, 64, 65, 67)  # two or three chunks: the rebased descriptor
BIG_E = 257  # two entity tiles
BIG_ROWS = 10241  # 513 query groups x 2 tiles = 1,026 blocks: the one-pass grid
SPLIT_ROWS = 45  # 3 query groups x 2 tiles: the split form


def key(D, E, rows):
    return "D%d_E%d_n%d" % (D, E, rows)


def small_cases():
    return [(D, E, n) for D in SMALL_D for E in SMALL_E for n in SMALL_ROWS]


def big_cases():
    return [(D, BIG_E, n) for D in BIG_D for n in (BIG_ROWS, SPLIT_ROWS)]


def hr_f64(eemb, remb2, h, r):
    """float64 (re, im) of h o r (embedding.py:55-61, fp32 phase divisor);
    remb2 is the (2 nrel, D) table with the negated half."""
    D = eemb.shape[1] // 2
    div = np.float32((GAMMA + 2.0) / D / np.pi)
    ph = (remb2[r] / div).astype(np.float64)
    hh = eemb.astype(np.float64)[h]
    re = hh[:, :D] * np.cos(ph) - hh[:, D:] * np.sin(ph)
    im = hh[:, :D] * np.sin(ph) + hh[:, D:] * np.cos(ph)
    return re, im


def make_inputs(D, E):
    """(eemb (E, 2D), remb (NREL, D), h, r) from a fixed seed, values of the
    trained tables' magnitude (up to twice the initial range (gamma + 2) / D,
    as the shipped UMLS table).  Every row prefix is a case's query list:
    row 0 queries relation 0, whose phases are zero, with a head that is a
    candidate (distance exactly 0, score exactly gamma); entity `near` (E > 1)
    is row 1's h o r plus 1e-6 noise."""
    rng = np.random.default_rng([20240607, D, E])
    rows = BIG_ROWS if E == BIG_E else max(SMALL_ROWS)
    span = 2.0 * (GAMMA + 2.0) / D
    eemb = rng.uniform(-span, span, (E, 2 * D)).astype(np.float32)
    remb = rng.uniform(-span, span, (NREL, D)).astype(np.float32)
    remb[0] = 0.0
    h = rng.integers(0, E, rows)
    r = rng.integers(0, 2 * NREL, rows)
    r[0] = 0
    if E > 1:
        near = int((h[1] + 1) % E)
        if near == h[0]:
            near = int((near + 1) % E)
        if near == h[1]:  # E == 2 cannot happen here; keep the head rows untouched
            raise AssertionError("no free entity for the near match")
        re, im = hr_f64(eemb, np.concatenate([remb, -remb]), h[1:2], r[1:2])
        eemb[near, :D] = (re[0] + rng.normal(0, 1e-6, D)).astype(np.float32)
        eemb[near, D:] = (im[0] + rng.normal(0, 1e-6, D)).astype(np.float32)
    return eemb, remb, h, r


def write_tables(path, eemb, remb):
    """The layout RotatE(path) reads."""
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as fo:
        json.dump({"hidden_dim": remb.shape[1], "gamma": GAMMA, "nentity": eemb.shape[0], "nrelation": NREL}, fo)
    np.save(os.path.join(path, "entity_embedding.npy"), eemb)
    np.save(os.path.join(path, "relation_embedding.npy"), remb)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float32).tobytes()).hexdigest()


def main():
    import torch

    from rnnlogic_amd.embedding import RotatE
    out_path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    dev = torch.device("cuda:0")
    rec = {}
    with tempfile.TemporaryDirectory() as tmp:
        for D, E, n in small_cases() + big_cases():
            eemb, remb, h, r = make_inputs(D, E)
            path = os.path.join(tmp, "D%d_E%d" % (D, E))
            write_tables(path, eemb, remb)
            rot = RotatE(path).to(dev)
            with torch.no_grad():
                got = rot(torch.from_numpy(h[:n]).to(dev), torch.from_numpy(r[:n]).to(dev)).cpu().numpy()
            rec["sha/" + key(D, E, n)] = np.array(sha(got))
            if D <= 32:
                rec["out/" + key(D, E, n)] = got
            print(key(D, E, n), rec["sha/" + key(D, E, n)][()][:16], flush=True)
    np.savez_compressed(out_path, **rec)
    print("wrote %s (%d bytes)" % (out_path, os.path.getsize(out_path)))


if __name__ == "__main__":
    main()
