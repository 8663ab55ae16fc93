"""The RotatE DIRECT kernels' inner loop (rotate_direct_kernel and
rotate_split_kernel, csrc/rotate.hip): entity planes read through a buffer
descriptor that is rebased per 32-dim chunk, two register sets alternated by
an unroll over two 2-dim blocks, a look-ahead clamped at the last dim.  A
buffer load outside its descriptor returns 0 instead of faulting, so a wrong
offset shows only as wrong scores — on shapes around every boundary of that
loop, each output is compared

* bitwise with what the commit before the loop's rewrite computed for the
  same inputs (tests/golden/_rotate_loop_parent.npz, recorded there by
  tools/make_golden_rotate_loop.py, whose seeded inputs this file reuses);
* with a float64 evaluation of embedding.py:45-70, within the TOL that
  tests/test_gpu_forward.py applies to the DIRECT mode;
* bitwise with the accumulating, atomic and two-piece launches;
* (split form, 45 rows) bitwise with the first rows of the one-pass launch.

The opt-in MFMA kernel (mode = ROTATE_MFMA, the expanded bf16x3 form) runs the
same shapes against the float64 evaluation alone: within TOL on every entry
but the candidates at (nearly) zero distance, the expanded form's cancellation
case, which are held to the bound that tests/test_gpu_forward.py computes for
such rows (run_mfma_case).  The recorded parent outputs are the DIRECT
kernels' and do not apply to it.
"""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO

sys.path.insert(0, os.path.join(REPO, "tools"))
import make_golden_rotate_loop as gen  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-4  # tests/test_gpu_forward.py: entity scores within 1e-4 fp32

_golden = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def golden():
    if not _golden:
        _golden["z"] = np.load(os.path.join(GOLDEN, "_rotate_loop_parent.npz"), allow_pickle=False)
    return _golden["z"]


def rotate_f64(eemb, remb2, gamma, h, r, dev):
    """tests/test_gpu_forward.py's _rotate_f64 (float64 restatement of
    embedding.py:45-70, fp32 phase divisor): h o r in numpy float64, the
    (rows, E, D) distance sum in torch float64 on the device, in row blocks."""
    D = eemb.shape[1] // 2
    div = np.float32((gamma + 2.0) / D / np.pi)
    ph = (remb2[r] / div).astype(np.float64)
    e = eemb.astype(np.float64)
    hh = e[h]
    re = torch.from_numpy(hh[:, :D] * np.cos(ph) - hh[:, D:] * np.sin(ph)).to(dev)
    im = torch.from_numpy(hh[:, :D] * np.sin(ph) + hh[:, D:] * np.cos(ph)).to(dev)
    et = torch.from_numpy(e).to(dev)
    out = torch.empty((len(h), e.shape[0]), dtype=torch.float64, device=dev)
    for i in range(0, len(h), 1024):
        s = slice(i, i + 1024)
        out[s] = gamma - torch.sqrt((re[s, None] - et[None, :, :D]) ** 2 + (im[s, None] - et[None, :, D:]) ** 2).sum(2)
    return out


def run_case(tmp_path, dev, D, E, n):
    """The plain call's scores (device tensor) after the four checks."""
    from rnnlogic_amd.embedding import RotatE
    eemb, remb, h, r = gen.make_inputs(D, E)
    h, r = h[:n], r[:n]
    gen.write_tables(str(tmp_path), eemb, remb)
    rot = RotatE(str(tmp_path)).to(dev)
    hh, rr = torch.from_numpy(h).to(dev), torch.from_numpy(r).to(dev)
    with torch.no_grad():
        got = rot(hh, rr)
        # (1) bitwise the commit before the rewrite
        got_np = got.cpu().numpy()
        z, k = golden(), gen.key(D, E, n)
        assert gen.sha(got_np) == str(z["sha/" + k]), "%s: scores differ from the recorded parent output" % k
        if "out/" + k in z.files:
            assert np.array_equal(got_np, z["out/" + k]), k
        # (2) float64
        want = rotate_f64(eemb, np.concatenate([remb, -remb]), gen.GAMMA, h, r, dev)
        err = float((got.double() - want).abs().max())
        print("%s: max |score - f64| = %.3g" % (k, err))
        assert err <= TOL, "%s: max |score - f64| = %g" % (k, err)
        # row 0: zero phases, the head is a candidate — distance exactly 0
        assert float(got[0, h[0]]) == np.float32(gen.GAMMA), (k, float(got[0, h[0]]))
        # (3) the accumulating, the atomic and the two-piece launches
        acc = rot.score_into(hh, rr, torch.zeros_like(got), accumulate=True)
        assert torch.equal(acc, got), (k, "accumulate=True")
        atom = rot.score_into(hh, rr, torch.zeros_like(got), accumulate=2)
        assert torch.equal(atom, got), (k, "accumulate=2")
        pcs = rot.score_into(hh, rr, torch.full_like(got, float("nan")), pieces=2, first_share=0.37)
        assert torch.equal(pcs, got), (k, "pieces=2")
    return got


@pytest.mark.parametrize("D,E,n", gen.small_cases())
def test_one_chunk(D, E, n, dev, tmp_path):
    """D <= 32: one chunk, always the one-pass kernel (the unroll over two
    blocks and the look-ahead clamp at every D mod 4, one lane or two tiles,
    one row or two query groups)."""
    run_case(tmp_path, dev, D, E, n)


@pytest.mark.parametrize("D", gen.BIG_D)
def test_chunk_boundary(D, dev, tmp_path):
    """D > 32: the descriptor rebased per chunk, the look-ahead across the
    chunk boundary — 10,241 rows x 257 entities (1,026 blocks: the one-pass
    grid) and the same inputs' first 45 rows (the split form)."""
    big = run_case(tmp_path / "big", dev, D, gen.BIG_E, gen.BIG_ROWS)
    small = run_case(tmp_path / "split", dev, D, gen.BIG_E, gen.SPLIT_ROWS)
    # (4) the split form == the one-pass kernel on the same rows
    assert torch.equal(small, big[:gen.SPLIT_ROWS]), float((small - big[:gen.SPLIT_ROWS]).abs().max())


def mfma_reference(eemb, remb2, gamma, h, r, dev):
    """(float64 scores, per-entry allowance) for the expanded MFMA form.

    DESIGN.md "RotatE numerics": the form reaches each term's squared distance
    s_d = |hr_d - t_d|^2 through |hr_d|^2 + |t_d|^2 - 2 hr_d . t_d, with an
    absolute error of up to delta_d = c 2^-24 (|hr_d|^2 + |t_d|^2), c = 8.
    The term sqrt(s_d) then moves by at most
    max(sqrt(s_d + delta_d) - sqrt(s_d), sqrt(s_d) - sqrt(max(s_d - delta_d, 0))):
    sqrt(delta_d) where h o r = t — summed over d, the bound that
    tests/test_gpu_forward.py's test_rotate_scores_vs_float64 applies to its
    near-match rows — and ~delta_d / (2 sqrt(s_d)), far below TOL, on an
    ordinary entry.  Nothing here comes from the kernel under test."""
    D = eemb.shape[1] // 2
    div = np.float32((gamma + 2.0) / D / np.pi)
    ph = (remb2[r] / div).astype(np.float64)
    e = eemb.astype(np.float64)
    hh = e[h]
    re = torch.from_numpy(hh[:, :D] * np.cos(ph) - hh[:, D:] * np.sin(ph)).to(dev)
    im = torch.from_numpy(hh[:, :D] * np.sin(ph) + hh[:, D:] * np.cos(ph)).to(dev)
    et = torch.from_numpy(e).to(dev)
    tn = et[:, :D] ** 2 + et[:, D:] ** 2
    want = torch.empty((len(h), e.shape[0]), dtype=torch.float64, device=dev)
    allow = torch.empty_like(want)
    for i in range(0, len(h), 512):
        b = slice(i, i + 512)
        sq = (re[b, None] - et[None, :, :D]) ** 2 + (im[b, None] - et[None, :, D:]) ** 2
        delta = 8 * 2.0 ** -24 * ((re[b] ** 2 + im[b] ** 2)[:, None] + tn[None])
        root = torch.sqrt(sq)
        want[b] = gamma - root.sum(2)
        allow[b] = torch.maximum(torch.sqrt(sq + delta) - root, root - torch.sqrt((sq - delta).clamp(min=0))).sum(2)
    return want, allow


def run_mfma_case(tmp_path, dev, D, E, n):
    """Every entry within TOL, or within the expanded form's documented
    allowance where that is larger: the candidates at (nearly) zero distance
    — row 0's head, make_inputs' planted near match of row 1, and the head of
    every other row that queries the zero-phase relation 0 or its inverse —
    and the few entries with one dim nearly equal by chance."""
    from rnnlogic_amd import _native
    from rnnlogic_amd.embedding import RotatE
    eemb, remb, h, r = gen.make_inputs(D, E)
    h, r = h[:n], r[:n]
    gen.write_tables(str(tmp_path), eemb, remb)
    rot = RotatE(str(tmp_path)).to(dev)
    rot.mode = _native.ROTATE_MFMA
    hh, rr = torch.from_numpy(h).to(dev), torch.from_numpy(r).to(dev)
    k = gen.key(D, E, n)
    with torch.no_grad():
        got = rot(hh, rr)
        want, allow = mfma_reference(eemb, np.concatenate([remb, -remb]), gen.GAMMA, h, r, dev)
        err = (got.double() - want).abs()
        loose = allow > TOL
        zero = torch.zeros_like(err)
        plain = float(torch.where(loose, zero, err).max())
        worst = float((err / allow.clamp(min=TOL)).max())
        print("%s MFMA: max |score - f64| %.3g where the allowance is <= TOL; %d of %d entries allow more "
              "(max err there %.3g, allowance up to %.3g; largest err / allowance %.3g)"
              % (k, plain, int(loose.sum()), err.numel(), float(torch.where(loose, err, zero).max()),
                 float(allow.max()), worst))
        assert float(allow[0, h[0]]) > TOL, k  # row 0: zero phases, the head is a candidate
        assert int(loose.sum()) <= 2 * n + err.numel() // 50, k  # the planted ones and a few by chance
        assert plain <= TOL, "%s: max |score - f64| = %g" % (k, plain)
        assert bool((err <= allow.clamp(min=TOL)).all()), (k, worst)
        acc = rot.score_into(hh, rr, torch.zeros_like(got), accumulate=True)
        assert torch.equal(acc, got), (k, "accumulate=True")
    return got


@pytest.mark.parametrize("D,E,n", gen.small_cases())
def test_mfma_one_chunk(D, E, n, dev, tmp_path):
    run_mfma_case(tmp_path, dev, D, E, n)


@pytest.mark.parametrize("D", gen.BIG_D)
def test_mfma_chunk_boundary(D, dev, tmp_path):
    run_mfma_case(tmp_path / "big", dev, D, gen.BIG_E, gen.BIG_ROWS)
    run_mfma_case(tmp_path / "split", dev, D, gen.BIG_E, gen.SPLIT_ROWS)
