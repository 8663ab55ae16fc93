"""RotatE training gradients on the HIP path (rnnl_rotate_backward through
embedding._RotatEScore) against torch autograd of the reference's
arithmetic (RotatE.forward_torch, embedding.py:45-70): eemb and remb
gradients for a random upstream gradient, including a row whose target
entity equals h under a zero-phase relation (|h o r - t| = 0 in every dim:
torch.norm's zero-gradient convention).

The shipped tables are run at B = 32; the synthetic ones (the seeded tables of
tools/make_golden_rotate_loop.py) at the shapes where the backward kernel's
indexing changes: it walks the queries 32 at a time (B = 1, 31, 33, 70), owns
1,024 entities per block (E = 1, 255, 1024, 1025, 2049), runs one grid row per
dim (D = 1, 3, 32, 33), lays its scratch out differently when the entity table
is frozen, and reads the entity planes with ld = E in the MFMA mode."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, Fixture

sys.path.insert(0, os.path.join(REPO, "tools"))
import make_golden_rotate_loop as gen  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", ["umls_emb_pna_rotate", "fb_lstm_sum_rotate"])
def test_rotate_backward_matches_torch(case):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rnnlogic_amd.embedding import RotatE
    fx = Fixture(case)
    dev = torch.device("cuda:0")
    rot = RotatE(fx.rotate_path()).to(dev)
    E, R2 = rot.num_entities, rot.remb.size(0)
    gen = torch.Generator().manual_seed(0)
    B = 32
    h = torch.randint(0, E, (B,), generator=gen).to(dev)
    r = torch.randint(0, R2, (B,), generator=gen).to(dev)
    with torch.no_grad():
        rot.remb[int(r[0])].zero_()  # row 0: h o r == h, so the target h has distance 0
    g = torch.randn(B, E, generator=gen).to(dev)
    grads = []
    for fn in (rot.forward_torch, rot.forward_grad):
        rot.zero_grad()
        s = fn(h, r)
        (s * g).sum().backward()
        grads.append((s.detach().clone(), rot.eemb.grad.clone(), rot.remb.grad.clone()))
    # float64 autograd of the same arithmetic: the yardstick for both fp32 paths
    rot64 = RotatE(fx.rotate_path()).to(dev).double()
    with torch.no_grad():
        rot64.remb[int(r[0])].zero_()
    (rot64.forward_torch(h, r) * g.double()).sum().backward()
    (s0, ge0, gr0), (s1, ge1, gr1) = grads
    assert float((s0 - s1).abs().max()) <= 1e-4
    for name, a, b, w in (("eemb", ge0, ge1, rot64.eemb.grad), ("remb", gr0, gr1, rot64.remb.grad)):
        a, b, w = a.cpu().numpy(), b.cpu().numpy(), w.cpu().numpy()
        assert np.isfinite(b).all(), name
        err = float(np.abs(a - b).max())
        scale = float(np.abs(a).max())
        e_hip, e_torch = float(np.abs(b - w).max()), float(np.abs(a - w).max())
        print("%s %s grad: max |hip - torch| %.3g, |hip - f64| %.3g, |torch - f64| %.3g (max |grad| %.3g)"
              % (case, name, err, e_hip, e_torch, scale))
        # within the fp32 torch path's own distance from float64 (x 2), or the
        # tolerance of the element-wise comparison with it
        if e_hip > 2 * e_torch:
            np.testing.assert_allclose(b, a, atol=1e-5 * scale + 1e-6, rtol=1e-4, err_msg=name)


def compare_grads(what, rot, rot64, h, r, g, score_check):
    """The criterion of test_rotate_backward_matches_torch for the
    parameters that require grad."""
    grads = []
    for fn in (rot.forward_torch, rot.forward_grad):
        rot.zero_grad(set_to_none=True)
        s = fn(h, r)
        (s * g).sum().backward()
        grads.append((s.detach().clone(), rot.eemb.grad, rot.remb.grad))
    rot64.zero_grad(set_to_none=True)
    (rot64.forward_torch(h, r) * g.double()).sum().backward()
    (s0, ge0, gr0), (s1, ge1, gr1) = grads
    score_check(s0, s1)
    for name, a, b, w in (("eemb", ge0, ge1, rot64.eemb.grad), ("remb", gr0, gr1, rot64.remb.grad)):
        assert (a is None) == (b is None) == (w is None), (what, name)
        if a is None:
            continue
        a, b, w = a.cpu().numpy(), b.cpu().numpy(), w.cpu().numpy()
        assert a.shape == b.shape and np.isfinite(b).all(), (what, name)
        err = float(np.abs(a - b).max())
        scale = float(np.abs(a).max())
        e_hip, e_torch = float(np.abs(b - w).max()), float(np.abs(a - w).max())
        print("%s %s grad: max |hip - torch| %.3g, |hip - f64| %.3g, |torch - f64| %.3g (max |grad| %.3g)"
              % (what, name, err, e_hip, e_torch, scale))
        if e_hip > 2 * e_torch:
            np.testing.assert_allclose(b, a, atol=1e-5 * scale + 1e-6, rtol=1e-4, err_msg="%s %s" % (what, name))


def synthetic_batch(D, E, B):
    """make_inputs' tables with a batch of B rows: row 0 queries the
    zero-phase relation 0 (its head is a candidate at distance 0), rows 1 and
    2 repeat a head and a relation, and the last row's upstream gradient is
    zero (B > 1).  make_inputs plants one entity 1e-6 away from its own row
    1's h o r, where the gradient's direction is ill-conditioned in fp32:
    that (head, relation) pair is kept out of the batch."""
    eemb, remb, gh, gr = gen.make_inputs(D, E)
    rng = np.random.default_rng([7, D, E, B])
    h = rng.integers(0, E, B)
    r = rng.integers(0, 2 * gen.NREL, B)
    r[0] = 0
    if B >= 3:
        h[2], r[2] = h[1], r[1]
    hit = (h == gh[1]) & (r == gr[1]) if E > 1 else np.zeros(B, bool)
    r[hit] = (r[hit] + 1) % (2 * gen.NREL)
    r[0] = 0
    g = torch.randn(B, E, generator=torch.Generator().manual_seed(B * 4099 + E))
    if B > 1:
        g[B - 1] = 0.0
    return eemb, remb, h, r, g


SHAPES = [(1, 1, 1), (31, 255, 3), (33, 1024, 32), (70, 1025, 33), (1, 2049, 32), (31, 1, 33), (33, 2049, 1),
          (70, 255, 1), (70, 1024, 3), (33, 1025, 3), (31, 2049, 33), (1, 1025, 1)]  # (B, E, D)


def test_shapes_cover_every_boundary_value():
    assert {s[0] for s in SHAPES} == {1, 31, 33, 70}
    assert {s[1] for s in SHAPES} == {1, 255, 1024, 1025, 2049}
    assert {s[2] for s in SHAPES} == {1, 3, 32, 33}


@pytest.mark.parametrize("train", ["eemb", "remb", "both"])
@pytest.mark.parametrize("B,E,D", SHAPES)
def test_rotate_backward_boundary_shapes(B, E, D, train, tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rnnlogic_amd.embedding import RotatE
    dev = torch.device("cuda:0")
    eemb, remb, h, r, g = synthetic_batch(D, E, B)
    gen.write_tables(str(tmp_path), eemb, remb)
    rot, rot64 = RotatE(str(tmp_path)).to(dev), RotatE(str(tmp_path)).to(dev).double()
    for m in (rot, rot64):
        m.eemb.requires_grad_(train != "remb")
        m.remb.requires_grad_(train != "eemb")
    h, r, g = torch.from_numpy(h).to(dev), torch.from_numpy(r).to(dev), g.to(dev)
    assert int(r[0]) == 0 and float(rot.remb[0].detach().abs().max()) == 0.0

    def score_check(s0, s1):
        assert float((s0 - s1).abs().max()) <= 1e-4
        assert float(s1[0, h[0]]) == np.float32(gen.GAMMA)  # the zero-distance candidate
    compare_grads("B%d E%d D%d %s" % (B, E, D, train), rot, rot64, h, r, g, score_check)


def test_rotate_backward_mfma_mode(tmp_path):
    """mode = ROTATE_MFMA: the backward transposes eemb itself and reads the
    planes with ld = E.  The forward's scores are then the expanded MFMA
    form's: within 1e-4, or within the form's documented allowance where
    that is larger (tests/test_gpu_rotate_loop.py mfma_reference: the
    candidates at zero distance — the head of every row that queries the
    zero-phase relation 0 or its inverse)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rnnlogic_amd import _native
    from rnnlogic_amd.embedding import RotatE
    from test_gpu_rotate_loop import mfma_reference
    dev = torch.device("cuda:0")
    B, E, D = 70, 1025, 33
    eemb, remb, h, r, g = synthetic_batch(D, E, B)
    gen.write_tables(str(tmp_path), eemb, remb)
    rot, rot64 = RotatE(str(tmp_path)).to(dev), RotatE(str(tmp_path)).to(dev).double()
    rot.mode = _native.ROTATE_MFMA
    want, allow = mfma_reference(eemb, np.concatenate([remb, -remb]), gen.GAMMA, h, r, dev)
    h, r, g = torch.from_numpy(h).to(dev), torch.from_numpy(r).to(dev), g.to(dev)

    def score_check(s0, s1):
        err = (s1.double() - want).abs()
        loose = allow > 1e-4
        print("MFMA forward: max |hip - f64| %.3g where the allowance is <= 1e-4, %.3g on the %d other entries "
              "(allowance up to %.3g)" % (float(err[~loose].max()), float(err[loose].max()), int(loose.sum()),
                                          float(allow.max())))
        assert float((s0.double() - want).abs().max()) <= 1e-4  # the torch path
        assert bool(loose[0, h[0]]) and int(loose.sum()) <= 2 * B
        assert bool((err <= allow.clamp(min=1e-4)).all())
    compare_grads("MFMA B%d E%d D%d" % (B, E, D), rot, rot64, h, r, g, score_check)
