"""The fixed-point node-gradient accumulation of the three training backward
paths (csrc/grad_fix.h, used by predictor.hip, backward.hip and pna_grad.hip)
computes, bit for bit, what the commit before its consolidation computed:
every output gradient of rnnl_predictor_backward, rnnl_predictorplus_backward
and rnnl_pna_features_backward on the cases of tools/make_golden_node_grads.py
(head A's 819 trie nodes on both sides of both LDS tables; head B's stars; a
mixed-relation launch, head = -1, whose head-A gradients sit within a few
units of the fixed-point grid; a NaN) against
tests/golden/_node_grads_parent.npz, which that tool recorded on the GPU in a
checkout of the parent commit.  NaNs must sit at the same positions.

Mutation check (scratch build, not committed): with to_fix applied
per bucket entry after the multiply by the count, instead of once per
candidate, the `mixed` case fails on all three paths.
"""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO

sys.path.insert(0, os.path.join(REPO, "tools"))
import make_golden_node_grads as gen  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def world(tmp_path_factory, dev):
    return gen.World(tmp_path_factory.mktemp("node_grads"), dev)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "_node_grads_parent.npz"), allow_pickle=False)


def same(golden, key, got):
    want = golden[key]
    assert got.dtype == want.dtype and got.shape == want.shape, key
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), "%s: NaN at other positions (%d, recorded %d)" % (
        key, int(np.isnan(got).sum()), int(nan.sum()))
    diff = (got != want) & ~nan
    assert not diff.any(), "%s: %d of %d entries differ from the recorded parent output, max |diff| %.3g" % (
        key, int(diff.sum()), got.size, float(np.abs(got[diff].astype(np.float64) - want[diff]).max()))
    if "sha/" + key in golden.files:
        assert gen.sha(got) == str(golden["sha/" + key]), key


@pytest.mark.parametrize("case", list(gen.CASES))
def test_em(world, golden, case):
    h, r, etr, head, G = world.rows(case)
    same(golden, "em/" + case, gen.em_grad(world, h, r, etr, G))


@pytest.mark.parametrize("case", list(gen.CASES))
def test_sum(world, golden, case):
    h, r, etr, head, G = world.rows(case)
    got = gen.sum_grads(world, h, r, etr, head, G)
    keys = [k for k in golden.files if k.startswith("sum/%s/" % case)]
    assert sorted(keys) == sorted("sum/%s/%s" % (case, n) for n in got) and len(keys) == 10
    for n, g in got.items():
        same(golden, "sum/%s/%s" % (case, n), g)


@pytest.mark.parametrize("case", list(gen.CASES))
def test_pna(world, golden, case):
    h, r, etr, head, G = world.rows(case)
    same(golden, "pna/" + case, gen.pna_grad(world, case, h, r, etr, head))


def test_cases_reach_the_branches(world, golden):
    """What the cases are chosen for, from the recorded outputs: head A's
    gradient reaches nodes past BW_LDS_NODES = 768; the NaN case's gradients
    hold NaNs and the others none; the mixed launch's head-A gradients are
    tiny but non-zero."""
    import plus_ref as pr
    node = pr.node_of_rule(world.rules)
    in_a = np.asarray([hd == pr.REL["A"] for hd, _ in world.rules.rules])
    far = in_a & (node - node[in_a].min() >= 768)
    assert far.sum() >= 40
    for k in ("sum/A/rule_emb", "pna/A"):
        assert golden[k][far].any() and golden[k][in_a & ~far].any(), k
    for k in golden.files:
        if k.startswith(("em/", "sum/", "pna/")) and k.split("/")[1] != "nan":
            assert not np.isnan(golden[k]).any(), k
    for k in ("em/nan", "sum/nan/rule_emb", "pna/nan"):
        assert np.isnan(golden[k]).any() and not np.isnan(golden[k]).all(), k
    for k in ("sum/mixed/rule_emb", "pna/mixed"):
        a = np.abs(golden[k][in_a])
        assert a.any() and a.max() < 2.0 ** -20 * np.abs(golden[k][~in_a]).max(), k
    assert [int(golden["seed/" + c][0]) for c in gen.CASES] == [s for _, s in gen.CASES.values()]
