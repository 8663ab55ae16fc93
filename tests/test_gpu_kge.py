"""The RotatE embedding trainer on the GPU (rnnlogic_amd/kge.py, csrc/kge.hip):
the negative sampler bit for bit against its numpy restatement, the training
step (scores, losses, both gradients) against float64 autograd of the torch
restatement (tests/kge_ref.py), bitwise repeatability, the recorded learning
curve of data/umls/RotatE_50, and the filtered evaluation against the MRR the
shipped tables' train.log records.

The step's shapes sit where its indexing changes: the workgroup has 64, 128 or
256 threads for D <= 64, <= 128 and above (D = 64, 65, 128, 129), 64 lanes or
all threads stride over d (D = 1, 3, 33, 50, 1000), the waves of a workgroup
share the N + 1 slots (N = 1 with four waves, N = 257), sweep 2 takes its slots
four at a time (N + 1 = 2, 4, 6, 8, 129, 131, 258), the entity pass decodes its
list into LDS 256 items at a time and keeps eight rows in flight (entity 0, in
slot 0 of every row, has a list of 256, 257, about 330 and about 515 items, so
of one tile exactly, one item more, two tiles and three; the other lists run
from empty to about 270; it sorts a list in LDS up to 4,096 items and in
global memory beyond: entity 0 of the (3000, 1, 2, 2) shape has about 6,000),
and the relation pass compacts its relation's rows
over the waves of a 128- or 256-thread block (B = 140 at D = 100, B = 257 at
D = 129: more rows than the block has threads)."""
import json
import os

import numpy as np
import pytest
import torch

import kge_ref
from kge_ref import write_graph

pytestmark = pytest.mark.gpu

GAMMA = 6.0
NREL = 5
# (B, N, E, D)
SHAPES = [(1, 1, 2, 1), (5, 7, 135, 3), (5, 128, 135, 50), (130, 7, 135, 64), (5, 257, 3000, 65),
          (130, 128, 3000, 33), (3, 130, 500, 1000), (4, 3, 40, 128), (2, 5, 40, 129), (3, 1, 9, 300),
          (300, 3, 40, 8), (257, 2, 3, 129), (140, 2, 7, 100), (255, 1, 5000, 2), (256, 1, 5000, 2),
          (3000, 1, 2, 2)]
LIST_TILE, LIST_BATCH = 256, 8  # kge_entity_kernel: items decoded into LDS at a time / rows in flight
SORT_LDS = 4096  # ... and the longest list it sorts in LDS (longer ones in place in global memory)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def umls():
    from rnnlogic_amd import datasets
    from rnnlogic_amd.data import KnowledgeGraph
    return KnowledgeGraph(datasets.materialize("umls"))


def test_shapes_cover_every_boundary_value():
    assert {s[3] for s in SHAPES} >= {1, 3, 33, 50, 64, 65, 128, 129, 1000}
    assert {(s[1] + 1) % 4 for s in SHAPES} == {0, 1, 2, 3}
    assert {s[1] for s in SHAPES} >= {1, 7, 128, 257}
    assert {s[0] for s in SHAPES} >= {1, 5, 130} and {s[2] for s in SHAPES} >= {2, 135, 3000}
    assert any(s[1] == 1 and s[3] > 128 for s in SHAPES)  # fewer slots than waves
    # the relation pass: more rows than a 128-thread and than a 256-thread block has threads
    assert any(s[0] > 128 and 64 < s[3] <= 128 for s in SHAPES) and any(s[0] > 256 and s[3] > 128 for s in SHAPES)
    # the entity pass: the longest list (entity 0's) at, just past and well past a tile, in both modes
    longest = {mode: {int(list_lengths(*s, mode).max()) for s in SHAPES} for mode in (0, 1)}
    every = np.concatenate([list_lengths(*s, mode) for s in SHAPES for mode in (0, 1)])
    for mode in (0, 1):
        assert {LIST_TILE, LIST_TILE + 1} <= longest[mode]
        assert any(LIST_TILE + 1 < n <= 2 * LIST_TILE for n in longest[mode]), longest[mode]
        assert any(2 * LIST_TILE < n <= SORT_LDS for n in longest[mode]), longest[mode]
        assert any(n > SORT_LDS for n in longest[mode]), longest[mode]
    assert (every == 0).any() and {int(n) % LIST_BATCH for n in every} == set(range(LIST_BATCH))


# ------------------------------------------------------------------ sampler
@pytest.mark.parametrize("B,N", [(1, 1), (5, 7), (130, 257)])
def test_sampler_is_bit_equal_to_the_restatement(B, N, umls, dev):
    from rnnlogic_amd import kge
    tr = kge.RotatETrainer(umls, 4, GAMMA, seed=7, device=dev)
    pos = tr.train_triples[np.random.default_rng(B).integers(0, len(tr.train_triples), B)]
    for mode, name in enumerate(kge.MODES):
        true = kge.true_answers(tr.train_triples, tr.num_entities, name)
        for step in (0, 12345):
            got = tr.sample_negatives(torch.from_numpy(pos).to(dev), mode, step, N)
            want, capped = kge_ref.sample_negatives(true, pos, mode, tr.num_entities, N, 7, step)
            assert capped == 0 and int(tr.capped.item()) == 0
            assert got.dtype == torch.int32 and tuple(got.shape) == (B, N)
            np.testing.assert_array_equal(got.cpu().numpy(), want)


def test_sampler_on_a_two_entity_graph(dev, tmp_path):
    """Each row has exactly one eligible entity: every slot holds it."""
    from rnnlogic_amd import kge
    from rnnlogic_amd.data import KnowledgeGraph
    g = KnowledgeGraph(write_graph(str(tmp_path / "two"), 2, 2, [(0, 0, 1), (1, 1, 0)]))
    tr = kge.RotatETrainer(g, 2, GAMMA, device=dev)
    pos = torch.from_numpy(tr.train_triples).to(dev)
    for mode in (0, 1):
        neg = tr.sample_negatives(pos, mode, 3, 50).cpu().numpy()
        assert int(tr.capped.item()) == 0
        eligible = tr.train_triples[:, 0 if mode == 0 else 2]  # the row's own anchor is the only non-answer
        assert (neg == eligible[:, None]).all()
        want, _ = kge_ref.sample_negatives(kge.true_answers(tr.train_triples, 2, kge.MODES[mode]), tr.train_triples,
                                           mode, 2, 50, 0, 3)
        np.testing.assert_array_equal(neg, want)


# --------------------------------------------------------------------- step
def make_batch(B, N, E, D, mode, weighted):
    """Seeded tables and a batch with, planted: relation 0 at zero phase and
    row 0 on it with anchor entity 0; entity 0 in slot 0 of every row (for row
    0 that negative is its anchor: s = gamma exactly, no gradient there);
    rows 1 and 2 sharing (h, r); a negative repeated within a row; the anchor
    of row 1 among the negatives of row 0."""
    rng = np.random.default_rng([B, N, E, D, mode])
    rho = (GAMMA + 2.0) / D
    eemb = rng.uniform(-rho, rho, (E, 2 * D)).astype(np.float32)
    remb = rng.uniform(-rho, rho, (NREL, D)).astype(np.float32)
    remb[0] = 0.0
    pos = np.stack([rng.integers(0, E, B), rng.integers(0, NREL, B), rng.integers(0, E, B)], axis=1)
    a_col, p_col = (2, 0) if mode else (0, 2)
    pos[0, a_col], pos[0, 1], pos[0, p_col] = 0, 0, E - 1
    if B >= 3:
        pos[2, 0], pos[2, 1] = pos[1, 0], pos[1, 1]
    neg = rng.integers(0, E, (B, N)).astype(np.int32)
    neg[:, 0] = 0
    if N >= 3:
        neg[:, N - 1] = neg[:, N - 2]
    if B >= 2 and N >= 2:
        neg[0, 1] = pos[1, a_col]
    w = rng.uniform(0.1, 1.0, B).astype(np.float32) if weighted else None
    return eemb, remb, pos.astype(np.int64), neg, w


def list_lengths(B, N, E, D, mode):
    """Items per entity of the batch: its negative slots, answers and anchors."""
    _, _, pos, neg, _ = make_batch(B, N, E, D, mode, False)
    return (np.bincount(neg.reshape(-1), minlength=E) + np.bincount(pos[:, 0], minlength=E)
            + np.bincount(pos[:, 2], minlength=E))


def reference(B, N, E, D, mode, alpha, weighted, dev):
    """float64 and float32 autograd of kge_ref.step for the batch."""
    eemb, remb, pos, neg, w = make_batch(B, N, E, D, mode, weighted)
    out = []
    for dt in (torch.float64, torch.float32):
        e = torch.from_numpy(eemb).to(dev, dt).requires_grad_(True)
        r = torch.from_numpy(remb).to(dev, dt).requires_grad_(True)
        sp, sn, losses = kge_ref.step(e, r, GAMMA, torch.from_numpy(pos).to(dev), torch.from_numpy(neg).to(dev),
                                      None if w is None else torch.from_numpy(w).to(dev), mode, alpha)
        losses[2].backward()
        out.append(dict(sp=sp.detach().cpu().numpy(), sn=sn.detach().cpu().numpy(),
                        losses=np.asarray([float(x.detach()) for x in losses]), de=e.grad.cpu().numpy(),
                        dr=r.grad.cpu().numpy()))
    return out


def run_hip(B, N, E, D, mode, alpha, weighted, dev):
    from rnnlogic_amd import kge
    eemb, remb, pos, neg, w = make_batch(B, N, E, D, mode, weighted)
    t = lambda x: None if x is None else torch.from_numpy(x).to(dev)  # noqa: E731
    out = kge.rotate_step(t(eemb), t(remb), GAMMA, t(pos), t(neg), t(w), mode, alpha)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in out], (eemb, remb, pos, neg, w)


@pytest.mark.parametrize("weighted", [True, False], ids=["w", "uni"])
@pytest.mark.parametrize("alpha", [0.0, 3.0, 50.0])
@pytest.mark.parametrize("mode", [0, 1], ids=["tail", "head"])
@pytest.mark.parametrize("B,N,E,D", SHAPES)
def test_step_matches_float64(B, N, E, D, mode, alpha, weighted, dev):
    (sp, sn, losses, de, dr), (eemb, remb, pos, neg, w) = run_hip(B, N, E, D, mode, alpha, weighted, dev)
    f64, f32 = reference(B, N, E, D, mode, alpha, weighted, dev)
    what = "B%d N%d E%d D%d %s a%g %s" % (B, N, E, D, "head" if mode else "tail", alpha, "w" if weighted else "uni")
    e_s = max(float(np.abs(sp - f64["sp"]).max()), float(np.abs(sn - f64["sn"]).max()))
    e_l = float(np.abs(losses - f64["losses"]).max())
    print("%s: max |score - f64| %.3g, max |loss - f64| %.3g (torch fp32: %.3g, %.3g)"
          % (what, e_s, e_l, max(float(np.abs(f32["sp"] - f64["sp"]).max()), float(np.abs(f32["sn"] - f64["sn"]).max())),
             float(np.abs(f32["losses"] - f64["losses"]).max())))
    assert e_s <= 1e-4
    assert sn[0, 0] == np.float32(GAMMA)  # row 0's negative at its own query: distance 0
    assert e_l <= 2e-4
    touched = np.zeros(E, bool)
    touched[neg.reshape(-1)] = True
    touched[pos[:, 0]] = touched[pos[:, 2]] = True
    assert not de[~touched].any(), "rows of untouched entities must be exactly 0"
    assert not dr[np.setdiff1d(np.arange(NREL), pos[:, 1])].any()
    for name, b, a, ref in (("d_eemb", de, f32["de"], f64["de"]), ("d_remb", dr, f32["dr"], f64["dr"])):
        assert b.shape == a.shape and np.isfinite(b).all(), (what, name)
        scale = float(np.abs(a).max())
        e_hip, e_torch = float(np.abs(b - ref).max()), float(np.abs(a - ref).max())
        print("%s %s: max |hip - torch| %.3g, |hip - f64| %.3g, |torch - f64| %.3g (max |grad| %.3g)"
              % (what, name, float(np.abs(a - b).max()), e_hip, e_torch, scale))
        # within the fp32 torch path's own distance from float64 (x 2), or the
        # tolerance of the element-wise comparison with it (tests/test_gpu_rotate_grad.py)
        if e_hip > 2 * e_torch:
            np.testing.assert_allclose(b, a, atol=1e-5 * scale + 1e-6, rtol=1e-4, err_msg="%s %s" % (what, name))


@pytest.mark.parametrize("B,N,E,D", [(130, 128, 3000, 33), (3, 130, 500, 1000), (130, 7, 135, 64), (257, 2, 3, 129),
                                     (3000, 1, 2, 2)])
def test_step_is_bitwise_repeatable(B, N, E, D, dev):
    for mode in (0, 1):
        first, _ = run_hip(B, N, E, D, mode, 3.0, True, dev)
        second, _ = run_hip(B, N, E, D, mode, 3.0, True, dev)
        for a, b in zip(first, second):
            assert a.tobytes() == b.tobytes()


def test_user_negatives_are_range_checked(umls, dev):
    from rnnlogic_amd import kge
    tr = kge.RotatETrainer(umls, 8, GAMMA, batch_size=4, negative_sample_size=3, device=dev)
    for bad in (torch.full((4, 3), tr.num_entities), torch.full((4, 3), -1), torch.zeros((3, 3), dtype=torch.int64)):
        with pytest.raises(ValueError):
            tr.train_step(neg=bad)
    assert tr.step == 0
    out = tr.train_step(neg=torch.zeros((4, 5), dtype=torch.int64))
    assert out.is_cuda and tuple(out.shape) == (3,) and bool(torch.isfinite(out).all()) and tr.step == 1


def test_training_is_bitwise_repeatable(umls, dev):
    from rnnlogic_amd import kge
    tables = []
    for _ in range(2):
        tr = kge.RotatETrainer(umls, 50, GAMMA, adversarial_temperature=3.0, seed=4, device=dev)
        losses = [tr.train_step() for _ in range(20)]
        tables.append((tr.eemb.detach().cpu().numpy().tobytes(), tr.remb.detach().cpu().numpy().tobytes(),
                       torch.stack(losses).cpu().numpy().tobytes()))
        assert int(tr.capped.item()) == 0 and tr.step == 20
    assert tables[0] == tables[1]


def test_learning_curve_of_the_shipped_umls_config(umls, dev):
    """301 steps of the RotatE_50 configuration: the mean total loss over
    steps 201-300 is within 0.03 of the 0.922338 its train.log records."""
    from rnnlogic_amd import kge
    tr = kge.RotatETrainer(umls, seed=0, device=dev, **kge_ref.UMLS_50)
    losses = torch.stack([tr.train_step() for _ in range(301)]).double().cpu().numpy()
    pos, neg, total = losses[201:301].mean(axis=0)
    print("steps 201-300: positive %.6f (log %.6f), negative %.6f (log %.6f), total %.6f (log %.6f)"
          % (pos, kge_ref.TRAIN_LOG["positive_sample_loss"], neg, kge_ref.TRAIN_LOG["negative_sample_loss"], total,
             kge_ref.TRAIN_LOG["loss"]))
    assert abs(total - kge_ref.TRAIN_LOG["loss"]) <= kge_ref.TRAIN_LOG_MARGIN


# ----------------------------------------------------------------- evaluate
@pytest.mark.parametrize("data,dim,mrr", [("umls", 200, 0.659847), ("kinship", 1000, 0.637454)])
def test_evaluate_reproduces_the_recorded_test_mrr(data, dim, mrr, dev):
    from rnnlogic_amd import datasets, kge
    from rnnlogic_amd.data import KnowledgeGraph
    g = KnowledgeGraph(datasets.materialize(data))
    tr = kge.RotatETrainer.load(g, datasets.rotate_path(data, dim), device=dev)
    m = tr.evaluate("test")
    print(data, dim, m)
    assert abs(m["MRR"] - mrr) < 5e-7, (m["MRR"], mrr)
    assert 1.0 <= m["MR"] <= g.entity_size and 0.0 <= m["HITS@1"] <= m["HITS@3"] <= m["HITS@10"] <= 1.0


def test_saved_tables_feed_predictorplus(umls, dev, tmp_path):
    from rnnlogic_amd import datasets, kge
    from rnnlogic_amd.predictors import PredictorPlus
    tr = kge.RotatETrainer(umls, 16, GAMMA, batch_size=32, negative_sample_size=16, device=dev)
    for _ in range(4):
        tr.train_step()
    out = str(tmp_path / "RotatE_16")
    tr.save(out)
    assert sorted(os.listdir(out)) == ["config.json", "entity_embedding.npy", "relation_embedding.npy"]
    model = PredictorPlus(umls, type="emb", entity_feature="RotatE", aggregator="sum", embedding_path=out)
    model.set_rules(datasets.rule_file("umls"))
    model = model.to(dev).eval()
    facts = [f for f in umls.test_facts if f[1] == umls.test_facts[0][1]][:16]
    h = torch.tensor([f[0] for f in facts], device=dev)
    r = torch.tensor([f[1] for f in facts], device=dev)
    with torch.no_grad():
        score, mask = model(h, r, None)
    assert tuple(score.shape) == (len(facts), umls.entity_size) and bool(torch.isfinite(score).all())


def test_command_line_trains_evaluates_and_saves(dev, tmp_path, capsys):
    from rnnlogic_amd import datasets, kge
    from rnnlogic_amd.embedding import RotatE
    out = str(tmp_path / "RotatE_8")
    kge.main(["--data_path", datasets.materialize("umls"), "--save_path", out, "--hidden_dim", "8", "--gamma", "6",
              "--adversarial_temperature", "3", "--batch_size", "64", "--negative_sample_size", "16", "--max_steps", "6",
              "--log_steps", "3", "--seed", "2"])
    text = capsys.readouterr().out
    for line in ("Training average positive_sample_loss at step 3:", "Training average negative_sample_loss at step 6:",
                 "Training average loss at step 6:", "Valid MRR at step 5:", "Test MRR at step 5:", "Test MR at step 5:",
                 "Test HITS@1 at step 5:", "Test HITS@3 at step 5:", "Test HITS@10 at step 5:"):
        assert line in text, line
    rot = RotatE(out)
    assert tuple(rot.eemb.shape) == (135, 16) and tuple(rot.remb.shape) == (92, 8)
    with pytest.raises(ValueError, match="regularization"):
        kge.main(["--data_path", datasets.materialize("umls"), "--save_path", out, "--regularization", "0.1"])
    # --init_checkpoint: the tables, hidden_dim, gamma and the recipe flags that are not given come from it
    more = str(tmp_path / "RotatE_8_more")
    kge.main(["--data_path", datasets.materialize("umls"), "--save_path", more, "--init_checkpoint", out,
              "--max_steps", "2", "--negative_sample_size", "5"])
    cfg = json.load(open(os.path.join(more, "config.json")))
    assert (cfg["hidden_dim"], cfg["gamma"], cfg["batch_size"], cfg["negative_sample_size"], cfg["max_steps"],
            cfg["adversarial_temperature"], cfg["seed"]) == (8, 6.0, 64, 5, 2, 3.0, 0)
    assert "Training average loss at step 2:" in capsys.readouterr().out
    assert not torch.equal(RotatE(more).eemb, rot.eemb)
    with pytest.raises(ValueError, match="hidden_dim"):
        kge.main(["--data_path", datasets.materialize("umls"), "--save_path", more, "--init_checkpoint", out,
                  "--hidden_dim", "16", "--max_steps", "1"])
