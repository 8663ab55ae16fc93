"""CPU tests of the RotatE embedding trainer (rnnlogic_amd/kge.py): the host
tables (subsampling weights, true-answer CSR, relation filter), the schedule,
save / load, argument validation of the new C entry points, the numpy
restatement of the negative sampler, and the torch restatement of the whole
recipe against the learning curve recorded for data/umls/RotatE_50."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import kge_ref
from kge_ref import write_graph

# (h, r, t) over 4 entities and 3 relations
TRIPLES = [(0, 0, 1), (0, 0, 2), (1, 0, 2), (2, 1, 0), (3, 1, 0), (0, 2, 3)]


@pytest.fixture()
def tiny(tmp_path):
    from rnnlogic_amd.data import KnowledgeGraph
    return KnowledgeGraph(write_graph(str(tmp_path / "g"), 4, 3, TRIPLES, [(1, 0, 3)], [(3, 2, 0)]))


def csr(lists):
    keys, offs, vals = lists.keys.numpy(), lists.offs.numpy(), lists.vals.numpy()
    assert (np.diff(keys) > 0).all() and len(offs) == len(keys) + 1
    return {int(k): vals[offs[i]:offs[i + 1]].tolist() for i, k in enumerate(keys)}


def test_weights_and_true_answers_on_a_hand_made_graph(tiny):
    from rnnlogic_amd.kge import RotatETrainer
    tr = RotatETrainer(tiny, 4, 6.0, device="cpu")
    # c(h, r): (0,0) 2, (1,0) 1, (2,1) 1, (3,1) 1, (0,2) 1;  c(r, t): (0,1) 1, (0,2) 2, (1,0) 2, (2,3) 1; each + 3
    want = [(5 + 4) ** -0.5, (5 + 5) ** -0.5, (4 + 5) ** -0.5, (4 + 5) ** -0.5, (4 + 5) ** -0.5, (4 + 4) ** -0.5]
    np.testing.assert_allclose(tr.weights_host, want, rtol=1e-7)
    assert tr.weights_host.dtype == np.float32
    E = 4
    assert csr(tr.true["tail"]) == {0 * E + 0: [1, 2], 0 * E + 1: [2], 1 * E + 2: [0], 1 * E + 3: [0], 2 * E + 0: [3]}
    assert csr(tr.true["head"]) == {0 * E + 1: [0], 0 * E + 2: [0, 1], 1 * E + 0: [2, 3], 2 * E + 3: [0]}
    assert tr.true["tail"].vals.dtype == torch.int32
    assert tuple(tr.eemb.shape) == (4, 8) and tuple(tr.remb.shape) == (3, 4)
    rho = (6.0 + 2.0) / 4
    assert float(tr.eemb.detach().abs().max()) <= rho and float(tr.remb.detach().abs().max()) <= rho


def test_num_relations_filter(tiny):
    from rnnlogic_amd.kge import RotatETrainer
    tr = RotatETrainer(tiny, 4, 6.0, num_relations=2, device="cpu")
    assert tr.train_triples.tolist() == [list(t) for t in TRIPLES if t[1] < 2]
    assert tuple(tr.remb.shape) == (2, 4) and len(tr.weights_host) == 5
    assert all(k // 4 < 2 for k in csr(tr.true["tail"]))
    assert tr._triples(tiny.test_facts).tolist() == [] and tr._triples(tiny.valid_facts).tolist() == [[1, 0, 3]]
    with pytest.raises(ValueError, match="num_relations"):
        RotatETrainer(tiny, 4, 6.0, num_relations=4, device="cpu")


def test_warm_up_schedule(tiny):
    """Steps 0 .. warm_up_steps run at the learning rate; once step
    warm_up_steps has run it drops tenfold with a fresh Adam, and again once
    step 3 warm_up_steps has run."""
    from rnnlogic_amd.kge import RotatETrainer
    tr = RotatETrainer(tiny, 4, 6.0, learning_rate=1e-3, max_steps=40, warm_up_steps=3, device="cpu")
    assert RotatETrainer(tiny, 4, 6.0, max_steps=40, device="cpu").warm_up_steps == 20
    lrs, opts = [], []
    for _ in range(12):
        lrs.append(tr.optimizer.param_groups[0]["lr"])
        opts.append(tr.optimizer)
        tr.optimizer.step()  # (zero gradients: fills Adam's state)
        assert len(tr.optimizer.state) == 2
        tr._after_step()
    np.testing.assert_allclose(lrs, [1e-3] * 4 + [1e-4] * 6 + [1e-5] * 2, rtol=1e-12)
    assert all(o is opts[0] for o in opts[:4]) and all(o is opts[4] for o in opts[4:10])
    assert opts[4] is not opts[0] and opts[10] is not opts[4] and opts[11] is opts[10]
    assert len(tr.optimizer.state) == 2 and tr.step == 12 and tr.warm_up_steps == 27
    # the reset: the optimiser of step 4 started without state
    tr2 = RotatETrainer(tiny, 4, 6.0, learning_rate=1e-3, max_steps=40, warm_up_steps=0, device="cpu")
    tr2.optimizer.step()
    tr2._after_step()
    assert len(tr2.optimizer.state) == 0 and tr2.optimizer.param_groups[0]["lr"] == pytest.approx(1e-4)


def test_save_rotate_load_round_trip(tiny, tmp_path):
    from rnnlogic_amd.embedding import RotatE
    from rnnlogic_amd.kge import RotatETrainer
    tr = RotatETrainer(tiny, 4, 6.0, batch_size=5, negative_sample_size=7, adversarial_temperature=3.0,
                       learning_rate=2e-4, seed=3, device="cpu")
    out = str(tmp_path / "RotatE_4")
    tr.save(out)
    cfg = json.load(open(os.path.join(out, "config.json")))
    shipped = json.load(open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "data", "umls", "RotatE_50",
                                          "config.json")))
    for key in ("model", "double_entity_embedding", "double_relation_embedding", "negative_sample_size", "hidden_dim",
                "gamma", "negative_adversarial_sampling", "adversarial_temperature", "batch_size", "regularization",
                "uni_weight", "learning_rate", "max_steps", "warm_up_steps", "nentity", "nrelation"):
        assert key in cfg and key in shipped, key
    assert (cfg["hidden_dim"], cfg["gamma"], cfg["nentity"], cfg["nrelation"]) == (4, 6.0, 4, 3)
    rot = RotatE(out)
    assert torch.equal(rot.eemb.detach(), tr.eemb.detach())
    assert torch.equal(rot.remb.detach(), torch.cat([tr.remb.detach(), -tr.remb.detach()]))
    assert rot.emb_dim == 4 and rot.num_entities == 4 and rot.gamma == 6.0
    back = RotatETrainer.load(tiny, out, device="cpu")
    assert torch.equal(back.eemb.detach(), tr.eemb.detach()) and torch.equal(back.remb.detach(), tr.remb.detach())
    assert (back.batch_size, back.negative_sample_size, back.alpha, back.learning_rate) == (5, 7, 3.0, 2e-4)
    assert RotatETrainer.load(tiny, out, device="cpu", batch_size=2).batch_size == 2
    mem = RotatE.from_tables(tr.eemb, tr.remb, 6.0)
    assert torch.equal(mem.eemb.detach(), rot.eemb.detach()) and torch.equal(mem.remb.detach(), rot.remb.detach())


def test_regularization_is_rejected(tiny):
    from rnnlogic_amd.kge import RotatETrainer
    with pytest.raises(ValueError, match="regularization"):
        RotatETrainer(tiny, 4, 6.0, regularization=1e-9, device="cpu")
    RotatETrainer(tiny, 4, 6.0, regularization=0.0, device="cpu")


def test_seed_range_is_checked(tiny):
    from rnnlogic_amd.kge import RotatETrainer
    for bad in (-1, 1 << 63):
        with pytest.raises(ValueError, match="seed"):
            RotatETrainer(tiny, 4, 6.0, seed=bad, device="cpu")
    RotatETrainer(tiny, 4, 6.0, seed=(1 << 63) - 2, device="cpu")


def test_train_step_needs_gpu(tiny):
    from rnnlogic_amd.kge import RotatETrainer
    with pytest.raises(RuntimeError, match="HIP path"):
        RotatETrainer(tiny, 4, 6.0, device="cpu").train_step()


def test_kge_entry_points_validate_without_gpu():
    from rnnlogic_amd import _native
    L = _native.lib()
    INV = _native.RNNL_ERR_INVALID
    p = ctypes.c_void_p(256)  # never dereferenced: validation comes first
    nb = ctypes.c_size_t()

    def sample(keys=p, positives=p, rows=4, mode=0, E=5, N=3, step=0, neg=p, capped=p, n_keys=2):
        return L.rnnl_kge_sample_negatives(keys, p, p, n_keys, positives, rows, mode, E, N, 1, step, neg, capped, None)
    for kw in (dict(positives=None), dict(neg=None), dict(capped=None), dict(rows=0), dict(E=0), dict(N=0),
               dict(mode=2), dict(step=-1), dict(keys=None), dict(n_keys=-1)):
        assert sample(**kw) == INV, kw
        assert b"rnnl_kge_sample_negatives" in L.rnnl_last_error()

    assert L.rnnl_kge_rotate_step_scratch(4, 3, 5, 2, ctypes.byref(nb)) == 0 and nb.value > 0
    small = nb.value
    assert L.rnnl_kge_rotate_step_scratch(400, 3, 5, 2, ctypes.byref(nb)) == 0 and nb.value > small
    for args in ((0, 3, 5, 2), (4, 0, 5, 2), (4, 3, 0, 2), (4, 3, 5, 0), (4, 3, 5, 4080), (1 << 24, 127, 5, 2)):
        assert L.rnnl_kge_rotate_step_scratch(*args, ctypes.byref(nb)) == INV, args
    assert L.rnnl_kge_rotate_step_scratch(4, 3, 5, 4079, ctypes.byref(nb)) == 0
    assert L.rnnl_kge_rotate_step_scratch(4, 3, 5, 2, None) == INV

    def step(eemb=p, remb=p, E=5, R=2, D=2, pos=p, neg=p, rows=4, N=3, mode=1, alpha=1.0, scratch=p, nbytes=1 << 30,
             ps=p, ns=p, losses=p, de=p, dr=p):
        return L.rnnl_kge_rotate_step(eemb, remb, E, R, D, 6.0, pos, neg, None, rows, N, mode, alpha, scratch, nbytes,
                                      ps, ns, losses, de, dr, None)
    for kw in (dict(eemb=None), dict(remb=None), dict(pos=None), dict(neg=None), dict(scratch=None), dict(ps=None),
               dict(ns=None), dict(losses=None), dict(de=None), dict(dr=None), dict(E=0), dict(R=0), dict(D=0),
               dict(rows=0), dict(N=0), dict(mode=-1), dict(alpha=-1.0), dict(alpha=float("nan")), dict(nbytes=16)):
        assert step(**kw) == INV, kw
        assert b"rnnl_kge_rotate_step" in L.rnnl_last_error()


# ------------------------------------------------------------------ sampler
def test_sampler_restatement_never_draws_a_true_answer():
    from rnnlogic_amd import datasets, kge
    from rnnlogic_amd.data import KnowledgeGraph
    g = KnowledgeGraph(datasets.materialize("umls"))
    tr = kge.RotatETrainer(g, 4, 6.0, device="cpu")
    pos = tr.train_triples[::7]
    for mode, name in enumerate(kge.MODES):
        true = kge.true_answers(tr.train_triples, tr.num_entities, name)
        neg, capped = kge_ref.sample_negatives(true, pos, mode, tr.num_entities, 33, 5, 11)
        assert capped == 0 and neg.dtype == np.int32 and neg.shape == (len(pos), 33)
        assert neg.min() >= 0 and neg.max() < tr.num_entities
        for i, (h, r, t) in enumerate(pos.tolist()):
            listed = true[r * tr.num_entities + (t if mode else h)]
            assert (t if mode == 0 else h) in listed
            assert not set(neg[i].tolist()) & set(listed)
        again, _ = kge_ref.sample_negatives(true, pos, mode, tr.num_entities, 33, 5, 11)
        other, _ = kge_ref.sample_negatives(true, pos, mode, tr.num_entities, 33, 5, 12)
        assert np.array_equal(neg, again) and not np.array_equal(neg, other)
        # a slot's draw depends on (seed, step, row, slot) alone, not on the call's shape
        wide, _ = kge_ref.sample_negatives(true, pos[:9], mode, tr.num_entities, 40, 5, 11)
        assert np.array_equal(wide[:, :33], neg[:9])


def test_sampler_restatement_is_uniform_over_the_eligible_entities():
    """kinship's first batch, 200 steps of 128 slots pooled per row: every
    eligible entity is drawn at a rate within 6 binomial sigma of 1 / m_i."""
    from rnnlogic_amd import datasets, kge
    from rnnlogic_amd.data import KnowledgeGraph
    g = KnowledgeGraph(datasets.materialize("kinship"))
    tr = kge.RotatETrainer(g, 4, 6.0, batch_size=128, negative_sample_size=128, device="cpu")
    pos = tr.train_triples[tr._next_batch().numpy()]
    E, steps, N = tr.num_entities, 200, 128
    for mode, name in enumerate(kge.MODES):
        true = kge.true_answers(tr.train_triples, E, name)
        counts = np.zeros((len(pos), E), dtype=np.int64)
        for step in range(steps):
            neg, capped = kge_ref.sample_negatives(true, pos, mode, E, N, 0, step)
            assert capped == 0
            for i in range(len(pos)):
                counts[i] += np.bincount(neg[i], minlength=E)
        n = steps * N
        worst = 0.0
        for i, (h, r, t) in enumerate(pos.tolist()):
            listed = true[r * E + (t if mode else h)]
            elig = np.setdiff1d(np.arange(E), listed)
            assert counts[i, listed].sum() == 0 and counts[i].sum() == n
            p = 1.0 / len(elig)
            z = np.abs(counts[i, elig] - n * p) / np.sqrt(n * p * (1 - p))
            worst = max(worst, float(z.max()))
        print("%s mode: largest deviation %.2f binomial sigma" % (name, worst))
        assert worst <= 6.0


@pytest.mark.slow
def test_restatement_reproduces_the_recorded_learning_curve():
    """The recipe (kge_ref.train_losses: the float32 torch step, the numpy
    sampler, Adam) on UMLS with the shipped RotatE_50 configuration, seed 0:
    the mean total loss over steps 201-300 is within 0.03 of the 0.922338
    its train.log records at step 300."""
    from rnnlogic_amd import datasets
    from rnnlogic_amd.data import KnowledgeGraph
    g = KnowledgeGraph(datasets.materialize("umls"))
    losses = kge_ref.train_losses(g, 301, seed=0, **kge_ref.UMLS_50)
    pos, neg, total = losses[201:301].mean(axis=0)
    print("steps 201-300: positive %.6f (log %.6f), negative %.6f (log %.6f), total %.6f (log %.6f)"
          % (pos, kge_ref.TRAIN_LOG["positive_sample_loss"], neg, kge_ref.TRAIN_LOG["negative_sample_loss"], total,
             kge_ref.TRAIN_LOG["loss"]))
    assert abs(total - kge_ref.TRAIN_LOG["loss"]) <= kge_ref.TRAIN_LOG_MARGIN
