"""Yardsticks of the RotatE embedding trainer (rnnlogic_amd/kge.py, csrc/kge.hip).

step():              the training step as torch ops under autograd, in the
                     dtype of the tables it is given (float64: the yardstick;
                     float32: the eager composition the HIP step is compared
                     and timed against).  It takes the negatives as input.
sample_negatives():  numpy restatement of rnnl_kge_sample_negatives'
                     counter-based generator and rejection, bit for bit
                     (include/rnnlogic_hip.h documents the generator).
train_losses():      the whole recipe on the CPU from these two and torch's Adam.
write_graph():       a small dataset directory for the tests of both files.

TRAIN_LOG: the averages the trainer that made data/umls/RotatE_50 logged at
step 300 (hidden_dim 50, gamma 6, adversarial temperature 3, batch and
negative size 128, learning rate 1e-4) — recorded results, the learning
curve a restatement of the recipe has to reproduce."""
import os

import numpy as np
import torch

TRAIN_LOG = {"positive_sample_loss": 1.427432, "negative_sample_loss": 0.417243, "loss": 0.922338}
# three times the widest deviation of the total over three seeds of a CPU restatement (0.0102)
TRAIN_LOG_MARGIN = 0.03
UMLS_50 = dict(hidden_dim=50, gamma=6.0, batch_size=128, negative_sample_size=128, adversarial_temperature=3.0,
               learning_rate=1e-4, max_steps=10000)

_G = np.uint64(0x9E3779B97F4A7C15)


def _mix(z):
    z = z ^ (z >> np.uint64(30))
    z = z * np.uint64(0xBF58476D1CE4E5B9)
    z = z ^ (z >> np.uint64(27))
    z = z * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def write_graph(path, n_entities, n_relations, train, valid=(), test=()):
    """A dataset directory in the format KnowledgeGraph reads, from (h, r, t) id triples."""
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "entities.dict"), "w") as f:
        f.write("".join("%d\te%d\n" % (i, i) for i in range(n_entities)))
    with open(os.path.join(path, "relations.dict"), "w") as f:
        f.write("".join("%d\tr%d\n" % (i, i) for i in range(n_relations)))
    for name, trip in (("train", train), ("valid", valid), ("test", test)):
        with open(os.path.join(path, name + ".txt"), "w") as f:
            f.write("".join("e%d\tr%d\te%d\n" % t for t in trip))
    return path


def sample_negatives(true, positives, mode, n_entities, n_neg, seed, step):
    """(neg (B, n_neg) int32, capped): `true` is kge.true_answers' dict for
    the mode, positives (B, 3) integers."""
    positives = np.asarray(positives, dtype=np.int64).reshape(-1, 3)
    B, E = len(positives), int(n_entities)
    member = np.zeros((B, E), dtype=bool)
    for i, (h, r, t) in enumerate(positives.tolist()):
        member[i, true.get(r * E + (t if mode else h), [])] = True
    rows = np.arange(B)[:, None]
    with np.errstate(over="ignore"):
        k0 = _mix(np.asarray([seed], dtype=np.uint64) + _G * np.asarray([step + 1], dtype=np.uint64))
        k1 = _mix(k0 ^ ((rows.astype(np.uint64) << np.uint64(32)) | np.arange(n_neg, dtype=np.uint64)[None, :]))
        ent = np.zeros((B, n_neg), dtype=np.int64)
        pending = np.ones((B, n_neg), dtype=bool)
        for attempt in range(64):
            draw = _mix(k1 + _G * np.uint64(attempt + 1)) >> np.uint64(32)
            e = ((draw * np.uint64(E)) >> np.uint64(32)).astype(np.int64)
            ent = np.where(pending, e, ent)
            pending &= member[rows, ent]
            if not pending.any():
                break
    return ent.astype(np.int32), int(pending.sum())


def step(eemb, remb, gamma, positives, neg, weights, mode, alpha):
    """(pos_score (B), neg_score (B, N), (positive, negative, total) losses)
    as differentiable torch ops.  eemb (E, 2D), remb (R, D) in float64 or
    float32; the phase divisor is the fp32 one of embedding.py either way."""
    D = remb.shape[1]
    div = float(np.float32((gamma + 2.0) / D / np.pi))
    positives, neg = positives.long(), neg.long()
    h, r, t = positives[:, 0], positives[:, 1], positives[:, 2]
    anchor, answer = (t, h) if mode else (h, t)
    a = eemb.index_select(0, anchor)
    phase = remb.index_select(0, r) / div
    c, s = torch.cos(phase), torch.sin(phase)
    if mode:
        s = -s
    qre = a[:, :D] * c - a[:, D:] * s
    qim = a[:, :D] * s + a[:, D:] * c
    cand = torch.cat([neg, answer[:, None]], dim=1)
    x = eemb[cand]
    diff = torch.stack([qre[:, None] - x[..., :D], qim[:, None] - x[..., D:]], dim=0)
    score = gamma - diff.norm(dim=0).sum(dim=-1)
    sneg, spos = score[:, :-1], score[:, -1]
    p = torch.softmax(alpha * sneg, dim=1).detach()
    negl = (p * torch.nn.functional.logsigmoid(-sneg)).sum(dim=1)
    posl = torch.nn.functional.logsigmoid(spos)
    w = torch.ones_like(posl) if weights is None else weights.to(posl.dtype)
    lp = -(w * posl).sum() / w.sum()
    ln = -(w * negl).sum() / w.sum()
    return spos, sneg, (lp, ln, (lp + ln) / 2)


def train_losses(graph, steps, seed=0, **cfg):
    """(steps, 3) losses of the recipe on the CPU: kge.RotatETrainer's
    initial tables, batch order, weights and schedule, this file's sampler and
    float32 step, torch's Adam."""
    from rnnlogic_amd import kge
    tr = kge.RotatETrainer(graph, seed=seed, device="cpu", **cfg)
    true = [kge.true_answers(tr.train_triples, tr.num_entities, m) for m in kge.MODES]
    out = np.zeros((steps, 3))
    for k in range(steps):
        mode = tr.step % 2
        idx = tr._next_batch()
        positives = tr.triples.index_select(0, idx)
        weights = None if tr.uni_weight else tr.weights.index_select(0, idx)
        neg, capped = sample_negatives(true[mode], positives.numpy(), mode, tr.num_entities, tr.negative_sample_size,
                                       tr.seed, tr.step)
        assert capped == 0
        tr.eemb.grad = tr.remb.grad = None
        _, _, losses = step(tr.eemb, tr.remb, tr.gamma, positives, torch.from_numpy(neg), weights, mode, tr.alpha)
        losses[2].backward()
        tr.optimizer.step()
        tr._after_step()
        out[k] = [float(x.detach()) for x in losses]
    return out
