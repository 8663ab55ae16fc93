"""RotatE entity-embedding training on the GPU: makes the tables that
`embedding.RotatE` loads (config.json, entity_embedding.npy,
relation_embedding.npy) from a graph's train triples.

The recipe is the one recorded in the shipped RotatE_<dim>/config.json files:
self-adversarial sampled negatives, the frequency subsampling weights, Adam
with one learning-rate drop.  The sampler and the step (scores, losses and
both gradients) are HIP kernels (csrc/kge.hip: rnnl_kge_sample_negatives,
rnnl_kge_rotate_step); Adam is torch's, over the dense tables.

    python -m rnnlogic_amd.kge --data_path data/umls --save_path out/RotatE_50 \\
        --hidden_dim 50 --gamma 6 --adversarial_temperature 3
"""
import argparse
import ctypes
import json
import os

import numpy as np
import torch

from . import _native
from .data import KnowledgeGraph, _DeviceLists
from .embedding import RotatE

MODES = ("tail", "head")


def true_answers(triples, n_entities, mode):
    """{key: ascending true answers without repeats} of (n, 3) triples: key
    r |E| + h -> tails (mode 'tail'), r |E| + t -> heads (mode 'head')."""
    a, b = (0, 2) if mode == "tail" else (2, 0)
    out = {}
    for row in triples.tolist():
        out.setdefault(row[1] * n_entities + row[a], set()).add(row[b])
    return {k: sorted(v) for k, v in out.items()}


def subsampling_weights(triples):
    """w = (c(h, r) + c(t, -r-1)) ** -0.5 per triple, c = 3 + the number of
    train triples with that (h, r) / that (r, t)."""
    hr, rt = {}, {}
    for h, r, t in triples.tolist():
        hr[(h, r)] = hr.get((h, r), 3) + 1
        rt[(r, t)] = rt.get((r, t), 3) + 1
    w = [1.0 / np.sqrt(hr[(h, r)] + rt[(r, t)]) for h, r, t in triples.tolist()]
    return np.asarray(w, dtype=np.float32)


def sample_negatives(lists, positives, mode, n_entities, n_neg, seed, step, capped=None):
    """rnnl_kge_sample_negatives: (B, n_neg) int32 negatives of the (B, 3)
    int64 device positives, none of them in the rows' lists (`lists`: a
    data._DeviceLists of true_answers).  capped: a 1-element int32 device
    tensor that receives the number of slots whose 64 draws were all rejected."""
    dev = positives.device
    if dev.type != "cuda":
        raise RuntimeError("the negative sampler runs on the HIP path; move the positives to a GPU")
    if not 0 <= int(seed) < 1 << 64:
        raise ValueError("seed must be in [0, 2^64), got %r" % (seed,))
    if capped is None:
        capped = torch.empty(1, dtype=torch.int32, device=dev)
    neg = torch.empty((positives.size(0), n_neg), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _native.call("rnnl_kge_sample_negatives", lists.keys.data_ptr(), lists.offs.data_ptr(),
                     lists.vals.data_ptr(), lists.keys.numel(), positives.data_ptr(), positives.size(0), int(mode),
                     int(n_entities), int(n_neg), int(seed), int(step), neg.data_ptr(), capped.data_ptr(),
                     torch.cuda.current_stream(dev).cuda_stream)
    return neg


def step_scratch(n_rows, n_neg, n_entities, dim, device):
    nb = ctypes.c_size_t()
    _native.call("rnnl_kge_rotate_step_scratch", n_rows, n_neg, n_entities, dim, ctypes.byref(nb))
    return torch.empty(nb.value, dtype=torch.uint8, device=device)


def rotate_step(eemb, remb, gamma, positives, neg, weights, mode, alpha, scratch=None, d_eemb=None, d_remb=None):
    """rnnl_kge_rotate_step on contiguous device tensors: eemb (E, 2D) and remb
    (R, D) fp32, positives (B, 3) int64, neg (B, N) int32, weights (B) fp32 or
    None.  Returns pos_score (B), neg_score (B, N), losses (3: positive,
    negative, total), d_eemb and d_remb (written whole)."""
    dev = eemb.device
    if dev.type != "cuda":
        raise RuntimeError("the RotatE training step runs on the HIP path; move the tables to a GPU")
    (B, N), (E, D2), (R, D) = neg.shape, eemb.shape, remb.shape
    if D2 != 2 * D or tuple(positives.shape) != (B, 3) or (weights is not None and tuple(weights.shape) != (B,)):
        raise ValueError("rotate_step: shapes do not fit")
    for x, dt in ((eemb, torch.float32), (remb, torch.float32), (positives, torch.int64), (neg, torch.int32)) + \
            (((weights, torch.float32),) if weights is not None else ()):
        if x.dtype != dt or not x.is_contiguous() or x.device != dev:
            raise ValueError("rotate_step: tensors must be contiguous, on one device, fp32 / int64 / int32")
    if scratch is None:
        scratch = step_scratch(B, N, E, D, dev)
    pos_score = torch.empty(B, dtype=torch.float32, device=dev)
    neg_score = torch.empty((B, N), dtype=torch.float32, device=dev)
    losses = torch.empty(3, dtype=torch.float32, device=dev)
    d_eemb = torch.empty((E, D2), dtype=torch.float32, device=dev) if d_eemb is None else d_eemb
    d_remb = torch.empty((R, D), dtype=torch.float32, device=dev) if d_remb is None else d_remb
    with torch.cuda.device(dev):
        _native.call("rnnl_kge_rotate_step", eemb.data_ptr(), remb.data_ptr(), E, R, D, float(gamma),
                     positives.data_ptr(), neg.data_ptr(), None if weights is None else weights.data_ptr(), B, N,
                     int(mode), float(alpha), scratch.data_ptr(), scratch.numel(), pos_score.data_ptr(),
                     neg_score.data_ptr(), losses.data_ptr(), d_eemb.data_ptr(), d_remb.data_ptr(),
                     torch.cuda.current_stream(dev).cuda_stream)
    return pos_score, neg_score, losses, d_eemb, d_remb


class RotatETrainer(object):
    def __init__(self, graph, hidden_dim, gamma, batch_size=128, negative_sample_size=128,
                 negative_adversarial_sampling=True, adversarial_temperature=1.0, uni_weight=False,
                 learning_rate=1e-4, max_steps=10000, warm_up_steps=None, num_relations=None, seed=0,
                 device=None, regularization=0.0, _tables=None):
        if regularization != 0:
            raise ValueError("regularization = %r is not supported: the RotatE recipe of the shipped tables has "
                             "regularization 0.0 and the training step has no regulariser" % (regularization,))
        if hidden_dim < 1 or batch_size < 1 or negative_sample_size < 1:
            raise ValueError("hidden_dim, batch_size and negative_sample_size must be positive")
        self.graph = graph
        self.device = torch.device(device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
        self.hidden_dim, self.gamma = int(hidden_dim), float(gamma)
        self.batch_size, self.negative_sample_size = int(batch_size), int(negative_sample_size)
        self.negative_adversarial_sampling = bool(negative_adversarial_sampling)
        self.adversarial_temperature = float(adversarial_temperature)
        self.alpha = self.adversarial_temperature if self.negative_adversarial_sampling else 0.0
        self.uni_weight = bool(uni_weight)
        self.learning_rate, self.max_steps = float(learning_rate), int(max_steps)
        self._warm_up_arg = None if warm_up_steps is None else int(warm_up_steps)  # as given: what config() records
        self.warm_up_steps = int(warm_up_steps) if warm_up_steps is not None else self.max_steps // 2
        self.num_entities = graph.entity_size
        self.num_relations = int(num_relations) if num_relations is not None else graph.relation_size
        if not 1 <= self.num_relations <= graph.relation_size:
            raise ValueError("num_relations must be in [1, %d]" % graph.relation_size)
        self.seed = int(seed)
        if not 0 <= self.seed < (1 << 63) - 1:  # the sampler's key, and torch generators seeded seed and seed + 1
            raise ValueError("seed must be in [0, 2^63 - 1), got %r" % (seed,))

        E, R, D = self.num_entities, self.num_relations, self.hidden_dim
        self.train_triples = self._triples(graph.train_facts)
        if len(self.train_triples) == 0:
            raise ValueError("no train triple has a relation below num_relations = %d" % R)
        self.weights_host = subsampling_weights(self.train_triples)
        dev = self.device
        self.triples = torch.from_numpy(self.train_triples).to(dev)
        self.weights = torch.from_numpy(self.weights_host).to(dev)
        self.true = {m: _DeviceLists(true_answers(self.train_triples, E, m), dev) for m in MODES}

        rho = (self.gamma + 2.0) / D
        if _tables is None:
            gen = torch.Generator().manual_seed(self.seed)
            eemb = (torch.rand(E, 2 * D, generator=gen) * 2 - 1) * rho
            remb = (torch.rand(R, D, generator=gen) * 2 - 1) * rho
        else:
            eemb, remb = (torch.as_tensor(x, dtype=torch.float32).clone() for x in _tables)
            if tuple(eemb.shape) != (E, 2 * D) or tuple(remb.shape) != (R, D):
                raise ValueError("tables of shape %s / %s do not fit %d entities, %d relations, dim %d"
                                 % (tuple(eemb.shape), tuple(remb.shape), E, R, D))
        self.eemb = eemb.to(dev).contiguous().requires_grad_(True)
        self.remb = remb.to(dev).contiguous().requires_grad_(True)
        # the step writes both gradients whole, every call
        self.eemb.grad = torch.zeros_like(self.eemb)
        self.remb.grad = torch.zeros_like(self.remb)
        self.lr = self.learning_rate
        self.optimizer = self._new_optimizer()
        self.step = 0
        self._order_gen = torch.Generator().manual_seed(self.seed + 1)
        self._order = torch.empty(0, dtype=torch.int64, device=dev)
        self._scratch = None
        self._filters = None
        self.capped = torch.zeros(1, dtype=torch.int32, device=dev)

    # ------------------------------------------------------------- host side
    def _triples(self, facts):
        tr = np.asarray(facts, dtype=np.int64).reshape(-1, 3)
        return np.ascontiguousarray(tr[tr[:, 1] < self.num_relations])

    def _new_optimizer(self):
        return torch.optim.Adam([self.eemb, self.remb], lr=self.lr)

    def _after_step(self):
        """The schedule, after step `self.step` ran: once it has reached
        warm_up_steps the learning rate drops tenfold, Adam starts afresh and
        the next drop moves to three times that step count."""
        if self.step >= self.warm_up_steps:
            self.lr = self.lr / 10
            self.optimizer = self._new_optimizer()
            self.warm_up_steps = self.warm_up_steps * 3
        self.step += 1

    def _next_batch(self):
        """The next batch_size indices of the shuffled epoch order, on the
        trainer's device (a new permutation, drawn on the host from the seeded
        generator and copied over once, is appended whenever the current one
        runs out)."""
        n, B = len(self.train_triples), self.batch_size
        while self._order.numel() < B:
            self._order = torch.cat([self._order, torch.randperm(n, generator=self._order_gen).to(self.device)])
        idx, self._order = self._order[:B], self._order[B:]
        return idx

    def config(self):
        return {"model": "RotatE", "double_entity_embedding": True, "double_relation_embedding": False,
                "data_path": getattr(self.graph, "data_path", None),
                "negative_sample_size": self.negative_sample_size, "hidden_dim": self.hidden_dim,
                "gamma": self.gamma, "negative_adversarial_sampling": self.negative_adversarial_sampling,
                "adversarial_temperature": self.adversarial_temperature, "batch_size": self.batch_size,
                "regularization": 0.0, "uni_weight": self.uni_weight, "learning_rate": self.learning_rate,
                "max_steps": self.max_steps, "warm_up_steps": self._warm_up_arg, "seed": self.seed,
                "nentity": self.num_entities, "nrelation": self.num_relations}

    def save(self, path):
        """config.json, entity_embedding.npy and relation_embedding.npy, as
        embedding.RotatE (and the reference's loader) read them."""
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, "config.json"), "w") as f:
            json.dump(self.config(), f)
        np.save(os.path.join(path, "entity_embedding.npy"), self.eemb.detach().cpu().numpy())
        np.save(os.path.join(path, "relation_embedding.npy"), self.remb.detach().cpu().numpy())

    @classmethod
    def load(cls, graph, path, **kw):
        """A trainer that starts from the tables saved under `path`; the recipe
        fields of its config.json are the defaults of the keyword arguments."""
        with open(os.path.join(path, "config.json")) as f:
            cfg = json.load(f)
        for key in ("batch_size", "negative_sample_size", "negative_adversarial_sampling",
                    "adversarial_temperature", "uni_weight", "learning_rate", "max_steps", "warm_up_steps"):
            if cfg.get(key) is not None:
                kw.setdefault(key, cfg[key])
        eemb = np.load(os.path.join(path, "entity_embedding.npy"), allow_pickle=False)
        remb = np.load(os.path.join(path, "relation_embedding.npy"), allow_pickle=False)
        kw.setdefault("num_relations", int(cfg["nrelation"]))
        return cls(graph, cfg["hidden_dim"], cfg["gamma"], _tables=(eemb, remb), **kw)

    # ----------------------------------------------------------- device side
    def _need_gpu(self, what):
        if self.device.type != "cuda":
            raise RuntimeError("%s runs on the HIP path; construct the trainer on a GPU" % what)

    def sample_negatives(self, positives, mode, step, n_neg=None):
        """(B, N) int32 negatives for (B, 3) int64 device positives;
        self.capped holds the call's count of capped slots."""
        self._need_gpu("sample_negatives")
        positives = positives.to(self.device, torch.int64).contiguous()
        return sample_negatives(self.true[MODES[mode]], positives, mode, self.num_entities,
                                int(n_neg or self.negative_sample_size), self.seed, step, self.capped)

    def _check_negatives(self, neg, rows):
        neg = torch.as_tensor(neg).to(self.device)
        if neg.dim() != 2 or neg.size(0) != rows or neg.size(1) < 1:
            raise ValueError("negatives must be (%d, N >= 1), got %s" % (rows, tuple(neg.shape)))
        if bool(((neg < 0) | (neg >= self.num_entities)).any()):
            raise ValueError("negatives outside [0, %d)" % self.num_entities)
        return neg.to(torch.int32).contiguous()

    @_native.on_self_device
    def train_step(self, neg=None):
        """One step: tail mode on even steps, head mode on odd ones.  Returns
        the (positive, negative, total) losses as a 3-element device tensor,
        without a synchronisation or a host copy (but for the epoch order: one
        copy of the new permutation per epoch, _next_batch).  neg: (B, N) negatives to use in place of
        the sampler's (range-checked; for tests)."""
        self._need_gpu("train_step")
        mode = self.step % 2
        if neg is not None:
            neg = self._check_negatives(neg, self.batch_size)
        idx = self._next_batch()
        positives = self.triples.index_select(0, idx)
        weights = None if self.uni_weight else self.weights.index_select(0, idx)
        if neg is None:
            neg = self.sample_negatives(positives, mode, self.step)
        if self._scratch is None or self._scratch[0] != tuple(neg.shape):
            self._scratch = (tuple(neg.shape), step_scratch(neg.size(0), neg.size(1), self.num_entities,
                                                            self.hidden_dim, self.device))
        _, _, losses, _, _ = rotate_step(self.eemb.detach(), self.remb.detach(), self.gamma, positives, neg, weights,
                                         mode, self.alpha, self._scratch[1], self.eemb.grad, self.remb.grad)
        self.optimizer.step()
        self._after_step()
        return losses

    def train(self, steps=None, log_steps=100, log=print):
        """Runs `steps` steps (default: up to max_steps) and logs the running
        means of the three losses every log_steps steps."""
        end = self.max_steps if steps is None else self.step + int(steps)
        acc, count = torch.zeros(3, dtype=torch.float64, device=self.device), 0
        while self.step < end:
            acc += self.train_step().double()
            count += 1
            if self.step % log_steps == 0 or self.step == end:
                mean = (acc / count).tolist()
                for name, v in zip(("positive_sample_loss", "negative_sample_loss", "loss"), mean):
                    log("Training average %s at step %d: %f" % (name, self.step, v))
                acc.zero_()
                count = 0
        return self

    @_native.on_self_device
    def evaluate(self, split="test", chunk=1024):
        """Filtered MRR, MR and HITS@1/3/10 of `split` ('valid' / 'test' /
        'train') over both modes: every other true answer of train, valid and
        test is filtered, rank = 1 + #(filtered scores > the answer's score)."""
        self._need_gpu("evaluate")
        dev, E, R = self.device, self.num_entities, self.num_relations
        if self._filters is None:
            every = np.concatenate([self._triples(getattr(self.graph, s + "_facts")) for s in ("train", "valid", "test")])
            self._filters = {m: _DeviceLists(true_answers(every, E, m), dev) for m in MODES}
        rows = torch.from_numpy(self._triples(getattr(self.graph, split + "_facts"))).to(dev)
        if rows.size(0) == 0:
            raise ValueError("split %r has no triple with a relation below num_relations" % split)
        rot = RotatE.from_tables(self.eemb.detach(), self.remb.detach(), self.gamma).to(dev)
        ranks = []
        stream = torch.cuda.current_stream(dev).cuda_stream
        for mode, name in enumerate(MODES):
            for lo in range(0, rows.size(0), chunk):
                part = rows[lo:lo + chunk]
                n = part.size(0)
                anchor = part[:, 0 if mode == 0 else 2].contiguous()
                answer = part[:, 2 if mode == 0 else 0].contiguous()
                rel = (part[:, 1] + (R if mode else 0)).contiguous()  # the negated half: h = t o conj(r)
                score = torch.empty((n, E), dtype=torch.float32, device=dev)
                rot.score_into(anchor, rel, score)
                flag = torch.empty((n, E), dtype=torch.uint8, device=dev)
                keys = (part[:, 1] * E + anchor).contiguous()
                self._filters[name].rows("rnnl_filter_flags", keys, E, flag)
                mask = torch.ones((n, E), dtype=torch.uint8, device=dev)
                L = torch.empty(n, dtype=torch.int64, device=dev)
                H = torch.empty(n, dtype=torch.int64, device=dev)
                _native.call("rnnl_filtered_ranks", score.data_ptr(), mask.data_ptr(), flag.data_ptr(),
                             answer.data_ptr(), n, E, L.data_ptr(), H.data_ptr(), stream)
                ranks.append(L)
        rk = torch.cat(ranks).double()
        out = {"MRR": (1.0 / rk).mean(), "MR": rk.mean()}
        for k in (1, 3, 10):
            out["HITS@%d" % k] = (rk <= k).double().mean()
        return {k: float(v) for k, v in out.items()}


RECIPE_DEFAULTS = dict(batch_size=128, negative_sample_size=128, negative_adversarial_sampling=1,
                       adversarial_temperature=1.0, uni_weight=0, regularization=0.0, learning_rate=1e-4,
                       max_steps=10000, warm_up_steps=None, num_relations=None, seed=0)


def main(argv=None):
    """Train (from random tables, or from --init_checkpoint), evaluate valid
    and test, save.  With --init_checkpoint the tables, hidden_dim, gamma and
    every recipe flag that is not given come from that directory's
    config.json; the step counter and the warm-up schedule start at 0."""
    p = argparse.ArgumentParser(description="Train RotatE entity embeddings on the GPU", epilog=main.__doc__)
    p.add_argument("--data_path", required=True)
    p.add_argument("--save_path", required=True)
    p.add_argument("--hidden_dim", type=int, default=None, help="default 500; with --init_checkpoint: its own")
    p.add_argument("--gamma", type=float, default=None, help="default 12.0; with --init_checkpoint: its own")
    for name, default in RECIPE_DEFAULTS.items():  # only the flags that are given reach RotatETrainer.load
        p.add_argument("--" + name, type=float if isinstance(default, float) else int, default=argparse.SUPPRESS,
                       help="default %s" % (default,))
    p.add_argument("--log_steps", type=int, default=100)
    p.add_argument("--init_checkpoint", default=None)
    a = p.parse_args(argv)
    given = {k: v for k, v in vars(a).items() if k in RECIPE_DEFAULTS}
    for flag in ("negative_adversarial_sampling", "uni_weight"):
        if flag in given:
            given[flag] = bool(given[flag])
    graph = KnowledgeGraph(a.data_path)
    if a.init_checkpoint:
        tr = RotatETrainer.load(graph, a.init_checkpoint, **given)
        for name, have in (("hidden_dim", tr.hidden_dim), ("gamma", tr.gamma)):
            if getattr(a, name) is not None and getattr(a, name) != have:
                raise ValueError("--%s %s differs from the checkpoint's %s" % (name, getattr(a, name), have))
    else:
        kw = dict(RECIPE_DEFAULTS, negative_adversarial_sampling=True, uni_weight=False)
        kw.update(given)
        tr = RotatETrainer(graph, 500 if a.hidden_dim is None else a.hidden_dim,
                           12.0 if a.gamma is None else a.gamma, **kw)
    tr.train(log_steps=a.log_steps)
    for split in ("valid", "test"):
        for k, v in tr.evaluate(split).items():
            print("%s %s at step %d: %f" % (split.capitalize(), k, tr.step - 1, v))
    tr.save(a.save_path)


if __name__ == "__main__":
    main()
