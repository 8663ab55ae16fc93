"""Records every output gradient of the three training backward paths —
rnnl_predictor_backward (the EM Predictor), rnnl_predictorplus_backward
(PredictorPlus SUM) and rnnl_pna_features_backward (PNA) — on the synthetic
graph of tests/plus_ref.small_graph into tests/golden/_node_grads_parent.npz.

The fixture pins the bits of the fixed-point node-gradient accumulation
across its consolidation into csrc/grad_fix.h: it is generated on the GPU in a
checkout of the commit BEFORE the consolidation (only this file is added
there) and tests/test_gpu_node_grads_pin.py compares what the library computes
now with it, so the expected values never come from the code under test.

  python tools/make_golden_node_grads.py [OUT.npz]

Cases (rows: plus_ref.SETS; the seeds below are stored in the file too):
  A      five rows of head A: 819 trie nodes, on both sides of BW_LDS_NODES =
         768 and PG_LDS_NODES = 96, bucket lists at and past BW_BIG.
  B      every star centre of head B once (1 .. 129 candidates a row).
  mixed  24 rows of heads A, B, C, D in one launch (head = -1: no LDS table).
         The gradient of row i of head A is scaled by 2^-(34 + 2 i): next to
         the other heads' O(1) gradients it lands within a few units of the
         launch's fixed-point grid, where "on the grid once per candidate,
         times the integer count" and "count x gradient, then onto the grid"
         give different integers — head A's path counts exceed 1, and its
         nodes see no other gradient, so the difference survives the final
         rounding.
  nan    five rows of head B with one NaN in the incoming gradient.

Per case: em/<case> = grad_node (float64) of rnnl_predictor_backward on the
grounding of the rows; sum/<case>/<parameter> = every parameter gradient that
rnnl_predictorplus_backward writes (PredictorPlus emb / sum / bias through
forward_autograd; the bias gradient is a torch column sum and is left out);
pna/<case> = d_x of _PnaStats under four incoming gradients given in (row,
entity) order.  sha/<key> = sha256 of the bytes of each array without a NaN.
The file name starts with an underscore because tests/conftest.py lists every
other tests/golden/*.npz as a forward-fixture case.
"""
import hashlib
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = os.path.join(REPO, "tests", "golden", "_node_grads_parent.npz")
# case: (plus_ref set, seed of the incoming gradients)
CASES = {"A": ("A5", 11), "B": ("stars", 12), "mixed": ("mixed", 13), "nan": ("B5", 14)}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def shrink_head_a(scale_rows, rel_of_row):
    """Row i (in row order) of head A -> 2^-(34 + 2 i), every other row 1."""
    import plus_ref as pr
    f = np.ones(len(rel_of_row), dtype=np.float64)
    rows = np.nonzero(np.asarray(rel_of_row) == pr.REL["A"])[0]
    f[rows] = np.ldexp(1.0, -(34 + 2 * np.arange(len(rows))))
    return f[scale_rows]


def upstream(case, rel, E):
    """The incoming score gradient (nq, E) float32 of `case` (before its NaN)."""
    import plus_ref as pr
    G = pr.upstream(len(rel), E, CASES[case][1]).astype(np.float64)
    if case == "mixed":
        G *= shrink_head_a(np.arange(len(rel)), rel)[:, None]
    return G.astype(np.float32)


def upstream4(case, row, rel):
    """PNA's four incoming gradients (C, 16) float32 for the candidates in
    (row, entity) order; `row` = their rows."""
    rng = np.random.default_rng([20250611, CASES[case][1]])
    gs = [rng.standard_normal((len(row), 16)) + 0.5 for _ in range(4)]
    if case == "mixed":
        gs = [g * shrink_head_a(row, rel)[:, None] for g in gs]
    gs = [g.astype(np.float32) for g in gs]
    if case == "nan":
        gs[1][len(row) // 2, 3] = np.nan
    return gs


class World:
    def __init__(self, root, dev):
        import torch

        import plus_ref as pr
        from oracle import reference_np as ref
        from rnnlogic_amd.data import KnowledgeGraph
        from rnnlogic_amd.predictors import Predictor, PredictorPlus
        self.dev = dev
        self.sg = pr.small_graph(root, 0)
        self.g = ref.Graph(self.sg["path"])
        self.rules = ref.Rules(self.sg["rules"], self.g.relation_size)
        self.graph = KnowledgeGraph(self.sg["path"])
        self.E = self.g.entity_size
        self.em = Predictor(self.graph, entity_feature="bias")
        self.em.set_rules(self.sg["rules"])
        self.em = self.em.to(dev)
        self.plus, self.sd = {}, {}
        for agg in ("sum", "pna"):
            sd = pr.params(self.sg, "emb", agg, pr.PARAM_SEED["emb", agg])
            m = PredictorPlus(self.graph, type="emb", num_layers=3, hidden_dim=16, entity_feature="bias",
                              aggregator=agg)
            m.set_rules(self.sg["rules"])
            with torch.no_grad():
                for n, prm in m.named_parameters():
                    prm.copy_(torch.from_numpy(sd[n]))
            self.plus[agg], self.sd[agg] = m.to(dev).train(), sd

    def rows(self, case):
        """(h, r, etr, head, G): head = the batch's relation, -1 for `mixed`."""
        import plus_ref as pr
        h, r, t, etr = pr.batch(self.sg, self.g, CASES[case][0])
        G = upstream(case, r, self.E)
        if case == "nan":  # at a candidate: the sixth of row 2
            c = pr.coo(self.g, self.rules, h, r, etr)
            k = int(np.nonzero(c["row"] == 2)[0][5])
            G[c["row"][k], c["ent"][k]] = np.nan
        return h, r, etr, (-1 if case == "mixed" else int(r[0])), G

    def to_dev(self, *arrays):
        import torch
        return [torch.from_numpy(np.ascontiguousarray(a)).to(self.dev) for a in arrays]


def em_grad(w, h, r, etr, G):
    """grad_node (n_nodes,) float64 of rnnl_predictor_backward."""
    import torch

    from rnnlogic_amd import _native
    m, dev = w.em, w.dev
    th, tr, te, tG = w.to_dev(h, r, etr, G)
    ws, scale, n_cand = m.ground(th, tr, te)
    nr = m.native_rules(dev)
    ld = m.head_roots(dev)[1]
    out = torch.zeros(max(nr.n_nodes, 1), dtype=torch.float64, device=dev)
    _native.call("rnnl_predictor_backward", ws.data_ptr(), len(h), scale, n_cand.data_ptr(), nr.ptr, tr.data_ptr(),
                 w.E, tG.data_ptr(), ld, out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def sum_grads(w, h, r, etr, head, G):
    """{parameter: gradient} of forward_autograd + backward(gradient=G), without the bias."""
    import torch
    m = w.plus["sum"]
    m.zero_grad(set_to_none=True)
    th, tr, te, tG = w.to_dev(h, r, etr, G)
    score, _ = m.forward_autograd(th, tr, te, query_r=head if head >= 0 else None)
    score.backward(gradient=tG)
    torch.cuda.synchronize()
    return {n: p.grad.detach().cpu().numpy().copy() for n, p in m.named_parameters()
            if n != "bias" and p.grad is not None}


def pna_grad(w, case, h, r, etr, head):
    """d_x (n_rules, 16) of _PnaStats on the rule_emb table."""
    import torch

    from rnnlogic_amd.predictors import _PnaStats
    m = w.plus["pna"]
    emb = torch.from_numpy(w.sd["pna"]["rule_emb"]).to(w.dev).requires_grad_(True)
    th, tr, te = w.to_dev(h, r, etr)
    out = _PnaStats.apply(m, emb, th, tr, te, head)
    row, ent = out[5].cpu().numpy(), out[6].cpu().numpy()
    order = np.argsort(row * w.E + ent, kind="stable")
    inv = torch.from_numpy(np.argsort(order)).to(w.dev)
    ups = [t[inv] for t in w.to_dev(*upstream4(case, row[order], r))]
    torch.autograd.backward(list(out[:4]), ups)
    torch.cuda.synchronize()
    return emb.grad.cpu().numpy()


def compute(root, dev):
    """{key: array} of every case, on the library at hand."""
    w = World(root, dev)
    rec = {}
    for case in CASES:
        h, r, etr, head, G = w.rows(case)
        rec["em/" + case] = em_grad(w, h, r, etr, G)
        for n, g in sum_grads(w, h, r, etr, head, G).items():
            rec["sum/%s/%s" % (case, n)] = g
        rec["pna/" + case] = pna_grad(w, case, h, r, etr, head)
    return rec


def main():
    import torch
    out_path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    with tempfile.TemporaryDirectory() as tmp:
        rec = compute(tmp, torch.device("cuda:0"))
    for k in sorted(rec):
        a = rec[k]
        print("%-58s %-14s nonzero %6d  NaN %6d  max |.| %.3g" % (
            k, a.shape, int(np.count_nonzero(a)), int(np.isnan(a).sum()),
            float(np.nanmax(np.abs(a))) if a.size and not np.isnan(a).all() else float("nan")), flush=True)
    for k in list(rec):
        if not np.isnan(rec[k]).any():
            rec["sha/" + k] = np.array(sha(rec[k]))
    import plus_ref as pr
    for case, (name, seed) in CASES.items():  # (incoming gradients, sum parameters, pna parameters)
        rec["seed/" + case] = np.array([seed, pr.PARAM_SEED["emb", "sum"], pr.PARAM_SEED["emb", "pna"]], dtype=np.int64)
    np.savez_compressed(out_path, **rec)
    print("wrote %s (%d bytes)" % (out_path, os.path.getsize(out_path)))


if __name__ == "__main__":
    main()
