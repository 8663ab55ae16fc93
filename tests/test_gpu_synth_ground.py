"""The grounding and scoring paths that no shipped dataset reaches, on the
synthetic graphs of tests/synth_graphs.py (tests/test_synth_audit.py holds
every query to its regime against the constants of csrc/fwd.h):

  few1..few5   <= HB_LOAD contributions on 200,003 entities: one hash pass
               over [0, E), wider than any workgroup size can rank — the
               unranked, unmerged bucket emission of hash_pass
  sparse       light windows merged into passes wider than 98,304 entities
  dense        the dense window_pass at lo > 0
  last         window_pass on the last window, cut by E
  limit, over  two windows with exactly HB_LOAD / HB_LOAD + 1 contributions
  spill        more level-1 keys than phase A's hash holds (the 64-probe
               give-up, the full-table compaction, batches longer than a
               workgroup), 5,000 unmerged entries at three shared candidates
  deg63..129   candidate counts around the scoring chunk of 64
  loop         the query's own edge is a self-loop met at hop 1 and hop 2;
               one candidate holds the same rule-end node twice
  (limit19)    2^19 entities: 19 entity bits in the grounding keys

Exact integers against the C oracle (oracle/ground_oracle.c), scores against
the numpy restatement of the reference (oracle/reference_np.py), and every
consumer of the unmerged buckets: the SUM / PNA scoring kernels, the pair
memo, the EM Predictor's score and H statistics, the COO export
(explain_rows), the fused backward and the overflow retry.
"""
import json
import os

import numpy as np
import pytest
import torch

import synth_graphs as sg
import topk_ref
from oracle import ground_c
from oracle import reference_np as ref

pytestmark = pytest.mark.gpu

TOL = 1e-4        # tests/test_gpu_forward.py: entity scores within 1e-4 fp32
SCORE_TOL = 1e-4  # tests/test_em_predictor.py
K = 10

CONFIGS = [(t, a, f) for a in ("sum", "pna") for t in ("emb", "lstm") for f in ("bias", "none", "RotatE")]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


class Env(object):
    """One synthetic graph on disk, its loaders, its oracle and its rows."""

    def __init__(self, spec, root):
        from rnnlogic_amd.data import KnowledgeGraph
        self.spec = spec
        self.path, self.rule_path = sg.write(spec, root / spec.name)
        self.graph = KnowledgeGraph(self.path)
        self.g = ref.Graph(self.path)
        self.rules = ref.Rules(self.rule_path, self.g.relation_size)
        self.orc = ground_c.Oracle(ground_c.CGraph(spec.E, spec.R, spec.facts), self.rules.rules, spec.R)
        self.names, self.h, self.r, self.t, self.etr = sg.rows(spec)
        assert self.g.adj[sg.R0][0][self.etr].tolist() == self.h.tolist()
        assert self.g.adj[sg.R0][1][self.etr].tolist() == self.t.tolist()
        # a D = 4 RotatE table
        rng = np.random.default_rng(11)
        self.rotate_path = str(root / (spec.name + "_rotate"))
        os.makedirs(self.rotate_path)
        with open(os.path.join(self.rotate_path, "config.json"), "w") as f:
            json.dump({"hidden_dim": 4, "gamma": 9.0, "nentity": spec.E, "nrelation": spec.R}, f)
        np.save(os.path.join(self.rotate_path, "entity_embedding.npy"),
                rng.uniform(-2.75, 2.75, (spec.E, 8)).astype(np.float32))
        np.save(os.path.join(self.rotate_path, "relation_embedding.npy"),
                rng.uniform(-2.75, 2.75, (spec.R, 4)).astype(np.float32))

    def model(self, dev, typ="emb", agg="sum", feature="bias"):
        """Seeded as tests/test_gpu_edge_cases.py's build(), hidden 16."""
        from rnnlogic_amd.predictors import PredictorPlus
        torch.manual_seed(0)
        m = PredictorPlus(self.graph, type=typ, hidden_dim=16, entity_feature=feature, aggregator=agg,
                          embedding_path=self.rotate_path if feature == "RotatE" else None)
        m.set_rules(self.rule_path)
        if feature == "bias":
            with torch.no_grad():
                m.bias.normal_()
        return m.to(dev).eval()

    def reference(self, model, typ, agg, feature, train):
        sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
        rot = ref.load_rotate(self.rotate_path) if feature == "RotatE" else None
        return ref.predictorplus_forward(sd, dict(type=typ, aggregator=agg, entity_feature=feature), self.g, self.rules,
                                         self.h, self.r, self.etr if train else None, rotate=rot)

    def dev_rows(self, dev, train, repeat=1, extra=True):
        """(h, r, etr or None) on the device and the oracle's removed edges:
        the regime queries, `extra` a row of the relation without rules,
        tiled to `repeat` rows."""
        h, r, etr, rs, rd = self.h, self.r, self.etr, self.h, self.t
        if extra:
            f4 = [f for f in self.spec.facts if f[1] == sg.R4][0]
            h, r, etr = np.append(h, f4[0]), np.append(r, sg.R4), np.append(etr, 0)
            rs, rd = np.append(rs, f4[0]), np.append(rd, f4[2])
        if repeat > 1:
            idx = np.arange(repeat) % len(h)
            h, r, etr, rs, rd = h[idx], r[idx], etr[idx], rs[idx], rd[idx]
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        return (to(h), to(r), to(etr) if train else None), (h, r, rs if train else None, rd if train else None)


@pytest.fixture(scope="module")
def main(tmp_path_factory):
    return Env(sg.main_graph(), tmp_path_factory.mktemp("synth"))


@pytest.fixture(scope="module")
def limit19(tmp_path_factory):
    return Env(sg.limit_graph(), tmp_path_factory.mktemp("synth19"))


@pytest.fixture(scope="module", autouse=True)
def shared_reference_grounding():
    """The reference's path counts do not depend on the model: each
    (rows, rule, removal) is grounded once for the whole module."""
    plain, memo = ref.grounding, {}

    def grounding(g, h, r, body, edges_to_remove):
        key = (id(g), np.asarray(h).tobytes(), int(r), tuple(body),
               None if edges_to_remove is None else np.asarray(edges_to_remove).tobytes())
        if key not in memo:
            memo[key] = plain(g, h, r, body, edges_to_remove)
            memo[key].setflags(write=False)
        return memo[key]
    ref.grounding = grounding
    yield
    ref.grounding = plain


def check_scores(got, gmask, want, wmask, what, tol=TOL):
    """tests/test_gpu_edge_cases.py's check(): masks and the non-finite
    pattern equal, finite scores within tol; returns the largest error."""
    assert np.array_equal(gmask, wmask), what
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin), what
    assert np.array_equal(got[~fin], want[~fin]), what  # -inf off the mask (feature none)
    d = np.zeros(want.shape)
    d[fin] = np.abs(got[fin].astype(np.float64) - want[fin])
    err = float(d.max(initial=0.0))
    print("%s: max |score - reference| %.3g (worst row %d)" % (what, err, int(d.max(1).argmax())))
    assert err <= tol, (what, err)
    return err


# ----------------------------------------------------------------------------- 1. exact integers
LAUNCHES = {
    # name (lanes per grounding workgroup): (rows the queries are tiled to, entity feature)
    "wide1024": (0, "bias"),     # <= WIDE_ROWS rows
    "solo512": (300, "bias"),    # more rows, the chip to itself
    "beside256": (300, "RotatE"),  # more rows beside the RotatE kernel (overlap)
}


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("agg", ["sum", "pna"])
@pytest.mark.parametrize("launch", sorted(LAUNCHES))
def test_digests_and_candidate_counts(main, dev, launch, agg, train):
    """forward_rows' path-count digests and candidate counts equal the C
    oracle's for every regime query, at all three workgroup sizes; repeated
    rows are bitwise their first occurrence."""
    repeat, feature = LAUNCHES[launch]
    model = main.model(dev, "emb", agg, feature)
    assert model.overlap is True and model.native_dedupe_min is None
    (h, r, etr), (oh, orr, rs, rd) = main.dev_rows(dev, train, repeat)
    want_d, want_n = main.orc.digests(oh, orr, rs, rd)
    dig = torch.zeros(h.numel(), dtype=torch.int64, device=dev)
    with torch.no_grad():
        score, mask, ncand = model.forward_rows(h, r, etr, return_ncand=True, digest=dig)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(ncand.cpu().numpy(), want_n)
    np.testing.assert_array_equal(dig.cpu().numpy().view(np.uint64), want_d)
    n = len(main.names) + 1
    for s in range(n, h.numel(), n):  # on the device: each repeat against the first block
        m = min(n, h.numel() - s)
        assert torch.equal(score[s:s + m], score[:m]), (launch, s)
        assert torch.equal(mask[s:s + m], mask[:m]), (launch, s)


@pytest.mark.parametrize("agg", ["sum", "pna"])
def test_digests_at_2_19_entities(limit19, dev, agg):
    model = limit19.model(dev, "emb", agg, "bias")
    for train in (False, True):
        (h, r, etr), (oh, orr, rs, rd) = limit19.dev_rows(dev, train)
        want_d, want_n = limit19.orc.digests(oh, orr, rs, rd)
        dig = torch.zeros(h.numel(), dtype=torch.int64, device=dev)
        with torch.no_grad():
            _, _, ncand = model.forward_rows(h, r, etr, return_ncand=True, digest=dig)
        np.testing.assert_array_equal(ncand.cpu().numpy(), want_n)
        np.testing.assert_array_equal(dig.cpu().numpy().view(np.uint64), want_d)


# ----------------------------------------------------------------------------- 2. scores and masks
@pytest.mark.parametrize("typ,agg,feature", CONFIGS)
def test_scores_match_reference(main, dev, typ, agg, feature):
    model = main.model(dev, typ, agg, feature)
    for train in (False, True):
        (h, r, etr), _ = main.dev_rows(dev, train, extra=False)
        with torch.no_grad():
            score, mask = model.forward_rows(h, r, etr)
        want, wmask = main.reference(model, typ, agg, feature, train)
        check_scores(score.cpu().numpy(), mask.cpu().numpy(), want, wmask,
                     "%s/%s/%s %s" % (typ, agg, feature, "train" if train else "eval"))


@pytest.mark.parametrize("typ,agg,feature", [("emb", "sum", "bias"), ("lstm", "pna", "none")])
def test_scores_at_2_19_entities(limit19, dev, typ, agg, feature):
    model = limit19.model(dev, typ, agg, feature)
    for train in (False, True):
        (h, r, etr), _ = limit19.dev_rows(dev, train, extra=False)
        with torch.no_grad():
            score, mask = model.forward_rows(h, r, etr)
        want, wmask = limit19.reference(model, typ, agg, feature, train)
        check_scores(score.cpu().numpy(), mask.cpu().numpy(), want, wmask,
                     "2^19 %s/%s/%s %s" % (typ, agg, feature, "train" if train else "eval"))


# ----------------------------------------------------------------------------- 3. consumers of the buckets
@pytest.mark.parametrize("feature", ["bias", "none"])
def test_em_predictor_forward_and_H(main, dev, feature):
    """The EM Predictor's score (sum of count x rule weight) and compute_H on
    the regime queries.  Rule weights of 1e-3: the spill query's 5,000-path
    scores stay near 5, where fp32 resolves far below SCORE_TOL."""
    from rnnlogic_amd.predictors import Predictor
    pred = Predictor(main.graph, entity_feature=feature)
    pred.set_rules(main.rule_path)
    torch.manual_seed(0)
    with torch.no_grad():
        pred.rule_weights.normal_().mul_(1e-3)
        if feature == "bias":
            pred.bias.normal_()
    pred = pred.to(dev).eval()
    sd = {k: v.detach().cpu().numpy() for k, v in pred.state_dict().items()}
    for train in (False, True):
        (h, r, etr), _ = main.dev_rows(dev, train, extra=False)
        what = "EM/%s %s" % (feature, "train" if train else "eval")
        with torch.no_grad():
            score, mask, ncand = pred.forward_rows(h, r, etr, return_ncand=True)
        want, wmask = ref.predictor_forward(sd, feature, main.g, main.rules, main.h, main.r,
                                            main.etr if train else None)
        check_scores(score.cpu().numpy(), mask.cpu().numpy(), want, wmask, what, SCORE_TOL)
        assert ncand.tolist() == [sg.audit(main.spec, n, train).n_cand for n in main.names]
        t = torch.from_numpy(main.t).to(dev)
        with torch.no_grad():
            H, index = pred.compute_H(h, r, t, etr)
        wH, windex = ref.predictor_compute_H(sd, main.g, main.rules, main.h, main.r, main.t,
                                             main.etr if train else None)
        np.testing.assert_array_equal(index.cpu().numpy(), windex)
        print("%s: max |H - reference| %.3g" % (what, float(np.abs(H.cpu().numpy() - wH).max())))
        np.testing.assert_allclose(H.cpu().numpy(), wH, atol=1e-5, rtol=0)


@pytest.mark.parametrize("kind", ["plus", "em"])
def test_explain_rows_equals_oracle_rule_counts(main, dev, kind):
    """explain_rows (the COO export) against the C oracle's per-rule path
    counts, exactly: per query its tail, its smallest and largest candidates,
    the shared spill targets, a non-candidate and an unused slot."""
    if kind == "plus":
        model = main.model(dev)
    else:
        from rnnlogic_amd.predictors import Predictor
        model = Predictor(main.graph, entity_feature="bias")
        model.set_rules(main.rule_path)
        model = model.to(dev).eval()
    E, nrule = main.spec.E, len(main.spec.rules)
    for train in (False, True):
        ents = []
        for n, (h, t) in main.spec.queries.items():
            ct = main.orc.candidates(h, sg.R0, h if train else -1, t if train else -1)[0]
            ents.append([t, int(ct[0]), int(ct[len(ct) // 2]), int(ct[-1]), 7, E - 1, 9, -1])
        ents = np.asarray(ents, dtype=np.int64)
        m = ents.shape[1]
        # the oracle counts paths to one tail per row: a row per (query, slot)
        qh, qr, qe = np.repeat(main.h, m), np.repeat(main.r, m), np.maximum(ents.reshape(-1), 0)
        rs, rd = (np.repeat(main.h, m), np.repeat(main.t, m)) if train else (None, None)
        rq_ptr, pos, _ = main.orc.query_stats(qh, qr, qe, rs, rd)
        assert (np.diff(rq_ptr) == nrule).all()
        pos = pos.reshape(-1, nrule)
        want = [[(i, int(c)) for i, c in enumerate(pos[s]) if c > 0] if ents.reshape(-1)[s] >= 0 else []
                for s in range(len(qe))]
        assert sum(1 for w in want if w) > 3 * len(main.names) and any(dict(w).get(2) == 5000 for w in want)
        (h, r, etr), _ = main.dev_rows(dev, train, extra=False)
        off, rule, count = [x.cpu().numpy() for x in
                            model.explain_rows(h, r, torch.from_numpy(ents).to(dev), edges_to_remove=etr)]
        assert len(off) == len(want) + 1 and off[0] == 0 and off[-1] == len(rule) == len(count)
        for s, w in enumerate(want):
            got = list(zip(rule[off[s]:off[s + 1]].tolist(), count[off[s]:off[s + 1]].tolist()))
            assert got == w, (kind, train, main.names[s // m], int(ents.reshape(-1)[s]), got, w)


@pytest.mark.parametrize("typ,feature,repeat", [("emb", "bias", 0), ("lstm", "none", 300), ("emb", "RotatE", 300)])
def test_pair_memo_is_bit_identical(main, dev, typ, feature, repeat):
    """The SUM pair memo keys a candidate's score by its one to three bucket
    entries; the unmerged buckets hold entries the merged ones never do (one
    node twice: the loop query).  On and off must agree bitwise."""
    from rnnlogic_amd import _native
    model = main.model(dev, typ, "sum", feature)
    (h, r, _), _ = main.dev_rows(dev, False, repeat)
    outs = []
    try:
        for on in (0, 1):
            _native.call("rnnl_debug_pair_memo", on)
            with torch.no_grad():
                outs.append(model.forward_rows(h, r, None, return_ncand=True))
            torch.cuda.synchronize()
    finally:
        _native.call("rnnl_debug_pair_memo", 1)
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("typ,agg,feature", [("emb", "sum", "bias"), ("lstm", "pna", "none")])
def test_predict_topk_on_own_scores(main, dev, typ, agg, feature):
    model = main.model(dev, typ, agg, feature)
    (h, r, _), _ = main.dev_rows(dev, False)
    with torch.no_grad():
        score, mask = model.forward_rows(h, r, None)
    got = [x.cpu().numpy() for x in model.predict_topk(h, r, K)]
    want = topk_ref.topk_ref(score.cpu().numpy(), mask.cpu().numpy(), None, None, K)
    topk_ref.assert_equal(got, want, "%s/%s/%s" % (typ, agg, feature))
    if feature == "none":  # only candidates are eligible: few1 has two, the relation without rules none
        assert got[2][0] == 2 and got[2][-1] == 0


# ----------------------------------------------------------------------------- 4. backward
@pytest.mark.parametrize("typ,agg,feature", [("emb", "sum", "bias"), ("lstm", "sum", "none"), ("emb", "pna", "bias"),
                                             ("lstm", "pna", "none")])
def test_fused_backward_matches_autograd(main, dev, typ, agg, feature):
    """tests/test_gpu_train.py's test_fused_backward_matches_autograd (its
    loss, its tolerances) on one training batch per regime query, each row's
    own edge removed, and on all of them tiled to 300 rows (the 512-lane
    grounding).  A batch is the regime query and the loop query: alone, a
    query whose candidates all carry the same rule counts (dense: 2,000
    candidates of one r1 path each) has a gradient of exactly zero for every
    rule parameter, and the comparison would hold fp32 noise of the autograd
    path (1e-6 measured) against the tolerance's absolute floor."""
    from rnnlogic_amd.predictors import PredictorPlus
    torch.manual_seed(5)
    model = PredictorPlus(main.graph, type=typ, num_layers=3, hidden_dim=16, entity_feature=feature, aggregator=agg)
    model.set_rules(main.rule_path)
    with torch.no_grad():
        for n, prm in model.named_parameters():
            prm.add_(torch.randn_like(prm) * 0.3)
    model = model.to(dev).train()
    loop, few5 = main.names.index("loop"), main.names.index("few5")
    batches = [(n, np.array([i, loop if i != loop else few5])) for i, n in enumerate(main.names)]
    batches.append(("all x 300", np.arange(300) % len(main.names)))
    for name, idx in batches:
        all_h, all_r, all_t, etr = [torch.from_numpy(a[idx]).to(dev) for a in (main.h, main.r, main.t, main.etr)]
        res = []
        for fused in (True, False):
            model.fused_backward = fused
            model.zero_grad(set_to_none=True)
            logits, mask = model(all_h, all_r, etr)
            assert bool(mask.any()), name
            lp = (torch.softmax(logits, dim=1) + 1e-8).log()
            tt = torch.zeros_like(lp)
            tt[torch.arange(len(idx), device=dev), all_t] = 1.0
            loss = -(lp[mask] * tt[mask]).sum() / torch.clamp(tt[mask].sum(), min=1)
            loss.backward()
            res.append((loss.item(), {n: (p.grad.detach().clone() if p.grad is not None else None)
                                      for n, p in model.named_parameters()}))
            del logits, lp, tt, loss
        (l1, g1), (l2, g2) = res
        assert abs(l1 - l2) <= 1e-5 * abs(l2), (name, l1, l2)
        for n in g2:
            a, b = g1[n], g2[n]
            if b is None:
                assert a is None or float(a.abs().max()) == 0.0, (name, n)
                continue
            atol = max(2e-4 * float(b.abs().max()), 1e-6)
            np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-3, atol=atol,
                                       err_msg="%s/%s/%s batch %s grad %s" % (typ, agg, feature, name, n))


# ----------------------------------------------------------------------------- 5. overflow retry
@pytest.mark.parametrize("agg", ["sum", "pna"])
def test_spill_query_alone_and_after_overflow_retry(main, dev, agg):
    """The spill query in a one-row launch — its 25,001 contributions are
    three times the per-query pool share — is bitwise the same row inside the
    launch of all queries; and again with the capacities lowered
    (rnnl_debug_capacity) so that the frontier, the contribution list and the
    pool all overflow and the launch is retried."""
    from rnnlogic_amd import _native
    model = main.model(dev, "emb", agg, "bias")
    (h, r, _), _ = main.dev_rows(dev, False)
    k = main.names.index("spill")
    assert sg.audit(main.spec, "spill").P > 8192
    with torch.no_grad():
        score, mask, ncand = model.forward_rows(h, r, None, return_ncand=True)
        one = model.forward_rows(h[k:k + 1], r[k:k + 1], None, return_ncand=True)
    torch.cuda.synchronize()
    print("spill alone: capacity_scale %d" % model.capacity_scale)
    want = (score[k:k + 1], mask[k:k + 1], ncand[k:k + 1])
    for a, b in zip(one, want):
        assert torch.equal(a, b)
    _native.call("rnnl_debug_capacity", 1024, 1024, 64)
    try:
        model.capacity_scale = 1
        model._ws, model._ws_chunks = {}, {}
        with torch.no_grad():
            again = model.forward_rows(h[k:k + 1], r[k:k + 1], None, return_ncand=True)
        torch.cuda.synchronize()
        retried = model.capacity_scale
    finally:
        _native.call("rnnl_debug_capacity", 0, 0, 0)
        model.capacity_scale = 1
        model._ws, model._ws_chunks = {}, {}
    print("spill alone, capacities 1024 / 1024 / 64: retried up to capacity_scale %d" % retried)
    assert retried > 1, "the lowered capacities did not overflow"
    for a, b in zip(again, want):
        assert torch.equal(a, b)
