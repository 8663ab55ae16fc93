"""predict_topk / explain_rows of both predictors and TrainerPredictor.predict
on the GPU (UMLS and kinship).

* predict_topk equals tests/topk_ref.py applied to the model's own
  forward_rows scores and mask, exactly.
* Against the CPU oracle (oracle/reference_np.py): every returned entity's
  oracle score is at least the oracle's k-th eligible score minus 2e-4 — the
  project's 1e-4 score tolerance taken on both sides of the comparison.
* Against rnnl_filtered_ranks on the same scores: the known tail kept in the
  filtered list sits between the rank bounds, L - 1 <= place <= H - 2, and is
  present whenever H - 1 <= k.
* explain_rows equals the reference grounding rule by rule, exactly, in eval
  mode and for a training batch with edges_to_remove, with a duplicated rule.
* TrainerPredictor.predict: positions, the TSV, and evaluate() unchanged
  around it (same MRR, no RNG draw).
"""
import numpy as np
import pytest
import torch

import topk_ref

pytestmark = pytest.mark.gpu

K = 10
MODELS = {  # name -> (dataset, kind, kwargs)
    "plus_lstm_sum_bias": ("umls", "plus", dict(type="lstm", entity_feature="bias", aggregator="sum")),
    "plus_emb_pna_none": ("kinship", "plus", dict(type="emb", entity_feature="none", aggregator="pna")),
    "em_bias": ("umls", "em", dict(entity_feature="bias")),
}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


_ENV, _MODEL = {}, {}


def _env(data):
    """(graph, train_set, test_set, oracle graph) of a dataset, built once."""
    if data not in _ENV:
        from oracle import reference_np as ref
        from rnnlogic_amd import datasets
        from rnnlogic_amd.data import KnowledgeGraph, TestDataset, TrainDataset
        from rnnlogic_amd.utils import set_seed
        set_seed(1)
        path = datasets.materialize(data)
        graph = KnowledgeGraph(path)
        _ENV[data] = (graph, TrainDataset(graph, 32), TestDataset(graph, 32), ref.Graph(path))
    return _ENV[data]


def _rule_tokens(data, duplicate=False):
    from rnnlogic_amd import datasets
    with open(datasets.rule_file(data)) as f:
        toks = [[int(x) for x in line.split()] for line in f if line.strip()]
    if duplicate:
        # a second copy, at the end of the list, of the rule that fires most on the first
        # explained relation's rows: both copies must be listed
        from oracle import reference_np as ref
        g = _env(data)[3]
        q, h, _ = _relation_rows(data)[0]
        ids, counts = _reference_counts(g, ref.Rules(toks, g.relation_size), q, h, None)
        toks = toks + [list(toks[int(ids[counts.reshape(len(ids), -1).sum(1).argmax()])])]
    return toks


def _model(name, dev, duplicate=False):
    """(model, oracle state dict, oracle Rules, config) with random weights."""
    key = (name, duplicate)
    if key not in _MODEL:
        from oracle import reference_np as ref
        from rnnlogic_amd.predictors import Predictor, PredictorPlus
        data, kind, kw = MODELS[name]
        graph = _env(data)[0]
        toks = _rule_tokens(data, duplicate)
        torch.manual_seed(3)
        if kind == "plus":
            model = PredictorPlus(graph, **kw)
            model.set_rules(toks)
        else:
            model = Predictor(graph, **kw)
            model.set_rules(toks)
            with torch.no_grad():
                # scores of a few units: the oracle's own fp32 sums stay well inside the 1e-4 tolerance
                model.rule_weights.normal_(0, 0.01)
        if kw["entity_feature"] == "bias":
            with torch.no_grad():
                model.bias.normal_()
        model = model.to(dev).eval()
        sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
        _MODEL[key] = (model, sd, ref.Rules(toks, graph.relation_size), dict(kw))
    return _MODEL[key]


def _eval_rows(data, dev, batches=8):
    from rnnlogic_amd.data import DeviceEvalBatches
    test_set = _env(data)[2]
    step = max(1, len(test_set) // batches)
    return DeviceEvalBatches(test_set, dev).rows(list(range(0, len(test_set), step))[:batches])


def _relation_rows(data, n_rel=6, per=32):
    """Up to `per` test rows of each of n_rel relations: [(q, h (B,), t (B,))]."""
    graph = _env(data)[0]
    by_rel = {}
    for h, r, t in graph.test_facts:
        by_rel.setdefault(r, []).append((h, t))
    rels = sorted(by_rel, key=lambda q: (-len(by_rel[q]), q))[:n_rel]
    return [(q, np.array([x[0] for x in by_rel[q][:per]]), np.array([x[1] for x in by_rel[q][:per]])) for q in rels]


@pytest.mark.parametrize("name", sorted(MODELS))
def test_predict_topk_equals_reference_on_own_scores(name, dev):
    model = _model(name, dev)[0]
    h, r, t, flag = _eval_rows(MODELS[name][0], dev)
    with torch.no_grad():
        score, mask = model.forward_rows(h, r, None)
    s, m, f, tt = score.cpu().numpy(), mask.cpu().numpy(), flag.cpu().numpy(), t.cpu().numpy()
    for fl, kp in ((flag, t), (flag, None), (None, None)):
        got = [x.cpu().numpy() for x in model.predict_topk(h, r, K, flag=fl, keep=kp)]
        want = topk_ref.topk_ref(s, m, f if fl is not None else None, tt if kp is not None else None, K)
        topk_ref.assert_equal(got, want, name)
    assert got[0].dtype == np.int32 and got[1].dtype == np.float32 and got[2].dtype == np.int32
    assert got[0].shape == (h.numel(), K) and got[2].shape == (h.numel(),)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_predict_topk_against_oracle(name, dev):
    from oracle import reference_np as ref
    model, sd, rules, kw = _model(name, dev)
    data, kind, _ = MODELS[name]
    g = _env(data)[3]
    worst = -np.inf
    for q, h, _ in _relation_rows(data):
        r = np.full(len(h), q)
        if kind == "plus":
            want, wmask = ref.predictorplus_forward(sd, kw, g, rules, h, r, None)
        else:
            want, wmask = ref.predictor_forward(sd, kw["entity_feature"], g, rules, h, r, None)
        index, _, valid = [x.cpu().numpy() for x in
                           model.predict_topk(torch.from_numpy(h).to(dev), torch.from_numpy(r).to(dev), K)]
        for i in range(len(h)):
            elig = np.sort(want[i][wmask[i] & ~np.isnan(want[i])])[::-1]
            kth = elig[K - 1] if len(elig) >= K else -np.inf
            assert valid[i] == min(K, len(elig))
            got = want[i][index[i, :valid[i]]]
            if np.isfinite(kth):
                worst = max(worst, float((kth - got).max()))
            assert (got >= kth - 2e-4).all(), (name, q, i, kth, got)
    print("%s: largest (oracle k-th score - oracle score of a returned entity) = %.3g" % (name, worst))


@pytest.mark.parametrize("name", sorted(MODELS))
def test_kept_tail_sits_between_the_rank_bounds(name, dev):
    from rnnlogic_amd.trainer import TrainerPredictor
    model = _model(name, dev)[0]
    data = MODELS[name][0]
    E = _env(data)[0].entity_size
    h, r, t, flag = _eval_rows(data, dev)
    with torch.no_grad():
        score, mask = model.forward_rows(h, r, None)
    L, H = [x.cpu().numpy() for x in TrainerPredictor.filtered_ranks(score, mask, flag, t, E)]
    index = model.predict_topk(h, r, K, flag=flag, keep=t)[0].cpu().numpy()
    cand = mask[torch.arange(h.numel(), device=dev), t].cpu().numpy()
    tt = t.cpu().numpy()
    assert cand.any()
    seen = 0
    for i in np.nonzero(cand)[0]:
        where = np.nonzero(index[i] == tt[i])[0]
        if H[i] - 1 <= K:
            assert len(where) == 1, (i, L[i], H[i])
        if len(where):
            assert L[i] - 1 <= where[0] <= H[i] - 2, (i, where[0], L[i], H[i])
            seen += 1
    assert seen


def _reference_counts(g, rules, q, h, etr):
    """(rule ids (R,), counts (R, B, |E|) int64) of the reference grounding of relation q's rules."""
    from oracle import reference_np as ref
    ids = np.array([i for i, _ in rules.relation2rules[q]], dtype=np.int64)
    counts = [ref.grounding(g, h, hd, body, etr) for _, (hd, body) in rules.relation2rules[q]]
    return ids, np.stack(counts) if counts else np.zeros((0, len(h), g.entity_size), dtype=np.int64)


def _reference_explanations(g, rules, q, h, etr, entities):
    """Per slot the exact [(rule, count)] of the reference grounding, ascending rule id."""
    ids, counts = _reference_counts(g, rules, q, h, etr)
    out = []
    for row in range(entities.shape[0]):
        for e in entities[row]:
            c = counts[:, row, e] if e >= 0 else counts[:, 0, 0] * 0
            nz = np.nonzero(c > 0)[0]
            out.append(list(zip(ids[nz].tolist(), c[nz].tolist())))
    return out


def _check_explanations(got, want, what):
    off, rule, count = [x.cpu().numpy() for x in got]
    assert off.dtype == np.int64 and rule.dtype == np.int64 and count.dtype == np.int64
    assert len(off) == len(want) + 1 and off[0] == 0 and off[-1] == len(rule) == len(count)
    for s, w in enumerate(want):
        assert list(zip(rule[off[s]:off[s + 1]].tolist(), count[off[s]:off[s + 1]].tolist())) == w, (what, s)


@pytest.mark.parametrize("name", ["plus_lstm_sum_bias", "em_bias"])
def test_explain_rows_equals_reference_grounding(name, dev):
    model, _, rules, _ = _model(name, dev, duplicate=True)
    data = MODELS[name][0]
    graph, train_set, _, g = _env(data)
    dup = len(rules.rules) - 1
    orig = rules.rules.index(rules.rules[dup])
    assert orig < dup
    both = 0
    # eval mode: six relations, up to 32 test rows each; per row its top 5, an unused slot
    # and the entity the duplicated rule reaches by most paths
    for q, h, _ in _relation_rows(data):
        th = torch.from_numpy(h).to(dev)
        tr = torch.full_like(th, q)
        top = model.predict_topk(th, tr, 5)[0]
        reach = np.full(len(h), -1, dtype=np.int32)
        if q == rules.rules[dup][0]:
            c = _reference_counts(g, rules, q, h, None)[1][-1]  # the copy is the relation's last rule
            reach = np.where(c.max(1) > 0, c.argmax(1), -1).astype(np.int32)
        ents = torch.cat([top, torch.full_like(top[:, :1], -1), torch.from_numpy(reach).to(dev).unsqueeze(1)], 1)
        want = _reference_explanations(g, rules, q, h, None, ents.cpu().numpy())
        _check_explanations(model.explain_rows(th, tr, ents), want, (name, q))
        # the same slots in chunks of 5 rows
        _check_explanations(model.explain_rows(th, tr, ents, chunk=5), want, (name, q, "chunks"))
        assert all(not w for w in want[5::7])
        both += sum(1 for w in want if dict(w).get(orig, 0) > 0 and dict(w).get(orig) == dict(w).get(dup))
    assert both, "no explained slot lists the duplicated rule"
    # one training batch, each row's own edge removed, every entity of every row: the
    # first batch where the removal changes a count (decided on the reference alone)
    for b in range(len(train_set)):
        all_h, all_r, _, _, etr = train_set[b]
        q = int(all_r[0])
        if (_reference_counts(g, rules, q, all_h.numpy(), etr.numpy())[1]
                != _reference_counts(g, rules, q, all_h.numpy(), None)[1]).any():
            break
    else:
        raise AssertionError("no training batch whose edge removal changes a path count")
    th, tr, te = all_h.to(dev), all_r.to(dev), etr.to(dev)
    ents = torch.arange(graph.entity_size, device=dev).unsqueeze(0).repeat(th.numel(), 1)
    want = _reference_explanations(g, rules, q, all_h.numpy(), etr.numpy(), ents.cpu().numpy())
    _check_explanations(model.explain_rows(th, tr, ents, edges_to_remove=te), want, (name, "train"))
    # and predict_topk takes the batch's edge removal
    top = model.predict_topk(th, tr, 5, edges_to_remove=te)
    with torch.no_grad():
        score, mask = model.forward_rows(th, tr, te)
    topk_ref.assert_equal([x.cpu().numpy() for x in top],
                          topk_ref.topk_ref(score.cpu().numpy(), mask.cpu().numpy(), None, None, 5), name)


def test_trainer_predict(dev, tmp_path):
    from rnnlogic_amd.data import ValidDataset
    from rnnlogic_amd.trainer import TrainerPredictor
    model = _model("plus_lstm_sum_bias", dev)[0]
    graph, train_set, test_set, _ = _env("umls")
    optim = torch.optim.Adam(model.parameters(), lr=0.005)
    solver = TrainerPredictor(model, train_set, ValidDataset(graph, 32), test_set, optim, gpus=[0])
    before = solver.evaluate("test")
    rng = torch.random.get_rng_state()
    path = str(tmp_path / "predictions.tsv")
    out = solver.predict("test", k=K, explain=3, output=path)
    assert torch.equal(torch.random.get_rng_state(), rng)
    assert solver.evaluate("test") == before
    n = len(out["h"])
    assert n == sum(len(b) for b in test_set.batches)
    assert out["index"].shape == (n, K) and out["score"].shape == (n, K) and out["valid"].shape == (n,)
    for i in range(n):
        where = np.nonzero(out["index"][i] == out["t"][i])[0]
        assert out["position"][i] == (where[0] if len(where) else -1)
    assert (out["position"] >= 0).any()
    assert len(out["explain_off"]) == 3 * n + 1 and out["explain_off"][-1] == len(out["explain_rule"])
    with open(path) as f:
        lines = [line.rstrip("\n").split("\t") for line in f]
    assert len(lines) == int(out["valid"].sum())
    at = 0
    for i in range(n):
        for j in range(int(out["valid"][i])):
            c = lines[at]
            at += 1
            assert graph.entity2id[c[0]] == out["h"][i] and graph.relation2id[c[1]] == out["r"][i]
            assert int(c[2]) == j + 1 and graph.entity2id[c[3]] == out["index"][i, j]
            assert np.float32(float(c[4])) == out["score"][i, j]
            assert (c[5] == "*") == (out["index"][i, j] == out["t"][i])
            a, b = out["explain_off"][[i * 3 + j, i * 3 + j + 1]] if j < 3 else (0, 0)
            assert len(c) == 6 + min(3, b - a)
            for pair in c[6:]:
                text, cnt = pair.rsplit(":", 1)
                hits = [s for s in range(a, b) if solver.rule_text(model.rules[out["explain_rule"][s]]) == text
                        and out["explain_count"][s] == int(cnt)]
                assert hits, pair
    # unfiltered lists hold the other known answers too
    plain = solver.predict("test", k=K, filtered=False)
    assert "explain_off" not in plain and (plain["index"] != out["index"]).any()
