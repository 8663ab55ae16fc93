"""The training lookahead driven by hand (prefetch / forward / check_deferred,
DESIGN §3.11) on kinship: which queued groundings a forward takes, drops and
counts, and that the scores, masks and gradients are those of the one-call
forward (prefetch_depth 0)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def kinship(dev):
    """(graph, rule file, three single-relation train batches of 8, 5 and 7
    rows as (all_h, all_r, edges_to_remove) on the device)."""
    from rnnlogic_amd import datasets
    from rnnlogic_amd.data import KnowledgeGraph, TrainDataset
    from rnnlogic_amd.utils import set_seed
    set_seed(5)
    graph = KnowledgeGraph(datasets.materialize("kinship"))
    train_set = TrainDataset(graph, 8)
    batches, seen = [], set()
    for rows in (8, 5, 7):  # one batch each of three relations
        idx = next(i for i, b in enumerate(train_set.batches) if len(b) == 8 and b[0][1] not in seen)
        seen.add(train_set.batches[idx][0][1])
        b = train_set[idx]
        batches.append(tuple(b[j][:rows].to(dev) for j in (0, 1, 4)))
    return graph, datasets.rule_file("kinship"), batches


def _make(which, graph, rules, dev):
    from rnnlogic_amd.predictors import Predictor, PredictorPlus
    torch.manual_seed(11)
    if which == "predictor":
        model = Predictor(graph, entity_feature="bias")
        model.set_rules(rules)
        with torch.no_grad():
            model.rule_weights.normal_(std=0.1)
            model.bias.normal_(std=0.1)
    else:
        model = PredictorPlus(graph, type="emb", hidden_dim=16, aggregator="sum", entity_feature="bias")
        model.set_rules(rules)
        with torch.no_grad():
            model.bias.normal_(std=0.1)
    return model.to(dev).train()


def _step(model, batch):
    """(score, mask, {name: gradient or None}) of forward + sum().backward()."""
    model.zero_grad(set_to_none=True)
    score, mask = model(*batch)
    score.sum().backward()
    grads = {n: (p.grad.detach().clone() if p.grad is not None else None) for n, p in model.named_parameters()}
    return score.detach().clone(), mask.clone(), grads


def _run(model, depth, A, B, C):
    """The steps with `depth`: prefetch A, B (and C, refused: the queue is
    full), forward B (A is dropped), forward C (never queued: the one-call
    path), check_deferred.  Returns (B's results, C's results)."""
    model.prefetch_depth = depth
    model.prefetch_dropped, model.prefetch_hits = 0, 0
    for batch in (A, B, C):
        model.prefetch(*batch)
    out = _step(model, B), _step(model, C)
    model.check_deferred()
    torch.cuda.synchronize()
    return out


def _compare(which, got, want, exact):
    for name, (s1, m1, g1), (s0, m0, g0) in zip("BC", got, want):
        assert torch.equal(m1, m0), (which, name)
        print("%s %s: max |score - one-call score| = %.3g" % (which, name, float((s1 - s0).abs().max())))
        for n in g0:
            if g0[n] is not None:
                print("%s %s: grad %s max |diff| = %.3g (max |grad| %.3g)" % (
                    which, name, n, float((g1[n] - g0[n]).abs().max()), float(g0[n].abs().max())))
        if exact:
            assert torch.equal(s1, s0), (which, name)
        else:
            torch.testing.assert_close(s1, s0, rtol=0, atol=1e-6)
        for n in g0:
            assert (g1[n] is None) == (g0[n] is None), (which, name, n)
            if g0[n] is None:
                continue
            if exact:
                assert torch.equal(g1[n], g0[n]), (which, name, n)
            else:
                torch.testing.assert_close(g1[n], g0[n], rtol=1e-5, atol=1e-7, msg="%s %s %s" % (which, name, n))


@pytest.mark.parametrize("which", ["predictor", "plus"])
def test_lookahead_by_hand(which, kinship, dev):
    """Two groundings queued, a third refused, the second one's forward: one
    drop, one hit; the rows that were never queued take the one-call path.
    Scores, masks and parameter gradients against prefetch_depth 0:
    Predictor bit-equal; PredictorPlus bit-equal as well — the comparison
    run on the commit before the lookahead became an object of its own gave
    max |diff| 0 for both batches' scores and every gradient, so bit-equality
    is what is asserted (not the rtol 0 / atol 1e-6 scores and rtol 1e-5 /
    atol 1e-7 gradients that would have applied otherwise).  After set_rules
    a queued grounding is gone: its rows' forward counts no hit."""
    graph, rules, (A, B, C) = kinship
    model = _make(which, graph, rules, dev)
    want = _run(model, 0, A, B, C)
    assert (model.prefetch_dropped, model.prefetch_hits) == (0, 0)
    got = _run(model, 2, A, B, C)
    assert (model.prefetch_dropped, model.prefetch_hits) == (1, 1)
    _compare(which, got, want, exact=True)

    model.prefetch(*A)
    model.set_rules(rules)
    model = model.to(dev).train()
    model(*A)
    model.check_deferred()
    torch.cuda.synchronize()
    assert model.prefetch_hits == 1
