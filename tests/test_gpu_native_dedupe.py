"""The overlapped RotatE forward (rnnl_predictorplus_forward_rotate) computes
duplicate (h, r) eval rows once: a row plan on the device, the forward over
the distinct keys written into each key's first row, and a copy to the
duplicates (csrc/dedupe.hip).  Every output — score, mask,
n_cand — is compared bitwise with the launch that computes every row
(rnnl_debug_dedupe(0))."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import Fixture

pytestmark = pytest.mark.gpu

_models, _graphs = {}, {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def graph_for(path):
    from rnnlogic_amd.data import KnowledgeGraph
    if path not in _graphs:
        _graphs[path] = KnowledgeGraph(path)
    return _graphs[path]


def model_for(case, dev):
    """(model, graph) of a golden case, or "umls_lstm_sum_rotate": UMLS with
    the SUM aggregator and RotatE (seeded weights; no fixture needed, the
    comparison is between two launches of the same model)."""
    from rnnlogic_amd import datasets
    from rnnlogic_amd.predictors import PredictorPlus
    if case not in _models:
        if case == "umls_lstm_sum_rotate":
            graph = graph_for(datasets.materialize("umls"))
            torch.manual_seed(0)
            model = PredictorPlus(graph, type="lstm", entity_feature="RotatE", aggregator="sum",
                                  embedding_path=datasets.rotate_path("umls"))
            model.set_rules(datasets.rule_file("umls"))
        else:
            fx = Fixture(case)
            graph = graph_for(fx.dataset_path())
            model = PredictorPlus(graph, embedding_path=fx.rotate_path(), **dict(fx.cfg["model"]))
            model.set_rules(fx.rule_path())
            sd = {k: torch.from_numpy(v) for k, v in fx.sd.items()}
            missing, unexpected = model.load_state_dict(sd, strict=False)
            assert not unexpected and all(k.startswith("RotatE.") for k in missing), (missing, unexpected)
        _models[case] = (model.to(dev).eval(), graph)
    return _models[case]


def run(model, h, r, dev, min_rows, etr=None, digest=False):
    """forward_rows with the native dedupe at `min_rows` (0: off, None: the
    default); numpy (score, mask, n_cand[, digest])."""
    from rnnlogic_amd import _native
    h = torch.as_tensor(np.asarray(h, dtype=np.int64)).to(dev)
    r = torch.as_tensor(np.asarray(r, dtype=np.int64)).to(dev)
    etr = torch.as_tensor(np.asarray(etr, dtype=np.int64)).to(dev) if etr is not None else None
    dig = torch.zeros(len(h), dtype=torch.int64, device=dev) if digest else None
    try:
        if min_rows is not None:
            _native.call("rnnl_debug_dedupe", min_rows)
        with torch.no_grad():
            out = model.forward_rows(h, r, etr, return_ncand=True, digest=dig)
        torch.cuda.synchronize()
    finally:
        _native.call("rnnl_debug_dedupe", -1)
    out = [x.cpu().numpy() for x in out]
    return out + [dig.cpu().numpy()] if digest else out


def assert_same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def split_form(model, n):
    """Whether a RotatE launch of n rows takes rotate_split_kernel +
    rotate_combine_kernel: the form is chosen by the row count alone (as
    test_rotate_split_form_is_bitwise selects it), and only the split form's
    workspace holds chunk sums beyond the 20-row h o r slabs."""
    from rnnlogic_amd import _native
    rot = model.RotatE
    need = ctypes.c_size_t()
    _native.call("rnnl_rotate_workspace_size", n, rot.num_entities, rot.emb_dim, int(rot.mode), ctypes.byref(need))
    hr = (n + 19) // 20 * rot.emb_dim * 2 * 20 * 4
    return need.value > (hr + 255) // 256 * 256


def distinct_rows(graph, n, seed=0):
    """n distinct (h, r) rows of the test split, in a seeded random order."""
    test = np.asarray(graph.test_facts, dtype=np.int64)[:, :2]
    _, first = np.unique(test[:, 1] * graph.entity_size + test[:, 0], return_index=True)
    rows = test[np.sort(first)]
    assert len(rows) >= n
    return rows[np.random.RandomState(seed).permutation(len(rows))[:n]]


def pattern(graph, name):
    d = distinct_rows(graph, 64)
    if name == "two_equal":  # nq = 2, nu = 1
        return d[[0, 0]]
    if name == "group_boundary_21":  # 20 distinct + a copy of row 0: past RotatE's 20-query group
        return d[list(range(20)) + [0]]
    if name == "batch_32":  # 31 distinct + a copy: one reference batch
        return d[list(range(31)) + [5]]
    if name == "one_key_41":  # multiplicity 41
        return d[[3] * 41]
    if name == "all_distinct_64":  # the identity path: no copy
        return d
    if name == "first_occurrence_last":  # a key seen only in the last row, duplicates before it
        return d[[0, 1, 0, 2, 1, 0, 7]]
    if name == "equal_h_or_r":  # equal h with different r, equal r with different h — not duplicates
        test = np.asarray(graph.test_facts, dtype=np.int64)[:, :2]
        a = test[0]
        same_h = test[(test[:, 0] == a[0]) & (test[:, 1] != a[1])]
        same_r = test[(test[:, 1] == a[1]) & (test[:, 0] != a[0])]
        other_r = same_h[0] if len(same_h) else np.array([a[0], (a[1] + 1) % graph.relation_size])
        rows = np.stack([a, other_r, same_r[0], a, other_r, same_r[0], a])
        assert len(np.unique(rows, axis=0)) == 3
        return rows
    if name == "sampled_3000":  # with replacement from the split
        test = np.asarray(graph.test_facts, dtype=np.int64)[:, :2]
        return test[np.random.RandomState(1).randint(0, len(test), 3000)]
    raise KeyError(name)


PATTERNS = ["two_equal", "group_boundary_21", "batch_32", "one_key_41", "all_distinct_64", "first_occurrence_last",
            "equal_h_or_r", "sampled_3000"]


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("case", ["umls_emb_pna_rotate", "umls_lstm_sum_rotate"])
def test_row_patterns_are_bitwise(case, name, dev):
    """The PNA case passes pieces = 2 (rotate_yield, the default), as
    evaluate() does; on UMLS's 135 entities every launch takes the split
    form, which has no yield point."""
    model, graph = model_for(case, dev)
    rows = pattern(graph, name)
    if case == "umls_emb_pna_rotate":
        assert model.rotate_yield
    nu = len(np.unique(rows, axis=0))
    if name in ("batch_32", "one_key_41"):  # few rows: split + combine, with and without the plan
        assert split_form(model, len(rows)) and split_form(model, nu)
    off = run(model, rows[:, 0], rows[:, 1], dev, 0)
    on = run(model, rows[:, 0], rows[:, 1], dev, 2)
    assert_same(off, on)
    assert off[1].all() and off[0].shape == (len(rows), graph.entity_size)


def test_overflow_retry_is_bitwise(dev):
    """Lowered capacities (as test_workspace_overflow_retry_is_bit_identical):
    the retry re-enters with a doubled capacity_scale and rebuilds the plan."""
    from rnnlogic_amd import _native
    model, graph = model_for("umls_lstm_sum_rotate", dev)
    test = np.asarray(graph.test_facts, dtype=np.int64)[:512, :2]
    rows = np.concatenate([test, test[:100]])
    want = run(model, rows[:, 0], rows[:, 1], dev, 0)
    _native.call("rnnl_debug_capacity", 1024, 1024, 64)
    try:
        model.capacity_scale = 1
        model._ws, model._ws_chunks = {}, {}
        got = run(model, rows[:, 0], rows[:, 1], dev, 2)
        retried = model.capacity_scale
    finally:
        _native.call("rnnl_debug_capacity", 0, 0, 0)
        model.capacity_scale = 1
        model._ws, model._ws_chunks = {}, {}
    assert retried > 1, "the lowered capacities did not overflow"
    assert_same(want, got)


@pytest.mark.parametrize("case", ["umls_emb_pna_rotate", "umls_lstm_sum_rotate"])
def test_not_applied_with_removed_edges_or_digest(case, dev):
    """Train-mode rows differ by their removed edge, and the digest is per
    row: both keep the plain launch."""
    model, graph = model_for(case, dev)
    train = np.asarray(graph.train_facts, dtype=np.int64)
    rel, cnt = np.unique(train[:, 1], return_counts=True)
    r0 = int(rel[np.argmax(cnt)])
    n_edges = int(cnt.max())
    assert n_edges >= 4
    heads = train[train[:, 1] == r0][:2, 0]
    h = np.array([heads[0]] * 4 + [heads[1]] * 3)
    r = np.full(len(h), r0)
    etr = np.array([0, 1, 0, 3, 2, 2, 1])
    assert_same(run(model, h, r, dev, 0, etr=etr), run(model, h, r, dev, 2, etr=etr))
    rows = pattern(graph, "sampled_3000")[:300]
    assert_same(run(model, rows[:, 0], rows[:, 1], dev, 0, digest=True),
                run(model, rows[:, 0], rows[:, 1], dev, 2, digest=True))


@pytest.mark.parametrize("case", ["umls_emb_pna_rotate", "umls_lstm_sum_rotate"])
def test_outputs_follow_the_key_in_any_row_order(case, dev):
    """The representatives are in first-occurrence order, so a shuffled copy
    of the same rows has another plan; every row's outputs are its key's."""
    model, graph = model_for(case, dev)
    rows = pattern(graph, "sampled_3000")[:700]
    perm = np.random.RandomState(2).permutation(len(rows))
    a = run(model, rows[:, 0], rows[:, 1], dev, 2)
    b = run(model, rows[perm, 0], rows[perm, 1], dev, 2)
    assert_same([x[perm] for x in a], b)
    key = rows[:, 1] * graph.entity_size + rows[:, 0]
    _, first, inv = np.unique(key, return_index=True, return_inverse=True)
    assert len(first) < len(rows)
    assert_same([x[first][inv] for x in a], a)  # a function of (h, r) only


def test_model_attribute_sets_the_minimum(dev):
    model, graph = model_for("umls_lstm_sum_rotate", dev)
    rows = pattern(graph, "one_key_41")
    off = run(model, rows[:, 0], rows[:, 1], dev, 0)
    try:
        model.native_dedupe_min = 2
        on = run(model, rows[:, 0], rows[:, 1], dev, None)
    finally:
        model.native_dedupe_min = None
    assert_same(off, on)


def test_fb_default_settings_are_bitwise(dev):
    """4,000 FB15k-237 test rows — above the default minimum, so this is the
    path evaluate() and the benchmark take."""
    model, graph = model_for("fb_lstm_sum_rotate", dev)
    test = np.asarray(graph.test_facts, dtype=np.int64)[:4000, :2]
    assert len(np.unique(test, axis=0)) < len(test)
    assert model.native_dedupe_min is None
    assert_same(run(model, test[:, 0], test[:, 1], dev, 0), run(model, test[:, 0], test[:, 1], dev, None))
