"""Rule bodies of up to five relations on the GPU (rnnl_rule_search_long,
rnnl_miner_set_rules_long; RuleMiner(max_body=4 | 5)) against the reference
miner's own pools (tests/golden/_rules_long_*.npz, tools/make_golden_rules_long.py)
and, for learn / H score / evaluation, against the fp64 restatements
tests/mine_ref.py and tests/mine_eval_ref.py, which are length-agnostic.

Pools: exact set and order equality.  Weights and H: the bounds of
tests/test_gpu_mine_learn.py (TOL_W, TOL_H), read from there.  Scores bitwise
and (num_g, num_ge) pairs exactly, as tests/test_gpu_mine_eval.py.
"""
import hashlib
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import mine_eval_ref
import mine_ref
from conftest import GOLDEN, REPO
from test_gpu_mine_learn import LR, TEMP, TOL_H, TOL_W, WD, flat_diff

pytestmark = pytest.mark.gpu

RANDOM = ["rand60", "sparse300", "dense40"]                 # no self-loop triples
CAPACITY = ["instar_2048", "instar_2049",                   # t's in-edges: staged in LDS / read from global memory
            "suffix_2048", "suffix_2049",                   # t's length-2 suffixes: sorted in LDS / edge by edge
            "set_over"]                                     # a triple with 3,902 rules of its own (dense40: 1,189)
GRAPHS = RANDOM + ["loops30"] + CAPACITY


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


_fx = {}


def fixture(name):
    """(graph, {4: pool, 5: pool}) of a _rules_long_ fixture; pools are [(head, body)] in the reference's order."""
    if name not in _fx:
        z = np.load(os.path.join(GOLDEN, "_rules_long_%s.npz" % name), allow_pickle=False)
        pools = {}
        for L in (4, 5):
            flat, rules, k = z["flat%d" % L].astype(np.int64).tolist(), [], 0
            while k < len(flat):
                rules.append((flat[k], tuple(flat[k + 2:k + 2 + flat[k + 1]])))
                k += 2 + flat[k + 1]
            pools[L] = rules
        graph = types.SimpleNamespace(train_facts=[tuple(int(x) for x in t) for t in z["triples"]],
                                      entity_size=int(z["E"]), relation_size=int(z["R"]))
        _fx[name] = (graph, pools)
    return _fx[name]


def long_miner(graph, dev, **attrs):
    from rnnlogic_amd.miner import RuleMiner
    miner = RuleMiner(graph, dev, max_body=5)
    for k, v in attrs.items():
        setattr(miner, k, v)
    return miner


# ------------------------------------------------------------- 1. the pools
@pytest.mark.parametrize("L", [4, 5])
@pytest.mark.parametrize("name", GRAPHS)
def test_search_matches_the_reference_pool(name, L, dev):
    """Same rules, same order; also after the table was too small and the
    search was retried, and with the suffixes of (almost) no tail kept in LDS."""
    graph, pools = fixture(name)
    want = pools[L]
    assert long_miner(graph, dev).search(L) == want
    small = long_miner(graph, dev, table_bits=10)
    assert small.search(L) == want
    assert small.table_bits > 10 or len(want) <= 512
    assert long_miner(graph, dev, suffix_cap=1).search(L) == want
    assert long_miner(graph, dev, suffix_cap=64).search(L) == want


def test_a_self_loop_triple_gives_one_rule_without_a_body(dev):
    graph, pools = fixture("loops30")
    assert (5, 0, 5) in graph.train_facts and (7, 1, 7) in graph.train_facts
    for L in (4, 5):
        got = long_miner(graph, dev).search(L)
        assert [r for r in got if not r[1]] == [(0, ()), (1, ())] and got == pools[L]
    alone = types.SimpleNamespace(train_facts=[(2, 1, 2), (2, 0, 3), (3, 0, 2)], entity_size=4, relation_size=2)
    assert long_miner(alone, dev).search(4) == [(1, ())]  # nothing is walked from (2, 1, 2)


def test_umls_at_length_4(dev):
    """501,799 rules; compared as arrays: counts per length and the digest of
    the reference's flat (head, len, body...) int32 stream."""
    from rnnlogic_amd import datasets
    from rnnlogic_amd.data import KnowledgeGraph
    from rnnlogic_amd.miner import unpack_long
    z = np.load(os.path.join(GOLDEN, "_rules_long_umls_L4.npz"), allow_pickle=False)
    graph = KnowledgeGraph(datasets.materialize("umls"))
    keys = np.sort(long_miner(graph, dev).search_keys(4))
    assert len(keys) == int(z["count"]) == 501799
    head, ln, body = unpack_long(keys, graph.relation_size, 4)
    assert np.bincount(ln, minlength=5).tolist() == [0] + z["per_len"].tolist()
    rows = np.concatenate([head[:, None], ln[:, None].astype(np.int64), body.astype(np.int64)], 1).astype(np.int32)
    used = np.arange(6)[None, :] < (2 + ln)[:, None]
    assert hashlib.sha256(rows[used].tobytes()).hexdigest() == str(z["sha256"])


@pytest.mark.parametrize("name", RANDOM)
def test_short_rules_of_the_long_search_are_the_short_search(name, dev):
    """Without self-loop triples, search(5) up to length 3 is search(3) of the untouched kernel."""
    from rnnlogic_amd.miner import RuleMiner
    graph, pools = fixture(name)
    assert RuleMiner.max_body == 3
    short = RuleMiner(graph, dev).search(3)
    assert len(short) > 300 and max(len(b) for _, b in short) == 3
    assert [r for r in long_miner(graph, dev).search(5) if len(r[1]) <= 3] == short
    assert long_miner(graph, dev).search(3) == short  # the same entry point, whatever max_body
    with pytest.raises(ValueError):
        RuleMiner(graph, dev).search(4)


def test_search_repeats(dev):
    graph, pools = fixture("rand60")
    miner = long_miner(graph, dev)
    a, b = np.sort(miner.search_keys(5)), np.sort(miner.search_keys(5))
    assert a.dtype == np.uint64 and len(a) == len(pools[5]) and np.array_equal(a, b)


def test_more_relations_than_a_key_of_five_holds(dev):
    from rnnlogic_amd import _native
    tri = [(0, 1024, 1), (0, 5, 2), (2, 6, 3), (3, 7, 4), (4, 1000, 1), (2, 1023, 1)]
    graph = types.SimpleNamespace(train_facts=tri, entity_size=5, relation_size=1025)
    miner = long_miner(graph, dev)
    with pytest.raises(_native.NativeError) as err:
        miner.search(5)
    assert err.value.code == _native.RNNL_ERR_INVALID and "1024" in str(err.value) and "1025" in str(err.value)
    assert miner.search(4) == [(1023, (6, 7, 1000)), (1024, (5, 1023)), (1024, (5, 6, 7, 1000))]


def test_table_past_the_budget_is_an_error(dev):
    graph, pools = fixture("rand60")
    miner = long_miner(graph, dev, table_bits=10, budget_bytes=1 << 17)  # 32,465 rules need 2 x 2^16 slots
    with pytest.raises(RuntimeError) as err:
        miner.search(5)
    assert "budget_bytes" in str(err.value)


# --------------------------------------- 2. weights, H scores and evaluation
def mixed_rules(name, per_length=3):
    """Per relation a list mixing lengths 0..5 from the reference's pool; the
    first four rules of relation 0 have lengths 5, 1, 4, 0 (one round of the
    evaluation kernel's four waves), and one body is there twice."""
    graph, pools = fixture(name)
    R = graph.relation_size
    rules = []
    for r in range(R):
        mine = [x for x in pools[5] if x[0] == r]
        pick = []
        for n in (5, 1, 4, 2, 3):
            of_n = [x for x in mine if len(x[1]) == n]
            pick += of_n[::max(1, len(of_n) // per_length)][:per_length]
        rules.append(pick)
    first = {n: next(x for x in rules[0] if len(x[1]) == n) for n in (5, 1, 4)}
    rules[0] = [first[5], first[1], first[4], (0, ())] + rules[0] + [first[5]]
    assert [len(b) for _, b in rules[0][:4]] == [5, 1, 4, 0]
    assert sorted(set(len(b) for rs in rules for _, b in rs)) == [0, 1, 2, 3, 4, 5]
    return graph, rules


def run_both(dev, graph, rules, priors, order, fast, top_k, portion, prior_weight, chunk=None):
    tri, E, R = graph.train_facts, graph.entity_size, graph.relation_size
    miner = long_miner(graph, dev, chunk_triples=chunk)
    miner.set_logic_rules(rules, priors)
    miner.learn(LR, WD, TEMP, fast=fast, portion=portion, order=order)
    miner.h_score(top_k, 1.0, prior_weight, portion=portion)
    ref = mine_ref.MineRef(tri, E, R)
    ref.set_logic_rules(rules, priors)
    n_used = int(len(tri) * portion)
    ref.learn(order, n_used, LR, WD, TEMP, fast)
    ref.h_score(order, n_used, top_k, 1.0, prior_weight)
    return miner.weights(), miner.H(), ref.weights(), ref.H


@pytest.mark.parametrize("name,fast,top_k,portion,prior_weight", [
    ("loops30", False, 0, 1.0, 0.0), ("loops30", True, 2, 0.5, 0.7), ("rand60", True, 0, 0.5, 0.0)])
def test_learn_and_h_score_with_bodies_of_every_length(dev, name, fast, top_k, portion, prior_weight):
    graph, rules = mixed_rules(name)
    priors = [[0.1 * k - 0.3 for k in range(len(rs))] for rs in rules]
    order = np.random.default_rng(1).permutation(len(graph.train_facts)).astype(np.int32)
    w, H, rw, rH = run_both(dev, graph, rules, priors, order, fast, top_k, portion, prior_weight)
    long_ones = [(r, k) for r, rs in enumerate(rules) for k, (_, b) in enumerate(rs) if len(b) >= 4]
    assert any(abs(rw[r][k]) > 1e-4 for r, k in long_ones)  # the long bodies ground and learn
    print("%s: |dwt| %.3g |dH| %.3g" % (name, flat_diff(w, rw), flat_diff(H, rH)))
    assert flat_diff(w, rw) <= TOL_W and flat_diff(H, rH) <= TOL_H


def test_chunking_is_bitwise_neutral(dev):
    graph, rules = mixed_rules("loops30")
    order = np.random.default_rng(3).permutation(len(graph.train_facts)).astype(np.int32)
    runs = [run_both(dev, graph, rules, None, order, False, 0, 1.0, 0.0, chunk=c)[:2] for c in (1, 7, None)]
    assert any(np.any(x != 0.0) for x in runs[0][0])
    for w, H in runs[1:]:
        assert all(np.array_equal(x, y) for x, y in zip(w, runs[0][0]))
        assert all(np.array_equal(x, y) for x, y in zip(H, runs[0][1]))


def test_short_lists_do_not_depend_on_the_entry_point(dev):
    """Rule lists of length <= 3 through rnnl_miner_set_rules (n x 3) and
    through rnnl_miner_set_rules_long (n x 5): the same bits."""
    from rnnlogic_amd.miner import RuleMiner
    graph, rules = mixed_rules("loops30")
    rules = [[x for x in rs if len(x[1]) <= 3] for rs in rules]
    order = np.random.default_rng(5).permutation(len(graph.train_facts)).astype(np.int32)
    out = []
    for miner in (RuleMiner(graph, dev), long_miner(graph, dev)):
        miner.set_logic_rules(rules)
        miner.learn(LR, WD, TEMP, order=order)
        miner.h_score(0)
        out.append((miner.weights(), miner.H(), miner.scores(graph.train_facts[:40]).cpu().numpy()))
    assert any(np.any(x != 0.0) for x in out[0][0]) and out[0][2].any()
    assert all(np.array_equal(x, y) for x, y in zip(out[0][0], out[1][0]))
    assert all(np.array_equal(x, y) for x, y in zip(out[0][1], out[1][1]))
    assert np.array_equal(out[0][2], out[1][2])


def test_mine_at_length_4_replays_the_restatement(dev):
    graph, pools = fixture("loops30")
    tri, E, R = graph.train_facts, graph.entity_size, graph.relation_size
    miner = long_miner(graph, dev)
    rng = np.random.default_rng(11)
    pool = [[x for x in pools[4] if x[0] == r] for r in range(R)]
    orders = [rng.permutation(len(tri)).astype(np.int32) for _ in range(2)]
    sels = [[np.sort(rng.permutation(len(pool[r]))[:25]).tolist() for r in range(R)] for _ in range(2)]
    out = miner.mine(4, 2, 25, 0, LR, WD, TEMP, 0, orders=orders, selections=sels)
    assert miner.get_logic_rules() == pool and any(len(b) == 4 for _, b, _ in out)
    H, wt = mine_ref.mine_replay(tri, E, R, pool, orders, sels, LR, WD, TEMP, 0)
    dH, dw = flat_diff(miner.pool_H, H), flat_diff(miner.weights(), wt)
    print("mine(4): |dH| %.3g |dwt| %.3g" % (dH, dw))
    assert dH <= TOL_H and dw <= TOL_W
    assert sorted(len(b) for _, b, _ in out) == sorted(len(b) for _, b in pools[4])


def quantised_weights(rules, seed):
    rng = np.random.default_rng(seed)
    return [[float(x) for x in rng.choice([0.0, 0.5, 0.5, -0.25, 0.1, 1e-3, -1.7], len(rs))] for rs in rules]


@pytest.mark.parametrize("name", ["loops30", "rand60", "suffix_2048"])
def test_evaluation_with_bodies_of_every_length(dev, name):
    """scores bitwise, pairs exactly, filtered and not.  loops30 and rand60
    hold their arrays in LDS (E <= 512), suffix_2048 (E = 2,098) in global memory."""
    if name == "suffix_2048":
        graph, pools = fixture(name)
        rules = [[x for x in pools[5] if x[0] == r] for r in range(graph.relation_size)]
        rules[0] = sorted(rules[0], key=lambda x: -len(x[1])) + [(0, ()), (0, (1,))]
        queries = [t for t in graph.train_facts if t[0] in (1, 2, 3)] + [(1, 0, 7), (2, 0, 0)]
    else:
        graph, rules = mixed_rules(name)
        queries = graph.train_facts[:60] + [(h, 0, t) for h in range(6) for t in (0, 5)]
    tri, E, R = graph.train_facts, graph.entity_size, graph.relation_size
    weights = quantised_weights(rules, 1)
    miner = long_miner(graph, dev)
    miner.set_logic_rules(rules)
    miner.set_weights(weights)
    ref = mine_eval_ref.MineEvalRef(tri, E, R)
    ref.set_rules(rules, weights)
    want = np.asarray([ref.scores(*q) for q in queries], dtype=np.float64).reshape(len(queries), E)
    got = miner.scores(queries).cpu().numpy()
    assert want.any() and np.array_equal(got, want)
    for filtered in (True, False):
        pairs = miner.eval_ranks(queries, filtered=filtered)
        assert np.array_equal(pairs, np.asarray(ref.pairs(queries, filtered), dtype=np.int64).reshape(-1, 2))
    m = miner.evaluate(triples=queries)
    assert tuple(m[k] for k in mine_eval_ref.METRIC_NAMES) == mine_eval_ref.metrics(ref.pairs(queries), E)


def test_path_count_past_32_bits_on_a_chain_of_five(dev):
    """100 parallel edges on each of five hops: 10^10 > 2^32 paths.  RNNL_ERR_RANGE from
    learn and from the evaluation; four hops (10^8) fit."""
    from rnnlogic_amd import _native
    tri = [(0, 0, 5)] + [(i, 1, i + 1) for i in range(5) for _ in range(100)]
    graph = types.SimpleNamespace(train_facts=tri, entity_size=6, relation_size=2)
    miner = long_miner(graph, dev)
    order = np.arange(len(tri), dtype=np.int32)
    miner.set_logic_rules([[(0, (1, 1, 1, 1, 1))], []])
    miner.set_weights([[0.5], []])
    with pytest.raises(_native.NativeError) as err:
        miner.learn(LR, WD, TEMP, order=order)
    assert err.value.code == _native.RNNL_ERR_RANGE
    with pytest.raises(_native.NativeError) as err:
        miner.eval_ranks([(0, 0, 5)])
    assert err.value.code == _native.RNNL_ERR_RANGE
    miner.set_logic_rules([[(0, (1, 1, 1, 1))], []])
    miner.set_weights([[0.5], []])
    assert miner.scores([(0, 0, 5)]).cpu().numpy().tolist() == [[0.0, 0.0, 0.0, 0.0, 0.5 * 1e8, 0.0]]
    miner.learn(LR, WD, TEMP, fast=True, order=order)
    assert abs(miner.weights()[0][0] - (0.5 - LR)) < 1e-12  # one destination, not the tail: Adam's first step is -lr


# ------------------------------------------------------------ 3. command line
def write_dataset(path, graph, valid, test):
    os.makedirs(path)
    with open(os.path.join(path, "entities.dict"), "w") as fo:
        fo.writelines("%d\te%d\n" % (e, e) for e in range(graph.entity_size))
    with open(os.path.join(path, "relations.dict"), "w") as fo:
        fo.writelines("%d\tr%d\n" % (r, r) for r in range(graph.relation_size))
    for name, triples in (("train.txt", graph.train_facts), ("valid.txt", valid), ("test.txt", test)):
        with open(os.path.join(path, name), "w") as fo:
            fo.writelines("e%d\tr%d\te%d\n" % t for t in triples)


def run_cli(args, cwd):
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "rnnlogic_amd.miner"] + args, check=True, env=env, cwd=str(cwd),
                          timeout=300, capture_output=True, text=True).stdout.splitlines()


def test_command_line_round_trip_at_length_4(dev, tmp_path):
    """-max-length 4 writes bodies of four relations and evaluates what it
    learned, as the API does; -rule-file takes that file (a default miner
    refuses it) and prints what the API says of the same file."""
    from rnnlogic_amd.data import KnowledgeGraph
    from rnnlogic_amd.miner import RuleMiner, metrics_line
    graph, pools = fixture("rand60")
    E, R = graph.entity_size, graph.relation_size
    held = [(h, r, (t + 7) % E) for h, r, t in graph.train_facts[:80]]
    data = str(tmp_path / "data")
    write_dataset(data, graph, held[:40], held[40:])
    args = ["-data-path", data, "-max-length", "4", "-iterations", "1", "-lr", str(LR), "-wd", str(WD), "-temp",
            str(TEMP), "-top-k", "0", "-top-n", "40", "-top-n-out", "0", "-output-file", str(tmp_path / "cli.txt")]
    mined = run_cli(args + ["-evaluate", "both"], tmp_path)
    kg = KnowledgeGraph(data)
    api = RuleMiner(kg, dev, max_body=4)
    api.mine(4, 1, 40, 0, LR, WD, TEMP, 0, seed=0)
    n = api.out_rules(str(tmp_path / "api.txt"), 0)
    assert n == len(pools[4]) and (tmp_path / "cli.txt").read_bytes() == (tmp_path / "api.txt").read_bytes()
    assert mined[-3:] == ["#Rules written: %d" % n, metrics_line("Valid", api.evaluate("valid")),
                          metrics_line("Test", api.evaluate("test"))]
    lines = (tmp_path / "cli.txt").read_text().splitlines()
    assert sum(1 for ln in lines if len(ln.split()) == 6) == sum(1 for _, b in pools[4] if len(b) == 4) > 1000
    with pytest.raises(ValueError):
        RuleMiner(kg, dev).read_rules(str(tmp_path / "cli.txt"))
    again = RuleMiner(kg, dev, max_body=5)
    assert again.read_rules(str(tmp_path / "cli.txt")) == n
    read = run_cli(["-data-path", data, "-rule-file", str(tmp_path / "cli.txt"), "-evaluate", "both"], tmp_path)
    assert read[-3:] == ["#Rules read: %d" % n, metrics_line("Valid", again.evaluate("valid")),
                         metrics_line("Test", again.evaluate("test"))]
