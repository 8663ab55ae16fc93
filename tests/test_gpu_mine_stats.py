"""Support, body size and PCA body size of rules on the GPU —
RuleMiner.rule_stats / pool_stats / head_pairs / confidence, the filters of
best_rules / out_rules, out_rule_stats, mine(prior=...) and the command line
(rnnl_miner_rule_stats, csrc/mine_stats.hip) — against the two restatements of
tests/mine_stats_ref.py: (a) boolean matrices and fp32 matmuls, (b) a set walk.

The counts are integers and are compared with np.array_equal.  The one
tolerance is TOL_H of test_gpu_mine_learn.py for the H scores of
mine(prior='pca'), which differ from the restatement in libm's exp only.
"""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import mine_ref
import mine_stats_ref as ms
from conftest import REPO

pytestmark = pytest.mark.gpu

TOL_H = 7.72e-15  # test_gpu_mine_learn.py
LR, WD, TEMP = 0.01, 0.0005, 100.0
KEYS = ("support", "body", "pca_body")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


_graphs, _dense = {}, {}


def real_graph(data):
    if data not in _graphs:
        from rnnlogic_amd import datasets
        from rnnlogic_amd.data import KnowledgeGraph
        _graphs[data] = KnowledgeGraph(datasets.materialize(data))
    return _graphs[data]


def real_dense(data):
    if data not in _dense:
        g = real_graph(data)
        _dense[data] = ms.DenseStats(g.train_facts, g.entity_size, g.relation_size)
    return _dense[data]


def fake_graph(triples, E, R, **more):
    return types.SimpleNamespace(train_facts=[tuple(t) for t in triples], entity_size=E, relation_size=R, **more)


def assert_same(got, want):
    for k in KEYS:
        assert len(got[k]) == len(want[k])
        for r, (a, b) in enumerate(zip(got[k], want[k])):
            assert a.dtype == np.int64 and np.array_equal(a, b), (k, r, a[:8], b[:8])


def check(dev, triples, E, R, rules, ref=None, max_body=5, **kw):
    from rnnlogic_amd.miner import RuleMiner
    miner = RuleMiner(fake_graph(triples, E, R), dev, max_body=max_body)
    ref = ref or ms.DenseStats(triples, E, R)
    want = ms.stats_of(ref, rules)
    got = miner.rule_stats(rules, **kw)
    assert_same(got, want)
    assert np.array_equal(miner.head_pairs(), ref.head_pairs())
    return miner, got, want


# ------------------------------------------------------------- 1. tiny graph
# the graph of test_gpu_mine_eval.py: relation 2 has triples but no rules there,
# relation 3 rules but no triples; (0,0,1) is there twice; (2,0,2) is a self-loop
TINY = [(0, 0, 1), (0, 0, 1), (2, 0, 2), (0, 0, 5), (6, 0, 7), (0, 1, 3), (0, 1, 4), (3, 1, 5), (4, 1, 5), (1, 1, 5),
        (5, 2, 0), (5, 2, 1), (3, 2, 4), (0, 1, 1), (2, 1, 2), (1, 0, 5), (7, 2, 6), (5, 1, 3)]
# its rule lists, plus: empty bodies, the body (1, 1) under three heads, (0, (1, 1)) listed twice
TINY_RULES = [
    [(0, ()), (0, (1,)), (0, (1, 1)), (0, (1, 2, 1)), (0, (0,)), (0, (1, 1)), (0, (0, 1)), (0, (1, 1, 2)), (0, (3,))],
    [(1, (0,)), (1, (1, 1)), (1, (0, 1)), (1, (1, 2, 0)), (1, ())],
    [(2, (1, 1))],
    [(3, (1,)), (3, (0, 1)), (3, ())],
]


def test_tiny_graph(dev):
    miner, got, _ = check(dev, TINY, 8, 4, TINY_RULES, max_body=3)
    assert (got["support"][0][0], got["body"][0][0], got["pca_body"][0][0]) == (1, 8, 4)  # 0 <- (): the self-loop
    assert (got["support"][0][1], got["body"][0][1], got["pca_body"][0][1]) == (3, 8, 5)
    assert got["support"][0][2] == got["support"][0][5] and got["pca_body"][0][2] == got["pca_body"][0][5]  # the copy
    assert got["body"][0][2] == got["body"][1][1] == got["body"][2][0] > 0  # one body, three heads
    assert got["support"][3].tolist() == [0, 0, 0] and got["pca_body"][3].tolist() == [0, 0, 0]
    assert got["body"][3].tolist()[0] == 8 and miner.head_pairs().tolist() == [5, 8, 4, 0]
    # the current lists of set_logic_rules are the default
    miner.set_logic_rules(TINY_RULES)
    assert_same(miner.rule_stats(), got)
    hp = miner.head_pairs()
    for kind in ("std", "pca", "head_coverage"):
        for pc in (0.0, 1.5):
            conf = miner.confidence(kind, pc)
            for r in range(4):
                want = ms.confidence(kind, got["support"][r], got["body"][r], got["pca_body"][r], hp[r],
                                     pc if kind != "head_coverage" else 0.0)
                assert conf[r].dtype == np.float64 and np.array_equal(conf[r], want)
    assert miner.confidence("head_coverage")[3].tolist() == [0.0, 0.0, 0.0]  # 0 / 0
    with pytest.raises(ValueError):
        miner.confidence("amie")
    with pytest.raises(ValueError):
        miner.rule_stats([[(0, (4,))], [], [], []])
    with pytest.raises(ValueError):
        miner.rule_stats([[(0, (1, 1, 1, 1, 1, 1))], [], [], []])
    assert_same(miner.rule_stats([[], [], [], []]), dict((k, [np.zeros(0, np.int64)] * 4) for k in KEYS))


def test_native_entry_checks_its_arguments(dev):
    import ctypes

    from rnnlogic_amd import _native
    from rnnlogic_amd.miner import RuleMiner
    miner = RuleMiner(fake_graph(TINY, 8, 4), dev)
    work = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    out = torch.zeros(64, dtype=torch.int64, device=dev)
    cnt = torch.zeros(4, dtype=torch.int64, device=dev)

    def call(ln, body, off, heads, work_bytes=1 << 16):
        arr = [np.ascontiguousarray(x, dtype=np.int32) for x in (ln, body, off, heads)]
        _native.call("rnnl_miner_rule_stats", miner._handle, len(ln), arr[0].ctypes.data, arr[1].ctypes.data,
                     arr[2].ctypes.data, arr[3].ctypes.data, 0, 0, work.data_ptr(), work_bytes, out.data_ptr(),
                     cnt.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)

    call([1, 2], [[1, 0, 0, 0, 0], [1, 1, 0, 0, 0]], [0, 1, 3], [0, 0, 2])
    torch.cuda.synchronize()
    for bad in (([6], [[0] * 5], [0, 1], [0]), ([-1], [[0] * 5], [0, 1], [0]), ([1], [[4, 0, 0, 0, 0]], [0, 1], [0]),
                ([1], [[0] * 5], [0, 1], [4]), ([1], [[0] * 5], [0, 2], [1, 1]), ([1], [[0] * 5], [0, 2], [2, 1]),
                ([1, 1], [[0] * 5] * 2, [0, 2, 1], [0, 1]), ([1], [[0] * 5], [1, 2], [0, 1])):
        with pytest.raises(_native.NativeError) as err:
            call(*bad)
        assert err.value.code == _native.RNNL_ERR_INVALID
    with pytest.raises(_native.NativeError):
        call([1], [[0] * 5], [0, 1], [0], work_bytes=16)
    nbytes = ctypes.c_size_t()
    _native.call("rnnl_miner_rule_stats_scratch", miner._handle, 2, 3, 0, ctypes.byref(nbytes))
    assert 256 <= nbytes.value <= 1 << 16  # 8 entities: the walk's arrays are LDS


# ------------------------- 2. frontiers and destination sets across the widths
def hub_graph(degrees):
    """One hub per degree: hub -0-> its own neighbours -1-> a few shared
    targets and back to the hubs -2-> ...; relation 3 holds the facts the rules
    are asked about."""
    H = len(degrees)
    E = H + sum(degrees) + 9
    tri, nxt = [], H
    first_target = H + sum(degrees)
    for i, deg in enumerate(degrees):
        for j in range(deg):
            n = nxt + j
            tri.append((i, 0, n))
            tri.append((n, 1, first_target + (j % 7)))
            if j % 3 == 0:
                tri.append((n, 1, (i + 1) % H))
            if j % 5 == 0:
                tri.append((n, 3, first_target + 1))
            if j == deg - 1:
                tri.append((i, 3, n))  # the last neighbour is a known tail of the hub
        tri += [(i, 3, first_target + 2), (i, 2, first_target + 8), (i, 3, i), (i, 0, nxt)]  # one edge twice
        nxt += deg
    tri += [(first_target + k, 2, k % H) for k in range(7)] + [(first_target + 8, 2, first_target + 8)]
    return tri, E, 4


HUB_RULES = [
    [(0, (0,)), (0, (2, 0)), (0, (0, 1, 2))],
    [(1, (0, 1))],
    [(2, (0, 1)), (2, (0, 1, 2, 0))],
    [(3, ()), (3, (0,)), (3, (0, 1)), (3, (0, 1, 0)), (3, (0, 1, 2)), (3, (0, 1, 2, 0)), (3, (0, 1, 2, 0, 1)),
     (3, (2, 2, 2, 2, 2)), (3, (1, 2, 0, 1, 0)), (3, (0, 1, 0, 1))],
]


@pytest.mark.parametrize("degrees", [(63, 64, 65, 300), (15, 16, 17, 1)])
def test_hubs_across_the_lane_and_workgroup_widths(dev, degrees):
    """Out-degrees around the 64 lanes of a wave and past the 256 threads of a
    workgroup; 15 / 16 / 17 lie around the frontier size at which the walk
    goes from one entity's run per step to one entity per lane."""
    tri, E, R = hub_graph(degrees)
    _, got, _ = check(dev, tri, E, R, HUB_RULES)
    assert got["body"][3][1] == sum(degrees)  # the doubled edge counts once
    assert got["support"][3][1] == len(degrees)  # each hub's last neighbour
    assert got["body"][3][6] > 0 and got["support"][3][0] == len(degrees)


def test_complete_graph_every_entity_is_a_destination(dev):
    E = 40
    tri = [(h, 0, t) for h in range(E) for t in range(E)] + [(h, 1, (h * 7 + 3) % E) for h in range(0, E, 2)]
    rules = [[(0, (0,)), (0, (0, 0, 0, 0)), (0, (0, 0, 0, 0, 0)), (0, (1, 0, 1))],
             [(1, (0,)), (1, (0, 0, 0, 0, 0)), (1, (1, 0, 0, 0)), (1, (0, 0, 0, 1)), (1, (1, 1, 1, 1))]]
    _, got, _ = check(dev, tri, E, 2, rules)
    assert got["body"][0][:3].tolist() == [E * E] * 3 and got["support"][0][:3].tolist() == [E * E] * 3
    assert got["support"][1][1] == E // 2 and got["pca_body"][1][1] == E * E // 2


# ----------------------------------------- 3. both sides of every capacity
@pytest.mark.parametrize("E", [1023, 1024, 1025])
def test_entities_in_lds_and_in_global_memory(dev, E):
    """1,024 entities are the most whose stamps and frontier lists are LDS;
    from 1,025 on they are the caller's global scratch."""
    R = 3
    tri = ms.random_graph(E, E, R, 5 * E)
    tri += [(E - 1, 0, 0), (0, 1, E - 1), (E - 1, 2, E - 1), (E - 2, 0, E - 1), (0, 0, E - 2)]
    rules = ms.random_rules(7, R, 30, 5)
    rules[0] += [(0, (1, 2)), (0, (0, 0, 0, 0, 0))]
    assert 30 <= sum(len(x) for x in rules) <= 80
    _, got, _ = check(dev, tri, E, R, rules, ref=ms.SetStats(tri, E, R))
    assert got["body"][0][-1] > E and got["support"][0][-1] > 0  # five hops reach most of the graph


@pytest.mark.parametrize("n_heads", [127, 128, 129, 131])
def test_more_heads_of_one_body_than_the_lds_sums_hold(dev, n_heads):
    """128 heads of a body are summed in LDS; the 129th and later add to global memory directly."""
    R, E = 131, 24
    rng = np.random.default_rng(n_heads)
    tri = [(int(h), int(r), int(t)) for h, r, t in zip(rng.integers(0, E, 900), rng.integers(0, R, 900),
                                                       rng.integers(0, E, 900))]
    tri += [(h, 0, (h + 1) % E) for h in range(E)] + [(h, 1, (h * 5) % E) for h in range(E)]
    tri += [(r % E, r, (5 * (r % E + 1)) % E) for r in range(120, R)]  # the last heads predict something
    rules = [[(r, (0, 1)), (r, (1,))] if r < n_heads else [(r, (2, 0))] for r in range(R)]
    _, got, _ = check(dev, tri, E, R, rules)
    assert sum(int(got["support"][r][0]) for r in range(n_heads)) > 0
    assert any(got["support"][r][0] > 0 for r in range(n_heads - 3, n_heads))


@pytest.mark.parametrize("E", [255, 256, 257])
def test_sources_of_one_item_around_the_workgroup_size(dev, E):
    """From 4,096 distinct bodies on an item is a body and up to 256 sources, one
    per thread of the workgroup: 257 entities make a second item per body."""
    R = 6
    tri = ms.random_graph(E + 1, E, R, 3 * E) + [(E - 1, r, (r * 11) % E) for r in range(R)] + [(0, 0, E - 1)]
    bodies = [()]
    for ln in range(1, 5):
        bodies += [tuple(int(x) for x in np.unravel_index(i, (R,) * ln)) for i in range(R ** ln)]
    rng = np.random.default_rng(3)
    bodies += [tuple(int(x) for x in np.unravel_index(int(i), (R,) * 5)) for i in rng.choice(R ** 5, 2700, False)]
    assert len(set(bodies)) == len(bodies) >= 4096
    rules = [[] for _ in range(R)]
    for i, b in enumerate(bodies):
        rules[i % R].append((i % R, b))
    _, got, _ = check(dev, tri, E, R, rules)
    assert sum(int(x.sum()) for x in got["support"]) > 0


# ------------------------------------------------------------ 4. grid-stride
def test_one_and_three_workgroups_give_the_default_grids_counts(dev):
    """2,163 distinct bodies on UMLS, more than the 2,048 workgroups of the
    default grid: whatever the grid, a workgroup's sums leave it per item."""
    from rnnlogic_amd.miner import RuleMiner
    graph = real_graph("umls")
    R = graph.relation_size
    bodies = [()] + [(a,) for a in range(R)] + [(a, b) for a in range(R) for b in range(R)]
    assert len(bodies) == 2163
    rules = [[] for _ in range(R)]
    for i, b in enumerate(bodies):
        for hd in sorted(set([i % R, (i * 7 + 1) % R, b[0] if b else 0])):
            rules[hd].append((hd, b))
    miner = RuleMiner(graph, dev)
    default = miner.rule_stats(rules)
    assert_same(default, ms.stats_of(real_dense("umls"), rules))
    for blocks in (1, 3):
        assert_same(miner.rule_stats(rules, max_blocks=blocks), default)


# ------------------------------------------------------------- 5. real data
@pytest.mark.parametrize("data", ["umls", "kinship"])
def test_length_2_pool_and_the_handle_stays_untouched(dev, data, tmp_path):
    from rnnlogic_amd.miner import RuleMiner
    graph = real_graph(data)
    miner = RuleMiner(graph, dev)
    miner.mine(2, 1, 20, 0, LR, WD, TEMP, 10, seed=0)
    before = (miner.weights(), miner.H(), miner.eval_ranks(graph.test_facts))
    assert any(np.any(w != 0.0) for w in before[0]) and any(np.any(h != 0.0) for h in before[1])
    got = miner.pool_stats()
    n = miner.out_rule_stats(str(tmp_path / "stats.txt"), 10)
    after = (miner.weights(), miner.H(), miner.eval_ranks(graph.test_facts))
    assert all(np.array_equal(a, b) for a, b in zip(before[0], after[0]))
    assert all(np.array_equal(a, b) for a, b in zip(before[1], after[1]))
    assert np.array_equal(before[2], after[2])
    pool = miner.get_logic_rules()
    assert_same(got, ms.stats_of(real_dense(data), pool))
    assert all(np.all(s >= 1) for s in got["support"])  # every rule of the pool was found from a train triple
    assert all(np.shares_memory(a, b) for a, b in zip(miner.pool_stats()["body"], got["body"]) if len(a))  # cached
    assert n == len((tmp_path / "stats.txt").read_text().splitlines()) == len(miner.best_rules(10))
    assert_same(miner.rule_stats(pool), got)
    miner.search(2)
    assert miner._pool_stats is None  # until the next search


@pytest.mark.parametrize("data", ["umls", "kinship"])
def test_sample_of_the_length_3_pool(dev, data):
    from rnnlogic_amd.miner import RuleMiner
    graph = real_graph(data)
    miner = RuleMiner(graph, dev)
    rules = miner.search(3)
    got = miner.pool_stats()
    off = np.searchsorted(np.asarray([hd for hd, _ in rules]), np.arange(graph.relation_size + 1))
    dense = real_dense(data)
    pick = np.sort(np.random.default_rng(11).choice(len(rules), 300, replace=False))
    for i in pick.tolist():
        hd, body = rules[i]
        k = i - off[hd]
        assert (got["support"][hd][k], got["body"][hd][k], got["pca_body"][hd][k]) == dense.stats(hd, body), rules[i]
    assert sum(len(x) for x in got["support"]) == len(rules)


# ---------------------------------------------------------- 6. repeatability
def test_two_runs_and_a_wrapping_stamp_give_identical_arrays(dev):
    from rnnlogic_amd.miner import RuleMiner
    E, R = 1500, 3  # the global scratch: stamps of an earlier call lie in memory the allocator hands out again
    tri = ms.random_graph(21, E, R, 6000)
    miner = RuleMiner(fake_graph(tri, E, R), dev, max_body=5)
    rules_a, rules_b = ms.random_rules(1, R, 40, 5), ms.random_rules(2, R, 40, 4)
    first = miner.rule_stats(rules_a)
    other = miner.rule_stats(rules_b)
    again = miner.rule_stats(rules_a)
    assert_same(again, first)
    ref = ms.SetStats(tri, E, R)
    assert_same(first, ms.stats_of(ref, rules_a))
    assert_same(other, ms.stats_of(ref, rules_b))
    # the visited stamps wrap past 2^32 - 1 a few units into the run, in LDS and in global memory
    head, ln, body, off = miner._listed(rules_a)
    for stamp in (0xFFFFFFF0, 0xFFFFFFFF, 0xFFFFFF00):
        sup, bod, pca = miner._stats_arrays(head, ln, body, first_stamp=stamp)
        assert np.array_equal(sup, np.concatenate(first["support"]))
        assert np.array_equal(bod, np.concatenate(first["body"]))
        assert np.array_equal(pca, np.concatenate(first["pca_body"]))
    small = RuleMiner(fake_graph(TINY, 8, 4), dev)
    head, ln, body, off = small._listed(TINY_RULES)
    want = small._stats_arrays(head, ln, body)
    for stamp in (0xFFFFFFF0, 0xFFFFFFFA):
        assert all(np.array_equal(a, b) for a, b in zip(small._stats_arrays(head, ln, body, first_stamp=stamp), want))


# ------------------------------------------------------- 7. confidence priors
def test_mine_with_pca_priors_against_the_replay(dev, tmp_path):
    from rnnlogic_amd.miner import RuleMiner
    graph = real_graph("kinship")
    R, E = graph.relation_size, graph.entity_size
    miner = RuleMiner(graph, dev)
    miner.search(2)
    pool = miner.get_logic_rules()
    sel = [list(range(len(pool[r])))[::3][:30] for r in range(R)]
    order = np.random.default_rng(9).permutation(len(graph.train_facts)).astype(np.int32)
    miner.mine(2, 1, 30, 0, LR, WD, TEMP, orders=[order], selections=[sel], prior="pca", prior_weight=0.5)
    subset = [[pool[r][i] for i in sel[r]] for r in range(R)]
    st = ms.stats_of(real_dense("kinship"), subset)
    priors = [ms.confidence("pca", st["support"][r], st["body"][r], st["pca_body"][r], 0).tolist() for r in range(R)]
    assert max(max(p) for p in priors if p) > min(min(p) for p in priors if p)
    ref = mine_ref.MineRef(graph.train_facts, E, R)
    ref.set_logic_rules(subset, priors)
    ref.learn(order, len(graph.train_facts), LR, WD, TEMP, False)
    ref.h_score(order, len(graph.train_facts), 0, 1.0, 0.5)
    worst = max(float(np.max(np.abs(np.asarray(ref.H[r]) - miner.pool_H[r][sel[r]]))) for r in range(R) if sel[r])
    print("mine(prior='pca', prior_weight=0.5): max |H - H_ref| = %.3g" % worst)
    assert worst <= TOL_H
    with_prior = [h.copy() for h in miner.pool_H]
    miner.mine(2, 1, 30, 0, LR, WD, TEMP, orders=[order], selections=[sel])  # the priors matter
    assert max(float(np.max(np.abs(a - b))) for a, b in zip(with_prior, miner.pool_H) if len(a)) > 1e6 * TOL_H
    with pytest.raises(ValueError):
        miner.mine(2, 1, 30, 0, LR, WD, TEMP, prior="amie")


def test_mine_with_default_arguments_writes_the_same_file(dev, tmp_path):
    from rnnlogic_amd.miner import RuleMiner
    graph = real_graph("kinship")
    old = RuleMiner(graph, dev)
    old.mine(2, 2, 20, 3, LR, WD, TEMP, 10, 5, None, None, 1.0)  # the argument list before the priors
    old.out_rules(str(tmp_path / "old.txt"), 10)
    new = RuleMiner(graph, dev)
    new.mine(2, 2, 20, 3, LR, WD, TEMP, 10, seed=5, prior=None, prior_weight=0.0, pc=0.0)
    new.out_rules(str(tmp_path / "new.txt"), 10, min_support=0, min_confidence=0.0, confidence="pca", pc=0.0)
    assert (tmp_path / "old.txt").read_bytes() == (tmp_path / "new.txt").read_bytes()
    assert len((tmp_path / "old.txt").read_text().splitlines()) > 100
    # a prior without weight changes nothing either; a weighted one does
    new.mine(2, 2, 20, 3, LR, WD, TEMP, 10, seed=5, prior="std", prior_weight=0.0)
    new.out_rules(str(tmp_path / "zero.txt"), 10)
    assert (tmp_path / "old.txt").read_bytes() == (tmp_path / "zero.txt").read_bytes()
    new.mine(2, 2, 20, 3, LR, WD, TEMP, 10, seed=5, prior="std", prior_weight=5.0)
    new.out_rules(str(tmp_path / "five.txt"), 10)
    assert (tmp_path / "old.txt").read_bytes() != (tmp_path / "five.txt").read_bytes()


# ---------------------------------------------------------- 8. command line
def run_cli(args, cwd):
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "rnnlogic_amd.miner"] + args, check=True, env=env, cwd=str(cwd),
                          timeout=300, capture_output=True, text=True).stdout.splitlines()


def parse_stats(path):
    rows = []
    for line in open(str(path)):
        tok = line.split()
        ids = [int(x) for x in tok[:-6]]
        rows.append(((ids[0], tuple(ids[1:])), tok[-6], tuple(int(x) for x in tok[-5:-2]), float(tok[-2]),
                     float(tok[-1])))
    return rows


def test_command_line_stats_file_filters_and_rule_file(dev, tmp_path, capsys):
    """One run of the module as a program; the other two argument lists go
    through the same main() in this process, which spares two interpreter starts."""
    from rnnlogic_amd.miner import RuleMiner, main
    graph = real_graph("umls")
    dense = real_dense("umls")
    args = ["-data-path", graph.data_path, "-max-length", "2", "-iterations", "1", "-lr", str(LR), "-wd", str(WD),
            "-temp", str(TEMP), "-top-k", "0", "-top-n", "20", "-top-n-out", "10"]
    miner = RuleMiner(graph, dev)
    miner.mine(2, 1, 20, 0, LR, WD, TEMP, 10, seed=0)
    miner.out_rules(str(tmp_path / "api.txt"), 10)
    # -stats-file: one line per rule written, the API's counts
    out = run_cli(args + ["-output-file", str(tmp_path / "r.txt"), "-stats-file", str(tmp_path / "s.txt")], tmp_path)
    assert (tmp_path / "r.txt").read_bytes() == (tmp_path / "api.txt").read_bytes()
    rules_lines = (tmp_path / "r.txt").read_text().splitlines()
    rows = parse_stats(tmp_path / "s.txt")
    assert out[-1] == "#Rules written: %d" % len(rows) and len(rows) == len(rules_lines)
    pool, st = miner.get_logic_rules(), miner.pool_stats()
    for (rule, H, counts, std, pca), line in zip(rows, rules_lines):
        k = pool[rule[0]].index(rule)
        assert counts == tuple(int(st[key][rule[0]][k]) for key in KEYS) == dense.stats(*rule)
        assert line == "%d%s %s" % (rule[0], "".join(" %d" % b for b in rule[1]), H)
        assert std == float("%.16f" % (counts[0] / counts[1])) and pca == float("%.16f" % (counts[0] / counts[2]))
    # the bounds: exactly the rules the restatement keeps, H descending then pool order, ten per head
    main(args + ["-output-file", str(tmp_path / "f.txt"), "-stats-file", str(tmp_path / "fs.txt"), "-min-support",
                 "1", "-min-conf", "0.1"])
    want = []
    for r, rules in enumerate(pool):
        keep = []
        for k in mine_ref.out_order(miner.pool_H[r].tolist()):
            sup, _, pca_body = dense.stats(*rules[k])
            if sup >= 1 and (sup / pca_body if pca_body else 0.0) >= 0.1:
                keep.append("%d%s %.16f" % (r, "".join(" %d" % b for b in rules[k][1]), miner.pool_H[r][k]))
        want += keep[:10]
    filtered = (tmp_path / "f.txt").read_text().splitlines()
    assert filtered == want and filtered != rules_lines and len(filtered) > 0
    assert [row[0] for row in parse_stats(tmp_path / "fs.txt")] == \
        [(int(ln.split()[0]), tuple(int(x) for x in ln.split()[1:-1])) for ln in filtered]
    assert miner.out_rules(str(tmp_path / "api_f.txt"), 10, 1, 0.1) == len(filtered)
    assert (tmp_path / "api_f.txt").read_text().splitlines() == filtered
    # -rule-file F -stats-file G: the statistics of a rule file, no -evaluate needed
    capsys.readouterr()
    main(["-data-path", graph.data_path, "-rule-file", str(tmp_path / "r.txt"), "-stats-file", str(tmp_path / "g.txt")])
    out = capsys.readouterr().out.splitlines()
    assert out[-2:] == ["#Rules read: %d" % len(rows), "#Rule statistics written: %d" % len(rows)]
    again = parse_stats(tmp_path / "g.txt")
    assert [(a[0], a[2], a[3], a[4]) for a in again] == [(a[0], a[2], a[3], a[4]) for a in rows]
    # what was an error stays one
    for bad in (["-rule-file", str(tmp_path / "r.txt")], ["-stats-file", str(tmp_path / "x.txt")],
                ["-rule-file", str(tmp_path / "r.txt"), "-output-file", str(tmp_path / "y.txt"), "-evaluate", "test"],
                ["-rule-file", str(tmp_path / "r.txt"), "-stats-file", str(tmp_path / "x.txt"), "-min-support", "1"]):
        with pytest.raises(SystemExit):
            main(["-data-path", graph.data_path] + bad)
