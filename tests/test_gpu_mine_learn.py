"""The miner after its search on the GPU — RuleMiner.set_logic_rules / learn /
h_score / mine / out_rules (rnnl_miner_learn, rnnl_miner_h_score,
csrc/mine_learn.hip) — against what the reference CLI printed with
`-threads 1` (tests/golden/_mine_*.npz, tools/make_golden_mine.py) and
against the fp64 restatement tests/mine_ref.py.

Tolerances: the kernels differ from the reference only in libm's exp (and, in
H_score, in summing the softmax denominator in a fixed tree of runs instead of one).  On
an MI355X the observed maxima over the reference fixtures were
max |dH| = 7.72e-17 and max |dwt| = 8.88e-16; the bounds are 100x
those, eleven orders below the 1.5e-3 by which a wrong triple order moves H.
"""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import mine_ref
from conftest import GOLDEN, REPO, golden_rules

pytestmark = pytest.mark.gpu

TOL_H = 7.72e-15
TOL_W = 8.88e-14
LR, WD, TEMP = 0.01, 0.0005, 100.0
FIXTURES = ["kinship_L2", "umls_L2", "umls_L3_sub", "kinship_L3_many"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


_graphs = {}


def real_graph(data):
    if data not in _graphs:
        from rnnlogic_amd import datasets
        from rnnlogic_amd.data import KnowledgeGraph
        _graphs[data] = KnowledgeGraph(datasets.materialize(data))
    return _graphs[data]


def flat_diff(got, want):
    return max([float(np.max(np.abs(np.asarray(g) - np.asarray(w)))) for g, w in zip(got, want) if len(w)] or [0.0])


# ------------------------------------------------------------ 1. fixtures
@pytest.mark.parametrize("case", FIXTURES)
def test_replay_of_reference_run(case, dev):
    from rnnlogic_amd.miner import RuleMiner
    graph = real_graph(case.split("_")[0])
    R = graph.relation_size
    fx = mine_ref.load_fixture(os.path.join(GOLDEN, "_mine_%s.npz" % case), R)
    a = fx["args"]
    miner = RuleMiner(graph, dev)
    out = miner.mine(a["max_length"], a["iterations"], a["top_n"], a["top_k"], a["lr"], a["wd"], a["temp"],
                     a["top_n_out"], orders=fx["orders"], selections=fx["selections"], portion=a["portion"])
    assert miner.get_logic_rules() == [[r for r in golden_rules(a["pool"]) if r[0] == hd] for hd in range(R)]
    got = np.asarray([miner.pool_H[r][k] for r, k in zip(fx["out_rel"], fx["out_idx"])])
    worst = float(np.max(np.abs(got - fx["out_H"])))
    print("%s: max |H_gpu - H_ref| = %.3g over %d rules" % (case, worst, len(got)))
    assert worst <= TOL_H
    ours = [[] for _ in range(R)]
    for hd, _, H in out:
        ours[hd].append(H)
    for r in range(R):
        want = fx["out_H"][fx["out_rel"] == r]
        assert len(ours[r]) == fx["out_len"][r]
        assert np.max(np.abs(np.asarray(ours[r][:len(want)]) - want), initial=0.0) <= TOL_H
        assert all(h == 0.0 for h in ours[r][len(want):])  # (only_selected: the rest was never selected)
    if a["max_length"] == 2:  # learn()'s weights against the restatement
        pool = miner.get_logic_rules()
        _, wt = mine_ref.mine_replay(graph.train_facts, graph.entity_size, R, pool, fx["orders"], fx["selections"],
                                     a["lr"], a["wd"], a["temp"], a["top_k"], a["portion"])
        dw = flat_diff(miner.weights(), wt)
        print("%s: max |wt_gpu - wt_ref| = %.3g" % (case, dw))
        assert dw <= TOL_W


# ------------------------------------------------------- 2. tiny graphs
def fake_graph(triples, E, R):
    return types.SimpleNamespace(train_facts=[tuple(t) for t in triples], entity_size=E, relation_size=R)


# relation 2 has triples but no rules, relation 3 rules but no triples; (0,0,1)
# is there twice; (2,0,2) is a self-loop; 0 -1-> {3,4} -1-> 5 are two parallel
# paths; nothing but its own edge leaves 6
TINY = [(0, 0, 1), (0, 0, 1), (2, 0, 2), (0, 0, 5), (6, 0, 7), (0, 1, 3), (0, 1, 4), (3, 1, 5), (4, 1, 5), (1, 1, 5),
        (5, 2, 0), (5, 2, 1), (3, 2, 4), (0, 1, 1), (2, 1, 2), (1, 0, 5), (7, 2, 6), (5, 1, 3)]
TINY_RULES = [
    [(0, ()), (0, (1,)), (0, (1, 1)), (0, (1, 2, 1)), (0, (0,)), (0, (1, 1)), (0, (0, 1)), (0, (1, 1, 2)), (0, (3,))],
    [(1, (0,)), (1, (1, 1)), (1, (0, 1)), (1, (1, 2, 0))],
    [],
    [(3, (1,)), (3, (0, 1))],
]
TINY_PRIORS = [[0.1 * k - 0.3 for k in range(len(rules))] for rules in TINY_RULES]


def many_rules_graph():
    """10 relations, every body of length 1..3 as relation 0's list: 1,110
    rules, more than the 1,024 lanes of the learn workgroup."""
    rng = np.random.default_rng(5)
    R, E = 10, 8
    tri = sorted(set((int(h), int(r), int(t)) for h, r, t in
                     zip(rng.integers(0, E, 90), rng.integers(0, R, 90), rng.integers(0, E, 90))))
    bodies = [(a,) for a in range(R)] + [(a, b) for a in range(R) for b in range(R)] + \
        [(a, b, c) for a in range(R) for b in range(R) for c in range(R)]
    rules = [[(0, b) for b in bodies]] + [[(r, (r - 1,)), (r, (0, r))] for r in range(1, R)]
    return tri, E, R, rules


def run_both(dev, triples, E, R, rules, priors, order, fast, top_k, portion, prior_weight, H_temperature=1.0,
             chunk=None):
    from rnnlogic_amd.miner import RuleMiner
    miner = RuleMiner(fake_graph(triples, E, R), dev)
    miner.chunk_triples = chunk
    miner.set_logic_rules(rules, priors)
    miner.learn(LR, WD, TEMP, fast=fast, portion=portion, order=order)
    miner.h_score(top_k, H_temperature, prior_weight, portion=portion)
    ref = mine_ref.MineRef(triples, E, R)
    ref.set_logic_rules(rules, priors)
    n_used = int(len(triples) * portion)
    ref.learn(order, n_used, LR, WD, TEMP, fast)
    ref.h_score(order, n_used, top_k, H_temperature, prior_weight)
    return miner.weights(), miner.H(), ref.weights(), ref.H


@pytest.mark.parametrize("fast,top_k,portion,prior_weight", [
    (False, 0, 1.0, 0.0), (True, 0, 1.0, 0.0), (False, 2, 1.0, 0.0), (False, 0, 0.5, 0.0), (True, 3, 0.5, 0.7),
    (False, 0, 1.0, 0.7)])
def test_tiny_graph_against_restatement(dev, fast, top_k, portion, prior_weight):
    order = np.random.default_rng(1).permutation(len(TINY)).astype(np.int32)
    w, H, rw, rH = run_both(dev, TINY, 8, 4, TINY_RULES, TINY_PRIORS, order, fast, top_k, portion, prior_weight,
                            H_temperature=2.0 if prior_weight else 1.0)
    assert any(abs(x) > 1e-3 for x in rw[0]) and sum(len(x) for x in w) == sum(len(r) for r in TINY_RULES)
    print("tiny: |dwt| %.3g |dH| %.3g" % (flat_diff(w, rw), flat_diff(H, rH)))
    assert flat_diff(w, rw) <= TOL_W and flat_diff(H, rH) <= TOL_H
    assert np.all(H[3] == 0.0) and np.all(w[3] == 0.0)  # rules, but no triples


def test_tiny_graph_top_k_ties_go_to_the_earlier_rule(dev):
    """Rules 2 and 5 of relation 0 are the same body, so their val ties; with
    top_k = 1 on the parallel-path triple (0, 0, 5) the share goes to one rule,
    and among exactly tied val to the earlier position."""
    order = np.asarray([3] + [i for i in range(len(TINY)) if i != 3], dtype=np.int32)
    _, H, _, rH = run_both(dev, TINY, 8, 4, TINY_RULES, None, order, False, 1, 1.5 / len(TINY), 0.0)
    assert flat_diff(H, rH) <= TOL_H
    assert np.count_nonzero(H[0]) == 1 and H[0][5] == 0.0


def test_triple_that_nothing_grounds(dev):
    """Only (6, 0, 7) is walked: no rule of relation 0 grounds it, so learn
    leaves every weight at 0 and H_score gives each of its rules 1 / nr / n."""
    order = np.asarray([4] + [i for i in range(len(TINY)) if i != 4], dtype=np.int32)
    w, H, rw, rH = run_both(dev, TINY, 8, 4, TINY_RULES, None, order, False, 0, 1.5 / len(TINY), 0.0)
    assert all(np.all(x == 0.0) for x in w)
    share = 1.0 / len(TINY_RULES[0]) / len(TINY)
    assert np.max(np.abs(H[0] - share)) <= 1e-17 and np.all(H[1] == 0.0)
    assert flat_diff(H, rH) <= TOL_H


def test_duplicated_triple_and_self_loop(dev):
    """(0, 0, 1) twice: walking it removes both copies, so 0 <- 0 reaches only
    5, whose target is 1 ((0, 0, 5) is a train triple).  (2, 0, 2) with the
    empty body in the list: the empty body reaches nothing."""
    order = np.asarray([0, 2] + [i for i in range(len(TINY)) if i not in (0, 2)], dtype=np.int32)
    w, H, rw, rH = run_both(dev, TINY, 8, 4, TINY_RULES, None, order, False, 0, 2.5 / len(TINY), 0.0)
    assert w[0][0] == 0.0 and rw[0][0] == 0.0  # the empty body is never updated
    assert w[0][4] > 0.0  # 0 <- 0 saw target 1 at its only destination
    assert flat_diff(w, rw) <= TOL_W and flat_diff(H, rH) <= TOL_H


@pytest.mark.parametrize("fast", [False, True])
def test_more_rules_than_lanes(dev, fast):
    tri, E, R, rules = many_rules_graph()
    assert len(rules[0]) > 1024
    order = np.random.default_rng(2).permutation(len(tri)).astype(np.int32)
    w, H, rw, rH = run_both(dev, tri, E, R, rules, None, order, fast, 0, 1.0, 0.0)
    g = mine_ref.MineRef(tri, E, R)
    assert max(c for t in tri for _, b in rules[0] for _, c in g.destinations(t[0], b, t)) > 1  # parallel paths
    print("many rules: |dwt| %.3g |dH| %.3g" % (flat_diff(w, rw), flat_diff(H, rH)))
    assert flat_diff(w, rw) <= TOL_W and flat_diff(H, rH) <= TOL_H


def hub_graph():
    """2,100 entities — past the 2,048 up to which the per-relation arrays
    live in LDS — with a hub: 0 -1-> 100 nodes -2-> 5, so 0 <- 1 has more
    destinations than the grounding workgroup's 64 lanes and 0 <- 1 2 reaches 5
    along 100 parallel paths."""
    mids = [20 * i + 3 for i in range(1, 101)]
    tri = [(0, 0, 5), (0, 0, mids[7]), (7, 0, 5), (2099, 0, 0), (5, 0, 2099)]
    tri += [(0, 1, x) for x in mids] + [(x, 2, 5) for x in mids] + [(7, 1, mids[3]), (5, 1, 2099), (2099, 2, 0)]
    rules = [[(0, (1,)), (0, (1, 2)), (0, (1, 2, 0)), (0, (0, 1)), (0, (2,))], [(1, (0,)), (1, (1, 2, 1))], []]
    return tri, 2100, 3, rules


@pytest.mark.parametrize("fast", [False, True])
def test_more_entities_than_the_lds_arrays_hold(dev, fast):
    tri, E, R, rules = hub_graph()
    order = np.random.default_rng(6).permutation(len(tri)).astype(np.int32)
    w, H, rw, rH = run_both(dev, tri, E, R, rules, None, order, fast, 0, 1.0, 0.0)
    g = mine_ref.MineRef(tri, E, R)
    assert len(g.destinations(0, (1,), (0, 0, 5))) == 100 and g.destinations(0, (1, 2), (0, 0, 5)) == [(5, 100)]
    print("hub: |dwt| %.3g |dH| %.3g" % (flat_diff(w, rw), flat_diff(H, rH)))
    assert flat_diff(w, rw) <= TOL_W and flat_diff(H, rH) <= TOL_H


def test_path_count_past_32_bits_is_reported(dev):
    """1,700 parallel edges on each of three hops: 1,700^3 > 2^32 paths.  The
    u32 count of an entry cannot hold that: RNNL_ERR_RANGE, not a wrapped count."""
    from rnnlogic_amd import _native
    from rnnlogic_amd.miner import RuleMiner
    tri = [(0, 0, 3)] + [(0, 1, 1)] * 1700 + [(1, 1, 2)] * 1700 + [(2, 1, 3)] * 1700
    miner = RuleMiner(fake_graph(tri, 4, 2), dev)
    miner.set_logic_rules([[(0, (1, 1, 1))], []])
    with pytest.raises(_native.NativeError) as err:
        miner.learn(LR, WD, TEMP, order=np.arange(len(tri), dtype=np.int32))
    assert err.value.code == _native.RNNL_ERR_RANGE
    miner.set_logic_rules([[(0, (1, 1))], []])  # 1,700^2 fits
    miner.learn(LR, WD, TEMP, fast=True, order=np.arange(len(tri), dtype=np.int32))
    # one destination (2, not a tail of (0, 0, .)): p = 1, target 0; Adam's first step is -lr
    assert abs(miner.weights()[0][0] + LR) < 1e-12


def test_count_past_32_bits_on_an_inner_hop_that_dead_ends(dev):
    """Where learn and evaluate differ on purpose.  A chain
    0 -0-> 1 -1-> 2 -2-> 3 -3-> 4, the first three edges 1,626 times each:
    1,626^3 = 4,298,942,376 > 2^32 paths reach entity 3, hop 4 carries that
    count on to entity 4, and no edge of relation 4 leaves entity 4.  The body
    [0, 1, 2, 3, 4] has no destination.  The query kernels report a count past
    32 bits on whichever hop carries it; the grounding of learn looks at the
    final counts only, finds none, and leaves the weight alone."""
    from rnnlogic_amd import _native
    from rnnlogic_amd.miner import RuleMiner
    assert 1626 ** 3 == 4298942376 > 2 ** 32
    tri = [(0, 0, 1)] * 1626 + [(1, 1, 2)] * 1626 + [(2, 2, 3)] * 1626 + [(3, 3, 4), (0, 5, 5)]
    miner = RuleMiner(fake_graph(tri, 6, 6), dev, max_body=5)
    miner.set_logic_rules([[], [], [], [], [], [(5, (0, 1, 2, 3, 4))]])
    for ask in (miner.scores, miner.eval_ranks):
        with pytest.raises(_native.NativeError) as err:
            ask([(0, 5, 5)])
        assert err.value.code == _native.RNNL_ERR_RANGE
    miner.learn(LR, WD, TEMP, order=np.arange(len(tri), dtype=np.int32))
    assert miner.weights()[5][0] == 0.0  # its initial value: no destination, no step


# ---------------------------------------------------------- 3. chunking
def test_chunking_is_bitwise_neutral(dev):
    tri, E, R, rules = many_rules_graph()
    order = np.random.default_rng(3).permutation(len(tri)).astype(np.int32)
    runs = [run_both(dev, tri, E, R, rules, None, order, False, 0, 1.0, 0.0, chunk=c)[:2] for c in (1, 7, None)]
    for w, H in runs[1:]:
        assert all(np.array_equal(x, y) for x, y in zip(w, runs[0][0]))
        assert all(np.array_equal(x, y) for x, y in zip(H, runs[0][1]))
    order = np.random.default_rng(4).permutation(len(TINY)).astype(np.int32)
    runs = [run_both(dev, TINY, 8, 4, TINY_RULES, TINY_PRIORS, order, False, 2, 1.0, 0.3, chunk=c)[:2]
            for c in (1, 7, None)]
    for w, H in runs[1:]:
        assert all(np.array_equal(x, y) for x, y in zip(w, runs[0][0]))
        assert all(np.array_equal(x, y) for x, y in zip(H, runs[0][1]))


# ------------------------------------- 4. repeatability, 5. round trip, CLI
CLI_ARGS = dict(max_length=2, iterations=2, top_n=20, top_k=0, lr=LR, wd=WD, temp=TEMP, top_n_out=10)


def test_mine_repeats_bitwise_and_round_trips(dev, tmp_path):
    from rnnlogic_amd.miner import RuleMiner
    from rnnlogic_amd.predictors import _read_rules
    graph = real_graph("kinship")
    files = []
    for k in range(2):
        miner = RuleMiner(graph, dev)
        out = miner.mine(seed=7, **CLI_ARGS)
        files.append(tmp_path / ("rules%d.txt" % k))
        assert miner.out_rules(str(files[-1]), CLI_ARGS["top_n_out"]) == len(out)
        if k:
            assert out == first
        first = out
    assert files[0].read_bytes() == files[1].read_bytes()
    assert 0 < len(first) <= 10 * graph.relation_size and any(H > 0 for _, _, H in first)
    assert _read_rules(str(files[0])) == [(hd, list(body)) for hd, body, _ in first]
    tok = files[0].read_text().splitlines()[0].split()
    assert len(tok[-1].split(".")[1]) == 16  # "%.16lf"


def test_command_line_module_writes_the_api_file(dev, tmp_path):
    from rnnlogic_amd.miner import RuleMiner
    graph = real_graph("kinship")
    miner = RuleMiner(graph, dev)
    miner.mine(seed=0, **CLI_ARGS)
    api = tmp_path / "api.txt"
    miner.out_rules(str(api), CLI_ARGS["top_n_out"])
    cli = tmp_path / "cli.txt"
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    subprocess.run([sys.executable, "-m", "rnnlogic_amd.miner", "-data-path", graph.data_path, "-output-file",
                    str(cli), "-max-length", "2", "-threads", "40", "-iterations", "2", "-lr", str(LR), "-wd",
                    str(WD), "-temp", str(TEMP), "-top-k", "0", "-top-n", "20", "-top-n-out", "10"],
                   check=True, env=env, cwd=str(tmp_path), timeout=300)
    assert cli.read_bytes() == api.read_bytes()
