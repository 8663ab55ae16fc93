"""The miner's evaluation on the GPU — RuleMiner.set_weights / read_rules /
scores / eval_ranks / evaluate (rnnl_miner_evaluate, csrc/mine_eval.hip) —
against what the reference's ReasoningPredictor::evaluate said
(tests/golden/_mine_eval_*.npz, tools/make_golden_mine_eval.py) and against the
fp64 restatement tests/mine_eval_ref.py.

No tolerances but one: scores are compared bitwise and the (num_g, num_ge)
pairs exactly, because a tie run decides the metrics and a last-bit difference
in a score moves an entity across it.  The metrics of the reference fixtures
are ~7,500-term fp64 sums of the same terms in the same order; the issue's
bound for them is 1e-12 relative.
"""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import mine_eval_ref
from conftest import GOLDEN, REPO

pytestmark = pytest.mark.gpu

LR, WD, TEMP = 0.01, 0.0005, 100.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


_graphs, _fixtures = {}, {}


def real_graph(data):
    if data not in _graphs:
        from rnnlogic_amd import datasets
        from rnnlogic_amd.data import KnowledgeGraph
        _graphs[data] = KnowledgeGraph(datasets.materialize(data))
    return _graphs[data]


def fixture(data):
    if data not in _fixtures:
        _fixtures[data] = mine_eval_ref.load_fixture(os.path.join(GOLDEN, "_mine_eval_%s.npz" % data))
    return _fixtures[data]


def write_rule_file(path, rel2rules, rel2weights):
    with open(path, "w") as fo:
        for rules, ws in zip(rel2rules, rel2weights):
            for (hd, body), w in zip(rules, ws):
                fo.write("%d%s %r\n" % (hd, "".join(" %d" % b for b in body), float(w)))  # repr round-trips


def fake_graph(triples, E, R, **more):
    return types.SimpleNamespace(train_facts=[tuple(t) for t in triples], entity_size=E, relation_size=R, **more)


def check_against_restatement(dev, triples, E, R, rules, weights, queries, known=None, **more):
    """scores bitwise, pairs exactly, filtered and unfiltered; returns the miner and the pairs."""
    from rnnlogic_amd.miner import RuleMiner
    miner = RuleMiner(fake_graph(triples, E, R, **more), dev)
    miner.set_logic_rules(rules)
    miner.set_weights(weights)
    ref = mine_eval_ref.MineEvalRef(triples, E, R, known=known)
    ref.set_rules(rules, weights)
    want = np.asarray([ref.scores(*q) for q in queries], dtype=np.float64).reshape(len(queries), E)
    got = miner.scores(queries).cpu().numpy()
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(got, want)
    out = {}
    for filtered in (True, False):
        pairs = miner.eval_ranks(queries, filtered=filtered)
        assert pairs.dtype == np.int64
        assert np.array_equal(pairs, np.asarray(ref.pairs(queries, filtered), dtype=np.int64).reshape(-1, 2))
        assert np.all(pairs[:, 1] - pairs[:, 0] >= 1)
        out[filtered] = pairs
    return miner, want, out


# ------------------------------------------------- 1. reference fixtures
@pytest.mark.parametrize("how", ["set_weights", "read_rules"])
@pytest.mark.parametrize("data", ["kinship", "umls"])
def test_reference_fixture(data, how, dev, tmp_path):
    from rnnlogic_amd.miner import RuleMiner
    graph, fx = real_graph(data), fixture(data)
    miner = RuleMiner(graph, dev)
    if how == "set_weights":
        miner.set_logic_rules(fx["rules"])
        miner.set_weights(fx["weights"])
    else:
        write_rule_file(str(tmp_path / "rules.txt"), fx["rules"], fx["weights"])
        assert miner.read_rules(str(tmp_path / "rules.txt")) == sum(len(x) for x in fx["rules"])
    assert all(np.array_equal(a, np.asarray(b)) for a, b in zip(miner.weights(), fx["weights"]))
    for split in ("valid", "test"):
        facts = getattr(graph, split + "_facts")
        pairs = miner.eval_ranks(facts)
        assert np.array_equal(pairs, fx["pairs"][split])
        m = miner.evaluate(split)
        assert m["n"] == len(facts)
        for name, want in zip(mine_eval_ref.METRIC_NAMES, fx["metrics"][split]):
            print("%s %s %s: %.17g (reference %.17g)" % (data, split, name, m[name], want))
            assert abs(m[name] - want) <= 1e-12 * abs(want)


# --------------------------------------------------------- 2. tiny graph
# (the graph and rule lists of test_gpu_mine_learn.py) relation 2 has triples
# but no rules, relation 3 rules but no triples; (0,0,1) is there twice;
# (2,0,2) is a self-loop; 0 -1-> {3,4} -1-> 5 are two parallel paths; nothing
# but its own edge leaves 6
TINY = [(0, 0, 1), (0, 0, 1), (2, 0, 2), (0, 0, 5), (6, 0, 7), (0, 1, 3), (0, 1, 4), (3, 1, 5), (4, 1, 5), (1, 1, 5),
        (5, 2, 0), (5, 2, 1), (3, 2, 4), (0, 1, 1), (2, 1, 2), (1, 0, 5), (7, 2, 6), (5, 1, 3)]
TINY_RULES = [
    [(0, ()), (0, (1,)), (0, (1, 1)), (0, (1, 2, 1)), (0, (0,)), (0, (1, 1)), (0, (0, 1)), (0, (1, 1, 2)), (0, (3,))],
    [(1, (0,)), (1, (1, 1)), (1, (0, 1)), (1, (1, 2, 0))],
    [],
    [(3, (1,)), (3, (0, 1))],
]
# a zero, a repeated value (0.5, and the two copies of the body (1, 1) get +0.5 and -0.5), negatives
TINY_WEIGHTS = [[3.0, 0.5, 0.5, -0.25, 0.0, -0.5, 0.1, 0.30000000000000004, 1.0], [1.0, -0.25, 0.5, 0.5], [],
                [0.7, -0.7]]
TINY_QUERIES = [
    (0, 0, 1),  # a train triple that occurs twice: both copies are removed; known tails of (0, 0): 1 and 5
    (0, 0, 5),  # the other known tail of the same row
    (3, 0, 6),  # not a train triple
    (5, 2, 0),  # relation 2 has no rules: every val is 0
    (0, 0, 7),  # nothing reaches 7 from 0
    (0, 0, 1),  # the same query again
    (6, 0, 7),  # nothing grounds at all
    (2, 0, 2),  # the self-loop, removed
    (0, 1, 5),  # relation 1, not a train triple; known tails of (0, 1): 1, 3, 4
    (0, 3, 3),  # a relation with rules and no triples
    (5, 2, 0),
]


def test_tiny_graph_against_restatement(dev):
    _, val, pairs = check_against_restatement(dev, TINY, 8, 4, TINY_RULES, TINY_WEIGHTS, TINY_QUERIES)
    # (0, 0, 1) is there twice: its removal drops both copies, so 0 <- 0 reaches only 5
    ref = mine_eval_ref.MineEvalRef(TINY, 8, 4)
    assert ref.g.destinations(0, (0,), (0, 0, 1)) == [(5, 1)] and ref.g.destinations(0, (0,), (0, 0, 5)) == [(1, 2)]
    assert np.all(val[3] == 0.0)  # no rules: num_g = 0, num_ge = every unskipped entity
    assert pairs[False][3].tolist() == [0, 8] and pairs[True][3].tolist() == [0, 7]  # (5, 2, 1) is known
    assert val[4][7] == 0.0 and val[4].any()
    assert np.array_equal(pairs[True][0], pairs[True][5]) and np.array_equal(val[0], val[5])
    assert not val[6].any() and pairs[False][6].tolist() == [0, 8]
    assert any(g != f for g, f in zip(pairs[True][:, 1].tolist(), pairs[False][:, 1].tolist()))


def test_tiny_graph_filters_by_valid_and_test_too(dev):
    """graph.valid_facts / test_facts join the known tails; the graph walked stays the train graph."""
    valid, test = [(0, 0, 3), (0, 0, 4)], [(0, 0, 6), (3, 0, 6)]
    _, _, pairs = check_against_restatement(dev, TINY, 8, 4, TINY_RULES, TINY_WEIGHTS, TINY_QUERIES + valid + test,
                                            known=TINY + valid + test, valid_facts=valid, test_facts=test)
    _, _, train_only = check_against_restatement(dev, TINY, 8, 4, TINY_RULES, TINY_WEIGHTS, TINY_QUERIES + valid + test)
    assert not np.array_equal(pairs[True], train_only[True]) and np.array_equal(pairs[False], train_only[False])


def test_set_weights_keeps_rules_and_set_rules_clears_weights(dev):
    from rnnlogic_amd.miner import RuleMiner
    miner = RuleMiner(fake_graph(TINY, 8, 4), dev)
    miner.set_logic_rules(TINY_RULES)
    miner.set_weights(TINY_WEIGHTS)
    assert all(np.array_equal(a, np.asarray(b)) for a, b in zip(miner.weights(), TINY_WEIGHTS))
    with pytest.raises(ValueError):
        miner.set_weights(TINY_WEIGHTS[:3])
    with pytest.raises(ValueError):
        miner.eval_ranks([(0, 0, 8)])
    with pytest.raises(ValueError):
        miner.evaluate(triples=[])
    miner.set_logic_rules(TINY_RULES)
    assert all(np.all(w == 0.0) for w in miner.weights())
    assert not miner.scores(TINY_QUERIES).cpu().numpy().any()


# ------------------------- 3. more rules than any lane or wave layout holds
def many_rules_graph():
    """10 relations, every body of length 1..3 as relation 0's list: 1,110 rules."""
    rng = np.random.default_rng(5)
    R, E = 10, 8
    tri = sorted(set((int(h), int(r), int(t)) for h, r, t in
                     zip(rng.integers(0, E, 90), rng.integers(0, R, 90), rng.integers(0, E, 90))))
    bodies = [(a,) for a in range(R)] + [(a, b) for a in range(R) for b in range(R)] + \
        [(a, b, c) for a in range(R) for b in range(R) for c in range(R)]
    rules = [[(0, b) for b in bodies]] + [[(r, (r - 1,)), (r, (0, r))] for r in range(1, R)]
    return tri, E, R, rules


def quantised_weights(rules, seed):
    rng = np.random.default_rng(seed)
    return [[float(x) for x in rng.choice([0.0, 0.5, 0.5, -0.25, 0.1, 1e-3, -1.7], len(rs))] for rs in rules]


def test_more_rules_than_lanes(dev):
    tri, E, R, rules = many_rules_graph()
    assert len(rules[0]) == 1110
    queries = tri + [(h, 0, t) for h in range(E) for t in (0, 5)]
    _, val, pairs = check_against_restatement(dev, tri, E, R, rules, quantised_weights(rules, 1), queries)
    assert np.any(pairs[True][:, 1] - pairs[True][:, 0] > 1) and np.any(pairs[True][:, 0] > 0)


# ---------------------------- 4. the regimes of the dense arrays (LDS / global)
def spread_graph(E):
    """A hub over the whole index range: 0 -1-> 100 nodes -2-> 5, some of them on
    to the last entities, so rules of length 1..3 reach entities at both ends
    (for E = 2,100: on both sides of index 2,048) and 0 <- 1 2 reaches 5 along
    100 parallel paths."""
    last = E - 1
    mids = sorted(set(3 + (i * (E - 10)) // 100 for i in range(1, 101)) - {5})
    tri = [(0, 0, 5), (0, 0, mids[7]), (7, 0, 5), (last, 0, 0), (5, 0, last), (0, 0, last - 1)]
    tri += [(0, 1, x) for x in mids] + [(x, 2, 5) for x in mids] + [(x, 2, last - 2) for x in mids[-30:]]
    tri += [(7, 1, mids[3]), (5, 1, last), (last, 2, 0), (last - 2, 0, last - 3), (5, 0, 1), (0, 1, last)]
    rules = [[(0, (1,)), (0, (1, 2)), (0, (1, 2, 0)), (0, (0, 1)), (0, (2,)), (0, (1, 2))],
             [(1, (0,)), (1, (1, 2, 1))], [(2, (0, 0)), (2, (2,))]]
    return tri, E, 3, rules, mids


@pytest.mark.parametrize("E", [512, 513, 2100])
def test_entities_in_lds_and_in_global_memory(dev, E):
    """512 entities are the most the LDS arrays hold; from 513 on val and the
    integer scratch are per-workgroup global memory."""
    tri, E, R, rules, mids = spread_graph(E)
    weights = [[0.5, -0.25, 1.0, 0.0, 0.5, 0.125], [1.0, 0.5], [0.5, 0.5]]
    queries = [(0, 0, 5), (0, 0, E - 1), (0, 0, E - 2), (7, 0, 5), (0, 0, mids[50]), (0, 1, E - 1), (E - 1, 2, 0),
               (5, 2, E - 3), (0, 0, 5)]
    _, val, pairs = check_against_restatement(dev, tri, E, R, rules, weights, queries)
    assert val[0][E - 4] == 30.0  # 0 -1-> 30 mids -2-> E-3 -0-> E-4: 1.0 * 30 paths at the far end
    assert val[0][5] == -0.25 * (len(mids)) + 0.125 * len(mids) and val[0][1] != 0.0


# -------------------------------------------------------- 5. range error
def test_path_count_past_32_bits_is_reported(dev):
    """1,700 parallel edges on each of three hops: 1,700^3 > 2^32 paths."""
    from rnnlogic_amd import _native
    from rnnlogic_amd.miner import RuleMiner
    tri = [(0, 0, 3)] + [(0, 1, 1)] * 1700 + [(1, 1, 2)] * 1700 + [(2, 1, 3)] * 1700
    miner = RuleMiner(fake_graph(tri, 4, 2), dev)
    miner.set_logic_rules([[(0, (1, 1, 1))], []])
    miner.set_weights([[0.5], []])
    with pytest.raises(_native.NativeError) as err:
        miner.eval_ranks([(0, 0, 3)])
    assert err.value.code == _native.RNNL_ERR_RANGE
    miner.set_logic_rules([[(0, (1, 1))], []])  # 1,700^2 fits
    miner.set_weights([[0.5], []])
    assert miner.scores([(0, 0, 3)]).cpu().numpy().tolist() == [[0.0, 0.0, 0.5 * 1700 * 1700, 0.0]]
    assert miner.eval_ranks([(0, 0, 3)]).tolist() == [[1, 4]]


# ---------------------------------------------------- 6. learned weights
def test_learned_weights_on_kinship(dev):
    """mine() at length 2, then evaluate('valid') with the weights it learned
    equals the restatement fed those very weights, exactly."""
    from rnnlogic_amd.miner import RuleMiner
    graph = real_graph("kinship")
    R, E = graph.relation_size, graph.entity_size
    miner = RuleMiner(graph, dev)
    miner.search(2)
    pool = miner.get_logic_rules()
    sel = [list(range(len(pool[r])))[::3][:30] for r in range(R)]
    order = np.random.default_rng(9).permutation(len(graph.train_facts)).astype(np.int32)
    miner.mine(2, 1, 30, 0, LR, WD, TEMP, orders=[order], selections=[sel])
    weights = miner.weights()
    assert any(np.any(w != 0.0) for w in weights)
    ref = mine_eval_ref.MineEvalRef(graph.train_facts, E, R,
                                    known=graph.train_facts + graph.valid_facts + graph.test_facts)
    ref.set_rules([[pool[r][i] for i in sel[r]] for r in range(R)], weights)
    want = ref.pairs(graph.valid_facts)
    assert np.array_equal(miner.eval_ranks(graph.valid_facts), np.asarray(want, dtype=np.int64))
    got = miner.evaluate("valid")
    assert tuple(got[k] for k in mine_eval_ref.METRIC_NAMES) == mine_eval_ref.metrics(want, E)
    assert got["n"] == len(graph.valid_facts) and got["mrr"] > 1.0 / E


# ------------------------------------------------------ 7. repeatability
def test_two_calls_are_bitwise_equal(dev):
    from rnnlogic_amd.miner import RuleMiner
    graph, fx = real_graph("kinship"), fixture("kinship")
    miner = RuleMiner(graph, dev)
    miner.set_logic_rules(fx["rules"])
    miner.set_weights(fx["weights"])
    s = [miner.scores(graph.test_facts).cpu().numpy() for _ in range(2)]
    p = [miner.eval_ranks(graph.test_facts) for _ in range(2)]
    assert s[0].any() and np.array_equal(s[0], s[1]) and np.array_equal(p[0], p[1])


# ------------------------------------------------------- 8. command line
def run_cli(args, cwd):
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "rnnlogic_amd.miner"] + args, check=True, env=env, cwd=str(cwd),
                          timeout=300, capture_output=True, text=True).stdout.splitlines()


def test_command_line_evaluates_a_rule_file(dev, tmp_path):
    from rnnlogic_amd.miner import metrics_line
    graph, fx = real_graph("umls"), fixture("umls")
    write_rule_file(str(tmp_path / "rules.txt"), fx["rules"], fx["weights"])
    out = run_cli(["-data-path", graph.data_path, "-rule-file", str(tmp_path / "rules.txt"), "-evaluate", "both"],
                  tmp_path)
    want = [metrics_line(name, dict(zip(mine_eval_ref.METRIC_NAMES, fx["metrics"][split])))
            for name, split in (("Valid", "valid"), ("Test", "test"))]
    assert out[-3:] == ["#Rules read: %d" % sum(len(x) for x in fx["rules"])] + want
    assert want[0].startswith("Valid | MR ") and " MRR " in want[0] and " HITS@1 " in want[0]


def test_command_line_mines_as_before_and_evaluates_on_request(dev, tmp_path):
    from rnnlogic_amd.miner import RuleMiner, metrics_line
    graph = real_graph("kinship")
    miner = RuleMiner(graph, dev)
    miner.mine(2, 1, 20, 0, LR, WD, TEMP, 10, seed=0)
    api = tmp_path / "api.txt"
    n = miner.out_rules(str(api), 10)
    args = ["-data-path", graph.data_path, "-max-length", "2", "-iterations", "1", "-lr", str(LR), "-wd", str(WD),
            "-temp", str(TEMP), "-top-k", "0", "-top-n", "20", "-top-n-out", "10", "-output-file"]
    plain = run_cli(args + [str(tmp_path / "plain.txt")], tmp_path)
    assert (tmp_path / "plain.txt").read_bytes() == api.read_bytes()
    assert plain[-1] == "#Rules written: %d" % n and not any(" | MR " in ln for ln in plain)
    both = run_cli(args + [str(tmp_path / "eval.txt"), "-evaluate", "valid"], tmp_path)
    assert (tmp_path / "eval.txt").read_bytes() == api.read_bytes()
    assert both == plain + [metrics_line("Valid", miner.evaluate("valid"))]
