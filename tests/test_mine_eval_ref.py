"""CPU side of the miner's evaluation: the restatement tests/mine_eval_ref.py
against what the reference's ReasoningPredictor::evaluate said
(tests/golden/_mine_eval_*.npz), rnnlogic_amd.miner.expectation_metrics on
hand-made pairs, and the argument errors of set_weights / read_rules that need
no device."""
import os

import numpy as np
import pytest

import mine_eval_ref
from conftest import GOLDEN
from rnnlogic_amd import miner as miner_mod


def read_split(path, name):
    def rd(f):
        with open(os.path.join(path, f)) as fi:
            return {ln.split()[1]: int(ln.split()[0]) for ln in fi if ln.strip()}
    e2i, r2i = rd("entities.dict"), rd("relations.dict")
    with open(os.path.join(path, name)) as fi:
        return [(e2i[h], r2i[r], e2i[t]) for h, r, t in (ln.split() for ln in fi if ln.strip())], len(e2i), len(r2i)


@pytest.mark.parametrize("data", ["kinship", "umls"])
def test_restatement_reproduces_the_reference(data):
    from rnnlogic_amd import datasets
    fx = mine_eval_ref.load_fixture(os.path.join(GOLDEN, "_mine_eval_%s.npz" % data))
    path = datasets.materialize(data)
    (train, E, R), (valid, _, _), (test, _, _) = (read_split(path, f) for f in ("train.txt", "valid.txt", "test.txt"))
    assert len(fx["rules"]) == R and max(len(x) for x in fx["rules"]) <= 40
    assert any(w == 0.0 for ws in fx["weights"] for w in ws) and any(w < 0.0 for ws in fx["weights"] for w in ws)
    ref = mine_eval_ref.MineEvalRef(train, E, R, known=train + valid + test)
    ref.set_rules(fx["rules"], fx["weights"])
    for split, triples in (("valid", valid), ("test", test)):
        want = fx["pairs"][split]
        assert len(want) == len(triples) and np.sum(want[:, 1] - want[:, 0] > 1) > 50  # tie runs are frequent
        got = ref.pairs(triples)
        assert np.array_equal(np.asarray(got, dtype=np.int64), want)
        assert np.asarray(mine_eval_ref.metrics(got, E)).tobytes() == fx["metrics"][split].tobytes()
        m = miner_mod.expectation_metrics(want, E)
        assert np.asarray([m[k] for k in mine_eval_ref.METRIC_NAMES]).tobytes() == fx["metrics"][split].tobytes()
        assert m["n"] == len(triples)


def test_expectation_metrics_by_hand():
    m = miner_mod.expectation_metrics([(0, 1)], 20)  # alone at rank 1
    assert (m["mr"], m["mrr"], m["hit1"], m["hit3"], m["hit10"], m["n"]) == (1.0, 1.0, 1.0, 1.0, 1.0, 1)
    m = miner_mod.expectation_metrics([(10, 11)], 20)  # alone at rank 11
    assert m["mr"] == 11.0 and abs(m["mrr"] - 1.0 / 11) < 1e-15 and (m["hit1"], m["hit3"], m["hit10"]) == (0, 0, 0)
    m = miner_mod.expectation_metrics([(1, 5)], 20)  # ranks 2..5, equally likely: the run crosses HITS@3
    assert m["mr"] == 3.5 and abs(m["mrr"] - (1 / 2 + 1 / 3 + 1 / 4 + 1 / 5) / 4) < 1e-15
    assert (m["hit1"], m["hit3"], m["hit10"]) == (0.0, 0.5, 1.0)
    m = miner_mod.expectation_metrics([(0, 20)], 20)  # every entity ties
    assert m["mr"] == 10.5 and m["hit1"] == 1 / 20 and m["hit3"] == 3 / 20 and m["hit10"] == 0.5
    pairs = [(0, 1), (10, 11), (1, 5), (0, 20), (8, 12)]
    m = miner_mod.expectation_metrics(np.asarray(pairs), 20)
    assert tuple(m[k] for k in mine_eval_ref.METRIC_NAMES) == mine_eval_ref.metrics(pairs, 20) and m["n"] == 5
    assert m["hit10"] == (1 + 0 + 1 + 0.5 + 0.5) / 5
    for bad in ([], [(3, 3)], [(0, 21)], [(-1, 2)]):
        with pytest.raises(ValueError):
            miner_mod.expectation_metrics(bad, 20)


def bare_miner(rule_off, n_relations):
    """A RuleMiner without a device handle: argument checks come before any device call."""
    import types
    m = object.__new__(miner_mod.RuleMiner)
    m._rule_off = np.asarray(rule_off, dtype=np.int32)
    m.graph = types.SimpleNamespace(relation_size=n_relations, entity_size=5)
    return m


def test_set_weights_argument_errors():
    m = bare_miner([0, 2, 2, 3], 3)
    for bad in ([[1.0, 2.0], []], [[1.0], [], [0.5]], [[1.0, 2.0], [], [0.5, 0.5]], [[1.0, float("nan")], [], [0.5]],
                [[1.0, 2.0], [], [float("inf")]]):
        with pytest.raises(ValueError):
            m.set_weights(bad)
    assert miner_mod.flatten_weights(m._rule_off, [[1.0, -2.0], [], np.asarray([0.5])]).tolist() == [1.0, -2.0, 0.5]


def test_read_rules_argument_errors(tmp_path):
    m = bare_miner([0, 0, 0, 0], 3)
    f = tmp_path / "rules.txt"
    for text in ("0 1 x\n", "0 3 0.5\n", "-1 1 0.5\n", "0 1 1 1 1 0.5\n", "0 1 nan\n", "0 1 inf\n", "0.5\n",
                 "0 1.5 2 0.5\n"):
        f.write_text("1 0 2 0.25\n" + text)
        with pytest.raises(ValueError):
            m.read_rules(str(f))
    with pytest.raises(OSError):
        m.read_rules(str(tmp_path / "missing.txt"))
    f.write_text("1 0 2 0.25\n\n1 2 -1e-3\n0 1\n2 0.5000000000000001\n1 0 2 0.25\n")
    rules, weights = miner_mod.read_rule_file(str(f), 3)
    assert rules == [[(0, (1,))], [(1, (0, 2)), (1, (2,)), (1, (0, 2))], [(2, ())]]
    assert weights == [[0.0], [0.25, -1e-3, 0.25], [0.5000000000000001]]
