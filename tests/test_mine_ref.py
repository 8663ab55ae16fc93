"""tests/mine_ref.py (the fp64 restatement of the reference miner's learn /
H_score / pool update) against what the reference CLI printed with
`-threads 1` (tests/golden/_mine_*_L2.npz, tools/make_golden_mine.py).  CPU
only: this pins the restatement the GPU tests compare against."""
import os

import pytest

import mine_ref
from conftest import GOLDEN, golden_rules


@pytest.mark.parametrize("case", ["kinship_L2", "umls_L2"])
def test_mine_ref_reproduces_reference_cli(case):
    from rnnlogic_amd import datasets
    from rnnlogic_amd.data import KnowledgeGraph
    graph = KnowledgeGraph(datasets.materialize(case.split("_")[0]))
    R = graph.relation_size
    fx = mine_ref.load_fixture(os.path.join(GOLDEN, "_mine_%s.npz" % case), R)
    a = fx["args"]
    pool = [[] for _ in range(R)]
    for hd, body in golden_rules(a["pool"]):
        pool[hd].append((hd, body))
    H, _ = mine_ref.mine_replay(graph.train_facts, graph.entity_size, R, pool, fx["orders"], fx["selections"],
                                a["lr"], a["wd"], a["temp"], a["top_k"], a["portion"])
    assert len(fx["out_H"]) == sum(len(p) for p in pool)
    worst = max(abs(H[r][k] - h) for r, k, h in zip(fx["out_rel"], fx["out_idx"], fx["out_H"]))
    print("max |H(mine_ref) - H(reference)| = %.3g" % worst)
    assert worst <= 1e-15
    # the printed order is H descending within a relation, relations ascending
    for r in range(R):
        seq = fx["out_H"][fx["out_rel"] == r]
        assert len(seq) == fx["out_len"][r] and all(seq[i] >= seq[i + 1] for i in range(len(seq) - 1))
