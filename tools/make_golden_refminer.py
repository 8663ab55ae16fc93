"""Recorded outputs of the REFERENCE path counter (rule_destination of
miner/rnnlogic.cpp, through oracle/_ref/libref_miner.so) for
tests/test_oracle_c.py: tests/golden/_refminer_<case>.npz with
  q      (n, 3)   the train triples queried (h, r, t); (h, r, t) is also the removed edge
  ptr    (n + 1,) entries of query k are [ptr[k], ptr[k + 1])
  rid    (m,)     global rule id (file order) of an entry
  dest   (m,)     destination entity
  count  (m,)     paths from h to dest along that rule's body

Usage: python tools/make_golden_refminer.py   (needs the reference miner build)
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from conftest import Fixture  # noqa: E402
from oracle import ground_c  # noqa: E402
from oracle import reference_np as ref  # noqa: E402

CASES = ["umls_lstm_sum_bias", "kinship_lstm_sum_none", "fb_lstm_sum_bias"]
N_QUERIES = 12


def record(case):
    fx = Fixture(case)
    g = ref.Graph(fx.dataset_path())
    rules = ref.Rules(fx.rule_path(), g.relation_size)
    miner = ground_c.RefMiner(fx.dataset_path())
    facts = np.asarray(g.train_facts)
    qs = facts[np.random.RandomState(3).choice(len(facts), N_QUERIES, replace=False)]
    ptr, rid, dest, count = [0], [], [], []
    try:
        for h, r, t in qs.tolist():
            for k, (hd, body) in rules.relation2rules[r]:
                d, c = miner.rule_destination(h, body, (h, r, t))
                rid.append(np.full(len(d), k, np.int32))
                dest.append(d.copy())
                count.append(c.copy())
            ptr.append(sum(len(x) for x in rid))
    finally:
        miner.close()
    cat = lambda xs: np.concatenate(xs).astype(np.int32) if xs else np.zeros(0, np.int32)  # noqa: E731
    return dict(q=qs.astype(np.int32), ptr=np.asarray(ptr, np.int64), rid=cat(rid), dest=cat(dest), count=cat(count))


if __name__ == "__main__":
    for case in CASES:
        out = os.path.join(REPO, "tests", "golden", "_refminer_%s.npz" % case)
        z = record(case)
        np.savez_compressed(out, **z)
        print(out, len(z["q"]), "queries,", len(z["rid"]), "entries,", os.path.getsize(out), "bytes")
