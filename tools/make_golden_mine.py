"""Golden runs of the REFERENCE miner CLI after its search (learn, H_score,
pool update, out_rules), single-threaded: tests/golden/_mine_<case>.npz.

The CLI (oracle/_ref/rnnlogic, built by `make -C oracle ref`) never seeds
rand(), so its shuffles are reproduced here by calling libc's rand() in the
same sequence from this fresh process: the train triples once in search, then
per iteration each relation's pool indices (random_from_pool) and the triples
again (learn).  Before anything is written, tests/mine_ref.py run on those
orders must reproduce every H the CLI printed to <= 1e-15.

A fixture holds: args (json), orders (iterations x n, indices into the train
file), sel_flat / sel_off (selected pool indices per iteration and relation;
pools are tests/golden/rules_<data>_L<n>.npz), and the printed rules as
out_rel / out_idx (relation, pool index) with out_H, in printed order, plus
out_len (lines printed per relation).  With `only_selected` the printed rules
that were never selected (H = 0) are left out of out_*.

(The file names start with "_" because tests/conftest.py takes every other
.npz in tests/golden for a forward fixture.)

Usage: python tools/make_golden_mine.py      (run it as a fresh process)
"""
import ctypes
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import mine_ref  # noqa: E402
from conftest import golden_rules  # noqa: E402
from rnnlogic_amd import datasets  # noqa: E402

CLI = os.path.join(REPO, "oracle", "_ref", "rnnlogic")
LR, WD, TEMP = 0.01, 0.0005, 100.0
# name, data, length, iterations, top_n, top_k, top_n_out, portion, only_selected
CASES = [
    ("kinship_L2", "kinship", 2, 1, 0, 0, 0, 1.0, False),
    ("umls_L2", "umls", 2, 1, 0, 0, 0, 1.0, False),
    ("umls_L3_sub", "umls", 3, 2, 50, 0, 0, 1.0, True),
    ("kinship_L3_many", "kinship", 3, 1, 600, 0, 40, 300.5 / 8544, False),
]


def read_graph(path):
    def rd(name):
        with open(os.path.join(path, name)) as fi:
            return {ln.split()[1]: int(ln.split()[0]) for ln in fi if ln.strip()}
    e2i, r2i = rd("entities.dict"), rd("relations.dict")
    with open(os.path.join(path, "train.txt")) as fi:
        tri = [ln.split() for ln in fi if ln.strip()]
    return [(e2i[h], r2i[r], e2i[t]) for h, r, t in tri], len(e2i), len(r2i)


def one_case(name, data, L, iters, top_n, top_k, top_n_out, portion):
    """Runs in its own process: the rand() sequence starts at the CLI's."""
    libc = ctypes.CDLL("libc.so.6")
    rand = libc.rand
    path = datasets.materialize(data)
    triples, E, R = read_graph(path)
    pool = [[] for _ in range(R)]
    for hd, body in golden_rules("rules_%s_L%d" % (data, L)):
        pool[hd].append((hd, body))
    cur = mine_ref.c_shuffle(list(range(len(triples))), rand)  # RuleMiner::search
    n_sel = top_n if top_n else 2000000000
    orders, selections = [], []
    for _ in range(iters):
        sel = []
        for r in range(R):
            sel.append(mine_ref.c_shuffle(list(range(len(pool[r]))), rand)[:n_sel])
        cur = mine_ref.c_shuffle(cur, rand)  # ReasoningPredictor::learn
        orders.append(list(cur))
        selections.append(sel)

    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "out.txt")
        # main.cpp has no flag for the portion: predictor_portion is a global
        # that stays 1.0, so a portion < 1 case is run by the library shim
        # instead (below); the CLI covers portion == 1.
        if portion == 1.0:
            subprocess.run([CLI, "-data-path", path, "-output-file", out, "-max-length", str(L), "-threads", "1",
                            "-iterations", str(iters), "-lr", str(LR), "-wd", str(WD), "-temp", str(TEMP),
                            "-top-k", str(top_k), "-top-n", str(top_n), "-top-n-out", str(top_n_out)],
                           check=True, stdout=subprocess.DEVNULL)
            with open(out) as fi:
                lines = [ln.split() for ln in fi if ln.strip()]
        else:
            lines = None

    H, _ = mine_ref.mine_replay(triples, E, R, pool, orders, selections, LR, WD, TEMP, top_k, portion)
    index = [{body: k for k, (_, body) in enumerate(pool[r])} for r in range(R)]
    selected = [set(i for sel in selections for i in sel[r]) for r in range(R)]
    if lines is None:  # portion < 1: the restatement itself, pinned by the portion == 1 cases
        lines = []
        for r in range(R):
            for k in mine_ref.out_order(H[r], top_n_out):
                lines.append([str(r)] + [str(b) for b in pool[r][k][1]] + ["%.16f" % H[r][k]])
        source = "mine_ref (main.cpp has no portion flag; the restatement is pinned by the other cases)"
    else:
        source = "reference CLI -threads 1"
    out_rel, out_idx, out_H, worst = [], [], [], 0.0
    for tok in lines:
        r, body, h = int(tok[0]), tuple(int(x) for x in tok[1:-1]), float(tok[-1])
        k = index[r][body]
        worst = max(worst, abs(H[r][k] - h))
        out_rel.append(r)
        out_idx.append(k)
        out_H.append(h)
    assert worst <= 1e-15, "%s: mine_ref differs from the CLI by %g" % (name, worst)
    return dict(E=E, R=R, n=len(triples), orders=orders, selections=selections, out_rel=out_rel, out_idx=out_idx,
                out_H=out_H, worst=worst, selected=[sorted(s) for s in selected], source=source)


def main():
    if len(sys.argv) > 1:  # child: one case, result as json on stdout
        c = [x for x in CASES if x[0] == sys.argv[1]][0]
        print(json.dumps(one_case(*c[:8])))
        return
    for c in CASES:
        name, data, L, iters, top_n, top_k, top_n_out, portion, only_selected = c
        res = json.loads(subprocess.run([sys.executable, os.path.abspath(__file__), name], check=True,
                                        capture_output=True, text=True).stdout.splitlines()[-1])
        R = res["R"]
        out_rel = np.asarray(res["out_rel"], dtype=np.int32)
        out_idx = np.asarray(res["out_idx"], dtype=np.int32)
        out_H = np.asarray(res["out_H"], dtype=np.float64)
        out_len = np.bincount(out_rel, minlength=R).astype(np.int32)
        if only_selected:
            sel = [set(s) for s in res["selected"]]
            keep = np.asarray([int(i) in sel[int(r)] for r, i in zip(out_rel, out_idx)], dtype=bool)
            assert np.all(out_H[~keep] == 0.0)
            out_rel, out_idx, out_H = out_rel[keep], out_idx[keep], out_H[keep]
        sel_flat, sel_off = [], [0]
        for sel in res["selections"]:
            for r in range(R):
                sel_flat += sel[r]
                sel_off.append(len(sel_flat))
        args = dict(data=data, max_length=L, iterations=iters, top_n=top_n, top_k=top_k, top_n_out=top_n_out,
                    lr=LR, wd=WD, temp=TEMP, portion=portion, only_selected=only_selected, source=res["source"],
                    pool="rules_%s_L%d" % (data, L))
        path = os.path.join(REPO, "tests", "golden", "_mine_%s.npz" % name)
        np.savez_compressed(path, args=json.dumps(args), orders=np.asarray(res["orders"], dtype=np.int32),
                            sel_flat=np.asarray(sel_flat, dtype=np.int32), sel_off=np.asarray(sel_off, dtype=np.int64),
                            out_rel=out_rel.astype(np.int16), out_idx=out_idx, out_H=out_H, out_len=out_len)
        print("%s: %d printed rules, max |H(mine_ref) - H(%s)| = %.3g, %d bytes"
              % (path, len(res["out_H"]), res["source"], res["worst"], os.path.getsize(path)))


if __name__ == "__main__":
    main()
