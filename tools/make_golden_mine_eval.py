"""Golden runs of the REFERENCE miner's ReasoningPredictor::evaluate, one
thread: tests/golden/_mine_eval_<data>.npz for kinship and UMLS.

A fixture holds the rules (the first RULES_PER_RELATION rules with a body per
relation of data/<data>/mined_rules.txt, in file order), one float64 weight
per rule, and what the reference said for them: the (num_g, num_ge) pair of
every valid and test triple (int16) and the five metrics per split
(mr, mrr, hit1, hit3, hit10).  The weights are drawn from
{0, 0.5, 0.5, -0.25, N(0,1), 1e-3 N(0,1)}, the normal draws of every odd
relation rounded to quarters: zeros, repeats and negatives keep tie runs
frequent, which is what the fixture is for.

The reference has no command line for evaluate, so a small driver (DRIVER
below; it holds none of the reference's text) is compiled against the
reference sources where they lie, into a temporary directory, and run there:
it sets the rules, writes the weights through get_logic_rules(), calls
evaluate(test, 1) and reads `ranks` through a derived class.  Doubles cross the
process boundary as hex floats, so nothing is rounded.  Before anything is
written, tests/mine_eval_ref.py must reproduce every pair exactly and every
metric bitwise.

(The file names start with "_" because tests/conftest.py takes every other
.npz in tests/golden for a forward fixture.)

Usage: python tools/make_golden_mine_eval.py [reference miner directory]
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import mine_eval_ref  # noqa: E402
from rnnlogic_amd import datasets  # noqa: E402

RULES_PER_RELATION = 40
SEEDS = {"kinship": 11, "umls": 12}

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>
#include "rnnlogic.h"

struct Peek : public ReasoningPredictor {
  const std::vector<std::pair<int, int> > &pairs() const { return ranks; }
};

int main(int argc, char **argv) {
  if (argc != 4) return 2;
  KnowledgeGraph kg;
  kg.read_data(argv[1]);
  const int R = kg.get_relation_size();
  std::vector<Rule> *lists = new std::vector<Rule>[R];
  std::vector<std::vector<double> > w(R);
  FILE *fi = fopen(argv[2], "r");
  if (!fi) return 3;
  int head, len;
  while (fscanf(fi, "%d %d", &head, &len) == 2) {
    Rule rule;
    rule.r_head = head;
    rule.type = len;
    for (int k = 0; k < len; ++k) {
      int b;
      if (fscanf(fi, "%d", &b) != 1) return 4;
      rule.r_body.push_back(b);
    }
    double x;
    if (fscanf(fi, "%la", &x) != 1) return 4;
    lists[head].push_back(rule);
    w[head].push_back(x);
  }
  fclose(fi);
  Peek p;
  p.init_knowledge_graph(&kg);
  p.set_logic_rules(lists);
  std::vector<Rule> *own = p.get_logic_rules();
  for (int r = 0; r < R; ++r)
    for (size_t k = 0; k < own[r].size(); ++k) own[r][k].wt.data = w[r][k];
  FILE *fo = fopen(argv[3], "w");
  if (!fo) return 5;
  for (int test = 0; test < 2; ++test) {
    Result res = p.evaluate(test != 0, 1);
    fprintf(fo, "%s %a %a %a %a %a %d\n", test ? "test" : "valid", res.mr, res.mrr, res.h1, res.h3, res.h10,
            (int)p.pairs().size());
    for (size_t i = 0; i < p.pairs().size(); ++i) fprintf(fo, "%d %d\n", p.pairs()[i].first, p.pairs()[i].second);
  }
  fclose(fo);
  return 0;
}
"""


def read_graph(path):
    def rd(name):
        with open(os.path.join(path, name)) as fi:
            return {ln.split()[1]: int(ln.split()[0]) for ln in fi if ln.strip()}
    e2i, r2i = rd("entities.dict"), rd("relations.dict")

    def tri(name):
        with open(os.path.join(path, name)) as fi:
            return [(e2i[h], r2i[r], e2i[t]) for h, r, t in (ln.split() for ln in fi if ln.strip())]
    return tri("train.txt"), tri("valid.txt"), tri("test.txt"), len(e2i), len(r2i)


def pick_rules(data, R):
    rel2rules = [[] for _ in range(R)]
    with open(datasets.rule_file(data)) as fi:
        for line in fi:
            tok = line.split()
            if tok and "." in tok[-1]:
                tok = tok[:-1]
            ids = [int(x) for x in tok]
            if len(ids) >= 2 and len(rel2rules[ids[0]]) < RULES_PER_RELATION:
                rel2rules[ids[0]].append((ids[0], tuple(ids[1:])))
    return rel2rules


def draw_weights(rel2rules, seed):
    rng = np.random.default_rng(seed)
    out = []
    for r, rules in enumerate(rel2rules):
        kind = rng.integers(0, 6, len(rules))
        normal = rng.standard_normal(len(rules))
        if r % 2:
            normal = np.round(normal * 4) / 4
        w = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4],
                      [0.0, 0.5, 0.5, -0.25, normal], 1e-3 * normal)
        out.append([float(x) for x in w])
    return out


def run_reference(ref_dir, path, rel2rules, rel2weights):
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "driver.cpp"), os.path.join(tmp, "driver")
        with open(src, "w") as fo:
            fo.write(DRIVER)
        subprocess.run(["g++", "-O3", "-w", "-std=c++14", "-I" + ref_dir, src, os.path.join(ref_dir, "rnnlogic.cpp"),
                        "-o", exe, "-lpthread"], check=True)
        rules_txt, out_txt = os.path.join(tmp, "rules.txt"), os.path.join(tmp, "out.txt")
        with open(rules_txt, "w") as fo:
            for rules, ws in zip(rel2rules, rel2weights):
                for (hd, body), w in zip(rules, ws):
                    fo.write("%d %d%s %s\n" % (hd, len(body), "".join(" %d" % b for b in body), float(w).hex()))
        subprocess.run([exe, path, rules_txt, out_txt], check=True, stdout=subprocess.DEVNULL)
        with open(out_txt) as fi:
            lines = [ln.split() for ln in fi]
    out, k = {}, 0
    while k < len(lines):
        name, n = lines[k][0], int(lines[k][6])
        out[name] = (np.asarray([float.fromhex(x) for x in lines[k][1:6]], dtype=np.float64),
                     np.asarray([[int(a), int(b)] for a, b in lines[k + 1:k + 1 + n]], dtype=np.int64).reshape(-1, 2))
        k += 1 + n
    return out


def main():
    ref_dir = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/miner"
    for data in ("kinship", "umls"):
        path = datasets.materialize(data)
        train, valid, test, E, R = read_graph(path)
        rel2rules = pick_rules(data, R)
        rel2weights = draw_weights(rel2rules, SEEDS[data])
        ref = run_reference(ref_dir, path, rel2rules, rel2weights)
        ours = mine_eval_ref.MineEvalRef(train, E, R, known=train + valid + test)
        ours.set_rules(rel2rules, rel2weights)
        tied = {}
        for name, triples in (("valid", valid), ("test", test)):
            metrics, pairs = ref[name]
            assert len(pairs) == len(triples)
            got = np.asarray(ours.pairs(triples), dtype=np.int64)
            assert np.array_equal(got, pairs), "%s %s: mine_eval_ref's pairs differ from the reference's" % (data, name)
            mine = np.asarray(mine_eval_ref.metrics(got.tolist(), E), dtype=np.float64)
            assert mine.tobytes() == metrics.tobytes(), "%s %s: metrics differ: %r %r" % (data, name, mine, metrics)
            assert pairs.max() < 2 ** 15
            tied[name] = (int(np.sum(pairs[:, 1] - pairs[:, 0] > 1)), int(np.max(pairs[:, 1] - pairs[:, 0])))
        flat = [(hd, body) for rules in rel2rules for hd, body in rules]
        out = os.path.join(REPO, "tests", "golden", "_mine_eval_%s.npz" % data)
        np.savez_compressed(
            out, data=data, n_relations=np.int32(R),
            rule_head=np.asarray([hd for hd, _ in flat], dtype=np.int16),
            rule_len=np.asarray([len(b) for _, b in flat], dtype=np.int8),
            rule_body=np.asarray([list(b) + [0] * (3 - len(b)) for _, b in flat], dtype=np.int16).reshape(-1, 3),
            weights=np.asarray([w for ws in rel2weights for w in ws], dtype=np.float64),
            pairs_valid=ref["valid"][1].astype(np.int16), pairs_test=ref["test"][1].astype(np.int16),
            metrics_valid=ref["valid"][0], metrics_test=ref["test"][0])
        print("%s: %d rules, tied rows (count, longest run) %r, mrr valid %.6f test %.6f, %d bytes"
              % (out, len(flat), tied, ref["valid"][0][1], ref["test"][0][1], os.path.getsize(out)))


if __name__ == "__main__":
    main()
