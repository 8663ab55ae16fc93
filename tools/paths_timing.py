"""Times the predictors' explain_paths next to explain_rows on the same rows and
slots, in one process:
  - UMLS, PredictorPlus lstm / sum / bias, and kinship, PredictorPlus emb / pna /
    none, with the shipped mined rules: the LDS regime (|E| <= 512);
  - WN18RR, PredictorPlus emb / pna / bias, with datasets.rule_file("wn18rr"):
    the levels in the caller's scratch; and the same without an entity feature
    (wn18rr-none), where only rule-reached entities are listed.
Weights are seeded random ones: neither call reads them, they only choose the
places that predict_topk lists.

Rows: the whole test split.  Slots: the first 3 places of predict_topk(k=10);
rules: per slot the first 3 of explain_rows by (count descending, rule id
ascending), picked on the device (top_rules); P = 3 paths per rule.  Two
warm-up calls each, then the two calls alternate, each bracketed by device
events (both end with a read-back, so the host side is inside); median, minimum
and maximum over the repeats, in milliseconds.  explain_rows grounds every rule
of each row's relation and exports the COO; explain_paths grounds the distinct
trie nodes among the 9 named rules, one at a time with all levels kept;
`distinct_nodes_per_row` is their mean number.  The counts of the two calls
are checked to be equal.

    python tools/paths_timing.py [--repeats 20] [--data umls,kinship,wn18rr,wn18rr-none] [--out FILE]
prints one JSON line.  Needs a GPU.  Not part of bench.py; a record, not a test.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SLOTS, RULES, P = 3, 3, 3
MODELS = {
    "umls": dict(type="lstm", entity_feature="bias", aggregator="sum"),
    "kinship": dict(type="emb", entity_feature="none", aggregator="pna"),
    "wn18rr": dict(type="emb", entity_feature="bias", aggregator="pna"),
    # the same graph and rules without an entity feature: only rule-reached entities are listed, so every place
    # has rules to name (under a random bias row most of WN18RR's first places are entities no rule reaches)
    "wn18rr-none": dict(type="emb", entity_feature="none", aggregator="pna"),
}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def stats(ms):
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms))


def load(data, dev):
    from rnnlogic_amd import datasets
    from rnnlogic_amd.data import KnowledgeGraph
    from rnnlogic_amd.predictors import PredictorPlus
    name = data.split("-")[0]
    graph = KnowledgeGraph(datasets.materialize(name))
    torch.manual_seed(3)
    model = PredictorPlus(graph, **MODELS[data])
    model.set_rules(datasets.rule_file(name))
    if MODELS[data]["entity_feature"] == "bias":
        with torch.no_grad():
            model.bias.normal_()
    return graph, model.to(dev).eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--data", default="umls,kinship,wn18rr,wn18rr-none")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("paths_timing needs a GPU")
    dev = torch.device("cuda:0")
    result = dict(tool="paths_timing", repeats=args.repeats, slots=SLOTS, rules_per_slot=RULES, paths_per_rule=P,
                  runs={})
    for data in args.data.split(","):
        graph, model = load(data, dev)
        q = torch.from_numpy(np.asarray(graph.test_facts, dtype=np.int64).reshape(-1, 3)).to(dev)
        h, r = q[:, 0].contiguous(), q[:, 1].contiguous()
        n, E = h.numel(), graph.entity_size
        ents = model.predict_topk(h, r, 10)[0][:, :SLOTS].contiguous()
        off, rule, count = model.explain_rows(h, r, ents)
        # (as predict(paths=) names them: a listed rule without a body is left out, WN18RR's file has four)
        named = model.listable(model.top_rules(off, rule, count, RULES)).view(n, SLOTS, RULES)
        calls = dict(explain_rows=lambda: model.explain_rows(h, r, ents),
                     explain_paths=lambda: model.explain_paths(h, r, ents, named, P))
        for _ in range(args.warmup):
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        ms, out = {name: [] for name in calls}, {}
        for _ in range(args.repeats):  # alternating: both calls see the same neighbours on the machine
            for name, fn in calls.items():
                t, out[name] = timed(fn)
                ms[name].append(t)
        listed, pcount, path = out["explain_paths"]
        # the counts of the named rules, read from explain_rows' CSR on the host
        off_h, rule_h, count_h = [x.cpu().numpy() for x in out["explain_rows"]]
        named_h, pcount_h = named.cpu().numpy().reshape(n * SLOTS, RULES), pcount.cpu().numpy().reshape(n * SLOTS, RULES)
        for s in range(n * SLOTS):
            by_rule = dict(zip(rule_h[off_h[s]:off_h[s + 1]].tolist(), count_h[off_h[s]:off_h[s + 1]].tolist()))
            for k, c in zip(named_h[s].tolist(), pcount_h[s].tolist()):
                assert c == (by_rule[k] if k >= 0 else 0), (data, s, k, c)
        node_of_rule = model.native_rules(dev).node_of_rule.cpu().numpy()
        rows = named.cpu().numpy().reshape(n, -1)
        distinct = float(np.mean([len(set(node_of_rule[row[row >= 0]].tolist())) for row in rows]))
        med = {name: statistics.median(v) for name, v in ms.items()}
        result["runs"][data] = dict(
            model="PredictorPlus %(type)s / %(aggregator)s / %(entity_feature)s" % MODELS[data], rows=n, entities=E,
            rules=len(model.rules), regime="lds" if E <= 512 else "scratch", distinct_nodes_per_row=distinct,
            entries_with_paths=int((pcount > 0).sum()), entries_cut=int((pcount > P).sum()),
            paths_listed=int(listed.sum()), max_count=int(pcount.max()), explain_rows_ms=stats(ms["explain_rows"]),
            explain_paths_ms=stats(ms["explain_paths"]), paths_over_explain=med["explain_paths"] / med["explain_rows"])
        print("%s: done" % data, file=sys.stderr, flush=True)
        del model
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
