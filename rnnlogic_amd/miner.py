"""RuleMiner: the reference miner (miner/main.cpp:27-49) on the GPU — the rule
search (RuleMiner::search, rnnlogic.cpp:505-589; rnnl_rule_search,
csrc/mine.hip), then one weight per rule learned by online Adam
(ReasoningPredictor::learn), the H score per rule (H_score), the pool's
running mean (RuleGenerator::update) and the rule file (out_rules)
(rnnl_miner_learn / rnnl_miner_h_score, csrc/mine_learn.hip).

    miner = RuleMiner(graph)            # graph: rnnlogic_amd.data.KnowledgeGraph; max_body=5: bodies up to 5
    rules = miner.search(max_length=3)  # [(head, body tuple)] in the reference's order
    miner.save("pool.txt")              # "type head body... H wt prior", as RuleMiner::save

    miner.mine(max_length=3, iterations=1, top_n=0, top_k=0, lr=0.01, wd=0.0005, temp=100)
    miner.out_rules("mined_rules.txt", top_n_out=0)    # "head body... H", H descending per relation

    miner.set_logic_rules(rel2rules)    # or step by step, as ReasoningPredictor
    miner.learn(lr, wd, temp); miner.h_score(top_k); miner.weights(); miner.H()

    miner.set_weights(rel2weights)      # or read_rules("mined_rules.txt"): rules + weights from a file
    miner.evaluate("test")              # dict(mr, mrr, hit1, hit3, hit10, n), as ReasoningPredictor::evaluate
    miner.eval_ranks(triples); miner.scores(triples)   # the (num_g, num_ge) pairs / the val rows behind it

    miner.predict_topk(queries, k=10)   # (h, r) or (h, r, t) -> device index, score, valid, position (filtered top-k)
    miner.explain(queries, index, 3)    # per listed tail: fired, total, the 3 rules that contribute most, their counts
    miner.predict("test", k=10, explain=3, output="pred.tsv")   # both, as numpy arrays and as a TSV file
    miner.explain_paths(queries, index, rule, 3)       # per listed rule: its first 3 grounding paths, their exact count
    miner.predict("test", k=10, explain=3, paths=2, output="pred.tsv")  # ... `rule:count:weight [a > x > b | ...]`

    miner.evaluate("test", side="both") # the two-sided protocol: tail pairs then head pairs, n = 2 x triples
    miner.predict_topk(queries, k=10, side="head")     # (h, r, t), h = -1 open: the first k heads of (?, r, t);
    miner.scores / eval_ranks / explain / predict(..., side="head")   # every call above on the head side

    miner.set_aggregation("noisy_or")   # or ("max", depth=1..3): how every query call above combines the rules that
    miner.set_weights(miner.confidence("pca"))         # reach an entity; weights are then confidences
    miner.score_value(score, r)         # a score as the value to show: the probability / the strongest rule's weight

    miner.rule_stats()                  # dict(support, body, pca_body): int64 per rule of the current lists (or of
    miner.pool_stats()                  # rel2rules given) / of the searched pool, in get_logic_rules() order
    miner.head_pairs(); miner.confidence("pca" | "std" | "head_coverage", pc=0.0)
    miner.mine(..., prior="pca", prior_weight=0.5)     # that confidence as the prior H_score weighs
    miner.out_rules(F, top_n_out, min_support=1, min_confidence=0.1, confidence="pca", pc=0.0)
    miner.out_rule_stats(S, top_n_out)  # "head body... H support body pca_body std pca" of the rules out_rules writes

    python -m rnnlogic_amd.miner -data-path D -output-file F -max-length 3 ...   # main.cpp's flags (-max-length 1..5)
    python -m rnnlogic_amd.miner -data-path D -output-file F ... -evaluate both  # + one metrics line per split
    python -m rnnlogic_amd.miner -data-path D -rule-file F -evaluate test        # evaluate a rule file, no mining
    python -m rnnlogic_amd.miner -data-path D -rule-file F -predict test -predictions-file P -k 10 -explain 3
    python -m rnnlogic_amd.miner -data-path D -rule-file F -queries-file Q -predictions-file P   # head<TAB>relation[<TAB>tail]
    python -m rnnlogic_amd.miner ... -predict test -explain 3 -paths 2 -predictions-file P    # + the paths behind each rule
    python -m rnnlogic_amd.miner -data-path D -rule-file F -evaluate test -side both   # tails, heads, both: a line each
    python -m rnnlogic_amd.miner -data-path D -rule-file F -predict test -side head -predictions-file P
    python -m rnnlogic_amd.miner ... -side head -queries-file Q -predictions-file P    # [head]<TAB>relation<TAB>tail
    python -m rnnlogic_amd.miner -data-path D -rule-file F -weights conf -agg noisy-or -evaluate test
    python -m rnnlogic_amd.miner ... -weights conf -conf pca -agg max -agg-depth 2 -predict test -predictions-file P

The pool equals the reference's for the same train graph: every relation
path of length <= max_length from h to t of a train triple (h, r, t), the
triple's own edge removed, as the rule r <- path; r <- r dropped; per head in
std::set<Rule> order (length, then body).  Bodies of up to three relations by
default; RuleMiner(graph, max_body=4 or 5) takes longer ones in search,
set_logic_rules, read_rules and mine (rnnl_rule_search_long: lengths 4 and 5
as the exact join of the forward paths from h with the length-2 suffixes into
t; at most 4,096 relations at length 4 and 1,024 at 5, the 64-bit key).  There
a triple with h == t gives the reference's one rule without a body;
search(max_length <= 3) walks on from such a triple, as it always did.

learn / h_score compute what the reference computes with one thread: a pure
function of the triple order (its multi-threaded run races on the weights and
is not reproducible), in fp64, bitwise repeatable and independent of how the
triples are cut into chunks.  The orders and rule subsets are drawn from
seeded numpy generators, or given (`orders`, `selections`) to replay a
reference run.  Where the reference leaves ties to std::sort they are defined
here: top-k by val descending then position in the rule list, out_rules by H
descending then pool order.

evaluate (ReasoningPredictor::evaluate, rnnlogic.cpp:968-1120) ranks the tail
of held-out triples by sum_k wt[k] * #paths on the train graph with the
triple's own edge removed (rnnl_miner_evaluate, csrc/mine_eval.hip).  The
scores are the reference's bit for bit (fp64, product then add, rule list
order per entity) and the two counts per triple — entities scoring above the
tail, and at least as high — are exact, so the expectation over the tie run
gives the reference's MR / MRR / HITS.

predict_topk / explain / predict answer a query with the same scores
(rnnl_miner_predict / rnnl_miner_explain, csrc/mine_predict.hip): the first k
tails by val descending, then entity id, among the entities some rule reaches
(or all), the other known tails of (h, r) left out; and per listed tail the
rules with a path to it, their counts and the ones that contribute most.  The
top k are selected inside the workgroup that built val, so the (n, |E|)
matrix of `scores` is never written.

explain_paths (rnnl_miner_paths_side, csrc/mine_paths.hip) shows
the paths a count stands for: per (query, listed entity, rule) the exact number
of grounding paths and the first few of them as entity sequences, ordered by
their entities read from the listed entity back toward the query's anchor.  It
counts paths whatever aggregation is set.

set_aggregation replaces the sum in all of these by the two
aggregations that belong to confidences: noisy-or, val[e] = sum of
-log1p(-w_k) over the rules that reach e, and max, val[e] = a key of the
strongest (and, at depth 2 and 3, next strongest) rules that reach e.  Both ask
only whether a rule reaches an entity, so no path count can pass 32 bits.

side="head" answers (?, r, t) with the same rules: val[e] =
sum_k wt[k] * #paths(e -> t along body k), grounded backward from t over the
in-edges with the triple's own edge removed, the other known heads of (r, t)
left out.  It is bit for bit the tail side of (t, r, h) on the transposed graph
with every body reversed.  evaluate(side="both") is the two-sided filtered
protocol: the tail pairs of all triples, then the head pairs, as one list.
"""
import ctypes
import math

import numpy as np
import torch

from . import _native


def flatten_weights(rule_off, rel2weights):
    """One float64 sequence per relation, of the lengths of the rule lists
    (rule_off: R + 1 offsets) -> the flat float64 array in list order."""
    R = len(rule_off) - 1
    if len(rel2weights) != R:
        raise ValueError("set_weights: one weight sequence per relation expected (%d, got %d)"
                         % (R, len(rel2weights)))
    flat = np.zeros(int(rule_off[-1]), dtype=np.float64)
    for r, w in enumerate(rel2weights):
        w = np.asarray(w, dtype=np.float64).reshape(-1)
        if len(w) != int(rule_off[r + 1] - rule_off[r]):
            raise ValueError("set_weights: relation %d has %d rules, got %d weights"
                             % (r, int(rule_off[r + 1] - rule_off[r]), len(w)))
        if not np.all(np.isfinite(w)):
            raise ValueError("set_weights: a weight of relation %d is not finite" % r)
        flat[int(rule_off[r]):int(rule_off[r + 1])] = w
    return flat


MAX_BODY = 5  # the longest body the native miner holds (RULE_STRIDE, csrc/internal.h)


def _check_max_body(max_body):
    if max_body not in (3, 4, 5):
        raise ValueError("max_body must be 3, 4 or 5 (got %r)" % (max_body,))
    return int(max_body)


def _too_long(what, max_body):
    if max_body < MAX_BODY:
        return "%s: rule bodies have at most %d relations (raise the limit with max_body=, up to %d)" % (
            what, max_body, MAX_BODY)
    return "%s: rule bodies have at most %d relations" % (what, max_body)


def long_key_bits(n_relations, max_length):
    """Bits per relation of a long rule key (rnnl_rule_key_bits): max(1,
    ceil(log2 R)); raises the native RNNL_ERR_INVALID, naming the bound, unless
    3 + (max_length + 1) * bits <= 64."""
    bits = ctypes.c_int32()
    _native.call("rnnl_rule_key_bits", int(n_relations), int(max_length), ctypes.byref(bits))
    return bits.value


def encode_long(rules, n_relations, max_length):
    """[(head, body)] -> long rule keys (numpy uint64): head | len (3 bits) |
    b1 .. b_max_length, `long_key_bits` per relation, bodies left-aligned."""
    bits = long_key_bits(n_relations, max_length)
    keys = np.zeros(len(rules), dtype=np.uint64)
    for i, (hd, body) in enumerate(rules):
        if len(body) > max_length:
            raise ValueError("encode_long: a body of %d relations in keys of max_length %d" % (len(body), max_length))
        k = ((int(hd) << 3) | len(body)) << (max_length * bits)
        for j, b in enumerate(body):
            k |= int(b) << ((max_length - 1 - j) * bits)
        keys[i] = k
    return keys


def unpack_long(keys, n_relations, max_length):
    """long rule keys -> (head int64, length int32, body int32 (n, max_length)), in the order given."""
    bits = long_key_bits(n_relations, max_length)
    keys = np.asarray(keys, dtype=np.uint64)
    m = np.uint64((1 << bits) - 1)
    top = keys >> np.uint64(max_length * bits)
    body = np.stack([(keys >> np.uint64((max_length - 1 - j) * bits)) & m for j in range(max_length)], 1)
    return (top >> np.uint64(3)).astype(np.int64), (top & np.uint64(7)).astype(np.int32), body.astype(np.int32)


def read_rule_file(file_name, n_relations, max_body=3):
    """A rule file of 'head body... x' lines (out_rules / mined_rules.txt) ->
    (rel2rules, rel2weights) in file order per head.  A last token that is not
    an integer is x, the weight; a line of integers alone has weight 0.  A body
    of more than max_body (3..5) relations is refused."""
    max_body = _check_max_body(max_body)
    rel2rules = [[] for _ in range(n_relations)]
    rel2weights = [[] for _ in range(n_relations)]
    with open(file_name) as fi:
        for no, line in enumerate(fi, 1):
            tok = line.split()
            if not tok:
                continue
            x = 0.0
            try:
                int(tok[-1])
            except ValueError:
                try:
                    x = float(tok[-1])
                except ValueError:
                    raise ValueError("%s:%d: %r is not a number" % (file_name, no, tok[-1]))
                tok = tok[:-1]
            try:
                ids = [int(v) for v in tok]
            except ValueError:
                raise ValueError("%s:%d: relation ids must be integers" % (file_name, no))
            if not ids:
                raise ValueError("%s:%d: no head relation" % (file_name, no))
            if any(v < 0 or v >= n_relations for v in ids):
                raise ValueError("%s:%d: relation id out of range [0, %d)" % (file_name, no, n_relations))
            if len(ids) > max_body + 1:
                raise ValueError(_too_long("%s:%d" % (file_name, no), max_body))
            if not math.isfinite(x):
                raise ValueError("%s:%d: the weight is not finite" % (file_name, no))
            rel2rules[ids[0]].append((ids[0], tuple(ids[1:])))
            rel2weights[ids[0]].append(x)
    return rel2rules, rel2weights


def expectation_metrics(ranks, n_entities):
    """ReasoningPredictor::evaluate's metrics (rnnlogic.cpp:1070-1116) of
    (num_g, num_ge) pairs: the true tail is equally likely at every rank of
    its tie run num_g + 1 .. num_ge, so each metric is the mean of its table
    over the run — cumulative tables, then one sum in triple order, in fp64 as
    the reference.  Returns dict(mr, mrr, hit1, hit3, hit10, n)."""
    ranks = np.asarray(ranks, dtype=np.int64).reshape(-1, 2)
    if len(ranks) == 0:
        raise ValueError("expectation_metrics: no ranks")
    E = int(n_entities)
    if np.any(ranks[:, 0] < 0) or np.any(ranks[:, 1] <= ranks[:, 0]) or np.any(ranks[:, 1] > E):
        raise ValueError("expectation_metrics: pairs must satisfy 0 <= num_g < num_ge <= n_entities")
    t_mr, t_mrr, t_h1, t_h3, t_h10 = ([0.0] * (E + 1) for _ in range(5))
    for rank in range(1, E + 1):
        t_mr[rank] = float(rank) + t_mr[rank - 1]
        t_mrr[rank] = 1.0 / rank + t_mrr[rank - 1]
        t_h1[rank] = (1.0 if rank <= 1 else 0.0) + t_h1[rank - 1]
        t_h3[rank] = (1.0 if rank <= 3 else 0.0) + t_h3[rank - 1]
        t_h10[rank] = (1.0 if rank <= 10 else 0.0) + t_h10[rank - 1]
    mr = mrr = hit1 = hit3 = hit10 = 0.0
    for g, ge in ranks.tolist():
        run = float(ge - g)
        mr += (t_mr[ge] - t_mr[g]) / run
        mrr += (t_mrr[ge] - t_mrr[g]) / run
        hit1 += (t_h1[ge] - t_h1[g]) / run
        hit3 += (t_h3[ge] - t_h3[g]) / run
        hit10 += (t_h10[ge] - t_h10[g]) / run
    n = float(len(ranks))
    return dict(mr=mr / n, mrr=mrr / n, hit1=hit1 / n, hit3=hit3 / n, hit10=hit10 / n, n=len(ranks))


def metrics_line(name, m):
    return "%s | MR %.6f MRR %.6f HITS@1 %.6f @3 %.6f @10 %.6f" % (name, m["mr"], m["mrr"], m["hit1"], m["hit3"],
                                                                  m["hit10"])


def _name(graph, table, i):
    """The dictionary name of id i (graph.id2entity / id2relation), or the id itself where the graph has none."""
    names = getattr(graph, table, None)
    try:
        return str(names[i])
    except (TypeError, KeyError, IndexError):
        return str(i)


def _check_side(side, what, both=False):
    if side not in (("tail", "head", "both") if both else ("tail", "head")):
        raise ValueError("%s: side must be 'tail'%s 'head'%s (got %r)"
                         % (what, "," if both else " or", " or 'both'" if both else "", side))
    return side


def _side_code(side):
    """The native RNNL_MINER_TAIL / RNNL_MINER_HEAD of a checked side."""
    return _native.MINER_HEAD if side == "head" else _native.MINER_TAIL


def _known_args(lists):
    """The native (known_keys, known_offs, known_vals, n_keys) of _DeviceLists, or of None: unfiltered."""
    if lists is None:
        return None, None, None, 0
    return lists.keys.data_ptr(), lists.offs.data_ptr(), lists.vals.data_ptr(), lists.keys.numel()


def read_queries_file(file_name, graph, side="tail"):
    """Lines `head<TAB>relation` (open) or `head<TAB>relation<TAB>tail`, in the
    names of the graph's dictionaries -> (n, 3) int64 with t = -1 for the open
    ones.  side 'head': `head<TAB>relation<TAB>tail`, or `<TAB>relation<TAB>tail`
    (an empty first field) for an open query, h = -1.  An unknown name or a
    malformed line is a ValueError naming the line."""
    head = _check_side(side, "read_queries_file") == "head"
    out = []
    with open(file_name) as fi:
        for no, line in enumerate(fi, 1):
            line = line.rstrip("\r\n")
            if not line.strip():
                continue
            tok = line.split("\t")
            if head and len(tok) != 3:
                raise ValueError("%s:%d: expected head<TAB>relation<TAB>tail or <TAB>relation<TAB>tail (head queries)"
                                 % (file_name, no))
            if len(tok) not in (2, 3):
                raise ValueError("%s:%d: expected head<TAB>relation or head<TAB>relation<TAB>tail" % (file_name, no))
            open_head = head and tok[0] == ""
            if not open_head and tok[0] not in graph.entity2id:
                raise ValueError("%s:%d: unknown entity %r" % (file_name, no, tok[0]))
            if tok[1] not in graph.relation2id:
                raise ValueError("%s:%d: unknown relation %r" % (file_name, no, tok[1]))
            if len(tok) == 3 and tok[2] not in graph.entity2id:
                raise ValueError("%s:%d: unknown entity %r" % (file_name, no, tok[2]))
            out.append((-1 if open_head else graph.entity2id[tok[0]], graph.relation2id[tok[1]],
                        graph.entity2id[tok[2]] if len(tok) == 3 else -1))
    return np.asarray(out, dtype=np.int64).reshape(-1, 3)


def group_rules(head, ln, body, n_relations):
    """Rules as arrays (head (n,), length (n,), body (n, w <= MAX_BODY)) ->
    what rnnl_miner_rule_stats takes and the way back: (body_len (nb,) int32,
    body_rel (nb, MAX_BODY) int32, head_off (nb + 1,) int32, head_rel int32,
    body_of (n,), slot_of (n,)).  Every distinct body once, per body its
    distinct heads ascending; rule i reads body count body_of[i] and
    (support, pca_body) slot slot_of[i], so a (head, body) listed twice reads
    the same slot twice."""
    head = np.asarray(head, dtype=np.int64).reshape(-1)
    ln = np.asarray(ln, dtype=np.int64).reshape(-1)
    n, R = len(head), max(int(n_relations), 1)
    wide = np.zeros((n, MAX_BODY), dtype=np.int64)
    body = np.asarray(body, dtype=np.int64).reshape(n, -1)
    wide[:, :body.shape[1]] = body
    wide[np.arange(MAX_BODY)[None, :] >= ln[:, None]] = 0  # whatever lies past a body's end does not tell bodies apart
    if (MAX_BODY + 1) * R ** MAX_BODY < 2 ** 62:
        key = ln.copy()
        for j in range(MAX_BODY):
            key = key * R + wide[:, j]
        ukey, first, body_of = np.unique(key, return_index=True, return_inverse=True)
        ub = np.concatenate([ln[first, None], wide[first]], 1)
    else:
        ub, body_of = np.unique(np.concatenate([ln[:, None], wide], 1), axis=0, return_inverse=True)
    body_of = body_of.reshape(-1)
    nb = len(ub)
    uslot, slot_of = np.unique(body_of * R + head, return_inverse=True)
    head_off = np.searchsorted(uslot // R, np.arange(nb + 1)).astype(np.int32)
    return (np.ascontiguousarray(ub[:, 0], dtype=np.int32), np.ascontiguousarray(ub[:, 1:], dtype=np.int32), head_off,
            np.ascontiguousarray(uslot % R, dtype=np.int32), body_of, slot_of.reshape(-1))


def confidence_of(support, denominator, pc=0.0):
    """support / (denominator + pc) in fp64, 0 / 0 = 0.0 (pc >= 0: AnyBURL's pessimistic constant)."""
    if not pc >= 0.0:
        raise ValueError("pc must be >= 0 (got %r)" % (pc,))
    sup = np.asarray(support, dtype=np.float64)
    den = np.asarray(denominator, dtype=np.float64) + float(pc)
    out = np.zeros(sup.shape, dtype=np.float64)
    np.divide(sup, den, out=out, where=den > 0.0)
    return out


def confidences(kind, support, body, pca_body, head_pairs, pc=0.0):
    """'std': support / (body + pc); 'pca': support / (pca_body + pc);
    'head_coverage': support / head_pairs (of the rule's head)."""
    if kind == "std":
        return confidence_of(support, body, pc)
    if kind == "pca":
        return confidence_of(support, pca_body, pc)
    if kind == "head_coverage":
        return confidence_of(support, head_pairs, 0.0)
    raise ValueError("confidence: kind must be 'std', 'pca' or 'head_coverage' (got %r)" % (kind,))


def keep_rules(support, conf, min_support=0, min_confidence=0.0):
    """The filter of best_rules / out_rules: True where a rule stays."""
    return (np.asarray(support) >= min_support) & (np.asarray(conf) >= min_confidence)


def path_text(path_row, graph=None):
    """One row of explain_paths' `path` (x_0 .. x_L, -1 past x_L) as `a > x > b`:
    entity names from the graph's dictionary, the ids themselves without a graph."""
    return " > ".join(_name(graph, "id2entity", int(x)) for x in path_row if int(x) >= 0)


AGGREGATIONS = ("sum", "noisy_or", "max")
MAX_CLASSES = _native.MINER_AGG_CLASS_MAX  # 131,071: three 17-bit classes fit the 51 bits of a max key
_NOISY_OR_CAP = 1.0 - 2.0 ** -53           # the largest double below 1: a confidence of 1 stays finite


def _per_relation_weights(weights):
    return [np.asarray(w, dtype=np.float64).reshape(-1) for w in weights]


def noisy_or_operand(weights):
    """weights[r][k] in [0, 1] (confidences, one sequence per relation) -> per
    relation the float64 array u_k = -log1p(-min(w_k, 1 - 2^-53)): the operand
    of the noisy-or aggregation, whose score is the sum of u_k over the firing
    rules = -log prod(1 - w_k).  Each element is math.log1p's (the C
    library's), so a plain Python restatement reproduces it bitwise whatever
    vector path numpy's own log1p takes.  A weight outside [0, 1] (or NaN) is a
    ValueError naming relation and rule index."""
    out = []
    for r, w in enumerate(_per_relation_weights(weights)):
        bad = np.flatnonzero(~((w >= 0.0) & (w <= 1.0)))
        if len(bad):
            raise ValueError("noisy_or: the weight %r of rule %d of relation %d is not in [0, 1]"
                             % (float(w[bad[0]]), int(bad[0]), r))
        out.append(np.asarray([-math.log1p(-min(x, _NOISY_OR_CAP)) for x in w.tolist()], dtype=np.float64))
    return out


def max_classes(weights):
    """weights[r][k] finite and >= 0 -> (classes, values): per relation the
    int64 class of each rule and the ascending distinct positive weights.
    values[r][c - 1] is the weight of class c = 1..C; equal weights share a
    class; a weight of 0 has class 0, which contributes nothing.  A negative or
    non-finite weight, or more than 131,071 classes in a relation, is a
    ValueError naming the relation (and the rule index)."""
    classes, values = [], []
    for r, w in enumerate(_per_relation_weights(weights)):
        bad = np.flatnonzero(~((w >= 0.0) & np.isfinite(w)))
        if len(bad):
            raise ValueError("max: the weight %r of rule %d of relation %d is not finite and >= 0"
                             % (float(w[bad[0]]), int(bad[0]), r))
        vals = np.unique(w[w > 0.0])
        if len(vals) > MAX_CLASSES:
            raise ValueError("max: relation %d has %d distinct positive weights, more than the %d classes a key holds"
                             % (r, len(vals), MAX_CLASSES))
        cls = np.where(w > 0.0, np.searchsorted(vals, w) + 1, 0).astype(np.int64)
        classes.append(cls)
        values.append(vals)
    return classes, values


def decode_max(score, values):
    """A max score (the key c1 * 2^34 + c2 * 2^17 + c3 as a double) and the
    relation's `values` of max_classes -> an array (..., 3) of the weights of
    the strongest, second and third strongest firing rule, 0.0 for an empty
    position.  A score that is no key of these classes is a ValueError."""
    s = np.asarray(score, dtype=np.float64)
    table = np.concatenate([[0.0], np.asarray(values, dtype=np.float64).reshape(-1)])
    if not np.all((s >= 0.0) & (s < 2.0 ** 51) & (np.floor(s) == s)):
        raise ValueError("decode_max: a score is not a max key (an integer in [0, 2^51))")
    k = s.astype(np.uint64)
    c = np.stack([k >> np.uint64(34), (k >> np.uint64(17)) & np.uint64(0x1FFFF), k & np.uint64(0x1FFFF)],
                 -1).astype(np.int64)
    if c.size and int(c.max()) >= len(table):
        raise ValueError("decode_max: class %d in a score, the relation has %d" % (int(c.max()), len(table) - 1))
    return table[c]


def noisy_or_probability(score):
    """The probability 1 - prod(1 - w_k) behind a noisy-or score: -expm1(-score)."""
    return -np.expm1(-np.asarray(score, dtype=np.float64))


def _check_agg(agg, depth, what="set_aggregation"):
    agg = {"noisy-or": "noisy_or"}.get(agg, agg)
    if agg not in AGGREGATIONS:
        raise ValueError("%s: agg must be 'sum', 'noisy_or' or 'max' (got %r)" % (what, agg))
    if isinstance(depth, bool) or int(depth) != depth or not 1 <= int(depth) <= 3:
        raise ValueError("%s: depth must be 1, 2 or 3 (got %r)" % (what, depth))
    return agg, int(depth)


def stats_line(head, body, x, support, body_size, pca_body, std, pca):
    return "%d%s %.16f %d %d %d %.16f %.16f\n" % (head, "".join(" %d" % b for b in body), x, support, body_size,
                                                  pca_body, std, pca)


class RuleMiner(object):
    max_body = 3  # the longest rule body search / set_logic_rules / read_rules / mine take; 3..5 per miner
    _agg, _agg_depth, _agg_stale, _agg_values, _rules_set = "sum", 1, False, None, False  # set_aggregation

    def __init__(self, graph, device=None, max_body=3):
        self.graph = graph
        self.max_body = _check_max_body(max_body)
        self.suffix_cap = 0           # long search: length-2 suffixes of a tail sorted in LDS (0: the most, 2,048)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        hrt = np.ascontiguousarray(np.asarray(graph.train_facts, dtype=np.int32).reshape(-1, 3))
        self._handle = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _native.call("rnnl_miner_create", hrt.ctypes.data, len(hrt), graph.entity_size, graph.relation_size,
                         ctypes.byref(self._handle))
        self.rules = []
        self.table_bits = 22
        self._hrt = hrt
        self._searched = None
        self._counters = torch.zeros(4, dtype=torch.int64, device=self.device)
        self._rng = np.random.default_rng(0)  # triple orders of learn() calls without one
        self._order = None
        self._rule_off = np.zeros(graph.relation_size + 1, dtype=np.int32)
        self._grounded = None
        self.pool, self.pool_H = None, None
        self.chunk_triples = None     # triples per grounding chunk; None: as many as budget_bytes allows
        self.budget_bytes = 1 << 30   # device memory for one chunk's (triple, rule, destination, count) entries
        self._known = None            # known tails over train + valid + test (eval_ranks), built once
        self._known_h = None          # known heads, the same
        self._rule_len = np.zeros(0, dtype=np.int32)       # the current rule lists, as _set_rule_arrays got them
        self._rule_body = np.zeros((0, 3), dtype=np.int32)
        self._pool_stats = None       # pool_stats() of the searched pool, until the next search
        self._head_pairs = None
        self._agg, self._agg_depth = "sum", 1   # set_aggregation: sticky over new rules and weights
        self._agg_stale = False       # the handle's mode / operand no longer follow the current rules and weights
        self._agg_values = None       # max: per relation the ascending distinct positive weights (decode_max)
        self._rules_set = False

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h is not None and h.value:
            try:
                _native.lib().rnnl_miner_destroy(h)
            except Exception:
                pass

    @staticmethod
    def decode(keys, n_relations=None, max_length=None):
        """rule keys (head<<47 | len<<45 | b1<<30 | b2<<15 | b3) -> [(head, body)] in key order.
        With n_relations and max_length (4 or 5): the long keys of search_keys(max_length)."""
        keys = np.sort(np.asarray(keys, dtype=np.uint64))
        if max_length is not None and max_length > 3:
            head, ln, b = unpack_long(keys, n_relations, max_length)
            b = b.tolist()
            return [(hd, tuple(b[i][:n])) for i, (hd, n) in enumerate(zip(head.tolist(), ln.tolist()))]
        m = np.uint64(0x7FFF)
        head = (keys >> np.uint64(47)).astype(np.int64)
        ln = ((keys >> np.uint64(45)) & np.uint64(3)).astype(np.int64)
        b = np.stack([(keys >> np.uint64(30)) & m, (keys >> np.uint64(15)) & m, keys & m], 1).astype(np.int64)
        return [(int(hd), tuple(int(x) for x in b[i, :n])) for i, (hd, n) in enumerate(zip(head, ln))]

    @torch.no_grad()
    def search_keys(self, max_length):
        """Device search; returns the distinct rule keys (numpy uint64, unsorted):
        the keys of decode() for max_length <= 3, the long keys (unpack_long)
        for 4 and 5."""
        if max_length > self.max_body:
            raise ValueError(_too_long("search(%d)" % max_length, self.max_body))
        long_form = max_length > 3
        if long_form:
            long_key_bits(self.graph.relation_size, max_length)  # RNNL_ERR_INVALID before anything is allocated
        stream = torch.cuda.current_stream(self.device).cuda_stream
        counters = torch.zeros(4, dtype=torch.int64, device=self.device)
        while True:
            cap = 1 << self.table_bits
            if long_form and 16 * cap > self.budget_bytes:
                raise RuntimeError("rule search: the rule set needs a table of 2 x %d bytes, past budget_bytes = %d"
                                   % (8 * cap, self.budget_bytes))
            table = torch.empty(cap, dtype=torch.int64, device=self.device)
            out = torch.empty(cap, dtype=torch.int64, device=self.device)
            if long_form:
                with torch.cuda.device(self.device):
                    _native.call("rnnl_rule_search_long", self._handle, int(max_length), int(self.suffix_cap),
                                 table.data_ptr(), cap, out.data_ptr(), cap, counters.data_ptr(), stream)
            else:
                _native.call("rnnl_rule_search", self._handle, int(max_length), table.data_ptr(), cap, out.data_ptr(),
                             cap, counters.data_ptr(), stream)
            c = counters.cpu().tolist()
            if c[1] == 0 and c[2] <= cap // 2:
                return out[:c[2]].cpu().numpy().view(np.uint64)
            self.table_bits += 1  # keep the open-addressing set at most half full
            if self.table_bits > 31:
                raise RuntimeError("rule search: rule set too large")

    def search(self, max_length):
        """RuleMiner::search over all train triples (portion 1)."""
        keys = np.sort(self.search_keys(max_length))
        self._searched = max_length
        self._pool_stats = None
        if max_length > 3:
            self.rules = self.decode(keys, self.graph.relation_size, max_length)
            head, ln, body = unpack_long(keys, self.graph.relation_size, max_length)
            wide = np.zeros((len(keys), MAX_BODY), dtype=np.int32)
            wide[:, :max_length] = body
            self._pool_arrays = (head, ln, wide)
            return self.rules
        self.rules = self.decode(keys)
        m = np.uint64(0x7FFF)
        self._pool_arrays = ((keys >> np.uint64(47)).astype(np.int64),  # head, length, body of self.rules
                             ((keys >> np.uint64(45)) & np.uint64(3)).astype(np.int32),
                             np.stack([(keys >> np.uint64(30)) & m, (keys >> np.uint64(15)) & m, keys & m],
                                      1).astype(np.int32))
        return self.rules

    def get_logic_rules(self):
        """Per head relation, its rules in order (RuleMiner::get_logic_rules)."""
        rel2rules = [[] for _ in range(self.graph.relation_size)]
        for hd, body in self.rules:
            rel2rules[hd].append((hd, body))
        return rel2rules

    # ------------------------------------------------- weights and H scores
    def set_logic_rules(self, rel2rules, priors=None):
        """ReasoningPredictor::set_logic_rules: rel2rules[r] = [(head, body)]
        are relation r's rules, in list order; weights, Adam state and H are
        cleared.  priors[r][k] (default 0) enters h_score with prior_weight.
        Bodies hold at most max_body relations."""
        R = self.graph.relation_size
        width = 3 if self.max_body == 3 else MAX_BODY
        if len(rel2rules) != R:
            raise ValueError("set_logic_rules: one rule list per relation expected")
        off, ln, body, pr = [0], [], [], []
        for r, rules in enumerate(rel2rules):
            for k, (hd, b) in enumerate(rules):
                if int(hd) != r:
                    raise ValueError("set_logic_rules: rule with head %d in the list of relation %d" % (hd, r))
                if len(b) > self.max_body:
                    raise ValueError(_too_long("set_logic_rules", self.max_body))
                ln.append(len(b))
                body.append([int(x) for x in b] + [0] * (width - len(b)))
                pr.append(float(priors[r][k]) if priors is not None else 0.0)
            off.append(len(ln))
        self._set_rule_arrays(off, ln, np.asarray(body, dtype=np.int32).reshape(-1, width), pr)

    def _set_rule_arrays(self, off, ln, body, prior):
        self._rule_off = np.ascontiguousarray(off, dtype=np.int32)
        ln = np.ascontiguousarray(ln, dtype=np.int32)
        body = np.ascontiguousarray(body, dtype=np.int32)
        pr = np.ascontiguousarray(prior, dtype=np.float64)
        self._rule_len, self._rule_body = ln, body
        self._rules_set = self._agg_stale = True  # (the native call puts the handle back to the sum)
        entry = "rnnl_miner_set_rules" if body.shape[1] == 3 else "rnnl_miner_set_rules_long"  # n x 3 / n x 5
        with torch.cuda.device(self.device):
            _native.call(entry, self._handle, self._rule_off.ctypes.data, ln.ctypes.data, body.ctypes.data,
                         pr.ctypes.data)
        self._grounded = None

    def _use_order(self, order, portion):
        n = len(self._hrt)
        if order is None:
            order = self._order if self._order is not None else self._rng.permutation(n)
        order = np.ascontiguousarray(order, dtype=np.int32)
        if order.shape != (n,) or not np.array_equal(np.sort(order), np.arange(n, dtype=np.int32)):
            raise ValueError("order must be a permutation of range(%d), the train triples" % n)
        self._order = order
        return order, int(n * portion)

    def _counted(self, entry, *args):
        """A native entry that ends in (counters, stream): on the current
        stream with the miner's counters, which are then read and checked.
        Returns the first counter, the entries of rnnl_miner_ground_count."""
        _native.call(entry, self._handle, *args, self._counters.data_ptr(),
                     torch.cuda.current_stream(self.device).cuda_stream)
        return self._check_counters()

    def _ground(self, order_dev, begin, count, pair_base):
        """The (triple, rule, destination, count) entries of one chunk, or
        None if they would exceed the byte budget and the chunk can be cut."""
        n_pairs = int(pair_base[-1])
        pb = torch.from_numpy(pair_base).to(self.device)
        pair_off = torch.empty(n_pairs + 1, dtype=torch.int64, device=self.device)
        total = self._counted("rnnl_miner_ground_count", order_dev.data_ptr(), begin, count, pb.data_ptr(), n_pairs,
                              pair_off.data_ptr())
        if total * 8 > self.budget_bytes and count > 1 and self.chunk_triples is None:
            return None
        dst = torch.empty(max(total, 1), dtype=torch.int32, device=self.device)
        cnt = torch.empty(max(total, 1), dtype=torch.int32, device=self.device)  # u32 path counts
        # the chain kernels index by these entries: read them only if they are whole
        self._counted("rnnl_miner_ground_fill", order_dev.data_ptr(), begin, count, pb.data_ptr(), n_pairs,
                      pair_off.data_ptr(), dst.data_ptr(), cnt.data_ptr(), total)
        return (begin, count, pb, n_pairs, pair_off, dst, cnt)

    def _check_counters(self):
        c = self._counters.cpu().tolist()
        if c[1]:
            raise _native.NativeError(_native.RNNL_ERR_RANGE, "rule miner: a path count does not fit 32 bits")
        if c[2] or c[3]:
            raise _native.NativeError(_native.RNNL_ERR_INTERNAL, "rule miner: grounding failed (flags %r)" % (c[1:],))
        return int(c[0])

    def _chunks(self, order, n_used):
        """Ground positions [0, n_used) of `order` chunk by chunk: whole chunks
        of chunk_triples if that is set, else as many triples as the byte
        budget allows (16 bytes per pair, 8 per entry)."""
        key = (hash(order.tobytes()), n_used)
        if self._grounded is not None and self._grounded[0] == key and np.array_equal(self._grounded[2], order):
            yield self._grounded[1]
            return
        order_dev = torch.from_numpy(order).to(self.device)
        nr_of = (self._rule_off[1:] - self._rule_off[:-1]).astype(np.int64)[self._hrt[order[:n_used], 1]]
        begin, first = 0, True
        step = self.chunk_triples
        while begin < n_used:
            if step is None:
                cum = np.cumsum(nr_of[begin:])
                count = max(1, int(np.searchsorted(cum, self.budget_bytes // 16, side="right")))
            else:
                count = min(step, n_used - begin)
            while True:
                pair_base = np.zeros(count + 1, dtype=np.int64)
                np.cumsum(nr_of[begin:begin + count], out=pair_base[1:])
                chunk = self._ground(order_dev, begin, count, pair_base)
                if chunk is not None:
                    break
                count = max(1, count // 2)
            chunk = chunk + (order_dev,)
            if first and count == n_used:  # the whole run in one chunk: h_score reuses learn's entries
                self._grounded = (key, chunk, order.copy())  # (kept until the rules are set again)
            first = False
            yield chunk
            begin += count

    @torch.no_grad()
    def learn(self, lr, wd, temp, fast=False, portion=1.0, order=None):
        """ReasoningPredictor::learn with one thread: online Adam over the
        first int(n * portion) triples of `order` (a permutation of the train
        triples; drawn from the miner's seeded generator if absent)."""
        order, n_used = self._use_order(order if order is not None else self._rng.permutation(len(self._hrt)),
                                        portion)
        self._agg_stale = True  # the weights move
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            for begin, count, pb, n_pairs, pair_off, dst, cnt, odev in self._chunks(order, n_used):
                _native.call("rnnl_miner_learn", self._handle, odev.data_ptr(), begin, count, pb.data_ptr(), n_pairs,
                             pair_off.data_ptr(), dst.data_ptr(), cnt.data_ptr(), float(lr), float(wd), float(temp),
                             int(bool(fast)), stream)

    @torch.no_grad()
    def h_score(self, top_k, H_temperature=1.0, prior_weight=0.0, portion=1.0, order=None):
        """ReasoningPredictor::H_score with one thread, over the order of the
        last learn() unless one is given (H_score does not shuffle)."""
        order, n_used = self._use_order(order, portion)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            for begin, count, pb, n_pairs, pair_off, dst, cnt, odev in self._chunks(order, n_used):
                _native.call("rnnl_miner_h_score", self._handle, odev.data_ptr(), begin, count, pb.data_ptr(),
                             n_pairs, pair_off.data_ptr(), dst.data_ptr(), cnt.data_ptr(), int(top_k),
                             float(H_temperature), float(prior_weight), stream)

    def _read(self, which):
        n = int(self._rule_off[-1])
        out = torch.empty(n, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _native.call("rnnl_miner_read", self._handle, out.data_ptr() if which == 0 else None,
                         out.data_ptr() if which == 1 else None, torch.cuda.current_stream(self.device).cuda_stream)
        flat = out.cpu().numpy()
        return [flat[a:b] for a, b in zip(self._rule_off[:-1], self._rule_off[1:])]

    def weights(self):
        """Per relation, the learned weight of each rule of its list (float64)."""
        return self._read(0)

    def H(self):
        """Per relation, the H score of each rule of its list (float64)."""
        return self._read(1)

    # ------------------------------------------- support and confidence
    @torch.no_grad()
    def _stats_arrays(self, head, ln, body, max_blocks=0, first_stamp=0):
        """(support, body, pca_body), int64 per rule, of rules given as arrays
        (rnnl_miner_rule_stats): each distinct body is walked once per source
        entity whatever the number of heads and copies it is listed with."""
        if len(head) == 0:
            return tuple(np.zeros(0, dtype=np.int64) for _ in range(3))
        return self._stats_grouped(group_rules(head, ln, body, self.graph.relation_size), max_blocks, first_stamp)

    @torch.no_grad()
    def _stats_grouped(self, grouped, max_blocks=0, first_stamp=0):
        """_stats_arrays of rules that group_rules has grouped already."""
        body_len, body_rel, head_off, head_rel, body_of, slot_of = grouped
        nb, ns = len(body_len), len(head_rel)
        nbytes = ctypes.c_size_t()
        _native.call("rnnl_miner_rule_stats_scratch", self._handle, nb, ns, int(max_blocks), ctypes.byref(nbytes))
        with torch.cuda.device(self.device):
            work = torch.empty(nbytes.value, dtype=torch.uint8, device=self.device)
            out = torch.empty(nb + 2 * ns, dtype=torch.int64, device=self.device)
            counters = torch.zeros(4, dtype=torch.int64, device=self.device)  # not the evaluation's
            _native.call("rnnl_miner_rule_stats", self._handle, nb, body_len.ctypes.data, body_rel.ctypes.data,
                         head_off.ctypes.data, head_rel.ctypes.data, int(max_blocks), int(first_stamp),
                         work.data_ptr(), nbytes.value, out.data_ptr(), counters.data_ptr(),
                         torch.cuda.current_stream(self.device).cuda_stream)
            flat = out.cpu().numpy()
            c = counters.cpu().tolist()
        if c[1] or c[2] or c[3]:
            raise _native.NativeError(_native.RNNL_ERR_INTERNAL, "rule statistics failed (flags %r)" % (c[1:],))
        return flat[nb:nb + ns][slot_of], flat[:nb][body_of], flat[nb + ns:][slot_of]

    def _listed(self, rel2rules):
        """(head, length, body, offsets) of rel2rules, or of the current lists."""
        R = self.graph.relation_size
        if rel2rules is None:
            off = self._rule_off.astype(np.int64)
            return np.repeat(np.arange(R), np.diff(off)), self._rule_len, self._rule_body, off
        if len(rel2rules) != R:
            raise ValueError("rule_stats: one rule list per relation expected")
        head, ln, body = [], [], []
        for r, rules in enumerate(rel2rules):
            for hd, b in rules:
                if int(hd) != r:
                    raise ValueError("rule_stats: rule with head %d in the list of relation %d" % (hd, r))
                if len(b) > MAX_BODY:
                    raise ValueError(_too_long("rule_stats", MAX_BODY))
                if any(int(x) < 0 or int(x) >= R for x in b):
                    raise ValueError("rule_stats: body relation out of range [0, %d)" % R)
                head.append(r)
                ln.append(len(b))
                body.append([int(x) for x in b] + [0] * (MAX_BODY - len(b)))
        off = np.concatenate([[0], np.cumsum([len(x) for x in rel2rules])]).astype(np.int64)
        return (np.asarray(head, dtype=np.int64), np.asarray(ln, dtype=np.int32),
                np.asarray(body, dtype=np.int32).reshape(-1, MAX_BODY), off)

    @staticmethod
    def _per_relation(flat, off):
        return [flat[a:b] for a, b in zip(off[:-1], off[1:])]

    def rule_stats(self, rel2rules=None, max_blocks=0):
        """dict(support, body, pca_body): per relation an int64 array parallel
        to its rule list — rel2rules[r] = [(head, body)], or the current lists
        of set_logic_rules / read_rules.  Exact counts on the whole train
        graph, no edge removed (unlike search, learn and evaluate): support =
        the known (h, t) pairs of the head the body reaches, body = all pairs
        the body reaches, pca_body = those whose h has some known tail.  The
        handle's rules, weights and H are not touched.  max_blocks bounds the
        kernel's grid (0: the default)."""
        head, ln, body, off = self._listed(rel2rules)
        sup, bod, pca = self._stats_arrays(head, ln, body, max_blocks)
        return dict(support=self._per_relation(sup, off), body=self._per_relation(bod, off),
                    pca_body=self._per_relation(pca, off))

    def head_pairs(self):
        """int64 per relation: its distinct (h, t) pairs in train."""
        if self._head_pairs is None:
            R = self.graph.relation_size
            rel = np.unique(self._hrt.reshape(-1, 3), axis=0)[:, 1] if len(self._hrt) else np.zeros(0, np.int64)
            self._head_pairs = np.bincount(rel, minlength=R).astype(np.int64)
        return self._head_pairs

    def confidence(self, kind="pca", pc=0.0, rel2rules=None):
        """Per relation a float64 array parallel to its rule list: 'std' =
        support / (body + pc), 'pca' = support / (pca_body + pc),
        'head_coverage' = support / head_pairs; 0 / 0 is 0.0."""
        confidences(kind, [], [], [], [], pc)  # a bad kind or pc before any device work
        st = self.rule_stats(rel2rules)
        hp = self.head_pairs()
        return [confidences(kind, s, b, p, hp[r], pc)
                for r, (s, b, p) in enumerate(zip(st["support"], st["body"], st["pca_body"]))]

    def _pool_flat(self):
        if self._searched is None:
            raise RuntimeError("RuleMiner.pool_stats: call search() or mine() first")
        if self._pool_stats is None:
            p_head, p_len, p_body = self._pool_arrays  # no Python tuples on the way
            self._pool_stats = self._stats_arrays(p_head, p_len, p_body)
        return self._pool_stats

    def pool_stats(self):
        """rule_stats of the searched pool, per relation in get_logic_rules()
        order; computed once per search."""
        sup, bod, pca = self._pool_flat()
        off = np.searchsorted(self._pool_arrays[0], np.arange(self.graph.relation_size + 1))
        return dict(support=self._per_relation(sup, off), body=self._per_relation(bod, off),
                    pca_body=self._per_relation(pca, off))

    def _pool_confidence(self, kind, pc):
        sup, bod, pca = self._pool_flat()
        return confidences(kind, sup, bod, pca, self.head_pairs()[self._pool_arrays[0]], pc)

    # ------------------------------------------------------------ evaluation
    def set_weights(self, rel2weights):
        """rel2weights[r][k] (float64) becomes the weight of rule k of relation
        r's current list; the rules' Adam state is cleared, H stays."""
        flat = flatten_weights(self._rule_off, rel2weights)
        self._agg_stale = True
        with torch.cuda.device(self.device):
            dev = torch.from_numpy(flat).to(self.device)
            _native.call("rnnl_miner_set_weights", self._handle, dev.data_ptr(),
                         torch.cuda.current_stream(self.device).cuda_stream)
            torch.cuda.current_stream(self.device).synchronize()  # dev is released on return

    # ----------------------------------------------------------- aggregation
    def set_aggregation(self, agg="sum", depth=1):
        """How scores / eval_ranks / evaluate / predict_topk / explain / predict
        combine the rules that reach an entity.  'sum' (the
        default, the reference's): weight * path count, summed.  'noisy_or':
        weights are confidences in [0, 1]; the score is the sum of -log1p(-w)
        over the firing rules, which ranks as 1 - prod(1 - w) does.  'max':
        weights finite and >= 0; the score is a key of the `depth` (1..3)
        strongest firing rules — depth 1 the plain max, 2 and 3 break its ties
        by the next strongest (decode_max reads the key).  Sticky: it survives
        set_logic_rules, set_weights, read_rules, learn and mine; the operand
        is derived from weights() again before the next query, and a weight the
        mode does not admit raises ValueError there, before any kernel runs.
        learn, h_score and the statistics never look at it."""
        self._agg, self._agg_depth = _check_agg(agg, depth)
        self._agg_stale = True

    @property
    def aggregation(self):
        """(agg, depth) as set_aggregation took them; depth is 1 unless agg is 'max'."""
        return self._agg, (self._agg_depth if self._agg == "max" else 1)

    def _sync_aggregation(self):
        """Before a query launch: the handle's mode and operand follow the
        current rules, weights and set_aggregation."""
        if not self._agg_stale or not self._rules_set:
            return  # (without rules the query itself is refused)
        code, operand, values = _native.MINER_AGG_SUM, None, None
        if self._agg == "noisy_or":
            code, operand = _native.MINER_AGG_NOISY_OR, noisy_or_operand(self.weights())
        elif self._agg == "max":
            classes, values = max_classes(self.weights())
            code, operand = _native.MINER_AGG_MAX, [c.astype(np.float64) for c in classes]
        with torch.cuda.device(self.device):
            dev = None
            if operand is not None:
                flat = np.concatenate(operand + [np.zeros(0, dtype=np.float64)])
                dev = torch.from_numpy(np.ascontiguousarray(flat, dtype=np.float64)).to(self.device)
            _native.call("rnnl_miner_set_aggregation", self._handle, code, self._agg_depth,
                         dev.data_ptr() if dev is not None else None,
                         torch.cuda.current_stream(self.device).cuda_stream)  # (synchronises: dev may go)
        self._agg_values = values
        self._agg_stale = False

    def score_value(self, score, r):
        """A score of relation r's queries as the value to show: the score
        itself ('sum'), the probability 1 - prod(1 - w) ('noisy_or'), the
        weight of the strongest firing rule ('max'; 0.0 if none).  Scores that
        are not finite (-inf past `valid`) stay as they are."""
        s = np.asarray(score, dtype=np.float64)
        if self._agg == "sum":
            return s
        fin = np.isfinite(s)
        if self._agg == "noisy_or":
            return np.where(fin, noisy_or_probability(np.where(fin, s, 0.0)), s)
        self._sync_aggregation()
        if self._agg_values is None:
            raise RuntimeError("RuleMiner.score_value: set the rules and weights first")
        return np.where(fin, decode_max(np.where(fin, s, 0.0), self._agg_values[int(r)])[..., 0], s)

    def read_rules(self, file_name):
        """Sets the rules of a 'head body... x' file (out_rules /
        mined_rules.txt), in file order per head, with x as the weight.
        Returns the number of rules read."""
        rel2rules, rel2weights = read_rule_file(file_name, self.graph.relation_size, self.max_body)
        self.set_logic_rules(rel2rules)
        self.set_weights(rel2weights)
        return sum(len(x) for x in rel2rules)

    def _queries(self, triples):
        q = np.ascontiguousarray(np.asarray(triples, dtype=np.int64).reshape(-1, 3))
        E, R = self.graph.entity_size, self.graph.relation_size
        if len(q) and (q.min() < 0 or q[:, 0].max() >= E or q[:, 2].max() >= E or q[:, 1].max() >= R):
            raise ValueError("query triple out of range")
        return q.astype(np.int32)

    def _known_lists(self, mode):
        from .data import _DeviceLists
        from .kge import true_answers
        every = [np.asarray(getattr(self.graph, name, None) or [], dtype=np.int64).reshape(-1, 3)
                 for name in ("train_facts", "valid_facts", "test_facts")]
        return _DeviceLists(true_answers(np.concatenate(every), self.graph.entity_size, mode), self.device)

    def _known_tails(self):
        if self._known is None:
            self._known = self._known_lists("tail")
        return self._known

    def _known_heads(self):
        """Keys r |E| + t -> the known heads over train, valid and test, built once."""
        if self._known_h is None:
            self._known_h = self._known_lists("head")
        return self._known_h

    def _known_side(self, side):
        return self._known_heads() if side == "head" else self._known_tails()

    @torch.no_grad()
    def _evaluate(self, triples, filtered, want_val, side="tail"):
        _check_side(side, "RuleMiner")
        q = self._queries(triples)
        n, E = len(q), self.graph.entity_size
        self._sync_aggregation()
        with torch.cuda.device(self.device):
            qd = torch.from_numpy(q).to(self.device)
            ranks = torch.zeros((n, 2), dtype=torch.int32, device=self.device)
            val = torch.zeros((n, E), dtype=torch.float64, device=self.device) if want_val else None
            known = self._known_side(side) if filtered else None
            self._counted("rnnl_miner_evaluate_side", _side_code(side), qd.data_ptr(), n, *_known_args(known),
                          ranks.data_ptr(), val.data_ptr() if want_val else None)
        return ranks, val

    def scores(self, triples, side="tail"):
        """(n, |E|) float64 on the device: per query (h, r, t) the val of every
        entity — sum over r's rules of weight * path count from h, the triple's
        own edge removed — bitwise what the reference computes.  side 'head':
        weight * path count from the entity to t, the same edge removed.
        After set_aggregation('noisy_or'): the sum of -log1p(-weight) over the
        rules with a path (noisy_or_probability gives the probability); after
        set_aggregation('max', depth): the key of the depth strongest such
        rules (decode_max gives their weights); +0.0 where no rule arrives."""
        return self._evaluate(triples, False, True, side)[1]

    def eval_ranks(self, triples, filtered=True, side="tail"):
        """(n, 2) numpy int64: per query (num_g, num_ge), the entities scoring
        above the true tail / at least as high (the tail included).  filtered:
        the other known tails of (h, r) over train, valid and test are left
        out (a graph without valid_facts / test_facts filters by train).  side
        'head': the same of the true head among the heads of (?, r, t), the
        other known heads of (r, t) left out."""
        return self._evaluate(triples, filtered, False, side)[0].cpu().numpy().astype(np.int64)

    def evaluate(self, split="test", triples=None, filtered=True, side="tail"):
        """ReasoningPredictor::evaluate over graph.valid_facts / test_facts
        (split 'valid' / 'test') or the given triples, with the current rules
        and weights: dict(mr, mrr, hit1, hit3, hit10, n).  side 'head': the
        head side of every triple; 'both': the tail pairs of all triples, then
        the head pairs, as one list — n is twice the triple count."""
        _check_side(side, "evaluate", both=True)
        if triples is None:
            if split not in ("valid", "test"):
                raise ValueError("evaluate: split must be 'valid' or 'test'")
            triples = getattr(self.graph, split + "_facts")
        pairs = [self.eval_ranks(triples, filtered, s) for s in (("tail", "head") if side == "both" else (side,))]
        return expectation_metrics(np.concatenate(pairs), self.graph.entity_size)

    # ----------------------------------------------------------- predictions
    def _pred_queries(self, queries, side="tail"):
        """(n, 2) (h, r) or (n, 3) (h, r, t) with t >= 0 or -1 -> (n, 3) int32, open queries with t = -1.
        side 'head': (n, 3) (h, r, t) with h >= 0 or -1, the open ones."""
        q = np.asarray(queries, dtype=np.int64)
        if q.size == 0:
            q = q.reshape(0, 3)
        if _check_side(side, "RuleMiner") == "head":
            if q.ndim != 2 or q.shape[1] != 3:
                raise ValueError("head-side queries must be (n, 3) (h, r, t), h = -1: an open query (got shape %r)"
                                 % (q.shape,))
            ans, name = 0, "h"  # the answer's column, the one that may be -1; the other end is the anchor
        else:
            if q.ndim != 2 or q.shape[1] not in (2, 3):
                raise ValueError("queries must be (n, 2) (h, r) or (n, 3) (h, r, t) (got shape %r)" % (q.shape,))
            if q.shape[1] == 2:
                q = np.concatenate([q, np.full((len(q), 1), -1, dtype=np.int64)], 1)
            ans, name = 2, "t"
        anchor = 2 - ans
        E, R = self.graph.entity_size, self.graph.relation_size
        if len(q) and (q[:, 1].min() < 0 or q[:, anchor].min() < 0 or q[:, ans].min() < -1
                       or q[:, anchor].max() >= E or q[:, ans].max() >= E or q[:, 1].max() >= R):
            raise ValueError("query out of range (h, t in [0, %d), r in [0, %d); %s = -1: an open query)"
                             % (E, R, name))
        return np.ascontiguousarray(q, dtype=np.int32)

    @torch.no_grad()
    def predict_topk(self, queries, k=10, filtered=True, candidates="reached", side="tail"):
        """The first k tails of each query by the score of `scores` (val
        descending, then entity id; rnnl_miner_predict, csrc/mine_predict.hip),
        without the (n, |E|) matrix.  queries: (n, 2) (h, r) — open: no edge is
        removed, no answer kept — or (n, 3) (h, r, t), t = -1 open as well.
        candidates 'reached': the entities some rule reaches (whatever its
        weight); 'all': every entity.  filtered: the other known tails of
        (h, r) over train, valid and test leave, t stays.  Returns device
        tensors: index (n, k) int32 (-1 past valid), score (n, k) float64
        (bitwise `scores`; -inf past valid), valid (n,) int32 = min(k,
        #eligible), position (n,) int32 = the 0-based place of t in the whole
        eligible order (also past k), -1 if t is not eligible or the query is
        open.  side 'head': the first k heads of (?, r, t) by the head-side
        score; queries (n, 3) (h, r, t), h = -1 open; the other known heads of
        (r, t) leave, h stays; position is the place of h.  The order and the
        scores are those of the aggregation set (set_aggregation): the noisy-or
        sum or the max key in place of the weighted path count; score_value
        turns a score into the value to show."""
        k = int(k)
        if not 1 <= k <= _native.MINER_TOPK_MAX:
            raise ValueError("predict_topk: k must be 1..%d (got %d)" % (_native.MINER_TOPK_MAX, k))
        if candidates not in ("reached", "all"):
            raise ValueError("predict_topk: candidates must be 'reached' or 'all' (got %r)" % (candidates,))
        q = self._pred_queries(queries, side)
        n = len(q)
        self._sync_aggregation()
        with torch.cuda.device(self.device):
            qd = torch.from_numpy(q).to(self.device)
            index = torch.empty((n, k), dtype=torch.int32, device=self.device)
            score = torch.empty((n, k), dtype=torch.float64, device=self.device)
            valid = torch.empty(n, dtype=torch.int32, device=self.device)
            position = torch.empty(n, dtype=torch.int32, device=self.device)
            known = self._known_side(side) if filtered else None
            self._counted("rnnl_miner_predict_side", _side_code(side), qd.data_ptr(), n, *_known_args(known), k,
                          _native.MINER_ALL if candidates == "all" else _native.MINER_REACHED, index.data_ptr(),
                          score.data_ptr(), valid.data_ptr(), position.data_ptr())
        return index, score, valid, position

    @torch.no_grad()
    def explain(self, queries, index, rules_per_tail=3, side="tail"):
        """The rules behind the entities index (n, m) int32 (-1: an unused
        slot; m <= 256) of each query (rnnl_miner_explain).  Returns device
        tensors: fired (n, m) int32 = the rules with a path to the entity,
        total (n, m) float64 = their weight * count summed in list order
        (bitwise the entity's score), rule (n, m, c) int32 = the c =
        rules_per_tail (1..16) rules with the largest weight * count, ties by
        list index, as indices into the relation's rule list (-1 unused), and
        count (n, m, c) int64 = their path counts.  side 'head': the entities
        are heads of (?, r, t), the paths run from the entity to t.  After
        set_aggregation('noisy_or' / 'max'): fired as before; total = the
        entity's score bitwise (the sum of -log1p(-weight) in list order / the
        key of all firing rules at the depth set); rule = the firing rules by
        weight descending, ties by list index; count = 1 for each of them (the
        paths are not counted, so no count can pass 32 bits)."""
        c = int(rules_per_tail)
        if not 1 <= c <= _native.MINER_EXPLAIN_MAX:
            raise ValueError("explain: rules_per_tail must be 1..%d (got %d)" % (_native.MINER_EXPLAIN_MAX, c))
        q = self._pred_queries(queries, side)
        n = len(q)
        self._sync_aggregation()
        with torch.cuda.device(self.device):
            idx = torch.as_tensor(index, device=self.device).to(torch.int32).contiguous()
            if idx.dim() != 2 or idx.shape[0] != n or not 1 <= idx.shape[1] <= _native.MINER_TOPK_MAX:
                raise ValueError("explain: index must be (n, m) with 1 <= m <= %d (got %r for %d queries)"
                                 % (_native.MINER_TOPK_MAX, tuple(idx.shape), n))
            m = idx.shape[1]
            qd = torch.from_numpy(q).to(self.device)
            fired = torch.empty((n, m), dtype=torch.int32, device=self.device)
            total = torch.empty((n, m), dtype=torch.float64, device=self.device)
            rule = torch.empty((n, m, c), dtype=torch.int32, device=self.device)
            count = torch.empty((n, m, c), dtype=torch.int64, device=self.device)
            self._counted("rnnl_miner_explain_side", _side_code(side), qd.data_ptr(), n, idx.data_ptr(), m, c,
                          fired.data_ptr(), total.data_ptr(), rule.data_ptr(), count.data_ptr())
        return fired, total, rule, count

    @torch.no_grad()
    def explain_paths(self, queries, index, rule, max_paths=3, side="tail"):
        """The grounding paths behind rules of listed entities
        (rnnl_miner_paths_side).  queries and index (n, m) as for
        `explain`; rule (n, m, c) int32, c <= 16: per slot indices into the
        relation's rule list, -1 unused — what `explain` returned, or any other
        rules of the list.  A path of rule r <- b1..bL is x_0 -b1-> x_1 ...
        -bL-> x_L over train edges, from the query's h to the entity (side
        'tail') or from the entity to the query's t (side 'head'), every copy
        of the query's own edge skipped; a triple that is in train twice gives
        two edges and so two equal paths.  Returns device tensors: listed
        (n, m, c) int32 = min(max_paths, count), count (n, m, c) int64 = the
        exact number of paths (`explain`'s count under 'sum'; 0 where the rule
        does not fire), path (n, m, c, max_paths, 6) int32 = the first `listed`
        paths as x_0 .. x_L, -1 past x_L and in unlisted rows.  Order: by the
        entities read from the listed entity back toward the anchor — tail
        side x_{L-1} ascending, then x_{L-2}, ...; head side x_1, then x_2, ....
        Paths are counted whatever set_aggregation says.  max_paths 1..64."""
        P = int(max_paths)
        if not 1 <= P <= _native.MINER_PATHS_MAX:
            raise ValueError("explain_paths: max_paths must be 1..%d (got %d)" % (_native.MINER_PATHS_MAX, P))
        q = self._pred_queries(queries, side)
        n = len(q)
        ishape = tuple(index.shape) if hasattr(index, "shape") else np.shape(index)
        if len(ishape) != 2 or ishape[0] != n or not 1 <= ishape[1] <= _native.MINER_TOPK_MAX:
            raise ValueError("explain_paths: index must be (n, m) with 1 <= m <= %d (got %r for %d queries)"
                             % (_native.MINER_TOPK_MAX, ishape, n))
        m = ishape[1]
        rshape = tuple(rule.shape) if hasattr(rule, "shape") else np.shape(rule)
        if len(rshape) != 3 or rshape[:2] != (n, m) or not 1 <= rshape[2] <= _native.MINER_EXPLAIN_MAX:
            raise ValueError("explain_paths: rule must be (n, m, c) with 1 <= c <= %d (got %r for index %r)"
                             % (_native.MINER_EXPLAIN_MAX, rshape, ishape))
        c = rshape[2]
        if n * m * c * P * _native.MINER_PATH_LEN >= 2 ** 31:
            raise ValueError("explain_paths: path would have 2^31 elements or more (cut the queries into smaller calls)")
        with torch.cuda.device(self.device):
            idx = torch.as_tensor(index, device=self.device).to(torch.int32).contiguous()
            rl = torch.as_tensor(rule, device=self.device).to(torch.int32).contiguous()
            qd = torch.from_numpy(q).to(self.device)
            listed = torch.empty((n, m, c), dtype=torch.int32, device=self.device)
            count = torch.empty((n, m, c), dtype=torch.int64, device=self.device)
            path = torch.empty((n, m, c, P, _native.MINER_PATH_LEN), dtype=torch.int32, device=self.device)
            self._counted("rnnl_miner_paths_side", _side_code(side), qd.data_ptr(), n, idx.data_ptr(), m,
                          rl.data_ptr(), c, P, listed.data_ptr(), count.data_ptr(), path.data_ptr())
        return listed, count, path

    def path_text(self, path_row):
        """A row of explain_paths' `path` in the entity names of the graph: `a > x > b`."""
        return path_text(path_row, self.graph)

    def predict(self, split="test", triples=None, k=10, filtered=True, explain=0, rules_per_tail=3,
                candidates="reached", output=None, side="tail", paths=0):
        """The miner's answers on graph.valid_facts / test_facts (split
        'valid' / 'test') or the given queries ((n, 2) or (n, 3), as
        predict_topk), with the current rules and weights.  Returns a dict of
        numpy arrays: h, r, t (n,), index / score (n, k), valid, position (n,)
        and, with explain = m > 0, explain_fired / explain_total (n, m') and
        explain_rule / explain_count (n, m', rules_per_tail) of the first m' =
        min(m, k) places (`explain`).  output: one TSV line per prediction —
        head, relation, place (1-based), tail, repr(score_value(score)), `*` on the known
        answer, then for the explained places `head <- b1, b2:count:weight`
        per listed rule, names from the graph's dictionaries.  side 'head':
        the heads of (?, r, t); the lines keep the triple's orientation —
        predicted head, relation, place written h1, h2, ..., the query's tail,
        score, `*`, rules.  paths = P > 0 (with explain > 0): explain_paths of
        the explained places and their listed rules as explain_paths_listed /
        explain_paths_count (n, m', rules_per_tail) and explain_path (n, m',
        rules_per_tail, P, 6); in the file each rule column becomes
        `head <- b1, b2:count:weight [a > x > b | a > y > b]`, ` | ...` appended
        inside the brackets where there are more paths than are listed."""
        _check_side(side, "predict")
        P = int(paths)
        if P and not 1 <= P <= _native.MINER_PATHS_MAX:
            raise ValueError("predict: paths must be 0..%d (got %d)" % (_native.MINER_PATHS_MAX, P))
        if P and min(int(explain), int(k)) <= 0:
            raise ValueError("predict: paths lists the paths of explained rules: give explain > 0 with it")
        if triples is None:
            if split not in ("valid", "test"):
                raise ValueError("predict: split must be 'valid' or 'test'")
            triples = getattr(self.graph, split + "_facts")
        q = self._pred_queries(triples, side)
        index, score, valid, position = self.predict_topk(q, k, filtered, candidates, side)
        out = dict(h=q[:, 0].astype(np.int64), r=q[:, 1].astype(np.int64), t=q[:, 2].astype(np.int64),
                   index=index.cpu().numpy(), score=score.cpu().numpy(), valid=valid.cpu().numpy(),
                   position=position.cpu().numpy())
        m = min(int(explain), int(k))
        if m > 0:
            names = ("explain_fired", "explain_total", "explain_rule", "explain_count")
            pnames = ("explain_paths_listed", "explain_paths_count", "explain_path")
            if len(q):
                got = self.explain(q, index[:, :m].contiguous(), rules_per_tail, side)
                out.update((name, v.cpu().numpy()) for name, v in zip(names, got))
                if P:
                    out.update((name, v.cpu().numpy()) for name, v in
                               zip(pnames, self.explain_paths(q, index[:, :m].contiguous(), got[2], P, side)))
            else:
                c = int(rules_per_tail)
                out.update(zip(names, (np.zeros((0, m), np.int32), np.zeros((0, m), np.float64),
                                       np.zeros((0, m, c), np.int32), np.zeros((0, m, c), np.int64))))
                if P:
                    out.update(zip(pnames, (np.zeros((0, m, c), np.int32), np.zeros((0, m, c), np.int64),
                                            np.zeros((0, m, c, P, _native.MINER_PATH_LEN), np.int32))))
        if output is not None:
            self._write_predictions(output, out, m, side)
        return out

    def rule_text(self, r, k, count=None, weight=None):
        """Rule k of relation r's list in relation names: `head <- b1, b2` (`:count:weight` appended if given)."""
        i = int(self._rule_off[r]) + int(k)
        body = self._rule_body[i][:int(self._rule_len[i])].tolist()
        text = "%s <- %s" % (_name(self.graph, "id2relation", r),
                             ", ".join(_name(self.graph, "id2relation", b) for b in body))
        return text if count is None else "%s:%d:%r" % (text, count, float(weight))

    def paths_text(self, rows, listed, count):
        """The bracket behind a rule column: the `listed` first rows of one (P, 6)
        block of explain_paths' `path`, ` | ...` where `count` says there are more."""
        parts = [self.path_text(row) for row in rows[:int(listed)]]
        return "[%s]" % " | ".join(parts + (["..."] if int(count) > int(listed) else []))

    def _write_predictions(self, path, out, m, side="tail"):
        wt = self.weights() if m > 0 else None
        head = side == "head"
        with_paths = m > 0 and "explain_path" in out
        with open(path, "w") as fo:
            for i in range(len(out["h"])):
                h, r, t = int(out["h"][i]), int(out["r"][i]), int(out["t"][i])
                for j in range(int(out["valid"][i])):
                    e = int(out["index"][i, j])
                    cols = [_name(self.graph, "id2entity", e if head else h), _name(self.graph, "id2relation", r),
                            "h%d" % (j + 1) if head else str(j + 1), _name(self.graph, "id2entity", t if head else e),
                            repr(float(self.score_value(out["score"][i, j], r))), "*" if e == (h if head else t) else ""]
                    if j < m and not with_paths:
                        cols += [self.rule_text(r, kk, c, wt[r][kk]) for kk, c in
                                 zip(out["explain_rule"][i, j].tolist(), out["explain_count"][i, j].tolist())
                                 if kk >= 0]
                    elif j < m:
                        cols += ["%s %s" % (self.rule_text(r, kk, c, wt[r][kk]),
                                            self.paths_text(out["explain_path"][i, j, s],
                                                            out["explain_paths_listed"][i, j, s],
                                                            out["explain_paths_count"][i, j, s]))
                                 for s, (kk, c) in enumerate(zip(out["explain_rule"][i, j].tolist(),
                                                                 out["explain_count"][i, j].tolist())) if kk >= 0]
                    fo.write("\t".join(cols) + "\n")
        return int(np.sum(out["valid"]))

    def mine(self, max_length, iterations, top_n, top_k, lr, wd, temp, top_n_out=0, seed=0, orders=None,
             selections=None, portion=1.0, prior=None, prior_weight=0.0, pc=0.0):
        """The reference miner's main loop (miner/main.cpp:27-49): search, then
        per iteration a rule subset per relation (top_n, 0 = all), learn,
        H_score and the pool's running mean of H.  orders[it] (a permutation
        of the train triples) and selections[it][r] (pool indices) replace the
        seeded draws, so a reference run can be replayed.  prior ('std' or
        'pca', with pc) makes that confidence of each selected rule its prior,
        which enters H_score as prior * prior_weight (the reference's slot;
        None: priors of 0, as the reference's miner).  Returns the rules
        out_rules would write: [(head, body, H)]."""
        if max_length > self.max_body:
            raise ValueError(_too_long("mine(max_length=%d)" % max_length, self.max_body))
        if prior not in (None, "std", "pca"):
            raise ValueError("mine: prior must be None, 'std' or 'pca' (got %r)" % (prior,))
        if not self.rules or self._searched != max_length:
            self.search(max_length)
        pool = self.get_logic_rules()
        R = self.graph.relation_size
        self.pool = pool
        self.pool_H = [np.zeros(len(p), dtype=np.float64) for p in pool]
        cn = [np.zeros(len(p), dtype=np.float64) for p in pool]
        p_head, p_len, p_body = self._pool_arrays  # the pool in search order: per head, then by key
        pool_off = np.searchsorted(p_head, np.arange(R + 1))
        pool_prior = self._pool_confidence(prior, pc) if prior is not None else None
        rng = np.random.default_rng(seed)
        for it in range(iterations):
            if selections is not None:
                sel = [np.asarray(selections[it][r], dtype=np.int64) for r in range(R)]
            else:
                sel = [rng.permutation(len(pool[r]))[:top_n if top_n else None] for r in range(R)]
            order = np.ascontiguousarray(orders[it] if orders is not None else rng.permutation(len(self._hrt)),
                                         dtype=np.int32)
            take = np.concatenate([pool_off[r] + sel[r] for r in range(R)]) if R else np.zeros(0, np.int64)
            off = np.concatenate([[0], np.cumsum([len(x) for x in sel])])
            self._set_rule_arrays(off, p_len[take], p_body[take],  # = set_logic_rules(subset, priors)
                                  pool_prior[take] if pool_prior is not None else np.zeros(len(take)))
            self.learn(lr, wd, temp, False, portion, order)
            self.h_score(top_k, 1.0, float(prior_weight), portion, self._order)
            for r, H in enumerate(self.H()):  # RuleGenerator::update
                self.pool_H[r][sel[r]] = (self.pool_H[r][sel[r]] * cn[r][sel[r]] + H) / (cn[r][sel[r]] + 1)
                cn[r][sel[r]] += 1
        self._grounded = None
        return self.best_rules(top_n_out)

    def _best(self, top_n_out, min_support, min_confidence, confidence, pc, want_stats):
        """Per relation the pool indices best_rules keeps, in its order, and the
        pool's statistics (None unless a bound or want_stats asks for them)."""
        if self.pool is None:
            raise RuntimeError("RuleMiner.best_rules / out_rules: call mine() first")
        filtering = min_support > 0 or min_confidence > 0.0
        st = conf = None
        if filtering or want_stats:
            st = self.pool_stats()
            hp = self.head_pairs()
            conf = {kind: [confidences(kind, st["support"][r], st["body"][r], st["pca_body"][r], hp[r], pc)
                           for r in range(len(self.pool))]
                    for kind in set(["std", "pca", confidence])}
            if any(len(a) != len(b) for a, b in zip(st["support"], self.pool)):
                raise RuntimeError("RuleMiner.best_rules: the pool was searched again since mine()")
        picks = []
        for r in range(len(self.pool)):
            idx = np.argsort(-self.pool_H[r], kind="stable")
            if filtering:  # rules below either bound leave before top_n_out counts
                idx = idx[keep_rules(st["support"][r], conf[confidence][r], min_support, min_confidence)[idx]]
            picks.append(idx[:top_n_out if top_n_out else None])
        return picks, st, conf

    def best_rules(self, top_n_out=0, min_support=0, min_confidence=0.0, confidence="pca", pc=0.0):
        """Per relation the pool's rules by H descending, then pool order; the
        first top_n_out (0 = all) of those with support >= min_support and
        confidence ('std', 'pca' or 'head_coverage', with pc) >=
        min_confidence: [(head, body, H)]."""
        picks, _, _ = self._best(top_n_out, min_support, min_confidence, confidence, pc, False)
        out = []
        for r, rules in enumerate(self.pool):
            for k in picks[r]:
                out.append((rules[k][0], rules[k][1], float(self.pool_H[r][k])))
        return out

    def out_rules(self, file_name, top_n_out=0, min_support=0, min_confidence=0.0, confidence="pca", pc=0.0):
        """RuleGenerator::out_rules (rnnlogic.cpp:1904-1935): 'head body... H'
        with H as %.16f — the mined_rules.txt of the reference pipeline.  The
        bounds are best_rules'."""
        rules = self.best_rules(top_n_out, min_support, min_confidence, confidence, pc)
        with open(file_name, "w") as fo:
            for hd, body, H in rules:
                fo.write("%d%s %.16f\n" % (hd, "".join(" %d" % x for x in body), H))
        return len(rules)

    def out_rule_stats(self, file_name, top_n_out=0, min_support=0, min_confidence=0.0, confidence="pca", pc=0.0):
        """The rules out_rules writes with the same arguments, one line each:
        'head body... H support body pca_body std pca' (H and the two
        confidences as %.16f)."""
        picks, st, conf = self._best(top_n_out, min_support, min_confidence, confidence, pc, True)
        n = 0
        with open(file_name, "w") as fo:
            for r, rules in enumerate(self.pool):
                for k in picks[r]:
                    fo.write(stats_line(rules[k][0], rules[k][1], float(self.pool_H[r][k]), st["support"][r][k],
                                        st["body"][r][k], st["pca_body"][r][k], conf["std"][r][k],
                                        conf["pca"][r][k]))
                    n += 1
        return n

    def write_list_stats(self, file_name, pc=0.0):
        """The current rule lists (set_logic_rules / read_rules) with their
        weight and statistics, in list order: 'head body... weight support
        body pca_body std pca'."""
        st, hp = self.rule_stats(), self.head_pairs()
        body, ln, n = self._rule_body.tolist(), self._rule_len.tolist(), 0
        with open(file_name, "w") as fo:
            for r, wt in enumerate(self.weights()):
                s, b, p = st["support"][r], st["body"][r], st["pca_body"][r]
                std, pca = confidences("std", s, b, p, hp[r], pc), confidences("pca", s, b, p, hp[r], pc)
                for k in range(len(wt)):
                    i = int(self._rule_off[r]) + k
                    fo.write(stats_line(r, body[i][:ln[i]], float(wt[k]), s[k], b[k], p[k], std[k], pca[k]))
                    n += 1
        return n

    def save(self, file_name):
        """RuleMiner::save (rnnlogic.cpp:591-610): 'type head body... H wt prior'
        (H, wt, prior are 0 after a search)."""
        with open(file_name, "w") as fo:
            for hd, body in self.rules:
                fo.write("%d %d%s %f %f %f\n" % (len(body), hd, "".join(" %d" % x for x in body), 0.0, 0.0, 0.0))
        return len(self.rules)


def main(argv=None):
    """python -m rnnlogic_amd.miner: the reference miner's command line
    (miner/main.cpp) — same flags, same defaults; -threads is accepted and
    ignored (the GPU run is the single-threaded semantics)."""
    import argparse

    from .data import KnowledgeGraph
    ap = argparse.ArgumentParser(prog="python -m rnnlogic_amd.miner", allow_abbrev=False)
    ap.add_argument("-data-path", dest="data_path", required=True)
    ap.add_argument("-output-file", dest="output_file", default=None)
    ap.add_argument("-max-length", dest="max_length", type=int, default=2)
    ap.add_argument("-threads", dest="threads", type=int, default=1)
    ap.add_argument("-iterations", dest="iterations", type=int, default=10)
    ap.add_argument("-lr", dest="lr", type=float, default=0.01)
    ap.add_argument("-wd", dest="wd", type=float, default=0.0)
    ap.add_argument("-temp", dest="temp", type=float, default=100.0)
    ap.add_argument("-top-k", dest="top_k", type=int, default=10)
    ap.add_argument("-top-n", dest="top_n", type=int, default=100)
    ap.add_argument("-top-n-out", dest="top_n_out", type=int, default=100)
    ap.add_argument("-seed", dest="seed", type=int, default=0)
    ap.add_argument("-evaluate", dest="evaluate", choices=["valid", "test", "both"], default=None)
    ap.add_argument("-rule-file", dest="rule_file", default=None)
    ap.add_argument("-stats-file", dest="stats_file", default=None)
    ap.add_argument("-min-support", dest="min_support", type=int, default=0)
    ap.add_argument("-min-conf", dest="min_conf", type=float, default=0.0)
    ap.add_argument("-conf", dest="conf", choices=["std", "pca"], default="pca")
    ap.add_argument("-pc", dest="pc", type=float, default=0.0)
    ap.add_argument("-prior", dest="prior", choices=["std", "pca"], default=None)
    ap.add_argument("-prior-weight", dest="prior_weight", type=float, default=0.0)
    ap.add_argument("-predict", dest="predict", choices=["valid", "test"], default=None)
    ap.add_argument("-queries-file", dest="queries_file", default=None)
    ap.add_argument("-predictions-file", dest="predictions_file", default=None)
    ap.add_argument("-k", dest="k", type=int, default=10)
    ap.add_argument("-explain", dest="explain", type=int, default=0)
    ap.add_argument("-rules-per-tail", dest="rules_per_tail", type=int, default=3)
    ap.add_argument("-paths", dest="paths", type=int, default=0)
    ap.add_argument("-candidates", dest="candidates", choices=["reached", "all"], default="reached")
    ap.add_argument("-side", dest="side", choices=["tail", "head", "both"], default="tail")
    ap.add_argument("-agg", dest="agg", choices=["sum", "noisy-or", "max"], default="sum")
    ap.add_argument("-agg-depth", dest="agg_depth", type=int, default=1)
    ap.add_argument("-weights", dest="weights", choices=["file", "conf"], default="file")
    a = ap.parse_args(argv)
    predicting = a.predict is not None or a.queries_file is not None
    if a.output_file is None and a.rule_file is None:
        ap.error("the following arguments are required: -output-file")
    if a.rule_file is not None and (a.output_file is not None
                                    or (a.evaluate is None and a.stats_file is None and not predicting)):
        ap.error("-rule-file evaluates a rule file: give -evaluate, -predict or -queries-file, and no -output-file")
    if a.predict is not None and a.queries_file is not None:
        ap.error("-predict takes a split, -queries-file a file of queries: give one of them")
    if predicting != (a.predictions_file is not None):
        ap.error("-predict / -queries-file write their answers to -predictions-file: give both or neither")
    if predicting and a.side == "both":
        ap.error("-side both belongs to -evaluate: -predict / -queries-file answer one side, tail or head")
    if predicting and not 1 <= a.k <= _native.MINER_TOPK_MAX:
        ap.error("-k must be 1..%d" % _native.MINER_TOPK_MAX)
    if predicting and (a.explain < 0 or not 1 <= a.rules_per_tail <= _native.MINER_EXPLAIN_MAX):
        ap.error("-explain must be >= 0 and -rules-per-tail 1..%d" % _native.MINER_EXPLAIN_MAX)
    if a.paths and not predicting:
        ap.error("-paths acts on -predict and -queries-file: give one of them")
    if predicting and not 0 <= a.paths <= _native.MINER_PATHS_MAX:
        ap.error("-paths must be 0..%d" % _native.MINER_PATHS_MAX)
    if predicting and a.paths and a.explain < 1:
        ap.error("-paths lists the paths of explained rules: give -explain with it")
    if a.rule_file is None and not 1 <= a.max_length <= MAX_BODY:
        ap.error("-max-length must be 1..%d" % MAX_BODY)
    if a.pc < 0.0 or a.min_support < 0:
        ap.error("-pc and -min-support must be >= 0")
    if a.rule_file is not None and (a.min_support or a.min_conf or a.prior is not None or a.prior_weight):
        ap.error("-min-support, -min-conf, -prior and -prior-weight belong to mining, not to -rule-file")
    if not 1 <= a.agg_depth <= 3:
        ap.error("-agg-depth must be 1..3")
    if a.agg_depth != 1 and a.agg != "max":
        ap.error("-agg-depth belongs to -agg max")
    if (a.agg != "sum" or a.weights != "file") and a.evaluate is None and not predicting:
        ap.error("-agg and -weights act on -evaluate, -predict and -queries-file: give one of them")
    # mining: bodies as long as asked for; a rule file: as long as the miner holds
    miner = RuleMiner(KnowledgeGraph(a.data_path),
                      max_body=MAX_BODY if a.rule_file is not None else max(3, a.max_length))
    # (a name the dictionaries do not know stops the run before it mines)
    queries = read_queries_file(a.queries_file, miner.graph, a.side) if a.queries_file is not None else None
    if a.output_file is not None:
        miner.mine(a.max_length, a.iterations, a.top_n, a.top_k, a.lr, a.wd, a.temp, a.top_n_out, seed=a.seed,
                   prior=a.prior, prior_weight=a.prior_weight, pc=a.pc)
        bounds = (a.min_support, a.min_conf, a.conf, a.pc)
        print("#Rules written: %d" % miner.out_rules(a.output_file, a.top_n_out, *bounds))
        if a.stats_file is not None:  # the pool's counts: the weights evaluated below stay the last iteration's
            miner.out_rule_stats(a.stats_file, a.top_n_out, *bounds)
    else:  # a rule file: no search, no learn
        print("#Rules read: %d" % miner.read_rules(a.rule_file))
        if a.stats_file is not None:
            print("#Rule statistics written: %d" % miner.write_list_stats(a.stats_file, a.pc))
    if a.weights == "conf":  # the confidences of the current lists become their weights
        miner.set_weights(miner.confidence(a.conf, a.pc))
    if a.agg != "sum":
        miner.set_aggregation(a.agg, a.agg_depth)
        try:
            miner._sync_aggregation()
        except ValueError as err:
            ap.error("-agg %s: %s (-weights conf takes the rules' confidences as weights)" % (a.agg, err))
    for split in {None: (), "both": ("valid", "test")}.get(a.evaluate, (a.evaluate,)):
        if a.side == "tail":
            print(metrics_line(split.capitalize(), miner.evaluate(split)))
            continue
        for side in (("tail", "head", "both") if a.side == "both" else (a.side,)):
            print(metrics_line("%s (%s)" % (split.capitalize(), side if side == "both" else side + "s"),
                               miner.evaluate(split, side=side)))
    if predicting:
        out = miner.predict(a.predict, queries, a.k, True, a.explain, a.rules_per_tail, a.candidates,
                            a.predictions_file, a.side, a.paths)
        print("#Predictions written: %d" % int(np.sum(out["valid"])))


if __name__ == "__main__":
    main()
