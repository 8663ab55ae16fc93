"""Golden rule pools with bodies of up to five relations, from the REFERENCE
miner (RuleMiner::search through ref_rule_search of oracle/_ref/libref_miner.so):
tests/golden/_rules_long_<graph>.npz for tests/test_gpu_miner_long.py.

Each small fixture holds a synthetic graph and the reference's pools:
    triples (n, 3), E, R, flat4, flat5   flat = (head, len, body...) in the reference's order
The UMLS fixture holds no pool, only what identifies it at max_length 4: the
rule count, the counts per length 1..4 and the sha256 of the flat int32 stream.

The graphs: three random ones (mixed, sparse, dense), one with two self-loop
triples (the reference records one body-less rule for each), and pairs of
graphs on either side of what the long search kernel holds in LDS (csrc/mine.hip):
    instar_*   2,048 / 2,049 in-edges of one tail (ICAP: staged / read from global memory)
    suffix_*   2,048 / 2,049 length-2 suffixes into one tail (S2CAP: sorted in LDS / edge by edge)
    set_*      a triple with fewer / more than 2,048 rules of its own (DCAP, the per-triple set)
Every pool is checked against a breadth-first restatement of rule_search in
Python before it is written, which also gives the per-triple figures above.

Usage: python tools/make_golden_rules_long.py
"""
import hashlib
import os
import random
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle import ground_c  # noqa: E402
from rnnlogic_amd import datasets  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")
ICAP = S2CAP = DCAP = 2048


def random_graph(E, R, n, seed, loops=()):
    rng = random.Random(seed)
    seen = set()
    while len(seen) < n:
        h, r, t = rng.randrange(E), rng.randrange(R), rng.randrange(E)
        if h != t:
            seen.add((h, r, t))
    tri = sorted(seen)
    rng.shuffle(tri)
    return tri + list(loops), E, R


def instar_graph(n_in):
    """Tail 0 with n_in in-edges: the triple (1, 0, 0) and n_in - 1 sources of
    one out-edge each.  1 reaches some of the sources in one, two and three
    hops, so the rules of (1, 0, 0) have lengths 2..5."""
    R = 5
    src = list(range(10, 10 + n_in - 1))
    tri = [(1, 0, 0)] + [(s, 1 + i % 4, 0) for i, s in enumerate(src)]
    tri += [(1, 1, src[0]), (1, 2, src[-1]), (1, 3, 2), (2, 4, src[1]), (2, 1, 3), (3, 2, src[-2]), (3, 3, 4),
            (4, 0, src[2]), (4, 4, src[len(src) // 2]), (3, 0, 1), (4, 1, 5), (5, 2, src[3])]
    return tri, 10 + n_in, R


def suffix_graph(n2):
    """n2 length-2 suffixes y -> z -> 0 into tail 0: 32 middle entities z with
    in-edges from sources y of one out-edge each; (1, 0, 0) reaches a few of
    the y in one, two and three hops."""
    R = 4
    zs = list(range(10, 42))
    tri = [(1, 0, 0)] + [(z, 1 + i % 3, 0) for i, z in enumerate(zs)]
    ny = n2 - 2  # (1, 3, z) and (3, 3, z) below are suffixes too
    ys = list(range(50, 50 + ny))
    per, k = ny // len(zs), 0
    for i, z in enumerate(zs):
        for _ in range(per + (1 if i < ny - per * len(zs) else 0)):
            tri.append((ys[k], (k + i) % R, z))
            k += 1
    assert k == ny
    tri += [(1, 1, 2), (2, 2, ys[0]), (2, 3, ys[-1]), (2, 0, 3), (3, 1, ys[ny // 2]), (3, 2, ys[7]), (1, 2, ys[3]),
            (1, 3, zs[5]), (3, 3, zs[9])]
    return tri, 50 + n2, R


def write_dataset(path, tri, E, R):
    with open(os.path.join(path, "entities.dict"), "w") as fo:
        for e in range(E):
            fo.write("%d\te%d\n" % (e, e))
    with open(os.path.join(path, "relations.dict"), "w") as fo:
        for r in range(R):
            fo.write("%d\tr%d\n" % (r, r))
    with open(os.path.join(path, "train.txt"), "w") as fo:
        for h, r, t in tri:
            fo.write("e%d\tr%d\te%d\n" % (h, r, t))
    for name in ("valid.txt", "test.txt"):
        with open(os.path.join(path, name), "w") as fo:
            h, r, t = tri[0]
            fo.write("e%d\tr%d\te%d\n" % (h, r, t))


def reference_pool(path, L, threads=8):
    m = ground_c.RefMiner(path)
    rules, sec = m.rule_search(L, threads=threads)
    m.close()
    return rules, sec


def restated_pool(tri, L):
    """rule_search, breadth first with the frontier deduplicated by (entity,
    prefix): the pool in the reference's order and the rules per triple."""
    out = {}
    for h, r, t in tri:
        out.setdefault(h, []).append((r, t))
    pool, per_triple = set(), []
    for h, r, t in tri:
        found = set()
        if h == t:
            found.add(())
        else:
            frontier = {(h, ())}
            for _ in range(L):
                nxt = set()
                for e, p in frontier:
                    for rel, dst in out.get(e, ()):
                        if (e, rel, dst) == (h, r, t):
                            continue
                        if dst == t:
                            found.add(p + (rel,))
                        else:
                            nxt.add((dst, p + (rel,)))
                frontier = nxt
            found.discard((r,))
        per_triple.append(len(found))
        pool.update((r, b) for b in found)
    return sorted(pool, key=lambda x: (x[0], len(x[1]), x[1])), per_triple


def suffixes_into(tri):
    """Per triple, what the kernel counts against S2CAP: the in-edges of the
    sources z of t's in-edges, z != t, (z, c2, t) not the triple itself."""
    ins = {}
    for h, r, t in tri:
        ins.setdefault(t, []).append((h, r))
    worst = 0
    for h, r, t in tri:
        if h == t:
            continue
        worst = max(worst, sum(len(ins.get(z, ())) for z, c2 in ins.get(t, ()) if z != t and not (z == h and c2 == r)))
    return worst, max(len(v) for v in ins.values())


def flat_of(rules):
    flat = []
    for hd, body in rules:
        flat += [hd, len(body)] + list(body)
    return np.asarray(flat, dtype=np.int16)


def main():
    graphs = {
        "rand60": random_graph(60, 6, 360, 1),
        "sparse300": random_graph(300, 7, 1500, 2),
        "dense40": random_graph(40, 4, 400, 3),
        "loops30": random_graph(30, 3, 120, 4, loops=[(5, 0, 5), (7, 1, 7)]),
        "instar_2048": instar_graph(ICAP),
        "instar_2049": instar_graph(ICAP + 1),
        "suffix_2048": suffix_graph(S2CAP),
        "suffix_2049": suffix_graph(S2CAP + 1),
        "set_over": random_graph(8, 5, 140, 5),
    }
    for name, (tri, E, R) in graphs.items():
        with tempfile.TemporaryDirectory() as tmp:
            write_dataset(tmp, tri, E, R)
            pools = {}
            for L in (4, 5):
                pools[L], sec = reference_pool(tmp, L)
                mine, per_triple = restated_pool(tri, L)
                assert mine == pools[L], (name, L)
            n2, nin = suffixes_into(tri)
            print("%-12s E %4d R %d triples %4d | rules L4 %6d L5 %6d | reference %.2f s | most rules of one triple "
                  "%d, in-edges %d, suffixes %d" % (name, E, R, len(tri), len(pools[4]), len(pools[5]), sec,
                                                    max(per_triple), nin, n2))
            if name.startswith("instar"):
                assert nin == int(name.split("_")[1])
            if name.startswith("suffix"):
                assert n2 == int(name.split("_")[1])
            if name == "set_over":
                assert max(per_triple) > DCAP
            if name == "dense40":  # the other side of set_over
                assert max(per_triple) < DCAP
            if name == "loops30":
                assert (0, ()) in pools[5] and (1, ()) in pools[4]
            np.savez_compressed(os.path.join(GOLDEN, "_rules_long_%s.npz" % name),
                                triples=np.asarray(tri, dtype=np.int16), E=E, R=R, flat4=flat_of(pools[4]),
                                flat5=flat_of(pools[5]))
    rules, sec = reference_pool(datasets.materialize("umls"), 4, threads=16)
    flat = []
    for hd, body in rules:
        flat += [hd, len(body)] + list(body)
    per_len = [sum(1 for _, b in rules if len(b) == k) for k in range(1, 5)]
    digest = hashlib.sha256(np.asarray(flat, dtype=np.int32).tobytes()).hexdigest()
    print("umls L4: %d rules, per length %r, reference %.1f s (16 threads), sha256 %s" % (len(rules), per_len, sec,
                                                                                        digest))
    np.savez_compressed(os.path.join(GOLDEN, "_rules_long_umls_L4.npz"), count=len(rules),
                        per_len=np.asarray(per_len, dtype=np.int64), sha256=digest)


if __name__ == "__main__":
    main()
