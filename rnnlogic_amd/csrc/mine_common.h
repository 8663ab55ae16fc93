// What every kernel file of the rule miner shares (mine.hip, mine_learn.hip,
// mine_stats.hip and, through mine_ground.h, mine_eval.hip, mine_predict.hip
// and mine_paths.hip): the counter slots, the search in a sorted int array, the
// relaxed u64 load, and the path-count grounding of mine_learn.hip and
// mine_ground.h: its scratch block and its hop.  One copy of each, so what
// scores() grounds is what learn() grounds, hop for hop.
#pragma once
#include <hip/hip_runtime.h>

#include "internal.h"

namespace rnnl {

// The four u64 counters every miner entry point takes, zeroed by the entry and
// read by the caller after it.  CTR_TOTAL: the entries of a chunk
// (rnnl_miner_ground_count); CTR_RANGE: a path count past 32 bits; CTR_INVALID:
// a triple, query or slot out of range; CTR_INTERNAL: the kernel met a state it
// rules out.  (The rule search of mine.hip counts other things in its slots:
// work queue, table full, keys written.)
enum : int { CTR_TOTAL = 0, CTR_RANGE = 1, CTR_INVALID = 2, CTR_INTERNAL = 3 };

__device__ __forceinline__ unsigned long long ld_u64(unsigned long long *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// first index in a[lo, hi) with a[i] >= k: a sorted int array in LDS or global
// memory; on the relations of an entity's (relation, other end)-sorted edges,
// the start of relation k's run
template <typename P>
__device__ __forceinline__ int lower_bound_i(P a, int lo, int hi, int k) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < k)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// The integer scratch of one grounding, E entities: counts A, counts B (u64 x E
// each), list A, list B (int x E each).  ca / la are the frontier (its dense
// path counts and its entities), cb / lb the next one; one swap per hop.
constexpr size_t GROUND_PER_E = 24;

struct GroundScratch {
  unsigned long long *ca, *cb;
  int *la, *lb;
  // block: the start of the scratch, idx: this grounding's block in it
  __device__ __forceinline__ GroundScratch(unsigned char *block, size_t idx, int E) {
    ca = reinterpret_cast<unsigned long long *>(block + idx * GROUND_PER_E * (size_t)E);
    cb = ca + E;
    la = reinterpret_cast<int *>(cb + E);
    lb = la + E;
  }
  // The view after `hops` swaps, for a reader of the result: ca / la are the
  // half that holds the last frontier.  Written as an offset into the block
  // chosen by the parity, not as a choice between two pointers: the compiler
  // keeps the first form as one masked add in the query kernels' rule loop.
  __device__ __forceinline__ static GroundScratch after(unsigned char *block, size_t idx, int E, int hops) {
    GroundScratch s(block, idx, E);
    unsigned long long *c0 = s.ca;
    int *l0 = reinterpret_cast<int *>(c0 + 2 * (size_t)E);
    s.ca = (hops & 1) ? c0 + E : c0;
    s.cb = (hops & 1) ? c0 : c0 + E;
    s.la = (hops & 1) ? l0 + E : l0;
    s.lb = (hops & 1) ? l0 : l0 + E;
    return s;
  }
  __device__ __forceinline__ void swap() {
    unsigned long long *tc = ca;
    ca = cb;
    cb = tc;
    int *tl = la;
    la = lb;
    lb = tl;
  }
};

// One hop of one wave: the frontier s.la[0, na) with the counts s.ca expands
// along relation rel into s.cb, an entity first touched appended to s.lb under
// the list counter *n_next (zeroed by the caller; integer atomics only).  Tail
// side (HEAD false): over the out-edges (so_*), forward; head side: over the
// in-edges (si_*, under in_off), backward.  Every copy of the query's own edge
// (h, r, t) is skipped: (e, rel, x) forward, (x, rel, e) backward; a side's far
// end at -1 skips nothing.  wide is set when a frontier count past 32 bits is
// carried over an edge.  The barriers before and after, the reset of the old
// frontier and the swap belong to the caller.
// COUNT false (the noisy-or and max aggregations of mine_ground.h, which ask
// only whether a rule reaches an entity): the dense slots hold 1 where the
// frontier is, not path counts: the first touch is an integer atomic OR with 1,
// the append as before; no count is read or carried and wide is never set.
template <bool HEAD, bool COUNT = true>
__device__ __forceinline__ void ground_hop(const MinerDev &d, const MinerLearnDev &l, const GroundScratch &s, int na,
                                           int lane, int rel, int h, int r, int t, int *n_next, bool &wide) {
  const int32_t *e_off = HEAD ? d.in_off : d.out_off;   // the edges of an entity on this side,
  const int32_t *e_rel = HEAD ? l.si_rel : l.so_rel;    // sorted by (relation, other end)
  const int32_t *e_end = HEAD ? l.si_src : l.so_dst;
  for (int i = lane; i < na; i += 64) {
    const int e = s.la[i];
    const unsigned long long n = COUNT ? ld_u64(&s.ca[e]) : 1ull;
    const int en = e_off[e + 1];
    for (int b = lower_bound_i(e_rel, e_off[e], en, rel); b < en && e_rel[b] == rel; ++b) {
      const int x = e_end[b];
      if (rel == r && (HEAD ? (x == h && e == t) : (e == h && x == t))) continue;
      if (COUNT) {
        wide |= n > 0xffffffffull;  // the paths through here alone are past 32 bits
        if (atomicAdd(&s.cb[x], n) == 0) s.lb[atomicAdd(n_next, 1)] = x;
      } else {
        if (atomicOr(&s.cb[x], 1ull) == 0) s.lb[atomicAdd(n_next, 1)] = x;
      }
    }
  }
}

}  // namespace rnnl
