// What the miner's evaluation (mine_eval.hip) and its predictions
// (mine_predict.hip) share: the layout of a workgroup's dense arrays, the
// grounding of one round of EW rules and the round's rules added into val.
// One copy of each, so the scores of a prediction are the evaluation's bit for
// bit.  Both files are compiled without contraction (-ffp-contract=off).
//
// Layout per workgroup, E entities: val (f64 x E), then per wave w the integer
// scratch counts A, counts B (u64 x E each), list A, list B (int x E each):
// EVAL_PER_E bytes per entity.  Up to EVAL_LDS_E entities it lives in LDS,
// above that in the handle's eval_scratch, zeroed when allocated and left
// zeroed by every query.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "internal.h"

namespace rnnl {

constexpr int EB = 256;          // threads per workgroup
constexpr int EW = EB / 64;      // waves: rules grounded at once
constexpr int EVAL_LDS_E = 512;  // everything in LDS up to this many entities (52 KiB)
constexpr size_t EVAL_PER_E = 8 + EW * 24;  // val (f64) + per wave: counts A, B (u64), lists A, B (int)
constexpr size_t EVAL_SCRATCH = 256u << 20;
constexpr int EVAL_MAX_BLOCKS = 2048;

enum : int { E_RANGE = 1, E_INVALID = 2, E_INTERNAL = 3 };

__device__ __forceinline__ unsigned long long eval_ld_u64(unsigned long long *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// first index in [lo, hi) of the (relation, other end)-sorted edges with relation >= r
__device__ __forceinline__ int eval_edge_lower(const int32_t *rel, int lo, int hi, int r) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (rel[mid] < r)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// SMALL: zero the integer scratch once per workgroup (the global scratch is
// zeroed when it is allocated and left zeroed by every query)
__device__ __forceinline__ void eval_zero_ints(unsigned char *ints, int E) {
  for (int i = threadIdx.x; i < EW * 2 * E; i += EB) {
    const int w = i / (2 * E);
    reinterpret_cast<unsigned long long *>(ints + (size_t)w * 24 * (size_t)E)[i - w * 2 * E] = 0ull;
  }
}

// Grounds rules rb + jb .. rb + jb + nw - 1 (nw <= EW) of relation r, wave w
// rule jb + w: frontier list + dense u64 path counts per hop in the wave's
// integer scratch, integer atomics only; every edge equal to (h, r, t) skipped
// on every hop.  Tail side (HEAD false): forward from h along the body over the
// out-edges (so_*), t = -1: no edge is skipped.  Head side: backward from t,
// hop k takes body[len - 1 - k] over the in-edges (si_*, under in_off), so the
// count at e is #paths(e -> t along the body); h = -1: no edge is skipped.  On
// return s_na[w] is the number of destinations of wave w's rule; its list and
// counts are in the half of the scratch that (length & 1) names.  Called by the
// whole workgroup.
template <bool HEAD>
__device__ __forceinline__ void eval_ground_round(const MinerDev &d, const MinerLearnDev &l, unsigned char *ints,
                                                  int h, int r, int t, int rb, int jb, int nw, int *s_n, int *s_na,
                                                  bool &wide) {
  const int E = d.E, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int32_t *e_off = HEAD ? d.in_off : d.out_off;   // the edges of an entity on this side,
  const int32_t *e_rel = HEAD ? l.si_rel : l.so_rel;    // sorted by (relation, other end)
  const int32_t *e_end = HEAD ? l.si_src : l.so_dst;
  const int start = HEAD ? t : h;
  int mx = 0;
  for (int w = 0; w < nw; ++w) mx = max(mx, l.rule_len[rb + jb + w]);
  const int rule = rb + jb + wid;
  const int len = wid < nw ? l.rule_len[rule] : 0;
  unsigned long long *ca = reinterpret_cast<unsigned long long *>(ints + (size_t)wid * 24 * (size_t)E);
  unsigned long long *cb = ca + E;
  int *la = reinterpret_cast<int *>(cb + E), *lb = la + E;
  int na = 0;
  if (len > 0) {
    if (lane == 0) {
      la[0] = start;
      ca[start] = 1;
    }
    na = 1;
  }
  for (int k = 0; k < mx; ++k) {
    const bool act = k < len;
    if (act && lane == 0) s_n[wid] = 0;
    __syncthreads();
    if (act) {
      const int rel = l.rule_body[RULE_STRIDE * rule + (HEAD ? len - 1 - k : k)];
      for (int i = lane; i < na; i += 64) {
        const int e = la[i];
        const unsigned long long n = eval_ld_u64(&ca[e]);
        const int en = e_off[e + 1];
        for (int b = eval_edge_lower(e_rel, e_off[e], en, rel); b < en && e_rel[b] == rel; ++b) {
          const int x = e_end[b];
          // the query's own edge, and every copy of it: (e, rel, x) forward, (x, rel, e) backward
          if (rel == r && (HEAD ? (x == h && e == t) : (e == h && x == t))) continue;
          wide |= n > 0xffffffffull;  // the paths through here alone are past 32 bits
          if (atomicAdd(&cb[x], n) == 0) lb[atomicAdd(&s_n[wid], 1)] = x;
        }
      }
    }
    __syncthreads();
    if (act) {
      for (int i = lane; i < na; i += 64) ca[la[i]] = 0;
      na = s_n[wid];
      unsigned long long *tc = ca;
      ca = cb;
      cb = tc;
      int *tl = la;
      la = lb;
      lb = tl;
    }
  }
  if (lane == 0) s_na[wid] = na;
  __syncthreads();
}

// the final counts and destination list of wave w's rule of length len (> 0)
__device__ __forceinline__ void eval_final(unsigned char *ints, int E, int w, int len, unsigned long long *&fc,
                                           const int *&fl) {
  unsigned long long *c0 = reinterpret_cast<unsigned long long *>(ints + (size_t)w * 24 * (size_t)E);
  const int *l0 = reinterpret_cast<const int *>(c0 + 2 * (size_t)E);
  fc = (len & 1) ? c0 + E : c0;  // one swap per hop
  fl = (len & 1) ? l0 + E : l0;
}

// The round's rules into val, one after the other: list order per destination,
// product first, then the add; the destinations of one rule are distinct, so no
// floating-point atomics.  Leaves the integer scratch zeroed.  REACHED: bit 0 of
// reached[x] is set for every destination (a path count > 0, whatever the
// weight), and a destination reached for the first time is appended to
// touched[*n_touched] (an LDS counter): the entities whose val was written.
template <bool REACHED>
__device__ __forceinline__ void eval_round_into_val(const MinerLearnDev &l, unsigned char *ints, int E, int rb, int jb,
                                                    int nw, const int *s_na, double *val, unsigned char *reached,
                                                    int *touched, int *n_touched, bool &wide) {
  for (int w = 0; w < nw; ++w) {
    const int len2 = l.rule_len[rb + jb + w];
    if (len2 == 0) continue;  // an empty body reaches nothing
    const double wt = l.wt[rb + jb + w];
    unsigned long long *fc;
    const int *fl;
    eval_final(ints, E, w, len2, fc, fl);
    const int n2 = s_na[w];
    for (int i = threadIdx.x; i < n2; i += EB) {
      const int x = fl[i];
      const unsigned long long c = eval_ld_u64(&fc[x]);
      wide |= c > 0xffffffffull;
      const double term = wt * (double)c;
      val[x] = val[x] + term;
      if (REACHED && c > 0 && !reached[x]) {  // one thread per x within a rule, a barrier between rules
        reached[x] = 1;
        touched[atomicAdd(n_touched, 1)] = x;
      }
      fc[x] = 0;
    }
    __syncthreads();
  }
}

// The per-workgroup global scratch of graphs past EVAL_LDS_E entities, kept in
// the handle: workgroups bounded by their scratch; zeroed once, every query
// leaves it zeroed.
inline int eval_scratch_ensure(rnnl_miner m, const char *who) {
  if (m->eval_scratch) return RNNL_OK;
  const size_t E = (size_t)m->d.E;
  const int32_t blocks =
      (int32_t)std::max<size_t>(16, std::min<size_t>(EVAL_MAX_BLOCKS, EVAL_SCRATCH / (EVAL_PER_E * E)));
  void *p = nullptr;
  if (hipMalloc(&p, (size_t)blocks * EVAL_PER_E * E) != hipSuccess) {
    set_error(std::string(who) + ": device allocation failed");
    return RNNL_ERR_NOMEM;
  }
  m->bufs.push_back(p);
  RNNL_HIP_CHECK(hipMemset(p, 0, (size_t)blocks * EVAL_PER_E * E));
  RNNL_HIP_CHECK(hipDeviceSynchronize());
  m->eval_scratch = static_cast<unsigned char *>(p);
  m->eval_blocks = blocks;
  return RNNL_OK;
}

}  // namespace rnnl
