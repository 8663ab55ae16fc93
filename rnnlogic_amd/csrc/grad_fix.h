// The order-free node-gradient accumulator of the three training backward
// paths: the EM Predictor (predictor.hip), PredictorPlus SUM (backward.hip)
// and PNA (pna_grad.hip).  Not part of the C-ABI.
//
// The rule.  A stats pass takes the launch's max |incoming
// gradient| (as float bits) and its sum of path counts; the scale is 2^s with
// s = 61 minus ilogb(sum k x max |g|), so every term and every partial sum fits
// int64.  Each gradient goes onto the 2^s grid ONCE per candidate (to_fix) and
// is then multiplied by each bucket entry's integer count: a (node, candidate)
// pair split over several entries — the grounding's raw duplicates, which vary
// with its LDS hash's insertion order — sums exactly like its merged entry.
// The adds are integer (unsigned long long words: an LDS table for the head's
// first nodes, int64 HBM atomics past it), so their order does not matter; a
// consumer sums the workgroups' partial rows and rounds once (from_fix).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "internal.h"

namespace rnnl {

// Wave (64-lane) butterflies: every lane gets the result.
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// A launch's stats words (zeroed by the host before the stats pass): the bits
// of max |gradient|, the sum of the path counts of the entries that take a
// gradient, and (PNA) the number of candidates.
struct GradStats {
  unsigned int max_bits, pad;
  unsigned long long sum_k, n_cand;
};

// This lane's share into the launch's stats: one atomic per wave and word (a
// max and integer sums: order-free), none for a zero.
__device__ __forceinline__ void grad_stats_publish(unsigned int m, unsigned long long k, unsigned long long n,
                                                   GradStats *st) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    m = max(m, (unsigned int)__shfl_xor((int)m, o, 64));
    k += __shfl_xor(k, o, 64);
    n += __shfl_xor(n, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (m) atomicMax(&st->max_bits, m);
    if (k) atomicAdd(&st->sum_k, k);
    if (n) atomicAdd(&st->n_cand, n);
  }
}

// s of the launch's 2^s grid; 0 where there is no gradient.  bad: a non-finite
// gradient (each path keeps its own fallback).  with_cands (PNA): each
// candidate's whole min / max gradient lands in an accumulator as well, one
// more term per candidate than the count x gradient products.
__device__ __forceinline__ int grad_fix_scale(const GradStats *st, bool with_cands, bool &bad) {
  const unsigned int mb = st->max_bits;
  bad = mb >= 0x7f800000u;
  const double terms = with_cands ? (double)st->sum_k + (double)st->n_cand : (double)st->sum_k;
  const double total = terms * (double)__uint_as_float(mb);
  return (bad || !(total > 0.0)) ? 0 : 61 - ilogb(total);
}

__device__ __forceinline__ long long to_fix(double v, int sc) { return llrint(ldexp(v, sc)); }
__device__ __forceinline__ double from_fix(long long v, int sc) { return ldexp((double)v, -sc); }

// The accumulator word of (node n, dim d) of a 16-wide table: in the
// workgroup's LDS table for the nl nodes from lo, in the HBM table past them.
__device__ __forceinline__ unsigned long long *node_word(unsigned long long *lds, unsigned long long *hbm, int n,
                                                         int lo, int nl, int d) {
  const unsigned ln = (unsigned)(n - lo);
  return ln < (unsigned)nl ? &lds[ln * 16 + d] : &hbm[(int64_t)n * 16 + d];
}

// The consumer's integer sum over the accumulation workgroups' partial rows:
// word gid of row b (rows row_stride words apart) is added into a[b mod 4];
// a tail of nrow mod 4 rows goes into a[0].  Integer adds: any order gives the
// same bits, and four accumulators keep four loads in flight.  SUM has one
// table a row and adds the four up; PNA lays its four tables out as four rows
// per workgroup, so a[k] is table k's sum over 4 x workgroups rows.
__device__ __forceinline__ void sum_partial_rows(const long long *__restrict__ gpart, int nrow, int64_t row_stride,
                                                 int64_t gid, long long (&a)[4]) {
  int b = 0;
  for (; b + 4 <= nrow; b += 4)
#pragma unroll
    for (int u = 0; u < 4; ++u) a[u] += gpart[(int64_t)(b + u) * row_stride + gid];
  for (; b < nrow; ++b) a[0] += gpart[(int64_t)b * row_stride + gid];
}

// The trie nodes [lo, hi) that a launch of `head` can give a gradient: the
// head's trie (a training batch is one relation), every node for head < 0,
// none for a head without rules.
inline void head_node_range(const rnnl_rules_s *r, int head, int &lo, int &hi) {
  lo = 0;
  hi = r->d.n_nodes;
  if (head < 0) return;
  lo = std::max(r->head_root[head], 0);
  hi = r->head_root[head] < 0 ? lo : lo + r->head_nodes[head];
}

}  // namespace rnnl
