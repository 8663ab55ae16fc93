// Rule mining on the GPU: the reference miner's
// RuleMiner::search (miner/rnnlogic.cpp:505-589) — for every train triple
// (h, r, t), every relation path of length <= L from h that reaches t while
// the triple's own edge is removed (KnowledgeGraph::rule_search,
// rnnlogic.cpp:350-382) becomes a rule r <- body; the pool is the set of
// distinct (head, body) over all triples, minus the trivial r <- r.
//
// The reference enumerates every path by DFS (deg^L per triple).  Here one
// workgroup per triple (dynamic dequeue):
//   depth 1  the out-edges of h (coalesced CSR range);
//   depth 2  load-balanced expansion of the depth-1 entities' out-edges
//            (block scan of degrees + binary search, as the grounding kernel);
//   depth 3  never expanded: a path ends at t iff its depth-2 entity y has an
//            edge (y, r3, t), so t's in-edges (sorted by source, staged in LDS)
//            are binary-searched for y — deg^2 work per triple instead of deg^3.
// A walk stops at t (the DFS returns at the goal), and the removed edge
// (h, r, t) is skipped at every depth, as in rule_search.  Rules are keyed
// head | len | b1 | b2 | b3 (15 bits each; numeric key order == the
// reference's std::set<Rule> order within a head) and inserted into a global
// open-addressing set, after a per-triple LDS set that drops the duplicates
// one triple produces.  Bodies of four and five relations: mine_long_kernel
// below (rnnl_rule_search_long), with keys and h == t handling of its own.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <numeric>
#include <string>
#include <vector>

#include "internal.h"
#include "mine_common.h"  // lower_bound_i

namespace rnnl {

constexpr int MB = 256;             // threads per workgroup
constexpr int ICAP = 2048;          // in-edges of t staged in LDS (else read from global)
constexpr int DBITS = 11;
constexpr int DCAP = 1 << DBITS;    // per-triple dedupe set
constexpr uint64_t KEMPTY = ~0ull;
constexpr int GPROBE = 1 << 14;     // global set probe bound (overflow past it)

__device__ __forceinline__ uint64_t rule_key(int head, int len, int b1, int b2, int b3) {
  return ((uint64_t)head << 47) | ((uint64_t)len << 45) | ((uint64_t)b1 << 30) | ((uint64_t)b2 << 15) |
         (uint64_t)b3;
}

__device__ __forceinline__ uint64_t key_hash(uint64_t k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdULL;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ULL;
  return k ^ (k >> 33);
}

struct MineSmem {
  int in_src[ICAP], in_rel[ICAP];
  unsigned long long dd[DCAP];
  int it_x[MB], it_r1[MB], it_off[MB];
  int ws[MB / 64 + 1];
  int q;
};

__device__ __forceinline__ void global_insert(uint64_t key, unsigned long long *table, int64_t cap,
                                              unsigned long long *flags) {
  uint64_t h = key_hash(key) & (uint64_t)(cap - 1);
  if (__hip_atomic_load(&flags[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;  // already too small
  for (int p = 0; p < GPROBE; ++p) {
    const unsigned long long v = __hip_atomic_load(&table[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (v == key) return;
    if (v == KEMPTY) {
      const unsigned long long old = atomicCAS(&table[h], KEMPTY, (unsigned long long)key);
      if (old == KEMPTY || old == key) return;
    }
    h = (h + 1) & (uint64_t)(cap - 1);
  }
  atomicOr(&flags[1], 1ull);  // set full: the caller retries with a larger table
}

template <typename SM>
__device__ __forceinline__ void emit_rule(SM &S, uint64_t key, unsigned long long *table, int64_t cap,
                                          unsigned long long *flags) {
  uint32_t h = (uint32_t)key_hash(key) & (DCAP - 1);
  for (int p = 0; p < 32; ++p) {
    const unsigned long long old = atomicCAS(&S.dd[h], KEMPTY, (unsigned long long)key);
    if (old == key) return;  // this triple already produced it
    if (old == KEMPTY) break;
    h = (h + 1) & (DCAP - 1);
  }
  global_insert(key, table, cap, flags);
}

__device__ __forceinline__ int mine_scan(int x, int *s_ws, int &total) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  int v = x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(v, o, 64);
    if (lane >= o) v += y;
  }
  if (lane == 63) s_ws[wid] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    int acc = 0;
    for (int w = 0; w < MB / 64; ++w) {
      const int t = s_ws[w];
      s_ws[w] = acc;
      acc += t;
    }
    s_ws[MB / 64] = acc;
  }
  __syncthreads();
  const int res = v - x + s_ws[wid];
  total = s_ws[MB / 64];
  __syncthreads();
  return res;
}

__global__ __launch_bounds__(MB) void mine_kernel(MinerDev m, int L, unsigned long long *table, int64_t cap,
                                                  unsigned long long *flags) {
  __shared__ MineSmem S;
  const int tid = threadIdx.x;
#pragma unroll 1
  while (true) {
    __syncthreads();
    if (tid == 0) {
      // a full set ends the search early: the caller retries with a larger table
      const bool full = __hip_atomic_load(&flags[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
      S.q = full ? m.n : (int)atomicAdd(&flags[0], 1ull);
    }
    __syncthreads();
    const int q = S.q;
    if (q >= m.n) break;
    const int h = m.th[q], r = m.tr[q], t = m.tt[q];
    // t's in-edges (sources ascending), staged when they fit
    const int ib = m.in_off[t], nin = m.in_off[t + 1] - ib;
    const bool staged = nin <= ICAP;
    if (staged)
      for (int i = tid; i < nin; i += MB) {
        S.in_src[i] = m.in_src[ib + i];
        S.in_rel[i] = m.in_rel[ib + i];
      }
    for (int i = tid; i < DCAP; i += MB) S.dd[i] = KEMPTY;
    __syncthreads();
    const int *isrc = staged ? S.in_src : m.in_src + ib;
    const int *irel = staged ? S.in_rel : m.in_rel + ib;
    const int ob = m.out_off[h], n1 = m.out_off[h + 1] - ob;
    for (int c1 = 0; c1 < n1; c1 += MB) {
      const int i = c1 + tid;
      int deg = 0;
      S.it_x[tid] = -1;
      if (i < n1) {
        const int x = m.out_dst[ob + i], r1 = m.out_rel[ob + i];
        if (!(r1 == r && x == t)) {  // the triple's own edge (rule_search's removed_triplet)
          if (x == t) {
            if (r1 != r) emit_rule(S, rule_key(r, 1, r1, 0, 0), table, cap, flags);  // r <- r is erased
          } else if (L >= 2) {
            S.it_x[tid] = x;
            S.it_r1[tid] = r1;
            deg = m.out_off[x + 1] - m.out_off[x];
          }
        }
      }
      int NE;
      S.it_off[tid] = mine_scan(deg, S.ws, NE);
      __syncthreads();
      const int nit = min(MB, n1 - c1);
      for (int e0 = 0; e0 < NE; e0 += MB) {
        const int j = e0 + tid;
        if (j < NE) {
          int lo = 0, hi = nit - 1;  // largest item with it_off <= j
          while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (S.it_off[mid] <= j)
              lo = mid;
            else
              hi = mid - 1;
          }
          const int x = S.it_x[lo], r1 = S.it_r1[lo];
          const int k = m.out_off[x] + (j - S.it_off[lo]);
          const int y = m.out_dst[k], r2 = m.out_rel[k];
          if (!(x == h && r2 == r && y == t)) {
            if (y == t) {
              emit_rule(S, rule_key(r, 2, r1, r2, 0), table, cap, flags);
            } else if (L >= 3) {
              for (int a = lower_bound_i(isrc, 0, nin, y); a < nin && isrc[a] == y; ++a) {
                const int r3 = irel[a];
                if (!(y == h && r3 == r)) emit_rule(S, rule_key(r, 3, r1, r2, r3), table, cap, flags);
              }
            }
          }
        }
      }
      __syncthreads();
    }
  }
}

// ------------------------------------------------- bodies of up to five relations
// rnnl_rule_search_long.  A path h = x0 -> ... -> xk = t is a rule iff every
// intermediate node differs from t and no hop equals (h, r, t) by value: both
// tests are local to a node or an edge, so the rules of length a + 2 are the
// exact join, on the middle entity y != t, of the valid forward prefixes
// (y, b1..ba) from h with the valid length-2 suffixes (y, c1, c2) into t.
//   suffixes  two levels of t's in-edges, packed y | c1 | c2, sorted in LDS
//             (bitonic) when at most suffix_cap of them; equal neighbours are
//             skipped when they are read.  Past that nothing is staged and a
//             suffix is found edge by edge: the out-edges of y whose target
//             has an in-edge of t (binary search of t's in-edges) — the same
//             set, so no capacity truncates anything.
//   forward   depth 1 and 2 streamed as in mine_kernel (lengths 1..3 are found
//             as there); length 4 joins depth 2 with the suffixes; for length 5
//             each chunk of depth-2 paths is expanded once more (second block
//             scan + binary search) and depth 3 is joined.
// A triple with h == t gives the reference's one body-less rule (the DFS
// returns at the goal at depth 0).  Keys: head | len (3 bits) | b1 .. b_slots,
// `bits` per relation, slots = max_length, bodies left-aligned.
constexpr int S2CAP = 2048;  // length-2 suffixes of t sorted in LDS (else edge by edge)

struct LongKey {
  int bits, slots;
};

__device__ __forceinline__ uint64_t lk_head(LongKey f, int head, int len) {
  return ((((uint64_t)head) << 3) | (uint64_t)len) << (f.slots * f.bits);
}
// body relation number i (0-based, i < slots)
__device__ __forceinline__ uint64_t lk_body(LongKey f, int i, int b) {
  return (uint64_t)b << ((f.slots - 1 - i) * f.bits);
}

struct LongSmem {
  int in_src[ICAP], in_rel[ICAP];
  unsigned long long dd[DCAP];
  unsigned long long s2[S2CAP];
  int it_x[MB], it_r1[MB], it_off[MB];
  int i2_y[MB], i2_off[MB];
  unsigned long long i2_p[MB];
  int ws[MB / 64 + 1];
  unsigned long long n2;
  int q;
};

// largest item in [0, MB) with off[item] <= j (items of degree 0 share the offset of their successor)
__device__ __forceinline__ int item_of(const int *off, int j) {
  int lo = 0, hi = MB - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= j)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

// every rule pre | c1 | c2 (slots i and i + 1) whose last two hops y -c1-> z -c2-> t are valid; y != t
template <typename P>
__device__ __forceinline__ void join_suffix(LongSmem &S, const MinerDev &m, LongKey f, bool sorted, int n2, int y,
                                            uint64_t pre, int i, int h, int r, int t, P isrc, P irel, int nin,
                                            unsigned long long *table, int64_t cap, unsigned long long *flags) {
  if (sorted) {
    const unsigned long long want = (unsigned long long)(unsigned)y << 32;
    int lo = 0, hi = n2;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (S.s2[mid] < want)
        lo = mid + 1;
      else
        hi = mid;
    }
    unsigned long long prev = KEMPTY;
    for (int a = lo; a < n2; ++a) {
      const unsigned long long v = S.s2[a];
      if ((int)(v >> 32) != y) break;
      if (v != prev)
        emit_rule(S, pre | lk_body(f, i, (int)((v >> 16) & 0xffff)) | lk_body(f, i + 1, (int)(v & 0xffff)), table, cap,
                  flags);
      prev = v;
    }
  } else {
    for (int k = m.out_off[y], ke = m.out_off[y + 1]; k < ke; ++k) {
      const int z = m.out_dst[k];
      if (z == t) continue;  // the walk stops at t (and the triple's own edge ends there)
      const uint64_t p1 = pre | lk_body(f, i, m.out_rel[k]);
      for (int a = lower_bound_i(isrc, 0, nin, z); a < nin && isrc[a] == z; ++a) {
        const int c2 = irel[a];
        if (!(z == h && c2 == r)) emit_rule(S, p1 | lk_body(f, i + 1, c2), table, cap, flags);
      }
    }
  }
}

template <typename P>
__device__ __forceinline__ void long_triple(LongSmem &S, const MinerDev &m, int L, LongKey f, int h, int r, int t,
                                            bool sorted, int n2, P isrc, P irel, int nin,
                                            unsigned long long *table, int64_t cap, unsigned long long *flags) {
  const int tid = threadIdx.x;
  const int ob = m.out_off[h], n1 = m.out_off[h + 1] - ob;
  for (int c1 = 0; c1 < n1; c1 += MB) {
    const int i = c1 + tid;
    int deg = 0;
    S.it_x[tid] = -1;
    if (i < n1) {
      const int x = m.out_dst[ob + i], r1 = m.out_rel[ob + i];
      if (!(r1 == r && x == t)) {  // the triple's own edge
        if (x == t) {
          if (r1 != r) emit_rule(S, lk_head(f, r, 1) | lk_body(f, 0, r1), table, cap, flags);  // r <- r is erased
        } else if (L >= 2) {
          S.it_x[tid] = x;
          S.it_r1[tid] = r1;
          deg = m.out_off[x + 1] - m.out_off[x];
        }
      }
    }
    int NE;
    S.it_off[tid] = mine_scan(deg, S.ws, NE);
    __syncthreads();
    for (int e0 = 0; e0 < NE; e0 += MB) {
      const int j = e0 + tid;
      int deg2 = 0;
      S.i2_y[tid] = -1;
      if (j < NE) {
        const int it = item_of(S.it_off, j);
        const int x = S.it_x[it], r1 = S.it_r1[it];
        const int k = m.out_off[x] + (j - S.it_off[it]);
        const int y = m.out_dst[k], r2 = m.out_rel[k];
        if (!(x == h && r2 == r && y == t)) {
          const uint64_t p2 = lk_body(f, 0, r1) | lk_body(f, 1, r2);
          if (y == t) {
            emit_rule(S, lk_head(f, r, 2) | p2, table, cap, flags);
          } else if (L >= 3) {
            for (int a = lower_bound_i(isrc, 0, nin, y); a < nin && isrc[a] == y; ++a) {
              const int r3 = irel[a];
              if (!(y == h && r3 == r)) emit_rule(S, lk_head(f, r, 3) | p2 | lk_body(f, 2, r3), table, cap, flags);
            }
            if (L >= 4)
              join_suffix(S, m, f, sorted, n2, y, lk_head(f, r, 4) | p2, 2, h, r, t, isrc, irel, nin, table, cap,
                          flags);
            if (L >= 5) {
              S.i2_y[tid] = y;
              S.i2_p[tid] = p2;
              deg2 = m.out_off[y + 1] - m.out_off[y];
            }
          }
        }
      }
      if (L >= 5) {  // the chunk's depth-2 paths once more
        int NE2;
        S.i2_off[tid] = mine_scan(deg2, S.ws, NE2);
        __syncthreads();
        for (int f0 = 0; f0 < NE2; f0 += MB) {
          const int g = f0 + tid;
          if (g < NE2) {
            const int it = item_of(S.i2_off, g);
            const int y = S.i2_y[it];
            const int k = m.out_off[y] + (g - S.i2_off[it]);
            const int z = m.out_dst[k];
            if (z != t)  // at t the walk stops: that rule has length 3
              join_suffix(S, m, f, sorted, n2, z, lk_head(f, r, 5) | S.i2_p[it] | lk_body(f, 2, m.out_rel[k]), 3, h, r,
                          t, isrc, irel, nin, table, cap, flags);
          }
        }
        __syncthreads();
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(MB) void mine_long_kernel(MinerDev m, int L, LongKey f, int s2cap,
                                                       unsigned long long *table, int64_t cap,
                                                       unsigned long long *flags) {
  __shared__ LongSmem S;
  const int tid = threadIdx.x;
#pragma unroll 1
  while (true) {
    __syncthreads();
    if (tid == 0) {
      const bool full = __hip_atomic_load(&flags[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
      S.q = full ? m.n : (int)atomicAdd(&flags[0], 1ull);
      S.n2 = 0;
    }
    __syncthreads();
    const int q = S.q;
    if (q >= m.n) break;
    const int h = m.th[q], r = m.tr[q], t = m.tt[q];
    if (h == t) {  // the goal is reached at depth 0: one rule without a body, nothing else
      if (tid == 0) global_insert(lk_head(f, r, 0), table, cap, flags);
      continue;
    }
    const int ib = m.in_off[t], nin = m.in_off[t + 1] - ib;
    const bool staged = nin <= ICAP;
    if (staged)
      for (int i = tid; i < nin; i += MB) {
        S.in_src[i] = m.in_src[ib + i];
        S.in_rel[i] = m.in_rel[ib + i];
      }
    for (int i = tid; i < DCAP; i += MB) S.dd[i] = KEMPTY;
    bool sorted = false;
    int n2 = 0;
    if (L >= 4) {
      // the length-2 suffixes y -c1-> z -c2-> t: z != t, (z, c2, t) not the triple's own edge, y != t
      for (int i = tid; i < nin; i += MB) {
        const int z = m.in_src[ib + i], c2 = m.in_rel[ib + i];
        if (z == t || (z == h && c2 == r)) continue;
        const int zb = m.in_off[z], nz = m.in_off[z + 1] - zb;
        const unsigned long long base = atomicAdd(&S.n2, (unsigned long long)nz);
        if (base + (unsigned long long)nz <= (unsigned long long)s2cap)
          for (int k = 0; k < nz; ++k) {
            const int y = m.in_src[zb + k];
            S.s2[base + k] = y == t ? KEMPTY
                                    : ((unsigned long long)(unsigned)y << 32) |
                                          ((unsigned long long)m.in_rel[zb + k] << 16) | (unsigned long long)c2;
          }
      }
      __syncthreads();
      sorted = S.n2 <= (unsigned long long)s2cap;
      if (sorted) {
        n2 = (int)S.n2;
        int P = 1;
        while (P < n2) P <<= 1;
        for (int i = n2 + tid; i < P; i += MB) S.s2[i] = KEMPTY;
        __syncthreads();
        for (int k = 2; k <= P; k <<= 1)
          for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += MB) {
              const int o = i ^ j;
              if (o > i) {
                const unsigned long long a = S.s2[i], b = S.s2[o];
                if ((a > b) == ((i & k) == 0)) {
                  S.s2[i] = b;
                  S.s2[o] = a;
                }
              }
            }
            __syncthreads();
          }
      }
    }
    __syncthreads();
    if (staged)
      long_triple(S, m, L, f, h, r, t, sorted, n2, (const int *)S.in_src, (const int *)S.in_rel, nin, table, cap,
                  flags);
    else
      long_triple(S, m, L, f, h, r, t, sorted, n2, m.in_src + ib, m.in_rel + ib, nin, table, cap, flags);
  }
}

__global__ void compact_kernel(const unsigned long long *__restrict__ table, int64_t cap,
                               unsigned long long *__restrict__ out, int64_t out_cap,
                               unsigned long long *__restrict__ flags) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += (int64_t)gridDim.x * blockDim.x) {
    const unsigned long long k = table[i];
    if (k != KEMPTY) {
      const unsigned long long pos = atomicAdd(&flags[2], 1ull);
      if ((int64_t)pos < out_cap) out[pos] = k;
    }
  }
}

}  // namespace rnnl

using namespace rnnl;

extern "C" {

int rnnl_miner_create(const int32_t *hrt, int64_t n, int32_t E, int32_t R, rnnl_miner *out) {
  if (!out || n < 0 || E <= 0 || R <= 0 || (n > 0 && !hrt) || R >= (1 << 15) || n >= INT32_MAX) {
    set_error("rnnl_miner_create: bad arguments (R < 32768 required)");
    return RNNL_ERR_INVALID;
  }
  for (int64_t i = 0; i < n; ++i)
    if (hrt[3 * i] < 0 || hrt[3 * i] >= E || hrt[3 * i + 2] < 0 || hrt[3 * i + 2] >= E || hrt[3 * i + 1] < 0 ||
        hrt[3 * i + 1] >= R) {
      set_error("rnnl_miner_create: triple out of range");
      return RNNL_ERR_INVALID;
    }
  // out-edges grouped by source, in-edges grouped by target with sources ascending
  std::vector<int32_t> out_off(E + 1, 0), in_off(E + 1, 0);
  for (int64_t i = 0; i < n; ++i) {
    ++out_off[hrt[3 * i] + 1];
    ++in_off[hrt[3 * i + 2] + 1];
  }
  std::partial_sum(out_off.begin(), out_off.end(), out_off.begin());
  std::partial_sum(in_off.begin(), in_off.end(), in_off.begin());
  std::vector<int32_t> out_dst(n), out_rel(n), fill(out_off.begin(), out_off.end() - 1);
  std::vector<int64_t> by_t(n);
  for (int64_t i = 0; i < n; ++i) {
    const int32_t k = fill[hrt[3 * i]]++;
    out_dst[k] = hrt[3 * i + 2];
    out_rel[k] = hrt[3 * i + 1];
    by_t[i] = i;
  }
  std::stable_sort(by_t.begin(), by_t.end(), [&](int64_t a, int64_t b) {
    if (hrt[3 * a + 2] != hrt[3 * b + 2]) return hrt[3 * a + 2] < hrt[3 * b + 2];
    return hrt[3 * a] < hrt[3 * b];
  });
  std::vector<int32_t> in_src(n), in_rel(n), th(n), tr(n), tt(n);
  for (int64_t i = 0; i < n; ++i) {
    in_src[i] = hrt[3 * by_t[i]];
    in_rel[i] = hrt[3 * by_t[i] + 1];
    th[i] = hrt[3 * i];
    tr[i] = hrt[3 * i + 1];
    tt[i] = hrt[3 * i + 2];
  }
  // the out-edges once more, sorted by (relation, target) within a source (mine_learn.hip)
  std::vector<int32_t> so_rel(n), so_dst(n);
  {
    std::vector<std::pair<int32_t, int32_t>> tmp;
    for (int32_t e = 0; e < E; ++e) {
      tmp.clear();
      for (int32_t k = out_off[e]; k < out_off[e + 1]; ++k) tmp.emplace_back(out_rel[k], out_dst[k]);
      std::sort(tmp.begin(), tmp.end());
      for (size_t k = 0; k < tmp.size(); ++k) {
        so_rel[out_off[e] + k] = tmp[k].first;
        so_dst[out_off[e] + k] = tmp[k].second;
      }
    }
  }
  // and the in-edges once more, sorted by (relation, source) within a target (the head side of mine_ground.h)
  std::vector<int32_t> si_rel(n), si_src(n);
  {
    std::vector<std::pair<int32_t, int32_t>> tmp;
    for (int32_t e = 0; e < E; ++e) {
      tmp.clear();
      for (int32_t k = in_off[e]; k < in_off[e + 1]; ++k) tmp.emplace_back(in_rel[k], in_src[k]);
      std::sort(tmp.begin(), tmp.end());
      for (size_t k = 0; k < tmp.size(); ++k) {
        si_rel[in_off[e] + k] = tmp[k].first;
        si_src[in_off[e] + k] = tmp[k].second;
      }
    }
  }
  rnnl_miner_s *mm = new rnnl_miner_s;
  auto up =[&](const std::vector<int32_t> &v, const int32_t *&dst) -> int {
    void *p = nullptr;
    const size_t bytes = std::max<size_t>(4, v.size() * 4);
    if (hipMalloc(&p, bytes) != hipSuccess) return RNNL_ERR_NOMEM;
    mm->bufs.push_back(p);
    if (!v.empty() && hipMemcpy(p, v.data(), v.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return RNNL_ERR_HIP;
    dst = static_cast<const int32_t *>(p);
    return RNNL_OK;
  };
  mm->d.E = E;
  mm->d.R = R;
  mm->d.n = (int32_t)n;
  int rc = RNNL_OK;
  for (auto pr : {std::make_pair(&out_off, &mm->d.out_off), std::make_pair(&out_dst, &mm->d.out_dst),
                  std::make_pair(&out_rel, &mm->d.out_rel), std::make_pair(&in_off, &mm->d.in_off),
                  std::make_pair(&in_src, &mm->d.in_src), std::make_pair(&in_rel, &mm->d.in_rel),
                  std::make_pair(&th, &mm->d.th), std::make_pair(&tr, &mm->d.tr), std::make_pair(&tt, &mm->d.tt),
                  std::make_pair(&so_rel, &mm->l.so_rel), std::make_pair(&so_dst, &mm->l.so_dst),
                  std::make_pair(&si_rel, &mm->l.si_rel), std::make_pair(&si_src, &mm->l.si_src)})
    if (rc == RNNL_OK) rc = up(*pr.first, *pr.second);
  if (rc != RNNL_OK) {
    for (void *p : mm->bufs) (void)hipFree(p);
    delete mm;
    set_error("rnnl_miner_create: device allocation/copy failed");
    return rc;
  }
  *out = mm;
  return RNNL_OK;
}

int rnnl_miner_destroy(rnnl_miner m) {
  if (!m) return RNNL_OK;
  for (void *p : m->bufs) (void)hipFree(p);
  for (void *p : m->rule_bufs) (void)hipFree(p);
  delete m;
  return RNNL_OK;
}

int rnnl_rule_search(rnnl_miner m, int32_t max_length, uint64_t *table, int64_t table_cap, uint64_t *rules_out,
                     int64_t out_cap, uint64_t *counters, void *stream) {
  if (!m || max_length < 1 || max_length > 3 || !table || table_cap < 1024 || (table_cap & (table_cap - 1)) ||
      !rules_out || out_cap < 0 || !counters) {
    set_error("rnnl_rule_search: bad arguments (max_length 1..3, table_cap a power of two >= 1024)");
    return RNNL_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  RNNL_HIP_CHECK(hipMemsetAsync(table, 0xff, (size_t)table_cap * 8, st));
  RNNL_HIP_CHECK(hipMemsetAsync(counters, 0, 4 * 8, st));
  unsigned long long *flags = reinterpret_cast<unsigned long long *>(counters);
  if (m->d.n > 0) {
    const unsigned grid = (unsigned)std::min<int64_t>(m->d.n, 256 * 4);
    hipLaunchKernelGGL(mine_kernel, dim3(grid), dim3(MB), 0, st, m->d, (int)max_length,
                       reinterpret_cast<unsigned long long *>(table), table_cap, flags);
  }
  hipLaunchKernelGGL(compact_kernel, dim3(1024), dim3(256), 0, st, reinterpret_cast<const unsigned long long *>(table),
                     table_cap, reinterpret_cast<unsigned long long *>(rules_out), out_cap, flags);
  RNNL_HIP_CHECK(hipGetLastError());
  return RNNL_OK;
}

int rnnl_rule_key_bits(int32_t n_relations, int32_t max_length, int32_t *bits) {
  if (n_relations < 1 || max_length < 1 || max_length > 5 || !bits) {
    set_error("rnnl_rule_key_bits: bad arguments (n_relations >= 1, max_length 1..5)");
    return RNNL_ERR_INVALID;
  }
  int b = 1;
  while (b < 31 && (1 << b) < n_relations) ++b;
  if (3 + (max_length + 1) * b > 64) {
    const int fit = (64 - 3) / (max_length + 1);
    set_error("rule keys of max_length " + std::to_string(max_length) + " hold at most " +
              std::to_string(1 << fit) + " relations (3 + (max_length + 1) * bits <= 64), the graph has " +
              std::to_string(n_relations));
    return RNNL_ERR_INVALID;
  }
  *bits = b;
  return RNNL_OK;
}

int rnnl_rule_search_long(rnnl_miner m, int32_t max_length, int32_t suffix_cap, uint64_t *table, int64_t table_cap,
                          uint64_t *rules_out, int64_t out_cap, uint64_t *counters, void *stream) {
  if (!m || max_length < 1 || max_length > 5 || suffix_cap < 0 || suffix_cap > S2CAP || !table || table_cap < 1024 ||
      (table_cap & (table_cap - 1)) || !rules_out || out_cap < 0 || !counters) {
    set_error("rnnl_rule_search_long: bad arguments (max_length 1..5, suffix_cap 0..2048, table_cap a power of two "
              ">= 1024)");
    return RNNL_ERR_INVALID;
  }
  int32_t bits = 0;
  const int rc = rnnl_rule_key_bits(m->d.R, max_length, &bits);
  if (rc != RNNL_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  RNNL_HIP_CHECK(hipMemsetAsync(table, 0xff, (size_t)table_cap * 8, st));
  RNNL_HIP_CHECK(hipMemsetAsync(counters, 0, 4 * 8, st));
  unsigned long long *flags = reinterpret_cast<unsigned long long *>(counters);
  if (m->d.n > 0) {
    const unsigned grid = (unsigned)std::min<int64_t>(m->d.n, 256 * 4);
    LongKey f;
    f.bits = bits;
    f.slots = max_length;
    hipLaunchKernelGGL(mine_long_kernel, dim3(grid), dim3(MB), 0, st, m->d, (int)max_length, f,
                       (int)(suffix_cap ? suffix_cap : S2CAP), reinterpret_cast<unsigned long long *>(table),
                       table_cap, flags);
  }
  hipLaunchKernelGGL(compact_kernel, dim3(1024), dim3(256), 0, st, reinterpret_cast<const unsigned long long *>(table),
                     table_cap, reinterpret_cast<unsigned long long *>(rules_out), out_cap, flags);
  RNNL_HIP_CHECK(hipGetLastError());
  return RNNL_OK;
}

}  // extern "C"
