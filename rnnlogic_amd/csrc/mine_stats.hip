// Support, body size and PCA body size of rules: the three
// counts AMIE and AnyBURL report, exact, on the miner handle's train graph as
// it was given — no inverses, and unlike search, learn and evaluate no edge
// removed.  With D_b(x) the set of entities reachable from x along the body b
// (D(x) = {x} for the empty body) and T_r(x) the distinct tails of (x, r):
//
//   body(b)        = sum over x of |D_b(x)|
//   support(r, b)  = sum over x of |D_b(x) & T_r(x)|
//   pca_body(r, b) = sum over x with T_r(x) not empty of |D_b(x)|
//
// The unit of work is (distinct body, source entity): the walk and `body` are
// shared by every head asked for with that body (a CSR of heads per body, the
// heads ascending).  One 256-thread workgroup takes an item = (body, chunk of
// up to 256 consecutive sources), grid-stride; it first lists the chunk's
// sources that have an out-edge of the body's first relation, then each of its
// four waves walks sources of that list on its own: hop by hop over the
// (source, relation, target)-sorted out-edges, frontier list A -> list B, an
// entity entering B when an integer exchange on its visited stamp returns an
// older stamp.  The stamp advances with every hop, so nothing is cleared
// between hops or units, nothing can overflow, and after the last hop
// "stamp == current" is membership in D(x).  Then the lanes pass over x's own
// sorted out-edges once: every distinct (relation, target) whose relation is a
// head of the body adds 1 to that head's support if the target's stamp is
// current, and the first edge of each such relation adds |D(x)| to its
// pca_body.  The sums of an item are kept in LDS (u64 integer adds) and leave
// it as one global integer add per (item, head): exact, order-free, bitwise
// repeatable.  No floating point.
//
// Up to STATS_LDS_E entities the per-wave arrays (stamps + two lists, 12 bytes
// per entity and wave) are LDS, above that a global scratch in the caller's
// workspace.  Prefix sharing between bodies is left out: every body is walked
// from its first relation.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "internal.h"
#include "mine_common.h"  // the counter slots and lower_bound_i

namespace rnnl {

constexpr int SB = 256;             // threads per workgroup = the most sources of one item
constexpr int SW = SB / 64;         // waves: sources walked at once
constexpr int STATS_LDS_E = 1024;   // 48 KiB of dynamic LDS + 3.3 KiB static: inside the 64 KiB of a workgroup
constexpr size_t STATS_PER_E = SW * 12;  // per wave: stamps (u32), list A, list B (int)
constexpr int STATS_HEADS = 128;    // heads of a body summed in LDS; further ones add to global memory directly
constexpr int STATS_COOP = 16;      // frontiers below this: the wave walks one entity's run together
constexpr size_t STATS_SCRATCH = 256u << 20;
constexpr int STATS_MAX_BLOCKS = 2048;
constexpr unsigned STAMP_ROOM = RULE_STRIDE + 1;  // stamps one unit takes at the most

struct StatsArgs {
  const int32_t *body_len, *body_rel, *head_off, *head_rel;  // n_bodies, n_bodies x RULE_STRIDE, n_bodies + 1, slots
  int64_t n_items;
  int32_t n_chunks, chunk;
  unsigned long long *body_cnt, *support, *pca;  // n_bodies, slots, slots
  unsigned char *scratch;
  unsigned stamp0;
  unsigned long long *flags;
};

namespace {

// what one wave wrote becomes visible to its other lanes: the stores complete, nothing moves across
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// The stamps are only touched by atomics (global ones execute in L2; the loads go there too).
template <bool SMALL>
__device__ __forceinline__ unsigned stamp_swap(unsigned *p, unsigned s) {
  return SMALL ? __hip_atomic_exchange(p, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
               : __hip_atomic_exchange(p, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool SMALL>
__device__ __forceinline__ unsigned stamp_load(unsigned *p) {
  return SMALL ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
               : __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

template <bool SMALL>
__global__ __launch_bounds__(SB) void stats_kernel(MinerDev d, MinerLearnDev l, StatsArgs a) {
  extern __shared__ unsigned stats_smem[];
  __shared__ unsigned long long s_sup[STATS_HEADS], s_pca[STATS_HEADS], s_body;
  __shared__ int s_src[SB], s_nsrc, s_cnt[SW];
  const int E = d.E, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  unsigned *base = SMALL ? stats_smem
                         : reinterpret_cast<unsigned *>(a.scratch + (size_t)blockIdx.x * STATS_PER_E * (size_t)E);
  unsigned *stamp = base + (size_t)wid * 3 * (size_t)E;  // wave w: stamps, list A, list B (E words each)
  int *l0 = reinterpret_cast<int *>(stamp + E), *l1 = l0 + E;
  for (int i = lane; i < E; i += 64) stamp[i] = 0u;  // LDS starts undefined, the scratch holds an earlier call's stamps
  unsigned s = a.stamp0;
  for (int i = tid; i < STATS_HEADS; i += SB) {
    s_sup[i] = 0ull;
    s_pca[i] = 0ull;
  }
  if (tid == 0) s_body = 0ull;
  __syncthreads();
#pragma unroll 1
  for (int64_t item = blockIdx.x; item < a.n_items; item += gridDim.x) {
    const int b = (int)(item / a.n_chunks);
    const int c0 = (int)(item - (int64_t)b * a.n_chunks) * a.chunk;
    const int len = a.body_len[b];
    const int hb = a.head_off[b], nh = a.head_off[b + 1] - hb;
    int rels[RULE_STRIDE];
#pragma unroll
    for (int k = 0; k < RULE_STRIDE; ++k) rels[k] = k < len ? a.body_rel[RULE_STRIDE * b + k] : 0;
    if (tid == 0) s_nsrc = 0;
    __syncthreads();
    {  // the chunk's sources that can start the body at all
      const int x = c0 + tid;
      if (tid < a.chunk && x < E) {
        const int eb = d.out_off[x], en = d.out_off[x + 1];
        bool go = len == 0;
        if (!go) {
          const int k = lower_bound_i(l.so_rel, eb, en, rels[0]);
          go = k < en && l.so_rel[k] == rels[0];
        }
        if (go) s_src[atomicAdd(&s_nsrc, 1)] = x;
      }
    }
    __syncthreads();
    const int nsrc = s_nsrc;
    unsigned long long nsum = 0ull;  // |D(x)| over this wave's sources
#pragma unroll 1
    for (int si = wid; si < nsrc; si += SW) {
      const int x = s_src[si];
      if (s > 0xffffffffu - STAMP_ROOM) {  // the stamps would wrap inside this unit: start over
        wave_sync();
        for (int i = lane; i < E; i += 64) stamp_swap<SMALL>(&stamp[i], 0u);
        s = 0u;
        wave_sync();
      }
      ++s;
      int *la = l0, *lb = l1;
      if (lane == 0) {
        la[0] = x;
        stamp_swap<SMALL>(&stamp[x], s);
      }
      int na = 1;
#pragma unroll 1
      for (int k = 0; k < len && na > 0; ++k) {
        const int rel = rels[k];
        ++s;
        if (lane == 0) s_cnt[wid] = 0;
        wave_sync();
        if (na < STATS_COOP) {  // few entities (the first hop always): the lanes share each one's run
          for (int i = 0; i < na; ++i) {
            const int e = la[i];
            const int eb = d.out_off[e], en = d.out_off[e + 1];
            const int lo = lower_bound_i(l.so_rel, eb, en, rel), hi = lower_bound_i(l.so_rel, lo, en, rel + 1);
            for (int q = lo + lane; q < hi; q += 64) {
              const int y = l.so_dst[q];
              if (stamp_swap<SMALL>(&stamp[y], s) != s) {
                const int pos = atomicAdd(&s_cnt[wid], 1);
                if (pos < E)
                  lb[pos] = y;
                else
                  atomicOr(&a.flags[CTR_INTERNAL], 1ull);
              }
            }
          }
        } else {
          for (int i = lane; i < na; i += 64) {
            const int e = la[i];
            const int en = d.out_off[e + 1];
            for (int q = lower_bound_i(l.so_rel, d.out_off[e], en, rel); q < en && l.so_rel[q] == rel; ++q) {
              const int y = l.so_dst[q];
              if (stamp_swap<SMALL>(&stamp[y], s) != s) {
                const int pos = atomicAdd(&s_cnt[wid], 1);
                if (pos < E)
                  lb[pos] = y;
                else
                  atomicOr(&a.flags[CTR_INTERNAL], 1ull);
              }
            }
          }
        }
        wave_sync();
        na = min(__builtin_amdgcn_readfirstlane(__hip_atomic_load(&s_cnt[wid], __ATOMIC_RELAXED,
                                                                  __HIP_MEMORY_SCOPE_WORKGROUP)), E);
        int *tl = la;
        la = lb;
        lb = tl;
      }
      if (na == 0) continue;  // the body reaches nothing from x
      wave_sync();
      nsum += (unsigned long long)na;
      if (nh > 0) {
        // x's own sorted out-edges: distinct (relation, target) pairs whose relation is a head of the body
        const int eb = d.out_off[x], en = d.out_off[x + 1];
        for (int q = eb + lane; q < en; q += 64) {
          const int rel = l.so_rel[q], y = l.so_dst[q];
          const bool first = q == eb || l.so_rel[q - 1] != rel;
          if (!first && l.so_dst[q - 1] == y) continue;  // a duplicate train edge
          const int p = lower_bound_i(a.head_rel, hb, hb + nh, rel);
          if (p == hb + nh || a.head_rel[p] != rel) continue;
          const bool hit = stamp_load<SMALL>(&stamp[y]) == s;
          const int slot = p - hb;
          if (slot < STATS_HEADS) {
            if (first) atomicAdd(&s_pca[slot], (unsigned long long)na);
            if (hit) atomicAdd(&s_sup[slot], 1ull);
          } else {
            if (first) atomicAdd(&a.pca[p], (unsigned long long)na);
            if (hit) atomicAdd(&a.support[p], 1ull);
          }
        }
      }
    }
    if (lane == 0 && nsum) atomicAdd(&s_body, nsum);
    __syncthreads();
    for (int i = tid; i < min(nh, STATS_HEADS); i += SB) {  // one add per (item, head)
      const unsigned long long u = s_sup[i], v = s_pca[i];
      if (u) atomicAdd(&a.support[hb + i], u);
      if (v) atomicAdd(&a.pca[hb + i], v);
      s_sup[i] = 0ull;
      s_pca[i] = 0ull;
    }
    if (tid == 0) {
      if (s_body) atomicAdd(&a.body_cnt[b], s_body);
      s_body = 0ull;
    }
    __syncthreads();
  }
}

}  // namespace rnnl

using namespace rnnl;

namespace {

struct StatsPlan {
  size_t arrays = 0, total = 0;  // bytes of the rule arrays (256-aligned), of the whole workspace
  int32_t blocks = 0, n_chunks = 0, chunk = 0;
  int64_t n_items = 0;
};

StatsPlan stats_plan(int32_t E, int64_t n_bodies, int64_t n_slots, int32_t max_blocks) {
  StatsPlan p;
  p.arrays = ((size_t)(n_bodies * (2 + RULE_STRIDE) + 1 + n_slots) * 4 + 255) & ~(size_t)255;
  // enough items to fill the grid where the bodies are few: chunks of 16..256 sources
  const int64_t per_body = std::max<int64_t>(1, (2 * STATS_MAX_BLOCKS + n_bodies - 1) / std::max<int64_t>(n_bodies, 1));
  p.chunk = (int32_t)std::min<int64_t>(SB, std::max<int64_t>(16, (E + per_body - 1) / per_body));
  p.n_chunks = (E + p.chunk - 1) / p.chunk;
  p.n_items = n_bodies * p.n_chunks;
  int64_t blocks = STATS_MAX_BLOCKS;
  if (E > STATS_LDS_E)
    blocks = std::max<int64_t>(16, std::min<int64_t>(blocks, (int64_t)(STATS_SCRATCH / (STATS_PER_E * (size_t)E))));
  if (max_blocks > 0) blocks = std::min<int64_t>(blocks, max_blocks);
  p.blocks = (int32_t)std::max<int64_t>(1, std::min<int64_t>(blocks, p.n_items));
  p.total = p.arrays + (E > STATS_LDS_E ? (size_t)p.blocks * STATS_PER_E * (size_t)E : 0);
  return p;
}

}  // namespace

extern "C" {

int rnnl_miner_rule_stats_scratch(rnnl_miner m, int64_t n_bodies, int64_t n_slots, int32_t max_blocks,
                                  size_t *bytes) {
  if (!m || !bytes || n_bodies < 0 || n_slots < 0 || max_blocks < 0 || n_bodies > INT32_MAX || n_slots > INT32_MAX) {
    set_error("rnnl_miner_rule_stats_scratch: bad arguments");
    return RNNL_ERR_INVALID;
  }
  *bytes = std::max<size_t>(256, stats_plan(m->d.E, n_bodies, n_slots, max_blocks).total);
  return RNNL_OK;
}

int rnnl_miner_rule_stats(rnnl_miner m, int64_t n_bodies, const int32_t *body_len, const int32_t *body_rel,
                          const int32_t *head_off, const int32_t *head_rel, int32_t max_blocks, uint32_t first_stamp,
                          void *work, size_t work_bytes, uint64_t *out, uint64_t *counters, void *stream) {
  const std::string who = "rnnl_miner_rule_stats";
  if (!m || n_bodies < 0 || n_bodies > INT32_MAX || !head_off || head_off[0] != 0 || max_blocks < 0 || !work ||
      !out || !counters || (n_bodies > 0 && (!body_len || !body_rel))) {
    set_error(who + ": bad arguments");
    return RNNL_ERR_INVALID;
  }
  const int R = m->d.R, E = m->d.E;
  for (int64_t b = 0; b < n_bodies; ++b) {
    if (body_len[b] < 0 || body_len[b] > RULE_STRIDE) {
      set_error(who + ": body length must be 0.." + std::to_string(RULE_STRIDE));
      return RNNL_ERR_INVALID;
    }
    for (int k = 0; k < body_len[b]; ++k)
      if (body_rel[RULE_STRIDE * b + k] < 0 || body_rel[RULE_STRIDE * b + k] >= R) {
        set_error(who + ": body relation out of range");
        return RNNL_ERR_INVALID;
      }
    if (head_off[b + 1] < head_off[b]) {
      set_error(who + ": head_off must not decrease");
      return RNNL_ERR_INVALID;
    }
  }
  const int64_t n_slots = head_off[n_bodies];
  if (n_slots > 0 && !head_rel) {
    set_error(who + ": head_rel missing");
    return RNNL_ERR_INVALID;
  }
  for (int64_t b = 0; b < n_bodies; ++b)
    for (int32_t i = head_off[b]; i < head_off[b + 1]; ++i)
      if (head_rel[i] < 0 || head_rel[i] >= R || (i > head_off[b] && head_rel[i - 1] >= head_rel[i])) {
        set_error(who + ": the heads of a body must be relations in range, ascending and distinct");
        return RNNL_ERR_INVALID;
      }
  const StatsPlan p = stats_plan(E, n_bodies, n_slots, max_blocks);
  if (work_bytes < p.total) {
    set_error(who + ": the workspace is smaller than rnnl_miner_rule_stats_scratch says");
    return RNNL_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  RNNL_HIP_CHECK(hipMemsetAsync(counters, 0, 4 * 8, st));
  RNNL_HIP_CHECK(hipMemsetAsync(out, 0, std::max<size_t>(8, (size_t)(n_bodies + 2 * n_slots) * 8), st));
  if (n_bodies == 0 || E == 0) return RNNL_OK;
  int32_t *w = static_cast<int32_t *>(work);
  int32_t *d_len = w, *d_rel = d_len + n_bodies, *d_off = d_rel + RULE_STRIDE * n_bodies;
  int32_t *d_head = d_off + n_bodies + 1;
  RNNL_HIP_CHECK(hipMemcpyAsync(d_len, body_len, (size_t)n_bodies * 4, hipMemcpyHostToDevice, st));
  RNNL_HIP_CHECK(hipMemcpyAsync(d_rel, body_rel, (size_t)n_bodies * 4 * RULE_STRIDE, hipMemcpyHostToDevice, st));
  RNNL_HIP_CHECK(hipMemcpyAsync(d_off, head_off, (size_t)(n_bodies + 1) * 4, hipMemcpyHostToDevice, st));
  if (n_slots > 0) RNNL_HIP_CHECK(hipMemcpyAsync(d_head, head_rel, (size_t)n_slots * 4, hipMemcpyHostToDevice, st));
  StatsArgs a = {};
  a.body_len = d_len;
  a.body_rel = d_rel;
  a.head_off = d_off;
  a.head_rel = d_head;
  a.n_items = p.n_items;
  a.n_chunks = p.n_chunks;
  a.chunk = p.chunk;
  a.body_cnt = reinterpret_cast<unsigned long long *>(out);
  a.support = a.body_cnt + n_bodies;
  a.pca = a.support + n_slots;
  a.scratch = static_cast<unsigned char *>(work) + p.arrays;
  a.stamp0 = first_stamp;
  a.flags = reinterpret_cast<unsigned long long *>(counters);
  if (E <= STATS_LDS_E)
    hipLaunchKernelGGL(stats_kernel<true>, dim3(p.blocks), dim3(SB), STATS_PER_E * (size_t)E, st, m->d, m->l, a);
  else
    hipLaunchKernelGGL(stats_kernel<false>, dim3(p.blocks), dim3(SB), 0, st, m->d, m->l, a);
  RNNL_HIP_CHECK(hipGetLastError());
  return RNNL_OK;
}

}  // extern "C"
