// The grounding paths behind a listed answer: for a query
// (h, r, t) of the open forms of §3.16 / §3.17, a slot entity e and a rule
// r <- b_1..b_L of relation r's list, the first P paths
// x_0 -b_1-> x_1 ... -b_L-> x_L from h to e (tail side: x_0 = h, x_L = e) or
// from e to t (head side: x_0 = e, x_L = t), every copy of the query's own edge
// (h, r, t) skipped on every hop as ground_hop skips it; an open query skips
// nothing.  A train triple that is in the graph twice is two edges: a path
// through it is listed twice, in adjacent places.  The number of paths is the
// count rnnl_miner_explain reports under the sum.
//
// Order: by the entities read from e back toward the anchor.  Tail side:
// x_{L-1} ascending, then x_{L-2}, ...; head side: x_1, then x_2, ....  With
// that order one grounding from the anchor per rule serves every slot, and a
// path follows from its number alone.
//
// rnnl_miner_paths_side.  paths_kernel<SMALL, HEAD>: one 256-thread workgroup
// per query, grid-stride, in the regimes of query_launch (mine_ground.h): the
// arrays in LDS up to EVAL_LDS_E entities, above that in a per-workgroup scratch
// of the handle (path_scratch, zeroed once, left zeroed by every query).  Per
// distinct rule that the query's (slot, entry) pairs name, in ascending index
// (the smallest index above the last one, a minimum over the <= 4,096 entries):
//
// 1. The body is grounded from the anchor with ground_hop<HEAD, true>
//    (mine_common.h), all levels kept: F_0 (1 at the anchor) .. F_L, dense u64
//    path counts, and per level the list of the entities first touched there.
//    The four waves share one hop: each takes a quarter of the frontier list,
//    the next level and its list counter are common (integer atomics).
// 2. One thread per (slot, entry, p) of that rule: count = F_L[e]; path number
//    p < min(P, count) stands at x = e with rank p and, for level L down to 1,
//    walks x's edges of the hop's relation on the side facing the anchor (tail
//    side: the in-edges, sorted by (relation, source); head side: the out-edges,
//    sorted by (relation, target)), from lower_bound_i, the query's own edge
//    skipped.  A run of m equal far ends y (a triple that is there m times)
//    stands for m * F_{level-1}[y] paths, each path below y m times in a row:
//    rank < m * F[y] descends to y with rank / m, otherwise rank -= m * F[y].
//    Falling off the run is CTR_INTERNAL.
// 3. The levels are cleared along their lists; a final count past 32 bits sets
//    CTR_RANGE there, a count past 32 bits carried over an edge sets it in
//    ground_hop: the counter comes out as from explain_kernel for these rules.
//
// Every output element is written by one thread: the entries that list nothing
// (an unused or invalid slot or rule, a rule without a body) before the rules,
// every other entry when its rule is grounded.  No float, no atomics on the
// outputs: the result is a function of the inputs alone.  The handle's
// aggregation is not looked at: paths are always counted.
//
// LDS, EVAL_LDS_E = 512 entities: 6 levels x (u64 + int) x 512 = 36 KiB of the
// 52 KiB query_launch asks for.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "internal.h"
#include "mine_ground.h"

namespace rnnl {

constexpr int PATH_LEN = RNNL_MINER_PATH_LEN;  // entities of the longest path
static_assert(PATH_LEN == RULE_STRIDE + 1, "a path has one entity more than the longest body has relations");
constexpr size_t PATH_PER_E = PATH_LEN * (8 + 4);  // per level the counts (u64) and the list (int)
static_assert(PATH_PER_E <= EVAL_PER_E, "the LDS query_launch asks for holds the levels");

struct PathArgs {
  const int32_t *queries;
  int64_t n;
  const int32_t *index, *rule;
  int32_t m, c, P;
  int32_t *listed;
  long long *count;
  int32_t *path;
  unsigned char *scratch;  // query_launch's (the evaluation's: not used here)
  unsigned char *levels;   // the handle's path_scratch, one block per workgroup
  unsigned long long *flags;
};

template <bool SMALL, bool HEAD>
__global__ __launch_bounds__(EB) void paths_kernel(MinerDev d, MinerLearnDev l, PathArgs a) {
  extern __shared__ unsigned long long path_smem[];
  __shared__ int s_nl[PATH_LEN];  // the entities of each level's list
  __shared__ int s_min[EW];
  const int E = d.E, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  unsigned char *base = SMALL ? reinterpret_cast<unsigned char *>(path_smem)
                              : a.levels + (size_t)blockIdx.x * PATH_PER_E * (size_t)E;
  unsigned long long *F = reinterpret_cast<unsigned long long *>(base);  // level k: F + k * E
  int *lst = reinterpret_cast<int *>(F + (size_t)PATH_LEN * E);          // level k: lst + k * E
  // the edges of an entity on the side facing the anchor, sorted by (relation, far end)
  const int32_t *u_off = HEAD ? d.out_off : d.in_off;
  const int32_t *u_rel = HEAD ? l.so_rel : l.si_rel;
  const int32_t *u_end = HEAD ? l.so_dst : l.si_src;
  if (SMALL)
    for (int i = tid; i < PATH_LEN * E; i += EB) F[i] = 0ull;
  __syncthreads();
  const int items = a.m * a.c;
#pragma unroll 1
  for (int64_t qi = blockIdx.x; qi < a.n; qi += gridDim.x) {
    const int h = a.queries[3 * qi], r = a.queries[3 * qi + 1], t = a.queries[3 * qi + 2];
    const int anc = HEAD ? t : h, ans = HEAD ? h : t;
    const bool bad = (unsigned)anc >= (unsigned)E || (unsigned)r >= (unsigned)d.R || ans < -1 || ans >= E;
    const int rb = bad ? 0 : l.rule_off[r], nr = bad ? 0 : l.rule_off[r + 1] - rb;
    const int32_t *q_index = a.index + qi * a.m, *q_rule = a.rule + qi * items;
    // entry `it` lists paths: its entity and its rule are in range and the rule has a body
    auto lists = [&](int it, int &ent, int &k) {
      ent = q_index[it / a.c];
      k = q_rule[it];
      return (unsigned)ent < (unsigned)E && (unsigned)k < (unsigned)nr && l.rule_len[rb + k] > 0;
    };
    // the entries that list nothing
    bool invalid = bad;
    for (int it = tid; it < items; it += EB) {
      int ent, k;
      if (lists(it, ent, k)) continue;
      invalid |= !bad && (ent < -1 || ent >= E || k < -1 || k >= nr);
      a.count[qi * items + it] = 0;
      a.listed[qi * items + it] = 0;
      int32_t *rows = a.path + (qi * items + it) * (int64_t)(a.P * PATH_LEN);
      for (int j = 0; j < a.P * PATH_LEN; ++j) rows[j] = -1;
    }
    if (invalid) atomicOr(&a.flags[CTR_INVALID], 1ull);
    bool wide = false;
    int cur = -1;  // the rules up to here are done
#pragma unroll 1
    while (true) {
      int mn = 0x7fffffff;
      for (int it = tid; it < items; it += EB) {
        int ent, k;
        if (lists(it, ent, k) && k > cur) mn = min(mn, k);
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) mn = min(mn, __shfl_xor(mn, o, 64));
      if (lane == 0) s_min[wid] = mn;
      if (tid < PATH_LEN) s_nl[tid] = tid == 0;  // level 0: the anchor alone
      __syncthreads();
#pragma unroll
      for (int w = 0; w < EW; ++w) mn = min(mn, s_min[w]);
      if (mn == 0x7fffffff) break;  // (the same for every thread)
      const int rule = rb + mn, len = l.rule_len[rule];
      const int32_t *body = l.rule_body + RULE_STRIDE * rule;
      if (tid == 0) {
        lst[0] = anc;
        F[anc] = 1ull;
      }
      // 1. level k -> k + 1, the waves on a quarter of the frontier each
      for (int k = 0; k < len; ++k) {
        __syncthreads();
        const int na = s_nl[k], per = (na + EW - 1) / EW, b0 = min(na, wid * per);
        GroundScratch s(base, 0, E);
        s.ca = F + (size_t)k * E;
        s.cb = s.ca + E;
        s.la = lst + (size_t)k * E + b0;
        s.lb = lst + (size_t)(k + 1) * E;
        ground_hop<HEAD, true>(d, l, s, min(per, na - b0), lane, body[HEAD ? len - 1 - k : k], h, r, t, &s_nl[k + 1],
                               wide);
      }
      __syncthreads();
      // 2. one thread per (entry of this rule, p)
      for (int w = tid; w < items * a.P; w += EB) {
        const int it = w / a.P, p = w - it * a.P;
        int ent, k;
        if (!lists(it, ent, k) || k != mn) continue;
        const unsigned long long cnt = ld_u64(&F[(size_t)len * E + ent]);
        const int nl = (int)min((unsigned long long)a.P, cnt);
        if (p == 0) {
          a.count[qi * items + it] = (long long)cnt;
          a.listed[qi * items + it] = nl;
        }
        int32_t *row = a.path + ((qi * items + it) * (int64_t)a.P + p) * PATH_LEN;
#pragma unroll
        for (int j = 0; j < PATH_LEN; ++j) row[j] = -1;
        if (p >= nl) continue;
        int x = ent;
        unsigned rank = (unsigned)p;  // < P, and it only falls
        row[HEAD ? 0 : len] = x;
        for (int lev = len; lev >= 1; --lev) {
          const int rel = body[HEAD ? len - lev : lev - 1];
          unsigned long long *Fp = F + (size_t)(lev - 1) * E;
          const int en = u_off[x + 1];
          int b = lower_bound_i(u_rel, u_off[x], en, rel), y = -1;
          bool found = false;
          while (b < en && u_rel[b] == rel) {
            y = u_end[b];
            unsigned mult = 0;  // the copies of this edge
            for (; b < en && u_rel[b] == rel && u_end[b] == y; ++b) ++mult;
            if (rel == r && (HEAD ? (x == h && y == t) : (y == h && x == t))) continue;
            const unsigned long long grp = ld_u64(&Fp[y]) * mult;
            if (rank < grp) {
              rank /= mult;
              found = true;
              break;
            }
            rank -= (unsigned)grp;
          }
          if (!found) {
            atomicOr(&a.flags[CTR_INTERNAL], 1ull);
            break;
          }
          x = y;
          row[HEAD ? len - lev + 1 : lev - 1] = x;
        }
      }
      __syncthreads();
      // 3. the levels back to zero, along their lists
      for (int k = 0; k <= len; ++k) {
        unsigned long long *Fk = F + (size_t)k * E;
        const int nk = s_nl[k];
        for (int i = tid; i < nk; i += EB) {
          const int x = lst[(size_t)k * E + i];
          if (k == len) wide |= ld_u64(&Fk[x]) > 0xffffffffull;
          Fk[x] = 0ull;
        }
      }
      __syncthreads();
      cur = mn;
    }
    if (wide) atomicOr(&a.flags[CTR_RANGE], 1ull);
    __syncthreads();  // s_min and s_nl are the next query's
  }
}

// The per-workgroup levels of graphs past EVAL_LDS_E entities, kept in the
// handle beside the evaluation's scratch and cut for its workgroups: zeroed
// once, every query leaves it zeroed.
static int path_scratch_ensure(rnnl_miner m) {
  if (m->path_scratch) return RNNL_OK;
  const size_t bytes = (size_t)m->eval_blocks * PATH_PER_E * (size_t)m->d.E;
  void *p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess) {
    set_error("rnnl_miner_paths: device allocation failed");
    return RNNL_ERR_NOMEM;
  }
  m->bufs.push_back(p);
  RNNL_HIP_CHECK(hipMemset(p, 0, bytes));
  RNNL_HIP_CHECK(hipDeviceSynchronize());
  m->path_scratch = static_cast<unsigned char *>(p);
  return RNNL_OK;
}

}  // namespace rnnl

using namespace rnnl;

extern "C" {

int rnnl_miner_paths_side(rnnl_miner m, int32_t side, const int32_t *queries, int64_t n, const int32_t *index,
                          int32_t n_slots, const int32_t *rule, int32_t c, int32_t max_paths, int32_t *listed,
                          int64_t *count, int32_t *path, uint64_t *counters, void *stream) {
  if (!check_side("rnnl_miner_paths", side)) return RNNL_ERR_INVALID;
  if (n_slots < 1 || n_slots > RNNL_MINER_TOPK_MAX) {
    set_error("rnnl_miner_paths: m (the slots per query) must be 1.." + std::to_string(RNNL_MINER_TOPK_MAX));
    return RNNL_ERR_INVALID;
  }
  if (c < 1 || c > RNNL_MINER_EXPLAIN_MAX) {
    set_error("rnnl_miner_paths: c (the rules per slot) must be 1.." + std::to_string(RNNL_MINER_EXPLAIN_MAX));
    return RNNL_ERR_INVALID;
  }
  if (max_paths < 1 || max_paths > RNNL_MINER_PATHS_MAX) {
    set_error("rnnl_miner_paths: max_paths (the paths per rule) must be 1.." + std::to_string(RNNL_MINER_PATHS_MAX));
    return RNNL_ERR_INVALID;
  }
  if (!m || !m->l.rule_off) {
    set_error("rnnl_miner_paths: no handle, or no rules (set the rules first)");
    return RNNL_ERR_INVALID;
  }
  if (n < 0 || (n > 0 && (!queries || !index || !rule || !listed || !count || !path)) || !counters) {
    set_error("rnnl_miner_paths: bad arguments (n >= 0, no null array)");
    return RNNL_ERR_INVALID;
  }
  const int64_t per_query = (int64_t)n_slots * c * max_paths * RNNL_MINER_PATH_LEN;  // < 2^25
  if (n > ((int64_t)0x7fffffff) / per_query) {
    set_error("rnnl_miner_paths: path would have 2^31 elements or more (cut the queries into smaller calls)");
    return RNNL_ERR_INVALID;
  }
  PathArgs a = {};
  a.queries = queries;
  a.n = n;
  a.index = index;
  a.rule = rule;
  a.m = n_slots;
  a.c = c;
  a.P = max_paths;
  a.listed = listed;
  a.count = reinterpret_cast<long long *>(count);
  a.path = path;
  return query_launch(
      m, "rnnl_miner_paths", side, n, 0, a, counters, stream,
      [](auto small, auto head, auto) { return paths_kernel<decltype(small)::value, decltype(head)::value>; },
      [&]() {
        const int rc = path_scratch_ensure(m);
        a.levels = m->path_scratch;
        return rc;
      });
}

}  // extern "C"
