// The grounding paths behind a predicted tail: rnnl_paths_rows.
// For row i = (all_h[i], all_r[i]) with optionally its own edge edges_to_remove[i],
// a slot entity e and a rule all_r[i] <- b_1..b_L named by its global id, the
// exact number of paths x_0 -b_1-> x_1 ... -b_L-> x_L from x_0 = h to x_L = e and
// the first max_paths of them.  The contract is the header's; what follows is how.
//
// Order: by the entities read from e back toward h: x_{L-1} ascending, then
// x_{L-2}, ... (the miner's tail-side order).  That is the order of
// GraphDev's in-edge view (the edges into an entity sorted by (relation, source)),
// so with the path counts of every level kept, path number p follows from p alone
// and one grounding from h per rule body serves every slot that names it.
//
// paths_rows_kernel<SMALL>: one 256-thread workgroup per row, grid-stride.  Six
// dense u64 count levels F_0..F_5 and the six lists of the entities first touched
// at each level, 72 B per entity: in LDS up to PATHS_LDS_E entities (SMALL), above
// that in the caller's scratch, one block per workgroup.  The kernel zeroes its
// levels when it starts and every body leaves them zeroed, so the scratch may
// arrive in any state and two callers never share one.
//
// Per distinct trie node that the row's (slot, entry) pairs name, in ascending
// node id (duplicate rules end at one node and share the grounding; the smallest
// node above the last one is a minimum over the entries):
//
// 1. Ground.  The body is read off the trie (node_rel along node_parent).  F_0 is
//    1 at h; hop k expands level k's list over the out-edges of relation b_{k+1}
//    (the compact per-vertex view of GraphDev) into level k + 1 with integer
//    atomics, an entity first touched appended to that level's list.  The four
//    waves take a quarter of the list each.  On hops of relation all_r[i] one
//    edge from the removed edge's source to its target is left out: the removed
//    edge (copies of one triple are interchangeable, so leaving out the first one
//    met gives the counts and the paths of leaving out that id).  A sum that
//    carries out of 64 bits sets CTR_RANGE.
// 2. Unrank, one thread per (slot, entry, p) of that node.  count = F_L[e].
//    Path p < min(max_paths, count) stands at x = e with rank p and, for level L
//    down to 1, walks x's in-edges of the hop's relation from lower_bound_i.  A
//    run of equal sources y with mult edges (the removed edge id not counted)
//    stands for mult * F_{level-1}[y] paths, every path below y mult times in a
//    row: rank below that descends to y with rank / mult, otherwise the run's
//    paths are taken off the rank.  Falling off the end is CTR_INTERNAL.
// 3. Clear.  Every level back to zero along its list: no sweep of |E|.
//
// Every output element is written by one thread (the entries that list nothing
// before the nodes, every other entry when its node is grounded); no float and no
// atomics on the outputs: the result is a function of the inputs alone.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "internal.h"
#include "mine_common.h"

namespace rnnl {

constexpr int PB = 256, PW = PB / 64;
constexpr int PATH_LEN = RNNL_PATH_LEN;       // entities of the longest path
constexpr int PATH_BODY = PATH_LEN - 1;       // relations of the longest body
constexpr int PATHS_RULES_MAX = 16;           // c: the rules named per slot
constexpr int PATHS_LDS_E = 512;              // entities up to which the levels live in LDS
constexpr int PATHS_BLOCKS = 128;             // workgroups of the scratch regime
constexpr int PATHS_GRID_LDS = 1024;          // workgroups of the LDS regime (36 KiB each: four per CU)
constexpr size_t PATHS_PER_E = PATH_LEN * (8 + 4);  // per level the counts (u64) and the list (int)
constexpr size_t PATHS_CTRL = 128;            // the control words in front of the LDS levels (keeps them 16-B aligned)

struct PathRowsArgs {
  const int64_t *all_h, *all_r, *etr;
  int32_t n, m, c, P;
  const int32_t *entity, *rule;
  int32_t *listed;
  long long *count;
  int32_t *path;
  unsigned char *scratch;
  unsigned long long *flags;
};

template <bool SMALL>
__global__ __launch_bounds__(PB) void paths_rows_kernel(GraphDev g, RulesDev rl, PathRowsArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char paths_smem[];
  int *s_nl = reinterpret_cast<int *>(paths_smem);  // [PATH_LEN] the entities of each level's list
  int *s_min = s_nl + 8;                            // [PW]
  int *s_body = s_nl + 16;                          // [PATH_BODY]
  const int E = g.E, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  unsigned char *base = SMALL ? paths_smem + PATHS_CTRL : a.scratch + (size_t)blockIdx.x * PATHS_PER_E * (size_t)E;
  unsigned long long *F = reinterpret_cast<unsigned long long *>(base);  // level k: F + k * E
  int *lst = reinterpret_cast<int *>(F + (size_t)PATH_LEN * E);          // level k: lst + k * E
  for (int i = tid; i < PATH_LEN * E; i += PB) F[i] = 0ull;
  __syncthreads();
  const int items = a.m * a.c;
#pragma unroll 1
  for (int qi = blockIdx.x; qi < a.n; qi += gridDim.x) {
    const long long h64 = a.all_h[qi], r64 = a.all_r[qi];
    bool bad = h64 < 0 || h64 >= E || r64 < 0 || r64 >= g.R;
    const int h = bad ? 0 : (int)h64, r = bad ? 0 : (int)r64;
    int rm_src = -1, rm_dst = -1, rm_id = -1;  // the row's own edge: relation r, relation-local id rm_id
    if (!bad && a.etr && a.etr[qi] >= 0) {
      const int eb = g.edge_base[r];
      if (a.etr[qi] >= g.edge_base[r + 1] - eb) {
        bad = true;
      } else {
        rm_id = (int)a.etr[qi];
        rm_src = g.edge_src[eb + rm_id];
        rm_dst = g.edge_dst[eb + rm_id];
      }
    }
    const int root = bad ? -1 : rl.head_root[r], root_end = root < 0 ? -1 : root + rl.head_nodes[r];
    const int32_t *q_ent = a.entity + (int64_t)qi * a.m, *q_rule = a.rule + (int64_t)qi * items;
    // entry `it` lists paths: its entity and rule id are in range, the rule is one of relation r with a body of
    // 1..PATH_BODY relations; node = where that body ends in r's trie
    auto lists = [&](int it, int &ent, int &k, int &node) {
      ent = q_ent[it / a.c];
      k = q_rule[it];
      node = -1;
      if ((unsigned)ent >= (unsigned)E || (unsigned)k >= (unsigned)rl.n_rules) return false;
      const int nd = rl.rule_node[k];
      if (nd <= root || nd >= root_end) return false;  // (root itself: an empty body)
      if (rl.node_depth[nd] > PATH_BODY) return false;
      node = nd;
      return true;
    };
    // the entries that list nothing
    bool invalid = bad;
    for (int it = tid; it < items; it += PB) {
      int ent, k, node;
      if (lists(it, ent, k, node)) continue;
      // unused: a -1 slot or a -1 entry; anything else that lists nothing is an error of the caller's
      invalid |= !(ent == -1 || k == -1) || ent < -1 || ent >= E || k < -1 || k >= rl.n_rules;
      const int64_t at = (int64_t)qi * items + it;
      a.count[at] = 0;
      a.listed[at] = 0;
      int32_t *rows = a.path + at * (int64_t)(a.P * PATH_LEN);
      for (int j = 0; j < a.P * PATH_LEN; ++j) rows[j] = -1;
    }
    if (invalid) atomicOr(&a.flags[CTR_INVALID], 1ull);
    bool carry = false, internal = false;
    int cur = -1;  // the nodes up to here are done
#pragma unroll 1
    while (true) {
      int mn = 0x7fffffff;
      for (int it = tid; it < items; it += PB) {
        int ent, k, node;
        if (lists(it, ent, k, node) && node > cur) mn = min(mn, node);
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) mn = min(mn, __shfl_xor(mn, o, 64));
      if (lane == 0) s_min[wid] = mn;
      if (tid < PATH_LEN) s_nl[tid] = tid == 0;  // level 0: h alone
      __syncthreads();
#pragma unroll
      for (int w = 0; w < PW; ++w) mn = min(mn, s_min[w]);
      if (mn == 0x7fffffff) break;  // (the same for every thread)
      const int len = rl.node_depth[mn];
      if (tid == 0) {
        int nd = mn;
        for (int j = len - 1; j >= 0; --j) {
          s_body[j] = rl.node_rel[nd];
          nd = rl.node_parent[nd];
        }
        lst[0] = h;
        F[h] = 1ull;
      }
      // 1. level k -> k + 1, the waves on a quarter of the list each
      for (int k = 0; k < len; ++k) {
        __syncthreads();
        const int na = min(s_nl[k], E), per = (na + PW - 1) / PW, b0 = min(na, wid * per), mine = min(per, na - b0);
        unsigned long long *Fa = F + (size_t)k * E, *Fb = Fa + E;
        const int *la = lst + (size_t)k * E + b0;
        int *lb = lst + (size_t)(k + 1) * E;
        const int rel = s_body[k];
        const uint32_t bit = 1u << (rel & 31);
        for (int i = lane; i < mine; i += 64) {
          const int v = la[i];
          const unsigned long long nv = ld_u64(&Fa[v]);
          const uint2 vb = g.vbits[(int64_t)v * g.W + (rel >> 5)];
          if (!(vb.x & bit)) continue;
          const int pos = (int)vb.y + __popc(vb.x & (bit - 1u));
          bool own = rel == r && v == rm_src;  // the row's own edge is still ahead among v's edges
          for (int b = g.dvoff[pos], be = g.dvoff[pos + 1]; b < be; ++b) {
            const int x = g.col[b];
            if (own && x == rm_dst) {
              own = false;
              continue;
            }
            const unsigned long long old = atomicAdd(&Fb[x], nv);
            carry |= old + nv < old;
            if (old == 0) {
              const int at = atomicAdd(&s_nl[k + 1], 1);
              if (at < E)
                lb[at] = x;
              else
                internal = true;  // (only after a sum wrapped to exactly zero)
            }
          }
        }
      }
      __syncthreads();
      // 2. one thread per (entry of this node, p)
      for (int w = tid; w < items * a.P; w += PB) {
        const int it = w / a.P, p = w - it * a.P;
        int ent, k, node;
        if (!lists(it, ent, k, node) || node != mn) continue;
        const unsigned long long cnt = ld_u64(&F[(size_t)len * E + ent]);
        const int nl = (int)min((unsigned long long)a.P, cnt);
        const int64_t at = (int64_t)qi * items + it;
        if (p == 0) {
          a.count[at] = (long long)cnt;
          a.listed[at] = nl;
        }
        int32_t *row = a.path + (at * a.P + p) * PATH_LEN;
#pragma unroll
        for (int j = 0; j < PATH_LEN; ++j) row[j] = -1;
        if (p >= nl) continue;
        int x = ent;
        unsigned rank = (unsigned)p;  // < P <= 64, and it only falls
        row[len] = x;
        for (int lev = len; lev >= 1; --lev) {
          const int rel = s_body[lev - 1];
          unsigned long long *Fp = F + (size_t)(lev - 1) * E;
          const int en = g.in_off[x + 1];
          int b = lower_bound_i(g.in_rel, g.in_off[x], en, rel), y = -1;
          const bool own = rel == r && x == rm_dst;  // the row's own edge is among these in-edges
          bool found = false;
          while (b < en && g.in_rel[b] == rel) {
            y = g.in_src[b];
            unsigned mult = 0;  // the edges y -rel-> x that are walked
            for (; b < en && g.in_rel[b] == rel && g.in_src[b] == y; ++b)
              mult += !(own && y == rm_src && g.in_eid[b] == rm_id);
            if (mult == 0) continue;
            const unsigned long long f = ld_u64(&Fp[y]);
            if (f >= (unsigned long long)RNNL_PATHS_MAX || f * mult > rank) {  // (f < 64: the product is small)
              rank /= mult;
              found = true;
              break;
            }
            rank -= (unsigned)(f * mult);
          }
          if (!found) {
            internal = true;
            break;
          }
          x = y;
          row[lev - 1] = x;
        }
      }
      __syncthreads();
      // 3. the levels back to zero, along their lists
      for (int k = 0; k <= len; ++k) {
        unsigned long long *Fk = F + (size_t)k * E;
        const int nk = min(s_nl[k], E);
        for (int i = tid; i < nk; i += PB) Fk[lst[(size_t)k * E + i]] = 0ull;
      }
      __syncthreads();
      cur = mn;
    }
    if (carry) atomicOr(&a.flags[CTR_RANGE], 1ull);
    if (internal) atomicOr(&a.flags[CTR_INTERNAL], 1ull);
    __syncthreads();  // s_min and s_nl are the next row's
  }
}

// The scratch of a launch over n_rows rows: nothing in the LDS regime, one block
// of levels per workgroup above it.
static size_t paths_scratch_bytes(int32_t E, int32_t n_rows) {
  if (E <= PATHS_LDS_E) return 0;
  return (size_t)std::max(1, std::min(n_rows, PATHS_BLOCKS)) * PATHS_PER_E * (size_t)E;
}

}  // namespace rnnl

using namespace rnnl;

extern "C" {

int rnnl_paths_rows_scratch(rnnl_graph g, int32_t n_rows, size_t *bytes) {
  if (!g || n_rows < 0 || !bytes) {
    set_error("rnnl_paths_rows_scratch: bad arguments (a graph, n_rows >= 0, bytes)");
    return RNNL_ERR_INVALID;
  }
  *bytes = paths_scratch_bytes(g->d.E, n_rows);
  return RNNL_OK;
}

int rnnl_paths_rows(rnnl_graph g, rnnl_rules r, const int64_t *all_h, const int64_t *all_r,
                    const int64_t *edges_to_remove, int32_t n_rows, const int32_t *entity, int32_t m,
                    const int32_t *rule, int32_t c, int32_t max_paths, int32_t *listed, int64_t *count, int32_t *path,
                    void *scratch, size_t scratch_bytes, uint64_t *counters, void *stream) {
  if (m < 1) {
    set_error("rnnl_paths_rows: m (the slots per row) must be at least 1");
    return RNNL_ERR_INVALID;
  }
  if (c < 1 || c > PATHS_RULES_MAX) {
    set_error("rnnl_paths_rows: c (the rules per slot) must be 1.." + std::to_string(PATHS_RULES_MAX));
    return RNNL_ERR_INVALID;
  }
  if (max_paths < 1 || max_paths > RNNL_PATHS_MAX) {
    set_error("rnnl_paths_rows: max_paths (the paths per rule) must be 1.." + std::to_string(RNNL_PATHS_MAX));
    return RNNL_ERR_INVALID;
  }
  if (!g || !r || r->E != g->d.E || r->R != g->d.R) {
    set_error("rnnl_paths_rows: no graph handle or no rules handle (or rules of another graph)");
    return RNNL_ERR_INVALID;
  }
  if (n_rows < 0 || (n_rows > 0 && (!all_h || !all_r || !entity || !rule || !listed || !count || !path)) ||
      !counters) {
    set_error("rnnl_paths_rows: bad arguments (n_rows >= 0, no null array)");
    return RNNL_ERR_INVALID;
  }
  const int64_t per_row = (int64_t)c * max_paths * RNNL_PATH_LEN;  // <= 6,144
  if ((int64_t)m > ((int64_t)0x7fffffff) / per_row ||
      (n_rows > 0 && (int64_t)n_rows > ((int64_t)0x7fffffff) / (per_row * m))) {
    set_error("rnnl_paths_rows: path would have 2^31 elements or more (cut the rows into smaller calls)");
    return RNNL_ERR_INVALID;
  }
  const size_t need = paths_scratch_bytes(g->d.E, n_rows);
  if (need > 0 && (!scratch || scratch_bytes < need || (reinterpret_cast<uintptr_t>(scratch) & 7))) {
    set_error("rnnl_paths_rows: scratch too small, null or not 8-byte aligned (rnnl_paths_rows_scratch gives the bytes)");
    return RNNL_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  RNNL_HIP_CHECK(hipMemsetAsync(counters, 0, 4 * sizeof(uint64_t), st));
  if (n_rows == 0) return RNNL_OK;
  PathRowsArgs a = {};
  a.all_h = all_h;
  a.all_r = all_r;
  a.etr = edges_to_remove;
  a.n = n_rows;
  a.m = m;
  a.c = c;
  a.P = max_paths;
  a.entity = entity;
  a.rule = rule;
  a.listed = listed;
  a.count = reinterpret_cast<long long *>(count);
  a.path = path;
  a.scratch = static_cast<unsigned char *>(scratch);
  a.flags = reinterpret_cast<unsigned long long *>(counters);
  if (need == 0) {
    const size_t lds = PATHS_CTRL + PATHS_PER_E * (size_t)g->d.E;
    hipLaunchKernelGGL(paths_rows_kernel<true>, dim3((unsigned)std::min(n_rows, PATHS_GRID_LDS)), dim3(PB), lds, st,
                       g->d, r->d, a);
  } else {
    hipLaunchKernelGGL(paths_rows_kernel<false>, dim3((unsigned)std::min(n_rows, PATHS_BLOCKS)), dim3(PB), PATHS_CTRL,
                       st, g->d, r->d, a);
  }
  RNNL_HIP_CHECK(hipGetLastError());
  return RNNL_OK;
}

}  // extern "C"
