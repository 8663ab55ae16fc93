// What the miner's three query kernels share (eval_kernel of mine_eval.hip,
// predict_kernel and explain_kernel of mine_predict.hip): the layout of a
// workgroup's dense arrays, the grounding of one round of EW rules (hop by hop
// with ground_hop of mine_common.h, which ground_kernel of mine_learn.hip runs
// as well), the round's rules added into val, the lookup of a query's known
// answers, and on the host the checks and the launch the three entry points
// have in common.  One copy of each, so the scores of a prediction are the
// evaluation's bit for bit.  Both files are compiled without contraction
// (-ffp-contract=off).
//
// Layout per workgroup, E entities: val (f64 x E), then per wave w the integer
// scratch of one grounding (GroundScratch, GROUND_PER_E bytes per entity):
// EVAL_PER_E bytes per entity.  predict_kernel adds its candidate list and its
// flag bytes (PRED_PER_E).  Up to EVAL_LDS_E entities all of it lives in LDS,
// above that in the handle's eval_scratch (and pred_flags), zeroed when
// allocated and left zeroed by every query.
//
// The aggregation (rnnl_miner_set_aggregation) is a template
// parameter AGG of the kernels, of a round's grounding and of the round into
// val.  AGG_SUM: path counts, val += wt * count.  AGG_NOISY_OR and AGG_MAX ask
// only whether a rule reaches an entity: the grounding marks the dense slots
// with 1 (ground_hop<HEAD, false>), and a destination's val takes the rule's
// operand l.op[k]: added (noisy-or), or inserted as a 17-bit class into the
// three-field key val holds (max).  The slots are written at the entities of a
// frontier list only (the first touch appends), and the resets walk those
// lists — the old frontier after every hop, the destinations when the round
// enters val — whatever the slots hold; so the scratch regime's "every query
// leaves it zeroed" holds in the new modes as it does for counts.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <type_traits>

#include "internal.h"
#include "mine_common.h"

namespace rnnl {

constexpr int EB = 256;          // threads per workgroup
constexpr int EW = EB / 64;      // waves: rules grounded at once
constexpr int EVAL_LDS_E = 512;  // everything in LDS up to this many entities (52 KiB)
constexpr size_t EVAL_PER_E = 8 + EW * GROUND_PER_E;  // val (f64) + per wave one grounding's integer scratch
constexpr size_t PRED_LIST_PER_E = 4;                 // predict_kernel's candidate list (int), behind those
constexpr size_t PRED_FLAG_PER_E = 1;                 // and its flag bytes, behind the list
constexpr size_t PRED_PER_E = PRED_LIST_PER_E + PRED_FLAG_PER_E;
constexpr size_t EVAL_SCRATCH = 256u << 20;
constexpr int EVAL_MAX_BLOCKS = 2048;

enum : int { AGG_SUM = RNNL_MINER_AGG_SUM, AGG_NOISY_OR = RNNL_MINER_AGG_NOISY_OR, AGG_MAX = RNNL_MINER_AGG_MAX };

// AGG_MAX: class a (> 0) of a firing rule enters the key of an entity: the
// three largest classes so far, with multiplicity, as 17-bit fields c1 c2 c3
// of an integer held exactly in a double; cut to `depth` fields.
__device__ __forceinline__ double agg_max_insert(double key, unsigned a, int depth) {
  const unsigned long long k = (unsigned long long)key;
  unsigned c1 = (unsigned)(k >> 34), c2 = (unsigned)(k >> 17) & 0x1ffffu, c3 = (unsigned)k & 0x1ffffu;
  if (a > c1) {
    c3 = c2;
    c2 = c1;
    c1 = a;
  } else if (a > c2) {
    c3 = c2;
    c2 = a;
  } else if (a > c3) {
    c3 = a;
  }
  if (depth < 3) c3 = 0;
  if (depth < 2) c2 = 0;
  return (double)(((unsigned long long)c1 << 34) | ((unsigned long long)c2 << 17) | c3);
}

// The known answers of (relation, anchor) pairs: keys r * E + anchor ascending,
// key i's answers vals[offs[i], offs[i + 1]) ascending.  keys == nullptr: none.
struct KnownLists {
  const int64_t *keys, *offs;
  const int32_t *vals;
  int64_t n_keys;
};

// the range [b0, b1) of vals that holds the known answers of (r, anc); false, and the range empty, if there are none.
// (k by value, and known_skip on the bare array: through a reference into the kernel's arguments predict_kernel
// compiles to other, longer code with four more VGPRs)
__device__ __forceinline__ bool known_range(const KnownLists k, int r, int anc, int E, int64_t &b0, int64_t &b1) {
  b0 = b1 = 0;
  if (k.keys) {
    const int64_t key = (int64_t)r * E + anc;
    int64_t lo = 0, hi = k.n_keys;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (k.keys[mid] < key)
        lo = mid + 1;
      else
        hi = mid;
    }
    if (lo < k.n_keys && k.keys[lo] == key) {
      b0 = k.offs[lo];
      b1 = k.offs[lo + 1];
      return true;
    }
  }
  return false;
}

// entry i = e of a range from b0 of the known lists' vals is no other known
// answer: out of range, the query's own answer ans, or a repeat of its predecessor
__device__ __forceinline__ bool known_skip(const int32_t *vals, int64_t i, int64_t b0, int e, int E, int ans) {
  if ((unsigned)e >= (unsigned)E || e == ans || (i > b0 && vals[i - 1] == e)) return true;
  return false;
}

// A workgroup's dense arrays: val and, behind it, the waves' integer scratch;
// the dynamic LDS (SMALL) or block blockIdx.x of the handle's scratch.
struct QueryArrays {
  unsigned char *base, *ints;
  double *val;
};

template <bool SMALL>
__device__ __forceinline__ QueryArrays query_arrays(unsigned char *scratch, int E) {
  extern __shared__ unsigned long long eval_smem[];
  QueryArrays q;
  q.base = SMALL ? reinterpret_cast<unsigned char *>(eval_smem)
                 : scratch + (size_t)blockIdx.x * EVAL_PER_E * (size_t)E;
  q.val = reinterpret_cast<double *>(q.base);
  q.ints = q.base + 8 * (size_t)E;
  return q;
}

// SMALL: zero the integer scratch once per workgroup, a barrier to follow (the
// global scratch is zeroed when it is allocated and left zeroed by every query)
__device__ __forceinline__ void eval_zero_ints(unsigned char *ints, int E) {
  for (int i = threadIdx.x; i < EW * 2 * E; i += EB) {
    const int w = i / (2 * E);
    GroundScratch(ints, w, E).ca[i - w * 2 * E] = 0ull;  // counts A and B are contiguous
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
// counts are in the half of the scratch that (length & 1) names.  wide is set
// when any hop carries a count past 32 bits on, whether or not the paths go on
// to a destination (ground_kernel of mine_learn.hip looks at the final counts
// only).  Called by the whole workgroup; the waves stay in step, a wave whose
// rule has ended (act false) only keeps the barriers.  AGG other than AGG_SUM:
// the slots hold 1 where a frontier is, no counts; wide is never set.
template <bool HEAD, int AGG = AGG_SUM>
__device__ __forceinline__ void eval_ground_round(const MinerDev &d, const MinerLearnDev &l, unsigned char *ints,
                                                  int h, int r, int t, int rb, int jb, int nw, int *s_n, int *s_na,
                                                  bool &wide) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int start = HEAD ? t : h;
  int mx = 0;
  for (int w = 0; w < nw; ++w) mx = max(mx, l.rule_len[rb + jb + w]);
  const int rule = rb + jb + wid;
  const int len = wid < nw ? l.rule_len[rule] : 0;
  GroundScratch s(ints, wid, d.E);
  int na = 0;
  if (len > 0) {
    if (lane == 0) {
      s.la[0] = start;
      s.ca[start] = 1;
    }
    na = 1;
  }
  for (int k = 0; k < mx; ++k) {
    const bool act = k < len;
    if (act && lane == 0) s_n[wid] = 0;
    __syncthreads();
    if (act)
      ground_hop<HEAD, AGG == AGG_SUM>(d, l, s, na, lane, l.rule_body[RULE_STRIDE * rule + (HEAD ? len - 1 - k : k)], h, r, t,
                       &s_n[wid], wide);
    __syncthreads();
    if (act) {
      for (int i = lane; i < na; i += 64) s.ca[s.la[i]] = 0;
      na = s_n[wid];
      s.swap();
    }
  }
  if (lane == 0) s_na[wid] = na;
  __syncthreads();
}

// the final counts (ca) and destination list (la) of wave w's rule of length len (> 0)
__device__ __forceinline__ GroundScratch eval_final(unsigned char *ints, int E, int w, int len) {
  return GroundScratch::after(ints, w, E, len);  // one swap per hop
}

// The round's rules into val, one after the other: list order per destination,
// product first, then the add; the destinations of one rule are distinct, so no
// floating-point atomics.  Leaves the integer scratch zeroed.  REACHED: bit 0 of
// reached[x] is set for every destination (a path count > 0, whatever the
// weight), and a destination reached for the first time is appended to
// touched[*n_touched] (an LDS counter): the entities whose val was written.
// AGG_NOISY_OR: val[x] + l.op[k] at every destination, no product.  AGG_MAX:
// the class l.op[k], if > 0, inserted into the key val[x] holds
// (agg_max_insert); one thread per destination within a rule and the barrier
// between rules, as for the sum.
template <bool REACHED, int AGG = AGG_SUM>
__device__ __forceinline__ void eval_round_into_val(const MinerLearnDev &l, unsigned char *ints, int E, int rb, int jb,
                                                    int nw, const int *s_na, double *val, unsigned char *reached,
                                                    int *touched, int *n_touched, bool &wide) {
  for (int w = 0; w < nw; ++w) {
    const int len2 = l.rule_len[rb + jb + w];
    if (len2 == 0) continue;  // an empty body reaches nothing
    const double wt = AGG == AGG_SUM ? l.wt[rb + jb + w] : l.op[rb + jb + w];
    const GroundScratch f = eval_final(ints, E, w, len2);
    const int n2 = s_na[w];
    for (int i = threadIdx.x; i < n2; i += EB) {
      const int x = f.la[i];
      const unsigned long long c = ld_u64(&f.ca[x]);
      if (AGG == AGG_SUM) {
        wide |= c > 0xffffffffull;
        const double term = wt * (double)c;
        val[x] = val[x] + term;
      } else if (AGG == AGG_NOISY_OR) {
        val[x] = val[x] + wt;
      } else if (wt > 0.0) {
        val[x] = agg_max_insert(val[x], (unsigned)wt, l.agg_depth);
      }
      if (REACHED && c > 0 && !reached[x]) {  // one thread per x within a rule, a barrier between rules
        reached[x] = 1;
        touched[atomicAdd(n_touched, 1)] = x;
      }
      f.ca[x] = 0;
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

// who: the entry point without its _side suffix, as its other messages name it
inline bool check_side(const char *who, int32_t side) {
  if (side == RNNL_MINER_TAIL || side == RNNL_MINER_HEAD) return true;
  set_error(std::string(who) + "_side: side must be RNNL_MINER_TAIL or RNNL_MINER_HEAD");
  return false;
}

// The caller's known-answer arrays, all three or none, into k (none, or no key:
// k.keys stays null).  False if only some are given; the message is the caller's.
inline bool known_lists(const int64_t *keys, const int64_t *offs, const int32_t *vals, int64_t n_keys, KnownLists &k) {
  k = KnownLists();
  if (!keys && !offs && !vals) return true;
  if (!keys || !offs || !vals || n_keys < 0) return false;
  if (n_keys > 0) k = KnownLists{keys, offs, vals, n_keys};
  return true;
}

struct NoPrep {
  int operator()() const { return RNNL_OK; }
};

// The launch of a query kernel over n queries, after the entry's own checks:
// clears the counters; picks the kernel by regime (SMALL: E <= EVAL_LDS_E, all
// arrays in dynamic LDS, EVAL_PER_E + extra_per_e bytes per entity; else in the
// handle's scratch, one block per workgroup) and by side; sets a.flags and
// a.scratch.  pick(small, head, agg) returns kernel<decltype(small)::value,
// decltype(head)::value, decltype(agg)::value>; agg is the handle's mode.  prep() runs in the scratch regime only, once the
// scratch and m->eval_blocks exist: what else the kernel needs per workgroup.
template <typename Args, typename Pick, typename Prep = NoPrep>
int query_launch(rnnl_miner m, const char *who, int32_t side, int64_t n, size_t extra_per_e, Args &a,
                 uint64_t *counters, void *stream, Pick pick, Prep prep = Prep()) {
  using T = std::true_type;
  using F = std::false_type;
  hipStream_t st = (hipStream_t)stream;
  RNNL_HIP_CHECK(hipMemsetAsync(counters, 0, 4 * 8, st));
  if (n == 0) return RNNL_OK;
  a.flags = reinterpret_cast<unsigned long long *>(counters);
  const bool head = side == RNNL_MINER_HEAD;
  auto kernel = [&](auto small) {  // the handle's mode and the side as template arguments
    auto by_side = [&](auto agg) { return head ? pick(small, T(), agg) : pick(small, F(), agg); };
    if (m->agg == AGG_NOISY_OR) return by_side(std::integral_constant<int, AGG_NOISY_OR>());
    if (m->agg == AGG_MAX) return by_side(std::integral_constant<int, AGG_MAX>());
    return by_side(std::integral_constant<int, AGG_SUM>());
  };
  if (m->d.E <= EVAL_LDS_E) {
    const unsigned grid = (unsigned)std::min<int64_t>(n, EVAL_MAX_BLOCKS);
    hipLaunchKernelGGL(kernel(T()), dim3(grid), dim3(EB),
                       (EVAL_PER_E + extra_per_e) * (size_t)m->d.E, st, m->d, m->l, a);
  } else {
    int rc = eval_scratch_ensure(m, who);
    if (rc == RNNL_OK) rc = prep();
    if (rc != RNNL_OK) return rc;
    a.scratch = m->eval_scratch;
    const unsigned grid = (unsigned)std::min<int64_t>(n, m->eval_blocks);
    hipLaunchKernelGGL(kernel(F()), dim3(grid), dim3(EB), 0, st, m->d, m->l, a);
  }
  RNNL_HIP_CHECK(hipGetLastError());
  return RNNL_OK;
}

}  // namespace rnnl
