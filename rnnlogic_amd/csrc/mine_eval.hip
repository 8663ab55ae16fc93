// The reference miner's evaluation of its rule weights (SURVEY §8(f) f4,
// DESIGN §3.10): ReasoningPredictor::evaluate_thread (miner/rnnlogic.cpp:
// 968-1043) per query triple (h, r, t), on the miner handle's own graph and
// with the rule lists and weights the handle holds.
//
//   val[e]  = sum over relation r's rules k, in list order, of
//             wt[k] * (double)#paths(h -> e along the body), every edge equal
//             to (h, r, t) skipped on every hop;
//   num_g   = #{e unskipped : val[e] >  val[t]}
//   num_ge  = #{e unskipped : val[e] >= val[t]}
// where e is skipped when e != t and (h, r, e) is a known triple.
//
// One 256-thread workgroup per query, grid-stride; the queries are independent
// once the weights are fixed.  Each of the four waves grounds one rule of a
// round of four into integer scratch of its own (frontier list + dense u64
// path counts per hop, integer atomics only, as ground_kernel of
// mine_learn.hip); then the round's rules are added into the dense fp64 val
// one after the other, in list order: product first, then the add, compiled
// without contraction, no floating-point atomics (the destinations of one rule
// are distinct).  So val is the reference's bit for bit.  Nothing is
// materialised per (triple, rule, destination).
//
// Up to EVAL_LDS_E entities val and the integer scratch live in LDS (104 bytes
// per entity, sized by the graph), above that in a per-workgroup global
// scratch kept in the handle.  The grounding of a round and the round into val
// are in mine_ground.h, which the predictions (mine_predict.hip) run as well; a
// hop of the grounding is ground_hop of mine_common.h, the one ground_kernel runs.
//
// The head side (rnnl_miner_evaluate_side with RNNL_MINER_HEAD):
// val[e] = sum of wt[k] * (double)#paths(e -> t along the body), grounded
// backward from t over the in-edges; h is the answer, the known lists are the
// known heads of (r, t).  The same kernel with h and t exchanging roles: `anc`
// is the end the grounding starts at, `ans` the answer's end.
//
// The aggregation (rnnl_miner_set_aggregation below): the third
// template parameter AGG.  AGG_SUM is everything above.  AGG_NOISY_OR and
// AGG_MAX ground reachability, not counts, and val[e] is the sum of the
// operands l.op[k] of the rules that reach e, or the key of their largest
// classes (mine_ground.h); the ranks are taken from val as above.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "internal.h"
#include "mine_ground.h"  // the layout, a round's grounding, the round into val, the known answers, the launch

namespace rnnl {

struct EvalArgs {
  const int32_t *queries;
  int64_t n;
  KnownLists known;
  int32_t *ranks;
  double *val_out;
  unsigned char *scratch;
  unsigned long long *flags;
};

template <bool SMALL, bool HEAD, int AGG>
__global__ __launch_bounds__(EB) void eval_kernel(MinerDev d, MinerLearnDev l, EvalArgs a) {
  __shared__ int s_n[EW], s_na[EW], s_g[EW], s_ge[EW];
  const int E = d.E, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const QueryArrays q = query_arrays<SMALL>(a.scratch, E);
  double *val = q.val;
  unsigned char *ints = q.ints;
  if (SMALL) eval_zero_ints(ints, E);
  __syncthreads();
#pragma unroll 1
  for (int64_t qi = blockIdx.x; qi < a.n; qi += gridDim.x) {
    const int h = a.queries[3 * qi], r = a.queries[3 * qi + 1], t = a.queries[3 * qi + 2];
    if ((unsigned)h >= (unsigned)E || (unsigned)t >= (unsigned)E || (unsigned)r >= (unsigned)d.R) {
      if (tid == 0) {
        atomicOr(&a.flags[CTR_INVALID], 1ull);
        a.ranks[2 * qi] = 0;
        a.ranks[2 * qi + 1] = 0;
      }
      continue;
    }
    const int anc = HEAD ? t : h, ans = HEAD ? h : t;
    for (int x = tid; x < E; x += EB) val[x] = 0.0;
    const int rb = l.rule_off[r], nr = l.rule_off[r + 1] - rb;
    bool wide = false;
#pragma unroll 1
    for (int jb = 0; jb < nr; jb += EW) {
      const int nw = min(EW, nr - jb);  // rules of this round
      eval_ground_round<HEAD, AGG>(d, l, ints, h, r, t, rb, jb, nw, s_n, s_na, wide);
      eval_round_into_val<false, AGG>(l, ints, E, rb, jb, nw, s_na, val, nullptr, nullptr, nullptr, wide);
    }
    if (wide) atomicOr(&a.flags[CTR_RANGE], 1ull);
    __syncthreads();
    const double t_val = val[ans];
    int g = 0, ge = 0;
    for (int x = tid; x < E; x += EB) {
      const double v = val[x];
      if (a.val_out) a.val_out[qi * (int64_t)E + x] = v;
      if (x != ans) {
        g += v > t_val;
        ge += v >= t_val;
      }
    }
    int64_t b0, b1;  // minus the other known tails of (h, r) / known heads of (r, t)
    if (known_range(a.known, r, anc, E, b0, b1))
      for (int64_t i = b0 + tid; i < b1; i += EB) {
        const int e = a.known.vals[i];
        if (known_skip(a.known.vals, i, b0, e, E, ans)) continue;
        const double v = val[e];
        g -= v > t_val;
        ge -= v >= t_val;
      }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      g += __shfl_down(g, o, 64);
      ge += __shfl_down(ge, o, 64);
    }
    if (lane == 0) {
      s_g[wid] = g;
      s_ge[wid] = ge;
    }
    __syncthreads();
    if (tid == 0) {
      int sg = 0, sge = 1;  // the answer itself always counts
      for (int w = 0; w < EW; ++w) {
        sg += s_g[w];
        sge += s_ge[w];
      }
      a.ranks[2 * qi] = sg;
      a.ranks[2 * qi + 1] = sge;
    }
    __syncthreads();
  }
}

// rnnl_miner_set_aggregation's check of its operand: finite and >= 0; is_max: an integer class <= 131,071
__global__ void agg_check_kernel(const double *op, int n, int is_max, unsigned int *bad) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const double v = op[i];
    bool ok = v >= 0.0 && v < INFINITY;  // (false for a NaN)
    if (ok && is_max) ok = v <= (double)RNNL_MINER_AGG_CLASS_MAX && (double)(unsigned)v == v;
    if (!ok) atomicOr(bad, 1u);
  }
}

}  // namespace rnnl

using namespace rnnl;

extern "C" {

int rnnl_miner_set_aggregation(rnnl_miner m, int32_t agg, int32_t depth, const double *operand, void *stream) {
  if (agg != RNNL_MINER_AGG_SUM && agg != RNNL_MINER_AGG_NOISY_OR && agg != RNNL_MINER_AGG_MAX) {
    set_error("rnnl_miner_set_aggregation: agg must be RNNL_MINER_AGG_SUM, _NOISY_OR or _MAX");
    return RNNL_ERR_INVALID;
  }
  if (agg == RNNL_MINER_AGG_MAX && (depth < 1 || depth > 3)) {
    set_error("rnnl_miner_set_aggregation: depth must be 1..3");
    return RNNL_ERR_INVALID;
  }
  if (!m || !m->l.rule_off || (agg != RNNL_MINER_AGG_SUM && m->l.n_rules > 0 && !operand)) {
    set_error("rnnl_miner_set_aggregation: bad arguments (set the rules first; an operand per rule)");
    return RNNL_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  const int n = m->l.n_rules;
  if (agg != RNNL_MINER_AGG_SUM && n > 0) {
    unsigned int *bad = nullptr, host_bad = 0;
    if (hipMalloc(reinterpret_cast<void **>(&bad), sizeof(unsigned int)) != hipSuccess) {
      set_error("rnnl_miner_set_aggregation: device allocation failed");
      return RNNL_ERR_NOMEM;
    }
    hipError_t e = hipMemsetAsync(bad, 0, sizeof(unsigned int), st);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(agg_check_kernel, dim3((unsigned)std::min(1024, (n + 255) / 256)), dim3(256), 0, st, operand,
                         n, (int)(agg == RNNL_MINER_AGG_MAX), bad);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&host_bad, bad, sizeof(unsigned int), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(bad);
    RNNL_HIP_CHECK(e);
    if (host_bad) {
      set_error(agg == RNNL_MINER_AGG_MAX
                    ? "rnnl_miner_set_aggregation: a class is not an integer in 0..131071"
                    : "rnnl_miner_set_aggregation: an operand is not finite and >= 0");
      return RNNL_ERR_INVALID;
    }
    RNNL_HIP_CHECK(hipMemcpyAsync(m->l.op, operand, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
    RNNL_HIP_CHECK(hipStreamSynchronize(st));
  }
  m->agg = agg;
  m->l.agg_depth = agg == RNNL_MINER_AGG_MAX ? depth : 1;
  return RNNL_OK;
}

int rnnl_miner_set_weights(rnnl_miner m, const double *weights, void *stream) {
  if (!m || !m->l.rule_off || (m->l.n_rules > 0 && !weights)) {
    set_error("rnnl_miner_set_weights: bad arguments (set the rules first)");
    return RNNL_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  const size_t bytes = (size_t)m->l.n_rules * 8;
  if (bytes) {
    RNNL_HIP_CHECK(hipMemcpyAsync(m->l.wt, weights, bytes, hipMemcpyDeviceToDevice, st));
    RNNL_HIP_CHECK(hipMemsetAsync(m->l.am, 0, 3 * bytes, st));  // am, av, at are contiguous
  }
  return RNNL_OK;
}

int rnnl_miner_evaluate_side(rnnl_miner m, int32_t side, const int32_t *queries, int64_t n,
                             const int64_t *known_keys, const int64_t *known_offs, const int32_t *known_vals,
                             int64_t n_keys, int32_t *ranks, double *val, uint64_t *counters, void *stream) {
  if (!check_side("rnnl_miner_evaluate", side)) return RNNL_ERR_INVALID;
  EvalArgs a = {};
  const bool known_ok = known_lists(known_keys, known_offs, known_vals, n_keys, a.known);
  if (!m || !m->l.rule_off || n < 0 || (n > 0 && (!queries || !ranks)) || !counters || !known_ok) {
    set_error("rnnl_miner_evaluate: bad arguments (set the rules first; the known-answer arrays all or none)");
    return RNNL_ERR_INVALID;
  }
  a.queries = queries;
  a.n = n;
  a.ranks = ranks;
  a.val_out = val;
  return query_launch(m, "rnnl_miner_evaluate", side, n, 0, a, counters, stream,
                      [](auto small, auto head, auto agg) {
                        return eval_kernel<decltype(small)::value, decltype(head)::value, decltype(agg)::value>;
                      });
}

int rnnl_miner_evaluate(rnnl_miner m, const int32_t *queries, int64_t n, const int64_t *known_keys,
                        const int64_t *known_offs, const int32_t *known_vals, int64_t n_keys, int32_t *ranks,
                        double *val, uint64_t *counters, void *stream) {
  return rnnl_miner_evaluate_side(m, RNNL_MINER_TAIL, queries, n, known_keys, known_offs, known_vals, n_keys, ranks,
                                  val, counters, stream);
}

}  // extern "C"
