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

template <bool SMALL, bool HEAD>
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
      eval_ground_round<HEAD>(d, l, ints, h, r, t, rb, jb, nw, s_n, s_na, wide);
      eval_round_into_val<false>(l, ints, E, rb, jb, nw, s_na, val, nullptr, nullptr, nullptr, wide);
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

}  // namespace rnnl

using namespace rnnl;

extern "C" {

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
                      [](auto small, auto head) { return eval_kernel<decltype(small)::value, decltype(head)::value>; });
}

int rnnl_miner_evaluate(rnnl_miner m, const int32_t *queries, int64_t n, const int64_t *known_keys,
                        const int64_t *known_offs, const int32_t *known_vals, int64_t n_keys, int32_t *ranks,
                        double *val, uint64_t *counters, void *stream) {
  return rnnl_miner_evaluate_side(m, RNNL_MINER_TAIL, queries, n, known_keys, known_offs, known_vals, n_keys, ranks,
                                  val, counters, stream);
}

}  // extern "C"
