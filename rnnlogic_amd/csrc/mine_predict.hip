// The rule miner's answers to a query: the filtered top-k tails
// of (h, r, ?) by the evaluation's val, and the rules behind each of them.
//
// rnnl_miner_predict.  One 256-thread workgroup per query, grid-stride, in the
// regimes of eval_kernel (mine_eval.hip): val and the integer scratch in LDS up
// to EVAL_LDS_E entities, in the handle's per-workgroup scratch above.  val[e]
// is formed by the code eval_kernel runs (mine_ground.h: rules in list order,
// product then add, no float atomics, the query's own edge skipped on every
// hop), so it is RuleMiner.scores bit for bit; the (n, |E|) matrix is never
// written.  A query with t = -1 is open: no edge is removed, no answer kept.
//
// One byte per entity beside val: bit 0 = reached (some rule with a body has a
// path count > 0 there, whatever its weight), bit 1 = another known tail of
// (h, r) (e != t, the lists and rule of eval_kernel; a duplicate sets the bit
// twice), bit 2 = eligible: (mode `all` or reached) and not bit 1 and val not
// NaN.  The weights a handle takes through RuleMiner are finite, so a NaN val
// needs an overflow (inf - inf); it is never listed and never counted.
//
// Nothing after the grounding walks all |E| entities.  The destinations that
// the rules reach for the first time are appended to a per-workgroup list (the
// touched entities: the only ones whose val is not +0.0), and every later step
// walks that list: eligibility, the counts behind position, the selection and,
// at the end of the query, the reset of val and of the flag bytes, which are
// zeroed in full once per workgroup.  In mode `all` the untouched entities are
// one tie run at +0.0 ordered by id, so at most k of them can be listed: the
// lowest untouched eligible ids are appended to the list as candidates (whole
// 256-id chunks until k are there), and their number ahead of t follows from
// counts (|E| - touched - known untouched, and the same below t).
//
// Order: val descending, then entity id ascending; -0.0 == +0.0, +-inf are
// ordinary values (the rule of topk.hip).  val maps to an order-preserving u64
// key; the list is the k largest (key, |E| - 1 - e) composites.  They are
// found by an MSB-first radix select, one byte per pass over the eligible
// candidates with a 256-bin LDS histogram: 8 passes over the key at most, then
// the bytes of the entity part, which takes the tie run at the k-th place by
// ascending id.  A pass ends the search as soon as the chosen bin holds
// exactly what is still missing.  The <= 256 survivors are sorted by a bitonic
// network in LDS.  Composites are distinct, so the list is a function of the
// inputs alone.
//
// rnnl_miner_explain grounds the query's rules again, in the same rounds; after
// each rule, in list order, the thread of a slot reads the rule's path count at
// the slot's entity and keeps its private list of the c largest contributions
// in the output arrays (insertion, no LDS, no atomics).  total adds
// wt * (double)count in list order, as val does.
//
// The head side (rnnl_miner_predict_side / rnnl_miner_explain_side
// with RNNL_MINER_HEAD): the first k heads of (?, r, t).  val is grounded
// backward from t (mine_ground.h), the known lists are the known heads of
// (r, t), and h is the answer, -1 when the query is open.  The same kernels
// with `anc` the end the grounding starts at and `ans` the answer's end;
// everything from eligibility on reads as on the tail side.
//
// The aggregation: the third template parameter AGG of both
// kernels.  Under AGG_NOISY_OR / AGG_MAX val is built from the rules' operands
// (mine_ground.h) and is still an ordinary non-negative double, so nothing
// from eligibility on changes.  explain_kernel reads 1, not a path count,
// where a rule arrives: a rule's contribution is its operand l.op[k], total
// adds it in list order (noisy-or) or inserts it into the key (max), the
// listed rules are those with the largest operand and every count is 1.
//
// LDS, EVAL_LDS_E = 512 entities: 52 KiB of eval_kernel's arrays + the list
// (2 KiB) + 512 flag bytes + the histogram, the sort buffer and counters
// (4.1 KiB): 58.6 KiB, under 64 KiB.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "internal.h"
#include "mine_ground.h"

namespace rnnl {

constexpr int PRED_K_MAX = RNNL_MINER_TOPK_MAX;  // the survivors are sorted one per thread
static_assert(PRED_K_MAX == EB, "one sort slot per thread");

struct PredArgs {
  const int32_t *queries;
  int64_t n;
  KnownLists known;
  int32_t k, all, blocks;  // blocks: the workgroups flag_scratch is cut for
  int32_t *index;
  double *score;
  int32_t *valid, *position;
  unsigned char *scratch, *flag_scratch;
  unsigned long long *flags;
};

struct ExplArgs {
  const int32_t *queries;
  int64_t n;
  const int32_t *index;
  int32_t m, c;
  int32_t *fired;
  double *total;
  int32_t *rule;
  long long *count;
  unsigned char *scratch;
  unsigned long long *flags;
};

namespace {

// larger key == larger val; -0.0 and +0.0 share a key; NaN is never keyed
__device__ __forceinline__ unsigned long long pred_key(double v) {
  unsigned long long b = (unsigned long long)__double_as_longlong(v);
  if (v == 0.0) b = 0ull;
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// (ka, ea) comes before (kb, eb): key descending, then entity ascending
__device__ __forceinline__ bool pred_before(unsigned long long ka, int ea, unsigned long long kb, int eb) {
  return ka > kb || (ka == kb && ea < eb);
}

// anc: the end the grounding starts at; ans: the answer's end, -1 in an open query
__device__ __forceinline__ bool query_bad(int anc, int r, int ans, int E, int R) {
  return (unsigned)anc >= (unsigned)E || (unsigned)r >= (unsigned)R || ans < -1 || ans >= E;
}

}  // namespace

enum : int { C_TOUCHED, C_ELIG, C_AHEAD, C_SURV, C_KNOWN, C_KNOWN_LT, C_TOUCHED_LT, C_CAND, C_N };

template <bool SMALL, bool HEAD, int AGG>
__global__ __launch_bounds__(EB) void predict_kernel(MinerDev d, MinerLearnDev l, PredArgs a) {
  __shared__ int s_n[EW], s_na[EW];
  __shared__ unsigned int s_hist[256], s_wtot[EW], s_sel[3];
  __shared__ unsigned long long s_key[PRED_K_MAX];
  __shared__ int s_ent[PRED_K_MAX];
  // touched entities; eligible among them; those ahead of the answer; survivors; known answers that left untouched,
  // and those of them below the answer; touched entities below the answer; candidates (touched + appended)
  __shared__ int s_cnt[C_N];
  const int E = d.E, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const QueryArrays q = query_arrays<SMALL>(a.scratch, E);
  double *val = q.val;
  unsigned char *ints = q.ints;
  // the candidate list (int x E) and the flag bytes (E): after eval_kernel's arrays / in scratch of their own, the
  // lists of all workgroups first
  int *cand = SMALL ? reinterpret_cast<int *>(q.base + EVAL_PER_E * (size_t)E)
                    : reinterpret_cast<int *>(a.flag_scratch) + (size_t)blockIdx.x * (size_t)E;
  unsigned char *flg = SMALL ? q.base + (EVAL_PER_E + PRED_LIST_PER_E) * (size_t)E
                             : a.flag_scratch + PRED_LIST_PER_E * (size_t)a.blocks * (size_t)E +
                                   (size_t)blockIdx.x * (size_t)E;
  int nb = 1;  // bytes of the entity part of a composite
  while (nb < 4 && ((unsigned)(E - 1) >> (8 * nb)) != 0) ++nb;
  if (SMALL) eval_zero_ints(ints, E);
  for (int x = tid; x < E; x += EB) {  // once: every query leaves val and the flags zeroed
    val[x] = 0.0;
    flg[x] = 0;
  }
  __syncthreads();
#pragma unroll 1
  for (int64_t qi = blockIdx.x; qi < a.n; qi += gridDim.x) {
    const int h = a.queries[3 * qi], r = a.queries[3 * qi + 1], t = a.queries[3 * qi + 2];
    const int anc = HEAD ? t : h, ans = HEAD ? h : t;
    if (query_bad(anc, r, ans, E, d.R)) {
      if (tid < a.k) {
        a.index[qi * a.k + tid] = -1;
        a.score[qi * a.k + tid] = -INFINITY;
      }
      if (tid == 0) {
        atomicOr(&a.flags[CTR_INVALID], 1ull);
        a.valid[qi] = 0;
        a.position[qi] = -1;
      }
      continue;
    }
    if (tid < C_N) s_cnt[tid] = 0;
    s_key[tid] = 0ull;  // past the survivors: sorts last
    s_ent[tid] = 0x7fffffff;
    __syncthreads();
    const int rb = l.rule_off[r], nr = l.rule_off[r + 1] - rb;
    bool wide = false;
#pragma unroll 1
    for (int jb = 0; jb < nr; jb += EW) {
      const int nw = min(EW, nr - jb);  // rules of this round
      eval_ground_round<HEAD, AGG>(d, l, ints, h, r, t, rb, jb, nw, s_n, s_na, wide);
      eval_round_into_val<true, AGG>(l, ints, E, rb, jb, nw, s_na, val, flg, cand, &s_cnt[C_TOUCHED], wide);
    }
    if (wide) atomicOr(&a.flags[CTR_RANGE], 1ull);
    __syncthreads();
    const int nt = s_cnt[C_TOUCHED];
    // the other known tails of (h, r) / heads of (r, t) leave (bit 1); those no rule reached are counted for `all`
    int64_t kb0, kb1;
    known_range(a.known, r, anc, E, kb0, kb1);
    int kn = 0, knlt = 0;
    for (int64_t i = kb0 + tid; i < kb1; i += EB) {
      const int e = a.known.vals[i];
      if (known_skip(a.known.vals, i, kb0, e, E, ans)) continue;
      const int f = flg[e];  // one thread per distinct e: the lists are ascending within a key
      flg[e] = f | 2;
      if (!(f & 1)) {
        ++kn;
        knlt += e < ans;
      }
    }
    __syncthreads();
    // eligibility (bit 2) of the touched entities, their number and the number of those ahead of t
    bool t_ok = false;
    unsigned long long t_key = 0;
    if (ans >= 0) {
      const double tv = val[ans];
      const int tf = flg[ans];  // bits 0 and 1 are final; bit 2 is written below
      t_ok = (a.all || (tf & 1)) && !(tf & 2) && tv == tv;
      t_key = pred_key(tv);
    }
    int ne = 0, ahead = 0, tlt = 0;
    for (int i = tid; i < nt; i += EB) {
      const int x = cand[i];
      const int f = flg[x];
      const double v = val[x];
      tlt += x < ans;
      if (!(f & 2) && v == v) {
        flg[x] = f | 4;
        ++ne;
        if (t_ok) ahead += pred_before(pred_key(v), x, t_key, ans);
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      ne += __shfl_down(ne, o, 64);
      ahead += __shfl_down(ahead, o, 64);
      tlt += __shfl_down(tlt, o, 64);
      kn += __shfl_down(kn, o, 64);
      knlt += __shfl_down(knlt, o, 64);
    }
    if (lane == 0) {
      atomicAdd(&s_cnt[C_ELIG], ne);
      atomicAdd(&s_cnt[C_AHEAD], ahead);
      atomicAdd(&s_cnt[C_TOUCHED_LT], tlt);
      atomicAdd(&s_cnt[C_KNOWN], kn);
      atomicAdd(&s_cnt[C_KNOWN_LT], knlt);
    }
    if (tid == 0) s_cnt[C_CAND] = nt;
    __syncthreads();
    int n_elig = s_cnt[C_ELIG];  // all eligible entities
    int nce = n_elig;            // the eligible candidates
    int position = t_ok ? s_cnt[C_AHEAD] : -1;
    if (a.all) {
      // the untouched eligible entities: val +0.0, ordered by id
      const unsigned long long zero_key = 0x8000000000000000ull;
      const int n_unt = E - nt - s_cnt[C_KNOWN];
      n_elig += n_unt;
      if (t_ok) {
        if (zero_key > t_key)
          position += n_unt;
        else if (zero_key == t_key)
          position += ans - s_cnt[C_TOUCHED_LT] - s_cnt[C_KNOWN_LT];
      }
      // the lowest of them become candidates: whole chunks of ids until k are there (more do no harm)
      const int want = min(a.k, n_unt);
      int have = 0;
#pragma unroll 1
      for (int x0 = 0; x0 < E && have < want; x0 += EB) {
        const int x = x0 + tid;
        if (x < E && flg[x] == 0) {
          flg[x] = 4;
          cand[atomicAdd(&s_cnt[C_CAND], 1)] = x;  // distinct entities: the list never passes E entries
        }
        __syncthreads();
        have = s_cnt[C_CAND] - nt;
        __syncthreads();
      }
      nce += have;
    }
    const int nc = s_cnt[C_CAND];
    const int nsel = min(a.k, n_elig);
    // the threshold: the first nd bytes of the nsel-th largest composite (nd = 0: every eligible candidate)
    int nd = 0;
    unsigned long long pk = 0;
    unsigned pr = 0;
    if (nce > a.k) {
      unsigned remaining = (unsigned)a.k;
#pragma unroll 1
      for (int p = 0; p < 8 + nb; ++p) {
        s_hist[tid] = 0;
        __syncthreads();
        int last = -1;
        unsigned run = 0;  // a thread's candidates of one tie run fall into one bin: one atomic per run
        for (int i = tid; i < nc; i += EB) {
          const int x = cand[i];
          if (!(flg[x] & 4)) continue;
          const unsigned long long kx = pred_key(val[x]);
          const unsigned rid = (unsigned)(E - 1 - x);
          bool in;
          int dg;
          if (p < 8) {
            in = p == 0 || (kx >> (64 - 8 * p)) == pk;
            dg = (int)((kx >> (56 - 8 * p)) & 255);
          } else {
            in = kx == pk && (p == 8 || (rid >> (8 * (nb - (p - 8)))) == pr);
            dg = (int)((rid >> (8 * (nb - 1 - (p - 8)))) & 255);
          }
          if (!in) continue;
          if (dg == last) {
            ++run;
          } else {
            if (run) atomicAdd(&s_hist[last], run);
            last = dg;
            run = 1;
          }
        }
        if (run) atomicAdd(&s_hist[last], run);
        __syncthreads();
        // bins from 255 down: thread i holds bin 255 - i; the bin where the running sum reaches `remaining`
        const unsigned hv = s_hist[255 - tid];
        unsigned inc = hv;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const unsigned u = __shfl_up(inc, o, 64);
          if (lane >= o) inc += u;
        }
        if (lane == 63) s_wtot[wid] = inc;
        __syncthreads();
        for (int w = 0; w < wid; ++w) inc += s_wtot[w];
        const unsigned above = inc - hv;
        if (above < remaining && remaining <= inc) {  // exactly one thread: 1 <= remaining <= the bins' sum
          s_sel[0] = 255u - (unsigned)tid;
          s_sel[1] = above;
          s_sel[2] = hv;
        }
        __syncthreads();
        remaining -= s_sel[1];
        if (p < 8)
          pk = (pk << 8) | s_sel[0];
        else
          pr = (pr << 8) | s_sel[0];
        nd = p + 1;
        if (s_sel[2] == remaining) break;  // the whole bin is taken (the last pass always ends here: bins of one)
      }
    }
    // the survivors, in any order
    bool overflow = false;
    for (int i = tid; i < nc; i += EB) {
      const int x = cand[i];
      if (!(flg[x] & 4)) continue;
      const unsigned long long kx = pred_key(val[x]);
      const unsigned rid = (unsigned)(E - 1 - x);
      bool take = true;
      if (nd > 8)
        take = kx > pk || (kx == pk && (rid >> (8 * (nb - (nd - 8)))) >= pr);
      else if (nd > 0)
        take = (kx >> (64 - 8 * nd)) >= pk;
      if (take) {
        const int slot = atomicAdd(&s_cnt[C_SURV], 1);
        if (slot < PRED_K_MAX) {
          s_key[slot] = kx;
          s_ent[slot] = x;
        } else {
          overflow = true;
        }
      }
    }
    __syncthreads();
    if (overflow || (tid == 0 && s_cnt[C_SURV] != nsel)) atomicOr(&a.flags[CTR_INTERNAL], 1ull);
    if (nsel > 1) {  // bitonic network over the PRED_K_MAX slots, one per thread
#pragma unroll 1
      for (int size = 2; size <= PRED_K_MAX; size <<= 1) {
#pragma unroll 1
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
          const int other = tid ^ stride;
          if (other > tid) {
            const unsigned long long k0 = s_key[tid], k1 = s_key[other];
            const int e0 = s_ent[tid], e1 = s_ent[other];
            const bool up = (tid & size) == 0;
            if (up ? pred_before(k1, e1, k0, e0) : pred_before(k0, e0, k1, e1)) {
              s_key[tid] = k1;
              s_ent[tid] = e1;
              s_key[other] = k0;
              s_ent[other] = e0;
            }
          }
          __syncthreads();
        }
      }
    }
    if (tid < a.k) {
      const int e = tid < nsel ? s_ent[tid] : -1;
      const bool ok = (unsigned)e < (unsigned)E;  // (an internal mismatch never indexes val out of range)
      a.index[qi * a.k + tid] = ok ? e : -1;
      a.score[qi * a.k + tid] = ok ? val[e] : -INFINITY;
    }
    if (tid == 0) {
      a.valid[qi] = nsel;
      a.position[qi] = position;
    }
    __syncthreads();
    // leave val and the flags zeroed: the candidates and the known tails are all that was written
    for (int i = tid; i < nc; i += EB) {
      const int x = cand[i];
      val[x] = 0.0;
      flg[x] = 0;
    }
    for (int64_t i = kb0 + tid; i < kb1; i += EB) {
      const int e = a.known.vals[i];
      if ((unsigned)e < (unsigned)E) flg[e] = 0;
    }
    __syncthreads();
  }
}

template <bool SMALL, bool HEAD, int AGG>
__global__ __launch_bounds__(EB) void explain_kernel(MinerDev d, MinerLearnDev l, ExplArgs a) {
  __shared__ int s_n[EW], s_na[EW];
  const int E = d.E, tid = threadIdx.x;
  unsigned char *ints = query_arrays<SMALL>(a.scratch, E).ints;  // the layout of eval_kernel; val is not used
  if (SMALL) eval_zero_ints(ints, E);
  __syncthreads();
#pragma unroll 1
  for (int64_t qi = blockIdx.x; qi < a.n; qi += gridDim.x) {
    const int h = a.queries[3 * qi], r = a.queries[3 * qi + 1], t = a.queries[3 * qi + 2];
    const bool bad = HEAD ? query_bad(t, r, h, E, d.R) : query_bad(h, r, t, E, d.R);
    const int64_t slot = qi * a.m + tid;
    int32_t *rl = a.rule + slot * a.c;  // this thread's list, if it has a slot
    long long *cl = a.count + slot * a.c;
    int ent = -1;
    if (tid < a.m) {
      ent = bad ? -1 : a.index[slot];
      if (ent < -1 || ent >= E) {
        atomicOr(&a.flags[CTR_INVALID], 1ull);
        ent = -1;
      }
      for (int j = 0; j < a.c; ++j) {
        rl[j] = -1;
        cl[j] = 0;
      }
      a.fired[slot] = 0;
      a.total[slot] = 0.0;
    }
    if (bad) {
      if (tid == 0) atomicOr(&a.flags[CTR_INVALID], 1ull);
      continue;
    }
    const int rb = l.rule_off[r], nr = l.rule_off[r + 1] - rb;
    bool wide = false;
    int nf = 0, nl = 0;
    double tot = 0.0;
#pragma unroll 1
    for (int jb = 0; jb < nr; jb += EW) {
      const int nw = min(EW, nr - jb);  // rules of this round
      eval_ground_round<HEAD, AGG>(d, l, ints, h, r, t, rb, jb, nw, s_n, s_na, wide);
      for (int w = 0; w < nw; ++w) {  // the round's rules one after the other: list order per slot
        const int len2 = l.rule_len[rb + jb + w];
        if (len2 == 0) continue;  // an empty body reaches nothing
        const GroundScratch f = eval_final(ints, E, w, len2);
        if (ent >= 0) {
          const unsigned long long c = ld_u64(&f.ca[ent]);  // 0 wherever the rule does not arrive
          if (c > 0) {
            // the contribution: wt * count (sum); the rule's operand, u_k or its class (noisy-or, max; c is 1)
            const double term = AGG == AGG_SUM ? l.wt[rb + jb + w] * (double)c : l.op[rb + jb + w];
            if (AGG != AGG_MAX)
              tot = tot + term;
            else if (term > 0.0)
              tot = agg_max_insert(tot, (unsigned)term, l.agg_depth);
            ++nf;
            int pos = nl;  // behind every listed rule that contributes at least as much
            while (pos > 0 && (AGG == AGG_SUM ? l.wt[rb + rl[pos - 1]] * (double)(unsigned long long)cl[pos - 1]
                                              : l.op[rb + rl[pos - 1]]) < term)
              --pos;
            if (pos < a.c) {
              for (int j = min(nl, a.c - 1); j > pos; --j) {
                rl[j] = rl[j - 1];
                cl[j] = cl[j - 1];
              }
              rl[pos] = jb + w;
              cl[pos] = (long long)c;
              nl = min(nl + 1, a.c);
            }
          }
        }
        __syncthreads();
        const int n2 = s_na[w];
        for (int i = tid; i < n2; i += EB) {
          const int x = f.la[i];
          wide |= ld_u64(&f.ca[x]) > 0xffffffffull;
          f.ca[x] = 0;
        }
        __syncthreads();
      }
    }
    if (wide) atomicOr(&a.flags[CTR_RANGE], 1ull);
    if (tid < a.m) {
      a.fired[slot] = nf;
      a.total[slot] = tot;
    }
    __syncthreads();
  }
}

}  // namespace rnnl

using namespace rnnl;

extern "C" {

int rnnl_miner_predict_side(rnnl_miner m, int32_t side, const int32_t *queries, int64_t n, const int64_t *known_keys,
                            const int64_t *known_offs, const int32_t *known_vals, int64_t n_keys, int32_t k,
                            int32_t candidates, int32_t *index, double *score, int32_t *valid, int32_t *position,
                            uint64_t *counters, void *stream) {
  if (!check_side("rnnl_miner_predict", side)) return RNNL_ERR_INVALID;
  if (k < 1 || k > RNNL_MINER_TOPK_MAX) {
    set_error("rnnl_miner_predict: k must be 1.." + std::to_string(RNNL_MINER_TOPK_MAX));
    return RNNL_ERR_INVALID;
  }
  if (candidates != RNNL_MINER_REACHED && candidates != RNNL_MINER_ALL) {
    set_error("rnnl_miner_predict: candidates must be RNNL_MINER_REACHED or RNNL_MINER_ALL");
    return RNNL_ERR_INVALID;
  }
  PredArgs a = {};
  if (!known_lists(known_keys, known_offs, known_vals, n_keys, a.known)) {
    set_error("rnnl_miner_predict: the known-answer arrays all or none");
    return RNNL_ERR_INVALID;
  }
  if (!m || !m->l.rule_off) {
    set_error("rnnl_miner_predict: no handle, or no rules (set the rules first)");
    return RNNL_ERR_INVALID;
  }
  if (n < 0 || (n > 0 && (!queries || !index || !score || !valid || !position)) || !counters) {
    set_error("rnnl_miner_predict: bad arguments (n >= 0, no null array)");
    return RNNL_ERR_INVALID;
  }
  a.queries = queries;
  a.n = n;
  a.k = k;
  a.all = candidates == RNNL_MINER_ALL;
  a.index = index;
  a.score = score;
  a.valid = valid;
  a.position = position;
  return query_launch(
      m, "rnnl_miner_predict", side, n, PRED_PER_E, a, counters, stream,
      [](auto small, auto head, auto agg) {
        return predict_kernel<decltype(small)::value, decltype(head)::value, decltype(agg)::value>;
      },
      [&]() {  // the lists and flags of the scratch's workgroups, in a buffer of their own
        if (!m->pred_flags) {
          void *p = nullptr;
          if (hipMalloc(&p, (size_t)m->eval_blocks * PRED_PER_E * (size_t)m->d.E) != hipSuccess) {
            set_error("rnnl_miner_predict: device allocation failed");
            return (int)RNNL_ERR_NOMEM;
          }
          m->bufs.push_back(p);
          m->pred_flags = static_cast<unsigned char *>(p);
        }
        a.flag_scratch = m->pred_flags;
        a.blocks = m->eval_blocks;
        return (int)RNNL_OK;
      });
}

int rnnl_miner_predict(rnnl_miner m, const int32_t *queries, int64_t n, const int64_t *known_keys,
                       const int64_t *known_offs, const int32_t *known_vals, int64_t n_keys, int32_t k,
                       int32_t candidates, int32_t *index, double *score, int32_t *valid, int32_t *position,
                       uint64_t *counters, void *stream) {
  return rnnl_miner_predict_side(m, RNNL_MINER_TAIL, queries, n, known_keys, known_offs, known_vals, n_keys, k,
                                 candidates, index, score, valid, position, counters, stream);
}

int rnnl_miner_explain_side(rnnl_miner m, int32_t side, const int32_t *queries, int64_t n, const int32_t *index,
                            int32_t n_slots, int32_t c, int32_t *fired, double *total, int32_t *rule, int64_t *count,
                            uint64_t *counters, void *stream) {
  if (!check_side("rnnl_miner_explain", side)) return RNNL_ERR_INVALID;
  if (n_slots < 1 || n_slots > RNNL_MINER_TOPK_MAX) {
    set_error("rnnl_miner_explain: m (the slots per query) must be 1.." + std::to_string(RNNL_MINER_TOPK_MAX));
    return RNNL_ERR_INVALID;
  }
  if (c < 1 || c > RNNL_MINER_EXPLAIN_MAX) {
    set_error("rnnl_miner_explain: c (the rules per slot) must be 1.." + std::to_string(RNNL_MINER_EXPLAIN_MAX));
    return RNNL_ERR_INVALID;
  }
  if (!m || !m->l.rule_off) {
    set_error("rnnl_miner_explain: no handle, or no rules (set the rules first)");
    return RNNL_ERR_INVALID;
  }
  if (n < 0 || (n > 0 && (!queries || !index || !fired || !total || !rule || !count)) || !counters) {
    set_error("rnnl_miner_explain: bad arguments (n >= 0, no null array)");
    return RNNL_ERR_INVALID;
  }
  ExplArgs a = {};
  a.queries = queries;
  a.n = n;
  a.index = index;
  a.m = n_slots;
  a.c = c;
  a.fired = fired;
  a.total = total;
  a.rule = rule;
  a.count = reinterpret_cast<long long *>(count);
  return query_launch(m, "rnnl_miner_explain", side, n, 0, a, counters, stream,
                      [](auto small, auto head, auto agg) {
                        return explain_kernel<decltype(small)::value, decltype(head)::value, decltype(agg)::value>;
                      });
}

int rnnl_miner_explain(rnnl_miner m, const int32_t *queries, int64_t n, const int32_t *index, int32_t n_slots,
                       int32_t c, int32_t *fired, double *total, int32_t *rule, int64_t *count, uint64_t *counters,
                       void *stream) {
  return rnnl_miner_explain_side(m, RNNL_MINER_TAIL, queries, n, index, n_slots, c, fired, total, rule, count, counters,
                                 stream);
}

}  // extern "C"
