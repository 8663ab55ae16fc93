// The reference miner after its search: one
// weight per rule learned by online Adam over the train triples
// (ReasoningPredictor::learn, miner/rnnlogic.cpp:728-845) and the H score per
// rule (H_score, :847-940), on the miner handle's own graph.  Everything on
// weights, Adam state, logits and H is fp64 and compiled without contraction,
// every sum has a fixed order and nothing floating-point is accumulated by
// atomics: the result is a function of the triple order alone, bitwise.
//
// Three stages per chunk of triples (the caller cuts chunks to a byte budget):
//   ground  one 64-thread workgroup per (triple, rule) pair walks the body hop
//           by hop (KnowledgeGraph::rule_destination, :412-442): a frontier
//           list + dense u64 path counts in a per-workgroup scratch, integer
//           atomics only; every edge equal to the triple (h, r, t) is skipped
//           on every hop, duplicates included.  A count pass gives the number
//           of destinations per pair, a one-workgroup scan the offsets, a fill
//           pass the (destination ascending, u32 count) entries.  A count past
//           u32 sets the range flag.
//   learn   one workgroup per head relation walks its triples of the chunk in
//           order.  Logits: wave 0 adds wt * count / temp into a dense array
//           rule after rule (list order per destination, as the reference's
//           map); softmax over the destinations ascending; then one lane per
//           rule runs that rule's Adam sequence over its own entries.
//   hscore  same walk; val per rule with lanes over rules, softmax over the
//           rules (or top-k: val descending, then rule position), H += share.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "internal.h"
#include "mine_common.h"  // the counters, the scratch of a grounding and its hop: the one the query kernels run

namespace rnnl {

constexpr int GB = 64;          // ground: threads per workgroup (one wave, as ground_hop takes it)
constexpr int LB = 1024;        // learn / hscore: threads per workgroup (lanes over a relation's rules)
constexpr int SMALL_E = 2048;   // dense per-relation arrays live in LDS up to this many entities
constexpr size_t GROUND_SCRATCH = 256u << 20;

// first index in [lo, hi) of the (relation, target)-sorted edges with (rel, dst) >= (r, x): the target lookup of
// learn_triple (the run of a relation alone is lower_bound_i on rel)
__device__ __forceinline__ int edge_lower(const int32_t *rel, const int32_t *dst, int lo, int hi, int r, int x) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const int a = rel[mid];
    if (a < r || (a == r && dst[mid] < x))
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// chunk position of a pair: the largest p in [0, count) with pair_base[p] <= pair
__device__ __forceinline__ int pair_triple(const int64_t *pair_base, int count, int64_t pair) {
  int lo = 0, hi = count - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (pair_base[mid] <= pair)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

// Per-workgroup scratch: one GroundScratch block.  A hop is the tail side of
// ground_hop; its report of a count past 32 bits carried over an inner hop is
// not used here: only the final counts become entries, so only they raise
// CTR_RANGE (the query kernels raise it on any hop: mine_ground.h).
template <bool FILL>
__global__ __launch_bounds__(GB) void ground_kernel(MinerDev d, MinerLearnDev l, const int32_t *__restrict__ order,
                                                    int64_t begin, int32_t count,
                                                    const int64_t *__restrict__ pair_base, int64_t npairs,
                                                    int64_t *pair_off, int32_t *__restrict__ ent_dst,
                                                    uint32_t *__restrict__ ent_cnt, int64_t ent_cap,
                                                    unsigned char *scratch, unsigned long long *flags) {
  const int E = d.E, tid = threadIdx.x;
  const GroundScratch s0(scratch, blockIdx.x, E);
  __shared__ int s_n;
#pragma unroll 1
  for (int64_t pair = blockIdx.x; pair < npairs; pair += gridDim.x) {
    const int p = pair_triple(pair_base, count, pair);
    const int ti = order[begin + p];
    int len = 0, h = 0, r = 0, t = 0, rule = 0;
    if ((unsigned)ti < (unsigned)d.n) {
      h = d.th[ti];
      r = d.tr[ti];
      t = d.tt[ti];
      rule = l.rule_off[r] + (int)(pair - pair_base[p]);
      if (rule < l.rule_off[r + 1])
        len = l.rule_len[rule];
      else if (tid == 0)
        atomicOr(&flags[CTR_INTERNAL], 1ull);
    } else if (tid == 0) {
      atomicOr(&flags[CTR_INVALID], 1ull);
    }
    GroundScratch s = s0;
    int na = 0;
    if (len > 0) {
      if (tid == 0) {
        s.la[0] = h;
        s.ca[h] = 1;
      }
      na = 1;
    }
    __syncthreads();
    for (int k = 0; k < len; ++k) {
      if (tid == 0) s_n = 0;
      __syncthreads();
      bool inner = false;  // a count past 32 bits on the way: not reported, see above
      ground_hop<false>(d, l, s, na, tid, l.rule_body[RULE_STRIDE * rule + k], h, r, t, &s_n, inner);
      __syncthreads();
      for (int i = tid; i < na; i += GB) s.ca[s.la[i]] = 0;
      na = s_n;
      __syncthreads();
      s.swap();
    }
    // la[0, na) are the destinations, ca[] their path counts
    unsigned long long *ca = s.ca;
    const int *la = s.la;
    bool wide = false;
    for (int i = tid; i < na; i += GB) wide |= ld_u64(&ca[la[i]]) > 0xffffffffull;
    if (wide) atomicOr(&flags[CTR_RANGE], 1ull);
    if (!FILL) {
      if (tid == 0) pair_off[pair] = na;
    } else {
      const int64_t base = pair_off[pair];
      if (pair_off[pair + 1] - base != na || base < 0 || base + na > ent_cap) {
        if (tid == 0) atomicOr(&flags[CTR_INTERNAL], 1ull);
      } else if (na <= GB) {
        if (tid < na) {
          const int x = la[tid];
          int rank = 0;
          for (int k = 0; k < na; ++k) rank += la[k] < x;
          ent_dst[base + rank] = x;
          ent_cnt[base + rank] = (uint32_t)ld_u64(&ca[x]);
        }
      } else {
        int run = 0;
        for (int b0 = 0; b0 < E; b0 += GB) {
          const int x = b0 + tid;
          const unsigned long long c = x < E ? ld_u64(&ca[x]) : 0ull;
          const unsigned long long bal = __ballot(c != 0);
          if (c != 0) {
            const int pos = run + __popcll(bal & ((1ull << tid) - 1ull));
            ent_dst[base + pos] = x;
            ent_cnt[base + pos] = (uint32_t)c;
          }
          run += __popcll(bal);
        }
      }
    }
    __syncthreads();
    for (int i = tid; i < na; i += GB) ca[la[i]] = 0;
    __syncthreads();
  }
}

// In-place exclusive scan of a[0, n) by one workgroup; a[n] and flags[CTR_TOTAL] get the total.
__global__ __launch_bounds__(1024) void scan_kernel(int64_t *a, int64_t n, unsigned long long *flags) {
  __shared__ long long ws[17];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  long long carry = 0;
  for (int64_t b = 0; b < n; b += 1024) {
    const int64_t i = b + tid;
    const long long x = i < n ? (long long)a[i] : 0ll;
    long long v = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const long long y = __shfl_up(v, o, 64);
      if (lane >= o) v += y;
    }
    if (lane == 63) ws[wid] = v;
    __syncthreads();
    if (tid == 0) {
      long long acc = 0;
      for (int w = 0; w < 16; ++w) {
        const long long s = ws[w];
        ws[w] = acc;
        acc += s;
      }
      ws[16] = acc;
    }
    __syncthreads();
    if (i < n) a[i] = (int64_t)(v - x + ws[wid] + carry);
    carry += ws[16];
    __syncthreads();
  }
  if (tid == 0) {
    a[n] = (int64_t)carry;
    flags[CTR_TOTAL] = (unsigned long long)carry;
  }
}

struct ChainArgs {
  const int32_t *order;
  int64_t begin;
  int32_t count;
  const int64_t *pair_base, *pair_off;
  const int32_t *ent_dst;
  const uint32_t *ent_cnt;
  unsigned char *scratch;  // per relation: E doubles, E ints (stamp), E ints (list)
  double lr, wd, temp, log_b1, log_b2;
  int32_t fast;
  int32_t top_k;
  double h_temp, prior_weight;
};

struct ChainSmem {
  double logit[SMALL_E];
  int stamp[SMALL_E], list[SMALL_E];
  double red[LB], part[32];
  int rel[LB], cnt[LB];
  int wc[LB / 64];
  double bc;
};

// Parameter::update (rnnlogic.cpp:67-82)
__device__ __forceinline__ void adam_update(double &data, double &m, double &v, double &t, double grad, double lr,
                                            double wd, double log_b1, double log_b2) {
  const double g = grad - wd * data;
  t += 1;
  m = 0.9 * m + 0.1 * g;
  v = 0.999 * v + 0.001 * g * g;
  const double bias1 = 1 - exp(log_b1 * t);
  const double bias2 = 1 - exp(log_b2 * t);
  const double mt = m / bias1;
  const double vt = sqrt(v) / sqrt(bias2) + 0.00000001;
  data += lr * mt / vt;
}

__device__ __forceinline__ double block_max(double x, ChainSmem &S) {
  S.red[threadIdx.x] = x;
  __syncthreads();
  for (int o = LB / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) S.red[threadIdx.x] = fmax(S.red[threadIdx.x], S.red[threadIdx.x + o]);
    __syncthreads();
  }
  const double r = S.red[0];
  __syncthreads();
  return r;
}

// One triple of ReasoningPredictor::learn_thread (:757-811) for the workgroup's relation.
__device__ __forceinline__ void learn_triple(const MinerDev &d, const MinerLearnDev &l, const ChainArgs &a,
                                             ChainSmem &S, double *logit, int *stamp, int *list, int p, int r,
                                             int rb, int nr) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int ti = a.order[a.begin + p];
  const int h = d.th[ti];
  const int64_t pb = a.pair_base[p];
  const int64_t e0 = a.pair_off[pb], e1 = a.pair_off[pb + nr];
  if (e0 == e1) return;  // no rule grounds: nothing changes
  const int seq = p + 1;
  // logits, in rule order per destination: the entries of 64 rules at a time
  // are read coalesced, then applied one rule after the other
  if (wid == 0) {
    for (int jb = 0; jb < nr; jb += 64) {
      const int j = jb + lane;
      const int64_t off = a.pair_off[pb + min(j, nr)];
      const double w = j < nr ? l.wt[rb + j] : 0.0;
      const int64_t bbeg = a.pair_off[pb + jb], bend = a.pair_off[pb + min(jb + 64, nr)];
      for (int64_t c0 = bbeg; c0 < bend; c0 += 64) {
        const int64_t e = c0 + lane;
        const bool act = e < bend;
        int dst = 0;
        uint32_t cnt = 0;
        if (act) {
          dst = a.ent_dst[e];
          cnt = a.ent_cnt[e];
        }
        int lo = 0, hi = 63;  // the entry's rule: the last lane whose offset is <= e
        while (__any(lo < hi)) {
          const int mid = (lo + hi + 1) >> 1;
          const long long o = __shfl((long long)off, mid, 64);
          if (lo < hi) {
            if (o <= e)
              lo = mid;
            else
              hi = mid - 1;
          }
        }
        const double term = __shfl(w, lo, 64) * (double)cnt / a.temp;
        unsigned long long todo = __ballot(act);
        while (todo) {
          const int first = __ffsll((long long)todo) - 1;
          const int jr = __shfl(lo, first, 64);
          const bool mine = act && lo == jr;
          if (mine) {
            if (stamp[dst] != seq) {
              stamp[dst] = seq;
              logit[dst] = 0.0 + term;
            } else {
              logit[dst] += term;
            }
          }
          todo &= ~__ballot(mine);
          __threadfence_block();
        }
      }
    }
  }
  __syncthreads();
  // the destinations, ascending
  int D = 0;
  for (int b0 = 0; b0 < d.E; b0 += LB) {
    const int x = b0 + tid;
    const bool has = x < d.E && stamp[x] == seq;
    const unsigned long long bal = __ballot(has);
    if (lane == 0) S.wc[wid] = __popcll(bal);
    __syncthreads();
    int before = D;
    for (int w = 0; w < wid; ++w) before += S.wc[w];
    if (has) list[before + __popcll(bal & ((1ull << lane) - 1ull))] = x;
    for (int w = 0; w < LB / 64; ++w) D += S.wc[w];
    __syncthreads();
  }
  double mx = -1000000.0;
  for (int i = tid; i < D; i += LB) mx = fmax(mx, logit[list[i]]);
  mx = block_max(mx, S);
  for (int i = tid; i < D; i += LB) logit[list[i]] = exp(logit[list[i]] - mx);
  __syncthreads();
  if (tid == 0) {
    double s = 0;
    for (int i = 0; i < D; ++i) s += logit[list[i]];
    S.bc = s;
  }
  __syncthreads();
  const double sum = S.bc;
  for (int i = tid; i < D; i += LB) {
    const int x = list[i];
    const int hb = d.out_off[h], he = d.out_off[h + 1];
    const int k = edge_lower(l.so_rel, l.so_dst, hb, he, r, x);
    const double target = (k < he && l.so_rel[k] == r && l.so_dst[k] == x) ? 1.0 : 0;
    logit[x] = (target - logit[x] / sum) / a.temp;
  }
  __syncthreads();
  // one lane per rule: its Adam sequence over its own destinations, ascending
  for (int j = tid; j < nr; j += LB) {
    const int64_t lb = a.pair_off[pb + j], le = a.pair_off[pb + j + 1];
    if (lb == le) continue;
    double data = l.wt[rb + j], m = l.am[rb + j], v = l.av[rb + j], t = l.at[rb + j];
    for (int64_t e = lb; e < le; ++e) {
      const double g = logit[a.ent_dst[e]];
      const uint32_t c = a.ent_cnt[e];
      if (a.fast)
        adam_update(data, m, v, t, g * (double)c, a.lr, a.wd, a.log_b1, a.log_b2);
      else
        for (uint32_t k = 0; k < c; ++k) adam_update(data, m, v, t, g, a.lr, a.wd, a.log_b1, a.log_b2);
    }
    l.wt[rb + j] = data;
    l.am[rb + j] = m;
    l.av[rb + j] = v;
    l.at[rb + j] = t;
  }
  __syncthreads();
}

// One triple of H_score_thread (:876-934).
__device__ __forceinline__ void hscore_triple(const MinerDev &d, const MinerLearnDev &l, const ChainArgs &a,
                                              ChainSmem &S, int *stamp, int p, int rb, int nr) {
  const int tid = threadIdx.x;
  const int ti = a.order[a.begin + p];
  const int t = d.tt[ti];
  const int64_t pb = a.pair_base[p];
  const int64_t e0 = a.pair_off[pb], e1 = a.pair_off[pb + nr];
  const int seq = p + 1;
  // distinct destinations over all rules
  int fresh = 0;
  for (int64_t e = e0 + tid; e < e1; e += LB) fresh += atomicExch(&stamp[a.ent_dst[e]], seq) != seq;
  S.cnt[tid] = fresh;
  __syncthreads();
  for (int o = LB / 2; o > 0; o >>= 1) {
    if (tid < o) S.cnt[tid] += S.cnt[tid + o];
    __syncthreads();
  }
  const double D = (double)S.cnt[0];
  __syncthreads();
  double mx = -1000000.0;
  for (int j = tid; j < nr; j += LB) {
    const double w = l.wt[rb + j];
    double val = l.prior[rb + j] * a.prior_weight;
    for (int64_t e = a.pair_off[pb + j], le = a.pair_off[pb + j + 1]; e < le; ++e) {
      const double wc = w * (double)a.ent_cnt[e];
      if (a.ent_dst[e] == t) val += wc;
      val -= wc / D;
    }
    if (a.top_k == 0) val /= a.h_temp;
    l.val[rb + j] = val;
    mx = fmax(mx, val);
  }
  const double n_train = (double)d.n;
  if (a.top_k == 0) {
    mx = block_max(mx, S);
    for (int j = tid; j < nr; j += LB) l.val[rb + j] = exp(l.val[rb + j] - mx);
    __syncthreads();
    // sum over the rules in a fixed order: LB contiguous runs, 32 runs of those, then these in order
    const int run = (nr + LB - 1) / LB;
    double s = 0;
    for (int j = tid * run; j < min(nr, (tid + 1) * run); ++j) s += l.val[rb + j];
    S.red[tid] = s;
    __syncthreads();
    if (tid < 32) {
      double part = 0;
      for (int i = tid * (LB / 32); i < (tid + 1) * (LB / 32); ++i) part += S.red[i];
      S.part[tid] = part;
    }
    __syncthreads();
    if (tid == 0) {
      double tot = 0;
      for (int i = 0; i < 32; ++i) tot += S.part[i];
      S.bc = tot;
    }
    __syncthreads();
    const double sum = S.bc;
    for (int j = tid; j < nr; j += LB) l.H[rb + j] += l.val[rb + j] / sum / n_train;
  } else {
    __syncthreads();
    for (int j = tid; j < nr; j += LB) {
      const double v = l.val[rb + j];
      int above = 0;  // val descending, then position ascending
      for (int k = 0; k < nr && above < a.top_k; ++k) {
        const double u = l.val[rb + k];
        above += (u > v) || (u == v && k < j);
      }
      if (above < a.top_k) l.H[rb + j] += 1.0 / (double)a.top_k / n_train;
    }
  }
  __syncthreads();
}

template <bool LEARN>
__global__ __launch_bounds__(LB) void chain_kernel(MinerDev d, MinerLearnDev l, ChainArgs a) {
  __shared__ ChainSmem S;
  const int r = blockIdx.x, tid = threadIdx.x;
  const int rb = l.rule_off[r], nr = l.rule_off[r + 1] - rb;
  if (nr == 0) return;
  const bool small = d.E <= SMALL_E;
  unsigned char *g = a.scratch + (size_t)r * 16 * (size_t)d.E;
  double *logit = small ? S.logit : reinterpret_cast<double *>(g);
  int *stamp = small ? S.stamp : reinterpret_cast<int *>(g + 8 * (size_t)d.E);
  int *list = small ? S.list : reinterpret_cast<int *>(g + 12 * (size_t)d.E);
  for (int x = tid; x < d.E; x += LB) stamp[x] = 0;
  __syncthreads();
  for (int p0 = 0; p0 < a.count; p0 += LB) {
    const int pp = p0 + tid;
    int rel = -1;
    if (pp < a.count) {
      const int ti = a.order[a.begin + pp];
      if ((unsigned)ti < (unsigned)d.n) rel = d.tr[ti];
    }
    const int ntile = min(LB, a.count - p0);
    __syncthreads();
    S.rel[tid] = rel;
    __syncthreads();
    for (int q = 0; q < ntile; ++q) {
      if (S.rel[q] != r) continue;
      if (LEARN)
        learn_triple(d, l, a, S, logit, stamp, list, p0 + q, r, rb, nr);
      else
        hscore_triple(d, l, a, S, stamp, p0 + q, rb, nr);
    }
  }
}

}  // namespace rnnl

using namespace rnnl;

namespace {

int dev_alloc(rnnl_miner m, size_t bytes, void **out) {
  void *p = nullptr;
  if (hipMalloc(&p, std::max<size_t>(bytes, 8)) != hipSuccess) return RNNL_ERR_NOMEM;
  m->rule_bufs.push_back(p);
  *out = p;
  return RNNL_OK;
}

bool chunk_args_ok(rnnl_miner m, const int32_t *order, int64_t begin, int64_t count, const int64_t *pair_base,
                   int64_t n_pairs, const int64_t *pair_off) {
  return m && m->l.rule_off && order && begin >= 0 && count >= 1 && count < INT32_MAX && pair_base && n_pairs >= 0 &&
         pair_off;
}

}  // namespace

extern "C" {

// stride: relations per rule in the caller's rule_body (3 or RULE_STRIDE); max_len: the longest body it may hold
static int set_rules_impl(rnnl_miner m, const int32_t *rule_off, const int32_t *rule_len, const int32_t *rule_body,
                          const double *prior, int stride, int max_len, const std::string &who) {
  if (!m || !rule_off || rule_off[0] != 0) {
    set_error(who + ": bad arguments");
    return RNNL_ERR_INVALID;
  }
  const int R = m->d.R, E = m->d.E;
  for (int r = 0; r < R; ++r)
    if (rule_off[r + 1] < rule_off[r]) {
      set_error(who + ": rule_off must not decrease");
      return RNNL_ERR_INVALID;
    }
  const int32_t n = rule_off[R];
  if (n > 0 && (!rule_len || !rule_body)) {
    set_error(who + ": rule_len / rule_body missing");
    return RNNL_ERR_INVALID;
  }
  for (int32_t i = 0; i < n; ++i) {
    if (rule_len[i] < 0 || rule_len[i] > max_len) {
      set_error(who + ": body length must be 0.." + std::to_string(max_len));
      return RNNL_ERR_INVALID;
    }
    for (int k = 0; k < rule_len[i]; ++k)
      if (rule_body[(size_t)stride * i + k] < 0 || rule_body[(size_t)stride * i + k] >= R) {
        set_error(who + ": body relation out of range");
        return RNNL_ERR_INVALID;
      }
  }
  std::vector<int32_t> packed((size_t)n * RULE_STRIDE, 0);  // the handle's storage: RULE_STRIDE per rule
  for (int32_t i = 0; i < n; ++i)
    for (int k = 0; k < rule_len[i]; ++k) packed[(size_t)RULE_STRIDE * i + k] = rule_body[(size_t)stride * i + k];
  RNNL_HIP_CHECK(hipDeviceSynchronize());  // earlier work may still read the old lists
  for (void *p : m->rule_bufs) (void)hipFree(p);
  m->rule_bufs.clear();
  const rnnl::MinerLearnDev keep = m->l;
  m->l = rnnl::MinerLearnDev();
  m->l.so_rel = keep.so_rel;
  m->l.so_dst = keep.so_dst;
  m->l.si_rel = keep.si_rel;
  m->l.si_src = keep.si_src;
  m->l.n_rules = n;
  // workgroups of the grounding pass: bounded by their scratch (GROUND_PER_E bytes per entity each)
  m->ground_blocks =
      (int32_t)std::max<size_t>(64, std::min<size_t>(4096, GROUND_SCRATCH / (GROUND_PER_E * (size_t)E)));
  void *p_off, *p_len, *p_body, *p_prior, *p_state, *p_gs, *p_cs;
  int rc = dev_alloc(m, (size_t)(R + 1) * 4, &p_off);
  if (rc == RNNL_OK) rc = dev_alloc(m, (size_t)n * 4, &p_len);
  if (rc == RNNL_OK) rc = dev_alloc(m, (size_t)n * 4 * RULE_STRIDE, &p_body);
  if (rc == RNNL_OK) rc = dev_alloc(m, (size_t)n * 8, &p_prior);
  if (rc == RNNL_OK) rc = dev_alloc(m, (size_t)n * 8 * 7, &p_state);
  if (rc == RNNL_OK) rc = dev_alloc(m, (size_t)m->ground_blocks * GROUND_PER_E * (size_t)E, &p_gs);
  if (rc == RNNL_OK) rc = dev_alloc(m, (size_t)R * 16 * (size_t)E, &p_cs);
  if (rc != RNNL_OK) {
    set_error(who + ": device allocation failed");
    return rc;
  }
  RNNL_HIP_CHECK(hipMemcpy(p_off, rule_off, (size_t)(R + 1) * 4, hipMemcpyHostToDevice));
  if (n > 0) {
    RNNL_HIP_CHECK(hipMemcpy(p_len, rule_len, (size_t)n * 4, hipMemcpyHostToDevice));
    RNNL_HIP_CHECK(hipMemcpy(p_body, packed.data(), (size_t)n * 4 * RULE_STRIDE, hipMemcpyHostToDevice));
    if (prior)
      RNNL_HIP_CHECK(hipMemcpy(p_prior, prior, (size_t)n * 8, hipMemcpyHostToDevice));
    else
      RNNL_HIP_CHECK(hipMemset(p_prior, 0, (size_t)n * 8));
  }
  RNNL_HIP_CHECK(hipMemset(p_state, 0, std::max<size_t>((size_t)n * 8 * 7, 8)));
  RNNL_HIP_CHECK(hipMemset(p_gs, 0, (size_t)m->ground_blocks * GROUND_PER_E * (size_t)E));
  m->l.rule_off = static_cast<const int32_t *>(p_off);
  m->l.rule_len = static_cast<const int32_t *>(p_len);
  m->l.rule_body = static_cast<const int32_t *>(p_body);
  m->l.prior = static_cast<const double *>(p_prior);
  double *st = static_cast<double *>(p_state);
  m->l.wt = st;
  m->l.am = st + n;
  m->l.av = st + 2 * (size_t)n;
  m->l.at = st + 3 * (size_t)n;
  m->l.H = st + 4 * (size_t)n;
  m->l.val = st + 5 * (size_t)n;
  m->l.op = st + 6 * (size_t)n;
  m->agg = RNNL_MINER_AGG_SUM;  // (agg_depth is 1 again with the fresh MinerLearnDev)
  m->ground_scratch = static_cast<unsigned char *>(p_gs);
  m->chain_scratch = static_cast<unsigned char *>(p_cs);
  return RNNL_OK;
}

int rnnl_miner_set_rules(rnnl_miner m, const int32_t *rule_off, const int32_t *rule_len, const int32_t *rule_body,
                         const double *prior) {
  return set_rules_impl(m, rule_off, rule_len, rule_body, prior, 3, 3, "rnnl_miner_set_rules");
}

int rnnl_miner_set_rules_long(rnnl_miner m, const int32_t *rule_off, const int32_t *rule_len,
                              const int32_t *rule_body, const double *prior) {
  return set_rules_impl(m, rule_off, rule_len, rule_body, prior, RULE_STRIDE, RULE_STRIDE,
                        "rnnl_miner_set_rules_long");
}

int rnnl_miner_ground_count(rnnl_miner m, const int32_t *order, int64_t begin, int64_t count,
                            const int64_t *pair_base, int64_t n_pairs, int64_t *pair_off, uint64_t *counters,
                            void *stream) {
  if (!chunk_args_ok(m, order, begin, count, pair_base, n_pairs, pair_off) || !counters ||
      begin + count > m->d.n) {
    set_error("rnnl_miner_ground_count: bad arguments (set the rules first; begin + count <= n_triples)");
    return RNNL_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  unsigned long long *flags = reinterpret_cast<unsigned long long *>(counters);
  RNNL_HIP_CHECK(hipMemsetAsync(counters, 0, 4 * 8, st));
  if (n_pairs > 0) {
    const unsigned grid = (unsigned)std::min<int64_t>(n_pairs, m->ground_blocks);
    hipLaunchKernelGGL(ground_kernel<false>, dim3(grid), dim3(GB), 0, st, m->d, m->l, order, begin, (int32_t)count,
                       pair_base, n_pairs, pair_off, (int32_t *)nullptr, (uint32_t *)nullptr, (int64_t)0,
                       m->ground_scratch, flags);
  }
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, st, pair_off, n_pairs, flags);
  RNNL_HIP_CHECK(hipGetLastError());
  return RNNL_OK;
}

int rnnl_miner_ground_fill(rnnl_miner m, const int32_t *order, int64_t begin, int64_t count,
                           const int64_t *pair_base, int64_t n_pairs, const int64_t *pair_off, int32_t *ent_dst,
                           uint32_t *ent_cnt, int64_t ent_cap, uint64_t *counters, void *stream) {
  if (!chunk_args_ok(m, order, begin, count, pair_base, n_pairs, pair_off) || !counters || !ent_dst || !ent_cnt ||
      ent_cap < 0 || begin + count > m->d.n) {
    set_error("rnnl_miner_ground_fill: bad arguments");
    return RNNL_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  if (n_pairs > 0) {
    const unsigned grid = (unsigned)std::min<int64_t>(n_pairs, m->ground_blocks);
    hipLaunchKernelGGL(ground_kernel<true>, dim3(grid), dim3(GB), 0, st, m->d, m->l, order, begin, (int32_t)count,
                       pair_base, n_pairs, const_cast<int64_t *>(pair_off), ent_dst, ent_cnt, ent_cap,
                       m->ground_scratch, reinterpret_cast<unsigned long long *>(counters));
  }
  RNNL_HIP_CHECK(hipGetLastError());
  return RNNL_OK;
}

static int chain_launch(rnnl_miner m, bool learn, ChainArgs a, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  a.scratch = m->chain_scratch;
  if (learn)
    hipLaunchKernelGGL(chain_kernel<true>, dim3(m->d.R), dim3(LB), 0, st, m->d, m->l, a);
  else
    hipLaunchKernelGGL(chain_kernel<false>, dim3(m->d.R), dim3(LB), 0, st, m->d, m->l, a);
  RNNL_HIP_CHECK(hipGetLastError());
  return RNNL_OK;
}

int rnnl_miner_learn(rnnl_miner m, const int32_t *order, int64_t begin, int64_t count, const int64_t *pair_base,
                     int64_t n_pairs, const int64_t *pair_off, const int32_t *ent_dst, const uint32_t *ent_cnt,
                     double lr, double wd, double temp, int32_t fast, void *stream) {
  if (!chunk_args_ok(m, order, begin, count, pair_base, n_pairs, pair_off) || !ent_dst || !ent_cnt ||
      begin + count > m->d.n || !(temp != 0) || !std::isfinite(lr) || !std::isfinite(wd) || !std::isfinite(temp)) {
    set_error("rnnl_miner_learn: bad arguments (finite lr / wd, temp != 0)");
    return RNNL_ERR_INVALID;
  }
  ChainArgs a = {};
  a.order = order;
  a.begin = begin;
  a.count = (int32_t)count;
  a.pair_base = pair_base;
  a.pair_off = pair_off;
  a.ent_dst = ent_dst;
  a.ent_cnt = ent_cnt;
  a.lr = lr;
  a.wd = wd;
  a.temp = temp;
  a.log_b1 = std::log(0.9);
  a.log_b2 = std::log(0.999);
  a.fast = fast ? 1 : 0;
  return chain_launch(m, true, a, stream);
}

int rnnl_miner_h_score(rnnl_miner m, const int32_t *order, int64_t begin, int64_t count, const int64_t *pair_base,
                       int64_t n_pairs, const int64_t *pair_off, const int32_t *ent_dst, const uint32_t *ent_cnt,
                       int32_t top_k, double h_temperature, double prior_weight, void *stream) {
  if (!chunk_args_ok(m, order, begin, count, pair_base, n_pairs, pair_off) || !ent_dst || !ent_cnt ||
      begin + count > m->d.n || top_k < 0 || !(h_temperature != 0) || !std::isfinite(h_temperature) ||
      !std::isfinite(prior_weight)) {
    set_error("rnnl_miner_h_score: bad arguments (top_k >= 0, H_temperature != 0)");
    return RNNL_ERR_INVALID;
  }
  ChainArgs a = {};
  a.order = order;
  a.begin = begin;
  a.count = (int32_t)count;
  a.pair_base = pair_base;
  a.pair_off = pair_off;
  a.ent_dst = ent_dst;
  a.ent_cnt = ent_cnt;
  a.top_k = top_k;
  a.h_temp = h_temperature;
  a.prior_weight = prior_weight;
  return chain_launch(m, false, a, stream);
}

int rnnl_miner_read(rnnl_miner m, double *weights, double *H, void *stream) {
  if (!m || !m->l.rule_off) {
    set_error("rnnl_miner_read: set the rules first");
    return RNNL_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  const size_t bytes = (size_t)m->l.n_rules * 8;
  if (bytes && weights) RNNL_HIP_CHECK(hipMemcpyAsync(weights, m->l.wt, bytes, hipMemcpyDeviceToDevice, st));
  if (bytes && H) RNNL_HIP_CHECK(hipMemcpyAsync(H, m->l.H, bytes, hipMemcpyDeviceToDevice, st));
  return RNNL_OK;
}

}  // extern "C"
