// Filtered top-k tail selection with a fully defined order (rnnl_topk_rows).
//
// Per row of the (n_rows x |E|) score matrix: the first k eligible entities by
// score descending, then entity id ascending.  An entity is eligible when its
// mask byte is set (mask NULL: all), its flag byte is set or it is the row's
// `keep` entity (flag NULL: all), and its score is not NaN.
//
// One workgroup per row, no temporary in global memory:
//   1. every float maps to an order-preserving uint32 key (sign fix-up, -0.0
//      folded onto +0.0; eligible keys are >= 0x007FFFFF, 0 marks "not
//      eligible");
//   2. an MSB-first radix select in three passes (11 + 11 + 10 bits, a
//      2,048-bin LDS histogram) finds the k-th largest key T and how many keys
//      == T belong to the result; the row is re-read per pass;
//   3. one more pass appends every key > T through an LDS cursor and the keys
//      == T either all (when all of them belong: the common case of distinct
//      scores) or the first ones in ascending entity order (per step of
//      8 x 256 consecutive entities a ballot prefix and one barrier, until
//      enough are taken);
//   4. the at most 1,024 survivors are sorted in LDS as 64-bit composites
//      (key << 32 | ~entity), descending, and written out with the stored
//      float re-read bit for bit.
// Every pass forms its keys with the same function (load_keys): the loads of
// a step (8 entities per thread: score, mask and flag) are issued together and
// unconditionally, the eligibility is plain arithmetic on their results —
// a short-circuit form makes each load wait for the previous one.
#include <hip/hip_runtime.h>

#include "internal.h"

namespace rnnl {

constexpr int kTopkThreads = 256;
constexpr int kTopkWaves = kTopkThreads / 64;
constexpr int kTopkUnroll = 8;                          // entities per thread and loop step
constexpr int kTopkStep = kTopkUnroll * kTopkThreads;   // entities per loop step
constexpr int kTopkBins = 2048;                         // 11-bit digits
constexpr int kTopkBinsPerThread = kTopkBins / kTopkThreads;

// Order-preserving key of a float: larger float <=> larger key; -0.0 == +0.0.
__device__ __forceinline__ uint32_t float_key(uint32_t u) {
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// The keys of entities base + j * 256 + tid (j < kTopkUnroll) of a row; 0
// where the entity is past the row's end or not eligible.
template <bool MASK, bool FLAG>
__device__ __forceinline__ void load_keys(const float *__restrict__ sr, const uint8_t *__restrict__ mr,
                                          const uint8_t *__restrict__ fr, int64_t keep, int E, int base,
                                          uint32_t (&key)[kTopkUnroll]) {
  uint32_t u[kTopkUnroll];
  uint8_t m[kTopkUnroll], f[kTopkUnroll];
#pragma unroll
  for (int j = 0; j < kTopkUnroll; ++j) {
    const int e = min(base + j * kTopkThreads + (int)threadIdx.x, E - 1);  // (in bounds; masked below)
    u[j] = __float_as_uint(sr[e]);
    m[j] = MASK ? mr[e] : (uint8_t)1;
    f[j] = FLAG ? fr[e] : (uint8_t)1;
  }
#pragma unroll
  for (int j = 0; j < kTopkUnroll; ++j) {
    const int e = base + j * kTopkThreads + (int)threadIdx.x;
    const bool ok = (e < E) & ((u[j] & 0x7FFFFFFFu) <= 0x7F800000u /* not NaN */) & (m[j] != 0) &
                    ((f[j] != 0) | ((int64_t)e == keep));
    key[j] = ok ? float_key(u[j]) : 0u;
  }
}

// Inclusive scan of one int per thread over the 256-thread block; *total
// receives the block sum.  s_wave: kTopkWaves ints; two barriers.
__device__ __forceinline__ int block_scan_incl(int v, int *s_wave, int *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(v, o, 64);
    if (lane >= o) v += up;
  }
  __syncthreads();  // s_wave's previous readers are done
  if (lane == 63) s_wave[wave] = v;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < kTopkWaves; ++w) {
    const int c = s_wave[w];
    before += w < wave ? c : 0;
    all += c;
  }
  *total = all;
  return v + before;
}

// Adds one to hist[bin] for every lane with bin >= 0.  The lanes that share
// the first counted lane's bin add once, together: rows whose scores share
// their upper bits (or are all equal) would otherwise serialise 64 adds to one
// LDS address.
__device__ __forceinline__ void hist_add(int *hist, int bin) {
  const uint64_t act = __ballot(bin >= 0);
  if (act == 0) return;
  const int leader = __ffsll((unsigned long long)act) - 1;
  const int lb = __shfl(bin, leader, 64);
  const uint64_t same = __ballot(bin == lb);
  if (bin == lb) {
    if ((int)(threadIdx.x & 63) == leader) atomicAdd(&hist[lb], (int)__popcll(same));
  } else if (bin >= 0) {
    atomicAdd(&hist[bin], 1);
  }
}

template <bool MASK, bool FLAG>
__global__ __launch_bounds__(kTopkThreads) void topk_rows_kernel(
    const float *__restrict__ score, const uint8_t *__restrict__ mask, const uint8_t *__restrict__ flag,
    const int64_t *__restrict__ keep, int E, int k, int32_t *__restrict__ out_index,
    float *__restrict__ out_score, int32_t *__restrict__ out_valid) {
  __shared__ uint64_t s_buf[RNNL_TOPK_MAX];
  __shared__ int s_hist[kTopkBins];
  __shared__ int s_wave[kTopkWaves];
  __shared__ int s_eq[2][kTopkUnroll][kTopkWaves];
  __shared__ int s_bin, s_bin_count, s_need, s_cursor;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row = blockIdx.x;
  const float *sr = score + row * E;
  const uint8_t *mr = MASK ? mask + row * E : nullptr;
  const uint8_t *fr = FLAG ? flag + row * E : nullptr;
  const int64_t kp = (FLAG && keep) ? keep[row] : -1;

  // ---- radix select: T = the k-th largest key, need = how many keys == T are taken
  uint32_t prefix = 0, known = 0;  // the bits of T found so far / their mask
  int need = k;                    // result slots left for keys with this prefix
  int n_elig = 0;
  bool take_all = false;           // at most k eligible: T = 0, everything eligible is taken
  int n_eq_total = 0;              // keys == T in the row
  for (int pass = 0; pass < 3; ++pass) {
    const int shift = pass == 0 ? 21 : (pass == 1 ? 10 : 0);
    const uint32_t digit = pass == 2 ? 0x3FFu : 0x7FFu;
#pragma unroll
    for (int i = 0; i < kTopkBinsPerThread; ++i) s_hist[i * kTopkThreads + tid] = 0;
    __syncthreads();
    for (int base = 0; base < E; base += kTopkStep) {
      uint32_t key[kTopkUnroll];
      load_keys<MASK, FLAG>(sr, mr, fr, kp, E, base, key);
#pragma unroll
      for (int j = 0; j < kTopkUnroll; ++j) {
        const bool in = key[j] != 0u && (key[j] & known) == prefix;
        hist_add(s_hist, in ? (int)((key[j] >> shift) & digit) : -1);
      }
    }
    __syncthreads();
    // thread t looks at bins 2047 - 8 t downwards: where the descending running count reaches `need`
    int mine[kTopkBinsPerThread], sum = 0;
#pragma unroll
    for (int i = 0; i < kTopkBinsPerThread; ++i) {
      mine[i] = s_hist[kTopkBins - 1 - (kTopkBinsPerThread * tid + i)];
      sum += mine[i];
    }
    int total;
    const int incl = block_scan_incl(sum, s_wave, &total);
    if (pass == 0) {
      n_elig = total;
      if (n_elig <= k) {
        take_all = true;
        break;
      }
    }
    if (incl >= need && incl - sum < need) {
      int run = incl - sum;
      bool found = false;
#pragma unroll
      for (int i = 0; i < kTopkBinsPerThread; ++i) {
        if (!found && run + mine[i] >= need) {
          s_bin = kTopkBins - 1 - (kTopkBinsPerThread * tid + i);
          s_need = need - run;
          s_bin_count = mine[i];
          found = true;
        }
        run += mine[i];
      }
    }
    __syncthreads();
    prefix |= (uint32_t)s_bin << shift;
    known |= digit << shift;
    need = s_need;
    n_eq_total = s_bin_count;  // after the last pass: the keys == T
    // (the next pass rewrites s_bin / s_need only after its own barriers)
  }

  const uint32_t T = take_all ? 0u : prefix;
  const int count = take_all ? n_elig : k;  // survivors
  const int n_above = take_all ? n_elig : k - need;
  const bool eq_all = !take_all && n_eq_total == need;  // every key == T belongs to the result
  const bool ordered = !take_all && !eq_all;

  // ---- gather the survivors
  int n2 = 1;
  while (n2 < count) n2 <<= 1;
  for (int i = tid; i < n2; i += kTopkThreads) s_buf[i] = 0;  // pads sort last
  if (tid == 0) s_cursor = 0;
  __syncthreads();
  // keys >= take_from go through the cursor, in any order (they are sorted below)
  const uint32_t take_from = take_all ? 1u : (eq_all ? T : T + 1u);
  int eq_seen = 0;  // ordered: keys == T in the steps so far (block-uniform)
  for (int base = 0, step = 0; base < E; base += kTopkStep, ++step) {
    uint32_t key[kTopkUnroll];
    load_keys<MASK, FLAG>(sr, mr, fr, kp, E, base, key);
#pragma unroll
    for (int j = 0; j < kTopkUnroll; ++j) {
      if (key[j] >= take_from) {
        const int e = base + j * kTopkThreads + tid;
        const int pos = atomicAdd(&s_cursor, 1);
        if (pos < RNNL_TOPK_MAX) s_buf[pos] = ((uint64_t)key[j] << 32) | (uint32_t)~e;
      }
    }
    if (ordered && eq_seen < need) {
      // the first `need` keys == T in ascending entity order: the step's 8 chunks of 256
      // consecutive entities in turn, a ballot prefix inside each
      uint64_t b[kTopkUnroll];
#pragma unroll
      for (int j = 0; j < kTopkUnroll; ++j) {
        b[j] = __ballot(key[j] == T);
        if (lane == 0) s_eq[step & 1][j][wave] = (int)__popcll(b[j]);
      }
      __syncthreads();  // (one per step: the steps alternate between the two halves of s_eq)
      int before = eq_seen;
#pragma unroll
      for (int j = 0; j < kTopkUnroll; ++j) {
        int mine = before;
#pragma unroll
        for (int w = 0; w < kTopkWaves; ++w) {
          const int n = s_eq[step & 1][j][w];
          mine += w < wave ? n : 0;
          before += n;
        }
        const int rank = mine + (int)__popcll(b[j] & ((1ull << lane) - 1ull));
        if (key[j] == T && rank < need) {
          const int e = base + j * kTopkThreads + tid;
          s_buf[n_above + rank] = ((uint64_t)T << 32) | (uint32_t)~e;
        }
      }
      eq_seen = before;
    }
  }
  __syncthreads();

  // ---- bitonic sort of s_buf[0 .. n2), descending
  for (int size = 2; size <= n2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = tid; i < (n2 >> 1); i += kTopkThreads) {
        const int lo = ((i & ~(stride - 1)) << 1) | (i & (stride - 1));
        const int hi = lo | stride;
        const uint64_t a = s_buf[lo], b = s_buf[hi];
        const bool desc = (lo & size) == 0;
        if (desc ? a < b : a > b) {
          s_buf[lo] = b;
          s_buf[hi] = a;
        }
      }
      __syncthreads();
    }
  }

  // ---- write out
  for (int i = tid; i < k; i += kTopkThreads) {
    int idx = -1;
    float val = -INFINITY;
    if (i < count) {
      idx = (int)~(uint32_t)s_buf[i];
      val = sr[idx];
    }
    out_index[row * k + i] = idx;
    out_score[row * k + i] = val;
  }
  if (tid == 0) out_valid[row] = count;
}

}  // namespace rnnl

using namespace rnnl;

extern "C" int rnnl_topk_rows(const float *score, const uint8_t *mask, const uint8_t *flag, const int64_t *keep,
                              int32_t n_rows, int32_t n_entities, int32_t k, int32_t *out_index, float *out_score,
                              int32_t *out_valid, void *stream) {
  if (!score || !out_index || !out_score || !out_valid || n_rows < 0 || n_entities < 1 || k < 1 ||
      k > RNNL_TOPK_MAX) {
    set_error("rnnl_topk_rows: bad arguments");
    return RNNL_ERR_INVALID;
  }
  if (n_rows == 0) return RNNL_OK;
  auto kernel = mask ? (flag ? topk_rows_kernel<true, true> : topk_rows_kernel<true, false>)
                     : (flag ? topk_rows_kernel<false, true> : topk_rows_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3(n_rows), dim3(kTopkThreads), 0, (hipStream_t)stream, score, mask, flag, keep,
                     n_entities, k, out_index, out_score, out_valid);
  RNNL_HIP_CHECK(hipGetLastError());
  return RNNL_OK;
}
