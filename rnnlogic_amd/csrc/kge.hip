// RotatE knowledge-graph-embedding training: the sampled-negative step
// (rnnl_kge_sample_negatives, rnnl_kge_rotate_step; include/rnnlogic_hip.h).
//
// A training row i is a positive (h, r, t) and a mode.  Its anchor a is h
// (tail mode) or t (head mode), its answer the other entity, and its query
// q = a o r (tail) or a o conj(r) (head), r = exp(i remb / div).  Row i
// scores its answer and N sampled entities x: s = gamma - sum_d |q_d - x_d|.
//
// The step has no float atomics; every sum has a fixed order:
//   kge_wsum_kernel    W = sum of the row weights (one block, fixed tree).
//   kge_row_kernel     one workgroup per row.  q goes to LDS and to the q
//                      table; sweep 1 gathers the N + 1 candidate rows (one
//                      wave per slot, lanes along d) and leaves the scores in
//                      LDS; the softmax, the loss terms and the coefficient
//                      c = dL/ds of every slot follow; sweep 2 gathers the
//                      rows again with the threads along d and accumulates
//                      dL/dq in slot order, and the chain rule turns it into
//                      the anchor row's gradient and d/d phase.
//   kge_count / scan / fill   a counting sort of the B (N + 2) items
//                      (row, slot) by entity: slots 0..N-1 the negatives, N
//                      the answer, N + 1 the anchor.  Integer atomics only;
//                      the order inside a list is settled by the next kernel.
//   kge_entity_kernel  one workgroup per entity: puts its list into item
//                      order (a bitonic sort in LDS; in place in global
//                      memory for a list of more than 4,096 items), decodes
//                      it into LDS 256 items at a time, then sums the
//                      contributions in that order, eight rows in flight per
//                      thread — c x unit(q_i - x_e) re-formed from the q
//                      table, or the anchor gradient — and writes the
//                      entity's row of d_eemb (zero when the list is empty).
//   kge_remb_kernel    d_remb[r] = sum over the rows of relation r, in row order.
//   kge_loss_kernel    the three losses (one block, fixed tree).
// The candidate rows are gathered twice and the q rows once per item: three
// passes of B N 2D floats.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "grad_fix.h"  // wave_sum, wave_max
#include "internal.h"

namespace rnnl {

constexpr int kKgeMaxAttempts = 64;
constexpr int kKgeLdsFloats = 16384 - 64;  // 64 KiB of dynamic LDS less the reduction slots
constexpr int kKgeRedSlots = 8;

__device__ __forceinline__ uint64_t kge_mix(uint64_t z) {
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}

__device__ __forceinline__ int kge_clamp(int64_t v, int n) {
  return (int)(v < 0 ? 0 : (v >= n ? n - 1 : v));
}

// ----------------------------------------------------------------- sampler
__global__ __launch_bounds__(256) void kge_sample_kernel(
    const int64_t *__restrict__ keys, const int64_t *__restrict__ offs, const int32_t *__restrict__ vals,
    int64_t n_keys, const int64_t *__restrict__ pos, int B, int mode, int E, int N, uint64_t seed, uint64_t step,
    int32_t *__restrict__ neg, int32_t *__restrict__ capped) {
  const int64_t total = (int64_t)B * N;
  const uint64_t k0 = kge_mix(seed + 0x9E3779B97F4A7C15ull * (step + 1ull));
  for (int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; m < total; m += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t row = (uint32_t)(m / N), slot = (uint32_t)(m % N);
    const int64_t key = pos[(int64_t)row * 3 + 1] * (int64_t)E + pos[(int64_t)row * 3 + (mode ? 2 : 0)];
    // the row's true answers: vals[lo, hi), ascending
    int64_t a = 0, b = n_keys;
    while (a < b) {
      const int64_t mid = (a + b) >> 1;
      if (keys[mid] < key) a = mid + 1; else b = mid;
    }
    int64_t lo = 0, hi = 0;
    if (a < n_keys && keys[a] == key) {
      lo = offs[a];
      hi = offs[a + 1];
    }
    const uint64_t k1 = kge_mix(k0 ^ (((uint64_t)row << 32) | (uint64_t)slot));
    int32_t ent = 0;
    bool taken = true;
    for (int attempt = 0; attempt < kKgeMaxAttempts && taken; ++attempt) {
      const uint64_t draw = kge_mix(k1 + 0x9E3779B97F4A7C15ull * ((uint64_t)attempt + 1ull)) >> 32;
      ent = (int32_t)((draw * (uint64_t)E) >> 32);
      int64_t x = lo, y = hi;
      while (x < y) {
        const int64_t mid = (x + y) >> 1;
        if (vals[mid] < ent) x = mid + 1; else y = mid;
      }
      taken = x < hi && vals[x] == ent;
    }
    if (taken) atomicAdd(capped, 1);
    neg[m] = ent;
  }
}

// ------------------------------------------------------------- reductions
// Sum / max over the block in a fixed order (the same value in every thread).
// red: kKgeRedSlots floats of LDS; two barriers.
template <bool MAX>
__device__ __forceinline__ float block_reduce(float v, float *red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  v = MAX ? wave_max(v) : wave_sum(v);
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  float t = red[0];
  for (int w = 1; w < nw; ++w) t = MAX ? fmaxf(t, red[w]) : t + red[w];
  return t;
}

__device__ __forceinline__ float log_sigmoid(float x) { return fminf(x, 0.f) - log1pf(expf(-fabsf(x))); }

__device__ __forceinline__ float sigmoid(float x) {
  const float e = expf(-fabsf(x));
  return x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}

__global__ __launch_bounds__(256) void kge_wsum_kernel(const float *__restrict__ w, int B, float *__restrict__ out) {
  __shared__ float red[kKgeRedSlots];
  float v = 0.f;
  for (int i = threadIdx.x; i < B; i += blockDim.x) v += w ? w[i] : 1.f;
  v = block_reduce<false>(v, red);
  if (threadIdx.x == 0) out[0] = v;
}

// ------------------------------------------------------------ row-major pass
struct KgeStep {
  const float *eemb, *remb;
  const int64_t *pos;
  const int32_t *neg;
  const float *weights;
  int E, R, D, B, N, mode;
  float gamma, alpha, div;
  float *wsum, *qtab, *ganchor, *dphase, *coef, *rowloss;
  float *pos_score, *neg_score;
};

__global__ __launch_bounds__(256) void kge_row_kernel(KgeStep k) {
  extern __shared__ float smem[];
  const int D = k.D, N = k.N, T = blockDim.x;
  float *q = smem;             // 2D: re | im
  float *cs = smem + 2 * D;    // 2D: cos | sin of the applied rotation (sin negated in head mode)
  float *sc = smem + 4 * D;    // N + 1: scores, then coefficients
  float *red = sc + N + 1;     // kKgeRedSlots
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = (T + 63) >> 6;
  const int64_t i = blockIdx.x;
  const int h = kge_clamp(k.pos[i * 3], k.E), r = kge_clamp(k.pos[i * 3 + 1], k.R), t = kge_clamp(k.pos[i * 3 + 2], k.E);
  const int anchor = k.mode ? t : h, answer = k.mode ? h : t;
  const float *__restrict__ eemb = k.eemb;
  const int32_t *__restrict__ negrow = k.neg + i * N;

  const float *arow = eemb + (int64_t)anchor * 2 * D;
  for (int d = tid; d < D; d += T) {
    const float ph = k.remb[(int64_t)r * D + d] / k.div;
    const float c = cosf(ph), s = k.mode ? -sinf(ph) : sinf(ph);
    const float are = arow[d], aim = arow[D + d];
    const float qre = are * c - aim * s, qim = are * s + aim * c;
    q[d] = qre;
    q[D + d] = qim;
    cs[d] = c;
    cs[D + d] = s;
    k.qtab[i * 2 * D + d] = qre;
    k.qtab[i * 2 * D + D + d] = qim;
  }
  __syncthreads();

  // sweep 1: one wave per slot, lanes along d
  for (int j = wave; j <= N; j += nw) {
    const int ent = j < N ? kge_clamp(negrow[j], k.E) : answer;
    const float *x = eemb + (int64_t)ent * 2 * D;
    float acc = 0.f;
#pragma unroll 4
    for (int d = lane; d < D; d += 64) {
      const float re = q[d] - x[d], im = q[D + d] - x[D + d];
      acc += sqrtf(re * re + im * im);
    }
    acc = wave_sum(acc);
    if (lane == 0) sc[j] = k.gamma - acc;
  }
  __syncthreads();

  // softmax over the negatives, the loss terms, dL/ds of every slot
  const float wi = k.weights ? k.weights[i] : 1.f;
  const float cscale = wi / (2.f * k.wsum[0]);
  float mx = -INFINITY;
  for (int j = tid; j < N; j += T) mx = fmaxf(mx, k.alpha * sc[j]);
  mx = block_reduce<true>(mx, red);
  float z = 0.f;
  for (int j = tid; j < N; j += T) z += expf(k.alpha * sc[j] - mx);
  z = block_reduce<false>(z, red);
  float nl = 0.f;
  for (int j = tid; j < N; j += T) {
    const float s = sc[j], p = expf(k.alpha * s - mx) / z;
    nl += p * log_sigmoid(-s);
    k.neg_score[i * N + j] = s;
    const float c = cscale * p * sigmoid(s);
    k.coef[i * (N + 1) + j] = c;
    sc[j] = c;  // (each thread rewrites only the slots it read)
  }
  nl = block_reduce<false>(nl, red);
  if (tid == 0) {
    const float sp = sc[N];
    const float c = -cscale * sigmoid(-sp);
    k.pos_score[i] = sp;
    k.rowloss[i * 2] = wi * log_sigmoid(sp);
    k.rowloss[i * 2 + 1] = wi * nl;
    k.coef[i * (N + 1) + N] = c;
    sc[N] = c;
  }
  __syncthreads();

  // sweep 2: threads along d, the slots in order; dL/dq = - sum_j c_j unit(q - x_j)
  for (int d = tid; d < D; d += T) {
    const float qre = q[d], qim = q[D + d];
    float gre = 0.f, gim = 0.f;
    for (int j0 = 0; j0 <= N; j0 += 4) {
      float xr[4], xi[4], c[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = min(j0 + u, N);
        const int ent = j < N ? kge_clamp(negrow[j], k.E) : answer;
        const float *x = eemb + (int64_t)ent * 2 * D;
        xr[u] = x[d];
        xi[u] = x[D + d];
        c[u] = j0 + u <= N ? sc[j] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float re = qre - xr[u], im = qim - xi[u];
        const float m = sqrtf(re * re + im * im);
        const float g = m > 0.f ? c[u] / m : 0.f;
        gre -= g * re;
        gim -= g * im;
      }
    }
    const float c = cs[d], s = cs[D + d];
    k.ganchor[i * 2 * D + d] = gre * c + gim * s;
    k.ganchor[i * 2 * D + D + d] = gim * c - gre * s;
    const float dth = gim * qre - gre * qim;  // dq / d(applied angle) = i q
    k.dphase[i * D + d] = k.mode ? -dth : dth;
  }
}

// --------------------------------------------------- items sorted by entity
__device__ __forceinline__ int kge_item_entity(const KgeStep &k, int64_t m) {
  const int64_t i = m / (k.N + 2);
  const int slot = (int)(m - i * (k.N + 2));
  if (slot < k.N) return kge_clamp(k.neg[i * k.N + slot], k.E);
  const bool want_t = (slot == k.N) != (k.mode != 0);  // answer in tail mode, anchor in head mode
  return kge_clamp(k.pos[i * 3 + (want_t ? 2 : 0)], k.E);
}

__global__ __launch_bounds__(256) void kge_count_kernel(KgeStep k, int64_t M, int32_t *__restrict__ cnt) {
  for (int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; m < M; m += (int64_t)gridDim.x * blockDim.x)
    atomicAdd(&cnt[kge_item_entity(k, m)], 1);
}

// off[e] = exclusive sum of cnt (cnt and off may not alias); off[E] = total; cur = a copy of off[0..E)
__global__ __launch_bounds__(256) void kge_scan_kernel(const int32_t *__restrict__ cnt, int E, int32_t *__restrict__ off,
                                                       int32_t *__restrict__ cur) {
  __shared__ int part[256];
  const int tid = threadIdx.x;
  const int per = (E + 255) / 256;
  const int a = (int)min((int64_t)tid * per, (int64_t)E), b = (int)min((int64_t)a + per, (int64_t)E);
  int s = 0;
  for (int e = a; e < b; ++e) s += cnt[e];
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int x = 0; x < 256; ++x) {
      const int v = part[x];
      part[x] = run;
      run += v;
    }
    off[E] = run;
  }
  __syncthreads();
  int run = part[tid];
  for (int e = a; e < b; ++e) {
    off[e] = run;
    cur[e] = run;
    run += cnt[e];
  }
}

__global__ __launch_bounds__(256) void kge_fill_kernel(KgeStep k, int64_t M, int32_t *__restrict__ cur,
                                                       int32_t *__restrict__ tmp) {
  for (int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; m < M; m += (int64_t)gridDim.x * blockDim.x) {
    const int p = atomicAdd(&cur[kge_item_entity(k, m)], 1);
    if (p >= 0 && p < M) tmp[p] = (int32_t)m;
  }
}

// ---------------------------------------------------------- entity-major pass
constexpr int kKgeListTile = 256;  // items decoded into LDS at a time
constexpr int kKgeBatch = 8;       // items whose rows a thread has in flight
constexpr int kKgeSortLds = 4096;  // the longest list that is sorted in LDS

// Sorts a[0 .. n) ascending with the whole block: a bitonic network whose comparators all put the smaller value
// at the lower index (each merge starts with a mirror step), so the n .. 2^k - 1 places of the padded network
// would hold +inf and stay put: comparators that reach past n are skipped, and n need not be a power of two.
// a is in LDS or in global memory (written by this block only); one barrier per step, uniform in n.
__device__ __forceinline__ void kge_block_sort(int *a, int n) {
  const int T = blockDim.x, tid = threadIdx.x;
  int64_t n2 = 1;  // (64-bit: a list may pass 2^30 items)
  while (n2 < n) n2 <<= 1;
  for (int64_t k2 = 2; k2 <= n2; k2 <<= 1) {
    const int h = (int)(k2 >> 1);
    for (int p = tid; p < (int)(n2 >> 1); p += T) {  // mirror step: i against the block's k2 - 1 - i
      const int blk = p / h, o = p - blk * h;
      const int64_t lo = blk * k2 + o, hi = blk * k2 + k2 - 1 - o;
      if (hi < n) {
        const int x = a[lo], y = a[hi];
        if (x > y) a[lo] = y, a[hi] = x;
      }
    }
    __syncthreads();
    for (int j = (int)(k2 >> 2); j >= 1; j >>= 1) {
      for (int p = tid; p < (int)(n2 >> 1); p += T) {
        const int64_t lo = (int64_t)(p / j) * 2 * j + (p % j), hi = lo + j;
        if (hi < n) {
          const int x = a[lo], y = a[hi];
          if (x > y) a[lo] = y, a[hi] = x;
        }
      }
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(256) void kge_entity_kernel(KgeStep k, const int32_t *__restrict__ off,
                                                         const int32_t *__restrict__ tmp, int32_t *__restrict__ items,
                                                         float *__restrict__ d_eemb) {
  __shared__ int s_sort[kKgeSortLds];
  __shared__ int s_row[kKgeListTile];   // the item's row; ~row for an anchor item
  __shared__ float s_c[kKgeListTile];   // its coefficient dL/ds
  const int D = k.D, N = k.N, T = blockDim.x, tid = threadIdx.x;
  const int64_t e = blockIdx.x;
  const int lo = off[e], n = off[e + 1] - lo;
  // the list in item order (the fill's atomics left it in any order): sorted in LDS, or in place in `items`
  // when it is longer than the LDS buffer
  if (n <= kKgeSortLds) {
    for (int a = tid; a < n; a += T) s_sort[a] = tmp[lo + a];
    __syncthreads();
    kge_block_sort(s_sort, n);
    for (int a = tid; a < n; a += T) items[lo + a] = s_sort[a];
  } else {
    for (int a = tid; a < n; a += T) items[lo + a] = tmp[lo + a];
    __syncthreads();
    kge_block_sort(items + lo, n);
  }
  __syncthreads();  // (the block reads back its own stores)
  const float *x = k.eemb + e * 2 * D;
  for (int d0 = 0; d0 < D; d0 += T) {  // (uniform: the loop holds barriers)
    const int d = min(d0 + tid, D - 1);
    const float xre = x[d], xim = x[D + d];
    float gre = 0.f, gim = 0.f;
    for (int t0 = 0; t0 < n; t0 += kKgeListTile) {
      const int nt = min(n - t0, kKgeListTile);
      __syncthreads();  // the previous tile's readers are done
      for (int l = tid; l < nt; l += T) {
        const int m = items[lo + t0 + l];
        const int i = m / (N + 2), slot = m - i * (N + 2);
        s_row[l] = slot == N + 1 ? ~i : i;
        s_c[l] = k.coef[(int64_t)i * (N + 1) + min(slot, N)];
      }
      __syncthreads();
      for (int l0 = 0; l0 < nt; l0 += kKgeBatch) {
        float vr[kKgeBatch], vi[kKgeBatch], c[kKgeBatch];
        bool anch[kKgeBatch];
#pragma unroll
        for (int u = 0; u < kKgeBatch; ++u) {
          const int l = min(l0 + u, nt - 1);
          const int code = s_row[l];
          anch[u] = code < 0;
          const float *src = (anch[u] ? k.ganchor : k.qtab) + (int64_t)(anch[u] ? ~code : code) * 2 * D;
          vr[u] = src[d];
          vi[u] = src[D + d];
          c[u] = s_c[l];
          if (l0 + u >= nt) c[u] = 0.f, anch[u] = false;  // (past the tile: adds an exact zero)
        }
#pragma unroll
        for (int u = 0; u < kKgeBatch; ++u) {
          if (anch[u]) {
            gre += vr[u];
            gim += vi[u];
          } else {
            const float re = vr[u] - xre, im = vi[u] - xim;
            const float mod = sqrtf(re * re + im * im);
            const float g = mod > 0.f ? c[u] / mod : 0.f;
            gre += g * re;
            gim += g * im;
          }
        }
      }
    }
    if (d0 + tid < D) {
      d_eemb[e * 2 * D + d] = gre;
      d_eemb[e * 2 * D + D + d] = gim;
    }
  }
}

// d_remb[r] = sum over the rows of relation r, in row order: the block lists its relation's rows among each
// blockDim consecutive ones (ballot prefix, row order kept), then every thread adds those rows' d/d phase at its d.
__global__ __launch_bounds__(256) void kge_remb_kernel(KgeStep k, float *__restrict__ d_remb) {
  __shared__ int s_rows[256];
  __shared__ int s_count[4];
  const int r = blockIdx.x, T = blockDim.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = (T + 63) >> 6;
  const int d = min((int)(blockIdx.y * T) + tid, k.D - 1);
  float acc = 0.f;
  for (int base = 0; base < k.B; base += T) {  // (uniform: the loop holds barriers)
    const int i = base + tid;
    const bool mine = i < k.B && kge_clamp(k.pos[(int64_t)min(i, k.B - 1) * 3 + 1], k.R) == r;
    const uint64_t bal = __ballot(mine);
    __syncthreads();  // the previous list's readers are done
    if (lane == 0) s_count[wave] = (int)__popcll(bal);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < nw; ++w) {
      before += w < wave ? s_count[w] : 0;
      total += s_count[w];
    }
    if (mine) s_rows[before + (int)__popcll(bal & ((1ull << lane) - 1ull))] = i;
    __syncthreads();
    for (int l = 0; l < total; ++l) acc += k.dphase[(int64_t)s_rows[l] * k.D + d];
  }
  if ((int)(blockIdx.y * T) + tid < k.D) d_remb[(int64_t)r * k.D + d] = acc / k.div;
}

__global__ __launch_bounds__(256) void kge_loss_kernel(const float *__restrict__ rowloss, const float *__restrict__ wsum,
                                                       int B, float *__restrict__ losses) {
  __shared__ float red[kKgeRedSlots];
  float p = 0.f, n = 0.f;
  for (int i = threadIdx.x; i < B; i += blockDim.x) {
    p += rowloss[i * 2];
    n += rowloss[i * 2 + 1];
  }
  p = block_reduce<false>(p, red);
  n = block_reduce<false>(n, red);
  if (threadIdx.x == 0) {
    const float lp = -p / wsum[0], ln = -n / wsum[0];
    losses[0] = lp;
    losses[1] = ln;
    losses[2] = (lp + ln) * 0.5f;
  }
}

// ------------------------------------------------------------ scratch layout
struct KgeScratch {
  size_t qtab, ganchor, dphase, coef, rowloss, wsum, cnt, off, cur, tmp, items, total;
};

static size_t kge_up(size_t v) { return (v + 255) & ~(size_t)255; }

static KgeScratch kge_layout(int64_t B, int64_t N, int64_t E, int64_t D) {
  KgeScratch s;
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t here = at;
    at += kge_up(bytes);
    return here;
  };
  const int64_t M = B * (N + 2);
  s.qtab = take((size_t)B * 2 * D * 4);
  s.ganchor = take((size_t)B * 2 * D * 4);
  s.dphase = take((size_t)B * D * 4);
  s.coef = take((size_t)B * (N + 1) * 4);
  s.rowloss = take((size_t)B * 2 * 4);
  s.wsum = take(4);
  s.cnt = take((size_t)(E + 1) * 4);
  s.off = take((size_t)(E + 1) * 4);
  s.cur = take((size_t)(E + 1) * 4);
  s.tmp = take((size_t)M * 4);
  s.items = take((size_t)M * 4);
  s.total = at;
  return s;
}

static bool kge_shape_ok(int32_t B, int32_t N, int32_t E, int32_t D) {
  if (B < 1 || N < 1 || E < 1 || D < 1) return false;
  if ((int64_t)B * ((int64_t)N + 2) > 0x7FFFFFFFll) return false;    // item ids are int32
  if (4 * (int64_t)D + N + 1 > kKgeLdsFloats) return false;          // the row kernel's LDS
  return true;
}

}  // namespace rnnl

using namespace rnnl;

extern "C" int rnnl_kge_sample_negatives(const int64_t *keys, const int64_t *offs, const int32_t *vals,
                                         int64_t n_keys, const int64_t *positives, int32_t n_rows, int32_t mode,
                                         int32_t n_entities, int32_t n_neg, uint64_t seed, int64_t step,
                                         int32_t *neg, int32_t *capped, void *stream) {
  if (!positives || !neg || !capped || n_rows < 1 || n_entities < 1 || n_neg < 1 || n_keys < 0 || step < 0 ||
      (mode != RNNL_KGE_TAIL && mode != RNNL_KGE_HEAD) || (n_keys > 0 && (!keys || !offs || !vals))) {
    set_error("rnnl_kge_sample_negatives: bad arguments");
    return RNNL_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  RNNL_HIP_CHECK(hipMemsetAsync(capped, 0, sizeof(int32_t), st));
  const int64_t total = (int64_t)n_rows * n_neg;
  const int blocks = (int)std::min<int64_t>((total + 255) / 256, 65536);
  hipLaunchKernelGGL(kge_sample_kernel, dim3(blocks), dim3(256), 0, st, keys, offs, vals, n_keys, positives, n_rows,
                     mode, n_entities, n_neg, seed, (uint64_t)step, neg, capped);
  RNNL_HIP_CHECK(hipGetLastError());
  return RNNL_OK;
}

extern "C" int rnnl_kge_rotate_step_scratch(int32_t n_rows, int32_t n_neg, int32_t n_entities, int32_t dim,
                                            size_t *bytes) {
  if (!bytes || !kge_shape_ok(n_rows, n_neg, n_entities, dim)) {
    set_error("rnnl_kge_rotate_step_scratch: bad arguments (sizes must be positive, n_rows (n_neg + 2) < 2^31, "
              "4 dim + n_neg + 1 <= 16320)");
    return RNNL_ERR_INVALID;
  }
  *bytes = kge_layout(n_rows, n_neg, n_entities, dim).total;
  return RNNL_OK;
}

extern "C" int rnnl_kge_rotate_step(const float *eemb, const float *remb, int32_t n_entities, int32_t n_relations,
                                    int32_t dim, float gamma, const int64_t *positives, const int32_t *neg,
                                    const float *weights, int32_t n_rows, int32_t n_neg, int32_t mode, float alpha,
                                    void *scratch, size_t scratch_bytes, float *pos_score, float *neg_score,
                                    float *losses, float *d_eemb, float *d_remb, void *stream) {
  if (!eemb || !remb || !positives || !neg || !scratch || !pos_score || !neg_score || !losses || !d_eemb || !d_remb ||
      n_relations < 1 || (mode != RNNL_KGE_TAIL && mode != RNNL_KGE_HEAD) ||
      !kge_shape_ok(n_rows, n_neg, n_entities, dim) || !(alpha >= 0.f)) {
    set_error("rnnl_kge_rotate_step: bad arguments (pointers non-null, sizes positive, n_rows (n_neg + 2) < 2^31, "
              "4 dim + n_neg + 1 <= 16320, alpha >= 0)");
    return RNNL_ERR_INVALID;
  }
  const KgeScratch L = kge_layout(n_rows, n_neg, n_entities, dim);
  if (scratch_bytes < L.total) {
    set_error("rnnl_kge_rotate_step: scratch smaller than rnnl_kge_rotate_step_scratch");
    return RNNL_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  char *base = (char *)scratch;
  KgeStep k;
  k.eemb = eemb;
  k.remb = remb;
  k.pos = positives;
  k.neg = neg;
  k.weights = weights;
  k.E = n_entities;
  k.R = n_relations;
  k.D = dim;
  k.B = n_rows;
  k.N = n_neg;
  k.mode = mode;
  k.gamma = gamma;
  k.alpha = alpha;
  k.div = (float)(((double)gamma + 2.0) / (double)dim / 3.141592653589793238462643383279);
  k.wsum = (float *)(base + L.wsum);
  k.qtab = (float *)(base + L.qtab);
  k.ganchor = (float *)(base + L.ganchor);
  k.dphase = (float *)(base + L.dphase);
  k.coef = (float *)(base + L.coef);
  k.rowloss = (float *)(base + L.rowloss);
  k.pos_score = pos_score;
  k.neg_score = neg_score;
  int32_t *cnt = (int32_t *)(base + L.cnt), *off = (int32_t *)(base + L.off), *cur = (int32_t *)(base + L.cur);
  int32_t *tmp = (int32_t *)(base + L.tmp), *items = (int32_t *)(base + L.items);
  const int64_t M = (int64_t)n_rows * (n_neg + 2);
  const int threads = dim <= 64 ? 64 : (dim <= 128 ? 128 : 256);  // threads run along d
  const size_t lds = (size_t)(4 * (int64_t)dim + n_neg + 1 + kKgeRedSlots) * sizeof(float);
  const int item_blocks = (int)std::min<int64_t>((M + 255) / 256, 65536);

  RNNL_HIP_CHECK(hipMemsetAsync(cnt, 0, (size_t)(n_entities + 1) * sizeof(int32_t), st));
  hipLaunchKernelGGL(kge_wsum_kernel, dim3(1), dim3(256), 0, st, weights, n_rows, k.wsum);
  hipLaunchKernelGGL(kge_row_kernel, dim3(n_rows), dim3(threads), lds, st, k);
  hipLaunchKernelGGL(kge_count_kernel, dim3(item_blocks), dim3(256), 0, st, k, M, cnt);
  hipLaunchKernelGGL(kge_scan_kernel, dim3(1), dim3(256), 0, st, cnt, n_entities, off, cur);
  hipLaunchKernelGGL(kge_fill_kernel, dim3(item_blocks), dim3(256), 0, st, k, M, cur, tmp);
  hipLaunchKernelGGL(kge_entity_kernel, dim3(n_entities), dim3(threads), 0, st, k, off, tmp, items, d_eemb);
  hipLaunchKernelGGL(kge_remb_kernel, dim3(n_relations, (dim + threads - 1) / threads), dim3(threads), 0, st, k,
                     d_remb);
  hipLaunchKernelGGL(kge_loss_kernel, dim3(1), dim3(256), 0, st, k.rowloss, k.wsum, n_rows, losses);
  RNNL_HIP_CHECK(hipGetLastError());
  return RNNL_OK;
}
