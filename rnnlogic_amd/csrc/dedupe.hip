// Row plan of an eval-mode forward for gfx950: an eval row's output depends
// on its (h, r) alone, so the forward runs once per distinct key and the
// result rows are copied to the duplicates (fwd.h Plan).
//
// plan_enqueue: the distinct keys in first-occurrence order.  Every row
// inserts its 64-bit key r |E| + h into an open-addressing table (CAS on the
// key) and takes the minimum of the row indices in its slot (atomicMin): the
// representative of a key is its smallest row whatever the order the rows
// arrive in, so the plan is deterministic.  A scan over the is-representative
// flags (per-block counts, one block over the counts, then the blocks again)
// numbers the representatives; the other rows look their key's number up
// through the representative.
//
// replicate_enqueue: after the forward has written the representatives' rows,
// score[i] = score[row_of[inv[i]]] for every other row and the candidate
// counts of all rows.
#include "fwd.h"

namespace rnnl {

constexpr unsigned long long PLAN_EMPTY = ~0ull;  // the table is filled with 0xff bytes

__global__ __launch_bounds__(PLAN_BS) void plan_insert_kernel(Plan pl) {
  const int i = blockIdx.x * PLAN_BS + threadIdx.x;
  if (i >= pl.nq) return;
  const unsigned long long key = (unsigned long long)pl.all_r[i] * (unsigned long long)pl.E +
                                 (unsigned long long)pl.all_h[i];
  const unsigned int msk = (1u << pl.hbits) - 1u;
  unsigned int slot = (unsigned int)mix64(key) & msk;
  // at most nq distinct keys in >= 2 nq slots: an empty slot is always reached
  for (;;) {
    const unsigned long long prev = atomicCAS(&pl.hkey[slot], PLAN_EMPTY, key);
    if (prev == PLAN_EMPTY || prev == key) break;
    slot = (slot + 1u) & msk;
  }
  atomicMin(&pl.hrow[slot], (unsigned int)i);
  pl.inv[i] = (int32_t)slot;
}

__device__ __forceinline__ bool plan_is_rep(const Plan &pl, int i) {
  return i < pl.nq && pl.hrow[pl.inv[i]] == (unsigned int)i;
}

// blk[b] = representatives among block b's rows
__global__ __launch_bounds__(PLAN_BS) void plan_count_kernel(Plan pl) {
  __shared__ int s_ws[PLAN_BS / 64 + 1];
  int total;
  block_scan<PLAN_BS>(plan_is_rep(pl, blockIdx.x * PLAN_BS + threadIdx.x) ? 1 : 0, s_ws, total);
  if (threadIdx.x == 0) pl.blk[blockIdx.x] = total;
}

// blk -> its exclusive prefix sums (one block), hdr[0] = nu
__global__ __launch_bounds__(1024) void plan_scan_kernel(Plan pl, int nb) {
  __shared__ int s_ws[1024 / 64 + 1];
  int carry = 0;
  for (int b0 = 0; b0 < nb; b0 += 1024) {
    const int b = b0 + (int)threadIdx.x;
    int total;
    const int x = b < nb ? pl.blk[b] : 0;
    const int ex = block_scan<1024>(x, s_ws, total);
    if (b < nb) pl.blk[b] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) pl.hdr[0] = (unsigned int)carry;
}

// the representatives' compact rows; their numbers by row in the (not yet
// used) compact candidate counts
__global__ __launch_bounds__(PLAN_BS) void plan_fill_kernel(Plan pl) {
  __shared__ int s_ws[PLAN_BS / 64 + 1];
  const int i = blockIdx.x * PLAN_BS + threadIdx.x;
  const bool rep = plan_is_rep(pl, i);
  int total;
  const int u = pl.blk[blockIdx.x] + block_scan<PLAN_BS>(rep ? 1 : 0, s_ws, total);
  if (rep) {  // u <= i < nq
    pl.row_of[u] = i;
    pl.uh[u] = pl.all_h[i];
    pl.ur[u] = pl.all_r[i];
    pl.n_cand[i] = u;
  }
}

// inv: a row's slot -> its key's representative -> that row's number
__global__ __launch_bounds__(PLAN_BS) void plan_inverse_kernel(Plan pl) {
  const int i = blockIdx.x * PLAN_BS + threadIdx.x;
  if (i < pl.nq) pl.inv[i] = pl.n_cand[pl.hrow[pl.inv[i]]];
}

void plan_enqueue(const Plan &pl, hipStream_t st) {
  const unsigned nb = (unsigned)((pl.nq + PLAN_BS - 1) / PLAN_BS);
  (void)hipMemsetAsync(pl.hkey, 0xff, (size_t)8 << pl.hbits, st);
  (void)hipMemsetAsync(pl.hrow, 0xff, (size_t)4 << pl.hbits, st);
  hipLaunchKernelGGL(plan_insert_kernel, dim3(nb), dim3(PLAN_BS), 0, st, pl);
  hipLaunchKernelGGL(plan_count_kernel, dim3(nb), dim3(PLAN_BS), 0, st, pl);
  hipLaunchKernelGGL(plan_scan_kernel, dim3(1), dim3(1024), 0, st, pl, (int)nb);
  hipLaunchKernelGGL(plan_fill_kernel, dim3(nb), dim3(PLAN_BS), 0, st, pl);
  hipLaunchKernelGGL(plan_inverse_kernel, dim3(nb), dim3(PLAN_BS), 0, st, pl);
}

// One block per (row, segment of REP_SEG entities).  The rows start at
// multiples of 4 |E| bytes — dword alignment only, and a source and its copy
// differ in their 16-byte phase — so the copy is in dwords, 256 contiguous
// bytes per wave and instruction, REP_SEG / 256 loads in flight per lane.
constexpr int REP_SEG = 4096;
__global__ __launch_bounds__(256) void replicate_kernel(Plan pl, int E, float *score,
                                                        int32_t *__restrict__ n_cand) {
  const int i = blockIdx.x;
  const int u = pl.inv[i];
  const int src = pl.row_of[u];
  if (blockIdx.y == 0 && threadIdx.x == 0) n_cand[i] = pl.n_cand[u];
  if (src == i) return;  // block-uniform
  const float *__restrict__ s = score + (int64_t)src * E;
  float *__restrict__ d = score + (int64_t)i * E;
  const int e0 = blockIdx.y * REP_SEG + (int)threadIdx.x;
  float v[REP_SEG / 256];
#pragma unroll
  for (int k = 0; k < REP_SEG / 256; ++k) {
    const int e = e0 + k * 256;
    v[k] = e < E ? s[e] : 0.f;
  }
#pragma unroll
  for (int k = 0; k < REP_SEG / 256; ++k) {
    const int e = e0 + k * 256;
    if (e < E) d[e] = v[k];
  }
}

void replicate_enqueue(const Plan &pl, int E, float *score, int32_t *n_cand, hipStream_t st) {
  hipLaunchKernelGGL(replicate_kernel, dim3((unsigned)pl.nq, (unsigned)((E + REP_SEG - 1) / REP_SEG)), dim3(256), 0,
                     st, pl, E, score, n_cand);
}

}  // namespace rnnl
