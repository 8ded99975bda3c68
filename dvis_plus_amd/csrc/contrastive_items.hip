// Contrastive item losses of CTVIS's CTCLPlugin (dvis_Plus/ctvis.py:753-769, 817-861), forward and backward — gfx950.
//
// An item i = one anchor row a, P_i positive rows p_k, N_i negative rows n_j, all rows of one (R, C) matrix `src`, given by index
// (CSR lists).  Its slots are numbered positives first: slot s of item i has the global number pos_ptr[i] + neg_ptr[i] + s.
//   reid[i] = logsumexp over all (n_j - p_k) . a and one 0 = softplus(LSE_j(n_j . a) + LSE_k(-p_k . a))      (0 for an empty side)
//   aux[i]  = (sum_k (cos(p_k, a) - 1)^2 + sum_j cos(n_j, a)^2) / (P_i + N_i),  cos(x, a) = x . a / (max(|x|, 1e-12) max(|a|, 1e-12))
//
// Forward, ONE launch, one workgroup of 4 waves per item: a wave takes every fourth slot, reads the slot's row once (at C = 256 one
// 16-byte load per lane) for both its dot with the anchor and its norm, and leaves dot and norm in the saved (slots) arrays; after
// the barrier the 256 threads walk the slots with stride CI_THREADS for the two maxima, then the two exponential sums and the aux
// sum.  Every reduction has a fixed shape (xor butterfly in the wave, the four waves added in wave order): the same bits every call.
//
// Backward, three launches, no atomics, nothing but the (slots) dots / norms and 3 floats per item was saved:
//   1. coef    per slot  alpha_s = g_reid d reid / d dot_s + g_aux e_s / (|x_s| |a|),  beta_s = -g_aux e_s cos_s / |x_s|^2  with
//              e_s = 2 (cos_s - label_s) / (P + N);  per item gamma = -sum_s g_aux e_s cos_s / |a|^2.
//              Then  d / d x_s = alpha_s a + beta_s x_s,   d / d a = sum_s alpha_s x_s + gamma a.
//   2. anchor  one workgroup per item writes its anchor gradient row (n, C) to the workspace: waves take every fourth slot, the four
//              partial rows are added in wave order.
//   3. rows    one wave per source row walks the row's (item, slot) occurrences in order (the transposed lists the host built),
//              then the items it anchors, and writes grad_src[r] ONCE; a row without occurrences gets exactly 0.
// Exact fp32; int64 addressing; every index is clamped into [0, R) on the device as well (the wrapper rejects such lists first).
#include <math.h>

#include "dvis_common.h"

namespace {

constexpr int CI_THREADS = 256;      // threads of a workgroup = slots one pass of the per-item reductions covers
constexpr int CI_WAVES = CI_THREADS / 64;
constexpr float CI_EPS = 1e-12f;     // F.normalize's eps

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
  return v;
}
__device__ __forceinline__ float dot4(const float4 a, const float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

__device__ __forceinline__ int clamp_row(int r, int64_t R) { return (r < 0 || r >= R) ? 0 : r; }

struct Item {
  int arow, P, N, pb, nb;
  int64_t base;
};
__device__ __forceinline__ Item load_item(int i, const int *anchor, const int *pos_ptr, const int *neg_ptr, int64_t R) {
  Item it;
  it.arow = clamp_row(anchor[i], R);
  it.pb = pos_ptr[i], it.nb = neg_ptr[i];
  it.P = max(pos_ptr[i + 1] - it.pb, 0), it.N = max(neg_ptr[i + 1] - it.nb, 0);
  it.base = (int64_t)it.pb + it.nb;
  return it;
}
__device__ __forceinline__ int slot_row(const Item &it, int s, const int *pos_idx, const int *neg_idx, int64_t R) {
  return clamp_row(s < it.P ? pos_idx[it.pb + s] : neg_idx[it.nb + (s - it.P)], R);
}

// sum (or max) of one value per thread over the workgroup, the same value in every thread: butterfly, then the waves in order.
template <bool MAX> __device__ __forceinline__ float block_reduce(float v, float *red) {
  v = MAX ? wave_max(v) : wave_sum(v);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red[wave] = v;
  __syncthreads();
  float r = red[0];
#pragma unroll
  for (int w = 1; w < CI_WAVES; ++w) r = MAX ? fmaxf(r, red[w]) : r + red[w];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(CI_THREADS) void contrastive_items_fwd_kernel(
    const float *__restrict__ src, int64_t R, int C, const int *__restrict__ anchor, const int *__restrict__ pos_ptr,
    const int *__restrict__ pos_idx, const int *__restrict__ neg_ptr, const int *__restrict__ neg_idx, float *__restrict__ reid,
    float *__restrict__ aux, float *dots, float *norms, float *__restrict__ stats) {
  __shared__ float red[CI_WAVES];
  const int i = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const Item it = load_item(i, anchor, pos_ptr, neg_ptr, R);
  const int tot = it.P + it.N;
  const float *a = src + (int64_t)it.arow * C;
  const int c0 = lane * 4;
  float an2 = 0.f;
  for (int c = c0; c < C; c += 256) {
    const float4 a4 = *(const float4 *)(a + c);
    an2 += dot4(a4, a4);
  }
  const float na_raw = sqrtf(wave_sum(an2));          // (every wave: no barrier needed for it)
  const float na = fmaxf(na_raw, CI_EPS);
  const float4 a0 = c0 < C ? *(const float4 *)(a + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
  for (int s = wave; s < tot; s += CI_WAVES) {
    const float *x = src + (int64_t)slot_row(it, s, pos_idx, neg_idx, R) * C;
    float d = 0.f, q = 0.f;
    for (int c = c0; c < C; c += 256) {
      const float4 x4 = *(const float4 *)(x + c);
      const float4 a4 = c == c0 ? a0 : *(const float4 *)(a + c);
      d += dot4(x4, a4);
      q += dot4(x4, x4);
    }
    d = wave_sum(d), q = wave_sum(q);
    if (lane == 0) dots[it.base + s] = d, norms[it.base + s] = sqrtf(q);
  }
  __syncthreads();                                     // the workgroup's own global stores are visible to it behind the barrier
  const float *dp = dots + it.base, *dn = dots + it.base + it.P;
  float mp = -INFINITY, mn = -INFINITY;
  for (int k = threadIdx.x; k < it.P; k += CI_THREADS) mp = fmaxf(mp, -dp[k]);
  for (int j = threadIdx.x; j < it.N; j += CI_THREADS) mn = fmaxf(mn, dn[j]);
  mp = block_reduce<true>(mp, red), mn = block_reduce<true>(mn, red);
  float sp = 0.f, sn = 0.f, sa = 0.f;
  for (int s = threadIdx.x; s < tot; s += CI_THREADS) {
    const float d = dp[s], nx = fmaxf(norms[it.base + s], CI_EPS);
    const float cs = d / (nx * na) - (s < it.P ? 1.f : 0.f);
    sa += cs * cs;
    if (s < it.P) sp += expf(-d - mp);
    else sn += expf(d - mn);
  }
  sp = block_reduce<false>(sp, red), sn = block_reduce<false>(sn, red), sa = block_reduce<false>(sa, red);
  if (threadIdx.x == 0) {
    const float Lp = it.P > 0 ? mp + logf(sp) : -INFINITY, Ln = it.N > 0 ? mn + logf(sn) : -INFINITY;
    float r = 0.f;
    if (it.P > 0 && it.N > 0) {
      const float z = Ln + Lp;
      r = z > 0.f ? z + log1pf(expf(-z)) : log1pf(expf(z));      // (NaN takes the second branch and stays NaN)
    }
    reid[i] = r;
    aux[i] = tot > 0 ? sa / (float)tot : 0.f;
    stats[3 * (int64_t)i] = Ln, stats[3 * (int64_t)i + 1] = Lp, stats[3 * (int64_t)i + 2] = na_raw;
  }
}

__global__ __launch_bounds__(CI_THREADS) void contrastive_items_coef_kernel(
    const int *__restrict__ anchor, const int *__restrict__ pos_ptr, const int *__restrict__ neg_ptr, int64_t R,
    const float *__restrict__ dots, const float *__restrict__ norms, const float *__restrict__ stats,
    const float *__restrict__ grad_reid, const float *__restrict__ grad_aux, float *__restrict__ alpha, float *__restrict__ beta,
    float *__restrict__ gamma) {
  __shared__ float red[CI_WAVES];
  const int i = blockIdx.x;
  const Item it = load_item(i, anchor, pos_ptr, neg_ptr, R);
  const int tot = it.P + it.N;
  const float Ln = stats[3 * (int64_t)i], Lp = stats[3 * (int64_t)i + 1], na_raw = stats[3 * (int64_t)i + 2];
  const float na = fmaxf(na_raw, CI_EPS), gr = grad_reid[i], ga = grad_aux[i];
  float sig = 0.f;
  if (it.P > 0 && it.N > 0) {
    const float z = Ln + Lp, e = expf(-fabsf(z));
    sig = z >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
    if (z != z) sig = z;
  }
  const float inv_tot = tot > 0 ? 1.f / (float)tot : 0.f;
  float gam = 0.f;
  for (int s = threadIdx.x; s < tot; s += CI_THREADS) {
    const bool pos = s < it.P;
    const float d = dots[it.base + s], nx_raw = norms[it.base + s], nx = fmaxf(nx_raw, CI_EPS);
    const float cr = pos ? -sig * expf(-d - Lp) : sig * expf(d - Ln);
    const float cs = d / (nx * na);
    const float e = ga * (2.f * (cs - (pos ? 1.f : 0.f)) * inv_tot);
    alpha[it.base + s] = gr * cr + e / (nx * na);
    beta[it.base + s] = nx_raw > CI_EPS ? -e * cs / (nx * nx) : 0.f;
    gam -= e * cs;
  }
  gam = block_reduce<false>(gam, red);
  if (threadIdx.x == 0) gamma[i] = na_raw > CI_EPS ? gam / (na * na) : 0.f;
}

__global__ __launch_bounds__(CI_THREADS) void contrastive_items_anchor_kernel(
    const float *__restrict__ src, int64_t R, int C, const int *__restrict__ anchor, const int *__restrict__ pos_ptr,
    const int *__restrict__ pos_idx, const int *__restrict__ neg_ptr, const int *__restrict__ neg_idx,
    const float *__restrict__ alpha, const float *__restrict__ gamma, float *__restrict__ ganchor) {
  __shared__ float4 red[CI_WAVES - 1][64];
  const int i = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const Item it = load_item(i, anchor, pos_ptr, neg_ptr, R);
  const int tot = it.P + it.N;
  const float *a = src + (int64_t)it.arow * C;
  const float gam = gamma[i];
  for (int cb = 0; cb < C; cb += 256) {                // (uniform trip count: every thread reaches the barriers)
    const int c = cb + lane * 4;
    const bool live = c < C;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int s = wave; s < tot; s += CI_WAVES) {
      const float al = alpha[it.base + s];
      if (live) {
        const float4 x4 = *(const float4 *)(src + (int64_t)slot_row(it, s, pos_idx, neg_idx, R) * C + c);
        acc.x += al * x4.x, acc.y += al * x4.y, acc.z += al * x4.z, acc.w += al * x4.w;
      }
    }
    if (wave > 0) red[wave - 1][lane] = acc;
    __syncthreads();
    if (wave == 0 && live) {
#pragma unroll
      for (int w = 0; w < CI_WAVES - 1; ++w) {
        const float4 p = red[w][lane];
        acc.x += p.x, acc.y += p.y, acc.z += p.z, acc.w += p.w;
      }
      const float4 a4 = *(const float4 *)(a + c);
      acc.x += gam * a4.x, acc.y += gam * a4.y, acc.z += gam * a4.z, acc.w += gam * a4.w;
      *(float4 *)(ganchor + (int64_t)i * C + c) = acc;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(CI_THREADS) void contrastive_items_rows_kernel(
    const float *__restrict__ src, int64_t R, int C, const int *__restrict__ anchor, int n, const int *__restrict__ row_ptr,
    const int *__restrict__ occ_slot, const int *__restrict__ occ_item, int64_t S, const int *__restrict__ arow_ptr,
    const int *__restrict__ arow_item, const float *__restrict__ alpha, const float *__restrict__ beta,
    const float *__restrict__ ganchor, float *__restrict__ grad_src) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r = (int64_t)blockIdx.x * CI_WAVES + wave;
  if (r >= R) return;                                  // (no barrier in this kernel)
  const int o0 = row_ptr[r], o1 = row_ptr[r + 1], q0 = arow_ptr[r], q1 = arow_ptr[r + 1];
  for (int c = lane * 4; c < C; c += 256) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float bsum = 0.f;
    for (int o = o0; o < o1; ++o) {
      int64_t s = occ_slot[o];
      int it = occ_item[o];
      if (s < 0 || s >= S) s = 0;
      if (it < 0 || it >= n) it = 0;
      const float al = alpha[s];
      bsum += beta[s];
      const float4 a4 = *(const float4 *)(src + (int64_t)clamp_row(anchor[it], R) * C + c);
      acc.x += al * a4.x, acc.y += al * a4.y, acc.z += al * a4.z, acc.w += al * a4.w;
    }
    if (o1 > o0) {                                     // (an unreferenced row stays exactly 0 whatever it holds)
      const float4 x4 = *(const float4 *)(src + r * C + c);
      acc.x += bsum * x4.x, acc.y += bsum * x4.y, acc.z += bsum * x4.z, acc.w += bsum * x4.w;
    }
    for (int q = q0; q < q1; ++q) {
      int it = arow_item[q];
      if (it < 0 || it >= n) it = 0;
      const float4 g4 = *(const float4 *)(ganchor + (int64_t)it * C + c);
      acc.x += g4.x, acc.y += g4.y, acc.z += g4.z, acc.w += g4.w;
    }
    *(float4 *)(grad_src + r * C + c) = acc;
  }
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
bool aligned4(const void *p) { return ((uintptr_t)p & 3) == 0; }

}  // namespace

DVIS_EXPORT int dvis_contrastive_items_tile(void) { return CI_THREADS; }

DVIS_EXPORT int dvis_contrastive_items(const float *src, int64_t R, int C, const int32_t *anchor, const int32_t *pos_ptr,
                                       const int32_t *pos_idx, const int32_t *neg_ptr, const int32_t *neg_idx, int n, int64_t S,
                                       float *reid, float *aux, float *dots, float *norms, float *stats, void *stream) {
  DVIS_REQUIRE(n >= 0 && R >= 1 && R < ((int64_t)1 << 31) && S >= 0 && S < ((int64_t)1 << 31), "contrastive_items: n >= 0, 1 <= R < 2^31 and 0 <= slots < 2^31 are required");
  DVIS_REQUIRE(C >= 4 && C % 4 == 0, "contrastive_items: C %% 4 == 0 is required (got %d)", C);
  if (n == 0) return DVIS_OK;
  DVIS_REQUIRE(src && anchor && pos_ptr && neg_ptr && pos_idx && neg_idx && reid && aux && dots && norms && stats,
               "contrastive_items: null pointer");
  DVIS_REQUIRE(aligned16(src), "contrastive_items: src must be 16-byte aligned");
  DVIS_REQUIRE(aligned4(anchor) && aligned4(pos_ptr) && aligned4(neg_ptr) && aligned4(pos_idx) && aligned4(neg_idx) && aligned4(reid) &&
                   aligned4(aux) && aligned4(dots) && aligned4(norms) && aligned4(stats),
               "contrastive_items: misaligned pointer");
  hipLaunchKernelGGL(contrastive_items_fwd_kernel, dim3((unsigned)n), dim3(CI_THREADS), 0, (hipStream_t)stream, src, R, C, anchor, pos_ptr,
                     pos_idx, neg_ptr, neg_idx, reid, aux, dots, norms, stats);
  return dvis_check_launch("contrastive_items_fwd_kernel");
}

// floats: alpha (S) | beta (S) | gamma (n) | pad to 4 | anchor gradients (n, C)
static int64_t ci_ws_anchor_offset(int n, int64_t S) { return (2 * S + n + 3) / 4 * 4; }

DVIS_EXPORT int64_t dvis_contrastive_items_backward_ws_bytes(int n, int64_t S, int C) {
  if (n < 0 || S < 0 || C < 4 || C % 4) return -1;
  return 4 * (ci_ws_anchor_offset(n, S) + (int64_t)n * C);
}

DVIS_EXPORT int dvis_contrastive_items_backward(const float *src, int64_t R, int C, const int32_t *anchor, const int32_t *pos_ptr,
                                                const int32_t *pos_idx, const int32_t *neg_ptr, const int32_t *neg_idx, int n, int64_t S,
                                                const int32_t *row_ptr, const int32_t *occ_slot, const int32_t *occ_item,
                                                const int32_t *arow_ptr, const int32_t *arow_item, const float *dots,
                                                const float *norms, const float *stats, const float *grad_reid, const float *grad_aux,
                                                float *grad_src, void *ws, void *stream) {
  DVIS_REQUIRE(n >= 0 && R >= 1 && R < ((int64_t)1 << 31) && S >= 0 && S < ((int64_t)1 << 31), "contrastive_items_backward: n >= 0, 1 <= R < 2^31 and 0 <= slots < 2^31 are required");
  DVIS_REQUIRE(C >= 4 && C % 4 == 0, "contrastive_items_backward: C %% 4 == 0 is required (got %d)", C);
  DVIS_REQUIRE(src && grad_src && row_ptr && arow_ptr, "contrastive_items_backward: null pointer");
  DVIS_REQUIRE(n == 0 || (anchor && pos_ptr && neg_ptr && pos_idx && neg_idx && occ_slot && occ_item && arow_item && dots && norms && stats &&
                          grad_reid && grad_aux && ws),
               "contrastive_items_backward: null pointer");
  DVIS_REQUIRE(aligned16(src) && aligned16(grad_src) && (n == 0 || aligned16(ws)), "contrastive_items_backward: src, grad_src and ws must be 16-byte aligned");
  DVIS_REQUIRE(grad_src != src, "contrastive_items_backward: grad_src must not alias src");
  DVIS_REQUIRE(aligned4(anchor) && aligned4(pos_ptr) && aligned4(neg_ptr) && aligned4(pos_idx) && aligned4(neg_idx) && aligned4(row_ptr) &&
                   aligned4(occ_slot) && aligned4(occ_item) && aligned4(arow_ptr) && aligned4(arow_item) && aligned4(dots) && aligned4(norms) &&
                   aligned4(stats) && aligned4(grad_reid) && aligned4(grad_aux),
               "contrastive_items_backward: misaligned pointer");
  const hipStream_t st = (hipStream_t)stream;
  float *alpha = (float *)ws, *beta = alpha + S, *gamma = beta + S, *ganchor = (float *)ws + ci_ws_anchor_offset(n, S);
  if (n > 0) {
    hipLaunchKernelGGL(contrastive_items_coef_kernel, dim3((unsigned)n), dim3(CI_THREADS), 0, st, anchor, pos_ptr, neg_ptr, R, dots, norms,
                       stats, grad_reid, grad_aux, alpha, beta, gamma);
    int rc = dvis_check_launch("contrastive_items_coef_kernel");
    if (rc != DVIS_OK) return rc;
    hipLaunchKernelGGL(contrastive_items_anchor_kernel, dim3((unsigned)n), dim3(CI_THREADS), 0, st, src, R, C, anchor, pos_ptr, pos_idx,
                       neg_ptr, neg_idx, alpha, gamma, ganchor);
    rc = dvis_check_launch("contrastive_items_anchor_kernel");
    if (rc != DVIS_OK) return rc;
  }
  hipLaunchKernelGGL(contrastive_items_rows_kernel, dim3((unsigned)((R + CI_WAVES - 1) / CI_WAVES)), dim3(CI_THREADS), 0, st, src, R, C,
                     anchor, n, row_ptr, occ_slot, occ_item, S, arow_ptr, arow_item, alpha, beta, ganchor, grad_src);
  return dvis_check_launch("contrastive_items_rows_kernel");
}
