// Classification of the open-vocabulary (FC-CLIP) heads — gfx950, fp32: the text-classifier epilogue and the geometric ensemble.
//
// ---- dvis_text_class_logits: get_classification_logits (ov_dvis/video_mask2former_transformer_decoder_ov.py:17-36)
//   out[r, k] = max over the templates n of class k of  s * <x_r, text_n> / max(||x_r||, 1e-12),   s = min(exp(logit_scale), 100)
// The products `dots` (R, N) come from the exact-fp32 GEMM the package already has (dvis_gemm_nt on the RAW x); this kernel is its
// epilogue: the row norm of x, the scale and the segmented maximum in one launch, one wave per row.  The reference normalises x,
// scales it, multiplies and takes the maxima in ~2 K + 6 launches; s / ||x|| is positive, so it commutes with the maximum.
// logit_scale is read from device memory (a parameter: no host synchronisation).  seg_ptr (K + 2) int32: prefix sums of
// num_templates over the K classes and the void group.  A NaN product gives a NaN logit (torch's max propagates it too).
// The norm is a fixed-order sum (lane-strided partials, then a butterfly): the same bits on every call.
//
// ---- dvis_ov_ensemble: the geometric ensemble of ov_dvis/meta_architecture_ov.py:603-642, one launch
//   p_in, p_out = softmax of the first K in- / out-vocabulary logits;  a_k = (overlapping_k ? alpha : beta) * (valid_r > 0)
//   c_k = log(p_in_k^(1 - a_k) * p_out_k^(a_k));   p_void = softmax over all K + 1 in-vocabulary logits, at the last one
//   out = log(cat(softmax(c) * (1 - p_void), p_void) + 1e-8)
// evaluated in the LOG domain: c_k = (1 - a_k) (in_k - lse(in)) + a_k (out_k - lse(out)).  The reference forms p ** a in fp32: at
// CLIP's logit scale (cosines x 100) the softmax of a losing class underflows to 0, 0 ** a = 0, log 0 = -inf and, multiplied by
// the 0 of the other branch's category mask, NaN.  Where the reference's value is finite the two forms agree, and after the
// final `+ 1e-8` an underflowed class is log(1e-8) in both; here every output is finite for finite inputs.
// One workgroup of 256 threads per row, K <= 2048 (8 classes per thread in registers), reductions in a fixed order.
#include "dvis_common.h"

namespace {

constexpr int kEnsThreads = 256, kEnsPer = 8;   // K <= 2048

__global__ __launch_bounds__(64) void text_logits_kernel(const float *__restrict__ x, long long x_stride,
                                                         const float *__restrict__ dots, long long dots_stride,
                                                         const float *__restrict__ logit_scale, const int *__restrict__ seg_ptr,
                                                         int D, int N, int K1, float *__restrict__ out) {
  const int r = blockIdx.x, lane = threadIdx.x;
  const float *xr = x + (size_t)r * x_stride;
  float ss = 0.f;
  for (int d = lane; d < D; d += 64) ss = fmaf(xr[d], xr[d], ss);
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) ss += __shfl_xor(ss, m);
  const float scale = fminf(expf(logit_scale[0]), 100.f) / fmaxf(sqrtf(ss), 1e-12f);
  const float *dr = dots + (size_t)r * dots_stride;
  for (int k = lane; k < K1; k += 64) {
    int lo = seg_ptr[k], hi = seg_ptr[k + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > N ? N : hi;          // (the host checks the list; a damaged device copy must not read past the row)
    float m = -INFINITY;
    for (int n = lo; n < hi; ++n) {
      const float v = dr[n];
      m = (v > m || v != v) ? v : m;
    }
    out[(size_t)r * K1 + k] = scale * m;
  }
}

// all-threads reductions over the workgroup in a fixed order: butterfly inside a wave, then the waves' values in wave order
template <bool MAX>
__device__ __forceinline__ float block_reduce(float v, float *lds) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const float o = __shfl_xor(v, m);
    v = MAX ? fmaxf(v, o) : v + o;
  }
  __syncthreads();   // the previous reduction's reads are done
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = lds[0];
#pragma unroll
  for (int w = 1; w < kEnsThreads / 64; ++w) t = MAX ? fmaxf(t, lds[w]) : t + lds[w];
  return t;
}

__global__ __launch_bounds__(kEnsThreads) void ov_ensemble_kernel(const float *__restrict__ in, const float *__restrict__ outv,
                                                                  const float *__restrict__ overlapping,
                                                                  const int *__restrict__ valid, float alpha, float beta, int K,
                                                                  float *__restrict__ out) {
  __shared__ float lds[kEnsThreads / 64];
  const int r = blockIdx.x, tid = threadIdx.x;
  const float *ir = in + (size_t)r * (K + 1), *orow = outv + (size_t)r * (K + 1);
  float vi[kEnsPer], vo[kEnsPer];
  float mi = -INFINITY, mo = -INFINITY;
#pragma unroll
  for (int i = 0; i < kEnsPer; ++i) {
    const int k = tid + i * kEnsThreads;
    vi[i] = k < K ? ir[k] : -INFINITY;
    vo[i] = k < K ? orow[k] : -INFINITY;
    mi = fmaxf(mi, vi[i]);
    mo = fmaxf(mo, vo[i]);
  }
  mi = block_reduce<true>(mi, lds);
  mo = block_reduce<true>(mo, lds);
  float si = 0.f, so = 0.f;
#pragma unroll
  for (int i = 0; i < kEnsPer; ++i) {
    const int k = tid + i * kEnsThreads;
    if (k < K) {
      si += expf(vi[i] - mi);
      so += expf(vo[i] - mo);
    }
  }
  si = block_reduce<false>(si, lds);
  so = block_reduce<false>(so, lds);
  const float lse_i = mi + logf(si), lse_o = mo + logf(so);
  // void: softmax over all K + 1 in-vocabulary logits, at the last one
  const float last = ir[K];
  const float m1 = fmaxf(mi, last);
  const float e_last = expf(last - m1);
  const float p_void = e_last / (si * expf(mi - m1) + e_last);
  const float on = valid ? (valid[r] > 0 ? 1.f : 0.f) : 1.f;
  float c[kEnsPer];
  float mc = -INFINITY;
#pragma unroll
  for (int i = 0; i < kEnsPer; ++i) {
    const int k = tid + i * kEnsThreads;
    c[i] = -INFINITY;
    if (k < K) {
      const float a = (overlapping[k] != 0.f ? alpha : beta) * on;
      c[i] = (1.f - a) * (vi[i] - lse_i) + a * (vo[i] - lse_o);
    }
    mc = fmaxf(mc, c[i]);
  }
  mc = block_reduce<true>(mc, lds);
  float sc = 0.f;
#pragma unroll
  for (int i = 0; i < kEnsPer; ++i) {
    const int k = tid + i * kEnsThreads;
    if (k < K) {
      c[i] = expf(c[i] - mc);
      sc += c[i];
    }
  }
  sc = block_reduce<false>(sc, lds);
  const float keep = 1.f - p_void;
  float *dst = out + (size_t)r * (K + 1);
#pragma unroll
  for (int i = 0; i < kEnsPer; ++i) {
    const int k = tid + i * kEnsThreads;
    if (k < K) dst[k] = logf(c[i] / sc * keep + 1e-8f);
  }
  if (tid == 0) dst[K] = logf(p_void + 1e-8f);
}

}  // namespace

DVIS_EXPORT int dvis_text_class_logits(const float *x, int64_t x_stride, const float *dots, int64_t dots_stride,
                                       const float *logit_scale, const int32_t *seg_ptr, int R, int D, int N, int K1, float *out,
                                       void *stream) {
  DVIS_REQUIRE(R >= 0 && D >= 1 && N >= 1, "text_class_logits: bad sizes (R=%d D=%d N=%d)", R, D, N);
  DVIS_REQUIRE(K1 >= 1 && K1 <= N, "text_class_logits: 1 <= segments <= N text rows: no segment may be empty (got %d segments, N=%d)",
               K1, N);
  if (R == 0) return DVIS_OK;
  DVIS_REQUIRE(x && dots && logit_scale && seg_ptr && out, "text_class_logits: null pointer");
  DVIS_REQUIRE(x_stride >= D && dots_stride >= N, "text_class_logits: row strides shorter than the rows (%lld < D=%d or %lld < N=%d)",
               (long long)x_stride, D, (long long)dots_stride, N);
  hipLaunchKernelGGL(text_logits_kernel, dim3((unsigned)R), dim3(64), 0, (hipStream_t)stream, x, (long long)x_stride, dots,
                     (long long)dots_stride, logit_scale, seg_ptr, D, N, K1, out);
  return dvis_check_launch("text_logits_kernel");
}

DVIS_EXPORT int dvis_ov_ensemble(const float *in_logits, const float *out_logits, const float *overlapping, const int32_t *valid,
                                 float alpha, float beta, int R, int K, float *out, void *stream) {
  DVIS_REQUIRE(R >= 0, "ov_ensemble: R >= 0 (got %d)", R);
  DVIS_REQUIRE(K >= 1 && K <= kEnsThreads * kEnsPer, "ov_ensemble: serves 1 <= K <= %d classes (got K=%d)", kEnsThreads * kEnsPer, K);
  if (R == 0) return DVIS_OK;
  DVIS_REQUIRE(in_logits && out_logits && overlapping && out, "ov_ensemble: null pointer");
  hipLaunchKernelGGL(ov_ensemble_kernel, dim3((unsigned)R), dim3(kEnsThreads), 0, (hipStream_t)stream, in_logits, out_logits,
                     overlapping, valid, alpha, beta, K, out);
  return dvis_check_launch("ov_ensemble_kernel");
}
