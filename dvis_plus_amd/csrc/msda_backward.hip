// Multi-scale deformable attention, backward — gfx950.
//
// Replaces ms_deformable_col2im_cuda and its 7 kernel variants
// (ops/src/cuda/ms_deform_im2col_cuda.cuh:306-925, host :961-1331; wrapper ms_deform_attn_cuda.cu:88-158).
// The reference picks a kernel by D (blocksize-aware / dynamic-smem / multi-block / global-atomic) because it
// assigns one thread per channel and reduces grad_loc / grad_w through shared memory.  Here a GROUP of 32 or
// 64 lanes (half / full wavefront) owns one (n, q, m) pair for every D: lanes stride over channels, the three
// scalar gradients of a sample are reduced with wavefront shuffles (no LDS, no __syncthreads), and grad_value
// gets lane-contiguous atomics (one 128-byte line per corner for D = 32).
//   d out / d w      = sum_c go[c] * bilinear(v)[c]
//   d out / d loc_x  = W * w * sum_c go[c] * (hh (v2 - v1) + lh (v4 - v3))      (corners outside the map = 0)
//   d out / d loc_y  = H * w * sum_c go[c] * (hw (v3 - v1) + lw (v4 - v2))
//   d out / d v_k[c] = go[c] * w * corner_weight_k
// Measured (round 4, tools/msda_bwd_time.py, profiles/r04_msda_bwd_time.txt): 695 us per 720p frame-layer (S = Lq = 19 320,
// M = 8, D = 32) = 0.019 of the HBM roofline on 103.9 MB of algorithmic traffic, 935 us at the ViT-L extractor shape; the forward
// takes 41 / 56 us.  The 237 M scalar adds per frame-layer are 7.4 M 128-byte-line atomic transactions (a 32-lane group hits one
// line per instruction) and that is the bound: ~10.6 G line-atomics/s.  A lane-owned 16-byte form (8 lanes x 4 channels per
// pair, as in the forward) was built and is 4x SLOWER (2808 us): every atomic instruction then touches a quarter of each
// line, i.e. four times as many L2 transactions.  What would help is fewer transactions — grad_value accumulated on chip
// per query tile before one atomic per line — not wider lanes.
#include "dvis_common.h"

#include <algorithm>

namespace {

template <typename A, int GS>
__device__ __forceinline__ A group_sum(A v) {
#pragma unroll
  for (int o = GS / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, GS);
  return v;
}

// DET (fp32 only): grad_value is accumulated in 64-bit FIXED POINT — every contribution is rounded to a multiple of 2^-e on its own
// (e from the launch's max |grad_out| x max |weight|: 42 bits below the largest possible contribution, 20 bits of headroom above it for
// colliding contributions; the resolution is ABSOLUTE — 2^-42 of that bound — not relative to a cell's own sum)
// and integer addition is associative, so the sum does not depend on the order the atomics land in: two runs give the same bits,
// which float atomics do not (the reference's backward is not reproducible either: ms_deform_im2col_cuda.cuh atomicAdd).
struct DetArgs {
  unsigned long long *acc;           // N * S * M * D accumulators (zeroed by the host function)
  const unsigned *absmax;            // bit patterns of max |grad_out|, max |attn weight|
};

__device__ __forceinline__ float det_scale(const unsigned *absmax) {
  const float bound = __uint_as_float(absmax[0]) * __uint_as_float(absmax[1]);
  int ex = 0;
  frexpf(bound > 0.f && bound < 3.0e38f ? bound : 1.f, &ex);      // bound < 2^ex
  return ldexpf(1.f, 42 - ex);
}

template <typename T, int GS, bool DET = false>
__global__ __launch_bounds__(256) void msda_bwd_kernel(
    const T *__restrict__ value, const int64_t *__restrict__ shapes, const int64_t *__restrict__ level_start,
    const T *__restrict__ loc, const T *__restrict__ w, const T *__restrict__ grad_out, size_t npairs, int S, int M,
    int D, int L, int Lq, int P, T *__restrict__ grad_value, T *__restrict__ grad_loc, T *__restrict__ grad_w,
    DetArgs det = {}) {
  constexpr int GPB = 256 / GS;
  float dscale = 0.f;
  if constexpr (DET) dscale = det_scale(det.absmax);
  const int gl = threadIdx.x % GS;
  const size_t pix = (size_t)M * D;
  for (size_t pair = (size_t)blockIdx.x * GPB + threadIdx.x / GS; pair < npairs; pair += (size_t)gridDim.x * GPB) {
    const int m = (int)(pair % M);
    const size_t n = pair / ((size_t)Lq * M);
    const T *go = grad_out + pair * D;
    for (int l = 0; l < L; ++l) {
      const int H = (int)shapes[2 * l], W = (int)shapes[2 * l + 1];
      const size_t lbase = ((n * S + (size_t)level_start[l]) * M + m) * D;
      for (int p = 0; p < P; ++p) {
        const size_t s = pair * (size_t)(L * P) + (size_t)l * P + p;
        const T x = loc[2 * s], y = loc[2 * s + 1], aw = w[s];
        const T h_im = y * (T)H - (T)0.5, w_im = x * (T)W - (T)0.5;
        T gw = 0, gx = 0, gy = 0;
        if (h_im > (T)-1 && w_im > (T)-1 && h_im < (T)H && w_im < (T)W) {   // group-uniform branch
          const T hf = floor(h_im), wf = floor(w_im);
          const int h0 = (int)hf, w0 = (int)wf;
          const T lh = h_im - hf, lw = w_im - wf, hh = (T)1 - lh, hw = (T)1 - lw;
          const bool ok1 = h0 >= 0 && w0 >= 0, ok2 = h0 >= 0 && w0 + 1 <= W - 1;
          const bool ok3 = h0 + 1 <= H - 1 && w0 >= 0, ok4 = h0 + 1 <= H - 1 && w0 + 1 <= W - 1;
          const long long i1 = (long long)lbase + ((long long)h0 * W + w0) * (long long)pix;
          const long long i2 = i1 + (long long)pix, i3 = i1 + (long long)W * (long long)pix, i4 = i3 + (long long)pix;
          for (int c = gl; c < D; c += GS) {
            const T a = ok1 ? value[i1 + c] : (T)0, b = ok2 ? value[i2 + c] : (T)0;
            const T e = ok3 ? value[i3 + c] : (T)0, f = ok4 ? value[i4 + c] : (T)0;
            const T g = go[c];
            gw += g * (hh * hw * a + hh * lw * b + lh * hw * e + lh * lw * f);
            gx += g * (hh * (b - a) + lh * (f - e));
            gy += g * (hw * (e - a) + lw * (f - b));
            const T ga = g * aw;
            if constexpr (DET) {
              auto add = [&](long long idx, float v) {
                atomicAdd(det.acc + idx, (unsigned long long)__float2ll_rn(v * dscale));      // two's complement: signed sums wrap correctly
              };
              if (ok1) add(i1 + c, (float)(ga * hh * hw));
              if (ok2) add(i2 + c, (float)(ga * hh * lw));
              if (ok3) add(i3 + c, (float)(ga * lh * hw));
              if (ok4) add(i4 + c, (float)(ga * lh * lw));
            } else {
              if (ok1) atomicAdd(grad_value + i1 + c, ga * hh * hw);
              if (ok2) atomicAdd(grad_value + i2 + c, ga * hh * lw);
              if (ok3) atomicAdd(grad_value + i3 + c, ga * lh * hw);
              if (ok4) atomicAdd(grad_value + i4 + c, ga * lh * lw);
            }
          }
        }
        gw = group_sum<T, GS>(gw);
        gx = group_sum<T, GS>(gx);
        gy = group_sum<T, GS>(gy);
        if (gl == 0) {
          grad_w[s] = gw;
          grad_loc[2 * s] = gx * aw * (T)W;
          grad_loc[2 * s + 1] = gy * aw * (T)H;
        }
      }
    }
  }
}

template <typename T>
int launch_bwd(const void *value, const int64_t *shapes, const int64_t *ls, const void *loc, const void *w,
               const void *go, int N, int S, int M, int D, int L, int Lq, int P, void *gv, void *gl, void *gw,
               hipStream_t st) {
  const size_t npairs = (size_t)N * Lq * M;
  if (D <= 32) {
    const size_t blocks = (npairs + 7) / 8;
    hipLaunchKernelGGL((msda_bwd_kernel<T, 32>), dim3((unsigned)(blocks > 262144 ? 262144 : blocks)), dim3(256), 0, st,
                       (const T *)value, shapes, ls, (const T *)loc, (const T *)w, (const T *)go, npairs, S, M, D, L,
                       Lq, P, (T *)gv, (T *)gl, (T *)gw);
  } else {
    const size_t blocks = (npairs + 3) / 4;
    hipLaunchKernelGGL((msda_bwd_kernel<T, 64>), dim3((unsigned)(blocks > 262144 ? 262144 : blocks)), dim3(256), 0, st,
                       (const T *)value, shapes, ls, (const T *)loc, (const T *)w, (const T *)go, npairs, S, M, D, L,
                       Lq, P, (T *)gv, (T *)gl, (T *)gw);
  }
  return dvis_check_launch("msda_bwd_kernel");
}

__global__ __launch_bounds__(256) void absmax_kernel(const float *__restrict__ x, size_t n, unsigned *__restrict__ out) {
  // fmaxf DROPS a NaN operand; the fixed-point form must see it (det_finish_kernel hands back NaN then): a NaN-keeping maximum
  auto nanmax = [](float a, float b) { return (a != a || b != b) ? __builtin_nanf("") : fmaxf(a, b); };
  float m = 0.f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) m = nanmax(m, fabsf(x[i]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = nanmax(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0) atomicMax(out, __float_as_uint(m));      // non-negative floats order like their bit patterns; NaN -> 0x7fc..: the largest
}

__global__ __launch_bounds__(256) void det_finish_kernel(const unsigned long long *__restrict__ acc, const unsigned *__restrict__ absmax,
                                                         float *__restrict__ grad_value, size_t n) {
  const float inv = 1.f / det_scale(absmax);
  // A NaN / Inf in grad_output or the weights (absmax keeps the largest BIT PATTERN: NaN > Inf > finite) has no fixed-point image:
  // the float-atomic form and the reference would hand back non-finite gradients, so does this one — a diverged training run must
  // not be hidden by torch.use_deterministic_algorithms(True).  Headroom: a cell's sum may reach 2^20 x the bound
  // (max |grad_out| x max |weight|) before the 64-bit accumulator wraps — 19 320 x 8 x 12 x 4 = 7.4 M < 2^23 colliding corner
  // contributions of weight <= 1 each would need every sample of a frame-layer to hit ONE pixel with full weight to get there.
  const float bound = __uint_as_float(absmax[0]) * __uint_as_float(absmax[1]);
  const bool finite = bound < 3.0e38f;      // false for Inf and NaN
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
    grad_value[i] = finite ? (float)((double)(long long)acc[i] * (double)inv) : __builtin_nanf("");
}


// ---- backward of dvis_msda_fused_forward (fp32) ------------------------------------------------------------------------------------
// Inputs are the forward's own: the RAW offset / logit rows and the reference points.  Per (n, q, m) the group recomputes what
// msda_fwd_tile<FUSED> computes — a = exp(logit - max) / sum over the L*P logits (max and sum in the forward's ascending order) and
// loc = ref + off / (W_l, H_l) — so neither sampling_locations nor the softmaxed weights (nor their gradients) ever exist in
// memory.  Lane j < L*P of the group owns sample j: it holds a_j and loc_j, the sample loop broadcasts them with a shuffle, and
// after a sample's three group sums lane j keeps t_j = sum_c go[c] bilinear_j[c], gx_j, gy_j (the corner-difference sums above).
//   grad_logit_j  = a_j (t_j - sum_k a_k t_k)          the inner sum in ascending k, one fixed order
//   grad_offset_j = (a_j gx_j, a_j gy_j)               d h_im / d loc = W_l and d loc / d off = 1 / W_l cancel analytically:
//                                                      NEITHER factor is multiplied in (msda_bwd_kernel's `* (T)W` has no image here)
//   grad_value    : the same corner contributions as msda_bwd_kernel, float atomics or (DET) the 64-bit fixed point.
// D == GS (one channel per lane), no LDS, no barrier.  The per-sample arithmetic is written in msda_bwd_kernel's operation order;
// that kernel is left alone (its bits are pinned by tests), so the few lines are repeated instead of shared.
template <int GS, int L, int P, bool DET>
__global__ __launch_bounds__(256) void msda_fused_bwd_kernel(
    const float *__restrict__ value, const int64_t *__restrict__ shapes, const int64_t *__restrict__ level_start,
    const float *__restrict__ refp, int nref, const float *__restrict__ offsets, int64_t off_stride,
    const float *__restrict__ logits, int64_t logit_stride, const float *__restrict__ grad_out, size_t npairs, int S, int M,
    int Lq, float *__restrict__ grad_value, float *__restrict__ grad_off, float *__restrict__ grad_logit, DetArgs det = {},
    unsigned *__restrict__ weight_absmax = nullptr) {
  constexpr int GPB = 256 / GS, LP = L * P, D = GS;
  static_assert(LP <= GS && LP % 4 == 0, "one lane per sample; logit rows are read 16 bytes at a time");
  float dscale = 0.f;
  if constexpr (DET) dscale = det_scale(det.absmax);
  const int gl = threadIdx.x % GS;
  const size_t pix = (size_t)M * D;
  const bool mine = gl < LP;                       // this lane owns sample gl of its pair
  const int ml = mine ? gl / P : 0;
  const int Hm = (int)shapes[2 * ml], Wm = (int)shapes[2 * ml + 1];
  for (size_t pair = (size_t)blockIdx.x * GPB + threadIdx.x / GS; pair < npairs; pair += (size_t)gridDim.x * GPB) {
    const int m = (int)(pair % M);
    const size_t row = pair / M;                   // n * Lq + q
    const size_t n = row / (size_t)Lq, q = row - n * (size_t)Lq;
    const float *lrow = logits + row * (size_t)logit_stride + (size_t)m * LP;
    float lg[LP];
#pragma unroll
    for (int k = 0; k < LP / 4; ++k) {
      const float4 v = *reinterpret_cast<const float4 *>(lrow + 4 * k);
      lg[4 * k] = v.x; lg[4 * k + 1] = v.y; lg[4 * k + 2] = v.z; lg[4 * k + 3] = v.w;
    }
    float mx = lg[0];
#pragma unroll
    for (int s = 1; s < LP; ++s) mx = fmaxf(mx, lg[s]);
    float sum = 0.f;
#pragma unroll
    for (int s = 0; s < LP; ++s) sum += expf(lg[s] - mx);
    if constexpr (DET) {
      // A NaN or +Inf logit makes every weight of the pair NaN (the sum is NaN), and a NaN contribution has no fixed-point image
      // (__float2ll_rn gives 0).  The unfused form's second absmax pass would see it; here the pair raises the weights' maximum to
      // NaN itself, and det_finish_kernel hands back NaN grad_value.  (Blocks that read the scale before or after differ only in
      // values that are then discarded.)
      if (gl == 0 && !(sum == sum)) atomicMax(weight_absmax, 0x7fc00000u);
    }
    float a = 0.f, lx = 0.f, ly = 0.f;
    if (mine) {
      a = expf(lrow[gl] - mx) / sum;
      const float2 o = *reinterpret_cast<const float2 *>(offsets + row * (size_t)off_stride + (size_t)m * (LP * 2) + 2 * gl);
      const float2 r = *reinterpret_cast<const float2 *>(refp + (((nref == 1 ? 0 : n) * (size_t)Lq + q) * L + ml) * 2);
      lx = r.x + o.x / (float)Wm;
      ly = r.y + o.y / (float)Hm;
    }
    const float g = grad_out[pair * D + gl];
    float tm = 0.f, gxm = 0.f, gym = 0.f;
#pragma unroll 1
    for (int l = 0; l < L; ++l) {
      const int H = (int)shapes[2 * l], W = (int)shapes[2 * l + 1];
      const size_t lbase = ((n * S + (size_t)level_start[l]) * M + m) * D;
#pragma unroll
      for (int p = 0; p < P; ++p) {
        const int j = l * P + p;
        const float x = __shfl(lx, j, GS), y = __shfl(ly, j, GS), aw = __shfl(a, j, GS);
        const float h_im = y * (float)H - 0.5f, w_im = x * (float)W - 0.5f;
        float gw = 0.f, gx = 0.f, gy = 0.f;
        if (h_im > -1.f && w_im > -1.f && h_im < (float)H && w_im < (float)W) {   // group-uniform branch
          const float hf = floorf(h_im), wf = floorf(w_im);
          const int h0 = (int)hf, w0 = (int)wf;
          const float lh = h_im - hf, lw = w_im - wf, hh = 1.f - lh, hw = 1.f - lw;
          const bool ok1 = h0 >= 0 && w0 >= 0, ok2 = h0 >= 0 && w0 + 1 <= W - 1;
          const bool ok3 = h0 + 1 <= H - 1 && w0 >= 0, ok4 = h0 + 1 <= H - 1 && w0 + 1 <= W - 1;
          const long long i1 = (long long)lbase + ((long long)h0 * W + w0) * (long long)pix + gl;
          const long long i2 = i1 + (long long)pix, i3 = i1 + (long long)W * (long long)pix, i4 = i3 + (long long)pix;
          const float va = ok1 ? value[i1] : 0.f, vb = ok2 ? value[i2] : 0.f;
          const float ve = ok3 ? value[i3] : 0.f, vf = ok4 ? value[i4] : 0.f;
          gw = g * (hh * hw * va + hh * lw * vb + lh * hw * ve + lh * lw * vf);
          gx = g * (hh * (vb - va) + lh * (vf - ve));
          gy = g * (hw * (ve - va) + lw * (vf - vb));
          const float ga = g * aw;
          if constexpr (DET) {
            auto add = [&](long long idx, float v) {
              atomicAdd(det.acc + idx, (unsigned long long)__float2ll_rn(v * dscale));      // two's complement: signed sums wrap correctly
            };
            if (ok1) add(i1, ga * hh * hw);
            if (ok2) add(i2, ga * hh * lw);
            if (ok3) add(i3, ga * lh * hw);
            if (ok4) add(i4, ga * lh * lw);
          } else {
            if (ok1) atomicAdd(grad_value + i1, ga * hh * hw);
            if (ok2) atomicAdd(grad_value + i2, ga * hh * lw);
            if (ok3) atomicAdd(grad_value + i3, ga * lh * hw);
            if (ok4) atomicAdd(grad_value + i4, ga * lh * lw);
          }
        }
        gw = group_sum<float, GS>(gw);
        gx = group_sum<float, GS>(gx);
        gy = group_sum<float, GS>(gy);
        if (gl == j) { tm = gw; gxm = gx; gym = gy; }
      }
    }
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < LP; ++k) dot = __builtin_fmaf(__shfl(a, k, GS), __shfl(tm, k, GS), dot);
    if (mine) {
      const size_t s = pair * (size_t)LP + gl;      // contiguous (N * Lq, M * L * P [* 2]) outputs
      grad_logit[s] = a * (tm - dot);
      *reinterpret_cast<float2 *>(grad_off + 2 * s) = make_float2(a * gxm, a * gym);
    }
  }
}

// the fixed-point scale of the fused backward comes from max |grad_out| alone: a finite softmaxed weight is <= 1 (a non-finite one
// is reported by the kernel itself)
__global__ void det_unit_weight_kernel(unsigned *__restrict__ absmax) { absmax[1] = __float_as_uint(1.f); }

template <int GS, int L, int P>
int launch_fused_bwd(const float *value, const int64_t *shapes, const int64_t *ls, const float *ref, int nref, const float *off,
                     int64_t off_stride, const float *lg, int64_t lg_stride, const float *go, size_t npairs, int S, int M, int Lq,
                     float *gv, float *goff, float *glg, const DetArgs *det, hipStream_t st) {
  const size_t blocks = (npairs + 256 / GS - 1) / (256 / GS);
  const dim3 grid((unsigned)(blocks > 262144 ? 262144 : blocks));
  if (det)
    hipLaunchKernelGGL((msda_fused_bwd_kernel<GS, L, P, true>), grid, dim3(256), 0, st, value, shapes, ls, ref, nref, off, off_stride,
                       lg, lg_stride, go, npairs, S, M, Lq, gv, goff, glg, *det, const_cast<unsigned *>(det->absmax) + 1);
  else
    hipLaunchKernelGGL((msda_fused_bwd_kernel<GS, L, P, false>), grid, dim3(256), 0, st, value, shapes, ls, ref, nref, off, off_stride,
                       lg, lg_stride, go, npairs, S, M, Lq, gv, goff, glg, DetArgs{});
  return dvis_check_launch("msda_fused_bwd_kernel");
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

DVIS_EXPORT int64_t dvis_msda_backward_det_ws_bytes(int N, int S, int M, int D) {
  if (N < 0 || S <= 0 || M <= 0 || D <= 0) return -1;
  return (int64_t)N * S * M * D * 8 + 16;
}

// fp32 backward with a run-to-run REPRODUCIBLE grad_value (see DetArgs); grad_loc / grad_w are per-sample reductions in a fixed
// order in both forms.  ws: dvis_msda_backward_det_ws_bytes bytes, 16-byte aligned.
DVIS_EXPORT int dvis_msda_backward_det(const float *value, const int64_t *shapes, const int64_t *level_start, const float *loc,
                                       const float *w, const float *grad_out, int N, int S, int M, int D, int L, int Lq, int P,
                                       float *grad_value, float *grad_loc, float *grad_w, void *ws, void *stream) {
  DVIS_REQUIRE(N >= 0 && S > 0 && M > 0 && D > 0 && L > 0 && Lq >= 0 && P > 0, "msda_backward_det: bad sizes");
  DVIS_REQUIRE(value && shapes && level_start && loc && w && grad_out && grad_value && grad_loc && grad_w && ws &&
                   (uintptr_t)ws % 16 == 0, "msda_backward_det: null / misaligned pointer");
  hipStream_t st = (hipStream_t)stream;
  const size_t nval = (size_t)N * S * M * D;
  if (N == 0) return DVIS_OK;
  if (Lq == 0) return dvis_zero_words(grad_value, nval, st, "msda_backward_det: zero grad_value");
  unsigned *absmax = (unsigned *)ws;
  unsigned long long *acc = (unsigned long long *)((char *)ws + 16);
  // (a kernel, not hipMemsetAsync: a memset node of a hipGraph fills with garbage from its second replay on, dvis_common.h)
  if (const int rc = dvis_zero_words(ws, 4 + nval * 2, st, "msda_backward_det: zero workspace")) return rc;
  const size_t ngo = (size_t)N * Lq * M * D, nw = (size_t)N * Lq * M * L * P;
  hipLaunchKernelGGL(absmax_kernel, dim3((unsigned)std::min<size_t>((ngo + 255) / 256, 2048)), dim3(256), 0, st, grad_out, ngo, absmax);
  hipLaunchKernelGGL(absmax_kernel, dim3((unsigned)std::min<size_t>((nw + 255) / 256, 2048)), dim3(256), 0, st, w, nw, absmax + 1);
  const size_t npairs = (size_t)N * Lq * M;
  const DetArgs det = {acc, absmax};
  if (D <= 32) {
    const size_t blocks = (npairs + 7) / 8;
    hipLaunchKernelGGL((msda_bwd_kernel<float, 32, true>), dim3((unsigned)(blocks > 262144 ? 262144 : blocks)), dim3(256), 0, st, value,
                       shapes, level_start, loc, w, grad_out, npairs, S, M, D, L, Lq, P, grad_value, grad_loc, grad_w, det);
  } else {
    const size_t blocks = (npairs + 3) / 4;
    hipLaunchKernelGGL((msda_bwd_kernel<float, 64, true>), dim3((unsigned)(blocks > 262144 ? 262144 : blocks)), dim3(256), 0, st, value,
                       shapes, level_start, loc, w, grad_out, npairs, S, M, D, L, Lq, P, grad_value, grad_loc, grad_w, det);
  }
  if (const int rc = dvis_check_launch("msda_bwd_kernel (deterministic)")) return rc;
  hipLaunchKernelGGL(det_finish_kernel, dim3((unsigned)std::min<size_t>((nval + 255) / 256, 65536)), dim3(256), 0, st, acc, absmax, grad_value,
                     nval);
  return dvis_check_launch("det_finish_kernel");
}

DVIS_EXPORT int dvis_msda_backward(int dtype, const void *value, const int64_t *shapes, const int64_t *level_start,
                                   const void *loc, const void *w, const void *grad_out, int N, int S, int M, int D,
                                   int L, int Lq, int P, void *grad_value, void *grad_loc, void *grad_w,
                                   void *stream) {
  DVIS_REQUIRE(N >= 0 && S > 0 && M > 0 && D > 0 && L > 0 && Lq >= 0 && P > 0, "msda_backward: bad sizes");
  if (N == 0 || Lq == 0) return DVIS_OK;
  DVIS_REQUIRE(value && shapes && level_start && loc && w && grad_out && grad_value && grad_loc && grad_w,
               "msda_backward: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (dtype == DVIS_F32)
    return launch_bwd<float>(value, shapes, level_start, loc, w, grad_out, N, S, M, D, L, Lq, P, grad_value, grad_loc,
                             grad_w, st);
  if (dtype == DVIS_F64)
    return launch_bwd<double>(value, shapes, level_start, loc, w, grad_out, N, S, M, D, L, Lq, P, grad_value, grad_loc,
                              grad_w, st);
  dvis_set_error("msda_backward: only fp32 / fp64 gradients are supported (got dtype %d)", dtype);
  return DVIS_E_UNSUPPORTED;
}

DVIS_EXPORT int64_t dvis_msda_fused_backward_ws_bytes(int N, int S, int M, int D) {
  return dvis_msda_backward_det_ws_bytes(N, S, M, D);
}

// Backward of dvis_msda_fused_forward (fp32).
// grad_offsets (N * Lq, M * L * P * 2) and grad_logits (N * Lq, M * L * P) are contiguous and the same bits in both forms and
// from run to run; the reference points get no gradient.  ws == NULL: grad_value through float atomics; otherwise
// dvis_msda_fused_backward_ws_bytes bytes, 16-byte aligned: the 64-bit fixed-point form (see DetArgs), reproducible.
// grad_value is fully written by the call in both forms.
DVIS_EXPORT int dvis_msda_fused_backward(const float *value, const int64_t *shapes, const int64_t *level_start, const float *ref,
                                         int Nref, const float *offsets, int64_t off_stride, const float *logits,
                                         int64_t logit_stride, const float *grad_out, int N, int S, int M, int D, int L, int Lq,
                                         int P, float *grad_value, float *grad_offsets, float *grad_logits, void *ws,
                                         void *stream) {
  DVIS_REQUIRE(N >= 0 && S > 0 && M > 0 && D > 0 && L > 0 && Lq >= 0 && P > 0, "msda_fused_backward: bad sizes");
  if (N == 0) return DVIS_OK;
  DVIS_REQUIRE(grad_value && (uintptr_t)ws % 16 == 0, "msda_fused_backward: null grad_value / misaligned workspace");
  hipStream_t st = (hipStream_t)stream;
  const size_t nval = (size_t)N * S * M * D;
  if (Lq == 0) return dvis_zero_words(grad_value, nval, st, "msda_fused_backward: zero grad_value");
  DVIS_REQUIRE(value && shapes && level_start && ref && offsets && logits && grad_out && grad_offsets && grad_logits,
               "msda_fused_backward: null pointer");
  DVIS_REQUIRE(Nref == 1 || Nref == N, "msda_fused_backward: Nref must be 1 or N");
  DVIS_REQUIRE(off_stride >= (int64_t)M * L * P * 2 && logit_stride >= (int64_t)M * L * P, "msda_fused_backward: row strides too small");
  DVIS_REQUIRE(off_stride % 4 == 0 && logit_stride % 4 == 0 && aligned16(offsets) && aligned16(logits) && aligned16(value) &&
                   aligned16(grad_out) && aligned16(grad_value) && aligned16(grad_offsets) && aligned16(grad_logits),
               "msda_fused_backward: 16-byte alignment required");
  DVIS_REQUIRE((size_t)S * M * D * sizeof(float) < 0x7fffffffu, "msda_fused_backward: frame slice >= 2 GiB");
  DVIS_REQUIRE((size_t)Lq * (size_t)(off_stride > logit_stride ? off_stride : logit_stride) * sizeof(float) < 0x7fffffffu,
               "msda_fused_backward: one frame of offsets/logits must stay below 2 GiB");
  if (!((D == 32 || D == 64) && P == 4 && (L == 1 || L == 3 || L == 4))) {
    dvis_set_error("msda_fused_backward: unsupported (D=%d, L=%d, P=%d); supported D in {32,64}, (L,P) in {(1,4),(3,4),(4,4)}", D, L, P);
    return DVIS_E_UNSUPPORTED;
  }
  DetArgs det{};
  if (ws) {
    unsigned *absmax = (unsigned *)ws;
    det = {(unsigned long long *)((char *)ws + 16), absmax};
    // (a kernel, not hipMemsetAsync: see dvis_msda_backward_det)
    if (const int rc = dvis_zero_words(ws, 4 + nval * 2, st, "msda_fused_backward: zero workspace")) return rc;
    const size_t ngo = (size_t)N * Lq * M * D;
    hipLaunchKernelGGL(absmax_kernel, dim3((unsigned)std::min<size_t>((ngo + 255) / 256, 2048)), dim3(256), 0, st, grad_out, ngo, absmax);
    hipLaunchKernelGGL(det_unit_weight_kernel, dim3(1), dim3(1), 0, st, absmax);
  } else if (const int rc = dvis_zero_words(grad_value, nval, st, "msda_fused_backward: zero grad_value")) {
    return rc;
  }
  const size_t npairs = (size_t)N * Lq * M;
  int rc = DVIS_OK;
#define DVIS_FUSED_BWD_CASE(d, l)                                                                                              \
  if (D == d && L == l)                                                                                                        \
    rc = launch_fused_bwd<d, l, 4>(value, shapes, level_start, ref, Nref, offsets, off_stride, logits, logit_stride, grad_out, \
                                   npairs, S, M, Lq, grad_value, grad_offsets, grad_logits, ws ? &det : nullptr, st);
  DVIS_FUSED_BWD_CASE(32, 1)
  DVIS_FUSED_BWD_CASE(32, 3)
  DVIS_FUSED_BWD_CASE(32, 4)
  DVIS_FUSED_BWD_CASE(64, 1)
  DVIS_FUSED_BWD_CASE(64, 3)
  DVIS_FUSED_BWD_CASE(64, 4)
#undef DVIS_FUSED_BWD_CASE
  if (rc || !ws) return rc;
  hipLaunchKernelGGL(det_finish_kernel, dim3((unsigned)std::min<size_t>((nval + 255) / 256, 65536)), dim3(256), 0, st, det.acc, det.absmax,
                     grad_value, nval);
  return dvis_check_launch("det_finish_kernel");
}
