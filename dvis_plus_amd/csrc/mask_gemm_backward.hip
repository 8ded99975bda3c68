// Backward of the mask-logit contraction with respect to the embeddings — gfx950, exact-fp32 MFMA, deterministic.
//
// Training-side counterpart of mask_gemm.hip MODE 0.  The forward is
//   logits = einsum("lbtqc,btchw->lbqthw", mask_embed, mask_features)     (dvis_Plus/tracker.py:379; per frame the
//   einsum("bqc,bchw->bqhw") of dvis_Plus/video_mask2former_transformer_decoder.py:363)
// and this file computes, per frame b, for g = dL/dlogits (B, R, HW) and feat (B, C, HW):
//   grad_embed[b, r, c] = sum_p g[b, r, p] * feat[b, c, p]          (B, R, C)
//   row_sum[b, r]       = sum_p g[b, r, p]                          (B, R)     (the gradient of a bias folded into the map)
// R = the rows of one frame: layers x queries in training (6 x 100), all sharing the frame's ONE feature map.
//
// Shape of the problem: a tiny output (R x C <= 600 x 256) and a contraction over the pixels (58 880 at 720p stride 4): split-K.
//   * grid = (pixel slabs, row blocks of 64 rows, frames).  A wave owns ONE 16-row tile of g and ALL channel tiles (CT <= 16
//     accumulators of 16 x 16): the big operand, g, is read from memory by exactly one wave, once; the feature slab is shared by
//     the four waves of a workgroup and by the row blocks of the frame through the caches (C x 4096 x 4 B = 4 MB per slab).
//   * both operands are pixel-contiguous, so both go from global memory straight into the MFMA operand layout: lane (j, k)
//     (j = lane & 15, k = lane >> 4) loads pixels [p + 16 k + 4 q, + 4) of row r0 + j (A) and of channel 16 ct + j (B) as one
//     16-byte word; element i of that word is the K index k of MFMA i.  The K index is permuted (MFMA i of sub-step q sums pixels
//     p + 16 k + 4 q + i over k), identically for A and B, so the sum runs over every pixel exactly once.  No LDS, no barrier.
//   * v_mfma_f32_16x16x4_f32 is a k-ordered fp32 fma chain: exact fp32 products and sums, no reduced precision.
//   * determinism: NO floating-point atomics.  A slab is kSlab = 4096 consecutive pixels — the slab count S = ceil(HW / 4096) is
//     a function of HW alone, not of the CU count — and a workgroup writes its partial tile to a workspace (B, S, R, C); a second
//     kernel adds the S partials in slab order.  S == 1 writes the result directly.  Same inputs, same bits, every call, whatever
//     the batch a frame is part of.
//   * traffic: the partials cost S * R * C * 4 B written and read once against R * HW * 4 B of g read: 2 C S / HW <= 2 C / 4096 =
//     12.5 % at C = 256 (15 slabs at 58 880 pixels: 18.4 MB against 141 MB per frame).
//   * out-of-range convention as in mask_gemm.hip: a row / channel / pixel that does not exist gets the buffer offset 2 GiB, past
//     a plane that the host checks to be shorter than 2 GiB, and reads 0.  VEC = false (HW % 4 != 0 or an unaligned base) loads
//     and bounds-checks every pixel on its own.
#include "dvis_common.h"

namespace {

constexpr int kSlab = 4096;      // pixels per slab (a multiple of the 64 pixels of a wave step)
constexpr int kRowTiles = 4;     // waves per workgroup = 16-row tiles per row block
constexpr unsigned kOOB = 0x80000000u;

// (two waves per SIMD: 64 accumulators + two sets of 64 fragment registers at CT = 16 fit the 256 registers of that occupancy)
template <int CT, bool VEC>
__global__ __launch_bounds__(64 * kRowTiles) __attribute__((amdgpu_waves_per_eu(2))) void mask_bwd_kernel(
    const float *__restrict__ g, const float *__restrict__ feat, int R, int C, int HW, int S, float *__restrict__ part,
    float *__restrict__ part_sum) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int j = lane & 15, kq = lane >> 4;
  const int s = blockIdx.x, b = blockIdx.z;
  const int r0 = (blockIdx.y * kRowTiles + wv) * 16;
  if (r0 >= R) return;   // wave-uniform; the kernel has no barrier
  const int p_lo = s * kSlab;
  const int p_hi = p_lo + kSlab < HW ? p_lo + kSlab : HW;

  const __amdgpu_buffer_rsrc_t rg =
      dvis_make_rsrc_uniform(g + (size_t)b * R * HW, (unsigned)((size_t)R * HW * sizeof(float)));
  const __amdgpu_buffer_rsrc_t rf =
      dvis_make_rsrc_uniform(feat + (size_t)b * C * HW, (unsigned)((size_t)C * HW * sizeof(float)));
  const bool row_ok = r0 + j < R;
  const unsigned a_base = (unsigned)(r0 + j) * (unsigned)HW * 4u;
  unsigned b_base[CT];
  bool ch_ok[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    ch_ok[ct] = ct * 16 + j < C;
    b_base[ct] = (unsigned)(ct * 16 + j) * (unsigned)HW * 4u;
  }

  // one 16-byte fragment: the 4 pixels [pix, pix + 4) of a row of g / a channel of feat, zeros where they do not exist
  auto load4 = [&](const __amdgpu_buffer_rsrc_t &rs, bool ok, unsigned base, int pix) -> dvis_f4 {
    if (VEC) {   // p_hi % 4 == 0: the four pixels exist together or not at all
      const unsigned off = ok && pix < p_hi ? base + (unsigned)pix * 4u : kOOB;
      return __builtin_bit_cast(dvis_f4, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0));
    }
    dvis_f4 v;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const unsigned off = ok && pix + n < p_hi ? base + (unsigned)(pix + n) * 4u : kOOB;
      v[n] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0));
    }
    return v;
  };
  auto load_step = [&](int pix, dvis_f4 &a, dvis_f4(&bf)[CT]) {
    a = load4(rg, row_ok, a_base, pix);
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) bf[ct] = load4(rf, ch_ok[ct], b_base[ct], pix);
  };

  dvis_f4 acc[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) acc[ct] = dvis_f4{0.f, 0.f, 0.f, 0.f};
  float rsum = 0.f;
  auto contract = [&](const dvis_f4 &a, const dvis_f4(&bf)[CT]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], bf[ct][i], acc[ct], 0, 0, 0);
    rsum += (a[0] + a[1]) + (a[2] + a[3]);
  };

  // sub-steps of 16 pixels per lane group, 64 per wave; double-buffered: the next fragments are in flight under the MFMAs
  const int nsub = ((p_hi - p_lo + 63) / 64) * 4;   // uniform
  auto pix_of = [&](int t) { return p_lo + (t >> 2) * 64 + 16 * kq + 4 * (t & 3); };
  dvis_f4 a0, a1, bf0[CT], bf1[CT];
  load_step(pix_of(0), a0, bf0);
#pragma unroll 1
  for (int t = 0; t < nsub; t += 2) {   // nsub % 4 == 0
    load_step(pix_of(t + 1), a1, bf1);
    contract(a0, bf0);
    if (t + 2 < nsub) load_step(pix_of(t + 2), a0, bf0);   // uniform
    contract(a1, bf1);
  }

  // ---- epilogue.  Accumulator layout: column (channel) = lane & 15, row = (lane >> 4) * 4 + reg.
  float *dst = part + ((size_t)b * S + s) * R * C;
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = r0 + kq * 4 + r, c = ct * 16 + j;
      if (row < R && c < C) dst[(size_t)row * C + c] = acc[ct][r];
    }
  // the four lane groups hold the sums of their pixels of row r0 + j: ((k0 + k1) + (k2 + k3)), the same in every lane
  rsum += __shfl_xor(rsum, 16);
  rsum += __shfl_xor(rsum, 32);
  if (kq == 0 && row_ok) part_sum[((size_t)b * S + s) * R + r0 + j] = rsum;
}

// out[b, i] = part[b, 0, i] + part[b, 1, i] + ... in slab order, i < n
__global__ __launch_bounds__(256) void sum_slabs_kernel(const float *__restrict__ part, float *__restrict__ out, int S, long long n,
                                                        long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const long long b = idx / n, i = idx - b * n;
  const float *src = part + (size_t)b * S * n + i;
  float v = src[0];
  for (int s = 1; s < S; ++s) v += src[(size_t)s * n];
  out[idx] = v;
}

int slabs_of(int64_t HW) { return (int)((HW + kSlab - 1) / kSlab); }

template <int CT, bool VEC>
void launch_bwd(const float *g, const float *feat, int B, int R, int C, int HW, int S, float *part, float *part_sum,
                hipStream_t st) {
  const int row_blocks = ((R + 15) / 16 + kRowTiles - 1) / kRowTiles;
  hipLaunchKernelGGL((mask_bwd_kernel<CT, VEC>), dim3(S, row_blocks, B), dim3(64 * kRowTiles), 0, st, g, feat, R, C, HW, S, part,
                     part_sum);
}

}  // namespace

DVIS_EXPORT int64_t dvis_mask_logits_backward_ws_bytes(int B, int R, int C, int64_t HW) {
  if (B <= 0 || R <= 0 || C <= 0 || HW <= 0) return 0;
  const int S = slabs_of(HW);
  return S == 1 ? 0 : (int64_t)B * S * R * (C + 1) * (int64_t)sizeof(float);
}

DVIS_EXPORT int dvis_mask_logits_backward(const float *g, const float *feat, int B, int R, int C, int64_t HW, float *grad_embed,
                                          float *row_sum, void *ws, void *stream) {
  DVIS_REQUIRE(B >= 0 && R > 0 && C > 0 && HW > 0, "mask_logits_backward: bad sizes");
  if (B == 0) return DVIS_OK;
  DVIS_REQUIRE(g && feat && grad_embed && row_sum, "mask_logits_backward: null pointer");
  DVIS_REQUIRE(C <= 256, "mask_logits_backward: supports C <= 256 (got C=%d)", C);
  DVIS_REQUIRE(B <= 65535, "mask_logits_backward: B <= 65535 frames (got %d)", B);
  DVIS_REQUIRE(R <= 65535 * 16 * kRowTiles, "mask_logits_backward: R <= %d rows per frame (got %d)", 65535 * 16 * kRowTiles, R);
  DVIS_REQUIRE(HW < (1ll << 31) && (long long)R * HW * 4 < (1ll << 31),
               "mask_logits_backward: one frame of the logit gradient (R x HW floats) must stay below 2 GiB");
  DVIS_REQUIRE((long long)C * HW * 4 < (1ll << 31), "mask_logits_backward: one frame of mask_features must stay below 2 GiB");
  const int S = slabs_of(HW);
  DVIS_REQUIRE(S == 1 || ws, "mask_logits_backward: %d pixel slabs need a workspace (dvis_mask_logits_backward_ws_bytes)", S);
  hipStream_t st = (hipStream_t)stream;
  float *part = S == 1 ? grad_embed : (float *)ws;
  float *part_sum = S == 1 ? row_sum : (float *)ws + (size_t)B * S * R * C;
  const bool vec = HW % 4 == 0 && (((uintptr_t)g | (uintptr_t)feat) & 15) == 0;
  const int ct = (C + 15) / 16;
#define DVIS_MB(CT_)                                                                                  \
  (vec ? launch_bwd<CT_, true>(g, feat, B, R, C, (int)HW, S, part, part_sum, st)                      \
       : launch_bwd<CT_, false>(g, feat, B, R, C, (int)HW, S, part, part_sum, st))
  if (ct <= 4)
    DVIS_MB(4);
  else if (ct <= 8)
    DVIS_MB(8);
  else
    DVIS_MB(16);
#undef DVIS_MB
  if (const int rc = dvis_check_launch("mask_bwd_kernel")) return rc;
  if (S > 1) {
    const long long n1 = (long long)R * C, t1 = (long long)B * n1, t2 = (long long)B * R;
    DVIS_REQUIRE((t1 + 255) / 256 < (1ll << 31), "mask_logits_backward: grid too large");
    hipLaunchKernelGGL(sum_slabs_kernel, dim3((unsigned)((t1 + 255) / 256)), dim3(256), 0, st, part, grad_embed, S, n1, t1);
    hipLaunchKernelGGL(sum_slabs_kernel, dim3((unsigned)((t2 + 255) / 256)), dim3(256), 0, st, part_sum, row_sum, S, (long long)R,
                       t2);
    return dvis_check_launch("sum_slabs_kernel");
  }
  return DVIS_OK;
}
