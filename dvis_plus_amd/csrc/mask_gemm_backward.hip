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
// The kernel is the slab core of mask_slab_core.h (shared with mask_pool.hip) with POOL = false: its structure, determinism and
// out-of-range convention are described there.  Traffic: the partials cost S * R * C * 4 B written and read once against
// R * HW * 4 B of g read: 2 C S / HW <= 2 C / 4096 = 12.5 % at C = 256 (15 slabs at 58 880 pixels: 18.4 MB against 141 MB per frame).
#include "mask_slab_core.h"

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
#define DVIS_MB(CT_)                                                                                               \
  (vec ? launch_slabs<CT_, true, false>(g, (long long)R * HW, HW, feat, B, R, C, (int)HW, S, part, part_sum, st)   \
       : launch_slabs<CT_, false, false>(g, (long long)R * HW, HW, feat, B, R, C, (int)HW, S, part, part_sum, st))
  if (ct <= 4)
    DVIS_MB(4);
  else if (ct <= 8)
    DVIS_MB(8);
  else
    DVIS_MB(16);
#undef DVIS_MB
  if (const int rc = dvis_check_launch("mask_slab_kernel")) return rc;
  if (S > 1) {
    const long long n1 = (long long)R * C, t1 = (long long)B * n1, t2 = (long long)B * R;
    DVIS_REQUIRE((t1 + 255) / 256 < (1ll << 31), "mask_logits_backward: grid too large");
    hipLaunchKernelGGL(sum_slabs_kernel<float>, dim3((unsigned)((t1 + 255) / 256)), dim3(256), 0, st, part, grad_embed, S, n1, t1);
    hipLaunchKernelGGL(sum_slabs_kernel<float>, dim3((unsigned)((t2 + 255) / 256)), dim3(256), 0, st, part_sum, row_sum, S, (long long)R,
                       t2);
    return dvis_check_launch("sum_slabs_kernel");
  }
  return DVIS_OK;
}
