// Mask pooling of the open-vocabulary (FC-CLIP) heads — gfx950, exact-fp32 MFMA, deterministic.
//
// The reference's MaskPooling (ov_dvis/video_mask2former_transformer_decoder_ov.py:39-67) writes a binary float (B, Q, H, W)
// tensor, divides it by its per-row sum in a second pass and contracts it with the map in an einsum.  Here, per frame b:
//   sum[b, q, c] = sum over the pixels p with logit[b, q, p] > 0 of x[b, c, p]           (B, Q, C)
//   count[b, q]  = the number of those pixels                                            (B, Q) int32
// and the mean, its `+ 1e-8` and any combination over frames stay with the caller (the refiner pools over (T H, W) and re-weights
// windows by pixel counts, ov_dvis/video_dvis_modules_ov.py:514-527).
//
// The kernel is the slab core of mask_slab_core.h with POOL = true: the A operand of the MFMA is `logit > 0 ? 1 : 0`, a select on
// the loaded logit (0.0, -0.0 and NaN are outside the mask, every positive value — denormals included — inside); the logits
// themselves never enter the arithmetic, and the binary tensor is never written.  The 0 / 1 operand then goes through the fp32
// MFMA with the map, so a row's sum is the k-ordered fp32 sum of 1 * x and 0 * x terms: exact selection for every finite x; a
// non-finite x of a frame reaches every row of THAT frame (0 * inf), as it does through the reference's einsum, and no other frame.
//   * the logits are a strided view: the (H, W) plane is contiguous, batch and query strides are given in elements, so a frame of
//     the (1, Q, T, H, W) inference logits is pooled in place;
//   * C up to 2048 in chunks of 128 channels (8 accumulator tiles and the 8 tiles of the two-level sum): grid.y = row blocks x
//     chunks; every chunk re-reads the logits (C = 256: twice; C = 1536 on the CLIP map: 12 reads of a 23 x 40 plane per query);
//   * two-level sums: the fma chain is cut every 64 pixels (mask_slab_core.h) — at 48 x 80 a single chain over the slab was 10 x as
//     far from the fp64 sum as a blocked CPU GEMM, the two-level sum is as close as that;
//   * the count of a slab is the row sum of the 0 / 1 operand (at most 512: exact in fp32), stored as int32 and added as integers;
//   * pixels are cut into slabs of 512 by their number alone (115 slabs x 4 workgroups for ONE 720p frame of 100 queries: with the
//     backward's 4096 that frame was 60 workgroups on 256 compute units), partials are added in slab order: no float atomics, the same bits
//     on every call, a frame's bits do not depend on B.  Every element of sum and count is written.  No memset, no host
//     synchronisation: capturable.  Workspace from the caller (dvis_mask_pool_ws_bytes; none for one slab).
#include "mask_slab_core.h"

namespace {
constexpr int kMaxQ = 256, kMaxC = 2048;
}

// the served shapes: everything else is refused before a launch, naming the value
static int mask_pool_check(int B, int Q, int C, int64_t HW) {
  DVIS_REQUIRE(B >= 0 && B <= 65535, "mask_pool: serves 0 <= B <= 65535 frames (got B=%d)", B);
  DVIS_REQUIRE(Q >= 1 && Q <= kMaxQ, "mask_pool: serves 1 <= Q <= %d queries (got Q=%d)", kMaxQ, Q);
  DVIS_REQUIRE(C >= 4 && C <= kMaxC && C % 4 == 0, "mask_pool: serves C %% 4 == 0 up to %d channels (got C=%d)", kMaxC, C);
  DVIS_REQUIRE(HW >= 1, "mask_pool: H W >= 1 (got %lld)", (long long)HW);
  DVIS_REQUIRE((long long)C * HW * 4 < (1ll << 31), "mask_pool: one frame of x must stay below 2^31 bytes (got C=%d x H W=%lld floats)",
               C, (long long)HW);
  DVIS_REQUIRE((long long)Q * HW * 4 < (1ll << 31),
               "mask_pool: one frame of the mask logits must stay below 2^31 bytes (got Q=%d x H W=%lld floats)", Q, (long long)HW);
  return DVIS_OK;
}

DVIS_EXPORT int dvis_mask_pool_plan(int B, int Q, int C, int64_t HW, int32_t *plan) {
  DVIS_REQUIRE(plan, "mask_pool_plan: null pointer");
  if (const int rc = mask_pool_check(B, Q, C, HW)) return rc;
  plan[0] = kPoolSlab;
  plan[1] = slabs_of(HW, kPoolSlab);
  return DVIS_OK;
}

DVIS_EXPORT int64_t dvis_mask_pool_ws_bytes(int B, int Q, int C, int64_t HW) {
  if (B <= 0 || Q <= 0 || C <= 0 || HW <= 0) return 0;
  const int S = slabs_of(HW, kPoolSlab);
  return S == 1 ? 0 : (int64_t)B * S * Q * (C + 1) * (int64_t)sizeof(float);
}

DVIS_EXPORT int dvis_mask_pool(const float *x, const float *logits, int64_t l_bstride, int64_t l_qstride, int B, int Q, int C,
                               int64_t HW, float *sum, int32_t *count, void *ws, void *stream) {
  if (const int rc = mask_pool_check(B, Q, C, HW)) return rc;
  if (B == 0) return DVIS_OK;
  DVIS_REQUIRE(x && logits && sum && count, "mask_pool: null pointer");
  DVIS_REQUIRE(l_bstride >= 0 && (Q == 1 || l_qstride >= HW),
               "mask_pool: the logit planes must not overlap: query stride >= H W and batch stride >= 0 (got %lld, %lld; H W=%lld)",
               (long long)l_qstride, (long long)l_bstride, (long long)HW);
  if (Q == 1) l_qstride = HW;
  DVIS_REQUIRE((15 * l_qstride + HW) * 4 < (1ll << 31),
               "mask_pool: 16 consecutive query planes must span less than 2^31 bytes (got query stride %lld elements)",
               (long long)l_qstride);
  const int S = slabs_of(HW, kPoolSlab);
  DVIS_REQUIRE(S == 1 || ws, "mask_pool: %d pixel slabs need a workspace (dvis_mask_pool_ws_bytes)", S);
  hipStream_t st = (hipStream_t)stream;
  float *part = S == 1 ? sum : (float *)ws;
  float *part_cnt = S == 1 ? (float *)count : (float *)ws + (size_t)B * S * Q * C;
  const bool vec = HW % 4 == 0 && l_bstride % 4 == 0 && l_qstride % 4 == 0 && (((uintptr_t)x | (uintptr_t)logits) & 15) == 0;
#define DVIS_MP(CT_)                                                                                                    \
  (vec ? launch_slabs<CT_, true, true>(logits, l_bstride, l_qstride, x, B, Q, C, (int)HW, S, part, part_cnt, st)        \
       : launch_slabs<CT_, false, true>(logits, l_bstride, l_qstride, x, B, Q, C, (int)HW, S, part, part_cnt, st))
  if (C <= 64)
    DVIS_MP(4);
  else
    DVIS_MP(8);   // C > 128: ceil(C / 128) channel chunks
#undef DVIS_MP
  if (const int rc = dvis_check_launch("mask_slab_kernel (mask_pool)")) return rc;
  if (S > 1) {
    const long long n1 = (long long)Q * C, t1 = (long long)B * n1, t2 = (long long)B * Q;
    hipLaunchKernelGGL(sum_slabs_kernel<float>, dim3((unsigned)((t1 + 255) / 256)), dim3(256), 0, st, part, sum, S, n1, t1);
    hipLaunchKernelGGL(sum_slabs_kernel<int>, dim3((unsigned)((t2 + 255) / 256)), dim3(256), 0, st, (const int *)part_cnt,
                       (int *)count, S, (long long)Q, t2);
    return dvis_check_launch("sum_slabs_kernel (mask_pool)");
  }
  return DVIS_OK;
}
