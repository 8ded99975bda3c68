// The pixel-slab contraction shared by mask_gemm_backward.hip and mask_pool.hip — gfx950, exact-fp32 MFMA, deterministic.
//
// Per frame b, for a row operand a (B, R, HW) and a map feat (B, C, HW):
//   part[b, s, r, c]  = sum over the pixels p of slab s of  A(a[b, r, p]) * feat[b, c, p]
//   part_sum[b, s, r] = sum over the pixels p of slab s of  A(a[b, r, p])
// POOL = false: A is the identity (the gradient of the mask logits with respect to the embeddings, mask_gemm_backward.hip);
// POOL = true : A(v) = v > 0 ? 1 : 0, a select on the loaded logit (mask pooling, mask_pool.hip) and part_sum holds int32 counts.
//
//   * grid = (pixel slabs, row blocks of 64 rows x channel chunks, frames).  A wave owns ONE 16-row tile of a and the CT <= 16
//     channel tiles of its chunk (CT accumulators of 16 x 16): within a chunk the big operand, a, is read from memory by exactly
//     one wave, once; the feature slab is shared by the four waves of a workgroup and by the row blocks of the frame through the
//     caches (C x 4096 x 4 B = 4 MB per slab).  C <= 16 CT is one chunk (the backward's domain: its launch is what it always was).
//   * both operands are pixel-contiguous, so both go from global memory straight into the MFMA operand layout: lane (j, k)
//     (j = lane & 15, k = lane >> 4) loads pixels [p + 16 k + 4 q, + 4) of row r0 + j (A) and of channel 16 ct + j (B) as one
//     16-byte word; element i of that word is the K index k of MFMA i.  The K index is permuted (MFMA i of sub-step q sums pixels
//     p + 16 k + 4 q + i over k), identically for A and B, so the sum runs over every pixel exactly once.  No LDS, no barrier.
//   * v_mfma_f32_16x16x4_f32 is a k-ordered fp32 fma chain: exact fp32 products and sums, no reduced precision.
//   * determinism: NO floating-point atomics.  A slab is SLAB consecutive pixels (4096 for the backward, 512 for the pool, whose
//     Q <= 256 rows make at most 4 row blocks per slab) — the slab count S = ceil(HW / SLAB) is
//     a function of HW alone, not of the CU count — and a workgroup writes its partial tile to a workspace (B, S, R, C); a second
//     kernel adds the S partials in slab order.  S == 1 writes the result directly.  Same inputs, same bits, every call, whatever
//     the batch a frame is part of.
//   * the rows of a may be strided (batch and row strides in elements; the pixels of a row are contiguous): a wave's buffer
//     descriptor starts at ITS 16-row tile, so the offsets inside it stay below 2 GiB however far apart the frames lie.
//   * out-of-range convention as in mask_gemm.hip: a row / channel / pixel that does not exist gets the buffer offset 2 GiB, past
//     a tile that the host checks to be shorter than 2 GiB, and reads 0 (A(0) = 0).  VEC = false (HW % 4 != 0, an unaligned base
//     or stride) loads and bounds-checks every pixel on its own.
#pragma once
#include "dvis_common.h"

namespace {

constexpr int kSlab = 4096;      // pixels per slab of the backward (SLAB: a multiple of the 64 pixels of a wave step)
constexpr int kPoolSlab = 512;   // ... of mask pooling: Q <= 256 rows are at most 4 row blocks, so the slabs are what fills the chip
constexpr int kRowTiles = 4;     // waves per workgroup = 16-row tiles per row block
constexpr unsigned kOOB = 0x80000000u;

// (two waves per SIMD: 64 accumulators + two sets of 64 fragment registers at CT = 16 fit the 256 registers of that occupancy;
// POOL carries a second set of CT accumulator tiles and is instantiated up to CT = 8)
template <int CT, bool VEC, bool POOL, int SLAB>
__global__ __launch_bounds__(64 * kRowTiles) __attribute__((amdgpu_waves_per_eu(2))) void mask_slab_kernel(
    const float *__restrict__ g, long long g_bstride, long long g_rstride, const float *__restrict__ feat, int R, int C, int HW,
    int S, float *__restrict__ part, float *__restrict__ part_sum) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int j = lane & 15, kq = lane >> 4;
  const int s = blockIdx.x, b = blockIdx.z;
  const int row_blocks = ((R + 15) / 16 + kRowTiles - 1) / kRowTiles;
  const int chunk = blockIdx.y / row_blocks;
  const int c0 = chunk * CT * 16;
  const int r0 = ((blockIdx.y - chunk * row_blocks) * kRowTiles + wv) * 16;
  if (r0 >= R) return;   // wave-uniform; the kernel has no barrier
  const int p_lo = s * SLAB;
  const int p_hi = p_lo + SLAB < HW ? p_lo + SLAB : HW;
  const int rows = R - r0 < 16 ? R - r0 : 16, chans = C - c0 < CT * 16 ? C - c0 : CT * 16;

  const __amdgpu_buffer_rsrc_t rg = dvis_make_rsrc_uniform(
      g + (size_t)b * g_bstride + (size_t)r0 * g_rstride, (unsigned)(((size_t)(rows - 1) * g_rstride + HW) * sizeof(float)));
  const __amdgpu_buffer_rsrc_t rf =
      dvis_make_rsrc_uniform(feat + ((size_t)b * C + c0) * HW, (unsigned)((size_t)chans * HW * sizeof(float)));
  const bool row_ok = j < rows;
  const unsigned a_base = (unsigned)j * (unsigned)g_rstride * 4u;
  unsigned b_base[CT];
  bool ch_ok[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    ch_ok[ct] = ct * 16 + j < chans;
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
    if (POOL) {   // membership: the comparison is false for 0.0, -0.0 and NaN, true for every positive value, denormals included
#pragma unroll
      for (int n = 0; n < 4; ++n) a[n] = a[n] > 0.f ? 1.f : 0.f;
    }
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) bf[ct] = load4(rf, ch_ok[ct], b_base[ct], pix);
  };

  dvis_f4 acc[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) acc[ct] = dvis_f4{0.f, 0.f, 0.f, 0.f};
  // POOL: two-level sums.  A pooled row is the sum of up to H W values of one sign-mixed map, and the error of ONE fma chain grows
  // with its length times the size of its partial sums; the MFMA chain is therefore cut at every wave step (64 pixels) and the
  // steps' tiles are added into `tot`: at 3840 pixels the distance to an fp64 sum drops six-fold, to that of a blocked CPU GEMM.
  // Still a fixed order.  (The backward keeps its single chain: its entry points keep their bits.)
  dvis_f4 tot[POOL ? CT : 1];
#pragma unroll
  for (int ct = 0; ct < (POOL ? CT : 1); ++ct) tot[ct] = dvis_f4{0.f, 0.f, 0.f, 0.f};
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
    if (POOL && ((t + 2) & 3) == 0) {   // uniform: a wave step (64 pixels) is complete — nsub % 4 == 0, so the last one is too
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        tot[ct] += acc[ct];
        acc[ct] = dvis_f4{0.f, 0.f, 0.f, 0.f};
      }
    }
  }

  // ---- epilogue.  Accumulator layout: column (channel) = lane & 15, row = (lane >> 4) * 4 + reg.
  float *dst = part + ((size_t)b * S + s) * R * C + c0;
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = r0 + kq * 4 + r, c = ct * 16 + j;
      if (row < R && c < chans) dst[(size_t)row * C + c] = POOL ? tot[ct][r] : acc[ct][r];
    }
  // the four lane groups hold the sums of their pixels of row r0 + j: ((k0 + k1) + (k2 + k3)), the same in every lane
  rsum += __shfl_xor(rsum, 16);
  rsum += __shfl_xor(rsum, 32);
  if (kq == 0 && row_ok && chunk == 0) {
    const size_t at = ((size_t)b * S + s) * R + r0 + j;
    if (POOL)
      reinterpret_cast<int *>(part_sum)[at] = (int)rsum;   // at most SLAB ones: exact
    else
      part_sum[at] = rsum;
  }
}

// out[b, i] = part[b, 0, i] + part[b, 1, i] + ... in slab order, i < n
template <typename T>
__global__ __launch_bounds__(256) void sum_slabs_kernel(const T *__restrict__ part, T *__restrict__ out, int S, long long n,
                                                        long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const long long b = idx / n, i = idx - b * n;
  const T *src = part + (size_t)b * S * n + i;
  T v = src[0];
  for (int s = 1; s < S; ++s) v += src[(size_t)s * n];
  out[idx] = v;
}

int slabs_of(int64_t HW, int slab = kSlab) { return (int)((HW + slab - 1) / slab); }

template <int CT, bool VEC, bool POOL>
void launch_slabs(const float *g, long long g_bstride, long long g_rstride, const float *feat, int B, int R, int C, int HW, int S,
                  float *part, float *part_sum, hipStream_t st) {
  const int row_blocks = ((R + 15) / 16 + kRowTiles - 1) / kRowTiles;
  const int chunks = (C + CT * 16 - 1) / (CT * 16);
  hipLaunchKernelGGL((mask_slab_kernel<CT, VEC, POOL, POOL ? kPoolSlab : kSlab>), dim3(S, row_blocks * chunks, B), dim3(64 * kRowTiles), 0, st, g, g_bstride,
                     g_rstride, feat, R, C, HW, S, part, part_sum);
}

}  // namespace
