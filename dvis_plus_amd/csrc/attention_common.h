// What attention.hip, attention_backward.hip and masked_attention_backward.hip share: the strided view of a (B, heads, L, d) tensor,
// the base-2 softmax constants, the host-side view checks, and — for the two backward files — the per-key pieces of the query-chunk
// loop whose numerics must stay the same in both.  Everything is static inline / __device__ __forceinline__: no translation unit.
#pragma once

#include <initializer_list>

#include "dvis_common.h"

// (an unnamed namespace, as in the files that include this: dvis_strides is a kernel parameter, and every kernel keeps its symbol)
namespace {

struct dvis_strides {
  int64_t b, h, r;   // floats between batch entries / heads / rows (last dim contiguous)
};

static inline dvis_strides dvis_strides_from(const int64_t *s) { return dvis_strides{s[0], s[1], s[2]}; }

// The softmax runs in base 2: scores are scaled by scale * log2(e), so exp(s - m) is ONE v_exp_f32 (a quarter-rate
// transcendental) per score instead of expf's range reduction around it.  Row statistics live in the same base-2 units; the
// normalised output does not care.
constexpr float kLog2e = 1.4426950408889634f;
__device__ __forceinline__ float ex2(float x) { return __builtin_amdgcn_exp2f(x); }

constexpr size_t kLdsLimit = 160 * 1024;   // LDS of a gfx950 workgroup

// The kernels' view contract on the host: no null pointer among `ptrs`, `strides` and `also_nonnull`; every pointer of `ptrs` 16-byte
// aligned (the kernels read and write float4) and every stride of `strides` a multiple of 4 floats.  `who` and `names` go into the
// messages ("attention_backward", "q/k/v/grad_out").
static inline int attn_check_views(const char *who, const char *names, std::initializer_list<const void *> ptrs,
                                   std::initializer_list<const int64_t *> strides,
                                   std::initializer_list<const void *> also_nonnull = {}) {
  bool all = true;
  uintptr_t al = 0;
  for (const void *p : ptrs) all = all && p, al |= (uintptr_t)p;
  for (const int64_t *s : strides) all = all && s;
  for (const void *p : also_nonnull) all = all && p;
  DVIS_REQUIRE(all, "%s: null pointer", who);
  int64_t st = 0;
  for (const int64_t *s : strides) st |= s[0] | s[1] | s[2];
  DVIS_REQUIRE((al & 15) == 0 && (st & 3) == 0, "%s: %s must be 16-byte aligned with strides that are multiples of 4 floats", who,
               names);
  return DVIS_OK;
}

// ---- the two backward kernels: attn_bwd_kernel (attention_backward.hip) and mab_tile_kernel (masked_attention_backward.hip).  Thread
// t owns key t of its workgroup, the queries are walked in chunks of kQC rows held in LDS at a row stride of DH + 4 floats.
constexpr int kQC = 16;        // queries per chunk

// Step (1) of a chunk: rows q0 .. q0 + kQC - 1 of Q and dO -> LDS; rows past Lq are zeros (they then add exact zeros to dK and dV).
template <int DH>
__device__ __forceinline__ void bwd_load_chunk(float *q_lds, float *g_lds, const float *qb, const float *gb, int64_t q_row_stride,
                                               int64_t g_row_stride, int q0, int Lq, int tid, int nthr) {
  constexpr int LS = DH + 4, C4 = DH / 4;
  for (int e = tid; e < kQC * C4; e += nthr) {
    const int row = e / C4, c4 = e - row * C4;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    if (q0 + row < Lq) {
      a = *reinterpret_cast<const float4 *>(qb + (size_t)(q0 + row) * q_row_stride + 4 * c4);
      b = *reinterpret_cast<const float4 *>(gb + (size_t)(q0 + row) * g_row_stride + 4 * c4);
    }
    *reinterpret_cast<float4 *>(&q_lds[row * LS + 4 * c4]) = a;
    *reinterpret_cast<float4 *>(&g_lds[row * LS + 4 * c4]) = b;
  }
}

// The key's K row as float4 pieces: from LDS (a row of floats) or from registers (an array of float4).
__device__ __forceinline__ float4 bwd_k4(const float *k_row, int c) { return *reinterpret_cast<const float4 *>(k_row + 4 * c); }
__device__ __forceinline__ float4 bwd_k4(const float4 *k_regs, int c) { return k_regs[c]; }

// Step (2) for one row of the chunk: *s_raw = q_i . k_t (unscaled: the caller scales it into log2 units), *dp = dO_i . v_t.  Each dot
// product runs as FOUR fma chains, one per component of the float4 pieces (dims c, c + 4, c + 8, ...), summed pairwise at the end: a
// single chain over d = 64 unscaled products carried 4 - 8 times the rounding error of a blocked fp32 dot product into the scores
// (with one query nothing averages it out of dv = p dO: 4.8e-07 against 1.1e-07 of an fp32 CPU run at Lq 1, Lk 17, d 64), and four
// independent chains are four times shorter on the fma latency.  The caller's loop over the rows of the chunk stays rolled
// (#pragma unroll 1): unrolled, hipcc issues the LDS reads of all 16 rows first and spills a thousand registers.
template <int DH, typename KSrc>
__device__ __forceinline__ void bwd_dots(KSrc k_src, const float4 *vr, const float *q_row, const float *g_row, float *s_raw,
                                         float *dp) {
  float4 s4 = make_float4(0.f, 0.f, 0.f, 0.f), d4 = s4;
#pragma unroll
  for (int c = 0; c < DH / 4; ++c) {
    const float4 kk = bwd_k4(k_src, c);
    const float4 vv = vr[c];
    const float4 qq = *reinterpret_cast<const float4 *>(q_row + 4 * c);
    const float4 gg = *reinterpret_cast<const float4 *>(g_row + 4 * c);
    s4.x = fmaf(qq.x, kk.x, s4.x);
    s4.y = fmaf(qq.y, kk.y, s4.y);
    s4.z = fmaf(qq.z, kk.z, s4.z);
    s4.w = fmaf(qq.w, kk.w, s4.w);
    d4.x = fmaf(gg.x, vv.x, d4.x);
    d4.y = fmaf(gg.y, vv.y, d4.y);
    d4.z = fmaf(gg.z, vv.z, d4.z);
    d4.w = fmaf(gg.w, vv.w, d4.w);
  }
  *s_raw = (s4.x + s4.y) + (s4.z + s4.w);
  *dp = (d4.x + d4.y) + (d4.z + d4.w);
}

// One row of the chunk into the key's gradients: dV[t] += p dO_i, dK[t] += ds Q_i (the rows in ascending order: the caller's loop).
template <int DH>
__device__ __forceinline__ void bwd_accumulate(float p, float ds, const float *q_row, const float *g_row, float4 *dka, float4 *dva) {
#pragma unroll
  for (int c = 0; c < DH / 4; ++c) {
    const float4 qq = *reinterpret_cast<const float4 *>(q_row + 4 * c);
    const float4 gg = *reinterpret_cast<const float4 *>(g_row + 4 * c);
    dva[c].x = fmaf(p, gg.x, dva[c].x);
    dva[c].y = fmaf(p, gg.y, dva[c].y);
    dva[c].z = fmaf(p, gg.z, dva[c].z);
    dva[c].w = fmaf(p, gg.w, dva[c].w);
    dka[c].x = fmaf(ds, qq.x, dka[c].x);
    dka[c].y = fmaf(ds, qq.y, dka[c].y);
    dka[c].z = fmaf(ds, qq.z, dka[c].z);
    dka[c].w = fmaf(ds, qq.w, dka[c].w);
  }
}

// The key's rows of dK (times scale) and dV, written once.
template <int DH>
__device__ __forceinline__ void bwd_store_dkdv(float *dkrow, float *dvrow, const float4 *dka, const float4 *dva, float scale) {
#pragma unroll
  for (int c = 0; c < DH / 4; ++c) {
    *reinterpret_cast<float4 *>(dkrow + 4 * c) = make_float4(dka[c].x * scale, dka[c].y * scale, dka[c].z * scale, dka[c].w * scale);
    *reinterpret_cast<float4 *>(dvrow + 4 * c) = dva[c];
  }
}

}  // namespace
