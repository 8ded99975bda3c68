// Backward of softmax(Q K^T * scale) V without a mask — gfx950, exact fp32 FMA, deterministic.
//
// Training-side counterpart of attention.hip for the temporal refiner's three attentions (dvis_Plus/refiner.py:104-139): over
// time (T = 11 - 21 keys, 100 - 200 sequences) and over the queries of a frame (100 - 200 keys), 8 heads of d = 32.  Autograd
// of nn.MultiheadAttention materialises the (B * heads, Lq, Lk) probabilities and runs five library GEMMs around a softmax
// backward; here one kernel recomputes the probabilities from q and k — the forward kernel saves nothing for it:
//   P = softmax(Q K^T * scale)    dV = P^T dO    dP = dO V^T    D = rowsum(P o dP)    dS = P o (dP - D)
//   dQ = scale * dS K             dK = scale * dS^T Q
//
// Shape of the problem: Lk <= 256 keys, so ONE workgroup owns a (batch entry, head) and thread t owns key t.
//   * K of the head lives in LDS for the whole kernel (row stride d + 4 floats); thread t keeps V[t, :] and its two outputs
//     dK[t, :] and dV[t, :] in registers (3 d = 192 at d = 64: one wave per SIMD may use all 512 registers).  V is needed by
//     nobody but its key's thread, so it never goes to LDS: at Lk = 256, d = 64 the kernel takes 109 KB of gfx950's 160 KB
//     (K 68 KB, the chunk's Q and dO 8.5 KB, its scores and dP 32 KB); K and V both resident would not fit next to them.
//   * the queries are walked in chunks of 16 in ascending order.  Per chunk: (1) Q and dO rows -> LDS; (2) thread t computes
//     its key's column of S and dP for the 16 rows (Q / dO rows are LDS broadcasts) and writes it to LDS; (3) 16 * R threads
//     reduce the rows — max, sum of exponentials, D — R lanes per row, a butterfly over those lanes at the end; (4) thread t
//     turns its column into P and dS, adds P dO to dV[t] and dS Q to dK[t], and leaves dS in LDS; (5) dQ = dS K, one thread
//     per output element, keys in ascending order.
//   * determinism: no atomics and no partial results across workgroups.  dK / dV add their queries in ascending order, dQ its
//     keys in ascending order; the row reductions are split over R = threads / 16 lanes, and the number of threads is a
//     function of Lk alone (64, 128 or 256).  A (batch entry, head) therefore gets the same bits whatever B is.
//   * exact fp32: fma chains on unsplit operands.  The softmax runs in base 2 as in attention.hip (v_exp_f32 on scores scaled
//     by scale * log2(e)).
#include <math.h>

#include "attention_common.h"

namespace {

constexpr int kMaxLk = 256;    // one thread per key

__host__ __device__ inline int score_stride(int Lk) { return Lk | 1; }

size_t lds_floats(int Lk, int d) { return (size_t)(Lk + 2 * kQC) * (d + 4) + 2 * (size_t)kQC * score_stride(Lk) + 4 * kQC; }

template <int DH>
__global__ __launch_bounds__(256) void attn_bwd_kernel(
    const float *__restrict__ q, dvis_strides qs, const float *__restrict__ k, dvis_strides ks_, const float *__restrict__ v,
    dvis_strides vs, const float *__restrict__ go, dvis_strides gs, float *__restrict__ dq, float *__restrict__ dk,
    float *__restrict__ dv, int B, int heads, int Lq, int Lk, float scale) {
  constexpr int LS = DH + 4, C4 = DH / 4;
  extern __shared__ float bwd_lds[];
  const int SS = score_stride(Lk);
  float *k_lds = bwd_lds;                  // Lk x LS
  float *q_lds = k_lds + Lk * LS;          // kQC x LS
  float *g_lds = q_lds + kQC * LS;         // kQC x LS   (dO)
  float *s_lds = g_lds + kQC * LS;         // kQC x SS   scores (log2 units), then dS
  float *p_lds = s_lds + kQC * SS;         // kQC x SS   dP
  float *st_lds = p_lds + kQC * SS;        // kQC x {m, 1 / l, D}

  const int tid = threadIdx.x, nthr = blockDim.x;
  const int R = nthr / kQC;                // lanes per row in the reductions: 4, 8 or 16
  const int bh = blockIdx.x;
  const int bi = bh / heads, hi = bh - bi * heads;
  const int C = heads * DH;
  const bool key_on = tid < Lk;
  const float sl2 = scale * kLog2e;

  const float *qb = q + (size_t)bi * qs.b + (size_t)hi * qs.h;
  const float *gb = go + (size_t)bi * gs.b + (size_t)hi * gs.h;
  const float *kb = k + (size_t)bi * ks_.b + (size_t)hi * ks_.h;
  const float *vb = v + (size_t)bi * vs.b + (size_t)hi * vs.h;

  for (int e = tid; e < Lk * C4; e += nthr) {
    const int row = e / C4, c4 = e - row * C4;
    *reinterpret_cast<float4 *>(&k_lds[row * LS + 4 * c4]) = *reinterpret_cast<const float4 *>(kb + (size_t)row * ks_.r + 4 * c4);
  }
  float4 vr[C4], dka[C4], dva[C4];
#pragma unroll
  for (int c = 0; c < C4; ++c) {
    vr[c] = key_on ? *reinterpret_cast<const float4 *>(vb + (size_t)tid * vs.r + 4 * c) : make_float4(0.f, 0.f, 0.f, 0.f);
    dka[c] = dva[c] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const float *krow = &k_lds[(key_on ? tid : 0) * LS];

  for (int q0 = 0; q0 < Lq; q0 += kQC) {
    // ---- (1) the chunk's rows of Q and dO; rows past Lq are zeros (they then add exact zeros to dK and dV)
    // (the text of bwd_load_chunk, inline: through the helper hipcc issues both global loads after both address computations, and
    // the d = 64 kernel measured 0.3 - 0.5 us of 275 slower at Lq 100, Lk 256)
    for (int e = tid; e < kQC * C4; e += nthr) {
      const int row = e / C4, c4 = e - row * C4;
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
      if (q0 + row < Lq) {
        a = *reinterpret_cast<const float4 *>(qb + (size_t)(q0 + row) * qs.r + 4 * c4);
        b = *reinterpret_cast<const float4 *>(gb + (size_t)(q0 + row) * gs.r + 4 * c4);
      }
      *reinterpret_cast<float4 *>(&q_lds[row * LS + 4 * c4]) = a;
      *reinterpret_cast<float4 *>(&g_lds[row * LS + 4 * c4]) = b;
    }
    __syncthreads();

    // ---- (2) this key's column: s = q_i . k_t (log2 units), dp = dO_i . v_t (bwd_dots says how, and why the loop stays rolled)
#pragma unroll 1
    for (int i = 0; key_on && i < kQC; ++i) {
      float s, dp;
      bwd_dots<DH>(krow, vr, &q_lds[i * LS], &g_lds[i * LS], &s, &dp);
      s_lds[i * SS + tid] = s * sl2;
      p_lds[i * SS + tid] = dp;
    }
    __syncthreads();

    // ---- (3) row statistics: R lanes per row, each over keys sub, sub + R, ..., then a butterfly over the R lanes
    {
      const int row = tid / R, sub = tid - row * R;
      const float *srow = &s_lds[row * SS], *prow = &p_lds[row * SS];
      float m = -INFINITY;
      for (int kk = sub; kk < Lk; kk += R) m = fmaxf(m, srow[kk]);
      for (int off = R >> 1; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
      float l = 0.f, dsum = 0.f;
      for (int kk = sub; kk < Lk; kk += R) {
        const float e = ex2(srow[kk] - m);
        l += e;
        dsum = fmaf(e, prow[kk], dsum);
      }
      for (int off = R >> 1; off > 0; off >>= 1) {
        l += __shfl_xor(l, off);
        dsum += __shfl_xor(dsum, off);
      }
      if (sub == 0) {
        const float inv = 1.f / l;        // l >= 1: the row's maximum contributes 2^0
        st_lds[row * 4] = m;
        st_lds[row * 4 + 1] = inv;
        st_lds[row * 4 + 2] = dsum * inv;
      }
    }
    __syncthreads();

    // ---- (4) P and dS of this key's column; dV[t] += P dO, dK[t] += dS Q; dS replaces the score in LDS for dQ
    // (threads past the last key own no column: they skip the step — no barrier inside — and touch no word another thread writes)
#pragma unroll 1
    for (int i = 0; key_on && i < kQC; ++i) {
      const int at = i * SS + tid;
      const float p = ex2(s_lds[at] - st_lds[i * 4]) * st_lds[i * 4 + 1];
      const float ds = p * (p_lds[at] - st_lds[i * 4 + 2]);
      s_lds[at] = ds;
      bwd_accumulate<DH>(p, ds, &q_lds[i * LS], &g_lds[i * LS], dka, dva);
    }
    __syncthreads();

    // ---- (5) dQ[i, c] = scale * sum_t dS[i, t] K[t, c], keys in ascending order
    for (int o = tid; o < kQC * DH; o += nthr) {
      const int i = o / DH, c = o - i * DH;
      if (q0 + i >= Lq) continue;
      const float *dsrow = &s_lds[i * SS];
      float acc = 0.f;
#pragma unroll 4
      for (int kk = 0; kk < Lk; ++kk) acc = fmaf(dsrow[kk], k_lds[kk * LS + c], acc);
      dq[((size_t)(q0 + i) * B + bi) * C + hi * DH + c] = acc * scale;
    }
    // (no barrier: the next chunk's step (1) writes q_lds / g_lds, last read before the barrier above, and its barrier
    // stands between these reads of s_lds and the next step (2))
  }

  if (key_on) {
    float *dkrow = dk + ((size_t)tid * B + bi) * C + hi * DH;
    float *dvrow = dv + ((size_t)tid * B + bi) * C + hi * DH;
    bwd_store_dkdv<DH>(dkrow, dvrow, dka, dva, scale);
  }
}

}  // namespace

// Threads per workgroup: one per key, rounded up to 64 / 128 / 256 — a function of Lk alone (see "determinism" above).  The launch
// takes its block size from here; tests ask the same function which geometry a case runs at.
DVIS_EXPORT int dvis_attention_backward_threads(int Lk) {
  if (Lk < 1 || Lk > kMaxLk) return 0;
  return Lk <= 64 ? 64 : Lk <= 128 ? 128 : 256;
}

DVIS_EXPORT int dvis_attention_backward(const float *q, const int64_t *q_strides, const float *k, const int64_t *k_strides,
                                        const float *v, const int64_t *v_strides, const float *grad_out, const int64_t *g_strides,
                                        float *dq, float *dk, float *dv, int B, int heads, int Lq, int Lk, int d, float scale,
                                        void *stream) {
  DVIS_REQUIRE(B >= 0 && heads > 0 && Lq >= 1 && Lk >= 1, "attention_backward: bad sizes");
  DVIS_REQUIRE(d == 32 || d == 64, "attention_backward: head dim must be 32 or 64 (got %d)", d);
  DVIS_REQUIRE(Lk <= kMaxLk, "attention_backward: serves at most %d keys (got Lk=%d)", kMaxLk, Lk);
  if (B == 0) return DVIS_OK;
  if (const int rc = attn_check_views("attention_backward", "q/k/v/grad_out", {q, k, v, grad_out, dq, dk, dv},
                                      {q_strides, k_strides, v_strides, g_strides}))
    return rc;
  DVIS_REQUIRE((long long)B * heads < (1ll << 31), "attention_backward: batch*heads must be below 2^31");
  const dvis_strides qs = dvis_strides_from(q_strides), ks = dvis_strides_from(k_strides);
  const dvis_strides vs = dvis_strides_from(v_strides), gs = dvis_strides_from(g_strides);
  const size_t lds = lds_floats(Lk, d) * sizeof(float);
  DVIS_REQUIRE(lds <= kLdsLimit, "attention_backward: %zu bytes of LDS exceed the %zu of a workgroup", lds, kLdsLimit);
  static DvisLdsOptIn opted32, opted64;
  if (const int rc = d == 32 ? dvis_lds_opt_in((const void *)attn_bwd_kernel<32>, lds, &opted32, "attn_bwd_kernel")
                             : dvis_lds_opt_in((const void *)attn_bwd_kernel<64>, lds, &opted64, "attn_bwd_kernel"))
    return rc;
  const int threads = dvis_attention_backward_threads(Lk);
  hipStream_t st = (hipStream_t)stream;
  if (d == 32)
    hipLaunchKernelGGL((attn_bwd_kernel<32>), dim3((unsigned)(B * heads)), dim3(threads), lds, st, q, qs, k, ks, v, vs, grad_out, gs,
                       dq, dk, dv, B, heads, Lq, Lk, scale);
  else
    hipLaunchKernelGGL((attn_bwd_kernel<64>), dim3((unsigned)(B * heads)), dim3(threads), lds, st, q, qs, k, ks, v, vs, grad_out, gs,
                       dq, dk, dv, B, heads, Lq, Lk, scale);
  return dvis_check_launch("attn_bwd_kernel");
}
