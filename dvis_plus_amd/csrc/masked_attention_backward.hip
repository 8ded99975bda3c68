// Backward of softmax(Q K^T * scale [+ mask]) V for LONG key sequences — gfx950, exact fp32 FMA, deterministic.
//
// Training-side counterpart of attention.hip for the masked cross-attention of the segmenter's transformer decoder
// (video_mask2former_transformer_decoder.py:258-361): 100 - 200 queries over every pixel of a stride-32 / 16 / 8 map (several hundred
// to about 15 000 keys), 8 heads of d = 32, and a per-query mask shared by the heads.  attention_backward.hip owns a (batch entry,
// head) with one workgroup and one thread per key, which ends at 256 keys; here the KEYS are cut into tiles of 256 over workgroups:
//   P = softmax(Q K^T * scale, blocked keys left out)    dV = P^T dO    dP = dO V^T    D = rowsum(P o dP)    dS = P o (dP - D)
//   dQ = scale * dS K                                     dK = scale * dS^T Q
// A blocked key has P = 0 exactly (a select, never arithmetic on infinities); a query row whose allowed_count is 0 ignores its mask
// (ibid. :296, as the forward kernel does on the device).
//
// Four launches, every one with a fixed summation order that depends on (Lq, Lk, d) alone:
//   (1) mab_tile_kernel<DH, 0>   grid (batch-head, key tile).  K of the tile -> LDS; the queries are walked in chunks of 16; thread t
//       computes its key's score and dP for the 16 rows (four fma chains over d, summed pairwise); 16 lanes per row reduce the
//       tile's maximum m_t, l_t = sum of 2^(s - m_t) and a_t = sum of 2^(s - m_t) dP over the ALLOWED keys (base 2 as in
//       attention.hip) -> workspace, three numbers per (tile, row).  A tile without an allowed key stores zeros.
//   (2) mab_rows_kernel          one thread per (batch-head, row): merges the tiles' triples in ascending tile order into the row's
//       (m, l) — kept as TWO numbers, so 16 allowed keys with equal scores give l = 16 and P = 1 / 16 exactly — and
//       D = sum_t a_t 2^(m_t - m) / l.  D comes from the probabilities this file recomputes, not from the forward's output
//       (rowsum(dO o O)): the two are equal in exact arithmetic, but the forward's scores carry another rounding, and with scores
//       of several hundred log2 units (an ulp of 6e-5 at 900) sum_t dS_t then misses 0 by that much times |dP| — which the large
//       common component of the keys turns into an error of dQ (6.6 x the fp32 CPU figure in the score-range test).
//   (3) mab_tile_kernel<DH, 1>   same grid and loop.  Thread t keeps V[t, :], dK[t, :] and dV[t, :] in registers; per row it computes
//       s and dP again (the same instructions: the same bits), P = 2^(s - m) / l (0 through a select where blocked), dS = P (dP - D), adds P dO to dV[t] and dS Q to dK[t] — the
//       queries in ascending order — and leaves dS in LDS; then the tile's share of dQ = dS K (keys of the tile in four interleaved
//       chains) goes to the workspace.  dK / dV belong to one workgroup: written once, no partials.
//   (4) mab_dq_kernel            dQ = scale * (sum of the tiles' shares in ascending tile order).
// No atomics, no scratch; a (batch entry, head)'s bits do not depend on B.  dQ goes through a workspace instead of a second kernel
// that walks the keys per query tile: that kernel would recompute every score and dP a third time (the expensive part), while the
// partials cost Lq * d floats per tile written and read once.
#include <math.h>

#include "attention_common.h"

namespace {

constexpr int kKT = 256;       // keys per tile = threads per workgroup: one thread per key
constexpr int kMaxLq = 256;
constexpr int kMaxLk = 65536;
constexpr int kSS = kKT + 1;   // row stride of the chunk's dS in LDS

struct mab_plan {
  int key_tile, query_tile, n_key_tiles, threads, k_rows;
  size_t lds_bytes;
};

mab_plan make_plan(int Lk, int d) {
  mab_plan p;
  p.key_tile = kKT;
  p.query_tile = kQC;
  p.n_key_tiles = (Lk + kKT - 1) / kKT;
  p.threads = kKT;
  p.k_rows = ((Lk < kKT ? Lk : kKT) + 3) & ~3;      // K rows held in LDS: a tile's keys, rounded up to the dQ loop's step of 4
  // K tile, the chunk's Q and dO, its scores / dS, its dP, its row statistics, its open flags
  p.lds_bytes = ((size_t)(p.k_rows + 2 * kQC) * (d + 4) + 2 * (size_t)kQC * kSS + 4 * kQC) * sizeof(float) + (size_t)kQC * kKT;
  return p;
}

// workspace sections (floats): row statistics {m, l, D, -} | per-tile {m_t, l_t, a_t, -} | per-tile dQ shares
size_t ws_stats(size_t BH, int Lq) { return BH * Lq * 4; }
size_t ws_pstats(size_t BH, int Lq, int nkt) { return BH * nkt * Lq * 4; }
size_t ws_part(size_t BH, int Lq, int nkt, int d) { return BH * nkt * Lq * d; }

// PASS 0: the tile's {m_t, l_t, a_t} per row -> pstats.  PASS 1: dK, dV and the tile's share of dQ -> part; reads stats.
template <int DH, int PASS>
__global__ __launch_bounds__(kKT) void mab_tile_kernel(
    const float *__restrict__ q, dvis_strides qs, const float *__restrict__ k, dvis_strides ks_, const float *__restrict__ v,
    dvis_strides vs, const float *__restrict__ go, dvis_strides gs, const uint8_t *__restrict__ mask,
    const int32_t *__restrict__ allowed, const float *__restrict__ stats, float *__restrict__ pstats, float *__restrict__ part,
    float *__restrict__ dk, float *__restrict__ dv, int B, int heads, int Lq, int Lk, int nkt, int k_rows, float scale) {
  constexpr int LS = DH + 4, C4 = DH / 4;
  extern __shared__ float mab_lds[];
  float *k_lds = mab_lds;                   // k_rows x LS
  float *q_lds = k_lds + k_rows * LS;       // kQC x LS
  float *g_lds = q_lds + kQC * LS;          // kQC x LS   (dO)
  float *s_lds = g_lds + kQC * LS;          // kQC x kSS  scores in log2 units (PASS 0) / dS (PASS 1)
  float *p_lds = s_lds + kQC * kSS;         // kQC x kSS  dP (PASS 0)
  float *st_lds = p_lds + kQC * kSS;        // kQC x {m, 1 / l, D, row uses its mask}
  uint8_t *o_lds = reinterpret_cast<uint8_t *>(st_lds + 4 * kQC);   // kQC x kKT   1 = the key is open for the row (PASS 0)

  const int tid = threadIdx.x;
  const int bh = blockIdx.x / nkt, tile = blockIdx.x - bh * nkt;
  const int bi = bh / heads, hi = bh - bi * heads;
  const int C = heads * DH;
  const int k0 = tile * kKT;
  const int nk = min(kKT, Lk - k0);         // keys of this tile
  const int key = k0 + tid;
  const bool key_on = tid < nk;
  const float sl2 = scale * kLog2e;

  const float *qb = q + (size_t)bi * qs.b + (size_t)hi * qs.h;
  const float *gb = go + (size_t)bi * gs.b + (size_t)hi * gs.h;
  const float *kb = k + (size_t)bi * ks_.b + (size_t)hi * ks_.h + (size_t)k0 * ks_.r;
  const float *vb = v + (size_t)bi * vs.b + (size_t)hi * vs.h;
  const uint8_t *mb = mask ? mask + (size_t)bi * Lq * Lk : nullptr;

  // the tile's K; the rows between nk and k_rows are zeros (the dQ loop runs over them)
  for (int e = tid; e < k_rows * C4; e += kKT) {
    const int row = e / C4, c4 = e - row * C4;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < nk) a = *reinterpret_cast<const float4 *>(kb + (size_t)row * ks_.r + 4 * c4);
    *reinterpret_cast<float4 *>(&k_lds[row * LS + 4 * c4]) = a;
  }
  // d = 32: the key's K row lives in registers next to its V row.  At d = 64 the registers are taken (256 with V, dK and dV): K
  // is read from LDS.
  constexpr bool kRegs = DH == 32;
  float4 vr[C4], kr[kRegs ? C4 : 1], dka[PASS ? C4 : 1], dva[PASS ? C4 : 1];
#pragma unroll
  for (int c = 0; c < C4; ++c) {
    vr[c] = key_on ? *reinterpret_cast<const float4 *>(vb + (size_t)key * vs.r + 4 * c) : make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (kRegs)
      kr[c] = key_on ? *reinterpret_cast<const float4 *>(kb + (size_t)tid * ks_.r + 4 * c) : make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (PASS != 0) dka[c] = dva[c] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const float *krow = &k_lds[(key_on ? tid : 0) * LS];

  for (int q0 = 0; q0 < Lq; q0 += kQC) {
    // the chunk's 16 mask bytes of this key, requested before anything waits (rows past Lq re-read the last row; their bits are
    // not used: such a row does not use its mask)
    unsigned blocked = 0;
    if (mb && key_on) {
#pragma unroll
      for (int i = 0; i < kQC; ++i) blocked |= (mb[(size_t)min(q0 + i, Lq - 1) * Lk + key] != 0 ? 1u : 0u) << i;
    }
    // ---- (1) the chunk's rows of Q and dO; rows past Lq are zeros.  PASS 1: the rows' statistics; a row past Lq gets 1 / l = 0,
    // so its P and dS are exact zeros
    bwd_load_chunk<DH>(q_lds, g_lds, qb, gb, qs.r, gs.r, q0, Lq, tid, kKT);
    if (tid < kQC) {
      const int row = q0 + tid;
      float m = 0.f, inv = 0.f, D = 0.f, masked = 0.f;
      if (row < Lq) {
        if (PASS) {
          const float *st = stats + ((size_t)bh * Lq + row) * 4;
          m = st[0];
          inv = st[1] > 0.f ? 1.f / st[1] : 0.f;      // l >= 1 whenever a key is allowed: its maximum contributes 2^0
          D = st[2];
        }
        if (mb && allowed[(size_t)bi * Lq + row] > 0) masked = 1.f;
      }
      st_lds[tid * 4] = m;
      st_lds[tid * 4 + 1] = inv;
      st_lds[tid * 4 + 2] = D;
      st_lds[tid * 4 + 3] = masked;
    }
    __syncthreads();

    // ---- (2) this key's column: s = q_i . k_t (log2 units), dp = dO_i . v_t (bwd_dots says how, and why the loop stays rolled)
#pragma unroll 1
    for (int i = 0; i < kQC; ++i) {
      float s = 0.f, dp = 0.f;
      bool open = false;
      if (key_on) {
        // (results in locals of this block: handing bwd_dots the addresses of s and dp, which live across the branch, cost 40 - 130
        // registers per thread)
        float s_raw, dp_raw;
        if constexpr (kRegs) bwd_dots<DH>(&kr[0], vr, &q_lds[i * LS], &g_lds[i * LS], &s_raw, &dp_raw);
        else bwd_dots<DH>(krow, vr, &q_lds[i * LS], &g_lds[i * LS], &s_raw, &dp_raw);
        // (__fmul_rn: never contracted with the subtraction of the row maximum — both passes must hold the same bits)
        s = __fmul_rn(s_raw, sl2);
        dp = dp_raw;
        open = true;
        if (st_lds[i * 4 + 3] != 0.f) open = ((blocked >> i) & 1u) == 0;
      }
      if constexpr (PASS == 0) {
        s_lds[i * kSS + tid] = s;
        p_lds[i * kSS + tid] = dp;
        o_lds[i * kKT + tid] = open ? 1 : 0;
      } else {
        // P and dS of this key for row i; a blocked key (and a thread past the tile's last key) takes exact zeros through the select
        const float p = open ? ex2(s - st_lds[i * 4]) * st_lds[i * 4 + 1] : 0.f;
        const float ds = open ? p * (dp - st_lds[i * 4 + 2]) : 0.f;
        s_lds[i * kSS + tid] = ds;
        bwd_accumulate<DH>(p, ds, &q_lds[i * LS], &g_lds[i * LS], dka, dva);
      }
    }
    __syncthreads();

    if constexpr (PASS == 0) {
      // ---- (3) the tile's maximum, sum and sum of 2^(s - max) dP per row over its open keys: 16 lanes per row, each over keys sub,
      // sub + 16, ..., then a butterfly over the 16 lanes
      constexpr int R = kKT / kQC;
      const int row = tid / R, sub = tid - row * R;
      const float *srow = &s_lds[row * kSS], *prow = &p_lds[row * kSS];
      const uint8_t *orow = &o_lds[row * kKT];
      float m = -INFINITY;
      int any = 0;
      for (int kk = sub; kk < nk; kk += R) {
        const bool open = orow[kk] != 0;
        m = open ? fmaxf(m, srow[kk]) : m;
        any |= open ? 1 : 0;
      }
      for (int off = R >> 1; off > 0; off >>= 1) {
        m = fmaxf(m, __shfl_xor(m, off));
        any |= __shfl_xor(any, off);
      }
      m = any ? m : 0.f;
      float l = 0.f, a = 0.f;
      for (int kk = sub; kk < nk; kk += R) {
        const bool open = orow[kk] != 0;
        const float e = open ? ex2(open ? srow[kk] - m : 0.f) : 0.f;
        l += e;
        a = fmaf(e, prow[kk], a);
      }
      for (int off = R >> 1; off > 0; off >>= 1) {
        l += __shfl_xor(l, off);
        a += __shfl_xor(a, off);
      }
      if (sub == 0 && q0 + row < Lq)
        *reinterpret_cast<float4 *>(pstats + (((size_t)bh * nkt + tile) * Lq + q0 + row) * 4) = make_float4(m, l, a, 0.f);
    } else {
      // ---- (4) the tile's share of dQ[i, c] = sum_t dS[i, t] K[t, c]: keys t, t + 4, ... in four chains, summed pairwise
      for (int o = tid; o < kQC * DH; o += kKT) {
        const int i = o / DH, c = o - i * DH;
        if (q0 + i >= Lq) continue;
        const float *dsrow = &s_lds[i * kSS];
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        for (int kk = 0; kk < k_rows; kk += 4) {
          a0 = fmaf(dsrow[kk], k_lds[kk * LS + c], a0);
          a1 = fmaf(dsrow[kk + 1], k_lds[(kk + 1) * LS + c], a1);
          a2 = fmaf(dsrow[kk + 2], k_lds[(kk + 2) * LS + c], a2);
          a3 = fmaf(dsrow[kk + 3], k_lds[(kk + 3) * LS + c], a3);
        }
        part[(((size_t)bh * nkt + tile) * Lq + q0 + i) * DH + c] = (a0 + a1) + (a2 + a3);
      }
    }
    // (no barrier: the next chunk's step (1) writes q_lds / g_lds / st_lds, last read before the barrier above, and its barrier
    // stands between these reads of s_lds / p_lds / o_lds and the next step (2))
  }

  if constexpr (PASS != 0) {
    const size_t at = ((size_t)key * B + bi) * C + hi * DH;
    if (key_on) bwd_store_dkdv<DH>(dk + at, dv + at, dka, dva, scale);
  }
}

// One thread per (batch-head, row): (m, l, D) from the tiles' triples in ascending tile order.
__global__ __launch_bounds__(256) void mab_rows_kernel(const float *__restrict__ pstats, float *__restrict__ stats, size_t rows, int Lq,
                                                       int nkt) {
  const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const size_t bh = r / Lq;
  const int row = (int)(r - bh * Lq);
  const float4 *ps = reinterpret_cast<const float4 *>(pstats) + (bh * nkt * Lq + row);
  float m = -INFINITY;
  int any = 0;
  for (int t = 0; t < nkt; ++t) {
    const float4 st = ps[(size_t)t * Lq];
    const bool has = st.y > 0.f;
    m = has ? fmaxf(m, st.x) : m;
    any |= has ? 1 : 0;
  }
  m = any ? m : 0.f;
  float l = 0.f, a = 0.f;
  for (int t = 0; t < nkt; ++t) {
    const float4 st = ps[(size_t)t * Lq];
    const bool has = st.y > 0.f;
    const float e = has ? ex2(has ? st.x - m : 0.f) : 0.f;
    l = fmaf(st.y, e, l);
    a = fmaf(st.z, e, a);
  }
  *reinterpret_cast<float4 *>(stats + r * 4) = make_float4(m, l, l > 0.f ? a * (1.f / l) : 0.f, 0.f);
}

// dQ = scale * (the tiles' shares added in ascending tile order); one thread per four channels of a (batch-head, row).
template <int DH>
__global__ __launch_bounds__(256) void mab_dq_kernel(const float *__restrict__ part, float *__restrict__ dq, size_t items, int B,
                                                     int heads, int Lq, int nkt, float scale) {
  constexpr int C4 = DH / 4;
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= items) return;
  const int c4 = (int)(e % C4);
  const size_t r = e / C4;
  const size_t bh = r / Lq;
  const int row = (int)(r - bh * Lq);
  const int bi = (int)(bh / heads), hi = (int)(bh - (size_t)bi * heads);
  const float *p = part + ((bh * nkt * Lq + row) * DH + 4 * c4);
  float4 acc = *reinterpret_cast<const float4 *>(p);
  for (int t = 1; t < nkt; ++t) {
    const float4 a = *reinterpret_cast<const float4 *>(p + (size_t)t * Lq * DH);
    acc.x += a.x;
    acc.y += a.y;
    acc.z += a.z;
    acc.w += a.w;
  }
  *reinterpret_cast<float4 *>(dq + ((size_t)row * B + bi) * heads * DH + hi * DH + 4 * c4) =
      make_float4(acc.x * scale, acc.y * scale, acc.z * scale, acc.w * scale);
}

int check_sizes(const char *who, int Lq, int Lk, int d) {
  DVIS_REQUIRE(d == 32 || d == 64, "%s: head dim must be 32 or 64 (got %d)", who, d);
  DVIS_REQUIRE(Lq >= 1 && Lq <= kMaxLq, "%s: serves 1 .. %d queries (got Lq=%d)", who, kMaxLq, Lq);
  DVIS_REQUIRE(Lk >= 1 && Lk <= kMaxLk, "%s: serves 1 .. %d keys (got Lk=%d)", who, kMaxLk, Lk);
  return DVIS_OK;
}

template <int DH>
int launch(const float *q, dvis_strides qs, const float *k, dvis_strides ks, const float *v, dvis_strides vs, const float *go,
           dvis_strides gs, const uint8_t *mask, const int32_t *allowed, float *dq, float *dk, float *dv, int B, int heads, int Lq,
           int Lk, float scale, float *ws, const mab_plan &plan, hipStream_t st) {
  const size_t BH = (size_t)B * heads;
  const int nkt = plan.n_key_tiles;
  float *stats = ws, *pstats = stats + ws_stats(BH, Lq), *part = pstats + ws_pstats(BH, Lq, nkt);
  static DvisLdsOptIn opted0, opted1;
  if (const int rc = dvis_lds_opt_in((const void *)mab_tile_kernel<DH, 0>, plan.lds_bytes, &opted0, "mab_tile_kernel")) return rc;
  if (const int rc = dvis_lds_opt_in((const void *)mab_tile_kernel<DH, 1>, plan.lds_bytes, &opted1, "mab_tile_kernel")) return rc;
  const dim3 grid((unsigned)(BH * nkt)), block(plan.threads);
  hipLaunchKernelGGL((mab_tile_kernel<DH, 0>), grid, block, plan.lds_bytes, st, q, qs, k, ks, v, vs, go, gs, mask, allowed,
                     (const float *)stats, pstats, part, dk, dv, B, heads, Lq, Lk, nkt, plan.k_rows, scale);
  if (const int rc = dvis_check_launch("mab_tile_kernel<stats>")) return rc;
  const size_t rows = BH * Lq;
  hipLaunchKernelGGL(mab_rows_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, (const float *)pstats, stats, rows, Lq,
                     nkt);
  if (const int rc = dvis_check_launch("mab_rows_kernel")) return rc;
  hipLaunchKernelGGL((mab_tile_kernel<DH, 1>), grid, block, plan.lds_bytes, st, q, qs, k, ks, v, vs, go, gs, mask, allowed,
                     (const float *)stats, pstats, part, dk, dv, B, heads, Lq, Lk, nkt, plan.k_rows, scale);
  if (const int rc = dvis_check_launch("mab_tile_kernel<grads>")) return rc;
  const size_t items = rows * (DH / 4);
  hipLaunchKernelGGL((mab_dq_kernel<DH>), dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, (const float *)part, dq, items, B,
                     heads, Lq, nkt, scale);
  return dvis_check_launch("mab_dq_kernel");
}

}  // namespace

// How the launch cuts the work: one thread per key, 256 keys per workgroup, the queries in chunks of 16 inside it.  The launch takes
// its grid, block and LDS size from make_plan; tests ask the same function.
DVIS_EXPORT int dvis_masked_attention_backward_plan(int Lq, int Lk, int d, int32_t *plan) {
  DVIS_REQUIRE(plan != nullptr, "masked_attention_backward_plan: null pointer");
  if (const int rc = check_sizes("masked_attention_backward_plan", Lq, Lk, d)) return rc;
  const mab_plan p = make_plan(Lk, d);
  plan[0] = p.key_tile;
  plan[1] = p.query_tile;
  plan[2] = p.n_key_tiles;
  plan[3] = p.threads;
  plan[4] = (int32_t)p.lds_bytes;
  return DVIS_OK;
}

DVIS_EXPORT int64_t dvis_masked_attention_backward_ws_bytes(int BH, int Lq, int Lk, int d) {
  if (BH <= 0 || Lq < 1 || Lq > kMaxLq || Lk < 1 || Lk > kMaxLk || (d != 32 && d != 64)) return 0;
  const int nkt = make_plan(Lk, d).n_key_tiles;
  return (int64_t)((ws_stats(BH, Lq) + ws_pstats(BH, Lq, nkt) + ws_part(BH, Lq, nkt, d)) * sizeof(float));
}

DVIS_EXPORT int dvis_masked_attention_backward(const float *q, const int64_t *q_strides, const float *k, const int64_t *k_strides,
                                               const float *v, const int64_t *v_strides,
                                               const float *grad_out, const int64_t *g_strides, const uint8_t *mask,
                                               const int32_t *allowed_count, float *dq, float *dk, float *dv, int B, int heads, int Lq,
                                               int Lk, int d, float scale, void *ws, void *stream) {
  DVIS_REQUIRE(B >= 0 && heads > 0, "masked_attention_backward: bad sizes");
  if (const int rc = check_sizes("masked_attention_backward", Lq, Lk, d)) return rc;
  if (B == 0) return DVIS_OK;
  if (const int rc = attn_check_views("masked_attention_backward", "q/k/v/grad_out", {q, k, v, grad_out, dq, dk, dv, ws},
                                      {q_strides, k_strides, v_strides, g_strides}))
    return rc;
  DVIS_REQUIRE(mask == nullptr || allowed_count != nullptr, "masked_attention_backward: a mask needs its allowed_count");
  const mab_plan plan = make_plan(Lk, d);
  DVIS_REQUIRE((long long)B * heads * plan.n_key_tiles < (1ll << 31),
               "masked_attention_backward: batch*heads*key tiles must be below 2^31");
  const dvis_strides qs = dvis_strides_from(q_strides), ks = dvis_strides_from(k_strides);
  const dvis_strides vs = dvis_strides_from(v_strides), gs = dvis_strides_from(g_strides);
  DVIS_REQUIRE(plan.lds_bytes <= kLdsLimit, "masked_attention_backward: %zu bytes of LDS exceed the %zu of a workgroup",
               plan.lds_bytes, kLdsLimit);
  hipStream_t st = (hipStream_t)stream;
  return d == 32 ? launch<32>(q, qs, k, ks, v, vs, grad_out, gs, mask, allowed_count, dq, dk, dv, B, heads, Lq, Lk, scale,
                              (float *)ws, plan, st)
                 : launch<64>(q, qs, k, ks, v, vs, grad_out, gs, mask, allowed_count, dq, dk, dv, B, heads, Lq, Lk, scale,
                              (float *)ws, plan, st);
}
