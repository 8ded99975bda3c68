// Shifted-window attention of the Swin backbone (mask2former/modeling/backbone/swin.py:131-171, 235-295, 413-440) as ONE kernel
// over the block's qkv projection on the UNPADDED token grid: F.pad, both torch.roll, window partition / reverse, the qkv permute,
// the relative-position-bias gather, the region mask, softmax, both products and the crop are index arithmetic on one read of the
// qkv rows and one write of the output rows.  Contract: include/dvis_hip.h.
//
// One workgroup = one (frame, window, head).  K and V of the window's N = ws^2 tokens (pad tokens: the qkv bias) and the head's
// raw bias table live in LDS; every wave owns 16-query tiles.  All products are v_mfma_f32_16x16x4_f32 (an fp32 fma chain):
//   S^T tile (16 keys x 16 queries) = K_tile (16 x 32) Q^T (32 x 16)   A = K from LDS (2 x ds_read_b128 per lane), B = Q in registers
//     -> lane (j = lane & 15, g = lane >> 4) holds the scores of query j against keys 16 t + 4 g + r, r = 0..3, of every key tile t:
//        a score row lives in the 4 lanes {j, j + 16, j + 32, j + 48}; max / sum = in-lane, then two cross-lane steps.
//   O^T (32 x 16 queries) = V^T P^T: the contraction runs over the keys in the order the score registers hold them (step r of tile
//     t contracts keys 16 t + 4 g + r), so P^T is the B operand as it stands: no transpose, no LDS round trip.  The A tile's 16 rows
//     are the head columns {2 i} (first accumulator) and {2 i + 1} (second): one ds_read_b64 of V per step, and a lane ends up with
//     the 8 consecutive columns 8 g .. 8 g + 7 of its query: two 16-byte stores.
// The contraction over the head dim likewise takes the columns in the order 8 g + s (step s): 32 contiguous bytes per lane.
// Exact fp32, no atomics, no workspace, fixed order: the same bits every call, and a frame's bits do not depend on B.
#include "dvis_common.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int WA_D = 32;    // head dim served
constexpr int WA_KS = 36;   // K row stride in floats: the 16 rows of a ds_read_b128 lane group fall on 16 distinct 16-byte slots
constexpr int WA_VS = 40;   // V row stride in floats: the two key rows of a ds_read_b64 half-wave fall on disjoint bank halves

template <int WS> struct WaCfg {
  static constexpr int N = WS * WS;
  static constexpr int NT = (N + 15) / 16;              // 16-token tiles (queries and keys)
  static constexpr int NP = NT * 16;
  static constexpr int WAVES = NT % 3 == 0 ? 3 : 4;     // ws = 12: 9 tiles on 3 waves; ws = 7: 4 tiles on 4 waves
  static constexpr int THREADS = WAVES * 64;
  static constexpr int TB = 2 * WS - 1;
  static constexpr int TN = TB * TB;
};

__device__ __forceinline__ int wa_region(int n, int Np, int ws, int shift) { return (n >= Np - ws) + (n >= Np - shift); }

template <int WS>
__global__ __launch_bounds__(WaCfg<WS>::THREADS) __attribute__((amdgpu_waves_per_eu(3))) void window_attention_kernel(
    const float *__restrict__ qkv, const float *__restrict__ qkv_bias, const float *__restrict__ table, float *__restrict__ out,
    int H, int W, int Hp, int Wp, int heads, int shift, float scale) {
  using Cfg = WaCfg<WS>;
  constexpr int N = Cfg::N, NT = Cfg::NT, NP = Cfg::NP, TB = Cfg::TB, TN = Cfg::TN;
  constexpr bool TAIL = N % 16 != 0;      // ws = 7: the last tile holds one token; ws = 12: nine full tiles
  __shared__ __attribute__((aligned(16))) float sK[NP * WA_KS];
  __shared__ __attribute__((aligned(16))) float sV[NP * WA_VS];
  __shared__ float sT[TN];
  __shared__ int sRow[NP];   // source row of a window token in its frame; -1: pad token; -2: beyond the window (tile tail)
  // per token: (region id of its shifted coordinate << 16) | (ly * (2 ws - 1) + lx), the token's term of the bias-table index
  __shared__ __attribute__((aligned(16))) int sKey[NP];

  const int tid = threadIdx.x;
  const int nWw = Wp / WS, nW = (Hp / WS) * nWw;
  const unsigned unit = blockIdx.x;
  const int head = unit % heads;
  const int win = (unit / heads) % nW;
  const int frame = unit / heads / nW;
  const int wy = win / nWw, wx = win % nWw;
  const int C = heads * WA_D;
  // per-frame bases in 64 bits; inside a frame every offset is below 2^31 bytes (checked by the caller)
  const float *fq = qkv + (size_t)frame * ((size_t)H * W * 3 * C);
  float *fo = out + (size_t)frame * ((size_t)H * W * C);

  for (int n = tid; n < NP; n += Cfg::THREADS) {
    int row = -2, reg = 0;
    if (n < N) {
      const int ys = wy * WS + n / WS, xs = wx * WS + n % WS;
      int sy = ys + shift, sx = xs + shift;
      sy -= sy >= Hp ? Hp : 0;
      sx -= sx >= Wp ? Wp : 0;
      row = (sy < H && sx < W) ? sy * W + sx : -1;
      if (shift > 0) reg = 3 * wa_region(ys, Hp, WS, shift) + wa_region(xs, Wp, WS, shift);
    }
    sRow[n] = row;
    sKey[n] = n < N ? (reg << 16) | ((n / WS) * TB + n % WS) : 0;
  }
  for (int i = tid; i < TN; i += Cfg::THREADS) sT[i] = table[(size_t)i * heads + head];
  __syncthreads();

  // K and V rows of the window: 16 float4 per token (8 of K, 8 of V), and the Q fragments of the wave's query tiles.  Every load is
  // unconditional (a pad or tail token reads the bias or a valid dummy address and is zeroed by a select), so that all of a
  // thread's loads are in flight together: one global round trip per workgroup, not one per loop turn.
  constexpr int LD = NP * 16 / Cfg::THREADS, QT = NT / Cfg::WAVES;
  static_assert(NP * 16 % Cfg::THREADS == 0 && NT % Cfg::WAVES == 0, "whole turns");
  const int lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, g = lane >> 4;
  const dvis_f4 zero4 = {0.f, 0.f, 0.f, 0.f};
  dvis_f4 kv[LD], qa[QT], qb[QT];
#pragma unroll
  for (int i = 0; i < LD; ++i) {
    const int it = tid + i * Cfg::THREADS;
    const int n = it >> 4, part = (it >> 3) & 1, c4 = it & 7;
    const int row = sRow[n];
    const unsigned col = (unsigned)(1 + part) * C + head * WA_D + c4 * 4;
    const float *src = row >= 0 ? fq + (unsigned)row * (unsigned)(3 * C) + col : (qkv_bias != nullptr ? qkv_bias + col : fq + col);
    kv[i] = *(const dvis_f4 *)src;
    if (row == -2 || (row == -1 && qkv_bias == nullptr)) kv[i] = zero4;
  }
#pragma unroll
  for (int i = 0; i < QT; ++i) {
    const int qn_raw = (wave + i * Cfg::WAVES) * 16 + j;
    const int qrow = sRow[qn_raw < N ? qn_raw : N - 1];
    const unsigned col = (unsigned)head * WA_D + 8 * g;
    const float *src = qrow >= 0 ? fq + (unsigned)qrow * (unsigned)(3 * C) + col : (qkv_bias != nullptr ? qkv_bias + col : fq + col);
    qa[i] = *(const dvis_f4 *)src;
    qb[i] = *(const dvis_f4 *)(src + 4);
    if (qrow < 0 && qkv_bias == nullptr) qa[i] = qb[i] = zero4;
  }
#pragma unroll
  for (int i = 0; i < LD; ++i) {
    const int it = tid + i * Cfg::THREADS;
    const int n = it >> 4, part = (it >> 3) & 1, c4 = it & 7;
    float *dst = part ? sV + n * WA_VS + c4 * 4 : sK + n * WA_KS + c4 * 4;
    *(dvis_f4 *)dst = kv[i];
  }
  __syncthreads();

#pragma unroll
  for (int qi = 0; qi < QT; ++qi) {
    const int qt = wave + qi * Cfg::WAVES;
    // K and V stay in LDS: without this the compiler hoists every (query-tile-invariant) LDS read out of the loop, 144 registers
    int lds0 = 0;
    asm volatile("" : "+v"(lds0));
    const int qn_raw = qt * 16 + j;
    const int qn = qn_raw < N ? qn_raw : N - 1;       // a tail lane repeats the last query and writes nothing
    const int qrow = sRow[qn];
    const int qkey = sKey[qn];
    const int qreg = qkey >> 16;
    const int qoff = (qkey & 0xffff) + (WS - 1) * TB + (WS - 1);      // table index = qoff - (ky (2 ws - 1) + kx)
    // B operand of S^T: Q[qn][8 g + s] * scale, s = 0..7 (pad token: the bias)
    const dvis_f4 a = qa[qi], b = qb[qi];
    const float qf[8] = {a.x * scale, a.y * scale, a.z * scale, a.w * scale, b.x * scale, b.y * scale, b.z * scale, b.w * scale};

    dvis_f4 s[NT];
    float m = -INFINITY;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const float *kp = sK + lds0 + (t * 16 + j) * WA_KS + 8 * g;
      const dvis_f4 k0 = *(const dvis_f4 *)kp, k1 = *(const dvis_f4 *)(kp + 4);
      dvis_f4 acc = {0.f, 0.f, 0.f, 0.f};
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(k0.x, qf[0], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(k0.y, qf[1], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(k0.z, qf[2], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(k0.w, qf[3], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(k1.x, qf[4], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(k1.y, qf[5], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(k1.z, qf[6], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(k1.w, qf[7], acc, 0, 0, 0);
      const dvis_v4u kk = *(const dvis_v4u *)(sKey + lds0 + t * 16 + 4 * g);      // the lane's four keys of this tile
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = acc[r] + sT[qoff - (int)(kk[r] & 0xffffu)];
        if ((int)(kk[r] >> 16) != qreg) v += -100.f;
        if (TAIL && t * 16 + 4 * g + r >= N) v = -INFINITY;
        acc[r] = v;
        m = fmaxf(m, v);
      }
      s[t] = acc;
    }
    m = fmaxf(m, __shfl_xor(m, 16));
    m = fmaxf(m, __shfl_xor(m, 32));

    float l = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = (TAIL && t * 16 + 4 * g + r >= N) ? 0.f : expf(s[t][r] - m);
        s[t][r] = p;
        l += p;
      }
    }
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);

    dvis_f4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = o0;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float2 v = *(const float2 *)(sV + lds0 + (t * 16 + 4 * g + r) * WA_VS + 2 * j);
        o0 = __builtin_amdgcn_mfma_f32_16x16x4f32(v.x, s[t][r], o0, 0, 0, 0);
        o1 = __builtin_amdgcn_mfma_f32_16x16x4f32(v.y, s[t][r], o1, 0, 0, 0);
      }
    }
    if (qn_raw < N && qrow >= 0) {      // the reverse roll and the crop: only un-padded source positions are written
      float *op = fo + (unsigned)qrow * (unsigned)C + head * WA_D + 8 * g;
      const dvis_f4 lo = {o0[0] / l, o1[0] / l, o0[1] / l, o1[1] / l};
      const dvis_f4 hi = {o0[2] / l, o1[2] / l, o0[3] / l, o1[3] / l};
      *(dvis_f4 *)op = lo;
      *(dvis_f4 *)(op + 4) = hi;
    }
  }
}

template <int WS>
int wa_launch(const float *qkv, const float *qkv_bias, const float *table, float *out, int H, int W, int Hp, int Wp, int heads,
              int shift, float scale, unsigned units, hipStream_t st) {
  hipLaunchKernelGGL(window_attention_kernel<WS>, dim3(units), dim3(WaCfg<WS>::THREADS), 0, st, qkv, qkv_bias, table, out, H, W, Hp, Wp,
                     heads, shift, scale);
  return dvis_check_launch("dvis_window_attention");
}

}  // namespace

DVIS_EXPORT int dvis_window_attention_supported(int ws, int d) { return d == WA_D && (ws == 7 || ws == 12); }

DVIS_EXPORT int dvis_window_attention(const float *qkv, const float *qkv_bias, const float *bias_table, float *out, int B, int H, int W,
                                      int heads, int d, int ws, int shift, float scale, void *stream) {
  DVIS_REQUIRE(dvis_window_attention_supported(ws, d),
               "dvis_window_attention: window size ws=%d with head dim d=%d is not served (served: d=32 with ws=7 or ws=12)", ws, d);
  DVIS_REQUIRE(B >= 0 && H > 0 && W > 0 && heads > 0, "dvis_window_attention: bad sizes B=%d H=%d W=%d heads=%d", B, H, W, heads);
  DVIS_REQUIRE(shift >= 0 && shift < ws, "dvis_window_attention: shift=%d must lie in [0, ws=%d)", shift, ws);
  DVIS_REQUIRE(qkv != nullptr && bias_table != nullptr && out != nullptr, "dvis_window_attention: null qkv / bias_table / out");
  DVIS_REQUIRE((((uintptr_t)qkv | (uintptr_t)out | (uintptr_t)qkv_bias) & 15) == 0,
               "dvis_window_attention: qkv, qkv_bias and out must be 16-byte aligned");
  const int64_t frame_bytes = (int64_t)H * W * 3 * heads * d * 4;
  DVIS_REQUIRE(frame_bytes < ((int64_t)1 << 31),
               "dvis_window_attention: one frame's qkv is %lld bytes; offsets inside a frame are 32-bit (below 2^31 bytes)",
               (long long)frame_bytes);
  const int nWh = (H + ws - 1) / ws, nWw = (W + ws - 1) / ws;
  const int64_t units = (int64_t)B * nWh * nWw * heads;
  DVIS_REQUIRE(units <= INT_MAX, "dvis_window_attention: %lld (frame, window, head) units exceed the grid", (long long)units);
  if (units == 0) return DVIS_OK;
  hipStream_t st = (hipStream_t)stream;
  if (ws == 7) return wa_launch<7>(qkv, qkv_bias, bias_table, out, H, W, nWh * ws, nWw * ws, heads, shift, scale, (unsigned)units, st);
  return wa_launch<12>(qkv, qkv_bias, bias_table, out, H, W, nWh * ws, nWw * ws, heads, shift, scale, (unsigned)units, st);
}
