// Depthwise 7 x 7 convolution + bias + LayerNorm over the channels on a TOKEN-major map: the first half of a ConvNeXt block (conv_dw,
// permute to NHWC, norm — everything up to the input of mlp.fc1) as ONE kernel: one read of the map, one write of the normalised
// rows, no NCHW round trip and no stored pre-norm tensor.  Contract: include/dvis_hip.h.
//
// One workgroup = one run of DL_RUN = 8 neighbouring tokens of a map row, all C channels: lane `tid` owns channels 4 tid .. 4 tid + 3
// (one 16-byte load per token), NW = ceil(C / 256) waves.  Per kernel row ky the lane loads the 8 + 6 tokens of the run's window in
// that row (out-of-map positions read a clamped address and are replaced by zeros) and the 4 x 7 weights of the row, and feeds the
// 8 x 4 accumulators: an output's 49 taps are ONE fma chain, ky outer and kx inner, padding taps included as zeros — its bits do not
// depend on where the pixel falls in a run, on B or on its batch mates.  The conv results never leave the registers: the channel
// mean is reduced first (in-lane (x + y) + (z + w), six xor steps inside the wave, then the waves' partial sums added in wave order
// from LDS), then the sum of squared deviations from that mean the same way — never E[z^2] - mean^2.  The reduction's shape is a
// function of C alone.  Exact fp32, no atomics, no workspace: the same bits every call.
#include "dvis_common.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int DL_RUN = 8;       // output tokens per workgroup, along x
constexpr int DL_MAX_C = 1536;  // 6 waves x 64 lanes x 4 channels

__device__ __forceinline__ float dl_wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// One kernel row of the lane's 4 channels: 4 runs of 7 consecutive floats (stride 49), each one dwordx4 + one dwordx3 load at a
// 4-byte-aligned address.  The lane's 49 x 4 weights do not fit in registers beside the window, so the ky loop stays rolled and
// takes them a row at a time (unrolled, the compiler gathers all 196 at the top: 250 registers and scratch).
typedef float dl_f4u __attribute__((ext_vector_type(4), aligned(4)));
typedef float dl_f3u __attribute__((ext_vector_type(3), aligned(4)));
__device__ __forceinline__ void dl_load_weights(const float *p, float (&k)[4][7]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const dl_f4u a = *(const dl_f4u *)(p + j * 49);
    const dl_f3u b = *(const dl_f3u *)(p + j * 49 + 4);
    k[j][0] = a.x, k[j][1] = a.y, k[j][2] = a.z, k[j][3] = a.w, k[j][4] = b.x, k[j][5] = b.y, k[j][6] = b.z;
  }
}

// Sum over the workgroup of one value per (lane, token): every lane gets the same total.  Waves are added in wave order.
template <int NW>
__device__ __forceinline__ void dl_block_sum(float (&v)[DL_RUN], float (*part)[DL_RUN], int wave, int lane) {
#pragma unroll
  for (int o = 0; o < DL_RUN; ++o) v[o] = dl_wave_sum(v[o]);
  if (NW == 1) return;
  if (lane == 0) {
#pragma unroll
    for (int o = 0; o < DL_RUN; ++o) part[wave][o] = v[o];
  }
  __syncthreads();
#pragma unroll
  for (int o = 0; o < DL_RUN; ++o) {
    float s = part[0][o];
#pragma unroll
    for (int k = 1; k < NW; ++k) s += part[k][o];
    v[o] = s;
  }
}

template <int NW>
__global__ __launch_bounds__(NW * 64) void dwconv7x7_ln_tokens_kernel(const float *__restrict__ x, float *__restrict__ out,
                                                                      int64_t batch_stride, int h, int w, int C, int xruns,
                                                                      const float *__restrict__ wt, const float *__restrict__ bias,
                                                                      const float *__restrict__ gamma, const float *__restrict__ beta,
                                                                      float eps) {
  __shared__ float sSum[NW][DL_RUN], sSq[NW][DL_RUN];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool active = 4 * tid < C;          // lanes beyond C compute on channel 0..3 and contribute zeros
  const int c4 = active ? 4 * tid : 0;
  const unsigned unit = blockIdx.x;
  const int x0 = (int)(unit % (unsigned)xruns) * DL_RUN;
  const unsigned r = unit / (unsigned)xruns;
  const int y = (int)(r % (unsigned)h);
  const size_t b = r / (unsigned)h;
  // per-frame base in 64 bits; inside a frame every element offset is below 2^29 (the caller checked 2^31 bytes)
  const float *xb = x + b * (size_t)batch_stride + c4;
  const float *wl = (const float *)__builtin_assume_aligned(wt + (size_t)c4 * 49, 16);

  const dvis_f4 zero4 = {0.f, 0.f, 0.f, 0.f};
  const dvis_f4 bv = bias != nullptr ? *(const dvis_f4 *)(bias + c4) : zero4;
  dvis_f4 acc[DL_RUN];
#pragma unroll
  for (int o = 0; o < DL_RUN; ++o) acc[o] = bv;

  unsigned xmask = 0u;
#pragma unroll
  for (int i = 0; i < DL_RUN + 6; ++i) xmask |= (x0 + i - 3 >= 0 && x0 + i - 3 < w) ? 1u << i : 0u;
  float k[4][7];
#pragma unroll 1
  for (int ky = 0; ky < 7; ++ky) {
    dl_load_weights(wl + ky * 7, k);
    const int yy = y + ky - 3;
    const unsigned ymask = yy >= 0 && yy < h ? xmask : 0u;      // bit i: window column i of this row lies inside the map
    const int yc = yy < 0 ? 0 : (yy >= h ? h - 1 : yy);
    const float *row = xb + (unsigned)(yc * w) * (unsigned)C;
    dvis_f4 col[DL_RUN + 6];
#pragma unroll
    for (int i = 0; i < DL_RUN + 6; ++i) {
      const int xx = x0 + i - 3;
      const int xc = xx < 0 ? 0 : (xx >= w ? w - 1 : xx);
      const dvis_f4 v = *(const dvis_f4 *)(row + (unsigned)xc * (unsigned)C);
      col[i] = (ymask >> i) & 1u ? v : zero4;
    }
#pragma unroll
    for (int o = 0; o < DL_RUN; ++o)
#pragma unroll
      for (int kx = 0; kx < 7; ++kx) {
        const dvis_f4 v = col[o + kx];
        acc[o].x = __builtin_fmaf(k[0][kx], v.x, acc[o].x), acc[o].y = __builtin_fmaf(k[1][kx], v.y, acc[o].y);
        acc[o].z = __builtin_fmaf(k[2][kx], v.z, acc[o].z), acc[o].w = __builtin_fmaf(k[3][kx], v.w, acc[o].w);
      }
  }

  const float inv_c = 1.f / (float)C;
  float m[DL_RUN], q[DL_RUN];
#pragma unroll
  for (int o = 0; o < DL_RUN; ++o) m[o] = active ? (acc[o].x + acc[o].y) + (acc[o].z + acc[o].w) : 0.f;
  dl_block_sum<NW>(m, sSum, wave, lane);
#pragma unroll
  for (int o = 0; o < DL_RUN; ++o) {
    m[o] *= inv_c;
    acc[o] -= m[o];
    q[o] = active ? (acc[o].x * acc[o].x + acc[o].y * acc[o].y) + (acc[o].z * acc[o].z + acc[o].w * acc[o].w) : 0.f;
  }
  dl_block_sum<NW>(q, sSq, wave, lane);
  if (!active) return;      // (after the last barrier)

  const dvis_f4 g = *(const dvis_f4 *)(gamma + c4), be = *(const dvis_f4 *)(beta + c4);
  float *ob = out + ((b * (size_t)h + (size_t)y) * (size_t)w + (size_t)x0) * (size_t)C + c4;
#pragma unroll
  for (int o = 0; o < DL_RUN; ++o) {
    if (x0 + o >= w) break;
    const float rstd = 1.f / sqrtf(q[o] * inv_c + eps);
    const dvis_f4 v = acc[o] * rstd * g + be;
    *(dvis_f4 *)(ob + (size_t)o * (size_t)C) = v;
  }
}

template <int NW>
int dl_launch(const float *x, float *out, int64_t batch_stride, int h, int w, int C, int xruns, unsigned units, const float *wt,
              const float *bias, const float *gamma, const float *beta, float eps, hipStream_t st) {
  hipLaunchKernelGGL(dwconv7x7_ln_tokens_kernel<NW>, dim3(units), dim3(NW * 64), 0, st, x, out, batch_stride, h, w, C, xruns, wt, bias,
                     gamma, beta, eps);
  return dvis_check_launch("dvis_dwconv7x7_ln_tokens");
}

}  // namespace

DVIS_EXPORT int dvis_dwconv7x7_ln_tokens_supported(int C) { return C % 4 == 0 && C >= 8 && C <= DL_MAX_C; }

DVIS_EXPORT int dvis_dwconv7x7_ln_tokens(const float *x, float *out, int64_t batch_stride, int B, int h, int w, int C, const float *weight,
                                         const float *bias, const float *gamma, const float *beta, float eps, void *stream) {
  DVIS_REQUIRE(dvis_dwconv7x7_ln_tokens_supported(C),
               "dvis_dwconv7x7_ln_tokens: C=%d channels are not served (served: C %% 4 == 0 with 8 <= C <= %d)", C, DL_MAX_C);
  DVIS_REQUIRE(B >= 0 && h > 0 && w > 0, "dvis_dwconv7x7_ln_tokens: bad sizes B=%d h=%d w=%d", B, h, w);
  DVIS_REQUIRE(x != nullptr && out != nullptr && weight != nullptr && gamma != nullptr && beta != nullptr,
               "dvis_dwconv7x7_ln_tokens: null x / out / weight / gamma / beta");
  DVIS_REQUIRE((((uintptr_t)x | (uintptr_t)out | (uintptr_t)weight | (uintptr_t)bias | (uintptr_t)gamma | (uintptr_t)beta) & 15) == 0,
               "dvis_dwconv7x7_ln_tokens: x=%p, out=%p, weight=%p, bias=%p, gamma=%p and beta=%p must be 16-byte aligned", (const void *)x,
               (const void *)out, (const void *)weight, (const void *)bias, (const void *)gamma, (const void *)beta);
  const int64_t frame = (int64_t)h * w * C;
  DVIS_REQUIRE(frame * 4 < ((int64_t)1 << 31),
               "dvis_dwconv7x7_ln_tokens: one frame is %lld bytes; offsets inside a frame are 32-bit (below 2^31 bytes)",
               (long long)(frame * 4));
  DVIS_REQUIRE(batch_stride % 4 == 0 && batch_stride >= frame,
               "dvis_dwconv7x7_ln_tokens: batch_stride=%lld must be a multiple of 4 floats and at least h w C = %lld",
               (long long)batch_stride, (long long)frame);
  if (B == 0) return DVIS_OK;
  const uintptr_t x_lo = (uintptr_t)x, x_hi = x_lo + (size_t)(((int64_t)(B - 1) * batch_stride + frame) * 4);
  const uintptr_t o_lo = (uintptr_t)out, o_hi = o_lo + (size_t)((int64_t)B * frame * 4);
  DVIS_REQUIRE(o_hi <= x_lo || x_hi <= o_lo,
               "dvis_dwconv7x7_ln_tokens: out=%p overlaps x=%p: in place is not possible (neighbouring tokens are read)", (const void *)out,
               (const void *)x);
  const int xruns = (w + DL_RUN - 1) / DL_RUN;
  const int64_t units = (int64_t)B * h * xruns;
  DVIS_REQUIRE(units <= INT_MAX, "dvis_dwconv7x7_ln_tokens: %lld (frame, row, run) units exceed the grid", (long long)units);
  hipStream_t st = (hipStream_t)stream;
  const unsigned u = (unsigned)units;
  switch ((C + 255) / 256) {
    case 1: return dl_launch<1>(x, out, batch_stride, h, w, C, xruns, u, weight, bias, gamma, beta, eps, st);
    case 2: return dl_launch<2>(x, out, batch_stride, h, w, C, xruns, u, weight, bias, gamma, beta, eps, st);
    case 3: return dl_launch<3>(x, out, batch_stride, h, w, C, xruns, u, weight, bias, gamma, beta, eps, st);
    case 4: return dl_launch<4>(x, out, batch_stride, h, w, C, xruns, u, weight, bias, gamma, beta, eps, st);
    case 5: return dl_launch<5>(x, out, batch_stride, h, w, C, xruns, u, weight, bias, gamma, beta, eps, st);
    default: return dl_launch<6>(x, out, batch_stride, h, w, C, xruns, u, weight, bias, gamma, beta, eps, st);
  }
}
