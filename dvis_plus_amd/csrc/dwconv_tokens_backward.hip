// Backward of the token-major depthwise 3 x 3 convolution (+ bias, + exact GELU) of the ViT-Adapter extractors' ConvFFN — gfx950.
//
// Forward (csrc/fused_elementwise.hip, dwconv3x3_tokens_kernel):  z = conv(x) + b,  out = gelu ? GELU(z) : z,  one level per launch.
// Only x is saved.  Three launches per level:
//   1. dwconv3x3_tokens_dz_kernel   the forward's register scheme (a lane holds 4 channels' 9 taps and walks 4 neighbouring tokens of a
//                                   row): recomputes z in the forward's tap order, forms dz = grad_out * gelu'(z) (erf form, as torch's
//                                   GeluBackward), writes dz to the workspace and — it holds the 3 x 6 window of x in registers —
//                                   accumulates its 36 + 4 partial sums of grad_weight / grad_bias.  The grid is BOUNDED (strips are
//                                   walked with a grid stride), a workgroup's four waves are added in wave order through LDS and one
//                                   partial row per workgroup goes to the workspace with 16-byte stores: no atomics.
//   2. dwconv3x3_tokens_dw_finalize_kernel   adds the workgroups' partials in a fixed order (16 slices in sequence, then the slices
//                                   in sequence) -> grad_weight (C, 9), grad_bias (C).  The same bits on every call.
//   3. dwconv3x3_tokens_dx_kernel   grad_x = the forward's convolution scheme on dz with the taps flipped, no bias, no GELU (a kernel of
//                                   its own because dz lies compact in the workspace while grad_x has the caller's batch stride).
// Exact fp32 throughout; int64 addressing.  Workspace: dz (B h w C floats) + partials (<= MAX_PARTS x 10 C): beyond dz it does not grow
// with the token count.
#include <math.h>

#include "dvis_common.h"

namespace {

constexpr int MAX_PARTS = 512;      // workgroups along x of the dz launch = partial rows (2 workgroups per CU are resident at 251 VGPRs)

__device__ __forceinline__ float gelu_grad(float z) {
  // torch's GeluBackward ("none"): cdf + z * pdf
  const float cdf = 0.5f * (1.f + erff(z * 0.70710678118654752440f));
  const float pdf = expf(-0.5f * z * z) * 0.39894228040143267794f;
  return cdf + z * pdf;
}

__global__ __launch_bounds__(256) void dwconv3x3_tokens_dz_kernel(const float *__restrict__ x, const float *__restrict__ go,
                                                                  float *__restrict__ dz, float *__restrict__ part, int64_t batch_stride,
                                                                  int B, int h, int w, int C, const float *__restrict__ wt,
                                                                  const float *__restrict__ bias, int gelu) {
  __shared__ float4 red[3 * 10 * 64];                   // waves 1..3: [wave - 1][sum][lane], 30 KB
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c4 = (blockIdx.y * 64 + lane) * 4;
  const bool live = c4 < C;                             // (no early return: every thread reaches the barrier)
  const int wq = (w + 3) / 4;
  const int64_t strips = (int64_t)B * h * wq, hwC = (int64_t)h * w * C;
  float4 gw[9], gb = float4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < 9; ++t) gw[t] = float4{0.f, 0.f, 0.f, 0.f};
  if (live) {
    float4 k[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) k[t] = float4{wt[(c4 + 0) * 9 + t], wt[(c4 + 1) * 9 + t], wt[(c4 + 2) * 9 + t], wt[(c4 + 3) * 9 + t]};
    const float4 bv = bias ? *reinterpret_cast<const float4 *>(bias + c4) : float4{0.f, 0.f, 0.f, 0.f};
    for (int64_t strip = (int64_t)blockIdx.x * 4 + wave; strip < strips; strip += (int64_t)gridDim.x * 4) {      // (b, y, x-quad)
      const int xq = (int)(strip % wq);
      const int64_t r = strip / wq;
      const int y = (int)(r % h);
      const int64_t b = r / h;
      const float *xb = x + b * batch_stride + c4;
      const int x0 = 4 * xq;
      float4 col[3][6];
#pragma unroll
      for (int dy = 0; dy < 3; ++dy) {
        const int yy = y + dy - 1;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
          const int xx = x0 + i - 1;
          col[dy][i] = yy >= 0 && yy < h && xx >= 0 && xx < w ? *reinterpret_cast<const float4 *>(xb + ((int64_t)yy * w + xx) * C)
                                                               : float4{0.f, 0.f, 0.f, 0.f};
        }
      }
      float4 g[4];
#pragma unroll
      for (int o = 0; o < 4; ++o)
        g[o] = x0 + o < w ? *reinterpret_cast<const float4 *>(go + b * batch_stride + c4 + ((int64_t)y * w + x0 + o) * C)
                          : float4{0.f, 0.f, 0.f, 0.f};
      if (gelu) {
        // z as the forward forms it: bias first, then the taps row by row, left to right (a row outside the map adds nothing)
        float4 acc[4] = {bv, bv, bv, bv};
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
          const int yy = y + dy - 1;
          if (yy < 0 || yy >= h) continue;
#pragma unroll
          for (int o = 0; o < 4; ++o)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
              const float4 kk = k[dy * 3 + dx], v = col[dy][o + dx];
              acc[o].x = __builtin_fmaf(kk.x, v.x, acc[o].x), acc[o].y = __builtin_fmaf(kk.y, v.y, acc[o].y);
              acc[o].z = __builtin_fmaf(kk.z, v.z, acc[o].z), acc[o].w = __builtin_fmaf(kk.w, v.w, acc[o].w);
            }
        }
#pragma unroll
        for (int o = 0; o < 4; ++o) {
          g[o].x *= gelu_grad(acc[o].x), g[o].y *= gelu_grad(acc[o].y);
          g[o].z *= gelu_grad(acc[o].z), g[o].w *= gelu_grad(acc[o].w);
        }
      }
      float *db = dz + b * hwC + c4;
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        if (x0 + o < w) *reinterpret_cast<float4 *>(db + ((int64_t)y * w + x0 + o) * C) = g[o];
        gb.x += g[o].x, gb.y += g[o].y, gb.z += g[o].z, gb.w += g[o].w;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
          for (int dx = 0; dx < 3; ++dx) {
            const float4 v = col[dy][o + dx];
            float4 &s = gw[dy * 3 + dx];
            s.x = __builtin_fmaf(g[o].x, v.x, s.x), s.y = __builtin_fmaf(g[o].y, v.y, s.y);
            s.z = __builtin_fmaf(g[o].z, v.z, s.z), s.w = __builtin_fmaf(g[o].w, v.w, s.w);
          }
      }
    }
  }
  // the workgroup's four waves in wave order, then one partial row: part[blockIdx.x][t][c], t = 0..8 the taps, 9 the bias
  if (wave > 0) {
    float4 *d = red + (wave - 1) * 10 * 64 + lane;
#pragma unroll
    for (int t = 0; t < 9; ++t) d[t * 64] = gw[t];
    d[9 * 64] = gb;
  }
  __syncthreads();
  if (wave == 0 && live) {
    for (int v = 0; v < 3; ++v) {
      const float4 *s = red + v * 10 * 64 + lane;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const float4 a = s[t * 64];
        gw[t].x += a.x, gw[t].y += a.y, gw[t].z += a.z, gw[t].w += a.w;
      }
      const float4 a = s[9 * 64];
      gb.x += a.x, gb.y += a.y, gb.z += a.z, gb.w += a.w;
    }
    float *p = part + (int64_t)blockIdx.x * 10 * C + c4;
#pragma unroll
    for (int t = 0; t < 9; ++t) *reinterpret_cast<float4 *>(p + (int64_t)t * C) = gw[t];
    *reinterpret_cast<float4 *>(p + (int64_t)9 * C) = gb;
  }
}

// part (nparts, 10, C) -> grad_weight (C, 9), grad_bias (C).  A thread adds one float4 column over one of 16 slices of the partial
// rows in sequence; the 16 slice sums are then added in sequence.  The order depends on nparts alone.
__global__ __launch_bounds__(256) void dwconv3x3_tokens_dw_finalize_kernel(const float *__restrict__ part, int nparts, int C,
                                                                           float *__restrict__ grad_weight,
                                                                           float *__restrict__ grad_bias) {
  __shared__ float4 sl[16 * 16];
  const int cl = threadIdx.x & 15, slice = threadIdx.x >> 4;
  const int64_t e = ((int64_t)blockIdx.x * 16 + cl) * 4;        // element of a (10, C) partial row
  const bool ok = e < (int64_t)10 * C;
  float4 s = float4{0.f, 0.f, 0.f, 0.f};
  if (ok) {
    const int per = (nparts + 15) / 16;
    const int p1 = min(nparts, (slice + 1) * per);
    for (int p = slice * per; p < p1; ++p) {
      const float4 a = *reinterpret_cast<const float4 *>(part + (int64_t)p * 10 * C + e);
      s.x += a.x, s.y += a.y, s.z += a.z, s.w += a.w;
    }
  }
  sl[slice * 16 + cl] = s;
  __syncthreads();
  if (slice == 0 && ok) {
    for (int v = 1; v < 16; ++v) {
      const float4 a = sl[v * 16 + cl];
      s.x += a.x, s.y += a.y, s.z += a.z, s.w += a.w;
    }
    const int t = (int)(e / C), c = (int)(e % C);
    const float r[4] = {s.x, s.y, s.z, s.w};
    if (t < 9) {
#pragma unroll
      for (int i = 0; i < 4; ++i) grad_weight[(int64_t)(c + i) * 9 + t] = r[i];
    } else if (grad_bias != nullptr) {
#pragma unroll
      for (int i = 0; i < 4; ++i) grad_bias[c + i] = r[i];
    }
  }
}

// grad_x = the convolution of dz with the taps flipped (k'[t] = k[8 - t]), no bias, no GELU: the forward kernel's scheme, reading dz
// with the workspace's compact batch stride and writing grad_x with the caller's.
__global__ __launch_bounds__(256) void dwconv3x3_tokens_dx_kernel(const float *__restrict__ dz, float *__restrict__ gx, int64_t dz_stride,
                                                                  int64_t batch_stride, int B, int h, int w, int C,
                                                                  const float *__restrict__ wt) {
  const int c4 = (blockIdx.y * 64 + (threadIdx.x & 63)) * 4;
  if (c4 >= C) return;
  const int wq = (w + 3) / 4;
  const int64_t strip = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);       // (b, y, x-quad)
  const int xq = (int)(strip % wq);
  const int64_t r = strip / wq;
  const int y = (int)(r % h);
  const int64_t b = r / h;
  if (b >= B) return;
  float4 k[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
    k[t] = float4{wt[(c4 + 0) * 9 + 8 - t], wt[(c4 + 1) * 9 + 8 - t], wt[(c4 + 2) * 9 + 8 - t], wt[(c4 + 3) * 9 + 8 - t]};
  const float *zb = dz + b * dz_stride + c4;
  float4 acc[4];
#pragma unroll
  for (int o = 0; o < 4; ++o) acc[o] = float4{0.f, 0.f, 0.f, 0.f};
  const int x0 = 4 * xq;
#pragma unroll
  for (int dy = 0; dy < 3; ++dy) {
    const int yy = y + dy - 1;
    if (yy < 0 || yy >= h) continue;
    float4 col[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const int xx = x0 + i - 1;
      col[i] = xx >= 0 && xx < w ? *reinterpret_cast<const float4 *>(zb + ((int64_t)yy * w + xx) * C) : float4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const float4 kk = k[dy * 3 + dx], v = col[o + dx];
        acc[o].x = __builtin_fmaf(kk.x, v.x, acc[o].x), acc[o].y = __builtin_fmaf(kk.y, v.y, acc[o].y);
        acc[o].z = __builtin_fmaf(kk.z, v.z, acc[o].z), acc[o].w = __builtin_fmaf(kk.w, v.w, acc[o].w);
      }
  }
  float *ob = gx + b * batch_stride + c4;
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    if (x0 + o >= w) break;
    *reinterpret_cast<float4 *>(ob + ((int64_t)y * w + x0 + o) * C) = acc[o];
  }
}

inline int dz_parts(int B, int h, int w) {
  const int64_t strips = (int64_t)B * h * ((w + 3) / 4);
  const int64_t blocks = (strips + 3) / 4;
  return (int)(blocks < MAX_PARTS ? blocks : MAX_PARTS);
}

}  // namespace

DVIS_EXPORT int64_t dvis_dwconv3x3_tokens_backward_ws_bytes(int B, int h, int w, int C) {
  if (B < 0 || h <= 0 || w <= 0 || C <= 0 || C % 4 != 0) return -1;
  return 4 * ((int64_t)B * h * w * C + (int64_t)dz_parts(B, h, w) * 10 * C);
}

DVIS_EXPORT int dvis_dwconv3x3_tokens_backward(const float *x, const float *grad_out, const float *weight, const float *bias, int gelu,
                                               int64_t batch_stride, int B, int h, int w, int C, float *grad_x, float *grad_weight,
                                               float *grad_bias, void *ws, void *stream) {
  DVIS_REQUIRE(x && grad_out && weight && grad_x && grad_weight && ws, "dwconv3x3_tokens_backward: null pointer");
  DVIS_REQUIRE(B >= 0 && h > 0 && w > 0 && C > 0 && C % 4 == 0 && batch_stride % 4 == 0 && batch_stride >= (int64_t)h * w * C,
               "dwconv3x3_tokens_backward: C %% 4 == 0 and a batch stride that is a multiple of 4 floats >= h * w * C are required");
  DVIS_REQUIRE(((uintptr_t)x | (uintptr_t)grad_out | (uintptr_t)grad_x | (uintptr_t)ws | (uintptr_t)(bias ? bias : weight)) % 16 == 0,
               "dwconv3x3_tokens_backward: 16-byte alignment");
  DVIS_REQUIRE(grad_x != grad_out && grad_x != x, "dwconv3x3_tokens_backward: grad_x must not alias grad_out or x");
  const hipStream_t st = (hipStream_t)stream;
  const int64_t strips = (int64_t)h * ((w + 3) / 4);
  DVIS_REQUIRE(strips * B < ((int64_t)1 << 32), "dwconv3x3_tokens_backward: too many tokens");
  const int nparts = dz_parts(B, h, w), cols = (C / 4 + 63) / 64;
  float *dz = (float *)ws;
  float *part = dz + (int64_t)B * h * w * C;
  if (nparts > 0) {
    hipLaunchKernelGGL(dwconv3x3_tokens_dz_kernel, dim3((unsigned)nparts, (unsigned)cols), dim3(256), 0, st, x, grad_out, dz, part,
                       batch_stride, B, h, w, C, weight, bias, gelu);
    const int rc = dvis_check_launch("dwconv3x3_tokens_dz_kernel");
    if (rc != DVIS_OK) return rc;
  }
  hipLaunchKernelGGL(dwconv3x3_tokens_dw_finalize_kernel, dim3((unsigned)((10 * C / 4 + 15) / 16)), dim3(256), 0, st, part, nparts, C,
                     grad_weight, grad_bias);
  int rc = dvis_check_launch("dwconv3x3_tokens_dw_finalize_kernel");
  if (rc != DVIS_OK || B == 0) return rc;
  hipLaunchKernelGGL(dwconv3x3_tokens_dx_kernel, dim3((unsigned)((strips * B + 3) / 4), (unsigned)cols), dim3(256), 0, st, dz, grad_x,
                     (int64_t)h * w * C, batch_stride, B, h, w, C, weight);
  return dvis_check_launch("dwconv3x3_tokens_dx_kernel");
}
