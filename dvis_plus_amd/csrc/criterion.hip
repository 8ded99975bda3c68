// Set-prediction supervision (matching cost + point-sampled mask losses) for gfx950, wave64.
//
//   dvis_match_cost        <- VideoHungarianMatcher.memory_efficient_forward up to C (mask2former_video/modeling/matcher.py:107-151)
//   dvis_point_sample_rows <- detectron2 point_sample on (R, 1, H, W) rows with per-row points (the oversampling pass of
//                             get_uncertain_point_coords_with_randomness, and the sampling primitive)
//   dvis_point_loss_fwd    <- point_sample x 2 + sigmoid_ce_loss + dice_loss (mask2former_video/modeling/criterion.py:21-67)
//   dvis_point_loss_bwd    <- their autograd, scattered through the four bilinear weights
//
// Sampling is F.grid_sample(x, 2 c - 1, bilinear, zeros, align_corners=False): pixel coordinate c * W - 0.5, a tap outside the
// map contributes zero.  All arithmetic fp32; targets fp32 or uint8 / bool (read as bytes, no float copy on the host).
// Layout: every map argument is CONTIGUOUS — the host front-ends (functions.py) make one .contiguous() copy of a strided view.
//
// Tiling of dvis_match_cost.  C[q][g] is four GEMM-shaped reductions over the N = T * K sample points with M = Q, N = G.  A
// workgroup (256 threads) owns one tile of 32 queries x 32 targets and a FIXED contiguous range of points; it walks the range
// in steps of 64 points: (1) every thread samples its share of the step's (32 + 32) x 64 values — one point per lane, the
// tap set-up shared by all rows — into LDS as x, sigmoid(x), softplus(x) and t; (2) thread (q, g mod 8) owns 4 outputs and
// accumulates  softplus(x) - t x  (= softplus(-x) t + softplus(x) (1 - t), without the cancelling sums) and  sigmoid(x) t  over
// the 64 points from LDS.  Partials per (split, q, g) go to a workspace and a finishing launch adds the splits in index order
// (in double), forms the three terms, the class term -softmax(logits)[q, ids[g]] and C.  The split of the point range depends on
// the shapes alone and every sum has one fixed order: no floating-point atomics, two runs give the same bits.
// Bound: the gathers (4 taps x (Q + G q-tiles) x N dwords, one 32-byte sector each in the worst case) — the arithmetic is
// 3 FLOP per (q, g, point), far below the vector rate; the kernel is latency / L2-gather bound, not HBM or VALU bound.
//
// dvis_point_loss_fwd: grid (splits, R), fixed split of a row's P points, wave shuffle tree + LDS in a fixed order, finishing
// launch over the splits: deterministic.  dvis_point_loss_bwd: one thread per (row, point), 4 fp32 vector atomics into grad_src
// (zeroed by dvis_zero_words); the reproducible form adds round(v * 2^k) into 64-bit integer cells instead (integer addition is
// associative) and a finishing launch scales back.  No scalar-memory writes anywhere: plain C++ and vector atomics only.
#include <algorithm>
#include <cmath>

#include "dvis_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kQT = 32;        // queries per workgroup tile
constexpr int kGT = 32;        // targets per workgroup tile
constexpr int kPS = 64;        // points per step
constexpr int kLd = kPS + 4;   // LDS row stride in floats (16-byte aligned rows, rows 4 banks apart)
constexpr int kMaxSplits = 128;
constexpr int kLossSplits = 16;

struct Taps {
  int o[4];      // element offsets inside one H x W map, -1 = outside
  float w[4];
};

__device__ __forceinline__ Taps make_taps(float cx, float cy, int H, int W) {
  Taps t;
  const float x = cx * (float)W - 0.5f, y = cy * (float)H - 0.5f;
  const float xf = floorf(x), yf = floorf(y);
  const float lx = x - xf, ly = y - yf;
  // out-of-range / non-finite coordinates: every tap outside
  const bool fin = (x > -2.f) && (y > -2.f) && (x < (float)W + 1.f) && (y < (float)H + 1.f);
  const int x0 = fin ? (int)xf : -2, y0 = fin ? (int)yf : -2;
  const bool xa = x0 >= 0 && x0 < W, xb = x0 + 1 >= 0 && x0 + 1 < W;
  const bool ya = y0 >= 0 && y0 < H, yb = y0 + 1 >= 0 && y0 + 1 < H;
  const int o = y0 * W + x0;
  t.o[0] = (xa && ya) ? o : -1;
  t.o[1] = (xb && ya) ? o + 1 : -1;
  t.o[2] = (xa && yb) ? o + W : -1;
  t.o[3] = (xb && yb) ? o + W + 1 : -1;
  t.w[0] = (1.f - lx) * (1.f - ly);
  t.w[1] = lx * (1.f - ly);
  t.w[2] = (1.f - lx) * ly;
  t.w[3] = lx * ly;
  return t;
}

template <typename T> __device__ __forceinline__ float ldf(const T *p) { return (float)*p; }

template <typename T> __device__ __forceinline__ float sample(const T *__restrict__ map, const Taps &t) {
  const float v0 = t.o[0] >= 0 ? ldf(map + t.o[0]) : 0.f;
  const float v1 = t.o[1] >= 0 ? ldf(map + t.o[1]) : 0.f;
  const float v2 = t.o[2] >= 0 ? ldf(map + t.o[2]) : 0.f;
  const float v3 = t.o[3] >= 0 ? ldf(map + t.o[3]) : 0.f;
  float r = t.w[0] * v0;
  r = __builtin_fmaf(t.w[1], v1, r);
  r = __builtin_fmaf(t.w[2], v2, r);
  r = __builtin_fmaf(t.w[3], v3, r);
  return r;
}

// torch's forms: softplus(x) = max(x, 0) + log1p(exp(-|x|)), sigmoid(x) = 1 / (1 + exp(-x))
__device__ __forceinline__ float softplus_f(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }

// ---- matching cost ---------------------------------------------------------------------------------------------------------
// grid (splits, q tiles, g tiles).  ws layout (floats): ce[S][Q][G] | dice[S][Q][G] | sig[S][Q] | tsum[S][G]
template <typename TT>
__global__ __launch_bounds__(kThreads) void match_cost_kernel(const float *__restrict__ pred, const TT *__restrict__ tgt,
                                                              const float *__restrict__ coords, int Q, int G, int T, int H, int W,
                                                              int Ht, int Wt, int K, int steps_per_split,
                                                              float *__restrict__ ws) {
  __shared__ __attribute__((aligned(16))) float sx[kQT * kLd], ss[kQT * kLd], sn[kQT * kLd], st[kGT * kLd];
  const int tid = threadIdx.x;
  const int S = gridDim.x, split = blockIdx.x;
  const int q0 = blockIdx.y * kQT, g0 = blockIdx.z * kGT;
  const int nq = min(kQT, Q - q0), ng = min(kGT, G - g0);
  const long long N = (long long)T * K;
  const long long HW = (long long)H * W, HWt = (long long)Ht * Wt;
  const int ql = tid >> 3, gs = tid & 7;      // this thread's outputs: (q0 + ql, g0 + gs + 8 j), j = 0..3
  float ce[4] = {0.f, 0.f, 0.f, 0.f}, di[4] = {0.f, 0.f, 0.f, 0.f}, sg = 0.f, ts[4] = {0.f, 0.f, 0.f, 0.f};
  const int pl = tid & (kPS - 1), rw = tid >> 6;     // sampling: point pl of the step (one per lane), rows rw, rw + 4, ...

  for (int step = 0; step < steps_per_split; ++step) {
    const long long n = ((long long)split * steps_per_split + step) * kPS + pl;
    const bool live = n < N;
    int t = 0;
    Taps tp, tq;      // prediction / target taps: the two may differ in size (the targets are at the padded image's)
    if (live) {
      t = (int)(n / K);
      const int k = (int)(n - (long long)t * K);
      tp = make_taps(coords[2 * k], coords[2 * k + 1], H, W);
      tq = make_taps(coords[2 * k], coords[2 * k + 1], Ht, Wt);
    }
    __syncthreads();      // the previous step's readers are done
    for (int r = rw; r < kQT; r += 4) {
      float x = 0.f, s = 0.f, sp = 0.f;
      if (live && r < nq) {
        x = sample(pred + ((long long)(q0 + r) * T + t) * HW, tp);
        s = sigmoid_f(x);
        sp = softplus_f(x);
      }
      sx[r * kLd + pl] = x;
      ss[r * kLd + pl] = s;
      sn[r * kLd + pl] = sp;
    }
    for (int r = rw; r < kGT; r += 4) {
      float v = 0.f;
      if (live && r < ng) v = sample(tgt + ((long long)(g0 + r) * T + t) * HWt, tq);
      st[r * kLd + pl] = v;
    }
    __syncthreads();
    float ce1[4] = {0.f, 0.f, 0.f, 0.f}, di1[4] = {0.f, 0.f, 0.f, 0.f}, sg1 = 0.f, ts1[4] = {0.f, 0.f, 0.f, 0.f};
    const dvis_f4 *px = (const dvis_f4 *)(sx + ql * kLd), *ps = (const dvis_f4 *)(ss + ql * kLd),
                  *pn = (const dvis_f4 *)(sn + ql * kLd);
#pragma unroll 2
    for (int p4 = 0; p4 < kPS / 4; ++p4) {
      const dvis_f4 x = px[p4], s = ps[p4], sp = pn[p4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const dvis_f4 tv = ((const dvis_f4 *)(st + (gs + 8 * j) * kLd))[p4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          ce1[j] += __builtin_fmaf(-tv[e], x[e], sp[e]);
          di1[j] = __builtin_fmaf(s[e], tv[e], di1[j]);
          ts1[j] += tv[e];
        }
      }
      sg1 += (s[0] + s[1]) + (s[2] + s[3]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      ce[j] += ce1[j];
      di[j] += di1[j];
      ts[j] += ts1[j];
    }
    sg += sg1;
  }
  // dead points were staged as x = s = sp = t = 0: softplus - t x = 0 and every other product is 0, so they add nothing
  const size_t SQG = (size_t)S * Q * G;
  float *wce = ws, *wdi = ws + SQG, *wsg = ws + 2 * SQG, *wts = wsg + (size_t)S * Q;
  if (ql < nq) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int g = gs + 8 * j;
      if (g < ng) {
        const size_t o = ((size_t)split * Q + q0 + ql) * G + g0 + g;
        wce[o] = ce[j];
        wdi[o] = di[j];
      }
    }
    if (gs == 0 && blockIdx.z == 0) wsg[(size_t)split * Q + q0 + ql] = sg;
  }
  if (ql == 0 && blockIdx.y == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int g = gs + 8 * j;
      if (g < ng) wts[(size_t)split * G + g0 + g] = ts[j];
    }
  }
}

// one thread per (q, g): adds the splits in index order, forms the terms and C
__global__ __launch_bounds__(kThreads) void match_cost_finish_kernel(const float *__restrict__ ws, const float *__restrict__ logits,
                                                                     const int64_t *__restrict__ ids, int Q, int G, int NC, int S,
                                                                     long long N, float w_class, float w_mask, float w_dice,
                                                                     float *__restrict__ C, float *__restrict__ terms) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= Q * G) return;
  const int q = i / G, g = i - q * G;
  const size_t SQG = (size_t)S * Q * G;
  const float *wce = ws, *wdi = ws + SQG, *wsg = ws + 2 * SQG, *wts = wsg + (size_t)S * Q;
  double ce = 0., di = 0., sg = 0., ts = 0.;
  for (int s = 0; s < S; ++s) {
    ce += (double)wce[((size_t)s * Q + q) * G + g];
    di += (double)wdi[((size_t)s * Q + q) * G + g];
    sg += (double)wsg[(size_t)s * Q + q];
    ts += (double)wts[(size_t)s * G + g];
  }
  const float cost_mask = (float)(ce / (double)N);
  const float cost_dice = (float)(1. - (2. * di + 1.) / (sg + ts + 1.));
  // -softmax(logits[q])[ids[g]]
  const float *lq = logits + (size_t)q * NC;
  float mx = lq[0];
  for (int c = 1; c < NC; ++c) mx = fmaxf(mx, lq[c]);
  float den = 0.f;
  for (int c = 0; c < NC; ++c) den += expf(lq[c] - mx);
  const int64_t id = ids[g];
  const float cost_class = (id >= 0 && id < NC) ? -(expf(lq[id] - mx) / den) : __builtin_nanf("");
  // the reference's order: cost_mask * m + cost_class * c + cost_dice * d
  C[i] = (w_mask * cost_mask + w_class * cost_class) + w_dice * cost_dice;
  if (terms) {
    const size_t QG = (size_t)Q * G;
    terms[i] = cost_class;
    terms[QG + i] = cost_mask;
    terms[2 * QG + i] = cost_dice;
  }
}

// ---- rows sampling ---------------------------------------------------------------------------------------------------------
template <typename TT>
__global__ __launch_bounds__(kThreads) void point_sample_rows_kernel(const TT *__restrict__ rows, const float *__restrict__ coords,
                                                                     long long R, int P, int H, int W, float *__restrict__ out) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= R * P) return;
  const long long r = i / P;
  const Taps tp = make_taps(coords[2 * i], coords[2 * i + 1], H, W);
  out[i] = sample(rows + r * (long long)H * W, tp);
}

// ---- point losses ----------------------------------------------------------------------------------------------------------
// fixed-order block sum of three values: shuffle tree inside a wave, then wave 0 adds the 4 wave results in order
__device__ __forceinline__ void block_sum3(float &a, float &b, float &c, float *red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_down(a, o, 64);
    b += __shfl_down(b, o, 64);
    c += __shfl_down(c, o, 64);
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) {
    red[wave * 3] = a;
    red[wave * 3 + 1] = b;
    red[wave * 3 + 2] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = ((red[0] + red[3]) + red[6]) + red[9];
    b = ((red[1] + red[4]) + red[7]) + red[10];
    c = ((red[2] + red[5]) + red[8]) + red[11];
  }
}

// grid (kLossSplits, R): partial[r][split][3] = sum bce, sum sigmoid t, sum sigmoid + sum t over the split's points
template <typename TT>
__global__ __launch_bounds__(kThreads) void point_loss_fwd_kernel(const float *__restrict__ src, const TT *__restrict__ tgt,
                                                                  const float *__restrict__ coords, int P, int H, int W, int Ht,
                                                                  int Wt, float *__restrict__ partial) {
  __shared__ float red[12];
  const int r = blockIdx.y, split = blockIdx.x;
  const int per = (P + kLossSplits - 1) / kLossSplits;
  const int p0 = split * per, p1 = min(P, p0 + per);
  const long long HW = (long long)H * W, HWt = (long long)Ht * Wt;
  const float *cr = coords + (size_t)r * P * 2;
  float bce = 0.f, a = 0.f, b = 0.f;
  for (int p = p0 + threadIdx.x; p < p1; p += kThreads) {
    const Taps tp = make_taps(cr[2 * p], cr[2 * p + 1], H, W), tq = make_taps(cr[2 * p], cr[2 * p + 1], Ht, Wt);
    const float x = sample(src + r * HW, tp), t = sample(tgt + r * HWt, tq);
    const float s = sigmoid_f(x);
    bce += __builtin_fmaf(-t, x, softplus_f(x));      // max(x, 0) - x t + log1p(exp(-|x|))
    a = __builtin_fmaf(s, t, a);
    b += s + t;
  }
  block_sum3(bce, a, b, red);
  if (threadIdx.x == 0) {
    float *o = partial + ((size_t)r * kLossSplits + split) * 3;
    o[0] = bce;
    o[1] = a;
    o[2] = b;
  }
}

__global__ __launch_bounds__(kThreads) void point_loss_finish_kernel(const float *__restrict__ partial, int R, float *__restrict__ out) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= R * 3) return;
  const int r = i / 3, c = i - 3 * r;
  double v = 0.;
  for (int s = 0; s < kLossSplits; ++s) v += (double)partial[((size_t)r * kLossSplits + s) * 3 + c];
  out[i] = (float)v;
}

// 2^k with |any pixel's sum| * 2^k < 2^62: a contribution is at most bound = |g_mask| / (P nm) + |g_dice| / (2 nm) for targets in
// [0, 1] (|2 t (b + 1) - (2 a + 1)| <= 2 (b + 1), b + 1 >= 1, sigmoid' <= 1 / 4), and at most 4 P of them meet in one pixel
__device__ __forceinline__ float fixed_scale(float g_mask, float g_dice, int P, float inv_nm) {
  const float bound = (fabsf(g_mask) / (float)P + 0.5f * fabsf(g_dice)) * inv_nm * 4.f * (float)P;
  if (!(bound > 0.f) || !(bound < 3.0e38f)) return 1.f;
  int e;
  frexpf(bound, &e);                       // bound < 2^e
  return ldexpf(1.f, min(max(61 - e, -120), 120));
}

template <typename TT, bool DET>
__global__ __launch_bounds__(kThreads) void point_loss_bwd_kernel(const float *__restrict__ src, const TT *__restrict__ tgt,
                                                                  const float *__restrict__ coords, const float *__restrict__ ab,
                                                                  const float *__restrict__ g_mask, const float *__restrict__ g_dice,
                                                                  long long R, int P, int H, int W, int Ht, int Wt, float inv_nm,
                                                                  float *__restrict__ grad, unsigned long long *__restrict__ acc) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= R * P) return;
  const long long r = i / P;
  const long long HW = (long long)H * W;
  const Taps tp = make_taps(coords[2 * i], coords[2 * i + 1], H, W);
  const float x = sample(src + r * HW, tp);
  const float t = sample(tgt + r * (long long)Ht * Wt, make_taps(coords[2 * i], coords[2 * i + 1], Ht, Wt));
  const float s = sigmoid_f(x);
  const float a = ab[3 * r + 1], b1 = ab[3 * r + 2] + 1.f;
  const float gm = *g_mask, gd = *g_dice;
  const float d_dice = -(2.f * t * b1 - (2.f * a + 1.f)) / (b1 * b1) * (s * (1.f - s));
  const float g = gm * (s - t) * (inv_nm / (float)P) + gd * d_dice * inv_nm;
  float scale = 1.f;
  if constexpr (DET) scale = fixed_scale(gm, gd, P, inv_nm);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (tp.o[k] < 0) continue;
    const float v = g * tp.w[k];
    if constexpr (DET)
      atomicAdd(acc + r * HW + tp.o[k], (unsigned long long)__float2ll_rn(v * scale));   // two's complement: signed sums wrap correctly
    else
      atomicAdd(grad + r * HW + tp.o[k], v);
  }
}

__global__ __launch_bounds__(kThreads) void point_loss_bwd_finish_kernel(const unsigned long long *__restrict__ acc,
                                                                         const float *__restrict__ g_mask,
                                                                         const float *__restrict__ g_dice, int P, float inv_nm,
                                                                         size_t n, float *__restrict__ grad) {
  const float gm = *g_mask, gd = *g_dice;
  const bool finite = fabsf(gm) < 3.0e38f && fabsf(gd) < 3.0e38f;      // NaN / Inf upstream has no fixed-point image: hand it back
  const double inv = 1. / (double)fixed_scale(gm, gd, P, inv_nm);
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads)
    grad[i] = finite ? (float)((double)(long long)acc[i] * inv) : __builtin_nanf("");
}

int match_splits(long long N, int *steps_per_split) {
  const long long steps = (N + kPS - 1) / kPS;
  const int S = (int)std::min<long long>(steps, kMaxSplits);
  *steps_per_split = (int)((steps + S - 1) / S);
  return (int)((steps + *steps_per_split - 1) / *steps_per_split);
}

bool map_sizes_ok(long long rows, int H, int W) {
  return H > 0 && W > 0 && (long long)H * W < (1ll << 30) && rows >= 0 && rows < (1ll << 31);
}

}  // namespace

DVIS_EXPORT int64_t dvis_match_cost_ws_bytes(int Q, int G, int T, int K) {
  if (Q <= 0 || G <= 0 || T <= 0 || K <= 0) return 0;
  int sps;
  const int S = match_splits((long long)T * K, &sps);
  return (int64_t)S * ((int64_t)2 * Q * G + Q + G) * 4;
}

DVIS_EXPORT int dvis_match_cost(const float *pred, const void *tgt, int tgt_u8, const float *coords, const float *logits,
                                const int64_t *tgt_ids, int Q, int G, int T, int H, int W, int Ht, int Wt, int K, int NC,
                                float w_class, float w_mask, float w_dice, float *C, float *terms, void *ws, void *stream) {
  DVIS_REQUIRE(Q > 0 && G > 0 && T > 0 && K > 0 && NC > 0, "match_cost: bad sizes Q %d G %d T %d K %d classes %d", Q, G, T, K, NC);
  DVIS_REQUIRE(map_sizes_ok((long long)Q * T, H, W) && map_sizes_ok((long long)G * T, Ht, Wt) && (long long)Q * G < (1ll << 30),
               "match_cost: maps too large");
  DVIS_REQUIRE(pred && tgt && coords && logits && tgt_ids && C && ws, "match_cost: null pointer");
  DVIS_REQUIRE((uintptr_t)ws % 4 == 0, "match_cost: misaligned workspace");
  hipStream_t st = (hipStream_t)stream;
  int sps;
  const int S = match_splits((long long)T * K, &sps);
  const dim3 grid(S, (Q + kQT - 1) / kQT, (G + kGT - 1) / kGT);
  if (tgt_u8)
    hipLaunchKernelGGL(match_cost_kernel<uint8_t>, grid, dim3(kThreads), 0, st, pred, (const uint8_t *)tgt, coords, Q, G, T, H, W, Ht,
                       Wt, K, sps, (float *)ws);
  else
    hipLaunchKernelGGL(match_cost_kernel<float>, grid, dim3(kThreads), 0, st, pred, (const float *)tgt, coords, Q, G, T, H, W, Ht, Wt, K,
                       sps, (float *)ws);
  if (const int rc = dvis_check_launch("match_cost_kernel")) return rc;
  hipLaunchKernelGGL(match_cost_finish_kernel, dim3((Q * G + kThreads - 1) / kThreads), dim3(kThreads), 0, st, (const float *)ws,
                     logits, tgt_ids, Q, G, NC, S, (long long)T * K, w_class, w_mask, w_dice, C, terms);
  return dvis_check_launch("match_cost_finish_kernel");
}

DVIS_EXPORT int dvis_point_sample_rows(const void *rows, int rows_u8, const float *coords, int64_t R, int P, int H, int W,
                                       float *out, void *stream) {
  DVIS_REQUIRE(R >= 0 && P >= 0 && map_sizes_ok(R, H, W) && R * (int64_t)P < (1ll << 40), "point_sample_rows: bad sizes");
  if (R == 0 || P == 0) return DVIS_OK;
  DVIS_REQUIRE(rows && coords && out, "point_sample_rows: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((R * P + kThreads - 1) / kThreads));
  DVIS_REQUIRE((R * P + kThreads - 1) / kThreads < (1ll << 31), "point_sample_rows: too many points");
  if (rows_u8)
    hipLaunchKernelGGL(point_sample_rows_kernel<uint8_t>, grid, dim3(kThreads), 0, st, (const uint8_t *)rows, coords, (long long)R, P,
                       H, W, out);
  else
    hipLaunchKernelGGL(point_sample_rows_kernel<float>, grid, dim3(kThreads), 0, st, (const float *)rows, coords, (long long)R, P, H,
                       W, out);
  return dvis_check_launch("point_sample_rows_kernel");
}

DVIS_EXPORT int64_t dvis_point_loss_ws_bytes(int64_t R) { return R > 0 ? R * kLossSplits * 3 * 4 : 0; }

DVIS_EXPORT int dvis_point_loss_fwd(const float *src, const void *tgt, int tgt_u8, const float *coords, int R, int P, int H, int W,
                                    int Ht, int Wt, float *out, void *ws, void *stream) {
  DVIS_REQUIRE(R >= 0 && R < 65536 && P > 0 && map_sizes_ok(R, H, W) && map_sizes_ok(R, Ht, Wt), "point_loss_fwd: bad sizes R %d P %d (R < 65536)", R, P);
  if (R == 0) return DVIS_OK;
  DVIS_REQUIRE(src && tgt && coords && out && ws, "point_loss_fwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(kLossSplits, R);
  if (tgt_u8)
    hipLaunchKernelGGL(point_loss_fwd_kernel<uint8_t>, grid, dim3(kThreads), 0, st, src, (const uint8_t *)tgt, coords, P, H, W,
                       Ht, Wt, (float *)ws);
  else
    hipLaunchKernelGGL(point_loss_fwd_kernel<float>, grid, dim3(kThreads), 0, st, src, (const float *)tgt, coords, P, H, W, Ht,
                       Wt, (float *)ws);
  if (const int rc = dvis_check_launch("point_loss_fwd_kernel")) return rc;
  hipLaunchKernelGGL(point_loss_finish_kernel, dim3((R * 3 + kThreads - 1) / kThreads), dim3(kThreads), 0, st, (const float *)ws, R,
                     out);
  return dvis_check_launch("point_loss_finish_kernel");
}

DVIS_EXPORT int dvis_point_loss_bwd(const float *src, const void *tgt, int tgt_u8, const float *coords, const float *sums,
                                    const float *g_mask, const float *g_dice, int R, int P, int H, int W, int Ht, int Wt,
                                    float num_masks, float *grad_src, void *det_ws, void *stream) {
  DVIS_REQUIRE(R >= 0 && R < 65536 && P > 0 && map_sizes_ok(R, H, W) && map_sizes_ok(R, Ht, Wt) && num_masks > 0.f, "point_loss_bwd: bad sizes / num_masks");
  if (R == 0) return DVIS_OK;
  DVIS_REQUIRE(src && tgt && coords && sums && g_mask && g_dice && grad_src, "point_loss_bwd: null pointer");
  DVIS_REQUIRE((uintptr_t)det_ws % 8 == 0, "point_loss_bwd: misaligned workspace");
  hipStream_t st = (hipStream_t)stream;
  const size_t n = (size_t)R * H * W;
  const float inv_nm = 1.f / num_masks;
  const dim3 grid((unsigned)(((long long)R * P + kThreads - 1) / kThreads));
  unsigned long long *acc = (unsigned long long *)det_ws;
  if (const int rc = acc ? dvis_zero_words(acc, n * 2, st, "point_loss_bwd: zero workspace")
                         : dvis_zero_words(grad_src, n, st, "point_loss_bwd: zero grad_src"))
    return rc;
#define DVIS_BWD(TT, DET)                                                                                                          \
  hipLaunchKernelGGL((point_loss_bwd_kernel<TT, DET>), grid, dim3(kThreads), 0, st, src, (const TT *)tgt, coords, sums, g_mask, \
                     g_dice, (long long)R, P, H, W, Ht, Wt, inv_nm, grad_src, acc)
  if (acc) {
    if (tgt_u8) DVIS_BWD(uint8_t, true); else DVIS_BWD(float, true);
  } else {
    if (tgt_u8) DVIS_BWD(uint8_t, false); else DVIS_BWD(float, false);
  }
#undef DVIS_BWD
  if (const int rc = dvis_check_launch("point_loss_bwd_kernel")) return rc;
  if (!acc) return DVIS_OK;
  hipLaunchKernelGGL(point_loss_bwd_finish_kernel, dim3((unsigned)std::min<size_t>((n + kThreads - 1) / kThreads, 65536)),
                     dim3(kThreads), 0, st, acc, g_mask, g_dice, P, inv_nm, n, grad_src);
  return dvis_check_launch("point_loss_bwd_finish_kernel");
}
