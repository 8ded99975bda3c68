// Prediction files of VIPSeg / VSPW from (T, H, W) id maps on the device — gfx950.
//
// Replaces the per-segment host passes of the reference's writers (dvis_Plus/data_video/):
//   vps_eval.py:112-143   per segment: `pan_seg_result == id` over the clip, `pan_format[mask] = color`, then per frame
//                         mask.sum() and np.where for the bbox
//   vss_eval.py:93-100    astype(np.uint8), np.unique, one `sem_seg_result_[sem_seg_result == cls] = cls_` per class
// Three kernels: the per-(frame, segment) area and bounds in one pass over the map, the RGB-encoded panoptic PNG pixels through a
// colour table, and the VSPW class map through a 256-entry id table.  The host (pred_writers.py) copies only their uint8 maps and
// the small stats table.  Integer only (LDS u32, global u64 atomics): results do not depend on the order the atomics land in.
//
// Stats: one thread owns 8 contiguous pixels per step of a grid-stride loop and keeps a running (id, count, bounds): an id change
// flushes the run with one atomic per field, and the run carries over from one step to the next.  A thread's pixels only move
// forward in the frame, so the run's first / last row are its ymin / ymax; x bounds are a running min / max.  The maps are blocky
// (segments are regions), so a run covers many pixels.  The (area, xmin, ymin, xmax, ymax) table lives in LDS while it fits in
// 64 KB (two workgroups per CU), then one u64 global atomic per field of every non-empty entry and workgroup; larger tables take
// the same loop with the run flushed straight into global memory.  Global minima are kept as kCoord - v under atomicMax, so a
// zeroed table is the empty one; a last pass turns them back and leaves empty entries all zero.
//
// Paint: 16 pixels per thread and step = four 16-byte loads of ids and 48 bytes of RGB = three 16-byte stores (one 16-byte store
// of class bytes for VSPW).  The output is the contiguous (T, H, W, 3) / (T, H, W) array, so the clip is one flat run of pixels
// whatever the width: only the last T * H * W mod 16 pixels take the byte-wise tail.
#include "dvis_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPix = 8;                      // stats: contiguous pixels per thread and step
constexpr int kStep = kThreads * kPix;       // stats: pixels per workgroup and step
constexpr size_t kLdsBytes = 64 * 1024;      // stats table per workgroup on the LDS path
constexpr int kFields = 5;                   // area, xmin, ymin, xmax, ymax
constexpr int kMaxLdsIds = (int)(kLdsBytes / (kFields * 4));
constexpr unsigned long long kCoord = 0x7fffffffull;   // global minima are stored as kCoord - v
constexpr int kRunNone = -1;
constexpr int kRunBad = -2;                  // id outside 0..n: counted in `bad`
constexpr int kPaintPix = 16;                // paint: pixels per thread and step
constexpr int kMaxLdsLut = 4096;             // colour entries held in LDS (16 KB; every workgroup loads its copy)
constexpr int kPaintBlocks = 1024;

template <bool kLds>
__device__ __forceinline__ void flush_run(int id, unsigned cnt, unsigned x0, unsigned y0, unsigned x1, unsigned y1,
                                          unsigned *s_tab, unsigned long long *g_tab, unsigned long long &bad) {
  if (id == kRunBad) {
    bad += cnt;
  } else if (kLds) {
    unsigned *e = s_tab + id * kFields;
    atomicAdd(&e[0], cnt);
    atomicMin(&e[1], x0);
    atomicMin(&e[2], y0);
    atomicMax(&e[3], x1);
    atomicMax(&e[4], y1);
  } else {
    unsigned long long *e = g_tab + (int64_t)id * kFields;
    atomicAdd(&e[0], (unsigned long long)cnt);
    atomicMax(&e[1], kCoord - x0);
    atomicMax(&e[2], kCoord - y0);
    atomicMax(&e[3], (unsigned long long)x1);
    atomicMax(&e[4], (unsigned long long)y1);
  }
}

// grid (gx, frames); workgroup (x, f) covers frame f's pixels x * kStep + i * gx * kStep .. into frame f's (n + 1) entries.
template <bool kLds>
__global__ __launch_bounds__(kThreads) void stats_kernel(const int *__restrict__ map, int W, int64_t hw, int n,
                                                         unsigned long long *__restrict__ out,
                                                         unsigned long long *__restrict__ bad_out) {
  extern __shared__ unsigned s_tab[];
  const int nent = n + 1;
  if (kLds) {
    for (int i = threadIdx.x; i < nent * kFields; i += kThreads) {
      const int fld = i % kFields;
      s_tab[i] = (fld == 1 || fld == 2) ? 0xffffffffu : 0u;
    }
    __syncthreads();
  }
  const int64_t f = blockIdx.y;
  const int *__restrict__ mf = map + f * hw;
  unsigned long long *g_tab = out + f * (int64_t)nent * kFields;
  int run_id = kRunNone;
  unsigned run = 0u, rx0 = 0u, ry0 = 0u, rx1 = 0u, ry1 = 0u;
  unsigned long long bad = 0ull;
  for (int64_t base = (int64_t)blockIdx.x * kStep + threadIdx.x * kPix; base < hw; base += (int64_t)gridDim.x * kStep) {
    const int cnt = (int)(hw - base < kPix ? hw - base : kPix);
    int v[kPix];
#pragma unroll
    for (int j = 0; j < kPix; ++j) v[j] = j < cnt ? mf[base + j] : 0;
    unsigned y = (unsigned)(base / W);
    unsigned x = (unsigned)(base - (int64_t)y * W);
#pragma unroll
    for (int j = 0; j < kPix; ++j) {
      if (j >= cnt) break;
      const int id = (unsigned)v[j] <= (unsigned)n ? v[j] : kRunBad;
      if (id == run_id) {
        ++run;
        rx0 = x < rx0 ? x : rx0;
        rx1 = x > rx1 ? x : rx1;
        ry1 = y;
      } else {
        if (run) flush_run<kLds>(run_id, run, rx0, ry0, rx1, ry1, s_tab, g_tab, bad);
        run_id = id;
        run = 1u;
        rx0 = rx1 = x;
        ry0 = ry1 = y;
      }
      if (++x == (unsigned)W) {
        x = 0u;
        ++y;
      }
    }
  }
  if (run) flush_run<kLds>(run_id, run, rx0, ry0, rx1, ry1, s_tab, g_tab, bad);
  if (bad) atomicAdd(bad_out, bad);
  if (kLds) {
    __syncthreads();
    for (int i = threadIdx.x; i < nent; i += kThreads) {
      const unsigned *e = s_tab + i * kFields;
      if (!e[0]) continue;
      unsigned long long *g = g_tab + (int64_t)i * kFields;
      atomicAdd(&g[0], (unsigned long long)e[0]);
      atomicMax(&g[1], kCoord - e[1]);
      atomicMax(&g[2], kCoord - e[2]);
      atomicMax(&g[3], (unsigned long long)e[3]);
      atomicMax(&g[4], (unsigned long long)e[4]);
    }
  }
}

// Stored minima back to coordinates; entries with no pixel become all zero.
__global__ __launch_bounds__(kThreads) void stats_finish_kernel(unsigned long long *__restrict__ out, int64_t nent) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= nent) return;
  unsigned long long *e = out + i * kFields;
  if (e[0]) {
    e[1] = kCoord - e[1];
    e[2] = kCoord - e[2];
  } else {
    e[1] = e[2] = e[3] = e[4] = 0ull;
  }
}

// Three dwords of packed RGB for four colours (0x00BBGGRR each): bytes r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3.
__device__ __forceinline__ void pack_rgb4(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned *w) {
  w[0] = c0 | (c1 << 24);
  w[1] = (c1 >> 8) | (c2 << 16);
  w[2] = (c2 >> 16) | (c3 << 8);
}

template <bool kLds>
__global__ __launch_bounds__(kThreads) void paint_rgb_kernel(const int *__restrict__ ids, int64_t npx,
                                                             const unsigned *__restrict__ lut, int nlut,
                                                             uint8_t *__restrict__ out) {
  extern __shared__ unsigned s_lut[];
  const unsigned *L = lut;
  if (kLds) {
    for (int i = threadIdx.x; i < nlut; i += kThreads) s_lut[i] = lut[i];
    __syncthreads();
    L = s_lut;
  }
  const int64_t ngroups = npx / kPaintPix;
  for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; g < ngroups; g += (int64_t)gridDim.x * kThreads) {
    const int4 *src = reinterpret_cast<const int4 *>(ids + g * kPaintPix);
    int v[kPaintPix];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int4 a = src[q];
      v[4 * q] = a.x;
      v[4 * q + 1] = a.y;
      v[4 * q + 2] = a.z;
      v[4 * q + 3] = a.w;
    }
    unsigned c[kPaintPix];
#pragma unroll
    for (int j = 0; j < kPaintPix; ++j) c[j] = (unsigned)v[j] < (unsigned)nlut ? L[v[j]] : 0u;
    unsigned w[12];
#pragma unroll
    for (int q = 0; q < 4; ++q) pack_rgb4(c[4 * q], c[4 * q + 1], c[4 * q + 2], c[4 * q + 3], w + 3 * q);
    uint4 *dst = reinterpret_cast<uint4 *>(out + g * (kPaintPix * 3));
    dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
    dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
    dst[2] = make_uint4(w[8], w[9], w[10], w[11]);
  }
  const int64_t p = ngroups * kPaintPix + threadIdx.x;            // the last npx mod 16 pixels
  if (blockIdx.x == 0 && p < npx) {
    const int id = ids[p];
    const unsigned col = (unsigned)id < (unsigned)nlut ? L[id] : 0u;
    out[3 * p] = (uint8_t)col;
    out[3 * p + 1] = (uint8_t)(col >> 8);
    out[3 * p + 2] = (uint8_t)(col >> 16);
  }
}

// lut[c] (LDS): dataset id 0..255 of class byte c, or -1 when c has no mapping (written as 255, counted in bad[c]).
__device__ __forceinline__ unsigned sem_byte(int v, const int *lut, int &bad_cls, unsigned &bad_run,
                                             unsigned long long *__restrict__ bad_out) {
  const int c = v & 255;
  const int d = lut[c];
  if (d >= 0) return (unsigned)d;
  if (c != bad_cls) {
    if (bad_run) atomicAdd(&bad_out[bad_cls], (unsigned long long)bad_run);
    bad_cls = c;
    bad_run = 0u;
  }
  ++bad_run;
  return 255u;
}

__global__ __launch_bounds__(kThreads) void sem_paint_kernel(const int *__restrict__ ids, int64_t npx,
                                                             const int *__restrict__ lut, uint8_t *__restrict__ out,
                                                             unsigned long long *__restrict__ bad_out) {
  __shared__ int s_lut[256];
  s_lut[threadIdx.x] = lut[threadIdx.x];                          // kThreads == 256
  __syncthreads();
  int bad_cls = 0;
  unsigned bad_run = 0u;
  const int64_t ngroups = npx / kPaintPix;
  for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; g < ngroups; g += (int64_t)gridDim.x * kThreads) {
    const int4 *src = reinterpret_cast<const int4 *>(ids + g * kPaintPix);
    unsigned w[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int4 a = src[q];
      w[q] = sem_byte(a.x, s_lut, bad_cls, bad_run, bad_out) | (sem_byte(a.y, s_lut, bad_cls, bad_run, bad_out) << 8) |
             (sem_byte(a.z, s_lut, bad_cls, bad_run, bad_out) << 16) | (sem_byte(a.w, s_lut, bad_cls, bad_run, bad_out) << 24);
    }
    *reinterpret_cast<uint4 *>(out + g * kPaintPix) = make_uint4(w[0], w[1], w[2], w[3]);
  }
  const int64_t p = ngroups * kPaintPix + threadIdx.x;
  if (blockIdx.x == 0 && p < npx) out[p] = (uint8_t)sem_byte(ids[p], s_lut, bad_cls, bad_run, bad_out);
  if (bad_run) atomicAdd(&bad_out[bad_cls], (unsigned long long)bad_run);
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

inline unsigned paint_blocks(int64_t npx) {
  int64_t b = (npx / kPaintPix + kThreads - 1) / kThreads;
  if (b > kPaintBlocks) b = kPaintBlocks;
  return (unsigned)(b < 1 ? 1 : b);
}

}  // namespace

DVIS_EXPORT int dvis_pan_segment_stats(const int32_t *map, int T, int H, int W, int n, int64_t *out, int64_t *bad,
                                       void *stream) {
  const int64_t hw = (int64_t)H * W;
  DVIS_REQUIRE(T >= 0 && T <= 65535 && H >= 0 && W >= 0 && hw < ((int64_t)1 << 31) && n >= 0 && n < (1 << 30),
               "pan_segment_stats: bad sizes (T <= 65535, H * W < 2^31, 0 <= n < 2^30)");
  const int64_t nent = (int64_t)T * (n + 1);
  DVIS_REQUIRE(nent * kFields < ((int64_t)1 << 40), "pan_segment_stats: table too large");
  DVIS_REQUIRE(out && bad && (T == 0 || hw == 0 || map), "pan_segment_stats: null pointer");
  hipStream_t st = (hipStream_t)stream;
  auto *o = reinterpret_cast<unsigned long long *>(out);
  if (const int rc = dvis_zero_words(out, (size_t)nent * kFields * 2, st, "pan_segment_stats: zero")) return rc;
  if (const int rc = dvis_zero_words(bad, 2, st, "pan_segment_stats: zero")) return rc;
  if (T == 0) return DVIS_OK;
  if (hw > 0) {
    int64_t gx = (hw + kStep - 1) / kStep;
    const int64_t cap = (1024 + T - 1) / T;                       // ~4 workgroups per CU over the whole launch
    if (gx > cap) gx = cap;
    auto *bd = reinterpret_cast<unsigned long long *>(bad);
    if (n + 1 <= kMaxLdsIds) {
      hipLaunchKernelGGL(stats_kernel<true>, dim3((unsigned)gx, (unsigned)T), dim3(kThreads),
                         (size_t)(n + 1) * kFields * 4, st, map, W, hw, n, o, bd);
    } else {
      hipLaunchKernelGGL(stats_kernel<false>, dim3((unsigned)gx, (unsigned)T), dim3(kThreads), 0, st, map, W, hw, n, o, bd);
    }
    if (const int rc = dvis_check_launch("pan_segment_stats")) return rc;
  }
  hipLaunchKernelGGL(stats_finish_kernel, dim3((unsigned)((nent + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, o, nent);
  return dvis_check_launch("pan_segment_stats: finish");
}

DVIS_EXPORT int dvis_pan_paint_rgb(const int32_t *map, int64_t npx, const int32_t *lut, int nlut, uint8_t *out,
                                   void *stream) {
  DVIS_REQUIRE(npx >= 0 && npx < ((int64_t)1 << 40) && nlut >= 0, "pan_paint_rgb: bad sizes");
  DVIS_REQUIRE(npx == 0 || (map && out && (nlut == 0 || lut)), "pan_paint_rgb: null pointer");
  DVIS_REQUIRE(aligned16(map) && aligned16(out), "pan_paint_rgb: map and out must be 16-byte aligned");
  if (npx == 0) return DVIS_OK;
  hipStream_t st = (hipStream_t)stream;
  const auto *L = reinterpret_cast<const unsigned *>(lut);
  if (nlut <= kMaxLdsLut) {
    hipLaunchKernelGGL(paint_rgb_kernel<true>, dim3(paint_blocks(npx)), dim3(kThreads), (size_t)nlut * 4, st, map, npx, L,
                       nlut, out);
  } else {
    hipLaunchKernelGGL(paint_rgb_kernel<false>, dim3(paint_blocks(npx)), dim3(kThreads), 0, st, map, npx, L, nlut, out);
  }
  return dvis_check_launch("pan_paint_rgb");
}

DVIS_EXPORT int dvis_sem_paint(const int32_t *map, int64_t npx, const int32_t *lut, uint8_t *out, int64_t *bad,
                               void *stream) {
  DVIS_REQUIRE(npx >= 0 && npx < ((int64_t)1 << 40), "sem_paint: bad sizes");
  DVIS_REQUIRE(lut && bad && (npx == 0 || (map && out)), "sem_paint: null pointer");
  DVIS_REQUIRE(aligned16(map) && aligned16(out), "sem_paint: map and out must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (const int rc = dvis_zero_words(bad, 256 * 2, st, "sem_paint: zero")) return rc;
  if (npx == 0) return DVIS_OK;
  hipLaunchKernelGGL(sem_paint_kernel, dim3(paint_blocks(npx)), dim3(kThreads), 0, st, map, npx, lut, out,
                     reinterpret_cast<unsigned long long *>(bad));
  return dvis_check_launch("sem_paint");
}
