// Test-time resize of decoded video frames on the device — gfx950.
//
// Replaces the host-side ResizeShortestEdge of the reference's demo and eval loaders:
//   demo_video/predictor.py:239-248           per frame: [:, :, ::-1] (FORMAT "RGB"), ResizeTransform.apply_image,
//                                             astype("float32").transpose(2, 0, 1)
//   dvis_Plus/data_video/dataset_mapper.py:333 the same transform in the eval mapper
// detectron2's ResizeTransform.apply_image resizes a uint8 image with Pillow's BILINEAR filter, and Pillow's 8-bit resample is
// integer fixed point over coefficient tables that depend only on the two sizes (ImagingResample, PRECISION_BITS = 22): a
// horizontal pass into a uint8 intermediate, then a vertical pass over it, each output = clip8(2^21 + sum in[xmin + k] * coef[k]).
// The tables (xmin, taps, int32 coefficients per output index) are built on the host (functions.resize_tables) in Pillow's own
// double arithmetic, so the device does integer multiply-adds only and the result is byte-identical to Pillow.
//
// One launch.  A workgroup owns (frame, band of bh output rows, tile of bw output columns):
//   1. it copies the input rows and columns its band and tile need (their spans come from the tables) into LDS with 16-byte
//      loads: a row segment starts at any byte (3-byte pixels, any width), so each row is staged from its 16-byte-aligned
//      start and remembers its offset; chunks that would cross the end of the input fall back to byte loads;
//   2. horizontal pass: every staged row x every output column of the tile, three channels, into a planar uint8 intermediate
//      in LDS (the value Pillow's horizontal pass writes for that pixel);
//   3. vertical pass: the band's output rows, written straight into the (T, 3, h, w) planes (channel order reversed on request).
//      A plane row of the tile starts at any byte (h * w and w may be odd), so each thread makes 4 bytes of one aligned dword of
//      the plane and stores it whole when all 4 belong to the tile, byte by byte at the two ends of the tile's row.
// The tile (bw, bh) is sized on the host so that the staged block, the intermediate and the tables fit 64 KB of LDS.  Integer
// only, no atomics: run-to-run identical.
#include "dvis_common.h"

#include <math.h>

namespace {

constexpr int kThreads = 256;
constexpr int kBw = 64;                      // output columns per tile (halved when a tile would not fit the LDS budget)
constexpr int kBh = 32;                      // output rows per band (halved first)
constexpr size_t kLdsBudget = 64 * 1024;
constexpr int kPrecision = 22;               // Pillow's PRECISION_BITS

inline int64_t round16(int64_t v) { return (v + 15) & ~(int64_t)15; }

// Input pixels a tile of n outputs can touch along one axis: xmin of the first ... xmin + taps of the last.  With
// center = (o + 0.5) * scale, xmin = trunc(center - support + 0.5) and xend = trunc(center + support + 0.5), the span is at most
// (n - 1) * scale + 2 * support + 1; +2 covers the rounding of the doubles.
inline int span_cap(int n, int in, double scale, double support) {
  const double s = (n - 1) * scale + 2.0 * support;
  const int64_t cap = (int64_t)s + 3;
  return (int)(cap < in ? cap : in);
}

struct Layout {
  int bw, bh, cap_x, cap_y;
  int64_t pitch_in, off_h, off_tx, off_ty, bytes;
};

inline Layout layout(int bw, int bh, int H, int W, int h, int w, int kx, int ky) {
  Layout L;
  const double sx = (double)W / w, sy = (double)H / h;
  L.bw = bw;
  L.bh = bh;
  L.cap_x = span_cap(bw, W, sx, sx > 1.0 ? sx : 1.0);
  L.cap_y = span_cap(bh, H, sy, sy > 1.0 ? sy : 1.0);
  L.pitch_in = round16((int64_t)L.cap_x * 3 + 30);   // 16-byte aligned start up to 15 bytes early, last chunk up to 15 late
  L.off_h = (int64_t)L.cap_y * L.pitch_in;
  L.off_tx = L.off_h + round16((int64_t)L.cap_y * 3 * bw);
  L.off_ty = L.off_tx + round16((int64_t)bw * (kx + 2) * 4);
  L.bytes = L.off_ty + round16((int64_t)bh * (ky + 2) * 4);
  return L;
}

// (row, col) over a row-major grid of `ncol` columns, thread `i` first, kThreads items per step: one division per thread, then
// an add and a carry per step.
struct Walk {
  int col, row, dcol, drow, ncol;
  __device__ Walk(int i, int n) : col(i % n), row(i / n), dcol(kThreads % n), drow(kThreads / n), ncol(n) {}
  __device__ void next() {
    col += dcol;
    row += drow;
    if (col >= ncol) {
      col -= ncol;
      ++row;
    }
  }
};

__device__ __forceinline__ unsigned clip8(int acc) {
  if (acc <= 0) return 0u;
  const int v = acc >> kPrecision;
  return v > 255 ? 255u : (unsigned)v;
}

// grid (column tiles, row bands, frames).  xtab / ytab: per output index [xmin, taps, coef[0..k-1]] (int32, k = kx / ky).
__global__ __launch_bounds__(kThreads) void frame_resize_kernel(const uint8_t *__restrict__ in, int64_t in_bytes, int H, int W,
                                                                uint8_t *__restrict__ out, int h, int w,
                                                                const int *__restrict__ xtab, int kx,
                                                                const int *__restrict__ ytab, int ky, int bw, int bh,
                                                                int cap_x, int cap_y, int pitch_in, int off_h, int off_tx,
                                                                int off_ty, int reverse) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint8_t *s_in = smem;
  uint8_t *s_h = smem + off_h;
  int *s_tx = reinterpret_cast<int *>(smem + off_tx);
  int *s_ty = reinterpret_cast<int *>(smem + off_ty);
  const int t = blockIdx.z;
  const int ox0 = blockIdx.x * bw, oy0 = blockIdx.y * bh;
  const int nx = min(bw, w - ox0), ny = min(bh, h - oy0);
  const int sx = kx + 2, sy = ky + 2;

  // the tile's table rows; spans from the first / last entries (xmin and xmin + taps are non-decreasing in the output index)
  for (int i = threadIdx.x; i < nx * sx; i += kThreads) s_tx[i] = xtab[(int64_t)ox0 * sx + i];
  for (int i = threadIdx.x; i < ny * sy; i += kThreads) s_ty[i] = ytab[(int64_t)oy0 * sy + i];
  const int *xl = xtab + (int64_t)(ox0 + nx - 1) * sx;
  const int *yl = ytab + (int64_t)(oy0 + ny - 1) * sy;
  const int c0 = max(xtab[(int64_t)ox0 * sx], 0);
  const int r0 = max(ytab[(int64_t)oy0 * sy], 0);
  const int span_x = max(min(min(xl[0] + xl[1], W) - c0, cap_x), 0);
  const int span_y = max(min(min(yl[0] + yl[1], H) - r0, cap_y), 0);

  // 1. stage rows r0 .. r0 + span_y - 1, bytes of columns c0 .. c0 + span_x - 1, from each row's 16-byte-aligned start
  const int nchunk = (int)((((int64_t)span_x * 3 + 15 + 15) >> 4));
  const int64_t frame_off = (int64_t)t * H * W * 3;
  for (Walk it(threadIdx.x, nchunk); it.row < span_y; it.next()) {
    const int r = it.row, q = it.col;
    const int64_t start = frame_off + ((int64_t)(r0 + r) * W + c0) * 3;
    const int64_t g = (start & ~(int64_t)15) + (int64_t)q * 16;
    if ((int64_t)q * 16 >= (start & 15) + (int64_t)span_x * 3) continue;   // past the segment (its last chunk is short)
    uint8_t *dst = s_in + (int64_t)r * pitch_in + q * 16;
    if (g + 16 <= in_bytes) {
      *reinterpret_cast<uint4 *>(dst) = *reinterpret_cast<const uint4 *>(in + g);
    } else {
      for (int b = 0; b < 16; ++b) dst[b] = g + b < in_bytes ? in[g + b] : (uint8_t)0;
    }
  }
  __syncthreads();

  // 2. horizontal pass: staged row r, output column j -> s_h[(r * 3 + c) * bw + j]
  for (Walk it(threadIdx.x, nx); it.row < span_y; it.next()) {
    const int r = it.row, j = it.col;
    const int *tx = s_tx + j * sx;
    const int64_t start = frame_off + ((int64_t)(r0 + r) * W + c0) * 3;
    const int xm = tx[0] - c0;
    const int taps = min(tx[1], span_x - xm);
    const uint8_t *src = s_in + (int64_t)r * pitch_in + (start & 15) + xm * 3;
    int a0 = 1 << (kPrecision - 1), a1 = a0, a2 = a0;
    for (int k = 0; k < taps; ++k) {
      const int cf = tx[2 + k];
      a0 += (int)src[3 * k] * cf;
      a1 += (int)src[3 * k + 1] * cf;
      a2 += (int)src[3 * k + 2] * cf;
    }
    s_h[(r * 3 + 0) * bw + j] = (uint8_t)clip8(a0);
    s_h[(r * 3 + 1) * bw + j] = (uint8_t)clip8(a1);
    s_h[(r * 3 + 2) * bw + j] = (uint8_t)clip8(a2);
  }
  __syncthreads();

  // 3. vertical pass: one aligned dword of an output plane row per item; plane c takes source channel c (2 - c reversed).
  // The 4 bytes are computed unconditionally (a byte outside the tile's row reads a neighbouring LDS byte) and only the
  // tile's own bytes are stored.
  const int units = (nx + 3) / 4 + 1;                 // dwords a row segment of nx bytes can touch
  for (int c = 0; c < 3; ++c) {
    const int cs = reverse ? 2 - c : c;
    for (Walk it(threadIdx.x, units); it.row < ny; it.next()) {
      const int oyl = it.row, u = it.col;
      const int64_t seg = (((int64_t)t * 3 + c) * h + (oy0 + oyl)) * w + ox0;   // the tile's row in the output, flat
      const int64_t d = (seg & ~(int64_t)3) + 4 * (int64_t)u;
      const int j0 = (int)(d - seg);                  // tile column of the dword's first byte (-3 .. nx - 1)
      if (j0 >= nx) continue;
      const int *ty = s_ty + oyl * sy;
      const int ym = ty[0] - r0;
      const int taps = min(ty[1], span_y - ym);
      const uint8_t *col = s_h + (ym * 3 + cs) * bw + j0;
      int acc[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[b] = 1 << (kPrecision - 1);
      for (int k = 0; k < taps; ++k) {
        const int cf = ty[2 + k];
        const uint8_t *row = col + k * 3 * bw;
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[b] += (int)row[b] * cf;
      }
      if (j0 >= 0 && j0 + 4 <= nx) {
        *reinterpret_cast<unsigned *>(out + d) = clip8(acc[0]) | (clip8(acc[1]) << 8) | (clip8(acc[2]) << 16) |
                                                 (clip8(acc[3]) << 24);
      } else {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          if (j0 + b >= 0 && j0 + b < nx) out[d + b] = (uint8_t)clip8(acc[b]);
        }
      }
    }
  }
}

}  // namespace

namespace {

// The largest tile (bw <= kBw, bh <= kBh, bh halved first) whose LDS fits kLdsBudget; DVIS_E_UNSUPPORTED for extreme down-scales.
int pick_tile(int H, int W, int h, int w, int kx, int ky, int *bw, int *bh) {
  int tw = kBw, th = kBh;
  for (;;) {
    const Layout L = layout(tw, th, H, W, h, w, kx, ky);
    if ((size_t)L.bytes <= kLdsBudget) {
      *bw = tw;
      if (bh) *bh = th;
      return (int)L.bytes;
    }
    if (th > 1) {
      th /= 2;
    } else if (tw > 4) {
      tw /= 2;
    } else {
      dvis_set_error("resize_frames_u8: %dx%d -> %dx%d needs more than %zu bytes of LDS per 4x1 tile", H, W, h, w, kLdsBudget);
      return DVIS_E_UNSUPPORTED;
    }
  }
}

}  // namespace

DVIS_EXPORT int dvis_resize_frames_u8(const uint8_t *in, int T, int H, int W, uint8_t *out, int h, int w, const int32_t *xtab,
                                      int kx, const int32_t *ytab, int ky, int reverse, void *stream) {
  DVIS_REQUIRE(T >= 0 && T <= 65535 && H > 0 && W > 0 && h > 0 && w > 0 && kx >= 1 && ky >= 1 && kx <= 4096 && ky <= 4096,
               "resize_frames_u8: bad sizes (0 <= T <= 65535, positive sizes)");
  DVIS_REQUIRE((int64_t)H * W * 3 < ((int64_t)1 << 31) && (int64_t)h * w * 3 < ((int64_t)1 << 31),
               "resize_frames_u8: a frame must be < 2^31 bytes");
  if (T == 0) return DVIS_OK;
  DVIS_REQUIRE(in && out && xtab && ytab, "resize_frames_u8: null pointer");
  DVIS_REQUIRE(((uintptr_t)in & 15u) == 0 && ((uintptr_t)out & 15u) == 0, "resize_frames_u8: in and out must be 16-byte aligned");
  int bw = 0, bh = 0;
  const int bytes = pick_tile(H, W, h, w, kx, ky, &bw, &bh);
  if (bytes < 0) return bytes;
  const Layout L = layout(bw, bh, H, W, h, w, kx, ky);
  const dim3 grid((unsigned)((w + bw - 1) / bw), (unsigned)((h + bh - 1) / bh), (unsigned)T);
  hipLaunchKernelGGL(frame_resize_kernel, grid, dim3(kThreads), (size_t)L.bytes, (hipStream_t)stream, in,
                     (int64_t)T * H * W * 3, H, W, out, h, w, xtab, kx, ytab, ky, bw, bh, L.cap_x, L.cap_y, (int)L.pitch_in,
                     (int)L.off_h, (int)L.off_tx, (int)L.off_ty, reverse ? 1 : 0);
  return dvis_check_launch("resize_frames_u8");
}
