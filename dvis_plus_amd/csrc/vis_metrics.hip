// Video instance segmentation scoring (YouTube-VIS / OVIS): COCO run-length encoding and per-video track intersections — gfx950.
//
// Replaces the host passes of the reference's VIS evaluation:
//   data_video/ytvis_eval.py:256-293       mask_util.encode of every (instance, frame) on the CPU, counts decoded to str
//   ytvis_api/ytvos.py:218-287             loadRes / annToRLE: RLE areas, uncompressed ground truth -> RLE
//   ytvis_api/ytvoseval.py:176-222         computeIoU: RLE merges pair by pair, frame by frame
// Everything counts in integers (u64 atomics of integer partial sums), so results do not depend on the order atomics land.
//
// RLE layout (COCO): the runs of a frame's pixels in column-major order (index x * H + y), alternating 0 / 1 and starting
// with a run of zeros (0 when pixel (0, 0) is set).  Masks come in row-major (N, H, W) bytes, any non-zero byte is "set".
#include "dvis_common.h"

namespace {

constexpr int kRows = 128;       // rows per (column group, row chunk) of the encode and decode passes
constexpr int kWave = 64;
constexpr int kStrThreads = 256;
constexpr int kIxThreads = 256;  // intersection workgroup: 4 waves x 64 lanes x 4 pixels = one 1024-pixel chunk
constexpr int kIxChunk = kIxThreads * 4;
constexpr int kIxWords = kIxChunk / 64;

// 4 bytes of a row at columns c .. c + 3 as a 4-bit nibble (bit j = column c + j set); columns >= W read as 0
template <bool kVec>
__device__ __forceinline__ uint32_t load_nib(const uint8_t *__restrict__ row, int c, int W) {
  uint32_t v;
  if (kVec) {
    v = *reinterpret_cast<const uint32_t *>(row + c);
  } else {
    v = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (c + j < W) v |= (uint32_t)row[c + j] << (8 * j);
  }
  return (uint32_t)((v & 0xffu) != 0u) | ((uint32_t)((v & 0xff00u) != 0u) << 1) | ((uint32_t)((v & 0xff0000u) != 0u) << 2) |
         ((uint32_t)((v & 0xff000000u) != 0u) << 3);
}

// One lane owns 4 adjacent columns of one row chunk of one mask.  The pixel before row y0 of column c is (y0 - 1, c), or for
// y0 == 0 the last pixel of column c - 1 (column-major order wraps there), or a virtual 0 before pixel (0, 0).
// kWrite == false: count the transitions of each column (table (N, W, nch)) and the set pixels (area, u64 atomics).
// kWrite == true:  write the transition positions x * H + y at the table's exclusive offsets toff.
template <bool kVec, bool kWrite>
__global__ __launch_bounds__(kWave) void rle_walk_kernel(const uint8_t *__restrict__ masks, int64_t N, int H, int W, int nch,
                                                         int gblocks, int64_t *__restrict__ trans,
                                                         unsigned long long *__restrict__ area,
                                                         const int64_t *__restrict__ toff, int32_t *__restrict__ bnd) {
  const int64_t b = blockIdx.x;
  const int gb = (int)(b % gblocks);
  const int ch = (int)((b / gblocks) % nch);
  const int64_t n = b / ((int64_t)gblocks * nch);
  const int c0 = (gb * kWave + (int)threadIdx.x) * 4;
  const bool valid = c0 < W && n < N;
  const int64_t HW = (int64_t)H * W;
  const uint8_t *__restrict__ m = masks + n * HW;
  const int y0 = ch * kRows, y1 = min(H, y0 + kRows);
  unsigned ones = 0u;
  if (valid) {
    uint32_t prev;
    if (y0 > 0) {
      prev = load_nib<kVec>(m + (int64_t)(y0 - 1) * W, c0, W);
    } else {
      const uint32_t last = load_nib<kVec>(m + (int64_t)(H - 1) * W, c0, W);
      const uint32_t left = c0 > 0 ? (uint32_t)(m[(int64_t)(H - 1) * W + c0 - 1] != 0) : 0u;
      prev = ((last << 1) & 0xeu) | left;
    }
    const uint32_t cols = W - c0 >= 4 ? 0xfu : (1u << (W - c0)) - 1u;   // columns past W: no transitions (their wrap pixel may be set)
    int cnt[4] = {0, 0, 0, 0};
    int64_t off[4] = {0, 0, 0, 0};
    if (kWrite) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (c0 + j < W) off[j] = toff[(n * W + c0 + j) * nch + ch];
    }
    for (int y = y0; y < y1; y += 8) {
      uint32_t v[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) v[r] = y + r < y1 ? load_nib<kVec>(m + (int64_t)(y + r) * W, c0, W) : 0u;
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        if (y + r >= y1) break;
        const uint32_t d = (v[r] ^ prev) & cols;
        prev = v[r];
        ones += __popc(v[r]);
        if (kWrite) {
          if (d) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if ((d >> j) & 1u) bnd[off[j]++] = (c0 + j) * H + y + r;
          }
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) cnt[j] += (d >> j) & 1u;
        }
      }
    }
    if (!kWrite) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (c0 + j < W) trans[(n * W + c0 + j) * nch + ch] = cnt[j];
    }
  }
  if (!kWrite) {
    unsigned long long s = ones;
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, kWave);
    if (threadIdx.x == 0 && s && n < N) atomicAdd(&area[n], s);
  }
}

// runs of mask n from its transition positions bnd[moff[n] .. moff[n + 1]): run j = b_{j+1} - b_j with b_0 = 0 and
// b_{k+1} = H * W; the mask's runs start at moff[n] + n.
__global__ __launch_bounds__(kStrThreads) void rle_runs_kernel(const int32_t *__restrict__ bnd, const int64_t *__restrict__ moff,
                                                              int64_t HW, uint32_t *__restrict__ runs) {
  const int64_t n = blockIdx.x;
  const int64_t base = moff[n], k = moff[n + 1] - base, roff = base + n;
  for (int64_t j = threadIdx.x; j <= k; j += kStrThreads) {
    const int64_t start = j ? bnd[base + j - 1] : 0;
    const int64_t end = j < k ? bnd[base + j] : HW;
    runs[roff + j] = (uint32_t)(end - start);
  }
}

// COCO's compressed RLE string (cocoapi maskApi.c rleToString): x = cnt[i] - cnt[i - 2] for i > 2, else cnt[i]; 5-bit groups,
// low bits first, each character c + 48 with 0x20 set while more groups follow.
__device__ __forceinline__ int rle_chars(long long x, uint8_t *out) {
  int n = 0;
  bool more = true;
  while (more) {
    int c = (int)(x & 0x1f);
    x >>= 5;
    more = (c & 0x10) ? x != -1 : x != 0;
    if (more) c |= 0x20;
    if (out) out[n] = (uint8_t)(c + 48);
    ++n;
  }
  return n;
}

// inclusive scan of one value per thread over the workgroup; returns the inclusive prefix, *total = workgroup sum
__device__ __forceinline__ long long block_scan(long long v, long long *s_wave, long long *total) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  for (int o = 1; o < kWave; o <<= 1) {
    const long long u = __shfl_up(v, o, kWave);
    if (lane >= o) v += u;
  }
  if (lane == kWave - 1) s_wave[wave] = v;
  __syncthreads();
  long long before = 0, sum = 0;
  for (int w = 0; w < kStrThreads / kWave; ++w) {
    if (w < wave) before += s_wave[w];
    sum += s_wave[w];
  }
  __syncthreads();
  *total = sum;
  return v + before;
}

// one workgroup per mask.  chars == nullptr: lens[n] = the string's length; else write it at chars + str_off[n].
__global__ __launch_bounds__(kStrThreads) void rle_strings_kernel(const uint32_t *__restrict__ runs,
                                                                 const int64_t *__restrict__ run_off,
                                                                 const int64_t *__restrict__ str_off,
                                                                 int64_t *__restrict__ lens, uint8_t *__restrict__ chars) {
  __shared__ long long s_wave[kStrThreads / kWave];
  const int64_t n = blockIdx.x;
  const int64_t r0 = run_off[n], m = run_off[n + 1] - r0;
  const uint32_t *__restrict__ cnt = runs + r0;
  long long carry = 0;
  for (int64_t j0 = 0; j0 < m; j0 += kStrThreads) {
    const int64_t j = j0 + threadIdx.x;
    long long x = 0;
    int len = 0;
    if (j < m) {
      x = (long long)cnt[j];
      if (j > 2) x -= (long long)cnt[j - 2];
      len = rle_chars(x, nullptr);
    }
    long long total;
    const long long incl = block_scan(len, s_wave, &total);
    if (chars && j < m) rle_chars(x, chars + str_off[n] + carry + incl - len);
    carry += total;
  }
  if (!chars && threadIdx.x == 0) lens[n] = carry;
}

// One lane owns one column of one row chunk of one mask: finds the run holding its first pixel (upper bound over the mask's
// cumulative run ends), then walks down the column.  Output rows are written across the wave (64 adjacent columns).
__global__ __launch_bounds__(kWave) void rle_decode_kernel(const int32_t *__restrict__ ends, const int64_t *__restrict__ run_off,
                                                          int64_t N, int H, int W, int nch, int gblocks,
                                                          uint8_t *__restrict__ out) {
  const int64_t b = blockIdx.x;
  const int gb = (int)(b % gblocks);
  const int ch = (int)((b / gblocks) % nch);
  const int64_t n = b / ((int64_t)gblocks * nch);
  const int x = gb * kWave + (int)threadIdx.x;
  if (x >= W || n >= N) return;
  const int64_t r0 = run_off[n], m = run_off[n + 1] - r0;
  if (m <= 0) return;
  const int32_t *__restrict__ e = ends + r0;
  const int y0 = ch * kRows, y1 = min(H, y0 + kRows);
  const int64_t pos0 = (int64_t)x * H + y0;
  int64_t lo = 0, hi = m - 1;                     // first j with e[j] > pos0, at most m - 1
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)e[mid] > pos0) hi = mid; else lo = mid + 1;
  }
  int64_t j = lo;
  uint8_t *__restrict__ o = out + n * (int64_t)H * W + x;
  for (int y = y0; y < y1; ++y) {
    const int64_t pos = (int64_t)x * H + y;
    while (j < m - 1 && pos >= (int64_t)e[j]) ++j;
    o[(int64_t)y * W] = (uint8_t)(j & 1);
  }
}

// I[p, g] += sum over frames of popcount(pred[p, t] & gt[g, t]).  Workgroup (x, t) takes frame t's 1024-pixel chunks
// x, x + gridDim.x, ...: every track's chunk is packed by wave ballots into 16 u64 words in LDS (each mask byte is read once),
// then threads own (p, g) pairs and add the popcounts of the ANDed words into LDS u32 counters; one u64 atomic per non-zero
// pair and workgroup at the end.  The bit order inside a word is the same permutation on both sides, so the counts are exact.
template <bool kVec>
__global__ __launch_bounds__(kIxThreads) void track_ix_kernel(const uint8_t *__restrict__ pred, int64_t pstride, int P,
                                                             const uint8_t *__restrict__ gt, int64_t gstride, int G,
                                                             int64_t HW, unsigned long long *__restrict__ out) {
  extern __shared__ unsigned long long s_words[];       // [(P + G)][kIxWords], then u32 counters [P * G]
  const int K = P + G, npair = P * G;
  unsigned *s_cnt = reinterpret_cast<unsigned *>(s_words + (size_t)K * kIxWords);
  for (int i = threadIdx.x; i < npair; i += kIxThreads) s_cnt[i] = 0u;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int64_t t = blockIdx.y;
  for (int64_t base = (int64_t)blockIdx.x * kIxChunk; base < HW; base += (int64_t)gridDim.x * kIxChunk) {
    const int64_t px = base + wave * (kWave * 4) + lane * 4;
    __syncthreads();                                     // the previous chunk's words are consumed
    for (int k = 0; k < K; ++k) {
      const uint8_t *__restrict__ src = (k < P ? pred + k * pstride : gt + (k - P) * gstride) + t * HW;
      uint32_t v = 0u;
      if (kVec) {
        if (px < HW) v = *reinterpret_cast<const uint32_t *>(src + px);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (px + j < HW) v |= (uint32_t)src[px + j] << (8 * j);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned long long w = __ballot(((v >> (8 * j)) & 0xffu) != 0u);
        if (lane == j) s_words[(size_t)k * kIxWords + wave * 4 + j] = w;
      }
    }
    __syncthreads();
    for (int q = threadIdx.x; q < npair; q += kIxThreads) {
      const int p = q / G, g = q - p * G;
      const unsigned long long *a = s_words + (size_t)p * kIxWords, *c = s_words + (size_t)(P + g) * kIxWords;
      unsigned acc = 0u;
#pragma unroll
      for (int w = 0; w < kIxWords; ++w) acc += (unsigned)__popcll(a[w] & c[w]);
      s_cnt[q] += acc;
    }
  }
  __syncthreads();
  for (int q = threadIdx.x; q < npair; q += kIxThreads)
    if (s_cnt[q]) atomicAdd(&out[q], (unsigned long long)s_cnt[q]);
}

int walk_grid(int64_t N, int H, int W, int groups_per_lane, int *nch, int *gblocks, int64_t *blocks) {
  *nch = (H + kRows - 1) / kRows;
  const int64_t cols = (W + groups_per_lane - 1) / groups_per_lane;
  *gblocks = (int)((cols + kWave - 1) / kWave);
  *blocks = N * *nch * *gblocks;
  return *blocks < ((int64_t)1 << 31);
}

}  // namespace

DVIS_EXPORT int dvis_rle_encode(const uint8_t *masks, int64_t N, int H, int W, int phase, int64_t *trans, int64_t *area,
                                const int64_t *toff, const int64_t *moff, int32_t *bnd, uint32_t *runs, void *stream) {
  DVIS_REQUIRE(N >= 0 && H >= 1 && W >= 1 && (int64_t)H * W < ((int64_t)1 << 31) && (phase == 0 || phase == 1),
               "rle_encode: bad sizes (H, W >= 1, H * W < 2^31, phase 0 or 1)");
  int nch, gblocks;
  int64_t blocks;
  DVIS_REQUIRE(walk_grid(N, H, W, 4, &nch, &gblocks, &blocks), "rle_encode: too many masks");
  hipStream_t st = (hipStream_t)stream;
  const bool vec = W % 4 == 0 && ((uintptr_t)masks & 3u) == 0;
  if (phase == 0) {
    DVIS_REQUIRE(trans && area && (N == 0 || masks), "rle_encode: null pointer (phase 0)");
    if (const int rc = dvis_zero_words(area, (size_t)N * 2, st, "rle_encode: zero")) return rc;
    if (N == 0) return DVIS_OK;
    auto *a = reinterpret_cast<unsigned long long *>(area);
    if (vec)
      hipLaunchKernelGGL((rle_walk_kernel<true, false>), dim3((unsigned)blocks), dim3(kWave), 0, st, masks, N, H, W, nch,
                         gblocks, trans, a, nullptr, nullptr);
    else
      hipLaunchKernelGGL((rle_walk_kernel<false, false>), dim3((unsigned)blocks), dim3(kWave), 0, st, masks, N, H, W, nch,
                         gblocks, trans, a, nullptr, nullptr);
    return dvis_check_launch("rle_walk_kernel<count>");
  }
  DVIS_REQUIRE(toff && moff && runs && (N == 0 || masks), "rle_encode: null pointer (phase 1)");
  if (N == 0) return DVIS_OK;
  if (vec)
    hipLaunchKernelGGL((rle_walk_kernel<true, true>), dim3((unsigned)blocks), dim3(kWave), 0, st, masks, N, H, W, nch, gblocks,
                       nullptr, nullptr, toff, bnd);
  else
    hipLaunchKernelGGL((rle_walk_kernel<false, true>), dim3((unsigned)blocks), dim3(kWave), 0, st, masks, N, H, W, nch,
                       gblocks, nullptr, nullptr, toff, bnd);
  if (const int rc = dvis_check_launch("rle_walk_kernel<write>")) return rc;
  DVIS_REQUIRE(N < ((int64_t)1 << 31), "rle_encode: too many masks");
  hipLaunchKernelGGL(rle_runs_kernel, dim3((unsigned)N), dim3(kStrThreads), 0, st, bnd, moff, (int64_t)H * W, runs);
  return dvis_check_launch("rle_runs_kernel");
}

DVIS_EXPORT int dvis_rle_strings(const uint32_t *runs, const int64_t *run_off, int64_t N, const int64_t *str_off, int64_t *lens,
                                 uint8_t *chars, void *stream) {
  DVIS_REQUIRE(N >= 0 && N < ((int64_t)1 << 31), "rle_strings: bad N");
  DVIS_REQUIRE(run_off && (chars ? str_off != nullptr : lens != nullptr) && (N == 0 || runs),
               "rle_strings: null pointer (count: lens; write: str_off and chars)");
  if (N == 0) return DVIS_OK;
  hipLaunchKernelGGL(rle_strings_kernel, dim3((unsigned)N), dim3(kStrThreads), 0, (hipStream_t)stream, runs, run_off, str_off,
                     lens, chars);
  return dvis_check_launch("rle_strings_kernel");
}

DVIS_EXPORT int dvis_rle_decode(const int32_t *ends, const int64_t *run_off, int64_t N, int H, int W, uint8_t *out,
                                void *stream) {
  DVIS_REQUIRE(N >= 0 && H >= 1 && W >= 1 && (int64_t)H * W < ((int64_t)1 << 31), "rle_decode: bad sizes");
  DVIS_REQUIRE(run_off && out && (N == 0 || ends), "rle_decode: null pointer");
  int nch, gblocks;
  int64_t blocks;
  DVIS_REQUIRE(walk_grid(N, H, W, 1, &nch, &gblocks, &blocks), "rle_decode: too many masks");
  if (N == 0) return DVIS_OK;
  hipLaunchKernelGGL(rle_decode_kernel, dim3((unsigned)blocks), dim3(kWave), 0, (hipStream_t)stream, ends, run_off, N, H, W,
                     nch, gblocks, out);
  return dvis_check_launch("rle_decode_kernel");
}

DVIS_EXPORT int dvis_track_intersections(const uint8_t *pred, int64_t pred_stride, int P, const uint8_t *gt, int64_t gt_stride,
                                         int G, int T, int64_t HW, int accumulate, int64_t *out, void *stream) {
  DVIS_REQUIRE(P >= 0 && G >= 0 && T >= 0 && T <= 65535 && HW >= 0 && HW < ((int64_t)1 << 31) && pred_stride >= 0 &&
                   gt_stride >= 0,
               "track_intersections: bad sizes (T <= 65535, H * W < 2^31)");
  const size_t lds = (size_t)(P + G) * kIxWords * 8 + (size_t)P * G * 4;
  DVIS_REQUIRE(lds <= 64 * 1024, "track_intersections: %d x %d tracks need %zu B of LDS (> 64 KB)", P, G, lds);
  DVIS_REQUIRE(out && (P == 0 || G == 0 || T == 0 || HW == 0 || (pred && gt)), "track_intersections: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (!accumulate)
    if (const int rc = dvis_zero_words(out, (size_t)P * G * 2, st, "track_intersections: zero")) return rc;
  if (P == 0 || G == 0 || T == 0 || HW == 0) return DVIS_OK;
  int64_t gx = (HW + kIxChunk - 1) / kIxChunk;
  const int64_t cap = (2048 + T - 1) / T;               // ~8 workgroups per CU over the launch
  if (gx > cap) gx = cap;
  const bool vec = HW % 4 == 0 && pred_stride % 4 == 0 && gt_stride % 4 == 0 && ((uintptr_t)pred & 3u) == 0 &&
                   ((uintptr_t)gt & 3u) == 0;
  auto *o = reinterpret_cast<unsigned long long *>(out);
  if (vec)
    hipLaunchKernelGGL(track_ix_kernel<true>, dim3((unsigned)gx, (unsigned)T), dim3(kIxThreads), lds, st, pred, pred_stride,
                       P, gt, gt_stride, G, HW, o);
  else
    hipLaunchKernelGGL(track_ix_kernel<false>, dim3((unsigned)gx, (unsigned)T), dim3(kIxThreads), lds, st, pred, pred_stride,
                       P, gt, gt_stride, G, HW, o);
  return dvis_check_launch("track_ix_kernel");
}
