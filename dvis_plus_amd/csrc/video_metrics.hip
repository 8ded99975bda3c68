// Video segmentation metrics as integer histograms over (T, H, W) id maps — gfx950.
//
// Replaces the per-segment / per-window numpy passes of the reference's scoring scripts (DVIS_Plus/utils/):
//   eval_vpq_vspw.py:77-216         np.unique over uint64 (gt, pred) tubes, once per window start and window length
//   segmentation_and_tracking_quality.py:131-221   np.unique / np.add.at per frame (class confusion, track pair areas)
//   eval_miou_vspw.py:_generate_matrix              np.bincount of num_class * gt + pred per frame
//   eval_vc_vspw.py:get_common                      k - 1 full-frame compares per window start and k
// Every metric reduces to counts that these three kernels produce in one pass over the pixels; the host (video_metrics.py)
// turns them into the reference's floats.  Counting is integer only (LDS u32, global u64 atomics): results do not depend on
// the order in which the atomics land.
//
// Histogram kernels: one thread owns 8 contiguous pixels per step of a grid-stride loop and keeps a running (bin, count):
// a bin change flushes the run with ONE atomic, and the run carries over from one step to the next.  The maps are blocky
// (segments are regions), so a run covers many pixels and the atomics stay far below one per pixel.  Bins live in LDS
// while the whole table fits in 64 KB (two workgroups per CU), then one u64 global atomic per non-zero bin and workgroup;
// larger tables take the same loop with the run flushed straight into global memory.
#include "dvis_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPix = 8;                     // contiguous pixels per thread and step
constexpr int kStep = kThreads * kPix;      // pixels per workgroup and step
constexpr size_t kLdsBytes = 64 * 1024;     // histogram + GT id table per workgroup on the LDS path
constexpr int kMaxTable = 16384;            // GT ids of one video (held in LDS on both paths)
constexpr int kBinDrop = -1;                // pixel not counted (outside the matrix by definition)
constexpr int kBinBad = -2;                 // pixel outside the declared value range: counted in `bad`

// (GT segment, predicted segment) of dvis_pan_pair_hist.  GT row: 0 VOID (id 0), 1 + i for table[i], ng + 1 for an id
// that the table does not list; prediction column p in 0..np.
struct PairMap {
  const int *table;    // sorted ascending, in LDS
  int ng, np;
  __device__ PairMap(const int *t, int ng_, int np_, int) : table(t), ng(ng_), np(np_) {}
  __device__ int operator()(int g, int p) const {
    if ((unsigned)p > (unsigned)np) return kBinBad;
    int row;
    if (g == 0) {
      row = 0;
    } else {
      int lo = 0, hi = ng;                  // lower_bound
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (table[mid] < g) lo = mid + 1; else hi = mid;
      }
      row = (lo < ng && table[lo] == g) ? lo + 1 : ng + 1;
    }
    return row * (np + 1) + p;
  }
};

// VSPW's label preprocessing (eval_miou_vspw.py:_generate_matrix) on uint8 labels: 0 -> 255, then - 1 in uint8, rows >= nc
// dropped; bin = nc * gt + pred as the reference's bincount (a prediction >= nc lands in the next row, as there); a bin
// past nc * nc (where the reference's reshape fails) or a negative prediction is `bad`.
struct SemMap {
  int nc;
  __device__ SemMap(const int *, int, int, int nc_) : nc(nc_) {}
  __device__ int operator()(int g, int p) const {
    int gg = g & 255;
    gg = ((gg == 0 ? 255 : gg) - 1) & 255;
    if (gg >= nc) return kBinDrop;
    const int64_t b = (int64_t)nc * gg + p;
    if (p < 0 || b >= (int64_t)nc * nc) return kBinBad;
    return (int)b;
  }
};

template <bool kLds>
__device__ __forceinline__ void flush(int bin, unsigned cnt, unsigned *s_hist, unsigned long long *g_hist,
                                      unsigned long long &bad) {
  if (bin >= 0) {
    if (kLds) atomicAdd(&s_hist[bin], cnt);
    else atomicAdd(&g_hist[bin], (unsigned long long)cnt);
  } else if (bin == kBinBad) {
    bad += cnt;
  }
}

// grid (gx, frames); workgroup (x, f) counts frame f's pixels x * kStep + i * gx * kStep .. into frame f's nbins bins.
template <class Map, bool kLds>
__global__ __launch_bounds__(kThreads) void hist_kernel(const int *__restrict__ a, const int *__restrict__ b,
                                                        int64_t frame_px, const int *__restrict__ table, int ng, int np,
                                                        int nc, int nbins, unsigned long long *__restrict__ out,
                                                        unsigned long long *__restrict__ bad_out) {
  extern __shared__ int smem[];
  int *s_table = smem;
  unsigned *s_hist = reinterpret_cast<unsigned *>(smem + ng);
  for (int i = threadIdx.x; i < ng; i += kThreads) s_table[i] = table[i];
  if (kLds)
    for (int i = threadIdx.x; i < nbins; i += kThreads) s_hist[i] = 0u;
  __syncthreads();

  const Map map(s_table, ng, np, nc);
  const int64_t f = blockIdx.y;
  const int *__restrict__ af = a + f * frame_px;
  const int *__restrict__ bf = b + f * frame_px;
  unsigned long long *g_hist = out + f * (int64_t)nbins;
  int run_bin = kBinDrop;
  unsigned run = 0u;
  unsigned long long bad = 0ull;
  for (int64_t base = (int64_t)blockIdx.x * kStep + threadIdx.x * kPix; base < frame_px;
       base += (int64_t)gridDim.x * kStep) {
    const int n = (int)(frame_px - base < kPix ? frame_px - base : kPix);
    int gv[kPix], pv[kPix];
#pragma unroll
    for (int j = 0; j < kPix; ++j) {
      gv[j] = j < n ? af[base + j] : 0;
      pv[j] = j < n ? bf[base + j] : 0;
    }
#pragma unroll
    for (int j = 0; j < kPix; ++j) {
      if (j >= n) break;
      const int bin = map(gv[j], pv[j]);
      if (bin == run_bin) {
        ++run;
      } else {
        if (run) flush<kLds>(run_bin, run, s_hist, g_hist, bad);
        run_bin = bin;
        run = 1u;
      }
    }
  }
  if (run) flush<kLds>(run_bin, run, s_hist, g_hist, bad);
  if (bad) atomicAdd(bad_out, bad);
  if (kLds) {
    __syncthreads();
    for (int i = threadIdx.x; i < nbins; i += kThreads)
      if (s_hist[i]) atomicAdd(&g_hist[i], (unsigned long long)s_hist[i]);
  }
}

template <class Map>
int launch_hist(const char *what, const int *a, const int *b, int64_t frame_px, int frames, const int *table, int ng,
                int np, int nc, int64_t nbins, int64_t *out, int64_t *bad, hipStream_t st) {
  if (const int rc = dvis_zero_words(out, (size_t)(frames * nbins * 2), st, what)) return rc;
  if (const int rc = dvis_zero_words(bad, 2, st, what)) return rc;
  if (frames == 0 || frame_px == 0) return DVIS_OK;
  int64_t gx = (frame_px + kStep - 1) / kStep;
  const int64_t cap = (1024 + frames - 1) / frames;           // ~4 workgroups per CU over the whole launch
  if (gx > cap) gx = cap;
  const size_t lds = (size_t)(ng + nbins) * 4;
  auto *o = reinterpret_cast<unsigned long long *>(out);
  auto *bd = reinterpret_cast<unsigned long long *>(bad);
  if (lds <= kLdsBytes) {
    hipLaunchKernelGGL((hist_kernel<Map, true>), dim3((unsigned)gx, (unsigned)frames), dim3(kThreads), lds, st, a, b,
                       frame_px, table, ng, np, nc, (int)nbins, o, bd);
  } else {
    hipLaunchKernelGGL((hist_kernel<Map, false>), dim3((unsigned)gx, (unsigned)frames), dim3(kThreads),
                       (size_t)ng * 4, st, a, b, frame_px, table, ng, np, nc, (int)nbins, o, bd);
  }
  return dvis_check_launch(what);
}

// VC counts.  One thread owns one pixel and walks its frames backwards once, keeping the length of the run of equal
// values that starts at frame t (GT and prediction); the window [t, t + k) is GT-constant iff the GT run is >= k.  Per
// (k, t) a wave adds its ballot's popcount to an LDS counter; one u64 atomic per counter and workgroup at the end.
constexpr int kMaxK = 4;
struct Ks {
  int k[kMaxK];
};

__global__ __launch_bounds__(kThreads) void vc_kernel(const int *__restrict__ gt, const int *__restrict__ pred, int T,
                                                      int64_t hw, Ks ks, int nk, unsigned long long *__restrict__ out_gt,
                                                      unsigned long long *__restrict__ out_both) {
  extern __shared__ unsigned s_cnt[];     // [2][nk][T]
  const int ncnt = 2 * nk * T;
  for (int i = threadIdx.x; i < ncnt; i += kThreads) s_cnt[i] = 0u;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  for (int64_t base = (int64_t)blockIdx.x * kThreads; base < hw; base += (int64_t)gridDim.x * kThreads) {  // wave-uniform trips
    const int64_t p = base + threadIdx.x;
    const bool valid = p < hw;
    const int64_t pc = valid ? p : hw - 1;
    int prev_g = 0, prev_p = 0, rg = 0, rp = 0;
    for (int t = T - 1; t >= 0; --t) {
      const int g = gt[(int64_t)t * hw + pc], q = pred[(int64_t)t * hw + pc];
      rg = (rg && g == prev_g) ? rg + 1 : 1;
      rp = (rp && q == prev_p) ? rp + 1 : 1;
      prev_g = g;
      prev_p = q;
      for (int i = 0; i < nk; ++i) {
        const int k = ks.k[i];
        if (t >= T - k) continue;           // the reference's range(len - k): windows 0 .. T - k - 1
        const bool okg = valid && rg >= k;
        const unsigned long long mg = __ballot(okg), mb = __ballot(okg && rp >= k);
        if (lane == 0) {
          if (mg) atomicAdd(&s_cnt[i * T + t], (unsigned)__popcll(mg));
          if (mb) atomicAdd(&s_cnt[(nk + i) * T + t], (unsigned)__popcll(mb));
        }
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < ncnt; i += kThreads) {
    const unsigned v = s_cnt[i];
    if (!v) continue;
    if (i < nk * T) atomicAdd(&out_gt[i], (unsigned long long)v);
    else atomicAdd(&out_both[i - nk * T], (unsigned long long)v);
  }
}

}  // namespace

DVIS_EXPORT int dvis_pan_pair_hist(const int32_t *gt, const int32_t *pred, const int32_t *gt_table, int Ng, int Np, int T,
                                   int64_t HW, int64_t *out, int64_t *bad, void *stream) {
  DVIS_REQUIRE(Ng >= 0 && Ng <= kMaxTable && Np >= 0 && T >= 0 && T <= 65535 && HW >= 0 && HW < ((int64_t)1 << 31),
               "pan_pair_hist: bad sizes (Ng <= %d, T <= 65535, H * W < 2^31)", kMaxTable);
  const int64_t nbins = (int64_t)(Ng + 2) * (Np + 1);
  DVIS_REQUIRE(nbins < ((int64_t)1 << 31) && (int64_t)T * nbins < ((int64_t)1 << 40), "pan_pair_hist: histogram too large");
  DVIS_REQUIRE(out && bad && (T == 0 || HW == 0 || (gt && pred)) && (Ng == 0 || gt_table),
               "pan_pair_hist: null pointer");
  return launch_hist<PairMap>("pan_pair_hist", gt, pred, HW, T, gt_table, Ng, Np, 0, nbins, out, bad, (hipStream_t)stream);
}

DVIS_EXPORT int dvis_sem_confusion(const int32_t *gt, const int32_t *pred, int64_t n, int num_class, int64_t *out,
                                   int64_t *bad, void *stream) {
  DVIS_REQUIRE(num_class >= 1 && num_class <= 256 && n >= 0 && n < ((int64_t)1 << 40),
               "sem_confusion: bad sizes (num_class 1..256)");
  DVIS_REQUIRE(out && bad && (n == 0 || (gt && pred)), "sem_confusion: null pointer");
  return launch_hist<SemMap>("sem_confusion", gt, pred, n, 1, nullptr, 0, 0, num_class, (int64_t)num_class * num_class,
                             out, bad, (hipStream_t)stream);
}

DVIS_EXPORT int dvis_video_consistency(const int32_t *gt, const int32_t *pred, int T, int64_t HW, const int32_t *ks, int nk,
                                       int64_t *gt_const, int64_t *both_const, void *stream) {
  DVIS_REQUIRE(T >= 0 && HW >= 0 && nk >= 1 && nk <= kMaxK && ks, "video_consistency: bad sizes (1..%d window lengths)", kMaxK);
  DVIS_REQUIRE((size_t)2 * nk * T * 4 <= kLdsBytes, "video_consistency: more than %zu frames x window lengths",
               kLdsBytes / 8);
  Ks kk{};
  for (int i = 0; i < nk; ++i) {
    DVIS_REQUIRE(ks[i] >= 1, "video_consistency: window length must be >= 1");
    kk.k[i] = ks[i];
  }
  DVIS_REQUIRE(gt_const && both_const && (T == 0 || HW == 0 || (gt && pred)), "video_consistency: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (const int rc = dvis_zero_words(gt_const, (size_t)nk * T * 2, st, "video_consistency: zero")) return rc;
  if (const int rc = dvis_zero_words(both_const, (size_t)nk * T * 2, st, "video_consistency: zero")) return rc;
  if (T == 0 || HW == 0) return DVIS_OK;
  int64_t blocks = (HW + kThreads - 1) / kThreads;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(vc_kernel, dim3((unsigned)blocks), dim3(kThreads), (size_t)2 * nk * T * 4, st, gt, pred, T, HW, kk, nk,
                     reinterpret_cast<unsigned long long *>(gt_const), reinterpret_cast<unsigned long long *>(both_const));
  return dvis_check_launch("vc_kernel");
}
