// K12 — time-series feature engineering of the structured-data workflow: get_TimeBeforeAfter (Applications/StructuredData.py:482-519)
// and get_RollingStats (:556-607) as scans over rows sorted by (group, time).
//
// nnl_seg_event_gaps: row indices are monotone, so no segmented operator is needed.  In scan position p (p = i forward, p = n - 1 - i
// backward) the first position of p's group is an inclusive max-scan of `boundary ? p : -1` and the last event before p an exclusive
// max-scan of `event ? p : -1`; the event belongs to p's group iff it is not before the group's first position.  Each direction is
// three launches (both directions ride in one grid, blockIdx.y): per-tile maxima, an exclusive scan of the tile maxima by ONE
// workgroup, and the in-tile scan with the carry applied.  No workgroup ever waits for another: there is no look-back.
// The tile carries need 2 ints per tile and direction; they live in the outputs themselves, in the slots of the tile's first row
// (seg_start / seg_end and the low word of before / after), which the apply launch reads before it overwrites them.
//
// nnl_seg_rolling: one thread per (row, column) walks its window oldest -> newest in fp64: O(window) per output, exact for
// integer-valued columns, right for the notebook's '8D' windows of at most 8 rows (no prefix-sum path for long windows).
#include "nnl_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kItems = 4;
constexpr int kTile = NNL_SEG_SCAN_TILE;
constexpr int kWaves = kThreads / NNL_WAVE;
static_assert(kThreads * kItems == kTile, "tile = threads x rows per thread");

struct I2 { int a, b; };      // two maxima travel through one scan
__device__ __forceinline__ I2 i2_max(I2 x, I2 y) { return I2{max(x.a, y.a), max(x.b, y.b)}; }

// a, b: this thread's maxima.  On return a, b = the maxima over all threads BEFORE this one (-1 for thread 0), ta, tb = over the block.
__device__ __forceinline__ void block_excl_max2(int& a, int& b, int& ta, int& tb, I2* lds) {
  I2 total;
  const I2 e = nnl_block_scan_exclusive<kWaves>(I2{a, b}, i2_max, I2{-1, -1}, lds, total);
  a = e.a; b = e.b;
  ta = total.a; tb = total.b;
}

struct GapArgs {
  const int64_t* t;
  const uint8_t* head;
  const uint8_t* event;
  int64_t n;
  double timescale;
  double* gap[2];        // before, after
  int32_t* seg[2];       // seg_start, seg_end
};

__device__ __forceinline__ int64_t row_of(int64_t p, int64_t n, int rev) { return rev ? n - 1 - p : p; }
// group boundary in scan order: the group's first row forward, its last row backward
__device__ __forceinline__ bool boundary_at(const GapArgs& a, int64_t p, int rev) {
  return p == 0 || a.head[rev ? a.n - p : p] != 0;
}
__device__ __forceinline__ int32_t* carry_h(const GapArgs& a, int64_t tile, int rev) { return a.seg[rev] + row_of(tile * kTile, a.n, rev); }
__device__ __forceinline__ int32_t* carry_e(const GapArgs& a, int64_t tile, int rev) {
  return reinterpret_cast<int32_t*>(a.gap[rev] + row_of(tile * kTile, a.n, rev));
}

// this thread's kItems positions: hv[k] / ev[k] = p if the position is a boundary / an event, else -1 (also past the end)
__device__ __forceinline__ void load_items(const GapArgs& a, int64_t p0, int rev, int* hv, int* ev) {
#pragma unroll
  for (int k = 0; k < kItems; ++k) {
    const int64_t p = p0 + k;
    hv[k] = ev[k] = -1;
    if (p < a.n) {
      if (boundary_at(a, p, rev)) hv[k] = (int)p;
      if (a.event[row_of(p, a.n, rev)] == 1) ev[k] = (int)p;
    }
  }
}

__global__ __launch_bounds__(kThreads) void gaps_tile_max_kernel(GapArgs a) {
  __shared__ I2 lds[kWaves];
  const int rev = blockIdx.y;
  const int64_t tile = blockIdx.x;
  int hv[kItems], ev[kItems];
  load_items(a, tile * kTile + (int64_t)threadIdx.x * kItems, rev, hv, ev);
  int h = -1, e = -1, th, te;
#pragma unroll
  for (int k = 0; k < kItems; ++k) {
    h = max(h, hv[k]);
    e = max(e, ev[k]);
  }
  block_excl_max2(h, e, th, te, lds);
  if (threadIdx.x == 0) {
    *carry_h(a, tile, rev) = th;
    *carry_e(a, tile, rev) = te;
  }
}

// one workgroup per direction: tile maxima -> maxima over all EARLIER tiles, in place
__global__ __launch_bounds__(kThreads) void gaps_carry_scan_kernel(GapArgs a, int64_t ntiles) {
  __shared__ I2 lds[kWaves];
  const int rev = blockIdx.x;
  int run_h = -1, run_e = -1;
  for (int64_t c = 0; c < ntiles; c += kThreads) {
    const int64_t tile = c + threadIdx.x;
    int h = -1, e = -1, th, te;
    if (tile < ntiles) {
      h = *carry_h(a, tile, rev);
      e = *carry_e(a, tile, rev);
    }
    block_excl_max2(h, e, th, te, lds);
    if (tile < ntiles) {
      *carry_h(a, tile, rev) = max(run_h, h);
      *carry_e(a, tile, rev) = max(run_e, e);
    }
    run_h = max(run_h, th);
    run_e = max(run_e, te);
  }
}

__global__ __launch_bounds__(kThreads) void gaps_apply_kernel(GapArgs a) {
  __shared__ I2 lds[kWaves];
  __shared__ int carry[2];
  const int rev = blockIdx.y;
  const int64_t tile = blockIdx.x;
  if (threadIdx.x == 0) {       // read before any thread of this tile overwrites the slots
    carry[0] = *carry_h(a, tile, rev);
    carry[1] = *carry_e(a, tile, rev);
  }
  const int64_t p0 = tile * kTile + (int64_t)threadIdx.x * kItems;
  int hv[kItems], ev[kItems];
  load_items(a, p0, rev, hv, ev);
  int h = -1, e = -1, th, te;
#pragma unroll
  for (int k = 0; k < kItems; ++k) {
    h = max(h, hv[k]);
    e = max(e, ev[k]);
  }
  block_excl_max2(h, e, th, te, lds);      // its barriers also order the carry[] read above
  h = max(h, carry[0]);
  e = max(e, carry[1]);
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
#pragma unroll
  for (int k = 0; k < kItems; ++k) {
    const int64_t p = p0 + k;
    if (p >= a.n) break;
    h = max(h, hv[k]);                     // inclusive: p may open its own group
    const int64_t i = row_of(p, a.n, rev);
    a.seg[rev][i] = (int32_t)row_of(h, a.n, rev);
    double g = nan;
    if (e >= h && e >= 0) {                // the last event before p lies in p's group (p's own event does not count)
      const int64_t j = row_of(e, a.n, rev);
      const int64_t d = rev ? a.t[j] - a.t[i] : a.t[i] - a.t[j];
      g = (double)d / a.timescale;
    }
    a.gap[rev][i] = g;
    e = max(e, ev[k]);                     // exclusive: counts from the next position on
  }
}

constexpr int kAllStats = NNL_ROLL_SUM | NNL_ROLL_MIN | NNL_ROLL_MAX | NNL_ROLL_MEAN | NNL_ROLL_STD | NNL_ROLL_COUNT;

__global__ __launch_bounds__(kThreads) void seg_rolling_kernel(const int64_t* __restrict__ t, const int32_t* __restrict__ seg_start,
                                                               const int32_t* __restrict__ seg_end, const double* __restrict__ x,
                                                               int64_t n, int64_t count_window, int64_t span, int forward, int stat_mask,
                                                               double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int64_t C = gridDim.y, c = blockIdx.y;
  // the row's group, clamped into the arrays whatever the caller handed over
  const int64_t g0 = min(max((int64_t)seg_start[i], (int64_t)0), i), g1 = max(min((int64_t)seg_end[i], n - 1), i);
  int64_t lo = i, hi = i;
  if (count_window > 0) {
    if (forward) hi = (g1 - i >= count_window - 1) ? i + count_window - 1 : g1;
    else lo = (i - g0 >= count_window - 1) ? i - (count_window - 1) : g0;
  } else {
    const int64_t ti = t[i];
    if (forward) { while (hi < g1 && t[hi + 1] - ti < span) ++hi; }
    else { while (lo > g0 && ti - t[lo - 1] < span) --lo; }
  }
  const double* __restrict__ xc = x + c * n;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  double sum = 0.0, mn = nan, mx = nan;
  int64_t cnt = 0;
  for (int64_t j = lo; j <= hi; ++j) {
    const double v = xc[j];
    if (v != v) continue;
    sum += v;
    mn = (cnt == 0 || v < mn) ? v : mn;
    mx = (cnt == 0 || v > mx) ? v : mx;
    ++cnt;
  }
  const double mean = cnt > 0 ? sum / (double)cnt : nan;
  double sd = nan;
  if ((stat_mask & NNL_ROLL_STD) && cnt >= 2) {
    double ss = 0.0;
    for (int64_t j = lo; j <= hi; ++j) {
      const double v = xc[j];
      if (v != v) continue;
      const double d = v - mean;
      ss += d * d;
    }
    sd = sqrt(ss / (double)(cnt - 1));
  }
  double* __restrict__ o = out + c * n + i;
  const int64_t plane = C * n;
  if (stat_mask & NNL_ROLL_SUM) { *o = cnt > 0 ? sum : nan; o += plane; }
  if (stat_mask & NNL_ROLL_MIN) { *o = mn; o += plane; }
  if (stat_mask & NNL_ROLL_MAX) { *o = mx; o += plane; }
  if (stat_mask & NNL_ROLL_MEAN) { *o = mean; o += plane; }
  if (stat_mask & NNL_ROLL_STD) { *o = sd; o += plane; }
  if (stat_mask & NNL_ROLL_COUNT) { *o = (double)cnt; }
}

}  // namespace

extern "C" int nnl_seg_event_gaps(const int64_t* t, const uint8_t* head, const uint8_t* event, int64_t n, double timescale,
                                  double* before, double* after, int32_t* seg_start, int32_t* seg_end, void* stream) {
  NNL_CHECK_ARG(n >= 1 && n < ((int64_t)1 << 31), "seg_event_gaps: n must lie in [1, 2^31) (got %lld)", (long long)n);
  NNL_CHECK_ARG(t && head && event && before && after && seg_start && seg_end, "seg_event_gaps: null pointer");
  NNL_CHECK_ARG(timescale == timescale && timescale != 0.0, "seg_event_gaps: timescale must be a non-zero number");
  hipStream_t s = (hipStream_t)stream;
  GapArgs a{t, head, event, n, timescale, {before, after}, {seg_start, seg_end}};
  const int64_t ntiles = nnl_cdiv(n, kTile);
  // read t 8 + head 1 + event 1 (twice each: tile maxima and apply), written 2 x (8 + 4) per row
  NnlProfScope prof(NNL_PROF_TABULAR, s, (double)n * (2 * 2 + 2 * 8 + 2 * 12));
  NNL_ROUTE("seg_event_gaps:tiles@%lld", (long long)ntiles);
  hipLaunchKernelGGL(gaps_tile_max_kernel, dim3((unsigned)ntiles, 2), dim3(kThreads), 0, s, a);
  NNL_CHECK_LAUNCH();
  hipLaunchKernelGGL(gaps_carry_scan_kernel, dim3(2), dim3(kThreads), 0, s, a, ntiles);
  NNL_CHECK_LAUNCH();
  hipLaunchKernelGGL(gaps_apply_kernel, dim3((unsigned)ntiles, 2), dim3(kThreads), 0, s, a);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}

extern "C" int nnl_seg_rolling(const int64_t* t, const int32_t* seg_start, const int32_t* seg_end, const double* x, int64_t n, int64_t C,
                               int64_t count_window, int64_t span, int forward, int stat_mask, double* out, void* stream) {
  NNL_CHECK_ARG(n >= 1 && n < ((int64_t)1 << 31), "seg_rolling: n must lie in [1, 2^31) (got %lld)", (long long)n);
  NNL_CHECK_ARG(C >= 1 && C <= 65535, "seg_rolling: C must lie in [1, 65535] (got %lld)", (long long)C);
  NNL_CHECK_ARG((count_window > 0) != (span > 0) && count_window >= 0 && span >= 0,
                "seg_rolling: exactly one of count_window > 0 and span > 0 must be given (got %lld and %lld)", (long long)count_window,
                (long long)span);
  NNL_CHECK_ARG(stat_mask >= 1 && stat_mask <= kAllStats, "seg_rolling: stat_mask must lie in [1, 63] (got %d)", stat_mask);
  NNL_CHECK_ARG(forward == 0 || forward == 1, "seg_rolling: forward must be 0 or 1");
  NNL_CHECK_ARG(t && seg_start && seg_end && x && out, "seg_rolling: null pointer");
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_TABULAR, s, (double)n * (16 + 8.0 * C * (1 + __builtin_popcount(stat_mask))));
  NNL_ROUTE("seg_rolling:%s:%s", count_window > 0 ? "count" : "span", forward ? "fwd" : "bwd");
  hipLaunchKernelGGL(seg_rolling_kernel, dim3((unsigned)nnl_cdiv(n, kThreads), (unsigned)C), dim3(kThreads), 0, s, t, seg_start, seg_end, x,
                     n, count_window, span, forward, stat_mask, out);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}
