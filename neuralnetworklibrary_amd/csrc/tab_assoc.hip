// K13 — association measures of the structured-data EDA (Applications/StructuredData.py:235-428): every pair of a call in a few
// launches instead of one crosstab / groupby / four corr per pair.
//
// Common shape.  The pair lists, cardinalities and offsets are HOST arrays: an entry validates them, cuts the pair list into chunks
// that share at most a few columns and hands each chunk to its kernel BY VALUE (kernel arguments, about 1 KiB), so nothing is
// uploaded.  A workgroup owns a contiguous span of row tiles (NNL_ASSOC_ROW_TILE rows each).  Per tile it stages the chunk's columns
// in LDS once and walks the chunk's pairs over them: inside a chunk a column is read once, not once per pair.  No workgroup waits
// for another.
//
// nnl_assoc_contingency: uint32 counts.  A pair whose table has at most NNL_ASSOC_LDS_CELLS cells (together with the chunk's other
// such tables) is counted in a workgroup-private LDS table with LDS integer atomics and flushed once per workgroup (non-zero cells
// only); a larger table takes global integer atomics directly.  Integers: exact and independent of the order.
// nnl_assoc_table_stats: one workgroup per pair, fp64, fixed order (thread-strided partial sums, shuffle tree, waves in order).
// nnl_assoc_cat_cont: per category count, sum and sum of squares of y - shift with fp64 atomics (LDS per workgroup, then global):
// the ONE family whose last bits may differ between calls.  Min / max of y ride along as order-preserving integer keys (atomicMax).
// nnl_assoc_cont_cont: per-thread fp64 accumulators, reduced over the wave by shuffles and over a workgroup's tiles in one LDS slot
// per (pair, wave), stored as per-workgroup partials and summed by one workgroup per pair: no atomics, the same bits on every call.
#include "nnl_common.h"

#include <cmath>
#include <vector>

namespace {

constexpr int kThreads = 256;
constexpr int kTile = NNL_ASSOC_ROW_TILE;
constexpr int kWaves = kThreads / NNL_WAVE;
constexpr int kMaxGrid = NNL_ASSOC_MAX_GROUPS;       // workgroups per launch = partial slabs of the cont x cont sums
constexpr int64_t kMaxCells = (int64_t)1 << 26;      // per table (offsets are int64; a cell index fits an int)
static_assert(kMaxGrid <= kThreads, "the final sums read one partial slab per thread");

constexpr int kCntCols = 8, kCntPairs = 32, kCntLdsCells = NNL_ASSOC_LDS_CELLS;
constexpr int kMomCats = 4, kMomConts = 2, kMomPairs = 8, kMomLdsCells = NNL_ASSOC_MOMENT_LDS_CELLS;
constexpr int kCorCols = 4, kCorPairs = 16, kCorK = 14;
constexpr int kFinPairs = 64;

struct CntChunk {
  int ncols, npairs;
  int col[kCntCols];
  struct { int xi, yi, cx, cy, lds, pad; long long off; } pair[kCntPairs];      // lds: first cell in the LDS table, -1 = global route
};
struct MomChunk {
  int ncat, ncont, npairs, pad;
  int cat[kMomCats], cont[kMomConts];
  struct { int xi, yi, card, lds; long long off; } pair[kMomPairs];             // off: first double of the pair's accumulators
};
struct CorChunk {
  int ncols, npairs;
  int col[kCorCols];
  struct { int xi, yi, gp; } pair[kCorPairs];                                   // gp: the pair's index in the call
};
struct FinChunk {
  struct { int cx, cy; long long off; } pair[kFinPairs];
};

// local index of column v in cols[0..n), appended if absent; -1 if the list is full
inline int local_col(int* cols, int& n, int cap, int v) {
  for (int i = 0; i < n; ++i)
    if (cols[i] == v) return i;
  if (n == cap) return -1;
  cols[n] = v;
  return n++;
}

struct Span { int64_t groups, tiles_per_group; };
inline Span row_spans(int64_t n) {
  const int64_t tiles = nnl_cdiv(n, kTile), per = nnl_cdiv(tiles, kMaxGrid);
  return {nnl_cdiv(tiles, per), per};              // every group owns at least one tile
}

// doubles (no NaN) as unsigned keys of the same order; 0 is below every key: "nothing seen"
__device__ __forceinline__ unsigned long long key_of(double d) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(d);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
}
__device__ __forceinline__ double double_of(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffULL) : ~k));
}

// ---- 1. contingency counts -------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void contingency_kernel(const int32_t* __restrict__ codes, int64_t n, int64_t tiles_per_group,
                                                               CntChunk c, int lds_cells, uint32_t* __restrict__ tables) {
  __shared__ int32_t stage[kCntCols][kTile];
  __shared__ uint32_t tab[kCntLdsCells];
  for (int i = threadIdx.x; i < lds_cells; i += kThreads) tab[i] = 0u;
  const int64_t tile0 = (int64_t)blockIdx.x * tiles_per_group;
  for (int64_t t = tile0; t < tile0 + tiles_per_group; ++t) {
    const int64_t r0 = t * kTile;
    if (r0 >= n) break;
    __syncthreads();                       // the table is zeroed / the last tile is read
    for (int k = 0; k < c.ncols; ++k) {
      const int32_t* __restrict__ src = codes + (int64_t)c.col[k] * n;
      for (int i = threadIdx.x; i < kTile; i += kThreads) stage[k][i] = r0 + i < n ? src[r0 + i] : -1;
    }
    __syncthreads();
    for (int p = 0; p < c.npairs; ++p) {
      const int xi = c.pair[p].xi, yi = c.pair[p].yi, cy = c.pair[p].cy, lds = c.pair[p].lds;
      const unsigned ucx = (unsigned)c.pair[p].cx, ucy = (unsigned)cy;
      uint32_t* __restrict__ g = tables + c.pair[p].off;
      for (int i = threadIdx.x; i < kTile; i += kThreads) {
        const int a = stage[xi][i], b = stage[yi][i];
        if ((unsigned)a < ucx && (unsigned)b < ucy) {      // a missing (-1) or out-of-range code counts nowhere
          const int cell = a * cy + b;
          if (lds >= 0) atomicAdd(&tab[lds + cell], 1u);
          else atomicAdd(&g[cell], 1u);
        }
      }
    }
  }
  __syncthreads();
  for (int p = 0; p < c.npairs; ++p) {
    const int lds = c.pair[p].lds;
    if (lds < 0) continue;
    const int cells = c.pair[p].cx * c.pair[p].cy;
    uint32_t* __restrict__ g = tables + c.pair[p].off;
    for (int i = threadIdx.x; i < cells; i += kThreads) {
      const uint32_t v = tab[lds + i];
      if (v) atomicAdd(&g[i], v);
    }
  }
}

// ---- 2. table -> n, non-empty rows / columns, H_X, H_Y, H_XY ---------------------------------------------------------

__global__ __launch_bounds__(kThreads) void table_stats_kernel(const uint32_t* __restrict__ tables, FinChunk c, double* __restrict__ out) {
  __shared__ double lds[kWaves];
  const int cx = c.pair[blockIdx.x].cx, cy = c.pair[blockIdx.x].cy;
  const uint32_t* __restrict__ T = tables + c.pair[blockIdx.x].off;
  double* __restrict__ o = out + (int64_t)blockIdx.x * 6;
  const int cells = cx * cy;
  double s = 0.0;
  for (int i = threadIdx.x; i < cells; i += kThreads) s += (double)T[i];
  const double N = nnl_block_reduce<kWaves>(s, NnlSum(), lds);
  if (N == 0.0) {
    if (threadIdx.x < 6) o[threadIdx.x] = 0.0;
    return;
  }
  double h = 0.0, nz = 0.0;
  for (int i = threadIdx.x; i < cells; i += kThreads) {
    const uint32_t v = T[i];
    if (v) {
      const double p = (double)v / N;
      h -= log(p) * p;
      nz += 1.0;
    }
  }
  double hxy = nnl_block_reduce<kWaves>(h, NnlSum(), lds);
  const double cells_seen = nnl_block_reduce<kWaves>(nz, NnlSum(), lds);
  double hx = 0.0, rows = 0.0;
  for (int r = threadIdx.x; r < cx; r += kThreads) {
    double m = 0.0;
    for (int j = 0; j < cy; ++j) m += (double)T[r * cy + j];
    if (m > 0.0) {
      const double p = m / N;
      hx -= log(p) * p;
      rows += 1.0;
    }
  }
  hx = nnl_block_reduce<kWaves>(hx, NnlSum(), lds);
  rows = nnl_block_reduce<kWaves>(rows, NnlSum(), lds);
  double hy = 0.0, cols = 0.0;
  for (int j = threadIdx.x; j < cy; j += kThreads) {
    double m = 0.0;
    for (int r = 0; r < cx; ++r) m += (double)T[r * cy + j];
    if (m > 0.0) {
      const double p = m / N;
      hy -= log(p) * p;
      cols += 1.0;
    }
  }
  hy = nnl_block_reduce<kWaves>(hy, NnlSum(), lds);
  cols = nnl_block_reduce<kWaves>(cols, NnlSum(), lds);
  // the reference clamps every cell of the observed x observed table at 1e-20: each empty one adds -1e-20 log(1e-20)
  hxy += (rows * cols - cells_seen) * (-(1e-20 * log(1e-20)));
  if (threadIdx.x == 0) {
    o[0] = N; o[1] = rows; o[2] = cols; o[3] = hx; o[4] = hy; o[5] = hxy;
  }
}

// ---- 3. categorical x continuous moments -----------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void cat_cont_kernel(const int32_t* __restrict__ codes, const double* __restrict__ vals,
                                                            const double* __restrict__ shift, int64_t n, int64_t tiles_per_group,
                                                            MomChunk c, int lds_cells, double* __restrict__ ws) {
  __shared__ int32_t stage_c[kMomCats][kTile];
  __shared__ double stage_y[kMomConts][kTile];
  __shared__ double acc[kMomLdsCells * 3];
  __shared__ double mm[kMomPairs][kWaves][2];
  const int lane = threadIdx.x & (NNL_WAVE - 1), w = threadIdx.x / NNL_WAVE;
  const double inf = __longlong_as_double(0x7ff0000000000000LL), nan = __longlong_as_double(0x7ff8000000000000LL);
  for (int i = threadIdx.x; i < lds_cells * 3; i += kThreads) acc[i] = 0.0;
  if (threadIdx.x < kMomPairs * kWaves) {
    mm[threadIdx.x / kWaves][threadIdx.x % kWaves][0] = inf;
    mm[threadIdx.x / kWaves][threadIdx.x % kWaves][1] = -inf;
  }
  const int64_t tile0 = (int64_t)blockIdx.x * tiles_per_group;
  for (int64_t t = tile0; t < tile0 + tiles_per_group; ++t) {
    const int64_t r0 = t * kTile;
    if (r0 >= n) break;
    __syncthreads();
    for (int k = 0; k < c.ncat; ++k) {
      const int32_t* __restrict__ src = codes + (int64_t)c.cat[k] * n;
      for (int i = threadIdx.x; i < kTile; i += kThreads) stage_c[k][i] = r0 + i < n ? src[r0 + i] : -1;
    }
    for (int k = 0; k < c.ncont; ++k) {
      const double* __restrict__ src = vals + (int64_t)c.cont[k] * n;
      const double s = shift[c.cont[k]];
      for (int i = threadIdx.x; i < kTile; i += kThreads) stage_y[k][i] = r0 + i < n ? src[r0 + i] - s : nan;
    }
    __syncthreads();
    for (int p = 0; p < c.npairs; ++p) {
      const int xi = c.pair[p].xi, yi = c.pair[p].yi, lds = c.pair[p].lds;
      const unsigned card = (unsigned)c.pair[p].card;
      double* __restrict__ g = ws + c.pair[p].off;
      double mn = inf, mx = -inf;
      for (int i = threadIdx.x; i < kTile; i += kThreads) {
        const int a = stage_c[xi][i];
        const double d = stage_y[yi][i];
        if ((unsigned)a < card && d == d) {
          if (lds >= 0) {                  // two branches: the compiler knows the address space of each
            double* cell = acc + (lds + a) * 3;
            atomicAdd(cell, 1.0);
            atomicAdd(cell + 1, d);
            atomicAdd(cell + 2, d * d);
          } else {
            double* cell = g + (int64_t)a * 3;
            atomicAdd(cell, 1.0);
            atomicAdd(cell + 1, d);
            atomicAdd(cell + 2, d * d);
          }
          mn = fmin(mn, d);
          mx = fmax(mx, d);
        }
      }
      mn = nnl_wave_min(mn);
      mx = nnl_wave_max(mx);
      if (lane == 0) {                     // this wave's own slot: no other wave touches it
        mm[p][w][0] = fmin(mm[p][w][0], mn);
        mm[p][w][1] = fmax(mm[p][w][1], mx);
      }
    }
  }
  __syncthreads();
  for (int p = 0; p < c.npairs; ++p) {
    const int lds = c.pair[p].lds, card = c.pair[p].card;
    double* __restrict__ g = ws + c.pair[p].off;
    if (lds >= 0) {
      for (int i = threadIdx.x; i < card * 3; i += kThreads) {
        const double v = acc[lds * 3 + i];
        if (v != 0.0) atomicAdd(&g[i], v);
      }
    }
    if (threadIdx.x == 0) {
      double mn = mm[p][0][0], mx = mm[p][0][1];
      for (int k = 1; k < kWaves; ++k) {
        mn = fmin(mn, mm[p][k][0]);
        mx = fmax(mx, mm[p][k][1]);
      }
      if (mn <= mx) {                      // shifted values; min is kept as the max of the negated value
        unsigned long long* keys = reinterpret_cast<unsigned long long*>(g + (int64_t)card * 3);
        atomicMax(&keys[0], key_of(-mn));
        atomicMax(&keys[1], key_of(mx));
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void cat_cont_final_kernel(const double* __restrict__ ws, FinChunk c, double* __restrict__ out) {
  __shared__ double lds[kWaves];
  const int card = c.pair[blockIdx.x].cx;
  const double* __restrict__ g = ws + c.pair[blockIdx.x].off;
  double* __restrict__ o = out + (int64_t)blockIdx.x * 6;
  double a = 0.0, b = 0.0, q = 0.0, ne = 0.0;
  for (int k = threadIdx.x; k < card; k += kThreads) {
    a += g[k * 3];
    b += g[k * 3 + 1];
    q += g[k * 3 + 2];
    ne += g[k * 3] > 0.0 ? 1.0 : 0.0;
  }
  const double N = nnl_block_reduce<kWaves>(a, NnlSum(), lds), S1 = nnl_block_reduce<kWaves>(b, NnlSum(), lds), S2 = nnl_block_reduce<kWaves>(q, NnlSum(), lds);
  ne = nnl_block_reduce<kWaves>(ne, NnlSum(), lds);
  if (N == 0.0) {
    if (threadIdx.x < 6) o[threadIdx.x] = 0.0;
    return;
  }
  const double mean = S1 / N, var = (S2 - S1 * S1 / N) / (N - 1.0);     // about the shift; ddof = 1
  double between = 0.0, dev = 0.0;
  for (int k = threadIdx.x; k < card; k += kThreads) {
    const double cnt = g[k * 3];
    if (cnt > 0.0) {
      const double d = g[k * 3 + 1] / cnt - mean;
      between += cnt * (d * d);
      dev = fmax(dev, fabs(d));
    }
  }
  between = nnl_block_reduce<kWaves>(between, NnlSum(), lds);
  dev = nnl_block_reduce<kWaves>(dev, NnlMax(), lds);
  if (threadIdx.x == 0) {
    const unsigned long long* keys = reinterpret_cast<const unsigned long long*>(g + (int64_t)card * 3);
    o[0] = N;
    o[1] = ne;
    o[2] = sqrt((between / N) / var);
    o[3] = dev / sqrt(var);
    o[4] = -double_of(keys[0]);
    o[5] = double_of(keys[1]);
  }
}

// ---- 4. continuous x continuous moments ------------------------------------------------------------------------------
// pass 1 (about the column shifts): 0 n, 1 Sx, 2 Sy, 3 Sxx, 4 Syy, 5 Sxy, 6 min x, 7 max x, 8 min y, 9 max y; the final sum adds
//   10 sx, 11 sy: the standard deviations of x and y over the pair's rows.
// pass 2 (about the pair's means), with a = |dx| - sx and b = |dy| - sy:
//   0 n, 1 Sdx, 2 Sdy, 3 Sdx2, 4 Sdy2, 5 Sdxdy, 6 Sa, 7 Sb, 8 Sa dy, 9 Sdx b, 10 Sab, 11 Saa, 12 Sbb.
// Why a and not |dx|: the centred sum of squares of |dx| from S|dx|^2 and S dx^2 would cancel badly when |dx| is nearly constant (a
// nearly balanced +-1 column).  mean|dx| <= sx always, and var|dx| = (sx - mean|dx|)(sx + mean|dx|), so about sx the squared mean
// of a is at most var(a): Saa - Sa^2/n loses at most one bit, whatever the data.

template <int PASS>
__global__ __launch_bounds__(kThreads) void cont_cont_kernel(const double* __restrict__ vals, const double* __restrict__ shift, int64_t n,
                                                             int64_t tiles_per_group, CorChunk c, int64_t P,
                                                             const double* __restrict__ stats1, double* __restrict__ part) {
  __shared__ double stage[kCorCols][kTile];
  __shared__ double acc[kCorPairs][kWaves][kCorK];
  const int lane = threadIdx.x & (NNL_WAVE - 1), w = threadIdx.x / NNL_WAVE;
  const double inf = __longlong_as_double(0x7ff0000000000000LL), nan = __longlong_as_double(0x7ff8000000000000LL);
  for (int i = threadIdx.x; i < kCorPairs * kWaves * kCorK; i += kThreads) {
    const int k = i % kCorK;
    (&acc[0][0][0])[i] = (PASS == 1 && (k == 6 || k == 8)) ? inf : (PASS == 1 && (k == 7 || k == 9)) ? -inf : 0.0;
  }
  const int64_t tile0 = (int64_t)blockIdx.x * tiles_per_group;
  for (int64_t t = tile0; t < tile0 + tiles_per_group; ++t) {
    const int64_t r0 = t * kTile;
    if (r0 >= n) break;
    __syncthreads();
    for (int k = 0; k < c.ncols; ++k) {
      const double* __restrict__ src = vals + (int64_t)c.col[k] * n;
      const double s = shift[c.col[k]];
      for (int i = threadIdx.x; i < kTile; i += kThreads) stage[k][i] = r0 + i < n ? src[r0 + i] - s : nan;
    }
    __syncthreads();
    for (int p = 0; p < c.npairs; ++p) {
      const int xi = c.pair[p].xi, yi = c.pair[p].yi;
      double v[kCorK];
#pragma unroll
      for (int k = 0; k < kCorK; ++k) v[k] = 0.0;
      double mx0 = 0.0, my0 = 0.0, sx0 = 0.0, sy0 = 0.0;
      if (PASS == 1) {
        v[6] = v[8] = inf;
        v[7] = v[9] = -inf;
      } else {
        const double* __restrict__ s1 = stats1 + (int64_t)c.pair[p].gp * kCorK;
        mx0 = s1[1] / s1[0];               // the pair's mean of x minus the column's shift
        my0 = s1[2] / s1[0];
        sx0 = s1[10];
        sy0 = s1[11];
      }
      for (int i = threadIdx.x; i < kTile; i += kThreads) {
        const double x = stage[xi][i], y = stage[yi][i];
        if (x == x && y == y) {
          v[0] += 1.0;
          if (PASS == 1) {
            v[1] += x; v[2] += y; v[3] += x * x; v[4] += y * y; v[5] += x * y;
            v[6] = fmin(v[6], x); v[7] = fmax(v[7], x); v[8] = fmin(v[8], y); v[9] = fmax(v[9], y);
          } else {
            const double dx = x - mx0, dy = y - my0, ax = fabs(dx) - sx0, ay = fabs(dy) - sy0;
            v[1] += dx; v[2] += dy; v[3] += dx * dx; v[4] += dy * dy; v[5] += dx * dy;
            v[6] += ax; v[7] += ay; v[8] += ax * dy; v[9] += dx * ay; v[10] += ax * ay; v[11] += ax * ax; v[12] += ay * ay;
          }
        }
      }
#pragma unroll
      for (int k = 0; k < kCorK; ++k) {
        if (PASS == 1 && (k == 6 || k == 8)) v[k] = nnl_wave_min(v[k]);
        else if (PASS == 1 && (k == 7 || k == 9)) v[k] = nnl_wave_max(v[k]);
        else if (k <= (PASS == 1 ? 5 : 12)) v[k] = nnl_wave_sum(v[k]);
      }
      if (lane == 0) {                     // this wave's own slots, tile after tile: a fixed order
#pragma unroll
        for (int k = 0; k < kCorK; ++k) {
          if (PASS == 1 && (k == 6 || k == 8)) acc[p][w][k] = fmin(acc[p][w][k], v[k]);
          else if (PASS == 1 && (k == 7 || k == 9)) acc[p][w][k] = fmax(acc[p][w][k], v[k]);
          else acc[p][w][k] += v[k];
        }
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < c.npairs * kCorK; i += kThreads) {
    const int p = i / kCorK, k = i % kCorK;
    double r = acc[p][0][k];
    for (int u = 1; u < kWaves; ++u) {
      if (PASS == 1 && (k == 6 || k == 8)) r = fmin(r, acc[p][u][k]);
      else if (PASS == 1 && (k == 7 || k == 9)) r = fmax(r, acc[p][u][k]);
      else r += acc[p][u][k];
    }
    part[((int64_t)blockIdx.x * P + c.pair[p].gp) * kCorK + k] = r;
  }
}

// one workgroup per pair: the partial slabs in order -> stats (pass 1) and the correlations.  out [P, 4]: n, degenerate, |c1|, abs max
template <int PASS>
__global__ __launch_bounds__(kThreads) void cont_cont_final_kernel(const double* __restrict__ part, int64_t groups, int64_t P,
                                                                   double* __restrict__ stats1, double* __restrict__ out) {
  __shared__ double lds[kWaves];
  const int64_t gp = blockIdx.x;
  const double inf = __longlong_as_double(0x7ff0000000000000LL), nan = __longlong_as_double(0x7ff8000000000000LL);
  const bool mine = (int64_t)threadIdx.x < groups;
  const double* __restrict__ src = part + ((int64_t)threadIdx.x * P + gp) * kCorK;
  double S[kCorK];
#pragma unroll
  for (int k = 0; k < kCorK; ++k) {
    if (PASS == 1 && (k == 6 || k == 8)) S[k] = -nnl_block_reduce<kWaves>(mine ? -src[k] : -inf, NnlMax(), lds);
    else if (PASS == 1 && (k == 7 || k == 9)) S[k] = nnl_block_reduce<kWaves>(mine ? src[k] : -inf, NnlMax(), lds);
    else S[k] = nnl_block_reduce<kWaves>(mine ? src[k] : 0.0, NnlSum(), lds);
  }
  if (threadIdx.x != 0) return;
  double* __restrict__ o = out + gp * 4;
  const double N = S[0];
  if (PASS == 1) {
    const bool degenerate = N == 0.0 || S[6] == S[7] || S[8] == S[9];
    const double cxx = S[3] - S[1] * S[1] / N, cyy = S[4] - S[2] * S[2] / N, cxy = S[5] - S[1] * S[2] / N;
    S[10] = degenerate ? 0.0 : sqrt(cxx / N);
    S[11] = degenerate ? 0.0 : sqrt(cyy / N);
    for (int k = 0; k < kCorK; ++k) stats1[gp * kCorK + k] = S[k];
    o[0] = N;
    o[1] = degenerate ? 1.0 : 0.0;
    o[2] = degenerate ? nan : fabs(cxy / sqrt(cxx * cyy));
    o[3] = nan;
  } else {
    if (o[1] != 0.0) return;
    const double cxx = S[3] - S[1] * S[1] / N, cyy = S[4] - S[2] * S[2] / N;
    const double caa = S[11] - S[6] * S[6] / N, cbb = S[12] - S[7] * S[7] / N;
    const double tiny = 1.4901161193847656e-08;                                       // 2^-26
    const double ma = stats1[gp * kCorK + 10] + S[6] / N, mb = stats1[gp * kCorK + 11] + S[7] / N;      // mean|dx|, mean|dy|
    const bool const_a = !(caa > N * ((tiny * ma) * (tiny * ma))), const_b = !(cbb > N * ((tiny * mb) * (tiny * mb)));
    double r = fabs((S[5] - S[1] * S[2] / N) / sqrt(cxx * cyy));
    if (!const_b) r = fmax(r, fabs((S[9] - S[1] * S[7] / N) / sqrt(cxx * cbb)));
    if (!const_a) r = fmax(r, fabs((S[8] - S[6] * S[2] / N) / sqrt(caa * cyy)));
    if (!const_a && !const_b) r = fmax(r, fabs((S[10] - S[6] * S[7] / N) / sqrt(caa * cbb)));
    o[3] = r;
  }
}

bool pairs_in_range(const int32_t* px, const int32_t* py, int64_t P, int64_t Vx, int64_t Vy) {
  for (int64_t p = 0; p < P; ++p)
    if (px[p] < 0 || px[p] >= Vx || py[p] < 0 || py[p] >= Vy) return false;
  return true;
}

}  // namespace

extern "C" int nnl_assoc_contingency(const int32_t* codes, const int32_t* card, int64_t V, int64_t n, const int32_t* pair_x,
                                     const int32_t* pair_y, const int64_t* offsets, int64_t P, uint32_t* tables, void* stream) {
  NNL_CHECK_ARG(codes && card && pair_x && pair_y && offsets && tables, "assoc_contingency: null pointer");
  NNL_CHECK_ARG(n >= 1 && n < ((int64_t)1 << 31), "assoc_contingency: n must lie in [1, 2^31) (got %lld)", (long long)n);
  NNL_CHECK_ARG(V >= 1 && P >= 1, "assoc_contingency: V and P must be at least 1 (got %lld, %lld)", (long long)V, (long long)P);
  NNL_CHECK_ARG(pairs_in_range(pair_x, pair_y, P, V, V), "assoc_contingency: a pair names a column outside [0, %lld)", (long long)V);
  for (int64_t v = 0; v < V; ++v) NNL_CHECK_ARG(card[v] >= 1, "assoc_contingency: cardinality %lld is below 1", (long long)v);
  NNL_CHECK_ARG(offsets[0] == 0, "assoc_contingency: offsets[0] must be 0");
  for (int64_t p = 0; p < P; ++p) {
    const int64_t cells = (int64_t)card[pair_x[p]] * card[pair_y[p]];
    NNL_CHECK_ARG(cells <= kMaxCells, "assoc_contingency: the table of pair %lld has %lld cells, above %lld", (long long)p,
                  (long long)cells, (long long)kMaxCells);
    NNL_CHECK_ARG(offsets[p + 1] - offsets[p] == cells, "assoc_contingency: offsets of pair %lld do not match its cardinalities",
                  (long long)p);
  }
  hipStream_t s = (hipStream_t)stream;
  const Span sp = row_spans(n);
  NnlProfScope prof(NNL_PROF_TABULAR, s, 4.0 * (double)n * (double)V + 4.0 * (double)offsets[P]);
  NNL_CHECK_HIP(hipMemsetAsync(tables, 0, sizeof(uint32_t) * (size_t)offsets[P], s));
  int n_lds = 0, n_global = 0, n_chunks = 0;
  int64_t p = 0;
  while (p < P) {
    CntChunk c{};
    int lds_cells = 0;
    while (p < P && c.npairs < kCntPairs) {
      const int saved = c.ncols;
      const int xi = local_col(c.col, c.ncols, kCntCols, pair_x[p]);
      const int yi = xi < 0 ? -1 : local_col(c.col, c.ncols, kCntCols, pair_y[p]);
      const int cx = card[pair_x[p]], cy = card[pair_y[p]];
      const int64_t cells = (int64_t)cx * cy;
      const bool fits = cells <= kCntLdsCells;
      if (yi < 0 || (fits && lds_cells + cells > kCntLdsCells && c.npairs > 0)) {
        c.ncols = saved;
        break;                             // the chunk is full: this pair opens the next one
      }
      auto& q = c.pair[c.npairs++];
      q.xi = xi; q.yi = yi; q.cx = cx; q.cy = cy; q.off = offsets[p];
      q.lds = fits ? lds_cells : -1;
      if (fits) { lds_cells += (int)cells; ++n_lds; } else ++n_global;
      ++p;
    }
    ++n_chunks;
    hipLaunchKernelGGL(contingency_kernel, dim3((unsigned)sp.groups), dim3(kThreads), 0, s, codes, n, sp.tiles_per_group, c, lds_cells,
                       tables);
    NNL_CHECK_LAUNCH();
  }
  NNL_ROUTE("assoc_contingency:lds=%d,global=%d,chunks=%d", n_lds, n_global, n_chunks);
  return NNL_OK;
}

extern "C" int nnl_assoc_table_stats(const uint32_t* tables, const int32_t* card, int64_t V, const int32_t* pair_x, const int32_t* pair_y,
                                     const int64_t* offsets, int64_t P, double* out, void* stream) {
  NNL_CHECK_ARG(tables && card && pair_x && pair_y && offsets && out, "assoc_table_stats: null pointer");
  NNL_CHECK_ARG(V >= 1 && P >= 1, "assoc_table_stats: V and P must be at least 1 (got %lld, %lld)", (long long)V, (long long)P);
  NNL_CHECK_ARG(pairs_in_range(pair_x, pair_y, P, V, V), "assoc_table_stats: a pair names a column outside [0, %lld)", (long long)V);
  for (int64_t p = 0; p < P; ++p) {
    const int64_t cx = card[pair_x[p]], cy = card[pair_y[p]];
    NNL_CHECK_ARG(cx >= 1 && cy >= 1 && cx * cy <= kMaxCells && offsets[p] >= 0 && offsets[p + 1] - offsets[p] == cx * cy,
                  "assoc_table_stats: offsets of pair %lld do not match its cardinalities", (long long)p);
  }
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_TABULAR, s, 3.0 * 4.0 * (double)(offsets[P] - offsets[0]));
  for (int64_t p0 = 0; p0 < P; p0 += kFinPairs) {
    FinChunk c{};
    const int m = (int)std::min<int64_t>(kFinPairs, P - p0);
    for (int k = 0; k < m; ++k) c.pair[k] = {card[pair_x[p0 + k]], card[pair_y[p0 + k]], offsets[p0 + k]};
    hipLaunchKernelGGL(table_stats_kernel, dim3(m), dim3(kThreads), 0, s, tables, c, out + p0 * 6);
    NNL_CHECK_LAUNCH();
  }
  return NNL_OK;
}

extern "C" size_t nnl_assoc_cat_cont_workspace_bytes(const int32_t* card, int64_t Vc, const int32_t* pair_x, int64_t P) {
  if (!card || !pair_x || Vc < 1 || P < 1) return 0;
  size_t doubles = 0;
  for (int64_t p = 0; p < P; ++p) {
    if (pair_x[p] < 0 || pair_x[p] >= Vc || card[pair_x[p]] < 1) return 0;
    doubles += (size_t)card[pair_x[p]] * 3 + 2;
  }
  return doubles * sizeof(double);
}

extern "C" int nnl_assoc_cat_cont(const int32_t* codes, const int32_t* card, int64_t Vc, const double* vals, const double* shift,
                                  int64_t Vy, int64_t n, const int32_t* pair_x, const int32_t* pair_y, int64_t P, void* workspace,
                                  size_t workspace_bytes, double* out, void* stream) {
  NNL_CHECK_ARG(codes && card && vals && shift && pair_x && pair_y && workspace && out, "assoc_cat_cont: null pointer");
  NNL_CHECK_ARG(n >= 1 && n < ((int64_t)1 << 31), "assoc_cat_cont: n must lie in [1, 2^31) (got %lld)", (long long)n);
  NNL_CHECK_ARG(Vc >= 1 && Vy >= 1 && P >= 1, "assoc_cat_cont: Vc, Vy and P must be at least 1 (got %lld, %lld, %lld)", (long long)Vc,
                (long long)Vy, (long long)P);
  NNL_CHECK_ARG(pairs_in_range(pair_x, pair_y, P, Vc, Vy), "assoc_cat_cont: a pair names a column outside [0, %lld) x [0, %lld)",
                (long long)Vc, (long long)Vy);
  for (int64_t v = 0; v < Vc; ++v)
    NNL_CHECK_ARG(card[v] >= 1 && card[v] <= kMaxCells, "assoc_cat_cont: cardinality %lld must lie in [1, %lld]", (long long)v,
                  (long long)kMaxCells);
  const size_t need = nnl_assoc_cat_cont_workspace_bytes(card, Vc, pair_x, P);
  NNL_CHECK_ARG(workspace_bytes >= need, "assoc_cat_cont: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  hipStream_t s = (hipStream_t)stream;
  const Span sp = row_spans(n);
  double* ws = static_cast<double*>(workspace);
  NnlProfScope prof(NNL_PROF_TABULAR, s, (double)n * (4.0 * (double)Vc + 8.0 * (double)Vy) + (double)need);
  NNL_CHECK_HIP(hipMemsetAsync(ws, 0, need, s));
  std::vector<int64_t> off((size_t)P);
  int64_t run = 0;
  for (int64_t p = 0; p < P; ++p) {
    off[(size_t)p] = run;
    run += (int64_t)card[pair_x[p]] * 3 + 2;
  }
  int n_lds = 0, n_global = 0, n_chunks = 0;
  int64_t p = 0;
  while (p < P) {
    MomChunk c{};
    int lds_cells = 0;
    while (p < P && c.npairs < kMomPairs) {
      const int saved_c = c.ncat, saved_y = c.ncont;
      const int xi = local_col(c.cat, c.ncat, kMomCats, pair_x[p]);
      const int yi = local_col(c.cont, c.ncont, kMomConts, pair_y[p]);
      const int cd = card[pair_x[p]];
      const bool fits = cd <= kMomLdsCells;
      if (xi < 0 || yi < 0 || (fits && lds_cells + cd > kMomLdsCells && c.npairs > 0)) {
        c.ncat = saved_c;
        c.ncont = saved_y;
        break;
      }
      auto& q = c.pair[c.npairs++];
      q.xi = xi; q.yi = yi; q.card = cd; q.off = off[(size_t)p];
      q.lds = fits ? lds_cells : -1;
      if (fits) { lds_cells += cd; ++n_lds; } else ++n_global;
      ++p;
    }
    ++n_chunks;
    hipLaunchKernelGGL(cat_cont_kernel, dim3((unsigned)sp.groups), dim3(kThreads), 0, s, codes, vals, shift, n, sp.tiles_per_group, c,
                       lds_cells, ws);
    NNL_CHECK_LAUNCH();
  }
  for (int64_t p0 = 0; p0 < P; p0 += kFinPairs) {
    FinChunk c{};
    const int m = (int)std::min<int64_t>(kFinPairs, P - p0);
    for (int k = 0; k < m; ++k) c.pair[k] = {card[pair_x[p0 + k]], 1, off[(size_t)(p0 + k)]};
    hipLaunchKernelGGL(cat_cont_final_kernel, dim3(m), dim3(kThreads), 0, s, ws, c, out + p0 * 6);
    NNL_CHECK_LAUNCH();
  }
  NNL_ROUTE("assoc_cat_cont:lds=%d,global=%d,chunks=%d", n_lds, n_global, n_chunks);
  return NNL_OK;
}

extern "C" size_t nnl_assoc_cont_cont_workspace_bytes(int64_t n, int64_t P) {
  if (n < 1 || P < 1) return 0;
  return (size_t)(row_spans(n).groups + 1) * (size_t)P * kCorK * sizeof(double);
}

extern "C" int nnl_assoc_cont_cont(const double* vals, const double* shift, int64_t V, int64_t n, const int32_t* pair_x,
                                   const int32_t* pair_y, int64_t P, int with_abs, void* workspace, size_t workspace_bytes, double* out,
                                   void* stream) {
  NNL_CHECK_ARG(vals && shift && pair_x && pair_y && workspace && out, "assoc_cont_cont: null pointer");
  NNL_CHECK_ARG(n >= 1 && n < ((int64_t)1 << 31), "assoc_cont_cont: n must lie in [1, 2^31) (got %lld)", (long long)n);
  NNL_CHECK_ARG(V >= 1 && P >= 1, "assoc_cont_cont: V and P must be at least 1 (got %lld, %lld)", (long long)V, (long long)P);
  NNL_CHECK_ARG(with_abs == 0 || with_abs == 1, "assoc_cont_cont: with_abs must be 0 or 1");
  NNL_CHECK_ARG(pairs_in_range(pair_x, pair_y, P, V, V), "assoc_cont_cont: a pair names a column outside [0, %lld)", (long long)V);
  const size_t need = nnl_assoc_cont_cont_workspace_bytes(n, P);
  NNL_CHECK_ARG(workspace_bytes >= need, "assoc_cont_cont: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  hipStream_t s = (hipStream_t)stream;
  const Span sp = row_spans(n);
  double* part = static_cast<double*>(workspace);
  double* stats1 = part + sp.groups * P * kCorK;
  std::vector<CorChunk> chunks;
  int64_t p = 0;
  while (p < P) {
    CorChunk c{};
    while (p < P && c.npairs < kCorPairs) {
      const int saved = c.ncols;
      const int xi = local_col(c.col, c.ncols, kCorCols, pair_x[p]);
      const int yi = xi < 0 ? -1 : local_col(c.col, c.ncols, kCorCols, pair_y[p]);
      if (yi < 0) {
        c.ncols = saved;
        break;
      }
      auto& q = c.pair[c.npairs++];
      q.xi = xi; q.yi = yi; q.gp = (int)p;
      ++p;
    }
    chunks.push_back(c);
  }
  NnlProfScope prof(NNL_PROF_TABULAR, s, 8.0 * (double)n * (double)V * (with_abs ? 2.0 : 1.0));
  for (const CorChunk& c : chunks) {
    hipLaunchKernelGGL(cont_cont_kernel<1>, dim3((unsigned)sp.groups), dim3(kThreads), 0, s, vals, shift, n, sp.tiles_per_group, c, P,
                       (const double*)stats1, part);
    NNL_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(cont_cont_final_kernel<1>, dim3((unsigned)P), dim3(kThreads), 0, s, (const double*)part, sp.groups, P, stats1, out);
  NNL_CHECK_LAUNCH();
  if (with_abs) {
    for (const CorChunk& c : chunks) {
      hipLaunchKernelGGL(cont_cont_kernel<2>, dim3((unsigned)sp.groups), dim3(kThreads), 0, s, vals, shift, n, sp.tiles_per_group, c, P,
                         (const double*)stats1, part);
      NNL_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(cont_cont_final_kernel<2>, dim3((unsigned)P), dim3(kThreads), 0, s, (const double*)part, sp.groups, P, stats1, out);
    NNL_CHECK_LAUNCH();
  }
  NNL_ROUTE("assoc_cont_cont:%s,chunks=%d,groups=%lld", with_abs ? "two-pass" : "one-pass", (int)chunks.size(), (long long)sp.groups);
  return NNL_OK;
}
