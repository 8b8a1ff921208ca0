// K19 line convolution: nn.Conv2d(C, K, (1, T) | (T, 1), stride 1, padding (0, T/2) | (T/2, 0)), the factorised convolutions of
// InceptionV4 (reference Applications/VisionModels/inceptionv4.py:114-115, 201-210, 239-240, 262-269).  NHWC fp32, T in {3, 5, 7},
// C % 4 == 0, K % 4 == 0; the filter is the channels_last parameter as it is stored, [K, T, C].  With p = T / 2
//   y[n,h,w,k] = bias[k] + sum_{t < T, c < C} x[n, h + (t - p) [axis = H], w + (t - p) [axis = W], c] * w[k,t,c]
// "same" along the filter's axis (positions outside the line read zero), nothing padded on the other axis.
//
// The image is a set of LINES: axis W gives N*H lines of length W at pixel stride 1, axis H gives N*W lines of length H at pixel stride W
// (line (n, w) starts at pixel n*H*W + w).  Both orientations run the same kernels; only the pixel number of (line, position) differs
// (LGeom::pixel), and it is used by the staging loads and the output stores alone.
//
// forward / dgrad (lineconv_fwd_kernel<T>): implicit GEMM, M = lines * L rows in LINE-MAJOR order, N = K, reduction T * C, on
//   v_mfma_f32_32x32x2_f32.  A workgroup (4 waves, 2 x 2, one 32 x 32 accumulator pair each) owns 64 consecutive rows x 64 filters; the rows are
//   whole short lines, or a segment of a long one, and a tile may begin and end in the middle of a line.  Per chunk of 16 channels
//   the rows' pixels are staged ONCE into an LDS panel in "panel coordinates": u(line ll of the tile, position pos) = ll (L + p) + pos + p,
//   pos in [-p, L).  The p coordinates in front of every line hold zeros: they are the leading halo of that line and the trailing halo of
//   the line before it (a tap reaches at most p positions past either end), written as zeros at staging time, as is everything past the
//   last line of the tensor.  The halo of a SEGMENT's cut end inside a line is real data of that line.  Tap t of GEMM row (ll, i) is
//   panel row u(ll, i) - p + t - u0: one address per lane, computed before the channel loop, plus t * pitch.  The k loop has no bounds
//   test, no mask and no select; every x element is fetched from memory once per K tile and used T times out of LDS.  The filter chunk
//   [64 filters][T][16 channels] goes through LDS too.  Which source pixel a panel row holds is decoded once per workgroup into an LDS
//   table (two integer divisions per panel row), not once per chunk.
//   dgrad is the same kernel: at stride 1 and "same" padding dx is the convolution of dy with the taps reversed and C, K exchanged, so it
//   runs on W^T [C, T, K] (nnl_conv2d_weight_transpose) with flip = 1, which stages tap T - 1 - t where the forward stages tap t.
//   LDS banks (fragment reads are ds_read_b128, served a quarter wave at a time, 16 lanes x 16 B = 64 banks): a lane's quad index is
//   row * pitch / 4 + const.  Panel pitch 20 floats = 5 quads and filter pitch 16 T + 4 floats = 4 T + 1 quads are odd, so 16 consecutive
//   rows fall on 16 different quad banks: the filter fragment is always free of conflicts, the panel fragment is free inside a line; a
//   quarter wave whose 16 rows straddle a line end skips p panel rows there and can meet a two-way conflict on at most p of its quads.
// wgrad (lineconv_wgrad_kernel<T>): dw[k,t,c] = sum_rows dy[row,k] * x[row shifted by t - p, c].  A workgroup owns 64 filters x 64 channels
//   and a slab of the line-major rows; it walks the slab in chunks of 32 rows, staging dy [32][64] and the same padded x panel [.][64] once
//   per chunk for all T taps; a wave owns a 32 x 32 piece with T accumulator tiles (16 registers per tap, 112 at T = 7).  The panel row
//   of each chunk row comes from a small LDS table, so the MFMA loop holds one table read and one multiply-add per T MFMAs.  Operands are
//   read as scalars [row][channel] (32 consecutive lanes = 32 consecutive banks; pitch 72 puts the other half wave, 4 rows on, 32 banks
//   further: no conflicts).  A slab's partial [K,T,C] goes to its own part of the workspace and a second launch adds the slabs in slab
//   order; one slab writes dw directly.
// No atomics anywhere: two calls on the same inputs give the same bits.
#include "nnl_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BM = 64, BN = 64, BK = 16;       // forward tile: rows x filters, channels per chunk
constexpr int APITCH = BK + 4;                 // panel pitch (floats)
constexpr int TL = 68;                         // pitch of the epilogue's output tile
constexpr int RB = 32;                         // wgrad: rows per chunk
constexpr int WT = 64;                         // wgrad: filters and channels per workgroup
constexpr int WP = 72;                         // wgrad: LDS pitch of both operands
constexpr int WG_ROWS = 256;                   // fewest rows per wgrad slab (a multiple of RB)
constexpr int WG_SLABS = 64;                   // most wgrad slabs
constexpr int WG_GRID = 512;                   // slabs are added until the grid has about this many workgroups

struct LGeom {
  int lines, L, C, K, M;                       // M = lines * L GEMM rows
  int inner, outer_px, pix_px;                 // pixel(line, pos) = (line / inner) outer_px + line % inner + pos pix_px
  int fwd_rows, wg_rows;                       // most panel rows of a forward tile / of a wgrad chunk
  __host__ __device__ int pixel(int line, int pos) const { return (line / inner) * outer_px + line % inner + pos * pix_px; }
};

// most panel rows of `rows` consecutive line-major GEMM rows: the rows, T - 1 halo positions, p zero positions per line end crossed
__host__ __device__ constexpr int panel_rows(int rows, int L, int T) { return rows + T - 1 + ((L + rows - 2) / L) * (T / 2); }

// the pixel held by panel coordinate u of a tile whose first line is line0, or -1 for a row of zeros
__device__ __forceinline__ int panel_pixel(const LGeom& g, int u, int line0, int p) {
  const int span = g.L + p;
  const int ll = u / span, pos = u - ll * span - p, line = line0 + ll;
  return (pos < 0 || line >= g.lines) ? -1 : g.pixel(line, pos);
}

template <int T>
__global__ __launch_bounds__(256) void lineconv_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                           const float* __restrict__ bias, float* __restrict__ y, LGeom g, int flip, int relu) {
  constexpr int P = T / 2, BP = T * BK + 4;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  int* s_src = reinterpret_cast<int*>(smem);                        // [fwd_rows] pixel of each panel row
  float* As = smem + ((g.fwd_rows + 3) & ~3);                       // [fwd_rows][APITCH]
  float* Bs = As + g.fwd_rows * APITCH;                             // [BN][T][BK] at pitch BP
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  const int grid_n = (g.K + BN - 1) / BN;
  const int tile_m = blockIdx.x / grid_n, tile_n = blockIdx.x - tile_m * grid_n;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int span = g.L + P;
  const int line0 = m0 / g.L, i0 = m0 - line0 * g.L;                // the tile's first row: panel coordinate u0 = i0 is panel row 0
  const int mlast = min(m0 + BM, g.M) - 1;
  const int llast = mlast / g.L;
  const int nrows = (llast - line0) * span + (mlast - llast * g.L) - i0 + T;        // <= g.fwd_rows (panel_rows)
  for (int r = tid; r < nrows; r += 256) s_src[r] = panel_pixel(g, r + i0, line0, P);
  // this lane's GEMM row (a row past the end computes the last row again and is not stored) and its fragment addresses
  const int m = min(m0 + wm * 32 + (lane & 31), mlast);
  const int ln = m / g.L;
  const float* a_frag = As + ((ln - line0) * span + (m - ln * g.L) - i0) * APITCH + (lane >> 5) * 4;
  const float* b_frag = Bs + (wn * 32 + (lane & 31)) * BP + (lane >> 5) * 4;
  f32x16 acc, acc2;                                                 // two chains: consecutive MFMAs are independent
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = acc2[e] = 0.f;
  __syncthreads();
  for (int c0 = 0; c0 < g.C; c0 += BK) {
    for (int i = tid; i < nrows * (BK / 4); i += 256) {
      const int r = i >> 2, c = c0 + (i & 3) * 4, px = s_src[r];
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (px >= 0 && c < g.C) v = *reinterpret_cast<const f32x4*>(x + (long)px * g.C + c);
      *reinterpret_cast<f32x4*>(As + r * APITCH + (i & 3) * 4) = v;
    }
    for (int i = tid; i < BN * T * (BK / 4); i += 256) {
      const int kr = i / (T * 4), rem = i - kr * (T * 4), t = rem >> 2, c = c0 + (rem & 3) * 4;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (n0 + kr < g.K && c < g.C) v = *reinterpret_cast<const f32x4*>(w + ((long)(n0 + kr) * T + (flip ? T - 1 - t : t)) * g.C + c);
      *reinterpret_cast<f32x4*>(Bs + kr * BP + t * BK + (rem & 3) * 4) = v;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const f32x4 a0 = *reinterpret_cast<const f32x4*>(a_frag + t * APITCH), a1 = *reinterpret_cast<const f32x4*>(a_frag + t * APITCH + 8);
      const f32x4 b0 = *reinterpret_cast<const f32x4*>(b_frag + t * BK), b1 = *reinterpret_cast<const f32x4*>(b_frag + t * BK + 8);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[j], b0[j], acc, 0, 0, 0);
        acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[j], b1[j], acc2, 0, 0, 0);
      }
    }
    __syncthreads();
  }
  // epilogue: the tile goes through LDS (free: the loop ended with a barrier) so that 16 lanes store 256 contiguous bytes of an output row
  float* tl = As;                                                   // [BM][TL]
#pragma unroll
  for (int e = 0; e < 16; ++e)
    tl[(wm * 32 + (e & 3) + 8 * (e >> 2) + (lane >> 5) * 4) * TL + wn * 32 + (lane & 31)] = acc[e] + acc2[e];
  __syncthreads();
#pragma unroll
  for (int k4 = 0; k4 < 4; ++k4) {
    const int idx4 = tid + k4 * 256, rl = idx4 >> 4, k = n0 + (idx4 & 15) * 4, row = m0 + rl;
    if (row > mlast || k >= g.K) continue;
    f32x4 v = *reinterpret_cast<const f32x4*>(tl + rl * TL + (idx4 & 15) * 4);
    if (bias != nullptr) v += *reinterpret_cast<const f32x4*>(bias + k);
    if (relu) v = f32x4{fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f)};
    const int line = row / g.L;
    *reinterpret_cast<f32x4*>(y + (long)g.pixel(line, row - line * g.L) * g.K + k) = v;
  }
}

template <int T>
__global__ __launch_bounds__(256) void lineconv_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ out,
                                                             LGeom g, int slab_rows) {
  constexpr int P = T / 2;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  int* s_src = reinterpret_cast<int*>(smem);                        // [wg_rows] pixel of each panel row
  int* s_prow = s_src + ((g.wg_rows + 3) & ~3);                     // [RB] panel row of tap 0 of each chunk row
  int* s_dpx = s_prow + RB;                                         // [RB] pixel of each chunk row, -1 past the slab's end
  float* ds = reinterpret_cast<float*>(s_dpx + RB);                 // [RB][WP] dy
  float* xs = ds + RB * WP;                                         // [wg_rows][WP] x panel
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wk = wave >> 1, wc = wave & 1, half = lane >> 5, l31 = lane & 31;
  const int ctiles = (g.C + WT - 1) / WT;
  const int k0 = (blockIdx.x / ctiles) * WT, c0 = (blockIdx.x % ctiles) * WT;
  const int r_begin = blockIdx.y * slab_rows, r_end = min(g.M, r_begin + slab_rows);
  const int span = g.L + P;
  f32x16 acc[T];
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
  for (int mc = r_begin; mc < r_end; mc += RB) {
    const int line0 = mc / g.L, i0 = mc - line0 * g.L;
    const int mlast = min(mc + RB, r_end) - 1;
    const int llast = mlast / g.L;
    const int nrows = (llast - line0) * span + (mlast - llast * g.L) - i0 + T;      // <= g.wg_rows
    if (tid < RB) {
      const int m = mc + tid, ln = m / g.L, pos = m - ln * g.L;
      const bool live = m <= mlast;
      s_prow[tid] = live ? (ln - line0) * span + pos - i0 : 0;      // a dead row multiplies dy = 0 with panel row 0, which is always staged
      s_dpx[tid] = live ? g.pixel(ln, pos) : -1;
    }
    for (int r = tid; r < nrows; r += 256) s_src[r] = panel_pixel(g, r + i0, line0, P);
    __syncthreads();
    for (int i = tid; i < RB * (WT / 4); i += 256) {
      const int r = i >> 4, q = (i & 15) * 4, px = s_dpx[r];
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (px >= 0 && k0 + q < g.K) v = *reinterpret_cast<const f32x4*>(dy + (long)px * g.K + k0 + q);
      *reinterpret_cast<f32x4*>(ds + r * WP + q) = v;
    }
    for (int i = tid; i < nrows * (WT / 4); i += 256) {
      const int r = i >> 4, q = (i & 15) * 4, px = s_src[r];
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (px >= 0 && c0 + q < g.C) v = *reinterpret_cast<const f32x4*>(x + (long)px * g.C + c0 + q);
      *reinterpret_cast<f32x4*>(xs + r * WP + q) = v;
    }
    __syncthreads();
#pragma unroll 4
    for (int s = 0; s < RB / 2; ++s) {                              // the MFMA reduces two rows: row 2 s + half comes from this half wave
      const int rr = 2 * s + half;
      const float a = ds[rr * WP + wk * 32 + l31];
      const float* xb = xs + s_prow[rr] * WP + wc * 32 + l31;
#pragma unroll
      for (int t = 0; t < T; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, xb[t * WP], acc[t], 0, 0, 0);
    }
    __syncthreads();
  }
  float* o = out + (long)blockIdx.y * g.K * T * g.C;
  const int c = c0 + wc * 32 + l31;
  if (c < g.C) {
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int k = k0 + wk * 32 + (e & 3) + 8 * (e >> 2) + half * 4;
        if (k < g.K) o[((long)k * T + t) * g.C + c] = acc[t][e];
      }
  }
}

__global__ __launch_bounds__(256) void lineconv_wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw, long numel, int slabs) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= numel) return;
  float a = part[i];
  for (int sl = 1; sl < slabs; ++sl) a += part[(long)sl * numel + i];       // slab order: fixed
  dw[i] = a;
}

int make_geom(const char* who, int64_t N, int64_t H, int64_t W, int64_t C, int64_t K, int T, int axis, LGeom* g) {
  NNL_CHECK_ARG(N > 0 && H > 0 && W > 0 && C > 0 && K > 0, "%s: sizes must be positive", who);
  NNL_CHECK_ARG(T == 3 || T == 5 || T == 7, "%s: T = %d taps (3, 5 or 7)", who, T);
  NNL_CHECK_ARG(axis == 0 || axis == 1, "%s: axis = %d (0: along H, a (T, 1) filter; 1: along W, a (1, T) filter)", who, axis);
  NNL_CHECK_ARG(C % 4 == 0 && K % 4 == 0, "%s: C = %ld and K = %ld must be multiples of 4", who, (long)C, (long)K);
  NNL_CHECK_ARG(N * H * W * (C > K ? C : K) < (1L << 31) && K * T * C < (1L << 31), "%s: tensor too large", who);
  const int L = (int)(axis == 1 ? W : H);
  g->lines = (int)(axis == 1 ? N * H : N * W);
  g->L = L; g->C = (int)C; g->K = (int)K; g->M = (int)(N * H * W);
  g->inner = axis == 1 ? 1 : (int)W;
  g->outer_px = axis == 1 ? (int)W : (int)(H * W);
  g->pix_px = axis == 1 ? 1 : (int)W;
  g->fwd_rows = panel_rows(BM, L, T);
  g->wg_rows = panel_rows(RB, L, T);
  return NNL_OK;
}

size_t fwd_lds(const LGeom& g, int T) {
  const size_t loop = ((g.fwd_rows + 3) & ~3) + (size_t)g.fwd_rows * APITCH + (size_t)BN * (T * BK + 4);
  const size_t epi = ((g.fwd_rows + 3) & ~3) + (size_t)BM * TL;
  return (loop > epi ? loop : epi) * sizeof(float);
}

// rows per wgrad slab: a multiple of RB, at least WG_ROWS, and no more slabs than fill the grid or than WG_SLABS
long wgrad_slab_rows(const LGeom& g) {
  const long tiles = nnl_cdiv(g.K, WT) * nnl_cdiv(g.C, WT);
  long slabs = WG_GRID / tiles;
  slabs = slabs < 1 ? 1 : (slabs > WG_SLABS ? WG_SLABS : slabs);
  const long rows = nnl_cdiv(nnl_cdiv(g.M, slabs), RB) * RB;
  return rows > WG_ROWS ? rows : WG_ROWS;
}

}  // namespace

extern "C" int nnl_lineconv2d_fwd(const float* x, const float* w, const float* bias, float* y, int64_t N, int64_t H, int64_t W, int64_t C,
                                  int64_t K, int T, int axis, int flip, int relu, void* stream) {
  LGeom g;
  if (int e = make_geom("lineconv2d_fwd", N, H, W, C, K, T, axis, &g)) return e;
  NNL_CHECK_ARG(x && w && y, "lineconv2d_fwd: null pointer");
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(flip ? NNL_PROF_CONV_DGRAD : NNL_PROF_CONV_FWD, s, 2.0 * g.M * T * C * K);
  const dim3 grid((unsigned)(nnl_cdiv(g.M, BM) * nnl_cdiv(K, BN)));
  const size_t shm = fwd_lds(g, T);
  NNL_ROUTE("lineconv_fwd<%d>:%s%s", T, axis ? "w" : "h", flip ? ",flip" : "");
  if (T == 3)
    hipLaunchKernelGGL(lineconv_fwd_kernel<3>, grid, dim3(256), shm, s, x, w, bias, y, g, flip, relu);
  else if (T == 5)
    hipLaunchKernelGGL(lineconv_fwd_kernel<5>, grid, dim3(256), shm, s, x, w, bias, y, g, flip, relu);
  else
    hipLaunchKernelGGL(lineconv_fwd_kernel<7>, grid, dim3(256), shm, s, x, w, bias, y, g, flip, relu);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}

extern "C" size_t nnl_lineconv2d_wgrad_workspace_bytes(int64_t N, int64_t H, int64_t W, int64_t C, int64_t K, int T, int axis) {
  LGeom g;
  if (make_geom("lineconv2d_wgrad_workspace_bytes", N, H, W, C, K, T, axis, &g)) return 0;
  const long slabs = nnl_cdiv(g.M, wgrad_slab_rows(g));
  return slabs > 1 ? (size_t)slabs * K * T * C * sizeof(float) : 0;
}

extern "C" int nnl_lineconv2d_wgrad(const float* x, const float* dy, float* dw, void* ws, size_t ws_bytes, int64_t N, int64_t H, int64_t W,
                                    int64_t C, int64_t K, int T, int axis, void* stream) {
  LGeom g;
  if (int e = make_geom("lineconv2d_wgrad", N, H, W, C, K, T, axis, &g)) return e;
  NNL_CHECK_ARG(x && dy && dw, "lineconv2d_wgrad: null pointer");
  const long rows = wgrad_slab_rows(g), slabs = nnl_cdiv(g.M, rows), numel = (long)K * T * C;
  if (slabs > 1 && (ws == nullptr || ws_bytes < (size_t)slabs * numel * sizeof(float)))
    return nnl_set_error(NNL_ERR_WORKSPACE, "lineconv2d_wgrad: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_CONV_WGRAD, s, 2.0 * g.M * T * C * K);
  float* out = slabs > 1 ? (float*)ws : dw;
  const dim3 grid((unsigned)(nnl_cdiv(K, WT) * nnl_cdiv(C, WT)), (unsigned)slabs);
  const size_t shm = (((g.wg_rows + 3) & ~3) + 2 * RB + (size_t)(RB + g.wg_rows) * WP) * sizeof(float);
  NNL_ROUTE("lineconv_wgrad<%d>:%s@s%ld", T, axis ? "w" : "h", slabs);
  if (T == 3)
    hipLaunchKernelGGL(lineconv_wgrad_kernel<3>, grid, dim3(256), shm, s, x, dy, out, g, (int)rows);
  else if (T == 5)
    hipLaunchKernelGGL(lineconv_wgrad_kernel<5>, grid, dim3(256), shm, s, x, dy, out, g, (int)rows);
  else
    hipLaunchKernelGGL(lineconv_wgrad_kernel<7>, grid, dim3(256), shm, s, x, dy, out, g, (int)rows);
  NNL_CHECK_LAUNCH();
  if (slabs > 1) {
    hipLaunchKernelGGL(lineconv_wgrad_reduce_kernel, dim3((unsigned)nnl_cdiv(numel, 256)), dim3(256), 0, s, (const float*)ws, dw, numel, (int)slabs);
    NNL_CHECK_LAUNCH();
  }
  return NNL_OK;
}
