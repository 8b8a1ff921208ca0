// K20 concat-fused residual 1x1 projection: the tail of the 40 residual blocks of InceptionResNetV2 (reference
// Applications/VisionModels/inceptionresnetv2.py:142-150 Block35, :194-201 Block17, :256-264 Block8)
//   y[m,k] = act( residual[m,k] + scale (bias[k] + sum_s sum_c x_s[m,c] w[k, off_s + c]) ),     act = ReLU or nothing.
// NHWC fp32.  The sources are n_src <= 4 separate tensors [M, C_s] (M = N H W, C_s % 4 == 0, Ctot = sum C_s <= 512); w is the 1x1 parameter
// as it is stored, [K, Ctot], K % 4 == 0; source s owns its columns off_s .. off_s + C_s.  torch.cat never exists in memory: the forward
// builds the concatenated rows in LDS only, the backward reads and writes the sources in place.
//
// forward (catproj_fwd_kernel): a workgroup (4 waves, 2 x 2, one 32 x 32 accumulator pair each, v_mfma_f32_32x32x2_f32) owns 64 rows and a
//   RANGE of 64-filter tiles.  It stages its 64 rows of all sources once into a resident panel [64][C16 + 4] (C16 = Ctot rounded up to the
//   16-channel chunk; the columns past Ctot and the rows past M hold zeros), 34 KB at Ctot = 128, 116 KB at 448, 129 KB at 512: dynamic
//   LDS above 64 KB.  Then it walks its filter tiles; per tile the w chunks [64 filters][16 channels] stream through a double-buffered
//   region: chunk i + 1 (or the first chunk of the next tile) is fetched into a register while the 8 MFMAs of chunk i run, written to the
//   other buffer behind them, and one barrier per chunk hands over.  The epilogue sends the tile through LDS (it aliases the w buffers)
//   so that 16 lanes store 256 contiguous bytes of an output row, and applies bias, scale, residual and ReLU there.
//   The planner (plan_split) hands one row tile's filter range to `split` workgroups: the smallest split that brings the grid to the
//   device's CU count, at most the number of filter tiles.  It splits OUTPUT tiles, never a reduction: every y[m,k] is one workgroup's sum
//   over the chunks in order, two MFMA chains added at the end, whatever the split.
//   LDS banks (ds_read_b128 is served a quarter wave at a time, 16 lanes x 16 B = 64 banks): a lane's quad index is row * pitch / 4 + const.
//   The panel pitch C16 + 4 floats = C16 / 4 + 1 quads (C16 / 4 is a multiple of 4) and the filter pitch 20 floats = 5 quads are odd, so the
//   16 consecutive rows of a quarter wave fall on 16 different quad banks: both fragment reads are free of conflicts.
// dgrad (catproj_dgrad_kernel): d x_s[m,c] = scale sum_k g[m,k] w[k, off_s + c], g = dy [y > 0] with ReLU, else dy.  64 rows x 64 concat
//   columns per workgroup, the reduction over K in chunks of 16.  w [K, Ctot] is already the [k][c] operand: no transpose.  g is gated
//   while dy and y are staged ([64][20], read as b128 like the forward's panel); the w chunk [16][72] is read as scalars: 32 consecutive
//   lanes = 32 consecutive banks, and the other half wave reads the row 4 further on, 4 x 72 = 288 = 32 (mod 64) banks away: no conflicts.
//   The next chunk of both is fetched into registers while the MFMAs run.  With ReLU the workgroups of column tile 0 store the staged g as
//   dres, the residual's gradient: the gate is never a pass of its own.  The store decodes per 4-column group which source owns it; a
//   tile may straddle source boundaries, a float4 never does (every C_s is a multiple of 4).
// wgrad (catproj_wgrad_kernel): dw[k, off_s + c] = scale sum_m g[m,k] x_s[m,c].  64 filters x 64 concat columns and a slab of rows per
//   workgroup, walked in chunks of 32 rows; g (gated as above) and the sources (read in place) are staged [32][96] and read as scalars:
//   32 consecutive lanes = 32 consecutive banks, the other half wave reads the next row, 96 = 32 (mod 64) banks away.  A slab's partial
//   [K, Ctot] goes to its own part of the workspace and a second launch adds the slabs in slab order and applies scale; one slab writes
//   scale x its sum to dw directly.
// No atomics anywhere: two calls on the same inputs give the same bits.
#include <limits.h>
#include "nnl_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BM = 64, BN = 64, BK = 16;       // tile: rows x filters (or concat columns), reduction chunk
constexpr int MAX_SRC = 4, MAX_CTOT = 512;
constexpr int WPITCH = BK + 4;                 // forward filter chunk / dgrad g chunk pitch (floats)
constexpr int TL = 68;                         // pitch of the epilogue's output tile
constexpr int TILE_FLOATS = BM * TL;           // >= 2 * BN * WPITCH and >= BM * WPITCH + BK * DP
constexpr int DP = 72;                         // dgrad: pitch of the w chunk [16][.]
constexpr int RB = 32;                         // wgrad: rows per chunk
constexpr int WP = 96;                         // wgrad: LDS pitch of both operands
constexpr int WG_ROWS = 256;                   // fewest rows per wgrad slab (a multiple of RB)
constexpr int WG_SLABS = 64;                   // most wgrad slabs
constexpr int WG_GRID = 512;                   // slabs are added until the grid has about this many workgroups

struct Cat {                                   // the sources (forward, wgrad) or their gradients (dgrad); unused slots: off = INT_MAX
  float* p[MAX_SRC];
  int c[MAX_SRC], off[MAX_SRC];
};

struct Plan {
  Cat cat;
  int n_src, M, Ctot, K;
};

// which tensor owns concat column `col` (a multiple of 4 below Ctot): its base, its channel count, the column inside it.  Unrolled over
// constant indices: the kernel argument is never indexed dynamically.
__device__ __forceinline__ void owner(const Cat& S, int col, float*& p, int& cs, int& loc) {
  p = S.p[0]; cs = S.c[0]; loc = col;
#pragma unroll
  for (int s = 1; s < MAX_SRC; ++s)
    if (col >= S.off[s]) { p = S.p[s]; cs = S.c[s]; loc = col - S.off[s]; }
}

__device__ __forceinline__ f32x4 gate(f32x4 d, f32x4 yv) {
  return f32x4{yv[0] > 0.f ? d[0] : 0.f, yv[1] > 0.f ? d[1] : 0.f, yv[2] > 0.f ? d[2] : 0.f, yv[3] > 0.f ? d[3] : 0.f};
}

__global__ __launch_bounds__(256) void catproj_fwd_kernel(Cat S, const float* __restrict__ w, const float* __restrict__ bias,
                                                          const float* __restrict__ residual, float* __restrict__ y, int M, int Ctot, int K,
                                                          int tps, int split, float scale, int relu) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int c16 = (Ctot + BK - 1) & ~(BK - 1), pitch = c16 + 4, nch = c16 / BK;
  float* Ap = smem;                                                 // [BM][pitch] the concatenated rows
  float* Ws = smem + BM * pitch;                                    // 2 x [BN][WPITCH]; the epilogue's [BM][TL] tile aliases it
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  const int tile_m = blockIdx.x / split, sp = blockIdx.x - tile_m * split;
  const int m0 = tile_m * BM;
  const int nt_end = min((K + BN - 1) / BN, (sp + 1) * tps);        // this workgroup's filter tiles: sp tps .. nt_end (never empty)
  // the panel: 16 lanes fetch 256 contiguous bytes of a row; the owner of a column group is decoded once per 4 rows
  for (int q = tid & 15; q < c16 / 4; q += 16) {
    const int col = q * 4;
    float* p; int cs, loc;
    owner(S, col, p, cs, loc);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = (tid >> 4) + 16 * j;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (col < Ctot && m0 + r < M) v = *reinterpret_cast<const f32x4*>(p + (long)(m0 + r) * cs + loc);
      *reinterpret_cast<f32x4*>(Ap + r * pitch + col) = v;
    }
  }
  const int kr = tid >> 2, cq = (tid & 3) * 4;                      // this thread's float4 of a filter chunk
  auto load_w = [&](int nt, int ch) {
    const int k = nt * BN + kr, c = ch * BK + cq;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (k < K && c < Ctot) v = *reinterpret_cast<const f32x4*>(w + (long)k * Ctot + c);
    return v;
  };
  const float* a_frag = Ap + (wm * 32 + (lane & 31)) * pitch + (lane >> 5) * 4;
  const float* b_frag = Ws + (wn * 32 + (lane & 31)) * WPITCH + (lane >> 5) * 4;
  float* w_st = Ws + kr * WPITCH + cq;
  f32x4 reg = load_w(sp * tps, 0);
  for (int nt = sp * tps; nt < nt_end; ++nt) {
    f32x16 acc, acc2;                                               // two chains: consecutive MFMAs are independent
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = acc2[e] = 0.f;
    *reinterpret_cast<f32x4*>(w_st) = reg;
    __syncthreads();                                                // (the first one also publishes the panel)
    for (int ch = 0; ch < nch; ++ch) {
      const bool more = ch + 1 < nch;
      if (more) reg = load_w(nt, ch + 1);                           // in flight while the MFMAs below run
      else if (nt + 1 < nt_end) reg = load_w(nt + 1, 0);
      const float* af = a_frag + ch * BK;
      const float* bf = b_frag + (ch & 1) * (BN * WPITCH);
      const f32x4 a0 = *reinterpret_cast<const f32x4*>(af), a1 = *reinterpret_cast<const f32x4*>(af + 8);
      const f32x4 b0 = *reinterpret_cast<const f32x4*>(bf), b1 = *reinterpret_cast<const f32x4*>(bf + 8);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[j], b0[j], acc, 0, 0, 0);
        acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[j], b1[j], acc2, 0, 0, 0);
      }
      if (more) *reinterpret_cast<f32x4*>(w_st + ((ch + 1) & 1) * (BN * WPITCH)) = reg;      // the buffer nobody reads in this step
      __syncthreads();
    }
    float* tl = Ws;                                                 // free: the loop ended with a barrier
#pragma unroll
    for (int e = 0; e < 16; ++e)
      tl[(wm * 32 + (e & 3) + 8 * (e >> 2) + (lane >> 5) * 4) * TL + wn * 32 + (lane & 31)] = acc[e] + acc2[e];
    __syncthreads();
#pragma unroll
    for (int k4 = 0; k4 < 4; ++k4) {
      const int idx4 = tid + k4 * 256, rl = idx4 >> 4, k = nt * BN + (idx4 & 15) * 4, row = m0 + rl;
      if (row >= M || k >= K) continue;
      f32x4 v = *reinterpret_cast<const f32x4*>(tl + rl * TL + (idx4 & 15) * 4);
      if (bias != nullptr) v += *reinterpret_cast<const f32x4*>(bias + k);
      v *= scale;
      if (residual != nullptr) v += *reinterpret_cast<const f32x4*>(residual + (long)row * K + k);
      if (relu) v = f32x4{fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f)};
      *reinterpret_cast<f32x4*>(y + (long)row * K + k) = v;
    }
    __syncthreads();                                                // the tile is read before the next filter chunk lands on it
  }
}

__global__ __launch_bounds__(256) void catproj_dgrad_kernel(Cat D, const float* __restrict__ dy, const float* __restrict__ y,
                                                            const float* __restrict__ w, float* __restrict__ dres, int M, int Ctot, int K,
                                                            float scale, int relu) {
  __shared__ __attribute__((aligned(16))) float smem[TILE_FLOATS];
  float* As = smem;                                                 // [BM][WPITCH] g
  float* Bs = smem + BM * WPITCH;                                   // [BK][DP] w chunk, [k][c] as stored
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1, half = lane >> 5, l31 = lane & 31;
  const int ctiles = (Ctot + BN - 1) / BN;
  const int tile_m = blockIdx.x / ctiles, tc = blockIdx.x - tile_m * ctiles;
  const int m0 = tile_m * BM, c0 = tc * BN, nch = (K + BK - 1) / BK;
  const int ar = tid >> 2, aq = (tid & 3) * 4;                      // this thread's float4 of g: row, k
  const int bk = tid >> 4, bq = (tid & 15) * 4;                     // and of the w chunk: k, column
  const bool keep = relu && tc == 0;
  auto load_g = [&](int ch) {
    const int k = ch * BK + aq, row = m0 + ar;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (row < M && k < K) {
      v = *reinterpret_cast<const f32x4*>(dy + (long)row * K + k);
      if (relu) v = gate(v, *reinterpret_cast<const f32x4*>(y + (long)row * K + k));
      if (keep) *reinterpret_cast<f32x4*>(dres + (long)row * K + k) = v;
    }
    return v;
  };
  auto load_w = [&](int ch) {
    const int k = ch * BK + bk, c = c0 + bq;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (k < K && c < Ctot) v = *reinterpret_cast<const f32x4*>(w + (long)k * Ctot + c);
    return v;
  };
  f32x16 acc, acc2;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = acc2[e] = 0.f;
  const float* a_frag = As + (wm * 32 + l31) * WPITCH + half * 4;
  const float* b_frag = Bs + half * 4 * DP + wn * 32 + l31;
  f32x4 rg = load_g(0), rw = load_w(0);
  for (int ch = 0; ch < nch; ++ch) {
    *reinterpret_cast<f32x4*>(As + ar * WPITCH + aq) = rg;
    *reinterpret_cast<f32x4*>(Bs + bk * DP + bq) = rw;
    __syncthreads();
    if (ch + 1 < nch) { rg = load_g(ch + 1); rw = load_w(ch + 1); } // in flight while the MFMAs below run
    const f32x4 a0 = *reinterpret_cast<const f32x4*>(a_frag), a1 = *reinterpret_cast<const f32x4*>(a_frag + 8);
#pragma unroll
    for (int j = 0; j < 4; ++j) {                                   // a0[j] is k = j + 4 half, a1[j] is k = 8 + j + 4 half
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[j], b_frag[j * DP], acc, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[j], b_frag[(8 + j) * DP], acc2, 0, 0, 0);
    }
    __syncthreads();
  }
  float* tl = smem;                                                 // [BM][TL]
#pragma unroll
  for (int e = 0; e < 16; ++e) tl[(wm * 32 + (e & 3) + 8 * (e >> 2) + half * 4) * TL + wn * 32 + l31] = acc[e] + acc2[e];
  __syncthreads();
#pragma unroll
  for (int k4 = 0; k4 < 4; ++k4) {
    const int idx4 = tid + k4 * 256, rl = idx4 >> 4, col = c0 + (idx4 & 15) * 4, row = m0 + rl;
    if (row >= M || col >= Ctot) continue;
    float* p; int cs, loc;
    owner(D, col, p, cs, loc);
    *reinterpret_cast<f32x4*>(p + (long)row * cs + loc) = *reinterpret_cast<const f32x4*>(tl + rl * TL + (idx4 & 15) * 4) * scale;
  }
}

__global__ __launch_bounds__(256) void catproj_wgrad_kernel(Cat S, const float* __restrict__ dy, const float* __restrict__ y,
                                                            float* __restrict__ out, int M, int Ctot, int K, int slab_rows, float oscale,
                                                            int relu) {
  __shared__ __attribute__((aligned(16))) float smem[2 * RB * WP];
  float* gs = smem;                                                 // [RB][WP] g
  float* xs = smem + RB * WP;                                       // [RB][WP] the sources' columns c0 .. c0 + 64
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wk = wave >> 1, wc = wave & 1, half = lane >> 5, l31 = lane & 31;
  const int ctiles = (Ctot + BN - 1) / BN;
  const int k0 = (blockIdx.x / ctiles) * BN, c0 = (blockIdx.x % ctiles) * BN;
  const int r_begin = blockIdx.y * slab_rows, r_end = min(M, r_begin + slab_rows);
  const int sr = tid >> 4, sq = (tid & 15) * 4;                     // this thread's two float4 of each operand: rows sr and sr + 16
  const bool live_k = k0 + sq < K, live_c = c0 + sq < Ctot;
  float* xp; int cs, loc;
  owner(S, live_c ? c0 + sq : 0, xp, cs, loc);
  f32x4 rg[2], rx[2];
  auto load = [&](int mc) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int row = mc + sr + 16 * j;
      rg[j] = rx[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (row < r_end && live_k) {
        rg[j] = *reinterpret_cast<const f32x4*>(dy + (long)row * K + k0 + sq);
        if (relu) rg[j] = gate(rg[j], *reinterpret_cast<const f32x4*>(y + (long)row * K + k0 + sq));
      }
      if (row < r_end && live_c) rx[j] = *reinterpret_cast<const f32x4*>(xp + (long)row * cs + loc);
    }
  };
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  load(r_begin);
  for (int mc = r_begin; mc < r_end; mc += RB) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      *reinterpret_cast<f32x4*>(gs + (sr + 16 * j) * WP + sq) = rg[j];
      *reinterpret_cast<f32x4*>(xs + (sr + 16 * j) * WP + sq) = rx[j];
    }
    __syncthreads();
    if (mc + RB < r_end) load(mc + RB);                             // in flight while the MFMAs below run
#pragma unroll 4
    for (int s = 0; s < RB / 2; ++s) {                              // the MFMA reduces two rows: row 2 s + half comes from this half wave
      const int rr = 2 * s + half;
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(gs[rr * WP + wk * 32 + l31], xs[rr * WP + wc * 32 + l31], acc, 0, 0, 0);
    }
    __syncthreads();
  }
  float* o = out + (long)blockIdx.y * K * Ctot;
  const int c = c0 + wc * 32 + l31;
  if (c < Ctot) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int k = k0 + wk * 32 + (e & 3) + 8 * (e >> 2) + half * 4;
      if (k < K) o[(long)k * Ctot + c] = acc[e] * oscale;
    }
  }
}

__global__ __launch_bounds__(256) void catproj_wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw, long numel, int slabs,
                                                                   float scale) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= numel) return;
  float a = part[i];
  for (int sl = 1; sl < slabs; ++sl) a += part[(long)sl * numel + i];       // slab order: fixed
  dw[i] = a * scale;
}

// the domain; `ptrs` may be null for the size queries
int make_plan(const char* who, const float* const* ptrs, const int64_t* chans, int n_src, int64_t M, int64_t K, Plan* P) {
  NNL_CHECK_ARG(n_src >= 1 && n_src <= MAX_SRC, "%s: n_src = %d sources (1 .. %d)", who, n_src, MAX_SRC);
  NNL_CHECK_ARG(chans != nullptr, "%s: null channel counts", who);
  NNL_CHECK_ARG(M > 0 && K > 0, "%s: sizes must be positive", who);
  NNL_CHECK_ARG(K % 4 == 0, "%s: K = %ld must be a multiple of 4", who, (long)K);
  int64_t ctot = 0;
  for (int s = 0; s < MAX_SRC; ++s) {
    P->cat.p[s] = nullptr; P->cat.c[s] = 0; P->cat.off[s] = INT_MAX;
  }
  for (int s = 0; s < n_src; ++s) {
    NNL_CHECK_ARG(chans[s] > 0 && chans[s] % 4 == 0, "%s: C_%d = %ld must be a positive multiple of 4", who, s, (long)chans[s]);
    NNL_CHECK_ARG(ctot + chans[s] <= MAX_CTOT, "%s: the sources have more than %d channels together", who, MAX_CTOT);
    P->cat.c[s] = (int)chans[s]; P->cat.off[s] = (int)ctot;
    ctot += chans[s];
  }
  NNL_CHECK_ARG(M < (1L << 31) && K < (1L << 31) && M * (K > ctot ? K : ctot) < (1L << 31) && K * ctot < (1L << 31), "%s: tensor too large", who);
  if (ptrs != nullptr)
    for (int s = 0; s < n_src; ++s) {
      NNL_CHECK_ARG(ptrs[s] != nullptr, "%s: source %d is a null pointer", who, s);
      P->cat.p[s] = const_cast<float*>(ptrs[s]);
    }
  P->n_src = n_src; P->M = (int)M; P->Ctot = (int)ctot; P->K = (int)K;
  return NNL_OK;
}

int cu_count() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) n = 256;
    cus = n;
  }
  return cus;
}

// how many workgroups share one row tile's filter range, and the filter tiles each of them takes
void plan_split(const Plan& P, int* split, int* tps) {
  const long row_tiles = nnl_cdiv(P.M, BM), ntn = nnl_cdiv(P.K, BN);
  long s = nnl_cdiv(cu_count(), row_tiles);
  s = s < 1 ? 1 : (s > ntn ? ntn : s);
  *tps = (int)nnl_cdiv(ntn, s);
  *split = (int)nnl_cdiv(ntn, *tps);                                // no workgroup without a tile
}

size_t fwd_lds(int Ctot) {
  const int c16 = (Ctot + BK - 1) & ~(BK - 1);
  return ((size_t)BM * (c16 + 4) + TILE_FLOATS) * sizeof(float);
}

// rows per wgrad slab: a multiple of RB, at least WG_ROWS, and no more slabs than fill the grid or than WG_SLABS
long wgrad_slab_rows(const Plan& P) {
  const long tiles = nnl_cdiv(P.K, BN) * nnl_cdiv(P.Ctot, BN);
  long slabs = WG_GRID / tiles;
  slabs = slabs < 1 ? 1 : (slabs > WG_SLABS ? WG_SLABS : slabs);
  const long rows = nnl_cdiv(nnl_cdiv(P.M, slabs), RB) * RB;
  return rows > WG_ROWS ? rows : WG_ROWS;
}

}  // namespace

extern "C" int nnl_catproj_fwd(const float* const* srcs, const int64_t* chans, int n_src, const float* w, const float* bias,
                               const float* residual, float* y, int64_t M, int64_t K, float scale, int relu, void* stream) {
  Plan P;
  NNL_CHECK_ARG(srcs != nullptr, "catproj_fwd: null source list");
  if (int e = make_plan("catproj_fwd", srcs, chans, n_src, M, K, &P)) return e;
  NNL_CHECK_ARG(w && y, "catproj_fwd: null pointer");
  hipStream_t s = (hipStream_t)stream;
  static bool attr_set = false;                                     // once, for the largest panel: dynamic LDS above 64 KB
  if (!attr_set) {
    NNL_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(catproj_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)fwd_lds(MAX_CTOT)));
    attr_set = true;
  }
  int split, tps;
  plan_split(P, &split, &tps);
  NnlProfScope prof(NNL_PROF_CONV_FWD, s, 2.0 * P.M * P.Ctot * P.K);
  NNL_ROUTE("catproj_fwd:n%d@x%d", n_src, split);
  hipLaunchKernelGGL(catproj_fwd_kernel, dim3((unsigned)(nnl_cdiv(P.M, BM) * split)), dim3(256), fwd_lds(P.Ctot), s, P.cat, w, bias, residual, y,
                     P.M, P.Ctot, P.K, tps, split, scale, relu);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}

extern "C" int nnl_catproj_dgrad(const float* dy, const float* y, const float* w, float* const* dsrcs, const int64_t* chans, int n_src,
                                 float* dres, int64_t M, int64_t K, float scale, int relu, void* stream) {
  Plan P;
  NNL_CHECK_ARG(dsrcs != nullptr, "catproj_dgrad: null gradient list");
  if (int e = make_plan("catproj_dgrad", dsrcs, chans, n_src, M, K, &P)) return e;
  NNL_CHECK_ARG(dy && w, "catproj_dgrad: null pointer");
  NNL_CHECK_ARG(!relu || (y && dres), "catproj_dgrad: the ReLU gate needs y and dres");
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_CONV_DGRAD, s, 2.0 * P.M * P.Ctot * P.K);
  NNL_ROUTE("catproj_dgrad:n%d%s", n_src, relu ? ",gate" : "");
  hipLaunchKernelGGL(catproj_dgrad_kernel, dim3((unsigned)(nnl_cdiv(P.M, BM) * nnl_cdiv(P.Ctot, BN))), dim3(256), 0, s, P.cat, dy, y, w, dres, P.M,
                     P.Ctot, P.K, scale, relu);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}

extern "C" size_t nnl_catproj_wgrad_workspace_bytes(const int64_t* chans, int n_src, int64_t M, int64_t K) {
  Plan P;
  if (make_plan("catproj_wgrad_workspace_bytes", nullptr, chans, n_src, M, K, &P)) return 0;
  const long slabs = nnl_cdiv(P.M, wgrad_slab_rows(P));
  return slabs > 1 ? (size_t)slabs * P.K * P.Ctot * sizeof(float) : 0;
}

extern "C" int nnl_catproj_wgrad(const float* const* srcs, const int64_t* chans, int n_src, const float* dy, const float* y, float* dw, void* ws,
                                 size_t ws_bytes, int64_t M, int64_t K, float scale, int relu, void* stream) {
  Plan P;
  NNL_CHECK_ARG(srcs != nullptr, "catproj_wgrad: null source list");
  if (int e = make_plan("catproj_wgrad", srcs, chans, n_src, M, K, &P)) return e;
  NNL_CHECK_ARG(dy && dw, "catproj_wgrad: null pointer");
  NNL_CHECK_ARG(!relu || y, "catproj_wgrad: the ReLU gate needs y");
  const long rows = wgrad_slab_rows(P), slabs = nnl_cdiv(P.M, rows), numel = (long)P.K * P.Ctot;
  if (slabs > 1 && (ws == nullptr || ws_bytes < (size_t)slabs * numel * sizeof(float)))
    return nnl_set_error(NNL_ERR_WORKSPACE, "catproj_wgrad: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_CONV_WGRAD, s, 2.0 * P.M * P.Ctot * P.K);
  NNL_ROUTE("catproj_wgrad:n%d%s@s%ld", n_src, relu ? ",gate" : "", slabs);
  const dim3 grid((unsigned)(nnl_cdiv(P.K, BN) * nnl_cdiv(P.Ctot, BN)), (unsigned)slabs);
  hipLaunchKernelGGL(catproj_wgrad_kernel, grid, dim3(256), 0, s, P.cat, dy, y, slabs > 1 ? (float*)ws : dw, P.M, P.Ctot, P.K, (int)rows,
                     slabs > 1 ? 1.f : scale, relu);
  NNL_CHECK_LAUNCH();
  if (slabs > 1) {
    hipLaunchKernelGGL(catproj_wgrad_reduce_kernel, dim3((unsigned)nnl_cdiv(numel, 256)), dim3(256), 0, s, (const float*)ws, dw, numel, (int)slabs,
                       scale);
    NNL_CHECK_LAUNCH();
  }
  return NNL_OK;
}
