// Grouped convolution at wide groups (Cg, Kg in {16, 32}: the 14 x 14 and 7 x 7 stages of ResNeXt-101 and SENet) on the exact-fp32 MFMA
// v_mfma_f32_16x16x4_f32.  Included by gconv.hip only (GGeom, f32x4 and the slab reduction live there).
//
// Lane mapping of the instruction (as used in lstm_bptt2.hip): lane l = (i = l % 16, kq = l / 16) supplies A[row i][slot kq] and
// B[slot kq][col i] and holds D[row 4 kq + v][col i] in accumulator element v.  A 16-column tile is one group at 16 columns per group
// and half a group at 32.
//
//   forward / dgrad  ONE template.  Per group a GEMM: rows = the flattened pixels (forward: N*P*Q outputs, dgrad: N*H*W inputs),
//                    columns = the group's COLS channels (Kg / Cg), reduction over (tap, the group's RED channels: Cg / Kg).  A workgroup
//                    (4 waves) owns a block of whole groups (two at RED = 16, one at 32) and walks 64-row tiles with blockIdx.x striding
//                    over them, so its filter block is staged in LDS once, as [group][tap][red / 4][col][red % 4]: lane (i, kq) reads
//                    the four B values of a tap as one 16-byte LDS word, consecutive lanes read consecutive words.  The dgrad stages
//                    the same global filter with the roles of k and c swapped; no transposed copy exists anywhere.  Wave w owns rows
//                    16 w .. 16 w + 15 and every column tile; lane (i, kq) loads channels 4 kq .. 4 kq + 3 (+16 at RED = 32) of row i at
//                    the tap as 16-byte global loads, zero outside the image, and element e feeds MFMA e against element e of the B word:
//                    within a tap the reduction order is a fixed permutation, the same on both operands.  The next tap's A vectors are
//                    loaded while the current tap's MFMAs issue.  At stride 2 three of four dgrad taps are such zeros (three layers per
//                    network; accepted).
//   wgrad            per (group, tap) a Kg x Cg product over the pixels: A = dy^T (lane: k = i of pixel kq of the step), B = x at the
//                    tap (lane: c = i of the same pixel), both 64-byte rows; one MFMA consumes four pixels.  A wave owns one
//                    (group, k tile, c tile) and keeps the accumulators of all R*R taps, so a dy value is loaded once for every tap.
//                    The pixels are cut into slices (grid.y); each slice writes its partial [K, R, R, Cg] slab and
//                    gconv_wgrad_reduce_kernel adds the slabs in slice order.
// No atomics: two calls give the same bits.
#pragma once

namespace {

constexpr int MF_ROWS = 64;      // rows of a forward / dgrad tile: 4 waves x 16
constexpr int MF_BLOCKS = 1024;  // workgroups the forward / dgrad grid aims at (4 per CU fit with 36 KB of LDS each)
constexpr int MF_WG_ROWS = 256;  // fewest pixels per wgrad slice
constexpr int MF_WG_SLICES = 64; // most wgrad slices

// the operand pixel that tap (r, s) of row pixel (a, b) reads.  Forward: the input pixel under the tap.  Dgrad: the output pixel whose
// tap (r, s) lands on input pixel (a, b) — it exists when (a + pad - r, b + pad - s) are non-negative multiples of the stride inside P x Q.
template <bool DGRAD>
__device__ __forceinline__ bool mf_tap_src(const GGeom& g, int a, int b, int r, int s, int* sa, int* sb) {
  if (!DGRAD) {
    *sa = a * g.stride - g.pad + r;
    *sb = b * g.stride - g.pad + s;
    return (unsigned)*sa < (unsigned)g.H && (unsigned)*sb < (unsigned)g.W;
  }
  const int th = a + g.pad - r, tw = b + g.pad - s, sh = g.stride - 1;      // stride 1 or 2: sh is both the shift and the remainder mask
  *sa = th >> sh;
  *sb = tw >> sh;
  return th >= 0 && tw >= 0 && ((th | tw) & sh) == 0 && *sa < g.P && *sb < g.Q;
}

template <int RED, int COLS, bool DGRAD>
__global__ __launch_bounds__(256) void gconv_mfma_kernel(const float* __restrict__ src, const float* __restrict__ w,
                                                         const float* __restrict__ bias, float* __restrict__ out, GGeom g, int tilesM,
                                                         int relu) {
  constexpr int GB = RED >= 32 ? 1 : 2, NJ = RED / 16, NT = COLS / 16, RQ = RED / 4;
  extern __shared__ float sw[];                       // [GB][tap][RED / 4][COLS][4]
  const int RR = g.R * g.R;
  const int g0 = blockIdx.y * GB, ng = min(GB, g.G - g0);
  const long wk = (long)RR * g.Cg;
  const float* wb = w + (long)g0 * g.Kg * wk;         // the block's filters [ng][Kg][tap][Cg]
  if (!DGRAD) {
    // red = c is the filter's fastest index: 16-byte global loads in memory order, 16-byte LDS stores
    for (int i = threadIdx.x; i < ng * COLS * RR * RQ; i += 256) {
      const int cq = i % RQ, tap = (i / RQ) % RR, kk = i / (RQ * RR);          // kk = gl * COLS + col
      const int gl = kk / COLS, col = kk % COLS;
      *reinterpret_cast<f32x4*>(sw + (((gl * RR + tap) * RQ + cq) * COLS + col) * 4) = *reinterpret_cast<const f32x4*>(wb + (long)i * 4);
    }
  } else {
    // red = k, col = c: scalar loads in memory order, the four k of a word land 4 bytes apart
    for (int i = threadIdx.x; i < ng * RED * RR * COLS; i += 256) {
      const int c = i % COLS, tap = (i / COLS) % RR, kk = i / (COLS * RR);      // kk = gl * RED + k
      const int gl = kk / RED, k = kk % RED;
      sw[(((gl * RR + tap) * RQ + (k >> 2)) * COLS + c) * 4 + (k & 3)] = wb[i];
    }
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, kq = lane >> 4;
  const int SA = DGRAD ? g.P : g.H, SB = DGRAD ? g.Q : g.W, SC = DGRAD ? g.K : g.C;      // the operand tensor [N, SA, SB, SC]
  const int RA = DGRAD ? g.H : g.P, RB = DGRAD ? g.W : g.Q, OC = DGRAD ? g.C : g.K;      // the rows [N, RA, RB] and their OC channels
  const long M = (long)g.N * RA * RB;
  for (int mt = blockIdx.x; mt < tilesM; mt += gridDim.x) {
    const long mw = (long)mt * MF_ROWS + wave * 16;   // the wave's first row
    const long m = mw + li;
    const bool live = m < M;
    const int b = (int)(m % RB), a = (int)((m / RB) % RA), n = (int)(m / ((long)RB * RA));
    f32x4 acc[GB][NT];
#pragma unroll
    for (int gl = 0; gl < GB; ++gl)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[gl][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto load = [&](f32x4 (&dst)[GB][NJ], int r, int s) {
      int sa, sb;
      const bool ok = mf_tap_src<DGRAD>(g, a, b, r, s, &sa, &sb) && live;
      const float* p = src + (((long)(ok ? n : 0) * SA + (ok ? sa : 0)) * SB + (ok ? sb : 0)) * SC + g0 * RED + 4 * kq;
#pragma unroll
      for (int gl = 0; gl < GB; ++gl)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          dst[gl][j] = ok && gl < ng ? *reinterpret_cast<const f32x4*>(p + gl * RED + 16 * j) : f32x4{0.f, 0.f, 0.f, 0.f};
    };
    f32x4 cur[GB][NJ], nxt[GB][NJ];
    load(cur, 0, 0);
    int r = 0, s = 0;
    for (int tap = 0; tap < RR; ++tap) {
      if (++s == g.R) { s = 0; ++r; }
      if (tap + 1 < RR) load(nxt, r, s);              // in flight while this tap's MFMAs issue
      const float* bp = sw + ((tap * RQ + kq) * COLS + li) * 4;
#pragma unroll
      for (int gl = 0; gl < GB; ++gl)
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          f32x4 bf[NT];
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) bf[nt] = *reinterpret_cast<const f32x4*>(bp + ((gl * RR * RQ + 4 * j) * COLS + 16 * nt) * 4);
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[gl][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur[gl][j][e], bf[nt][e], acc[gl][nt], 0, 0, 0);
        }
#pragma unroll
      for (int gl = 0; gl < GB; ++gl)
#pragma unroll
        for (int j = 0; j < NJ; ++j) cur[gl][j] = nxt[gl][j];
    }
    // the lane holds rows 4 kq + v of column li of every tile; the rows are flat in the output ([N, RA, RB, OC])
#pragma unroll
    for (int gl = 0; gl < GB; ++gl) {
      if (gl >= ng) break;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int ch = (g0 + gl) * COLS + nt * 16 + li;
        const float bv = bias != nullptr ? bias[ch] : 0.f;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const long mr = mw + 4 * kq + v;
          float o = acc[gl][nt][v];
          if (bias != nullptr) o += bv;
          if (relu) o = fmaxf(o, 0.f);
          if (mr < M) out[mr * OC + ch] = o;
        }
      }
    }
  }
}

// one wave = (group, 16 filters, 16 channels) x all R*R taps over the pixels [blockIdx.y * rows, +rows) of the flattened N*P*Q, four per MFMA
template <int R>
__global__ __launch_bounds__(256) void gconv_mfma_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                               float* __restrict__ out, GGeom g, int units, long npq, long rows,
                                                               long numel) {
  constexpr int RR = R * R;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, kq = lane >> 4;
  const int unit = blockIdx.x * 4 + wave;
  if (unit >= units) return;                          // (wave-uniform; the kernel has no barrier)
  const int NCT = g.Cg / 16, NKT = g.Kg / 16;
  const int ct = unit % NCT, kt = (unit / NCT) % NKT, grp = unit / (NCT * NKT);
  const long m0 = (long)blockIdx.y * rows, m1 = min(npq, m0 + rows);
  long m = m0 + kq;                                   // the lane's pixel of the current step
  int q = (int)(m % g.Q), p = (int)((m / g.Q) % g.P), n = (int)(m / ((long)g.Q * g.P));
  const float* dyp = dy + grp * g.Kg + kt * 16 + li;
  const float* xp = x + grp * g.Cg + ct * 16 + li;
  auto load = [&](float& av, float (&bv)[RR]) {
    const bool live = m < m1;
    av = live ? dyp[m * g.K] : 0.f;
#pragma unroll
    for (int t = 0; t < RR; ++t) {
      const int h = p * g.stride - g.pad + t / R, ww = q * g.stride - g.pad + t % R;
      const bool ok = live && (unsigned)h < (unsigned)g.H && (unsigned)ww < (unsigned)g.W;
      bv[t] = ok ? xp[(((long)n * g.H + h) * g.W + ww) * g.C] : 0.f;      // (ok: n < N, the pixel is inside the slice)
    }
  };
  f32x4 acc[RR];
#pragma unroll
  for (int t = 0; t < RR; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  float a, bq[RR], an, bn[RR];
  load(a, bq);
  const int steps = (int)((m1 - m0 + 3) / 4);
  for (int st = 0; st < steps; ++st) {
    m += 4;
    q += 4;
    while (q >= g.Q) {
      q -= g.Q;
      if (++p == g.P) { p = 0; ++n; }
    }
    load(an, bn);                                     // the next four pixels (zeros past the slice), in flight under this step's MFMAs
#pragma unroll
    for (int t = 0; t < RR; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bq[t], acc[t], 0, 0, 0);
    a = an;
#pragma unroll
    for (int t = 0; t < RR; ++t) bq[t] = bn[t];
  }
  float* o = out + (long)blockIdx.y * numel + ((long)(grp * g.Kg + kt * 16 + 4 * kq) * RR) * g.Cg + ct * 16 + li;
#pragma unroll
  for (int v = 0; v < 4; ++v)
#pragma unroll
    for (int t = 0; t < RR; ++t) o[((long)v * RR + t) * g.Cg] = acc[t][v];
}

// The shape test of the MFMA route, per direction.  NNL_GCONV_MFMA = 0 sends every shape to the direct kernels (the A/B of
// tools/bench_gconv.py; nothing else).
enum { MF_FWD, MF_DGRAD, MF_WGRAD };
static bool mfma_route(const GGeom& g, int dir) {
  (void)dir;
  const bool dom = (g.Cg == 16 || g.Cg == 32) && (g.Kg == 16 || g.Kg == 32);
  return dom && NNL_ENV_INT("NNL_GCONV_MFMA", 1) != 0;
}

static long mfma_wgrad_rows(const GGeom& g) {
  const long npq = (long)g.N * g.P * g.Q;
  return npq / MF_WG_SLICES > MF_WG_ROWS ? nnl_cdiv(nnl_cdiv(npq, MF_WG_SLICES), 4) * 4 : MF_WG_ROWS;
}

// forward (DGRAD = false: src = x, out = y) and dgrad (src = dy, out = dx, no bias, no ReLU)
template <int RED, int COLS, bool DGRAD>
static void launch_mfma_t(const float* src, const float* w, const float* bias, float* out, const GGeom& g, int relu, hipStream_t s) {
  constexpr int GB = RED >= 32 ? 1 : 2;
  const long M = (long)g.N * (DGRAD ? g.H * g.W : g.P * g.Q);
  const int tilesM = (int)nnl_cdiv(M, MF_ROWS), gy = (int)nnl_cdiv(g.G, GB);
  const int per = (int)nnl_cdiv(tilesM, (gy < MF_BLOCKS ? MF_BLOCKS / gy : 1));          // tiles per workgroup: the filter block is staged once for them
  const dim3 grid((unsigned)nnl_cdiv(tilesM, per), (unsigned)gy);
  const size_t shm = (size_t)GB * g.R * g.R * RED * COLS * sizeof(float);      // <= 36 KB
  hipLaunchKernelGGL((gconv_mfma_kernel<RED, COLS, DGRAD>), grid, dim3(256), shm, s, src, w, bias, out, g, tilesM, relu);
}

template <bool DGRAD>
static void launch_mfma(const float* src, const float* w, const float* bias, float* out, const GGeom& g, int relu, hipStream_t s) {
  const int red = DGRAD ? g.Kg : g.Cg, cols = DGRAD ? g.Cg : g.Kg;
  if (red == 16 && cols == 16) launch_mfma_t<16, 16, DGRAD>(src, w, bias, out, g, relu, s);
  else if (red == 16) launch_mfma_t<16, 32, DGRAD>(src, w, bias, out, g, relu, s);
  else if (cols == 16) launch_mfma_t<32, 16, DGRAD>(src, w, bias, out, g, relu, s);
  else launch_mfma_t<32, 32, DGRAD>(src, w, bias, out, g, relu, s);
}

static void launch_mfma_wgrad(const float* x, const float* dy, float* out, const GGeom& g, long npq, long rows, long slices, long numel,
                              hipStream_t s) {
  const int units = g.G * (g.Kg / 16) * (g.Cg / 16);
  const dim3 grid((unsigned)nnl_cdiv(units, 4), (unsigned)slices);
  if (g.R == 1)
    hipLaunchKernelGGL(gconv_mfma_wgrad_kernel<1>, grid, dim3(256), 0, s, x, dy, out, g, units, npq, rows, numel);
  else
    hipLaunchKernelGGL(gconv_mfma_wgrad_kernel<3>, grid, dim3(256), 0, s, x, dy, out, g, units, npq, rows, numel);
}

}  // namespace
