// K15 grouped convolution (nn.Conv2d(groups=G); reference Applications/VisionModels/senet.py:178-180, 205-206, 229-230: the 3x3 of
// SEBottleneck / SEResNeXtBottleneck), NHWC fp32, filter [K, R, R, Cg] = the parameter's own channels_last memory.
//
// Direct VALU kernels.  On gfx950 the fp32 MFMA runs at the fp32 vector rate, and at Cg <= 8 these layers are bound by their activation
// traffic (Cg = Kg = 4, C = 128, 56 x 56, 64 images: 205 MB in + out against 1.5 GFMA), so the design is about reading every activation
// once from HBM:
//   forward / dgrad  one workgroup = an 8 x 8 pixel tile x a block of whole groups.  The input halo of the tile (for the dgrad: the
//                    window of dy the tile's taps reach) is staged once in LDS; one lane owns one pixel, the four waves walk over quads
//                    of four consecutive output channels of one group, so the filter addresses are wave-uniform.  Each accumulator
//                    runs over its taps in the fixed order (r, s, c).  A reduction wider than 32 channels per group reads its
//                    operand through the cache instead of LDS (no shape of the SENet family does).
//   wgrad            one thread = four filters k x one (r, s, c); the N*P*Q pixels are cut into S slices (grid.y), each slice writes
//                    its partial filter gradient to its own slab of the workspace and a second launch adds the slabs in slice order.
//                    S == 1 writes dw directly.
// No atomics anywhere: two calls on the same inputs give the same bits.
#include "nnl_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int TILE = 8;          // 8 x 8 pixels per workgroup: one pixel per lane of a wave
constexpr int LDS_RED = 32;      // widest per-group reduction (Cg forward, Kg dgrad) that is staged in LDS
constexpr int WG_ROWS = 256;     // fewest pixels per wgrad slice
constexpr int WG_SLICES = 256;   // most wgrad slices

struct GGeom { int N, H, W, C, K, G, R, stride, pad, P, Q, Cg, Kg; };

// groups per workgroup: as many whole groups as fit LDS_RED reduction channels
int groups_per_block(int red) { return red >= LDS_RED ? 1 : LDS_RED / red; }

template <bool LDS>
__global__ __launch_bounds__(256) void gconv_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ bias, float* __restrict__ y, GGeom g, int GB,
                                                        int relu) {
  extern __shared__ float sx[];                       // [HT * HT pixels][Cbp]: the input halo of the tile, GB * Cg channels per pixel
  const int tilesQ = (g.Q + TILE - 1) / TILE;
  const int p0 = (blockIdx.x / tilesQ) * TILE, q0 = (blockIdx.x % tilesQ) * TILE;
  const int g0 = blockIdx.y * GB, n = blockIdx.z;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int HT = (TILE - 1) * g.stride + g.R;
  const int Cb = GB * g.Cg, Cbp = Cb | 1;             // odd pixel pitch: neighbouring pixels land in different banks
  const int h0 = p0 * g.stride - g.pad, w0 = q0 * g.stride - g.pad;
  if (LDS) {
    for (int i = threadIdx.x; i < HT * HT * Cb; i += 256) {
      const int c = i % Cb, pix = i / Cb;
      const int h = h0 + pix / HT, ww = w0 + pix % HT, ch = g0 * g.Cg + c;
      float v = 0.f;
      if ((unsigned)h < (unsigned)g.H && (unsigned)ww < (unsigned)g.W && ch < g.C) v = x[(((long)n * g.H + h) * g.W + ww) * g.C + ch];
      sx[pix * Cbp + c] = v;
    }
    __syncthreads();
  }
  const int lp = lane >> 3, lq = lane & 7;
  const int p = p0 + lp, q = q0 + lq;
  const bool live = p < g.P && q < g.Q;
  const int KQ = (g.Kg + 3) / 4;                      // quads of output channels per group (the last one may be partial)
  const long wk = (long)g.R * g.R * g.Cg;             // filter elements per output channel
  for (int u = wave; u < GB * KQ; u += 4) {           // (wave-uniform: scalar filter loads)
    const int gl = u / KQ, grp = g0 + gl;
    if (grp >= g.G) break;
    const int kl = (u % KQ) * 4, k0 = grp * g.Kg + kl;
    const int nk = min(4, g.Kg - kl);
    const float* wj[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) wj[j] = w + (long)(k0 + min(j, nk - 1)) * wk;      // a partial quad repeats its last filter (not stored)
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int r = 0; r < g.R; ++r)
      for (int s = 0; s < g.R; ++s) {
        const int t = (r * g.R + s) * g.Cg;
        if (LDS) {
          const float* xp = sx + ((lp * g.stride + r) * HT + lq * g.stride + s) * Cbp + gl * g.Cg;
          for (int c = 0; c < g.Cg; ++c) {
            const float xv = xp[c];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = __builtin_fmaf(xv, wj[j][t + c], acc[j]);
          }
        } else {
          const int h = p * g.stride - g.pad + r, ww = q * g.stride - g.pad + s;
          const bool in = live && (unsigned)h < (unsigned)g.H && (unsigned)ww < (unsigned)g.W;
          const float* xp = x + (((long)n * g.H + (in ? h : 0)) * g.W + (in ? ww : 0)) * g.C + grp * g.Cg;
          for (int c = 0; c < g.Cg; ++c) {
            const float xv = in ? xp[c] : 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = __builtin_fmaf(xv, wj[j][t + c], acc[j]);
          }
        }
      }
    if (!live) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (bias != nullptr) acc[j] += bias[k0 + min(j, nk - 1)];
      if (relu) acc[j] = fmaxf(acc[j], 0.f);
    }
    float* yp = y + (((long)n * g.P + p) * g.Q + q) * g.K + k0;
    if ((g.Kg & 3) == 0) {
      *reinterpret_cast<f32x4*>(yp) = f32x4{acc[0], acc[1], acc[2], acc[3]};
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < nk) yp[j] = acc[j];
    }
  }
}

// dx[n,h,w,c] = sum_{r,s} sum_{k in group(c)} dy[n,p,q,k] * w[k,r,s,c] over the taps with p = (h + pad - r) / stride, q likewise, integral
template <bool LDS>
__global__ __launch_bounds__(256) void gconv_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                          float* __restrict__ dx, GGeom g, int GB) {
  extern __shared__ float sdy[];                      // [DT * DT pixels][Kbp]: the window of dy the tile's taps reach
  const int tilesW = (g.W + TILE - 1) / TILE;
  const int h0 = (blockIdx.x / tilesW) * TILE, w0 = (blockIdx.x % tilesW) * TILE;
  const int g0 = blockIdx.y * GB, n = blockIdx.z;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  // a tap of pixel h needs p * stride = h + pad - r: p >= pb, and p <= (h0 + TILE - 1 + pad) / stride <= pb + DT - 1
  const int DT = (TILE - 1 + g.R - 1) / g.stride + 2;
  const int pb = max(0, h0 + g.pad - g.R + 1) / g.stride, qb = max(0, w0 + g.pad - g.R + 1) / g.stride;
  const int Kb = GB * g.Kg, Kbp = Kb | 1;
  if (LDS) {
    for (int i = threadIdx.x; i < DT * DT * Kb; i += 256) {
      const int k = i % Kb, pix = i / Kb;
      const int p = pb + pix / DT, q = qb + pix % DT, ch = g0 * g.Kg + k;
      float v = 0.f;
      if (p < g.P && q < g.Q && ch < g.K) v = dy[(((long)n * g.P + p) * g.Q + q) * g.K + ch];
      sdy[pix * Kbp + k] = v;
    }
    __syncthreads();
  }
  const int h = h0 + (lane >> 3), ww = w0 + (lane & 7);
  const bool live = h < g.H && ww < g.W;
  const int CQ = (g.Cg + 3) / 4;                      // quads of input channels per group
  const long wk = (long)g.R * g.R * g.Cg;
  for (int u = wave; u < GB * CQ; u += 4) {
    const int gl = u / CQ, grp = g0 + gl;
    if (grp >= g.G) break;
    const int cl = (u % CQ) * 4;
    const int nc = min(4, g.Cg - cl);
    int cj[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) cj[j] = cl + min(j, nc - 1);
    const float* wg = w + (long)grp * g.Kg * wk;      // the group's filters [Kg][R][R][Cg]
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int r = 0; r < g.R; ++r) {
      const int th = h + g.pad - r;
      const int p = th / g.stride;
      const bool okh = live && th >= 0 && th - p * g.stride == 0 && p < g.P;
      for (int s = 0; s < g.R; ++s) {
        const int tw = ww + g.pad - s;
        const int q = tw / g.stride;
        const bool ok = okh && tw >= 0 && tw - q * g.stride == 0 && q < g.Q;
        const float* wt = wg + (r * g.R + s) * g.Cg;
        if (LDS) {
          const float* dp = sdy + (ok ? ((p - pb) * DT + (q - qb)) * Kbp + gl * g.Kg : 0);
          for (int k = 0; k < g.Kg; ++k) {
            const float dv = ok ? dp[k] : 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = __builtin_fmaf(dv, wt[k * wk + cj[j]], acc[j]);
          }
        } else {
          const float* dp = dy + (((long)n * g.P + (ok ? p : 0)) * g.Q + (ok ? q : 0)) * g.K + grp * g.Kg;
          for (int k = 0; k < g.Kg; ++k) {
            const float dv = ok ? dp[k] : 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = __builtin_fmaf(dv, wt[k * wk + cj[j]], acc[j]);
          }
        }
      }
    }
    if (!live) continue;
    float* xp = dx + (((long)n * g.H + h) * g.W + ww) * g.C + grp * g.Cg + cl;
    if ((g.Cg & 3) == 0) {
      *reinterpret_cast<f32x4*>(xp) = f32x4{acc[0], acc[1], acc[2], acc[3]};
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < nc) xp[j] = acc[j];
    }
  }
}

// one thread = (group, quad of filters, r, s, c) over the pixels [blockIdx.y * rows, +rows) of the flattened N*P*Q, in pixel order
__global__ __launch_bounds__(256) void gconv_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                          float* __restrict__ out, GGeom g, long units, long npq, long rows, long numel) {
  long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= units) return;
  const int KQ = (g.Kg + 3) / 4;
  const int c = (int)(t % g.Cg); t /= g.Cg;
  const int s = (int)(t % g.R); t /= g.R;
  const int r = (int)(t % g.R); t /= g.R;
  const int kl = (int)(t % KQ) * 4, grp = (int)(t / KQ);
  const int nk = min(4, g.Kg - kl), k0 = grp * g.Kg + kl;
  int kj[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) kj[j] = k0 + min(j, nk - 1);
  const long m0 = (long)blockIdx.y * rows, m1 = min(npq, m0 + rows);
  int q = (int)(m0 % g.Q), p = (int)((m0 / g.Q) % g.P), n = (int)(m0 / ((long)g.Q * g.P));
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (long m = m0; m < m1; ++m) {
    const int h = p * g.stride - g.pad + r, ww = q * g.stride - g.pad + s;
    if ((unsigned)h < (unsigned)g.H && (unsigned)ww < (unsigned)g.W) {
      const float xv = x[(((long)n * g.H + h) * g.W + ww) * g.C + grp * g.Cg + c];
      const float* dp = dy + m * g.K;
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = __builtin_fmaf(xv, dp[kj[j]], acc[j]);
    }
    if (++q == g.Q) {
      q = 0;
      if (++p == g.P) { p = 0; ++n; }
    }
  }
  float* o = out + (long)blockIdx.y * numel;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < nk) o[((long)(k0 + j) * g.R * g.R + r * g.R + s) * g.Cg + c] = acc[j];
}

__global__ __launch_bounds__(256) void gconv_wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw, long numel,
                                                                 int slices) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= numel) return;
  float a = part[i];
  for (int sl = 1; sl < slices; ++sl) a += part[(long)sl * numel + i];      // slice order: fixed
  dw[i] = a;
}

int make_geom(const char* who, int64_t N, int64_t H, int64_t W, int64_t C, int64_t K, int64_t G, int R, int stride, int pad, GGeom* g) {
  NNL_CHECK_ARG(N > 0 && H > 0 && W > 0 && C > 0 && K > 0 && G > 0, "%s: sizes must be positive", who);
  NNL_CHECK_ARG(C % G == 0 && K % G == 0, "%s: groups = %ld must divide C = %ld and K = %ld", who, (long)G, (long)C, (long)K);
  NNL_CHECK_ARG(R == 1 || R == 3, "%s: kernel_size R = %d (1 or 3)", who, R);
  NNL_CHECK_ARG(stride == 1 || stride == 2, "%s: stride = %d (1 or 2)", who, stride);
  NNL_CHECK_ARG(pad >= 0 && pad <= R / 2, "%s: padding = %d (0 .. R / 2)", who, pad);
  NNL_CHECK_ARG(H + 2 * pad >= R && W + 2 * pad >= R, "%s: filter larger than the padded input", who);
  const int64_t P = (H + 2 * pad - R) / stride + 1, Q = (W + 2 * pad - R) / stride + 1;
  NNL_CHECK_ARG(N < 65536 && G < 65536 && N * H * W * C < (1L << 31) && N * P * Q * K < (1L << 31) && K * R * R * (C / G) < (1L << 31),
                "%s: tensor too large", who);
  *g = GGeom{(int)N, (int)H, (int)W, (int)C, (int)K, (int)G, R, stride, pad, (int)P, (int)Q, (int)(C / G), (int)(K / G)};
  return NNL_OK;
}

long wgrad_rows(const GGeom& g) {
  const long npq = (long)g.N * g.P * g.Q;
  return npq / WG_SLICES > WG_ROWS ? nnl_cdiv(npq, WG_SLICES) : WG_ROWS;
}

}  // namespace

extern "C" int nnl_gconv2d_fwd(const float* x, const float* w, const float* bias, float* y, int64_t N, int64_t H, int64_t W, int64_t C,
                               int64_t K, int64_t G, int R, int stride, int pad, int relu, void* stream) {
  GGeom g;
  if (int e = make_geom("gconv2d_fwd", N, H, W, C, K, G, R, stride, pad, &g)) return e;
  NNL_CHECK_ARG(x && w && y, "gconv2d_fwd: null pointer");
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_CONV_FWD, s, 2.0 * N * g.P * g.Q * K * R * R * g.Cg);
  const bool lds = g.Cg <= LDS_RED;
  const int GB = groups_per_block(g.Cg);
  const int HT = (TILE - 1) * stride + R;
  const size_t shm = lds ? (size_t)HT * HT * ((GB * g.Cg) | 1) * sizeof(float) : 0;
  const dim3 grid((unsigned)(nnl_cdiv(g.P, TILE) * nnl_cdiv(g.Q, TILE)), (unsigned)nnl_cdiv(G, GB), (unsigned)N);
  NNL_ROUTE("gconv_fwd<%s>", lds ? "lds" : "cache");
  if (lds)
    hipLaunchKernelGGL(gconv_fwd_kernel<true>, grid, dim3(256), shm, s, x, w, bias, y, g, GB, relu);
  else
    hipLaunchKernelGGL(gconv_fwd_kernel<false>, grid, dim3(256), 0, s, x, w, bias, y, g, GB, relu);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}

extern "C" int nnl_gconv2d_dgrad(const float* dy, const float* w, float* dx, int64_t N, int64_t H, int64_t W, int64_t C, int64_t K,
                                 int64_t G, int R, int stride, int pad, void* stream) {
  GGeom g;
  if (int e = make_geom("gconv2d_dgrad", N, H, W, C, K, G, R, stride, pad, &g)) return e;
  NNL_CHECK_ARG(dy && w && dx, "gconv2d_dgrad: null pointer");
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_CONV_DGRAD, s, 2.0 * N * g.P * g.Q * K * R * R * g.Cg);
  const bool lds = g.Kg <= LDS_RED;
  const int GB = groups_per_block(g.Kg);
  const int DT = (TILE - 1 + R - 1) / stride + 2;
  const size_t shm = lds ? (size_t)DT * DT * ((GB * g.Kg) | 1) * sizeof(float) : 0;
  const dim3 grid((unsigned)(nnl_cdiv(H, TILE) * nnl_cdiv(W, TILE)), (unsigned)nnl_cdiv(G, GB), (unsigned)N);
  NNL_ROUTE("gconv_dgrad<%s>", lds ? "lds" : "cache");
  if (lds)
    hipLaunchKernelGGL(gconv_dgrad_kernel<true>, grid, dim3(256), shm, s, dy, w, dx, g, GB);
  else
    hipLaunchKernelGGL(gconv_dgrad_kernel<false>, grid, dim3(256), 0, s, dy, w, dx, g, GB);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}

extern "C" size_t nnl_gconv2d_workspace_bytes(int64_t N, int64_t H, int64_t W, int64_t C, int64_t K, int64_t G, int R, int stride,
                                              int pad) {
  GGeom g;
  if (make_geom("gconv2d_workspace_bytes", N, H, W, C, K, G, R, stride, pad, &g)) return 0;
  const long slices = nnl_cdiv((long)g.N * g.P * g.Q, wgrad_rows(g));
  return slices > 1 ? (size_t)slices * K * R * R * g.Cg * sizeof(float) : 0;
}

extern "C" int nnl_gconv2d_wgrad(const float* x, const float* dy, float* dw, void* ws, size_t ws_bytes, int64_t N, int64_t H, int64_t W,
                                 int64_t C, int64_t K, int64_t G, int R, int stride, int pad, void* stream) {
  GGeom g;
  if (int e = make_geom("gconv2d_wgrad", N, H, W, C, K, G, R, stride, pad, &g)) return e;
  NNL_CHECK_ARG(x && dy && dw, "gconv2d_wgrad: null pointer");
  const long npq = (long)g.N * g.P * g.Q, rows = wgrad_rows(g), slices = nnl_cdiv(npq, rows);
  const long numel = (long)K * R * R * g.Cg;
  if (slices > 1 && (ws == nullptr || ws_bytes < (size_t)slices * numel * sizeof(float)))
    return nnl_set_error(NNL_ERR_WORKSPACE, "gconv2d_wgrad: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_CONV_WGRAD, s, 2.0 * npq * K * R * R * g.Cg);
  const long units = (long)G * ((g.Kg + 3) / 4) * R * R * g.Cg;
  NNL_ROUTE("gconv_wgrad@s%ld", slices);
  hipLaunchKernelGGL(gconv_wgrad_kernel, dim3((unsigned)nnl_cdiv(units, 256), (unsigned)slices), dim3(256), 0, s, x, dy,
                     slices > 1 ? (float*)ws : dw, g, units, npq, rows, numel);
  NNL_CHECK_LAUNCH();
  if (slices > 1) {
    hipLaunchKernelGGL(gconv_wgrad_reduce_kernel, dim3((unsigned)nnl_cdiv(numel, 256)), dim3(256), 0, s, (const float*)ws, dw, numel,
                       (int)slices);
    NNL_CHECK_LAUNCH();
  }
  return NNL_OK;
}
