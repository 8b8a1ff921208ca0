// K18 depthwise convolution (nn.Conv2d(C, C, R, groups=C); reference Applications/VisionModels/nasnet.py:93-107 SeparableConv2d), NHWC
// fp32, filter [C, 1, R, R] = the parameter as it is stored.  R in {3, 5, 7}, stride in {1, 2}, any C.
//
// There is no reduction over channels, so the layer is bound by its activation traffic (R = 7: 98 flop per 8 bytes moved); the kernels
// are about fetching every activation from memory about once, with channel-innermost 16-byte accesses:
//   forward  one workgroup = a TP x TQ tile of output pixels x a tile of 64 channels.  The filter tile ([R*R taps][64 channels]) and the
//            input patch of the tile ([(TP-1) stride + R][(TQ-1) stride + R][64]) are staged in LDS once, the optional input ReLU is
//            applied on that load, everything outside the image is staged as zero.  One thread owns one channel vector (V = 4
//            channels when C % 4 == 0, V = 1 otherwise) and walks over the tile's pixels; an accumulator runs over its taps in the
//            fixed order (r, s).
//   dgrad    gather: one workgroup = an 8 x 8 tile of INPUT pixels x 64 channels; the window of dy that the tile's taps reach is staged
//            in LDS; one thread sums, per input pixel and channel vector, over the taps whose output position exists, in (r, s) order;
//            with relu_in the result is gated by x > 0.
//   wgrad    one workgroup = (a tile of 64 channels, a slab of the flattened N*P*Q).  A lane owns one channel and all R*R taps, the four
//            waves take the slab's pixels round-robin; the four partials are added in wave order through LDS, a slab's sums go to its
//            own part of the workspace and a second launch adds the slabs in slab order.  One slab writes dw directly.
// Padding is asymmetric on purpose: tap (r, s) of output (p, q) reads x[p stride - pad_lo + r, q stride - pad_lo + s], and the caller
// states P and Q (the "pad top/left, convolve at stride 2, drop the first row and column" idiom of nasnet.py:152-167 folds into that).
// No atomics anywhere: two calls on the same inputs give the same bits.
#include "nnl_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int CT = 64;             // channels per workgroup
constexpr int DG_TILE = 8;         // dgrad: 8 x 8 input pixels per workgroup
constexpr int WG_ROWS = 256;       // fewest pixels per wgrad slab
constexpr int WG_SLABS = 256;      // most wgrad slabs
constexpr int LDS_LIMIT = 65536;   // static + dynamic LDS of one workgroup stays below the default limit

struct DGeom { int N, H, W, C, P, Q, R, stride, pad_lo; };

template <int V> struct Vec;
template <> struct Vec<1> { typedef float T; };
template <> struct Vec<4> { typedef f32x4 T; };

template <int V> __device__ __forceinline__ typename Vec<V>::T vzero();
template <> __device__ __forceinline__ float vzero<1>() { return 0.f; }
template <> __device__ __forceinline__ f32x4 vzero<4>() { return f32x4{0.f, 0.f, 0.f, 0.f}; }

__device__ __forceinline__ float vrelu(float v) { return fmaxf(v, 0.f); }
__device__ __forceinline__ f32x4 vrelu(f32x4 v) { return f32x4{fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f)}; }
__device__ __forceinline__ float vfma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ f32x4 vfma(f32x4 a, f32x4 b, f32x4 c) {
  return f32x4{__builtin_fmaf(a[0], b[0], c[0]), __builtin_fmaf(a[1], b[1], c[1]), __builtin_fmaf(a[2], b[2], c[2]),
               __builtin_fmaf(a[3], b[3], c[3])};
}
__device__ __forceinline__ float vgate(float g, float x) { return x > 0.f ? g : 0.f; }
__device__ __forceinline__ f32x4 vgate(f32x4 g, f32x4 x) {
  return f32x4{x[0] > 0.f ? g[0] : 0.f, x[1] > 0.f ? g[1] : 0.f, x[2] > 0.f ? g[2] : 0.f, x[3] > 0.f ? g[3] : 0.f};
}

// the filter tile of channels [c0, c0 + 64) as [tap][64]; channels beyond C are zero
__device__ __forceinline__ void stage_filter(const float* __restrict__ w, float* sw, int c0, int C, int RR) {
  for (int i = threadIdx.x; i < RR * CT; i += 256) {
    const int c = i / RR, t = i - c * RR;                         // consecutive threads read consecutive filter elements
    sw[t * CT + c] = c0 + c < C ? w[(long)(c0 + c) * RR + t] : 0.f;
  }
}

template <int V>
__global__ __launch_bounds__(256) void dwconv_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ bias, float* __restrict__ y, DGeom g, int TP, int TQ,
                                                         int relu_in) {
  typedef typename Vec<V>::T VT;
  constexpr int CL = CT / V;                                        // channel lanes
  constexpr int PL = 256 / CL;                                      // pixel lanes
  extern __shared__ float smem[];
  const int RR = g.R * g.R;
  float* sw = smem;                                                 // [RR][64]
  float* sx = smem + RR * CT;                                       // [HT][WT][64]
  const int tilesQ = (g.Q + TQ - 1) / TQ;
  const int p0 = (blockIdx.x / tilesQ) * TP, q0 = (blockIdx.x % tilesQ) * TQ;
  const int c0 = blockIdx.y * CT, n = blockIdx.z;
  const int HT = (TP - 1) * g.stride + g.R, WT = (TQ - 1) * g.stride + g.R;
  const int h0 = p0 * g.stride - g.pad_lo, w0 = q0 * g.stride - g.pad_lo;
  stage_filter(w, sw, c0, g.C, RR);
  for (int i = threadIdx.x; i < HT * WT * CL; i += 256) {
    const int cl = i % CL, pix = i / CL;
    const int h = h0 + pix / WT, ww = w0 + pix % WT, c = c0 + cl * V;
    VT v = vzero<V>();
    if ((unsigned)h < (unsigned)g.H && (unsigned)ww < (unsigned)g.W && c < g.C) {
      v = *reinterpret_cast<const VT*>(x + (((long)n * g.H + h) * g.W + ww) * g.C + c);
      if (relu_in) v = vrelu(v);
    }
    *reinterpret_cast<VT*>(sx + pix * CT + cl * V) = v;
  }
  __syncthreads();
  const int cl = threadIdx.x % CL, pl = threadIdx.x / CL;
  const int c = c0 + cl * V;
  if (c >= g.C) return;
  VT b = vzero<V>();
  if (bias != nullptr) b = *reinterpret_cast<const VT*>(bias + c);
  for (int pix = pl; pix < TP * TQ; pix += PL) {
    const int lp = pix / TQ, lq = pix - lp * TQ;
    const int p = p0 + lp, q = q0 + lq;
    if (p >= g.P || q >= g.Q) continue;
    VT acc = vzero<V>();
    for (int r = 0; r < g.R; ++r) {
      const float* xr = sx + ((lp * g.stride + r) * WT + lq * g.stride) * CT + cl * V;
      const float* wr = sw + r * g.R * CT + cl * V;
      for (int s = 0; s < g.R; ++s)
        acc = vfma(*reinterpret_cast<const VT*>(xr + s * CT), *reinterpret_cast<const VT*>(wr + s * CT), acc);
    }
    acc += b;
    *reinterpret_cast<VT*>(y + (((long)n * g.P + p) * g.Q + q) * g.C + c) = acc;
  }
}

// dx[n,h,w,c] = sum_{r,s} dy[n,p,q,c] * w[c,r,s] over the taps with p stride = h + pad_lo - r, q stride = w + pad_lo - s, 0 <= p < P, 0 <= q < Q
template <int V>
__global__ __launch_bounds__(256) void dwconv_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                           const float* __restrict__ x, float* __restrict__ dx, DGeom g, int DT,
                                                           int relu_in) {
  typedef typename Vec<V>::T VT;
  constexpr int CL = CT / V;
  constexpr int PL = 256 / CL;
  extern __shared__ float smem[];
  const int RR = g.R * g.R;
  float* sw = smem;                                                 // [RR][64]
  float* sd = smem + RR * CT;                                       // [DT][DT][64]
  const int tilesW = (g.W + DG_TILE - 1) / DG_TILE;
  const int h0 = (blockIdx.x / tilesW) * DG_TILE, w0 = (blockIdx.x % tilesW) * DG_TILE;
  const int c0 = blockIdx.y * CT, n = blockIdx.z;
  // a tap of pixel h needs p stride = h + pad_lo - r: p >= pb, and p <= (h0 + 7 + pad_lo) / stride <= pb + DT - 1
  const int tlo_h = h0 + g.pad_lo - g.R + 1, tlo_w = w0 + g.pad_lo - g.R + 1;
  const int pb = tlo_h > 0 ? (tlo_h + g.stride - 1) / g.stride : 0, qb = tlo_w > 0 ? (tlo_w + g.stride - 1) / g.stride : 0;
  stage_filter(w, sw, c0, g.C, RR);
  for (int i = threadIdx.x; i < DT * DT * CL; i += 256) {
    const int cl = i % CL, pix = i / CL;
    const int p = pb + pix / DT, q = qb + pix % DT, c = c0 + cl * V;
    VT v = vzero<V>();
    if (p < g.P && q < g.Q && c < g.C) v = *reinterpret_cast<const VT*>(dy + (((long)n * g.P + p) * g.Q + q) * g.C + c);
    *reinterpret_cast<VT*>(sd + pix * CT + cl * V) = v;
  }
  __syncthreads();
  const int cl = threadIdx.x % CL, pl = threadIdx.x / CL;
  const int c = c0 + cl * V;
  if (c >= g.C) return;
  for (int pix = pl; pix < DG_TILE * DG_TILE; pix += PL) {
    const int h = h0 + pix / DG_TILE, ww = w0 + pix % DG_TILE;
    if (h >= g.H || ww >= g.W) continue;
    VT acc = vzero<V>();
    for (int r = 0; r < g.R; ++r) {
      const int th = h + g.pad_lo - r;
      if (th < 0) break;                                            // (th only falls with r)
      const int p = th / g.stride;
      if (th - p * g.stride != 0 || p >= g.P) continue;
      for (int s = 0; s < g.R; ++s) {
        const int tw = ww + g.pad_lo - s;
        if (tw < 0) break;
        const int q = tw / g.stride;
        if (tw - q * g.stride != 0 || q >= g.Q) continue;
        acc = vfma(*reinterpret_cast<const VT*>(sd + ((p - pb) * DT + (q - qb)) * CT + cl * V),
                   *reinterpret_cast<const VT*>(sw + (r * g.R + s) * CT + cl * V), acc);
      }
    }
    const long o = (((long)n * g.H + h) * g.W + ww) * g.C + c;
    if (relu_in) acc = vgate(acc, *reinterpret_cast<const VT*>(x + o));
    *reinterpret_cast<VT*>(dx + o) = acc;
  }
}

// one lane = one channel x all R*R taps; wave v of the workgroup takes the pixels m0 + v, m0 + v + 4, ... of the slab [m0, m1)
template <int R>
__global__ __launch_bounds__(256) void dwconv_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                           float* __restrict__ out, DGeom g, long npq, long rows, int relu_in) {
  constexpr int RR = R * R;
  __shared__ float red[3][RR][CT];                                  // the partials of waves 1 .. 3
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * CT + lane;
  const bool live = c < g.C;
  const long m0 = (long)blockIdx.y * rows, m1 = min(npq, m0 + rows);
  float acc[RR];
#pragma unroll
  for (int t = 0; t < RR; ++t) acc[t] = 0.f;
  if (live)
    for (long m = m0 + wave; m < m1; m += 4) {
      const int q = (int)(m % g.Q), p = (int)((m / g.Q) % g.P), n = (int)(m / ((long)g.Q * g.P));
      const float d = dy[m * g.C + c];
      const int hb = p * g.stride - g.pad_lo, wb = q * g.stride - g.pad_lo;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int h = hb + r;
        if ((unsigned)h >= (unsigned)g.H) continue;
        const float* xr = x + ((long)n * g.H + h) * g.W * g.C + c;
#pragma unroll
        for (int s = 0; s < R; ++s) {
          const int ww = wb + s;
          if ((unsigned)ww >= (unsigned)g.W) continue;
          float xv = xr[(long)ww * g.C];
          if (relu_in) xv = fmaxf(xv, 0.f);
          acc[r * R + s] = __builtin_fmaf(d, xv, acc[r * R + s]);
        }
      }
    }
  if (wave > 0) {
#pragma unroll
    for (int t = 0; t < RR; ++t) red[wave - 1][t][lane] = acc[t];
  }
  __syncthreads();
  if (wave == 0 && live) {
    float* o = out + ((long)blockIdx.y * g.C + c) * RR;
#pragma unroll
    for (int t = 0; t < RR; ++t) o[t] = ((acc[t] + red[0][t][lane]) + red[1][t][lane]) + red[2][t][lane];     // wave order: fixed
  }
}

__global__ __launch_bounds__(256) void dwconv_wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw, long numel,
                                                                  int slabs) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= numel) return;
  float a = part[i];
  for (int sl = 1; sl < slabs; ++sl) a += part[(long)sl * numel + i];       // slab order: fixed
  dw[i] = a;
}

int make_geom(const char* who, int64_t N, int64_t H, int64_t W, int64_t C, int64_t P, int64_t Q, int R, int stride, int pad_lo, DGeom* g) {
  NNL_CHECK_ARG(N > 0 && H > 0 && W > 0 && C > 0, "%s: sizes must be positive", who);
  NNL_CHECK_ARG(R == 3 || R == 5 || R == 7, "%s: kernel_size R = %d (3, 5 or 7)", who, R);
  NNL_CHECK_ARG(stride == 1 || stride == 2, "%s: stride = %d (1 or 2)", who, stride);
  NNL_CHECK_ARG(pad_lo >= 0 && pad_lo <= R - 1, "%s: pad_lo = %d (0 .. R - 1)", who, pad_lo);
  NNL_CHECK_ARG(P >= 1 && (P - 1) * stride - pad_lo <= H - 1, "%s: P = %ld: every window must touch the %ld rows", who, (long)P, (long)H);
  NNL_CHECK_ARG(Q >= 1 && (Q - 1) * stride - pad_lo <= W - 1, "%s: Q = %ld: every window must touch the %ld columns", who, (long)Q, (long)W);
  NNL_CHECK_ARG(N < 65536 && C < 65536L * CT && N * H * W * C < (1L << 31) && N * P * Q * C < (1L << 31), "%s: tensor too large", who);
  *g = DGeom{(int)N, (int)H, (int)W, (int)C, (int)P, (int)Q, R, stride, pad_lo};
  return NNL_OK;
}

// forward tile: 8 x 8 output pixels at stride 1; at stride 2 the largest of 4 x 8, 4 x 4 whose patch and filter fit LDS
void fwd_tile(const DGeom& g, int* TP, int* TQ, size_t* shm) {
  const int cand[3][2] = {{8, 8}, {4, 8}, {4, 4}};
  for (int i = 0; i < 3; ++i) {
    *TP = cand[i][0]; *TQ = cand[i][1];
    const int HT = (*TP - 1) * g.stride + g.R, WT = (*TQ - 1) * g.stride + g.R;
    *shm = ((size_t)g.R * g.R + (size_t)HT * WT) * CT * sizeof(float);
    if (*shm <= (size_t)LDS_LIMIT) return;
  }
}

long wgrad_rows(const DGeom& g) {
  const long npq = (long)g.N * g.P * g.Q;
  return npq / WG_SLABS > WG_ROWS ? nnl_cdiv(npq, WG_SLABS) : WG_ROWS;
}

}  // namespace

extern "C" int nnl_dwconv2d_fwd(const float* x, const float* w, const float* bias, float* y, int64_t N, int64_t H, int64_t W, int64_t C,
                                int64_t P, int64_t Q, int R, int stride, int pad_lo, int relu_in, void* stream) {
  DGeom g;
  if (int e = make_geom("dwconv2d_fwd", N, H, W, C, P, Q, R, stride, pad_lo, &g)) return e;
  NNL_CHECK_ARG(x && w && y, "dwconv2d_fwd: null pointer");
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_CONV_FWD, s, 2.0 * N * P * Q * C * R * R);
  int TP, TQ;
  size_t shm;
  fwd_tile(g, &TP, &TQ, &shm);
  const dim3 grid((unsigned)(nnl_cdiv(P, TP) * nnl_cdiv(Q, TQ)), (unsigned)nnl_cdiv(C, CT), (unsigned)N);
  const bool vec = C % 4 == 0;
  NNL_ROUTE("dwconv_fwd<%s>:%dx%d", vec ? "v4" : "v1", TP, TQ);
  if (vec)
    hipLaunchKernelGGL(dwconv_fwd_kernel<4>, grid, dim3(256), shm, s, x, w, bias, y, g, TP, TQ, relu_in);
  else
    hipLaunchKernelGGL(dwconv_fwd_kernel<1>, grid, dim3(256), shm, s, x, w, bias, y, g, TP, TQ, relu_in);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}

extern "C" int nnl_dwconv2d_dgrad(const float* dy, const float* w, const float* x, float* dx, int64_t N, int64_t H, int64_t W, int64_t C,
                                  int64_t P, int64_t Q, int R, int stride, int pad_lo, int relu_in, void* stream) {
  DGeom g;
  if (int e = make_geom("dwconv2d_dgrad", N, H, W, C, P, Q, R, stride, pad_lo, &g)) return e;
  NNL_CHECK_ARG(dy && w && dx, "dwconv2d_dgrad: null pointer");
  NNL_CHECK_ARG(!relu_in || x, "dwconv2d_dgrad: relu_in needs x");
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_CONV_DGRAD, s, 2.0 * N * P * Q * C * R * R);
  const int DT = (DG_TILE + R - 2) / stride + 1;
  const size_t shm = ((size_t)R * R + (size_t)DT * DT) * CT * sizeof(float);
  const dim3 grid((unsigned)(nnl_cdiv(H, DG_TILE) * nnl_cdiv(W, DG_TILE)), (unsigned)nnl_cdiv(C, CT), (unsigned)N);
  const bool vec = C % 4 == 0;
  NNL_ROUTE("dwconv_dgrad<%s>", vec ? "v4" : "v1");
  if (vec)
    hipLaunchKernelGGL(dwconv_dgrad_kernel<4>, grid, dim3(256), shm, s, dy, w, x, dx, g, DT, relu_in);
  else
    hipLaunchKernelGGL(dwconv_dgrad_kernel<1>, grid, dim3(256), shm, s, dy, w, x, dx, g, DT, relu_in);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}

extern "C" size_t nnl_dwconv2d_wgrad_workspace_bytes(int64_t N, int64_t H, int64_t W, int64_t C, int64_t P, int64_t Q, int R, int stride,
                                                     int pad_lo) {
  DGeom g;
  if (make_geom("dwconv2d_wgrad_workspace_bytes", N, H, W, C, P, Q, R, stride, pad_lo, &g)) return 0;
  const long slabs = nnl_cdiv((long)g.N * g.P * g.Q, wgrad_rows(g));
  return slabs > 1 ? (size_t)slabs * C * R * R * sizeof(float) : 0;
}

extern "C" int nnl_dwconv2d_wgrad(const float* x, const float* dy, float* dw, void* ws, size_t ws_bytes, int64_t N, int64_t H, int64_t W,
                                  int64_t C, int64_t P, int64_t Q, int R, int stride, int pad_lo, int relu_in, void* stream) {
  DGeom g;
  if (int e = make_geom("dwconv2d_wgrad", N, H, W, C, P, Q, R, stride, pad_lo, &g)) return e;
  NNL_CHECK_ARG(x && dy && dw, "dwconv2d_wgrad: null pointer");
  const long npq = (long)g.N * g.P * g.Q, rows = wgrad_rows(g), slabs = nnl_cdiv(npq, rows);
  const long numel = (long)C * R * R;
  if (slabs > 1 && (ws == nullptr || ws_bytes < (size_t)slabs * numel * sizeof(float)))
    return nnl_set_error(NNL_ERR_WORKSPACE, "dwconv2d_wgrad: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_CONV_WGRAD, s, 2.0 * npq * C * R * R);
  float* out = slabs > 1 ? (float*)ws : dw;
  const dim3 grid((unsigned)nnl_cdiv(C, CT), (unsigned)slabs);
  NNL_ROUTE("dwconv_wgrad<%d>@s%ld", R, slabs);
  if (R == 3)
    hipLaunchKernelGGL(dwconv_wgrad_kernel<3>, grid, dim3(256), 0, s, x, dy, out, g, npq, rows, relu_in);
  else if (R == 5)
    hipLaunchKernelGGL(dwconv_wgrad_kernel<5>, grid, dim3(256), 0, s, x, dy, out, g, npq, rows, relu_in);
  else
    hipLaunchKernelGGL(dwconv_wgrad_kernel<7>, grid, dim3(256), 0, s, x, dy, out, g, npq, rows, relu_in);
  NNL_CHECK_LAUNCH();
  if (slabs > 1) {
    hipLaunchKernelGGL(dwconv_wgrad_reduce_kernel, dim3((unsigned)nnl_cdiv(numel, 256)), dim3(256), 0, s, (const float*)ws, dw, numel,
                       (int)slabs);
    NNL_CHECK_LAUNCH();
  }
  return NNL_OK;
}
