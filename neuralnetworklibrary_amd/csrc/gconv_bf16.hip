// K24 opt-in bf16 matrix-core GROUPED convolutions: the 3x3 of the SENet / SE-ResNeXt / ResNeXt bottlenecks (nn.Conv2d(groups = G), reference
// Applications/VisionModels/senet.py:178-180, 205-206, 229-230 and resnext.py's bottleneck) with bf16 OPERANDS and fp32 accumulation.
// Semantics as conv_bf16.hip: every tensor stays fp32 in memory (NHWC activations, the filter [K, R, R, Cg] in the parameter's own
// channels_last memory), an operand is rounded to bf16 (nearest even, v_cvt_pk_bf16_f32) on its way into LDS, the products run on
// v_mfma_f32_16x16x32_bf16, sums and epilogue are fp32.  A bf16 x bf16 product is exact in fp32.
// Domain (nnl_gconv2d_bf16_supported): R in {1, 3}, stride 1 or 2, pad <= R / 2, Cg and Kg each in {4, 8, 16, 32}, any G, N, H, W.
//
// Lane mapping of the instruction (tools/mfma16x16x32_probe.hip): lane l = (i = l % 16, kq = l / 16) supplies A[row i][k = 8 kq .. 8 kq + 7]
// and B[the same k][col i] as ONE 16-byte fragment each and holds D[row 4 kq + v][col i] in accumulator element v.
//
// At Cg <= 8 these layers are bound by activation traffic, not arithmetic, so the MFMA is spent wastefully: ONE data path serves every
// Cg / Kg, with block-diagonal filter tiles that are mostly zeros at narrow groups.
//
// forward / dgrad (gconv_bf16_kernel<NT, DGRAD>, ONE template): rows = pixels (forward: outputs, dgrad: inputs), reduction = (tap, a SPAN of
//   32 consecutive reduction channels = 32 / RED whole groups; RED = Cg forward, Kg dgrad), columns = the COLS channels (Kg / Cg) of those
//   groups, in tiles of 16, at most NT <= 4 tiles per workgroup (a span with more columns is cut into column chunks: grid.y).
//   filter: staged ONCE per workgroup from the plain fp32 filter (no pack launch, no transposed copy: the dgrad reads the same memory with
//     the roles of c and k exchanged) as block-diagonal [tap][column tile][16 columns][32 k] bf16 tiles, zero where a k row's group is
//     not the column's group.  The workgroup then strides over pixel tiles (blockIdx.x).
//   activations: a pixel tile is 8 x 8; its halo of the span (forward: (7 stride + R)^2 input pixels, dgrad: the window of dy its taps reach,
//     at most (8 + R - 1)^2 at stride 1 and 5^2 at stride 2) is staged once, as bf16, [halo pixel][32 channels] = 64 B per pixel, plus one
//     pixel of zeros: every activation is rounded once and read from memory once per tile, and a tap is a different LDS address of the same
//     halo.  A dgrad tap that fails the stride predicate reads the zero pixel (at stride 2 three of four taps; accepted: traffic-bound).
//   MFMA: the FILTER fragment is the A operand and the PIXEL fragment the B operand, so a lane ends up with 4 consecutive channels of ITS
//     pixel: the epilogue (bias, ReLU) is one 16-byte store per lane and tile, 4 lanes cover 64 contiguous bytes.  Wave w owns tile rows
//     2 w, 2 w + 1.  LDS: a 64-byte row is 4 chunks of 16 B, chunk' = chunk ^ ((row >> 2) & 3) (as conv_bf16.hip): the ds_read_b128 of 16
//     consecutive rows are conflict-free.
// wgrad (gconv_bf16_wgrad_kernel<R>): per 16 filters kt the groups they belong to span max(1, 16 / Kg) Cg input channels, cut into tiles of
//   16: a wave owns one (kt, channel tile) and the accumulators of ALL R^2 taps (9 x 4 VGPRs) over the pixels of its slab, 32 per k-step.
//   Per step it loads 32 pixels x 16 channels of dy once and of x at each tap (the taps of a step overlap: they meet in the cache, memory is
//   read once), 2 pixels x 4 channels per lane, and transposes them pixel-major through LDS as bf16 ([channel][32 pixels] planes, the
//   swizzle above), where a lane's fragment is 8 pixels of one channel.  Only the own-group elements of the 16 x 16 block are stored; the
//   rest are computed and dropped.  Pixels are cut into slabs (grid.y); the partial [K, R, R, Cg] slabs go to a workspace and
//   gconv_bf16_fold_kernel adds them in slab order; one slab writes dw directly.
// No atomics, no cooperative launch: two calls on the same inputs give the same bits.
#include "nnl_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int SPAN = 32;         // reduction channels of a workgroup = the k of one MFMA
constexpr int TILE = 8;          // pixel tile: 8 x 8, 16 pixels per wave
constexpr int MAX_NT = 4;        // most 16-column tiles per workgroup
constexpr int FD_BLOCKS = 2048;  // workgroups the forward / dgrad grid aims at
constexpr int WG_STEP = 32;      // wgrad: pixels per k-step
constexpr int WG_ROWS = 256;     // fewest pixels per wgrad slab (a multiple of WG_STEP)
constexpr int WG_SLABS = 256;    // most wgrad slabs
constexpr int WG_GRID = 1024;    // slabs are added until the grid has about this many workgroups

struct GGeom { int N, H, W, C, K, G, R, stride, pad, P, Q, Cg, Kg; };

__device__ __forceinline__ unsigned pk_bf16(float a, float b) {
  bf16x2 t = {(__bf16)a, (__bf16)b};           // v_cvt_pk_bf16_f32: round to nearest even; a is the low half
  return __builtin_bit_cast(unsigned, t);
}

__device__ __forceinline__ u32x4 pk_bf16x8(const f32x4& a, const f32x4& b) {
  return u32x4{pk_bf16(a[0], a[1]), pk_bf16(a[2], a[3]), pk_bf16(b[0], b[1]), pk_bf16(b[2], b[3])};
}

// byte offset of 16-byte chunk `chunk` of 64-byte row `row`
__device__ __forceinline__ int swz(int row, int chunk) { return row * 64 + ((chunk ^ ((row >> 2) & 3)) << 4); }

template <int NT, bool DGRAD>
__global__ __launch_bounds__(256) void gconv_bf16_kernel(const float* __restrict__ src, const float* __restrict__ w,
                                                         const float* __restrict__ bias, float* __restrict__ out, GGeom g, int HT, int tiles,
                                                         int chunks, int relu) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];      // [R R][NT][16][64 B] filter tiles | [HT HT + 1][64 B] halo
  const int RR = g.R * g.R, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, kq = lane >> 4;
  unsigned char* sB = smem;
  unsigned char* sH = smem + RR * NT * 1024;
  const int RED = DGRAD ? g.Kg : g.Cg, COLS = DGRAD ? g.Cg : g.Kg;
  const int SA = DGRAD ? g.P : g.H, SB = DGRAD ? g.Q : g.W, SC = DGRAD ? g.K : g.C;      // the operand tensor [N, SA, SB, SC]
  const int RA = DGRAD ? g.H : g.P, RB = DGRAD ? g.W : g.Q, OC = DGRAD ? g.C : g.K;      // the rows [N, RA, RB] and their OC channels
  const int span = blockIdx.y / chunks, chunk = blockIdx.y - span * chunks;
  const int r0 = span * SPAN;                                                            // first reduction channel
  const int span_col0 = (r0 / RED) * COLS, col0 = span_col0 + chunk * NT * 16;           // first column of the span / of this workgroup
  const int col_end = min(min(OC, span_col0 + (SPAN / RED) * COLS), col0 + NT * 16);     // columns this workgroup stores
  // ---- the block-diagonal filter tiles: 8 consecutive k of one column per item
  for (int i = tid; i < RR * NT * 64; i += 256) {
    const int kc = i & 3, col = (i >> 2) & 15, ct = (i >> 6) % NT, tap = i / (64 * NT);
    const int cc = col0 + ct * 16 + col;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int rc = r0 + kc * 8 + j;
      v[j] = 0.f;
      if (cc < col_end && rc < SC && rc / RED == cc / COLS)
        v[j] = DGRAD ? w[((long)rc * RR + tap) * g.Cg + cc % g.Cg] : w[((long)cc * RR + tap) * g.Cg + rc % g.Cg];
    }
    *reinterpret_cast<u32x4*>(sB + (tap * NT + ct) * 1024 + swz(col, kc)) =
        u32x4{pk_bf16(v[0], v[1]), pk_bf16(v[2], v[3]), pk_bf16(v[4], v[5]), pk_bf16(v[6], v[7])};
  }
  const int ZP = HT * HT;                                                                // the pixel of zeros
  if (tid < 4) *reinterpret_cast<u32x4*>(sH + ZP * 64 + tid * 16) = u32x4{0u, 0u, 0u, 0u};
  const int tA = (RA + TILE - 1) / TILE, tB = (RB + TILE - 1) / TILE, sh = g.stride - 1;
  const int la = 2 * wave + (li >> 3), lb = li & 7;                                      // the lane's pixel of the tile
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int tb = t % tB, ta = (t / tB) % tA, n = t / (tB * tA);
    const int a0 = ta * TILE, b0 = tb * TILE;
    int oa, ob;                                                                          // the halo's origin in the operand raster
    if (!DGRAD) {
      oa = a0 * g.stride - g.pad;
      ob = b0 * g.stride - g.pad;
    } else {                                                                             // ceil((a0 + pad - (R - 1)) / stride), a0 even
      oa = (a0 + g.pad - g.R + 1 + sh) >> sh;
      ob = (b0 + g.pad - g.R + 1 + sh) >> sh;
    }
    __syncthreads();                                                                     // the previous tile's reads are done
    for (int i = tid; i < ZP * 4; i += 256) {
      const int kc = i & 3, hp = i >> 2, hb = hp % HT, ha = hp / HT;
      const int sa = oa + ha, sb = ob + hb, ch = r0 + kc * 8;
      f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = {0.f, 0.f, 0.f, 0.f};
      if ((unsigned)sa < (unsigned)SA && (unsigned)sb < (unsigned)SB) {
        const float* p = src + (((long)n * SA + sa) * SB + sb) * SC + ch;
        if (ch + 4 <= SC) v0 = *reinterpret_cast<const f32x4*>(p);
        if (ch + 8 <= SC) v1 = *reinterpret_cast<const f32x4*>(p + 4);
      }
      *reinterpret_cast<u32x4*>(sH + swz(hp, kc)) = pk_bf16x8(v0, v1);
    }
    __syncthreads();
    f32x4 acc[NT];
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    int r = 0, s = 0;
    for (int tap = 0; tap < RR; ++tap) {
      int hp;
      if (!DGRAD) {
        hp = (la * g.stride + r) * HT + lb * g.stride + s;
      } else {
        const int th = a0 + la + g.pad - r, tw = b0 + lb + g.pad - s;                    // the stride predicate; below the origin never
        hp = ((th | tw) & sh) == 0 ? ((th >> sh) - oa) * HT + (tw >> sh) - ob : ZP;
      }
      const bf16x8 px = *reinterpret_cast<const bf16x8*>(sH + swz(hp, kq));
      const unsigned char* bp = sB + tap * NT * 1024 + swz(li, kq);
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) {
        const bf16x8 fl = *reinterpret_cast<const bf16x8*>(bp + ct * 1024);
        acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fl, px, acc[ct], 0, 0, 0);     // D[channel 4 kq + v][pixel li]
      }
      if (++s == g.R) { s = 0; ++r; }
    }
    const int a = a0 + la, b = b0 + lb;
    if (a < RA && b < RB) {
      float* o = out + (((long)n * RA + a) * RB + b) * OC;
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) {
        const int ch = col0 + ct * 16 + 4 * kq;
        if (ch >= col_end) continue;
        f32x4 v = acc[ct];
        if (bias != nullptr) v += *reinterpret_cast<const f32x4*>(bias + ch);
        if (relu) v = f32x4{fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f)};
        *reinterpret_cast<f32x4*>(o + ch) = v;
      }
    }
  }
}

// one wave = (16 filters kt, 16-channel tile j of the groups they belong to) x all R R taps over the pixels [blockIdx.y rows, + rows)
template <int R>
__global__ __launch_bounds__(256) void gconv_bf16_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ out,
                                                               GGeom g, int units, int nct, long npq, long rows, long numel) {
  constexpr int RR = R * R;
  __shared__ __attribute__((aligned(16))) unsigned char smem[4 * (RR + 1) * 1024];       // per wave: the dy plane, then one x plane per tap
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, kq = lane >> 4;
  unsigned char* pl = smem + wave * (RR + 1) * 1024;
  const int unit = blockIdx.x * 4 + wave;
  const bool live = unit < units;                                                        // (a dead wave still meets the barriers)
  const int j = unit % nct, kt = unit / nct;
  const int k0 = kt * 16, c0 = (k0 / g.Kg) * g.Cg + 16 * j;
  const int cq = lane & 3, pq = lane >> 2;                                               // staging share: 4 channels of pixels 2 pq, 2 pq + 1
  const bool kok = live && k0 + 4 * cq + 4 <= g.K, cok = live && c0 + 4 * cq + 4 <= g.C;
  const long m0 = (long)blockIdx.y * rows, m1 = min(npq, m0 + rows);
  f32x4 acc[RR];
#pragma unroll
  for (int t = 0; t < RR; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (long mc = m0; mc < m1; mc += WG_STEP) {
    f32x4 rg[2], rx[RR][2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const long m = mc + 2 * pq + e;
      rg[e] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < RR; ++t) rx[t][e] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (m < m1) {
        const int q = (int)(m % g.Q), p = (int)((m / g.Q) % g.P), n = (int)(m / ((long)g.Q * g.P));
        if (kok) rg[e] = *reinterpret_cast<const f32x4*>(dy + m * g.K + k0 + 4 * cq);
#pragma unroll
        for (int t = 0; t < RR; ++t) {
          const int h = p * g.stride - g.pad + t / R, ww = q * g.stride - g.pad + t % R;
          if (cok && (unsigned)h < (unsigned)g.H && (unsigned)ww < (unsigned)g.W)
            rx[t][e] = *reinterpret_cast<const f32x4*>(x + (((long)n * g.H + h) * g.W + ww) * g.C + c0 + 4 * cq);
        }
      }
    }
    __syncthreads();                                                                     // the previous step's fragments are read
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int off = swz(4 * cq + jj, pq >> 2) + (pq & 3) * 4;                          // [channel][pixel]: this lane's pixel pair
      *reinterpret_cast<unsigned*>(pl + off) = pk_bf16(rg[0][jj], rg[1][jj]);
#pragma unroll
      for (int t = 0; t < RR; ++t) *reinterpret_cast<unsigned*>(pl + (1 + t) * 1024 + off) = pk_bf16(rx[t][0][jj], rx[t][1][jj]);
    }
    __syncthreads();
    const bf16x8 a = *reinterpret_cast<const bf16x8*>(pl + swz(li, kq));                 // filter li, pixels 8 kq .. 8 kq + 7
#pragma unroll
    for (int t = 0; t < RR; ++t) {
      const bf16x8 b = *reinterpret_cast<const bf16x8*>(pl + (1 + t) * 1024 + swz(li, kq));
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[t], 0, 0, 0);           // D[filter 4 kq + v][channel li]
    }
  }
  const int c = c0 + li;
  if (!live || c >= g.C) return;                                                         // (after the last barrier)
  float* o = out + (long)blockIdx.y * numel;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int k = k0 + 4 * kq + v;
    if (k >= g.K || k / g.Kg != c / g.Cg) continue;                                      // only the own-group elements exist in dw
#pragma unroll
    for (int t = 0; t < RR; ++t) o[((long)k * RR + t) * g.Cg + c % g.Cg] = acc[t][v];
  }
}

__global__ __launch_bounds__(256) void gconv_bf16_fold_kernel(const float* __restrict__ part, float* __restrict__ dw, long numel, int slabs) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= numel) return;
  float a = part[i];
  for (int sl = 1; sl < slabs; ++sl) a += part[(long)sl * numel + i];                    // slab order: fixed
  dw[i] = a;
}

inline bool lane_width(int64_t v) { return v == 4 || v == 8 || v == 16 || v == 32; }

// the domain; nothing is reported through nnl_last_error when `who` is null (the plain query)
int make_geom(const char* who, int64_t N, int64_t H, int64_t W, int64_t C, int64_t K, int64_t G, int R, int stride, int pad, GGeom* g) {
#define GBF16_DOMAIN(cond, ...)                                                                       \
  do {                                                                                                \
    if (!(cond)) return who ? nnl_set_error(NNL_ERR_INVALID_ARG, __VA_ARGS__) : NNL_ERR_INVALID_ARG;  \
  } while (0)
  const char* name = who ? who : "";
  GBF16_DOMAIN(N > 0 && H > 0 && W > 0 && C > 0 && K > 0 && G > 0, "%s: sizes must be positive", name);
  GBF16_DOMAIN(C % G == 0 && K % G == 0, "%s: groups = %ld must divide C = %ld and K = %ld", name, (long)G, (long)C, (long)K);
  GBF16_DOMAIN(lane_width(C / G) && lane_width(K / G), "%s: channels per group %ld in, %ld out (each 4, 8, 16 or 32)", name, (long)(C / G),
               (long)(K / G));
  GBF16_DOMAIN(R == 1 || R == 3, "%s: kernel_size R = %d (1 or 3)", name, R);
  GBF16_DOMAIN(stride == 1 || stride == 2, "%s: stride = %d (1 or 2)", name, stride);
  GBF16_DOMAIN(pad >= 0 && pad <= R / 2, "%s: padding = %d (0 .. R / 2)", name, pad);
  GBF16_DOMAIN(H + 2 * pad >= R && W + 2 * pad >= R, "%s: filter larger than the padded input", name);
  const int64_t P = (H + 2 * pad - R) / stride + 1, Q = (W + 2 * pad - R) / stride + 1, lim = (int64_t)1 << 31;
  GBF16_DOMAIN(N < 65536 && C < 65536 * 4 && K < 65536 * 4 && N * H * W * C < lim && N * P * Q * K < lim && K * R * R * (C / G) < lim,
               "%s: tensor too large", name);
#undef GBF16_DOMAIN
  *g = GGeom{(int)N, (int)H, (int)W, (int)C, (int)K, (int)G, R, stride, pad, (int)P, (int)Q, (int)(C / G), (int)(K / G)};
  return NNL_OK;
}

// forward (DGRAD = false: src = x, out = y) and dgrad (src = dy, out = dx, no bias, no ReLU)
template <int NT, bool DGRAD>
void launch_t(const float* src, const float* w, const float* bias, float* out, const GGeom& g, int chunks, int relu, hipStream_t s) {
  const int HT = !DGRAD ? (TILE - 1) * g.stride + g.R : (g.stride == 1 ? TILE + g.R - 1 : 5);
  const int RA = DGRAD ? g.H : g.P, RB = DGRAD ? g.W : g.Q, SC = DGRAD ? g.K : g.C;
  const long tiles = (long)g.N * nnl_cdiv(RA, TILE) * nnl_cdiv(RB, TILE);                // < 2^31: fewer than pixels
  const long gy = nnl_cdiv(SC, SPAN) * chunks;                                           // < 65536: C, K < 2^18 and chunks <= 4
  const long per = nnl_cdiv(tiles, gy < FD_BLOCKS ? FD_BLOCKS / gy : 1);                 // tiles per workgroup: the filter is staged once for them
  const dim3 grid((unsigned)nnl_cdiv(tiles, per), (unsigned)gy);
  const size_t shm = (size_t)g.R * g.R * NT * 1024 + (size_t)(HT * HT + 1) * 64;         // <= 36 KB + 18.1 KB
  hipLaunchKernelGGL((gconv_bf16_kernel<NT, DGRAD>), grid, dim3(256), shm, s, src, w, bias, out, g, HT, (int)tiles, chunks, relu);
}

template <bool DGRAD>
void launch(const float* src, const float* w, const float* bias, float* out, const GGeom& g, int relu, hipStream_t s) {
  const int red = DGRAD ? g.Kg : g.Cg, cols = DGRAD ? g.Cg : g.Kg;
  const int ncols = (SPAN / red) * cols;                                                 // 4 .. 256, a power of two
  const int nt = ncols <= 16 ? 1 : (ncols == 32 ? 2 : MAX_NT), chunks = ncols > MAX_NT * 16 ? ncols / (MAX_NT * 16) : 1;
  if (nt == 1) launch_t<1, DGRAD>(src, w, bias, out, g, chunks, relu, s);
  else if (nt == 2) launch_t<2, DGRAD>(src, w, bias, out, g, chunks, relu, s);
  else launch_t<MAX_NT, DGRAD>(src, w, bias, out, g, chunks, relu, s);
}

int wgrad_ctiles(const GGeom& g) { return (int)nnl_cdiv((long)g.Cg * (g.Kg >= 16 ? 1 : 16 / g.Kg), 16); }

// pixels per wgrad slab: a multiple of WG_STEP, at least WG_ROWS, and no more slabs than fill the grid or than WG_SLABS
long wgrad_rows(const GGeom& g) {
  const long npq = (long)g.N * g.P * g.Q, wgs = nnl_cdiv(nnl_cdiv(g.K, 16) * wgrad_ctiles(g), 4);
  long slabs = WG_GRID / wgs;
  slabs = slabs < 1 ? 1 : (slabs > WG_SLABS ? WG_SLABS : slabs);
  const long rows = nnl_cdiv(nnl_cdiv(npq, slabs), WG_STEP) * WG_STEP;
  return rows > WG_ROWS ? rows : WG_ROWS;
}

}  // namespace

extern "C" int nnl_gconv2d_bf16_supported(int64_t N, int64_t H, int64_t W, int64_t C, int64_t K, int64_t G, int R, int stride, int pad) {
  GGeom g;
  return make_geom(nullptr, N, H, W, C, K, G, R, stride, pad, &g) == NNL_OK ? 1 : 0;
}

extern "C" int nnl_gconv2d_bf16_fwd(const float* x, const float* w, const float* bias, float* y, int64_t N, int64_t H, int64_t W, int64_t C,
                                    int64_t K, int64_t G, int R, int stride, int pad, int relu, void* stream) {
  GGeom g;
  if (int e = make_geom("gconv2d_bf16_fwd", N, H, W, C, K, G, R, stride, pad, &g)) return e;
  NNL_CHECK_ARG(x && w && y, "gconv2d_bf16_fwd: null pointer");
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_CONV_FWD, s, 2.0 * N * g.P * g.Q * K * R * R * g.Cg);
  NNL_ROUTE("gconv_bf16_fwd<cg%d,kg%d>", g.Cg, g.Kg);
  launch<false>(x, w, bias, y, g, relu ? 1 : 0, s);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}

extern "C" int nnl_gconv2d_bf16_dgrad(const float* dy, const float* w, float* dx, int64_t N, int64_t H, int64_t W, int64_t C, int64_t K,
                                      int64_t G, int R, int stride, int pad, void* stream) {
  GGeom g;
  if (int e = make_geom("gconv2d_bf16_dgrad", N, H, W, C, K, G, R, stride, pad, &g)) return e;
  NNL_CHECK_ARG(dy && w && dx, "gconv2d_bf16_dgrad: null pointer");
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_CONV_DGRAD, s, 2.0 * N * g.P * g.Q * K * R * R * g.Cg);
  NNL_ROUTE("gconv_bf16_dgrad<cg%d,kg%d>", g.Cg, g.Kg);
  launch<true>(dy, w, nullptr, dx, g, 0, s);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}

extern "C" size_t nnl_gconv2d_bf16_workspace_bytes(int64_t N, int64_t H, int64_t W, int64_t C, int64_t K, int64_t G, int R, int stride,
                                                   int pad) {
  GGeom g;
  if (make_geom(nullptr, N, H, W, C, K, G, R, stride, pad, &g)) return 0;
  const long slabs = nnl_cdiv((long)g.N * g.P * g.Q, wgrad_rows(g));
  return slabs > 1 ? (size_t)slabs * K * R * R * g.Cg * sizeof(float) : 0;
}

extern "C" int nnl_gconv2d_bf16_wgrad(const float* x, const float* dy, float* dw, void* ws, size_t ws_bytes, int64_t N, int64_t H, int64_t W,
                                      int64_t C, int64_t K, int64_t G, int R, int stride, int pad, void* stream) {
  GGeom g;
  if (int e = make_geom("gconv2d_bf16_wgrad", N, H, W, C, K, G, R, stride, pad, &g)) return e;
  NNL_CHECK_ARG(x && dy && dw, "gconv2d_bf16_wgrad: null pointer");
  const long npq = (long)g.N * g.P * g.Q, rows = wgrad_rows(g), slabs = nnl_cdiv(npq, rows), numel = (long)K * R * R * g.Cg;
  if (slabs > 1 && (ws == nullptr || ws_bytes < (size_t)slabs * numel * sizeof(float)))
    return nnl_set_error(NNL_ERR_WORKSPACE, "gconv2d_bf16_wgrad: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_CONV_WGRAD, s, 2.0 * npq * numel);
  NNL_ROUTE("gconv_bf16_wgrad<cg%d,kg%d>@s%ld", g.Cg, g.Kg, slabs);
  const int nct = wgrad_ctiles(g), units = (int)nnl_cdiv(g.K, 16) * nct;
  const dim3 grid((unsigned)nnl_cdiv(units, 4), (unsigned)slabs);
  float* o = slabs > 1 ? (float*)ws : dw;
  if (R == 1)
    hipLaunchKernelGGL(gconv_bf16_wgrad_kernel<1>, grid, dim3(256), 0, s, x, dy, o, g, units, nct, npq, rows, numel);
  else
    hipLaunchKernelGGL(gconv_bf16_wgrad_kernel<3>, grid, dim3(256), 0, s, x, dy, o, g, units, nct, npq, rows, numel);
  NNL_CHECK_LAUNCH();
  if (slabs > 1) {
    hipLaunchKernelGGL(gconv_bf16_fold_kernel, dim3((unsigned)nnl_cdiv(numel, 256)), dim3(256), 0, s, (const float*)ws, dw, numel, (int)slabs);
    NNL_CHECK_LAUNCH();
  }
  return NNL_OK;
}
