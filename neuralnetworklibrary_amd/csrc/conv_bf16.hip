// K21 opt-in bf16 matrix-core convolutions: the dense body convolutions of the ResNet / RetinaNet / SENet / ResNeXt / Inception models
// (nn.Conv2d inside BasicBlock.forward / Bottleneck.forward, reference Applications/VisionModels/retinanet.py:43-59, 77-97, the 1x1
// downsample :344-348) with bf16 OPERANDS and fp32 accumulation.  Every tensor stays fp32 in memory: an operand is rounded to bf16
// (round to nearest even, v_cvt_pk_bf16_f32) in registers on its way into LDS, the products run on v_mfma_f32_32x32x16_bf16 (a lane holds
// 8 consecutive reduction indices of one row), the accumulators and the epilogue are fp32.  A bf16 x bf16 product is exact in fp32, so
// the result is the fp32 sum of the exact products of the rounded operands.
// Domain (nnl_conv2d_bf16_supported): groups 1, dilation 1, square filter with R S <= 49, stride 1 or 2, symmetric zero padding,
// C % 8 == 0 and K % 8 == 0.  NHWC activations, KRSC filter, as the fp32 kernels.
//
// filter (conv_bf16_pack_kernel): one small launch per call writes a bf16 copy of the filter, [K][R S][C] for the forward and the
//   transpose [C][R S][K] for the dgrad, so that the reduction of either direction is ONE contiguous run of R S Cin bf16 per output column
//   and a k-step's share is a 16-byte load with no conversion.  Traffic: 4 KRSC bytes read and 2 KRSC written once; every row tile
//   then re-reads 2 bytes per filter element instead of 4 (the fp32 dgrad's transpose writes and re-reads 4).
// forward / dgrad (conv_bf16_igemm_kernel<DGRAD>): implicit GEMM, rows = output pixels (dgrad: input pixels), columns = output
//   channels (dgrad: input channels), reduction = the R S Cin / 8 CHUNKS of 8 channels inside a tap, numbered tap-major; a k-step is 4
//   consecutive chunks (32 reduction indices), which may straddle a tap; the last step's missing chunks are zeros.  A workgroup (4 waves,
//   2 x 2, one 32 x 32 tile each on two accumulator chains) owns 64 rows x 64 columns.  Thread t stages chunk t & 3 of row t >> 2 of
//   both operands: its row's pixel coordinates are decoded once before the loop, its (tap, channel) position advances by additions only.
//   Per step it issues two 16-byte fp32 loads of the activation and one 16-byte load of the packed filter for the NEXT step, runs the
//   two MFMAs of this step, converts (4 cvt_pk) and writes one ds_write_b128 per operand into the other LDS buffer; one barrier per step.
//   The forward gathers x[n, p stride - pad + r, q stride - pad + s]; the dgrad gathers dy[n, (h + pad - r) / stride, (w + pad - s) / stride]
//   where both quotients are integral (the stride predicate): every dx pixel passes through the epilogue, so the shortcut addend is fused
//   at either stride.  Epilogue through LDS: 16 lanes store 256 contiguous bytes of a row; bias, addend, ReLU / sigmoid there.
//   LDS: a tile row is 32 bf16 = 64 B = 4 chunks of 16 B, chunk' = chunk ^ ((row >> 2) & 3).  ds_read_b128 is served 16 lanes at a time
//   over 64 banks = 256 B: the 16 consecutive rows of a quarter wave are 4 groups of 4 rows; a group fills 256 B at one chunk slot each
//   and the four groups take four different slots: no conflicts.  The write of 16 lanes covers the 256 contiguous bytes of 4 rows.
// wgrad (conv_bf16_wgrad_kernel): dw[k, r, s, c] = sum over the output pixels of dy[., k] x[. shifted by the tap, c].  The reduction runs over
//   pixels, the slow axis of both operands, so a step's 64 pixels are TRANSPOSED on their way into LDS: thread t loads 4 consecutive
//   pixels x 4 consecutive channels of each operand (float4 loads, 16 lanes = 256 contiguous bytes of a pixel), packs per channel its
//   4 pixels into 8 bytes and writes them (ds_write_b64) into a [channel][pixel] plane, where a lane reads its 8 pixels with one
//   ds_read_b128.  A workgroup owns 64 filters x 64 channels of ONE tap and a slab of pixels; the taps are the fastest grid index, so the
//   R S workgroups that share a dy tile and overlapping x pixels run together and meet in L2 (x is staged per tap: a shifted tap
//   moves the pixel axis by 2 bytes, which a 16-byte fragment read cannot follow).  Split-K over pixels: each slab writes its partial
//   [K][R S][C] to the workspace and a second launch adds the slabs in slab order.
//   LDS: a plane row is 64 bf16 = 128 B = 8 chunks, chunk' = chunk ^ (((row >> 1) ^ (row >> 4)) & 7).  Reads: 16 consecutive rows are
//   8 pairs; a pair fills the two 128-B halves of the bank window at one slot and the 8 pairs take 8 different slots: no conflicts.
//   Writes (32 lanes at a time: rows 4 i + j of 16 channel quads i, two pixel quads): the 16 rows take 8 different slots, 2-way.
// No atomics anywhere: two calls on the same inputs give the same bits.
#include "nnl_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int BM = 64, BN = 64;                // tile: rows x columns
constexpr int SC = 4;                          // igemm: 8-channel chunks per k-step
constexpr int ROWB = SC * 16;                  // igemm: bytes of a tile row in LDS
constexpr int OPB = BM * ROWB;                 // igemm: bytes of one operand's tile
constexpr int TL = 68;                         // pitch of the epilogue's fp32 output tile
constexpr int BP = 64;                         // wgrad: pixels per step
constexpr int PLB = 64 * BP * 2;               // wgrad: bytes of one operand's [64][BP] bf16 plane
constexpr int WG_ROWS = 256;                   // fewest pixels per wgrad slab (a multiple of BP)
constexpr int WG_SLABS = 64;                   // most wgrad slabs
constexpr int WG_GRID = 1024;                  // slabs are added until the grid has about this many workgroups

__device__ __forceinline__ unsigned pk_bf16(float a, float b) {
  bf16x2 t = {(__bf16)a, (__bf16)b};           // v_cvt_pk_bf16_f32: round to nearest even; a is the low half
  return __builtin_bit_cast(unsigned, t);
}

struct Gather {                                // what the igemm kernel reads rows from, and what it writes
  int H, W, Cin;                               // the gathered tensor's raster and channels (forward: x; dgrad: dy)
  int OH, OW, Cout;                            // the output raster and channels
  int R, S, stride, pad;
  int M;                                       // output pixels
  int cpt, nchunks;                            // chunks per tap, chunks of the whole reduction
};

// out[col][chunk q] (8 bf16) of the packed filter: forward col = k, reduction (tap, c); dgrad col = c, reduction (tap, k)
__global__ __launch_bounds__(256) void conv_bf16_pack_kernel(const float* __restrict__ w, u32x4* __restrict__ out, int K, int RS, int C,
                                                             int transpose) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (!transpose) {
    if (i >= (long)K * RS * C / 8) return;
    const f32x4 a = *reinterpret_cast<const f32x4*>(w + i * 8), b = *reinterpret_cast<const f32x4*>(w + i * 8 + 4);
    out[i] = u32x4{pk_bf16(a[0], a[1]), pk_bf16(a[2], a[3]), pk_bf16(b[0], b[1]), pk_bf16(b[2], b[3])};
    return;
  }
  const int k8n = K / 8;
  if (i >= (long)C * RS * k8n) return;
  const int c = (int)(i % C), k8 = (int)((i / C) % k8n), t = (int)(i / ((long)C * k8n));     // c fastest: the reads coalesce
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = w[((long)(k8 * 8 + j) * RS + t) * C + c];
  out[((long)c * RS + t) * k8n + k8] = u32x4{pk_bf16(v[0], v[1]), pk_bf16(v[2], v[3]), pk_bf16(v[4], v[5]), pk_bf16(v[6], v[7])};
}

template <bool DGRAD>
__global__ __launch_bounds__(256) void conv_bf16_igemm_kernel(const float* __restrict__ src, const u32x4* __restrict__ wp,
                                                              const float* __restrict__ bias, const float* __restrict__ addend,
                                                              float* __restrict__ out, Gather g, int act) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[BM * TL * 4];     // 2 x (A tile + B tile) = 16 KB; the epilogue's tile aliases them
  static_assert(BM * TL * 4 >= 4 * OPB, "the operand buffers must fit");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  const int col_tiles = (g.Cout + BN - 1) / BN;
  const int tile_m = blockIdx.x / col_tiles, tn = blockIdx.x - tile_m * col_tiles;
  const int m0 = tile_m * BM, n0 = tn * BN;
  // ---- this thread's staging share: chunk `sch` of row `srow` of both operands; the row's coordinates are decoded once
  const int srow = tid >> 2, sch = tid & 3;
  const int m = m0 + srow;
  const bool row_ok = m < g.M;
  const int ow = m % g.OW, tq = m / g.OW, oh = tq % g.OH, n = tq / g.OH;
  const int h0 = DGRAD ? oh + g.pad : oh * g.stride - g.pad, w0 = DGRAD ? ow + g.pad : ow * g.stride - g.pad;
  const int sh = g.stride - 1;                                      // stride 1 or 2: the quotient is a shift, the remainder a mask
  const long img = (long)n * g.H;
  const int bcol = n0 + srow;
  const bool col_ok = bcol < g.Cout;
  const u32x4* wrow = wp + (long)(col_ok ? bcol : 0) * g.nchunks;
  int q = sch, c8 = sch % g.cpt, tap = sch / g.cpt, r = tap / g.S, s = tap - r * g.S;     // position in the reduction; advanced by additions
  f32x4 ra0, ra1;
  u32x4 rb;
  auto load = [&]() {
    ra0 = ra1 = f32x4{0.f, 0.f, 0.f, 0.f};
    rb = u32x4{0u, 0u, 0u, 0u};
    if (q >= g.nchunks) return;
    if (col_ok) rb = wrow[q];
    int h, w;
    bool ok;
    if (DGRAD) {
      const int th = h0 - r, tw = w0 - s;
      h = th >> sh; w = tw >> sh;
      ok = th >= 0 && tw >= 0 && ((th | tw) & sh) == 0 && h < g.H && w < g.W;
    } else {
      h = h0 + r; w = w0 + s;
      ok = (unsigned)h < (unsigned)g.H && (unsigned)w < (unsigned)g.W;
    }
    if (ok && row_ok) {
      const float* p = src + ((img + h) * g.W + w) * g.Cin + c8 * 8;
      ra0 = *reinterpret_cast<const f32x4*>(p);
      ra1 = *reinterpret_cast<const f32x4*>(p + 4);
    }
  };
  auto advance = [&]() {
    q += SC; c8 += SC;
    while (c8 >= g.cpt) {
      c8 -= g.cpt;
      if (++s == g.S) { s = 0; ++r; }
    }
  };
  const int st_off = srow * ROWB + ((sch ^ ((srow >> 2) & 3)) * 16);
  auto commit = [&](int buf) {
    unsigned char* base = smem + buf * 2 * OPB + st_off;
    *reinterpret_cast<u32x4*>(base) = u32x4{pk_bf16(ra0[0], ra0[1]), pk_bf16(ra0[2], ra0[3]), pk_bf16(ra1[0], ra1[1]), pk_bf16(ra1[2], ra1[3])};
    *reinterpret_cast<u32x4*>(base + OPB) = rb;
  };
  const int fa = wm * 32 + (lane & 31), fb = wn * 32 + (lane & 31), fk = lane >> 5;
  const int a_off0 = fa * ROWB + ((fk ^ ((fa >> 2) & 3)) * 16), a_off1 = fa * ROWB + (((2 + fk) ^ ((fa >> 2) & 3)) * 16);
  const int b_off0 = OPB + fb * ROWB + ((fk ^ ((fb >> 2) & 3)) * 16), b_off1 = OPB + fb * ROWB + (((2 + fk) ^ ((fb >> 2) & 3)) * 16);
  f32x16 acc, acc2;                                                 // two chains: consecutive MFMAs are independent
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = acc2[e] = 0.f;
  const int steps = (g.nchunks + SC - 1) / SC;
  load();
  commit(0);
  __syncthreads();
  for (int it = 0; it < steps; ++it) {
    const int cur = it & 1;
    const bool more = it + 1 < steps;
    if (more) { advance(); load(); }                                // in flight while the MFMAs below run
    const unsigned char* base = smem + cur * 2 * OPB;
    const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(base + a_off0), b0 = *reinterpret_cast<const bf16x8*>(base + b_off0);
    const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(base + a_off1), b1 = *reinterpret_cast<const bf16x8*>(base + b_off1);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc, 0, 0, 0);
    acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc2, 0, 0, 0);
    if (more) commit(cur ^ 1);                                      // the buffer nobody reads in this step
    __syncthreads();
  }
  float* tl = reinterpret_cast<float*>(smem);                       // free: the loop ended with a barrier
#pragma unroll
  for (int e = 0; e < 16; ++e) tl[(wm * 32 + (e & 3) + 8 * (e >> 2) + fk * 4) * TL + wn * 32 + (lane & 31)] = acc[e] + acc2[e];
  __syncthreads();
#pragma unroll
  for (int k4 = 0; k4 < 4; ++k4) {
    const int idx4 = tid + k4 * 256, rl = idx4 >> 4, col = n0 + (idx4 & 15) * 4, row = m0 + rl;
    if (row >= g.M || col >= g.Cout) continue;
    f32x4 v = *reinterpret_cast<const f32x4*>(tl + rl * TL + (idx4 & 15) * 4);
    if (bias != nullptr) v += *reinterpret_cast<const f32x4*>(bias + col);
    if (addend != nullptr) v += *reinterpret_cast<const f32x4*>(addend + (long)row * g.Cout + col);
    if (act == 1) v = f32x4{fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f)};
    if (act == 2) v = f32x4{nnl_sigmoid(v[0]), nnl_sigmoid(v[1]), nnl_sigmoid(v[2]), nnl_sigmoid(v[3])};
    *reinterpret_cast<f32x4*>(out + (long)row * g.Cout + col) = v;
  }
}

struct WGeom {
  int H, W, C, K, P, Q, R, S, stride, pad;
  int M;                                       // output pixels N P Q
  int slab_rows;
};

__device__ __forceinline__ int wg_swz(int row) { return ((row >> 1) ^ (row >> 4)) & 7; }

__global__ __launch_bounds__(256) void conv_bf16_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ out,
                                                              WGeom g) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[4 * PLB];          // 2 x (dy plane + x plane) = 32 KB
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wk = wave >> 1, wc = wave & 1, half = lane >> 5, l31 = lane & 31;
  const int RS = g.R * g.S, ctiles = (g.C + BN - 1) / BN;
  const int tap = blockIdx.x % RS, tt = blockIdx.x / RS, tc = tt % ctiles, tk = tt / ctiles;
  const int r = tap / g.S, s = tap - r * g.S;
  const int k0 = tk * BM, c0 = tc * BN;
  const int m_begin = blockIdx.y * g.slab_rows, m_end = min(g.M, m_begin + g.slab_rows);
  const int cq = tid & 15, pq = tid >> 4;                            // this thread's 4 channels and 4 pixels of a step
  const bool live_k = k0 + cq * 4 < g.K, live_c = c0 + cq * 4 < g.C;
  f32x4 rg[4], rx[4];
  auto load = [&](int mc) {
    const int m = mc + pq * 4;
    int q = m % g.Q, t = m / g.Q, p = t % g.P, n = t / g.P;           // decoded once per step; the other three pixels follow by additions
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      rg[i] = rx[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (m + i < m_end) {
        if (live_k) rg[i] = *reinterpret_cast<const f32x4*>(dy + (long)(m + i) * g.K + k0 + cq * 4);
        const int h = p * g.stride - g.pad + r, w = q * g.stride - g.pad + s;
        if (live_c && (unsigned)h < (unsigned)g.H && (unsigned)w < (unsigned)g.W)
          rx[i] = *reinterpret_cast<const f32x4*>(x + (((long)n * g.H + h) * g.W + w) * g.C + c0 + cq * 4);
      }
      if (++q == g.Q) {
        q = 0;
        if (++p == g.P) { p = 0; ++n; }
      }
    }
  };
  auto commit = [&](int buf) {
    unsigned char* base = smem + buf * 2 * PLB;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int ch = cq * 4 + j, off = ch * (BP * 2) + (((pq >> 1) ^ wg_swz(ch)) * 16) + (pq & 1) * 8;
      *reinterpret_cast<u32x2*>(base + off) = u32x2{pk_bf16(rg[0][j], rg[1][j]), pk_bf16(rg[2][j], rg[3][j])};
      *reinterpret_cast<u32x2*>(base + PLB + off) = u32x2{pk_bf16(rx[0][j], rx[1][j]), pk_bf16(rx[2][j], rx[3][j])};
    }
  };
  const int fa = wk * 32 + l31, fb = wc * 32 + l31;
  f32x16 acc, acc2;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = acc2[e] = 0.f;
  load(m_begin);
  commit(0);
  __syncthreads();
  int cur = 0;
  for (int mc = m_begin; mc < m_end; mc += BP) {
    const bool more = mc + BP < m_end;
    if (more) load(mc + BP);                                        // in flight while the MFMAs below run
    const unsigned char* base = smem + cur * 2 * PLB;
#pragma unroll
    for (int j = 0; j < 4; ++j) {                                   // 16 pixels each: chunk 2 j + half holds this lane's 8
      const bf16x8 a = *reinterpret_cast<const bf16x8*>(base + fa * (BP * 2) + (((2 * j + half) ^ wg_swz(fa)) * 16));
      const bf16x8 b = *reinterpret_cast<const bf16x8*>(base + PLB + fb * (BP * 2) + (((2 * j + half) ^ wg_swz(fb)) * 16));
      if (j & 1) acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc2, 0, 0, 0);
      else acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
    }
    if (more) commit(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  }
  float* o = out + (long)blockIdx.y * g.K * RS * g.C;
  const int c = c0 + fb;
  if (c < g.C) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int k = k0 + wk * 32 + (e & 3) + 8 * (e >> 2) + half * 4;
      if (k < g.K) o[((long)k * RS + tap) * g.C + c] = acc[e] + acc2[e];
    }
  }
}

__global__ __launch_bounds__(256) void conv_bf16_wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw, long numel,
                                                                     int slabs) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= numel) return;
  float a = part[i];
  for (int sl = 1; sl < slabs; ++sl) a += part[(long)sl * numel + i];           // slab order: fixed
  dw[i] = a;
}

// the domain; nothing is reported through nnl_last_error when `who` is null (the plain query)
int check_geom(const char* who, const nnl_conv_geom_t* g) {
#define BF16_DOMAIN(cond, ...)                                                    \
  do {                                                                            \
    if (!(cond)) return who ? nnl_set_error(NNL_ERR_INVALID_ARG, __VA_ARGS__) : NNL_ERR_INVALID_ARG; \
  } while (0)
  const char* name = who ? who : "";
  BF16_DOMAIN(g != nullptr, "%s: null geometry", name);
  BF16_DOMAIN(g->N > 0 && g->H > 0 && g->W > 0 && g->C > 0 && g->K > 0 && g->R > 0 && g->S > 0 && g->P > 0 && g->Q > 0 && g->pad >= 0,
              "%s: sizes must be positive", name);
  BF16_DOMAIN(g->R == g->S && g->R * g->S <= 49, "%s: filter %dx%d (square, at most 49 taps)", name, g->R, g->S);
  BF16_DOMAIN(g->stride == 1 || g->stride == 2, "%s: stride %d (1 or 2)", name, g->stride);
  BF16_DOMAIN(g->C % 8 == 0 && g->K % 8 == 0, "%s: C = %d and K = %d must be multiples of 8", name, g->C, g->K);
  BF16_DOMAIN(g->H + 2 * g->pad >= g->R && g->W + 2 * g->pad >= g->S && g->P == (g->H + 2 * g->pad - g->R) / g->stride + 1 &&
                  g->Q == (g->W + 2 * g->pad - g->S) / g->stride + 1,
              "%s: P x Q = %d x %d is not the output size of this geometry", name, g->P, g->Q);
  const int64_t lim = (int64_t)1 << 31;
  BF16_DOMAIN((int64_t)g->N * g->H * g->W * g->C < lim && (int64_t)g->N * g->P * g->Q * g->K < lim && (int64_t)g->K * g->R * g->S * g->C < lim,
              "%s: tensor too large", name);
#undef BF16_DOMAIN
  return NNL_OK;
}

// pixels per wgrad slab: a multiple of BP, at least WG_ROWS, and no more slabs than fill the grid or than WG_SLABS
long wgrad_slab_rows(const nnl_conv_geom_t* g) {
  const long M = (long)g->N * g->P * g->Q, tiles = nnl_cdiv(g->K, BM) * nnl_cdiv(g->C, BN) * g->R * g->S;
  long slabs = WG_GRID / tiles;
  slabs = slabs < 1 ? 1 : (slabs > WG_SLABS ? WG_SLABS : slabs);
  const long rows = nnl_cdiv(nnl_cdiv(M, slabs), BP) * BP;
  return rows > WG_ROWS ? rows : WG_ROWS;
}

}  // namespace

extern "C" int nnl_conv2d_bf16_supported(const nnl_conv_geom_t* g) { return check_geom(nullptr, g) == NNL_OK ? 1 : 0; }

extern "C" int nnl_conv2d_bf16_pack_filter(const float* w, void* wp, const nnl_conv_geom_t* g, int transpose, void* stream) {
  if (int e = check_geom("conv2d_bf16_pack_filter", g)) return e;
  NNL_CHECK_ARG(w && wp, "conv2d_bf16_pack_filter: null pointer");
  const long n8 = (long)g->K * g->R * g->S * g->C / 8;
  NNL_ROUTE("conv_bf16_pack%s", transpose ? ":t" : "");
  hipLaunchKernelGGL(conv_bf16_pack_kernel, dim3((unsigned)nnl_cdiv(n8, 256)), dim3(256), 0, (hipStream_t)stream, w, (u32x4*)wp, g->K,
                     g->R * g->S, g->C, transpose ? 1 : 0);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}

extern "C" int nnl_conv2d_bf16_fwd(const float* x, const void* wp, const float* bias, float* y, const nnl_conv_geom_t* g, int relu,
                                   void* stream) {
  if (int e = check_geom("conv2d_bf16_fwd", g)) return e;
  NNL_CHECK_ARG(x && wp && y, "conv2d_bf16_fwd: null pointer");
  NNL_CHECK_ARG(relu >= 0 && relu <= 2, "conv2d_bf16_fwd: relu = %d (0 none, 1 ReLU, 2 sigmoid)", relu);
  Gather G{g->H, g->W, g->C, g->P, g->Q, g->K, g->R, g->S, g->stride, g->pad, g->N * g->P * g->Q, g->C / 8, g->R * g->S * (g->C / 8)};
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_CONV_FWD, s, 2.0 * G.M * g->K * g->R * g->S * g->C);
  NNL_ROUTE("conv_bf16_igemm<fwd>");
  hipLaunchKernelGGL(conv_bf16_igemm_kernel<false>, dim3((unsigned)(nnl_cdiv(G.M, BM) * nnl_cdiv(G.Cout, BN))), dim3(256), 0, s, x,
                     (const u32x4*)wp, bias, (const float*)nullptr, y, G, relu);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}

extern "C" int nnl_conv2d_bf16_dgrad(const float* dy, const void* wpt, float* dx, const nnl_conv_geom_t* g, const float* addend,
                                     void* stream) {
  if (int e = check_geom("conv2d_bf16_dgrad", g)) return e;
  NNL_CHECK_ARG(dy && wpt && dx, "conv2d_bf16_dgrad: null pointer");
  Gather G{g->P, g->Q, g->K, g->H, g->W, g->C, g->R, g->S, g->stride, g->pad, g->N * g->H * g->W, g->K / 8, g->R * g->S * (g->K / 8)};
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_CONV_DGRAD, s, 2.0 * g->N * g->P * g->Q * g->K * g->R * g->S * g->C);
  NNL_ROUTE("conv_bf16_igemm<dgrad>%s", addend ? ":addend" : "");
  hipLaunchKernelGGL(conv_bf16_igemm_kernel<true>, dim3((unsigned)(nnl_cdiv(G.M, BM) * nnl_cdiv(G.Cout, BN))), dim3(256), 0, s, dy,
                     (const u32x4*)wpt, (const float*)nullptr, addend, dx, G, 0);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}

extern "C" size_t nnl_conv2d_bf16_wgrad_workspace_bytes(const nnl_conv_geom_t* g) {
  if (check_geom(nullptr, g)) return 0;
  const long slabs = nnl_cdiv((long)g->N * g->P * g->Q, wgrad_slab_rows(g));
  return slabs > 1 ? (size_t)slabs * g->K * g->R * g->S * g->C * sizeof(float) : 0;
}

extern "C" int nnl_conv2d_bf16_wgrad(const float* x, const float* dy, float* dw, const nnl_conv_geom_t* g, void* ws, size_t ws_bytes,
                                     void* stream) {
  if (int e = check_geom("conv2d_bf16_wgrad", g)) return e;
  NNL_CHECK_ARG(x && dy && dw, "conv2d_bf16_wgrad: null pointer");
  const long M = (long)g->N * g->P * g->Q, rows = wgrad_slab_rows(g), slabs = nnl_cdiv(M, rows), numel = (long)g->K * g->R * g->S * g->C;
  if (slabs > 1 && (ws == nullptr || ws_bytes < (size_t)slabs * numel * sizeof(float)))
    return nnl_set_error(NNL_ERR_WORKSPACE, "conv2d_bf16_wgrad: workspace too small");
  WGeom G{g->H, g->W, g->C, g->K, g->P, g->Q, g->R, g->S, g->stride, g->pad, (int)M, (int)rows};
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_CONV_WGRAD, s, 2.0 * M * numel);
  NNL_ROUTE("conv_bf16_wgrad@s%ld", slabs);
  const dim3 grid((unsigned)(nnl_cdiv(g->K, BM) * nnl_cdiv(g->C, BN) * g->R * g->S), (unsigned)slabs);
  hipLaunchKernelGGL(conv_bf16_wgrad_kernel, grid, dim3(256), 0, s, x, dy, slabs > 1 ? (float*)ws : dw, G);
  NNL_CHECK_LAUNCH();
  if (slabs > 1) {
    hipLaunchKernelGGL(conv_bf16_wgrad_reduce_kernel, dim3((unsigned)nnl_cdiv(numel, 256)), dim3(256), 0, s, (const float*)ws, dw, numel, (int)slabs);
    NNL_CHECK_LAUNCH();
  }
  return NNL_OK;
}
