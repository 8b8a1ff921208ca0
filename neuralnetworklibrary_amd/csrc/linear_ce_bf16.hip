// K23 fused bf16 decoder + softmax cross-entropy: loss = mean_r( logsumexp_j z[r, j] - z[r, target[r]] ), z = rb(x) rb(w)^T summed in fp32,
// for the language model's tied decoder ([seq bs, emb] x [V, emb]^T, V = 47 343) WITHOUT the [M, N] logits or their gradient ever reaching
// memory: the flash-attention scheme on a classifier head.  Operand rounding, LDS tiles and staging are those of linear_bf16.hip
// (linear_bf16_tiles.h); products on v_mfma_f32_32x32x16_bf16, everything after them fp32.  Domain: M, N >= 1, 1 <= K <= 512.
//
// FORWARD, linear_ce_fwd_kernel: grid = row tiles of 128 x vocabulary RANGES (a whole number of 128-column tiles, at least two, as many
//   ranges as bring the grid to about 1536 workgroups; the range is the fastest grid index, so the workgroups that run together share a row
//   tile of x in L2).  Per column tile the stream kernel's K loop (x and w DIRECT, 32-deep steps, two LDS buffers, register prefetch, one
//   barrier per step; 40 KB), but with the operand roles swapped: w is the MFMA's A operand and x its B operand, so a LANE holds one row of
//   x and its 16 accumulator registers hold 16 columns.  A wave is 64 rows x 64 columns: per row a lane sees 32 columns of a tile, all in
//   its own registers (the kernel is held to 256 registers: two workgroups per SIMD set).  The epilogue stores nothing: columns >= N become
//   -inf, then per row  m' = max(m, max_j z), s = s exp(m - m') + sum_j exp(z_j - m')  (the 16 columns of an accumulator added in register
//   order, then the two accumulators), and z[r, target[r]] is picked up where the target column passes by.  At the end of the range the 4
//   lanes that share a row (2 half waves x 2 column waves) merge through LDS in a fixed order and {m, s, z_t} go to the workspace
//   [range][3][M].
//   linear_ce_finish_kernel merges the ranges of a row in range order: lse = m + log s, loss_rows = lse - z_t (0 and the index-error flag
//   for a target outside [0, N)); linear_ce_mean_kernel: the mean over all M rows in a fixed order.
// BACKWARD, linear_ce_bwd_kernel<MODE, KT>: D[r, j] = (exp(z[r, j] - lse[r]) - [j == target[r]]) g / M, recomputed tile by tile, split
//   into two bf16 operands hi = rb(D), lo = rb(D - hi) (one rounding is off by up to 2^-8 of D, the pair by 2^-16) and laid into LDS in
//   operand layout; dx = (hi + lo) rb(w) (MODE DX) and dw = (hi + lo)^T rb(x) (MODE DW), hi before lo in every accumulator, are ONE kernel
//   with the roles of the two matrices exchanged.  A workgroup OWNS 64 rows of one matrix (DX: x, DW: w) and WALKS 128-row tiles of the
//   other inside its slab.  Per walked tile:
//     1. z = walked tile x owned tile^T over K (both DIRECT, the stream loop; the walked rows are the A operand, so a lane holds one OWNED
//        row and its registers hold walked rows: 4 consecutive ones per register quad);
//     2. D from the accumulators (DX: lse and target of the lane's own row in registers; DW: those of the walked tile's 128 rows in LDS),
//        zero for rows >= M and columns >= N, packed 4 walked indices = 8 bytes per ds_write_b64 into 4 sub-tiles (hi, and 4 more for lo)
//        of 64 owned rows x 32 walked indices: exactly the streamed-tile layout with the walked index as the reduction axis;
//     3. acc[64 owned rows][K] += D x walked tile, the walked matrix staged TRANSPOSED (operand rows = its columns, 128 at a time), one
//        128 x 32 tile per step through two LDS buffers.  The accumulator is 64 x 128 KT floats (KT = ceil(K / 128) <= 4: 128 registers per
//        lane at K = 512), a wave holding 32 of every 128 columns.
//   LDS: 30 KB of stream buffers (steps 1 and 3 share them; step 3 needs 20 KB, so two lo sub-tiles live in the last 10) + 20 KB of D hi +
//   10 KB of D lo + 1 KB of row statistics = 61 KB.  The walked axis is cut into slabs (a multiple of 128, at least 512, at most 16 slabs,
//   as many as bring the grid to about 1024 workgroups); each slab writes its partial [rows][K] to the workspace and linear_ce_fold_kernel
//   adds them in slab order; one slab writes the result itself.
// No atomics anywhere: two calls on the same inputs give the same bits.
#include "linear_bf16_tiles.h"

namespace {

constexpr int KMAX = 512;                      // the accumulator of the backward kernels holds a whole row of K
constexpr int OWN = 64;                        // rows a backward workgroup owns
constexpr int OTILEB = OWN * TP;               // bytes of a 64-row streamed tile
constexpr int FWD_GRID = 1536;                 // ranges are added until the forward grid has about this many workgroups
constexpr int RANGE_MIN = 2;                   // fewest column tiles of a range (but for the last one)
constexpr int SLAB_MIN = 512;                  // fewest walked rows per backward slab (a multiple of BN)
constexpr int SLAB_MAX = 16;                   // most slabs
constexpr int SPLIT_GRID = 1024;               // slabs are added until a backward grid has about this many workgroups
static_assert(SLAB_MIN % BN == 0, "a slab is a whole number of walked tiles");

struct MSZ { float m, s, zt; };                // of a set of columns of one row: their maximum, sum exp(z - m), and z[target] or -inf

__device__ __forceinline__ float shift_of(float m) { return m == -INFINITY ? 0.f : m; }       // an empty set shifts by 0: exp(-inf - 0) = 0

__device__ __forceinline__ MSZ msz_merge(MSZ a, MSZ b) {
  const float m = fmaxf(a.m, b.m), sh = shift_of(m);
  return MSZ{m, a.s * expf(a.m - sh) + b.s * expf(b.m - sh), fmaxf(a.zt, b.zt)};
}

__device__ __forceinline__ int reg_index(int e, int half) { return (e & 3) + 8 * (e >> 2) + 4 * half; }   // the A-side index of accumulator register e

struct FwdPlan {
  long M, N, K, ldx, ldw;
  int ranges, range_tiles, col_tiles, vecx, vecw;
};

__global__ __launch_bounds__(256, 2) void linear_ce_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                            const int64_t* __restrict__ target, float* __restrict__ part, FwdPlan p) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[4 * TILEB];        // 2 x (x tile + w tile) = 40 KB
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1, half = lane >> 5, l31 = lane & 31;
  const int tr = blockIdx.x / p.ranges, rg = blockIdx.x - tr * p.ranges;
  const long r0 = (long)tr * BN;
  const int ct_end = min(p.col_tiles, (rg + 1) * p.range_tiles);
  f32x4 rx[4], rw[4];
  MSZ st[2];
  long tg[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const long row = r0 + (wm * 2 + i) * 32 + l31;
    st[i] = MSZ{-INFINITY, 0.f, -INFINITY};
    tg[i] = row < p.M ? (long)target[row] : -1;
  }
  for (int ct = rg * p.range_tiles; ct < ct_end; ++ct) {
    const long c0 = (long)ct * BN;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    load_direct(x, p.ldx, r0, p.M, 0, p.K, p.vecx, rx);
    load_direct(w, p.ldw, c0, p.N, 0, p.K, p.vecw, rw);
    commit_direct(smem, rx);
    commit_direct(smem + TILEB, rw);
    __syncthreads();
    int cur = 0;
    for (long red = 0; red < p.K; red += KS) {
      const bool more = red + KS < p.K;
      if (more) {                                                     // in flight while the MFMAs below run
        load_direct(x, p.ldx, r0, p.M, red + KS, p.K, p.vecx, rx);
        load_direct(w, p.ldw, c0, p.N, red + KS, p.K, p.vecw, rw);
      }
      const unsigned char* base = smem + cur * 2 * TILEB;
#pragma unroll
      for (int kh = 0; kh < 2; ++kh) {
        const int ch = 2 * kh + half;
        bf16x8 fx[2], fw[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) fx[i] = frag(base, (wm * 2 + i) * 32 + l31, ch);
#pragma unroll
        for (int j = 0; j < 2; ++j) fw[j] = frag(base + TILEB, (wn * 2 + j) * 32 + l31, ch);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fw[j], fx[i], acc[i][j], 0, 0, 0);   // columns in registers
      }
      if (more) {
        commit_direct(smem + (cur ^ 1) * 2 * TILEB, rx);
        commit_direct(smem + (cur ^ 1) * 2 * TILEB + TILEB, rw);
      }
      __syncthreads();
      cur ^= 1;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      float tmax = -INFINITY;
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const long col = c0 + (wn * 2 + j) * 32 + reg_index(e, half);
          const float v = col < p.N ? acc[i][j][e] : -INFINITY;         // a zero-filled pad column is no logit
          acc[i][j][e] = v;
          tmax = fmaxf(tmax, v);
          if (col == tg[i]) st[i].zt = v;
        }
      const float m = fmaxf(st[i].m, tmax), sh = shift_of(m);
      float t[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        t[j] = expf(acc[i][j][0] - sh);
#pragma unroll
        for (int e = 1; e < 16; ++e) t[j] += expf(acc[i][j][e] - sh);
      }
      st[i].s = st[i].s * expf(st[i].m - sh) + (t[0] + t[1]);
      st[i].m = m;
    }
  }
  // (every K loop ended with a barrier: smem is free)  the 4 partials of a row, in the order (column wave, half wave)
  MSZ* lds = reinterpret_cast<MSZ*>(smem);                              // [4][128]
#pragma unroll
  for (int i = 0; i < 2; ++i) lds[(wn * 2 + half) * BN + (wm * 2 + i) * 32 + l31] = st[i];
  __syncthreads();
  if (tid < BN && r0 + tid < p.M) {
    MSZ a = lds[tid];
#pragma unroll
    for (int q = 1; q < 4; ++q) a = msz_merge(a, lds[q * BN + tid]);
    float* o = part + (long)rg * 3 * p.M + r0 + tid;
    o[0] = a.m;
    o[p.M] = a.s;
    o[2 * p.M] = a.zt;
  }
}

__global__ __launch_bounds__(256) void linear_ce_finish_kernel(const float* __restrict__ part, const int64_t* __restrict__ target,
                                                               float* __restrict__ lse, float* __restrict__ loss_rows, long M, long N, int ranges,
                                                               int32_t* __restrict__ err_flag) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= M) return;
  MSZ a{part[r], part[M + r], part[2 * M + r]};
  for (int rg = 1; rg < ranges; ++rg) {                                 // range order: fixed
    const float* q = part + (long)rg * 3 * M + r;
    a = msz_merge(a, MSZ{q[0], q[M], q[2 * M]});
  }
  const float l = a.m + logf(a.s);
  lse[r] = l;
  const int64_t t = target[r];
  if (t >= 0 && t < N) {
    loss_rows[r] = l - a.zt;
  } else {
    loss_rows[r] = 0.f;
    if (err_flag) *err_flag = 1;
  }
}

// out[0] = mean(v[0 .. n))  (a single block, fixed order)
__global__ __launch_bounds__(256) void linear_ce_mean_kernel(const float* __restrict__ v, float* __restrict__ out, long n) {
  __shared__ float red[256];
  float a = 0.f;
  for (long i = threadIdx.x; i < n; i += 256) a += v[i];
  a = nnl_block_tree_reduce<256>(a, NnlSum(), red);
  if (threadIdx.x == 0) out[0] = a / (float)n;
}

struct BwdPlan {
  long M, N, K;
  long own_n, walk_n;                          // rows of the owned and of the walked matrix: DX M, N; DW N, M
  long ld_own, ld_walk, slab_len;              // (a slab is a multiple of BN walked rows)
  int vec_own, vec_walk;
};

enum { DX = 0, DW = 1 };

template <int MODE, int KT>
__global__ __launch_bounds__(256) void linear_ce_bwd_kernel(const float* __restrict__ own, const float* __restrict__ walk,
                                                            const int64_t* __restrict__ target, const float* __restrict__ lse,
                                                            const float* __restrict__ gup, float* __restrict__ out, BwdPlan p) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * (OTILEB + TILEB)];       // step 1: 2 x (owned + walked tile); step 3: 2 walked tiles
  __shared__ __attribute__((aligned(16))) unsigned char dt[4 * OTILEB];                   // D hi: 4 sub-tiles of 64 owned rows x 32 walked indices
  __shared__ __attribute__((aligned(16))) unsigned char dlo[2 * OTILEB];                  // D lo: sub-tiles 2, 3; 0 and 1 lie in the third of smem
  auto lo_tile = [&](int sub) { return sub < 2 ? smem + 2 * TILEB + sub * OTILEB : dlo + (sub - 2) * OTILEB; };   // that step 3 leaves free
  __shared__ float lse_s[BN];                                                             // DW: the walked tile's rows of x
  __shared__ int tg_s[BN];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
  const long o0 = (long)blockIdx.x * OWN;
  const long q_begin = (long)blockIdx.y * p.slab_len, q_end = min(p.walk_n, q_begin + p.slab_len);
  const float scale = gup[0] / (float)p.M;
  float lse_r[2];
  long tg_r[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {                                          // DX: the lane's own rows of x
    const long row = o0 + i * 32 + l31;
    const bool ok = MODE == DX && row < p.M;
    lse_r[i] = ok ? lse[row] : INFINITY;                                 // exp(z - inf) = 0: a row >= M has D = 0
    tg_r[i] = ok ? (long)target[row] : -1;
  }
  f32x16 acc[2][KT];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][kt][e] = 0.f;
  f32x4 ro[2], rw[4];
  for (long q0 = q_begin; q0 < q_end; q0 += BN) {
    if (MODE == DW && tid < BN) {                                       // (read in step 2, behind step 1's barriers; the last reader was the
      const long row = q0 + tid;                                        // previous tile's step 2, in front of step 3's)
      const int64_t t = row < p.M ? target[row] : -1;
      lse_s[tid] = row < p.M ? lse[row] : INFINITY;
      tg_s[tid] = t >= 0 && t < p.N ? (int)t : -1;
    }
    // 1. z[walked 128][owned 64]: wave = 32 walked rows (registers) x 64 owned rows (lanes)
    f32x16 z[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) z[i][e] = 0.f;
    load_direct<1>(own, p.ld_own, o0, p.own_n, 0, p.K, p.vec_own, ro);
    load_direct(walk, p.ld_walk, q0, p.walk_n, 0, p.K, p.vec_walk, rw);
    commit_direct<1>(smem, ro);
    commit_direct(smem + OTILEB, rw);
    __syncthreads();
    int cur = 0;
    for (long red = 0; red < p.K; red += KS) {
      const bool more = red + KS < p.K;
      if (more) {
        load_direct<1>(own, p.ld_own, o0, p.own_n, red + KS, p.K, p.vec_own, ro);
        load_direct(walk, p.ld_walk, q0, p.walk_n, red + KS, p.K, p.vec_walk, rw);
      }
      const unsigned char* base = smem + cur * (OTILEB + TILEB);
#pragma unroll
      for (int kh = 0; kh < 2; ++kh) {
        const int ch = 2 * kh + half;
        const bf16x8 fq = frag(base + OTILEB, wave * 32 + l31, ch);
#pragma unroll
        for (int i = 0; i < 2; ++i) z[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fq, frag(base, i * 32 + l31, ch), z[i], 0, 0, 0);
      }
      if (more) {
        commit_direct<1>(smem + (cur ^ 1) * (OTILEB + TILEB), ro);
        commit_direct(smem + (cur ^ 1) * (OTILEB + TILEB) + OTILEB, rw);
      }
      __syncthreads();
      cur ^= 1;
    }
    // 2. D, rounded to bf16, into sub-tile `wave` (its 32 walked indices): register quad c = chunk c, this half wave's 8 bytes of it
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float d[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int wi = wave * 32 + reg_index(4 * c + k, half);        // walked index inside the tile
          const long col = MODE == DX ? q0 + wi : o0 + i * 32 + l31;    // the vocabulary index
          const float l = MODE == DX ? lse_r[i] : lse_s[wi];
          const long t = MODE == DX ? tg_r[i] : (long)tg_s[wi];
          const float pr = expf(z[i][4 * c + k] - l);
          d[k] = col < p.N ? (pr - (col == t ? 1.f : 0.f)) * scale : 0.f;
        }
        const unsigned h0 = pk_bf16(d[0], d[1]), h1 = pk_bf16(d[2], d[3]);       // D = hi + lo: lo = rb(D - hi), exact to 2^-16 of D
        const unsigned l0 = pk_bf16(d[0] - __uint_as_float(h0 << 16), d[1] - __uint_as_float(h0 & 0xffff0000u));
        const unsigned l1 = pk_bf16(d[2] - __uint_as_float(h1 << 16), d[3] - __uint_as_float(h1 & 0xffff0000u));
        const int off = tile_off(i * 32 + l31, c) + half * 8;
        *reinterpret_cast<u32x2*>(dt + wave * OTILEB + off) = u32x2{h0, h1};
        *reinterpret_cast<u32x2*>(lo_tile(wave) + off) = u32x2{l0, l1};
      }
    // 3. acc[owned 64][K] += D[owned 64][walked 128] x walked tile [128][K]: per step 32 walked rows x 128 columns, staged TRANSPOSED
    load_trans(walk, p.ld_walk, 0, p.K, q0, p.walk_n, p.vec_walk, rw);
    commit_trans(smem, rw);
    __syncthreads();                                                    // (also: D is complete)
    cur = 0;
    for (int sub = 0; sub < 4; ++sub) {
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) {
        const bool more = kt + 1 < KT || sub < 3;
        if (more) load_trans(walk, p.ld_walk, kt + 1 < KT ? (kt + 1) * BN : 0, p.K, q0 + (kt + 1 < KT ? sub : sub + 1) * KS, p.walk_n, p.vec_walk, rw);
        const unsigned char* base = smem + cur * TILEB;
#pragma unroll
        for (int kh = 0; kh < 2; ++kh) {
          const int ch = 2 * kh + half;
          const bf16x8 fb = frag(base, wave * 32 + l31, ch);
#pragma unroll
          for (int i = 0; i < 2; ++i) {                                   // hi, then lo: a fixed order
            acc[i][kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag(dt + sub * OTILEB, i * 32 + l31, ch), fb, acc[i][kt], 0, 0, 0);
            acc[i][kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag(lo_tile(sub), i * 32 + l31, ch), fb, acc[i][kt], 0, 0, 0);
          }
        }
        if (more) commit_trans(smem + (cur ^ 1) * TILEB, rw);
        __syncthreads();
        cur ^= 1;
      }
    }
  }
  float* o = out + (long)blockIdx.y * p.own_n * p.K;                    // the slab's partial in the workspace; one slab: the result itself
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
      const long col = kt * BN + wave * 32 + l31;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const long row = o0 + i * 32 + reg_index(e, half);
        if (row < p.own_n && col < p.K) o[row * p.K + col] = acc[i][kt][e];
      }
    }
}

__global__ __launch_bounds__(256) void linear_ce_fold_kernel(const float* __restrict__ part, float* __restrict__ out, long numel, int slabs) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= numel) return;
  float s = part[i];
  for (int sl = 1; sl < slabs; ++sl) s += part[(long)sl * numel + i];            // slab order: fixed
  out[i] = s;
}

bool in_domain(int64_t M, int64_t N, int64_t K) { return M > 0 && N > 0 && K > 0 && K <= KMAX && M < DIM_MAX && N < DIM_MAX; }

// the forward's column tiles per range
long range_tiles(long M, long N) {
  const long col_tiles = nnl_cdiv(N, BN);
  long want = FWD_GRID / nnl_cdiv(M, BN);
  want = want < 1 ? 1 : want;
  const long len = nnl_cdiv(col_tiles, want);
  return len > RANGE_MIN ? len : RANGE_MIN;
}

// a backward walk over `walk_n` rows for `own_n` owned rows: the slab length (a multiple of BN, at least SLAB_MIN)
long slab_len(long walk_n, long own_n) {
  long want = SPLIT_GRID / nnl_cdiv(own_n, OWN);
  want = want < 1 ? 1 : (want > SLAB_MAX ? SLAB_MAX : want);
  const long len = nnl_cdiv(nnl_cdiv(walk_n, want), BN) * BN;
  return len > SLAB_MIN ? len : SLAB_MIN;
}

long slab_count(long walk_n, long own_n) { return nnl_cdiv(walk_n, slab_len(walk_n, own_n)); }

size_t part_bytes(long slabs, long rows, long K) { return slabs > 1 ? (size_t)slabs * rows * K * sizeof(float) : 0; }

template <int MODE>
int launch_bwd(const float* own, const float* walk, const int64_t* target, const float* lse, const float* g, float* out, float* ws, BwdPlan P,
               hipStream_t s) {
  const long slabs = nnl_cdiv(P.walk_n, P.slab_len), numel = P.own_n * P.K;
  const dim3 grid((unsigned)nnl_cdiv(P.own_n, OWN), (unsigned)slabs);
  float* o = slabs > 1 ? ws : out;
  NNL_ROUTE("linear_ce_bf16_%s%s@s%ld", MODE == DX ? "dx" : "dw", P.vec_own && P.vec_walk ? "" : ":dword", slabs);
  switch (nnl_cdiv(P.K, BN)) {
    case 1: hipLaunchKernelGGL((linear_ce_bwd_kernel<MODE, 1>), grid, dim3(256), 0, s, own, walk, target, lse, g, o, P); break;
    case 2: hipLaunchKernelGGL((linear_ce_bwd_kernel<MODE, 2>), grid, dim3(256), 0, s, own, walk, target, lse, g, o, P); break;
    case 3: hipLaunchKernelGGL((linear_ce_bwd_kernel<MODE, 3>), grid, dim3(256), 0, s, own, walk, target, lse, g, o, P); break;
    default: hipLaunchKernelGGL((linear_ce_bwd_kernel<MODE, 4>), grid, dim3(256), 0, s, own, walk, target, lse, g, o, P); break;
  }
  NNL_CHECK_LAUNCH();
  if (slabs > 1) {
    hipLaunchKernelGGL(linear_ce_fold_kernel, dim3((unsigned)nnl_cdiv(numel, 256)), dim3(256), 0, s, (const float*)ws, out, numel, (int)slabs);
    NNL_CHECK_LAUNCH();
  }
  return NNL_OK;
}

}  // namespace

extern "C" int nnl_linear_ce_bf16_supported(int64_t M, int64_t N, int64_t K) { return in_domain(M, N, K) ? 1 : 0; }

extern "C" size_t nnl_linear_ce_bf16_fwd_workspace_bytes(int64_t M, int64_t N, int64_t K) {
  if (!in_domain(M, N, K)) return 0;
  return (size_t)nnl_cdiv(nnl_cdiv(N, BN), range_tiles(M, N)) * 3 * M * sizeof(float);
}

extern "C" int nnl_linear_ce_bf16_fwd(const float* x, const float* w, const int64_t* target, float* lse, float* loss_rows, float* loss_mean,
                                      int64_t M, int64_t N, int64_t K, int64_t ldx, int64_t ldw, void* ws, size_t ws_bytes, int32_t* err_flag,
                                      void* stream) {
  NNL_CHECK_ARG(in_domain(M, N, K), "linear_ce_bf16_fwd: M = %ld, N = %ld, K = %ld outside 0 < M, N < 2^31 - 256, 0 < K <= %d", (long)M, (long)N,
                (long)K, KMAX);
  NNL_CHECK_ARG(x && w && target && lse && loss_rows && loss_mean, "linear_ce_bf16_fwd: null pointer");
  NNL_CHECK_ARG(ldx >= K && ldw >= K, "linear_ce_bf16_fwd: a row stride is shorter than its row (ldx %ld, ldw %ld, K %ld)", (long)ldx, (long)ldw,
                (long)K);
  const long rt = range_tiles(M, N), col_tiles = nnl_cdiv(N, BN), ranges = nnl_cdiv(col_tiles, rt), grid = nnl_cdiv(M, BN) * ranges;
  NNL_CHECK_ARG(grid < DIM_MAX, "linear_ce_bf16_fwd: too many tiles");
  if (ws == nullptr || ws_bytes < (size_t)ranges * 3 * M * sizeof(float))
    return nnl_set_error(NNL_ERR_WORKSPACE, "linear_ce_bf16_fwd: workspace too small");
  FwdPlan P{M, N, K, ldx, ldw, (int)ranges, (int)rt, (int)col_tiles, vec_ok(x, ldx), vec_ok(w, ldw)};
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_GEMM, s, 2.0 * M * N * K);
  NNL_ROUTE("linear_ce_bf16_fwd%s@r%ld", P.vecx && P.vecw ? "" : ":dword", ranges);
  hipLaunchKernelGGL(linear_ce_fwd_kernel, dim3((unsigned)grid), dim3(256), 0, s, x, w, target, (float*)ws, P);
  NNL_CHECK_LAUNCH();
  hipLaunchKernelGGL(linear_ce_finish_kernel, dim3((unsigned)nnl_cdiv(M, 256)), dim3(256), 0, s, (const float*)ws, target, lse, loss_rows, (long)M,
                     (long)N, (int)ranges, err_flag);
  NNL_CHECK_LAUNCH();
  hipLaunchKernelGGL(linear_ce_mean_kernel, dim3(1), dim3(256), 0, s, (const float*)loss_rows, loss_mean, (long)M);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}

extern "C" size_t nnl_linear_ce_bf16_bwd_workspace_bytes(int64_t M, int64_t N, int64_t K, int want_dx, int want_dw) {
  if (!in_domain(M, N, K)) return 0;
  return (want_dx ? part_bytes(slab_count(N, M), M, K) : 0) + (want_dw ? part_bytes(slab_count(M, N), N, K) : 0);
}

extern "C" int nnl_linear_ce_bf16_bwd(const float* x, const float* w, const int64_t* target, const float* lse, const float* g, float* dx, float* dw,
                                      int64_t M, int64_t N, int64_t K, int64_t ldx, int64_t ldw, void* ws, size_t ws_bytes, void* stream) {
  NNL_CHECK_ARG(in_domain(M, N, K), "linear_ce_bf16_bwd: M = %ld, N = %ld, K = %ld outside 0 < M, N < 2^31 - 256, 0 < K <= %d", (long)M, (long)N,
                (long)K, KMAX);
  NNL_CHECK_ARG(x && w && target && lse && g && (dx || dw), "linear_ce_bf16_bwd: null pointer");
  NNL_CHECK_ARG(ldx >= K && ldw >= K, "linear_ce_bf16_bwd: a row stride is shorter than its row (ldx %ld, ldw %ld, K %ld)", (long)ldx, (long)ldw,
                (long)K);
  const size_t dx_bytes = dx ? part_bytes(slab_count(N, M), M, K) : 0, dw_bytes = dw ? part_bytes(slab_count(M, N), N, K) : 0;
  if (dx_bytes + dw_bytes > 0 && (ws == nullptr || ws_bytes < dx_bytes + dw_bytes))
    return nnl_set_error(NNL_ERR_WORKSPACE, "linear_ce_bf16_bwd: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int vx = vec_ok(x, ldx), vw = vec_ok(w, ldw);
  NnlProfScope prof(NNL_PROF_GEMM, s, 4.0 * M * N * K * ((dx ? 1 : 0) + (dw ? 1 : 0)));
  if (dx) {
    BwdPlan P{M, N, K, M, N, ldx, ldw, slab_len(N, M), vx, vw};
    if (int e = launch_bwd<DX>(x, w, target, lse, g, dx, (float*)ws, P, s)) return e;
  }
  if (dw) {
    BwdPlan P{M, N, K, N, M, ldw, ldx, slab_len(M, N), vw, vx};
    if (int e = launch_bwd<DW>(w, x, target, lse, g, dw, (float*)((char*)ws + dx_bytes), P, s)) return e;
  }
  return NNL_OK;
}
