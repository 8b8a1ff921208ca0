// K22 opt-in bf16 matrix-core Linear: the language model's tied decoder (reference Applications/Text.py:572, [seq bs, emb] x [V, emb]^T) and the
// input projection gx = x w_ih^T of nn.LSTM (Text.py:495-513), with bf16 OPERANDS and fp32 accumulation, forward, dgrad and wgrad.  Every
// tensor stays fp32 in memory: an operand is rounded to bf16 (nearest even, v_cvt_pk_bf16_f32) in registers on its way into LDS, products
// run on v_mfma_f32_32x32x16_bf16 (a lane holds 8 consecutive reduction indices of one row), accumulators and epilogue are fp32.
// Domain: any M, N, K >= 1, explicit row strides (ldx, ldw >= K; ldy, lddy >= N).  Rows need not be 16-byte aligned (a logits row is 47 343
// floats): an operand whose pointer is 16-byte aligned and whose stride is a multiple of 4 is read with float4 loads, any other with dword
// loads; the tails of every axis are zero-filled while staging, so the MFMA loops carry no bounds test.
//
// LDS tiles: a STREAMED tile is 128 operand rows x 32 reduction indices = 4 chunks of 8 bf16 (16 B) per row, row pitch 80 B (one pad
//   chunk), chunk' = chunk ^ ((row >> 4) & 3).  ds_read_b128 is served 16 lanes at a time over a 256-B bank window: 16 consecutive rows share
//   their swizzle and 80 r mod 256 takes 16 different multiples of 16: no conflicts.  An operand whose reduction axis is contiguous in memory
//   (DIRECT: x and W in the forward, dy in the dgrad) is staged one 16-B chunk per thread and row; one whose reduction axis is the ROW index
//   of the matrix in memory (TRANSPOSED: W in the dgrad, dy and x in the wgrad) is staged as 4 reduction rows x 4 columns per thread (a
//   float4 per row, 32 lanes = 512 contiguous bytes), packed per column into 8 bytes (ds_write_b64): the swizzle spreads the 32 lanes of a
//   half wave over 16 slots of 16 B and the other half wave (the odd reduction quad) takes the other 8 bytes of each: 2 passes for 512 B.
// One kernel, linear_bf16_stream_kernel<MODE>: both operands streamed in 32-deep steps through two LDS buffers each (40 KB, three workgroups
//   per CU), register prefetch of the next step while the 8 MFMAs of this one run, one barrier per step; 128 x 128 output tile, 2 x 2 waves
//   of 64 x 64 (four accumulators), fp32 stored straight from the accumulators (32 lanes = 128 contiguous bytes).
//   FWD: y = rb(x) rb(W)^T (+ bias) (+ ReLU), both DIRECT, the sum over K never split; the column tile is the fastest grid index, so the
//     workgroups that run together share a row tile of x in L2.  (A variant that kept a 128-row bf16 panel of x resident in LDS for the whole K
//     and walked a run of column tiles was measured first: 106 KB of LDS leave one workgroup per CU and it ran at half the speed of this
//     kernel at K = 400 — 1487 against 803 us at the decoder — so it is not kept.)
//   DGRAD: dx[M,K] = rb(dy) rb(W), reduction over N; WGRAD: dW[N,K] = rb(dy)^T rb(x), reduction over M.  The reduction is cut into SLABS (a
//     multiple of 32, at least 512 deep, at most 16, as many as bring the grid to about 1024 workgroups): each slab writes its partial tile
//     to the workspace and linear_bf16_fold_kernel adds the slabs in slab order; one slab writes the result itself, with no workspace and
//     no fold.  The wgrad workgroups of the first k-tile column also sum the UNROUNDED dy they stage, per column in a fixed order (thread,
//     then the 8 reduction quads through LDS, then the slabs): the bias gradient.
// No atomics anywhere: two calls on the same inputs give the same bits.
#include "linear_bf16_tiles.h"

namespace {

constexpr int SLAB_MIN = 512;                  // fewest reduction indices per backward slab (a multiple of KS)
constexpr int SLAB_MAX = 16;                   // most slabs
constexpr int SPLIT_GRID = 1024;                 // slabs are added until the backward grid has about this many workgroups
static_assert(SLAB_MIN % KS == 0, "a slab is a whole number of steps");

struct StreamPlan {
  long R, C;                                   // the output matrix [R][C]: dgrad M x K, wgrad N x K
  long red, slab_len;                          // the reduction axis (dgrad N, wgrad M) and a slab's share of it (a multiple of KS)
  long lda, ldb;                               // row strides of the operands in memory: dgrad dy / W, wgrad dy / x, forward x / W
  int col_tiles, veca, vecb;
  long ldo;                                    // row stride of the output (C but for the forward's ldy)
  int relu;
};

enum { DGRAD = 0, WGRAD = 1, FWD = 2 };

// dgrad: a = dy [M][lda] (DIRECT: output rows are its rows), b = W [N][ldb] (TRANSPOSED: output columns are its columns).
// wgrad: a = dy [M][lda] (TRANSPOSED: output rows are its columns), b = x [M][ldb] (TRANSPOSED); dbias: per-slab column sums of dy or null.
// forward without a panel: a = x [M][lda] (DIRECT), b = W [N][ldb] (DIRECT: output columns are its rows), one slab; bias / ReLU epilogue.
template <int MODE>
__global__ __launch_bounds__(256) void linear_bf16_stream_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                 const float* __restrict__ bias, float* __restrict__ out,
                                                                 float* __restrict__ dbias, StreamPlan p) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[4 * TILEB];        // 2 x (a tile + b tile) = 40 KB
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1, half = lane >> 5, l31 = lane & 31;
  const int tr = blockIdx.x / p.col_tiles, tc = blockIdx.x - tr * p.col_tiles;
  const long r0 = (long)tr * BN, c0 = (long)tc * BN;
  const long red_begin = (long)blockIdx.y * p.slab_len, red_end = min(p.red, red_begin + p.slab_len);
  const bool sum_dy = MODE == WGRAD && dbias != nullptr && tc == 0;
  f32x4 ra[4], rb[4], dsum = {0.f, 0.f, 0.f, 0.f};
  auto load = [&](long red) {
    if (MODE == WGRAD) load_trans(a, p.lda, r0, p.R, red, red_end, p.veca, ra);
    else load_direct(a, p.lda, r0, p.R, red, red_end, p.veca, ra);
    if (MODE == FWD) load_direct(b, p.ldb, c0, p.C, red, red_end, p.vecb, rb);
    else load_trans(b, p.ldb, c0, p.C, red, red_end, p.vecb, rb);
  };
  auto commit = [&](int buf) {
    unsigned char* base = smem + buf * 2 * TILEB;
    if (MODE == WGRAD) {
      commit_trans(base, ra);
      if (sum_dy) dsum += (ra[0] + ra[1]) + (ra[2] + ra[3]);         // unrounded, 4 columns of this thread's 4 rows: a fixed order
    } else {
      commit_direct(base, ra);
    }
    if (MODE == FWD) commit_direct(base + TILEB, rb);
    else commit_trans(base + TILEB, rb);
  };
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  load(red_begin);
  commit(0);
  __syncthreads();
  int cur = 0;
  for (long red = red_begin; red < red_end; red += KS) {
    const bool more = red + KS < red_end;
    if (more) load(red + KS);                                       // in flight while the MFMAs below run
    const unsigned char* base = smem + cur * 2 * TILEB;
#pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
      const int ch = 2 * kh + half;
      bf16x8 fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) fa[i] = frag(base, (wm * 2 + i) * 32 + l31, ch);
#pragma unroll
      for (int j = 0; j < 2; ++j) fb[j] = frag(base + TILEB, (wn * 2 + j) * 32 + l31, ch);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
    if (more) commit(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  }
  float* o = out + (long)blockIdx.y * p.R * p.C;                    // the slab's partial in the workspace; one slab: the result itself
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const long col = c0 + (wn * 2 + j) * 32 + l31;
      const float bv = (MODE == FWD && bias != nullptr && col < p.C) ? bias[col] : 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const long row = r0 + (wm * 2 + i) * 32 + (e & 3) + 8 * (e >> 2) + 4 * half;
        float v = acc[i][j][e];
        if (MODE == FWD) {
          v += bv;
          if (p.relu) v = fmaxf(v, 0.f);
        }
        if (row < p.R && col < p.C) o[row * p.ldo + col] = v;
      }
    }
  if (sum_dy) {                                                     // (uniform per workgroup; the loop ended with a barrier: smem is free)
    float* part = reinterpret_cast<float*>(smem);                   // [8 reduction quads][128 columns]
    *reinterpret_cast<f32x4*>(part + (tid >> 5) * BN + (tid & 31) * 4) = dsum;
    __syncthreads();
    if (tid < BN && r0 + tid < p.R) {
      float s = part[tid];
#pragma unroll
      for (int q = 1; q < 8; ++q) s += part[q * BN + tid];
      dbias[(long)blockIdx.y * p.R + r0 + tid] = s;
    }
  }
}

__global__ __launch_bounds__(256) void linear_bf16_fold_kernel(const float* __restrict__ part, float* __restrict__ out, long numel, int slabs) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= numel) return;
  float s = part[i];
  for (int sl = 1; sl < slabs; ++sl) s += part[(long)sl * numel + i];            // slab order: fixed
  out[i] = s;
}

int check_dims(const char* who, int64_t M, int64_t N, int64_t K) {
  NNL_CHECK_ARG(M > 0 && N > 0 && K > 0, "%s: M = %ld, N = %ld, K = %ld must be positive", who, (long)M, (long)N, (long)K);
  NNL_CHECK_ARG(M < DIM_MAX && N < DIM_MAX && K < DIM_MAX, "%s: a dimension of 2^31 or more", who);
  return NNL_OK;
}

// a backward reduction of `red` indices over `tiles` output tiles: the slab length (a multiple of KS, at least SLAB_MIN)
long slab_len(long red, long tiles) {
  long want = SPLIT_GRID / tiles;
  want = want < 1 ? 1 : (want > SLAB_MAX ? SLAB_MAX : want);
  const long len = nnl_cdiv(nnl_cdiv(red, want), KS) * KS;
  return len > SLAB_MIN ? len : SLAB_MIN;
}

long tile_count(long R, long C) { return nnl_cdiv(R, BN) * nnl_cdiv(C, BN); }

int fold(const float* part, float* out, long numel, long slabs, hipStream_t s) {
  hipLaunchKernelGGL(linear_bf16_fold_kernel, dim3((unsigned)nnl_cdiv(numel, 256)), dim3(256), 0, s, part, out, numel, (int)slabs);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}

}  // namespace

extern "C" int nnl_linear_bf16_fwd(const float* x, const float* w, const float* bias, float* y, int64_t M, int64_t N, int64_t K, int64_t ldx,
                                   int64_t ldw, int64_t ldy, int relu, void* stream) {
  if (int e = check_dims("linear_bf16_fwd", M, N, K)) return e;
  NNL_CHECK_ARG(x && w && y, "linear_bf16_fwd: null pointer");
  NNL_CHECK_ARG(ldx >= K && ldw >= K && ldy >= N, "linear_bf16_fwd: a row stride is shorter than its row (ldx %ld, ldw %ld, K %ld; ldy %ld, N %ld)",
                (long)ldx, (long)ldw, (long)K, (long)ldy, (long)N);
  const long tiles = tile_count(M, N);
  NNL_CHECK_ARG(tiles < DIM_MAX, "linear_bf16_fwd: too many tiles");
  StreamPlan P{M, N, K, nnl_cdiv(K, KS) * KS, ldx, ldw, (int)nnl_cdiv(N, BN), vec_ok(x, ldx), vec_ok(w, ldw), ldy, relu ? 1 : 0};   // one slab: the sum is never split
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_GEMM, s, 2.0 * M * N * K);
  NNL_ROUTE("linear_bf16_fwd%s", P.veca && P.vecb ? "" : ":dword");
  hipLaunchKernelGGL(linear_bf16_stream_kernel<FWD>, dim3((unsigned)tiles), dim3(256), 0, s, x, w, bias, y, (float*)nullptr, P);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}

extern "C" size_t nnl_linear_bf16_dgrad_workspace_bytes(int64_t M, int64_t N, int64_t K) {
  if (M <= 0 || N <= 0 || K <= 0 || M >= DIM_MAX || N >= DIM_MAX || K >= DIM_MAX) return 0;
  const long slabs = nnl_cdiv(N, slab_len(N, tile_count(M, K)));
  return slabs > 1 ? (size_t)slabs * M * K * sizeof(float) : 0;
}

extern "C" int nnl_linear_bf16_dgrad(const float* dy, const float* w, float* dx, int64_t M, int64_t N, int64_t K, int64_t lddy, int64_t ldw,
                                     void* ws, size_t ws_bytes, void* stream) {
  if (int e = check_dims("linear_bf16_dgrad", M, N, K)) return e;
  NNL_CHECK_ARG(dy && w && dx, "linear_bf16_dgrad: null pointer");
  NNL_CHECK_ARG(lddy >= N && ldw >= K, "linear_bf16_dgrad: a row stride is shorter than its row (lddy %ld, N %ld; ldw %ld, K %ld)", (long)lddy,
                (long)N, (long)ldw, (long)K);
  const long tiles = tile_count(M, K), len = slab_len(N, tiles), slabs = nnl_cdiv(N, len);
  NNL_CHECK_ARG(tiles < DIM_MAX, "linear_bf16_dgrad: too many tiles");
  if (slabs > 1 && (ws == nullptr || ws_bytes < (size_t)slabs * M * K * sizeof(float)))
    return nnl_set_error(NNL_ERR_WORKSPACE, "linear_bf16_dgrad: workspace too small");
  StreamPlan P{M, K, N, len, lddy, ldw, (int)nnl_cdiv(K, BN), vec_ok(dy, lddy), vec_ok(w, ldw), K, 0};
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_GEMM, s, 2.0 * M * N * K);
  NNL_ROUTE("linear_bf16_dgrad%s@s%ld", P.veca && P.vecb ? "" : ":dword", slabs);
  hipLaunchKernelGGL(linear_bf16_stream_kernel<DGRAD>, dim3((unsigned)tiles, (unsigned)slabs), dim3(256), 0, s, dy, w, (const float*)nullptr,
                     slabs > 1 ? (float*)ws : dx, (float*)nullptr, P);
  NNL_CHECK_LAUNCH();
  return slabs > 1 ? fold((const float*)ws, dx, (long)M * K, slabs, s) : NNL_OK;
}

extern "C" size_t nnl_linear_bf16_wgrad_workspace_bytes(int64_t M, int64_t N, int64_t K) {
  if (M <= 0 || N <= 0 || K <= 0 || M >= DIM_MAX || N >= DIM_MAX || K >= DIM_MAX) return 0;
  const long slabs = nnl_cdiv(M, slab_len(M, tile_count(N, K)));
  return slabs > 1 ? (size_t)slabs * (N * K + N) * sizeof(float) : 0;
}

extern "C" int nnl_linear_bf16_wgrad(const float* x, const float* dy, float* dw, float* db, int64_t M, int64_t N, int64_t K, int64_t ldx,
                                     int64_t lddy, void* ws, size_t ws_bytes, void* stream) {
  if (int e = check_dims("linear_bf16_wgrad", M, N, K)) return e;
  NNL_CHECK_ARG(x && dy && dw, "linear_bf16_wgrad: null pointer");
  NNL_CHECK_ARG(ldx >= K && lddy >= N, "linear_bf16_wgrad: a row stride is shorter than its row (ldx %ld, K %ld; lddy %ld, N %ld)", (long)ldx,
                (long)K, (long)lddy, (long)N);
  const long tiles = tile_count(N, K), len = slab_len(M, tiles), slabs = nnl_cdiv(M, len), numel = (long)N * K;
  NNL_CHECK_ARG(tiles < DIM_MAX, "linear_bf16_wgrad: too many tiles");
  if (slabs > 1 && (ws == nullptr || ws_bytes < (size_t)slabs * (numel + N) * sizeof(float)))
    return nnl_set_error(NNL_ERR_WORKSPACE, "linear_bf16_wgrad: workspace too small");
  StreamPlan P{N, K, M, len, lddy, ldx, (int)nnl_cdiv(K, BN), vec_ok(dy, lddy), vec_ok(x, ldx), K, 0};
  float* dw_part = slabs > 1 ? (float*)ws : dw;                     // [slabs][N][K], then the bias partials [slabs][N]
  float* db_part = db == nullptr ? nullptr : (slabs > 1 ? (float*)ws + slabs * numel : db);
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_GEMM, s, 2.0 * M * N * K);
  NNL_ROUTE("linear_bf16_wgrad%s%s@s%ld", P.veca && P.vecb ? "" : ":dword", db ? ":db" : "", slabs);
  hipLaunchKernelGGL(linear_bf16_stream_kernel<WGRAD>, dim3((unsigned)tiles, (unsigned)slabs), dim3(256), 0, s, dy, x, (const float*)nullptr, dw_part,
                     db_part, P);
  NNL_CHECK_LAUNCH();
  if (slabs > 1) {
    if (int e = fold(dw_part, dw, numel, slabs, s)) return e;
    if (db != nullptr) return fold(db_part, db, N, slabs, s);
  }
  return NNL_OK;
}
