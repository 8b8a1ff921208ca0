// Operand staging of the bf16 matrix-core Linear family (linear_bf16.hip, linear_ce_bf16.hip): fp32 matrices in memory, rounded to bf16
// (nearest even, v_cvt_pk_bf16_f32) in registers on their way into LDS, read back as v_mfma_f32_32x32x16_bf16 fragments (a lane holds 8
// consecutive reduction indices of one operand row).
// A STREAMED tile is up to 128 operand rows x 32 reduction indices = 4 chunks of 8 bf16 (16 B) per row, row pitch 80 B (one pad chunk),
// chunk' = chunk ^ ((row >> 4) & 3).  ds_read_b128 is served 16 lanes at a time over a 256-B bank window: 16 consecutive rows share their
// swizzle and 80 r mod 256 takes 16 different multiples of 16: no conflicts.  An operand whose reduction axis is contiguous in memory
// (DIRECT) is staged one 16-B chunk per thread and row; one whose reduction axis is the ROW index of the matrix in memory (TRANSPOSED) is
// staged as 4 reduction rows x 4 columns per thread (a float4 per row, 32 lanes = 512 contiguous bytes), packed per column into 8 bytes
// (ds_write_b64): the swizzle spreads the 32 lanes of a half wave over 16 slots of 16 B and the other half wave (the odd reduction quad)
// takes the other 8 bytes of each: 2 passes for 512 B.  The tails of every axis are zero-filled while staging.  256 threads.
#pragma once
#include "nnl_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int BN = 128;                        // operand rows of a streamed tile (= columns of a forward tile, both sides of a backward tile)
constexpr int KS = 32;                         // reduction indices per step
constexpr int TP = 80;                         // bytes of a streamed tile row: 4 chunks + 1 pad
constexpr int TILEB = BN * TP;                 // bytes of one streamed tile

__device__ __forceinline__ unsigned pk_bf16(float a, float b) {
  bf16x2 t = {(__bf16)a, (__bf16)b};           // v_cvt_pk_bf16_f32: round to nearest even; a is the low half
  return __builtin_bit_cast(unsigned, t);
}

// p[0 .. 3] where they exist (`valid` elements from p on), zeros elsewhere; one float4 load when the operand allows it
__device__ __forceinline__ f32x4 load4(const float* __restrict__ p, long valid, bool vec) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (valid <= 0) return v;
  if (vec && valid >= 4) return *reinterpret_cast<const f32x4*>(p);
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < valid) v[j] = p[j];
  return v;
}

__device__ __forceinline__ u32x4 pack8(f32x4 a, f32x4 b) {
  return u32x4{pk_bf16(a[0], a[1]), pk_bf16(a[2], a[3]), pk_bf16(b[0], b[1]), pk_bf16(b[2], b[3])};
}

__device__ __forceinline__ int tile_off(int row, int chunk) { return row * TP + ((chunk ^ ((row >> 4) & 3)) * 16); }

__device__ __forceinline__ bf16x8 frag(const unsigned char* tile, int row, int chunk) {
  return *reinterpret_cast<const bf16x8*>(tile + tile_off(row, chunk));
}

// DIRECT operand: matrix rows row0 .. row0 + 64 H - 1 (those below nrows), reduction indices red0 .. red0 + 31 (those below red_end)
// contiguous in memory.  Thread t holds chunk t & 3 of rows t >> 2 and, for H = 2, 64 + (t >> 2).
template <int H = 2>
__device__ __forceinline__ void load_direct(const float* __restrict__ base, long ld, long row0, long nrows, long red0, long red_end, bool vec,
                                            f32x4 (&r)[2 * H]) {
  const int tid = threadIdx.x;
  const long red = red0 + (tid & 3) * 8;
#pragma unroll
  for (int h = 0; h < H; ++h) {
    const long row = row0 + (tid >> 2) + 64 * h;
    r[2 * h] = r[2 * h + 1] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (row < nrows) {
      const float* p = base + row * ld + red;
      r[2 * h] = load4(p, red_end - red, vec);
      r[2 * h + 1] = load4(p + 4, red_end - red - 4, vec);
    }
  }
}

template <int H = 2>
__device__ __forceinline__ void commit_direct(unsigned char* tile, const f32x4 (&r)[2 * H]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int h = 0; h < H; ++h) *reinterpret_cast<u32x4*>(tile + tile_off((tid >> 2) + 64 * h, tid & 3)) = pack8(r[2 * h], r[2 * h + 1]);
}

// TRANSPOSED operand: the reduction index is the matrix ROW (red0 .. red0 + 31, those below red_end), the operand rows are its columns
// col0 .. col0 + 127 (those below ncols).  Thread t holds reduction rows 4 (t >> 5) .. + 3 of columns 4 (t & 31) .. + 3.
__device__ __forceinline__ void load_trans(const float* __restrict__ base, long ld, long col0, long ncols, long red0, long red_end, bool vec,
                                           f32x4 (&r)[4]) {
  const int tid = threadIdx.x;
  const long col = col0 + (tid & 31) * 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long red = red0 + (tid >> 5) * 4 + i;
    r[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (red < red_end) r[i] = load4(base + red * ld + col, ncols - col, vec);
  }
}

__device__ __forceinline__ void commit_trans(unsigned char* tile, const f32x4 (&r)[4]) {
  const int tid = threadIdx.x, cq = tid & 31, pq = tid >> 5;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    *reinterpret_cast<u32x2*>(tile + tile_off(cq * 4 + j, pq >> 1) + (pq & 1) * 8) = u32x2{pk_bf16(r[0][j], r[1][j]), pk_bf16(r[2][j], r[3][j])};
}

bool vec_ok(const void* p, long ld) { return ((uintptr_t)p & 15) == 0 && ld % 4 == 0; }

const long DIM_MAX = (1L << 31) - 256;         // tile arithmetic on an axis stays inside an int

}  // namespace
