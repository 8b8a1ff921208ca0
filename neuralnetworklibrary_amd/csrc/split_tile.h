// The split schedule of the three 64x64-tile conv kernels (igemm_taps_kernel, wino_kernel, wino2_kernel), device side (the plan, its
// search and the binding to a launch: split_plan.h): which tile and k slice a workgroup owns, the hand-over of a split tile to its last
// arriver, the slab sum, and the float4 finish of output pieces with the BatchNorm partial statistics.  Functions that read schedule or
// epilogue fields are templates over the kernel's parameter struct: the three structs use the same field names (as split_bind does).
#pragma once
#include "igemm.h"

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int kSc1 = 1 << 4;         // gfx940+ cache policy bit: device (agent) scope — write-through stores / L2-bypassing loads

template <int POL>
__device__ __forceinline__ f32x4 buf_load4_policy(__amdgpu_buffer_rsrc_t rsrc, unsigned voff) {
  const i32x4 v = __builtin_bit_cast(i32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)voff, 0, POL));
  return __builtin_bit_cast(f32x4, v);
}
#define buf_load4_pol(rsrc, voff, pol) buf_load4_policy<pol>(rsrc, voff)


// ---- 1. tile decode: blockIdx.x -> the tile (`logical`) and the k slice `kslice` of `nslices` this workgroup computes.  Balanced
// schedule (p.bal; grid.x = n_main_tiles*main_ks + n_tail_tiles*tail_slices): main tiles first, XCD-remapped, then the tail tiles; a sliced
// tail tile's slab rows start at row0 = p.tail_row0 (in_tail).  Otherwise one whole tile per workgroup, XCD-remapped.
struct SplitTile {
  int logical, kslice, nslices, row0;
  bool in_tail;
};

template <class Params>
__device__ __forceinline__ SplitTile split_tile_decode(const Params& p) {
  SplitTile t{0, 0, 1, 0, false};
  if (p.bal) {
    const int nmb = p.n_main_tiles * p.main_ks;
    if ((int)blockIdx.x < nmb) {
      const int u = nnl_xcd_remap(blockIdx.x, nmb);
      t.logical = u / p.main_ks;
      t.kslice = u - t.logical * p.main_ks;
      t.nslices = p.main_ks;
    } else {
      const int tb = (int)blockIdx.x - nmb;
      const int tt = tb / p.tail_slices;
      t.kslice = tb - tt * p.tail_slices;
      t.logical = p.n_main_tiles + tt;
      t.nslices = p.tail_slices;
      if (t.nslices > 1) { t.row0 = p.tail_row0; t.in_tail = true; }
    }
  } else {
    t.logical = nnl_xcd_remap(blockIdx.x, gridDim.x);
  }
  return t;
}

// ---- 2. hand-over of a split tile.  Cross-workgroup hand-over WITHOUT cache-wide fences: a device-scope __threadfence() writes back and
// invalidates the whole L2 of the XCD (measured: 4x slower LSTM steps, W_hh loses its L2 residency).  Instead the caller has written its
// partial tile with agent-scope (sc1, write-through) stores; here every wave drains its stores (vmcnt 0) before the workgroup takes its
// ticket on the tile's counter (nobody ever waits, so no deadlock is possible), and the workgroup that draws the last ticket — the only one
// this returns true for — reads the slabs with agent-scope loads that bypass its own L2 (slab_sum4).  RESET: the counter is zero at rest
// (the finishing workgroup resets it); without it the caller zeroes the counters before every launch.  Call from uniform control flow.
template <bool RESET>
__device__ __forceinline__ bool split_tile_handover(int* counter, int nslices, int tid) {
  __shared__ int ticket;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) ticket = __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  if (ticket != nslices - 1) return false;         // someone else finishes this tile
  if (RESET && tid == 0) __hip_atomic_store(counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return true;
}

// ---- 3. slab sum: the float4 at element `off` of every slice's slab (slab s at s * sstride), added in slice order (deterministic whoever
// is last) with eight sc1 loads in flight per trip (a loop over single loads waits for every one of them)
__device__ __forceinline__ f32x4 slab_sum4(__amdgpu_buffer_rsrc_t rs, long off, long sstride, int nslices) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  for (int sl0 = 0; sl0 < nslices; sl0 += 8) {
    f32x4 part[8];
#pragma unroll
    for (int sl = 0; sl < 8; ++sl)
      if (sl0 + sl < nslices) part[sl] = buf_load4_pol(rs, (unsigned)(((long)(sl0 + sl) * sstride + off) * 4), kSc1);
#pragma unroll
    for (int sl = 0; sl < 8; ++sl)
      if (sl0 + sl < nslices) v += part[sl];
  }
  return v;
}

// ---- 4. finish of a float4 piece: + bias[boff..] + add[aoff..], activation (relu: 0 none, 1 ReLU, 2 sigmoid — SIG instantiations only) ...
template <bool SIG>
__device__ __forceinline__ f32x4 finish4(f32x4 v, const float* bias, long boff, const float* add, long aoff, int relu) {
  if (bias) v += *reinterpret_cast<const f32x4*>(bias + boff);
  if (add) v += *reinterpret_cast<const f32x4*>(add + aoff);
  if (relu == 1) { v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f); }
  else if (SIG && relu == 2) { v[0] = nnl_sigmoid(v[0]); v[1] = nnl_sigmoid(v[1]); v[2] = nnl_sigmoid(v[2]); v[3] = nnl_sigmoid(v[3]); }
  return v;
}

// ... stored at p.y + o (columns c4..c4+3), and, when the launch produces BatchNorm statistics, added to this thread's running sums of
// (y - pivot) and (y - pivot)^2 for its four columns
template <bool SIG, class Params>
__device__ __forceinline__ void finish_piece(const Params& p, f32x4 v, int c4, long o, float (&fs1)[4], float (&fs2)[4]) {
  v = finish4<SIG>(v, p.bias, c4, p.add, o, p.relu);
  *reinterpret_cast<f32x4*>(p.y + o) = v;
  if (p.bn_part) {
    const f32x4 pv = *reinterpret_cast<const f32x4*>(p.bn_pivot + c4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { const float d = v[e] - pv[e]; fs1[e] += d; fs2[e] += d * d; }
  }
}

// ---- 5. BatchNorm partials of a tile: thread t holds the sums of columns (t & 15)*4..+3 over its pieces (rows t>>4, +16, ...); the 16 row
// lanes of a column are added through `red` (LDS, [16 row lanes][64 cols][2] floats, free once the k loop is over) in a fixed order and
// written to p.bn_part[(tile_m * Nc + column) * 2 + {0, 1}].  No-op without p.bn_part; call from uniform control flow.
template <class Params>
__device__ __forceinline__ void bn_partials_write(const Params& p, const float (&fs1)[4], const float (&fs2)[4], float* red, int tid,
                                                  int tile_m, int n0) {
  if (!p.bn_part) return;
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    red[(((tid >> 4) * 64) + (tid & 15) * 4 + e) * 2 + 0] = fs1[e];
    red[(((tid >> 4) * 64) + (tid & 15) * 4 + e) * 2 + 1] = fs2[e];
  }
  __syncthreads();
  if (tid < 64 && n0 + tid < p.Nc) {
    float a = 0.f, b = 0.f;
    for (int r = 0; r < 16; ++r) { a += red[(r * 64 + tid) * 2]; b += red[(r * 64 + tid) * 2 + 1]; }
    p.bn_part[((long)tile_m * p.Nc + n0 + tid) * 2 + 0] = a;
    p.bn_part[((long)tile_m * p.Nc + n0 + tid) * 2 + 1] = b;
  }
}
