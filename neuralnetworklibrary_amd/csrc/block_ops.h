// Device-side wave and workgroup primitives shared by every kernel file: reductions, scans, the scalar sigmoid (gfx950, 64-lane waves).
//
// Every primitive combines its values in ONE fixed order, spelled out at its definition, so a result is the same bits on every call.
// A value is any trivially copyable type made of 32-bit words (float, double, int, unsigned long long, small structs); an operator is
// any callable T(T, T).  Where the operator is not commutative, its first argument is the earlier thread (or this lane, in a reduce).
//
// Barrier contract of the block-level primitives (nnl_block_reduce, nnl_block_tree_reduce, nnl_block_scan*), which every thread of
// the workgroup must call together:
//   * each begins with a barrier before it writes its scratch, so it assumes no synchronisation by the caller and may be called again
//     at once with the same scratch;
//   * each ends with every thread having read what it needs behind a second barrier, and leaves the scratch holding partials: a caller
//     that wants the scratch for something ELSE afterwards puts a barrier of its own in front of that.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

#ifndef NNL_WAVE
#define NNL_WAVE 64
#endif

__device__ __forceinline__ float nnl_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

struct NnlSum {
  template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct NnlMax {   // fmax for the floating types (a NaN loses), a > b ? a : b for the integers
  __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); }
  __device__ __forceinline__ double operator()(double a, double b) const { return fmax(a, b); }
  template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a > b ? a : b; }
};
struct NnlMin {
  __device__ __forceinline__ float operator()(float a, float b) const { return fminf(a, b); }
  __device__ __forceinline__ double operator()(double a, double b) const { return fmin(a, b); }
};

enum NnlShfl { NNL_SHFL_XOR, NNL_SHFL_UP, NNL_SHFL_DOWN };

// v of lane (lane ^ o), (lane - o) or (lane + o), word by word; up / down return the lane's own v where there is no such lane
template <NnlShfl MODE, class T>
__device__ __forceinline__ T nnl_shfl(T v, int o) {
  static_assert(std::is_trivially_copyable<T>::value && sizeof(T) % 4 == 0, "a value is a whole number of 32-bit words");
  int w[sizeof(T) / 4];
  __builtin_memcpy(w, &v, sizeof(T));
#pragma unroll
  for (unsigned i = 0; i < sizeof(T) / 4; ++i)
    w[i] = MODE == NNL_SHFL_XOR ? __shfl_xor(w[i], o, NNL_WAVE) : MODE == NNL_SHFL_UP ? __shfl_up(w[i], o, NNL_WAVE) : __shfl_down(w[i], o, NNL_WAVE);
  __builtin_memcpy(&v, w, sizeof(T));
  return v;
}

// ---- wave ----------------------------------------------------------------------------------------------------------------------------
// xor butterfly, distances 32 down to 1: every lane returns the result (the same bits in every lane when op is commutative)
template <class T, class Op>
__device__ __forceinline__ T nnl_wave_reduce(T v, Op op) {
#pragma unroll
  for (int o = NNL_WAVE / 2; o > 0; o >>= 1) v = op(v, nnl_shfl<NNL_SHFL_XOR>(v, o));
  return v;
}
template <class T> __device__ __forceinline__ T nnl_wave_sum(T v) { return nnl_wave_reduce(v, NnlSum()); }
template <class T> __device__ __forceinline__ T nnl_wave_max(T v) { return nnl_wave_reduce(v, NnlMax()); }
template <class T> __device__ __forceinline__ T nnl_wave_min(T v) { return nnl_wave_reduce(v, NnlMin()); }

// inclusive scan in lane order (Hillis-Steele, distances 1 up to 32).  REVERSE: over this lane and the LATER ones (a suffix scan)
template <bool REVERSE = false, class T, class Op>
__device__ __forceinline__ T nnl_wave_scan(T v, Op op) {
  const int lane = threadIdx.x & (NNL_WAVE - 1);
#pragma unroll
  for (int o = 1; o < NNL_WAVE; o <<= 1) {
    const T u = nnl_shfl<REVERSE ? NNL_SHFL_DOWN : NNL_SHFL_UP>(v, o);
    if (REVERSE ? lane + o < NNL_WAVE : lane >= o) v = REVERSE ? op(v, u) : op(u, v);
  }
  return v;
}

// ---- workgroup of WAVES waves ------------------------------------------------------------------------------------------------------------
enum NnlFold { NNL_FOLD_IN_ORDER, NNL_FOLD_PAIRWISE };

// wave butterfly, then the WAVES partials ((p0 + p1) + p2) + ... in every thread; NNL_FOLD_PAIRWISE (4 waves): (p0 + p1) + (p2 + p3)
template <int WAVES, NnlFold FOLD = NNL_FOLD_IN_ORDER, class T, class Op>
__device__ __forceinline__ T nnl_block_reduce(T v, Op op, T* lds /* [WAVES] */) {
  static_assert(FOLD == NNL_FOLD_IN_ORDER || WAVES == 4, "the pairwise fold is written for 4 waves");
  v = nnl_wave_reduce(v, op);
  __syncthreads();
  if ((threadIdx.x & (NNL_WAVE - 1)) == 0) lds[threadIdx.x / NNL_WAVE] = v;
  __syncthreads();
  if (FOLD == NNL_FOLD_PAIRWISE) return op(op(lds[0], lds[1]), op(lds[2], lds[3]));
  T r = lds[0];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) r = op(r, lds[w]);
  return r;
}

// LDS halving tree over N threads: red[t] += red[t + N/2], then N/4, ... 1; every thread returns red[0]
template <int N, class T, class Op>
__device__ __forceinline__ T nnl_block_tree_reduce(T v, Op op, T* red /* [N] */) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int w = N / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] = op(red[threadIdx.x], red[threadIdx.x + w]);
    __syncthreads();
  }
  return red[0];
}

// The scans' common part.  On return v = the wave's inclusive scan at this lane, total = the fold of all the waves' totals in wave
// order, and the result = the fold of the totals of the waves BEFORE this one (REVERSE: after it); both folds start from `identity`.
template <int WAVES, bool REVERSE, class T, class Op>
__device__ __forceinline__ T nnl_block_scan_carry(T& v, Op op, T identity, T* lds, T& total) {
  const int lane = threadIdx.x & (NNL_WAVE - 1), w = threadIdx.x / NNL_WAVE;
  v = nnl_wave_scan<REVERSE>(v, op);
  __syncthreads();
  if (lane == (REVERSE ? 0 : NNL_WAVE - 1)) lds[w] = v;
  __syncthreads();
  T carry = identity;
  total = identity;
#pragma unroll
  for (int j = 0; j < WAVES; ++j) {
    const T p = lds[j];
    if (REVERSE ? j > w : j < w) carry = op(carry, p);
    total = op(total, p);
  }
  return carry;
}

// inclusive scan in thread order (REVERSE: over this thread and the later ones); total = over the whole workgroup
template <int WAVES, bool REVERSE = false, class T, class Op>
__device__ __forceinline__ T nnl_block_scan(T v, Op op, T identity, T* lds /* [WAVES] */, T& total) {
  const T carry = nnl_block_scan_carry<WAVES, REVERSE>(v, op, identity, lds, total);
  return REVERSE ? op(v, carry) : op(carry, v);
}

// exclusive scan in thread order: over the threads BEFORE this one, `identity` for thread 0
template <int WAVES, class T, class Op>
__device__ __forceinline__ T nnl_block_scan_exclusive(T v, Op op, T identity, T* lds /* [WAVES] */, T& total) {
  const T carry = nnl_block_scan_carry<WAVES, false>(v, op, identity, lds, total);
  const T prev = nnl_shfl<NNL_SHFL_UP>(v, 1);
  return (threadIdx.x & (NNL_WAVE - 1)) == 0 ? carry : op(carry, prev);
}
