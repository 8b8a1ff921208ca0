// K15 squeeze-and-excitation tail of the SENet blocks (reference Applications/VisionModels/senet.py:118-137 SEModule, :161-162 the
// block's `+ residual` and ReLU), NHWC fp32, all HBM-bound:
//   out = relu( x * sigmoid(z[n, c]) + residual ),   z = fc2(relu(fc1(mean_hw(x))))   (the two FCs are GEMMs: ops.linear)
//   * squeeze       m[n, c] = mean over the HW pixels: four pixel lanes per channel, each summing its pixels in order, added in lane order;
//   * excite fwd    one pass, 16-byte accesses, the sigmoid recomputed per element from the [N, C] logits;
//   * excite bwd    g = dy * [out > 0]; dres = g; dx = g * sigmoid(z); dz[n, c] = sigmoid'(z) * sum_h g * x.  One thread owns a channel
//                   of one image for its pixel lane, the sum runs in fp64 in a fixed order (no atomics): dz is rounded once;
//   * squeeze bwd   dx += dm[n, c] / HW (the mean's gradient reaches every pixel), a second small pass once the FCs' backward gave dm.
// Algorithmic bytes: squeeze 4 * in; excite fwd 4 * (x + residual + out); excite bwd 4 * (dy + out + x + dx + dres); squeeze bwd 8 * dx.
#include "nnl_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));


// block = 256 threads = 64 channel lanes x 4 pixel lanes; grid = (ceil(C/64), N)
__global__ __launch_bounds__(256) void se_squeeze_kernel(const float* __restrict__ x, float* __restrict__ m, int HW, int C) {
  __shared__ float ssum[4][64];
  const int cl = threadIdx.x & 63, pl = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl, n = blockIdx.y;
  float s = 0.f;
  if (c < C)
    for (int p = pl; p < HW; p += 4) s += x[((long)n * HW + p) * C + c];
  ssum[pl][cl] = s;
  __syncthreads();
  if (pl == 0 && c < C) m[(long)n * C + c] = (((ssum[0][cl] + ssum[1][cl]) + ssum[2][cl]) + ssum[3][cl]) / (float)HW;
}

__global__ __launch_bounds__(256) void se_excite_fwd_kernel(const float* __restrict__ x, const float* __restrict__ z,
                                                            const float* __restrict__ res, float* __restrict__ out, long total4,
                                                            long hw_c4, int C4) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (long)gridDim.x * blockDim.x) {
    const int c4 = (int)(i % C4);
    const long n = i / hw_c4;
    const f32x4 xv = reinterpret_cast<const f32x4*>(x)[i];
    const f32x4 zv = reinterpret_cast<const f32x4*>(z)[n * C4 + c4];
    f32x4 r = {0.f, 0.f, 0.f, 0.f};
    if (res != nullptr) r = reinterpret_cast<const f32x4*>(res)[i];
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = fmaxf(xv[e] * nnl_sigmoid(zv[e]) + r[e], 0.f);
    reinterpret_cast<f32x4*>(out)[i] = o;
  }
}

// block = 64 channel lanes x 4 pixel lanes; grid = (ceil(C/64), N)
__global__ __launch_bounds__(256) void se_excite_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ out,
                                                            const float* __restrict__ x, const float* __restrict__ z,
                                                            float* __restrict__ dx, float* __restrict__ dres, float* __restrict__ dz,
                                                            int HW, int C) {
  __shared__ double ssum[4][64];
  const int cl = threadIdx.x & 63, pl = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl, n = blockIdx.y;
  double acc = 0.0, sig = 0.0;
  if (c < C) {
    sig = 1.0 / (1.0 + exp(-(double)z[(long)n * C + c]));
    const float sf = (float)sig;
    for (int p = pl; p < HW; p += 4) {
      const long i = ((long)n * HW + p) * C + c;
      const float g = out[i] > 0.f ? dy[i] : 0.f;
      if (dres != nullptr) dres[i] = g;
      dx[i] = g * sf;
      acc += (double)g * (double)x[i];
    }
  }
  ssum[pl][cl] = acc;
  __syncthreads();
  if (pl == 0 && c < C)
    dz[(long)n * C + c] = (float)(sig * (1.0 - sig) * (((ssum[0][cl] + ssum[1][cl]) + ssum[2][cl]) + ssum[3][cl]));
}

__global__ __launch_bounds__(256) void se_squeeze_bwd_kernel(const float* __restrict__ dm, float* __restrict__ dx, long total4, long hw_c4,
                                                             int C4, float hw) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (long)gridDim.x * blockDim.x) {
    const int c4 = (int)(i % C4);
    const long n = i / hw_c4;
    const f32x4 d = reinterpret_cast<const f32x4*>(dm)[n * C4 + c4];
    f32x4 v = reinterpret_cast<f32x4*>(dx)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] += d[e] / hw;
    reinterpret_cast<f32x4*>(dx)[i] = v;
  }
}

int ew_blocks(long total) {
  long b = nnl_cdiv(total, 256);
  if (b > 65536) b = 65536;
  return (int)(b < 1 ? 1 : b);
}

bool se_sizes_ok(int64_t N, int64_t HW, int64_t C) {
  return N > 0 && HW > 0 && C > 0 && N < 65536 && HW < (1L << 30) && C < (1L << 22) && N * HW * C < (1L << 40);
}

}  // namespace

extern "C" int nnl_se_squeeze(const float* x, float* m, int64_t N, int64_t HW, int64_t C, void* stream) {
  NNL_CHECK_ARG(x && m && se_sizes_ok(N, HW, C), "se_squeeze: bad argument");
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_ELEMENTWISE, s, 4.0 * N * HW * C);
  hipLaunchKernelGGL(se_squeeze_kernel, dim3((unsigned)nnl_cdiv(C, 64), (unsigned)N), dim3(256), 0, s, x, m, (int)HW, (int)C);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}

extern "C" int nnl_se_excite_fwd(const float* x, const float* z, const float* residual, float* out, int64_t N, int64_t HW, int64_t C,
                                 void* stream) {
  NNL_CHECK_ARG(x && z && out && se_sizes_ok(N, HW, C) && C % 4 == 0, "se_excite_fwd: bad argument (C %% 4 == 0)");
  hipStream_t s = (hipStream_t)stream;
  const long total4 = N * HW * (C / 4);
  NnlProfScope prof(NNL_PROF_ELEMENTWISE, s, (residual ? 12.0 : 8.0) * N * HW * C);
  hipLaunchKernelGGL(se_excite_fwd_kernel, dim3(ew_blocks(total4)), dim3(256), 0, s, x, z, residual, out, total4, (long)(HW * (C / 4)),
                     (int)(C / 4));
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}

extern "C" int nnl_se_excite_bwd(const float* dy, const float* out, const float* x, const float* z, float* dx, float* dres, float* dz,
                                 int64_t N, int64_t HW, int64_t C, void* stream) {
  NNL_CHECK_ARG(dy && out && x && z && dx && dz && se_sizes_ok(N, HW, C), "se_excite_bwd: bad argument");
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_ELEMENTWISE, s, (dres ? 20.0 : 16.0) * N * HW * C);
  hipLaunchKernelGGL(se_excite_bwd_kernel, dim3((unsigned)nnl_cdiv(C, 64), (unsigned)N), dim3(256), 0, s, dy, out, x, z, dx, dres, dz,
                     (int)HW, (int)C);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}

extern "C" int nnl_se_squeeze_bwd(const float* dm, float* dx, int64_t N, int64_t HW, int64_t C, void* stream) {
  NNL_CHECK_ARG(dm && dx && se_sizes_ok(N, HW, C) && C % 4 == 0, "se_squeeze_bwd: bad argument (C %% 4 == 0)");
  hipStream_t s = (hipStream_t)stream;
  const long total4 = N * HW * (C / 4);
  NnlProfScope prof(NNL_PROF_ELEMENTWISE, s, 8.0 * N * HW * C);
  hipLaunchKernelGGL(se_squeeze_bwd_kernel, dim3(ew_blocks(total4)), dim3(256), 0, s, dm, dx, total4, (long)(HW * (C / 4)), (int)(C / 4),
                     (float)HW);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}
