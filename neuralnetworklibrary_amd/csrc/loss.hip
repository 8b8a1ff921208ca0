// nn.MSELoss(reduction='mean') — the 'cont' loss of General/Learner.py:20 (`loss_func_dict['cont']`) that closes the collaborative-
// filtering and structured-data steps — and nn.BCEWithLogitsLoss() — the 'multi_label' loss of the same line, which
// closes the multi-label image step.  A 64 - 1024 sample step is launch-bound: ATen runs either loss as an elementwise kernel + a
// reduction forward and one or more backward; here the forward is ONE launch for up to 65 536 elements (a single 1024-thread
// block, fixed-order tree: bitwise reproducible), two above that, and the backward one elementwise launch that takes the upstream
// scalar gradient from device memory (no host sync).  The F-beta metric of General/LossesMetrics.py:70-78 sits at the end of the file.
#include "nnl_common.h"

namespace {

constexpr int kLossBlock = 1024;
constexpr long kLossOneBlock = 65536;
constexpr int kLossMaxBlocks = 256;

struct SqErr {   // (a - b)^2
  __device__ __forceinline__ float operator()(float a, float b) const {
    const float d = a - b;
    return d * d;
  }
};
struct BceLogits {   // max(x, 0) - x t + log1p(exp(-|x|)): no overflow for any finite x, targets anywhere in [0, 1]
  __device__ __forceinline__ float operator()(float x, float t) const { return (fmaxf(x, 0.f) - x * t) + log1pf(expf(-fabsf(x))); }
};

// one block: out[0] = scale * sum term(a, b);  several blocks: part[blockIdx.x] = its share (scale applied by loss_final_kernel)
template <class Term>
__global__ __launch_bounds__(kLossBlock) void loss_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out,
                                                               long n, float scale) {
  __shared__ float red[kLossBlock];
  const Term term;
  float acc = 0.f;
  for (long i = (long)blockIdx.x * kLossBlock + threadIdx.x; i < n; i += (long)gridDim.x * kLossBlock) acc += term(a[i], b[i]);
  const float s = nnl_block_tree_reduce<kLossBlock>(acc, NnlSum(), red);
  if (threadIdx.x == 0) out[blockIdx.x] = gridDim.x == 1 ? s * scale : s;
}

__global__ __launch_bounds__(kLossBlock) void loss_final_kernel(const float* __restrict__ part, int nparts, float* __restrict__ out, float scale) {
  __shared__ float red[kLossBlock];
  const float s = nnl_block_tree_reduce<kLossBlock>((int)threadIdx.x < nparts ? part[threadIdx.x] : 0.f, NnlSum(), red);
  if (threadIdx.x == 0) out[0] = s * scale;
}

__global__ __launch_bounds__(256) void mse_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ gout,
                                                       float* __restrict__ da, long n, float scale) {
  const float g = (gout ? gout[0] : 1.f) * scale;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) da[i] = g * (a[i] - b[i]);
}

// dx = (sigmoid(x) - t) * g.  vec: all three pointers 16-byte aligned -> float4 body, scalar tail of n % 4
__global__ __launch_bounds__(256) void bce_logits_bwd_kernel(const float* __restrict__ x, const float* __restrict__ t, const float* __restrict__ gout,
                                                              float* __restrict__ dx, long n, float scale, int vec) {
  const float g = (gout ? gout[0] : 1.f) * scale;
  const long tid = (long)blockIdx.x * 256 + threadIdx.x, nthreads = (long)gridDim.x * 256;
  const long n4 = vec ? n / 4 : 0;
  for (long i = tid; i < n4; i += nthreads) {
    const float4 xv = reinterpret_cast<const float4*>(x)[i], tv = reinterpret_cast<const float4*>(t)[i];
    float4 d;
    d.x = g * (nnl_sigmoid(xv.x) - tv.x);
    d.y = g * (nnl_sigmoid(xv.y) - tv.y);
    d.z = g * (nnl_sigmoid(xv.z) - tv.z);
    d.w = g * (nnl_sigmoid(xv.w) - tv.w);
    reinterpret_cast<float4*>(dx)[i] = d;
  }
  for (long i = n4 * 4 + tid; i < n; i += nthreads) dx[i] = g * (nnl_sigmoid(x[i]) - t[i]);
}

template <class Term>
int loss_fwd(const char* what, const float* a, const float* b, float* loss, int64_t n, void* workspace, size_t workspace_bytes, hipStream_t s) {
  const float scale = 1.f / (float)n;
  if (n <= kLossOneBlock) {
    hipLaunchKernelGGL(loss_fwd_kernel<Term>, dim3(1), dim3(kLossBlock), 0, s, a, b, loss, (long)n, scale);
    NNL_CHECK_LAUNCH();
    return NNL_OK;
  }
  if (workspace == nullptr || workspace_bytes < (size_t)kLossMaxBlocks * sizeof(float)) return nnl_set_error(NNL_ERR_WORKSPACE, "%s: workspace too small", what);
  long blocks = nnl_cdiv(n, (long)kLossBlock * 8);
  if (blocks > kLossMaxBlocks) blocks = kLossMaxBlocks;
  hipLaunchKernelGGL(loss_fwd_kernel<Term>, dim3((unsigned)blocks), dim3(kLossBlock), 0, s, a, b, (float*)workspace, (long)n, scale);
  NNL_CHECK_LAUNCH();
  hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(kLossBlock), 0, s, (const float*)workspace, (int)blocks, loss, scale);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}

}  // namespace

extern "C" size_t nnl_mse_workspace_bytes(int64_t n) { return n > kLossOneBlock ? (size_t)kLossMaxBlocks * sizeof(float) : 0; }

extern "C" int nnl_mse_fwd(const float* pred, const float* target, float* loss, int64_t n, void* workspace, size_t workspace_bytes,
                           void* stream) {
  NNL_CHECK_ARG(pred && target && loss && n > 0, "mse_fwd: bad argument");
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_ELEMENTWISE, s, 8.0 * n);
  return loss_fwd<SqErr>("mse_fwd", pred, target, loss, n, workspace, workspace_bytes, s);
}

extern "C" int nnl_mse_bwd(const float* pred, const float* target, const float* grad_out, float* dpred, int64_t n, void* stream) {
  NNL_CHECK_ARG(pred && target && dpred && n > 0, "mse_bwd: bad argument");
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_ELEMENTWISE, s, 12.0 * n);
  long blocks = nnl_cdiv(n, 256L * 4);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(mse_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, s, pred, target, grad_out, dpred, (long)n, 2.f / (float)n);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}

// ---- nn.BCEWithLogitsLoss() (General/Learner.py:20, `loss_func_dict['multi_label']`) ----
extern "C" size_t nnl_bce_logits_workspace_bytes(int64_t n) { return nnl_mse_workspace_bytes(n); }

extern "C" int nnl_bce_logits_fwd(const float* logits, const float* target, float* loss, int64_t n, void* workspace, size_t workspace_bytes,
                                  void* stream) {
  NNL_CHECK_ARG(logits && target && loss && n > 0, "bce_logits_fwd: bad argument");
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_ELEMENTWISE, s, 8.0 * n);
  return loss_fwd<BceLogits>("bce_logits_fwd", logits, target, loss, n, workspace, workspace_bytes, s);
}

extern "C" int nnl_bce_logits_bwd(const float* logits, const float* target, const float* grad_out, float* dlogits, int64_t n, void* stream) {
  NNL_CHECK_ARG(logits && target && dlogits && n > 0, "bce_logits_bwd: bad argument");
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_ELEMENTWISE, s, 12.0 * n);
  const int vec = (((uintptr_t)logits | (uintptr_t)target | (uintptr_t)dlogits) & 15) == 0;
  long blocks = nnl_cdiv(n, 256L * 4);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(bce_logits_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, s, logits, target, grad_out, dlogits, (long)n, 1.f / (float)n, vec);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}

// ---- FullyConnectedNet's 'sigmoidal' output activation (reference General/Layers.py:150-152): y = lo + (hi - lo) * sigmoid(x) ----
// three ATen kernels forward and three backward on a [bs, 1] tensor; here one each.  The forward also keeps s = sigmoid(x), so the
// backward is torch's own formula dx = dy * (hi - lo) * s * (1 - s) (re-deriving s from y would lose its low bits near lo).
namespace {
__global__ __launch_bounds__(256) void scaled_sigmoid_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, float* __restrict__ sg, long n,
                                                                  float lo, float hi) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float s = nnl_sigmoid(x[i]);
    sg[i] = s;
    y[i] = lo + (hi - lo) * s;
  }
}
__global__ __launch_bounds__(256) void scaled_sigmoid_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ sg, float* __restrict__ dx,
                                                                  long n, float lo, float hi) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float s = sg[i];
    dx[i] = (dy[i] * (hi - lo)) * ((1.f - s) * s);
  }
}
}  // namespace

extern "C" int nnl_scaled_sigmoid_fwd(const float* x, float* y, float* sig, int64_t n, float lo, float hi, void* stream) {
  NNL_CHECK_ARG(x && y && sig && n > 0 && hi != lo, "scaled_sigmoid_fwd: bad argument");
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_ELEMENTWISE, s, 8.0 * n);
  long blocks = nnl_cdiv(n, 256L * 4);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(scaled_sigmoid_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, y, sig, (long)n, lo, hi);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}

extern "C" int nnl_scaled_sigmoid_bwd(const float* dy, const float* sig, float* dx, int64_t n, float lo, float hi, void* stream) {
  NNL_CHECK_ARG(dy && sig && dx && n > 0 && hi != lo, "scaled_sigmoid_bwd: bad argument");
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_ELEMENTWISE, s, 12.0 * n);
  long blocks = nnl_cdiv(n, 256L * 4);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(scaled_sigmoid_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, s, dy, sig, dx, (long)n, lo, hi);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}

// ---- fbeta_loss.__call__ (General/LossesMetrics.py:70-78): the multi-label F-beta metric, which the Planet notebook evaluates at five
// thresholds per validation minibatch (a dozen ATen launches each).  One wave per row: the lanes stride over the C columns and a
// butterfly adds them (sums of 0/1 products: exact); the row arithmetic is torch's, operation for operation, in fp32; every wave adds
// its rows' scores in row order and the block adds its 16 waves in wave order, so the mean is bitwise reproducible.
namespace {

constexpr int kFbetaWaves = kLossBlock / NNL_WAVE;
constexpr long kFbetaOneBlockRows = 4096;

__global__ __launch_bounds__(kLossBlock) void fbeta_kernel(const float* __restrict__ pred, const float* __restrict__ target, float* __restrict__ out,
                                                            long N, long C, float beta2, float threshold, int use_thresh, float eps, float scale) {
  __shared__ float red[kFbetaWaves];
  const int wave = threadIdx.x / NNL_WAVE, lane = threadIdx.x % NNL_WAVE;
  float acc = 0.f;
  for (long r = (long)blockIdx.x * kFbetaWaves + wave; r < N; r += (long)gridDim.x * kFbetaWaves) {
    float tp = 0.f, sp = 0.f, st = 0.f;
    for (long c = lane; c < C; c += NNL_WAVE) {
      const float x = pred[r * C + c], t = target[r * C + c];
      const float p = use_thresh ? (nnl_sigmoid(x) >= threshold ? 1.f : 0.f) : x;
      tp += p * t;
      sp += p;
      st += t;
    }
    tp = nnl_wave_sum(tp);
    sp = nnl_wave_sum(sp);
    st = nnl_wave_sum(st);
    const float p = tp / (sp + eps), rc = tp / (st + eps);
    acc += ((1.f + beta2) * (p * rc)) / ((beta2 * p + rc) + eps);
  }
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int w = 0; w < kFbetaWaves; ++w) s += red[w];
    out[blockIdx.x] = gridDim.x == 1 ? s * scale : s;
  }
}

}  // namespace

extern "C" size_t nnl_fbeta_workspace_bytes(int64_t N, int64_t C) {
  (void)C;
  return N > kFbetaOneBlockRows ? (size_t)kLossMaxBlocks * sizeof(float) : 0;
}

extern "C" int nnl_fbeta(const float* pred, const float* target, float* out, int64_t N, int64_t C, float beta2, float threshold, int use_thresh,
                         float eps, void* workspace, size_t workspace_bytes, void* stream) {
  NNL_CHECK_ARG(pred && target && out && N > 0 && C > 0, "fbeta: bad argument");
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_ELEMENTWISE, s, 8.0 * N * C);
  const float scale = 1.f / (float)N;
  if (N <= kFbetaOneBlockRows) {
    hipLaunchKernelGGL(fbeta_kernel, dim3(1), dim3(kLossBlock), 0, s, pred, target, out, (long)N, (long)C, beta2, threshold, use_thresh, eps, scale);
    NNL_CHECK_LAUNCH();
    return NNL_OK;
  }
  if (workspace == nullptr || workspace_bytes < nnl_fbeta_workspace_bytes(N, C)) return nnl_set_error(NNL_ERR_WORKSPACE, "fbeta: workspace too small");
  long blocks = nnl_cdiv(N, (long)kFbetaWaves * 16);
  if (blocks > kLossMaxBlocks) blocks = kLossMaxBlocks;
  hipLaunchKernelGGL(fbeta_kernel, dim3((unsigned)blocks), dim3(kLossBlock), 0, s, pred, target, (float*)workspace, (long)N, (long)C, beta2, threshold,
                     use_thresh, eps, scale);
  NNL_CHECK_LAUNCH();
  hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(kLossBlock), 0, s, (const float*)workspace, (int)blocks, out, scale);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}
