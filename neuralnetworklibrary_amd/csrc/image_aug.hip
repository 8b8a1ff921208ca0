// K9 — the classification Transform of the vision head (Transform.__call__, Applications/Vision.py:449-507) on a device-resident
// uint8 dataset: crop, cv2.resize(INTER_LINEAR), cv2.warpAffine(BORDER_REFLECT), fliplr, rot90, lighting and normalisation of one
// minibatch, fp32 NHWC out.  The chain runs BACKWARDS per output pixel (image_aug_index.h): the resized and the warped image are
// never written; a pixel reads up to 16 source pixels of one small neighbourhood (cache hits) and writes 12 bytes.
//
// Schedule: one thread per output pixel, one workgroup per 256 consecutive pixels of one sample (grid = pixel blocks x samples).
// Lighting needs the per-channel mean of the sample's transformed image, so the training transform is two launches: the geometric
// pass also writes each workgroup's channel sums to the workspace; the second pass adds a sample's partials in a fixed order (every
// workgroup of the sample adds the same values in the same order), then lights, clips and normalises in place.  No float atomics:
// results are bitwise repeatable.  Without lighting (the eval transform) the geometric pass normalises and is the only launch.
#include "nnl_common.h"
#include "image_aug_index.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / NNL_WAVE;

struct AugArgs {
  const uint8_t* arena; int64_t arena_bytes;
  const nnl_image_desc_t* desc; int64_t n_images;
  const nnl_image_aug_param_t* params;
  float* out; float* partial;          // partial [bs, nblk, 3]
  int sz_h, sz_w, npix, nblk;
  float mean[3], std[3];
  int has_stats;
};

template <bool LIGHT>
__global__ __launch_bounds__(kBlock) void image_aug_geometric_kernel(AugArgs a) {
  __shared__ float s_red[kWaves];
  const int b = blockIdx.y, pix = blockIdx.x * kBlock + threadIdx.x;
  const nnl_image_aug_param_t p = a.params[b];
  float v[3] = {0.f, 0.f, 0.f};
  if (pix < a.npix) {
    const int oy = pix / a.sz_w, ox = pix - oy * a.sz_w;
    iaug_geometric_pixel(a.arena, a.arena_bytes, a.desc, a.n_images, p, oy, ox, a.sz_h, a.sz_w, v);
    float* o = a.out + ((int64_t)b * a.npix + pix) * 3;
    for (int c = 0; c < 3; ++c) o[c] = (!LIGHT && a.has_stats) ? (v[c] - a.mean[c]) / a.std[c] : v[c];
  }
  if (LIGHT) {
    float* part = a.partial + ((int64_t)b * a.nblk + blockIdx.x) * 3;
    for (int c = 0; c < 3; ++c) {
      const float s = nnl_block_reduce<kWaves>(v[c], NnlSum(), s_red);
      if (threadIdx.x == 0) part[c] = s;
    }
  }
}

__global__ __launch_bounds__(kBlock) void image_aug_lighting_kernel(AugArgs a) {
  __shared__ float s_red[kWaves];
  const int b = blockIdx.y, pix = blockIdx.x * kBlock + threadIdx.x;
  const nnl_image_aug_param_t p = a.params[b];
  const bool light = !(p.flags & NNL_IMAGE_AUG_NO_LIGHTING);
  if (!light && !a.has_stats) return;                      // (uniform over the workgroup)
  float mu[3] = {0.f, 0.f, 0.f};
  if (light) {
    const float* part = a.partial + (int64_t)b * a.nblk * 3;
    for (int c = 0; c < 3; ++c) {
      float acc = 0.f;
      for (int k = threadIdx.x; k < a.nblk; k += kBlock) acc += part[k * 3 + c];
      mu[c] = nnl_block_reduce<kWaves>(acc, NnlSum(), s_red) / (float)a.npix;
    }
  }
  if (pix >= a.npix) return;
  float* o = a.out + ((int64_t)b * a.npix + pix) * 3;
  for (int c = 0; c < 3; ++c) {
    float x = o[c];
    if (light) x = fminf(fmaxf(((x - mu[c]) * p.cont + p.bal) + mu[c], 0.f), 1.f);
    if (a.has_stats) x = (x - a.mean[c]) / a.std[c];
    o[c] = x;
  }
}

bool sizes_ok(int64_t bs, int64_t sz_h, int64_t sz_w) {
  return bs >= 1 && bs <= 65535 && sz_h >= 1 && sz_w >= 1 && sz_h <= (1 << 14) && sz_w <= (1 << 14);
}

}  // namespace

extern "C" size_t nnl_image_aug_workspace_bytes(int64_t bs, int64_t sz_h, int64_t sz_w) {
  if (!sizes_ok(bs, sz_h, sz_w)) return 0;
  return (size_t)(bs * nnl_cdiv(sz_h * sz_w, kBlock) * 3) * sizeof(float);
}

extern "C" int nnl_image_aug(const uint8_t* arena, int64_t arena_bytes, const nnl_image_desc_t* desc, int64_t n_images,
                             const nnl_image_aug_param_t* params, int64_t bs, int64_t sz_h, int64_t sz_w, const float* mean_std,
                             int lighting, float* out, void* workspace, size_t workspace_bytes, void* stream) {
  NNL_CHECK_ARG(arena && desc && params && out, "image_aug: null pointer");
  NNL_CHECK_ARG(arena_bytes >= 3 && n_images >= 1, "image_aug: empty arena (%lld bytes, %lld images)", (long long)arena_bytes,
                (long long)n_images);
  NNL_CHECK_ARG(sizes_ok(bs, sz_h, sz_w), "image_aug: bs must be in [1, 65535] and sz in [1, 16384] (got %lld, %lld x %lld)",
                (long long)bs, (long long)sz_h, (long long)sz_w);
  if (lighting) {
    const size_t need = nnl_image_aug_workspace_bytes(bs, sz_h, sz_w);
    if (workspace == nullptr || workspace_bytes < need)
      return nnl_set_error(NNL_ERR_WORKSPACE, "image_aug: workspace too small (%zu < %zu bytes)", workspace_bytes, need);
  }
  hipStream_t s = (hipStream_t)stream;
  const int64_t npix = sz_h * sz_w;
  NnlProfScope prof(NNL_PROF_ELEMENTWISE, s, (lighting ? 36.0 : 12.0) * bs * npix);
  AugArgs a{arena, arena_bytes, desc, n_images, params, out, (float*)workspace, (int)sz_h, (int)sz_w, (int)npix,
            (int)nnl_cdiv(npix, kBlock), {0.f, 0.f, 0.f}, {1.f, 1.f, 1.f}, mean_std != nullptr};
  if (mean_std)
    for (int c = 0; c < 3; ++c) { a.mean[c] = mean_std[c]; a.std[c] = mean_std[3 + c]; }
  const dim3 grid((unsigned)a.nblk, (unsigned)bs);
  if (lighting) hipLaunchKernelGGL(image_aug_geometric_kernel<true>, grid, dim3(kBlock), 0, s, a);
  else hipLaunchKernelGGL(image_aug_geometric_kernel<false>, grid, dim3(kBlock), 0, s, a);
  NNL_CHECK_LAUNCH();
  if (lighting) {
    hipLaunchKernelGGL(image_aug_lighting_kernel, grid, dim3(kBlock), 0, s, a);
    NNL_CHECK_LAUNCH();
  }
  return NNL_OK;
}
