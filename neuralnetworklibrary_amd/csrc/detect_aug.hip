// K10 — the detection data path of the vision head (TransformBBox.__call__ and AspectRatioCollater, Applications/Vision.py:559-603,
// 758-812) on the device-resident uint8 dataset of K9: lighting, normalisation, fliplr, cv2.resize(INTER_LINEAR) to the sample's own
// size, the jitter offset and the zero padding to the minibatch's [Hp, Wp], fp32 NHWC out; and the boxes of every sample flipped,
// scaled and shifted in float64, padded with -1 to [N, 4].  The chain runs BACKWARDS per output pixel (detect_aug_index.h): nothing
// but the padded minibatch is ever written.  The lighting mean is that of the SOURCE image (:576), a per-image constant uploaded with
// the dataset, so the training transform is one pass like the eval transform: no workspace, no second launch, bitwise repeatable.
// What a source byte becomes (float(v) / 255, lit, normalised) depends on the sample and the channel alone, so a workgroup first
// fills the sample's 768-entry tap table in LDS and a pixel's twelve taps are lookups: without it the kernel is bound by its
// 48 division sequences per thread, not by its output write.
//
// Schedule: ONE launch, grid = (pixel blocks + box blocks) x samples.  A pixel workgroup covers 256 x PIX consecutive pixels of one
// sample, PIX consecutive pixels of one row per thread: most of a minibatch is padding or a plain streaming write, and with Wp a
// multiple of 4 (the collater pads to 32) a thread's 48 bytes go out as three 16-byte stores.  Any other Wp, or an unaligned out, takes
// the one-pixel instantiation.  A box workgroup (blockIdx.x past the pixel blocks) does 256 box slots of the sample, one per thread.
#include "nnl_common.h"
#include "detect_aug_index.h"

// 1: four pixels per thread where the shape allows it; 0: always one pixel per thread (DESIGN.md section 3 K10 has both timings)
#ifndef NNL_DETECT_AUG_WIDE
#define NNL_DETECT_AUG_WIDE 1
#endif
static_assert(NNL_DETECT_AUG_WIDE == 0 || NNL_DETECT_AUG_WIDE == 1, "NNL_DETECT_AUG_WIDE is a 0 / 1 switch");

namespace {

constexpr int kBlock = 256;

struct DetArgs {
  const uint8_t* arena; int64_t arena_bytes;
  const nnl_image_desc_t* desc; int64_t n_images;
  const float* image_mean;
  const double* box_arena; const int64_t* cat_arena; int64_t n_boxes;
  const nnl_detect_aug_param_t* params;
  float* out; float* boxes; int64_t* cats;
  int Hp, Wp, N, nblk_pix;
  int64_t row_jit, col_jit;
  double rand_scale;
  float mean[3], std[3];
  int has_stats;
};

template <int PIX>
__global__ __launch_bounds__(kBlock) void detect_aug_kernel(DetArgs a) {
  const int k = blockIdx.y;
  const nnl_detect_aug_param_t p = a.params[k];
  if ((int)blockIdx.x >= a.nblk_pix) {                                     // box workgroups (uniform over the workgroup)
    const int j = ((int)blockIdx.x - a.nblk_pix) * kBlock + (int)threadIdx.x;
    if (j >= a.N) return;
    int64_t first;
    const int64_t count = daug_box_range(p, a.n_boxes, &first);
    float b[4] = {-1.f, -1.f, -1.f, -1.f};
    int64_t cat = -1;
    if (j < count) {
      const nnl_image_desc_t d = a.desc[iaug_clampl(p.image, 0, a.n_images - 1)];
      daug_box(a.box_arena + (first + j) * 4, (int)iaug_clampl(d.W, 1, 1 << 24), (p.flags & NNL_IMAGE_AUG_FLIP) != 0, p.scale,
               a.rand_scale, a.row_jit, a.col_jit, b);
      cat = a.cat_arena[first + j];
    }
    const int64_t slot = (int64_t)k * a.N + j;
    for (int c = 0; c < 4; ++c) a.boxes[slot * 4 + c] = b[c];
    a.cats[slot] = cat;
    return;
  }
  // the sample's tap table (detect_aug_index.h): what a source byte of channel c becomes, lit and normalised
  __shared__ float s_lut[kDaugLut];
  const DaugSample s = daug_sample(a.desc, a.n_images, a.image_mean, p);
  daug_fill_lut(s_lut, (int)threadIdx.x, kBlock, s, a.mean, a.std, a.has_stats);              // one byte value per thread
  __syncthreads();
  const int per_row = a.Wp / PIX;                                          // PIX divides Wp (the launcher's choice)
  const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (g >= (int64_t)a.Hp * per_row) return;
  const int oy = (int)(g / per_row), ox0 = (int)(g - (int64_t)oy * per_row) * PIX;
  float v[PIX * 3];
  for (int i = 0; i < PIX * 3; ++i) v[i] = 0.f;
  int y, x;
  if (daug_inside(oy, a.row_jit, s.rh, &y))
    for (int i = 0; i < PIX; ++i)
      if (daug_inside(ox0 + i, a.col_jit, s.rw, &x)) daug_pixel(a.arena, a.arena_bytes, s, s_lut, y, x, v + 3 * i);
  float* o = a.out + (((int64_t)k * a.Hp + oy) * a.Wp + ox0) * 3;
  if constexpr (PIX == 4) {
    float4* o4 = reinterpret_cast<float4*>(o);                              // 48 (k Hp Wp + oy Wp + ox0) bytes past an aligned base
    for (int i = 0; i < 3; ++i) o4[i] = make_float4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
  } else {
    for (int i = 0; i < PIX * 3; ++i) o[i] = v[i];
  }
}

}  // namespace

extern "C" int nnl_detect_aug(const uint8_t* arena, int64_t arena_bytes, const nnl_image_desc_t* desc, int64_t n_images,
                              const float* image_mean, const double* box_arena, const int64_t* cat_arena, int64_t n_boxes,
                              const nnl_detect_aug_param_t* params, int64_t bs, int64_t Hp, int64_t Wp, int64_t N, int64_t row_jit,
                              int64_t col_jit, double rand_scale, const float* mean_std, float* out, float* boxes, int64_t* cats,
                              void* stream) {
  NNL_CHECK_ARG(arena && desc && image_mean && box_arena && cat_arena && params && out && boxes && cats, "detect_aug: null pointer");
  NNL_CHECK_ARG(arena_bytes >= 3 && n_images >= 1 && n_boxes >= 1, "detect_aug: empty arena (%lld bytes, %lld images, %lld boxes)",
                (long long)arena_bytes, (long long)n_images, (long long)n_boxes);
  NNL_CHECK_ARG(bs >= 1 && bs <= 65535, "detect_aug: bs must be in [1, 65535] (got %lld)", (long long)bs);
  NNL_CHECK_ARG(Hp >= 1 && Wp >= 1 && Hp <= (1 << 14) && Wp <= (1 << 14), "detect_aug: Hp and Wp must be in [1, 16384] (got %lld x %lld)",
                (long long)Hp, (long long)Wp);
  NNL_CHECK_ARG(N >= 1 && N <= (1 << 20), "detect_aug: N must be in [1, 2^20] (got %lld)", (long long)N);
  NNL_CHECK_ARG(row_jit >= 0 && col_jit >= 0 && row_jit <= (1 << 14) && col_jit <= (1 << 14),
                "detect_aug: row_jit and col_jit must be in [0, 16384] (got %lld, %lld)", (long long)row_jit, (long long)col_jit);
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_ELEMENTWISE, s, 12.0 * bs * Hp * Wp);
  const bool wide = NNL_DETECT_AUG_WIDE && Wp % 4 == 0 && ((uintptr_t)out & 15) == 0;
  DetArgs a{arena, arena_bytes, desc, n_images, image_mean, box_arena, cat_arena, n_boxes, params, out, boxes, cats,
            (int)Hp, (int)Wp, (int)N, (int)nnl_cdiv(Hp * (Wp / (wide ? 4 : 1)), kBlock), row_jit, col_jit, rand_scale,
            {0.f, 0.f, 0.f}, {1.f, 1.f, 1.f}, mean_std != nullptr};
  if (mean_std)
    for (int c = 0; c < 3; ++c) { a.mean[c] = mean_std[c]; a.std[c] = mean_std[3 + c]; }
  const dim3 grid((unsigned)(a.nblk_pix + nnl_cdiv(N, kBlock)), (unsigned)bs);
#if NNL_DETECT_AUG_WIDE
  if (wide) hipLaunchKernelGGL(detect_aug_kernel<4>, grid, dim3(kBlock), 0, s, a);
  else
#endif
    hipLaunchKernelGGL(detect_aug_kernel<1>, grid, dim3(kBlock), 0, s, a);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}
