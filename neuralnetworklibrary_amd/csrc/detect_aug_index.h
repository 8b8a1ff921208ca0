// Index, pixel and box arithmetic of the detection collater (csrc/detect_aug.hip; TransformBBox.__call__ and AspectRatioCollater,
// Applications/Vision.py:559-603, 758-812, run backwards one output pixel or one box slot at a time), on top of image_aug_index.h.
// Host and device compile the same inline functions: tools/detect_aug_index_check.cpp walks them on the CPU under the address and
// undefined-behaviour sanitizers.  Every function is total: any row, jitter or box range gives in-range reads, so no parameter
// table can make a caller read outside the image arena, the mean table or the box arenas.
#pragma once
#include "image_aug_index.h"

// one sample with every field made sane
struct DaugSample {
  IaugWindow w;          // the whole image as the window
  int rh, rw;            // resized size, >= 1
  float sy, sx;          // cv2.resize's source steps H / rh, W / rw
  int flip, lit;
  float bal, cont;
  float mu[3];           // channel means of the source image
};

IAUG_HD DaugSample daug_sample(const nnl_image_desc_t* desc, int64_t n_images, const float* image_mean, const nnl_detect_aug_param_t& p) {
  nnl_image_aug_param_t q = {};
  q.image = p.image;
  q.crop_h = q.crop_w = 1 << 24;                       // clamped to H x W: the window is the image
  DaugSample s;
  s.w = iaug_window(desc, n_images, q);
  s.rh = iaug_clampi(p.rh, 1, 1 << 24);
  s.rw = iaug_clampi(p.rw, 1, 1 << 24);
  s.sy = iaug_resize_scale(s.w.H, s.rh);
  s.sx = iaug_resize_scale(s.w.W, s.rw);
  s.flip = (p.flags & NNL_IMAGE_AUG_FLIP) != 0;
  s.lit = !(p.flags & NNL_IMAGE_AUG_NO_LIGHTING);
  s.bal = p.bal;
  s.cont = p.cont;
  const float* mu = image_mean + iaug_clampl(p.image, 0, n_images - 1) * 3;
  for (int c = 0; c < 3; ++c) s.mu[c] = mu[c];
  return s;
}

// output index o under a jitter: *r = o - jit, true iff it lies in [0, n) (any int jitter: the difference is taken in 64 bits)
IAUG_HD bool daug_inside(int o, int64_t jit, int n, int* r) {
  const int64_t v = (int64_t)o - iaug_clampl(jit, -(1LL << 32), 1LL << 32);
  *r = (int)iaug_clampl(v, -1, 1 << 24);
  return v >= 0 && v < n;
}

// one tap: float(v) / 255.0f, lit (:577), normalised (:580), each step rounded to fp32 as numpy rounds it
IAUG_HD float daug_tap(uint8_t v, float mu, const DaugSample& s, float mean, float std, int has_stats) {
  float u = iaug_unit(v);
  if (s.lit) u = fminf(fmaxf(((u - mu) * s.cont + s.bal) + mu, 0.f), 1.f);
  if (has_stats) u = (u - mean) / std;
  return u;
}

// A tap depends on the sample, the channel and the source byte alone: entry c * 256 + v of the sample's 768-entry tap table.
// The kernel fills it once per workgroup and every tap of a pixel is a lookup: 768 tap evaluations per workgroup instead of 12 per
// output pixel, bit for bit the same values.
constexpr int kDaugLut = 3 * 256;
IAUG_HD void daug_fill_lut(float* lut, int v_first, int v_step, const DaugSample& s, const float* mean, const float* std, int has_stats) {
  for (int c = 0; c < 3; ++c)
    for (int v = v_first; v < 256; v += v_step) lut[c * 256 + v] = daug_tap((uint8_t)v, s.mu[c], s, mean[c], std[c], has_stats);
}

// pixel (y, x) of the resized image, y in [0, rh), x in [0, rw): bilinear of four lit, normalised taps of the (flipped) source,
// the taps read from the sample's table `lut` (daug_fill_lut)
IAUG_HD void daug_pixel(const uint8_t* arena, int64_t arena_bytes, const DaugSample& s, const float* lut, int y, int x, float* out) {
  int ya, yb, xa, xb;
  float wy, wx;
  iaug_resize_taps(y, s.sy, s.w.H, &ya, &yb, &wy);
  iaug_resize_taps(x, s.sx, s.w.W, &xa, &xb, &wx);
  if (s.flip) { xa = s.w.W - 1 - xa; xb = s.w.W - 1 - xb; }
  const uint8_t* paa = arena + iaug_src_offset(s.w, arena_bytes, ya, xa);
  const uint8_t* pab = arena + iaug_src_offset(s.w, arena_bytes, ya, xb);
  const uint8_t* pba = arena + iaug_src_offset(s.w, arena_bytes, yb, xa);
  const uint8_t* pbb = arena + iaug_src_offset(s.w, arena_bytes, yb, xb);
  for (int c = 0; c < 3; ++c) {
    const float* t = lut + c * 256;
    const float top = iaug_lerp(t[paa[c]], t[pab[c]], wx);
    const float bot = iaug_lerp(t[pba[c]], t[pbb[c]], wx);
    out[c] = iaug_lerp(top, bot, wy);
  }
}

// the box range of a row clamped into the arenas (n_boxes >= 1): *first in [0, n_boxes), the count in [0, n_boxes - *first]
IAUG_HD int64_t daug_box_range(const nnl_detect_aug_param_t& p, int64_t n_boxes, int64_t* first) {
  *first = iaug_clampl(p.box_first, 0, n_boxes - 1);
  return iaug_clampl(p.box_count, 0, n_boxes - *first);
}

// box `b` (xmin, ymin, xmax, ymax; float64) of an image W wide -> the collated box in float64, every product and sum rounded on its
// own (numpy evaluates :600, :776 and :783-784 one array operation at a time).  A fused multiply-add here would change the last bit
// of the double, which the one rounding to fp32 that follows hides in all but one case in 2^28 or so: no comparison of fp32 boxes
// can see a contraction.  What keeps it out: the pragma below (clang: device and host), -ffp-contract=off on every build line of the
// library, and tools/detect_aug_index_check.cpp, which compares THESE doubles bit for bit with arithmetic forced through volatiles
// (build that tool with -ffp-contract=off: g++ has no per-function switch that survives inlining, and the tool fails without it
// wherever the host has fused multiply-adds).
IAUG_HD void daug_box_f64(const double* b, int W, int flip, double scale, double rand_scale, int64_t row_jit, int64_t col_jit, double* out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double cols = (double)W, cj = (double)col_jit, rj = (double)row_jit;
  const double x0 = flip ? cols - b[2] : b[0];
  const double x1 = flip ? cols - b[0] : b[2];
  const double sx0 = (x0 * scale) * rand_scale, sy0 = (b[1] * scale) * rand_scale;
  const double sx1 = (x1 * scale) * rand_scale, sy1 = (b[3] * scale) * rand_scale;
  out[0] = sx0 + cj;
  out[1] = sy0 + rj;
  out[2] = sx1 + cj;
  out[3] = sy1 + rj;
}

// ... and its one rounding to fp32 (:805)
IAUG_HD void daug_box(const double* b, int W, int flip, double scale, double rand_scale, int64_t row_jit, int64_t col_jit, float* out) {
  double d[4];
  daug_box_f64(b, W, flip, scale, rand_scale, row_jit, col_jit, d);
  for (int c = 0; c < 4; ++c) out[c] = (float)d[c];
}
