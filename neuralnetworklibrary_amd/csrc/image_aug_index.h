// Index and coordinate arithmetic of the image augmenter (csrc/image_aug.hip; Applications/Vision.py:449-507 run backwards, one
// output pixel at a time): dihedral inverse, inverse affine map, reflect, resize taps, crop window, arena offset.  Host and
// device compile the same inline functions: tools/image_aug_index_check.cpp walks them on the CPU under the address and
// undefined-behaviour sanitizers.  Every function is total: any int / float input gives an in-range result, so no
// parameter table can make a caller read outside [arena, arena + arena_bytes).
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/nnl.h"

#if defined(__HIPCC__)
#define IAUG_HD __host__ __device__ __forceinline__
#else
#define IAUG_HD inline
#endif

IAUG_HD int iaug_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }          // hi >= lo
IAUG_HD int64_t iaug_clampl(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// cv2 BORDER_REFLECT, fedcba|abcdefgh|hgfedcb: index i of a length-n axis, valid at any distance (n >= 1)
IAUG_HD int iaug_reflect(int i, int n) {
  const int p = 2 * n;
  int m = i % p;
  if (m < 0) m += p;
  if (m >= n) m = p - 1 - m;
  return iaug_clampi(m, 0, n - 1);
}

// floor of a source coordinate and its fraction; coordinates beyond +-2^24 pixels (and NaN) are pinned first, so the
// conversion to int is always defined
IAUG_HD void iaug_floor(float s, int* i0, float* frac) {
  if (!(s >= -16777216.f)) s = -16777216.f;
  if (s > 16777216.f) s = 16777216.f;
  const float f = floorf(s);
  *i0 = (int)f;
  *frac = s - f;
}

// output pixel (oy, ox) of np.rot90(np.fliplr(img) if flip else img, rot) -> pixel (wy, wx) of img (rot 1 and 3: square images)
IAUG_HD void iaug_undo_dihedral(int oy, int ox, int sz_h, int sz_w, int flip, int rot, int* wy, int* wx) {
  int fy, fx;
  switch (rot & 3) {
    case 1: fy = ox; fx = sz_h - 1 - oy; break;
    case 2: fy = sz_h - 1 - oy; fx = sz_w - 1 - ox; break;
    case 3: fy = sz_w - 1 - ox; fx = oy; break;
    default: fy = oy; fx = ox; break;
  }
  *wy = fy;
  *wx = flip ? sz_w - 1 - fx : fx;
}

// inverse rotate-zoom map: destination pixel (x, y) -> source coordinate (sx, sy)
IAUG_HD void iaug_affine(const float* m, int x, int y, float* sx, float* sy) {
  const float fx = (float)x, fy = (float)y;
  *sx = (m[0] * fx + m[1] * fy) + m[2];
  *sy = (m[3] * fx + m[4] * fy) + m[5];
}

// (float)(L_src / sz) of cv2.resize's half-pixel rule, the quotient taken in double
IAUG_HD float iaug_resize_scale(int l_src, int sz) { return (float)((double)l_src / (double)sz); }

// cv2.resize(INTER_LINEAR) at output index o: source coordinate (o + 0.5) scale - 0.5, taps a, b clamped to [0, l_src), weight of b
IAUG_HD void iaug_resize_taps(int o, float scale, int l_src, int* a, int* b, float* w) {
  const float f = ((float)o + 0.5f) * scale - 0.5f;
  int i0;
  iaug_floor(f, &i0, w);
  *a = iaug_clampi(i0, 0, l_src - 1);
  *b = iaug_clampi(i0 + 1, 0, l_src - 1);
}

// one sample's source window with every field made sane: image >= 1 x 1 inside the arena, crop >= 1 x 1
struct IaugWindow {
  int64_t base;      // byte offset of the image
  int H, W;          // image size
  int cy, cx, ch, cw;
};

IAUG_HD IaugWindow iaug_window(const nnl_image_desc_t* desc, int64_t n_images, const nnl_image_aug_param_t& p) {
  const nnl_image_desc_t d = desc[iaug_clampl(p.image, 0, n_images - 1)];
  IaugWindow w;
  w.base = d.offset;
  w.H = (int)iaug_clampl(d.H, 1, 1 << 24);
  w.W = (int)iaug_clampl(d.W, 1, 1 << 24);
  w.ch = iaug_clampi(p.crop_h, 1, w.H);
  w.cw = iaug_clampi(p.crop_w, 1, w.W);
  w.cy = iaug_clampi(p.crop_y, 0, w.H - w.ch);
  w.cx = iaug_clampi(p.crop_x, 0, w.W - w.cw);
  return w;
}

// byte offset of channel 0 of crop pixel (y, x): clamped into the crop, the image, and (three bytes) the arena
IAUG_HD int64_t iaug_src_offset(const IaugWindow& w, int64_t arena_bytes, int y, int x) {
  const int iy = iaug_clampi(w.cy + iaug_clampi(y, 0, w.ch - 1), 0, w.H - 1);
  const int ix = iaug_clampi(w.cx + iaug_clampi(x, 0, w.cw - 1), 0, w.W - 1);
  const int64_t off = w.base + ((int64_t)iy * w.W + ix) * 3;
  return iaug_clampl(off, 0, arena_bytes - 3);
}

IAUG_HD float iaug_lerp(float a, float b, float w) { return a * (1.f - w) + b * w; }

// float(v) / 255.0f, correctly rounded, without the division sequence (48 of them per output pixel would cost more than the
// memory traffic): q = v r with r = fl(1 / 255), one residual step, one correction.  Bit-equal to the true division for every
// v in 0..255 (tools/image_aug_index_check.cpp compares all 256).
IAUG_HD float iaug_unit(uint8_t v) {
  const float r = 1.0f / 255.0f, f = (float)v;
  const float q = f * r;
  return fmaf(fmaf(-q, 255.0f, f), r, q);
}

// pixel (ry, rx) of the resized crop: out[c] = bilinear of the four source pixels, each float(v) / 255.0f (iaug_unit)
IAUG_HD void iaug_resized_pixel(const uint8_t* arena, int64_t arena_bytes, const IaugWindow& w, int ry, int rx, float scale_y,
                                float scale_x, float* out) {
  int ya, yb, xa, xb;
  float wy, wx;
  iaug_resize_taps(ry, scale_y, w.ch, &ya, &yb, &wy);
  iaug_resize_taps(rx, scale_x, w.cw, &xa, &xb, &wx);
  const uint8_t* paa = arena + iaug_src_offset(w, arena_bytes, ya, xa);
  const uint8_t* pab = arena + iaug_src_offset(w, arena_bytes, ya, xb);
  const uint8_t* pba = arena + iaug_src_offset(w, arena_bytes, yb, xa);
  const uint8_t* pbb = arena + iaug_src_offset(w, arena_bytes, yb, xb);
  for (int c = 0; c < 3; ++c) {
    const float top = iaug_lerp(iaug_unit(paa[c]), iaug_unit(pab[c]), wx);
    const float bot = iaug_lerp(iaug_unit(pba[c]), iaug_unit(pbb[c]), wx);
    out[c] = iaug_lerp(top, bot, wy);
  }
}

// output pixel (oy, ox) of the geometric chain (crop, resize, rotate-zoom, flip, rot90) of sample p: up to 16 source pixels
IAUG_HD void iaug_geometric_pixel(const uint8_t* arena, int64_t arena_bytes, const nnl_image_desc_t* desc, int64_t n_images,
                                  const nnl_image_aug_param_t& p, int oy, int ox, int sz_h, int sz_w, float* out) {
  const IaugWindow w = iaug_window(desc, n_images, p);
  const float scale_y = iaug_resize_scale(w.ch, sz_h), scale_x = iaug_resize_scale(w.cw, sz_w);
  int wy, wx;
  iaug_undo_dihedral(oy, ox, sz_h, sz_w, (p.flags & NNL_IMAGE_AUG_FLIP) != 0, p.rot, &wy, &wx);
  if (p.flags & NNL_IMAGE_AUG_NO_WARP) {
    iaug_resized_pixel(arena, arena_bytes, w, wy, wx, scale_y, scale_x, out);
    return;
  }
  float sx, sy, fx, fy;
  int x0, y0;
  iaug_affine(p.m, wx, wy, &sx, &sy);
  iaug_floor(sx, &x0, &fx);
  iaug_floor(sy, &y0, &fy);
  const int xa = iaug_reflect(x0, sz_w), xb = iaug_reflect(x0 + 1, sz_w);
  const int ya = iaug_reflect(y0, sz_h), yb = iaug_reflect(y0 + 1, sz_h);
  float aa[3], ab[3], ba[3], bb[3];
  iaug_resized_pixel(arena, arena_bytes, w, ya, xa, scale_y, scale_x, aa);
  iaug_resized_pixel(arena, arena_bytes, w, ya, xb, scale_y, scale_x, ab);
  iaug_resized_pixel(arena, arena_bytes, w, yb, xa, scale_y, scale_x, ba);
  iaug_resized_pixel(arena, arena_bytes, w, yb, xb, scale_y, scale_x, bb);
  for (int c = 0; c < 3; ++c) out[c] = iaug_lerp(iaug_lerp(aa[c], ab[c], fx), iaug_lerp(ba[c], bb[c], fx), fy);
}
