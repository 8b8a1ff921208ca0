// Host-only walk of the image augmenter's index arithmetic (neuralnetworklibrary_amd/csrc/image_aug_index.h), meant to be built
// with the host compiler and -fsanitize=address,undefined and run on the CPU:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/image_aug_index_check.cpp -o image_aug_index_check
//   ./image_aug_index_check
//
// It builds the arena of tests/test_image_pipeline.py (noise images 13x17, 17x13, 16x16, 9x31, 40x23, 5x7 back to back, the odd
// one last, in an exactly sized heap block), walks every output pixel of the tested shapes (sz 8, 12, 16 and 8 x 12; every flip
// and rot; rotation by -10, 10, 37 and 170 degrees; zoom 1.0, 1.05 and 1.3; centre, float and whole-image crops) plus hostile
// parameter rows (wild coefficients, NaN, negative and oversized crops, image indices out of range), and reads the arena through
// every computed index.  Any read outside the block, signed overflow or undefined float-to-int conversion stops the run.
// It also checks that iaug_unit(v) equals float(v) / 255.0f for all 256 values.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../neuralnetworklibrary_amd/csrc/image_aug_index.h"

namespace {

void inverse_rotate_zoom(int sz_h, int sz_w, double deg, double zoom, float* m) {
  const double pi = 3.14159265358979323846;
  const double a = zoom * std::cos(deg * pi / 180.0), b = zoom * std::sin(deg * pi / 180.0);
  const double cx = sz_w / 2, cy = sz_h / 2;
  const double tx = (1 - a) * cx - b * cy, ty = b * cx + (1 - a) * cy;         // getRotationMatrix2D: [a b tx; -b a ty]
  const double det = a * a + b * b;
  const double i00 = a / det, i01 = -b / det, i10 = b / det, i11 = a / det;
  m[0] = (float)i00; m[1] = (float)i01; m[2] = (float)(-(i00 * tx + i01 * ty));
  m[3] = (float)i10; m[4] = (float)i11; m[5] = (float)(-(i10 * tx + i11 * ty));
}

double walk(const uint8_t* arena, int64_t arena_bytes, const std::vector<nnl_image_desc_t>& desc, const nnl_image_aug_param_t& p,
            int sz_h, int sz_w) {
  double sum = 0;
  for (int oy = 0; oy < sz_h; ++oy)
    for (int ox = 0; ox < sz_w; ++ox) {
      float v[3];
      iaug_geometric_pixel(arena, arena_bytes, desc.data(), (int64_t)desc.size(), p, oy, ox, sz_h, sz_w, v);
      sum += v[0] + v[1] + v[2];
    }
  return sum;
}

}  // namespace

int main() {
  for (int v = 0; v < 256; ++v) {                                          // iaug_unit IS the true division, bit for bit
    volatile float num = (float)v, den = 255.0f;
    const float want = num / den;
    if (iaug_unit((uint8_t)v) != want) { std::printf("iaug_unit(%d) = %.9g, %d / 255.0f = %.9g\n", v, iaug_unit((uint8_t)v), v, want); return 1; }
  }
  const int shapes[6][2] = {{13, 17}, {17, 13}, {16, 16}, {9, 31}, {40, 23}, {5, 7}};
  std::vector<nnl_image_desc_t> desc;
  int64_t bytes = 0;
  for (auto& s : shapes) {
    desc.push_back({bytes, s[0], s[1]});
    bytes += (int64_t)s[0] * s[1] * 3;
  }
  uint8_t* arena = (uint8_t*)std::malloc((size_t)bytes);                   // exactly sized: one byte past the end is caught
  uint32_t lcg = 12345u;
  for (int64_t i = 0; i < bytes; ++i) { lcg = lcg * 1664525u + 1013904223u; arena[i] = (uint8_t)(lcg >> 24); }

  const int sizes[4][2] = {{8, 8}, {12, 12}, {16, 16}, {8, 12}};
  const double degs[5] = {0, -10, 10, 37, 170}, zooms[3] = {1.0, 1.05, 1.3};
  const double crops[4] = {0.5, 0.25, 0.7, -1};                            // centre-like, float crop points, -1: whole image
  long walked = 0;
  double sum = 0;
  for (auto& sz : sizes)
    for (size_t i = 0; i < desc.size(); ++i)
      for (double crop : crops)
        for (double deg : degs)
          for (double zoom : zooms)
            for (int flip = 0; flip < 2; ++flip)
              for (int rot = 0; rot < 4; ++rot) {
                if (sz[0] != sz[1] && (rot & 1)) continue;
                const int H = (int)desc[i].H, W = (int)desc[i].W, L = H < W ? H : W;
                nnl_image_aug_param_t p{};
                p.image = (int64_t)i;
                if (crop < 0) { p.crop_h = H; p.crop_w = W; }
                else { p.crop_h = p.crop_w = L; p.crop_y = (int)((H - L) * crop); p.crop_x = (int)((W - L) * crop); }
                p.flags = (flip ? NNL_IMAGE_AUG_FLIP : 0) | (deg == 0 ? NNL_IMAGE_AUG_NO_WARP : 0);
                p.rot = rot;
                inverse_rotate_zoom(sz[0], sz[1], deg, zoom, p.m);
                sum += walk(arena, bytes, desc, p, sz[0], sz[1]);
                ++walked;
              }

  // hostile rows: nothing below is a valid transform; every read must still land inside the arena
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float wild[8] = {0.f, 1e30f, -1e30f, inf, -inf, nan, 3.4e38f, -7.25f};
  const int32_t ints[6] = {0, -1, 1 << 30, -(1 << 30), 2147483647, (-2147483647 - 1)};
  const int64_t images[5] = {-1, 6, 1LL << 40, -(1LL << 62), 5};
  for (int k = 0; k < 8 * 6 * 5; ++k) {
    nnl_image_aug_param_t p{};
    p.image = images[k % 5];
    p.crop_y = ints[k % 6]; p.crop_x = ints[(k / 2) % 6]; p.crop_h = ints[(k / 3) % 6]; p.crop_w = ints[(k / 5) % 6];
    for (int j = 0; j < 6; ++j) p.m[j] = wild[(k + 3 * j) % 8];
    p.flags = (k % 7 == 0) ? NNL_IMAGE_AUG_NO_WARP : (k & 2);
    p.rot = ints[(k / 7) % 6];
    for (auto& sz : sizes) { (void)walk(arena, bytes, desc, p, sz[0], sz[1]); ++walked; }
  }
  // a descriptor table that lies about its images
  std::vector<nnl_image_desc_t> bad = {{bytes - 1, 1 << 20, 1 << 20}, {-5, 40, 23}, {1LL << 50, -3, 0}};
  for (size_t i = 0; i < bad.size(); ++i) {
    nnl_image_aug_param_t p{};
    p.image = (int64_t)i; p.crop_h = 1 << 20; p.crop_w = 1 << 20; p.flags = NNL_IMAGE_AUG_NO_WARP;
    (void)walk(arena, bytes, bad, p, 16, 16);
    ++walked;
  }
  std::free(arena);
  std::printf("image_aug_index_check: %ld parameter rows walked, checksum %.6f, clean\n", walked, sum);
  return 0;
}
