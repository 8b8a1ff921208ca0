// Host-only walk of the detection collater's index, pixel and box arithmetic (neuralnetworklibrary_amd/csrc/detect_aug_index.h),
// meant to be built with the host compiler and -fsanitize=address,undefined and run on the CPU:
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/detect_aug_index_check.cpp -o detect_aug_index_check
//   ./detect_aug_index_check
//
// It builds the arenas of tests/test_detection_pipeline.py (noise images 13x17, 17x13, 16x16, 9x31, 40x23, 5x7 back to back, the
// odd one last; 0, 1, 3, 0, 2, 5 boxes) in exactly sized heap blocks and walks every output pixel and every box slot of the tested
// minibatches (scale 0.6, 1.0, 1.7; rand_scale 0.8, 1.2; jitter (0, 0) and (3, 5); flip; lighting on and off) exactly as the
// kernel's threads do, plus hostile rows: huge and negative rh / rw, negative and huge jitter, box ranges before and past the arena,
// image numbers out of range, NaN lighting, a descriptor table that lies.  Any read outside a block, signed overflow or undefined
// conversion stops the run.  It also checks the box arithmetic for contraction: the FLOAT64 results of daug_box_f64 are compared
// bit for bit with unfused arithmetic (every product and sum forced through a volatile), and the run fails unless some of the
// compared coordinates come out differently under std::fma.  The fp32 boxes cannot show this (the last bit of a double almost
// never survives the rounding to fp32), so they are only checked to be the cast of those doubles.  -ffp-contract=off is part of
// the build line: without it g++ contracts the inlined header function wherever the host has fused multiply-adds (-march=native),
// and this check then fails, as it should.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../neuralnetworklibrary_amd/csrc/detect_aug_index.h"

namespace {

struct Arenas {
  uint8_t* arena; int64_t bytes;
  std::vector<nnl_image_desc_t> desc;
  float* image_mean;                                                       // exactly [n_images, 3]
  double* boxes; int64_t* cats; int64_t n_boxes;                           // exactly [n_boxes, 4], [n_boxes]
};

// one minibatch the way detect_aug_kernel walks it: every pixel of [Hp, Wp] and N box slots per row
double walk(const Arenas& A, const std::vector<nnl_image_desc_t>& desc, const nnl_detect_aug_param_t& p, int Hp, int Wp, int N,
            int64_t row_jit, int64_t col_jit, double rand_scale, bool has_stats) {
  const float mean[3] = {0.485f, 0.456f, 0.406f}, std[3] = {0.229f, 0.224f, 0.225f};
  const int64_t n_images = (int64_t)desc.size();
  double sum = 0;
  const DaugSample s = daug_sample(desc.data(), n_images, A.image_mean, p);
  float lut[kDaugLut];
  daug_fill_lut(lut, 0, 1, s, mean, std, has_stats);
  for (int oy = 0; oy < Hp; ++oy) {
    int y, x;
    if (!daug_inside(oy, row_jit, s.rh, &y)) continue;
    for (int ox = 0; ox < Wp; ++ox)
      if (daug_inside(ox, col_jit, s.rw, &x)) {
        float v[3];
        daug_pixel(A.arena, A.bytes, s, lut, y, x, v);
        for (int c = 0; c < 3; ++c)
          if (v[c] == v[c]) sum += v[c];
      }
  }
  int64_t first;
  const int64_t count = daug_box_range(p, A.n_boxes, &first);
  for (int j = 0; j < N && j < count; ++j) {
    const nnl_image_desc_t d = desc[iaug_clampl(p.image, 0, n_images - 1)];
    float b[4];
    daug_box(A.boxes + (first + j) * 4, (int)iaug_clampl(d.W, 1, 1 << 24), (p.flags & NNL_IMAGE_AUG_FLIP) != 0, p.scale, rand_scale,
             row_jit, col_jit, b);
    sum += (double)A.cats[first + j];
    for (int c = 0; c < 4; ++c)
      if (b[c] == b[c] && std::fabs(b[c]) < 1e30f) sum += b[c];
  }
  return sum;
}

// numpy's order with every intermediate rounded to double on its own; *fused: the same with the scale product and the jitter sum
// contracted into one std::fma, the form a contracting compiler would emit
void box_unfused(const double* b, int W, int flip, double scale, double rand_scale, int64_t row_jit, int64_t col_jit, double* out,
                 double* fused) {
  const double in[4] = {flip ? (double)W - b[2] : b[0], b[1], flip ? (double)W - b[0] : b[2], b[3]};
  const double jit[4] = {(double)col_jit, (double)row_jit, (double)col_jit, (double)row_jit};
  for (int c = 0; c < 4; ++c) {
    volatile double t = in[c] * scale;
    const double scaled = t;
    t = scaled * rand_scale;
    t = t + jit[c];
    out[c] = t;
    fused[c] = std::fma(scaled, rand_scale, jit[c]);
  }
}

}  // namespace

int main() {
  const int shapes[6][2] = {{13, 17}, {17, 13}, {16, 16}, {9, 31}, {40, 23}, {5, 7}};
  const int counts[6] = {0, 1, 3, 0, 2, 5};
  Arenas A;
  A.bytes = 0;
  for (auto& s : shapes) {
    A.desc.push_back({A.bytes, s[0], s[1]});
    A.bytes += (int64_t)s[0] * s[1] * 3;
  }
  A.arena = (uint8_t*)std::malloc((size_t)A.bytes);                        // exactly sized: one byte past the end is caught
  uint32_t lcg = 12345u;
  auto next = [&lcg]() { lcg = lcg * 1664525u + 1013904223u; return lcg >> 8; };
  for (int64_t i = 0; i < A.bytes; ++i) A.arena[i] = (uint8_t)(next() >> 16);
  A.image_mean = (float*)std::malloc(sizeof(float) * 3 * A.desc.size());
  for (size_t i = 0; i < A.desc.size(); ++i) {
    int64_t sums[3] = {0, 0, 0};
    const int64_t npix = A.desc[i].H * A.desc[i].W;
    for (int64_t q = 0; q < npix; ++q)
      for (int c = 0; c < 3; ++c) sums[c] += A.arena[A.desc[i].offset + q * 3 + c];
    for (int c = 0; c < 3; ++c) A.image_mean[i * 3 + c] = (float)((double)sums[c] / (255.0 * (double)npix));
  }
  A.n_boxes = 0;
  std::vector<int64_t> first;
  for (int c : counts) { first.push_back(A.n_boxes); A.n_boxes += c; }
  A.boxes = (double*)std::malloc(sizeof(double) * 4 * (size_t)A.n_boxes);
  A.cats = (int64_t*)std::malloc(sizeof(int64_t) * (size_t)A.n_boxes);
  for (int64_t i = 0; i < A.n_boxes; ++i) {
    for (int c = 0; c < 4; ++c) A.boxes[i * 4 + c] = (double)next() / 16777216.0 * 40.0 + (c >= 2 ? 3.0 : 0.0);
    A.cats[i] = (int64_t)(next() % 3);
  }

  // ---- daug_box_f64 against unfused double arithmetic, bit for bit IN FLOAT64; among the compared coordinates there must be some
  // that a fused multiply-add changes, or the comparison proves nothing
  const double scales[4] = {0.6, 1.0, 1.7, 0.8374651}, rands[3] = {0.8, 1.2, 1.0731};
  long box_cases = 0, fma_differs = 0;
  for (int64_t i = 0; i < A.n_boxes; ++i)
    for (double sc : scales)
      for (double rs : rands)
        for (int flip = 0; flip < 2; ++flip)
          for (int jit = 0; jit < 6; jit += 5) {
            double got[4], want[4], fused[4];
            float got32[4];
            daug_box_f64(A.boxes + i * 4, 23, flip, sc, rs, jit, jit + 3, got);
            daug_box(A.boxes + i * 4, 23, flip, sc, rs, jit, jit + 3, got32);
            box_unfused(A.boxes + i * 4, 23, flip, sc, rs, jit, jit + 3, want, fused);
            for (int c = 0; c < 4; ++c) {
              if (got[c] != want[c]) {
                std::printf("daug_box_f64: box %lld coordinate %d: %.17g, unfused %.17g (fused %.17g): contracted arithmetic?\n",
                            (long long)i, c, got[c], want[c], fused[c]);
                return 1;
              }
              if (got32[c] != (float)want[c]) { std::printf("daug_box: box %lld coordinate %d is not the cast of its double\n", (long long)i, c); return 1; }
              if (fused[c] != want[c]) ++fma_differs;
              ++box_cases;
            }
          }
  if (fma_differs == 0) { std::printf("daug_box_f64: no compared coordinate tells fused from unfused arithmetic\n"); return 1; }

  // ---- the tested minibatches
  const double img_scales[3] = {0.6, 1.0, 1.7}, rand_scales[2] = {0.8, 1.2};
  const int jitters[2][2] = {{0, 0}, {3, 5}};
  long walked = 0;
  double sum = 0;
  for (double sc : img_scales)
    for (double rs : rand_scales)
      for (auto& jit : jitters)
        for (int flip = 0; flip < 2; ++flip)
          for (int lit = 0; lit < 2; ++lit)
            for (size_t i = 0; i < A.desc.size(); ++i) {
              nnl_detect_aug_param_t p{};
              p.image = (int64_t)i; p.box_first = first[i]; p.box_count = counts[i];
              p.rh = (int)((double)shapes[i][0] * sc * rs); p.rw = (int)((double)shapes[i][1] * sc * rs);
              p.flags = (flip ? NNL_IMAGE_AUG_FLIP : 0) | (lit ? 0 : NNL_IMAGE_AUG_NO_LIGHTING);
              p.bal = lit ? 0.3f : 0.f; p.cont = 1.5f; p.scale = sc;
              const int Hp = 32 * ((p.rh + jit[0] + 31) / 32), Wp = 32 * ((p.rw + jit[1] + 31) / 32);
              sum += walk(A, A.desc, p, Hp, Wp, 5, jit[0], jit[1], rs, lit != 0);
              ++walked;
            }

  // ---- hostile rows: nothing below is a valid minibatch; every read must still land inside its block
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float wild[6] = {0.f, 1e30f, -inf, nan, 3.4e38f, -7.25f};
  const double wild_d[6] = {0.0, 1e300, -1e300, (double)nan, (double)inf, -3.5};
  const int32_t ints[7] = {0, -1, 1, 1 << 30, -(1 << 30), 2147483647, (-2147483647 - 1)};
  const int64_t longs[7] = {-1, 6, 1LL << 40, -(1LL << 62), 5, 11, 9223372036854775807LL};
  const int64_t jits[6] = {0, -1, -(1LL << 40), 1LL << 40, 7, (-9223372036854775807LL - 1)};
  for (int k = 0; k < 7 * 7 * 6; ++k) {
    nnl_detect_aug_param_t p{};
    p.image = longs[k % 7];
    p.box_first = longs[(k / 2) % 7]; p.box_count = ints[(k / 3) % 7];
    p.rh = ints[k % 7]; p.rw = ints[(k / 7) % 7];
    p.flags = ints[(k / 5) % 7];
    p.bal = wild[k % 6]; p.cont = wild[(k / 6) % 6]; p.scale = wild_d[(k / 4) % 6];
    (void)walk(A, A.desc, p, 32, 64, 9, jits[k % 6], jits[(k / 6) % 6], wild_d[k % 6], (k & 1) != 0);
    ++walked;
  }
  // a descriptor table that lies about its images
  std::vector<nnl_image_desc_t> bad = {{A.bytes - 1, 1 << 20, 1 << 20}, {-5, 40, 23}, {1LL << 50, -3, 0}};
  Arenas B = A;
  B.image_mean = (float*)std::malloc(sizeof(float) * 3 * bad.size());
  for (size_t i = 0; i < 3 * bad.size(); ++i) B.image_mean[i] = 0.5f;
  for (size_t i = 0; i < bad.size(); ++i) {
    nnl_detect_aug_param_t p{};
    p.image = (int64_t)i; p.rh = 1 << 20; p.rw = 1 << 20; p.box_count = 3; p.scale = 1.0;
    (void)walk(B, bad, p, 32, 32, 4, 3, 5, 1.0, true);
    ++walked;
  }
  std::free(B.image_mean);
  std::free(A.arena); std::free(A.image_mean); std::free(A.boxes); std::free(A.cats);
  std::printf("detect_aug_index_check: %ld box coordinates equal unfused arithmetic in float64 (%ld of them differ in float64 under a fused multiply-add), "
              "%ld parameter rows walked, checksum %.6f, clean\n", box_cases, fma_differs, walked, sum);
  return 0;
}
