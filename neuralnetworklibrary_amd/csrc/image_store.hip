// K16 — the resident image set (device_data.ImageStore): exact channel statistics of uint8 images that live back to back in one
// device arena (get_stats, Applications/Vision.py:93-118), and a uint8 -> uint8 bilinear resample between two arenas (the
// downscale-on-upload of `presize`; save_resized, :64-91).  Arena and descriptor convention of K9 (image_aug.hip).
//
// nnl_image_stats.  Integer sums only: out[i][c] = sum v, out[i][3 + c] = sum v^2 over the H W bytes of channel c, added in
// uint32 per 16-byte load, uint64 per thread, uint64 over the workgroup (block_ops.h) and with ONE 64-bit integer atomic per
// workgroup, channel and moment to global memory: exact, so the order of the atomics cannot show.  Schedule: grid = (split,
// images); an image is NNL_IMAGE_STATS_TILE_BYTES-byte tiles and workgroup x takes tiles x, x + split, ...: a large image is
// spread over `split` workgroups and the result does not depend on `split`.  A thread reads 16-byte words at 16-byte-ALIGNED
// addresses: the word that holds an image's first or last byte also holds a neighbour's bytes, which are masked by position;
// a word that is not wholly inside [arena, arena + arena_bytes) is read byte by byte, only the bytes of the image.  Pixels are 3
// bytes, so the channel of a word's first byte changes from word to word: byte i of a word goes to slot i % 3 and the three slot
// sums are rotated into channels once per word.
//
// nnl_image_resize_u8.  One thread per destination pixel, grid = (split, images) with 256-pixel tiles taken the same way.
// The definition (include/nnl.h repeats it): with sy = (float)((double)Hs / Hd), fy = ((float)oy + 0.5f) * sy - 0.5f,
// y0 = floor(fy), wy = fy - y0, ya = clamp(y0, 0, Hs - 1), yb = clamp(y0 + 1, 0, Hs - 1) and the same along x
// (iaug_resize_scale, iaug_resize_taps), per channel, every operation rounded to fp32 on its own (no contraction):
//   top = v[ya][xa] * (1 - wx) + v[ya][xb] * wx;  bot = v[yb][xa] * (1 - wx) + v[yb][xb] * wx;
//   r = top * (1 - wy) + bot * wy;   dst = (uint8)min(max(rintf(r), 0), 255)        (rintf: ties to even)
// the interpolation order of iaug_resized_pixel on float(v), without the division by 255.  Hd = Hs, Wd = Ws gives wy = wx = 0
// and the source bytes.  This is NOT cv2.resize on uint8 (11-bit fixed-point weights).
#include "nnl_common.h"
#include "image_aug_index.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / NNL_WAVE;
constexpr int kWord = 16;                                                   // bytes per load
constexpr int kTile = NNL_IMAGE_STATS_TILE_BYTES;                           // image bytes per workgroup step
constexpr int kWordsPerTile = kTile / kWord + 1;                            // + 1: a tile that starts inside a word ends inside one more
constexpr int kResizeTile = kBlock;                                         // destination pixels per workgroup step
constexpr int64_t kMaxSide = 1 << 24;
constexpr int kMaxGridY = 65535;
static_assert(kTile % kWord == 0 && kTile >= kWord, "a tile is whole words");

// image `d` is >= 1 x 1, at most 2^24 a side, and lies inside [0, bytes)
__device__ __forceinline__ bool desc_ok(const nnl_image_desc_t& d, int64_t bytes) {
  if (d.offset < 0 || d.H < 1 || d.W < 1 || d.H > kMaxSide || d.W > kMaxSide || d.offset > bytes) return false;
  return d.H * d.W * 3 <= bytes - d.offset;                                 // H W 3 <= 3 * 2^48: no overflow
}

// v[k], k in 0..2, by selects (a register array under a per-thread index would go to scratch)
__device__ __forceinline__ uint32_t pick3(const uint32_t* v, int k) { return k == 0 ? v[0] : (k == 1 ? v[1] : v[2]); }

struct StatsArgs {
  const uint8_t* arena; int64_t arena_bytes;
  const nnl_image_desc_t* desc;
  int64_t first;                                                            // desc row of blockIdx.y == 0
  unsigned long long* out;                                                  // row of blockIdx.y == 0
};

__global__ __launch_bounds__(kBlock) void image_stats_kernel(StatsArgs a) {
  __shared__ unsigned long long s_red[kWaves];
  const nnl_image_desc_t d = a.desc[a.first + blockIdx.y];
  unsigned long long* out = a.out + (int64_t)blockIdx.y * 6;
  if (!desc_ok(d, a.arena_bytes)) {                                         // (uniform over the workgroup) nothing is read
    if (blockIdx.x == 0 && threadIdx.x < 6) out[threadIdx.x] = NNL_IMAGE_STATS_INVALID;
    return;
  }
  const int64_t nbytes = d.H * d.W * 3;
  const int64_t ntiles = (nbytes + kTile - 1) / kTile;
  if ((int64_t)blockIdx.x >= ntiles) return;
  const uintptr_t img = (uintptr_t)a.arena + (uintptr_t)d.offset;           // address of the image's byte 0
  const uintptr_t lo_arena = (uintptr_t)a.arena, hi_arena = lo_arena + (uintptr_t)a.arena_bytes;   // addresses are compared as integers;
  // every load goes through a.arena + (address - lo_arena), so it stays a global (not a flat) access
  unsigned long long sum[3] = {0, 0, 0}, sq[3] = {0, 0, 0};
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uintptr_t lo = img + (uintptr_t)(t * kTile);                      // this tile's bytes: [lo, hi)
    const uintptr_t hi = img + (uintptr_t)(t * kTile + kTile < nbytes ? t * kTile + kTile : nbytes);
    const uintptr_t w0 = lo & ~(uintptr_t)(kWord - 1);
    for (int j = threadIdx.x; j < kWordsPerTile; j += kBlock) {
      const uintptr_t w = w0 + (uintptr_t)j * kWord;
      if (w >= hi) break;
      uint32_t s[3] = {0, 0, 0}, q[3] = {0, 0, 0};
      if (w >= lo && w + kWord <= hi) {                                     // interior word: inside the image, so inside the arena
        const uint4 v = *(const uint4*)(a.arena + (int64_t)(w - lo_arena));
        const uint32_t r[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < kWord; ++i) {
          const uint32_t b = (r[i >> 2] >> (8 * (i & 3))) & 0xffu;
          s[i % 3] += b;
          q[i % 3] += b * b;
        }
      } else if (w >= lo_arena && w + kWord <= hi_arena) {                  // edge word inside the arena: one load, bytes masked
        const uint4 v = *(const uint4*)(a.arena + (int64_t)(w - lo_arena));
        const uint32_t r[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < kWord; ++i) {
          const uint32_t b = (w + i >= lo && w + i < hi) ? (r[i >> 2] >> (8 * (i & 3))) & 0xffu : 0u;
          s[i % 3] += b;
          q[i % 3] += b * b;
        }
      } else {                                                              // the word crosses an end of the arena: bytes of the tile only
#pragma unroll
        for (int i = 0; i < kWord; ++i) {
          const uint32_t b = (w + i >= lo && w + i < hi) ? a.arena[(int64_t)(w + i - lo_arena)] : 0u;
          s[i % 3] += b;
          q[i % 3] += b * b;
        }
      }
      // channel of the word's byte 0: (w - img) mod 3, w may lie up to 15 bytes in front of the image
      const int p0 = (int)(((int64_t)w - (int64_t)img + 48) % 3);
      // slot k holds channel (p0 + k) % 3
      const int k0 = p0 == 0 ? 0 : 3 - p0;                                  // slot of channel 0
      const int k1 = k0 == 2 ? 0 : k0 + 1, k2 = k1 == 2 ? 0 : k1 + 1;
      sum[0] += pick3(s, k0); sum[1] += pick3(s, k1); sum[2] += pick3(s, k2);
      sq[0] += pick3(q, k0); sq[1] += pick3(q, k1); sq[2] += pick3(q, k2);
    }
  }
  for (int c = 0; c < 3; ++c) {
    const unsigned long long ts = nnl_block_reduce<kWaves>(sum[c], NnlSum(), s_red);
    const unsigned long long tq = nnl_block_reduce<kWaves>(sq[c], NnlSum(), s_red);
    if (threadIdx.x == 0) {
      atomicAdd(out + c, ts);
      atomicAdd(out + 3 + c, tq);
    }
  }
}

struct ResizeArgs {
  const uint8_t* src; int64_t src_bytes;
  const nnl_image_desc_t* src_desc;
  uint8_t* dst; int64_t dst_bytes;
  const nnl_image_desc_t* dst_desc;
  int64_t first;                                                            // desc row of blockIdx.y == 0
};

__global__ __launch_bounds__(kBlock) void image_resize_u8_kernel(ResizeArgs a) {
  const nnl_image_desc_t ds = a.src_desc[a.first + blockIdx.y], dd = a.dst_desc[a.first + blockIdx.y];
  if (!desc_ok(ds, a.src_bytes) || !desc_ok(dd, a.dst_bytes)) return;       // (uniform) nothing is read or written
  IaugWindow w;
  w.base = ds.offset; w.H = (int)ds.H; w.W = (int)ds.W;
  w.cy = 0; w.cx = 0; w.ch = w.H; w.cw = w.W;
  const int Hd = (int)dd.H, Wd = (int)dd.W;
  const int64_t npix = (int64_t)Hd * Wd;
  const float sy = iaug_resize_scale(w.H, Hd), sx = iaug_resize_scale(w.W, Wd);
  for (int64_t t = blockIdx.x; t * kResizeTile < npix; t += gridDim.x) {
    const int64_t pix = t * kResizeTile + threadIdx.x;
    if (pix >= npix) break;
    const int oy = (int)(pix / Wd), ox = (int)(pix - (int64_t)oy * Wd);
    int ya, yb, xa, xb;
    float wy, wx;
    iaug_resize_taps(oy, sy, w.H, &ya, &yb, &wy);
    iaug_resize_taps(ox, sx, w.W, &xa, &xb, &wx);
    const uint8_t* paa = a.src + iaug_src_offset(w, a.src_bytes, ya, xa);
    const uint8_t* pab = a.src + iaug_src_offset(w, a.src_bytes, ya, xb);
    const uint8_t* pba = a.src + iaug_src_offset(w, a.src_bytes, yb, xa);
    const uint8_t* pbb = a.src + iaug_src_offset(w, a.src_bytes, yb, xb);
    uint8_t* o = a.dst + dd.offset + pix * 3;
    for (int c = 0; c < 3; ++c) {
      const float top = iaug_lerp((float)paa[c], (float)pab[c], wx);
      const float bot = iaug_lerp((float)pba[c], (float)pbb[c], wx);
      const float r = rintf(iaug_lerp(top, bot, wy));
      o[c] = (uint8_t)fminf(fmaxf(r, 0.f), 255.f);
    }
  }
}

// workgroups per image: twice the tiles of the MEAN image of the arena, so that a set of equal images wastes at most half of the
// (empty, immediately returning) workgroups and a lone large image still spreads
unsigned split_for(int64_t arena_units, int64_t n_images, int64_t tile, int64_t cap) {
  int64_t s = 2 * nnl_cdiv(nnl_cdiv(arena_units, n_images), tile);
  return (unsigned)(s < 1 ? 1 : (s > cap ? cap : s));
}

}  // namespace

extern "C" int nnl_image_stats(const uint8_t* arena, int64_t arena_bytes, const nnl_image_desc_t* desc, int64_t n_images,
                               int64_t first, int64_t count, uint64_t* out, void* stream) {
  NNL_CHECK_ARG(arena && desc && out, "image_stats: null pointer");
  NNL_CHECK_ARG(arena_bytes >= 3 && n_images >= 1, "image_stats: empty arena (%lld bytes, %lld images)", (long long)arena_bytes,
                (long long)n_images);
  NNL_CHECK_ARG(first >= 0 && count >= 1 && count <= n_images - first, "image_stats: window [%lld, %lld + %lld) outside [0, %lld)",
                (long long)first, (long long)first, (long long)count, (long long)n_images);
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_ELEMENTWISE, s, (double)arena_bytes);
  NNL_CHECK_HIP(hipMemsetAsync(out, 0, (size_t)count * 6 * sizeof(uint64_t), s));
  const unsigned split = split_for(arena_bytes, n_images, kTile, 256);
  for (int64_t i = 0; i < count; i += kMaxGridY) {
    const int64_t m = count - i < kMaxGridY ? count - i : kMaxGridY;
    StatsArgs a{arena, arena_bytes, desc, first + i, (unsigned long long*)out + i * 6};
    hipLaunchKernelGGL(image_stats_kernel, dim3(split, (unsigned)m), dim3(kBlock), 0, s, a);
    NNL_CHECK_LAUNCH();
  }
  return NNL_OK;
}

extern "C" int nnl_image_resize_u8(const uint8_t* src_arena, int64_t src_bytes, const nnl_image_desc_t* src_desc, uint8_t* dst_arena,
                                   int64_t dst_bytes, const nnl_image_desc_t* dst_desc, int64_t n_images, void* stream) {
  NNL_CHECK_ARG(src_arena && src_desc && dst_arena && dst_desc, "image_resize_u8: null pointer");
  NNL_CHECK_ARG(src_bytes >= 3 && dst_bytes >= 3 && n_images >= 1, "image_resize_u8: empty arena (%lld -> %lld bytes, %lld images)",
                (long long)src_bytes, (long long)dst_bytes, (long long)n_images);
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_ELEMENTWISE, s, (double)dst_bytes);
  const unsigned split = split_for(dst_bytes / 3, n_images, kResizeTile, 1024);
  for (int64_t i = 0; i < n_images; i += kMaxGridY) {
    const int64_t m = n_images - i < kMaxGridY ? n_images - i : kMaxGridY;
    ResizeArgs a{src_arena, src_bytes, src_desc, dst_arena, dst_bytes, dst_desc, i};
    hipLaunchKernelGGL(image_resize_u8_kernel, dim3(split, (unsigned)m), dim3(kBlock), 0, s, a);
    NNL_CHECK_LAUNCH();
  }
  return NNL_OK;
}
