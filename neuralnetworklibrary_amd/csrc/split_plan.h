// The split schedule of the three 64x64-tile conv kernels (igemm_taps_kernel, wino_kernel, wino2_kernel), host side: the plan, its
// geometry, the cost model and search the direct and 1-D Winograd kernels share, and the binding of a plan to a launch.  The device side
// (a workgroup's tile and slice, the hand-over to the last arriver, the slab sum and the finish of the output) is split_tile.h.
//
// T = grid_m x grid_n tiles of 64 schedule rows (output pixels, pairs or quads) x 64 channels.  The first n_main_tiles ("main": whole
// multiples of 256 workgroups, whole tile rows) are cut into main_ks k slices, the leftover tail tiles into tail_slices; a slice writes
// its partial tile into a slab of the workspace, [main slabs][tail slabs], and the last arriver on the tile's counter sums the slabs in
// slice order.  A plan is a pure function of the shape (and the NNL_* switches), so the *_workspace_bytes() query and the launch agree.
#pragma once
#include "nnl_common.h"

constexpr int kCUs = 256;

static inline size_t align4(size_t floats) { return (floats + 3) & ~(size_t)3; }

struct SplitPlan {
  int on, bk, main_ks, n_main_tiles, tail_slices, tail_row0;
  size_t main_floats, tail_floats;        // workspace: [main slabs][tail slabs]
  double t_us;                            // predicted time of the chosen plan
  int pos_cs;                             // wino2_kernel only, > 0: the position-split instantiation, channel slices per position
};

// The schedule's geometry for `ks` main and `S` tail slices: T tiles in rows of gn, `rows` schedule rows of `row_floats` output floats
// each.  Fills the six geometry fields of *pl (tail_slices is 1 when there is no tail) and returns the number of tail tiles.
static inline long split_geometry(long T, long gn, long rows, long row_floats, int ks, int S, SplitPlan* pl) {
  long n_main = ((T * ks / kCUs) * kCUs / ks / gn) * gn;               // main tiles: whole multiples of 256 workgroups, whole tile rows
  if (n_main > T) n_main = T;
  const long tail = T - n_main;
  const long row0 = (n_main / gn) * 64 < rows ? (n_main / gn) * 64 : rows;
  pl->main_ks = ks; pl->n_main_tiles = (int)n_main; pl->tail_slices = tail ? S : 1; pl->tail_row0 = (int)row0;
  pl->main_floats = ks > 1 ? (size_t)ks * row0 * row_floats : 0;
  pl->tail_floats = (S > 1 && tail) ? (size_t)S * (rows - row0) * row_floats : 0;
  return tail;
}

// What the shared search knows about a kernel
struct SplitKernel {
  int bk;                 // k block of the instantiation that would run
  long iters;             // k iterations of a whole tile
  double us_per_iter;     // us per k iteration per CU-resident workgroup set (measured ~113 TF/s ceiling)
  long occ;               // resident workgroups per CU (LDS- / VGPR-limited)
  int row_factor;         // output rows per schedule row
  bool balance;           // false: the unsplit launch, timed
  double accept;          // a plan is taken below accept x the unsplit time (0.99: a >= 1 % predicted win; above 1 forces, for A/B runs)
  int force_ks, force_S;  // > 0: only that main / tail slice count (whatever it costs) where the shape allows it
};

// The plan with the shortest predicted time for a rows x Nc output
static inline SplitPlan split_search(const SplitKernel& k, long rows, int Nc) {
  SplitPlan best{};
  const long gn = nnl_cdiv(Nc, 64), T = nnl_cdiv(rows, 64) * gn, I = k.iters;
  best.bk = k.bk;
  auto wave_iters = [&](long blocks, long iters) {                     // busiest CU's iterations for `blocks` equal workgroups
    if (blocks <= 0) return 0.0;
    const long cap = k.occ * kCUs;                                     // full residency waves, then the remainder on top
    const long full = blocks / cap, rem = blocks - full * cap;         // (measured: 1568 workgroups at occupancy 6 take 7 units)
    return (double)(full * k.occ + nnl_cdiv(rem, kCUs)) * iters;
  };
  const double plain = wave_iters(T, I) * k.us_per_iter;
  best.t_us = plain;
  if (!k.balance) return best;
  double best_t = (k.force_ks > 0 || k.force_S > 0) ? 1e300 : plain * k.accept;
  const int plan_extra = 2;                                            // k iterations' worth of fix-up cost per sliced workgroup
  const double plan_bw = 16000 * 1.0e3;                                // slab traffic bandwidth, bytes per us
  for (int ks = 1; ks <= 4; ks *= 2) {
    if (k.force_ks > 0 && ks != k.force_ks) continue;
    if (I / ks < 8) break;
    const long it_main = nnl_cdiv(I, ks);
    static const int kSlices[] = {1, 2, 3, 4, 6, 8, 9, 12, 16, 18, 24, 32, 36, 48};
    for (int S : kSlices) {
      SplitPlan c{};
      const long tail = split_geometry(T, gn, rows, (long)k.row_factor * Nc, ks, S, &c);
      if (tail == 0 && S > 1) break;
      if (S > 1 && I / S < 4) break;
      if (k.force_S > 0 && tail > 0 && S != k.force_S) continue;
      const long it_tail = nnl_cdiv(I, S);
      double t = (wave_iters((T - tail) * ks, it_main) + wave_iters(tail * S, it_tail + (S > 1 ? plan_extra : 0))) * k.us_per_iter;
      const long row0 = c.tail_row0;
      const double main_b = ks > 1 ? (2.0 * ks + 1) * row0 * k.row_factor * Nc * 4 : 0;
      const double tail_b = S > 1 ? (2.0 * S + 1) * (rows - row0) * k.row_factor * Nc * 4 : 0;
      t += (main_b + tail_b) / plan_bw + (ks > 1 ? 1 : 0) + (S > 1 && tail ? 1 : 0);      // slab traffic (write + re-read) + fix-up latency
      if (t < best_t) {
        best_t = t;
        best = c;
        best.on = 1; best.bk = k.bk; best.t_us = t;
      }
    }
  }
  if (best.on && best.main_ks == 1 && best.tail_slices == 1) best.on = 0;
  return best;
}

// Do the caller's buffers hold the plan?  A kernel that finishes its split tiles in-kernel only needs a counter per tile and reads a slab
// region through one 2 GB buffer resource; the direct kernel (reduce_pass) addresses its slabs with 64-bit pointers and, without counters
// for every tile, leaves the sums to slab_reduce_kernel: *counters is cleared then.  head_floats: what precedes the slabs in the workspace.
static inline bool split_plan_fits(const SplitPlan& pl, long T, int** counters, long n_counters, size_t ws_bytes, size_t head_floats,
                                   bool reduce_pass) {
  if (T > n_counters) *counters = nullptr;
  if (!reduce_pass && (*counters == nullptr || pl.main_floats * sizeof(float) >= (1UL << 31) || pl.tail_floats * sizeof(float) >= (1UL << 31)))
    return false;
  return ws_bytes >= (head_floats + pl.main_floats + pl.tail_floats) * sizeof(float);
}

// Binds a plan to a launch of one of the three kernels (p.grid_m, p.grid_n and p.Nc set): slabs at `slabs`, `rows` schedule rows of
// row_factor output rows each.  Returns the grid size.
template <class Params>
unsigned split_bind(Params& p, const SplitPlan& pl, float* slabs, long rows, int row_factor, int* counters) {
  const long T = (long)p.grid_m * p.grid_n, row_floats = (long)row_factor * p.Nc;
  p.bal = 1; p.main_ks = pl.main_ks; p.n_main_tiles = pl.n_main_tiles; p.tail_slices = pl.tail_slices; p.tail_row0 = pl.tail_row0;
  p.main_out = slabs; p.main_slab_stride = pl.tail_row0 * row_floats;
  p.tail_out = slabs + pl.main_floats; p.tail_slab_stride = (rows - pl.tail_row0) * row_floats;
  p.tile_counters = counters;                                          // in-kernel fix-up of the split tiles
  return (unsigned)(pl.n_main_tiles * pl.main_ks + (T - pl.n_main_tiles) * pl.tail_slices);
}
