// K14 — detection evaluation: the COCO / Pascal protocol of pycocotools' COCOeval for boxes (Applications/pycocotools/cocoeval.py:171-198,
// 243-428) and the mean average precision of Applications/Vision.py:1696-1747 (mAP1), both instead of Python loops over (category,
// threshold, image).
//
// Common shape.  A GROUP is an (image, category) pair with at least one detection or one ground truth; groups are sorted by (category,
// image), so a category is a contiguous span of groups, of detections and of ground truths.  Every offset array is a device array the
// caller has checked (non-decreasing, ending at the array length).  The groups are independent and the matching is sequential only
// inside one: one wave per group.  The curves of a (category, threshold) are segmented scans over the category's detections in score
// order (one stable sort per category, made by the caller): one workgroup per curve walks 256-element tiles with a carried prefix,
// forward for the running sums and backward for the running maximum from the right.  No workgroup waits for another, nothing is added
// with floating-point atomics: the same inputs give the same bits.
//
// nnl_det_coco_match: the overlap matrix of a group is computed once, in fp64, one operation at a time, and serves all A x T
// matchers of the group; each (area range, threshold) runs the reference's greedy loop in a lane of its own.  The matrix and the
// matchers' "ground truth taken" bytes live in LDS when they fit kLdsDoubles and in the caller's scratch buffer (at scr_off[g])
// when they do not: no bound on detections or ground truths per group.  A group whose buffer does not fit where the caller said
// is skipped and reported in status[0] (the caller raises), never truncated.
// nnl_det_coco_accumulate: precision / scores / recall of cocoeval.py:323-428.
// nnl_det_map_match: fp32 jaccard of Vision.py:1696-1728 on the fly, first arg-max prediction per ground truth, one flag per threshold.
// nnl_det_map_integrate: Vision.py:1730-1747.
#include "nnl_common.h"

#include <cmath>

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / NNL_WAVE;
constexpr int kLdsDoubles = NNL_DET_EVAL_LDS_DOUBLES;

struct MatchParams {
  int T, A;
  double thr[NNL_DET_EVAL_MAX_T];
  double lo[NNL_DET_EVAL_MAX_A], hi[NNL_DET_EVAL_MAX_A];
};
struct AccumParams {
  int T, A, M, R;
  int max_dets[NNL_DET_EVAL_MAX_M];
  double rec[NNL_DET_EVAL_MAX_R];
};
struct MapParams {
  int T;
  double thr[NNL_DET_EVAL_MAX_T];
};

// ---- a. COCO matching ------------------------------------------------------------------------------------------------------

// cocoeval.py:171-198 (the overlap, maskUtils.iou for boxes) and :243-321 (evaluateImg) for one group per wave
__global__ __launch_bounds__(NNL_WAVE) void coco_match_kernel(const int32_t* __restrict__ dt_off, const int32_t* __restrict__ gt_off,
                                                              const double* __restrict__ dt_box, const double* __restrict__ gt_box,
                                                              const double* __restrict__ gt_area, const uint8_t* __restrict__ gt_flags,
                                                              const int64_t* __restrict__ scr_off, double* __restrict__ scratch,
                                                              int64_t scratch_doubles, MatchParams P, int64_t NG, int64_t Nd,
                                                              int32_t* __restrict__ dtm, uint8_t* __restrict__ dtig,
                                                              int32_t* __restrict__ npig, int32_t* __restrict__ status) {
  __shared__ double lds[kLdsDoubles];
  const int64_t g = blockIdx.x;
  const int lane = threadIdx.x;
  const int d0 = dt_off[g], D = dt_off[g + 1] - d0, q0 = gt_off[g], G = gt_off[g + 1] - q0;
  const int AT = P.A * P.T;

  // ground truths that count in each area range (gtIg == 0, :259-262, :380)
  for (int a = 0; a < P.A; ++a) {
    int cnt = 0;
    for (int j = lane; j < G; j += NNL_WAVE) {
      const double ar = gt_area[q0 + j];
      cnt += !((gt_flags[q0 + j] & 2) || ar < P.lo[a] || ar > P.hi[a]);
    }
    cnt = nnl_wave_sum(cnt);
    if (lane == 0) npig[(int64_t)a * NG + g] = cnt;
  }
  if (D == 0) return;
  if (G == 0) {                                  // nothing to match: a detection outside the range is ignored (:306-307)
    for (int64_t e = lane; e < (int64_t)AT * D; e += NNL_WAVE) {
      const int c = (int)(e / D), d = (int)(e % D), a = c / P.T;
      const double ar = dt_box[(int64_t)(d0 + d) * 4 + 2] * dt_box[(int64_t)(d0 + d) * 4 + 3];
      dtm[(int64_t)c * Nd + d0 + d] = 0;
      dtig[(int64_t)c * Nd + d0 + d] = (ar < P.lo[a] || ar > P.hi[a]) ? 1 : 0;
    }
    return;
  }

  // the group's buffer: D x G overlaps, then AT x G "taken" bytes, then A x G (ignored | crowd << 1) bytes
  const int64_t need = (int64_t)D * G + ((int64_t)(AT + P.A) * G + 7) / 8;
  const int64_t so = scr_off[g];
  double* buf;
  if (so < 0) {
    if (need > kLdsDoubles) { if (lane == 0) atomicOr(status, 1); return; }
    buf = lds;
  } else {
    if (so + need > scratch_doubles) { if (lane == 0) atomicOr(status, 1); return; }
    buf = scratch + so;
  }
  double* iou = buf;
  uint8_t* taken = reinterpret_cast<uint8_t*>(buf + (int64_t)D * G);
  uint8_t* gflag = taken + (int64_t)AT * G;

  for (int64_t e = lane; e < (int64_t)D * G; e += NNL_WAVE) {
    const int d = (int)(e / G), j = (int)(e % G);
    const double* db = dt_box + (int64_t)(d0 + d) * 4;
    const double* gb = gt_box + (int64_t)(q0 + j) * 4;
    const double w = fmin(db[0] + db[2], gb[0] + gb[2]) - fmax(db[0], gb[0]);
    const double h = fmin(db[1] + db[3], gb[1] + gb[3]) - fmax(db[1], gb[1]);
    double o = 0.0;
    if (!(w <= 0.0 || h <= 0.0)) {
      const double inter = w * h, da = db[2] * db[3];
      const double u = (gt_flags[q0 + j] & 1) ? da : da + gb[2] * gb[3] - inter;
      o = inter / u;
    }
    iou[e] = o;
  }
  for (int64_t e = lane; e < (int64_t)AT * G; e += NNL_WAVE) taken[e] = 0;
  for (int64_t e = lane; e < (int64_t)P.A * G; e += NNL_WAVE) {
    const int a = (int)(e / G), j = (int)(e % G);
    const double ar = gt_area[q0 + j];
    const uint8_t f = gt_flags[q0 + j];
    gflag[e] = (uint8_t)((((f & 2) || ar < P.lo[a] || ar > P.hi[a]) ? 1 : 0) | ((f & 1) << 1));
  }
  __syncthreads();

  for (int c = lane; c < AT; c += NNL_WAVE) {
    const int a = c / P.T, t = c % P.T;
    uint8_t* tk = taken + (int64_t)c * G;
    const uint8_t* gf = gflag + (int64_t)a * G;
    for (int d = 0; d < D; ++d) {
      double bar = fmin(P.thr[t], 1.0 - 1e-10);
      int m = -1, m_ig = 0;
      const double* row = iou + (int64_t)d * G;
      // not ignored ground truths first, then the ignored ones, each in their own order (the stable argsort of :265)
      for (int phase = 0; phase < 2; ++phase) {
        if (phase == 1 && m > -1 && m_ig == 0) break;          // matched to a regular one: stop at the first ignored (:291)
        for (int j = 0; j < G; ++j) {
          const uint8_t f = gf[j];
          if ((f & 1) != phase) continue;
          if (tk[j] && !(f & 2)) continue;                     // already matched and not a crowd (:288)
          if (row[j] < bar) continue;                          // ties go to the later ground truth (:294)
          bar = row[j];
          m = j;
          m_ig = phase;
        }
      }
      const int64_t at = (int64_t)c * Nd + d0 + d;
      if (m >= 0) {
        tk[m] = 1;
        dtm[at] = m + 1;
        dtig[at] = (uint8_t)m_ig;
      } else {
        const double ar = dt_box[(int64_t)(d0 + d) * 4 + 2] * dt_box[(int64_t)(d0 + d) * 4 + 3];
        dtm[at] = 0;
        dtig[at] = (ar < P.lo[a] || ar > P.hi[a]) ? 1 : 0;
      }
    }
  }
}

// ---- workgroup scans ---------------------------------------------------------------------------------------------------------

struct I3 { int k, t, f; };
__device__ __forceinline__ I3 i3_add(I3 a, I3 b) { return I3{a.k + b.k, a.t + b.t, a.f + b.f}; }

constexpr I3 kZero3 = {0, 0, 0};

// ---- b. COCO accumulation ------------------------------------------------------------------------------------------------------

// first index r in [0, R) with rec[r] > x (rec ascending)
__device__ __forceinline__ int upper_bound(const double* rec, int R, double x) {
  int lo = 0, hi = R;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (rec[mid] > x) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// cocoeval.py:361-418 for one (category k, area range a, maxDets entry m, threshold t)
__global__ __launch_bounds__(kThreads) void coco_accumulate_kernel(const int32_t* __restrict__ cat_grp_off, const int32_t* __restrict__ cat_dt_off,
                                                                   const int32_t* __restrict__ order, const int32_t* __restrict__ dt_rank,
                                                                   const double* __restrict__ dt_score, const int32_t* __restrict__ dtm,
                                                                   const uint8_t* __restrict__ dtig, const int32_t* __restrict__ npig,
                                                                   AccumParams P, int64_t K, int64_t NG, int64_t Nd,
                                                                   double* __restrict__ precision, double* __restrict__ scores,
                                                                   double* __restrict__ recall) {
  __shared__ double rec[NNL_DET_EVAL_MAX_R];
  __shared__ int pos[NNL_DET_EVAL_MAX_R];
  __shared__ I3 lds_i[kWaves];
  __shared__ double lds_d[kWaves];
  __shared__ double tile[kThreads];
  const int tid = threadIdx.x;
  int b = blockIdx.x;
  const int t = b % P.T; b /= P.T;
  const int m = b % P.M; b /= P.M;
  const int a = b % P.A;
  const int k = b / P.A;
  const int R = P.R;
  const int64_t rstride = K * P.A * P.M;                                     // precision[t, r, k, a, m]
  const int64_t out0 = (int64_t)t * R * rstride + ((int64_t)k * P.A + a) * P.M + m;
  const int64_t rc_at = (((int64_t)t * K + k) * P.A + a) * P.M + m;            // recall[t, k, a, m]

  for (int r = tid; r < R; r += kThreads) { rec[r] = P.rec[r]; pos[r] = -1; }
  const int g0 = cat_grp_off[k], g1 = cat_grp_off[k + 1];
  I3 np{0, 0, 0}, tot;
  for (int g = g0 + tid; g < g1; g += kThreads) np.k += npig[(int64_t)a * NG + g];
  nnl_block_scan<kWaves>(np, i3_add, kZero3, lds_i, tot);                                               // also the barrier behind rec / pos
  const int n_pig = tot.k;
  if (g0 == g1 || n_pig == 0) {                                              // no group, or no ground truth that counts: stays -1 (:368, :381)
    for (int r = tid; r < R; r += kThreads) { precision[out0 + r * rstride] = -1.0; scores[out0 + r * rstride] = -1.0; }
    if (tid == 0) recall[rc_at] = -1.0;
    return;
  }
  const int i0 = cat_dt_off[k], n = cat_dt_off[k + 1] - i0, max_det = P.max_dets[m];
  const int64_t plane = (int64_t)(a * P.T + t) * Nd;
  const double dn = (double)n_pig;

  auto flags = [&](int i) {
    I3 v{0, 0, 0};
    if (i < n) {
      const int d = order[i0 + i];
      if (dt_rank[d] < max_det) {
        const bool mt = dtm[plane + d] != 0, ig = dtig[plane + d] != 0;
        v.k = 1; v.t = (mt && !ig) ? 1 : 0; v.f = (!mt && !ig) ? 1 : 0;
      }
    }
    return v;
  };

  // forward: running sums; the position where the recall first reaches each threshold (searchsorted(side='left'), :410)
  I3 carry{0, 0, 0};
  for (int base = 0; base < n; base += kThreads) {
    const I3 f = flags(base + tid);
    I3 s = nnl_block_scan<kWaves>(f, i3_add, kZero3, lds_i, tot);
    s.k += carry.k; s.t += carry.t; s.f += carry.f;
    if (f.k && (f.t || s.k == 1)) {
      const double rc = (double)s.t / dn;
      const int r_lo = s.k == 1 ? 0 : upper_bound(rec, R, (double)(s.t - f.t) / dn);
      const int r_hi = upper_bound(rec, R, rc);
      for (int r = r_lo; r < r_hi; ++r) pos[r] = base + tid;
    }
    carry.k += tot.k; carry.t += tot.t; carry.f += tot.f;
  }
  __syncthreads();
  if (tid == 0) recall[rc_at] = carry.k ? (double)carry.t / dn : 0.0;        // :397-400

  // backward: the same sums from the totals, precision, its running maximum from the right (:406-408), and the picks (:412-414)
  I3 end = carry;
  double right = -1.0, tile_max;
  const double eps = 2.220446049250313e-16;                                  // np.spacing(1)
  for (int base = ((n - 1) / kThreads) * kThreads; n > 0 && base >= 0; base -= kThreads) {
    const I3 f = flags(base + tid);
    I3 s = nnl_block_scan<kWaves>(f, i3_add, kZero3, lds_i, tot);
    const I3 start{end.k - tot.k, end.t - tot.t, end.f - tot.f};
    s.t += start.t; s.f += start.f;
    const double pr = f.k ? (double)s.t / ((double)s.f + (double)s.t + eps) : -1.0;
    const double sm = fmax(nnl_block_scan<kWaves, true>(pr, NnlMax(), (double)-INFINITY, lds_d, tile_max), right);
    tile[tid] = sm;
    __syncthreads();
    for (int r = tid; r < R; r += kThreads) {
      const int p = pos[r];
      if (p >= base && p < base + kThreads) {
        precision[out0 + r * rstride] = tile[p - base];
        scores[out0 + r * rstride] = dt_score[order[i0 + p]];
      }
    }
    right = tile[0];
    __syncthreads();
    end = start;
  }
  for (int r = tid; r < R; r += kThreads)
    if (pos[r] < 0) { precision[out0 + r * rstride] = 0.0; scores[out0 + r * rstride] = 0.0; }   // not reached: the try / except of :411-416
}

// ---- c. mAP1 matching ------------------------------------------------------------------------------------------------------------

// Vision.py:1696-1728 for one group per wave: lanes take ground truths, each walks the group's predictions
__global__ __launch_bounds__(NNL_WAVE) void map_match_kernel(const int32_t* __restrict__ pr_off, const int32_t* __restrict__ gt_off,
                                                             const float* __restrict__ pr_box, const float* __restrict__ gt_box,
                                                             MapParams P, int64_t Np, uint8_t* __restrict__ correct) {
  const int64_t g = blockIdx.x;
  const int p0 = pr_off[g], n = pr_off[g + 1] - p0, q0 = gt_off[g], G = gt_off[g + 1] - q0;
  if (n == 0) return;
  for (int j = threadIdx.x; j < G; j += NNL_WAVE) {
    const float* tb = gt_box + (int64_t)(q0 + j) * 4;
    const float t0 = tb[0], t1 = tb[1], t2 = tb[2], t3 = tb[3];
    const float a1 = (t2 - t0) * (t3 - t1);
    float best = 0.f;
    int arg = 0;
    for (int p = 0; p < n; ++p) {
      const float* pb = pr_box + (int64_t)(p0 + p) * 4;
      const float a2 = (pb[2] - pb[0]) * (pb[3] - pb[1]);
      const float iw = fmaxf(fminf(t2, pb[2]) - fmaxf(t0, pb[0]), 0.f);
      const float ih = fmaxf(fminf(t3, pb[3]) - fmaxf(t1, pb[1]), 0.f);
      const float inter = iw * ih;
      const float v = inter / (a1 + a2 - inter);
      if (p == 0 || v > best || (v != v && best == best)) { best = v; arg = p; }      // the first maximum; a NaN wins, as in argmax
    }
    for (int t = 0; t < P.T; ++t)
      if ((double)best > P.thr[t]) correct[(int64_t)t * Np + p0 + arg] = 1;          // strictly above (:1727); racing writers agree
  }
}

// ---- d. mAP1 integration ------------------------------------------------------------------------------------------------------

// Vision.py:1730-1747 for one (category c, threshold t).  Inside a run of equal scores the correct predictions come first
// (sorted(zip(score, correct), reverse=True)): the j-th correct one of a run that starts at position h (0-based) after q correct ones
// sits at position h + j (1-based) and is the (q + j)-th correct overall, whichever members of the run are the correct ones.
__global__ __launch_bounds__(kThreads) void map_integrate_kernel(const int32_t* __restrict__ cat_pr_off, const int32_t* __restrict__ order,
                                                                 const double* __restrict__ score, const uint8_t* __restrict__ correct,
                                                                 const int64_t* __restrict__ ntrue, int64_t C, int64_t Np,
                                                                 double* __restrict__ scratch, double* __restrict__ out) {
  __shared__ I3 lds_i[kWaves];
  __shared__ unsigned long long lds_u[kWaves];
  __shared__ double lds_d[kWaves];
  const int tid = threadIdx.x;
  const int c = blockIdx.x % C, t = blockIdx.x / C;
  const int i0 = cat_pr_off[c], n = cat_pr_off[c + 1] - i0;
  const uint8_t* ok = correct + (int64_t)t * Np;
  double* v = scratch + (int64_t)t * Np + i0;

  int seen = 0;                                   // correct predictions before the tile
  unsigned long long head = 0;                    // (start of the current run) << 32 | correct predictions before it
  for (int base = 0; base < n; base += kThreads) {
    const int i = base + tid;
    I3 f{0, 0, 0}, tot;
    unsigned long long key = 0, ktot;
    if (i < n) {
      f.k = ok[order[i0 + i]] ? 1 : 0;
    }
    I3 s = nnl_block_scan<kWaves>(f, i3_add, kZero3, lds_i, tot);
    s.k += seen;
    if (i < n && (i == 0 || score[order[i0 + i]] != score[order[i0 + i - 1]]))
      key = ((unsigned long long)(unsigned)i << 32) | (unsigned)(s.k - f.k);
    key = nnl_block_scan<kWaves>(key, NnlMax(), 0ULL, lds_u, ktot);      // 0: "nothing seen", below every key
    if (head > key) key = head;
    if (i < n) {
      const int h = (int)(key >> 32), q = (int)(key & 0xffffffffULL);
      v[i] = f.k ? (double)s.k * (1.0 / (double)(h + s.k - q)) : 0.0;        // tp * (1 / position), as :1741-1742
    }
    seen += tot.k;
    if (ktot > head) head = ktot;
  }
  // backward: running maximum from the right over the correct positions, summed at the correct positions (:1744-1747)
  double right = 0.0, acc = 0.0, tile_max;
  for (int base = ((n - 1) / kThreads) * kThreads; n > 0 && base >= 0; base -= kThreads) {
    const int i = base + tid;
    const double x = i < n ? v[i] : 0.0;
    const double sm = fmax(nnl_block_scan<kWaves, true>(x, NnlMax(), (double)-INFINITY, lds_d, tile_max), right);
    if (x > 0.0) acc += sm;
    right = fmax(tile_max, right);               // what thread 0 holds: the maximum from this tile's first position on
  }
  const double total = nnl_block_reduce<kWaves>(acc, NnlSum(), lds_d);
  if (tid == 0) out[(int64_t)t * C + c] = total / (double)ntrue[c];          // 0 / 0 = nan without ground truth, as the host gives
}

bool finite_all(const double* v, int n) {
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

}  // namespace

extern "C" int nnl_det_coco_match(const int32_t* dt_off, const int32_t* gt_off, const double* dt_box, const double* gt_box,
                                  const double* gt_area, const uint8_t* gt_flags, const int64_t* scr_off, int64_t NG, int64_t Nd, int64_t Ng,
                                  const double* iou_thrs, int64_t T, const double* area_rng, int64_t A, void* scratch, size_t scratch_bytes,
                                  int32_t* dtm, uint8_t* dtig, int32_t* npig, int32_t* status, void* stream) {
  NNL_CHECK_ARG(dt_off && gt_off && scr_off && iou_thrs && area_rng && npig && status, "det_coco_match: null pointer");
  NNL_CHECK_ARG(NG >= 1 && NG < ((int64_t)1 << 31), "det_coco_match: NG must lie in [1, 2^31) (got %lld)", (long long)NG);
  NNL_CHECK_ARG(Nd >= 0 && Nd < ((int64_t)1 << 31) && Ng >= 0 && Ng < ((int64_t)1 << 31),
                "det_coco_match: Nd and Ng must lie in [0, 2^31) (got %lld, %lld)", (long long)Nd, (long long)Ng);
  NNL_CHECK_ARG(Nd == 0 || (dt_box && dtm && dtig), "det_coco_match: null detection pointer");
  NNL_CHECK_ARG(Ng == 0 || (gt_box && gt_area && gt_flags), "det_coco_match: null ground-truth pointer");
  NNL_CHECK_ARG(T >= 1 && T <= NNL_DET_EVAL_MAX_T && A >= 1 && A <= NNL_DET_EVAL_MAX_A,
                "det_coco_match: T must lie in [1, %d] and A in [1, %d] (got %lld, %lld)", NNL_DET_EVAL_MAX_T, NNL_DET_EVAL_MAX_A,
                (long long)T, (long long)A);
  NNL_CHECK_ARG(finite_all(iou_thrs, (int)T) && finite_all(area_rng, 2 * (int)A), "det_coco_match: a threshold or area bound is not finite");
  NNL_CHECK_ARG(scratch_bytes == 0 || scratch, "det_coco_match: null scratch of %zu bytes", scratch_bytes);
  MatchParams P;
  P.T = (int)T; P.A = (int)A;
  for (int t = 0; t < T; ++t) P.thr[t] = iou_thrs[t];
  for (int a = 0; a < A; ++a) { P.lo[a] = area_rng[2 * a]; P.hi[a] = area_rng[2 * a + 1]; }
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_ELEMENTWISE, s, 32.0 * (double)Nd + 41.0 * (double)Ng + 5.0 * (double)A * (double)T * (double)Nd);
  NNL_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
  NNL_ROUTE("det_coco_match:lanes=%d", (int)(A * T));
  coco_match_kernel<<<dim3((unsigned)NG), dim3(NNL_WAVE), 0, s>>>(dt_off, gt_off, dt_box, gt_box, gt_area, gt_flags, scr_off, (double*)scratch,
                                                                  (int64_t)(scratch_bytes / sizeof(double)), P, NG, Nd, dtm, dtig, npig, status);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}

extern "C" int nnl_det_coco_accumulate(const int32_t* cat_grp_off, const int32_t* cat_dt_off, const int32_t* order, const int32_t* dt_rank,
                                       const double* dt_score, const int32_t* dtm, const uint8_t* dtig, const int32_t* npig, int64_t K,
                                       int64_t NG, int64_t Nd, int64_t T, int64_t A, const int32_t* max_dets, int64_t M,
                                       const double* rec_thrs, int64_t R, double* precision, double* scores, double* recall, void* stream) {
  NNL_CHECK_ARG(cat_grp_off && cat_dt_off && npig && max_dets && rec_thrs && precision && scores && recall, "det_coco_accumulate: null pointer");
  NNL_CHECK_ARG(Nd == 0 || (order && dt_rank && dt_score && dtm && dtig), "det_coco_accumulate: null detection pointer");
  NNL_CHECK_ARG(K >= 1 && NG >= 1 && NG < ((int64_t)1 << 31) && Nd >= 0 && Nd < ((int64_t)1 << 31),
                "det_coco_accumulate: K >= 1, NG in [1, 2^31) and Nd in [0, 2^31) (got %lld, %lld, %lld)", (long long)K, (long long)NG, (long long)Nd);
  NNL_CHECK_ARG(T >= 1 && T <= NNL_DET_EVAL_MAX_T && A >= 1 && A <= NNL_DET_EVAL_MAX_A && M >= 1 && M <= NNL_DET_EVAL_MAX_M && R >= 1 &&
                    R <= NNL_DET_EVAL_MAX_R,
                "det_coco_accumulate: T in [1, %d], A in [1, %d], M in [1, %d], R in [1, %d] (got %lld, %lld, %lld, %lld)", NNL_DET_EVAL_MAX_T,
                NNL_DET_EVAL_MAX_A, NNL_DET_EVAL_MAX_M, NNL_DET_EVAL_MAX_R, (long long)T, (long long)A, (long long)M, (long long)R);
  NNL_CHECK_ARG(K * A * M * T < ((int64_t)1 << 31), "det_coco_accumulate: K x A x M x T = %lld curves, above 2^31", (long long)(K * A * M * T));
  for (int64_t m = 0; m < M; ++m) NNL_CHECK_ARG(max_dets[m] >= 1, "det_coco_accumulate: maxDets[%lld] is below 1", (long long)m);
  NNL_CHECK_ARG(finite_all(rec_thrs, (int)R), "det_coco_accumulate: a recall threshold is not finite");
  for (int64_t r = 1; r < R; ++r) NNL_CHECK_ARG(rec_thrs[r - 1] <= rec_thrs[r], "det_coco_accumulate: recThrs must ascend (at %lld)", (long long)r);
  AccumParams P;
  P.T = (int)T; P.A = (int)A; P.M = (int)M; P.R = (int)R;
  for (int m = 0; m < M; ++m) P.max_dets[m] = max_dets[m];
  for (int r = 0; r < R; ++r) P.rec[r] = rec_thrs[r];
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_ELEMENTWISE, s, 2.0 * (double)M * (double)A * (double)T * 13.0 * (double)Nd + 16.0 * (double)(T * R * K * A * M));
  NNL_ROUTE("det_coco_accumulate:curves=%lld", (long long)(K * A * M * T));
  coco_accumulate_kernel<<<dim3((unsigned)(K * A * M * T)), dim3(kThreads), 0, s>>>(cat_grp_off, cat_dt_off, order, dt_rank, dt_score, dtm, dtig,
                                                                                   npig, P, K, NG, Nd, precision, scores, recall);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}

extern "C" int nnl_det_map_match(const int32_t* pr_off, const int32_t* gt_off, const float* pr_box, const float* gt_box, int64_t NG,
                                 int64_t Np, int64_t Ng, const double* thrs, int64_t T, uint8_t* correct, void* stream) {
  NNL_CHECK_ARG(pr_off && gt_off && thrs, "det_map_match: null pointer");
  NNL_CHECK_ARG(NG >= 1 && NG < ((int64_t)1 << 31), "det_map_match: NG must lie in [1, 2^31) (got %lld)", (long long)NG);
  NNL_CHECK_ARG(Np >= 0 && Np < ((int64_t)1 << 31) && Ng >= 0 && Ng < ((int64_t)1 << 31),
                "det_map_match: Np and Ng must lie in [0, 2^31) (got %lld, %lld)", (long long)Np, (long long)Ng);
  NNL_CHECK_ARG(Np == 0 || (pr_box && correct), "det_map_match: null prediction pointer");
  NNL_CHECK_ARG(Ng == 0 || gt_box, "det_map_match: null ground-truth pointer");
  NNL_CHECK_ARG(T >= 1 && T <= NNL_DET_EVAL_MAX_T, "det_map_match: T must lie in [1, %d] (got %lld)", NNL_DET_EVAL_MAX_T, (long long)T);
  NNL_CHECK_ARG(finite_all(thrs, (int)T), "det_map_match: a threshold is not finite");
  MapParams P;
  P.T = (int)T;
  for (int t = 0; t < T; ++t) P.thr[t] = thrs[t];
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_ELEMENTWISE, s, 16.0 * (double)(Np + Ng) + (double)T * (double)Np);
  if (Np == 0) return NNL_OK;
  NNL_CHECK_HIP(hipMemsetAsync(correct, 0, (size_t)T * (size_t)Np, s));
  map_match_kernel<<<dim3((unsigned)NG), dim3(NNL_WAVE), 0, s>>>(pr_off, gt_off, pr_box, gt_box, P, Np, correct);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}

extern "C" size_t nnl_det_map_integrate_workspace_bytes(int64_t Np, int64_t T) {
  if (Np < 0 || T < 1 || Np >= ((int64_t)1 << 31) || T > NNL_DET_EVAL_MAX_T) return 0;
  return sizeof(double) * (size_t)Np * (size_t)T;
}

extern "C" int nnl_det_map_integrate(const int32_t* cat_pr_off, const int32_t* order, const double* score, const uint8_t* correct,
                                     const int64_t* ntrue, int64_t C, int64_t Np, int64_t T, void* workspace, size_t workspace_bytes,
                                     double* out, void* stream) {
  NNL_CHECK_ARG(cat_pr_off && ntrue && out, "det_map_integrate: null pointer");
  NNL_CHECK_ARG(C >= 1 && T >= 1 && T <= NNL_DET_EVAL_MAX_T && C * T < ((int64_t)1 << 31),
                "det_map_integrate: C >= 1, T in [1, %d] and C x T below 2^31 (got %lld, %lld)", NNL_DET_EVAL_MAX_T, (long long)C, (long long)T);
  NNL_CHECK_ARG(Np >= 0 && Np < ((int64_t)1 << 31), "det_map_integrate: Np must lie in [0, 2^31) (got %lld)", (long long)Np);
  NNL_CHECK_ARG(Np == 0 || (order && score && correct), "det_map_integrate: null prediction pointer");
  const size_t need = nnl_det_map_integrate_workspace_bytes(Np, T);
  if (need > 0 && (!workspace || workspace_bytes < need))
    return nnl_set_error(NNL_ERR_WORKSPACE, "det_map_integrate: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_ELEMENTWISE, s, (double)T * (double)Np * (4.0 + 8.0 + 1.0 + 16.0) + 8.0 * (double)(C * T));
  map_integrate_kernel<<<dim3((unsigned)(C * T)), dim3(kThreads), 0, s>>>(cat_pr_off, order, score, correct, ntrue, C, Np, (double*)workspace, out);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}
