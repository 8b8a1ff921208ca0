// K5d — language-model text generation (LanguageModelNet.predict_from_string, reference Applications/Text.py:655-676): the decode
// regime, batch 1 and one timestep, where every layer is a matrix-vector product that reads each weight once per token.  fp32 only.
//  * nnl_lstm_cell_b1: one LSTM layer, one timestep, batch 1.  One wave owns hidden unit j: it streams the four gate rows j, H+j,
//    2H+j, 3H+j of w_ih and w_hh straight into registers with 16-byte loads (no LDS staging: nothing is reused), reduces over its 64
//    lanes, and lane 0 applies the cell.  A unit needs no other unit's result, so a layer is one plain launch.
//  * nnl_lm_next_token: tied decoder, softmax, special-token mask, top-k and the seeded draw in two launches.  The slice kernel gives
//    each workgroup kSliceRows vocabulary rows: logits stay in LDS, and what leaves is the slice max, the slice sum of exponentials
//    and the slice's k largest eligible (logit, index) pairs.  The pick kernel (one workgroup) merges the partials, keeps the global
//    top-k in descending order, turns them into exp(l - max) / sum over ALL V entries, and draws.
// No kernel synchronises across workgroups: the launch boundary is the only barrier.  Every sum has a fixed order: repeatable bit for bit.
#include <limits.h>

#include "nnl_common.h"

namespace {

constexpr int kCellWaves = 4;                   // hidden units per workgroup (one wave each)
constexpr int kSliceRows = 64;                  // vocabulary rows per workgroup of the slice kernel (= one wave for the slice statistics)
constexpr int kBlock = 256;
constexpr int kMaxK = 64;
constexpr int kMaxSlices = 4096;                // the pick kernel keeps every slice's head (logit, index) in LDS: 32 KB
constexpr int kMaxLd = 8192;                    // the slice kernel keeps h in LDS

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

__device__ __forceinline__ float dot4(const float4 a, const float4 b, float acc) {
  acc = fmaf(a.x, b.x, acc);
  acc = fmaf(a.y, b.y, acc);
  acc = fmaf(a.z, b.z, acc);
  return fmaf(a.w, b.w, acc);
}

// elements [4q, 4q+4) of a vector with n valid entries; one 16-byte load where the vector allows it
__device__ __forceinline__ float4 vec4(const float* v, int n, bool aligned, int q) {
  const int k = 4 * q;
  if (aligned && k + 4 <= n) return ld4(v + k);
  float4 r;
  r.x = k < n ? v[k] : 0.f;
  r.y = k + 1 < n ? v[k + 1] : 0.f;
  r.z = k + 2 < n ? v[k + 2] : 0.f;
  r.w = k + 3 < n ? v[k + 3] : 0.f;
  return r;
}

// acc[g] += w[g*H + j, :] . v for the four gates; rows of ld floats (ld % 4 == 0), v has n valid entries (the rest counts as zero).
// With one wave per unit a SIMD holds about one wave (H = 1150: 1152 waves on 1024 SIMDs), so the loads in flight are what ONE wave
// issues: four 64-lane chunks per trip, sixteen 16-byte weight loads per lane, then two, then one.
__device__ __forceinline__ void gate_rows_dot(const float* __restrict__ w, long ld, int H, int j, const float* __restrict__ v, int n,
                                              int lane, float acc[4]) {
  const bool aligned = (reinterpret_cast<uintptr_t>(v) & 15) == 0;
  const int nq = (int)(ld >> 2);
  const float* r0 = w + (long)j * ld;
  const float* r1 = w + ((long)H + j) * ld;
  const float* r2 = w + (2L * H + j) * ld;
  const float* r3 = w + (3L * H + j) * ld;
  int q = lane;
  for (; q + 192 < nq; q += 256) {
    float4 a[4][4], vv[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      a[c][0] = ld4(r0 + 4 * q + 256 * c);
      a[c][1] = ld4(r1 + 4 * q + 256 * c);
      a[c][2] = ld4(r2 + 4 * q + 256 * c);
      a[c][3] = ld4(r3 + 4 * q + 256 * c);
      vv[c] = vec4(v, n, aligned, q + 64 * c);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[g] = dot4(a[c][g], vv[c], acc[g]);
    }
  }
  for (; q + 64 < nq; q += 128) {
    const float4 a0 = ld4(r0 + 4 * q), a1 = ld4(r1 + 4 * q), a2 = ld4(r2 + 4 * q), a3 = ld4(r3 + 4 * q);
    const float4 b0 = ld4(r0 + 4 * q + 256), b1 = ld4(r1 + 4 * q + 256), b2 = ld4(r2 + 4 * q + 256), b3 = ld4(r3 + 4 * q + 256);
    const float4 va = vec4(v, n, aligned, q), vb = vec4(v, n, aligned, q + 64);
    acc[0] = dot4(b0, vb, dot4(a0, va, acc[0]));
    acc[1] = dot4(b1, vb, dot4(a1, va, acc[1]));
    acc[2] = dot4(b2, vb, dot4(a2, va, acc[2]));
    acc[3] = dot4(b3, vb, dot4(a3, va, acc[3]));
  }
  if (q < nq) {
    const float4 a0 = ld4(r0 + 4 * q), a1 = ld4(r1 + 4 * q), a2 = ld4(r2 + 4 * q), a3 = ld4(r3 + 4 * q);
    const float4 va = vec4(v, n, aligned, q);
    acc[0] = dot4(a0, va, acc[0]);
    acc[1] = dot4(a1, va, acc[1]);
    acc[2] = dot4(a2, va, acc[2]);
    acc[3] = dot4(a3, va, acc[3]);
  }
}


// x == nullptr: the input is row tokens[pos] of emb [V, ld_emb] (I valid entries), read on the device; an id outside [0, V) reads as a zero row
__global__ __launch_bounds__(kCellWaves * 64) void lstm_cell_b1_kernel(
    const float* __restrict__ w_ih, long ldi, const float* __restrict__ w_hh, long ldh, const float* __restrict__ bias,
    const float* __restrict__ x, const float* __restrict__ emb, long ld_emb, const int64_t* __restrict__ tokens, long pos, long V,
    const float* __restrict__ h, const float* c, float* __restrict__ h_out, float* c_out, int I, int H) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * kCellWaves + (threadIdx.x >> 6);
  if (j >= H) return;                            // whole waves leave; no barrier below
  const float* xv = x;
  int xn = (int)ldi;                             // a vector input is zero-padded to ldi
  if (x == nullptr) {
    const int64_t id = tokens[pos];
    const bool ok = id >= 0 && id < V;
    xv = emb + (ok ? id : 0) * ld_emb;
    xn = ok ? I : 0;
  }
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  gate_rows_dot(w_ih, ldi, H, j, xv, xn, lane, acc);
  gate_rows_dot(w_hh, ldh, H, j, h, (int)ldh, lane, acc);
#pragma unroll
  for (int g = 0; g < 4; ++g) acc[g] = nnl_wave_sum(acc[g]);
  if (lane == 0) {                               // torch's gate order: i, f, g, o
    const float gi = nnl_sigmoid(acc[0] + bias[j]);
    const float gf = nnl_sigmoid(acc[1] + bias[H + j]);
    const float gg = tanhf(acc[2] + bias[2 * H + j]);
    const float go = nnl_sigmoid(acc[3] + bias[3 * H + j]);
    const float cn = gf * c[j] + gi * gg;
    c_out[j] = cn;
    h_out[j] = go * tanhf(cn);
  }
}

// ---- next token ------------------------------------------------------------------------------------------------------------------
// partials of slice s: part[s * (2 + 2k)] = { max, sum exp(l - max), k logits (descending; -inf past the eligible ones), k indices (int bits) }

__device__ __forceinline__ bool better(float av, int ai, float bv, int bi) { return av > bv || (av == bv && ai < bi); }

__global__ __launch_bounds__(kBlock) void lm_slice_kernel(const float* __restrict__ emb, long ld, const float* __restrict__ h, int E,
                                                          int V, int k, int n_special, float* __restrict__ part,
                                                          float* __restrict__ logits_out) {
  extern __shared__ __align__(16) float hs[];    // h, zero past E: ld floats
  __shared__ float lg[kSliceRows];
  const int tid = threadIdx.x;
  for (int i = tid; i < ld; i += kBlock) hs[i] = i < E ? h[i] : 0.f;
  __syncthreads();
  const int v0 = blockIdx.x * kSliceRows;
  const int group = tid >> 4, sub = tid & 15;    // 16 lanes per row, 16 rows per pass, 4 passes: 4 independent rows in flight per lane
  const int nq = (int)(ld >> 2);
  const float* rows[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int v = v0 + p * 16 + group;
    rows[p] = emb + (long)(v < V ? v : V - 1) * ld;   // rows past V re-read the last row (in bounds) and are dropped below
  }
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
  for (int q = sub; q < nq; q += 16) {
    const float4 a0 = ld4(rows[0] + 4 * q), a1 = ld4(rows[1] + 4 * q), a2 = ld4(rows[2] + 4 * q), a3 = ld4(rows[3] + 4 * q);
    const float4 b = *reinterpret_cast<const float4*>(hs + 4 * q);
    acc[0] = dot4(a0, b, acc[0]);
    acc[1] = dot4(a1, b, acc[1]);
    acc[2] = dot4(a2, b, acc[2]);
    acc[3] = dot4(a3, b, acc[3]);
  }
#pragma unroll
  for (int p = 0; p < 4; ++p) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) acc[p] += __shfl_xor(acc[p], o, 64);
    const int r = p * 16 + group, v = v0 + r;
    if (sub == 0) {
      lg[r] = v < V ? acc[p] : -INFINITY;
      if (logits_out && v < V) logits_out[v] = acc[p];
    }
  }
  __syncthreads();
  if (tid >= kSliceRows) return;                 // the slice statistics are one wave's work
  const int v = v0 + tid;
  const float l = lg[tid];
  const float m = nnl_wave_max(l);
  const float s = nnl_wave_sum(v < V ? expf(l - m) : 0.f);
  float* out = part + (long)blockIdx.x * (2 + 2 * k);
  int* out_idx = reinterpret_cast<int*>(out + 2 + k);
  if (tid == 0) { out[0] = m; out[1] = s; }
  const int hi = v0 + kSliceRows < V ? v0 + kSliceRows : V;
  const int lo = v0 > n_special ? v0 : n_special;
  const int n_elig = hi > lo ? hi - lo : 0;      // eligible rows of this slice: ranks 0 .. n_elig-1 below, the other slots hold the sentinel
  if (tid < k && tid >= n_elig) { out[2 + tid] = -INFINITY; out_idx[tid] = INT_MAX; }
  if (v < V && v >= n_special) {
    int rank = 0;                                // ties go to the lower index
    for (int j = lo - v0; j < hi - v0; ++j) rank += better(lg[j], j, l, tid) ? 1 : 0;
    if (rank < k) { out[2 + rank] = l; out_idx[rank] = v; }
  }
}

struct Cand { float v; int i; int s; };

__device__ __forceinline__ Cand cand_best(Cand a, Cand b) { return better(b.v, b.i, a.v, a.i) ? b : a; }

constexpr Cand kNoCand = {-INFINITY, INT_MAX, -1};

// the best remaining head among the slices this thread owns (s = tid, tid + kBlock, ...); a taken or empty slice holds index INT_MAX
__device__ __forceinline__ Cand own_best(const float* hv, const int* hi, int n_slices, int tid) {
  Cand best = kNoCand;
  for (int s = tid; s < n_slices; s += kBlock)
    if (hi[s] != INT_MAX) best = cand_best(best, Cand{hv[s], hi[s], s});
  return best;
}

// One workgroup.  (1) global max and the sum rescaled to it; (2) the k slices with the best heads — every member of the global top-k lies
// in one of them, since k better heads would be k better candidates; (3) their k sorted lists, fetched into LDS in one round trip, are
// merged by one wave; (4) probabilities, partial sums, draw.  Global memory is read in three independent sweeps, never once per round.
__global__ __launch_bounds__(kBlock) void lm_pick_kernel(const float* __restrict__ part, int n_slices, int k, const float* __restrict__ u,
                                                         long step, int64_t* __restrict__ tokens, long pos,
                                                         float* __restrict__ top_probs, int64_t* __restrict__ top_indices) {
  extern __shared__ __align__(16) float dyn[];   // (2): hv[n_slices], hi[n_slices]; (3): lv[k * k], li[k * k]
  constexpr int kWaves = kBlock / NNL_WAVE;
  __shared__ float wv[kWaves];
  __shared__ Cand wc[kWaves];
  __shared__ int sel[kMaxK];
  __shared__ float top_v[kMaxK], csum[kMaxK];
  __shared__ int top_i[kMaxK];
  const int tid = threadIdx.x, lane = tid & 63;
  const int stride = 2 + 2 * k;
  float* hv = dyn;
  int* hi = reinterpret_cast<int*>(dyn + n_slices);
  // thread-sequential over the owned slices, xor tree over the wave, waves in order: a fixed order
  float m = -INFINITY;
  for (int s = tid; s < n_slices; s += kBlock) {
    const float* p = part + (long)s * stride;
    m = fmaxf(m, p[0]);
    hv[s] = p[2];
    hi[s] = reinterpret_cast<const int*>(p + 2 + k)[0];
  }
  const float M = nnl_block_reduce<kWaves>(m, NnlMax(), wv);
  float sum = 0.f;
  for (int s = tid; s < n_slices; s += kBlock) sum += part[(long)s * stride + 1] * expf(part[(long)s * stride] - M);
  const float S = nnl_block_reduce<kWaves>(sum, NnlSum(), wv);
  Cand mine = own_best(hv, hi, n_slices, tid);
  for (int r = 0; r < k; ++r) {
    const Cand w = nnl_block_reduce<kWaves>(mine, cand_best, wc);
    if (tid == 0) sel[r] = w.s;                  // -1: fewer than k slices hold an eligible entry
    if (w.s >= 0 && (w.s % kBlock) == tid) {     // its owner takes the winning slice out (a thread reads only its own slices' heads)
      hi[w.s] = INT_MAX;
      mine = own_best(hv, hi, n_slices, tid);
    }
  }
  __syncthreads();                               // sel[] is complete, hv / hi are dead
  float* lv = dyn;
  int* li = reinterpret_cast<int*>(dyn + k * k);
  for (int t = tid; t < k * k; t += kBlock) {
    const int sl = sel[t / k], q = t % k;
    const float* p = part + (long)(sl < 0 ? 0 : sl) * stride;
    lv[t] = sl < 0 ? -INFINITY : p[2 + q];
    li[t] = sl < 0 ? INT_MAX : reinterpret_cast<const int*>(p + 2 + k)[q];
  }
  __syncthreads();
  if (tid >= NNL_WAVE) return;
  int hd = 0;                                    // lane t < k owns list t
  auto head_of = [&](int h) { return (lane < k && h < k && li[lane * k + h] != INT_MAX) ? Cand{lv[lane * k + h], li[lane * k + h], lane} : kNoCand; };
  Cand cur = head_of(0);
  for (int r = 0; r < k; ++r) {
    const Cand w = nnl_wave_reduce(cur, cand_best);
    if (lane == 0) { top_v[r] = w.v; top_i[r] = w.i; }
    if (w.s == lane) cur = head_of(++hd);
  }
  if (lane == 0) {
    // the reference's probabilities exp(l - max) / sum over all V entries, their sequential fp32 partial sums c_m, and the draw:
    // slot j = #{ m in 1..k-1 : c_m <= u * c_k }
    float c = 0.f;
    for (int q = 0; q < k; ++q) {
      const float p = expf(top_v[q] - M) / S;
      c = c + p;
      csum[q] = c;
      if (top_probs) top_probs[step * k + q] = p;
      if (top_indices) top_indices[step * k + q] = top_i[q];
    }
    const float t = u[step] * csum[k - 1];
    int j = 0;
    for (int q = 0; q + 1 < k; ++q) j += csum[q] <= t ? 1 : 0;
    tokens[pos + 1] = top_i[j];
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int nnl_lstm_cell_b1(const float* w_ih, int64_t ldi, const float* w_hh, int64_t ldh, const float* bias, const float* x,
                                const float* emb, int64_t ld_emb, const int64_t* tokens, int64_t pos, int64_t V, const float* h,
                                const float* c, float* h_out, float* c_out, int64_t I, int64_t H, void* stream) {
  NNL_CHECK_ARG(I > 0 && H > 0 && H < (1 << 28) && I < (1 << 28), "lstm_cell_b1: bad sizes");
  NNL_CHECK_ARG(ldi >= I && ldh >= H && ldi % 4 == 0 && ldh % 4 == 0 && ldi < (1 << 28) && ldh < (1 << 28),
                "lstm_cell_b1: leading dimensions must be multiples of 4 floats (16-byte rows) and cover I / H");
  NNL_CHECK_ARG(w_ih && w_hh && bias && h && c && h_out && c_out, "lstm_cell_b1: null pointer");
  NNL_CHECK_ARG(aligned16(w_ih) && aligned16(w_hh) && aligned16(h) && (x == nullptr || aligned16(x)),
                "lstm_cell_b1: w_ih, w_hh, x and h must be 16-byte aligned");
  NNL_CHECK_ARG(h_out != h, "lstm_cell_b1: h_out must not alias h (every wave reads all of h)");
  if (x == nullptr)
    NNL_CHECK_ARG(emb && tokens && pos >= 0 && V > 0 && ld_emb >= I, "lstm_cell_b1: without x, an embedding table and a token position are needed");
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_LSTM, s, 8.0 * H * (ldi + ldh));
  NNL_ROUTE("lstm_cell_b1:%s", x ? "vec" : "tok");
  hipLaunchKernelGGL(lstm_cell_b1_kernel, dim3((unsigned)nnl_cdiv(H, kCellWaves)), dim3(kCellWaves * 64), 0, s, w_ih, (long)ldi, w_hh,
                     (long)ldh, bias, x, emb, (long)ld_emb, tokens, (long)pos, (long)V, h, c, h_out, c_out, (int)I, (int)H);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}

extern "C" size_t nnl_lm_next_token_workspace_bytes(int64_t V, int64_t k) {
  if (V <= 0 || k < 1 || k > kMaxK) return 0;
  return (size_t)nnl_cdiv(V, kSliceRows) * (size_t)(2 + 2 * k) * sizeof(float);
}

extern "C" int nnl_lm_next_token(const float* emb, int64_t ld_emb, const float* h, int64_t V, int64_t E, int64_t k, int64_t n_special,
                                 const float* u, int64_t step, int64_t* tokens, int64_t pos, float* top_probs, int64_t* top_indices,
                                 float* logits_out, void* workspace, size_t workspace_bytes, void* stream) {
  NNL_CHECK_ARG(V > 0 && V < (1L << 31) && E > 0 && n_special >= 0 && step >= 0 && pos >= -1, "lm_next_token: bad sizes");
  NNL_CHECK_ARG(k >= 1 && k <= kMaxK && k <= V - n_special, "lm_next_token: k must be in [1, 64] and at most the number of eligible tokens");
  NNL_CHECK_ARG(ld_emb >= E && ld_emb % 4 == 0, "lm_next_token: the table's leading dimension must be a multiple of 4 floats and cover E");
  NNL_CHECK_ARG(emb && h && u && tokens && aligned16(emb), "lm_next_token: null or unaligned pointer");
  const int64_t n_slices = nnl_cdiv(V, kSliceRows);
  if (n_slices > kMaxSlices || ld_emb > kMaxLd)
    return nnl_set_error(NNL_ERR_UNSUPPORTED, "lm_next_token: V above %d or rows above %d floats", kMaxSlices * kSliceRows, kMaxLd);
  if (workspace == nullptr || workspace_bytes < nnl_lm_next_token_workspace_bytes(V, k))
    return nnl_set_error(NNL_ERR_WORKSPACE, "lm_next_token: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_GEMM, s, 2.0 * V * E);
  NNL_ROUTE("lm_next_token@%d", (int)n_slices);
  hipLaunchKernelGGL(lm_slice_kernel, dim3((unsigned)n_slices), dim3(kBlock), (size_t)ld_emb * sizeof(float), s, emb, (long)ld_emb, h,
                     (int)E, (int)V, (int)k, (int)n_special, (float*)workspace, logits_out);
  NNL_CHECK_LAUNCH();
  hipLaunchKernelGGL(lm_pick_kernel, dim3(1), dim3(kBlock), sizeof(float) * 2 * (size_t)(n_slices > k * k ? n_slices : k * k), s, (const float*)workspace, (int)n_slices,
                     (int)k, u, (long)step, tokens, (long)pos, top_probs, top_indices);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}
