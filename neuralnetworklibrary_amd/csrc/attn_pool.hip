// K5c — attention pooling of the text classifier's decoder (TextClassificationDecoder.forward, Applications/Text.py:588-609),
// everything after attn1 = relu(Linear(enc_out)):
//   s[t,b] = h[t,b,:].w2 + b2;  q[:,b] = softmax of s[:,b] over the non-pad positions (x[b,t] != pad);
//   pooled[b,:] = sum_t q[t,b] enc[t,b,:].
// The reference takes the softmax over ALL t, masks and renormalises (Text.py:599-601); the two differ only in rounding, except
// that a column without a non-pad token divides 0 by 0 there: that column's attn and pooled are NaN here too.
//
// Schedule: one workgroup per (column b, chunk of L consecutive timesteps), blockIdx.x = b * nch + chunk.  A workgroup streams its
// rows once (h for the scores, then enc_out for the weighted sum: T*B*(E+A)*4 bytes in all) and writes a partial {chunk max, sum of
// exponentials, E-wide weighted sum} to a workspace slab; the last workgroup to arrive for a column (an agent-scope counter, zero at
// rest) merges the column's partials in chunk order.  No float atomics: every sum has a fixed order, results are bitwise repeatable.
//
// Hand-off (plain HIP): every thread ends its slab stores with an agent-scope release fence (each wave drains its stores and writes
// back its L2) before the barrier; one lane then takes a ticket with a relaxed agent-scope add; the last arriver acquires at agent
// scope in every wave before it reads any other workgroup's slab, and puts the counter back to zero.  Handed-off data is read
// through plain (not __restrict__) pointers, so the reads stay on the vector path behind the acquire.
#include "nnl_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / NNL_WAVE;
constexpr int kMaxRows = 512;            // rows of one chunk (LDS: the chunk's scores / weights)
constexpr int kMinRows = 8;              // a chunk's slab is ~1/L of its streamed bytes: keep L >= 8
constexpr int kTargetBlocks = 512;       // 2 workgroups per CU on the 256 CUs: every workgroup's release writes back its XCD's L2,
                                         // so fewer, longer chunks measured faster (B = 64, device time per fwd / bwd pair: 2048
                                         // workgroups 165 + 184 us at T = 300, 1024: 90 + 112, 512: 56 + 69, 256: 43 + 74)

struct Plan { long nch, L; };

Plan plan(long T, long B) {
  long nch = nnl_cdiv(kTargetBlocks, B);
  const long by_min = nnl_cdiv(T, kMinRows);
  if (nch > by_min) nch = by_min;
  const long by_max = nnl_cdiv(T, kMaxRows);
  if (nch < by_max) nch = by_max;
  if (nch < 1) nch = 1;
  const long L = nnl_cdiv(T, nch);
  return {nnl_cdiv(T, L), L};
}

// workspace layout, in floats.  Forward: scores [B*T] | {m, s} [B*nch*2] | weighted sums [B*nch*E].
// Backward: g [B*T] | c partials [B*nch] | dw2/db2 partials [B*nch*(A+1)] | column partials [B*(A+1)].
struct Layout { long sc, ms, acc, fwd_end, g, cpart, dwp, colp, bwd_end; };

Layout layout(long T, long B, long E, long A) {
  const Plan p = plan(T, B);
  auto up4 = [](long n) { return (n + 3) / 4 * 4; };     // 16-byte aligned sections
  Layout l;
  l.sc = 0;
  l.ms = up4(B * T);
  l.acc = l.ms + up4(B * p.nch * 2);
  l.fwd_end = l.acc + up4(B * p.nch * E);
  l.g = 0;
  l.cpart = up4(B * T);
  l.dwp = l.cpart + up4(B * p.nch);
  l.colp = l.dwp + up4(B * p.nch * (A + 1));
  l.bwd_end = l.colp + up4(B * (A + 1));
  return l;
}

// ---- rows as float4 units (length a multiple of 4, 16-byte aligned) or as scalars ------------------------------------
__device__ __forceinline__ float vld(const float* p, float) { return *p; }
__device__ __forceinline__ float4 vld(const float* p, float4) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void vst(float* p, float v) { *p = v; }
__device__ __forceinline__ void vst(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float vdot(float a, float b) { return a * b; }
__device__ __forceinline__ float vdot(float4 a, float4 b) { return (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w); }
__device__ __forceinline__ float vscale(float s, float v) { return s * v; }
__device__ __forceinline__ float4 vscale(float s, float4 v) { return make_float4(s * v.x, s * v.y, s * v.z, s * v.w); }
__device__ __forceinline__ float vadd(float a, float b) { return a + b; }
__device__ __forceinline__ float4 vadd(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 as4(float v) { return make_float4(v, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 as4(float4 v) { return v; }
__device__ __forceinline__ float from4(float4 v, float) { return v.x; }
__device__ __forceinline__ float4 from4(float4 v, float4) { return v; }
template <typename V> constexpr int vwidth() { return sizeof(V) / sizeof(float); }

// dot(row[0..n), w[0..n)) by one wave, lanes over the units of V: a fixed order
template <typename V>
__device__ __forceinline__ float wave_row_dot(const float* __restrict__ row, const float* __restrict__ w, int n, int lane) {
  constexpr int VW = vwidth<V>();
  float acc = 0.f;
  for (int k = lane; k < n / VW; k += NNL_WAVE) acc += vdot(vld(row + k * VW, V()), vld(w + k * VW, V()));
  return nnl_wave_sum(acc);
}

// publish this workgroup's stores and draw a ticket from *counter; true (in every thread) for the last of `n` arrivals, which
// then sees the stores of every other arrival: agent-scope release in every storing wave, agent-scope acquire in every wave
__device__ __forceinline__ bool arrive_last(int32_t* counter, int n, int* ticket_lds) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  __syncthreads();
  if (threadIdx.x == 0) *ticket_lds = __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  const bool last = *ticket_lds == n - 1;
  if (last) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (threadIdx.x == 0) __hip_atomic_store(counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // zero at rest
  }
  return last;
}

// threads over the `nu` units of a row, G = 256 / min(nu, 256) row groups (group gi takes rows gi, gi + G, ...)
struct Cols {
  int cpp, G, gi, c;
  __device__ Cols(int nu, int tid) {
    cpp = nu < kBlock ? nu : kBlock;
    G = kBlock / cpp;
    gi = tid / cpp;
    c = tid - gi * cpp;
  }
};

// ---- forward --------------------------------------------------------------------------------------------------------
struct FwdArgs {
  const float* h; const float* w2; const float* b2; const float* enc; const int64_t* x; int64_t pad;
  float* attn; float* pooled;
  int T, B, E, A, nch, L;
  float* sc; float* ms; float* acc;
  int32_t* counters;
};

template <typename VE, typename VA>
__global__ __launch_bounds__(kBlock) void attn_pool_fwd_kernel(FwdArgs p) {
  __shared__ float s_e[kMaxRows];                 // the chunk's scores, then exp(s - chunk max)
  __shared__ float4 s_part[kBlock];               // row-group partials of the weighted sum
  __shared__ float s_red[kWaves];
  __shared__ int s_ticket;
  constexpr int VW = vwidth<VE>();
  const int tid = threadIdx.x, lane = tid & (NNL_WAVE - 1), wave = tid / NNL_WAVE;
  const int b = blockIdx.x / p.nch, chunk = blockIdx.x - b * p.nch;
  const int t0 = chunk * p.L, L = min(p.L, p.T - t0);
  const long ld = (long)p.B;                      // [T, B, *] rows: row (t, b) = t * B + b
  const float b2 = *p.b2;

  // 1. scores of the chunk's rows, one wave per row; pads -> -inf
  for (int i = wave; i < L; i += kWaves) {
    const int t = t0 + i;
    const float d = wave_row_dot<VA>(p.h + ((long)t * ld + b) * p.A, p.w2, p.A, lane);
    if (lane == 0) s_e[i] = (p.x[(long)b * p.T + t] != p.pad) ? d + b2 : -INFINITY;
  }
  __syncthreads();
  float mloc = -INFINITY;
  for (int i = tid; i < L; i += kBlock) mloc = fmaxf(mloc, s_e[i]);
  const float m = nnl_block_reduce<kWaves>(mloc, NnlMax(), s_red);
  float* scol = p.sc + (long)b * p.T;
  for (int i = tid; i < L; i += kBlock) {
    const float s = s_e[i];
    scol[t0 + i] = s;                             // raw scores: the column's last arriver turns them into attn
    s_e[i] = (s == -INFINITY) ? 0.f : expf(s - m);
  }
  __syncthreads();
  float sloc = 0.f;
  for (int i = tid; i < L; i += kBlock) sloc += s_e[i];
  const float ssum = nnl_block_reduce<kWaves>(sloc, NnlSum(), s_red);

  // 2. weighted sum of the enc_out rows; row groups combined in order through LDS
  const int nu = p.E / VW;
  const Cols cl(nu, tid);
  const long slab = (long)b * p.nch + chunk;
  float* accp = p.acc + slab * p.E;
  const float* __restrict__ encb = p.enc + (long)b * p.E;
  const long rs = ld * p.E;                       // stride of consecutive t
  if (cl.gi < cl.G) {
    for (int j = cl.c; j < nu; j += cl.cpp) {
      const float* __restrict__ col = encb + j * VW;
      VE a = from4(make_float4(0.f, 0.f, 0.f, 0.f), VE());
      const int G = cl.G;
      int i = cl.gi;
      for (; i + 3 * G < L; i += 4 * G) {         // 4 rows' loads in flight
        const VE r0 = vld(col + (t0 + i) * rs, VE());
        const VE r1 = vld(col + (t0 + i + G) * rs, VE());
        const VE r2 = vld(col + (t0 + i + 2 * G) * rs, VE());
        const VE r3 = vld(col + (t0 + i + 3 * G) * rs, VE());
        a = vadd(a, vscale(s_e[i], r0));
        a = vadd(a, vscale(s_e[i + G], r1));
        a = vadd(a, vscale(s_e[i + 2 * G], r2));
        a = vadd(a, vscale(s_e[i + 3 * G], r3));
      }
      for (; i < L; i += G) a = vadd(a, vscale(s_e[i], vld(col + (t0 + i) * rs, VE())));
      if (cl.G == 1) vst(accp + j * VW, a);
      else s_part[tid] = as4(a);
    }
  }
  if (cl.G > 1) {
    __syncthreads();
    if (tid < cl.cpp) {
      float4 w = s_part[tid];
      for (int k = 1; k < cl.G; ++k) {
        const float4 o = s_part[k * cl.cpp + tid];
        w.x += o.x; w.y += o.y; w.z += o.z; w.w += o.w;
      }
      vst(accp + tid * VW, from4(w, VE()));
    }
  }
  if (tid == 0) {
    p.ms[2 * slab] = m;
    p.ms[2 * slab + 1] = ssum;
  }

  // 3. the column's last arriver merges the partials in chunk order: pooled[b,:] and attn[:,b]
  if (!arrive_last(p.counters + b, p.nch, &s_ticket)) return;
  const float* msb = p.ms + 2 * (long)b * p.nch;
  float ml = -INFINITY;
  for (int k = tid; k < p.nch; k += kBlock) ml = fmaxf(ml, msb[2 * k]);
  const float M = nnl_block_reduce<kWaves>(ml, NnlMax(), s_red);
  float sl = 0.f;
  for (int k = tid; k < p.nch; k += kBlock) {
    const float mk = msb[2 * k];
    sl += mk == -INFINITY ? 0.f : msb[2 * k + 1] * expf(mk - M);
  }
  const float S = nnl_block_reduce<kWaves>(sl, NnlSum(), s_red);           // 0 only when the column holds no non-pad token
  const float* accb = p.acc + (long)b * p.nch * p.E;
  for (int j = tid; j < p.E; j += kBlock) {
    float a = 0.f;
    for (int k = 0; k < p.nch; ++k) {
      const float mk = msb[2 * k];
      if (mk != -INFINITY) a += expf(mk - M) * accb[(long)k * p.E + j];
    }
    p.pooled[(long)b * p.E + j] = S > 0.f ? a / S : NAN;
  }
  for (int t = tid; t < p.T; t += kBlock) {
    const float s = scol[t];
    p.attn[(long)t * ld + b] = S > 0.f ? (s == -INFINITY ? 0.f : expf(s - M) / S) : NAN;
  }
}

// ---- backward -------------------------------------------------------------------------------------------------------
struct BwdArgs {
  const float* h; const float* w2; const float* enc; const float* attn; const float* dpooled; const float* dattn;
  float* dh; float* denc; float* dw2; float* db2;
  int T, B, E, A, nch, L;
  float* g; float* cpart; float* dwp; float* colp;
  int32_t* counters;
};

// launch 1, one pass over enc_out: g[t,b] = enc[t,b,:].dpooled[b,:] + dattn[t,b], denc[t,b,:] = q[t,b] dpooled[b,:], and the
// chunk's partial of c[b] = sum_t q g
template <typename VE>
__global__ __launch_bounds__(kBlock) void attn_pool_bwd1_kernel(BwdArgs p) {
  __shared__ float s_qg[kMaxRows];
  constexpr int VW = vwidth<VE>();
  const int tid = threadIdx.x, lane = tid & (NNL_WAVE - 1), wave = tid / NNL_WAVE;
  const int b = blockIdx.x / p.nch, chunk = blockIdx.x - b * p.nch;
  const int t0 = chunk * p.L, L = min(p.L, p.T - t0);
  const long ld = (long)p.B;
  const float* __restrict__ dp = p.dpooled + (long)b * p.E;
  const int nu = p.E / VW;
  for (int i = wave; i < L; i += kWaves) {
    const int t = t0 + i;
    const long row = ((long)t * ld + b) * p.E;
    const float q = p.attn[(long)t * ld + b];
    float acc = 0.f;
    for (int k = lane; k < nu; k += NNL_WAVE) {
      const VE d = vld(dp + k * VW, VE());
      acc += vdot(vld(p.enc + row + k * VW, VE()), d);
      vst(p.denc + row + k * VW, vscale(q, d));
    }
    acc = nnl_wave_sum(acc);
    if (lane == 0) {
      const float gv = acc + (p.dattn ? p.dattn[(long)t * ld + b] : 0.f);
      p.g[(long)b * p.T + t] = gv;
      s_qg[i] = q * gv;
    }
  }
  __syncthreads();
  if (tid == 0) {
    float c = 0.f;
    for (int i = 0; i < L; ++i) c += s_qg[i];
    p.cpart[(long)b * p.nch + chunk] = c;
  }
}

// launch 2: c[b] from launch 1's chunk partials (every workgroup of a column adds the same values in the same order),
// dlogit = q (g - c), dh[t,b,:] = dlogit w2; dw2 = sum dlogit h[t,b,:] and db2 = sum dlogit: workgroup partials, summed in
// chunk order by the column's last arriver, the columns in order by the last column
template <typename VA>
__global__ __launch_bounds__(kBlock) void attn_pool_bwd2_kernel(BwdArgs p) {
  __shared__ float s_dl[kMaxRows];
  __shared__ float4 s_part[kBlock];
  __shared__ float s_c;
  __shared__ int s_ticket;
  constexpr int VW = vwidth<VA>();
  const int tid = threadIdx.x;
  const int b = blockIdx.x / p.nch, chunk = blockIdx.x - b * p.nch;
  const int t0 = chunk * p.L, L = min(p.L, p.T - t0);
  const long ld = (long)p.B;
  const int A1 = p.A + 1;
  if (tid == 0) {
    float c = 0.f;
    for (int k = 0; k < p.nch; ++k) c += p.cpart[(long)b * p.nch + k];
    s_c = c;
  }
  __syncthreads();
  const float cb = s_c;
  for (int i = tid; i < L; i += kBlock) {
    const int t = t0 + i;
    s_dl[i] = p.attn[(long)t * ld + b] * (p.g[(long)b * p.T + t] - cb);
  }
  __syncthreads();
  const long slab = (long)b * p.nch + chunk;
  float* dwp = p.dwp + slab * A1;                 // A + 1 floats per slab: scalar stores
  const int nu = p.A / VW;
  const Cols cl(nu, tid);
  const long rs = ld * p.A;
  if (cl.gi < cl.G) {
    for (int j = cl.c; j < nu; j += cl.cpp) {
      const VA w = vld(p.w2 + j * VW, VA());
      VA a = from4(make_float4(0.f, 0.f, 0.f, 0.f), VA());
      const long base = ((long)t0 * ld + b) * p.A + j * VW;
      for (int i = cl.gi; i < L; i += cl.G) {
        const float dl = s_dl[i];
        a = vadd(a, vscale(dl, vld(p.h + base + i * rs, VA())));
        vst(p.dh + base + i * rs, vscale(dl, w));
      }
      if (cl.G == 1) {
        const float4 a4 = as4(a);
        dwp[j * VW] = a4.x;
        if (VW == 4) { dwp[j * VW + 1] = a4.y; dwp[j * VW + 2] = a4.z; dwp[j * VW + 3] = a4.w; }
      } else {
        s_part[tid] = as4(a);
      }
    }
  }
  if (cl.G > 1) {
    __syncthreads();
    if (tid < cl.cpp) {
      float4 w = s_part[tid];
      for (int k = 1; k < cl.G; ++k) {
        const float4 o = s_part[k * cl.cpp + tid];
        w.x += o.x; w.y += o.y; w.z += o.z; w.w += o.w;
      }
      dwp[tid * VW] = w.x;
      if (VW == 4) { dwp[tid * VW + 1] = w.y; dwp[tid * VW + 2] = w.z; dwp[tid * VW + 3] = w.w; }
    }
  }
  if (tid == 0) {
    float d = 0.f;
    for (int i = 0; i < L; ++i) d += s_dl[i];
    dwp[p.A] = d;
  }
  if (!arrive_last(p.counters + b, p.nch, &s_ticket)) return;
  const float* colin = p.dwp + (long)b * p.nch * A1;
  for (int j = tid; j < A1; j += kBlock) {
    float a = 0.f;
    for (int k = 0; k < p.nch; ++k) a += colin[(long)k * A1 + j];
    p.colp[(long)b * A1 + j] = a;
  }
  if (!arrive_last(p.counters + p.B, p.B, &s_ticket)) return;
  const float* colp = p.colp;
  for (int j = tid; j < A1; j += kBlock) {
    float a = 0.f;
    for (int k = 0; k < p.B; ++k) a += colp[(long)k * A1 + j];
    if (j < p.A) p.dw2[j] = a;
    else *p.db2 = a;
  }
}

bool aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }

int check_sizes(int64_t T, int64_t B, int64_t E, int64_t A, int32_t* counters, int64_t n_counters, void* workspace,
                size_t workspace_bytes, const char* who) {
  NNL_CHECK_ARG(T > 0 && B > 0 && E > 0 && A > 0, "%s: T, B, E, A must be >= 1 (got %lld, %lld, %lld, %lld)", who, (long long)T,
                (long long)B, (long long)E, (long long)A);
  NNL_CHECK_ARG(T < (1L << 30) && B < (1L << 30) && E < (1L << 30) && A < (1L << 30) && T * B < (1L << 40) &&
                    T * B * (E > A ? E : A) < (1L << 56),
                "%s: sizes too large", who);
  NNL_CHECK_ARG(B * plan(T, B).nch < (1L << 31), "%s: grid too large", who);
  NNL_CHECK_ARG(counters != nullptr && n_counters >= B + 1, "%s: needs B + 1 = %lld counters (got %lld)", who, (long long)(B + 1),
                (long long)n_counters);
  const size_t need = nnl_attn_pool_workspace_bytes(T, B, E, A);
  if (workspace == nullptr || workspace_bytes < need)
    return nnl_set_error(NNL_ERR_WORKSPACE, "%s: workspace too small (%zu < %zu bytes)", who, workspace_bytes, need);
  NNL_CHECK_ARG(aligned16(workspace), "%s: workspace must be 16-byte aligned", who);
  return NNL_OK;
}

}  // namespace

extern "C" size_t nnl_attn_pool_workspace_bytes(int64_t T, int64_t B, int64_t E, int64_t A) {
  if (T <= 0 || B <= 0 || E <= 0 || A <= 0 || T >= (1L << 30) || B >= (1L << 30) || E >= (1L << 30) || A >= (1L << 30)) return 0;
  const Layout l = layout(T, B, E, A);
  return (size_t)(l.fwd_end > l.bwd_end ? l.fwd_end : l.bwd_end) * sizeof(float);
}

extern "C" int nnl_attn_pool_fwd(const float* h, const float* w2, const float* b2, const float* enc_out, const int64_t* x,
                                 int64_t pad_token, float* attn, float* pooled, int64_t T, int64_t B, int64_t E, int64_t A,
                                 void* workspace, size_t workspace_bytes, int32_t* counters, int64_t n_counters, void* stream) {
  NNL_CHECK_ARG(h && w2 && b2 && enc_out && x && attn && pooled, "attn_pool_fwd: null pointer");
  if (int st = check_sizes(T, B, E, A, counters, n_counters, workspace, workspace_bytes, "attn_pool_fwd")) return st;
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_ELEMENTWISE, s, 2.0 * T * B * (E + A));
  const Plan pl = plan(T, B);
  const Layout l = layout(T, B, E, A);
  float* ws = (float*)workspace;
  FwdArgs a{h, w2, b2, enc_out, x, pad_token, attn, pooled, (int)T, (int)B, (int)E, (int)A, (int)pl.nch, (int)pl.L,
            ws + l.sc, ws + l.ms, ws + l.acc, counters};
  const bool ve = E % 4 == 0 && aligned16(enc_out), va = A % 4 == 0 && aligned16(h) && aligned16(w2);
  const dim3 grid((unsigned)(B * pl.nch));
  if (ve && va) hipLaunchKernelGGL((attn_pool_fwd_kernel<float4, float4>), grid, dim3(kBlock), 0, s, a);
  else if (ve) hipLaunchKernelGGL((attn_pool_fwd_kernel<float4, float>), grid, dim3(kBlock), 0, s, a);
  else if (va) hipLaunchKernelGGL((attn_pool_fwd_kernel<float, float4>), grid, dim3(kBlock), 0, s, a);
  else hipLaunchKernelGGL((attn_pool_fwd_kernel<float, float>), grid, dim3(kBlock), 0, s, a);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}

extern "C" int nnl_attn_pool_bwd(const float* h, const float* w2, const float* enc_out, const float* attn, const float* dpooled,
                                 const float* dattn, float* dh, float* denc, float* dw2, float* db2, int64_t T, int64_t B, int64_t E,
                                 int64_t A, void* workspace, size_t workspace_bytes, int32_t* counters, int64_t n_counters,
                                 void* stream) {
  NNL_CHECK_ARG(h && w2 && enc_out && attn && dpooled && dh && denc && dw2 && db2, "attn_pool_bwd: null pointer");
  if (int st = check_sizes(T, B, E, A, counters, n_counters, workspace, workspace_bytes, "attn_pool_bwd")) return st;
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_ELEMENTWISE, s, 2.0 * T * B * (2 * E + 2 * A));
  const Plan pl = plan(T, B);
  const Layout l = layout(T, B, E, A);
  float* ws = (float*)workspace;
  BwdArgs a{h, w2, enc_out, attn, dpooled, dattn, dh, denc, dw2, db2, (int)T, (int)B, (int)E, (int)A, (int)pl.nch, (int)pl.L,
            ws + l.g, ws + l.cpart, ws + l.dwp, ws + l.colp, counters};
  const bool ve = E % 4 == 0 && aligned16(enc_out) && aligned16(dpooled) && aligned16(denc);
  const bool va = A % 4 == 0 && aligned16(h) && aligned16(w2) && aligned16(dh);
  const dim3 grid((unsigned)(B * pl.nch));
  if (ve) hipLaunchKernelGGL((attn_pool_bwd1_kernel<float4>), grid, dim3(kBlock), 0, s, a);
  else hipLaunchKernelGGL((attn_pool_bwd1_kernel<float>), grid, dim3(kBlock), 0, s, a);
  NNL_CHECK_LAUNCH();
  if (va) hipLaunchKernelGGL((attn_pool_bwd2_kernel<float4>), grid, dim3(kBlock), 0, s, a);
  else hipLaunchKernelGGL((attn_pool_bwd2_kernel<float>), grid, dim3(kBlock), 0, s, a);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}
