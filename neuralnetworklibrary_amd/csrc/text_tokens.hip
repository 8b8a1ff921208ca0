// K17 — the tokeniser and vocabulary of the text workflow (Applications/Text.py:28-122: Tokenizer, tokenize_mp, numericalize) on one
// resident byte buffer.  The grammar is the package's own (Applications/Text.py's Tokenizer docstring): whether a
// token STARTS at byte i is a function of bytes i - 5 .. i + 4 of i's text (starts_at, text_grammar.h), so every byte decides for itself.  Only two
// things walk further, each from one thread and bounded by the end of the text: a token's length (to the next start, whitespace or the
// text's end) and the case rule's run (is the word run that begins here all upper case?).
//
// Token bounds are a scan: per-tile counts, an exclusive scan of the tile counts by ONE workgroup, and the in-tile scan with the
// carry applied (the launches of nnl_seg_event_gaps, tab_features.hip).  The vocabulary is an open-addressing table keyed by a 64-bit
// hash of the lowered bytes: one compare-and-swap per probe step, integer atomics only, no thread waits for a value another thread
// writes, every probe loop ends after `cap` steps.  A verify launch compares every token with the first token of its slot, so a hash
// collision is DETECTED (the caller rehashes with another seed) and the result is exact.  Phases are separate launches: what one
// phase wrote is visible to the next through the kernel boundary.
#include "nnl_common.h"
#include "text_grammar.h"

namespace {

using namespace nnl_text_grammar;

constexpr int kThreads = 256;
constexpr int kItems = 4;
constexpr int kTile = NNL_TEXT_TILE;
constexpr int kWaves = kThreads / NNL_WAVE;
static_assert(kThreads * kItems == kTile, "tile = threads x bytes per thread");

struct Corpus {
  const uint8_t* b;
  int64_t B;
  const int64_t* off;   // [n + 1]
  int64_t n;
  int mode;
};

// the text of byte i: the last j in [0, n) with off[j] <= i (empty texts before it are skipped); bounds clamped into the buffer
__device__ __forceinline__ int64_t text_of(const Corpus& c, int64_t i) {
  int64_t lo = 0, hi = c.n - 1;
  while (lo < hi) {                                       // at most 63 steps
    const int64_t mid = lo + (hi - lo + 1) / 2;
    if (c.off[mid] <= i) lo = mid; else hi = mid - 1;
  }
  return lo;
}
__device__ __forceinline__ TextView view_of(const Corpus& c, int64_t j) {
  const int64_t a = c.off[j], e = c.off[j + 1];
  return TextView{c.b, min(max(a, (int64_t)0), c.B), min(max(e, (int64_t)0), c.B)};
}

// this thread's kItems bytes: cnt[k] tokens start at byte i0 + k; views[k] is that byte's text
__device__ __forceinline__ void load_counts(const Corpus& c, int64_t i0, int* cnt, TextView* views) {
#pragma unroll
  for (int k = 0; k < kItems; ++k) cnt[k] = 0;
  if (i0 >= c.B) return;
  int64_t j = text_of(c, i0);
  TextView v = view_of(c, j);
#pragma unroll
  for (int k = 0; k < kItems; ++k) {
    const int64_t i = i0 + k;
    views[k] = v;
    if (i >= c.B) continue;
    while (i >= v.t1 && j + 1 < c.n) v = view_of(c, ++j);   // bounded by n
    views[k] = v;
    cnt[k] = starts_at(v, i, c.mode);
  }
}

__global__ __launch_bounds__(kThreads) void text_count_kernel(Corpus c, int64_t* __restrict__ tile_base) {
  __shared__ int lds[kWaves];
  int cnt[kItems];
  TextView views[kItems];
  load_counts(c, (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kItems, cnt, views);
  int s = 0;
#pragma unroll
  for (int k = 0; k < kItems; ++k) s += cnt[k];
  s = nnl_block_reduce<kWaves>(s, NnlSum(), lds);
  if (threadIdx.x == 0) tile_base[blockIdx.x] = s;
}

// ONE workgroup: tile counts -> the count of all EARLIER tiles, in place; tile_base[ntiles] = the total
__global__ __launch_bounds__(kThreads) void text_carry_kernel(int64_t* __restrict__ tile_base, int64_t ntiles) {
  __shared__ long long lds[kWaves];
  long long run = 0;
  for (int64_t c0 = 0; c0 < ntiles; c0 += kThreads) {
    const int64_t tile = c0 + threadIdx.x;
    long long v = tile < ntiles ? (long long)tile_base[tile] : 0, total;
    const long long e = nnl_block_scan_exclusive<kWaves>(v, NnlSum(), (long long)0, lds, total);
    if (tile < ntiles) tile_base[tile] = run + e;
    run += total;
  }
  if (threadIdx.x == 0) tile_base[ntiles] = run;
}

__global__ __launch_bounds__(kThreads) void text_fill_kernel(Corpus c, const int64_t* __restrict__ tile_base, int64_t T,
                                                             int32_t* __restrict__ tok_start, int32_t* __restrict__ tok_len) {
  __shared__ int lds[kWaves];
  const int64_t i0 = (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kItems;
  int cnt[kItems];
  TextView views[kItems];
  load_counts(c, i0, cnt, views);
  int s = 0, total;
#pragma unroll
  for (int k = 0; k < kItems; ++k) s += cnt[k];
  const int e = nnl_block_scan_exclusive<kWaves>(s, NnlSum(), 0, lds, total);
  int64_t rank = tile_base[blockIdx.x] + e;
#pragma unroll
  for (int k = 0; k < kItems; ++k) {
    if (cnt[k] == 0) continue;
    const int64_t i = i0 + k;
    if (cnt[k] == 2) {
      if (rank >= 0 && rank < T) { tok_start[rank] = (int32_t)i; tok_len[rank] = NNL_TEXT_TUP_LEN; }
      ++rank;
    }
    if (rank >= 0 && rank < T) { tok_start[rank] = (int32_t)i; tok_len[rank] = token_length(views[k], i, c.mode); }
    ++rank;
  }
}

// text j owns the tokens whose start lies in [off[j], off[j+1]): text_tok_off[j] = the number of tokens that start before off[j]
__global__ __launch_bounds__(kThreads) void text_tok_off_kernel(Corpus c, const int32_t* __restrict__ tok_start, int64_t T,
                                                                int64_t* __restrict__ text_tok_off) {
  const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (j > c.n) return;
  int64_t lo = 0, hi = T;                                   // first t with tok_start[t] >= off[j]
  if (j == c.n) lo = T;
  const int64_t target = c.off[j];
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if ((int64_t)tok_start[mid] < target) lo = mid + 1; else hi = mid;
  }
  text_tok_off[j] = lo;
}

// ---- tokens as byte strings ------------------------------------------------------------------------------------------------------------
struct TokStream {
  const uint8_t* b;
  int64_t B;
  const int32_t* start;
  const int32_t* len;
  int lower;            // 1: A-Z read as a-z (the grammar mode)
};
struct Tok { int64_t s; int len; bool tup; };

__device__ __forceinline__ Tok tok_of(const TokStream& ts, int64_t t) {
  const int l = ts.len[t];
  const int64_t s = ts.start[t];
  if (l == NNL_TEXT_TUP_LEN) return Tok{0, 4, true};
  if (l < 0 || s < 0 || s + l > ts.B) return Tok{0, 0, false};     // a record outside the buffer reads as an empty token
  return Tok{s, l, false};
}
__device__ __forceinline__ int tok_byte(const TokStream& ts, const Tok& k, int p) {
  if (k.tup) return p == 0 ? 't' : p == 1 ? '_' : p == 2 ? 'u' : 'p';
  const int c = ts.b[k.s + p];
  return ts.lower ? to_lower(c) : c;
}
__device__ bool tok_equal(const TokStream& A, const Tok& a, const TokStream& Bs, const Tok& b) {
  if (a.len != b.len) return false;
  for (int p = 0; p < a.len; ++p)
    if (tok_byte(A, a, p) != tok_byte(Bs, b, p)) return false;
  return true;
}

__global__ __launch_bounds__(kThreads) void text_hash_kernel(TokStream ts, int64_t T, uint64_t seed, uint64_t mask,
                                                             uint64_t* __restrict__ keys) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= T) return;
  const Tok k = tok_of(ts, t);
  uint64_t h = 0xcbf29ce484222325ull ^ (seed * 0x9E3779B97F4A7C15ull);      // FNV-1a over the bytes, then a 64-bit finaliser
  for (int p = 0; p < k.len; ++p) {
    h ^= (uint64_t)tok_byte(ts, k, p);
    h *= 0x100000001b3ull;
  }
  h ^= (uint64_t)k.len;
  h ^= h >> 33; h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull;
  h ^= h >> 33;
  h &= mask;
  keys[t] = h ? h : (mask & (~mask + 1));                    // 0 is the empty slot
}

// ---- the table ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t home_slot(uint64_t key, int log2cap) { return (int64_t)((key * 0x9E3779B97F4A7C15ull) >> (64 - log2cap)); }

__global__ __launch_bounds__(kThreads) void vocab_reset_kernel(uint64_t* __restrict__ table_key, int32_t* __restrict__ table_count,
                                                               int32_t* __restrict__ table_first, int64_t cap, int32_t* __restrict__ status) {
  const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (s == 0) *status = 0;
  if (s >= cap) return;
  table_key[s] = 0;
  table_count[s] = 0;
  table_first[s] = 0x7fffffff;
}

__global__ __launch_bounds__(kThreads) void vocab_insert_kernel(const uint64_t* __restrict__ keys, int64_t T, uint64_t* table_key,
                                                                int32_t* table_count, int32_t* table_first, int64_t cap, int log2cap,
                                                                int32_t* __restrict__ tok_slot, int32_t* status) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= T) return;
  const uint64_t key = keys[t];
  int64_t s = home_slot(key, log2cap);
  int32_t found = -1;
  for (int64_t step = 0; step < cap; ++step) {              // bounded by the capacity, not by what other threads do
    const unsigned long long old = atomicCAS(reinterpret_cast<unsigned long long*>(table_key + s), 0ull, (unsigned long long)key);
    if (old == 0ull || old == key) { found = (int32_t)s; break; }
    s = (s + 1) & (cap - 1);
  }
  tok_slot[t] = found;
  if (found < 0) { atomicOr(status, NNL_TEXT_STATUS_OVERFLOW); return; }
  atomicAdd(table_count + found, 1);
  atomicMin(table_first + found, (int32_t)t);
}

__global__ __launch_bounds__(kThreads) void vocab_verify_kernel(TokStream ts, const int32_t* __restrict__ tok_slot, int64_t T, TokStream fs,
                                                                int64_t FT, const int32_t* __restrict__ table_first, int64_t cap,
                                                                int32_t* mismatches) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= T) return;
  const int32_t s = tok_slot[t];
  if (s < 0 || s >= cap) return;                            // no slot: the overflow bit already says so
  const int32_t f = table_first[s];
  bool same = false;
  if (f >= 0 && f < FT) same = tok_equal(ts, tok_of(ts, t), fs, tok_of(fs, f));
  if (!same) atomicAdd(mismatches, 1);                      // the compiler folds a wave's adds into one
}

__global__ __launch_bounds__(kThreads) void vocab_compact_kernel(const uint64_t* __restrict__ table_key, const int32_t* __restrict__ table_count,
                                                                 const int32_t* __restrict__ table_first, int64_t cap,
                                                                 const int32_t* __restrict__ tok_start, const int32_t* __restrict__ tok_len,
                                                                 int64_t T, int32_t* __restrict__ list, int64_t max_rows, int32_t* n_rows) {
  const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (s >= cap || table_key[s] == 0) return;
  const int64_t row = atomicAdd(n_rows, 1);
  if (row >= max_rows) return;
  const int32_t f = table_first[s];
  const bool ok = f >= 0 && f < T;
  int32_t* r = list + row * 5;
  r[0] = (int32_t)s;
  r[1] = table_count[s];
  r[2] = f;
  r[3] = ok ? tok_start[f] : 0;
  r[4] = ok ? tok_len[f] : 0;
}

__global__ __launch_bounds__(kThreads) void vocab_zero_ids_kernel(int32_t* __restrict__ slot_id, int64_t cap) {
  const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (s < cap) slot_id[s] = 0;
}
__global__ __launch_bounds__(kThreads) void vocab_assign_kernel(const int32_t* __restrict__ slots, const int32_t* __restrict__ ids, int64_t K,
                                                                int32_t* __restrict__ slot_id, int64_t cap) {
  const int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (k >= K) return;
  const int32_t s = slots[k];
  if (s >= 0 && s < cap) slot_id[s] = ids[k];
}

__global__ __launch_bounds__(kThreads) void vocab_lookup_kernel(TokStream ts, const uint64_t* __restrict__ keys, int64_t T, TokStream vs,
                                                                int64_t VT, const uint64_t* __restrict__ table_key,
                                                                const int32_t* __restrict__ table_first, int64_t cap, int log2cap,
                                                                int32_t* __restrict__ tok_slot) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= T) return;
  const uint64_t key = keys[t];
  int64_t s = home_slot(key, log2cap);
  int32_t found = -1;
  for (int64_t step = 0; step < cap; ++step) {
    const uint64_t k = table_key[s];
    if (k == 0) break;                                     // an empty slot ends every probe sequence: the token is not in the vocabulary
    if (k == key) {                                        // the only slot that can hold it: equal bytes or absent
      const int32_t f = table_first[s];
      if (f >= 0 && f < VT && tok_equal(ts, tok_of(ts, t), vs, tok_of(vs, f))) found = (int32_t)s;
      break;
    }
    s = (s + 1) & (cap - 1);
  }
  tok_slot[t] = found;
}

__global__ __launch_bounds__(kThreads) void text_ids_kernel(const int32_t* __restrict__ tok_slot, const int32_t* __restrict__ slot_id,
                                                            int64_t cap, const int64_t* __restrict__ text_tok_off, int64_t n, int64_t T,
                                                            int reverse, int64_t* __restrict__ ids) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= T) return;
  const int32_t s = tok_slot[t];
  const int64_t id = (s >= 0 && s < cap) ? (int64_t)slot_id[s] : 0;
  int64_t p = t;
  if (reverse) {
    int64_t lo = 0, hi = n - 1;                             // the last j with text_tok_off[j] <= t
    while (lo < hi) {
      const int64_t mid = lo + (hi - lo + 1) / 2;
      if (text_tok_off[mid] <= t) lo = mid; else hi = mid - 1;
    }
    p = text_tok_off[lo] + (text_tok_off[lo + 1] - 1 - t);
  }
  if (p >= 0 && p < T) ids[p] = id;
}

constexpr int64_t kMaxBytes = ((int64_t)1 << 31) - 1;
inline bool mode_ok(int mode) { return mode == NNL_TEXT_MODE_GRAMMAR || mode == NNL_TEXT_MODE_SPLIT; }
inline int log2_of_cap(int64_t cap) {      // -1 unless cap is a power of two in [16, 2^30]
  if (cap < 16 || cap > ((int64_t)1 << 30) || (cap & (cap - 1))) return -1;
  return __builtin_ctzll((unsigned long long)cap);
}
inline unsigned grid_of(int64_t items) { return (unsigned)nnl_cdiv(items, kThreads); }

}  // namespace

extern "C" int nnl_text_token_count(const uint8_t* bytes, int64_t B, const int64_t* text_off, int64_t n, int mode, int64_t* tile_base,
                                    void* stream) {
  NNL_CHECK_ARG(B >= 0 && B <= kMaxBytes, "text_token_count: B must lie in [0, 2^31) (got %lld)", (long long)B);
  NNL_CHECK_ARG(n >= 1 && n <= kMaxBytes, "text_token_count: n must lie in [1, 2^31) (got %lld)", (long long)n);
  NNL_CHECK_ARG(mode_ok(mode), "text_token_count: mode must be NNL_TEXT_MODE_GRAMMAR or NNL_TEXT_MODE_SPLIT (got %d)", mode);
  NNL_CHECK_ARG(bytes && text_off && tile_base, "text_token_count: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const Corpus c{bytes, B, text_off, n, mode};
  const int64_t ntiles = nnl_cdiv(B, kTile);
  NnlProfScope prof(NNL_PROF_ELEMENTWISE, s, (double)B + 16.0 * (double)ntiles);
  NNL_ROUTE("text_token_count:tiles@%lld", (long long)ntiles);
  if (ntiles > 0) {
    hipLaunchKernelGGL(text_count_kernel, dim3((unsigned)ntiles), dim3(kThreads), 0, s, c, tile_base);
    NNL_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(text_carry_kernel, dim3(1), dim3(kThreads), 0, s, tile_base, ntiles);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}

extern "C" int nnl_text_token_fill(const uint8_t* bytes, int64_t B, const int64_t* text_off, int64_t n, int mode, const int64_t* tile_base,
                                   int64_t T, int32_t* tok_start, int32_t* tok_len, int64_t* text_tok_off, void* stream) {
  NNL_CHECK_ARG(B >= 0 && B <= kMaxBytes, "text_token_fill: B must lie in [0, 2^31) (got %lld)", (long long)B);
  NNL_CHECK_ARG(n >= 1 && n <= kMaxBytes, "text_token_fill: n must lie in [1, 2^31) (got %lld)", (long long)n);
  NNL_CHECK_ARG(T >= 0 && T <= kMaxBytes, "text_token_fill: T must lie in [0, 2^31) (got %lld)", (long long)T);
  NNL_CHECK_ARG(mode_ok(mode), "text_token_fill: mode must be NNL_TEXT_MODE_GRAMMAR or NNL_TEXT_MODE_SPLIT (got %d)", mode);
  NNL_CHECK_ARG(bytes && text_off && tile_base && tok_start && tok_len && text_tok_off, "text_token_fill: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const Corpus c{bytes, B, text_off, n, mode};
  const int64_t ntiles = nnl_cdiv(B, kTile);
  NnlProfScope prof(NNL_PROF_ELEMENTWISE, s, (double)B + 8.0 * (double)T + 16.0 * (double)n);
  NNL_ROUTE("text_token_fill:tiles@%lld", (long long)ntiles);
  if (ntiles > 0 && T > 0) {
    hipLaunchKernelGGL(text_fill_kernel, dim3((unsigned)ntiles), dim3(kThreads), 0, s, c, tile_base, T, tok_start, tok_len);
    NNL_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(text_tok_off_kernel, dim3(grid_of(n + 1)), dim3(kThreads), 0, s, c, tok_start, T, text_tok_off);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}

extern "C" int nnl_text_token_hash(const uint8_t* bytes, int64_t B, const int32_t* tok_start, const int32_t* tok_len, int64_t T, int mode,
                                   uint64_t seed, uint64_t hash_mask, uint64_t* keys, void* stream) {
  NNL_CHECK_ARG(B >= 0 && B <= kMaxBytes, "text_token_hash: B must lie in [0, 2^31) (got %lld)", (long long)B);
  NNL_CHECK_ARG(T >= 0 && T <= kMaxBytes, "text_token_hash: T must lie in [0, 2^31) (got %lld)", (long long)T);
  NNL_CHECK_ARG(mode_ok(mode), "text_token_hash: mode must be NNL_TEXT_MODE_GRAMMAR or NNL_TEXT_MODE_SPLIT (got %d)", mode);
  NNL_CHECK_ARG(hash_mask != 0, "text_token_hash: hash_mask must not be 0");
  NNL_CHECK_ARG(bytes && tok_start && tok_len && keys, "text_token_hash: null pointer");
  if (T == 0) return NNL_OK;
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_ELEMENTWISE, s, (double)B + 16.0 * (double)T);
  const TokStream ts{bytes, B, tok_start, tok_len, mode == NNL_TEXT_MODE_GRAMMAR};
  hipLaunchKernelGGL(text_hash_kernel, dim3(grid_of(T)), dim3(kThreads), 0, s, ts, T, seed, hash_mask, keys);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}

extern "C" int nnl_text_vocab_insert(const uint64_t* keys, int64_t T, uint64_t* table_key, int32_t* table_count, int32_t* table_first,
                                     int64_t cap, int reset, int32_t* tok_slot, int32_t* status, void* stream) {
  NNL_CHECK_ARG(T >= 0 && T <= kMaxBytes, "text_vocab_insert: T must lie in [0, 2^31) (got %lld)", (long long)T);
  const int log2cap = log2_of_cap(cap);
  NNL_CHECK_ARG(log2cap > 0, "text_vocab_insert: cap must be a power of two in [16, 2^30] (got %lld)", (long long)cap);
  NNL_CHECK_ARG(keys && table_key && table_count && table_first && tok_slot && status, "text_vocab_insert: null pointer");
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_ELEMENTWISE, s, 28.0 * (double)T + (reset ? 16.0 * (double)cap : 0.0));
  if (reset) {
    hipLaunchKernelGGL(vocab_reset_kernel, dim3(grid_of(cap)), dim3(kThreads), 0, s, table_key, table_count, table_first, cap, status);
    NNL_CHECK_LAUNCH();
  }
  if (T == 0) return NNL_OK;
  hipLaunchKernelGGL(vocab_insert_kernel, dim3(grid_of(T)), dim3(kThreads), 0, s, keys, T, table_key, table_count, table_first, cap, log2cap,
                     tok_slot, status);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}

extern "C" int nnl_text_vocab_verify(const uint8_t* bytes, int64_t B, const int32_t* tok_start, const int32_t* tok_len, const int32_t* tok_slot,
                                     int64_t T, int mode, const uint8_t* fbytes, int64_t FB, const int32_t* ftok_start,
                                     const int32_t* ftok_len, int64_t FT, int fmode, const int32_t* table_first, int64_t cap,
                                     int32_t* mismatches, void* stream) {
  NNL_CHECK_ARG(B >= 0 && B <= kMaxBytes && FB >= 0 && FB <= kMaxBytes, "text_vocab_verify: B and FB must lie in [0, 2^31) (got %lld, %lld)",
                (long long)B, (long long)FB);
  NNL_CHECK_ARG(T >= 0 && T <= kMaxBytes && FT >= 0 && FT <= kMaxBytes, "text_vocab_verify: T and FT must lie in [0, 2^31) (got %lld, %lld)",
                (long long)T, (long long)FT);
  NNL_CHECK_ARG(mode_ok(mode) && mode_ok(fmode), "text_vocab_verify: modes must be NNL_TEXT_MODE_GRAMMAR or NNL_TEXT_MODE_SPLIT (got %d, %d)",
                mode, fmode);
  NNL_CHECK_ARG(log2_of_cap(cap) > 0, "text_vocab_verify: cap must be a power of two in [16, 2^30] (got %lld)", (long long)cap);
  NNL_CHECK_ARG(bytes && tok_start && tok_len && tok_slot && fbytes && ftok_start && ftok_len && table_first && mismatches,
                "text_vocab_verify: null pointer");
  if (T == 0) return NNL_OK;
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_ELEMENTWISE, s, 2.0 * (double)B + 24.0 * (double)T);
  const TokStream ts{bytes, B, tok_start, tok_len, mode == NNL_TEXT_MODE_GRAMMAR};
  const TokStream fs{fbytes, FB, ftok_start, ftok_len, fmode == NNL_TEXT_MODE_GRAMMAR};
  hipLaunchKernelGGL(vocab_verify_kernel, dim3(grid_of(T)), dim3(kThreads), 0, s, ts, tok_slot, T, fs, FT, table_first, cap, mismatches);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}

extern "C" int nnl_text_vocab_compact(const uint64_t* table_key, const int32_t* table_count, const int32_t* table_first, int64_t cap,
                                      const int32_t* tok_start, const int32_t* tok_len, int64_t T, int32_t* list, int64_t max_rows,
                                      int32_t* n_rows, void* stream) {
  NNL_CHECK_ARG(log2_of_cap(cap) > 0, "text_vocab_compact: cap must be a power of two in [16, 2^30] (got %lld)", (long long)cap);
  NNL_CHECK_ARG(T >= 0 && T <= kMaxBytes, "text_vocab_compact: T must lie in [0, 2^31) (got %lld)", (long long)T);
  NNL_CHECK_ARG(max_rows >= 1 && max_rows <= kMaxBytes / 5, "text_vocab_compact: max_rows must lie in [1, 2^31 / 5) (got %lld)",
                (long long)max_rows);
  NNL_CHECK_ARG(table_key && table_count && table_first && tok_start && tok_len && list && n_rows, "text_vocab_compact: null pointer");
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_ELEMENTWISE, s, 8.0 * (double)cap);
  hipLaunchKernelGGL(vocab_compact_kernel, dim3(grid_of(cap)), dim3(kThreads), 0, s, table_key, table_count, table_first, cap, tok_start,
                     tok_len, T, list, max_rows, n_rows);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}

extern "C" int nnl_text_vocab_assign(const int32_t* slots, const int32_t* ids, int64_t K, int32_t* slot_id, int64_t cap, void* stream) {
  NNL_CHECK_ARG(log2_of_cap(cap) > 0, "text_vocab_assign: cap must be a power of two in [16, 2^30] (got %lld)", (long long)cap);
  NNL_CHECK_ARG(K >= 0 && K <= cap, "text_vocab_assign: K must lie in [0, cap] (got %lld)", (long long)K);
  NNL_CHECK_ARG(slots && ids && slot_id, "text_vocab_assign: null pointer");
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_ELEMENTWISE, s, 4.0 * (double)cap + 12.0 * (double)K);
  hipLaunchKernelGGL(vocab_zero_ids_kernel, dim3(grid_of(cap)), dim3(kThreads), 0, s, slot_id, cap);
  NNL_CHECK_LAUNCH();
  if (K == 0) return NNL_OK;
  hipLaunchKernelGGL(vocab_assign_kernel, dim3(grid_of(K)), dim3(kThreads), 0, s, slots, ids, K, slot_id, cap);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}

extern "C" int nnl_text_vocab_lookup(const uint8_t* bytes, int64_t B, const int32_t* tok_start, const int32_t* tok_len, const uint64_t* keys,
                                     int64_t T, int mode, const uint8_t* vbytes, int64_t VB, const int32_t* vtok_start, const int32_t* vtok_len,
                                     int64_t VT, const uint64_t* table_key, const int32_t* table_first, int64_t cap, int32_t* tok_slot,
                                     void* stream) {
  NNL_CHECK_ARG(B >= 0 && B <= kMaxBytes && VB >= 0 && VB <= kMaxBytes, "text_vocab_lookup: B and VB must lie in [0, 2^31) (got %lld, %lld)",
                (long long)B, (long long)VB);
  NNL_CHECK_ARG(T >= 0 && T <= kMaxBytes && VT >= 0 && VT <= kMaxBytes, "text_vocab_lookup: T and VT must lie in [0, 2^31) (got %lld, %lld)",
                (long long)T, (long long)VT);
  NNL_CHECK_ARG(mode_ok(mode), "text_vocab_lookup: mode must be NNL_TEXT_MODE_GRAMMAR or NNL_TEXT_MODE_SPLIT (got %d)", mode);
  const int log2cap = log2_of_cap(cap);
  NNL_CHECK_ARG(log2cap > 0, "text_vocab_lookup: cap must be a power of two in [16, 2^30] (got %lld)", (long long)cap);
  NNL_CHECK_ARG(bytes && tok_start && tok_len && keys && vbytes && vtok_start && vtok_len && table_key && table_first && tok_slot,
                "text_vocab_lookup: null pointer");
  if (T == 0) return NNL_OK;
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_ELEMENTWISE, s, (double)B + 32.0 * (double)T);
  const TokStream ts{bytes, B, tok_start, tok_len, mode == NNL_TEXT_MODE_GRAMMAR};
  const TokStream vs{vbytes, VB, vtok_start, vtok_len, 0};       // the vocabulary's strings are compared as they are
  hipLaunchKernelGGL(vocab_lookup_kernel, dim3(grid_of(T)), dim3(kThreads), 0, s, ts, keys, T, vs, VT, table_key, table_first, cap, log2cap,
                     tok_slot);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}

extern "C" int nnl_text_ids_write(const int32_t* tok_slot, const int32_t* slot_id, int64_t cap, const int64_t* text_tok_off, int64_t n,
                                  int64_t T, int reverse, int64_t* ids, void* stream) {
  NNL_CHECK_ARG(log2_of_cap(cap) > 0, "text_ids_write: cap must be a power of two in [16, 2^30] (got %lld)", (long long)cap);
  NNL_CHECK_ARG(n >= 1 && n <= kMaxBytes, "text_ids_write: n must lie in [1, 2^31) (got %lld)", (long long)n);
  NNL_CHECK_ARG(T >= 0 && T <= kMaxBytes, "text_ids_write: T must lie in [0, 2^31) (got %lld)", (long long)T);
  NNL_CHECK_ARG(tok_slot && slot_id && text_tok_off && ids, "text_ids_write: null pointer");
  if (T == 0) return NNL_OK;
  hipStream_t s = (hipStream_t)stream;
  NnlProfScope prof(NNL_PROF_ELEMENTWISE, s, 16.0 * (double)T);
  hipLaunchKernelGGL(text_ids_kernel, dim3(grid_of(T)), dim3(kThreads), 0, s, tok_slot, slot_id, cap, text_tok_off, n, T, reverse ? 1 : 0, ids);
  NNL_CHECK_LAUNCH();
  return NNL_OK;
}
