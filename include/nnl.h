/*
 * nnl.h — C ABI of libnnl_hip.so: the MI355X (gfx950) kernels behind the Learner.fit() hot path.
 *
 * The reference (NickTravers/NeuralNetworkLibrary) has NO FFI / plugin registry: every FLOP is an
 * eager torch op called from its nn.Modules.  The drop-in boundary is therefore
 * the set of torch call sites on the hot path; each entry point below names the reference call site
 * (file:line, relative to the reference root) whose arithmetic it replaces.  The Python host side
 * (neuralnetworklibrary_amd/ops.py) binds these with ctypes and calls them from
 * torch.autograd.Function.forward/backward — see INTEGRATION.md for the reference-side stub.
 *
 * Conventions
 *  - plain pointers + sizes, no torch types.  All pointers are DEVICE pointers unless stated.
 *  - every call is asynchronous on `stream` (a hipStream_t passed as void*); no implicit device sync.
 *  - the library never allocates/frees device memory and keeps no pointer past return; workspaces are
 *    caller-owned, sized by the matching *_workspace_bytes().
 *  - return 0 on success, negative nnl_status_t on failure; nnl_last_error() gives the text
 *    (thread-local).  No C++ exception crosses the ABI.
 *  - fp32 everywhere (the reference is fp32, README.md:19-24); indices are int64 (torch LongTensor).
 *  - activations are NHWC ("channels_last" physical layout of a logical NCHW torch tensor);
 *    conv filters are KRSC (= channels_last physical layout of a logical [K,C,R,S] parameter).
 */
#ifndef NNL_H_
#define NNL_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  NNL_OK = 0,
  NNL_ERR_INVALID_ARG = -1,
  NNL_ERR_HIP = -2,
  NNL_ERR_UNSUPPORTED = -3,
  NNL_ERR_WORKSPACE = -4
} nnl_status_t;

int nnl_version(void);
const char* nnl_last_error(void);
/* The NNL_* tuning / A-B environment switches are read once per call site; this makes every site read its variable again
 * (tests and the A/B tools change a switch inside one process). */
int nnl_reload_env(void);

/* ---- profiling hooks (bench.py roofline leg): HIP events recorded on the launch stream --------- */
enum { NNL_PROF_CONV_FWD = 0, NNL_PROF_CONV_DGRAD = 1, NNL_PROF_CONV_WGRAD = 2, NNL_PROF_EMBDOT = 3,
       NNL_PROF_TABULAR = 4, NNL_PROF_RETINA_LOSS = 5, NNL_PROF_LSTM = 6, NNL_PROF_SOFTMAX_CE = 7,
       NNL_PROF_ELEMENTWISE = 8, NNL_PROF_GEMM = 9, NNL_PROF_OPTIM = 10, NNL_PROF_KINDS = 11 };
/* enable!=0 starts recording (bounded event pool); 0 stops. */
int nnl_prof_enable(int enable);
/* Synchronises the recorded events and returns, per kind: launches, total ms, total algorithmic work
 * (flops or bytes as documented per op).  Arrays have NNL_PROF_KINDS entries. Resets the pool. */
int nnl_prof_collect(int64_t* launches, double* total_ms, double* total_work);
/* The same plus, per kind, the EXECUTED work: algorithmic work x (multiplies issued / algorithmic multiplies) of each launch — 1 for the direct
 * kernels, 1 / 1.5 for the 1-D Winograd kernels (forward, dgrad, Winograd-domain wgrad), 1 / 2.25 for the 2-D ones.  total_exec may be NULL. */
int nnl_prof_collect2(int64_t* launches, double* total_ms, double* total_work, double* total_exec);
/* Data-parallel overlap under hipGraph replay (host side: neuralnetworklibrary_amd/dist.py, GradSync.reduce_overlapped; replaces nothing in the
 * single-GPU reference — SURVEY.md 8e).  A captured training step contains nnl_dp_bump(step) at its start and nnl_dp_signal(flag + k, step)
 * right after the last gradient of all-reduce bucket k; after each replay the host enqueues, on a side stream, nnl_dp_wait(flag + k, n, ...)
 * (n = number of replays so far) followed by bucket k's RCCL all-reduce, which therefore starts while the rest of the replayed backward
 * still runs.  The wait kernel is one lane polling with s_sleep, bounded in WALL TIME by timeout_us (the device's constant-rate counter; then
 * *err = 1 and it returns: the stream always drains; the host reads *err with the step's loss and raises). */
int nnl_dp_bump(int32_t* step, void* stream);
int nnl_dp_signal(int32_t* flag, const int32_t* step, void* stream);
int nnl_dp_wait(const int32_t* flag, int32_t value, int64_t timeout_us, int32_t* err, void* stream);
/* First 16 hex digits of the sha256 over the library's sources (csrc/ *.hip, *.h, Makefile, include/nnl.h; csrc/Makefile) it was built from. */
const char* nnl_source_stamp(void);

/* ---- K4: EmbeddingDotBias (CollabFilterNet.forward, Applications/CollabFiltering.py:196-204) ----
 * y_b = lo + (hi-lo)*sigmoid( sum_d U[x[b,0],d]*M[x[b,1],d] + bu[x[b,0]] + bi[x[b,1]] )   (has_range!=0)
 * y_b =                         sum_d ...                + bu + bi                       (has_range==0)
 * x: int64 [n,2]; U [n_user,D]; M [n_item,D]; bu [n_user]; bi [n_item]; y [n]; z [n] (pre-activation,
 * saved for backward; may be NULL).  Out-of-range indices are reported through *err_flag (device int32,
 * may be NULL; set to 1) and the sample is skipped — torch raises IndexError at the same place. */
int nnl_embdotbias_fwd(const int64_t* x, const float* U, const float* M, const float* bu, const float* bi,
                       float* y, float* z, int64_t n, int64_t n_user, int64_t n_item, int64_t D,
                       int has_range, float lo, float hi, int32_t* err_flag, void* stream);
/* Backward of the above = the four dense embedding_backward scatter-adds + sigmoid/mul backward
 * (autograd of CollabFiltering.py:198-203).  dU/dM/dbu/dbi are DENSE tables (nn.Embedding sparse=False,
 * General/Layers.py:59) which this call first zero-fills, then scatter-adds into. */
/* Deterministic by default: with a workspace of nnl_*_bwd_workspace_bytes the samples that hit one table row are added in
 * SAMPLE ORDER (rank sort + segment sum, csrc/scatter_det.h) — torch's CPU embedding_dense_backward order, bitwise reproducible.
 * workspace == NULL (or NNL_SCATTER_ATOMIC=1, or more than 32768 samples): fp32 atomicAdd in arrival order. */
size_t nnl_embdotbias_bwd_workspace_bytes(int64_t n);
int nnl_embdotbias_bwd(const int64_t* x, const float* U, const float* M, const float* z, const float* dy,
                       float* dU, float* dM, float* dbu, float* dbi, int64_t n, int64_t n_user,
                       int64_t n_item, int64_t D, int has_range, float lo, float hi, void* workspace, size_t workspace_bytes, void* stream);

/* ---- K1: conv2d as implicit GEMM on the exact-fp32 MFMA --------------------------------------------
 * Replaces the cuDNN convolutions called by nn.Conv2d inside BasicBlock.forward / Bottleneck.forward
 * (Applications/VisionModels/retinanet.py:43-59, 77-97), the stem (:304), the 1x1 downsample (:344-348),
 * PyramidFeatures (:126-148) and the RetinaNet heads (:187-217, :260-295), and their autograd backward.
 * x [N,H,W,C] NHWC, w [K,R,S,C] KRSC, y [N,P,Q,K] NHWC; P = floor((H+2*pad-R)/stride)+1 with H+2*pad >= R (validated). C%4==0
 * (the host pads the 3-channel stem input to 4), K%4==0 for dgrad/wgrad.  fp32 in, fp32 accumulate:
 * results equal a k-ordered fmaf chain (MI355X_MICROARCH.md, Matrix cores). */
typedef struct {
  int32_t N, H, W, C;   /* input  NHWC */
  int32_t K, R, S;      /* filter KRSC */
  int32_t stride, pad;  /* same in both spatial dims (all reference convs are symmetric) */
  int32_t P, Q;         /* output spatial size */
} nnl_conv_geom_t;

/* y = act(conv(x, w) (+ bias[K])); `relu` selects the output activation: 0 none, 1 ReLU, 2 sigmoid (ClassificationModel's
 * `output_act`, reference retinanet.py:286; needs C % 16 == 0).  bias may be NULL.
 * workspace (optional, nnl_conv2d_fwd_workspace_bytes(g); NULL = none): lets the launch use the balanced schedule —
 * when the tile grid is not a multiple of the 256 CUs, the last tiles (or all of them) are cut into k slices whose
 * partial slabs are summed in a fixed order (bitwise reproducible run to run). */
size_t nnl_conv2d_fwd_workspace_bytes(const nnl_conv_geom_t* g);
/* tile_counters (optional): a PERSISTENT device array of nnl_conv2d_tile_counters() int32, zero-initialised once by the
 * caller and never touched otherwise (one per device and stream).  With it the last k slice of a split tile to finish sums
 * the slabs in slice order and writes the output inside the conv kernel (no separate reduce launch); each counter returns
 * to zero before the kernel ends.  NULL: the slabs are reduced by a second launch. */
int64_t nnl_conv2d_tile_counters(void);
/* BatchNorm statistics in the epilogue (optional; all three of bn_partials / bn_pivot / bn_rows or none): when the launch uses
 * the 64x64 tile, the workgroup that produces the final values of a tile also writes, per tile row t = m/64 and channel c,
 * bn_partials[(t*K + c)*2 + {0,1}] = sum over the tile's rows of (y - bn_pivot[c]) and of its square (bn_pivot: any [K] device
 * array close to the mean, e.g. running_mean).  *bn_rows (HOST int, set before return) = number of tile rows written, or 0
 * when this launch could not produce them (other tile shape, first-generation kernel): pass both to nnl_bn_fwd, which then
 * skips its own statistics pass over y.  bn_partials needs ceil(N*P*Q/64) * K * 2 floats. */
int nnl_conv2d_fwd(const float* x, const float* w, const float* bias, float* y, const nnl_conv_geom_t* g,
                   int relu, void* workspace, size_t workspace_bytes, int32_t* tile_counters, float* bn_partials,
                   const float* bn_pivot, int32_t* bn_rows, void* stream);
/* y = conv(x, w) + bias + nearest-x2-upsample(small), small = [N, P/2, Q/2, K]: the FPN top-down merge `P5_upsampled + P4_1(C4)`,
 * `P3_1(C3) + P4_upsampled` (reference retinanet.py:126-148: nn.Upsample(scale_factor=2, mode='nearest') + add) inside the
 * lateral convolution's epilogue.  P, Q even; C % 16 == 0. */
int nnl_conv2d_fwd_add_up2(const float* x, const float* w, const float* bias, const float* small, float* y,
                           const nnl_conv_geom_t* g, void* stream);
/* its gradient with respect to `small`: dsmall[n,h,w,c] = sum of the 2x2 block of dy[N,2h,2w,C] (upsample_nearest2d backward). */
int nnl_upsample2_bwd(const float* dy, float* dsmall, int64_t N, int64_t h, int64_t w, int64_t C, void* stream);
/* wt[C,R,S,K] = transpose of w[K,R,S,C] over (K,C): the B operand of dgrad. */
int nnl_conv2d_weight_transpose(const float* w, float* wt, int K, int R, int S, int C, void* stream);
/* The same transpose for MANY filters in one launch (all convolutions of a model, once per backward pass instead of one small
 * launch per layer).  desc: DEVICE array, one entry per filter; tile_tensor: DEVICE int32 [n_tiles], the entry each 32x32 tile
 * belongs to (entry i owns tiles [first_tile, first_tile + R*S*ceil(K/32)*ceil(C/32))). */
typedef struct {
  const float* w;   /* [K,RS,C] */
  float* wt;        /* [C,RS,K] */
  int32_t K, RS, C, first_tile;
} nnl_wt_desc_t;
int nnl_conv2d_weight_transpose_multi(const nnl_wt_desc_t* desc, const int32_t* tile_tensor, int64_t n_tiles,
                                      double total_elems, void* stream);
/* dx[N,H,W,C] = sum_{r,s,k} dy[n,(h+pad-r)/stride,(w+pad-s)/stride,k] * wt[c,r,s,k] (integral taps only). */
size_t nnl_conv2d_dgrad_workspace_bytes(const nnl_conv_geom_t* g);   /* optional workspace, as for the forward */
/* addend (optional, [N,H,W,C]; K % 16 == 0 and at most 49 filter taps, at stride 1 or with a 3x3 / pad 1 filter at stride 2 — anything
 * else is refused with NNL_ERR_UNSUPPORTED): dx = dgrad + addend — the
 * gradient that reaches the block input through the shortcut of BasicBlock / Bottleneck (identity, or the input gradient
 * of the downsample convolution; retinanet.py:43-59,344-348) is added in the epilogue instead of by a separate autograd
 * accumulation kernel.  A stride-2 dgrad with even H and W runs its four output-parity classes in one launch. */
int nnl_conv2d_dgrad(const float* dy, const float* wt, float* dx, const nnl_conv_geom_t* g, const float* addend,
                     void* workspace, size_t workspace_bytes, int32_t* tile_counters, void* stream);
/* ---- 3x3 / stride 1 / pad 1 on the fused Winograd F(2,3) kernel (csrc/wino.hip) -------------------------------------------
 * nnl_conv2d_fwd and the stride-1 nnl_conv2d_dgrad use it on their own whenever the planner predicts it to be faster than the
 * direct implicit-GEMM kernel (NNL_CONV_WINO: 0 never, 1 by predicted time = default, 2 wherever it applies); results agree
 * with the direct kernel to fp32 rounding (measured 6e-6 .. 1e-5 absolute on O(1) outputs, tools/bench_wino.py).  The three
 * entry points below expose the kernel and the planners directly for the A/B tools and tests:
 *   out[N,H,W,K] = conv3x3_pad1(x[N,H,W,C], filt) (+ bias[K]) (+ add[N,H,W,K]) (ReLU when relu == 1); flip == 0: filt = w[K,3,3,C];
 *   flip == 1: filt = wt[K,3,3,C] read as wt[.,2-r,2-s,.] (the dgrad filter: x = dy, K = C_in of the layer, wt = W^T[C,R,S,K]).
 *   ws: nnl_debug_conv_wino_workspace_bytes bytes; counters: n_counters zeroed int32 (zero again on return) or NULL (plain grid);
 *   bn_part / bn_pivot (both or neither): BatchNorm partial statistics as for nnl_conv2d_fwd, one per 64 output pairs.
 * nnl_debug_conv_plan_times: out[0..3] (FOUR doubles) = predicted launch time (us) of the direct / the 1-D Winograd / the 2-D kernel for that
 *   problem (out[3] = -1: the spatially staged 2-D kernel of round 4 was removed in round 5);
 *   returns 1 when the dispatcher would pick the Winograd kernel, else 0. */
/* Prepared filters.  The transformed filter of a layer depends on its weights only, so a caller that knows all its layers can
 * transform them in ONE launch per step instead of one per convolution call:
 *   nnl_conv2d_wino_preferred(g, dgrad): which kernel nnl_conv2d_fwd (dgrad = 0) / nnl_conv2d_dgrad (dgrad = 1) takes for geometry g (given
 *     the workspace of the size query): 0 direct, 1 the 1-D F(2,3) Winograd kernel, 2 the 2-D F(2x2,3x3) one;
 *   nnl_wino_filter_multi: descriptor d transforms src [rows,3,3,ch] into dst [rows,4,3,ch]; flip = 0 with src = w[K,3,3,C]
 *     (rows = K, ch = C) gives the FORWARD filter, flip = 1 with src = W^T[C,3,3,K] (rows = C, ch = K: nnl_conv2d_weight_transpose)
 *     the DGRAD filter; block_desc[b] = descriptor served by block b, first_block = its first block, ceil(rows*3*ch / 256) blocks each;
 *   nnl_conv2d_fwd_pre / nnl_conv2d_dgrad_pre: nnl_conv2d_fwd / nnl_conv2d_dgrad with `u` = that prepared filter (NULL: exactly the
 *     plain entry points); u is used only when a Winograd kernel is taken and must then hold the layout of THAT kernel (nnl_conv2d_wino_preferred:
 *     1 -> rows * 12 * ch floats, 2 -> rows * 16 * ch floats, two_d = 1). */
typedef struct {
  const float* src;
  float* dst;
  int32_t rows, ch, flip, first_block;
  int32_t two_d, reserved;                   /* two_d = 1: dst [rows,16,ch] for the 2-D F(2x2,3x3) kernel, ceil(rows*ch / 256) blocks */
} nnl_wino_desc_t;
int nnl_conv2d_wino_preferred(const nnl_conv_geom_t* g, int dgrad);
int nnl_wino_filter_multi(const nnl_wino_desc_t* desc, const int32_t* block_desc, int64_t n_blocks, void* stream);
int nnl_conv2d_fwd_pre(const float* x, const float* w, const float* bias, float* y, const nnl_conv_geom_t* g, int relu,
                       void* workspace, size_t workspace_bytes, int32_t* tile_counters, float* bn_partials, const float* bn_pivot,
                       int32_t* bn_rows, const float* u, void* stream);
int nnl_conv2d_dgrad_pre(const float* dy, const float* wt, float* dx, const nnl_conv_geom_t* g, const float* addend,
                         void* workspace, size_t workspace_bytes, int32_t* tile_counters, const float* u, void* stream);
size_t nnl_debug_conv_wino_workspace_bytes(int N, int H, int W, int C, int K);
int nnl_debug_conv_wino_fwd(const float* x, const float* filt, const float* bias, const float* add, float* y, void* ws,
                            size_t ws_bytes, int32_t* counters, long n_counters, float* bn_part, const float* bn_pivot, int N,
                            int H, int W, int C, int K, int relu, int flip, void* stream);
/* the same through the 2-D F(2x2, 3x3) kernel (csrc/wino2.hip) */
size_t nnl_debug_conv_wino2_workspace_bytes(int N, int H, int W, int C, int K);
int nnl_debug_conv_wino2_fwd(const float* x, const float* filt, const float* bias, const float* add, float* y, void* ws,
                            size_t ws_bytes, int32_t* counters, long n_counters, float* bn_part, const float* bn_pivot, int N,
                            int H, int W, int C, int K, int relu, int flip, void* stream);
int nnl_debug_conv_plan_times(int N, int H, int W, int C, int K, double* out);

/* Route notes (debug, host side only): which kernels a call launched, and under which plan.
 *   nnl_debug_route_record(enable): start (1) or stop (0) recording on the CALLING THREAD; either way the buffer is cleared.
 *   nnl_debug_route_collect(out, n): copies the notes recorded since ("name;name;...", NUL-terminated) into out[n] and clears the buffer;
 *     returns the number of notes, or NNL_ERR_INVALID_ARG when out is NULL or too small (the buffer is kept then).
 * A name is `kernel<template arguments>:plan flags` and maps to one launch in conv2d.hip / wino.hip / wino2.hip (lstm_*: to one call
 * of nnl_lstm_fwd / nnl_lstm_bwd, see nnl_debug_lstm_plan); text after an `@` is a numeric detail of the plan (slice counts).  Recording changes no launch; when it is off a note costs one branch.
 * The tabular / collab / small-linear calls leave ONE note per successful call that launched something (none for an error return or an
 * early return at bs / n / M = 0):
 *   tab_renorm, tab_gather, tab_scatter_bwd<det>, tab_scatter_bwd<atomic>, tab_scan_bwd@blocks=<n_scan_blocks>+<blocks of the continuous part>;
 *   embdot_fwd, embdot_bwd<scan>, embdot_bwd<det>:one_block | :four_fills, embdot_bwd<atomic>:one_block | :four_fills (one_block: the
 *   four gradients are adjacent, [dU | dM | dbu | dbi], and were zero-filled by one memset; four_fills: four memsets);
 *   linear_small_fwd, linear_small_bwd:<the outputs asked for, of dx dw db, run together>@slabs=<64-row slabs of the dw / db reduction, 0 without one>. */
int nnl_debug_route_record(int enable);
int nnl_debug_route_collect(char* out, size_t n);
/* dw[K,R,S,C] = sum_{n,p,q} dy[n,p,q,k] * x[n,p*stride-pad+r,q*stride-pad+s,c]; split-K partial slabs are
 * reduced in a fixed order (bitwise reproducible).  workspace: nnl_conv2d_wgrad_workspace_bytes(g). */
size_t nnl_conv2d_wgrad_workspace_bytes(const nnl_conv_geom_t* g);
int nnl_conv2d_wgrad(const float* x, const float* dy, float* dw, const nnl_conv_geom_t* g, void* workspace,
                     size_t workspace_bytes, void* stream);
/* out[c] = sum_r a[r][c]  (bias gradients of conv / linear layers), two fixed-order stages (reproducible). */
size_t nnl_colsum_workspace_bytes(int64_t rows, int64_t cols);
/* out = src[0] + ... + src[n-1], added in that order; n in 1..8 dense fp32 tensors of numel elements, 16-byte aligned; src is a HOST
 * array of device pointers.  Replaces autograd's chain of accumulation kernels for a parameter that several forward calls share:
 * RetinaNet's head convolutions run on the five pyramid levels (RegressionModel / ClassificationModel.forward, retinanet.py:187-217,
 * 260-295), so each of their 20 weight / bias gradients was four ATen add launches per step (91 per step in all). */
int nnl_sum_tensors(const float* const* src, int n, float* out, int64_t numel, void* stream);
int nnl_colsum(const float* a, float* out, int64_t rows, int64_t cols, void* workspace, size_t workspace_bytes,
               void* stream);
/* ReLU backward gate of a conv + bias + ReLU layer (the RetinaNet head convs, retinanet.py:192-199,262-272) fused with its bias
 * gradient: g[rows,cols] = dy * [y > 0] and, if colsum != NULL, colsum[c] = sum_rows g[:,c] (fixed-order, reproducible) in one
 * pass over dy and y.  Workspace (only with colsum): nnl_colsum_workspace_bytes(rows, cols). */
int nnl_relu_gate_colsum(const float* dy, const float* y, float* g, float* colsum, int64_t rows, int64_t cols, void* workspace,
                         size_t workspace_bytes, void* stream);
/* The same pass for either fused output activation of nnl_conv2d_fwd: act 1 = ReLU gate (as above), act 2 = sigmoid gate
 * g = dy * y * (1 - y) with y the sigmoid's output (torch's sigmoid_backward; retinanet.py:286 under autograd). */
int nnl_act_gate_colsum(const float* dy, const float* y, float* g, float* colsum, int64_t rows, int64_t cols, int act,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ---- K2: BatchNorm fused with the residual add and ReLU that follow it ---------------------------------
 * Replaces nn.BatchNorm2d + `out += residual` + ReLU of BasicBlock/Bottleneck.forward (retinanet.py:47-48,53-57,
 * 81-95), the stem bn1+relu (:305-306,372-373), and nn.BatchNorm1d of Linear / StructuredDataNet
 * (General/Layers.py:35,40; StructuredData.py:1046,1078).  x,y,residual: [rows, C] row-major (NHWC: rows=N*H*W).
 * training!=0: batch statistics (biased variance for the normalisation; running_var gets the unbiased one) and
 *   running = (1-momentum)*running + momentum*batch   (running_* may be NULL: track_running_stats=False);
 * training==0: normalise with running_mean / running_var.
 * y = (x-mean)*invstd*gamma + beta [+ residual] [ReLU].  save_mean/save_invstd [C] are kept for backward.
 * Evaluated per channel as x*scale + shift (scale = invstd*gamma, shift = beta - mean*scale) while |mean*scale| <= 16, and as
 * (x - mean)*scale + beta above: the first form's rounding error grows with |mean*scale| (2^-23 * |mean*scale|), not with |y|.
 * num_batches_tracked (device int64, may be NULL): nn.BatchNorm's step counter, incremented by the training call.
 * ext_partials / ext_rows / ext_pivot (optional, training only): the (sum, sum of squares) partials written by the
 * convolution that produced x (nnl_conv2d_fwd, bn_partials) with the pivot it used — the statistics pass over x is skipped.
 * pivot_out (optional, training; may alias ext_pivot): receives this step's batch mean — the natural pivot of the next step.
 * relu_mask (optional, with relu != 0): ceil(rows*C/32) + 2 words; bit e of the flat [rows, C] element index is set when
 * y > 0.  Pass it to the backward instead of y: the ReLU gate then costs 1 bit instead of 32 per element of HBM traffic. */
size_t nnl_bn_workspace_bytes(int64_t rows, int64_t C);
int nnl_bn_fwd(const float* x, const float* gamma, const float* beta, const float* residual, float* y,
               float* save_mean, float* save_invstd, float* running_mean, float* running_var, int64_t rows,
               int64_t C, float eps, float momentum, int training, int relu, int64_t* num_batches_tracked,
               uint32_t* relu_mask, const float* ext_partials, int64_t ext_rows, const float* ext_pivot, float* pivot_out,
               void* workspace, size_t workspace_bytes, void* stream);
/* g = dy * [y > 0] (if relu; the gate comes from relu_mask when given, else from y);  dbeta = sum g;  dgamma = sum g*xhat;
 * dres = g (if dres != NULL);
 * dx = gamma*invstd*(g - dbeta/n - xhat*dgamma/n) (training) or gamma*invstd*g (eval). dgamma/dbeta may be NULL. */
int nnl_bn_bwd(const float* dy, const float* y, const uint32_t* relu_mask, const float* x, const float* gamma,
               const float* mean, const float* invstd, float* dx, float* dres, float* dgamma, float* dbeta, int64_t rows,
               int64_t C, int training, int relu, void* workspace, size_t workspace_bytes, void* stream);

/* BatchNorm -> ReLU -> MaxPool2d(ks, stride, pad) in one pass: the ResNet stem (reference retinanet.py:372-374, torchvision's
 * bn1 / relu / maxpool).  x [N,H,W,C] is the convolution output; y [N,P,Q,C] the pooled activation, idx [N,P,Q,C] the window
 * position (kh*ks + kw) of each maximum (torch's tie rule); the normalised activation itself is never written.  save_scale /
 * save_shift [C] receive the per-channel affine (the backward recomputes its ReLU gate from them); statistics, running-stat
 * update and num_batches_tracked as nnl_bn_fwd.  C % 4 == 0 and C/4 dividing 256 (nnl_bn_relu_maxpool_supported).
 * Workspace: nnl_bn_workspace_bytes(N*H*W, C). */
int nnl_bn_relu_maxpool_supported(int64_t C);
int nnl_bn_relu_maxpool_fwd(const float* x, const float* gamma, const float* beta, float* y, uint8_t* idx, float* save_mean,
                            float* save_invstd, float* save_scale, float* save_shift, float* running_mean, float* running_var,
                            int64_t N, int64_t H, int64_t W, int64_t C, int64_t P, int64_t Q, int ks, int stride, int pad, float eps,
                            float momentum, int training, int64_t* num_batches_tracked, void* workspace, size_t workspace_bytes,
                            void* stream);
/* dx [N,H,W,C], dgamma, dbeta from the pooled gradient dpool [N,P,Q,C]: every input pixel gathers dpool over the windows whose
 * arg-max it is (no atomics: reproducible), gated by the recomputed ReLU, then the two BatchNorm backward passes.  y (optional: the
 * forward's pooled output) lets the reduction pass run over the pooled outputs alone (xhat at an arg-max = (y - beta) / gamma):
 * it then reads neither x nor the windows.  The geometry is checked as in the forward: the call is refused (-1, nothing launched)
 * unless ks*ks <= 255, 2*pad <= ks, P == (H + 2*pad - ks)/stride + 1 and Q likewise (idx and dpool are indexed by P and Q as
 * stated), C passes nnl_bn_relu_maxpool_supported and N*H*W*C < 2^33. */
int nnl_bn_relu_maxpool_bwd(const float* dpool, const float* y, const uint8_t* idx, const float* x, const float* gamma,
                            const float* beta, const float* mean, const float* invstd, const float* scale, const float* shift,
                            float* dx, float* dgamma, float* dbeta,
                            int64_t N, int64_t H, int64_t W, int64_t C, int64_t P, int64_t Q, int ks, int stride, int pad,
                            int training, void* workspace, size_t workspace_bytes, void* stream);

/* What the BatchNorm entry points above would launch for a [rows, C] matrix, from the planner functions they call themselves
 * (csrc/batchnorm.hip: make_shape, ew_grid, bnpool_grid).  Host-only: no HIP call, works without a GPU.  out10 (TEN int32) =
 *   [0] VEC   floats per access: 4 when C % 4 == 0, else 1          [1] L    lanes of a wave along the channel groups (CG = C / VEC)
 *   [2] rpb   rows one block covers per loop iteration              [3] gx   row blocks = partials per channel of the reductions
 *   [4] gy    channel-group tiles                                   [5] 1 when gx was clamped to the row-block cap / gy, else 0
 *   [6] blocks of the elementwise (apply) kernels                   [7] the row-block cap itself
 *   [8] [9] nnl_bn_relu_maxpool_bwd's reduction grid over the inputs (y == NULL) and over the pooled outputs (y given) for the stem
 *           geometry N,H,W,P,Q; -1 when N <= 0 or C is refused by nnl_bn_relu_maxpool_supported.
 * Returns 1, or 0 (out10 untouched) for sizes the entry points refuse. */
int nnl_debug_bn_plan(int64_t rows, int64_t C, int64_t N, int64_t H, int64_t W, int64_t P, int64_t Q, int32_t* out10);

/* Cross-replica (synchronised) training-mode BatchNorm for data parallelism (global-batch statistics equal
 * to the single-GPU reference's).  Split-phase, the host runs the collective in between (neuralnetworklibrary_amd/ops.py):
 *   fwd:  nnl_bn_sync_stats -> all_gather of `stats` (2C+2 floats per rank) -> nnl_bn_sync_fwd
 *   bwd:  nnl_bn_sync_bwd_reduce -> all_reduce(sum) of `sums` (2C floats) -> nnl_bn_sync_bwd
 * stats = {mean_r[C], M2_r[C] = sum (x-mean_r)^2, rows>>16, rows&0xFFFF}; all_stats = [world][2C+2] in rank order, merged
 * with the pairwise (Chan) update in that order, so all ranks get bit-identical mean / invstd / running statistics.
 * dgamma / dbeta are this rank's LOCAL sums (the gradient all-reduce averages them like every other parameter);
 * dx uses the global sums and the global row count. */
int nnl_bn_sync_stats(const float* x, float* stats, int64_t rows, int64_t C, void* workspace, size_t workspace_bytes,
                      void* stream);
int nnl_bn_sync_fwd(const float* x, const float* all_stats, int world, const float* gamma, const float* beta,
                    const float* residual, float* y, float* save_mean, float* save_invstd, float* running_mean,
                    float* running_var, int64_t rows, int64_t C, float eps, float momentum, int relu,
                    int64_t* num_batches_tracked, uint32_t* relu_mask, void* workspace, size_t workspace_bytes, void* stream);
int nnl_bn_sync_bwd_reduce(const float* dy, const float* y, const uint32_t* relu_mask, const float* x, const float* mean,
                           const float* invstd, float* sums, int64_t rows, int64_t C, int relu, void* workspace,
                           size_t workspace_bytes, void* stream);
int nnl_bn_sync_bwd(const float* dy, const float* y, const uint32_t* relu_mask, const float* x, const float* gamma,
                    const float* mean, const float* invstd, const float* local_sums, const float* global_sums,
                    const float* all_stats,
                    int world, float* dx, float* dres, float* dgamma, float* dbeta, int64_t rows, int64_t C, int relu,
                    void* workspace, size_t workspace_bytes, void* stream);

/* ---- pooling of the vision path (NHWC; maxpool takes any C: 4-channel vectors when C % 4 == 0, a scalar-channel route otherwise) ----
 * nn.MaxPool2d(ksize, stride, pad) of the ResNet stem (Applications/VisionModels/retinanet.py:307,374; torchvision
 * resnet.maxpool) with torch's tie rule — `if ((val > max) || isnan(val))` in (kh, kw) scan order.  idx [N,P,Q,C] uint8 =
 * kh*ksize + kw of the winning tap, kept for the backward, which GATHERS (each input pixel sums dy over the windows whose
 * arg-max it is): no atomics, bitwise reproducible.  (P, Q) is the module's output size: floor mode, or ceil_mode=True (the pool of
 * the SENet stem, Applications/VisionModels/senet.py:314-315) by torch's rule — round up, then drop a last window that would start
 * beyond the input plus its left padding; taps outside the input are skipped on every side.  Any other P / Q is an invalid argument. */
int nnl_maxpool2d_fwd(const float* x, float* y, uint8_t* idx, int64_t N, int64_t H, int64_t W, int64_t C, int64_t P,
                      int64_t Q, int ksize, int stride, int pad, void* stream);
int nnl_maxpool2d_bwd(const float* dy, const uint8_t* idx, float* dx, int64_t N, int64_t H, int64_t W, int64_t C,
                      int64_t P, int64_t Q, int ksize, int stride, int pad, void* stream);
/* AdaptiveConcatPool2d (General/Layers.py:78-87): out[n, 0:C] = max over the HW pixels, out[n, C:2C] = their mean;
 * argmax [N,C] int32 = pixel index torch's adaptive_max_pool2d would report (first maximum / last NaN); the backward sends
 * dout[:, :C] to that pixel and dout[:, C:]/HW to every pixel. */
int nnl_concat_pool_fwd(const float* x, float* out, int32_t* argmax, int64_t N, int64_t HW, int64_t C, void* stream);
int nnl_concat_pool_bwd(const float* dout, const int32_t* argmax, float* dx, int64_t N, int64_t HW, int64_t C, void* stream);

/* ---- K15: grouped convolution, nn.Conv2d(groups = G) (Applications/VisionModels/senet.py:178-180, 205-206, 229-230) --------------
 * Activations NHWC fp32; the filter is the parameter's own channels_last memory: logical [K, C/G, R, R] stored [K, R, R, Cg], and dw
 * comes back in that layout.  Output channel k reads the input channels [g Cg, (g + 1) Cg) of its group g = k / (K / G).
 * Domain: G divides C and K (any Cg = C/G >= 1, Kg = K/G >= 1), R in {1, 3}, stride in {1, 2}, 0 <= pad <= R / 2, N < 65536, every
 * tensor below 2^31 elements; anything else is NNL_ERR_INVALID_ARG and nothing is launched.  P = (H + 2 pad - R) / stride + 1, Q likewise.
 * Direct kernels (csrc/gconv.hip), every sum in a fixed order and no atomics: two calls on the same inputs give the same bits.
 * nnl_gconv2d_fwd (Applications/VisionModels/senet.py:178-180, 205-206, 229-230): y = conv(x, w) + bias (bias may be NULL), ReLU when relu != 0. */
int nnl_gconv2d_fwd(const float* x, const float* w, const float* bias, float* y, int64_t N, int64_t H, int64_t W, int64_t C, int64_t K,
                    int64_t G, int R, int stride, int pad, int relu, void* stream);
/* nnl_gconv2d_dgrad (backward of senet.py:178-180, 205-206, 229-230): dx [N,H,W,C] from dy [N,P,Q,K] taken at the convolution's output;
 * every element of dx is written. */
int nnl_gconv2d_dgrad(const float* dy, const float* w, float* dx, int64_t N, int64_t H, int64_t W, int64_t C, int64_t K, int64_t G,
                      int R, int stride, int pad, void* stream);
/* nnl_gconv2d_wgrad (backward of senet.py:178-180, 205-206, 229-230): dw [K, R, R, Cg].  The N*P*Q pixels are cut into slices whose
 * partial sums go to the workspace (nnl_gconv2d_workspace_bytes; 0 = one slice, ws may be NULL) and are added in slice order by a second
 * launch; a workspace that is too small is NNL_ERR_WORKSPACE. */
size_t nnl_gconv2d_workspace_bytes(int64_t N, int64_t H, int64_t W, int64_t C, int64_t K, int64_t G, int R, int stride, int pad);
int nnl_gconv2d_wgrad(const float* x, const float* dy, float* dw, void* ws, size_t ws_bytes, int64_t N, int64_t H, int64_t W, int64_t C,
                      int64_t K, int64_t G, int R, int stride, int pad, void* stream);

/* ---- K18: depthwise convolution, nn.Conv2d(C, C, R, groups = C) (Applications/VisionModels/nasnet.py SeparableConv2d) ------------------
 * Activations NHWC fp32; w is the parameter as it is stored, [C, 1, R, R]; dw comes back in that layout.  R in {3, 5, 7}, stride in {1, 2},
 * any C (a 4-channel vector route when C % 4 == 0, a scalar-channel route otherwise).  The padding is stated from the top/left only: tap
 * (r, s) of output (p, q) reads x[p stride - pad_lo + r, q stride - pad_lo + s], everything outside the image reads as zero, and the
 * caller states P and Q: 0 <= pad_lo <= R - 1, P >= 1, (P - 1) stride - pad_lo <= H - 1 (every window touches the image), Q likewise.
 * N < 65536, every tensor below 2^31 elements.  Anything else is NNL_ERR_INVALID_ARG and nothing is launched.
 * relu_in != 0 convolves max(x, 0) (the ReLU in front of every BranchSeparables, whose input other branches read un-rectified).
 * Every sum runs in a fixed order and there are no atomics: two calls on the same inputs give the same bits.
 * nnl_dwconv2d_fwd: y [N,P,Q,C] = conv(act(x), w) + bias (bias may be NULL). */
int nnl_dwconv2d_fwd(const float* x, const float* w, const float* bias, float* y, int64_t N, int64_t H, int64_t W, int64_t C, int64_t P,
                     int64_t Q, int R, int stride, int pad_lo, int relu_in, void* stream);
/* nnl_dwconv2d_dgrad: dx [N,H,W,C] from dy [N,P,Q,C], gathered per input pixel over the taps whose output position exists; every element
 * of dx is written.  With relu_in the result is gated by x > 0 (x is required then, and may be NULL otherwise). */
int nnl_dwconv2d_dgrad(const float* dy, const float* w, const float* x, float* dx, int64_t N, int64_t H, int64_t W, int64_t C, int64_t P,
                       int64_t Q, int R, int stride, int pad_lo, int relu_in, void* stream);
/* nnl_dwconv2d_wgrad: dw[c, r, s] = sum over n, p, q of dy * act(x).  The N*P*Q pixels are cut into slabs whose partial sums go to the
 * workspace (nnl_dwconv2d_wgrad_workspace_bytes; 0 = one slab, ws may be NULL) and are added in slab order by a second launch; a
 * workspace that is too small is NNL_ERR_WORKSPACE. */
size_t nnl_dwconv2d_wgrad_workspace_bytes(int64_t N, int64_t H, int64_t W, int64_t C, int64_t P, int64_t Q, int R, int stride, int pad_lo);
int nnl_dwconv2d_wgrad(const float* x, const float* dy, float* dw, void* ws, size_t ws_bytes, int64_t N, int64_t H, int64_t W, int64_t C,
                       int64_t P, int64_t Q, int R, int stride, int pad_lo, int relu_in, void* stream);

/* ---- K18: average pooling and strided subsampling of the NASNet cells (nasnet.py AvgPoolPad, the cells' AvgPool2d, path_1 / path_2) ----
 * nnl_avgpool2d_*: nn.AvgPool2d(ksize, stride, pad, count_include_pad), NHWC, any C, with the same stated-P/Q, pad_lo convention and
 * checks as the depthwise convolution (1 <= ksize <= 15, 0 <= pad_lo <= ksize - 1).  The divisor of a window is the number of its taps
 * inside the image (count_include_pad == 0) or ksize^2.  The backward gathers: no atomics. */
int nnl_avgpool2d_fwd(const float* x, float* y, int64_t N, int64_t H, int64_t W, int64_t C, int64_t P, int64_t Q, int ksize, int stride,
                      int pad_lo, int count_include_pad, void* stream);
int nnl_avgpool2d_bwd(const float* dy, float* dx, int64_t N, int64_t H, int64_t W, int64_t C, int64_t P, int64_t Q, int ksize, int stride,
                      int pad_lo, int count_include_pad, void* stream);
/* nnl_subsample2d_*: y[p, q] = x[p stride + off, q stride + off], or 0 outside the image: AvgPool2d(1, stride) (off = 0) and the
 * ZeroPad2d((0, 1, 0, 1)) -> [1:, 1:] -> AvgPool2d(1, 2) chain (off = 1).  The backward writes every element of dx. */
int nnl_subsample2d_fwd(const float* x, float* y, int64_t N, int64_t H, int64_t W, int64_t C, int64_t P, int64_t Q, int stride, int off,
                        void* stream);
int nnl_subsample2d_bwd(const float* dy, float* dx, int64_t N, int64_t H, int64_t W, int64_t C, int64_t P, int64_t Q, int stride, int off,
                        void* stream);

/* ---- K15: squeeze-and-excitation tail of a SENet block (Applications/VisionModels/senet.py:118-137 SEModule, :161-162) -------------
 *   out = relu( x * sigmoid(z[n, c]) + residual ),  z = fc2(relu(fc1(m))),  m[n, c] = mean over the HW pixels of x   (x NHWC = [N, HW, C])
 * nnl_se_squeeze: m [N, C], summed in a fixed order.  nnl_se_excite_fwd: one pass; z holds the PRE-sigmoid logits; residual may be NULL;
 * C % 4 == 0.  nnl_se_excite_bwd: g = dy * [out > 0]; dres = g (dres may be NULL); dx = g * sigmoid(z); dz[n, c] = sigmoid'(z) *
 * sum_h g * x, accumulated in fp64 in a fixed order and rounded once.  nnl_se_squeeze_bwd: dx += dm[n, c] / HW, the gradient of the mean
 * (C % 4 == 0).  No atomics: bitwise repeatable.  N < 65536, HW < 2^30, C < 2^22. */
int nnl_se_squeeze(const float* x, float* m, int64_t N, int64_t HW, int64_t C, void* stream);
int nnl_se_excite_fwd(const float* x, const float* z, const float* residual, float* out, int64_t N, int64_t HW, int64_t C, void* stream);
int nnl_se_excite_bwd(const float* dy, const float* out, const float* x, const float* z, float* dx, float* dres, float* dz, int64_t N,
                      int64_t HW, int64_t C, void* stream);
int nnl_se_squeeze_bwd(const float* dm, float* dx, int64_t N, int64_t HW, int64_t C, void* stream);

/* ---- detection inference: the device half of BBoxPredictor.__call__ / nms (Applications/VisionModels/retinanet.py:523-812)
 * nnl_bbox_decode: per (image, anchor) best class (first maximum) and its score; keep score > thresh; decode the box
 *   (cx + w*(reg0*std0+mean0), ..., w*exp(reg2*std2+mean2), ...), clip to [0,width]x[0,height], drop empty boxes
 *   (retinanet.py:762-800).  anchors [A,4], reg [bs,A,4], clas [bs,A,K]; mean4 / std4 are HOST arrays.  Candidates are
 *   appended per image in arbitrary order: cand_* have capacity A per image, cand_order = anchor index, cand_count [bs].
 * nnl_nms: top_k candidates by (score descending, order ascending), then greedy non-maximum suppression inside a class with
 *   IoU > max_overlap (retinanet.py:581-604; IoU in the reference's fp32 operation order).  cand_order may be NULL (= position).
 *   kept_* [bs][top_k] in descending score order, kept_count [bs].  The remaining list filters of nms() (relative
 *   thresholds, inclusions, cross-class duplicates, max_boxes) act on the few survivors and stay on the host.
 * The contracts in full (tests/detect_cases.py pins each of them):
 *   decode   the class is the FIRST maximum of the K scores; a NaN among them drops the anchor.  The compare is strict: a score equal
 *            to thresh is dropped.  A box is dropped when its clipped width or height is not > 0.  Written: cand_count [bs], and of
 *            cand_boxes / cand_classes / cand_scores / cand_order the slots [0, cand_count) of every image; no other slot is touched.
 *            The order of the slots is not defined (atomic append): cand_order identifies them.
 *   nms      The candidates of an image are the slots [0, min(cand_count, cap)): a cand_count above cap is read as cap.  They are
 *            ranked by the TOTAL order (score descending, cand_order ascending; the slot position when cand_order is NULL), so the
 *            result does not depend on the order of the slots; cand_order values of one image must differ.  -0.0 and +0.0 are one
 *            score.  The first min(n, top_k) of the ranking enter the suppression — the cut comes BEFORE it.  In rank order a box is
 *            kept unless an earlier KEPT box of the same class has IoU > max_overlap (strict; a suppressed box suppresses nothing; an
 *            IoU of 0/0 = NaN suppresses nothing).  Written: kept_count [bs] and the slots [0, kept_count) of kept_boxes /
 *            kept_classes / kept_scores, bitwise copies of the candidates; no other slot is touched.  top_k may exceed cap.
 *            workspace: nnl_nms_workspace_bytes(bs, top_k) bytes (0 for non-positive sizes), 16-byte aligned, contents irrelevant. */
int nnl_bbox_decode(const float* anchors, const float* reg, const float* clas, int64_t bs, int64_t A, int64_t K,
                    const float* mean4, const float* std4, float thresh, float width, float height, float* cand_boxes,
                    int32_t* cand_classes, float* cand_scores, int32_t* cand_order, int32_t* cand_count, void* stream);
/* nnl_bbox_decode with the clip window [x_min, x_max] x [y_min, y_max] (0 <= x_min < x_max, 0 <= y_min < y_max) in place of
 * [0, width] x [0, height]: ImageLearner.TTA_bbox clips every pass's boxes to the part of the padded, jittered minibatch that IS the
 * image, [col_jit, col_jit + rw] x [row_jit, row_jit + rh], so that the undone boxes lie inside the original image. */
int nnl_bbox_decode_window(const float* anchors, const float* reg, const float* clas, int64_t bs, int64_t A, int64_t K,
                           const float* mean4, const float* std4, float thresh, float x_min, float y_min, float x_max, float y_max,
                           float* cand_boxes, int32_t* cand_classes, float* cand_scores, int32_t* cand_order, int32_t* cand_count,
                           void* stream);
size_t nnl_nms_workspace_bytes(int64_t bs, int64_t top_k);
int nnl_nms(const float* cand_boxes, const int32_t* cand_classes, const float* cand_scores, const int32_t* cand_order,
            const int32_t* cand_count, int64_t bs, int64_t cap, int64_t top_k, float max_overlap, float* kept_boxes,
            int32_t* kept_classes, float* kept_scores, int32_t* kept_count, void* workspace, size_t workspace_bytes,
            void* stream);

/* ---- K11: detection test-time augmentation — the undo and concatenation of ImageLearner.TTA_bbox (Applications/Vision.py:2084-2112)
 * The reference maps every pass's surviving boxes back to the original image with four numpy expressions per (pass, image) and
 * concatenates the passes as Python lists.  Here, for L images, P passes and M slots per pass, in ONE launch (one workgroup per image):
 * boxes [L,P,M,4] (xmin, ymin, xmax, ymax), classes [L,P,M], scores [L,P,M]; counts [L,P] = survivors of (image, pass), in slots
 * [0, count) in descending score order.  undo [L,P]: x -= col_jit, y -= row_jit (:2093), every coordinate times inv (:2094; inv =
 * 1 / (rand_scale scale) taken in float64 by the caller and rounded ONCE to fp32, as numpy does with a Python float against a float32
 * array), then with flip != 0 (xmin, xmax) = (cols - xmax, cols - xmin) (:2096).  fp32, every operation rounded on its own (no fused
 * multiply-add): bit for bit what numpy computes.
 * Out, in the layout nnl_nms reads with cap = P M: image l's candidates compacted in pass order, then slot order (:2105-2112);
 * cand_order = that position, so that nnl_nms's tie rule (score descending, order ascending) sees the reference's concatenation
 * order; cand_count [L].  The slots past cand_count are written too (box 0, class -1, score 0, order = position): the output is a
 * function of the input alone, no atomics.  A count outside [0, M] is not followed: that pass contributes nothing and *err_flag
 * (device int32, may be NULL) is set to 1.  L in [1, 2^31), P in [1, 64], M >= 1, P M <= 2^20. */
typedef struct {
  float col_jit, row_jit;        /* the pass's jitter: left and top padding of the transformed image */
  float inv;                     /* fp32(1.0 / (rand_scale * scale)) */
  float cols;                    /* width of the ORIGINAL image */
  int32_t flip;                  /* != 0: the pass mirrored the image */
} nnl_tta_undo_t;                /* 20 bytes */
int nnl_tta_bbox_merge(const float* boxes, const int32_t* classes, const float* scores, const int32_t* counts,
                       const nnl_tta_undo_t* undo, int64_t L, int64_t P, int64_t M, float* cand_boxes, int32_t* cand_classes,
                       float* cand_scores, int32_t* cand_order, int32_t* cand_count, int32_t* err_flag, void* stream);

/* ---- K3: categorical-embedding front end of StructuredDataNet --------------------------------------------
 * Replaces, per categorical column j, EmbeddingDrop.forward (General/Layers.py:74-76: nn.Embedding(max_norm=1.5)
 * in-place renorm + gather + per-sample dropout mask) and the two torch.cat calls of StructuredDataNet.forward
 * (Applications/StructuredData.py:1075-1082).  Descriptor arrays are DEVICE arrays with one entry per column:
 * tables[j] (pointer to W_j [card[j], dim[j]]), card, dim, col_off (first output column of column j);
 * col_table[c] = column owning output column c (c < cat_width = sum dim); row_off[j] = first global row id of
 * table j, row_table[r] = table owning global row r (r < total_rows = sum card); flags: int32[total_rows], zero
 * on entry and on exit.
 * Indices outside [0, card[j]) — negative, card[j] and above, and 64-bit values whose low 32 bits would be in range — are SKIPPED by
 * every call below: zero output columns in the forward, no gradient from that sample to column j in all three backward routes.  Only
 * nnl_tab_renorm reports them (*err_flag = 1); nnl_tab_gather_fwd and the backward calls take no flag and stay silent, so a caller that
 * does not renorm (max_norm = None) and cannot vouch for its indices has to check them itself. */
/* In-place max_norm renormalisation of every row looked up by xcat [bs, ncat] (each distinct row exactly once):
 * rows with L2 norm > max_norm are scaled by max_norm/(norm+1e-7)  (torch embedding_renorm_). */
int nnl_tab_renorm(const int64_t* xcat, float* const* tables, const int32_t* card, const int32_t* dim,
                   const int32_t* row_off, const int32_t* row_table, int32_t* flags, int64_t bs, int32_t ncat,
                   int32_t total_rows, float max_norm, int32_t* err_flag, void* stream);
/* out [bs, ld_out]: columns [col_off[j], +dim[j]) = tables[j][xcat[b,j]] * row_mask[j,b]  (row_mask [ncat,bs] or
 * NULL = ones); columns [cat_width, +n_cont) = cont[b,:] * cont_mask[b,:] (cont_mask NULL = ones); rest = 0. */
int nnl_tab_gather_fwd(const int64_t* xcat, const float* const* tables, const int32_t* card, const int32_t* dim,
                       const int32_t* col_off, const int32_t* col_table, const float* row_mask, const float* cont,
                       const float* cont_mask, float* out, int64_t bs, int32_t ncat, int32_t cat_width,
                       int32_t n_cont, int32_t ld_out, void* stream);
/* Backward: dense table gradients (nn.Embedding sparse=False) scatter-added into ONE flat zero-filled buffer
 * dtab_flat (table j at element offset grad_off[j]), and dcont [bs, n_cont] = dout[:, cat_width:] * cont_mask. */
size_t nnl_tab_scatter_bwd_workspace_bytes(int64_t bs, int32_t ncat);      /* deterministic scatter: see nnl_embdotbias_bwd */
int nnl_tab_scatter_bwd(const int64_t* xcat, const int32_t* card, const int32_t* dim, const int32_t* col_off,
                        const int32_t* col_table, const int64_t* grad_off, const float* row_mask,
                        const float* cont_mask, const float* dout, float* dtab_flat, int64_t dtab_elems,
                        float* dcont, int64_t bs, int32_t ncat, int32_t cat_width, int32_t n_cont, int32_t ld_out,
                        void* workspace, size_t workspace_bytes, void* stream);
/* The same backward WITHOUT a sort, in one launch (round 4; embedding widths <= 32): block b < n_scan_blocks owns the flat elements
 * blk_first[b] .. +255 of column blk_col[b]'s [card][dim] gradient and scans that column's bs indices in sample order (the
 * summation order of nnl_tab_scatter_bwd's deterministic path); every element of dtab_flat is written (no zero fill needed), the
 * continuous columns' gradient rides along.  dout may have any row stride ld_out >= cat_width + n_cont. */
int nnl_tab_scan_bwd(const int64_t* xcat, const int32_t* card, const int32_t* dim, const int32_t* col_off,
                     const int64_t* grad_off, const float* row_mask, const float* cont_mask, const float* dout,
                     float* dtab_flat, float* dcont, const int32_t* blk_col, const int32_t* blk_first, int32_t n_scan_blocks,
                     int32_t max_dim, int64_t bs, int32_t ncat, int32_t cat_width, int32_t n_cont, int32_t ld_out, void* stream);

/* dst [rows, Cp] = src [rows, C] followed by zero columns (channel padding to the kernels' 4-float granularity, one launch). */
int nnl_pad_cols(const float* src, float* dst, int64_t rows, int64_t C, int64_t Cp, void* stream);
/* Two dropout keep masks from ONE uniform draw u [na + nb]: a[i] = (u[i] < keep_a) / keep_a, b[i] = (u[na + i] < keep_b) / keep_b —
 * the per-sample row masks of EmbeddingDrop and the continuous-input mask of StructuredDataNet (General/Layers.py:75-76,
 * StructuredData.py:1079: nn.Dropout applied to ones / to the inputs: Bernoulli(keep) / keep). */
int nnl_keep_masks(const float* u, float* a, int64_t na, float keep_a, float* b, int64_t nb, float keep_b, void* stream);

/* nn.Linear with 1 - 4 output features (the last layer of FullyConnectedNet, General/Layers.py:146 — the tabular regression head):
 * y [M,N] = x [M,K] (row stride ldx) w[N,K]^T + bias.  Backward: dx [M,K] dense, dw [N,K], db [N] (any may be NULL), fixed-order
 * sums (csrc/linear_small.hip); M = 0 zero-fills dw and db.  A workspace that is NULL or smaller than
 * nnl_linear_small_bwd_workspace_bytes (needed for dw or db) is NNL_ERR_WORKSPACE, and no output is written. */
int nnl_linear_small_supported(int64_t N);
int nnl_linear_small_fwd(const float* x, const float* w, const float* bias, float* y, int64_t M, int64_t K, int64_t ldx, int64_t N,
                         void* stream);
size_t nnl_linear_small_bwd_workspace_bytes(int64_t M, int64_t K, int64_t N);
int nnl_linear_small_bwd(const float* dy, const float* x, const float* w, float* dx, float* dw, float* db, int64_t M, int64_t K,
                         int64_t ldx, int64_t N, void* workspace, size_t workspace_bytes, void* stream);

/* ---- K6: fused RetinaNet detection loss (anchor matching + focal + smooth-L1) -----------------------------
 * Replaces SSD_loss.__call__ and everything it calls per image (Applications/Vision.py:1620-1644 -> ssd1 :1568-1605,
 * match_anchors_objects :1474-1511, jaccard :234-256, focal_loss_retina :1513-1530, smoothL1_loss_retina :1532-1566).
 * anchors [A,4]; reg [bs,A,4]; clas [bs,A,K] (probabilities); boxes [bs,M,4], cats int64 [bs,M], both padded with -1
 * (Vision.py:798-809), M <= 128.  Outputs: out[3] = {(1-beta)*reg + beta*clas, reg_loss, clas_loss} (batch means),
 * state int32 [bs,A] (>=0 matched object, -1 negative, -2 ignored) and npos float [bs] are kept for backward.
 * Preconditions (relied on, not checked): every anchor has positive area — a zero-area anchor against a zero-area object gives
 * IoU 0/0, which the kernel's comparisons file as negative where torch's max makes the anchor ignored; generated anchors never
 * have zero area; cats are in [0, K) or negative (any negative value = padding row, anywhere in the list); anchors, reg and boxes
 * are 16-byte aligned (clas and dclas too when K % 4 == 0).  M = 0 may come with boxes = cats = NULL; with M > 0 both calls
 * refuse NULL.  Sizes: 0 < bs < 65536, 0 < A < 2^30, 0 < K <= 4096, 0 <= M <= 128, else NNL_ERR_INVALID_ARG; a workspace that is
 * NULL or smaller than nnl_retina_loss_workspace_bytes(bs, A) = bs * ceil(A / 256) * 12 bytes is NNL_ERR_WORKSPACE. */
size_t nnl_retina_loss_workspace_bytes(int64_t bs, int64_t A);
int nnl_retina_loss_fwd(const float* anchors, const float* reg, const float* clas, const float* boxes,
                        const int64_t* cats, int32_t* state, float* npos, float* out, int64_t bs, int64_t A,
                        int64_t K, int64_t M, float beta, float alpha, float gamma, void* workspace,
                        size_t workspace_bytes, void* stream);
/* dreg [bs,A,4], dclas [bs,A,K] = d out[0] / d reg, d clas times *grad_out (device scalar). */
int nnl_retina_loss_bwd(const float* anchors, const float* reg, const float* clas, const float* boxes,
                        const int64_t* cats, const int32_t* state, const float* npos, const float* grad_out,
                        float* dreg, float* dclas, int64_t bs, int64_t A, int64_t K, int64_t M, float beta,
                        float alpha, float gamma, void* stream);

/* ---- K5: recurrence of one weight-dropped LSTM layer --------------------------------------------------------
 * Replaces nn.LSTM(num_layers=1) as called by WeightDropLSTM1.forward (Applications/Text.py:495-513) inside
 * LSTM_Encoder.forward (:543-548): gates_t = gx_t + h_{t-1} W_hh^T, c_t = s(f) c_{t-1} + s(i) tanh(g),
 * h_t = s(o) tanh(c_t), gate order i,f,g,o (torch).  gx [T,B,4H] = x_t W_ih^T + b_ih + b_hh for all t (one big
 * GEMM done by the caller with nnl_conv2d_fwd as a 1x1 conv).  Padded operands (the GEMM k dimension must be a
 * multiple of 32): Hp = nnl_lstm_padded_hidden(H) = ceil32(H), Gp = nnl_lstm_padded_gates(H) = ceil32(4H);
 * w_hh_pad [4H, Hp] = (dropped) W_hh with zero-padded rows; h0, c0 [B,H].  Outputs y [T,B,H] (h_t), cy [T,B,H] (c_t)
 * and gates [T,B,4H] (ACTIVATED i,f,g,o) — the last two are saved for backward.
 * One kernel launch per timestep: the recurrent GEMM runs in k slices over <= 256 workgroups and the workgroup that finishes
 * a tile last (atomic ticket, nobody waits) sums the slices in a fixed order and applies the cell (csrc/lstm.hip).
 * PERSISTENT path (csrc/lstm_persist.hip; B <= 64 and the per-workgroup W_hh slice fits the LDS — the AWD-LSTM shapes): ONE
 * cooperative launch per layer and direction; ceil(H/U) <= 256 workgroups keep their 4U rows of W_hh in LDS for all T steps,
 * exchange h_t through a k-major buffer with one slot per timestep and meet at a grid barrier per step.
 * err_flag: one int32 of device memory (may be NULL: per-timestep path only); a persistent launch whose grid barrier times out
 * sets it to 2 and drains. */
int64_t nnl_lstm_padded_hidden(int64_t H);
int64_t nnl_lstm_padded_gates(int64_t H);
size_t nnl_lstm_workspace_bytes(int64_t T, int64_t B, int64_t H);
int nnl_lstm_fwd(const float* gx, const float* w_hh_pad, const float* h0, const float* c0, float* y, float* cy,
                 float* gates, int64_t T, int64_t B, int64_t H, void* workspace, size_t workspace_bytes, int32_t* err_flag,
                 void* stream);
/* BPTT: dy [T,B,H] (may be NULL), dhT / dcT [B,H] (may be NULL = 0), w_hh_t_pad [H, Gp] = W_hh^T with zero-padded rows.
 * Outputs dgates_pad [T,B,Gp] (columns < 4H: gradient of the PRE-activation gates = d gx; columns >= 4H are not written
 * and must be zero on entry; the caller derives dW_ih, dW_hh, db, dx from it with the GEMM entry points), dh0, dc0 [B,H]. */
int nnl_lstm_bwd(const float* dy, const float* dhT, const float* dcT, const float* gates, const float* cy,
                 const float* c0, const float* w_hh_t_pad, float* dgates_pad, float* dh0, float* dc0, int64_t T, int64_t B,
                 int64_t H, void* workspace, size_t workspace_bytes, int32_t* err_flag, void* stream);
/* The partition (KG x NG workgroups, k-slice Ks, column slice Ns, NT column tiles -> out5) the 2-D persistent BPTT kernel
 * (csrc/lstm_bptt2.hip) would use for this shape; returns 0 when the shape does not fit it.  Host-only. */
int nnl_debug_lstm_bptt2_plan(int64_t B, int64_t H, int32_t* out5);
/* What the host code of csrc/lstm.hip, lstm_persist.hip and lstm_bptt2.hip decides for batch B and hidden size H (tests/lstm_cases.py
 * derives from it which loops and template instantiations a case reaches).  Host only: no HIP call, works without a device.  It calls
 * the functions the entry points call (make_plan, shape_of, plan2).  out14:
 *   [0] Hp    padded hidden size                                    [1] Gp   padded gate columns
 *   [2] tf    tiles of a per-timestep forward launch                [3] tb   tiles of a per-timestep backward GEMM
 *   [4] sf    k slices of the per-timestep forward                  [5] sb   k slices (slabs) of the per-timestep backward
 *   [6] 1 when the persistent kernels (lstm_persist.hip) take the shape, else 0
 *   [7] U     hidden units per workgroup = their template argument  [8] NWG  their workgroups   (both reported also where [6] is 0)
 *   [9] 1 when the 2-D partitioned BPTT (lstm_bptt2.hip) takes the shape, else 0; then
 *   [10] NT, [11] PB  its template arguments                        [12] KG, [13] NG  its partition   (all four 0 where [9] is 0)
 * Which of these kernels a call runs depends further on NNL_LSTM_PERSIST, NNL_LSTM_FUSED_BWD and err_flag; the route notes
 * (nnl_debug_route_record) name the one that ran: lstm_persist_fwd<U>@NWG, lstm_step_fwd@sf, lstm_bptt2<NT,PB>@KGxNG,
 * lstm_persist_bwd<U>@NWG, lstm_step_bwd@sb, lstm_step_bwd:fused@sb — one per call, written after its launches were issued.
 * Returns 1, or 0 (out14 untouched) for sizes the entry points refuse, B >= 2^24 or out14 == NULL. */
int nnl_debug_lstm_plan(int64_t B, int64_t H, int32_t* out14);

/* nn.MSELoss(reduction='mean') — `loss_func_dict['cont']` (General/Learner.py:20), the loss of the collaborative-filtering and
 * structured-data heads: *loss = mean((pred - target)^2) over n fp32 elements (one launch up to 65 536 samples, fixed-order sum);
 * backward: dpred = *grad_out (device scalar, NULL = 1) * 2 (pred - target) / n.  Workspace only above 65 536 samples. */
size_t nnl_mse_workspace_bytes(int64_t n);
int nnl_mse_fwd(const float* pred, const float* target, float* loss, int64_t n, void* workspace, size_t workspace_bytes, void* stream);
int nnl_mse_bwd(const float* pred, const float* target, const float* grad_out, float* dpred, int64_t n, void* stream);
/* nn.BCEWithLogitsLoss() — `loss_func_dict['multi_label']` (General/Learner.py:20), the loss of the multi-label image classifier
 * (Planet notebook): *loss = mean(max(x, 0) - x t + log1p(exp(-|x|))) over n fp32 elements, targets anywhere in [0, 1] (one launch up
 * to 65 536 elements, fixed-order sum: bitwise reproducible); backward: dlogits = *grad_out (device scalar, NULL = 1) *
 * (sigmoid(x) - t) / n, 16-byte accesses when the three pointers are 16-byte aligned.  Workspace only above 65 536 elements. */
size_t nnl_bce_logits_workspace_bytes(int64_t n);
int nnl_bce_logits_fwd(const float* logits, const float* target, float* loss, int64_t n, void* workspace, size_t workspace_bytes, void* stream);
int nnl_bce_logits_bwd(const float* logits, const float* target, const float* grad_out, float* dlogits, int64_t n, void* stream);
/* fbeta_loss.__call__ (General/LossesMetrics.py:70-78), the multi-label F-beta metric, on pred / target fp32 [N, C]: per row
 * p_c = use_thresh ? (sigmoid(pred_c) >= threshold) : pred_c, tp = sum p t, prec = tp / (sum p + eps), rec = tp / (sum t + eps),
 * f = (1 + beta2) prec rec / (beta2 prec + rec + eps), all in fp32 in that order; *out = mean over the rows, summed in a fixed
 * order.  One launch up to 4 096 rows, two (and a workspace) above. */
size_t nnl_fbeta_workspace_bytes(int64_t N, int64_t C);
int nnl_fbeta(const float* pred, const float* target, float* out, int64_t N, int64_t C, float beta2, float threshold, int use_thresh, float eps,
              void* workspace, size_t workspace_bytes, void* stream);
/* FullyConnectedNet's 'sigmoidal' output activation (General/Layers.py:150-152): y = lo + (hi - lo) * sig, sig = sigmoid(x) (both
 * written); backward: dx = dy * (hi - lo) * sig * (1 - sig). */
int nnl_scaled_sigmoid_fwd(const float* x, float* y, float* sig, int64_t n, float lo, float hi, void* stream);
int nnl_scaled_sigmoid_bwd(const float* dy, const float* sig, float* dx, int64_t n, float lo, float hi, void* stream);

/* ---- K5b: embedding with per-vocabulary-row dropout mask, fused softmax + cross-entropy -----------------------
 * nnl_embedding_rowmask_*: EmbeddingDropout.forward, F.embedding(x, W * mask[V,1], pad) (Text.py:465-475):
 * out[i,:] = W[x[i],:] * rowmask[x[i]] (rowmask NULL = ones); backward zero-fills dW [V,D] and scatter-adds
 * dout[i,:]*rowmask[x[i]] except for x[i] == padding_idx (pass -1 for none).  The backward adds the samples of a row in a fixed order
 * (route note emb_rowmask_bwd<det>) when it has its workspace, n <= 32768 and NNL_SCATTER_ATOMIC is not 1; else with fp32 atomics
 * (emb_rowmask_bwd<atomic>), which is not bitwise reproducible. */
int nnl_embedding_rowmask_fwd(const int64_t* x, const float* W, const float* rowmask, float* out, int64_t n,
                              int64_t V, int64_t D, int32_t* err_flag, void* stream);
size_t nnl_embedding_rowmask_bwd_workspace_bytes(int64_t n);               /* deterministic scatter: see nnl_embdotbias_bwd */
int nnl_embedding_rowmask_bwd(const int64_t* x, const float* rowmask, const float* dout, float* dW, int64_t n,
                              int64_t V, int64_t D, int64_t padding_idx, void* workspace, size_t workspace_bytes, void* stream);
/* F.cross_entropy(logits [rows,V], target [rows], reduction='mean') (Text.py:773; also nn.CrossEntropyLoss of
 * General/Learner.py:20).  row_stats [rows][2] (8-byte aligned) = {m, log s} per row, m = max_v logits[r,v] and s = sum_v exp(logits[r,v] - m): the two
 * halves of logsumexp are stored apart from forward to backward.  For |m| > 16 they are never added: loss_rows[r] = log s -
 * (logits[r,target[r]] - m), so that no rounding is relative to |m| (softmax is shift-invariant, and so are the results up to rounding).
 * For |m| <= 16 the kernels form lse = m + log s, loss_rows[r] = lse - logits[r,target[r]] and p = exp(logits - lse), bit for bit what
 * they formed while they stored lse alone; that sum rounds by at most (16 + log s) 2^-24.  *loss_mean = mean over all rows.
 * A -inf logit (a masked class) has probability and gradient exactly 0; a row of nothing but -inf, or one holding NaN or +inf, gives
 * NaN as F.cross_entropy does.  A target outside [0, V): loss_rows[r] = 0 and *err_flag = 1 (err_flag may be NULL).
 * Backward: dlogits = (p - onehot) * (*grad_out) / rows, p = exp((logits - m) - log s) (|m| <= 16: exp(logits - lse)). */
int nnl_softmax_ce_fwd(const float* logits, const int64_t* target, float* row_stats, float* loss_rows, float* loss_mean,
                       int64_t rows, int64_t V, int32_t* err_flag, void* stream);
/* ld_dlogits >= V: row stride of dlogits; columns [V, ld_dlogits) are written as zeros (a gradient buffer whose rows are already
 * padded to the GEMM granularity saves the consumer an 848 MB pad copy at V = 47 343). */
int nnl_softmax_ce_bwd(const float* logits, const int64_t* target, const float* row_stats, const float* grad_out,
                       float* dlogits, int64_t rows, int64_t V, int64_t ld_dlogits, void* stream);
/* AR / TAR regularisers of RegSeqCrossEntropyLoss (Text.py:765-777) on h = enc_out [T, R] (R = bs * emb_dim, contiguous):
 * out3[0] = alpha * mean(h^2) + beta * mean((h[1:] - h[:-1])^2), out3[1] = mean(h^2), out3[2] = the second mean; fixed-order
 * two-stage sums (bitwise reproducible).  Backward: dh = *grad_out (device scalar, NULL = 1) * d out3[0] / dh. */
size_t nnl_seq_reg_workspace_bytes(int64_t T, int64_t R);
int nnl_seq_reg_fwd(const float* h, float* out3, int64_t T, int64_t R, float alpha, float beta, void* workspace,
                    size_t workspace_bytes, void* stream);
int nnl_seq_reg_bwd(const float* h, const float* grad_out, float* dh, int64_t T, int64_t R, float alpha, float beta, void* stream);
/* WeightDropLSTM1's weight drop (Text.py:495-513: W = Dropout_p(W_hh_raw), one mask per forward call) fused with the zero
 * padding / un-padding of the recurrent matrix: out[r, c] = src[r*ld_src + c] * m(r, c) for c < H and 0 for H <= c < ld_out.
 * m = mask[r*H + c] when mask != NULL (an explicit, already scaled mask: parity tests, keyed dropout); otherwise
 * m = [u(seed, r*H + c) >= p] / (1 - p) from a counter-based hash (p = 0: m = 1, a padded copy).  The same call with
 * (src = dW, ld_src = its row stride, ld_out = H) is the backward: dW_raw = dW * m — no mask tensor is stored. */
int nnl_weight_drop(const float* src, int64_t ld_src, const float* mask, float* out, int64_t ld_out, int64_t rows, int64_t H,
                    uint64_t seed, float p, void* stream);

/* ---- K5d: text generation, LanguageModelNet.predict_from_string (Text.py:655-676): batch 1, one timestep, fp32 --------------
 * One LSTM layer for one token (Text.py:655-676, the T = 1 / B = 1 case of the layer its loop runs): gates = w_ih x + w_hh h + bias
 * (bias [4H] = b_ih + b_hh, pre-summed), torch's gate order i, f, g, o, c_out = f c + i g, h_out = o tanh(c_out).  One wave per hidden
 * unit streams its four gate rows with 16-byte loads; a plain launch, no synchronisation between workgroups.  w_ih [4H, ldi] and
 * w_hh [4H, ldh] hold zeros in columns >= I / >= H; ldi and ldh must be multiples of 4 floats (a 1150-float row is not 16-byte
 * aligned on odd rows) and cover I / H, and w_ih, w_hh, x, h must be 16-byte aligned: anything else is NNL_ERR_INVALID_ARG and
 * nothing is launched.  x [ldi] and h [ldh] are zero-padded vectors; h_out [>= H] and c_out [>= H]: only entries < H are written.
 * h_out must not alias h (every wave reads all of h); c_out may alias c.  x == NULL: the input is row tokens[pos] of emb [V, ld_emb]
 * (entries < I; ld_emb >= I, any alignment), the id read on the device; an id outside [0, V) reads as a zero row. */
int nnl_lstm_cell_b1(const float* w_ih, int64_t ldi, const float* w_hh, int64_t ldh, const float* bias, const float* x,
                     const float* emb, int64_t ld_emb, const int64_t* tokens, int64_t pos, int64_t V, const float* h,
                     const float* c, float* h_out, float* c_out, int64_t I, int64_t H, void* stream);
/* The rest of one generated token (Text.py:655-676, lines 667-672): logits l = emb [V, ld_emb] h (the tied decoder; h [E], ld_emb
 * a multiple of 4 floats, emb 16-byte aligned), p = softmax(l) over ALL V entries, entries < n_special excluded from the choice,
 * the k largest p in descending order (ties: lower index), fp32 partial sums c_1 .. c_k taken sequentially, and the seeded draw
 * slot j = #{ m in 1..k-1 : c_m <= u[step] * c_k }: tokens[pos + 1] = index of slot j.  Optional outputs: top_probs [*, k] and
 * top_indices [*, k] get row `step`; logits_out [V] (debug) gets the logits, which otherwise never leave LDS.  Two launches (slices
 * of 64 vocabulary rows, then one workgroup that merges them); fixed-order sums, bitwise repeatable.  1 <= k <= 64,
 * k <= V - n_special; V <= 262 144 and ld_emb <= 8192 (NNL_ERR_UNSUPPORTED above). */
size_t nnl_lm_next_token_workspace_bytes(int64_t V, int64_t k);
int nnl_lm_next_token(const float* emb, int64_t ld_emb, const float* h, int64_t V, int64_t E, int64_t k, int64_t n_special,
                      const float* u, int64_t step, int64_t* tokens, int64_t pos, float* top_probs, int64_t* top_indices,
                      float* logits_out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- K5c: attention pooling of TextClassificationDecoder (Text.py:575-609), everything after attn1 ----------------------
 * h = relu(attn1(enc_out)) [T,B,A], w2 [A] and b2 [1] (device: attn2's weight and bias), enc_out [T,B,E], x [B,T] int64 tokens:
 *   s[t,b] = h[t,b,:].w2 + b2;  attn[:,b] = softmax of s[:,b] over the positions with x[b,t] != pad_token (the reference's
 *   softmax -> mask -> renormalise, Text.py:598-601, up to rounding);  pooled[b,:] = sum_t attn[t,b] enc_out[t,b,:] (:604-605).
 * A column with no non-pad token is NaN in attn and pooled (the reference's 0/0).  Backward, given dpooled [B,E] and dattn [T,B]
 * (NULL = 0): g = enc_out.dpooled + dattn, c[b] = sum_t attn g, dlogit = attn (g - c); denc = attn dpooled (written, not
 * accumulated), dh = dlogit w2, dw2 = sum dlogit h, *db2 = sum dlogit.  Every sum has a fixed order (bitwise repeatable, no float
 * atomics); `counters`: >= B + 1 int32 that are zero at rest and are left zero (nnl_conv2d_tile_counters' buffer fits); the
 * workspace (16-byte aligned) serves both directions. */
size_t nnl_attn_pool_workspace_bytes(int64_t T, int64_t B, int64_t E, int64_t A);
int nnl_attn_pool_fwd(const float* h, const float* w2, const float* b2, const float* enc_out, const int64_t* x, int64_t pad_token,
                      float* attn, float* pooled, int64_t T, int64_t B, int64_t E, int64_t A, void* workspace, size_t workspace_bytes,
                      int32_t* counters, int64_t n_counters, void* stream);
int nnl_attn_pool_bwd(const float* h, const float* w2, const float* enc_out, const float* attn, const float* dpooled,
                      const float* dattn, float* dh, float* denc, float* dw2, float* db2, int64_t T, int64_t B, int64_t E, int64_t A,
                      void* workspace, size_t workspace_bytes, int32_t* counters, int64_t n_counters, void* stream);

/* ---- K9: image augmentation of the classification Transform (Applications/Vision.py:449-507), everything after decode ------
 * One fp32 NHWC minibatch out [bs, sz_h, sz_w, 3] from a uint8 arena that holds every image of a dataset back to back (HWC, RGB);
 * desc[i] = {byte offset, H, W} of image i (int64: the arena may exceed 2 GB), params[b] = what Transform.__call__ drew for sample
 * b.  Per output pixel, the reference's chain run backwards (Vision.py:449-507): undo np.rot90(img, rot) (:493) and np.fliplr
 * (:492); apply the inverse map m of cv2.warpAffine(getRotationMatrix2D(...), borderMode=BORDER_REFLECT) (:488-489): source
 * (m[0] x + m[1] y + m[2], m[3] x + m[4] y + m[5]), bilinear over its four integer taps, each tap index reflected on its own
 * (fedcba|abcdefgh|hgfedcb, any distance); each tap is a pixel of cv2.resize(crop, (sz_w, sz_h), INTER_LINEAR) (:484): source
 * coordinate (o + 0.5) (L_src / sz) - 0.5, two taps per axis clamped to the crop; the crop window (:469-481) is read from the
 * arena as float(v) / 255.0f (open_image, :54-61).  Neither the resized nor the warped image is ever written.  Unlike cv2.warpAffine
 * the source coordinates are NOT rounded to 1/32 pixel.  Every source index is finally clamped into its image and into the arena:
 * no table can make the kernel read outside [arena, arena + arena_bytes).
 * lighting != 0 (the training transform): the geometric pass also writes per-workgroup channel sums to the workspace and a second
 * launch adds them in a fixed order (no float atomics: bitwise repeatable), applies clip((x - mu) cont + bal + mu, 0, 1) with mu
 * the per-channel mean of the sample's transformed image (:496-498) to every sample without NNL_IMAGE_AUG_NO_LIGHTING, then
 * (x - mean) / std (:504), in place.  lighting == 0 (the eval transform): one launch, normalised in the geometric pass.
 * mean_std: HOST pointer to {mean[3], std[3]}, NULL = no normalisation (stats=None). */
typedef struct {
  int64_t offset;        /* byte offset of pixel (0, 0), channel 0 in the arena */
  int64_t H, W;
} nnl_image_desc_t;
enum { NNL_IMAGE_AUG_NO_WARP = 1, NNL_IMAGE_AUG_FLIP = 2, NNL_IMAGE_AUG_NO_LIGHTING = 4 };
typedef struct {
  int64_t image;                              /* row of desc */
  int32_t crop_y, crop_x, crop_h, crop_w;     /* crop window in the image (the whole image for crop_type None) */
  float m[6];                                 /* inverse rotate-zoom map (ignored with NNL_IMAGE_AUG_NO_WARP) */
  int32_t flags;                              /* NNL_IMAGE_AUG_* */
  int32_t rot;                                /* k of np.rot90, 0..3 (1 and 3 need sz_h == sz_w) */
  float bal, cont;
} nnl_image_aug_param_t;                      /* 64 bytes */
size_t nnl_image_aug_workspace_bytes(int64_t bs, int64_t sz_h, int64_t sz_w);
int nnl_image_aug(const uint8_t* arena, int64_t arena_bytes, const nnl_image_desc_t* desc, int64_t n_images,
                  const nnl_image_aug_param_t* params, int64_t bs, int64_t sz_h, int64_t sz_w, const float* mean_std, int lighting,
                  float* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- K10: detection minibatch — TransformBBox.__call__ (Applications/Vision.py:559-603) and AspectRatioCollater (:758-812) -------
 * One padded minibatch from the arena / descriptor table of K9, in ONE launch: out fp32 NHWC [bs, Hp, Wp, 3], boxes fp32 [bs, N, 4],
 * cats int64 [bs, N].  image_mean[i] = the three channel means of image i as float(v) / 255 (np.mean(img, axis=(0, 1)), :576): they
 * depend on the image alone, so the caller computes them once from exact integer sums and lighting needs no workspace and no second
 * launch.  params[k] = what TransformBBox drew for sample k and what the collater derived from it; row_jit, col_jit and rand_scale are
 * those of the first sample of the minibatch (:764-766).
 * Image, per output pixel (oy, ox) of sample k, the chain run backwards: y = oy - row_jit, x = ox - col_jit; outside [0, rh) x [0, rw)
 * the value is 0.0f, the zeros of the collater written after normalisation (:780-781, :793-796).  Inside: the taps of
 * cv2.resize(img, (rw, rh), INTER_LINEAR) (:774) from the H x W source — source coordinate (o + 0.5) (L_src / r) - 0.5, two taps per axis
 * clamped, no antialiasing; with NNL_IMAGE_AUG_FLIP source column c is W - 1 - c (np.fliplr before the resize, :583-584); each tap
 * is u = float(v) / 255.0f (open_image, :54-61), lit unless NNL_IMAGE_AUG_NO_LIGHTING as clip((u - mu_c) cont + bal + mu_c, 0, 1)
 * (:576-577), then (. - mean_c) / std_c (:580); the four taps are interpolated last.  Every source index is clamped into its image
 * and into the arena: no table can make the kernel read outside [arena, arena + arena_bytes).
 * Boxes, slot j of sample k: j < box_count: box box_first + j of the float64 arena [n_boxes, 4] (xmin, ymin, xmax, ymax), in FLOAT64
 * and without fused multiply-adds, as numpy does it: flipped x (W - xmax, W - xmin) (:598-600), (b scale) rand_scale (:776), + col_jit
 * on x and + row_jit on y (:782-784), then ONE rounding to fp32 (:805); its category from cat_arena.  Otherwise box and category are -1
 * (:801-802, :808-809).  The box range is clamped into the arenas.  The box work rides in extra workgroups of the image launch.
 * mean_std: HOST pointer to {mean[3], std[3]}, NULL = no normalisation.  bs in [1, 65535], Hp and Wp in [1, 16384], N in [1, 2^20],
 * row_jit and col_jit >= 0. */
typedef struct {
  int64_t image;                 /* row of desc and of image_mean */
  int64_t box_first;             /* first box of the image in box_arena / cat_arena */
  int32_t box_count;
  int32_t rh, rw;                /* resized size: int(H scale rand_scale), int(W scale rand_scale) */
  int32_t flags;                 /* NNL_IMAGE_AUG_FLIP, NNL_IMAGE_AUG_NO_LIGHTING */
  float bal, cont;
  double scale;                  /* the image's own scale (get_AspectRatioScale) */
} nnl_detect_aug_param_t;        /* 48 bytes */
int nnl_detect_aug(const uint8_t* arena, int64_t arena_bytes, const nnl_image_desc_t* desc, int64_t n_images, const float* image_mean,
                   const double* box_arena, const int64_t* cat_arena, int64_t n_boxes, const nnl_detect_aug_param_t* params,
                   int64_t bs, int64_t Hp, int64_t Wp, int64_t N, int64_t row_jit, int64_t col_jit, double rand_scale,
                   const float* mean_std, float* out, float* boxes, int64_t* cats, void* stream);

/* ---- K16: the resident image set — channel statistics and resample of uint8 arenas (device_data.ImageStore) ------------------
 * Arena and descriptor convention of K9: uint8 HWC RGB images back to back, desc[i] = {byte offset, H, W}; offsets are arbitrary
 * (no alignment is assumed).  Both entries validate every descriptor row they use IN THE KERNEL against the arena size (offset >= 0,
 * 1 <= H, W <= 2^24, offset + 3 H W <= bytes) and read or write nothing for a row that fails; no byte outside [arena, arena +
 * arena_bytes) is read, also not by the 16-byte loads at an image's unaligned ends.  Both are stream-ordered and do not synchronise.
 *
 * nnl_image_stats (get_stats, Applications/Vision.py:93-118; the per-image means of TransformBBox's lighting, :576): out uint64
 * [count, 6], row k for image first + k: out[k][c] = sum of the raw byte values of channel c, out[k][3 + c] = sum of their squares.
 * Integer arithmetic only (uint32 per load, uint64 above, one 64-bit integer atomic per workgroup and sum): the result is exact and
 * does not depend on the order of addition or on how an image is split.  An image is cut into NNL_IMAGE_STATS_TILE_BYTES-byte tiles
 * that `split` workgroups take in turn (split = twice the tiles of the arena's mean image, at most 256), so one large image does not
 * run on one CU.  The entry zeroes `out`.  Status: the return value covers the host-visible arguments (null pointers, an empty arena,
 * a window outside [0, n_images)) and the launch; a descriptor row that fails the validation above is reported in its row of `out`,
 * all six entries = NNL_IMAGE_STATS_INVALID (no image reaches that value: 255^2 2^48 < 2^64 - 1), and the caller must raise
 * (ops.image_stats does).
 *
 * nnl_image_resize_u8 (save_resized, Vision.py:64-91; ImageStore's presize): image i of src is resampled to the H, W of dst_desc[i]
 * and written at dst_desc[i].offset.  THE DEFINITION, per destination pixel (oy, ox) and channel, Hs x Ws -> Hd x Wd, every operation
 * rounded to fp32 on its own (compiled without floating-point contraction):
 *   sy = (float)((double)Hs / (double)Hd);  fy = ((float)oy + 0.5f) * sy - 0.5f;  y0 = floor(fy);  wy = fy - y0;
 *   ya = clamp(y0, 0, Hs - 1);  yb = clamp(y0 + 1, 0, Hs - 1);            and sx, fx, x0, wx, xa, xb likewise from Ws, Wd, ox
 *   top = v[ya][xa] * (1 - wx) + v[ya][xb] * wx;   bot = v[yb][xa] * (1 - wx) + v[yb][xb] * wx;      v = (float)byte
 *   dst = (uint8) min(max(rintf(top * (1 - wy) + bot * wy), 0), 255)                                  rintf: ties to even
 * i.e. the half-pixel taps of K9's resize (iaug_resize_scale, iaug_resize_taps) and its interpolation order (iaug_resized_pixel)
 * without the division by 255; no antialiasing.  Hd = Hs and Wd = Ws reproduces the source bytes.  It is NOT cv2.resize on uint8
 * images: OpenCV interpolates those with 11-bit fixed-point weights, and its bytes differ from these by +-1 in places; OpenCV is
 * not available where this library is tested, so no claim is made against it.  A pair of rows of which either fails the validation
 * is skipped (nothing written). */
#define NNL_IMAGE_STATS_TILE_BYTES 16384
#define NNL_IMAGE_STATS_INVALID 0xffffffffffffffffull
int nnl_image_stats(const uint8_t* arena, int64_t arena_bytes, const nnl_image_desc_t* desc, int64_t n_images, int64_t first,
                    int64_t count, uint64_t* out, void* stream);
int nnl_image_resize_u8(const uint8_t* src_arena, int64_t src_bytes, const nnl_image_desc_t* src_desc, uint8_t* dst_arena,
                        int64_t dst_bytes, const nnl_image_desc_t* dst_desc, int64_t n_images, void* stream);

/* ---- K8: fused multi-tensor Optimizer.step ------------------------------------------------------------------------
 * Replaces Optimizer.step (General/Optimizer.py:58-70): decoupled weight decay X *= 1 - wd_g*lr_g (:60-67), global-norm
 * clip (:54-56, torch.nn.utils.clip_grad_norm_) and the torch.optim SGD(momentum) / Adam update (General/Learner.py:17-19)
 * for all parameter tensors at once.  `tensors` is a DEVICE array of n_tensors descriptors; param / grad / state arrays of
 * one tensor share one dense layout and are indexed flat.  grad == NULL: decay only.  lr and decay (= 1 - wd*lr, or 1)
 * are per tensor (layer-group learning rates).  (chunk_tensor[c], chunk_off[c]) maps workgroup c to a piece of
 * nnl_optim_chunk_elems() elements.  kind 0 = SGD (state1 = momentum buffer, zero before the first step; momentum may be
 * 0), kind 1 = Adam (state1 = exp_avg, state2 = exp_avg_sq).  `hyper` is a DEVICE array of 8 floats {momentum (SGD) or
 * 1-beta1 (Adam), beta1, beta2, eps, bc1 = 1-beta1^t, sqrt(bc2) = sqrt(1-beta2^t), clip max_norm, 1-beta2} (1-beta rounded once from
 * double by the caller, as torch.optim.Adam's scalar arguments are): hyper-parameters are read from
 * memory so that a captured hipGraph of the whole step can be replayed with new values.  use_clip != 0: gradients are
 * scaled by min(1, max_norm/(||g||_2 + 1e-6)) (also written back to .grad, as clip_grad_norm_ does; a NaN norm gives a NaN
 * coefficient, an Inf norm the coefficient 0, as there); clip_workspace: n_chunks + 2 floats, [0] = coefficient, [1] = total norm on
 * return. */
typedef struct {
  float* param;
  float* grad;
  float* state1;
  float* state2;
  int64_t numel;
  float lr;
  float decay;
} nnl_optim_tensor_t;
int64_t nnl_optim_chunk_elems(void);
/* tensors[i].lr / .decay = dyn[2i] / dyn[2i+1] (i < n), hyper[0..8) = dyn[2n ..): the per-step values of a REPLAYED step, patched into the
 * table after its captured upload (see csrc/optim.hip). */
int nnl_optim_patch(nnl_optim_tensor_t* tensors, float* hyper, const float* dyn, int64_t n, void* stream);
int nnl_optim_step(const nnl_optim_tensor_t* tensors, const int32_t* chunk_tensor, const int64_t* chunk_off,
                   int64_t n_chunks, int kind, const float* hyper, int use_clip, float* clip_workspace, void* stream);

/* ---- K12: time-series features of the structured-data workflow ------------------------------------------------------
 * Both entries read n rows ALREADY SORTED by (group, time ascending), 1 <= n < 2^31: t int64 [n] (nanoseconds of a timestamp, or a
 * plain integer index), head uint8 [n] = 1 on the first row of every group (row 0 counts as one whatever it holds).  Outputs are
 * float64.  Arguments are validated before any HIP call.
 *
 * nnl_seg_event_gaps replaces the per-row Python loops of get_TimeBeforeAfter (Applications/StructuredData.py:482-519, once per
 * group and direction): before[i] = (double)(t[i] - t[j]) / timescale with j the last row strictly before i in i's group with
 * event[j] == 1, NaN if there is none; after[i] = (double)(t[j] - t[i]) / timescale with j the next such row strictly after i.  A
 * row's own event does not count for that row (:499-502 append before they update last_event).  It also writes seg_start[i] and
 * seg_end[i], int32 [n]: the first and the last row of i's group, which nnl_seg_rolling reads.  Three launches, no workspace: the
 * scan's tile carries (NNL_SEG_SCAN_TILE rows per tile) pass through the output arrays.
 *
 * nnl_seg_rolling replaces the per-group pandas rolling calls of get_RollingStats (:556-607): x float64 [C, n] (column c at
 * x + c n), out float64 [popcount(stat_mask), C, n], the requested statistics in the fixed order of the NNL_ROLL_* bits.  Exactly one
 * of count_window > 0 (rows) and span > 0 (in t's units) is given.  The window of row i never leaves i's group [seg_start[i],
 * seg_end[i]] and is, backward (forward == 0): rows j <= i with t[j] > t[i] - span (pandas' closed='right'), or rows
 * [max(seg_start, i - w + 1), i]; forward (forward == 1): rows j >= i with t[j] < t[i] + span (the reference's reverse_datetime,
 * :521-528, :572-574), or rows [i, min(seg_end, i + w - 1)].  NaN entries are skipped; Count is the number of non-NaN entries; Sum,
 * Min, Max and Mean are NaN when Count < 1; Std has ddof = 1 and is NaN when Count < 2 (min_periods of :580-596).  One thread per
 * (row, column) adds its window oldest to newest in fp64 (Std: a second walk over (x - mean)^2): O(window) per output. */
#define NNL_SEG_SCAN_TILE 1024
enum { NNL_ROLL_SUM = 1, NNL_ROLL_MIN = 2, NNL_ROLL_MAX = 4, NNL_ROLL_MEAN = 8, NNL_ROLL_STD = 16, NNL_ROLL_COUNT = 32 };
int nnl_seg_event_gaps(const int64_t* t, const uint8_t* head, const uint8_t* event, int64_t n, double timescale, double* before,
                       double* after, int32_t* seg_start, int32_t* seg_end, void* stream);
int nnl_seg_rolling(const int64_t* t, const int32_t* seg_start, const int32_t* seg_end, const double* x, int64_t n, int64_t C,
                    int64_t count_window, int64_t span, int forward, int stat_mask, double* out, void* stream);

/* ---- K13: association measures of the structured-data EDA (Applications/StructuredData.py:235-428) -------------------------
 * Columns live on the device, one after another: codes int32 [V, n] (category codes in [0, card[v]), -1 = missing; a code outside
 * that range counts as missing too), vals float64 [V, n] (NaN = missing; no +-inf) with shift float64 [V] on the device (the
 * caller's centre of each column, its nanmean: every sum is taken over vals - shift).  1 <= n < 2^31.  card, pair_x, pair_y and
 * offsets are HOST arrays: pair p associates column pair_x[p] with column pair_y[p].  Every entry validates its arguments before
 * any HIP call (null pointers, n, P >= 1, pair indices inside [0, V), offsets against the cardinalities) and cuts the pair list
 * into chunks that travel to the kernels as arguments; a workgroup stages a tile of NNL_ASSOC_ROW_TILE rows of a chunk's columns in
 * LDS once and walks the chunk's pairs over it.
 *
 * nnl_assoc_contingency: tables uint32 [offsets[P]], the table of pair p row-major [card[x], card[y]] at offsets[p]
 * (offsets[0] = 0, at most 2^26 cells per table): the number of rows with both codes present.  The entry zeroes the tables.
 * Tables of at most NNL_ASSOC_LDS_CELLS cells are counted in LDS per workgroup and flushed once, larger ones with global atomics;
 * the result is exact either way.  Route note: "assoc_contingency:lds=<pairs>,global=<pairs>,chunks=<launches>".
 * nnl_assoc_table_stats: out float64 [P, 6] = n, non-empty rows, non-empty columns, H_X, H_Y (natural log, from the marginals) and
 * H_XY, which adds -1e-20 log(1e-20) for every empty cell of the non-empty rows x non-empty columns (the reference's clamp).
 * Fixed reduction order: the same table gives the same bits.
 *
 * nnl_assoc_cat_cont: x indexes codes [Vc, n], y indexes vals [Vy, n]; rows with a code and a non-NaN value count.
 * out float64 [P, 6] = n, non-empty categories, correlation ratio sqrt((sum_c n_c (mean_c - mean)^2 / n) / var_ddof1(y)),
 * max_c |mean_c - mean| / std_ddof1(y), min and max of y - shift.  Per-category sums are fp64 atomics (LDS for up to
 * NNL_ASSOC_MOMENT_LDS_CELLS categories, else global): the last bits may differ between calls.  The workspace
 * (nnl_assoc_cat_cont_workspace_bytes, 0 for invalid arguments) is zeroed by the entry.
 *
 * nnl_assoc_cont_cont: out float64 [P, 4] = n, degenerate (1.0 if n = 0 or either column holds one distinct value on the pair's
 * rows, else 0.0), |corr(x, y)|, and, with_abs = 1, max |corr| over (x, y), (x, |y - my|), (|x - mx|, y), (|x - mx|, |y - my|) with
 * mx, my the means over the pair's rows (a second pass over the rows), else NaN.  |x - mx| counts as constant, and its two
 * correlations are skipped, when its centred sum of squares is at most n (2^-26 mean|x - mx|)^2.  Both values are NaN for a
 * degenerate pair.  No atomics: at most NNL_ASSOC_MAX_GROUPS per-workgroup partial sums per pair, added in a fixed order. */
#define NNL_ASSOC_ROW_TILE 1024
#define NNL_ASSOC_LDS_CELLS 6144
#define NNL_ASSOC_MOMENT_LDS_CELLS 1152
#define NNL_ASSOC_MAX_GROUPS 256
int nnl_assoc_contingency(const int32_t* codes, const int32_t* card, int64_t V, int64_t n, const int32_t* pair_x, const int32_t* pair_y,
                          const int64_t* offsets, int64_t P, uint32_t* tables, void* stream);
int nnl_assoc_table_stats(const uint32_t* tables, const int32_t* card, int64_t V, const int32_t* pair_x, const int32_t* pair_y,
                          const int64_t* offsets, int64_t P, double* out, void* stream);
size_t nnl_assoc_cat_cont_workspace_bytes(const int32_t* card, int64_t Vc, const int32_t* pair_x, int64_t P);
int nnl_assoc_cat_cont(const int32_t* codes, const int32_t* card, int64_t Vc, const double* vals, const double* shift, int64_t Vy,
                       int64_t n, const int32_t* pair_x, const int32_t* pair_y, int64_t P, void* workspace, size_t workspace_bytes,
                       double* out, void* stream);
size_t nnl_assoc_cont_cont_workspace_bytes(int64_t n, int64_t P);
int nnl_assoc_cont_cont(const double* vals, const double* shift, int64_t V, int64_t n, const int32_t* pair_x, const int32_t* pair_y,
                        int64_t P, int with_abs, void* workspace, size_t workspace_bytes, double* out, void* stream);

/* ---- K14: detection evaluation (Applications/pycocotools/cocoeval.py:171-198, 243-428; Applications/Vision.py:1696-1747) ------
 * A group is an (image, category) pair with at least one detection or one ground truth; groups are sorted by (category, image id),
 * so group g owns detections [dt_off[g], dt_off[g+1]) and ground truths [gt_off[g], gt_off[g+1]) and category k owns groups
 * [cat_grp_off[k], cat_grp_off[k+1]) and detections [cat_dt_off[k], cat_dt_off[k+1]).  Every array but the parameter lists
 * (thresholds, area ranges, maxDets: HOST arrays, validated and passed to the kernels as arguments) is a DEVICE array.  The entries
 * validate sizes and the parameter lists before any HIP call; the CALLER checks, before the upload, that every offset array is
 * non-decreasing, starts at 0 and ends at the length of what it indexes, and that order / dt_rank are in range.
 * Limits: T <= NNL_DET_EVAL_MAX_T thresholds, A <= NNL_DET_EVAL_MAX_A area ranges, M <= NNL_DET_EVAL_MAX_M maxDets entries,
 * R <= NNL_DET_EVAL_MAX_R recall thresholds, fewer than 2^31 groups / detections / ground truths; none on the size of a group.
 *
 * nnl_det_coco_match (cocoeval.py:171-198 computeIoU, :243-321 evaluateImg): dt_box / gt_box float64 [., 4] = [x, y, w, h]; the
 * detections of a group sorted by score descending (stable) and cut to maxDets[-1] by the caller; gt_area the annotation's area;
 * gt_flags bit 0 = iscrowd, bit 1 = ignore.  area_rng float64 [A, 2].  The overlap of detection D and ground truth G, fp64, one
 * operation at a time: w = min(D.x + D.w, G.x + G.w) - max(D.x, G.x), h likewise, 0 if w <= 0 or h <= 0, else
 * w h / (crowd ? D.w D.h : D.w D.h + G.w G.h - w h); computed once per group for all A x T matchers, each of which runs the
 * reference's greedy loop in a lane of its own (one wave per group).  A group needs D G + ceil((A T + A) G / 8) doubles: in LDS
 * up to NNL_DET_EVAL_LDS_DOUBLES (scr_off[g] = -1), else at scratch + scr_off[g] doubles (scr_off int64 [NG]).  Outputs:
 * dtm int32 [A, T, Nd] = position of the matched ground truth in its group + 1, or 0; dtig uint8 [A, T, Nd] the detection's
 * ignore bit; npig int32 [A, NG] the group's ground truths that are not ignored in range a; status int32 [1] = 1 if a group's
 * buffer did not fit where scr_off put it (the group is skipped: the caller must raise).
 * nnl_det_coco_accumulate (cocoeval.py:323-428): one workgroup per (k, a, m, t).  order int32 [Nd]: the detections of each category
 * in stable descending-score order over (group, rank); dt_rank int32 [Nd] the rank inside the group; entry m keeps rank <
 * max_dets[m].  precision, scores float64 [T, R, K, A, M], recall float64 [T, K, A, M]; a (k, a) block without a group or without a
 * counting ground truth is -1.  rec_thrs must ascend.
 * nnl_det_map_match (Vision.py:1696-1728): pr_box / gt_box float32 [., 4] min-max boxes; fp32 jaccard in retinanet.jaccard's
 * operation order; every ground truth marks its first arg-max prediction in correct uint8 [T, Np] (zeroed by the entry) where the
 * overlap, widened to fp64, is > thrs[t].
 * nnl_det_map_integrate (Vision.py:1730-1747): one workgroup per (category, threshold); order int32 [Np] the predictions of each
 * category by descending score (ties in any order: the entry puts the correct ones of a run of equal scores first), score float64
 * [Np], ntrue int64 [C].  out float64 [T, C] = sum of the max-smoothed precision at the correct positions / ntrue (0 / 0 = NaN).
 * The workspace holds T Np doubles.  Fixed summation order: the same inputs give the same bits. */
#define NNL_DET_EVAL_MAX_T 16
#define NNL_DET_EVAL_MAX_A 8
#define NNL_DET_EVAL_MAX_M 8
#define NNL_DET_EVAL_MAX_R 128
#define NNL_DET_EVAL_LDS_DOUBLES 2048
int nnl_det_coco_match(const int32_t* dt_off, const int32_t* gt_off, const double* dt_box, const double* gt_box, const double* gt_area,
                       const uint8_t* gt_flags, const int64_t* scr_off, int64_t NG, int64_t Nd, int64_t Ng, const double* iou_thrs, int64_t T,
                       const double* area_rng, int64_t A, void* scratch, size_t scratch_bytes, int32_t* dtm, uint8_t* dtig, int32_t* npig,
                       int32_t* status, void* stream);
int nnl_det_coco_accumulate(const int32_t* cat_grp_off, const int32_t* cat_dt_off, const int32_t* order, const int32_t* dt_rank,
                            const double* dt_score, const int32_t* dtm, const uint8_t* dtig, const int32_t* npig, int64_t K, int64_t NG,
                            int64_t Nd, int64_t T, int64_t A, const int32_t* max_dets, int64_t M, const double* rec_thrs, int64_t R,
                            double* precision, double* scores, double* recall, void* stream);
int nnl_det_map_match(const int32_t* pr_off, const int32_t* gt_off, const float* pr_box, const float* gt_box, int64_t NG, int64_t Np,
                      int64_t Ng, const double* thrs, int64_t T, uint8_t* correct, void* stream);
size_t nnl_det_map_integrate_workspace_bytes(int64_t Np, int64_t T);
int nnl_det_map_integrate(const int32_t* cat_pr_off, const int32_t* order, const double* score, const uint8_t* correct, const int64_t* ntrue,
                          int64_t C, int64_t Np, int64_t T, void* workspace, size_t workspace_bytes, double* out, void* stream);

/* ---- K17: tokeniser and vocabulary of the text workflow (Applications/Text.py:28-122) ----------------------------------------
 * A corpus is ONE resident byte buffer: bytes uint8 [B], 0 <= B < 2^31, and text_off int64 [n+1] (n >= 1, text_off[0] = 0,
 * non-decreasing, text_off[n] = B; the CALLER checks that before the upload), text j being bytes [text_off[j], text_off[j+1]).  No
 * token crosses a text boundary and no rule looks across one.  mode NNL_TEXT_MODE_GRAMMAR cuts by the byte grammar of DESIGN.md
 * section 8 (what Tokenizer.proc_text / spacy_tok and do_caps do, Text.py:40-41, 58-67, 69-75) and compares, hashes and returns tokens
 * with A-Z lowered; NNL_TEXT_MODE_SPLIT cuts maximal runs of non-whitespace bytes and lowers nothing (what numericalize reads,
 * Text.py:95-122).  A token is a record (tok_start int32, tok_len int32); the pseudo-token t_up has tok_len = NNL_TEXT_TUP_LEN and the
 * start of the token it precedes, and stands for the four bytes "t_up" wherever a token's bytes are read.  Every pointer is a
 * DEVICE pointer; the caller owns every buffer; arguments are validated before any HIP call.  Integer atomics only, every phase its
 * own launch, no workgroup waits for another, every loop is bounded by B, T, n or the table's capacity.
 *
 * nnl_text_token_count (replaces the token lists of Text.py:77-93 as a count): per-tile token counts (tiles of NNL_TEXT_TILE bytes,
 * t_up included), then their exclusive scan by one workgroup: tile_base int64 [cdiv(B, NNL_TEXT_TILE) + 1], the last entry the total
 * T, which the host reads once to size the outputs of nnl_text_token_fill.
 * nnl_text_token_fill (Text.py:40-41, 69-75): tok_start, tok_len int32 [T] in byte order, and text_tok_off int64 [n+1]: text j owns
 * tokens [text_tok_off[j], text_tok_off[j+1]).  T must be the total nnl_text_token_count gave for the same bytes, offsets and mode.
 * nnl_text_token_hash (the hashing inside collections.Counter, Text.py:113): keys uint64 [T] = (h(seed, the token's lowered bytes)
 * AND hash_mask), a zero result replaced by hash_mask's lowest set bit: key 0 means "empty slot".  hash_mask != 0.
 * nnl_text_vocab_insert (Counter, Text.py:112-113): open addressing, linear probing from a slot derived from the key, in table_key
 * uint64 [cap], table_count int32 [cap], table_first int32 [cap]; cap a power of two in [16, 2^30].  reset != 0 clears the table and
 * status first (a launch of its own).  One 64-bit compare-and-swap per probe step; on a hit or a win the slot's count is incremented,
 * its first token index atomicMin-ed with t, and tok_slot[t] = slot.  A token that finds no slot in cap steps sets bit
 * NNL_TEXT_STATUS_OVERFLOW of status int32 [1] and gets tok_slot[t] = -1.  Which of two keys sharing a home slot gets it depends on
 * arrival order, so slot NUMBERS differ between calls; counts and first indices do not.
 * nnl_text_vocab_verify: every token with a slot compares its length and lowered bytes with token table_first[slot], in the token
 * stream ftok_start / ftok_len / fbytes that slot's first index refers to (the same stream for a corpus's own vocabulary);
 * mismatches int32 [1] is incremented per differing token (the caller zeroes it).  Zero mismatches = every slot holds ONE string.
 * nnl_text_vocab_compact: the occupied slots as rows (slot, count, first, tok_start[first], tok_len[first]) of list int32 [max_rows, 5]
 * in no particular order, n_rows int32 [1] (zeroed by the caller) their number; rows beyond max_rows are counted, not written.
 * nnl_text_vocab_assign (the stoi dict of Text.py:114-117): slot_id int32 [cap] = 0 everywhere, then slot_id[slots[k]] = ids[k]
 * for k < K (slots, ids int32 [K]; two launches).
 * nnl_text_vocab_lookup (the defaultdict lookups of Text.py:119-120 for a GIVEN stoi): the vocabulary's strings are a token stream of
 * their own (vbytes, vtok_start, vtok_len), inserted and verified by the entries above.  Data token t probes with keys[t]: an empty
 * slot or cap steps give tok_slot[t] = -1; a slot with the same key gives that slot if the token's lowered bytes equal the
 * vocabulary string table_first[slot], else -1 (the vocabulary's keys are distinct once verified, so no other slot can hold it).
 * nnl_text_ids_write (Text.py:120, :144): ids int64 [T], ids[p] = tok_slot[t] < 0 ? 0 : slot_id[tok_slot[t]], p = t, or with
 * reverse != 0 the mirror position of t inside its text. */
#define NNL_TEXT_TILE 1024
#define NNL_TEXT_TUP_LEN (-1)
enum { NNL_TEXT_MODE_GRAMMAR = 0, NNL_TEXT_MODE_SPLIT = 1 };
enum { NNL_TEXT_STATUS_OVERFLOW = 1 };
int nnl_text_token_count(const uint8_t* bytes, int64_t B, const int64_t* text_off, int64_t n, int mode, int64_t* tile_base, void* stream);
int nnl_text_token_fill(const uint8_t* bytes, int64_t B, const int64_t* text_off, int64_t n, int mode, const int64_t* tile_base, int64_t T,
                        int32_t* tok_start, int32_t* tok_len, int64_t* text_tok_off, void* stream);
int nnl_text_token_hash(const uint8_t* bytes, int64_t B, const int32_t* tok_start, const int32_t* tok_len, int64_t T, int mode,
                        uint64_t seed, uint64_t hash_mask, uint64_t* keys, void* stream);
int nnl_text_vocab_insert(const uint64_t* keys, int64_t T, uint64_t* table_key, int32_t* table_count, int32_t* table_first, int64_t cap,
                          int reset, int32_t* tok_slot, int32_t* status, void* stream);
int nnl_text_vocab_verify(const uint8_t* bytes, int64_t B, const int32_t* tok_start, const int32_t* tok_len, const int32_t* tok_slot,
                          int64_t T, int mode, const uint8_t* fbytes, int64_t FB, const int32_t* ftok_start, const int32_t* ftok_len,
                          int64_t FT, int fmode, const int32_t* table_first, int64_t cap, int32_t* mismatches, void* stream);
int nnl_text_vocab_compact(const uint64_t* table_key, const int32_t* table_count, const int32_t* table_first, int64_t cap,
                           const int32_t* tok_start, const int32_t* tok_len, int64_t T, int32_t* list, int64_t max_rows, int32_t* n_rows,
                           void* stream);
int nnl_text_vocab_assign(const int32_t* slots, const int32_t* ids, int64_t K, int32_t* slot_id, int64_t cap, void* stream);
int nnl_text_vocab_lookup(const uint8_t* bytes, int64_t B, const int32_t* tok_start, const int32_t* tok_len, const uint64_t* keys,
                          int64_t T, int mode, const uint8_t* vbytes, int64_t VB, const int32_t* vtok_start, const int32_t* vtok_len,
                          int64_t VT, const uint64_t* table_key, const int32_t* table_first, int64_t cap, int32_t* tok_slot, void* stream);
int nnl_text_ids_write(const int32_t* tok_slot, const int32_t* slot_id, int64_t cap, const int64_t* text_tok_off, int64_t n, int64_t T,
                       int reverse, int64_t* ids, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NNL_H_ */
