"""torch.autograd.Function wrappers around the C ABI of libnnl_hip.so (include/nnl.h).

Each Function is the device-side replacement of one group of eager torch ops in the reference (call sites
cited per class).  Tensors are handed over as raw device pointers + sizes on torch's CURRENT stream; there
is no CPU fallback — a non-CUDA tensor raises NnlError.
"""
import collections
import contextlib
import ctypes
import os
import weakref

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, require_cuda, stream

__all__ = ['mse_loss', 'bce_with_logits', 'fbeta', 'scaled_sigmoid', 'embdotbias', 'index_error_flag', 'raise_if_index_error', 'conv2d', 'to_nhwc', 'from_nhwc', 'linear', 'bn_act', 'concat_pool2d', 'TabularPlan', 'tab_embed_concat', 'embedding_renorm_drop', 'retina_loss', 'image_aug', 'grouped_conv2d', 'se_excite']

_ERR_FLAGS = {}


def _flags(device):
    key = (device.type, device.index)
    if key not in _ERR_FLAGS:
        _ERR_FLAGS[key] = torch.zeros(2, dtype=torch.int32, device=device)
    return _ERR_FLAGS[key]


def index_error_flag(device):
    """Per-device int32 flag that gather kernels set when they meet an out-of-range index (the sample is
    skipped, nothing faults).  Checked without a per-step sync by `raise_if_index_error()`."""
    return _flags(device)[0:1]


def lstm_timeout_flag(device):
    """Its own word next to the index flag: the persistent LSTM kernels store 2 here when their grid barrier times out (a gather
    kernel's plain store of 1 into the index word can then no longer overwrite it)."""
    return _flags(device)[1:2]


def raise_for_flag(code):
    "bit 0: index out of range (torch's nn.Embedding failure); bit 1: persistent-LSTM barrier time-out"
    if code & 2:
        raise _lib.NnlError("the persistent LSTM kernel's grid barrier timed out (results of that step are invalid)")
    if code & 1:
        raise IndexError("index out of range in self")


def raise_if_index_error():
    """One D2H read per call: raises IndexError (torch's nn.Embedding failure) if any gather kernel since the
    last call saw an out-of-range index.  The Learner calls this at the end of every epoch, evaluate() and predict()
    (General/Learner.py `_raise_if_index_error`, which also makes the decision rank-uniform under data parallelism)."""
    for flag in _ERR_FLAGS.values():
        v = flag.tolist()
        code = (1 if v[0] else 0) | (2 if v[1] else 0)
        if code:
            flag.zero_()
            raise_for_flag(code)


def _f32c(t):
    return t.contiguous() if t.dtype == torch.float32 else t.float().contiguous()


def _workspace(nbytes, device, *, floor=False):
    """the scratch buffer a library call asked for (its *_workspace_bytes query): None — a NULL pointer — for zero bytes, unless
    floor=True asks for a minimal buffer instead.  Which of the two a site passes is deliberate and kept per site: the conv entry
    points consider the Winograd kernels only with a non-null workspace; the reductions always got a non-null pointer."""
    if not nbytes and not floor:
        return None
    return torch.empty(max((nbytes + 3) // 4, 1), dtype=torch.float32, device=device)


class _EmbDotBias(torch.autograd.Function):
    """CollabFilterNet.forward (reference Applications/CollabFiltering.py:196-204): four embedding gathers,
    row-wise dot, bias adds and the scaled sigmoid in ONE kernel; backward = the four dense scatter-adds."""

    @staticmethod
    def forward(ctx, x, U, M, bu, bi, lo, hi):
        require_cuda(x, U, M, bu, bi)
        x = x.contiguous()
        if x.dtype != torch.int64:
            x = x.long()
        U, M, bu, bi = _f32c(U), _f32c(M), _f32c(bu), _f32c(bi)
        n, D = x.shape[0], U.shape[1]
        y = torch.empty(n, dtype=torch.float32, device=x.device)
        z = torch.empty(n, dtype=torch.float32, device=x.device)
        has_range = lo is not None
        check(lib.nnl_embdotbias_fwd(ptr(x), ptr(U), ptr(M), ptr(bu), ptr(bi), ptr(y), ptr(z), n, U.shape[0],
                                     M.shape[0], D, int(has_range), float(lo or 0.), float(hi or 0.),
                                     ptr(index_error_flag(x.device)), stream()))
        ctx.save_for_backward(x, U, M, z)
        ctx.rng = (has_range, float(lo or 0.), float(hi or 0.))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, U, M, z = ctx.saved_tensors
        has_range, lo, hi = ctx.rng
        dy = _f32c(dy)
        nu, ni, D = U.shape[0], M.shape[0], U.shape[1]
        flat = torch.empty((nu + ni) * (D + 1), dtype=torch.float32, device=U.device)       # [dU | dM | dbu | dbi]: one fill in C
        dU, dM = flat[:nu * D].view(nu, D), flat[nu * D:(nu + ni) * D].view(ni, D)
        dbu, dbi = flat[(nu + ni) * D:(nu + ni) * D + nu].view(nu, 1), flat[(nu + ni) * D + nu:].view(ni, 1)
        wsb = int(lib.nnl_embdotbias_bwd_workspace_bytes(x.shape[0]))          # sample-order (deterministic) scatter-add
        ws = _workspace(wsb, U.device, floor=True)                              # never a null
        check(lib.nnl_embdotbias_bwd(ptr(x), ptr(U), ptr(M), ptr(z), ptr(dy), ptr(dU), ptr(dM), ptr(dbu), ptr(dbi),
                                     x.shape[0], U.shape[0], M.shape[0], U.shape[1], int(has_range), lo, hi,
                                     ptr(ws), wsb, stream()))
        return None, dU, dM, dbu, dbi, None, None


class _MSE(torch.autograd.Function):
    """nn.MSELoss() (reference General/Learner.py:20, the 'cont' loss): one launch forward, one backward."""

    @staticmethod
    def forward(ctx, pred, target):
        require_cuda(pred, target)
        p, t = _f32c(pred).reshape(-1), _f32c(target).reshape(-1)
        n = p.numel()
        loss = torch.empty((), dtype=torch.float32, device=p.device)
        wsb = int(lib.nnl_mse_workspace_bytes(n))
        ws = _workspace(wsb, p.device)
        check(lib.nnl_mse_fwd(ptr(p), ptr(t), ptr(loss), n, ptr(ws), wsb, stream()))
        ctx.save_for_backward(p, t)
        ctx.shape = pred.shape
        return loss

    @staticmethod
    def backward(ctx, dloss):
        p, t = ctx.saved_tensors
        g = _f32c(dloss).reshape(1)
        dp = torch.empty_like(p)
        check(lib.nnl_mse_bwd(ptr(p), ptr(t), ptr(g), ptr(dp), p.numel(), stream()))
        return dp.view(ctx.shape), None


def mse_loss(pred, target):
    "mean((pred - target)^2) as a 0-dim tensor; gradient with respect to `pred` only (targets are data)"
    return _MSE.apply(pred, target)


class _BCEWithLogits(torch.autograd.Function):
    """nn.BCEWithLogitsLoss() (reference General/Learner.py:20, the 'multi_label' loss): one launch forward, one backward."""

    @staticmethod
    def forward(ctx, input, target):
        require_cuda(input, target)
        x, t = _f32c(input).reshape(-1), _f32c(target).reshape(-1)
        n = x.numel()
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        wsb = int(lib.nnl_bce_logits_workspace_bytes(n))
        ws = _workspace(wsb, x.device)
        check(lib.nnl_bce_logits_fwd(ptr(x), ptr(t), ptr(loss), n, ptr(ws), wsb, stream()))
        ctx.save_for_backward(x, t)
        ctx.shape = input.shape
        return loss

    @staticmethod
    def backward(ctx, dloss):
        x, t = ctx.saved_tensors
        g = _f32c(dloss).reshape(1)
        dx = torch.empty_like(x)
        check(lib.nnl_bce_logits_bwd(ptr(x), ptr(t), ptr(g), ptr(dx), x.numel(), stream()))
        return dx.view(ctx.shape), None


def bce_with_logits(input, target):
    "mean(max(x, 0) - x t + log1p(exp(-|x|))) as a 0-dim tensor; gradient with respect to `input` only (targets are data)"
    return _BCEWithLogits.apply(input, target)


def fbeta(pred, target, beta, threshold=0.5, use_thresh=True, eps=1e-9):
    """fbeta_loss.__call__ (reference General/LossesMetrics.py:70-78) on [N, C] logits (use_thresh) or 0/1 predictions and 0/1 targets:
    the mean over the rows of the F-beta score, a 0-dim tensor, in one launch (no gradient: a metric)."""
    require_cuda(pred, target)
    p, t = _f32c(pred.detach()), _f32c(target.detach())
    if p.dim() != 2 or p.shape != t.shape or p.numel() == 0:
        raise ValueError('fbeta: pred and target must be non-empty [N, C] tensors of one shape (got %s, %s)' % (tuple(pred.shape), tuple(target.shape)))
    N, C = p.shape
    out = torch.empty((), dtype=torch.float32, device=p.device)
    wsb = int(lib.nnl_fbeta_workspace_bytes(N, C))
    ws = _workspace(wsb, p.device)
    check(lib.nnl_fbeta(ptr(p), ptr(t), ptr(out), N, C, float(beta) ** 2, float(threshold), int(bool(use_thresh)), float(eps), ptr(ws), wsb, stream()))
    return out


class _ScaledSigmoid(torch.autograd.Function):
    """lo + (hi - lo) * sigmoid(x): FullyConnectedNet's 'sigmoidal' output activation (reference General/Layers.py:150-152)"""

    @staticmethod
    def forward(ctx, x, lo, hi):
        require_cuda(x)
        xc = _f32c(x)
        y, sg = torch.empty_like(xc), torch.empty_like(xc)
        check(lib.nnl_scaled_sigmoid_fwd(ptr(xc), ptr(y), ptr(sg), xc.numel(), float(lo), float(hi), stream()))
        ctx.save_for_backward(sg)
        ctx.rng = (float(lo), float(hi))
        return y

    @staticmethod
    def backward(ctx, dy):
        sg, = ctx.saved_tensors
        dyc = _f32c(dy)
        dx = torch.empty_like(sg)
        check(lib.nnl_scaled_sigmoid_bwd(ptr(dyc), ptr(sg), ptr(dx), sg.numel(), ctx.rng[0], ctx.rng[1], stream()))
        return dx, None, None


def scaled_sigmoid(x, lo, hi):
    return _ScaledSigmoid.apply(x, float(lo), float(hi))


def embdotbias(x, U, M, bu, bi, output_range=None):
    """y = lo + (hi-lo)*sigmoid(<U[x[:,0]], M[x[:,1]]> + bu[x[:,0]] + bi[x[:,1]]); x int64 [n,2]."""
    lo, hi = (None, None) if output_range is None else (float(output_range[0]), float(output_range[1]))
    return _EmbDotBias.apply(x, U, M, bu, bi, lo, hi)


# ---------------------------------------------------------------------------------------------------------
# K1 conv2d.  Logical tensors stay NCHW / [K,C,R,S] (drop-in API, state_dict layout); the kernels see their
# channels_last physical images: activations NHWC, filters KRSC.
# ---------------------------------------------------------------------------------------------------------
def to_nhwc(x):
    """[N,C,H,W] logical -> contiguous [N,H,W,C] tensor (no copy when x is already channels_last)."""
    return x.permute(0, 2, 3, 1).contiguous()


def from_nhwc(x):
    """contiguous [N,H,W,C] -> logical [N,C,H,W] view (channels_last strides)."""
    return x.permute(0, 3, 1, 2)


def _geom(N, H, W, C, K, R, S, stride, pad):
    P = (H + 2 * pad - R) // stride + 1
    Q = (W + 2 * pad - S) // stride + 1
    return _lib.ConvGeom(N, H, W, C, K, R, S, stride, pad, P, Q)


def _pad_c4(t_nhwc):
    """pad the innermost (channel) dim of an NHWC / KRSC tensor to a multiple of 4 with zeros."""
    C = t_nhwc.shape[-1]
    if C % 4 == 0:
        return t_nhwc
    if t_nhwc.is_cuda and t_nhwc.dtype == torch.float32 and t_nhwc.is_contiguous() and not (torch.is_grad_enabled() and t_nhwc.requires_grad):
        Cp = C + 4 - C % 4                                # one launch (torch's pad is a fill + a strided copy)
        out = torch.empty(t_nhwc.shape[:-1] + (Cp,), dtype=torch.float32, device=t_nhwc.device)
        check(lib.nnl_pad_cols(ptr(t_nhwc), ptr(out), t_nhwc.numel() // C, C, Cp, stream()))
        return out
    return torch.nn.functional.pad(t_nhwc, (0, 4 - C % 4))


# ---- prepared conv filters: one window object per model --------------------------------------------------------------------------
# The transformed filter of a 3x3 / stride 1 / pad 1 layer (include/nnl.h: nnl_wino_filter_multi) and the transpose W^T of a dgrad depend
# on the weights only; producing them inside every convolution call costs one extra launch per call (58 + 37 per ResNet-34 step).  A
# training step opens a WINDOW on its model instead (`filter_window`: prepare_forward .. prepare_backward .. finish_backward): all
# filters of the layers that took a Winograd kernel in the LAST step are transformed in one launch per pass, all transposes in one, and
# the convolutions pick them up by weight address.  The window closes before the optimizer touches the weights, so a filter modified
# later can never meet a stale transform: the views exist only in the open object, and nothing is handed out through a closed one.
_OPEN = None          # the _Filters whose window is open (at most one), or None


def _wino_u_numel(rows, ch, mode):
    "floats of the transformed filter in the layout of kernel `mode` (include/nnl.h: nnl_conv2d_wino_preferred)"
    return rows * 16 * ch if mode == 2 else rows * 12 * ch


class _FilterBatch:
    """persistent output buffers (one flat allocation) + device descriptor table + block -> descriptor table of one *_multi entry.
    items = [(view key, view shape, blocks of the launch, f(dst pointer, first block) -> descriptor row)]; `extra`: the entry's
    arguments between the block count and the stream.  (`entry` is the symbol's NAME: the model, and this with it, must stay deep-copyable.)"""

    def __init__(self, key, dev, entry, desc_dtype, items, extra=()):
        self.key, self.entry, self.extra = key, entry, extra
        sizes = [int(np.prod(shape)) for _, shape, _, _ in items]
        self.flat = torch.empty(sum(sizes), dtype=torch.float32, device=dev)
        desc = np.zeros(len(items), dtype=desc_dtype)
        block_desc, self.views, off = [], {}, 0
        for i, ((k, shape, nb, row), n) in enumerate(zip(items, sizes)):
            v = self.views[k] = self.flat[off:off + n].view(shape)
            off += n
            desc[i] = row(v.data_ptr(), len(block_desc))
            block_desc += [i] * nb
        self.n_blocks = len(block_desc)
        self.desc = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
        self.block_desc = torch.tensor(block_desc, dtype=torch.int32, device=dev)

    def run(self):
        check(getattr(lib, self.entry)(ptr(self.desc), ptr(self.block_desc), self.n_blocks, *self.extra, stream()))


def _wino_batch(key, srcs):
    """nnl_wino_filter_multi over srcs = [(key_ptr, src tensor [rows,3,3,ch], flip, mode)], mode as nnl_conv2d_wino_preferred:
    1 -> U [rows,12,ch] (1-D kernel), 2 -> U [rows,16,ch] (2-D kernel); views by (key_ptr, mode)"""
    def item(k, t, flip, mode):
        rows, ch = t.shape[0], t.shape[3]
        nb = (rows * ch + 255) // 256 if mode == 2 else (rows * 3 * ch + 255) // 256
        return (k, mode), (_wino_u_numel(rows, ch, mode),), nb, lambda dst, first: (t.data_ptr(), dst, rows, ch, flip, first, 1 if mode == 2 else 0, 0)
    dtype = np.dtype([('src', '<u8'), ('dst', '<u8'), ('rows', '<i4'), ('ch', '<i4'), ('flip', '<i4'), ('first', '<i4'), ('two_d', '<i4'), ('reserved', '<i4')])
    return _FilterBatch(key, srcs[0][1].device, 'nnl_wino_filter_multi', dtype, [item(*s) for s in srcs])


def _wt_batch(key, weights):
    "nnl_conv2d_weight_transpose_multi over the conv filters [K,C,R,S] of one model; views W^T [C,R,S,K] by weight address"
    def item(w):
        K, C, R, S = w.shape
        return w.data_ptr(), (C, R, S, K), R * S * ((K + 31) // 32) * ((C + 31) // 32), lambda dst, first: (w.data_ptr(), dst, K, R * S, C, first)
    dtype = np.dtype([('w', '<u8'), ('wt', '<u8'), ('K', '<i4'), ('RS', '<i4'), ('C', '<i4'), ('first', '<i4')])
    return _FilterBatch(key, weights[0].device, 'nnl_conv2d_weight_transpose_multi', dtype, [item(w) for w in weights],
                        (float(sum(w.numel() for w in weights)),))


class _Filters:
    "the prepared-filter state of ONE model (model._nnl_filters; it dies with the model)"

    def __init__(self, model):
        # the module walk costs ~0.1 ms per step on a host-bound model: done once.  A conv added later transforms its own filter (slower, correct)
        self.mods = [m for m in model.modules() if getattr(m, 'nnl_hip_conv', False)]
        self.step = 0         # training-step counter (open): the recorded modes of a weight are those of its LAST step
        self.modes = {}       # weight data_ptr -> [[step stamp, modes the forward calls took], [stamp, modes the dgrad calls took]] (sets; 1 = 1-D,
                              # 2 = 2-D kernel): a weight shared between geometries (RetinaNet's heads: five pyramid levels) may need BOTH layouts
        self.batches = {}     # 'fwd' / 'bwd' / 'wt' -> the persistent forward U / dgrad U' / W^T batch (_FilterBatch)
        # the views the convolutions read, filled ONLY while the window is open:
        self.u = ({}, {})     # [0] forward, [1] dgrad: (weight data_ptr, kernel mode) -> U [K,4|16,3|1,C] / U' [C,...,K] in that kernel's layout
        self.wt = {}          # weight data_ptr -> W^T tensor [C,R,S,K]
        self.wt_padded = {}   # (weight data_ptr, shape, pad) -> transposed, channel-padded filter of a K % 16 != 0 dgrad

    def open(self):
        global _OPEN
        finish_backward()                # (whichever model's window was left open)
        self.step += 1                   # a new training step: the modes recorded from here on replace the previous step's
        _OPEN = self

    def recorded(self, key_ptr, which):
        return self.modes[key_ptr][which][1] if key_ptr in self.modes else ()

    def _run(self, slot, key, build, *args):
        """the persistent batch `slot` after its launch, rebuilt first when its key (the weights' pointers, shapes and modes) changed; None
        when that happens while the stream is capturing (buffers are built during the eager warm-up steps): nothing is published then"""
        batch = self.batches.get(slot)
        if batch is None or batch.key != key:
            if torch.cuda.is_current_stream_capturing():
                return None
            batch = self.batches[slot] = build(key, *args)
        batch.run()
        return batch

    def _run_wino(self, which, srcs):
        if srcs and os.environ.get('NNL_WINO_PREPARE', '1') != '0':
            batch = self._run(('fwd', 'bwd')[which], tuple((k, t.data_ptr(), tuple(t.shape), mode) for k, t, _, mode in srcs), _wino_batch, srcs)
            if batch is not None:
                self.u[which].update(batch.views)

    def prepare_forward(self):
        self.open()
        srcs = []
        for m in self.mods:
            w = m.weight
            modes = self.recorded(w.data_ptr(), 0)
            if (modes and w.is_cuda and w.dim() == 4 and w.shape[2] == 3 and w.shape[3] == 3 and w.dtype == torch.float32
                    and w.is_contiguous(memory_format=torch.channels_last)):
                srcs += [(w.data_ptr(), w.permute(0, 2, 3, 1), 0, mode) for mode in sorted(modes)]    # KRSC view of the same memory
        self._run_wino(0, srcs)

    def prepare_backward(self):
        if _OPEN is not self:
            self.open()
        ws = [m.weight for m in self.mods
              if m.weight.is_cuda and m.weight.dim() == 4 and m.weight.shape[1] % 4 == 0
              and m.weight.shape[0] % 4 == 0 and m.weight.dtype == torch.float32
              and m.weight.is_contiguous(memory_format=torch.channels_last)]
        if len(ws) < 2 or sum(w.requires_grad for w in ws) * 2 < len(ws):
            return
        batch = self._run('wt', tuple((w.data_ptr(), tuple(w.shape)) for w in ws), _wt_batch, ws)
        if batch is not None:
            self.wt.update(batch.views)
            # the dgrad Winograd filters U' [C,4,3,K] of the layers whose last dgrad took the Winograd kernel, from the transposes above
            self._run_wino(1, [(w.data_ptr(), batch.views[w.data_ptr()], 1, mode) for w in ws if w.shape[2] == 3 and w.shape[3] == 3
                               for mode in sorted(self.recorded(w.data_ptr(), 1))])

    def wino(self, key_ptr, which, g):
        """the prepared filter, or None, for the forward (which = 0) / dgrad (1) call of geometry g on the weight at key_ptr.  Inside the
        window the call's kernel mode (nnl_conv2d_wino_preferred: 0 direct, 1 Winograd 1-D, 2 Winograd 2-D) is remembered per weight
        for the next step's batch, and the prepared buffer is handed over only when its size is that of the mode's layout.  key_ptr 0
        (a channel-padded dgrad: it transforms its own filter) records and finds nothing.  Neither does any call outside the window —
        evaluation, no_grad, other batch sizes, a bare loss.backward() with neither prepare call (the first bracketed step after it
        transforms per call, the second uses the batch: same bits): an evaluation forward must not change the next training step's
        batch (a rebuild would free buffers a captured step still reads), and grad mode cannot tell the two apart here: autograd runs
        every Function's forward with it off."""
        if _OPEN is not self or not key_ptr:
            return None
        mode = int(lib.nnl_conv2d_wino_preferred(g, which)) if (g.R == 3 and g.S == 3 and g.stride == 1) else 0
        if mode or key_ptr in self.modes:
            e = self.modes.setdefault(key_ptr, [[-1, set()], [-1, set()]])[which]
            if e[0] != self.step:                        # first call of this training step: forget the old modes
                e[0], e[1] = self.step, set()
            if mode:
                e[1].add(mode)
        u = self.u[which].get((key_ptr, mode)) if mode else None
        rows, ch = (g.C, g.K) if which else (g.K, g.C)
        return u if u is not None and u.numel() == _wino_u_numel(rows, ch, mode) else None


_CLOSED = _Filters(torch.nn.Module())     # never opened, so never written: what a convolution outside every window asks (nothing recorded, nothing found)


def _filters(model):
    if getattr(model, '_nnl_filters', None) is None:
        object.__setattr__(model, '_nnl_filters', _Filters(model))
    return model._nnl_filters


def prepare_forward(model):
    """Call right before the forward of a TRAINING step (filter_window does): opens the window and transforms the Winograd filters of
    every HipConv2d whose forward took a Winograd kernel in the last step, in one launch; valid until finish_backward()."""
    _filters(model).prepare_forward()


def prepare_backward(model):
    """Call right before `loss.backward()` (filter_window's backward does; opens the window itself when prepare_forward did not):
    transposes the filters of every HipConv2d of `model` in ONE launch (one small launch per layer otherwise), transforms the dgrad
    Winograd filters from them, and exposes both to the convolutions' backward until finish_backward()."""
    _filters(model).prepare_backward()


def finish_backward():
    "closes the window of everything prepare_forward / prepare_backward exposed (the optimizer is about to change the weights)"
    global _OPEN
    if _OPEN is not None:
        for views in (*_OPEN.u, _OPEN.wt, _OPEN.wt_padded):
            views.clear()
        _OPEN = None


def prepared_batches(model):
    """the persistent filter batches (_FilterBatch) the last prepare_forward / prepare_backward of `model` ran.  A captured step bakes
    raw pointers to their buffers and descriptor tables into its graph and must keep them alive (Learner._GraphedStep): the next step
    at another batch size may replace the model's batch when the layers' Winograd modes change."""
    return tuple(_filters(model).batches.values())


def prepared_filter_counts():
    "(forward U, dgrad U', W^T) views the open window exposes to the convolutions; zeros when none is open"
    f = _OPEN or _CLOSED
    return len(f.u[0]), len(f.u[1]), len(f.wt)


@contextlib.contextmanager
def filter_window(model):
    """with ops.filter_window(model) as backward: loss = loss_func(model(x), y); backward(loss)
    One training step's prepared-filter window: entering is prepare_forward, backward(loss) is prepare_backward + loss.backward(), and
    leaving — also by an exception anywhere in the body — is finish_backward: the window never outlives a failed step, whose next
    forward may follow a weight change."""
    def backward(loss):
        prepare_backward(model)
        loss.backward()
    prepare_forward(model)
    try:
        yield backward
    finally:
        finish_backward()


# Gradient buffers whose rows are ALREADY padded with zeros to the GEMM granularity (the softmax-CE backward at V % 16 != 0, the
# LSTM's dgates at 4H % 32 != 0): the producer registers the padded base tensor, hands autograd the [:, :K] view, and the linear
# layer that receives it (through whatever reshape / permute views autograd inserts) recognises its base and uses the padded rows
# directly.  Keyed by id() and guarded by a weak reference, so a recycled id can never match.
_PADDED_GRADS = {}


def register_padded_grad(base, ld):
    if len(_PADDED_GRADS) > 64:
        for k in [k for k, (r, _) in _PADDED_GRADS.items() if r() is None]:
            del _PADDED_GRADS[k]
    _PADDED_GRADS[id(base)] = (weakref.ref(base), int(ld))


def _padded_rows(dy, K):
    "dy logical [N, K, 1, 1]: the [N,1,1,ld] tensor over its registered zero-padded base, or None"
    base = dy._base if dy._is_view() else None
    ent = _PADDED_GRADS.get(id(base)) if base is not None else None
    if ent is None or ent[0]() is not base or dy.dim() != 4 or dy.shape[2] != 1 or dy.shape[3] != 1:
        return None
    ld = ent[1]
    if dy.dtype != torch.float32 or dy.stride(1) != 1 or dy.stride(0) != ld or ld < K or ld % 16 != 0 or dy.storage_offset() % ld != 0:
        return None
    if dy.storage_offset() + dy.shape[0] * ld > base.numel():
        return None
    return torch.as_strided(base, (dy.shape[0], 1, 1, ld), (ld, ld, ld, 1), dy.storage_offset())


_TILE_COUNTERS = {}


def _tile_counters(device):
    """persistent zero-at-rest ticket counters of the conv kernels' in-kernel split-tile fix-up (include/nnl.h), one buffer per
    device: every op of this package runs on torch's current stream, one conv at a time (a captured step replays on that same
    stream).  Created on first use outside stream capture (eager warm-up steps precede every capture)."""
    t = _TILE_COUNTERS.get(device.index)
    if t is None:
        if torch.cuda.is_current_stream_capturing():
            return None
        t = _TILE_COUNTERS[device.index] = torch.zeros(int(lib.nnl_conv2d_tile_counters()), dtype=torch.int32, device=device)
    return t


class GradSlot:
    """Side channel between two autograd Functions of one residual block: the BN that closes the block parks the gradient of
    its identity shortcut here (instead of returning it to autograd) and the block's FIRST convolution adds it in the
    epilogue of its dgrad kernel — one accumulation kernel and three tensor passes less per block.  Valid because the first
    convolution's backward always runs after the closing BN's backward (it depends on it through the main path) and both
    consume the same tensor x.
    A block with a projection shortcut uses it the same way: the downsample convolution (`give_slot`) parks ITS input gradient
    here and returns none to autograd.  There is no dependency between the two convolutions' backward nodes (the engine runs
    the later-created downsample first), so the hand-over is guarded: the consumer closes the slot when it runs, and a
    producer that finds it closed returns its gradient to autograd as usual."""
    __slots__ = ('tensor', 'closed')

    def __init__(self):
        self.tensor = None
        self.closed = False



# ---- parameters shared by several forward calls of one step (RetinaNet's heads on the five pyramid levels) ----------------------------
# Autograd sums the per-call gradients of such a parameter with a chain of accumulation kernels (4 adds per tensor and step; 91 ATen
# launches per RetinaNet step, 0.54 ms: profiles/r4_retinanet_kernel_stats.csv).  `shared_params(modules, n)` hands every parameter
# of `modules` out as n ALIASES (same storage) produced by one autograd node whose backward adds the n gradients in call order with ONE
# launch (nnl_sum_tensors); HipConv2d.forward takes the next alias of its weight / bias (`fan_param`).  The same sum as autograd's
# accumulation up to the order of the additions (call order here, backward order there); bitwise reproducible run to run.
_FAN = {}


class _FanOut(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, n):
        ctx.n = n
        return tuple(p.detach().view(p.shape) for _ in range(n))

    @staticmethod
    def backward(ctx, *grads):
        have = [g for g in grads if g is not None]
        if not have:
            return None, None
        if len(have) == 1:
            return have[0], None
        g0 = have[0]
        dense = all(g.is_cuda and g.dtype == torch.float32 and g.shape == g0.shape and g.stride() == g0.stride() and g.data_ptr() % 16 == 0
                    and (g.is_contiguous() or (g.dim() == 4 and g.is_contiguous(memory_format=torch.channels_last))) for g in have)
        if not dense or len(have) > 8:
            out = have[0]
            for g in have[1:]:
                out = out + g
            return out, None
        out = torch.empty_like(g0)                       # (preserves the dense layout of the operands)
        arr = (ctypes.c_void_p * len(have))(*[g.data_ptr() for g in have])
        check(lib.nnl_sum_tensors(arr, len(have), ptr(out), g0.numel(), stream()))
        return out, None


class shared_params:
    """with shared_params([module, ...], n_calls): ... the n_calls forward calls of the modules ...   (training with autograd only:
    outside it — evaluation, no_grad — the modules use their parameters directly)"""

    def __init__(self, modules, n):
        self.modules, self.n, self.keys = modules, int(n), []

    def __enter__(self):
        if self.n > 1 and torch.is_grad_enabled():
            for m in self.modules:
                for p in m.parameters():
                    if p.requires_grad and p.is_cuda and id(p) not in _FAN:
                        _FAN[id(p)] = list(_FanOut.apply(p, self.n))
                        self.keys.append(id(p))
        return self

    def __exit__(self, *exc):
        for k in self.keys:
            _FAN.pop(k, None)
        return False


def fan_param(p):
    "the next alias of a parameter inside `shared_params`, else the parameter itself"
    if p is None or not _FAN:
        return p
    lst = _FAN.get(id(p))
    return lst.pop(0) if lst else p


# What a convolution's forward leaves for _conv_backward.  g: geometry of the saved (channel-padded) operands; relu: 0 none, 1 ReLU,
# 2 sigmoid; c_in: input channels before padding; w_layout: (shape, strides) of the weight as autograd sees it; slot / give_slot: see
# GradSlot; grad_dst: the weight's segment of the flat all-reduce bucket (dist.GradSync); uses: [forward uses of the weight this step]
_ConvState = collections.namedtuple('_ConvState', 'g relu has_bias c_in w_layout slot give_slot grad_dst uses')


def _conv_operands(x, weight, bias, stride, pad):
    "(x NHWC and weight KRSC, channels padded to 4; fp32 bias or None; the geometry; the uninitialised NHWC output) of a forward call"
    xn = _pad_c4(to_nhwc(_f32c(x) if x.dim() != 4 else x.float()))
    wn = _pad_c4(to_nhwc(weight.float()))
    N, H, W, C = xn.shape
    K, R, S, _ = wn.shape
    g = _geom(N, H, W, C, K, R, S, stride, pad)
    y = torch.empty((N, g.P, g.Q, K), dtype=torch.float32, device=x.device)
    return xn, wn, (None if bias is None else _f32c(bias)), g, y


def _conv_state(x, weight, bias, g, relu, slot=None, give_slot=None):
    "the _ConvState of one forward call (every conv Function builds it here); counts the call as a use of `weight`"
    uses = getattr(weight, '_nnl_uses', None)
    if uses is not None:
        uses[0] += 1
    return _ConvState(g, relu, bias is not None, x.shape[1], (tuple(weight.shape), tuple(weight.stride())), slot, give_slot,
                      getattr(weight, '_nnl_grad_dst', None), uses)


def _with_k(g, K):
    "the geometry g with K output channels"
    return _geom(g.N, g.H, g.W, g.C, K, g.R, g.S, g.stride, g.pad)


def _conv_backward(st, xn, wn, y, dy, needs):
    """(dx, dw, db) of a convolution from its _ConvState, the tensors its forward saved (y: the output, for the activation gate), the
    logical [N,K,P,Q] output gradient and `needs` = which of the three are wanted.  (dy4, w4, g4): the operands with K padded to a
    multiple of 4 — or to the width of the registered buffer dy arrived in — for wgrad and the bias sum; the dgrad derives its own."""
    if dy is None:
        return None, None, None
    g, K = st.g, st.g.K
    want_db = st.has_bias and needs[2]
    db = None
    pre = _padded_rows(dy, K) if (not st.relu and g.R == 1 and g.S == 1 and g.H == 1 and g.W == 1) else None
    if pre is not None and pre.shape[-1] != K:
        dy4 = pre     # arrived in a zero-padded buffer: every pass runs on the padded K, a multiple of 16 (the dgrad pads no further)
    else:
        dy4 = to_nhwc(dy.float())
        if st.relu:
            dy4, db = _conv_act_gate(y, dy4, g, st.relu, want_db)
        if K % 4 != 0:                      # e.g. RetinaNet 36/180-channel output convs: pad dy's channels
            dy4 = _pad_c4(dy4)
    w4, g4 = wn, g
    if dy4.shape[-1] != K:
        w4, g4 = torch.nn.functional.pad(wn, (0, 0, 0, 0, 0, 0, 0, dy4.shape[-1] - K)), _with_k(g, dy4.shape[-1])
    dx = dw = None
    if needs[0]:
        dx = _conv_dgrad(st, dy4, w4, g4, K)
    elif st.slot is not None:               # closed even when nobody wants dx: a later producer must not park a tensor nobody consumes
        st.slot.tensor, st.slot.closed = None, True
    if needs[1]:
        dw = _conv_wgrad(st, xn, dy4, g4, K)
    if db is None and want_db:
        db = _conv_bias_grad(dy4, g4, K)
    return dx, dw, db


def _conv_act_gate(y, dyn, g, relu, want_db):
    "ReLU / sigmoid gate (+ the bias gradient of the gated dy) in one pass -> (gated dy, db or None)"
    rows = g.N * g.P * g.Q
    gated = torch.empty_like(dyn)
    cb = int(lib.nnl_colsum_workspace_bytes(rows, g.K)) if want_db else 0
    cws = _workspace(cb, dyn.device, floor=True) if want_db else None      # never a null
    db = torch.empty(g.K, dtype=torch.float32, device=dyn.device) if want_db else None
    check(lib.nnl_act_gate_colsum(ptr(dyn), ptr(y), ptr(gated), ptr(db), rows, g.K, int(relu), ptr(cws), cb, stream()))
    return gated, db


def _conv_dgrad_operands(dy4, w4, g4, K):
    """(dy, W^T [C,R,S,K'], geometry) of the dgrad: the K-padded-to-4 set as is, or with K padded on to a multiple of 16; the filter
    transpose comes from the caches of prepare_backward's window where it can"""
    ktail = g4.R == 1 and g4.S == 1 and g4.K % 4 == 0            # the tap kernel masks the k tail itself
    dyd, gd, padk, wkey = dy4, g4, 0, None
    f = _OPEN or _CLOSED                     # (f.wt is non-empty only inside the backward window, after the batched transposes)
    if g4.K % 16 != 0 and g4.K >= 32 and not ktail:
        # dgrad reduces over K: the tap-table kernel needs K % 16 == 0 (RetinaNet's 36- / 180-channel output convs would
        # fall back to the first-generation kernel, ~2.5x slower); zero channels cost one copy of dy
        padk = 16 - g4.K % 16
        dyd, gd = torch.nn.functional.pad(dy4, (0, padk)), _with_k(g4, g4.K + padk)
        wkey = (w4.data_ptr(), tuple(w4.shape), padk)
        wt = f.wt_padded.get(wkey) if f.wt else None           # a shared filter (RetinaNet's output convs on five levels): padded + transposed ONCE per backward pass
    else:
        wt = f.wt.get(w4.data_ptr()) if g4.K == K else None
        if wt is not None and tuple(wt.shape) != (g4.C, g4.R, g4.S, g4.K):
            wt = None
    if wt is None:
        wd = torch.nn.functional.pad(w4, (0, 0, 0, 0, 0, 0, 0, padk)) if padk else w4
        wt = torch.empty((gd.C, gd.R, gd.S, gd.K), dtype=torch.float32, device=dy4.device)
        check(lib.nnl_conv2d_weight_transpose(ptr(wd), ptr(wt), gd.K, gd.R, gd.S, gd.C, stream()))
        if wkey is not None and f.wt:                         # (only inside the prepare_backward .. finish_backward window: weights are fixed there)
            f.wt_padded[wkey] = wt
    return dyd, wt, gd


def _conv_dgrad(st, dy4, w4, g4, K):
    "the logical input gradient (with the GradSlot shortcut added), or None when it was parked in st.give_slot"
    dyd, wt, g = _conv_dgrad_operands(dy4, w4, g4, K)
    dxn = torch.empty((g.N, g.H, g.W, g.C), dtype=torch.float32, device=dyd.device)
    wsb = int(lib.nnl_conv2d_dgrad_workspace_bytes(g))
    dws = _workspace(wsb, dyd.device)                       # None at 0 bytes: no Winograd kernel without a workspace
    shortcut = None
    if st.slot is not None:
        shortcut, st.slot.tensor, st.slot.closed = st.slot.tensor, None, True
    # stride 2: every output-parity class of a 3x3 / pad 1 filter has a tap, so every dx pixel passes through the epilogue
    # (more than 49 taps, or a raster wider than 32 with pad > 127: the first-generation kernel, which has no addend — the library refuses it)
    fuse = shortcut is not None and g.K % 16 == 0 and g.R * g.S <= 49 and shortcut.numel() == dxn.numel() \
        and ((g.stride == 1 and (g.S <= 32 or g.pad <= 127)) or (g.stride == 2 and g.R == 3 and g.S == 3 and g.pad == 1))
    # a channel-padded dgrad transforms its own filter: not recorded under the weight (key 0; a 1x1 filter's mode 0 records nothing)
    u = (_OPEN or _CLOSED).wino(w4.data_ptr() if g.K == K else 0, 1, g)
    check(lib.nnl_conv2d_dgrad_pre(ptr(dyd), ptr(wt), ptr(dxn), g, ptr(shortcut) if fuse else None, ptr(dws), wsb,
                                   ptr(_tile_counters(dyd.device) if wsb else None), ptr(u), stream()))
    if shortcut is not None and not fuse:
        dxn += shortcut.view_as(dxn)
    give = st.give_slot
    if give is not None and not give.closed and st.c_in == g.C:
        give.tensor = dxn                           # the block's first conv adds it inside its dgrad kernel
        return None
    return from_nhwc(dxn[..., :st.c_in] if st.c_in != g.C else dxn)


def _conv_wgrad(st, xn, dy4, g4, K):
    "the weight gradient in the weight's logical shape, written straight into the data-parallel bucket where that is safe"
    dst = st.grad_dst
    # in place only for a weight used ONCE this step: the gradients of a shared weight (RetinaNet heads on 5 pyramid
    # levels) are summed by autograd and must not alias each other
    if dst is not None and st.uses is not None and st.uses[0] == 1 and dst.dim() == 4 and g4.K == K and st.c_in == g4.C \
            and dst.permute(0, 2, 3, 1).is_contiguous() and tuple(dst.shape) == (g4.K, g4.C, g4.R, g4.S):
        dwn = dst.permute(0, 2, 3, 1)               # the bucket segment, viewed KRSC: the kernel writes it in place
    else:
        dwn = torch.empty((g4.K, g4.R, g4.S, g4.C), dtype=torch.float32, device=dy4.device)
    wsb = int(lib.nnl_conv2d_wgrad_workspace_bytes(g4))
    ws = _workspace(wsb, dy4.device, floor=True)            # never a null
    check(lib.nnl_conv2d_wgrad(ptr(xn), ptr(dy4), ptr(dwn), g4, ptr(ws), wsb, stream()))
    dw = from_nhwc(dwn[:K, :, :, :st.c_in])
    # a 1x1 filter's [K, C, 1, 1] gradient: give it EXACTLY the parameter's strides (the size-1 dimensions make them ambiguous);
    # otherwise AccumulateGrad sees a layout mismatch and clones it into the parameter's layout — one device copy per 1x1
    # convolution and step (53 of RetinaNet's 68 rocclr_copyBuffer launches, profiles/r5_retinanet_kernel_stats.csv)
    wshape, wstride = st.w_layout
    if (g4.R == 1 and g4.S == 1 and wshape == tuple(dw.shape) and wstride != tuple(dw.stride()) and dw.is_contiguous(memory_format=torch.channels_last)
            and wstride[1] == 1 and wstride[0] == dw.shape[1]):
        dw = dw.as_strided(wshape, wstride)
    return dw


def _conv_bias_grad(dy4, g4, K):
    "column sums of dy (the first K of them: the rest are padding)"
    rows = g4.N * g4.P * g4.Q
    db_full = torch.empty(g4.K, dtype=torch.float32, device=dy4.device)
    cb = int(lib.nnl_colsum_workspace_bytes(rows, g4.K))
    cws = _workspace(cb, dy4.device, floor=True)            # never a null
    check(lib.nnl_colsum(ptr(dy4), ptr(db_full), rows, g4.K, ptr(cws), cb, stream()))
    return db_full[:K]


class _Conv2d(torch.autograd.Function):
    """nn.Conv2d forward/backward (reference Applications/VisionModels/retinanet.py:26-28,66-71,106-124,169-185,
    241-257,304,345) on the fp32-MFMA implicit-GEMM kernels; optional fused bias + ReLU epilogue."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, pad, relu, slot=None, bn_pivot=None, give_slot=None):
        require_cuda(x, weight, bias)
        xn, wn, b, g, y = _conv_operands(x, weight, bias, stride, pad)
        N, K = g.N, g.K
        ctx.st = _conv_state(x, weight, bias, g, relu, slot, give_slot)
        wsb = int(lib.nnl_conv2d_fwd_workspace_bytes(g))         # balanced-schedule slabs (0 when the plain launch is used)
        ws = _workspace(wsb, x.device)                           # None at 0 bytes: no Winograd kernel without a workspace
        part, rows = None, _lib.i32(0)
        if bn_pivot is not None:                                  # BatchNorm statistics from the conv epilogue (include/nnl.h)
            part = torch.empty(((N * g.P * g.Q + 63) // 64) * K * 2, dtype=torch.float32, device=x.device)
        u = (_OPEN or _CLOSED).wino(wn.data_ptr(), 0, g)                   # the filter prepared for this step, if any — in THIS call's layout
        check(lib.nnl_conv2d_fwd_pre(ptr(xn), ptr(wn), ptr(b), ptr(y), g, int(relu), ptr(ws), wsb, ptr(_tile_counters(x.device) if wsb else None),
                                     ptr(part), ptr(bn_pivot), ctypes.byref(rows) if part is not None else None, ptr(u), stream()))
        if part is None or rows.value == 0:
            part = torch.empty(0, dtype=torch.float32, device=x.device)
        else:
            part = part[:rows.value * K * 2]
        ctx.mark_non_differentiable(part)
        ctx.set_materialize_grads(False)              # no zero-filled gradient tensor for `part` in backward: dy may be None
        ctx.save_for_backward(xn, wn, y if relu else None)        # relu: 0 none, 1 ReLU, 2 sigmoid (both gates need the OUTPUT y)
        return from_nhwc(y), part

    @staticmethod
    def backward(ctx, dy, _dpart=None):
        xn, wn, y = ctx.saved_tensors
        return _conv_backward(ctx.st, xn, wn, y, dy, ctx.needs_input_grad[:3]) + (None,) * 6


def _conv(x, weight, bias, *, stride=1, pad=0, relu=0, slot=None, bn_pivot=None, give_slot=None):
    "(y, BatchNorm partials) of _Conv2d: the one place that spells its argument order"
    return _Conv2d.apply(x, weight, bias, int(stride), int(pad), int(relu), slot, bn_pivot, give_slot)


def conv2d(x, weight, bias=None, stride=1, pad=0, relu=False, grad_slot=None, give_slot=None):
    """y = act(conv2d(x, weight, bias, stride, padding=pad)); relu: False / 0 none, True / 1 ReLU, 2 sigmoid (fused into the
    kernel epilogue; the backward gate and the bias gradient are one pass); x logical [N,C,H,W], weight [K,C,R,S].
    grad_slot: see GradSlot (the shortcut gradient of a residual block, added to dx inside the dgrad kernel)."""
    return _conv(x, weight, bias, stride=stride, pad=pad, relu=relu, slot=grad_slot, give_slot=give_slot)[0]


class _ConvAddUp2(torch.autograd.Function):
    """conv2d(x, weight, bias) + nearest-x2-upsample(small) in ONE kernel (reference PyramidFeatures.forward,
    retinanet.py:126-148: `P5_upsampled + P4_1(C4)`, `P3_1(C3) + P4_upsampled`); backward = the convolution's backward on dy plus
    the 2x2 block sums of dy for `small` (nnl_upsample2_bwd)."""

    @staticmethod
    def forward(ctx, x, weight, bias, small, stride, pad):
        require_cuda(x, weight, bias, small)
        xn, wn, b, g, y = _conv_operands(x, weight, bias, stride, pad)
        sn = to_nhwc(small.float())
        ctx.small_shape = (g.N, g.P // 2, g.Q // 2, g.K)
        if tuple(sn.shape) != ctx.small_shape or g.P % 2 or g.Q % 2:
            raise _lib.NnlError('conv_add_upsampled: `small` %s is not [N, K, P/2, Q/2] of the %dx%d output' % (tuple(small.shape), g.P, g.Q))
        ctx.st = _conv_state(x, weight, bias, g, 0)
        check(lib.nnl_conv2d_fwd_add_up2(ptr(xn), ptr(wn), ptr(b), ptr(sn), ptr(y), g, stream()))
        ctx.save_for_backward(xn, wn)
        return from_nhwc(y)

    @staticmethod
    def backward(ctx, dy):
        dsmall = None
        if ctx.needs_input_grad[3]:
            dyn = to_nhwc(dy.float())
            N, h, w, K = ctx.small_shape
            ds = torch.empty(ctx.small_shape, dtype=torch.float32, device=dy.device)
            check(lib.nnl_upsample2_bwd(ptr(dyn), ptr(ds), N, h, w, K, stream()))
            dsmall = from_nhwc(ds)
        xn, wn = ctx.saved_tensors
        return _conv_backward(ctx.st, xn, wn, None, dy, ctx.needs_input_grad[:3]) + (dsmall, None, None)


def conv_add_upsampled(x, weight, bias, small, stride=1, pad=0):
    "conv2d(x, weight, bias) + F.interpolate(small, scale_factor=2, mode='nearest'), fused (FPN top-down merge)"
    return _ConvAddUp2.apply(x, weight, bias, small, int(stride), int(pad))


def conv2d_with_bn_stats(x, weight, bias, stride, pad, bn_pivot, grad_slot=None, give_slot=None):
    """conv2d whose epilogue also reduces the BatchNorm batch statistics of its output against `bn_pivot` [K].  Returns (y, partials);
    partials is empty when this launch could not produce them (the BatchNorm then runs its own statistics pass)."""
    return _conv(x, weight, bias, stride=stride, pad=pad, slot=grad_slot, bn_pivot=bn_pivot, give_slot=give_slot)


def _rows_in_place(x):
    "a 2-D fp32 matrix whose rows are dense (any row stride): usable by the kernels that take a leading dimension"
    return x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and x.stride(0) >= x.shape[1]


class _LinearSmall(torch.autograd.Function):
    """nn.Linear with 1 - 4 output features (FullyConnectedNet.final_lin of the regression heads, General/Layers.py:146): one wave
    per row forward, fixed-order column reductions backward (csrc/linear_small.hip) instead of a 64-wide MFMA tile per column."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        require_cuda(x, weight, bias)
        x = x if _rows_in_place(x) else _f32c(x)
        w = _f32c(weight)
        b = None if bias is None else _f32c(bias)
        M, K = x.shape
        N = w.shape[0]
        y = torch.empty(M, N, dtype=torch.float32, device=x.device)
        check(lib.nnl_linear_small_fwd(ptr(x), ptr(w), ptr(b), ptr(y), M, K, x.stride(0) if M > 1 else K, N, stream()))
        ctx.save_for_backward(x, w)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        M, K = x.shape
        N = w.shape[0]
        dy = _f32c(dy)
        dev = dy.device
        dx = torch.empty(M, K, dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        dw = torch.empty(N, K, dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        db = torch.empty(N, dtype=torch.float32, device=dev) if (ctx.has_bias and ctx.needs_input_grad[2]) else None
        wsb = int(lib.nnl_linear_small_bwd_workspace_bytes(M, K, N)) if (dw is not None or db is not None) else 0
        ws = _workspace(wsb, dev)
        check(lib.nnl_linear_small_bwd(ptr(dy), ptr(x), ptr(w), ptr(dx), ptr(dw), ptr(db), M, K, x.stride(0) if M > 1 else K, N, ptr(ws), wsb,
                                       stream()))
        return dx, dw, db


def linear(x, weight, bias=None, relu=False):
    """y = x @ weight.T + bias [+ ReLU] (nn.Linear; reference General/Layers.py:39,146; Text.py:572) on the same
    fp32-MFMA implicit-GEMM kernels: a Linear is the 1x1 convolution of a 1x1 'image' per sample.  Leading dims of x
    are flattened into rows."""
    lead = x.shape[:-1]
    x2 = x.reshape(-1, x.shape[-1])
    if not relu and weight.shape[0] <= 4 and x2.is_cuda and x2.shape[0] > 0:
        return _LinearSmall.apply(x2, weight, bias).reshape(*lead, weight.shape[0])
    y = _conv(x2[:, :, None, None], weight[:, :, None, None], bias, relu=relu)[0]
    return y.reshape(*lead, weight.shape[0])


def _rows_view(x):
    """logical [N,C,H,W] (or [rows,C]) -> contiguous [rows, C] matrix + a function mapping such a matrix back."""
    if x.dim() == 4:
        xn = to_nhwc(x.float())
        N, H, W, C = xn.shape
        return xn.view(-1, C), (lambda m: from_nhwc(m.view(N, H, W, C)))
    if x.dim() == 2:
        return _f32c(x), (lambda m: m)
    if x.dim() == 3:                                    # BatchNorm1d on [N, C, L]
        xn = x.float().permute(0, 2, 1).contiguous()
        N, L, C = xn.shape
        return xn.view(-1, C), (lambda m: m.view(N, L, C).permute(0, 2, 1))
    raise ValueError('bn_act: unsupported input rank %d' % x.dim())


def _relu_mask(rows, C, device):
    "uninitialised keep-bit buffer for nnl_bn_fwd (1 bit per element, + 2 words of slack)"
    return torch.empty((rows * C + 31) // 32 + 2, dtype=torch.int32, device=device)


def _bn_grad_buffers(ctx, xm, gamma, has_res):
    "dx, dres (only when the residual wants a gradient), dgamma, dbeta for a BatchNorm backward to fill"
    dx = torch.empty_like(xm)
    dres = torch.empty_like(xm) if (has_res and ctx.needs_input_grad[1]) else None
    dgamma = torch.empty(xm.shape[1], dtype=torch.float32, device=xm.device) if gamma is not None else None
    dbeta = torch.empty(xm.shape[1], dtype=torch.float32, device=xm.device) if gamma is not None else None
    return dx, dres, dgamma, dbeta


def _bn_grads(ctx, back, dx, dres, dgamma, dbeta):
    "the gradients of (x, residual, gamma, beta); with a GradSlot the residual's goes to the block's first conv, which adds it to its dx"
    if ctx.slot is not None and dres is not None:
        ctx.slot.tensor, dres = dres, None
    return back(dx), None if dres is None else back(dres), dgamma, dbeta


class _BNAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, gamma, beta, running_mean, running_var, training, momentum, eps, relu, nbt, slot=None, ext=None,
                pivot_out=None):
        require_cuda(x, residual, gamma, beta)
        ctx.slot = slot
        xm, back = _rows_view(x)
        rows, C = xm.shape
        rm = None if residual is None else _rows_view(residual)[0]
        y = torch.empty_like(xm)
        mean = torch.empty(C, dtype=torch.float32, device=xm.device)
        invstd = torch.empty(C, dtype=torch.float32, device=xm.device)
        wsb = int(lib.nnl_bn_workspace_bytes(rows, C))
        ws = _workspace(wsb, xm.device)
        mask = _relu_mask(rows, C, xm.device) if relu else None      # 1 bit / element for the backward's ReLU gate
        check(lib.nnl_bn_fwd(ptr(xm), ptr(gamma), ptr(beta), ptr(rm), ptr(y), ptr(mean), ptr(invstd), ptr(running_mean),
                             ptr(running_var), rows, C, float(eps), float(momentum), int(training), int(relu), ptr(nbt),
                             ptr(mask), ptr(ext[0]) if ext else None, (ext[0].numel() // (2 * C)) if ext else 0,
                             ptr(ext[1]) if ext else None, ptr(pivot_out), ptr(ws), wsb, stream()))
        ctx.save_for_backward(xm, mask, gamma, mean, invstd)
        ctx.cfg = (training, relu, residual is not None, back)
        return back(y)

    @staticmethod
    def backward(ctx, dy):
        xm, mask, gamma, mean, invstd = ctx.saved_tensors
        training, relu, has_res, back = ctx.cfg
        dym = _rows_view(dy)[0]
        rows, C = xm.shape
        dx, dres, dgamma, dbeta = _bn_grad_buffers(ctx, xm, gamma, has_res)
        wsb = int(lib.nnl_bn_workspace_bytes(rows, C))
        ws = _workspace(wsb, xm.device)
        check(lib.nnl_bn_bwd(ptr(dym), None, ptr(mask), ptr(xm), ptr(gamma), ptr(mean), ptr(invstd), ptr(dx), ptr(dres),
                             ptr(dgamma), ptr(dbeta), rows, C, int(training), int(relu), ptr(ws), wsb, stream()))
        return _bn_grads(ctx, back, dx, dres, dgamma, dbeta) + (None,) * 10


class _SyncBNAct(torch.autograd.Function):
    """Training-mode BatchNorm with statistics over the GLOBAL batch of a data-parallel job: two kernels +
    one small all_gather forward (2C+2 floats per rank), two kernels + one all_reduce backward (2C floats).  `group` is a
    torch.distributed process group (None = WORLD); gather_fn / reduce_fn are injectable for single-process tests."""

    @staticmethod
    def forward(ctx, x, residual, gamma, beta, running_mean, running_var, momentum, eps, relu, nbt, group, comm, slot=None):
        require_cuda(x, residual, gamma, beta)
        ctx.slot = slot
        xm, back = _rows_view(x)
        rows, C = xm.shape
        rm = None if residual is None else _rows_view(residual)[0]
        dev = xm.device
        wsb = int(lib.nnl_bn_workspace_bytes(rows, C))
        ws = _workspace(wsb, dev)
        stats = torch.empty(2 * C + 2, dtype=torch.float32, device=dev)
        check(lib.nnl_bn_sync_stats(ptr(xm), ptr(stats), rows, C, ptr(ws), wsb, stream()))
        all_stats = comm.all_gather(stats, group)                  # [world, 2C+2], rank order
        world = all_stats.shape[0]
        y = torch.empty_like(xm)
        mean = torch.empty(C, dtype=torch.float32, device=dev)
        invstd = torch.empty(C, dtype=torch.float32, device=dev)
        mask = _relu_mask(rows, C, dev) if relu else None
        check(lib.nnl_bn_sync_fwd(ptr(xm), ptr(all_stats), world, ptr(gamma), ptr(beta), ptr(rm), ptr(y), ptr(mean), ptr(invstd),
                                  ptr(running_mean), ptr(running_var), rows, C, float(eps), float(momentum), int(relu), ptr(nbt),
                                  ptr(mask), ptr(ws), wsb, stream()))
        ctx.save_for_backward(xm, mask, gamma, mean, invstd, all_stats)
        ctx.cfg = (relu, residual is not None, back, group, comm)
        return back(y)

    @staticmethod
    def backward(ctx, dy):
        xm, mask, gamma, mean, invstd, all_stats = ctx.saved_tensors
        relu, has_res, back, group, comm = ctx.cfg
        dym = _rows_view(dy)[0]
        rows, C = xm.shape
        dev = xm.device
        wsb = int(lib.nnl_bn_workspace_bytes(rows, C))
        ws = _workspace(wsb, dev)
        sums = torch.empty(2 * C, dtype=torch.float32, device=dev)
        check(lib.nnl_bn_sync_bwd_reduce(ptr(dym), None, ptr(mask), ptr(xm), ptr(mean), ptr(invstd), ptr(sums), rows, C, int(relu),
                                         ptr(ws), wsb, stream()))
        total = comm.all_reduce_sum(sums, group)                   # a new tensor; `sums` keeps the local values
        dx, dres, dgamma, dbeta = _bn_grad_buffers(ctx, xm, gamma, has_res)
        check(lib.nnl_bn_sync_bwd(ptr(dym), None, ptr(mask), ptr(xm), ptr(gamma), ptr(mean), ptr(invstd), ptr(sums), ptr(total),
                                  ptr(all_stats), int(all_stats.shape[0]), ptr(dx), ptr(dres), ptr(dgamma), ptr(dbeta), rows, C,
                                  int(relu), ptr(ws), wsb, stream()))
        return _bn_grads(ctx, back, dx, dres, dgamma, dbeta) + (None,) * 9


class DistComm:
    "the two collectives SyncBN needs, over torch.distributed (RCCL on the GPUs of a node; gloo in tests)"

    @staticmethod
    def all_gather(t, group):
        import torch.distributed as dist
        w = dist.get_world_size(group)
        out = torch.empty((w,) + tuple(t.shape), dtype=t.dtype, device=t.device)
        dist.all_gather(list(out.unbind(0)), t, group=group)
        return out

    @staticmethod
    def all_reduce_sum(t, group):
        import torch.distributed as dist
        out = t.clone()
        dist.all_reduce(out, op=dist.ReduceOp.SUM, group=group)
        return out


def _bn_mode(bn):
    "(training, momentum, nbt incremented inside the finalize kernel, rmean, rvar); momentum None = cumulative average (bn_act only)"
    training = bn.training or (bn.running_mean is None)
    momentum, nbt = 0.0, None
    if bn.training and bn.track_running_stats:
        nbt, momentum = bn.num_batches_tracked, bn.momentum
    stats = not training or bn.track_running_stats
    return training, momentum, nbt, (bn.running_mean if stats else None), (bn.running_var if stats else None)


def bn_act(bn, x, residual=None, relu=True, grad_slot=None, ext_stats=None, pivot_out=None):
    """BatchNorm (train: batch statistics + running-stat update; eval: running stats) -> (+ residual) -> ReLU in the HIP
    kernels of batchnorm.hip: the bn -> `out += residual` -> relu tail of BasicBlock / Bottleneck (reference
    retinanet.py:47-48,53-57,81-95), the stem (:372-373) and the BatchNorm1d layers (General/Layers.py:40).
    `bn` is the nn.BatchNorm{1,2}d module holding weight / bias / running stats (state_dict unchanged).  A module marked by
    dist.enable_sync_bn (`bn.nnl_sync = (group, comm)`) uses global-batch statistics in training mode."""
    training, momentum, nbt, rmean, rvar = _bn_mode(bn)
    if momentum is None:                                   # cumulative moving average: the factor needs the count on the host
        nbt.add_(1)
        momentum, nbt = 1.0 / float(nbt.item()), None
    sync = getattr(bn, 'nnl_sync', None)
    if sync is not None and training:
        return _SyncBNAct.apply(x, residual, bn.weight, bn.bias, rmean, rvar, momentum, bn.eps, relu, nbt, sync[0], sync[1],
                                grad_slot)
    ext = ext_stats if (ext_stats is not None and training and ext_stats[0].numel() > 0) else None
    return _BNAct.apply(x, residual, bn.weight, bn.bias, rmean, rvar, training, momentum, bn.eps, relu, nbt, grad_slot, ext,
                        pivot_out if training else None)


class _ConcatPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        require_cuda(x)
        xn = to_nhwc(x.float())
        N, H, W, C = xn.shape
        out = torch.empty(N, 2 * C, dtype=torch.float32, device=x.device)
        am = torch.empty(N, C, dtype=torch.int32, device=x.device)
        check(lib.nnl_concat_pool_fwd(ptr(xn), ptr(out), ptr(am), N, H * W, C, stream()))
        ctx.save_for_backward(am)
        ctx.shape = (N, H, W, C)
        return out.view(N, 2 * C, 1, 1)

    @staticmethod
    def backward(ctx, dout):
        (am,) = ctx.saved_tensors
        N, H, W, C = ctx.shape
        dx = torch.empty(N, H, W, C, dtype=torch.float32, device=dout.device)
        check(lib.nnl_concat_pool_bwd(ptr(_f32c(dout.reshape(N, 2 * C))), ptr(am), ptr(dx), N, H * W, C, stream()))
        return from_nhwc(dx)


def conv_bn_act(conv, bn, x, residual=None, relu=True, conv_slot=None, bn_slot=None, conv_give=None):
    """bn_act(bn, conv(x), residual, relu) for a HipConv2d followed by BatchNorm — the conv -> bn -> (+shortcut) -> relu unit of the
    ResNet blocks (retinanet.py:43-59,77-97,304-306).  In training mode the convolution's epilogue reduces the batch statistics
    as shifted sums sum(y - pivot), sum((y - pivot)^2), so the BatchNorm does not re-read the activation for them.  The pivot is
    the batch mean of the PREVIOUS training step of this layer (kept in `bn._nnl_pivot`, written by the finalize kernel): it
    sits within a fraction of a standard deviation of the new mean, which keeps the variance free of cancellation; the first
    step (no pivot yet) runs the stand-alone statistics pass."""
    fuse = (bn.training and bn.track_running_stats and bn.running_mean is not None and bn.momentum is not None
            and getattr(bn, 'nnl_sync', None) is None and x.is_cuda and conv.bias is None and not conv.fuse_relu
            and torch.is_grad_enabled() and os.environ.get('NNL_BN_EPI_STATS', '1') != '0')

    def unfused(**kw):
        return bn_act(bn, conv(x, grad_slot=conv_slot, give_slot=conv_give), residual=residual, relu=relu, grad_slot=bn_slot, **kw)
    if not fuse:
        return unfused()
    pivot = getattr(bn, '_nnl_pivot', None)
    if pivot is None or pivot.device != x.device or pivot.numel() != bn.num_features:
        if torch.cuda.is_current_stream_capturing():
            return unfused()
        pivot = torch.empty(bn.num_features, dtype=torch.float32, device=x.device)
        object.__setattr__(bn, '_nnl_pivot', pivot)                  # plain attribute: not a buffer, not in the state_dict
        return unfused(pivot_out=pivot)
    y, part = conv2d_with_bn_stats(x, conv.weight, None, conv.stride[0], conv.padding[0], pivot, conv_slot, conv_give)
    return bn_act(bn, y, residual=residual, relu=relu, grad_slot=bn_slot, ext_stats=(part, pivot), pivot_out=pivot)


def linear_relu_bn(lin, bn, x):
    """bn(relu(lin(x))) — the Linear block of FullyConnectedNet (reference General/Layers.py:37-41: Linear -> ReLU -> BatchNorm1d, BN
    AFTER the ReLU).  In training mode the GEMM's epilogue reduces the batch statistics of relu(x W^T + b) as shifted sums (as
    conv_bn_act does for convolutions), so the BatchNorm1d does not re-read the activation for them."""
    fuse = (bn.training and bn.track_running_stats and bn.running_mean is not None and bn.momentum is not None
            and getattr(bn, 'nnl_sync', None) is None and x.is_cuda and x.dim() == 2 and torch.is_grad_enabled()
            and os.environ.get('NNL_BN_EPI_STATS', '1') != '0')
    pivot = getattr(bn, '_nnl_pivot', None) if fuse else None
    if not fuse or pivot is None or pivot.device != x.device or pivot.numel() != bn.num_features:
        y = linear(x, lin.weight, lin.bias, relu=True)
        if not fuse or torch.cuda.is_current_stream_capturing():
            return bn_act(bn, y, relu=False)
        pivot = torch.empty(bn.num_features, dtype=torch.float32, device=x.device)
        object.__setattr__(bn, '_nnl_pivot', pivot)                  # plain attribute: not a buffer, not in the state_dict
        return bn_act(bn, y, relu=False, pivot_out=pivot)
    y, part = _conv(x[:, :, None, None], lin.weight[:, :, None, None], lin.bias, relu=1, bn_pivot=pivot)
    return bn_act(bn, y.reshape(x.shape[0], lin.weight.shape[0]), relu=False, ext_stats=(part, pivot), pivot_out=pivot)


def concat_pool2d(x):
    """cat([AdaptiveMaxPool2d(1), AdaptiveAvgPool2d(1)], 1) -> [N, 2C, 1, 1]  (AdaptiveConcatPool2d, General/Layers.py:78-87);
    the max gradient goes to the first arg-max pixel, as torch's adaptive max pool does (pool.hip)."""
    return _ConcatPool.apply(x)


def pool_out_size(H, ksize, stride, pad, ceil_mode=False):
    """nn.MaxPool2d's output size along one axis.  ceil_mode (the SENet stem pool, senet.py:314-315): torch's rule — round up, then drop
    a last window that would start beyond the input plus its left padding."""
    if not ceil_mode:
        return (H + 2 * pad - ksize) // stride + 1
    out = -((H + 2 * pad - ksize) // -stride) + 1
    return out - 1 if (out - 1) * stride >= H + pad else out


class _MaxPool2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ksize, stride, pad, ceil_mode=False):
        require_cuda(x)
        xn = to_nhwc(x.float())
        N, H, W, C = xn.shape
        P, Q = pool_out_size(H, ksize, stride, pad, ceil_mode), pool_out_size(W, ksize, stride, pad, ceil_mode)
        y = torch.empty(N, P, Q, C, dtype=torch.float32, device=x.device)
        idx = torch.empty(N, P, Q, C, dtype=torch.uint8, device=x.device)
        check(lib.nnl_maxpool2d_fwd(ptr(xn), ptr(y), ptr(idx), N, H, W, C, P, Q, ksize, stride, pad, stream()))
        ctx.save_for_backward(idx)
        ctx.cfg = (N, H, W, C, P, Q, ksize, stride, pad)
        return from_nhwc(y)

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        N, H, W, C, P, Q, ksize, stride, pad = ctx.cfg
        dyn = to_nhwc(dy.float())
        dx = torch.empty(N, H, W, C, dtype=torch.float32, device=dy.device)
        check(lib.nnl_maxpool2d_bwd(ptr(dyn), ptr(idx), ptr(dx), N, H, W, C, P, Q, ksize, stride, pad, stream()))
        return from_nhwc(dx), None, None, None, None


class _BNReLUMaxPool(torch.autograd.Function):
    """maxpool(relu(batch_norm(x))) — the ResNet stem tail (reference retinanet.py:372-374) — without materialising the
    normalised activation: batchnorm.hip nnl_bn_relu_maxpool_{fwd,bwd}.  Saves x (the conv output), the uint8 window index and
    the per-channel affine."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, training, momentum, eps, nbt, ksize, stride, pad):
        require_cuda(x, gamma, beta)
        xn = to_nhwc(x.float())
        N, H, W, C = xn.shape
        P, Q = (H + 2 * pad - ksize) // stride + 1, (W + 2 * pad - ksize) // stride + 1
        dev = x.device
        y = torch.empty(N, P, Q, C, dtype=torch.float32, device=dev)
        idx = torch.empty(N, P, Q, C, dtype=torch.uint8, device=dev)
        stats = torch.empty(4, C, dtype=torch.float32, device=dev)               # mean, invstd, scale, shift
        wsb = int(lib.nnl_bn_workspace_bytes(N * H * W, C))
        ws = _workspace(wsb, dev)
        check(lib.nnl_bn_relu_maxpool_fwd(ptr(xn), ptr(gamma), ptr(beta), ptr(y), ptr(idx), ptr(stats[0]), ptr(stats[1]),
                                          ptr(stats[2]), ptr(stats[3]), ptr(running_mean), ptr(running_var), N, H, W, C, P, Q,
                                          ksize, stride, pad, float(eps), float(momentum), int(training), ptr(nbt), ptr(ws), wsb,
                                          stream()))
        ctx.save_for_backward(xn, idx, gamma, beta, stats, y)
        ctx.cfg = (N, H, W, C, P, Q, ksize, stride, pad, training)
        return from_nhwc(y)

    @staticmethod
    def backward(ctx, dy):
        xn, idx, gamma, beta, stats, y = ctx.saved_tensors
        N, H, W, C, P, Q, ksize, stride, pad, training = ctx.cfg
        dyn = to_nhwc(dy.float())
        dx = torch.empty_like(xn)
        dgamma = torch.empty(C, dtype=torch.float32, device=xn.device) if gamma is not None else None
        dbeta = torch.empty(C, dtype=torch.float32, device=xn.device) if gamma is not None else None
        wsb = int(lib.nnl_bn_workspace_bytes(N * H * W, C))
        ws = _workspace(wsb, xn.device)
        check(lib.nnl_bn_relu_maxpool_bwd(ptr(dyn), ptr(y), ptr(idx), ptr(xn), ptr(gamma), ptr(beta), ptr(stats[0]), ptr(stats[1]),
                                          ptr(stats[2]), ptr(stats[3]), ptr(dx), ptr(dgamma), ptr(dbeta), N, H, W, C, P, Q, ksize, stride, pad,
                                          int(training), ptr(ws), wsb, stream()))
        return (from_nhwc(dx), dgamma, dbeta) + (None,) * 9


def conv_bn_relu_maxpool(conv, bn, pool, x):
    """pool(relu(bn(conv(x)))) for the ResNet stem (conv7x7/2 -> BatchNorm -> ReLU -> MaxPool 3/2/1; reference
    retinanet.py:304-307,371-374).  BatchNorm, ReLU and the pooling run as one pass over the convolution output whenever the
    pooling is the plain floor-mode square max-pool and the BatchNorm is a local (non-synchronised) one; otherwise the three
    stages run one after the other."""
    k, s, p = pool.kernel_size, pool.stride, pool.padding
    fuse = (x.is_cuda and isinstance(pool, torch.nn.MaxPool2d) and all(isinstance(v, int) for v in (k, s, p))
            and pool.dilation == 1 and not pool.ceil_mode and not pool.return_indices and 2 * p <= k and k * k <= 255
            and not (bn.training and getattr(bn, 'nnl_sync', None) is not None)
            and (bn.running_mean is not None or bn.training)
            and not (bn.training and bn.track_running_stats and bn.momentum is None)
            and bool(lib.nnl_bn_relu_maxpool_supported(bn.num_features)))
    if not fuse:
        return pool(conv_bn_act(conv, bn, x, relu=True))
    y = conv(x)
    training, momentum, nbt, rmean, rvar = _bn_mode(bn)    # (momentum is not None: the cumulative average was refused above)
    return _BNReLUMaxPool.apply(y, bn.weight, bn.bias, rmean, rvar, training, momentum, bn.eps, nbt, k, s, p)


def maxpool2d(x, ksize=3, stride=2, pad=1, ceil_mode=False):
    """nn.MaxPool2d(ksize, stride, pad, ceil_mode=ceil_mode) (no dilation) — the ResNet stem pool (retinanet.py:307,374), in ceil
    mode the SENet one (senet.py:314-315) and NASNet's MaxPoolPad (nasnet.py:65-76, as ksize 3 / stride 2 / pad 0) — NHWC, any channel
    count (4-channel vectors when it is a multiple of 4, a scalar-channel route otherwise); torch's first-maximum tie rule, deterministic
    gather-style backward (pool.hip).  ceil_mode changes the output size only: the kernels skip the taps outside the input."""
    return _MaxPool2d.apply(x, int(ksize), int(stride), int(pad), bool(ceil_mode))


# ---------------------------------------------------------------------------------------------------------
# K15 grouped convolution and squeeze-excite (the SENet family, Applications/VisionModels/senet.py)
# ---------------------------------------------------------------------------------------------------------
def _gconv_check(x_shape, w_shape, stride, pad, groups):
    "the domain of csrc/gconv.hip, checked before any launch (and before any device is needed): names the offending argument"
    if len(x_shape) != 4 or len(w_shape) != 4:
        raise NotImplementedError('grouped_conv2d: x %s and weight %s must be 4-D' % (tuple(x_shape), tuple(w_shape)))
    C, (K, Cg, R, S) = x_shape[1], w_shape
    if R != S or R not in (1, 3):
        raise NotImplementedError('grouped_conv2d: kernel_size %dx%d is not supported (1x1 or 3x3)' % (R, S))
    if stride not in (1, 2):
        raise NotImplementedError('grouped_conv2d: stride %r is not supported (1 or 2)' % (stride,))
    if pad not in (0, 1) or pad > R // 2:
        raise NotImplementedError('grouped_conv2d: padding %r is not supported (0 .. kernel_size // 2)' % (pad,))
    if groups < 1 or C % groups or K % groups or C // groups != Cg:
        raise NotImplementedError('grouped_conv2d: groups %r must divide the %d input and %d output channels (weight holds %d inputs per group)'
                                  % (groups, C, K, Cg))


class _GroupedConv2d(torch.autograd.Function):
    """nn.Conv2d(groups=G) forward / backward (reference Applications/VisionModels/senet.py:178-180, 205-206, 229-230) on the direct
    kernels of csrc/gconv.hip; optional fused bias + ReLU epilogue.  Plain autograd: no GradSlot, no prepared filters."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, pad, groups, relu):
        _gconv_check(x.shape, weight.shape, stride, pad, groups)
        require_cuda(x, weight, bias)
        xn, wn = to_nhwc(x.float()), to_nhwc(weight.float())                 # (no copy: both are stored channels_last)
        b = None if bias is None else _f32c(bias)
        N, H, W, C = xn.shape
        K, R = wn.shape[0], wn.shape[1]
        g = _geom(N, H, W, C, K, R, R, stride, pad)
        y = torch.empty((N, g.P, g.Q, K), dtype=torch.float32, device=x.device)
        check(lib.nnl_gconv2d_fwd(ptr(xn), ptr(wn), ptr(b), ptr(y), N, H, W, C, K, groups, R, stride, pad, int(relu), stream()))
        ctx.cfg = (g, groups, bool(relu), bias is not None)
        ctx.save_for_backward(xn, wn, y if relu else None)
        return from_nhwc(y)

    @staticmethod
    def backward(ctx, dy):
        xn, wn, y = ctx.saved_tensors
        g, groups, relu, has_bias = ctx.cfg
        dims = (g.N, g.H, g.W, g.C, g.K, groups, g.R, g.stride, g.pad)
        want_db = has_bias and ctx.needs_input_grad[2]
        dyn, db = to_nhwc(dy.float()), None
        if relu:
            dyn, db = _conv_act_gate(y, dyn, g, 1, want_db)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(xn)
            check(lib.nnl_gconv2d_dgrad(ptr(dyn), ptr(wn), ptr(dx), *dims, stream()))
            dx = from_nhwc(dx)
        if ctx.needs_input_grad[1]:
            dw = torch.empty_like(wn)                                        # [K, R, R, Cg]: the parameter's own layout
            wsb = int(lib.nnl_gconv2d_workspace_bytes(*dims))
            ws = _workspace(wsb, dyn.device)
            check(lib.nnl_gconv2d_wgrad(ptr(xn), ptr(dyn), ptr(dw), ptr(ws), wsb, *dims, stream()))
            dw = from_nhwc(dw)
        if db is None and want_db:
            db = _conv_bias_grad(dyn, g, g.K)
        return dx, dw, db, None, None, None, None


def grouped_conv2d(x, weight, bias, stride, pad, groups, relu=False):
    """y = [relu](conv2d(x, weight, bias, stride, padding=pad, groups=groups)); x logical [N,C,H,W], weight [K, C/groups, R, R] stored
    channels_last.  Domain: R in {1, 3}, stride in {1, 2}, pad in {0, 1} and <= R // 2, groups divides C and K; anything else raises
    NotImplementedError naming the argument."""
    return _GroupedConv2d.apply(x, weight, bias, int(stride), int(pad), int(groups), bool(relu))


class _SEExcite(torch.autograd.Function):
    """relu(x * sigmoid(fc2(relu(fc1(mean_hw(x))))) + residual): SEModule plus the block's closing add and ReLU (reference
    Applications/VisionModels/senet.py:118-137, 161-162) — squeeze, the scaling pass and their backward in csrc/se.hip, the two FCs
    through `linear` on the [N, C] matrix (their backward is the recorded graph of those two calls)."""

    @staticmethod
    def forward(ctx, x, residual, w1, b1, w2, b2):
        require_cuda(x, residual, w1, b1, w2, b2)
        xn = to_nhwc(x.float())
        rn = None if residual is None else to_nhwc(residual.float())
        N, H, W, C = xn.shape
        if rn is not None and rn.shape != xn.shape:
            raise _lib.NnlError('se_excite: residual %s does not match x %s' % (tuple(residual.shape), tuple(x.shape)))
        m = torch.empty(N, C, dtype=torch.float32, device=x.device)
        check(lib.nnl_se_squeeze(ptr(xn), ptr(m), N, H * W, C, stream()))
        track = any(ctx.needs_input_grad)
        with torch.enable_grad() if track else contextlib.nullcontext():
            if track:
                m.requires_grad_(True)
            z = linear(linear(m, w1.reshape(w1.shape[0], C), b1, relu=True), w2.reshape(C, w2.shape[1]), b2)
        zd = _f32c(z.detach())
        out = torch.empty_like(xn)
        check(lib.nnl_se_excite_fwd(ptr(xn), ptr(zd), ptr(rn), ptr(out), N, H * W, C, stream()))
        ctx.fc = (m, z, (w1, b1, w2, b2)) if track else None
        ctx.has_res = rn is not None
        ctx.save_for_backward(xn, zd, out)
        return from_nhwc(out)

    @staticmethod
    def backward(ctx, dy):
        xn, zd, out = ctx.saved_tensors
        N, H, W, C = xn.shape
        dyn = to_nhwc(dy.float())
        dx, dz = torch.empty_like(xn), torch.empty_like(zd)
        dres = torch.empty_like(xn) if (ctx.has_res and ctx.needs_input_grad[1]) else None
        check(lib.nnl_se_excite_bwd(ptr(dyn), ptr(out), ptr(xn), ptr(zd), ptr(dx), ptr(dres), ptr(dz), N, H * W, C, stream()))
        m, z, params = ctx.fc
        ctx.fc = None
        live = [p is not None and p.requires_grad for p in params]
        grads = iter(torch.autograd.grad(z, [m] + [p for p, on in zip(params, live) if on], dz, allow_unused=True))
        dm = next(grads)
        if ctx.needs_input_grad[0]:
            check(lib.nnl_se_squeeze_bwd(ptr(_f32c(dm)), ptr(dx), N, H * W, C, stream()))
        dparams = tuple(next(grads) if on else None for on in live)
        return ((from_nhwc(dx) if ctx.needs_input_grad[0] else None), (None if dres is None else from_nhwc(dres))) + dparams


def se_excite(x, fc1, fc2, residual=None):
    """relu(x * sigmoid(fc2(relu(fc1(avg_pool(x))))) + residual) for the 1x1 convolutions fc1 [C/r, C, 1, 1] and fc2 [C, C/r, 1, 1]
    (with bias) of an SEModule; residual None = no shortcut term.  x logical [N,C,H,W], C a multiple of 4."""
    return _SEExcite.apply(x, residual, fc1.weight, fc1.bias, fc2.weight, fc2.bias)


# ---------------------------------------------------------------------------------------------------------
# K18 depthwise convolution, average pooling and strided subsampling (NASNet-A-Large, Applications/VisionModels/nasnet.py)
# ---------------------------------------------------------------------------------------------------------
def fold_zero_pad(H, R, stride, pad, z):
    """(pad_lo, P) of the single window op that equals `ZeroPad2d((z, 0, z, 0))` -> a window op (kernel R, `stride`, symmetric padding
    `pad`) -> `[1:, 1:]` along an axis of H (reference nasnet.py:65-90, 152-167).  Output i of the chain is output i + 1 of the op on the
    padded axis, whose window starts at (i + 1) stride - pad - z in the un-padded coordinates: pad_lo = pad + z - stride; and the chain
    keeps (H + z + 2 pad - R) // stride + 1 - 1 outputs.  At R = 3, stride = pad = z = 1 it degenerates to the plain op (1, H)."""
    return pad + z - stride, (H + z + 2 * pad - R) // stride


def _window_args(H, W, R, stride, pad, pad_lo, out_size):
    "(pad_lo, P, Q) of a window op: symmetric `pad` unless pad_lo / out_size state the folded form"
    if pad_lo is None:
        pad_lo = pad
    if out_size is None:
        P, Q = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
    else:
        P, Q = (out_size, out_size) if isinstance(out_size, int) else out_size
    return int(pad_lo), int(P), int(Q)


def _window_check(who, x_shape, R, rmax_text, r_ok, stride, stride_ok, pad, pad_lo, out_size):
    "the shared domain of csrc/dwconv.hip and the average pool, checked before any device is needed: names the offending argument"
    if len(x_shape) != 4:
        raise NotImplementedError('%s: x %s must be 4-D' % (who, tuple(x_shape)))
    if not r_ok:
        raise NotImplementedError('%s: kernel_size %r is not supported (%s)' % (who, R, rmax_text))
    if not stride_ok:
        raise NotImplementedError('%s: stride %r is not supported' % (who, stride))
    if not isinstance(pad, int) or pad < 0 or pad > R // 2:
        raise NotImplementedError('%s: padding %r is not supported (0 .. kernel_size // 2)' % (who, pad))
    H, W = x_shape[2], x_shape[3]
    lo, P, Q = _window_args(H, W, R, stride, pad, pad_lo, out_size)
    if lo < 0 or lo > R - 1:
        raise NotImplementedError('%s: pad_lo %r is not supported (0 .. kernel_size - 1)' % (who, lo))
    if P < 1 or Q < 1 or (P - 1) * stride - lo > H - 1 or (Q - 1) * stride - lo > W - 1:
        raise NotImplementedError('%s: out_size %r is not supported: every window must touch the %d x %d input' % (who, (P, Q), H, W))
    return lo, P, Q


def _dwconv_check(x_shape, w_shape, stride, pad, pad_lo, out_size):
    if len(w_shape) != 4:
        raise NotImplementedError('depthwise_conv2d: weight %s must be 4-D' % (tuple(w_shape),))
    K, Cg, R, S = w_shape
    if len(x_shape) == 4 and (K != x_shape[1] or Cg != 1):
        raise NotImplementedError('depthwise_conv2d: weight %s is not depthwise for %d input channels (groups == in_channels == '
                                  'out_channels)' % (tuple(w_shape), x_shape[1]))
    return _window_check('depthwise_conv2d', x_shape, R, '3x3, 5x5 or 7x7', R == S and R in (3, 5, 7), stride, stride in (1, 2), pad,
                         pad_lo, out_size)


def _avgpool_check(x_shape, ksize, stride, pad, pad_lo, out_size):
    return _window_check('avgpool2d', x_shape, ksize, 'an int in 1 .. 15', isinstance(ksize, int) and 1 <= ksize <= 15, stride,
                         isinstance(stride, int) and stride >= 1, pad, pad_lo, out_size)


class _DepthwiseConv2d(torch.autograd.Function):
    """nn.Conv2d(C, C, R, groups=C) forward / backward (reference nasnet.py:93-107) on csrc/dwconv.hip, with the input ReLU of a
    BranchSeparables fused into the load.  Plain autograd: no GradSlot, no prepared filters."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, pad, pad_lo, out_size, relu_in):
        lo, P, Q = _dwconv_check(x.shape, weight.shape, stride, pad, pad_lo, out_size)
        require_cuda(x, weight, bias)
        xn, wn = to_nhwc(x.float()), _f32c(weight)                           # weight [C, 1, R, R] as stored
        b = None if bias is None else _f32c(bias)
        N, H, W, C = xn.shape
        R = wn.shape[2]
        y = torch.empty((N, P, Q, C), dtype=torch.float32, device=x.device)
        check(lib.nnl_dwconv2d_fwd(ptr(xn), ptr(wn), ptr(b), ptr(y), N, H, W, C, P, Q, R, stride, lo, int(relu_in), stream()))
        ctx.cfg = (N, H, W, C, P, Q, R, stride, lo, int(relu_in), bias is not None)
        ctx.save_for_backward(xn, wn)
        return from_nhwc(y)

    @staticmethod
    def backward(ctx, dy):
        xn, wn = ctx.saved_tensors
        dims, relu_in, has_bias = ctx.cfg[:9], ctx.cfg[9], ctx.cfg[10]
        N, H, W, C, P, Q = dims[:6]
        dyn = to_nhwc(dy.float())
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(xn)
            check(lib.nnl_dwconv2d_dgrad(ptr(dyn), ptr(wn), ptr(xn), ptr(dx), *dims, relu_in, stream()))
            dx = from_nhwc(dx)
        if ctx.needs_input_grad[1]:
            dw = torch.empty_like(wn)
            wsb = int(lib.nnl_dwconv2d_wgrad_workspace_bytes(*dims))
            ws = _workspace(wsb, dyn.device)
            check(lib.nnl_dwconv2d_wgrad(ptr(xn), ptr(dyn), ptr(dw), ptr(ws), wsb, *dims, relu_in, stream()))
        if has_bias and ctx.needs_input_grad[2]:
            db = torch.empty(C, dtype=torch.float32, device=dyn.device)
            cb = int(lib.nnl_colsum_workspace_bytes(N * P * Q, C))
            cws = _workspace(cb, dyn.device, floor=True)
            check(lib.nnl_colsum(ptr(dyn), ptr(db), N * P * Q, C, ptr(cws), cb, stream()))
        return dx, dw, db, None, None, None, None, None


def depthwise_conv2d(x, weight, bias, stride, pad, pad_lo=None, out_size=None, relu_in=False):
    """y = conv2d([relu](x), weight, bias, stride, padding=pad, groups=C); x logical [N,C,H,W], weight [C, 1, R, R].  Domain: R in
    {3, 5, 7}, stride in {1, 2}, any C.  pad_lo / out_size state an asymmetric form instead (tap r of output p reads row p stride -
    pad_lo + r; out_size = P or (P, Q)): see fold_zero_pad.  Anything else raises NotImplementedError naming the argument."""
    return _DepthwiseConv2d.apply(x, weight, bias, int(stride), pad, pad_lo, out_size, bool(relu_in))


class _AvgPool2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ksize, stride, pad, count_include_pad, pad_lo, out_size):
        lo, P, Q = _avgpool_check(x.shape, ksize, stride, pad, pad_lo, out_size)
        require_cuda(x)
        xn = to_nhwc(x.float())
        N, H, W, C = xn.shape
        y = torch.empty((N, P, Q, C), dtype=torch.float32, device=x.device)
        ctx.cfg = (N, H, W, C, P, Q, ksize, stride, lo, int(count_include_pad))
        check(lib.nnl_avgpool2d_fwd(ptr(xn), ptr(y), *ctx.cfg, stream()))
        return from_nhwc(y)

    @staticmethod
    def backward(ctx, dy):
        N, H, W, C = ctx.cfg[:4]
        dyn = to_nhwc(dy.float())
        dx = torch.empty((N, H, W, C), dtype=torch.float32, device=dy.device)
        check(lib.nnl_avgpool2d_bwd(ptr(dyn), ptr(dx), *ctx.cfg, stream()))
        return from_nhwc(dx), None, None, None, None, None, None


def avgpool2d(x, ksize, stride, pad, count_include_pad=True, pad_lo=None, out_size=None):
    """nn.AvgPool2d(ksize, stride, pad, count_include_pad=...) (floor mode), NHWC, any channel count (pool.hip); pad_lo / out_size as
    for depthwise_conv2d.  ksize 1 .. 15; anything else raises NotImplementedError naming the argument."""
    return _AvgPool2d.apply(x, ksize, stride, pad, bool(count_include_pad), pad_lo, out_size)


def _subsample_check(x_shape, stride, off):
    if len(x_shape) != 4:
        raise NotImplementedError('subsample2d: x %s must be 4-D' % (tuple(x_shape),))
    if not isinstance(stride, int) or stride < 1:
        raise NotImplementedError('subsample2d: stride %r is not supported (an int >= 1)' % (stride,))
    if not isinstance(off, int) or off < 0 or off >= max(stride, 2):
        raise NotImplementedError('subsample2d: off %r is not supported (0 .. stride - 1)' % (off,))


class _Subsample2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, stride, off):
        _subsample_check(x.shape, stride, off)
        require_cuda(x)
        xn = to_nhwc(x.float())
        N, H, W, C = xn.shape
        P, Q = (H - 1) // stride + 1, (W - 1) // stride + 1
        y = torch.empty((N, P, Q, C), dtype=torch.float32, device=x.device)
        ctx.cfg = (N, H, W, C, P, Q, stride, off)
        check(lib.nnl_subsample2d_fwd(ptr(xn), ptr(y), *ctx.cfg, stream()))
        return from_nhwc(y)

    @staticmethod
    def backward(ctx, dy):
        N, H, W, C = ctx.cfg[:4]
        dyn = to_nhwc(dy.float())
        dx = torch.empty((N, H, W, C), dtype=torch.float32, device=dy.device)
        check(lib.nnl_subsample2d_bwd(ptr(dyn), ptr(dx), *ctx.cfg, stream()))
        return from_nhwc(dx), None, None


def subsample2d(x, stride, off):
    """y[p, q] = x[p stride + off, q stride + off] (0 outside the image), (H - 1) // stride + 1 outputs per axis: AvgPool2d(1, stride)
    for off = 0, and the ZeroPad2d((0, 1, 0, 1)) -> [1:, 1:] -> AvgPool2d(1, 2) chain of nasnet.py:232-238, 263-266 for off = 1."""
    return _Subsample2d.apply(x, stride, off)


# ---------------------------------------------------------------------------------------------------------
# K3 tabular front end
# ---------------------------------------------------------------------------------------------------------
class TabularPlan:
    """Device-side descriptor arrays for a list of embedding tables (see include/nnl.h, K3).  Rebuilt when a table
    moves (data_ptr / device change)."""

    def __init__(self, weights):
        dev = weights[0].device
        self.key = tuple((w.data_ptr(), tuple(w.shape)) for w in weights) + (str(dev),)
        self.sync = None
        card = [int(w.shape[0]) for w in weights]
        dim = [int(w.shape[1]) for w in weights]
        self.ncat, self.cat_width, self.total_rows = len(weights), sum(dim), sum(card)
        col_off = np.concatenate([[0], np.cumsum(dim)[:-1]]).astype(np.int32)
        row_off = np.concatenate([[0], np.cumsum(card)[:-1]]).astype(np.int32)
        sizes = [c * d for c, d in zip(card, dim)]
        self.grad_sizes, self.shapes = sizes, [tuple(w.shape) for w in weights]
        grad_off = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        self.grad_elems = int(sum(sizes))
        t = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt).to(dev)
        self.ptrs = t(np.array([w.data_ptr() for w in weights], dtype=np.int64), torch.int64)
        self.card, self.dim = t(card, torch.int32), t(dim, torch.int32)
        self.col_off, self.row_off, self.grad_off = t(col_off, torch.int32), t(row_off, torch.int32), t(grad_off, torch.int64)
        self.col_table = t(np.repeat(np.arange(self.ncat), dim), torch.int32)
        self.row_table = t(np.repeat(np.arange(self.ncat), card), torch.int32)
        self.flags = torch.zeros(self.total_rows, dtype=torch.int32, device=dev)
        # sort-free backward (nnl_tab_scan_bwd): 256 flat gradient elements of ONE column per block
        self.max_dim = max(dim) if dim else 0
        blk_col, blk_first = [], []
        for j, n in enumerate(sizes):
            for f in range(0, n, 256):
                blk_col.append(j)
                blk_first.append(f)
        self.n_scan_blocks = len(blk_col)
        self.blk_col, self.blk_first = t(blk_col or [0], torch.int32), t(blk_first or [0], torch.int32)

    @staticmethod
    def for_weights(weights, cached=None):
        key = tuple((w.data_ptr(), tuple(w.shape)) for w in weights) + (str(weights[0].device),)
        return cached if (cached is not None and cached.key == key) else TabularPlan(weights)


class _TabEmbedConcat(torch.autograd.Function):
    """StructuredDataNet.forward front end (reference Applications/StructuredData.py:1074-1082 + General/Layers.py:74-76)."""

    @staticmethod
    def forward(ctx, xcat, cont, row_mask, cont_mask, plan, max_norm, *weights):
        require_cuda(xcat, cont, *weights)
        for w in weights:
            if not (w.is_contiguous() and w.dtype == torch.float32):
                raise _lib.NnlError('tab_embed_concat: embedding tables must be contiguous fp32 parameters')
        xcat = xcat.contiguous().long()
        bs = xcat.shape[0]
        n_cont = 0 if cont is None else cont.shape[1]
        cont = None if cont is None else _f32c(cont)
        row_mask = None if row_mask is None else _f32c(row_mask)
        cont_mask = None if cont_mask is None else _f32c(cont_mask)
        if max_norm is not None:
            # data parallel: the in-place renorm must hit the rows looked up by ANY rank, or the replicas' tables diverge
            # (Learner's replayed data-parallel step gathers them BEFORE the graph — StructuredDataNet.nnl_dp_prepare — and hands the
            # static buffer over as a fourth element: no collective inside the captured forward)
            if plan.sync is None:
                xren = xcat
            elif len(plan.sync) > 3 and plan.sync[3] is not None:
                xren = plan.sync[3]
            else:
                xren = _global_lookup_indices(xcat, plan.sync[:3])
            check(lib.nnl_tab_renorm(ptr(xren), ptr(plan.ptrs), ptr(plan.card), ptr(plan.dim), ptr(plan.row_off),
                                     ptr(plan.row_table), ptr(plan.flags), xren.shape[0], plan.ncat, plan.total_rows,
                                     float(max_norm), ptr(index_error_flag(xcat.device)), stream()))
        ld = plan.cat_width + n_cont
        out = torch.empty(bs, ld, dtype=torch.float32, device=xcat.device)
        check(lib.nnl_tab_gather_fwd(ptr(xcat), ptr(plan.ptrs), ptr(plan.card), ptr(plan.dim), ptr(plan.col_off),
                                     ptr(plan.col_table), ptr(row_mask), ptr(cont), ptr(cont_mask), ptr(out), bs, plan.ncat,
                                     plan.cat_width, n_cont, ld, stream()))
        ctx.save_for_backward(xcat, row_mask, cont_mask)
        ctx.plan, ctx.n_cont = plan, n_cont
        return out

    @staticmethod
    def backward(ctx, dout):
        xcat, row_mask, cont_mask = ctx.saved_tensors
        plan, n_cont = ctx.plan, ctx.n_cont
        bs = xcat.shape[0]
        flat = torch.empty(max(plan.grad_elems, 1), dtype=torch.float32, device=dout.device)
        dcont = torch.empty(bs, n_cont, dtype=torch.float32, device=dout.device) if (n_cont and ctx.needs_input_grad[1]) else None
        # (the scan costs gradient elements x minibatch compares — Rossmann: 7e4 x 1024; tables of 1e5+ rows go to the sorted scatter)
        if plan.ncat and bs and 0 < plan.max_dim <= 32 and plan.grad_elems * bs <= (1 << 28) and os.environ.get('NNL_TAB_SCAN', '1') != '0':
            # one launch, no sort, no zero fill; a row-strided gradient (the slice of a channel-padded buffer) is read in place
            if not (dout.dtype == torch.float32 and dout.dim() == 2 and dout.stride(1) == 1 and dout.stride(0) >= dout.shape[1]):
                dout = _f32c(dout)
            check(lib.nnl_tab_scan_bwd(ptr(xcat), ptr(plan.card), ptr(plan.dim), ptr(plan.col_off), ptr(plan.grad_off), ptr(row_mask),
                                       ptr(cont_mask), ptr(dout), ptr(flat), ptr(dcont), ptr(plan.blk_col), ptr(plan.blk_first),
                                       plan.n_scan_blocks, plan.max_dim, bs, plan.ncat, plan.cat_width, n_cont, dout.stride(0), stream()))
        else:
            dout = _f32c(dout)
            wsb = int(lib.nnl_tab_scatter_bwd_workspace_bytes(bs, plan.ncat))            # sample-order (deterministic) scatter-add
            ws = _workspace(wsb, dout.device, floor=True)                                # never a null
            check(lib.nnl_tab_scatter_bwd(ptr(xcat), ptr(plan.card), ptr(plan.dim), ptr(plan.col_off), ptr(plan.col_table),
                                          ptr(plan.grad_off), ptr(row_mask), ptr(cont_mask), ptr(dout), ptr(flat), plan.grad_elems,
                                          ptr(dcont), bs, plan.ncat, plan.cat_width, n_cont, dout.shape[1], ptr(ws), wsb, stream()))
        grads, o = [], 0
        for n, shp in zip(plan.grad_sizes, plan.shapes):
            grads.append(flat[o:o + n].view(shp))
            o += n
        return (None, dcont, None, None, None, None) + tuple(grads)


def _global_lookup_indices(xcat, sync):
    """All ranks' categorical indices of this step ([sum of local batch sizes (padded), ncat]) — SURVEY.md §8e: "all-gather of
    touched embedding indices so max_norm renorm hits the same rows on every rank".  sync = (group, comm, capacity): shards
    are padded to `capacity` rows (the per-rank full batch size) so the collective has a fixed shape and needs no host
    synchronisation; padding rows are replaced by a real looked-up row (renorm is idempotent per row)."""
    group, comm, cap = sync[:3]
    bs, ncat = xcat.shape
    if bs > cap:
        raise _lib.NnlError(f'tab_embed_concat: local batch {bs} exceeds the data-parallel capacity {cap}')
    pad = torch.zeros(cap + 1, ncat, dtype=torch.int64, device=xcat.device)
    pad[:bs] = xcat
    pad[cap, 0] = bs
    g = comm.all_gather(pad, group)                                   # [world, cap + 1, ncat]
    counts, rows = g[:, cap, 0], g[:, :cap]
    valid = torch.arange(cap, device=xcat.device)[None, :] < counts[:, None]
    flat = rows.reshape(-1, ncat)
    fill = flat[valid.reshape(-1).to(torch.uint8).argmax()]             # first real row of any rank
    return torch.where(valid.reshape(-1, 1), flat, fill).contiguous()


def keep_masks(shape_a, keep_a, shape_b, keep_b, device):
    """Two scaled Bernoulli keep masks (value 0 or 1/keep) from one uniform draw and one launch; a shape may be None."""
    na = 0 if shape_a is None else int(torch.Size(shape_a).numel())
    nb = 0 if shape_b is None else int(torch.Size(shape_b).numel())
    u = torch.rand(na + nb, dtype=torch.float32, device=device)
    a = torch.empty(shape_a, dtype=torch.float32, device=device) if na else None
    b = torch.empty(shape_b, dtype=torch.float32, device=device) if nb else None
    check(lib.nnl_keep_masks(ptr(u), ptr(a), na, float(keep_a), ptr(b), nb, float(keep_b), stream()))
    return a, b


def tab_embed_concat(xcat, weights, row_mask=None, cont=None, cont_mask=None, max_norm=None, plan=None, sync=None):
    """[bs, sum(d_j) + n_cont] = cat_j( W_j[xcat[:,j]] * row_mask[j][:,None] ) ++ cont*cont_mask, after the in-place
    max_norm renorm of the looked-up rows (of all ranks' lookups when `sync` = (group, comm, capacity) is given).
    Returns (out, plan)."""
    plan = TabularPlan.for_weights(weights, plan)
    plan.sync = sync
    return _TabEmbedConcat.apply(xcat, cont, row_mask, cont_mask, plan, max_norm, *weights), plan


def embedding_renorm_drop(x, weight, mask, max_norm):
    """EmbeddingDrop.forward for ONE column (General/Layers.py:74-76): emb(x) * mask.unsqueeze(1)."""
    out, _ = tab_embed_concat(x.view(-1, 1), [weight], None if mask is None else mask.view(1, -1), None, None, max_norm)
    return out


# ---------------------------------------------------------------------------------------------------------
# K6 fused RetinaNet loss
# ---------------------------------------------------------------------------------------------------------
class _RetinaLoss(torch.autograd.Function):
    """SSD_loss.__call__ (reference Applications/Vision.py:1620-1644 and everything below it) as one fused forward
    kernel and one fused backward kernel; returns [total, reg_loss, clas_loss].  Gradient flows through `total`."""

    @staticmethod
    def forward(ctx, anchors, reg, clas, boxes, cats, beta, alpha, gamma):
        require_cuda(anchors, reg, clas, boxes, cats)
        anchors, reg, clas, boxes = _f32c(anchors), _f32c(reg), _f32c(clas), _f32c(boxes)
        cats = cats.contiguous().long()
        bs, A, K = clas.shape
        M = boxes.shape[1]
        dev = clas.device
        state = torch.empty(bs, A, dtype=torch.int32, device=dev)
        npos = torch.empty(bs, dtype=torch.float32, device=dev)
        out = torch.empty(3, dtype=torch.float32, device=dev)
        wsb = int(lib.nnl_retina_loss_workspace_bytes(bs, A))
        ws = _workspace(wsb, dev, floor=True)                   # never a null
        check(lib.nnl_retina_loss_fwd(ptr(anchors), ptr(reg), ptr(clas), ptr(boxes), ptr(cats), ptr(state), ptr(npos), ptr(out),
                                      bs, A, K, M, float(beta), float(alpha), float(gamma), ptr(ws), wsb, stream()))
        ctx.save_for_backward(anchors, reg, clas, boxes, cats, state, npos)
        ctx.hyper = (float(beta), float(alpha), float(gamma))
        return out

    @staticmethod
    def backward(ctx, dout):
        anchors, reg, clas, boxes, cats, state, npos = ctx.saved_tensors
        beta, alpha, gamma = ctx.hyper
        bs, A, K = clas.shape
        gup = _f32c(dout)[0:1].contiguous()
        dreg, dclas = torch.empty_like(reg), torch.empty_like(clas)
        check(lib.nnl_retina_loss_bwd(ptr(anchors), ptr(reg), ptr(clas), ptr(boxes), ptr(cats), ptr(state), ptr(npos), ptr(gup),
                                      ptr(dreg), ptr(dclas), bs, A, K, boxes.shape[1], beta, alpha, gamma, stream()))
        return None, dreg, dclas, None, None, None, None, None


def retina_loss(anchors, reg, clas, boxes, cats, beta=0.5, alpha=0.25, gamma=2.0):
    """[ (1-beta)*reg_loss + beta*clas_loss, reg_loss, clas_loss ] for a batch (see include/nnl.h, K6)."""
    return _RetinaLoss.apply(anchors, reg, clas, boxes, cats, beta, alpha, gamma)


# ---------------------------------------------------------------------------------------------------------
# K9 image augmentation: the classification Transform on a device-resident uint8 dataset (include/nnl.h).
# ---------------------------------------------------------------------------------------------------------
# nnl_image_aug_param_t: one 64-byte row per sample of the minibatch
IMAGE_AUG_PARAM = np.dtype([('image', '<i8'), ('crop_y', '<i4'), ('crop_x', '<i4'), ('crop_h', '<i4'), ('crop_w', '<i4'),
                            ('m', '<f4', (6,)), ('flags', '<i4'), ('rot', '<i4'), ('bal', '<f4'), ('cont', '<f4')])
IMAGE_AUG_NO_WARP, IMAGE_AUG_FLIP, IMAGE_AUG_NO_LIGHTING = 1, 2, 4


def image_aug(arena, desc, params, sz, stats=None, lighting=False):
    """Transform.__call__ (reference Applications/Vision.py:449-507) for one minibatch, everything after decode, in one launch
    (eval) or two (lighting): arena uint8 [bytes] = every image of the dataset back to back (HWC, RGB); desc int64 [n_images, 3] =
    (byte offset, H, W) per image; params uint8 [bs, 64] = IMAGE_AUG_PARAM rows; sz = (sz_h, sz_w); stats = [mean[3], std[3]] or
    None.  Returns fp32 [bs, sz_h, sz_w, 3] (NHWC: `from_nhwc` gives the logical NCHW view).  Not differentiable: images are data."""
    require_cuda(arena, desc, params)
    if arena.dtype != torch.uint8 or desc.dtype != torch.int64 or params.dtype != torch.uint8:
        raise TypeError('image_aug: arena and params must be uint8 and desc int64')
    if not (arena.is_contiguous() and desc.is_contiguous() and params.is_contiguous()):
        raise ValueError('image_aug: arena, desc and params must be contiguous')
    if desc.dim() != 2 or desc.shape[1] != 3 or params.dim() != 2 or params.shape[1] != IMAGE_AUG_PARAM.itemsize:
        raise ValueError('image_aug: desc must be [n_images, 3] and params [bs, %d]' % IMAGE_AUG_PARAM.itemsize)
    bs, (sz_h, sz_w) = params.shape[0], sz
    out = torch.empty(bs, sz_h, sz_w, 3, dtype=torch.float32, device=arena.device)
    ms = None
    if stats is not None:
        ms = (ctypes.c_float * 6)(*[float(np.float32(v)) for v in list(stats[0]) + list(stats[1])])
    wsb = int(lib.nnl_image_aug_workspace_bytes(bs, sz_h, sz_w)) if lighting else 0
    ws = _workspace(wsb, arena.device)
    check(lib.nnl_image_aug(ptr(arena), arena.numel(), ptr(desc), desc.shape[0], ptr(params), bs, sz_h, sz_w, ms, int(bool(lighting)),
                            ptr(out), ptr(ws), wsb, stream()))
    return out


# ---------------------------------------------------------------------------------------------------------
# K10 detection minibatch: TransformBBox + AspectRatioCollater on the device-resident dataset (include/nnl.h).
# ---------------------------------------------------------------------------------------------------------
# nnl_detect_aug_param_t: one 48-byte row per sample of the minibatch
DETECT_AUG_PARAM = np.dtype([('image', '<i8'), ('box_first', '<i8'), ('box_count', '<i4'), ('rh', '<i4'), ('rw', '<i4'),
                             ('flags', '<i4'), ('bal', '<f4'), ('cont', '<f4'), ('scale', '<f8')])


def detect_aug(arena, desc, image_mean, box_arena, cat_arena, params, Hp, Wp, N, row_jit, col_jit, rand_scale, stats=None):
    """TransformBBox.__call__ and AspectRatioCollater (reference Applications/Vision.py:559-603, 758-812) for one minibatch, everything
    after decode, in one launch: arena uint8 [bytes] and desc int64 [n_images, 3] as for `image_aug`; image_mean fp32 [n_images, 3] =
    channel means of float(v) / 255 per image; box_arena float64 [n_boxes, 4] (xmin, ymin, xmax, ymax) and cat_arena int64 [n_boxes] =
    every image's boxes back to back (n_boxes >= 1); params uint8 [bs, 48] = DETECT_AUG_PARAM rows; row_jit, col_jit, rand_scale: the
    minibatch's values; stats = [mean[3], std[3]] or None.  Returns (fp32 [bs, Hp, Wp, 3] NHWC, fp32 [bs, N, 4], int64 [bs, N]).
    Not differentiable: images and boxes are data."""
    require_cuda(arena, desc, image_mean, box_arena, cat_arena, params)
    if arena.dtype != torch.uint8 or desc.dtype != torch.int64 or params.dtype != torch.uint8:
        raise TypeError('detect_aug: arena and params must be uint8 and desc int64')
    if image_mean.dtype != torch.float32 or box_arena.dtype != torch.float64 or cat_arena.dtype != torch.int64:
        raise TypeError('detect_aug: image_mean must be float32, box_arena float64 and cat_arena int64')
    if not all(t.is_contiguous() for t in (arena, desc, image_mean, box_arena, cat_arena, params)):
        raise ValueError('detect_aug: every input must be contiguous')
    if desc.dim() != 2 or desc.shape[1] != 3 or tuple(image_mean.shape) != (desc.shape[0], 3):
        raise ValueError('detect_aug: desc must be [n_images, 3] and image_mean [n_images, 3]')
    if box_arena.dim() != 2 or box_arena.shape[1] != 4 or box_arena.shape[0] < 1 or tuple(cat_arena.shape) != (box_arena.shape[0],):
        raise ValueError('detect_aug: box_arena must be [n_boxes, 4] with n_boxes >= 1 and cat_arena [n_boxes]')
    if params.dim() != 2 or params.shape[1] != DETECT_AUG_PARAM.itemsize:
        raise ValueError('detect_aug: params must be [bs, %d]' % DETECT_AUG_PARAM.itemsize)
    bs, Hp, Wp, N = params.shape[0], int(Hp), int(Wp), int(N)
    out = torch.empty(bs, Hp, Wp, 3, dtype=torch.float32, device=arena.device)
    boxes = torch.empty(bs, N, 4, dtype=torch.float32, device=arena.device)
    cats = torch.empty(bs, N, dtype=torch.int64, device=arena.device)
    ms = None
    if stats is not None:
        ms = (ctypes.c_float * 6)(*[float(np.float32(v)) for v in list(stats[0]) + list(stats[1])])
    check(lib.nnl_detect_aug(ptr(arena), arena.numel(), ptr(desc), desc.shape[0], ptr(image_mean), ptr(box_arena), ptr(cat_arena),
                             box_arena.shape[0], ptr(params), bs, Hp, Wp, N, int(row_jit), int(col_jit), float(rand_scale), ms,
                             ptr(out), ptr(boxes), ptr(cats), stream()))
    return out, boxes, cats


__all__ += ['detect_aug']


# ---------------------------------------------------------------------------------------------------------
# K16 the resident image set: exact channel sums and a uint8 resample of arenas (include/nnl.h).
# ---------------------------------------------------------------------------------------------------------
IMAGE_STATS_TILE_BYTES = 16384            # NNL_IMAGE_STATS_TILE_BYTES: an image above this many bytes is split over workgroups
_IMAGE_STATS_INVALID = -1                 # NNL_IMAGE_STATS_INVALID seen through int64


def _check_arena(name, arena, desc):
    require_cuda(arena, desc)
    if arena.dtype != torch.uint8 or desc.dtype != torch.int64:
        raise TypeError('%s: an arena must be uint8 and its desc int64' % name)
    if not (arena.is_contiguous() and desc.is_contiguous()) or arena.dim() != 1:
        raise ValueError('%s: an arena must be a contiguous 1-d tensor and its desc contiguous' % name)
    if desc.dim() != 2 or desc.shape[1] != 3:
        raise ValueError('%s: desc must be [n_images, 3]' % name)


def image_stats(arena, desc, first=0, count=None):
    """Exact per-image channel sums of a uint8 arena (nnl_image_stats): arena uint8 [bytes] and desc int64 [n_images, 3] as for
    `image_aug`; rows [first, first + count) of desc (default: all).  Returns a numpy uint64 [count, 6] = (sum v per channel, sum v^2
    per channel) of the raw byte values.  Integer sums: exact and the same bits on every call.  The table is read back to the host
    (it is 48 bytes per image); a desc row that does not lie inside the arena raises ValueError (the kernel reads nothing for it)."""
    _check_arena('image_stats', arena, desc)
    count = desc.shape[0] - int(first) if count is None else int(count)
    out = torch.empty(max(count, 0), 6, dtype=torch.int64, device=arena.device)
    check(lib.nnl_image_stats(ptr(arena), arena.numel(), ptr(desc), desc.shape[0], int(first), count, ptr(out), stream()))
    table = out.cpu().numpy()
    bad = np.nonzero((table == _IMAGE_STATS_INVALID).all(axis=1))[0]
    if len(bad):
        raise ValueError('image_stats: desc row %d does not describe an image inside the arena of %d bytes' % (int(first) + int(bad[0]), arena.numel()))
    return table.view(np.uint64)


def image_resize_u8(src_arena, src_desc, dst_desc, dst_arena=None):
    """Image i of the uint8 arena `src_arena` (src_desc int64 [n, 3] = byte offset, H, W) resampled to the H, W of dst_desc[i] and
    written at dst_desc[i]'s offset of `dst_arena` (nnl_image_resize_u8; include/nnl.h holds the formula: half-pixel bilinear on
    float(v), rintf, clamp; equal sizes copy).  dst_arena=None allocates one that ends with the last image of dst_desc (one small
    read-back).  Returns dst_arena."""
    _check_arena('image_resize_u8', src_arena, src_desc)
    if tuple(dst_desc.shape) != tuple(src_desc.shape):
        raise ValueError('image_resize_u8: dst_desc must have one row per row of src_desc')
    if dst_arena is None:
        d = dst_desc.cpu().numpy()
        dst_arena = torch.empty(int((d[:, 0] + 3 * d[:, 1] * d[:, 2]).max()), dtype=torch.uint8, device=src_arena.device)
    _check_arena('image_resize_u8', dst_arena, dst_desc)
    check(lib.nnl_image_resize_u8(ptr(src_arena), src_arena.numel(), ptr(src_desc), ptr(dst_arena), dst_arena.numel(), ptr(dst_desc),
                                  src_desc.shape[0], stream()))
    return dst_arena


__all__ += ['image_stats', 'image_resize_u8', 'IMAGE_STATS_TILE_BYTES']


# ---------------------------------------------------------------------------------------------------------
# K11 detection test-time augmentation: the undo and concatenation of TTA_bbox (include/nnl.h).
# ---------------------------------------------------------------------------------------------------------
# nnl_tta_undo_t: one 20-byte row per (image, pass)
TTA_UNDO = np.dtype([('col_jit', '<f4'), ('row_jit', '<f4'), ('inv', '<f4'), ('cols', '<f4'), ('flip', '<i4')])


def tta_undo_rows(draws, scales, cols):
    """The TTA_UNDO rows of one pass (reference Applications/Vision.py:2086-2096): draws = the pass's per-image values in dataset order
    (DetectionBatches.last_draws: row_jit, col_jit, rand_scale and flip AS APPLIED), scales [n] the images' own scales and cols [n]
    their original widths.  inv = 1 / (rand_scale scale) in float64, rounded once to fp32 (numpy: a Python float against a float32
    array)."""
    rows = np.zeros(len(draws), dtype=TTA_UNDO)
    for i, d in enumerate(draws):
        rows[i] = (d['col_jit'], d['row_jit'], np.float32(1.0 / (float(d['rand_scale']) * float(scales[i]))), cols[i], int(d['flip'] != 0))
    return rows


def tta_bbox_merge(boxes, classes, scores, counts, undo):
    """The per-pass survivors of TTA_bbox mapped back to the original images and concatenated per image, in one launch: boxes fp32
    [L, P, M, 4], classes int32 [L, P, M], scores fp32 [L, P, M], counts int32 [L, P] (survivors in slots [0, count), descending
    score), undo uint8 [L, P, 20] = TTA_UNDO rows.  Returns (cand_boxes [L, P M, 4], cand_classes, cand_scores, cand_order [L, P M],
    cand_count [L]): what nnl_nms reads with cap = P M.  A count outside [0, M] raises the device's index-error flag
    (`raise_if_index_error`) and that pass contributes nothing."""
    require_cuda(boxes, classes, scores, counts, undo)
    if boxes.dtype != torch.float32 or scores.dtype != torch.float32 or classes.dtype != torch.int32 or counts.dtype != torch.int32 \
            or undo.dtype != torch.uint8:
        raise TypeError('tta_bbox_merge: boxes and scores must be float32, classes and counts int32 and undo uint8')
    if not all(t.is_contiguous() for t in (boxes, classes, scores, counts, undo)):
        raise ValueError('tta_bbox_merge: every input must be contiguous')
    if boxes.dim() != 4 or boxes.shape[3] != 4:
        raise ValueError('tta_bbox_merge: boxes must be [L, P, M, 4]')
    L, P, M = boxes.shape[:3]
    if tuple(classes.shape) != (L, P, M) or tuple(scores.shape) != (L, P, M) or tuple(counts.shape) != (L, P) \
            or tuple(undo.shape) != (L, P, TTA_UNDO.itemsize):
        raise ValueError('tta_bbox_merge: classes and scores must be [L, P, M], counts [L, P] and undo [L, P, %d]' % TTA_UNDO.itemsize)
    dev = boxes.device
    cbox = torch.empty(L, P * M, 4, dtype=torch.float32, device=dev)
    ccls = torch.empty(L, P * M, dtype=torch.int32, device=dev)
    cscore = torch.empty(L, P * M, dtype=torch.float32, device=dev)
    corder = torch.empty(L, P * M, dtype=torch.int32, device=dev)
    ccount = torch.empty(L, dtype=torch.int32, device=dev)
    check(lib.nnl_tta_bbox_merge(ptr(boxes), ptr(classes), ptr(scores), ptr(counts), ptr(undo), L, P, M, ptr(cbox), ptr(ccls), ptr(cscore),
                                 ptr(corder), ptr(ccount), ptr(index_error_flag(dev)), stream()))
    return cbox, ccls, cscore, corder, ccount


__all__ += ['tta_bbox_merge', 'tta_undo_rows']


# ---------------------------------------------------------------------------------------------------------
# K12 time-series features of the structured-data workflow (include/nnl.h): rows sorted by (group, time).
# ---------------------------------------------------------------------------------------------------------
SEG_SCAN_TILE = 1024                     # NNL_SEG_SCAN_TILE: rows per scan tile (tests place group boundaries on its edges)
ROLL_STATS = ['Sum', 'Min', 'Max', 'Mean', 'Std', 'Count']      # bit k of stat_mask, and the order of the output planes


def _seg_rows(name, t, **others):
    "t int64 [n] and every other array uint8 / int32 [n] as named, contiguous, on t's device"
    require_cuda(t, *[a for a, _ in others.values()])
    if t.dtype != torch.int64 or t.dim() != 1 or t.numel() < 1:
        raise ValueError('%s: t must be a non-empty int64 vector' % name)
    for key, (a, dtype) in others.items():
        if a.dtype != dtype or tuple(a.shape) != tuple(t.shape) or a.device != t.device:
            raise ValueError('%s: %s must be %s [%d] on %s' % (name, key, dtype, t.numel(), t.device))
    return [t.contiguous()] + [a.contiguous() for a, _ in others.values()]


def seg_event_gaps(t, head, event, timescale=1.0):
    """Time since the last and until the next event inside each group, for rows sorted by (group, time): t int64 [n], head uint8 [n]
    (1 on the first row of a group), event uint8 [n].  Returns (before, after, seg_start, seg_end): float64 [n] gaps in units of
    `timescale` (NaN where the group has no such event; a row's own event does not count) and int32 [n] first / last row of the
    row's group."""
    t, head, event = _seg_rows('seg_event_gaps', t, head=(head, torch.uint8), event=(event, torch.uint8))
    n, dev = t.numel(), t.device
    before, after = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
    seg_start, seg_end = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    check(lib.nnl_seg_event_gaps(ptr(t), ptr(head), ptr(event), n, float(timescale), ptr(before), ptr(after), ptr(seg_start), ptr(seg_end),
                                 stream()))
    return before, after, seg_start, seg_end


def seg_rolling(t, seg_start, seg_end, x, stats, count_window=0, span=0, forward=False):
    """Rolling statistics inside each group: x float64 [C, n], stats a list out of ROLL_STATS, exactly one of count_window (rows) and
    span (t's units) positive; seg_start / seg_end as seg_event_gaps returns them.  Returns float64 [len(stats), C, n] in the order of
    `stats`.  NaN entries are skipped (Std: ddof 1, NaN below two entries; Count 0 and the others NaN for an empty window)."""
    t, seg_start, seg_end = _seg_rows('seg_rolling', t, seg_start=(seg_start, torch.int32), seg_end=(seg_end, torch.int32))
    require_cuda(x)
    n = t.numel()
    if x.dtype != torch.float64 or x.dim() != 2 or x.shape[1] != n or x.device != t.device:
        raise ValueError('seg_rolling: x must be float64 [C, %d] on %s' % (n, t.device))
    unknown = [s for s in stats if s not in ROLL_STATS]
    if unknown or not stats or len(set(stats)) != len(stats):
        raise ValueError('seg_rolling: stats must be distinct names out of %s (got %r)' % (ROLL_STATS, list(stats)))
    x = x.contiguous()
    mask = sum(1 << ROLL_STATS.index(s) for s in stats)
    planes = [s for s in ROLL_STATS if s in stats]
    out = torch.empty(len(planes), x.shape[0], n, dtype=torch.float64, device=t.device)
    check(lib.nnl_seg_rolling(ptr(t), ptr(seg_start), ptr(seg_end), ptr(x), n, x.shape[0], int(count_window), int(span), int(bool(forward)),
                              mask, ptr(out), stream()))
    return out if planes == list(stats) else out[[planes.index(s) for s in stats]]


__all__ += ['seg_event_gaps', 'seg_rolling', 'SEG_SCAN_TILE', 'ROLL_STATS']


# ---------------------------------------------------------------------------------------------------------
# K13 association measures of the structured-data EDA (include/nnl.h): many column pairs per call.
# codes int32 [V, n] (-1 missing), vals float64 [V, n] (NaN missing) and shift float64 [V] are device tensors; card and the pair
# lists are host integer sequences.
# ---------------------------------------------------------------------------------------------------------
ASSOC_ROW_TILE = 1024                    # NNL_ASSOC_ROW_TILE: rows a workgroup stages at a time
ASSOC_LDS_CELLS = 6144                   # NNL_ASSOC_LDS_CELLS: largest contingency table counted in LDS
ASSOC_MOMENT_LDS_CELLS = 1152            # NNL_ASSOC_MOMENT_LDS_CELLS: most categories whose moments are summed in LDS
ASSOC_MAX_GROUPS = 256                   # NNL_ASSOC_MAX_GROUPS: workgroups per launch
ASSOC_CONTINGENCY_PAIRS = 32             # pairs one contingency launch takes (a longer list is cut into several launches)
ASSOC_CONT_PAIRS = 16                    # pairs one cont x cont launch takes
ASSOC_MAX_TABLE_CELLS = 2 ** 26          # per table
ASSOC_MAX_CALL_CELLS = 2 ** 28           # all tables of one call (1 GiB of uint32): the caller chunks its pair list below this


def _host_i32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int64).astype(np.int32))


def _hp(a):
    return ctypes.c_void_p(a.ctypes.data)


def _assoc_pairs(name, pair_x, pair_y, Vx, Vy):
    px, py = _host_i32(pair_x), _host_i32(pair_y)
    if px.ndim != 1 or px.shape != py.shape or len(px) < 1:
        raise ValueError('%s: pair_x and pair_y must be equally long, non-empty lists' % name)
    if px.min() < 0 or px.max() >= Vx or py.min() < 0 or py.max() >= Vy:
        raise ValueError('%s: a pair names a column outside [0, %d) x [0, %d)' % (name, Vx, Vy))
    return px, py


def _assoc_columns(name, t, dtype, what):
    require_cuda(t)
    if t.dtype != dtype or t.dim() != 2 or t.shape[0] < 1 or not 1 <= t.shape[1] < 2 ** 31:
        raise ValueError('%s: %s must be %s [V, n] with 1 <= n < 2^31' % (name, what, dtype))
    return t.contiguous()


def _assoc_card(name, card, V):
    card = _host_i32(card)
    if card.shape != (V,) or card.min() < 1:
        raise ValueError('%s: card must hold %d cardinalities of at least 1' % (name, V))
    return card


def assoc_table_offsets(card, pair_x, pair_y):
    "int64 [P+1]: where the row-major [card[x], card[y]] table of each pair starts in the tables vector"
    card = np.asarray(card, dtype=np.int64)
    cells = card[np.asarray(pair_x, dtype=np.int64)] * card[np.asarray(pair_y, dtype=np.int64)]
    return np.concatenate([[0], np.cumsum(cells)]).astype(np.int64)


def assoc_contingency(codes, card, pair_x, pair_y):
    """Contingency tables of many column pairs: codes int32 [V, n] on the device, card [V], pair_x / pair_y [P] host integers.
    Returns (tables, offsets): tables int32 [offsets[P]] on the device (exact counts of the rows where both codes are present; the
    table of pair p is tables[offsets[p]:offsets[p+1]].view(card[x], card[y])) and offsets as assoc_table_offsets gives them."""
    codes = _assoc_columns('assoc_contingency', codes, torch.int32, 'codes')
    V, n = codes.shape
    card = _assoc_card('assoc_contingency', card, V)
    px, py = _assoc_pairs('assoc_contingency', pair_x, pair_y, V, V)
    offsets = assoc_table_offsets(card, px, py)
    cells = np.diff(offsets)
    if cells.max() > ASSOC_MAX_TABLE_CELLS:
        raise ValueError('assoc_contingency: a table of %d cells exceeds the limit of %d' % (cells.max(), ASSOC_MAX_TABLE_CELLS))
    if offsets[-1] > ASSOC_MAX_CALL_CELLS:
        raise ValueError('assoc_contingency: %d cells in one call exceed the limit of %d: pass fewer pairs per call'
                         % (offsets[-1], ASSOC_MAX_CALL_CELLS))
    tables = torch.empty(int(offsets[-1]), dtype=torch.int32, device=codes.device)
    check(lib.nnl_assoc_contingency(ptr(codes), _hp(card), V, n, _hp(px), _hp(py), _hp(offsets), len(px), ptr(tables), stream()))
    return tables, offsets


def assoc_table_stats(tables, card, pair_x, pair_y, offsets):
    """float64 [P, 6] on the device from assoc_contingency's tables: n, non-empty rows, non-empty columns, H_X, H_Y and H_XY (with
    the reference's 1e-20 clamp term for every empty cell of the observed table).  Bit-equal from call to call."""
    require_cuda(tables)
    if tables.dtype != torch.int32 or tables.dim() != 1:
        raise ValueError('assoc_table_stats: tables must be the int32 vector assoc_contingency returns')
    card = _assoc_card('assoc_table_stats', card, len(card))
    px, py = _assoc_pairs('assoc_table_stats', pair_x, pair_y, len(card), len(card))
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    if not np.array_equal(offsets, assoc_table_offsets(card, px, py)) or offsets[-1] != tables.numel():
        raise ValueError('assoc_table_stats: offsets do not match the cardinalities of the pairs and the length of tables')
    out = torch.empty(len(px), 6, dtype=torch.float64, device=tables.device)
    check(lib.nnl_assoc_table_stats(ptr(tables.contiguous()), _hp(card), len(card), _hp(px), _hp(py), _hp(offsets), len(px), ptr(out),
                                    stream()))
    return out


def _assoc_vals(name, vals, shift):
    vals = _assoc_columns(name, vals, torch.float64, 'vals')
    require_cuda(shift)
    if shift.dtype != torch.float64 or tuple(shift.shape) != (vals.shape[0],) or shift.device != vals.device:
        raise ValueError('%s: shift must be float64 [%d] on %s' % (name, vals.shape[0], vals.device))
    return vals, shift.contiguous()


def assoc_cat_cont(codes, card, vals, shift, pair_x, pair_y):
    """Moments of a continuous column per category, many pairs at once: pair p = (codes[pair_x[p]], vals[pair_y[p]]).  Returns float64
    [P, 6] on the device: n, non-empty categories, correlation ratio, raw max correlation ratio, min and max of vals - shift, over
    the rows where the code is present and the value is not NaN.  The per-category sums are fp64 atomics: the last bits of the two
    ratios may differ between calls (n, the category count, min and max do not)."""
    codes = _assoc_columns('assoc_cat_cont', codes, torch.int32, 'codes')
    vals, shift = _assoc_vals('assoc_cat_cont', vals, shift)
    if vals.shape[1] != codes.shape[1] or vals.device != codes.device:
        raise ValueError('assoc_cat_cont: codes and vals must hold the same rows on one device')
    card = _assoc_card('assoc_cat_cont', card, codes.shape[0])
    if card.max() > ASSOC_MAX_TABLE_CELLS:
        raise ValueError('assoc_cat_cont: %d categories exceed the limit of %d' % (card.max(), ASSOC_MAX_TABLE_CELLS))
    px, py = _assoc_pairs('assoc_cat_cont', pair_x, pair_y, codes.shape[0], vals.shape[0])
    nbytes = int(lib.nnl_assoc_cat_cont_workspace_bytes(_hp(card), len(card), _hp(px), len(px)))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=codes.device)
    out = torch.empty(len(px), 6, dtype=torch.float64, device=codes.device)
    check(lib.nnl_assoc_cat_cont(ptr(codes), _hp(card), codes.shape[0], ptr(vals), ptr(shift), vals.shape[0], codes.shape[1], _hp(px),
                                 _hp(py), len(px), ptr(ws), nbytes, ptr(out), stream()))
    return out


def assoc_cont_cont(vals, shift, pair_x, pair_y, with_abs=True):
    """Correlations of many pairs of continuous columns.  Returns float64 [P, 4] on the device: n, degenerate (1.0: no common row, or a
    column with one distinct value on the pair's rows), |corr(x, y)| and, with_abs, the absolute maximum correlation (a second pass
    about the pair's means), else NaN.  No atomics: bit-equal from call to call."""
    vals, shift = _assoc_vals('assoc_cont_cont', vals, shift)
    V, n = vals.shape
    px, py = _assoc_pairs('assoc_cont_cont', pair_x, pair_y, V, V)
    nbytes = int(lib.nnl_assoc_cont_cont_workspace_bytes(n, len(px)))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=vals.device)
    out = torch.empty(len(px), 4, dtype=torch.float64, device=vals.device)
    check(lib.nnl_assoc_cont_cont(ptr(vals), ptr(shift), V, n, _hp(px), _hp(py), len(px), int(bool(with_abs)), ptr(ws), nbytes, ptr(out),
                                  stream()))
    return out


__all__ += ['assoc_contingency', 'assoc_table_stats', 'assoc_table_offsets', 'assoc_cat_cont', 'assoc_cont_cont', 'ASSOC_ROW_TILE',
            'ASSOC_LDS_CELLS', 'ASSOC_MOMENT_LDS_CELLS', 'ASSOC_MAX_GROUPS', 'ASSOC_CONTINGENCY_PAIRS', 'ASSOC_CONT_PAIRS',
            'ASSOC_MAX_TABLE_CELLS', 'ASSOC_MAX_CALL_CELLS']


# ---------------------------------------------------------------------------------------------------------
# K14 detection evaluation (include/nnl.h): the COCO / Pascal protocol of COCOeval for boxes and the mAP of Vision.py:1696-1800.
# det_eval_pack is pure numpy and needs no device; det_eval_coco / det_map upload its arrays in ONE buffer, launch, and copy ONE
# buffer back, with no synchronisation in between.
# ---------------------------------------------------------------------------------------------------------
DET_EVAL_MAX_T, DET_EVAL_MAX_A, DET_EVAL_MAX_M, DET_EVAL_MAX_R = 16, 8, 8, 128      # NNL_DET_EVAL_MAX_*
DET_EVAL_LDS_DOUBLES = 2048              # NNL_DET_EVAL_LDS_DOUBLES: a larger group's overlap matrix goes to the scratch buffer


def _pred_arrays(pred, i):
    "one image's [boxes, classes, scores] of predict('val') as (boxes [n, 4] in their own dtype, classes int64 [n], scores [n])"
    boxes, classes, scores = pred
    n = len(boxes)
    if len(classes) != n or len(scores) != n:
        raise ValueError('predictions[%d]: %d boxes, %d classes, %d scores' % (i, n, len(classes), len(scores)))
    if n == 0:
        return np.zeros((0, 4), np.float32), np.zeros(0, np.int64), np.zeros(0, np.float64)
    B = np.stack([np.asarray(b.detach().cpu() if torch.is_tensor(b) else b) for b in boxes]) if not isinstance(boxes, np.ndarray) else boxes
    if B.ndim != 2 or B.shape[1] != 4:
        raise ValueError('predictions[%d]: boxes must be [n, 4] (got %r)' % (i, B.shape))
    if isinstance(classes, np.ndarray) and isinstance(scores, np.ndarray):
        return B, classes.astype(np.int64), scores.astype(np.float64)
    return B, np.array([int(c) for c in classes], dtype=np.int64), np.array([float(s) for s in scores], dtype=np.float64)


def _csr(sorted_keys, groups):
    "offsets int32 [len(groups) + 1] of each group's span in a sorted key vector"
    return np.concatenate([np.searchsorted(sorted_keys, groups, side='left'), [len(sorted_keys)]]).astype(np.int32)


def _check_csr(name, off, n_groups, length):
    off = np.asarray(off)
    if off.shape != (n_groups + 1,) or off[0] != 0 or off[-1] != length or (np.diff(off.astype(np.int64)) < 0).any():
        raise ValueError('det_eval: offsets %s must be non-decreasing, start at 0 and end at %d' % (name, length))


def det_eval_pack(predictions, targets=None, coco=None, image_ids=None, cat2dscat=None, max_det=100, n_categories=None):
    """Flat arrays and offsets of nnl_det_* from `predictions` (the predict('val') format: [boxes, classes, scores] per image, min-max
    boxes) and the ground truth.  Pure numpy.  Two layouts:
    coco=<annotation dict>, image_ids=[id of image i], cat2dscat={model category: dataset category id}: the COCOeval layout.  A
      detection is [float(b0), float(b1), float(b2 - b0), float(b3 - b1)] with the subtraction in the dtype the box arrives in
      (Vision.py:2166), float(score), cat2dscat[category]; groups are sorted by (sorted category id, ascending image id), a group's
      detections by descending score (stable) and cut to `max_det`, its ground truths in annotation order with the annotation's
      area, iscrowd and ignore ('ignore' key, else iscrowd, else 0: cocoeval.py:114-116).  Images are np.unique(image_ids), categories
      the sorted ids of coco['categories']; annotations of other images and detections of other categories do not take part.
    targets=<val_ds.y: [(box, category), ...] per image>, n_categories=C: the mAP layout (Vision.py:1749-1769): float32 min-max
      boxes, groups sorted by (category, image), predictions and targets of a group in their own order.
    Raises ValueError for a prediction category outside the map / [0, C), an annotation id of 0 (coco) and a ground-truth box of
    non-positive area (targets)."""
    if (coco is None) == (targets is None):
        raise ValueError('det_eval_pack: give either coco= (with image_ids and cat2dscat) or targets= (with n_categories)')
    N = len(predictions)
    per = [_pred_arrays(p, i) for i, p in enumerate(predictions)]
    counts = np.array([len(b) for b, _, _ in per], dtype=np.int64)
    img_of = np.repeat(np.arange(N, dtype=np.int64), counts)
    cls = np.concatenate([c for _, c, _ in per]) if N else np.zeros(0, np.int64)
    score = np.concatenate([s for _, _, s in per]) if N else np.zeros(0, np.float64)
    if coco is not None:
        if image_ids is None or cat2dscat is None or len(image_ids) != N:
            raise ValueError('det_eval_pack: the coco layout needs image_ids (one per prediction list) and cat2dscat')
        cat_ids = np.unique(np.array([c['id'] for c in coco['categories']], dtype=np.int64))
        img_ids = np.unique(np.asarray(image_ids, dtype=np.int64))
        K, I = len(cat_ids), len(img_ids)
        unknown = sorted(set(cls.tolist()) - set(cat2dscat))
        if unknown:
            raise ValueError('det_eval_pack: prediction categories %r are absent from the category map' % (unknown,))
        lut = {c: int(cat2dscat[c]) for c in set(cls.tolist())}
        dscat = np.array([lut[c] for c in cls.tolist()], dtype=np.int64)
        xywh = [np.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], axis=1).astype(np.float64) for b, _, _ in per]
        box = np.concatenate(xywh) if N else np.zeros((0, 4))
        k_of = np.searchsorted(cat_ids, dscat)
        known = cat_ids[np.minimum(k_of, K - 1)] == dscat if K else np.zeros(len(dscat), bool)
        i_of = np.searchsorted(img_ids, np.asarray(image_ids, dtype=np.int64))[img_of]
        key = (k_of * I + i_of)[known]
        box, score = box[known], score[known]
        srt = np.lexsort((-score, key))                                     # stable: by group, then descending score
        key, box, score = key[srt], box[srt], score[srt]
        anns = coco['annotations']
        if any(a['id'] == 0 for a in anns):
            raise ValueError("det_eval_pack: an annotation has id 0, which COCOeval cannot tell from 'unmatched' (cocoeval.py:303, 307)")
        a_img = np.array([a['image_id'] for a in anns], dtype=np.int64)
        a_cat = np.array([a['category_id'] for a in anns], dtype=np.int64)
        gi, gk = np.searchsorted(img_ids, a_img), np.searchsorted(cat_ids, a_cat)
        use = np.zeros(len(anns), bool)
        if len(anns) and K and I:
            use = (img_ids[np.minimum(gi, I - 1)] == a_img) & (cat_ids[np.minimum(gk, K - 1)] == a_cat)
        sel = np.nonzero(use)[0]
        gkey = (gk * I + gi)[sel]
        gs = np.argsort(gkey, kind='stable')
        sel, gkey = sel[gs], gkey[gs]
        gt_box = np.array([[float(v) for v in anns[j]['bbox']] for j in sel], dtype=np.float64).reshape(-1, 4)
        gt_area = np.array([float(anns[j]['area']) for j in sel], dtype=np.float64)
        crowd = np.array([1 if anns[j].get('iscrowd', 0) else 0 for j in sel], dtype=np.uint8)
        ignore = np.array([1 if (anns[j]['ignore'] if 'ignore' in anns[j] else anns[j].get('iscrowd', 0)) else 0 for j in sel], dtype=np.uint8)
        groups = np.unique(np.concatenate([key, gkey]))
        dt_off = _csr(key, groups)
        rank = np.arange(len(key), dtype=np.int64) - np.repeat(dt_off[:-1].astype(np.int64), np.diff(dt_off))
        keep = rank < int(max_det)                                          # dt[0:maxDets[-1]] (cocoeval.py:183-184)
        key, box, score, rank = key[keep], box[keep], score[keep], rank[keep]
        dt_off = _csr(key, groups)
        grp_cat = groups // max(I, 1)
        cat_grp_off = np.searchsorted(grp_cat, np.arange(K + 1), side='left').astype(np.int32)
        return {'kind': 'coco', 'K': K, 'I': I, 'max_det': int(max_det), 'cat_ids': cat_ids, 'img_ids': img_ids,
                'grp_cat': grp_cat.astype(np.int32), 'grp_img': (groups % max(I, 1)).astype(np.int32),
                'dt_off': dt_off, 'gt_off': _csr(gkey, groups), 'cat_grp_off': cat_grp_off, 'cat_dt_off': dt_off[cat_grp_off],
                'dt_box': np.ascontiguousarray(box), 'dt_score': score, 'dt_rank': rank.astype(np.int32),
                'order': np.lexsort((-score, key // max(I, 1))).astype(np.int32),      # per category: stable descending score
                'gt_box': gt_box, 'gt_area': gt_area, 'gt_flags': (crowd | (ignore << 1)).astype(np.uint8), 'gt_ann': sel.astype(np.int64)}
    C = int(n_categories) if n_categories is not None else 0
    if C < 1 or len(targets) != N:
        raise ValueError('det_eval_pack: the mAP layout needs n_categories >= 1 and one target list per prediction list')
    if len(cls) and (cls.min() < 0 or cls.max() >= C):
        raise ValueError('det_eval_pack: prediction categories must lie in [0, %d) (got %d .. %d)' % (C, cls.min(), cls.max()))
    box = np.concatenate([b.astype(np.float32) for b, _, _ in per]) if N else np.zeros((0, 4), np.float32)
    key = cls * N + img_of
    srt = np.argsort(key, kind='stable')
    key, box, score = key[srt], box[srt], score[srt]
    t_box = np.array([np.asarray(b, dtype=np.float32) for y in targets for b, _ in y], dtype=np.float32).reshape(-1, 4)
    t_cls = np.array([int(c) for y in targets for _, c in y], dtype=np.int64)
    t_img = np.repeat(np.arange(N, dtype=np.int64), [len(y) for y in targets])
    if len(t_cls) and (t_cls.min() < 0 or t_cls.max() >= C):
        raise ValueError('det_eval_pack: target categories must lie in [0, %d)' % C)
    bad = ~((t_box[:, 2] - t_box[:, 0] > 0) & (t_box[:, 3] - t_box[:, 1] > 0))
    if bad.any():
        raise ValueError('det_eval_pack: ground-truth box %r of image %d has no positive area: its overlap with a degenerate prediction '
                         'is 0 / 0' % (t_box[bad][0].tolist(), int(t_img[bad][0])))
    gkey = t_cls * N + t_img
    gs = np.argsort(gkey, kind='stable')
    gkey, t_box = gkey[gs], t_box[gs]
    groups = np.unique(np.concatenate([key, gkey]))
    pr_off = _csr(key, groups)
    cat_grp_off = np.searchsorted(groups // max(N, 1), np.arange(C + 1), side='left').astype(np.int32)
    return {'kind': 'map', 'C': C, 'N': N, 'grp_cat': (groups // max(N, 1)).astype(np.int32), 'grp_img': (groups % max(N, 1)).astype(np.int32),
            'pr_off': pr_off, 'gt_off': _csr(gkey, groups), 'cat_grp_off': cat_grp_off, 'cat_pr_off': pr_off[cat_grp_off],
            'pr_box': np.ascontiguousarray(box), 'pr_score': score, 'order': np.lexsort((-score, key // max(N, 1))).astype(np.int32),
            'gt_box': np.ascontiguousarray(t_box), 'ntrue': np.bincount(t_cls, minlength=C).astype(np.int64)}


_NP2T = {np.dtype(np.float64): torch.float64, np.dtype(np.float32): torch.float32, np.dtype(np.int32): torch.int32,
         np.dtype(np.int64): torch.int64, np.dtype(np.uint8): torch.uint8}


def _det_upload(arrays, device):
    "the named host arrays as views of ONE device buffer (one host-to-device copy)"
    device = torch.device(device)
    if device.type != 'cuda':
        raise _lib.NnlError('nnl HIP op called for a non-CUDA device: the MI355X path has no CPU fallback')
    spans, total = {}, 0
    for name, a in arrays.items():
        spans[name] = total
        total += (a.nbytes + 15) // 16 * 16
    host = np.zeros(max(total, 16), dtype=np.uint8)
    for name, a in arrays.items():
        host[spans[name]:spans[name] + a.nbytes] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    buf = torch.from_numpy(host).to(device)
    out = {name: buf[spans[name]:spans[name] + a.nbytes].view(_NP2T[a.dtype]).view(a.shape) for name, a in arrays.items()}
    out['_buffer'] = buf
    return out


def _det_params(iouThrs, areaRng=None):
    thr = np.ascontiguousarray(np.asarray(iouThrs, dtype=np.float64).reshape(-1))
    if not 1 <= len(thr) <= DET_EVAL_MAX_T or not np.isfinite(thr).all():
        raise ValueError('det_eval: between 1 and %d finite thresholds (got %r)' % (DET_EVAL_MAX_T, thr.tolist()))
    if areaRng is None:
        return thr
    rng = np.ascontiguousarray(np.asarray(areaRng, dtype=np.float64))
    if rng.ndim != 2 or rng.shape[1] != 2 or not 1 <= len(rng) <= DET_EVAL_MAX_A or not np.isfinite(rng).all():
        raise ValueError('det_eval: areaRng must be [A, 2] finite numbers, 1 <= A <= %d' % DET_EVAL_MAX_A)
    return thr, rng


def _coco_checked(packed):
    if not isinstance(packed, dict) or packed.get('kind') != 'coco':
        raise ValueError("det_eval_coco: `packed` must come from det_eval_pack(..., coco=...)")
    p = packed
    NG, Nd, Ng, K = len(p['grp_cat']), len(p['dt_score']), len(p['gt_area']), int(p['K'])
    if NG < 1 or K < 1:
        raise ValueError('det_eval_coco: nothing to evaluate (no detection and no ground truth in the evaluated images and categories)')
    _check_csr('dt_off', p['dt_off'], NG, Nd)
    _check_csr('gt_off', p['gt_off'], NG, Ng)
    _check_csr('cat_grp_off', p['cat_grp_off'], K, NG)
    _check_csr('cat_dt_off', p['cat_dt_off'], K, Nd)
    if not np.array_equal(p['cat_dt_off'], np.asarray(p['dt_off'])[p['cat_grp_off']]):
        raise ValueError('det_eval_coco: cat_dt_off does not match dt_off at cat_grp_off')
    order = np.asarray(p['order'])
    if order.shape != (Nd,) or p['dt_rank'].shape != (Nd,) or p['dt_box'].shape != (Nd, 4) or p['gt_box'].shape != (Ng, 4) \
            or p['gt_flags'].shape != (Ng,):
        raise ValueError('det_eval_coco: array lengths do not match the offsets')
    if Nd:
        seg = np.repeat(np.arange(K), np.diff(p['cat_dt_off']))
        lo, hi = np.asarray(p['cat_dt_off'])[seg], np.asarray(p['cat_dt_off'])[seg + 1]
        if (order < lo).any() or (order >= hi).any():
            raise ValueError('det_eval_coco: order leaves its category')
    return NG, Nd, Ng, K


def _coco_scratch(packed, A, T):
    "scr_off int64 [NG] (-1: the group's buffer fits LDS) and the scratch size in doubles"
    D, G = np.diff(packed['dt_off']).astype(np.int64), np.diff(packed['gt_off']).astype(np.int64)
    need = D * G + ((A * T + A) * G + 7) // 8
    big = (need > DET_EVAL_LDS_DOUBLES) & (D > 0) & (G > 0)
    off = np.full(len(D), -1, dtype=np.int64)
    off[big] = np.cumsum(need[big]) - need[big]
    return off, int(need[big].sum())


def _coco_launch(packed, iouThrs, areaRng, device, recThrs=None, maxDets=None):
    "upload, nnl_det_coco_match and, with recThrs, nnl_det_coco_accumulate; everything stays on the device"
    NG, Nd, Ng, K = _coco_checked(packed)
    thr, rng = _det_params(iouThrs, areaRng)
    T, A = len(thr), len(rng)
    if recThrs is not None:
        rec = np.ascontiguousarray(np.asarray(recThrs, dtype=np.float64).reshape(-1))
        md = np.ascontiguousarray(np.asarray(maxDets, dtype=np.int64).reshape(-1).astype(np.int32))
        if not 1 <= len(rec) <= DET_EVAL_MAX_R or not np.isfinite(rec).all() or (np.diff(rec) < 0).any():
            raise ValueError('det_eval_coco: recThrs must be 1 to %d ascending finite numbers' % DET_EVAL_MAX_R)
        if not 1 <= len(md) <= DET_EVAL_MAX_M or md.min() < 1 or (np.diff(md) < 0).any() or md[-1] != packed['max_det']:
            raise ValueError('det_eval_coco: maxDets must be 1 to %d ascending positive numbers ending at the %d the detections were cut to'
                             % (DET_EVAL_MAX_M, packed['max_det']))
    scr_off, scr_doubles = _coco_scratch(packed, A, T)
    names = ['dt_off', 'gt_off', 'cat_grp_off', 'cat_dt_off', 'order', 'dt_rank', 'dt_score', 'dt_box', 'gt_box', 'gt_area', 'gt_flags']
    dev = _det_upload(dict({n: np.ascontiguousarray(packed[n]) for n in names}, scr_off=scr_off), device)
    device = dev['_buffer'].device
    scratch = torch.empty(max(scr_doubles, 1), dtype=torch.float64, device=device)
    dtm = torch.empty(A, T, Nd, dtype=torch.int32, device=device)
    dtig = torch.empty(A, T, Nd, dtype=torch.uint8, device=device)
    npig = torch.empty(A, NG, dtype=torch.int32, device=device)
    res = {'dtm': dtm, 'dtig': dtig, 'npig': npig, '_keep': (dev, scratch)}
    if recThrs is None:
        status = torch.empty(2, dtype=torch.int32, device=device)
    else:
        R, M = len(rec), len(md)
        n_pr, n_rc = T * R * K * A * M, T * K * A * M
        out = torch.empty(2 * n_pr + n_rc + 1, dtype=torch.float64, device=device)         # one buffer: one copy back
        status = out[-1:].view(torch.int32)
        res.update(out=out, shape_pr=(T, R, K, A, M), shape_rc=(T, K, A, M))
    res['status'] = status
    check(lib.nnl_det_coco_match(ptr(dev['dt_off']), ptr(dev['gt_off']), ptr(dev['dt_box']), ptr(dev['gt_box']), ptr(dev['gt_area']),
                                 ptr(dev['gt_flags']), ptr(dev['scr_off']), NG, Nd, Ng, _hp(thr), T, _hp(rng), A, ptr(scratch),
                                 scr_doubles * 8, ptr(dtm), ptr(dtig), ptr(npig), ptr(status), stream()))
    if recThrs is not None:
        o = res['out']
        check(lib.nnl_det_coco_accumulate(ptr(dev['cat_grp_off']), ptr(dev['cat_dt_off']), ptr(dev['order']), ptr(dev['dt_rank']),
                                          ptr(dev['dt_score']), ptr(dtm), ptr(dtig), ptr(npig), K, NG, Nd, T, A, _hp(md), M, _hp(rec), R,
                                          ptr(o[:n_pr]), ptr(o[n_pr:2 * n_pr]), ptr(o[2 * n_pr:2 * n_pr + n_rc]), stream()))
    return res


def _coco_status(flag):
    if int(flag) != 0:
        raise _lib.NnlError('nnl_det_coco_match skipped a group whose overlap matrix did not fit the buffer it was given (status %d)' % int(flag))


def det_eval_coco_match(packed, iouThrs, areaRng, device='cuda'):
    """evaluateImg of every group (cocoeval.py:243-321) for all area ranges and thresholds: host arrays (dtm int32 [A, T, Nd], the
    matched ground truth's position in its group + 1 or 0; dtig uint8 [A, T, Nd]; npig int32 [A, NG], the group's ground truths not
    ignored in the range).  Nd and NG count det_eval_pack's detections and groups."""
    res = _coco_launch(packed, iouThrs, areaRng, device)
    status = res['status'].cpu()
    _coco_status(status[0])
    return res['dtm'].cpu().numpy(), res['dtig'].cpu().numpy(), res['npig'].cpu().numpy()


def det_eval_coco(packed, iouThrs, recThrs, maxDets, areaRng, device='cuda'):
    """COCOeval.evaluate + accumulate for boxes with useCats=1 (cocoeval.py:129-428) on det_eval_pack(..., coco=...)'s arrays: returns
    host arrays (precision [T, R, K, A, M], recall [T, K, A, M], scores [T, R, K, A, M]) as COCOeval.eval holds them.  One upload, two
    launches, one copy back.  maxDets must ascend and end at the max_det the detections were cut to; recThrs must ascend."""
    res = _coco_launch(packed, iouThrs, areaRng, device, recThrs, maxDets)
    host = res['out'].cpu().numpy()
    _coco_status(host[-1:].view(np.int32)[0])
    n_pr, n_rc = int(np.prod(res['shape_pr'])), int(np.prod(res['shape_rc']))
    return (host[:n_pr].reshape(res['shape_pr']), host[2 * n_pr:2 * n_pr + n_rc].reshape(res['shape_rc']),
            host[n_pr:2 * n_pr].reshape(res['shape_pr']))


def _map_launch(packed, thresholds, device, integrate):
    if not isinstance(packed, dict) or packed.get('kind') != 'map':
        raise ValueError("det_map: `packed` must come from det_eval_pack(..., targets=...)")
    p = packed
    NG, Np, Ng, C = len(p['grp_cat']), len(p['pr_score']), len(p['gt_box']), int(p['C'])
    _det_params(thresholds)
    # `jaccard > thresh` of Vision.py:1727 compares a float32 with the threshold under numpy's promotion rules (a Python float is
    # taken to float32 by numpy >= 2): the kernel compares in fp64 against the threshold as that comparison sees it
    thr = np.array([float((np.float32(0) + t).dtype.type(t)) for t in (thresholds if np.ndim(thresholds) else [thresholds])], dtype=np.float64)
    T = len(thr)
    if NG < 1:
        if torch.device(device).type != 'cuda':
            raise _lib.NnlError('nnl HIP op called for a non-CUDA device: the MI355X path has no CPU fallback')
        return {'empty': True, 'T': T, 'C': C, 'ntrue': p['ntrue']}
    _check_csr('pr_off', p['pr_off'], NG, Np)
    _check_csr('gt_off', p['gt_off'], NG, Ng)
    _check_csr('cat_grp_off', p['cat_grp_off'], C, NG)
    _check_csr('cat_pr_off', p['cat_pr_off'], C, Np)
    order = np.asarray(p['order'])
    if order.shape != (Np,) or p['pr_box'].shape != (Np, 4) or p['gt_box'].shape != (Ng, 4) or p['ntrue'].shape != (C,):
        raise ValueError('det_map: array lengths do not match the offsets')
    if Np:
        seg = np.repeat(np.arange(C), np.diff(p['cat_pr_off']))
        if (order < np.asarray(p['cat_pr_off'])[seg]).any() or (order >= np.asarray(p['cat_pr_off'])[seg + 1]).any():
            raise ValueError('det_map: order leaves its category')
    names = ['pr_off', 'gt_off', 'cat_pr_off', 'order', 'pr_score', 'pr_box', 'gt_box', 'ntrue']
    dev = _det_upload({n: np.ascontiguousarray(p[n]) for n in names}, device)
    device = dev['_buffer'].device
    correct = torch.empty(T, Np, dtype=torch.uint8, device=device)
    check(lib.nnl_det_map_match(ptr(dev['pr_off']), ptr(dev['gt_off']), ptr(dev['pr_box']), ptr(dev['gt_box']), NG, Np, Ng, _hp(thr), T,
                                ptr(correct), stream()))
    res = {'correct': correct, '_keep': dev}
    if integrate:
        nbytes = int(lib.nnl_det_map_integrate_workspace_bytes(Np, T))
        ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=device)
        out = torch.empty(T, C, dtype=torch.float64, device=device)
        check(lib.nnl_det_map_integrate(ptr(dev['cat_pr_off']), ptr(dev['order']), ptr(dev['pr_score']), ptr(correct), ptr(dev['ntrue']), C,
                                        Np, T, ptr(ws), nbytes, ptr(out), stream()))
        res.update(out=out, _ws=ws)
    return res


def det_map_match(packed, thresholds, device='cuda'):
    "the is_correct flags of mAP1 (Vision.py:1696-1728) for every threshold: host uint8 [T, Np] over det_eval_pack's prediction order"
    res = _map_launch(packed, thresholds, device, False)
    if res.get('empty'):
        return np.zeros((res['T'], 0), dtype=np.uint8)
    return res['correct'].cpu().numpy()


def det_map(packed, thresholds, device='cuda'):
    """mAP1 of every (threshold, category) (Vision.py:1696-1747) on det_eval_pack(..., targets=...)'s arrays: host float64 [T, C], 0.0
    for a category without predictions and nan for one without ground truth, as the host code gives.  One upload, two launches, one
    copy back; the same inputs give the same bits."""
    res = _map_launch(packed, thresholds, device, True)
    if res.get('empty'):                                  # no prediction and no ground truth at all: 0.0 / 0
        return np.full((res['T'], res['C']), np.nan)
    return res['out'].cpu().numpy()


__all__ += ['det_eval_pack', 'det_eval_coco', 'det_eval_coco_match', 'det_map', 'det_map_match', 'DET_EVAL_LDS_DOUBLES', 'DET_EVAL_MAX_T',
            'DET_EVAL_MAX_A', 'DET_EVAL_MAX_M', 'DET_EVAL_MAX_R']

from .ops_text import (lstm_layer, embedding_rowmask, softmax_cross_entropy, cross_entropy_nd, seq_activation_reg)  # noqa: E402,F401
__all__ += ['lstm_layer', 'embedding_rowmask', 'softmax_cross_entropy', 'cross_entropy_nd', 'seq_activation_reg', 'conv_add_upsampled']
