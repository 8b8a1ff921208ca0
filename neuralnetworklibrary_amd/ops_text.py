"""Language-model ops on the C ABI (K5 / K5b): LSTM layer, embedding with vocabulary-row dropout, fused softmax-CE.
Imported into `ops` (use `ops.lstm_layer`, `ops.embedding_rowmask`, `ops.softmax_cross_entropy`).  Text generation (K5d):
`LstmCellB1` / `lstm_cell_b1` and `LmNextToken` / `lm_next_token`, the batch-1 decode kernels of csrc/lm_generate.hip.  Tokeniser and
vocabulary (K17): `TextCorpus`, `token_bounds`, `vocab_build_exact`, `text_numericalize`, the kernels of csrc/text_tokens.hip."""
import torch
import torch.nn.functional as F

from . import _lib
from ._lib import check, lib, ptr, require_cuda, stream


def _f32c(t):
    return t.contiguous() if t.dtype == torch.float32 else t.float().contiguous()


def _ceil4(n):
    return (n + 3) // 4 * 4


class _LSTMRecurrence(torch.autograd.Function):
    """The time recurrence of nn.LSTM(num_layers=1) (reference Applications/Text.py:483,513) given the input
    projections gx [T,B,4H]: forward = nnl_lstm_fwd, backward = nnl_lstm_bwd (BPTT) + one GEMM for dW_hh."""

    @staticmethod
    def forward(ctx, gx, w_raw, h0, c0, wmask=None, p=0.0, seed=0):
        """w_raw [4H,H]: the RAW recurrent matrix; the weight drop W = w_raw * m (Text.py:495-513) — m = `wmask` (explicit, already
        scaled) or Bernoulli(1-p)/(1-p) from (seed, element index) — and the zero padding to the kernels' k granularity are ONE
        pass (nnl_weight_drop); the backward re-derives m for dW_raw = dW * m."""
        require_cuda(gx, w_raw, h0, c0, wmask)
        gx, w_raw = _f32c(gx), _f32c(w_raw)
        T, B, G = gx.shape
        H = G // 4
        h0, c0 = _f32c(h0).view(B, H), _f32c(c0).view(B, H)
        Hp = int(lib.nnl_lstm_padded_hidden(H))
        dev = gx.device
        wm = None if wmask is None else _f32c(wmask)
        ctx.drop = (wm is not None or p > 0.0, float(p), int(seed))
        if Hp == H and not ctx.drop[0]:
            w_pad = w_raw
        else:
            w_pad = torch.empty(G, Hp, dtype=torch.float32, device=dev)
            check(lib.nnl_weight_drop(ptr(w_raw), H, ptr(wm), ptr(w_pad), Hp, G, H, int(seed), float(p), stream()))
        w_hh = w_pad                                        # [4H, Hp]: columns >= H are zero
        y = torch.empty(T, B, H, dtype=torch.float32, device=dev)
        cy = torch.empty(T, B, H, dtype=torch.float32, device=dev)
        from .ops import _workspace, lstm_timeout_flag
        gates = torch.empty(T, B, G, dtype=torch.float32, device=dev)
        wsb = int(lib.nnl_lstm_workspace_bytes(T, B, H))
        ws = _workspace(wsb, dev)
        check(lib.nnl_lstm_fwd(ptr(gx), ptr(w_pad), ptr(h0), ptr(c0), ptr(y), ptr(cy), ptr(gates), T, B, H, ptr(ws), wsb,
                               ptr(lstm_timeout_flag(dev)), stream()))
        ctx.save_for_backward(w_hh, h0, c0, y, cy, gates, wm)
        return y, y[-1].clone(), cy[-1].clone()

    @staticmethod
    def backward(ctx, dy, dhT, dcT):
        w_hh, h0, c0, y, cy, gates, wm = ctx.saved_tensors
        T, B, H = y.shape
        G = 4 * H
        dev = y.device
        Hw = w_hh.shape[1]                                  # H, or the padded row length of the dropped matrix
        dy = None if dy is None else _f32c(dy)
        dhT = None if dhT is None else _f32c(dhT)
        dcT = None if dcT is None else _f32c(dcT)
        Gp = int(lib.nnl_lstm_padded_gates(H))
        w_t = torch.empty(Hw, G, dtype=torch.float32, device=dev)        # rows >= H (the zero pad columns of w_hh) are never read
        check(lib.nnl_conv2d_weight_transpose(ptr(w_hh), ptr(w_t), G, 1, 1, Hw, stream()))
        if Gp != G:
            w_t = F.pad(w_t, (0, Gp - G))
        dgates = torch.empty(T, B, Gp, dtype=torch.float32, device=dev)
        if Gp != G:
            dgates[:, :, G:].zero_()                         # only the pad columns must be zero (round 4 zero-filled all 82 MB per layer)
        dh0 = torch.empty(B, H, dtype=torch.float32, device=dev)
        dc0 = torch.empty(B, H, dtype=torch.float32, device=dev)
        from .ops import _workspace, lstm_timeout_flag
        wsb = int(lib.nnl_lstm_workspace_bytes(T, B, H))
        ws = _workspace(wsb, dev)
        check(lib.nnl_lstm_bwd(ptr(dy), ptr(dhT), ptr(dcT), ptr(gates), ptr(cy), ptr(c0), ptr(w_t), ptr(dgates), ptr(dh0),
                               ptr(dc0), T, B, H, ptr(ws), wsb, ptr(lstm_timeout_flag(dev)), stream()))
        dw = None
        if ctx.needs_input_grad[1]:
            # dW_hh[4H,H] = sum_t dgates_t^T h_{t-1}: the wgrad kernel on a 1x1 "conv" over T*B "pixels"
            Hp = _ceil4(H)
            # h_{t-1} for t = 0 .. T-1, rows padded to Hp: ONE big strided copy (round 4: cat + pad = a copy, a fill and another copy)
            hprev = torch.empty(T, B, Hp, dtype=torch.float32, device=dev)
            hprev[0, :, :H] = h0
            if T > 1:
                hprev[1:, :, :H] = y[:-1]
            if Hp != H:
                hprev[:, :, H:].zero_()
            hprev = hprev.view(T * B, Hp)
            g = _lib.ConvGeom(T * B, 1, 1, Hp, Gp, 1, 1, 1, 0, 1, 1)
            dwp = torch.empty(Gp, Hp, dtype=torch.float32, device=dev)
            wb = int(lib.nnl_conv2d_wgrad_workspace_bytes(g))
            wws = _workspace(wb, dev, floor=True)             # never a null
            use, p, seed = ctx.drop
            dw = torch.empty(G, H, dtype=torch.float32, device=dev) if use else dwp[:G, :H]
            check(lib.nnl_conv2d_wgrad(ptr(hprev), ptr(dgates.view(T * B, Gp)), ptr(dwp), g, ptr(wws), wb, stream()))
            if use:                                          # dW_raw = dW * m, un-padded in the same pass
                check(lib.nnl_weight_drop(ptr(dwp), Hp, ptr(wm), ptr(dw), H, G, H, seed, p, stream()))
        if Gp != G:
            from .ops import register_padded_grad
            register_padded_grad(dgates, Gp)                 # rows already padded with zeros: the input GEMM's backward uses them as is
        return dgates[:, :, :G], dw, dh0.view_as(h0), dc0.view_as(c0), None, None, None


def lstm_layer(x, h0, c0, w_ih, w_hh, b_ih, b_hh, weight_mask=None, weight_p=0.0):
    """One-layer LSTM over x [T,B,I] with initial state (h0, c0) [1,B,H] (or [B,H]).  w_hh is the RAW recurrent matrix: the
    weight drop of WeightDropLSTM1 (Text.py:495-513) happens inside (`weight_mask`: an explicit scaled mask; else a fresh
    Bernoulli(1 - weight_p) mask per call, its seed drawn from torch's CPU generator so `torch.manual_seed` governs it).
    Returns y [T,B,H], (hT [1,B,H], cT [1,B,H]) like nn.LSTM."""
    from . import ops
    T, B, _ = x.shape
    H = w_hh.shape[1]
    gx = ops.linear(x.reshape(T * B, -1), w_ih, b_ih + b_hh).view(T, B, 4 * H)
    seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if (weight_mask is None and weight_p > 0) else 0
    y, hT, cT = _LSTMRecurrence.apply(gx, w_hh, h0.reshape(B, H), c0.reshape(B, H), weight_mask, float(weight_p), seed)
    return y, (hT.view(1, B, H), cT.view(1, B, H))


class _EmbeddingRowMask(torch.autograd.Function):
    """F.embedding(x, W * mask[V,1], padding_idx) (reference Applications/Text.py:473-474) without materialising W*mask."""

    @staticmethod
    def forward(ctx, x, W, rowmask, padding_idx):
        from .ops import index_error_flag
        require_cuda(x, W, rowmask)
        xi = x.contiguous().long()
        W = _f32c(W)
        rm = None if rowmask is None else _f32c(rowmask).view(-1)
        V, D = W.shape
        out = torch.empty(xi.numel(), D, dtype=torch.float32, device=W.device)
        check(lib.nnl_embedding_rowmask_fwd(ptr(xi), ptr(W), ptr(rm), ptr(out), xi.numel(), V, D,
                                            ptr(index_error_flag(W.device)), stream()))
        ctx.save_for_backward(xi, rm)
        ctx.meta = (V, D, -1 if padding_idx is None else int(padding_idx))
        return out.view(*x.shape, D)

    @staticmethod
    def backward(ctx, dout):
        from .ops import _workspace
        xi, rm = ctx.saved_tensors
        V, D, pad = ctx.meta
        dout = _f32c(dout)
        dW = torch.empty(V, D, dtype=torch.float32, device=dout.device)
        wsb = int(lib.nnl_embedding_rowmask_bwd_workspace_bytes(xi.numel()))         # sample-order (deterministic) scatter-add
        ws = _workspace(wsb, dout.device, floor=True)                                 # never a null
        check(lib.nnl_embedding_rowmask_bwd(ptr(xi), ptr(rm), ptr(dout), ptr(dW), xi.numel(), V, D, pad, ptr(ws), wsb, stream()))
        return None, dW, None, None


def embedding_rowmask(x, W, rowmask=None, padding_idx=None):
    return _EmbeddingRowMask.apply(x, W, rowmask, padding_idx)


class _SoftmaxCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target):
        from .ops import index_error_flag
        require_cuda(logits, target)
        logits = _f32c(logits)
        target = target.contiguous().long()
        rows, V = logits.shape
        dev = logits.device
        stats = torch.empty(rows, 2, dtype=torch.float32, device=dev)      # {max, log sum exp(x - max)} per row, kept apart
        loss_rows = torch.empty(rows, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        check(lib.nnl_softmax_ce_fwd(ptr(logits), ptr(target), ptr(stats), ptr(loss_rows), ptr(loss), rows, V,
                                     ptr(index_error_flag(dev)), stream()))
        ctx.save_for_backward(logits, target, stats)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        logits, target, stats = ctx.saved_tensors
        from .ops import register_padded_grad
        g = _f32c(dloss).view(1)
        rows, V = logits.shape
        Vp = (V + 15) // 16 * 16
        # rows padded to the GEMM granularity (zeros in the pad columns): the producing linear layer's backward uses the buffer as
        # is instead of re-padding it (V = 47 343: an 848 MB fill + copy per step)
        buf = torch.empty(rows, Vp, dtype=torch.float32, device=logits.device)
        check(lib.nnl_softmax_ce_bwd(ptr(logits), ptr(target), ptr(stats), ptr(g), ptr(buf), rows, V, Vp, stream()))
        if Vp == V:
            return buf, None
        register_padded_grad(buf, Vp)
        return buf[:, :V], None


def softmax_cross_entropy(logits, target):
    """mean_r( logsumexp(logits[r]) - logits[r, target[r]] ) for logits [rows, V], target [rows]."""
    return _SoftmaxCE.apply(logits, target)


def cross_entropy_nd(preds, target):
    """F.cross_entropy(preds, target) for class-dim-1 inputs: [N,C] with target [N], or [N,C,d1..] with [N,d1..]."""
    if preds.dim() == 2:
        return softmax_cross_entropy(preds, target)
    C = preds.shape[1]
    if preds.dim() == 3 and preds.permute(2, 0, 1).is_contiguous():
        # the language-model decoder returns lin(x).permute(1,2,0): a [bs,V,seq] VIEW of a contiguous [seq,bs,V]
        # buffer (Text.py:572) — use that buffer as is (the mean does not depend on the row order)
        return softmax_cross_entropy(preds.permute(2, 0, 1).reshape(-1, C), target.transpose(0, 1).reshape(-1))
    perm = [0] + list(range(2, preds.dim())) + [1]
    return softmax_cross_entropy(preds.permute(*perm).reshape(-1, C), target.reshape(-1))


class _SeqReg(torch.autograd.Function):
    """alpha * mean(h^2) + beta * mean((h[1:] - h[:-1])^2) for h = enc_out [T, bs, E] (reference Text.py:765-777: the AR / TAR
    terms of RegSeqCrossEntropyLoss) — one reduction pass forward, one elementwise pass backward."""

    @staticmethod
    def forward(ctx, h, alpha, beta):
        from .ops import _workspace
        require_cuda(h)
        h = _f32c(h)
        T = h.shape[0]
        R = h.numel() // max(T, 1)
        out = torch.empty(3, dtype=torch.float32, device=h.device)
        wsb = int(lib.nnl_seq_reg_workspace_bytes(T, R))
        ws = _workspace(wsb, h.device, floor=True)          # never a null
        check(lib.nnl_seq_reg_fwd(ptr(h), ptr(out), T, R, float(alpha), float(beta), ptr(ws), wsb, stream()))
        ctx.save_for_backward(h)
        ctx.ab = (float(alpha), float(beta))
        return out[0]

    @staticmethod
    def backward(ctx, dout):
        h, = ctx.saved_tensors
        T = h.shape[0]
        R = h.numel() // max(T, 1)
        g = _f32c(dout).reshape(1)
        dh = torch.empty_like(h)
        check(lib.nnl_seq_reg_bwd(ptr(h), ptr(g), ptr(dh), T, R, ctx.ab[0], ctx.ab[1], stream()))
        return dh, None, None


def seq_activation_reg(enc_out, alpha, beta):
    "AR + TAR regulariser of RegSeqCrossEntropyLoss as a 0-dim tensor (see _SeqReg)"
    return _SeqReg.apply(enc_out, float(alpha), float(beta))


class _AttentionPool(torch.autograd.Function):
    """TextClassificationDecoder's attention pooling after attn1 (reference Text.py:598-605): scores h.w2 + b2, softmax over the
    non-pad timesteps of each column, attention-weighted sum of enc_out — nnl_attn_pool_fwd / _bwd.  Saves h, enc_out and attn;
    no host synchronisation either way."""

    @staticmethod
    def forward(ctx, h, w2, b2, enc_out, x, pad_token):
        from .ops import _tile_counters, _workspace
        require_cuda(h, w2, b2, enc_out, x)
        ctx.w2_shape, ctx.b2_shape = w2.shape, b2.shape
        h, enc_out = _f32c(h), _f32c(enc_out)
        w2, b2 = _f32c(w2).view(-1), _f32c(b2).view(-1)
        T, B, E = enc_out.shape
        A = h.shape[2]
        if tuple(h.shape) != (T, B, A) or w2.numel() != A or b2.numel() != 1 or tuple(x.shape) != (B, T):
            raise _lib.NnlError('attention_pool: shapes h %s, w2 %s, b2 %s, enc_out %s, x %s do not match'
                                % (tuple(h.shape), tuple(w2.shape), tuple(b2.shape), tuple(enc_out.shape), tuple(x.shape)))
        xi = x.contiguous().long()
        dev = enc_out.device
        attn = torch.empty(T, B, dtype=torch.float32, device=dev)
        pooled = torch.empty(B, E, dtype=torch.float32, device=dev)
        wsb = int(lib.nnl_attn_pool_workspace_bytes(T, B, E, A))
        ws = _workspace(wsb, dev)
        cnt = _tile_counters(dev)
        check(lib.nnl_attn_pool_fwd(ptr(h), ptr(w2), ptr(b2), ptr(enc_out), ptr(xi), int(pad_token), ptr(attn), ptr(pooled),
                                    T, B, E, A, ptr(ws), wsb, ptr(cnt), cnt.numel(), stream()))
        ctx.save_for_backward(h, w2, enc_out, attn)
        ctx.set_materialize_grads(False)                 # training never uses attn: its gradient stays None (no [T,B] zero fill)
        return attn, pooled

    @staticmethod
    def backward(ctx, dattn, dpooled):
        from .ops import _tile_counters, _workspace
        h, w2, enc_out, attn = ctx.saved_tensors
        T, B, E = enc_out.shape
        A = h.shape[2]
        dev = enc_out.device
        dpooled = torch.zeros(B, E, dtype=torch.float32, device=dev) if dpooled is None else _f32c(dpooled)
        dattn = None if dattn is None else _f32c(dattn)
        dh = torch.empty_like(h)
        denc = torch.empty_like(enc_out)
        dw2 = torch.empty(A, dtype=torch.float32, device=dev)
        db2 = torch.empty(1, dtype=torch.float32, device=dev)
        wsb = int(lib.nnl_attn_pool_workspace_bytes(T, B, E, A))
        ws = _workspace(wsb, dev)
        cnt = _tile_counters(dev)
        check(lib.nnl_attn_pool_bwd(ptr(h), ptr(w2), ptr(enc_out), ptr(attn), ptr(dpooled), ptr(dattn), ptr(dh), ptr(denc),
                                    ptr(dw2), ptr(db2), T, B, E, A, ptr(ws), wsb, ptr(cnt), cnt.numel(), stream()))
        return dh, dw2.view(ctx.w2_shape), db2.view(ctx.b2_shape), denc, None, None


def attention_pool(h, w2, b2, enc_out, x, pad_token=1):
    """h = relu(attn1(enc_out)) [T,B,A], attn2's weight w2 [1,A] and bias b2 [1], enc_out [T,B,E], tokens x [B,T] ->
    (attn [T,B], pooled [B,E]) of TextClassificationDecoder (reference Text.py:597-605; pad token 1 is hard-coded there).
    A column without a non-pad token gives NaN, as the reference's 0/0 does."""
    return _AttentionPool.apply(h, w2, b2, enc_out, x, pad_token)


# ---- text generation (K5d): batch 1, one timestep; no autograd ---------------------------------------------------------------------

def padded_rows(w, w_hh=False):
    """w [R, C] fp32 with rows padded with zeros to a multiple of 4 floats (16-byte rows for nnl_lstm_cell_b1 / nnl_lm_next_token);
    w itself when C already is one.  w_hh=True pads through nnl_weight_drop (p = 0, no mask), as the LSTM layer does."""
    require_cuda(w)
    w = _f32c(w.detach())
    R, Cc = w.shape
    Cp = _ceil4(Cc)
    if Cp == Cc:
        return w
    out = torch.empty(R, Cp, dtype=torch.float32, device=w.device)
    if w_hh:
        check(lib.nnl_weight_drop(ptr(w), Cc, None, ptr(out), Cp, R, Cc, 0, 0.0, stream()))
    else:
        check(lib.nnl_pad_cols(ptr(w), ptr(out), R, Cc, Cp, stream()))
    return out


class LstmCellB1:
    """One LSTM layer, one timestep, batch 1 (nnl_lstm_cell_b1; reference Text.py:655-676 runs it through nn.LSTM) on fixed buffers:
    w_ih [4H, ldi] and w_hh [4H, ldh] with zero-padded rows (`padded_rows`), bias = b_ih + b_hh [4H], h [ldh] and x [ldi] zero-padded
    vectors, c [H].  A call writes h_out[:H] (must not be h) and c_out[:H] (may be c).  x=None: the input is row tokens[pos] of emb,
    read on the device.  Every argument is converted once here, so that a decode loop pays one foreign call per launch."""

    def __init__(self, w_ih, w_hh, bias, h, c, h_out, c_out, I, H, x=None, emb=None, tokens=None):
        require_cuda(w_ih, w_hh, bias, h, c, h_out, c_out, x, emb, tokens)
        self._keep = (w_ih, w_hh, bias, h, c, h_out, c_out, x, emb, tokens)
        ld_emb, V = (emb.stride(0), emb.shape[0]) if emb is not None else (0, 0)
        self._head = (ptr(w_ih), w_ih.stride(0), ptr(w_hh), w_hh.stride(0), ptr(bias), ptr(x), ptr(emb), ld_emb, ptr(tokens))
        self._tail = (V, ptr(h), ptr(c), ptr(h_out), ptr(c_out), int(I), int(H))

    def __call__(self, pos=0, on_stream=None):
        check(lib.nnl_lstm_cell_b1(*self._head, int(pos), *self._tail, on_stream or stream()))


def lstm_cell_b1(w_ih, w_hh, bias, h, c, h_out, c_out, I, H, x=None, emb=None, tokens=None, pos=0):
    "one call of LstmCellB1 (see there); returns (h_out, c_out)"
    LstmCellB1(w_ih, w_hh, bias, h, c, h_out, c_out, I, H, x, emb, tokens)(pos)
    return h_out, c_out


def lm_next_token_workspace(V, k, device):
    return torch.empty(max(int(lib.nnl_lm_next_token_workspace_bytes(V, k)) // 4, 1), dtype=torch.float32, device=device)


class LmNextToken:
    """The rest of a generated token (nnl_lm_next_token; reference Text.py:667-672) on fixed buffers: tied decoder emb [V, ld] . h [E],
    softmax over all V, the first n_special entries excluded, top-k, and the draw with the uniform u[step].  A call (h, step, pos)
    writes tokens[pos + 1] (int64, on the device) and, if given, row `step` of top_probs / top_indices [*, k].  Nothing is read back."""

    def __init__(self, emb, k, u, tokens, top_probs=None, top_indices=None, n_special=4, E=None, logits_out=None, workspace=None):
        require_cuda(emb, u, tokens, top_probs, top_indices, logits_out, workspace)
        V = emb.shape[0]
        ws = lm_next_token_workspace(V, k, emb.device) if workspace is None else workspace
        self._keep = (emb, u, tokens, top_probs, top_indices, logits_out, ws)
        self._emb = (ptr(emb), emb.stride(0))
        self._mid = (V, emb.shape[1] if E is None else int(E), int(k), int(n_special), ptr(u))
        self._tokens = ptr(tokens)
        self._tail = (ptr(top_probs), ptr(top_indices), ptr(logits_out), ptr(ws), ws.numel() * 4)

    def __call__(self, h, step, pos, on_stream=None):
        require_cuda(h)
        check(lib.nnl_lm_next_token(*self._emb, ptr(h), *self._mid, int(step), self._tokens, int(pos), *self._tail, on_stream or stream()))


def lm_next_token(emb, h, k, u, step, tokens, pos, top_probs=None, top_indices=None, n_special=4, E=None, logits_out=None,
                  workspace=None):
    "one call of LmNextToken (see there); returns tokens"
    LmNextToken(emb, k, u, tokens, top_probs, top_indices, n_special, E, logits_out, workspace)(h, step, pos)
    return tokens


# ---- tokeniser and vocabulary (K17, csrc/text_tokens.hip): a corpus is one resident byte buffer ---------------------------------------

TEXT_TILE = 1024                         # NNL_TEXT_TILE: bytes per scan tile (tests place tokens on its edges)
TEXT_TUP_LEN = -1                        # NNL_TEXT_TUP_LEN: tok_len of the pseudo-token t_up
TEXT_MODE_GRAMMAR, TEXT_MODE_SPLIT = 0, 1
TEXT_STATUS_OVERFLOW = 1
TEXT_MAX_BYTES = 2 ** 31 - 1
TEXT_HASH_MASK = 2 ** 64 - 1             # the product path keeps all 64 key bits; tests narrow it to force collisions
TEXT_SEEDS = (0x243F6A8885A308D3, 0x13198A2E03707344, 0xA4093822299F31D0)      # a mismatch retries with the next; then RuntimeError
TEXT_SPECIALS = ('_unk_', '_pad_', '_bos_', '_eos_')


def _text_device(device=None):
    return torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)


class TextCorpus:
    """Texts as ONE byte buffer on the device plus their offsets: `data` bytes [B] (B < 2^31, else ValueError: chunking is not built),
    `offsets` n + 1 non-decreasing ints from 0 to B, text j = data[offsets[j]:offsets[j + 1]].  Offsets and bytes travel in one upload.
    `host` keeps the bytes for decoding the few strings the host needs (the vocabulary)."""

    def __init__(self, data, offsets, device=None):
        import numpy as np
        data = bytes(data)
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64).reshape(-1))
        if len(data) > TEXT_MAX_BYTES:
            raise ValueError('TextCorpus: %d bytes; one resident buffer holds fewer than 2^31 (chunking is not built)' % len(data))
        if off.size < 2 or off[0] != 0 or off[-1] != len(data) or (np.diff(off) < 0).any():
            raise ValueError('TextCorpus: offsets must be n + 1 >= 2 non-decreasing values from 0 to len(data)')
        self.host, self.host_offsets, self.n, self.B = data, off, off.size - 1, len(data)
        head = off.size * 8
        buf = np.empty(head + max(self.B, 1), dtype=np.uint8)
        buf[:head] = off.view(np.uint8)
        buf[head:head + self.B] = np.frombuffer(data, dtype=np.uint8)
        dev = torch.from_numpy(buf).to(_text_device(device))
        self.offsets, self.bytes = dev[:head].view(torch.int64), dev[head:]

    @classmethod
    def from_texts(cls, texts, device=None):
        "texts: byte strings, laid end to end (the grammar never looks across a text boundary, so no separator is needed)"
        import numpy as np
        texts = [bytes(t) for t in texts]
        if not texts:
            raise ValueError('TextCorpus: no texts')
        off = np.zeros(len(texts) + 1, dtype=np.int64)
        np.cumsum([len(t) for t in texts], out=off[1:])
        if off[-1] > TEXT_MAX_BYTES:
            raise ValueError('TextCorpus: %d bytes; one resident buffer holds fewer than 2^31 (chunking is not built)' % off[-1])
        return cls(b''.join(texts), off, device)


class TextTokens:
    "token records of a corpus on the device: start / len int32 [T] (len TEXT_TUP_LEN = the pseudo-token t_up), text_off int64 [n + 1]"

    def __init__(self, start, length, text_off, T, mode):
        self.start, self.len, self.text_off, self.T, self.mode = start, length, text_off, T, mode


def token_bounds(corpus, mode=TEXT_MODE_GRAMMAR):
    """Cuts `corpus` into tokens (nnl_text_token_count, one read of the total, nnl_text_token_fill).  The records and the per-text
    token offsets share one int64 buffer [T + n + 1] so that ids and offsets later come back in one copy (see text_numericalize)."""
    require_cuda(corpus.bytes)
    dev = corpus.bytes.device
    ntiles = (corpus.B + TEXT_TILE - 1) // TEXT_TILE
    tile_base = torch.empty(ntiles + 1, dtype=torch.int64, device=dev)
    check(lib.nnl_text_token_count(ptr(corpus.bytes), corpus.B, ptr(corpus.offsets), corpus.n, int(mode), ptr(tile_base), stream()))
    T = int(tile_base[-1].item())
    rec = torch.empty(2, max(T, 1), dtype=torch.int32, device=dev)
    text_off = torch.empty(corpus.n + 1, dtype=torch.int64, device=dev)
    check(lib.nnl_text_token_fill(ptr(corpus.bytes), corpus.B, ptr(corpus.offsets), corpus.n, int(mode), ptr(tile_base), T, ptr(rec[0]),
                                  ptr(rec[1]), ptr(text_off), stream()))
    return TextTokens(rec[0], rec[1], text_off, T, int(mode))


def token_hash(corpus, toks, seed, hash_mask=None):
    "uint64 keys [T] (as an int64 tensor) of the tokens' lowered bytes (nnl_text_token_hash); key 0 never occurs"
    mask = TEXT_HASH_MASK if hash_mask is None else int(hash_mask)
    keys = torch.empty(max(toks.T, 1), dtype=torch.int64, device=corpus.bytes.device)
    check(lib.nnl_text_token_hash(ptr(corpus.bytes), corpus.B, ptr(toks.start), ptr(toks.len), toks.T, toks.mode, int(seed) & (2 ** 64 - 1),
                                  mask, ptr(keys), stream()))
    return keys


def vocab_capacity(T):
    "the table size for T tokens: a power of two >= 2 T and >= 1024"
    cap = 1024
    while cap < 2 * T:
        cap *= 2
    return cap


class VocabTable:
    "caller-allocated open-addressing table: key uint64 [cap] (0 = empty), count int32 [cap], first int32 [cap], status int32 [1]"

    def __init__(self, cap, device=None):
        dev = _text_device(device)
        self.cap = int(cap)
        self.key = torch.empty(self.cap, dtype=torch.int64, device=dev)
        self.count = torch.empty(self.cap, dtype=torch.int32, device=dev)
        self.first = torch.empty(self.cap, dtype=torch.int32, device=dev)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)


def vocab_insert(keys, T, table, reset=True):
    """The raw insert (nnl_text_vocab_insert): returns tok_slot int32 [T] (-1 = no slot found).  table.status gets the overflow bit;
    the call itself always returns: the probe loop ends after table.cap steps."""
    tok_slot = torch.empty(max(T, 1), dtype=torch.int32, device=keys.device)
    check(lib.nnl_text_vocab_insert(ptr(keys), T, ptr(table.key), ptr(table.count), ptr(table.first), table.cap, 1 if reset else 0,
                                    ptr(tok_slot), ptr(table.status), stream()))
    return tok_slot


def vocab_verify(corpus, toks, tok_slot, table, first_corpus=None, first_toks=None):
    "the number of tokens whose bytes differ from the first token of their slot (nnl_text_vocab_verify); 0 = the table is exact"
    fc, ft = first_corpus or corpus, first_toks or toks
    mism = torch.zeros(1, dtype=torch.int32, device=corpus.bytes.device)
    check(lib.nnl_text_vocab_verify(ptr(corpus.bytes), corpus.B, ptr(toks.start), ptr(toks.len), ptr(tok_slot), toks.T, toks.mode,
                                    ptr(fc.bytes), fc.B, ptr(ft.start), ptr(ft.len), ft.T, ft.mode, ptr(table.first), table.cap, ptr(mism),
                                    stream()))
    return mism


def vocab_build(corpus, toks, seed, hash_mask=None, cap=None):
    """hash, insert and verify with ONE seed: (table, tok_slot, mismatches).  RuntimeError if the table overflowed; a non-zero
    mismatch count means two different strings share a slot and the table must not be used (vocab_build_exact retries)."""
    keys = token_hash(corpus, toks, seed, hash_mask)
    table = VocabTable(vocab_capacity(toks.T) if cap is None else cap, corpus.bytes.device)
    tok_slot = vocab_insert(keys, toks.T, table)
    mism = vocab_verify(corpus, toks, tok_slot, table)
    status, mism = (int(v) for v in torch.cat([table.status, mism]).tolist())          # one small read for both
    if status & TEXT_STATUS_OVERFLOW:
        raise RuntimeError('text vocabulary: the table of %d slots overflowed (%d tokens)' % (table.cap, toks.T))
    return table, tok_slot, mism


def vocab_build_exact(corpus, toks, hash_mask=None, cap=None):
    "vocab_build over TEXT_SEEDS until no token mismatches its slot: (table, tok_slot, seed); RuntimeError after the last seed"
    for seed in TEXT_SEEDS:
        table, tok_slot, mism = vocab_build(corpus, toks, seed, hash_mask, cap)
        if mism == 0:
            return table, tok_slot, seed
    raise RuntimeError('text vocabulary: hash collisions under %d seeds in a row (%d tokens still differ from their slot)' % (len(TEXT_SEEDS), mism))


def vocab_compact(table, toks):
    """The occupied slots as a numpy int32 array [K, 5] = (slot, count, first, tok_start[first], tok_len[first]), sorted by `first`
    (nnl_text_vocab_compact writes them in no particular order).  Counts and first indices are the same on every call; the slot
    numbers depend on which of two colliding keys arrived first."""
    dev = table.key.device
    max_rows = max(min(table.cap, toks.T), 1)
    out = torch.zeros(max_rows * 5 + 1, dtype=torch.int32, device=dev)           # rows, then the row counter: one copy back
    check(lib.nnl_text_vocab_compact(ptr(table.key), ptr(table.count), ptr(table.first), table.cap, ptr(toks.start), ptr(toks.len), toks.T,
                                     ptr(out), max_rows, ptr(out[max_rows * 5:]), stream()))
    host = out.cpu().numpy()
    K = int(host[-1])
    if K > max_rows:
        raise RuntimeError('text vocabulary: %d occupied slots for %d tokens' % (K, toks.T))
    rows = host[:K * 5].reshape(K, 5)
    return rows[rows[:, 2].argsort(kind='stable')]


def vocab_assign(table, slots, ids):
    "slot_id int32 [cap]: 0 everywhere but slot_id[slots[k]] = ids[k] (nnl_text_vocab_assign); slots, ids: host integer sequences"
    import numpy as np
    dev = table.key.device
    K = len(slots)
    both = np.zeros((2, max(K, 1)), dtype=np.int32)
    both[0, :K], both[1, :K] = slots, ids
    both = torch.from_numpy(both).to(dev)
    slot_id = torch.empty(table.cap, dtype=torch.int32, device=dev)
    check(lib.nnl_text_vocab_assign(ptr(both[0]), ptr(both[1]), K, ptr(slot_id), table.cap, stream()))
    return slot_id


def vocab_lookup(corpus, toks, keys, vcorpus, vtoks, table):
    "tok_slot int32 [T]: the slot of the vocabulary string equal to each token, -1 if there is none (nnl_text_vocab_lookup)"
    tok_slot = torch.empty(max(toks.T, 1), dtype=torch.int32, device=corpus.bytes.device)
    check(lib.nnl_text_vocab_lookup(ptr(corpus.bytes), corpus.B, ptr(toks.start), ptr(toks.len), ptr(keys), toks.T, toks.mode,
                                    ptr(vcorpus.bytes), vcorpus.B, ptr(vtoks.start), ptr(vtoks.len), vtoks.T, ptr(table.key), ptr(table.first),
                                    table.cap, ptr(tok_slot), stream()))
    return tok_slot


def ids_write(tok_slot, slot_id, cap, toks, n, reverse=False, out=None):
    "ids int64 [T] = slot_id[tok_slot] (0 where tok_slot < 0), every text's tokens mirrored if `reverse` (nnl_text_ids_write)"
    ids = torch.empty(max(toks.T, 1), dtype=torch.int64, device=tok_slot.device) if out is None else out
    check(lib.nnl_text_ids_write(ptr(tok_slot), ptr(slot_id), int(cap), ptr(toks.text_off), int(n), toks.T, 1 if reverse else 0, ptr(ids), stream()))
    return ids


def _token_string(corpus, start, length, lower):
    if length == TEXT_TUP_LEN:
        return 't_up'
    b = corpus.host[start:start + length]
    return (b.lower() if lower else b).decode('utf-8', 'surrogateescape')        # bytes.lower() lowers A-Z only


def token_strings(corpus, toks):
    "the tokens of every text as Python strings: list (per text) of lists — one copy back of the records, then host slicing"
    import numpy as np
    rec = torch.stack([toks.start, toks.len]).cpu().numpy()
    off = toks.text_off.cpu().numpy()
    data = corpus.host.lower() if toks.mode == TEXT_MODE_GRAMMAR else corpus.host
    out = []
    for j in range(corpus.n):
        row = []
        for t in range(int(off[j]), int(off[j + 1])):
            s, l = int(rec[0, t]), int(rec[1, t])
            row.append('t_up' if l == TEXT_TUP_LEN else data[s:s + l].decode('utf-8', 'surrogateescape'))
        out.append(row)
    return out


class TextIds:
    """What text_numericalize returns: ids int64 [T] and offsets int64 [n + 1] (numpy; text j = ids[offsets[j]:offsets[j + 1]]), the
    stoi dict, and, for a vocabulary built here, counts = {token: occurrences} of the kept tokens (None for a given stoi)."""

    def __init__(self, ids, offsets, stoi, counts):
        self.ids, self.offsets, self.stoi, self.counts = ids, offsets, stoi, counts

    def lists(self):
        flat = self.ids.tolist()
        off = self.offsets.tolist()
        return [flat[off[j]:off[j + 1]] for j in range(len(off) - 1)]


def text_numericalize(corpus, mode, max_vocab=60000, min_freq=6, stoi=None, reverse=False, hash_mask=None, cap=None):
    """Token ids of every text of `corpus`, on the device end to end: token bounds, then either a vocabulary built from the corpus
    (stoi=None: hash, insert, verify, compact; the host sorts the distinct tokens by (-count, first occurrence), cuts at max_vocab, THEN
    drops count < min_freq — numericalize's order, Text.py:113-114 — and prefixes TEXT_SPECIALS) or a lookup in the given `stoi`
    (absent tokens give 0).  A hash collision is detected, never merged: the build retries with the next seed and raises RuntimeError
    after the last, as it does when the table overflows.  Only the kept vocabulary strings (and the distinct tokens as long as a special,
    to find one spelled like it) are decoded on the host."""
    import numpy as np
    toks = token_bounds(corpus, mode)
    dev = corpus.bytes.device
    lower = mode == TEXT_MODE_GRAMMAR
    counts = None
    if stoi is None:
        names, counts = list(TEXT_SPECIALS), {}
        if toks.T:
            table, tok_slot, _ = vocab_build_exact(corpus, toks, hash_mask, cap)
            rows = vocab_compact(table, toks)
            order = np.lexsort((rows[:, 2], -rows[:, 1].astype(np.int64)))[:max_vocab]
            kept = rows[order]
            kept = kept[kept[:, 1] >= min_freq]
            for slot, count, first, start, length in kept.tolist():
                names.append(_token_string(corpus, start, length, lower))
                counts[names[-1]] = count
            slots, ids = kept[:, 0].tolist(), list(range(len(TEXT_SPECIALS), len(names)))        # the id is the position in `names`
            # a corpus token spelled like a special that was NOT kept still finds the special's entry in stoi (Text.py:119-120)
            for slot, count, first, start, length in rows[np.isin(rows[:, 4], [len(s) for s in TEXT_SPECIALS])].tolist():
                s = _token_string(corpus, start, length, lower)
                if s in TEXT_SPECIALS and s not in counts:
                    slots.append(slot)
                    ids.append(TEXT_SPECIALS.index(s))
            slot_id = vocab_assign(table, slots, ids)
        stoi = {s: i for i, s in enumerate(names)}     # as Text.py:117: a corpus token spelled like a special takes the later position
    else:
        vocab = list(stoi.items())
        if any(not (0 <= int(i) < 2 ** 31) for _, i in vocab):
            raise ValueError('text_numericalize: stoi values must lie in [0, 2^31)')
        if toks.T and vocab:
            vcorpus = TextCorpus.from_texts([s.encode('utf-8', 'surrogateescape') for s, _ in vocab], dev)
            vrec = np.stack([vcorpus.host_offsets[:-1], np.diff(vcorpus.host_offsets)]).astype(np.int32)
            vrec = torch.from_numpy(vrec).to(dev)
            vtoks = TextTokens(vrec[0], vrec[1], vcorpus.offsets, len(vocab), TEXT_MODE_SPLIT)     # each string is one token, as it is
            table, _, seed = vocab_build_exact(vcorpus, vtoks, hash_mask, cap)
            rows = vocab_compact(table, vtoks)
            slot_id = vocab_assign(table, rows[:, 0], [int(vocab[f][1]) for f in rows[:, 2].tolist()])
            tok_slot = vocab_lookup(corpus, toks, token_hash(corpus, toks, seed, hash_mask), vcorpus, vtoks, table)
        elif toks.T:
            table = VocabTable(16, dev)
            tok_slot = torch.full((toks.T,), -1, dtype=torch.int32, device=dev)
            slot_id = torch.zeros(16, dtype=torch.int32, device=dev)
    both = torch.empty(toks.T + corpus.n + 1, dtype=torch.int64, device=dev)      # ids | offsets: one copy back
    both[toks.T:] = toks.text_off
    if toks.T:
        ids_write(tok_slot, slot_id, table.cap, toks, corpus.n, reverse, out=both)
    host = both.cpu().numpy()
    return TextIds(host[:toks.T], host[toks.T:], stoi, counts)
