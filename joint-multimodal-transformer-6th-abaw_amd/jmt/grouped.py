"""Grouped execution of the JMT block's parallel branches (MultimodalTransformer_w_JR,
mm_multi_transformers.py:118-214): the three encoders and the six cross-attentions run as
batched launches instead of 3 / 6 separate ones.

The reference applies three same-shaped TransformerEncoderLayers to v, a and the joint
representation (:132-136), then three nn.MultiheadAttention modules twice each (:142-167), then
`out_layer1` to the concatenation of the six outputs (:201-211).  Here the three encoder inputs
live in ONE stacked buffer X (3, B, T, E); every GEMM of the three encoders is one launch whose
per-batch operands come from pointer tables (weights, biases, gradient buffers: each module keeps
its own nn.Parameters, so state_dict keys are untouched), the attention core runs over 3B
sequences in one launch, and the six cross-attentions likewise over 6 stacked (query, key) pairs.
The backward of each group is written out explicitly: gradients that the reference's autograd
would sum from several uses (a stream's encoder output feeds 4 projections) are produced by ONE
K-concatenated dgrad GEMM per stream (K = 6E; 5E with one dQ per shared query, see
CrossAttention6Fn), and weight gradients are accumulated in place
(beta = 1) by batched wgrad GEMMs — no autograd adds, no cross-stream synchronisation, and a
single HIP stream that captures into a hipGraph (jmt/graph.py).

Every GEMM here is linear_gemm.fwd / dgrad / wgrad on Operands built from the stacked buffers
(lg.strided for a whole (G, B, T, F) buffer, lg.table / lg.ksegs of (tensor, offset) blocks for a
selection of groups); bias sums that a weight gradient cannot fuse go through lg.bias_grad.  A
weight gradient held for the end of the backward pass keeps its operands through the Operands
themselves: a call site says `intact=` and never lists tensors.

Stacked layouts (compute dtype, row-major, rows in (b, t) order per group):
  X, Y   (G, B, T, E)     encoder group input / output            G = 3
  QKV    (G', B, T, 3E)   packed in-projection outputs            G' = 3 (encoders), 6 (pairs)
  O      (G', B, T, E)    attention outputs (before out_proj)
"""
from __future__ import annotations

import os
from typing import List

import torch
from torch.autograd import Function

from . import linear_gemm as lg
from . import ops
from .functional import (AttnOperand, Rows, _cast_keep_layout, _grad_buffer, _grad_done, _match,
                         _operand, _out, _ptr, attn_backward, attn_dropout_rate, attn_forward,
                         attn_plan, compute_dtype, weight_as, wgrad_defer_ok, wgrad_scope)

_enabled = {"on": os.environ.get("JMT_GROUPED", "1") != "0"}

# the six cross-attentions in the reference's order (mm_multi_transformers.py:142-167), which is
# also the order of torch.cat in the FC head (:201-211): (module, query stream, key/value stream)
# with module 0 = cross_attention_v, 1 = cross_attention_p, 2 = cross_attention_pv and stream
# 0 = visual, 1 = physiological (audio), 2 = joint representation.
CROSS_PAIRS = ((0, 0, 1), (1, 1, 0), (2, 2, 0), (0, 0, 2), (2, 2, 1), (1, 1, 2))


def enabled() -> bool:
    return _enabled["on"]


def set_enabled(on: bool) -> None:
    _enabled["on"] = bool(on)


# ------------------------------------------------------------------------- grouped GEMMs
def _kcat_ok(rows: int, n_ptrs: int, cd) -> bool:
    """Whether a per-batch K-segment wgrad (lg.ksegs, jmt_gemm operand mode 3) applies: the
    segment length (rows) a multiple of the 128-B K-tile and the pointer table within 8 entries."""
    return (_merge_wgrads["on"] and cd != torch.float32 and rows % 64 == 0 and n_ptrs <= 8)


# one weight-gradient launch for the two uses of each cross-attention module (K-concatenated
# pairs) and for the encoders' W1 / W2 (JMT_WGRAD_MERGE=0: the round-5 launches, A/B switch)
_merge_wgrads = {"on": os.environ.get("JMT_WGRAD_MERGE", "1") != "0"}


def _contig(t: torch.Tensor, cd) -> torch.Tensor:
    if t.dtype != cd:
        t = ops.cast(t.contiguous(), cd)
    return t if t.is_contiguous() else t.contiguous()


# ------------------------------------------------------------------------- stacking
class StackGroupsFn(Function):
    """X = stack(xs) -> (G, B, T, E) in the compute dtype (one strided copy per stream); the
    backward hands out views of the incoming gradient."""

    @staticmethod
    def forward(ctx, *xs):
        cd = compute_dtype()
        x0 = xs[0]
        B, T, E = x0.shape
        X = torch.empty(len(xs), B, T, E, dtype=cd, device=x0.device)
        for g, x in enumerate(xs):
            assert tuple(x.shape) == (B, T, E), "StackGroupsFn: streams must share (B, T, E)"
            if x.stride(-1) != 1 or x.stride(1) != E * x.stride(2) or x.stride(0) != T * x.stride(1):
                x = x.contiguous()
            ops.copy2d(x.data_ptr(), ops.dt(x), X[g].data_ptr(), ops.dt(X), B * T, E,
                       x.stride(1), 1, E, 1)
        return X

    @staticmethod
    def backward(ctx, dX):
        return tuple(dX[g] for g in range(dX.shape[0]))


def stack_groups(*xs) -> torch.Tensor:
    return StackGroupsFn.apply(*xs)


class JointSlots:
    """StackJointFn's stacked (3, B, T, E) buffer allocated ahead of its producers: they write the
    two streams into slot(0) and slot(1) (`out=` of linear / l2_normalize), and StackJointFn, given
    this object, copies only an input that is not already its slot.  A plain Python object:
    autograd sees the buffer first as StackJointFn's output."""

    def __init__(self, B: int, T: int, E: int, device):
        self.X = torch.empty(3, B, T, E, dtype=compute_dtype(), device=device)

    def slot(self, g: int) -> torch.Tensor:
        return self.X[g]


def _is_slot(x: torch.Tensor, s: torch.Tensor) -> bool:
    """x already is the slot s: same storage, offset, shape, strides and dtype."""
    return (x.dtype == s.dtype and x.device == s.device and
            x.untyped_storage().data_ptr() == s.untyped_storage().data_ptr() and
            x.storage_offset() == s.storage_offset() and x.shape == s.shape and
            x.stride() == s.stride())


class StackJointFn(Function):
    """X = stack(v, p, cat(v, p) W^T + b) -> (3, B, T, E): the two streams and the joint
    representation of out_layer_pv (mm_multi_transformers.py:120-124) in one stacked buffer;
    the K-concatenated GEMM writes the third slot directly.  The backward adds out_layer_pv's
    input gradients into the first two slots of the incoming dX with the dgrad GEMM's beta = 1
    epilogue, so the two uses of v and p need no separate gradient sum.  slots (JointSlots): X
    is the caller's buffer, and an input that already is its slot is not copied."""

    @staticmethod
    def forward(ctx, v, p, W, b, slots=None):
        cd = compute_dtype()
        B, T, E = v.shape
        assert tuple(p.shape) == (B, T, E) and W.shape == (E, 2 * E), (v.shape, p.shape, W.shape)
        if slots is not None and tuple(slots.X.shape) == (3, B, T, E) and slots.X.dtype == cd \
                and slots.X.device == v.device and slots.X.is_contiguous():
            X = slots.X
        else:
            X = torch.empty(3, B, T, E, dtype=cd, device=v.device)
        for g, x in enumerate((v, p)):
            if _is_slot(x, X[g]):
                continue
            if x.stride(-1) != 1 or x.stride(1) != E * x.stride(2) or \
                    x.stride(0) != T * x.stride(1):
                x = x.contiguous()
            ops.copy2d(x.data_ptr(), ops.dt(x), X[g].data_ptr(), ops.dt(X), B * T, E,
                       x.stride(1), 1, E, 1)
        lg.fwd(lg.kcat([X[0], X[1]], E, E), B * T, W, b, lg.strided(X[2], E), cd)
        ctx.save_for_backward(X, W, b)
        ctx.meta = (cd, v.dtype, p.dtype)
        return X

    @staticmethod
    def backward(ctx, dX):
        X, W, b = ctx.saved_tensors
        cd, vdt, pdt = ctx.meta
        G3, B, T, E = X.shape
        # the incoming gradient is this Function's alone (the stacked X feeds the encoder group
        # only): its first two slots receive out_layer_pv's input gradients in place
        dX = _contig(dX, cd)
        G = Rows(dX[2])
        lg.dgrad(G.op(), G.rows, E, W, lg.table([dX[0], dX[1]], E), cd, kseg=E, beta=1.0)
        # deferred to the end-of-backward group: dX[2] is read by nobody else (the node hands on
        # dX[0] / dX[1] only) and X is this node's saved forward buffer
        lg.wgrad(G.op(), lg.table([X[0], X[1]], E), G.rows, E, W, cd, b, kseg=E, defer=True)
        dv = dX[0] if vdt == cd else _cast_keep_layout(dX[0], vdt)
        dp = dX[1] if pdt == cd else _cast_keep_layout(dX[1], pdt)
        return dv, dp, None, None, None


def stack_joint(v, p, W, b, slots=None) -> torch.Tensor:
    return StackJointFn.apply(v, p, W, b, slots)


class StackTokensFn(Function):
    """The SELF_ATTEN head's token stack (mm_multi_transformers.py:171-178) from the stacked
    cross-attention outputs O6 (S, B, T, E): a (B, T, S, E) buffer filled by S strided copies,
    returned as its seq-first (S, B*T, E) view.  The backward writes dO6 (S, B, T, E) with S
    strided copies — one gradient buffer, no per-slice zero-fill / copy / sum as the autograd of
    S separate selections of O6 would run."""

    @staticmethod
    def forward(ctx, X):
        cd = compute_dtype()
        X = _contig(X, cd)
        S, B, T, E = X.shape
        buf = torch.empty(B, T, S, E, dtype=cd, device=X.device)
        for s in range(S):
            ops.copy2d(X[s].data_ptr(), ops.dt(X), _ptr(buf, s * E), ops.dt(buf), B * T, E, E, 1,
                       S * E, 1)
        ctx.meta = (S, B, T, E, cd)
        return buf.view(B * T, S, E).permute(1, 0, 2)

    @staticmethod
    def backward(ctx, g):
        S, B, T, E, cd = ctx.meta
        gb = g.permute(1, 0, 2)                      # (B*T, S, E) logical
        if gb.dtype != cd or gb.stride(2) != 1 or gb.stride(1) != E or gb.stride(0) != S * E:
            gb = gb.to(cd).contiguous()
        dX = torch.empty(S, B, T, E, dtype=cd, device=g.device)
        for s in range(S):
            ops.copy2d(_ptr(gb, s * E), ops.dt(gb), dX[s].data_ptr(), ops.dt(dX), B * T, E, S * E,
                       1, E, 1)
        return dX


def stack_tokens(X) -> torch.Tensor:
    return StackTokensFn.apply(X)


class LastQueryMHAFn(Function):
    """nn.MultiheadAttention(last, enc, enc) with last = enc[-1:] (the SELF_ATTEN head's final
    attention, mm_multi_transformers.py:186-193: only the last query row is kept): q from the
    last token's rows, packed k|v from all tokens, attention core, out_proj; returns (N, E).
    The backward adds the query path's input gradient into the last token's rows of the key /
    value path's input gradient with a beta = 1 GEMM epilogue — no zero-filled slice gradient
    and no gradient sum."""

    @staticmethod
    def forward(ctx, enc, Win, bin_, Wout, bout, H, drop_p=0.0):
        cd = compute_dtype()
        L, N, E = enc.shape
        X = Rows(enc, cd)                              # rows in enc's memory order
        kv = X.like(2 * E, cd)
        lg.fwd(X.op(), X.rows, Win, bin_, _out(kv, X.perm), cd, E, 2 * E)
        xl = X.t[-1:]
        XL = Rows(xl)
        q = XL.like(E, cd)
        lg.fwd(XL.op(), XL.rows, Win, bin_, _out(q, XL.perm), cd, 0, E)
        o, asaved = attn_forward(q, kv, kv, E, H, 0, 0, E, drop_p=drop_p)
        O = Rows(o)
        y = O.like(E, cd)
        lg.fwd(O.op(), O.rows, Wout, bout, _out(y, O.perm), cd)
        ctx.save_for_backward(X.t, q, kv, o, Win, bin_, Wout, bout)
        ctx.asaved = asaved
        ctx.meta = (cd, enc.dtype, X.perm, XL.perm, O.perm)
        return y[0]

    @staticmethod
    def backward(ctx, gy):
        x, q, kv, o, Win, bin_, Wout, bout = ctx.saved_tensors
        cd, xdt, xperm, xlperm, operm = ctx.meta
        L, N, E = x.shape
        O = Rows(o)
        G = _match(gy.unsqueeze(0), Rows(O.like(E, cd)), cd)          # (1, N, E) in o's order
        do = O.like(E, cd)
        lg.dgrad(G.op(), G.rows, E, Wout, _out(do, O.perm), cd)
        lg.wgrad(G.op(), O.op(), G.rows, E, Wout, cd, bout)
        X = Rows(x)
        dkv = X.like(2 * E, cd)
        dq = Rows(q).like(E, cd)
        attn_backward(ctx.asaved, do, dq, dkv, dkv)
        DKV = Rows(dkv)
        dx = X.like(E, cd)
        lg.dgrad(DKV.op(), DKV.rows, 2 * E, Win, _out(dx, X.perm), cd, E)
        lg.wgrad(DKV.op(), X.op(), DKV.rows, 2 * E, Win, cd, bin_, E)
        DQ = Rows(dq)
        XL = Rows(x[-1:])
        dxl = dx[-1:]
        lg.dgrad(DQ.op(), DQ.rows, E, Win, _out(dxl, XL.perm), cd, beta=1.0)
        lg.wgrad(DQ.op(), XL.op(), DQ.rows, E, Win, cd, bin_)
        if xdt != cd:
            dx = _cast_keep_layout(dx, xdt)
        ctx.asaved = None
        return dx, None, None, None, None, None, None


def attn_drop_rate(modules) -> float:
    """The attention dropout rate of the MultiheadAttention modules one launch serves (their
    `dropout` while training, 0 in eval; modules without the attribute count as 0).  One launch
    takes one mask call and one rate: modules that disagree raise ValueError."""
    rates = {float(m.drop_rate()) if hasattr(m, "drop_rate") else 0.0 for m in modules}
    if len(rates) > 1:
        raise ValueError(f"attention modules of one grouped launch disagree on dropout: "
                         f"{sorted(rates)}")
    p = rates.pop() if rates else 0.0
    return p if p > 0.0 and attn_dropout_rate(p) > 0.0 else 0.0     # below 1 / 512: none


def last_query_mha(enc, mha) -> torch.Tensor:
    return LastQueryMHAFn.apply(enc, mha.in_proj_weight, mha.in_proj_bias, mha.out_proj.weight,
                                mha.out_proj.bias, mha.num_heads, attn_drop_rate([mha]))


# ------------------------------------------------------------------------- encoder group
def encoder_layer_params(layer) -> List[torch.Tensor]:
    """The 12 parameters of one TransformerEncoderLayer (mm_multi_transformers.py:48-70)."""
    a, ff = layer.attention, layer.feed_forward
    return [a.in_proj_weight, a.in_proj_bias, a.out_proj.weight, a.out_proj.bias,
            ff[0].weight, ff[0].bias, ff[len(ff) - 1].weight, ff[len(ff) - 1].bias,
            layer.layer_norm1.weight, layer.layer_norm1.bias,
            layer.layer_norm2.weight, layer.layer_norm2.bias]


class EncoderGroupFn(Function):
    """G post-LN encoder layers (mm_multi_transformers.py:61-70, one per stream, same shapes,
    own weights) on the stacked seq-first input X (G, B, T, E):
        Y_g = LN2(H_g + W2 relu(W1 H_g + b1) + b2),  H_g = LN1(X_g + MHA_g(X_g, X_g, X_g)).
    params: 12 per group (encoder_layer_params).
    batch_axis: the self-attention runs over the B axis of each group (sequences of length B,
    one per t) — MultimodalTransformer_wo_JR feeds its encoders batch-first tensors
    (mm_transformers.py:119-122); the attention core is then one launch per group (a group's
    (B, T) rows are a (seq, batch)-strided layout, the G groups together are not), every GEMM,
    LayerNorm and bias reduction stays one grouped launch.
    kr (meta): the KeyRanges of a (B, T) key padding mask; sequence g B + b of the one attention
    launch uses entry b.  A mask over time has no meaning on the batch axis."""

    @staticmethod
    def forward(ctx, X, meta, *params):
        H, eps1, eps2, batch_axis, kr, drop_p = meta
        if kr is not None and batch_axis:
            raise NotImplementedError("a key padding mask over time with attention over the "
                                      "batch axis")
        cd = compute_dtype()
        X = _contig(X, cd)
        G, B, T, E = X.shape
        R = B * T
        dev = X.device
        P = [params[12 * g:12 * g + 12] for g in range(G)]
        hid = P[0][4].shape[0]
        col = lambda k: [p[k] for p in P]                       # parameter k of every group
        sd = lambda t: lg.strided(t, t.shape[-1], R * t.shape[-1])   # a stacked (G, B, T, F)
        # packed in-projection (3 groups, one launch)
        QKV = torch.empty(G, B, T, 3 * E, dtype=cd, device=dev)
        lg.fwd(sd(X), R, col(0), col(1), sd(QKV), cd)
        if batch_axis:
            # QKV[g] (B, T, 3E) read as seq-first (L = B, N = T): attention over the batch axis
            outs = [attn_forward(QKV[g], QKV[g], QKV[g], E, H, 0, E, 2 * E, drop_p=drop_p)
                    for g in range(G)]
            O = [o for o, _ in outs]                           # G x (B, T, E)
            asaved = [sv for _, sv in outs]
        else:
            sf = QKV.view(G * B, T, 3 * E).permute(1, 0, 2)      # (T, G*B, 3E) seq-first
            # memory (G*B, T, E); with dropout one mask call for the whole launch
            o, asaved = attn_forward(sf, sf, sf, E, H, 0, E, 2 * E, kr=kr, drop_p=drop_p)
            O = o.permute(1, 0, 2)
        A1 = torch.empty(G, B, T, E, dtype=cd, device=dev)
        lg.fwd(lg.table(O, E) if batch_axis else lg.strided(O, E, R * E), R, col(2), col(3),
               sd(A1), cd)
        H1 = torch.empty_like(A1)
        st1 = torch.empty(2, G * R, dtype=torch.float32, device=dev)
        if not ops.layernorm_fwd_grouped(X, A1, [p[8] for p in P], [p[9] for p in P], eps1, H1,
                                         st1[0], st1[1]):
            for g in range(G):
                ops.layernorm_fwd(X[g], E, A1[g], E, P[g][8], P[g][9], eps1, H1[g], E,
                                  st1[0, g * R:], st1[1, g * R:], R, E)
        F1 = torch.empty(G, B, T, hid, dtype=cd, device=dev)
        lg.fwd(sd(H1), R, col(4), col(5), sd(F1), cd, relu=True)
        F2 = torch.empty(G, B, T, E, dtype=cd, device=dev)
        lg.fwd(sd(F1), R, col(6), col(7), sd(F2), cd)
        Y = torch.empty_like(A1)
        st2 = torch.empty(2, G * R, dtype=torch.float32, device=dev)
        if not ops.layernorm_fwd_grouped(H1, F2, [p[10] for p in P], [p[11] for p in P], eps2, Y,
                                         st2[0], st2[1]):
            for g in range(G):
                ops.layernorm_fwd(H1[g], E, F2[g], E, P[g][10], P[g][11], eps2, Y[g], E,
                                  st2[0, g * R:], st2[1, g * R:], R, E)
        ctx.params = params
        ctx.state = (X, QKV, asaved, O, A1, H1, st1, F1, F2, st2)
        ctx.meta = (G, B, T, E, hid, cd, batch_axis)
        return Y

    @staticmethod
    def backward(ctx, dY):
        G, B, T, E, hid, cd, batch_axis = ctx.meta
        X, QKV, asaved, O, A1, H1, st1, F1, F2, st2 = ctx.state
        params = ctx.params
        P = [params[12 * g:12 * g + 12] for g in range(G)]
        R = B * T
        dev = X.device
        col = lambda k: [p[k] for p in P]                       # parameter k of every group
        sd = lambda t: lg.strided(t, t.shape[-1], R * t.shape[-1])   # a stacked (G, B, T, F)
        dY = _contig(dY, cd)

        def ln_bwd(x, r, dy, st, gamma, beta, dx, bias=None):
            """LayerNorm backward per group; with `bias` (the biases of the linears whose
            outputs r entered the residual sums) their gradients — the column sums of dx — are
            reduced in the same launch pair.  Returns whether they were.
            The fused bias sum reduces the fp32 dx before it is rounded to the compute dtype;
            the fallback column sum (lg.bias_grad) reads the rounded dx — the same quantity, one
            rounding apart.  The kernels take one accumulate flag for all their outputs, so when
            any of the gradient buffers is missing (a frozen parameter) every output goes to a
            scratch block and the present buffers accumulate it afterwards."""
            fused = bias is not None
            # all G groups in one launch pair when every gradient buffer exists
            gb = [_grad_buffer(t) for t in gamma]
            bb = [_grad_buffer(t) for t in beta]
            sb = [_grad_buffer(t) for t in bias] if fused else []
            if all(t is not None for t in gb + bb + sb) and ops.layernorm_bwd_grouped(
                    x, r, dy, st[0], st[1], gamma, dx, gb, bb, sb if fused else None,
                    True) is not None:
                for g in range(G):
                    _grad_done(gamma[g], beta[g], *([bias[g]] if fused else []))
                return fused
            for g in range(G):
                bufs = [_grad_buffer(gamma[g]), _grad_buffer(beta[g])]
                if fused:
                    bufs.append(_grad_buffer(bias[g]))
                tmp = None
                if any(b is None for b in bufs):
                    tmp = torch.zeros(3, E, dtype=torch.float32, device=dev)
                outs = bufs if tmp is None else [tmp[0], tmp[1], tmp[2]]
                args = (x[g], E, r[g], E, dy[g], E, st[0, g * R:], st[1, g * R:], gamma[g], dx[g],
                        E, outs[0], outs[1])
                done = fused and ops.layernorm_bwd_dsum(
                    *args, outs[2] if tmp is None else tmp[2], tmp is None, R, E) is not None
                if not done:
                    ops.layernorm_bwd(*args, tmp is None, R, E)
                if tmp is not None:
                    for b, t in zip(bufs[:3 if done else 2], tmp):
                        if b is not None:
                            b.add_(t)
                if done:
                    _grad_done(gamma[g], beta[g], bias[g])
                    continue
                _grad_done(gamma[g], beta[g])
                if fused:        # shape not covered by the fused form: this group's bias apart
                    lg.bias_grad(lg.strided(dx[g].view(R, E), E), R, E, [bias[g]])
            return fused

        # LN2: dS2 = d(H1 + F2)
        dS = torch.empty(G, B, T, E, dtype=cd, device=dev)
        b2_done = ln_bwd(H1, F2, dY, st2, [p[10] for p in P], [p[11] for p in P], dS,
                         bias=[p[7] for p in P])
        # FFN (the ReLU mask is fused into the W2 dgrad epilogue)
        dF1 = torch.empty(G, B, T, hid, dtype=cd, device=dev)
        lg.dgrad(sd(dS), R, E, col(6), sd(dF1), cd, aux=F1, ldaux=hid)
        # With hid == E, W1's weight gradient (dF1 and H1 are ready here) goes in the same launch:
        # 2 G entries of 512 x 512 over the B T rows (24 tiles at G = 3: the split-K ping-pong
        # kernel) instead of two 12-tile launches on the 128 x 128 split plan
        merged = _merge_wgrads["on"] and hid == E and 2 * G <= 8 and cd != torch.float32
        # stage B (ops: the end-of-backward group): the weight gradients below are queued, so
        # nothing may write their operands again before the backward pass ends —
        #   W2 (+ W1 merged)  dS, F1 (+ dF1, H1)   dH1 goes to a fresh buffer (c_in = dS) and dO
        #                                          takes that buffer, dead after LN1's backward
        #   W1                dF1, H1              not written again
        #   out_proj          dS1, O               dX goes to a fresh buffer (c_in = dS1)
        #   in_proj           dQKV, X              not written again (X: the saved input)
        # F1, H1, O and X are saved forward buffers that the backward only reads.
        late = wgrad_defer_ok(cd)
        if merged:
            # b2 already summed (by LN2's backward): its entries stay None and W1's bias
            # gradient is still taken inside the launch
            bsw = ([None] * G if b2_done else col(7)) + col(5)
            each = lambda *ts: lg.table([(t, g * R * E) for t in ts for g in range(G)], E)
            if not lg.wgrad(each(dS, dF1), each(F1, H1), R, E, col(6) + col(4), cd, bsw,
                            intact=late, fallback=False):
                if not b2_done:
                    lg.bias_grad(sd(dS), R, E, col(7))
                lg.bias_grad(sd(dF1), R, hid, col(5))
        else:
            lg.wgrad(sd(dS), sd(F1), R, E, col(6), cd, None if b2_done else col(7), intact=late)
        # dH1 = dS2 + dF1 . W1  (in place on dS: beta = 1; stage B: into a fresh buffer, dS is
        # the queued W2 weight gradient's operand)
        dH1 = torch.empty_like(dS) if late else dS
        lg.dgrad(sd(dF1), R, hid, col(4), sd(dH1), cd, beta=1.0, c_in=dS if late else None)
        if not merged:
            lg.wgrad(sd(dF1), sd(H1), R, hid, col(4), cd, col(5), intact=late)
        # LN1: dS1 = d(X + A1)
        dS1 = torch.empty_like(dS)
        bo_done = ln_bwd(X, A1, dH1, st1, [p[8] for p in P], [p[9] for p in P], dS1,
                         bias=[p[3] for p in P])
        # out_proj
        dO = dH1    # reuse: dH1 is dead
        lg.dgrad(sd(dS1), R, E, col(2), sd(dO), cd)
        lg.wgrad(sd(dS1), lg.table(O, E) if batch_axis else lg.strided(O, E, R * E), R, E,
                 col(2), cd, None if bo_done else col(3), intact=late)
        # attention core -> packed dQKV
        dQKV = torch.empty(G, B, T, 3 * E, dtype=cd, device=dev)
        if batch_axis:
            for g in range(G):
                attn_backward(asaved[g], dO[g], dQKV[g], dQKV[g], dQKV[g])
        else:
            dsf = dQKV.view(G * B, T, 3 * E).permute(1, 0, 2)
            attn_backward(asaved, dO.view(G * B, T, E).permute(1, 0, 2), dsf, dsf, dsf)
        # in_proj: dX = dS1 + dQKV . W_in  (in place on dS1; stage B: into a fresh buffer, dS1 is
        # the queued out_proj weight gradient's operand — the returned dX is accumulated into
        # again downstream, StackJointFn)
        dX = torch.empty_like(dS1) if late else dS1
        lg.dgrad(sd(dQKV), R, 3 * E, col(0), sd(dX), cd, beta=1.0, c_in=dS1 if late else None)
        lg.wgrad(sd(dQKV), sd(X), R, 3 * E, col(0), cd, col(1), intact=late)
        ctx.state = None
        return (dX, None) + (None,) * len(params)


def encoder_group(X, layers, num_heads: int, batch_axis: bool = False, kr=None):
    """Apply `layers` (one TransformerEncoderLayer per stream) to the stacked X (attention over
    T, or over B with batch_axis).  kr: the KeyRanges of a (B, T) key padding mask.  Attention
    dropout: the layers' attention modules' rate (attn_drop_rate)."""
    params = [p for layer in layers for p in encoder_layer_params(layer)]
    meta = (num_heads, layers[0].layer_norm1.eps, layers[0].layer_norm2.eps, bool(batch_axis),
            kr, attn_drop_rate([layer.attention for layer in layers]))
    return EncoderGroupFn.apply(X, meta, *params)


# the wo_JR model's two cross-attentions (mm_transformers.py:125-135): (module, query, key/value)
# with module 0 = cross_attention_v, 1 = cross_attention_p, stream 0 = visual, 1 = physiological
CROSS_PAIRS_WO_JR = ((0, 0, 1), (1, 1, 0))


# ------------------------------------------------------------------------- cross attentions
def mha_params(mha) -> List[torch.Tensor]:
    return [mha.in_proj_weight, mha.in_proj_bias, mha.out_proj.weight, mha.out_proj.bias]


# Pairs that apply the same module to the same query stream (CROSS_PAIRS: 0 and 3, 1 and 5,
# 2 and 4) have the same query projection.  It is computed once, the attention kernels read it
# from the first use's rows of QKV (JMT_CA_SHARED_Q=0: every pair projects its own, the launches
# of before), and the two uses' query gradients leave the chip as ONE dQ = dS_i K_i + dS_j K_j
# (JMT_CA_DQ_MERGE=0: one dQ per pair, summed by the K-concatenated GEMMs downstream; bitwise
# the unshared results).
_shared_q = {"on": os.environ.get("JMT_CA_SHARED_Q", "1") != "0",
             "merge": os.environ.get("JMT_CA_DQ_MERGE", "1") != "0"}


def shared_query_table(pairs):
    """qtab[i] = the first pair with pair i's (module, query stream); None without duplicates."""
    first, qtab = {}, []
    for i, (m, q, _) in enumerate(pairs):
        qtab.append(first.setdefault((m, q), i))
    return qtab if any(t != i for i, t in enumerate(qtab)) and len(pairs) <= 8 else None


class CrossAttention6Fn(Function):
    """The six key-is-value cross-attentions of mm_multi_transformers.py:142-167 on the stacked
    encoder outputs Y (3, B, T, E) -> O6 (6, B, T, E) in the reference's concatenation order
    (CROSS_PAIRS).  params: 4 per module (mha_params) for cross_attention_v / _p / _pv.
    kr (meta): the KeyRanges of a (B, T) key padding mask; sequence p B + b uses entry b."""

    @staticmethod
    def forward(ctx, Y, meta, *params):
        H, pairs, kr, drop_p = meta
        cd = compute_dtype()
        Y = _contig(Y, cd)
        S, B, T, E = Y.shape
        R = B * T
        dev = Y.device
        M = [params[4 * m:4 * m + 4] for m in range(len(params) // 4)]
        NP = len(pairs)
        QKV = torch.empty(NP, B, T, 3 * E, dtype=cd, device=dev)
        in_w = [M[m][0] for m, _, _ in pairs]
        in_b = [M[m][1] for m, _, _ in pairs]
        sf = QKV.view(NP * B, T, 3 * E).permute(1, 0, 2)
        qtab = shared_query_table(pairs) if _shared_q["on"] else None
        if qtab is not None:
            # the backward's buffers as this node builds them: dQKV laid out like QKV, dO
            # batch-major (NP * B, T, E) with row stride E
            oq, ok, ov = (_operand(sf, c, cd) for c in (0, E, 2 * E))
            od = AttnOperand(True, E)
            # (with dropout the plan is "mh" or "gemm", never shared: every pair projects its own)
            if not attn_plan(cd, NP * B, H, T, T, E, oq, ok, ov, od, od, oq, ok, ov,
                             kr=kr is not None, drop=drop_p > 0.0).shared_q:
                qtab = None
        # queries and packed key/values, one launch each.  Shared queries: the projection of the
        # first use only (the q columns of the other uses' rows of QKV stay unused); otherwise
        # each module's query projection is evaluated for both of its calls, as the reference does
        # The two launches read Y and write disjoint columns of QKV: one grouped launch where
        # lg.group16_scope takes them
        qkv = lg.strided(QKV, 3 * E, R * 3 * E)
        with lg.group16_scope():
            if qtab is not None:
                fu = [i for i, t in enumerate(qtab) if t == i]
                lg.fwd(lg.table([Y[pairs[i][1]] for i in fu], E), R, [in_w[i] for i in fu],
                       [in_b[i] for i in fu], lg.blocks([QKV[i] for i in fu], 3 * E), cd, 0, E)
            else:
                lg.fwd(lg.table([Y[q] for _, q, _ in pairs], E), R, in_w, in_b, qkv, cd, 0, E)
            lg.fwd(lg.table([Y[k] for _, _, k in pairs], E), R, in_w, in_b,
                   lg.strided((QKV, E), 3 * E, R * 3 * E), cd, E, 2 * E)
        qshare = (B, qtab) if qtab is not None else None
        o, asaved = attn_forward(sf, sf, sf, E, H, 0, E, 2 * E, qshare=qshare, kr=kr,
                                 drop_p=drop_p)
        O = o.permute(1, 0, 2)                                   # (NP*B, T, E) memory
        O6 = torch.empty(NP, B, T, E, dtype=cd, device=dev)
        lg.fwd(lg.strided(O, E, R * E), R, [M[m][2] for m, _, _ in pairs],
               [M[m][3] for m, _, _ in pairs], lg.strided(O6, E, R * E), cd)
        ctx.params = params
        ctx.state = (Y, QKV, asaved, O)
        ctx.meta = (pairs, S, B, T, E, cd, qtab)
        return O6

    @staticmethod
    def backward(ctx, dO6):
        pairs, S, B, T, E, cd, qtab = ctx.meta
        Y, QKV, asaved, O = ctx.state
        params = ctx.params
        M = [params[4 * m:4 * m + 4] for m in range(len(params) // 4)]
        NP = len(pairs)
        R = B * T
        dev = Y.device
        dO6 = _contig(dO6, cd)
        # stage B (ops: the end-of-backward group): the weight gradients are queued and their
        # operands must stay intact (lg.wgrad keeps the tensors, from the operands).  dO6 is this node's incoming gradient (ConcatLinearFn's fresh dX, or
        # StackTokensFn's on the SELF_ATTEN head path: autograd has summed into it before this
        # node runs and nobody holds it afterwards), O and Y are saved forward buffers, and dQKV
        # is only read after the attention backward has written it.
        late = wgrad_defer_ok(cd)
        in_w = [M[m][0] for m, _, _ in pairs]
        in_b = [M[m][1] for m, _, _ in pairs]
        out_w = [M[m][2] for m, _, _ in pairs]
        out_b = [M[m][3] for m, _, _ in pairs]
        sel = lambda ps, idx: [ps[i] for i in idx]
        blk = lambda t, i: (t, i * R * E)       # pair / stream i's (B, T, E) block of t
        # launches of the batched wgrads: each launch holds distinct modules
        halves, seen = [[]], [set()]
        for i, (m, _, _) in enumerate(pairs):
            if m in seen[-1]:
                halves.append([])
                seen.append(set())
            halves[-1].append(i)
            seen[-1].add(m)
        # out_proj: input gradient
        dO = torch.empty(NP, B, T, E, dtype=cd, device=dev)
        lg.dgrad(lg.strided(dO6, E, R * E), R, E, out_w, lg.strided(dO, E, R * E), cd)

        # the two uses of each module (one per half) as the K-segments of one batch entry:
        # h0[u] and h1[u] are the pairs of module ms[u]
        kcat = (len(halves) == 2 and len(halves[0]) == len(halves[1]) and
                sorted(pairs[i][0] for i in halves[0]) ==
                sorted(pairs[i][0] for i in halves[1]) and
                _kcat_ok(R, 2 * len(halves[0]), cd))
        if kcat:
            h0 = list(halves[0])
            h1 = [next(j for j in halves[1] if pairs[j][0] == pairs[i][0]) for i in h0]
            uses = list(zip(h0, h1))
        # one dQ per shared query (in the first use's q columns of dQKV; the second use's stay
        # unwritten): when every query is used exactly twice and, for the K-concatenated weight
        # gradients, the two uses of every module are the two uses of one query
        merge = (qtab is not None and _shared_q["merge"] and
                 all(qtab.count(i) == 2 for i in set(qtab)) and
                 (not kcat or all(qtab[i] == i and qtab[j] == i for i, j in zip(h0, h1))))
        # out_proj weight / bias gradients (the launches take offsets into dO6 / O; only the
        # column-sum fallback needs views)
        kw = dict(intact=late, fallback=False)
        if kcat:
            if not lg.wgrad(lg.ksegs([[blk(dO6, i), blk(dO6, j)] for i, j in uses], E, R),
                            lg.ksegs([[blk(O, i), blk(O, j)] for i, j in uses], E, R), R, E,
                            sel(out_w, h0), cd, sel(out_b, h0), **kw):
                lg.bias_grad(lg.ksegs([[dO6[i], dO6[j]] for i, j in uses], E, R), R, E,
                             sel(out_b, h0))
        else:
            rest = [h for h in halves if not lg.wgrad(
                lg.table([blk(dO6, i) for i in h], E), lg.table([blk(O, i) for i in h], E), R, E,
                sel(out_w, h), cd, sel(out_b, h), **kw)]
            for h in rest:
                lg.bias_grad(lg.table([dO6[i] for i in h], E), R, E, sel(out_b, h))
        # attention core -> packed dQKV (NP, B, T, 3E)
        dQKV = torch.empty(NP, B, T, 3 * E, dtype=cd, device=dev)
        dsf = dQKV.view(NP * B, T, 3 * E).permute(1, 0, 2)
        attn_backward(asaved, dO.view(NP * B, T, E).permute(1, 0, 2), dsf, dsf, dsf,
                      qshare=(B, qtab) if qtab is not None else None, merge_dq=merge)

        # in_proj weight gradients: query rows [0, E) from the query stream, key/value rows
        # [E, 3E) from the key stream
        dq = lambda i, off=0: (dQKV, i * R * 3 * E + off)     # pair i's packed gradient rows
        Yc = lambda i, c: blk(Y, pairs[i][c])                 # its query (1) / key (2) stream
        # the query-row and key / value-row launches sit next to each other: one grouped launch
        # (their rows of W.grad / b.grad are disjoint).  They share one bias: the key / value
        # launch sums it only if the query launch did, else the whole rows go through the column
        # sum afterwards
        if kcat:
            ws, bs = sel(in_w, h0), sel(in_b, h0)
            seg = lambda off: lg.ksegs([[dq(i, off), dq(j, off)] for i, j in uses], 3 * E, R)
            yseg = lambda c: lg.ksegs([[Yc(i, c), Yc(j, c)] for i, j in uses], E, R)
            with wgrad_scope(cd):
                if merge:
                    # the merged dQ against the query stream: a plain problem over K = B T
                    fq = lg.wgrad(lg.table([dq(i) for i in h0], 3 * E),
                                  lg.table([Yc(i, 1) for i in h0], E), R, E, ws, cd, bs, **kw)
                else:
                    fq = lg.wgrad(seg(0), yseg(1), R, E, ws, cd, bs, **kw)
                fkv = lg.wgrad(seg(E), yseg(2), R, 2 * E, ws, cd, bs if fq else None, E, **kw)
            if not (fq and fkv):
                assert not fq, "query-row bias sums fused without the key / value rows"
                for b, (i, j) in zip(bs, uses):
                    lg.bias_grad(lg.strided(dQKV[i], 3 * E), R, 3 * E, [b])
                    if merge:       # the second use has key / value columns only
                        lg.bias_grad(lg.strided(dQKV[j].view(R, 3 * E)[:, E:], 3 * E), R,
                                     2 * E, [b], E)
                    else:
                        lg.bias_grad(lg.strided(dQKV[j], 3 * E), R, 3 * E, [b])
        else:
            rest = []
            for h in halves:
                ws, bs = sel(in_w, h), sel(in_b, h)
                # with a merged dQ, query rows from the pairs that hold one only
                hq = [i for i in h if qtab[i] == i] if merge else h
                with wgrad_scope(cd):
                    fq = not hq or lg.wgrad(lg.table([dq(i) for i in hq], 3 * E),
                                            lg.table([Yc(i, 1) for i in hq], E), R, E,
                                            sel(in_w, hq), cd, sel(in_b, hq), **kw)
                    fkv = lg.wgrad(lg.table([dq(i, E) for i in h], 3 * E),
                                   lg.table([Yc(i, 2) for i in h], E), R, 2 * E, ws, cd,
                                   bs if fq else None, E, **kw)
                if fq and fkv:
                    continue
                assert not (fq and hq), "query-row bias sums fused without the key / value rows"
                if not merge:
                    rest.append(h)
                    continue
                for i, b in zip(h, bs):
                    c0 = 0 if i in hq else E
                    lg.bias_grad(lg.strided(dQKV[i].view(R, 3 * E)[:, c0:], 3 * E), R, 3 * E - c0,
                                 [b], c0)
            for h in rest:
                lg.bias_grad(lg.table([dQKV[i] for i in h], 3 * E), R, 3 * E, sel(in_b, h))
        # stream gradients: every use of stream s (as a query: rows [0,E) of W_in; as a key /
        # value: rows [E,2E) and [2E,3E)) is one K-segment of ONE dgrad GEMM (K = nseg * E); a
        # merged dQ is one segment for both of its uses
        dY = torch.zeros(S, B, T, E, dtype=cd, device=dev) if any(
            not any(q == s or k == s for _, q, k in pairs) for s in range(S)) else \
            torch.empty(S, B, T, E, dtype=cd, device=dev)
        segs = []
        for s in range(S):
            dys, wts = [], []
            for i, (m, q, k) in enumerate(pairs):
                Wc = weight_as(M[m][0], cd)
                if q == s and not (merge and qtab[i] != i):
                    dys.append((dQKV, i * R * 3 * E))
                    wts.append((Wc, 0))
                if k == s:
                    dys += [(dQKV, i * R * 3 * E + E), (dQKV, i * R * 3 * E + 2 * E)]
                    wts += [(Wc, E * E), (Wc, 2 * E * E)]
            segs.append((dys, wts))
        # one launch per stream (600 128x128 tiles each, under one round of the chip's resident
        # slots); the three write different dY[s] — one grouped launch where lg.group16_scope
        # takes them, two rounds of the persistent grid instead of three
        with lg.group16_scope():
            for s, (dys, wts) in enumerate(segs):
                if dys:     # (lg.dgrad: at most 8 K-segments per launch)
                    lg.dgrad(lg.kcat(dys, 3 * E, E), R, E, lg.kcat(wts, E, E),
                             lg.strided(dY[s], E), cd)
        ctx.state = None
        return (dY, None) + (None,) * len(params)


def cross_attention6(Y, modules, num_heads: int, pairs=CROSS_PAIRS, kr=None):
    params = [p for mod in modules for p in mha_params(mod)]
    return CrossAttention6Fn.apply(Y, (num_heads, pairs, kr, attn_drop_rate(modules)), *params)


# ------------------------------------------------------------------------- concat head
class ConcatLinearFn(Function):
    """y = cat(X[0], ..., X[S-1], dim=-1) . W^T + b for a stacked X (S, B, T, E): the FC head's
    torch.cat + out_layer1 (mm_multi_transformers.py:201-211) as one K-concatenated GEMM; the
    backward writes the stacked dX in one batched dgrad launch and W.grad in one batched wgrad."""

    @staticmethod
    def forward(ctx, X, W, b):
        cd = compute_dtype()
        X = _contig(X, cd)
        S, B, T, E = X.shape
        R = B * T
        N = W.shape[0]
        assert W.shape[1] == S * E
        dev = X.device
        y = torch.empty(B, T, N, dtype=cd, device=dev)
        lg.fwd(lg.kcat([X[s] for s in range(S)], E, E), R, W, b, lg.strided(y, N), cd)
        ctx.save_for_backward(X, W, b)
        ctx.meta = cd
        return y

    @staticmethod
    def backward(ctx, dy):
        X, W, b = ctx.saved_tensors
        cd = ctx.meta
        S, B, T, E = X.shape
        R = B * T
        N = W.shape[0]
        dev = X.device
        dy = _contig(dy, cd)
        dX = torch.empty_like(X)
        lg.dgrad(lg.strided(dy, N), R, N, W, lg.strided(dX, E, R * E), cd, kseg=E)
        # the S K-segments share dY: segment 0 also takes its row sums (the bias grad).
        # Stage B (ops: the end-of-backward group): dy is this node's incoming gradient
        # (autograd has summed the regressors' into it before this node runs) and X its
        # saved input; neither is written again
        lg.wgrad(lg.strided(dy, N), lg.strided(X, E, R * E), R, N, W, cd, b, kseg=E,
                 intact=True)
        return dX, None, None


def concat_linear(X, W, b):
    return ConcatLinearFn.apply(X, W, b)
