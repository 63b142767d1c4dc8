"""Autograd functions of the JMT hot path.  Forward and backward of every op are launches of
libjmt_hip.so kernels (jmt/ops.py); torch supplies device memory, streams and the autograd tape.

Layout conventions
  * Activations are (rows, features) with the feature axis contiguous.  A logical tensor whose
    leading axes are a permutation of a dense buffer (the reference's permute(1,0,2) between
    (B,T,E) and seq-first (T,B,E), mm_multi_transformers.py:127-129) is processed in memory order
    and results are returned with the same permutation: permutes are free.
  * Parameters stay fp32 nn.Parameters (state_dict compatible).  In 16-bit compute mode each
    weight is read through a cached bf16/f16 shadow (re-cast only when the parameter changes).
  * Parameter gradients are written straight into `param.grad` by the wgrad GEMM / reduction
    kernels (beta=1 accumulate), so weights used several times (cross_attention_v is called
    twice, mm_multi_transformers.py:142-167) and slices of the packed in_proj weight need no
    autograd adds.
"""
from __future__ import annotations

import collections
import contextlib

import math
import os
from typing import NamedTuple, Optional

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import linear_gemm as lg
from . import ops
from . import streams
from ._lib import F32, JMTError

# ------------------------------------------------------------------------- precision policy
_policy = {"dtype": None}


def set_compute_dtype(dtype: Optional[torch.dtype]):
    """None = auto (16-bit under torch.autocast, fp32 otherwise); or force fp32 / bf16 / fp16."""
    assert dtype in (None, torch.float32, torch.bfloat16, torch.float16)
    _policy["dtype"] = dtype


def compute_dtype() -> torch.dtype:
    if _policy["dtype"] is not None:
        return _policy["dtype"]
    if torch.is_autocast_enabled("cuda"):
        return torch.get_autocast_dtype("cuda")
    return torch.float32


class compute_mode:
    """`with compute_mode(torch.bfloat16): ...`"""

    def __init__(self, dtype):
        self.dtype = dtype

    def __enter__(self):
        self.prev = _policy["dtype"]
        _policy["dtype"] = self.dtype
        return self

    def __exit__(self, *a):
        _policy["dtype"] = self.prev


def _vec(dtype: torch.dtype) -> int:
    return 4 if dtype == torch.float32 else 8


# ------------------------------------------------------------------------- weight shadows
def weight_as(w: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """fp32 parameter -> contiguous compute-dtype copy.

    * Parameters owned by FusedSGD with a shadow of this dtype read that shadow (the SGD kernel
      rewrites it in the same pass as the fp32 weight, without bumping `_version`).  An in-place
      write from anywhere else (load_state_dict, copy_, ...) bumps `_version`: the shadow is then
      re-cast IN PLACE, so the optimizer keeps updating the buffer the forward reads.
    * Parameters owned by FusedSGD without a matching shadow are never cached: the fused step
      changes them without a version bump, so a cached cast would freeze them.  (A captured
      hipGraph then replays the cast every step.)
    * Anything else is cached on the parameter and re-cast when its version / storage changes."""
    if w.dtype == dtype:
        return w if w.is_contiguous() else w.contiguous()
    fused = getattr(w, "_jmt_fused", None)
    if fused is not None:
        if fused[0] is not None and fused[0].dtype == dtype:
            if fused[1] != w._version or fused[2] != w.data_ptr():
                ops.cast(w.detach(), dtype, out=fused[0])
                w._jmt_fused = (fused[0], w._version, w.data_ptr())
            return fused[0]
        return ops.cast(w.detach(), dtype)
    ent = getattr(w, "_jmt_shadow", None)
    if ent is not None and ent[0] == w._version and ent[1] == dtype and ent[2] == w.data_ptr():
        return ent[3]
    t = ops.cast(w.detach(), dtype)
    w._jmt_shadow = (w._version, dtype, w.data_ptr(), t)
    return t


def register_shadow(w: torch.Tensor, shadow: Optional[torch.Tensor]):
    """Used by the fused optimizer, which rewrites `shadow` (or nothing: None) in the same kernel
    as `w`: from now on `w` changes without a version bump (see weight_as)."""
    w._jmt_fused = (shadow, w._version, w.data_ptr())
    w._jmt_shadow = None


# Set by jmt.dist.GradBucketer: called with the parameters whose gradient writes have just been
# enqueued on the current stream (the last write of a parameter makes its bucket ready).
_grad_hook = None


def _grad_done(*ps) -> None:
    if _grad_hook is not None:
        _grad_hook([p for p in ps if p is not None and p.requires_grad])


# Bumped by every in-place parameter-gradient write (_grad_buffer: every HIP writer asks for its
# buffer there): jmt.optim.FusedSGD skips its zero fill while nothing has written a gradient since
# its last step zeroed them (jmt_sgd_step_zero).
_grad_gen = [0]


def _grad_buffer(p: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    if p is None or not p.requires_grad:
        return None
    _grad_gen[0] += 1
    streams.join_after_backward()
    if p.grad is None:
        p.grad = torch.zeros_like(p, memory_format=torch.contiguous_format)
    return p.grad


# ------------------------------------------------------------------------- row layouts
class Rows:
    """A logical tensor (..., F) seen as `rows` rows of F contiguous features at row stride `ld`,
    in memory order (a permutation `perm` of the leading axes)."""

    __slots__ = ("t", "shape", "perm", "rows", "ld", "F")

    def __init__(self, x: torch.Tensor, dtype: Optional[torch.dtype] = None):
        if dtype is not None and x.dtype != dtype:
            x = _cast_keep_layout(x, dtype)
        if x.stride(-1) != 1:
            x = x.contiguous()
        nd = x.dim()
        lead = list(range(nd - 1))
        perm = sorted(lead, key=lambda d: (-x.stride(d), d))
        dims = [d for d in perm if x.shape[d] != 1]
        ok = all(x.stride(a) == x.stride(b) * x.shape[b] for a, b in zip(dims[:-1], dims[1:]))
        ld = x.stride(dims[-1]) if dims else max(x.shape[-1], 1)
        # (a column vector F == 1 with ld == 1 is a dense vector: keep its row order)
        F = x.shape[-1]
        v = _vec(x.dtype)
        bad_layout = not ok or ld < F
        if bad_layout or (ld % v and F > 1) or x.data_ptr() % 16:
            # re-pack: rows in memory order `keep` (the existing order when the layout is
            # row-regular — other operands of the same GEMMs share it — else the logical one),
            # row stride padded to the 16-B vector (narrow outputs such as Linear(64, 2))
            keep = lead if bad_layout else perm
            Fp = F if (F <= 1 or F % v == 0) else -(-F // v) * v
            y = torch.empty([x.shape[d] for d in keep] + [Fp], dtype=x.dtype, device=x.device)
            if Fp != F:
                y = y[..., :F]
            inv = [0] * len(keep)
            for i, d in enumerate(keep):
                inv[d] = i
            y = y.permute(*inv, nd - 1)
            y.copy_(x)
            x = y
            perm = keep
            ld = max(Fp, 1)
            dims = [d for d in perm if x.shape[d] != 1]
        self.t = x
        self.shape = tuple(x.shape)
        self.perm = perm
        r = 1
        for d in lead:
            r *= x.shape[d]
        self.rows = r
        self.ld = ld
        self.F = x.shape[-1]

    def like(self, F2: int, dtype: torch.dtype, pad_to: int = 1) -> torch.Tensor:
        """New tensor, same logical leading shape and axis order, last dim F2 (row stride padded
        to a multiple of `pad_to`)."""
        Fm = -(-F2 // pad_to) * pad_to
        msizes = [self.shape[d] for d in self.perm] + [Fm]
        y = torch.empty(msizes, dtype=dtype, device=self.t.device)
        if Fm != F2:
            y = y[..., :F2]
        inv = [0] * len(self.perm)
        for i, d in enumerate(self.perm):
            inv[d] = i
        return y.permute(*inv, len(self.perm))

    def op(self) -> "lg.Operand":
        """The rows as one GEMM operand."""
        return lg.strided(self.t, self.ld)

    def same_rows(self, other: "Rows") -> bool:
        return self.perm == other.perm and self.shape[:-1] == other.shape[:-1]


def _cast_keep_layout(x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    if x.stride(-1) == 1 and x.is_contiguous():
        return ops.cast(x, dtype)
    L = Rows(x)
    y = L.like(L.F, dtype)
    ops.copy2d(L.t.data_ptr(), ops.dt(L.t), y.data_ptr(), ops.dt(y), L.rows, L.F, L.ld, 1,
               _ld(y, L.perm), 1)
    return y


def _ld(y: torch.Tensor, perm) -> int:
    dims = [d for d in perm if y.shape[d] != 1]
    return y.stride(dims[-1]) if dims else max(y.shape[-1], 1)


def _out(y: torch.Tensor, perm) -> "lg.Operand":
    """A tensor made by Rows.like as one GEMM operand."""
    return lg.strided(y, _ld(y, perm))


def _ptr(t: torch.Tensor, elem_off: int = 0) -> int:
    return t.data_ptr() + elem_off * t.element_size()


def _match(g: torch.Tensor, L: Rows, dtype: torch.dtype) -> Rows:
    """Bring an incoming gradient to layout L and compute dtype."""
    G = Rows(g, dtype)
    if G.same_rows(L):
        return G
    y = L.like(L.F if g.shape[-1] == L.F else g.shape[-1], dtype)
    y.copy_(g)   # rare: autograd handed us a differently laid-out gradient
    return Rows(y)


def _dc(d: torch.dtype) -> int:
    return ops.dt(d)


# ------------------------------------------------------------------------- weight-gradient queue
def wgrad_group_ok() -> bool:
    """Whether weight-gradient launches may be queued and flushed grouped (ops.wgrad_scope /
    defer): not under a GradBucketer, whose buckets complete in the profiled launch order."""
    return _grad_hook is None and ops.wgrad_group_enabled()


def wgrad_defer_ok(cd) -> bool:
    """Whether a weight gradient of compute dtype `cd` whose operands stay intact may be held
    until the end of the backward pass (ops: stage B, defer="late"): where grouping is allowed
    and the grouped launch takes the operands (16-bit), unless JMT_WGRAD_DEFER=0."""
    return wgrad_group_ok() and cd != torch.float32 and ops.wgrad_defer_mode() != "off"


def wgrad_scope(cd=torch.float32):
    """ops.wgrad_scope() where grouping is allowed (held for the end-of-backward flush where
    wgrad_defer_ok(cd)), else a no-op context."""
    return ops.wgrad_scope(defer=wgrad_defer_ok(cd)) if wgrad_group_ok() else \
        contextlib.nullcontext()


# ------------------------------------------------------------------------- preallocated outputs
class Into:
    """A preallocated output (`out=` of linear / l2_normalize) handed to a Function as a plain
    Python object: autograd does not see it as an input, so the result is an ordinary fresh output
    that lives in the caller's buffer — no in-place bookkeeping, and no earlier value of the
    buffer is read by anyone.  The producers save their inputs, never their outputs, so a buffer
    that several producers fill slot by slot (grouped.JointSlots) invalidates no saved tensor."""
    __slots__ = ("t",)

    def __init__(self, t: torch.Tensor):
        self.t = t


def _into(out: Optional[Into], L: Rows, F2: int, dtype: torch.dtype, who: str) -> torch.Tensor:
    """The tensor of `out` after checking that it is what L.like(F2, dtype) would allocate for
    rows in their logical order: same shape and dtype, contiguous, 16-B aligned; else L.like."""
    if out is None:
        return L.like(F2, dtype)
    y = out.t
    if (list(L.perm) != sorted(L.perm) or tuple(y.shape) != L.shape[:-1] + (F2,) or
            y.dtype != dtype or y.device != L.t.device or not y.is_contiguous() or
            y.data_ptr() % 16 or (F2 > 1 and F2 % _vec(dtype))):
        raise JMTError(f"{who}: out= must be a contiguous, 16-B aligned {dtype} tensor of shape "
                       f"{L.shape[:-1] + (F2,)} for an input whose rows are in logical order")
    return y


# ------------------------------------------------------------------------- Linear
class LinearFn(Function):
    """y = cat(xs, -1) @ W[r0:r0+n]^T + b[r0:r0+n]

    nn.Linear (fc_layer.py:6-12, two_transformers.py:56, mm_multi_transformers.py:99,102,
    mm_transformers.py:117) and the packed in_proj slices / out_proj of nn.MultiheadAttention.
    Several `xs` are K-concatenated inside the GEMM without a copy (the torch.cat of
    mm_multi_transformers.py:120-124, 201-211; mm_transformers.py:140-144; FeatureConcatFC)."""

    @staticmethod
    def forward(ctx, W, b, r0, n, out_dtype, out, *xs):
        cd = compute_dtype()
        lay = [Rows(x, cd) for x in xs]
        L0 = lay[0]
        for l in lay[1:]:
            if not l.same_rows(L0) or l.ld != L0.ld or l.F != L0.F:
                raise RuntimeError("LinearFn: concatenated inputs must share one row layout")
        kseg = L0.F
        if len(lay) > 1 and kseg % (32 if cd == torch.float32 else 64):
            raise RuntimeError("LinearFn: concat segment width must be a multiple of 64")
        odt = out_dtype if out_dtype is not None else cd
        y = _into(out, L0, n, odt, "linear")
        xin = [l.t for l in lay]
        lg.fwd(lg.kcat(xin, L0.ld, kseg), L0.rows, W, b, _out(y, L0.perm), cd, r0, n)
        ctx.save_for_backward(W, b, *xin)
        ctx.meta = (r0, n, cd, L0, kseg, [x.dtype for x in xs])
        return y

    @staticmethod
    def backward(ctx, gy):
        W, b = ctx.saved_tensors[:2]
        xin = ctx.saved_tensors[2:]
        r0, n, cd, L0, kseg, in_dtypes = ctx.meta
        Gy = _match(gy, Rows(L0.like(n, cd)), cd)
        nseg = len(xin)
        dxs = [None] * nseg
        need = [ctx.needs_input_grad[6 + i] for i in range(nseg)]
        if any(need):
            outs = [L0.like(kseg, cd) for _ in range(nseg)]
            lg.dgrad(Gy.op(), Gy.rows, n, W, lg.table(outs, _ld(outs[0], L0.perm)), cd, r0, kseg)
            for i in range(nseg):
                if need[i]:
                    dxs[i] = outs[i] if in_dtypes[i] == cd else _cast_keep_layout(outs[i],
                                                                                  in_dtypes[i])
        # no input gradient: nothing runs behind this node that could write gy or the saved
        # inputs, so the launch may join the end-of-backward group
        lg.wgrad(Gy.op(), lg.table(xin, L0.ld), Gy.rows, n, W, cd, b, r0, kseg,
                 defer=not any(need))
        return (None, None, None, None, None, None, *dxs)


def linear(xs, W, b=None, r0=0, n=None, out_dtype=None, out=None):
    """out: a preallocated tensor the GEMM writes (the layout the call would allocate itself)."""
    if isinstance(xs, torch.Tensor):
        xs = (xs,)
    if n is None:
        n = W.shape[0]
    return LinearFn.apply(W, b, r0, n, out_dtype, Into(out) if out is not None else None, *xs)


# ------------------------------------------------------------------------- regressor dropout
# The mask of the regressors' dropout (v_dropout / a_dropout) is a function of a per-device state
# block {seed_lo, seed_hi, call, stream} and the element's (memory row, column) — csrc/dropout.h,
# DESIGN.md §4.  A forward takes a copy of the block and advances `call` on the device
# (ops.dropout_next), its backward regenerates the mask from that copy: nothing is stored per
# element, and a replayed hipGraph draws a new mask per replay.
_drop_state = {}


def _u32(v: int) -> int:
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= (1 << 31) else v     # the uint32 word as an int32 value


def _drop_device(device=None) -> torch.device:
    d = torch.device("cuda" if device is None else device)
    return torch.device("cuda", torch.cuda.current_device()) if d.index is None else d


def _default_stream_id() -> int:
    import torch.distributed as dist
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


def _drop_block(device) -> torch.Tensor:
    dev = _drop_device(device)
    st = _drop_state.get(dev)
    if st is None:
        seed = torch.initial_seed()
        st = torch.tensor([_u32(seed), _u32(seed >> 32), 0, _u32(_default_stream_id())],
                          dtype=torch.int32, device=dev)
        _drop_state[dev] = st
    return st


def set_dropout_state(seed: int, call: int = 0, stream: Optional[int] = None, device=None):
    """Set the dropout state block of `device` (default: the current one): the 64-bit seed, the
    number of masks drawn so far and the stream id (default: the distributed rank, 0 without
    one).  Restoring what dropout_state() returned resumes the mask sequence of a checkpoint.
    Off the step: copies to the device; the block keeps its address (captured graphs read it)."""
    if stream is None:
        stream = _default_stream_id()
    st = _drop_block(device)
    st.copy_(torch.tensor([_u32(seed), _u32(seed >> 32), _u32(call), _u32(stream)],
                          dtype=torch.int32))


def dropout_state(device=None) -> dict:
    """{"seed", "call", "stream"} of `device`'s dropout state block (synchronises the host)."""
    w = [int(v) & 0xFFFFFFFF for v in _drop_block(device).cpu().tolist()]
    return {"seed": w[0] | (w[1] << 32), "call": w[2], "stream": w[3]}


def _check_rate(p) -> float:
    p = float(p or 0.0)
    if not 0.0 <= p < 1.0:
        raise JMTError(f"dropout rate {p} outside [0, 1)")
    return p


# ------------------------------------------------------------------------- MLP
class MLPFn(Function):
    """y = drop_p(relu(x W1^T + b1)) W2^T + b2, ReLU fused into the first GEMM's epilogue and its
    backward mask fused into the second GEMM's dgrad epilogue.  The transformer feed-forward
    (mm_multi_transformers.py:52-56, p = 0), one V / A regressor (two_transformers.py:104-114)
    and the pretrainer's (:131-162).  p > 0: the counter-based mask (csrc/dropout.h) is applied
    in place to h after the ReLU GEMM and to dh after the masked dgrad (h~ > 0 <=> h > 0 and
    kept, so the dgrad's mask operand stays right); the W2 gradients read h~."""

    @staticmethod
    def forward(ctx, W1, b1, W2, b2, out_dtype, x, p=0.0):
        cd = compute_dtype()
        L = Rows(x, cd)
        hid, nout = W1.shape[0], W2.shape[0]
        h = L.like(hid, cd)
        ldh = _ld(h, L.perm)
        lg.fwd(L.op(), L.rows, W1, b1, lg.strided(h, ldh), cd, relu=True)
        ctr = None
        if p > 0.0:
            ctr = ops.dropout_next(_drop_block(h.device))
            ops.dropout(h, ldh, h, ldh, L.rows, hid, hid, p, p, ctr)
        odt = out_dtype if out_dtype is not None else cd
        y = L.like(nout, odt)
        lg.fwd(lg.strided(h, ldh), L.rows, W2, b2, _out(y, L.perm), cd)
        ctx.save_for_backward(W1, b1, W2, b2, L.t, h, ctr)
        ctx.meta = (cd, L, x.dtype, odt, p)
        return y

    @staticmethod
    def backward(ctx, gy):
        W1, b1, W2, b2, xin, h, ctr = ctx.saved_tensors
        cd, L, xdt, odt, p = ctx.meta
        hid, nout = W1.shape[0], W2.shape[0]
        Gy = _match(gy, Rows(L.like(nout, cd)), cd)
        H = Rows(h)
        dh = L.like(hid, cd)
        ldh = _ld(dh, L.perm)
        lg.dgrad(Gy.op(), Gy.rows, nout, W2, lg.strided(dh, ldh), cd, aux=h, ldaux=H.ld)
        if ctr is not None:
            ops.dropout(dh, ldh, dh, ldh, L.rows, hid, hid, p, p, ctr)
        if odt == torch.float32 and cd != torch.float32 and nout <= 16:
            # fp32 output (the V/A regressors' last layer, two_transformers.py:104-114): its
            # weight / bias gradients are sums over all rows of the fp32 loss gradient, which
            # nearly cancel (sum_i dL/dx_i = n c0 for the CCC): summing a 16-bit rounded copy
            # would cost up to ~20 % relative error, so they are reduced from fp32 dY and an
            # fp32 copy of the (small) hidden activations with the exact-f32 MFMA GEMM.
            G = _match(gy, Rows(L.like(nout, torch.float32)), torch.float32)
            hx, dt = Rows(_cast_keep_layout(h, torch.float32)), torch.float32
        else:
            G, hx, dt = Gy, H, cd
        lg.wgrad(G.op(), hx.op(), G.rows, nout, W2, dt)
        lg.bias_grad(G.op(), G.rows, nout, [b2])
        Gh = Rows(dh)
        dx = None
        if ctx.needs_input_grad[5]:
            dx = L.like(L.F, cd)
            lg.dgrad(Gh.op(), Gh.rows, hid, W1, _out(dx, L.perm), cd)
            if xdt != cd:
                dx = _cast_keep_layout(dx, xdt)
        lg.wgrad(Gh.op(), lg.strided(xin, L.ld), Gh.rows, hid, W1, cd, b1)
        return None, None, None, None, None, dx, None


def mlp(x, W1, b1, W2, b2, out_dtype=None, p=0.0):
    """p: dropout rate between the ReLU and the second layer (0 = none: nothing is launched)."""
    return MLPFn.apply(W1, b1, W2, b2, out_dtype, x, _check_rate(p))


_pair_mlp = {"on": os.environ.get("JMT_PAIR_MLP", "1") != "0"}
_fused_head_on = {"on": os.environ.get("JMT_FUSED_HEAD", "1") != "0"}


# A/B switches of the head / loss tail (each default on; 0 = the launches it replaced):
#   JMT_HEAD_PERM         the fused head writes seq-first predictions in their logical order
#                         (jmt_head_*_perm) instead of a transposing copy after it
#   JMT_CCC_FUSED_FINISH  one-rank CCC losses: statistics and finish in one launch
#   JMT_STACK_INPLACE     the video projection and the normalised audio are written into their
#                         slots of the stacked X (models/two_transformers.py, grouped.StackJointFn)
_tail = {"head_perm": os.environ.get("JMT_HEAD_PERM", "1") != "0",
         "ccc_fused_finish": os.environ.get("JMT_CCC_FUSED_FINISH", "1") != "0",
         "stack_inplace": os.environ.get("JMT_STACK_INPLACE", "1") != "0"}


def head_perm_enabled() -> bool:
    return _tail["head_perm"]


def set_head_perm(on: bool) -> None:
    _tail["head_perm"] = bool(on)


def ccc_fused_finish_enabled() -> bool:
    return _tail["ccc_fused_finish"]


def set_ccc_fused_finish(on: bool) -> None:
    _tail["ccc_fused_finish"] = bool(on)


def stack_inplace_enabled() -> bool:
    return _tail["stack_inplace"]


def set_stack_inplace(on: bool) -> None:
    _tail["stack_inplace"] = bool(on)


def pair_mlps_enabled() -> bool:
    """Two_transformers runs its V / A regressors as one MLPPairFn (JMT_PAIR_MLP=0: two MLPFn)."""
    return _pair_mlp["on"]


def set_pair_mlps(on: bool) -> None:
    _pair_mlp["on"] = bool(on)


class MLPPairFn(Function):
    """(MLP_a(x), MLP_b(x)) for two same-shaped MLPs on ONE input: the V and A regressors of
    two_transformers.py:104-114,125-126.  Per output element the arithmetic is
    MLPFn's, with half the launches: both first layers are one GEMM launch (a 2-entry weight /
    bias table writing [h_a | h_b] side by side), both second layers one launch over the halves
    of h, and in the backward both second-layer input gradients, both second-layer and both
    first-layer weight gradients are one launch each, both first-layer bias gradients one grouped
    column sum; the input gradient is the two dgrads and the same 16-bit add autograd performs
    for the two uses of x.  Dropout rates (p_a, p_b), either > 0: one state-block copy per call
    (ops.dropout_next); the fused-head route masks h in registers (the *_drop head kernels, h
    itself stays unmasked in memory), the GEMM route masks the pair buffer h and then dh in
    place, one launch each with split = hid (as MLPFn)."""

    @staticmethod
    def forward(ctx, W1a, b1a, W2a, b2a, W1b, b1b, W2b, b2b, out_dtype, x, p_a=0.0, p_b=0.0):
        cd = compute_dtype()
        L = Rows(x, cd)
        hid, nout = W1a.shape[0], W2a.shape[0]
        h = L.like(2 * hid, cd)
        ldh = _ld(h, L.perm)
        # both first layers: one launch writing [h_a | h_b] side by side
        lg.fwd(L.op(), L.rows, (W1a, W1b), (b1a, b1b), lg.strided(h, ldh, hid), cd, relu=True)
        odt = out_dtype if out_dtype is not None else cd
        fused = MLPPairFn._fused_head(cd, hid, nout)
        # x seq-first over batch-first rows (the FC head's av): the head kernels store the
        # outputs in their logical order, contiguous, through the row map pq
        pq = MLPPairFn._head_perm(L) if fused else None
        if pq is not None:
            ys = [torch.empty(L.shape[:-1] + (nout,), dtype=odt, device=h.device)
                  for _ in range(2)]
            ldy = nout
        else:
            ys = [L.like(nout, odt), L.like(nout, odt)]
            ldy = _ld(ys[0], L.perm)
        W2c = [weight_as(W2a, cd), weight_as(W2b, cd)] if fused else None
        ctr = None
        if p_a > 0.0 or p_b > 0.0:
            ctr = ops.dropout_next(_drop_block(h.device))
            if not fused:
                ops.dropout(h, ldh, h, ldh, L.rows, 2 * hid, hid, p_a, p_b, ctr)
        if fused and ctr is not None:
            ops.head_fwd_drop(h, ldh, L.rows, nout, W2c, (b2a, b2b), ys, ldy, p_a, p_b, ctr,
                              perm=pq)
        elif fused:
            # both second layers as one row kernel over [h_a | h_b] (csrc/head.hip)
            ops.head_fwd(h, ldh, L.rows, nout, W2c, (b2a, b2b), ys, ldy, perm=pq)
        else:
            # both second layers: one GEMM launch over the halves of h (2-entry tables)
            lg.fwd(lg.strided(h, ldh, hid), L.rows, (W2a, W2b), (b2a, b2b),
                   lg.table(ys, _ld(ys[0], L.perm)), cd)
        ctx.save_for_backward(W1a, b1a, W2a, b2a, W1b, b1b, W2b, b2b, L.t, h, ctr)
        ctx.meta = (cd, L, x.dtype, odt, fused, p_a, p_b, pq)
        return ys[0], ys[1]

    @staticmethod
    def _head_perm(L: Rows):
        """(P, Q) of the head kernels' row map when the two leading dims of x are a transposition
        of its row order in memory (logical (T, B), rows r = b T + t: P = T, Q = B), else None
        (JMT_HEAD_PERM=0: always None, the outputs keep x's row order)."""
        if not _tail["head_perm"] or list(L.perm) != [1, 0] or L.rows >= 1 << 31:
            return None
        T, B = L.shape[0], L.shape[1]
        return (T, B) if T > 1 and B > 1 else None

    @staticmethod
    def _fused_head(cd, hid, nout) -> bool:
        """The output layers run as csrc/head.hip row kernels (16-bit compute, hidden width 128,
        k <= 24: the V / A regressors and configs[4]'s 20-bin head); JMT_FUSED_HEAD=0 keeps
        the GEMM form."""
        return (_fused_head_on["on"] and cd != torch.float32 and hid == ops.HEAD_HID and
                nout <= ops.HEAD_KMAX)

    @staticmethod
    def _w2_grads(Gs, hh, ldhh, hid, nout, W2s, b2s, dt):
        """W2_g.grad += G_g^T h_g (both in one launch when the gradients share a row stride and
        neither weight is frozen), b2_g.grad += column sums of G_g."""
        if (nout == 1 or Gs[0].ld == Gs[1].ld) and all(W.requires_grad for W in W2s):
            lg.wgrad(lg.table([G.t for G in Gs], Gs[0].ld), lg.strided(hh, ldhh, hid),
                     Gs[0].rows, nout, W2s, dt, queue=False)
        else:
            for half, (G, W2) in enumerate(zip(Gs, W2s)):
                lg.wgrad(G.op(), lg.strided(hh[..., half * hid:(half + 1) * hid], ldhh), G.rows,
                         nout, W2, dt)
        for G, b2 in zip(Gs, b2s):
            lg.bias_grad(G.op(), G.rows, nout, [b2])

    @staticmethod
    @once_differentiable
    def backward(ctx, gya, gyb):
        W1a, b1a, W2a, b2a, W1b, b1b, W2b, b2b, xin, h, ctr = ctx.saved_tensors
        cd, L, xdt, odt, fused, p_a, p_b, pq = ctx.meta
        hid, nout = W1a.shape[0], W2a.shape[0]
        dev = h.device
        ldh = _ld(h, L.perm)
        hs = (h[..., :hid], h[..., hid:])
        dh = L.like(2 * hid, cd)
        dhs = (dh[..., :hid], dh[..., hid:])

        gys = []
        for gy in (gya, gyb):
            if gy is None:
                gy = torch.zeros(L.like(nout, odt).shape, dtype=odt, device=dev)
            gys.append(gy)
        if fused:       # (the route the forward took: with dropout, h is masked only off it)
            # dh (ReLU-masked) and both output layers' weight / bias gradients in one row
            # kernel from the fp32 loss gradient (csrc/head.hip), then the input gradient as ONE
            # K-concatenated GEMM dx = [dh_a | dh_b] [W1a; W1b] (one rounding of the sum of both
            # heads' contributions, no separate add)
            gdt = torch.float32 if odt == torch.float32 else cd
            if pq is not None:
                # the gradients of the logically contiguous outputs, read through the forward's
                # row map as they arrive (no re-layout into x's row order)
                gts = [gy if gy.dtype == gdt and gy.is_contiguous() else
                       gy.to(gdt).contiguous() for gy in gys]
                ldg = nout
            else:
                G2 = [_match(gy, Rows(L.like(nout, gdt)), gdt) for gy in gys]
                if G2[1].ld != G2[0].ld or G2[1].perm != G2[0].perm:
                    G2[1] = _match(G2[1].t, G2[0], gdt)
                gts, ldg = [G.t for G in G2], G2[0].ld
            W2c = [weight_as(W2a, cd), weight_as(W2b, cd)]
            dw2 = [_grad_buffer(W2a), _grad_buffer(W2b)]
            db2 = [_grad_buffer(b2a), _grad_buffer(b2b)]
            if ctr is not None:
                ops.head_bwd_drop(h, ldh, L.rows, nout, W2c, gts, ldg, dh, ldh, dw2, db2, p_a,
                                  p_b, ctr, perm=pq)
            else:
                ops.head_bwd(h, ldh, L.rows, nout, W2c, gts, ldg, dh, ldh, dw2, db2, perm=pq)
            _grad_done(W2a, W2b, b2a, b2b)
            dx = None
            if ctx.needs_input_grad[9]:
                dx = L.like(L.F, cd)
                W1c = [weight_as(W1a, cd), weight_as(W1b, cd)]
                lg.dgrad(lg.strided(dh, ldh), L.rows, 2 * hid, lg.kcat(W1c, L.F, hid),
                         _out(dx, L.perm), cd)
                if xdt != cd:
                    dx = _cast_keep_layout(dx, xdt)
            # one batched launch (+ one grouped column-sum launch pair)
            lg.wgrad(lg.strided(dh, ldh, hid), lg.strided(xin, L.ld), L.rows, hid, (W1a, W1b),
                     cd, (b1a, b1b), queue=False)
            return (None,) * 9 + (dx, None, None)
        Gys = [_match(gy, Rows(L.like(nout, cd)), cd) for gy in gys]
        if nout == 1 or Gys[0].ld == Gys[1].ld:
            # both second-layer input gradients (ReLU-masked) in one launch into [dh_a | dh_b]
            lg.dgrad(lg.table([G.t for G in Gys], Gys[0].ld), L.rows, nout, (W2a, W2b),
                     lg.strided(dh, ldh, hid), cd, aux=h, ldaux=ldh)
        else:
            for Gy, W2, hp, dhp in zip(Gys, (W2a, W2b), hs, dhs):
                lg.dgrad(Gy.op(), Gy.rows, nout, W2, lg.strided(dhp, ldh), cd, aux=hp, ldaux=ldh)
        if ctr is not None:
            ops.dropout(dh, ldh, dh, ldh, L.rows, 2 * hid, hid, p_a, p_b, ctr)
        if odt == torch.float32 and cd != torch.float32 and nout <= 16:     # as in MLPFn
            h32 = _cast_keep_layout(h, torch.float32)
            G32 = [_match(gy, Rows(L.like(nout, torch.float32)), torch.float32) for gy in gys]
            MLPPairFn._w2_grads(G32, h32, _ld(h32, L.perm), hid, nout, (W2a, W2b),
                                (b2a, b2b), torch.float32)
        else:
            MLPPairFn._w2_grads(Gys, h, ldh, hid, nout, (W2a, W2b), (b2a, b2b), cd)
        dx = None
        if ctx.needs_input_grad[9]:
            dx = L.like(L.F, cd)
            dxb = L.like(L.F, cd)
            for dhp, W1, o in zip(dhs, (W1a, W1b), (dx, dxb)):
                Gh = Rows(dhp)
                lg.dgrad(Gh.op(), Gh.rows, hid, W1, _out(o, L.perm), cd)
            # the sum of the two input gradients rounded as autograd rounds it (a beta = 1
            # accumulate in the second dgrad saves this add but rounds once less, which moved an
            # fp16 gradient of the H8/L2 golden case 0.02 % past the error model's bound)
            dx.add_(dxb)
            if xdt != cd:
                dx = _cast_keep_layout(dx, xdt)
        # one batched launch (+ one grouped column-sum launch pair)
        lg.wgrad(lg.strided(dh, ldh, hid), lg.strided(xin, L.ld), L.rows, hid, (W1a, W1b),
                 cd, (b1a, b1b), queue=False)
        return (None,) * 9 + (dx, None, None)


def mlp_pair(x, mlp_a, mlp_b, out_dtype=None, p=(0.0, 0.0)):
    """Both regressor MLPs (jmt.nn.MLP: Linear, ReLU, [Dropout], Linear) on the same x; p: the
    two dropout rates in effect (0 in eval)."""
    la1, la2 = mlp_a[0], mlp_a[len(mlp_a) - 1]
    lb1, lb2 = mlp_b[0], mlp_b[len(mlp_b) - 1]
    return MLPPairFn.apply(la1.weight, la1.bias, la2.weight, la2.bias, lb1.weight, lb1.bias,
                           lb2.weight, lb2.bias, out_dtype, x, _check_rate(p[0]),
                           _check_rate(p[1]))


# ------------------------------------------------------------------------- L2 normalize
class L2NormFn(Function):
    """F.normalize(x, p=2, dim=-1, eps=1e-12) (two_transformers.py:118-119)."""

    @staticmethod
    def forward(ctx, x, eps, out=None):
        cd = compute_dtype()
        L = Rows(x)
        y = _into(out, L, L.F, cd, "l2_normalize")
        inv = torch.empty(L.rows, dtype=torch.float32, device=x.device)
        ops.l2norm_fwd(L.t, L.ld, L.rows, L.F, y, _ld(y, L.perm), inv, eps)
        ctx.save_for_backward(L.t, inv)
        ctx.meta = (L, eps, cd)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, inv = ctx.saved_tensors
        L, eps, cd = ctx.meta
        G = _match(gy, Rows(L.like(L.F, cd)), cd)
        dx = L.like(L.F, x.dtype)
        ops.l2norm_bwd(x, L.ld, G.t, G.ld, inv, eps, dx, _ld(dx, L.perm), L.rows, L.F)
        return dx, None, None


def l2_normalize(x, eps=1e-12, out=None):
    """out: a preallocated tensor the kernel writes (the layout the call would allocate itself)."""
    return L2NormFn.apply(x, eps, Into(out) if out is not None else None)


# ------------------------------------------------------------------------- residual LayerNorm
class AddLayerNormFn(Function):
    """y = LayerNorm(x + r) (mm_multi_transformers.py:64-70: x = layer_norm(x + sublayer(x)))."""

    @staticmethod
    def forward(ctx, x, r, gamma, beta, eps):
        cd = compute_dtype()
        L = Rows(x, cd)
        R = Rows(r, cd) if r is not None else None
        if R is not None and not R.same_rows(L):
            rr = L.like(L.F, cd)
            rr.copy_(r)
            R = Rows(rr)
        y = L.like(L.F, cd)
        mean = torch.empty(L.rows, dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        ops.layernorm_fwd(L.t, L.ld, R.t if R else None, R.ld if R else 0, gamma, beta, eps, y,
                          _ld(y, L.perm), mean, rstd, L.rows, L.F)
        ctx.save_for_backward(L.t, R.t if R else None, gamma, beta, mean, rstd)
        ctx.meta = (L, R.ld if R else 0, cd, x.dtype, r.dtype if r is not None else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, r, gamma, beta, mean, rstd = ctx.saved_tensors
        L, ldr, cd, xdt, rdt = ctx.meta
        G = _match(gy, Rows(L.like(L.F, cd)), cd)
        dx = L.like(L.F, cd)
        dg = _grad_buffer(gamma)
        db = _grad_buffer(beta)
        tmp = None
        if dg is None or db is None:
            # one accumulate flag for both outputs: with a buffer missing both go to scratch and
            # the present one accumulates it (gradient accumulation stays intact)
            tmp = torch.zeros(2, L.F, dtype=torch.float32, device=x.device)
        ops.layernorm_bwd(x, L.ld, r, ldr, G.t, G.ld, mean, rstd, gamma, dx, _ld(dx, L.perm),
                          dg if tmp is None else tmp[0], db if tmp is None else tmp[1],
                          tmp is None, L.rows, L.F)
        if tmp is not None:
            for b, t in ((dg, tmp[0]), (db, tmp[1])):
                if b is not None:
                    b.add_(t)
        _grad_done(gamma, beta)
        dxx = dx if xdt == cd else _cast_keep_layout(dx, xdt)
        drr = None
        if r is not None:
            drr = dx if rdt == cd else _cast_keep_layout(dx, rdt)
        return dxx, drr, None, None, None


def add_layer_norm(x, r, gamma, beta, eps=1e-5):
    return AddLayerNormFn.apply(x, r, gamma, beta, eps)


# ------------------------------------------------------------------------- attention core
def _round_up(a, b):
    return -(-a // b) * b


class KeyRanges:
    """A key padding mask as one run of valid keys per sequence: `table` is the device array of
    int32 {kbeg, kend} pairs the *_kr kernels read (include/jmt.h), `B` its entries, `Lk` the
    mask's key count.  Sequence n of a launch uses entry n % B, so the grouped launches (3 B and
    6 B sequences) share the table of the B windows.  Built by key_ranges()."""
    __slots__ = ("table", "B", "Lk")

    def __init__(self, table, B, Lk):
        self.table, self.B, self.Lk = table, B, Lk

    @property
    def op(self):
        """(table, kr_mod): the `kr` operand of the ops.attn_* wrappers."""
        return (self.table, self.B)


_KR_PENDING = {}     # device -> int32 count of mask rows that were not one non-empty run


def key_ranges(key_padding_mask) -> "KeyRanges":
    """The KeyRanges of a (B, Lk) bool / uint8 key padding mask (True = ignore the key, torch's
    convention), by one kernel (jmt_kpm_ranges; no torch op, so a captured step stays free of
    torch kernels).  Padding is contiguous: every row must hold exactly one non-empty run of valid
    keys (padded on the left, on the right or both).  A row without a valid key (torch returns NaN
    there) or with a hole is counted on the device.  Eager: the count is read here (one host
    read) and a non-zero count raises ValueError.  Under graph capture no host read is possible:
    the count accumulates on the device and check_key_ranges() (or the next eager key_ranges call)
    raises on it.  A KeyRanges passes through unchanged."""
    m = key_padding_mask
    if isinstance(m, KeyRanges):
        return m
    if not torch.is_tensor(m) or m.dtype not in (torch.bool, torch.uint8):
        raise NotImplementedError("key_padding_mask: a bool (or uint8) mask or a KeyRanges; float "
                                  "masks are not used on the JMT path")
    if m.dim() != 2:
        raise ValueError(f"key_padding_mask must be (N, Lk), got {tuple(m.shape)}")
    dev = m.device
    capturing = dev.type == "cuda" and torch.cuda.is_current_stream_capturing()
    bad = _KR_PENDING.get(dev)
    if bad is None:
        if capturing:
            raise RuntimeError("key_ranges under graph capture: run it once eagerly first (the "
                               "bad-mask counter is allocated there)")
        bad = _KR_PENDING[dev] = torch.zeros(1, dtype=torch.int32, device=dev)
    if m.stride(1) != 1:
        m = m.contiguous()
    B, Lk = m.shape
    table = torch.empty(2 * B, dtype=torch.int32, device=dev)
    ops.kpm_ranges(m, table, bad)
    if not capturing:
        check_key_ranges(dev)
    return KeyRanges(table, B, Lk)


def check_key_ranges(dev=None):
    """Raise ValueError if a key_ranges call since the last check saw a mask row that is not one
    non-empty run of valid keys (the count kept on the device while the step was replayed from a
    graph); clears the count."""
    devs = [dev] if dev is not None else list(_KR_PENDING)
    n = 0
    for d in devs:
        bad = _KR_PENDING.get(d)
        if bad is not None:
            c = int(bad.item())
            if c:
                bad.zero_()
            n += c
    if n:
        raise ValueError(f"key_padding_mask: {n} row(s) are not one non-empty run of valid keys "
                         "(a row with every key masked, or valid keys that are not contiguous)")


class AttnCoreFn(Function):
    """softmax(Q K^T / sqrt(dh)) V per (batch, head) — the core of F.multi_head_attention_forward
    (SURVEY.md §8a a6).  Q/K/V are column slices (qcol/kcol/vcol) of the in-projection outputs
    q_src (Lq, N, *), k_src / v_src (Lk, N, *) in any strided seq-first layout, so self-attention
    (one packed qkv) and key-is-value cross-attention (q + packed kv) read their projections in
    place and write their gradients into packed buffers consumed by ONE in_proj dgrad/wgrad.
    16-bit head_dim 512: the fused kernels of attn.hip (no score matrix in the forward; the
    backward recomputes P from lse).  Otherwise scores are materialised as fp32 (N, H, Lq, ldS),
    probabilities in the compute dtype."""

    @staticmethod
    def _probs(q_src, k_src, E, H, qcol, kcol, ldS, scale, cd, kr=None):
        """P = softmax(scale Q K^T) as (N, H, Lq, ldS) in the compute dtype (score GEMM into fp32
        + jmt_softmax_fwd; kr: over each sequence's key range, zero outside it)."""
        Lq, N = q_src.shape[0], q_src.shape[1]
        Lk = k_src.shape[0]
        dh = E // H
        dev = q_src.device
        bS = (H * Lq * ldS, Lq * ldS)
        S = torch.empty(N * H * Lq * ldS, dtype=torch.float32, device=dev)
        ops.gemm(M=Lq, N=Lk, K=dh, ab_dtype=_dc(cd), c_dtype=F32,
                 a=[_ptr(q_src, qcol)], lda=q_src.stride(0), a_kmajor=True,
                 sA=(q_src.stride(1), dh),
                 b=[_ptr(k_src, kcol)], ldb=k_src.stride(0), b_kmajor=True,
                 sB=(k_src.stride(1), dh),
                 c=[S.data_ptr()], ldc=ldS, sC=bS, batch0=N, batch1=H, device=dev)
        P = torch.empty(N * H * Lq * ldS, dtype=cd, device=dev)
        ops.softmax_fwd(S, ldS, N * H * Lq, Lk, scale, P, ldS, kr=kr, rows_per_seq=H * Lq)
        return P

    @staticmethod
    def forward(ctx, q_src, k_src, v_src, E, H, qcol, kcol, vcol, kr=None, drop_p=0.0):
        o, saved = attn_forward(q_src, k_src, v_src, E, H, qcol, kcol, vcol, kr=kr,
                                drop_p=drop_p)
        # which inputs are the same tensor (saved tensors are not guaranteed to unpack to the
        # same Python objects, so the aliasing is recorded here)
        owner = (0, 0 if k_src is q_src else 1,
                 0 if v_src is q_src else (1 if v_src is k_src else 2))
        ctx.save_for_backward(*saved[0])
        ctx.meta = (saved[1], owner)
        return o

    @staticmethod
    @once_differentiable
    def backward(ctx, go):
        tensors = ctx.saved_tensors
        meta, owner = ctx.meta
        q_src, k_src, v_src = tensors[:3]
        cd = meta.cd
        # one gradient buffer per distinct source tensor (packed qkv -> one buffer)
        srcs = (q_src, k_src, v_src)
        bufs = [None, None, None]
        E, cols = meta.E, (meta.qcol, meta.kcol, meta.vcol)
        for i in range(3):
            if owner[i] == i:
                width = srcs[i].shape[-1]
                bufs[i] = Rows(srcs[i]).like(width, cd)
                # columns of a source that no Q/K/V slice reads get a zero gradient
                covered = set()
                for j in range(3):
                    if owner[j] == i:
                        covered.update(range(cols[j], cols[j] + E))
                if len(covered) < width:
                    bufs[i].zero_()
        attn_backward((tensors, meta), go, bufs[owner[0]], bufs[owner[1]], bufs[owner[2]])
        grads = [bufs[i] if owner[i] == i else None for i in range(3)]
        return (*grads, None, None, None, None, None, None, None)


def _small_aligned(t, col, cd):
    """Row starts 16-B (fp32: 32-B) aligned and strides multiples of 8 elements, as
    jmt_small_attn_* require (include/jmt.h)."""
    es = t.element_size()
    return ((t.data_ptr() + col * es) % (32 if es == 4 else 16) == 0
            and t.stride(0) % 8 == 0 and t.stride(1) % 8 == 0)


class AttnOperand(NamedTuple):
    """What attn_plan asks of an operand view: `aligned` as _small_aligned at its column offset,
    `stride` its row stride in elements."""
    aligned: bool
    stride: int


def _operand(t, col, cd) -> AttnOperand:
    return AttnOperand(_small_aligned(t, col, cd), t.stride(0))


class AttnPlan(NamedTuple):
    """fwd: "small" | "short" | "fused" | "mh" (the fused multi-head kernels, head dim 64 or
    128) | "gemm" (GEMM + softmax).  rows: the fused forward is the whole-row kernel (False for
    "mh").  bwd (None while the gradient buffers are unknown): "small" | "short" | "pds_dkdv"
    (P / dS kernel + attn_dkdv with dQ) | "bwd64_dkdv" (64-row backward with dQ + attn_dkdv) |
    "bwd64_gemm" (64-row backward + two batched GEMMs) | "mh" (whenever the forward ran "mh") |
    "gemm".  shared_q: the *_sq launches take the call (whole-row forward and "pds_dkdv"; never
    "mh").  With key ranges (kr) the answers are "short", "fused" on the whole-row kernel (its
    backward must come out "pds_dkdv": attn_backward raises otherwise), "mh" or "gemm": the
    kernels that take a range table."""
    fwd: str
    rows: bool
    bwd: Optional[str]
    shared_q: bool


# what attn_backward keeps of an attn_forward call besides its tensors (fwd: AttnPlan.fwd)
# kr: the key range operand (table, kr_mod) of a call with ranges, else None
# drop: (p, state copy) of a call with attention dropout (the operand of the ops wrappers), else
# None
AttnMeta = collections.namedtuple("AttnMeta", "E H qcol kcol vcol ldS scale cd fwd kr drop",
                                  defaults=(None,))


def attn_dropout_rate(p) -> float:
    """The attention dropout rate in effect for `p`.  The mask spends 8 bits per element
    (csrc/dropout.h), so the rate is quantised to 1 / 256: p_eff = floor(256 p + 1/2) / 256, and
    kept probabilities are scaled by 1 / (1 - p_eff).  p < 1 / 512 is no dropout at all."""
    return ops.attn_dropout_rate(_check_rate(p))


def _attn_drop_counter_ok(N, H, Lq) -> bool:
    """The mask's counter holds 32 bits of (sequence, head, 4-query block)."""
    return N * H * ((Lq + 3) // 4) <= 1 << 32


def attn_plan(cd, N, H, Lq, Lk, E, q, k, v, o, go=None, dq=None, dk=None, dv=None,
              fwd=None, kr=False, drop=False) -> AttnPlan:
    """The one place an attention call's kernels are chosen (host only, no tensors).  q .. dv:
    AttnOperand of each view, the gradient ones (go: dO as attn_backward normalises it) once they
    exist.  fwd: the forward path already taken (attn_backward; the saved state fixes it).  The
    switches (ops._attn_fused / _attn_short / _attn_mh / _attn_dkdv / _attn_pds, the library's forward-rows
    switch) are read at every call and the kernels' ranges are asked of the library.  kr: the call
    carries key ranges, which the small kernels, the 64-row forward and the 64-row backward do
    not take.  drop: the call carries attention dropout: "small", "short" and "fused" have no
    masked form and decline; the answer is "mh" where the multi-head kernels take the call and
    the mask's counter covers it, else "gemm"."""
    dh = E // H
    half = cd != torch.float32
    if fwd is None:
        aligned = q.aligned and k.aligned and v.aligned and o.aligned
        # the multi-head kernels: asked last, after "small", "short" and "fused" have declined
        mh = lambda: (half and aligned and
                      ops.attn_mh_ok(_dc(cd), dh, N, H, Lq, Lk, q.stride, k.stride, v.stride))
        if drop:
            fwd = "mh" if mh() and _attn_drop_counter_ok(N, H, Lq) else "gemm"
        elif kr:
            if half and aligned and ops.attn_short_ok(_dc(cd), dh, Lq, Lk):
                fwd = "short"
            elif (half and ops.attn_supported(_dc(cd), dh) and
                  ops.attn_fwd_rows_ok(N, H, Lq, Lk, k.stride, v.stride)):
                fwd = "fused"
            elif mh():
                fwd = "mh"
            else:
                fwd = "gemm"
        elif aligned and ops.small_attn_ok(E, H, Lq, Lk):
            fwd = "small"
        elif half and aligned and ops.attn_short_ok(_dc(cd), dh, Lq, Lk):
            fwd = "short"
        elif half and ops.attn_supported(_dc(cd), dh):
            fwd = "fused"
        elif mh():
            fwd = "mh"
        else:
            fwd = "gemm"
    rows = fwd == "fused" and ops.attn_fwd_rows_ok(N, H, Lq, Lk, k.stride, v.stride)
    bwd = None
    if None not in (go, dq, dk, dv):
        bwd = fwd
        if fwd == "fused":
            ldp = ops.attn_dkdv_ldp(Lk)
            bwd = "bwd64_gemm"
            if (ops._attn_dkdv["on"] and dk.aligned and dv.aligned and
                    ops.attn_dkdv_ok(N, H, Lq, Lk, ldp, go.stride, q.stride, dk.stride,
                                     dv.stride)):
                bwd = "bwd64_dkdv"
                if (ops._attn_pds["on"] and dq.aligned and k.aligned and
                        ops.attn_bwd_pds_ok(N, H, Lq, Lk, ldp, k.stride, v.stride) and
                        ops.attn_dkdv_ok(N, H, Lq, Lk, ldp, go.stride, q.stride, dk.stride,
                                         dv.stride, k.stride, dq.stride)):
                    bwd = "pds_dkdv"
    return AttnPlan(fwd, rows, bwd, rows and bwd == "pds_dkdv")


def attn_forward(q_src, k_src, v_src, E, H, qcol, kcol, vcol, qshare=None, kr=None, drop_p=0.0):
    """softmax(Q K^T / sqrt(dh)) V on seq-first strided views (see AttnCoreFn).  Returns the
    output (Lq, N, E) (memory order of q_src's rows) and the state attn_backward needs.
    qshare = (spp, qtab): sequence p spp + b reads the Q rows of sequence qtab[p] spp + b
    (ops.attn_fwd_sq; the caller has asked attn_plan with its gradient layouts).
    kr: a KeyRanges; sequence n attends to the keys of its entry n % kr.B only.  A call with
    ranges never runs unmasked: attn_plan sends it to a kernel that takes the table.
    drop_p: dropout on the probabilities, O = dropout(softmax(S)) V, at the rate
    attn_dropout_rate(drop_p).  The call takes one state copy (ops.dropout_next: one `call` for
    the whole launch) and keeps (p, copy) for its backward.  A rate that rounds to 0 (and 0 itself)
    takes no copy and launches exactly the kernels of a call without dropout."""
    cd = compute_dtype()
    drop_p = _check_rate(drop_p)
    if drop_p > 0.0 and attn_dropout_rate(drop_p) == 0.0:
        drop_p = 0.0
    for t in (q_src, k_src, v_src):
        assert t.dtype == cd and t.stride(-1) == 1
    Lq, N = q_src.shape[0], q_src.shape[1]
    Lk = k_src.shape[0]
    dh = E // H
    dev = q_src.device
    ldS = _round_up(Lk, 8)
    bS = (H * Lq * ldS, Lq * ldS)
    scale = 1.0 / math.sqrt(dh)
    o = Rows(q_src).like(E, cd)
    if kr is not None:
        if kr.Lk != Lk or N % kr.B:
            raise ValueError(f"key ranges of a ({kr.B}, {kr.Lk}) mask on {N} sequences of {Lk} "
                             "keys")
        kr = kr.op
    plan = attn_plan(cd, N, H, Lq, Lk, E, _operand(q_src, qcol, cd), _operand(k_src, kcol, cd),
                     _operand(v_src, vcol, cd), _operand(o, 0, cd), kr=kr is not None,
                     drop=drop_p > 0.0)
    drop = (drop_p, ops.dropout_next(_drop_block(dev))) if drop_p > 0.0 else None
    if qshare is not None and not (plan.fwd == "fused" and plan.rows):
        raise JMTError("attn_forward: qshare on an unsupported shape")
    if kr is not None and (plan.fwd == "small" or (plan.fwd == "fused" and not plan.rows)):
        raise JMTError(f"attn_forward: key ranges on a path that takes none ({plan.fwd})")
    krk = {} if kr is None else {"kr": kr}
    if drop is not None:
        assert plan.fwd in ("mh", "gemm")
        if plan.fwd == "mh":
            krk["drop"] = drop
    if plan.fwd == "small":
        # short sequences (SELF_ATTEN head, intra-modal fusion): one wave per sequence, the
        # fp32 probabilities (N*H*Lq*Lk floats) kept for the backward (small_attn.hip)
        P = torch.empty(N * H * Lq * Lk, dtype=torch.float32, device=dev)
        ops.small_attn_fwd(_dc(cd), N, H, Lq, Lk, E,
                           _ptr(q_src, qcol), (q_src.stride(0), q_src.stride(1)),
                           _ptr(k_src, kcol), (k_src.stride(0), k_src.stride(1)),
                           _ptr(v_src, vcol), (v_src.stride(0), v_src.stride(1)),
                           o.data_ptr(), (o.stride(0), o.stride(1)), scale, P)
        tensors = (q_src, k_src, v_src, P, None, None)
    elif plan.fwd in ("short", "fused", "mh"):
        # one kernel: scores stay on chip (attn.hip; Lq, Lk <= 32, the batch-axis attention of
        # wo_JR and the T = 16 real-data windows: one block per sequence, attn_short.hip); only
        # lse is kept for the backward, which recomputes the probabilities ("mh": head dim 64 /
        # 128, attn_mh.hip)
        lse = torch.empty(N * H * Lq, dtype=torch.float32, device=dev)
        (ops.attn_short_fwd if plan.fwd == "short" else
         ops.attn_mh_fwd if plan.fwd == "mh" else
         ops.attn_fwd_sq if qshare is not None else ops.attn_fwd)(
                     _dc(cd), N, H, Lq, Lk, dh,
                     _ptr(q_src, qcol), (q_src.stride(0), q_src.stride(1)),
                     _ptr(k_src, kcol), (k_src.stride(0), k_src.stride(1)),
                     _ptr(v_src, vcol), (v_src.stride(0), v_src.stride(1)),
                     o.data_ptr(), (o.stride(0), o.stride(1)), scale, lse,
                     *(qshare if qshare is not None else ()), **krk)
        tensors = (q_src, k_src, v_src, None, o, lse)
    else:
        P = AttnCoreFn._probs(q_src, k_src, E, H, qcol, kcol, ldS, scale, cd, kr)
        Pv = P
        if drop is not None:
            # the unmasked P stays for the backward; P~ = M o P feeds the P V GEMM only
            Pv = torch.empty_like(P)
            ops.attn_dropout(P, ldS, Pv, ldS, N * H, Lq, Lk, drop[0], drop[1])
        ops.gemm(M=Lq, N=dh, K=Lk, ab_dtype=_dc(cd), c_dtype=_dc(cd),
                 a=[Pv.data_ptr()], lda=ldS, a_kmajor=True, sA=bS,
                 b=[_ptr(v_src, vcol)], ldb=v_src.stride(0), b_kmajor=False,
                 sB=(v_src.stride(1), dh),
                 c=[o.data_ptr()], ldc=o.stride(0), sC=(o.stride(1), dh),
                 batch0=N, batch1=H, device=dev)
        tensors = (q_src, k_src, v_src, P, None, None)
    return o, (tensors, AttnMeta(E, H, qcol, kcol, vcol, ldS, scale, cd, plan.fwd, kr, drop))


def attn_backward(saved, go, dq, dk, dv, qshare=None, merge_dq=False):
    """Gradients of attn_forward written into dq / dk / dv (seq-first views laid out like the
    sources; the same qcol/kcol/vcol column offsets; dq/dk/dv may be the same packed buffer).
    qshare: as attn_forward's.  dQ is then still written per sequence, unless merge_dq: one
    dQ = dS_i K_i + dS_j K_j per shared query in its first use's rows of dq, the second use's
    rows left unwritten.  The path is attn_plan's answer for the buffers as they are handed in."""
    (q_src, k_src, v_src, *_), meta = saved
    E, H, qcol, kcol, vcol, _, _, cd, fwd, kr, drop = meta
    Lq, N = q_src.shape[0], q_src.shape[1]
    Lk = k_src.shape[0]
    v8 = _vec(cd)
    if go.dtype != cd or go.stride(-1) != 1 or go.stride(0) % v8 or go.stride(1) % v8:
        go = _cast_keep_layout(go if go.stride(-1) == 1 else go.contiguous(), cd)
    if fwd != "gemm" and not _small_aligned(go, 0, cd):
        go = go.clone(memory_format=torch.contiguous_format)
    # decided again with the buffers at hand and the switches as they are now
    bwd = attn_plan(cd, N, H, Lq, Lk, E, _operand(q_src, qcol, cd), _operand(k_src, kcol, cd),
                    _operand(v_src, vcol, cd), None, _operand(go, 0, cd), _operand(dq, qcol, cd),
                    _operand(dk, kcol, cd), _operand(dv, vcol, cd), fwd=fwd,
                    kr=kr is not None).bwd
    if kr is not None and bwd not in ("short", "pds_dkdv", "mh", "gemm"):
        raise JMTError("attn_backward: key ranges with buffers the P / dS + dK / dV / dQ kernels "
                       f"do not take (attn_plan: {bwd})")
    if qshare is not None and bwd != "pds_dkdv":
        raise JMTError("attn_backward: qshare with buffers the P / dS + dK / dV / dQ kernels "
                       f"do not take (attn_plan: {bwd})")
    # the fused kernels' layout contract covers the gradient buffers too: a misaligned one is
    # written through an aligned (contiguous) temporary and copied back.  Aliased buffers
    # (packed qkv — possibly distinct view objects of one buffer) share one temporary: keyed
    # on the memory the view spans, not on the Python object.
    outs, tmps = [], {}
    for buf, col in ((dq, qcol), (dk, kcol), (dv, vcol)):
        if bwd == "gemm" or _small_aligned(buf, col, cd):
            outs.append(buf)
            continue
        key = (buf.data_ptr(), tuple(buf.shape), tuple(buf.stride()))
        if key not in tmps:
            tmps[key] = (buf, buf.clone(memory_format=torch.contiguous_format))
        outs.append(tmps[key][1])
    _attn_backward_launch(bwd, saved, go, *outs, qshare, merge_dq)
    for buf, tmp in tmps.values():
        buf.copy_(tmp)


def _attn_backward_launch(bwd, saved, go, dq, dk, dv, qshare, merge_dq):
    """The launches of attn_backward's path `bwd` (attn_plan) on normalised buffers."""
    (q_src, k_src, v_src, P, o, lse), meta = saved
    E, H, qcol, kcol, vcol, ldS, scale, cd, _, kr, drop = meta
    krk = {} if kr is None else {"kr": kr}
    if drop is not None:
        if bwd not in ("mh", "gemm"):
            raise JMTError(f"attn_backward: attention dropout on a path without a mask ({bwd})")
        if bwd == "mh":
            krk["drop"] = drop
    Lq, N = q_src.shape[0], q_src.shape[1]
    Lk = k_src.shape[0]
    dh = E // H
    dev = q_src.device
    sq_l, sq_n = q_src.stride(0), q_src.stride(1)
    sk_l, sk_n = k_src.stride(0), k_src.stride(1)
    sv_l, sv_n = v_src.stride(0), v_src.stride(1)
    so_l, so_n = go.stride(0), go.stride(1)
    if bwd in ("small", "short", "mh"):
        gouts = [a for t, c in ((dq, qcol), (dk, kcol), (dv, vcol))
                 for a in (_ptr(t, c), (t.stride(0), t.stride(1)))]
        if bwd == "mh":
            # P recomputed from lse in the dQ and in the dK / dV kernel (no P / dS in HBM);
            # delta = rowsum(dO o O) passes from the first to the second through this workspace
            delta = torch.empty(N * H * Lq, dtype=torch.float32, device=dev)
            ops.attn_mh_bwd(_dc(cd), N, H, Lq, Lk, dh, go.data_ptr(), (so_l, so_n),
                            o.data_ptr(), (o.stride(0), o.stride(1)),
                            _ptr(q_src, qcol), (sq_l, sq_n), _ptr(k_src, kcol), (sk_l, sk_n),
                            _ptr(v_src, vcol), (sv_l, sv_n), lse, *gouts, scale, delta, **krk)
        elif bwd == "small":
            ops.small_attn_bwd(_dc(cd), N, H, Lq, Lk, E, go.data_ptr(), (so_l, so_n),
                               _ptr(q_src, qcol), (sq_l, sq_n), _ptr(k_src, kcol), (sk_l, sk_n),
                               _ptr(v_src, vcol), (sv_l, sv_n), P, *gouts, scale)
        else:
            # P recomputed from lse; dQ, dK and dV from one kernel (no P / dS in HBM)
            ops.attn_short_bwd(_dc(cd), N, H, Lq, Lk, dh, go.data_ptr(), (so_l, so_n),
                               o.data_ptr(), (o.stride(0), o.stride(1)),
                               _ptr(q_src, qcol), (sq_l, sq_n), _ptr(k_src, kcol), (sk_l, sk_n),
                               _ptr(v_src, vcol), (sv_l, sv_n), lse, *gouts, scale, **krk)
        return
    if bwd in ("pds_dkdv", "bwd64_dkdv"):
        # P and dS (rows of 128-key tiles) -> dK = dS^T Q and dV = P^T dO in one persistent
        # kernel; with the 128-row P / dS kernel (default) dQ = dS K is that kernel's third
        # product (JMT_ATTN_PDS=0: dQ inside the 64-row backward kernel instead)
        ldp = ops.attn_dkdv_ldp(Lk)
        P = torch.empty(N * H * Lq * ldp, dtype=cd, device=dev)
        dS = torch.empty(N * H * Lq * ldp, dtype=cd, device=dev)
        pds = bwd == "pds_dkdv"
        dq_args = (_ptr(dq, qcol), (dq.stride(0), dq.stride(1)))
        if qshare is not None:
            ops.attn_bwd_sq(_dc(cd), N, H, Lq, Lk, dh, go.data_ptr(), (so_l, so_n),
                            o.data_ptr(), (o.stride(0), o.stride(1)),
                            _ptr(q_src, qcol), (sq_l, sq_n), _ptr(k_src, kcol), (sk_l, sk_n),
                            _ptr(v_src, vcol), (sv_l, sv_n), lse, P, dS, ldp, scale, *qshare,
                            **krk)
            ops.attn_dkdv_sq(_dc(cd), N, H, Lq, Lk, dh, P, dS, ldp, go.data_ptr(), (so_l, so_n),
                             _ptr(q_src, qcol), (sq_l, sq_n), _ptr(dk, kcol),
                             (dk.stride(0), dk.stride(1)), _ptr(dv, vcol),
                             (dv.stride(0), dv.stride(1)), _ptr(k_src, kcol), (sk_l, sk_n),
                             *dq_args, *qshare, merge_dq)
            return
        ops.attn_bwd(_dc(cd), N, H, Lq, Lk, dh, go.data_ptr(), (so_l, so_n),
                     o.data_ptr(), (o.stride(0), o.stride(1)),
                     _ptr(q_src, qcol), (sq_l, sq_n), _ptr(k_src, kcol), (sk_l, sk_n),
                     _ptr(v_src, vcol), (sv_l, sv_n), lse, P, dS, ldp,
                     *((None, (0, 0)) if pds else dq_args), scale, **krk)
        ops.attn_dkdv(_dc(cd), N, H, Lq, Lk, dh, P, dS, ldp, go.data_ptr(), (so_l, so_n),
                      _ptr(q_src, qcol), (sq_l, sq_n), _ptr(dk, kcol),
                      (dk.stride(0), dk.stride(1)), _ptr(dv, vcol), (dv.stride(0), dv.stride(1)),
                      *((_ptr(k_src, kcol), (sk_l, sk_n)) + dq_args if pds else ()))
        return
    bS = (H * Lq * ldS, Lq * ldS)
    dS = torch.empty(N * H * Lq * ldS, dtype=cd, device=dev)
    if bwd == "bwd64_gemm":
        # P recomputed from lse, dP, softmax backward and dQ = dS K in one kernel; the exact P
        # and dS are written once for the dK / dV products below
        P = torch.empty(N * H * Lq * ldS, dtype=cd, device=dev)
        ops.attn_bwd(_dc(cd), N, H, Lq, Lk, dh, go.data_ptr(), (so_l, so_n),
                     o.data_ptr(), (o.stride(0), o.stride(1)),
                     _ptr(q_src, qcol), (sq_l, sq_n), _ptr(k_src, kcol), (sk_l, sk_n),
                     _ptr(v_src, vcol), (sv_l, sv_n), lse, P, dS, ldS,
                     _ptr(dq, qcol), (dq.stride(0), dq.stride(1)), scale)
    else:
        dP = torch.empty(N * H * Lq * ldS, dtype=torch.float32, device=dev)
        ops.gemm(M=Lq, N=Lk, K=dh, ab_dtype=_dc(cd), c_dtype=F32,
                 a=[go.data_ptr()], lda=so_l, a_kmajor=True, sA=(so_n, dh),
                 b=[_ptr(v_src, vcol)], ldb=sv_l, b_kmajor=True, sB=(sv_n, dh),
                 c=[dP.data_ptr()], ldc=ldS, sC=bS, batch0=N, batch1=H, device=dev)
        if drop is not None:
            # dP = M o (dO V^T) in place; the softmax backward takes the unmasked P
            ops.attn_dropout(dP, ldS, dP, ldS, N * H, Lq, Lk, drop[0], drop[1])
        ops.softmax_bwd(P, ldS, dP, ldS, N * H * Lq, Lk, scale, dS, ldS)
        del dP
        # dQ = dS K
        ops.gemm(M=Lq, N=dh, K=Lk, ab_dtype=_dc(cd), c_dtype=_dc(cd),
                 a=[dS.data_ptr()], lda=ldS, a_kmajor=True, sA=bS,
                 b=[_ptr(k_src, kcol)], ldb=sk_l, b_kmajor=False, sB=(sk_n, dh),
                 c=[_ptr(dq, qcol)], ldc=dq.stride(0), sC=(dq.stride(1), dh), batch0=N,
                 batch1=H, device=dev)
    # dK = dS^T Q
    ops.gemm(M=Lk, N=dh, K=Lq, ab_dtype=_dc(cd), c_dtype=_dc(cd),
             a=[dS.data_ptr()], lda=ldS, a_kmajor=False, sA=bS,
             b=[_ptr(q_src, qcol)], ldb=sq_l, b_kmajor=False, sB=(sq_n, dh),
             c=[_ptr(dk, kcol)], ldc=dk.stride(0), sC=(dk.stride(1), dh), batch0=N,
             batch1=H, device=dev)
    if drop is not None:
        # dV = P~^T dO with the forward's P~ regenerated (out of place: P is a saved tensor, a
        # retained graph reads it again)
        Pm = torch.empty_like(P)
        ops.attn_dropout(P, ldS, Pm, ldS, N * H, Lq, Lk, drop[0], drop[1])
        P = Pm
    # dV = P^T dO
    ops.gemm(M=Lk, N=dh, K=Lq, ab_dtype=_dc(cd), c_dtype=_dc(cd),
             a=[P.data_ptr()], lda=ldS, a_kmajor=False, sA=bS,
             b=[go.data_ptr()], ldb=so_l, b_kmajor=False, sB=(so_n, dh),
             c=[_ptr(dv, vcol)], ldc=dv.stride(0), sC=(dv.stride(1), dh), batch0=N,
             batch1=H, device=dev)


def multihead_attention(query, key, value, in_w, in_b, out_w, out_b, num_heads, kr=None,
                        dropout_p=0.0):
    """nn.MultiheadAttention(E, H, dropout=dropout_p)(query, key, value) in training mode (pass
    0 in eval), seq-first (L, N, E).
    Every reference call site passes key is value: then K and V come from
    one packed in_proj GEMM (and Q too for self-attention).  kr: the KeyRanges of a
    key_padding_mask.  dropout_p: on the attention probabilities (attn_forward's drop_p)."""
    E = in_w.shape[1]
    if query is key and key is value:
        qkv = linear(query, in_w, in_b, 0, 3 * E)
        o = AttnCoreFn.apply(qkv, qkv, qkv, E, num_heads, 0, E, 2 * E, kr, dropout_p)
    elif key is value:
        q = linear(query, in_w, in_b, 0, E)
        kv = linear(key, in_w, in_b, E, 2 * E)
        o = AttnCoreFn.apply(q, kv, kv, E, num_heads, 0, 0, E, kr, dropout_p)
    else:
        q = linear(query, in_w, in_b, 0, E)
        k = linear(key, in_w, in_b, E, E)
        v = linear(value, in_w, in_b, 2 * E, E)
        o = AttnCoreFn.apply(q, k, v, E, num_heads, 0, 0, 0, kr, dropout_p)
    return linear(o, out_w, out_b)


def multihead_attention_shared_query(query, keys, in_w, in_b, out_w, out_b, num_heads,
                                     kr=None, dropout_p=0.0):
    """[nn.MultiheadAttention(query, k, k) for k in keys] with ONE query projection: the
    reference applies each cross_attention_* module twice to the same query
    (mm_multi_transformers.py:142-167), so the q = query W_q^T + b_q GEMM is computed once."""
    E = in_w.shape[1]
    q = linear(query, in_w, in_b, 0, E)
    outs = []
    for key in keys:
        kv = linear(key, in_w, in_b, E, 2 * E)
        o = AttnCoreFn.apply(q, kv, kv, E, num_heads, 0, 0, E, kr, dropout_p)
        outs.append(linear(o, out_w, out_b))
    return outs


# ------------------------------------------------------------------------- stack / transpose
class StackSeqFn(Function):
    """torch.stack(xs, dim=2) of seq-first (T, B, E) tensors followed by permute(1,0,2,3),
    flatten(0,1), permute(1,0,2) (mm_multi_transformers.py:171-178) — or of batch-first (B,T,E)
    tensors followed by flatten(0,1).permute(1,0,2) (intra_modal_transformer_fusion.py:93-97):
    returns the seq-first (S, B*T, E) view of one (B, T, S, E) buffer filled by strided copies.
    The backward hands out strided views of the incoming gradient (no copies)."""

    @staticmethod
    def forward(ctx, seq_first_in, *xs):
        cd = compute_dtype()
        S = len(xs)
        x0 = xs[0]
        if seq_first_in:
            T, B, E = x0.shape
        else:
            B, T, E = x0.shape
        buf = torch.empty(B, T, S, E, dtype=cd, device=x0.device)
        for s, x in enumerate(xs):
            xb = x.permute(1, 0, 2) if seq_first_in else x      # (B, T, E) logical
            if xb.stride(2) == 1 and xb.stride(0) == T * xb.stride(1):
                ops.copy2d(xb.data_ptr(), ops.dt(xb), _ptr(buf, s * E), ops.dt(buf), B * T, E,
                           xb.stride(1), 1, S * E, 1)
            else:
                for bi in range(B):
                    xr = xb[bi]
                    ops.copy2d(xr.data_ptr(), ops.dt(xr), _ptr(buf, (bi * T * S + s) * E),
                               ops.dt(buf), T, E, xr.stride(0), xr.stride(1), S * E, 1)
        ctx.meta = (S, seq_first_in, B, T, E)
        return buf.view(B * T, S, E).permute(1, 0, 2)

    @staticmethod
    def backward(ctx, g):
        S, seq_first_in, B, T, E = ctx.meta
        gb = g.permute(1, 0, 2)
        gb = gb.view(B, T, S, E) if gb.is_contiguous() else gb.reshape(B, T, S, E)
        res = [gb[:, :, s, :].permute(1, 0, 2) if seq_first_in else gb[:, :, s, :]
               for s in range(S)]
        return (None, *res)


def stack_seq(xs, seq_first_in=True):
    return StackSeqFn.apply(seq_first_in, *xs)


class TransposeCopyFn(Function):
    """Contiguous copy of a 2-D (T, B) view (the seq-first V/A predictions of the FC head,
    two_transformers.py:125-128) so that train.py:303-307's .view(-1, T*B) works."""

    @staticmethod
    def forward(ctx, x):
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
        ops.copy2d(x.data_ptr(), ops.dt(x), out.data_ptr(), ops.dt(out), x.shape[0], x.shape[1],
                   x.stride(0), x.stride(1), x.shape[1], 1)
        ctx.meta = (x.shape, x.stride(), x.dtype)
        return out

    @staticmethod
    def backward(ctx, g):
        shape, stride, dtype = ctx.meta
        base = torch.empty_strided(shape, stride, dtype=g.dtype, device=g.device)
        ops.copy2d(g.data_ptr(), ops.dt(g), base.data_ptr(), ops.dt(base), shape[0], shape[1],
                   g.stride(0), g.stride(1), base.stride(0), base.stride(1))
        return base


# ------------------------------------------------------------------------- CCC losses
class CCCLossFn(Function):
    """losses/loss.py:18-32 (kind 0) and losses/CCCLoss.py:15-43 (kind 1) as one statistics
    kernel + (optional) all-gather of 8 doubles per rank + one finish kernel; backward is one
    elementwise kernel.  With a process group the loss is the GLOBAL-batch CCC, exactly what the
    reference computes after its DataParallel gather."""

    @staticmethod
    def forward(ctx, pred, label, kind, k, ignore, lo, hi, eps, bs, group, add=None):
        dev = pred.device
        pred_c = pred if pred.is_contiguous() else pred.contiguous()
        lab = label
        if lab.dtype == torch.float64:
            lab = lab.float().contiguous()       # (the kernel's statistics are float64 anyway)
        elif lab.dtype != torch.float32 or not lab.is_contiguous():
            lab = ops.cast(lab, torch.float32)
        stats = torch.empty(8, dtype=torch.float64, device=dev)
        if add is not None and (add.dtype != torch.float32 or add.numel() != 1):
            raise ValueError("ccc loss: `add` must be an fp32 scalar")
        world = 1
        if group is not None:
            import torch.distributed as dist
            world = dist.get_world_size(group)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        coef = torch.empty(8, dtype=torch.float64, device=dev)
        if world == 1 and _tail["ccc_fused_finish"]:
            # one rank: nothing to gather between the statistics and the finish — one launch
            ops.ccc_stats_finish(kind, pred_c, lab, k, ignore, lo, hi, stats, bs, eps, loss, coef,
                                 add=add)
        else:
            ops.ccc_stats(kind, pred_c, lab, k, ignore, lo, hi, stats)
            stats_all = stats
            if world > 1:
                from .graph import collective
                stats_all = torch.empty(8 * world, dtype=torch.float64, device=dev)
                # on the host between two segment replays under a SegmentedStep capture
                collective(lambda sa=stats_all, st=stats:
                           dist.all_gather_into_tensor(sa, st, group=group))
            ops.ccc_finish(kind, world, stats_all, bs, eps, loss, coef, add=add)
        ctx.save_for_backward(pred_c, lab, coef)
        ctx.meta = (kind, k, ignore, lo, hi, pred.shape, add.shape if add is not None else None)
        return loss

    @staticmethod
    def backward(ctx, g):
        pred, lab, coef = ctx.saved_tensors
        kind, k, ignore, lo, hi, shape, add_shape = ctx.meta
        g = g.to(torch.float32) if g.dtype != torch.float32 else g
        g = g.contiguous()
        dpred = torch.empty_like(pred)
        ops.ccc_bwd(kind, pred, lab, k, ignore, lo, hi, coef, g, dpred)
        # d(add + loss) / d add = 1: the incoming gradient as is (no kernel), in add's shape
        return (dpred.view(shape), None, None, None, None, None, None, None, None, None,
                g.view(add_shape) if add_shape is not None else None)


def ccc_loss(pred, label, eps=1e-8, digitize_num=1, rng=(-1.0, 1.0), group=None, add=None):
    """add: an fp32 scalar (e.g. the other head's loss) returned summed with this loss by the
    finish kernel — train.py:311's v_loss + a_loss without an add launch."""
    k = int(digitize_num)
    return CCCLossFn.apply(pred, label, 0, k, 0.0, float(rng[0]), float(rng[1]), float(eps), 1,
                           group, add)


def ccc_loss_ignore(pred, label, ignore=-5.0, group=None):
    # losses/CCCLoss.py:17 divides by y_pred.size(0) of the (gathered) batch: for the (1, B*T)
    # view of train.py:303-307 that is 1 on every rank; for 1-D predictions the gathered size(0)
    # is the sum of the ranks' sizes (-1: summed on the device by jmt_ccc_finish)
    bs = pred.shape[0] if pred.dim() >= 2 else -1
    return CCCLossFn.apply(pred, label, 1, 1, float(ignore), -1.0, 1.0, 0.0, int(bs), group)


_CE_EDGES: dict = {}
_CE_PENDING: dict = {}       # device -> float64 count of out-of-range labels seen under capture
# eager CELoss reads the out-of-range label count at once (one host read, where the reference's
# own digitize synchronises); False defers it to the device flag like a captured step
CE_EAGER_LABEL_CHECK = [True]


def _ce_label_check(stats_all, dev):
    """The reference digitizes on the host and F.cross_entropy raises IndexError on the bin -1
    a label below range[0] gets (losses/loss.py:45-51).  The statistics kernel counts those
    labels (stats[2] of every rank).  Eager: the count is read here (the reference synchronises
    in the same place, y.data.cpu()) and a non-zero count raises.  Under hipGraph capture no host
    read is possible: the count accumulates into a per-device flag on the device, which the next
    eager CELoss call (or check_ce_labels()) reads and raises on."""
    counts = stats_all[2::4]
    capturing = dev.type == "cuda" and torch.cuda.is_current_stream_capturing()
    pend = _CE_PENDING.get(dev)
    if pend is None:
        if capturing:
            raise RuntimeError("CELoss under graph capture: run it once eagerly first (the "
                               "out-of-range label flag is allocated there)")
        pend = _CE_PENDING[dev] = torch.zeros((), dtype=torch.float64, device=dev)
    if capturing or not CE_EAGER_LABEL_CHECK[0]:
        pend.add_(counts.sum())
        return
    check_ce_labels(dev, extra=counts)


def check_ce_labels(dev=None, extra=None):
    """Raise IndexError if a CELoss call since the last check saw a label below range[0] (the
    count kept on the device while the step was replayed from a graph); clears the flag."""
    devs = [dev] if dev is not None else list(_CE_PENDING)
    bad = 0.0
    for d in devs:
        pend = _CE_PENDING.get(d)
        if pend is not None:
            bad += float(pend)
            pend.zero_()
    if extra is not None:
        bad += float(extra.sum())
    if bad > 0:
        raise IndexError(f"CELoss: {int(bad)} label(s) below range[0] digitize to class -1 "
                         "(Target -1 is out of bounds.)")


class CELossFn(Function):
    """losses/loss.py:34-51 CELoss on the device: digitize + weighted log-softmax NLL in one
    statistics kernel, (optional) all-gather of 4 doubles per rank, one finish kernel; backward
    one elementwise kernel.  Host synchronisation: one read of the out-of-range label count per
    eager call (`CE_EAGER_LABEL_CHECK`, default on: the reference's own digitize reads the labels
    on the host at the same point, loss.py:48, and F.cross_entropy raises there); with it off, and
    always under graph capture, the count accumulates on the device and `check_ce_labels()` raises
    on it later, so the step issues without a host read."""

    @staticmethod
    def forward(ctx, x, label, k, lo, hi, weights, group):
        dev = x.device
        xc = x if x.is_contiguous() else x.contiguous()
        lab = label.reshape(-1)
        if lab.dtype == torch.float64:
            # the reference digitizes the label's own values against float64 edges
            # (loss.py:48, np.digitize): a float64 label within fp32 rounding of an edge must
            # not change bin by the cast, so the bin is found here in float64 and the kernel
            # gets an fp32 representative of it (the bin centre; lo - 1 below the range, where
            # the reference raises and the kernel yields NaN)
            key = (lo, hi, k, str(dev))
            edges = _CE_EDGES.get(key)
            if edges is None:            # numpy's linspace bit for bit (torch's differs by ulps)
                import numpy as np
                edges = _CE_EDGES[key] = torch.from_numpy(np.linspace(lo, hi, num=k + 1)).to(dev)
            idx = torch.bucketize(lab, edges, right=True) - 1           # np.digitize - 1
            centre = ((edges[:-1] + edges[1:]) * 0.5).float()
            lab = torch.where(idx < 0, torch.full_like(centre[:1], lo - 1.0),
                              centre[idx.clamp(0, k - 1)]).contiguous()
        elif lab.dtype != torch.float32 or not lab.is_contiguous():
            lab = ops.cast(lab, torch.float32)
        w = None
        if weights is not None:
            w = weights if (weights.device == dev and weights.dtype == torch.float32 and
                            weights.is_contiguous()) else \
                weights.to(device=dev, dtype=torch.float32).contiguous()
        stats = torch.empty(4, dtype=torch.float64, device=dev)
        ops.ce_stats(xc, lab, k, lo, hi, w, stats)
        world, stats_all = 1, stats
        if group is not None:
            import torch.distributed as dist
            world = dist.get_world_size(group)
            if world > 1:
                from .graph import collective
                stats_all = torch.empty(4 * world, dtype=torch.float64, device=dev)
                # deferred to between two segment replays under a SegmentedStep capture
                collective(lambda sa=stats_all, st=stats:
                           dist.all_gather_into_tensor(sa, st, group=group))
        loss = torch.empty((), dtype=torch.float32, device=dev)
        coef = torch.empty(1, dtype=torch.float64, device=dev)
        ops.ce_finish(world, stats_all, loss, coef)
        _ce_label_check(stats_all, dev)
        ctx.save_for_backward(xc, lab, coef, w)
        ctx.meta = (k, lo, hi, x.shape)
        return loss

    @staticmethod
    def backward(ctx, g):
        x, lab, coef, w = ctx.saved_tensors
        k, lo, hi, shape = ctx.meta
        g = g.to(torch.float32).contiguous()
        dx = torch.empty_like(x)
        ops.ce_bwd(x, lab, k, lo, hi, w, coef, g, dx)
        return dx.view(shape), None, None, None, None, None, None


def ce_loss(x, label, digitize_num, rng=(-1.0, 1.0), weights=None, group=None):
    k = int(digitize_num)
    if x.dim() != 2 or x.shape[1] != k:
        raise ValueError(f"CELoss: logits must be (N, {k}), got {tuple(x.shape)}")
    if label.numel() != x.shape[0]:
        raise ValueError(f"CELoss: {label.numel()} labels for {x.shape[0]} rows")
    return CELossFn.apply(x, label, k, float(rng[0]), float(rng[1]), weights, group)

