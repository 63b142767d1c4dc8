"""The GEMMs of every linear layer: y = x W^T + b forward, input gradient, weight gradient and
the bias column sum, for one problem (jmt/functional.py: Rows layouts) or a batch of them
(jmt/grouped.py: stacked buffers, per-group parameter tables).

An Operand is a batch of row-major matrices as jmt_gemm_desc sees one: pointers, leading
dimension, mode, batch stride, K-segment length — and the tensors the pointers point into.  It
is built from tensors (a view, or (tensor, element offset)), never from integers, so whoever
holds an Operand holds its memory.  wgrad() hands those tensors to ops.gemm as `keep`: a
weight gradient queued until the end of the backward pass (ops: stage A / stage B) keeps its
operands alive and stream-ordered by construction; the caller only says whether they stay
intact (`intact`), never which tensors they are.

ops.gemm calls that stay where they are, because they are no linear layer: the attention
core's score / context GEMMs and their backward (functional.AttnCoreFn, attn_forward,
_attn_backward_launch: two batch axes over (sequence, head), no weight, no bias).
"""
from __future__ import annotations

import os
from typing import NamedTuple, Tuple

import torch

from . import functional as F
from . import ops

_fused_bgrad = {"on": os.environ.get("JMT_FUSED_BGRAD", "1") != "0"}


def fused_bgrad_ok(cd) -> bool:
    """Bias gradients as the A row sums of their weight-gradient GEMM (jmt_gemm_desc.dbias_tab,
    16-bit operands only); JMT_FUSED_BGRAD=0 keeps the separate column-sum launches."""
    return _fused_bgrad["on"] and cd in (torch.bfloat16, torch.float16)


# ------------------------------------------------------------------------- operands
STRIDED, TABLE, KCAT, KSEGS = 0, 1, 2, 3


_KEYS = {s: (s, "ld" + s, s + "_mode", "s" + s.upper(), s + "_kseg") for s in "abc"}


class Operand(NamedTuple):
    """mode STRIDED: matrix g at ptrs[0] + g * stride elements;  TABLE: matrix g at ptrs[g];
    KCAT: ONE matrix whose K axis is the concatenation of len(ptrs) segments of kseg;
    KSEGS: matrix g is the K-concatenation of ptrs[g * nseg : (g + 1) * nseg].
    owners[i] is the tensor ptrs[i] points into."""
    ptrs: Tuple[int, ...]
    ld: int
    mode: int
    stride: int
    kseg: int
    owners: tuple

    def args(self, side: str) -> dict:
        """The operand's ops.gemm keywords (side "a", "b" or "c")."""
        p, ld, mode, st, ks = _KEYS[side]
        kw = {p: self.ptrs, ld: self.ld, mode: self.mode, st: (self.stride, 0)}
        if side != "c":
            kw[ks] = self.kseg
        return kw

    def block_stride(self):
        """Element stride between the matrices when they are equally spaced blocks (strided, or
        a table of consecutive ones), else None."""
        if self.mode == STRIDED:
            return self.stride
        es = self.owners[0].element_size()
        d = {q - p for p, q in zip(self.ptrs[:-1], self.ptrs[1:])}
        if self.mode == TABLE and len(d) == 1 and min(d) > 0 and min(d) % es == 0:
            return min(d) // es
        return None

    def matrix(self, i: int) -> torch.Tensor:
        """A tensor that starts at ptrs[i]: the view the operand was built from, or the flat
        tail of the tensor an offset was given into."""
        t = self.owners[i]
        off = (self.ptrs[i] - t.data_ptr()) // t.element_size()
        return t if off == 0 else t.view(-1)[off:]


def _operand(items, ld, mode, stride=0, kseg=0) -> Operand:
    ptrs, owners = [], []
    for x in items:
        t, off = x if isinstance(x, tuple) else (x, 0)
        ptrs.append(t.data_ptr() + off * t.element_size())
        owners.append(t)
    return Operand(tuple(ptrs), ld, mode, stride, kseg, tuple(owners))


def strided(x, ld: int, stride: int = 0) -> Operand:
    """x: a tensor / view, or (tensor, element offset) — as every item below."""
    if type(x) is tuple:
        return Operand((x[0].data_ptr() + x[1] * x[0].element_size(),), ld, STRIDED, stride, 0,
                       x[:1])
    return Operand((x.data_ptr(),), ld, STRIDED, stride, 0, (x,))


def table(items, ld: int) -> Operand:
    """One item: the strided form (one base pointer)."""
    return _operand(items, ld, TABLE) if len(items) > 1 else strided(items[0], ld)


def blocks(items, ld: int) -> Operand:
    """table(items), as a strided operand when the items are equally spaced."""
    op = _operand(items, ld, TABLE)
    s = op.block_stride() if len(items) > 1 else 0
    return op if s is None else op._replace(ptrs=op.ptrs[:1], mode=STRIDED, stride=s)


def kcat(items, ld: int, kseg: int) -> Operand:
    return _operand(items, ld, KCAT, 0, kseg)


def ksegs(groups, ld: int, kseg: int) -> Operand:
    return _operand([x for g in groups for x in g], ld, KSEGS, 0, kseg)


def _weights(W, cd, r0: int):
    """(rows r0.. of the compute-dtype copies as a B operand, Kin, one problem?)."""
    if isinstance(W, torch.Tensor):
        Wc = F.weight_as(W, cd)
        Kin = Wc.shape[1]
        return strided((Wc, r0 * Kin), Kin), Kin, True
    Wc = [F.weight_as(w, cd) for w in W]
    Kin = Wc[0].shape[1]
    es = Wc[0].element_size()
    return Operand(tuple(w.data_ptr() + r0 * Kin * es for w in Wc), Kin, TABLE, 0, 0,
                   tuple(Wc)), Kin, False


# ------------------------------------------------------------------------- grouped launches
def group16_scope():
    """The fwd() / dgrad() calls inside — independent of each other — leave as one grouped launch
    where ops.group16_scope takes them (16-bit, whole 256-row panels, each alone on the ping-pong
    kernel), else exactly as they would outside; their operand tensors are kept until then."""
    return ops.group16_scope()


# ------------------------------------------------------------------------- forward
def fwd(A: Operand, rows: int, W, b, C: Operand, cd, r0: int = 0, n=None, relu: bool = False):
    """C[g] = A[g] (rows x Kin) . W_g[r0:r0+n]^T + b_g[r0:r0+n] (relu).  W / b: one parameter
    (one problem; b may be None) or a list per batch entry (b: a list or None)."""
    Bw, Kin, single = _weights(W, cd, r0)
    n = Bw.owners[0].shape[0] - r0 if n is None else n
    sl = slice(r0, r0 + n)
    bias = {"bias": b[sl] if b is not None else None} if single else \
        {"bias_tab": [t[sl] for t in b] if b is not None else None}
    if A.mode == KCAT and len(A.ptrs) == 1:
        A = A._replace(mode=STRIDED, kseg=0)
    kw = A.args("a")
    if rows == 1:       # a single row: its stride is never used, any 16-B multiple serves
        kw["lda"] = F._vec(cd)
    ops.gemm(M=rows, N=n, K=Kin, ab_dtype=ops.dt(cd), c_dtype=ops.dt(C.owners[0]),
             a_kmajor=True, b_kmajor=True, batch0=1 if single else len(Bw.ptrs), bias_mode=1,
             relu=relu, device=C.owners[0].device, keep=(*A.owners, *Bw.owners, *C.owners),
             **kw, **Bw.args("b"), **C.args("c"), **bias)


# ------------------------------------------------------------------------- input gradient
def dgrad(dY: Operand, rows: int, n: int, W, C: Operand, cd, r0: int = 0, kseg=None,
          beta: float = 0.0, aux=None, ldaux: int = 0, c_in=None):
    """C[g] (+)= dY[g] (rows x n) . W_g[r0:r0+n]  (masked by aux > 0: ReLU backward).
    W: a list of parameters, one per batch entry;  or one parameter, whose Kin columns are cut
    into Kin / kseg batch entries (the K-segments of a concatenated forward; default: one);  or a
    KCAT Operand of weight rows (dY then holds the matching K-segments, or is one matrix over
    their whole K): one matrix product, at most 8 segments per launch, accumulated.
    c_in (with beta != 0): C[g] = beta * c_in[g] + ..., a buffer laid out like C that stays
    intact (jmt_gemm_cin).  Where the planner splits K — the reduce adds into C itself — c_in
    is copied into C first and the launch accumulates in place: the same bits."""
    common = dict(M=rows, ab_dtype=ops.dt(cd), c_dtype=ops.dt(C.owners[0]), b_kmajor=False,
                  aux=aux, ldaux=ldaux, device=C.owners[0].device)
    if isinstance(W, Operand):
        nseg = len(W.ptrs)
        assert dY.mode == KCAT or nseg <= 8
        for c0 in range(0, nseg, 8):
            a = dY._replace(ptrs=dY.ptrs[c0:c0 + 8]) if dY.mode == KCAT else dY
            w = W._replace(ptrs=W.ptrs[c0:c0 + 8])
            ops.gemm(N=W.ld, K=len(w.ptrs) * W.kseg, a_kmajor=True, beta=beta if c0 == 0 else 1.0,
                     keep=(*a.owners, *w.owners, *C.owners), **common, **a.args("a"),
                     **w.args("b"), **C.args("c"))
        return
    Bw, Kin, single = _weights(W, cd, r0)
    N = Kin if kseg is None or not single else kseg
    nb = Kin // N if single else len(Bw.ptrs)
    if single:
        Bw = Bw._replace(stride=N)
    kw = dY.args("a")
    if n == 1:          # dY is a column: read it as an MN-major operand (row stride irrelevant)
        kw["lda"] = F._vec(cd)
    cin = None
    if c_in is not None:
        assert beta != 0.0 and C.mode == STRIDED and C.stride == rows * C.ld and \
            c_in.is_contiguous()
        if ops.auto_splits(rows, N, n, nb, ops.dt(cd)) > 1:
            ops.copy2d(c_in.data_ptr(), ops.dt(c_in), C.ptrs[0], common["c_dtype"], nb * rows, N,
                       C.ld, 1, C.ld, 1)
        else:
            cin = [c_in.data_ptr()]
    ops.gemm(N=N, K=n, a_kmajor=n != 1, batch0=nb, beta=beta, c_in=cin,
             ldcin=C.ld if c_in is not None else 0, keep=(*dY.owners, *Bw.owners, *C.owners),
             **common, **kw, **Bw.args("b"), **C.args("c"))


# ------------------------------------------------------------------------- weight gradient
def wgrad(dY: Operand, X: Operand, rows: int, n: int, W, cd, b=None, r0: int = 0, kseg=None,
          intact: bool = False, defer: bool = False, queue: bool = True,
          fallback: bool = True) -> bool:
    """W_g.grad[r0:r0+n] += dY[g]^T X[g]  (fp32, split-K over the rows; KSEGS operands: rows per
    segment, summed over a group's segments), and with biases b_g.grad[r0:r0+n] += the column
    sums of dY[g]: inside the same GEMM (its A row sums) when n > 1 and fused_bgrad_ok(cd) —
    the return value — else, with `fallback`, by bias_grad() right after the launch.
    W / b: a list per batch entry (distinct parameters: their regions are written concurrently;
    a None bias entry: no bias gradient for that group; a frozen W or b: written to scratch);
    or one parameter, whose Kin columns are cut into Kin / kseg batch entries that share dY (only
    entry 0 sums it; a frozen W: nothing is launched, a frozen b: no sums).
    intact: nothing writes dY or X again before the backward pass ends — the launch may be held
    for the end-of-backward group (ops: stage B) where functional.wgrad_defer_ok(cd).  defer:
    stage A, for the backward's last launches.  queue=False: launched now, whatever the queue."""
    single = isinstance(W, torch.Tensor)
    Ws, bs = ((W,), None if b is None else (b,)) if single else (W, b)
    dev = dY.owners[0].device
    Kin = Ws[0].shape[1]
    grads = []
    for w in Ws:
        g = F._grad_buffer(w)
        if g is None and single:
            if fallback and b is not None:
                bias_grad(dY, rows, n, bs, r0)
            return False
        grads.append(g if g is not None else torch.zeros_like(w))
    dbt = None
    if bs is not None and n > 1 and fused_bgrad_ok(cd):
        dbt = []
        for t in bs:
            gb = F._grad_buffer(t)
            dbt.append(None if t is None else gb[r0:r0 + n] if gb is not None else
                       None if single else torch.empty(n, dtype=torch.float32, device=dev))
        if single:
            dbt = dbt + [None] * (Kin // (kseg or Kin) - 1) if gb is not None else None
    if single:
        N = kseg or Kin
        Cg, nb = strided((grads[0], r0 * Kin), Kin, N), Kin // N
    else:
        N, nb = Kin, len(Ws)
        Cg = _operand([(g, r0 * Kin) for g in grads], Kin, TABLE)
    nseg = len(dY.ptrs) // nb if dY.mode == KSEGS else 1

    def done():
        F._grad_done(*Ws)
        if dbt is not None:
            F._grad_done(*bs)

    kw = dY.args("a")
    if n == 1:          # the single row of dY^T is the contiguous dY column (K-major)
        kw["lda"] = F._vec(cd)
    ops.gemm(M=n, N=N, K=nseg * rows, ab_dtype=ops.dt(cd), c_dtype=ops.F32, a_kmajor=n == 1,
             b_kmajor=False, batch0=nb, beta=1.0, dbias_tab=dbt, device=dev,
             done=done if queue else None,
             keep=(*dY.owners, *X.owners, *grads, *(t for t in dbt or () if t is not None)),
             defer="late" if intact and F.wgrad_defer_ok(cd) else
             defer if F.wgrad_group_ok() else False,
             **kw, **X.args("b"), **Cg.args("c"))
    if not queue:
        done()
    if dbt is None and fallback and bs is not None:
        bias_grad(dY, rows, n, bs, r0)
    return dbt is not None


def bias_grad(dY: Operand, rows: int, n: int, bs, r0: int = 0):
    """b_g.grad[r0:r0+n] += the column sums of dY[g] (rows x n; KSEGS: of every segment): one
    grouped launch pair for several equally spaced blocks (the bs must be distinct parameters),
    else one column sum per matrix.  A None entry is skipped."""
    G = len(bs)
    sdy = dY.block_stride()
    if G > 1 and sdy is not None and dY.mode != KSEGS and all(t is not None for t in bs):
        dbs = []
        for t in bs:
            gb = F._grad_buffer(t)
            dbs.append(gb[r0:r0 + n] if gb is not None else
                       torch.empty(n, dtype=torch.float32, device=dY.owners[0].device))
        ops.colsum_grouped(dY.ptrs[0], ops.dt(dY.owners[0]), G, dY.ld, sdy, rows, n, dbs,
                           beta_acc=True, device=dY.owners[0].device)
        F._grad_done(*bs)
        return
    nseg = len(dY.ptrs) // G if dY.mode == KSEGS else 1
    for i in range(G * nseg):
        t = bs[i // nseg]
        gb = F._grad_buffer(t)
        if gb is not None:
            ops.colsum(dY.matrix(i), dY.ld, rows, n, gb[r0:r0 + n], beta_acc=True)
            F._grad_done(t)
