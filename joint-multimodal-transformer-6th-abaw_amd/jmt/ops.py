"""Thin, typed wrappers over the C-ABI: torch tensors in, kernel launches on the current HIP
stream out.  No math happens here — every op is one (or a few) libjmt_hip.so launches."""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Optional, Sequence

import torch

from . import _lib
from ._lib import BF16, F16, F32, GemmDesc

_DT = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}


def dt(t_or_dtype) -> int:
    d = t_or_dtype if isinstance(t_or_dtype, torch.dtype) else t_or_dtype.dtype
    try:
        return _DT[d]
    except KeyError:
        raise _lib.JMTError(f"unsupported dtype {d}") from None


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _require_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.JMTError("JMT HIP ops need device tensors (there is no CPU path)")


def workspace(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


# ------------------------------------------------------------------------------------ GEMM
_launch_hook = None


def set_launch_hook(hook) -> None:
    """hook(info: dict, launch: callable) -> result; used by bench.py to bracket launches of one
    GEMM instance with HIP events on the launch stream.  None disables."""
    global _launch_hook
    _launch_hook = hook


def auto_splits(M: int, N: int, K: int, batch: int, ab_dtype: int) -> int:
    """Split-K factor from the library's GEMM planner (jmt_gemm_plan_splits)."""
    return int(_lib.load().jmt_gemm_plan_splits(ab_dtype, M, N, K, batch))


def gemm(*, M: int, N: int, K: int, ab_dtype: int, c_dtype: int,
         a: Sequence[int], lda: int, a_kmajor: bool,
         b: Sequence[int], ldb: int, b_kmajor: bool,
         c: Sequence[int], ldc: int,
         a_mode: int = 0, b_mode: int = 0, c_mode: int = 0, a_kseg: int = 0, b_kseg: int = 0,
         batch0: int = 1, batch1: int = 1, sA=(0, 0), sB=(0, 0), sC=(0, 0),
         alpha: float = 1.0, beta: float = 0.0, bias: Optional[torch.Tensor] = None,
         bias_mode: int = 1, relu: bool = False, aux: Optional[torch.Tensor] = None,
         ldaux: int = 0, splits: Optional[int] = None, bias_tab=None, dbias_tab=None,
         dbias_acc: bool = True, device=None, done=None, keep=(), defer: bool = False,
         c_in: Optional[Sequence[int]] = None, ldcin: int = 0) -> None:
    """dbias_tab: per-b0 fp32 outputs (None: skip that entry) that receive (dbias_acc: += ) the
    row sums of A — a weight-gradient GEMM's bias gradient (jmt_gemm_desc ABI 4).
    c_in / ldcin: the epilogue's beta * C operand comes from this table (parallel to `c`, its own
    leading dimension) and C is only written (jmt_gemm_cin: 16-bit C, no split-K).
    done: called once the launch is enqueued (a weight gradient's completion report).  A launch
    with `done` may be held in the weight-gradient queue (wgrad_scope, or with defer=True /
    defer="late" — stage A / stage B below — until the end of the running backward pass) and
    flushed with its neighbours as one jmt_gemm_grouped launch; `keep` are the tensors its
    operands live in.  A launch without `done` issued inside a group16_scope is collected until
    the scope's exit (one jmt_gemm_group16 launch, or this launch as it is), with its `keep`."""
    d = GemmDesc()
    d.ab_dtype, d.c_dtype = ab_dtype, c_dtype
    d.aux_dtype = dt(aux) if aux is not None else c_dtype
    d.M, d.N, d.K = M, N, K
    for i, p in enumerate(a):
        d.a[i] = p
    for i, p in enumerate(b):
        d.b[i] = p
    for i, p in enumerate(c):
        d.c[i] = p
    d.n_a, d.n_b, d.n_c = len(a), len(b), len(c)
    d.a_mode, d.b_mode, d.c_mode = a_mode, b_mode, c_mode
    d.a_kseg, d.b_kseg = a_kseg, b_kseg
    d.a_kmajor, d.b_kmajor = int(a_kmajor), int(b_kmajor)
    d.lda, d.ldb, d.ldc, d.ldaux = lda, ldb, ldc, ldaux
    d.batch0, d.batch1 = batch0, batch1
    d.sA0, d.sA1 = sA
    d.sB0, d.sB1 = sB
    d.sC0, d.sC1 = sC
    d.alpha, d.beta = alpha, beta
    d.bias = bias.data_ptr() if bias is not None else None
    d.bias_mode = bias_mode if (bias is not None or bias_tab) else 0
    if bias_tab:
        for i, t in enumerate(bias_tab):
            d.bias_tab[i] = t.data_ptr()
        d.n_bias = len(bias_tab)
    d.relu = int(relu)
    d.aux = aux.data_ptr() if aux is not None else None
    if dbias_tab:
        for i, t in enumerate(dbias_tab):
            d.dbias_tab[i] = t.data_ptr() if t is not None else None
        d.n_dbias = len(dbias_tab)
        d.dbias_acc = int(dbias_acc)
    fam = {(True, True): "gemm_NT", (True, False): "gemm_NN", (False, False): "gemm_TN",
           (False, True): "gemm_TT"}[(bool(a_kmajor), bool(b_kmajor))]
    info = {"family": fam, "ab_dtype": ab_dtype, "c_dtype": c_dtype,
            "a_kmajor": bool(a_kmajor), "b_kmajor": bool(b_kmajor), "M": M, "N": N,
            "K": K, "batch": batch0 * batch1, "beta": beta,
            "dbias": bool(dbias_tab),
            "flops": 2.0 * M * N * K * batch0 * batch1,
            "bytes": batch0 * batch1 * ((M + N) * K * (4 if ab_dtype == F32 else 2) +
                                        M * N * (4 if c_dtype == F32 else 2)),
            "inplace": any(p in list(c) for p in list(a) + list(b))}

    def single():
        sp = splits if splits is not None else auto_splits(M, N, K, batch0 * batch1, ab_dtype)
        d.splits = sp
        ws = None
        if sp > 1:
            nbytes = _lib.load().jmt_gemm_workspace_bytes(M, N, batch0 * batch1, sp)
            if dbias_tab:
                # the A row sums' split partials after the slabs (16-B aligned: the slab bytes are)
                dbytes = sp * batch0 * M * 4
                ws = workspace(nbytes + dbytes, device)
                d.dbias_ws = ws.data_ptr() + nbytes
                d.dbias_ws_bytes = dbytes
            else:
                ws = workspace(nbytes, device)
            d.workspace = ws.data_ptr()
            d.ws_bytes = nbytes
        if c_in is not None:
            tab = (C.c_void_p * len(c_in))(*c_in)
            launch = lambda: _lib.check(_lib.load().jmt_gemm_cin(
                C.byref(d), tab, len(c_in), ldcin or ldc, stream()), "jmt_gemm_cin")
        else:
            launch = lambda: _lib.check(_lib.load().jmt_gemm(C.byref(d), stream()), "jmt_gemm")
        if _launch_hook is not None:
            _launch_hook(info, launch)
        else:
            launch()
        return ws   # keep alive until the launch is ordered (caching allocator is stream-ordered)

    if done is not None and splits is None and _wgrad_enqueue(
            _WgradEntry(d, info, single, done, tuple(keep), device), defer):
        return None
    if done is None and _g16["depth"] > 0:
        # (splits as single() would set them: what the group's checks and the planner see)
        sp = splits if splits is not None else auto_splits(M, N, K, batch0 * batch1, ab_dtype)
        _g16["ents"].append((d, info, single, sp, c_in is not None, tuple(keep)))
        return None
    ws = single()
    if done is not None:
        done()
    return ws


# ------------------------------------------------------------------ grouped weight gradients
# The step's weight gradients are few 256 x 256 tiles over a long K each: launched one by one,
# every launch spreads its tiles over a full grid of split-K items and pays a slab set and a
# reduce launch of its own.  Launches are queued instead and flushed as jmt_gemm_grouped launches
# (+ one reduce each).  JMT_WGRAD_GROUP=0: every launch as before.
#
# Who is queued (rounds 8 and 11):
#   stage A  launches that already sit next to each other: the calls inside a wgrad_scope(),
#            and the backward's last three (defer=True), flushed by an end-of-backward callback;
#   stage B  every weight gradient whose operands are left intact until the end of the backward
#            (defer="late"): held with the stage-A entries and flushed with them as ONE group.
# JMT_WGRAD_DEFER=0 switches stage B off (stage A as before); JMT_WGRAD_DEFER=single holds the
# stage-B entries to the end of the backward but launches what stage A launches, unit by unit —
# the same launches as JMT_WGRAD_DEFER=0, only later, so an operand overwritten before the flush
# shows as a bitwise difference.
_wgrad_group = {"on": os.environ.get("JMT_WGRAD_GROUP", "1") != "0"}
_wgrad_defer = {"mode": {"0": "off", "single": "single"}.get(
    os.environ.get("JMT_WGRAD_DEFER", "1"), "on")}


def wgrad_group_enabled() -> bool:
    return _wgrad_group["on"]


def wgrad_defer_mode() -> str:
    """'off', 'single' or 'on' (JMT_WGRAD_DEFER); 'off' without grouping."""
    return _wgrad_defer["mode"] if _wgrad_group["on"] else "off"


class _WgradEntry:
    __slots__ = ("d", "info", "single", "done", "keep", "device", "stream")

    def __init__(self, d, info, single, done, keep, device, stream=None):
        self.d, self.info, self.single, self.done = d, info, single, done
        self.keep, self.device = keep, device
        self.stream = stream if stream is not None else torch.cuda.current_stream()


# deferred: the units held for the end-of-backward callback, in program order.  A unit is
# (kind, entries): "tail" a stage-A deferred entry, "scope" the entries of one wgrad_scope,
# "late" a stage-B entry.
_wq = {"depth": 0, "scoped": [], "deferred": [], "task": None, "scope_defer": False}


def _wgrad_hold(kind: str, ents) -> bool:
    """Queue a unit for the end-of-backward flush; False outside a backward pass."""
    task = torch._C._current_graph_task_id()
    if task < 0:                        # outside a backward pass: nothing would flush it
        return False
    if _wq["task"] != task:             # (a backward that raised cannot leave stale entries)
        _wq["deferred"].clear()
        _wq["task"] = task

        def _cb():
            _wq["task"] = None
            units, _wq["deferred"] = _wq["deferred"], []
            _wgrad_flush_units(units)

        torch.autograd.Variable._execution_engine.queue_callback(_cb)
    _wq["deferred"].append((kind, list(ents)))
    return True


def _wgrad_flush_units(units) -> None:
    if wgrad_defer_mode() == "on":      # stage B: everything as one flush
        wgrad_flush([e for _, ents in units for e in ents])
        return
    # stage A's launches: every scope as its own flush, every stage-B entry alone, the stage-A
    # tail together and last (where it already ran)
    tail = []
    for kind, ents in units:
        if kind == "tail":
            tail += ents
        else:
            wgrad_flush(ents)
    wgrad_flush(tail)


def _wgrad_enqueue(e: "_WgradEntry", defer) -> bool:
    if not _wgrad_group["on"]:
        return False
    if _wq["depth"] > 0:
        _wq["scoped"].append(e)
        return True
    if defer == "late":
        return wgrad_defer_mode() != "off" and _wgrad_hold("late", [e])
    if not defer:
        return False
    return _wgrad_hold("tail", [e])


class wgrad_scope:
    """Weight-gradient launches issued inside (ops.gemm with `done`) are flushed together at the
    exit, on the stream current there: for launches that already sit next to each other.
    defer: with stage B on, the entries are held for the end-of-backward flush instead (their
    operands must stay intact until then)."""

    def __init__(self, defer: bool = False):
        self.defer = bool(defer)

    def __enter__(self):
        if _wq["depth"] == 0:
            _wq["scope_defer"] = self.defer
        _wq["depth"] += 1
        return self

    def __exit__(self, et, ev, tb):
        _wq["depth"] -= 1
        if _wq["depth"] == 0:
            ents, _wq["scoped"] = _wq["scoped"], []
            if et is None:
                if not (_wq["scope_defer"] and wgrad_defer_mode() != "off" and
                        _wgrad_hold("scope", ents)):
                    wgrad_flush(ents)
        return False


def _out_ranges(d):
    """The byte ranges [lo, hi) a queued problem writes: C per batch entry and the dbias rows."""
    nb = max(int(d.batch0), 1)
    span = ((d.M - 1) * d.ldc + d.N) * 4
    out = []
    for b in range(nb):
        lo = d.c[b] if d.c_mode == 1 else d.c[0] + b * d.sC0 * 4
        out.append((lo, lo + span))
    for b in range(min(int(d.n_dbias), nb)):
        if d.dbias_tab[b]:
            out.append((d.dbias_tab[b], d.dbias_tab[b] + d.M * 4))
    return out


def _overlaps(ra, rb) -> bool:
    return any(a0 < b1 and b0 < a1 for a0, a1 in ra for b0, b1 in rb)


def wgrad_partition(entries):
    """(groups, rest): the entries jmt_gemm_grouped takes (jmt_gemm_grouped_plan says so per
    entry) as groups of up to 16 problems of one dtype / layout / device within the pointer pool,
    the others in `rest`.  Two problems of one launch read-modify-write their outputs
    concurrently, so an entry whose C or dbias ranges overlap an earlier entry's goes into a
    later launch than that entry's (the two halves of a module outside the K-concat path,
    beta = 1 onto the same rows).  A pure host function."""
    lib = _lib.load()
    groups, rest = [], []
    for e in entries:
        e.d.splits = 0
        if lib.jmt_gemm_grouped_plan(C.byref(e.d), 1, None) != _lib.OK:
            rest.append(e)
            continue
        key = (e.d.ab_dtype, e.d.a_kmajor, e.d.b_kmajor, e.device)
        rng = _out_ranges(e.d)
        first = 0                       # the first group after every overlapping earlier entry
        for gi, g in enumerate(groups):
            if any(_overlaps(rng, r) for r in g[2]):
                first = gi + 1
        for g in groups[first:]:
            if g[0] == key and len(g[1]) < 16 and \
                    sum(x.d.n_a + x.d.n_b + x.d.n_c + x.d.n_dbias for x in g[1] + [e]) <= 216:
                g[1].append(e)
                g[2].append(rng)
                break
        else:
            groups.append((key, [e], [rng]))
    out = []
    for _, ents, _ in groups:
        if len(ents) == 1:
            rest.append(ents[0])
        else:
            out.append(ents)
    return out, rest


def wgrad_flush(entries) -> None:
    """Launch the queued weight gradients on the current stream: those the grouped form takes as
    grouped launches (wgrad_partition), the rest (the 128-row regressor gradient, fp32 compute,
    ...) through jmt_gemm as before; then report every entry done."""
    if not entries:
        return
    lib = _lib.load()
    cur = torch.cuda.current_stream()
    for st in {e.stream for e in entries}:
        if st != cur:                   # operands written on a branch stream
            cur.wait_stream(st)
    groups, rest = wgrad_partition(entries)
    for ents in groups:
        n = len(ents)
        arr = (GemmDesc * n)(*[e.d for e in ents])
        nbytes = lib.jmt_gemm_grouped_workspace_bytes(arr, n)
        ws = workspace(nbytes, ents[0].device)
        launch = lambda: _lib.check(lib.jmt_gemm_grouped(arr, n, ws.data_ptr(), nbytes, stream()),
                                    "jmt_gemm_grouped")
        if _launch_hook is not None:
            info = dict(ents[0].info, grouped=n,
                        flops=sum(e.info["flops"] for e in ents),
                        bytes=sum(e.info["bytes"] for e in ents),
                        dbias=any(e.info["dbias"] for e in ents))
            _launch_hook(info, launch)
        else:
            launch()
    for e in rest:
        e.single()
    for e in entries:
        e.done()
        if e.stream != cur:
            for t in e.keep:
                if isinstance(t, torch.Tensor) and t.is_cuda:
                    t.record_stream(cur)


def gemm_grouped(descs, device, splits_out=None):
    """jmt_gemm_grouped on GemmDesc structures (tests, probes): returns the workspace."""
    lib = _lib.load()
    n = len(descs)
    arr = (GemmDesc * n)(*descs)
    if splits_out is not None:
        sp = (C.c_int * n)()
        _lib.check(lib.jmt_gemm_grouped_plan(arr, n, sp), "jmt_gemm_grouped_plan")
        splits_out[:] = list(sp)
    nbytes = lib.jmt_gemm_grouped_workspace_bytes(arr, n)
    ws = workspace(nbytes, device)
    _lib.check(lib.jmt_gemm_grouped(arr, n, ws.data_ptr(), nbytes, stream()), "jmt_gemm_grouped")
    return ws


# ------------------------------------------------------------------ grouped 16-bit-C GEMMs
# Forward / input-gradient launches that sit next to each other and do not depend on each other
# (the cross-attention block's query and key / value projections; its three stream gradients)
# as ONE jmt_gemm_group16 launch: each alone leaves part of the persistent grid idle in its last
# round and pays its own pipeline fill.  JMT_GEMM_GROUP16=0: every launch as before.
_group16 = {"on": os.environ.get("JMT_GEMM_GROUP16", "1") != "0"}
_g16 = {"depth": 0, "ents": []}


def gemm_group16(descs, check_only: bool = False) -> int:
    """jmt_gemm_group16 on GemmDesc structures, on the current stream; check_only: the code of
    jmt_gemm_group16_ok, nothing is launched."""
    lib = _lib.load()
    n = len(descs)
    arr = (GemmDesc * n)(*descs)
    if check_only:
        return int(lib.jmt_gemm_group16_ok(arr, n))
    _lib.check(lib.jmt_gemm_group16(arr, n, stream()), "jmt_gemm_group16")
    return _lib.OK


class group16_scope:
    """ops.gemm calls issued inside (forward / input-gradient launches: no `done`) are collected
    and launched at the exit, on the stream current there: as one jmt_gemm_group16 launch when
    the group takes them AND each of them alone would run unsplit on the ping-pong kernel
    (jmt_gemm_persist_cfg == 45: the grouped launch then has the bits of the launches it
    replaces); otherwise one by one, in the order and form they were issued in.  The calls must
    not depend on each other's results."""

    def __enter__(self):
        _g16["depth"] += 1
        return self

    def __exit__(self, et, ev, tb):
        _g16["depth"] -= 1
        if _g16["depth"] == 0:
            ents, _g16["ents"] = _g16["ents"], []
            if et is None:
                _group16_flush(ents)
        return False


def _group16_flush(ents) -> None:
    if not ents:
        return
    lib = _lib.load()
    n = len(ents)
    ok = _group16["on"] and 2 <= n <= 8 and not any(e[4] for e in ents)
    if ok:
        for d, _, _, sp, _, _ in ents:
            d.splits = sp
            ok = ok and sp <= 1 and lib.jmt_gemm_persist_cfg(C.byref(d)) == 45
    if ok:
        arr = (GemmDesc * n)(*[e[0] for e in ents])
        ok = lib.jmt_gemm_group16_ok(arr, n) == _lib.OK
    if not ok:
        for e in ents:
            e[2]()
        return
    launch = lambda: _lib.check(lib.jmt_gemm_group16(arr, n, stream()), "jmt_gemm_group16")
    if _launch_hook is not None:
        info = dict(ents[0][1], grouped=n, flops=sum(e[1]["flops"] for e in ents),
                    bytes=sum(e[1]["bytes"] for e in ents))
        _launch_hook(info, launch)
    else:
        launch()


# ------------------------------------------------------------------------------------ rows

def l2norm_fwd(x2: torch.Tensor, ldx: int, rows: int, D: int, y2: torch.Tensor, ldy: int,
               inv_norm: torch.Tensor, eps: float):
    _require_cuda(x2, y2)
    _lib.call("jmt_l2norm_fwd", dt(x2), dt(y2), rows, D, x2.data_ptr(), ldx, y2.data_ptr(), ldy,
              inv_norm.data_ptr(), eps, stream())


def l2norm_bwd(x2, ldx, dy2, lddy, inv_norm, eps, dx2, lddx, rows, D):
    _lib.call("jmt_l2norm_bwd", dt(x2), dt(dy2), dt(dx2), rows, D, x2.data_ptr(), ldx,
              dy2.data_ptr(), lddy, inv_norm.data_ptr(), eps, dx2.data_ptr(), lddx, stream())


def layernorm_fwd(x, ldx, r, ldr, gamma, beta, eps, y, ldy, mean, rstd, rows, D):
    _lib.call("jmt_layernorm_fwd", dt(x), dt(y), rows, D, x.data_ptr(), ldx,
              r.data_ptr() if r is not None else None, ldr, gamma.data_ptr(), beta.data_ptr(),
              eps, y.data_ptr(), ldy, mean.data_ptr(), rstd.data_ptr(), stream())


def layernorm_bwd(x, ldx, r, ldr, dy, lddy, mean, rstd, gamma, dx, lddx, dgamma, dbeta,
                  beta_acc, rows, D):
    nblk = _lib.load().jmt_layernorm_bwd_blocks(rows)
    part = torch.empty(max(nblk, 1) * 2 * D, dtype=torch.float32, device=x.device)
    _lib.call("jmt_layernorm_bwd", dt(x), dt(dy), dt(dx), rows, D, x.data_ptr(), ldx,
              r.data_ptr() if r is not None else None, ldr, dy.data_ptr(), lddy,
              mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), dx.data_ptr(), lddx,
              dgamma.data_ptr(), dbeta.data_ptr(), int(beta_acc), part.data_ptr(), stream())
    return part


def layernorm_bwd_dsum(x, ldx, r, ldr, dy, lddy, mean, rstd, gamma, dx, lddx, dgamma, dbeta,
                       dsum, beta_acc, rows, D):
    """layernorm_bwd plus dsum (+)= column sums of dx; returns the partials buffer, or None when
    the shape is not covered (nothing written: the caller reduces dsum itself)."""
    nblk = _lib.load().jmt_layernorm_bwd_blocks(rows)
    part = torch.empty(max(nblk, 1) * 3 * D, dtype=torch.float32, device=x.device)
    rc = _lib.load().jmt_layernorm_bwd_dsum(
        dt(x), dt(dy), dt(dx), rows, D, x.data_ptr(), ldx,
        r.data_ptr() if r is not None else None, ldr, dy.data_ptr(), lddy, mean.data_ptr(),
        rstd.data_ptr(), gamma.data_ptr(), dx.data_ptr(), lddx, dgamma.data_ptr(),
        dbeta.data_ptr(), dsum.data_ptr(), int(beta_acc), part.data_ptr(), stream())
    if rc == _lib.ERR_UNSUPPORTED:
        return None
    _lib.check(rc, "jmt_layernorm_bwd_dsum")
    return part


def _ptr_array(ts):
    arr = (C.c_void_p * len(ts))(*[t.data_ptr() if t is not None else None for t in ts])
    return arr


def layernorm_fwd_grouped(X, R, gammas, betas, eps, Y, mean, rstd):
    """Y[g] = LayerNorm(X[g] (+ R[g])) with (gammas[g], betas[g]) for the G groups of the stacked
    (G, rows, D) tensors in one launch; mean / rstd (G * rows).  False when the shape is not
    covered (nothing written: the caller runs the groups one by one)."""
    G, D = X.shape[0], X.shape[-1]
    rows = X[0].numel() // D
    ga, be = _ptr_array(gammas), _ptr_array(betas)
    rc = _lib.load().jmt_layernorm_fwd_grouped(
        dt(X), dt(Y), G, rows, D, X.data_ptr(), D, X[0].numel(),
        R.data_ptr() if R is not None else None, D, R[0].numel() if R is not None else 0,
        ga, be, eps, Y.data_ptr(), D, Y[0].numel(), mean.data_ptr(), rstd.data_ptr(), stream())
    if rc == _lib.ERR_UNSUPPORTED:
        return False
    _lib.check(rc, "jmt_layernorm_fwd_grouped")
    return True


def layernorm_bwd_grouped(X, R, dY, mean, rstd, gammas, dX, dgammas, dbetas, dsums, beta_acc):
    """Grouped jmt_layernorm_bwd(_dsum) over the stacked (G, rows, D) tensors: one launch + one
    reduce; dsums None or a list of column-sum outputs.  Returns the partials buffer (keep it
    alive until the launches are ordered) or None when the shape is not covered."""
    G, D = X.shape[0], X.shape[-1]
    rows = X[0].numel() // D
    nblk = _lib.load().jmt_layernorm_bwd_grouped_blocks(rows)
    ns = 3 if dsums is not None else 2
    part = torch.empty(max(nblk, 1) * ns * D * G, dtype=torch.float32, device=X.device)
    rc = _lib.load().jmt_layernorm_bwd_grouped(
        dt(X), dt(dY), dt(dX), G, rows, D, X.data_ptr(), D, X[0].numel(),
        R.data_ptr() if R is not None else None, D, R[0].numel() if R is not None else 0,
        dY.data_ptr(), D, dY[0].numel(), mean.data_ptr(), rstd.data_ptr(), _ptr_array(gammas),
        dX.data_ptr(), D, dX[0].numel(), _ptr_array(dgammas), _ptr_array(dbetas),
        _ptr_array(dsums) if dsums is not None else None, int(beta_acc), part.data_ptr(),
        stream())
    if rc == _lib.ERR_UNSUPPORTED:
        return None
    _lib.check(rc, "jmt_layernorm_bwd_grouped")
    return part


def softmax_fwd(s, lds, rows, n, scale, p, ldp, kr=None, rows_per_seq=1):
    """kr = (int32 {kbeg, kend} table, kr_mod): the softmax over each sequence's key range only
    (row r belongs to sequence r // rows_per_seq), P zero outside it (jmt_softmax_fwd_kr)."""
    if kr is not None:
        _lib.call("jmt_softmax_fwd_kr", dt(p), rows, n, s.data_ptr(), lds, scale, p.data_ptr(),
                  ldp, kr[0].data_ptr(), kr[1], rows_per_seq, stream())
        return
    _lib.call("jmt_softmax_fwd", dt(p), rows, n, s.data_ptr(), lds, scale, p.data_ptr(), ldp,
              stream())


def kpm_ranges(mask, kr, bad):
    """Key range table of an (N, Lk) bool / uint8 key padding mask (True = ignore) into kr
    (int32, 2 N); bad (int32, 1) += rows that are not one non-empty run of valid keys."""
    N, Lk = mask.shape
    assert mask.element_size() == 1 and mask.stride(1) == 1
    _lib.call("jmt_kpm_ranges", N, Lk, mask.data_ptr(), mask.stride(0), kr.data_ptr(),
              bad.data_ptr(), stream())


def softmax_bwd(p, ldp, dp, lddp, rows, n, scale, ds, ldds):
    _lib.call("jmt_softmax_bwd", dt(p), dt(ds), rows, n, p.data_ptr(), ldp, dp.data_ptr(), lddp,
              scale, ds.data_ptr(), ldds, stream())


_attn_fused = {"on": os.environ.get("JMT_ATTN_FUSED", "1") != "0"}


def attn_supported(dtype: int, dh: int) -> bool:
    return _attn_fused["on"] and bool(_lib.load().jmt_attn_supported(dtype, dh))


def _hooked(info, launch):
    if _launch_hook is not None:
        return _launch_hook(info, launch)
    return launch()


def noop():
    _lib.call("jmt_noop", stream())


def _kr_args(kr):
    """(table pointer, kr_mod) of a key range operand kr = (int32 table, kr_mod), or ()."""
    return () if kr is None else (kr[0].data_ptr(), kr[1])


def attn_fwd(dtype, N, H, Lq, Lk, dh, q_ptr, sq, k_ptr, sk, v_ptr, sv, o_ptr, so, scale, lse,
             kr=None):
    """Fused softmax(scale Q K^T) V + lse; sq/sk/sv/so = (row stride, batch stride) in
    elements.  kr = (int32 {kbeg, kend} table, kr_mod): sequence n attends to keys
    [kbeg, kend) of entry n % kr_mod only (jmt_attn_fwd_kr: the whole-row kernel)."""
    name = "jmt_attn_fwd" if kr is None else "jmt_attn_fwd_kr"
    launch = lambda: _lib.call(name, dtype, N, H, Lq, Lk, dh, q_ptr, sq[0], sq[1],
                               k_ptr, sk[0], sk[1], v_ptr, sv[0], sv[1], o_ptr, so[0], so[1],
                               scale, lse.data_ptr() if lse is not None else None,
                               *_kr_args(kr), stream())
    es = 4 if dtype == F32 else 2
    _hooked({"family": "attn_fwd", "flops": 4.0 * N * H * Lq * Lk * dh,
             "bytes": float(N * H) * ((2 * Lq + 2 * Lk) * dh * es + 4 * Lq)}, launch)


def attn_bwd(dtype, N, H, Lq, Lk, dh, go_ptr, sgo, o_ptr, so, q_ptr, sq, k_ptr, sk, v_ptr, sv,
             lse, p, ds, ldp, dq_ptr, sdq, scale, kr=None):
    """P = exp(scale Q K^T - lse) and dS = scale P o (dO V^T - rowsum(dO o O)) written to p / ds
    (ldp), dQ = dS K; dq_ptr None: P and dS only (the 128-row kernel; dQ from attn_dkdv).
    kr: key ranges as attn_fwd (jmt_attn_bwd_kr: dq_ptr None only)."""
    if kr is not None:
        if dq_ptr is not None:
            raise _lib.JMTError("attn_bwd: key ranges need the P / dS form (dq_ptr None)")
        launch = lambda: _lib.call("jmt_attn_bwd_kr", dtype, N, H, Lq, Lk, dh, go_ptr, sgo[0],
                                   sgo[1], o_ptr, so[0], so[1], q_ptr, sq[0], sq[1], k_ptr, sk[0],
                                   sk[1], v_ptr, sv[0], sv[1], lse.data_ptr(), p.data_ptr(),
                                   ds.data_ptr(), ldp, scale, *_kr_args(kr), stream())
    else:
        launch = lambda: _lib.call("jmt_attn_bwd", dtype, N, H, Lq, Lk, dh, go_ptr, sgo[0],
                                   sgo[1], o_ptr, so[0], so[1], q_ptr, sq[0], sq[1], k_ptr, sk[0],
                                   sk[1], v_ptr, sv[0], sv[1], lse.data_ptr(), p.data_ptr(),
                                   ds.data_ptr(), ldp, dq_ptr, sdq[0], sdq[1], scale, stream())
    # algorithmic: two products per launch — dP and dQ, or (dq_ptr None) the S recompute and dP
    # (cdna_hip_programming.md counts the recompute as one of the backward's five products);
    # bytes: dO, O, Q, K, V, (dQ,) lse and the P / dS rows handed to attn_dkdv
    es = 4 if dtype == F32 else 2
    nrow = 3 if dq_ptr is None else 4
    lw = -(-Lk // 32) * 32 if dq_ptr is None else ldp     # P / dS columns written
    _hooked({"family": "attn_bwd", "flops": 4.0 * N * H * Lq * Lk * dh,
             "bytes": float(N * H) * ((nrow * Lq + 2 * Lk) * dh * es + 4 * Lq +
                                      2 * Lq * lw * es)}, launch)


_attn_dkdv = {"on": os.environ.get("JMT_ATTN_DKDV", "1") != "0"}
# the 128-row P / dS backward kernel with dQ as jmt_attn_dkdv's third product (round 6);
# JMT_ATTN_PDS=0 keeps dQ in the 64-row backward kernel (A/B switch)
_attn_pds = {"on": os.environ.get("JMT_ATTN_PDS", "1") != "0"}


def attn_fwd_rows_ok(N, H, Lq, Lk, sk_l, sv_l) -> bool:
    """jmt_attn_fwd takes the whole-row kernel for these sizes and K / V row strides, so
    attn_fwd_sq accepts them (jmt_attn_fwd_rows_ok; the forward-rows switch included)."""
    return bool(_lib.load().jmt_attn_fwd_rows_ok(N, H, Lq, Lk, sk_l, sv_l))


def attn_bwd_pds_ok(N, H, Lq, Lk, ldp, sk_l, sv_l) -> bool:
    """attn_bwd with dq_ptr None (the 128-row P / dS kernel) takes these sizes and row strides
    (jmt_attn_bwd_pds_ok)."""
    return bool(_lib.load().jmt_attn_bwd_pds_ok(N, H, Lq, Lk, ldp, sk_l, sv_l))


def attn_dkdv_ldp(Lk: int) -> int:
    """P / dS row stride jmt_attn_dkdv reads (whole 128-key tiles)."""
    return (Lk + 127) // 128 * 128


def attn_dkdv_ok(N, H, Lq, Lk, ldp, sgo_l, sq_l, sdk_l, sdv_l, sk_l=0, sdq_l=None) -> bool:
    """attn_dkdv takes these sizes and row strides (jmt_attn_dkdv_ok); sdq_l (with sk_l): the
    launch with dQ."""
    return bool(_lib.load().jmt_attn_dkdv_ok(N, H, Lq, Lk, ldp, sgo_l, sq_l, sk_l, sdk_l, sdv_l,
                                             sdq_l or 0, int(sdq_l is not None)))


def attn_dkdv(dtype, N, H, Lq, Lk, dh, p, ds, ldp, go_ptr, sgo, q_ptr, sq, dk_ptr, sdk, dv_ptr,
              sdv, k_ptr=None, sk=(0, 0), dq_ptr=None, sdq=(0, 0)):
    """dV = P^T dO and dK = dS^T Q per (n, h) from attn_bwd's P / dS (ldp >= attn_dkdv_ldp(Lk));
    with dq_ptr also dQ = dS K (k_ptr: the attention's K operand); one persistent kernel in place
    of two (three) batched GEMMs (off with JMT_ATTN_DKDV=0)."""
    launch = lambda: _lib.call("jmt_attn_dkdv", dtype, N, H, Lq, Lk, dh, p.data_ptr(),
                               ds.data_ptr(), ldp, go_ptr, sgo[0], sgo[1], q_ptr, sq[0], sq[1],
                               k_ptr, sk[0], sk[1], dk_ptr, sdk[0], sdk[1], dv_ptr, sdv[0],
                               sdv[1], dq_ptr, sdq[0], sdq[1], stream())
    # algorithmic: the two (three) products; bytes: P, dS (128-key tiles), dO and Q read once per
    # head, dK and dV written (+ K read per 128-query tile, dS again (32-key chunks), dQ written)
    es = 4 if dtype == F32 else 2
    nprod = 2 if dq_ptr is None else 3
    extra = 0.0 if dq_ptr is None else (Lk + Lq) * dh * es + Lq * (-(-Lk // 32) * 32) * es
    _hooked({"family": "attn_dkdv", "flops": 2.0 * nprod * N * H * Lq * Lk * dh,
             "bytes": float(N * H) * ((2 * Lq + 2 * Lk) * dh * es +
                                      2 * Lq * attn_dkdv_ldp(Lk) * es + extra)}, launch)


# ---- shared queries (jmt_attn_*_sq): sequence n = p spp + b reads the Q of sequence
# qtab[p] spp + b.  The launch records keep the unshared families and algorithmic counts.
def _qtab(qtab):
    return (C.c_int * len(qtab))(*qtab), len(qtab)


def attn_fwd_sq(dtype, N, H, Lq, Lk, dh, q_ptr, sq, k_ptr, sk, v_ptr, sv, o_ptr, so, scale, lse,
                spp, qtab, kr=None):
    """attn_fwd with shared queries (the whole-row kernel: Lq > 64); kr: key ranges as attn_fwd
    (jmt_attn_fwd_sq_kr)."""
    tab, npair = _qtab(qtab)
    name = "jmt_attn_fwd_sq" if kr is None else "jmt_attn_fwd_sq_kr"
    launch = lambda: _lib.call(name, dtype, N, H, Lq, Lk, dh, q_ptr, sq[0], sq[1],
                               k_ptr, sk[0], sk[1], v_ptr, sv[0], sv[1], o_ptr, so[0], so[1],
                               scale, lse.data_ptr() if lse is not None else None, spp, tab,
                               npair, *_kr_args(kr), stream())
    es = 4 if dtype == F32 else 2
    _hooked({"family": "attn_fwd", "flops": 4.0 * N * H * Lq * Lk * dh, "shared_q": True,
             "bytes": float(N * H) * ((2 * Lq + 2 * Lk) * dh * es + 4 * Lq)}, launch)


def attn_bwd_sq(dtype, N, H, Lq, Lk, dh, go_ptr, sgo, o_ptr, so, q_ptr, sq, k_ptr, sk, v_ptr, sv,
                lse, p, ds, ldp, scale, spp, qtab, kr=None):
    """attn_bwd's P / dS form (dq_ptr None) with shared queries; kr: key ranges as attn_fwd
    (jmt_attn_bwd_sq_kr)."""
    tab, npair = _qtab(qtab)
    name = "jmt_attn_bwd_sq" if kr is None else "jmt_attn_bwd_sq_kr"
    launch = lambda: _lib.call(name, dtype, N, H, Lq, Lk, dh, go_ptr, sgo[0],
                               sgo[1], o_ptr, so[0], so[1], q_ptr, sq[0], sq[1], k_ptr, sk[0],
                               sk[1], v_ptr, sv[0], sv[1], lse.data_ptr(), p.data_ptr(),
                               ds.data_ptr(), ldp, scale, spp, tab, npair, *_kr_args(kr),
                               stream())
    es = 4 if dtype == F32 else 2
    lw = -(-Lk // 32) * 32
    _hooked({"family": "attn_bwd", "flops": 4.0 * N * H * Lq * Lk * dh, "shared_q": True,
             "bytes": float(N * H) * ((3 * Lq + 2 * Lk) * dh * es + 4 * Lq +
                                      2 * Lq * lw * es)}, launch)


def attn_dkdv_sq(dtype, N, H, Lq, Lk, dh, p, ds, ldp, go_ptr, sgo, q_ptr, sq, dk_ptr, sdk, dv_ptr,
                 sdv, k_ptr, sk, dq_ptr, sdq, spp, qtab, merge_dq):
    """attn_dkdv (with dQ) on shared queries; merge_dq: one dQ = dS_i K_i + dS_j K_j per query,
    in the first use's rows of dq (the second use's rows are left unwritten)."""
    tab, npair = _qtab(qtab)
    launch = lambda: _lib.call("jmt_attn_dkdv_sq", dtype, N, H, Lq, Lk, dh, p.data_ptr(),
                               ds.data_ptr(), ldp, go_ptr, sgo[0], sgo[1], q_ptr, sq[0], sq[1],
                               k_ptr, sk[0], sk[1], dk_ptr, sdk[0], sdk[1], dv_ptr, sdv[0],
                               sdv[1], dq_ptr, sdq[0], sdq[1], spp, tab, npair, int(merge_dq),
                               stream())
    es = 4 if dtype == F32 else 2
    nq = N // 2 if merge_dq else N        # dQ tensors written
    extra = (Lk + Lq) * dh * es + Lq * (-(-Lk // 32) * 32) * es
    _hooked({"family": "attn_dkdv", "flops": 6.0 * N * H * Lq * Lk * dh, "shared_q": True,
             "merge_dq": bool(merge_dq),
             "bytes": float(N * H) * ((2 * Lq + 2 * Lk) * dh * es +
                                      2 * Lq * attn_dkdv_ldp(Lk) * es + extra) -
                      float((N - nq) * H) * Lq * dh * es}, launch)


def attn_short_ok(dtype: int, dh: int, Lq: int, Lk: int) -> bool:
    """Shapes the one-block-per-sequence fused kernels cover (jmt_attn_short_*: 16-bit, dh = 512,
    Lq, Lk <= 32); off with JMT_ATTN_FUSED=0 or JMT_ATTN_SHORT=0 (A/B switch)."""
    return (_attn_fused["on"] and _attn_short["on"] and
            bool(_lib.load().jmt_attn_short_supported(dtype, dh, Lq, Lk)))


_attn_short = {"on": os.environ.get("JMT_ATTN_SHORT", "1") != "0"}


def attn_short_fwd(dtype, N, H, Lq, Lk, dh, q_ptr, sq, k_ptr, sk, v_ptr, sv, o_ptr, so, scale,
                   lse, kr=None):
    """jmt_attn_fwd's result (o, lse) for Lq, Lk <= 32: one block per (n, h); kr: key ranges as
    attn_fwd (jmt_attn_short_fwd_kr)."""
    name = "jmt_attn_short_fwd" if kr is None else "jmt_attn_short_fwd_kr"
    launch = lambda: _lib.call(name, dtype, N, H, Lq, Lk, dh, q_ptr, sq[0], sq[1],
                               k_ptr, sk[0], sk[1], v_ptr, sv[0], sv[1], o_ptr, so[0], so[1],
                               scale, lse.data_ptr(), *_kr_args(kr), stream())
    es = 4 if dtype == F32 else 2
    _hooked({"family": "attn_short_fwd", "flops": 4.0 * N * H * Lq * Lk * dh,
             "bytes": float(N * H) * ((2 * Lq + 2 * Lk) * dh * es + 4 * Lq)}, launch)


def attn_short_bwd(dtype, N, H, Lq, Lk, dh, go_ptr, sgo, o_ptr, so, q_ptr, sq, k_ptr, sk, v_ptr,
                   sv, lse, dq_ptr, sdq, dk_ptr, sdk, dv_ptr, sdv, scale, kr=None):
    """dQ, dK, dV of attn_short_fwd in one kernel (P recomputed from lse; no P / dS in HBM); kr:
    the forward's key ranges (jmt_attn_short_bwd_kr)."""
    name = "jmt_attn_short_bwd" if kr is None else "jmt_attn_short_bwd_kr"
    launch = lambda: _lib.call(name, dtype, N, H, Lq, Lk, dh, go_ptr, sgo[0],
                               sgo[1], o_ptr, so[0], so[1], q_ptr, sq[0], sq[1], k_ptr, sk[0],
                               sk[1], v_ptr, sv[0], sv[1], lse.data_ptr(), dq_ptr, sdq[0], sdq[1],
                               dk_ptr, sdk[0], sdk[1], dv_ptr, sdv[0], sdv[1], scale,
                               *_kr_args(kr), stream())
    # algorithmic: dP, dQ, dK, dV (the P recompute is not counted); bytes: q, o, dO, k, v, lse
    # read, dq, dk, dv written
    es = 4 if dtype == F32 else 2
    _hooked({"family": "attn_short_bwd", "flops": 8.0 * N * H * Lq * Lk * dh,
             "bytes": float(N * H) * ((4 * Lq + 4 * Lk) * dh * es + 4 * Lq)}, launch)


# the fused multi-head kernels (attn_mh.hip: dh 64 / 128); JMT_ATTN_MH=0 keeps the GEMM + softmax
# path for those head dims (A/B switch)
_attn_mh = {"on": os.environ.get("JMT_ATTN_MH", "1") != "0"}


def attn_mh_ok(dtype: int, dh: int, N: int, H: int, Lq: int, Lk: int, sq_l: int, sk_l: int,
               sv_l: int) -> bool:
    """Shapes the fused multi-head kernels cover (jmt_attn_mh_ok: 16-bit, dh 64 or 128, the
    kernels' size and row stride limits); off with JMT_ATTN_FUSED=0 or JMT_ATTN_MH=0."""
    return (_attn_fused["on"] and _attn_mh["on"] and
            bool(_lib.load().jmt_attn_mh_ok(dtype, dh, N, H, Lq, Lk, sq_l, sk_l, sv_l)))


def _mh_tail(base, kr, drop):
    """Entry point and trailing arguments of a multi-head attention call: `base`, `base`_kr or,
    with drop = (p, counter block), `base`_drop (range table or NULL, kr_mod, p, ctr)."""
    if drop is None:
        return (base if kr is None else base + "_kr"), _kr_args(kr)
    p, ctr = drop
    _require_cuda(ctr)
    return base + "_drop", ((_kr_args(kr) or (None, 1)) + (float(p), ctr.data_ptr()))


def attn_mh_fwd(dtype, N, H, Lq, Lk, dh, q_ptr, sq, k_ptr, sk, v_ptr, sv, o_ptr, so, scale, lse,
                kr=None, drop=None):
    """Flash-attention forward for dh 64 / 128 (o and lse; one block per 64 query rows of an
    (n, h)); kr: key ranges as attn_fwd (jmt_attn_mh_fwd_kr); drop = (p, ctr): dropout on the
    probabilities with the mask of the state copy ctr (jmt_attn_mh_fwd_drop)."""
    name, tail = _mh_tail("jmt_attn_mh_fwd", kr, drop)
    launch = lambda: _lib.call(name, dtype, N, H, Lq, Lk, dh, q_ptr, sq[0], sq[1],
                               k_ptr, sk[0], sk[1], v_ptr, sv[0], sv[1], o_ptr, so[0], so[1],
                               scale, lse.data_ptr() if lse is not None else None,
                               *tail, stream())
    # bytes: q, k, v read, o and lse written
    _hooked({"family": "attn_mh_fwd", "flops": 4.0 * N * H * Lq * Lk * dh,
             "bytes": float(N * H) * ((2 * Lq + 2 * Lk) * dh * 2 + 4 * Lq)}, launch)


def attn_mh_bwd(dtype, N, H, Lq, Lk, dh, go_ptr, sgo, o_ptr, so, q_ptr, sq, k_ptr, sk, v_ptr,
                sv, lse, dq_ptr, sdq, dk_ptr, sdk, dv_ptr, sdv, scale, delta, kr=None,
                drop=None):
    """dQ, dK, dV of attn_mh_fwd: the dQ kernel (which also writes delta = rowsum(dO o O), N H Lq
    floats) and the dK / dV kernel behind one entry point, P recomputed from lse in both, no
    atomics; kr: the forward's key ranges (jmt_attn_mh_bwd_kr); drop: the forward's (p, ctr),
    from which both kernels regenerate its mask (jmt_attn_mh_bwd_drop)."""
    name, tail = _mh_tail("jmt_attn_mh_bwd", kr, drop)
    launch = lambda: _lib.call(name, dtype, N, H, Lq, Lk, dh, go_ptr, sgo[0],
                               sgo[1], o_ptr, so[0], so[1], q_ptr, sq[0], sq[1], k_ptr, sk[0],
                               sk[1], v_ptr, sv[0], sv[1], lse.data_ptr(), dq_ptr, sdq[0], sdq[1],
                               dk_ptr, sdk[0], sdk[1], dv_ptr, sdv[0], sdv[1], scale,
                               delta.data_ptr(), *tail, stream())
    # algorithmic: the five products of a flash backward (S, dP, dV, dK, dQ); bytes: q, k, v, o,
    # dO read, dq, dk, dv written, lse read, delta written
    _hooked({"family": "attn_mh_bwd", "flops": 10.0 * N * H * Lq * Lk * dh,
             "bytes": float(N * H) * ((4 * Lq + 4 * Lk) * dh * 2 + 8 * Lq)}, launch)


SMALL_ATTN_MAX_L = 8


def small_attn_ok(E: int, H: int, Lq: int, Lk: int) -> bool:
    """Shapes jmt_small_attn_* cover (include/jmt.h): E = 512, E/8/H a power of two, L <= 8
    (off with the fused kernels: JMT_ATTN_FUSED=0 selects the GEMM + softmax path)."""
    g = E // 8 // H if H > 0 and E % (8 * H) == 0 else 0
    return (_attn_fused["on"] and E == 512 and g > 0 and (g & (g - 1)) == 0 and 1 <= Lq <= SMALL_ATTN_MAX_L
            and 1 <= Lk <= SMALL_ATTN_MAX_L)


def small_attn_fwd(dtype, N, H, Lq, Lk, E, q_ptr, sq, k_ptr, sk, v_ptr, sv, o_ptr, so, scale,
                   p):
    """O = softmax(scale Q K^T) V for Lq, Lk <= 8, one wave per sequence; p (fp32,
    N*H*Lq*Lk) keeps the probabilities for small_attn_bwd."""
    launch = lambda: _lib.call("jmt_small_attn_fwd", dtype, N, H, Lq, Lk, E, q_ptr, sq[0],
                               sq[1], k_ptr, sk[0], sk[1], v_ptr, sv[0], sv[1], o_ptr, so[0],
                               so[1], scale, p.data_ptr() if p is not None else None, stream())
    es = 4 if dtype == F32 else 2
    nbytes = float(N) * (2 * Lq + 2 * Lk) * E * es + (4.0 * N * H * Lq * Lk if p is not None
                                                       else 0.0)
    _hooked({"family": "small_attn_fwd", "flops": 4.0 * N * Lq * Lk * E, "bytes": nbytes},
            launch)


def small_attn_bwd(dtype, N, H, Lq, Lk, E, go_ptr, sgo, q_ptr, sq, k_ptr, sk, v_ptr, sv, p,
                   dq_ptr, sdq, dk_ptr, sdk, dv_ptr, sdv, scale):
    """dQ, dK, dV of small_attn_fwd from the kept P (no score recompute)."""
    launch = lambda: _lib.call("jmt_small_attn_bwd", dtype, N, H, Lq, Lk, E, go_ptr, sgo[0],
                               sgo[1], q_ptr, sq[0], sq[1], k_ptr, sk[0], sk[1], v_ptr, sv[0],
                               sv[1], p.data_ptr(), dq_ptr, sdq[0], sdq[1], dk_ptr, sdk[0],
                               sdk[1], dv_ptr, sdv[0], sdv[1], scale, stream())
    es = 4 if dtype == F32 else 2
    nbytes = float(N) * (3 * Lq + 4 * Lk) * E * es + 4.0 * N * H * Lq * Lk
    _hooked({"family": "small_attn_bwd", "flops": 8.0 * N * Lq * Lk * E, "bytes": nbytes},
            launch)


def colsum(dy, ld, rows, N, db, beta_acc=False):
    nblk = _lib.load().jmt_colsum_blocks(rows)
    part = torch.empty(max(nblk, 1) * N, dtype=torch.float32, device=dy.device)
    _lib.call("jmt_colsum", dt(dy), rows, N, dy.data_ptr(), ld, db.data_ptr(), int(beta_acc),
              part.data_ptr(), stream())
    return part


def colsum_grouped(dy_ptr: int, dtype: int, G: int, ld: int, sdy: int, rows: int, N: int,
                   dbs, beta_acc=True, device=None):
    """db_g (+)= column sums of the g-th (rows x N) block at dy_ptr + g*sdy, one launch pair."""
    nblk = _lib.load().jmt_colsum_blocks(rows)
    part = torch.empty(max(nblk, 1) * N * G, dtype=torch.float32, device=device)
    tab = (C.c_void_p * 8)(*[d.data_ptr() for d in dbs])
    _lib.call("jmt_colsum_grouped", dtype, G, rows, N, dy_ptr, ld, sdy, tab, int(beta_acc),
              part.data_ptr(), stream())
    return part


def copy2d(src_ptr, src_dt, dst_ptr, dst_dt, rows, cols, src_rs, src_cs, dst_rs, dst_cs,
           accumulate=False):
    _lib.call("jmt_copy2d", src_dt, dst_dt, rows, cols, src_ptr, src_rs, src_cs, dst_ptr, dst_rs,
              dst_cs, int(accumulate), stream())


def cast(src: torch.Tensor, dtype: torch.dtype, out: Optional[torch.Tensor] = None):
    """Contiguous dtype conversion through jmt_copy2d (weight shadows, label upcasts)."""
    _require_cuda(src)
    src = src if src.is_contiguous() else src.contiguous()
    if out is None:
        out = torch.empty(src.shape, dtype=dtype, device=src.device)
    n = src.numel()
    copy2d(src.data_ptr(), dt(src), out.data_ptr(), dt(out), 1, n, n, 1, n, 1)
    return out


# ------------------------------------------------------------------------------------ CCC

def ccc_stats(kind, pred, label, k, ignore, lo, hi, stats):
    n = label.numel()
    _lib.call("jmt_ccc_stats", kind, dt(pred), n, k, pred.data_ptr(), label.data_ptr(), ignore,
              lo, hi, stats.data_ptr(), stream())


def ccc_finish(kind, world, stats_all, bs, eps, loss, coef, add=None):
    """add (fp32 scalar tensor or None): loss = add + this loss, in the same kernel."""
    if add is None:
        _lib.call("jmt_ccc_finish", kind, world, stats_all.data_ptr(), bs, eps, loss.data_ptr(),
                  coef.data_ptr(), stream())
    else:
        _lib.call("jmt_ccc_finish_add", kind, world, stats_all.data_ptr(), bs, eps,
                  add.data_ptr(), loss.data_ptr(), coef.data_ptr(), stream())


def ccc_stats_finish(kind, pred, label, k, ignore, lo, hi, stats, bs, eps, loss, coef, add=None):
    """ccc_stats then ccc_finish(world = 1) on those statistics as one launch
    (jmt_ccc_stats_finish / _add): the same stats, loss and coef."""
    n = label.numel()
    head = (kind, dt(pred), n, k, pred.data_ptr(), label.data_ptr(), ignore, lo, hi,
            stats.data_ptr(), bs, eps)
    if add is None:
        _lib.call("jmt_ccc_stats_finish", *head, loss.data_ptr(), coef.data_ptr(), stream())
    else:
        _lib.call("jmt_ccc_stats_finish_add", *head, add.data_ptr(), loss.data_ptr(),
                  coef.data_ptr(), stream())


HEAD_HID, HEAD_KMAX = 128, 24      # csrc/head.hip


def head_fwd(h, ldh, rows, k, w2, b2, ys, ldy, perm=None):
    """Both regressors' output layers (csrc/head.hip jmt_head_fwd).  perm = (P, Q): memory row r
    of h is stored at row (r mod P) * Q + r div P of ys (jmt_head_fwd_perm)."""
    p = lambda t: t.data_ptr() if t is not None else None
    name, pq = ("jmt_head_fwd", ()) if perm is None else ("jmt_head_fwd_perm", tuple(perm))
    _lib.call(name, dt(h), dt(ys[0]), rows, HEAD_HID, k, h.data_ptr(), ldh,
              w2[0].data_ptr(), w2[1].data_ptr(), p(b2[0]), p(b2[1]), ys[0].data_ptr(),
              ys[1].data_ptr(), ldy, *pq, stream())


def head_bwd(h, ldh, rows, k, w2, gys, ldgy, dh, lddh, dw2, db2, perm=None):
    """dh (ReLU-masked) and += weight / bias gradients of both output layers (jmt_head_bwd).
    perm = (P, Q): gys are read through head_fwd's row map (jmt_head_bwd_perm)."""
    p = lambda t: t.data_ptr() if t is not None else None
    nbytes = _lib.load().jmt_head_bwd_workspace_bytes(rows)
    ws = torch.empty(max(1, nbytes // 4), dtype=torch.float32, device=h.device)
    name, pq = ("jmt_head_bwd", ()) if perm is None else ("jmt_head_bwd_perm", tuple(perm))
    _lib.call(name, dt(h), dt(gys[0]), rows, HEAD_HID, k, h.data_ptr(), ldh,
              w2[0].data_ptr(), w2[1].data_ptr(), gys[0].data_ptr(), gys[1].data_ptr(), ldgy,
              dh.data_ptr(), lddh, p(dw2[0]), p(dw2[1]), p(db2[0]), p(db2[1]), ws.data_ptr(),
              *pq, stream())


# ------------------------------------------------------------------------------------ dropout
# Counter-based regressor dropout (csrc/dropout.h).  State blocks and counters are 4-element
# int32 tensors holding the uint32 words {seed_lo, seed_hi, call, stream}.

def dropout_next(state: torch.Tensor) -> torch.Tensor:
    """A fresh copy of the state block for one forward / backward pair; state.call += 1."""
    _require_cuda(state)
    out = torch.empty(4, dtype=torch.int32, device=state.device)
    _lib.call("jmt_dropout_next", state.data_ptr(), out.data_ptr(), stream())
    return out


def dropout(x, ldx, y, ldy, rows, cols, split, p0, p1, ctr):
    """y = m . x over (rows x cols) (jmt_dropout; y may be x); columns < split use p0."""
    _require_cuda(x, y, ctr)
    _lib.call("jmt_dropout", dt(x), x.data_ptr(), ldx, y.data_ptr(), ldy, rows, cols, split,
              float(p0), float(p1), ctr.data_ptr(), stream())


def dropout_reference(ctr, rows, cols, split, p0, p1):
    """Host only: the (rows, cols) fp32 multipliers of state block `ctr` (4 ints) as a numpy
    array (jmt_dropout_reference)."""
    import numpy as np
    words = (C.c_uint32 * 4)(*[int(v) & 0xFFFFFFFF for v in ctr])
    out = np.empty((rows, cols), dtype=np.float32)
    _lib.call("jmt_dropout_reference", words, rows, cols, split, float(p0), float(p1),
              out.ctypes.data_as(_lib.c_fp))
    return out


def attn_dropout_rate(p) -> float:
    """The rate in effect of attention dropout p: T8 / 256 with T8 = floor(256 p + 1/2)
    (jmt_attn_dropout_rate; no GPU call).  Raises for p outside [0, 1) or with T8 > 255."""
    r = float(_lib.load().jmt_attn_dropout_rate(float(p)))
    if r < 0.0:
        raise _lib.JMTError(f"attention dropout rate {p}: outside [0, 1) or above 255.5 / 256")
    return r


def attn_dropout(x, ldx, y, ldy, NH, Lq, Lk, p, ctr):
    """y = M o x on an (NH Lq, ld) buffer of probabilities or of dP (jmt_attn_dropout: the
    attention mask of state copy ctr; y may be x; out of place the columns [Lk, ldy) become 0)."""
    _require_cuda(x, y, ctr)
    launch = lambda: _lib.call("jmt_attn_dropout", dt(x), x.data_ptr(), ldx, y.data_ptr(), ldy,
                               NH, Lq, Lk, float(p), ctr.data_ptr(), stream())
    es = x.element_size()
    _hooked({"family": "attn_dropout", "flops": 0.0, "bytes": 2.0 * NH * Lq * Lk * es}, launch)


def attn_dropout_reference(ctr, NH, Lq, Lk, p):
    """Host only: the (NH, Lq, Lk) fp32 multipliers of state block `ctr` (4 ints) as a numpy
    array (jmt_attn_dropout_reference)."""
    import numpy as np
    words = (C.c_uint32 * 4)(*[int(v) & 0xFFFFFFFF for v in ctr])
    out = np.empty((NH, Lq, Lk), dtype=np.float32)
    _lib.call("jmt_attn_dropout_reference", words, NH, Lq, Lk, float(p),
              out.ctypes.data_as(_lib.c_fp))
    return out


def head_fwd_drop(h, ldh, rows, k, w2, b2, ys, ldy, p0, p1, ctr, perm=None):
    """head_fwd on the dropout-masked hidden activations (jmt_head_fwd_drop / _perm_drop)."""
    p = lambda t: t.data_ptr() if t is not None else None
    name, pq = ("jmt_head_fwd_drop", ()) if perm is None else \
        ("jmt_head_fwd_perm_drop", tuple(perm))
    _lib.call(name, dt(h), dt(ys[0]), rows, HEAD_HID, k, h.data_ptr(), ldh,
              w2[0].data_ptr(), w2[1].data_ptr(), p(b2[0]), p(b2[1]), ys[0].data_ptr(),
              ys[1].data_ptr(), ldy, *pq, float(p0), float(p1), ctr.data_ptr(), stream())


def head_bwd_drop(h, ldh, rows, k, w2, gys, ldgy, dh, lddh, dw2, db2, p0, p1, ctr, perm=None):
    """head_bwd with the forward's mask regenerated from `ctr` (jmt_head_bwd_drop / _perm_drop)."""
    p = lambda t: t.data_ptr() if t is not None else None
    nbytes = _lib.load().jmt_head_bwd_workspace_bytes(rows)
    ws = torch.empty(max(1, nbytes // 4), dtype=torch.float32, device=h.device)
    name, pq = ("jmt_head_bwd_drop", ()) if perm is None else \
        ("jmt_head_bwd_perm_drop", tuple(perm))
    _lib.call(name, dt(h), dt(gys[0]), rows, HEAD_HID, k, h.data_ptr(), ldh,
              w2[0].data_ptr(), w2[1].data_ptr(), gys[0].data_ptr(), gys[1].data_ptr(), ldgy,
              dh.data_ptr(), lddh, p(dw2[0]), p(dw2[1]), p(db2[0]), p(db2[1]), ws.data_ptr(),
              *pq, float(p0), float(p1), ctr.data_ptr(), stream())


def ce_stats(x, label, k, lo, hi, weights, stats):
    n = x.numel() // k
    _lib.call("jmt_ce_stats", dt(x), n, k, x.data_ptr(), label.data_ptr(), lo, hi,
              weights.data_ptr() if weights is not None else None, stats.data_ptr(), stream())


def ce_finish(world, stats_all, loss, coef):
    _lib.call("jmt_ce_finish", world, stats_all.data_ptr(), loss.data_ptr(), coef.data_ptr(),
              stream())


def ce_bwd(x, label, k, lo, hi, weights, coef, grad_loss, dx):
    n = x.numel() // k
    _lib.call("jmt_ce_bwd", dt(x), n, k, x.data_ptr(), label.data_ptr(), lo, hi,
              weights.data_ptr() if weights is not None else None, coef.data_ptr(),
              grad_loss.data_ptr() if grad_loss is not None else None, dx.data_ptr(), stream())


def ce_labels(label, k, lo, hi):
    out = torch.empty(label.numel(), dtype=torch.int64, device=label.device)
    _lib.call("jmt_ce_labels", label.numel(), k, label.data_ptr(), lo, hi, out.data_ptr(),
              stream())
    return out


def ccc_bwd(kind, pred, label, k, ignore, lo, hi, coef, grad_loss, dpred):
    n = label.numel()
    _lib.call("jmt_ccc_bwd", kind, dt(pred), n, k, pred.data_ptr(), label.data_ptr(), ignore, lo,
              hi, coef.data_ptr(), grad_loss.data_ptr() if grad_loss is not None else None,
              dpred.data_ptr(), stream())


def mask_indices(label: torch.Tensor, ignore: float):
    n = label.numel()
    idx = torch.empty(max(n, 1), dtype=torch.int64, device=label.device)
    cnt = torch.empty(1, dtype=torch.int64, device=label.device)
    _lib.call("jmt_mask_indices", n, label.data_ptr(), ignore, idx.data_ptr(), cnt.data_ptr(),
              stream())
    return idx, cnt


# ------------------------------------------------------------------------------------ SGD

def sgd_step(param, grad, buf, lr, momentum, dampening, weight_decay, nesterov, first,
             grad_scale=1.0, shadow=None, zero_grad=False):
    """zero_grad: grad is zeroed by the same kernel after it is read (jmt_sgd_step_zero)."""
    _lib.call("jmt_sgd_step_zero" if zero_grad else "jmt_sgd_step", param.numel(),
              param.data_ptr(), grad.data_ptr(),
              buf.data_ptr() if buf is not None else None, lr, momentum, dampening, weight_decay,
              int(nesterov), int(first), grad_scale,
              shadow.data_ptr() if shadow is not None else None,
              dt(shadow) if shadow is not None else BF16, stream())
