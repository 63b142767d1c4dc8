"""The whole-row attention forward (csrc/attn.hip attn_fwd_rows_kernel: 128-row items, a wave
owns 16 rows over all 512 head dims, 32-key tiles, one barrier per tile) against an fp32 torch
reference computed from the same rounded inputs, on packed strided layouts (q a slice of an
(Lq, N, 3 E) buffer, k / v slices of an (Lk, N, 2 E) buffer, o a column slot of a larger
NaN-filled buffer).  Tolerances are those of test_gpu_kernels.test_fused_attention_fwd_vs_fp32."""
import contextlib
import functools
import math

import pytest
import torch

from jmt import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
DH = 512
GUARD = 5                     # rows of sentinel past Lq in the destination buffer
SCALE = 1.0 / math.sqrt(DH)


@contextlib.contextmanager
def fwd_rows(on):
    """Force the forward kernel choice in-process: 1 whole-row kernel (for Lq > 64), 0 the 64-row
    kernel."""
    lib = _lib.load()
    lib.jmt_attn_set_fwd_rows(int(on))
    try:
        yield
    finally:
        lib.jmt_attn_set_fwd_rows(-1)


def _reference(qp, kp, vp, H):
    """fp32 O (Lq, N, H * 512) and lse ((n H + h) Lq + l) from the rounded operands."""
    Lq, N = qp.shape[:2]
    Lk = kp.shape[0]
    q4, k4, v4 = (t.float().reshape(t.shape[0], N, H, DH) for t in (qp, kp, vp))
    s = torch.einsum("lnhd,knhd->nhlk", q4, k4) * SCALE
    o = torch.einsum("nhlk,knhd->lnhd", torch.softmax(s, -1), v4).reshape(Lq, N, H * DH)
    assert s.shape == (N, H, Lq, Lk)
    return o, torch.logsumexp(s, -1).reshape(-1)


@functools.lru_cache(maxsize=None)
def _case(cd, Lq, Lk, N, H):
    """Inputs and reference of one shape, computed once and shared by the tests that use it."""
    E = DH * H
    g = torch.Generator(device=DEV).manual_seed(71)
    q = torch.randn(N, Lq, 3 * E, device=DEV, generator=g).to(cd).permute(1, 0, 2)
    kv = torch.randn(N, Lk, 2 * E, device=DEV, generator=g).to(cd).permute(1, 0, 2)
    qp, kp, vp = q[..., E:2 * E], kv[..., :E], kv[..., E:]
    ref, lref = _reference(qp, kp, vp, H)
    return qp, kp, vp, ref, lref


def _run(qp, kp, vp, H, with_lse=True):
    """jmt_attn_fwd into the middle column slot of a NaN-filled (Lq + GUARD, N, 3 E) buffer;
    returns (whole buffer, o view, whole lse buffer)."""
    Lq, N, E = qp.shape
    Lk = kp.shape[0]
    obuf = torch.full((Lq + GUARD, N, 3 * E), float("nan"), device=DEV, dtype=qp.dtype)
    o = obuf[:Lq, :, E:2 * E]
    lse = torch.full((N * H * Lq + GUARD,), float("nan"), device=DEV, dtype=torch.float32)
    ops.attn_fwd(ops.dt(qp), N, H, Lq, Lk, DH, qp.data_ptr(), (qp.stride(0), qp.stride(1)),
                 kp.data_ptr(), (kp.stride(0), kp.stride(1)), vp.data_ptr(),
                 (vp.stride(0), vp.stride(1)), o.data_ptr(), (o.stride(0), o.stride(1)), SCALE,
                 lse if with_lse else None)
    torch.cuda.synchronize()
    return obuf, o, lse


def _check(cd, obuf, o, lse, ref, lref, what=""):
    Lq, N, E = o.shape
    err = (o.float() - ref).abs().max().item()
    tol = (1e-2 if cd == torch.bfloat16 else 2e-3) * max(ref.abs().max().item(), 1.0)
    el = (lse[:lref.numel()] - lref).abs().max().item()
    tl = 1e-3 * max(lref.abs().max().item(), 1.0)
    print(f"{what} o err {err:.3e} (tol {tol:.3e})  lse err {el:.3e} (tol {tl:.3e})")
    assert torch.isfinite(o.float()).all(), "a row below Lq is not finite"
    assert torch.isnan(obuf[Lq:].float()).all(), "guard rows past Lq written"
    assert torch.isnan(obuf[:Lq, :, :E].float()).all(), "left column slot written"
    assert torch.isnan(obuf[:Lq, :, 2 * E:].float()).all(), "right column slot written"
    assert err <= tol, err
    assert torch.isnan(lse[lref.numel():]).all(), "lse written past its end"
    assert el <= tl, el


# Lq just past the dispatch edge (65) and past each 128-row block edge (128, 129, 257), the
# 44-row tail of L = 300 (waves 3-7 of the last item idle); Lk around the 32-key tile and its
# masks (1, 31, 32, 33, 65, 300); two heads; more items than CUs (600: the persistent loop and
# its item-to-item prefetch)
SHAPES = [(65, 33, 2, 1), (129, 1, 2, 1), (128, 32, 1, 1), (300, 300, 3, 1), (257, 65, 2, 1),
          (70, 31, 3, 1), (129, 33, 3, 2), (129, 33, 300, 1)]


@pytest.mark.parametrize("cd", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("Lq,Lk,N,H", SHAPES)
def test_fwd_rows_vs_fp32(cd, Lq, Lk, N, H):
    qp, kp, vp, ref, lref = _case(cd, Lq, Lk, N, H)
    with fwd_rows(1):
        obuf, o, lse = _run(qp, kp, vp, H)
    _check(cd, obuf, o, lse, ref, lref, f"rows {(Lq, Lk, N, H)}")


def test_fwd_rows_lse_null():
    """lse = NULL is accepted: the same O, no log-sum-exp written anywhere."""
    cd = torch.bfloat16
    qp, kp, vp, ref, lref = _case(cd, 129, 33, 3, 2)
    with fwd_rows(1):
        obuf, o, lse = _run(qp, kp, vp, 2, with_lse=False)
        _, o2, _ = _run(qp, kp, vp, 2)
    assert torch.isnan(lse).all()
    assert torch.equal(o, o2)
    assert (o.float() - ref).abs().max().item() <= 1e-2 * max(ref.abs().max().item(), 1.0)


def test_fwd_rows_forced_rescale():
    """The lazy-rescale branch (a row max rising > 8 log2 units) on every 32-key tile of
    Lk = 96: row 7 of sequence 0 meets a key worth ~12 log2 units in tile 1 and one worth ~23 in
    tile 2 (a rescale of live state twice), the single row of the second 128-row item (row 128,
    sequence 1) one in the last tile (cdna_hip_programming.md §5.4 rule 26)."""
    cd = torch.bfloat16
    E, Lq, Lk, N = DH, 129, 96, 2
    g = torch.Generator(device=DEV).manual_seed(72)
    q = torch.randn(N, Lq, E, device=DEV, generator=g) * 0.3
    k = torch.randn(N, Lk, E, device=DEV, generator=g) * 0.3
    v = torch.randn(N, Lk, E, device=DEV, generator=g)
    k[0, 40] = q[0, 7] * 4.0
    k[0, 70] = q[0, 7] * 8.0
    k[1, 95] = q[1, 128] * 8.0
    qp, kp, vp = (t.to(cd).permute(1, 0, 2) for t in (q, k, v))
    s = torch.einsum("lnd,knd->nlk", qp.float(), kp.float()) * SCALE * 1.4426950408889634
    m0, m1, m2 = (s[0, 7, 32 * t:32 * t + 32].max().item() for t in range(3))
    assert m1 > m0 + 8 and m2 > m1 + 8, (m0, m1, m2)         # the branch is taken on each tile
    assert s[1, 128, 64:].max().item() > s[1, 128, :64].max().item() + 8
    ref, lref = _reference(qp, kp, vp, 1)
    with fwd_rows(1):
        obuf, o, lse = _run(qp, kp, vp, 1)
    _check(cd, obuf, o, lse, ref, lref, "forced rescale")
    assert (o[7, 0].float() - vp[70, 0].float()).abs().max().item() <= 2e-2
    assert (o[128, 1].float() - vp[95, 1].float()).abs().max().item() <= 2e-2


def _kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return names or None


def test_fwd_rows_dispatch():
    """Switch on: Lq = 129 launches attn_fwd_rows_kernel, Lq = 64 the 64-row attn_fwd_kernel
    (whose arithmetic the short-sequence kernel reproduces); switch off: the 64-row kernel."""
    cd = torch.bfloat16
    big = _case(cd, 129, 33, 3, 2)[:3]
    g = torch.Generator(device=DEV).manual_seed(73)
    small = [torch.randn(2, 64, DH, device=DEV, generator=g).to(cd).permute(1, 0, 2)
             for _ in range(3)]
    with fwd_rows(1):
        n_big = _kernel_names(lambda: _run(*big, 2))
        n_small = _kernel_names(lambda: _run(*small, 1))
    with fwd_rows(0):
        n_off = _kernel_names(lambda: _run(*big, 2))
    if n_big is None or n_small is None or n_off is None:
        pytest.skip("torch.profiler recorded no device kernels")
    assert any("attn_fwd_rows_kernel" in n for n in n_big), n_big
    assert any("attn_fwd_kernel" in n for n in n_small), n_small
    assert not any("attn_fwd_rows_kernel" in n for n in n_small), n_small
    assert any("attn_fwd_kernel" in n for n in n_off), n_off
    assert not any("attn_fwd_rows_kernel" in n for n in n_off), n_off


@pytest.mark.parametrize("cd", [torch.bfloat16, torch.float16])
def test_fwd_rows_against_64_row_kernel(cd):
    """Both kernels on the same inputs at (300, 300, 3): each inside the fp32 tolerance, their
    lse within the lse tolerance of each other, and the P / dS backward run from the whole-row
    forward's (o, lse) inside the bounds of test_fused_attention_bwd_vs_fp32."""
    Lq, Lk, N, H, E = 300, 300, 3, 1, DH
    qp, kp, vp, ref, lref = _case(cd, Lq, Lk, N, H)
    with fwd_rows(0):
        obuf0, o0, lse0 = _run(qp, kp, vp, H)
    with fwd_rows(1):
        obuf1, o1, lse1 = _run(qp, kp, vp, H)
    _check(cd, obuf0, o0, lse0, ref, lref, "64-row")
    _check(cd, obuf1, o1, lse1, ref, lref, "whole-row")
    dl = (lse1[:N * Lq] - lse0[:N * Lq]).abs().max().item()
    print(f"|lse_rows - lse_64| {dl:.3e}  |o_rows - o_64| "
          f"{(o1.float() - o0.float()).abs().max().item():.3e}")
    assert dl <= 1e-3 * max(lref.abs().max().item(), 1.0)

    g = torch.Generator(device=DEV).manual_seed(74)
    go = torch.randn(Lq, N, E, device=DEV, generator=g).to(cd)
    ldp = ops.attn_dkdv_ldp(Lk)
    P = torch.full((N * Lq * ldp,), float("nan"), device=DEV, dtype=cd)
    dS = torch.full((N * Lq * ldp,), float("nan"), device=DEV, dtype=cd)
    lse = lse1[:N * Lq].contiguous()
    ops.attn_bwd(ops.dt(qp), N, 1, Lq, Lk, E, go.data_ptr(), (go.stride(0), go.stride(1)),
                 o1.data_ptr(), (o1.stride(0), o1.stride(1)), qp.data_ptr(),
                 (qp.stride(0), qp.stride(1)), kp.data_ptr(), (kp.stride(0), kp.stride(1)),
                 vp.data_ptr(), (vp.stride(0), vp.stride(1)), lse, P, dS, ldp, None, (0, 0),
                 SCALE)
    torch.cuda.synchronize()
    s = torch.einsum("lnd,knd->nlk", qp.float(), kp.float()) * SCALE
    pr = torch.softmax(s, -1)
    dp = torch.einsum("lnd,knd->nlk", go.float(), vp.float())
    delta = (go.float() * o1.float()).sum(-1).t().unsqueeze(-1)
    dsr = pr * (dp - delta) * SCALE
    Pg = P.view(N, ldp // 32, Lq, 32).permute(0, 2, 1, 3).reshape(N, Lq, ldp)
    dSg = dS.view(N, ldp // 32, Lq, 32).permute(0, 2, 1, 3).reshape(N, Lq, ldp)
    lw = -(-Lk // 32) * 32
    assert torch.isfinite(Pg[..., :lw].float()).all() and torch.isfinite(dSg[..., :lw].float()).all()
    assert (Pg[..., Lk:lw] == 0).all() and (dSg[..., Lk:lw] == 0).all()
    u = 2.0 ** -8 if cd == torch.bfloat16 else 2.0 ** -11
    e_p = (Pg[..., :Lk].float() - pr).abs().max().item()
    floor = 4 * u * SCALE * dp.abs().max().item()
    e_ds = (dSg[..., :Lk].float() - dsr).abs().max().item()
    print(f"P err {e_p:.3e} (tol {2 * u:.3e})  dS err {e_ds:.3e} "
          f"(tol {8 * u * dsr.abs().max().item() + floor:.3e})")
    assert e_p <= 2 * u
    assert e_ds <= 8 * u * dsr.abs().max().item() + floor, e_ds
