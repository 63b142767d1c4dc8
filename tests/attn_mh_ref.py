"""Shared pieces of the multi-head attention tests (tests/test_gpu_attn_mh*.py): packed inputs,
the entry points on NaN-poisoned buffers, the float64 reference and the project's error bounds.

Layouts as tests/test_gpu_attn_short.py: q is the first E columns of a packed (Lq, N, 3E) view,
k / v the two halves of a packed (Lk, N, 2E) one; dq goes to the MIDDLE slot of a NaN-filled
(Lq, N, 3E) buffer and dk / dv into a NaN-filled (Lk, N, 2E) one.  E = 512, head h at columns
h * dh."""
import math

import torch

from jmt import functional as JF
from jmt import ops

DEV = "cuda"
E = 512


def inputs(cd, Lq, Lk, N, seed=41):
    g = torch.Generator(device=DEV).manual_seed(seed)
    qkv = torch.randn(N, Lq, 3 * E, device=DEV, generator=g).to(cd).permute(1, 0, 2)
    kv = torch.randn(N, Lk, 2 * E, device=DEV, generator=g).to(cd).permute(1, 0, 2)
    go = torch.randn(Lq, N, E, device=DEV, generator=g).to(cd)
    return qkv, kv, go


def st(t):
    return (t.stride(0), t.stride(1))


def kr_op(ranges, mod):
    """The `kr` operand of a list of (kbeg, kend) pairs, one per table entry."""
    assert len(ranges) == mod
    return (torch.tensor(ranges, dtype=torch.int32, device=DEV).reshape(-1).contiguous(), mod)


def fwd(qkv, kv, H, kr=None):
    Lq, N = qkv.shape[:2]
    Lk = kv.shape[0]
    o = torch.full((Lq, N, E), float("nan"), device=DEV, dtype=qkv.dtype)
    lse = torch.full((N * H * Lq,), float("nan"), device=DEV)
    ops.attn_mh_fwd(ops.dt(qkv), N, H, Lq, Lk, E // H, qkv[..., :E].data_ptr(), st(qkv),
                    kv[..., :E].data_ptr(), st(kv), kv[..., E:].data_ptr(), st(kv), o.data_ptr(),
                    st(o), 1.0 / math.sqrt(E // H), lse, kr=kr)
    return o, lse


def bwd(qkv, kv, go, o, lse, H, kr=None):
    Lq, N = qkv.shape[:2]
    Lk = kv.shape[0]
    cd = qkv.dtype
    dqkv = torch.full((N, Lq, 3 * E), float("nan"), device=DEV, dtype=cd).permute(1, 0, 2)
    dkv = torch.full((N, Lk, 2 * E), float("nan"), device=DEV, dtype=cd).permute(1, 0, 2)
    delta = torch.full((N * H * Lq,), float("nan"), device=DEV)
    ops.attn_mh_bwd(ops.dt(qkv), N, H, Lq, Lk, E // H, go.data_ptr(), st(go), o.data_ptr(), st(o),
                    qkv[..., :E].data_ptr(), st(qkv), kv[..., :E].data_ptr(), st(kv),
                    kv[..., E:].data_ptr(), st(kv), lse, dqkv[..., E:2 * E].data_ptr(), st(dqkv),
                    dkv[..., :E].data_ptr(), st(dkv), dkv[..., E:].data_ptr(), st(dkv),
                    1.0 / math.sqrt(E // H), delta, kr=kr)
    torch.cuda.synchronize()
    # the neighbouring columns of the packed dq buffer stay untouched
    assert torch.isnan(dqkv[..., :E].float()).all() and torch.isnan(dqkv[..., 2 * E:].float()).all()
    return dqkv[..., E:2 * E], dkv[..., :E], dkv[..., E:], delta


def valid_keys(Lk, N, ranges=None):
    """(N, Lk) bool: key k of sequence n is inside its range (entry n % len(ranges))."""
    ar = torch.arange(Lk, device=DEV)
    if ranges is None:
        return torch.ones(N, Lk, dtype=torch.bool, device=DEV)
    r = torch.tensor([ranges[n % len(ranges)] for n in range(N)], device=DEV)
    return (ar[None] >= r[:, :1]) & (ar[None] < r[:, 1:])


def ref64(qkv, kv, go, H, o=None, ranges=None):
    """float64 from the same rounded inputs, all heads at once; o: the 16-bit output delta is
    taken from (None: the float64 output itself).  Tensors come back as (L, N, E), lse as
    (N * H * Lq), dpmax (over the valid keys) per head."""
    Lq, N = qkv.shape[:2]
    Lk = kv.shape[0]
    dh = E // H
    scale = 1.0 / math.sqrt(dh)
    hv = lambda t: t.double().reshape(t.shape[0], N, H, dh)
    q, k, v, d = hv(qkv[..., :E]), hv(kv[..., :E]), hv(kv[..., E:]), hv(go)
    ok = valid_keys(Lk, N, ranges)[:, None, None, :]
    s = torch.einsum("lnhd,knhd->nhlk", q, k) * scale
    s = s.masked_fill(~ok, float("-inf"))
    p = torch.softmax(s, -1)
    oo = torch.einsum("nhlk,knhd->lnhd", p, v)
    dp = torch.einsum("lnhd,knhd->nhlk", d, v)
    delta = (d * (oo if o is None else hv(o))).sum(-1).permute(1, 2, 0).unsqueeze(-1)
    ds = p * (dp - delta) * scale
    return dict(o=oo.reshape(Lq, N, E), lse=torch.logsumexp(s, -1).reshape(-1),
                dq=torch.einsum("nhlk,knhd->lnhd", ds, k).reshape(Lq, N, E),
                dk=torch.einsum("nhlk,lnhd->knhd", ds, q).reshape(Lk, N, E),
                dv=torch.einsum("nhlk,lnhd->knhd", p, d).reshape(Lk, N, E),
                dpmax=(dp * ok).abs().amax((0, 2, 3)),
                # for fp32_residue: the largest sum of |dO| |V| products behind one dP entry and
                # the largest column sum of P
                absdp=(torch.einsum("lnhd,knhd->nhlk", d.abs(), v.abs()) * ok).max().item(),
                pcolmax=p.sum(2).max().item())


def fp32_residue(ref, qkv, kv, H):
    """What the fp32 sums behind dP - Delta can leave in dq / dk where the exact dS cancels.
    The fused kernels take Delta = rowsum(dO o O) and dP = dO V^T as two fp32 sums of dh products
    each, in different orders; either is off by at most (dh - 1) 2^-24 times its sum of absolute
    products, which is at most A = max sum_d |dO_d| |V_d| (O is a convex combination of V rows).
    So dS = scale P (dP - Delta) carries up to scale P 2 (dh - 1) 2^-24 A of it, dq = dS K up to
    that times max|K| (a row of P sums to 1) and dk = dS^T Q up to that times max|Q| times the
    largest column sum of P.  The GEMM path's softmax backward forms Delta = rowsum(P o dP) from
    the very dP it subtracts it from, so with one key (P = 1) it returns the exact 0 and an error
    RATIO against it says nothing: below this residue the residue is the bound."""
    dh = E // H
    r = (1.0 / math.sqrt(dh)) * 2 * (dh - 1) * 2.0 ** -24 * ref["absdp"]
    return dict(o=0.0, dv=0.0, dq=r * kv[..., :E].float().abs().max().item(),
                dk=r * qkv[..., :E].float().abs().max().item() * ref["pcolmax"])


def errors(got, ref):
    """max |got - ref| per output name."""
    return {n: (got[n].double() - ref[n]).abs().max().item() for n in got}


def check_bounds(cd, qkv, kv, got, ref, H, what=""):
    """The forms of tests/test_gpu_attn_short.py, per head: o 1e-2 / 2e-3 max(|o|, 1), lse 1e-3
    max(|lse|, 1), dq / dk 16 u max|ref| + 4 u scale max|dP| max|K or Q|, dv 8 u max|ref|."""
    dh = E // H
    bf = cd == torch.bfloat16
    u = 2.0 ** -8 if bf else 2.0 ** -11
    if "lse" in got:
        err = (got["lse"].double() - ref["lse"]).abs().max().item()
        tol = 1e-3 * max(ref["lse"].abs().max().item(), 1.0)
        print(f"{what} lse err {err:.3e} tol {tol:.3e}")
        assert err <= tol
    for h in range(H):
        sl = slice(h * dh, (h + 1) * dh)
        floor = 4 * u * (1.0 / math.sqrt(dh)) * ref["dpmax"][h].item()
        qmax = qkv[..., :E][..., sl].float().abs().max().item()
        kmax = kv[..., :E][..., sl].float().abs().max().item()
        amax = lambda n: ref[n][..., sl].abs().max().item()
        tols = dict(o=(1e-2 if bf else 2e-3) * max(amax("o"), 1.0),
                    dq=16 * u * amax("dq") + floor * kmax, dk=16 * u * amax("dk") + floor * qmax,
                    dv=8 * u * amax("dv"))
        for n, tol in tols.items():
            if n not in got:
                continue
            assert torch.isfinite(got[n][..., sl].float()).all(), (what, n, h)
            err = (got[n][..., sl].double() - ref[n][..., sl]).abs().max().item()
            if h == 0:
                print(f"{what} {n} head 0 err {err:.3e} tol {tol:.3e}")
            assert err <= tol, (what, n, h, err, tol)


def gemm_path(cd, qkv, kv, go, H, ranges=None):
    """The GEMM + softmax path of the same build on the same views (the fused kernels switched
    off): o, dq, dk, dv."""
    Lq, N = qkv.shape[:2]
    Lk = kv.shape[0]
    kr = None
    if ranges is not None:
        kr = JF.KeyRanges(kr_op(ranges, len(ranges))[0], len(ranges), Lk)
    dqkv = torch.full((N, Lq, 3 * E), float("nan"), device=DEV, dtype=cd).permute(1, 0, 2)
    dkv = torch.full((N, Lk, 2 * E), float("nan"), device=DEV, dtype=cd).permute(1, 0, 2)
    ops._attn_mh["on"] = ops._attn_fused["on"] = False
    try:
        with JF.compute_mode(cd):
            o, saved = JF.attn_forward(qkv, kv, kv, E, H, 0, 0, E, kr=kr)
            assert saved[1].fwd == "gemm"
            JF.attn_backward(saved, go, dqkv, dkv, dkv)
    finally:
        ops._attn_mh["on"] = ops._attn_fused["on"] = True
    torch.cuda.synchronize()
    return dict(o=o, dq=dqkv[..., :E], dk=dkv[..., :E], dv=dkv[..., E:])
