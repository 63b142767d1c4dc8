"""Shared pieces of the attention dropout tests (tests/test_attn_dropout_ref.py,
tests/test_gpu_attn_mh_dropout.py): the mask restated in numpy from its specification (DESIGN.md
section 4; independent of csrc/dropout.h), the multi-head entry points with `drop` on NaN-poisoned
buffers, the float64 reference with the mask injected and its bounds.

  element   (nh, l, k), nh = n H + h
  key       (seed_lo, seed_hi)
  counter   (nh QB + (l >> 2), k >> 2, call, stream), QB = ceil(Lq / 4)
  byte      byte k & 3 of output word l & 3
  keep      byte >= T8, T8 = floor(256 p + 1/2) with p the float32 rate; p_eff = T8 / 256
  scale     s = 1 / (1 - p_eff) in float32; T8 = 0: everything kept, s = 1
"""
import math

import numpy as np
import torch

from jmt import ops
from tests import attn_mh_ref as R
from tests import dropout_ref as D

DEV = R.DEV
E = R.E


def threshold(p) -> int:
    return int(math.floor(256.0 * float(np.float32(p)) + 0.5))


def rate(p) -> float:
    return threshold(p) / 256.0


def scale(p) -> np.float32:
    return np.float32(1.0) / (np.float32(1.0) - np.float32(rate(p)))


def mask_bytes(ctr, NH, Lq, Lk):
    """The (NH, Lq, Lk) uint32 array of mask bytes under state block ctr = (seed_lo, seed_hi,
    call, stream)."""
    seed_lo, seed_hi, call, stream = (int(v) & 0xFFFFFFFF for v in ctr)
    QB, KB = (Lq + 3) // 4, (Lk + 3) // 4
    qb = (np.arange(NH, dtype=np.uint64)[:, None] * np.uint64(QB) +
          np.arange(QB, dtype=np.uint64)[None, :]).reshape(-1, 1)
    kb = np.arange(KB, dtype=np.uint64)[None, :]
    w = np.stack(D.philox4x32_10((qb, kb, call, stream), (seed_lo, seed_hi)), axis=-1)
    # [query block, key block, word = l & 3, byte = k & 3]
    b = (w[..., None] >> (np.uint32(8) * np.arange(4, dtype=np.uint32))) & np.uint32(255)
    b = b.reshape(NH, QB, KB, 4, 4).transpose(0, 1, 3, 2, 4).reshape(NH, 4 * QB, 4 * KB)
    return np.ascontiguousarray(b[:, :Lq, :Lk])


def mask(ctr, NH, Lq, Lk, p):
    """float32 (NH, Lq, Lk) multipliers: 0 or s."""
    b = mask_bytes(ctr, NH, Lq, Lk)
    return np.where(b >= threshold(p), scale(p), np.float32(0.0)).astype(np.float32)


def ctr_tensor(ctr):
    """A device state copy (what ops.dropout_next hands a forward) of the host words `ctr`."""
    w = [int(v) & 0xFFFFFFFF for v in ctr]
    return torch.tensor([v - (1 << 32) if v >= (1 << 31) else v for v in w], dtype=torch.int32,
                        device=DEV)


def lib_mask(ctr, N, H, Lq, Lk, p):
    """The library's host reference as a float64 (N, H, Lq, Lk) device tensor."""
    m = ops.attn_dropout_reference(ctr, N * H, Lq, Lk, p)
    return torch.from_numpy(m).to(DEV).double().reshape(N, H, Lq, Lk)


def fwd(qkv, kv, H, drop, kr=None, v=None):
    """attn_mh_ref.fwd with drop = (p, state copy); v: a (Lk, N, E) tensor in place of the packed
    value half."""
    Lq, N = qkv.shape[:2]
    Lk = kv.shape[0]
    o = torch.full((Lq, N, E), float("nan"), device=DEV, dtype=qkv.dtype)
    lse = torch.full((N * H * Lq,), float("nan"), device=DEV)
    vp, vs = (kv[..., E:].data_ptr(), R.st(kv)) if v is None else (v.data_ptr(), R.st(v))
    ops.attn_mh_fwd(ops.dt(qkv), N, H, Lq, Lk, E // H, qkv[..., :E].data_ptr(), R.st(qkv),
                    kv[..., :E].data_ptr(), R.st(kv), vp, vs, o.data_ptr(), R.st(o),
                    1.0 / math.sqrt(E // H), lse, kr=kr, drop=drop)
    return o, lse


def bwd(qkv, kv, go, o, lse, H, drop, kr=None):
    """attn_mh_ref.bwd with drop = (p, state copy)."""
    Lq, N = qkv.shape[:2]
    Lk = kv.shape[0]
    cd = qkv.dtype
    dqkv = torch.full((N, Lq, 3 * E), float("nan"), device=DEV, dtype=cd).permute(1, 0, 2)
    dkv = torch.full((N, Lk, 2 * E), float("nan"), device=DEV, dtype=cd).permute(1, 0, 2)
    delta = torch.full((N * H * Lq,), float("nan"), device=DEV)
    ops.attn_mh_bwd(ops.dt(qkv), N, H, Lq, Lk, E // H, go.data_ptr(), R.st(go), o.data_ptr(),
                    R.st(o), qkv[..., :E].data_ptr(), R.st(qkv), kv[..., :E].data_ptr(), R.st(kv),
                    kv[..., E:].data_ptr(), R.st(kv), lse, dqkv[..., E:2 * E].data_ptr(),
                    R.st(dqkv), dkv[..., :E].data_ptr(), R.st(dkv), dkv[..., E:].data_ptr(),
                    R.st(dkv), 1.0 / math.sqrt(E // H), delta, kr=kr, drop=drop)
    torch.cuda.synchronize()
    assert torch.isnan(dqkv[..., :E].float()).all() and torch.isnan(dqkv[..., 2 * E:].float()).all()
    return dqkv[..., E:2 * E], dkv[..., :E], dkv[..., E:], delta


def ref64_drop(qkv, kv, go, H, M, o=None, ranges=None):
    """attn_mh_ref.ref64 with the multipliers M (N, H, Lq, Lk; float64) injected: O = (M o P) V,
    dV = (M o P)^T dO, dP = M o (dO V^T), dS = scale P o (dP - delta); dpmax from the masked dP."""
    Lq, N = qkv.shape[:2]
    Lk = kv.shape[0]
    dh = E // H
    sc = 1.0 / math.sqrt(dh)
    hv = lambda t: t.double().reshape(t.shape[0], N, H, dh)
    q, k, v, d = hv(qkv[..., :E]), hv(kv[..., :E]), hv(kv[..., E:]), hv(go)
    ok = R.valid_keys(Lk, N, ranges)[:, None, None, :]
    s = torch.einsum("lnhd,knhd->nhlk", q, k) * sc
    s = s.masked_fill(~ok, float("-inf"))
    p = torch.softmax(s, -1)
    pm = p * M
    oo = torch.einsum("nhlk,knhd->lnhd", pm, v)
    dp = M * torch.einsum("lnhd,knhd->nhlk", d, v)
    delta = (d * (oo if o is None else hv(o))).sum(-1).permute(1, 2, 0).unsqueeze(-1)
    ds = p * (dp - delta) * sc
    return dict(o=oo.reshape(Lq, N, E), lse=torch.logsumexp(s, -1).reshape(-1),
                dq=torch.einsum("nhlk,knhd->lnhd", ds, k).reshape(Lq, N, E),
                dk=torch.einsum("nhlk,lnhd->knhd", ds, q).reshape(Lk, N, E),
                dv=torch.einsum("nhlk,lnhd->knhd", pm, d).reshape(Lk, N, E),
                dpmax=(dp * ok).abs().amax((0, 2, 3)),
                delta=delta.reshape(-1),
                absdp=(torch.einsum("lnhd,knhd->nhlk", d.abs(), v.abs()) * ok).max().item(),
                pcolmax=p.sum(2).max().item())


def o_tol(cd, ref_o_head, s):
    """o against s (1e-2 bf16 / 2e-3 fp16) max(|o|, 1): every kept probability is multiplied by
    s after it is rounded, so the rounding errors behind o scale by s, also where |o| < 1 (the
    constant floor of the plain form does not scale by itself)."""
    return float(s) * (1e-2 if cd == torch.bfloat16 else 2e-3) * max(
        ref_o_head.abs().max().item(), 1.0)


def check_bounds(cd, qkv, kv, got, ref, H, s, what=""):
    """lse, dq, dk, dv under attn_mh_ref.check_bounds unchanged against the masked reference
    (its bounds are relative to the reference's magnitudes, which contain s), o under o_tol."""
    R.check_bounds(cd, qkv, kv, {n: t for n, t in got.items() if n != "o"}, ref, H, what=what)
    if "o" not in got:
        return
    dh = E // H
    for h in range(H):
        sl = slice(h * dh, (h + 1) * dh)
        assert torch.isfinite(got["o"][..., sl].float()).all(), (what, "o", h)
        err = (got["o"][..., sl].double() - ref["o"][..., sl]).abs().max().item()
        tol = o_tol(cd, ref["o"][..., sl], s)
        if h == 0:
            print(f"{what} o head 0 err {err:.3e} tol {tol:.3e}")
        assert err <= tol, (what, "o", h, err, tol)
