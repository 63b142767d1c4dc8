"""Shared queries in the attention kernels (jmt_attn_fwd_sq / jmt_attn_bwd_sq / jmt_attn_dkdv_sq)
and in the grouped cross-attention block (jmt/grouped.py CrossAttention6Fn).

Every query is used by two sequences.  Reading Q through the table changes one address only, so
the forward, the P / dS kernel and dK / dV must be bitwise what the unshared entry points give on
a Q buffer that holds each query once per sequence.  The merged dQ = dS_i K_i + dS_j K_j (one fp32
accumulator over the keys of both sequences, rounded once) is checked against fp32 and, with one
use's dS zeroed, bitwise against the unshared dQ of the other use: that pins the chunk order and
the per-sequence masking of the keys past Lk.

Layout as tests/test_gpu_attn_dkdv_tiles.py: packed buffers prefilled with 7.0, the untouched
columns asserted, NaN in the P / dS columns past Lk.  The q columns of the second uses hold NaN in
the shared buffer: nothing may read them."""
import functools

import pytest
import torch

from jmt import _lib, ops

DEV = "cuda"

# (Lq, Lk, N, queries, H); N sequences = 4 pairs of N / 4, pairs 2 and 3 reuse the queries of
# pairs 1 and 0 (crossed, as CROSS_PAIRS' second uses are)
QTAB = [0, 1, 1, 0]
SHAPES = [
    (300, 300, 4, 2, 1),      # the step shape
    (160, 160, 4, 2, 1),      # exactly one tile
    (161, 161, 4, 2, 2),      # one row into a second tile, two heads
    (77, 130, 4, 2, 2),       # ragged: the seam inside a 32-key chunk, the ldp clamp
    (65, 33, 4, 2, 1),        # the smallest Lq the rows kernel takes
    (161, 161, 140, 70, 1),   # more items than CUs in all three kernels
]
DTYPES = [torch.bfloat16, torch.float16]
st = lambda t: (t.stride(0), t.stride(1))


def _src(n, spp):
    return QTAB[n // spp] * spp + n % spp


@functools.lru_cache(maxsize=None)
def _inputs(cd, Lq, Lk, N, nq, H):
    """Shared and materialised Q (packed (L, N, 3 E) views), K / V, dO.  Computed once per case
    and left unchanged."""
    assert N == 2 * nq and N % 4 == 0
    spp = N // 4
    E = 512 * H
    g = torch.Generator(device=DEV).manual_seed(47)
    qkv_m = torch.randn(N, Lq, 3 * E, device=DEV, generator=g).to(cd)
    for n in range(N):
        qkv_m[n, :, :E] = qkv_m[_src(n, spp), :, :E]
    qkv_s = qkv_m.clone()
    for n in range(N):
        if _src(n, spp) != n:
            qkv_s[n, :, :E] = float("nan")
    kk = torch.randn(N, Lk, 3 * E, device=DEV, generator=g).to(cd).permute(1, 0, 2)
    go = torch.randn(Lq, N, E, device=DEV, generator=g).to(cd)
    return spp, qkv_s.permute(1, 0, 2), qkv_m.permute(1, 0, 2), kk, go


@functools.lru_cache(maxsize=None)
def _fwd(cd, Lq, Lk, N, nq, H):
    """(o, lse) of the unshared entry point on the materialised Q and of the shared one."""
    spp, qs, qm, kk, go = _inputs(cd, Lq, Lk, N, nq, H)
    E = 512 * H
    res = []
    for shared in (False, True):
        q = qs if shared else qm
        o = torch.full((N, Lq, E), 7.0, device=DEV, dtype=cd).permute(1, 0, 2)
        lse = torch.full((N * H * Lq,), 7.0, device=DEV, dtype=torch.float32)
        args = (ops.dt(q), N, H, Lq, Lk, 512, q.data_ptr(), st(q), kk[..., E:].data_ptr(), st(kk),
                kk[..., 2 * E:].data_ptr(), st(kk), o.data_ptr(), st(o), 512 ** -0.5, lse)
        if shared:
            ops.attn_fwd_sq(*args, spp, QTAB)
        else:
            ops.attn_fwd(*args)
        torch.cuda.synchronize()
        res.append((o, lse))
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("cd", DTYPES)
@pytest.mark.parametrize("Lq,Lk,N,nq,H", SHAPES)
def test_fwd_shared_q_bitwise(cd, Lq, Lk, N, nq, H):
    (o_m, lse_m), (o_s, lse_s) = _fwd(cd, Lq, Lk, N, nq, H)
    assert torch.isfinite(o_s.float()).all() and torch.isfinite(lse_s).all()
    assert torch.equal(o_m.view(torch.int16), o_s.view(torch.int16))
    assert torch.equal(lse_m.view(torch.int32), lse_s.view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("cd", DTYPES)
@pytest.mark.parametrize("Lq,Lk,N,nq,H", SHAPES)
def test_pds_shared_q_bitwise(cd, Lq, Lk, N, nq, H):
    """P and dS (tile-major, every byte of the hand-off buffers) of jmt_attn_bwd_sq against
    jmt_attn_bwd(dq = NULL) on the materialised Q."""
    spp, qs, qm, kk, go = _inputs(cd, Lq, Lk, N, nq, H)
    (o, lse), _ = _fwd(cd, Lq, Lk, N, nq, H)
    E = 512 * H
    ldp = ops.attn_dkdv_ldp(Lk)
    res = []
    for shared in (False, True):
        q = qs if shared else qm
        P = torch.full((N * H * Lq * ldp,), 7.0, device=DEV, dtype=cd)
        dS = torch.full((N * H * Lq * ldp,), 7.0, device=DEV, dtype=cd)
        args = (ops.dt(q), N, H, Lq, Lk, 512, go.data_ptr(), st(go), o.data_ptr(), st(o),
                q.data_ptr(), st(q), kk[..., E:].data_ptr(), st(kk), kk[..., 2 * E:].data_ptr(),
                st(kk), lse, P, dS, ldp)
        if shared:
            ops.attn_bwd_sq(*args, 512 ** -0.5, spp, QTAB)
        else:
            ops.attn_bwd(*args, None, (0, 0), 512 ** -0.5)
        torch.cuda.synchronize()
        res.append((P, dS))
    (P_m, dS_m), (P_s, dS_s) = res
    assert not torch.isnan(P_s.float()).any() and not torch.isnan(dS_s.float()).any()
    assert torch.equal(P_m.view(torch.int16), P_s.view(torch.int16))
    assert torch.equal(dS_m.view(torch.int16), dS_s.view(torch.int16))


@functools.lru_cache(maxsize=None)
def _pds(cd, Lq, Lk, N, nq, H):
    """Synthetic P / dS with NaN past Lk (row-major for the references, tile-major for the
    kernels), and the two seam variants of dS: the first / the second uses' columns < Lk zeroed."""
    spp = N // 4
    g = torch.Generator(device=DEV).manual_seed(53)
    ldp = ops.attn_dkdv_ldp(Lk)
    P = torch.full((N * H, Lq, ldp), float("nan"), device=DEV, dtype=cd)
    dS = torch.full((N * H, Lq, ldp), float("nan"), device=DEV, dtype=cd)
    P[..., :Lk] = torch.rand(N * H, Lq, Lk, device=DEV, generator=g).to(cd)
    dS[..., :Lk] = (torch.randn(N * H, Lq, Lk, device=DEV, generator=g) * 0.1).to(cd)
    first = torch.tensor([_src(n, spp) == n for n in range(N)], device=DEV)
    first = first.repeat_interleave(H)
    dS_f, dS_s = dS.clone(), dS.clone()           # only the first / only the second uses' dS
    dS_f[~first, :, :Lk] = 0
    dS_s[first, :, :Lk] = 0
    tiled = lambda t: t.view(N * H, Lq, ldp // 32, 32).permute(0, 2, 1, 3).contiguous()
    return ldp, P, dS, tiled(P), {"all": tiled(dS), "first": tiled(dS_f), "second": tiled(dS_s)}


def _dkdv(cd, Lq, Lk, N, nq, H, tile, mode, ds_key="all"):
    """One jmt_attn_dkdv launch; mode: 'unshared' (materialised Q), 'shared' (per-pair dQ) or
    'merged'.  Returns the packed (dK | dV) buffer and the packed dQ buffer."""
    lib = _lib.load()
    spp, qs, qm, kk, go = _inputs(cd, Lq, Lk, N, nq, H)
    ldp, _, _, Pt, dSt = _pds(cd, Lq, Lk, N, nq, H)
    E = 512 * H
    q = qm if mode == "unshared" else qs
    out = torch.full((N, Lk, 3 * E), 7.0, device=DEV, dtype=cd).permute(1, 0, 2)
    dqo = torch.full((N, Lq, 3 * E), 7.0, device=DEV, dtype=cd).permute(1, 0, 2)
    try:
        assert lib.jmt_attn_dkdv_set_tile(tile) == _lib.OK
        assert lib.jmt_attn_dkdv_plan(Lq, Lk, H, out.stride(0), out.stride(0), dqo.stride(0),
                                      1) == tile
        args = (ops.dt(q), N, H, Lq, Lk, 512, Pt, dSt[ds_key], ldp, go.data_ptr(), st(go),
                q.data_ptr(), st(q), out[..., E:2 * E].data_ptr(), st(out),
                out[..., 2 * E:].data_ptr(), st(out), kk[..., E:].data_ptr(), st(kk),
                dqo[..., :E].data_ptr(), st(dqo))
        if mode == "unshared":
            ops.attn_dkdv(*args)
        else:
            ops.attn_dkdv_sq(*args, spp, QTAB, mode == "merged")
        torch.cuda.synchronize()
    finally:
        lib.jmt_attn_dkdv_set_tile(-1)
    return out, dqo


@pytest.mark.gpu
@pytest.mark.parametrize("cd", DTYPES)
@pytest.mark.parametrize("Lq,Lk,N,nq,H", SHAPES)
def test_dkdv_shared_q_bitwise(cd, Lq, Lk, N, nq, H):
    """dK / dV (and the per-pair dQ) of jmt_attn_dkdv_sq against jmt_attn_dkdv on the
    materialised Q, for the forced 128-row and the forced 160-row tile."""
    E = 512 * H
    for tile in (128, 160):
        o_m, q_m = _dkdv(cd, Lq, Lk, N, nq, H, tile, "unshared")
        o_s, q_s = _dkdv(cd, Lq, Lk, N, nq, H, tile, "shared")
        assert torch.isfinite(o_s.float()).all() and torch.isfinite(q_s.float()).all()
        assert torch.equal(o_m.view(torch.int16), o_s.view(torch.int16)), tile
        assert torch.equal(q_m.view(torch.int16), q_s.view(torch.int16)), tile
        assert (o_s[..., :E].float() == 7.0).all() and (q_s[..., E:].float() == 7.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("cd", DTYPES)
@pytest.mark.parametrize("Lq,Lk,N,nq,H", SHAPES)
def test_merged_dq_vs_fp32(cd, Lq, Lk, N, nq, H):
    """The merged dQ against einsum(dS_i, K_i) + einsum(dS_j, K_j) in fp32 on the same 16-bit
    inputs; bound of test_attn_dkdv_160_vs_fp32 (fp32 accumulation of L products, one 16-bit
    rounding) with L = 2 Lk: 2 u max|ref| + 1e-6 L.  dK / dV stay bitwise the unshared ones."""
    spp, qs, qm, kk, go = _inputs(cd, Lq, Lk, N, nq, H)
    _, _, dS, _, _ = _pds(cd, Lq, Lk, N, nq, H)
    E = 512 * H
    o_m, _ = _dkdv(cd, Lq, Lk, N, nq, H, 160, "unshared")
    out, dqo = _dkdv(cd, Lq, Lk, N, nq, H, 160, "merged")
    assert torch.equal(o_m.view(torch.int16), out.view(torch.int16))
    dSr = dS[..., :Lk].float().view(N, H, Lq, Lk)
    kr = kk[..., E:2 * E].float().reshape(Lk, N, H, 512)
    per = torch.einsum("nhqk,knhd->qnhd", dSr, kr).reshape(Lq, N, E)
    firsts = [n for n in range(N) if _src(n, spp) == n]
    second = {f: next(n for n in range(N) if n != f and _src(n, spp) == f) for f in firsts}
    ref = torch.stack([per[:, f] + per[:, second[f]] for f in firsts], 1)
    got = dqo[..., :E][:, firsts].float()
    assert torch.isfinite(got).all()
    u = 2.0 ** -8 if cd == torch.bfloat16 else 2.0 ** -11
    err = (got - ref).abs().max().item()
    bound = 2 * u * ref.abs().max().item() + 1e-6 * 2 * Lk
    print(f"merged dQ err {err:.3e} bound {bound:.3e}")
    assert err <= bound, (err, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("cd", DTYPES)
@pytest.mark.parametrize("Lq,Lk,N,nq,H", SHAPES)
def test_merged_dq_seam(cd, Lq, Lk, N, nq, H):
    """With the second use's dS zeroed (columns < Lk; the NaN padding kept) the merged dQ is
    bitwise the unshared dQ of the first use, with the first use's zeroed that of the second use;
    both tiles give bitwise the same merged dQ; the second uses' dQ rows keep the sentinel."""
    spp = N // 4
    E = 512 * H
    firsts = [n for n in range(N) if _src(n, spp) == n]
    seconds = [next(n for n in range(N) if n != f and _src(n, spp) == f) for f in firsts]
    _, q_un = _dkdv(cd, Lq, Lk, N, nq, H, 160, "unshared")
    for key, srcs in (("first", firsts), ("second", seconds)):
        _, q_mg = _dkdv(cd, Lq, Lk, N, nq, H, 160, "merged", key)
        assert torch.isfinite(q_mg[..., :E][:, firsts].float()).all()
        assert torch.equal(q_mg[..., :E][:, firsts].contiguous().view(torch.int16),
                           q_un[..., :E][:, srcs].contiguous().view(torch.int16)), key
    _, q128 = _dkdv(cd, Lq, Lk, N, nq, H, 128, "merged")
    _, q160 = _dkdv(cd, Lq, Lk, N, nq, H, 160, "merged")
    assert torch.equal(q128.view(torch.int16), q160.view(torch.int16))
    assert (q160[:, seconds].float() == 7.0).all()
    assert (q160[..., E:].float() == 7.0).all()


@pytest.mark.gpu
def test_shared_q_refusals():
    """Lq = 64 (the 64-row forward kernel) and fp32: JMT_ERR_UNSUPPORTED, nothing written."""
    lib = _lib.load()
    import ctypes as C
    tab = (C.c_int * 4)(*QTAB)
    for dtype, Lq in ((torch.bfloat16, 64), (torch.float32, 300)):
        N, Lk, E = 4, 96, 512
        q = torch.zeros(N, Lq, 3 * E, device=DEV, dtype=dtype).permute(1, 0, 2)
        kk = torch.zeros(N, Lk, 3 * E, device=DEV, dtype=dtype).permute(1, 0, 2)
        o = torch.full((N, Lq, E), 7.0, device=DEV, dtype=dtype).permute(1, 0, 2)
        lse = torch.full((N * Lq,), 7.0, device=DEV, dtype=torch.float32)
        rc = lib.jmt_attn_fwd_sq(ops.dt(q), N, 1, Lq, Lk, 512, q.data_ptr(), *st(q),
                                 kk[..., E:].data_ptr(), *st(kk), kk[..., 2 * E:].data_ptr(),
                                 *st(kk), o.data_ptr(), *st(o), 512 ** -0.5, lse.data_ptr(), 1, tab,
                                 4, None)
        assert rc == _lib.ERR_UNSUPPORTED, (dtype, rc)
        ldp = ops.attn_dkdv_ldp(Lk)
        P = torch.full((N * Lq * ldp,), 7.0, device=DEV, dtype=dtype)
        dS = torch.full((N * Lq * ldp,), 7.0, device=DEV, dtype=dtype)
        if dtype == torch.float32:
            rc = lib.jmt_attn_bwd_sq(ops.dt(q), N, 1, Lq, Lk, 512, o.data_ptr(), *st(o),
                                     o.data_ptr(), *st(o), q.data_ptr(), *st(q),
                                     kk[..., E:].data_ptr(), *st(kk), kk[..., 2 * E:].data_ptr(),
                                     *st(kk), lse.data_ptr(), P.data_ptr(), dS.data_ptr(), ldp,
                                     512 ** -0.5, 1, tab, 4, None)
            assert rc == _lib.ERR_UNSUPPORTED, rc
            rc = lib.jmt_attn_dkdv_sq(ops.dt(q), N, 1, Lq, Lk, 512, P.data_ptr(), dS.data_ptr(),
                                      ldp, o.data_ptr(), *st(o), q.data_ptr(), *st(q),
                                      kk[..., E:].data_ptr(), *st(kk), kk[..., E:].data_ptr(),
                                      *st(kk), kk[..., 2 * E:].data_ptr(), *st(kk), q.data_ptr(),
                                      *st(q), 1, tab, 4, 1, None)
            assert rc == _lib.ERR_UNSUPPORTED, rc
        torch.cuda.synchronize()
        assert (o.float() == 7.0).all() and (lse == 7.0).all()
        assert (P.float() == 7.0).all() and (dS.float() == 7.0).all()
        assert (kk.float() == 0).all() and (q.float() == 0).all()


# ----------------------------------------------------------------------- CrossAttention6Fn
def _ca6(arm, cd, pairs, record=None):
    """One forward + backward of cross_attention6 at B = 2, T = 77 on fixed inputs and weights
    (all bf16-representable, so the fp32 compute mode sees the same values).
    arm: 'off' (JMT_CA_SHARED_Q=0), 'stage1' (JMT_CA_DQ_MERGE=0) or 'default'."""
    from jmt import functional as JF, grouped
    B, T, E, H = 2, 77, 512, 1
    g = torch.Generator(device="cpu").manual_seed(61)
    nmod = 1 + max(m for m, _, _ in pairs)
    r16 = lambda t: t.to(torch.bfloat16).float()
    mods = []
    for _ in range(nmod):
        m = torch.nn.MultiheadAttention(E, H)
        with torch.no_grad():
            m.in_proj_weight.copy_(r16(torch.randn(3 * E, E, generator=g) * E ** -0.5))
            m.in_proj_bias.copy_(r16(torch.randn(3 * E, generator=g) * 0.1))
            m.out_proj.weight.copy_(r16(torch.randn(E, E, generator=g) * E ** -0.5))
            m.out_proj.bias.copy_(r16(torch.randn(E, generator=g) * 0.1))
        mods.append(m.to(DEV))
    Y = r16(torch.randn(3, B, T, E, generator=g)).to(DEV, cd).requires_grad_(True)
    dO6 = r16(torch.randn(len(pairs), B, T, E, generator=g)).to(DEV, cd)
    prev = dict(grouped._shared_q)
    grouped._shared_q.update(on=arm != "off", merge=arm == "default")
    if record is not None:
        keys = ("family", "M", "N", "K", "batch", "beta", "grouped", "shared_q", "merge_dq")
        ops.set_launch_hook(lambda info, launch: (
            record.append(tuple(info.get(k) for k in keys)), launch())[1])
    try:
        with JF.compute_mode(cd):
            O6 = grouped.cross_attention6(Y, mods, H, pairs)
            O6.backward(dO6)
        torch.cuda.synchronize()
    finally:
        grouped._shared_q.update(prev)
        ops.set_launch_hook(None)
    out = {"O6": O6.detach(), "dY": Y.grad}
    for i, m in enumerate(mods):
        out[f"in_w{i}"], out[f"in_b{i}"] = m.in_proj_weight.grad, m.in_proj_bias.grad
        out[f"out_w{i}"], out[f"out_b{i}"] = m.out_proj.weight.grad, m.out_proj.bias.grad
    return out


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.mark.gpu
def test_cross_attention6_arms():
    """Stage 1 (shared Q, per-pair dQ) is bitwise the unshared block.  The default (merged dQ)
    is bitwise too, except dY and the q rows of the in_proj gradients: there the one 16-bit
    rounding of dQ moves (dQ_i and dQ_j rounded, then summed in fp32, against summed in fp32 and
    rounded once), so against the fp32 compute mode the default arm's max-abs error may exceed
    the unshared arm's by at most u max|ref|, one 16-bit rounding of the largest value.

    Measured (MI355X; max-abs error against fp32, unshared -> default): dY 1.158e-2 -> 1.158e-2
    (max|ref| 2.72); in_proj_weight q rows 6.64e-2 -> 6.79e-2, 6.57e-2 -> 6.84e-2, 6.52e-2 ->
    6.54e-2 (max|ref| 14.9, 15.2, 16.4); in_proj_bias q rows 5.27e-2 -> 5.51e-2, 4.58e-2 ->
    4.17e-2, 4.83e-2 -> 5.92e-2 (max|ref| 9.92, 11.98, 9.89; the allowance u max|ref| is
    3.9e-2 - 4.7e-2 there)."""
    from jmt.grouped import CROSS_PAIRS
    E = 512
    cd = torch.bfloat16
    off, s1, dflt = (_ca6(a, cd, CROSS_PAIRS) for a in ("off", "stage1", "default"))
    ref = _ca6("off", torch.float32, CROSS_PAIRS)
    for k in off:
        assert torch.equal(_bits(off[k]), _bits(s1[k])), f"stage 1: {k}"
    u = 2.0 ** -8
    for k in off:
        if k == "dY" or k.startswith("in_w") or k.startswith("in_b"):
            a, b, r = off[k].float(), dflt[k].float(), ref[k].float()
            if k != "dY":       # the key / value rows stay bitwise, the q rows move
                assert torch.equal(_bits(off[k][E:]), _bits(dflt[k][E:])), k
                a, b, r = a[:E], b[:E], r[:E]
            e_off, e_def = (a - r).abs().max().item(), (b - r).abs().max().item()
            print(f"{k}: max|ref| {r.abs().max().item():.4e} err off {e_off:.4e} "
                  f"default {e_def:.4e}")
            assert torch.isfinite(b).all()
            assert e_def <= e_off + u * r.abs().max().item(), (k, e_off, e_def)
        else:
            assert torch.equal(_bits(off[k]), _bits(dflt[k])), f"default: {k}"


@pytest.mark.gpu
def test_cross_attention6_no_duplicates_keeps_launches():
    """The wo_JR pairs share no query: all three arms issue the same launches and results."""
    from jmt.grouped import CROSS_PAIRS_WO_JR
    recs, outs = {}, {}
    for arm in ("off", "stage1", "default"):
        recs[arm] = []
        outs[arm] = _ca6(arm, torch.bfloat16, CROSS_PAIRS_WO_JR, recs[arm])
    assert recs["off"] and recs["off"] == recs["stage1"] == recs["default"]
    assert not any(r[-2] for r in recs["off"])
    for k in outs["off"]:
        assert torch.equal(_bits(outs["off"][k]), _bits(outs["default"][k])), k
    # and with duplicates the default arm does take the shared launches
    from jmt.grouped import CROSS_PAIRS
    rec = []
    _ca6("default", torch.bfloat16, CROSS_PAIRS, rec)
    assert sum(1 for r in rec if r[-2]) == 3 and any(r[-1] for r in rec)
