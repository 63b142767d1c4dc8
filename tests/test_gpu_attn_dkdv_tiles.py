"""jmt_attn_dkdv with 160-row items (csrc/attn_dkdv.hip, NKG = 10) against its 128-row form and
against fp32 products, and the host rule that picks the tile (jmt_attn_dkdv_plan).

The two tiles contract every output element over the same 32-deep chunks in the same order, so
dK, dV and dQ must be bitwise equal.  Shapes are the smallest at which each mechanism of the
160-row form can go wrong (one tile exactly, one row into a second tile, the ldp clamp, more items
than CUs)."""
import functools

import pytest
import torch

from jmt import _lib, ops

DEV = "cuda"

SHAPES = [
    (300, 300, 2, 1),     # the step shape
    (160, 160, 2, 1),     # exactly one tile
    (161, 161, 2, 2),     # one row into a second tile, two heads
    (1, 65, 2, 1),        # degenerate
    (129, 1, 2, 1),       # degenerate
    (77, 130, 2, 2),      # the ldp clamp: 256 < 320
    (40, 500, 2, 1),      # the clamp with several tiles: 512 < 640
    (320, 159, 2, 1),     # dQ with two full query tiles
    (161, 161, 70, 1),    # 420 items > CUs: the persistent walk, stages across items, store counts
]
DTYPES = [torch.bfloat16, torch.float16]


@functools.lru_cache(maxsize=None)
def _run(cd, Lq, Lk, N, H):
    """The layout of test_attn_dkdv_vs_fp32 (with dq): NaN in the P / dS columns past Lk, packed
    (L, N, 3 E) outputs filled with 7.0.  Returns {tile: (out, dqo)}, the inputs of the fp32
    products, and the tile the rule takes; computed once per case and left unchanged."""
    lib = _lib.load()
    E = 512 * H
    g = torch.Generator(device=DEV).manual_seed(31)
    ldp = ops.attn_dkdv_ldp(Lk)
    P = torch.full((N * H, Lq, ldp), float("nan"), device=DEV, dtype=cd)
    dS = torch.full((N * H, Lq, ldp), float("nan"), device=DEV, dtype=cd)
    P[..., :Lk] = torch.rand(N * H, Lq, Lk, device=DEV, generator=g).to(cd)
    dS[..., :Lk] = (torch.randn(N * H, Lq, Lk, device=DEV, generator=g) * 0.1).to(cd)
    qkv = torch.randn(N, Lq, 3 * E, device=DEV, generator=g).to(cd).permute(1, 0, 2)
    go = torch.randn(Lq, N, E, device=DEV, generator=g).to(cd)
    qv = qkv[..., :E]
    kk = torch.randn(N, Lk, 2 * E, device=DEV, generator=g).to(cd).permute(1, 0, 2)
    kv_ = kk[..., E:]
    st = lambda t: (t.stride(0), t.stride(1))
    tiled = lambda t: t.view(N * H, Lq, ldp // 32, 32).permute(0, 2, 1, 3).contiguous()
    Pt, dSt = tiled(P), tiled(dS)
    res = {}
    try:
        for tile in (128, 160):
            assert lib.jmt_attn_dkdv_set_tile(tile) == _lib.OK
            out = torch.full((N, Lk, 3 * E), 7.0, device=DEV, dtype=cd).permute(1, 0, 2)
            dqo = torch.full((N, Lq, 3 * E), 7.0, device=DEV, dtype=cd).permute(1, 0, 2)
            assert lib.jmt_attn_dkdv_plan(Lq, Lk, H, out.stride(0), out.stride(0),
                                          dqo.stride(0), 1) == tile
            ops.attn_dkdv(ops.dt(qkv), N, H, Lq, Lk, 512, Pt, dSt, ldp, go.data_ptr(), st(go),
                          qv.data_ptr(), st(qkv), out[..., E:2 * E].data_ptr(), st(out),
                          out[..., 2 * E:].data_ptr(), st(out), kv_.data_ptr(), st(kk),
                          dqo[..., :E].data_ptr(), st(dqo))
            torch.cuda.synchronize()
            res[tile] = (out, dqo)
    finally:
        lib.jmt_attn_dkdv_set_tile(-1)
    return res, (P, dS, go, qv, kv_)


@pytest.mark.gpu
@pytest.mark.parametrize("cd", DTYPES)
@pytest.mark.parametrize("Lq,Lk,N,H", SHAPES)
def test_attn_dkdv_160_bitwise_equals_128(cd, Lq, Lk, N, H):
    """dK, dV and dQ of the forced 160-row tile are bitwise those of the forced 128-row tile, and
    neither touches the other columns of the packed buffers."""
    res, _ = _run(cd, Lq, Lk, N, H)
    E = 512 * H
    (o128, q128), (o160, q160) = res[128], res[160]
    assert torch.isfinite(o160.float()).all() and torch.isfinite(q160.float()).all()
    assert torch.equal(o128.view(torch.int16), o160.view(torch.int16))
    assert torch.equal(q128.view(torch.int16), q160.view(torch.int16))
    assert (o160[..., :E].float() == 7.0).all()
    assert (q160[..., E:].float() == 7.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("cd", DTYPES)
@pytest.mark.parametrize("Lq,Lk,N,H", SHAPES)
def test_attn_dkdv_160_vs_fp32(cd, Lq, Lk, N, H):
    """The forced 160-row tile against the fp32 einsum products of the same 16-bit inputs, with
    the bounds of test_attn_dkdv_vs_fp32: 2 u max|ref| + 1e-6 L (fp32 accumulation of L products,
    the result rounded once to 16 bits)."""
    res, (P, dS, go, qv, kv_) = _run(cd, Lq, Lk, N, H)
    E = 512 * H
    out, dqo = res[160]
    dk, dv, dq = out[..., E:2 * E], out[..., 2 * E:], dqo[..., :E]
    Pr = P[..., :Lk].float().view(N, H, Lq, Lk)
    dSr = dS[..., :Lk].float().view(N, H, Lq, Lk)
    gor = go.float().view(Lq, N, H, 512)
    qr = qv.float().reshape(Lq, N, H, 512)
    kr = kv_.float().reshape(Lk, N, H, 512)
    dvr = torch.einsum("nhqk,qnhd->knhd", Pr, gor).reshape(Lk, N, E)
    dkr = torch.einsum("nhqk,qnhd->knhd", dSr, qr).reshape(Lk, N, E)
    dqr = torch.einsum("nhqk,knhd->qnhd", dSr, kr).reshape(Lq, N, E)
    u = 2.0 ** -8 if cd == torch.bfloat16 else 2.0 ** -11
    for got, ref, L in ((dv, dvr, Lq), (dk, dkr, Lq), (dq, dqr, Lk)):
        assert torch.isfinite(got.float()).all()
        err = (got.float() - ref).abs().max().item()
        print(f"err {err:.3e} bound {2 * u * ref.abs().max().item() + 1e-6 * L:.3e}")
        assert err <= 2 * u * ref.abs().max().item() + 1e-6 * L, (err, ref.abs().max().item())


def test_attn_dkdv_plan_rule():
    """jmt_attn_dkdv_plan (no GPU call): 160 where 160-row items cost strictly less per head,
    [2 ceil(Lk/KT) ceil(Lq/32) + ceil(Lq/KT) ceil(Lk/32)] chunks x KT rows (the measured time of a
    chunk follows the item's rows, not its staged bytes: DESIGN.md §4 round 9); ties and
    everything else keep 128.

    (161, 161) is two tiles with either size, so 160 rows can only pad more: the rule keeps 128
    there, as any rule that prices an item by its size must (the request for this change listed
    160 for that shape, against its own formula)."""
    lib = _lib.load()
    s = 3 * 512
    plan = lambda Lq, Lk, sdk=s, dq=1: lib.jmt_attn_dkdv_plan(Lq, Lk, 1, sdk, s, s, dq)
    try:
        assert lib.jmt_attn_dkdv_set_tile(0) == _lib.OK
        assert plan(300, 300) == 160
        assert plan(160, 160) == 160
        assert plan(129, 1) == 128
        assert plan(1024, 1024) == 128              # 1120 padded rows against 1024
        assert plan(128, 128) == 128
        assert plan(256, 256) == 128
        assert plan(161, 161) == 128
        assert plan(300, 300, dq=0) == 128          # the row-major P / dS path stays on 128
        # a dK row stride inside the 128-row 32-bit range (< 2^23) and outside the 160-row one
        sl = 7_000_000
        assert 128 * sl * 2 < 2 ** 31 <= 160 * sl * 2
        assert plan(300, 300, sdk=sl) == 128
        # forced tiles: 160 only where it is valid
        assert lib.jmt_attn_dkdv_set_tile(160) == _lib.OK
        assert plan(128, 128) == 160 and plan(300, 300, dq=0) == 128
        assert plan(300, 300, sdk=sl) == 128
        assert lib.jmt_attn_dkdv_set_tile(128) == _lib.OK
        assert plan(300, 300) == 128
        assert lib.jmt_attn_dkdv_set_tile(96) != _lib.OK
    finally:
        lib.jmt_attn_dkdv_set_tile(-1)
