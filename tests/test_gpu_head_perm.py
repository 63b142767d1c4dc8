"""The regressor head kernels (csrc/head.hip) with a row map on y / gy and with their row loads
issued ahead.

jmt_head_fwd_perm / jmt_head_bwd_perm (and the *_perm_drop forms) against the entries without a
map plus a torch permutation, bit for bit (y, dh, dW2, db2): the map only moves where a row of y is
stored and where a row of gy is read, every sum keeps its order.  (P, Q) = (5, 3) stays under one
wave, (16, 4) is exactly one block, (17, 4) crosses a block with a partial last wave, (300, 2) is
the step's T with more blocks.

The batched loads against a float64 reference at rows = 1, 15, 16, 63, 64, 65 (one row, a wave
one short, a full wave, a block one short, a full block, one row into the next block), through
both the plain entries and the identity map P = rows, Q = 1.  Bounds from the number formats
(u32 = 2^-24; u = 2^-8 bf16, 2^-11 fp16):
  y    fp32 sum of 128 exact products and the bias:  |dy|  <= 136 u32 (sum |h||w| + |b|)
  dh   k-term fp32 sum, rounded once to 16 bits:     |ddh| <= u |dh| + (k + 2) u32 sum |gy||w|
       (+ 2^-25 in fp16: half the spacing of its subnormals, below 2^-14)
  dW2  fp32 sum over the rows of fp32 products:      |dW|  <= (rows + 8) u32 sum |gy||h|
  db2  fp32 sum over the rows:                       |db|  <= (rows + 8) u32 sum |gy|
All outputs start as NaN with guard rows behind them; the guards must stay NaN and the rows must
all be written."""
import pytest
import torch

from jmt import functional as JF
from jmt import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
GUARD = 3
U32 = 2.0 ** -24


def _inputs(rows, k, hdt, gdt, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    h = r(rows + GUARD, 256).clamp_(min=0).to(hdt).to(DEV)           # post-ReLU, with zeros
    w2 = [(r(k, 128) / 8).to(hdt).to(DEV) for _ in range(2)]
    b2 = [r(k).to(DEV) for _ in range(2)]
    gy = [r(rows, k).to(gdt).to(DEV) for _ in range(2)]
    dw0 = [r(k, 128).to(DEV) for _ in range(2)]                      # the += targets' old values
    db0 = [r(k).to(DEV) for _ in range(2)]
    return h, w2, b2, gy, dw0, db0


def _nan(rows, cols, dtype):
    return torch.full((rows + GUARD, cols), float("nan"), dtype=dtype, device=DEV)


def _guards_ok(t, rows):
    return bool(torch.isnan(t[rows:]).all()) and not bool(torch.isnan(t[:rows]).any())


def _fwd(h, w2, b2, rows, k, ydt, perm, drop):
    ys = [_nan(rows, k, ydt) for _ in range(2)]
    if drop is None:
        ops.head_fwd(h, 256, rows, k, w2, b2, ys, k, perm=perm)
    else:
        ops.head_fwd_drop(h, 256, rows, k, w2, b2, ys, k, *drop, perm=perm)
    torch.cuda.synchronize()
    assert all(_guards_ok(y, rows) for y in ys)
    return [y[:rows] for y in ys]


def _bwd(h, w2, gy, dw0, db0, rows, k, perm, drop):
    dh = _nan(rows, 256, h.dtype)
    dw = [t.clone() for t in dw0]
    db = [t.clone() for t in db0]
    if drop is None:
        ops.head_bwd(h, 256, rows, k, w2, gy, k, dh, 256, dw, db, perm=perm)
    else:
        ops.head_bwd_drop(h, 256, rows, k, w2, gy, k, dh, 256, dw, db, *drop, perm=perm)
    torch.cuda.synchronize()
    assert _guards_ok(dh, rows)
    return dh[:rows], dw, db


def _row_map(P, Q):
    r = torch.arange(P * Q, device=DEV)
    return (r % P) * Q + r // P


def _check_perm(P, Q, k, hdt, ydt, drop):
    rows = P * Q
    h, w2, b2, gy_l, dw0, db0 = _inputs(rows, k, hdt, ydt, 1000 * P + k)
    idx = _row_map(P, Q)
    assert sorted(idx.tolist()) == list(range(rows))
    y_base = _fwd(h, w2, b2, rows, k, ydt, None, drop)
    y_perm = _fwd(h, w2, b2, rows, k, ydt, (P, Q), drop)
    for yb, yp in zip(y_base, y_perm):
        assert torch.equal(yp[idx], yb)
    # gy_l is in the logical order the perm entry reads; the plain entry gets it in h's order
    gy_m = [g[idx].contiguous() for g in gy_l]
    dh_b, dw_b, db_b = _bwd(h, w2, gy_m, dw0, db0, rows, k, None, drop)
    dh_p, dw_p, db_p = _bwd(h, w2, gy_l, dw0, db0, rows, k, (P, Q), drop)
    assert torch.equal(dh_p, dh_b)
    for a, b in zip(dw_p + db_p, dw_b + db_b):
        assert torch.equal(a, b)
    for a, b in zip(dw_p + db_p, dw0 + db0):
        assert not torch.equal(a, b)                                 # (something was added)


@pytest.mark.parametrize("hdt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("k", [1, 2, 20])
@pytest.mark.parametrize("PQ", [(5, 3), (16, 4), (17, 4), (300, 2)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_perm_entries_match_plain_plus_permutation(PQ, k, hdt):
    _check_perm(PQ[0], PQ[1], k, hdt, torch.float32, None)


@pytest.mark.parametrize("hdt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("k", [1, 20])
def test_perm_entries_16bit_y_and_gy(k, hdt):
    _check_perm(17, 4, k, hdt, hdt, None)


@pytest.mark.parametrize("k", [1, 20])
def test_perm_entries_with_dropout(k):
    """The mask stays a function of h's memory row: the map moves y / gy only."""
    ctr = torch.tensor([12345, 678, 3, 0], dtype=torch.int32, device=DEV)
    _check_perm(17, 4, k, torch.bfloat16, torch.float32, (0.3, 0.5, ctr))
    # and the mask does something: the dropped forward differs from the plain one
    h, w2, b2, _, _, _ = _inputs(68, k, torch.bfloat16, torch.float32, 5)
    assert not torch.equal(_fwd(h, w2, b2, 68, k, torch.float32, (17, 4), None)[0],
                           _fwd(h, w2, b2, 68, k, torch.float32, (17, 4), (0.3, 0.5, ctr))[0])


@pytest.mark.parametrize("ident", [False, True], ids=["plain", "identity_map"])
@pytest.mark.parametrize("hdt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("k", [1, 20])
@pytest.mark.parametrize("rows", [1, 15, 16, 63, 64, 65])
def test_batched_loads_against_float64(rows, k, hdt, ident):
    u = 2.0 ** -8 if hdt == torch.bfloat16 else 2.0 ** -11
    tiny = 0.0 if hdt == torch.bfloat16 else 2.0 ** -25
    h, w2, b2, gy, dw0, db0 = _inputs(rows, k, hdt, torch.float32, 77 * rows + k)
    perm = (rows, 1) if ident else None
    ys = _fwd(h, w2, b2, rows, k, torch.float32, perm, None)
    dh, dw, db = _bwd(h, w2, gy, dw0, db0, rows, k, perm, None)
    hd = h[:rows].double()
    for g in range(2):
        hg, W, G = hd[:, 128 * g:128 * (g + 1)], w2[g].double(), gy[g].double()
        y64 = hg @ W.T + b2[g].double()
        ybound = 136 * U32 * (hg.abs() @ W.abs().T + b2[g].double().abs())
        assert bool(((ys[g].double() - y64).abs() <= ybound).all())
        dh64 = (G @ W) * (hg > 0)
        dbound = u * dh64.abs() + (k + 2) * U32 * (G.abs() @ W.abs()) + tiny
        assert bool(((dh[:, 128 * g:128 * (g + 1)].double() - dh64).abs() <= dbound).all())
        dw64 = G.T @ hg
        wbound = (rows + 8) * U32 * (G.abs().T @ hg.abs() + dw0[g].double().abs())
        assert bool(((dw[g].double() - dw0[g].double() - dw64).abs() <= wbound).all())
        bbound = (rows + 8) * U32 * (G.abs().sum(0) + db0[g].double().abs())
        assert bool(((db[g].double() - db0[g].double() - G.sum(0)).abs() <= bbound).all())


def test_mlp_pair_takes_the_map_and_returns_contiguous_outputs():
    """MLPPairFn on a seq-first view of batch-first rows: logically contiguous outputs through the
    row map, bit-identical (outputs, input and parameter gradients) to the switch-off route,
    whose outputs keep x's transposed row order."""
    from jmt.nn import MLP
    torch.manual_seed(3)
    T, B, E = 37, 6, 1024
    va, aa = MLP(E, 128, 1, dropout=0.0).to(DEV), MLP(E, 128, 1, dropout=0.0).to(DEV)
    x0 = torch.randn(B, T, E, device=DEV).permute(1, 0, 2)
    res = {}
    try:
        for on in (False, True):
            JF.set_head_perm(on)
            x = x0.clone().requires_grad_(True)
            assert x.stride() == x0.stride()
            for p in list(va.parameters()) + list(aa.parameters()):
                p.grad = None
            with JF.compute_mode(torch.bfloat16):
                v, a = JF.mlp_pair(x, va, aa, out_dtype=torch.float32)
                gv = torch.linspace(-1, 1, v.numel(), device=DEV).view_as(v)
                ga = torch.cos(torch.arange(a.numel(), device=DEV, dtype=torch.float32)).view_as(a)
                ((v * gv).sum() + (a * ga).sum()).backward()
            torch.cuda.synchronize()
            res[on] = (v.detach(), a.detach(), x.grad.detach(),
                       [p.grad.clone() for m in (va, aa) for p in m.parameters()])
    finally:
        JF.set_head_perm(True)
    assert res[True][0].is_contiguous() and res[True][1].is_contiguous()
    assert not res[False][0].is_contiguous()
    for r, g in zip(res[False][:3], res[True][:3]):
        assert r.shape == g.shape and torch.equal(r, g)
    for r, g in zip(res[False][3], res[True][3]):
        assert torch.equal(r, g)
