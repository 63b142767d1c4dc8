"""Every branch of csrc/ccc.hip against the float64 references of tests/loss_ref.py (bound per
element: one rounding of the stored type + K unit cond, K measured on the CPU), through jmt.ops:
the CCC statistics / finish / backward kernels, the rank combination, CELoss, label digitizing
and mask compaction, and a thin layer through the loss modules.

Outputs are pre-filled with NaN (a sentinel for the integer ones) and every buffer, inputs
included, lies between two guard regions: inputs carry NaN there, so a read past either end
poisons a statistic, and the outputs' guards must come back untouched."""
import functools
import math
import warnings

import numpy as np
import pytest
import torch

from jmt import _lib, ops
from tests import loss_ref as R
from tests.loss_ref import BF, DT_NAME, E24, F64, FS, HI, IGNORE, LO

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = math.nan
GUARD = 64
SENTINEL = -7
I64 = torch.int64
warnings.filterwarnings("ignore", message="std\\(\\): degrees of freedom")

# largest error / bound per family over this run (printed by the last test of the file)
RATIOS = {}


def _note(family, ratio):
    RATIOS[family] = max(RATIOS.get(family, 0.0), ratio)


def _check(family, got, ref, cond, od, K, un, what):
    # 16-bit outputs apart: there the rounding to the stored type alone reaches the bound
    _note(family + ("" if od in (FS, F64) else ", 16-bit output"),
          R.check(got, ref, cond, od, K, un, what))


# ------------------------------------------------------------------ buffers
def _buf(shape, dtype, data=None, fill=NAN):
    """A contiguous tensor of `shape` between two guards of GUARD elements, everything `fill`;
    `data` (CPU, same shape and dtype) copied in.  The view's data_ptr() is the operand."""
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    n = int(np.prod(shape))
    flat = torch.full((GUARD + n + GUARD,), fill, dtype=dtype, device=DEV)
    view = flat[GUARD:GUARD + n].view(shape)
    if data is not None:
        assert tuple(data.shape) == shape and data.dtype == dtype, (data.shape, data.dtype)
        view.copy_(data.to(DEV))
    view.gflat = flat
    view.gfill = fill
    return view


def _same(t, fill):
    return bool(torch.isnan(t).all()) if isinstance(fill, float) and math.isnan(fill) else \
        bool((t == fill).all())


def _guards_ok(*views):
    for v in views:
        n = v.numel()
        assert _same(v.gflat[:GUARD], v.gfill), "guard before the buffer written"
        assert _same(v.gflat[GUARD + n:], v.gfill), "guard after the buffer written"


def _untouched(*views):
    for v in views:
        assert _same(v.gflat, v.gfill), "output written by a rejected call"


def _id(c):
    if isinstance(c, tuple) and hasattr(c, "_fields"):
        return "-".join(DT_NAME.get(v, str(v)) if not isinstance(v, str) else v for v in c)
    return DT_NAME.get(c, str(c))


def _scalar(v):
    return torch.full((1,), v, dtype=FS, device=DEV)


# ------------------------------------------------------------------ CCC: one rank
def _ccc_case(c):
    pred, y = R.ccc_inputs(c)
    refs = {gl: R.ccc_reference(c.kind, [pred], [y], c.k, IGNORE, LO, HI, 1, c.eps, gl)
            for gl in (1.0, R.GRAD_LOSS)}
    return pred, y, refs


def _finish(kind, world, stats_all, bs, eps, ref, k, what):
    """jmt_ccc_finish on `stats_all` against `ref`: loss, coef (its documented zeros included),
    and the same call with `add`: fp32(add + loss), bit for bit.  Returns coef."""
    loss, coef = _buf(1, FS), _buf(8, F64)
    ops.ccc_finish(kind, world, stats_all, bs, eps, loss, coef)
    loss2, coef2 = _buf(1, FS), _buf(8, F64)
    add = _scalar(R.ADD)
    ops.ccc_finish(kind, world, stats_all, bs, eps, loss2, coef2, add=add)
    torch.cuda.synchronize()
    _check("ccc_loss", loss[0], ref.loss, ref.c_loss, FS, R.K_CCC_LOSS, E24, what + " loss")
    _check("stats", coef, ref.coef, ref.c_coef, F64, R.K_STATS, R.unit(k), what + " coef")
    got = coef.cpu()
    assert float(got[5]) == float(ref.coef[5]) and float(got[6]) == 0 and float(got[7]) == 0
    want = add.cpu() + loss.cpu()                        # one fp32 addition, NaN stays NaN
    if math.isnan(float(want)):
        assert math.isnan(float(loss2)), what
    else:
        assert torch.equal(loss2.cpu().view(torch.int32), want.view(torch.int32)), \
            (what, float(loss2), float(want))
    assert torch.equal(coef2.cpu().view(I64), got.view(I64))
    _guards_ok(loss, coef, loss2, coef2)
    return coef


def _backward(kind, k, predv, labv, coef, pred_dt, refs, r, what):
    """jmt_ccc_bwd of rank r without and with an upstream gradient."""
    for gl in (1.0, R.GRAD_LOSS):
        ref = refs[gl]
        dpred = _buf(tuple(predv.shape), pred_dt)
        ops.ccc_bwd(kind, predv, labv, k, IGNORE, LO, HI, coef,
                    None if gl == 1.0 else _scalar(gl), dpred)
        torch.cuda.synchronize()
        _check("ccc_grad, k = 1" if k == 1 else "ccc_grad, k > 1", dpred, ref.grads[r],
               ref.c_grads[r], pred_dt, R.K_CCC_GRAD, R.unit(k),
               f"{what} dpred (grad_loss {gl})")
        _guards_ok(dpred)


@pytest.mark.parametrize("c", R.CCC_CASES + R.CCC_GRID_CASES, ids=_id)
def test_ccc_stats_finish_bwd(c):
    pred, y, refs = _ccc_case(c)
    ref = refs[1.0]
    predv, labv = _buf(tuple(pred.shape), c.dt, pred), _buf(c.n, FS, y)
    stats = _buf(8, F64)
    ops.ccc_stats(c.kind, predv, labv, c.k, IGNORE, LO, HI, stats)
    torch.cuda.synchronize()
    _check("stats", stats, ref.st.s, ref.st.c, F64, R.K_STATS, R.unit(c.k), "stats")
    got = stats.cpu()
    assert float(got[0]) == float(ref.st.s[0]) and float(got[6]) == c.n and float(got[7]) == 0
    _guards_ok(stats)
    coef = _finish(c.kind, 1, stats, 1, c.eps, ref, c.k, "finish")
    _backward(c.kind, c.k, predv, labv, coef, c.dt, refs, 0, "bwd")


# ------------------------------------------------------------------ CCC: rank combination
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("rc", R.RANK_CASES, ids=lambda rc: rc.name)
def test_ccc_rank_combination(rc, kind):
    """World 1, 2 and 8 with unequal ranks against the statistics of the concatenated batch:
    loss, coef and every rank's gradient, for each bs."""
    data = R.rank_inputs(rc, kind)
    preds, labels = [d[0] for d in data], [d[1] for d in data]
    world = len(data)
    eps = R.EPS if kind == 0 else 0.0
    dev = [(_buf(p.numel(), FS, p), _buf(y.numel(), FS, y)) for p, y in data]
    stats_all = _buf(8 * world, F64)
    for r, (pv, yv) in enumerate(dev):
        ops.ccc_stats(kind, pv, yv, 1, IGNORE, LO, HI, stats_all[8 * r:8 * r + 8])
    torch.cuda.synchronize()
    _guards_ok(stats_all)
    for r, (p, y) in enumerate(data):
        one = R.ccc_stats(kind, p, y, 1, IGNORE, LO, HI)
        _check("stats", stats_all[8 * r:8 * r + 8], one.s, one.c, F64, R.K_STATS, R.E53,
               f"rank {r} stats")
    for bs in (R.RANK_BS if kind == 1 else (1,)):
        refs = {gl: R.ccc_reference(kind, preds, labels, 1, IGNORE, LO, HI, bs, eps, gl)
                for gl in (1.0, R.GRAD_LOSS)}
        coef = _finish(kind, world, stats_all, bs, eps, refs[1.0], 1, f"bs {bs}")
        for r, (pv, yv) in enumerate(dev):
            _backward(kind, 1, pv, yv, coef, FS, refs, r, f"bs {bs} rank {r}")


# ------------------------------------------------------------------ CELoss
@functools.lru_cache(maxsize=4)
def _ce_case(c, bad_label=False):
    x, y, w = R.ce_inputs(c, bad_label)
    cls = R.ce_bins(y, c.k, c.lo, c.hi)
    st = R.ce_stats(x, cls, w)
    return x, y, w, cls, st, R.ce_loss([st])


def _ce_labels(labv, k, lo, hi):
    out = _buf(labv.numel(), I64, fill=SENTINEL)
    _lib.call("jmt_ce_labels", labv.numel(), k, labv.data_ptr(), lo, hi, out.data_ptr(),
              ops.stream())
    return out


def _ce_backward(c, xv, labv, wv, coef, x, cls, w, sw, what):
    for gl in (1.0, R.GRAD_LOSS):
        g, cg = R.ce_grad(x, cls, w, sw, gl)
        dx = _buf((c.n, c.k), c.dt)
        ops.ce_bwd(xv, labv, c.k, c.lo, c.hi, wv, coef, None if gl == 1.0 else _scalar(gl), dx)
        torch.cuda.synchronize()
        _check("ce_grad", dx, g, cg, c.dt, R.K_CE_GRAD, E24, f"{what} dx (grad_loss {gl})")
        _guards_ok(dx)


@pytest.mark.parametrize("c", R.CE_CASES + [R.CE_GRID_CASE], ids=_id)
def test_ce_labels_stats_finish_bwd(c):
    x, y, w, cls, st, fin = _ce_case(c)
    xv, labv = _buf((c.n, c.k), c.dt, x), _buf(c.n, FS, y)
    wv = _buf(c.k, FS, w) if w is not None else None
    lab = _ce_labels(labv, c.k, c.lo, c.hi)
    stats, loss, coef = _buf(4, F64), _buf(1, FS), _buf(1, F64)
    ops.ce_stats(xv, labv, c.k, c.lo, c.hi, wv, stats)
    ops.ce_finish(1, stats, loss, coef)
    torch.cuda.synchronize()
    assert torch.equal(lab.cpu(), cls)
    _check("ce_loss", stats[:2], st.s[:2], st.c[:2], F64, R.K_CE_LOSS, E24, "stats")
    assert float(stats[2]) == 0 and float(stats[3]) == 0
    _check("ce_loss", loss[0], fin.loss, fin.c_loss, FS, R.K_CE_LOSS, E24, "loss")
    _check("ce_loss", coef[0], fin.coef, fin.c_coef, F64, R.K_CE_LOSS, E24, "coef")
    _guards_ok(lab, stats, loss, coef)
    _ce_backward(c, xv, labv, wv, coef, x, cls, w, st.s[1], "bwd")


@pytest.mark.parametrize("c", [R._ce(1025, 7), R._ce(4133, 64, BF, "rand", R.CE_RANGES[2])],
                         ids=_id)
def test_ce_label_below_range(c):
    """One label an fp32 ulp below lo: bin -1, counted in stats[2] and left out of the sums; the
    loss and coef are NaN, hence the whole gradient; with a finite coef only that row is NaN."""
    x, y, w, cls, st, fin = _ce_case(c, True)
    row = c.n // 2
    assert int(cls[row]) == -1 and int((cls < 0).sum()) == 1 and math.isnan(float(fin.loss))
    xv, labv = _buf((c.n, c.k), c.dt, x), _buf(c.n, FS, y)
    wv = _buf(c.k, FS, w) if w is not None else None
    lab = _ce_labels(labv, c.k, c.lo, c.hi)
    stats, loss, coef = _buf(4, F64), _buf(1, FS), _buf(1, F64)
    ops.ce_stats(xv, labv, c.k, c.lo, c.hi, wv, stats)
    ops.ce_finish(1, stats, loss, coef)
    dx = _buf((c.n, c.k), c.dt, fill=1.0)
    ops.ce_bwd(xv, labv, c.k, c.lo, c.hi, wv, coef, None, dx)
    torch.cuda.synchronize()
    assert torch.equal(lab.cpu(), cls)
    _check("ce_loss", stats[:2], st.s[:2], st.c[:2], F64, R.K_CE_LOSS, E24, "stats")
    assert float(stats[2]) == 1 and float(stats[3]) == 0
    assert math.isnan(float(loss)) and math.isnan(float(coef))          # NaN == NaN, explicitly
    assert bool(torch.isnan(dx).all())
    _guards_ok(lab, stats, loss, coef, dx)
    good = _buf(1, F64, (1.0 / st.s[1]).reshape(1))
    _ce_backward(c, xv, labv, wv, good, x, cls, w, st.s[1], "finite coef")


@pytest.mark.parametrize("world", [2, 8])
def test_ce_finish_sums_the_ranks(world):
    """ce_finish over unequal ranks (one of them empty) == the whole batch; a rank's backward
    with the combined coef is its slice of the whole batch's gradient."""
    c = R._ce(4133, 7, w="rand")
    x, y, w, cls, st, fin = _ce_case(c)
    cuts = [0, 1500, 4133] if world == 2 else [0, 1, 64, 64, 1100, 2124, 2125, 4000, 4133]
    wv = _buf(c.k, FS, w)
    stats_all = _buf(4 * world, F64)
    parts = []
    for r in range(world):
        a, b = cuts[r], cuts[r + 1]
        parts.append((_buf((b - a, c.k), c.dt, x[a:b]), _buf(b - a, FS, y[a:b])))
        ops.ce_stats(*parts[-1], c.k, c.lo, c.hi, wv, stats_all[4 * r:4 * r + 4])
    loss, coef = _buf(1, FS), _buf(1, F64)
    ops.ce_finish(world, stats_all, loss, coef)
    torch.cuda.synchronize()
    _check("ce_loss", loss[0], fin.loss, fin.c_loss, FS, R.K_CE_LOSS, E24, "loss")
    _check("ce_loss", coef[0], fin.coef, fin.c_coef, F64, R.K_CE_LOSS, E24, "coef")
    _guards_ok(stats_all, loss, coef)
    g, cg = R.ce_grad(x, cls, w, st.s[1], R.GRAD_LOSS)
    for r, (xv, labv) in enumerate(parts):
        a, b = cuts[r], cuts[r + 1]
        dx = _buf((b - a, c.k), c.dt)
        ops.ce_bwd(xv, labv, c.k, c.lo, c.hi, wv, coef, _scalar(R.GRAD_LOSS), dx)
        torch.cuda.synchronize()
        _check("ce_grad", dx, g[a:b], cg[a:b], c.dt, R.K_CE_GRAD, E24, f"rank {r} dx")
        _guards_ok(dx)


# ------------------------------------------------------------------ mask_indices
@pytest.mark.parametrize("n,pat", R.MASK_CASES)
def test_mask_indices(n, pat):
    y = R.mask_inputs(n, pat)
    ref = R.mask_indices(y, IGNORE)
    labv = _buf(n, FS, y)
    idx, cnt = _buf(max(n, 1), I64, fill=SENTINEL), _buf(1, I64, fill=SENTINEL)
    _lib.call("jmt_mask_indices", n, labv.data_ptr(), IGNORE, idx.data_ptr(), cnt.data_ptr(),
              ops.stream())
    torch.cuda.synchronize()
    assert int(cnt) == ref.size
    got = idx.cpu().numpy()
    np.testing.assert_array_equal(got[:ref.size], ref)
    assert (got[ref.size:] == SENTINEL).all(), "written past the count"
    _guards_ok(idx, cnt)
    # the public wrapper allocates its own outputs
    idx2, cnt2 = ops.mask_indices(labv, IGNORE)
    assert int(cnt2) == ref.size
    np.testing.assert_array_equal(idx2[:ref.size].cpu().numpy(), ref)


# ------------------------------------------------------------------ argument checks
@pytest.mark.parametrize("k", [0, 65])
def test_ccc_rejects_unsupported_k(k):
    n = 8
    pred, lab = _buf(n * max(k, 1), FS, fill=0.5), _buf(n, FS, fill=0.25)
    stats, dpred, coef = _buf(8, F64), _buf(n * max(k, 1), FS), _buf(8, F64, fill=1.0)
    with pytest.raises(_lib.JMTError, match=r"\(-1\)"):
        ops.ccc_stats(0, pred, lab, k, IGNORE, LO, HI, stats)
    with pytest.raises(_lib.JMTError, match=r"\(-1\)"):
        ops.ccc_bwd(0, pred, lab, k, IGNORE, LO, HI, coef, None, dpred)
    torch.cuda.synchronize()
    _untouched(stats, dpred)


@pytest.mark.parametrize("k", [0, 1, 65])
def test_ce_rejects_unsupported_k(k):
    n = 8
    x, lab = _buf(n * max(k, 1), FS, fill=0.5), _buf(n, FS, fill=0.25)
    stats, dx, coef = _buf(4, F64), _buf(n * max(k, 1), FS), _buf(1, F64, fill=1.0)
    out = _buf(n, I64, fill=SENTINEL)
    with pytest.raises(_lib.JMTError, match=r"\(-1\)"):
        _lib.call("jmt_ce_stats", ops.dt(x), n, k, x.data_ptr(), lab.data_ptr(), LO, HI, None,
                  stats.data_ptr(), ops.stream())
    with pytest.raises(_lib.JMTError, match=r"\(-1\)"):
        _lib.call("jmt_ce_bwd", ops.dt(x), n, k, x.data_ptr(), lab.data_ptr(), LO, HI, None,
                  coef.data_ptr(), None, dx.data_ptr(), ops.stream())
    with pytest.raises(_lib.JMTError, match=r"\(-1\)"):
        _lib.call("jmt_ce_labels", n, k, lab.data_ptr(), LO, HI, out.data_ptr(), ops.stream())
    torch.cuda.synchronize()
    _untouched(stats, dx, out)


# ------------------------------------------------------------------ through the loss modules
MODULE_N = (R.TAIL + 1, R.TAIL + 1024 + 37)
UP = R.GRAD_LOSS           # upstream gradient of the modules' backward


def _strided(t):
    """The same values as a non-contiguous tensor (every second element of a wider buffer)."""
    wide = torch.zeros(t.shape + (2,), dtype=t.dtype, device=DEV)
    wide[..., 0] = t.to(DEV)
    v = wide[..., 0]
    assert not v.is_contiguous() or v.numel() <= 1
    return v


def _module_inputs(n, k, kind):
    """Logits (n, k) as a transposed (k, n) view and labels as float64, non-contiguous (1, n);
    the labels hold fp32 values, so the cast the losses make of them is exact."""
    c = R._ccc(kind, n, k)
    pred, y = R.ccc_inputs(c, "module")
    if k == 1:
        x = _strided(pred).requires_grad_(True)
    else:
        x = pred.t().contiguous().to(DEV).t().requires_grad_(True)
        assert not x.is_contiguous() and x.shape == (n, k)
    return c, pred, y, x, _strided(y.double())


@pytest.mark.parametrize("n", MODULE_N)
def test_module_ccc_digitized(n):
    from losses.loss import CCCLoss
    k = 5
    c, pred, y, x, yd = _module_inputs(n, k, 0)
    loss = CCCLoss(k)(x, yd.view(1, n))
    (loss * UP).backward()
    ref = R.ccc_reference(0, [pred], [y], k, IGNORE, LO, HI, 1, R.EPS, UP)
    _check("ccc_loss", loss.detach(), ref.loss, ref.c_loss, FS, R.K_CCC_LOSS, E24, "loss")
    assert x.grad.shape == (n, k)
    _check("ccc_grad, k > 1", x.grad, ref.grads[0], ref.c_grads[0], FS, R.K_CCC_GRAD, E24, "grad")


@pytest.mark.parametrize("n", MODULE_N)
def test_module_ccc_ignore_1d(n):
    """losses.CCCLoss.CCCLoss on 1-D strided predictions: bs is the pre-mask size."""
    from losses.CCCLoss import CCCLoss
    c, pred, y, x, yd = _module_inputs(n, 1, 1)
    assert x.shape == (n,) and int((y == IGNORE).sum()) > 0
    loss = CCCLoss(IGNORE)(x, yd)
    (loss * UP).backward()
    ref = R.ccc_reference(1, [pred], [y], 1, IGNORE, LO, HI, -1, 0.0, UP)
    _check("ccc_loss", loss.detach(), ref.loss, ref.c_loss, FS, R.K_CCC_LOSS, E24, "loss")
    assert x.grad.shape == (n,)
    _check("ccc_grad, k = 1", x.grad, ref.grads[0], ref.c_grads[0], FS, R.K_CCC_GRAD, R.E53,
           "grad")


def _ce_module_ref(pred, y, k, gl):
    cls = R.ce_bins(y, k, LO, HI)
    st = R.ce_stats(pred, cls, None)
    g, cg = R.ce_grad(pred, cls, None, st.s[1], gl)
    return R.ce_loss([st]), g, cg


@pytest.mark.parametrize("n", MODULE_N)
def test_module_celoss(n):
    from losses.loss import CELoss
    k = 5
    c, pred, y, x, yd = _module_inputs(n, k, 0)
    loss = CELoss(k)(x, yd.view(1, n))
    (loss * UP).backward()
    fin, g, cg = _ce_module_ref(pred, y, k, UP)
    _check("ce_loss", loss.detach(), fin.loss, fin.c_loss, FS, R.K_CE_LOSS, E24, "loss")
    assert x.grad.shape == (n, k)
    _check("ce_grad", x.grad, g, cg, FS, R.K_CE_GRAD, E24, "grad")


@pytest.mark.parametrize("n", MODULE_N)
def test_module_ccc_ce(n):
    """alpha ccc + beta ce with alpha, beta exact in fp32: each part within its own bound, plus
    one fp32 rounding for each product and for the sum torch forms of them."""
    from losses.loss import CCC_CE_Loss
    k, alpha, beta = 5, 0.25, 0.75
    c, pred, y, x, yd = _module_inputs(n, k, 0)
    loss = CCC_CE_Loss(k, alpha=alpha, beta=beta)(x, yd.view(1, n))
    (loss * UP).backward()
    r1 = R.ccc_reference(0, [pred], [y], k, IGNORE, LO, HI, 1, R.EPS, UP * alpha)
    fin, g, cg = _ce_module_ref(pred, y, k, UP * beta)
    want = alpha * r1.loss + beta * fin.loss
    tol = (alpha * R.bound(r1.loss, r1.c_loss, FS, R.K_CCC_LOSS, E24)
           + beta * R.bound(fin.loss, fin.c_loss, FS, R.K_CE_LOSS, E24) + E24 * want.abs())
    assert abs(float(loss) - float(want)) <= float(tol), (float(loss), float(want), float(tol))
    assert x.grad.shape == (n, k)
    gw = r1.grads[0] + g
    gtol = (R.bound(r1.grads[0], r1.c_grads[0], FS, R.K_CCC_GRAD, E24)
            + R.bound(g, cg, FS, R.K_CE_GRAD, E24) + E24 * gw.abs())
    err = (x.grad.cpu().double() - gw).abs()
    assert bool((err <= gtol).all()), float((err / gtol).max())
    _note("module_sum", float((err / gtol).max()))


def test_report_largest_ratios():
    """Largest error / bound per family over the tests of this file that ran before (DESIGN.md
    records the figures of a whole run)."""
    for fam, r in sorted(RATIOS.items()):
        print(f"largest error / bound, {fam}: {r:.4f}")
    assert all(r <= 1.0 for r in RATIOS.values())
