"""Every dispatch branch of csrc/rowops.hip against the float64 references of tests/rowops_ref.py
(bound: one rounding of the stored type + K 2^-24 cond per element, K measured on the CPU).

Outputs are pre-filled with NaN (or known values where the result accumulates); every case checks
the values, that the padding columns [D, ld) and a guard row after the last stay untouched, and
for softmax that the padding is exactly zero.  Inputs carry NaN in their padding too, so a kernel
that reads past a row's end fails the value check."""
import functools
import math

import pytest
import torch

from jmt import _lib, ops
from tests import rowops_ref as R
from tests.rowops_ref import BF, FH, FS, F64, DT_NAME

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = math.nan


# ------------------------------------------------------------------ buffers
def _buf(rows, D, ld, dtype, data=None, off=0, fill=NAN):
    """(rows + 1) x ld elements behind `off` leading ones, all `fill`; `data` (rows x D, CPU) in
    the first D columns.  Returns the (rows + 1, ld) view: its data_ptr() is the operand."""
    flat = torch.full((off + (rows + 1) * ld,), fill, dtype=dtype, device=DEV)
    view = flat[off:].view(rows + 1, ld)
    if data is not None:
        assert data.shape == (rows, D) and data.dtype == dtype
        view[:rows, :D] = data.to(DEV)
    view.base = flat
    view.lead = off
    return view


def _vec(n, data=None, off=0, fill=NAN):
    """fp32 vector of n behind `off` floats and before 8 guard floats."""
    flat = torch.full((off + n + 8,), fill, dtype=FS, device=DEV)
    v = flat[off:off + n]
    if data is not None:
        v.copy_(data.to(DEV))
    v.base = flat
    v.lead = off
    return v


def _same(t, fill):
    return bool(torch.isnan(t).all()) if math.isnan(fill) else bool((t == fill).all())


def _untouched(view, rows, D, fill=NAN):
    assert _same(view[:rows, D:], fill), "padding columns written"
    assert _same(view[rows:], fill), "guard row written"
    assert _same(view.base[:view.lead], fill), "lead written"


def _vec_untouched(v, fill=NAN):
    n = v.numel()
    assert _same(v.base[:v.lead], fill) and _same(v.base[v.lead + n:], fill), "vector guard written"


def _d(t):
    return None if t is None else t.to(F64)


def _case_id(c):
    if isinstance(c, tuple) and hasattr(c, "_fields"):
        return "-".join(DT_NAME.get(v, str(v)) if not isinstance(v, str) else (v or "_")
                        for v in c)
    return None


# ------------------------------------------------------------------ LayerNorm
class NS(dict):
    __getattr__ = dict.__getitem__


@functools.lru_cache(maxsize=None)
def _ln_ref(rows, D, dt, gdt, with_r, tag=""):
    """Operands (stored dtypes, CPU) and the float64 forward / backward of one operand set; the
    backward reads the reference statistics rounded to fp32."""
    x, r, gamma, beta, dy = R.ln_inputs(rows, D, dt, gdt, with_r, tag)
    f = R.ln_fwd(_d(x), _d(r), _d(gamma), _d(beta), R.LN_EPS)
    mean, rstd = f.mean.float(), f.rstd.float()
    b = R.ln_bwd(_d(x), _d(r), _d(dy), _d(mean), _d(rstd), _d(gamma))
    return NS(x=x, r=r, gamma=gamma, beta=beta, dy=dy, f=f, b=b, mean=mean, rstd=rstd)


def _ln_operands(c, o):
    """Device operands of case c: x (offset by one element for "xoff"), r, gamma ("goff": one
    float off its 16-B alignment)."""
    x = _buf(c.rows, c.D, c.ld, c.dt, o.x, off=1 if c.force == "xoff" else 0)
    r = _buf(c.rows, c.D, c.ld, c.dt, o.r) if o.r is not None else None
    gamma = _vec(c.D, o.gamma, off=1 if c.force == "goff" else 0)
    return x, r, gamma


@pytest.mark.parametrize("with_r", [False, True], ids=["nor", "r"])
@pytest.mark.parametrize("c", R.LN_CASES, ids=_case_id)
def test_layernorm_fwd(c, with_r):
    o = _ln_ref(c.rows, c.D, c.dt, c.gdt, with_r)
    x, r, gamma = _ln_operands(c, o)
    beta = _vec(c.D, o.beta)
    y = _buf(c.rows, c.D, c.ld, c.ydt)
    mean, rstd = _vec(c.rows), _vec(c.rows)
    ops.layernorm_fwd(x, c.ld, r, c.ld, gamma, beta, R.LN_EPS, y, c.ld, mean, rstd, c.rows, c.D)
    torch.cuda.synchronize()
    R.check(y[:c.rows, :c.D], o.f.y, o.f.c_y, c.ydt, R.K_LN, "y")
    R.check(mean, o.f.mean, o.f.c_mean, FS, R.K_LN, "mean")
    R.check(rstd, o.f.rstd, o.f.c_rstd, FS, R.K_LN, "rstd")
    _untouched(y, c.rows, c.D)
    _vec_untouched(mean)
    _vec_untouched(rstd)


def _acc_out(D, beta_acc, seed):
    """An accumulating fp32 output: NaN-filled for beta_acc = 0 (the old contents must not be
    read), known non-zero contents for beta_acc = 1.  Returns (device vector, old or None)."""
    if not beta_acc:
        return _vec(D), None
    old = torch.randn(D, generator=torch.Generator().manual_seed(seed)) + 2
    return _vec(D, old), _d(old)


def _check_acc(got, old, val, cond, what):
    if old is not None:
        val, cond = R.acc(old, val, cond)
    R.check(got, val, cond, FS, R.K_LN, what)
    _vec_untouched(got)


@pytest.mark.parametrize("beta_acc", [0, 1], ids=["set", "acc"])
@pytest.mark.parametrize("with_r", [False, True], ids=["nor", "r"])
@pytest.mark.parametrize("c", R.LN_CASES, ids=_case_id)
def test_layernorm_bwd(c, with_r, beta_acc):
    o = _ln_ref(c.rows, c.D, c.dt, c.gdt, with_r)
    x, r, gamma = _ln_operands(c, o)
    dy = _buf(c.rows, c.D, c.ld, c.gdt, o.dy)
    dx = _buf(c.rows, c.D, c.ld, c.ddt)
    dgamma, og = _acc_out(c.D, beta_acc, 1)
    dbeta, ob = _acc_out(c.D, beta_acc, 2)
    ops.layernorm_bwd(x, c.ld, r, c.ld, dy, c.ld, _vec(c.rows, o.mean), _vec(c.rows, o.rstd),
                      gamma, dx, c.ld, dgamma, dbeta, beta_acc, c.rows, c.D)
    torch.cuda.synchronize()
    R.check(dx[:c.rows, :c.D], o.b.dx, o.b.c_dx, c.ddt, R.K_LN, "dx")
    _untouched(dx, c.rows, c.D)
    _check_acc(dgamma, og, o.b.dgamma, o.b.c_dgamma, "dgamma")
    _check_acc(dbeta, ob, o.b.dbeta, o.b.c_dbeta, "dbeta")


@pytest.mark.parametrize("beta_acc", [0, 1], ids=["set", "acc"])
@pytest.mark.parametrize("with_r", [False, True], ids=["nor", "r"])
@pytest.mark.parametrize("c", R.LN_DSUM_CASES, ids=_case_id)
def test_layernorm_bwd_dsum(c, with_r, beta_acc):
    o = _ln_ref(c.rows, c.D, c.dt, c.gdt, with_r)
    x, r, gamma = _ln_operands(c, o)
    dy = _buf(c.rows, c.D, c.ld, c.gdt, o.dy)
    dx = _buf(c.rows, c.D, c.ld, c.ddt)
    dgamma, og = _acc_out(c.D, beta_acc, 1)
    dbeta, ob = _acc_out(c.D, beta_acc, 2)
    dsum, os_ = _acc_out(c.D, beta_acc, 3)
    part = ops.layernorm_bwd_dsum(x, c.ld, r, c.ld, dy, c.ld, _vec(c.rows, o.mean),
                                  _vec(c.rows, o.rstd), gamma, dx, c.ld, dgamma, dbeta, dsum,
                                  beta_acc, c.rows, c.D)
    torch.cuda.synchronize()
    assert part is not None
    R.check(dx[:c.rows, :c.D], o.b.dx, o.b.c_dx, c.ddt, R.K_LN, "dx")
    _untouched(dx, c.rows, c.D)
    _check_acc(dgamma, og, o.b.dgamma, o.b.c_dgamma, "dgamma")
    _check_acc(dbeta, ob, o.b.dbeta, o.b.c_dbeta, "dbeta")
    _check_acc(dsum, os_, o.b.dsum, o.b.c_dsum, "dsum")


@pytest.mark.parametrize("D,ld", [(256, 256), (512, 513)], ids=["D256", "ld513"])
def test_layernorm_bwd_dsum_uncovered_layout_writes_nothing(D, ld):
    """A width or a row stride outside the vector kernels: None, all four outputs as they were."""
    c = R._ln(19, D, BF, ld=ld)
    o = _ln_ref(c.rows, c.D, c.dt, c.gdt, True)
    x, r, gamma = _ln_operands(c, o)
    dy = _buf(c.rows, c.D, c.ld, c.gdt, o.dy)
    dx = _buf(c.rows, c.D, c.ld, c.ddt, fill=5.0)
    outs = [_vec(c.D, fill=7.0) for _ in range(3)]
    part = ops.layernorm_bwd_dsum(x, c.ld, r, c.ld, dy, c.ld, _vec(c.rows, o.mean),
                                  _vec(c.rows, o.rstd), gamma, dx, c.ld, *outs, 1, c.rows, c.D)
    torch.cuda.synchronize()
    assert part is None
    assert bool((dx.base == 5.0).all()) and all(bool((v.base == 7.0).all()) for v in outs)


def test_layernorm_rejects_rows_wider_than_2048():
    """The generic kernels hold a row in 32 registers per lane: D = 2049 is an argument error."""
    c = R._ln(3, 2049, FS)
    x = _buf(c.rows, c.D, c.ld, FS, torch.ones(c.rows, c.D))
    y = _buf(c.rows, c.D, c.ld, FS)
    gamma, beta, mean, rstd = _vec(c.D, fill=1.0), _vec(c.D, fill=0.0), _vec(c.rows), _vec(c.rows)
    with pytest.raises(_lib.JMTError):
        ops.layernorm_fwd(x, c.ld, None, c.ld, gamma, beta, R.LN_EPS, y, c.ld, mean, rstd, c.rows,
                          c.D)
    dgamma, dbeta = _vec(c.D), _vec(c.D)
    with pytest.raises(_lib.JMTError):
        ops.layernorm_bwd(x, c.ld, None, c.ld, x, c.ld, mean, rstd, gamma, y, c.ld, dgamma, dbeta,
                          0, c.rows, c.D)
    torch.cuda.synchronize()
    assert all(_same(t.base, NAN) for t in (y, mean, rstd, dgamma, dbeta))


# ------------------------------------------------------------------ grouped LayerNorm
def _stack(G, rows, D, dtype, datas=None):
    """(G, rows, D) contiguous operand + one guard row, NaN-filled."""
    flat = _buf(G * rows, D, D, dtype,
                torch.cat(list(datas)) if datas is not None else None)
    t = flat[:G * rows].view(G, rows, D)
    t.guard = flat
    return t


@pytest.mark.parametrize("with_r", [False, True], ids=["nor", "r"])
@pytest.mark.parametrize("c", R.LN_GRP_CASES, ids=_case_id)
def test_layernorm_fwd_grouped(c, with_r):
    rows = R.LN_GRP_ROWS
    os_ = [_ln_ref(rows, c.D, c.dt, c.dt, with_r, f"g{g}") for g in range(c.G)]
    X = _stack(c.G, rows, c.D, c.dt, (o.x for o in os_))
    Rr = _stack(c.G, rows, c.D, c.dt, (o.r for o in os_)) if with_r else None
    Y = _stack(c.G, rows, c.D, c.dt)
    gammas = [_vec(c.D, o.gamma) for o in os_]
    betas = [_vec(c.D, o.beta) for o in os_]
    mean, rstd = _vec(c.G * rows), _vec(c.G * rows)
    assert ops.layernorm_fwd_grouped(X, Rr, gammas, betas, R.LN_EPS, Y, mean, rstd)
    torch.cuda.synchronize()
    for g, o in enumerate(os_):
        R.check(Y[g], o.f.y, o.f.c_y, c.dt, R.K_LN, f"y[{g}]")
        R.check(mean[g * rows:(g + 1) * rows], o.f.mean, o.f.c_mean, FS, R.K_LN, f"mean[{g}]")
        R.check(rstd[g * rows:(g + 1) * rows], o.f.rstd, o.f.c_rstd, FS, R.K_LN, f"rstd[{g}]")
    _untouched(Y.guard, c.G * rows, c.D)
    _vec_untouched(mean)
    _vec_untouched(rstd)


@pytest.mark.parametrize("beta_acc", [0, 1], ids=["set", "acc"])
@pytest.mark.parametrize("with_dsum", [False, True], ids=["nods", "dsum"])
@pytest.mark.parametrize("with_r", [False, True], ids=["nor", "r"])
@pytest.mark.parametrize("c", R.LN_GRP_CASES, ids=_case_id)
def test_layernorm_bwd_grouped(c, with_r, with_dsum, beta_acc):
    rows = R.LN_GRP_ROWS
    os_ = [_ln_ref(rows, c.D, c.dt, c.dt, with_r, f"g{g}") for g in range(c.G)]
    X = _stack(c.G, rows, c.D, c.dt, (o.x for o in os_))
    Rr = _stack(c.G, rows, c.D, c.dt, (o.r for o in os_)) if with_r else None
    dY = _stack(c.G, rows, c.D, c.dt, (o.dy for o in os_))
    dX = _stack(c.G, rows, c.D, c.dt)
    gammas = [_vec(c.D, o.gamma) for o in os_]
    mean = _vec(c.G * rows, torch.cat([o.mean for o in os_]))
    rstd = _vec(c.G * rows, torch.cat([o.rstd for o in os_]))
    outs = [[_acc_out(c.D, beta_acc, 10 * g + k) for g in range(c.G)] for k in range(3)]
    dev = [[v for v, _ in col] for col in outs]
    part = ops.layernorm_bwd_grouped(X, Rr, dY, mean, rstd, gammas, dX, dev[0], dev[1],
                                     dev[2] if with_dsum else None, beta_acc)
    torch.cuda.synchronize()
    assert part is not None
    for g, o in enumerate(os_):
        R.check(dX[g], o.b.dx, o.b.c_dx, c.dt, R.K_LN, f"dx[{g}]")
        _check_acc(*outs[0][g], o.b.dgamma, o.b.c_dgamma, f"dgamma[{g}]")
        _check_acc(*outs[1][g], o.b.dbeta, o.b.c_dbeta, f"dbeta[{g}]")
        if with_dsum:
            _check_acc(*outs[2][g], o.b.dsum, o.b.c_dsum, f"dsum[{g}]")
        else:   # not passed: stays as it was
            v, old = outs[2][g]
            assert _same(v.base, NAN) if old is None else torch.equal(v.cpu().double(), old)
    _untouched(dX.guard, c.G * rows, c.D)


def test_layernorm_grouped_uncovered_width_writes_nothing():
    """D = 256 has no vector kernel: the grouped entry points decline and leave every output."""
    rows, D, G = R.LN_GRP_ROWS, 256, 3
    os_ = [_ln_ref(rows, D, BF, BF, True, f"g{g}") for g in range(G)]
    X = _stack(G, rows, D, BF, (o.x for o in os_))
    Rr = _stack(G, rows, D, BF, (o.r for o in os_))
    Y = _stack(G, rows, D, BF)
    gammas = [_vec(D, o.gamma) for o in os_]
    betas = [_vec(D, o.beta) for o in os_]
    mean, rstd = _vec(G * rows), _vec(G * rows)
    assert ops.layernorm_fwd_grouped(X, Rr, gammas, betas, R.LN_EPS, Y, mean, rstd) is False
    outs = [[_vec(D) for _ in range(G)] for _ in range(3)]
    assert ops.layernorm_bwd_grouped(X, Rr, X, _vec(G * rows, fill=0.0), _vec(G * rows, fill=1.0),
                                     gammas, Y, outs[0], outs[1], outs[2], 0) is None
    torch.cuda.synchronize()
    assert _same(Y.guard.base, NAN) and _same(mean.base, NAN) and _same(rstd.base, NAN)
    assert all(_same(v.base, NAN) for col in outs for v in col)


# ------------------------------------------------------------------ L2 normalize
@pytest.mark.parametrize("c", R.L2_CASES, ids=_case_id)
def test_l2norm_fwd_bwd(c):
    rows = R.L2_ROWS
    x, dy = R.l2_inputs(c.D, c.dt, c.ydt)
    f = R.l2_fwd(_d(x), R.L2_EPS)
    assert float(f.norm[2]) == 0 and 0 < float(f.norm[4]) < R.L2_EPS
    xb = _buf(rows, c.D, c.ld, c.dt, x)
    y = _buf(rows, c.D, c.ld, c.ydt)
    inv = _vec(rows)
    ops.l2norm_fwd(xb, c.ld, rows, c.D, y, c.ld, inv, R.L2_EPS)
    torch.cuda.synchronize()
    R.check(y[:rows, :c.D], f.y, f.c_y, c.ydt, R.K_L2, "y")
    R.check(inv, f.inv, f.c_inv, FS, R.K_L2, "inv_norm")
    _untouched(y, rows, c.D)
    _vec_untouched(inv)
    inv_in = f.inv.float()
    b = R.l2_bwd(_d(x), _d(dy), _d(inv_in), R.L2_EPS)
    dx = _buf(rows, c.D, c.ld, c.ddt)
    ops.l2norm_bwd(xb, c.ld, _buf(rows, c.D, c.ld, c.ydt, dy), c.ld, _vec(rows, inv_in), R.L2_EPS,
                   dx, c.ld, rows, c.D)
    torch.cuda.synchronize()
    R.check(dx[:rows, :c.D], b.dx, b.c_dx, c.ddt, R.K_L2, "dx")
    _untouched(dx, rows, c.D)


# ------------------------------------------------------------------ softmax
def _ldp(n):
    return (n + 7) // 8 * 8 + 8


@pytest.mark.parametrize("n,pdt", R.SM_FWD_CASES, ids=lambda v: DT_NAME.get(v, str(v)))
def test_softmax_fwd(n, pdt):
    rows, lds, ldp = R.SM_ROWS, n + 3, _ldp(n)
    s, _ = R.softmax_inputs(n)
    f = R.softmax_fwd(_d(s), R.SM_SCALE)
    p = _buf(rows, n, ldp, pdt)
    ops.softmax_fwd(_buf(rows, n, lds, FS, s), lds, rows, n, R.SM_SCALE, p, ldp)
    torch.cuda.synchronize()
    R.check(p[:rows, :n], f.p, f.c_p, pdt, R.K_SOFTMAX, "p")
    assert bool((p[:rows, n:] == 0).all()), "padding not zero"
    assert _same(p[rows:], NAN), "guard row written"


@pytest.mark.parametrize("n,pdt,sdt", R.SM_BWD_CASES, ids=lambda v: DT_NAME.get(v, str(v)))
def test_softmax_bwd(n, pdt, sdt):
    rows, lddp, ldp = R.SM_ROWS, n + 3, _ldp(n)
    s, dp = R.softmax_inputs(n)
    p = R.softmax_fwd(_d(s), R.SM_SCALE).p.to(pdt)
    b = R.softmax_bwd(_d(p), _d(dp), R.SM_SCALE)
    ds = _buf(rows, n, ldp, sdt)
    ops.softmax_bwd(_buf(rows, n, ldp, pdt, p), ldp, _buf(rows, n, lddp, FS, dp), lddp, rows, n,
                    R.SM_SCALE, ds, ldp)
    torch.cuda.synchronize()
    R.check(ds[:rows, :n], b.ds, b.c_ds, sdt, R.K_SOFTMAX, "ds")
    assert bool((ds[:rows, n:] == 0).all()), "padding not zero"
    assert _same(ds[rows:], NAN), "guard row written"


# ------------------------------------------------------------------ column sums
@pytest.mark.parametrize("beta_acc", [0, 1], ids=["set", "acc"])
@pytest.mark.parametrize("dt,rows,N,ld", R.CS_CASES, ids=lambda v: DT_NAME.get(v, str(v)))
def test_colsum(dt, rows, N, ld, beta_acc):
    dy, old = R.colsum_inputs(dt, rows, N)
    ref = R.colsum(_d(dy), _d(old) if beta_acc else None)
    db = _vec(N, old) if beta_acc else _vec(N)
    ops.colsum(_buf(rows, N, ld, dt, dy), ld, rows, N, db, beta_acc=bool(beta_acc))
    torch.cuda.synchronize()
    R.check(db, ref.db, ref.c_db, FS, R.K_COLSUM, "db")
    _vec_untouched(db)


@pytest.mark.parametrize("beta_acc", [0, 1], ids=["set", "acc"])
def test_colsum_partials_off_16_bytes(beta_acc):
    """A partials buffer that is not 16-B aligned sends a vector-width N to the scalar reduce."""
    dt, rows, N, ld = BF, 300, 136, 144
    dy, old = R.colsum_inputs(dt, rows, N)
    ref = R.colsum(_d(dy), _d(old) if beta_acc else None)
    db = _vec(N, old) if beta_acc else _vec(N)
    nblk = _lib.load().jmt_colsum_blocks(rows)
    part = _vec(nblk * N, off=1)
    dyb = _buf(rows, N, ld, dt, dy)
    _lib.call("jmt_colsum", ops.dt(dt), rows, N, dyb.data_ptr(), ld, db.data_ptr(), beta_acc,
              part.data_ptr(), ops.stream())
    torch.cuda.synchronize()
    R.check(db, ref.db, ref.c_db, FS, R.K_COLSUM, "db")
    _vec_untouched(db)
    _vec_untouched(part)


@pytest.mark.parametrize("dt", [FS, BF, FH], ids=DT_NAME.get)
def test_colsum_no_rows(dt):
    """rows = 0: beta_acc = 0 zeroes db, beta_acc = 1 leaves it."""
    dy = _buf(0, 16, 16, dt)
    db = _vec(16)
    ops.colsum(dy, 16, 0, 16, db, beta_acc=False)
    torch.cuda.synchronize()
    assert bool((db == 0).all())
    _vec_untouched(db)
    db = _vec(16, fill=3.0)
    ops.colsum(dy, 16, 0, 16, db, beta_acc=True)
    torch.cuda.synchronize()
    assert bool((db.base == 3.0).all())


@pytest.mark.parametrize("beta_acc", [0, 1], ids=["set", "acc"])
@pytest.mark.parametrize("G", [1, 8])
@pytest.mark.parametrize("dt", [FS, BF, FH], ids=DT_NAME.get)
def test_colsum_grouped(dt, G, beta_acc):
    rows, N, ld = 257, 16, 24
    sdy = rows * ld + 40                       # groups further apart than their rows
    flat = torch.full((G * sdy + ld,), NAN, dtype=dt, device=DEV)
    refs, dbs = [], []
    for g in range(G):
        dy, old = R.colsum_inputs(dt, rows, N, f"g{g}")
        flat[g * sdy:g * sdy + rows * ld].view(rows, ld)[:, :N] = dy.to(DEV)
        refs.append(R.colsum(_d(dy), _d(old) if beta_acc else None))
        dbs.append(_vec(N, old) if beta_acc else _vec(N))
    ops.colsum_grouped(flat.data_ptr(), ops.dt(dt), G, ld, sdy, rows, N, dbs,
                       beta_acc=bool(beta_acc), device=flat.device)
    torch.cuda.synchronize()
    for g in range(G):
        R.check(dbs[g], refs[g].db, refs[g].c_db, FS, R.K_COLSUM, f"db[{g}]")
        _vec_untouched(dbs[g])


# ------------------------------------------------------------------ jmt_copy2d (exact)
def _copy_ref(src, dst_old, dd):
    return R.copy2d(_d(src), _d(dst_old)).to(FS).to(dd)


@pytest.mark.parametrize("dd", [FS, BF, FH], ids=DT_NAME.get)
@pytest.mark.parametrize("sd", [FS, BF, FH], ids=DT_NAME.get)
def test_copy2d_rows_vector(sd, dd):
    """copy_rows_vec_kernel: both column strides 1, cols % 8 == 0, padded row strides."""
    g = torch.Generator().manual_seed(21)
    src = torch.randn(3, 16, generator=g).to(sd)
    s, d = _buf(3, 16, 24, sd, src), _buf(3, 16, 32, dd)
    ops.copy2d(s.data_ptr(), ops.dt(sd), d.data_ptr(), ops.dt(dd), 3, 16, 24, 1, 32, 1)
    torch.cuda.synchronize()
    assert torch.equal(d[:3, :16].cpu(), _copy_ref(src, None, dd))
    _untouched(d, 3, 16)


@pytest.mark.parametrize("dd", [FS, BF, FH], ids=DT_NAME.get)
@pytest.mark.parametrize("sd", [FS, BF], ids=DT_NAME.get)
def test_copy2d_generic(sd, dd):
    """copy2d_kernel: a transpose of 37 x 5, a source column stride of 2, and accumulate."""
    g = torch.Generator().manual_seed(22)
    src = torch.randn(37, 10, generator=g).to(sd)
    s = src.to(DEV)
    # transpose of the first 5 columns: dst (5 x 37) element (c, r) = src (r, c)
    d = _buf(5, 37, 40, dd)
    ops.copy2d(s.data_ptr(), ops.dt(sd), d.data_ptr(), ops.dt(dd), 37, 5, 10, 1, 1, 40)
    torch.cuda.synchronize()
    assert torch.equal(d[:5, :37].cpu(), _copy_ref(src[:, :5].t(), None, dd))
    _untouched(d, 5, 37)
    # every second source column into 5 dense ones
    d = _buf(37, 5, 8, dd)
    ops.copy2d(s.data_ptr(), ops.dt(sd), d.data_ptr(), ops.dt(dd), 37, 5, 10, 2, 8, 1)
    torch.cuda.synchronize()
    assert torch.equal(d[:37, :5].cpu(), _copy_ref(src[:, ::2], None, dd))
    _untouched(d, 37, 5)
    # accumulate: dst = round(dst + src), a layout the vector kernel would take without it
    old = torch.randn(3, 8, generator=g).to(dd)
    d = _buf(3, 8, 8, dd, old)
    ops.copy2d(s.data_ptr(), ops.dt(sd), d.data_ptr(), ops.dt(dd), 3, 8, 10, 1, 8, 1,
               accumulate=True)
    torch.cuda.synchronize()
    assert torch.equal(d[:3, :8].cpu(), _copy_ref(src[:3, :8], old, dd))
    _untouched(d, 3, 8)


def test_copy2d_generic_grid_stride_wrap():
    """2049 x 1031 elements exceed the 8192 x 256 threads of copy2d_kernel's capped grid."""
    rows, cols = 2049, 1031
    src = torch.randn(rows, 2 * cols, generator=torch.Generator().manual_seed(23))
    s = src.to(DEV)
    d = _buf(rows, cols, cols, BF)
    ops.copy2d(s.data_ptr(), ops.dt(FS), d.data_ptr(), ops.dt(BF), rows, cols, 2 * cols, 2,
               cols, 1)
    torch.cuda.synchronize()
    assert torch.equal(d[:rows].cpu(), src[:, ::2].to(BF))
    _untouched(d, rows, cols)


def test_copy2d_vector_grid_stride_wrap():
    """4100 x 8192 elements exceed the 16384 x 256 x 8 of copy_rows_vec_kernel's capped grid."""
    rows, cols = 4100, 8192
    src = torch.randn(rows, cols, device=DEV, generator=torch.Generator(DEV).manual_seed(24)
                      ).to(BF)
    d = _buf(rows, cols, cols, BF)
    ops.copy2d(src.data_ptr(), ops.dt(BF), d.data_ptr(), ops.dt(BF), rows, cols, cols, 1, cols, 1)
    torch.cuda.synchronize()
    assert torch.equal(d[:rows], src)
    _untouched(d, rows, cols)
