"""CPU checks of tests/rowops_ref.py: the float64 references agree with float64 autograd, the
comparator accepts honest fp32 evaluations of the same formulas over the whole case table (so
the bound is not too tight) and rejects every listed mutation (so it is tight enough)."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from tests import rowops_ref as R
from tests.rowops_ref import BF, FH, FS, F64

OUT_DTYPES = (FS, BF, FH)
SUMS = (R.sum_sequential, R.sum_pairwise)


def _d(t):
    return None if t is None else t.to(F64)


def _f(t):
    return None if t is None else t.float()


# ------------------------------------------------------------------ references vs autograd
def _close(a, b, tol=1e-12):
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), \
        float((a - b).abs().max())


@pytest.mark.parametrize("with_r", [False, True])
@pytest.mark.parametrize("D", [37, 512])
def test_ln_reference_matches_autograd(D, with_r):
    x, r, gamma, beta, dy = (_d(t) for t in R.ln_inputs(19, D, FS, FS, with_r))
    t = (x + r if with_r else x).clone().requires_grad_(True)
    gm, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = F.layer_norm(t, (D,), gm, bt, R.LN_EPS)
    y.backward(dy)
    f = R.ln_fwd(x, r, gamma, beta, R.LN_EPS)
    b = R.ln_bwd(x, r, dy, f.mean, f.rstd, gamma)
    _close(f.y, y.detach())
    _close(f.mean, t.detach().mean(1))
    _close(f.rstd, 1 / torch.sqrt(t.detach().var(1, unbiased=False) + R.LN_EPS))
    _close(b.dx, t.grad)
    _close(b.dgamma, gm.grad)
    _close(b.dbeta, bt.grad)
    _close(b.dsum, t.grad.sum(0))


@pytest.mark.parametrize("D", [1, 37, 512])
def test_l2_reference_matches_autograd(D):
    x, dy = (_d(t) for t in R.l2_inputs(D, FS, FS))
    xa = x.clone().requires_grad_(True)
    y = F.normalize(xa, p=2.0, dim=1, eps=R.L2_EPS)
    y.backward(dy)
    f = R.l2_fwd(x, R.L2_EPS)
    b = R.l2_bwd(x, dy, f.inv, R.L2_EPS)
    _close(f.y, y.detach())
    # 1e-12 of the largest gradient (1 / eps on the clamped rows)
    _close(b.dx, xa.grad)
    assert float(f.norm[2]) == 0 and 0 < float(f.norm[4]) < R.L2_EPS < float(f.norm[0])


@pytest.mark.parametrize("n", R.SM_N)
def test_softmax_reference_matches_autograd(n):
    s, dp = (_d(t) for t in R.softmax_inputs(n))
    sa = s.clone().requires_grad_(True)
    p = torch.softmax(sa * R.SM_SCALE, 1)
    p.backward(dp)
    f = R.softmax_fwd(s, R.SM_SCALE)
    _close(f.p, p.detach())
    _close(R.softmax_bwd(f.p, dp, R.SM_SCALE).ds, sa.grad)


def test_colsum_and_copy2d_references():
    dy, old = (_d(t) for t in R.colsum_inputs(BF, 300, 65))
    _close(R.colsum(dy).db, dy.sum(0))
    _close(R.colsum(dy, old).db, old + dy.sum(0))
    assert R.colsum(dy[:0]).db.abs().max() == 0
    assert torch.equal(R.copy2d(dy), dy) and torch.equal(R.copy2d(dy, dy), 2 * dy)


def test_summations():
    a = torch.randn(7, 13, generator=torch.Generator().manual_seed(0), dtype=F64)
    for s in SUMS:
        for dim in (0, 1):
            _close(s(a, dim), a.sum(dim))
        assert s(a[:0], 0).shape == (13,) and float(s(a[:0], 0).abs().max()) == 0
    # fp32: the two orders are really different evaluations
    b = torch.randn(3, 1000, generator=torch.Generator().manual_seed(1))
    assert not torch.equal(R.sum_sequential(b, 1), R.sum_pairwise(b, 1))


# ------------------------------------------------------------------ the case table, evaluated
def _ln_value_cases():
    """Distinct operand sets of the LayerNorm tables: (rows, D, dt, gdt, with_r, tag)."""
    seen = []
    for c in R.LN_CASES + R.LN_DSUM_CASES:
        for with_r in (False, True):
            k = (c.rows, c.D, c.dt, c.gdt, with_r, "")
            if k not in seen:
                seen.append(k)
    for c in R.LN_GRP_CASES:
        for g in range(c.G):
            for with_r in (False, True):
                k = (R.LN_GRP_ROWS, c.D, c.dt, c.dt, with_r, f"g{g}")
                if k not in seen:
                    seen.append(k)
    return seen


def _ln_eval(key, sum_, dtype):
    """Forward and backward of one operand set: the float64 reference (sum_exact, F64) or an fp32
    emulation.  The backward reads the reference's mean / rstd rounded to fp32, as a kernel would
    read a stored forward."""
    rows, D, dt, gdt, with_r, tag = key
    x, r, gamma, beta, dy = (None if t is None else t.to(dtype)
                             for t in R.ln_inputs(rows, D, dt, gdt, with_r, tag))
    f = R.ln_fwd(x, r, gamma, beta, R.LN_EPS, sum_)
    f64 = f if dtype == F64 else _ln_eval(key, R.sum_exact, F64)[0]
    b = R.ln_bwd(x, r, dy, f64.mean.float().to(dtype), f64.rstd.float().to(dtype), gamma, sum_)
    return f, b


LN_OUTS = (("y", True), ("mean", False), ("rstd", False))
LN_BOUTS = (("dx", True), ("dgamma", False), ("dbeta", False), ("dsum", False))


def _family_results(family):
    """Yields (got, ref, cond, out_dtype) for every output of every case, emulation and output
    dtype of one family."""
    if family == "ln":
        for key in _ln_value_cases():
            f64, b64 = _ln_eval(key, R.sum_exact, F64)
            for s in SUMS:
                f, b = _ln_eval(key, s, FS)
                for res, ref, outs in ((f, f64, LN_OUTS), (b, b64, LN_BOUTS)):
                    for name, stored in outs:
                        for od in (OUT_DTYPES if stored else (FS,)):
                            yield (getattr(res, name).to(od), getattr(ref, name),
                                   getattr(ref, "c_" + name), od)
    elif family == "l2":
        for D, dt, ydt in sorted({(c.D, c.dt, c.ydt) for c in R.L2_CASES}, key=str):
            x, dy = R.l2_inputs(D, dt, ydt)
            f64 = R.l2_fwd(_d(x), R.L2_EPS)
            inv = f64.inv.float()
            b64 = R.l2_bwd(_d(x), _d(dy), _d(inv), R.L2_EPS)
            for s in SUMS:
                f = R.l2_fwd(_f(x), R.L2_EPS, s)
                b = R.l2_bwd(_f(x), _f(dy), inv, R.L2_EPS, s)
                yield f.inv, f64.inv, f64.c_inv, FS
                for od in OUT_DTYPES:
                    yield f.y.to(od), f64.y, f64.c_y, od
                    yield b.dx.to(od), b64.dx, b64.c_dx, od
    elif family == "softmax":
        for n in R.SM_N:
            s_, dp = R.softmax_inputs(n)
            f64 = R.softmax_fwd(_d(s_), R.SM_SCALE)
            for s in SUMS:
                f = R.softmax_fwd(s_, R.SM_SCALE, s)
                for od in OUT_DTYPES:
                    yield f.p.to(od), f64.p, f64.c_p, od
                for pdt in OUT_DTYPES:
                    p = f64.p.to(pdt)
                    b64 = R.softmax_bwd(_d(p), _d(dp), R.SM_SCALE)
                    b = R.softmax_bwd(_f(p), dp, R.SM_SCALE, s)
                    for od in OUT_DTYPES:
                        yield b.ds.to(od), b64.ds, b64.c_ds, od
    elif family == "colsum":
        for dt, rows, N in sorted({(dt, rows, N) for dt, rows, N, _ in R.CS_CASES}, key=str):
            dy, old = R.colsum_inputs(dt, rows, N)
            for o in (None, old):
                ref = R.colsum(_d(dy), _d(o))
                for s in SUMS:
                    yield R.colsum(_f(dy), o, s).db, ref.db, ref.c_db, FS
    else:
        raise KeyError(family)


FAMILY_K = {"ln": "K_LN", "l2": "K_L2", "softmax": "K_SOFTMAX", "colsum": "K_COLSUM"}


@functools.lru_cache(maxsize=None)
def _measured(family):
    worst, n_fail = 0.0, 0
    K = getattr(R, FAMILY_K[family])
    for got, ref, cond, od in _family_results(family):
        worst = max(worst, R.slack(got, ref, cond, od))
        n_fail += not R.passes(got, ref, cond, od, K)
    return worst, n_fail


@pytest.mark.parametrize("family", sorted(FAMILY_K))
def test_bound_accepts_fp32_emulations(family):
    """Both fp32 emulations pass `check` on every case, in every output dtype."""
    worst, n_fail = _measured(family)
    assert n_fail == 0, (family, worst)


@pytest.mark.parametrize("family", sorted(FAMILY_K))
def test_k_is_4x_measured(family):
    """K is 4 x the largest slack of the emulations, rounded up by a few per cent, no more."""
    worst, _ = _measured(family)
    K = getattr(R, FAMILY_K[family])
    print(f"{family}: measured slack {worst:.4f}, K = {K}")
    assert math.isfinite(worst) and 4 * worst <= K <= 4 * worst * 1.15, (family, worst, K)


# ------------------------------------------------------------------ mutations
def _ln_fwd_mut(x, r, gamma, beta, eps, mut=None):
    """Copy of R.ln_fwd with one defect switched on."""
    D = x.shape[1]
    t = x + r if r is not None and mut != "no_residual" else x
    mean = t.sum(1) / D
    d = t - mean[:, None]
    var = (d * d).sum(1) / (D - 1 if mut == "unbiased" else D)
    rstd = 1.0 / torch.sqrt(var if mut == "no_eps" else var + eps)
    gm = gamma.roll(1) if mut == "gamma_shift" else gamma
    return d * rstd[:, None] * gm + beta, mean, rstd


def _ln_bwd_mut(x, r, dy, mean, rstd, gamma, mut=None):
    """Copy of R.ln_bwd with one defect switched on."""
    D = x.shape[1]
    t = x + r if r is not None and mut != "no_residual" else x
    xhat = (t - mean[:, None]) * rstd[:, None]
    gd = dy * (gamma.roll(1) if mut == "gamma_shift" else gamma)
    s1 = gd.sum(1) / D
    s2 = (gd * xhat).sum(1) / D
    if mut == "no_s1":
        s1 = torch.zeros_like(s1)
    if mut == "no_s2":
        s2 = torch.zeros_like(s2)
    dx = rstd[:, None] * (gd - s1[:, None] - xhat * s2[:, None])
    last = -1 if mut == "drop_last_row" else None
    dgamma = (dy * (t if mut == "dgamma_from_x" else xhat))[:last].sum(0)
    dbeta = dy[:last].sum(0)
    dsum = (dy if mut == "dsum_from_dy" else dx)[:last].sum(0)
    return dx, dgamma, dbeta, dsum


def _ln_mut_cases():
    """A handful of LayerNorm cases, with r, in float64: (case, x, r, gamma, beta, dy, f, b)."""
    for c in (R._ln(19, 512, BF), R._ln(19, 37, FS), R._ln(19, 1024, FH), R._ln(19, 258, BF)):
        x, r, gamma, beta, dy = (_d(t) for t in R.ln_inputs(c.rows, c.D, c.dt, c.gdt, True))
        f = R.ln_fwd(x, r, gamma, beta, R.LN_EPS)
        mean, rstd = _d(f.mean.float()), _d(f.rstd.float())
        yield c, x, r, gamma, beta, dy, f, R.ln_bwd(x, r, dy, mean, rstd, gamma), mean, rstd


def test_mutated_copies_are_faithful():
    for c, x, r, gamma, beta, dy, f, b, mean, rstd in _ln_mut_cases():
        y, m, s = _ln_fwd_mut(x, r, gamma, beta, R.LN_EPS)
        assert torch.equal(y, f.y) and torch.equal(m, f.mean) and torch.equal(s, f.rstd)
        for got, name in zip(_ln_bwd_mut(x, r, dy, mean, rstd, gamma),
                             ("dx", "dgamma", "dbeta", "dsum")):
            assert torch.equal(got, getattr(b, name)), name


def _rejected_ln(mut, outputs):
    """For each named output: is the mutant rejected on at least one case (value rounded to the
    case's stored dtype, as a kernel would leave it)?"""
    hit = {o: False for o in outputs}
    for c, x, r, gamma, beta, dy, f, b, mean, rstd in _ln_mut_cases():
        y, m, s = _ln_fwd_mut(x, r, gamma, beta, R.LN_EPS, mut)
        dx, dgamma, dbeta, dsum = _ln_bwd_mut(x, r, dy, mean, rstd, gamma, mut)
        got = {"y": (y.to(c.ydt), f.y, f.c_y, c.ydt), "mean": (m.float(), f.mean, f.c_mean, FS),
               "rstd": (s.float(), f.rstd, f.c_rstd, FS), "dx": (dx.to(c.ddt), b.dx, b.c_dx, c.ddt),
               "dgamma": (dgamma.float(), b.dgamma, b.c_dgamma, FS),
               "dbeta": (dbeta.float(), b.dbeta, b.c_dbeta, FS),
               "dsum": (dsum.float(), b.dsum, b.c_dsum, FS)}
        for o in outputs:
            hit[o] |= not R.passes(*got[o], R.K_LN)
    return hit


@pytest.mark.parametrize("mut,outputs", [
    ("unbiased", ("y", "rstd")),                       # 1
    ("no_eps", ("y", "rstd")),                         # 2
    ("no_residual", ("y", "mean", "rstd", "dx", "dgamma")),   # 3
    ("gamma_shift", ("y", "dx")),                      # 4
    ("no_s1", ("dx",)),                                # 5
    ("no_s2", ("dx",)),                                # 6
    ("dgamma_from_x", ("dgamma",)),                    # 7
    ("drop_last_row", ("dgamma", "dbeta", "dsum")),    # 8
    ("dsum_from_dy", ("dsum",)),                       # 10
])
def test_layernorm_mutations_rejected(mut, outputs):
    hit = _rejected_ln(mut, outputs)
    assert all(hit.values()), (mut, hit)


def test_no_eps_is_seen_on_the_low_variance_and_constant_rows():
    """Mutation 2 is observable only because the table holds such rows: on them alone."""
    for c, x, r, gamma, beta, dy, f, b, mean, rstd in _ln_mut_cases():
        y, _, s = _ln_fwd_mut(x, r, gamma, beta, R.LN_EPS, "no_eps")
        for row in (3, 5):
            assert not R.passes(s[row:row + 1].float(), f.rstd[row:row + 1],
                                f.c_rstd[row:row + 1], FS, R.K_LN), (c, row)
        assert not R.passes(y[3:4].to(c.ydt), f.y[3:4], f.c_y[3:4], c.ydt, R.K_LN), c


def test_colsum_mutations_rejected():
    hit8 = hit9a = hit9b = False
    for dt, rows, N in ((BF, 300, 65), (FS, 257, 4), (FH, 256, 136), (BF, 1, 3)):
        dy, old = (_d(t) for t in R.colsum_inputs(dt, rows, N))
        plain, accd = R.colsum(dy), R.colsum(dy, old)
        hit8 |= not R.passes(dy[:-1].sum(0).float(), plain.db, plain.c_db, FS, R.K_COLSUM)   # 8
        hit9a |= not R.passes(plain.db.float(), accd.db, accd.c_db, FS, R.K_COLSUM)          # 9
        hit9b |= not R.passes(accd.db.float(), plain.db, plain.c_db, FS, R.K_COLSUM)         # 9
    assert hit8 and hit9a and hit9b


def test_layernorm_beta_acc_mutation_rejected():
    """9, LayerNorm family: dgamma / dbeta with the old contents dropped, or added unasked."""
    for c, x, r, gamma, beta, dy, f, b, mean, rstd in _ln_mut_cases():
        old = torch.randn(c.D, generator=torch.Generator().manual_seed(3), dtype=F64)
        for name in ("dgamma", "dbeta", "dsum"):
            v, cv = getattr(b, name), getattr(b, "c_" + name)
            av, ac = R.acc(old, v, cv)
            assert not R.passes(v.float(), av, ac, FS, R.K_LN), (c, name)
            assert not R.passes(av.float(), v, cv, FS, R.K_LN), (c, name)
            assert R.passes(av.float(), av, ac, FS, R.K_LN), (c, name)


@pytest.mark.parametrize("od", OUT_DTYPES)
def test_unwritten_last_column_and_dirty_padding_rejected(od):
    """11 and 17: an element left at its NaN prefill, and the smallest non-zero padding value."""
    x, dy = (_d(t) for t in R.l2_inputs(37, FS, FS))
    f = R.l2_fwd(x, R.L2_EPS)
    got = f.y.to(od)
    assert R.passes(got, f.y, f.c_y, od, R.K_L2)
    got[-1, -1] = math.nan
    assert not R.passes(got, f.y, f.c_y, od, R.K_L2)
    s, _ = R.softmax_inputs(65)
    p = R.softmax_fwd(_d(s), R.SM_SCALE)
    got = p.p.to(od)
    got[0, -1] = math.nan
    assert not R.passes(got, p.p, p.c_p, od, R.K_SOFTMAX)
    x, r, gamma, beta, dy = (_d(t) for t in R.ln_inputs(19, 37, FS, FS, True))
    fl = R.ln_fwd(x, r, gamma, beta, R.LN_EPS)
    got = fl.y.to(od)
    got[7, -1] = math.nan
    assert not R.passes(got, fl.y, fl.c_y, od, R.K_LN)
    pad = torch.zeros(5, 3, dtype=od)
    z = torch.zeros(5, 3, dtype=F64)
    assert R.passes(pad, z, z, od, R.K_SOFTMAX)
    pad[2, 1] = torch.finfo(od).smallest_normal if od == FS else \
        torch.tensor(1, dtype=torch.int16).view(od)
    assert float(pad[2, 1]) > 0 and not R.passes(pad, z, z, od, R.K_SOFTMAX)


@pytest.mark.parametrize("D", [1, 37, 512])
def test_l2_mutations_rejected(D):
    x, dy = (_d(t) for t in R.l2_inputs(D, FS, FS))
    f = R.l2_fwd(x, R.L2_EPS)
    b = R.l2_bwd(x, dy, f.inv, R.L2_EPS)
    y = x * f.inv[:, None]
    proj = (dy - y * (y * dy).sum(1)[:, None]) * f.inv[:, None]         # 12: projection everywhere
    assert R.passes(b.dx.float(), b.dx, b.c_dx, FS, R.K_L2)
    # row 4 is clamped with x != 0 (at D = 1 its projection is 0, its true gradient dy / eps)
    assert not R.passes(proj[4:5].float(), b.dx[4:5], b.c_dx[4:5], FS, R.K_L2)
    inv = 1.0 / f.norm                                                  # 13: eps ignored
    assert not R.passes(inv[4:5].float(), f.inv[4:5], f.c_inv[4:5], FS, R.K_L2)
    assert not R.passes((x * inv[:, None])[4:5].float(), f.y[4:5], f.c_y[4:5], FS, R.K_L2)
    assert not R.passes((x * inv[:, None])[2:3].float(), f.y[2:3], f.c_y[2:3], FS, R.K_L2)


@pytest.mark.parametrize("n", R.SM_N)
def test_softmax_mutations_rejected(n):
    s, dp = (_d(t) for t in R.softmax_inputs(n))
    f = R.softmax_fwd(s, R.SM_SCALE)
    b = R.softmax_bwd(f.p, dp, R.SM_SCALE)
    for od in OUT_DTYPES:
        got = (torch.softmax(s, 1) * R.SM_SCALE).to(od)                 # 14
        assert not R.passes(got, f.p, f.c_p, od, R.K_SOFTMAX)
        if n > 1:   # at one column dS is 0 whatever the scale
            got = (f.p * (dp - (f.p * dp).sum(1)[:, None])).to(od)      # 15
            assert not R.passes(got, b.ds, b.c_ds, od, R.K_SOFTMAX)
            got = (R.SM_SCALE * f.p * (dp - (f.p * dp)[:, :-1].sum(1)[:, None])).to(od)   # 16
            assert not R.passes(got, b.ds, b.c_ds, od, R.K_SOFTMAX)


def test_softmax_bwd_short_dot_rejected_at_one_column():
    """16 at n = 1: the true dS is 0 (p = 1, dot = dp) and a dot over no column leaves scale dp."""
    s, dp = (_d(t) for t in R.softmax_inputs(1))
    f = R.softmax_fwd(s, R.SM_SCALE)
    b = R.softmax_bwd(f.p, dp, R.SM_SCALE)
    # cond = 2 scale |dp|, so the mutant's error scale |dp| is 2^23 / K bounds away
    assert not R.passes((R.SM_SCALE * f.p * dp).float(), b.ds, b.c_ds, FS, R.K_SOFTMAX)


@pytest.mark.parametrize("dd", OUT_DTYPES)
def test_copy2d_accumulate_mutation_rejected(dd):
    g = torch.Generator().manual_seed(5)
    src, dst = torch.randn(3, 16, generator=g), torch.randn(3, 16, generator=g).to(dd)
    ref = R.copy2d(_d(src), _d(dst)).to(FS).to(dd)
    assert torch.equal(ref, (dst.float() + src).to(dd))      # fp32 add, one rounding
    assert not torch.equal(R.copy2d(_d(src)).to(FS).to(dd), ref)        # 18
