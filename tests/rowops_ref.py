"""References, comparator and case table for the row-op kernels (csrc/rowops.hip).

Not a test: tests/test_rowops_ref.py validates what is here on the CPU, tests/test_gpu_rowops.py
runs the kernels against it.

Every reference is written out term by term and is generic over the tensor dtype and over the
summation (`sum_`): in float64 with torch's own sum it is the reference, in float32 with
`sum_sequential` / `sum_pairwise` it is an emulation of an honest fp32 kernel, which is how the
constants K below were measured.  Inputs are the already-rounded operands exactly as the kernel
reads them (16-bit tensors upcast, `eps` / `scale` rounded to fp32 by `f32`), 2-D, without padding.

Each reference returns the value and, beside it (`c_<name>`), the magnitude `cond` of what an fp32
evaluation cancels or sums; `check` compares elementwise against
    u(out_dtype) * max(|ref|, tiny(out_dtype)) + K * 2^-24 * cond
(no max-over-tensor tolerance).  max(., tiny) is the rounding of the stored type below its
smallest normal number, where the error of one rounding is half the subnormal spacing,
u * tiny, and no longer u * |ref| (fp16 softmax probabilities get there).
"""
import math
from collections import namedtuple
from types import SimpleNamespace as NS

import torch

F64 = torch.float64
E24 = 2.0 ** -24
U = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
TINY = {torch.float32: 2.0 ** -126, torch.bfloat16: 2.0 ** -126, torch.float16: 2.0 ** -14}

# One constant per family: 4 x the largest slack (|emu - ref| - u |ref|) / (2^-24 cond) that the
# two fp32 emulations (left-to-right and pairwise sums) show against the float64 reference over
# the whole case table below, every output dtype (tests/test_rowops_ref.py::test_k_is_4x_measured
# recomputes it; the wave reduction of the kernels associates differently from either).  Never
# taken from the HIP kernels.
K_LN = 195.0      # measured 47.69 (y at D = 2047, left-to-right sums)
K_L2 = 155.0      # measured 37.54 (y at D = 2048, left-to-right sums)
K_SOFTMAX = 380.0  # measured 88.28 (p at scaled logits of +-74: fp32 rounds s * scale); rounded
#                    up by 7 %, as the emulation's exp may differ by an ulp between CPUs
K_COLSUM = 36.0    # measured 8.84 (300 rows, left-to-right sums)


def f32(v: float) -> float:
    """The value a C `float` argument takes."""
    return float(torch.tensor(v, dtype=torch.float32))


# ------------------------------------------------------------------------------- summation
def sum_exact(a, dim):
    return a.sum(dim)


def sum_sequential(a, dim):
    a = a.movedim(dim, 0).contiguous()
    s = torch.zeros_like(a.sum(0))
    for i in range(a.shape[0]):
        s = s + a[i]
    return s


def sum_pairwise(a, dim):
    a = a.movedim(dim, -1)
    n = a.shape[-1]
    if n == 0:
        return a.sum(-1)
    p = 1 << (n - 1).bit_length()
    if p != n:
        a = torch.cat([a, a.new_zeros(*a.shape[:-1], p - n)], -1)
    while a.shape[-1] > 1:
        a = a[..., 0::2] + a[..., 1::2]
    return a[..., 0]


# ------------------------------------------------------------------------------- references
def ln_fwd(x, r, gamma, beta, eps, sum_=sum_exact):
    D = x.shape[1]
    t = x + r if r is not None else x
    mean = sum_(t, 1) / D
    d = t - mean[:, None]
    var = sum_(d * d, 1) / D
    rstd = 1.0 / torch.sqrt(var + eps)
    y = d * rstd[:, None] * gamma + beta
    am = mean.abs()[:, None]
    c_y = (t.abs() + am) * rstd[:, None] * gamma.abs() + beta.abs()
    c_mean = sum_(t.abs(), 1) / D
    # d(rstd) = rstd^3/2 d(var); each d carries (|t| + |mean|) 2^-24, so d(var) <= mean_c
    # 2 |d| (|t| + |mean|) 2^-24, plus the roundings of the sum, sqrt and division (relative)
    c_rstd = rstd * (1.0 + rstd * rstd * sum_(d.abs() * (t.abs() + am), 1) / D)
    return NS(y=y, mean=mean, rstd=rstd, c_y=c_y, c_mean=c_mean, c_rstd=c_rstd)


def ln_bwd(x, r, dy, mean, rstd, gamma, sum_=sum_exact):
    D = x.shape[1]
    t = x + r if r is not None else x
    xhat = (t - mean[:, None]) * rstd[:, None]
    gd = dy * gamma
    s1 = sum_(gd, 1) / D
    s2 = sum_(gd * xhat, 1) / D
    dx = rstd[:, None] * (gd - s1[:, None] - xhat * s2[:, None])
    c_dx = rstd[:, None] * (gd.abs() + (sum_(gd.abs(), 1) / D)[:, None]
                            + xhat.abs() * (sum_((gd * xhat).abs(), 1) / D)[:, None])
    dgamma = sum_(dy * xhat, 0)
    dbeta = sum_(dy, 0)
    dsum = sum_(dx, 0)
    # dgamma and dsum sum values that the kernel computed itself: their summands carry the
    # cancellation of xhat = (t - mean) rstd and of dx, so cond sums the summands' own cond
    # (>= their magnitude).  With sum |dy xhat| and sum |dx| alone a single row, where the sum
    # is the summand, already needs K = 134 and 1900 in honest fp32.
    c_xhat = (t.abs() + mean.abs()[:, None]) * rstd[:, None]
    return NS(dx=dx, dgamma=dgamma, dbeta=dbeta, dsum=dsum, c_dx=c_dx,
              c_dgamma=sum_(dy.abs() * c_xhat, 0), c_dbeta=sum_(dy.abs(), 0),
              c_dsum=sum_(c_dx, 0))


def l2_fwd(x, eps, sum_=sum_exact):
    norm = torch.sqrt(sum_(x * x, 1))
    inv = 1.0 / torch.clamp(norm, min=eps)
    y = x * inv[:, None]
    return NS(y=y, inv=inv, norm=norm, c_y=y.abs(), c_inv=inv)


def l2_bwd(x, dy, inv, eps, sum_=sum_exact):
    """`inv` as the forward stored it; the clamp is decided from x: not clamped iff ||x|| > eps."""
    live = torch.sqrt(sum_(x * x, 1)) > eps
    y = x * inv[:, None]
    dot = sum_(y * dy, 1)
    proj = (dy - y * dot[:, None]) * inv[:, None]
    dx = torch.where(live[:, None], proj, dy * inv[:, None])
    c_dx = inv[:, None] * (dy.abs() + y.abs() * sum_((y * dy).abs(), 1)[:, None])
    return NS(dx=dx, c_dx=c_dx)


def softmax_fwd(s, scale, sum_=sum_exact):
    a = s * scale
    e = torch.exp(a - a.max(1, keepdim=True).values)
    p = e / sum_(e, 1)[:, None]
    return NS(p=p, c_p=p.abs())


def softmax_bwd(p, dp, scale, sum_=sum_exact):
    dot = sum_(p * dp, 1)
    ds = scale * p * (dp - dot[:, None])
    c_ds = scale * p * (dp.abs() + sum_(p * dp.abs(), 1)[:, None])
    return NS(ds=ds, c_ds=c_ds)


def colsum(dy, old=None, sum_=sum_exact):
    """Column sums of dy (rows x N), added onto `old` when given (beta_acc = 1)."""
    s, c = sum_(dy, 0), sum_(dy.abs(), 0)
    if old is not None:
        s, c = old + s, old.abs() + c
    return NS(db=s, c_db=c)


def acc(old, val, cond):
    """beta_acc = 1 onto `old` for any column-type result: value and cond."""
    return old + val, old.abs() + cond


def copy2d(src, dst=None):
    """dst = src, or dst + src with accumulate; the kernel works in fp32 and rounds once to the
    destination type: compare with copy2d(...).to(torch.float32).to(dst_dtype), exactly."""
    return src if dst is None else dst + src


# ------------------------------------------------------------------------------- comparator
def bound(ref, cond, out_dtype, K):
    ref, cond = ref.to(F64), cond.to(F64)
    return U[out_dtype] * ref.abs().clamp(min=TINY[out_dtype]) + K * E24 * cond


def slack(got, ref, cond, out_dtype):
    """Largest (|got - ref| - u max(|ref|, tiny)) / (2^-24 cond); elements with cond == 0 must be
    within the rounding term alone and count as 0 (inf when they are not)."""
    got, ref, cond = got.to(F64), ref.to(F64), cond.to(F64)
    if got.numel() == 0:
        return 0.0
    over = (got - ref).abs() - U[out_dtype] * ref.abs().clamp(min=TINY[out_dtype])
    over = torch.where(torch.isnan(over), torch.full_like(over, math.inf), over)
    q = torch.where(over <= 0, torch.zeros_like(over), over / (E24 * cond))
    return float(q.max())


def check(got, ref, cond, out_dtype, K, what=""):
    """Fails unless |got - ref| <= u |ref| + K 2^-24 cond for every element (NaN fails)."""
    assert got.shape == ref.shape == cond.shape, (what, got.shape, ref.shape, cond.shape)
    if got.numel() == 0:
        return
    g, r = got.detach().cpu().to(F64), ref.to(F64)
    b = bound(r, cond, out_dtype, K)
    err = (g - r).abs()
    bad = ~(err <= b)
    if bad.any():
        i = int(torch.where(bad.flatten(), (err / b.clamp(min=1e-300)).flatten().nan_to_num(
            nan=math.inf), torch.zeros(())).argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), g.shape))
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {g.numel()} elements out of bound; worst at {idx}: got "
            f"{float(g.flatten()[i])!r} ref {float(r.flatten()[i])!r} bound "
            f"{float(b.flatten()[i]):.3e} cond {float(cond.to(F64).flatten()[i]):.3e}")


def passes(got, ref, cond, out_dtype, K):
    try:
        check(got, ref, cond, out_dtype, K)
    except AssertionError:
        return False
    return True


# ------------------------------------------------------------------------------- case table
BF, FH, FS = torch.bfloat16, torch.float16, torch.float32
DT_NAME = {BF: "bf16", FH: "fp16", FS: "fp32"}
LN_EPS = f32(1e-5)
L2_EPS = f32(1e-3)
SM_SCALE = f32(0.37)


def _gen(*key):
    """A generator seeded from the case's parameters (stable across processes, unlike hash())."""
    text = "|".join(str(k) for k in key)
    return torch.Generator().manual_seed(
        sum((i + 1) * 7919 * (ord(ch) + 13) for i, ch in enumerate(text)) % (2 ** 31))


# LayerNorm.  dt: x / r; ydt: forward output; gdt: dy; ddt: dx.  ld: row stride of every 2-D
# operand; force: how a vector D is pushed onto the generic kernels ("xoff": x one element off
# its alignment, "goff": gamma one float off).
LnCase = namedtuple("LnCase", "rows D dt ydt gdt ddt ld force")


def _ln(rows, D, dt, ld=None, force="", ydt=None, gdt=None, ddt=None):
    return LnCase(rows, D, dt, ydt or dt, gdt or dt, ddt or dt, ld or D, force)


LN_CASES = (
    # vector kernels NV = 2 / 3 / 4: one row; one 16-row block + a 3-row tail
    [_ln(rows, D, dt) for D in (512, 768, 1024) for dt in (FS, BF, FH) for rows in (1, 19)]
    # D = 512 16-bit: ld 512 is the C8 backward (above), ld 516 its 8-byte form
    + [_ln(rows, 512, dt, ld=516) for dt in (BF, FH) for rows in (1, 19)]
    # generic kernels: ragged ends, v[32] at its limit, slab reduce straddling split (258) and
    # its scalar form (37)
    + [_ln(19, D, dt) for D in (37, 256, 258, 300, 2047, 2048) for dt in (FS, BF)]
    + [_ln(19, 512, BF, force="xoff"), _ln(19, 512, BF, force="goff"), _ln(19, 512, BF, ld=513),
       _ln(19, 512, FS, ld=513)]
    # mixed dtypes
    + [_ln(19, 512, BF, ydt=FS, gdt=FS, ddt=BF), _ln(19, 512, FS, ydt=FS, gdt=BF, ddt=FS)]
    # 323 blocks: the 4x-unrolled slab loop, its remainder loop and a ragged last block
    + [_ln(5157, 512, BF)]
)
# jmt_layernorm_bwd_dsum (backward only)
LN_DSUM_CASES = ([_ln(19, D, BF, ld=ld) for D in (512, 768, 1024) for ld in (D, D + 4)]
                 + [_ln(19, D, FS) for D in (512, 768, 1024)])
# grouped: rows = 37 = 32 + 5, so the wave whose first row is 36 has its paired row 40 past the end
LnGrpCase = namedtuple("LnGrpCase", "G D dt")
LN_GRP_CASES = [LnGrpCase(G, D, dt) for G in (1, 3, 8) for D in (512, 768, 1024)
                for dt in (BF, FH, FS)]
LN_GRP_ROWS = 37


def ln_inputs(rows, D, dt, gdt, with_r, tag=""):
    """x, r (or None), gamma, beta, dy as the kernel reads them (stored dtypes).  Non-zero mean,
    gamma != 1, beta != 0; from 19 rows on, row 3 has a variance comparable to eps (2^-9 randn,
    exact in bf16 / fp16) and row 5 is constant."""
    g = _gen("ln", rows, D, DT_NAME[dt], with_r, tag)
    x = 3 * torch.randn(rows, D, generator=g) + 1
    r = torch.randn(rows, D, generator=g) if with_r else None
    if rows >= 19:
        x[3] = 2.0 ** -9 * torch.randn(D, generator=g).to(BF).float()
        x[5] = 1.5
        if with_r:
            r[3] = 2.0 ** -9 * torch.randn(D, generator=g).to(BF).float()
            r[5] = 0.25
    gamma = 1 + 0.5 * torch.randn(D, generator=g)
    beta = 0.5 * torch.randn(D, generator=g)
    dy = torch.randn(rows, D, generator=g)
    return (x.to(dt), r.to(dt) if with_r else None, gamma, beta, dy.to(gdt))


# L2 normalize.  dt: x; ydt: y and dy; ddt: dx.  rows = 7: row 2 zero, row 4 with 0 < ||x|| < eps.
L2Case = namedtuple("L2Case", "D dt ydt ddt ld")
L2_ROWS = 7
L2_CASES = (
    [L2Case(D, dt, dt, dt, D) for D in (512, 1024, 2048) for dt in (FS, BF, FH)]
    + [L2Case(D, FS, ydt, FS, D) for D in (512, 1024, 2048) for ydt in (BF, FH)]   # L2NormFn's mix
    + [L2Case(D, dt, dt, dt, D) for D in (1, 37, 768) for dt in (FS, BF, FH)]
    + [L2Case(512, dt, dt, dt, 513) for dt in (FS, BF)]
)


def l2_inputs(D, dt, ydt):
    g = _gen("l2", D, DT_NAME[dt], DT_NAME[ydt])
    x = torch.randn(L2_ROWS, D, generator=g) + 0.25
    x[2] = 0
    x[4] = x[4] * (0.3 * L2_EPS / float(x[4].double().norm()))
    dy = torch.randn(L2_ROWS, D, generator=g)
    return x.to(dt), dy.to(ydt)


# softmax: rows = 5, lds = n + 3, ldp = roundup(n, 8) + 8
SM_ROWS = 5
SM_N = (1, 63, 64, 65, 300)
SM_FWD_CASES = [(n, pdt) for n in SM_N for pdt in (FS, BF, FH)]
SM_BWD_CASES = [(n, pdt, sdt) for n in SM_N for pdt, sdt in ((BF, BF), (FH, FH), (FS, FS), (BF, FS))]


def softmax_inputs(n):
    """Logits (fp32) and dp (fp32).  Row 0 reaches +200 and row 1 -200, each spread over 100
    (37 after the scale), so that the max subtraction matters and no probability underflows fp32;
    row 3 is constant."""
    g = _gen("sm", n)
    s = torch.randn(SM_ROWS, n, generator=g) * 4
    s[0] = 100 + 100 * torch.rand(n, generator=g)
    s[1] = -100 - 100 * torch.rand(n, generator=g)
    s[0, 0], s[1, 0] = 200.0, -200.0
    s[3] = 7.25
    dp = torch.randn(SM_ROWS, n, generator=g)
    return s, dp


# column sums: (N, ld) per kernel; the vector form needs N and ld multiples of 16 B
CS_ROWS_LIST = (1, 255, 256, 257, 300)


def colsum_shapes(dt):
    v = 4 if dt == FS else 8
    return [(v, v), (136, 144), (1, 1), (3, 5), (64, 65), (65, 67), (300, 301)]


CS_CASES = [(dt, rows, N, ld) for dt in (FS, BF, FH) for rows in CS_ROWS_LIST
            for N, ld in colsum_shapes(dt)]


def colsum_inputs(dt, rows, N, tag=""):
    g = _gen("cs", DT_NAME[dt], rows, N, tag)
    dy = (torch.randn(rows, N, generator=g) + 0.5).to(dt)
    old = torch.randn(N, generator=g)
    return dy, old
