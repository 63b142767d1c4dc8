"""References, comparator and case table for the loss kernels (csrc/ccc.hip).

Not a test: tests/test_loss_ref.py validates what is here on the CPU, tests/test_gpu_losses.py
runs the kernels against it.

Every reference is written out term by term and is generic over the dtype in which a prediction
value / a row's log-sum-exp is evaluated (`dt`) and over the summation (`sum_`): in float64 with
torch's own sum it is the reference; with `dt` = float32 and `sum_sequential` / `sum_pairwise` it
emulates an honest kernel of the same mix as csrc/ccc.hip (per-element softmax work in fp32, the
long sums and the loss algebra in double), which is how the constants K below were measured.
Inputs are the operands exactly as the kernel reads them: 16-bit tensors upcast, `lo` / `hi` /
`eps` / `ignore` rounded to fp32 by `f32`.

Each reference returns the value and beside it the magnitude `cond` of what the evaluation
cancels or sums; `check` compares elementwise, every element, against
    u(out_dtype) * max(|ref|, tiny) + K * unit * cond
u(float64) = 2^-53, u(float32) = 2^-24 (the kernels compute in double and round once to the
stored type); a 16-bit output is rounded twice (double -> float -> 16 bit), so its u is the
half-ulp of the type plus 2^-24.  `unit` is 2^-53 for the float64 outputs (statistics, coef) and
the CCC gradient at k = 1, where the predictions are exact inputs and only the order of the
double sums differs, and 2^-24 at k > 1, where `pred_value` is an fp32 softmax expectation; the
loss scalars (evaluated in fp32 op order) and everything of CELoss use 2^-24.

exp / log model.  The kernels use __expf / __logf: exp(x) is exp2 of the fp32-rounded
x * log2(e), log(x) is log2(x) * ln(2) rounded.  The fp32 emulation evaluates them that way
(`_exp`, `_log`), so the |z - max| 2^-24 error of the exponent's argument is inside the
measurement of K.
"""
import math
from collections import namedtuple
from types import SimpleNamespace as NS

import numpy as np
import torch

from oracle import jmt_ref as O
from tests.rowops_ref import BF, DT_NAME, F64, FH, FS, _gen, f32, sum_exact, sum_pairwise

E24 = 2.0 ** -24
E53 = 2.0 ** -53
U = {F64: E53, FS: E24, BF: 2.0 ** -8 + E24, FH: 2.0 ** -11 + E24}
TINY = {F64: 2.0 ** -1022, FS: 2.0 ** -126, BF: 2.0 ** -126, FH: 2.0 ** -14}

TAIL = 24 * 1024      # ccc_stats_kernel: RC * CT elements are register-cached, the rest re-read
BLOCK = 1024          # mask_indices_kernel: elements per trip of its outer loop
MAXK = 64
IGNORE = f32(-5.0)
EPS = f32(1e-8)

# One constant per family: 4 x the largest slack (|emu - ref| - u |ref|) / (unit cond) that the
# two emulations (left-to-right and pairwise sums) show against the float64 reference over the
# whole case table below (tests/test_loss_ref.py::test_k_is_4x_measured recomputes it; the
# kernels' wave reduction associates differently from either).  Never taken from the HIP kernels.
# The constants are rounded up by about 5 %, as the emulation's exp2 / log2 may differ by an ulp
# between CPUs.  coef counts with the statistics (float64 outputs whose error is the sums').
K_STATS = 215.0     # measured 51.34 (n = 262444, kind 1, left-to-right double sums, in 2^-53)
K_CCC_LOSS = 2.45   # measured 0.581 (the fp32 op order against the float64 formula)
K_CCC_GRAD = 8.0    # measured 1.913 (dL/dz at k > 1; at k = 1 the one rounding covers it)
K_CE_LOSS = 0.12    # measured 0.0283 (cond sums every row's magnitudes, their errors average out)
K_CE_GRAD = 11.2    # measured 2.655

FLUSH = 2.0 ** -126 / E24
LOG2E32 = f32(math.log2(math.e))
LN2_32 = f32(math.log(2.0))


def unit(k):
    return E53 if k == 1 else E24


# ------------------------------------------------------------------------------- summation
def sum_sequential(a, dim):
    """Left to right in a's own dtype (numpy's accumulate adds one element at a time)."""
    if a.shape[dim] == 0:
        return a.sum(dim)
    return torch.from_numpy(np.asarray(np.take(np.add.accumulate(a.numpy(), axis=dim), -1,
                                               axis=dim)))


def _exp(a):
    if a.dtype == F64:
        return torch.exp(a)
    return torch.exp2(a * LOG2E32)


def _log(a):
    if a.dtype == F64:
        return torch.log(a)
    return torch.log2(a) * LN2_32


# ------------------------------------------------------------------------------- CCC
def bins(k, lo, hi):
    """bin_value: numpy.linspace(lo, hi, k) in float64, cast to fp32."""
    return torch.from_numpy(np.linspace(lo, hi, k).astype(np.float32))


def pred_value(z, k, lo, hi, sum_=sum_exact):
    """x: the prediction itself (k = 1, z of shape (n,)) or sum_c softmax(z)_c bins_c (z (n, k)),
    in z's dtype.  c_x: what one fp32 evaluation may lose of x, in 2^-24 (|x| at k = 1).  p, rel:
    the softmax and the relative error, in 2^-24, of one of its fp32 entries."""
    if k == 1:
        return NS(x=z, c_x=z.abs(), p=None, rel=None, b=None)
    b = bins(k, lo, hi).to(z.dtype)
    d = z - z.max(1, keepdim=True).values
    e = _exp(d)
    s = sum_(e, 1)
    x = sum_(e * b, 1) / s
    p = e / s[:, None]
    rel = 2.0 + d.abs() + sum_(p * (1.0 + d.abs()), 1)[:, None]
    c_x = sum_(p * rel * b.abs(), 1) + x.abs()
    return NS(x=x, c_x=c_x, p=p, rel=rel, b=b)


def ccc_stats(kind, pred, label, k, ignore, lo, hi, sum_=sum_exact, dt=F64, mut=None):
    """The eight doubles of one rank, s = (valid count, mean x, mean y, Sxx, Syy, Sxy, pre-mask
    n, 0), their cond c, and the compacted x, y with their own cond (cx, cy) and positions idx.
    Ignored elements are compacted away before anything is computed from them.  With no valid
    element the means are 0, as the kernel documents."""
    n = label.numel()
    pos = torch.arange(n)
    keep = torch.ones(n, dtype=torch.bool) if kind == 0 else label != ignore
    if mut == "tail_unmasked":
        keep = keep | (pos >= TAIL)
    if mut == "tail_dropped":
        keep = keep & (pos < TAIL)
    idx = torch.nonzero(keep).flatten()
    pv = pred_value(pred[idx].to(dt), k, lo, hi, sum_)
    x, cx = pv.x.to(F64), pv.c_x.to(F64)
    y = label[idx].to(F64)
    cy = y.abs()
    c = idx.numel()
    s, cs = torch.zeros(8, dtype=F64), torch.zeros(8, dtype=F64)
    s[0], s[6] = c, n
    if c > 0:
        mx, my = sum_(x, 0) / c, sum_(y, 0) / c
        cmx, cmy = sum_(cx, 0) / c, sum_(cy, 0) / c
        dx, dy = x - mx, y - my
        if mut == "tail_uncentred":      # raw moments beyond the register-cached part
            t = idx >= TAIL
            h = ~t
            nt = float(t.sum())
            sxt, syt = sum_(x[t], 0), sum_(y[t], 0)
            xx = sum_((dx * dx)[h], 0) + (sum_((x * x)[t], 0) - 2 * mx * sxt + nt * mx * mx)
            yy = sum_((dy * dy)[h], 0) + (sum_((y * y)[t], 0) - 2 * my * syt + nt * my * my)
            xy = sum_((dx * dy)[h], 0) + (sum_((x * y)[t], 0) - mx * syt - my * sxt + nt * mx * my)
        else:
            xx, yy, xy = sum_(dx * dx, 0), sum_(dy * dy, 0), sum_(dx * dy, 0)
        s[1], s[2], s[3], s[4], s[5] = mx, my, xx, yy, xy
        ex, ey = cx + cmx, cy + cmy
        cs[1], cs[2] = cmx, cmy
        cs[3] = sum_(2 * dx.abs() * ex + dx * dx, 0)
        cs[4] = sum_(2 * dy.abs() * ey + dy * dy, 0)
        cs[5] = sum_(dx.abs() * ey + dy.abs() * ex + (dx * dy).abs(), 0)
    return NS(s=s, c=cs, x=x, y=y, cx=cx, cy=cy, idx=idx, pv=pv, n=n)


def ccc_stats_cat(kind, preds, labels, k, ignore, lo, hi, **kw):
    """The statistics of the ranks' concatenated batch, computed from the data."""
    return ccc_stats(kind, torch.cat(list(preds)), torch.cat(list(labels)), k, ignore, lo, hi, **kw)


def ccc_combine(stats_all):
    """Whole-batch statistics from the ranks' eight doubles, directly (weighted mean, then every
    rank's centred sums shifted to it): not Chan's running update."""
    S = torch.stack([torch.as_tensor(s, dtype=F64) for s in stats_all])
    nr = S[:, 0]
    out = torch.zeros(8, dtype=F64)
    out[0], out[6] = nr.sum(), S[:, 6].sum()
    if float(out[0]) > 0:
        mx, my = (nr * S[:, 1]).sum() / out[0], (nr * S[:, 2]).sum() / out[0]
        ex, ey = S[:, 1] - mx, S[:, 2] - my
        out[1], out[2] = mx, my
        out[3] = (S[:, 3] + nr * ex * ex).sum()
        out[4] = (S[:, 4] + nr * ey * ey).sum()
        out[5] = (S[:, 5] + nr * ex * ey).sum()
    return out


def ccc_combine_chan(stats_all, mut=None):
    """Emulation of the finish kernel's combination: Chan et al.'s update in rank order, ranks
    without a valid element skipped ("empty_as_one": folded in as one element instead)."""
    n, mx, my, xx, yy, xy = (float(v) for v in stats_all[0][:6])
    pre = sum(float(s[6]) for s in stats_all)
    for s in stats_all[1:]:
        nb, bx, by, bxx, byy, bxy = (float(v) for v in s[:6])
        if nb <= 0:
            if mut != "empty_as_one":
                continue
            nb = 1.0
        if n <= 0:
            n, mx, my, xx, yy, xy = nb, bx, by, bxx, byy, bxy
            continue
        nt = n + nb
        dx, dy, f = bx - mx, by - my, n * nb / nt
        xx, yy, xy = xx + bxx + dx * dx * f, yy + byy + dy * dy * f, xy + bxy + dx * dy * f
        mx, my, n = mx + dx * nb / nt, my + dy * nb / nt, nt
    return torch.tensor([n, mx, my, xx, yy, xy, pre, 0.0], dtype=F64)


def ccc_loss(kind, s, bs, eps, dt=F64, mut=None):
    """The loss from whole-batch statistics, in `dt` (the kernel rounds the double statistics to
    fp32 and follows the fp32 op order of losses/loss.py:23-32 and losses/CCCLoss.py:24-43).
    bs (kind 1): the pre-mask size(0); < 0 stands for the summed pre-mask counts s[6]."""
    n, mx, my, xx, yy, xy = (s[i].to(dt) for i in range(6))
    nm1 = n if mut == "biased" else n - 1.0
    dm = mx - my
    if kind == 0:
        rho = xy / (torch.sqrt(xx) * torch.sqrt(yy) + eps)
        xs, ys = torch.sqrt(xx / nm1), torch.sqrt(yy / nm1)
        return 1.0 - 2.0 * rho * xs * ys / (xs * xs + ys * ys + dm * dm)
    if float(n) <= 1.0:
        return torch.zeros((), dtype=dt)
    b = n if mut == "bs_valid" else (s[6].to(dt) if bs < 0 else torch.tensor(float(bs), dtype=dt))
    x_std, y_std = torch.sqrt(yy / nm1), torch.sqrt(xx / nm1)
    den = x_std * x_std + y_std * y_std + dm * dm + 1e-8
    return 1.0 - 2.0 * xy / (den * b)


def _loss_derivs(kind, s, bs, eps, hessian=False):
    """dL/d(mx, my, Sxx, Syy, Sxy) of ccc_loss at s by float64 autograd (None where the loss
    does not depend on the statistics), and the 5 x 5 second derivatives when asked."""
    def f(v):
        return ccc_loss(kind, torch.cat([s[:1], v, s[6:]]), bs, eps)
    v = s[1:6].clone().requires_grad_(True)
    L = f(v)
    if not L.requires_grad:
        return None, None
    g, = torch.autograd.grad(L, v)
    H = torch.autograd.functional.hessian(f, s[1:6].clone()) if hessian else None
    return g, H


def ccc_coefs(kind, s, bs, eps, mut=None):
    """coef = (c0, c1, c2, mx, my, valid, 0, 0) with dL/dx_i = c0 + c1 (x_i - mx) + c2 (y_i - my):
    the chain rule through the statistics (d mx / dx_i = 1 / n, d Sxx / dx_i = 2 (x_i - mx),
    d Sxy / dx_i = y_i - my), the derivatives of the loss by autograd.  "grad_no_eps": the
    gradient of the eps-free kind-0 loss."""
    out = torch.zeros(8, dtype=F64)
    out[3], out[4] = s[1], s[2]
    g, _ = _loss_derivs(kind, s, bs, 0.0 if mut == "grad_no_eps" else eps)
    if g is not None:
        out[0], out[1], out[2], out[5] = g[0] / s[0], 2 * g[2], g[4], 1.0
    return out


def ccc_loss_cond(kind, st, k, bs, eps):
    """cond of the fp32 loss scalar: its own roundings, and every statistic's rounding to fp32
    (and at k > 1 its cond) carried through the loss's derivatives."""
    g, _ = _loss_derivs(kind, st.s, bs, eps)
    L = ccc_loss(kind, st.s, bs, eps)
    c = 1.0 + (1.0 - L).abs()
    if g is not None:
        c = c + (g.abs() * (st.s[1:6].abs() + (st.c[1:6] if k > 1 else 0.0))).sum()
    return c


def ccc_grad_cond(kind, st, k, bs, eps, grad_loss, G):
    """cond, in unit(k), of coef[0:3] and of the gradient G (= dL/dx per valid element, st's
    compacted order; for k > 1 the (valid, k) dL/dz): the statistics' cond through the second
    derivatives of the loss, plus the cancellation of (x_i - mx) and (y_i - my)."""
    g, H = _loss_derivs(kind, st.s, bs, eps, hessian=True)
    c_coef = torch.zeros(3, dtype=F64)
    if g is None:
        return c_coef, torch.zeros_like(G)
    n = st.s[0]
    dg = H.abs() @ st.c[1:6] + g.abs()
    c_coef = torch.stack([dg[0] / n, 2 * dg[2], dg[4]])
    dx, dy = st.x - st.s[1], st.y - st.s[2]
    a = abs(grad_loss)
    Gx = G if k == 1 else None
    if k > 1:
        p, b = st.pv.p.to(F64), st.pv.b.to(F64)
        w = p * (b - st.x[:, None])
        Gx = a * (g[0] / n + 2 * g[2] * dx + g[4] * dy)
    c = a * (c_coef[0] + c_coef[1] * dx.abs() + 2 * g[2].abs() * (st.cx + st.c[1])
             + c_coef[2] * dy.abs() + g[4].abs() * (st.cy + st.c[2])) + Gx.abs()
    if k == 1:
        return c_coef, c
    rel = st.pv.rel.to(F64)
    c = c[:, None] * w.abs() + Gx.abs()[:, None] * p * (
        (1.0 + rel) * (b - st.x[:, None]).abs() + b.abs() + st.cx[:, None])
    return c_coef, c


def _scatter(vals, idx, n):
    out = torch.zeros((n,) + tuple(vals.shape[1:]), dtype=vals.dtype)
    out[idx] = vals
    return out


def ccc_grad(kind, preds, labels, k, ignore, lo, hi, bs, eps, grad_loss=1.0):
    """(loss, [dL/dpred of every rank], the gradient of the valid elements alone) by float64
    autograd through the float64 loss formulas of oracle/jmt_ref.py over the ranks' concatenated
    batch, times grad_loss.  Ignored elements are compacted away first and get exact zeros.  The
    oracle's ignore-masked loss divides by its input's size(0): it is called on the (1, N) view
    (bs = 1) and the ccc term divided by bs."""
    pred, label = torch.cat(list(preds)), torch.cat(list(labels))
    n = label.numel()
    keep = torch.ones(n, dtype=torch.bool) if kind == 0 else label != ignore
    idx = torch.nonzero(keep).flatten()
    z = pred[idx].to(F64).clone().requires_grad_(True)
    y = label[idx].to(F64)
    x = pred_value(z, k, lo, hi).x
    m = idx.numel()
    if kind == 0:
        L = O.ccc_loss(x.view(1, m), y.view(1, m), eps=eps, digitize_num=1)
    else:
        L1 = O.ccc_loss_ignore(x.view(1, m), y.view(1, m), ignore=ignore)
        b = float(bs) if bs > 0 else float(n)
        L = 1.0 - (1.0 - L1) / b if L1.requires_grad else L1.to(F64)
    gz = torch.zeros_like(z)
    if L.requires_grad:
        gz, = torch.autograd.grad(L, z)
    full = _scatter(gz.detach() * grad_loss, idx, n)
    grads = list(full.split([t.numel() for t in labels]))
    return L.detach().to(F64), grads, gz.detach() * grad_loss


def ccc_grad_emu(kind, coef, pred, label, k, ignore, lo, hi, grad_loss, sum_, out_dtype):
    """The backward kernel's evaluation from given coef: double at k = 1, the softmax part in
    fp32 at k > 1; rounded to fp32, then to the stored type."""
    n = label.numel()
    keep = torch.ones(n, dtype=torch.bool) if kind == 0 else label != ignore
    if float(coef[5]) == 0.0:
        keep = torch.zeros(n, dtype=torch.bool)
    idx = torch.nonzero(keep).flatten()
    pv = pred_value(pred[idx].to(FS), k, lo, hi, sum_)
    d = (coef[0] + coef[1] * (pv.x.to(F64) - coef[3]) + coef[2] * (label[idx].to(F64) - coef[4])
         ) * grad_loss
    d = d.float()
    if k > 1:
        d = d[:, None] * pv.p * (pv.b - pv.x[:, None])
    return _scatter(d, idx, n).to(out_dtype)


def ccc_reference(kind, preds, labels, k, ignore, lo, hi, bs, eps, grad_loss=1.0):
    """Everything the three kernels produce for ranks `preds` / `labels`, in float64, with cond:
    st (whole-batch statistics), loss, coef[0:8], the ranks' gradients."""
    st = ccc_stats_cat(kind, preds, labels, k, ignore, lo, hi)
    L, grads, gz = ccc_grad(kind, preds, labels, k, ignore, lo, hi, bs, eps, grad_loss)
    c_coef3, c_gz = ccc_grad_cond(kind, st, k, bs, eps, grad_loss, gz)
    n = sum(t.numel() for t in labels)
    c_grads = list(_scatter(c_gz, st.idx, n).split([t.numel() for t in labels]))
    coef = ccc_coefs(kind, st.s, bs, eps)
    c_coef = torch.zeros(8, dtype=F64)
    c_coef[0:3], c_coef[3], c_coef[4] = c_coef3, st.c[1], st.c[2]
    return NS(st=st, loss=L, c_loss=ccc_loss_cond(kind, st, k, bs, eps), coef=coef, c_coef=c_coef,
              grads=grads, c_grads=c_grads)


def ccc_emulate(kind, preds, labels, k, ignore, lo, hi, bs, eps, grad_loss, sum_, mut=None):
    """The three kernels as an honest fp32 / double mix (see the module docstring): the ranks'
    statistics, their combination by Chan's update, the fp32 loss, coef and the gradients in the
    predictions' own dtype.  `mut` switches one defect on (tests/test_loss_ref.py)."""
    ranks = [ccc_stats(kind, p, y, k, ignore, lo, hi, sum_, FS, mut)
             for p, y in zip(preds, labels)]
    s = ccc_combine_chan([r.s for r in ranks], mut)
    loss = ccc_loss(kind, s, bs, eps, FS, mut)
    coef = ccc_coefs(kind, s, bs, eps, mut)
    if mut == "bs_valid":
        coef = ccc_coefs(kind, s, int(s[0]), eps)
    grads = [ccc_grad_emu(kind, coef, p, y, k, ignore, lo, hi, grad_loss, sum_, p.dtype)
             for p, y in zip(preds, labels)]
    return NS(ranks=ranks, s=s, loss=loss, coef=coef, grads=grads)


# ------------------------------------------------------------------------------- CE
def ce_edges(k, lo, hi):
    return np.linspace(lo, hi, num=k + 1)


def ce_bins(label, k, lo, hi, mut=None):
    """np.digitize(y, linspace(lo, hi, k + 1)) - 1 with the top bin clamped; NaN -> k - 1 (numpy
    puts it past the last edge); a label below lo -> -1.  "edges_fp32": edges rounded to fp32."""
    e = ce_edges(k, lo, hi)
    if mut == "edges_fp32":
        e = e.astype(np.float32)
    c = np.digitize(label.numpy(), e) - 1
    c[c == k] = k - 1
    return torch.from_numpy(c.astype(np.int64))


def _ce_rows(x, dt, sum_):
    z = x.to(dt)
    m = z.max(1, keepdim=True).values
    d = z - m
    e = _exp(d)
    s = sum_(e, 1)
    p = e / s[:, None]
    S = sum_(p * (1.0 + d.abs()), 1)
    return z, m[:, 0], d, s, p, S


def ce_stats(x, cls, w, sum_=sum_exact, dt=F64):
    """s = (sum w nll, sum w, labels below lo, 0) of one rank with nll_i = logsumexp(x_i) -
    x_i[c_i] (rows with c_i = -1 only counted), and cond c of s[0], s[1] in 2^-24."""
    ok = cls >= 0
    z, m, d, s, p, S = _ce_rows(x[ok], dt, sum_)
    c = cls[ok]
    zc = z.gather(1, c[:, None])[:, 0]
    nll = ((m + _log(s)) - zc).to(F64)
    wi = (w.to(F64)[c] if w is not None else torch.ones(c.numel(), dtype=F64))
    c_nll = (m.abs() + _log(s).abs() + zc.abs() + S + nll.abs().to(dt)).to(F64)
    out = torch.tensor([0.0, 0.0, float((~ok).sum()), 0.0], dtype=F64)
    out[0], out[1] = sum_(wi * nll, 0), sum_(wi, 0)
    cs = torch.zeros(4, dtype=F64)
    cs[0], cs[1] = sum_(wi * c_nll, 0), out[1]
    return NS(s=out, c=cs)


def ce_loss(stats_all):
    """loss = sum w nll / sum w over the ranks (NaN with any label below lo), coef = 1 / sum w,
    and the loss's cond from the ranks' cond."""
    S = torch.stack([st.s for st in stats_all])
    C = torch.stack([st.c for st in stats_all])
    sl, sw, bad = S[:, 0].sum(), S[:, 1].sum(), S[:, 2].sum()
    if float(bad) > 0:
        nan = torch.tensor(math.nan, dtype=F64)
        return NS(loss=nan, coef=nan, c_loss=nan, c_coef=nan)
    loss = sl / sw
    return NS(loss=loss, coef=1.0 / sw, c_loss=C[:, 0].sum() / sw + loss.abs(),
              c_coef=C[:, 1].sum() / (sw * sw))


def ce_grad(x, cls, w, sw, grad_loss=1.0):
    """d loss / d logits = grad_loss w[c_i] / sum w (softmax(x_i) - onehot(c_i)) by float64
    autograd through float64 log-softmax (sw: the ranks' summed weight); NaN rows where c_i = -1.
    Returns the gradient and its cond in 2^-24."""
    ok = cls >= 0
    z = x.to(F64).clone().requires_grad_(True)
    lp = torch.log_softmax(z, 1)
    c = cls.clamp(min=0)
    wi = (w.to(F64)[c] if w is not None else torch.ones(c.numel(), dtype=F64))
    L = (wi * -lp.gather(1, c[:, None])[:, 0])[ok].sum() / sw
    g, = torch.autograd.grad(L, z)
    g = g * grad_loss
    _, _, d, _, p, S = _ce_rows(x, F64, sum_exact)
    hot = torch.zeros_like(p).scatter_(1, c[:, None], 1.0)
    sc = (wi / sw * abs(grad_loss))[:, None]
    # FLUSH: an fp32 softmax entry below the smallest normal number is rounded on the subnormal
    # grid or flushed to zero (the hardware exp2 returns no subnormals): up to 2^-126, absolute
    cond = sc * (p * (3.0 + d.abs() + S[:, None]) + hot + FLUSH) + g.abs()
    g[~ok] = math.nan
    cond[~ok] = math.nan
    return g, cond


def ce_grad_emu(x, cls, w, coef, grad_loss, sum_, out_dtype):
    """The backward kernel's evaluation: the scale in double rounded to fp32, the rest fp32."""
    _, _, _, s, _, _ = _ce_rows(x, FS, sum_)
    z = x.to(FS)
    e = _exp(z - z.max(1, keepdim=True).values)
    c = cls.clamp(min=0)
    wi = (w.to(F64)[c] if w is not None else torch.ones(c.numel(), dtype=F64))
    sc = (wi * coef * grad_loss).float()
    sc[cls < 0] = math.nan
    hot = torch.zeros_like(e).scatter_(1, c[:, None], 1.0)
    return (sc[:, None] * (e * (1.0 / s)[:, None] - hot)).to(out_dtype)


# ------------------------------------------------------------------------------- mask_indices
def mask_indices(label, ignore):
    return np.flatnonzero(label.numpy() != np.float32(ignore))


def mask_indices_blocked(label, ignore, mut=None):
    """The kernel's scheme: BLOCK elements per trip, written from a running base ("base_stuck":
    advanced after the first trip only).  Returns (idx of length n, -1 where unwritten; count)."""
    y = label.numpy()
    n = y.size
    idx = np.full(n, -1, dtype=np.int64)
    base = 0
    for off in range(0, n, BLOCK):
        kept = off + np.flatnonzero(y[off:off + BLOCK] != np.float32(ignore))
        idx[base:base + kept.size] = kept
        if mut != "base_stuck" or off == 0:
            base += kept.size
    return idx, base


# ------------------------------------------------------------------------------- comparator
def bound(ref, cond, out_dtype, K, un):
    ref, cond = ref.to(F64), cond.to(F64)
    return U[out_dtype] * ref.abs().clamp(min=TINY[out_dtype]) + K * un * cond


def slack(got, ref, cond, out_dtype, un):
    """Largest (|got - ref| - u max(|ref|, tiny)) / (unit cond) over the elements whose reference
    is a number; elements with cond == 0 must be within the rounding term alone and count as 0
    (inf when they are not, and for a NaN where the reference has none or the reverse)."""
    got, ref, cond = got.to(F64), ref.to(F64), cond.to(F64)
    if got.numel() == 0:
        return 0.0
    if not torch.equal(torch.isnan(got), torch.isnan(ref)):
        return math.inf
    num = ~torch.isnan(ref)
    got, ref, cond = got[num], ref[num], cond[num]
    if got.numel() == 0:
        return 0.0
    over = (got - ref).abs() - U[out_dtype] * ref.abs().clamp(min=TINY[out_dtype])
    over = torch.where(torch.isnan(over), torch.full_like(over, math.inf), over)
    q = torch.where(over <= 0, torch.zeros_like(over), over / (un * cond))
    return float(q.max())


def check(got, ref, cond, out_dtype, K, un, what=""):
    """Fails unless |got - ref| <= u max(|ref|, tiny) + K unit cond for every element.  Where the
    reference is NaN the value must be NaN, and nowhere else."""
    got = torch.as_tensor(got).detach().cpu()
    ref, cond = torch.as_tensor(ref), torch.as_tensor(cond)
    assert got.shape == ref.shape == cond.shape, (what, got.shape, ref.shape, cond.shape)
    if got.numel() == 0:
        return 0.0
    g, r = got.to(F64), ref.to(F64)
    rn = torch.isnan(r)
    assert torch.equal(torch.isnan(g), rn), \
        f"{what}: NaN in {int((torch.isnan(g) != rn).sum())} places where the reference differs"
    b = bound(r, cond, out_dtype, K, un)
    err = (g - r).abs()
    bad = ~(err <= b) & ~rn
    ratio = torch.where(rn, torch.zeros_like(err), err / b.clamp(min=1e-300))
    if bad.any():
        i = int(torch.where(bad.flatten(), ratio.flatten().nan_to_num(nan=math.inf),
                            torch.zeros(())).argmax())
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {g.numel()} elements out of bound; worst at flat index "
            f"{i}: got {float(g.flatten()[i])!r} ref {float(r.flatten()[i])!r} bound "
            f"{float(b.flatten()[i]):.3e} cond {float(cond.to(F64).flatten()[i]):.3e}")
    return float(ratio.max())


def passes(*a, **kw):
    try:
        check(*a, **kw)
    except AssertionError:
        return False
    return True


# ------------------------------------------------------------------------------- case table
# CCC statistics -> finish -> backward of one rank.  pat (kind 1; kind 0 masks nothing):
#   none      nothing ignored
#   5pct      about 5 % ignored
#   head      every element below TAIL ignored: only the tail loops see a valid element
#   tail      every element from TAIL on ignored: the tail loops' own ignore test
#   all       all ignored
#   one_tail  exactly one valid element, in the tail
#   two_split exactly two valid elements, TAIL - 1 and the last
# data: "std" (mean 0.1, spread 0.3) or "himean" (mean 0.9, spread 1e-3: an un-centred second
# pass shows).  Ignored positions carry NaN / +Inf / -Inf predictions.
CccCase = namedtuple("CccCase", "kind n k dt pat data eps")
CCC_N = (1, 2, 63, 1024, 1025, 24575, 24576, 24577, 25637, 49157)   # 25637 = TAIL + 1024 + 37
CCC_PATS = ("none", "5pct", "head", "tail", "all", "one_tail", "two_split")
CCC_KDT = [(k, dt) for k in (1, 2, 5, 64) for dt in (FS, BF, FH)]
EPS_BIG = f32(0.5)      # an eps that the kind-0 gradient cannot lose unnoticed


def _ccc(kind, n, k=1, dt=FS, pat=None, data="std", eps=EPS):
    return CccCase(kind, n, k, dt, pat or ("none" if kind == 0 else "5pct"), data,
                   eps if kind == 0 else 0.0)


CCC_CASES = list(dict.fromkeys(
    # every n at k = 1, fp32: one block trip, the register-cached part full to the element, the
    # tail loops with 1, 1061 and 24581 elements
    [_ccc(kind, n) for kind in (0, 1) for n in CCC_N]
    # every (k, dtype) pair below and beyond TAIL; k = 2 and k = MAXK, 16-bit predictions,
    # digitized predictions with the ignore mask
    + [_ccc(kind, n, k, dt) for kind in (0, 1) for n in (1025, 24577) for k, dt in CCC_KDT]
    # every ignore pattern where a tail exists, and the ones that need none on small n
    + [_ccc(1, n, pat=p) for n in (25637, 49157) for p in CCC_PATS]
    + [_ccc(1, n, pat=p) for n in (1, 2, 1025) for p in ("none", "all")]
    + [_ccc(1, 24577, 5, BF, pat=p) for p in ("head", "two_split")]
    # mean far from zero relative to the spread
    + [_ccc(kind, n, data="himean") for kind in (0, 1) for n in (1025, 49157)]
    # kind 0 with an eps that matters
    + [_ccc(0, n, eps=EPS_BIG) for n in (2, 63)]
))
# n = 262144 + 300: one trip more than the 1024 x 256 threads of ccc_bwd / ce_bwd / ce_labels
GRID_N = 1024 * 256 + 300
CCC_GRID_CASES = [_ccc(0, GRID_N), _ccc(1, GRID_N)]
LO, HI = f32(-1.0), f32(1.0)
ADD = 0.8125 + 2.0 ** -20           # the fp32 scalar `add` of the fused l1 + l2
GRAD_LOSS = -2.5


def ccc_keep(n, pat, g):
    pos = torch.arange(n)
    if pat == "none":
        return torch.ones(n, dtype=torch.bool)
    if pat == "5pct":
        return torch.rand(n, generator=g) >= 0.05
    if pat == "head":
        return pos >= TAIL
    if pat == "tail":
        return pos < TAIL
    if pat == "all":
        return torch.zeros(n, dtype=torch.bool)
    if pat == "one":
        return pos == n // 2
    if pat == "one_tail":
        return pos == TAIL + (n - TAIL) // 2
    if pat == "two_split":
        return (pos == TAIL - 1) | (pos == n - 1)
    raise KeyError(pat)


def ccc_data(n, k, dt, pat, data, kind, tag=""):
    """pred ((n,) or (n, k), stored dtype) and label ((n,) fp32) of one rank."""
    g = _gen("ccc", n, k, DT_NAME[dt], pat, data, kind, tag)
    r1, r2 = torch.randn(n, generator=g), torch.randn(n, generator=g)
    if data == "himean":
        t = 0.9 + 1e-3 * r1
        y = 0.9 + 1e-3 * (0.7 * r1 + 0.7 * r2)
    else:
        t = 0.3 * r1 + 0.1
        y = (0.8 * t - 0.2 + 0.25 * r2).clamp(-1.0, 1.0)   # means 0.1 and -0.12 apart
    if k == 1:
        pred = t
    else:       # logits leaning to the label's bin, so that the expectation follows the label
        pred = 2.0 * torch.randn(n, k, generator=g)
        near = ((y + 1.0) * 0.5 * (k - 1)).round().long().clamp(0, k - 1)
        pred.scatter_add_(1, near[:, None], torch.full((n, 1), 3.0))
    keep = ccc_keep(n, pat, g) if kind == 1 else torch.ones(n, dtype=torch.bool)
    junk = torch.tensor([math.nan, math.inf, -math.inf])[torch.arange(n) % 3]
    y = torch.where(keep, y, torch.full_like(y, IGNORE))
    pred = torch.where(keep if k == 1 else keep[:, None], pred, junk if k == 1 else junk[:, None])
    return pred.to(dt), y


def ccc_inputs(c, tag=""):
    return ccc_data(c.n, c.k, c.dt, c.pat, c.data, c.kind, tag)


# Rank combination (k = 1, fp32): per rank (n, pattern), patterns as above plus "one" (a single
# valid element).  Kind 0 masks nothing, so there only the sizes matter (n = 0 is its empty rank).
RankCase = namedtuple("RankCase", "name ranks")
RANK_CASES = [
    RankCase("w1", ((300, "5pct"),)),
    RankCase("w2_first_none", ((200, "all"), (300, "5pct"))),
    RankCase("w2_first_n0", ((0, "none"), (300, "5pct"))),
    RankCase("w2_all_empty", ((50, "all"), (0, "none"))),
    RankCase("w2_n0_n0", ((0, "none"), (0, "none"))),
    RankCase("w8_unequal", ((100, "5pct"), (37, "all"), (0, "none"), (1, "none"), (500, "5pct"),
                            (64, "one"), (TAIL + 424, "5pct"), (3, "none"))),
    RankCase("w8_two_valid_apart", ((5, "all"), (64, "one"), (9, "all"), (0, "none"),
                                    (7, "all"), (2, "all"), (33, "one"), (1, "all"))),
    RankCase("w8_all_empty", tuple((n, "all") for n in (5, 0, 1, 1024, 1025, 3, 0, 64))),
]
RANK_BS = (1, 7, -1)


def rank_inputs(rc, kind):
    return [ccc_data(n, 1, FS, pat, "std", kind, f"{rc.name}.{r}")
            for r, (n, pat) in enumerate(rc.ranks)]


# CELoss.  w: None, "rand", or "zero" (random with one class weight 0).
CeCase = namedtuple("CeCase", "n k dt w lo hi")
CE_N = (1, 1023, 1024, 1025, 4133)
CE_RANGES = ((-1.0, 1.0), (0.0, 1.0), (-0.3, 2.5))


def _ce(n, k=7, dt=FS, w=None, rng=(-1.0, 1.0)):
    return CeCase(n, k, dt, w, f32(rng[0]), f32(rng[1]))


CE_CASES = list(dict.fromkeys(
    [_ce(n) for n in CE_N]
    + [_ce(1025, k, dt) for k in (2, 7, 64) for dt in (FS, BF, FH)]
    + [_ce(n, k, w=w) for n in (1025, 4133) for k in (2, 7, 64) for w in ("rand", "zero")]
    + [_ce(n, k, rng=r) for n in (1023, 4133) for k in (2, 7, 64) for r in CE_RANGES]
    + [_ce(4133, 64, BF, "rand", CE_RANGES[2])]
))
CE_GRID_CASE = _ce(GRID_N, 2)


def ce_edge_labels(k, lo, hi):
    """Every edge, one fp32 ulp on either side of it, hi, above hi and NaN (fp32); the one label
    below lo (an ulp under the first edge) left out."""
    e = ce_edges(k, lo, hi).astype(np.float32)
    big = np.float32(1e30)
    y = np.concatenate([e, np.nextafter(e, big), np.nextafter(e, -big),
                        np.array([hi, hi + 0.5, np.nan], np.float32)])
    return y[~(y < np.float32(lo))]


def ce_inputs(c, bad_label=False):
    """Logits ((n, k), stored dtype; every fourth row scaled to reach +-80), labels ((n,) fp32:
    the edge labels spread over the rows, uniform in [lo, hi] between them), weights or None."""
    g = _gen("ce", c.n, c.k, DT_NAME[c.dt], c.w, c.lo, c.hi)
    x = 3.0 * torch.randn(c.n, c.k, generator=g)
    x[::4] *= 80.0 / x[::4].abs().max()
    y = c.lo + (c.hi - c.lo) * torch.rand(c.n, generator=g)
    e = torch.from_numpy(ce_edge_labels(c.k, c.lo, c.hi))
    m = min(c.n, e.numel())
    step = max(1, c.n // m)
    y[0:m * step:step] = e[torch.randperm(e.numel(), generator=g)[:m]] if c.n < e.numel() else e
    if bad_label:
        y[c.n // 2] = float(np.nextafter(np.float32(c.lo), np.float32(-1e30)))
    w = None
    if c.w is not None:
        w = torch.rand(c.k, generator=g) + 0.5
        if c.w == "zero":
            w[c.k // 2] = 0.0
    return x.to(c.dt), y, w


# mask_indices
MASK_N = (0, 1, 63, 64, 1023, 1024, 1025, 2111, 19200)
MASK_PATS = ("all_kept", "none_kept", "random", "last_only")
MASK_CASES = [(n, p) for n in MASK_N for p in MASK_PATS]


def mask_inputs(n, pat):
    g = _gen("mask", n, pat)
    y = torch.rand(n, generator=g) * 2 - 1
    if pat == "none_kept":
        y[:] = IGNORE
    elif pat == "random":
        y[torch.rand(n, generator=g) < 0.4] = IGNORE
    elif pat == "last_only":
        y[:max(n - 1, 0)] = IGNORE
    return y
