"""CPU checks of tests/loss_ref.py: the float64 references agree with oracle/jmt_ref.py and the
committed golden loss cases, the comparator accepts honest fp32 / double evaluations of the same
formulas over the whole case table (so the bounds can be met) and rejects every listed mutation
of those evaluations (so the bounds and the table are tight enough)."""
import functools
import math
import warnings

import numpy as np
import pytest
import torch

from oracle import jmt_ref as O
from tests import loss_ref as R
from tests.golden import spec
from tests.loss_ref import BF, E24, F64, FS, IGNORE, LO, HI
from tests.oracle_cases import oracle_loss

SUMS = (R.sum_sequential, R.sum_pairwise)
warnings.filterwarnings("ignore", message="std\\(\\): degrees of freedom")


# ------------------------------------------------------------------ references vs the oracle
def _golden_eval(case):
    """Loss and gradient of one golden loss case through the float64 references."""
    x_np, y_np = spec.loss_inputs(case)
    x, y = torch.from_numpy(x_np), torch.from_numpy(y_np).reshape(-1)
    if case["kind"] == "ce":
        k = case["k"]
        cls = R.ce_bins(y, k, LO, HI)
        st = R.ce_stats(x, cls, None)
        g, _ = R.ce_grad(x, cls, None, st.s[1])
        return float(R.ce_loss([st]).loss), g.numpy()
    kind = 0 if case["kind"] == "ccc" else 1
    k = case.get("k", 1)
    bs = 1 if x.dim() == 2 else -1
    pred = x.reshape(-1) if k == 1 else x
    ref = R.ccc_reference(kind, [pred], [y], k, IGNORE, LO, HI, bs, R.EPS if kind == 0 else 0.0)
    # the statistics route (ccc_stats -> ccc_loss) and the oracle-autograd route give one loss
    L = R.ccc_loss(kind, ref.st.s, bs, R.EPS)
    assert abs(float(L) - float(ref.loss)) <= 1e-12 * max(1.0, abs(float(L)))
    return float(ref.loss), ref.grads[0].reshape(x.shape).numpy()


@pytest.mark.parametrize("case", spec.LOSS_CASES, ids=[c["tag"] for c in spec.LOSS_CASES])
def test_references_vs_golden_and_fp32_oracle(golden, case):
    l, g = _golden_eval(case)
    for rl, rg in ((float(golden[case["tag"] + "/loss"]), golden[case["tag"] + "/grad"]),
                   oracle_loss(case)):
        assert abs(l - rl) < 1e-5 * max(1.0, abs(l))
        assert np.abs(g - rg).max() <= 1e-5 * max(1.0, np.abs(rg).max())


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("rc", R.RANK_CASES, ids=lambda rc: rc.name)
def test_combine_is_the_whole_batch(rc, kind):
    """ccc_combine of the ranks' statistics == the statistics of the concatenated data, and so
    is Chan's update (the emulation of the finish kernel), to float64 rounding."""
    data = R.rank_inputs(rc, kind)
    preds, labels = [d[0] for d in data], [d[1] for d in data]
    whole = R.ccc_stats_cat(kind, preds, labels, 1, IGNORE, LO, HI)
    parts = [R.ccc_stats(kind, p, y, 1, IGNORE, LO, HI).s for p, y in data]
    for got in (R.ccc_combine(parts), R.ccc_combine_chan(parts)):
        assert float((got - whole.s).abs().max()) <= 1e-12 * max(1.0, float(whole.s.abs().max()))
        assert float(got[0]) == float(whole.s[0]) and float(got[6]) == float(whole.s[6])


@pytest.mark.parametrize("c", [R._ccc(0, 63), R._ccc(0, 63, eps=R.EPS_BIG), R._ccc(0, 1025, 5),
                               R._ccc(1, 1025), R._ccc(1, 1025, 5), R._ccc(0, 2),
                               R._ccc(1, 25637, pat="two_split")], ids=str)
@pytest.mark.parametrize("bs", [1, 7, -1])
def test_coef_chain_rule_equals_oracle_autograd(c, bs):
    """c0 + c1 (x - mx) + c2 (y - my) with coef from ccc_coefs (autograd through the statistics)
    is the oracle's autograd gradient: the two routes share no algebra."""
    pred, y = R.ccc_inputs(c)
    ref = R.ccc_reference(c.kind, [pred], [y], c.k, IGNORE, LO, HI, bs, c.eps, R.GRAD_LOSS)
    co, st = ref.coef, ref.st
    d = (co[0] + co[1] * (st.x - co[3]) + co[2] * (st.y - co[4])) * R.GRAD_LOSS
    if c.k > 1:
        d = d[:, None] * st.pv.p * (st.pv.b - st.x[:, None])
    got = R._scatter(d, st.idx, c.n)
    assert float(co[5]) == 1.0
    assert float((got - ref.grads[0]).abs().max()) <= 1e-11 * float(ref.grads[0].abs().max())


def test_bins_and_ce_bins():
    assert torch.equal(R.bins(5, -1.0, 1.0), torch.tensor([-1.0, -0.5, 0.0, 0.5, 1.0]))
    for k in (2, 7, 64):
        for lo, hi in R.CE_RANGES:
            lo, hi = R.f32(lo), R.f32(hi)
            y = np.concatenate([R.ce_edge_labels(k, lo, hi),
                                [np.nextafter(np.float32(lo), np.float32(-9))]]).astype(np.float32)
            e = R.ce_edges(k, lo, hi)
            ref = np.digitize(y, e) - 1
            ref[ref == k] = k - 1
            got = R.ce_bins(torch.from_numpy(y), k, lo, hi).numpy()
            np.testing.assert_array_equal(got, ref)
            # the definition, counted: edges <= y, minus one; NaN past the last edge
            cnt = (e[None, :] <= y[:, None].astype(np.float64)).sum(1) - 1
            cnt[np.isnan(y)] = k
            np.testing.assert_array_equal(got, np.minimum(cnt, k - 1))
            assert got[-1] == -1 and got.max() == k - 1 and got[:-1].min() == 0


@pytest.mark.parametrize("c", [R._ce(1025, 7, w="rand"), R._ce(4133, 64), R._ce(1023, 2)], ids=str)
def test_ce_reference_vs_oracle(c):
    x, y, w = R.ce_inputs(c)
    cls = R.ce_bins(y, c.k, c.lo, c.hi)
    st = R.ce_stats(x, cls, w)
    g, _ = R.ce_grad(x, cls, w, st.s[1], R.GRAD_LOSS)
    xr = x.float().requires_grad_(True)          # the oracle in fp32, as the golden cases run it
    ref = O.ce_loss(xr, y, c.k, rng=(c.lo, c.hi), weights=w)
    ref.backward()
    assert abs(float(R.ce_loss([st]).loss) - float(ref)) <= 1e-5 * max(1.0, abs(float(ref)))
    gr = R.GRAD_LOSS * xr.grad.double()
    assert float((g - gr).abs().max()) <= 1e-5 * max(1.0, float(gr.abs().max()))


def test_summations_and_intrinsic_model():
    a = torch.randn(3, 1000, generator=torch.Generator().manual_seed(1))
    assert not torch.equal(R.sum_sequential(a, 1), R.sum_pairwise(a, 1))
    assert torch.equal(R.sum_sequential(a[:1, :3], 1), (a[:1, 0] + a[:1, 1]) + a[:1, 2])
    assert R.sum_sequential(a[:, :0], 1).shape == (3,)
    # the fp32 exp model differs from a correctly rounded exp by the argument's rounding
    x = torch.linspace(-80, 0, 4001)
    rel = ((R._exp(x).double() - torch.exp(x.double())) / torch.exp(x.double())).abs()
    assert 0 < float(rel.max()) <= (80 * math.log2(math.e) + 2) * E24


@pytest.mark.parametrize("n,pat", R.MASK_CASES)
def test_mask_indices_blocked_scheme(n, pat):
    y = R.mask_inputs(n, pat)
    idx, cnt = R.mask_indices_blocked(y, IGNORE)
    ref = R.mask_indices(y, IGNORE)
    assert cnt == ref.size and np.array_equal(idx[:cnt], ref) and (idx[cnt:] == -1).all()


# ------------------------------------------------------------------ the case table, evaluated
def _ccc_results(kind, preds, labels, k, bs_list, eps, mut=None):
    """(family, got, ref, cond, out_dtype, unit) of every output, both emulations, each bs, with
    and without an upstream gradient."""
    un = R.unit(k)
    for bs in bs_list:
        for gl in (1.0, R.GRAD_LOSS):
            ref = R.ccc_reference(kind, preds, labels, k, IGNORE, LO, HI, bs, eps, gl)
            for s in SUMS:
                e = R.ccc_emulate(kind, preds, labels, k, IGNORE, LO, HI, bs, eps, gl, s, mut)
                if len(preds) == 1:
                    one = R.ccc_stats(kind, preds[0], labels[0], k, IGNORE, LO, HI)
                    yield "stats", e.ranks[0].s, one.s, one.c, F64, un
                yield "stats", e.s, ref.st.s, ref.st.c, F64, un
                yield "loss", e.loss.double(), ref.loss, ref.c_loss, FS, E24
                yield "stats", e.coef, ref.coef, ref.c_coef, F64, un
                for ge, gr, gc, p in zip(e.grads, ref.grads, ref.c_grads, preds):
                    yield "grad", ge, gr, gc, p.dtype, un


def _ccc_case_results(c, mut=None):
    pred, y = R.ccc_inputs(c)
    yield from _ccc_results(c.kind, [pred], [y], c.k, (1,), c.eps, mut)


def _rank_results(rc, kind, mut=None):
    data = R.rank_inputs(rc, kind)
    yield from _ccc_results(kind, [d[0] for d in data], [d[1] for d in data], 1,
                            R.RANK_BS if kind == 1 else (1,), R.EPS if kind == 0 else 0.0, mut)


def _ce_results(c, mut=None):
    x, y, w = R.ce_inputs(c)
    cls = R.ce_bins(y, c.k, c.lo, c.hi)
    st = R.ce_stats(x, cls, w)
    fin = R.ce_loss([st])
    cls_e = R.ce_bins(y, c.k, c.lo, c.hi, mut)
    for gl in (1.0, R.GRAD_LOSS):
        g, cg = R.ce_grad(x, cls, w, st.s[1], gl)
        for s in SUMS:
            e = R.ce_stats(x, cls_e, w, s, FS)
            fe = R.ce_loss([e])
            loss = e.s[0] / c.n if mut == "norm_by_n" else fe.loss
            yield "ce_loss", e.s[:2], st.s[:2], st.c[:2], F64, E24
            yield "ce_loss", loss.float().double(), fin.loss, fin.c_loss, FS, E24
            yield "ce_loss", fe.coef, fin.coef, fin.c_coef, F64, E24
            yield "ce_grad", R.ce_grad_emu(x, cls_e, w, fe.coef, gl, s, c.dt), g, cg, c.dt, E24


def _family_results():
    for c in R.CCC_CASES + R.CCC_GRID_CASES:
        yield from _ccc_case_results(c)
    for rc in R.RANK_CASES:
        for kind in (0, 1):
            yield from _rank_results(rc, kind)
    for c in R.CE_CASES + [R.CE_GRID_CASE]:
        yield from _ce_results(c)


FAMILY_K = {"stats": "K_STATS", "loss": "K_CCC_LOSS", "grad": "K_CCC_GRAD",
            "ce_loss": "K_CE_LOSS", "ce_grad": "K_CE_GRAD"}


@functools.lru_cache(maxsize=None)
def _measured():
    worst = {f: 0.0 for f in FAMILY_K}
    fails = {f: 0 for f in FAMILY_K}
    for fam, got, ref, cond, od, un in _family_results():
        worst[fam] = max(worst[fam], R.slack(got, ref, cond, od, un))
        fails[fam] += not R.passes(got, ref, cond, od, getattr(R, FAMILY_K[fam]), un)
    return worst, fails


@pytest.mark.parametrize("family", sorted(FAMILY_K))
def test_bound_accepts_emulations(family):
    """Both emulations pass `check` on every case of the table: the bounds can be met."""
    worst, fails = _measured()
    assert fails[family] == 0, (family, worst[family])


@pytest.mark.parametrize("family", sorted(FAMILY_K))
def test_k_is_4x_measured(family):
    """K is 4 x the largest slack of the emulations, rounded up by a few per cent, no more."""
    worst, _ = _measured()
    K = getattr(R, FAMILY_K[family])
    print(f"{family}: measured slack {worst[family]:.4f}, K = {K}")
    assert math.isfinite(worst[family]) and 4 * worst[family] <= K <= 4 * worst[family] * 1.15, \
        (family, worst[family], K)


# ------------------------------------------------------------------ mutations
def _rejected(results, family):
    """Does any output of `family` among `results` violate its bound?"""
    return any(not R.passes(got, ref, cond, od, getattr(R, FAMILY_K[fam]), un)
               for fam, got, ref, cond, od, un in results if fam == family)


TAIL_CASES = [c for c in R.CCC_CASES if c.n > R.TAIL and c.k == 1]


@pytest.mark.parametrize("mut", ["tail_dropped", "tail_uncentred", "tail_unmasked"])
def test_tail_mutations_rejected(mut):
    """Elements >= 24576 dropped; tail second pass un-centred; ignore mask not applied in the
    tail.  Each must show in the statistics of some case with a tail; the two that change a
    statistic beyond fp32 rounding also in the fp32 loss (raw moments in double lose about
    2^-53 n^1.5 mean^2, which only the float64 outputs can show)."""
    hit = {f: False for f in (("stats",) if mut == "tail_uncentred" else ("stats", "loss"))}
    for c in TAIL_CASES:
        res = list(_ccc_case_results(c, mut))
        for f in hit:
            hit[f] |= _rejected(res, f)
    assert all(hit.values()), (mut, hit)


def test_tail_mutations_need_their_cases():
    """Which part of the table each tail mutation is seen on: the un-centred pass only where the
    mean is far from zero relative to the spread, the missing mask only where the tail holds an
    ignored element, and no case without a tail sees any of them."""
    seen = {m: {c for c in TAIL_CASES if _rejected(_ccc_case_results(c, m), "stats")}
            for m in ("tail_uncentred", "tail_unmasked")}
    assert seen["tail_uncentred"] and all(c.data == "himean" for c in seen["tail_uncentred"])
    assert seen["tail_unmasked"] and all(c.kind == 1 and c.pat != "none"
                                         for c in seen["tail_unmasked"])
    for m in ("tail_dropped", "tail_uncentred", "tail_unmasked"):
        c = R._ccc(1, R.TAIL)
        assert not _rejected(_ccc_case_results(c, m), "stats")


@pytest.mark.parametrize("mut,family,cases", [
    ("biased", "loss", [R._ccc(0, 63), R._ccc(1, 1025), R._ccc(0, 49157)]),
    ("grad_no_eps", "grad", [R._ccc(0, 2, eps=R.EPS_BIG), R._ccc(0, 63, eps=R.EPS_BIG)]),
])
def test_formula_mutations_rejected(mut, family, cases):
    """Biased variance (n for n - 1) in the loss; the eps term dropped from the kind-0 gradient."""
    for c in cases:
        assert _rejected(_ccc_case_results(c, mut), family), (mut, c)


def test_bs_as_valid_count_rejected():
    """kind 1: bs taken as the valid count instead of the pre-mask size."""
    for c in (R._ccc(1, 1025), R._ccc(1, 25637, pat="head")):
        res = list(_ccc_case_results(c, "bs_valid"))
        assert _rejected(res, "loss") and _rejected(res, "grad"), c
    for rc in R.RANK_CASES:
        if rc.name in ("w2_first_none", "w8_unequal"):
            res = list(_rank_results(rc, 1, "bs_valid"))
            assert _rejected(res, "loss") and _rejected(res, "grad"), rc.name


def test_empty_rank_folded_in_rejected():
    """An empty rank folded in as if it had one element: seen in the statistics of every layout
    that has an empty rank after the first (kind 0 masks nothing: its empty ranks have n = 0)."""
    for rc in R.RANK_CASES:
        for kind in (0, 1):
            data = R.rank_inputs(rc, kind)
            valid = [int((y != IGNORE).sum()) if kind == 1 else y.numel() for _, y in data]
            expect = any(v == 0 for v in valid[1:])
            got = _rejected(_rank_results(rc, kind, "empty_as_one"), "stats")
            assert got == expect, (rc.name, kind, valid)
    unequal = next(rc for rc in R.RANK_CASES if rc.name == "w8_unequal")
    for kind in (0, 1):
        assert _rejected(_rank_results(unequal, kind, "empty_as_one"), "loss"), kind


def test_ce_mutations_rejected():
    """CE normalised by n instead of the summed weights; CE edges built in fp32."""
    assert _rejected(_ce_results(R._ce(1025, 7, w="rand"), "norm_by_n"), "ce_loss")
    assert not _rejected(_ce_results(R._ce(1025, 7), "norm_by_n"), "ce_loss")   # equal unweighted
    hit = {f: False for f in ("ce_loss", "ce_grad")}
    for c in R.CE_CASES:
        if c.n >= 1023 and c.w is None and c.dt == FS:
            res = list(_ce_results(c, "edges_fp32"))
            for f in hit:
                hit[f] |= _rejected(res, f)
    assert all(hit.values()), hit


def test_mask_indices_stuck_base_rejected():
    """base not advanced after the first 1024: every case with a kept element beyond the first
    trip differs, and no other."""
    for n, pat in R.MASK_CASES:
        y = R.mask_inputs(n, pat)
        ref = R.mask_indices(y, IGNORE)
        idx, cnt = R.mask_indices_blocked(y, IGNORE, "base_stuck")
        same = cnt == ref.size and np.array_equal(idx[:cnt], ref)
        assert same == (not (ref >= R.BLOCK).any()), (n, pat)
    assert any(n > R.BLOCK and p != "none_kept" for n, p in R.MASK_CASES)


def test_comparator_rejects_nan_and_unwritten():
    ref = torch.tensor([1.0, 0.0, math.nan], dtype=F64)
    cond = torch.tensor([1.0, 0.0, 1.0], dtype=F64)
    assert R.passes(torch.tensor([1.0, 0.0, math.nan]), ref, cond, FS, 1.0, E24)
    assert R.passes(torch.tensor([1.0, -0.0, math.nan]), ref, cond, FS, 1.0, E24)
    assert not R.passes(torch.tensor([1.0, math.nan, math.nan]), ref, cond, FS, 1.0, E24)
    assert not R.passes(torch.tensor([1.0, 0.0, 0.0]), ref, cond, FS, 1.0, E24)
    assert not R.passes(torch.tensor([1.0, 2.0 ** -140, math.nan]), ref, cond, FS, 1.0, E24)
    assert not R.passes(torch.tensor([1.0 + 2.0 ** -21, 0.0, math.nan]), ref, cond, FS, 1.0, E24)
    assert math.isinf(R.slack(torch.tensor([1.0, 0.0, 0.0]), ref, cond, FS, E24))
    assert R.passes(torch.tensor([1.0]).to(BF), torch.tensor([1.0 + 2.0 ** -9], dtype=F64),
                    torch.zeros(1, dtype=F64), BF, 0.0, E24)
