"""Key ranges in the attention kernels (include/jmt.h "Key ranges"): a key padding mask as one
run of valid keys [kbeg, kend) per sequence, read by the whole-row forward, the P / dS backward,
the short kernels and the range form of the softmax from a device table, entry n % kr_mod.

Inputs as tests/test_gpu_attn_short.py: randn packed q|k|v layouts, E = 512, scale 1/sqrt(512),
NaN-prefilled outputs.  References in fp32 / float64 torch from the same rounded inputs, masked
scores set to -inf before the softmax, lse over the valid keys.  Every sequence of a launch gets
a different range, so a range taken from the wrong item of a persistent block shows.

The short kernels' comparison against the long path of test_gpu_attn_short.py has no ranged
counterpart (the 64-row kernels take no ranges), so they are checked against fp32 only."""
import math

import pytest
import torch

from jmt import functional as JF
from jmt import ops
from jmt._lib import JMTError

from tests import rowops_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
E = 512
SCALE = 1.0 / math.sqrt(E)
NAN = float("nan")


def _st(t):
    return (t.stride(0), t.stride(1))


def _inputs(cd, Lq, Lk, N, H=1, seed=41):
    """q from a packed (Lq, N, 3E') buffer, k / v from a (Lk, N, 2E') one (E' = 512 H), dO
    contiguous."""
    Eh = E * H
    g = torch.Generator(device=DEV).manual_seed(seed)
    qkv = torch.randn(N, Lq, 3 * Eh, device=DEV, generator=g).to(cd).permute(1, 0, 2)
    kv = torch.randn(N, Lk, 2 * Eh, device=DEV, generator=g).to(cd).permute(1, 0, 2)
    go = torch.randn(Lq, N, Eh, device=DEV, generator=g).to(cd)
    return qkv, kv, go


def _table(ranges):
    """(device int32 table, kr_mod) of a list of (kbeg, kend)."""
    t = torch.tensor([v for r in ranges for v in r], dtype=torch.int32, device=DEV)
    return (t, len(ranges))


def _valid(ranges, N, Lk):
    """(N, Lk) bool, True where key k of sequence n is inside its range (entry n % len)."""
    k = torch.arange(Lk, device=DEV)
    rows = [(k >= ranges[n % len(ranges)][0]) & (k < ranges[n % len(ranges)][1]) for n in range(N)]
    return torch.stack(rows)


def _ref(qkv, kv, go, o, H, valid):
    """fp32 reference per head with masked scores at -inf: o, lse, dq, dk, dv (Delta from the
    16-bit O as the kernels)."""
    Eh = E * H
    outs = []
    for h in range(H):
        sl = slice(h * E, (h + 1) * E)
        q = qkv[..., :Eh][..., sl].float()
        k = kv[..., :Eh][..., sl].float()
        v = kv[..., Eh:][..., sl].float()
        s = torch.einsum("lnd,knd->nlk", q, k) * SCALE
        s = s.masked_fill(~valid[:, None, :], -math.inf)
        p = torch.softmax(s, -1)
        r = dict(o=torch.einsum("nlk,knd->lnd", p, v), lse=torch.logsumexp(s, -1), p=p)
        if go is not None:
            d = go[..., sl].float()
            dp = torch.einsum("lnd,knd->nlk", d, v)
            delta = (d * o[..., sl].float()).sum(-1).t().unsqueeze(-1)
            ds = p * (dp - delta) * SCALE
            r.update(dq=torch.einsum("nlk,knd->lnd", ds, k), dk=torch.einsum("nlk,lnd->knd", ds, q),
                     dv=torch.einsum("nlk,lnd->knd", p, d), dpmax=dp.abs().max().item())
        outs.append(r)
    return outs


def _check_fwd(cd, o, lse, refs, Lq, N, H):
    for h, r in enumerate(refs):
        sl = slice(h * E, (h + 1) * E)
        tol = (1e-2 if cd == torch.bfloat16 else 2e-3) * max(r["o"].abs().max().item(), 1.0)
        err = (o[..., sl].float() - r["o"]).abs().max().item()
        print(f"h{h} o err {err:.3e} tol {tol:.3e}")
        assert err <= tol
        got = lse.view(N, H, Lq)[:, h]
        lerr = (got - r["lse"]).abs().max().item()
        ltol = 1e-3 * max(r["lse"].abs().max().item(), 1.0)
        print(f"h{h} lse err {lerr:.3e} tol {ltol:.3e}")
        assert lerr <= ltol


def _check_bwd(cd, qkv, kv, dq, dk, dv, refs, H):
    """The bounds of test_short_bwd_vs_fp32_and_long_path."""
    Eh = E * H
    u = 2.0 ** -8 if cd == torch.bfloat16 else 2.0 ** -11
    for h, r in enumerate(refs):
        sl = slice(h * E, (h + 1) * E)
        floor = 4 * u * SCALE * r["dpmax"]
        qmax = qkv[..., :Eh][..., sl].float().abs().max().item()
        kmax = kv[..., :Eh][..., sl].float().abs().max().item()
        for name, t, rel, fl in (("dq", dq, 16, floor * kmax), ("dk", dk, 16, floor * qmax),
                                 ("dv", dv, 8, 0.0)):
            err = (t[..., sl].float() - r[name]).abs().max().item()
            tol = rel * u * r[name].abs().max().item() + fl
            print(f"h{h} {name} err {err:.3e} tol {tol:.3e}")
            assert err <= tol, name


# ------------------------------------------------------------------ whole-row forward, P / dS
def _rows_fwd(cd, qkv, kv, Lq, Lk, N, H, kr, qshare=None, q=None):
    Eh = E * H
    qsrc = qkv if q is None else q
    qp, kp, vp = qsrc[..., :Eh], kv[..., :Eh], kv[..., Eh:]
    o = torch.full((Lq, N, Eh), NAN, device=DEV, dtype=cd)
    lse = torch.full((N * H * Lq,), NAN, device=DEV)
    fn = ops.attn_fwd if qshare is None else ops.attn_fwd_sq
    fn(ops.dt(kv), N, H, Lq, Lk, E, qp.data_ptr(), _st(qsrc), kp.data_ptr(), _st(kv),
       vp.data_ptr(), _st(kv), o.data_ptr(), _st(o), SCALE, lse, *(qshare or ()),
       **({} if kr is None else {"kr": kr}))
    return o, lse


def _rows_pds(cd, qkv, kv, go, o, lse, Lq, Lk, N, H, kr, qshare=None, q=None):
    """Tile-major P / dS of the P / dS kernel into NaN-prefilled buffers."""
    Eh = E * H
    qsrc = qkv if q is None else q
    ldp = ops.attn_dkdv_ldp(Lk)
    P = torch.full((N * H * Lq * ldp,), NAN, device=DEV, dtype=cd)
    dS = torch.full((N * H * Lq * ldp,), NAN, device=DEV, dtype=cd)
    args = (ops.dt(kv), N, H, Lq, Lk, E, go.data_ptr(), _st(go), o.data_ptr(), _st(o),
            qsrc[..., :Eh].data_ptr(), _st(qsrc), kv[..., :Eh].data_ptr(), _st(kv),
            kv[..., Eh:].data_ptr(), _st(kv), lse, P, dS, ldp)
    krk = {} if kr is None else {"kr": kr}
    if qshare is None:
        ops.attn_bwd(*args, None, (0, 0), SCALE, **krk)
    else:
        ops.attn_bwd_sq(*args, SCALE, *qshare, **krk)
    return P, dS, ldp


def _rows_dkdv(cd, qkv, kv, go, P, dS, ldp, Lq, Lk, N, H):
    """dQ / dK / dV by jmt_attn_dkdv (unchanged by key ranges) into NaN-poisoned packed buffers;
    the untouched neighbours must stay NaN."""
    Eh = E * H
    dqkv = torch.full((N, Lq, 3 * Eh), NAN, device=DEV, dtype=cd).permute(1, 0, 2)
    dkv = torch.full((N, Lk, 2 * Eh), NAN, device=DEV, dtype=cd).permute(1, 0, 2)
    ops.attn_dkdv(ops.dt(kv), N, H, Lq, Lk, E, P, dS, ldp, go.data_ptr(), _st(go),
                  qkv[..., :Eh].data_ptr(), _st(qkv), dkv[..., :Eh].data_ptr(), _st(dkv),
                  dkv[..., Eh:].data_ptr(), _st(dkv), kv[..., :Eh].data_ptr(), _st(kv),
                  dqkv[..., Eh:2 * Eh].data_ptr(), _st(dqkv))
    torch.cuda.synchronize()
    assert torch.isnan(dqkv[..., :Eh].float()).all() and torch.isnan(dqkv[..., 2 * Eh:].float()).all()
    return dqkv[..., Eh:2 * Eh], dkv[..., :Eh], dkv[..., Eh:]


def _tiles(X, N, H, Lq, Lk, ldp):
    """The written tiles of a tile-major P / dS buffer as (N, H, Lq, 32 ceil(Lk / 32)) keys."""
    nt = -(-Lk // 32)
    t = X.view(N * H, ldp // 32, Lq, 32)[:, :nt]
    return t.permute(0, 2, 1, 3).reshape(N, H, Lq, nt * 32)


def _ranges6(Lk):
    return [(0, Lk), (0, 1), (37, Lk), (32, 64), (31, 33), (5, 29)]


def _run_rows(cd, Lq, Lk, N, H, kr, qkv, kv, go):
    o, lse = _rows_fwd(cd, qkv, kv, Lq, Lk, N, H, kr)
    P, dS, ldp = _rows_pds(cd, qkv, kv, go, o, lse, Lq, Lk, N, H, kr)
    dq, dk, dv = _rows_dkdv(cd, qkv, kv, go, P, dS, ldp, Lq, Lk, N, H)
    return dict(o=o, lse=lse, P=_tiles(P, N, H, Lq, Lk, ldp), dS=_tiles(dS, N, H, Lq, Lk, ldp),
                dq=dq.contiguous(), dk=dk.contiguous(), dv=dv.contiguous())


@pytest.mark.parametrize("cd", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("Lq,Lk,N,H,first", [(130, 100, 6, 1, 0), (70, 70, 4, 2, 0), (70, 70, 4, 2, 2)])
def test_rows_fwd_pds_with_ranges(cd, Lq, Lk, N, H, first):
    # one range of the list per sequence; the 4-sequence shape takes the six in two passes
    ranges = _ranges6(Lk)[first:first + N]
    assert len(ranges) == N
    kr = _table(ranges)
    valid = _valid(ranges, N, Lk)
    qkv, kv, go = _inputs(cd, Lq, Lk, N, H)
    got = _run_rows(cd, Lq, Lk, N, H, kr, qkv, kv, go)
    refs = _ref(qkv, kv, go, got["o"], H, valid)
    _check_fwd(cd, got["o"], got["lse"], refs, Lq, N, H)
    _check_bwd(cd, qkv, kv, got["dq"], got["dk"], got["dv"], refs, H)
    # exact: P and dS zero in every masked column of every written tile (keys past Lk too)
    nk = got["P"].shape[-1]
    vpad = torch.zeros(N, nk, dtype=torch.bool, device=DEV)
    vpad[:, :Lk] = valid
    for name in ("P", "dS"):
        t = got[name].float()
        assert not torch.isnan(t).any(), name
        masked = t.masked_select(~vpad[:, None, None, :].expand_as(t))
        assert bool((masked == 0).all()), name
    # dK and dV rows of masked keys are exact zeros
    for name in ("dk", "dv"):
        t = got[name].float()                      # (Lk, N, E')
        assert bool((t.permute(1, 0, 2)[~valid] == 0).all()), name
    # other finite K / V rows outside the ranges change no output bit
    g = torch.Generator(device=DEV).manual_seed(5)
    kv2 = kv.clone()
    noise = torch.randn(kv.shape, device=DEV, generator=g).to(cd) * 3
    sel = (~valid).t()[:, :, None].expand_as(kv2)      # (Lk, N, 2E')
    kv2 = torch.where(sel, noise, kv2)
    kv2 = kv2.permute(1, 0, 2).contiguous().permute(1, 0, 2)
    got2 = _run_rows(cd, Lq, Lk, N, H, kr, qkv, kv2, go)
    for name in ("o", "lse", "P", "dS", "dq"):
        assert torch.equal(got[name], got2[name]), name
    for name in ("dk", "dv"):                      # valid keys' rows; masked rows are zero in both
        assert torch.equal(got[name], got2[name]), name


@pytest.mark.parametrize("cd", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("Lq,Lk,N,H", [(130, 100, 6, 1), (70, 70, 4, 2)])
def test_rows_full_ranges_are_bit_identical_to_no_ranges(cd, Lq, Lk, N, H):
    qkv, kv, go = _inputs(cd, Lq, Lk, N, H, seed=43)
    a = _run_rows(cd, Lq, Lk, N, H, None, qkv, kv, go)
    b = _run_rows(cd, Lq, Lk, N, H, _table([(0, Lk)] * 2), qkv, kv, go)
    for name in a:
        assert torch.equal(a[name], b[name]), name


def test_rows_more_items_than_cus_every_neighbour_differs():
    cd, Lq, Lk, N, H = torch.bfloat16, 130, 70, 300, 1
    ranges = [(5 * (n % 7), 70 - 9 * (n % 5)) for n in range(N)]
    kr = _table(ranges)
    valid = _valid(ranges, N, Lk)
    qkv, kv, go = _inputs(cd, Lq, Lk, N, H, seed=47)
    got = _run_rows(cd, Lq, Lk, N, H, kr, qkv, kv, go)
    refs = _ref(qkv, kv, go, got["o"], H, valid)
    _check_fwd(cd, got["o"], got["lse"], refs, Lq, N, H)
    _check_bwd(cd, qkv, kv, got["dq"], got["dk"], got["dv"], refs, H)
    assert bool((got["dk"].float().permute(1, 0, 2)[~valid] == 0).all())
    assert bool((got["dv"].float().permute(1, 0, 2)[~valid] == 0).all())


def test_bad_table_is_clamped():
    """Ranges outside [0, Lk] and kend < kbeg are clamped in the kernel: the results are those of
    the clamped table (an empty range gives unspecified values and is not part of this case)."""
    cd, Lq, Lk, N, H = torch.bfloat16, 130, 100, 4, 1
    qkv, kv, go = _inputs(cd, Lq, Lk, N, H, seed=53)
    a = _run_rows(cd, Lq, Lk, N, H, _table([(-7, 1 << 30), (-(1 << 31), 50), (90, 101), (3, 100)]),
                  qkv, kv, go)
    b = _run_rows(cd, Lq, Lk, N, H, _table([(0, 100), (0, 50), (90, 100), (3, 100)]), qkv, kv, go)
    for name in a:
        assert torch.equal(a[name], b[name]), name


def test_masked_index_query_rows_do_not_move_their_wave_neighbours():
    """Where queries and keys share the axis, a padded frame is a query row too.  The forward's
    lazy-rescale vote is per wave of 16 query rows; with ranges, rows whose own index is a masked
    key stay out of the other rows' vote, so other values in them change no bit of a valid row
    (scores spread widely here, so that rescales after the first tile do happen)."""
    cd, L, N = torch.bfloat16, 70, 3
    ranges = [(23, L), (0, 50), (5, 61)]
    kr = _table(ranges)
    valid = _valid(ranges, N, L)
    g = torch.Generator(device=DEV).manual_seed(67)
    q = (torch.randn(N, L, E, device=DEV, generator=g) * 6).to(cd).permute(1, 0, 2)
    kv = torch.randn(N, L, 2 * E, device=DEV, generator=g).to(cd).permute(1, 0, 2)
    noise = (torch.randn(N, L, E, device=DEV, generator=g) * 6).to(cd).permute(1, 0, 2)
    q2 = torch.where((~valid).t()[:, :, None], noise, q)
    q2 = q2.permute(1, 0, 2).contiguous().permute(1, 0, 2)
    o1, lse1 = _rows_fwd(cd, q, kv, L, L, N, 1, kr, q=q)
    o2, lse2 = _rows_fwd(cd, q, kv, L, L, N, 1, kr, q=q2)
    torch.cuda.synchronize()
    rows = valid.t()                                           # (L, N)
    assert not torch.equal(o1[~rows], o2[~rows])
    assert torch.equal(o1[rows], o2[rows])
    assert torch.equal(lse1.view(N, L)[valid], lse2.view(N, L)[valid])
    r = _ref(q, kv, None, None, 1, valid)[0]
    assert (o1.float() - r["o"]).abs().max().item() <= 1e-2 * max(r["o"].abs().max().item(), 1.0)


# ------------------------------------------------------------------ _sq forms
def test_sq_forms_equal_unshared_ranged_entry_points():
    cd, Lq, Lk, H, spp = torch.bfloat16, 130, 100, 1, 3
    qtab = [0, 0]                                   # pair 1 reads pair 0's queries
    N = len(qtab) * spp
    kr = _table([(0, Lk), (37, Lk), (31, 33)])
    qkv, kv, go = _inputs(cd, Lq, Lk, N, H, seed=59)
    # the Q buffer that holds each query once per sequence
    src = [qtab[n // spp] * spp + n % spp for n in range(N)]
    qfull = qkv[:, src].permute(1, 0, 2).contiguous().permute(1, 0, 2)
    o1, lse1 = _rows_fwd(cd, qkv, kv, Lq, Lk, N, H, kr, qshare=(spp, qtab))
    o2, lse2 = _rows_fwd(cd, qkv, kv, Lq, Lk, N, H, kr, q=qfull)
    P1, dS1, ldp = _rows_pds(cd, qkv, kv, go, o1, lse1, Lq, Lk, N, H, kr, qshare=(spp, qtab))
    P2, dS2, _ = _rows_pds(cd, qkv, kv, go, o2, lse2, Lq, Lk, N, H, kr, q=qfull)
    torch.cuda.synchronize()
    assert not torch.equal(qfull[..., :E], qkv[..., :E])       # the table is not the identity
    assert torch.equal(o1, o2) and torch.equal(lse1, lse2)
    assert torch.equal(_tiles(P1, N, H, Lq, Lk, ldp), _tiles(P2, N, H, Lq, Lk, ldp))
    assert torch.equal(_tiles(dS1, N, H, Lq, Lk, ldp), _tiles(dS2, N, H, Lq, Lk, ldp))
    refs = _ref(qfull, kv, None, None, H, _valid([(0, Lk), (37, Lk), (31, 33)], N, Lk))
    _check_fwd(cd, o1, lse1, refs, Lq, N, H)


# ------------------------------------------------------------------ short kernels
@pytest.mark.parametrize("cd", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("Lq,Lk,N", [(32, 32, 7), (9, 17, 5), (1, 32, 3), (32, 1, 2)])
def test_short_kernels_with_ranges(cd, Lq, Lk, N):
    # [0, Lk), [3, Lk), [0, Lk - 2), [Lk - 1, Lk) cycled over n; at Lk = 1 the two that would be
    # empty (unspecified values) become the nearest non-empty range
    cyc = [(0, Lk), (min(3, Lk - 1), Lk), (0, max(Lk - 2, 1)), (Lk - 1, Lk)]
    ranges = [cyc[n % 4] for n in range(N)]
    kr = _table(ranges)
    valid = _valid(ranges, N, Lk)
    qkv, kv, go = _inputs(cd, Lq, Lk, N)
    o = torch.full((Lq, N, E), NAN, device=DEV, dtype=cd)
    lse = torch.full((N * Lq,), NAN, device=DEV)
    ops.attn_short_fwd(ops.dt(qkv), N, 1, Lq, Lk, E, qkv[..., :E].data_ptr(), _st(qkv),
                       kv[..., :E].data_ptr(), _st(kv), kv[..., E:].data_ptr(), _st(kv),
                       o.data_ptr(), _st(o), SCALE, lse, kr=kr)
    dqkv = torch.full((N, Lq, 3 * E), NAN, device=DEV, dtype=cd).permute(1, 0, 2)
    dkv = torch.full((N, Lk, 2 * E), NAN, device=DEV, dtype=cd).permute(1, 0, 2)
    ops.attn_short_bwd(ops.dt(qkv), N, 1, Lq, Lk, E, go.data_ptr(), _st(go), o.data_ptr(), _st(o),
                       qkv[..., :E].data_ptr(), _st(qkv), kv[..., :E].data_ptr(), _st(kv),
                       kv[..., E:].data_ptr(), _st(kv), lse, dqkv[..., E:2 * E].data_ptr(),
                       _st(dqkv), dkv[..., :E].data_ptr(), _st(dkv), dkv[..., E:].data_ptr(),
                       _st(dkv), SCALE, kr=kr)
    torch.cuda.synchronize()
    assert torch.isnan(dqkv[..., :E].float()).all() and torch.isnan(dqkv[..., 2 * E:].float()).all()
    dq, dk, dv = dqkv[..., E:2 * E], dkv[..., :E], dkv[..., E:]
    for t in (o, dq, dk, dv):
        assert torch.isfinite(t.float()).all()
    refs = _ref(qkv, kv, go, o, 1, valid)
    _check_fwd(cd, o, lse, refs, Lq, N, 1)
    _check_bwd(cd, qkv, kv, dq, dk, dv, refs, 1)
    assert bool((dk.float().permute(1, 0, 2)[~valid] == 0).all())
    assert bool((dv.float().permute(1, 0, 2)[~valid] == 0).all())


# ------------------------------------------------------------------ softmax range form
def test_softmax_range_form():
    rows_per_seq, nseq, n = 40, 2, 50
    rows, lds, ldp = nseq * rows_per_seq, n + 3, 64
    ranges = [(7, 50), (0, 33)]
    g = torch.Generator().manual_seed(3)
    s = torch.randn(rows, n, generator=g) * 4
    scale = R.SM_SCALE
    sb = torch.full((rows, lds), NAN, device=DEV)
    sb[:, :n] = s.to(DEV)
    p = torch.full((rows + 1, ldp), NAN, device=DEV)
    ops.softmax_fwd(sb, lds, rows, n, scale, p, ldp, kr=_table(ranges), rows_per_seq=rows_per_seq)
    torch.cuda.synchronize()
    assert torch.isnan(p[rows]).all(), "guard row written"
    for q, (b, e) in enumerate(ranges):
        rs = slice(q * rows_per_seq, (q + 1) * rows_per_seq)
        f = R.softmax_fwd(s[rs, b:e].to(torch.float64), scale)
        R.check(p[rs, b:e], f.p, f.c_p, torch.float32, R.K_SOFTMAX, f"p seq {q}")
        assert bool((p[rs, :b] == 0).all()) and bool((p[rs, e:] == 0).all()), "masked not zero"


# ------------------------------------------------------------------ mask -> ranges
def _mask(rows, Lk):
    m = torch.ones(len(rows), Lk, dtype=torch.bool)
    for i, spans in enumerate(rows):
        for b, e in spans:
            m[i, b:e] = False
    return m.to(DEV)


def test_kpm_ranges_table_and_bad_rows():
    Lk = 70
    ok = [[(12, 70)], [(0, 55)], [(3, 64)], [(0, 70)], [(69, 70)], [(0, 1)]]
    kr = JF.key_ranges(_mask(ok, Lk))
    assert kr.B == len(ok) and kr.Lk == Lk
    assert kr.table.cpu().tolist() == [v for spans in ok for v in spans[0]]
    # a strided mask (row stride > Lk) and a uint8 one
    wide = torch.ones(len(ok), 2 * Lk, dtype=torch.bool, device=DEV)
    wide[:, :Lk] = _mask(ok, Lk)
    assert torch.equal(JF.key_ranges(wide[:, :Lk]).table, kr.table)
    assert torch.equal(JF.key_ranges(_mask(ok, Lk).to(torch.uint8)).table, kr.table)
    with pytest.raises(ValueError):                # a row of all True
        JF.key_ranges(_mask([[(0, 70)], []], Lk))
    JF.check_key_ranges()                          # the counter was cleared by the raise
    with pytest.raises(ValueError):                # a hole
        JF.key_ranges(_mask([[(0, 10), (20, 70)]], Lk))
    JF.check_key_ranges()
    with pytest.raises(NotImplementedError):       # float masks
        JF.key_ranges(torch.zeros(2, Lk, device=DEV))
    assert JF.key_ranges(kr) is kr


# ------------------------------------------------------------------ dispatch
def _op(aligned=True, stride=1536):
    return JF.AttnOperand(aligned, stride)


def test_plan_with_ranges():
    bf, f32 = torch.bfloat16, torch.float32
    a = _op()
    g = (a,) * 4
    p = JF.attn_plan(bf, 3, 1, 16, 16, E, a, a, a, a, *g, kr=True)
    assert (p.fwd, p.bwd) == ("short", "short")
    p = JF.attn_plan(bf, 3, 1, 6, 6, E, a, a, a, a, *g, kr=True)      # not "small"
    assert (p.fwd, p.bwd) == ("short", "short")
    p = JF.attn_plan(bf, 3, 1, 70, 70, E, a, a, a, a, *g, kr=True)
    assert (p.fwd, p.rows, p.bwd) == ("fused", True, "pds_dkdv")
    p = JF.attn_plan(bf, 3, 1, 40, 50, E, a, a, a, a, *g, kr=True)    # no whole-row forward
    assert (p.fwd, p.bwd) == ("gemm", "gemm")
    p = JF.attn_plan(f32, 3, 1, 70, 70, E, a, a, a, a, *g, kr=True)
    assert (p.fwd, p.bwd) == ("gemm", "gemm")
    # without ranges the answers are the old ones
    assert JF.attn_plan(bf, 3, 1, 40, 50, E, a, a, a, a).fwd == "fused"
    assert JF.attn_plan(bf, 3, 1, 6, 6, E, a, a, a, a).fwd == "small"


def test_ranged_call_on_the_gemm_path_matches_reference():
    """A 16-bit (40, 50) call with ranges: no whole-row forward (Lq <= 64), so GEMM + the range
    softmax; it must not run unmasked."""
    cd, Lq, Lk, N = torch.bfloat16, 40, 50, 4
    ranges = [(0, 50), (13, 50), (0, 31), (20, 21)]
    mask = ~_valid(ranges, N, Lk)
    qkv, kv, go = _inputs(cd, Lq, Lk, N, seed=61)
    fams = []
    ops.set_launch_hook(lambda info, launch: (fams.append(info.get("family")), launch())[1])
    try:
        with JF.compute_mode(cd):
            kr = JF.key_ranges(mask)
            o, saved = JF.attn_forward(qkv, kv, kv, E, 1, 0, 0, E, kr=kr)
    finally:
        ops.set_launch_hook(None)
    torch.cuda.synchronize()
    assert saved[1].fwd == "gemm" and "attn_fwd" not in fams
    r = _ref(qkv, kv, None, None, 1, ~mask)[0]
    tol = 1e-2 * max(r["o"].abs().max().item(), 1.0)
    assert (o.float() - r["o"]).abs().max().item() <= tol
    # ranges of another mask shape are refused, not ignored
    with pytest.raises(ValueError), JF.compute_mode(cd):
        JF.attn_forward(qkv, kv, kv, E, 1, 0, 0, E, kr=JF.key_ranges(mask[:, :40]))
    with pytest.raises(JMTError):                  # the 64-row forward takes no table
        o2 = torch.empty(Lq, N, E, device=DEV, dtype=cd)
        ops.attn_fwd(ops.dt(qkv), N, 1, Lq, Lk, E, qkv.data_ptr(), _st(qkv), kv.data_ptr(),
                     _st(kv), kv[..., E:].data_ptr(), _st(kv), o2.data_ptr(), _st(o2), SCALE,
                     torch.empty(N * Lq, device=DEV), kr=_table(ranges))
