"""Attention dropout: the counter-based mask inside the fused multi-head
kernels (csrc/attn_mh.hip, DROP = true), on the GEMM + softmax path (jmt_attn_dropout) and through
jmt.nn.MultiheadAttention, a captured graph and Two_transformers.

The mask every check expects is the library's host reference (jmt_attn_dropout_reference), which
tests/test_attn_dropout_ref.py ties to the numpy restatement of the specification on the CPU."""
import math

import pytest
import torch

from jmt import functional as JF
from jmt import grouped, ops
from jmt import nn as jnn
from oracle.hashinit import init_module_
from tests import attn_drop_ref as A
from tests import attn_mh_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
E = 512
SEED = 0x1234_5678_9ABC_DEF0
CDS = [torch.bfloat16, torch.float16]


def _ctr(call, stream=0):
    return (SEED & 0xFFFFFFFF, SEED >> 32, call, stream)


# ---------------------------------------------------------------- 1. the mask, read out exactly

@pytest.mark.parametrize("cd", CDS, ids=["bf16", "fp16"])
@pytest.mark.parametrize("p", [0.25, 0.1], ids=str)
def test_mask_read_out(cd, p):
    """V_j = one-hot rows for keys [64 j, 64 j + 64): O[l, h dh + d] = s P[l, 64 j + d] where
    the key is kept and exactly 0 where it is dropped.  q is scaled by 1/4, so every probability
    is within e^{+-3} of 1 / Lk and non-zero in either type."""
    Lq, Lk, N, H = 70, 130, 3, 8
    dh = E // H
    qkv, kv, _ = R.inputs(cd, Lq, Lk, N, seed=43)
    qkv = (qkv.float() * torch.cat([torch.full((E,), 0.25), torch.ones(2 * E)]).to(DEV)).to(cd)
    ctr = _ctr(5, 1)
    keep = torch.from_numpy(ops.attn_dropout_reference(ctr, N * H, Lq, Lk, p) != 0).to(DEV)
    keep = keep.reshape(N, H, Lq, Lk)
    assert 0 < keep.float().mean().item() < 1
    ranges = [(3, 101), (64, 130), (3, 101)]
    for kr, valid in ((None, R.valid_keys(Lk, N)),
                      (R.kr_op(ranges, 3), R.valid_keys(Lk, N, ranges))):
        want = keep & valid[:, None, None, :]
        for j in range(3):
            v = torch.zeros(Lk, N, H, dh, device=DEV, dtype=cd)
            ks = torch.arange(64 * j, min(64 * j + 64, Lk), device=DEV)
            v[ks, :, :, ks - 64 * j] = 1.0
            o, _ = A.fwd(qkv, kv, H, (p, A.ctr_tensor(ctr)), kr=kr, v=v.reshape(Lk, N, E))
            torch.cuda.synchronize()
            got = (o.reshape(Lq, N, H, dh) != 0).permute(1, 2, 0, 3)       # (N, H, Lq, d)
            exp = torch.zeros_like(got)
            exp[..., :len(ks)] = want[..., 64 * j:64 * j + len(ks)]
            assert torch.equal(got, exp), (kr is not None, j, (got != exp).sum().item())


# ---------------------------------------------------------------- 2. against float64

SHAPES = [(1, 1, 1, 8), (9, 17, 5, 8), (33, 31, 3, 8), (65, 129, 2, 8), (129, 65, 3, 4),
          (70, 70, 40, 8)]
RANGES = [(5, 97), (64, 129)]
_inputs = {}


def _in(cd, shape):
    """Inputs and the p = 0 forward of one (dtype, shape): computed once, left unchanged."""
    key = (cd, shape)
    if key not in _inputs:
        Lq, Lk, N, H = shape
        qkv, kv, go = R.inputs(cd, Lq, Lk, N)
        _inputs[key] = (qkv, kv, go, R.fwd(qkv, kv, H)[1],
                        R.fwd(qkv, kv, H, kr=R.kr_op(RANGES, 2))[1] if N % 2 == 0 else None)
    return _inputs[key]


def _vs_float64(cd, shape, p, ranges):
    Lq, Lk, N, H = shape
    qkv, kv, go, lse0, lse0_kr = _in(cd, shape)
    ctr = _ctr(17, 2)
    drop = (p, A.ctr_tensor(ctr))
    kr = None if ranges is None else R.kr_op(ranges, len(ranges))
    o, lse = A.fwd(qkv, kv, H, drop, kr=kr)
    dq, dk, dv, delta = A.bwd(qkv, kv, go, o, lse, H, drop, kr=kr)
    # the softmax is normalised before the mask: lse is the p = 0 one, bit for bit
    assert torch.equal(lse, lse0 if ranges is None else lse0_kr)
    M = A.lib_mask(ctr, N, H, Lq, Lk, p)
    ref = A.ref64_drop(qkv, kv, go, H, M, o=o, ranges=ranges)
    got = dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv)
    A.check_bounds(cd, qkv, kv, got, ref, H, A.scale(p), what=f"{shape} p={p}")
    # delta = rowsum(dO o O) of the masked 16-bit O
    d = ref["delta"]
    assert (delta.double() - d).abs().max().item() <= 1e-5 * max(d.abs().max().item(), 1.0)


@pytest.mark.parametrize("cd", CDS, ids=["bf16", "fp16"])
@pytest.mark.parametrize("p", [0.1, 0.5], ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_drop_vs_float64(cd, shape, p):
    _vs_float64(cd, shape, p, None)


@pytest.mark.parametrize("cd", CDS, ids=["bf16", "fp16"])
@pytest.mark.parametrize("p", [0.1, 0.5], ids=str)
def test_drop_vs_float64_key_ranges(cd, p):
    _vs_float64(cd, (65, 129, 2, 8), p, RANGES)


# ---------------------------------------------------------------- 3. state

def test_backward_regenerates_its_own_forwards_mask():
    cd, (Lq, Lk, N, H), p = torch.bfloat16, (33, 31, 3, 8), 0.5
    qkv, kv, go = R.inputs(cd, Lq, Lk, N, seed=47)
    JF.set_dropout_state(SEED, call=30, stream=0)
    st = JF._drop_block(DEV)
    c1, c2 = ops.dropout_next(st), ops.dropout_next(st)
    assert c1.tolist()[2] == 30 and c2.tolist()[2] == 31 and JF.dropout_state()["call"] == 32
    o1, lse1 = A.fwd(qkv, kv, H, (p, c1))
    o2, _ = A.fwd(qkv, kv, H, (p, c2))
    assert not torch.equal(o1, o2)
    dq, dk, dv, _ = A.bwd(qkv, kv, go, o1, lse1, H, (p, c1))
    M = A.lib_mask(_ctr(30), N, H, Lq, Lk, p)
    ref = A.ref64_drop(qkv, kv, go, H, M, o=o1)
    A.check_bounds(cd, qkv, kv, dict(dq=dq, dk=dk, dv=dv), ref, H, A.scale(p), what="first call")
    again = A.bwd(qkv, kv, go, o1, lse1, H, (p, c1))
    for a, b in zip((dq, dk, dv), again):
        assert torch.equal(a, b)


def test_dropped_keys_get_exactly_zero_dv():
    cd, (Lq, Lk, N, H), p = torch.bfloat16, (1, 130, 2, 8), 0.5
    dh = E // H
    qkv, kv, go = R.inputs(cd, Lq, Lk, N, seed=53)
    ctr = _ctr(3)
    drop = (p, A.ctr_tensor(ctr))
    o, lse = A.fwd(qkv, kv, H, drop)
    _, _, dv, _ = A.bwd(qkv, kv, go, o, lse, H, drop)
    keep = torch.from_numpy(ops.attn_dropout_reference(ctr, N * H, Lq, Lk, p) != 0).to(DEV)
    keep = keep.reshape(N, H, Lk).permute(2, 0, 1)                    # (Lk, N, H): one query row
    dvh = dv.reshape(Lk, N, H, dh)
    assert (dvh[~keep] == 0).all()
    assert (dvh[keep] != 0).any(-1).all()


# ---------------------------------------------------------------- 4. p = 0 and eval

def _module_run(m, x, cd, w):
    fams = []
    for q in m.parameters():
        q.grad = None
    xd = x.clone().requires_grad_(True)
    ops.set_launch_hook(lambda info, launch: (fams.append(info["family"]), launch())[1])
    try:
        with JF.compute_mode(cd):
            out, _ = m(xd, xd, xd)
            (w * out.float()).mean().backward()
        torch.cuda.synchronize()
    finally:
        ops.set_launch_hook(None)
    return out.detach(), xd.grad, {k: q.grad.clone() for k, q in m.named_parameters()}, fams


def _mha(H, dropout):
    m = jnn.MultiheadAttention(E, H, dropout=dropout)
    init_module_(m, "")
    return m.to(DEV)


def test_rate_zero_and_eval_are_the_plain_kernels():
    cd, (Lq, Lk, N, H) = torch.bfloat16, (65, 129, 2, 8)
    qkv, kv, go = R.inputs(cd, Lq, Lk, N)
    o0, lse0 = R.fwd(qkv, kv, H)
    g0 = R.bwd(qkv, kv, go, o0, lse0, H)
    drop = (1.0 / 1024, A.ctr_tensor(_ctr(1)))                        # T8 = 0
    o, lse = A.fwd(qkv, kv, H, drop)
    g = A.bwd(qkv, kv, go, o, lse, H, drop)
    assert torch.equal(o, o0) and torch.equal(lse, lse0)
    for a, b in zip(g, g0):
        assert torch.equal(a, b)
    # the module in eval(), and at a rate that rounds to 0
    gen = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn(37, 2, E, device=DEV, generator=gen)
    w = torch.rand(37, 2, E, device=DEV, generator=gen) + 0.5
    plain = _module_run(_mha(8, 0.0), x, cd, w)
    JF.set_dropout_state(SEED, call=40, stream=0)
    for m in (_mha(8, 0.3).eval(), _mha(8, 1.0 / 1024)):
        got = _module_run(m, x, cd, w)
        assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
        for k in plain[2]:
            assert torch.equal(got[2][k], plain[2][k]), k
        assert got[3] == plain[3]
    assert JF.dropout_state()["call"] == 40
    assert [f for f in plain[3] if f.startswith("attn")] == ["attn_mh_fwd", "attn_mh_bwd"]


# ---------------------------------------------------------------- 5. the GEMM + softmax path

@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16],
                         ids=["f32", "bf16", "f16"])
def test_mask_kernel_matches_reference(dt):
    NH, Lq, Lk, ld, p = 5, 9, 130, 136, 0.25
    ctr = _ctr(11, 4)
    gen = torch.Generator(device=DEV).manual_seed(9)
    x = (torch.randn(NH * Lq, ld, device=DEV, generator=gen) + 3.0).to(dt)
    m = torch.from_numpy(ops.attn_dropout_reference(ctr, NH, Lq, Lk, p)).to(DEV).reshape(-1, Lk)
    want = (x[:, :Lk].float() * m).to(dt)            # one product in fp32, rounded once
    y = torch.full_like(x, float("nan"))
    ops.attn_dropout(x, ld, y, ld, NH, Lq, Lk, p, A.ctr_tensor(ctr))
    torch.cuda.synchronize()
    assert torch.equal(y[:, :Lk], want) and (y[:, Lk:] == 0).all()
    # another stride out of place, then in place (padding columns stay)
    y2 = torch.full((NH * Lq, 132), float("nan"), device=DEV, dtype=dt)
    ops.attn_dropout(x, ld, y2, 132, NH, Lq, Lk, p, A.ctr_tensor(ctr))
    z = x.clone()
    ops.attn_dropout(z, ld, z, ld, NH, Lq, Lk, p, A.ctr_tensor(ctr))
    torch.cuda.synchronize()
    assert torch.equal(y2[:, :Lk], want) and (y2[:, Lk:] == 0).all()
    assert torch.equal(z[:, :Lk], want) and torch.equal(z[:, Lk:], x[:, Lk:])


def _mha64(m, x, M, w):
    """nn.MultiheadAttention self-attention in float64 with the multipliers M (N, H, L, L)
    injected: in-projection, softmax, mask, P V, out-projection; output, input gradient and
    parameter gradients of mean(w o out)."""
    H, dh = m.num_heads, E // m.num_heads
    prm = {k: q.detach().double().requires_grad_(True) for k, q in m.named_parameters()}
    xd = x.double().requires_grad_(True)
    L, N = x.shape[:2]
    qkv = xd @ prm["in_proj_weight"].t() + prm["in_proj_bias"]
    q, k, v = (t.reshape(L, N, H, dh) for t in qkv.split(E, -1))
    s = torch.einsum("lnhd,knhd->nhlk", q, k) / math.sqrt(dh)
    pm = torch.softmax(s, -1) * M
    o = torch.einsum("nhlk,knhd->lnhd", pm, v).reshape(L, N, E)
    out = o @ prm["out_proj.weight"].t() + prm["out_proj.bias"]
    (w.double() * out).mean().backward()
    return out.detach(), xd.grad, {k: t.grad for k, t in prm.items()}


@pytest.mark.parametrize("H", [1, 2], ids=["H1", "H2"])
def test_gemm_path_module_fp32(H):
    """num_heads 1 and 2 (head dims 512 and 256: no fused multi-head kernel) in fp32 compute:
    plan "gemm"; the project's fp32 tolerances: 1e-4 of the largest value on
    outputs, 1e-3 on gradients."""
    T, B, p = 37, 2, 0.25
    m = _mha(H, p)
    gen = torch.Generator(device=DEV).manual_seed(13)
    x = torch.randn(T, B, E, device=DEV, generator=gen)
    w = torch.rand(T, B, E, device=DEV, generator=gen) + 0.5
    JF.set_dropout_state(SEED, call=50, stream=1)
    out, dx, grads, fams = _module_run(m, x, torch.float32, w)
    assert JF.dropout_state()["call"] == 51
    assert fams.count("attn_dropout") == 3 and not any(f.startswith("attn_mh") for f in fams)
    M = A.lib_mask(_ctr(50, 1), B, H, T, T, p)
    rout, rdx, rgrads = _mha64(m, x, M, w)
    rel = lambda a, b: (a.double() - b).abs().max().item() / b.abs().max().item()
    assert rel(out, rout) <= 1e-4
    assert rel(dx, rdx) <= 1e-3
    for k in rgrads:
        assert rel(grads[k], rgrads[k]) <= 1e-3, k


# ---------------------------------------------------------------- 6. module and graph

def test_module_bf16_vs_float64():
    """MultiheadAttention(512, 8, dropout = 0.25) in bf16 at (37, 2) on the fused kernels against
    the float64 module with the call's mask.  The output bound is test 2's bound on o carried
    through the out-projection: |dy_i| <= sum_j |W_ij| |do_j| <= max_i sum_j |W_ij| tol_o, plus
    the 16-bit operands of the two projections (x, W rounded to bf16: 3 roundings of relative
    2^-9 on a sum of 512 products, taken at their absolute sums) and one rounding of y."""
    T, B, H, p, cd = 37, 2, 8, 0.25, torch.bfloat16
    m = _mha(H, p)
    gen = torch.Generator(device=DEV).manual_seed(17)
    x = torch.randn(T, B, E, device=DEV, generator=gen)
    w = torch.rand(T, B, E, device=DEV, generator=gen) + 0.5
    JF.set_dropout_state(SEED, call=60, stream=0)
    out, dx, grads, fams = _module_run(m, x, cd, w)
    assert JF.dropout_state()["call"] == 61
    assert [f for f in fams if f.startswith("attn")] == ["attn_mh_fwd", "attn_mh_bwd"]
    M = A.lib_mask(_ctr(60), B, H, T, T, p)
    rout, rdx, rgrads = _mha64(m, x, M, w)
    u = 2.0 ** -9
    Wo = m.out_proj.weight.detach().double()
    rowsum = Wo.abs().sum(1).max().item()
    tol_o = float(A.scale(p)) * 1e-2 * 1.0         # |o| <= max|v| ~ 1: the floor of the form
    err = (out.double() - rout).abs().max().item()
    tol = rowsum * (tol_o + 3 * u * 4.0) + 2 * u * rout.abs().max().item()
    print(f"module out err {err:.3e} tol {tol:.3e}")
    assert err <= tol
    # gradients: finite, and close in the aggregate (their exact bounds are test 2's, at the
    # kernel level); 5 % of the largest value
    for k, r in dict(rgrads, input=rdx).items():
        g = dx if k == "input" else grads[k]
        assert torch.isfinite(g).all()
        e = (g.double() - r).abs().max().item()
        print(f"module grad {k} err {e:.3e} max {r.abs().max().item():.3e}")
        assert e <= 5e-2 * r.abs().max().item(), k


def test_graph_replays_draw_new_masks_and_state_resumes():
    cd, H, p = torch.bfloat16, 8, 0.25
    qkv, kv, go = R.inputs(cd, 65, 33, 2, seed=73)

    def run():
        dqkv = torch.zeros(2, 65, 3 * E, device=DEV, dtype=cd).permute(1, 0, 2)
        dkv = torch.zeros(2, 33, 2 * E, device=DEV, dtype=cd).permute(1, 0, 2)
        with JF.compute_mode(cd):
            o, saved = JF.attn_forward(qkv, kv, kv, E, H, 0, 0, E, drop_p=p)
            assert saved[1].fwd == "mh" and saved[1].drop is not None
            JF.attn_backward(saved, go, dqkv, dkv, dkv)
        return o, dqkv, dkv

    JF.set_dropout_state(SEED, call=70, stream=0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()

    def replay():
        graph.replay()
        torch.cuda.synchronize()
        return [t.clone() for t in outs]

    JF.set_dropout_state(SEED, call=80, stream=0)
    first, second = replay(), replay()
    assert JF.dropout_state()["call"] == 82
    assert not torch.equal(first[0], second[0]) and not torch.equal(first[2], second[2])
    JF.set_dropout_state(SEED, call=80, stream=0)
    again = replay()
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    # and the replay is the eager call of the same state
    JF.set_dropout_state(SEED, call=80, stream=0)
    eager = run()
    torch.cuda.synchronize()
    for a, b in zip(first, eager):
        assert torch.equal(a, b)


# ---------------------------------------------------------------- 7. model plumbing

def _model(num_heads):
    from models.two_transformers import Two_transformers
    m = Two_transformers(0.0, 0.0, num_heads, 1, "TRANSFORMER", "FC", 2048)
    init_module_(m, "")
    return m.to(DEV)


def _model_run(m, audio, video, w, rec=None):
    for q in m.parameters():
        q.grad = None
    if rec is not None:
        ops.set_launch_hook(lambda info, launch: (rec.append(dict(info)), launch())[1])
    try:
        with JF.compute_mode(torch.bfloat16):
            vo, ao = m(audio, video)
            if m.training:
                ((w[0].reshape(vo.shape) * vo).mean() +
                 (w[1].reshape(ao.shape) * ao).mean()).backward()
        torch.cuda.synchronize()
    finally:
        ops.set_launch_hook(None)
    grads = {k: q.grad.clone() for k, q in m.named_parameters() if q.grad is not None}
    return torch.stack([vo.detach().float(), ao.detach().float()]), grads


def _model_inputs(B=2, T=37):
    gen = torch.Generator(device=DEV).manual_seed(5)
    audio = torch.randn(B, T, E, device=DEV, generator=gen)
    video = torch.randn(B, T, 2048, device=DEV, generator=gen)
    w = torch.rand(2, B * T, device=DEV, generator=gen) + 0.5
    return audio, video, w


def test_model_h8_dropout():
    p = 0.25
    audio, video, w = _model_inputs()
    m = _model(8)
    out0_eval, _ = _model_run(m.eval(), audio, video, w)
    out0, g0 = _model_run(m.train(), audio, video, w)
    assert jnn.set_attention_dropout(m, p) is m
    assert all(a.dropout == p for a in m.modules() if isinstance(a, jnn.MultiheadAttention))
    # (a) eval: the p = 0 model
    JF.set_dropout_state(SEED, call=100, stream=0)
    out_eval, _ = _model_run(m.eval(), audio, video, w)
    assert torch.equal(out_eval, out0_eval) and JF.dropout_state()["call"] == 100
    # (b) training: every attention on the fused kernels, one call per launch
    rec = []
    out, g = _model_run(m.train(), audio, video, w, rec)
    fams = [r["family"] for r in rec]
    attn = [f for f in fams if f.startswith(("attn", "small_attn"))]
    n_fwd = attn.count("attn_mh_fwd")
    assert n_fwd >= 2 and attn.count("attn_mh_bwd") == n_fwd and len(attn) == 2 * n_fwd, attn
    assert not [r for r in rec if r["family"].startswith("gemm") and r.get("batch", 1) >= 8 and
                64 in (r["N"], r["K"])]
    assert JF.dropout_state()["call"] == 100 + n_fwd
    assert not torch.equal(out, out0)
    # (c) the same masks on the GEMM + softmax path: the difference of the two paths may be at
    # most 4 s times their difference at p = 0 (both the parent's code), plus one bf16 ulp of the
    # quantity's largest value
    def gemm_run(mm):
        ops._attn_mh["on"] = False
        try:
            return _model_run(mm, audio, video, w)
        finally:
            ops._attn_mh["on"] = True
    JF.set_dropout_state(SEED, call=100, stream=0)
    out_g, g_g = gemm_run(m)
    assert JF.dropout_state()["call"] == 100 + n_fwd
    jnn.set_attention_dropout(m, 0.0)
    out0_g, g0_g = gemm_run(m)
    s = float(A.scale(p))
    worst = 0.0
    for k in ["outputs"] + sorted(g):
        a, b, a0, b0 = ((out, out_g, out0, out0_g) if k == "outputs" else
                        (g[k], g_g[k], g0[k], g0_g[k]))
        d0 = (a0.double() - b0.double()).abs().max().item()
        d = (a.double() - b.double()).abs().max().item()
        ulp = 2.0 ** -8 * max(a.abs().max().item(), b.abs().max().item())
        ratio = d / max(4 * s * d0 + ulp, 1e-300)
        worst = max(worst, ratio)
        print(f"{k}: d0 {d0:.3e} d {d:.3e} bound {4 * s * d0 + ulp:.3e} ratio {ratio:.3f}")
        assert d <= 4 * s * d0 + ulp, (k, d, d0)
    print(f"largest d / bound: {worst:.3f}")


def test_model_h1_dropout_trains_on_the_gemm_path():
    audio, video, w = _model_inputs()
    m = _model(1)
    out0_eval, _ = _model_run(m.eval(), audio, video, w)
    out0, _ = _model_run(m.train(), audio, video, w)
    jnn.set_attention_dropout(m, 0.25)
    JF.set_dropout_state(SEED, call=0, stream=0)
    rec = []
    out, g = _model_run(m.train(), audio, video, w, rec)
    fams = [r["family"] for r in rec]
    n = JF.dropout_state()["call"]
    assert n >= 2 and fams.count("attn_dropout") == 3 * n
    assert not [f for f in fams if f.startswith(("attn_", "small_attn")) and f != "attn_dropout"]
    assert torch.isfinite(out).all() and not torch.equal(out, out0)
    assert len(g) > 20 and all(torch.isfinite(t).all() for t in g.values())
    out_eval, _ = _model_run(m.eval(), audio, video, w)
    assert torch.equal(out_eval, out0_eval)


def test_grouped_modules_must_agree():
    m = _model(8)
    jnn.set_attention_dropout(m, 0.25)
    att = [a for a in m.modules() if isinstance(a, jnn.MultiheadAttention)]
    att[0].dropout = 0.5
    audio, video, w = _model_inputs()
    grouped.set_enabled(True)
    with pytest.raises(ValueError, match="disagree"):
        _model_run(m.train(), audio, video, w)


def test_plan_with_dropout():
    Op = JF.AttnOperand
    bf, f32 = torch.bfloat16, torch.float32
    q = Op(True, 1536)
    assert JF.attn_plan(bf, 3, 8, 6, 6, E, q, q, q, Op(True, E)).fwd == "small"
    assert JF.attn_plan(bf, 3, 8, 6, 6, E, q, q, q, Op(True, E), drop=True).fwd == "mh"
    assert JF.attn_plan(bf, 3, 1, 70, 70, E, q, q, q, Op(True, E)).fwd == "fused"
    assert JF.attn_plan(bf, 3, 1, 70, 70, E, q, q, q, Op(True, E), drop=True).fwd == "gemm"
    assert JF.attn_plan(bf, 3, 1, 16, 16, E, q, q, q, Op(True, E), drop=True).fwd == "gemm"
    assert JF.attn_plan(f32, 3, 8, 70, 70, E, q, q, q, Op(True, E), drop=True).fwd == "gemm"
    assert JF.attn_plan(bf, 3, 4, 70, 70, E, q, q, q, Op(True, E), kr=True, drop=True).fwd == "mh"
    with pytest.raises(JF.JMTError):
        jnn.MultiheadAttention(E, 8, dropout=1.0)
