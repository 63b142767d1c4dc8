"""functional.attn_plan against what attn_forward / attn_backward launch: for one geometry per
path the launches recorded under ops.set_launch_hook are the families of the path the plan named
(the plan evaluated here from the same layouts, the expected path names as literals)."""
import pytest
import torch

from jmt import functional as JF
from jmt import ops
from jmt.functional import AttnOperand as Op

pytestmark = pytest.mark.gpu
DEV = "cuda"
E, H = 512, 1

# launches of each path, in order (the softmax kernels of the GEMM path are not hooked)
FWD_LAUNCHES = {"small": ["small_attn_fwd"], "short": ["attn_short_fwd"], "fused": ["attn_fwd"],
                "gemm": ["gemm_NT", "gemm_NN"]}
BWD_LAUNCHES = {"small": ["small_attn_bwd"], "short": ["attn_short_bwd"],
                "pds_dkdv": ["attn_bwd", "attn_dkdv"], "bwd64_dkdv": ["attn_bwd", "attn_dkdv"],
                "bwd64_gemm": ["attn_bwd", "gemm_TN", "gemm_TN"],
                "gemm": ["gemm_NT", "gemm_NN", "gemm_TN", "gemm_TN"]}
# products of the attn_dkdv launch: dK, dV and, behind the P / dS kernel, dQ
DKDV_PRODUCTS = {"pds_dkdv": 3, "bwd64_dkdv": 2}

CASES = [
    # id, (Lq, Lk, N), dtype, dQ offset (elements), _attn_dkdv, (forward, whole rows, backward)
    ("small", (6, 6, 3), torch.bfloat16, 0, True, ("small", False, "small")),
    ("short", (20, 32, 2), torch.bfloat16, 0, True, ("short", False, "short")),
    ("fused64", (64, 64, 1), torch.bfloat16, 0, True, ("fused", False, "pds_dkdv")),
    ("rows", (65, 33, 2), torch.bfloat16, 0, True, ("fused", True, "pds_dkdv")),
    ("dq_offset", (65, 33, 2), torch.bfloat16, 4, True, ("fused", True, "bwd64_dkdv")),
    ("dkdv_off", (65, 33, 2), torch.bfloat16, 0, False, ("fused", True, "bwd64_gemm")),
    ("fp32", (65, 33, 2), torch.float32, 0, True, ("gemm", False, "gemm")),
]


def _record(rec):
    ops.set_launch_hook(lambda info, launch: (rec.append(dict(info)), launch())[1])


@pytest.mark.parametrize("name,shape,cd,dq_off,dkdv,want", CASES, ids=[c[0] for c in CASES])
def test_launches_follow_attn_plan(name, shape, cd, dq_off, dkdv, want):
    """dq_offset: a dQ buffer 8 B off a 16-B boundary leaves the P / dS + dQ pair of kernels; the
    64-row backward writes dQ through an aligned temporary that attn_backward copies back."""
    Lq, Lk, N = shape
    g = torch.Generator(device=DEV).manual_seed(71)
    qkv = torch.randn(N, Lq, 3 * E, device=DEV, generator=g).to(cd).permute(1, 0, 2)
    kv = torch.randn(N, Lk, 2 * E, device=DEV, generator=g).to(cd).permute(1, 0, 2)
    go = torch.randn(Lq, N, E, device=DEV, generator=g).to(cd)
    # dQ in the q columns of a packed buffer that starts dq_off elements into its allocation
    dq = torch.zeros(N * Lq * 3 * E + dq_off, device=DEV, dtype=cd)[dq_off:].view(
        N, Lq, 3 * E).permute(1, 0, 2)
    dkv = torch.zeros(N, Lk, 2 * E, device=DEV, dtype=cd).permute(1, 0, 2)
    rec_f, rec_b = [], []
    ops._attn_dkdv["on"] = dkdv
    JF.set_compute_dtype(cd)
    try:
        ops_ = [JF._operand(qkv, 0, cd), JF._operand(kv, 0, cd), JF._operand(kv, E, cd),
                Op(True, E), JF._operand(go, 0, cd), JF._operand(dq, 0, cd),
                JF._operand(dkv, 0, cd), JF._operand(dkv, E, cd)]
        plan = JF.attn_plan(cd, N, H, Lq, Lk, E, *ops_)
        _record(rec_f)
        o, saved = JF.attn_forward(qkv, kv, kv, E, H, 0, 0, E)
        _record(rec_b)
        JF.attn_backward(saved, go, dq, dkv, dkv)
        torch.cuda.synchronize()
    finally:
        ops.set_launch_hook(None)
        JF.set_compute_dtype(None)
        ops._attn_dkdv["on"] = True
    assert (plan.fwd, plan.rows, plan.bwd) == want
    assert saved[1].fwd == plan.fwd
    assert [r["family"] for r in rec_f] == FWD_LAUNCHES[plan.fwd]
    assert [r["family"] for r in rec_b] == BWD_LAUNCHES[plan.bwd]
    assert not any(r.get("shared_q") for r in rec_f + rec_b)
    if plan.bwd in DKDV_PRODUCTS:
        assert rec_b[1]["flops"] == 2.0 * DKDV_PRODUCTS[plan.bwd] * N * H * Lq * Lk * E
    for t in (o, dq[..., :E], dkv):
        assert torch.isfinite(t.float()).all()
    assert dq[..., :E].float().abs().max().item() > 0 and dkv.float().abs().max().item() > 0
    if dq_off:
        # the same kernels on an aligned dQ buffer (JMT_ATTN_PDS=0): bitwise the same gradients
        dq2, dkv2 = torch.zeros_like(qkv), torch.zeros_like(dkv)
        ops._attn_pds["on"] = False
        try:
            JF.attn_backward(saved, go, dq2, dkv2, dkv2)
            torch.cuda.synchronize()
        finally:
            ops._attn_pds["on"] = True
        assert torch.equal(dq, dq2) and torch.equal(dkv, dkv2)


def test_cross_attention6_takes_the_shared_query_launches():
    """grouped.cross_attention6 at B = 1, T = 65: the plan of its layouts (QKV and dQKV packed
    (6, T, 3E), dO batch-major) admits shared queries, and its attention launches are the
    *_sq ones of that path."""
    from jmt import grouped
    from jmt.grouped import CROSS_PAIRS
    cd = torch.bfloat16
    B, T = 1, 65
    g = torch.Generator(device="cpu").manual_seed(72)
    mods = []
    for _ in range(1 + max(m for m, _, _ in CROSS_PAIRS)):
        m = torch.nn.MultiheadAttention(E, H)
        with torch.no_grad():
            m.in_proj_weight.copy_(torch.randn(3 * E, E, generator=g) * E ** -0.5)
            m.out_proj.weight.copy_(torch.randn(E, E, generator=g) * E ** -0.5)
        mods.append(m.to(DEV))
    Y = torch.randn(3, B, T, E, generator=g).to(DEV, cd).requires_grad_(True)
    dO6 = torch.randn(len(CROSS_PAIRS), B, T, E, generator=g).to(DEV, cd)
    q, od = Op(True, 3 * E), Op(True, E)
    rec = []
    _record(rec)
    try:
        with JF.compute_mode(cd):
            plan = JF.attn_plan(cd, len(CROSS_PAIRS) * B, H, T, T, E, q, q, q, od, od, q, q, q)
            O6 = grouped.cross_attention6(Y, mods, H, CROSS_PAIRS)
            O6.backward(dO6)
        torch.cuda.synchronize()
    finally:
        ops.set_launch_hook(None)
    assert plan == JF.AttnPlan("fused", True, "pds_dkdv", True)
    attn = [r for r in rec if r["family"].startswith("attn")]
    assert [r["family"] for r in attn] == FWD_LAUNCHES[plan.fwd] + BWD_LAUNCHES[plan.bwd]
    assert all(r.get("shared_q") for r in attn)
    assert torch.isfinite(O6.float()).all() and torch.isfinite(Y.grad.float()).all()
