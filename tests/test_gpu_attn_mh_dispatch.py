"""functional.attn_plan's "mh" answer through every layer: attn_forward / attn_backward,
jmt.nn.MultiheadAttention(512, 8), Two_transformers(num_heads=8) with and without a key padding
mask, grouped and ungrouped, and a captured graph.  With num_heads 8 or 4 every time-axis
attention used to run as batched GEMMs + softmax kernels with the probabilities kept in memory;
the first test here fails without the fused multi-head kernels."""
import pytest
import torch

from jmt import functional as JF
from jmt import grouped, ops
from jmt import nn as jnn
from oracle.hashinit import init_module_

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
E = 512
GEMM_FWD = ["gemm_NT", "gemm_NN"]
GEMM_BWD = ["gemm_NT", "gemm_NN", "gemm_TN", "gemm_TN"]


def _views(cd, Lq, Lk, N, seed=71):
    g = torch.Generator(device=DEV).manual_seed(seed)
    qkv = torch.randn(N, Lq, 3 * E, device=DEV, generator=g).to(cd).permute(1, 0, 2)
    kv = torch.randn(N, Lk, 2 * E, device=DEV, generator=g).to(cd).permute(1, 0, 2)
    go = torch.randn(Lq, N, E, device=DEV, generator=g).to(cd)
    return qkv, kv, go


def _fwd_bwd(cd, qkv, kv, go, H, qcol=0):
    """attn_forward + attn_backward under a launch hook: (families forward, families backward,
    saved meta, o, dqkv, dkv)."""
    Lq, N = qkv.shape[:2]
    Lk = kv.shape[0]
    dqkv = torch.zeros(N, Lq, qkv.shape[2], device=DEV, dtype=cd).permute(1, 0, 2)
    dkv = torch.zeros(N, Lk, 2 * E, device=DEV, dtype=cd).permute(1, 0, 2)
    rec_f, rec_b = [], []
    hook = lambda rec: ops.set_launch_hook(
        lambda info, launch: (rec.append(info["family"]), launch())[1])
    try:
        with JF.compute_mode(cd):
            hook(rec_f)
            o, saved = JF.attn_forward(qkv, kv, kv, E, H, qcol, 0, E)
            hook(rec_b)
            JF.attn_backward(saved, go, dqkv, dkv, dkv)
        torch.cuda.synchronize()
    finally:
        ops.set_launch_hook(None)
    return rec_f, rec_b, saved[1], o, dqkv, dkv


def test_h8_attention_runs_the_mh_kernels():
    cd = torch.bfloat16
    qkv, kv, go = _views(cd, 65, 33, 2)
    rec_f, rec_b, meta, o, dqkv, dkv = _fwd_bwd(cd, qkv, kv, go, 8)
    assert rec_f == ["attn_mh_fwd"] and rec_b == ["attn_mh_bwd"]
    assert meta.fwd == "mh"
    for t in (o, dqkv[..., :E], dkv):
        assert torch.isfinite(t.float()).all() and t.float().abs().max().item() > 0
    assert (dqkv[..., E:] == 0).all()            # the other columns of the packed buffer
    # H = 4 (head dim 128) as well
    rec_f, rec_b, meta, *_ = _fwd_bwd(cd, qkv, kv, go, 4)
    assert (rec_f, rec_b, meta.fwd) == (["attn_mh_fwd"], ["attn_mh_bwd"], "mh")


def test_switch_off_restores_the_gemm_path():
    cd = torch.bfloat16
    qkv, kv, go = _views(cd, 65, 33, 2)
    ops._attn_mh["on"] = False
    try:
        rec_f, rec_b, meta, *_ = _fwd_bwd(cd, qkv, kv, go, 8)
    finally:
        ops._attn_mh["on"] = True
    assert (rec_f, rec_b, meta.fwd) == (GEMM_FWD, GEMM_BWD, "gemm")


def test_every_other_answer_stays():
    bf = torch.bfloat16
    # fp32 stays on the GEMM path
    rec_f, rec_b, meta, *_ = _fwd_bwd(torch.float32, *_views(torch.float32, 65, 33, 2), 8)
    assert (rec_f, rec_b, meta.fwd) == (GEMM_FWD, GEMM_BWD, "gemm")
    # H = 1 stays on the head dim 512 kernels
    rec_f, rec_b, meta, *_ = _fwd_bwd(bf, *_views(bf, 65, 33, 2), 1)
    assert (rec_f, rec_b, meta.fwd) == (["attn_fwd"], ["attn_bwd", "attn_dkdv"], "fused")
    # L <= 8 stays on the one-wave kernels
    rec_f, rec_b, meta, *_ = _fwd_bwd(bf, *_views(bf, 6, 6, 3), 8)
    assert (rec_f, rec_b, meta.fwd) == (["small_attn_fwd"], ["small_attn_bwd"], "small")
    # a q view 8 B off a 16-B boundary keeps the plan's "gemm" answer (asked of the plan with the
    # view's own operand: the GEMMs themselves want 16-B aligned operands)
    qkv, kv, go = _views(bf, 65, 33, 2)
    wide = torch.randn(2, 65, 3 * E + 8, device=DEV).to(bf).permute(1, 0, 2)
    opn = lambda t, c: JF._operand(t, c, bf)
    od = JF.AttnOperand(True, E)
    assert not opn(wide, 4).aligned
    for q, want in ((opn(wide, 4), "gemm"), (opn(qkv, 0), "mh")):
        plan = JF.attn_plan(bf, 2, 8, 65, 33, E, q, opn(kv, 0), opn(kv, E), od, od, q, opn(kv, 0),
                            opn(kv, E))
        assert (plan.fwd, plan.rows, plan.bwd, plan.shared_q) == (want, False, want, False)
    # H = 2 (head dim 256) stays on the GEMM path
    rec_f, rec_b, meta, *_ = _fwd_bwd(bf, qkv, kv, go, 2)
    assert (rec_f, rec_b, meta.fwd) == (GEMM_FWD, GEMM_BWD, "gemm")


# ---- jmt.nn.MultiheadAttention(512, 8) against torch.nn.MultiheadAttention in float64

def _mha_run(m, x, w, mask, cd, fams):
    for p in m.parameters():
        p.grad = None
    xd = x.to(DEV).requires_grad_(True)
    ops.set_launch_hook(lambda info, launch: (fams.append(info["family"]), launch())[1])
    try:
        with JF.compute_mode(cd):
            out, _ = m(xd, xd, xd, key_padding_mask=None if mask is None else mask.to(DEV))
            (w.to(DEV) * out.float()).mean().backward()
        torch.cuda.synchronize()
    finally:
        ops.set_launch_hook(None)
    res = {k: p.grad.double().cpu() for k, p in m.named_parameters()}
    res["input"] = xd.grad.double().cpu()
    res["out"] = out.detach().double().cpu()
    return res


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "key_padding_mask"])
def test_mha_h8_matches_torch_float64(masked):
    T, B, H, cd = 37, 2, 8, torch.bfloat16
    g = torch.Generator().manual_seed(21)
    ref = torch.nn.MultiheadAttention(E, H).double()
    with torch.no_grad():
        ref.in_proj_weight.copy_(torch.randn(3 * E, E, generator=g) * E ** -0.5)
        ref.in_proj_bias.copy_(torch.randn(3 * E, generator=g) * 0.1)
        ref.out_proj.weight.copy_(torch.randn(E, E, generator=g) * E ** -0.5)
        ref.out_proj.bias.copy_(torch.randn(E, generator=g) * 0.1)
    m = jnn.MultiheadAttention(E, H)
    m.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    m = m.to(DEV)
    x = torch.randn(T, B, E, generator=g)
    w = torch.randn(T, B, E, generator=g)
    mask = None
    if masked:
        mask = torch.zeros(B, T, dtype=torch.bool)
        mask[0, :11] = True
        mask[1, :30] = True
    xr = x.double().requires_grad_(True)
    out_r, _ = ref(xr, xr, xr, key_padding_mask=mask, need_weights=False)
    (w.double() * out_r).mean().backward()
    want = {k: p.grad for k, p in ref.named_parameters()}
    want["input"], want["out"] = xr.grad, out_r.detach()

    fams, fams_g = [], []
    got = _mha_run(m, x, w, mask, cd, fams)
    ops._attn_mh["on"] = False
    try:
        got_g = _mha_run(m, x, w, mask, cd, fams_g)
    finally:
        ops._attn_mh["on"] = True
    assert fams.count("attn_mh_fwd") == 1 and fams.count("attn_mh_bwd") == 1
    assert not any(f.startswith("attn_mh") for f in fams_g)
    # the attention GEMMs (N H batches) are gone; the projections' GEMMs stay
    assert len(fams_g) - len(fams) == len(GEMM_FWD) + len(GEMM_BWD) - 2
    for k in sorted(want):
        err = (got[k] - want[k]).abs().max().item()
        err_g = (got_g[k] - want[k]).abs().max().item()
        print(f"{k}: mh {err:.3e} gemm {err_g:.3e} ratio {err / max(err_g, 1e-300):.3f} "
              f"(max |ref| {want[k].abs().max().item():.3e})")
    for k in sorted(want):
        assert torch.isfinite(got[k]).all(), k
        err = (got[k] - want[k]).abs().max().item()
        err_g = (got_g[k] - want[k]).abs().max().item()
        assert err <= 1.5 * err_g, (k, err, err_g)


# ---- Two_transformers(num_heads = 8)

def _model():
    from models.two_transformers import Two_transformers
    m = Two_transformers(0.0, 0.0, 8, 1, "TRANSFORMER", "FC", 2048)
    init_module_(m, "")
    return m.to(DEV)


def _model_run(m, cd, audio, video, w, mask, rec):
    for p in m.parameters():
        p.grad = None
    ops.set_launch_hook(lambda info, launch: (rec.append(dict(info)), launch())[1])
    try:
        with JF.compute_mode(cd):
            vo, ao = m(audio, video, key_padding_mask=mask) if mask is not None else m(audio, video)
            B, T = audio.shape[:2]
            lay = (lambda t: t.t()) if vo.shape == (T, B) and T != B else (lambda t: t)
            loss = ((lay(w[0]) * vo).sum() + (lay(w[1]) * ao).sum()) / vo.numel()
            loss.backward()
        torch.cuda.synchronize()
    finally:
        ops.set_launch_hook(None)
    grads = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    return lay(vo.detach()), lay(ao.detach()), grads, loss.detach()


def _attention_launches(rec):
    """(mh forward launches, mh backward launches, other attention launches): an attention GEMM
    is a batched GEMM over (sequence, head) pairs with the head dim 64 as one of its extents."""
    fams = [r["family"] for r in rec]
    other = [r["family"] for r in rec
             if (r["family"].startswith(("attn_", "small_attn")) and
                 not r["family"].startswith("attn_mh"))
             or (r["family"].startswith("gemm") and r["batch"] >= 8 and 64 in (r["N"], r["K"]))]
    return fams.count("attn_mh_fwd"), fams.count("attn_mh_bwd"), other


@pytest.mark.parametrize("on", [True, False], ids=["grouped", "ungrouped"])
@pytest.mark.parametrize("T,masked", [(37, False), (70, True)], ids=["T37", "T70_left_padded"])
def test_two_transformers_h8(T, masked, on):
    cd, B = torch.bfloat16, 2
    m = _model()
    g = torch.Generator(device=DEV).manual_seed(5)
    audio = torch.randn(B, T, E, device=DEV, generator=g)
    video = torch.randn(B, T, 2048, device=DEV, generator=g)
    w = torch.randn(2, B, T, device=DEV, generator=g)
    mask = None
    if masked:
        mask = torch.zeros(B, T, dtype=torch.bool, device=DEV)
        mask[0, :23] = True
        mask[1, :50] = True
        w = w * (~mask)
    rec = []
    grouped.set_enabled(on)
    try:
        v1, a1, g1, loss = _model_run(m, cd, audio, video, w, mask, rec)
        # the switch-off run shows what the records above replaced
        rec_g = []
        ops._attn_mh["on"] = False
        try:
            _model_run(m, cd, audio, video, w, mask, rec_g)
        finally:
            ops._attn_mh["on"] = True
        if masked:
            pad = mask[:, :, None]
            audio2 = torch.where(pad, torch.randn(B, T, E, device=DEV, generator=g) * 3, audio)
            video2 = torch.where(pad, torch.randn(B, T, 2048, device=DEV, generator=g) * 3, video)
            v2, a2, g2, _ = _model_run(m, cd, audio2, video2, w, mask, [])
    finally:
        grouped.set_enabled(True)
    n_fwd, n_bwd, other = _attention_launches(rec)
    # 3 encoders + 6 cross-attentions: 2 launches grouped, 9 otherwise, each with its backward
    assert n_fwd == n_bwd == (2 if on else 9), (n_fwd, n_bwd)
    assert other == [], other
    assert len(_attention_launches(rec_g)[2]) == 6 * n_fwd
    valid = ~mask if masked else torch.ones(B, T, dtype=torch.bool, device=DEV)
    assert torch.isfinite(v1[valid]).all() and torch.isfinite(a1[valid]).all()
    assert torch.isfinite(loss)
    assert len(g1) > 20
    for k in g1:
        assert torch.isfinite(g1[k]).all(), k
    if masked:
        # other finite values inside the padded frames: no prediction at a valid frame and no
        # parameter-gradient bit moves
        assert torch.equal(v1[valid], v2[valid]) and torch.equal(a1[valid], a2[valid])
        assert g1.keys() == g2.keys()
        for k in g1:
            assert torch.equal(g1[k], g2[k]), k


def test_mh_attention_in_a_captured_graph():
    """One attention forward + backward at (65, 33, 2), H = 8, captured with torch.cuda.graph and
    replayed twice: bit for bit the eager results (no host state, no allocation outside the
    capture's pool, every launch on the capturing stream)."""
    cd, H = torch.bfloat16, 8
    qkv, kv, go = _views(cd, 65, 33, 2, seed=73)

    def run():
        dqkv = torch.zeros(2, 65, 3 * E, device=DEV, dtype=cd).permute(1, 0, 2)
        dkv = torch.zeros(2, 33, 2 * E, device=DEV, dtype=cd).permute(1, 0, 2)
        with JF.compute_mode(cd):
            o, saved = JF.attn_forward(qkv, kv, kv, E, H, 0, 0, E)
            assert saved[1].fwd == "mh"
            JF.attn_backward(saved, go, dqkv, dkv, dkv)
        return o, dqkv, dkv

    eager = [t.clone() for t in run()]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    for _ in range(2):
        for t in outs:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(outs, eager):
            # dqkv: only the q columns are written (the rest was zeroed inside the capture)
            assert torch.equal(a, b)
