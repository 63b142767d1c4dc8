"""Two_transformers(..., 'TRANSFORMER', ...).forward(key_padding_mask=...): the (B, T) mask is
converted to key ranges once and used by the three encoders and the six cross-attentions, on the
grouped and the ungrouped path, with the FC and the SELF_ATTEN head.

B = 3 windows: one left-padded, one right-padded, one full; T = 70 (whole-row kernels, shared
queries, grouped launches) and T = 16 (short kernels).  Objective mean(w * outputs) with w = 0 at
padded frames.

Invariance (bf16, exact): masked keys get probability exactly 0, padded rows receive a zero
output gradient from the objective, a zero dO row gives dP = Delta = dS = 0, so padded rows
contribute exact zeros to every deterministic weight- and bias-gradient sum: other finite values
in the padded frames change no prediction at a valid frame and no parameter gradient bit.
Truncation (fp32): with every window right-padded to the same length, the masked model equals
the unmasked model on the truncated input at the project's fp32 tolerances.

One more path had to be closed for this to hold at T = 70: a padded frame is also a QUERY row,
and the whole-row forward votes its lazy rescale per wave of 16 query rows, so with one vote over
all rows a padded row's scores changed the rounding of its neighbours' O (14 of 334 valid
predictions moved by up to 2.2e-2 with padding 23 / 50, none with 16-row-aligned padding).  The
range form of the kernel keeps rows whose own index is a masked key out of the other rows' vote
(key ranges); test_..._16_row_aligned keeps the case that never depended on it."""
import pytest
import torch

from jmt import functional as JF
from jmt import grouped, ops
from jmt.graph import GraphedStep
from oracle.hashinit import init_module_

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
E = 512
B = 3


def _model(head):
    from models.two_transformers import Two_transformers
    m = Two_transformers(0.0, 0.0, 1, 1, "TRANSFORMER", head, vision_in_ft=512)
    init_module_(m, "")
    return m.to(DEV)


def _mask(T, runs):
    m = torch.ones(len(runs), T, dtype=torch.bool, device=DEV)
    for b, (s, e) in enumerate(runs):
        m[b, s:e] = False
    return m


def _runs(T, aligned=False):
    """Valid runs of the three windows: left-padded, right-padded, full.  aligned (T = 70): the
    padding covers whole 16-row groups of query rows."""
    if aligned:
        return [(32, T), (0, 48), (0, T)]
    return [(23, T), (0, 50), (0, T)] if T == 70 else [(5, T), (0, 11), (0, T)]


def _inputs(T, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    audio = torch.randn(B, T, E, device=DEV, generator=g)
    video = torch.randn(B, T, E, device=DEV, generator=g)
    w = torch.randn(2, B, T, device=DEV, generator=g)
    return audio, video, w


def _run(m, cd, audio, video, w, mask, denom=None):
    """Forward + backward of mean(w * outputs) (sum / denom); returns the predictions as (B, T)
    and the parameter gradients."""
    for p in m.parameters():
        p.grad = None
    with JF.compute_mode(cd):
        vo, ao = m(audio, video, key_padding_mask=mask) if mask is not None else m(audio, video)
        T = audio.shape[1]
        lay = (lambda t: t.t()) if vo.shape == (T, B) and T != B else (lambda t: t)
        denom = denom or vo.numel()
        loss = ((lay(w[0]) * vo).sum() + (lay(w[1]) * ao).sum()) / denom
        loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    return lay(vo.detach()), lay(ao.detach()), grads, loss.detach()


@pytest.mark.parametrize("on", [True, False], ids=["grouped", "ungrouped"])
@pytest.mark.parametrize("T", [70, 16])
@pytest.mark.parametrize("head", ["FC", "SELF_ATTEN"])
def test_padded_frames_change_nothing(head, T, on):
    _padded_frames_change_nothing(head, T, on, _runs(T))


@pytest.mark.parametrize("on", [True, False], ids=["grouped", "ungrouped"])
@pytest.mark.parametrize("head", ["FC", "SELF_ATTEN"])
def test_padded_frames_change_nothing_16_row_aligned(head, on):
    """T = 70 with padding that covers whole 16-row groups of query rows (see the module
    docstring): no valid frame shares a wave of the whole-row forward with a padded one."""
    _padded_frames_change_nothing(head, 70, on, _runs(70, aligned=True))


def _padded_frames_change_nothing(head, T, on, runs):
    cd = torch.bfloat16
    m = _model(head)
    mask = _mask(T, runs)
    audio, video, w = _inputs(T, 5)
    w = w * (~mask)                                          # zero weight at padded frames
    g = torch.Generator(device=DEV).manual_seed(6)
    pad = mask[:, :, None]
    audio2 = torch.where(pad, torch.randn(B, T, E, device=DEV, generator=g) * 3, audio)
    video2 = torch.where(pad, torch.randn(B, T, E, device=DEV, generator=g) * 3, video)
    # the time-axis attentions are on the kernels this is about, not on the GEMM path
    q, od = JF.AttnOperand(True, 3 * E), JF.AttnOperand(True, E)
    for n in (3 * B, 6 * B):
        plan = JF.attn_plan(cd, n, 1, T, T, E, q, q, q, od, od, q, q, q, kr=True)
        assert (plan.fwd, plan.bwd) == (("fused", "pds_dkdv") if T == 70 else ("short", "short"))
    fams = []
    ops.set_launch_hook(lambda info, launch: (fams.append(info.get("family")), launch())[1])
    grouped.set_enabled(on)
    try:
        v1, a1, g1, _ = _run(m, cd, audio, video, w, mask)
        n_fwd = fams.count("attn_fwd" if T == 70 else "attn_short_fwd")
        n_bwd = fams.count("attn_bwd" if T == 70 else "attn_short_bwd")
        v2, a2, g2, _ = _run(m, cd, audio2, video2, w, mask)
    finally:
        grouped.set_enabled(True)
        ops.set_launch_hook(None)
    # 3 encoders + 6 cross-attentions: 2 launches grouped, 9 otherwise, each with its backward
    assert n_fwd == n_bwd == (2 if on else 9), (n_fwd, n_bwd, fams)
    valid = ~mask
    assert torch.isfinite(v1[valid]).all() and torch.isfinite(a1[valid]).all()
    dv, da = (v1 - v2)[valid].abs(), (a1 - a2)[valid].abs()
    print(f"predictions: {int((dv > 0).sum()) + int((da > 0).sum())} of {2 * dv.numel()} differ, "
          f"max |d| {max(dv.max().item(), da.max().item()):.3e} "
          f"(max |pred| {max(v1[valid].abs().max().item(), a1[valid].abs().max().item()):.3e})")
    assert g1.keys() == g2.keys() and len(g1) > 20
    worst = max(((g1[k] - g2[k]).abs().max().item() / max(g1[k].abs().max().item(), 1e-30), k)
                for k in g1)
    print(f"gradients: {sum(not torch.equal(g1[k], g2[k]) for k in g1)} of {len(g1)} differ, "
          f"worst max |d| / max |g| {worst[0]:.3e} ({worst[1]})")
    assert torch.equal(v1[valid], v2[valid]) and torch.equal(a1[valid], a2[valid])
    for k in g1:
        assert torch.isfinite(g1[k]).all(), k
        assert torch.equal(g1[k], g2[k]), k
    # and the mask is not a no-op: without it the padded frames do reach the valid predictions
    grouped.set_enabled(on)
    try:
        v3, _, _, _ = _run(m, cd, audio2, video2, w, None)
    finally:
        grouped.set_enabled(True)
    assert not torch.equal(v1[valid], v3[valid])


@pytest.mark.parametrize("on", [True, False], ids=["grouped", "ungrouped"])
@pytest.mark.parametrize("head", ["FC", "SELF_ATTEN"])
def test_right_padding_equals_truncation_fp32(head, on):
    cd, T, Lp = torch.float32, 70, 50
    m = _model(head)
    mask = _mask(T, [(0, Lp)] * B)
    audio, video, w = _inputs(T, 9)
    w = w * (~mask)
    grouped.set_enabled(on)
    try:
        v1, a1, g1, _ = _run(m, cd, audio, video, w, mask, denom=B * Lp)
        v2, a2, g2, _ = _run(m, cd, audio[:, :Lp].contiguous(), video[:, :Lp].contiguous(),
                             w[:, :, :Lp].contiguous(), None, denom=B * Lp)
    finally:
        grouped.set_enabled(True)
    for got, ref in ((v1[:, :Lp], v2), (a1[:, :Lp], a2)):
        err = (got - ref).abs().max().item()
        print(f"pred err {err:.3e} tol {1e-4 * ref.abs().max().item():.3e}")
        assert err <= 1e-4 * ref.abs().max().item()
    assert g1.keys() == g2.keys()
    for k in g1:
        err = (g1[k] - g2[k]).abs().max().item()
        tol = 1e-3 * g2[k].abs().max().item()
        print(f"{k} err {err:.3e} tol {tol:.3e}")
        assert err <= tol, k


def test_none_with_a_mask_raises():
    from models.two_transformers import Two_transformers
    m = Two_transformers(0.0, 0.0, 1, 1, "NONE", "FC", vision_in_ft=512).to(DEV)
    audio, video, _ = _inputs(16, 1)
    with pytest.raises(NotImplementedError):
        m(audio, video, key_padding_mask=_mask(16, _runs(16)))
    fc = Two_transformers(0.0, 0.0, 1, 1, "FC", "FC", vision_in_ft=512).to(DEV)
    with JF.compute_mode(torch.float32):                     # no attention: the mask is ignored
        a = fc(audio, video, key_padding_mask=_mask(16, _runs(16)))
        b = fc(audio, video)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_graph_replay_reads_the_mask_buffer():
    """Forward + backward captured with a static mask buffer; a replay after another mask is
    written into the buffer equals the eager run with that mask bit for bit, and a bad mask
    written before a replay is reported by check_key_ranges() afterwards."""
    cd, T = torch.bfloat16, 70
    m = _model("FC")
    audio, video, w = _inputs(T, 13)
    mask_a, mask_b = _mask(T, _runs(T)), _mask(T, [(0, 61), (7, T), (30, 41)])
    buf = mask_a.clone()
    params = [p for p in m.parameters()]

    def step():
        for p in params:
            if p.grad is not None:
                p.grad.zero_()
        with JF.compute_mode(cd):
            vo, ao = m(audio, video, key_padding_mask=buf)
            loss = ((w[0].t() * vo).sum() + (w[1].t() * ao).sum()) / vo.numel()
            loss.backward()
        return loss.detach()

    step()                                                   # eager: gradients and the counter exist
    gs = GraphedStep(step).capture(warmup=1)
    buf.copy_(mask_b)
    loss_g = gs.replay().clone()
    torch.cuda.synchronize()
    grads_g = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    JF.check_key_ranges()                                    # both masks were fine
    loss_e = step()                                          # eager, with mask_b in the buffer
    torch.cuda.synchronize()
    assert torch.equal(loss_g, loss_e), (float(loss_g), float(loss_e))
    for k, p in m.named_parameters():
        if p.grad is not None:
            assert torch.equal(grads_g[k], p.grad), k
    # mask_a gives other numbers: the replay did read the buffer
    buf.copy_(mask_a)
    assert not torch.equal(gs.replay().clone(), loss_g)
    # a bad mask (window 1 fully padded) written before a replay
    buf[1] = True
    gs.replay()
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        JF.check_key_ranges()
    JF.check_key_ranges()                                    # cleared
