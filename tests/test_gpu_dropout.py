"""Regressor dropout on the HIP path (csrc/dropout.h, dropout.hip, the DROP head kernels,
jmt.functional.MLPFn / MLPPairFn, Two_transformers): the mask kernel against the host reference
bit for bit, the state block's tick, the functions against a float64 evaluation that multiplies
by the numpy reference mask (tests/dropout_ref.py), the model without torch's dropout, and a
captured step that draws a new mask per replay.

fp32 tolerances are DESIGN.md's fp32 row: 1e-4 for outputs, 1e-3 for gradients, as the largest
absolute error of a tensor relative to the largest reference magnitude of that tensor."""
import numpy as np
import pytest
import torch

from jmt import functional as JF
from jmt import ops
from jmt.graph import GraphedStep
from jmt.nn import MLP
from jmt.optim import FusedSGD, used_parameters
from oracle.hashinit import init_module_
from tests import dropout_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SEED = 0x0BADC0DE_12345678
DTYPES = pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16],
                                 ids=["f32", "bf16", "f16"])


def _ctr(call=5, stream=3, seed=SEED):
    words = (seed & 0xFFFFFFFF, seed >> 32, call, stream)
    t = torch.tensor([JF._u32(w) for w in words], dtype=torch.int32, device=DEV)
    return words, t


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ------------------------------------------------------------------ mask kernel
@DTYPES
@pytest.mark.parametrize("rows", [1, 63, 65, 130])
@pytest.mark.parametrize("cols", [4, 128, 256, 260])
def test_mask_kernel_matches_reference(dt, rows, cols):
    split = 4 if cols == 4 else 128
    p = (0.3, 0.5)
    words, ctr = _ctr()
    m = torch.from_numpy(R.mask(words, rows, cols, split, *p))
    assert np.array_equal(ops.dropout_reference(words, rows, cols, split, *p), m.numpy())
    ld, guard = cols + 12, 2
    # a NaN-prefilled buffer with guard rows above and below and padding right of `cols`
    full = torch.full((rows + 2 * guard, ld), float("nan"), dtype=dt, device=DEV)
    y = full[guard:guard + rows]
    x = torch.ones(rows, ld, dtype=dt, device=DEV)
    ops.dropout(x, ld, y, ld, rows, cols, split, *p, ctr)
    torch.cuda.synchronize()
    got = full.cpu()
    assert torch.equal(_bits(got[guard:guard + rows, :cols].contiguous()),
                       _bits(m.to(dt)))                       # ones * m: the multiplier itself
    assert bool(torch.isnan(got[:guard]).all()) and bool(torch.isnan(got[guard + rows:]).all())
    assert bool(torch.isnan(got[guard:guard + rows, cols:]).all())
    # random x: (x.float() * m).to(dt) as torch computes it on the CPU, out of place == in place
    g = torch.Generator().manual_seed(rows * 1000 + cols)
    xr = torch.randn(rows, ld, generator=g).to(dt)
    want = (xr[:, :cols].float() * m).to(dt)
    xd = xr.to(DEV)
    out = torch.full((rows, ld), float("nan"), dtype=dt, device=DEV)
    ops.dropout(xd, ld, out, ld, rows, cols, split, *p, ctr)
    inplace = xd.clone()
    ops.dropout(inplace, ld, inplace, ld, rows, cols, split, *p, ctr)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out[:, :cols].cpu().contiguous()), _bits(want))
    assert torch.equal(_bits(inplace[:, :cols].cpu().contiguous()), _bits(want))
    assert torch.equal(_bits(inplace[:, cols:].cpu().contiguous()),
                       _bits(xr[:, cols:].contiguous()))      # padding untouched in place
    assert torch.equal(_bits(xd.cpu()), _bits(xr))            # the source of the copy form too


def test_mask_kernel_rejects_bad_arguments():
    from jmt._lib import JMTError
    _, ctr = _ctr()
    x = torch.ones(8, 16, dtype=torch.bfloat16, device=DEV)
    for args in [(x, 16, x, 16, 8, 6, 4, 0.1, 0.1), (x, 16, x, 16, 8, 8, 6, 0.1, 0.1),
                 (x, 16, x, 16, 8, 8, 4, 1.0, 0.1), (x, 6, x, 16, 8, 4, 4, 0.1, 0.1),
                 (x, 16, x, 16, 2 ** 32, 8, 4, 0.1, 0.1)]:
        with pytest.raises(JMTError):
            ops.dropout(*args, ctr)


# ------------------------------------------------------------------ state block
def test_dropout_next_copies_then_ticks():
    JF.set_dropout_state(SEED, call=2 ** 32 - 2, stream=3)
    st = JF._drop_block(DEV)
    before = st.clone()
    out = ops.dropout_next(st)
    torch.cuda.synchronize()
    assert torch.equal(out, before)
    assert JF.dropout_state() == {"seed": SEED, "call": 2 ** 32 - 1, "stream": 3}
    out2 = ops.dropout_next(st)
    assert [int(v) & 0xFFFFFFFF for v in out2.cpu().tolist()][2] == 2 ** 32 - 1
    assert JF.dropout_state()["call"] == 0                    # wraps; seed and stream stay
    assert JF.dropout_state()["seed"] == SEED and JF.dropout_state()["stream"] == 3


def _gys(n, shape):
    """Output gradients without cancellation (all positive): the output-layer weight and bias
    gradients are sums over the rows, and a relative bound on a sum that nearly cancels (the
    linspace(-1, 1) of test_mlp_pair_matches_two_mlps sums to 0) would bound nothing."""
    i = torch.arange(n, dtype=torch.float32)
    return ((0.25 + 0.75 * i / max(n - 1, 1)).view(shape),
            (0.6 + 0.4 * torch.cos(i)).view(shape))


def _mlp_pair_run(x, va, aa, p, cd):
    """Forward (+ backward) of the pair; returns outputs, dx, parameter gradients."""
    for m in (va, aa):
        for q in m.parameters():
            q.grad = None
    xx = x.clone().requires_grad_(True)
    with JF.compute_mode(cd):
        v, a = JF.mlp_pair(xx, va, aa, out_dtype=torch.float32, p=p)
        gv, ga = (g.to(DEV) for g in _gys(v.numel(), v.shape))
        ((v * gv).sum() + (a * ga).sum()).backward()
    torch.cuda.synchronize()
    grads = [q.grad.clone() for m in (va, aa) for q in m.parameters()]
    return [v.detach(), a.detach(), xx.grad.detach().float()] + grads


@pytest.mark.parametrize("cd", [torch.float32, torch.bfloat16], ids=["fp32-gemm", "bf16-head"])
def test_two_forwards_then_their_backwards_in_reverse_order(cd):
    """Each backward regenerates its own forward's mask from the 16 bytes that forward kept."""
    torch.manual_seed(3)
    E, rows, p = 128, 65, (0.3, 0.5)
    va, aa = MLP(E, 128, 1, dropout=p[0]).to(DEV), MLP(E, 128, 1, dropout=p[1]).to(DEV)
    x = torch.randn(rows, E, device=DEV)
    singles = []
    for call in (10, 11):
        JF.set_dropout_state(SEED, call=call, stream=0)
        singles.append(_mlp_pair_run(x, va, aa, p, cd))
    JF.set_dropout_state(SEED, call=10, stream=0)
    xs = [x.clone().requires_grad_(True) for _ in range(2)]
    with JF.compute_mode(cd):
        outs = [JF.mlp_pair(xx, va, aa, out_dtype=torch.float32, p=p) for xx in xs]
        for i in (1, 0):
            v, a = outs[i]
            gv, ga = (g.to(DEV) for g in _gys(v.numel(), v.shape))
            ((v * gv).sum() + (a * ga).sum()).backward()
    torch.cuda.synchronize()
    assert JF.dropout_state()["call"] == 12
    for i in (0, 1):
        assert torch.equal(outs[i][0], singles[i][0]) and torch.equal(outs[i][1], singles[i][1])
        assert torch.equal(xs[i].grad, singles[i][2])
    assert not torch.equal(xs[0].grad, xs[1].grad)


# ------------------------------------------------------------------ float64 reference
def _ref64(x, mods, masks, gys):
    """float64 torch evaluation of MLPs on x with the given (rows, 128) multipliers; returns
    outputs, dx and parameter gradients in the order of _mlp_pair_run."""
    xx = x.detach().double().cpu().requires_grad_(True)
    ps, outs = [], []
    for mod, m in zip(mods, masks):
        l1, l2 = mod[0], mod[len(mod) - 1]
        w = [t.detach().double().cpu().requires_grad_(True)
             for t in (l1.weight, l1.bias, l2.weight, l2.bias)]
        h = torch.relu(xx @ w[0].t() + w[1]) * m.double()
        outs.append(h @ w[2].t() + w[3])
        ps += w
    sum((o * g.double().cpu()).sum() for o, g in zip(outs, gys)).backward()
    return [o.detach() for o in outs] + [xx.grad] + [q.grad for q in ps]


def _close32(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        tol = 1e-4 if i < what else 1e-3
        scale = float(w.abs().max())
        err = float((g.double().cpu() - w).abs().max())
        assert g.shape == w.shape and err <= tol * scale, (i, err, scale)


@pytest.mark.parametrize("k", [1, 20])
@pytest.mark.parametrize("rows", [1, 65, 222])
def test_mlp_pair_fp32_matches_float64_with_reference_mask(k, rows):
    torch.manual_seed(11)
    E, p = 1024, (0.3, 0.5)
    va, aa = MLP(E, 128, k, dropout=p[0]).to(DEV), MLP(E, 128, k, dropout=p[1]).to(DEV)
    x = torch.randn(rows, E, device=DEV)                  # contiguous: row = memory row
    JF.set_dropout_state(SEED, call=7, stream=2)
    got = _mlp_pair_run(x, va, aa, p, torch.float32)
    assert JF.dropout_state()["call"] == 8
    m = torch.from_numpy(R.mask((SEED & 0xFFFFFFFF, SEED >> 32, 7, 2), rows, 256, 128, *p))
    want = _ref64(x, (va, aa), (m[:, :128], m[:, 128:]), _gys(rows * k, (rows, k)))
    _close32(got, want, 2)


@pytest.mark.parametrize("cd", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("k", [1, 20])
@pytest.mark.parametrize("rows", [(1, 1), (13, 5), (37, 6)], ids=["1", "65", "222"])
def test_mlp_pair_16bit_fused_head_as_accurate_as_gemm_route(cd, k, rows):
    """The criterion of test_mlp_pair_matches_two_mlps: against the fp32 pair under the same
    mask, the fused head's error is <= 1.5 x max(the GEMM route's error, u) per quantity."""
    torch.manual_seed(13)
    T, B = rows
    E, p = 1024, (0.3, 0.5)
    va, aa = MLP(E, 128, k, dropout=p[0]).to(DEV), MLP(E, 128, k, dropout=p[1]).to(DEV)
    x = torch.randn(B, T, E, device=DEV).permute(1, 0, 2)      # seq-first view
    runs = {}
    try:
        for name, c, fused in (("fused", cd, True), ("gemm", cd, False),
                               ("fp32", torch.float32, True)):
            JF._fused_head_on["on"] = fused
            JF.set_dropout_state(SEED, call=21, stream=0)
            runs[name] = _mlp_pair_run(x, va, aa, p, c)
    finally:
        JF._fused_head_on["on"] = True
    u = 2 ** -8 if cd == torch.bfloat16 else 2 ** -11
    for r32, r, g in zip(runs["fp32"], runs["gemm"], runs["fused"]):
        assert r.shape == g.shape
        den = max(float(r32.norm()), 1e-2)
        e_gemm = float((r.float() - r32).norm()) / den
        e_fused = float((g.float() - r32).norm()) / den
        assert e_fused <= 1.5 * max(e_gemm, u), (e_fused, e_gemm)


@pytest.mark.parametrize("rows", [1, 65, 222])
def test_mlp_fp32_matches_float64_with_reference_mask(rows):
    """MLPFn as SingleBackbonePretrainer uses it (512 -> 128 -> 2)."""
    torch.manual_seed(17)
    p = 0.4
    mod = MLP(512, 128, 2, dropout=p).to(DEV)
    x = torch.randn(rows, 512, device=DEV)
    xx = x.clone().requires_grad_(True)
    JF.set_dropout_state(SEED, call=9, stream=1)
    with JF.compute_mode(torch.float32):
        y = mod(xx, out_dtype=torch.float32)
        gy = _gys(y.numel(), y.shape)[1].to(DEV)
        (y * gy).sum().backward()
    torch.cuda.synchronize()
    got = [y.detach(), xx.grad] + [q.grad for q in mod.parameters()]
    m = torch.from_numpy(R.mask((SEED & 0xFFFFFFFF, SEED >> 32, 9, 1), rows, 128, 128, p, p))
    want = _ref64(x, (mod,), (m,), (gy.cpu(),))
    _close32(got, want, 1)
    mod.eval()
    with JF.compute_mode(torch.float32):
        y_eval = mod(x, out_dtype=torch.float32)
    assert JF.dropout_state()["call"] == 10                 # eval draws nothing
    assert not torch.equal(y_eval, y.detach())


# ------------------------------------------------------------------ model
def _model(pv, pa):
    from models.two_transformers import Two_transformers
    m = Two_transformers(pv, pa, 1, 1, "TRANSFORMER", "FC", 2048)
    init_module_(m, "")
    return m.to(DEV)


def _model_inputs(B=2, T=8):
    g = torch.Generator(device=DEV).manual_seed(5)
    return (torch.randn(B, T, 512, device=DEV, generator=g),
            torch.randn(B, T, 2048, device=DEV, generator=g))


def _train_once(m, a, v, cd=torch.float32):
    for q in m.parameters():
        q.grad = None
    with JF.compute_mode(cd):
        vo, ao = m(a, v)
        (vo.sum() + 2 * ao.sum()).backward()
    torch.cuda.synchronize()
    return vo.detach(), ao.detach(), {n: q.grad.clone() for n, q in m.named_parameters()
                                      if q.grad is not None}


def test_model_trains_without_torch_dropout(monkeypatch):
    m = _model(0.3, 0.5).train()
    a, v = _model_inputs()

    def boom(*args, **kw):
        raise AssertionError("torch dropout on the regressor path")

    monkeypatch.setattr(torch.nn.functional, "dropout", boom)
    monkeypatch.setattr(torch, "dropout", boom)
    seen = []
    orig = JF.MLPPairFn.apply

    def spy(*args):
        seen.append(args[-2:])
        return orig(*args)

    monkeypatch.setattr(JF.MLPPairFn, "apply", spy)
    JF.set_dropout_state(SEED, call=0, stream=0)
    vo, ao, grads = _train_once(m, a, v)
    assert seen == [(0.3, 0.5)]
    assert JF.dropout_state()["call"] == 1
    assert bool(torch.isfinite(vo).all()) and bool(torch.isfinite(ao).all())
    assert float(grads["vregressor.0.weight"].norm()) > 0


def test_model_eval_equals_the_undropped_model():
    m, m0 = _model(0.3, 0.5).eval(), _model(0.0, 0.0).eval()
    m0.load_state_dict(m.state_dict())
    a, v = _model_inputs()
    JF.set_dropout_state(SEED, call=4, stream=0)
    for cd in (torch.float32, torch.bfloat16):
        with JF.compute_mode(cd), torch.no_grad():
            vo, ao = m(a, v)
            vo0, ao0 = m0(a, v)
        assert torch.equal(vo, vo0) and torch.equal(ao, ao0)
    assert JF.dropout_state()["call"] == 4


@pytest.mark.parametrize("cd", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_model_masks_differ_per_call_and_repeat_per_state(cd):
    m = _model(0.3, 0.5).train()
    a, v = _model_inputs()
    JF.set_dropout_state(SEED, call=0, stream=0)
    r0 = _train_once(m, a, v, cd)
    r1 = _train_once(m, a, v, cd)
    assert not torch.equal(r0[0], r1[0]) and not torch.equal(r0[1], r1[1])
    saved = JF.dropout_state()
    assert saved["call"] == 2
    JF.set_dropout_state(SEED, call=0, stream=0)
    again = _train_once(m, a, v, cd)
    assert torch.equal(again[0], r0[0]) and torch.equal(again[1], r0[1])
    assert again[2].keys() == r0[2].keys()
    for n in r0[2]:
        assert torch.equal(again[2][n], r0[2][n]), n
    JF.set_dropout_state(SEED, call=0, stream=1)               # another rank's stream
    other = _train_once(m, a, v, cd)
    assert not torch.equal(other[0], r0[0])


# ------------------------------------------------------------------ graph
def _step_setup(cd, B=2, T=8):
    from models.fc_layer import FcLayer
    from losses.loss import CCCLoss
    m = _model(0.3, 0.5).train()
    fc = FcLayer(1024, 512)
    init_module_(fc, "fc.")
    fc = fc.to(DEV)
    g = torch.Generator(device=DEV).manual_seed(7)
    audio = torch.randn(B, T, 1024, device=DEV, generator=g)
    video = torch.randn(B, T, 2048, device=DEV, generator=g)
    lv = (torch.rand(B, T, device=DEV, generator=g) * 2 - 1).view(-1, B * T)
    la = (torch.rand(B, T, device=DEV, generator=g) * 2 - 1).view(-1, B * T)
    crit = CCCLoss(1)

    def fwd_bwd():
        with JF.compute_mode(cd):
            vo, ao = m(fc(audio), video)
            loss = crit(vo.view(-1, B * T), lv) + crit(ao.view(-1, B * T), la)
            loss.backward()
        return loss

    params = used_parameters(fwd_bwd, list(m.parameters()) + list(fc.parameters()))
    opt = FusedSGD(params, lr=1e-2, momentum=0.9, dampening=0.0, weight_decay=1e-4,
                   nesterov=True, shadow_dtype=cd if cd != torch.float32 else None)

    def step():
        opt.zero_grad()
        loss = fwd_bwd()
        opt.step()
        return loss.detach()

    return step, opt


@pytest.mark.parametrize("cd", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_graph_replay_draws_new_masks_like_eager(cd):
    """3 replays of the captured step == 3 eager steps from the same (seed, call): the eager run
    takes 2 warm-up steps (calls 0, 1), the graphed run one eager step and the capture's own
    warm-up step (calls 0, 1; the capture pass itself executes nothing), so both take their 3
    measured steps at calls 2, 3, 4."""
    step_e, opt_e = _step_setup(cd)
    JF.set_dropout_state(SEED, call=0, stream=0)
    for _ in range(2):
        step_e()
    eager = [float(step_e()) for _ in range(3)]
    torch.cuda.synchronize()
    pe = opt_e.flat_p.clone()
    assert JF.dropout_state()["call"] == 5

    step_g, opt_g = _step_setup(cd)
    JF.set_dropout_state(SEED, call=0, stream=0)
    step_g()
    gs = GraphedStep(step_g).capture(warmup=1)
    assert JF.dropout_state()["call"] == 2
    graphed = [float(gs.replay()) for _ in range(3)]
    torch.cuda.synchronize()
    assert graphed == eager, (graphed, eager)
    assert torch.equal(opt_g.flat_p, pe)
    assert JF.dropout_state()["call"] == 5
    assert len(set(graphed)) == 3, graphed
