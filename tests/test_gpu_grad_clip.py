"""Gradient-norm clipping in the fused optimizers (csrc/grad_norm.hip, the *_clip step entry
points, jmt/optim.py) on the GPU:

* the norm kernels against the float64 reference of tests/clip_ref.py on its case table, every
  figure within 2^-23 relative (derived there), with NaN guards past the buffer and the scratch;
* the central identity: a clipped step on g is, bit for bit, the unclipped step on fp32(c * g);
* three steps of SGD against clip_grad_norm_ + torch.optim.SGD in float64 on the same gradients;
* the clipped step captured into a hipGraph replays like it steps eagerly, follows
  set_max_grad_norm between replays, and adds exactly the norm launches to the step."""
import math

import pytest
import torch

from jmt import _lib
from jmt import functional as JF
from jmt import ops
from jmt.graph import GraphedStep
from jmt.optim import FusedAdam, FusedSGD, GradScaler, used_parameters
from oracle.hashinit import init_module_
from tests import clip_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
GUARD = 64
NAN = float("nan")


def _grid():
    return torch.cuda.get_device_properties(0).multi_processor_count * R.BLOCKS_PER_CU


# ------------------------------------------------------------------------------- norm kernels
def _run_norm(g, max_norm, gs=1.0, off=None, amp=None):
    """jmt_grad_norm on g (fp32, CPU) placed in a buffer with NaN guards behind it; returns
    ((norm, coef, seg norms), raw state, the buffers for the guard checks)."""
    n = g.numel()
    buf = torch.full((n + GUARD,), NAN, dtype=torch.float32, device=DEV)
    buf[:n].copy_(g)
    nseg = len(off) - 1 if off is not None else 0
    nbytes = _lib.load().jmt_grad_norm_scratch(n, nseg)
    assert nbytes > 0 and nbytes % 8 == 0
    scratch = torch.full((nbytes // 8 + GUARD,), NAN, dtype=torch.float64, device=DEV)
    state = torch.tensor([0.0, 0.0, 0.0, 0.0, -7.0, -7.0, max_norm, -7.0], dtype=torch.float32,
                         device=DEV)
    seg_off = torch.tensor(off, dtype=torch.int64, device=DEV) if nseg else None
    seg_norm = torch.full((nseg + GUARD,), NAN, dtype=torch.float32, device=DEV)
    _lib.call("jmt_grad_norm", n, buf.data_ptr(), state.data_ptr(), scratch.data_ptr(), nbytes,
              seg_off.data_ptr() if nseg else None, nseg, seg_norm.data_ptr() if nseg else None,
              gs, amp.data_ptr() if amp is not None else None, ops.stream())
    torch.cuda.synchronize()
    st = state.cpu()
    segs = seg_norm[:nseg].double().cpu().tolist()
    return (float(st[5]), float(st[4]), segs), st, (buf, scratch, seg_norm, nbytes // 8, nseg)


@pytest.fixture(scope="module")
def table():
    return {c[0]: c for c in R.cases(_grid())}


@pytest.fixture(scope="module")
def refs(table):
    return {k: R.reference(*c[1:]) for k, c in table.items()}


CASE_NAMES = [c[0] for c in R.cases(1)]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_norm_kernel_against_float64(table, refs, name):
    _, g, max_norm, gs, off = table[name]
    ref = refs[name]
    got, st, (buf, scratch, seg_norm, nscr, nseg) = _run_norm(g, max_norm, gs, off)
    n = g.numel()
    print(name, n, "norm", got[0], ref[0], "coef", got[1], ref[1])
    for a, b in zip(got[2], ref[2]):
        print("  seg", a, b)
    # only slots 4 and 5 are written; max_norm is an input
    assert st[[0, 1, 2, 3]].tolist() == [0.0] * 4 and float(st[7]) == -7.0
    assert float(st[6]) == R.f32(max_norm) or (math.isinf(max_norm) and math.isinf(float(st[6])))
    # the guards: nothing past n was read (it would poison the norm) or written
    assert bool(torch.isnan(buf[n:]).all())
    assert torch.equal(buf[:n].cpu().view(torch.int32), g.contiguous().view(torch.int32))
    assert bool(torch.isnan(scratch[nscr:]).all())
    assert bool(torch.isnan(seg_norm[nseg:]).all())
    assert R.close(got[0], ref[0]), (name, "norm", got[0], ref[0])
    assert R.close(got[1], ref[1]), (name, "coef", got[1], ref[1])
    # without a table the kernel writes no segment norms (the reference's one segment is the total)
    assert len(got[2]) == (len(ref[2]) if off is not None else 0)
    for i, (a, b) in enumerate(zip(got[2], ref[2])):
        assert R.close(a, b), (name, "segment", i, a, b)
    if off is not None and math.isfinite(ref[0]):
        # the total is the sum of the segment sums: the stored segment norms reproduce it
        tot = 0.0
        for a in got[2]:
            tot += a * a
        assert R.close(math.sqrt(tot), ref[0]), (name, math.sqrt(tot), ref[0])


def test_partials_exceed_the_fold_block(table):
    n = table["second_trip"][1].numel()
    assert n == _grid() * R.CHUNK + 300
    if _grid() >= R.FOLD_THREADS:
        assert -(-n // R.CHUNK) > R.FOLD_THREADS


def test_non_finite_follow_torch(table):
    got, _, _ = _run_norm(*table["nan"][1:])
    assert math.isnan(got[0]) and math.isnan(got[1])
    got, _, _ = _run_norm(*table["inf"][1:])
    assert got[0] == math.inf and got[1] == 0.0
    got, _, _ = _run_norm(*table["inf_measure_only"][1:])
    assert got[0] == math.inf and math.isnan(got[1])


@pytest.mark.parametrize("name", ["second_trip", "seg37"])
def test_two_runs_are_bit_identical(table, name):
    _, g, max_norm, gs, off = table[name]
    a, sa, ba = _run_norm(g, max_norm, gs, off)
    b, sb, bb = _run_norm(g, max_norm, gs, off)
    assert torch.equal(sa.view(torch.int32), sb.view(torch.int32))
    assert torch.equal(ba[2][:ba[4]].view(torch.int32), bb[2][:bb[4]].view(torch.int32))
    assert torch.equal(ba[1][:ba[3]].view(torch.int64), bb[1][:bb[3]].view(torch.int64))


def test_unscale_factor_comes_from_the_scaler_state(table):
    """amp != NULL: gs = amp[1], the grad_scale argument is ignored."""
    _, g, max_norm, gs, off = table["seg_unscale"]
    amp = torch.tensor([1.0 / gs, gs, 0.0, 0.0, 0.0], dtype=torch.float32, device=DEV)
    a, sa, _ = _run_norm(g, max_norm, gs, off)
    b, sb, _ = _run_norm(g, max_norm, 123.0, off, amp=amp)
    assert torch.equal(sa, sb) and a == b


# ------------------------------------------------------------------------------- step identity
SHAPES = [(37, 5), (64,), (129, 33), (1000,), (3,), (70, 64)]


def _params(seed=0):
    gen = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(*s, generator=gen).to(DEV)) for s in SHAPES]


def _make(kind, shadow, fzg, max_grad_norm):
    kw = dict(shadow_dtype=shadow, fuse_zero_grad=fzg, max_grad_norm=max_grad_norm)
    if kind == "sgd":
        return FusedSGD(_params(), lr=1e-2, momentum=0.9, nesterov=True, weight_decay=1e-4,
                        device_lr=True, **kw)
    return FusedAdam(_params(), lr=1e-3, weight_decay=1e-4, amsgrad=(kind == "adam_ams"), **kw)


def _flat_grads(opt, seed, scale=1.0):
    """Random gradients in the flat layout, the padding zero."""
    gen = torch.Generator().manual_seed(100 + seed)
    g = torch.zeros(opt.numel)
    for p, off in zip(opt.params, opt.offsets):
        g[off:off + p.numel()] = torch.randn(p.numel(), generator=gen) * scale
    return g.to(DEV)


def _same_state(a, b):
    for name in ("flat_p", "shadow", "flat_g") + a._BUFFERS:
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), name
        if x is not None:
            assert torch.equal(x.view(torch.int16 if x.element_size() == 2 else torch.int32),
                               y.view(torch.int16 if y.element_size() == 2 else torch.int32)), name
    assert torch.equal(a.state[:4], b.state[:4])


KINDS = pytest.mark.parametrize("kind", ["sgd", "adam", "adam_ams"])
SHADOWS = pytest.mark.parametrize("shadow", [None, torch.bfloat16], ids=["no_shadow", "bf16"])
FZG = pytest.mark.parametrize("fzg", [False, True], ids=["keep_grad", "fuse_zero_grad"])


@KINDS
@SHADOWS
@FZG
def test_clipped_step_is_the_unclipped_step_on_c_times_g(kind, shadow, fzg):
    g0 = _flat_grads(_make(kind, None, False, None), 0)
    max_norm = float(g0.double().norm()) / 10.0
    opt, twin = _make(kind, shadow, fzg, max_norm), _make(kind, shadow, fzg, None)
    for k in range(3):
        g = _flat_grads(opt, k)
        opt.flat_g.copy_(g)
        opt.step()
        c = opt.clip_coef().clone()
        assert 0.05 < float(c) < 0.2
        twin.flat_g.copy_(g * c)                       # torch's fp32 product
        twin.step()
        if not fzg:
            assert torch.equal(opt.flat_g, g)          # the clipped step leaves the gradient
            twin.flat_g.copy_(g)
        _same_state(opt, twin)
    assert R.close(float(opt.grad_norm()), float(g.double().norm()))
    per = [float(g[o:o + p.numel()].double().norm()) for p, o in zip(opt.params, opt.offsets)]
    assert all(R.close(a, b) for a, b in zip(opt.grad_norms().tolist(), per))


@KINDS
def test_below_the_threshold_the_step_is_unchanged(kind):
    g0 = _flat_grads(_make(kind, None, False, None), 0)
    max_norm = float(g0.double().norm()) * 3.0
    opt, twin = _make(kind, torch.bfloat16, False, max_norm), _make(kind, torch.bfloat16, False,
                                                                    None)
    for k in range(3):
        g = _flat_grads(opt, k)
        opt.flat_g.copy_(g)
        twin.flat_g.copy_(g)
        opt.step()
        twin.step()
        assert float(opt.clip_coef()) == 1.0
        _same_state(opt, twin)
    # measure only: never clips, whatever the norm
    opt = _make(kind, None, False, math.inf)
    opt.flat_g.copy_(g * 1e6)
    opt.step()
    assert float(opt.clip_coef()) == 1.0 and R.close(float(opt.grad_norm()),
                                                    float((g * 1e6).double().norm()))


@KINDS
@FZG
def test_identity_under_grad_scaler(kind, fzg):
    S = 256.0
    g0 = _flat_grads(_make(kind, None, False, None), 0)
    max_norm = float(g0.double().norm()) / 10.0
    opt, twin = _make(kind, torch.bfloat16, fzg, max_norm), _make(kind, torch.bfloat16, fzg, None)
    sc, sct = (GradScaler(init_scale=S, growth_interval=1000, device=DEV) for _ in range(2))
    for k in range(3):
        gs = _flat_grads(opt, k, scale=S)              # what a scaled loss leaves
        opt.flat_g.copy_(gs)
        sc.step(opt)
        sc.update()
        c = opt.clip_coef().clone()
        assert 0.05 < float(c) < 0.2
        # the norm is the unscaled gradient's
        assert R.close(float(opt.grad_norm()), float(gs.double().norm()) / S)
        twin.flat_g.copy_(gs * c)
        sct.step(twin)
        sct.update()
        if not fzg:
            twin.flat_g.copy_(gs)
        _same_state(opt, twin)
        assert torch.equal(sc.state, sct.state)
    # an overflowed step is skipped as without clipping: parameters stay, the scale backs off
    before = {n: getattr(opt, n).clone() for n in ("flat_p", "shadow") + opt._BUFFERS
              if getattr(opt, n) is not None}
    bad = _flat_grads(opt, 9, scale=S)
    bad[5] = math.inf
    opt.flat_g.copy_(bad)
    sc.step(opt)
    sc.update()
    torch.cuda.synchronize()
    for n, t in before.items():
        assert torch.equal(getattr(opt, n), t), n
    assert sc.get_scale() == S / 2 and float(opt.state[1]) == (3.0 if kind != "sgd" else 0.0)
    assert not math.isfinite(float(opt.grad_norm()))
    # and the next clean step overwrites the norm slots
    opt.flat_g.copy_(_flat_grads(opt, 10, scale=S / 2))
    sc.step(opt)
    assert math.isfinite(float(opt.grad_norm())) and 0.05 < float(opt.clip_coef()) < 0.2


def test_threshold_survives_an_old_checkpoint():
    """A state block saved without clipping has zeros in slots 4-7: loading it keeps this
    optimizer's threshold, and the unclipped optimizer loads a clipped one's block as before."""
    old, new = _make("adam", None, False, None), _make("adam", None, False, 0.5)
    old.flat_g.copy_(_flat_grads(old, 0))
    old.step()
    assert old.state[4:].tolist() == [0.0] * 4
    new.load_state_dict(old.state_dict())
    assert float(new.state[6]) == 0.5 and torch.equal(new.state[:4], old.state[:4])
    new.flat_g.copy_(_flat_grads(new, 1))
    new.step()
    assert 0.0 < float(new.clip_coef()) < 1.0
    old.load_state_dict(new.state_dict())
    assert torch.equal(old.flat_p, new.flat_p)
    with pytest.raises(RuntimeError, match="max_grad_norm"):
        old.grad_norm()


# ------------------------------------------------------------------------------- the model
def _setup(cd, kind, scaler=False, B=4, T=37, **okw):
    """The small model of tests/test_gpu_lr_graph.py with the optimizer's keywords open."""
    from models.two_transformers import Two_transformers
    from models.fc_layer import FcLayer
    from losses.loss import CCCLoss
    m = Two_transformers(0.0, 0.0, 1, 1, "TRANSFORMER", "FC", 2048)
    fc = FcLayer(1024, 512)
    init_module_(m, "")
    init_module_(fc, "fc.")
    m, fc = m.to(DEV), fc.to(DEV)
    g = torch.Generator(device=DEV).manual_seed(7)
    audio = torch.randn(B, T, 1024, device=DEV, generator=g)
    video = torch.randn(B, T, 2048, device=DEV, generator=g)
    lv = (torch.rand(B, T, device=DEV, generator=g) * 2 - 1).view(-1, B * T)
    la = (torch.rand(B, T, device=DEV, generator=g) * 2 - 1).view(-1, B * T)
    crit = CCCLoss(1)
    sc = GradScaler(init_scale=256.0, growth_interval=1000, device=DEV) if scaler else None

    def fwd_bwd():
        with JF.compute_mode(cd):
            vo, ao = m(fc(audio), video)
            loss = crit(vo.view(-1, B * T), lv) + crit(ao.view(-1, B * T), la)
            (sc.scale(loss) if sc is not None else loss).backward()
        return loss

    params = used_parameters(fwd_bwd, list(m.parameters()) + list(fc.parameters()))
    shadow = cd if cd != torch.float32 else None
    if kind == "adam":
        opt = FusedAdam(params, lr=1e-3, weight_decay=1e-4, shadow_dtype=shadow, **okw)
    else:
        opt = FusedSGD(params, lr=1e-2, momentum=0.9, dampening=0.0, weight_decay=1e-4,
                       nesterov=True, shadow_dtype=shadow, device_lr=True, **okw)

    def step():
        opt.zero_grad()
        loss = fwd_bwd()
        if sc is not None:
            sc.step(opt)
            sc.update()
        else:
            opt.step()
        return loss.detach()

    return step, opt, fwd_bwd


def test_three_sgd_steps_against_torch_float64():
    """clip_grad_norm_ + torch.optim.SGD on a float64 replica of the flat parameters, fed our
    gradients cast up.  Tolerance: the per-tensor max-abs error over max-abs value <= 1e-5 of
    tests/test_gpu_train.py::test_fused_sgd_bf16_matches_torch_sgd."""
    step, opt, fwd_bwd = _setup(torch.float32, "sgd_dev", max_grad_norm=math.inf)
    opt.zero_grad()
    fwd_bwd()
    max_norm = float(opt.flat_g.double().norm()) / 4.0     # every step clips
    opt.set_max_grad_norm(max_norm)
    P = torch.nn.Parameter(opt.flat_p.double().clone())
    ref = torch.optim.SGD([P], lr=1e-2, momentum=0.9, dampening=0.0, weight_decay=1e-4,
                          nesterov=True)
    for k in range(3):
        opt.zero_grad()
        fwd_bwd()
        P.grad = opt.flat_g.double().clone()
        tn = float(torch.nn.utils.clip_grad_norm_([P], R.f32(max_norm)))
        ref.step()
        opt.step()
        print("step", k, "norm", float(opt.grad_norm()), tn, "coef", float(opt.clip_coef()))
        assert float(opt.clip_coef()) < 1.0
        assert R.close(float(opt.grad_norm()), tn), (k, float(opt.grad_norm()), tn)
        for p, off in zip(opt.params, opt.offsets):
            a = opt.flat_p[off:off + p.numel()].double()
            b = P.detach()[off:off + p.numel()]
            err = float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
            assert err <= 1e-5, (k, off, err)


# ------------------------------------------------------------------------------- graph
def _sequence(run, opt):
    """One step measuring only, the threshold from its norm, 2 steps, the threshold doubled, 2
    steps: the same calls whether `run` steps eagerly or replays."""
    losses = []
    torch.cuda.synchronize()
    n0 = float(opt.grad_norm())
    opt.set_max_grad_norm(n0 / 10.0)
    for _ in range(2):
        losses.append(float(run()))
    opt.set_max_grad_norm(n0 / 5.0)
    for _ in range(2):
        losses.append(float(run()))
    torch.cuda.synchronize()
    return losses, n0


@pytest.mark.parametrize("cd", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["sgd_dev", "adam"])
@pytest.mark.parametrize("scaler", [False, True], ids=["plain", "scaler"])
def test_captured_clipped_step_replays_like_eager(cd, kind, scaler):
    step_e, opt_e, _ = _setup(cd, kind, scaler, max_grad_norm=math.inf)
    for _ in range(2):
        step_e()
    eager, n0e = _sequence(step_e, opt_e)

    step_g, opt_g, _ = _setup(cd, kind, scaler, max_grad_norm=math.inf)
    step_g()
    gs = GraphedStep(step_g).capture(warmup=1)
    graphed, n0g = _sequence(gs.replay, opt_g)
    assert n0e == n0g and graphed == eager, (graphed, eager)
    assert torch.equal(opt_g.flat_p, opt_e.flat_p)
    assert torch.equal(opt_g.state.view(torch.int32), opt_e.state.view(torch.int32))
    assert torch.equal(opt_g.grad_norms().view(torch.int32), opt_e.grad_norms().view(torch.int32))
    assert float(opt_g.clip_coef()) < 1.0 and float(opt_g.state[6]) == R.f32(n0g / 5.0)


@pytest.mark.parametrize("kind", ["sgd_dev", "adam"])
def test_clipping_adds_exactly_the_norm_launches(kind):
    fams = {}
    for clip in (None, 1.0):
        step, opt, _ = _setup(torch.bfloat16, kind, max_grad_norm=clip)
        step()
        rec = []

        def hook(info, launch, rec=rec):
            rec.append(info["family"])
            return launch()

        ops.set_launch_hook(hook)
        try:
            step()
        finally:
            ops.set_launch_hook(None)
        fams[clip] = rec
    base = {"sgd_dev": "sgd_step_dev", "adam": "adam_step"}[kind]
    plain, clipped = fams[None], fams[1.0]
    assert plain.count(base) == 1 and "grad_norm" not in plain and base + "_clip" not in plain
    assert clipped.count("grad_norm") == 1 and clipped.count(base + "_clip") == 1
    assert base not in clipped
    i = clipped.index("grad_norm")
    assert clipped[i + 1] == base + "_clip"            # the norm right before the step kernel
    if kind == "adam":
        assert clipped[i - 1] == "opt_tick"
    assert [f for f in clipped if f != "grad_norm"] == \
        [base + "_clip" if f == base else f for f in plain]
