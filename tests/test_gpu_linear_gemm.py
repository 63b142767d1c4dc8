"""jmt/linear_gemm.py: the one fwd / dgrad / wgrad / bias_grad of every linear layer, per operand
form, against float64 torch products; frozen parameters in a batched launch and in the whole
model; and that a weight-gradient launch keeps the tensors its operands live in.

Tolerance: tests/test_gpu_kernels.py's _tol (2e-4 sqrt(K) for 16-bit operands, 2e-5 sqrt(K) for
fp32, times the reference's largest magnitude), K the reduction length of the product.  Outputs
are fp32 buffers, so no output rounding enters."""
import math
import os
import subprocess
import sys

import pytest
import torch

from jmt import linear_gemm as lg
from jmt import ops
from jmt._lib import BF16, F32

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROWS, N, KIN = 128, 128, 64
BF = torch.bfloat16


def _tol(dt, K):        # tests/test_gpu_kernels.py
    return 2e-5 * math.sqrt(max(K, 1)) if dt == F32 else 2e-4 * math.sqrt(max(K, 1))


def _close(got, ref, dt, K, what):
    err = (got.double() - ref).abs().max().item()
    assert err <= _tol(dt, K) * max(1.0, ref.abs().max().item()), (what, err)


def _rand(gen, *shape, dtype=BF):
    return torch.randn(*shape, device=DEV, generator=gen).to(dtype)


def _params(gen, G, n=N, kin=KIN):
    """G weights / biases whose fp32 values are bf16 numbers (their 16-bit copies are exact)."""
    Ws = [torch.nn.Parameter(_rand(gen, n, kin).float()) for _ in range(G)]
    bs = [torch.nn.Parameter(_rand(gen, n).float()) for _ in range(G)]
    return Ws, bs


class _Keeps:
    """Wraps ops.gemm: the `keep` of every call that passes `done`."""

    def __enter__(self):
        self.orig, self.keeps = ops.gemm, []

        def gemm(**kw):
            if kw.get("done") is not None:
                self.keeps.append(kw.get("keep", ()))
            return self.orig(**kw)

        ops.gemm = gemm
        return self

    def __exit__(self, *a):
        ops.gemm = self.orig

    def covers(self, *operands):
        assert len(self.keeps) == 1
        held = {t.untyped_storage().data_ptr() for t in self.keeps[0] if t is not None}
        for op in operands:
            for t in op.owners:
                assert t.untyped_storage().data_ptr() in held


def _batched(form, gen):
    """(A, dY, X2, Y2, dX2 operands; X, dY as lists of float64 matrices) for G = 3 problems."""
    G = 3
    if form == "strided":
        X, dY = _rand(gen, G, ROWS, KIN), _rand(gen, G, ROWS, N)
        Y = torch.zeros(G, ROWS, N, device=DEV)
        dX = torch.zeros(G, ROWS, KIN, device=DEV)
        sd = lambda t: lg.strided(t, t.shape[-1], ROWS * t.shape[-1])
        return sd(X), sd(dY), sd(Y), sd(dX), list(X), list(dY), list(Y), list(dX)
    X = [_rand(gen, ROWS, KIN) for _ in range(G)]
    dY = [_rand(gen, ROWS + 8, N)[8:] for _ in range(G)]          # views at an offset
    Y = [torch.zeros(ROWS, N, device=DEV) for _ in range(G)]
    dX = [torch.zeros(ROWS, KIN, device=DEV) for _ in range(G)]
    return (lg.table(X, KIN), lg.table(dY, N), lg.table(Y, N), lg.table(dX, KIN), X, dY, Y, dX)


@pytest.mark.parametrize("form", ["strided", "table"])
def test_batched_forms(form):
    gen = torch.Generator(device=DEV).manual_seed(1)
    Ws, bs = _params(gen, 3)
    A, dYo, Yo, dXo, X, dY, Y, dX = _batched(form, gen)
    lg.fwd(A, ROWS, Ws, bs, Yo, BF)
    lg.dgrad(dYo, ROWS, N, Ws, dXo, BF)
    with _Keeps() as k:
        assert lg.wgrad(dYo, A, ROWS, N, Ws, BF, bs) is True
    k.covers(dYo, A)
    torch.cuda.synchronize()
    for g in range(3):
        W, b = Ws[g].detach().double(), bs[g].detach().double()
        _close(Y[g], X[g].double() @ W.T + b, BF16, KIN, ("fwd", g))
        _close(dX[g], dY[g].double() @ W, BF16, N, ("dgrad", g))
        _close(Ws[g].grad, dY[g].double().T @ X[g].double(), BF16, ROWS, ("wgrad", g))
        _close(bs[g].grad, dY[g].double().sum(0), BF16, ROWS, ("bgrad", g))


def test_kcat_forward_two_segments():
    """A concatenated forward (K = 2 segments), its per-segment dgrad and its weight gradient:
    one parameter whose columns are cut into two batch entries that share dY."""
    gen = torch.Generator(device=DEV).manual_seed(2)
    (W,), (b,) = _params(gen, 1, N, 2 * KIN)
    X = [_rand(gen, ROWS, KIN) for _ in range(2)]
    dY = _rand(gen, ROWS, N)
    Y = torch.zeros(ROWS, N, device=DEV)
    dX = [torch.zeros(ROWS, KIN, device=DEV) for _ in range(2)]
    lg.fwd(lg.kcat(X, KIN, KIN), ROWS, W, b, lg.strided(Y, N), BF)
    lg.dgrad(lg.strided(dY, N), ROWS, N, W, lg.table(dX, KIN), BF, kseg=KIN)
    with _Keeps() as k:
        assert lg.wgrad(lg.strided(dY, N), lg.table(X, KIN), ROWS, N, W, BF, b, kseg=KIN) is True
    k.covers(lg.strided(dY, N), lg.table(X, KIN))
    torch.cuda.synchronize()
    Wd, Xc = W.detach().double(), torch.cat(X, 1).double()
    _close(Y, Xc @ Wd.T + b.detach().double(), BF16, 2 * KIN, "fwd")
    _close(torch.cat(dX, 1), dY.double() @ Wd, BF16, N, "dgrad")
    _close(W.grad, dY.double().T @ Xc, BF16, ROWS, "wgrad")
    _close(b.grad, dY.double().sum(0), BF16, ROWS, "bgrad")


def _ksegs(gen, G=2, seg=64):
    dY = [[_rand(gen, seg, N) for _ in range(2)] for _ in range(G)]
    X = [[_rand(gen, seg, KIN) for _ in range(2)] for _ in range(G)]
    refW = [sum(d.double().T @ x.double() for d, x in zip(dY[g], X[g])) for g in range(G)]
    refb = [sum(d.double().sum(0) for d in dY[g]) for g in range(G)]
    return lg.ksegs(dY, N, seg), lg.ksegs(X, KIN, seg), refW, refb


def test_ksegs_wgrad_two_segments_of_64_rows():
    gen = torch.Generator(device=DEV).manual_seed(3)
    Ws, bs = _params(gen, 2)
    dYo, Xo, refW, refb = _ksegs(gen)
    with _Keeps() as k:
        assert lg.wgrad(dYo, Xo, 64, N, Ws, BF, bs) is True
    k.covers(dYo, Xo)
    torch.cuda.synchronize()
    for g in range(2):
        _close(Ws[g].grad, refW[g], BF16, 128, ("wgrad", g))
        _close(bs[g].grad, refb[g], BF16, 128, ("bgrad", g))


@pytest.mark.parametrize("cd", [torch.float32, BF])
def test_single_output_column(cd):
    """n = 1 (rows 100, K-in 128): dY is a column, read with the operand flipped; the bias
    gradient takes the column sum."""
    dt = F32 if cd == torch.float32 else BF16
    rows, kin = 100, 128
    gen = torch.Generator(device=DEV).manual_seed(4)
    (W,), (b,) = _params(gen, 1, 1, kin)
    X, dY = _rand(gen, rows, kin, dtype=cd), _rand(gen, rows, 1, dtype=cd)
    Y = torch.zeros(rows, 1, device=DEV)
    dX = torch.zeros(rows, kin, device=DEV)
    lg.fwd(lg.strided(X, kin), rows, W, b, lg.strided(Y, 1), cd)
    lg.dgrad(lg.strided(dY, 1), rows, 1, W, lg.strided(dX, kin), cd)
    assert lg.wgrad(lg.strided(dY, 1), lg.strided(X, kin), rows, 1, W, cd, b) is False
    torch.cuda.synchronize()
    Wd = W.detach().double()
    _close(Y, X.double() @ Wd.T + b.detach().double(), dt, kin, "fwd")
    _close(dX, dY.double() @ Wd, dt, 1, "dgrad")
    _close(W.grad, dY.double().T @ X.double(), dt, rows, "wgrad")
    _close(b.grad, dY.double().sum(0), dt, rows, "bgrad")


@pytest.mark.parametrize("form", ["strided", "ksegs"])
@pytest.mark.parametrize("variant", ["unfused", "none_entry", "frozen"])
def test_bias_variants(form, variant):
    """JMT_FUSED_BGRAD off (the column-sum fallback); a None bias entry; a frozen W and a frozen
    b in a batched launch: the other entries are unaffected, a frozen one's .grad stays None."""
    gen = torch.Generator(device=DEV).manual_seed(5)
    G = 3 if form == "strided" else 2
    Ws, bs = _params(gen, G)
    if form == "strided":
        A, dYo, _, _, X, dY, _, _ = _batched("strided", gen)
        rows = ROWS
        refW = [dY[g].double().T @ X[g].double() for g in range(G)]
        refb = [dY[g].double().sum(0) for g in range(G)]
    else:
        dYo, A, refW, refb = _ksegs(gen)
        rows = 64
    bl = list(bs)
    if variant == "none_entry":
        bl[1] = None
    if variant == "frozen":
        Ws[0].requires_grad_(False)
        bs[1].requires_grad_(False)
    prev = lg._fused_bgrad["on"]
    lg._fused_bgrad["on"] = variant != "unfused"
    try:
        fused = lg.wgrad(dYo, A, rows, N, Ws, BF, bl)
    finally:
        lg._fused_bgrad["on"] = prev
    torch.cuda.synchronize()
    assert fused is (variant != "unfused")
    for g in range(G):
        if variant == "frozen" and g == 0:
            assert Ws[g].grad is None
        else:
            _close(Ws[g].grad, refW[g], BF16, 128, ("wgrad", g))
        if variant in ("none_entry", "frozen") and g == 1:
            assert bs[g].grad is None
        else:
            _close(bs[g].grad, refb[g], BF16, 128, ("bgrad", g))


# ------------------------------------------------------------------------- frozen, whole model
FROZEN = ("mm_transformer.physiological_encoder.layers.0.feed_forward.0.bias",
          "mm_transformer.cross_attention_p.in_proj_weight",
          "mm_transformer.out_layer1.bias", "vregressor.3.weight")

_FROZEN_SCRIPT = r"""
import sys, torch
sys.path[:0] = [sys.argv[1], sys.argv[2]]
from jmt import functional as JF
from tests.parity import build_tt
from losses.loss import CCCLoss
frozen = sys.argv[4:]
B, T = 4, 64
g = torch.Generator().manual_seed(3)
a = torch.randn(B, T, 1024, generator=g).cuda(); v = torch.randn(B, T, 2048, generator=g).cuda()
yv = (torch.rand(1, B * T, generator=g) * 2 - 1).cuda()
ya = (torch.rand(1, B * T, generator=g) * 2 - 1).cuda()
crit = CCCLoss(1)
res = {}
for arm in ("all", "frozen"):
    m, fc = build_tt({"H": 1, "L": 1, "jm": "TRANSFORMER", "fmt": "FC", "vin": 2048})
    named = list(m.named_parameters()) + [("fc." + k, p) for k, p in fc.named_parameters()]
    if arm == "frozen":
        for k, p in named:
            if k in frozen:
                p.requires_grad_(False)
    with JF.compute_mode(torch.bfloat16):
        vo, ao = m(fc(a), v)
        loss = crit(vo.reshape(1, -1), yv) + crit(ao.reshape(1, -1), ya)
        loss.backward()
    torch.cuda.synchronize()
    res[arm] = {k: None if p.grad is None else p.grad.detach().cpu() for k, p in named}
torch.save(res, sys.argv[3])
"""


def test_frozen_parameters_leave_the_other_gradients_bitwise(tmp_path):
    """TRANSFORMER / FC, bf16, (B, T) = (4, 64) with JMT_WGRAD_GROUP=0 JMT_FUSED_BGRAD=0 (every
    launch's plan depends on its own shape only): with FROZEN frozen, every other parameter's
    gradient is bitwise the unfrozen run's, and the frozen ones have none.  (Holds on the commit
    before jmt/linear_gemm.py too: no parameter needs an exception.)"""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(repo, "joint-multimodal-transformer-6th-abaw_amd")
    out = str(tmp_path / "frozen.pt")
    env = dict(os.environ, JMT_WGRAD_GROUP="0", JMT_FUSED_BGRAD="0")
    r = subprocess.run([sys.executable, "-c", _FROZEN_SCRIPT, repo, pkg, out, *FROZEN],
                       capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    res = torch.load(out)
    assert set(FROZEN) <= set(res["all"])
    bad = []
    for k, g0 in res["all"].items():
        g1 = res["frozen"][k]
        if k in FROZEN:
            assert g0 is not None and g1 is None, k
        elif (g0 is None) != (g1 is None) or (g0 is not None and not torch.equal(g0, g1)):
            bad.append(k)
    assert not bad, bad
