"""Stage B of the grouped weight gradients (jmt/ops.py, jmt/grouped.py): every weight gradient of
the step that jmt_gemm_grouped takes is held, with its operand tensors, until the end of the
backward pass and flushed as one group.  Held operands must not be written again, so the two
accumulating dgrads of the encoder backward write a fresh buffer and read their addend through
jmt_gemm_cin.

JMT_WGRAD_DEFER=single holds the same entries but launches what JMT_WGRAD_DEFER=0 launches, only
later: any operand overwritten before the flush shows as a bitwise difference between the two.
One forward + backward at B = 4, T = 64 (bf16, TRANSFORMER / FC) per arm, each in a fresh child
process (the switches are read at import)."""
import os
import subprocess
import sys

import pytest
import torch

from jmt import ops
from jmt._lib import BF16, F32, GemmDesc

_STEP_SCRIPT = r"""
import os, sys, torch
sys.path[:0] = [sys.argv[1], sys.argv[2]]
out, bucketer = sys.argv[3], sys.argv[4] == "1"
from jmt import functional as JF, ops
from tests.parity import build_tt
from losses.loss import CCCLoss
B, T = 4, 64
m, fc = build_tt({"H": 1, "L": 1, "jm": "TRANSFORMER", "fmt": "FC", "vin": 2048})
g = torch.Generator().manual_seed(3)
a = torch.randn(B, T, 1024, generator=g).cuda(); v = torch.randn(B, T, 2048, generator=g).cuda()
yv = (torch.rand(1, B * T, generator=g) * 2 - 1).cuda()
ya = (torch.rand(1, B * T, generator=g) * 2 - 1).cuda()
crit = CCCLoss(1)
params = list(m.parameters()) + list(fc.parameters())
launches, res = [], {}

def hook(info, launch):
    launches.append((info["family"], info.get("grouped", 1)))
    return launch()

def fwd_bwd():
    with JF.compute_mode(torch.bfloat16):
        vo, ao = m(fc(a), v)
        loss = crit(vo.reshape(1, -1), yv) + crit(ao.reshape(1, -1), ya)
        loss.backward()
    res.update(loss=loss.detach().float().cpu(), vo=vo.detach().float().cpu(),
               ao=ao.detach().float().cpu())
    return loss

if bucketer:
    import torch.distributed as dist
    from jmt import dist as jdist
    from jmt.optim import FusedSGD
    dist.init_process_group("gloo", init_method="file://" + out + ".store", rank=0, world_size=1)
    ps, counts = jdist.grad_write_profile(fwd_bwd, params)
    opt = FusedSGD(ps, lr=1e-3, momentum=0.9, weight_decay=1e-4, nesterov=True,
                   shadow_dtype=torch.bfloat16)
    bk = jdist.GradBucketer(opt, counts, bucket_bytes=1 << 20, group=dist.group.WORLD)
    opt.zero_grad()
    bk.begin()
    ops.set_launch_hook(hook)
    fwd_bwd()
    ops.set_launch_hook(None)
    bk.finish()
else:
    for p in params:
        p.grad = None
    ops.set_launch_hook(hook)
    fwd_bwd()
    ops.set_launch_hook(None)
torch.cuda.synchronize()
names = [k for k, _ in m.named_parameters()] + ["fc." + k for k, _ in fc.named_parameters()]
res["grads"] = {k: p.grad.detach().float().cpu() for k, p in zip(names, params)
                if p.grad is not None}
res["grouped"] = [n for f, n in launches if f == "gemm_TN" and n > 1]
torch.save(res, out)
"""

_cache = {}


def _child(tmp_path_factory, defer, bucketer=False):
    """The step under JMT_WGRAD_DEFER=defer ("" = unset), once per arm for the whole module."""
    key = (defer, bucketer)
    if key not in _cache:
        repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        pkg = os.path.join(repo, "joint-multimodal-transformer-6th-abaw_amd")
        out = str(tmp_path_factory.mktemp("defer") / f"step_{defer or 'on'}_{int(bucketer)}.pt")
        env = {k: v for k, v in os.environ.items() if k != "JMT_WGRAD_DEFER"}
        if defer:
            env["JMT_WGRAD_DEFER"] = defer
        r = subprocess.run([sys.executable, "-c", _STEP_SCRIPT, repo, pkg, out,
                            str(int(bucketer))], capture_output=True, text=True, timeout=240,
                           env=env)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
        _cache[key] = torch.load(out)
    return _cache[key]


@pytest.mark.gpu
def test_single_arm_is_bitwise_the_undeferred_step(tmp_path_factory):
    """single vs 0: the same launches on operands held to the end of the backward — the loss,
    both predictions and every parameter gradient are bitwise equal."""
    off, one = _child(tmp_path_factory, "0"), _child(tmp_path_factory, "single")
    for k in ("loss", "vo", "ao"):
        assert torch.equal(one[k], off[k]), k
    assert one["grads"] and one["grads"].keys() == off["grads"].keys()
    bad = [k for k, g0 in off["grads"].items() if not torch.equal(one["grads"][k], g0)]
    assert not bad, bad
    assert one["grouped"] == off["grouped"], (one["grouped"], off["grouped"])


@pytest.mark.gpu
def test_default_arm_groups_the_step_within_the_gradient_bound(tmp_path_factory):
    """default vs 0: every gradient within the floor of the strict suite's per-gradient bound
    (tests/parity.py: K_STRICT x 2u relative L2, as test_step_gradients_grouped_vs_ungrouped),
    the forward untouched, and at most two grouped TN launches in the backward."""
    from tests.parity import K_STRICT, UNIT
    off, on = _child(tmp_path_factory, "0"), _child(tmp_path_factory, "")
    for k in ("loss", "vo", "ao"):
        assert torch.equal(on[k], off[k]), k
    assert on["grads"] and on["grads"].keys() == off["grads"].keys()
    bound = K_STRICT * 2 * UNIT[torch.bfloat16]
    worst = 0.0
    for k, g0 in off["grads"].items():
        e = float((on["grads"][k] - g0).norm() / max(float(g0.norm()), 1e-30))
        worst = max(worst, e)
        assert e <= bound, (k, e, bound)
    print(f"deferred vs undeferred: worst relative gradient difference {worst:.3e} "
          f"(bound {bound:.3e}); grouped launches {on['grouped']} (undeferred {off['grouped']})")
    assert 1 <= len(on["grouped"]) <= 2, on["grouped"]


@pytest.mark.gpu
def test_bucketer_defers_nothing(tmp_path_factory):
    """With a GradBucketer installed (gloo, world 1) the gradients complete in the profiled
    order: default vs 0 is bitwise equal and nothing is grouped."""
    off, on = _child(tmp_path_factory, "0", True), _child(tmp_path_factory, "", True)
    assert not on["grouped"] and not off["grouped"]
    assert on["grads"] and on["grads"].keys() == off["grads"].keys()
    for k, g0 in off["grads"].items():
        assert torch.equal(on["grads"][k], g0), k


# ------------------------------------------------------------------------------ host only
def _entry(c, db=None, M=256, N=256, K=1024):
    """A queued weight gradient on never dereferenced pointers (the partition is a host function)."""
    fake = 0x10000
    d = GemmDesc()
    d.ab_dtype, d.c_dtype, d.aux_dtype = BF16, F32, F32
    d.M, d.N, d.K = M, N, K
    d.batch0 = d.batch1 = 1
    d.alpha = d.beta = 1.0
    d.lda, d.ldb, d.ldc = M, N, N
    d.a[0], d.b[0], d.c[0] = fake, fake, c
    d.n_a = d.n_b = d.n_c = 1
    if db is not None:
        d.dbias_tab[0], d.n_dbias, d.dbias_acc = db, 1, 1
    return ops._WgradEntry(d, {}, None, None, (), "dev", stream="stream")


def test_overlapping_outputs_never_share_a_launch():
    """Two problems of one grouped launch read-modify-write their outputs concurrently: an entry
    whose C range (or dbias range) overlaps an earlier entry's lands in a later launch."""
    X, Y, Z, W = 0x100000, 0x200000, 0x300000, 0x400000
    DB = 0x500000
    e1, e2, e3, e4 = _entry(X, db=DB), _entry(Y), _entry(X), _entry(Z)
    e5 = _entry(Y + 256 * 255 * 4)          # the last row of e2's C range
    e6 = _entry(W, db=DB + 255 * 4)         # the last element of e1's dbias range
    e7 = _entry(Z + 256 * 256 * 4)          # right behind e4's range: no overlap
    groups, rest = ops.wgrad_partition([e1, e2, e3, e4, e5, e6, e7])
    assert not rest
    assert groups == [[e1, e2, e4, e7], [e3, e5, e6]], \
        [[[e1, e2, e3, e4, e5, e6, e7].index(e) + 1 for e in g] for g in groups]
    # a third write of the same rows goes one launch further, alone -> through jmt_gemm, last
    e8 = _entry(X)
    groups, rest = ops.wgrad_partition([e1, e2, e3, e4, e5, e8])
    assert groups == [[e1, e2, e4], [e3, e5]] and rest == [e8]
