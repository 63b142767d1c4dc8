"""jmt_attn_mh_{fwd,bwd} (csrc/attn_mh.hip): the fused multi-head attention kernels for head dims
64 (H = 8) and 128 (H = 4) at E = 512, bf16 and fp16, at the kernel level.

The shapes straddle every tile size of the kernels (16 rows per wave, 32-row MFMA chunks, 64-row
items and LDS tiles) by +-1 and end on (70, 70, 40, 8): 320 (n, h) pairs, more blocks than CUs.
o, lse, dq, dk, dv against a float64 reference from the same rounded inputs (Delta from the
kernel's 16-bit O) under the bounds of tests/test_gpu_attn_short.py, and against the error of the
GEMM + softmax path of the same build on the same inputs: the fused path's error may not exceed
that path's error times FWD_MARGIN (o) / BWD_MARGIN (dq, dk, dv); where that path's error is
below what fp32 summation can leave in dq / dk when dS cancels exactly (attn_mh_ref.fp32_residue:
with one key the GEMM path returns an exact 0), that residue is the bound instead.  The GEMM path
keeps no lse, so lse has its absolute bound only.  DESIGN.md section 4 records the measured errors
and reasons about BWD_MARGIN."""
import math

import pytest
import torch

from jmt import ops
from jmt._lib import JMTError
from tests import attn_mh_ref as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
E = 512

SHAPES = [(1, 1, 1, 8), (9, 17, 5, 8), (33, 31, 3, 8), (64, 64, 2, 4), (65, 129, 2, 8),
          (129, 65, 3, 4), (128, 300, 1, 4), (300, 300, 2, 8), (70, 70, 40, 8)]
CDS = [torch.bfloat16, torch.float16]
FWD_MARGIN = 1.5     # a different fp32 summation order
# Both paths multiply P / dS rounded to 16 bits and accumulate in fp32, so their errors are two
# draws of the same rounding noise; the maximum of one draw over a few thousand elements exceeds
# the other's by well under 2 x (DESIGN.md section 4 lists the measured ratios).
BWD_MARGIN = 2.0

_cache = {}


def _case(cd, shape):
    """Everything the tests of one (dtype, shape) share, computed once and left unchanged."""
    key = (cd, shape)
    if key not in _cache:
        Lq, Lk, N, H = shape
        qkv, kv, go = M.inputs(cd, Lq, Lk, N)
        o, lse = M.fwd(qkv, kv, H)
        dq, dk, dv, delta = M.bwd(qkv, kv, go, o, lse, H)
        got = dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv)
        ref = M.ref64(qkv, kv, go, H, o=o)
        _cache[key] = dict(qkv=qkv, kv=kv, go=go, got=got, delta=delta, ref=ref)
    return _cache[key]


@pytest.mark.parametrize("cd", CDS, ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mh_vs_float64(cd, shape):
    c = _case(cd, shape)
    H = shape[3]
    assert not torch.isnan(c["got"]["lse"]).any() and not torch.isnan(c["got"]["o"].float()).any()
    M.check_bounds(cd, c["qkv"], c["kv"], c["got"], c["ref"], H, what=f"{shape}")
    # the Delta workspace: rowsum(dO o O) of the 16-bit O, laid out like lse
    Lq, N = c["qkv"].shape[:2]
    d = (c["go"].double() * c["got"]["o"].double()).reshape(Lq, N, H, E // H).sum(-1)
    d = d.permute(1, 2, 0).reshape(-1)
    assert (c["delta"].double() - d).abs().max().item() <= 1e-5 * max(d.abs().max().item(), 1.0)


@pytest.mark.parametrize("cd", CDS, ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mh_error_not_above_gemm_path(cd, shape):
    c = _case(cd, shape)
    H = shape[3]
    g = M.gemm_path(cd, c["qkv"], c["kv"], c["go"], H)
    # the GEMM path takes Delta = rowsum(P o dP), not the 16-bit O: its reference is all float64
    gref = M.ref64(c["qkv"], c["kv"], c["go"], H)
    eg = M.errors(g, gref)
    em = M.errors({n: c["got"][n] for n in g}, c["ref"])
    res = M.fp32_residue(c["ref"], c["qkv"], c["kv"], H)
    for n in ("o", "dq", "dk", "dv"):
        margin = FWD_MARGIN if n == "o" else BWD_MARGIN
        print(f"{shape} {n}: mh {em[n]:.3e} gemm {eg[n]:.3e} ratio "
              f"{em[n] / max(eg[n], 1e-30):.3f} (margin {margin}, fp32 residue {res[n]:.1e})")
    for n in ("o", "dq", "dk", "dv"):
        margin = FWD_MARGIN if n == "o" else BWD_MARGIN
        assert em[n] <= max(margin * eg[n], res[n]), (n, em[n], eg[n], res[n])


@pytest.mark.parametrize("cd", CDS, ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", [(65, 129, 2, 8), (70, 70, 40, 8), (129, 65, 3, 4)],
                         ids=lambda s: "x".join(map(str, s)))
def test_mh_backward_is_deterministic(cd, shape):
    c = _case(cd, shape)
    H = shape[3]
    o, lse = M.fwd(c["qkv"], c["kv"], H)
    assert torch.equal(o, c["got"]["o"]) and torch.equal(lse, c["got"]["lse"])
    dq, dk, dv, _ = M.bwd(c["qkv"], c["kv"], c["go"], o, lse, H)
    for a, n in ((dq, "dq"), (dk, "dk"), (dv, "dv")):
        assert torch.equal(a, c["got"][n]), n


def test_mh_heads_permute_bit_for_bit():
    """H = 8: permuting the 64-column head blocks of q / k / v / dO permutes the head blocks of
    every output bit for bit (a head's result depends on its own columns only)."""
    cd, (Lq, Lk, N, H) = torch.bfloat16, (65, 129, 2, 8)
    c = _case(cd, (Lq, Lk, N, H))
    perm = torch.tensor([3, 0, 7, 1, 6, 2, 5, 4], device=DEV)
    cols = (perm[:, None] * 64 + torch.arange(64, device=DEV)[None]).reshape(-1)

    def pblocks(t, nblk):                      # permute the heads inside each E-wide slot
        parts = [t[..., i * E:(i + 1) * E][..., cols] for i in range(nblk)]
        return torch.cat(parts, -1)

    qkv2 = pblocks(c["qkv"], 3).permute(1, 0, 2).contiguous().permute(1, 0, 2)
    kv2 = pblocks(c["kv"], 2).permute(1, 0, 2).contiguous().permute(1, 0, 2)
    go2 = pblocks(c["go"], 1).contiguous()
    o2, lse2 = M.fwd(qkv2, kv2, H)
    dq2, dk2, dv2, _ = M.bwd(qkv2, kv2, go2, o2, lse2, H)
    g = c["got"]
    assert torch.equal(o2, g["o"][..., cols])
    assert torch.equal(lse2.view(N, H, Lq), g["lse"].view(N, H, Lq)[:, perm])
    assert torch.equal(dq2, g["dq"][..., cols])
    assert torch.equal(dk2, g["dk"][..., cols])
    assert torch.equal(dv2, g["dv"][..., cols])


def test_mh_nothing_to_do_and_unsupported():
    cd = torch.bfloat16
    qkv, kv, go = M.inputs(cd, 8, 8, 2)
    lse = torch.empty(2 * 8 * 8, device=DEV)
    o = torch.full((8, 2, E), 7.0, device=DEV, dtype=cd)
    fams = []
    ops.set_launch_hook(lambda info, launch: (fams.append(info.get("family")), launch())[1])
    try:
        a = lambda t, c0=0: (t[..., c0:].data_ptr(), M.st(t))
        # N = 0 and Lq = 0: JMT_OK, nothing written
        ops.attn_mh_fwd(ops.dt(qkv), 0, 8, 8, 8, 64, *a(qkv), *a(kv), *a(kv, E), *a(o), 0.125, lse)
        ops.attn_mh_fwd(ops.dt(qkv), 2, 8, 0, 8, 64, *a(qkv), *a(kv), *a(kv, E), *a(o), 0.125, lse)
        ops.attn_mh_bwd(ops.dt(qkv), 0, 8, 8, 8, 64, *a(go), *a(o), *a(qkv), *a(kv), *a(kv, E),
                        lse, *a(qkv), *a(kv), *a(kv, E), 0.125, lse)
        torch.cuda.synchronize()
        assert (o == 7.0).all()
        # head dim 256 (num_heads = 2): no fused kernel
        with pytest.raises(JMTError, match="jmt_attn_mh_ok"):
            ops.attn_mh_fwd(ops.dt(qkv), 2, 2, 8, 8, 256, *a(qkv), *a(kv), *a(kv, E), *a(o),
                            1.0 / math.sqrt(256), lse)
        with pytest.raises(JMTError, match="jmt_attn_mh_ok"):
            ops.attn_mh_bwd(ops.dt(qkv), 2, 2, 8, 8, 256, *a(go), *a(o), *a(qkv), *a(kv),
                            *a(kv, E), lse, *a(qkv), *a(kv), *a(kv, E), 1.0 / math.sqrt(256), lse)
    finally:
        ops.set_launch_hook(None)
    assert not ops.attn_mh_ok(ops.dt(qkv), 256, 2, 2, 8, 8, 1536, 1024, 1024)
    assert ops.attn_mh_ok(ops.dt(qkv), 64, 2, 8, 8, 8, 1536, 1024, 1024)
