"""The two places of the cross-attention block that hand independent GEMMs to one
jmt_gemm_group16 launch (jmt/grouped.py CrossAttention6Fn through lg.group16_scope): the query
and key / value in-projections of the forward, and the three per-stream input gradients of the
backward.

A grouped launch replaces launches only where it keeps their bits: ops.group16_scope groups when
every problem alone would run unsplit on the ping-pong kernel (jmt_gemm_persist_cfg == 45).  At
the test's B = 2, T = 128 (256 rows) the planner gives the five problems other kernels and a
split K, so the first case pins the single launches where c3 has them — cfg 45 forced, split
counts 1, in both arms — and compares switch on against switch off; the second case leaves the
planner alone and checks that the group is then refused and the parent's launches run."""
import pytest
import torch

from jmt import _lib, functional as JF, grouped, ops
from jmt.grouped import CROSS_PAIRS

DEV = "cuda"
E, H = 512, 1
CD = torch.bfloat16


def _modules(seed=31):
    g = torch.Generator(device="cpu").manual_seed(seed)
    mods = []
    for _ in range(1 + max(m for m, _, _ in CROSS_PAIRS)):
        m = torch.nn.MultiheadAttention(E, H)
        with torch.no_grad():
            m.in_proj_weight.copy_(torch.randn(3 * E, E, generator=g) * E ** -0.5)
            m.in_proj_bias.copy_(torch.randn(3 * E, generator=g) * 0.1)
            m.out_proj.weight.copy_(torch.randn(E, E, generator=g) * E ** -0.5)
            m.out_proj.bias.copy_(torch.randn(E, generator=g) * 0.1)
        mods.append(m.to(DEV))
    return mods


def _inputs(B, T, seed=32):
    g = torch.Generator(device="cpu").manual_seed(seed)
    Y = torch.randn(3, B, T, E, generator=g).to(DEV, CD)
    dO6 = torch.randn(len(CROSS_PAIRS), B, T, E, generator=g).to(DEV, CD)
    return Y, dO6


def _kernel_names(fn):
    """(result of fn, names of the device kernels it launched — None if the profiler saw none)"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return out, names or None


def _step(mods, Y0, dO6, on, pin):
    """One forward + backward; returns (tensors to compare, launch records, kernel names)."""
    lib = _lib.load()
    for m in mods:
        for p in m.parameters():
            p.grad = None
    Y = Y0.clone().requires_grad_(True)
    rec = []
    auto = ops.auto_splits
    ops._group16["on"] = on
    if pin:
        lib.jmt_gemm_set_debug(45 << 8)
        ops.auto_splits = lambda *a: 1
    ops.set_launch_hook(lambda info, launch: (rec.append(dict(info)), launch())[1])

    def run():
        with JF.compute_mode(CD):
            O6 = grouped.cross_attention6(Y, mods, H, CROSS_PAIRS)
            O6.backward(dO6)
        return O6

    try:
        O6, names = _kernel_names(run)
    finally:
        ops.set_launch_hook(None)
        ops.auto_splits = auto
        ops._group16["on"] = True
        lib.jmt_gemm_set_debug(0)
    out = [O6.detach().clone(), Y.grad.detach().clone()]
    for m in mods:
        out += [p.grad.detach().clone() for p in m.parameters()]
    return out, rec, names


def _gemms(rec, fam):
    """the 16-bit-C launches of one family, as (grouped count or 1, N, K)"""
    return [(r.get("grouped", 1), r["N"], r["K"]) for r in rec
            if r["family"] == fam and r.get("c_dtype") != _lib.F32]


@pytest.mark.gpu
def test_grouped_launches_replace_five_and_keep_the_bits():
    """B = 2, T = 128 with the single launches pinned to the ping-pong kernel: switch on, one
    grouped launch stands where the query and key / value projections were (NT) and one where the
    three stream gradients were (NN) — the launch records and the profiler's kernel names say
    so — and the outputs, the input gradient and every parameter gradient are bitwise equal."""
    mods = _modules()
    Y, dO6 = _inputs(2, 128)
    _step(mods, Y, dO6, on=False, pin=True)            # (the weights' 16-bit copies are cast once)
    off, rec0, names0 = _step(mods, Y, dO6, on=False, pin=True)
    on, rec1, names1 = _step(mods, Y, dO6, on=True, pin=True)
    for a, b in zip(on, off):
        assert torch.equal(a, b)
    nt0, nt1 = _gemms(rec0, "gemm_NT"), _gemms(rec1, "gemm_NT")
    nn0, nn1 = _gemms(rec0, "gemm_NN"), _gemms(rec1, "gemm_NN")
    assert all(g == 1 for g, _, _ in nt0 + nn0)
    # forward: (q, N = E) + (k|v, N = 2E) -> one record of two problems, the first one's shape
    assert [x for x in nt1 if x[0] > 1] == [(2, E, E)]
    assert len(nt1) == len(nt0) - 1
    # backward: three K-concatenated stream gradients -> one record of three problems
    grp = [x for x in nn1 if x[0] > 1]
    assert len(grp) == 1 and grp[0][0] == 3 and grp[0][1] == E and grp[0][2] % E == 0
    assert len(nn1) == len(nn0) - 2
    f0 = sum(r["flops"] for r in rec0 if r["family"] in ("gemm_NT", "gemm_NN"))
    f1 = sum(r["flops"] for r in rec1 if r["family"] in ("gemm_NT", "gemm_NN"))
    assert f0 == f1, "the grouped records must carry the summed work"
    if names0 is not None and names1 is not None:
        n16 = [n for n in names1 if "gemm_group16_kernel" in n]
        assert len(n16) == 2 and not any("gemm_group16_kernel" in n for n in names0)
        pp = lambda names: sum("gemm_pp2_kernel" in n for n in names)
        assert pp(names0) - pp(names1) == 5, (pp(names0), pp(names1))
        assert len(names0) - len(names1) == 3


@pytest.mark.gpu
@pytest.mark.parametrize("B,T", [(2, 128), (2, 77)])
def test_refused_group_runs_the_parents_launches(B, T):
    """With the planner left alone: at 256 rows the five problems are not ping-pong launches
    (few tiles, split K), at 154 rows no whole row panel exists — either way the scope launches
    what the switch-off arm launches, in its order, and the results are equal."""
    mods = _modules()
    Y, dO6 = _inputs(B, T)
    _step(mods, Y, dO6, on=False, pin=False)           # (the weights' 16-bit copies are cast once)
    off, rec0, names0 = _step(mods, Y, dO6, on=False, pin=False)
    on, rec1, names1 = _step(mods, Y, dO6, on=True, pin=False)
    for a, b in zip(on, off):
        assert torch.equal(a, b)
    key = lambda r: (r["family"], r.get("M"), r.get("N"), r.get("K"), r.get("batch"),
                     r.get("grouped", 1))
    assert [key(r) for r in rec1] == [key(r) for r in rec0]
    assert not any(r.get("grouped") for r in rec1 if r.get("c_dtype", _lib.F32) != _lib.F32)
    if names0 is not None and names1 is not None:
        assert sorted(names1) == sorted(names0)
        assert not any("gemm_group16_kernel" in n for n in names1)


@pytest.mark.gpu
def test_captured_graph_replays_equal_eager():
    """The forward's grouped projection launch inside a captured graph: two replays give the
    eager result (the launch holds no workspace and no host state)."""
    lib = _lib.load()
    mods = _modules()
    Y, _ = _inputs(2, 128)
    auto = ops.auto_splits
    lib.jmt_gemm_set_debug(45 << 8)
    ops.auto_splits = lambda *a: 1
    rec = []
    try:
        with torch.no_grad(), JF.compute_mode(CD):
            ops.set_launch_hook(lambda info, launch: (rec.append(dict(info)), launch())[1])
            eager = grouped.cross_attention6(Y, mods, H, CROSS_PAIRS).clone()
            ops.set_launch_hook(None)
            torch.cuda.synchronize()
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                grouped.cross_attention6(Y, mods, H, CROSS_PAIRS)      # warm-up off the capture
            torch.cuda.current_stream().wait_stream(s)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = grouped.cross_attention6(Y, mods, H, CROSS_PAIRS)
            for _ in range(2):
                out.zero_()
                graph.replay()
                torch.cuda.synchronize()
                assert torch.equal(out, eager)
    finally:
        ops.set_launch_hook(None)
        ops.auto_splits = auto
        lib.jmt_gemm_set_debug(0)
    assert any(r.get("grouped") == 2 for r in rec), "the eager run did not take the grouped launch"
