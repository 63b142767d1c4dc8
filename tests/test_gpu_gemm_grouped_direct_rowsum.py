"""jmt_gemm_grouped: a problem with ONE split and a dbias table finishes its A row sums in the GEMM
kernel (csrc/gemm_persist.hip GroupSrc::epilogue: the item of column panel 0 writes dbias_tab[b0][m], the
other items store into an area nobody reads), so row sums no longer force a second split
(csrc/gemm.hip group_plan) and such a problem takes neither a slab nor a block of the reduce.

GPU shapes: 512 x 512 over K = 256 (two column panels: the second owns no row sums), 256 x 512
over K = 256 with two batch entries and the table [db, NULL], and 256 x 256 over K = 1344 (split:
its sums still go through the reduce) — in one group."""
import pytest
import torch

from jmt import _lib, ops
from tests.test_gpu_gemm_grouped import C3_SHAPES, DEV, PAD, _host_descs, _plan, _Prob


def test_plan_c3_step_group_with_row_sums_plans_as_without():
    """The c3 step's ten weight gradients with a dbias table on every problem: the split counts
    and the slab bytes are those of the same shapes without (row sums no longer force 2 splits),
    and the workspace is the slabs plus the row-sum areas — [split][b0][M] floats of a split
    problem, one 256-float tile of a one-split problem."""
    rc0, sp0, ws0 = _plan(_host_descs(C3_SHAPES))
    rc1, sp1, ws1 = _plan(_host_descs(C3_SHAPES, dbias=range(len(C3_SHAPES))))
    assert rc0 == _lib.OK and rc1 == _lib.OK
    assert sp1 == sp0, (sp1, sp0)
    assert min(sp1) == 1, "the group has one-split problems"
    slabs = sum(s * b * M * N * 4 for (M, N, K, b), s in zip(C3_SHAPES, sp1) if s > 1)
    assert ws0 == slabs, (ws0, slabs)
    areas = sum((256 if s == 1 else s * b * M) * 4 for (M, N, K, b), s in zip(C3_SHAPES, sp1))
    print(f"c3 group with row sums: splits {sp1}, slabs {slabs} B, row-sum areas {areas} B")
    assert ws1 == slabs + areas, (ws1, slabs, areas)


def _group(seed=11):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    return [_Prob(512, 512, 256, 1, 1, False, False, gen, table=False, dbias=True),
            _Prob(256, 512, 256, 1, 2, False, False, gen, table=True, dbias=True),   # [db, NULL]
            _Prob(256, 256, 1344, 1, 1, False, False, gen, table=False, dbias=True)]


def _launch(probs, acc, dbias=True, dbg=0):
    lib = _lib.load()
    for p in probs:
        p.fresh()
    descs = []
    for p in probs:
        d = p.desc()
        d.dbias_acc = acc
        if not dbias:
            d.n_dbias = 0
        descs.append(d)
    sp = [0] * len(probs)
    lib.jmt_gemm_set_debug(dbg)
    try:
        ws = ops.gemm_grouped(descs, DEV, splits_out=sp)
        torch.cuda.synchronize()
    finally:
        lib.jmt_gemm_set_debug(0)
    del ws
    return sp, [(p.C.clone(), [d.clone() if d is not None else None for d in p.db])
                for p in probs]


def _rowsum_ref(p, i):
    """float64 row sums of batch entry i's 16-bit A (MN-major storage: (K, M + PAD)) and the
    largest sum of magnitudes over its rows."""
    a = p.A[i][:, :p.M].double()
    return a.sum(0), a.abs().sum(0).max().item()


@pytest.mark.gpu
@pytest.mark.parametrize("acc", [0, 1])
def test_one_split_problems_finish_their_row_sums(acc):
    lib = _lib.load()
    probs = _group()
    sp, got = _launch(probs, acc)
    print("splits", sp)
    assert sp[0] == 1 and sp[1] == 1 and sp[2] >= 2, sp
    # C: the bits of the same group without any dbias table (guard rows / columns included),
    # within the split-K tests' bound of fp32, guards untouched
    sp_n, plain = _launch(probs, acc, dbias=False)
    assert sp_n == sp
    for i, p in enumerate(probs):
        assert torch.equal(got[i][0], plain[i][0]), (i, "C differs from the launch without dbias")
        for b in range(p.nb):
            inner = got[i][0][b, 1:p.M + 1, PAD:PAD + p.N]
            err = (inner - p.ref[b]).abs().max().item()
            print(f"p{i} b{b}: |C - ref| {err:.3e} bound {2e-3 * p.scale[b]:.3e}")
            assert err <= 2e-3 * p.scale[b], (i, b, err)
            g, g0 = got[i][0][b].clone(), p.C0[b].clone()
            g[1:p.M + 1, PAD:PAD + p.N] = 0
            g0[1:p.M + 1, PAD:PAD + p.N] = 0
            assert torch.equal(g, g0), (i, b, "C guard rows / columns written")
        # the launch without dbias left every db buffer alone
        for d, d0 in zip(plain[i][1], p.db0):
            assert d is None or torch.equal(d, d0)
    # row sums: float64 column sums of the 16-bit A, (+)= onto the random initial values
    for i, p in enumerate(probs):
        for b in range(p.nb):
            d, d0 = got[i][1][b], p.db0[b]
            if d is None:                                  # the NULL table entry
                assert i == 1 and b == 1
                continue
            ref, scale = _rowsum_ref(p, b)
            base = d0[PAD:PAD + p.M].double() if acc else 0.0
            err = (d[PAD:PAD + p.M].double() - base - ref).abs().max().item()
            bound = 1e-6 * scale + 1e-5
            print(f"p{i} b{b} acc={acc}: |rowsum - ref| {err:.3e} bound {bound:.3e}")
            assert err <= bound, (i, b, err, bound)
            assert torch.equal(d[:PAD], d0[:PAD]) and torch.equal(d[PAD + p.M:], d0[PAD + p.M:]), \
                (i, b, "dbias guard elements written")
    # the split problem alone through ops.gemm(splits=...) on the split-K ping-pong kernel
    p = probs[2]
    p.fresh()
    kw = p.kwargs()
    kw["dbias_acc"] = bool(acc)
    lib.jmt_gemm_set_debug(44 << 8)
    try:
        ops.gemm(splits=sp[2], **kw)
        torch.cuda.synchronize()
    finally:
        lib.jmt_gemm_set_debug(0)
    assert torch.equal(p.C, got[2][0]), "split problem: C differs from jmt_gemm alone"
    assert torch.equal(p.db[0], got[2][1][0]), "split problem: row sums differ from jmt_gemm alone"
    # stores drained at every wait (debug flag 32): the deadline counts change no result
    _, drained = _launch(probs, acc, dbg=32)
    for i in range(len(probs)):
        assert torch.equal(drained[i][0], got[i][0]), (i, "C changed with the stores drained")
        for a, b in zip(drained[i][1], got[i][1]):
            assert a is None or torch.equal(a, b), (i, "row sums changed with the stores drained")
