"""jmt_gemm_grouped: several weight-gradient problems of different shapes, leading dimensions and
pointer tables as the items of one split-K ping-pong launch and one reduce launch
(csrc/gemm_persist.hip gemm_group_kernel / group_reduce_kernel, csrc/gemm.hip group_plan), and
the weight-gradient queue of jmt.ops that feeds it from the training step.

The shapes are the smallest at which each mechanism can go wrong: a single tile, a pointer-table
batch, per-batch K-segments whose split ranges start inside a segment, a problem short enough to
take one split and write C directly, and more items than CUs (the second round of the walk),
with problems of one shape and with a second item of another shape than the first."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

from jmt import _lib, ops
from jmt._lib import BF16, F32, GemmDesc

DEV = "cuda"
PAD = 8          # guard columns / extra leading dimension (elements)


def _desc(M, N, K, batch0=1, **kw):
    d = GemmDesc()
    d.ab_dtype, d.c_dtype, d.aux_dtype = BF16, F32, F32
    d.M, d.N, d.K = M, N, K
    d.batch0, d.batch1 = batch0, 1
    d.alpha, d.beta = 1.0, 1.0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


# ------------------------------------------------------------------------------ host only
C3_SHAPES = [(1024, 512, 19200, 6), (512, 512, 38400, 3), (512, 512, 38400, 3),
             (1024, 512, 38400, 3), (512, 512, 19200, 6), (512, 512, 19200, 3),
             (1536, 512, 19200, 3), (512, 512, 19200, 2), (512, 2048, 19200, 1),
             (512, 1024, 19200, 1)]


def _host_descs(shapes, dbias=()):
    """Descriptors with aligned, never dereferenced pointers (the planner is a host function)."""
    fake = 0x10000
    out = []
    for i, (M, N, K, b) in enumerate(shapes):
        d = _desc(M, N, K, b, lda=M, ldb=N, ldc=N, a_mode=1, b_mode=1, c_mode=1)
        for j in range(b):
            d.a[j] = d.b[j] = d.c[j] = fake
        d.n_a = d.n_b = d.n_c = b
        if i in dbias:
            for j in range(b):
                d.dbias_tab[j] = fake
            d.n_dbias = b
        out.append(d)
    return out


def _plan(descs):
    lib = _lib.load()
    n = len(descs)
    arr = (GemmDesc * n)(*descs)
    sp = (C.c_int * n)()
    rc = lib.jmt_gemm_grouped_plan(arr, n, sp)
    return rc, list(sp), int(lib.jmt_gemm_grouped_workspace_bytes(arr, n))


def test_plan_splits_slabs_and_workspace():
    """Every problem gets >= 1 split of >= 4 K-tiles (>= 2 splits with row sums); the slabs and
    the row-sum partials the kernel addresses ([split][b0][M][N] per split problem, then
    [split][b0][M] per problem) are disjoint by construction when the workspace holds exactly
    their sum — which jmt_gemm_grouped_workspace_bytes must report."""
    shapes = [(256, 256, 1344, 1), (512, 256, 640, 2), (256, 512, 4480, 1), (512, 512, 256, 1)]
    for dbias in ((), (1, 2)):
        rc, sp, ws = _plan(_host_descs(shapes, dbias))
        assert rc == _lib.OK
        need = 0
        for i, ((M, N, K, b), s) in enumerate(zip(shapes, sp)):
            assert s >= (2 if i in dbias else 1) and (K // 64) // s >= 4, (shapes[i], s)
            need += s * b * M * N * 4 if s > 1 else 0
            need += s * b * M * 4 if dbias else 0
        assert sp[3] == 1, "a 4 K-tile problem writes C directly"
        assert ws == need, (ws, need)
    # a forced count is kept (normalised as jmt_gemm does)
    ds = _host_descs([(512, 512, 2048, 1)] * 2)
    ds[0].splits = 8
    assert _plan(ds)[1][0] == 8


def test_plan_c3_step_group_fills_rounds_with_fewer_slab_bytes():
    """The c3 step's ten 256-multiple weight gradients as ONE group: the items fill whole rounds
    of the persistent grid (256 blocks without a device) to at least 90 % — a partial last round
    idles its CUs for a whole item, the padding bound jmt_gemm's planner uses for a tile — and
    the slabs are fewer bytes than those of today's ten separate plans (jmt_gemm_plan_splits)."""
    lib = _lib.load()
    rc, sp, ws = _plan(_host_descs(C3_SHAPES))
    assert rc == _lib.OK
    G = 256
    items = sum((M // 256) * (N // 256) * b * s for (M, N, K, b), s in zip(C3_SHAPES, sp))
    rounds = -(-items // G)
    assert items >= 0.9 * rounds * G, (items, rounds, sp)
    today = 0
    for (M, N, K, b) in C3_SHAPES:
        s = lib.jmt_gemm_plan_splits(BF16, M, N, K, b)
        today += lib.jmt_gemm_workspace_bytes(M, N, b, s)
    print(f"c3 group: splits {sp}, {items} items, slab bytes {ws} vs {today} separately")
    assert ws < today, (ws, today)


def test_unsupported_descriptors_are_refused():
    lib = _lib.load()
    base = [(512, 256, 1024, 1), (256, 256, 2048, 1)]

    def rc_of(mut):
        ds = _host_descs(base)
        mut(ds)
        return _plan(ds)[0]

    assert rc_of(lambda ds: None) == _lib.OK
    U = _lib.ERR_UNSUPPORTED
    assert rc_of(lambda ds: setattr(ds[1], "ab_dtype", F32)) == U
    assert rc_of(lambda ds: setattr(ds[0], "M", 384)) == U
    assert rc_of(lambda ds: setattr(ds[0], "N", 128)) == U
    assert rc_of(lambda ds: setattr(ds[1], "K", 2000)) == U
    assert rc_of(lambda ds: setattr(ds[1], "relu", 1)) == U
    assert rc_of(lambda ds: setattr(ds[0], "bias", 0x10000)) == U
    assert rc_of(lambda ds: setattr(ds[0], "aux", 0x10000)) == U
    assert rc_of(lambda ds: setattr(ds[1], "c_dtype", BF16)) == U
    assert rc_of(lambda ds: setattr(ds[1], "b_kmajor", 1)) == U
    assert rc_of(lambda ds: setattr(ds[0], "a_mode", 2)) == U
    assert b"jmt_gemm_grouped" in lib.jmt_last_error()
    arr = (GemmDesc * 2)(*_host_descs(base))
    assert lib.jmt_gemm_grouped(arr, 17, None, 0, None) == _lib.ERR_ARG
    assert lib.jmt_gemm_grouped(arr, 2, None, 0, None) == _lib.ERR_ARG   # no workspace
    assert b"workspace bytes" in lib.jmt_last_error()


# ------------------------------------------------------------------------------ GPU
def _operand(rows, K, kmajor, gen, nbuf=1):
    """nbuf logical (rows x K) bf16 operands with a leading dimension larger than the row.
    Returns (storages, logical fp32 matrices, ld)."""
    st, lg = [], []
    for _ in range(nbuf):
        if kmajor:
            s = torch.randn(rows, K + PAD, device=DEV, generator=gen).to(torch.bfloat16)
            l = s[:, :K].float()
        else:
            s = torch.randn(K, rows + PAD, device=DEV, generator=gen).to(torch.bfloat16)
            l = s[:, :rows].float().t()
        st.append(s)
        lg.append(l)
    return st, lg, (K if kmajor else rows) + PAD


class _Prob:
    """One problem of the mixed group: operands, guarded C / dbias buffers, fp32 reference."""

    def __init__(self, M, N, kseg, nseg, nb, ak, bk, gen, table, dbias, splits=0):
        self.M, self.N, self.K, self.nb, self.ak, self.bk = M, N, kseg * nseg, nb, ak, bk
        self.kseg, self.nseg, self.table, self.splits = kseg, nseg, table, splits
        self.A, Al, self.lda = _operand(M, kseg, ak, gen, nb * nseg)
        self.B, Bl, self.ldb = _operand(N, kseg, bk, gen, nb * nseg)
        self.ldc = N + 2 * PAD
        # guard rows above / below and PAD guard columns left / right of every C
        self.C0 = torch.randn(nb, M + 2, self.ldc, device=DEV, generator=gen)
        self.db0 = [torch.randn(M + 2 * PAD, device=DEV, generator=gen) if dbias and
                    (i == 0 or not table) else None for i in range(nb)] if dbias else None
        self.ref, self.scale, self.rref, self.rscale = [], [], [], []
        for i in range(nb):
            ss = range(i * nseg, (i + 1) * nseg)
            self.ref.append(self.C0[i, 1:M + 1, PAD:PAD + N] + sum(Al[s] @ Bl[s].t() for s in ss))
            self.scale.append(sum((Al[s].abs() @ Bl[s].abs().t()).max().item() for s in ss))
            self.rref.append(sum(Al[s].sum(1) for s in ss))
            self.rscale.append(sum(Al[s].abs().sum(1) for s in ss).max().item())
        self.fresh()

    def fresh(self):
        self.C = self.C0.clone()
        self.db = [d.clone() if d is not None else None for d in self.db0] if self.db0 else None

    def kwargs(self):
        nb, nseg = self.nb, self.nseg
        cp = [self.C[i, 1:, PAD:].data_ptr() for i in range(nb)]
        kw = dict(M=self.M, N=self.N, K=self.K, ab_dtype=BF16, c_dtype=F32,
                  a=[t.data_ptr() for t in self.A], lda=self.lda, a_kmajor=self.ak,
                  b=[t.data_ptr() for t in self.B], ldb=self.ldb, b_kmajor=self.bk,
                  ldc=self.ldc, batch0=nb, beta=1.0, device=DEV)
        if nseg > 1:
            kw.update(a_mode=3, b_mode=3, a_kseg=self.kseg, b_kseg=self.kseg)
        elif self.table:
            kw.update(a_mode=1, b_mode=1)
        if self.table:
            kw.update(c=cp, c_mode=1)
        else:
            assert nb == 1
            kw.update(c=cp[:1])
        if self.db:
            kw.update(dbias_tab=[d[PAD:PAD + self.M] if d is not None else None for d in self.db],
                      dbias_acc=True)
        return kw

    def desc(self):
        kw = self.kwargs()
        d = _desc(self.M, self.N, self.K, self.nb, lda=self.lda, ldb=self.ldb, ldc=self.ldc,
                  a_kmajor=int(self.ak), b_kmajor=int(self.bk), a_mode=kw.get("a_mode", 0),
                  b_mode=kw.get("b_mode", 0), c_mode=kw.get("c_mode", 0),
                  a_kseg=kw.get("a_kseg", 0), b_kseg=kw.get("b_kseg", 0), splits=self.splits)
        for name, ptrs in (("a", kw["a"]), ("b", kw["b"]), ("c", kw["c"])):
            for i, p in enumerate(ptrs):
                getattr(d, name)[i] = p
        d.n_a, d.n_b, d.n_c = len(kw["a"]), len(kw["b"]), len(kw["c"])
        if self.db:
            for i, t in enumerate(kw["dbias_tab"]):
                d.dbias_tab[i] = t.data_ptr() if t is not None else None
            d.n_dbias, d.dbias_acc = self.nb, 1
        return d

    def check(self, tag):
        M, N = self.M, self.N
        for i in range(self.nb):
            got = self.C[i, 1:M + 1, PAD:PAD + N]
            err = (got - self.ref[i]).abs().max().item()
            print(f"{tag} b{i}: |C - ref| {err:.3e} bound {2e-3 * self.scale[i]:.3e}")
            assert err <= 2e-3 * self.scale[i], (tag, i, err)
            g, g0 = self.C[i].clone(), self.C0[i].clone()
            g[1:M + 1, PAD:PAD + N] = 0
            g0[1:M + 1, PAD:PAD + N] = 0
            assert torch.equal(g, g0), (tag, i, "C guard rows / columns written")
            if self.db and self.db[i] is not None:
                d, d0 = self.db[i], self.db0[i]
                rerr = (d[PAD:PAD + M] - d0[PAD:PAD + M] - self.rref[i]).abs().max().item()
                print(f"{tag} b{i}: |rowsum - ref| {rerr:.3e} bound "
                      f"{1e-6 * self.rscale[i] + 1e-5:.3e}")
                assert rerr <= 1e-6 * self.rscale[i] + 1e-5, (tag, i, rerr)
                assert torch.equal(d[:PAD], d0[:PAD]) and torch.equal(d[PAD + M:], d0[PAD + M:])


def _mixed_group(ak, bk, seed=7):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    rs = not ak and not bk
    return [_Prob(256, 256, 1344, 1, 1, ak, bk, gen, table=False, dbias=False),
            _Prob(512, 256, 640, 1, 2, ak, bk, gen, table=True, dbias=rs),     # [db, NULL]
            _Prob(256, 512, 2240, 2, 1, ak, bk, gen, table=True, dbias=rs),
            _Prob(512, 512, 256, 1, 1, ak, bk, gen, table=False, dbias=False)]


def _run_group(probs, dbg=0):
    lib = _lib.load()
    for p in probs:
        p.fresh()
    sp = [0] * len(probs)
    lib.jmt_gemm_set_debug(dbg)
    try:
        ws = ops.gemm_grouped([p.desc() for p in probs], DEV, splits_out=sp)
        torch.cuda.synchronize()
    finally:
        lib.jmt_gemm_set_debug(0)
    del ws
    return sp


@pytest.mark.gpu
@pytest.mark.parametrize("ak,bk", [(False, False), (True, True), (True, False), (False, True)])
def test_mixed_group_vs_fp32_and_bit_identity(ak, bk):
    """Four problems in one call (different lda / ldb / ldc, each larger than its row; beta = 1
    onto random C; TN with row sums on two problems, one table entry NULL) against fp32 with the
    split-K tests' bounds, guard rows / columns untouched; then each problem alone through
    ops.gemm(splits=splits_p) under cfg 44: C and the row sums bit-identical; and the group
    again with debug flag 32 (stores drained at every wait): bit-identical."""
    lib = _lib.load()
    probs = _mixed_group(ak, bk)
    sp = _run_group(probs)
    print("splits", sp)
    assert sp[3] == 1 and min(sp[:3]) >= 2
    # the mode-3 problem: a split range starts inside a K-segment
    nkt, seg = probs[2].K // 64, probs[2].kseg // 64
    assert any((s * nkt // sp[2]) % seg for s in range(sp[2]))
    for i, p in enumerate(probs):
        p.check(f"grouped[{ak},{bk}] p{i}")
    got = [(p.C.clone(), [d.clone() if d is not None else None for d in p.db] if p.db else None)
           for p in probs]
    for i, p in enumerate(probs):
        p.fresh()
        lib.jmt_gemm_set_debug(44 << 8)
        try:
            ops.gemm(splits=sp[i], **p.kwargs())
            torch.cuda.synchronize()
        finally:
            lib.jmt_gemm_set_debug(0)
        assert torch.equal(p.C, got[i][0]), (i, "C differs from jmt_gemm alone")
        if p.db:
            for a, b in zip(p.db, got[i][1]):
                assert a is None or torch.equal(a, b), (i, "row sums differ from jmt_gemm alone")
    _run_group(probs, dbg=32)
    for i, p in enumerate(probs):
        assert torch.equal(p.C, got[i][0]), (i, "C changed with the stores drained")
        if p.db:
            for a, b in zip(p.db, got[i][1]):
                assert a is None or torch.equal(a, b)


@pytest.mark.gpu
def test_more_items_than_cus():
    """Nine 512 x 512 x 2048 problems forced to 8 splits: 288 items, so blocks walk a second
    item (of another problem) on any grid."""
    gen = torch.Generator(device=DEV).manual_seed(9)
    probs = [_Prob(512, 512, 2048, 1, 1, False, False, gen, table=False, dbias=(i % 2 == 0),
                   splits=8) for i in range(9)]
    sp = _run_group(probs)
    assert sp == [8] * 9
    for i, p in enumerate(probs):
        p.check(f"nine p{i}")


@pytest.mark.gpu
@pytest.mark.parametrize("ak,bk", [(False, False), (True, True), (True, False), (False, True)])
def test_second_item_of_another_shape_bit_identical(ak, bk):
    """The schedule's stream crossing from one problem shape to another inside a block, for every
    layout.  Two shapes alternate: 256 x 512 over K = 1024 as two 512-row segments per batch entry
    (a_mode = b_mode = 3), forced to 4 splits of 4 K-tiles, so splits 1 and 3 begin inside a
    segment; and 512 x 256 over K = 512, forced to 2 splits.  No knob shrinks the grid, so the
    launch must hold more items than CUs, as in test_more_items_than_cus.  One entry of each shape
    is 8 + 4 items, and a call takes 16 problems at most (128 items), so each problem has three
    batch entries instead: 8 x (24 + 12) = 288 items.  A grid of 256 gives each XCD 36 consecutive
    logical items — one pair of problems — and a block's second item lies 32 items behind its
    first: in the pair's 512 x 256 problem when the first is one of the first four of the
    256 x 512 one.  Each problem's C (and, TN, the row sums) must have the bits of
    ops.gemm(splits=...) on it alone under cfg 44, the comparison of
    test_mixed_group_vs_fp32_and_bit_identity."""
    lib = _lib.load()
    gen = torch.Generator(device=DEV).manual_seed(11)
    rs = not ak and not bk
    probs = []
    for i in range(8):
        probs.append(_Prob(256, 512, 512, 2, 3, ak, bk, gen, table=True, dbias=rs and i < 4,
                           splits=4))
        probs.append(_Prob(512, 256, 512, 1, 3, ak, bk, gen, table=True, dbias=False, splits=2))
    sp = _run_group(probs)
    assert sp == [4, 2] * 8
    items = sum((p.M // 256) * (p.N // 256) * p.nb * s for p, s in zip(probs, sp))
    assert items == 288
    for i, p in enumerate(probs):
        p.check(f"two shapes[{ak},{bk}] p{i}")
    got = [(p.C.clone(), [d.clone() if d is not None else None for d in p.db] if p.db else None)
           for p in probs]
    for i, p in enumerate(probs):
        p.fresh()
        lib.jmt_gemm_set_debug(44 << 8)
        try:
            ops.gemm(splits=sp[i], **p.kwargs())
            torch.cuda.synchronize()
        finally:
            lib.jmt_gemm_set_debug(0)
        assert torch.equal(p.C, got[i][0]), (i, "C differs from jmt_gemm alone")
        if p.db:
            for a, b in zip(p.db, got[i][1]):
                assert a is None or torch.equal(a, b), (i, "row sums differ from jmt_gemm alone")


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
fams = []

def fwd_bwd():
    with JF.compute_mode(torch.bfloat16):
        vo, ao = m(fc(a), v)
        loss = crit(vo.reshape(1, -1), yv) + crit(ao.reshape(1, -1), ya)
        loss.backward()
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
    ops.set_launch_hook(lambda info, launch: (fams.append(info.get("grouped", 1)), launch())[1])
    fwd_bwd()
    ops.set_launch_hook(None)
    bk.finish()
else:
    for p in params:
        p.grad = None
    ops.set_launch_hook(lambda info, launch: (fams.append(info.get("grouped", 1)), launch())[1])
    fwd_bwd()
    ops.set_launch_hook(None)
torch.cuda.synchronize()
names = [k for k, _ in m.named_parameters()] + ["fc." + k for k, _ in fc.named_parameters()]
torch.save({"grads": {k: p.grad.detach().float().cpu() for k, p in zip(names, params)
                      if p.grad is not None},
            "grouped": [n for n in fams if n > 1]}, out)
"""


def _step_child(tmp_path, group, bucketer):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(repo, "joint-multimodal-transformer-6th-abaw_amd")
    out = str(tmp_path / f"grads_g{group}_b{int(bucketer)}.pt")
    r = subprocess.run([sys.executable, "-c", _STEP_SCRIPT, repo, pkg, out, str(int(bucketer))],
                       capture_output=True, text=True, timeout=240,
                       env=dict(os.environ, JMT_WGRAD_GROUP=str(group)))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return torch.load(out)


@pytest.mark.gpu
def test_step_gradients_grouped_vs_ungrouped(tmp_path):
    """One forward + backward at B = 4, T = 64 (bf16, TRANSFORMER / FC) with JMT_WGRAD_GROUP 1
    and 0 in fresh child processes.  The grouped run must issue grouped launches, and every
    parameter gradient must agree within the floor of the strict suite's per-gradient bound
    (tests/parity.py: K_STRICT x 2u relative L2; the suite's bound is never below it)."""
    from tests.parity import K_STRICT, UNIT
    on, off = _step_child(tmp_path, 1, False), _step_child(tmp_path, 0, False)
    assert on["grouped"] and not off["grouped"], (on["grouped"], off["grouped"])
    assert on["grads"] and on["grads"].keys() == off["grads"].keys()
    bound = K_STRICT * 2 * UNIT[torch.bfloat16]
    worst = 0.0
    for k, g0 in off["grads"].items():
        e = float((on["grads"][k] - g0).norm() / max(float(g0.norm()), 1e-30))
        worst = max(worst, e)
        assert e <= bound, (k, e, bound)
    print(f"grouped vs ungrouped: worst relative gradient difference {worst:.3e} (bound {bound:.3e})")


@pytest.mark.gpu
def test_step_gradients_with_bucketer_are_bit_identical(tmp_path):
    """With a GradBucketer installed (gloo, world 1) the gradients complete in the profiled
    order: nothing is grouped, and the gradients have today's bits whatever JMT_WGRAD_GROUP says."""
    on, off = _step_child(tmp_path, 1, True), _step_child(tmp_path, 0, True)
    assert not on["grouped"] and not off["grouped"]
    assert on["grads"] and on["grads"].keys() == off["grads"].keys()
    for k, g0 in off["grads"].items():
        assert torch.equal(on["grads"][k], g0), k
