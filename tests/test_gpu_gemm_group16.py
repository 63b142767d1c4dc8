"""jmt_gemm_group16: several forward / input-gradient problems with 16-bit C as the tiles of one
ping-pong launch (csrc/gemm_persist.hip Group16Src / gemm_group16_kernel, csrc/gemm.hip
group16_plan).

Every output of a grouped launch must have the bits of the same problem run alone through
jmt_gemm forced onto the ping-pong kernel (cfg 45), and of the same launch with debug flag 32
(the epilogue's stores are not counted, every deadline drains them).  The shapes are the smallest
at which each mechanism can go wrong: one and two tiles per row panel, an odd K-tile count
(K = 320), 64-deep K-concat segments (a segment boundary at every K-tile of an item's stream),
per-batch K-concat, pointer tables, strided batches, bias tables with an absent entry; and three
grids: fewer items than blocks, three blocks walking four or five items each across the
problems' boundaries (different ld, K and K-segments on the two sides), and exactly one round.

float64 bound (per element, from the number formats): the operands are exact in 16 bits, the
fp32 accumulation of K products and the bias is off by at most K 2^-24 S, S = |alpha| |A| |B| +
|bias| (K 2^-23 S asked: the MFMA's internal order is not IEEE's), and the round-to-nearest
16-bit store adds the unit roundoff u |x|, u = 2^-8 (bf16: 8 significant bits) / 2^-11 (fp16).
The single launch is held to the same bound first, and the group then has its bits."""
import ctypes as C

import pytest
import torch

from jmt import _lib, ops
from jmt._lib import BF16, F16, F32, GemmDesc

DEV = "cuda"
PAD = 8          # guard columns / extra leading dimension (elements; 16 B)
TDT = {BF16: torch.bfloat16, F16: torch.float16}
UOUT = {BF16: 2.0 ** -8, F16: 2.0 ** -11}


class _Op:
    """A (or B): nb logical (rows x K) matrices.  mode 0: equally spaced in one buffer; 1: a
    pointer per entry; 2: ONE matrix as K / kseg segments; 3: every entry as K / kseg segments.
    Every piece has a leading dimension larger than its row."""

    def __init__(self, rows, K, nb, mode, kseg, kmajor, dtype, gen):
        self.mode, self.kseg = mode, kseg if mode >= 2 else 0
        seg = kseg if mode >= 2 else K
        nseg = K // seg
        ne = 1 if mode == 2 else nb
        if kmajor:
            buf = torch.randn(ne * nseg, rows, seg + PAD, device=DEV, generator=gen).to(dtype)
            pieces = [buf[i, :, :seg] for i in range(ne * nseg)]
            self.ld, self.stride = seg + PAD, rows * (seg + PAD)
        else:
            buf = torch.randn(ne * nseg, seg, rows + PAD, device=DEV, generator=gen).to(dtype)
            pieces = [buf[i, :, :rows].t() for i in range(ne * nseg)]
            self.ld, self.stride = rows + PAD, seg * (rows + PAD)
        self.buf = buf
        es = buf.element_size()
        base = buf.data_ptr()
        ptrs = [base + i * self.stride * es for i in range(ne * nseg)]
        self.ptrs = ptrs[:1] if mode == 0 else ptrs
        # entry g's logical matrix in float64 (mode 2: the same for every entry)
        self.logical = [torch.cat([pieces[(0 if mode == 2 else g) * nseg + s].double()
                                   for s in range(nseg)], dim=1) for g in range(nb)]


class _Prob:
    def __init__(self, M, N, K, nb, amode, akseg, bmode, bkseg, bias, ak, bk, dt, gen,
                 alpha=1.0, ctable=False):
        dtype = TDT[dt]
        self.M, self.N, self.K, self.nb, self.ak, self.bk, self.dt = M, N, K, nb, ak, bk, dt
        self.alpha, self.ctable = alpha, ctable
        self.A = _Op(M, K, nb, amode, akseg, ak, dtype, gen)
        self.B = _Op(N, K, nb, bmode, bkseg, bk, dtype, gen)
        self.ldc = N + 2 * PAD
        self.C0 = torch.randn(nb, M + 2, self.ldc, device=DEV, generator=gen).to(dtype)
        # bias: None, "one" vector, "tab" per entry, "absent": a table whose odd entries are NULL
        self.bias_kind = bias
        nbv = 0 if bias is None else 1 if bias == "one" else nb
        self.bias = [torch.randn(N, device=DEV, generator=gen) for _ in range(nbv)]
        self.zero = torch.zeros(N, device=DEV)
        self.ref, self.tol = [], []
        for g in range(nb):
            a, b = self.A.logical[g], self.B.logical[g]
            bv = self._bias_of(g)
            bv = bv.double() if bv is not None else torch.zeros(N, device=DEV, dtype=torch.float64)
            r = alpha * (a @ b.t()) + bv
            s = abs(alpha) * (a.abs() @ b.abs().t()) + bv.abs()
            self.ref.append(r)
            self.tol.append(UOUT[dt] * r.abs() + K * 2.0 ** -23 * s)
        self.fresh()

    def _bias_of(self, g):
        if self.bias_kind is None:
            return None
        if self.bias_kind == "one":
            return self.bias[0]
        if self.bias_kind == "absent" and g % 2 == 1:
            return None
        return self.bias[g]

    def fresh(self):
        self.C = self.C0.clone()

    def cptrs(self):
        es = self.C.element_size()
        p0 = self.C.data_ptr() + (self.ldc + PAD) * es
        st = (self.M + 2) * self.ldc
        return [p0 + g * st * es for g in range(self.nb)], st

    def desc(self):
        d = GemmDesc()
        d.ab_dtype = d.c_dtype = d.aux_dtype = self.dt
        d.M, d.N, d.K = self.M, self.N, self.K
        d.batch0, d.batch1 = self.nb, 1
        d.alpha, d.beta = self.alpha, 0.0
        d.a_kmajor, d.b_kmajor = int(self.ak), int(self.bk)
        for name, op in (("a", self.A), ("b", self.B)):
            for i, p in enumerate(op.ptrs):
                getattr(d, name)[i] = p
            setattr(d, "n_" + name, len(op.ptrs))
            setattr(d, name + "_mode", op.mode)
            setattr(d, name + "_kseg", op.kseg)
            setattr(d, "ld" + name, op.ld)
            setattr(d, "s" + name.upper() + "0", op.stride if op.mode == 0 else 0)
        cp, st = self.cptrs()
        d.ldc = self.ldc
        if self.ctable:
            for i, p in enumerate(cp):
                d.c[i] = p
            d.n_c, d.c_mode = self.nb, 1
        else:
            d.c[0], d.n_c, d.c_mode, d.sC0 = cp[0], 1, 0, st
        if self.bias_kind == "one":
            d.bias, d.bias_mode = self.bias[0].data_ptr(), 1
        elif self.bias_kind is not None:
            for g in range(self.nb):
                t = self._bias_of(g)
                d.bias_tab[g] = t.data_ptr() if t is not None else None
            d.n_bias, d.bias_mode = self.nb, 1
        return d

    def single(self):
        """The same problem alone through ops.gemm (the caller forces cfg 45); an absent bias
        entry is a vector of zeros there (alpha * acc + 0 either way)."""
        cp, st = self.cptrs()
        kw = dict(M=self.M, N=self.N, K=self.K, ab_dtype=self.dt, c_dtype=self.dt,
                  a=self.A.ptrs, lda=self.A.ld, a_kmajor=self.ak, a_mode=self.A.mode,
                  a_kseg=self.A.kseg, sA=(self.A.stride if self.A.mode == 0 else 0, 0),
                  b=self.B.ptrs, ldb=self.B.ld, b_kmajor=self.bk, b_mode=self.B.mode,
                  b_kseg=self.B.kseg, sB=(self.B.stride if self.B.mode == 0 else 0, 0),
                  ldc=self.ldc, batch0=self.nb, alpha=self.alpha, splits=1, device=DEV)
        if self.ctable:
            kw.update(c=cp, c_mode=1)
        else:
            kw.update(c=cp[:1], sC=(st, 0))
        if self.bias_kind == "one":
            kw.update(bias=self.bias[0])
        elif self.bias_kind is not None:
            kw.update(bias_tab=[self._bias_of(g) if self._bias_of(g) is not None else self.zero
                                for g in range(self.nb)])
        ops.gemm(**kw)

    def region(self, C=None):
        C = self.C if C is None else C
        return C[:, 1:self.M + 1, PAD:PAD + self.N]

    def check(self, tag):
        got = self.region().double()
        worst = 0.0
        for g in range(self.nb):
            err = (got[g] - self.ref[g]).abs()
            ratio = (err / self.tol[g]).max().item()
            worst = max(worst, ratio)
            assert ratio <= 1.0, (tag, g, err.max().item(), ratio)
        c, c0 = self.C.clone(), self.C0.clone()
        self.region(c).zero_()
        self.region(c0).zero_()
        assert torch.equal(c, c0), (tag, "C guard rows / columns written")
        return worst


def _mixed(ak, bk, dt, seed=5):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    kw = dict(ak=ak, bk=bk, dt=dt, gen=gen)
    return [_Prob(512, 256, 320, 2, 1, 0, 1, 0, "absent", ctable=True, **kw),
            _Prob(256, 512, 512, 1, 2, 64, 2, 256, None, **kw),
            _Prob(256, 256, 256, 3, 3, 128, 0, 0, "one", **kw),
            _Prob(512, 512, 320, 1, 0, 0, 2, 64, "tab", alpha=0.5, **kw)]


def _run(probs, dbg=0, grid=0):
    lib = _lib.load()
    for p in probs:
        p.fresh()
    lib.jmt_gemm_set_debug(dbg)
    lib.jmt_gemm_group16_set_grid(grid)
    try:
        ops.gemm_group16([p.desc() for p in probs])
        torch.cuda.synchronize()
    finally:
        lib.jmt_gemm_set_debug(0)
        lib.jmt_gemm_group16_set_grid(0)


def _singles(probs):
    lib = _lib.load()
    out = []
    for p in probs:
        p.fresh()
        lib.jmt_gemm_set_debug(45 << 8)
        try:
            desc = p.desc()
            desc.splits = 1
            assert lib.jmt_gemm_persist_cfg(C.byref(desc)) == 45
            p.single()
            torch.cuda.synchronize()
        finally:
            lib.jmt_gemm_set_debug(0)
        out.append(p.C.clone())
    return out


def _compare(probs, tag, grids):
    alone = _singles(probs)
    for i, p in enumerate(probs):
        w = p.check(f"{tag} alone p{i}")
        print(f"{tag} p{i}: alone, worst error / float64 bound {w:.3f}")
    for grid in grids:
        for dbg in (0, 32):
            _run(probs, dbg, grid)
            for i, p in enumerate(probs):
                assert torch.equal(p.C, alone[i]), \
                    (tag, f"grid {grid} dbg {dbg}: problem {i} differs from jmt_gemm alone")
                w = p.check(f"{tag} grid {grid} dbg {dbg} p{i}")
            print(f"{tag}: grid {grid} dbg {dbg} bit-identical, last worst / bound {w:.3f}")


LAYOUTS = [(True, True), (True, False)]          # NT (forward), NN (input gradient)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("ak,bk", LAYOUTS)
def test_mixed_group_bit_identical(ak, bk, dt):
    """Four problems (13 items) that differ in M, N, K, batch count, operand modes, leading
    dimensions, bias and alpha: with one block per item (fewer items than CUs) and with three
    blocks that walk four or five items each across the problems' boundaries."""
    probs = _mixed(ak, bk, dt)
    assert sum((p.M // 256) * (p.N // 256) * p.nb for p in probs) == 13
    _compare(probs, f"mixed[{ak},{bk},{dt}]", (0, 3))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("ak,bk", LAYOUTS)
def test_exactly_one_round(ak, bk, dt):
    """Two strided-batch problems whose items are exactly one per block of the persistent grid
    (the CU count rounded down to a multiple of 8)."""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count & ~7
    gen = torch.Generator(device=DEV).manual_seed(6)
    kw = dict(ak=ak, bk=bk, dt=dt, gen=gen)
    n1 = ncu // 2
    n2 = (ncu - n1) // 2
    probs = [_Prob(256, 256, 256, n1, 0, 0, 0, 0, "one", **kw),
             _Prob(256, 512, 320, n2, 0, 0, 0, 0, None, **kw)]
    assert n1 + 2 * n2 == ncu
    _compare(probs, f"one round[{ak},{bk},{dt}]", (0,))


@pytest.mark.gpu
def test_refusals_write_nothing():
    """Every refusal of include/jmt.h on a real group: the documented code, before any launch —
    every C buffer keeps its bytes."""
    lib = _lib.load()
    probs = _mixed(True, True, BF16)
    U, A = _lib.ERR_UNSUPPORTED, _lib.ERR_ARG

    def rc_of(mut, n=None):
        for p in probs:
            p.fresh()
        ds = [p.desc() for p in probs]
        ds = mut(ds) or ds
        arr = (GemmDesc * len(ds))(*ds)
        n = len(ds) if n is None else n
        rc_ok = lib.jmt_gemm_group16_ok(arr, n)
        rc = lib.jmt_gemm_group16(arr, n, ops.stream())
        torch.cuda.synchronize()
        assert rc == rc_ok
        if rc != _lib.OK:
            for p in probs:
                assert torch.equal(p.C, p.C0), "a refused group wrote C"
        return rc

    def st(i, **kw):
        def f(ds):
            for k, v in kw.items():
                setattr(ds[i], k, v)
        return f

    def ptr(i, name, k, v):
        def f(ds):
            getattr(ds[i], name)[k] = v
        return f

    def many(ds):
        out = []
        for j in range(8):
            d = probs[0].desc()
            for name in "abc":
                for k in range(8):
                    getattr(d, name)[k] = getattr(d, name)[0]
                setattr(d, "n_" + name, 8)
            d.n_bias, d.bias, d.bias_mode = 0, probs[3].bias[0].data_ptr(), 1
            out.append(d)
        return out

    fb = probs[2].bias[0].data_ptr()
    assert rc_of(st(1, ab_dtype=F32, c_dtype=F32)) == U
    assert rc_of(st(0, c_dtype=F32)) == U
    assert rc_of(st(2, ab_dtype=F16, c_dtype=F16)) == U                   # mixed dtype
    assert rc_of(st(1, b_kmajor=0)) == U                                  # mixed layout
    assert rc_of(lambda ds: (setattr(ds[0], "n_dbias", 2), ds[0].dbias_tab.__setitem__(0, fb),
                             ds[0].dbias_tab.__setitem__(1, fb)) and None) == U   # row sums
    assert rc_of(st(3, splits=2)) == U
    assert rc_of(st(0, M=384)) == U                                       # partial row panel
    assert rc_of(st(2, bias_mode=2)) == U                                 # bias per row
    assert rc_of(st(1, relu=1)) == U                                      # mixed EPI
    assert rc_of(st(3, beta=1.0)) == U
    assert rc_of(many) == U                                               # pointer pool
    assert b"table pointers" in lib.jmt_last_error()
    assert rc_of(ptr(0, "a", 1, None)) == A
    assert rc_of(ptr(1, "b", 0, probs[1].B.ptrs[0] + 2)) == A
    assert rc_of(ptr(0, "c", 0, None)) == A
    assert rc_of(st(0, n_b=1)) == A                                       # short table
    assert rc_of(st(1, n_a=4)) == A                                       # short K-concat table
    assert rc_of(st(2, n_a=5)) == A
    assert rc_of(lambda ds: ds[1].c.__setitem__(0, ds[3].c[0])) == A      # overlapping C
    assert b"overlap" in lib.jmt_last_error()
    assert rc_of(lambda ds: None) == _lib.OK                              # the group itself runs
    assert not any(torch.equal(p.C, p.C0) for p in probs)
