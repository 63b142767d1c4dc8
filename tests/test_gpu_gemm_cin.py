"""jmt_gemm_cin: jmt_gemm with the epilogue's beta * C operand read from another buffer (a table
parallel to C with its own leading dimension), so that an accumulating input gradient leaves its
addend intact for a weight gradient that reads it later (csrc/gemm.hip gemm_epilogue,
csrc/gemm_persist.hip persist_epilogue).

Only a load address changes, so every case asks for bits: C equals the in-place launch on a C
preloaded with c_in's contents, c_in is unchanged, and C's guard rows / columns are untouched
(ldc != ldcin, both larger than N).  The shapes are the smallest that reach each epilogue form:
one ragged 128 x 128 tile pair (both store forms of the one-block kernel), two batch entries of
full 256 x 256 tiles on the persistent kernel (with and without the ReLU mask), and a partial last
row panel on the ping-pong kernel."""
import ctypes as C

import pytest
import torch

from jmt import _lib, ops
from jmt._lib import BF16, F16, F32, GemmDesc

DEV = "cuda"
PAD = 8
DT = {torch.bfloat16: BF16, torch.float16: F16}


class _Case:
    """dX = alpha * A . B + beta * c_in (A K-major, B MN-major: the dgrad layout), nb batch
    entries at one batch stride sC for C, c_in and the mask.  C and the mask hold rows of ldc
    elements from one guard row and PAD guard columns into each entry's block, c_in rows of
    ldcin elements from PAD elements into it."""

    def __init__(self, M, N, K, nb, dtype, aux, seed):
        g = torch.Generator(device=DEV).manual_seed(seed)
        rnd = lambda *s: torch.randn(*s, device=DEV, generator=g).to(dtype)
        self.M, self.N, self.K, self.nb, self.dtype = M, N, K, nb, dtype
        self.lda, self.ldb = K + PAD, N + PAD
        self.A, self.B = rnd(nb, M, self.lda), rnd(nb, K, self.ldb)
        self.ldc, self.ldcin = N + 2 * PAD, N + 4 * PAD
        self.sC = (M + 2) * self.ldcin             # holds (M + 2) rows of either kind
        self.C0 = rnd(nb * self.sC)
        self.cin = rnd(nb * self.sC)
        self.aux = rnd(nb * self.sC) if aux else None

    def c_view(self, buf, b):                      # the M x N block of batch entry b (C / mask)
        v = buf[b * self.sC:][:(self.M + 2) * self.ldc].view(self.M + 2, self.ldc)
        return v[1:self.M + 1, PAD:PAD + self.N]

    def cin_view(self, b):
        v = self.cin[b * self.sC + PAD:][:self.M * self.ldcin].view(self.M, self.ldcin)
        return v[:, :self.N]

    def launch(self, Cbuf, c_in, cfg):
        M, N, K, nb = self.M, self.N, self.K, self.nb
        es = Cbuf.element_size()
        off = (self.ldc + PAD) * es
        kw = dict(M=M, N=N, K=K, ab_dtype=DT[self.dtype], c_dtype=DT[self.dtype],
                  a=[self.A.data_ptr()], lda=self.lda, a_kmajor=True, sA=(M * self.lda, 0),
                  b=[self.B.data_ptr()], ldb=self.ldb, b_kmajor=False, sB=(K * self.ldb, 0),
                  c=[Cbuf.data_ptr() + off], ldc=self.ldc, sC=(self.sC, 0), batch0=nb,
                  alpha=0.5, beta=0.75, splits=1, device=DEV)
        if self.aux is not None:
            kw.update(aux=self.aux[self.ldc + PAD:], ldaux=self.ldc)
        if c_in:
            kw.update(c_in=[self.cin.data_ptr() + PAD * es], ldcin=self.ldcin)
        lib = _lib.load()
        lib.jmt_gemm_set_debug(cfg << 8)
        try:
            ops.gemm(**kw)
            torch.cuda.synchronize()
        finally:
            lib.jmt_gemm_set_debug(0)

    def check(self, cfg, tag):
        bits = lambda t: t.view(torch.int16)
        ref = self.C0.clone()
        for b in range(self.nb):
            self.c_view(ref, b).copy_(self.cin_view(b))
        pre = ref.clone()
        self.launch(ref, False, cfg)                 # in place on C preloaded with c_in
        got, cin0 = self.C0.clone(), self.cin.clone()
        self.launch(got, True, cfg)
        assert torch.equal(bits(self.cin), bits(cin0)), (tag, "c_in written")
        assert not torch.equal(bits(ref), bits(pre)), (tag, "nothing written")
        # C's guard rows / columns and the slack between the entries are C0's in both
        for b in range(self.nb):
            assert torch.equal(bits(self.c_view(got, b)), bits(self.c_view(ref, b))), \
                (tag, b, "bits differ from the in-place launch")
        g0 = self.C0.clone()
        for b in range(self.nb):
            self.c_view(g0, b).copy_(self.c_view(got, b))
        assert torch.equal(bits(got), bits(g0)), (tag, "guard elements written")
        # and the values are the formula's (fp32 products of the 16-bit operands): the output's
        # one rounding to 16 bits is at most 2^-9 of its magnitude, the fp32 sums far below it
        for b in range(self.nb):
            want = 0.5 * self.A[b, :, :self.K].float() @ self.B[b, :, :self.N].float() + \
                0.75 * self.cin_view(b).float()
            if self.aux is not None:
                want = torch.where(self.c_view(self.aux, b).float() > 0, want,
                                   torch.zeros_like(want))
            err = (self.c_view(got, b).float() - want).abs().max().item()
            bound = 2.0 ** -8 * max(want.abs().max().item(), 1.0)
            print(f"{tag} b{b}: |C - fp32| {err:.3e} bound {bound:.3e}")
            assert err <= bound, (tag, b, err, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_one_block_kernel_ragged(dtype):
    """M = 130, N = 72, K = 64: the first wave tile is whole (paired 16-B stores), the others
    are cut by N = 72 and M = 130 (the guarded 8-B / scalar stores)."""
    _Case(130, 72, 64, 1, dtype, False, 1).check(0, "one-block")


@pytest.mark.gpu
@pytest.mark.parametrize("aux", [False, True])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_persistent_kernel_two_batch_entries(dtype, aux):
    """512 x 256 x 128, two batch entries, on the persistent kernel (cfg 40): beta * C alone
    (EPI 1) and with the ReLU mask (EPI 3)."""
    _Case(512, 256, 128, 2, dtype, aux, 2).check(40, f"persistent aux={aux}")


@pytest.mark.gpu
@pytest.mark.parametrize("M", [300, 296])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_ping_pong_partial_last_panel(dtype, M):
    """N = 256, K = 512 under cfg 45 with a partial last row panel: M = 300, and M = 296 (the
    ping-pong kernel takes partial panels of whole 8-row groups; 300 rows run wherever jmt_gemm
    sends them)."""
    _Case(M, 256, 512, 1, dtype, False, 3).check(45, f"ping-pong M={M}")


def test_refusals_before_any_launch():
    """Host only (never dereferenced pointers): fp32 C and a forced split are JMT_ERR_UNSUPPORTED,
    beta == 0, a NULL / short table and a misaligned or too short ldcin JMT_ERR_ARG."""
    lib = _lib.load()
    fake = 0x10000

    def desc(**kw):
        d = GemmDesc()
        d.ab_dtype, d.c_dtype, d.aux_dtype = BF16, BF16, BF16
        d.M, d.N, d.K = 256, 256, 128
        d.a[0] = d.b[0] = d.c[0] = fake
        d.n_a = d.n_b = d.n_c = 1
        d.a_kmajor, d.b_kmajor = 1, 0
        d.lda, d.ldb, d.ldc = 128, 256, 256
        d.batch0 = d.batch1 = 1
        d.alpha, d.beta = 1.0, 1.0
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    tab = (C.c_void_p * 1)(fake)
    call = lambda d, t=tab, n=1, ld=256: lib.jmt_gemm_cin(C.byref(d), t, n, ld, None)
    assert call(desc(c_dtype=F32, aux_dtype=F32)) == _lib.ERR_UNSUPPORTED
    assert b"16-bit C" in lib.jmt_last_error()
    assert call(desc(splits=2)) == _lib.ERR_UNSUPPORTED
    assert b"split-K" in lib.jmt_last_error()
    assert call(desc(beta=0.0)) == _lib.ERR_ARG
    assert b"beta" in lib.jmt_last_error()
    assert call(desc(), None) == _lib.ERR_ARG
    assert b"c_in table" in lib.jmt_last_error()
    assert call(desc(), (C.c_void_p * 1)(None)) == _lib.ERR_ARG
    assert b"c_in[0]" in lib.jmt_last_error()
    d2 = desc(c_mode=1, batch0=2, n_c=2)
    d2.c[1] = fake
    assert call(d2) == _lib.ERR_ARG                      # one entry for two batch entries
    assert b"c_in table" in lib.jmt_last_error()
    assert call(desc(), ld=260) == _lib.ERR_ARG
    assert b"ldcin" in lib.jmt_last_error()
    assert call(desc(), ld=128) == _lib.ERR_ARG          # shorter than a row of C
