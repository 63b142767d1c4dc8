"""tests/clip_ref.py on the CPU: the float64 reference equals torch.nn.utils.clip_grad_norm_ on
float64 tensors, and each seeded defect of a clipping kernel falls outside the bound somewhere on
the case table (so tests/test_gpu_grad_clip.py, which holds the kernels to that bound on that
table, would see it)."""
import math

import pytest
import torch

from tests import clip_ref as R

GRID = 8          # one CU's worth of blocks: the table's sizes scale with the grid


@pytest.fixture(scope="module")
def table():
    return R.cases(GRID)


def test_reference_matches_torch_clip_grad_norm(table):
    for name, g, max_norm, gs, off in table:
        unscaled = g.double() * R.f32(gs)
        segs = list(zip(off[:-1], off[1:])) if off is not None else [(0, g.numel())]
        ps = []
        for b, e in segs:
            p = torch.zeros(e - b, dtype=torch.float64, requires_grad=True)
            p.grad = unscaled[b:e].clone()
            ps.append(p)
        tn = float(torch.nn.utils.clip_grad_norm_(ps, R.f32(max_norm), error_if_nonfinite=False))
        norm, coef, seg = R.reference(g, max_norm, gs, off)
        tight = lambda x, ref: (math.isnan(ref) and math.isnan(x)) or x == ref or \
            abs(x - ref) <= 1e-12 * abs(ref)
        assert tight(norm, tn), (name, norm, tn)
        for (b, e), p, s in zip(segs, ps, seg):
            assert tight(s, float(unscaled[b:e].norm())), name
            # what torch did to the gradients is the coefficient
            want = unscaled[b:e] * coef
            if math.isnan(coef):
                assert bool(torch.isnan(p.grad).all()), name
            else:
                fin = torch.isfinite(want)
                assert torch.allclose(p.grad[fin], want[fin], rtol=1e-12, atol=0.0), name
                assert bool((torch.isnan(p.grad[~fin]) | (p.grad[~fin] == want[~fin])).all())


def test_case_table_covers_the_issue(table):
    names = {c[0] for c in table}
    for n in (1, 3, 4, 63, 64, 65, R.CHUNK - 1, R.CHUNK, R.CHUNK + 1):
        assert f"n{n}" in names
    by = {c[0]: c for c in table}
    assert by["second_trip"][1].numel() == GRID * R.CHUNK + 300
    assert -(-R.cases(2 * R.FOLD_THREADS)[9][1].numel() // R.CHUNK) > R.FOLD_THREADS
    assert sorted(len(c[4]) - 1 for c in table if c[4] is not None) == [1, 2, 3, 3, 37]
    for c in table:
        if c[4] is not None:
            assert all(o % 64 == 0 for o in c[4]) and c[4][-1] == c[1].numel()
    assert by["seg37"][4][-1] - by["seg37"][4][-2] == 64            # a 64-element segment last
    assert bool((by["seg37"][1] == 0).any())                       # zero padding inside
    # the value cases are what they say
    assert not bool(torch.isfinite(by["huge"][1] ** 2).any())       # fp32 squares overflow
    assert float(by["subnormal"][1].abs().max()) < 2.0 ** -126
    assert math.isnan(R.reference(*by["nan"][1:])[1])
    inf = R.reference(*by["inf"][1:])
    assert inf[0] == math.inf and inf[1] == 0.0
    assert R.reference(*by["below_max"][1:])[1] == 1.0


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_seeded_defect_falls_outside_the_bound(table, defect):
    caught = []
    for name, g, max_norm, gs, off in table:
        ref = R.reference(g, max_norm, gs, off)
        bad = R.reference(g, max_norm, gs, off, defect=defect, grid=GRID)
        if not R.agrees(bad, ref):
            caught.append(name)
    assert caught, f"no case of the table tells {defect} from the reference"


def test_bound_accepts_an_honest_fp32_rounding(table):
    """The reference's figures rounded once to fp32 (what a kernel exact in double would store)
    are inside the bound on every case."""
    for name, g, max_norm, gs, off in table:
        ref = R.reference(g, max_norm, gs, off)
        got = (R.f32(ref[0]), R.f32(ref[1]), [R.f32(s) for s in ref[2]])
        assert R.agrees(got, ref), name
