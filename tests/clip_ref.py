"""Float64 reference, bound and case table for gradient-norm clipping (csrc/grad_norm.hip).

Not a test: tests/test_clip_ref.py validates what is here on the CPU (against
torch.nn.utils.clip_grad_norm_ on float64 tensors, and that seeded defects fall outside the
bound), tests/test_gpu_grad_clip.py runs the kernels against it.

`reference` returns (norm, coef, per-segment norms) of the UNSCALED gradient gs * g:
    segment sums  sum(g[b:e]^2) in float64,  total = their sum in index order,
    norm = gs * sqrt(total),  coef = clamp(max_norm / (norm + 1e-6), max=1)  (NaN stays NaN).

Bound (derived, not measured): the kernel sums in double, whose own error is <= n * 2^-53 ~ 1e-9
relative for the sizes here, and rounds once to fp32 (2^-24); with a factor 2 on top every output
must satisfy |x - ref| <= 2^-23 * |ref|.
"""
import math

import torch

CHUNK = 4096          # grad_norm.hip GN_CHUNK: elements per block trip, from a segment's start
BLOCKS_PER_CU = 8     # GN_BLOCKS_PER_CU: the grid is at most this many blocks per CU
FOLD_THREADS = 1024   # GN_FOLD_THREADS: the one block that folds the chunk partials
EPS = 1e-6
BOUND = 2.0 ** -23

DEFECTS = ("no_eps", "no_clamp", "scaled_norm", "drop_tail", "drop_second_trip",
           "segment_off_by_chunk", "nan_to_one")


def f32(x: float) -> float:
    return float(torch.tensor(x, dtype=torch.float32))


def reference(g: torch.Tensor, max_norm: float, gs: float = 1.0, seg_off=None, defect=None,
              grid: int = 0):
    """g: 1-D tensor (its first n elements are the buffer), seg_off: ascending offsets
    [0, ..., n] or None (one segment).  defect: one of DEFECTS, a wrong kernel to tell apart
    (`grid` blocks for "drop_second_trip")."""
    g = g.detach().double().cpu()
    n = g.numel()
    off = list(seg_off) if seg_off is not None else [0, n]
    if defect == "segment_off_by_chunk" and len(off) > 2:
        off[1] = min(off[1] + CHUNK, off[2])
    sums, chunk = [], 0
    for b, e in zip(off[:-1], off[1:]):
        if defect == "drop_tail":
            e = b + (e - b) // 4 * 4
        s = 0.0
        for c0 in range(b, e, CHUNK):           # the chunks in index order
            if not (defect == "drop_second_trip" and chunk >= grid):
                s += float((g[c0:min(c0 + CHUNK, e)] ** 2).sum())
            chunk += 1
        sums.append(s)
    total = 0.0
    for s in sums:
        total += s
    gs, max_norm = f32(gs), f32(max_norm)       # as the kernel reads them
    norm = math.sqrt(total) * (1.0 if defect == "scaled_norm" else gs)
    den = norm if defect == "no_eps" else norm + EPS
    coef = max_norm / den if den != 0.0 else math.inf
    if math.isinf(max_norm) and math.isinf(den):
        coef = math.nan
    if defect == "nan_to_one":
        coef = 1.0 if math.isnan(coef) else min(coef, 1.0)
    elif defect != "no_clamp" and coef > 1.0:     # a NaN is not > 1: it stays
        coef = 1.0
    return norm, coef, [math.sqrt(s) * gs for s in sums]


def close(x: float, ref: float) -> bool:
    if math.isnan(ref):
        return math.isnan(x)
    if math.isinf(ref):
        return x == ref
    return abs(x - ref) <= BOUND * abs(ref)


def agrees(got, ref) -> bool:
    """(norm, coef, seg norms) against the reference, every figure within the bound."""
    return (close(got[0], ref[0]) and close(got[1], ref[1]) and len(got[2]) == len(ref[2]) and
            all(close(a, b) for a, b in zip(got[2], ref[2])))


# ------------------------------------------------------------------------------- case table
def _values(kind: str, n: int, seed: int) -> torch.Tensor:
    gen = torch.Generator().manual_seed(seed)
    u = torch.rand(n, generator=gen, dtype=torch.float64) * 0.5 + 0.5       # [0.5, 1)
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()
    if kind == "normal":
        x = torch.randn(n, generator=gen, dtype=torch.float64)
    elif kind == "small":                        # norm ~ 1e-2: the 1e-6 in the coefficient counts
        x = u * sign * (1e-2 / math.sqrt(n))
    elif kind == "huge":                         # fp32 squares overflow, double ones do not
        x = torch.full((n,), 1e30, dtype=torch.float64)
    elif kind == "subnormal":                    # below 2^-126; the norm of >= 1024 is normal
        x = u * sign * 1e-38
    elif kind == "spike":                        # one huge element among tiny ones
        x = u * sign * 1e-20
        x[n // 3] = 1e10
    elif kind == "nan":
        x = torch.randn(n, generator=gen, dtype=torch.float64)
        x[n // 2] = math.nan
    elif kind == "inf":
        x = torch.randn(n, generator=gen, dtype=torch.float64)
        x[n // 2] = math.inf
    else:
        raise ValueError(kind)
    return x.float()


def _segments(lens):
    """Offsets of segments of the given real lengths, each padded with zeros to a multiple of 64
    (the layout of _FlatOptimizer._init_flat), and the mask of the real elements."""
    off, n = [0], 0
    for k in lens:
        n += -(-k // 64) * 64
        off.append(n)
    mask = torch.zeros(n, dtype=torch.bool)
    for b, k in zip(off, lens):
        mask[b:b + k] = True
    return off, mask


def cases(grid: int):
    """[(name, g fp32 (n,), max_norm, gs, seg_off or None)]: the sizes at which the kernel can go
    wrong for a launch of at most `grid` blocks.  Without a table: n around the vector width and
    the 64-element unit, one block trip -1 / 0 / +1, the grid's one-trip reach + 300 (a second
    grid-stride trip; more partials than the fold block has threads once grid > FOLD_THREADS).
    With one: 1, 2 and 37 segments, of 64 elements and of many chunks, a 64-element segment last,
    zero padding inside."""
    out = []
    for i, n in enumerate((1, 3, 4, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1)):
        out.append((f"n{n}", _values("normal", n, i), 0.1 * math.sqrt(n), 1.0, None))
    n2 = grid * CHUNK + 300
    out.append(("second_trip", _values("normal", n2, 20), 0.1 * math.sqrt(n2), 1.0, None))
    out.append(("below_max", _values("normal", 65, 21), 100.0, 1.0, None))
    out.append(("small_norm", _values("small", 4099, 22), 1e-3, 1.0, None))
    out.append(("unscale", _values("normal", 4099, 23) * 256.0, 1.0, 1.0 / 256.0, None))
    out.append(("measure_only", _values("normal", 67, 24), math.inf, 1.0, None))
    out.append(("huge", _values("huge", 65, 25), 1.0, 1.0, None))
    out.append(("subnormal", _values("subnormal", CHUNK + 7, 26), 1e-37, 1.0, None))
    out.append(("spike", _values("spike", 2 * CHUNK + 5, 27), 1.0, 1.0, None))
    out.append(("nan", _values("nan", CHUNK + 5, 28), 1.0, 1.0, None))
    out.append(("inf", _values("inf", CHUNK + 5, 29), 1.0, 1.0, None))
    out.append(("inf_measure_only", _values("inf", 67, 30), math.inf, 1.0, None))
    seg_tables = {
        "seg1": [3 * CHUNK + 70],
        "seg2": [64, 2 * CHUNK + 1],
        "seg2_chunks": [2 * CHUNK + 64, 5 * CHUNK - 3, 64],
        "seg37": [(64, 1, 5 * CHUNK + 129, 640, 37, CHUNK, CHUNK + 1)[i % 7] for i in range(36)]
                 + [64],
    }
    for i, (name, lens) in enumerate(seg_tables.items()):
        off, mask = _segments(lens)
        g = _values("normal", off[-1], 40 + i) * mask
        out.append((name, g, 0.1 * math.sqrt(off[-1]), 1.0, off))
    off, mask = _segments([CHUNK + 64, 1500, 64])
    out.append(("seg_unscale", _values("normal", off[-1], 50) * mask * 256.0, 2.0, 1.0 / 256.0,
                off))
    return out
