"""Key ranges on the fused multi-head attention kernels (jmt_attn_mh_{fwd,bwd}_kr): per-sequence
runs of valid keys from a table of kr_mod entries (sequence n uses entry n % kr_mod).

The ranges cover left, right and both-sides padding, one single key, a range inside one 64-key
tile and ranges that leave whole tiles empty on the left (and on the right).  Checked against the
masked float64 reference under the bounds of tests/test_gpu_attn_mh.py; a full table equals the
plain entry points bit for bit; K / V rows outside the ranges are never read into a result; dK /
dV rows outside them are exact zeros; padded query rows change no other row's bits; a bad table
is clamped, values and addresses."""
import os
import subprocess
import sys

import pytest
import torch

from jmt import _lib
from tests import attn_mh_ref as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
E = 512

# (Lq, Lk, N, H) -> {kr_mod: ranges}
CASES = {
    (70, 70, 6, 8): {6: [(23, 70), (0, 50), (5, 60), (37, 38), (3, 20), (66, 70)],
                     2: [(5, 60), (66, 70)]},
    (33, 129, 4, 4): {4: [(70, 129), (0, 50), (128, 129), (65, 100)],
                      2: [(70, 129), (5, 60)]},
}
PARAMS = [(s, mod) for s, d in CASES.items() for mod in d]
IDS = ["x".join(map(str, s)) + f"-mod{mod}" for s, mod in PARAMS]


def _run(qkv, kv, go, H, kr):
    o, lse = M.fwd(qkv, kv, H, kr=kr)
    dq, dk, dv, _ = M.bwd(qkv, kv, go, o, lse, H, kr=kr)
    return dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv)


def _same(a, b, names=("o", "lse", "dq", "dk", "dv")):
    for n in names:
        assert torch.equal(a[n], b[n]), n


@pytest.mark.parametrize("cd", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape,mod", PARAMS, ids=IDS)
def test_mh_key_ranges_vs_masked_float64(cd, shape, mod):
    Lq, Lk, N, H = shape
    ranges = CASES[shape][mod]
    qkv, kv, go = M.inputs(cd, Lq, Lk, N, seed=43)
    got = _run(qkv, kv, go, H, M.kr_op(ranges, mod))
    ref = M.ref64(qkv, kv, go, H, o=got["o"], ranges=ranges)
    M.check_bounds(cd, qkv, kv, got, ref, H, what=f"{shape} mod {mod}")
    # dK / dV rows of keys outside a range: exact zeros (the buffers arrived as NaN)
    out = ~M.valid_keys(Lk, N, ranges).t()                       # (Lk, N)
    assert out.any()
    for n in ("dk", "dv"):
        assert (got[n][out] == 0).all(), n
    # K / V rows outside the ranges hold other finite values: no output or gradient bit moves
    g = torch.Generator(device=DEV).manual_seed(5)
    noise = (torch.randn(N, Lk, 2 * E, device=DEV, generator=g) * 3).to(cd).permute(1, 0, 2)
    kv2 = torch.where(out[:, :, None], noise, kv).permute(1, 0, 2).contiguous().permute(1, 0, 2)
    assert not torch.equal(kv2, kv)
    _same(_run(qkv, kv2, go, H, M.kr_op(ranges, mod)), got)


@pytest.mark.parametrize("shape", list(CASES), ids=lambda s: "x".join(map(str, s)))
def test_mh_full_table_equals_plain_entry_points(shape):
    Lq, Lk, N, H = shape
    cd = torch.bfloat16
    qkv, kv, go = M.inputs(cd, Lq, Lk, N, seed=44)
    plain = _run(qkv, kv, go, H, None)
    _same(_run(qkv, kv, go, H, M.kr_op([(0, Lk)] * 2, 2)), plain)


def test_mh_padded_query_rows_change_no_other_row():
    """Queries and keys on one axis (self-attention over padded windows): a frame outside the
    key range is also a query row.  Other finite values in the q / dO rows of those frames
    change no bit of o / lse at the other rows; with their dO rows zero in both runs they change
    no bit of dK / dV either (P^T dO and dS = scale P (dP - Delta) are exact zeros there)."""
    cd, (L, N, H), mod = torch.bfloat16, (70, 6, 8), 6
    ranges = CASES[(70, 70, 6, 8)][mod]
    qkv, kv, go = M.inputs(cd, L, L, N, seed=45)
    pad = ~M.valid_keys(L, N, ranges).t()                        # (L, N): padded frames
    go = torch.where(pad[:, :, None], torch.zeros_like(go), go)
    g = torch.Generator(device=DEV).manual_seed(6)
    noise = (torch.randn(N, L, 3 * E, device=DEV, generator=g) * 3).to(cd).permute(1, 0, 2)
    qkv2 = torch.where(pad[:, :, None], noise, qkv).permute(1, 0, 2).contiguous().permute(1, 0, 2)
    kr = M.kr_op(ranges, mod)
    a = _run(qkv, kv, go, H, kr)
    b = _run(qkv2, kv, go, H, kr)
    keep = ~pad
    assert torch.equal(a["o"][keep], b["o"][keep])
    la, lb = (t["lse"].view(N, H, L).permute(2, 0, 1) for t in (a, b))
    assert torch.equal(la[keep], lb[keep])
    assert not torch.equal(a["o"][pad], b["o"][pad])             # the padded rows did change
    assert torch.equal(a["dq"][keep], b["dq"][keep])
    _same(a, b, ("dk", "dv"))


def _clamp_case():
    cd, (Lq, Lk, N, H) = torch.bfloat16, (70, 70, 6, 8)
    qkv, kv, go = M.inputs(cd, Lq, Lk, N, seed=46)
    bad = [(50, 20), (-5, 200), (10, 500), (-7, 3), (69, 1 << 30), (0, 70)]
    good = [(50, 50), (0, 70), (10, 70), (0, 3), (69, 70), (0, 70)]
    return qkv, kv, go, H, bad, good


def test_mh_bad_table_is_clamped():
    """kbeg > kend and kend > Lk: the kernels clamp kbeg to [0, Lk] and kend to [kbeg, Lk], so the
    values are those of the clamped table (the empty range included) and no address moves."""
    qkv, kv, go, H, bad, good = _clamp_case()
    a = _run(qkv, kv, go, H, M.kr_op(bad, 6))
    b = _run(qkv, kv, go, H, M.kr_op(good, 6))
    _same(a, b)
    # once more under the index-checking build of the library, if it has been built
    blib = os.path.join(os.path.dirname(_lib.LIB_PATH), "libjmt_hip_bounds.so")
    if not os.path.exists(blib):
        return
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import torch\n"
            "from jmt import _lib\n"
            "from tests import test_gpu_attn_mh_key_ranges as T, attn_mh_ref as M\n"
            "lib = _lib.load()\n"
            "assert lib.jmt_bounds_violations(1) >= 0\n"
            "qkv, kv, go, H, bad, good = T._clamp_case()\n"
            "T._run(qkv, kv, go, H, M.kr_op(bad, 6))\n"
            "torch.cuda.synchronize()\n"
            "print('violations', lib.jmt_bounds_violations(0))\n")
    env = dict(os.environ, JMT_LIB=blib)
    env["PYTHONPATH"] = os.pathsep.join([repo, os.path.dirname(os.path.dirname(_lib.LIB_PATH)),
                                         env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True,
                       timeout=300, cwd=repo)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "violations 0" in r.stdout, r.stdout
