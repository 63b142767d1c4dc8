"""The multi-head attention entry points without a GPU: their host code (range function, argument
checks, error formatting) under AddressSanitizer in a stand-alone program (csrc/abi_check_mh.cpp,
built by `make asan` next to abi_check and run directly: nothing is preloaded and no Python code
runs under the sanitizer), and functional.attn_plan's "mh" answer."""
import os
import subprocess

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "joint-multimodal-transformer-6th-abaw_amd", "csrc")


def test_mh_host_code_under_asan():
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not installed")
    jobs = str(min(8, os.cpu_count() or 4))
    subprocess.run(["make", "-C", CSRC, "build/asan/abi_check_mh", "-j", jobs], check=True,
                   timeout=1200, stdout=subprocess.DEVNULL)
    exe = os.path.join(CSRC, "build", "asan", "abi_check_mh")
    syms = subprocess.run(["nm", exe], capture_output=True, text=True).stdout
    assert "__asan_init" in syms or "__asan_report_load" in syms, "not ASan-instrumented"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0"))
    assert "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and r.stdout.strip().endswith("abi_check_mh: ok"), \
        (r.stdout, r.stderr[-2000:])


def test_attn_plan_mh_answers():
    """(bf16, N = 2, 65 x 33) on aligned operands: "mh" for H = 8 and H = 4 (head dims 64 and
    128), forward and backward, never whole rows or shared queries, with and without key ranges;
    "gemm" with the switch off, for H = 2 (head dim 256), for fp32 and for a misaligned k; H = 1
    keeps its answer."""
    from jmt import ops
    from jmt.functional import AttnOperand as Op, AttnPlan, attn_plan
    bf, E = torch.bfloat16, 512

    def plan(cd, H, fwd=None, kr=False, **kw):
        d = dict(q=Op(True, 3 * E), k=Op(True, 2 * E), v=Op(True, 2 * E), o=Op(True, E),
                 go=Op(True, E), dq=Op(True, 3 * E), dk=Op(True, 2 * E), dv=Op(True, 2 * E))
        d.update(kw)
        return attn_plan(cd, 2, H, 65, 33, E, fwd=fwd, kr=kr, **d)

    mh, gemm = AttnPlan("mh", False, "mh", False), AttnPlan("gemm", False, "gemm", False)
    for H in (8, 4):
        assert plan(bf, H) == mh
        assert plan(torch.float16, H) == mh
        assert plan(bf, H, kr=True) == mh
        assert plan(torch.float32, H) == gemm
        assert plan(bf, H, k=Op(False, 2 * E)) == gemm
        assert plan(bf, H, o=Op(False, E)) == gemm
        # misaligned gradient buffers do not change the answer (aligned temporaries)
        assert plan(bf, H, dq=Op(False, 3 * E), dk=Op(False, 2 * E)) == mh
        ops._attn_mh["on"] = False
        try:
            assert plan(bf, H) == gemm
            assert plan(bf, H, kr=True) == gemm
            # the backward of a forward that ran "mh" stays "mh": the saved state fixes it
            assert plan(bf, H, fwd="mh").bwd == "mh"
        finally:
            ops._attn_mh["on"] = True
        ops._attn_fused["on"] = False
        try:
            assert plan(bf, H) == gemm
        finally:
            ops._attn_fused["on"] = True
    assert plan(bf, 2) == gemm and plan(bf, 2, kr=True) == gemm
    assert plan(bf, 16) == gemm                           # head dim 32
    assert plan(bf, 1) == AttnPlan("fused", True, "pds_dkdv", True)
    # "small" and "short" are asked first
    q = Op(True, 3 * E)
    assert attn_plan(bf, 3, 8, 6, 6, E, q, q, q, Op(True, E)).fwd == "small"
    assert attn_plan(bf, 3, 8, 9, 9, E, q, q, q, Op(True, E)).fwd == "mh"
