"""The attention dropout entry points without a GPU: their host code (rate quantisation, argument
checks, the counter limit, the host reference) under AddressSanitizer in a stand-alone program
(csrc/abi_check_attn_drop.cpp, built by `make asan` and run directly: nothing is preloaded and no
Python code runs under the sanitizer)."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "joint-multimodal-transformer-6th-abaw_amd", "csrc")


def test_attn_drop_host_code_under_asan():
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not installed")
    jobs = str(min(8, os.cpu_count() or 4))
    subprocess.run(["make", "-C", CSRC, "build/asan/abi_check_attn_drop", "-j", jobs], check=True,
                   timeout=1200, stdout=subprocess.DEVNULL)
    exe = os.path.join(CSRC, "build", "asan", "abi_check_attn_drop")
    syms = subprocess.run(["nm", exe], capture_output=True, text=True).stdout
    assert "__asan_init" in syms or "__asan_report_load" in syms, "not ASan-instrumented"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0"))
    assert "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and r.stdout.strip().endswith("abi_check_attn_drop: ok"), \
        (r.stdout, r.stderr[-2000:])
