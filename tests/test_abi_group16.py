"""The grouped 16-bit-C GEMM entry points without a GPU: their host code (every refusal of
jmt_gemm_group16 / jmt_gemm_group16_ok, the C overlap test, jmt_gemm_persist_cfg) under
AddressSanitizer and UndefinedBehaviorSanitizer in a stand-alone program
(csrc/abi_check_group16.cpp, built by `make asan16` and run directly: nothing is preloaded and
no Python code runs under the sanitizers)."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "joint-multimodal-transformer-6th-abaw_amd", "csrc")


def test_group16_host_code_under_asan_ubsan():
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not installed")
    jobs = str(min(8, os.cpu_count() or 4))
    subprocess.run(["make", "-C", CSRC, "asan16", "-j", jobs], check=True, timeout=1200,
                   stdout=subprocess.DEVNULL)
    exe = os.path.join(CSRC, "build", "asan16", "abi_check_group16")
    syms = subprocess.run(["nm", exe], capture_output=True, text=True).stdout
    assert "__asan_init" in syms or "__asan_report_load" in syms, "not ASan-instrumented"
    assert "__ubsan_handle" in syms, "not UBSan-instrumented"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0"))
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and r.stdout.strip().endswith("abi_check_group16: ok"), \
        (r.stdout, r.stderr[-2000:])
