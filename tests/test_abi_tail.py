"""The head / loss tail entry points without a GPU: the host code of jmt_head_fwd_perm,
jmt_head_bwd_perm, their *_perm_drop forms and jmt_ccc_stats_finish(_add) (row maps that do not
tile the rows, null pointers, k out of range) under AddressSanitizer and
UndefinedBehaviorSanitizer in a stand-alone program (csrc/abi_check_tail.cpp, built by
`make asan_tail` and run directly: nothing is preloaded and no Python code runs under the
sanitizers), and their ctypes prototypes."""
import os
import subprocess

import pytest

from jmt import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "joint-multimodal-transformer-6th-abaw_amd", "csrc")


def test_tail_host_code_under_asan_ubsan():
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not installed")
    jobs = str(min(8, os.cpu_count() or 4))
    subprocess.run(["make", "-C", CSRC, "asan_tail", "-j", jobs], check=True, timeout=1200,
                   stdout=subprocess.DEVNULL)
    exe = os.path.join(CSRC, "build", "asan_tail", "abi_check_tail")
    syms = subprocess.run(["nm", exe], capture_output=True, text=True).stdout
    assert "__asan_init" in syms or "__asan_report_load" in syms, "not ASan-instrumented"
    assert "__ubsan_handle" in syms, "not UBSan-instrumented"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0"))
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and r.stdout.strip().endswith("abi_check_tail: ok"), \
        (r.stdout, r.stderr[-2000:])


def test_new_entry_points_are_bound():
    lib = _lib.load()
    P = _lib._PROTOS
    for name in ("jmt_head_fwd_perm", "jmt_head_bwd_perm", "jmt_head_fwd_perm_drop",
                 "jmt_head_bwd_perm_drop", "jmt_ccc_stats_finish", "jmt_ccc_stats_finish_add"):
        assert name in _lib.EXPORTED and hasattr(lib, name)
    i64 = [_lib.c_i64, _lib.c_i64]
    # the row map (P, Q) sits before the stream, in the dropout forms before (p0, p1, ctr)
    for base in ("jmt_head_fwd", "jmt_head_bwd"):
        a = P[base][1]
        assert P[base + "_perm"] == (P[base][0], a[:-1] + i64 + a[-1:])
        d = P[base + "_drop"][1]
        assert P[base + "_perm_drop"] == (P[base][0], d[:-4] + i64 + d[-4:])
    s, f, fa = (P[n][1] for n in ("jmt_ccc_stats", "jmt_ccc_finish", "jmt_ccc_finish_add"))
    assert P["jmt_ccc_stats_finish"][1] == s[:-1] + f[3:]          # after stats: bs, eps, ...
    assert P["jmt_ccc_stats_finish_add"][1] == s[:-1] + fa[3:]
    assert lib.jmt_abi_version() == 7                              # entry points added only
    assert lib.jmt_head_fwd_perm(1, 0, 12, 128, 1, None, 256, None, None, None, None, None, None,
                                 1, 4, 3, None) == -1
    assert b"jmt_head_fwd_perm" in lib.jmt_last_error()
