// Host-side check of the multi-head attention entry points (jmt_attn_mh_*), built with
// AddressSanitizer by `make asan` next to abi_check and run on the CPU by
// tests/test_abi_attn_mh.py.  Every new entry point is driven with arguments it must refuse
// before a launch (no kernel runs, no GPU is needed): each call must return the documented
// JMT_ERR_* code and leave a bounded, non-empty jmt_last_error() that names the check.
#include <stdint.h>
#include <initializer_list>
#include <stdio.h>
#include <string.h>

#include "../../include/jmt.h"

static int g_fail = 0;

// refused with exactly `code` and a message that names the check
static void expect_rc(const char* what, int rc, int code, const char* needle) {
  const char* e = jmt_last_error();
  const size_t n = e ? strnlen(e, 1024) : 0;
  if (rc != code || n == 0 || n >= 512 || !strstr(e, needle)) {
    fprintf(stderr, "FAIL %s: rc=%d (want %d) err='%s' (want '%s')\n", what, rc, code,
            e ? e : "(null)", needle);
    ++g_fail;
  }
}

static void expect_eq(const char* what, int got, int want) {
  if (got != want) {
    fprintf(stderr, "FAIL %s: %d, not %d\n", what, got, want);
    ++g_fail;
  }
}

int main() {
  if (jmt_abi_version() != JMT_ABI_VERSION) {
    fprintf(stderr, "FAIL abi version\n");
    return 1;
  }
  alignas(16) char buf[64];
  void* algn = (void*)buf;        // aligned, never dereferenced (the checks fail first)
  void* misal = (void*)(buf + 2);
  float* fl = (float*)buf;
  alignas(8) const int krt[4] = {0, 70, 5, 60};

  // one call of each entry point; the operands are the macro's parameters
#define FWD(dt, N, H, Lq, Lk, dh, q, sq, k, sk, v, sv, o, so)                                   \
  jmt_attn_mh_fwd(dt, N, H, Lq, Lk, dh, q, sq, 512, k, sk, 512, v, sv, 512, o, so, 512, 0.125f, \
                  fl, nullptr)
#define FWD_KR(dt, N, H, Lq, Lk, dh, q, sq, kr, mod)                                            \
  jmt_attn_mh_fwd_kr(dt, N, H, Lq, Lk, dh, q, sq, 512, algn, 1024, 512, algn, 1024, 512, algn,  \
                     1024, 512, 0.125f, fl, kr, mod, nullptr)
#define BWD(dt, N, H, Lq, Lk, dh, go, sgo, q, sq, dq, sdq, dv, lse, delta)                      \
  jmt_attn_mh_bwd(dt, N, H, Lq, Lk, dh, go, sgo, 512, algn, 1024, 512, q, sq, 512, algn, 1024,  \
                  512, algn, 1024, 512, lse, dq, sdq, 512, algn, 1024, 512, dv, 1024, 512,      \
                  0.125f, delta, nullptr)
#define BWD_KR(dt, N, H, Lq, Lk, dh, q, sq, kr, mod)                                            \
  jmt_attn_mh_bwd_kr(dt, N, H, Lq, Lk, dh, algn, 1024, 512, algn, 1024, 512, q, sq, 512, algn,  \
                     1024, 512, algn, 1024, 512, fl, algn, 1024, 512, algn, 1024, 512, algn,    \
                     1024, 512, 0.125f, fl, kr, mod, nullptr)
  const char* OKMSG = "jmt_attn_mh_ok";

  // jmt_attn_mh_ok: the range itself
  expect_eq("ok bf16 64", jmt_attn_mh_ok(JMT_BF16, 64, 2, 8, 70, 70, 1536, 1024, 1024) != 0, 1);
  expect_eq("ok f16 128", jmt_attn_mh_ok(JMT_F16, 128, 2, 4, 1, 1, 512, 512, 512) != 0, 1);
  expect_eq("ok max L", jmt_attn_mh_ok(JMT_BF16, 64, 1, 1, 1 << 20, 1 << 20, 64, 64, 64) != 0, 1);
  expect_eq("ok f32", jmt_attn_mh_ok(JMT_F32, 64, 2, 8, 70, 70, 1536, 1024, 1024), 0);
  expect_eq("ok dh 32", jmt_attn_mh_ok(JMT_BF16, 32, 2, 16, 70, 70, 1536, 1024, 1024), 0);
  expect_eq("ok dh 256", jmt_attn_mh_ok(JMT_BF16, 256, 2, 2, 70, 70, 1536, 1024, 1024), 0);
  expect_eq("ok dh 512", jmt_attn_mh_ok(JMT_BF16, 512, 2, 1, 70, 70, 1536, 1024, 1024), 0);
  expect_eq("ok Lk 0", jmt_attn_mh_ok(JMT_BF16, 64, 2, 8, 70, 0, 1536, 1024, 1024), 0);
  expect_eq("ok Lq past", jmt_attn_mh_ok(JMT_BF16, 64, 1, 1, (1 << 20) + 1, 70, 64, 64, 64), 0);
  expect_eq("ok Lk past", jmt_attn_mh_ok(JMT_BF16, 64, 1, 1, 70, (1 << 20) + 1, 64, 64, 64), 0);
  // 2^17 * 2^14 sequences-heads of one tile each = 2^31 items: one past the grid limit
  expect_eq("ok items past", jmt_attn_mh_ok(JMT_BF16, 64, 1 << 17, 1 << 14, 64, 64, 64, 64, 64), 0);
  expect_eq("ok items at", jmt_attn_mh_ok(JMT_BF16, 64, (1 << 17) - 1, 1 << 14, 64, 64, 64, 64,
                                          64) != 0, 1);
  expect_eq("ok stride past", jmt_attn_mh_ok(JMT_BF16, 64, 2, 8, 70, 70, 1LL << 31, 1024, 1024), 0);
  expect_eq("ok stride negative", jmt_attn_mh_ok(JMT_BF16, 64, 2, 8, 70, 70, 1536, -8, 1024), 0);

  // outside jmt_attn_mh_ok: JMT_ERR_UNSUPPORTED before anything else is looked at
  for (int dh : {32, 256, 512}) {
    expect_rc("fwd dh", FWD(JMT_BF16, 2, 512 / dh, 70, 70, dh, algn, 1536, algn, 1024, algn, 1024,
                            algn, 512), JMT_ERR_UNSUPPORTED, OKMSG);
    expect_rc("fwd_kr dh", FWD_KR(JMT_BF16, 2, 512 / dh, 70, 70, dh, algn, 1536, krt, 2),
              JMT_ERR_UNSUPPORTED, OKMSG);
    expect_rc("bwd dh", BWD(JMT_BF16, 2, 512 / dh, 70, 70, dh, algn, 512, algn, 1536, algn, 1536,
                            algn, fl, fl), JMT_ERR_UNSUPPORTED, OKMSG);
    expect_rc("bwd_kr dh", BWD_KR(JMT_BF16, 2, 512 / dh, 70, 70, dh, algn, 1536, krt, 2),
              JMT_ERR_UNSUPPORTED, OKMSG);
  }
  expect_rc("fwd f32", FWD(JMT_F32, 2, 8, 70, 70, 64, algn, 1536, algn, 1024, algn, 1024, algn,
                           512), JMT_ERR_UNSUPPORTED, OKMSG);
  expect_rc("fwd_kr f32", FWD_KR(JMT_F32, 2, 8, 70, 70, 64, algn, 1536, krt, 2),
            JMT_ERR_UNSUPPORTED, OKMSG);
  expect_rc("bwd f32", BWD(JMT_F32, 2, 8, 70, 70, 64, algn, 512, algn, 1536, algn, 1536, algn, fl,
                           fl), JMT_ERR_UNSUPPORTED, OKMSG);
  expect_rc("bwd_kr f32", BWD_KR(JMT_F32, 2, 8, 70, 70, 64, algn, 1536, krt, 2),
            JMT_ERR_UNSUPPORTED, OKMSG);
  expect_rc("fwd Lq past", FWD(JMT_BF16, 1, 1, (1 << 20) + 1, 70, 64, algn, 64, algn, 64, algn, 64,
                               algn, 64), JMT_ERR_UNSUPPORTED, OKMSG);
  expect_rc("bwd Lk past", BWD(JMT_BF16, 1, 1, 70, (1 << 20) + 1, 64, algn, 64, algn, 64, algn, 64,
                               algn, fl, fl), JMT_ERR_UNSUPPORTED, OKMSG);
  expect_rc("fwd items past", FWD(JMT_BF16, 1 << 17, 1 << 14, 64, 64, 64, algn, 64, algn, 64, algn,
                                  64, algn, 64), JMT_ERR_UNSUPPORTED, OKMSG);
  expect_rc("fwd_kr q stride past", FWD_KR(JMT_BF16, 2, 8, 70, 70, 64, algn, 1LL << 31, krt, 2),
            JMT_ERR_UNSUPPORTED, OKMSG);
  expect_rc("bwd_kr Lk 0", BWD_KR(JMT_BF16, 2, 8, 70, 0, 64, algn, 1536, krt, 2),
            JMT_ERR_UNSUPPORTED, OKMSG);

  // inside the range: pointers, strides and tables are JMT_ERR_ARG
  expect_rc("fwd null q", FWD(JMT_BF16, 2, 8, 70, 70, 64, nullptr, 1536, algn, 1024, algn, 1024,
                              algn, 512), JMT_ERR_ARG, "operand 0");
  expect_rc("fwd misaligned k", FWD(JMT_BF16, 2, 8, 70, 70, 64, algn, 1536, misal, 1024, algn,
                                    1024, algn, 512), JMT_ERR_ARG, "operand 1");
  expect_rc("fwd null v", FWD(JMT_F16, 2, 4, 70, 70, 128, algn, 1536, algn, 1024, nullptr, 1024,
                              algn, 512), JMT_ERR_ARG, "operand 2");
  expect_rc("fwd misaligned o", FWD(JMT_BF16, 2, 8, 70, 70, 64, algn, 1536, algn, 1024, algn, 1024,
                                    misal, 512), JMT_ERR_ARG, "operand 3");
  expect_rc("fwd q stride 1532", FWD(JMT_BF16, 2, 8, 70, 70, 64, algn, 1532, algn, 1024, algn,
                                     1024, algn, 512), JMT_ERR_ARG, "stride 0");
  expect_rc("fwd o stride 516", FWD(JMT_BF16, 2, 8, 70, 70, 64, algn, 1536, algn, 1024, algn, 1024,
                                    algn, 516), JMT_ERR_ARG, "stride 6");
  expect_rc("fwd_kr misaligned q", FWD_KR(JMT_BF16, 2, 8, 70, 70, 64, misal, 1536, krt, 2),
            JMT_ERR_ARG, "operand 0");
  expect_rc("fwd_kr null table", FWD_KR(JMT_BF16, 2, 8, 70, 70, 64, algn, 1536, nullptr, 2),
            JMT_ERR_ARG, "key range table");
  expect_rc("fwd_kr misaligned table", FWD_KR(JMT_BF16, 2, 8, 70, 70, 64, algn, 1536, krt + 1, 1),
            JMT_ERR_ARG, "key range table");
  expect_rc("fwd_kr kr_mod 0", FWD_KR(JMT_BF16, 2, 8, 70, 70, 64, algn, 1536, krt, 0), JMT_ERR_ARG,
            "kr_mod");
  expect_rc("fwd_kr N % kr_mod", FWD_KR(JMT_BF16, 3, 8, 70, 70, 64, algn, 1536, krt, 2),
            JMT_ERR_ARG, "kr_mod");
  expect_rc("bwd null dO", BWD(JMT_BF16, 2, 8, 70, 70, 64, nullptr, 512, algn, 1536, algn, 1536,
                               algn, fl, fl), JMT_ERR_ARG, "operand 0");
  expect_rc("bwd misaligned q", BWD(JMT_BF16, 2, 8, 70, 70, 64, algn, 512, misal, 1536, algn, 1536,
                                    algn, fl, fl), JMT_ERR_ARG, "operand 2");
  expect_rc("bwd misaligned dq", BWD(JMT_F16, 2, 4, 70, 70, 128, algn, 512, algn, 1536, misal,
                                     1536, algn, fl, fl), JMT_ERR_ARG, "operand 5");
  expect_rc("bwd null dv", BWD(JMT_BF16, 2, 8, 70, 70, 64, algn, 512, algn, 1536, algn, 1536,
                               nullptr, fl, fl), JMT_ERR_ARG, "operand 7");
  expect_rc("bwd dO stride 516", BWD(JMT_BF16, 2, 8, 70, 70, 64, algn, 516, algn, 1536, algn, 1536,
                                     algn, fl, fl), JMT_ERR_ARG, "stride 0");
  expect_rc("bwd dq stride 1540", BWD(JMT_BF16, 2, 8, 70, 70, 64, algn, 512, algn, 1536, algn,
                                      1540, algn, fl, fl), JMT_ERR_ARG, "stride 10");
  expect_rc("bwd null lse", BWD(JMT_BF16, 2, 8, 70, 70, 64, algn, 512, algn, 1536, algn, 1536,
                                algn, nullptr, fl), JMT_ERR_ARG, "lse");
  expect_rc("bwd null delta", BWD(JMT_BF16, 2, 8, 70, 70, 64, algn, 512, algn, 1536, algn, 1536,
                                  algn, fl, nullptr), JMT_ERR_ARG, "delta");
  expect_rc("bwd misaligned delta", BWD(JMT_BF16, 2, 8, 70, 70, 64, algn, 512, algn, 1536, algn,
                                        1536, algn, fl, (float*)(buf + 2)), JMT_ERR_ARG, "delta");
  expect_rc("bwd_kr q stride 1532", BWD_KR(JMT_BF16, 2, 8, 70, 70, 64, algn, 1532, krt, 2),
            JMT_ERR_ARG, "stride 4");
  expect_rc("bwd_kr null table", BWD_KR(JMT_BF16, 2, 8, 70, 70, 64, algn, 1536, nullptr, 2),
            JMT_ERR_ARG, "key range table");
  expect_rc("bwd_kr misaligned table", BWD_KR(JMT_BF16, 2, 8, 70, 70, 64, algn, 1536, krt + 1, 1),
            JMT_ERR_ARG, "key range table");
  expect_rc("bwd_kr N % kr_mod", BWD_KR(JMT_BF16, 3, 8, 70, 70, 64, algn, 1536, krt, 2),
            JMT_ERR_ARG, "kr_mod");

  // nothing to do: JMT_OK without a launch, whatever else the arguments are
  expect_eq("fwd N 0", FWD(JMT_BF16, 0, 8, 70, 70, 64, nullptr, 1536, nullptr, 1024, nullptr, 1024,
                           nullptr, 512), JMT_OK);
  expect_eq("fwd Lq 0", FWD(JMT_BF16, 2, 8, 0, 70, 64, nullptr, 1536, nullptr, 1024, nullptr, 1024,
                            nullptr, 512), JMT_OK);
  expect_eq("fwd_kr N 0", FWD_KR(JMT_BF16, 0, 8, 70, 70, 64, nullptr, 1536, nullptr, 2), JMT_OK);
  expect_eq("bwd N 0", BWD(JMT_BF16, 0, 8, 70, 70, 64, nullptr, 512, nullptr, 1536, nullptr, 1536,
                           nullptr, nullptr, nullptr), JMT_OK);
  expect_eq("bwd_kr Lq 0", BWD_KR(JMT_BF16, 2, 8, 0, 70, 64, nullptr, 1536, nullptr, 2), JMT_OK);

  if (g_fail) {
    fprintf(stderr, "abi_check_mh: %d failure(s)\n", g_fail);
    return 1;
  }
  printf("abi_check_mh: ok\n");
  return 0;
}
