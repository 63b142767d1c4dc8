// Host-side check of the attention dropout entry points (jmt_attn_mh_fwd_drop / _bwd_drop,
// jmt_attn_dropout, jmt_attn_dropout_reference, jmt_attn_dropout_rate), built with
// AddressSanitizer by `make asan` next to abi_check_mh and run on the CPU by
// tests/test_abi_attn_drop.py.  Every entry point is driven with arguments it must refuse before
// a launch (no kernel runs, no GPU is needed): each call must return the documented JMT_ERR_*
// code and leave a bounded, non-empty jmt_last_error() that names the check.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/jmt.h"

static int g_fail = 0;

static void expect_rc(const char* what, int rc, int code, const char* needle) {
  const char* e = jmt_last_error();
  const size_t n = e ? strnlen(e, 1024) : 0;
  if (rc != code || n == 0 || n >= 512 || !strstr(e, needle)) {
    fprintf(stderr, "FAIL %s: rc=%d (want %d) err='%s' (want '%s')\n", what, rc, code,
            e ? e : "(null)", needle);
    ++g_fail;
  }
}

static void expect_eq(const char* what, double got, double want) {
  if (got != want) {
    fprintf(stderr, "FAIL %s: %g, not %g\n", what, got, want);
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
  const uint32_t* ctr = (const uint32_t*)buf;
  const uint32_t* ctr_mis = (const uint32_t*)(buf + 2);
  alignas(8) const int krt[4] = {0, 70, 5, 60};

#define FWD(dt, N, H, Lq, dh, q, sq, kr, mod, p, c)                                              \
  jmt_attn_mh_fwd_drop(dt, N, H, Lq, 70, dh, q, sq, 512, algn, 1024, 512, algn, 1024, 512, algn, \
                       1024, 512, 0.125f, fl, kr, mod, p, c, nullptr)
#define BWD(dt, N, H, Lq, dh, q, sq, kr, mod, p, c)                                              \
  jmt_attn_mh_bwd_drop(dt, N, H, Lq, 70, dh, algn, 1024, 512, algn, 1024, 512, q, sq, 512, algn, \
                       1024, 512, algn, 1024, 512, fl, algn, 1024, 512, algn, 1024, 512, algn,   \
                       1024, 512, 0.125f, fl, kr, mod, p, c, nullptr)

  // the rate and its quantisation
  expect_eq("rate 0.1", jmt_attn_dropout_rate(0.1f), 26.0 / 256);
  expect_eq("rate 0.25", jmt_attn_dropout_rate(0.25f), 0.25);
  expect_eq("rate 1/1024", jmt_attn_dropout_rate(1.0f / 1024), 0.0);
  expect_eq("rate 255.4/256", jmt_attn_dropout_rate(255.4f / 256), 255.0 / 256);
  expect_eq("rate 0.999", jmt_attn_dropout_rate(0.999f), -1.0);
  expect_eq("rate 1", jmt_attn_dropout_rate(1.0f), -1.0);
  expect_eq("rate -0.1", jmt_attn_dropout_rate(-0.1f), -1.0);

  for (int b = 0; b < 2; ++b) {
    const char* nm = b ? "jmt_attn_mh_bwd_drop" : "jmt_attn_mh_fwd_drop";
#define CALL(...) (b ? BWD(__VA_ARGS__) : FWD(__VA_ARGS__))
    // outside jmt_attn_mh_ok: JMT_ERR_UNSUPPORTED before anything else is looked at
    expect_rc(nm, CALL(JMT_BF16, 2, 1, 70, 512, algn, 1536, nullptr, 1, 0.1f, ctr),
              JMT_ERR_UNSUPPORTED, "jmt_attn_mh_ok");
    expect_rc(nm, CALL(JMT_F32, 2, 8, 70, 64, algn, 1536, nullptr, 1, 0.1f, ctr),
              JMT_ERR_UNSUPPORTED, "jmt_attn_mh_ok");
    // the rate
    expect_rc(nm, CALL(JMT_BF16, 2, 8, 70, 64, algn, 1536, nullptr, 1, 1.0f, ctr), JMT_ERR_ARG,
              "outside [0, 1)");
    expect_rc(nm, CALL(JMT_BF16, 2, 8, 70, 64, algn, 1536, nullptr, 1, -0.25f, ctr), JMT_ERR_ARG,
              "outside [0, 1)");
    expect_rc(nm, CALL(JMT_BF16, 2, 8, 70, 64, algn, 1536, nullptr, 1, 0.999f, ctr), JMT_ERR_ARG,
              "T8");
    // the counter block
    expect_rc(nm, CALL(JMT_BF16, 2, 8, 70, 64, algn, 1536, nullptr, 1, 0.1f, nullptr),
              JMT_ERR_ARG, "counter block");
    expect_rc(nm, CALL(JMT_BF16, 2, 8, 70, 64, algn, 1536, krt, 2, 0.1f, ctr_mis), JMT_ERR_ARG,
              "counter block");
    expect_rc(nm, CALL(JMT_BF16, 2, 8, 70, 64, algn, 1536, nullptr, 1, 0.0f, nullptr),
              JMT_ERR_ARG, "counter block");
    // the counter limit: 2^14 * 2^12 (n, h) pairs of 2^10 queries = 2^34 query blocks of 4, inside
    // jmt_attn_mh_ok (2^30 items of 64 query rows)
    expect_rc(nm, CALL(JMT_BF16, 1 << 14, 1 << 12, 1024, 64, algn, 64, nullptr, 1, 0.1f, ctr),
              JMT_ERR_UNSUPPORTED, "2^32 query blocks");
    // operands, strides and tables as the plain entry points
    expect_rc(nm, CALL(JMT_BF16, 2, 8, 70, 64, misal, 1536, nullptr, 1, 0.1f, ctr), JMT_ERR_ARG,
              "operand");
    expect_rc(nm, CALL(JMT_BF16, 2, 8, 70, 64, nullptr, 1536, krt, 2, 0.1f, ctr), JMT_ERR_ARG,
              "operand");
    expect_rc(nm, CALL(JMT_F16, 2, 4, 70, 128, algn, 1532, nullptr, 1, 0.5f, ctr), JMT_ERR_ARG,
              "stride");
    expect_rc(nm, CALL(JMT_BF16, 2, 8, 70, 64, algn, 1536, krt + 1, 1, 0.1f, ctr), JMT_ERR_ARG,
              "key range table");
    expect_rc(nm, CALL(JMT_BF16, 3, 8, 70, 64, algn, 1536, krt, 2, 0.1f, ctr), JMT_ERR_ARG,
              "kr_mod");
    // T8 = 0 goes through the plain path's checks
    expect_rc(nm, CALL(JMT_BF16, 2, 8, 70, 64, misal, 1536, nullptr, 1, 0.001f, ctr), JMT_ERR_ARG,
              "operand");
    // nothing to do
    expect_eq(nm, CALL(JMT_BF16, 0, 8, 70, 64, nullptr, 1536, nullptr, 1, 2.0f, nullptr), JMT_OK);
    expect_eq(nm, CALL(JMT_BF16, 2, 8, 0, 64, nullptr, 1536, nullptr, 1, 2.0f, nullptr), JMT_OK);
#undef CALL
  }

  // jmt_attn_dropout
#define DROP(dt, x, ldx, y, ldy, NH, Lq, Lk, p, c) \
  jmt_attn_dropout(dt, x, ldx, y, ldy, NH, Lq, Lk, p, c, nullptr)
  expect_rc("drop dtype", DROP(7, algn, 136, algn, 136, 4, 9, 130, 0.1f, ctr), JMT_ERR_ARG,
            "dtype");
  expect_rc("drop null", DROP(JMT_F32, nullptr, 136, algn, 136, 4, 9, 130, 0.1f, ctr), JMT_ERR_ARG,
            "null pointer");
  expect_rc("drop ctr", DROP(JMT_F32, algn, 136, algn, 136, 4, 9, 130, 0.1f, nullptr), JMT_ERR_ARG,
            "counter block");
  expect_rc("drop p", DROP(JMT_F32, algn, 136, algn, 136, 4, 9, 130, 1.5f, ctr), JMT_ERR_ARG,
            "outside [0, 1)");
  expect_rc("drop T8", DROP(JMT_F32, algn, 136, algn, 136, 4, 9, 130, 0.999f, ctr), JMT_ERR_ARG,
            "T8");
  expect_rc("drop ld short", DROP(JMT_BF16, algn, 128, algn, 136, 4, 9, 130, 0.1f, ctr),
            JMT_ERR_ARG, "row strides");
  expect_rc("drop ld odd", DROP(JMT_BF16, algn, 134, algn, 136, 4, 9, 130, 0.1f, ctr), JMT_ERR_ARG,
            "row strides");
  expect_rc("drop misaligned", DROP(JMT_BF16, misal, 136, algn, 136, 4, 9, 130, 0.1f, ctr),
            JMT_ERR_ARG, "8-B aligned");
  expect_rc("drop in place strides", DROP(JMT_F32, algn, 136, algn, 144, 4, 9, 130, 0.1f, ctr),
            JMT_ERR_ARG, "in place");
  expect_rc("drop sizes", DROP(JMT_F32, algn, 136, algn, 136, -1, 9, 130, 0.1f, ctr), JMT_ERR_ARG,
            "bad sizes");
  expect_rc("drop counter limit", DROP(JMT_F32, algn, 8, algn, 8, 1LL << 31, 9, 5, 0.1f, ctr),
            JMT_ERR_UNSUPPORTED, "2^32 query blocks");
  expect_eq("drop nothing", DROP(JMT_F32, algn, 136, algn, 136, 0, 9, 130, 0.1f, ctr), JMT_OK);

  // the host reference: refusals, then a 4 x 4 block read back
  float out[2 * 5 * 6];
  expect_rc("ref null", jmt_attn_dropout_reference(nullptr, 2, 5, 6, 0.5f, out), JMT_ERR_ARG,
            "null pointer");
  expect_rc("ref p", jmt_attn_dropout_reference(ctr, 2, 5, 6, 1.0f, out), JMT_ERR_ARG, "[0, 1)");
  expect_rc("ref T8", jmt_attn_dropout_reference(ctr, 2, 5, 6, 0.999f, out), JMT_ERR_ARG, "T8");
  expect_rc("ref sizes", jmt_attn_dropout_reference(ctr, 2, -5, 6, 0.5f, out), JMT_ERR_ARG,
            "bad sizes");
  const uint32_t words[4] = {1u, 2u, 3u, 4u};
  expect_eq("ref ok", jmt_attn_dropout_reference(words, 2, 5, 6, 0.5f, out), JMT_OK);
  int kept = 0;
  for (int i = 0; i < 60; ++i) {
    if (out[i] != 0.f && out[i] != 2.f) ++g_fail;
    kept += out[i] != 0.f;
  }
  if (kept == 0 || kept == 60) {
    fprintf(stderr, "FAIL ref mask: %d of 60 kept\n", kept);
    ++g_fail;
  }
  expect_eq("ref p 0", jmt_attn_dropout_reference(words, 2, 5, 6, 0.0f, out), JMT_OK);
  for (int i = 0; i < 60; ++i)
    if (out[i] != 1.f) ++g_fail;

  if (g_fail) {
    fprintf(stderr, "abi_check_attn_drop: %d failure(s)\n", g_fail);
    return 1;
  }
  printf("abi_check_attn_drop: ok\n");
  return 0;
}
