// Host-side check of the head / loss tail entry points (jmt_head_fwd_perm, jmt_head_bwd_perm,
// their *_perm_drop forms, jmt_ccc_stats_finish, jmt_ccc_stats_finish_add), built with
// AddressSanitizer and UndefinedBehaviorSanitizer by `make asan_tail` from the translation units
// they reach and run on the CPU by tests/test_abi_tail.py.  Every entry point is driven with
// arguments it must refuse before a launch (no kernel runs, no GPU is needed): each call must
// return JMT_ERR_ARG and leave a bounded, non-empty jmt_last_error() that names the check.
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

static void expect_eq(const char* what, long long got, long long want) {
  if (got != want) {
    fprintf(stderr, "FAIL %s: %lld, not %lld\n", what, got, want);
    ++g_fail;
  }
}

int main() {
  if (jmt_abi_version() != JMT_ABI_VERSION) {
    fprintf(stderr, "FAIL abi version\n");
    return 1;
  }
  alignas(16) char buf[64];       // aligned, never dereferenced (the checks fail first)
  void* al = buf;
  void* misal = buf + 4;
  float* fl = (float*)buf;
  double* db = (double*)buf;
  const uint32_t* ctr = (const uint32_t*)buf;
  const int64_t big = (int64_t)1 << 31;

  // ---- forward, row map
#define FWD(rows, k, h, w0, y0, ldy, P, Q)                                                   \
  jmt_head_fwd_perm(JMT_BF16, JMT_F32, rows, 128, k, h, 256, w0, al, nullptr, nullptr, y0, al, \
                    ldy, P, Q, nullptr)
  const char* F = "jmt_head_fwd_perm";
  expect_rc("fwd P*Q short", FWD(12, 1, al, al, al, 1, 3, 3), JMT_ERR_ARG, "P * Q = rows");
  expect_rc("fwd P*Q long", FWD(12, 1, al, al, al, 1, 4, 4), JMT_ERR_ARG, "P * Q = rows");
  expect_rc("fwd P 0", FWD(12, 1, al, al, al, 1, 0, 12), JMT_ERR_ARG, "P * Q = rows");
  expect_rc("fwd Q negative", FWD(12, 1, al, al, al, 1, -3, -4), JMT_ERR_ARG, "P * Q = rows");
  expect_rc("fwd P past rows", FWD(12, 1, al, al, al, 1, big * 4, 3), JMT_ERR_ARG,
            "P * Q = rows");
  expect_rc("fwd product wraps", FWD(12, 1, al, al, al, 1, (int64_t)1 << 62, 4), JMT_ERR_ARG,
            "P * Q = rows");
  expect_rc("fwd rows past", FWD(big, 1, al, al, al, 1, big, 1), JMT_ERR_ARG, "31 bits");
  expect_rc("fwd name", FWD(12, 1, al, al, al, 1, 5, 3), JMT_ERR_ARG, F);
  expect_rc("fwd null h", FWD(12, 1, nullptr, al, al, 1, 4, 3), JMT_ERR_ARG, "null pointer");
  expect_rc("fwd null W2", FWD(12, 1, al, nullptr, al, 1, 4, 3), JMT_ERR_ARG, "null pointer");
  expect_rc("fwd null y", FWD(12, 1, al, al, nullptr, 1, 4, 3), JMT_ERR_ARG, "outputs");
  expect_rc("fwd k 0", FWD(12, 0, al, al, al, 1, 4, 3), JMT_ERR_ARG, "k = 0");
  expect_rc("fwd k 25", FWD(12, 25, al, al, al, 25, 4, 3), JMT_ERR_ARG, "k = 25");
  expect_rc("fwd ldy under k", FWD(12, 20, al, al, al, 19, 4, 3), JMT_ERR_ARG, "outputs");
  expect_rc("fwd misaligned h", FWD(12, 1, misal, al, al, 1, 4, 3), JMT_ERR_ARG, "8-B aligned");
  expect_rc("fwd negative rows", FWD(-1, 1, al, al, al, 1, 1, 1), JMT_ERR_ARG, "null pointer");
  expect_eq("fwd rows 0", FWD(0, 1, al, al, al, 1, 1, 1), JMT_OK);
  expect_rc("fwd hidden width",
            jmt_head_fwd_perm(JMT_BF16, JMT_F32, 12, 64, 1, al, 256, al, al, nullptr, nullptr, al,
                              al, 1, 4, 3, nullptr), JMT_ERR_ARG, "hidden width");
  expect_rc("fwd y dtype",
            jmt_head_fwd_perm(JMT_BF16, JMT_F16, 12, 128, 1, al, 256, al, al, nullptr, nullptr, al,
                              al, 1, 4, 3, nullptr), JMT_ERR_ARG, "y dtype");

  // ---- backward, row map
#define BWD(rows, k, h, g0, dh, ws, ldgy, P, Q)                                              \
  jmt_head_bwd_perm(JMT_F16, JMT_F32, rows, 128, k, h, 256, al, al, g0, al, ldgy, dh, 256, fl, \
                    fl, fl, fl, ws, P, Q, nullptr)
  const char* B = "jmt_head_bwd_perm";
  expect_rc("bwd P*Q", BWD(68, 1, al, al, al, fl, 1, 17, 3), JMT_ERR_ARG, "P * Q = rows");
  expect_rc("bwd P 0", BWD(68, 1, al, al, al, fl, 1, 0, 0), JMT_ERR_ARG, "P * Q = rows");
  expect_rc("bwd rows past", BWD(big + 2, 1, al, al, al, fl, 1, big + 2, 1), JMT_ERR_ARG,
            "31 bits");
  expect_rc("bwd name", BWD(68, 1, al, al, al, fl, 1, 17, 3), JMT_ERR_ARG, B);
  expect_rc("bwd null h", BWD(68, 1, nullptr, al, al, fl, 1, 17, 4), JMT_ERR_ARG, "null pointer");
  expect_rc("bwd null gy", BWD(68, 1, al, nullptr, al, fl, 1, 17, 4), JMT_ERR_ARG,
            "bad gradient buffers");
  expect_rc("bwd null dh", BWD(68, 1, al, al, nullptr, fl, 1, 17, 4), JMT_ERR_ARG,
            "bad gradient buffers");
  expect_rc("bwd null workspace", BWD(68, 1, al, al, al, nullptr, 1, 17, 4), JMT_ERR_ARG,
            "bad gradient buffers");
  expect_rc("bwd misaligned dh", BWD(68, 1, al, al, misal, fl, 1, 17, 4), JMT_ERR_ARG,
            "bad gradient buffers");
  expect_rc("bwd k 0", BWD(68, 0, al, al, al, fl, 1, 17, 4), JMT_ERR_ARG, "k = 0");
  expect_rc("bwd k 25", BWD(68, 25, al, al, al, fl, 25, 17, 4), JMT_ERR_ARG, "k = 25");
  expect_rc("bwd ldgy under k", BWD(68, 2, al, al, al, fl, 1, 17, 4), JMT_ERR_ARG,
            "bad gradient buffers");
  expect_eq("bwd rows 0", BWD(0, 1, al, al, al, fl, 1, 1, 1), JMT_OK);

  // ---- the dropout forms: the mask arguments first, then the same checks under their own names
#define FWDD(rows, P, Q, p0, c)                                                                \
  jmt_head_fwd_perm_drop(JMT_BF16, JMT_F32, rows, 128, 1, al, 256, al, al, nullptr, nullptr, al, \
                         al, 1, P, Q, p0, 0.5f, c, nullptr)
#define BWDD(rows, P, Q, p0, c)                                                               \
  jmt_head_bwd_perm_drop(JMT_BF16, JMT_F32, rows, 128, 1, al, 256, al, al, al, al, 1, al, 256, \
                         fl, fl, fl, fl, fl, P, Q, p0, 0.5f, c, nullptr)
  expect_rc("fwd drop null ctr", FWDD(12, 4, 3, 0.3f, nullptr), JMT_ERR_ARG, "null counter");
  expect_rc("fwd drop rate", FWDD(12, 4, 3, 1.f, ctr), JMT_ERR_ARG, "[0, 1)");
  expect_rc("fwd drop P*Q", FWDD(12, 5, 3, 0.3f, ctr), JMT_ERR_ARG,
            "jmt_head_fwd_perm_drop: row map");
  expect_rc("fwd drop rows past", FWDD(big, big, 1, 0.3f, ctr), JMT_ERR_ARG, "31 bits");
  expect_rc("bwd drop null ctr", BWDD(12, 4, 3, 0.3f, nullptr), JMT_ERR_ARG, "null counter");
  expect_rc("bwd drop rate", BWDD(12, 4, 3, -0.1f, ctr), JMT_ERR_ARG, "[0, 1)");
  expect_rc("bwd drop P*Q", BWDD(12, 4, 4, 0.3f, ctr), JMT_ERR_ARG,
            "jmt_head_bwd_perm_drop: row map");

  // ---- the entries without a map keep their names and take no map
  expect_rc("head_fwd name",
            jmt_head_fwd(JMT_BF16, JMT_F32, 12, 128, 0, al, 256, al, al, nullptr, nullptr, al, al,
                         1, nullptr), JMT_ERR_ARG, "jmt_head_fwd: k = 0");

  // ---- CCC statistics + finish in one launch
#define CSF(kind, n, k, pred, lab, st, loss, coef)                                            \
  jmt_ccc_stats_finish(kind, JMT_F32, n, k, pred, lab, -5.f, -1.f, 1.f, st, 1, 1e-8f, loss, coef, \
                       nullptr)
  expect_rc("csf kind", CSF(2, 10, 1, al, fl, db, fl, db), JMT_ERR_ARG, "kind");
  expect_rc("csf bins 0", CSF(0, 10, 0, al, fl, db, fl, db), JMT_ERR_ARG, "digitize_num 0");
  expect_rc("csf bins 65", CSF(0, 10, 65, al, fl, db, fl, db), JMT_ERR_ARG, "digitize_num 65");
  expect_rc("csf negative n", CSF(0, -1, 1, al, fl, db, fl, db), JMT_ERR_ARG, "negative n");
  expect_rc("csf null pred", CSF(0, 10, 1, nullptr, fl, db, fl, db), JMT_ERR_ARG, "null pointer");
  expect_rc("csf null label", CSF(1, 10, 1, al, nullptr, db, fl, db), JMT_ERR_ARG,
            "null pointer");
  expect_rc("csf null stats", CSF(0, 10, 1, al, fl, nullptr, fl, db), JMT_ERR_ARG,
            "null pointer");
  expect_rc("csf null loss", CSF(0, 10, 1, al, fl, db, nullptr, db), JMT_ERR_ARG, "null pointer");
  expect_rc("csf null coef", CSF(0, 10, 1, al, fl, db, fl, nullptr), JMT_ERR_ARG, "null pointer");
  expect_rc("csf dtype",
            jmt_ccc_stats_finish(0, 9, 10, 1, al, fl, -5.f, -1.f, 1.f, db, 1, 1e-8f, fl, db,
                                 nullptr), JMT_ERR_ARG, "dtype");
  expect_rc("csf_add null loss",
            jmt_ccc_stats_finish_add(0, JMT_F32, 10, 1, al, fl, -5.f, -1.f, 1.f, db, 1, 1e-8f, fl,
                                     nullptr, db, nullptr), JMT_ERR_ARG, "null pointer");
  expect_rc("csf_add kind",
            jmt_ccc_stats_finish_add(-1, JMT_F32, 10, 1, al, fl, -5.f, -1.f, 1.f, db, 1, 1e-8f, fl,
                                     fl, db, nullptr), JMT_ERR_ARG, "jmt_ccc_stats_finish: kind");

  if (g_fail) {
    fprintf(stderr, "abi_check_tail: %d failure(s)\n", g_fail);
    return 1;
  }
  printf("abi_check_tail: ok\n");
  return 0;
}
