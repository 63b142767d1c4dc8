// Host-side check of the gradient-norm clipping entry points (jmt_grad_norm,
// jmt_grad_norm_scratch, jmt_adam_step_clip, jmt_sgd_step_dev_clip), built with AddressSanitizer
// by `make asan` next to abi_check_mh and run on the CPU by tests/test_abi_grad_norm.py.  Every
// entry point is driven with arguments it must refuse before a launch (no kernel runs, no GPU is
// needed): each call must return JMT_ERR_ARG and leave a bounded, non-empty jmt_last_error()
// that names the check.
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
  float* fl = (float*)buf;
  float* misal = (float*)(buf + 4);
  double* db = (double*)buf;
  const int64_t* so = (const int64_t*)buf;

  // the scratch query: one double per chunk of 4096 elements, one more chunk per segment
  expect_eq("scratch n 0", jmt_grad_norm_scratch(0, 0), 8);
  expect_eq("scratch one chunk", jmt_grad_norm_scratch(4096, 0), 16);
  expect_eq("scratch segments", jmt_grad_norm_scratch(10 * 4096 + 5, 37), (10 + 37) * 8);
  expect_eq("scratch negative n", jmt_grad_norm_scratch(-1, 0), -1);
  expect_eq("scratch negative nseg", jmt_grad_norm_scratch(64, -1), -1);
  expect_eq("scratch nseg past", jmt_grad_norm_scratch(64, 2049), -1);
  expect_eq("scratch n past", jmt_grad_norm_scratch((int64_t)1 << 42, 0), -1);
  expect_eq("scratch n times nseg past", jmt_grad_norm_scratch((int64_t)1 << 32, 2048), -1);
  expect_eq("scratch n at", jmt_grad_norm_scratch(((int64_t)1 << 42) - 1, 0),
            ((int64_t)1 << 30) * 8);
  const int64_t need = jmt_grad_norm_scratch(1 << 20, 3);

#define GN(n, g, st, sc, bytes, off, nseg, sn) \
  jmt_grad_norm(n, g, st, sc, bytes, off, nseg, sn, 1.f, nullptr, nullptr)
  expect_rc("negative n", GN(-1, fl, fl, db, need, so, 3, fl), JMT_ERR_ARG, "negative n");
  expect_rc("n past", GN((int64_t)1 << 42, fl, fl, db, need, so, 3, fl), JMT_ERR_ARG, "2^30");
  expect_rc("n times nseg past", GN((int64_t)1 << 32, fl, fl, db, need, so, 2048, fl), JMT_ERR_ARG,
            "2^30");
  expect_rc("null grad", GN(1 << 20, nullptr, fl, db, need, so, 3, fl), JMT_ERR_ARG, "null grad");
  expect_rc("null state", GN(1 << 20, fl, nullptr, db, need, so, 3, fl), JMT_ERR_ARG,
            "null state");
  expect_rc("null scratch", GN(1 << 20, fl, fl, nullptr, need, so, 3, fl), JMT_ERR_ARG,
            "null scratch");
  expect_rc("misaligned grad", GN(1 << 20, misal, fl, db, need, so, 3, fl), JMT_ERR_ARG,
            "aligned");
  expect_rc("misaligned scratch", GN(1 << 20, fl, fl, (double*)(buf + 4), need, so, 3, fl),
            JMT_ERR_ARG, "aligned");
  expect_rc("negative nseg", GN(1 << 20, fl, fl, db, need, so, -1, fl), JMT_ERR_ARG,
            "negative nseg");
  expect_rc("nseg past", GN(1 << 20, fl, fl, db, need, so, 2049, fl), JMT_ERR_ARG, "2048");
  expect_rc("null seg_off", GN(1 << 20, fl, fl, db, need, nullptr, 3, fl), JMT_ERR_ARG,
            "null seg_off");
  expect_rc("null seg_norm", GN(1 << 20, fl, fl, db, need, so, 3, nullptr), JMT_ERR_ARG,
            "null seg_norm");
  expect_rc("scratch one short", GN(1 << 20, fl, fl, db, need - 1, so, 3, fl), JMT_ERR_ARG,
            "jmt_grad_norm_scratch asks for");
  expect_rc("scratch of fewer segments", GN(1 << 20, fl, fl, db, jmt_grad_norm_scratch(1 << 20, 0),
                                            so, 3, fl), JMT_ERR_ARG,
            "jmt_grad_norm_scratch asks for");
  expect_rc("scratch 0", GN(0, fl, fl, db, 0, nullptr, 0, nullptr), JMT_ERR_ARG,
            "jmt_grad_norm_scratch asks for");
  expect_rc("scratch negative", GN(64, fl, fl, db, -8, nullptr, 0, nullptr), JMT_ERR_ARG,
            "jmt_grad_norm_scratch asks for");

  // the clipped step entry points: the checks of jmt_adam_step / jmt_sgd_step_dev under their
  // own names
#define ADAM(n, p, g, m, v, vm, st, b1, sh, sdt)                                              \
  jmt_adam_step_clip(n, p, g, m, v, vm, st, b1, 0.999, 1e-8f, 0.f, 1.f, nullptr, 0, sh, sdt, \
                     nullptr)
  const char* A = "jmt_adam_step_clip";
  expect_rc("adam negative n", ADAM(-1, fl, fl, fl, fl, nullptr, fl, 0.9, nullptr, JMT_BF16),
            JMT_ERR_ARG, A);
  expect_rc("adam null grad", ADAM(64, fl, nullptr, fl, fl, nullptr, fl, 0.9, nullptr, JMT_BF16),
            JMT_ERR_ARG, "jmt_adam_step_clip: null pointer");
  expect_rc("adam null state", ADAM(64, fl, fl, fl, fl, nullptr, nullptr, 0.9, nullptr, JMT_BF16),
            JMT_ERR_ARG, "jmt_adam_step_clip: null state");
  expect_rc("adam misaligned", ADAM(64, fl, misal, fl, fl, nullptr, fl, 0.9, nullptr, JMT_BF16),
            JMT_ERR_ARG, "16-B aligned");
  expect_rc("adam misaligned vmax", ADAM(64, fl, fl, fl, fl, misal, fl, 0.9, nullptr, JMT_BF16),
            JMT_ERR_ARG, "16-B aligned");
  expect_rc("adam shadow dtype", ADAM(64, fl, fl, fl, fl, nullptr, fl, 0.9, buf, JMT_F32),
            JMT_ERR_ARG, "shadow_dt");
  expect_rc("adam shadow misaligned", ADAM(64, fl, fl, fl, fl, nullptr, fl, 0.9, buf + 4, JMT_F16),
            JMT_ERR_ARG, "8-B aligned");
  expect_rc("adam beta", ADAM(64, fl, fl, fl, fl, nullptr, fl, 1.0, nullptr, JMT_BF16),
            JMT_ERR_ARG, "betas");
  expect_eq("adam n 0", ADAM(0, fl, fl, fl, fl, nullptr, fl, 0.9, nullptr, JMT_BF16), JMT_OK);

#define SGD(n, p, g, b, st, mom, sh, sdt) \
  jmt_sgd_step_dev_clip(n, p, g, b, st, mom, 0.f, 0.f, 0, 0, 1.f, nullptr, 0, sh, sdt, nullptr)
  expect_rc("sgd negative n", SGD(-1, fl, fl, fl, fl, 0.9f, nullptr, JMT_BF16), JMT_ERR_ARG,
            "jmt_sgd_step_dev_clip: negative n");
  expect_rc("sgd null param", SGD(64, nullptr, fl, fl, fl, 0.9f, nullptr, JMT_BF16), JMT_ERR_ARG,
            "jmt_sgd_step_dev_clip: null pointer");
  expect_rc("sgd null state", SGD(64, fl, fl, fl, nullptr, 0.9f, nullptr, JMT_BF16), JMT_ERR_ARG,
            "jmt_sgd_step_dev_clip: null state");
  expect_rc("sgd momentum without buffer", SGD(64, fl, fl, nullptr, fl, 0.9f, nullptr, JMT_BF16),
            JMT_ERR_ARG, "momentum needs a buffer");
  expect_rc("sgd misaligned buffer", SGD(64, fl, fl, misal, fl, 0.9f, nullptr, JMT_BF16),
            JMT_ERR_ARG, "16-B aligned");
  expect_rc("sgd shadow dtype", SGD(64, fl, fl, fl, fl, 0.9f, buf, 7), JMT_ERR_ARG, "shadow_dt");
  expect_rc("sgd shadow misaligned", SGD(64, fl, fl, fl, fl, 0.9f, buf + 2, JMT_BF16), JMT_ERR_ARG,
            "8-B aligned");
  expect_eq("sgd n 0", SGD(0, fl, fl, fl, fl, 0.9f, nullptr, JMT_BF16), JMT_OK);

  // the entry points without clipping keep their own names in their messages
  expect_rc("adam_step name", jmt_adam_step(-1, fl, fl, fl, fl, nullptr, fl, 0.9, 0.999, 1e-8f, 0.f,
                                            1.f, nullptr, 0, nullptr, JMT_BF16, nullptr),
            JMT_ERR_ARG, "jmt_adam_step: negative n");
  expect_rc("sgd_step_dev name", jmt_sgd_step_dev(-1, fl, fl, fl, fl, 0.9f, 0.f, 0.f, 0, 0, 1.f,
                                                  nullptr, 0, nullptr, JMT_BF16, nullptr),
            JMT_ERR_ARG, "jmt_sgd_step_dev: negative n");

  if (g_fail) {
    fprintf(stderr, "abi_check_grad_norm: %d failure(s)\n", g_fail);
    return 1;
  }
  printf("abi_check_grad_norm: ok\n");
  return 0;
}
