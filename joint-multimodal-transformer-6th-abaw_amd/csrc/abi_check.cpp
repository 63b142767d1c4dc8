// Host-side ABI check, built with AddressSanitizer by `make asan` (host code only: the kernels
// are compiled out with --offload-host-only) and run by tests/test_abi.py on the CPU (SURVEY.md
// §5 "Race detection / sanitizers").  Every entry point of include/jmt.h that validates its
// arguments is driven with invalid ones (null / misaligned pointers, bad sizes, unsupported
// dtypes, oversized tables); each must return a negative JMT_ERR_* and leave a bounded,
// non-empty jmt_last_error() — all in the library's host code (argument checks, planners, error
// formatting), so ASan sees every host-side byte the ABI touches.  No GPU is needed.
#include <stdio.h>
#include <string.h>

#include "../../include/jmt.h"

static int g_fail = 0;

// the error message names the check (not a later failure, e.g. a launch without a device)
static void expect_msg(const char* what, const char* needle) {
  const char* e = jmt_last_error();
  if (!e || !strstr(e, needle)) {
    fprintf(stderr, "FAIL %s: err='%s' lacks '%s'\n", what, e ? e : "(null)", needle);
    ++g_fail;
  }
}

static void expect_err(const char* what, int rc) {
  const char* e = jmt_last_error();
  const size_t n = e ? strnlen(e, 1024) : 0;
  if (rc >= 0 || n == 0 || n >= 512) {
    fprintf(stderr, "FAIL %s: rc=%d err='%s'\n", what, rc, e ? e : "(null)");
    ++g_fail;
  }
}

static void expect_eq(const char* what, int got, int want) {
  if (got != want) {
    fprintf(stderr, "FAIL %s: %d, not %d\n", what, got, want);
    ++g_fail;
  }
}

// refused with exactly `code` and a message that names the check
static void expect_rc(const char* what, int rc, int code, const char* needle) {
  expect_err(what, rc);
  expect_msg(what, needle);
  expect_eq(what, rc, code);
}

// dev switch of the forward, outside include/jmt.h (csrc/attn.hip)
extern "C" int jmt_attn_set_fwd_rows(int on);

int main() {
  if (jmt_abi_version() != JMT_ABI_VERSION) {
    fprintf(stderr, "FAIL abi version\n");
    return 1;
  }
  alignas(16) char buf[64];
  float* fnull = nullptr;
  void* misal = (void*)(buf + 1);
  void* algn = (void*)buf;        // aligned, never dereferenced (the checks fail first)

  // GEMM: descriptor validation and the host planners
  jmt_gemm_desc d;
  memset(&d, 0, sizeof(d));
  d.ab_dtype = JMT_BF16; d.c_dtype = JMT_BF16; d.M = 128; d.N = 128; d.K = 128;
  d.n_a = d.n_b = d.n_c = 1; d.batch0 = d.batch1 = 1; d.lda = d.ldb = d.ldc = 128;
  d.alpha = 1.f;
  expect_err("gemm null operands", jmt_gemm(&d, nullptr));
  d.a[0] = misal; d.b[0] = misal; d.c[0] = misal;
  expect_err("gemm misaligned operands", jmt_gemm(&d, nullptr));
  d.n_a = 9;
  expect_err("gemm pointer table > 8", jmt_gemm(&d, nullptr));
  d.n_a = 1; d.ab_dtype = 7;
  expect_err("gemm dtype", jmt_gemm(&d, nullptr));
  d.ab_dtype = JMT_BF16; d.M = -5;
  expect_err("gemm negative M", jmt_gemm(&d, nullptr));
  // A row sums (ABI 4): table entries, layout and table size are checked before any launch
  d.M = 128; d.a[0] = d.b[0] = d.c[0] = (void*)buf; d.c_dtype = JMT_F32;
  d.a_kmajor = 0; d.b_kmajor = 0; d.n_dbias = 1; d.dbias_tab[0] = nullptr;
  expect_err("gemm dbias null entry", jmt_gemm(&d, nullptr));
  expect_msg("gemm dbias null entry", "every dbias_tab entry");
  d.dbias_tab[0] = (float*)buf; d.a_kmajor = 1;
  expect_err("gemm dbias K-major A", jmt_gemm(&d, nullptr));
  expect_msg("gemm dbias K-major A", "row sums");
  d.a_kmajor = 0; d.n_dbias = 9;
  expect_err("gemm dbias table > 8", jmt_gemm(&d, nullptr));
  expect_msg("gemm dbias table > 8", "dbias table");
  d.n_dbias = 0;
  expect_err("gemm null desc", jmt_gemm(nullptr, nullptr));
  // jmt_gemm_cin: the beta * C operand from another table — refused before any launch
  {
    const void* cin[1] = {algn};
#define CIN_ERR(what, code, needle, set, reset)                                  \
    do {                                                                         \
      set;                                                                       \
      const int rc_ = jmt_gemm_cin(&d, cin, 1, 128, nullptr);                    \
      expect_err(what, rc_);                                                     \
      expect_msg(what, needle);                                                  \
      if (rc_ != code) {                                                         \
        fprintf(stderr, "FAIL %s: rc=%d, not %d\n", what, rc_, (int)code);       \
        ++g_fail;                                                                \
      }                                                                          \
      reset;                                                                     \
    } while (0)
    d.c_dtype = JMT_BF16; d.beta = 1.f;
    CIN_ERR("gemm_cin fp32 C", JMT_ERR_UNSUPPORTED, "16-bit C", d.c_dtype = JMT_F32,
            d.c_dtype = JMT_BF16);
    CIN_ERR("gemm_cin forced splits", JMT_ERR_UNSUPPORTED, "split-K", d.splits = 2, d.splits = 0);
    CIN_ERR("gemm_cin beta 0", JMT_ERR_ARG, "beta == 0", d.beta = 0.f, d.beta = 1.f);
    CIN_ERR("gemm_cin null entry", JMT_ERR_ARG, "c_in[0]", cin[0] = nullptr, cin[0] = algn);
    CIN_ERR("gemm_cin misaligned entry", JMT_ERR_ARG, "c_in[0]", cin[0] = misal, cin[0] = algn);
#undef CIN_ERR
    expect_err("gemm_cin null table", jmt_gemm_cin(&d, nullptr, 1, 128, nullptr));
    expect_msg("gemm_cin null table", "c_in table");
    d.c_mode = 1; d.batch0 = 2; d.n_c = 2; d.c[1] = algn;
    expect_err("gemm_cin short table", jmt_gemm_cin(&d, cin, 1, 128, nullptr));
    expect_msg("gemm_cin short table", "c_in table");
    d.c_mode = 0; d.batch0 = 1; d.n_c = 1;
    expect_err("gemm_cin misaligned ldcin", jmt_gemm_cin(&d, cin, 1, 132, nullptr));
    expect_msg("gemm_cin misaligned ldcin", "ldcin");
    expect_err("gemm_cin null desc", jmt_gemm_cin(nullptr, cin, 1, 128, nullptr));
    d.c_dtype = JMT_F32; d.beta = 0.f;
  }
  size_t ws = 0;
  for (int m = 1; m <= 1 << 16; m *= 7)
    for (int s = 1; s <= 256; s *= 4) ws += jmt_gemm_workspace_bytes(m, 512, 3, s);
  int splits = 0;
  for (int k = 16; k <= 1 << 20; k *= 5)
    splits += jmt_gemm_plan_splits(JMT_BF16, 1024, 512, k, 1) +
              jmt_gemm_plan_splits(JMT_F32, 7, 3, k, 6);
  if (ws == 0 || splits <= 0) {
    fprintf(stderr, "FAIL planners ws=%zu splits=%d\n", ws, splits);
    ++g_fail;
  }
  // grouped weight gradients: everything outside the grouped form is refused before any launch
  {
    jmt_gemm_desc gd[2];
    memset(gd, 0, sizeof(gd));
    for (int i = 0; i < 2; ++i) {
      gd[i].ab_dtype = JMT_BF16; gd[i].c_dtype = JMT_F32; gd[i].M = 512; gd[i].N = 256;
      gd[i].K = 1024 * (i + 1); gd[i].n_a = gd[i].n_b = gd[i].n_c = 1;
      gd[i].batch0 = gd[i].batch1 = 1; gd[i].lda = 512; gd[i].ldb = 256; gd[i].ldc = 256;
      gd[i].alpha = 1.f; gd[i].beta = 1.f; gd[i].a[0] = gd[i].b[0] = gd[i].c[0] = algn;
    }
    int sp[2] = {0, 0};
    if (jmt_gemm_grouped_plan(gd, 2, sp) != JMT_OK || sp[0] < 1 || sp[1] < 1 ||
        jmt_gemm_grouped_workspace_bytes(gd, 2) == 0) {
      fprintf(stderr, "FAIL grouped plan: %s\n", jmt_last_error());
      ++g_fail;
    }
    expect_err("grouped null descs", jmt_gemm_grouped(nullptr, 2, nullptr, 0, nullptr));
    expect_err("grouped 17 problems", jmt_gemm_grouped(gd, 17, nullptr, 0, nullptr));
    expect_err("grouped no workspace", jmt_gemm_grouped(gd, 2, nullptr, 0, nullptr));
    expect_msg("grouped no workspace", "workspace bytes");
#define GRP_UNSUP(what, set, reset)                                              \
    do {                                                                         \
      set;                                                                       \
      const int rc_ = jmt_gemm_grouped(gd, 2, algn, (size_t)1 << 40, nullptr);   \
      expect_err(what, rc_);                                                     \
      if (rc_ != JMT_ERR_UNSUPPORTED) {                                          \
        fprintf(stderr, "FAIL %s: rc=%d, not JMT_ERR_UNSUPPORTED\n", what, rc_); \
        ++g_fail;                                                                \
      }                                                                          \
      reset;                                                                     \
    } while (0)
    GRP_UNSUP("grouped fp32 operands", gd[1].ab_dtype = JMT_F32, gd[1].ab_dtype = JMT_BF16);
    GRP_UNSUP("grouped M % 256", gd[1].M = 384, gd[1].M = 512);
    GRP_UNSUP("grouped N % 256", gd[0].N = 128, gd[0].N = 256);
    GRP_UNSUP("grouped K % 64", gd[0].K = 1000, gd[0].K = 1024);
    GRP_UNSUP("grouped bias", gd[1].bias = (const float*)algn, gd[1].bias = nullptr);
    GRP_UNSUP("grouped relu", gd[0].relu = 1, gd[0].relu = 0);
    GRP_UNSUP("grouped aux", gd[1].aux = algn, gd[1].aux = nullptr);
    GRP_UNSUP("grouped 16-bit C", gd[1].c_dtype = JMT_BF16, gd[1].c_dtype = JMT_F32);
    GRP_UNSUP("grouped mixed majorness", gd[1].a_kmajor = 1, gd[1].a_kmajor = 0);
    GRP_UNSUP("grouped K-concat mode 2", gd[0].a_mode = 2, gd[0].a_mode = 0);
    GRP_UNSUP("grouped batch1", gd[0].batch1 = 2, gd[0].batch1 = 1);
#undef GRP_UNSUP
    gd[0].c[0] = misal;
    expect_err("grouped misaligned C", jmt_gemm_grouped(gd, 2, algn, (size_t)1 << 40, nullptr));
    gd[0].c[0] = algn; gd[0].n_dbias = 1; gd[0].dbias_tab[0] = nullptr;
    expect_err("grouped dbias null entry", jmt_gemm_grouped(gd, 2, algn, (size_t)1 << 40, nullptr));
    expect_msg("grouped dbias null entry", "every dbias_tab entry");
    // row sums no longer force a second split: the plan with a dbias table on both problems
    // is the plan without, and a forced single split is taken
    int sp_rs[2] = {0, 0};
    for (int i = 0; i < 2; ++i) { gd[i].n_dbias = 1; gd[i].dbias_tab[0] = (float*)algn; }
    int rc_rs = jmt_gemm_grouped_plan(gd, 2, sp_rs);
    const bool same = rc_rs == JMT_OK && sp_rs[0] == sp[0] && sp_rs[1] == sp[1];
    gd[1].splits = 1;
    rc_rs = jmt_gemm_grouped_plan(gd, 2, sp_rs);
    if (!same || rc_rs != JMT_OK || sp_rs[1] != 1 ||
        jmt_gemm_grouped_workspace_bytes(gd, 2) == 0) {
      fprintf(stderr, "FAIL grouped plan with row sums: %s (splits %d %d vs %d %d)\n",
              jmt_last_error(), sp_rs[0], sp_rs[1], sp[0], sp[1]);
      ++g_fail;
    }
  }

  // row ops
  expect_err("l2norm_fwd null", jmt_l2norm_fwd(JMT_BF16, JMT_BF16, 8, 512, nullptr, 512, nullptr,
                                               512, fnull, 1e-12f, nullptr));
  expect_err("layernorm_fwd dtype", jmt_layernorm_fwd(9, JMT_BF16, 8, 512, misal, 512, nullptr, 0,
                                                      fnull, fnull, 1e-5f, misal, 512, fnull,
                                                      fnull, nullptr));
  expect_err("softmax_fwd null", jmt_softmax_fwd(JMT_BF16, 8, 300, nullptr, 304, 1.f, nullptr, 304,
                                                 nullptr));
  expect_err("colsum null", jmt_colsum(JMT_BF16, 64, 512, nullptr, 512, fnull, 0, fnull, nullptr));
  expect_err("copy2d dtype", jmt_copy2d(5, 6, 4, 4, misal, 4, 1, misal, 4, 1, 0, nullptr));

  // attention
  expect_err("attn_fwd head dim", jmt_attn_fwd(JMT_BF16, 2, 1, 300, 300, 64, misal, 512, 512,
                                               misal, 512, 512, misal, 512, 512, misal, 512, 512,
                                               0.1f, fnull, nullptr));
  expect_err("attn_fwd misaligned", jmt_attn_fwd(JMT_BF16, 2, 1, 300, 300, 512, misal, 512, 512,
                                                 misal, 512, 512, misal, 512, 512, misal, 512,
                                                 512, 0.1f, fnull, nullptr));
  expect_err("attn_bwd sizes", jmt_attn_bwd(JMT_BF16, -1, 1, 300, 300, 512, misal, 1, 1, misal, 1,
                                            1, misal, 1, 1, misal, 1, 1, misal, 1, 1, fnull,
                                            misal, misal, 8, misal, 1, 1, 0.1f, nullptr));
  expect_err("attn_dkdv ldp", jmt_attn_dkdv(JMT_BF16, 2, 1, 300, 300, 512, misal, misal, 320,
                                           misal, 512, 512, misal, 512, 512, nullptr, 0, 0,
                                           misal, 512, 512, misal, 512, 512, nullptr, 0, 0,
                                           nullptr));
  expect_err("attn_dkdv head dim", jmt_attn_dkdv(JMT_BF16, 2, 1, 300, 300, 64, misal, misal, 384,
                                                 misal, 512, 512, misal, 512, 512, nullptr, 0, 0,
                                                 misal, 512, 512, misal, 512, 512, nullptr, 0,
                                                 0, nullptr));
  expect_err("attn_dkdv dq misaligned", jmt_attn_dkdv(JMT_BF16, 2, 1, 300, 300, 512, algn, algn,
                                                      384, algn, 512, 512, algn, 512, 512, misal,
                                                      512, 512, algn, 512, 512, algn, 512, 512,
                                                      misal, 512, 512, nullptr));
  // tile-major P / dS (dq != NULL): ldp covers 128-key tiles but is no multiple of 32
  expect_err("attn_dkdv dq ldp % 32", jmt_attn_dkdv(JMT_BF16, 2, 1, 300, 300, 512, algn, algn,
                                                    392, algn, 512, 512, algn, 512, 512, algn,
                                                    512, 512, algn, 512, 512, algn, 512, 512,
                                                    algn, 512, 512, nullptr));
  if (jmt_attn_dkdv_plan(300, 300, 1, 512, 512, 512, 1) != 160 ||
      jmt_attn_dkdv_plan(300, 300, 1, 512, 512, 512, 0) != 128 ||
      jmt_attn_dkdv_plan(256, 256, 1, 512, 512, 512, 1) != 128) {
    fprintf(stderr, "FAIL attn_dkdv_plan\n");
    ++g_fail;
  }
  expect_err("attn_bwd pds ldp", jmt_attn_bwd(JMT_BF16, 2, 1, 300, 300, 512, algn, 512, 512,
                                              algn, 512, 512, algn, 512, 512, algn, 512, 512,
                                              algn, 512, 512, fnull, algn, algn, 300, nullptr,
                                              0, 0, 0.1f, nullptr));
  // The ranges of the attention kernels (jmt_attn_*_ok): one geometry just inside and one just
  // outside each limit of include/jmt.h, the expected answers as literals; the entry point
  // refuses every outside geometry (aligned dummy operands) before a launch.
  {
    const int64_t S20 = 1 << 20, S23 = 1 << 23;   // 1024 rows x 2^20 x 2 B = 128 x 2^23 x 2 B = 2 GiB
    const int id2[2] = {0, 1};
#define FWD_SQ(N, H, Lq, Lk, sk, sv, spp)                                                     \
    jmt_attn_fwd_sq(JMT_BF16, N, H, Lq, Lk, 512, algn, 512, 512, algn, sk, 512, algn, sv, 512,  \
                    algn, 512, 512, 0.1f, fnull, spp, id2, 2, nullptr)
#define BWD_PDS(N, H, Lq, Lk, ldp, sk, sv)                                                    \
    jmt_attn_bwd(JMT_BF16, N, H, Lq, Lk, 512, algn, 512, 512, algn, 512, 512, algn, 512, 512,   \
                 algn, sk, 512, algn, sv, 512, (const float*)algn, algn, algn, ldp, nullptr, 0, \
                 0, 0.1f, nullptr)
#define DKDV(N, H, Lq, Lk, ldp, sgo, sq, sk, sdk, sdv, sdq, dq)                               \
    jmt_attn_dkdv(JMT_BF16, N, H, Lq, Lk, 512, algn, algn, ldp, algn, sgo, 512, algn, sq, 512,  \
                  algn, sk, 512, algn, sdk, 512, algn, sdv, 512, (dq) ? algn : nullptr, sdq,    \
                  512, nullptr)
    // whole-row forward: Lq > 64, Lk K / V rows below 2 GiB, items, the forward-rows switch
    expect_eq("fwd_rows Lq 65", jmt_attn_fwd_rows_ok(2, 1, 65, 300, 512, 512), 1);
    expect_eq("fwd_rows Lq 64", jmt_attn_fwd_rows_ok(2, 1, 64, 300, 512, 512), 0);
    expect_rc("fwd_sq Lq 64", FWD_SQ(2, 1, 64, 300, 512, 512, 1), JMT_ERR_UNSUPPORTED, "whole-row");
    expect_eq("fwd_rows K in", jmt_attn_fwd_rows_ok(2, 1, 300, 1024, S20 - 8, 512), 1);
    expect_eq("fwd_rows K out", jmt_attn_fwd_rows_ok(2, 1, 300, 1024, S20, 512), 0);
    expect_rc("fwd_sq K out", FWD_SQ(2, 1, 300, 1024, S20, 512, 1), JMT_ERR_UNSUPPORTED,
              "whole-row");
    expect_eq("fwd_rows V in", jmt_attn_fwd_rows_ok(2, 1, 300, 1024, 512, S20 - 8), 1);
    expect_eq("fwd_rows V out", jmt_attn_fwd_rows_ok(2, 1, 300, 1024, 512, S20), 0);
    expect_rc("fwd_sq V out", FWD_SQ(2, 1, 300, 1024, 512, S20, 1), JMT_ERR_UNSUPPORTED,
              "whole-row");
    expect_eq("fwd_rows items in", jmt_attn_fwd_rows_ok((1 << 24) - 2, 128, 65, 300, 512, 512), 1);
    expect_eq("fwd_rows items out", jmt_attn_fwd_rows_ok(1 << 24, 128, 65, 300, 512, 512), 0);
    expect_rc("fwd_sq items out", FWD_SQ(1 << 24, 128, 65, 300, 512, 512, 1 << 23), JMT_ERR_ARG,
              "bad sizes");
    jmt_attn_set_fwd_rows(0);
    expect_eq("fwd_rows switched off", jmt_attn_fwd_rows_ok(2, 1, 300, 300, 512, 512), 0);
    expect_rc("fwd_sq switched off", FWD_SQ(2, 1, 300, 300, 512, 512, 1), JMT_ERR_UNSUPPORTED,
              "whole-row");
    jmt_attn_set_fwd_rows(-1);
    expect_eq("fwd_rows switch reset", jmt_attn_fwd_rows_ok(2, 1, 300, 300, 512, 512), 1);
    // P / dS backward: ldp a multiple of 32 covering Lk, (Lq + 128) ldp 16-bit values below
    // 1 GiB, Lk K / V rows below 2 GiB
    expect_eq("pds in", jmt_attn_bwd_pds_ok(2, 1, 300, 300, 320, 512, 512), 1);
    expect_eq("pds ldp % 32", jmt_attn_bwd_pds_ok(2, 1, 300, 300, 328, 512, 512), 0);
    expect_rc("bwd pds ldp % 32", BWD_PDS(2, 1, 300, 300, 328, 512, 512), JMT_ERR_ARG, "ldp");
    expect_eq("pds ldp cover in", jmt_attn_bwd_pds_ok(2, 1, 300, 289, 320, 512, 512), 1);
    expect_eq("pds ldp cover out", jmt_attn_bwd_pds_ok(2, 1, 300, 321, 320, 512, 512), 0);
    expect_rc("bwd pds ldp cover", BWD_PDS(2, 1, 300, 321, 320, 512, 512), JMT_ERR_ARG, "ldp");
    expect_eq("pds 1 GiB in", jmt_attn_bwd_pds_ok(1, 1, 16255, 300, 32768, 512, 512), 1);
    expect_eq("pds 1 GiB out", jmt_attn_bwd_pds_ok(1, 1, 16256, 300, 32768, 512, 512), 0);
    expect_rc("bwd pds 1 GiB", BWD_PDS(1, 1, 16256, 300, 32768, 512, 512), JMT_ERR_ARG, "1 GiB");
    expect_eq("pds K in", jmt_attn_bwd_pds_ok(1, 1, 300, 1024, 1024, S20 - 8, 512), 1);
    expect_eq("pds K out", jmt_attn_bwd_pds_ok(1, 1, 300, 1024, 1024, S20, 512), 0);
    expect_rc("bwd pds K", BWD_PDS(1, 1, 300, 1024, 1024, S20, 512), JMT_ERR_ARG, "2 GiB");
    expect_eq("pds V out", jmt_attn_bwd_pds_ok(1, 1, 300, 1024, 1024, 512, S20), 0);
    expect_rc("bwd pds V", BWD_PDS(1, 1, 300, 1024, 1024, 512, S20), JMT_ERR_ARG, "2 GiB");
    expect_eq("pds items in", jmt_attn_bwd_pds_ok((1 << 24) - 2, 128, 65, 33, 64, 512, 512), 1);
    expect_eq("pds items out", jmt_attn_bwd_pds_ok(1 << 24, 128, 65, 33, 64, 512, 512), 0);
    expect_rc("bwd pds items", BWD_PDS(1 << 24, 128, 65, 33, 64, 512, 512), JMT_ERR_ARG,
              "bad sizes");
    // dK / dV (/ dQ)
    expect_eq("dkdv in", jmt_attn_dkdv_ok(2, 1, 300, 300, 384, 512, 512, 512, 512, 512, 512, 1), 1);
    expect_eq("dkdv in, no dq", jmt_attn_dkdv_ok(2, 1, 300, 300, 384, 512, 512, 0, 512, 512, 0, 0), 1);
    expect_eq("dkdv ldp cover", jmt_attn_dkdv_ok(2, 1, 300, 300, 320, 512, 512, 0, 512, 512, 0, 0), 0);
    expect_rc("dkdv ldp cover", DKDV(2, 1, 300, 300, 320, 512, 512, 0, 512, 512, 0, 0), JMT_ERR_ARG,
              "128-key tiles");
    expect_eq("dkdv dK stride in",
              jmt_attn_dkdv_ok(2, 1, 300, 300, 384, 512, 512, 0, S23 - 8, S23 - 8, 0, 0), 1);
    expect_eq("dkdv dK stride out",
              jmt_attn_dkdv_ok(2, 1, 300, 300, 384, 512, 512, 0, S23, 512, 0, 0), 0);
    expect_rc("dkdv dK stride out", DKDV(2, 1, 300, 300, 384, 512, 512, 0, S23, 512, 0, 0),
              JMT_ERR_ARG, "dK / dV row stride");
    expect_eq("dkdv dV stride out",
              jmt_attn_dkdv_ok(2, 1, 300, 300, 384, 512, 512, 0, 512, S23, 0, 0), 0);
    expect_eq("dkdv dK stride below the heads",
              jmt_attn_dkdv_ok(2, 2, 300, 300, 384, 1024, 1024, 0, 1016, 1024, 0, 0), 0);
    expect_rc("dkdv dK stride below the heads",
              DKDV(2, 2, 300, 300, 384, 1024, 1024, 0, 1016, 1024, 0, 0), JMT_ERR_ARG,
              "dK / dV row stride");
    expect_eq("dkdv dQ stride in",
              jmt_attn_dkdv_ok(2, 1, 300, 300, 384, 512, 512, 512, 512, 512, S23 - 8, 1), 1);
    expect_eq("dkdv dQ stride out",
              jmt_attn_dkdv_ok(2, 1, 300, 300, 384, 512, 512, 512, 512, 512, S23, 1), 0);
    expect_eq("dkdv dQ stride unused",
              jmt_attn_dkdv_ok(2, 1, 300, 300, 384, 512, 512, 512, 512, 512, S23, 0), 1);
    expect_rc("dkdv dQ stride out", DKDV(2, 1, 300, 300, 384, 512, 512, 512, 512, 512, S23, 1),
              JMT_ERR_ARG, "dQ / K row stride");
    expect_eq("dkdv K rows in",
              jmt_attn_dkdv_ok(1, 1, 300, 1024, 1024, 512, 512, S20 - 8, 512, 512, 512, 1), 1);
    expect_eq("dkdv K rows out",
              jmt_attn_dkdv_ok(1, 1, 300, 1024, 1024, 512, 512, S20, 512, 512, 512, 1), 0);
    expect_rc("dkdv K rows out", DKDV(1, 1, 300, 1024, 1024, 512, 512, S20, 512, 512, 512, 1),
              JMT_ERR_ARG, "dQ / K row stride");
    expect_eq("dkdv ldp % 32, no dq",
              jmt_attn_dkdv_ok(2, 1, 300, 300, 392, 512, 512, 0, 512, 512, 0, 0), 1);
    expect_eq("dkdv ldp % 32",
              jmt_attn_dkdv_ok(2, 1, 300, 300, 392, 512, 512, 512, 512, 512, 512, 1), 0);
    expect_eq("dkdv dO rows in",
              jmt_attn_dkdv_ok(1, 1, 1024, 300, 384, S20 - 8, 512, 0, 512, 512, 0, 0), 1);
    expect_eq("dkdv dO rows out",
              jmt_attn_dkdv_ok(1, 1, 1024, 300, 384, S20, 512, 0, 512, 512, 0, 0), 0);
    expect_rc("dkdv dO rows out", DKDV(1, 1, 1024, 300, 384, S20, 512, 0, 512, 512, 0, 0),
              JMT_ERR_ARG, "exceed 2 GiB");
    expect_eq("dkdv Q rows out",
              jmt_attn_dkdv_ok(1, 1, 1024, 300, 384, 512, S20, 0, 512, 512, 0, 0), 0);
    expect_eq("dkdv P rows in",
              jmt_attn_dkdv_ok(1, 1, 32767, 32768, 32768, 512, 512, 0, 512, 512, 0, 0), 1);
    expect_eq("dkdv P rows out",
              jmt_attn_dkdv_ok(1, 1, 32768, 32768, 32768, 512, 512, 0, 512, 512, 0, 0), 0);
    // items of the planned tile: Lq = Lk = 300 with dQ is 6 items of 160 rows per head (9 of
    // 128), Lq = Lk = 128 with dQ 3 of 128, without dQ 2
    expect_eq("dkdv items in, 160 rows",
              jmt_attn_dkdv_ok(357913941, 1, 300, 300, 384, 512, 512, 512, 512, 512, 512, 1), 1);
    expect_eq("dkdv items out, 160 rows",
              jmt_attn_dkdv_ok(357913942, 1, 300, 300, 384, 512, 512, 512, 512, 512, 512, 1), 0);
    expect_rc("dkdv items out, 160 rows",
              DKDV(357913942, 1, 300, 300, 384, 512, 512, 512, 512, 512, 512, 1), JMT_ERR_ARG,
              "too many items");
    expect_eq("dkdv items in, 128 rows",
              jmt_attn_dkdv_ok(715827882, 1, 128, 128, 128, 512, 512, 512, 512, 512, 512, 1), 1);
    expect_eq("dkdv items out, 128 rows",
              jmt_attn_dkdv_ok(715827883, 1, 128, 128, 128, 512, 512, 512, 512, 512, 512, 1), 0);
    expect_eq("dkdv items in, no dq",
              jmt_attn_dkdv_ok((1 << 30) - 1, 1, 128, 128, 128, 512, 512, 0, 512, 512, 0, 0), 1);
    expect_eq("dkdv items out, no dq",
              jmt_attn_dkdv_ok(1 << 30, 1, 128, 128, 128, 512, 512, 0, 512, 512, 0, 0), 0);
    expect_rc("dkdv items out, no dq",
              DKDV(1 << 30, 1, 128, 128, 128, 512, 512, 0, 512, 512, 0, 0), JMT_ERR_ARG,
              "too many items");
#undef FWD_SQ
#undef BWD_PDS
#undef DKDV
  }
  // shared queries: the table is checked before anything else of the launch
  {
    const int id2[2] = {0, 1}, fwd[2] = {1, 1}, chain[3] = {0, 0, 1}, three[3] = {0, 0, 0};
    const int big[9] = {0, 1, 2, 3, 4, 5, 6, 7, 8};
    expect_err("attn_fwd_sq fp32", jmt_attn_fwd_sq(JMT_F32, 2, 1, 300, 300, 512, algn, 512, 512,
                                                   algn, 512, 512, algn, 512, 512, algn, 512, 512,
                                                   0.1f, fnull, 1, id2, 2, nullptr));
    expect_err("attn_fwd_sq Lq 64", jmt_attn_fwd_sq(JMT_BF16, 2, 1, 64, 300, 512, algn, 512, 512,
                                                    algn, 512, 512, algn, 512, 512, algn, 512,
                                                    512, 0.1f, fnull, 1, id2, 2, nullptr));
    expect_err("attn_fwd_sq null table", jmt_attn_fwd_sq(JMT_BF16, 2, 1, 300, 300, 512, algn, 512,
                                                         512, algn, 512, 512, algn, 512, 512,
                                                         algn, 512, 512, 0.1f, fnull, 1, nullptr,
                                                         2, nullptr));
    expect_err("attn_fwd_sq N != npair spp", jmt_attn_fwd_sq(JMT_BF16, 3, 1, 300, 300, 512, algn,
                                                             512, 512, algn, 512, 512, algn, 512,
                                                             512, algn, 512, 512, 0.1f, fnull, 1,
                                                             id2, 2, nullptr));
    expect_err("attn_fwd_sq 9 pairs", jmt_attn_fwd_sq(JMT_BF16, 9, 1, 300, 300, 512, algn, 512,
                                                      512, algn, 512, 512, algn, 512, 512, algn,
                                                      512, 512, 0.1f, fnull, 1, big, 9, nullptr));
    expect_err("attn_fwd_sq forward source", jmt_attn_fwd_sq(JMT_BF16, 2, 1, 300, 300, 512, algn,
                                                             512, 512, algn, 512, 512, algn, 512,
                                                             512, algn, 512, 512, 0.1f, fnull, 1,
                                                             fwd, 2, nullptr));
    expect_err("attn_bwd_sq chained source", jmt_attn_bwd_sq(JMT_BF16, 3, 1, 300, 300, 512, algn,
                                                             512, 512, algn, 512, 512, algn, 512,
                                                             512, algn, 512, 512, algn, 512, 512,
                                                             fnull, algn, algn, 384, 0.1f, 1,
                                                             chain, 3, nullptr));
    expect_err("attn_bwd_sq ldp", jmt_attn_bwd_sq(JMT_BF16, 2, 1, 300, 300, 512, algn, 512, 512,
                                                  algn, 512, 512, algn, 512, 512, algn, 512, 512,
                                                  algn, 512, 512, fnull, algn, algn, 300, 0.1f, 1,
                                                  id2, 2, nullptr));
    expect_err("attn_dkdv_sq dq null", jmt_attn_dkdv_sq(JMT_BF16, 2, 1, 300, 300, 512, algn, algn,
                                                        384, algn, 512, 512, algn, 512, 512, algn,
                                                        512, 512, algn, 512, 512, algn, 512, 512,
                                                        nullptr, 0, 0, 1, id2, 2, 0, nullptr));
    expect_err("attn_dkdv_sq spp 0", jmt_attn_dkdv_sq(JMT_BF16, 2, 1, 300, 300, 512, algn, algn,
                                                      384, algn, 512, 512, algn, 512, 512, algn,
                                                      512, 512, algn, 512, 512, algn, 512, 512,
                                                      algn, 512, 512, 0, id2, 2, 0, nullptr));
    // merged dQ: a query used three times, and one used once
    expect_err("attn_dkdv_sq merge 3 uses", jmt_attn_dkdv_sq(JMT_BF16, 3, 1, 300, 300, 512, algn,
                                                             algn, 384, algn, 512, 512, algn, 512,
                                                             512, algn, 512, 512, algn, 512, 512,
                                                             algn, 512, 512, algn, 512, 512, 1,
                                                             three, 3, 1, nullptr));
    expect_err("attn_dkdv_sq merge 1 use", jmt_attn_dkdv_sq(JMT_BF16, 2, 1, 300, 300, 512, algn,
                                                            algn, 384, algn, 512, 512, algn, 512,
                                                            512, algn, 512, 512, algn, 512, 512,
                                                            algn, 512, 512, algn, 512, 512, 1, id2,
                                                            2, 1, nullptr));
  }
  // key ranges: the table arguments are checked on the host, and shapes the range kernels do
  // not take are refused before anything is launched
  {
    alignas(8) const int krt[4] = {0, 300, 5, 290};
    const int id2[2] = {0, 1};
#define FWD_KR(N_, Lq_, kr_, mod_)                                                              \
  jmt_attn_fwd_kr(JMT_BF16, N_, 1, Lq_, 300, 512, algn, 512, 512, algn, 512, 512, algn, 512, 512, \
                  algn, 512, 512, 0.1f, fnull, kr_, mod_, nullptr)
#define BWD_KR(N_, kr_, mod_)                                                                   \
  jmt_attn_bwd_kr(JMT_BF16, N_, 1, 300, 300, 512, algn, 512, 512, algn, 512, 512, algn, 512, 512, \
                  algn, 512, 512, algn, 512, 512, fnull1, algn, algn, 384, 0.1f, kr_, mod_, nullptr)
    const float* fnull1 = (const float*)algn;
    expect_rc("attn_fwd_kr null table", FWD_KR(2, 300, nullptr, 2), JMT_ERR_ARG, "key range table");
    expect_rc("attn_fwd_kr kr_mod 0", FWD_KR(2, 300, krt, 0), JMT_ERR_ARG, "kr_mod");
    expect_rc("attn_fwd_kr N % kr_mod", FWD_KR(3, 300, krt, 2), JMT_ERR_ARG, "kr_mod");
    expect_err("attn_fwd_kr misaligned table", FWD_KR(2, 300, krt + 1, 1));
    expect_rc("attn_fwd_kr Lq 64 (64-row kernel)", FWD_KR(2, 64, krt, 2), JMT_ERR_UNSUPPORTED,
              "whole-row kernel only");
    expect_err("attn_bwd_kr null table", BWD_KR(2, nullptr, 2));
    expect_rc("attn_bwd_kr N % kr_mod", BWD_KR(3, krt, 2), JMT_ERR_ARG, "kr_mod");
    expect_err("attn_fwd_sq_kr null table",
               jmt_attn_fwd_sq_kr(JMT_BF16, 2, 1, 300, 300, 512, algn, 512, 512, algn, 512, 512,
                                  algn, 512, 512, algn, 512, 512, 0.1f, fnull, 1, id2, 2, nullptr,
                                  2, nullptr));
    expect_err("attn_bwd_sq_kr kr_mod 0",
               jmt_attn_bwd_sq_kr(JMT_BF16, 2, 1, 300, 300, 512, algn, 512, 512, algn, 512, 512,
                                  algn, 512, 512, algn, 512, 512, algn, 512, 512, fnull1, algn,
                                  algn, 384, 0.1f, 1, id2, 2, krt, 0, nullptr));
    expect_err("attn_short_fwd_kr null table",
               jmt_attn_short_fwd_kr(JMT_BF16, 2, 1, 16, 16, 512, algn, 512, 512, algn, 512, 512,
                                     algn, 512, 512, algn, 512, 512, 0.1f, fnull, nullptr, 2,
                                     nullptr));
    expect_err("attn_short_fwd_kr Lk 33",
               jmt_attn_short_fwd_kr(JMT_BF16, 2, 1, 16, 33, 512, algn, 512, 512, algn, 512, 512,
                                     algn, 512, 512, algn, 512, 512, 0.1f, fnull, krt, 2, nullptr));
    expect_err("attn_short_bwd_kr N % kr_mod",
               jmt_attn_short_bwd_kr(JMT_BF16, 3, 1, 16, 16, 512, algn, 512, 512, algn, 512, 512,
                                     algn, 512, 512, algn, 512, 512, algn, 512, 512, fnull1, algn,
                                     512, 512, algn, 512, 512, algn, 512, 512, 0.1f, krt, 2,
                                     nullptr));
    expect_err("softmax_fwd_kr null table",
               jmt_softmax_fwd_kr(JMT_BF16, 8, 300, fnull1, 304, 1.f, algn, 304, nullptr, 2, 4,
                                  nullptr));
    expect_err("softmax_fwd_kr sequences % kr_mod",
               jmt_softmax_fwd_kr(JMT_BF16, 12, 300, fnull1, 304, 1.f, algn, 304, krt, 2, 4,
                                  nullptr));
    expect_err("kpm_ranges null", jmt_kpm_ranges(2, 300, nullptr, 300, nullptr, nullptr, nullptr));
    expect_err("kpm_ranges ld < Lk", jmt_kpm_ranges(2, 300, algn, 200, (int*)algn, (int*)algn,
                                                    nullptr));
#undef FWD_KR
#undef BWD_KR
  }
  expect_err("small_attn_fwd null", jmt_small_attn_fwd(JMT_BF16, 4, 1, 6, 6, 512, nullptr, 512,
                                                       512, nullptr, 512, 512, nullptr, 512, 512,
                                                       nullptr, 512, 512, 0.1f, fnull, nullptr));

  // losses
  expect_err("ccc_stats kind", jmt_ccc_stats(3, JMT_F32, 10, 1, misal, fnull, 0.f, -1.f, 1.f,
                                             nullptr, nullptr));
  expect_err("ccc_stats bins", jmt_ccc_stats(0, JMT_F32, 10, 100, misal, fnull, 0.f, -1.f, 1.f,
                                             (double*)buf, nullptr));
  expect_err("ccc_finish null", jmt_ccc_finish(0, 0, nullptr, 1, 1e-8f, fnull, nullptr, nullptr));
  expect_err("ccc_finish_add null", jmt_ccc_finish_add(0, 1, nullptr, 1, 1e-8f, fnull, fnull,
                                                       nullptr, nullptr));
  expect_err("ce_stats bins", jmt_ce_stats(JMT_F32, 10, 1, misal, fnull, -1.f, 1.f, fnull,
                                           (double*)buf, nullptr));
  expect_err("ce_bwd null", jmt_ce_bwd(JMT_F32, 10, 5, nullptr, fnull, -1.f, 1.f, fnull, nullptr,
                                       fnull, nullptr, nullptr));
  expect_err("ce_labels null", jmt_ce_labels(10, 5, fnull, -1.f, 1.f, nullptr, nullptr));
  expect_err("mask_indices null", jmt_mask_indices(10, fnull, -5.f, nullptr, nullptr, nullptr));

  // optimizer, validation post-processing, feature store
  expect_err("sgd null", jmt_sgd_step(10, fnull, fnull, fnull, 0.1f, 0.9f, 0.f, 0.f, 1, 1, 1.f,
                                      nullptr, JMT_BF16, nullptr));
  expect_err("sgd_zero null", jmt_sgd_step_zero(10, fnull, nullptr, fnull, 0.1f, 0.9f, 0.f, 0.f,
                                                1, 1, 1.f, nullptr, JMT_BF16, nullptr));
  expect_err("sgd_amp_zero null", jmt_sgd_step_amp_zero(10, fnull, fnull, fnull, 0.1f, 0.9f,
                                                        0.f, 0.f, 1, 1, nullptr, nullptr,
                                                        JMT_BF16, nullptr));
  // device-resident optimizer state: tick, Adam, SGD with lr = state[0]
  float* fal = (float*)algn;
  expect_err("opt_tick null state", jmt_opt_tick(nullptr, 0.9, 0.999, nullptr, nullptr));
  expect_msg("opt_tick null state", "null state");
  expect_err("opt_tick beta", jmt_opt_tick(fal, 1.0, 0.999, nullptr, nullptr));
  expect_err("adam null param", jmt_adam_step(10, fnull, fal, fal, fal, nullptr, fal, 0.9, 0.999,
                                              1e-8f, 0.f, 1.f, nullptr, 0, nullptr, JMT_BF16,
                                              nullptr));
  expect_msg("adam null param", "null pointer");
  expect_err("adam null moments", jmt_adam_step(10, fal, fal, fnull, fnull, nullptr, fal, 0.9,
                                                0.999, 1e-8f, 0.f, 1.f, nullptr, 0, nullptr,
                                                JMT_BF16, nullptr));
  expect_err("adam null state", jmt_adam_step(10, fal, fal, fal, fal, nullptr, nullptr, 0.9,
                                              0.999, 1e-8f, 0.f, 1.f, nullptr, 0, nullptr,
                                              JMT_BF16, nullptr));
  expect_msg("adam null state", "null state");
  expect_err("adam amsgrad null state", jmt_adam_step(10, fal, fal, fal, fal, fal, nullptr, 0.9,
                                                      0.999, 1e-8f, 0.f, 1.f, nullptr, 1, nullptr,
                                                      JMT_BF16, nullptr));
  expect_msg("adam amsgrad null state", "null state");
  expect_err("adam misaligned param", jmt_adam_step(10, (float*)(buf + 4), fal, fal, fal, nullptr,
                                                    fal, 0.9, 0.999, 1e-8f, 0.f, 1.f, nullptr, 0,
                                                    nullptr, JMT_BF16, nullptr));
  expect_msg("adam misaligned param", "16-B aligned");
  expect_err("adam shadow_dt", jmt_adam_step(10, fal, fal, fal, fal, nullptr, fal, 0.9, 0.999,
                                             1e-8f, 0.f, 1.f, nullptr, 0, algn, JMT_F32, nullptr));
  expect_msg("adam shadow_dt", "shadow_dt");
  expect_err("adam misaligned shadow", jmt_adam_step(10, fal, fal, fal, fal, nullptr, fal, 0.9,
                                                     0.999, 1e-8f, 0.f, 1.f, nullptr, 0,
                                                     (void*)(buf + 2), JMT_BF16, nullptr));
  expect_msg("adam misaligned shadow", "8-B aligned");
  expect_err("sgd_dev null", jmt_sgd_step_dev(10, fnull, fal, fal, fal, 0.9f, 0.f, 0.f, 1, 1, 1.f,
                                              nullptr, 0, nullptr, JMT_BF16, nullptr));
  expect_err("sgd_dev null state", jmt_sgd_step_dev(10, fal, fal, fal, nullptr, 0.9f, 0.f, 0.f, 1,
                                                    1, 1.f, nullptr, 1, nullptr, JMT_BF16,
                                                    nullptr));
  expect_msg("sgd_dev null state", "null state");
  expect_err("sgd_dev momentum buffer", jmt_sgd_step_dev(10, fal, fal, fnull, fal, 0.9f, 0.f, 0.f,
                                                         1, 1, 1.f, nullptr, 0, nullptr, JMT_BF16,
                                                         nullptr));
  expect_err("sgd_dev misaligned param", jmt_sgd_step_dev(10, (float*)(buf + 4), fal, fal, fal,
                                                          0.9f, 0.f, 0.f, 1, 1, 1.f, nullptr, 0,
                                                          nullptr, JMT_BF16, nullptr));
  expect_msg("sgd_dev misaligned param", "16-B aligned");
  expect_err("sgd_dev shadow_dt", jmt_sgd_step_dev(10, fal, fal, fal, fal, 0.9f, 0.f, 0.f, 1, 1,
                                                   1.f, nullptr, 0, algn, 9, nullptr));
  expect_msg("sgd_dev shadow_dt", "shadow_dt");
  expect_err("vp_ccc null", jmt_vp_ccc(10, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
  expect_err("gather null", jmt_gather_rows(JMT_F32, JMT_BF16, 4, 512, nullptr, 512, 4, nullptr,
                                            nullptr, 512, nullptr));

  // regressor dropout: state tick, mask kernel, the head kernels' DROP entries, host reference
  {
    uint32_t* ual = (uint32_t*)algn;
    const int64_t big = (int64_t)1 << 32;
    expect_rc("dropout_next null state", jmt_dropout_next(nullptr, ual, nullptr), JMT_ERR_ARG,
              "null state");
    expect_rc("dropout_next null out", jmt_dropout_next(ual, nullptr, nullptr), JMT_ERR_ARG,
              "null out");
    expect_rc("dropout null ctr", jmt_dropout(JMT_BF16, algn, 256, algn, 256, 8, 256, 128, 0.3f,
                                              0.5f, nullptr, nullptr), JMT_ERR_ARG,
              "null counter");
    expect_rc("dropout p = 1", jmt_dropout(JMT_BF16, algn, 256, algn, 256, 8, 256, 128, 0.3f,
                                           1.0f, ual, nullptr), JMT_ERR_ARG, "[0, 1)");
    expect_rc("dropout negative p", jmt_dropout(JMT_BF16, algn, 256, algn, 256, 8, 256, 128,
                                                -0.1f, 0.5f, ual, nullptr), JMT_ERR_ARG,
              "[0, 1)");
    expect_rc("dropout cols 6", jmt_dropout(JMT_BF16, algn, 8, algn, 8, 8, 6, 4, 0.3f, 0.5f, ual,
                                            nullptr), JMT_ERR_ARG, "multiple of 4");
    expect_rc("dropout split 6", jmt_dropout(JMT_BF16, algn, 8, algn, 8, 8, 8, 6, 0.3f, 0.5f,
                                             ual, nullptr), JMT_ERR_ARG, "split");
    expect_rc("dropout misaligned", jmt_dropout(JMT_BF16, (void*)(buf + 2), 256, algn, 256, 8,
                                                256, 128, 0.3f, 0.5f, ual, nullptr), JMT_ERR_ARG,
              "8-B aligned");
    expect_rc("dropout odd f32 stride", jmt_dropout(JMT_F32, algn, 257, algn, 256, 8, 256, 128,
                                                    0.3f, 0.5f, ual, nullptr), JMT_ERR_ARG,
              "8-B aligned");
    expect_rc("dropout rows 2^32", jmt_dropout(JMT_BF16, algn, 256, algn, 256, big, 256, 128,
                                               0.3f, 0.5f, ual, nullptr), JMT_ERR_ARG,
              "32 bits of row");
    expect_rc("dropout dtype", jmt_dropout(7, algn, 256, algn, 256, 8, 256, 128, 0.3f, 0.5f, ual,
                                           nullptr), JMT_ERR_ARG, "dtype");
    expect_rc("head_fwd_drop null ctr",
              jmt_head_fwd_drop(JMT_BF16, JMT_F32, 8, 128, 1, algn, 256, algn, algn, nullptr,
                                nullptr, algn, algn, 1, 0.3f, 0.5f, nullptr, nullptr),
              JMT_ERR_ARG, "null counter");
    expect_rc("head_fwd_drop p = 1",
              jmt_head_fwd_drop(JMT_BF16, JMT_F32, 8, 128, 1, algn, 256, algn, algn, nullptr,
                                nullptr, algn, algn, 1, 1.0f, 0.5f, ual, nullptr),
              JMT_ERR_ARG, "[0, 1)");
    expect_rc("head_fwd_drop rows 2^32",
              jmt_head_fwd_drop(JMT_BF16, JMT_F32, big, 128, 1, algn, 256, algn, algn, nullptr,
                                nullptr, algn, algn, 1, 0.3f, 0.5f, ual, nullptr),
              JMT_ERR_ARG, "32 bits of row");
    expect_rc("head_fwd_drop misaligned",
              jmt_head_fwd_drop(JMT_BF16, JMT_F32, 8, 128, 1, misal, 256, algn, algn, nullptr,
                                nullptr, algn, algn, 1, 0.3f, 0.5f, ual, nullptr),
              JMT_ERR_ARG, "8-B aligned");
    expect_rc("head_bwd_drop null ctr",
              jmt_head_bwd_drop(JMT_BF16, JMT_F32, 8, 128, 1, algn, 256, algn, algn, algn, algn,
                                1, algn, 256, nullptr, nullptr, nullptr, nullptr, (float*)algn,
                                0.3f, 0.5f, nullptr, nullptr),
              JMT_ERR_ARG, "null counter");
    expect_rc("head_bwd_drop p = 1",
              jmt_head_bwd_drop(JMT_BF16, JMT_F32, 8, 128, 1, algn, 256, algn, algn, algn, algn,
                                1, algn, 256, nullptr, nullptr, nullptr, nullptr, (float*)algn,
                                0.3f, 1.0f, ual, nullptr),
              JMT_ERR_ARG, "[0, 1)");
    expect_rc("head_bwd_drop rows 2^32",
              jmt_head_bwd_drop(JMT_BF16, JMT_F32, big, 128, 1, algn, 256, algn, algn, algn,
                                algn, 1, algn, 256, nullptr, nullptr, nullptr, nullptr,
                                (float*)algn, 0.3f, 0.5f, ual, nullptr),
              JMT_ERR_ARG, "32 bits of row");
    expect_rc("head_bwd_drop misaligned dh",
              jmt_head_bwd_drop(JMT_BF16, JMT_F32, 8, 128, 1, algn, 256, algn, algn, algn, algn,
                                1, misal, 256, nullptr, nullptr, nullptr, nullptr, (float*)algn,
                                0.3f, 0.5f, ual, nullptr),
              JMT_ERR_ARG, "bad gradient buffers");
    const uint32_t hctr[4] = {1u, 2u, 3u, 4u};
    float m8[8];
    expect_rc("dropout_reference null", jmt_dropout_reference(nullptr, 1, 4, 4, 0.f, 0.f, m8),
              JMT_ERR_ARG, "null pointer");
    expect_rc("dropout_reference p = 1", jmt_dropout_reference(hctr, 1, 4, 4, 1.0f, 0.f, m8),
              JMT_ERR_ARG, "[0, 1)");
    expect_rc("dropout_reference cols 6", jmt_dropout_reference(hctr, 1, 6, 4, 0.1f, 0.f, m8),
              JMT_ERR_ARG, "multiples of 4");
    expect_rc("dropout_reference rows 2^32", jmt_dropout_reference(hctr, big, 4, 4, 0.1f, 0.f,
                                                                   m8), JMT_ERR_ARG,
              "32 bits of row");
    // valid call: every element is 0 or s, p = 0 keeps everything (ASan sees the writes)
    expect_eq("dropout_reference ok", jmt_dropout_reference(hctr, 2, 4, 4, 0.f, 0.5f, m8), JMT_OK);
    for (int i = 0; i < 8; ++i)
      if (m8[i] != 1.f) {
        fprintf(stderr, "FAIL dropout_reference p = 0: m[%d] = %g\n", i, m8[i]);
        ++g_fail;
      }
    expect_eq("dropout_reference ok", jmt_dropout_reference(hctr, 1, 8, 4, 0.5f, 0.75f, m8),
              JMT_OK);
    for (int i = 0; i < 8; ++i) {
      const float s = i < 4 ? 2.f : 4.f;
      if (m8[i] != 0.f && m8[i] != s) {
        fprintf(stderr, "FAIL dropout_reference: m[%d] = %g\n", i, m8[i]);
        ++g_fail;
      }
    }
  }

  if (jmt_bounds_violations(0) != -1) {
    fprintf(stderr, "FAIL bounds counters present in the default build\n");
    ++g_fail;
  }
  printf("abi_check: %s (%d failures)\n", g_fail ? "FAIL" : "ok", g_fail);
  return g_fail ? 1 : 0;
}
