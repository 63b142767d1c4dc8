// Host-side check of the grouped 16-bit-C GEMM entry points (jmt_gemm_group16,
// jmt_gemm_group16_ok, jmt_gemm_persist_cfg), built with AddressSanitizer and
// UndefinedBehaviorSanitizer by `make asan16` and run on the CPU by tests/test_abi_group16.py.
// Every refusal of include/jmt.h is driven with descriptors whose pointers are aligned but
// never dereferenced: the checks fail before a launch, so no kernel runs and no GPU is needed.
// Each call must return the documented JMT_ERR_* code and leave a bounded, non-empty
// jmt_last_error() that names the entry point.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/jmt.h"

static int g_fail = 0;

static void expect_rc(const char* what, int rc, int code) {
  const char* e = jmt_last_error();
  const size_t n = e ? strnlen(e, 1024) : 0;
  if (rc != code || (code != JMT_OK && (n == 0 || n >= 512 || !strstr(e, "jmt_gemm_group16")))) {
    fprintf(stderr, "FAIL %s: rc=%d (want %d) err='%s'\n", what, rc, code, e ? e : "(null)");
    ++g_fail;
  }
}

static const uintptr_t kBase = 0x10000000;     // aligned, never dereferenced

// problem i of a valid group: NT, bf16, M x N x K, `nb` batch entries through pointer tables,
// C regions 16 MiB apart
static jmt_gemm_desc prob(int i, int M, int N, int K, int nb) {
  jmt_gemm_desc d;
  memset(&d, 0, sizeof(d));
  d.ab_dtype = d.c_dtype = d.aux_dtype = JMT_BF16;
  d.M = M; d.N = N; d.K = K;
  d.a_kmajor = d.b_kmajor = 1;
  d.lda = K; d.ldb = K; d.ldc = N;
  d.batch0 = nb; d.batch1 = 1;
  d.alpha = 1.f;
  d.a_mode = d.b_mode = d.c_mode = nb > 1 ? 1 : 0;
  d.n_a = d.n_b = d.n_c = nb;
  for (int k = 0; k < nb; ++k) {
    d.a[k] = (const void*)(kBase + 0x100);
    d.b[k] = (const void*)(kBase + 0x200);
    d.c[k] = (void*)(kBase + ((uintptr_t)(i * 8 + k + 1) << 24));
  }
  return d;
}

template <class F>
static void refused(const char* what, int code, F mutate) {
  jmt_gemm_desc g[3] = {prob(0, 512, 256, 512, 2), prob(1, 256, 512, 320, 1),
                        prob(2, 256, 256, 256, 3)};
  mutate(g);
  expect_rc(what, jmt_gemm_group16_ok(g, 3), code);
  // the launching entry point runs the same checks first: nothing reaches a kernel
  expect_rc(what, jmt_gemm_group16(g, 3, nullptr), code);
}

int main() {
  if (jmt_abi_version() != JMT_ABI_VERSION) {
    fprintf(stderr, "FAIL abi version\n");
    return 1;
  }
  const int U = JMT_ERR_UNSUPPORTED, A = JMT_ERR_ARG;
  static float biasv[4];
  {
    jmt_gemm_desc g[3] = {prob(0, 512, 256, 512, 2), prob(1, 256, 512, 320, 1),
                          prob(2, 256, 256, 256, 3)};
    expect_rc("valid group", jmt_gemm_group16_ok(g, 3), JMT_OK);
    expect_rc("valid single", jmt_gemm_group16_ok(g, 1), JMT_OK);
    expect_rc("null descs", jmt_gemm_group16_ok(nullptr, 2), A);
    expect_rc("0 problems", jmt_gemm_group16_ok(g, 0), A);
    jmt_gemm_desc nine[9];
    for (int i = 0; i < 9; ++i) nine[i] = prob(i, 256, 256, 256, 1);
    expect_rc("8 problems", jmt_gemm_group16_ok(nine, 8), JMT_OK);
    expect_rc("9 problems", jmt_gemm_group16_ok(nine, 9), A);
    expect_rc("9 problems launch", jmt_gemm_group16(nine, 9, nullptr), A);
  }
  // JMT_ERR_UNSUPPORTED: the caller runs jmt_gemm on each problem
  refused("fp32 operands", U, [](jmt_gemm_desc* g) { g[1].ab_dtype = g[1].c_dtype = JMT_F32; });
  refused("fp32 C", U, [](jmt_gemm_desc* g) { g[0].c_dtype = JMT_F32; });
  refused("mixed dtype", U, [](jmt_gemm_desc* g) { g[2].ab_dtype = g[2].c_dtype = JMT_F16; });
  refused("mixed A layout", U, [](jmt_gemm_desc* g) { g[1].a_kmajor = 0; });
  refused("mixed B layout", U, [](jmt_gemm_desc* g) { g[2].b_kmajor = 0; });
  refused("row sums", U, [](jmt_gemm_desc* g) {
    g[0].n_dbias = 2;
    g[0].dbias_tab[0] = g[0].dbias_tab[1] = biasv;
  });
  refused("split-K", U, [](jmt_gemm_desc* g) { g[0].splits = 2; });
  refused("partial row panel", U, [](jmt_gemm_desc* g) { g[0].M = 384; });
  refused("N not a tile", U, [](jmt_gemm_desc* g) { g[1].N = 384; });
  refused("K not a K-tile", U, [](jmt_gemm_desc* g) { g[1].K = 300; });
  refused("K too short", U, [](jmt_gemm_desc* g) { g[2].K = 192; });
  refused("batch1", U, [](jmt_gemm_desc* g) { g[2].batch1 = 2; });
  refused("bias per row", U, [](jmt_gemm_desc* g) { g[1].bias = biasv; g[1].bias_mode = 2; });
  refused("mixed EPI: relu", U, [](jmt_gemm_desc* g) { g[1].relu = 1; });
  refused("mixed EPI: beta", U, [](jmt_gemm_desc* g) { g[0].beta = 1.f; });
  refused("mixed EPI: aux", U, [](jmt_gemm_desc* g) { g[2].aux = (const void*)kBase; });
  refused("bias floats", U, [](jmt_gemm_desc* g) {
    g[0].N = 4352;                        // 2 entries x 4352 floats > 8192
    g[0].ldc = 4352;
    g[0].bias_mode = 1;
    g[0].n_bias = 2;
    g[0].bias_tab[0] = g[0].bias_tab[1] = biasv;
  });
  {
    // 8 problems x (8 + 8 + 8 + 1) pointers = 200 > the pool's 192
    jmt_gemm_desc g[8];
    for (int i = 0; i < 8; ++i) {
      g[i] = prob(i, 256, 256, 256, 8);
      g[i].bias_mode = 1;
      g[i].bias = biasv;
    }
    expect_rc("pointer pool", jmt_gemm_group16_ok(g, 8), U);
    expect_rc("pointer pool launch", jmt_gemm_group16(g, 8, nullptr), U);
    expect_rc("pointer pool: 7 fit", jmt_gemm_group16_ok(g, 7), JMT_OK);
  }
  // JMT_ERR_ARG
  refused("bad dtype", A, [](jmt_gemm_desc* g) { g[0].ab_dtype = 7; });
  refused("null A", A, [](jmt_gemm_desc* g) { g[0].a[1] = nullptr; });
  refused("misaligned A", A, [](jmt_gemm_desc* g) { g[1].a[0] = (const void*)(kBase + 8); });
  refused("null B", A, [](jmt_gemm_desc* g) { g[1].b[0] = nullptr; });
  refused("misaligned B", A, [](jmt_gemm_desc* g) { g[2].b[2] = (const void*)(kBase + 2); });
  refused("null C", A, [](jmt_gemm_desc* g) { g[2].c[1] = nullptr; });
  refused("misaligned C", A, [](jmt_gemm_desc* g) {
    g[0].c[0] = (void*)((uintptr_t)g[0].c[0] + 8);
  });
  refused("misaligned bias", A, [](jmt_gemm_desc* g) {
    g[1].bias = (const float*)((const char*)biasv + 2);
    g[1].bias_mode = 1;
  });
  refused("short A table", A, [](jmt_gemm_desc* g) { g[0].n_a = 1; });
  refused("short B table", A, [](jmt_gemm_desc* g) { g[2].n_b = 2; });
  refused("short C table", A, [](jmt_gemm_desc* g) { g[2].n_c = 2; });
  refused("short bias table", A, [](jmt_gemm_desc* g) {
    g[2].bias_mode = 1;
    g[2].n_bias = 2;
    g[2].bias_tab[0] = g[2].bias_tab[1] = biasv;
  });
  refused("table size", A, [](jmt_gemm_desc* g) { g[0].n_c = 9; });
  refused("short K-concat table", A, [](jmt_gemm_desc* g) {
    g[1].a_mode = 2;
    g[1].a_kseg = 64;                     // K = 320 needs 5 segments, the table holds 1
  });
  refused("K-concat segment", A, [](jmt_gemm_desc* g) { g[1].b_mode = 2; g[1].b_kseg = 100; });
  refused("short per-batch K-concat table", A, [](jmt_gemm_desc* g) {
    g[0].a_mode = 3;
    g[0].a_kseg = 256;                    // 2 entries x 2 segments, the table holds 2
  });
  refused("bad mode", A, [](jmt_gemm_desc* g) { g[0].c_mode = 2; });
  refused("lda", A, [](jmt_gemm_desc* g) { g[0].lda = 516; });
  refused("ldc < N", A, [](jmt_gemm_desc* g) { g[1].ldc = 256; });
  refused("ldc", A, [](jmt_gemm_desc* g) { g[1].ldc = 516; });
  refused("batch stride", A, [](jmt_gemm_desc* g) { g[1].sC0 = 4; });
  refused("empty", A, [](jmt_gemm_desc* g) { g[1].M = 0; });
  // overlapping C: the same region; a region that starts inside another's rows; interleaved
  // columns that reach into each other; interleaved columns at different pitches
  refused("C same region", A, [](jmt_gemm_desc* g) { g[1].c[0] = g[0].c[1]; });
  refused("C inside another", A, [](jmt_gemm_desc* g) {
    g[1].c[0] = (void*)((uintptr_t)g[2].c[2] + 256 * 2 * 16);
  });
  refused("C columns collide", A, [](jmt_gemm_desc* g) {
    g[1].ldc = g[2].ldc = 768;
    g[1].c[0] = (void*)((uintptr_t)g[2].c[0] + 128 * 2);   // columns [128, 640) over [0, 256)
  });
  refused("C pitches differ", A, [](jmt_gemm_desc* g) {
    g[1].ldc = 1024;
    g[2].ldc = 768;
    g[1].c[0] = (void*)((uintptr_t)g[2].c[0] + 256 * 2);
  });
  {
    // disjoint columns of the same rows at one pitch are no overlap (the packed QKV buffer)
    jmt_gemm_desc g[2] = {prob(0, 256, 256, 256, 1), prob(1, 256, 512, 256, 1)};
    g[0].ldc = g[1].ldc = 768;
    g[1].c[0] = (void*)((uintptr_t)g[0].c[0] + 256 * 2);
    expect_rc("C disjoint columns", jmt_gemm_group16_ok(g, 2), JMT_OK);
    // strided batch entries: entry 1 of problem 0 lands on problem 1
    g[0] = prob(0, 256, 256, 256, 1);
    g[1] = prob(1, 256, 256, 256, 1);
    g[0].batch0 = 2;
    g[0].sC0 = ((uintptr_t)g[1].c[0] - (uintptr_t)g[0].c[0]) / 2;
    expect_rc("C strided entry collides", jmt_gemm_group16_ok(g, 2), A);
  }
  // jmt_gemm_persist_cfg: a host function; a refused descriptor is 0, not an error
  {
    jmt_gemm_desc d = prob(0, 512, 256, 512, 2);
    const int c = jmt_gemm_persist_cfg(&d);
    if (c != 0 && c != 45 && c != 40 && c != 43) {
      fprintf(stderr, "FAIL persist_cfg: %d\n", c);
      ++g_fail;
    }
    d.splits = 4;                         // split-K (and no workspace): never persistent
    if (jmt_gemm_persist_cfg(&d) != 0 || jmt_gemm_persist_cfg(nullptr) != 0) {
      fprintf(stderr, "FAIL persist_cfg of a split / null descriptor\n");
      ++g_fail;
    }
  }
  jmt_gemm_group16_set_grid(0);
  if (g_fail) {
    fprintf(stderr, "abi_check_group16: %d failure(s)\n", g_fail);
    return 1;
  }
  printf("abi_check_group16: ok\n");
  return 0;
}
