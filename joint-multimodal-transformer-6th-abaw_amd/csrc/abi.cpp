// Error plumbing and version probes of the C-ABI (include/jmt.h).
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

#include "../../include/jmt.h"
#include "dropout.h"

namespace jmt {

static thread_local char g_err[512] = "";

int set_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

// per-translation-unit device counters of the bounds-check build (common.h JMT_DCHECK)
static unsigned (*g_bounds[16])(bool) = {};
static int g_nbounds = 0;

int register_bounds_counter(unsigned (*read)(bool reset)) {
  if (g_nbounds < 16) g_bounds[g_nbounds++] = read;
  return g_nbounds;
}

}  // namespace jmt

extern "C" int jmt_abi_version(void) { return JMT_ABI_VERSION; }

// Bounds-check build (`make bounds`, -DJMT_BOUNDS=1): failed device index checks since the last
// reset (synchronises the device); -1 in the default build, which has no checks.
extern "C" long long jmt_bounds_violations(int reset) {
  if (jmt::g_nbounds == 0) return -1;
  if (hipDeviceSynchronize() != hipSuccess) return -2;
  long long n = 0;
  for (int i = 0; i < jmt::g_nbounds; ++i) n += jmt::g_bounds[i](reset != 0);
  return n;
}
extern "C" const char* jmt_last_error(void) { return jmt::g_err; }

// Host reference of the dropout mask: the multiplier (0 or s) of every element of a
// (rows x cols) block, from the header the kernels compile (dropout.h).
extern "C" int jmt_dropout_reference(const uint32_t ctr[4], int64_t rows, int64_t cols,
                                     int64_t split, float p0, float p1, float* out) {
  using namespace jmt;
  if (!ctr || !out) return set_error(JMT_ERR_ARG, "jmt_dropout_reference: null pointer");
  if (rows < 0 || rows >= ((int64_t)1 << 32))
    return set_error(JMT_ERR_ARG, "jmt_dropout_reference: rows = %lld (the counter holds 32 "
                     "bits of row)", (long long)rows);
  if (cols < 0 || cols % 4 || split < 0 || split > cols || split % 4)
    return set_error(JMT_ERR_ARG, "jmt_dropout_reference: cols = %lld / split = %lld must be "
                     "multiples of 4, split in [0, cols]", (long long)cols, (long long)split);
  if (!(p0 >= 0.f && p0 < 1.f && p1 >= 0.f && p1 < 1.f))
    return set_error(JMT_ERR_ARG, "jmt_dropout_reference: rates must be in [0, 1)");
  const uint32_t T[2] = {dropout_threshold(p0), dropout_threshold(p1)};
  const float s[2] = {dropout_scale(p0), dropout_scale(p1)};
  for (int64_t r = 0; r < rows; ++r)
    for (int64_t q = 0; q < cols / 4; ++q) {
      const int g = 4 * q < split ? 0 : 1;
      dropout_quad(ctr, (uint32_t)r, (uint32_t)q, T[g], s[g], out + r * cols + 4 * q);
    }
  return JMT_OK;
}
extern "C" float jmt_attn_dropout_rate(float p) {
  using namespace jmt;
  if (!(p >= 0.f && p < 1.f)) return -1.f;
  const uint32_t T8 = attn_dropout_threshold(p);
  return T8 <= 255u ? attn_dropout_rate(T8) : -1.f;
}
extern "C" int jmt_attn_dropout_reference(const uint32_t ctr[4], int64_t NH, int64_t Lq,
                                          int64_t Lk, float p, float* out) {
  using namespace jmt;
  if (!ctr || !out) return set_error(JMT_ERR_ARG, "jmt_attn_dropout_reference: null pointer");
  if (NH < 0 || Lq < 0 || Lk < 0 || Lq >= ((int64_t)1 << 31) || Lk >= ((int64_t)1 << 31))
    return set_error(JMT_ERR_ARG, "jmt_attn_dropout_reference: bad sizes (NH %lld Lq %lld Lk "
                     "%lld)", (long long)NH, (long long)Lq, (long long)Lk);
  if (!(p >= 0.f && p < 1.f))
    return set_error(JMT_ERR_ARG, "jmt_attn_dropout_reference: rate must be in [0, 1)");
  const uint32_t T8 = attn_dropout_threshold(p);
  if (T8 > 255u)
    return set_error(JMT_ERR_ARG, "jmt_attn_dropout_reference: rate %g rounds to T8 = %u > 255",
                     (double)p, T8);
  const uint32_t QB = attn_dropout_qblocks(Lq);
  if (NH * (int64_t)QB > ((int64_t)1 << 32))
    return set_error(JMT_ERR_UNSUPPORTED, "jmt_attn_dropout_reference: NH ceil(Lq / 4) exceeds "
                     "the counter's 2^32 query blocks");
  const float s = attn_dropout_scale(T8);
  for (int64_t nh = 0; nh < NH; ++nh)
    for (int64_t l = 0; l < Lq; ++l)
      for (int64_t k = 0; k < Lk; ++k)
        out[(nh * Lq + l) * Lk + k] =
            attn_dropout_mult(ctr, QB, (uint32_t)nh, (uint32_t)l, (uint32_t)k, T8, s);
  return JMT_OK;
}
// GEMM (3 dtypes x 4 layouts + split-K reduce) + row ops + CCC + SGD; informational only.
extern "C" int jmt_kernel_count(void) { return 12 + 1 + 8 + 4 + 2 + 4; }
