// Counter-based dropout (dropout.h) outside the fused head kernels:
//   jmt_dropout_next  one thread: out = state, then state.call += 1 — the 16 bytes a forward keeps
//                     so that its backward regenerates the same mask, and a replayed graph draws
//                     a new `call` per replay without re-capture
//   jmt_dropout       y = m . x over a (rows x cols) block, in place or not: the regressors'
//                     hidden activations on the GEMM route (functional.MLPFn / MLPPairFn), once
//                     on h after the ReLU GEMM and once on dh after the masked dgrad
// A lane owns one quad (4 consecutive columns = one Philox call): one 8-B access for the 16-bit
// types, two for fp32; the product is formed in fp32 and rounded once.
#include "common.h"
#include "dropout.h"

namespace jmt {

__global__ void dropout_next_kernel(uint32_t* st, uint32_t* out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const uint32_t c = st[2];
  out[0] = st[0];
  out[1] = st[1];
  out[2] = c;
  out[3] = st[3];
  st[2] = c + 1u;
}

template <typename T> struct Quad;   // 4 consecutive elements <-> 8-B accesses
template <> struct Quad<float> {
  static __device__ __forceinline__ void ld(const float* p, float* v) {
    const float2 a = *(const float2*)p, b = *(const float2*)(p + 2);
    v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
  }
  static __device__ __forceinline__ void st(float* p, const float* v) {
    *(float2*)p = make_float2(v[0], v[1]);
    *(float2*)(p + 2) = make_float2(v[2], v[3]);
  }
};
template <> struct Quad<__bf16> {
  static __device__ __forceinline__ void ld(const __bf16* p, float* v) {
    const uint2 u = *(const uint2*)p;
    const __bf16* e = (const __bf16*)&u;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (float)e[i];
  }
  static __device__ __forceinline__ void st(__bf16* p, const float* v) {
    __bf16 e[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) e[i] = (__bf16)v[i];
    *(uint2*)p = *(const uint2*)e;
  }
};
template <> struct Quad<_Float16> {
  static __device__ __forceinline__ void ld(const _Float16* p, float* v) {
    const uint2 u = *(const uint2*)p;
    const _Float16* e = (const _Float16*)&u;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (float)e[i];
  }
  static __device__ __forceinline__ void st(_Float16* p, const float* v) {
    _Float16 e[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) e[i] = (_Float16)v[i];
    *(uint2*)p = *(const uint2*)e;
  }
};

struct DropArgs {
  const void* x;
  void* y;
  int64_t ldx, ldy, rows;
  int quads, split_quad;     // cols / 4, split / 4
  uint32_t T[2];
  float s[2];
  const uint32_t* ctr;
};

template <typename T>
__global__ __launch_bounds__(256) void dropout_kernel(DropArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t r = i / a.quads;
  if (r >= a.rows) return;
  const int q = (int)(i - r * a.quads);
  const uint32_t ctr[4] = {a.ctr[0], a.ctr[1], a.ctr[2], a.ctr[3]};
  const int g = q < a.split_quad ? 0 : 1;
  float m[4], v[4];
  dropout_quad(ctr, (uint32_t)r, (uint32_t)q, a.T[g], a.s[g], m);
  JMT_DCHECK(4 * q + 3 < a.ldx && 4 * q + 3 < a.ldy);
  Quad<T>::ld((const T*)a.x + r * a.ldx + 4 * q, v);
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] *= m[e];
  Quad<T>::st((T*)a.y + r * a.ldy + 4 * q, v);
}

}  // namespace jmt

using namespace jmt;

extern "C" int jmt_dropout_next(uint32_t* state, uint32_t* out, void* stream) {
  JMT_CHECK_ARG(state, "jmt_dropout_next: null state");
  JMT_CHECK_ARG(out, "jmt_dropout_next: null out");
  JMT_CHECK_ARG(((uintptr_t)state & 3) == 0 && ((uintptr_t)out & 3) == 0,
                "jmt_dropout_next: state / out not 4-B aligned");
  hipLaunchKernelGGL(dropout_next_kernel, dim3(1), dim3(64), 0, as_stream(stream), state, out);
  JMT_LAUNCH_CHECK("jmt_dropout_next");
  return JMT_OK;
}

extern "C" int jmt_dropout(int dt, const void* x, int64_t ldx, void* y, int64_t ldy, int64_t rows,
                           int64_t cols, int64_t split, float p0, float p1, const uint32_t* ctr,
                           void* stream) {
  JMT_CHECK_ARG(dt == JMT_F32 || dt == JMT_BF16 || dt == JMT_F16, "jmt_dropout: dtype %d", dt);
  JMT_CHECK_ARG(x && y, "jmt_dropout: null pointer");
  JMT_CHECK_ARG(ctr, "jmt_dropout: null counter block");
  JMT_CHECK_ARG(rows >= 0 && rows < ((int64_t)1 << 32),
                "jmt_dropout: rows = %lld (the counter holds 32 bits of row)", (long long)rows);
  JMT_CHECK_ARG(cols >= 0 && cols < ((int64_t)1 << 31) && cols % 4 == 0,
                "jmt_dropout: cols = %lld must be a multiple of 4", (long long)cols);
  JMT_CHECK_ARG(split >= 0 && split <= cols && split % 4 == 0,
                "jmt_dropout: split = %lld must be a multiple of 4 in [0, cols]", (long long)split);
  JMT_CHECK_ARG(p0 >= 0.f && p0 < 1.f && p1 >= 0.f && p1 < 1.f,
                "jmt_dropout: rates must be in [0, 1)");
  const int es = dtype_size(dt);
  JMT_CHECK_ARG(ldx >= cols && ldy >= cols, "jmt_dropout: row stride below cols");
  JMT_CHECK_ARG(((uintptr_t)x & 7) == 0 && ((uintptr_t)y & 7) == 0 && (ldx * es) % 8 == 0 &&
                    (ldy * es) % 8 == 0 && ((uintptr_t)ctr & 3) == 0,
                "jmt_dropout: x / y rows not 8-B aligned");
  if (rows == 0 || cols == 0) return JMT_OK;
  const int64_t nblk = (rows * (cols / 4) + 255) / 256;
  JMT_CHECK_ARG(nblk < ((int64_t)1 << 31), "jmt_dropout: %lld x %lld exceeds one launch",
                (long long)rows, (long long)cols);
  DropArgs a = {};
  a.x = x; a.y = y; a.ldx = ldx; a.ldy = ldy; a.rows = rows;
  a.quads = (int)(cols / 4); a.split_quad = (int)(split / 4);
  a.T[0] = dropout_threshold(p0); a.T[1] = dropout_threshold(p1);
  a.s[0] = dropout_scale(p0); a.s[1] = dropout_scale(p1);
  a.ctr = ctr;
  const dim3 grid((unsigned)nblk);
  hipStream_t st = as_stream(stream);
  if (dt == JMT_F32) hipLaunchKernelGGL(dropout_kernel<float>, grid, dim3(256), 0, st, a);
  else if (dt == JMT_BF16) hipLaunchKernelGGL(dropout_kernel<__bf16>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(dropout_kernel<_Float16>, grid, dim3(256), 0, st, a);
  JMT_LAUNCH_CHECK("jmt_dropout");
  return JMT_OK;
}
