// Counter-based dropout (dropout.h) outside the fused head kernels:
//   jmt_dropout_next  one thread: out = state, then state.call += 1 — the 16 bytes a forward keeps
//                     so that its backward regenerates the same mask, and a replayed graph draws
//                     a new `call` per replay without re-capture
//   jmt_dropout       y = m . x over a (rows x cols) block, in place or not: the regressors'
//                     hidden activations on the GEMM route (functional.MLPFn / MLPPairFn), once
//                     on h after the ReLU GEMM and once on dh after the masked dgrad
//   jmt_attn_dropout  the attention mask (8 bits per element, 4 x 4 blocks) on the GEMM + softmax
//                     path's probabilities and on its dP
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

// The attention mask (dropout.h) on a materialised (NH Lq, ld) buffer: the GEMM + softmax path's
// probabilities (out of place: P~ for the P V and dV GEMMs) and its fp32 dP (in place).  A lane
// owns 4 consecutive keys of one row = one word of the block's Philox call.
struct AttnDropArgs {
  const void* x;
  void* y;
  int64_t ldx, ldy, rows;    // rows = NH Lq
  int Lq, Lk, quads;         // quads per row: ceil(Lk / 4) in place, ldy / 4 out of place
  uint32_t T8, QB;
  float s;
  const uint32_t* ctr;
};

template <typename T>
__global__ __launch_bounds__(256) void attn_dropout_kernel(AttnDropArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = i / a.quads;
  if (row >= a.rows) return;
  const int q = (int)(i - row * a.quads);
  const bool inplace = a.x == a.y;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  JMT_DCHECK(4 * q + 3 < a.ldy);
  if (4 * q < a.Lk) {
    const uint32_t ctr[4] = {a.ctr[0], a.ctr[1], a.ctr[2], a.ctr[3]};
    const uint32_t nh = (uint32_t)(row / a.Lq), l = (uint32_t)(row - (int64_t)nh * a.Lq);
    const Philox4 o = attn_dropout_block(ctr, nh * a.QB + (l >> 2), (uint32_t)q);
    JMT_DCHECK(4 * q + 3 < a.ldx);
    Quad<T>::ld((const T*)a.x + row * a.ldx + 4 * q, v);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (4 * q + e < a.Lk) v[e] *= attn_dropout_byte(o, l, (uint32_t)e) >= a.T8 ? a.s : 0.f;
      else if (!inplace) v[e] = 0.f;               // padding columns: zeros out of place
    }
  }
  Quad<T>::st((T*)a.y + row * a.ldy + 4 * q, v);
}

}  // namespace jmt

using namespace jmt;

extern "C" int jmt_attn_dropout(int dt, const void* x, int64_t ldx, void* y, int64_t ldy,
                                int64_t NH, int64_t Lq, int64_t Lk, float p, const uint32_t* ctr,
                                void* stream) {
  JMT_CHECK_ARG(dt == JMT_F32 || dt == JMT_BF16 || dt == JMT_F16, "jmt_attn_dropout: dtype %d",
                dt);
  JMT_CHECK_ARG(x && y, "jmt_attn_dropout: null pointer");
  JMT_CHECK_ARG(ctr != nullptr && ((uintptr_t)ctr & 3) == 0,
                "jmt_attn_dropout: counter block null or not 4-B aligned");
  JMT_CHECK_ARG(NH >= 0 && Lq >= 0 && Lk >= 0 && Lq < ((int64_t)1 << 31) &&
                    Lk < ((int64_t)1 << 31) - 4,
                "jmt_attn_dropout: bad sizes (NH %lld Lq %lld Lk %lld)", (long long)NH,
                (long long)Lq, (long long)Lk);
  JMT_CHECK_ARG(p >= 0.f && p < 1.f, "jmt_attn_dropout: rate %g outside [0, 1)", (double)p);
  const uint32_t T8 = attn_dropout_threshold(p);
  JMT_CHECK_ARG(T8 <= 255u, "jmt_attn_dropout: rate %g rounds to T8 = %u > 255", (double)p, T8);
  const int64_t lkq = 4 * ((Lk + 3) / 4);
  const int es = dtype_size(dt);
  JMT_CHECK_ARG(ldx >= lkq && ldy >= lkq && ldx % 4 == 0 && ldy % 4 == 0 &&
                    ldy < ((int64_t)1 << 31),
                "jmt_attn_dropout: row strides must be multiples of 4 and hold ceil(Lk / 4) quads");
  JMT_CHECK_ARG(((uintptr_t)x & 7) == 0 && ((uintptr_t)y & 7) == 0 && (ldx * es) % 8 == 0 &&
                    (ldy * es) % 8 == 0,
                "jmt_attn_dropout: x / y rows not 8-B aligned");
  JMT_CHECK_ARG(x != y || ldx == ldy, "jmt_attn_dropout: in place with two row strides");
  const uint32_t QB = attn_dropout_qblocks(Lq);
  if (NH * (int64_t)QB > ((int64_t)1 << 32))
    return set_error(JMT_ERR_UNSUPPORTED, "jmt_attn_dropout: NH %lld Lq %lld: NH ceil(Lq / 4) "
                     "exceeds the dropout counter's 2^32 query blocks", (long long)NH,
                     (long long)Lq);
  if (NH == 0 || Lq == 0 || Lk == 0) return JMT_OK;
  AttnDropArgs a = {};
  a.x = x; a.y = y; a.ldx = ldx; a.ldy = ldy; a.rows = NH * Lq;
  a.Lq = (int)Lq; a.Lk = (int)Lk;
  a.quads = (int)(x == y ? lkq / 4 : ldy / 4);
  a.T8 = T8; a.QB = QB; a.s = attn_dropout_scale(T8);
  a.ctr = ctr;
  const int64_t nblk = (a.rows * a.quads + 255) / 256;
  JMT_CHECK_ARG(nblk < ((int64_t)1 << 31), "jmt_attn_dropout: %lld x %lld exceeds one launch",
                (long long)a.rows, (long long)Lk);
  const dim3 grid((unsigned)nblk);
  hipStream_t st = as_stream(stream);
  if (dt == JMT_F32) hipLaunchKernelGGL(attn_dropout_kernel<float>, grid, dim3(256), 0, st, a);
  else if (dt == JMT_BF16)
    hipLaunchKernelGGL(attn_dropout_kernel<__bf16>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(attn_dropout_kernel<_Float16>, grid, dim3(256), 0, st, a);
  JMT_LAUNCH_CHECK("jmt_attn_dropout");
  return JMT_OK;
}

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
