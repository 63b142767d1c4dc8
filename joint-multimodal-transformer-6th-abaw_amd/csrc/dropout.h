// The regressor dropout mask: one specification for every kernel that applies it
// (dropout.hip, head.hip) and for the host reference (abi.cpp jmt_dropout_reference).  Plain C++,
// host and device.
//
//   generator  Philox4x32-10
//   key        (seed_lo, seed_hi)                       } the device state block
//   counter    (row, quad, call, stream)                } uint32[4] = seed_lo, seed_hi, call, stream
//              row = memory row of the masked buffer, quad = column / 4; output word i belongs
//              to column 4 quad + i
//   keep       word >= T, T = (uint32)((double)p * 2^32)   (p = 0: T = 0, everything is kept)
//   scale      kept elements are multiplied by s = 1.0f / (1.0f - p), dropped ones by 0
//   columns < split use p0, the others p1
// The mask is a function of (state block, row, column) alone: the backward regenerates it from the
// 16 bytes the forward kept, nothing is stored per element.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define JMT_HD __host__ __device__ inline
#else
#define JMT_HD inline
#endif

namespace jmt {

struct Philox4 {
  uint32_t w[4];
};

JMT_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                             uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r) {
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
  }
  Philox4 o;
  o.w[0] = c0; o.w[1] = c1; o.w[2] = c2; o.w[3] = c3;
  return o;
}

// keep threshold and scale of a rate 0 <= p < 1
JMT_HD uint32_t dropout_threshold(float p) { return (uint32_t)((double)p * 4294967296.0); }
JMT_HD float dropout_scale(float p) { return 1.0f / (1.0f - p); }

// the four words of (row, quad) under state block `ctr`
JMT_HD Philox4 dropout_words(const uint32_t* ctr, uint32_t row, uint32_t quad) {
  return philox4x32_10(row, quad, ctr[2], ctr[3], ctr[0], ctr[1]);
}

// the multipliers (0 or s) of one quad whose columns share threshold T and scale s
JMT_HD void dropout_quad(const uint32_t* ctr, uint32_t row, uint32_t quad, uint32_t T, float s,
                         float* m) {
  const Philox4 o = dropout_words(ctr, row, quad);
  for (int i = 0; i < 4; ++i) m[i] = o.w[i] >= T ? s : 0.f;
}

// The attention dropout mask: one specification for the fused multi-head kernels
// (attn_mh.hip), the GEMM + softmax path (dropout.hip jmt_attn_dropout) and the host reference
// (abi.cpp jmt_attn_dropout_reference).  8 bits per element; the unit is a block of 4 queries x
// 4 keys = the 16 bytes of one Philox4x32-10 call.
//
//   element    (nh, l, k): nh = n H + h, query l, key k (absolute indices)
//   key        (seed_lo, seed_hi)                       } the regressors' state block, a `call`
//   counter    (nh QB + (l >> 2), k >> 2, call, stream) } of its own per attention forward
//              QB = ceil(Lq / 4); N H QB <= 2^32
//   byte       byte k & 3 (bits 8 (k & 3) upward) of output word l & 3
//   keep       byte >= T8, T8 = floor(256 p + 1/2) <= 255: the rate is quantised to
//              p_eff = T8 / 256; T8 = 0: no mask
//   scale      kept probabilities are multiplied by s = 1.0f / (1.0f - p_eff), dropped ones by 0
JMT_HD uint32_t attn_dropout_threshold(float p) { return (uint32_t)(256.0 * (double)p + 0.5); }
JMT_HD float attn_dropout_rate(uint32_t T8) { return (float)T8 / 256.0f; }
JMT_HD float attn_dropout_scale(uint32_t T8) { return 1.0f / (1.0f - attn_dropout_rate(T8)); }
JMT_HD uint32_t attn_dropout_qblocks(int64_t Lq) { return (uint32_t)((Lq + 3) / 4); }

// the 16 bytes of block (qblk, kblk), qblk = nh QB + (l >> 2), kblk = k >> 2
JMT_HD Philox4 attn_dropout_block(const uint32_t* ctr, uint32_t qblk, uint32_t kblk) {
  return philox4x32_10(qblk, kblk, ctr[2], ctr[3], ctr[0], ctr[1]);
}
// the byte of query l, key k in its block's words
JMT_HD uint32_t attn_dropout_byte(const Philox4& o, uint32_t l, uint32_t k) {
  return (o.w[l & 3u] >> (8u * (k & 3u))) & 255u;
}
// the multiplier (0 or s) of element (nh, l, k)
JMT_HD float attn_dropout_mult(const uint32_t* ctr, uint32_t QB, uint32_t nh, uint32_t l,
                               uint32_t k, uint32_t T8, float s) {
  const Philox4 o = attn_dropout_block(ctr, nh * QB + (l >> 2), k >> 2);
  return attn_dropout_byte(o, l, k) >= T8 ? s : 0.f;
}

}  // namespace jmt
