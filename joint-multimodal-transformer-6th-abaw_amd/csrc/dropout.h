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

}  // namespace jmt
