// Fused multi-head attention for head dims 64 and 128 (num_heads 8 and 4 at model width 512),
// gfx950 wave64: a flash-attention forward and a two-kernel backward, with key ranges.
//
// At dh = 64 / 128 the whole tile problem fits on chip (attn.hip, dh = 512, had to split it): a
// wave keeps its 16 query rows (forward, dQ) or its 16 keys (dK / dV) as MFMA fragments in
// registers, and the other side streams through LDS in 64-row tiles that the block's 4 waves
// share.  Every product is v_mfma_f32_16x16x32 with the STREAMED side as the A operand, so the
// accumulator of the first product (scores, dP) has the wave's own row on the lane index and is,
// after rounding, directly the B operand of the second product (P V, dS K, P^T dO, dS^T Q), whose A
// operand is the transposed read (ds_read_b64_tr_b16) of the same LDS image:
//
//  * attn_mh_fwd_kernel, item (n, h, 64 queries): S^T = K Q^T per 64-key tile, online softmax in
//    fp32 with exp2 and scale * log2(e) folded, O^T += V^T P.  A lane holds ONE query (column
//    li = lane & 15), its 16 keys of the tile and 4 dims of every 16-dim output tile, so the
//    running max, the rescale and the sum are per row by construction: no vote across rows, a
//    padded query row cannot change a valid row's bits.  Writes O (16-bit) and lse.
//  * attn_mh_dq_kernel, item (n, h, 64 queries): delta = rowsum(dO o O) from the 16-bit O, then per
//    key tile S^T and dP^T = V dO^T, P = exp2(S scale log2e - lse log2e), dS = scale P o (dP -
//    delta), dQ^T += K^T dS.  Writes dQ and delta (fp32, laid out like lse).
//  * attn_mh_dkdv_kernel, item (n, h, 64 keys), stream-ordered after it: the key on the lane;
//    sweeps the 64-query tiles (Q and dO images, lse and delta in LDS), S = Q K^T, dP = dO V^T,
//    dV^T += dO^T P, dK^T += Q^T dS in registers.  No atomics: every output element has one
//    writer and one summation order, so the backward is bitwise reproducible.
//
// Key ranges (KR = true): keys outside [kbeg, kend) get probability 0 by selection (never by
// exponentiating -inf), are staged as zeros (their K / V rows are not read), and key tiles wholly
// outside the range are skipped by the forward and the dQ kernel; the dK / dV kernel writes
// exact zeros for them without a sweep.  The KR = false instantiations take AttnMhArgs alone.
//
// Attention dropout (DROP = true): the 8-bit counter-based mask of dropout.h, regenerated in
// registers by all three kernels (one Philox call per lane and tile, shared by DPP within quads of
// lanes; mh_drop_tile).  The DROP = false instantiations are the code of before.
#include "attn_common.h"
#include "dropout.h"

namespace jmt {

constexpr int MH_ROWS = 64;                        // rows of a block's item and of an LDS tile
constexpr int MH_MAXL = 1 << 20;                   // jmt_attn_mh_ok: Lq, Lk limit

struct AttnMhArgs {
  const void* q;
  const void* k;
  const void* v;
  const void* o;      // backward: the forward's output (delta)
  const void* go;     // backward: dO
  void* out;          // forward: o
  float* lse;         // forward: written (may be null); backward: read
  float* delta;       // dQ kernel: written; dK / dV kernel: read
  void* dq;
  void* dk;
  void* dv;
  int64_t sq_l, sq_n, sk_l, sk_n, sv_l, sv_n, so_l, so_n, sgo_l, sgo_n;
  int64_t sdq_l, sdq_n, sdk_l, sdk_n, sdv_l, sdv_n;
  int Lq, Lk, H, ntile;                            // ntile: 64-row tiles of the item axis
  float scale, scale_log2;
};

typedef unsigned mh_u32x4 __attribute__((ext_vector_type(4)));

// Attention dropout (DROP = true; the mask of dropout.h): the state copy of the call, the keep
// threshold, QB = ceil(Lq / 4) and the scale of the kept probabilities.  Like the range table it
// travels behind the kernel's arguments, so the DROP = false instantiations are the parent's.
struct MhDrop {
  const uint32_t* ctr;
  uint32_t T8, QB;
  float s;
};
template <typename A>
struct WithDrop : A {
  MhDrop dr;
};
template <bool KR, bool DROP>
using MhArgs = std::conditional_t<DROP, WithDrop<KrArgs<AttnMhArgs, KR>>, KrArgs<AttnMhArgs, KR>>;

// lane C of every quad of 4 adjacent lanes to the whole quad (DPP quad_perm, EXEC all ones)
template <int C>
__device__ __forceinline__ uint32_t mh_quad_bcast(uint32_t x) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, C * 0x55, 0xf, 0xf, false);
}
// The mask bytes of a lane's 16 elements of one 64 x 64 tile: byte r of m[c] is the byte of
// element (c, r).  The four lanes li = 4 a .. 4 a + 3 of equal g meet the same four 4 x 4 blocks
// c = 0 .. 3: lane li & 3 = j makes the one Philox call of block c = j (the caller passes that
// block's counter words), and the quad hands the words round.  QL (forward, dQ): the query on the
// lane, keys 16 c + 4 g + r: the lane takes word l & 3 = li & 3 of every block, whose byte r is
// key r's.  !QL (dK / dV): the key on the lane, queries 16 c + 4 g + r: the lane takes byte
// k & 3 = li & 3 of word r.
template <bool QL, int C>
__device__ __forceinline__ uint32_t mh_drop_block(const Philox4& o, int j) {
  const uint32_t w0 = mh_quad_bcast<C>(o.w[0]), w1 = mh_quad_bcast<C>(o.w[1]);
  const uint32_t w2 = mh_quad_bcast<C>(o.w[2]), w3 = mh_quad_bcast<C>(o.w[3]);
  if constexpr (QL) {
    return j == 0 ? w0 : j == 1 ? w1 : j == 2 ? w2 : w3;
  } else {
    const int sh = 8 * j;
    return ((w0 >> sh) & 255u) | (((w1 >> sh) & 255u) << 8) | (((w2 >> sh) & 255u) << 16) |
           ((w3 >> sh) << 24);
  }
}
template <bool QL>
__device__ __forceinline__ void mh_drop_tile(const uint32_t (&ctr)[4], uint32_t qblk,
                                             uint32_t kblk, int li, uint32_t (&m)[4]) {
  uint32_t c[4] = {ctr[0], ctr[1], ctr[2], ctr[3]};
#if defined(__HIP_DEVICE_COMPILE__) && defined(__OPTIMIZE__)
  // The key is wave-uniform, so hipcc would keep all ten round keys of it in SGPRs across the
  // tile loop (the dK / dV kernel then runs out of them).  Opaque here: they are re-derived per
  // tile by a few scalar adds beside the vector work.
  asm volatile("" : "+s"(c[0]), "+s"(c[1]));
#endif
  const Philox4 o = attn_dropout_block(c, qblk, kblk);
  const int j = li & 3;
  m[0] = mh_drop_block<QL, 0>(o, j);
  m[1] = mh_drop_block<QL, 1>(o, j);
  m[2] = mh_drop_block<QL, 2>(o, j);
  m[3] = mh_drop_block<QL, 3>(o, j);
}
// All ones where element (c, r) of m = dm[c] is kept (byte >= T8, T8 >= 1), else 0; mh_masked
// applies it to a value.  Plain vector arithmetic, opaque to the compiler: as compares, a tile's
// sixteen keep bits take a pair of SGPRs each, more than the dK / dV kernel has to give.
__device__ __forceinline__ uint32_t mh_keep(uint32_t m, int r, uint32_t T8) {
  uint32_t k = (uint32_t)((int32_t)(T8 - 1u - ((m >> (8 * r)) & 255u)) >> 31);
#if defined(__HIP_DEVICE_COMPILE__) && defined(__OPTIMIZE__)
  asm("" : "+v"(k));
#endif
  return k;
}
__device__ __forceinline__ float mh_masked(float x, uint32_t keep) {
  return __uint_as_float(__float_as_uint(x) & keep);
}

// Byte offset of 16-B chunk ch of row `row` in a [64][DH] 16-bit image.  The XOR serves the row
// reads (ds_read_b128: 16 rows, one chunk) and the transposed reads (a 32-lane half: 8 rows, one
// chunk pair) alike; 256-B rows take the dual-use image of the programming guide (T10 (b)).
template <int DH>
__device__ __forceinline__ int mh_off(int row, int ch) {
  if constexpr (DH == 128) return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
  else return 128 * row + 16 * (ch ^ ((((row >> 1) & 3) << 1) | ((row >> 3) & 1)));
}

// One 64-row tile, rows r0 .. r0 + 63 of a strided view, through registers: mh_load issues the
// global loads (rows outside [lo, hi) are zeros and are not read), mh_store writes the image.
template <typename T, int DH>
__device__ __forceinline__ void mh_load(mh_u32x4 (&r)[DH / 32], const T* base, int64_t ld, int r0,
                                        int lo, int hi, int L) {
  constexpr int CPR = DH / 8;
#pragma unroll
  for (int i = 0; i < DH / 32; ++i) {
    const int idx = i * 256 + (int)threadIdx.x;
    const int row = idx / CPR, ch = idx % CPR, src = r0 + row;
    r[i] = mh_u32x4{0u, 0u, 0u, 0u};
    if (src >= lo && src < hi) {
      JMT_DCHECK(src >= 0 && src < L);
      r[i] = *(const mh_u32x4*)(base + (int64_t)src * ld + 8 * ch);
    }
  }
}
template <int DH>
__device__ __forceinline__ void mh_store(char* img, const mh_u32x4 (&r)[DH / 32]) {
  constexpr int CPR = DH / 8;
#pragma unroll
  for (int i = 0; i < DH / 32; ++i) {
    const int idx = i * 256 + (int)threadIdx.x;
    *(mh_u32x4*)(img + mh_off<DH>(idx / CPR, idx % CPR)) = r[i];
  }
}

// A-operand fragment of image rows: row `row`, elements 32 ks + 8 g .. + 7
template <typename T, int DH>
__device__ __forceinline__ typename Frag16<T>::t mh_row(const char* img, int row, int ks, int g) {
  return *(const typename Frag16<T>::t*)(img + mh_off<DH>(row, 4 * ks + g));
}
// A-operand fragment of the TRANSPOSED image: row = column 16 t + li of the image, k slot
// 8 g + j = image row r32 + 16 (j >> 2) + 4 g + (j & 3): the order in which a lane's two
// accumulator tiles of 16 rows hold their rows (4 g + r), so the rounded accumulators are the
// matching B operand.  Every lane supplies its address (EXEC all ones at every call).
template <typename T, int DH>
__device__ __forceinline__ typename Frag16<T>::t mh_tr(const char* img, int r32, int t, int li,
                                                       int g) {
  typedef typename Frag16<T>::h Hf;
  const int row = r32 + 4 * g + (li >> 2), ch = 2 * t + ((li & 3) >> 1), sub = 8 * (li & 1);
  const Hf lo = tr_read<Hf>(img + mh_off<DH>(row, ch) + sub);
  const Hf hi = tr_read<Hf>(img + mh_off<DH>(row + 16, ch) + sub);
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// store the lane's 4 consecutive dims 16 t + 4 g .. + 3 of every output tile of one row
template <typename T, int DH>
__device__ __forceinline__ void mh_store_row(const f32x4 (&acc)[DH / 16], float mul, T* row, int g,
                                             bool valid) {
  typedef typename Frag16<T>::h Hf;
  if (!valid) return;
#pragma unroll
  for (int t = 0; t < DH / 16; ++t) {
    // mul == 0 (an empty range, a key outside it): exact zeros whatever the accumulator holds
    const Hf v = {from_f<T>(mul != 0.f ? acc[t][0] * mul : 0.f),
                  from_f<T>(mul != 0.f ? acc[t][1] * mul : 0.f),
                  from_f<T>(mul != 0.f ? acc[t][2] * mul : 0.f),
                  from_f<T>(mul != 0.f ? acc[t][3] * mul : 0.f)};
    *(Hf*)(row + 16 * t + 4 * g) = v;
  }
}

template <typename T, int DH, bool KR, bool DROP>
__global__ __launch_bounds__(256, 2) void attn_mh_fwd_kernel(MhArgs<KR, DROP> p) {
  typedef typename Frag16<T>::t F;
  constexpr int NKS = DH / 32, NT = DH / 16, IMG = MH_ROWS * DH * 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* kimg = smem;
  char* vimg = smem + IMG;

  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int g = lane >> 4, li = lane & 15;
  const int item = blockIdx.x, qt = item % p.ntile, nh = item / p.ntile;
  const int n = nh / p.H, hd = nh % p.H;
  const int qr = MH_ROWS * qt + 16 * w + li, qc = min(qr, p.Lq - 1);
  int kbeg, kend;
  key_range<KR>(p, n, p.Lk, kbeg, kend);
  const int kt0 = kbeg / MH_ROWS, kt1 = (kend + MH_ROWS - 1) / MH_ROWS;
  const T* kb = (const T*)p.k + (int64_t)n * p.sk_n + hd * DH;
  const T* vb = (const T*)p.v + (int64_t)n * p.sv_n + hd * DH;
  JMT_DCHECK(qc >= 0 && qc < p.Lq && n >= 0 && hd < p.H);
  F qf[NKS];
  {
    const T* qrow = (const T*)p.q + (int64_t)n * p.sq_n + hd * DH + (int64_t)qc * p.sq_l + 8 * g;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) qf[ks] = *(const F*)(qrow + 32 * ks);
  }
  mh_u32x4 kreg[NKS], vreg[NKS];
  if (kt0 < kt1) {
    mh_load<T, DH>(kreg, kb, p.sk_l, MH_ROWS * kt0, kbeg, kend, p.Lk);
    mh_load<T, DH>(vreg, vb, p.sv_l, MH_ROWS * kt0, kbeg, kend, p.Lk);
  }
  float m = -1e30f, l = 0.f;                       // running max (log2 units), this lane's sum
  f32x4 o[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  uint32_t dctr[4] = {0u, 0u, 0u, 0u}, dqb = 0u;   // DROP: the state copy, the lane's query block
  if constexpr (DROP) {
#pragma unroll
    for (int i = 0; i < 4; ++i) dctr[i] = __builtin_amdgcn_readfirstlane(p.dr.ctr[i]);
    dqb = (uint32_t)nh * p.dr.QB + (uint32_t)(qr >> 2);
  }

  for (int kt = kt0; kt < kt1; ++kt) {
    __syncthreads();                               // the previous tile's reads are done
    mh_store<DH>(kimg, kreg);
    mh_store<DH>(vimg, vreg);
    __syncthreads();
    if (kt + 1 < kt1) {                            // the next tile's loads fly under this tile
      mh_load<T, DH>(kreg, kb, p.sk_l, MH_ROWS * (kt + 1), kbeg, kend, p.Lk);
      mh_load<T, DH>(vreg, vb, p.sv_l, MH_ROWS * (kt + 1), kbeg, kend, p.Lk);
    }
    // DROP: this lane's Philox call (key block 16 kt + 4 j + g, j = li & 3) beside the score MFMAs
    uint32_t dm[4] = {0u, 0u, 0u, 0u};
    if constexpr (DROP)
      mh_drop_tile<true>(dctr, dqb, (uint32_t)(16 * kt + 4 * (li & 3) + g), li, dm);
    // s[c][r] = <query li, key 64 kt + 16 c + 4 g + r>
    f32x4 s[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      s[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks)
        s[c] = mfma16(mh_row<T, DH>(kimg, 16 * c + li, ks, g), qf[ks], s[c]);
    }
    float tmax = -1e30f;
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = MH_ROWS * kt + 16 * c + 4 * g + r;
        const bool in = key >= kbeg && key < kend;
        s[c][r] = in ? s[c][r] * p.scale_log2 : -1e30f;
        tmax = fmaxf(tmax, s[c][r]);
      }
    tmax = pl_pair_max(tmax);                      // over the row's 4 lanes: this row only
    const float mn = fmaxf(m, tmax);
    const float alpha = __builtin_amdgcn_exp2f(m - mn);
    m = mn;
    l *= alpha;
#pragma unroll
    for (int t = 0; t < NT; ++t) o[t] *= alpha;
    F pf[2];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = MH_ROWS * kt + 16 * c + 4 * g + r;
        const bool in = key >= kbeg && key < kend;
        const float pv = in ? __builtin_amdgcn_exp2f(s[c][r] - mn) : 0.f;
        l += pv;                                   // the sum stays unmasked: lse is the plain one
        if constexpr (DROP) pf[c >> 1][4 * (c & 1) + r] =
            from_f<T>(mh_masked(pv, mh_keep(dm[c], r, p.dr.T8)));
        else pf[c >> 1][4 * (c & 1) + r] = from_f<T>(pv);
      }
#pragma unroll
    for (int cc = 0; cc < 2; ++cc)
#pragma unroll
      for (int t = 0; t < NT; ++t)
        o[t] = mfma16(mh_tr<T, DH>(vimg, 32 * cc, t, li, g), pf[cc], o[t]);
  }
  l = pl_pair_sum(l);
  float inv = l > 0.f ? 1.f / l : 0.f;             // an empty range: zeros
  if constexpr (DROP) inv *= p.dr.s;               // the kept probabilities' scale
  JMT_DCHECK(qr < p.Lq || qc == p.Lq - 1);
  mh_store_row<T, DH>(o, inv, (T*)p.out + (int64_t)n * p.so_n + hd * DH + (int64_t)qr * p.so_l, g,
                      qr < p.Lq);
  if (qr < p.Lq && g == 0 && p.lse)
    p.lse[(int64_t)nh * p.Lq + qr] = (m + __builtin_amdgcn_logf(l)) * 0.69314718055994531f;
}

template <typename T, int DH, bool KR, bool DROP>
__global__ __launch_bounds__(256, 2) void attn_mh_dq_kernel(MhArgs<KR, DROP> p) {
  typedef typename Frag16<T>::t F;
  constexpr int NKS = DH / 32, NT = DH / 16, IMG = MH_ROWS * DH * 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* kimg = smem;
  char* vimg = smem + IMG;

  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int g = lane >> 4, li = lane & 15;
  const int item = blockIdx.x, qt = item % p.ntile, nh = item / p.ntile;
  const int n = nh / p.H, hd = nh % p.H;
  const int qr = MH_ROWS * qt + 16 * w + li, qc = min(qr, p.Lq - 1);
  int kbeg, kend;
  key_range<KR>(p, n, p.Lk, kbeg, kend);
  const int kt0 = kbeg / MH_ROWS, kt1 = (kend + MH_ROWS - 1) / MH_ROWS;
  const T* kb = (const T*)p.k + (int64_t)n * p.sk_n + hd * DH;
  const T* vb = (const T*)p.v + (int64_t)n * p.sv_n + hd * DH;
  JMT_DCHECK(qc >= 0 && qc < p.Lq && n >= 0 && hd < p.H);
  F qf[NKS], df[NKS];
  float delta = 0.f;
  {
    const int64_t c0 = (int64_t)hd * DH + 8 * g;
    const T* qrow = (const T*)p.q + (int64_t)n * p.sq_n + (int64_t)qc * p.sq_l + c0;
    const T* grow = (const T*)p.go + (int64_t)n * p.sgo_n + (int64_t)qc * p.sgo_l + c0;
    const T* orow = (const T*)p.o + (int64_t)n * p.so_n + (int64_t)qc * p.so_l + c0;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      qf[ks] = *(const F*)(qrow + 32 * ks);
      df[ks] = *(const F*)(grow + 32 * ks);
      const F of = *(const F*)(orow + 32 * ks);
#pragma unroll
      for (int e = 0; e < 8; ++e) delta += (float)of[e] * (float)df[ks][e];
    }
  }
  delta = pl_pair_sum(delta);
  const float lse2 = p.lse[(int64_t)nh * p.Lq + qc] * 1.4426950408889634f;
  mh_u32x4 kreg[NKS], vreg[NKS];
  if (kt0 < kt1) {
    mh_load<T, DH>(kreg, kb, p.sk_l, MH_ROWS * kt0, kbeg, kend, p.Lk);
    mh_load<T, DH>(vreg, vb, p.sv_l, MH_ROWS * kt0, kbeg, kend, p.Lk);
  }
  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  uint32_t dctr[4] = {0u, 0u, 0u, 0u}, dqb = 0u;   // DROP: as the forward
  if constexpr (DROP) {
#pragma unroll
    for (int i = 0; i < 4; ++i) dctr[i] = __builtin_amdgcn_readfirstlane(p.dr.ctr[i]);
    dqb = (uint32_t)nh * p.dr.QB + (uint32_t)(qr >> 2);
  }

  for (int kt = kt0; kt < kt1; ++kt) {
    __syncthreads();
    mh_store<DH>(kimg, kreg);
    mh_store<DH>(vimg, vreg);
    __syncthreads();
    if (kt + 1 < kt1) {
      mh_load<T, DH>(kreg, kb, p.sk_l, MH_ROWS * (kt + 1), kbeg, kend, p.Lk);
      mh_load<T, DH>(vreg, vb, p.sv_l, MH_ROWS * (kt + 1), kbeg, kend, p.Lk);
    }
    uint32_t dm[4] = {0u, 0u, 0u, 0u};
    if constexpr (DROP)
      mh_drop_tile<true>(dctr, dqb, (uint32_t)(16 * kt + 4 * (li & 3) + g), li, dm);
    F dsf[2];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f}, d = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        s = mfma16(mh_row<T, DH>(kimg, 16 * c + li, ks, g), qf[ks], s);
        d = mfma16(mh_row<T, DH>(vimg, 16 * c + li, ks, g), df[ks], d);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = MH_ROWS * kt + 16 * c + 4 * g + r;
        const bool in = key >= kbeg && key < kend;
        const float pv = in ? __builtin_amdgcn_exp2f(s[r] * p.scale_log2 - lse2) : 0.f;
        float dp = d[r];
        if constexpr (DROP) dp = mh_masked(dp * p.dr.s, mh_keep(dm[c], r, p.dr.T8));  // M o dO V^T
        dsf[c >> 1][4 * (c & 1) + r] = from_f<T>(in ? p.scale * pv * (dp - delta) : 0.f);
      }
    }
#pragma unroll
    for (int cc = 0; cc < 2; ++cc)
#pragma unroll
      for (int t = 0; t < NT; ++t)
        acc[t] = mfma16(mh_tr<T, DH>(kimg, 32 * cc, t, li, g), dsf[cc], acc[t]);
  }
  JMT_DCHECK(qr < p.Lq || qc == p.Lq - 1);
  mh_store_row<T, DH>(acc, 1.f,
                      (T*)p.dq + (int64_t)n * p.sdq_n + hd * DH + (int64_t)qr * p.sdq_l, g,
                      qr < p.Lq);
  if (qr < p.Lq && g == 0) p.delta[(int64_t)nh * p.Lq + qr] = delta;
}

template <typename T, int DH, bool KR, bool DROP>
__global__ __launch_bounds__(256, 2) void attn_mh_dkdv_kernel(MhArgs<KR, DROP> p) {
  typedef typename Frag16<T>::t F;
  constexpr int NKS = DH / 32, NT = DH / 16, IMG = MH_ROWS * DH * 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* qimg = smem;
  char* dimg = smem + IMG;
  float* rowc = (float*)(smem + 2 * IMG);          // lse log2e of the tile's 64 rows, then delta

  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int g = lane >> 4, li = lane & 15;
  const int item = blockIdx.x, kt = item % p.ntile, nh = item / p.ntile;
  const int n = nh / p.H, hd = nh % p.H;
  const int k0 = MH_ROWS * kt, kr = k0 + 16 * w + li, kc = min(kr, p.Lk - 1);
  int kbeg, kend;
  key_range<KR>(p, n, p.Lk, kbeg, kend);
  const bool kin = kr >= kbeg && kr < kend;
  JMT_DCHECK(kc >= 0 && kc < p.Lk && n >= 0 && hd < p.H);
  T* dkrow = (T*)p.dk + (int64_t)n * p.sdk_n + hd * DH + (int64_t)kr * p.sdk_l;
  T* dvrow = (T*)p.dv + (int64_t)n * p.sdv_n + hd * DH + (int64_t)kr * p.sdv_l;
  f32x4 dk[NT], dv[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) dk[t] = dv[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (KR && (k0 >= kend || k0 + MH_ROWS <= kbeg)) {   // block-uniform: no valid key in the tile
    mh_store_row<T, DH>(dk, 0.f, dkrow, g, kr < p.Lk);
    mh_store_row<T, DH>(dv, 0.f, dvrow, g, kr < p.Lk);
    return;
  }
  F kf[NKS], vf[NKS];
  {
    const T* krow = (const T*)p.k + (int64_t)n * p.sk_n + hd * DH + (int64_t)kc * p.sk_l + 8 * g;
    const T* vrow = (const T*)p.v + (int64_t)n * p.sv_n + hd * DH + (int64_t)kc * p.sv_l + 8 * g;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      kf[ks] = *(const F*)(krow + 32 * ks);
      vf[ks] = *(const F*)(vrow + 32 * ks);
    }
  }
  const T* qb = (const T*)p.q + (int64_t)n * p.sq_n + hd * DH;
  const T* gb = (const T*)p.go + (int64_t)n * p.sgo_n + hd * DH;
  const float* lrow = p.lse + (int64_t)nh * p.Lq;
  const float* drow = p.delta + (int64_t)nh * p.Lq;
  const int nqt = (p.Lq + MH_ROWS - 1) / MH_ROWS;
  mh_u32x4 qreg[NKS], greg[NKS];
  float creg = 0.f;
  // thread t < 64: lse of row t of the tile (in log2 units); 64 <= t < 128: delta of row t - 64
  auto load_consts = [&](int q0) {
    const int row = q0 + ((int)threadIdx.x & 63);
    creg = 0.f;
    if (threadIdx.x < 128 && row < p.Lq) {
      JMT_DCHECK(row >= 0);
      creg = threadIdx.x < 64 ? lrow[row] * 1.4426950408889634f : drow[row];
    }
  };
  mh_load<T, DH>(qreg, qb, p.sq_l, 0, 0, p.Lq, p.Lq);
  mh_load<T, DH>(greg, gb, p.sgo_l, 0, 0, p.Lq, p.Lq);
  load_consts(0);
  uint32_t dctr[4] = {0u, 0u, 0u, 0u}, dqb = 0u;   // DROP: the state copy, query block 4 j + g
  if constexpr (DROP) {
#pragma unroll
    for (int i = 0; i < 4; ++i) dctr[i] = __builtin_amdgcn_readfirstlane(p.dr.ctr[i]);
    dqb = (uint32_t)nh * p.dr.QB + (uint32_t)(4 * (li & 3) + g);
  }

  for (int qt = 0; qt < nqt; ++qt) {
    __syncthreads();
    mh_store<DH>(qimg, qreg);
    mh_store<DH>(dimg, greg);
    if (threadIdx.x < 128) rowc[threadIdx.x] = creg;
    __syncthreads();
    if (qt + 1 < nqt) {
      mh_load<T, DH>(qreg, qb, p.sq_l, MH_ROWS * (qt + 1), 0, p.Lq, p.Lq);
      mh_load<T, DH>(greg, gb, p.sgo_l, MH_ROWS * (qt + 1), 0, p.Lq, p.Lq);
      load_consts(MH_ROWS * (qt + 1));
    }
    // DROP: this lane's Philox call is query block 16 qt + 4 j + g (j = li & 3) of its key block
    uint32_t dm[4] = {0u, 0u, 0u, 0u};
    if constexpr (DROP)
      mh_drop_tile<false>(dctr, dqb + (uint32_t)(16 * qt), (uint32_t)(kr >> 2), li, dm);
    // s[r] = <query 64 qt + 16 c + 4 g + r, key kr>: the key on the lane
    F pf[2], dsf[2];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f}, d = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        s = mfma16(mh_row<T, DH>(qimg, 16 * c + li, ks, g), kf[ks], s);
        d = mfma16(mh_row<T, DH>(dimg, 16 * c + li, ks, g), vf[ks], d);
      }
      const f32x4 l4 = *(const f32x4*)(rowc + 16 * c + 4 * g);
      const f32x4 d4 = *(const f32x4*)(rowc + 64 + 16 * c + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qi = MH_ROWS * qt + 16 * c + 4 * g + r;
        const bool in = kin && qi < p.Lq;
        const float pv = in ? __builtin_amdgcn_exp2f(s[r] * p.scale_log2 - l4[r]) : 0.f;
        float dp = d[r];
        if constexpr (DROP) {
          // dV takes the masked P (its scale s waits for the store), dS the masked dP and the
          // plain P
          const uint32_t keep = mh_keep(dm[c], r, p.dr.T8);
          pf[c >> 1][4 * (c & 1) + r] = from_f<T>(mh_masked(pv, keep));
          dp = mh_masked(dp * p.dr.s, keep);
        } else {
          pf[c >> 1][4 * (c & 1) + r] = from_f<T>(pv);
        }
        dsf[c >> 1][4 * (c & 1) + r] = from_f<T>(in ? p.scale * pv * (dp - d4[r]) : 0.f);
      }
    }
#pragma unroll
    for (int cc = 0; cc < 2; ++cc)
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        dv[t] = mfma16(mh_tr<T, DH>(dimg, 32 * cc, t, li, g), pf[cc], dv[t]);
        dk[t] = mfma16(mh_tr<T, DH>(qimg, 32 * cc, t, li, g), dsf[cc], dk[t]);
      }
  }
  // keys of this tile outside the range: exact zeros (the buffers arrive uninitialised)
  JMT_DCHECK(kr < p.Lk || kc == p.Lk - 1);
  mh_store_row<T, DH>(dk, kin ? 1.f : 0.f, dkrow, g, kr < p.Lk);
  float vmul = 1.f;
  if constexpr (DROP) vmul = p.dr.s;
  mh_store_row<T, DH>(dv, kin ? vmul : 0.f, dvrow, g, kr < p.Lk);
}

static int64_t mh_tiles(int L) { return ((int64_t)L + MH_ROWS - 1) / MH_ROWS; }

static int mh_check(const char* name, int N, int H, const void* const* ptrs, int nptr,
                    const int64_t* strides, int nstr) {
  JMT_CHECK_ARG(N > 0 && H > 0, "%s: bad sizes (N %d H %d)", name, N, H);
  for (int i = 0; i < nptr; ++i)
    JMT_CHECK_ARG(ptrs[i] != nullptr && ((uintptr_t)ptrs[i] & 15) == 0,
                  "%s: operand %d null or not 16-B aligned", name, i);
  for (int i = 0; i < nstr; ++i)
    JMT_CHECK_ARG(strides[i] >= 0 && strides[i] % 8 == 0,
                  "%s: stride %d negative or not a multiple of 8 elements", name, i);
  return JMT_OK;
}

// launch K<T, DH, KR, DROP> for the runtime (dt, dh, kr, dr) on ntile-tile items
#define MH_LAUNCH(KERNEL, LDS_OF, a, kr, dr, dt, dh, grid, st)                                 \
  by_elem(dt, [&](auto e) {                                                                    \
    using T = typename decltype(e)::type;                                                      \
    auto go = [&](auto dhc) {                                                                  \
      constexpr int DH = decltype(dhc)::value;                                                 \
      constexpr int LDS = LDS_OF(DH);                                                          \
      auto run = [&](auto krc, auto drc) {                                                     \
        constexpr bool KR = decltype(krc)::value, DROP = decltype(drc)::value;                 \
        MhArgs<KR, DROP> ak;                                                                   \
        static_cast<AttnMhArgs&>(ak) = a;                                                      \
        if constexpr (KR) ak.kr = *kr;                                                         \
        if constexpr (DROP) ak.dr = *dr;                                                       \
        attn_launch<KERNEL<T, DH, KR, DROP>, LDS, 256>(grid, st, ak);                          \
      };                                                                                       \
      if (kr && dr) run(std::true_type{}, std::true_type{});                                   \
      else if (dr) run(std::false_type{}, std::true_type{});                                   \
      else if (kr) run(std::true_type{}, std::false_type{});                                   \
      else run(std::false_type{}, std::false_type{});                                          \
    };                                                                                         \
    if (dh == 64) go(std::integral_constant<int, 64>{});                                       \
    else go(std::integral_constant<int, 128>{});                                               \
  })
#define MH_LDS2(DH) (2 * MH_ROWS * (DH) * 2)                    /* two images */
#define MH_LDS2C(DH) (2 * MH_ROWS * (DH) * 2 + 2 * MH_ROWS * 4) /* + lse and delta of a tile */

}  // namespace jmt

using namespace jmt;

extern "C" int jmt_attn_mh_ok(int dt, int dh, int N, int H, int Lq, int Lk, int64_t sq_l,
                              int64_t sk_l, int64_t sv_l) {
  const int64_t smax = (1LL << 31) - 1;
  return (dt == JMT_BF16 || dt == JMT_F16) && (dh == 64 || dh == 128) && N >= 1 && H >= 1 &&
         Lq >= 1 && Lq <= MH_MAXL && Lk >= 1 && Lk <= MH_MAXL &&
         (int64_t)N * H * mh_tiles(Lq) <= smax && (int64_t)N * H * mh_tiles(Lk) <= smax &&
         sq_l >= 0 && sq_l <= smax && sk_l >= 0 && sk_l <= smax && sv_l >= 0 && sv_l <= smax;
}

static int mh_unsupported(const char* name, int dt, int dh, int N, int H, int Lq, int Lk) {
  return set_error(JMT_ERR_UNSUPPORTED,
                   "%s: dtype %d / head dim %d / N %d H %d Lq %d Lk %d / row strides outside "
                   "jmt_attn_mh_ok", name, dt, dh, N, H, Lq, Lk);
}

// The checks of the *_drop entry points on (p, ctr) and the counter limit N H QB <= 2^32; fills
// `d`.  d->T8 == 0 (p < 1 / 512): no mask, the caller launches the plain kernels.
static int mh_drop_check(const char* name, int N, int H, int Lq, float p, const uint32_t* ctr,
                         MhDrop* d) {
  JMT_CHECK_ARG(p >= 0.f && p < 1.f, "%s: dropout rate %g outside [0, 1)", name, (double)p);
  const uint32_t T8 = attn_dropout_threshold(p);
  JMT_CHECK_ARG(T8 <= 255u, "%s: dropout rate %g rounds to T8 = %u > 255 (the rate is quantised "
                "to 1 / 256)", name, (double)p, T8);
  JMT_CHECK_ARG(ctr != nullptr && ((uintptr_t)ctr & 3) == 0,
                "%s: dropout counter block null or not 4-B aligned", name);
  const uint32_t QB = attn_dropout_qblocks(Lq);
  if ((int64_t)N * H * QB > ((int64_t)1 << 32))
    return set_error(JMT_ERR_UNSUPPORTED, "%s: N %d H %d Lq %d: N H ceil(Lq / 4) exceeds the "
                     "dropout counter's 2^32 query blocks", name, N, H, Lq);
  d->ctr = ctr;
  d->T8 = T8;
  d->QB = QB;
  d->s = attn_dropout_scale(T8);
  return JMT_OK;
}

static void mh_fill(AttnMhArgs& a, int H, int Lq, int Lk, float scale) {
  a.H = H;
  a.Lq = Lq;
  a.Lk = Lk;
  a.scale = scale;
  a.scale_log2 = scale * 1.4426950408889634f;
}

// jmt_attn_mh_fwd (kr == NULL) and jmt_attn_mh_fwd_kr
static int mh_fwd_impl(const char* name, int dt, int N, int H, int Lq, int Lk, int dh,
                       const void* q, int64_t sq_l, int64_t sq_n, const void* k, int64_t sk_l,
                       int64_t sk_n, const void* v, int64_t sv_l, int64_t sv_n, void* o,
                       int64_t so_l, int64_t so_n, float scale, float* lse, const KeyRange* kr,
                       const MhDrop* dr, void* stream) {
  if (N == 0 || Lq == 0) return JMT_OK;
  if (!jmt_attn_mh_ok(dt, dh, N, H, Lq, Lk, sq_l, sk_l, sv_l))
    return mh_unsupported(name, dt, dh, N, H, Lq, Lk);
  const void* ptrs[] = {q, k, v, o};
  const int64_t strides[] = {sq_l, sq_n, sk_l, sk_n, sv_l, sv_n, so_l, so_n};
  int rc = mh_check(name, N, H, ptrs, 4, strides, 8);
  if (rc != JMT_OK) return rc;
  if (kr && (rc = key_range_check(name, N, kr->tab, kr->mod)) != JMT_OK) return rc;
  AttnMhArgs a = {};
  a.q = q; a.k = k; a.v = v; a.out = o; a.lse = lse;
  a.sq_l = sq_l; a.sq_n = sq_n; a.sk_l = sk_l; a.sk_n = sk_n; a.sv_l = sv_l; a.sv_n = sv_n;
  a.so_l = so_l; a.so_n = so_n;
  mh_fill(a, H, Lq, Lk, scale);
  a.ntile = (int)mh_tiles(Lq);
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)((int64_t)N * H * a.ntile));
  MH_LAUNCH(attn_mh_fwd_kernel, MH_LDS2, a, kr, dr, dt, dh, grid, st);
  JMT_LAUNCH_CHECK(name);
  return JMT_OK;
}

extern "C" int jmt_attn_mh_fwd(int dt, int N, int H, int Lq, int Lk, int dh, const void* q,
                               int64_t sq_l, int64_t sq_n, const void* k, int64_t sk_l,
                               int64_t sk_n, const void* v, int64_t sv_l, int64_t sv_n, void* o,
                               int64_t so_l, int64_t so_n, float scale, float* lse,
                               void* stream) {
  return mh_fwd_impl("jmt_attn_mh_fwd", dt, N, H, Lq, Lk, dh, q, sq_l, sq_n, k, sk_l, sk_n, v,
                     sv_l, sv_n, o, so_l, so_n, scale, lse, nullptr, nullptr, stream);
}

extern "C" int jmt_attn_mh_fwd_kr(int dt, int N, int H, int Lq, int Lk, int dh, const void* q,
                                  int64_t sq_l, int64_t sq_n, const void* k, int64_t sk_l,
                                  int64_t sk_n, const void* v, int64_t sv_l, int64_t sv_n, void* o,
                                  int64_t so_l, int64_t so_n, float scale, float* lse,
                                  const int* kr, int kr_mod, void* stream) {
  const KeyRange r = {kr, kr_mod};
  return mh_fwd_impl("jmt_attn_mh_fwd_kr", dt, N, H, Lq, Lk, dh, q, sq_l, sq_n, k, sk_l, sk_n, v,
                     sv_l, sv_n, o, so_l, so_n, scale, lse, &r, nullptr, stream);
}

// jmt_attn_mh_bwd (kr == NULL) and jmt_attn_mh_bwd_kr: the dQ kernel, then the dK / dV kernel
static int mh_bwd_impl(const char* name, int dt, int N, int H, int Lq, int Lk, int dh,
                       const void* go, int64_t sgo_l, int64_t sgo_n, const void* o, int64_t so_l,
                       int64_t so_n, const void* q, int64_t sq_l, int64_t sq_n, const void* k,
                       int64_t sk_l, int64_t sk_n, const void* v, int64_t sv_l, int64_t sv_n,
                       const float* lse, void* dq, int64_t sdq_l, int64_t sdq_n, void* dk,
                       int64_t sdk_l, int64_t sdk_n, void* dv, int64_t sdv_l, int64_t sdv_n,
                       float scale, float* delta, const KeyRange* kr, const MhDrop* dr,
                       void* stream) {
  if (N == 0 || Lq == 0) return JMT_OK;
  if (!jmt_attn_mh_ok(dt, dh, N, H, Lq, Lk, sq_l, sk_l, sv_l))
    return mh_unsupported(name, dt, dh, N, H, Lq, Lk);
  const void* ptrs[] = {go, o, q, k, v, dq, dk, dv};
  const int64_t strides[] = {sgo_l, sgo_n, so_l, so_n, sq_l, sq_n, sk_l, sk_n, sv_l, sv_n,
                             sdq_l, sdq_n, sdk_l, sdk_n, sdv_l, sdv_n};
  int rc = mh_check(name, N, H, ptrs, 8, strides, 16);
  if (rc != JMT_OK) return rc;
  JMT_CHECK_ARG(lse != nullptr && ((uintptr_t)lse & 3) == 0, "%s: lse missing or misaligned",
                name);
  JMT_CHECK_ARG(delta != nullptr && ((uintptr_t)delta & 3) == 0,
                "%s: delta workspace missing or misaligned", name);
  if (kr && (rc = key_range_check(name, N, kr->tab, kr->mod)) != JMT_OK) return rc;
  AttnMhArgs a = {};
  a.q = q; a.k = k; a.v = v; a.o = o; a.go = go; a.lse = (float*)lse; a.delta = delta;
  a.dq = dq; a.dk = dk; a.dv = dv;
  a.sq_l = sq_l; a.sq_n = sq_n; a.sk_l = sk_l; a.sk_n = sk_n; a.sv_l = sv_l; a.sv_n = sv_n;
  a.so_l = so_l; a.so_n = so_n; a.sgo_l = sgo_l; a.sgo_n = sgo_n;
  a.sdq_l = sdq_l; a.sdq_n = sdq_n; a.sdk_l = sdk_l; a.sdk_n = sdk_n; a.sdv_l = sdv_l;
  a.sdv_n = sdv_n;
  mh_fill(a, H, Lq, Lk, scale);
  hipStream_t st = as_stream(stream);
  {
    a.ntile = (int)mh_tiles(Lq);
    const dim3 grid((unsigned)((int64_t)N * H * a.ntile));
    MH_LAUNCH(attn_mh_dq_kernel, MH_LDS2, a, kr, dr, dt, dh, grid, st);
    JMT_LAUNCH_CHECK(name);
  }
  {
    a.ntile = (int)mh_tiles(Lk);
    const dim3 grid((unsigned)((int64_t)N * H * a.ntile));
    MH_LAUNCH(attn_mh_dkdv_kernel, MH_LDS2C, a, kr, dr, dt, dh, grid, st);
    JMT_LAUNCH_CHECK(name);
  }
  return JMT_OK;
}

extern "C" int jmt_attn_mh_bwd(int dt, int N, int H, int Lq, int Lk, int dh, const void* go,
                               int64_t sgo_l, int64_t sgo_n, const void* o, int64_t so_l,
                               int64_t so_n, const void* q, int64_t sq_l, int64_t sq_n,
                               const void* k, int64_t sk_l, int64_t sk_n, const void* v,
                               int64_t sv_l, int64_t sv_n, const float* lse, void* dq,
                               int64_t sdq_l, int64_t sdq_n, void* dk, int64_t sdk_l,
                               int64_t sdk_n, void* dv, int64_t sdv_l, int64_t sdv_n, float scale,
                               float* delta, void* stream) {
  return mh_bwd_impl("jmt_attn_mh_bwd", dt, N, H, Lq, Lk, dh, go, sgo_l, sgo_n, o, so_l, so_n, q,
                     sq_l, sq_n, k, sk_l, sk_n, v, sv_l, sv_n, lse, dq, sdq_l, sdq_n, dk, sdk_l,
                     sdk_n, dv, sdv_l, sdv_n, scale, delta, nullptr, nullptr, stream);
}

extern "C" int jmt_attn_mh_bwd_kr(int dt, int N, int H, int Lq, int Lk, int dh, const void* go,
                                  int64_t sgo_l, int64_t sgo_n, const void* o, int64_t so_l,
                                  int64_t so_n, const void* q, int64_t sq_l, int64_t sq_n,
                                  const void* k, int64_t sk_l, int64_t sk_n, const void* v,
                                  int64_t sv_l, int64_t sv_n, const float* lse, void* dq,
                                  int64_t sdq_l, int64_t sdq_n, void* dk, int64_t sdk_l,
                                  int64_t sdk_n, void* dv, int64_t sdv_l, int64_t sdv_n,
                                  float scale, float* delta, const int* kr, int kr_mod,
                                  void* stream) {
  const KeyRange r = {kr, kr_mod};
  return mh_bwd_impl("jmt_attn_mh_bwd_kr", dt, N, H, Lq, Lk, dh, go, sgo_l, sgo_n, o, so_l, so_n,
                     q, sq_l, sq_n, k, sk_l, sk_n, v, sv_l, sv_n, lse, dq, sdq_l, sdq_n, dk,
                     sdk_l, sdk_n, dv, sdv_l, sdv_n, scale, delta, &r, nullptr, stream);
}

// jmt_attn_mh_fwd_drop / jmt_attn_mh_bwd_drop: attention dropout on the probabilities (the mask
// of dropout.h), with or without a range table (kr == NULL: none).  T8 == 0: the plain kernels.
extern "C" int jmt_attn_mh_fwd_drop(int dt, int N, int H, int Lq, int Lk, int dh, const void* q,
                                    int64_t sq_l, int64_t sq_n, const void* k, int64_t sk_l,
                                    int64_t sk_n, const void* v, int64_t sv_l, int64_t sv_n,
                                    void* o, int64_t so_l, int64_t so_n, float scale, float* lse,
                                    const int* kr, int kr_mod, float p, const uint32_t* ctr,
                                    void* stream) {
  const char* name = "jmt_attn_mh_fwd_drop";
  if (N == 0 || Lq == 0) return JMT_OK;
  if (!jmt_attn_mh_ok(dt, dh, N, H, Lq, Lk, sq_l, sk_l, sv_l))
    return mh_unsupported(name, dt, dh, N, H, Lq, Lk);
  MhDrop d = {};
  const int rc = mh_drop_check(name, N, H, Lq, p, ctr, &d);
  if (rc != JMT_OK) return rc;
  const KeyRange r = {kr, kr_mod};
  return mh_fwd_impl(name, dt, N, H, Lq, Lk, dh, q, sq_l, sq_n, k, sk_l, sk_n, v, sv_l, sv_n, o,
                     so_l, so_n, scale, lse, kr ? &r : nullptr, d.T8 ? &d : nullptr, stream);
}

extern "C" int jmt_attn_mh_bwd_drop(int dt, int N, int H, int Lq, int Lk, int dh, const void* go,
                                    int64_t sgo_l, int64_t sgo_n, const void* o, int64_t so_l,
                                    int64_t so_n, const void* q, int64_t sq_l, int64_t sq_n,
                                    const void* k, int64_t sk_l, int64_t sk_n, const void* v,
                                    int64_t sv_l, int64_t sv_n, const float* lse, void* dq,
                                    int64_t sdq_l, int64_t sdq_n, void* dk, int64_t sdk_l,
                                    int64_t sdk_n, void* dv, int64_t sdv_l, int64_t sdv_n,
                                    float scale, float* delta, const int* kr, int kr_mod, float p,
                                    const uint32_t* ctr, void* stream) {
  const char* name = "jmt_attn_mh_bwd_drop";
  if (N == 0 || Lq == 0) return JMT_OK;
  if (!jmt_attn_mh_ok(dt, dh, N, H, Lq, Lk, sq_l, sk_l, sv_l))
    return mh_unsupported(name, dt, dh, N, H, Lq, Lk);
  MhDrop d = {};
  const int rc = mh_drop_check(name, N, H, Lq, p, ctr, &d);
  if (rc != JMT_OK) return rc;
  const KeyRange r = {kr, kr_mod};
  return mh_bwd_impl(name, dt, N, H, Lq, Lk, dh, go, sgo_l, sgo_n, o, so_l, so_n, q, sq_l, sq_n, k,
                     sk_l, sk_n, v, sv_l, sv_n, lse, dq, sdq_l, sdq_n, dk, sdk_l, sdk_n, dv, sdv_l,
                     sdv_n, scale, delta, kr ? &r : nullptr, d.T8 ? &d : nullptr, stream);
}
