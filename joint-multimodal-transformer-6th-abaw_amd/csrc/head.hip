// Output layer of the V / A regressor pair (two_transformers.py:104-114: Linear(dim, 128) ->
// ReLU -> Dropout(0) -> Linear(128, k), applied to the same input by `vregressor` and
// `aregressor`, :125-126) as two small row kernels instead of three GEMM launches.
//
// The two heads read the halves of ONE hidden buffer h = [h_0 | h_1] (rows x 2*128, row stride
// ldh, 16-bit; the first layers' grouped GEMM writes it, ReLU applied):
//   forward : y_g[r][o]  = sum_j h_g[r][j] W2_g[o][j] + b2_g[o]          (fp32 accumulation)
//   backward: dh_g[r][j] = [h_g[r][j] > 0] sum_o gy_g[r][o] W2_g[o][j]     (16-bit out)
//             dW2_g[o][j] += sum_r gy_g[r][o] h_g[r][j],  db2_g[o] += sum_r gy_g[r][o]
// k = nout <= 24 (1 for the V / A regressors, 20 for configs[4]'s expression-style head).
// With dropout (v_dropout / a_dropout > 0, the jmt_head_*_drop entries) h above is h~ = m . h,
// the mask m regenerated per lane from its counter (dropout.h), and dh carries the scale s.
//
// A wave owns one row at a time: lanes 0-31 head 0, lanes 32-63 head 1, each lane 4 consecutive
// hidden units, so a row of h is one 512-B coalesced access; the k dot products reduce over the
// head's 32 lanes with xor shuffles.  The weight / bias gradients are sums over all B*T rows:
// per-lane fp32 accumulators, summed over the block's waves in LDS in a fixed order, one fp32
// slab per block, and a fixed-order reduce over the blocks (deterministic; the graph replay is
// bit-identical to eager).  The weight gradient is an exact fp32 sum of fp32 gy x (16-bit h as
// fp32), as the GEMM path's fp32 route did (functional.MLPFn: these sums nearly cancel for the
// CCC loss, so a 16-bit rounded copy of gy is avoided).
//
// Replaces, per step (B=64, T=300): the N = 1 forward GEMM (10 us), the K = 1 masked dgrad GEMM
// (16 us), the M = 1 fp32 weight-gradient GEMM with its 256-way split-K (36 us) and the bias
// column sum; HBM-bound: the kernels read h once (9.8 MB) and write dh once.
//
// Row loads are issued ahead: a wave loads its rows of h (and, backward, of gy) into registers in
// batches before the shuffle / accumulate chain that consumes them, instead of one dependent load
// per row; rows >= `rows` are predicated off (no load is issued past the last row).  Every sum
// keeps its order, so the results are those of the row-at-a-time walk, bit for bit.
//
// The PERM instantiations (jmt_head_*_perm) store y and read gy through a row map: memory row r
// of h pairs with row (r mod P) * Q + r div P of y / gy, P * Q = rows.  With h in (B, T) memory
// order and P = T, Q = B the predictions come out as a contiguous (T, B, k) tensor — the
// seq-first layout two_transformers.py returns — without a transposing copy after the kernel.
#include <type_traits>

#include "common.h"
#include "dropout.h"

namespace jmt {

constexpr int HD_HID = 128;        // hidden width of the regressors (two_transformers.py:104)
constexpr int HD_KMAX = 24;        // largest k of the fused path
constexpr int HD_RPW = 16;         // rows per wave per block

template <typename T> struct V4l;   // 4 consecutive 16-bit values <-> 8-B accesses
template <> struct V4l<__bf16> {
  static __device__ __forceinline__ void cvt(const uint2 u, float* v) {
    const __bf16* e = (const __bf16*)&u;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (float)e[i];
  }
  static __device__ __forceinline__ void ld(const __bf16* p, float* v) { cvt(*(const uint2*)p, v); }
  static __device__ __forceinline__ void st(__bf16* p, const float* v) {
    __bf16 e[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) e[i] = (__bf16)v[i];
    *(uint2*)p = *(const uint2*)e;
  }
};
template <> struct V4l<_Float16> {
  static __device__ __forceinline__ void cvt(const uint2 u, float* v) {
    const _Float16* e = (const _Float16*)&u;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (float)e[i];
  }
  static __device__ __forceinline__ void ld(const _Float16* p, float* v) {
    cvt(*(const uint2*)p, v);
  }
  static __device__ __forceinline__ void st(_Float16* p, const float* v) {
    _Float16 e[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) e[i] = (_Float16)v[i];
    *(uint2*)p = *(const uint2*)e;
  }
};

// a lane's quad of row r as loaded; `in` false: no load is issued
template <bool FULL>
__device__ __forceinline__ uint2 ld_quad(const void* p, bool in) {
  uint2 u = make_uint2(0u, 0u);
  if (FULL || in) u = *(const uint2*)p;
  return u;
}

// rows a wave loads ahead of the chain that consumes them: all 16 for k = 1 (8 B of h and one gy
// per row and lane); the k <= 24 kernels hold k quads of weights (and, backward, of weight
// gradient sums) per lane and batch fewer
template <int K> struct HeadAhead {
  static constexpr int FWD = K == 1 ? HD_RPW : 4;
  static constexpr int BWD = K == 1 ? HD_RPW : 2;
};

// the row of y / gy that pairs with memory row r of h, walked row by row: (r mod P) * Q + r div P
struct RowWalk {
  uint32_t m, d, P;
  int64_t Q;
  __device__ __forceinline__ RowWalk(int64_t r, int64_t P_, int64_t Q_)
      : m((uint32_t)r % (uint32_t)P_), d((uint32_t)r / (uint32_t)P_), P((uint32_t)P_), Q(Q_) {}
  __device__ __forceinline__ int64_t row() const { return (int64_t)m * Q + d; }
  __device__ __forceinline__ void next() {
    if (++m == P) { m = 0; ++d; }
  }
};

// sum over the 32 lanes of this lane's half-wave
__device__ __forceinline__ float half_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 8, 64);
  v += __shfl_xor(v, 4, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 1, 64);
  return v;
}

struct HeadArgs {
  const void* h;
  int64_t ldh;
  const void* w2[2];     // (k, 128) each, compute dtype
  const float* b2[2];
  void* y[2];            // forward outputs (rows, k) at row stride ldy
  int64_t ldy;
  const void* gy[2];     // backward: incoming gradients (rows, k) at row stride ldgy
  int64_t ldgy;
  void* dh;              // backward: (rows, 256) at row stride lddh
  int64_t lddh;
  float* partials;       // backward: per block 2 * k * (128 + 1) floats
  float* dw2[2];
  float* db2[2];
  int64_t rows;
  int k;
  int64_t P, Q;          // row map of y / gy (the PERM instantiations; P * Q = rows < 2^31)
};

// Dropout between the ReLU and the output layers (the DROP instantiations: jmt_head_*_drop).  A
// lane's 4 hidden units are quad `lane` of row r of the (rows x 256) buffer: one Philox call
// (dropout.h) gives their multipliers, h~ = m . h is formed in fp32 registers and never stored.
struct HeadDrop {
  uint32_t T[2];         // keep thresholds of the two halves
  float s[2];            // 1 / (1 - p) of the two halves
  const uint32_t* ctr;   // the forward's copy of the state block (jmt_dropout_next)
};

// The DROP kernels take HeadArgs with the mask arguments appended; the plain ones keep their
// parameter (and with it their code, down to the offsets of the implicit arguments).
struct HeadArgsDrop : HeadArgs {
  HeadDrop dr;
};
template <bool DROP> struct HeadParam { typedef HeadArgs t; };
template <> struct HeadParam<true> { typedef HeadArgsDrop t; };

template <typename TH, typename TY, int K, bool DROP, bool PERM>
__global__ __launch_bounds__(256) void head_fwd_kernel(typename HeadParam<DROP>::t a) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int g = lane >> 5, c = 4 * (lane & 31);
  const int k = K == 1 ? 1 : a.k;
  float wv[K][4];
  const TH* W = (const TH*)a.w2[g];
#pragma unroll
  for (int o = 0; o < K; ++o)
    if (o < k) V4l<TH>::ld(W + o * HD_HID + c, wv[o]);
  // the biases once, in registers (a load per stored element would wait on the rows in flight)
  const float* bp = a.b2[g];
  float bv[K];
#pragma unroll
  for (int o = 0; o < K; ++o) bv[o] = (bp && o < k) ? bp[o] : 0.f;
  TY* yp = (TY*)a.y[g];
  uint32_t ctr[4] = {0u, 0u, 0u, 0u}, dT = 0u;
  float ds = 1.f;
  if constexpr (DROP) {
#pragma unroll
    for (int e = 0; e < 4; ++e) ctr[e] = a.dr.ctr[e];
    dT = g ? a.dr.T[1] : a.dr.T[0];
    ds = g ? a.dr.s[1] : a.dr.s[0];
  }
  const int64_t r0 = ((int64_t)blockIdx.x * 4 + w) * HD_RPW;
  if (r0 >= a.rows) return;
  const TH* hp = (const TH*)a.h + g * HD_HID + c;
  constexpr int NB = HeadAhead<K>::FWD;
  // FULL: all 16 rows of the wave exist (every load unconditional); else the last wave's walk
  auto walk = [&](auto full) {
    constexpr bool FULL = decltype(full)::value;
    RowWalk rw(PERM ? r0 : 0, PERM ? a.P : 1, PERM ? a.Q : 1);
    for (int i0 = 0; i0 < HD_RPW; i0 += NB) {
      if (!FULL && r0 + i0 >= a.rows) break;
      uint2 raw[NB];
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const int64_t r = r0 + i0 + j;
        raw[j] = ld_quad<FULL>(hp + r * a.ldh, r < a.rows);
      }
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const int64_t r = r0 + i0 + j;
        if (!FULL && r >= a.rows) continue;   // (no break: raw[] must stay in registers)
        const int64_t yr = PERM ? rw.row() : r;
        if (PERM) rw.next();
        float hv[4];
        V4l<TH>::cvt(raw[j], hv);
        if (DROP) {
          float m[4];
          dropout_quad(ctr, (uint32_t)r, (uint32_t)lane, dT, ds, m);
#pragma unroll
          for (int e = 0; e < 4; ++e) hv[e] *= m[e];
        }
#pragma unroll
        for (int o = 0; o < K; ++o) {
          if (o < k) {            // (no break: the loop must unroll to keep wv in registers)
            float s = hv[0] * wv[o][0] + hv[1] * wv[o][1] + hv[2] * wv[o][2] + hv[3] * wv[o][3];
            s = half_sum(s);
            if ((lane & 31) == 0) yp[yr * a.ldy + o] = from_f<TY>(s + bv[o]);
          }
        }
      }
    }
  };
  if (r0 + HD_RPW <= a.rows) walk(std::true_type{});
  else walk(std::false_type{});
}

template <typename TH, typename TG, int K, bool DROP, bool PERM>
__global__ __launch_bounds__(256) void head_bwd_kernel(typename HeadParam<DROP>::t a) {
  __shared__ float red[2][HD_KMAX * HD_HID + HD_KMAX];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int g = lane >> 5, c = 4 * (lane & 31);
  const int k = K == 1 ? 1 : a.k;
  float wv[K][4], aw[K][4], ab[K];
  const TH* W = (const TH*)a.w2[g];
#pragma unroll
  for (int o = 0; o < K; ++o) {
    if (o < k) V4l<TH>::ld(W + o * HD_HID + c, wv[o]);
    ab[o] = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) aw[o][e] = 0.f;
  }
  const TG* gp = (const TG*)a.gy[g];
  uint32_t ctr[4] = {0u, 0u, 0u, 0u}, dT = 0u;
  float ds = 1.f;
  if constexpr (DROP) {
#pragma unroll
    for (int e = 0; e < 4; ++e) ctr[e] = a.dr.ctr[e];
    dT = g ? a.dr.T[1] : a.dr.T[0];
    ds = g ? a.dr.s[1] : a.dr.s[0];
  }
  const int64_t r0 = ((int64_t)blockIdx.x * 4 + w) * HD_RPW;
  const TH* hp = (const TH*)a.h + g * HD_HID + c;
  constexpr int NB = HeadAhead<K>::BWD;
  // (a wave past the last row walks nothing and adds its zero sums to the block's, as before)
  auto walk = [&](auto full) {
    constexpr bool FULL = decltype(full)::value;
    RowWalk rw(PERM ? r0 : 0, PERM ? a.P : 1, PERM ? a.Q : 1);
    for (int i0 = 0; i0 < HD_RPW; i0 += NB) {
      if (!FULL && r0 + i0 >= a.rows) break;
      uint2 raw[NB];
      TG gq[NB][K];
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const int64_t r = r0 + i0 + j;
        const bool in = r < a.rows;
        raw[j] = ld_quad<FULL>(hp + r * a.ldh, in);
        const int64_t yr = PERM ? rw.row() : r;
        if (PERM) rw.next();
#pragma unroll
        for (int o = 0; o < K; ++o) {
          gq[j][o] = from_f<TG>(0.f);
          if (o < k && (FULL || in)) gq[j][o] = gp[yr * a.ldgy + o];
        }
      }
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const int64_t r = r0 + i0 + j;
        if (!FULL && r >= a.rows) continue;   // (no break: raw[] / gq[] must stay in registers)
        float hv[4], d[4] = {0.f, 0.f, 0.f, 0.f};
        V4l<TH>::cvt(raw[j], hv);
        if (DROP) {
          float m[4];
          dropout_quad(ctr, (uint32_t)r, (uint32_t)lane, dT, ds, m);
#pragma unroll
          for (int e = 0; e < 4; ++e) hv[e] *= m[e];
        }
#pragma unroll
        for (int o = 0; o < K; ++o) {
          if (o < k) {
            const float gy = to_f(gq[j][o]);
            ab[o] += gy;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              d[e] += gy * wv[o][e];
              aw[o][e] += gy * hv[e];
            }
          }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) d[e] = hv[e] > 0.f ? (DROP ? ds * d[e] : d[e]) : 0.f;
        V4l<TH>::st((TH*)a.dh + r * a.lddh + g * HD_HID + c, d);
      }
    }
  };
  if (r0 + HD_RPW <= a.rows) walk(std::true_type{});
  else if (r0 < a.rows) walk(std::false_type{});
  // block sum of the weight / bias gradient partials, waves added in a fixed order
  for (int ww = 0; ww < 4; ++ww) {
    if (w == ww) {
#pragma unroll
      for (int o = 0; o < K; ++o) {
        if (o < k) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float& t = red[g][o * HD_HID + c + e];
            t = ww == 0 ? aw[o][e] : t + aw[o][e];
          }
          if ((lane & 31) == 0) {
            float& t = red[g][HD_KMAX * HD_HID + o];
            t = ww == 0 ? ab[o] : t + ab[o];
          }
        }
      }
    }
    __syncthreads();
  }
  // compact slab of this block: per head k*128 weight sums then k bias sums
  const int SK = k * (HD_HID + 1);
  float* slab = a.partials + (int64_t)blockIdx.x * 2 * SK;
  for (int i = threadIdx.x; i < 2 * SK; i += blockDim.x) {
    const int gg = i / SK, j = i % SK;
    slab[i] = j < k * HD_HID ? red[gg][j] : red[gg][HD_KMAX * HD_HID + (j - k * HD_HID)];
  }
}

// fixed-order sum of the blocks' slabs into the gradient buffers (+=): one wave per output
// (wave-uniform index), lane l adds slabs l, l + 64, ... in order, then a fixed xor butterfly;
// lane 0 stores.  (One thread per output walking all ~300 slabs serially was a 74 us chain of
// dependent L2 loads per step: profiles/r03_p1_kernel_stats.csv.)
__global__ __launch_bounds__(256) void head_reduce_kernel(HeadArgs a, int nblk) {
  const int SK = a.k * (HD_HID + 1);
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= 2 * SK) return;
  const int g = i / SK, j = i % SK;
  const bool isw = j < a.k * HD_HID;
  float* dst = isw ? a.dw2[g] : a.db2[g];
  if (!dst) return;
  float s = 0.f;
  for (int b = lane; b < nblk; b += 64) s += a.partials[(int64_t)b * 2 * SK + i];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) dst[isw ? j : j - a.k * HD_HID] += s;
}

static int head_blocks(int64_t rows) { return (int)((rows + 4 * HD_RPW - 1) / (4 * HD_RPW)); }

}  // namespace jmt

using namespace jmt;

extern "C" size_t jmt_head_bwd_workspace_bytes(int64_t rows) {
  return (size_t)head_blocks(rows) * 2 * (HD_KMAX * HD_HID + HD_KMAX) * sizeof(float);
}

static int head_check(const char* name, int h_dt, int64_t rows, int hid, int k, const void* h,
                      int64_t ldh, const void* w0, const void* w1) {
  JMT_CHECK_ARG(h_dt == JMT_BF16 || h_dt == JMT_F16, "%s: h must be bf16 / f16", name);
  JMT_CHECK_ARG(hid == HD_HID, "%s: hidden width %d (128 supported)", name, hid);
  JMT_CHECK_ARG(k >= 1 && k <= HD_KMAX, "%s: k = %d (1..%d supported)", name, k, HD_KMAX);
  JMT_CHECK_ARG(rows >= 0 && h && w0 && w1, "%s: null pointer", name);
  JMT_CHECK_ARG(ldh % 4 == 0 && ((uintptr_t)h & 7) == 0 && ((uintptr_t)w0 & 7) == 0 &&
                    ((uintptr_t)w1 & 7) == 0, "%s: h / W2 not 8-B aligned", name);
  return JMT_OK;
}

// the *_drop entries' mask arguments -> HeadDrop
static int head_drop_args(const char* name, int64_t rows, float p0, float p1, const uint32_t* ctr,
                          HeadDrop* dr) {
  JMT_CHECK_ARG(ctr && ((uintptr_t)ctr & 3) == 0, "%s: null counter block", name);
  JMT_CHECK_ARG(p0 >= 0.f && p0 < 1.f && p1 >= 0.f && p1 < 1.f, "%s: rates must be in [0, 1)",
                name);
  JMT_CHECK_ARG(rows < ((int64_t)1 << 32), "%s: rows = %lld (the counter holds 32 bits of row)",
                name, (long long)rows);
  dr->T[0] = dropout_threshold(p0); dr->T[1] = dropout_threshold(p1);
  dr->s[0] = dropout_scale(p0); dr->s[1] = dropout_scale(p1);
  dr->ctr = ctr;
  return JMT_OK;
}

// the *_perm entries' row map -> HeadArgs (P * Q = rows; the kernels walk it in 32 bits)
static int head_perm_args(const char* name, int64_t rows, int64_t P, int64_t Q, HeadArgs* a) {
  JMT_CHECK_ARG(rows < ((int64_t)1 << 31), "%s: rows = %lld (the row map walks 31 bits)", name,
                (long long)rows);
  JMT_CHECK_ARG(P >= 1 && Q >= 1 && P <= rows && Q <= rows && P * Q == rows,
                "%s: row map P = %lld, Q = %lld does not tile rows = %lld (P * Q = rows)", name,
                (long long)P, (long long)Q, (long long)rows);
  a->P = P; a->Q = Q;
  return JMT_OK;
}

// perm: the row map (P, Q) applies to y (the *_perm entries); else y is stored in h's row order
static int head_fwd_impl(const char* name, int h_dt, int y_dt, int64_t rows, int hid, int k,
                         const void* h, int64_t ldh, const void* w2_0, const void* w2_1,
                         const float* b2_0, const float* b2_1, void* y_0, void* y_1, int64_t ldy,
                         bool perm, int64_t P, int64_t Q, const HeadDrop* drop, void* stream) {
  int rc = head_check(name, h_dt, rows, hid, k, h, ldh, w2_0, w2_1);
  if (rc != JMT_OK) return rc;
  JMT_CHECK_ARG(y_dt == JMT_F32 || y_dt == h_dt, "%s: y dtype", name);
  JMT_CHECK_ARG(y_0 && y_1 && ldy >= k, "%s: outputs", name);
  if (rows == 0) return JMT_OK;
  HeadArgs a = {};
  a.h = h; a.ldh = ldh; a.w2[0] = w2_0; a.w2[1] = w2_1; a.b2[0] = b2_0; a.b2[1] = b2_1;
  a.y[0] = y_0; a.y[1] = y_1; a.ldy = ldy; a.rows = rows; a.k = k; a.P = rows; a.Q = 1;
  if (perm && (rc = head_perm_args(name, rows, P, Q, &a)) != JMT_OK) return rc;
  HeadArgsDrop ad = {};
  (HeadArgs&)ad = a;
  if (drop) ad.dr = *drop;
  const dim3 grid(head_blocks(rows));
  hipStream_t st = as_stream(stream);
#define HFWD2(TH, TY, K, PM)                                                                   \
  {                                                                                            \
    if (drop)                                                                                  \
      hipLaunchKernelGGL((head_fwd_kernel<TH, TY, K, true, PM>), grid, dim3(256), 0, st, ad);  \
    else hipLaunchKernelGGL((head_fwd_kernel<TH, TY, K, false, PM>), grid, dim3(256), 0, st, a); \
  }
#define HFWD1(TH, TY, K)              \
  {                                   \
    if (perm) HFWD2(TH, TY, K, true)  \
    else HFWD2(TH, TY, K, false)      \
  }
#define HFWD(TH, TY)                  \
  {                                   \
    if (k == 1) HFWD1(TH, TY, 1)      \
    else HFWD1(TH, TY, HD_KMAX)       \
  }
  if (h_dt == JMT_BF16) {
    if (y_dt == JMT_F32) HFWD(__bf16, float) else HFWD(__bf16, __bf16)
  } else {
    if (y_dt == JMT_F32) HFWD(_Float16, float) else HFWD(_Float16, _Float16)
  }
#undef HFWD
#undef HFWD1
#undef HFWD2
  JMT_LAUNCH_CHECK(name);
  return JMT_OK;
}

extern "C" int jmt_head_fwd(int h_dt, int y_dt, int64_t rows, int hid, int k, const void* h,
                            int64_t ldh, const void* w2_0, const void* w2_1, const float* b2_0,
                            const float* b2_1, void* y_0, void* y_1, int64_t ldy, void* stream) {
  return head_fwd_impl("jmt_head_fwd", h_dt, y_dt, rows, hid, k, h, ldh, w2_0, w2_1, b2_0, b2_1,
                       y_0, y_1, ldy, false, 0, 0, nullptr, stream);
}

extern "C" int jmt_head_fwd_perm(int h_dt, int y_dt, int64_t rows, int hid, int k, const void* h,
                                 int64_t ldh, const void* w2_0, const void* w2_1,
                                 const float* b2_0, const float* b2_1, void* y_0, void* y_1,
                                 int64_t ldy, int64_t P, int64_t Q, void* stream) {
  return head_fwd_impl("jmt_head_fwd_perm", h_dt, y_dt, rows, hid, k, h, ldh, w2_0, w2_1, b2_0,
                       b2_1, y_0, y_1, ldy, true, P, Q, nullptr, stream);
}

extern "C" int jmt_head_fwd_drop(int h_dt, int y_dt, int64_t rows, int hid, int k, const void* h,
                                 int64_t ldh, const void* w2_0, const void* w2_1,
                                 const float* b2_0, const float* b2_1, void* y_0, void* y_1,
                                 int64_t ldy, float p0, float p1, const uint32_t* ctr,
                                 void* stream) {
  HeadDrop dr = {};
  int rc = head_drop_args("jmt_head_fwd_drop", rows, p0, p1, ctr, &dr);
  if (rc != JMT_OK) return rc;
  return head_fwd_impl("jmt_head_fwd_drop", h_dt, y_dt, rows, hid, k, h, ldh, w2_0, w2_1, b2_0,
                       b2_1, y_0, y_1, ldy, false, 0, 0, &dr, stream);
}

extern "C" int jmt_head_fwd_perm_drop(int h_dt, int y_dt, int64_t rows, int hid, int k,
                                      const void* h, int64_t ldh, const void* w2_0,
                                      const void* w2_1, const float* b2_0, const float* b2_1,
                                      void* y_0, void* y_1, int64_t ldy, int64_t P, int64_t Q,
                                      float p0, float p1, const uint32_t* ctr, void* stream) {
  HeadDrop dr = {};
  int rc = head_drop_args("jmt_head_fwd_perm_drop", rows, p0, p1, ctr, &dr);
  if (rc != JMT_OK) return rc;
  return head_fwd_impl("jmt_head_fwd_perm_drop", h_dt, y_dt, rows, hid, k, h, ldh, w2_0, w2_1,
                       b2_0, b2_1, y_0, y_1, ldy, true, P, Q, &dr, stream);
}

// perm: the row map (P, Q) applies to gy (the *_perm entries); dh keeps h's row order
static int head_bwd_impl(const char* name, int h_dt, int gy_dt, int64_t rows, int hid, int k,
                         const void* h, int64_t ldh, const void* w2_0, const void* w2_1,
                         const void* gy_0, const void* gy_1, int64_t ldgy, void* dh, int64_t lddh,
                         float* dw2_0, float* dw2_1, float* db2_0, float* db2_1, float* partials,
                         bool perm, int64_t P, int64_t Q, const HeadDrop* drop, void* stream) {
  int rc = head_check(name, h_dt, rows, hid, k, h, ldh, w2_0, w2_1);
  if (rc != JMT_OK) return rc;
  JMT_CHECK_ARG(gy_dt == JMT_F32 || gy_dt == h_dt, "%s: gy dtype", name);
  JMT_CHECK_ARG(gy_0 && gy_1 && dh && partials && ldgy >= k && lddh % 4 == 0 &&
                    ((uintptr_t)dh & 7) == 0, "%s: bad gradient buffers", name);
  if (rows == 0) return JMT_OK;
  HeadArgs a = {};
  a.h = h; a.ldh = ldh; a.w2[0] = w2_0; a.w2[1] = w2_1;
  a.gy[0] = gy_0; a.gy[1] = gy_1; a.ldgy = ldgy; a.dh = dh; a.lddh = lddh;
  a.partials = partials; a.dw2[0] = dw2_0; a.dw2[1] = dw2_1; a.db2[0] = db2_0; a.db2[1] = db2_1;
  a.rows = rows; a.k = k; a.P = rows; a.Q = 1;
  if (perm && (rc = head_perm_args(name, rows, P, Q, &a)) != JMT_OK) return rc;
  HeadArgsDrop ad = {};
  (HeadArgs&)ad = a;
  if (drop) ad.dr = *drop;
  const int nblk = head_blocks(rows);
  hipStream_t st = as_stream(stream);
#define HBWD2(TH, TG, K, PM)                                                                  \
  {                                                                                           \
    if (drop)                                                                                 \
      hipLaunchKernelGGL((head_bwd_kernel<TH, TG, K, true, PM>), dim3(nblk), dim3(256), 0, st, \
                         ad);                                                                 \
    else                                                                                      \
      hipLaunchKernelGGL((head_bwd_kernel<TH, TG, K, false, PM>), dim3(nblk), dim3(256), 0, st, \
                         a);                                                                  \
  }
#define HBWD1(TH, TG, K)              \
  {                                   \
    if (perm) HBWD2(TH, TG, K, true)  \
    else HBWD2(TH, TG, K, false)      \
  }
#define HBWD(TH, TG)                  \
  {                                   \
    if (k == 1) HBWD1(TH, TG, 1)      \
    else HBWD1(TH, TG, HD_KMAX)       \
  }
  if (h_dt == JMT_BF16) {
    if (gy_dt == JMT_F32) HBWD(__bf16, float) else HBWD(__bf16, __bf16)
  } else {
    if (gy_dt == JMT_F32) HBWD(_Float16, float) else HBWD(_Float16, _Float16)
  }
#undef HBWD
#undef HBWD1
#undef HBWD2
  JMT_LAUNCH_CHECK(name);
  if (dw2_0 || dw2_1 || db2_0 || db2_1) {
    const int SK = k * (HD_HID + 1);
    hipLaunchKernelGGL(head_reduce_kernel, dim3((2 * SK + 3) / 4), dim3(256), 0, st, a, nblk);
    JMT_LAUNCH_CHECK(name);
  }
  return JMT_OK;
}

extern "C" int jmt_head_bwd(int h_dt, int gy_dt, int64_t rows, int hid, int k, const void* h,
                            int64_t ldh, const void* w2_0, const void* w2_1, const void* gy_0,
                            const void* gy_1, int64_t ldgy, void* dh, int64_t lddh, float* dw2_0,
                            float* dw2_1, float* db2_0, float* db2_1, float* partials,
                            void* stream) {
  return head_bwd_impl("jmt_head_bwd", h_dt, gy_dt, rows, hid, k, h, ldh, w2_0, w2_1, gy_0, gy_1,
                       ldgy, dh, lddh, dw2_0, dw2_1, db2_0, db2_1, partials, false, 0, 0, nullptr,
                       stream);
}

extern "C" int jmt_head_bwd_perm(int h_dt, int gy_dt, int64_t rows, int hid, int k, const void* h,
                                 int64_t ldh, const void* w2_0, const void* w2_1,
                                 const void* gy_0, const void* gy_1, int64_t ldgy, void* dh,
                                 int64_t lddh, float* dw2_0, float* dw2_1, float* db2_0,
                                 float* db2_1, float* partials, int64_t P, int64_t Q,
                                 void* stream) {
  return head_bwd_impl("jmt_head_bwd_perm", h_dt, gy_dt, rows, hid, k, h, ldh, w2_0, w2_1, gy_0,
                       gy_1, ldgy, dh, lddh, dw2_0, dw2_1, db2_0, db2_1, partials, true, P, Q,
                       nullptr, stream);
}

extern "C" int jmt_head_bwd_drop(int h_dt, int gy_dt, int64_t rows, int hid, int k, const void* h,
                                 int64_t ldh, const void* w2_0, const void* w2_1,
                                 const void* gy_0, const void* gy_1, int64_t ldgy, void* dh,
                                 int64_t lddh, float* dw2_0, float* dw2_1, float* db2_0,
                                 float* db2_1, float* partials, float p0, float p1,
                                 const uint32_t* ctr, void* stream) {
  HeadDrop dr = {};
  int rc = head_drop_args("jmt_head_bwd_drop", rows, p0, p1, ctr, &dr);
  if (rc != JMT_OK) return rc;
  return head_bwd_impl("jmt_head_bwd_drop", h_dt, gy_dt, rows, hid, k, h, ldh, w2_0, w2_1, gy_0,
                       gy_1, ldgy, dh, lddh, dw2_0, dw2_1, db2_0, db2_1, partials, false, 0, 0, &dr,
                       stream);
}

extern "C" int jmt_head_bwd_perm_drop(int h_dt, int gy_dt, int64_t rows, int hid, int k,
                                      const void* h, int64_t ldh, const void* w2_0,
                                      const void* w2_1, const void* gy_0, const void* gy_1,
                                      int64_t ldgy, void* dh, int64_t lddh, float* dw2_0,
                                      float* dw2_1, float* db2_0, float* db2_1, float* partials,
                                      int64_t P, int64_t Q, float p0, float p1,
                                      const uint32_t* ctr, void* stream) {
  HeadDrop dr = {};
  int rc = head_drop_args("jmt_head_bwd_perm_drop", rows, p0, p1, ctr, &dr);
  if (rc != JMT_OK) return rc;
  return head_bwd_impl("jmt_head_bwd_perm_drop", h_dt, gy_dt, rows, hid, k, h, ldh, w2_0, w2_1,
                       gy_0, gy_1, ldgy, dh, lddh, dw2_0, dw2_1, db2_0, db2_1, partials, true, P, Q,
                       &dr, stream);
}
