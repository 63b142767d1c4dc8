// Gradient-norm clipping for the fused optimizers (torch.nn.utils.clip_grad_norm_, L2) without a
// second read-modify-write pass: a read-only pass over the flat fp32 gradient buffer produces the
// norm and the clip coefficient in the optimizer's device state block, and the step kernels
// (adam.hip, CLIP) multiply each gradient by it as they read it.
//   grad_norm_kernel       one double partial per chunk of GN_CHUNK elements
//   grad_norm_fold_kernel  one block: per-segment sums, their sum, norm / coefficient -> state
// The buffer is cut into segments (the parameters of _FlatOptimizer; one segment [0, n) without a
// table) and every segment into chunks of GN_CHUNK elements counted from the segment's start, so
// no chunk straddles two segments.  Squares are accumulated in double (fp32 squares of 1e30
// overflow): per thread, wave, block.  Every partial has one writer and the fold adds them in one
// fixed order (lane-strided into four accumulators, then the xor tree of wave_sum_d), the total
// being the fixed-order sum of the segment sums: no floating-point atomics, so the result is
// bitwise reproducible from run to run and between an eager launch and a graph replay.
#include "common.h"

namespace jmt {

constexpr int GN_THREADS = 256;
constexpr int GN_LOADS = 4;                                // 16-B loads in flight per lane
constexpr int GN_CHUNK = GN_THREADS * GN_LOADS * 4;        // 4096 elements (16 KB) per block trip
constexpr int GN_BLOCKS_PER_CU = 8;                        // the grid: this many per CU, no more
constexpr int GN_FOLD_THREADS = 1024;
constexpr int GN_MAX_SEG = 2048;                           // prefix table, segment sums in LDS
constexpr int GN_STAGE = 4096;                             // partials the fold stages through LDS

// [b, e) of segment s, clamped into [0, n] so that a bad table can never index past the buffer
__device__ __forceinline__ void seg_bounds(const int64_t* seg_off, int nseg, int64_t n, int s,
                                           int64_t& b, int64_t& e) {
  if (nseg == 0) {
    b = 0;
    e = n;
    return;
  }
  b = seg_off[s];
  e = seg_off[s + 1];
  JMT_DCHECK(b >= 0 && b <= e && e <= n);
  b = b < 0 ? 0 : b > n ? n : b;
  e = e < b ? b : e > n ? n : e;
}

// coff[s] = chunks of the segments before s (coff[S] = all of them), the same in every block of
// either kernel.  NT threads; S <= GN_MAX_SEG.
template <int NT>
__device__ __forceinline__ void chunk_prefix(const int64_t* seg_off, int nseg, int64_t n, int S,
                                             int* coff, int* wtot) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int per = (S + NT - 1) / NT;
  int loc = 0;
  for (int k = 0; k < per; ++k) {
    const int s = t * per + k;
    if (s < S) {
      int64_t b, e;
      seg_bounds(seg_off, nseg, n, s, b, e);
      loc += (int)((e - b + GN_CHUNK - 1) / GN_CHUNK);
      coff[s + 1] = loc;
    }
  }
  int inc = loc;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(inc, o, 64);
    if (lane >= o) inc += u;
  }
  if (lane == 63) wtot[w] = inc;
  __syncthreads();
  int base = inc - loc;
  for (int i = 0; i < w; ++i) base += wtot[i];
  for (int k = 0; k < per; ++k) {
    const int s = t * per + k;
    if (s < S) coff[s + 1] += base;
  }
  if (t == 0) coff[0] = 0;
  __syncthreads();
}

__device__ __forceinline__ double sq_acc(double acc, float x) {
  const double d = (double)x;
  return fma(d, d, acc);
}

__global__ __launch_bounds__(GN_THREADS) void grad_norm_kernel(int64_t n,
                                                               const float* __restrict__ g,
                                                               const int64_t* __restrict__ seg_off,
                                                               int nseg, double* __restrict__ part,
                                                               int npart) {
  __shared__ int coff[GN_MAX_SEG + 1];
  __shared__ int wtot[GN_THREADS / 64];
  __shared__ double red[GN_THREADS / 64];
  const int S = nseg > 0 ? nseg : 1;
  chunk_prefix<GN_THREADS>(seg_off, nseg, n, S, coff, wtot);
  const int total = coff[S] < npart ? coff[S] : npart;
  const int tid = threadIdx.x;
  for (int v = blockIdx.x; v < total; v += gridDim.x) {
    int lo = 0, hi = S;                      // the last segment that starts at or before chunk v
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (coff[mid] <= v) lo = mid;
      else hi = mid;
    }
    int64_t b, e;
    seg_bounds(seg_off, nseg, n, lo, b, e);
    const int64_t beg = b + (int64_t)(v - coff[lo]) * GN_CHUNK;
    const int64_t end = beg + GN_CHUNK < e ? beg + GN_CHUNK : e;
    JMT_DCHECK(beg >= 0 && beg < end && end <= n && v < npart);
    double acc = 0.0;
    if ((beg & 3) == 0) {
      const int64_t nv = (end - beg) >> 2;
      const f32x4* gv = (const f32x4*)(g + beg);
      f32x4 x[GN_LOADS];
#pragma unroll
      for (int k = 0; k < GN_LOADS; ++k) {
        const int i = tid + k * GN_THREADS;
        x[k] = i < nv ? gv[i] : f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int k = 0; k < GN_LOADS; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = sq_acc(acc, x[k][j]);
      const int64_t t = beg + (nv << 2) + tid;       // scalar tail: (end - beg) % 4 elements
      if (tid < 4 && t < end) acc = sq_acc(acc, g[t]);
    } else {                                          // a segment that does not start on 16 B
      for (int64_t i = beg + tid; i < end; i += GN_THREADS) acc = sq_acc(acc, g[i]);
    }
    acc = wave_sum_d(acc);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) part[v] = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
  }
}

__global__ __launch_bounds__(GN_FOLD_THREADS) void grad_norm_fold_kernel(
    int64_t n, const int64_t* __restrict__ seg_off, int nseg, const double* __restrict__ part,
    int npart, float* __restrict__ seg_norm, float* __restrict__ state, float gs_arg,
    const float* __restrict__ amp) {
  __shared__ int coff[GN_MAX_SEG + 1];
  __shared__ int wtot[GN_FOLD_THREADS / 64];
  __shared__ double ssum[GN_MAX_SEG];
  __shared__ double stage[GN_STAGE];
  const int S = nseg > 0 ? nseg : 1;
  chunk_prefix<GN_FOLD_THREADS>(seg_off, nseg, n, S, coff, wtot);
  const double gs = (double)(amp ? amp[1] : gs_arg);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  // up to GN_STAGE partials (16.7 M elements) come in with one round of coalesced loads, all in
  // flight at once: the waves below would otherwise each wait out a load per segment.  The adds
  // and their order are the same from either source.
  const int total = coff[S] < npart ? coff[S] : npart;
  const bool staged = total <= GN_STAGE;
  if (staged) {
    for (int c = threadIdx.x; c < total; c += GN_FOLD_THREADS) stage[c] = part[c];
    __syncthreads();
  }
  auto ld = [&](int c) {
    JMT_DCHECK(c >= 0 && c < npart);
    return staged ? stage[c] : part[c];
  };
  for (int s = w; s < S; s += GN_FOLD_THREADS / 64) {
    const int c1 = coff[s + 1] < total ? coff[s + 1] : total;
    // lane l adds partials l, l + 64, ... of the segment into 4 rotating accumulators
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int c = coff[s] + lane;
    for (; c + 192 < c1; c += 256) {
      a0 += ld(c);
      a1 += ld(c + 64);
      a2 += ld(c + 128);
      a3 += ld(c + 192);
    }
    for (; c < c1; c += 64) a0 += ld(c);
    double a = wave_sum_d((a0 + a1) + (a2 + a3));
    if (lane == 0) {
      ssum[s] = a;
      if (nseg > 0) seg_norm[s] = (float)(sqrt(a) * gs);
    }
  }
  __syncthreads();
  if (w != 0) return;
  double tot = 0.0;
  for (int s = lane; s < S; s += 64) tot += ssum[s];
  tot = wave_sum_d(tot);
  if (lane != 0) return;
  const double norm = sqrt(tot) * gs;               // of the unscaled gradient
  const double mx = (double)state[6];
  // torch.nn.utils.clip_grad_norm_(error_if_nonfinite=False): clamp(max / (norm + 1e-6), max=1)
  // keeps a NaN (fmin would answer 1) and turns an infinite norm into 0
  double c = mx / (norm + 1e-6);
  if (c > 1.0) c = 1.0;
  state[4] = (float)c;
  state[5] = (float)norm;
}

static inline bool al(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// chunk partials the grid may write: every segment ends with at most one partial chunk
static inline int64_t gn_parts(int64_t n, int nseg) {
  return n / GN_CHUNK + (nseg > 0 ? nseg : 1);
}

// the kernels count chunks in int: no table, however wrong, may make the count overflow
static inline bool gn_size_ok(int64_t n, int nseg) {
  return n / GN_CHUNK < ((int64_t)1 << 30) / (nseg > 0 ? nseg : 1);
}

static int gn_cus() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v < 8)
      v = 256;
    cus = v;
  }
  return cus;
}

}  // namespace jmt

using namespace jmt;

extern "C" int64_t jmt_grad_norm_scratch(int64_t n, int nseg) {
  if (n < 0 || nseg < 0 || nseg > GN_MAX_SEG || !gn_size_ok(n, nseg)) return -1;
  return gn_parts(n, nseg) * (int64_t)sizeof(double);
}

extern "C" int jmt_grad_norm(int64_t n, const float* grad, float* state, double* scratch,
                             int64_t scratch_bytes, const int64_t* seg_off, int nseg,
                             float* seg_norm, float grad_scale, const float* amp, void* stream) {
  JMT_CHECK_ARG(n >= 0, "jmt_grad_norm: negative n");
  JMT_CHECK_ARG(grad, "jmt_grad_norm: null grad");
  JMT_CHECK_ARG(state, "jmt_grad_norm: null state");
  JMT_CHECK_ARG(scratch, "jmt_grad_norm: null scratch");
  JMT_CHECK_ARG(al(grad, 16) && al(scratch, 8),
                "jmt_grad_norm: grad must be 16-B aligned, scratch 8-B aligned");
  JMT_CHECK_ARG(nseg >= 0, "jmt_grad_norm: negative nseg");
  JMT_CHECK_ARG(nseg <= GN_MAX_SEG, "jmt_grad_norm: nseg beyond %d segments", GN_MAX_SEG);
  JMT_CHECK_ARG(gn_size_ok(n, nseg),
                "jmt_grad_norm: n / %d chunks times nseg must stay under 2^30", GN_CHUNK);
  JMT_CHECK_ARG(nseg == 0 || seg_off, "jmt_grad_norm: null seg_off with nseg > 0");
  JMT_CHECK_ARG(nseg == 0 || seg_norm, "jmt_grad_norm: null seg_norm with nseg > 0");
  const int64_t parts = gn_parts(n, nseg);
  JMT_CHECK_ARG(scratch_bytes >= parts * (int64_t)sizeof(double),
                "jmt_grad_norm: scratch of %lld bytes, jmt_grad_norm_scratch asks for %lld",
                (long long)scratch_bytes, (long long)(parts * (int64_t)sizeof(double)));
  const int64_t cap = (int64_t)gn_cus() * GN_BLOCKS_PER_CU;
  const int blocks = (int)(parts < cap ? parts : cap);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(grad_norm_kernel, dim3(blocks), dim3(GN_THREADS), 0, st, n, grad, seg_off,
                     nseg, scratch, (int)parts);
  JMT_LAUNCH_CHECK("jmt_grad_norm");
  hipLaunchKernelGGL(grad_norm_fold_kernel, dim3(1), dim3(GN_FOLD_THREADS), 0, st, n, seg_off,
                     nseg, (const double*)scratch, (int)parts, seg_norm, state, grad_scale, amp);
  JMT_LAUNCH_CHECK("jmt_grad_norm");
  return JMT_OK;
}
