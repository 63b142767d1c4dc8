// Optimizer steps that read their scalars from a device-resident state block, so a captured
// hipGraph follows a learning-rate schedule (and Adam's bias corrections) without re-capture:
//   jmt_opt_tick      one thread: step += 1, step_size and bc2_sqrt from lr, beta^step (double)
//   jmt_adam_step     torch.optim.Adam / AMSGrad (L2 weight decay) over the flat fp32 buffers
//   jmt_sgd_step_dev  sgd.hip's update with lr = state[0]
// state (fp32[8], include/jmt.h): lr, step, step_size = lr / (1 - beta1^step),
// bc2_sqrt = sqrt(1 - beta2^step), clip coefficient, gradient norm, max_norm (grad_norm.hip), 1
// reserved.  Both step kernels are pure streams: 16 B per lane per array (8 B for the 16-bit
// shadow), grid-stride, scalar tail for n % 4.
//   jmt_adam_step_clip / jmt_sgd_step_dev_clip  the same kernels with CLIP: every gradient is
//   first multiplied by c = state[4], a product rounded on its own, so that a clipped step on g
//   is bit for bit the unclipped step on fp32(c g)
#include "common.h"

namespace jmt {

__global__ void opt_tick_kernel(float* st, double b1, double b2, const float* amp) {
  if (threadIdx.x != 0) return;
  if (amp && amp[2] != 0.f) return;        // found_inf: torch skips optimizer.step()
  const float step = st[1] + 1.f;          // exact to 2^24, then stays (both corrections are 1)
  st[1] = step;
  const double bc1 = 1.0 - pow(b1, (double)step);
  const double bc2 = 1.0 - pow(b2, (double)step);
  st[2] = (float)((double)st[0] / bc1);
  st[3] = (float)sqrt(bc2);
}

struct AdamK {
  float w1, b2, w2, eps, wd, gs, step_size, bc2_sqrt;   // w1 = 1 - beta1, w2 = 1 - beta2
  float c;                                              // CLIP: state[4]
};

// c g rounded once to fp32, never contracted into the multiply-adds that follow it
__device__ __forceinline__ float clip_mul(float g, float c) {
#pragma clang fp contract(off)
  return __fmul_rn(g, c);
}

template <bool AMS, bool CLIP>
__device__ __forceinline__ float adam_elem(float w, float g, float& m, float& v, float& vm,
                                           const AdamK& k) {
  if constexpr (CLIP) g = clip_mul(g, k.c);
  g *= k.gs;
  if (k.wd != 0.f) g += k.wd * w;
  m = m + k.w1 * (g - m);
  v = k.b2 * v + (k.w2 * g) * g;
  float s = v;
  if constexpr (AMS) {
    vm = fmaxf(vm, v);
    s = vm;
  }
  const float denom = sqrtf(s) / k.bc2_sqrt + k.eps;
  return w - k.step_size * (m / denom);
}

template <typename TS, bool AMS, bool ZG, bool CLIP>
__global__ __launch_bounds__(256) void adam_kernel(int64_t n, float* __restrict__ p,
                                                   float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v,
                                                   float* __restrict__ vmax,
                                                   const float* __restrict__ state, float w1,
                                                   float b2, float w2, float eps, float wd,
                                                   float gs, const float* __restrict__ amp,
                                                   TS* __restrict__ shadow) {
  typedef typename Frag16<TS>::h TS4;
  const bool skip = amp && amp[2] != 0.f;    // found_inf: no update (the grads still zeroed)
  if (skip && !ZG) return;
  const AdamK k = {w1, b2, w2, eps, wd, amp ? amp[1] : gs, state[2], state[3],
                   CLIP ? state[4] : 1.f};
  const int64_t n4 = n >> 2;
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (int64_t i = tid; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    if (skip) {
      ((f32x4*)g)[i] = zero;
      continue;
    }
    f32x4 w = ((const f32x4*)p)[i];
    const f32x4 gg = ((const f32x4*)g)[i];
    f32x4 mm = ((const f32x4*)m)[i];
    f32x4 vv = ((const f32x4*)v)[i];
    f32x4 vm = zero;
    if constexpr (AMS) vm = ((const f32x4*)vmax)[i];
    if constexpr (ZG) ((f32x4*)g)[i] = zero;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float mj = mm[j], vj = vv[j], vmj = vm[j];
      w[j] = adam_elem<AMS, CLIP>(w[j], gg[j], mj, vj, vmj, k);
      mm[j] = mj;
      vv[j] = vj;
      vm[j] = vmj;
    }
    ((f32x4*)p)[i] = w;
    ((f32x4*)m)[i] = mm;
    ((f32x4*)v)[i] = vv;
    if constexpr (AMS) ((f32x4*)vmax)[i] = vm;
    if (shadow) {
      TS4 s;
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] = from_f<TS>(w[j]);
      ((TS4*)shadow)[i] = s;
    }
  }
  const int64_t t = (n4 << 2) + tid;         // scalar tail: the first n % 4 threads of the grid
  if (tid < 4 && t < n) {
    if (skip) {
      g[t] = 0.f;
      return;
    }
    float mj = m[t], vj = v[t], vmj = 0.f;
    if constexpr (AMS) vmj = vmax[t];
    const float gj = g[t];
    if constexpr (ZG) g[t] = 0.f;
    const float nw = adam_elem<AMS, CLIP>(p[t], gj, mj, vj, vmj, k);
    p[t] = nw;
    m[t] = mj;
    v[t] = vj;
    if constexpr (AMS) vmax[t] = vmj;
    if (shadow) shadow[t] = from_f<TS>(nw);
  }
}

// sgd_kernel / sgd_amp_kernel (sgd.hip) element for element, in their arithmetic order
template <bool CLIP>
__device__ __forceinline__ float sgd_elem(float w, float d, float& b, float lr, float mom,
                                          float damp, float wd, int nesterov, int first,
                                          float gs, float c) {
  if constexpr (CLIP) d = clip_mul(d, c);
  d = d * gs;
  if (wd != 0.f) d += wd * w;
  if (mom != 0.f) {
    b = first ? d : b * mom + (1.f - damp) * d;
    d = nesterov ? d + mom * b : b;
  }
  return w - lr * d;
}

template <typename TS, bool ZG, bool CLIP>
__global__ __launch_bounds__(256) void sgd_dev_kernel(int64_t n, float* __restrict__ p,
                                                      float* __restrict__ g,
                                                      float* __restrict__ buf,
                                                      const float* __restrict__ state, float mom,
                                                      float damp, float wd, int nesterov,
                                                      int first_step, float gs_arg,
                                                      const float* __restrict__ amp,
                                                      TS* __restrict__ shadow) {
  typedef typename Frag16<TS>::h TS4;
  const bool skip = amp && amp[2] != 0.f;
  if (skip && !ZG) return;
  const float lr = state[0];
  const float c = CLIP ? state[4] : 1.f;
  const float gs = amp ? amp[1] : gs_arg;
  const int first = amp ? (first_step && amp[4] == 0.f) : first_step;
  const bool has_buf = mom != 0.f;
  const int64_t n4 = n >> 2;
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (int64_t i = tid; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    if (skip) {
      ((f32x4*)g)[i] = zero;
      continue;
    }
    f32x4 w = ((const f32x4*)p)[i];
    const f32x4 gg = ((const f32x4*)g)[i];
    f32x4 bb = zero;
    if (has_buf && !first) bb = ((const f32x4*)buf)[i];
    if constexpr (ZG) ((f32x4*)g)[i] = zero;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float bj = bb[j];
      w[j] = sgd_elem<CLIP>(w[j], gg[j], bj, lr, mom, damp, wd, nesterov, first, gs, c);
      bb[j] = bj;
    }
    ((f32x4*)p)[i] = w;
    if (has_buf) ((f32x4*)buf)[i] = bb;
    if (shadow) {
      TS4 s;
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] = from_f<TS>(w[j]);
      ((TS4*)shadow)[i] = s;
    }
  }
  const int64_t t = (n4 << 2) + tid;
  if (tid < 4 && t < n) {
    if (skip) {
      g[t] = 0.f;
      return;
    }
    float bj = (has_buf && !first) ? buf[t] : 0.f;
    const float gj = g[t];
    if constexpr (ZG) g[t] = 0.f;
    const float nw = sgd_elem<CLIP>(p[t], gj, bj, lr, mom, damp, wd, nesterov, first, gs, c);
    p[t] = nw;
    if (has_buf) buf[t] = bj;
    if (shadow) shadow[t] = from_f<TS>(nw);
  }
}

static inline bool al(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// 256 threads x 4 elements per block, at most 2048 blocks (8 per CU), at least one (the tail)
static inline int stream_blocks(int64_t n) {
  int64_t b = ((n >> 2) + 255) / 256;
  return (int)(b < 1 ? 1 : b > 2048 ? 2048 : b);
}

}  // namespace jmt

using namespace jmt;

extern "C" int jmt_opt_tick(float* state, double beta1, double beta2, const float* amp,
                            void* stream) {
  JMT_CHECK_ARG(state, "jmt_opt_tick: null state");
  JMT_CHECK_ARG(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0,
                "jmt_opt_tick: betas must be in [0, 1)");
  hipLaunchKernelGGL(opt_tick_kernel, dim3(1), dim3(64), 0, as_stream(stream), state, beta1,
                     beta2, amp);
  JMT_LAUNCH_CHECK("jmt_opt_tick");
  return JMT_OK;
}

template <bool CLIP>
static int adam_launch(const char* fn, int64_t n, float* param, float* grad, float* exp_avg,
                       float* exp_avg_sq, float* max_exp_avg_sq, const float* state, double beta1,
                       double beta2, float eps, float weight_decay, float grad_scale,
                       const float* amp, int zero_grad, void* shadow, int shadow_dt,
                       void* stream) {
  JMT_CHECK_ARG(n >= 0, "%s: negative n", fn);
  JMT_CHECK_ARG(param && grad && exp_avg && exp_avg_sq, "%s: null pointer", fn);
  JMT_CHECK_ARG(state, "%s: null state", fn);
  JMT_CHECK_ARG(al(param, 16) && al(grad, 16) && al(exp_avg, 16) && al(exp_avg_sq, 16) &&
                    al(max_exp_avg_sq, 16),
                "%s: param, grad and the moment buffers must be 16-B aligned", fn);
  JMT_CHECK_ARG(!shadow || shadow_dt == JMT_BF16 || shadow_dt == JMT_F16,
                "%s: shadow_dt must be bf16 or f16", fn);
  JMT_CHECK_ARG(al(shadow, 8), "%s: shadow must be 8-B aligned", fn);
  JMT_CHECK_ARG(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0,
                "%s: betas must be in [0, 1)", fn);
  if (n == 0) return JMT_OK;
  const int blocks = stream_blocks(n);
  hipStream_t st = as_stream(stream);
  // torch forms 1 - beta in Python doubles and rounds once
  const float w1 = (float)(1.0 - beta1), b2 = (float)beta2, w2 = (float)(1.0 - beta2);
#define JMT_ADAM(TS, AMS, ZG)                                                                    \
  hipLaunchKernelGGL((adam_kernel<TS, AMS, ZG, CLIP>), dim3(blocks), dim3(256), 0, st, n, param, \
                     grad, exp_avg, exp_avg_sq, max_exp_avg_sq, state, w1, b2, w2, eps,          \
                     weight_decay, grad_scale, amp, (TS*)shadow)
#define JMT_ADAM_T(TS)                                        \
  do {                                                        \
    if (max_exp_avg_sq && zero_grad) JMT_ADAM(TS, true, true); \
    else if (max_exp_avg_sq) JMT_ADAM(TS, true, false);       \
    else if (zero_grad) JMT_ADAM(TS, false, true);            \
    else JMT_ADAM(TS, false, false);                          \
  } while (0)
  if (shadow && shadow_dt == JMT_F16) JMT_ADAM_T(_Float16);
  else JMT_ADAM_T(__bf16);
#undef JMT_ADAM_T
#undef JMT_ADAM
  JMT_LAUNCH_CHECK(fn);
  return JMT_OK;
}

extern "C" int jmt_adam_step(int64_t n, float* param, float* grad, float* exp_avg,
                             float* exp_avg_sq, float* max_exp_avg_sq, const float* state,
                             double beta1, double beta2, float eps, float weight_decay,
                             float grad_scale, const float* amp, int zero_grad, void* shadow,
                             int shadow_dt, void* stream) {
  return adam_launch<false>("jmt_adam_step", n, param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq,
                            state, beta1, beta2, eps, weight_decay, grad_scale, amp, zero_grad,
                            shadow, shadow_dt, stream);
}

extern "C" int jmt_adam_step_clip(int64_t n, float* param, float* grad, float* exp_avg,
                                  float* exp_avg_sq, float* max_exp_avg_sq, const float* state,
                                  double beta1, double beta2, float eps, float weight_decay,
                                  float grad_scale, const float* amp, int zero_grad,
                                  void* shadow, int shadow_dt, void* stream) {
  return adam_launch<true>("jmt_adam_step_clip", n, param, grad, exp_avg, exp_avg_sq,
                           max_exp_avg_sq, state, beta1, beta2, eps, weight_decay, grad_scale,
                           amp, zero_grad, shadow, shadow_dt, stream);
}

template <bool CLIP>
static int sgd_dev_launch(const char* fn, int64_t n, float* param, float* grad,
                          float* momentum_buf, const float* state, float momentum,
                          float dampening, float weight_decay, int nesterov, int first_step,
                          float grad_scale, const float* amp, int zero_grad, void* shadow,
                          int shadow_dt, void* stream) {
  JMT_CHECK_ARG(n >= 0, "%s: negative n", fn);
  JMT_CHECK_ARG(param && grad, "%s: null pointer", fn);
  JMT_CHECK_ARG(state, "%s: null state", fn);
  JMT_CHECK_ARG(momentum == 0.f || momentum_buf, "%s: momentum needs a buffer", fn);
  JMT_CHECK_ARG(al(param, 16) && al(grad, 16) && al(momentum_buf, 16),
                "%s: param, grad and the momentum buffer must be 16-B aligned", fn);
  JMT_CHECK_ARG(!shadow || shadow_dt == JMT_BF16 || shadow_dt == JMT_F16,
                "%s: shadow_dt must be bf16 or f16", fn);
  JMT_CHECK_ARG(al(shadow, 8), "%s: shadow must be 8-B aligned", fn);
  if (n == 0) return JMT_OK;
  const int blocks = stream_blocks(n);
  hipStream_t st = as_stream(stream);
#define JMT_SGDD(TS, ZG)                                                                        \
  hipLaunchKernelGGL((sgd_dev_kernel<TS, ZG, CLIP>), dim3(blocks), dim3(256), 0, st, n, param,   \
                     grad, momentum_buf, state, momentum, dampening, weight_decay, nesterov,     \
                     first_step, grad_scale, amp, (TS*)shadow)
  const bool f16 = shadow && shadow_dt == JMT_F16;
  if (f16 && zero_grad) JMT_SGDD(_Float16, true);
  else if (f16) JMT_SGDD(_Float16, false);
  else if (zero_grad) JMT_SGDD(__bf16, true);
  else JMT_SGDD(__bf16, false);
#undef JMT_SGDD
  JMT_LAUNCH_CHECK(fn);
  return JMT_OK;
}

extern "C" int jmt_sgd_step_dev(int64_t n, float* param, float* grad, float* momentum_buf,
                                const float* state, float momentum, float dampening,
                                float weight_decay, int nesterov, int first_step,
                                float grad_scale, const float* amp, int zero_grad, void* shadow,
                                int shadow_dt, void* stream) {
  return sgd_dev_launch<false>("jmt_sgd_step_dev", n, param, grad, momentum_buf, state, momentum,
                               dampening, weight_decay, nesterov, first_step, grad_scale, amp,
                               zero_grad, shadow, shadow_dt, stream);
}

extern "C" int jmt_sgd_step_dev_clip(int64_t n, float* param, float* grad, float* momentum_buf,
                                     const float* state, float momentum, float dampening,
                                     float weight_decay, int nesterov, int first_step,
                                     float grad_scale, const float* amp, int zero_grad,
                                     void* shadow, int shadow_dt, void* stream) {
  return sgd_dev_launch<true>("jmt_sgd_step_dev_clip", n, param, grad, momentum_buf, state,
                              momentum, dampening, weight_decay, nesterov, first_step,
                              grad_scale, amp, zero_grad, shadow, shadow_dt, stream);
}
