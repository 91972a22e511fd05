// Device optimisers of the Keras training surface (asr_optimizer_update, include/asr.h): SGD with
// momentum / Nesterov, Adam with AMSGrad, RMSprop, in the Keras 2.1.6-tf forms (the ones TF 1.12's
// tf.keras.optimizers ships), and the executors' plain Adam step (asr_adam_update, k_adam).  One launch
// per update whatever the optimiser, k_adam's grid-stride shape, fp32 throughout, no host synchronisation.  The state is `slots` buffers of n floats,
// back to back, owned and zero-initialised by the caller.
//
// Every element is read and written once per buffer it touches and nothing is reused, so the kernel
// is bound by HBM traffic: (2 + 2 * slots) * 4 bytes per element (AMSGrad: 32 B, SGD / RMSprop: 16 B).
//
// Adam without AMSGrad computes k_adam's expressions in k_adam's order, so the two give the same
// bits on the same inputs (tests/test_gpu_keras_api.py compares them).
#include <math.h>

#include <algorithm>

#include "asr_common.h"

namespace asr {

__global__ void k_adam(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                       float* __restrict__ v, long n, float lr_t, float b1, float b2, float eps, float gscale) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float gi = g[i] * gscale;
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    p[i] -= lr_t * mi / (sqrtf(vi) + eps);
  }
}

namespace {

struct OptParams {
  float* p;
  const float* g;
  float* s0;  // SGD: m;  Adam: m;  RMSprop: a
  float* s1;  // Adam: v
  float* s2;  // Adam + AMSGRAD: v-hat
  long n;
  float lr;  // Adam: lr_t (the bias correction is folded in on the host)
  float a, b, eps, gscale;
};

template <int KIND, int FLAGS>
__global__ void k_optimizer(const OptParams P) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < P.n; i += (long)gridDim.x * blockDim.x) {
    // every product and sum rounded on its own, as k_adam compiles (its m and v products are packed
    // multiplies, never fused with the sums): left to the compiler, this kernel's m became an fma and
    // differed from k_adam's in the last bit
#pragma clang fp contract(off)
    const float gi = P.g[i] * P.gscale;
    if constexpr (KIND == ASR_OPT_SGD) {
      const float vi = P.a * P.s0[i] - P.lr * gi;
      P.s0[i] = vi;
      if constexpr ((FLAGS & ASR_OPT_NESTEROV) != 0) P.p[i] = P.p[i] + P.a * vi - P.lr * gi;
      else P.p[i] = P.p[i] + vi;
    } else if constexpr (KIND == ASR_OPT_ADAM) {
      const float mi = P.a * P.s0[i] + (1.f - P.a) * gi;
      const float vi = P.b * P.s1[i] + (1.f - P.b) * gi * gi;
      P.s0[i] = mi;
      P.s1[i] = vi;
      if constexpr ((FLAGS & ASR_OPT_AMSGRAD) != 0) {
        const float vh = fmaxf(P.s2[i], vi);
        P.s2[i] = vh;
        P.p[i] -= P.lr * mi / (sqrtf(vh) + P.eps);
      } else {
        P.p[i] -= P.lr * mi / (sqrtf(vi) + P.eps);
      }
    } else {  // ASR_OPT_RMSPROP
      const float ai = P.a * P.s0[i] + (1.f - P.a) * gi * gi;
      P.s0[i] = ai;
      P.p[i] -= P.lr * gi / (sqrtf(ai) + P.eps);
    }
  }
}

// the flags a kind takes
int kind_flags(int kind) {
  return kind == ASR_OPT_SGD ? ASR_OPT_NESTEROV : kind == ASR_OPT_ADAM ? ASR_OPT_AMSGRAD : 0;
}

bool kind_known(int kind) { return kind == ASR_OPT_SGD || kind == ASR_OPT_ADAM || kind == ASR_OPT_RMSPROP; }

}  // namespace
}  // namespace asr

using namespace asr;

extern "C" {

int asr_adam_update(float* params, const float* grads, float* m, float* v, long n, float lr, float beta1, float beta2,
                    float eps, long step, float grad_scale, asr_stream_t stream) {
  if (!params || !grads || !m || !v || n < 0 || step < 1) return fail(ASR_E_ARG, "asr_adam_update: bad arguments");
  const double lr_t = (double)lr * sqrt(1.0 - pow((double)beta2, (double)step)) / (1.0 - pow((double)beta1, (double)step));
  const unsigned grid = (unsigned)std::max<long>(1, std::min<long>((n + 255) / 256, 4096));
  hipLaunchKernelGGL(k_adam, dim3(grid), dim3(256), 0, (hipStream_t)stream, params, grads, m, v, n, (float)lr_t,
                     beta1, beta2, eps, grad_scale);
  ASR_LAUNCH_CHECK("k_adam");
  return ASR_OK;
}

int asr_optimizer_slots(int kind, int flags) {
  if (!kind_known(kind) || (flags & ~kind_flags(kind))) return -1;
  if (kind == ASR_OPT_ADAM) return (flags & ASR_OPT_AMSGRAD) ? 3 : 2;
  return 1;
}

int asr_optimizer_update(const asr_optimizer_config* cfg, float* params, const float* grads, float* state, long n,
                         asr_stream_t stream) {
  if (!cfg || !params || !grads || !state) return fail(ASR_E_ARG, "asr_optimizer_update: null pointer");
  if (n < 0 || cfg->step < 1)
    return fail(ASR_E_ARG, "asr_optimizer_update: n = %ld (>= 0), step = %ld (>= 1)", n, cfg->step);
  if (!kind_known(cfg->kind)) return fail(ASR_E_ARG, "asr_optimizer_update: unknown kind %d", cfg->kind);
  if (cfg->flags & ~kind_flags(cfg->kind))
    return fail(ASR_E_ARG, "asr_optimizer_update: flags %d do not belong to kind %d", cfg->flags, cfg->kind);
  if (n == 0) return ASR_OK;
  OptParams P;
  P.p = params;
  P.g = grads;
  P.s0 = state;
  P.s1 = state + n;
  P.s2 = state + 2 * n;
  P.n = n;
  P.lr = cfg->lr;
  P.a = cfg->a;
  P.b = cfg->b;
  P.eps = cfg->eps;
  P.gscale = cfg->grad_scale;
  if (cfg->kind == ASR_OPT_ADAM)  // as asr_adam_update: the bias correction in double, rounded once
    P.lr = (float)((double)cfg->lr * sqrt(1.0 - pow((double)cfg->b, (double)cfg->step)) /
                   (1.0 - pow((double)cfg->a, (double)cfg->step)));
  const dim3 grid((unsigned)std::max<long>(1, std::min<long>((n + 255) / 256, 4096))), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (cfg->kind == ASR_OPT_SGD) {
    if (cfg->flags & ASR_OPT_NESTEROV) hipLaunchKernelGGL((k_optimizer<ASR_OPT_SGD, ASR_OPT_NESTEROV>), grid, block, 0, s, P);
    else hipLaunchKernelGGL((k_optimizer<ASR_OPT_SGD, 0>), grid, block, 0, s, P);
  } else if (cfg->kind == ASR_OPT_ADAM) {
    if (cfg->flags & ASR_OPT_AMSGRAD) hipLaunchKernelGGL((k_optimizer<ASR_OPT_ADAM, ASR_OPT_AMSGRAD>), grid, block, 0, s, P);
    else hipLaunchKernelGGL((k_optimizer<ASR_OPT_ADAM, 0>), grid, block, 0, s, P);
  } else {
    hipLaunchKernelGGL((k_optimizer<ASR_OPT_RMSPROP, 0>), grid, block, 0, s, P);
  }
  ASR_LAUNCH_CHECK("k_optimizer");
  return ASR_OK;
}

}  // extern "C"
