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
//
// The weight regulariser of the same surface (asr_regularize, include/asr.h) follows the optimisers:
// Keras' l2 and the smoothness-in-depth penalty of Haber & Ruthotto over a table of parameter segments,
// two launches whatever the table holds.
#include <math.h>

#include <algorithm>
#include <cmath>

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

// ---- asr_regularize ---------------------------------------------------------------------------
// The work is the flattened sum over segments of count * layers floats, cut into chunks of kRegChunk
// consecutive floats of ONE segment (a segment's last chunk is short), so conv1's 432 floats and a block
// stack's hundreds of thousands load the workgroups alike.  Every workgroup reads the table (at most 256
// entries) into LDS, scans the segments' chunk counts there and walks the chunks blockIdx.x, blockIdx.x +
// gridDim.x, ...; a chunk's segment is found by bisection in the scanned counts.  A thread takes four
// consecutive floats of its chunk: one 16-byte access where the segment's offset, count and layer_stride
// are multiples of four floats (then the four share a layer and are aligned), four scalar ones elsewhere.
//
// R and dR are formed in fp64 from the fp32 parameters (the differences p_l - p_{l-1} cancel; the
// traffic, not the arithmetic, bounds the kernel), so a gradient is rounded twice (dR / grad_scale to
// fp32, then the add) and R once.  Each thread's fp64 sum goes through a fixed LDS tree to one partial per
// workgroup, stored (never added atomically) in the workspace; k_reg_finish sums the partials in a fixed
// order: R has the same bits in every run with the same arguments.
constexpr int kRegThreads = 256, kRegChunk = 4 * kRegThreads, kRegMaxBlocks = 1024;

struct RegSeg {  // asr_reg_segment with the derived chunk range
  long offset, count, stride, total;
  int layers;
  float l2, smooth;
};

__device__ __forceinline__ double reg_block_sum(double v, double* red) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int s = kRegThreads / 2; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  return red[0];
}

// one float p of a layer, prev / next the same float of the layers below / above (where has_prev / has_next):
// its term of R (returned) and, with GRAD, g += dR / grad_scale
template <bool GRAD>
__device__ __forceinline__ double reg_elem(double l2, double sm, bool has_prev, bool has_next, float pf, float prevf,
                                           float nextf, float& g, double inv_gscale) {
  const double p = pf;
  const double dp = has_prev ? p - (double)prevf : 0.0;
  if constexpr (GRAD) {
    const double dn = has_next ? p - (double)nextf : 0.0;
    const double dR = 2.0 * l2 * p + 2.0 * sm * (dp + dn);
    g += (float)(dR * inv_gscale);
  }
  return l2 * p * p + sm * dp * dp;
}

template <bool GRAD>
__global__ __launch_bounds__(kRegThreads) void k_regularize(const asr_reg_segment* __restrict__ segs, int n_segs,
                                                            const float* __restrict__ params,
                                                            float* __restrict__ grads, double inv_gscale, int vec_ok,
                                                            double* __restrict__ partials) {
  __shared__ RegSeg S[ASR_REG_MAX_SEGMENTS];
  __shared__ long ends[ASR_REG_MAX_SEGMENTS];  // inclusive scan of the segments' chunk counts
  __shared__ double red[kRegThreads];
  const int t = threadIdx.x;
  long mine = 0;
  if (t < n_segs) {
    const asr_reg_segment s = segs[t];
    RegSeg r;
    r.offset = s.offset, r.count = s.count, r.stride = s.layer_stride, r.layers = s.layers;
    r.total = s.count * (long)s.layers;
    r.l2 = s.l2, r.smooth = s.smooth;
    S[t] = r;
    // a segment with both coefficients zero adds nothing and leaves its gradients alone
    mine = (s.l2 > 0.f || s.smooth > 0.f) ? (r.total + kRegChunk - 1) / kRegChunk : 0;
  }
  ends[t] = mine;
  __syncthreads();
  for (int d = 1; d < kRegThreads; d <<= 1) {
    const long add = t >= d ? ends[t - d] : 0;
    __syncthreads();
    ends[t] += add;
    __syncthreads();
  }
  const long n_chunks = ends[kRegThreads - 1];
  double acc = 0.0;
  for (long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    int lo = 0, hi = n_segs - 1;  // the first segment whose scanned count exceeds c
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (ends[mid] > c) hi = mid;
      else lo = mid + 1;
    }
    const RegSeg& sg = S[lo];
    const long e = (c - (ends[lo] - (sg.total + kRegChunk - 1) / kRegChunk)) * kRegChunk + 4 * t;
    if (e >= sg.total) continue;
    const bool smooth = sg.smooth > 0.f && sg.layers > 1;  // else no neighbour is read
    const double l2 = sg.l2, sm = sg.smooth;
    // four floats from e on share a layer and are 16-byte aligned
    const bool vec = vec_ok && e + 4 <= sg.total && (sg.offset & 3) == 0 &&
                     (sg.layers == 1 || ((sg.count | sg.stride) & 3) == 0);
    if (vec) {
      const long l = e / sg.count, a = sg.offset + l * sg.stride + (e - l * sg.count);
      const bool hp = smooth && l > 0, hn = smooth && l + 1 < sg.layers;
      const f32x4 p = *reinterpret_cast<const f32x4*>(params + a);
      f32x4 pv = {0.f, 0.f, 0.f, 0.f}, nx = pv, g = pv;
      if (hp) pv = *reinterpret_cast<const f32x4*>(params + a - sg.stride);
      if constexpr (GRAD) {
        if (hn) nx = *reinterpret_cast<const f32x4*>(params + a + sg.stride);
        g = *reinterpret_cast<const f32x4*>(grads + a);
      }
      float gv[4] = {g[0], g[1], g[2], g[3]};
      for (int i = 0; i < 4; ++i) acc += reg_elem<GRAD>(l2, sm, hp, hn, p[i], pv[i], nx[i], gv[i], inv_gscale);
      if constexpr (GRAD) {
        const f32x4 out = {gv[0], gv[1], gv[2], gv[3]};
        *reinterpret_cast<f32x4*>(grads + a) = out;
      }
    } else {
      const long last = e + 4 < sg.total ? e + 4 : sg.total;
      for (long ei = e; ei < last; ++ei) {
        const long l = ei / sg.count, a = sg.offset + l * sg.stride + (ei - l * sg.count);
        const bool hp = smooth && l > 0, hn = smooth && l + 1 < sg.layers;
        const float p = params[a];
        float pv = 0.f, nx = 0.f, g = 0.f;
        if (hp) pv = params[a - sg.stride];
        if constexpr (GRAD) {
          if (hn) nx = params[a + sg.stride];
          g = grads[a];
        }
        acc += reg_elem<GRAD>(l2, sm, hp, hn, p, pv, nx, g, inv_gscale);
        if constexpr (GRAD) grads[a] = g;
      }
    }
  }
  const double sum = reg_block_sum(acc, red);
  if (t == 0) partials[blockIdx.x] = sum;  // every workgroup stores: what the workspace held does not matter
}

__global__ __launch_bounds__(kRegThreads) void k_reg_finish(const double* __restrict__ partials, int n,
                                                            float* __restrict__ loss_inout,
                                                            float* __restrict__ penalty_out) {
  __shared__ double red[kRegThreads];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += kRegThreads) acc += partials[i];
  const double R = reg_block_sum(acc, red);
  if (threadIdx.x == 0) {
    if (penalty_out) *penalty_out = (float)R;
    if (loss_inout) *loss_inout = (float)((double)*loss_inout + R);
  }
}

int reg_blocks(int n_segments, long n_params) {
  const long chunks = (n_params + kRegChunk - 1) / kRegChunk + n_segments;  // segments do not overlap
  return (int)std::max<long>(1, std::min<long>(chunks, kRegMaxBlocks));
}

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

int asr_regularize_check(const asr_reg_segment* host_segments, int n_segments, long n_params) {
  if (n_segments < 0 || n_segments > ASR_REG_MAX_SEGMENTS)
    return fail(ASR_E_ARG, "asr_regularize_check: n_segments = %d (0..%d)", n_segments, ASR_REG_MAX_SEGMENTS);
  if (n_segments == 0) return ASR_OK;
  if (!host_segments) return fail(ASR_E_ARG, "asr_regularize_check: null segment table");
  if (n_params < 0) return fail(ASR_E_ARG, "asr_regularize_check: n_params = %ld", n_params);
  for (int i = 0; i < n_segments; ++i) {
    const asr_reg_segment& s = host_segments[i];
    if (s.count < 1 || s.layers < 1 || s.layer_stride < s.count)
      return fail(ASR_E_ARG, "asr_regularize_check: segment %d: count = %ld (>= 1), layers = %d (>= 1), layer_stride = %ld (>= count)",
                  i, s.count, s.layers, s.layer_stride);
    if (s.offset < 0 || s.offset > n_params || s.count > n_params ||
        (s.layers > 1 && s.layer_stride > (n_params - s.offset - s.count) / (s.layers - 1)) ||
        s.offset + (s.layers - 1) * s.layer_stride + s.count > n_params)
      return fail(ASR_E_ARG, "asr_regularize_check: segment %d (offset %ld, count %ld, layer_stride %ld, layers %d) ends beyond the %ld parameters",
                  i, s.offset, s.count, s.layer_stride, s.layers, n_params);
    if (!(s.l2 >= 0.f) || !(s.smooth >= 0.f) || !std::isfinite(s.l2) || !std::isfinite(s.smooth))
      return fail(ASR_E_ARG, "asr_regularize_check: segment %d: l2 = %g, smooth = %g (finite, >= 0)", i, (double)s.l2,
                  (double)s.smooth);
  }
  // two segments overlap when a layer of one shares floats with a layer of the other.  Layers of segment i
  // are [o_i + l * st_i, + c_i); only the layers of j that start in (lo - c_j, hi) can meet layer [lo, hi).
  for (int i = 0; i < n_segments; ++i) {
    const asr_reg_segment& a = host_segments[i];
    for (int j = i + 1; j < n_segments; ++j) {
      const asr_reg_segment& b = host_segments[j];
      const long a_end = a.offset + (a.layers - 1) * a.layer_stride + a.count;
      const long b_end = b.offset + (b.layers - 1) * b.layer_stride + b.count;
      if (a_end <= b.offset || b_end <= a.offset) continue;
      // walk the layers of the segment with fewer of them; for each, the one candidate window in the other
      const asr_reg_segment& f = a.layers <= b.layers ? a : b;
      const asr_reg_segment& m = a.layers <= b.layers ? b : a;
      for (int l = 0; l < f.layers; ++l) {
        const long lo = f.offset + l * f.layer_stride, hi = lo + f.count;
        // layers k of m with m.offset + k * st < hi and m.offset + k * st + m.count > lo
        long k0 = lo - m.count - m.offset;  // k * st > k0
        k0 = k0 < 0 ? 0 : k0 / m.layer_stride + 1;
        const long k1 = hi - 1 - m.offset;  // k * st <= k1
        if (k1 < 0) continue;
        if (k0 <= std::min<long>(k1 / m.layer_stride, m.layers - 1))
          return fail(ASR_E_ARG, "asr_regularize_check: segments %d and %d overlap", i, j);
      }
    }
  }
  return ASR_OK;
}

size_t asr_regularize_workspace_bytes(int n_segments, long n_params) {
  if (n_segments <= 0 || n_segments > ASR_REG_MAX_SEGMENTS || n_params < 0) return 0;
  return (size_t)reg_blocks(n_segments, n_params) * sizeof(double);
}

int asr_regularize(const asr_reg_segment* segments, int n_segments, const float* params, float* grads,
                   float grad_scale, float* loss_inout, float* penalty_out, void* ws, size_t ws_bytes,
                   asr_stream_t stream) {
  if (n_segments < 0 || n_segments > ASR_REG_MAX_SEGMENTS)
    return fail(ASR_E_ARG, "asr_regularize: n_segments = %d (0..%d)", n_segments, ASR_REG_MAX_SEGMENTS);
  if (n_segments == 0) return ASR_OK;
  if (!segments || !params) return fail(ASR_E_ARG, "asr_regularize: null pointer");
  if (grads && !(std::isfinite(grad_scale) && grad_scale > 0.f))
    return fail(ASR_E_ARG, "asr_regularize: grad_scale = %g (finite, > 0)", (double)grad_scale);
  if (!ws || ws_bytes < sizeof(double) || ((uintptr_t)ws & 7))
    return fail(ASR_E_WORKSPACE, "asr_regularize: workspace of %zu bytes (asr_regularize_workspace_bytes; 8-byte aligned)",
                ws_bytes);
  // one workgroup per partial the workspace holds: the chunks are walked with that stride
  const int blocks = (int)std::min<size_t>(ws_bytes / sizeof(double), kRegMaxBlocks);
  const int vec_ok = (((uintptr_t)params | (uintptr_t)grads) & 15) == 0;
  double* partials = (double*)ws;
  hipStream_t s = (hipStream_t)stream;
  if (grads)
    hipLaunchKernelGGL(k_regularize<true>, dim3(blocks), dim3(kRegThreads), 0, s, segments, n_segments, params, grads,
                       1.0 / (double)grad_scale, vec_ok, partials);
  else
    hipLaunchKernelGGL(k_regularize<false>, dim3(blocks), dim3(kRegThreads), 0, s, segments, n_segments, params,
                       (float*)nullptr, 1.0, vec_ok, partials);
  ASR_LAUNCH_CHECK("k_regularize");
  if (loss_inout || penalty_out) {
    hipLaunchKernelGGL(k_reg_finish, dim3(1), dim3(kRegThreads), 0, s, (const double*)partials, blocks, loss_inout,
                       penalty_out);
    ASR_LAUNCH_CHECK("k_reg_finish");
  }
  return ASR_OK;
}

}  // extern "C"
