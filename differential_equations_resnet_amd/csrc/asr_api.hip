// C ABI entry points (include/asr.h): conv forward/backward dispatch and the
// native single-block-network executor (stem, L Euler blocks, head, loss,
// backward, Adam).
//
// Reference call stack replaced: Training.train's
// sess.run(train_step) (training/training.py:578-597) over the graph built by
// get_single_block_resnet_build_function (models/tfkeras_resnets.py:547-602)
// and Training._build_optimizer (training/training.py:283-304).
#include <math.h>

#include <vector>

#include "asr_common.h"
#include "asr_internal.h"

namespace asr {
static bool mfma_supported(int C, int W) { return (C == 16 || C == 32 || C == 64) && W == 32; }

static int check_shape(int N, int H, int W, int C) {
  if (N < 1 || H < 1 || W < 1 || C < 1) return fail(ASR_E_ARG, "bad shape N=%d H=%d W=%d C=%d", N, H, W, C);
  if ((long)N * H * W * C > (1L << 40)) return fail(ASR_E_ARG, "shape too large");
  return ASR_OK;
}

// the shapes of the bf16 3 x 3 kernels (MFMA at W = 32, the any-width convb_* elsewhere: W = 16 / 8, and the
// column-strip kernels at W >= 48)
static int check_bf16_conv(int C, int W) {
  if (!mfma_supported(C, W) && !convb_supported(W, C))
    return fail(ASR_E_UNSUPPORTED, "bf16 conv needs C in {16,32,64,128,256} and W == 8 or W %% 16 == 0 (C=%d W=%d)", C,
                W);
  return ASR_OK;
}

static int check_kernel_size(const char* fn, int kernel_size) {
  if (kernel_size < 1 || kernel_size > 15 || !(kernel_size & 1))
    return fail(ASR_E_ARG, "%s: kernel_size %d (odd, 1..15)", fn, kernel_size);
  return ASR_OK;
}

// ---------------------------------------------------------------------------
// conv backward workspace
// ---------------------------------------------------------------------------
// `stages` = conv applications whose weight-gradient slabs are reduced
// together (1: Euler block / bare conv, 2: RK2 midpoint block).  RK2 also
// needs the inter-stage gradient g.
struct BwdWs {
  size_t dz, slabs, red, g, total;
};

static BwdWs bwd_ws_layout(int N, int H, int W, int C, int dtype, int stages = 1, int K = 3, int slab_rows = -1) {
  BwdWs b{};
  const long E = (long)K * K * C * C;
  const long P = (long)N * H * W * C;
  // bf16 at C in {128, 256} (k_wgradbw): the rows its grid writes (a row is 0.6 / 2.4 MB), not the 512-row maximum
  const bool wide = dtype == ASR_BF16 && K == 3 && C > 64 && convb_supported(W, C);
  const int nsl = slab_rows >= 0 ? slab_rows : (wide ? bf16_block_slab_rows(N, H, W, C) : kMaxBlockSlabs) * stages;
  WsCursor c;
  b.dz = c.take(dtype == ASR_F32 ? (size_t)P * 4 : 0);
  b.slabs = c.take((size_t)nsl * (E + C) * 4);
  b.red = c.take(reduce_ws_bytes(nsl, E + C));
  b.g = c.take(stages > 1 ? (size_t)P * (dtype == ASR_BF16 ? 2 : 4) : 0);
  b.total = c.off;
  return b;
}

// The stem's backward workspace (the network executor's bwdws area, shared with
// the blocks' BwdWs): dz1 in fp32, conv1's weight-gradient slabs, reduce_and_project's rows.
struct StemWs {
  size_t dz, slabs, red, total;
};

static StemWs stem_ws_layout(long P, int Cin, int C, int K = 3) {
  StemWs w{};
  const long ES1 = (long)K * K * Cin * C + C;
  WsCursor c;
  w.dz = c.take((size_t)P * 4);
  w.slabs = c.take((size_t)kMaxBlockSlabs * ES1 * 4);
  w.red = c.take(reduce_ws_bytes(kMaxBlockSlabs, ES1));
  w.total = c.off;
  return w;
}

// One conv application's backward: dx = [dy] + extra + A^T dz and the
// weight-gradient slabs (written at `slabs`, count in *nsl).
//   EULER: dz = h*dy*mask; CONV: dz = dy.  skip_dy drops the +dy residual of
//   EULER (the second RK2 stage); extra (nullable) is added to dx (the first
//   RK2 stage adds the step's outer dy).
static int block_backward(int mode, const void* dy, const void* x, const uint8_t* mask, const void* w, float h,
                          float gamma, int N, int H, int W, int C, int dtype, void* dx, bool need_w, const void* extra,
                          bool skip_dy, float* slabs, float* dz_scratch, int* nsl, hipStream_t s, bool relu_dx = false,
                          int* relu_done = nullptr, const float* fold_slabs = nullptr, int fold_P = 0,
                          float* fold_grp = nullptr, int* fold_done = nullptr, bool accum_slabs = false) {
  *nsl = 0;
  if (relu_done) *relu_done = 0;
  if (fold_done) *fold_done = 0;
  if (dtype == ASR_BF16) {
    if (!dx && !need_w) return ASR_OK;
    if (!mfma_supported(C, W)) {  // W != 32: the any-width bf16 kernels (plain Euler blocks and bare convs)
      if (extra || skip_dy || relu_dx || fold_slabs || accum_slabs || !convb_supported(W, C))
        return fail(ASR_E_UNSUPPORTED, "bf16 backward at C=%d W=%d: plain Euler blocks and convs only", C, W);
      return convb_backward(dy, mask, x, w, h, 2.f * gamma, N, H, W, C, dx, need_w, slabs, nsl, s,
                            mode == ASR_MODE_CONV);
    }
    const int cm = (mode == ASR_MODE_EULER) ? 2 : 3;  // BWD_EULER / BWD_CONV
    return block_bwd_mfma(cm, dy, x, mask, w, h, 2.f * gamma, N, H, W, C, dx, slabs, nsl, extra, skip_dy ? 1 : 0, s,
                          relu_dx ? 1 : 0, relu_done, fold_slabs, fold_P, fold_grp, fold_done, accum_slabs ? 1 : 0);
  }
  if (accum_slabs) return fail(ASR_E_UNSUPPORTED, "slab accumulation: bf16 path only");
  const bool euler = mode == ASR_MODE_EULER;
  if (euler && conv32_fused_bwd_supported(W, C))  // fp32 MFMA: dz formed while staging, no dz pass
    return conv32_bwd_fused((const float*)dy, mask, h, (const float*)x, (const float*)w, 2.f * gamma,
                            (const float*)extra, skip_dy, N, H, W, C, (float*)dx, need_w, slabs, nsl, s);
  ASR_TRY(make_dz(euler ? F_EULER : F_CONV, dy, mask, nullptr, h, N, H, W, C, 0, dz_scratch, s));
  if (dx)
    ASR_TRY(conv_f32((euler && !skip_dy) ? B_EULER : B_CONV, dz_scratch, dx, nullptr, (const float*)w, nullptr, h,
                     2.f * gamma, (const float*)dy, N, H, W, C, C, 0, s, (const float*)extra));
  if (need_w) ASR_TRY(wgrad_f32(x, 0, dz_scratch, N, H, W, C, C, slabs, nsl, s));
  return ASR_OK;
}

// One fp32 Euler block's backward that leaves its weight-gradient slabs (*nsl rows of 9C^2 + C
// floats) at `slabs` for the caller to reduce together with other blocks' (reduce_slab_layers).
int conv_backward_keep_slabs(const void* dy, const void* x, const uint8_t* mask, const void* w, float h, float gamma,
                             int N, int H, int W, int C, void* dx, void* ws, float* slabs, int* nsl, hipStream_t s) {
  const BwdWs L = bwd_ws_layout(N, H, W, C, ASR_F32);
  return block_backward(ASR_MODE_EULER, dy, x, mask, w, h, gamma, N, H, W, C, ASR_F32, dx, true, nullptr, false, slabs,
                        (float*)((unsigned char*)ws + L.dz), nsl, s);
}

// RK2 (explicit midpoint) block, BASELINE config 5 (an extension: the
// reference integrates with forward Euler only, tfkeras_resnets.py:69-92):
//   xm = x + (h/2) relu(A x + b)          (mask1 = [A x + b > 0])
//   y  = x + h relu(A xm + b)             (mask2 = [A xm + b > 0])
// Both stages run the Euler kernels; the second takes its residual from x.
static int rk2_forward_impl(const void* x, void* xmid, void* y, uint8_t* mask1, uint8_t* mask2, const void* w,
                            const float* bias, float h, int N, int H, int W, int C, int dtype, hipStream_t s) {
  if (dtype == ASR_BF16) {
    ASR_TRY(block_fwd_mfma(0, x, nullptr, xmid, mask1, w, bias, 0.5f * h, N, H, W, C, s));
    return block_fwd_mfma(0, xmid, x, y, mask2, w, bias, h, N, H, W, C, s);
  }
  ASR_TRY(conv_f32(F_EULER, x, xmid, mask1, (const float*)w, bias, 0.5f * h, 0.f, nullptr, N, H, W, C, C, 0, s));
  return conv_f32(F_EULER, xmid, y, mask2, (const float*)w, bias, h, 0.f, nullptr, N, H, W, C, C, 0, s,
                  (const float*)x);
}

// Backward of rk2_forward_impl: with dz2 = h dy mask2 and g = A^T dz2 (the
// gradient reaching xm), dz1 = (h/2) g mask1 and dx = dy + g + A^T dz1;
// dW collects x (x) dz1 + xm (x) dz2.  bf16: both stages run on the same
// persistent grid, so the first stage adds its slabs onto the second's (one
// slab set per block, *nsl = the grid); fp32: two slab sets, reduced together.
// fold_* as block_bwd_mfma (carried by the second stage's kernel).
static int rk2_backward_slabs(const void* dy, const void* x, const void* xmid, const uint8_t* mask1,
                              const uint8_t* mask2, const void* w, float h, float gamma, int N, int H, int W, int C,
                              int dtype, void* dx, void* g, bool need_w, float* slabs, float* dz_scratch, int* nsl,
                              hipStream_t s, const float* fold_slabs = nullptr, int fold_P = 0,
                              float* fold_grp = nullptr, int* fold_done = nullptr) {
  int n2 = 0, n1 = 0;
  // bf16: both stages run on the same persistent grid (block_bwd_grid of the
  // same shape), so the first stage can add onto the second's slabs
  const bool one_set = dtype == ASR_BF16;
  ASR_TRY(block_backward(ASR_MODE_EULER, dy, xmid, mask2, w, h, gamma, N, H, W, C, dtype, g, need_w, nullptr, true,
                         slabs, dz_scratch, &n2, s, false, nullptr, fold_slabs, fold_P, fold_grp, fold_done));
  ASR_TRY(block_backward(ASR_MODE_EULER, g, x, mask1, w, 0.5f * h, gamma, N, H, W, C, dtype, dx, need_w, dy, false,
                         one_set ? slabs : slabs + (long)n2 * (9L * C * C + C), dz_scratch, &n1, s, false, nullptr,
                         nullptr, 0, nullptr, nullptr, one_set));
  *nsl = one_set ? n2 : n1 + n2;
  return ASR_OK;
}

// ---------------------------------------------------------------------------
// optimizer
// ---------------------------------------------------------------------------
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

// dz1 = dx1 * [x1 > 0] in place (bf16, 8 elements per thread): the stem's
// relu' for networks whose first block's backward cannot fuse it (RK2)
__global__ __launch_bounds__(256) void k_relu_grad_bf16(bf16* __restrict__ d, const bf16* __restrict__ x, long n8) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    bf16x8 dv = ((const bf16x8*)d)[i];
    const bf16x8 xv = ((const bf16x8*)x)[i];
#pragma unroll
    for (int e = 0; e < 8; ++e) dv[e] = (float)xv[e] > 0.f ? dv[e] : (bf16)0.f;
    ((bf16x8*)d)[i] = dv;
  }
}

// host: k_relu_grad_bf16 over n elements (n % 8 == 0), in place on d
int relu_grad_bf16(void* d, const void* x, long n, hipStream_t s) {
  if (n % 8) return fail(ASR_E_ARG, "relu_grad_bf16: n %% 8 != 0");
  const long n8 = n / 8;
  hipLaunchKernelGGL(k_relu_grad_bf16, dim3((unsigned)std::max<long>(1, std::min<long>((n8 + 255) / 256, 4096))),
                     dim3(256), 0, s, (bf16*)d, (const bf16*)x, n8);
  ASR_LAUNCH_CHECK("k_relu_grad_bf16");
  return ASR_OK;
}

// ---------------------------------------------------------------------------
// metrics
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_segment_sq_norms(const float* __restrict__ x, const long* __restrict__ off,
                                                          float* __restrict__ out) {
  const long b = off[blockIdx.x], e = off[blockIdx.x + 1];
  float acc = 0.f;
  for (long i = b + threadIdx.x; i < e; i += blockDim.x) acc = fmaf(x[i], x[i], acc);
  for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
  __shared__ float part[4];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}

// loss == nullptr: the batch-mean Keras categorical cross-entropy is computed
// from the probabilities here (evaluation runs forward only).
__global__ __launch_bounds__(256) void k_batch_metrics(const float* __restrict__ probs, const float* __restrict__ tgt,
                                                       const float* __restrict__ loss, int N, int K,
                                                       float* __restrict__ accum) {
  __shared__ int correct;
  __shared__ float lsum[4];
  if (threadIdx.x == 0) correct = 0;
  __syncthreads();
  float l = 0.f;
  for (int n = threadIdx.x; n < N; n += blockDim.x) {
    const float* p = probs + (long)n * K;
    const float* t = tgt + (long)n * K;
    int ap = 0, at = 0;
    float bp = p[0], bt = t[0], s = 0.f;
    for (int k = 0; k < K; ++k) {  // first maximum, as tf.argmax
      if (p[k] > bp) bp = p[k], ap = k;
      if (t[k] > bt) bt = t[k], at = k;
      s += p[k];
    }
    if (ap == at) atomicAdd(&correct, 1);
    if (!loss)
      for (int k = 0; k < K; ++k) {
        // clipped from above (q = 1: the float above 1.f - 1e-7f): -log(1 - 1e-7) = 1e-7; the float
        // 1.f - 1e-7f is 1 - 2^-23, whose log is 19 % larger
        const float q = p[k] / s;
        l -= t[k] * (q > 1.f - 1e-7f ? -1e-7f : logf(fmaxf(q, 1e-7f)));
      }
  }
  for (int d = 32; d >= 1; d >>= 1) l += __shfl_xor(l, d, 64);
  if ((threadIdx.x & 63) == 0) lsum[threadIdx.x >> 6] = l;
  __syncthreads();
  if (threadIdx.x == 0) {
    accum[0] += loss ? *loss : ((lsum[0] + lsum[1]) + (lsum[2] + lsum[3])) / (float)N;
    accum[1] += (float)correct;
    accum[2] += (float)N;
    accum[3] += 1.f;
  }
}

// ---------------------------------------------------------------------------
// network layout
// ---------------------------------------------------------------------------
template <typename Tin>
__global__ void k_normalize(const Tin* __restrict__ img, long n, float mean, float inv_std, int use_norm,
                            float* __restrict__ out) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float v = (float)img[i];
    if (use_norm) v = (v - mean) * inv_std;
    out[i] = v;
  }
}

struct NetLayout {
  long ntheta, P, E, wstride;  // wstride in elements of the W dtype
  long off_c1k, off_c1b, off_blk, blk_stride, off_fck, off_fcb, nparams;
  bool sep_bwd;  // operator not antisymmetric: dgrad uses W_bwd = -flip(W)^T
  bool rk2;      // RK2 midpoint blocks (x_mid activations, two masks per block)
  int stages;    // conv applications per block (1 Euler, 2 RK2)
  long grp_stride;  // floats of slab group sums per layer
  size_t grp;  // per-layer slab group sums, projected after the whole backward
  size_t slabs_all;  // fp32: every block's slabs, pass 1 of all blocks in one launch after the loop
  long slab_stride;
  size_t w_src, w_src_bwd, theta_dst, wbuf, wbuf_bwd, x0, acts, xmids, masks, dxa, dxb, dxg, bwdws, slabs2, slabs, red, probs,
      loss_per, dlogits, gap, total;
  long mask_bytes;
  int act_bytes;
  bool fast_stem;
  bool deep;          // C=16 stack path: one fused launch forward, one backward (asr_deep16.hip)
  size_t deep_slabs;  // its weight-gradient slabs [L][rows][E+C]
  bool inference;     // ASR_VARIANT_INFERENCE: forward-only workspace (3 activation slots, no backward buffers)
  bool stack_bwd;     // C=64 Euler bf16: all blocks' backward in one k_bwd3_stack launch
  bool stack_pair;    // ... with pair-local slabs (antisymmetric operator: the 74 D tiles, not dW)
  int stack_grid;     // its workgroups
  size_t theta_dst_tm, stack_slabs, stack_done;  // tile-major projection map, [L][grid][E+C] slabs, counters
  size_t theta_dst_pr;  // the pull-back from the pair-local slabs (stack_pair)
  int f32_rows;         // fp32: slab rows of one block application's weight gradient (f32_block_slab_rows)
  size_t grow;        // stacked Euler backward: dL/dx_L as one bf16 row per image (the GAP gradient) [N][C]
  BwdWs bw;           // inside bwdws: one block's backward workspace (asr_conv_backward's layout) ...
  StemWs stem;        // ... and, after the blocks, the stem's
  int k1, kb;         // conv1's and the blocks' kernel size (3, 5 or 7)
  bool stem_kxk;      // k1 != 3 on a shape of the bf16 matrix-core k x k stem (stem_kxk_supported)
  bool kxk;           // kb != 3: one launch per block on the k x k kernels, no stack
  int kxk_rows;       // ... whose weight gradient writes this many slab rows per block
};

// asr_net_config's kernel sizes: 0 means 3
static int net_k1(const asr_net_config* c) { return c->conv1_kernel_size ? c->conv1_kernel_size : 3; }
static int net_kb(const asr_net_config* c) { return c->kernel_size ? c->kernel_size : 3; }

static const char kNetKernelSizes[] =
    "kernel_size and conv1_kernel_size in {0 (= 3), 3, 5, 7}; kernel_size 5 / 7: ASR_PARAM_GENERAL or "
    "ASR_PARAM_REGULAR blocks, Euler integrator, float32 at any shape, bfloat16 at C in {16, 32, 64} and "
    "W in {8, 16, 32}; kernel_size 3 in bfloat16: C in {16, 32, 64, 128, 256} and W == 8 or W % 16 == 0 (RK2: W == 32, "
    "C <= 64)";

static int check_net_kernel_size(const char* field, int k) {
  if (k == 3 || k == 5 || k == 7) return ASR_OK;
  return fail((k < 1 || !(k & 1)) ? ASR_E_ARG : ASR_E_UNSUPPORTED, "%s %d: the network takes %s", field, k,
              kNetKernelSizes);
}

static int net_check(const asr_net_config* c) {
  if (!c) return fail(ASR_E_ARG, "null config");
  ASR_TRY(check_shape(c->N, c->H, c->W, c->C));
  if (c->L < 1 || c->Cin < 1 || c->num_classes < 1)
    return fail(ASR_E_ARG, "bad net config (L=%d Cin=%d K=%d C=%d)", c->L, c->Cin, c->num_classes, c->C);
  if (c->num_classes > 256 || c->C > 256)  // (as asr_stages_check: one workgroup of 256 threads per image)
    return fail(ASR_E_UNSUPPORTED, "the head takes C and num_classes <= 256 (C=%d K=%d)", c->C, c->num_classes);
  if (c->dtype != ASR_F32 && c->dtype != ASR_BF16) return fail(ASR_E_ARG, "bad dtype");
  if (param_is_antisymmetric(c->param_kind, c->antisymmetric) < 0) return ASR_E_ARG;
  if (c->param_kind == ASR_PARAM_3BY3 && !c->antisymmetric)
    return fail(ASR_E_ARG, "the 3by3 parametrisation is always antisymmetric");
  if (c->integrator != ASR_INTEGRATOR_EULER && c->integrator != ASR_INTEGRATOR_RK2)
    return fail(ASR_E_ARG, "bad integrator %d", c->integrator);
  if (c->variant & ~(ASR_VARIANT_NO_FOLD | ASR_VARIANT_STEM_FWD_VALU | ASR_VARIANT_STEM_WGRAD_VALU | ASR_VARIANT_PER_BLOCK_FWD |
                    ASR_VARIANT_PER_BLOCK_BWD | ASR_VARIANT_INFERENCE | ASR_VARIANT_TIMED | ASR_VARIANT_FULL_DXL |
                    ASR_VARIANT_FULL_SLABS | ASR_VARIANT_W_BF16))
    return fail(ASR_E_ARG, "bad variant bits 0x%x", c->variant);
  const int kb = net_kb(c);
  ASR_TRY(check_net_kernel_size("conv1_kernel_size", net_k1(c)));
  ASR_TRY(check_net_kernel_size("kernel_size", kb));
  if (kb != 3) {
    if (c->param_kind == ASR_PARAM_3BY3)
      return fail(ASR_E_ARG, "the 3by3 parametrisation has kernel_size 3 (kernel_size=%d): the network takes %s", kb,
                  kNetKernelSizes);
    if (c->integrator == ASR_INTEGRATOR_RK2)
      return fail(ASR_E_UNSUPPORTED, "RK2 blocks with kernel_size %d: the network takes %s", kb, kNetKernelSizes);
    if (c->dtype == ASR_BF16 && !convk_bf16_supported(kb, c->W, c->C))
      return fail(ASR_E_UNSUPPORTED, "bf16 network with kernel_size %d at C=%d W=%d: the network takes %s", kb, c->C,
                  c->W, kNetKernelSizes);
    return ASR_OK;
  }
  if (c->dtype == ASR_BF16 && !mfma_supported(c->C, c->W)) {
    // off W = 32 the blocks run one by one on the any-width kernels: plain Euler blocks only
    if (!convb_supported(c->W, c->C))
      return fail(ASR_E_UNSUPPORTED,
                  "bf16 network needs C in {16,32,64,128,256} and W == 8 or W %% 16 == 0 (C=%d W=%d)", c->C, c->W);
    if (c->integrator == ASR_INTEGRATOR_RK2)
      return fail(ASR_E_UNSUPPORTED, "bf16 network with RK2 blocks needs W == 32 and C in {16,32,64} (C=%d W=%d)", c->C,
                  c->W);
  }
  return ASR_OK;
}

static NetLayout net_layout(const asr_net_config* c) {
  NetLayout L{};
  const int C = c->C, K = c->num_classes;
  L.k1 = net_k1(c);
  L.kb = net_kb(c);
  L.kxk = L.kb != 3;
  L.ntheta = theta_count_k(C, L.kb, c->param_kind, c->antisymmetric);
  L.sep_bwd = param_is_antisymmetric(c->param_kind, c->antisymmetric) == 0;
  L.rk2 = c->integrator == ASR_INTEGRATOR_RK2;
  L.stages = L.rk2 ? 2 : 1;
  L.P = (long)c->N * c->H * c->W * C;
  L.E = (long)L.kb * L.kb * C * C;
  L.act_bytes = c->dtype == ASR_BF16 ? 2 : 4;
  L.wstride = c->dtype == ASR_BF16 ? (long)(C / 16) * ((L.kb * L.kb * C + 31) / 32) * 512 : L.E;
  L.off_c1k = 0;
  L.off_c1b = (long)L.k1 * L.k1 * c->Cin * C;
  L.off_blk = L.off_c1b + C;
  L.blk_stride = L.ntheta + C;
  L.off_fck = L.off_blk + (long)c->L * L.blk_stride;
  L.off_fcb = L.off_fck + (long)C * K;
  L.nparams = L.off_fcb + K;
  L.mask_bytes = asr_mask_bytes(c->N, c->H, c->W, C);
  L.fast_stem = L.k1 == 3 && stem_supported(c->Cin, c->H, c->W, C);
  L.stem_kxk = c->dtype == ASR_BF16 && L.k1 != 3 && stem_kxk_supported(L.k1, c->Cin, c->W, C);
  L.inference = (c->variant & ASR_VARIANT_INFERENCE) != 0;
  const bool tr = !L.inference;  // training buffers
  L.deep = !L.kxk && c->dtype == ASR_BF16 && !L.rk2 && deep16_supported(c->H, c->W, C);
  L.stack_bwd = !L.kxk && tr && c->dtype == ASR_BF16 && block_stack_bwd_supported(c->N, c->H, c->W, C);
  L.stack_grid = L.stack_bwd ? block_stack_bwd_grid(c->N) : 0;
  L.stack_pair = L.stack_bwd && !L.sep_bwd;
  WsCursor ws;
  L.w_src = ws.take((size_t)L.E * 4);
  L.w_src_bwd = ws.take(L.sep_bwd && tr ? (size_t)L.E * 4 : 0);
  L.theta_dst = ws.take((size_t)L.ntheta * 2 * 4);
  L.wbuf = ws.take((size_t)c->L * L.wstride * L.act_bytes);
  L.wbuf_bwd = ws.take(L.sep_bwd && tr ? (size_t)c->L * L.wstride * L.act_bytes : 0);
  L.x0 = ws.take(L.fast_stem ? 0 : (size_t)c->N * c->H * c->W * c->Cin * 4);
  // training keeps x_0 .. x_L for the backward; inference ping-pongs (x_0 + 2 slots)
  L.acts = ws.take((size_t)(tr ? c->L + 1 : 3) * L.P * L.act_bytes);
  L.xmids = ws.take(L.rk2 ? (size_t)(tr ? c->L : 1) * L.P * L.act_bytes : 0);
  L.masks = ws.take(tr ? (size_t)L.stages * c->L * L.mask_bytes : 0);  // RK2: mask1 of every block, then mask2
  L.dxa = ws.take(tr ? (size_t)L.P * L.act_bytes : 0);
  L.dxb = ws.take(tr ? (size_t)L.P * L.act_bytes : 0);
  L.dxg = ws.take(L.rk2 && tr ? (size_t)L.P * L.act_bytes : 0);
  // per-block backward workspace (asr_conv_backward layout), reused by the stem.
  // fp32 keeps every block's slabs in slabs_all, sized by the grid its weight
  // gradient runs (not the 512-row maximum): no slab rows here, no slabs2
  // k x k blocks: one slab set in the backward workspace, reduced into the block's group sums right after its launch
  const bool f32 = c->dtype == ASR_F32;
  L.kxk_rows = !L.kxk ? 0 : f32 ? wgrad_f32_chunks(c->N, c->H) : wgradk_bf16_slab_rows(L.kb, c->N, c->H, c->W, C);
  L.f32_rows = f32 && !L.kxk ? f32_block_slab_rows(c->N, c->H, c->W, C) : 0;
  // bf16 blocks at C in {128, 256}: every slab area by the rows k_wgradbw writes (Euler only there: one stage)
  const int bf_rows = !f32 && !L.kxk && C > 64 ? bf16_block_slab_rows(c->N, c->H, c->W, C) : kMaxBlockSlabs;
  L.bw = bwd_ws_layout(c->N, c->H, c->W, C, c->dtype, L.stages, L.kb, L.kxk ? L.kxk_rows : f32 ? 0 : -1);
  L.stem = stem_ws_layout(L.P, c->Cin, C, L.k1);
  L.bwdws = ws.take(tr ? std::max(L.bw.total, L.stem.total) : 0);
  // odd Euler blocks' slabs (even ones use the backward workspace's): a
  // block's slabs stay readable while the next block's kernel reduces them
  L.slabs2 = ws.take(tr && !f32 && !L.kxk ? (size_t)L.stages * bf_rows * (L.E + C) * 4 : 0);  // every other block's slabs
  const int rows = L.kxk ? L.kxk_rows : f32 ? L.stages * L.f32_rows : L.stages * bf_rows;
  L.grp_stride = (long)reduce_groups(rows) * (L.E + C);
  L.grp = ws.take(tr ? (size_t)c->L * L.grp_stride * 4 : 0);
  L.slab_stride = (long)rows * (L.E + C);
  L.slabs_all = ws.take(tr && f32 && !L.kxk ? (size_t)c->L * L.slab_stride * 4 : 0);
  L.deep_slabs = ws.take(L.deep && tr ? deep16_slab_bytes(c->N, c->L) : 0);
  L.theta_dst_tm = ws.take(L.stack_bwd ? (size_t)L.ntheta * 2 * 4 : 0);
  L.theta_dst_pr = ws.take(L.stack_pair ? (size_t)L.ntheta * 2 * 4 : 0);
  L.stack_slabs = ws.take(L.stack_bwd ? (size_t)c->L * L.stack_grid * (L.E + C) * 4 : 0);
  L.stack_done = ws.take(L.stack_bwd ? (size_t)stack_done_words(c->L) * 4 : 0);
  L.grow = ws.take(L.stack_bwd && !L.rk2 ? (size_t)c->N * C * 2 : 0);
  L.probs = ws.take((size_t)c->N * K * 4);
  L.loss_per = ws.take(tr ? (size_t)c->N * 4 : 0);
  L.dlogits = ws.take(tr ? (size_t)c->N * K * 4 : 0);
  L.gap = ws.take(tr ? (size_t)c->N * C * 4 : 0);
  L.total = ws.off;
  return L;
}

// ASR_VARIANT_TIMED: HIP events around the block launches of the last timed
// asr_net_forward / asr_net_forward_backward (asr_net_kernel_times): 0-1 the
// blocks' forward, 2-3 the stacked backward kernel, 3-4 its post-launch slab
// reductions and the projection onto theta.  Measurement only.  The events are
// kept per device (created on that device at its first timed call); on one
// device, timed calls from several host threads at once overwrite each
// other's times (one timing thread per device).
constexpr int kMaxTimedDevices = 64;
struct TimedEvents {
  hipEvent_t ev[5];
  bool made;
  unsigned rec;  // bit i: event i recorded by the last timed call on this device
};
static TimedEvents g_tev[kMaxTimedDevices];

static TimedEvents* timed_events_here() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxTimedDevices) return nullptr;
  return &g_tev[dev];
}

static int timed_event(const asr_net_config* c, int i, hipStream_t s) {
  if (!(c->variant & ASR_VARIANT_TIMED)) return ASR_OK;
  TimedEvents* t = timed_events_here();
  if (!t) return fail(ASR_E_HIP, "ASR_VARIANT_TIMED: no current device (or device id >= %d)", kMaxTimedDevices);
  if (!t->made) {
    for (auto& e : t->ev) ASR_TRY(hip_check(hipEventCreate(&e), "hipEventCreate"));
    t->made = true;
  }
  if (i == 0) t->rec = 0;
  ASR_TRY(hip_check(hipEventRecord(t->ev[i], s), "hipEventRecord"));
  t->rec |= 1u << i;
  return ASR_OK;
}

// x_L of a forward: training keeps every activation (slot L); evaluation
// ping-pongs (the C=64 stack over slots 1-2 of the inference layout, the
// per-block kernels over slots 0-1)
static unsigned char* net_xL(const asr_net_config* c, const NetLayout& L, unsigned char* ws, bool training,
                             bool stack_fwd) {
  const size_t a = (size_t)L.P * L.act_bytes;
  if (training) return ws + L.acts + (size_t)c->L * a;
  if (stack_fwd) return ws + L.acts + (size_t)(1 + (c->L - 1) % 2) * a;
  return ws + L.acts + (size_t)(c->L & 1) * a;
}

// the normalised input (v - mean) * inv_std as fp32, at L.x0: the generic stem arm's operand
static int net_normalize(const asr_net_config* c, const NetLayout& L, const void* images, unsigned char* ws,
                         hipStream_t s) {
  const float inv_std = c->use_norm ? 1.f / c->divide_by_stddev : 1.f;
  const long nin = (long)c->N * c->H * c->W * c->Cin;
  float* x0 = (float*)(ws + L.x0);
  const unsigned gn = (unsigned)std::min<long>((nin + 255) / 256, 4096);
  if (c->input_u8)
    hipLaunchKernelGGL(k_normalize<uint8_t>, dim3(gn), dim3(256), 0, s, (const uint8_t*)images, nin, c->subtract_mean,
                       inv_std, c->use_norm, x0);
  else
    hipLaunchKernelGGL(k_normalize<float>, dim3(gn), dim3(256), 0, s, (const float*)images, nin, c->subtract_mean,
                       inv_std, c->use_norm, x0);
  ASR_LAUNCH_CHECK("k_normalize");
  return ASR_OK;
}

static int net_forward_impl(const asr_net_config* c, const NetLayout& L, const float* params, const void* images,
                            bool training, unsigned char* ws, hipStream_t s, unsigned char** xL_out = nullptr) {
  const int C = c->C, N = c->N, H = c->H, W = c->W;
  const bool bf = c->dtype == ASR_BF16;
  const float inv_std = c->use_norm ? 1.f / c->divide_by_stddev : 1.f;
  if (training && L.inference) return fail(ASR_E_ARG, "an ASR_VARIANT_INFERENCE workspace has no training buffers");
  // 1. materialise W for all L blocks (one launch)
  //    (bf16: balanced rounding of the antisymmetric pairs, k_theta_to_w_pack_bal; ASR_VARIANT_W_BF16: to nearest)
  const bool bal = !(c->variant & ASR_VARIANT_W_BF16);
  if (L.kxk) {  // k x k blocks: the single-layer ABI's packs (bf16 rounded to nearest), all L layers per launch
    const float* th = params + L.off_blk;
    const int32_t* src = (const int32_t*)(ws + L.w_src);
    const int32_t* src_bwd = (const int32_t*)(ws + L.w_src_bwd);
    if (bf) {
      ASR_TRY(asr_theta_to_w_k_bf16(th, L.blk_stride, c->L, C, L.kb, src, c->gamma, ws + L.wbuf, L.wstride, s));
      if (training && L.sep_bwd)
        ASR_TRY(asr_theta_to_w_k_bf16(th, L.blk_stride, c->L, C, L.kb, src_bwd, 0.f, ws + L.wbuf_bwd, L.wstride, s));
    } else {
      ASR_TRY(asr_theta_to_w_k(th, L.blk_stride, c->L, C, L.kb, src, c->gamma, (float*)(ws + L.wbuf), L.wstride, s));
      if (training && L.sep_bwd)
        ASR_TRY(asr_theta_to_w_k(th, L.blk_stride, c->L, C, L.kb, src_bwd, 0.f, (float*)(ws + L.wbuf_bwd), L.wstride,
                                 s));
    }
  } else if (bf)
    ASR_TRY(theta_to_w_bf16(params + L.off_blk, L.blk_stride, c->L, C, (const int32_t*)(ws + L.w_src), c->gamma,
                            ws + L.wbuf, L.wstride, bal, s,
                            c->param_kind != ASR_PARAM_REGULAR ? (const int32_t*)(ws + L.theta_dst) : nullptr,
                            L.ntheta));
  else
    ASR_TRY(asr_theta_to_w(params + L.off_blk, L.blk_stride, c->L, C, (const int32_t*)(ws + L.w_src), c->gamma,
                           ws + L.wbuf, L.wstride, c->dtype, s));
  if (training && L.sep_bwd && !L.kxk) {  // (the transposed map pairs the same entries: W_bwd = -W^T after the rounding too)
    if (bf)
      ASR_TRY(theta_to_w_bf16(params + L.off_blk, L.blk_stride, c->L, C, (const int32_t*)(ws + L.w_src_bwd), 0.f,
                              ws + L.wbuf_bwd, L.wstride, bal, s));
    else
      ASR_TRY(asr_theta_to_w(params + L.off_blk, L.blk_stride, c->L, C, (const int32_t*)(ws + L.w_src_bwd), 0.f,
                             ws + L.wbuf_bwd, L.wstride, c->dtype, s));
  }
  unsigned char* acts = ws + L.acts;
  auto act = [&](int i) -> unsigned char* {
    const int slot = training ? i : (i & 1);
    return acts + (size_t)slot * L.P * L.act_bytes;
  };
  if (xL_out) *xL_out = net_xL(c, L, ws, training, false);
  // 2. normalisation + conv1 + relu (tfkeras_resnets.py:555-572)
  if (L.fast_stem && bf && stem_fwd_mfma_supported(c->Cin, H, W, C) && !(c->variant & ASR_VARIANT_STEM_FWD_VALU)) {
    ASR_TRY(stem_fwd_mfma(images, c->input_u8, params + L.off_c1k, params + L.off_c1b, N, H, W, c->Cin, C,
                          c->subtract_mean, inv_std, c->use_norm, act(0), s));
  } else if (L.stem_kxk && !(c->variant & ASR_VARIANT_STEM_FWD_VALU)) {
    ASR_TRY(stem_fwd_kxk(L.k1, images, c->input_u8, params + L.off_c1k, params + L.off_c1b, N, H, W, c->Cin, C,
                         c->subtract_mean, inv_std, c->use_norm, act(0), s));
  } else if (L.fast_stem) {
    ASR_TRY(stem_forward(images, c->input_u8, params + L.off_c1k, params + L.off_c1b, N, H, W, c->Cin, C,
                         c->subtract_mean, inv_std, c->use_norm, act(0), bf ? 1 : 0, s));
  } else {
    float* x0 = (float*)(ws + L.x0);
    ASR_TRY(net_normalize(c, L, images, ws, s));
    ASR_TRY(conv_f32(F_RELU, x0, act(0), nullptr, params + L.off_c1k, params + L.off_c1b, 1.f, 0.f, nullptr, N, H,
                     W, c->Cin, C, bf ? 1 : 0, s, nullptr, L.k1));
  }
  // 3. L Euler blocks (tfkeras_resnets.py:579-582 -> :28-94), or RK2 blocks
  ASR_TRY(timed_event(c, 0, s));
  if (L.deep) {  // C=16: all L steps in one launch, images resident in LDS
    ASR_TRY(deep16_forward(act(0), act(training ? 1 : c->L), L.P, training ? (uint8_t*)(ws + L.masks) : nullptr,
                           L.mask_bytes, ws + L.wbuf, params + L.off_blk + L.ntheta, L.blk_stride, c->h, N, c->L,
                           training, s));
    return timed_event(c, 1, s);
  }
  if (bf && training && L.rk2 && block_stack_fwd_supported(N, H, W, C) && !(c->variant & ASR_VARIANT_PER_BLOCK_FWD)) {
    // C=64 RK2: all 2L stages in one launch
    uint8_t* m1 = (uint8_t*)(ws + L.masks);
    ASR_TRY(block_stack_fwd_rk2_mfma(act(0), act(1), ws + L.xmids, (long)L.P, m1, m1 + (size_t)c->L * L.mask_bytes,
                                     (long)L.mask_bytes, ws + L.wbuf, (long)L.wstride, params + L.off_blk + L.ntheta,
                                     L.blk_stride, c->h, N, H, W, C, c->L, s));
    return timed_event(c, 1, s);
  }
  if (bf && !L.rk2 && !L.kxk && (training || L.inference) && block_stack_fwd_supported(N, H, W, C) &&
      !(c->variant & ASR_VARIANT_PER_BLOCK_FWD)) {
    // C=64: all L blocks in one launch (whole images per workgroup); inference
    // ping-pongs x_l between slots 1 and 2 with no relu masks
    if (training) {
      ASR_TRY(block_stack_fwd_mfma(act(0), act(1), (long)L.P, (uint8_t*)(ws + L.masks), (long)L.mask_bytes,
                                   ws + L.wbuf, (long)L.wstride, params + L.off_blk + L.ntheta, L.blk_stride, c->h, N,
                                   H, W, C, c->L, s));
    } else {
      ASR_TRY(block_stack_fwd_mfma(acts, acts + (size_t)L.P * L.act_bytes, (long)L.P, nullptr, 0, ws + L.wbuf,
                                   (long)L.wstride, params + L.off_blk + L.ntheta, L.blk_stride, c->h, N, H, W, C,
                                   c->L, s, 2));
      if (xL_out) *xL_out = net_xL(c, L, ws, false, true);
    }
    return timed_event(c, 1, s);
  }
  for (int l = 0; l < c->L; ++l) {
    const float* bias = params + L.off_blk + (long)l * L.blk_stride + L.ntheta;
    const unsigned char* wl = ws + L.wbuf + (size_t)l * L.wstride * L.act_bytes;
    uint8_t* mask = training ? (uint8_t*)(ws + L.masks) + (size_t)l * L.mask_bytes : nullptr;
    if (L.rk2) {
      unsigned char* xm = ws + L.xmids + (training ? (size_t)l * L.P * L.act_bytes : 0);
      uint8_t* mask2 = training ? mask + (size_t)c->L * L.mask_bytes : nullptr;
      ASR_TRY(rk2_forward_impl(act(l), xm, act(l + 1), mask, mask2, wl, bias, c->h, N, H, W, C, c->dtype, s));
    } else if (L.kxk && bf) {
      ASR_TRY(convk_bf16(F_EULER, L.kb, act(l), act(l + 1), mask, wl, bias, c->h, 0.f, nullptr, N, H, W, C, s));
    } else if (L.kxk) {
      ASR_TRY(conv_f32_k(F_EULER, L.kb, act(l), act(l + 1), mask, (const float*)wl, bias, c->h, 0.f, nullptr, N, H, W,
                         C, s, nullptr));
    } else if (bf && !mfma_supported(C, W)) {  // W != 32: the any-width kernels (column strips at W >= 48)
      ASR_TRY(convb_forward(act(l), act(l + 1), mask, wl, bias, c->h, N, H, W, C, s));
    } else if (bf) {
      ASR_TRY(block_fwd_mfma(0, act(l), nullptr, act(l + 1), mask, wl, bias, c->h, N, H, W, C, s));
    } else {
      ASR_TRY(conv_f32(F_EULER, act(l), act(l + 1), mask, (const float*)wl, bias, c->h, 0.f, nullptr, N, H, W, C, C,
                       0, s));
    }
  }
  return timed_event(c, 1, s);
}

// ---------------------------------------------------------------------------
// A stage whose L Euler blocks run fused: the host sequence behind the stack
// ABI (asr_block_stack_*, below) and the multi-stage executor (asr_stages.hip)
// ---------------------------------------------------------------------------
int fused_stage_kind(int H, int W, int C, int dtype) {
  if (dtype == ASR_BF16 && deep16_supported(H, W, C)) return kFusedDeep16;
  return stage_img_supported(H, W, C, dtype) ? kFusedImg : kFusedNone;
}

// x0 -> ys (layer l's output at ys + l y_stride, its relu mask at masks + l mask_stride), one launch.  deep16 also
// takes store_all = false (x_L only, at ys) and null masks; the image-resident kernels need every output, bias and
// masks.
int fused_stage_forward(int kind, int dtype, const void* x0, void* ys, long y_stride, uint8_t* masks, long mask_stride,
                        const void* w, long w_stride, const float* bias, long bias_stride, float h, int N, int H, int W,
                        int C, int L, bool store_all, hipStream_t s) {
  if (kind == kFusedDeep16)
    return deep16_forward(x0, ys, y_stride, masks, mask_stride, w, bias, bias_stride, h, N, L, store_all, s);
  if (kind != kFusedImg || !store_all)
    return fail(ASR_E_ARG, "fused_stage_forward: kind %d, store_all %d", kind, store_all);
  return stage_img_forward(dtype, x0, ys, y_stride, masks, mask_stride, w, w_stride, bias, bias_stride, h, N, H, W, C,
                           L, s);
}

// Its backward.  d holds dL/dx_L; dx_0 ends in d or in e (*in_e).  deep16 ping-pongs between the two (d is
// overwritten; dx0_copy, nullable: dx_0 is also copied there, right behind the kernel); the image-resident kernel
// reads d, writes e and stores the gradient entering each layer at dys ([L][N H W C], unpadded).
// dparams == nullptr: input gradient only.  Else every layer's weight gradient: slabs [L][slab_stride] (the
// caller's room: slab_rows rows a layer; ASR_E_WORKSPACE if the launch wrote another count), pass 1 into
// grp [L][grp_stride], pass 2 + projection onto theta: [dtheta | dbias] of layer l at dparams + l dp_stride.
int fused_stage_backward(const char* who, int kind, int dtype, void* d, void* e, int* in_e, void* dx0_copy, void* dys,
                         const void* xs, long x_stride, const uint8_t* masks, long mask_stride, const void* w,
                         long w_stride, float h, float two_gamma, int N, int H, int W, int C, int L, float* slabs,
                         long slab_stride, int slab_rows, float* grp, long grp_stride, const int32_t* theta_dst,
                         long n_theta, float* dparams, long dp_stride, hipStream_t s) {
  const long E = 9L * C * C, P = (long)N * H * W * C;
  int rows = 0;
  if (kind == kFusedDeep16) {  // dx resident in LDS, one slab set per layer
    ASR_TRY(deep16_backward(d, e, xs, x_stride, masks, mask_stride, w, h, two_gamma, N, L, slabs, &rows, in_e, s));
    if (dx0_copy)
      ASR_TRY(hip_check(hipMemcpyAsync(dx0_copy, *in_e ? e : d, (size_t)P * 2, hipMemcpyDeviceToDevice, s),
                        "hipMemcpyAsync"));
    if (!dparams) return ASR_OK;
    if (rows != slab_rows) return fail(ASR_E_WORKSPACE, "%s: deep16 slab rows %d != %d", who, rows, slab_rows);
    ASR_TRY(reduce_slabs_to_groups(slabs, L * rows, E + C, grp, s));
    return project_layers(grp, grp_stride, reduce_groups(rows), E, C, theta_dst, n_theta, L, dparams, dp_stride, s);
  }
  if (kind != kFusedImg) return fail(ASR_E_ARG, "%s: not a fused stage", who);
  // input gradients in one launch (a workgroup per image), then every layer's weight gradient in one: x_l and
  // the gradient entering layer l, dys + l P
  *in_e = 1;
  ASR_TRY(stage_img_backward(dtype, d, dys, P, e, masks, mask_stride, w, w_stride, h, two_gamma, N, H, W, C, L, s));
  if (!dparams) return ASR_OK;
  ASR_TRY(wgrad_layers(dtype, xs, x_stride, dys, P, masks, mask_stride, h, N, H, W, C, L, slabs, slab_stride, &rows, s));
  if (rows > slab_rows) return fail(ASR_E_WORKSPACE, "%s: %d slab rows > the workspace's %d", who, rows, slab_rows);
  ASR_TRY(reduce_slab_layers(slabs, slab_stride, rows, E + C, grp, grp_stride, L, s));
  return project_layers(grp, grp_stride, reduce_groups(rows), E, C, theta_dst, n_theta, L, dparams, dp_stride, s);
}

}  // namespace asr

using namespace asr;

extern "C" {

long asr_mask_bytes(int N, int H, int W, int C) {
  if (N < 1 || H < 1 || W < 1 || C < 1) return -1;
  return ((long)N * H * W * C + 31) / 32 * 4;
}

int asr_conv_forward(int mode, const void* x, void* y, uint8_t* mask, const void* w, const float* bias, float h,
                     int N, int H, int W, int C, int dtype, asr_stream_t stream) {
  ASR_TRY(check_shape(N, H, W, C));
  if (!x || !y || !w) return fail(ASR_E_ARG, "asr_conv_forward: null pointer");
  if (mode != ASR_MODE_EULER && mode != ASR_MODE_CONV) return fail(ASR_E_ARG, "asr_conv_forward: bad mode %d", mode);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == ASR_BF16) {
    ASR_TRY(check_bf16_conv(C, W));
    if (!mfma_supported(C, W))  // W = 16 / 8 (multi-stage nets): the any-width bf16 kernels, Euler block or bare conv
      return convb_forward(x, y, mask, w, bias, h, N, H, W, C, s, mode == ASR_MODE_CONV);
    if (mode == ASR_MODE_EULER && deep16_supported(H, W, C))
      return deep16_forward(x, y, 0, mask, 0, w, bias, 0, h, N, 1, true, s);
    return block_fwd_mfma(mode == ASR_MODE_EULER ? 0 : 1, x, nullptr, y, mask, w, bias, h, N, H, W, C, s);
  }
  if (dtype == ASR_F32)
    return conv_f32(mode == ASR_MODE_EULER ? F_EULER : F_CONV, x, y, mask, (const float*)w, bias, h, 0.f, nullptr, N,
                    H, W, C, C, 0, s);
  return fail(ASR_E_ARG, "asr_conv_forward: bad dtype %d", dtype);
}

// The image-resident stage kernels' vector accesses need per-layer strides that keep every layer aligned
// (a stride of 0 means "not passed to this call").  bf16: 8-B y stores, 2-B
// mask stores, 16-B W fragment / bias / x (k_wgradb) loads; fp32: 16-B y
// stores and bias / x (k_wgrad32) loads, 2-B mask stores, scalar W loads.
static int stack_img_check_strides(const char* who, int dtype, long y_stride, long mask_stride, long w_stride,
                                   long bias_stride, long x_stride) {
  const bool bf = dtype == ASR_BF16;
  if (y_stride % 4) return fail(ASR_E_ARG, "%s: y_stride %% 4 != 0 on the image-resident path", who);
  if (mask_stride % 2) return fail(ASR_E_ARG, "%s: mask_stride %% 2 != 0 on the image-resident path", who);
  if (bf && w_stride % 8) return fail(ASR_E_ARG, "%s: w_stride %% 8 != 0 on the image-resident path", who);
  if (bias_stride % 4) return fail(ASR_E_ARG, "%s: bias_stride %% 4 != 0 on the image-resident path", who);
  if (x_stride % (bf ? 8 : 4))
    return fail(ASR_E_ARG, "%s: x_stride %% %d != 0 on the image-resident path", who, bf ? 8 : 4);
  return ASR_OK;
}

int asr_block_stack_forward(const void* x0, void* ys, long y_stride, uint8_t* masks, long mask_stride, const void* w,
                            long w_stride, const float* bias, long bias_stride, float h, int N, int H, int W, int C,
                            int L, int dtype, int store_all, asr_stream_t stream) {
  ASR_TRY(check_shape(N, H, W, C));
  if (!x0 || !ys || !w || L < 1) return fail(ASR_E_ARG, "asr_block_stack_forward: null pointer or L < 1");
  if (store_all && L > 1 && y_stride < (long)N * H * W * C)
    return fail(ASR_E_ARG, "asr_block_stack_forward: y_stride smaller than one activation");
  hipStream_t s = (hipStream_t)stream;
  const int fused = fused_stage_kind(H, W, C, dtype);
  if (fused == kFusedDeep16) {
    if (L > 1 && w_stride != (long)asr_wpack_elems(C))
      return fail(ASR_E_ARG, "asr_block_stack_forward: w_stride must be asr_wpack_elems(C) on the fused path");
    return fused_stage_forward(fused, dtype, x0, ys, y_stride, masks, mask_stride, w, w_stride, bias, bias_stride, h, N,
                               H, W, C, L, store_all != 0, s);
  }
  if (dtype == ASR_BF16) ASR_TRY(check_bf16_conv(C, W));
  if (dtype != ASR_F32 && dtype != ASR_BF16) return fail(ASR_E_ARG, "asr_block_stack_forward: bad dtype");
  const size_t es = dtype == ASR_BF16 ? 2 : 4;
  if (!store_all && L > 1) return fail(ASR_E_UNSUPPORTED, "asr_block_stack_forward: store_all=0 needs the fused path");
  // image-resident stages: all L blocks in one launch, a workgroup per image.  The kernels store every
  // layer and read bias and masks unconditionally; calls without them take the per-block sequence.
  if (fused == kFusedImg && store_all && bias && masks) {
    ASR_TRY(stack_img_check_strides("asr_block_stack_forward", dtype, y_stride, mask_stride, w_stride, bias_stride, 0));
    return fused_stage_forward(fused, dtype, x0, ys, y_stride, masks, mask_stride, w, w_stride, bias, bias_stride, h, N,
                               H, W, C, L, true, s);
  }
  if (dtype == ASR_BF16 && block_stack_fwd_supported(N, H, W, C))
    return block_stack_fwd_mfma(x0, ys, L > 1 ? y_stride : (long)N * H * W * C, masks, mask_stride, w, w_stride, bias,
                                bias_stride, h, N, H, W, C, L, s);
  for (int l = 0; l < L; ++l) {
    const void* xi = l == 0 ? x0 : (const unsigned char*)ys + (size_t)(l - 1) * y_stride * es;
    void* yo = (unsigned char*)ys + (size_t)l * y_stride * es;
    ASR_TRY(asr_conv_forward(ASR_MODE_EULER, xi, yo, masks ? masks + (size_t)l * mask_stride : nullptr,
                             (const unsigned char*)w + (size_t)l * w_stride * es, bias ? bias + l * bias_stride : nullptr,
                             h, N, H, W, C, dtype, stream));
  }
  return ASR_OK;
}

// workspace of asr_block_stack_backward: two dx buffers, then either the
// fused path's slabs + group rows or one per-block backward workspace
struct StackWs {
  size_t da, db, slabs, grp, blk, done, tdst, g, dys, total;
  int fused;  // fused_stage_kind (RK2: kFusedNone)
  bool stack64;
  int grid;
  int rows;  // fused: the slab rows per layer the workspace holds
};
static StackWs stack_ws_layout(int N, int H, int W, int C, int L, int dtype, bool rk2 = false) {
  StackWs w{};
  const size_t act = (size_t)N * H * W * C * (dtype == ASR_BF16 ? 2 : 4);
  const long ES = 9L * C * C + C;
  w.fused = rk2 ? kFusedNone : fused_stage_kind(H, W, C, dtype);
  w.stack64 = dtype == ASR_BF16 && w.fused == kFusedNone && block_stack_bwd_supported(N, H, W, C);
  w.grid = w.stack64 ? block_stack_bwd_grid(N) : 0;
  WsCursor c;
  w.da = c.take(act);
  w.db = c.take(act);
  if (w.fused == kFusedImg) {  // the gradient entering every layer (L activations, unpadded), slabs [L][rows][ES], grp
    w.rows = f32_block_slab_rows(N, H, W, C);
    w.dys = c.take(L * act);
    w.slabs = c.take((size_t)L * w.rows * ES * 4);
    w.grp = c.take((size_t)L * reduce_groups(w.rows) * ES * 4);
  } else if (w.fused == kFusedDeep16) {
    w.rows = (int)(deep16_slab_bytes(N, 1) / ((size_t)ES * 4));
    w.slabs = c.take(deep16_slab_bytes(N, L));
    w.grp = c.take((size_t)L * reduce_groups(kMaxBlockSlabs) * ES * 4);
  } else if (w.stack64) {  // slabs [L][grid][ES] (tile-major dW), group rows, counters, tile-major theta map
    w.slabs = c.take((size_t)L * w.grid * ES * 4);
    w.grp = c.take((size_t)L * reduce_groups(w.grid) * ES * 4);
    w.done = c.take((size_t)stack_done_words(L) * 4);
    w.tdst = c.take((size_t)2 * 9 * C * C * 4);
    if (rk2) w.g = c.take(act);  // the gradient reaching x_mid between a block's two stages
  } else {
    w.blk = c.take(bwd_ws_layout(N, H, W, C, dtype).total);
  }
  w.total = c.off;
  return w;
}

// The C=64 stack kernel behind asr_block_stack_backward (xmids = masks2 = nullptr) and
// asr_rk2_stack_backward: dyL into the kernel's ping-pong pair, one launch for all L blocks,
// dx0 out, then the slab passes the launch left over and the projection onto theta.
static int stack64_backward(const char* who, const StackWs& Lw, const void* dyL, const void* xs, const void* xmids,
                            long x_stride, const uint8_t* masks, const uint8_t* masks2, long mask_stride,
                            const void* w, long w_stride, const int32_t* theta_dst, long n_theta, float h, float gamma,
                            int N, int H, int W, int C, int L, void* dx0, float* dparams, unsigned char* base,
                            hipStream_t s) {
  if (n_theta > 9L * C * C) return fail(ASR_E_ARG, "%s: n_theta > 9*C*C", who);
  const size_t act = (size_t)N * H * W * C * 2;
  ASR_TRY(hip_check(hipMemcpyAsync(base + Lw.da, dyL, act, hipMemcpyDeviceToDevice, s), "hipMemcpyAsync"));
  float* slabs = (float*)(base + Lw.slabs);
  float* grp = (float*)(base + Lw.grp);
  // the stack ABI's operator is antisymmetric (its dgrad is A^T = -A + 2 gamma I): pair-local slabs
  const long ES = stack_slab_floats(C, 1), sst = (long)Lw.grid * ES, gst = (long)reduce_groups(Lw.grid) * ES;
  int lfold = L;
  ASR_TRY(block_stack_bwd_mfma(base + Lw.da, base + Lw.db, xs, x_stride, masks, mask_stride, w, w_stride, h,
                               2.f * gamma, N, H, W, C, L, 0, slabs, sst, grp, gst, (unsigned*)(base + Lw.done),
                               &lfold, s, xmids, masks2, xmids ? base + Lw.g : nullptr, nullptr, 1, 1));
  ASR_TRY(hip_check(hipMemcpyAsync(dx0, base + ((L & 1) ? Lw.db : Lw.da), act, hipMemcpyDeviceToDevice, s),
                    "hipMemcpyAsync"));
  if (!dparams) return ASR_OK;
  ASR_TRY(stack_bwd_reduce_rest(slabs, sst, Lw.grid, ES, grp, gst, L, lfold, (const unsigned*)(base + Lw.done), s));
  int32_t* tm = (int32_t*)(base + Lw.tdst);
  ASR_TRY(theta_dst_pair(theta_dst, n_theta, C, tm, s));
  return project_layers(grp, gst, reduce_groups(Lw.grid), ES - C, C, tm, n_theta, L, dparams, n_theta + C, s);
}

size_t asr_block_stack_backward_workspace_bytes(int N, int H, int W, int C, int L, int dtype) {
  if (check_shape(N, H, W, C) != ASR_OK || L < 1) return 0;
  return stack_ws_layout(N, H, W, C, L, dtype).total;
}

int asr_block_stack_backward(const void* dyL, const void* xs, long x_stride, const uint8_t* masks, long mask_stride,
                             const void* w, long w_stride, const int32_t* theta_dst, long n_theta, float h,
                             float gamma, int N, int H, int W, int C, int L, int dtype, void* dx0, float* dparams,
                             void* ws, size_t ws_bytes, asr_stream_t stream) {
  ASR_TRY(check_shape(N, H, W, C));
  if (!dyL || !xs || !masks || !w || !dx0 || L < 1) return fail(ASR_E_ARG, "asr_block_stack_backward: null pointer");
  if (dparams && !theta_dst) return fail(ASR_E_ARG, "asr_block_stack_backward: theta_dst needed for dparams");
  if (dtype != ASR_F32 && dtype != ASR_BF16) return fail(ASR_E_ARG, "asr_block_stack_backward: bad dtype");
  if (dtype == ASR_BF16) ASR_TRY(check_bf16_conv(C, W));
  const StackWs Lw = stack_ws_layout(N, H, W, C, L, dtype);
  if (Lw.fused == kFusedImg)
    ASR_TRY(stack_img_check_strides("asr_block_stack_backward", dtype, 0, 0, w_stride, 0, x_stride));
  if (!ws || ws_bytes < Lw.total) return fail(ASR_E_WORKSPACE, "asr_block_stack_backward: workspace too small");
  if (Lw.fused == kFusedDeep16 && w_stride != (long)asr_wpack_elems(C))
    return fail(ASR_E_ARG, "asr_block_stack_backward: w_stride must be asr_wpack_elems(C) on the fused path");
  hipStream_t s = (hipStream_t)stream;
  unsigned char* base = (unsigned char*)ws;
  const size_t es = dtype == ASR_BF16 ? 2 : 4, act = (size_t)N * H * W * C * es;
  if (Lw.fused != kFusedNone) {
    // the image-resident kernel reads dyL and writes dx0; deep16 ping-pongs in the workspace pair (dyL copied in,
    // dx0 copied out by the shared function)
    const bool deep = Lw.fused == kFusedDeep16;
    const long ES = 9L * C * C + C;
    if (deep) ASR_TRY(hip_check(hipMemcpyAsync(base + Lw.da, dyL, act, hipMemcpyDeviceToDevice, s), "hipMemcpyAsync"));
    int in_e = 0;
    return fused_stage_backward("asr_block_stack_backward", Lw.fused, dtype, deep ? base + Lw.da : (void*)dyL,
                                deep ? base + Lw.db : dx0, &in_e, deep ? dx0 : nullptr, base + Lw.dys, xs, x_stride,
                                masks, mask_stride, w, w_stride, h, 2.f * gamma, N, H, W, C, L,
                                (float*)(base + Lw.slabs), (long)Lw.rows * ES, Lw.rows, (float*)(base + Lw.grp),
                                (long)reduce_groups(Lw.rows) * ES, theta_dst, n_theta, dparams, n_theta + C, s);
  }
  if (Lw.stack64)
    return stack64_backward("asr_block_stack_backward", Lw, dyL, xs, nullptr, x_stride, masks, nullptr, mask_stride, w,
                            w_stride, theta_dst, n_theta, h, gamma, N, H, W, C, L, dx0, dparams, base, s);
  // per-block kernels, last block first
  const void* dcur = dyL;
  for (int l = L - 1; l >= 0; --l) {
    void* dnext = l == 0 ? dx0 : base + ((l & 1) ? Lw.db : Lw.da);
    float* dp = dparams ? dparams + (long)l * (n_theta + C) : nullptr;
    ASR_TRY(asr_conv_backward(ASR_MODE_EULER, dcur, (const unsigned char*)xs + (size_t)l * x_stride * es,
                              masks + (size_t)l * mask_stride, (const unsigned char*)w + (size_t)l * w_stride * es,
                              theta_dst, n_theta, h, gamma, N, H, W, C, dtype, dnext, dp, dp ? dp + n_theta : nullptr,
                              nullptr, base + Lw.blk, ws_bytes - Lw.blk, stream));
    dcur = dnext;
  }
  return ASR_OK;
}

int asr_rk2_stack_forward(const void* x0, void* ys, void* xmids, long y_stride, uint8_t* masks1, uint8_t* masks2,
                          long mask_stride, const void* w, long w_stride, const float* bias, long bias_stride, float h,
                          int N, int H, int W, int C, int L, int dtype, asr_stream_t stream) {
  ASR_TRY(check_shape(N, H, W, C));
  if (!x0 || !ys || !xmids || !w || L < 1) return fail(ASR_E_ARG, "asr_rk2_stack_forward: null pointer or L < 1");
  if (dtype != ASR_BF16 || !block_stack_fwd_supported(N, H, W, C))
    return fail(ASR_E_UNSUPPORTED, "asr_rk2_stack_forward: bf16, C=64, W=32 only (C=%d W=%d)", C, W);
  if ((masks1 == nullptr) != (masks2 == nullptr)) return fail(ASR_E_ARG, "asr_rk2_stack_forward: masks1/masks2");
  return block_stack_fwd_rk2_mfma(x0, ys, xmids, y_stride, masks1, masks2, mask_stride, w, w_stride, bias,
                                  bias_stride, h, N, H, W, C, L, (hipStream_t)stream);
}

size_t asr_rk2_stack_backward_workspace_bytes(int N, int H, int W, int C, int L, int dtype) {
  if (check_shape(N, H, W, C) != ASR_OK || L < 1) return 0;
  const StackWs w = stack_ws_layout(N, H, W, C, L, dtype, true);
  return w.stack64 ? w.total : 0;
}

int asr_rk2_stack_backward(const void* dyL, const void* xs, const void* xmids, long x_stride, const uint8_t* masks1,
                           const uint8_t* masks2, long mask_stride, const void* w, long w_stride,
                           const int32_t* theta_dst, long n_theta, float h, float gamma, int N, int H, int W, int C,
                           int L, int dtype, void* dx0, float* dparams, void* ws, size_t ws_bytes,
                           asr_stream_t stream) {
  ASR_TRY(check_shape(N, H, W, C));
  if (!dyL || !xs || !xmids || !masks1 || !masks2 || !w || !dx0 || L < 1)
    return fail(ASR_E_ARG, "asr_rk2_stack_backward: null pointer");
  if (dparams && !theta_dst) return fail(ASR_E_ARG, "asr_rk2_stack_backward: theta_dst needed for dparams");
  const StackWs Lw = stack_ws_layout(N, H, W, C, L, dtype, true);
  if (!Lw.stack64) return fail(ASR_E_UNSUPPORTED, "asr_rk2_stack_backward: bf16, C=64, W=32 only (C=%d W=%d)", C, W);
  if (!ws || ws_bytes < Lw.total) return fail(ASR_E_WORKSPACE, "asr_rk2_stack_backward: workspace too small");
  return stack64_backward("asr_rk2_stack_backward", Lw, dyL, xs, xmids, x_stride, masks1, masks2, mask_stride, w,
                          w_stride, theta_dst, n_theta, h, gamma, N, H, W, C, L, dx0, dparams, (unsigned char*)ws,
                          (hipStream_t)stream);
}

size_t asr_conv_backward_workspace_bytes_k(int N, int H, int W, int C, int kernel_size) {
  if (check_shape(N, H, W, C) != ASR_OK || kernel_size < 1 || !(kernel_size & 1)) return 0;
  return bwd_ws_layout(N, H, W, C, ASR_F32, 1, kernel_size).total;
}

// Conv2DAntisymmetric(kernel_size != 3) (…Conv2DAntisymmetric.py:60-68, 109-145, 163-170): the
// same operator family on a K x K kernel, fp32 (the reference's precision) on the VALU kernels;
// K = 3 is asr_conv_forward / asr_conv_backward.
int asr_conv_forward_k(int mode, int kernel_size, const float* x, float* y, uint8_t* mask, const float* w,
                       const float* bias, float h, int N, int H, int W, int C, asr_stream_t stream) {
  ASR_TRY(check_shape(N, H, W, C));
  if (!x || !y || !w) return fail(ASR_E_ARG, "asr_conv_forward_k: null pointer");
  if (mode != ASR_MODE_EULER && mode != ASR_MODE_CONV) return fail(ASR_E_ARG, "asr_conv_forward_k: bad mode %d", mode);
  ASR_TRY(check_kernel_size("asr_conv_forward_k", kernel_size));
  return conv_f32_k(mode == ASR_MODE_EULER ? F_EULER : F_CONV, kernel_size, x, y, mask, w, bias, h, 0.f, nullptr, N, H, W,
                    C, (hipStream_t)stream, nullptr);
}

int asr_conv_backward_k(int mode, int kernel_size, const float* dy, const float* x, const uint8_t* mask,
                        const float* w, const int32_t* theta_dst, long n_theta, float h, float gamma, int N, int H,
                        int W, int C, float* dx, float* dtheta, float* dbias, float* dw, void* ws, size_t ws_bytes,
                        asr_stream_t stream) {
  ASR_TRY(check_shape(N, H, W, C));
  if (mode != ASR_MODE_EULER && mode != ASR_MODE_CONV) return fail(ASR_E_ARG, "asr_conv_backward_k: bad mode %d", mode);
  ASR_TRY(check_kernel_size("asr_conv_backward_k", kernel_size));
  if (!dy || !w || (mode == ASR_MODE_EULER && !mask)) return fail(ASR_E_ARG, "asr_conv_backward_k: null pointer");
  if ((dtheta || dbias || dw) && !x) return fail(ASR_E_ARG, "asr_conv_backward_k: x needed for weight gradients");
  if (dtheta && !theta_dst) return fail(ASR_E_ARG, "asr_conv_backward_k: theta_dst needed for dtheta");
  const BwdWs Lw = bwd_ws_layout(N, H, W, C, ASR_F32, 1, kernel_size);
  if (!ws || ws_bytes < Lw.total) return fail(ASR_E_WORKSPACE, "asr_conv_backward_k: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  unsigned char* base = (unsigned char*)ws;
  float* dz = (float*)(base + Lw.dz);
  float* slabs = (float*)(base + Lw.slabs);
  const bool euler = mode == ASR_MODE_EULER;
  ASR_TRY(make_dz(euler ? F_EULER : F_CONV, dy, mask, nullptr, h, N, H, W, C, 0, dz, s));
  if (dx) ASR_TRY(conv_f32_k(euler ? B_EULER : B_CONV, kernel_size, dz, dx, nullptr, w, nullptr, h, 2.f * gamma, dy, N, H,
                             W, C, s, nullptr));
  if (dtheta || dbias || dw) {
    int nsl = 0;
    ASR_TRY(wgrad_f32(x, 0, dz, N, H, W, C, C, slabs, &nsl, s, kernel_size));
    ASR_TRY(reduce_and_project(slabs, nsl, (long)kernel_size * kernel_size * C * C, C, dtheta ? theta_dst : nullptr,
                               n_theta, dtheta, dbias, dw, (float*)(base + Lw.red), s));
  }
  return ASR_OK;
}

// The same layer in bf16 (fp32 accumulation) on the matrix cores (asr_conv_kxk.hip), for
// kernel_size in {5, 7}, C in {16, 32, 64}, W in {8, 16, 32}; w: asr_theta_to_w_k_bf16's pack.
static int check_k_bf16(const char* fn, int kernel_size, int W, int C) {
  ASR_TRY(check_kernel_size(fn, kernel_size));
  if (!convk_bf16_supported(kernel_size, W, C))
    return fail(ASR_E_UNSUPPORTED,
                "%s: the bf16 k x k kernels take kernel_size in {5, 7}, C in {16, 32, 64}, W in {8, 16, 32} "
                "(kernel_size=%d C=%d W=%d)", fn, kernel_size, C, W);
  return ASR_OK;
}

// workspace of asr_conv_backward_k_bf16: the weight-gradient slabs, then reduce_and_project's rows
struct BwdWsK {
  size_t slabs, red, total;
  int rows;
};
static BwdWsK bwd_ws_layout_k_bf16(int N, int H, int W, int C, int K) {
  BwdWsK b{};
  const long ES = (long)K * K * C * C + C;
  b.rows = wgradk_bf16_slab_rows(K, N, H, W, C);
  WsCursor c;
  b.slabs = c.take((size_t)b.rows * ES * 4);
  b.red = c.take(reduce_ws_bytes(b.rows, ES));
  b.total = c.off;
  return b;
}

int asr_conv_forward_k_bf16(int mode, int kernel_size, const void* x, void* y, uint8_t* mask, const void* w,
                            const float* bias, float h, int N, int H, int W, int C, asr_stream_t stream) {
  ASR_TRY(check_shape(N, H, W, C));
  if (!x || !y || !w) return fail(ASR_E_ARG, "asr_conv_forward_k_bf16: null pointer");
  if (mode != ASR_MODE_EULER && mode != ASR_MODE_CONV)
    return fail(ASR_E_ARG, "asr_conv_forward_k_bf16: bad mode %d", mode);
  ASR_TRY(check_k_bf16("asr_conv_forward_k_bf16", kernel_size, W, C));
  return convk_bf16(mode == ASR_MODE_EULER ? F_EULER : F_CONV, kernel_size, x, y, mask, w, bias, h, 0.f, nullptr, N, H,
                    W, C, (hipStream_t)stream);
}

size_t asr_conv_backward_workspace_bytes_k_bf16(int N, int H, int W, int C, int kernel_size) {
  if (check_shape(N, H, W, C) != ASR_OK || !convk_bf16_supported(kernel_size, W, C)) return 0;
  return bwd_ws_layout_k_bf16(N, H, W, C, kernel_size).total;
}

int asr_conv_backward_k_bf16(int mode, int kernel_size, const void* dy, const void* x, const uint8_t* mask,
                             const void* w, const int32_t* theta_dst, long n_theta, float h, float gamma, int N, int H,
                             int W, int C, void* dx, float* dtheta, float* dbias, float* dw, void* ws, size_t ws_bytes,
                             asr_stream_t stream) {
  ASR_TRY(check_shape(N, H, W, C));
  if (mode != ASR_MODE_EULER && mode != ASR_MODE_CONV)
    return fail(ASR_E_ARG, "asr_conv_backward_k_bf16: bad mode %d", mode);
  ASR_TRY(check_k_bf16("asr_conv_backward_k_bf16", kernel_size, W, C));
  if (!dy || !w || (mode == ASR_MODE_EULER && !mask)) return fail(ASR_E_ARG, "asr_conv_backward_k_bf16: null pointer");
  if ((dtheta || dbias || dw) && !x) return fail(ASR_E_ARG, "asr_conv_backward_k_bf16: x needed for weight gradients");
  if (dtheta && !theta_dst) return fail(ASR_E_ARG, "asr_conv_backward_k_bf16: theta_dst needed for dtheta");
  const BwdWsK Lw = bwd_ws_layout_k_bf16(N, H, W, C, kernel_size);
  if (!ws || ws_bytes < Lw.total) return fail(ASR_E_WORKSPACE, "asr_conv_backward_k_bf16: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  unsigned char* base = (unsigned char*)ws;
  const bool euler = mode == ASR_MODE_EULER;
  if (dx) ASR_TRY(convk_bf16(euler ? B_EULER : B_CONV, kernel_size, dy, dx, nullptr, w, nullptr, h, 2.f * gamma,
                             euler ? mask : nullptr, N, H, W, C, s));
  if (dtheta || dbias || dw) {
    float* slabs = (float*)(base + Lw.slabs);
    int nsl = 0;
    ASR_TRY(wgradk_bf16(kernel_size, x, dy, euler ? mask : nullptr, euler ? h : 1.f, N, H, W, C, slabs, &nsl, s));
    ASR_TRY(reduce_and_project(slabs, nsl, (long)kernel_size * kernel_size * C * C, C, dtheta ? theta_dst : nullptr,
                               n_theta, dtheta, dbias, dw, (float*)(base + Lw.red), s));
  }
  return ASR_OK;
}

size_t asr_conv_backward_workspace_bytes(int N, int H, int W, int C, int dtype) {
  if (check_shape(N, H, W, C) != ASR_OK) return 0;
  return bwd_ws_layout(N, H, W, C, dtype).total;
}

int asr_conv_backward(int mode, const void* dy, const void* x, const uint8_t* mask, const void* w,
                      const int32_t* theta_dst, long n_theta, float h, float gamma, int N, int H, int W, int C,
                      int dtype, void* dx, float* dtheta, float* dbias, float* dw_hwio, void* ws, size_t ws_bytes,
                      asr_stream_t stream) {
  ASR_TRY(check_shape(N, H, W, C));
  if (mode != ASR_MODE_EULER && mode != ASR_MODE_CONV) return fail(ASR_E_ARG, "asr_conv_backward: bad mode %d", mode);
  if (!dy || !w || (mode == ASR_MODE_EULER && !mask)) return fail(ASR_E_ARG, "asr_conv_backward: null pointer");
  if ((dtheta || dbias || dw_hwio) && !x) return fail(ASR_E_ARG, "asr_conv_backward: x needed for weight gradients");
  if (dtheta && !theta_dst) return fail(ASR_E_ARG, "asr_conv_backward: theta_dst needed for dtheta");
  if (dtype != ASR_F32 && dtype != ASR_BF16) return fail(ASR_E_ARG, "asr_conv_backward: bad dtype");
  if (dtype == ASR_BF16) ASR_TRY(check_bf16_conv(C, W));
  const BwdWs L = bwd_ws_layout(N, H, W, C, dtype);
  if (!ws || ws_bytes < L.total) return fail(ASR_E_WORKSPACE, "asr_conv_backward: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  unsigned char* base = (unsigned char*)ws;
  float* slabs = (float*)(base + L.slabs);
  const bool need_w = dtheta || dbias || dw_hwio;
  int nsl = 0;
  ASR_TRY(block_backward(mode, dy, x, mask, w, h, gamma, N, H, W, C, dtype, dx, need_w, nullptr, false, slabs,
                         (float*)(base + L.dz), &nsl, s));
  if (need_w)
    ASR_TRY(reduce_and_project(slabs, nsl, 9L * C * C, C, dtheta ? theta_dst : nullptr, n_theta, dtheta, dbias,
                               dw_hwio, (float*)(base + L.red), s));
  return ASR_OK;
}

static int check_block_args(const char* fn, int N, int H, int W, int C, int dtype) {
  ASR_TRY(check_shape(N, H, W, C));
  if (dtype != ASR_F32 && dtype != ASR_BF16) return fail(ASR_E_ARG, "%s: bad dtype %d", fn, dtype);
  if (dtype == ASR_BF16 && !mfma_supported(C, W))
    return fail(ASR_E_UNSUPPORTED, "%s: bf16 needs C in {16,32,64} and W == 32 (C=%d W=%d)", fn, C, W);
  return ASR_OK;
}

int asr_rk2_forward(const void* x, void* xmid, void* y, uint8_t* mask1, uint8_t* mask2, const void* w,
                    const float* bias, float h, int N, int H, int W, int C, int dtype, asr_stream_t stream) {
  ASR_TRY(check_block_args("asr_rk2_forward", N, H, W, C, dtype));
  if (!x || !xmid || !y || !w) return fail(ASR_E_ARG, "asr_rk2_forward: null pointer");
  if (x == xmid || x == y || xmid == y) return fail(ASR_E_ARG, "asr_rk2_forward: x, xmid and y must not alias");
  return rk2_forward_impl(x, xmid, y, mask1, mask2, w, bias, h, N, H, W, C, dtype, (hipStream_t)stream);
}

size_t asr_rk2_backward_workspace_bytes(int N, int H, int W, int C, int dtype) {
  if (check_shape(N, H, W, C) != ASR_OK) return 0;
  return bwd_ws_layout(N, H, W, C, dtype, 2).total;
}

int asr_rk2_backward(const void* dy, const void* x, const void* xmid, const uint8_t* mask1, const uint8_t* mask2,
                     const void* w, const int32_t* theta_dst, long n_theta, float h, float gamma, int N, int H, int W,
                     int C, int dtype, void* dx, float* dtheta, float* dbias, float* dw_hwio, void* ws,
                     size_t ws_bytes, asr_stream_t stream) {
  ASR_TRY(check_block_args("asr_rk2_backward", N, H, W, C, dtype));
  if (!dy || !x || !xmid || !mask1 || !mask2 || !w) return fail(ASR_E_ARG, "asr_rk2_backward: null pointer");
  if (dtheta && !theta_dst) return fail(ASR_E_ARG, "asr_rk2_backward: theta_dst needed for dtheta");
  const BwdWs L = bwd_ws_layout(N, H, W, C, dtype, 2);
  if (!ws || ws_bytes < L.total) return fail(ASR_E_WORKSPACE, "asr_rk2_backward: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  unsigned char* base = (unsigned char*)ws;
  float* slabs = (float*)(base + L.slabs);
  const bool need_w = dtheta || dbias || dw_hwio;
  int nsl = 0;
  ASR_TRY(rk2_backward_slabs(dy, x, xmid, mask1, mask2, w, h, gamma, N, H, W, C, dtype, dx, base + L.g, need_w, slabs,
                             (float*)(base + L.dz), &nsl, s));
  if (need_w)
    ASR_TRY(reduce_and_project(slabs, nsl, 9L * C * C, C, dtheta ? theta_dst : nullptr, n_theta, dtheta, dbias,
                               dw_hwio, (float*)(base + L.red), s));
  return ASR_OK;
}

long asr_net_param_count(const asr_net_config* cfg) {
  if (net_check(cfg) != ASR_OK) return -1;
  return net_layout(cfg).nparams;
}

size_t asr_net_workspace_bytes(const asr_net_config* cfg) {
  if (net_check(cfg) != ASR_OK) return 0;
  return net_layout(cfg).total;
}

int asr_net_prepare(const asr_net_config* cfg, void* ws, size_t ws_bytes) {
  ASR_TRY(net_check(cfg));
  const NetLayout L = net_layout(cfg);
  if (!ws || ws_bytes < L.total) return fail(ASR_E_WORKSPACE, "asr_net_prepare: workspace too small");
  ASR_TRY(check_ws_device(ws, "asr_net_prepare"));
  std::vector<int32_t> w_src((size_t)L.E), theta_dst((size_t)L.ntheta * 2);
  ASR_TRY(param_map_k(cfg->C, L.kb, cfg->param_kind, cfg->antisymmetric, w_src.data(), theta_dst.data()));
  unsigned char* b = (unsigned char*)ws;
  if (L.sep_bwd && !L.inference) {
    std::vector<int32_t> w_bwd((size_t)L.E);
    ASR_TRY(param_map_transpose_k(cfg->C, L.kb, w_src.data(), w_bwd.data()));
    ASR_TRY(hip_check(hipMemcpy(b + L.w_src_bwd, w_bwd.data(), w_bwd.size() * 4, hipMemcpyHostToDevice), "hipMemcpy"));
  }
  ASR_TRY(hip_check(hipMemcpy(b + L.w_src, w_src.data(), w_src.size() * 4, hipMemcpyHostToDevice), "hipMemcpy"));
  ASR_TRY(hip_check(hipMemcpy(b + L.theta_dst, theta_dst.data(), theta_dst.size() * 4, hipMemcpyHostToDevice),
                    "hipMemcpy"));
  if (L.stack_pair) {  // the same pull-back from k_bwd3_stack's pair-local D slabs
    std::vector<int32_t> pr(theta_dst.size());
    ASR_TRY(theta_dst_pair_host(theta_dst.data(), L.ntheta, cfg->C, pr.data()));
    ASR_TRY(hip_check(hipMemcpy(b + L.theta_dst_pr, pr.data(), pr.size() * 4, hipMemcpyHostToDevice), "hipMemcpy"));
  }
  if (L.stack_bwd) {  // the same map into k_bwd3_stack's tile-major dW slabs (ASR_VARIANT_FULL_SLABS):
    // entry e = m*C + o of the row-major dW -> ((m/16 * C/16 + o/16) * 64 + 16*((m%16)/4) + o%16) * 4 + m%4
    const int C = cfg->C;
    std::vector<int32_t> tm(theta_dst);
    for (auto& v : tm) {
      if (v < 0) continue;
      const long e = v >> 1, m = e / C, o = e % C;
      const long et = (((m / 16) * (C / 16) + o / 16) * 64 + 16 * ((m % 16) / 4) + o % 16) * 4 + m % 4;
      v = (int32_t)((et << 1) | (v & 1));
    }
    ASR_TRY(hip_check(hipMemcpy(b + L.theta_dst_tm, tm.data(), tm.size() * 4, hipMemcpyHostToDevice), "hipMemcpy"));
  }
  return ASR_OK;
}

int asr_net_forward(const asr_net_config* cfg, const float* params, const void* images, float* probs, void* ws,
                    size_t ws_bytes, asr_stream_t stream) {
  ASR_TRY(net_check(cfg));
  const NetLayout L = net_layout(cfg);
  if (!params || !images || !probs) return fail(ASR_E_ARG, "asr_net_forward: null pointer");
  if (!ws || ws_bytes < L.total) return fail(ASR_E_WORKSPACE, "asr_net_forward: workspace too small");
  ASR_TRY(check_ws_device(ws, "asr_net_forward"));
  hipStream_t s = (hipStream_t)stream;
  unsigned char* b = (unsigned char*)ws;
  unsigned char* xL = nullptr;
  ASR_TRY(net_forward_impl(cfg, L, params, images, false, b, s, &xL));
  ASR_TRY(head(xL, cfg->dtype == ASR_BF16, params + L.off_fck, params + L.off_fcb, nullptr, cfg->N, cfg->H * cfg->W,
               cfg->C, cfg->num_classes, probs, nullptr, nullptr, nullptr, nullptr, s));
  return ASR_OK;
}

int asr_net_check_status(const asr_net_config* cfg, const void* ws, size_t ws_bytes, asr_stream_t stream) {
  ASR_TRY(net_check(cfg));
  const NetLayout L = net_layout(cfg);
  if (!ws || ws_bytes < L.total) return fail(ASR_E_WORKSPACE, "asr_net_check_status: workspace too small");
  ASR_TRY(check_ws_device(ws, "asr_net_check_status"));
  // the stream's own completion status only (hipGetLastError would report, and clear,
  // whatever error another HIP call on this thread left behind)
  return hip_check(hipStreamSynchronize((hipStream_t)stream), "hipStreamSynchronize");
}

int asr_net_kernel_times(float* us) {
  if (!us) return fail(ASR_E_ARG, "asr_net_kernel_times: null output");
  const TimedEvents* t = timed_events_here();
  if (!t || !t->made || !(t->rec & 3u))
    return fail(ASR_E_ARG, "asr_net_kernel_times: no ASR_VARIANT_TIMED call recorded on the current device");
  for (int i = 0; i < 3; ++i) us[i] = -1.f;
  for (int i = 0; i < 3; ++i) {
    const int a = i == 0 ? 0 : i + 1, e = a + 1;
    if ((t->rec >> a & 1u) && (t->rec >> e & 1u)) {
      ASR_TRY(hip_check(hipEventSynchronize(t->ev[e]), "hipEventSynchronize"));
      float ms = 0.f;
      ASR_TRY(hip_check(hipEventElapsedTime(&ms, t->ev[a], t->ev[e]), "hipEventElapsedTime"));
      us[i] = ms * 1e3f;
    }
  }
  return ASR_OK;
}

int asr_net_forward_backward(const asr_net_config* cfg, const float* params, const void* images, const float* targets,
                             float* grads, float* loss, float* probs, void* ws, size_t ws_bytes,
                             asr_stream_t stream) {
  ASR_TRY(net_check(cfg));
  const NetLayout L = net_layout(cfg);
  if (!params || !images || !targets || !grads || !loss) return fail(ASR_E_ARG, "asr_net_forward_backward: null");
  if (!ws || ws_bytes < L.total) return fail(ASR_E_WORKSPACE, "asr_net_forward_backward: workspace too small");
  // before any launch: an inference layout has no backward buffers (its maps for the
  // transposed operator and the training activations are absent)
  if (L.inference)
    return fail(ASR_E_ARG, "asr_net_forward_backward: an ASR_VARIANT_INFERENCE workspace has no training buffers");
  ASR_TRY(check_ws_device(ws, "asr_net_forward_backward"));
  hipStream_t s = (hipStream_t)stream;
  unsigned char* b = (unsigned char*)ws;
  const int C = cfg->C, N = cfg->N, H = cfg->H, W = cfg->W, K = cfg->num_classes;
  const bool bf = cfg->dtype == ASR_BF16;
  const bool stacked = L.stack_bwd && !(cfg->variant & ASR_VARIANT_PER_BLOCK_BWD);
  ASR_TRY(net_forward_impl(cfg, L, params, images, true, b, s));
  auto act = [&](int i) { return b + L.acts + (size_t)i * L.P * L.act_bytes; };
  // head: probabilities, per-image loss, dlogits, dL/dx_L
  unsigned char* dcur = b + L.dxa;
  unsigned char* dnext = b + L.dxb;
  float* probs_ws = probs ? probs : (float*)(b + L.probs);
  // the stacked Euler backward stages its top block's dy from one row per image (the GAP gradient is
  // constant over the pixels): the head writes N x C values instead of the full dL/dx_L tensor
  const bool grow = stacked && !L.rk2 && !(cfg->variant & ASR_VARIANT_FULL_DXL);
  ASR_TRY(head(act(cfg->L), bf, params + L.off_fck, params + L.off_fcb, targets, N, H * W, C, K, probs_ws,
               (float*)(b + L.loss_per), (float*)(b + L.dlogits), (float*)(b + L.gap), grow ? nullptr : dcur, s,
               grow ? b + L.grow : nullptr));
  ASR_TRY(head_param_grads((const float*)(b + L.gap), (const float*)(b + L.dlogits), N, C, K, grads + L.off_fck,
                           grads + L.off_fcb, (const float*)(b + L.loss_per), loss, s));
  // blocks, last to first
  const int32_t* theta_dst = (const int32_t*)(b + L.theta_dst);
  int nsl_blk = 0;
  int dz1_fused = 0;  // dcur holds dz1 = dx1 * [x1 > 0] after the block loop
  const float* pend_slabs = nullptr;  // the slabs whose pass-1 reduction is still pending
  int pend_P = 0;
  float* pend_grp = nullptr;
  const bool fold_on = !(cfg->variant & ASR_VARIANT_NO_FOLD);               // else the reduction as separate launches
  const bool stem_v1 = (cfg->variant & ASR_VARIANT_STEM_WGRAD_VALU) != 0;  // fp32 VALU stem wgrad
  ASR_TRY(timed_event(cfg, 2, s));  // (measurement) the blocks' backward starts
  if (L.deep) {  // C=16: all L blocks in one launch (dx resident in LDS), one slab set per layer
    // (fused_stage_backward's deep16 sequence written out: timed event 3 sits between the kernel and its reductions)
    int rows = 0, in_b = 0;
    float* slabs = (float*)(b + L.deep_slabs);
    ASR_TRY(deep16_backward(dcur, dnext, act(0), L.P, (const uint8_t*)(b + L.masks), L.mask_bytes,
                            b + (L.sep_bwd ? L.wbuf_bwd : L.wbuf), cfg->h, L.sep_bwd ? 0.f : 2.f * cfg->gamma, N,
                            cfg->L, slabs, &rows, &in_b, s));
    ASR_TRY(timed_event(cfg, 3, s));
    if (in_b) std::swap(dcur, dnext);
    const int G = reduce_groups(rows);
    ASR_TRY(reduce_slabs_to_groups(slabs, cfg->L * rows, L.E + C, (float*)(b + L.grp), s));
    ASR_TRY(project_layers((float*)(b + L.grp), (long)G * (L.E + C), G, L.E, C, theta_dst, L.ntheta, cfg->L,
                           grads + L.off_blk, L.blk_stride, s));
    ASR_TRY(timed_event(cfg, 4, s));
  }
  if (stacked) {  // C=64: all L blocks in one launch, tile-major slabs
    const int grid = L.stack_grid;
    const bool pair = L.stack_pair && !(cfg->variant & ASR_VARIANT_FULL_SLABS);
    const long ES = stack_slab_floats(C, pair ? 1 : 0), sst = (long)grid * ES;
    float* slabs = (float*)(b + L.stack_slabs);
    float* grp = (float*)(b + L.grp);
    // (RK2: the first block's first stage has the extra term, so the stem's relu' runs separately)
    const int ro0 = (L.fast_stem || L.stem_kxk) && !stem_v1 && !L.rk2;
    int lfold = cfg->L;
    const uint8_t* m1 = (const uint8_t*)(b + L.masks);
    ASR_TRY(block_stack_bwd_mfma(dcur, dnext, act(0), L.P, m1, L.mask_bytes, b + (L.sep_bwd ? L.wbuf_bwd : L.wbuf),
                                 L.wstride, cfg->h, L.sep_bwd ? 0.f : 2.f * cfg->gamma, N, H, W, C, cfg->L, ro0, slabs,
                                 sst, grp, L.grp_stride, (unsigned*)(b + L.stack_done), &lfold, s,
                                 L.rk2 ? b + L.xmids : nullptr, L.rk2 ? m1 + (size_t)cfg->L * L.mask_bytes : nullptr,
                                 L.rk2 ? b + L.dxg : nullptr, grow ? b + L.grow : nullptr, fold_on ? 1 : 0,
                                 pair ? 1 : 0));
    ASR_TRY(timed_event(cfg, 3, s));
    // pass 1 of the blocks below lfold, and of any block whose in-launch fold was
    // flagged (a workgroup's wait ran out), before the projection reads them
    ASR_TRY(stack_bwd_reduce_rest(slabs, sst, grid, ES, grp, L.grp_stride, cfg->L, lfold,
                                  (const unsigned*)(b + L.stack_done), s));
    if (cfg->L & 1) std::swap(dcur, dnext);
    dz1_fused = ro0;
    ASR_TRY(project_layers(grp, L.grp_stride, reduce_groups(grid), ES - C, C,
                           (const int32_t*)(b + (pair ? L.theta_dst_pr : L.theta_dst_tm)), L.ntheta, cfg->L,
                           grads + L.off_blk, L.blk_stride, s));
    ASR_TRY(timed_event(cfg, 4, s));
  }
  if (L.kxk) {  // k x k blocks: one dgrad and one weight-gradient launch per block, pass 1 of its slabs right behind
    float* slabs_k = (float*)(b + L.bwdws + L.bw.slabs);
    float* dz_k = (float*)(b + L.bwdws + L.bw.dz);
    for (int l = cfg->L - 1; l >= 0; --l) {
      const unsigned char* wl = b + (L.sep_bwd ? L.wbuf_bwd : L.wbuf) + (size_t)l * L.wstride * L.act_bytes;
      const uint8_t* mask = (const uint8_t*)(b + L.masks) + (size_t)l * L.mask_bytes;
      const float two_gamma = L.sep_bwd ? 0.f : 2.f * cfg->gamma;
      int nsl = 0;
      if (bf) {
        ASR_TRY(convk_bf16(B_EULER, L.kb, dcur, dnext, nullptr, wl, nullptr, cfg->h, two_gamma, mask, N, H, W, C, s));
        ASR_TRY(wgradk_bf16(L.kb, act(l), dcur, mask, cfg->h, N, H, W, C, slabs_k, &nsl, s));
      } else {
        ASR_TRY(make_dz(F_EULER, dcur, mask, nullptr, cfg->h, N, H, W, C, 0, dz_k, s));
        ASR_TRY(conv_f32_k(B_EULER, L.kb, dz_k, dnext, nullptr, (const float*)wl, nullptr, cfg->h, two_gamma,
                           (const float*)dcur, N, H, W, C, s, nullptr));
        ASR_TRY(wgrad_f32(act(l), 0, dz_k, N, H, W, C, C, slabs_k, &nsl, s, L.kb));
      }
      if (nsl < 1 || nsl > L.kxk_rows)  // (the device differs from the one the workspace was sized on)
        return fail(ASR_E_WORKSPACE, "k x k block %d wrote %d slab rows, the workspace holds %d", l, nsl, L.kxk_rows);
      ASR_TRY(reduce_slabs_to_groups(slabs_k, nsl, L.E + C, (float*)(b + L.grp) + (size_t)l * L.grp_stride, s));
      nsl_blk = nsl;
      std::swap(dcur, dnext);
    }
  }
  // bf16 off W = 32: convb_backward fuses neither the stem's relu' nor another block's slab reduction (the
  // stem arms below apply relu' themselves, the pending reduction runs as its own launch)
  const bool blk_fuses = !bf || mfma_supported(C, W);
  for (int l = (L.deep || stacked || L.kxk) ? -1 : cfg->L - 1; l >= 0; --l) {
    const unsigned char* wl = b + (L.sep_bwd ? L.wbuf_bwd : L.wbuf) + (size_t)l * L.wstride * L.act_bytes;
    const uint8_t* mask = (const uint8_t*)(b + L.masks) + (size_t)l * L.mask_bytes;
    const float gam = L.sep_bwd ? 0.f : cfg->gamma;
    float* grp_l = (float*)(b + L.grp) + (size_t)l * L.grp_stride;
    // a block's slabs alternate between two buffers; pass 1 of the previous
    // (deeper) block's reduction rides in this block's (second-stage) kernel
    // when it can (else it runs here), and this block's waits for the next
    // block (or the end of the loop)
    // (fp32: every block keeps its own slabs; one launch reduces them all after the loop)
    float* slabs_l = !bf ? (float*)(b + L.slabs_all) + (size_t)l * L.slab_stride
                         : (float*)(b + ((l & 1) ? L.slabs2 : L.bwdws + L.bw.slabs));
    int nsl = 0, folded = 0;
    if (L.rk2) {
      const unsigned char* xm = b + L.xmids + (size_t)l * L.P * L.act_bytes;
      ASR_TRY(rk2_backward_slabs(dcur, act(l), xm, mask, mask + (size_t)cfg->L * L.mask_bytes, wl, cfg->h, gam, N, H,
                                 W, C, cfg->dtype, dnext, b + L.dxg, true, slabs_l, (float*)(b + L.bwdws + L.bw.dz),
                                 &nsl, s, fold_on ? pend_slabs : nullptr, fold_on ? pend_P : 0, pend_grp, &folded));
    } else {
      ASR_TRY(block_backward(ASR_MODE_EULER, dcur, act(l), mask, wl, cfg->h, gam, N, H, W, C, cfg->dtype, dnext, true,
                             nullptr, false, slabs_l, (float*)(b + L.bwdws + L.bw.dz), &nsl, s,
                             l == 0 && (L.fast_stem || L.stem_kxk) && bf && !stem_v1 && blk_fuses,
                             l == 0 ? &dz1_fused : nullptr, fold_on && blk_fuses ? pend_slabs : nullptr,
                             fold_on && blk_fuses ? pend_P : 0, pend_grp, &folded));
    }
    nsl_blk = nsl;
    std::swap(dcur, dnext);
    if (!bf) {
      if (nsl > L.stages * L.f32_rows)  // (the device differs from the one the workspace was sized on)
        return fail(ASR_E_WORKSPACE, "fp32 block %d wrote %d slab rows, the workspace holds %d (sized on another device?)",
                    l, nsl, L.stages * L.f32_rows);
      continue;
    }
    if (pend_P > 0 && !folded) ASR_TRY(reduce_slabs_to_groups(pend_slabs, pend_P, L.E + C, pend_grp, s));
    pend_slabs = slabs_l;
    pend_P = nsl;
    pend_grp = grp_l;
  }
  if (pend_P > 0) ASR_TRY(reduce_slabs_to_groups(pend_slabs, pend_P, L.E + C, pend_grp, s));
  if (!bf && !L.deep && !stacked && !L.kxk && nsl_blk > 0)  // (every block of a network has the same slab count)
    ASR_TRY(reduce_slab_layers((const float*)(b + L.slabs_all), L.slab_stride, nsl_blk, L.E + C,
                               (float*)(b + L.grp), L.grp_stride, cfg->L, s));
  // pass 2 of every block's weight-gradient reduction + projection onto theta, one launch
  if (!L.deep && !stacked) {
    ASR_TRY(timed_event(cfg, 3, s));  // (per-block kernels: their slab passes ride inside)
    ASR_TRY(project_layers((float*)(b + L.grp), L.grp_stride, reduce_groups(nsl_blk), L.E, C, theta_dst, L.ntheta,
                           cfg->L, grads + L.off_blk, L.blk_stride, s));
    ASR_TRY(timed_event(cfg, 4, s));
  }
  // stem: dz1 = dx1 * [x1 > 0]; conv1 weight/bias gradient from the normalised input
  const long E1 = (long)L.k1 * L.k1 * cfg->Cin * C;
  float* dz = (float*)(b + L.bwdws + L.stem.dz);
  float* slabs = (float*)(b + L.bwdws + L.stem.slabs);
  float* red = (float*)(b + L.bwdws + L.stem.red);
  int nsl = 0;
  const float inv_std = cfg->use_norm ? 1.f / cfg->divide_by_stddev : 1.f;
  if (L.fast_stem && bf && !dz1_fused && !stem_v1 && stem_wgrad_mfma_supported(cfg->Cin, H, W, C) && L.P % 8 == 0) {
    ASR_TRY(relu_grad_bf16(dcur, act(0), L.P, s));
    dz1_fused = 1;
  }
  if (L.stem_kxk && !stem_v1) {  // the k x k conv1 on the matrix cores, from dz1 in bf16
    if (!dz1_fused) ASR_TRY(relu_grad_bf16(dcur, act(0), L.P, s));
    ASR_TRY(stem_wgrad_kxk(L.k1, images, cfg->input_u8, dcur, N, H, W, cfg->Cin, C, cfg->subtract_mean, inv_std,
                           cfg->use_norm, slabs, &nsl, s));
  } else if (L.fast_stem && dz1_fused && stem_wgrad_mfma_supported(cfg->Cin, H, W, C)) {
    ASR_TRY(stem_wgrad_mfma(images, cfg->input_u8, dcur, N, H, W, cfg->Cin, C, cfg->subtract_mean, inv_std,
                            cfg->use_norm, slabs, &nsl, s));
  } else if (L.fast_stem) {  // (masking an already-masked dz1 again is exact)
    ASR_TRY(stem_wgrad(images, cfg->input_u8, dcur, act(0), bf, N, H, W, cfg->Cin, C, cfg->subtract_mean, inv_std,
                       cfg->use_norm, slabs, &nsl, s));
  } else {
    // (the forward left x0 there unless the matrix-core k x k stem ran it)
    if (L.stem_kxk && !(cfg->variant & ASR_VARIANT_STEM_FWD_VALU)) ASR_TRY(net_normalize(cfg, L, images, b, s));
    ASR_TRY(make_dz(F_RELU, dcur, nullptr, act(0), 1.f, N, H, W, C, bf ? 1 : 0, dz, s));
    ASR_TRY(wgrad_f32(b + L.x0, 0, dz, N, H, W, cfg->Cin, C, slabs, &nsl, s, L.k1));
  }
  ASR_TRY(reduce_and_project(slabs, nsl, E1, C, nullptr, 0, nullptr, grads + L.off_c1b, grads + L.off_c1k, red, s));
  return ASR_OK;
}

int asr_segment_sq_norms(const float* x, const long* offsets, int n_segments, float* out, asr_stream_t stream) {
  if (!x || !offsets || !out || n_segments < 0) return fail(ASR_E_ARG, "asr_segment_sq_norms: bad arguments");
  if (n_segments == 0) return ASR_OK;
  hipLaunchKernelGGL(k_segment_sq_norms, dim3(n_segments), dim3(256), 0, (hipStream_t)stream, x, offsets, out);
  ASR_LAUNCH_CHECK("k_segment_sq_norms");
  return ASR_OK;
}

int asr_batch_metrics(const float* probs, const float* targets, const float* loss, int N, int K, float* accum,
                      asr_stream_t stream) {
  if (!probs || !targets || !accum || N < 1 || K < 1) return fail(ASR_E_ARG, "asr_batch_metrics: bad args");
  hipLaunchKernelGGL(k_batch_metrics, dim3(1), dim3(256), 0, (hipStream_t)stream, probs, targets, loss, N, K, accum);
  ASR_LAUNCH_CHECK("k_batch_metrics");
  return ASR_OK;
}

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

}  // extern "C"
