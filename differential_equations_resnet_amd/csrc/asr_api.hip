// The layer-level C ABI (include/asr.h): conv, RK2 block and block-stack forward/backward dispatch
// (asr_conv_*, asr_rk2_*, asr_block_stack_*, asr_*_k, asr_*_k_bf16), the fused-stage host sequences
// both executors share, and the batch metrics.  The network executors built on it are asr_net.hip
// (single stage) and asr_stages.hip (multi-stage).
#include <math.h>

#include "asr_common.h"
#include "asr_internal.h"

namespace asr {
// the shapes of the bf16 3 x 3 block kernels on the matrix cores at W = 32
bool mfma_supported(int C, int W) { return (C == 16 || C == 32 || C == 64) && W == 32; }

int check_shape(int N, int H, int W, int C) {
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
BwdWs bwd_ws_layout(int N, int H, int W, int C, int dtype, int stages, int K, int slab_rows) {
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

// One conv application's backward: dx = [dy] + extra + A^T dz and the
// weight-gradient slabs (written at `slabs`, count in *nsl).
//   EULER: dz = h*dy*mask; CONV: dz = dy.  skip_dy drops the +dy residual of
//   EULER (the second RK2 stage); extra (nullable) is added to dx (the first
//   RK2 stage adds the step's outer dy).
int block_backward(int mode, const void* dy, const void* x, const uint8_t* mask, const void* w, float h, float gamma,
                   int N, int H, int W, int C, int dtype, void* dx, bool need_w, const void* extra, bool skip_dy,
                   float* slabs, float* dz_scratch, int* nsl, hipStream_t s, bool relu_dx, int* relu_done,
                   const float* fold_slabs, int fold_P, float* fold_grp, int* fold_done, bool accum_slabs) {
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
int rk2_forward_impl(const void* x, void* xmid, void* y, uint8_t* mask1, uint8_t* mask2, const void* w,
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
int rk2_backward_slabs(const void* dy, const void* x, const void* xmid, const uint8_t* mask1, const uint8_t* mask2,
                       const void* w, float h, float gamma, int N, int H, int W, int C, int dtype, void* dx, void* g,
                       bool need_w, float* slabs, float* dz_scratch, int* nsl, hipStream_t s, const float* fold_slabs,
                       int fold_P, float* fold_grp, int* fold_done) {
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

}  // extern "C"
