/*
 * asr.h — C ABI of libasr.so, the MI355X-native hot path of the
 * antisymmetric-ResNet (pierluigiferrari/differential_equations_resnet).
 *
 * One Euler block of the reference is
 *     x_{n+1} = x_n + h * relu(conv3x3(x_n, W(theta)) + b)
 * (models/tfkeras_resnets.py:69-92) where W(theta) is re-materialised from the
 * layer's free parameters on every step
 * (layers/tfkeras_layer_Conv2DAntisymmetric3By3.py:85-171).
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a device pointer unless
 *     the comment says "host";
 *   - activations NHWC, kernels HWIO [3][3][C_in][C_out] (reference layout);
 *   - stream contract (enforced by tests/test_gpu_streams.py on the GPU and by
 *     tests/test_streams_cpu.py over the sources): every call is a stateless
 *     launch on the caller's stream: every kernel launch and asynchronous copy
 *     of a call is issued on the stream it was passed and nowhere else.  No
 *     call synchronises or allocates (workspaces are caller-owned, sized by
 *     the *_workspace_bytes queries), apart from the entry points marked
 *     "blocking; not capturable" (asr_net_prepare, asr_stages_prepare,
 *     asr_net_check_status, asr_net_kernel_times, asr_stack_status, and the
 *     asr_debug_* readers).  Every other call may therefore run on any stream
 *     beside other work and be recorded into a HIP graph and replayed;
 *   - every entry point returns 0 on success and a negative ASR_E* code on
 *     failure; asr_last_error() returns a thread-local message.  Nothing
 *     throws across the ABI;
 *   - buffer contract (every section below restates its part; enforced by
 *     tests/test_gpu_buffers.py): what an output or a workspace holds before a
 *     call is irrelevant (no call reads a byte of them that it has not written
 *     itself), relu masks need not be pre-zeroed, and no byte outside the
 *     documented size of any buffer, input or output, is read or written.
 *
 * Each declaration cites the reference interface it replaces.
 */
#ifndef ASR_H_
#define ASR_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* asr_stream_t; /* a hipStream_t (0 = null stream) */

/* error codes */
#define ASR_OK 0
#define ASR_E_ARG (-1)         /* invalid argument (shape, dtype, null)       */
#define ASR_E_UNSUPPORTED (-2) /* valid but not implemented on this device    */
#define ASR_E_WORKSPACE (-3)   /* workspace too small                          */
#define ASR_E_HIP (-4)         /* HIP runtime error (see asr_last_error)       */
#define ASR_E_DEVICE (-5)      /* no usable gfx950 device                      */

/* activation dtypes */
#define ASR_F32 0
#define ASR_BF16 1

/* parametrisations of the antisymmetric kernel (what theta means) */
#define ASR_PARAM_3BY3 0    /* Conv2DAntisymmetric3By3: a,b,c,d then
                               input_kernels_for_output_kernel_{o}[3,3,C-o-1]
                               (…3By3.py:104-141, :219-245)                   */
#define ASR_PARAM_GENERAL 1 /* Conv2DAntisymmetric (kernel_size 3): per o the
                               centro_sym_{i}_{j} scalars then
                               input_kernels_for_output_kernel_{o}[3,3,C-o-1,1]
                               (…Conv2DAntisymmetric.py:109-145)              */
#define ASR_PARAM_REGULAR 2 /* plain Conv2D kernel [3,3,C,C] (the regular
                               identity block, tfkeras_resnets.py:76-83):
                               theta IS W in HWIO order                       */

/* block integrators (asr_net_config.integrator) */
#define ASR_INTEGRATOR_EULER 0
#define ASR_INTEGRATOR_RK2 1

/* conv modes */
#define ASR_MODE_EULER 0 /* y = x + h*relu(conv(x)+b); mask = [conv(x)+b > 0]
                            (tfkeras_resnets.py:69-92)                        */
#define ASR_MODE_CONV 1  /* y = conv(x) + b  (the layer's call(),
                            …3By3.py:157-171)                                 */

const char* asr_last_error(void);
int asr_abi_version(void);

/* Number of gfx950 compute units of the current device (0 on failure). */
int asr_device_cu_count(void);

/* ------------------------------------------------------------------------
 * Parametrisation (host-side, pure arithmetic)
 * --------------------------------------------------------------------- */

/* Number of free kernel parameters (no bias).  3BY3: 4C + 9C(C-1)/2.
 * Replaces the add_weight calls of …3By3.py:119-124, :219-245 and
 * …Conv2DAntisymmetric.py:123-128, :234-239. */
long asr_theta_count(int C, int kind, int antisymmetric);

/* Host: fill the element map of W(theta).
 *   w_src[e] for every HWIO element e = ((ky*3+kx)*C+i)*C+o:
 *      (j<<1)|neg  => W[e] = (neg ? -1 : +1) * theta[j]
 *      -1          => W[e] = gamma (non-trainable centre, …3By3.py:248-250)
 *   theta_dst[2*j+0], theta_dst[2*j+1]: the (<=2) W elements theta[j] feeds,
 *      encoded (e<<1)|neg, -1 if unused.  This is the pull-back used for the
 *      weight-gradient projection (autodiff of …3By3.py:115-141).
 * w_src: 9*C*C int32, theta_dst: 2*asr_theta_count int32 (host memory). */
int asr_param_map(int C, int kind, int antisymmetric, int32_t* w_src, int32_t* theta_dst);

/* Host: 1 if the operator A of this parametrisation satisfies
 * A + A^T = 2*gamma*I (3by3, general with antisymmetric=1), else 0; <0 on
 * bad arguments.  For such kinds the backward pass applies A^T with the
 * forward W (asr_conv_backward's identity).  Otherwise the caller
 * materialises the transposed operator W_bwd = -flip(W)^T from the map
 * asr_param_map_transpose returns, with asr_theta_to_w_mirror, and passes it
 * (with gamma 0) as the backward's w. */
int asr_param_is_antisymmetric(int kind, int antisymmetric);
int asr_param_map_transpose(int C, const int32_t* w_src, int32_t* w_src_bwd);
/* Host: the pull-back of an antisymmetric parametrisation (C = 64) from the
 * pair-local slabs of the stacked backward (asr_block_stack_backward, the
 * network's C=64 bf16 backward): every theta's entries (e, mirror(e)) of
 * theta_dst (asr_param_map) become 1 or 2 entries (s << 1 | neg) into a slab
 * of 74 16x16 tiles of D = dW - dW*^T (dW*[t][i][o] = dW[8-t][o][i]): tile
 * 16p + 4a + b holds D(tap p < 4, input tile a, output tile b); 64 + k the
 * tap-4 cross pair k; 70 + c tap 4's self tile c (raw, transposed for odd c);
 * element (r, c) of tile T at T*256 + ((r/4)*16 + c)*4 + r%4.  ASR_E_ARG when
 * some theta is not an antisymmetric pair. */
int asr_param_map_pair(int C, const int32_t* theta_dst, long n_theta, int32_t* theta_dst_pair);

/* Elements of the packed bf16 W consumed by the MFMA kernels. */
long asr_wpack_elems(int C);

/* Materialise W for L layers in one launch (replaces the per-step
 * slice/neg/concat/stack graph of …3By3.py:113-141).
 *   theta:  layer l's theta at theta + l*theta_stride (float32)
 *   w_src:  device copy of asr_param_map's w_src
 *   dtype == ASR_BF16: w_out (bf16) gets the MFMA fragment-packed layout,
 *                      layer l at l*w_stride elements.  Balanced rounding
 *                      (C <= 64, maps that pair every off-diagonal entry with
 *                      its antisymmetric partner: the 3by3 and general kinds):
 *                      each pair takes the bf16 neighbour that keeps every
 *                      output channel's sum of rounding errors near zero, so
 *                      W stays exactly antisymmetric and no channel carries a
 *                      fixed offset through a deep stack; otherwise round to
 *                      nearest.  Deterministic; restated bit-exactly by
 *                      tests/helpers.py w_bf16_balanced;
 *   dtype == ASR_F32:  w_out (float) gets plain HWIO [3][3][C][C].
 * Buffers: every element of every layer of w_out is written whatever it held;
 * with strides above a layer's size the elements between layers are neither
 * read (theta) nor written (w_out). */
int asr_theta_to_w(const float* theta, long theta_stride, int L, int C, const int32_t* w_src,
                   float gamma, void* w_out, long w_stride, int dtype, asr_stream_t stream);

/* (ABI 13) The backward's W of an operator that is not antisymmetric:
 * W_bwd = -flip(W)^T of the W that asr_theta_to_w gives for the same theta
 * (gamma plays no part: such a map has no constant entries).
 *   w_src_bwd: device copy of asr_param_map_transpose's map of the forward map;
 *   every other argument as in asr_theta_to_w.
 * ASR_F32, and ASR_BF16 where asr_theta_to_w rounds to nearest: the same as
 * asr_theta_to_w on w_src_bwd with gamma 0 (round to nearest even commutes
 * with negation and with the permutation).  ASR_BF16 with balanced rounding:
 * the pairs take the forward pack's decisions (the error sums start from the
 * forward's diagonal errors, not from their negation), so that every entry is
 * bit for bit the negated entry of the forward pack at the flipped tap and
 * swapped channels; asr_theta_to_w on w_src_bwd rounds about a quarter of the
 * entries to the other neighbour, and a backward with it is the gradient of a
 * slightly different forward.  The caller states that the map is a transpose
 * by calling this function; nothing is inferred from the map. */
int asr_theta_to_w_mirror(const float* theta, long theta_stride, int L, int C, const int32_t* w_src_bwd,
                          void* w_out, long w_stride, int dtype, asr_stream_t stream);

/* ------------------------------------------------------------------------
 * Fused antisymmetric 3x3 conv / Euler block
 * --------------------------------------------------------------------- */

/* Forward.  mode ASR_MODE_EULER: y = x + h*relu(conv(x,W)+b), mask written;
 * ASR_MODE_CONV: y = conv(x,W)+b (mask may be NULL).
 *   x, y: [N,H,W,C] in dtype;  w: output of asr_theta_to_w for dtype;
 *   bias: C floats or NULL;  mask: asr_mask_bytes(N,H,W,C) bytes, relu bit of
 *   element (pixel, o) at bit index pixel*C + o (NHWC bit order, LSB first).
 * float32 takes any shape.  bfloat16 (forward, backward and the stack calls
 * below) takes C in {16, 32, 64, 128, 256} (ABI 12: 128 and 256) and W == 8 or
 * W a multiple of 16 (the MFMA tile is 16 pixels of one row), any H: k_convb /
 * k_wgradb over whole rows at W in {32, 16, 8}, over column strips of 32
 * pixels from W = 48 on; at C in {128, 256} the same items on k_convbw (W
 * streamed from its pack) and k_wgradbw (the weight gradient over 64 x 64
 * channel blocks).  Any other bf16 shape is ASR_E_UNSUPPORTED before any
 * launch.  asr_theta_to_w's bf16 pack rounds W to nearest above C = 64 (the
 * balanced rounding is C <= 64): an antisymmetric W stays exactly
 * antisymmetric, and deep stacks at C >= 128 carry the per-channel offset of
 * nearest rounding that ASR_VARIANT_W_BF16 describes (not measured at these
 * widths).  asr_conv_backward_workspace_bytes stays <= 64 MB at C >= 128 for
 * every N, H, W (the weight gradient writes at most 48 MB of slabs).
 * Replaces Conv2DAntisymmetric3By3.call (…3By3.py:157-171) and
 * single_layer_identity_block's relu/scale/add (tfkeras_resnets.py:89-92).
 * Buffers: y and every byte of mask up to asr_mask_bytes (padding bits
 * included) are overwritten whatever they held, mask need not be pre-zeroed,
 * and nothing outside x, w, bias, y and mask at their documented sizes is
 * read or written. */
int asr_conv_forward(int mode, const void* x, void* y, uint8_t* mask, const void* w,
                     const float* bias, float h, int N, int H, int W, int C, int dtype,
                     asr_stream_t stream);

long asr_mask_bytes(int N, int H, int W, int C);

/* Backward of asr_conv_forward (the autodiff of training.py:300 through the
 * block).  Given dy = dL/dy:
 *   EULER: dz = h*dy*mask;  dx = dy + A^T dz = dy - conv(dz,W) + 2*gamma*dz
 *   CONV:  dz = dy;         dx = A^T dz      =    - conv(dz,W) + 2*gamma*dz
 *   dW = sum_p patch(x) (x) dz, projected onto theta through theta_dst
 *   (device copy of asr_param_map's theta_dst); db = sum_p dz.
 * dtheta / dbias / dx may be NULL to skip that output; dw_hwio (float
 * [3][3][C][C], may be NULL) receives the unprojected dW.
 * ws: caller workspace of asr_conv_backward_workspace_bytes bytes.
 * Buffers: the contents of ws and of the outputs before the call are
 * irrelevant (the slab reduction reads exactly the rows this call wrote), each
 * requested output is the same bits whichever others are requested, and
 * nothing outside the documented sizes (ws: the queried bytes) is read or
 * written.  The same holds for the stack calls declared next: with strides
 * larger than a layer, the bytes between consecutive layers are neither read
 * nor written. */
/* A stack of L Euler blocks in one call (the deep-stack path, BASELINE
 * config C3: single_layer_identity_block applied L times,
 * tfkeras_resnets.py:579-582).  Layer l reads x_l (x0 for l = 0) and writes
 * x_{l+1} to ys + l*y_stride elements and its relu mask to masks +
 * l*mask_stride bytes (masks may be NULL); with store_all == 0 only x_L is
 * written, to ys.  w: layer l's asr_theta_to_w output at w + l*w_stride
 * elements; bias: layer l's at bias + l*bias_stride (may be NULL).  bf16 at
 * C=16, H=W=32 runs all L steps in one launch with every image resident in
 * LDS; bf16 at C=64, W=32 (store_all) runs all L steps in one launch with
 * whole images per workgroup; the image-resident stage shapes (bf16 at
 * 16x16x32, 8x8x64 and 8x8x32, fp32 at 16x16x32 and 8x8x64; H == W) run all L
 * steps in one launch with a workgroup per image, when store_all != 0 and
 * bias and masks are both given (without one of them the per-block sequence
 * runs).  On that path the strides must keep every layer's vector accesses
 * aligned, else ASR_E_ARG before any launch: y_stride % 4, mask_stride % 2,
 * bias_stride % 4 and, in bf16, w_stride % 8.  Other shapes (bf16: C in
 * {16,32,64,128,256}, W == 8 or W % 16 == 0) run the per-block kernels in
 * sequence. */
int asr_block_stack_forward(const void* x0, void* ys, long y_stride, uint8_t* masks, long mask_stride,
                            const void* w, long w_stride, const float* bias, long bias_stride, float h,
                            int N, int H, int W, int C, int L, int dtype, int store_all, asr_stream_t stream);

/* Backward of asr_block_stack_forward over all L blocks: dyL = dL/dx_L;
 * xs: x_l at xs + l*x_stride elements (x_0 first, i.e. the stack's input
 * followed by its stored outputs); masks / w as the forward.  dx0 receives
 * dL/dx_0; dparams (may be NULL) layer l's [dtheta (n_theta) | dbias (C)] at
 * dparams + l*(n_theta + C), projected through theta_dst.  bf16 at C=16,
 * H=W=32 runs one fused launch with dx resident in LDS (w_stride must be
 * asr_wpack_elems(16)); bf16 at C=64, W=32 runs one launch over all blocks
 * (whole images per workgroup, weight-gradient slabs reduced in-launch);
 * the image-resident stage shapes of asr_block_stack_forward run one launch
 * for the input gradients (a workgroup per image) and, with dparams, one for
 * every layer's weight gradient (x_stride % 8 and w_stride % 8 in bf16,
 * x_stride % 4 in fp32, else ASR_E_ARG before any launch); other shapes run
 * asr_conv_backward per block.  The operator is the antisymmetric one: the
 * forward's w with A^T = -A + 2*gamma*I. */
size_t asr_block_stack_backward_workspace_bytes(int N, int H, int W, int C, int L, int dtype);
int asr_block_stack_backward(const void* dyL, const void* xs, long x_stride, const uint8_t* masks, long mask_stride,
                             const void* w, long w_stride, const int32_t* theta_dst, long n_theta, float h,
                             float gamma, int N, int H, int W, int C, int L, int dtype, void* dx0, float* dparams,
                             void* ws, size_t ws_bytes, asr_stream_t stream);

size_t asr_conv_backward_workspace_bytes(int N, int H, int W, int C, int dtype);
int asr_conv_backward(int mode, const void* dy, const void* x, const uint8_t* mask,
                      const void* w, const int32_t* theta_dst, long n_theta, float h,
                      float gamma, int N, int H, int W, int C, int dtype, void* dx,
                      float* dtheta, float* dbias, float* dw_hwio, void* ws, size_t ws_bytes,
                      asr_stream_t stream);

/* ------------------------------------------------------------------------
 * Conv2DAntisymmetric(kernel_size = k) for odd k != 3
 * (layers/tfkeras_layer_Conv2DAntisymmetric.py:60-68, 109-145, 163-170):
 * the same operator family on a k x k kernel (k = 3 is the functions above).
 * fp32 (the reference's precision; bf16 for k = 5 and 7: the next section);
 * W HWIO [k,k,C,C]; maps of k*k*C*C entries.  The antisymmetric kinds keep A^T = -A + 2 gamma I, so
 * asr_conv_backward_k takes the forward W (else W_bwd of
 * asr_param_map_transpose_k with gamma 0), as asr_conv_backward.
 * Buffers as asr_conv_forward / asr_conv_backward: prior contents of outputs,
 * mask and ws are irrelevant, mask need not be pre-zeroed, nothing outside the
 * documented sizes is read or written.
 * ---------------------------------------------------------------------- */
long asr_theta_count_k(int C, int kernel_size, int kind, int antisymmetric);
int asr_param_map_k(int C, int kernel_size, int kind, int antisymmetric, int32_t* w_src, int32_t* theta_dst);
int asr_param_map_transpose_k(int C, int kernel_size, const int32_t* w_src, int32_t* w_src_bwd);
int asr_theta_to_w_k(const float* theta, long theta_stride, int L, int C, int kernel_size, const int32_t* w_src,
                     float gamma, float* w_out, long w_stride, asr_stream_t stream);
int asr_conv_forward_k(int mode, int kernel_size, const float* x, float* y, uint8_t* mask, const float* w,
                       const float* bias, float h, int N, int H, int W, int C, asr_stream_t stream);
size_t asr_conv_backward_workspace_bytes_k(int N, int H, int W, int C, int kernel_size);
int asr_conv_backward_k(int mode, int kernel_size, const float* dy, const float* x, const uint8_t* mask,
                        const float* w, const int32_t* theta_dst, long n_theta, float h, float gamma, int N, int H,
                        int W, int C, float* dx, float* dtheta, float* dbias, float* dw, void* ws, size_t ws_bytes,
                        asr_stream_t stream);

/* ------------------------------------------------------------------------
 * The same layer in bf16 (ABI 9): bf16 activations and W, fp32 accumulation,
 * on v_mfma_f32_16x16x32_bf16, both modes, forward and backward.
 * Supported set: kernel_size in {5, 7}, C in {16, 32, 64}, W in {8, 16, 32},
 * any H >= 1 and N >= 1; every other odd kernel_size 1..15 or shape returns
 * ASR_E_UNSUPPORTED (use the fp32 functions above).
 *   asr_wpack_elems_k: elements of one layer's packed W, (C/16)*KS*512 with
 *     KS = ceil(k*k*C / 32); < 0 outside the supported set.
 *   asr_theta_to_w_k_bf16: the 3x3 pack's layout with 9 replaced by k*k: the
 *     element of output channel o and reduction index kappa = tap*C + i
 *     (tap = ky*k + kx) sits at
 *       (((o/16)*KS + kappa/32)*64 + o%16 + 16*((kappa%32)/8))*8 + kappa%8,
 *     zero for kappa >= k*k*C; layer l at w_pack + l*w_stride elements.
 *     Rounded to nearest even (not the 3x3 pack's balanced rounding), so an
 *     antisymmetric W stays exactly antisymmetric off the diagonal and the
 *     pack of asr_param_map_transpose_k's map is bit for bit -flip(W)^T of
 *     the forward pack.
 *   asr_conv_forward_k_bf16 / asr_conv_backward_k_bf16: as the fp32 pair, x /
 *     y / dy / dx bf16 [N,H,W,C], w one layer's pack, mask in the layout of
 *     asr_conv_forward.  EULER's dz = h*(dy & mask): the mask is applied to the
 *     bf16 dy exactly and h in fp32 (the weight gradients' sums, the dx terms).
 *     dw (may be NULL) receives the unprojected dW, float [k][k][C][C].
 *   asr_conv_backward_workspace_bytes_k_bf16: weight-gradient slabs of
 *     k*k*C*C + C floats and their reduction rows; the slab count is bounded by
 *     48 MB of slabs and by 256, so the workspace stays <= 64 MB for every
 *     supported shape (49.8 MB at k = 7, C = 64: 59 slabs of 803 KB); 0
 *     outside the supported set.
 *   Buffers as the fp32 pair: prior contents of outputs, mask, w_pack and ws
 *     are irrelevant (asr_theta_to_w_k_bf16 writes the pack's zero padding
 *     itself and, with w_stride above a layer's elements, leaves the bytes
 *     between layers alone), nothing outside the documented sizes is read or
 *     written.
 * ---------------------------------------------------------------------- */
long asr_wpack_elems_k(int C, int kernel_size);
int asr_theta_to_w_k_bf16(const float* theta, long theta_stride, int L, int C, int kernel_size, const int32_t* w_src,
                          float gamma, void* w_pack, long w_stride, asr_stream_t stream);
int asr_conv_forward_k_bf16(int mode, int kernel_size, const void* x, void* y, uint8_t* mask, const void* w,
                            const float* bias, float h, int N, int H, int W, int C, asr_stream_t stream);
size_t asr_conv_backward_workspace_bytes_k_bf16(int N, int H, int W, int C, int kernel_size);
int asr_conv_backward_k_bf16(int mode, int kernel_size, const void* dy, const void* x, const uint8_t* mask,
                             const void* w, const int32_t* theta_dst, long n_theta, float h, float gamma, int N, int H,
                             int W, int C, void* dx, float* dtheta, float* dbias, float* dw, void* ws, size_t ws_bytes,
                             asr_stream_t stream);

/* ------------------------------------------------------------------------
 * RK2 (explicit midpoint) block — an EXTENSION, not in the reference
 * (BASELINE.json config 5; the reference integrates with forward Euler,
 * tfkeras_resnets.py:69-92).  Same W and bias in both stages:
 *   xmid = x + (h/2)*relu(conv(x,W)+b)      mask1 = [conv(x,W)+b > 0]
 *   y    = x + h*relu(conv(xmid,W)+b)       mask2 = [conv(xmid,W)+b > 0]
 * Each stage is the fused Euler kernel (the second takes its residual from x).
 * xmid and both masks are kept for the backward; masks may be NULL for
 * inference.  Buffers: prior contents of xmid, y, the masks (not pre-zeroed),
 * the backward's outputs and its ws are irrelevant; nothing outside the
 * documented sizes is read or written (asr_rk2_stack_* likewise).
 * --------------------------------------------------------------------- */
int asr_rk2_forward(const void* x, void* xmid, void* y, uint8_t* mask1, uint8_t* mask2, const void* w,
                    const float* bias, float h, int N, int H, int W, int C, int dtype,
                    asr_stream_t stream);

/* Backward of asr_rk2_forward: dz2 = h*dy*mask2, g = A^T dz2,
 * dz1 = (h/2)*g*mask1, dx = dy + g + A^T dz1; dW = patch(x) (x) dz1 +
 * patch(xmid) (x) dz2 projected onto theta; db = sum(dz1 + dz2).
 * Outputs as asr_conv_backward; ws of asr_rk2_backward_workspace_bytes. */
size_t asr_rk2_backward_workspace_bytes(int N, int H, int W, int C, int dtype);
int asr_rk2_backward(const void* dy, const void* x, const void* xmid, const uint8_t* mask1,
                     const uint8_t* mask2, const void* w, const int32_t* theta_dst, long n_theta,
                     float h, float gamma, int N, int H, int W, int C, int dtype, void* dx,
                     float* dtheta, float* dbias, float* dw_hwio, void* ws, size_t ws_bytes,
                     asr_stream_t stream);

/* A stack of L RK2 blocks in one call (config 5's network path): block l reads
 * x_l (x0 for l = 0), writes x_mid_l to xmids + l*y_stride and x_{l+1} to
 * ys + l*y_stride elements, mask1 / mask2 of block l to masks1 / masks2 +
 * l*mask_stride bytes; w, bias as asr_block_stack_forward.  bf16 at C=64,
 * W=32 (>= 4 row bands per image) runs all 2L stages in one launch; other
 * shapes return ASR_E_UNSUPPORTED. */
int asr_rk2_stack_forward(const void* x0, void* ys, void* xmids, long y_stride, uint8_t* masks1, uint8_t* masks2,
                          long mask_stride, const void* w, long w_stride, const float* bias, long bias_stride, float h,
                          int N, int H, int W, int C, int L, int dtype, asr_stream_t stream);

/* Backward of asr_rk2_stack_forward: dyL = dL/dx_L; x_l at xs + l*x_stride
 * (x_0 first), x_mid_l at xmids + l*x_stride; dx0, dparams as
 * asr_block_stack_backward.  One launch over all blocks' two stages (bf16,
 * C=64, W=32). */
size_t asr_rk2_stack_backward_workspace_bytes(int N, int H, int W, int C, int L, int dtype);
int asr_rk2_stack_backward(const void* dyL, const void* xs, const void* xmids, long x_stride, const uint8_t* masks1,
                           const uint8_t* masks2, long mask_stride, const void* w, long w_stride,
                           const int32_t* theta_dst, long n_theta, float h, float gamma, int N, int H, int W, int C,
                           int L, int dtype, void* dx0, float* dparams, void* ws, size_t ws_bytes,
                           asr_stream_t stream);

/* ------------------------------------------------------------------------
 * Whole single-block network (get_single_block_resnet_build_function,
 * tfkeras_resnets.py:511-604, antisymmetric, num_stages=2, strides (1,1),
 * no BN/pooling):  normalise -> conv1+relu -> L Euler blocks -> GAP ->
 * Dense(num_classes, softmax); loss = mean Keras categorical cross-entropy
 * on the probabilities (training.py:295).
 * Parameters are ONE float32 buffer in Keras get_weights() order:
 *   conv1 kernel [3,3,Cin,C], conv1 bias [C],
 *   L x (theta [asr_theta_count(C, param_kind, antisymmetric)], bias [C]),
 *   fc kernel [C,K], fc bias [K].
 * C and num_classes above 256 return ASR_E_UNSUPPORTED (the head runs one
 * 256-thread workgroup per image), as asr_stages_check does.
 * Buffers: a workspace holds nothing a step depends on but what
 * asr_net_prepare uploaded and what the step itself wrote before reading it
 * (the masks and slab rows carved from it are never assumed zero), so a step
 * gives the same bits on a fresh, a recycled or a just-used workspace; grads,
 * loss and probs are overwritten; nothing outside asr_net_workspace_bytes and
 * the documented sizes is read or written.
 * --------------------------------------------------------------------- */
typedef struct asr_net_config {
  int N, H, W, Cin, C, L, num_classes;
  float h, gamma;
  float subtract_mean, divide_by_stddev; /* applied when use_norm != 0   */
  int use_norm;
  int dtype;    /* activation dtype: ASR_F32 or ASR_BF16                */
  int input_u8; /* images are uint8 (1) or float32 (0), NHWC            */
  int param_kind;    /* ASR_PARAM_3BY3 / _GENERAL / _REGULAR of the blocks */
  int antisymmetric; /* Conv2DAntisymmetric(antisymmetric=...); 1 otherwise */
  int integrator;    /* ASR_INTEGRATOR_EULER (the reference's block) or
                        ASR_INTEGRATOR_RK2 (extension, asr_rk2_forward)     */
  int variant;       /* 0 = the production kernel composition; ASR_VARIANT_*
                        bits select slower, independently written kernels
                        for the same math (cross-checks in the tests)      */
  /* ABI 10 (trailing, so a zero-filled tail means the 3 x 3 network): */
  int kernel_size;       /* the blocks' kernel size: 0 (= 3), 3, 5 or 7     */
  int conv1_kernel_size; /* conv1's kernel size:     0 (= 3), 3, 5 or 7     */
} asr_net_config;
/* Accepted kernel sizes (everything else is refused before any launch, with
 * this set in asr_last_error(): ASR_E_ARG for an even or non-positive size
 * and for the 3by3 kind with kernel_size != 3, ASR_E_UNSUPPORTED otherwise):
 *   - float32: conv1_kernel_size and kernel_size in {3, 5, 7} at any shape the
 *     float32 network takes; kernel_size != 3 needs ASR_PARAM_GENERAL or
 *     ASR_PARAM_REGULAR (Conv2DAntisymmetric(kernel_size), a regular Conv2D);
 *   - bfloat16, kernel_size in {5, 7}: the set of asr_conv_forward_k_bf16,
 *     C in {16, 32, 64} and W in {8, 16, 32}, any H;
 *   - bfloat16, kernel_size 3: C in {16, 32, 64, 128, 256} and W == 8 or
 *     W % 16 == 0 (asr_conv_forward's bf16 set), for any conv1_kernel_size.
 *     W == 32 at C <= 64 runs what it ran before; any other width, and every
 *     width at C in {128, 256}, runs one launch per block, forward
 *     and backward (Euler blocks only), conv1 on the VALU / generic arms and
 *     the variant bits PER_BLOCK_*, NO_FOLD, FULL_DXL, FULL_SLABS have no
 *     effect there;
 *   - ASR_INTEGRATOR_RK2 needs kernel_size 3 (any conv1_kernel_size) and, in
 *     bfloat16, W == 32 and C in {16, 32, 64};
 *   - ASR_VARIANT_INFERENCE works for every accepted config.
 * With both sizes 0 or 3 every call launches what it launched at ABI 9.
 * kernel_size != 3 runs one launch per block, forward and backward (the
 * kernels of asr_conv_forward_k / _k_bf16; W(theta) of all L layers in one
 * asr_theta_to_w_k / _k_bf16 launch, bf16 rounded to nearest); the variant
 * bits PER_BLOCK_*, NO_FOLD, FULL_DXL, FULL_SLABS and W_BF16 have no effect
 * there.  conv1_kernel_size != 3: bfloat16 networks with Cin = 3, C in
 * {16, 32, 64} and W in {8, 16, 32} run conv1 and its weight gradient on
 * the matrix cores (k_stem_fwd_kxk / k_stem_wgrad_kxk: the 3 x 3 stem's
 * arithmetic, bf16 (v - mean) against inv_std * W1 as bf16 hi + lo, fp32
 * sums); float32 networks, other shapes and ASR_VARIANT_STEM_FWD_VALU /
 * _STEM_WGRAD_VALU run a normalisation pass and the generic fp32 k x k conv /
 * weight gradient.
 * Parameter layout: conv1 kernel [k1,k1,Cin,C]; a block's theta count is
 * asr_theta_count_k(C, kernel_size, param_kind, antisymmetric). */

/* asr_net_config.variant bits (all 0 in production) */
#define ASR_VARIANT_NO_FOLD 1      /* reduce every block's weight-gradient slabs in
                                      its own launch instead of folding the pass
                                      into the next block's backward kernel; the
                                      C=64 stacked backward then has no in-launch
                                      hand-off (a cross-check arm: without it a
                                      missed hand-off degrades gracefully)       */
#define ASR_VARIANT_STEM_FWD_VALU 2 /* bf16 stem forward on the fp32 VALU kernel
                                       (conv1_kernel_size != 3: the generic one) */
#define ASR_VARIANT_STEM_WGRAD_VALU 4 /* stem weight gradient on the fp32 VALU
                                        kernel from dx1 and x1 (relu' not fused
                                        into the first block's backward)       */
#define ASR_VARIANT_PER_BLOCK_FWD 8 /* C=64 bf16 training forward: one k_fwd3
                                       launch per block instead of the single
                                       all-blocks k_fwd3_stack launch         */
#define ASR_VARIANT_PER_BLOCK_BWD 16 /* C=64 bf16 Euler backward: one k_bwd3 launch
                                        per block (slab pass folded into the
                                        next one) instead of k_bwd3_stack     */
#define ASR_VARIANT_INFERENCE 32  /* forward-only workspace: x_0 and two ping-pong
                                     activation slots, no masks / backward
                                     buffers (asr_net_forward only; the C=64 bf16
                                     blocks run as one k_fwd3_stack launch)     */
#define ASR_VARIANT_TIMED 64      /* record HIP events around the block launches
                                     (measurement; asr_net_kernel_times)       */
#define ASR_VARIANT_FULL_DXL 128  /* C=64 bf16 Euler stacked backward: the head
                                     writes dL/dx_L as a full [N,H,W,C] tensor
                                     that the top block reads, instead of the
                                     per-image row it is constant over
                                     (cross-check of the synthesised dy)        */
#define ASR_VARIANT_FULL_SLABS 256 /* C=64 bf16 stacked backward of an antisymmetric
                                      operator: publish the full dW (144 tiles per
                                      workgroup slab) instead of the pair-local
                                      D = dW - dW*^T (74 tiles) the projection
                                      needs (cross-check and A/B arm)           */
#define ASR_VARIANT_W_BF16 512    /* bf16 networks: W rounded to nearest bf16
                                     instead of asr_theta_to_w's balanced
                                     rounding.  Same speed; the nearest
                                     rounding offsets every output channel by
                                     a fixed sum that every pixel of every
                                     layer sees, and over C3's 108 blocks that
                                     reaches 2.7e-2 relative L2 of a block's
                                     gradient vs the fp32 reference
                                     (tests/test_gpu_depth.py)    */

long asr_net_param_count(const asr_net_config* cfg);
size_t asr_net_workspace_bytes(const asr_net_config* cfg);
/* One-time setup of a workspace (uploads the parameter maps with synchronous
 * copies: blocking; not capturable). */
int asr_net_prepare(const asr_net_config* cfg, void* ws, size_t ws_bytes);
/* probs: [N, K] float (softmax outputs, the Model's output). */
int asr_net_forward(const asr_net_config* cfg, const float* params, const void* images,
                    float* probs, void* ws, size_t ws_bytes, asr_stream_t stream);
/* One training forward+backward: targets [N,K] float (one-hot);
 * grads: same layout as params (overwritten); loss: 1 float (batch mean);
 * probs may be NULL. */
int asr_net_forward_backward(const asr_net_config* cfg, const float* params, const void* images,
                             const float* targets, float* grads, float* loss, float* probs,
                             void* ws, size_t ws_bytes, asr_stream_t stream);
/* Host, blocking; not capturable (synchronises the stream): ASR_OK, or ASR_E_HIP with the
 * runtime's error when work on the stream failed (the stream's status only:
 * a pending error of another HIP call on this thread is neither reported nor
 * cleared).  (Since ABI 6 a missed
 * in-launch hand-off of the C=64 stacked backward is not an error: it costs
 * speed, see asr_stack_status.) */
int asr_net_check_status(const asr_net_config* cfg, const void* ws, size_t ws_bytes, asr_stream_t stream);

/* Host, blocking; not capturable (waits for the events of that call): device
 * times in microseconds of the last asr_net_forward /
 * asr_net_forward_backward called with ASR_VARIANT_TIMED: us[0] the L blocks'
 * forward (the single stack launch where one runs), us[1] the L blocks'
 * backward kernels (the single stack launch k_bwd3_stack / k_bwd16_fused
 * where one runs), us[2] the weight-gradient reductions left after them and
 * the projection onto theta; -1 for a part that call did not run. */
int asr_net_kernel_times(float* us);

/* Host, blocking; not capturable (allocates, and copies device to host on the
 * current device): the number of
 * degraded in-launch slab hand-offs of the C=64 stacked backward (k_bwd3_stack)
 * since the last reset, >= 0 (or a negative error code).  A workgroup whose
 * bounded wait (~1-2 ms) for the other workgroups' weight-gradient slabs of a
 * block runs out flags that block and stops waiting for the rest of its
 * launch; the flagged blocks' slab reduction is then recomputed after the
 * launch, on the same stream, before the projection: the gradients are those
 * of the full hand-off, only slower (e.g. a grid that is not co-resident
 * because another kernel or process shares the device).  reset != 0 clears
 * the count in the same device atomic that reads it (a backward running on
 * another stream meanwhile loses no count). */
int asr_stack_status(int reset);
/* Test knob: force the stacked backward's grid (0: one workgroup per CU;
 * larger than the resident capacity makes hand-offs run out and degrade, see
 * asr_stack_status).  Workspace sizes depend on the grid: query them after
 * setting it. */
int asr_debug_stack_backward(int grid);

/* ------------------------------------------------------------------------
 * Multi-stage single-block ResNet (ABI 7): get_single_block_resnet_build_function
 * with num_stages > 2 (models/tfkeras_resnets.py:547-597), e.g. the He-style
 * ResNet-32: conv1 (3x3 'same', stride 1) + relu, then stages of identity Euler
 * blocks at 32^2 x 16, 16^2 x 32, 8^2 x 64; a stage whose filters or stride
 * change opens with single_layer_conv_block (tfkeras_resnets.py:204-269):
 *     y = relu(conv_3x3(x, K2, stride) + b2) + conv_1x1(x, K1, stride) + b1
 * (the 3x3 'same' with TF's asymmetric stride padding, the 1x1 'valid'), then
 * GAP + Dense softmax.  fp32 (the reference's precision); no BN / pooling.
 * Buffers as the single-block network: prior contents of outputs, masks and
 * workspaces (the transition's and asr_stages_workspace_bytes) are irrelevant,
 * and nothing outside the documented sizes is read or written.
 * ---------------------------------------------------------------------- */

/* The transition alone.  x [N,H,W,Ci] -> y [N,Ho,Wo,Co], Ho = ceil(H/stride);
 * k2 HWIO [3,3,Ci,Co], k1 [1,1,Ci,Co]; mask: N*Ho*Wo*Co bytes, 1 where
 * conv_3x3 + b2 > 0 (may be NULL).  Replaces single_layer_conv_block's
 * Conv2D '2' / '1' + relu + add (tfkeras_resnets.py:238-269). */
int asr_transition_forward(const float* x, float* y, uint8_t* mask, const float* k2, const float* b2,
                           const float* k1, const float* b1, int N, int H, int W, int Ci, int Co, int stride,
                           asr_stream_t stream);
/* Its backward: dx = dL/dx (may be NULL); dparams (may be NULL): the
 * gradients [dK2 | db2 | dK1 | db1] contiguous (the parameter order of
 * asr_stages_config). */
size_t asr_transition_backward_workspace_bytes(int N, int H, int W, int Ci, int Co, int stride);
int asr_transition_backward(const float* dy, const float* x, const uint8_t* mask, const float* k2, const float* k1,
                            int N, int H, int W, int Ci, int Co, int stride, float* dx, float* dparams, void* ws,
                            size_t ws_bytes, asr_stream_t stream);

#define ASR_STAGES_MAX 8
typedef struct asr_stages_config {
  int N, H, W, Cin, num_classes;
  int n_stages;               /* identity-block stages (the reference's num_stages - 1) */
  int C[ASR_STAGES_MAX];      /* filters of stage s (C[0] = conv1's filters)           */
  int L[ASR_STAGES_MAX];      /* identity blocks of stage s (>= 0)                     */
  int stride[ASR_STAGES_MAX]; /* s > 0: the opening transition's stride (1 or 2), 0 =
                                 no transition (then C[s] == C[s-1]); stride[0] = 0   */
  float h, gamma;
  float subtract_mean, divide_by_stddev; /* applied when use_norm != 0 */
  int use_norm, input_u8, param_kind, antisymmetric;
  int dtype;                  /* ABI 8: ASR_F32 (0) or ASR_BF16: the identity blocks'
                                 activations and convs (bf16 MFMA, fp32 accumulation
                                 and weight gradients); the transitions compute in fp32 */
} asr_stages_config;
/* params / grads (float32): conv1 kernel [3,3,Cin,C0], bias [C0]; per stage s:
 * the transition (if any) K2 [3,3,C[s-1],C[s]], b2, K1 [1,1,C[s-1],C[s]], b1,
 * then L[s] x (theta [asr_theta_count(C[s], param_kind, antisymmetric)], bias
 * [C[s]]); fc kernel [C_last, K], bias [K]. */
/* ASR_OK, or the code (and asr_last_error) the calls below fail with for this
 * config: ASR_E_ARG for a malformed one, ASR_E_UNSUPPORTED for a shape the
 * kernels do not take (e.g. a bf16 stage with blocks outside C {16,32,64,128,256} x
 * {W == 8 or W % 16 == 0}: asr_conv_forward's bf16 set; such stages run one
 * launch per block off the fused stage shapes).
 * ABI 8.  Host only. */
int asr_stages_check(const asr_stages_config* cfg);
long asr_stages_param_count(const asr_stages_config* cfg);
size_t asr_stages_workspace_bytes(const asr_stages_config* cfg);
/* One-time setup of a workspace (uploads every stage's parameter maps with
 * synchronous copies: blocking; not capturable). */
int asr_stages_prepare(const asr_stages_config* cfg, void* ws, size_t ws_bytes);
int asr_stages_forward(const asr_stages_config* cfg, const float* params, const void* images, float* probs,
                       void* ws, size_t ws_bytes, asr_stream_t stream);
int asr_stages_forward_backward(const asr_stages_config* cfg, const float* params, const void* images,
                                const float* targets, float* grads, float* loss, float* probs, void* ws,
                                size_t ws_bytes, asr_stream_t stream);

/* tf.train.AdamOptimizer.apply_gradients (training.py:300-301), TF1
 * epsilon-hat form; step is the 1-based update count; g is multiplied by
 * grad_scale first (1/world for data-parallel mean). */
int asr_adam_update(float* params, const float* grads, float* m, float* v, long n, float lr,
                    float beta1, float beta2, float eps, long step, float grad_scale,
                    asr_stream_t stream);

/* The tf.keras.optimizers of TF 1.12 (Keras 2.1.6-tf) behind Model.compile /
 * fit: one launch per update whatever the optimiser, fp32, no host
 * synchronisation.  Additional exports of ABI 12; asr_adam_update is unchanged.
 * With g = grads * grad_scale:
 *   SGD      v = momentum*m - lr*g;  m <- v;
 *            p <- p + momentum*v - lr*g with ASR_OPT_NESTEROV, else p <- p + v
 *   Adam     lr_t = lr*sqrt(1 - beta_2^step)/(1 - beta_1^step) (host, double);
 *            m <- beta_1 m + (1 - beta_1) g;  v <- beta_2 v + (1 - beta_2) g^2;
 *            with ASR_OPT_AMSGRAD  vhat <- max(vhat, v), p <- p - lr_t m/(sqrt(vhat) + eps),
 *            else p <- p - lr_t m/(sqrt(v) + eps): the bits of asr_adam_update
 *   RMSprop  a <- rho a + (1 - rho) g^2;  p <- p - lr g/(sqrt(a) + eps)
 * Keras' decay is the host's: it passes lr = lr0 / (1 + decay * iterations).
 * Buffers: params and state are read-modify-write over exactly n and slots * n
 * floats, grads is read over n; nothing outside them is read or written
 * (asr_adam_update likewise). */
enum { ASR_OPT_SGD = 0, ASR_OPT_ADAM = 1, ASR_OPT_RMSPROP = 2 };
enum { ASR_OPT_NESTEROV = 1 /* SGD */, ASR_OPT_AMSGRAD = 2 /* Adam */ };
typedef struct asr_optimizer_config {
  int kind, flags;
  float lr;         /* the host has already applied Keras' decay */
  float a, b;       /* SGD: momentum, -;  Adam: beta_1, beta_2;  RMSprop: rho, - */
  float eps;
  long step;        /* 1-based update count (Adam's bias correction); >= 1 */
  float grad_scale; /* g is multiplied by it first (1/world) */
} asr_optimizer_config;
/* Host only: the n-float state buffers the optimiser needs (SGD 1: m; Adam 2:
 * m, v; Adam + AMSGRAD 3: m, v, vhat; RMSprop 1: a), or -1 for an unknown kind
 * or a flag that does not belong to the kind. */
int asr_optimizer_slots(int kind, int flags);
/* state: [slots][n] floats, caller-owned, zero-initialised before the first
 * update.  ASR_E_ARG before any launch for a null pointer, n < 0, step < 1, an
 * unknown kind or a flag that does not belong to the kind; n == 0 is ASR_OK. */
int asr_optimizer_update(const asr_optimizer_config* cfg, float* params, const float* grads,
                         float* state, long n, asr_stream_t stream);

/* Weight regularisers of the same surface (additional exports of ABI 12):
 * Keras' l2 (tf.keras.regularizers.l2, which Model.fit adds to the loss it
 * trains and reports) and the smoothness-in-depth penalty of Haber & Ruthotto,
 * "Stable architectures for deep neural networks", R = 1/(2h) sum_j ||K_j -
 * K_{j-1}||^2, over a table of segments of the flat parameter buffer.  A
 * segment is `layers` runs of `count` floats, layer_stride floats apart (one
 * run for a plain variable; a stack of identity blocks has its thetas, and
 * its biases, at the stride n_theta + C).  With p_l[j] float j of layer l:
 *   R     = sum over segments of  l2 * sum p^2
 *                               + smooth * sum_{l>=1} sum_j (p_l[j] - p_{l-1}[j])^2
 *   dR/dp_l[j] = 2 l2 p_l[j] + 2 smooth ((p_l - p_{l-1})[j] [l > 0]
 *                                        + (p_l - p_{l+1})[j] [l < layers - 1])
 * asr_regularize, with grads:   grads[i] += dR/dp[i] / grad_scale for every
 *   covered float i (grad_scale is what the optimiser launch will multiply g
 *   by, 1/world or 1: the update sees dR once, so the call goes after the
 *   all-reduce); grads == NULL is the forward-only form of evaluation;
 * with loss_inout:  *loss_inout += R;   with penalty_out:  *penalty_out = R.
 * Floats no segment covers (the biases between two layers' thetas when
 * layer_stride > count) are neither read for R nor written in grads, and
 * nothing outside params / grads / the workspace / the two scalars is touched.
 *
 * Contract, as for every call of this header: no allocation, no host
 * synchronisation, every launch on `stream` (capturable into a HIP graph),
 * prior workspace contents irrelevant.  Two launches at most (one without
 * loss_inout and penalty_out) whatever n_segments is; none for n_segments ==
 * 0, which is ASR_OK.  R and dR are formed in fp64 from the fp32 parameters;
 * the workgroups' partial sums of R are stored in the workspace and summed
 * in a fixed order (no floating-point atomics), so R and grads are bitwise
 * reproducible for equal arguments (the workspace size included: one
 * workgroup runs per 8 bytes of it, at most 1024).  Accesses are 16 bytes
 * wide where offset, count and layer_stride are multiples of 4 floats (count
 * free for layers == 1) and params / grads are 16-byte aligned.
 *
 * `segments` of asr_regularize is a DEVICE copy of the table, which the call
 * cannot inspect: the caller checks the host table once with
 * asr_regularize_check before uploading it.  That returns ASR_E_ARG (the
 * segment named in asr_last_error) for n_segments outside 0..256; count < 1,
 * layers < 1 or layer_stride < count; a segment that ends beyond n_params; a
 * negative or non-finite coefficient; two segments whose covered floats
 * overlap (segments may interleave: thetas and biases at one stride).
 * asr_regularize itself returns ASR_E_ARG for n_segments outside 0..256, a
 * null segments / params or, with grads, a grad_scale that is not finite and
 * positive, and ASR_E_WORKSPACE for a workspace below 8 bytes or not 8-byte
 * aligned (any size from 8 bytes on computes the same sums, slower). */
typedef struct asr_reg_segment {
  long offset;       /* first float of layer 0 in the flat parameter buffer   */
  long count;        /* floats per layer                                      */
  long layer_stride; /* layer l starts at offset + l*layer_stride (>= count)  */
  int layers;        /* >= 1; 1 for a plain variable                          */
  float l2;          /* Keras l2(l):  R += l2 * sum p^2                       */
  float smooth;      /* R += smooth * sum_{l>=1} sum_j (p_l[j] - p_{l-1}[j])^2 */
} asr_reg_segment;
#define ASR_REG_MAX_SEGMENTS 256
/* Host only. */
int asr_regularize_check(const asr_reg_segment* host_segments, int n_segments, long n_params);
/* Host only: 0 for n_segments outside 1..256 or n_params < 0. */
size_t asr_regularize_workspace_bytes(int n_segments, long n_params);
int asr_regularize(const asr_reg_segment* segments, int n_segments, const float* params, float* grads,
                   float grad_scale, float* loss_inout, float* penalty_out, void* ws, size_t ws_bytes,
                   asr_stream_t stream);

/* ------------------------------------------------------------------------
 * Training-loop metrics, accumulated on the device (no per-step host sync).
 * ---------------------------------------------------------------------- */

/* out[i] = sum_{j in [offsets[i], offsets[i+1])} x[j]^2 for i < n_segments
 * (offsets: device int64 [n_segments+1]).  The per-layer gradient
 * mean-norm ||g|| / size of training.py:356-409 is sqrt(out[i]) / size. */
int asr_segment_sq_norms(const float* x, const long* offsets, int n_segments, float* out,
                         asr_stream_t stream);

/* Streaming mean loss + accuracy (tf.metrics.mean / tf.metrics.accuracy,
 * training.py:316-354): accum[0] += *loss, accum[1] += #{argmax probs ==
 * argmax targets}, accum[2] += N, accum[3] += 1.  loss may be NULL: the
 * batch-mean Keras categorical cross-entropy of probs is used (evaluation). */
int asr_batch_metrics(const float* probs, const float* targets, const float* loss, int N, int K,
                      float* accum, asr_stream_t stream);

/* ------------------------------------------------------------------------
 * Device-side image augmentation (ABI 11): the reference's dataset
 * preprocessors (dataset_utils/tf_dataset_preprocessors_image_classification.py:
 * RandomCrop, Resize, ResizeWithPad, RandomFlipLeftRight, RandomBrightness,
 * RandomSaturation) applied while a batch is gathered from the dataset array
 * in HBM: one launch per batch does gather by index -> crop -> bilinear resize
 * (or resize with zero padding) -> left-right flip -> colour operations, with
 * no intermediate tensor and no host synchronisation.  Nothing random happens
 * on the device: the host draws one asr_aug_item per output image and the
 * kernel applies it, so the batch is a pure function of the table.
 *
 * Semantics are those of the TF 1.12 calls the reference makes:
 *   crop      output window [y0, y0+ch) x [x0, x0+cw) of source row src
 *             (tf.image.random_crop);
 *   resize    tf.image.resize_images, bilinear, align_corners=False, legacy
 *             coordinates: output index d reads source coordinate
 *             s = d * (in / out), lo = floor(s), hi = min(lo + 1, in - 1),
 *             f = s - lo; top = tl + (tr - tl) * fx, bottom likewise,
 *             out = top + (bottom - top) * fy; float32 arithmetic, float32
 *             output on the input's scale (0..255 from uint8);
 *   pad       tf.image.resize_image_with_pad: the window resized to rh x rw
 *             sits at (pad_top, pad_left) of the Ho x Wo output, zeros
 *             elsewhere (the caller computes the extent and offsets);
 *   flip      output column x reads column Wo - 1 - x; with flip_src the
 *             crop window's columns are mirrored before the resize instead
 *             (a flip listed before the resize: the legacy coordinates are
 *             not symmetric, so the two differ);
 *   brightness  tf.image.adjust_brightness: float32 x + delta, unclipped;
 *             uint8 x * (1/255) + delta, then back as convert_image_dtype
 *             (saturate): * 255.5, clamp to [0, 255], truncate;
 *   saturation  tf.image.adjust_saturation, 3 channels: v = max(r,g,b),
 *             range = v - min(r,g,b), s = v > 0 ? range / v : 0; for
 *             range > 0, n = 1 / (6 range) and h = n (g - b) if r == v, else
 *             n (b - r) + 2/6 if g == v, else n (r - g) + 4/6, h += 1 if
 *             h < 0 (h = 0 for range <= 0); s <- clip(s * factor, 0, 1);
 *             c = s v, m = v - c, d = 6 h, x = c (1 - |d mod 2 - 1|),
 *             k = int(d) mod 6: (r,g,b) = m + (c,x,0), (x,c,0), (0,c,x),
 *             (0,x,c), (x,0,c), (c,0,x) for k = 0..5.  uint8 images go
 *             through the same [0, 1] conversion and back, per operation.
 * Output dtype: uint8 when the source is uint8 and no resize runs, float32
 * otherwise.
 * ---------------------------------------------------------------------- */
#define ASR_U8 2 /* image dtype of the augmentation (with ASR_F32) */

#define ASR_AUG_RESIZE_NONE 0     /* Ho x Wo is the crop window itself         */
#define ASR_AUG_RESIZE_BILINEAR 1 /* window ch x cw -> Ho x Wo                 */
#define ASR_AUG_RESIZE_PAD 2      /* window ch x cw -> rh x rw inside Ho x Wo  */

#define ASR_AUG_NONE 0
#define ASR_AUG_BRIGHTNESS 1
#define ASR_AUG_SATURATION 2

/* One output image's parameters (32 bytes; a device array of N of them). */
typedef struct asr_aug_item {
  int32_t src;        /* row of the dataset array                             */
  int32_t y0, x0;     /* crop window origin in the source image              */
  int32_t ch, cw;     /* crop window size (ignored without a resize: Ho, Wo) */
  int32_t flip;       /* 0 or 1                                               */
  float brightness;   /* the delta                                            */
  float saturation;   /* the factor                                           */
} asr_aug_item;

/* One call's description (host). */
typedef struct asr_aug_plan {
  int Hs, Ws, Cch;    /* source images [n_src, Hs, Ws, Cch]; Cch 1 or 3      */
  int src_dtype;      /* ASR_U8 or ASR_F32                                    */
  int Ho, Wo;         /* output images [N, Ho, Wo, Cch]                       */
  int dst_dtype;      /* ASR_U8 (uint8 source, no resize) or ASR_F32          */
  int resize;         /* ASR_AUG_RESIZE_*                                     */
  int rh, rw;         /* ASR_AUG_RESIZE_PAD: the resized extent ...           */
  int pad_top, pad_left; /* ... and its offset in the output                 */
  int flip_src;       /* mirror the crop window, not the output (see above)   */
  int color[2];       /* ASR_AUG_* in the order they run; ASR_AUG_NONE skips  */
} asr_aug_plan;

/* dst[i] = augment(src[items[i].src], items[i]) for i < N, on the caller's
 * stream.  src: the dataset array (n_src rows); dst: 16-B aligned.
 * Checked on the host before any launch: null pointers, N < 1, sizes < 1, a
 * window (no resize: Ho x Wo) larger than the source, a padded extent outside
 * the output, an unknown resize mode or colour operation and a dst_dtype other
 * than the rule above give ASR_E_ARG; a channel count other than 1 or 3,
 * saturation on one channel, an unknown dtype and 2^31 or more output pixels
 * give ASR_E_UNSUPPORTED with the value in asr_last_error().
 * The device table is NOT validated on the host (no synchronisation): items
 * must hold 0 <= src < n_src and windows inside the source.  The kernel clamps
 * src, the window size and its origin into the array, so a bad table gives
 * wrong pixels, never an access outside src.
 * Buffers: every byte of dst (the zero border of a padded resize included) is
 * written whatever it held; nothing outside src, items and dst is read or
 * written. */
int asr_augment_batch(const void* src, long n_src, const asr_aug_plan* plan, const asr_aug_item* items, int N,
                      void* dst, asr_stream_t stream);

/* ------------------------------------------------------------------------
 * Data-parallel collectives (RCCL over xGMI; one process per GPU).  NEW: the
 * reference is single-device (experiments_antisymmetric_resnet_v6.ipynb:361);
 * SURVEY.md §8(e) adds one all-reduce of the flat fp32 gradient buffer per
 * step (the batch is split by image: no BatchNorm, batch-mean loss,
 * training.py:295) and one broadcast of the initial parameters.
 * ---------------------------------------------------------------------- */
#define ASR_DIST_UNIQUE_ID_BYTES 128

/* Host: rank 0 creates the communicator id (out: 128 host bytes) and hands
 * it to every rank out of band (file, TCP store, ...). */
int asr_dist_unique_id(void* out);
/* Host, blocking, collective over all ranks: create this process's
 * communicator on the current HIP device. */
int asr_dist_init(int rank, int world, const void* unique_id);
/* In place on the caller's stream: buf = sum over ranks (dtype ASR_F32/BF16). */
int asr_dist_allreduce_sum(void* buf, size_t count, int dtype, asr_stream_t stream);
/* In place on the caller's stream: buf = root's buf. */
int asr_dist_broadcast(void* buf, size_t count, int dtype, int root, asr_stream_t stream);
/* World size of the live communicator (0 when none). */
int asr_dist_world_size(void);
/* Destroy the communicator (no-op without one). */
int asr_dist_finalize(void);

#ifdef __cplusplus
}
#endif
#endif /* ASR_H_ */
