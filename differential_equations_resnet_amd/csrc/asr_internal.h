// Host functions and constants shared between the libasr translation units:
// every function that one .hip file defines and another calls is declared
// here, once, with its default arguments, under the file that defines it.
// Every .hip file includes this header, the defining one too, so a signature
// that drifts from its definition does not compile.  (Only set_error and fail
// of asr_theta.hip sit in asr_common.h, whose inline hip_check calls fail.)
#pragma once
#include "asr_common.h"

namespace asr {

// conv modes of the 3x3 block kernels (asr_conv_f32.hip: conv_f32's fmode, the dispatch of asr_api.hip and
// asr_net.hip; asr_conv_bf16.hip)
enum { F_EULER = 0, F_CONV = 1, F_RELU = 2, B_EULER = 3, B_CONV = 4 };

// Most weight-gradient slabs one launch writes: the grid bound of the block and
// stack kernels and of stem_wgrad_mfma (asr_block_mfma.hip), and the slab rows
// the workspaces reserve per block (asr_api.hip, asr_net.hip).
constexpr int kMaxBlockSlabs = 512;
// The name for code about the stem's weight gradient: stem_wgrad's grid bound
// (asr_stem_head.hip), the stem slab rows of the multi-stage workspace
// (asr_stages.hip).  One value with the block cap, not a second choice: both
// stem launchers fill the same areas, stem_wgrad_mfma bounded by the block cap
// and stem_wgrad by this one, and the single-stage workspace sizes its stem
// slabs by the block cap, the multi-stage one by this one.
constexpr int kMaxStemSlabs = kMaxBlockSlabs;

// ---- asr_theta.hip ---------------------------------------------------------
// compute units of the current device; 0 when the query fails (asr_device_cu_count reports that)
int cu_count();
// the same for sizing a grid or a workspace: where the query fails, an MI355X's 256
inline int launch_cus() { const int cus = cu_count(); return cus > 0 ? cus : 256; }
// p[0 .. words) = 0 (32-bit words, p 4-byte aligned) by a kernel on s.  Not hipMemsetAsync: recorded into a HIP
// graph, its memset node was seen to run out of order with the work enqueued before the replay
// (tests/test_gpu_streams.py: relu masks keeping bits of their previous contents), a kernel node is not.
int zero_words(void* p, long words, hipStream_t s);
// A network / stage workspace must live on the current device: its layout (the
// weight-gradient slab rows, hence every offset after them) follows the CU
// count of the device current when it was sized, and the kernels size their
// grids by the device current at launch.  ASR_E_WORKSPACE, before any launch,
// when ws is not device memory of the current device.
int check_ws_device(const void* ws, const char* who);
long theta_count(int C, int kind, int antisymmetric);
int param_map(int C, int kind, int antisymmetric, int32_t* w_src, int32_t* theta_dst);
int param_is_antisymmetric(int kind, int antisymmetric);
int param_map_transpose(int C, const int32_t* w_src, int32_t* w_bwd);
// the same for a k x k layer (odd k; the 3by3 kind has k = 3 only)
long theta_count_k(int C, int k, int kind, int antisymmetric);
int param_map_k(int C, int k, int kind, int antisymmetric, int32_t* w_src, int32_t* theta_dst);
int param_map_transpose_k(int C, int k, const int32_t* w_src, int32_t* w_bwd);
// One launch of the balanced bf16 weight pack for several layer sets (PackJob, asr_common.h)
constexpr int kMaxPackJobs = 16;
int theta_to_w_bf16_jobs(const PackJob* jobs, int njobs, hipStream_t s);
int theta_to_w_bf16(const float* theta, long theta_stride, int L, int C, const int32_t* w_src, float gamma, void* w,
                    long w_stride, bool balance, hipStream_t s, const int32_t* theta_dst = nullptr,
                    long n_theta = 0, bool mirror = false);
int reduce_and_project(const float* slabs, int P, long E, int Cb, const int32_t* theta_dst, long n_theta,
                       float* dtheta, float* dbias, float* dw_out, float* ws, hipStream_t s);
size_t reduce_ws_bytes(int P, long ES);
int reduce_groups(int P);
int reduce_slabs_to_groups(const float* slabs, int P, long ES, float* grp, hipStream_t s);
int reduce_slab_layers(const float* slabs, long slab_stride, int P, long ES, float* grp, long grp_stride, int L,
                       hipStream_t s);
int project_layers(float* grp, long grp_stride, int G, long E, int Cb, const int32_t* theta_dst, long n_theta,
                   int L, float* out, long out_stride, hipStream_t s);
int theta_dst_pair(const int32_t* in, long n_theta, int C, int32_t* out, hipStream_t s);
int theta_dst_pair_host(const int32_t* in, long n_theta, int C, int32_t* out);

// ---- asr_block_mfma.hip ----------------------------------------------------
int block_fwd_mfma(int mode, const void* x, const void* resid, void* y, uint8_t* mask, const void* w,
                   const float* bias, float h, int N, int H, int W, int C, hipStream_t s);
// relu_dx (optional): dx *= [x > 0] when the kernel supports it (*relu_done = 1).
// fold_* (optional): pass 1 of another slab set's reduction (fold_P slabs ->
// reduce_groups(fold_P) group rows at fold_grp), folded into the kernel when
// it supports it (*fold_done = 1); else the caller reduces them itself.
int block_bwd_mfma(int mode, const void* dy, const void* x, const uint8_t* mask, const void* w, float h,
                   float two_gamma, int N, int H, int W, int C, void* dx, float* slabs, int* nslabs, const void* extra,
                   int skip_dy, hipStream_t s, int relu_dx = 0, int* relu_done = nullptr,
                   const float* fold_slabs = nullptr, int fold_P = 0, float* fold_grp = nullptr,
                   int* fold_done = nullptr, int accum = 0);
int stem_wgrad_mfma(const void* img, int input_u8, const void* dz1, int N, int H, int W, int Cin, int C, float mean,
                    float inv_std, int use_norm, float* slabs, int* nslabs, hipStream_t s);
bool stem_wgrad_mfma_supported(int Cin, int H, int W, int C);
int stem_fwd_mfma(const void* img, int input_u8, const float* w1, const float* b1, int N, int H, int W, int Cin, int C,
                  float mean, float inv_std, int use_norm, void* out, hipStream_t s);
bool stem_fwd_mfma_supported(int Cin, int H, int W, int C);
// the 5 x 5 / 7 x 7 conv1 of the bf16 networks: Cin = 3, C in {16, 32, 64}, W in {8, 16, 32}, any H
bool stem_kxk_supported(int K, int Cin, int W, int C);
int stem_fwd_kxk(int K, const void* img, int input_u8, const float* w1, const float* b1, int N, int H, int W, int Cin,
                 int C, float mean, float inv_std, int use_norm, void* out, hipStream_t s);
int stem_wgrad_kxk(int K, const void* img, int input_u8, const void* dz1, int N, int H, int W, int Cin, int C,
                   float mean, float inv_std, int use_norm, float* slabs, int* nslabs, hipStream_t s);
bool block_stack_fwd_supported(int N, int H, int W, int C);
int block_stack_fwd_mfma(const void* x0, void* ys, long y_stride, uint8_t* masks, long mask_stride, const void* w,
                         long w_stride, const float* bias, long bias_stride, float h, int N, int H, int W, int C, int L,
                         hipStream_t s, int slots = 0);
// RK2: 2L stages in one launch (k_fwd3_stack<..., RK2>): x_l -> xmid_l (xm + l*y_stride,
// mask1 at masks + l*mask_stride) -> x_{l+1} (mask2 at masks2 + l*mask_stride)
int block_stack_fwd_rk2_mfma(const void* x0, void* ys, void* xm, long y_stride, uint8_t* masks, uint8_t* masks2,
                             long mask_stride, const void* w, long w_stride, const float* bias, long bias_stride,
                             float h, int N, int H, int W, int C, int L, hipStream_t s);
bool block_stack_bwd_supported(int N, int H, int W, int C);
int block_stack_bwd_grid(int N);
int stack_done_words(int L);
long stack_slab_floats(int C, int pair);
int block_stack_bwd_mfma(void* dbuf0, void* dbuf1, const void* xs, long x_stride, const uint8_t* masks,
                         long mask_stride, const void* w, long w_stride, float h, float two_gamma, int N, int H, int W,
                         int C, int L, int ro0, float* slabs, long slab_stride, float* grp, long grp_stride,
                         unsigned* done, int* lfold_out, hipStream_t s, const void* xm = nullptr,
                         const uint8_t* masks2 = nullptr, void* gbuf = nullptr, const void* gtop = nullptr,
                         int fold = 1, int pair = 0);
int stack_bwd_reduce_rest(const float* slabs, long slab_stride, int grid, long ES, float* grp, long grp_stride, int L,
                          int lfold, const unsigned* done, hipStream_t s);

// ---- asr_conv_f32.hip ------------------------------------------------------
int conv_f32(int fmode, const void* xin, void* out, uint8_t* mask, const float* w, const float* bias, float h,
             float two_gamma, const float* dy, int N, int H, int W, int Ci, int Co, int out_bf16, hipStream_t s,
             const float* extra = nullptr, int K = 3);
int conv_f32_k(int fmode, int K, const void* xin, void* out, uint8_t* mask, const float* w, const float* bias, float h,
               float two_gamma, const float* dy, int N, int H, int W, int C, hipStream_t s, const float* extra);
int make_dz(int fmode, const void* dy, const uint8_t* mask, const void* relu_src, float h, int N, int H, int W, int C,
            int src_bf16, float* dz, hipStream_t s);
int wgrad_f32(const void* x, int x_bf16, const float* dz, int N, int H, int W, int Ci, int Co, float* slabs,
              int* nslabs, hipStream_t s, int K = 3);
int wgrad_f32_chunks(int N, int H);
int f32_block_slab_rows(int N, int H, int W, int C);
bool conv32_fused_bwd_supported(int W, int C);
int conv32_bwd_fused(const float* dy, const uint8_t* mask, float h, const float* x, const float* w, float two_gamma,
                     const float* extra, bool skip_dy, int N, int H, int W, int C, float* dx, bool need_w,
                     float* slabs, int* nslabs, hipStream_t s);
// wgrad_layers' fp32 half (k_wgrad32, blockIdx.y = layer; dz = h dy [relu bit] formed in the kernel)
int wgrad32_layers(const float* x0, long x_stride, const float* dys, long d_stride, const uint8_t* masks,
                   long mask_stride, float h, int N, int H, int W, int C, int L, float* slabs, long slab_stride,
                   int* nslabs, hipStream_t s);
// bf16 <-> fp32, elementwise (n a multiple of 8)
int convert_bf16_f32(const void* src, void* dst, long n, int to_f32, hipStream_t s);

// ---- asr_conv_bf16.hip -----------------------------------------------------
// bf16 Euler blocks and bare convs at any width the 16-pixel MFMA tile takes (W = 8 or W % 16 == 0): the
// multi-stage nets' path, and every single-stage shape off W = 32
bool convb_supported(int W, int C);
// slab rows one such block's weight gradient writes (the workspaces that keep every block's slabs)
int bf16_block_slab_rows(int N, int H, int W, int C);
int convb_forward(const void* x, void* y, uint8_t* mask, const void* w, const float* bias, float h, int N, int H, int W,
                  int C, hipStream_t s, bool conv_only = false);
int convb_backward(const void* dy, const uint8_t* mask, const void* x, const void* w, float h, float two_gamma, int N,
                   int H, int W, int C, void* dx, bool need_w, float* slabs, int* nslabs, hipStream_t s,
                   bool conv_only = false);
// wgrad_layers' bf16 half (k_wgradb over bands, blockIdx.y = layer), C in {16, 32, 64}, W in {32, 16, 8}
int wgradb_layers(const bf16* x0, long x_stride, const bf16* dys, long d_stride, const uint8_t* masks, long mask_stride,
                  float h, int N, int H, int W, int C, int L, float* slabs, long slab_stride, int* nslabs,
                  hipStream_t s);

// ---- asr_stage_img.hip -----------------------------------------------------
// the image-resident stages (all L blocks of a 16 x 16 x 32 or 8 x 8 x 64 stage in one launch);
// dtype (ASR_BF16 / ASR_F32) picks the kernels; activations, W and dys are of that type
bool stage_img_supported(int H, int W, int C, int dtype);
int stage_img_forward(int dtype, const void* x0, void* ys, long y_stride, uint8_t* masks, long mask_stride,
                      const void* w, long w_stride, const float* bias, long bias_stride, float h, int N, int H, int W,
                      int C, int L, hipStream_t s);
int stage_img_backward(int dtype, const void* dyL, void* dys, long d_stride, void* dx0, const uint8_t* masks,
                       long mask_stride, const void* w, long w_stride, float h, float two_gamma, int N, int H, int W,
                       int C, int L, hipStream_t s);
int wgrad_layers(int dtype, const void* x0, long x_stride, const void* dys, long d_stride, const uint8_t* masks,
                 long mask_stride, float h, int N, int H, int W, int C, int L, float* slabs, long slab_stride,
                 int* nslabs, hipStream_t s);

// ---- asr_conv_kxk.hip ------------------------------------------------------
// bf16 Conv2DAntisymmetric(kernel_size = K), K in {5, 7}, C in {16, 32, 64}, W in {32, 16, 8}
bool convk_bf16_supported(int K, int W, int C);
int convk_bf16(int fmode, int K, const void* xin, void* out, uint8_t* mask, const void* w, const float* bias, float h,
               float two_gamma, const uint8_t* dmask, int N, int H, int W, int C, hipStream_t s);
int wgradk_bf16_slab_rows(int K, int N, int H, int W, int C);
int wgradk_bf16(int K, const void* x, const void* dy, const uint8_t* mask, float h, int N, int H, int W, int C,
                float* slabs, int* nslabs, hipStream_t s);

// ---- asr_deep16.hip --------------------------------------------------------
// the C = 16, 32 x 32 bf16 stage as one fused forward / backward launch
bool deep16_supported(int H, int W, int C);
int deep16_forward(const void* x0, void* y0, long y_stride, uint8_t* mask0, long mask_stride, const void* wpack,
                   const float* bias, long bias_stride, float h, int N, int L, bool store_all, hipStream_t s);
size_t deep16_slab_bytes(int N, int L);
int deep16_backward(void* dbufA, void* dbufB, const void* xs, long x_stride, const uint8_t* masks, long mask_stride,
                    const void* wpack, float h, float two_gamma, int N, int L, float* slabs, int* slab_rows,
                    int* dx0_in_b, hipStream_t s);

// ---- asr_stem_head.hip -----------------------------------------------------
bool stem_supported(int Cin, int H, int W, int C);
int stem_forward(const void* img, int input_u8, const float* w1, const float* b1, int N, int H, int W, int Cin, int C,
                 float mean, float inv_std, int use_norm, void* out, int out_bf16, hipStream_t s);
int stem_wgrad(const void* img, int input_u8, const void* dx1, const void* x1, int act_bf16, int N, int H, int W,
               int Cin, int C, float mean, float inv_std, int use_norm, float* slabs, int* nslabs, hipStream_t s);
int head(const void* xL, int act_bf16, const float* fck, const float* fcb, const float* targets, int N, int HW, int C,
         int K, float* probs, float* loss_per, float* dlogits, float* gap, void* dxL, hipStream_t s,
         void* growL = nullptr);
int head_param_grads(const float* gap, const float* dlogits, int N, int C, int K, float* dfck, float* dfcb,
                     const float* loss_per, float* loss_out, hipStream_t s);
// dz1 = dx1 * [x1 > 0] in place (bf16, n % 8 == 0): the stem's relu' where block 0's backward did not fuse it
int relu_grad_bf16(void* d, const void* x, long n, hipStream_t s);

// ---- asr_augment.hip -------------------------------------------------------
// the dataset preprocessors in one launch per batch (asr_augment_batch, asr.h, is this with a void* stream)
int augment_batch(const void* src, long n_src, const asr_aug_plan* plan, const asr_aug_item* items, int N, void* dst,
                  hipStream_t s);

// ---- asr_api.hip -----------------------------------------------------------
// (the layer-level ABI's helpers that the executors, asr_net.hip and asr_stages.hip, call)
bool mfma_supported(int C, int W);
int check_shape(int N, int H, int W, int C);
// BwdWs (asr_common.h) of one conv application (stages = 2: an RK2 block); slab_rows < 0: the rows its kernel may write
BwdWs bwd_ws_layout(int N, int H, int W, int C, int dtype, int stages = 1, int K = 3, int slab_rows = -1);
int block_backward(int mode, const void* dy, const void* x, const uint8_t* mask, const void* w, float h, float gamma,
                   int N, int H, int W, int C, int dtype, void* dx, bool need_w, const void* extra, bool skip_dy,
                   float* slabs, float* dz_scratch, int* nsl, hipStream_t s, bool relu_dx = false,
                   int* relu_done = nullptr, const float* fold_slabs = nullptr, int fold_P = 0,
                   float* fold_grp = nullptr, int* fold_done = nullptr, bool accum_slabs = false);
int rk2_forward_impl(const void* x, void* xmid, void* y, uint8_t* mask1, uint8_t* mask2, const void* w,
                     const float* bias, float h, int N, int H, int W, int C, int dtype, hipStream_t s);
int rk2_backward_slabs(const void* dy, const void* x, const void* xmid, const uint8_t* mask1, const uint8_t* mask2,
                       const void* w, float h, float gamma, int N, int H, int W, int C, int dtype, void* dx, void* g,
                       bool need_w, float* slabs, float* dz_scratch, int* nsl, hipStream_t s,
                       const float* fold_slabs = nullptr, int fold_P = 0, float* fold_grp = nullptr,
                       int* fold_done = nullptr);
int conv_backward_keep_slabs(const void* dy, const void* x, const uint8_t* mask, const void* w, float h, float gamma,
                             int N, int H, int W, int C, void* dx, void* ws, float* slabs, int* nsl, hipStream_t s);
// A stage whose L Euler blocks run in one launch: deep16 (bf16, 32 x 32 x 16) before the
// image-resident kernels (stage_img_supported); the stack ABI and the multi-stage executor
// run both through fused_stage_forward / fused_stage_backward.
constexpr int kFusedNone = 0;
constexpr int kFusedDeep16 = 1;
constexpr int kFusedImg = 2;
int fused_stage_kind(int H, int W, int C, int dtype);
int fused_stage_forward(int kind, int dtype, const void* x0, void* ys, long y_stride, uint8_t* masks, long mask_stride,
                        const void* w, long w_stride, const float* bias, long bias_stride, float h, int N, int H, int W,
                        int C, int L, bool store_all, hipStream_t s);
int fused_stage_backward(const char* who, int kind, int dtype, void* d, void* e, int* in_e, void* dx0_copy, void* dys,
                         const void* xs, long x_stride, const uint8_t* masks, long mask_stride, const void* w,
                         long w_stride, float h, float two_gamma, int N, int H, int W, int C, int L, float* slabs,
                         long slab_stride, int slab_rows, float* grp, long grp_stride, const int32_t* theta_dst,
                         long n_theta, float* dparams, long dp_stride, hipStream_t s);

}  // namespace asr
