// The bf16 MFMA kernels of the antisymmetric Euler block at W = 32 (gfx950),
// one translation unit: the kernels live in the family headers included below
// (in this order; each opens with its kernels' design), this file holds the
// host side: the launchers and their grids and LDS sizes, the *_supported
// predicates, the stacked backward's post-launch reduction and the extern "C"
// debug and status entry points.
// One unit because the kernels' code generation depends on what else the module
// holds, and the diagnostic builds (-DASR_STAMP_BUILD, -DASR_BLK_TRACE) share
// their device buffers between the per-block and the stack kernels.
#include <stdlib.h>

#include "asr_common.h"
#include "asr_internal.h"
// (the order of the kernels' definitions)
#include "asr_blk_common.h"
#include "asr_blk_fwd.h"
#include "asr_blk_bwd.h"
#include "asr_blk_stack.h"
#include "asr_blk_stem.h"

namespace asr {

// ---------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------
constexpr int kBwdBR = 4;
constexpr int kFwdBR = 4;  // k_fwd3 / k_fwd3_stack row band

#if ASR_BLK_TRACE
}  // namespace asr
extern "C" int asr_debug_blk_trace(void* trace, size_t tbytes, void* clock, size_t cbytes) {
  if (hipMemcpyFromSymbol(trace, HIP_SYMBOL(asr::blk::g_btrace), tbytes) != hipSuccess) return -1;
  return hipMemcpyFromSymbol(clock, HIP_SYMBOL(asr::blk::g_bclock), cbytes) == hipSuccess ? 0 : -1;
}
extern "C" int asr_debug_blk_switch(void* dst, size_t bytes) {  // g_bswitch (k_bwd3_stack block switches)
  if (bytes > sizeof(asr::blk::g_bswitch)) bytes = sizeof(asr::blk::g_bswitch);
  return hipMemcpyFromSymbol(dst, HIP_SYMBOL(asr::blk::g_bswitch), bytes) == hipSuccess ? 0 : -1;
}
namespace asr {
#endif

static int persistent_grid(long items) {
  const int cus = launch_cus();
  return (int)std::max<long>(1, std::min<long>({items, (long)cus, (long)kMaxBlockSlabs}));
}

template <int C, int W, int BR, int NW>
static int launch_fwd_v(int mode, const void* x, const void* resid, void* y, uint8_t* mask, const void* w,
                        const float* bias, float h, int N, int H, hipStream_t s) {
  static_assert(NW % blk::Geo<C>::OSPLIT == 0, "waves must cover the o-split");
  const long items = (long)N * ((H + BR - 1) / BR);
  if (items > 0x7fffffffL) return fail(ASR_E_UNSUPPORTED, "bf16 block: too many row bands (%ld)", items);
  const int cus = launch_cus();
  const int grid = (int)std::max<long>(1, std::min<long>(items, (long)cus * (8 / NW)));
  const size_t lds = 2 * (size_t)(BR + 2) * (W + 2) * C * 2;
  if constexpr (C == 64 && W == 32 && BR == 4 && NW == 4) {
    if (!resid || mode == blk::FWD_EULER) {
      const int grid3 = (int)std::max<long>(1, std::min<long>(items, (long)cus * kFwd3Wgs));
      if (mode == blk::FWD_EULER && resid)
        hipLaunchKernelGGL((blk::k_fwd3<C, W, BR, blk::FWD_EULER, 3, true>), dim3(grid3), dim3(256), lds, s,
                           (const bf16*)x, (const bf16*)resid, (bf16*)y, mask, (const bf16*)w, bias, h, N, H);
      else if (mode == blk::FWD_EULER)
        hipLaunchKernelGGL((blk::k_fwd3<C, W, BR, blk::FWD_EULER, 3>), dim3(grid3), dim3(256), lds, s, (const bf16*)x,
                           nullptr, (bf16*)y, mask, (const bf16*)w, bias, h, N, H);
      else
        hipLaunchKernelGGL((blk::k_fwd3<C, W, BR, blk::FWD_CONV, 3>), dim3(grid3), dim3(256), lds, s, (const bf16*)x,
                           nullptr, (bf16*)y, mask, (const bf16*)w, bias, h, N, H);
      ASR_LAUNCH_CHECK("k_fwd3");
      return ASR_OK;
    }
  }
  if constexpr (C >= 32) {
    if (mode == blk::FWD_EULER && resid) {  // second RK2 stage: residual from the step input
      hipLaunchKernelGGL((blk::k_fwd_pipe<C, W, BR, blk::FWD_EULER, NW, true>), dim3(grid), dim3(64 * NW), lds, s,
                         (const bf16*)x, (const bf16*)resid, (bf16*)y, mask, (const bf16*)w, bias, h, N, H);
    } else if (mode == blk::FWD_EULER) {
      hipLaunchKernelGGL((blk::k_fwd_pipe<C, W, BR, blk::FWD_EULER, NW>), dim3(grid), dim3(64 * NW), lds, s,
                         (const bf16*)x, nullptr, (bf16*)y, mask, (const bf16*)w, bias, h, N, H);
    } else {
      hipLaunchKernelGGL((blk::k_fwd_pipe<C, W, BR, blk::FWD_CONV, NW>), dim3(grid), dim3(64 * NW), lds, s,
                         (const bf16*)x, nullptr, (bf16*)y, mask, (const bf16*)w, bias, h, N, H);
    }
  } else {
    if (mode == blk::FWD_EULER)
      hipLaunchKernelGGL((blk::k_fwd<C, W, BR, blk::FWD_EULER, NW>), dim3(grid), dim3(64 * NW), lds, s,
                         (const bf16*)x, (const bf16*)resid, (bf16*)y, mask, (const bf16*)w, bias, h, N, H);
    else
      hipLaunchKernelGGL((blk::k_fwd<C, W, BR, blk::FWD_CONV, NW>), dim3(grid), dim3(64 * NW), lds, s,
                         (const bf16*)x, (const bf16*)resid, (bf16*)y, mask, (const bf16*)w, bias, h, N, H);
  }
  ASR_LAUNCH_CHECK("k_fwd");
  return ASR_OK;
}

template <int C, int W>
static int launch_fwd(int mode, const void* x, const void* resid, void* y, uint8_t* mask, const void* w,
                      const float* bias, float h, int N, int H, hipStream_t s) {
  // 4-row bands, 4 waves (one 16-channel o-tile each at C=64), 2 WGs per CU
  // (geometry chosen by A/B on MI355X against 8x8, 4x8 and 8x4)
  return launch_fwd_v<C, W, 4, 4>(mode, x, resid, y, mask, w, bias, h, N, H, s);
}

template <int C, int W>
static int launch_bwd(int mode, const void* dy, const void* x, const uint8_t* mask, const void* w, float h,
                      float two_gamma, int N, int H, void* dx, float* slabs, int* nslabs, const void* extra,
                      int skip_dy, int relu_dx, int* relu_done, const float* fold_slabs, int fold_P, float* fold_grp,
                      int* fold_done, int accum, hipStream_t s) {
  const long items = (long)N * ((H + kBwdBR - 1) / kBwdBR);
  if (items > 0x7fffffffL) return fail(ASR_E_UNSUPPORTED, "bf16 block: too many row bands (%ld)", items);
  const int grid = persistent_grid(items);
  *nslabs = grid;
  using L = blk::BwdLds<C, W, kBwdBR>;
  const size_t red = (size_t)(12288 + 4 * 64) * 4;
  const size_t lds = std::max((size_t)(extra ? L::TOTAL_XT : L::TOTAL), red);
#define ASR_LAUNCH_BWD(M, XT)                                                                                    \
  hipLaunchKernelGGL((blk::k_bwd<C, W, kBwdBR, M, XT>), dim3(grid), dim3(512), lds, s, (const bf16*)dy, (const bf16*)x, \
                     mask, (const bf16*)w, h, two_gamma, N, H, (bf16*)dx, slabs, (const bf16*)extra, skip_dy, accum)
  const bool xt = extra != nullptr || skip_dy != 0 || accum != 0;
  if constexpr (C == 64) {
    // v2: the Euler block, the plain conv, and both RK2 stages (the first: extra
    // dx term + slab accumulation); other compositions run the v1 kernel
    const bool xt2 = extra && accum && !skip_dy && mode == blk::BWD_EULER && !relu_dx;
    if (xt2 || (!extra && !accum && (mode == blk::BWD_EULER || !skip_dy))) {
      using L2 = blk::Bwd2Lds<C, W, kBwdBR>;
      const size_t lds2 = std::max((size_t)L2::TOTAL, red);
      // the folded pass gives each thread one 16-B chunk: at most 512 per WG
      const long fchunks = (long)((fold_P + 31) / 32) * ((9 * C * C + C) / 4);
      if ((fchunks + grid - 1) / grid > 512) fold_P = 0;
#define ASR_LAUNCH_BWD3(M, RO, XT)                                                                            \
  hipLaunchKernelGGL((blk::k_bwd3<C, W, kBwdBR, M, RO, XT>), dim3(grid), dim3(768), lds2, s, (const bf16*)dy,    \
                     (const bf16*)x, mask, (const bf16*)w, h, two_gamma, N, H, (bf16*)dx, slabs, fold_slabs, fold_P, \
                     fold_grp, skip_dy, (const bf16*)extra)
      if (xt2) ASR_LAUNCH_BWD3(blk::BWD_EULER, false, true);
      else if (mode == blk::BWD_EULER && relu_dx) {
        ASR_LAUNCH_BWD3(blk::BWD_EULER, true, false);
        if (relu_done) *relu_done = 1;
      } else if (mode == blk::BWD_EULER) ASR_LAUNCH_BWD3(blk::BWD_EULER, false, false);
      else ASR_LAUNCH_BWD3(blk::BWD_CONV, false, false);
#undef ASR_LAUNCH_BWD3
      ASR_LAUNCH_CHECK("k_bwd3");
      if (fold_done) *fold_done = fold_P > 0;
      return ASR_OK;
    }
  }
  if (mode == blk::BWD_EULER) {
    if (xt) ASR_LAUNCH_BWD(blk::BWD_EULER, true);
    else ASR_LAUNCH_BWD(blk::BWD_EULER, false);
  } else {
    if (xt) ASR_LAUNCH_BWD(blk::BWD_CONV, true);
    else ASR_LAUNCH_BWD(blk::BWD_CONV, false);
  }
#undef ASR_LAUNCH_BWD
  ASR_LAUNCH_CHECK("k_bwd");
  return ASR_OK;
}

// ---------------------------------------------------------------------------
// stem weight gradient on MFMA (see k_stem_wgrad_mfma)
// ---------------------------------------------------------------------------
static size_t stem_wgrad_mfma_lds(int H, int C) {
  return (size_t)H * 34 * 64 + 2 * 8 * 34 * (C / 8) * 16 + (size_t)(H + 2) * 34 * 3 * 4;
}

bool stem_wgrad_mfma_supported(int Cin, int H, int W, int C) {
  return Cin == 3 && W == 32 && (C == 64 || C == 16) && H % 8 == 0 && H >= 8 &&
         stem_wgrad_mfma_lds(H, C) <= 160 * 1024;
}

int stem_wgrad_mfma(const void* img, int input_u8, const void* dz1, int N, int H, int W, int Cin, int C, float mean,
                    float inv_std, int use_norm, float* slabs, int* nslabs, hipStream_t s) {
  if (!stem_wgrad_mfma_supported(Cin, H, W, C)) return fail(ASR_E_UNSUPPORTED, "stem wgrad (MFMA): unsupported shape");
  const int cus = launch_cus();
  const int grid = std::max(1, std::min(N, std::min(cus, kMaxBlockSlabs)));
  *nslabs = grid;
  const size_t lds = std::max(stem_wgrad_mfma_lds(H, C), (size_t)4 * 32 * C * 4);  // (reduction area)
  const float m = use_norm ? mean : 0.f, is = use_norm ? inv_std : 1.f;
#define ASR_STEMW(CC, TI)                                                                                   \
  hipLaunchKernelGGL((blk::k_stem_wgrad_mfma<CC, TI>), dim3(grid), dim3(256), lds, s, (const TI*)img, \
                     (const bf16*)dz1, N, H, m, is, slabs)
  if (C == 64) {
    if (input_u8) ASR_STEMW(64, uint8_t);
    else ASR_STEMW(64, float);
  } else {
    if (input_u8) ASR_STEMW(16, uint8_t);
    else ASR_STEMW(16, float);
  }
#undef ASR_STEMW
  ASR_LAUNCH_CHECK("k_stem_wgrad_mfma");
  return ASR_OK;
}

bool stem_fwd_mfma_supported(int Cin, int H, int W, int C) {
  const size_t lds = (size_t)(H + 2) * 34 * 3 * 4;
  return Cin == 3 && W == 32 && (C == 64 || C == 16) && H >= 1 && lds <= 160 * 1024;
}

int stem_fwd_mfma(const void* img, int input_u8, const float* w1, const float* b1, int N, int H, int W, int Cin, int C,
                  float mean, float inv_std, int use_norm, void* out, hipStream_t s) {
  if (!stem_fwd_mfma_supported(Cin, H, W, C)) return fail(ASR_E_UNSUPPORTED, "stem fwd (MFMA): unsupported shape");
  const int cus = launch_cus();
  const int grid = std::max(1, std::min(N, 4 * cus));
  const size_t lds = (size_t)(H + 2) * 34 * 3 * 4;
  const float m = use_norm ? mean : 0.f, is = use_norm ? inv_std : 1.f;
#define ASR_STEMF(CC, TI)                                                                                     \
  hipLaunchKernelGGL((blk::k_stem_fwd_mfma<CC, TI>), dim3(grid), dim3(256), lds, s, (const TI*)img, w1, b1, N, H, m, \
                     is, (bf16*)out)
  if (C == 64) {
    if (input_u8) ASR_STEMF(64, uint8_t);
    else ASR_STEMF(64, float);
  } else {
    if (input_u8) ASR_STEMF(16, uint8_t);
    else ASR_STEMF(16, float);
  }
#undef ASR_STEMF
  ASR_LAUNCH_CHECK("k_stem_fwd_mfma");
  return ASR_OK;
}

// ---------------------------------------------------------------------------
// the 5 x 5 / 7 x 7 stem on MFMA (k_stem_fwd_kxk, k_stem_wgrad_kxk): row bands, any H
// ---------------------------------------------------------------------------
bool stem_kxk_supported(int K, int Cin, int W, int C) {
  return (K == 5 || K == 7) && Cin == 3 && (W == 32 || W == 16 || W == 8) && (C == 16 || C == 32 || C == 64);
}

// every (K, C, W) of the supported set, u8 and float images
#define ASR_STEMK_CASES(K_)                                                                                     \
  ASR_STEMK(K_, 16, 8) ASR_STEMK(K_, 16, 16) ASR_STEMK(K_, 16, 32) ASR_STEMK(K_, 32, 8) ASR_STEMK(K_, 32, 16)   \
  ASR_STEMK(K_, 32, 32) ASR_STEMK(K_, 64, 8) ASR_STEMK(K_, 64, 16) ASR_STEMK(K_, 64, 32)

template <int C, int W, int K, typename TI>
static int launch_stem_fwd_kxk(const void* img, const float* w1, const float* b1, int N, int H, float m, float is,
                               void* out, hipStream_t s) {
  const long items = (long)N * ((H + blk::StemK<W, K>::BRF - 1) / blk::StemK<W, K>::BRF);
  const int grid = (int)std::max<long>(1, std::min<long>(items, 2L * launch_cus()));
  hipLaunchKernelGGL((blk::k_stem_fwd_kxk<C, W, K, TI>), dim3(grid), dim3(256), 0, s, (const TI*)img, w1, b1, N, H, m,
                     is, (bf16*)out);
  ASR_LAUNCH_CHECK("k_stem_fwd_kxk");
  return ASR_OK;
}

int stem_fwd_kxk(int K, const void* img, int input_u8, const float* w1, const float* b1, int N, int H, int W, int Cin,
                 int C, float mean, float inv_std, int use_norm, void* out, hipStream_t s) {
  if (!stem_kxk_supported(K, Cin, W, C) || N < 1 || H < 1)
    return fail(ASR_E_UNSUPPORTED, "stem fwd (MFMA, K=%d): unsupported shape", K);
  const float m = use_norm ? mean : 0.f, is = use_norm ? inv_std : 1.f;
#define ASR_STEMK(K_, C_, W_)                                                                                  \
  if (K == K_ && C == C_ && W == W_)                                                                           \
    return input_u8 ? launch_stem_fwd_kxk<C_, W_, K_, uint8_t>(img, w1, b1, N, H, m, is, out, s)               \
                    : launch_stem_fwd_kxk<C_, W_, K_, float>(img, w1, b1, N, H, m, is, out, s);
  ASR_STEMK_CASES(5)
  ASR_STEMK_CASES(7)
#undef ASR_STEMK
  return fail(ASR_E_UNSUPPORTED, "stem fwd (MFMA, K=%d): unsupported shape", K);
}

template <int C, int W, int K, typename TI>
static int launch_stem_wgrad_kxk(const void* img, const void* dz1, int N, int H, float m, float is, float* slabs,
                                 int* nslabs, hipStream_t s) {
  const long items = (long)N * ((H + blk::StemK<W, K>::BRW - 1) / blk::StemK<W, K>::BRW);
  const int grid = persistent_grid(items);  // (<= kMaxBlockSlabs; every workgroup has an item and writes its slab)
  *nslabs = grid;
  hipLaunchKernelGGL((blk::k_stem_wgrad_kxk<C, W, K, TI>), dim3(grid), dim3(256), 0, s, (const TI*)img,
                     (const bf16*)dz1, N, H, m, is, slabs);
  ASR_LAUNCH_CHECK("k_stem_wgrad_kxk");
  return ASR_OK;
}

int stem_wgrad_kxk(int K, const void* img, int input_u8, const void* dz1, int N, int H, int W, int Cin, int C,
                   float mean, float inv_std, int use_norm, float* slabs, int* nslabs, hipStream_t s) {
  *nslabs = 0;
  if (!stem_kxk_supported(K, Cin, W, C) || N < 1 || H < 1)
    return fail(ASR_E_UNSUPPORTED, "stem wgrad (MFMA, K=%d): unsupported shape", K);
  const float m = use_norm ? mean : 0.f, is = use_norm ? inv_std : 1.f;
#define ASR_STEMK(K_, C_, W_)                                                                                  \
  if (K == K_ && C == C_ && W == W_)                                                                           \
    return input_u8 ? launch_stem_wgrad_kxk<C_, W_, K_, uint8_t>(img, dz1, N, H, m, is, slabs, nslabs, s)      \
                    : launch_stem_wgrad_kxk<C_, W_, K_, float>(img, dz1, N, H, m, is, slabs, nslabs, s);
  ASR_STEMK_CASES(5)
  ASR_STEMK_CASES(7)
#undef ASR_STEMK
  return fail(ASR_E_UNSUPPORTED, "stem wgrad (MFMA, K=%d): unsupported shape", K);
}
#undef ASR_STEMK_CASES

int block_fwd_mfma(int mode, const void* x, const void* resid, void* y, uint8_t* mask, const void* w,
                   const float* bias, float h, int N, int H, int W, int C, hipStream_t s) {
  if (W != 32) return fail(ASR_E_UNSUPPORTED, "bf16 block: W=%d not supported (W must be 32)", W);
  switch (C) {
    case 16: return launch_fwd<16, 32>(mode, x, resid, y, mask, w, bias, h, N, H, s);
    case 32: return launch_fwd<32, 32>(mode, x, resid, y, mask, w, bias, h, N, H, s);
    case 64: return launch_fwd<64, 32>(mode, x, resid, y, mask, w, bias, h, N, H, s);
  }
  return fail(ASR_E_UNSUPPORTED, "bf16 block: C=%d not supported (16, 32, 64)", C);
}

bool block_stack_fwd_supported(int N, int H, int W, int C) {
  return C == 64 && W == 32 && N >= 1 && (H + kFwdBR - 1) / kFwdBR >= 4;
}

// k_fwd3_stack (Euler and RK2): whole images per workgroup, two workgroups per CU; LDS = its ring of three tiles
static int stack_fwd_grid(int N) { return std::max(1, std::min(N, 2 * launch_cus())); }
static size_t stack_fwd_lds(int W, int C) { return 3 * (size_t)(kFwdBR + 2) * (W + 2) * C * 2; }

// all L Euler blocks in one launch (k_fwd3_stack); x_l of block l >= 1 is
// ys + (l-1)*y_stride, its output ys + l*y_stride (elements)
int block_stack_fwd_mfma(const void* x0, void* ys, long y_stride, uint8_t* masks, long mask_stride, const void* w,
                         long w_stride, const float* bias, long bias_stride, float h, int N, int H, int W, int C, int L,
                         hipStream_t s, int slots) {
  if (!block_stack_fwd_supported(N, H, W, C) || L < 1)
    return fail(ASR_E_UNSUPPORTED, "stack forward: needs C=64, W=32, >= 4 row bands per image (C=%d W=%d H=%d)", C, W, H);
  if (y_stride < (long)N * H * W * C) return fail(ASR_E_ARG, "stack forward: y_stride smaller than one activation");
  if (slots != 0 && slots != 2) return fail(ASR_E_ARG, "stack forward: slots must be 0 or 2");
  const int grid = stack_fwd_grid(N);
  const size_t lds = stack_fwd_lds(W, C);
  hipLaunchKernelGGL((blk::k_fwd3_stack<64, 32, kFwdBR>), dim3(grid), dim3(256), lds, s, (const bf16*)x0,
                     (bf16*)ys, y_stride, masks, mask_stride, (const bf16*)w, w_stride, bias, bias_stride, h, N, H, L,
                     slots);
  ASR_LAUNCH_CHECK("k_fwd3_stack");
  return ASR_OK;
}

// test knobs (asr_debug_stack_backward): a forced grid (0: one workgroup per
// CU) and the bound of the slab hand-off's wait (0: the default)
static int g_stack_grid_override = 0;

// dynamic LDS of k_bwd3_stack: the v2 tiles + mask table, then its "late" word
static size_t stack_bwd_lds() { return (size_t)blk::Bwd2Lds<64, 32, kBwdBR>::TOTAL + 16; }

// k_bwd3_stack workgroups the device keeps resident per CU (both
// instantiations; cached per device): the in-launch hand-off is fast only with
// the whole grid resident, so the stacked path is used only when this is >= 1
static int stack_bwd_resident_per_cu() {
  static int dev_cached = -1, per = 0;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  if (dev != dev_cached) {
    int a = 0, b = 0, c = 0, d = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, blk::k_bwd3_stack<64, 32, kBwdBR, false, false>, 768,
                                                     stack_bwd_lds()) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, blk::k_bwd3_stack<64, 32, kBwdBR, true, false>, 768,
                                                     stack_bwd_lds()) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&c, blk::k_bwd3_stack<64, 32, kBwdBR, false, true>, 768,
                                                     stack_bwd_lds()) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&d, blk::k_bwd3_stack<64, 32, kBwdBR, true, true>, 768,
                                                     stack_bwd_lds()) != hipSuccess)
      return 0;
    per = std::min(std::min(a, b), std::min(c, d));
    dev_cached = dev;
  }
  return per;
}

bool block_stack_bwd_supported(int N, int H, int W, int C) {
  return C == 64 && W == 32 && N >= 1 && (H + kBwdBR - 1) / kBwdBR >= 4 && stack_bwd_resident_per_cu() >= 1;
}

// workgroups of k_bwd3_stack: one per CU at most (the in-launch slab
// hand-off needs every workgroup resident), whole images each
int block_stack_bwd_grid(int N) {
  const int cus = launch_cus();
  const int cap = g_stack_grid_override > 0 ? g_stack_grid_override : cus;
  return std::max(1, std::min(N, std::min(cap, kMaxBlockSlabs)));
}

int stack_done_words(int L) { return 2 * L + 4; }

// floats per slab of k_bwd3_stack: the full dW (9C^2 + C) or, pair-local, the 74 D tiles + db
long stack_slab_floats(int C, int pair) { return pair ? (long)PairSlabLayout::ES : 9L * C * C + C; }

// the backward of L Euler blocks in one launch (k_bwd3_stack).  dbuf0 holds
// dL/dx_L on entry, or gtop (Euler) its per-image row (the head's GAP
// gradient, bf16 [N][C]): then dbuf0 is not read.  Block 0's dx ends in dbuf[L & 1].  Block l's slabs (grid
// of them, tile-major dW) at slabs + l*slab_stride; blocks >= lfold leave as
// 32-slab group sums at grp + l*grp_stride (unless flagged), the rest as slabs:
// stack_bwd_reduce_rest finishes both.  done: stack_done_words(L) words, zeroed
// here: the per-block publish counters [0, L+4) and the per-block flags
// [L+4, 2L+4) of folds whose wait ran out.
int block_stack_bwd_mfma(void* dbuf0, void* dbuf1, const void* xs, long x_stride, const uint8_t* masks,
                         long mask_stride, const void* w, long w_stride, float h, float two_gamma, int N, int H, int W,
                         int C, int L, int ro0, float* slabs, long slab_stride, float* grp, long grp_stride,
                         unsigned* done, int* lfold_out, hipStream_t s, const void* xm, const uint8_t* masks2,
                         void* gbuf, const void* gtop, int fold, int pair) {
  if (!block_stack_bwd_supported(N, H, W, C) || L < 1)
    return fail(ASR_E_UNSUPPORTED, "stack backward: needs C=64, W=32, >= 4 row bands per image (C=%d W=%d H=%d)", C, W, H);
  const int grid = block_stack_bwd_grid(N);
  const long ES = stack_slab_floats(C, pair);
  if (slab_stride < (long)grid * ES) return fail(ASR_E_ARG, "stack backward: slab_stride too small");
  // in-kernel pass 1 needs <= 512 group-row chunks per workgroup (one per wgrad thread)
  const long fchunks = (long)((grid + 31) / 32) * (ES / 4);
  // fold = 0: no in-launch pass 1, so no workgroup ever waits for another (no
  // co-residency needed: e.g. several processes sharing one device)
  const int lfold = fold && (fchunks + grid - 1) / grid <= 512 ? 2 : L;
  if (lfold_out) *lfold_out = lfold;
  ASR_TRY(zero_words(done, stack_done_words(L), s));
  unsigned* skipf = done + L + 4;
  const size_t lds = stack_bwd_lds();
#define ASR_STACK_BWD(RK, PR)                                                                                   \
  hipLaunchKernelGGL((blk::k_bwd3_stack<64, 32, kBwdBR, RK, PR>), dim3(grid), dim3(768), lds, s, (bf16*)dbuf0,         \
                     (bf16*)dbuf1, (const bf16*)xs, x_stride, masks, mask_stride, (const bf16*)w, w_stride, h,         \
                     two_gamma, N, H, L, RK ? 0 : ro0, slabs, slab_stride, grp, grp_stride, done, skipf, lfold,        \
                     RK ? (const bf16*)xm : nullptr, RK ? masks2 : nullptr, RK ? (bf16*)gbuf : nullptr,                \
                     RK ? nullptr : (const bf16*)gtop)
  if (xm) {  // RK2: both stages of every block (x_mid stack at xm, stride x_stride; masks2; g scratch)
    if (!masks2 || !gbuf) return fail(ASR_E_ARG, "stack backward (RK2): masks2 and the g buffer are required");
    if (pair) ASR_STACK_BWD(true, true);
    else ASR_STACK_BWD(true, false);
  } else {
    if (pair) ASR_STACK_BWD(false, true);
    else ASR_STACK_BWD(false, false);
  }
#undef ASR_STACK_BWD
  ASR_LAUNCH_CHECK("k_bwd3_stack");
  return ASR_OK;
}

// Pass 1 of the stacked backward's weight-gradient reduction left after the
// launch: blocks below lfold always, blocks at or above it only where a fold's
// wait ran out (flags[l] != 0: their group rows are recomputed from the slabs,
// all published by now).  Same sums in the same order as k_reduce_slabs and
// the in-launch fold (32-slab groups): deterministic either way.
__global__ __launch_bounds__(256) void k_reduce_slabs_flagged(const float* __restrict__ slabs, long slab_stride, long ES,
                                                              int P, float* __restrict__ grp, long grp_stride, int L,
                                                              int lfold, const unsigned* __restrict__ flags) {
  const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
  const int g = blockIdx.y;
  const int p0 = 32 * g, p1 = min(P, p0 + 32);
  for (int l = 0; l < L; ++l) {
    if (l >= lfold && flags[l] == 0u) continue;
    if (e >= ES) continue;
    const float* in = slabs + (long)l * slab_stride;
    float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, acc3 = 0.f;
    int p = p0;
    for (; p + 3 < p1; p += 4) {
      acc0 += in[(long)p * ES + e];
      acc1 += in[(long)(p + 1) * ES + e];
      acc2 += in[(long)(p + 2) * ES + e];
      acc3 += in[(long)(p + 3) * ES + e];
    }
    for (; p < p1; ++p) acc0 += in[(long)p * ES + e];
    grp[(long)l * grp_stride + (long)g * ES + e] = (acc0 + acc1) + (acc2 + acc3);
  }
}

int stack_bwd_reduce_rest(const float* slabs, long slab_stride, int grid, long ES, float* grp, long grp_stride, int L,
                          int lfold, const unsigned* done, hipStream_t s) {
  const int G = (grid + 31) / 32;
  hipLaunchKernelGGL(k_reduce_slabs_flagged, dim3((unsigned)((ES + 255) / 256), G), dim3(256), 0, s, slabs,
                     slab_stride, ES, grid, grp, grp_stride, L, lfold, done + L + 4);
  ASR_LAUNCH_CHECK("k_reduce_slabs_flagged");
  return ASR_OK;
}

int block_stack_fwd_rk2_mfma(const void* x0, void* ys, void* xm, long y_stride, uint8_t* masks, uint8_t* masks2,
                             long mask_stride, const void* w, long w_stride, const float* bias, long bias_stride,
                             float h, int N, int H, int W, int C, int L, hipStream_t s) {
  if (!block_stack_fwd_supported(N, H, W, C) || L < 1 || !xm)
    return fail(ASR_E_UNSUPPORTED, "RK2 stack forward: needs C=64, W=32, >= 4 row bands per image");
  if (y_stride < (long)N * H * W * C) return fail(ASR_E_ARG, "RK2 stack forward: y_stride smaller than one activation");
  const int grid = stack_fwd_grid(N);
  const size_t lds = stack_fwd_lds(W, C);
  hipLaunchKernelGGL((blk::k_fwd3_stack<64, 32, kFwdBR, true>), dim3(grid), dim3(256), lds, s, (const bf16*)x0,
                     (bf16*)ys, y_stride, masks, mask_stride, (const bf16*)w, w_stride, bias, bias_stride, h, N, H, L, 0,
                     (bf16*)xm, masks2);
  ASR_LAUNCH_CHECK("k_fwd3_stack<RK2>");
  return ASR_OK;
}

int block_bwd_mfma(int mode, const void* dy, const void* x, const uint8_t* mask, const void* w, float h,
                   float two_gamma, int N, int H, int W, int C, void* dx, float* slabs, int* nslabs, const void* extra,
                   int skip_dy, hipStream_t s, int relu_dx, int* relu_done, const float* fold_slabs, int fold_P,
                   float* fold_grp, int* fold_done, int accum) {
  if (relu_done) *relu_done = 0;
  if (fold_done) *fold_done = 0;
  if (fold_P > kMaxBlockSlabs) fold_P = 0;  // (never: slab counts are grid sizes)
  if (W != 32) return fail(ASR_E_UNSUPPORTED, "bf16 block: W=%d not supported (W must be 32)", W);
  switch (C) {
    case 16:
      return launch_bwd<16, 32>(mode, dy, x, mask, w, h, two_gamma, N, H, dx, slabs, nslabs, extra, skip_dy, relu_dx,
                                relu_done, fold_slabs, fold_P, fold_grp, fold_done, accum, s);
    case 32:
      return launch_bwd<32, 32>(mode, dy, x, mask, w, h, two_gamma, N, H, dx, slabs, nslabs, extra, skip_dy, relu_dx,
                                relu_done, fold_slabs, fold_P, fold_grp, fold_done, accum, s);
    case 64:
      return launch_bwd<64, 32>(mode, dy, x, mask, w, h, two_gamma, N, H, dx, slabs, nslabs, extra, skip_dy, relu_dx,
                                relu_done, fold_slabs, fold_P, fold_grp, fold_done, accum, s);
  }
  return fail(ASR_E_UNSUPPORTED, "bf16 block: C=%d not supported (16, 32, 64)", C);
}

}  // namespace asr

// test knob: force the stacked backward's grid (a grid larger than the
// resident capacity makes the in-launch hand-off run out and degrade to the
// post-launch reduction); 0 restores the default (one workgroup per CU)
extern "C" int asr_debug_stack_backward(int grid) {
  if (grid < 0 || grid > asr::kMaxBlockSlabs)
    return asr::fail(ASR_E_ARG, "asr_debug_stack_backward: grid must be in 0..%d", asr::kMaxBlockSlabs);
  asr::g_stack_grid_override = grid;
  return ASR_OK;
}

// host, blocking: waits of stacked-backward workgroups that ran out since the
// last reset (each one a slower launch, never a wrong gradient); reset != 0
// then clears the count (atomically with the read, on the device).  Each call
// has its own result word (concurrent callers never read each other's), and
// the launch status comes from hipLaunchKernel itself: no hipGetLastError,
// which would also report and clear an unrelated pending error.
extern "C" int asr_stack_status(int reset) {
  unsigned* d = nullptr;
  if (hipMalloc(&d, sizeof(unsigned)) != hipSuccess) return asr::fail(ASR_E_HIP, "asr_stack_status: hipMalloc failed");
  int rs = reset ? 1 : 0;
  void* args[] = {&rs, &d};
  hipError_t e = hipLaunchKernel((const void*)asr::blk::k_stack_status_take, dim3(1), dim3(1), args, 0, (hipStream_t)0);
  unsigned n = 0;
  if (e == hipSuccess) e = hipMemcpy(&n, d, sizeof(n), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) return asr::fail(ASR_E_HIP, "asr_stack_status: %s", hipGetErrorString(e));
  return (int)std::min<unsigned>(n, 0x7fffffffu);
}

#if ASR_STAMP_BUILD
extern "C" int asr_debug_stamps(void* host, size_t bytes) {
  if (bytes > sizeof(asr::blk::g_stamps)) bytes = sizeof(asr::blk::g_stamps);
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(asr::blk::g_stamps), bytes) == hipSuccess ? 0 : -4;
}
#endif
