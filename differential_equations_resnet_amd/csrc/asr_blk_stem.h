// The stem (conv1: 3 -> C channels, 3x3 SAME, + relu; C = 16 or 64, W = 32) on
// the bf16 matrix cores, for the bf16 networks (part of asr_block_mfma.hip's
// translation unit; the fp32 VALU stem kernels, any C and Cin, are in
// asr_stem_head.hip).  Both kernels are 256 threads, whole images per
// workgroup, the image staged in LDS as v - mean:
//   k_stem_fwd_mfma    one k-step (27 taps x channels padded to 32), W1 as bf16 hi + lo;
//   k_stem_wgrad_mfma  K = pixels, dz1 rows by LDS-DMA in 8-row bands, one
//                      [dW1 | db1] slab per workgroup;
//   k_stem_fwd_kxk, k_stem_wgrad_kxk  the 5 x 5 and 7 x 7 conv1 (C in {16, 32, 64}, W in {8, 16, 32}, any
//                      H), row bands instead of whole images: below the 3 x 3 kernels.
#pragma once
#include <type_traits>

#include "asr_blk_common.h"
#include "asr_common.h"
#include "asr_device.h"

namespace asr {
namespace blk {

// ===========================================================================
// Stem weight gradient on MFMA (C = 16 or 64, CIN=3, W=32, H % 8 == 0), from dz1 =
// dx1 * [x1 > 0] (written by the first block's backward, k_bwd3<..., RO> or k_bwd3_stack with ro0):
//   dW1[kappa][o] = inv_std * sum_p (img[p + tap] - mean)[ci] * dz1[p][o]
//   db1[o]        = sum_p dz1[p][o]
// (models/tfkeras_resnets.py:555-572: input normalisation, then the 3x3 SAME
// conv1 + relu).  K = pixels (one image row per k-step), M = kappa = tap*3 +
// ci (27, a row of ones at 27 for db1, padded to 32), N = o.  The image's
// im2col sits in LDS as a 32-channel tile of bf16 (v - mean): exact for u8
// input with a half-integer mean, so the bf16 products are exact and only
// the fp32 accumulation rounds.  dz1 rows stream in by LDS-DMA, 8-row bands
// double-buffered; both operands come from transposed LDS reads exactly as
// in the blocks' weight gradient.  One slab [dW1 (27*C) | db1 (C)] per WG.
// ===========================================================================
template <int C, typename Tin>
__global__ __launch_bounds__(256) void k_stem_wgrad_mfma(const Tin* __restrict__ img, const bf16* __restrict__ dz1,
                                                         int N, int H, float mean, float inv_std,
                                                         float* __restrict__ slabs) {
  constexpr int W = 32, CIN = 3, TW = W + 2, BRS = 8, KC = 9 * CIN, NT = C / 16;
  constexpr int IMROW = TW * 4 * 16, DZROW = TW * (C / 8) * 16, DZT = BRS * DZROW;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int IM = 0, DZ0 = H * IMROW, FT = DZ0 + 2 * DZT;  // im2col | 2 dz1 bands | staged image (fp32, halo)
  float* ft = (float*)(lds + FT);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, lx = lane & 15, tq = lx >> 2, tp = lx & 3;
  const int nbands = H / BRS;
  for (int i = tid; i < (H + 2) * TW * CIN; i += 256) ft[i] = 0.f;  // halo stays zero
  f32x4 acc[2][NT];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int n0 = blockIdx.x, items = ((N - n0 + (int)gridDim.x - 1) / (int)gridDim.x) * nbands;
  auto band_n = [&](int it) { return n0 + (it / nbands) * (int)gridDim.x; };
  auto dma_band = [&](int it, int buf) {
    dma_rows<C, W>(dz1, lds + DZ0 + buf * DZT, band_n(it), (it % nbands) * BRS, BRS, H, wave, 4, lane);
  };
  if (items > 0) dma_band(0, 0);
  for (int it = 0; it < items; ++it) {
    const int buf = it & 1, b = it % nbands;
    if (b == 0) {  // a new image: stage it (fp32, v - mean) and build its im2col
      const int n = band_n(it);
      __syncthreads();  // the previous image's im2col fully read
      const Tin* src = img + (long)n * H * W * CIN;
      for (int i = tid; i < H * W * CIN; i += 256) {
        const int ci = i % CIN, p = i / CIN;
        ft[((p / W + 1) * TW + p % W + 1) * CIN + ci] = (float)src[i] - mean;
      }
      __syncthreads();
      for (int p = tid; p < H * W; p += 256) {
        const int y = p / W, x = p % W;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          bf16x8 v;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int kap = 8 * q + j;
            float f = 0.f;
            if (kap < KC) {
              const int tap = kap / CIN, ci = kap % CIN;
              f = ft[((y + tap / 3) * TW + x + tap % 3) * CIN + ci];
            } else if (kap == KC) {
              f = 1.f;  // db1 row
            }
            v[j] = (bf16)f;
          }
          *(bf16x8*)(lds + IM + toff<32>(y, x + 1, q, TW)) = v;
        }
      }
    }
    barrier_vm(0);  // band it landed (and the im2col is written)
    if (it + 1 < items) dma_band(it + 1, buf ^ 1);
    const unsigned char* dzt = lds + DZ0 + buf * DZT;
#pragma unroll
    for (int k = 0; k < BRS / 4; ++k) {  // this wave's rows of the band
      const int r = wave + 4 * k, y = b * BRS + r;
      const int pb = 8 * g + tq;
      bf16x8 A[2], B[NT];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        const int q = 2 * mt + (tp >> 1);
        A[mt] = tr_pair(lds + IM + toff<32>(y, pb + 1, q, TW) + 8 * (tp & 1),
                        lds + IM + toff<32>(y, pb + 5, q, TW) + 8 * (tp & 1));
      }
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int q = 2 * nt + (tp >> 1);
        B[nt] = tr_pair(dzt + toff<C>(r, pb + 1, q, TW) + 8 * (tp & 1), dzt + toff<C>(r, pb + 5, q, TW) + 8 * (tp & 1));
      }
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[mt], B[nt], acc[mt][nt], 0, 0, 0);
    }
  }
  // the 4 waves' partials, summed in a fixed order (deterministic)
  barrier_vm(0);
  float* red = (float*)lds;  // [4 waves][32 m][C]
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int e = 0; e < 4; ++e) red[(wave * 32 + 16 * mt + 4 * g + e) * C + 16 * nt + lx] = acc[mt][nt][e];
  __syncthreads();
  float* slab = slabs + (long)blockIdx.x * (KC * C + C);
  for (int i = tid; i < (KC + 1) * C; i += 256) {
    const float v = (red[i] + red[32 * C + i]) + (red[2 * 32 * C + i] + red[3 * 32 * C + i]);
    slab[i] = i < KC * C ? v * inv_std : v;  // rows 0..26 dW1, row 27 db1
  }
}

// ===========================================================================
// Stem forward on MFMA (C = 16 or 64, CIN=3, W=32): x1 = relu(conv3x3((v - mean) *
// inv_std, W1) + b1), bf16 NHWC out (models/tfkeras_resnets.py:555-572).
// M = o (C/16 tiles), K = kappa = tap*3 + ci (27, padded to 32: one k-step),
// N = 16 pixels.  B: lane (pixel lx, kappa 8g..8g+7) gathers its 8 patch
// values from the image staged in LDS as fp32 v - mean (bf16-exact for u8
// input with a half-integer mean); A = inv_std * W1^T split into bf16 hi +
// lo parts held in registers (two MFMAs per tile: W1 to ~16 mantissa bits,
// so the result matches the fp32 VALU kernel to accumulation-order noise).
// Epilogue: + b1 (fp32), relu, bf16, 16-B stores at C=64 (a 16-lane row swap
// between o-tile pairs gives each lane 8 consecutive channels), 8-B stores at
// C=16 (one o-tile: 16 pixels x 32 B contiguous per tile).
// ===========================================================================
template <int C, typename Tin>
__global__ __launch_bounds__(256) void k_stem_fwd_mfma(const Tin* __restrict__ img, const float* __restrict__ w1,
                                                       const float* __restrict__ b1, int N, int H, float mean,
                                                       float inv_std, bf16* __restrict__ out) {
  constexpr int W = 32, CIN = 3, TW = W + 2, KC = 9 * CIN, MT = C / 16;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  float* ft = (float*)lds;  // staged image (fp32 v - mean), zero halo
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, lx = lane & 15;
  for (int i = tid; i < (H + 2) * TW * CIN; i += 256) ft[i] = 0.f;  // halo stays zero
  // A fragments: lane (o = 16 mt + lx, kappa 8g..8g+7), hi and lo bf16 parts
  bf16x8 Ah[MT], Al[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int kap = 8 * g + j;
      const float wv = kap < KC ? w1[kap * C + 16 * mt + lx] * inv_std : 0.f;
      const bf16 hi = (bf16)wv;
      Ah[mt][j] = hi;
      Al[mt][j] = (bf16)(wv - (float)hi);
    }
  float bz[MT][4];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int e = 0; e < 4; ++e) bz[mt][e] = b1 ? b1[16 * mt + 4 * g + e] : 0.f;
  // B operand: lane (pixel lx, kappa 8g..8g+7) read straight from the staged
  // image: tap (ky, kx), channel ci of kappa = offset (ky*TW + kx)*CIN + ci
  int koff[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int kap = min(8 * g + j, KC - 1), tap = kap / CIN, ci = kap % CIN;
    koff[j] = ((tap / 3) * TW + tap % 3) * CIN + ci;
  }
  for (int n = blockIdx.x; n < N; n += gridDim.x) {
    __syncthreads();  // the previous image fully read
    const Tin* src = img + (long)n * H * W * CIN;
    for (int i = tid; i < H * W * CIN; i += 256) {
      const int ci = i % CIN, p = i / CIN;
      ft[((p / W + 1) * TW + p % W + 1) * CIN + ci] = (float)src[i] - mean;
    }
    __syncthreads();
    // pixel tiles: wave w takes tiles w, w+4, ... (16 pixels of one row each)
    for (int pt = wave; pt < H * W / 16; pt += 4) {
      const int y = pt / (W / 16), x0 = (pt % (W / 16)) * 16;
      const float* pb = ft + (y * TW + x0 + lx) * CIN;
      bf16x8 B;
#pragma unroll
      for (int j = 0; j < 8; ++j) B[j] = (bf16)((8 * g + j < KC) ? pb[koff[j]] : 0.f);
      f32x4 acc[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        acc[mt] = f32x4{bz[mt][0], bz[mt][1], bz[mt][2], bz[mt][3]};
        acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah[mt], B, acc[mt], 0, 0, 0);
        acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Al[mt], B, acc[mt], 0, 0, 0);
      }
      // lane (g, lx): channels 16 mt + 4g + e of pixel x0 + lx
      u32x2 ov[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        bf16x4 o4;
#pragma unroll
        for (int e = 0; e < 4; ++e) o4[e] = (bf16)fmaxf(acc[mt][e], 0.f);
        ov[mt] = *(const u32x2*)&o4;
      }
      bf16* orow = out + (((long)n * H + y) * W + x0 + lx) * C;
      if constexpr (MT == 1) {
        *(u32x2*)(orow + 4 * g) = ov[0];
      } else {
#pragma unroll
        for (int mp = 0; mp < MT / 2; ++mp) {  // o-tiles 2mp, 2mp+1 -> lane row g: channels 16(2mp + (g&1)) + 8(g>>1)
          const auto s0 = __builtin_amdgcn_permlane16_swap(ov[2 * mp][0], ov[2 * mp + 1][0], false, false);
          const auto s1 = __builtin_amdgcn_permlane16_swap(ov[2 * mp][1], ov[2 * mp + 1][1], false, false);
          *(u32x4*)(orow + 16 * (2 * mp + (g & 1)) + 8 * (g >> 1)) = u32x4{s0[0], s1[0], s0[1], s1[1]};
        }
      }
    }
  }
}

// ===========================================================================
// The K x K stem, K = 5 or 7 (conv1 of get_single_block_resnet_build_function(kernel_size = K),
// models/tfkeras_resnets.py:563-572), for the bf16 networks: CIN = 3, C in {16, 32, 64}, W in {8, 16, 32},
// any H >= 1.  The numerical contract of the 3 x 3 kernels above: the image staged in LDS as fp32 v - mean with
// a zero halo of K/2 (bf16-exact for u8 input with a half-integer mean), inv_std * W1 as bf16 hi + lo, fp32
// accumulation, bias and relu.  Both kernels are 256 threads and walk (image, row band) items; a band is
// staged with its K - 1 halo rows, so H is free and no im2col is kept (at K = 7 a 32 x 32 image's would be
// 350 KB): the patch operand is gathered from the staged image, 8 values per lane and k-step.
// ===========================================================================
template <int W_, int K>
struct StemK {
  static constexpr int W = W_, CIN = 3, KC = K * K * CIN, TW = W + K - 1;
  static constexpr int KS = (KC + 31) / 32;      // forward k-steps: 3 (75 -> 96) at K = 5, 5 (147 -> 160) at K = 7
  static constexpr int BRF = 512 / W;            // forward band: 512 pixels = 32 tiles of 16, 8 a wave
  static constexpr int BRW = 256 / W;            // weight-gradient band: 256 pixels = 8 chunks of 32
  static constexpr int MT = (KC + 1 + 15) / 16;  // weight-gradient m-tiles (kappa and the ones row): 5 / 10
  static constexpr int MTW = (MT + 3) / 4;       // ... of one wave (tiles wave, wave + 4, ...)
};

// band rows y0 - K/2 .. of image n -> ft [ROWS][TW][3] (fp32 v - mean, zeros outside the image)
template <int W, int K, int ROWS, typename Tin>
__device__ __forceinline__ void stemk_stage(const Tin* __restrict__ img, int n, int y0, int H, float mean,
                                            float* __restrict__ ft, int tid) {
  constexpr int CIN = 3, TW = W + K - 1, R = K / 2;
  for (int i = tid; i < ROWS * TW * CIN; i += 256) {
    const int ci = i % CIN, c = (i / CIN) % TW, r = i / (CIN * TW);
    const int gy = y0 + r - R, gx = c - R;
    float v = 0.f;
    if ((unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W)
      v = (float)img[(((long)n * H + gy) * W + gx) * CIN + ci] - mean;
    ft[i] = v;
  }
}

// Forward: x1 = relu(conv_KxK((v - mean) * inv_std, W1) + b1), bf16 NHWC.  M = o, reduction kappa = tap * 3 + ci
// in KS k-steps, N = 16 pixels (pixel 16 tile + lx of the band: a tile spans two rows at W = 8).  The A
// fragments (hi + lo of every o-tile and k-step: 160 VGPRs at C = 64, K = 7) stay in registers: the 4 waves of
// a workgroup run one per SIMD.  Two MFMAs per o-tile and k-step; the epilogue of k_stem_fwd_mfma.
template <int C, int W, int K, typename Tin>
__global__ __launch_bounds__(256) void k_stem_fwd_kxk(const Tin* __restrict__ img, const float* __restrict__ w1,
                                                      const float* __restrict__ b1, int N, int H, float mean,
                                                      float inv_std, bf16* __restrict__ out) {
  using G = StemK<W, K>;
  constexpr int CIN = 3, TW = G::TW, KC = G::KC, KS = G::KS, MT = C / 16, BR = G::BRF, ROWS = BR + K - 1;
  __shared__ float ft[ROWS * TW * CIN];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, lx = lane & 15;
  bf16x8 Ah[MT][KS], Al[MT][KS];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int kap = 32 * ks + 8 * g + j;
        const float wv = kap < KC ? w1[kap * C + 16 * mt + lx] * inv_std : 0.f;
        const bf16 hi = (bf16)wv;
        Ah[mt][ks][j] = hi;
        Al[mt][ks][j] = (bf16)(wv - (float)hi);
      }
  float bz[MT][4];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int e = 0; e < 4; ++e) bz[mt][e] = b1 ? b1[16 * mt + 4 * g + e] : 0.f;
  int koff[KS][8];  // tap (ky, kx), channel ci of kappa -> offset in ft from the pixel's own (row, col)
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int kap = min(32 * ks + 8 * g + j, KC - 1), tap = kap / CIN, ci = kap % CIN;
      koff[ks][j] = ((tap / K) * TW + tap % K) * CIN + ci;
    }
  const int nb = (H + BR - 1) / BR;
  const long items = (long)N * nb;
  for (long item = blockIdx.x; item < items; item += gridDim.x) {
    const int n = (int)(item / nb), y0 = (int)(item % nb) * BR;
    __syncthreads();  // the previous band fully read
    stemk_stage<W, K, ROWS>(img, n, y0, H, mean, ft, tid);
    __syncthreads();
    const int rows = min(BR, H - y0), ntiles = (rows * W + 15) / 16;
    for (int pt = wave; pt < ntiles; pt += 4) {
      const int p = 16 * pt + lx, yl = p / W, x = p % W;  // (yl <= BR - 1: the staged rows cover its patch)
      const float* pb = ft + (yl * TW + x) * CIN;
      bf16x8 B[KS];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) B[ks][j] = (bf16)((32 * ks + 8 * g + j < KC) ? pb[koff[ks][j]] : 0.f);
      f32x4 acc[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        acc[mt] = f32x4{bz[mt][0], bz[mt][1], bz[mt][2], bz[mt][3]};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah[mt][ks], B[ks], acc[mt], 0, 0, 0);
          acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Al[mt][ks], B[ks], acc[mt], 0, 0, 0);
        }
      }
      // lane (g, lx): channels 16 mt + 4g + e of pixel p
      u32x2 ov[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        bf16x4 o4;
#pragma unroll
        for (int e = 0; e < 4; ++e) o4[e] = (bf16)fmaxf(acc[mt][e], 0.f);
        ov[mt] = *(const u32x2*)&o4;
      }
      const bool live = y0 + yl < H;  // (a partial last tile: pixels past the band's rows)
      bf16* orow = out + (((long)n * H + y0 + yl) * W + x) * C;
      if constexpr (MT == 1) {
        if (live) *(u32x2*)(orow + 4 * g) = ov[0];
      } else {
#pragma unroll
        for (int mp = 0; mp < MT / 2; ++mp) {  // o-tiles 2mp, 2mp+1 -> lane row g: channels 16(2mp + (g&1)) + 8(g>>1)
          const auto s0 = __builtin_amdgcn_permlane16_swap(ov[2 * mp][0], ov[2 * mp + 1][0], false, false);
          const auto s1 = __builtin_amdgcn_permlane16_swap(ov[2 * mp][1], ov[2 * mp + 1][1], false, false);
          if (live) *(u32x4*)(orow + 16 * (2 * mp + (g & 1)) + 8 * (g >> 1)) = u32x4{s0[0], s1[0], s0[1], s1[1]};
        }
      }
    }
  }
}

// Weight gradient, from dz1 = dx1 * [x1 > 0] (bf16):
//   dW1[kappa][o] = inv_std * sum_p (img[p + tap] - mean)[ci] * dz1[p][o],   db1[o] = sum_p dz1[p][o]
// K = pixels (chunks of 32 of a 256-pixel band), M = kappa (the ones row of db1 at kappa = K*K*3, inside the
// padding), N = o.  dz1's band sits in LDS pixel-major (C + 8 channels a pixel) and is read with
// ds_read_b64_tr_b16: lane (g, lx) gets channel lx of pixels 4g .. 4g + 3 and 16 + 4g .. 16 + 4g + 3 of the
// chunk, and gathers the same 8 pixels of its kappa row from the staged image.  The MT m-tiles are dealt to the
// 4 waves (tiles wave, wave + 4, ...), each wave over every o-tile: no cross-wave reduction.  A workgroup keeps
// its accumulators over a contiguous run of items and writes one [dW1 | db1] slab: a fixed order of sums.
template <int C, int W, int K, typename Tin>
__global__ __launch_bounds__(256) void k_stem_wgrad_kxk(const Tin* __restrict__ img, const bf16* __restrict__ dz1,
                                                        int N, int H, float mean, float inv_std,
                                                        float* __restrict__ slabs) {
  using G = StemK<W, K>;
  constexpr int CIN = 3, TW = G::TW, KC = G::KC, MT = G::MT, MTW = G::MTW, NT = C / 16, BR = G::BRW;
  constexpr int ROWS = BR + K - 1, PS = C + 8, C8 = C / 8, NPX = BR * W;
  __shared__ float ft[ROWS * TW * CIN];
  __shared__ __attribute__((aligned(16))) bf16 dzt[NPX * PS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, lx = lane & 15, q = lx >> 2, pq = lx & 3;
  int koff[MTW], kind[MTW];  // kind 0: an image value, 1: the ones row, 2: padding
#pragma unroll
  for (int i = 0; i < MTW; ++i) {
    const int mt = wave + 4 * i, kap = 16 * mt + lx;
    const int kc = min(kap, KC - 1), tap = kc / CIN, ci = kc % CIN;
    koff[i] = ((tap / K) * TW + tap % K) * CIN + ci;
    kind[i] = (mt < MT && kap < KC) ? 0 : (mt < MT && kap == KC) ? 1 : 2;
  }
  f32x4 acc[MTW][NT];
#pragma unroll
  for (int i = 0; i < MTW; ++i)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[i][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  const int nb = (H + BR - 1) / BR;
  const long items = (long)N * nb;
  const long i0 = (long)blockIdx.x * items / gridDim.x, i1 = (long)(blockIdx.x + 1) * items / gridDim.x;
  for (long item = i0; item < i1; ++item) {
    const int n = (int)(item / nb), y0 = (int)(item % nb) * BR;
    __syncthreads();  // the previous band fully read
    stemk_stage<W, K, ROWS>(img, n, y0, H, mean, ft, tid);
    const bf16* src = dz1 + ((long)n * H + y0) * W * C;  // the band's rows are contiguous: 16-B chunk i = (pixel, c8)
    for (int i = tid; i < NPX * C8; i += 256) {
      const int P = i / C8, c8 = i % C8;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (y0 + P / W < H) v = *(const uint4*)(src + 8L * i);
      *(uint4*)(dzt + P * PS + 8 * c8) = v;
    }
    __syncthreads();
    const int rows = min(BR, H - y0), nch = (rows * W + 31) / 32;  // (32 nch <= NPX: every pixel read is staged)
    for (int ch = 0; ch < nch; ++ch) {
      const int k1 = 32 * ch + 4 * g + q;  // the pixel whose 8-B piece this lane addresses (and 16 further)
      bf16x8 B[NT];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ASR_LDS s16x4*)(dzt + k1 * PS + 16 * nt + 4 * pq));
        const s16x4 b =
            __builtin_amdgcn_ds_read_tr16_b64_v4i16((ASR_LDS s16x4*)(dzt + (k1 + 16) * PS + 16 * nt + 4 * pq));
        const s16x8 c = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
        B[nt] = __builtin_bit_cast(bf16x8, c);
      }
      const int pa = 32 * ch + 4 * g, pb = pa + 16;  // this lane's two runs of 4 pixels (4 | W: each within a row)
      const float* fa = ft + ((pa / W) * TW + pa % W) * CIN;
      const float* fb = ft + ((pb / W) * TW + pb % W) * CIN;
#pragma unroll
      for (int i = 0; i < MTW; ++i) {
        if (wave + 4 * i < MT) {  // (wave-uniform)
          bf16x8 A;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            A[j] = (bf16)(kind[i] == 0 ? fa[CIN * j + koff[i]] : kind[i] == 1 ? 1.f : 0.f);
            A[4 + j] = (bf16)(kind[i] == 0 ? fb[CIN * j + koff[i]] : kind[i] == 1 ? 1.f : 0.f);
          }
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
            acc[i][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A, B[nt], acc[i][nt], 0, 0, 0);
        }
      }
    }
  }
  mfma_bf16_settle();
  // D row 4g + e = kappa 16 mt + 4g + e, column lx = o 16 nt + lx; slab [dW1 (KC x C) | db1 (C)]
  float* slab = slabs + (long)blockIdx.x * (KC * C + C);
#pragma unroll
  for (int i = 0; i < MTW; ++i)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int m = 16 * (wave + 4 * i) + 4 * g + e;
        if (m <= KC) slab[m * C + 16 * nt + lx] = m < KC ? acc[i][nt][e] * inv_std : acc[i][nt][e];
      }
}

}  // namespace blk
}  // namespace asr
