// Image-resident stages: all L Euler blocks of a small stage in one launch, a
// workgroup per image with the image in LDS, in bf16 (k_stagef / k_stageb) and
// in fp32 (k_stagef32 / k_stageb32), behind stage_img_forward /
// stage_img_backward; wgrad_layers runs the stage's weight gradients in one
// launch on the block kernels' k_wgradb (asr_conv_bf16.hip) or k_wgrad32
// (asr_conv_f32.hip).
#include "asr_common.h"
#include "asr_conv3x3.h"
#include "asr_internal.h"

namespace asr {

// ===========================================================================
// Image-resident bf16 stages (k_stagef / k_stageb): all L Euler blocks of a
// 16 x 16 x 32 or 8 x 8 x 64 stage in one launch, a workgroup per image with
// the image in LDS (20.3 / 12.5 KiB with its zero halo), as the deep16 kernels
// do for 32 x 32 x 16.  The conv is k_convb's (v_mfma_f32_16x16x32_bf16, the
// layer's A fragments in registers, B one 16-B LDS read per k-step); between
// layers only LDS traffic and a barrier.
//   forward: ping-pong image buffers; each layer's y and relu mask to HBM (the
//     backward reads them), y into the other buffer;
//   backward (input gradient only): dy in LDS, dz = dy & mask_l into the halo
//     tile, dx = dy - h conv(dz) + 2 gamma h dz written over dy in place (a lane
//     reads and writes only its own pixel's channels); the gradient entering
//     each layer below the top goes to HBM for the weight gradient (k_wgradb
//     per layer, unchanged), dx_0 at the end.
// ===========================================================================
template <int C, int W_>
struct StImg {
  static constexpr int NW = 4, NTH = 64 * NW;  // waves per image
  static constexpr int W = W_, H = W_, TW = W + 2, OT = C / 16, WPT = NW / OT, KS = (9 * C + 31) / 32, C8 = C / 8;
  static constexpr int T = H * W / 16;              // 16-pixel tiles per image
  static_assert((T / WPT) % 2 == 0, "image-resident stage: a wave's tiles come in pairs (two MFMA chains)");
  static constexpr int PS = C + 8;          // a pixel's elements in LDS (padded, as BfBand)
  static constexpr int IMGE = (H + 2) * TW * PS;    // elements of a haloed image tile
  static constexpr int NCH = H * W * C8;            // 16-B chunks of an image
  static_assert((W == 16 && C == 32) || (W == 8 && C == 64) || (W == 8 && C == 32),
                "image-resident stage: 16 x 16 x 32, 8 x 8 x 32 or 8 x 8 x 64");
};

template <int C, int W>
__device__ __forceinline__ int st_off(int r, int c) {  // element offset of interior pixel (r, c) in a haloed tile
  return ((r + 1) * StImg<C, W>::TW + c + 1) * StImg<C, W>::PS;
}

// an LDS-only workgroup barrier: the layers' global stores (y, masks, dy) stay in flight across it
// (__syncthreads waits for them too: a full store round trip per layer)
__device__ __forceinline__ void st_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// an image's NCH 16-B chunks from global into LDS, put(i, v) storing chunk i: every load of a thread
// issued before its first store (a load-store loop waited for each load in turn)
template <int NCH, int NTH, typename V, typename T, typename Put>
__device__ __forceinline__ void st_fetch_image(const T* __restrict__ src, int tid, Put put) {
  constexpr int NPT = (NCH + NTH - 1) / NTH, EPC = 16 / (int)sizeof(T);
  V v[NPT];
#pragma unroll
  for (int k = 0; k < NPT; ++k) {
    const int i = tid + k * NTH;
    if (i < NCH) v[k] = *(const V*)(src + (long)EPC * i);
  }
#pragma unroll
  for (int k = 0; k < NPT; ++k) {
    const int i = tid + k * NTH;
    if (i < NCH) put(i, v[k]);
  }
}

constexpr int kStIpw = 1;
// IPW images per workgroup: 1 (a wave's two MFMA chains are two tiles of the image); 2 (the chains are
// one tile of each image, the layer's A fragments shared) measured -7 % (r05ar: half the workgroups)
template <int C, int W>
__global__ __launch_bounds__((StImg<C, W>::NTH)) void k_stagef(const bf16* __restrict__ x0, bf16* __restrict__ ys, long y_stride,
                                                uint8_t* __restrict__ masks, long mask_stride,
                                                const bf16* __restrict__ wpack, long w_stride,
                                                const float* __restrict__ bias, long bias_stride, float h, int N,
                                                int L) {
  using G = StImg<C, W>;
  constexpr int TW = G::TW, KS = G::KS, OT = G::OT, IPW = kStIpw, TP = 2 / IPW;
  extern __shared__ __attribute__((aligned(16))) bf16 lds_stf[];  // [IPW][2][IMGE]
  auto imgb = [&](int im, int pp) { return lds_stf + (im * 2 + pp) * G::IMGE; };
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, lx = lane & 15;
  const int ot = wave % OT, rw = wave / OT;
  for (int i = tid; i < IPW * 2 * G::IMGE / 8; i += G::NTH) ((uint4*)lds_stf)[i] = make_uint4(0u, 0u, 0u, 0u);
  st_barrier();
  for (int n0 = IPW * blockIdx.x; n0 < N; n0 += IPW * gridDim.x) {
    const int nimg = min(IPW, N - n0);  // (uniform)
    for (int im = 0; im < nimg; ++im) {
      const long ib = (long)(n0 + im) * G::H * W * C;
      bf16* dst = imgb(im, 0);
      st_fetch_image<G::NCH, G::NTH, uint4>(x0 + ib, tid, [&](int i, const uint4& v) {
        const int px = i / G::C8, c8 = i % G::C8;
        *(uint4*)(dst + st_off<C, W>(px / W, px % W) + 8 * c8) = v;
      });
    }
    st_barrier();
    for (int l = 0; l < L; ++l) {
      bf16x8 A[KS];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        A[ks] = *(const bf16x8*)(wpack + (long)l * w_stride + (((long)ot * KS + ks) * 64 + lane) * 8);
      const f32x4 bz = *(const f32x4*)(bias + (long)l * bias_stride + 16 * ot + 4 * g);
      uint8_t* ml = masks + (long)l * mask_stride;
      auto epi = [&](int im, int p, const f32x4& acc) {
        const bf16* cur = imgb(im, l & 1);
        bf16* nxt = imgb(im, (l & 1) ^ 1);
        const long n = n0 + im;
        const int r = p / W, px = p % W;
        const int co = st_off<C, W>(r, px) + 16 * ot + 4 * g;
        const uint2 cw = *(const uint2*)(cur + co);
        const float ctr[4] = {__uint_as_float(cw.x << 16), __uint_as_float(cw.x & 0xffff0000u),
                              __uint_as_float(cw.y << 16), __uint_as_float(cw.y & 0xffff0000u)};
        float v[4];
        unsigned nib = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          nib |= (acc[e] > 0.f ? 1u : 0u) << e;
          v[e] = fmaf(h, fmaxf(acc[e], 0.f), ctr[e]);
        }
        const uint2 yw = make_uint2(pk_bf16_rn(v[0], v[1]), pk_bf16_rn(v[2], v[3]));
        *(uint2*)(nxt + co) = yw;
        const long pix = n * G::H * W + p;
        *(uint2*)(ys + (long)l * y_stride + pix * C + 16 * ot + 4 * g) = yw;
        unsigned m = nib << (4 * g);
        m |= (unsigned)__shfl_xor((int)m, 16, 64);
        m |= (unsigned)__shfl_xor((int)m, 32, 64);
        if (g == 0) *(uint16_t*)(ml + (pix * C + 16 * ot) / 8) = (uint16_t)m;
      };
#pragma unroll 1
      for (int j = 0; j < G::T / G::WPT; j += TP) {
        int pc[2], rc[2], xc[2];
        const bf16* bc[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {  // chain c: image c / TP, tile j + c % TP
          pc[c] = 16 * (rw + (j + c % TP) * G::WPT) + lx;
          rc[c] = pc[c] / W;
          xc[c] = pc[c] % W;
          bc[c] = imgb(c / TP, l & 1);
        }
        f32x4 acc[2] = {bz, bz};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const int kap = 32 * ks + 8 * g;
          const int t = min(kap / C, 8), i0c = kap - (kap / C) * C;
          uint4 b[2];
#pragma unroll
          for (int c = 0; c < 2; ++c)
            b[c] = *(const uint4*)(bc[c] + ((rc[c] + t / 3) * TW + xc[c] + t % 3) * G::PS + i0c);
#pragma unroll
          for (int c = 0; c < 2; ++c)
            acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[ks], __builtin_bit_cast(bf16x8, b[c]), acc[c], 0, 0, 0);
        }
        mfma_bf16_settle();
#pragma unroll
        for (int c = 0; c < 2; ++c)
          if (c / TP < nimg) epi(c / TP, pc[c], acc[c]);
      }
      st_barrier();  // layer l's outputs complete; the inputs free
    }
  }
}

template <int C, int W>
__global__ __launch_bounds__((StImg<C, W>::NTH)) void k_stageb(const bf16* __restrict__ dyL, bf16* __restrict__ dys, long d_stride,
                                                bf16* __restrict__ dx0, const uint8_t* __restrict__ masks,
                                                long mask_stride, const bf16* __restrict__ wpack, long w_stride,
                                                float h, float two_gamma, int N, int L) {
  using G = StImg<C, W>;
  constexpr int TW = G::TW, KS = G::KS, OT = G::OT, IPW = kStIpw, TP = 2 / IPW;
  constexpr int DYE = G::H * W * G::PS;
  extern __shared__ __attribute__((aligned(16))) bf16 lds_stb[];  // [IPW][dz (haloed) | dy]
  auto dzb = [&](int im) { return lds_stb + im * (G::IMGE + DYE); };
  auto dyb = [&](int im) { return lds_stb + im * (G::IMGE + DYE) + G::IMGE; };
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, lx = lane & 15;
  const int ot = wave % OT, rw = wave / OT;
  const float hg = h * two_gamma;
  for (int i = tid; i < IPW * (G::IMGE + DYE) / 8; i += G::NTH) ((uint4*)lds_stb)[i] = make_uint4(0u, 0u, 0u, 0u);
  for (int n0 = IPW * blockIdx.x; n0 < N; n0 += IPW * gridDim.x) {
    const int nimg = min(IPW, N - n0);  // (uniform)
    st_barrier();  // (the previous images' dx read out)
    for (int im = 0; im < nimg; ++im) {
      const long ib = (long)(n0 + im) * G::H * W * C;
      bf16* dst = dyb(im);
      st_fetch_image<G::NCH, G::NTH, uint4>(dyL + ib, tid, [&](int i, const uint4& v) {
        *(uint4*)(dst + (i / G::C8) * G::PS + 8 * (i % G::C8)) = v;
      });
    }
    for (int l = L - 1; l >= 0; --l) {
      bf16x8 A[KS];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        A[ks] = *(const bf16x8*)(wpack + (long)l * w_stride + (((long)ot * KS + ks) * 64 + lane) * 8);
      // layer l's relu bits, loaded before the barrier (a byte load per chunk inside the loop below
      // waited for each in turn)
      const uint8_t* ml = masks + (long)l * mask_stride;
      constexpr int NPT = (G::NCH + G::NTH - 1) / G::NTH;
      unsigned mb[IPW][NPT];
#pragma unroll
      for (int im = 0; im < IPW; ++im)
#pragma unroll
        for (int k = 0; k < NPT; ++k) {
          const int i = tid + k * G::NTH;
          mb[im][k] = (im < nimg && i < G::NCH) ? ml[((long)(n0 + im) * G::H * W * C + 8L * i) >> 3] : 0u;
        }
      st_barrier();  // dy of layer l complete (loaded, or the previous layer's dx); dz free
      for (int im = 0; im < nimg; ++im) {
        const long ib = (long)(n0 + im) * G::H * W * C;
#pragma unroll
        for (int k = 0; k < NPT; ++k) {
          const int i = tid + k * G::NTH;
          if (i >= G::NCH) break;
          const int px = i / G::C8, c8 = i % G::C8;
          const uint4 v = *(const uint4*)(dyb(im) + px * G::PS + 8 * c8);
          *(uint4*)(dys + (long)l * d_stride + ib + 8L * i) = v;  // the gradient entering layer l (its wgrad's dy)
          *(uint4*)(dzb(im) + st_off<C, W>(px / W, px % W) + 8 * c8) = mask8_bf16(v, mb[im][k]);
        }
      }
      st_barrier();  // dz complete
      auto epi = [&](int im, int p, const f32x4& acc) {
        const int r = p / W, px = p % W;
        const int cz = st_off<C, W>(r, px) + 16 * ot + 4 * g, cy = p * G::PS + 16 * ot + 4 * g;
        const uint2 zw = *(const uint2*)(dzb(im) + cz), dw = *(const uint2*)(dyb(im) + cy);
        const float z4[4] = {__uint_as_float(zw.x << 16), __uint_as_float(zw.x & 0xffff0000u),
                             __uint_as_float(zw.y << 16), __uint_as_float(zw.y & 0xffff0000u)};
        const float d4[4] = {__uint_as_float(dw.x << 16), __uint_as_float(dw.x & 0xffff0000u),
                             __uint_as_float(dw.y << 16), __uint_as_float(dw.y & 0xffff0000u)};
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaf(hg, z4[e], fmaf(-h, acc[e], d4[e]));
        *(uint2*)(dyb(im) + cy) = make_uint2(pk_bf16_rn(v[0], v[1]), pk_bf16_rn(v[2], v[3]));  // (own pixel, own channels)
      };
#pragma unroll 1
      for (int j = 0; j < G::T / G::WPT; j += TP) {
        int pc[2], rc[2], xc[2];
        const bf16* bc[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          pc[c] = 16 * (rw + (j + c % TP) * G::WPT) + lx;
          rc[c] = pc[c] / W;
          xc[c] = pc[c] % W;
          bc[c] = dzb(c / TP);
        }
        f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const int kap = 32 * ks + 8 * g;
          const int t = min(kap / C, 8), i0c = kap - (kap / C) * C;
          uint4 b[2];
#pragma unroll
          for (int c = 0; c < 2; ++c)
            b[c] = *(const uint4*)(bc[c] + ((rc[c] + t / 3) * TW + xc[c] + t % 3) * G::PS + i0c);
#pragma unroll
          for (int c = 0; c < 2; ++c)
            acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[ks], __builtin_bit_cast(bf16x8, b[c]), acc[c], 0, 0, 0);
        }
        mfma_bf16_settle();
#pragma unroll
        for (int c = 0; c < 2; ++c)
          if (c / TP < nimg) epi(c / TP, pc[c], acc[c]);
      }
    }
    st_barrier();  // dx_0 complete
    for (int im = 0; im < nimg; ++im) {
      const long ib = (long)(n0 + im) * G::H * W * C;
      for (int i = tid; i < G::NCH; i += G::NTH)
        *(uint4*)(dx0 + ib + 8L * i) = *(const uint4*)(dyb(im) + (i / G::C8) * G::PS + 8 * (i % G::C8));
    }
  }
}

// ---------------------------------------------------------------------------
// The fp32 image-resident stages (k_stagef32 / k_stageb32: the reference's
// precision, v_mfma_f32_16x16x4_f32): the same structure as k_stagef /
// k_stageb with fp32 image tiles (pixel stride C + 4 floats, dynamic LDS) and
// the fp32 block's conventions: W in HWIO fp32, A = W^T fragments of the
// wave's o-tile in registers (k_conv32's), dz = h dy [relu bit] staged in
// fp32, dx = dy - conv(dz) + 2 gamma dz.
// ---------------------------------------------------------------------------
template <int C, int W_>
struct StImg32 {
  // NW waves per image: the fp32 MFMA is 4x the bf16's cycles per FLOP, and at the reference's batch
  // sizes (128) one 4-wave workgroup per image would leave half the SIMDs idle
  static constexpr int NW = 4, NTH = 64 * NW;
  static constexpr int W = W_, H = W_, TW = W + 2, OT = C / 16, OQ = C / 16, WPT = NW / OT, PS = C + 4;
  static constexpr int T = H * W / 16, IMGF = (H + 2) * TW * PS, NCH = H * W * C / 4;
  static_assert((W == 16 && C == 32) || (W == 8 && C == 64), "fp32 image-resident stage: 16 x 16 x 32 or 8 x 8 x 64");
};

template <int C, int W>
__device__ __forceinline__ int st32_off(int r, int c) {
  return ((r + 1) * StImg32<C, W>::TW + c + 1) * StImg32<C, W>::PS;
}

template <int C, int W>
__global__ __launch_bounds__((StImg32<C, W>::NTH)) void k_stagef32(const float* __restrict__ x0, float* __restrict__ ys, long y_stride,
                                                  uint8_t* __restrict__ masks, long mask_stride,
                                                  const float* __restrict__ w, long w_stride,
                                                  const float* __restrict__ bias, long bias_stride, float h, int N,
                                                  int L) {
  using G = StImg32<C, W>;
  constexpr int TW = G::TW, OQ = G::OQ, OT = G::OT, PS = G::PS;
  extern __shared__ __attribute__((aligned(16))) float lds_sf[];
  float* img0 = lds_sf;
  float* img1 = lds_sf + G::IMGF;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, lx = lane & 15;
  const int ot = wave % OT, rw = wave / OT;
  for (int i = tid; i < 2 * G::IMGF / 4; i += G::NTH) ((f32x4*)lds_sf)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  __syncthreads();
  for (int n = blockIdx.x; n < N; n += gridDim.x) {
    const long ib = (long)n * G::H * W * C;
    st_fetch_image<G::NCH, G::NTH, f32x4>(x0 + ib, tid, [&](int i, const f32x4& v) {
      const int px = i / (C / 4), c4 = i % (C / 4);
      *(f32x4*)(img0 + st32_off<C, W>(px / W, px % W) + 4 * c4) = v;
    });
    __syncthreads();
    for (int l = 0; l < L; ++l) {
      const float* cur = (l & 1) ? img1 : img0;
      float* nxt = (l & 1) ? img0 : img1;
      const float* wl = w + (long)l * w_stride;
      float A[9][OQ][4];
#pragma unroll
      for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int q = 0; q < OQ; ++q)
#pragma unroll
          for (int s4 = 0; s4 < 4; ++s4) A[t][q][s4] = wl[((long)t * C + 16 * q + 4 * g + s4) * C + 16 * ot + lx];
      const f32x4 bz = *(const f32x4*)(bias + (long)l * bias_stride + 16 * ot + 4 * g);
      float* yl = ys + (long)l * y_stride + ib;
      uint8_t* ml = masks + (long)l * mask_stride;
      auto epi = [&](int p, const f32x4& acc) {
        const int r = p / W, px = p % W;
        const int co = st32_off<C, W>(r, px) + 16 * ot + 4 * g;
        const f32x4 ctr = *(const f32x4*)(cur + co);
        f32x4 v;
        unsigned nib = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          nib |= (acc[e] > 0.f ? 1u : 0u) << e;
          v[e] = ctr[e] + h * fmaxf(acc[e], 0.f);
        }
        *(f32x4*)(nxt + co) = v;
        *(f32x4*)(yl + (long)p * C + 16 * ot + 4 * g) = v;
        const long pix = (long)n * G::H * W + p;
        unsigned m = nib << (4 * g);
        m |= (unsigned)__shfl_xor((int)m, 16, 64);
        m |= (unsigned)__shfl_xor((int)m, 32, 64);
        if (g == 0) *(uint16_t*)(ml + (pix * C + 16 * ot) / 8) = (uint16_t)m;
      };
#pragma unroll 1
      for (int j = 0; j < G::T / G::WPT; j += 2) {
        const int p0 = 16 * (rw + j * G::WPT) + lx, p1 = 16 * (rw + (j + 1) * G::WPT) + lx;
        const int r0 = p0 / W, x0p = p0 % W, r1 = p1 / W, x1p = p1 % W;
        f32x4 acc0 = bz, acc1 = bz;
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
          for (int q = 0; q < OQ; ++q) {
            const f32x4 b0 = *(const f32x4*)(cur + ((r0 + t / 3) * TW + x0p + t % 3) * PS + 16 * q + 4 * g);
            const f32x4 b1 = *(const f32x4*)(cur + ((r1 + t / 3) * TW + x1p + t % 3) * PS + 16 * q + 4 * g);
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
              acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(A[t][q][s4], b0[s4], acc0, 0, 0, 0);
              acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(A[t][q][s4], b1[s4], acc1, 0, 0, 0);
            }
          }
        mfma_f32_settle();
        epi(p0, acc0);
        epi(p1, acc1);
      }
      st_barrier();  // layer l's outputs complete in nxt; cur free
    }
  }
}

template <int C, int W>
__global__ __launch_bounds__((StImg32<C, W>::NTH)) void k_stageb32(const float* __restrict__ dyL, float* __restrict__ dys, long d_stride,
                                                  float* __restrict__ dx0, const uint8_t* __restrict__ masks,
                                                  long mask_stride, const float* __restrict__ w, long w_stride,
                                                  float h, float two_gamma, int N, int L) {
  using G = StImg32<C, W>;
  constexpr int TW = G::TW, OQ = G::OQ, OT = G::OT, PS = G::PS;
  extern __shared__ __attribute__((aligned(16))) float lds_sb[];
  float* dzt = lds_sb;              // dz = h dy [relu bit], zero halo
  float* dyt = lds_sb + G::IMGF;    // dy (becomes dx), pixel stride PS
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, lx = lane & 15;
  const int ot = wave % OT, rw = wave / OT;
  for (int i = tid; i < G::IMGF / 4; i += G::NTH) ((f32x4*)dzt)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int n = blockIdx.x; n < N; n += gridDim.x) {
    const long ib = (long)n * G::H * W * C;
    st_fetch_image<G::NCH, G::NTH, f32x4>(dyL + ib, tid, [&](int i, const f32x4& v) {
      *(f32x4*)(dyt + (i / (C / 4)) * PS + 4 * (i % (C / 4))) = v;
    });
    for (int l = L - 1; l >= 0; --l) {
      // layer l's relu bytes, loaded before the barrier (a byte load per chunk inside the loop below
      // waited for each in turn)
      const uint8_t* ml = masks + (long)l * mask_stride;
      constexpr int NPT = (G::NCH + G::NTH - 1) / G::NTH;
      unsigned mb[NPT];
#pragma unroll
      for (int k = 0; k < NPT; ++k) {
        const int i = tid + k * G::NTH;
        mb[k] = i < G::NCH ? ml[(ib + 4L * i) >> 3] : 0u;
      }
      st_barrier();  // dy of layer l complete; dz free
#pragma unroll
      for (int k = 0; k < NPT; ++k) {
        const int i = tid + k * G::NTH;
        if (i >= G::NCH) break;
        const int px = i / (C / 4), c4 = i % (C / 4);
        const f32x4 v = *(const f32x4*)(dyt + px * PS + 4 * c4);
        *(f32x4*)(dys + (long)l * d_stride + ib + 4L * i) = v;  // the gradient entering layer l (its wgrad's dy)
        const unsigned nib = mb[k] >> ((ib + 4L * i) & 7);  // (masked_dz4's bits: pixel * C + channel)
        f32x4 z;
#pragma unroll
        for (int j = 0; j < 4; ++j) z[j] = ((nib >> j) & 1u) ? h * v[j] : 0.f;
        *(f32x4*)(dzt + st32_off<C, W>(px / W, px % W) + 4 * c4) = z;
      }
      const float* wl = w + (long)l * w_stride;
      float A[9][OQ][4];
#pragma unroll
      for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int q = 0; q < OQ; ++q)
#pragma unroll
          for (int s4 = 0; s4 < 4; ++s4) A[t][q][s4] = wl[((long)t * C + 16 * q + 4 * g + s4) * C + 16 * ot + lx];
      st_barrier();  // dz complete
      auto epi = [&](int p, const f32x4& acc) {
        const int r = p / W, px = p % W;
        const int cz = st32_off<C, W>(r, px) + 16 * ot + 4 * g, cy = p * PS + 16 * ot + 4 * g;
        const f32x4 z4 = *(const f32x4*)(dzt + cz), d4 = *(const f32x4*)(dyt + cy);
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = d4[e] - acc[e] + two_gamma * z4[e];
        *(f32x4*)(dyt + cy) = v;  // (own pixel, own channels)
      };
#pragma unroll 1
      for (int j = 0; j < G::T / G::WPT; j += 2) {
        const int p0 = 16 * (rw + j * G::WPT) + lx, p1 = 16 * (rw + (j + 1) * G::WPT) + lx;
        const int r0 = p0 / W, x0p = p0 % W, r1 = p1 / W, x1p = p1 % W;
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
          for (int q = 0; q < OQ; ++q) {
            const f32x4 b0 = *(const f32x4*)(dzt + ((r0 + t / 3) * TW + x0p + t % 3) * PS + 16 * q + 4 * g);
            const f32x4 b1 = *(const f32x4*)(dzt + ((r1 + t / 3) * TW + x1p + t % 3) * PS + 16 * q + 4 * g);
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
              acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(A[t][q][s4], b0[s4], acc0, 0, 0, 0);
              acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(A[t][q][s4], b1[s4], acc1, 0, 0, 0);
            }
          }
        mfma_f32_settle();
        epi(p0, acc0);
        epi(p1, acc1);
      }
    }
    st_barrier();  // dx_0 complete
    for (int i = tid; i < G::NCH; i += G::NTH)
      *(f32x4*)(dx0 + ib + 4L * i) = *(const f32x4*)(dyt + (i / (C / 4)) * PS + 4 * (i % (C / 4)));
    st_barrier();  // (dyt reused by the next image)
  }
}

// The image-resident stages behind one interface: dtype picks k_stagef / k_stageb / k_wgradb (ASR_BF16) or
// k_stagef32 / k_stageb32 / k_wgrad32 (ASR_F32), and every activation / W pointer is of that type.
static constexpr bool stage_bf16_c_w(int C, int W) {
  return (W == 16 && C == 32) || (W == 8 && C == 64) || (W == 8 && C == 32);
}
static constexpr bool stage_f32_c_w(int C, int W) { return (W == 16 && C == 32) || (W == 8 && C == 64); }
bool stage_img_supported(int H, int W, int C, int dtype) {
  if (H != W) return false;
  if (dtype == ASR_BF16) return stage_bf16_c_w(C, W);
  return dtype == ASR_F32 && stage_f32_c_w(C, W);
}
static const char* stage_img_name(int dtype) {
  return dtype == ASR_BF16 ? "image-resident stage" : "fp32 image-resident stage";
}

// the image-resident stage forward: x0 [N][H][W][C] -> ys (L layers at y_stride), masks (L at mask_stride)
int stage_img_forward(int dtype, const void* x0, void* ys, long y_stride, uint8_t* masks, long mask_stride,
                      const void* w, long w_stride, const float* bias, long bias_stride, float h, int N, int H, int W,
                      int C, int L, hipStream_t s) {
  if (!stage_img_supported(H, W, C, dtype))
    return fail(ASR_E_UNSUPPORTED, "%s: H=%d W=%d C=%d", stage_img_name(dtype), H, W, C);
  if (dtype == ASR_BF16)
    return dispatch_c_w<stage_bf16_c_w>(stage_img_name(dtype), C, W, [&](auto c, auto sw) -> int {
      using G = StImg<decltype(c)::value, decltype(sw)::value>;
      const unsigned grid = (unsigned)std::max(1, (N + kStIpw - 1) / kStIpw);
      const size_t lds = (size_t)kStIpw * 2 * G::IMGE * 2;
      hipLaunchKernelGGL((k_stagef<decltype(c)::value, G::W>), dim3(grid), dim3(G::NTH), lds, s, (const bf16*)x0,
                         (bf16*)ys, y_stride, masks, mask_stride, (const bf16*)w, w_stride, bias, bias_stride, h, N,
                         L);
      ASR_LAUNCH_CHECK("k_stagef");
      return ASR_OK;
    });
  return dispatch_c_w<stage_f32_c_w>(stage_img_name(dtype), C, W, [&](auto c, auto sw) -> int {
    using G = StImg32<decltype(c)::value, decltype(sw)::value>;
    const size_t lds = (size_t)2 * G::IMGF * 4;
    hipLaunchKernelGGL((k_stagef32<decltype(c)::value, G::W>), dim3((unsigned)std::max(1, N)), dim3(G::NTH), lds, s,
                       (const float*)x0, (float*)ys, y_stride, masks, mask_stride, (const float*)w, w_stride, bias,
                       bias_stride, h, N, L);
    ASR_LAUNCH_CHECK("k_stagef32");
    return ASR_OK;
  });
}

// its backward (input gradient): dyL -> dx0; dys: the gradient entering each layer 0 .. L-1 (d_stride apart)
int stage_img_backward(int dtype, const void* dyL, void* dys, long d_stride, void* dx0, const uint8_t* masks,
                       long mask_stride, const void* w, long w_stride, float h, float two_gamma, int N, int H, int W,
                       int C, int L, hipStream_t s) {
  if (!stage_img_supported(H, W, C, dtype))
    return fail(ASR_E_UNSUPPORTED, "%s: H=%d W=%d C=%d", stage_img_name(dtype), H, W, C);
  if (dtype == ASR_BF16)
    return dispatch_c_w<stage_bf16_c_w>(stage_img_name(dtype), C, W, [&](auto c, auto sw) -> int {
      using G = StImg<decltype(c)::value, decltype(sw)::value>;
      const unsigned grid = (unsigned)std::max(1, (N + kStIpw - 1) / kStIpw);
      const size_t lds = (size_t)kStIpw * (G::IMGE + G::H * G::W * G::PS) * 2;
      hipLaunchKernelGGL((k_stageb<decltype(c)::value, G::W>), dim3(grid), dim3(G::NTH), lds, s, (const bf16*)dyL,
                         (bf16*)dys, d_stride, (bf16*)dx0, masks, mask_stride, (const bf16*)w, w_stride, h, two_gamma,
                         N, L);
      ASR_LAUNCH_CHECK("k_stageb");
      return ASR_OK;
    });
  return dispatch_c_w<stage_f32_c_w>(stage_img_name(dtype), C, W, [&](auto c, auto sw) -> int {
    using G = StImg32<decltype(c)::value, decltype(sw)::value>;
    const size_t lds = (size_t)(G::IMGF + G::H * G::W * G::PS) * 4;
    hipLaunchKernelGGL((k_stageb32<decltype(c)::value, G::W>), dim3((unsigned)std::max(1, N)), dim3(G::NTH), lds, s,
                       (const float*)dyL, (float*)dys, d_stride, (float*)dx0, masks, mask_stride, (const float*)w,
                       w_stride, h, two_gamma, N, L);
    ASR_LAUNCH_CHECK("k_stageb32");
    return ASR_OK;
  });
}

// the weight-gradient slabs of L layers in one launch (k_wgradb / k_wgrad32, blockIdx.y = layer): layer l reads
// x0 + l x_stride, dys + l d_stride, masks + l mask_stride and writes slabs + l slab_stride
int wgrad_layers(int dtype, const void* x0, long x_stride, const void* dys, long d_stride, const uint8_t* masks,
                 long mask_stride, float h, int N, int H, int W, int C, int L, float* slabs, long slab_stride,
                 int* nslabs, hipStream_t s) {
  if (dtype == ASR_BF16)
    return wgradb_layers((const bf16*)x0, x_stride, (const bf16*)dys, d_stride, masks, mask_stride, h, N, H, W, C, L,
                         slabs, slab_stride, nslabs, s);
  return wgrad32_layers((const float*)x0, x_stride, (const float*)dys, d_stride, masks, mask_stride, h, N, H, W, C, L,
                        slabs, slab_stride, nslabs, s);
}

}  // namespace asr
