// bf16 path of Conv2DAntisymmetric(kernel_size = K) for K in {5, 7}
// (layers/tfkeras_layer_Conv2DAntisymmetric.py:60-68, 109-145, 163-170): the
// K x K SAME conv / Euler block and its backward on v_mfma_f32_16x16x32_bf16,
// bf16 activations and W, fp32 accumulation, for C in {16, 32, 64} and
// W in {8, 16, 32} (any H, any N).  The fp32 path of the same layer is the VALU
// pair k_conv_f32 / k_wgrad_f32 (asr_conv_f32.hip).
//
// Forward / data gradient (k_convk): k_convb's implicit GEMM D[o][px] =
// sum_kappa W^T[o][kappa] X[kappa][px], kappa = tap * C + i, with the loops the
// other way round.  The reduction is K*K*C long (3136 at K = 7, C = 64: 98
// k-steps, a 401 KB pack), so a wave cannot hold its o-tile's A fragments as
// k_convb does (392 VGPRs).  Instead a workgroup (4 waves) owns a band of
// 256 output pixels of one image (BR = 256 / W rows: 8, 16 or 32), staged with
// its K/2 halo in LDS ((BR + K - 1) x (W + K - 1) pixels of C + 8 bf16, zeros
// outside the image); every wave keeps the accumulators of its share of the
// band's 16 pixel tiles resident (C = 64: 16 tiles x 4 VGPRs; C = 32: 8;
// C = 16: 4) and sweeps the k-steps once: each step's A fragment is one 16-B
// load per lane from the pack (asr_theta_to_w_k_bf16; fetched a group of 4
// steps ahead of its use) and feeds one MFMA per resident tile, whose B
// fragment is one 16-B LDS read (the pixel shifted by the step's tap, 8
// channels).  A partial band (H not a multiple of BR, or an image lower than
// the band) skips its empty tiles in blocks of 4.
//   L2 traffic: a sweep reads its o-tile's pack once: 1 KiB per k-step for
//   16 MFMAs per wave = 64 B per MFMA on a full band (k_convb: 0 in the loop,
//   the fragments live in registers), 16 B / clk / CU at the MFMA's 16 clk.
//   An 8 x 8 image fills 4 of a band's 16 tiles: 256 B per MFMA there.
//   Each tile's B fragment of the next step is read right after the MFMA that
//   consumed the current one (NT reads in flight per wave; sched_barrier pins
//   the order, hipcc otherwise sinks every read to its use and waits for it).
//   LDS per workgroup (tile, + the band's dy copy in B_EULER), K = 7:
//     C = 64: 76 608 B (+ 36 864)  -> LDS admits 2 workgroups per CU forward, 1 backward;
//     C = 32: 42 560 B (+ 20 480)  -> 3 / 2;   C = 16: 25 536 B (+ 12 288) -> 6 / 4
//   (the W = 32 and W = 8 tiles; W = 16 is smaller.  K = 5: 62 208 / 34 560 /
//   20 736 B at W = 32).  The size is dynamic LDS, raised past 64 KB per launch
//   (160 KB per CU on gfx950).  The registers bind first: the resident tiles,
//   their B fragments and the A groups take 380-480 VGPRs at C = 64 (one wave
//   per SIMD: 1 workgroup per CU), 210-290 at C = 32 (1-2), 180-210 at C = 16
//   (2); the launch asks the runtime for the resident count and sizes the
//   persistent grid by it (at most 4 per CU).
//   F_EULER: y = x + h relu(conv(x) + b), relu-mask bits (asr.h layout);
//   F_CONV:  y = conv(x) + b;
//   B_EULER: the tile holds dz = dy & mask (exact), dx = dy - h conv(dz) + 2 gamma h dz;
//   B_CONV:  dx = -conv(dz) + 2 gamma dz, dz = dy.
//
// Weight gradient (k_wgradk): k_wgradb's pixel-reduction GEMM D[t][i][o] =
// h sum_px x[px + tap t][i] dz[px][o] (dz = dy & mask exact in bf16, h on the
// fp32 sums; db = h sum_px dz on MFMA, ones x dz).  K*K taps x (C/16)^2 tiles
// of accumulators (784 tiles at K = 7, C = 64) do not fit one workgroup, so
// blockIdx.y is the tap row ky: a workgroup stages the band's BR = 128 / W
// rows of x shifted by ky - K/2 (with the column halo) and of dz, pixel-major
// with C + 8 channels per pixel, and reads both operands with
// ds_read_b64_tr_b16 (k_wgradb's k order); wave (i-tile, NO o-tiles) holds the
// row's K taps x NO tiles (56 VGPRs at K = 7).  At C < 64 four waves split the
// band's 32-pixel chunks and each writes a slab of its own (no LDS reduction);
// the K workgroups of one blockIdx.x fill disjoint tap rows of the same slabs
// ([dW | db] of K*K*C*C + C floats; db from ky = 0).  The slab count is bounded
// by 48 MB of slabs (59 at K = 7, C = 64) and by 256.
#include <algorithm>

#include "asr_common.h"
#include "asr_internal.h"

namespace asr {

namespace {

template <int C, int W_, int K>
struct KxkBand {
  static constexpr int OT = C / 16, W = W_, PAD = K / 2, TW = W + K - 1, BR = 256 / W, TR = BR + K - 1, PS = C + 8;
  static constexpr int TILEE = TR * TW * PS;      // elements of the haloed band tile
  static constexpr int DYE = BR * W * PS;         // the band's own rows of dy (B_EULER)
  static constexpr int T = 16;                    // 16-pixel tiles per band
  static constexpr int WPT = 4 / OT, NT = T / WPT;  // waves sharing an o-tile, tiles per wave
  static constexpr int JB = NT < 4 ? NT : 4;      // tiles skipped together in a partial band
  static constexpr int KS = (K * K * C + 31) / 32;
  static constexpr int U = 4;                     // k-steps per A fetch group
  static_assert(W == 8 || W == 16 || W == 32, "bf16 k x k band: W in {8, 16, 32}");
  static_assert(K == 5 || K == 7, "bf16 k x k band: K in {5, 7}");
  static constexpr size_t lds(int mode) { return (size_t)(TILEE + (mode == B_EULER ? DYE : 0)) * sizeof(bf16); }
};

// 8 bf16 masked by 8 relu bits (bit j -> halfword j)
__device__ __forceinline__ uint4 kxk_mask8(uint4 v, unsigned bits) {
  auto h2 = [&](unsigned b) { return ((b & 1u) ? 0xffffu : 0u) | ((b & 2u) ? 0xffff0000u : 0u); };
  v.x &= h2(bits);
  v.y &= h2(bits >> 2);
  v.z &= h2(bits >> 4);
  v.w &= h2(bits >> 6);
  return v;
}

template <int C, int W, int K, int MODE>
__global__ __launch_bounds__(256) void k_convk(const bf16* __restrict__ xin, bf16* __restrict__ out,
                                               uint8_t* __restrict__ mask, const bf16* __restrict__ wpack,
                                               const float* __restrict__ bias, float h, float two_gamma, int N, int H,
                                               const uint8_t* __restrict__ dmask) {
  using G = KxkBand<C, W, K>;
  constexpr int OT = G::OT, TW = G::TW, BR = G::BR, KS = G::KS, C8 = C / 8, PAD = G::PAD, NT = G::NT, U = G::U;
  // 16-B chunks of the tile (at most 17 per thread: K = 7, C = 64); up to 9 of a thread's loads in flight
  // before their stores (all 17 spilled at C = 64, W = 8)
  constexpr int NCH = G::TR * TW * C8, NPT = (NCH + 255) / 256, SB = NPT < 9 ? NPT : 9;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_kxk[];
  bf16* tile = (bf16*)lds_kxk;
  bf16* dyc = tile + G::TILEE;  // B_EULER: the band's own rows of dy unmasked (the epilogue's dy term)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, lx = lane & 15;
  const int ot = wave % OT, rw = wave / OT;
  const int nb = (H + BR - 1) / BR;
  const long items = (long)N * nb;
  const long i0 = (long)blockIdx.x * items / gridDim.x, i1 = (long)(blockIdx.x + 1) * items / gridDim.x;
  const bf16* wp = wpack + ((long)ot * KS * 64 + lane) * 8;  // k-step ks of this o-tile: wp + 512 ks
  f32x4 bz = {0.f, 0.f, 0.f, 0.f};
  if ((MODE == F_EULER || MODE == F_CONV) && bias) bz = *(const f32x4*)(bias + 16 * ot + 4 * g);
  // lane lx's pixel of the wave's tile j: band pixel 16 (rw + j WPT) + lx (W = 8: a tile spans two rows)
  int pb[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int bp = 16 * (rw + j * G::WPT) + lx;
    pb[j] = ((bp / W) * TW + bp % W) * G::PS;
  }
  for (long item = i0; item < i1; ++item) {
    const int n = (int)(item / nb), y0 = (int)(item % nb) * BR;
    const int rows = min(BR, H - y0), tact = (rows * W + 15) / 16;  // the band's tiles with a row inside the image
    __syncthreads();  // the previous band's tile consumed
#pragma unroll 1
    for (int b0 = 0; b0 < NCH; b0 += 256 * SB) {
      uint4 v[SB];
      unsigned pm[SB];
#pragma unroll
      for (int k = 0; k < SB; ++k) {
        const int i = b0 + tid + 256 * k;
        const int r = i / (TW * C8), rem = i % (TW * C8), col = rem / C8, c8 = rem % C8;
        const int gy = y0 - PAD + r, gx = col - PAD;
        v[k] = make_uint4(0u, 0u, 0u, 0u);
        pm[k] = 0u;
        if (i < NCH && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W) {
          const long e = (((long)n * H + gy) * W + gx) * C + 8 * c8;
          v[k] = *(const uint4*)(xin + e);
          if (MODE == B_EULER) pm[k] = dmask[e >> 3];
        }
      }
#pragma unroll
      for (int k = 0; k < SB; ++k) {
        const int i = b0 + tid + 256 * k;
        if (i < NCH) {
          const int r = i / (TW * C8), rem = i % (TW * C8), col = rem / C8, c8 = rem % C8;
          bf16* dst = tile + (r * TW + col) * G::PS + 8 * c8;
          if constexpr (MODE == B_EULER) {  // the tile gets dz = dy & mask; the band's rows keep dy
            *(uint4*)dst = kxk_mask8(v[k], pm[k]);
            if (r >= PAD && r < PAD + BR && col >= PAD && col < PAD + W)
              *(uint4*)(dyc + ((r - PAD) * W + col - PAD) * G::PS + 8 * c8) = v[k];
          } else {
            *(uint4*)dst = v[k];
          }
        }
      }
    }
    __syncthreads();
    f32x4 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = bz;
    // one sweep over the k-steps, the accumulators resident; A a group of U steps ahead
    bf16x8 Ac[U], An[U];
#pragma unroll
    for (int u = 0; u < U; ++u) Ac[u] = *(const bf16x8*)(wp + 512L * min(u, KS - 1));
    // the lane's tile offset of k-step ks: its tap's pixel shift and channel run
    auto step_off = [&](int ks) {
      const int kap = 32 * ks + 8 * g;
      // (the last k-step's taps past K*K pad A with zeros: read any tap's pixels)
      const int t = min(kap / C, K * K - 1), i0c = kap % C;
      return ((t / K) * TW + t % K) * G::PS + i0c;
    };
    constexpr int KSM = KS / U * U;  // k-steps in whole groups; the KS % U others follow the loop
    if (tact == G::T) {
      // full band: every tile active, no branch in the loop; the B fragments of step ks + 1 are
      // read while step ks's MFMAs run (one wave per SIMD at C = 64: nothing else hides the LDS latency)
      // (tile j's fragment of the next step replaces the one its MFMA just consumed: NT reads in flight)
      uint4 B[NT];
      {
        const int so = step_off(0);
#pragma unroll
        for (int j = 0; j < NT; ++j) B[j] = *(const uint4*)(tile + pb[j] + so);
      }
      auto step = [&](const bf16x8& A, int ks) {
        const bf16* tn = tile + step_off(min(ks + 1, KS - 1));
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A, __builtin_bit_cast(bf16x8, B[j]), acc[j], 0, 0, 0);
          B[j] = *(const uint4*)(tn + pb[j]);
          // (keeps this order: left alone, hipcc sinks every read to just before its MFMA and waits for it)
          __builtin_amdgcn_sched_barrier(0);
        }
      };
#pragma unroll 1
      for (int k0 = 0; k0 < KSM; k0 += U) {
#pragma unroll
        for (int u = 0; u < U; ++u) An[u] = *(const bf16x8*)(wp + 512L * min(k0 + U + u, KS - 1));
#pragma unroll
        for (int u = 0; u < U; ++u) step(Ac[u], k0 + u);
#pragma unroll
        for (int u = 0; u < U; ++u) Ac[u] = An[u];
      }
#pragma unroll
      for (int u = 0; u < KS - KSM; ++u) step(Ac[u], KSM + u);
    } else {
      // partial band: the empty tiles skipped in blocks of JB
      auto step = [&](const bf16x8& A, int ks) {
        const int so = step_off(ks);
#pragma unroll
        for (int jb = 0; jb < NT; jb += G::JB) {
          if (rw + jb * G::WPT < tact) {  // (wave-uniform)
#pragma unroll
            for (int j = jb; j < jb + G::JB; ++j) {
              const uint4 bv = *(const uint4*)(tile + pb[j] + so);
              acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A, __builtin_bit_cast(bf16x8, bv), acc[j], 0, 0, 0);
            }
          }
        }
      };
#pragma unroll 1
      for (int k0 = 0; k0 < KSM; k0 += U) {
#pragma unroll
        for (int u = 0; u < U; ++u) An[u] = *(const bf16x8*)(wp + 512L * min(k0 + U + u, KS - 1));
#pragma unroll
        for (int u = 0; u < U; ++u) step(Ac[u], k0 + u);
#pragma unroll
        for (int u = 0; u < U; ++u) Ac[u] = An[u];
      }
#pragma unroll
      for (int u = 0; u < KS - KSM; ++u) step(Ac[u], KSM + u);
    }
    mfma_bf16_settle();  // (the epilogue branches: every path must see the result's wait states)
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int tau = rw + j * G::WPT;
      if (tau >= tact) break;  // (wave-uniform; rows only grow with tau)
      const int bp = 16 * tau + lx, r = bp / W, px = bp % W;
      const bool ok = y0 + r < H;
      const long pix = ((long)n * H + y0 + r) * W + px;
      const long oi = pix * C + 16 * ot + 4 * g;  // this lane's 4 channels
      const uint2 cw = *(const uint2*)(tile + ((r + PAD) * TW + px + PAD) * G::PS + 16 * ot + 4 * g);  // x or dz at the pixel
      const float ctr[4] = {__uint_as_float(cw.x << 16), __uint_as_float(cw.x & 0xffff0000u),
                            __uint_as_float(cw.y << 16), __uint_as_float(cw.y & 0xffff0000u)};
      float v[4];
      if constexpr (MODE == F_EULER) {
        unsigned nib = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float z = acc[j][e];
          nib |= (z > 0.f ? 1u : 0u) << e;
          v[e] = fmaf(h, fmaxf(z, 0.f), ctr[e]);
        }
        if (mask) {  // the pixel's 16 channels of this o-tile: 4 nibbles, one 16-bit store
          unsigned m = nib << (4 * g);
          m |= (unsigned)__shfl_xor((int)m, 16, 64);
          m |= (unsigned)__shfl_xor((int)m, 32, 64);
          if (g == 0 && ok) *(uint16_t*)(mask + (pix * C + 16 * ot) / 8) = (uint16_t)m;
        }
      } else if constexpr (MODE == F_CONV) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc[j][e];
      } else if constexpr (MODE == B_CONV) {  // dz = dy (the tile): dx = -A dz + 2 gamma dz
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaf(two_gamma, ctr[e], -acc[j][e]);
      } else {  // B_EULER: the tile holds dz = dy & mask
        const uint2 dw = *(const uint2*)(dyc + (r * W + px) * G::PS + 16 * ot + 4 * g);
        const float d0[4] = {__uint_as_float(dw.x << 16), __uint_as_float(dw.x & 0xffff0000u),
                             __uint_as_float(dw.y << 16), __uint_as_float(dw.y & 0xffff0000u)};
        const float hg = h * two_gamma;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaf(hg, ctr[e], fmaf(-h, acc[j][e], d0[e]));
      }
      if (ok) *(uint2*)(out + oi) = make_uint2(pk_bf16_rn(v[0], v[1]), pk_bf16_rn(v[2], v[3]));
    }
  }
}

template <int C, int W, int K, int MODE>
int launch_convk(const bf16* xin, bf16* out, uint8_t* mask, const bf16* w, const float* bias, float h, float two_gamma,
                 int N, int H, const uint8_t* dmask, hipStream_t s) {
  using G = KxkBand<C, W, K>;
  constexpr size_t lds = G::lds(MODE);
  static_assert(lds <= 160 * 1024, "bf16 k x k band: LDS per workgroup");
  const long items = (long)N * ((H + G::BR - 1) / G::BR);
  // once per instantiation and device (a device beyond the table: every call): the dynamic-LDS limit, raised
  // where the band needs more than the default, and the persistent workgroups per CU: what registers and
  // LDS keep resident (1 if the runtime cannot say)
  static int resident[64];
  int dev = 0, uncached = 0;
  ASR_TRY(hip_check(hipGetDevice(&dev), "hipGetDevice"));
  int* res = dev >= 0 && dev < 64 ? &resident[dev] : &uncached;
  if (*res == 0) {
    if (lds > 64 * 1024)  // above the default dynamic-LDS limit
      ASR_TRY(hip_check(hipFuncSetAttribute((const void*)k_convk<C, W, K, MODE>,
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds),
                        "hipFuncSetAttribute"));
    int nblk = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nblk, k_convk<C, W, K, MODE>, 256, lds);
    *res = (e == hipSuccess && nblk > 0) ? nblk : 1;
    if (e != hipSuccess) (void)hipGetLastError();
  }
  const int per_cu = std::min(4, *res);
  const long grid = std::max<long>(1, std::min<long>(items, (long)per_cu * launch_cus()));
  hipLaunchKernelGGL((k_convk<C, W, K, MODE>), dim3((unsigned)grid), dim3(256), lds, s, xin, out, mask, w, bias, h,
                     two_gamma, N, H, dmask);
  ASR_LAUNCH_CHECK("k_convk");
  return ASR_OK;
}

template <int C, int W, int K>
int convk_modes(int fmode, const bf16* xin, bf16* out, uint8_t* mask, const bf16* w, const float* bias, float h,
                float two_gamma, int N, int H, const uint8_t* dmask, hipStream_t s) {
  switch (fmode) {
    case F_EULER: return launch_convk<C, W, K, F_EULER>(xin, out, mask, w, bias, h, 0.f, N, H, nullptr, s);
    case F_CONV: return launch_convk<C, W, K, F_CONV>(xin, out, nullptr, w, bias, 1.f, 0.f, N, H, nullptr, s);
    case B_EULER: return launch_convk<C, W, K, B_EULER>(xin, out, nullptr, w, nullptr, h, two_gamma, N, H, dmask, s);
    case B_CONV: return launch_convk<C, W, K, B_CONV>(xin, out, nullptr, w, nullptr, 1.f, two_gamma, N, H, nullptr, s);
  }
  return fail(ASR_E_ARG, "conv bf16 k x k: bad mode %d", fmode);
}

// ---------------------------------------------------------------------------
// weight gradient
// ---------------------------------------------------------------------------
template <int C, int W_, int K>
struct KxkWg {
  static constexpr int OT = C / 16, W = W_, TW = W + K - 1, BR = 128 / W, PS = C + 8, C8 = C / 8;
  static constexpr int NO = C == 16 ? 1 : 2, TS = OT * (OT / NO);  // waves of one (i-tile, NO o-tiles) set
  static constexpr int SPL = C == 64 ? 1 : 4;                      // waves splitting the band's chunks: a slab each
  static constexpr int NW = TS * SPL, NTH = 64 * NW;
  static constexpr int XCH = BR * TW * C8, DCH = BR * W * C8;
  static constexpr int XE = BR * TW * PS, DE = BR * W * PS;
  static constexpr int XPT = (XCH + NTH - 1) / NTH, DPT = (DCH + NTH - 1) / NTH;  // 16-B chunks per thread
  static constexpr long E = (long)K * K * C * C, ES = E + C;
};

// slab rows of one weight gradient: at most 48 MB of slabs and 256 rows
template <int C, int W, int K>
int wgradk_grid(int N, int H) {
  using G = KxkWg<C, W, K>;
  const long items = (long)N * ((H + G::BR - 1) / G::BR);
  const long cap = std::min<long>(256, (48L << 20) / (G::ES * 4)) / G::SPL;
  return (int)std::max<long>(1, std::min<long>(items, cap));
}

// one transposed-read k run: 4 pixels' 4 channels -> the lane's 4 bf16 of one channel
__device__ __forceinline__ s16x4 kxk_tr4(const bf16* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((ASR_LDS s16x4*)p);
}

// MASKED false: dz = dy (the bare conv's weight gradient; dmask unused)
template <int C, int W, int K, bool MASKED>
__global__ __launch_bounds__((KxkWg<C, W, K>::NTH)) void k_wgradk(const bf16* __restrict__ x,
                                                                  const bf16* __restrict__ dy,
                                                                  const uint8_t* __restrict__ dmask, int N, int H,
                                                                  float h, float* __restrict__ slabs) {
  using G = KxkWg<C, W, K>;
  constexpr int TW = G::TW, BR = G::BR, NO = G::NO, OT = G::OT, PS = G::PS, C8 = G::C8;
  __shared__ __attribute__((aligned(16))) bf16 xt[G::XE];   // [BR][TW][PS]: x rows shifted by the tap row
  __shared__ __attribute__((aligned(16))) bf16 dzt[G::DE];  // [BR][W][PS]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, lx = lane & 15;
  const int q = lx >> 2, pq = lx & 3;
  const int ts = wave % G::TS, sp = wave / G::TS;
  const int it = ts / (OT / NO), ob = (ts % (OT / NO)) * NO;
  const int ky = blockIdx.y;
  const int nb = (H + BR - 1) / BR;
  const long items = (long)N * nb;
  const long i0 = (long)blockIdx.x * items / gridDim.x, i1 = (long)(blockIdx.x + 1) * items / gridDim.x;
  f32x4 acc[K][NO], accb[NO];
#pragma unroll
  for (int t = 0; t < K; ++t)
#pragma unroll
    for (int o = 0; o < NO; ++o) acc[t][o] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int o = 0; o < NO; ++o) accb[o] = f32x4{0.f, 0.f, 0.f, 0.f};
  // the lane's 8-B piece of channels 16 ch + 4 pq .. +3 at pixel P of a tile
  auto piece = [&](const bf16* tile, int P, int ch) { return tile + P * PS + 16 * ch + 4 * pq; };
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  auto frag = [&](const bf16* tile, int P1, int P2, int ch) {
    const s16x4 a = kxk_tr4(piece(tile, P1, ch)), b = kxk_tr4(piece(tile, P2, ch));
    const s16x8 c = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    return __builtin_bit_cast(bf16x8, c);
  };
  bf16x8 ones;
#pragma unroll
  for (int j = 0; j < 8; ++j) ones[j] = (bf16)1.f;
  // persistent over bands: the next band's global loads are in flight during this band's MFMAs
  // (dz = dy & mask formed at the LDS store, so nothing waits for them before)
  uint4 px[G::XPT], pd[G::DPT];
  unsigned pm[G::DPT];
  auto fetch = [&](long item) {
    const int n = (int)(item / nb), y0 = (int)(item % nb) * BR;
#pragma unroll
    for (int k = 0; k < G::XPT; ++k) {
      const int i = tid + k * G::NTH;
      const int r = i / (TW * C8), rem = i % (TW * C8), col = rem / C8, c8 = rem % C8;
      const int gy = y0 + r + ky - K / 2, gx = col - K / 2;
      px[k] = make_uint4(0u, 0u, 0u, 0u);
      if (i < G::XCH && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W)
        px[k] = *(const uint4*)(x + (((long)n * H + gy) * W + gx) * C + 8 * c8);
    }
#pragma unroll
    for (int k = 0; k < G::DPT; ++k) {
      const int i = tid + k * G::NTH;
      const int r = i / (W * C8);
      pd[k] = make_uint4(0u, 0u, 0u, 0u);
      pm[k] = 0u;
      if (i < G::DCH && y0 + r < H) {
        const long e = ((long)n * H + y0) * W * C + 8L * i;
        pd[k] = *(const uint4*)(dy + e);
        if constexpr (MASKED) pm[k] = dmask[e >> 3];
      }
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int k = 0; k < G::XPT; ++k) {
      const int i = tid + k * G::NTH;
      const int P = i / C8, c8 = i % C8;  // (P = r * TW + col)
      if (i < G::XCH) *(uint4*)(xt + P * PS + 8 * c8) = px[k];
    }
#pragma unroll
    for (int k = 0; k < G::DPT; ++k) {
      const int i = tid + k * G::NTH;
      const int P = i / C8, c8 = i % C8;
      if (i < G::DCH) *(uint4*)(dzt + P * PS + 8 * c8) = MASKED ? kxk_mask8(pd[k], pm[k]) : pd[k];
    }
  };
  if (i0 < i1) fetch(i0);
  for (long item = i0; item < i1; ++item) {
    const int y0 = (int)(item % nb) * BR;
    __syncthreads();  // the previous band's operands consumed
    store();
    __syncthreads();
    if (item + 1 < i1) fetch(item + 1);
    const int rows = min(BR, H - y0), nch = (rows * W + 31) / 32;
    for (int ch = sp; ch < nch; ch += G::SPL) {  // (wave-uniform: EXEC stays full for the transposed reads)
      const int k1 = 32 * ch + 4 * g + q, k2 = k1 + 16;
      const int r1 = k1 / W, c1 = k1 % W, r2 = k2 / W, c2 = k2 % W;
      bf16x8 B[NO];
#pragma unroll
      for (int o = 0; o < NO; ++o) B[o] = frag(dzt, r1 * W + c1, r2 * W + c2, ob + o);
#pragma unroll
      for (int t = 0; t < K; ++t) {
        const bf16x8 A = frag(xt, r1 * TW + c1 + t, r2 * TW + c2 + t, it);
#pragma unroll
        for (int o = 0; o < NO; ++o) acc[t][o] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A, B[o], acc[t][o], 0, 0, 0);
      }
      if (it == 0 && ky == 0) {
#pragma unroll
        for (int o = 0; o < NO; ++o) accb[o] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, B[o], accb[o], 0, 0, 0);
      }
    }
  }
  mfma_bf16_settle();
  float* slab = slabs + ((long)blockIdx.x * G::SPL + sp) * G::ES;
#pragma unroll
  for (int t = 0; t < K; ++t)
#pragma unroll
    for (int o = 0; o < NO; ++o)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        slab[((long)(ky * K + t) * C + 16 * it + 4 * g + e) * C + 16 * (ob + o) + lx] = h * acc[t][o][e];
  if (it == 0 && ky == 0 && g == 0) {
#pragma unroll
    for (int o = 0; o < NO; ++o) slab[G::E + 16 * (ob + o) + lx] = h * accb[o][0];
  }
}

template <int C, int W, int K>
int launch_wgradk(const bf16* x, const bf16* dy, const uint8_t* mask, int N, int H, float h, float* slabs,
                  int* nslabs, hipStream_t s) {
  using G = KxkWg<C, W, K>;
  const int gx = wgradk_grid<C, W, K>(N, H);
  if (mask)
    hipLaunchKernelGGL((k_wgradk<C, W, K, true>), dim3(gx, K), dim3(G::NTH), 0, s, x, dy, mask, N, H, h, slabs);
  else
    hipLaunchKernelGGL((k_wgradk<C, W, K, false>), dim3(gx, K), dim3(G::NTH), 0, s, x, dy, mask, N, H, h, slabs);
  ASR_LAUNCH_CHECK("k_wgradk");
  *nslabs = gx * G::SPL;
  return ASR_OK;
}

template <int C, int W, int K>
int wgradk_rows(int N, int H) {
  return wgradk_grid<C, W, K>(N, H) * KxkWg<C, W, K>::SPL;
}

}  // namespace

// every (K, C, W) of the supported set
#define ASR_KXK_CASES(K_)                                                                                      \
  ASR_KXK(K_, 16, 8) ASR_KXK(K_, 16, 16) ASR_KXK(K_, 16, 32) ASR_KXK(K_, 32, 8) ASR_KXK(K_, 32, 16)            \
  ASR_KXK(K_, 32, 32) ASR_KXK(K_, 64, 8) ASR_KXK(K_, 64, 16) ASR_KXK(K_, 64, 32)

bool convk_bf16_supported(int K, int W, int C) {
  return (K == 5 || K == 7) && (W == 32 || W == 16 || W == 8) && (C == 16 || C == 32 || C == 64);
}

// fmode F_EULER / F_CONV: xin = x; B_EULER / B_CONV: xin = dy (dmask: the relu bits of B_EULER).
// w: asr_theta_to_w_k_bf16's pack of one layer.
int convk_bf16(int fmode, int K, const void* xin, void* out, uint8_t* mask, const void* w, const float* bias, float h,
               float two_gamma, const uint8_t* dmask, int N, int H, int W, int C, hipStream_t s) {
#define ASR_KXK(K_, C_, W_)                                                                                     \
  if (K == K_ && C == C_ && W == W_)                                                                            \
    return convk_modes<C_, W_, K_>(fmode, (const bf16*)xin, (bf16*)out, mask, (const bf16*)w, bias, h, two_gamma, N, \
                                   H, dmask, s);
  ASR_KXK_CASES(5)
  ASR_KXK_CASES(7)
#undef ASR_KXK
  return fail(ASR_E_UNSUPPORTED, "conv bf16 k x k: K=%d C=%d W=%d", K, C, W);
}

// slab rows wgradk_bf16 writes (each K*K*C*C + C floats); 0 outside the supported set
int wgradk_bf16_slab_rows(int K, int N, int H, int W, int C) {
#define ASR_KXK(K_, C_, W_) \
  if (K == K_ && C == C_ && W == W_) return wgradk_rows<C_, W_, K_>(N, H);
  ASR_KXK_CASES(5)
  ASR_KXK_CASES(7)
#undef ASR_KXK
  return 0;
}

// slabs of h sum patch_K(x) (x) dz, dz = dy & mask (mask nullptr: dz = dy)
int wgradk_bf16(int K, const void* x, const void* dy, const uint8_t* mask, float h, int N, int H, int W, int C,
                float* slabs, int* nslabs, hipStream_t s) {
  *nslabs = 0;
#define ASR_KXK(K_, C_, W_)          \
  if (K == K_ && C == C_ && W == W_) \
    return launch_wgradk<C_, W_, K_>((const bf16*)x, (const bf16*)dy, mask, N, H, h, slabs, nslabs, s);
  ASR_KXK_CASES(5)
  ASR_KXK_CASES(7)
#undef ASR_KXK
  return fail(ASR_E_UNSUPPORTED, "conv bf16 k x k weight gradient: K=%d C=%d W=%d", K, C, W);
}

}  // namespace asr
