// bf16 path of the 3x3 conv / Euler block at any stage width on
// v_mfma_f32_16x16x32_bf16: k_convb / k_wgradb at C in {16, 32, 64}, k_convbw /
// k_wgradbw at C in {128, 256}, behind convb_forward / convb_backward, and
// k_wgradb over a stage's layers (wgradb_layers) for the image-resident
// stages of asr_stage_img.hip.
#include "asr_common.h"
#include "asr_conv3x3.h"
#include "asr_internal.h"

namespace asr {

// ===========================================================================
// bf16 block kernels at any stage width (W in {32, 16, 8}; column strips at W >= 48, W % 16 == 0; C in {16, 32, 64}):
// the multi-stage nets' identity blocks in bf16 (the He-style ResNet-32 at the
// metric's precision, tfkeras_resnets.py:575-593).  k_conv32's geometry (asr_conv_f32.hip) on
// v_mfma_f32_16x16x32_bf16: a workgroup (4 waves) owns a band of BR = 4 output
// rows of one image, the BR + 2 input rows staged in LDS as bf16 (pixel-major,
// C channels contiguous; zero rows outside the image and zero halo columns),
// every wave keeps its o-tile's A = W^T fragments (asr_theta_to_w's bf16 pack:
// lane (lx, g) holds W^T[16 ot + lx][32 ks + 8 g .. + 7]) in registers and walks
// its share of the band's 16-pixel tiles.  B fragment of k-step ks, lane (lx, g):
// kappa = 32 ks + 8 g .. + 7 = tap t, channels i0 .. i0 + 7 of the pixel shifted
// by t: one 16-B LDS read.  The accumulator lane (lx, g) holds channels 4g..4g+3
// of pixel lx, as in the fp32 kernel (the same epilogue and mask nibbles).
//   F_EULER: y = x + h relu(conv(x) + b), relu-mask bits;
//   B_EULER: the tile holds dz = dy & mask (exact), dx = dy - h conv(dz) + 2 gamma h dz.
// The weight gradient is k_wgradb (below): bf16 MFMA on x and dz = dy & mask,
// fp32 accumulation, slabs reduced in fp32 as the bf16 stacks'.
// ===========================================================================
template <int C, int W_>
struct BfBand {
  // PS: a pixel's elements in the LDS tiles, padded so the 16 lanes of a 16-B read (16 consecutive
  // pixels) fall on distinct banks (unpadded, C = 64 put them on 2 bank groups: 8-way conflicts)
  static constexpr int OT = C / 16, W = W_, TW = W + 2, BR = 4, PS = C + 8, TILEE = (BR + 2) * TW * PS;
  static constexpr int T = BR * W / 16;  // 16-pixel tiles per band
  static constexpr int WPT = 4 / OT;     // waves sharing an o-tile
  static constexpr int KS = (9 * C + 31) / 32;
  static_assert(W == 8 || W == 16 || W == 32, "bf16 band: W in {8, 16, 32}");
};

// ---------------------------------------------------------------------------
// Column strips: k_convb / k_wgradb on images wider than the one band they
// stage, a run-time image width W >= 48, W % 16 == 0 (a 16-pixel MFMA tile
// lies in one row).  A work item is (image, band of 4 rows, strip of SW = 32
// columns); the LDS tiles are those of the W = 32 instantiations (6 rows x 34
// pixels of x, 4 x 32 of dz), the two halo columns read from the neighbouring
// strips and zero only at the image's own edges.  With W % 32 == 16 the last
// strip has 16 columns: its columns past the image are staged as zeros, the
// forward / dgrad skips their tiles (wave-uniform), the weight gradient runs
// them (x and dz both zero there: the products are exactly 0, and EXEC stays
// full for the transposed reads).  Only the global and mask-bit addresses use
// W; the mask layout is asr.h's at any width.  A band of an image SW wide is
// the same item with one strip (ns = 1, x0 = 0) and W = SW at compile time.
// ---------------------------------------------------------------------------
constexpr int kStripW = 32;
static bool strip_width(int W) { return W >= 48 && W % 16 == 0; }
static long strip_items(int N, int H, int W) { return (long)N * ((H + 3) / 4) * ((W + kStripW - 1) / kStripW); }

// item -> image n, first row y0 and first column x0 of its band (BR rows) x strip (strips of a band adjacent)
template <int BR, int SW>
__device__ __forceinline__ void strip_item(long item, int nb, int ns, int& n, int& y0, int& x0) {
  x0 = (int)(item % ns) * SW;
  const long band = item / ns;
  y0 = (int)(band % nb) * BR;
  n = (int)(band / nb);
}

// An item is a band of 4 rows of an image SW wide, or (STRIP) a band x a strip of SW = 32 columns of an image
// Wimg wide
template <int C, int SW, bool STRIP, int MODE>
__global__ __launch_bounds__(256) void k_convb(const bf16* __restrict__ xin, bf16* __restrict__ out,
                                               uint8_t* __restrict__ mask, const bf16* __restrict__ wpack,
                                               const float* __restrict__ bias, float h, float two_gamma, int N, int H,
                                               int Wimg, const uint8_t* __restrict__ dmask) {
  using G = BfBand<C, SW>;
  static_assert(!STRIP || SW == kStripW, "a band x strip item is 4 x 32 pixels");
  constexpr int OT = G::OT, TW = G::TW, BR = G::BR, KS = G::KS, C8 = C / 8;
  constexpr int NCH = (BR + 2) * TW * C8, NPT = (NCH + 255) / 256;
  __shared__ __attribute__((aligned(16))) bf16 tile[G::TILEE];
  // backward: the item's own pixels of dy unmasked (the epilogue's dy term), beside the dz tile
  __shared__ __attribute__((aligned(16))) bf16 dyc[MODE == B_EULER ? BR * SW * G::PS : 8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, lx = lane & 15;
  const int ot = wave % OT, rw = wave / OT;
  const int W = STRIP ? Wimg : SW;
  const int nb = (H + BR - 1) / BR, ns = STRIP ? (W + SW - 1) / SW : 1;
  const long items = (long)N * nb * ns;
  // persistent: a run of items per workgroup, the W fragments loaded once, the next item's pixels
  // in registers while this item's MFMAs run
  const long i0 = (long)blockIdx.x * items / gridDim.x, i1 = (long)(blockIdx.x + 1) * items / gridDim.x;
  bf16x8 A[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) A[ks] = *(const bf16x8*)(wpack + (((long)ot * KS + ks) * 64 + lane) * 8);
  f32x4 bz = {0.f, 0.f, 0.f, 0.f};
  if ((MODE == F_EULER || MODE == F_CONV) && bias) bz = *(const f32x4*)(bias + 16 * ot + 4 * g);
  uint4 pf[NPT];
  unsigned pm[NPT];
  auto fetch = [&](long item) {
    int n, y0, x0;
    strip_item<BR, SW>(item, nb, ns, n, y0, x0);
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
      const int i = tid + 256 * k;
      const int r = i / (TW * C8), rem = i % (TW * C8), col = rem / C8, c8 = rem % C8;
      const int gy = y0 - 1 + r, gx = x0 - 1 + col;  // (halo columns: the neighbouring strips' pixels)
      pf[k] = make_uint4(0u, 0u, 0u, 0u);
      pm[k] = 0u;
      if (i < NCH && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W) {
        const long e = (((long)n * H + gy) * W + gx) * C + 8 * c8;
        pf[k] = *(const uint4*)(xin + e);
        if (MODE == B_EULER) pm[k] = dmask[e >> 3];
      }
    }
  };
  if (i0 < i1) fetch(i0);
  for (long item = i0; item < i1; ++item) {
    int n, y0, x0;
    strip_item<BR, SW>(item, nb, ns, n, y0, x0);
    __syncthreads();  // the previous item's tile consumed
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
      const int i = tid + 256 * k;
      if (i >= NCH) break;
      const int r = i / (TW * C8), rem = i % (TW * C8), col = rem / C8, c8 = rem % C8;
      bf16* dst = tile + (r * TW + col) * G::PS + 8 * c8;
      if constexpr (MODE == B_EULER) {  // the tile gets dz = dy & mask; the item's own pixels keep dy
        *(uint4*)dst = mask8_bf16(pf[k], pm[k]);
        if (r >= 1 && r <= BR && col >= 1 && col <= SW) *(uint4*)(dyc + ((r - 1) * SW + col - 1) * G::PS + 8 * c8) = pf[k];
      } else {
        *(uint4*)dst = pf[k];
      }
    }
    __syncthreads();
    if (item + 1 < i1) fetch(item + 1);
    constexpr int NT = (G::T + G::WPT - 1) / G::WPT;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int tau = rw + j * G::WPT;
      if (tau >= G::T) break;  // (wave-uniform)
      const int bp = 16 * tau + lx, r = bp / SW, px = bp % SW;
      if (SW >= 16 && y0 + r >= H) break;  // (wave-uniform for SW >= 16; rows only grow with tau)
      if constexpr (STRIP)
        if (x0 + 16 * (tau % (SW / 16)) >= W) continue;  // (wave-uniform: the missing half of a 16-column last strip)
      f32x4 acc = bz;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int kap = 32 * ks + 8 * g;
        const int t = min(kap / C, 8), i0c = kap - (kap / C) * C;  // (C = 16, last k-step: tap 9 pads A with zeros)
        const uint4 bv = *(const uint4*)(tile + ((r + t / 3) * TW + px + t % 3) * G::PS + i0c);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[ks], __builtin_bit_cast(bf16x8, bv), acc, 0, 0, 0);
      }
      mfma_bf16_settle();  // (the epilogue branches: every path must see the result's wait states)
      const bool ok = STRIP || y0 + r < H;  // (per lane only at SW = 8, where a tile spans two rows)
      const long pix = ((long)n * H + y0 + r) * W + x0 + px;
      const long oi = pix * C + 16 * ot + 4 * g;  // this lane's 4 channels
      const uint2 cw = *(const uint2*)(tile + ((r + 1) * TW + px + 1) * G::PS + 16 * ot + 4 * g);  // x or dz at the pixel
      const float ctr[4] = {__uint_as_float(cw.x << 16), __uint_as_float(cw.x & 0xffff0000u),
                            __uint_as_float(cw.y << 16), __uint_as_float(cw.y & 0xffff0000u)};
      float v[4];
      if constexpr (MODE == F_EULER) {
        unsigned nib = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float z = acc[e];
          nib |= (z > 0.f ? 1u : 0u) << e;
          v[e] = fmaf(h, fmaxf(z, 0.f), ctr[e]);
        }
        if (mask) {  // the pixel's 16 channels of this o-tile: 4 nibbles, one 16-bit store
          unsigned m = nib << (4 * g);
          m |= (unsigned)__shfl_xor((int)m, 16, 64);
          m |= (unsigned)__shfl_xor((int)m, 32, 64);
          if (g == 0 && ok) *(uint16_t*)(mask + (pix * C + 16 * ot) / 8) = (uint16_t)m;
        }
      } else if constexpr (MODE == F_CONV) {  // the bare layer call: z = conv(x, W) + b
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc[e];
      } else if constexpr (MODE == B_CONV) {  // its backward: dz = dy (the tile), dx = A^T dz = -A dz + 2 gamma dz
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaf(two_gamma, ctr[e], -acc[e]);
      } else {  // B_EULER: the tile holds dz = dy & mask
        const uint2 dw = *(const uint2*)(dyc + (r * SW + px) * G::PS + 16 * ot + 4 * g);
        const float d0[4] = {__uint_as_float(dw.x << 16), __uint_as_float(dw.x & 0xffff0000u),
                             __uint_as_float(dw.y << 16), __uint_as_float(dw.y & 0xffff0000u)};
        const float hg = h * two_gamma;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaf(hg, ctr[e], fmaf(-h, acc[e], d0[e]));
      }
      if (ok) *(uint2*)(out + oi) = make_uint2(pk_bf16_rn(v[0], v[1]), pk_bf16_rn(v[2], v[3]));
    }
  }
}

// C in {128, 256}: k_convbw / k_wgradbw (below), the same items with W streamed from its pack
static bool wide_c(int C) { return C == 128 || C == 256; }
static int wgrad_wide_rows(int N, int H, int W, int C);

// W = 8, or a multiple of the 16-pixel MFMA tile: k_convb / k_wgradb over bands at W in {32, 16, 8}, over
// column strips at W >= 48
bool convb_supported(int W, int C) {
  return (W == 8 || (W >= 16 && W % 16 == 0)) && (C == 16 || C == 32 || C == 64 || wide_c(C));
}

// W: the image width (= SW unless STRIP)
template <int C, int SW, bool STRIP, int MODE>
static int launch_convb(const bf16* xin, bf16* out, uint8_t* mask, const bf16* w, const float* bias, float h,
                        float two_gamma, int N, int H, int W, const uint8_t* dmask, hipStream_t s) {
  const long items = STRIP ? strip_items(N, H, W) : (long)N * ((H + 3) / 4);
  const int cus = launch_cus();
  const long grid = std::max<long>(1, std::min<long>(items, 4L * cus));  // 4 persistent workgroups per CU (r05r)
  hipLaunchKernelGGL((k_convb<C, SW, STRIP, MODE>), dim3((unsigned)grid), dim3(256), 0, s, xin, out, mask, w, bias, h,
                     two_gamma, N, H, W, dmask);
  ASR_LAUNCH_CHECK("k_convb");
  return ASR_OK;
}

// ---------------------------------------------------------------------------
// The bf16 weight gradient at any stage width on v_mfma_f32_16x16x32_bf16
// (k_wgradb): D[t][i][o] = h sum_px x[px + tap t][i] dz[px][o], dz = dy & mask
// (exact in bf16; h applied to the fp32 sums), db[o] = h sum_px dz[px][o].
// K = pixels: a workgroup stages a band of BR = 128 / W rows of one image (x
// with its halo rows / columns, dz) in LDS, pixel-major with C channels
// contiguous, and reads both operands with ds_read_b64_tr_b16 (T10): a 16-lane
// group's lane (q, p) addresses pixel q of 4, channels 4p .. 4p+3, and lane lx
// receives channel lx of the 4 pixels -- the MFMA fragment's k run.  A 32-pixel
// chunk's k order is permuted the same way in both operands: lane group g takes
// pixels 4g .. 4g+3 (first read) and 16 + 4g .. (second), so a 32-lane half
// reads 8 consecutive pixels.  The 16-B chunk c of pixel P sits at chunk
// c ^ f(P) (f = 2 ((P >> 1) & 3) at C = 64, 2 ((P >> 2) & 1) at C = 32, 0 at
// C = 16): the half's 8 pixels x 32 B then cover all 64 banks.
// Waves: TS pair splits (i-tile it, NO o-tiles: the 9 taps' A fragments feed
// NO MFMAs each) x PS chunk splits, partials summed through LDS at the end;
// db on MFMA (ones x dz) in the it = 0 waves.  Persistent over bands, the next
// band's global loads in flight during this band's MFMAs (dz = dy & mask formed
// at the LDS store, so nothing waits for them before); one [dW | db] slab
// per workgroup, the rows the fp32 wgrad grid sizes (f32_block_slab_rows).
// ---------------------------------------------------------------------------
template <int C, int W_>
struct WgB {
  static constexpr int OT = C / 16, W = W_, TW = W + 2, BR = 128 / W;
  static constexpr int NO = C == 16 ? 1 : 2, TS = OT * (OT / NO), PS = C == 64 ? 1 : 4, NW = TS * PS, NTH = 64 * NW;
  static constexpr int C8 = C / 8, XCH = (BR + 2) * TW * C8, DCH = BR * W * C8;
  static constexpr int XPT = (XCH + NTH - 1) / NTH, DPT = (DCH + NTH - 1) / NTH;
  static constexpr int XE = (BR + 2) * TW * C, DE = BR * W * C;
  static constexpr int ACC = (9 + 1) * NO;  // accumulator tiles per wave (9 taps + db per o-tile)
  static constexpr size_t LDS = (size_t)(XE + DE) * 2 + (PS > 1 ? (size_t)TS * ACC * 256 * 4 : 0);
  static_assert(W == 8 || W == 16 || W == 32, "bf16 wgrad: W in {8, 16, 32}");
  __host__ __device__ static constexpr int swz(int P) {
    return C == 64 ? 2 * ((P >> 1) & 3) : C == 32 ? 2 * ((P >> 2) & 1) : 0;
  }
};

// one transposed-read k run: 4 pixels' 4 channels -> the lane's 4 bf16 of one channel
__device__ __forceinline__ s16x4 tr4(const bf16* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((ASR_LDS s16x4*)p);
}

// An item is 128 pixels: a band of BR = 128 / SW rows of an image SW wide, or (STRIP) a band of 4 rows x a
// strip of SW = 32 columns of an image Wimg wide (WgB<C, 32>'s tiles, waves and swizzle; a 32-pixel chunk is
// then one row of the strip).  MASKED false: dz = dy (the bare conv's weight gradient, B_CONV; dmask unused)
template <int C, int SW, bool STRIP, bool MASKED>
__global__ __launch_bounds__((WgB<C, SW>::NTH)) void k_wgradb(const bf16* __restrict__ x, const bf16* __restrict__ dy,
                                                            const uint8_t* __restrict__ dmask, int N, int H, float h,
                                                            int Wimg, float* __restrict__ slabs, long x_stride,
                                                            long dy_stride, long m_stride, long s_stride) {
  using G = WgB<C, SW>;
  static_assert(!STRIP || SW == kStripW, "a band x strip item is 4 x 32 pixels");
  const int W = STRIP ? Wimg : SW;
  // several layers in one launch (bands only): blockIdx.y is the layer (strides in elements / bytes / floats)
  if constexpr (!STRIP) {
    x += blockIdx.y * x_stride;
    dy += blockIdx.y * dy_stride;
    dmask += blockIdx.y * m_stride;
    slabs += blockIdx.y * s_stride;
  }
  constexpr int TW = G::TW, BR = G::BR, NO = G::NO, OT = G::OT, E = 9 * C * C;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_wb[];
  bf16* xt = (bf16*)lds_wb;               // [BR+2][TW][C] (chunk-swizzled per pixel)
  bf16* dzt = xt + G::XE;                 // [BR][SW][C]
  float* red = (float*)(dzt + G::DE);     // [TS][ACC][64][4] (PS > 1)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, lx = lane & 15;
  const int q = lx >> 2, pq = lx & 3;
  const int ts = wave % G::TS, ps = wave / G::TS;
  const int it = ts / (OT / NO), ob = (ts % (OT / NO)) * NO;
  const int nb = (H + BR - 1) / BR, ns = STRIP ? (W + SW - 1) / SW : 1;
  const long items = (long)N * nb * ns;
  const long i0 = (long)blockIdx.x * items / gridDim.x, i1 = (long)(blockIdx.x + 1) * items / gridDim.x;
  f32x4 acc[9][NO], accb[NO];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int o = 0; o < NO; ++o) acc[t][o] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int o = 0; o < NO; ++o) accb[o] = f32x4{0.f, 0.f, 0.f, 0.f};
  uint4 px[G::XPT], pd[G::DPT];
  unsigned pm[G::DPT];  // the relu bits, applied at the LDS store: masking here would wait for the loads
  auto fetch = [&](long item) {
    int n, y0, x0;
    strip_item<BR, SW>(item, nb, ns, n, y0, x0);
#pragma unroll
    for (int k = 0; k < G::XPT; ++k) {
      const int i = tid + k * G::NTH;
      px[k] = make_uint4(0u, 0u, 0u, 0u);
      const int r = i / (TW * G::C8), rem = i % (TW * G::C8), col = rem / G::C8, c8 = rem % G::C8;
      const int gy = y0 - 1 + r, gx = x0 - 1 + col;  // (halo columns: the neighbouring strips' pixels)
      if (i < G::XCH && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W)
        px[k] = *(const uint4*)(x + (((long)n * H + gy) * W + gx) * C + 8 * c8);
    }
#pragma unroll
    for (int k = 0; k < G::DPT; ++k) {
      const int i = tid + k * G::NTH;
      pd[k] = make_uint4(0u, 0u, 0u, 0u);
      pm[k] = 0u;
      const int P = i / G::C8, c8 = i % G::C8, r = P / SW, c = P % SW;
      // (rows past the image and, in a 16-column last strip, columns past it: zeros)
      if (i < G::DCH && y0 + r < H && (!STRIP || x0 + c < W)) {
        // (a band's rows are contiguous in the image)
        const long e = STRIP ? (((long)n * H + y0 + r) * W + x0 + c) * C + 8 * c8 : ((long)n * H + y0) * W * C + 8L * i;
        pd[k] = *(const uint4*)(dy + e);
        if constexpr (MASKED) pm[k] = dmask[e >> 3];
      }
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int k = 0; k < G::XPT; ++k) {
      const int i = tid + k * G::NTH;
      const int P = i / G::C8, c8 = i % G::C8;
      if (i < G::XCH) *(uint4*)(xt + P * C + 8 * (c8 ^ G::swz(P))) = px[k];
    }
#pragma unroll
    for (int k = 0; k < G::DPT; ++k) {
      const int i = tid + k * G::NTH;
      const int P = i / G::C8, c8 = i % G::C8;
      if (i < G::DCH) *(uint4*)(dzt + P * C + 8 * (c8 ^ G::swz(P))) = MASKED ? mask8_bf16(pd[k], pm[k]) : pd[k];
    }
  };
  // the lane's 8-B piece of channels 16 ch + 4 pq .. +3 at pixel P of a tile
  auto piece = [&](const bf16* tile, int P, int ch) {
    const int c16 = 2 * ch + (pq >> 1);
    return tile + P * C + 8 * (c16 ^ G::swz(P)) + 4 * (pq & 1);
  };
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  auto frag = [&](const bf16* tile, int P1, int P2, int ch) {
    const s16x4 a = tr4(piece(tile, P1, ch)), b = tr4(piece(tile, P2, ch));
    const s16x8 c = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    return __builtin_bit_cast(bf16x8, c);
  };
  bf16x8 ones;
#pragma unroll
  for (int j = 0; j < 8; ++j) ones[j] = (bf16)1.f;
  if (i0 < i1) fetch(i0);
  for (long item = i0; item < i1; ++item) {
    const int y0 = (int)((item / ns) % nb) * BR;
    // a 16-column last strip's missing half runs too: x and dz are both zero there, the products exactly 0
    const int rows = min(BR, H - y0), nch = STRIP ? rows : (rows * SW + 31) / 32;  // (32-pixel chunks: a strip's rows)
    __syncthreads();  // the previous item's operands consumed
    store();
    __syncthreads();
    if (item + 1 < i1) fetch(item + 1);  // in flight during this item's MFMAs
    for (int ch = ps; ch < nch; ch += G::PS) {  // (wave-uniform: EXEC stays full for the transposed reads)
      const int k1 = 32 * ch + 4 * g + q, k2 = k1 + 16;
      const int r1 = k1 / SW, c1 = k1 % SW, r2 = k2 / SW, c2 = k2 % SW;
      bf16x8 B[NO];
#pragma unroll
      for (int o = 0; o < NO; ++o) B[o] = frag(dzt, r1 * SW + c1, r2 * SW + c2, ob + o);
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int d = (t / 3) * TW + t % 3;
        const bf16x8 A = frag(xt, r1 * TW + c1 + d, r2 * TW + c2 + d, it);
#pragma unroll
        for (int o = 0; o < NO; ++o) acc[t][o] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A, B[o], acc[t][o], 0, 0, 0);
      }
      if (it == 0) {
#pragma unroll
        for (int o = 0; o < NO; ++o) accb[o] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, B[o], accb[o], 0, 0, 0);
      }
    }
  }
  // the PS chunk-split partials, summed in a fixed order through LDS (one split at a time)
  if constexpr (G::PS > 1) {
    float* mine = red + (long)ts * G::ACC * 256;
#pragma unroll 1
    for (int src = 1; src < G::PS; ++src) {
      __syncthreads();
      if (ps == src) {
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
          for (int o = 0; o < NO; ++o) *(f32x4*)(mine + ((t * NO + o) * 64 + lane) * 4) = acc[t][o];
#pragma unroll
        for (int o = 0; o < NO; ++o) *(f32x4*)(mine + ((9 * NO + o) * 64 + lane) * 4) = accb[o];
      }
      __syncthreads();
      if (ps == 0) {
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
          for (int o = 0; o < NO; ++o) acc[t][o] += *(const f32x4*)(mine + ((t * NO + o) * 64 + lane) * 4);
#pragma unroll
        for (int o = 0; o < NO; ++o) accb[o] += *(const f32x4*)(mine + ((9 * NO + o) * 64 + lane) * 4);
      }
    }
  }
  if (ps == 0) {
    float* slab = slabs + (long)blockIdx.x * (E + C);
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int o = 0; o < NO; ++o)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          slab[((long)t * C + 16 * it + 4 * g + e) * C + 16 * (ob + o) + lx] = h * acc[t][o][e];
    if (it == 0 && g == 0) {
#pragma unroll
      for (int o = 0; o < NO; ++o) slab[E + 16 * (ob + o) + lx] = h * accb[o][0];
    }
  }
}

// bands (128 pixels) per workgroup of k_wgradb (profiles/r05_he32_bf16_ab.txt; re-measured after round 6's
// reductions: profiles/r06ai_wgradb_grid_ab.txt)
static constexpr int wgradb_minb(int C) { return C == 16 ? 1 : C == 32 ? 8 : 32; }

// k_wgradb's grid over column strips = its slab rows (one [dW | db] slab per workgroup), for the launcher and
// for every workspace that keeps a block's slabs (bf16_block_slab_rows).  Items per workgroup as over bands
// (an item is 128 pixels there too); at most two workgroups per CU and kMaxBlockSlabs rows.
static int wgrad_strip_grid(int N, int H, int W, int C) {
  const long items = strip_items(N, H, W);
  const int minb = wgradb_minb(C);
  return (int)std::max<long>(1, std::min<long>({(items + minb - 1) / minb, 2L * launch_cus(), (long)kMaxBlockSlabs}));
}

// W: the image width (= SW unless STRIP).  Several layers per launch over bands only.
template <int C, int SW, bool STRIP, bool MASKED>
static int launch_wgradb(const bf16* x, const bf16* dy, const uint8_t* mask, int N, int H, int W, float h,
                         float* slabs, int* nslabs, hipStream_t s, int layers = 1, long x_stride = 0,
                         long dy_stride = 0, long m_stride = 0, long s_stride = 0) {
  using G = WgB<C, SW>;
  int grid;
  if constexpr (STRIP) {
    grid = wgrad_strip_grid(N, H, W, C);
  } else {
    // at most the fp32 wgrad's grid: the rows the workspaces size per block (f32_block_slab_rows)
    const long items = (long)N * ((H + G::BR - 1) / G::BR);
    constexpr int minb = wgradb_minb(C);
    grid = (int)std::max<long>(1, std::min<long>((items + minb - 1) / minb, f32_block_slab_rows(N, H, SW, C)));
  }
  hipLaunchKernelGGL((k_wgradb<C, SW, STRIP, MASKED>), dim3(grid, layers), dim3(G::NTH), G::LDS, s, x, dy, mask, N, H,
                     h, W, slabs, x_stride, dy_stride, m_stride, s_stride);
  ASR_LAUNCH_CHECK("k_wgradb");
  *nslabs = grid;
  return ASR_OK;
}

// Slab rows one bf16 3x3 block's weight gradient writes on the any-width kernels (convb_backward): the
// strip grid at W >= 48, else at most the fp32 MFMA grid (launch_wgradb)
int bf16_block_slab_rows(int N, int H, int W, int C) {
  if (wide_c(C) && convb_supported(W, C)) return wgrad_wide_rows(N, H, W, C);  // (k_wgradbw's pixel splits)
  return strip_width(W) && convb_supported(W, C) ? wgrad_strip_grid(N, H, W, C) : f32_block_slab_rows(N, H, W, C);
}

// ===========================================================================
// bf16 blocks at C in {128, 256} (k_convbw / k_wgradbw): k_convb's items, tiles,
// fragment maps and epilogue, but an o-tile's KS = 9C/32 A fragments (144 / 288
// VGPRs) no longer fit in registers, and k_wgradb's 9 (C/16)^2 accumulator
// tiles no longer fit in a workgroup.
// Forward / dgrad (k_convbw): 8 waves; a wave owns a pair of o-tiles (one B read
// from LDS feeds two MFMAs) and every 16-pixel tile of one item: 2 x NTW <= 16
// accumulators.  C = 256 has 8 pairs: a workgroup runs one item per pass over
// the pack.  C = 128 has 4: it stages two items and runs them in one pass (wave
// = pair x item), which halves the pack bytes read per item.  A wave streams its
// pair's A fragments from the pack (L2-resident) in chunks of KQ = 4 k-steps (2
// where it holds 16 accumulators: registers), the next chunk's loads in flight
// during this chunk's MFMAs.  The LDS tile of an item is k_convb's (6 x (SW + 2)
// pixels, C + 8 elements a pixel: 55.5 KB at C = 128, twice that for the pass's
// two items; 107.7 KB at 256); B_EULER takes the epilogue's dy
// term from global memory (the item has just read it), so only the dz tile
// lives in LDS.
// Weight gradient (k_wgradbw): k_wgradb's C = 64 geometry on a (i-block,
// o-block) pair of 64 x 64 channels, blockIdx.y = ib * (C/64) + ob: the
// workgroup stages those 128-B slices of x and dz, walks its share (blockIdx.x
// of gridDim.x pixel splits) of the 128-pixel items and writes its block of slab
// row blockIdx.x; db from the ib = 0 workgroups.
// ===========================================================================
template <int C, int SW>
struct BfWide {
  static constexpr int OT = C / 16, TW = SW + 2, BR = 4, PS = C + 8, TILEE = (BR + 2) * TW * PS;
  static constexpr int T = BR * SW / 16;  // 16-pixel tiles per item
  static constexpr int NW = 8, NTH = 64 * NW;
  // o-tile pairs; items per pass over W (a wave per pair and item); tiles per wave: all of its item's
  static constexpr int NOP = OT / 2, IPP = NW / NOP, NTW = T;
  static constexpr int KS = 9 * C / 32, KQ = NTW == 8 ? 2 : 4, NQ = KS / KQ, QT = C / 32 / KQ;  // k-steps, chunk, chunks, chunks per tap
  static constexpr int C8 = C / 8, NCH = (BR + 2) * TW * C8, NPT = (NCH + NTH - 1) / NTH;
  static constexpr int NPT4 = (NPT + 3) / 4 * 4;  // staging: groups of 4 chunks per thread (the tail past NCH idle)
  static constexpr size_t LDS = (size_t)IPP * TILEE * 2;
  static_assert(C == 128 || C == 256, "wide bf16 band: C in {128, 256}");
  static_assert(SW == 8 || SW == 16 || SW == 32, "wide bf16 band: W in {8, 16, 32}");
  static_assert(NOP * IPP == NW && NQ * KQ == KS && QT * KQ * 32 == C && LDS <= 160 * 1024, "wide bf16 band: geometry");
};

template <int C, int SW, bool STRIP, int MODE>
__global__ __launch_bounds__(512) void k_convbw(const bf16* __restrict__ xin, bf16* __restrict__ out,
                                                uint8_t* __restrict__ mask, const bf16* __restrict__ wpack,
                                                const float* __restrict__ bias, float h, float two_gamma, int N, int H,
                                                int Wimg, const uint8_t* __restrict__ dmask) {
  using G = BfWide<C, SW>;
  static_assert(!STRIP || SW == kStripW, "a band x strip item is 4 x 32 pixels");
  constexpr int TW = G::TW, BR = G::BR, KS = G::KS, C8 = G::C8, NTW = G::NTW, PS = G::PS, KQ = G::KQ, NQ = G::NQ;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_cw[];
  // [IPP][BR+2][TW][PS]: x, or dz = dy & mask (B_EULER), of the pass's items; this wave's item is ph
  bf16* tile = (bf16*)lds_cw + (threadIdx.x >> 6) / G::NOP * G::TILEE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, lx = lane & 15;
  const int ot0 = 2 * (wave % G::NOP), ph = wave / G::NOP;
  const int W = STRIP ? Wimg : SW;
  const int nb = (H + BR - 1) / BR, ns = STRIP ? (W + SW - 1) / SW : 1;
  const long items = (long)N * nb * ns;
  // persistent over passes of IPP items
  const long passes = (items + G::IPP - 1) / G::IPP;
  const long i0 = (long)blockIdx.x * passes / gridDim.x * G::IPP;
  const long i1 = min(items, (long)(blockIdx.x + 1) * passes / gridDim.x * G::IPP);
  f32x4 bz[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  if ((MODE == F_EULER || MODE == F_CONV) && bias) {
#pragma unroll
    for (int o = 0; o < 2; ++o) bz[o] = *(const f32x4*)(bias + 16 * (ot0 + o) + 4 * g);
  }
  // fragment (ot, ks) of the pack: 1 KB at ((ot KS + ks) 64 + lane) 8
  const bf16* wl = wpack + ((long)ot0 * KS * 64 + lane) * 8;
  // lane lx's pixel of tile tau is item pixel 16 tau + lx
  int tb[NTW], trow[NTW], tpx[NTW];
#pragma unroll
  for (int j = 0; j < NTW; ++j) {
    const int bp = 16 * j + lx;
    trow[j] = bp / SW;
    tpx[j] = bp % SW;
    tb[j] = (trow[j] * TW + tpx[j]) * PS + 8 * g;
  }
  for (long base = i0; base < i1; base += G::IPP) {
    __syncthreads();  // the previous pass's tiles consumed
    // stage rows y0-1 .. y0+BR, columns x0-1 .. x0+SW of each item of the pass (zeros outside the image),
    // 4 loads in flight per thread (rolled: unrolled, every chunk's addresses stay in registers across the
    // item loop)
#pragma unroll 1
    for (int k0 = 0; k0 < G::IPP * G::NPT4; k0 += 4) {
      const int u = k0 / G::NPT4, ku = k0 % G::NPT4;
      if (base + u >= i1) break;  // (an odd last pass: one item)
      bf16* stile = (bf16*)lds_cw + u * G::TILEE;
      int n, y0, x0;
      strip_item<BR, SW>(base + u, nb, ns, n, y0, x0);
      uint4 v[4];
      unsigned pm[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int i = tid + G::NTH * (ku + k);
        const int r = i / (TW * C8), rem = i % (TW * C8), col = rem / C8, c8 = rem % C8;
        const int gy = y0 - 1 + r, gx = x0 - 1 + col;
        v[k] = make_uint4(0u, 0u, 0u, 0u);
        pm[k] = 0u;
        if (i < G::NCH && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W) {
          const long e = (((long)n * H + gy) * W + gx) * C + 8 * c8;
          v[k] = *(const uint4*)(xin + e);
          if (MODE == B_EULER) pm[k] = dmask[e >> 3];
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int i = tid + G::NTH * (ku + k);
        const int r = i / (TW * C8), rem = i % (TW * C8), col = rem / C8, c8 = rem % C8;
        if (i < G::NCH) *(uint4*)(stile + (r * TW + col) * PS + 8 * c8) = MODE == B_EULER ? mask8_bf16(v[k], pm[k]) : v[k];
      }
    }
    __syncthreads();
    const long item = base + ph;
    if (item >= i1) continue;  // (wave-uniform; the next pass begins with the barrier)
    int n, y0, x0;
    strip_item<BR, SW>(item, nb, ns, n, y0, x0);
    f32x4 acc[2][NTW];
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
      for (int j = 0; j < NTW; ++j) acc[o][j] = bz[o];
    bf16x8 Aa[KQ][2], Ab[KQ][2];
    auto load_a = [&](bf16x8(&A)[KQ][2], int q) {
#pragma unroll
      for (int s = 0; s < KQ; ++s)
#pragma unroll
        for (int o = 0; o < 2; ++o) A[s][o] = *(const bf16x8*)(wl + ((long)o * KS + KQ * q + s) * 512);
    };
    // chunk q: k-steps KQ q .. KQ q + KQ - 1 = tap t, channels c0 + 32 s + 8 g .. + 7 of the pixel shifted by t
    auto mac = [&](const bf16x8(&A)[KQ][2], int q) {
      const int t = q / G::QT, c0 = (q % G::QT) * (32 * KQ);
      const int off = ((t / 3) * TW + t % 3) * PS + c0;
#pragma unroll
      for (int s = 0; s < KQ; ++s)
#pragma unroll
        for (int j = 0; j < NTW; ++j) {
          const uint4 bv = *(const uint4*)(tile + tb[j] + off + 32 * s);
#pragma unroll
          for (int o = 0; o < 2; ++o)
            acc[o][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[s][o], __builtin_bit_cast(bf16x8, bv), acc[o][j], 0, 0, 0);
        }
    };
    load_a(Aa, 0);
#pragma unroll 1
    for (int q = 0; q < NQ; q += 2) {
      if (q + 1 < NQ) load_a(Ab, q + 1);
      mac(Aa, q);
      if (q + 2 < NQ) load_a(Aa, q + 2);
      if (q + 1 < NQ) mac(Ab, q + 1);
    }
    mfma_bf16_settle();  // (the epilogue branches: every path must see the result's wait states)
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
      for (int j = 0; j < NTW; ++j) {
        const int ot = ot0 + o, r = trow[j], px = tpx[j];
        const bool ok = y0 + r < H && (!STRIP || x0 + px < W);  // (rows past the image; a 16-column last strip)
        const long pix = ((long)n * H + y0 + r) * W + x0 + px;
        const long oi = pix * C + 16 * ot + 4 * g;  // this lane's 4 channels
        const uint2 cw = *(const uint2*)(tile + ((r + 1) * TW + px + 1) * PS + 16 * ot + 4 * g);  // x or dz at the pixel
        const float ctr[4] = {__uint_as_float(cw.x << 16), __uint_as_float(cw.x & 0xffff0000u),
                              __uint_as_float(cw.y << 16), __uint_as_float(cw.y & 0xffff0000u)};
        const f32x4 a = acc[o][j];
        float v[4];
        if constexpr (MODE == F_EULER) {
          unsigned nib = 0;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            nib |= (a[e] > 0.f ? 1u : 0u) << e;
            v[e] = fmaf(h, fmaxf(a[e], 0.f), ctr[e]);
          }
          if (mask) {  // the pixel's 16 channels of this o-tile: 4 nibbles, one 16-bit store
            unsigned m = nib << (4 * g);
            m |= (unsigned)__shfl_xor((int)m, 16, 64);
            m |= (unsigned)__shfl_xor((int)m, 32, 64);
            if (g == 0 && ok) *(uint16_t*)(mask + (pix * C + 16 * ot) / 8) = (uint16_t)m;
          }
        } else if constexpr (MODE == F_CONV) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = a[e];
        } else if constexpr (MODE == B_CONV) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = fmaf(two_gamma, ctr[e], -a[e]);
        } else {  // B_EULER: the tile holds dz = dy & mask, dy itself from global memory
          uint2 dw = make_uint2(0u, 0u);
          if (ok) dw = *(const uint2*)(xin + oi);
          const float d0[4] = {__uint_as_float(dw.x << 16), __uint_as_float(dw.x & 0xffff0000u),
                               __uint_as_float(dw.y << 16), __uint_as_float(dw.y & 0xffff0000u)};
          const float hg = h * two_gamma;
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = fmaf(hg, ctr[e], fmaf(-h, a[e], d0[e]));
        }
        if (ok) *(uint2*)(out + oi) = make_uint2(pk_bf16_rn(v[0], v[1]), pk_bf16_rn(v[2], v[3]));
      }
  }
}

// W: the image width (= SW unless STRIP)
template <int C, int SW, bool STRIP, int MODE>
static int launch_convbw(const bf16* xin, bf16* out, uint8_t* mask, const bf16* w, const float* bias, float h,
                         float two_gamma, int N, int H, int W, const uint8_t* dmask, hipStream_t s) {
  using G = BfWide<C, SW>;
  constexpr size_t lds = G::LDS;
  if (lds > 64 * 1024) {  // above the default dynamic-LDS limit: raised once per instantiation and device
    static bool raised[64];
    int dev = 0;
    ASR_TRY(hip_check(hipGetDevice(&dev), "hipGetDevice"));
    if (dev < 0 || dev >= 64 || !raised[dev]) {
      ASR_TRY(hip_check(hipFuncSetAttribute((const void*)k_convbw<C, SW, STRIP, MODE>,
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds),
                        "hipFuncSetAttribute"));
      if (dev >= 0 && dev < 64) raised[dev] = true;
    }
  }
  const long items = STRIP ? strip_items(N, H, W) : (long)N * ((H + 3) / 4);
  const long passes = (items + G::IPP - 1) / G::IPP;  // (a pass: IPP items under one read of the pack)
  const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(2, 160 * 1024 / lds));  // persistent workgroups per CU
  const long grid = std::max<long>(1, std::min<long>(passes, (long)per_cu * launch_cus()));
  hipLaunchKernelGGL((k_convbw<C, SW, STRIP, MODE>), dim3((unsigned)grid), dim3(G::NTH), lds, s, xin, out, mask, w, bias,
                     h, two_gamma, N, H, W, dmask);
  ASR_LAUNCH_CHECK("k_convbw");
  return ASR_OK;
}

// k_wgradb's C = 64 workgroup on channel blocks (ib, ob) of an image CT channels deep.  An item is 128 pixels
// as there; the workgroup's share of the items is blockIdx.x of gridDim.x, its slab row blockIdx.x.
template <int CT, int SW, bool STRIP, bool MASKED>
__global__ __launch_bounds__((WgB<64, SW>::NTH)) void k_wgradbw(const bf16* __restrict__ x, const bf16* __restrict__ dy,
                                                               const uint8_t* __restrict__ dmask, int N, int H, float h,
                                                               int Wimg, float* __restrict__ slabs) {
  constexpr int C = 64, NB = CT / C;
  using G = WgB<C, SW>;
  static_assert(!STRIP || SW == kStripW, "a band x strip item is 4 x 32 pixels");
  static_assert(G::PS == 1 && G::NO == 2, "k_wgradbw: the C = 64 wave layout");
  const int W = STRIP ? Wimg : SW;
  const int ib = blockIdx.y / NB, obk = blockIdx.y % NB;  // the input- and output-channel blocks
  constexpr int TW = G::TW, BR = G::BR, NO = G::NO, OT = G::OT;
  constexpr long E = 9L * CT * CT;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_ww[];
  bf16* xt = (bf16*)lds_ww;  // [BR+2][TW][64] (chunk-swizzled per pixel)
  bf16* dzt = xt + G::XE;    // [BR][SW][64]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, lx = lane & 15;
  const int q = lx >> 2, pq = lx & 3;
  const int it = wave / (OT / NO), ob = (wave % (OT / NO)) * NO;
  const int nb = (H + BR - 1) / BR, ns = STRIP ? (W + SW - 1) / SW : 1;
  const long items = (long)N * nb * ns;
  const long i0 = (long)blockIdx.x * items / gridDim.x, i1 = (long)(blockIdx.x + 1) * items / gridDim.x;
  f32x4 acc[9][NO], accb[NO];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int o = 0; o < NO; ++o) acc[t][o] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int o = 0; o < NO; ++o) accb[o] = f32x4{0.f, 0.f, 0.f, 0.f};
  uint4 px[G::XPT], pd[G::DPT];
  unsigned pm[G::DPT];  // the relu bits, applied at the LDS store
  auto fetch = [&](long item) {
    int n, y0, x0;
    strip_item<BR, SW>(item, nb, ns, n, y0, x0);
#pragma unroll
    for (int k = 0; k < G::XPT; ++k) {
      const int i = tid + k * G::NTH;
      px[k] = make_uint4(0u, 0u, 0u, 0u);
      const int r = i / (TW * G::C8), rem = i % (TW * G::C8), col = rem / G::C8, c8 = rem % G::C8;
      const int gy = y0 - 1 + r, gx = x0 - 1 + col;  // (halo columns: the neighbouring strips' pixels)
      if (i < G::XCH && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W)
        px[k] = *(const uint4*)(x + (((long)n * H + gy) * W + gx) * CT + C * ib + 8 * c8);
    }
#pragma unroll
    for (int k = 0; k < G::DPT; ++k) {
      const int i = tid + k * G::NTH;
      pd[k] = make_uint4(0u, 0u, 0u, 0u);
      pm[k] = 0u;
      const int P = i / G::C8, c8 = i % G::C8, r = P / SW, c = P % SW;
      // (rows past the image and, in a 16-column last strip, columns past it: zeros)
      if (i < G::DCH && y0 + r < H && (!STRIP || x0 + c < W)) {
        const long e = (((long)n * H + y0 + r) * W + x0 + c) * CT + C * obk + 8 * c8;
        pd[k] = *(const uint4*)(dy + e);
        if constexpr (MASKED) pm[k] = dmask[e >> 3];
      }
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int k = 0; k < G::XPT; ++k) {
      const int i = tid + k * G::NTH;
      const int P = i / G::C8, c8 = i % G::C8;
      if (i < G::XCH) *(uint4*)(xt + P * C + 8 * (c8 ^ G::swz(P))) = px[k];
    }
#pragma unroll
    for (int k = 0; k < G::DPT; ++k) {
      const int i = tid + k * G::NTH;
      const int P = i / G::C8, c8 = i % G::C8;
      if (i < G::DCH) *(uint4*)(dzt + P * C + 8 * (c8 ^ G::swz(P))) = MASKED ? mask8_bf16(pd[k], pm[k]) : pd[k];
    }
  };
  // the lane's 8-B piece of channels 16 ch + 4 pq .. +3 at pixel P of a tile
  auto piece = [&](const bf16* tile, int P, int ch) {
    const int c16 = 2 * ch + (pq >> 1);
    return tile + P * C + 8 * (c16 ^ G::swz(P)) + 4 * (pq & 1);
  };
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  auto frag = [&](const bf16* tile, int P1, int P2, int ch) {
    const s16x4 a = tr4(piece(tile, P1, ch)), b = tr4(piece(tile, P2, ch));
    const s16x8 c = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    return __builtin_bit_cast(bf16x8, c);
  };
  bf16x8 ones;
#pragma unroll
  for (int j = 0; j < 8; ++j) ones[j] = (bf16)1.f;
  if (i0 < i1) fetch(i0);
  for (long item = i0; item < i1; ++item) {
    const int y0 = (int)((item / ns) % nb) * BR;
    const int rows = min(BR, H - y0), nch = STRIP ? rows : (rows * SW + 31) / 32;  // (32-pixel chunks: a strip's rows)
    __syncthreads();  // the previous item's operands consumed
    store();
    __syncthreads();
    if (item + 1 < i1) fetch(item + 1);  // in flight during this item's MFMAs
    for (int ch = 0; ch < nch; ++ch) {  // (wave-uniform: EXEC stays full for the transposed reads)
      const int k1 = 32 * ch + 4 * g + q, k2 = k1 + 16;
      const int r1 = k1 / SW, c1 = k1 % SW, r2 = k2 / SW, c2 = k2 % SW;
      bf16x8 B[NO];
#pragma unroll
      for (int o = 0; o < NO; ++o) B[o] = frag(dzt, r1 * SW + c1, r2 * SW + c2, ob + o);
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int d = (t / 3) * TW + t % 3;
        const bf16x8 A = frag(xt, r1 * TW + c1 + d, r2 * TW + c2 + d, it);
#pragma unroll
        for (int o = 0; o < NO; ++o) acc[t][o] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A, B[o], acc[t][o], 0, 0, 0);
      }
      if (ib == 0 && it == 0) {  // (db once per o-block: the ib = 0 workgroups)
#pragma unroll
        for (int o = 0; o < NO; ++o) accb[o] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, B[o], accb[o], 0, 0, 0);
      }
    }
  }
  float* slab = slabs + (long)blockIdx.x * (E + CT);
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int o = 0; o < NO; ++o)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        slab[((long)t * CT + C * ib + 16 * it + 4 * g + e) * CT + C * obk + 16 * (ob + o) + lx] = h * acc[t][o][e];
  if (ib == 0 && it == 0 && g == 0) {
#pragma unroll
    for (int o = 0; o < NO; ++o) slab[E + C * obk + 16 * (ob + o) + lx] = h * accb[o][0];
  }
}

// k_wgradbw's pixel splits = its slab rows (launcher and every workspace): at least 8 items (1024 pixels) a
// workgroup, two workgroups per CU over the (C/64)^2 channel-block pairs, at most 48 MB of slabs
static int wgrad_wide_rows(int N, int H, int W, int C) {
  const long items = strip_width(W) ? strip_items(N, H, W) : (long)N * ((H + 128 / W - 1) / (128 / W));
  const long nblk = (long)(C / 64) * (C / 64), cap = 48000000L / ((9L * C * C + C) * 4);
  return (int)std::max<long>(1, std::min<long>({(items + 7) / 8, std::max<long>(1, 2L * launch_cus() / nblk), cap}));
}

template <int C, int SW, bool STRIP, bool MASKED>
static int launch_wgradbw(const bf16* x, const bf16* dy, const uint8_t* mask, int N, int H, int W, float h,
                          float* slabs, int* nslabs, hipStream_t s) {
  using G = WgB<64, SW>;
  const int rows = wgrad_wide_rows(N, H, W, C);
  hipLaunchKernelGGL((k_wgradbw<C, SW, STRIP, MASKED>), dim3(rows, (C / 64) * (C / 64)), dim3(G::NTH), G::LDS, s, x, dy,
                     mask, N, H, h, W, slabs);
  ASR_LAUNCH_CHECK("k_wgradbw");
  *nslabs = rows;
  return ASR_OK;
}

// The any-width kernels' instantiation for (C, W): f(C, SW, STRIP) as integral constants, the tile width and
// the strip flag chosen here alone -- (32, true) at a strip width, else (W, false); ASR_E_UNSUPPORTED off
// convb_supported's shapes
static constexpr bool convb_tile(int, int) { return true; }  // (dispatch_c_w's predicate: every C x tile width)
template <typename F>
static int dispatch_c_sw(const char* what, int C, int W, F&& f) {
  if (!convb_supported(W, C)) return fail(ASR_E_UNSUPPORTED, "%s: C=%d W=%d", what, C, W);
  const bool strip = strip_width(W);
  return dispatch_c_w<convb_tile>(what, C, strip ? kStripW : W, [&](auto c, auto sw) -> int {
    if constexpr (decltype(sw)::value == kStripW)
      if (strip) return f(c, sw, std::true_type{});
    return f(c, sw, std::false_type{});
  });
}

// y = x + h relu(conv(x, W) + b) in bf16 (w: asr_theta_to_w's ASR_BF16 pack of one layer); with
// conv_only the bare layer call y = conv(x, W) + b (…3By3.py:157-171; no mask, h unused)
int convb_forward(const void* x, void* y, uint8_t* mask, const void* w, const float* bias, float h, int N, int H, int W,
                  int C, hipStream_t s, bool conv_only) {
  return dispatch_c_sw("conv bf16 (any width)", C, W, [&](auto c, auto sw, auto strip) -> int {
    constexpr int CC = decltype(c)::value, SW = decltype(sw)::value;
    constexpr bool ST = decltype(strip)::value;
    if constexpr (CC >= 128) {  // W streamed from the pack
      if (conv_only)
        return launch_convbw<CC, SW, ST, F_CONV>((const bf16*)x, (bf16*)y, nullptr, (const bf16*)w, bias, 1.f, 0.f, N,
                                                 H, W, nullptr, s);
      return launch_convbw<CC, SW, ST, F_EULER>((const bf16*)x, (bf16*)y, mask, (const bf16*)w, bias, h, 0.f, N, H, W,
                                                nullptr, s);
    } else {
      if (conv_only)
        return launch_convb<CC, SW, ST, F_CONV>((const bf16*)x, (bf16*)y, nullptr, (const bf16*)w, bias, 1.f, 0.f, N, H,
                                                W, nullptr, s);
      return launch_convb<CC, SW, ST, F_EULER>((const bf16*)x, (bf16*)y, mask, (const bf16*)w, bias, h, 0.f, N, H, W,
                                               nullptr, s);
    }
  });
}

// The Euler block's backward in bf16: dx = dy - h conv(dy & mask, W) + 2 gamma h (dy & mask)
// (W: the forward pack for antisymmetric operators, whose transpose is -A + 2 gamma I; the
// transposed operator's pack with gamma = 0 otherwise) and the weight-gradient slabs
// (k_wgradb on the bf16 x and dz = dy & mask, h on the fp32 sums).  conv_only: the bare layer
// call's backward, dz = dy: dx = -conv(dy, W) + 2 gamma dy, slabs of x (x) dy (h unused)
int convb_backward(const void* dy, const uint8_t* mask, const void* x, const void* w, float h, float two_gamma, int N,
                   int H, int W, int C, void* dx, bool need_w, float* slabs, int* nslabs, hipStream_t s,
                   bool conv_only) {
  *nslabs = 0;
  return dispatch_c_sw("conv bf16 backward (any width)", C, W, [&](auto c, auto sw, auto strip) -> int {
    constexpr int CC = decltype(c)::value, SW = decltype(sw)::value;
    constexpr bool ST = decltype(strip)::value;
    if constexpr (CC >= 128) {  // W streamed from the pack; the weight gradient over channel blocks
      if (dx) {
        if (conv_only)
          ASR_TRY((launch_convbw<CC, SW, ST, B_CONV>((const bf16*)dy, (bf16*)dx, nullptr, (const bf16*)w, nullptr, 1.f,
                                                     two_gamma, N, H, W, nullptr, s)));
        else
          ASR_TRY((launch_convbw<CC, SW, ST, B_EULER>((const bf16*)dy, (bf16*)dx, nullptr, (const bf16*)w, nullptr, h,
                                                      two_gamma, N, H, W, mask, s)));
      }
      if (!need_w) return ASR_OK;
      if (conv_only)
        return launch_wgradbw<CC, SW, ST, false>((const bf16*)x, (const bf16*)dy, nullptr, N, H, W, 1.f, slabs, nslabs,
                                                 s);
      return launch_wgradbw<CC, SW, ST, true>((const bf16*)x, (const bf16*)dy, mask, N, H, W, h, slabs, nslabs, s);
    } else {
      if (dx) {
        if (conv_only)
          ASR_TRY((launch_convb<CC, SW, ST, B_CONV>((const bf16*)dy, (bf16*)dx, nullptr, (const bf16*)w, nullptr, 1.f,
                                                    two_gamma, N, H, W, nullptr, s)));
        else
          ASR_TRY((launch_convb<CC, SW, ST, B_EULER>((const bf16*)dy, (bf16*)dx, nullptr, (const bf16*)w, nullptr, h,
                                                     two_gamma, N, H, W, mask, s)));
      }
      if (!need_w) return ASR_OK;
      if (conv_only)
        return launch_wgradb<CC, SW, ST, false>((const bf16*)x, (const bf16*)dy, nullptr, N, H, W, 1.f, slabs, nslabs, s);
      return launch_wgradb<CC, SW, ST, true>((const bf16*)x, (const bf16*)dy, mask, N, H, W, h, slabs, nslabs, s);
    }
  });
}

// The bf16 weight-gradient slabs of L layers in one launch (k_wgradb over bands, blockIdx.y = layer):
// wgrad_layers' bf16 half (asr_stage_img.hip)
static constexpr bool wgradb_layers_c_w(int C, int) { return C <= 64; }
int wgradb_layers(const bf16* x0, long x_stride, const bf16* dys, long d_stride, const uint8_t* masks, long mask_stride,
                  float h, int N, int H, int W, int C, int L, float* slabs, long slab_stride, int* nslabs,
                  hipStream_t s) {
  return dispatch_c_w<wgradb_layers_c_w>("bf16 weight gradient", C, W, [&](auto c, auto sw) -> int {
    return launch_wgradb<decltype(c)::value, decltype(sw)::value, false, true>(
        x0, dys, masks, N, H, W, h, slabs, nslabs, s, L, x_stride, d_stride, mask_stride, slab_stride);
  });
}

}  // namespace asr
