// fp32 path of the 3x3 conv / Euler block: fp32 MFMA (v_mfma_f32_16x16x4_f32)
// for the network's blocks (C in {16, 32, 64}, W in {32, 16, 8}: the single-stage
// nets and the stages of the multi-stage ones), exact fp32 FMA chains on the
// VALU for every other shape.
//
// This is the reference-precision path (the reference computes everything in
// fp32, layers/tfkeras_layer_Conv2DAntisymmetric3By3.py:157-171), used for the
// fp32 parity configuration (BASELINE config 1), for shapes the bf16 MFMA
// kernels do not cover, and for the stem conv (models/tfkeras_resnets.py:563-572,
// a regular 3x3 conv with C_in = 3).  It shares the mask layout, the theta
// projection and the API with the bf16 path (asr_conv_bf16.hip, which sizes
// its weight-gradient grid by f32_block_slab_rows here; asr_stage_img.hip runs
// k_wgrad32 over a stage's layers through wgrad32_layers).  At the end, the
// elementwise bf16 <-> fp32 conversion of the multi-stage nets' transitions.
#include "asr_common.h"
#include "asr_conv3x3.h"
#include "asr_internal.h"

namespace asr {

// One wave = (n, y, 16-pixel tile, 16-channel tile).  Lane (g = lane>>4,
// lx = lane&15) computes pixel 16*pt+lx, channels 16*ot+4g .. +3 (the MFMA D
// fragment map).  Relu mask: bit (pixel*C + o) (asr.h), set with atomicOr on
// a zeroed buffer because C need not be a multiple of 8 here.  K x K kernel
// (odd K, SAME: pad K/2), HWIO weights [K][K][Ci][Co].
template <typename Tout, int MODE>
__global__ __launch_bounds__(256) void k_conv_f32(const float* __restrict__ xin, Tout* __restrict__ out,
                                                  uint32_t* __restrict__ mask, const float* __restrict__ w,
                                                  const float* __restrict__ bias, float h, float two_gamma,
                                                  const float* __restrict__ dy, const float* __restrict__ extra,
                                                  int N, int H, int W, int Ci, int Co, int K) {
  const int PT = (W + 15) / 16, OT = (Co + 15) / 16;
  const long tasks = (long)N * H * PT * OT;
  const long task = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (task >= tasks) return;
  const int lane = threadIdx.x & 63, g = lane >> 4, lx = lane & 15;
  const int ot = (int)(task % OT);
  long rest = task / OT;
  const int pt = (int)(rest % PT);
  rest /= PT;
  const int y = (int)(rest % H);
  const int n = (int)(rest / H);
  const int px = 16 * pt + lx;
  const int o0 = 16 * ot + 4 * g;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  if (px < W) {
    for (int tap = 0; tap < K * K; ++tap) {
      const int gy = y + tap / K - K / 2, gx = px + tap % K - K / 2;
      if (gy < 0 || gy >= H || gx < 0 || gx >= W) continue;
      const float* xp = xin + (((long)n * H + gy) * W + gx) * Ci;
      const float* wp = w + (long)tap * Ci * Co;
      for (int i = 0; i < Ci; ++i) {
        const float xv = xp[i];
        const float* wr = wp + (long)i * Co + o0;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (o0 + e < Co) acc[e] = fmaf(xv, wr[e], acc[e]);
      }
    }
  }
  const long pix = (((long)n * H + y) * W + px);
  unsigned nib = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int o = o0 + e;
    const bool ok = px < W && o < Co;
    float v = 0.f;
    if constexpr (MODE <= F_RELU) {
      const float z = acc[e] + ((bias && o < Co) ? bias[o] : 0.f);
      if constexpr (MODE == F_EULER) {
        if (ok && z > 0.f) nib |= 1u << e;
        // residual: the input, or `extra` (the step input of the second RK2 stage)
        if (ok) v = (extra ? extra[pix * Co + o] : xin[pix * Ci + o]) + h * fmaxf(z, 0.f);
      } else if constexpr (MODE == F_CONV) {
        v = z;
      } else {
        v = fmaxf(z, 0.f);
      }
    } else {
      // dgrad: xin holds dz (float), dy the incoming gradient (float)
      if (ok) {
        const float dz = xin[pix * Ci + o];
        v = (MODE == B_EULER ? dy[pix * Co + o] : 0.f) - acc[e] + two_gamma * dz;
        if (extra) v += extra[pix * Co + o];  // RK2 first stage: + the step's outer dy
      }
    }
    if (ok) out[pix * Co + o] = from_f32<Tout>(v);
  }
  if constexpr (MODE == F_EULER) {
    if (mask && nib) {
      const long b0 = pix * Co + o0;  // first of this lane's 4 channels
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if ((nib >> e) & 1u) atomicOr(mask + ((b0 + e) >> 5), 1u << ((b0 + e) & 31));
    }
  }
}

// dz = h*dy*mask (EULER), dy (CONV) or dy*[src > 0] (RELU), as float.
template <typename T>
__global__ void k_make_dz(const T* __restrict__ dy, const uint8_t* __restrict__ mask, const T* __restrict__ relu_src,
                          int mode, float h, int N, int H, int W, int C, float* __restrict__ dz) {
  const long P = (long)N * H * W * C;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < P; idx += (long)gridDim.x * blockDim.x) {
    const float d = to_f32(dy[idx]);
    float v = d;
    if (mode == F_EULER) {
      v = ((mask[idx >> 3] >> (idx & 7)) & 1) ? h * d : 0.f;  // bit idx = pixel*C + o
    } else if (mode == F_RELU) {
      v = to_f32(relu_src[idx]) > 0.f ? d : 0.f;
    }
    dz[idx] = v;
  }
}

// dW[tap][i][o] partial over a chunk of image rows:
//   slab[chunk][(tap*Ci + i)*Co + o] = sum_{rows in chunk, px} x[p+s(tap)][i] * dz[p][o]
// (slab rows are E + Co floats: dW partial then the db partial of k_db_f32)
template <typename Tx>
__global__ __launch_bounds__(256) void k_wgrad_f32(const Tx* __restrict__ x, const float* __restrict__ dz, int N,
                                                   int H, int W, int Ci, int Co, int rows_per_chunk,
                                                   float* __restrict__ slabs, int K) {
  const long E = (long)K * K * Ci * Co;
  const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (e >= E) return;
  const int o = (int)(e % Co);
  const int i = (int)((e / Co) % Ci);
  const int tap = (int)(e / ((long)Ci * Co));
  const int sy = tap / K - K / 2, sx = tap % K - K / 2;
  const long R = (long)N * H;
  const long r0 = (long)blockIdx.y * rows_per_chunk, r1 = min(R, r0 + rows_per_chunk);
  float acc = 0.f;
  for (long rr = r0; rr < r1; ++rr) {
    const int y = (int)(rr % H);
    const int n = (int)(rr / H);
    const int gy = y + sy;
    if (gy < 0 || gy >= H) continue;
    const Tx* xr = x + ((long)n * H + gy) * W * Ci;
    const float* dr = dz + ((long)n * H + y) * W * Co;
    const int p0 = max(0, -sx), p1 = min(W, W - sx);
    for (int p = p0; p < p1; ++p) acc = fmaf(to_f32(xr[(long)(p + sx) * Ci + i]), dr[(long)p * Co + o], acc);
  }
  slabs[(long)blockIdx.y * (E + Co) + e] = acc;
}

// db partial per chunk of pixel rows, into the slab row tail: slabs[chunk][E + o]
__global__ void k_db_f32(const float* __restrict__ dz, long rows, int W, int C, int rows_per_chunk, long E,
                         float* __restrict__ slabs) {
  const int o = threadIdx.x;
  if (o >= C) return;
  const long r0 = (long)blockIdx.x * rows_per_chunk, r1 = min(rows, r0 + rows_per_chunk);
  float acc = 0.f;
  for (long p = r0 * W; p < r1 * W; ++p) acc += dz[p * C + o];
  slabs[(long)blockIdx.x * (E + C) + E + o] = acc;
}

// ===========================================================================
// fp32 on the matrix cores: v_mfma_f32_16x16x4_f32 (fp32 operands, fp32
// accumulation: the reference's precision, …3By3.py:157-171) for the 3x3
// SAME conv / Euler block with C_in = C_out = C in {16, 32, 64}, W in {32, 16, 8}.
//
// Forward / dgrad (k_conv32): implicit GEMM D[o][px] = sum_kappa W^T[o][kappa]
// X[kappa][px], kappa = (tap, i).  A workgroup (4 waves) owns a band of BR = 4
// output rows of one image: the BR + 2 input rows (zero rows outside the
// image, zero halo columns) are staged in LDS once, every wave keeps its
// o-tile's A = W^T fragments in registers for the launch (9C/4 VGPRs) and
// walks its share of the band's 16-pixel tiles (band pixel 16 tile + lx; at
// W = 8 a tile spans two rows; C=16: the 4 waves deal the tiles round-robin;
// C=64: one o-tile per wave, every tile).  K-step s of channel group q at a tap gives lane (lx, g) the
// channel 16q + 4g + s, so one 16-B LDS read per lane (the pixel's channels
// 16q+4g .. +3) feeds four MFMAs.  The accumulator lane (lx, g) holds
// channels 4g .. 4g+3 of pixel lx: the residual / dy / dz operands and the
// output are 16-B accesses, and the relu-mask nibbles of a pixel's 16
// channels are merged across the 4 lane groups into one 16-bit store (every
// bit written: no memset, no atomics).
// Weight gradient (k_wgrad32): D[i][o] = sum_px x[px + tap][i] dz[px][o] per
// tap, K = 4 pixels per MFMA (one fp32 per lane from LDS for each operand).
// 12 waves: (tap row ky, o-tile, row split); each holds the 3 taps of its row
// x C/16 i-tiles of its o-tile in accumulators over a persistent run of
// bands, the row-split partials are summed through LDS at the end and the
// workgroup writes one [dW | db] slab (db on MFMA: ones x dz in the ky = 1
// waves), reduced by the same two-pass k_reduce_slabs / projection as the
// bf16 path.
// ===========================================================================
template <int C, int W_>
struct F32Band {
  // pixel strides in LDS (floats), padded against bank conflicts: PSC for the conv's 16-B reads
  // (16 lanes = 16 consecutive pixels on distinct banks), PSW for the wgrad's 4-B reads (the two
  // lane groups of a 32-lane half, one pixel apart, on disjoint banks); unpadded, a C = 64 tile
  // put the 16 lanes of a conv read on one bank group
  static constexpr int PSC = C + 4, PSW = C >= 32 ? C + 16 : C;
  static constexpr int OT = C / 16, W = W_, TW = W + 2, BR = 4, TILEF = (BR + 2) * TW * PSC;
  static constexpr int TILEW = (BR + 2) * TW * PSW;  // the wgrad's x tile
  static constexpr int T = BR * W / 16;  // 16-pixel tiles per band (band pixel p = 16 tile + lx: row p / W, col p % W)
  static constexpr int WPT = 4 / OT;    // forward / dgrad: waves sharing an o-tile, tiles dealt round-robin
  static constexpr int RS = 4 / OT;     // wgrad row split: 3 * OT * RS = 12 waves
  static constexpr int DZF = BR * W * PSW;
  static_assert(W == 8 || W == 16 || W == 32, "fp32 MFMA band: W in {8, 16, 32}");
};

// 4 consecutive floats (a 16-B load)
__device__ __forceinline__ f32x4 load4f(const float* p) { return *(const f32x4*)p; }

// dz = h dy [relu bit] of 4 channels (bit index pixel*C + c, C a multiple of 16: a nibble)
__device__ __forceinline__ f32x4 masked_dz4(f32x4 v, const uint8_t* __restrict__ dmask, long bit, float dh) {
  const unsigned nib = (unsigned)(dmask[bit >> 3] >> (bit & 7));
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = ((nib >> j) & 1u) ? dh * v[j] : 0.f;
  return v;
}

// stage rows y0-1 .. y0+BR of image n into tile (zeros outside the image and
// in the two halo columns), float4 per thread; with dmask, src is dy and the
// tile gets dz = dh * dy * [relu bit] (the Euler block's dz, no separate pass)
template <int C, int W, int PS = C, int NT = 256>
__device__ __forceinline__ void f32_stage_rows(const float* __restrict__ src, float* tile, int n, int y0, int H,
                                               int tid, const uint8_t* __restrict__ dmask = nullptr,
                                               float dh = 1.f) {
  using G = F32Band<C, W>;
  constexpr int C4 = C / 4, NCH = (G::BR + 2) * G::TW * C4, NIT = (NCH + NT - 1) / NT, B = 4;
  // B loads in flight before their stores (a rolled loop waited for each load in turn)
#pragma unroll
  for (int k0 = 0; k0 < NIT; k0 += B) {
    f32x4 v[B];
    long ev[B];
    unsigned mb[B];  // the relu byte of each element (with dmask), loaded beside its values
#pragma unroll
    for (int k = 0; k < B; ++k) {
      const int i = tid + (k0 + k) * NT;
      const int r = i / (G::TW * C4), rem = i % (G::TW * C4), col = rem / C4, c4 = rem % C4;
      const int gy = y0 - 1 + r, gx = col - 1;
      v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
      ev[k] = -1;
      mb[k] = 0u;
      if (k0 + k < NIT && i < NCH && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)G::W) {
        ev[k] = (((long)n * H + gy) * G::W + gx) * C + 4 * c4;
        v[k] = load4f(src + ev[k]);
        if (dmask) mb[k] = dmask[ev[k] >> 3];
      }
    }
#pragma unroll
    for (int k = 0; k < B; ++k) {
      const int i = tid + (k0 + k) * NT;
      if (k0 + k < NIT && i < NCH) {
        const int r = i / (G::TW * C4), rem = i % (G::TW * C4), col = rem / C4, c4 = rem % C4;
        if (dmask && ev[k] >= 0) {  // (masked_dz4 on the preloaded byte: dz = dh dy [relu bit])
          const unsigned nib = mb[k] >> (ev[k] & 7);
#pragma unroll
          for (int j = 0; j < 4; ++j) v[k][j] = ((nib >> j) & 1u) ? dh * v[k][j] : 0.f;
        }
        *(f32x4*)(tile + (r * G::TW + col) * PS + 4 * c4) = v[k];
      }
    }
  }
}

template <int C, int W, int MODE>
__global__ __launch_bounds__(256) void k_conv32(const float* __restrict__ xin, float* __restrict__ out,
                                                uint8_t* __restrict__ mask, const float* __restrict__ w,
                                                const float* __restrict__ bias, float h, float two_gamma,
                                                const float* __restrict__ dy, const float* __restrict__ extra, int N,
                                                int H, const uint8_t* __restrict__ dmask) {
  using G = F32Band<C, W>;
  constexpr int OT = G::OT, TW = G::TW, BR = G::BR;
  __shared__ __attribute__((aligned(16))) float tile[G::TILEF];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, lx = lane & 15;
  const int ot = wave % OT, rw = wave / OT;
  const int nb = (H + BR - 1) / BR;
  const int n = blockIdx.x / nb, y0 = (blockIdx.x % nb) * BR;
  if (n >= N) return;
  // A = W^T of o-tile ot (HWIO W): A[t][q][s] = W[t][16q + 4g + s][16 ot + lx]
  float A[9][OT][4];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int q = 0; q < OT; ++q)
#pragma unroll
      for (int s = 0; s < 4; ++s) A[t][q][s] = w[((long)t * C + 16 * q + 4 * g + s) * C + 16 * ot + lx];
  f32x4 bz = {0.f, 0.f, 0.f, 0.f};
  if (MODE <= F_RELU && bias) bz = *(const f32x4*)(bias + 16 * ot + 4 * g);
  // (backward with dmask: xin is dy, the tile gets dz = h dy [relu bit])
  f32_stage_rows<C, W, G::PSC, 256>(xin, tile, n, y0, H, tid, MODE >= B_EULER ? dmask : nullptr, h);
  __syncthreads();
  // wave (ot, rw) takes the band's 16-pixel tiles rw, rw + WPT, ..; lane lx's pixel of tile tau is band
  // pixel 16 tau + lx (W = 8: a tile spans two rows, so validity is per lane)
  constexpr int NT = (G::T + G::WPT - 1) / G::WPT;
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int tau = rw + j * G::WPT;
    if (tau >= G::T) break;  // (wave-uniform)
    const int bp = 16 * tau + lx, r = bp / W, px = bp % W;
    if (W >= 16 && y0 + r >= H) break;  // (wave-uniform for W >= 16; rows only grow with tau)
    f32x4 acc = bz;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int q = 0; q < OT; ++q) {
        const f32x4 bv = *(const f32x4*)(tile + ((r + t / 3) * TW + px + t % 3) * G::PSC + 16 * q + 4 * g);
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(A[t][q][s], bv[s], acc, 0, 0, 0);
      }
    mfma_f32_settle();  // (the epilogue branches: every path must see the result's wait states)
    {
      const bool ok = y0 + r < H;
      const long pix = ((long)n * H + y0 + r) * W + px;
      const long oi = pix * C + 16 * ot + 4 * g;  // this lane's 4 channels
      const f32x4 ctr = *(const f32x4*)(tile + ((r + 1) * TW + px + 1) * G::PSC + 16 * ot + 4 * g);  // x or dz at the pixel
      f32x4 v;
      if constexpr (MODE == F_EULER) {
        const f32x4 res = (extra && ok) ? *(const f32x4*)(extra + oi) : ctr;
        unsigned nib = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float z = acc[e];
          nib |= (z > 0.f ? 1u : 0u) << e;
          v[e] = res[e] + h * fmaxf(z, 0.f);
        }
        if (mask) {  // the pixel's 16 channels of this o-tile: 4 nibbles, one 16-bit store
          unsigned m = nib << (4 * g);
          m |= (unsigned)__shfl_xor((int)m, 16, 64);
          m |= (unsigned)__shfl_xor((int)m, 32, 64);
          if (g == 0 && ok) *(uint16_t*)(mask + (pix * C + 16 * ot) / 8) = (uint16_t)m;
        }
      } else if constexpr (MODE == F_CONV) {
        v = acc;
      } else {  // B_EULER / B_CONV: the tile holds dz; dx = [dy] - A dz + 2 gamma dz [+ extra]
        f32x4 d0 = {0.f, 0.f, 0.f, 0.f};
        if (ok) {
          if constexpr (MODE == B_EULER) d0 = *(const f32x4*)(dy + oi);
          if (extra) d0 += *(const f32x4*)(extra + oi);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = d0[e] - acc[e] + two_gamma * ctr[e];
      }
      if (ok) *(f32x4*)(out + oi) = v;
    }
  }
}

template <int C, int W>
__global__ __launch_bounds__(768) void k_wgrad32(const float* __restrict__ x, const float* __restrict__ dz, int N,
                                                 int H, float* __restrict__ slabs, const uint8_t* __restrict__ dmask,
                                                 float dh, long x_stride = 0, long dz_stride = 0, long m_stride = 0,
                                                 long s_stride = 0) {
  using G = F32Band<C, W>;
  // several layers in one launch: blockIdx.y is the layer
  x += blockIdx.y * x_stride;
  dz += blockIdx.y * dz_stride;
  if (dmask) dmask += blockIdx.y * m_stride;
  slabs += blockIdx.y * s_stride;
  constexpr int OT = G::OT, TW = G::TW, BR = G::BR, RS = G::RS, E = 9 * C * C;
  extern __shared__ __attribute__((aligned(16))) float lds32[];
  float* xt = lds32;               // [BR+2][TW][C]
  float* dzt = lds32 + G::TILEW;   // [BR][W][PSW]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, lx = lane & 15;
  const int ky = wave / (OT * RS), ot = (wave / RS) % OT, rs = wave % RS;
  const int nb = (H + BR - 1) / BR;
  const long items = (long)N * nb;
  const long i0 = (long)blockIdx.x * items / gridDim.x, i1 = (long)(blockIdx.x + 1) * items / gridDim.x;
  f32x4 acc[3][OT], accb = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kx = 0; kx < 3; ++kx)
#pragma unroll
    for (int it = 0; it < OT; ++it) acc[kx][it] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (long item = i0; item < i1; ++item) {
    const int n = (int)(item / nb), y0 = (int)(item % nb) * BR;
    const int rows = min(BR, H - y0);
    __syncthreads();  // the previous item's tiles consumed
    f32_stage_rows<C, W, G::PSW, 768>(x, xt, n, y0, H, tid);
    for (int i = tid; i < BR * G::W * C / 4; i += 768) {
      const int r = i / (G::W * C / 4);
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (r < rows) {
        const long e = ((long)n * H + y0) * G::W * C + 4 * i;
        v = load4f(dz + e);
        if (dmask) v = masked_dz4(v, dmask, e, dh);  // dz is dy here: dz = dh dy [relu bit]
      }
      *(f32x4*)(dzt + (i / (C / 4)) * G::PSW + 4 * (i % (C / 4))) = v;
    }
    __syncthreads();
    for (int r = rs; r < rows; r += RS) {
#pragma unroll
      for (int s = 0; s < G::W / 4; ++s) {
        const int p = 4 * s + g;  // this lane's pixel (k index) of the step
        const float bv = dzt[(r * G::W + p) * G::PSW + 16 * ot + lx];
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
#pragma unroll
          for (int it = 0; it < OT; ++it) {
            const float av = xt[((r + ky) * TW + p + kx) * G::PSW + 16 * it + lx];
            acc[kx][it] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[kx][it], 0, 0, 0);
          }
        if (ky == 1) accb = __builtin_amdgcn_mfma_f32_16x16x4f32(1.f, bv, accb, 0, 0, 0);
      }
    }
  }
  // sum the RS row-split partials through LDS (fixed order), one slab per workgroup
  constexpr int PW = (3 * OT + 1) * 256;  // floats per wave: its tiles, then db
  if constexpr (RS > 1) {
    __syncthreads();  // (the last item's tiles consumed)
    if (rs != 0) {
      float* mine = lds32 + wave * PW;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx)
#pragma unroll
        for (int it = 0; it < OT; ++it) *(f32x4*)(mine + ((kx * OT + it) * 64 + lane) * 4) = acc[kx][it];
      *(f32x4*)(mine + (3 * OT * 64 + lane) * 4) = accb;
    }
    __syncthreads();
    if (rs == 0) {
#pragma unroll
      for (int q = 1; q < RS; ++q) {
        const float* th = lds32 + (wave + q) * PW;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
#pragma unroll
          for (int it = 0; it < OT; ++it) acc[kx][it] += *(const f32x4*)(th + ((kx * OT + it) * 64 + lane) * 4);
        accb += *(const f32x4*)(th + (3 * OT * 64 + lane) * 4);
      }
    }
  }
  if (rs == 0) {
    float* slab = slabs + (long)blockIdx.x * (E + C);
#pragma unroll
    for (int kx = 0; kx < 3; ++kx)
#pragma unroll
      for (int it = 0; it < OT; ++it)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          slab[((long)(3 * ky + kx) * C + 16 * it + 4 * g + j) * C + 16 * ot + lx] = acc[kx][it][j];
    // db: the ky = 1 waves' ones x dz (every row of that product is the column sum)
    if (ky == 1 && g == 0) slab[E + 16 * ot + lx] = accb[0];
  }
}

template <int C, int W>
static size_t wgrad32_lds() {
  using G = F32Band<C, W>;
  const size_t stage = (size_t)(G::TILEW + G::DZF) * 4;
  const size_t red = G::RS > 1 ? (size_t)12 * (3 * G::OT + 1) * 256 * 4 : 0;
  return std::max(stage, red);
}

// the multi-stage nets' 16x16 and 8x8 stages (asr_stages.hip) run the same kernels at W = 16 / 8
static constexpr bool conv32_c_w(int C, int W) {  // (dispatch_c_w's predicate)
  return (W == 32 || W == 16 || W == 8) && (C == 16 || C == 32 || C == 64);
}
static bool conv32_supported(int W, int Ci, int Co) { return Ci == Co && conv32_c_w(Ci, W); }

template <int C, int W, int MODE>
static int launch_conv32(const void* xin, void* out, uint8_t* mask, const float* w, const float* bias, float h,
                         float two_gamma, const float* dy, const float* extra, int N, int H, hipStream_t s,
                         const uint8_t* dmask = nullptr) {
  const long blocks = (long)N * ((H + 3) / 4);
  if (blocks > 0x7fffffffL) return fail(ASR_E_ARG, "conv f32: problem too large");
  hipLaunchKernelGGL((k_conv32<C, W, MODE>), dim3((unsigned)blocks), dim3(256), 0, s, (const float*)xin,
                     (float*)out, mask, w, bias, h, two_gamma, dy, extra, N, H, dmask);
  ASR_LAUNCH_CHECK("k_conv32");
  return ASR_OK;
}

// (both callers test conv32_supported first: the dispatcher's own rejection is not reached)
template <int MODE>
static int conv32_dispatch(int C, int W, const void* xin, void* out, uint8_t* mask, const float* w, const float* bias,
                           float h, float two_gamma, const float* dy, const float* extra, int N, int H, hipStream_t s,
                           const uint8_t* dmask = nullptr) {
  return dispatch_c_w<conv32_c_w>("conv f32 (MFMA)", C, W, [&](auto c, auto sw) -> int {
    return launch_conv32<decltype(c)::value, decltype(sw)::value, MODE>(xin, out, mask, w, bias, h, two_gamma, dy,
                                                                        extra, N, H, s, dmask);
  });
}

// k_wgrad32's grid = its slab rows (one [dW | db] slab per workgroup)
template <int C, int W>
static int wgrad32_grid(int N, int H) {
  const long items = (long)N * ((H + 3) / 4);
  const int cus = launch_cus();
  const int per_cu = std::max(1, std::min(2, (int)((160 * 1024) / wgrad32_lds<C, W>())));
  // at least minb bands per workgroup at C = 32 / 64: a slab row is 37 / 148 KB, written and read back
  constexpr int minb = C == 64 ? 16 : C == 32 ? 8 : 1;  // (profiles/r05al_f32_wgrad_rows_ab.txt)
  return (int)std::max<long>(1, std::min<long>({(items + minb - 1) / minb, (long)per_cu * cus, (long)kMaxBlockSlabs}));
}

template <int C, int W>
static int launch_wgrad32(const float* x, const float* dz, int N, int H, float* slabs, int* nslabs, hipStream_t s,
                          const uint8_t* dmask = nullptr, float dh = 1.f, int layers = 1, long x_stride = 0,
                          long dz_stride = 0, long m_stride = 0, long s_stride = 0) {
  const size_t lds = wgrad32_lds<C, W>();
  const int grid = wgrad32_grid<C, W>(N, H);
  hipLaunchKernelGGL((k_wgrad32<C, W>), dim3(grid, layers), dim3(768), lds, s, x, dz, N, H, slabs, dmask, dh,
                     x_stride, dz_stride, m_stride, s_stride);
  ASR_LAUNCH_CHECK("k_wgrad32");
  *nslabs = grid;
  return ASR_OK;
}

template <typename Tout, int MODE>
static int launch_conv_f32(const void* xin, void* out, uint8_t* mask, const float* w, const float* bias, float h,
                           float two_gamma, const float* dy, const float* extra, int N, int H, int W, int Ci, int Co,
                           hipStream_t s, int K = 3) {
  const long tasks = (long)N * H * ((W + 15) / 16) * ((Co + 15) / 16);
  const long blocks = (tasks + 3) / 4;
  if (blocks > 0x7fffffffL) return fail(ASR_E_ARG, "conv f32: problem too large");
  if (MODE == F_EULER && mask) {
    ASR_TRY(zero_words(mask, ((long)N * H * W * Co + 31) / 32, s));  // (the kernel ORs its bits in)
  }
  hipLaunchKernelGGL((k_conv_f32<Tout, MODE>), dim3((unsigned)blocks), dim3(256), 0, s, (const float*)xin,
                     (Tout*)out, (uint32_t*)mask, w, bias, h, two_gamma, dy, extra, N, H, W, Ci, Co, K);
  ASR_LAUNCH_CHECK("k_conv_f32");
  return ASR_OK;
}

int conv_f32(int fmode, const void* xin, void* out, uint8_t* mask, const float* w, const float* bias, float h,
             float two_gamma, const float* dy, int N, int H, int W, int Ci, int Co, int out_bf16, hipStream_t s,
             const float* extra, int K) {
  if (K == 3 && conv32_supported(W, Ci, Co) && fmode != F_RELU) {  // the network's blocks: fp32 MFMA
    switch (fmode) {
      case F_EULER: return conv32_dispatch<F_EULER>(Ci, W, xin, out, mask, w, bias, h, two_gamma, dy, extra, N, H, s);
      case F_CONV: return conv32_dispatch<F_CONV>(Ci, W, xin, out, mask, w, bias, h, two_gamma, dy, extra, N, H, s);
      case B_EULER: return conv32_dispatch<B_EULER>(Ci, W, xin, out, mask, w, bias, h, two_gamma, dy, extra, N, H, s);
      case B_CONV: return conv32_dispatch<B_CONV>(Ci, W, xin, out, mask, w, bias, h, two_gamma, dy, extra, N, H, s);
    }
  }
  switch (fmode) {
    case F_EULER:
      return launch_conv_f32<float, F_EULER>(xin, out, mask, w, bias, h, two_gamma, dy, extra, N, H, W, Ci, Co, s, K);
    case F_CONV:
      return launch_conv_f32<float, F_CONV>(xin, out, mask, w, bias, h, two_gamma, dy, extra, N, H, W, Ci, Co, s, K);
    case F_RELU:
      if (out_bf16)
        return launch_conv_f32<bf16, F_RELU>(xin, out, mask, w, bias, h, two_gamma, dy, extra, N, H, W, Ci, Co, s, K);
      return launch_conv_f32<float, F_RELU>(xin, out, mask, w, bias, h, two_gamma, dy, extra, N, H, W, Ci, Co, s, K);
    case B_EULER:
      return launch_conv_f32<float, B_EULER>(xin, out, mask, w, bias, h, two_gamma, dy, extra, N, H, W, Ci, Co, s, K);
    case B_CONV:
      return launch_conv_f32<float, B_CONV>(xin, out, mask, w, bias, h, two_gamma, dy, extra, N, H, W, Ci, Co, s, K);
  }
  return fail(ASR_E_ARG, "conv f32: bad mode");
}

// K x K (odd K != 3: Conv2DAntisymmetric(kernel_size), …Conv2DAntisymmetric.py:60-68, 109-145) on the
// fp32 VALU kernel, same modes as conv_f32
int conv_f32_k(int fmode, int K, const void* xin, void* out, uint8_t* mask, const float* w, const float* bias, float h,
               float two_gamma, const float* dy, int N, int H, int W, int C, hipStream_t s, const float* extra) {
  if (K == 3) return conv_f32(fmode, xin, out, mask, w, bias, h, two_gamma, dy, N, H, W, C, C, 0, s, extra);
  switch (fmode) {
    case F_EULER:
      return launch_conv_f32<float, F_EULER>(xin, out, mask, w, bias, h, two_gamma, dy, extra, N, H, W, C, C, s, K);
    case F_CONV:
      return launch_conv_f32<float, F_CONV>(xin, out, mask, w, bias, h, two_gamma, dy, extra, N, H, W, C, C, s, K);
    case B_EULER:
      return launch_conv_f32<float, B_EULER>(xin, out, mask, w, bias, h, two_gamma, dy, extra, N, H, W, C, C, s, K);
    case B_CONV:
      return launch_conv_f32<float, B_CONV>(xin, out, mask, w, bias, h, two_gamma, dy, extra, N, H, W, C, C, s, K);
  }
  return fail(ASR_E_ARG, "conv f32 (k=%d): bad mode", K);
}

int make_dz(int fmode, const void* dy, const uint8_t* mask, const void* relu_src, float h, int N, int H, int W, int C,
            int src_bf16, float* dz, hipStream_t s) {
  const long P = (long)N * H * W * C;
  const unsigned grid = (unsigned)std::min<long>((P + 255) / 256, 8192);
  if (src_bf16)
    hipLaunchKernelGGL(k_make_dz<bf16>, dim3(grid), dim3(256), 0, s, (const bf16*)dy, mask, (const bf16*)relu_src,
                       fmode, h, N, H, W, C, dz);
  else
    hipLaunchKernelGGL(k_make_dz<float>, dim3(grid), dim3(256), 0, s, (const float*)dy, mask,
                       (const float*)relu_src, fmode, h, N, H, W, C, dz);
  ASR_LAUNCH_CHECK("k_make_dz");
  return ASR_OK;
}

// The fp32 Euler block's backward on the matrix cores without the dz pass:
// dgrad (B_EULER, or B_CONV when skip_dy: the second RK2 stage) and the weight
// gradient stage dz = h dy [relu bit] straight from dy and the mask.  Only for
// conv32_supported shapes (else ASR_E_UNSUPPORTED: the caller runs make_dz +
// conv_f32 + wgrad_f32).
bool conv32_fused_bwd_supported(int W, int C) { return conv32_supported(W, C, C); }

int conv32_bwd_fused(const float* dy, const uint8_t* mask, float h, const float* x, const float* w, float two_gamma,
                     const float* extra, bool skip_dy, int N, int H, int W, int C, float* dx, bool need_w,
                     float* slabs, int* nslabs, hipStream_t s) {
  if (!conv32_supported(W, C, C)) return fail(ASR_E_UNSUPPORTED, "conv f32 fused backward: C=%d W=%d", C, W);
  *nslabs = 0;
  if (dx) {
    if (skip_dy)
      ASR_TRY(conv32_dispatch<B_CONV>(C, W, dy, dx, nullptr, w, nullptr, h, two_gamma, nullptr, extra, N, H, s, mask));
    else
      ASR_TRY(conv32_dispatch<B_EULER>(C, W, dy, dx, nullptr, w, nullptr, h, two_gamma, dy, extra, N, H, s, mask));
  }
  if (!need_w) return ASR_OK;
  return dispatch_c_w<conv32_c_w>("conv f32 fused backward", C, W, [&](auto c, auto sw) -> int {
    return launch_wgrad32<decltype(c)::value, decltype(sw)::value>(x, dy, N, H, slabs, nslabs, s, mask, h);
  });
}

// number of row chunks used by the fp32 wgrad (bounded by kMaxBlockSlabs in the
// workspace sizing of the callers)
int wgrad_f32_chunks(int N, int H) {
  const long R = (long)N * H;
  long chunks = std::min<long>(R, 256);
  return (int)std::max<long>(chunks, 1);
}

// Slab rows one fp32 3x3 C -> C block application's weight gradient writes
// (conv32_bwd_fused / wgrad_f32): the workspace of the fp32 networks keeps
// every block's slabs, so it is sized by this, not by the 512-row maximum.
// On the device the workspace was sized for (the MFMA grid follows its CU count).
int f32_block_slab_rows(int N, int H, int W, int C) {
  if (!conv32_supported(W, C, C)) return wgrad_f32_chunks(N, H);
  return dispatch_c_w<conv32_c_w>("fp32 block slab rows", C, W, [&](auto c, auto sw) -> int {
    return wgrad32_grid<decltype(c)::value, decltype(sw)::value>(N, H);
  });
}

int wgrad_f32(const void* x, int x_bf16, const float* dz, int N, int H, int W, int Ci, int Co, float* slabs,
              int* nslabs, hipStream_t s, int K) {
  if (!x_bf16 && K == 3 && conv32_supported(W, Ci, Co))  // the network's blocks: fp32 MFMA, db included
    return dispatch_c_w<conv32_c_w>("wgrad f32 (MFMA)", Ci, W, [&](auto c, auto sw) -> int {
      return launch_wgrad32<decltype(c)::value, decltype(sw)::value>((const float*)x, dz, N, H, slabs, nslabs, s);
    });
  const long R = (long)N * H;
  const int chunks = wgrad_f32_chunks(N, H);
  const int rpc = (int)((R + chunks - 1) / chunks);
  const int nch = (int)((R + rpc - 1) / rpc);
  const long E = (long)K * K * Ci * Co;
  dim3 grid((unsigned)((E + 255) / 256), nch);
  if (x_bf16)
    hipLaunchKernelGGL(k_wgrad_f32<bf16>, grid, dim3(256), 0, s, (const bf16*)x, dz, N, H, W, Ci, Co, rpc, slabs, K);
  else
    hipLaunchKernelGGL(k_wgrad_f32<float>, grid, dim3(256), 0, s, (const float*)x, dz, N, H, W, Ci, Co, rpc, slabs, K);
  ASR_LAUNCH_CHECK("k_wgrad_f32");
  if (Co > 1024) return fail(ASR_E_UNSUPPORTED, "db: C > 1024");
  hipLaunchKernelGGL(k_db_f32, dim3(nch), dim3(((Co + 63) / 64) * 64), 0, s, dz, R, W, Co, rpc, E, slabs);
  ASR_LAUNCH_CHECK("k_db_f32");
  *nslabs = nch;
  return ASR_OK;
}

// The fp32 weight-gradient slabs of L layers in one launch (k_wgrad32, blockIdx.y = layer, dz = h dy [relu bit]):
// wgrad_layers' fp32 half (asr_stage_img.hip).  Its shapes are the stages of the fp32 nets that run it, fewer
// than conv32_supported's: the other four pairs stay rejected, as before the dispatcher.
static constexpr bool wgrad32_layers_c_w(int C, int W) {
  return (C == 32 && W == 16) || (C == 64 && W == 8) || (C == 16 && W == 32) || (C == 32 && W == 32) ||
         (C == 64 && W == 16);
}
int wgrad32_layers(const float* x0, long x_stride, const float* dys, long d_stride, const uint8_t* masks,
                   long mask_stride, float h, int N, int H, int W, int C, int L, float* slabs, long slab_stride,
                   int* nslabs, hipStream_t s) {
  return dispatch_c_w<wgrad32_layers_c_w>("fp32 weight gradient (layers)", C, W, [&](auto c, auto sw) -> int {
    return launch_wgrad32<decltype(c)::value, decltype(sw)::value>(x0, dys, N, H, slabs, nslabs, s, masks, h, L,
                                                                   x_stride, d_stride, mask_stride, slab_stride);
  });
}

// elementwise bf16 <-> fp32 (the multi-stage bf16 net's transitions run in fp32)
__global__ void k_bf16_to_f32(const bf16* __restrict__ a, float* __restrict__ b, long n8) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    const uint4 u = ((const uint4*)a)[i];
    const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int k = 0; k < 4; ++k)
      ((float2*)b)[4 * i + k] = make_float2(__uint_as_float(w[k] << 16), __uint_as_float(w[k] & 0xffff0000u));
  }
}
__global__ void k_f32_to_bf16(const float* __restrict__ a, bf16* __restrict__ b, long n8) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    const float4 p = ((const float4*)a)[2 * i], q = ((const float4*)a)[2 * i + 1];
    ((uint4*)b)[i] = make_uint4(pk_bf16_rn(p.x, p.y), pk_bf16_rn(p.z, p.w), pk_bf16_rn(q.x, q.y), pk_bf16_rn(q.z, q.w));
  }
}
int convert_bf16_f32(const void* src, void* dst, long n, int to_f32, hipStream_t s) {
  if (n % 8) return fail(ASR_E_ARG, "bf16 <-> fp32: element count %ld not a multiple of 8", n);
  const long n8 = n / 8;
  const unsigned grid = (unsigned)std::max<long>(1, std::min<long>((n8 + 255) / 256, 8192));
  if (to_f32)
    hipLaunchKernelGGL(k_bf16_to_f32, dim3(grid), dim3(256), 0, s, (const bf16*)src, (float*)dst, n8);
  else
    hipLaunchKernelGGL(k_f32_to_bf16, dim3(grid), dim3(256), 0, s, (const float*)src, (bf16*)dst, n8);
  ASR_LAUNCH_CHECK("k_bf16_f32");
  return ASR_OK;
}

}  // namespace asr
