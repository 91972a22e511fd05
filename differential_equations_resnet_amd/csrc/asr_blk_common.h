// What the bf16 MFMA block kernels of asr_block_mfma.hip's translation unit
// share: measured settings, the diagnostic stamp / trace macros and buffers,
// geometry (Geo, Band), LDS-DMA staging (toff, dma_*, zero_halo_cols), the conv
// on a row (conv_row) and on a band (conv_band*), load_A*, item_range, ItemCursor.
//
// Reference operator: Conv2DAntisymmetric3By3.call (tf.nn.conv2d SAME NHWC +
// bias, layers/tfkeras_layer_Conv2DAntisymmetric3By3.py:157-171) inside
// single_layer_identity_block (relu, h*, +input: models/tfkeras_resnets.py:69-92)
// and its autodiff (training/training.py:300).
//
// Work item = one band of BR output rows of one image.  A persistent
// workgroup walks a contiguous run of items (consecutive bands of the same
// images, so halo rows are L2 hits).  The input rows of item i+1 are copied
// HBM -> LDS by global_load_lds (no VGPR staging) while item i is computed;
// the XOR swizzle of the LDS image is applied on the per-lane SOURCE address
// (the DMA writes 1 KiB lane-linear), halo columns are zeroed once, rows
// outside the image come from a zero page.
//
// Math (implicit GEMM on v_mfma_f32_16x16x32_bf16, kappa = tap*C + i):
//   forward  Z^T[o][p]  = sum_kappa W^T[o][kappa] X[p][kappa]      (A = W^T in VGPRs)
//   dgrad    (A dz)     : the same GEMM on dz = h*dy*mask, because
//                         A^T = -A + 2*gamma*I for the assembled W:
//                         dx = dy - A dz + 2*gamma*dz
//   wgrad    dW[kappa][o] = sum_p X[p + s(tap)][i] dz[p][o]          (K = pixels;
//                         both operands read with ds_read_b64_tr_b16)
#pragma once
#include <type_traits>

#include "asr_common.h"
#include "asr_device.h"

// Measured settings (each an A/B of whole steps in the commit log; the other arms were removed in
// round 6 and stay in git history).  The v1 backward (C = 16 / 32, RK2 stages): 75 % of its prefetch
// DMAs issued by the dgrad waves, inside their k-steps.  The v2/v3 backward's convert: relu-mask
// expansion from a 4 KiB LDS table.  The forward pipe: y as 16-B stores; halo rows of a band that
// continues the previous band's image copied in LDS.
constexpr int kBwdDgradDmaPct = 75;
constexpr int kFwd3Wgs = 3;  // k_fwd3 workgroups per CU (grid = min(bands, 3 x CUs))
// k_bwd3 wgrad waves: DMA pieces issued right after the barrier, the rest one per row (A/B: spreading them
// lengthened the MFMA phase as much as it saved; the stacks: all at once 16 vs 9 +0.3-0.5 %, 4 -0.7 %)
constexpr int kBwd3Dma0 = 16;

namespace asr {

namespace blk {

// Diagnostic build only (-DASR_STAMP_BUILD=1, cdna_hip_programming.md §7
// in-kernel stamps): s_memtime at phase boundaries of the fused backward,
// lane 0 of waves 0 (dgrad) and 4 (wgrad), into a buffer nothing else reads.
#ifndef ASR_STAMP_BUILD
#define ASR_STAMP_BUILD 0
#endif
#if ASR_STAMP_BUILD
constexpr int kStampBands = 16, kStampSlots = 8;
__device__ unsigned long long g_stamps[512][2][kStampBands][kStampSlots];
#define ASR_STAMP(band, slot)                                                                      \
  do {                                                                                             \
    if ((wave == 0 || wave == 4) && (band) < kStampBands) {                                        \
      unsigned long long _t;                                                                       \
      __builtin_amdgcn_sched_barrier(0);                                                           \
      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(_t)::"memory");                   \
      __builtin_amdgcn_sched_barrier(0);                                                           \
      if (lane == 0) g_stamps[blockIdx.x][wave >> 2][(band)][(slot)] = _t;                         \
    }                                                                                              \
  } while (0)
#else
#define ASR_STAMP(band, slot) \
  do {                        \
  } while (0)
#endif

enum { FWD_EULER = 0, FWD_CONV = 1, BWD_EULER = 2, BWD_CONV = 3 };

// Diagnostic build only (-DASR_BLK_TRACE=1): s_memtime stamps per band of
// workgroup 0 in k_fwd3 (kernel 0, wave 0) and k_bwd3 (kernel 1, role 0 =
// dgrad wave 0, role 1 = wgrad wave 4), and the clock probe pair (s_memtime,
// s_memrealtime) at the start and end of wave 0 in every workgroup; into
// buffers nothing else reads (asr_debug_blk_trace).
#ifndef ASR_BLK_TRACE
#define ASR_BLK_TRACE 0
#endif
#if ASR_BLK_TRACE
constexpr int kTrBands = 40, kTrSlots = 8;
__device__ unsigned long long g_btrace[2][2][kTrBands][kTrSlots];
__device__ unsigned long long g_bclock[2][1024][4];
// every workgroup at every block switch of k_bwd3_stack (the first band of block l), [wg][l][slot]:
// 0 wgrad wave 4 before the done[] poll, 1 after the poll and fence, 2 after its band barrier,
// 3 dgrad wave 0 before its band barrier, 4 after it (s_memtime: durations inside a workgroup);
// 5 / 6 s_memrealtime at slots 0 / 2 (100 MHz, one time base for every workgroup)
constexpr int kSwBlocks = 128, kSwSlots = 7;
__device__ unsigned long long g_bswitch[256][kSwBlocks][kSwSlots];
__device__ __forceinline__ void tr_store(unsigned long long* p, unsigned long long t) {
  unsigned lo = (unsigned)t, hi = (unsigned)(t >> 32);
  asm volatile("v_mov_b32 %0, %0\n\tv_mov_b32 %1, %1" : "+v"(lo), "+v"(hi));  // vector store
  *p = ((unsigned long long)hi << 32) | lo;
}
#define ASR_BTR(kern, role, band, slot)                                                         \
  do {                                                                                          \
    if (blockIdx.x == 0 && (threadIdx.x & 63) == 0 && (band) < kTrBands)                        \
      tr_store(&g_btrace[kern][role][band][slot], __builtin_amdgcn_s_memtime());                \
  } while (0)
#define ASR_BSW(l, slot, rt)                                                                   \
  do {                                                                                         \
    if ((threadIdx.x & 63) == 0 && blockIdx.x < 256 && (l) < kSwBlocks)                       \
      tr_store(&g_bswitch[blockIdx.x][l][slot],                                                \
               (rt) ? __builtin_amdgcn_s_memrealtime() : __builtin_amdgcn_s_memtime());       \
  } while (0)
#define ASR_BCLK(kern, which)                                                                    \
  do {                                                                                           \
    if (threadIdx.x == 0 && blockIdx.x < 1024) {                                                 \
      tr_store(&g_bclock[kern][blockIdx.x][2 * (which)], __builtin_amdgcn_s_memtime());          \
      tr_store(&g_bclock[kern][blockIdx.x][2 * (which) + 1], __builtin_amdgcn_s_memrealtime());  \
    }                                                                                            \
  } while (0)
#else
#define ASR_BSW(l, slot, rt) \
  do {                       \
  } while (0)
#define ASR_BTR(kern, role, band, slot) \
  do {                                  \
  } while (0)
#define ASR_BCLK(kern, which) \
  do {                        \
  } while (0)
#endif

template <int C>
struct Geo {
  static constexpr int NQ = C / 8;              // 16-byte chunks per pixel
  static constexpr int OT = C / 16;             // 16-channel tiles
  static constexpr int KS = (9 * C + 31) / 32;  // 32-deep k-steps of the conv GEMM
  static constexpr int OSPLIT = (C == 64) ? 2 : 1;
  static constexpr int OTW = OT / OSPLIT;       // o-tiles per conv wave
  static constexpr int MT = 9 * C / 16;         // wgrad m-tiles
  static constexpr int MTW = 9;                 // wgrad m-tiles per wave
  static constexpr int TG = MT / MTW;           // wgrad tile groups
  static constexpr int KSPLIT = 4 / TG;         // wgrad waves sharing a tile group
  static constexpr int PPI = 512 / C;           // pixels per 1 KiB DMA instruction
  __device__ __forceinline__ static int swz(int col) {
    if constexpr (C == 64) return col & 7;
    else if constexpr (C == 32) return (col >> 1) & 3;
    else return 0;
  }
};

template <int C>
__device__ __forceinline__ int toff(int row, int col, int q, int TW) {
  return ((row * TW + col) * Geo<C>::NQ + (q ^ Geo<C>::swz(col))) * 16;
}

// DMA image rows [gy0, gy0+nrows) of image n (rows outside [0,H) -> zeros) into
// tile rows [0, nrows), interior columns 1..W.  One instruction = PPI pixels.
// The lane's source offset inside a PPI-pixel segment does not depend on the
// segment (swz(col) only sees col mod 8 / mod 16, and PPI is a multiple of
// that), so per instruction only a wave-uniform base changes.
template <int C, int W>
__device__ __forceinline__ int dma_lane_off(int lane) {
  using G = Geo<C>;
  const int pl = lane / G::NQ, p = lane % G::NQ;
  return pl * C + (p ^ G::swz(1 + pl)) * 8;  // elements
}

// The loops below run on a wave-uniform index (readfirstlane), so they are
// scalar loops: per instruction only an SGPR base (row start or the zero
// page) and M0 change; the per-lane part is one 32-bit offset.
//
// One instruction j of a row stream: image rows [gy0, gy0+nrows) of image n
// (rows outside [0,H) -> zeros) into tile rows [0, nrows), interior columns.
template <int C, int W>
__device__ __forceinline__ void dma_row_instr(const bf16* __restrict__ src, unsigned char* tile, int n, int gy0, int j,
                                              int H, unsigned loff) {
  using G = Geo<C>;
  constexpr int TW = W + 2, NQ = G::NQ, PPI = G::PPI, IPR = W / PPI;
  const int r = (unsigned)j / IPR, seg = (unsigned)j % IPR;  // wave-uniform
  const int gy = gy0 + r;
  const unsigned char* base = ((unsigned)gy < (unsigned)H)
                                  ? (const unsigned char*)src + ((long)n * H + gy) * (W * C * 2) + seg * (PPI * C * 2)
                                  : (const unsigned char*)g_zero_page;
  dma16(base + loff, tile + ((r * TW + 1 + seg * PPI) * NQ) * 16);
}

// dma_row_instr to a tile at an LDS byte address (no generic -> LDS pointer cast: its
// null check trips a ROCm 7.2 codegen bug in the register-tight stacked backward)
template <int C, int W>
__device__ __forceinline__ void dma_row_instr_at(const bf16* __restrict__ src, unsigned tile, int n, int gy0, int j,
                                                 int H, unsigned loff) {
  using G = Geo<C>;
  constexpr int TW = W + 2, NQ = G::NQ, PPI = G::PPI, IPR = W / PPI;
  const int r = (unsigned)j / IPR, seg = (unsigned)j % IPR;  // wave-uniform
  const int gy = gy0 + r;
  const unsigned char* base = ((unsigned)gy < (unsigned)H)
                                  ? (const unsigned char*)src + ((long)n * H + gy) * (W * C * 2) + seg * (PPI * C * 2)
                                  : (const unsigned char*)g_zero_page;
  dma16_at(base + loff, tile + (unsigned)((r * TW + 1 + seg * PPI) * NQ) * 16u);
}

// Image row gy (zeros outside [0, H)) into a tile row: its W / PPI = 4 pieces in
// one dma16x4_at (the lane's swizzled source offset is the same for every
// piece: the swizzle is segment-invariant).  tile_row = the tile row's LDS byte address.
template <int C, int W>
__device__ __forceinline__ void dma_row_whole_at(const bf16* __restrict__ src, unsigned tile_row, int n, int gy, int H,
                                                 unsigned loff) {
  using G = Geo<C>;
  constexpr int NQ = G::NQ, PPI = G::PPI;
  static_assert(W / PPI == 4 && PPI * C * 2 == 1024 && PPI * NQ * 16 == 1024, "whole-row DMA: four 1 KiB pieces");
  const unsigned char* base = ((unsigned)gy < (unsigned)H)
                                  ? (const unsigned char*)src + ((long)n * H + gy) * (W * C * 2)
                                  : (const unsigned char*)g_zero_page;
  dma16x4_at(base + loff, tile_row + (unsigned)(NQ * 16));
}

template <int C, int W>
__device__ __forceinline__ void dma_rows(const bf16* __restrict__ src, unsigned char* tile, int n, int gy0,
                                         int nrows, int H, int wave, int nwaves, int lane) {
  using G = Geo<C>;
  constexpr int PPI = G::PPI, IPR = W / PPI;
  static_assert(W % PPI == 0, "image width must be a multiple of the DMA pixel group");
  static_assert(PPI % 16 == 0 || (PPI % 8 == 0 && C == 64), "segment-invariant swizzle");
  const unsigned loff = (unsigned)dma_lane_off<C, W>(lane) * 2u;  // bytes, < 1 KiB
  for (int j = __builtin_amdgcn_readfirstlane(wave); j < nrows * IPR; j += nwaves)
    dma_row_instr<C, W>(src, tile, n, gy0, j, H, loff);
}

// One 1 KiB chunk j of the relu-mask bytes of rows [gy0, gy0+nrows) (W*C/8
// bytes per row) into a lane-linear LDS array (bytes outside the image ->
// zeros).  The band's rows are contiguous in memory; only chunks that reach
// outside the image take the per-lane select.
template <int C, int W>
__device__ __forceinline__ void dma_mask_instr(const uint8_t* __restrict__ mask, unsigned char* mt, int n, int gy0,
                                               int nrows, int j, int H, int lane) {
  constexpr int RB = W * C / 8;  // bytes per image row
  const int total = nrows * RB;
  const long band0 = ((long)n * H + gy0) * RB;
  const int lo = max(0, -gy0) * RB, hi = (min(H, gy0 + nrows) - gy0) * RB;  // valid bytes of the band
  const int b0 = j * 1024, b = b0 + lane * 16;
  const void* s;
  if (b0 >= lo && b0 + 1024 <= hi && b0 + 1024 <= total)  // whole chunk valid (uniform)
    s = (const void*)(mask + band0 + b);
  else
    s = (b >= lo && b < hi && b < total) ? (const void*)(mask + band0 + b) : (const void*)(g_zero_page + lane);
  dma16(s, mt + b0);
}

template <int C, int W>
__device__ __forceinline__ void dma_mask_rows(const uint8_t* __restrict__ mask, unsigned char* mt, int n, int gy0,
                                              int nrows, int H, int wave, int nwaves, int lane) {
  const int total = nrows * (W * C / 8);
  for (int j = __builtin_amdgcn_readfirstlane(wave); j * 1024 < total; j += nwaves)
    dma_mask_instr<C, W>(mask, mt, n, gy0, nrows, j, H, lane);
}

// zero the halo columns (0 and W+1) of a tile with `rows` rows
template <int C, int W>
__device__ __forceinline__ void zero_halo_cols(unsigned char* tile, int rows, int tid, int nthreads) {
  constexpr int TW = W + 2, NQ = Geo<C>::NQ;
  for (int i = tid; i < rows * 2 * NQ; i += nthreads) {
    const int q = i % NQ, side = (i / NQ) & 1, r = i / (2 * NQ);
    *(uint4*)(tile + toff<C>(r, side ? W + 1 : 0, q, TW)) = make_uint4(0, 0, 0, 0);
  }
}

// Per-lane LDS offsets of the conv GEMM's B fragments.  k-step ks covers
// kappa = 32*ks + 8*g + j (g = lane>>4): for C >= 32 that is tap 32*ks/C and
// chunk qb + g (qb = (32*ks % C)/8), so only the 3 column shifts x the C/32
// chunk bases are lane-dependent (3 or 6 VGPRs); the tap row and the pixel
// tile become ds_read immediates.  For C = 16 the tap itself depends on g,
// so all KS offsets are lane values.
template <int C, int W>
struct Frag {
  static constexpr int TW = W + 2, NQ = C / 8, KS = Geo<C>::KS;
  static constexpr int NB = (C >= 32) ? 3 * (C / 32) : KS;
  int o[NB];
  __device__ __forceinline__ void init(int g, int lx) {
    if constexpr (C >= 32) {
#pragma unroll
      for (int kx = 0; kx < 3; ++kx)
#pragma unroll
        for (int cb = 0; cb < C / 32; ++cb) o[kx * (C / 32) + cb] = toff<C>(0, lx + kx, 4 * cb + g, TW);
    } else {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        int tap = (32 * ks + 8 * g) / C;
        if (tap > 8) tap = 8;  // C=16 tail k-step: A is zero there
        o[ks] = toff<C>(tap / 3, lx + tap % 3, (32 * ks + 8 * g) % C / 8, TW);
      }
    }
  }
  template <int ks>
  static constexpr int slot() {
    if constexpr (C >= 32) return ((32 * ks / C) % 3) * (C / 32) + (32 * ks % C) / 32;
    else return ks;
  }
  template <int ks, int pt>
  static constexpr int imm() {
    if constexpr (C >= 32) return ((32 * ks / C) / 3) * TW * NQ * 16 + pt * 16 * NQ * 16;
    else return pt * 16 * NQ * 16;
  }
};

template <int C, int W, int ks>
__device__ __forceinline__ void conv_issue(const unsigned (&ra)[Frag<C, W>::NB], bf16x8 (&B)[W / 16]) {
  if constexpr (W / 16 >= 1) B[0] = ds_read128<Frag<C, W>::template imm<ks, 0>()>(ra[Frag<C, W>::template slot<ks>()]);
  if constexpr (W / 16 >= 2) B[1] = ds_read128<Frag<C, W>::template imm<ks, 1>()>(ra[Frag<C, W>::template slot<ks>()]);
  static_assert(W / 16 <= 2, "conv_issue handles up to two pixel tiles");
}

// one k-step of the software pipeline: B of step ks lives in buffer ks%3;
// the reads of step ks+1 are in flight, those of ks+2 are issued after the
// MFMAs of ks (three buffers: a read never targets registers an MFMA issued
// in the previous step may still be reading).
template <int C, int W, int ks, typename Hook>
__device__ __forceinline__ void conv_step(const unsigned (&ra)[Frag<C, W>::NB],
                                          const bf16x8 (&A)[Geo<C>::OTW][Geo<C>::KS],
                                          f32x4 (&acc)[Geo<C>::OTW][W / 16], bf16x8 (&B)[3][W / 16], Hook& hook) {
  using G = Geo<C>;
  constexpr int PT = W / 16, KS = G::KS;
  if constexpr (ks < KS) {
    lgkm_wait<(ks + 1 < KS) ? PT : 0>();
#pragma unroll
    for (int pt = 0; pt < PT; ++pt)
#pragma unroll
      for (int t = 0; t < G::OTW; ++t)
        acc[t][pt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[t][ks], B[ks % 3][pt], acc[t][pt], 0, 0, 0);
    if constexpr (ks + 2 < KS) conv_issue<C, W, ks + 2>(ra, B[(ks + 2) % 3]);
    hook();
    conv_step<C, W, ks + 1>(ra, A, acc, B, hook);
  }
}

// conv GEMM of one output row (tile row r is the row above it), accumulated
// onto the caller's initial acc (the bias in the forward)
struct NoStepHook {
  __device__ __forceinline__ void operator()() const {}
};

// hook() runs once per k-step, after that step's MFMAs are issued (the
// backward interleaves its next-band DMA issue with the dgrad MFMAs that way)
template <int C, int W, typename Hook = NoStepHook>
__device__ __forceinline__ void conv_row(const unsigned char* tile, int r, const bf16x8 (&A)[Geo<C>::OTW][Geo<C>::KS],
                                         const Frag<C, W>& f, f32x4 (&acc)[Geo<C>::OTW][W / 16], Hook hook = {}) {
  using G = Geo<C>;
  constexpr int TW = W + 2, PT = W / 16;
  const unsigned rb = lds_u32(tile + r * TW * G::NQ * 16);
  unsigned ra[Frag<C, W>::NB];
#pragma unroll
  for (int k = 0; k < Frag<C, W>::NB; ++k) ra[k] = rb + (unsigned)f.o[k];
  bf16x8 B[3][PT];
  lgkm_wait<0>();  // nothing else of ours outstanding on the LDS counter
  conv_issue<C, W, 0>(ra, B[0]);
  if constexpr (G::KS > 1) conv_issue<C, W, 1>(ra, B[1]);
  conv_step<C, W, 0>(ra, A, acc, B, hook);
}

// ---------------------------------------------------------------------------
// Band conv (C >= 32): one wave = one 16-channel output tile over RB output
// rows.  The B fragment of input row ir (tap column kx, channel block cb)
// serves the MFMAs of every (output row r, tap row ky) with r + ky = ir, so
// RB+2 fragment reads feed 3*RB MFMAs per pixel tile (0.5 reads per MFMA
// at one o-tile per wave, the W fragments of that tile, 4*KS VGPRs, stay
// resident).  Fully unrolled, LDS reads software-pipelined two stages ahead.
// ---------------------------------------------------------------------------
template <int C, int W, int RB>
struct Band {
  static constexpr int TW = W + 2, NQ = C / 8, PT = W / 16, NCB = C / 32, KS = Geo<C>::KS;
  static constexpr int NR = RB + 2;             // input rows per band
  static constexpr int NS = 3 * NCB * NR;       // pipeline stages (kx, cb, input row)
  static constexpr int ROWB = TW * NQ * 16;     // LDS bytes per tile row
  static constexpr int PTB = 16 * NQ * 16;      // LDS bytes per 16-pixel tile
  static_assert(C % 32 == 0, "band conv needs whole 32-channel k-steps per tap");
  static_assert(NR * ROWB < 65536, "ds_read immediate offset range");
};

// input rows 0, 1 (the halo rows shared with the previous band) at baseh, rows 2.. at base
// (the same tile when baseh == base)
template <int C, int W, int RB, int S>
__device__ __forceinline__ void band_issue(unsigned base, unsigned baseh, const unsigned (&lo)[3 * Band<C, W, RB>::NCB],
                                           bf16x8 (&B)[Band<C, W, RB>::PT]) {
  using BD = Band<C, W, RB>;
  constexpr int blk = S / BD::NR, ir = S % BD::NR;
  const unsigned b = (ir < 2 ? baseh : base) + lo[blk];
  B[0] = ds_read128<ir * BD::ROWB>(b);
  if constexpr (BD::PT >= 2) B[1] = ds_read128<ir * BD::ROWB + BD::PTB>(b);
  static_assert(BD::PT <= 2, "band conv handles up to two pixel tiles");
}

// MFMAs of output row ir - KY (if inside the band) with tap (KY, kx)
template <int C, int W, int RB, int ir, int kx, int cb, int KY>
__device__ __forceinline__ void band_mfma(const bf16x8 (&A)[Geo<C>::KS], f32x4 (&acc)[RB][W / 16],
                                          const bf16x8 (&B)[W / 16]) {
  constexpr int r = ir - KY;
  if constexpr (r >= 0 && r < RB) {
    constexpr int ks = (KY * 3 + kx) * Band<C, W, RB>::NCB + cb;
#pragma unroll
    for (int pt = 0; pt < W / 16; ++pt)
      acc[r][pt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[ks], B[pt], acc[r][pt], 0, 0, 0);
  }
}

struct NoHook {
  template <typename U>
  __device__ __forceinline__ void operator()(U) const {}
};

// hook(integral_constant<int, u>) is called once for u = 0 .. NU-1, spread
// evenly over the pipeline stages (the forward interleaves the previous
// band's epilogue with this band's MFMAs that way)
template <int C, int W, int RB, int NU, int S, typename Hook>
__device__ __forceinline__ void band_step(unsigned base, unsigned baseh, const unsigned (&lo)[3 * Band<C, W, RB>::NCB],
                                          const bf16x8 (&A)[Geo<C>::KS], f32x4 (&acc)[RB][W / 16],
                                          bf16x8 (&B)[3][W / 16], Hook& hook) {
  using BD = Band<C, W, RB>;
  constexpr int PT = BD::PT;
  if constexpr (S < BD::NS) {
    constexpr int blk = S / BD::NR, ir = S % BD::NR;
    constexpr int kx = blk / BD::NCB, cb = blk % BD::NCB;
    lgkm_wait<(S + 1 < BD::NS) ? PT : 0>();
    band_mfma<C, W, RB, ir, kx, cb, 0>(A, acc, B[S % 3]);
    band_mfma<C, W, RB, ir, kx, cb, 1>(A, acc, B[S % 3]);
    band_mfma<C, W, RB, ir, kx, cb, 2>(A, acc, B[S % 3]);
    if constexpr (S + 2 < BD::NS) band_issue<C, W, RB, S + 2>(base, baseh, lo, B[(S + 2) % 3]);
    if constexpr (NU > 0) {
      constexpr int SP = BD::NS / NU;
      if constexpr (SP > 0 && S % SP == SP / 2 && S / SP < NU) hook(std::integral_constant<int, S / SP>{});
    }
    band_step<C, W, RB, NU, S + 1>(base, baseh, lo, A, acc, B, hook);
  }
}

// acc[r][pt] += conv over the RB output rows whose first input row is the
// tile row at LDS byte address `base`
template <int C, int W, int RB, int NU = 0, typename Hook = NoHook>
__device__ __forceinline__ void conv_band2(unsigned base, unsigned baseh, const unsigned (&lo)[3 * Band<C, W, RB>::NCB],
                                           const bf16x8 (&A)[Geo<C>::KS], f32x4 (&acc)[RB][W / 16], Hook hook = {}) {
  bf16x8 B[3][W / 16];
  lgkm_wait<0>();
  band_issue<C, W, RB, 0>(base, baseh, lo, B[0]);
  band_issue<C, W, RB, 1>(base, baseh, lo, B[1]);
  band_step<C, W, RB, NU, 0>(base, baseh, lo, A, acc, B, hook);
}
template <int C, int W, int RB, int NU = 0, typename Hook = NoHook>
__device__ __forceinline__ void conv_band(unsigned base, const unsigned (&lo)[3 * Band<C, W, RB>::NCB],
                                          const bf16x8 (&A)[Geo<C>::KS], f32x4 (&acc)[RB][W / 16], Hook hook = {}) {
  conv_band2<C, W, RB, NU, Hook>(base, base, lo, A, acc, hook);
}

template <int C, int W, int RB>
__device__ __forceinline__ void band_lane_offsets(int g, int lx, unsigned (&lo)[3 * Band<C, W, RB>::NCB]) {
  using BD = Band<C, W, RB>;
#pragma unroll
  for (int kx = 0; kx < 3; ++kx)
#pragma unroll
    for (int cb = 0; cb < BD::NCB; ++cb) lo[kx * BD::NCB + cb] = (unsigned)toff<C>(0, lx + kx, 4 * cb + g, BD::TW);
}

// W^T fragments of one 16-channel output tile
template <int C>
__device__ __forceinline__ void load_A1(const bf16* __restrict__ wpack, int ot, int lane, bf16x8 (&A)[Geo<C>::KS]) {
#pragma unroll
  for (int ks = 0; ks < Geo<C>::KS; ++ks)
    A[ks] = *(const bf16x8*)(wpack + (((long)ot * Geo<C>::KS + ks) * 64 + lane) * 8);
}

// load_A1 / the 4 bias values of lane group g by untracked loads (see
// gload128_untracked): for the stacks' per-block reloads, whose results the
// next item's barrier_vm retires.  Unconditional loads into the registers the
// values live in (a null bias reads the zero page): a conditional load would
// make hipcc merge the two values with copies that read the registers before
// the load retires.
template <int C, int KS0 = 0>
__device__ __forceinline__ void load_A1_untracked_at(const unsigned char* base, unsigned voff, bf16x8 (&A)[Geo<C>::KS]) {
  if constexpr (KS0 < Geo<C>::KS) {
    u32x4 v = __builtin_bit_cast(u32x4, A[KS0]);
    // the base advances by 4 KiB every 4 loads (an SALU add): only a load right after
    // such an add (or the readfirstlane of the first) needs the 5 wait states
    gload128_untracked<(KS0 % 4) * 1024, KS0 % 4 == 0>(v, base + (KS0 / 4) * 4096, voff);
    A[KS0] = __builtin_bit_cast(bf16x8, v);
    load_A1_untracked_at<C, KS0 + 1>(base, voff, A);
  }
}
template <int C>
__device__ __forceinline__ void load_A1_untracked(const bf16* __restrict__ wpack, int ot, int lane,
                                                  bf16x8 (&A)[Geo<C>::KS]) {
  const auto* base = (const unsigned char*)uniform_ptr((const unsigned char*)wpack + (long)ot * Geo<C>::KS * 1024);
  load_A1_untracked_at<C>(base, (unsigned)lane * 16u, A);
}
// b: the wave's 16 bias values (wave-uniform); lane group g reads 4 of them
__device__ __forceinline__ void load_bias4_untracked(const float* __restrict__ b, int g, float (&bz)[4]) {
  const void* base = uniform_ptr(b ? (const void*)b : (const void*)g_zero_page);
  const unsigned voff = (unsigned)g * 16u;
  gload32_untracked<0>(bz[0], base, voff);
  gload32_untracked<4>(bz[1], base, voff);
  gload32_untracked<8>(bz[2], base, voff);
  gload32_untracked<12>(bz[3], base, voff);
}

template <int C>
__device__ __forceinline__ void load_A(const bf16* __restrict__ wpack, int oh, int lane,
                                       bf16x8 (&A)[Geo<C>::OTW][Geo<C>::KS]) {
  using G = Geo<C>;
#pragma unroll
  for (int t = 0; t < G::OTW; ++t)
#pragma unroll
    for (int ks = 0; ks < G::KS; ++ks)
      A[t][ks] = *(const bf16x8*)(wpack + (((long)(oh * G::OTW + t) * G::KS + ks) * 64 + lane) * 8);
}

// contiguous run of items for this workgroup
__device__ __forceinline__ void item_range(int items, int* i0, int* i1) {
  const int per = items / (int)gridDim.x, rem = items % (int)gridDim.x;
  const int b = blockIdx.x;
  *i0 = b * per + min(b, rem);
  *i1 = *i0 + per + (b < rem ? 1 : 0);
}

// (image, band) of consecutive items without a division per item
struct ItemCursor {
  int n, b;
  __device__ __forceinline__ ItemCursor(int it, int nb) : n(it / nb), b(it % nb) {}
  __device__ __forceinline__ void next(int nb) {
    if (++b == nb) {
      b = 0;
      ++n;
    }
  }
};

}  // namespace blk
}  // namespace asr
