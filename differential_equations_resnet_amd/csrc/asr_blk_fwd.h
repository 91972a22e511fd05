// Per-block forward of the bf16 Euler block at W = 32 (one launch per block;
// part of asr_block_mfma.hip's translation unit): y = x + h relu(conv(x) + b)
// with the relu mask (FWD_EULER), or the bare conv(x) + b (FWD_CONV).  All
// three kernels are persistent over 4-row bands, 256 threads (4 waves), with
// the next band's input rows in flight by LDS-DMA into the other tile buffer;
// launch_fwd_v (asr_block_mfma.hip) picks by C:
//   k_fwd       C = 16: a row at a time (conv_row), conv then epilogue, 2 workgroups per CU;
//   k_fwd_pipe  C = 32, and at C = 64 the compositions k_fwd3 leaves out: band
//               form, band i+1's MFMAs interleaved with band i's epilogue;
//   k_fwd3      C = 64: band form at three workgroups per CU, no cross-band pipeline.
// Each kernel's own comment has its protocol.
#pragma once
#include <type_traits>

#include "asr_blk_common.h"
#include "asr_common.h"
#include "asr_device.h"

namespace asr {
namespace blk {

// ===========================================================================
// forward
// ===========================================================================
template <int C, int W, int BR, int MODE, int NW>
__global__ __launch_bounds__(64 * NW) void k_fwd(const bf16* __restrict__ x, const bf16* __restrict__ resid,
                                             bf16* __restrict__ y, uint8_t* __restrict__ mask,
                                             const bf16* __restrict__ wpack, const float* __restrict__ bias,
                                             float h, int N, int H) {
  using G = Geo<C>;
  constexpr int TW = W + 2, PT = W / 16, NQ = G::NQ, OTW = G::OTW;
  constexpr int TILE = (BR + 2) * TW * NQ * 16;
  constexpr int RS = NW / G::OSPLIT;  // waves splitting the band's rows
  constexpr bool EULER = MODE == FWD_EULER;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int oh = wave % G::OSPLIT, rg = wave / G::OSPLIT;
  const int g = lane >> 4, lx = lane & 15;

  bf16x8 A[OTW][G::KS];
  load_A<C>(wpack, oh, lane, A);
  Frag<C, W> boff;
  boff.init(g, lx);
  float bz[OTW][4];
#pragma unroll
  for (int t = 0; t < OTW; ++t)
#pragma unroll
    for (int e = 0; e < 4; ++e) bz[t][e] = bias ? bias[16 * (oh * OTW + t) + 4 * g + e] : 0.f;

  zero_halo_cols<C, W>(lds, BR + 2, tid, 64 * NW);
  zero_halo_cols<C, W>(lds + TILE, BR + 2, tid, 64 * NW);
  const int nb = (H + BR - 1) / BR;
  int i0, i1;
  item_range(N * nb, &i0, &i1);
  ItemCursor cur(i0, nb), nxt(i0, nb);
  if (i0 < i1) {
    const int y0 = cur.b * BR;
    dma_rows<C, W>(x, lds, cur.n, y0 - 1, min(BR, H - y0) + 2, H, wave, NW, lane);
  }
  nxt.next(nb);
  int nst = 0;  // global stores this wave issued after the DMA it must now wait for
  for (int it = i0; it < i1; ++it, cur.next(nb), nxt.next(nb)) {
    const int buf = (it - i0) & 1;
    unsigned char* tile = lds + buf * TILE;
    barrier_vm(nst);  // this item's DMA has landed; the other buffer is free
    nst = 0;
    if (it + 1 < i1) {
      const int y1 = nxt.b * BR;
      dma_rows<C, W>(x, lds + (buf ^ 1) * TILE, nxt.n, y1 - 1, min(BR, H - y1) + 2, H, wave, NW, lane);
    }
    const int n = cur.n, y0 = cur.b * BR;
    const int rows = min(BR, H - y0);
    for (int r = rg; r < rows; r += RS) {
      f32x4 acc[OTW][PT];
#pragma unroll
      for (int t = 0; t < OTW; ++t)
#pragma unroll
        for (int pt = 0; pt < PT; ++pt) acc[t][pt] = f32x4{bz[t][0], bz[t][1], bz[t][2], bz[t][3]};
      conv_row<C, W>(tile, r, A, boff, acc);
      const int gy = y0 + r;
      nst += PT * (OTW + ((EULER && mask) ? 1 : 0));
#pragma unroll
      for (int pt = 0; pt < PT; ++pt) {
        const int px = 16 * pt + lx;
        unsigned mword = 0;
#pragma unroll
        for (int t = 0; t < OTW; ++t) {
          const int o0 = 16 * (oh * OTW + t) + 4 * g;
          bf16x4 o4;
          if constexpr (EULER) {
            // residual: x itself (LDS tile) or, for the second RK2 stage, the step's input
            const bf16x4 xr = resid ? *(const bf16x4*)(resid + (((long)n * H + gy) * W + px) * C + o0)
                                    : *(const bf16x4*)(tile + toff<C>(r + 1, px + 1, o0 >> 3, TW) + (o0 & 4) * 2);
            unsigned nib = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float z = acc[t][pt][e];
              const bool pos = z > 0.f;  // relu'(z) as TF's ReluGrad: z > 0
              nib |= (pos ? 1u : 0u) << e;
              o4[e] = (bf16)fmaf(h, pos ? z : 0.f, (float)xr[e]);
            }
            mword |= nib << (16 * t + 4 * g);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) o4[e] = (bf16)acc[t][pt][e];
          }
          *(bf16x4*)(y + (((long)n * H + gy) * W + px) * C + o0) = o4;
        }
        if constexpr (EULER) {
          // OR over the four lane groups g (lanes lx, lx+16, lx+32, lx+48)
          const auto s16 = __builtin_amdgcn_permlane16_swap(mword, mword, false, false);
          mword = s16[0] | s16[1];
          const auto s32 = __builtin_amdgcn_permlane32_swap(mword, mword, false, false);
          mword = s32[0] | s32[1];
          if (mask && g == 0) {
            uint8_t* mp = mask + ((((long)n * H + gy) * W + px) * C + 16 * oh * OTW) / 8;
            if constexpr (OTW == 2)
              *(uint32_t*)mp = mword;
            else
              *(uint16_t*)mp = (uint16_t)mword;
          }
        }
      }
    }
  }
}

template <int NU, int U = 0, typename F, typename Acc, typename Xr, typename Cur>
__device__ __forceinline__ void epi_all_units(F& f, const Acc& acc, const Xr& xr, const Cur& c) {
  if constexpr (U < NU) {
    f(std::integral_constant<int, U>{}, acc, xr, c);
    epi_all_units<NU, U + 1>(f, acc, xr, c);
  }
}

// Forward, band form with a software pipeline across bands: the MFMAs of
// band i+1 are interleaved with the epilogue (VALU + stores) of band i, so
// the matrix pipe and the vector ALU of one wave work at the same time.
// RESG (second RK2 stage, default): the residual `resid` read from global
// memory.  Band i+1's loads are issued right after band i+2's DMA and
// consumed (an empty asm that reads them) right after the next barrier, before
// any later DMA: hipcc's own vmcnt wait for a load counts only the memory ops
// it sees, so a use behind a younger inline-asm DMA would wait for that DMA.
template <int C, int W, int BR, int MODE, int NW, bool RESG = false>
__global__ __launch_bounds__(64 * NW, 2) void k_fwd_pipe(const bf16* __restrict__ x, const bf16* __restrict__ resid,
                                                  bf16* __restrict__ y, uint8_t* __restrict__ mask,
                                                  const bf16* __restrict__ wpack, const float* __restrict__ bias,
                                                  float h, int N, int H) {
  using G = Geo<C>;
  constexpr int TW = W + 2, PT = W / 16, NQ = G::NQ, OT = C / 16;
  constexpr int TILE = (BR + 2) * TW * NQ * 16;
  static_assert(NW % OT == 0, "waves must cover the o-tiles");
  constexpr int RS = NW / OT, RB = BR / RS;
  static_assert(BR % RS == 0, "row groups must split the band");
  using BD = Band<C, W, RB>;
  // epilogue units: (row, pixel tile), or rows with both pixel tiles stored
  // as 16-B chunks
  constexpr bool ST16 = PT == 2;
  constexpr int NU = ST16 ? RB : RB * PT;
  constexpr bool EULER = MODE == FWD_EULER;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ot = wave % OT, rg = wave / OT;
  const int g = lane >> 4, lx = lane & 15;
  const int o0 = 16 * ot + 4 * g;
  const int r0 = rg * RB;

  bf16x8 A[G::KS];
  load_A1<C>(wpack, ot, lane, A);
  unsigned lo[3 * BD::NCB];
  band_lane_offsets<C, W, RB>(g, lx, lo);
  float bz[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) bz[e] = bias ? bias[o0 + e] : 0.f;
  const unsigned ly = (unsigned)(lx * C + o0);
  const unsigned lm = (unsigned)(lx * (C / 8) + 2 * ot);
  const unsigned lxr = (unsigned)(toff<C>(r0 + 1, lx + 1, o0 >> 3, TW) + (o0 & 4) * 2);

  zero_halo_cols<C, W>(lds, BR + 2, tid, 64 * NW);
  zero_halo_cols<C, W>(lds + TILE, BR + 2, tid, 64 * NW);
  const int nb = (H + BR - 1) / BR;
  int i0, i1;
  item_range(N * nb, &i0, &i1);
  if (i0 >= i1) return;
  ItemCursor cur(i0, nb), nx1(i0, nb), nx2(i0, nb);  // items it, it+1, it+2
  nx1.next(nb);
  nx2.next(nb);
  nx2.next(nb);
  auto dma = [&](const ItemCursor& c, int buf) {
    const int yy = c.b * BR;
    dma_rows<C, W>(x, lds + buf * TILE, c.n, yy - 1, min(BR, H - yy) + 2, H, wave, NW, lane);
  };
  // band c continues band p's image (p's tile in the other buffer, complete):
  // its halo rows 0, 1 are p's rows BR, BR+1 -> copy them (interior columns),
  // DMA only rows 2..
  auto dma_next2 = [&](const ItemCursor& c, const ItemCursor& p, int buf) {
    if (c.n != p.n || c.b != p.b + 1) {
      dma(c, buf);
      return;
    }
    const int yy = c.b * BR;
    constexpr int ROWB = TW * NQ * 16;
    dma_rows<C, W>(x, lds + buf * TILE + 2 * ROWB, c.n, yy + 1, min(BR, H - yy), H, wave, NW, lane);
    // plain LDS accesses (the DMA is inline asm, invisible to the compiler,
    // so it waits only lgkmcnt for these; asm reads with a deferred wait are
    // unsafe where hipcc copies their results before the wait)
    const uint4* src = (const uint4*)(lds + (buf ^ 1) * TILE + BR * ROWB);
    uint4* dst = (uint4*)(lds + buf * TILE);
    constexpr int NCH = 2 * W * NQ;
    for (int i = tid; i < NCH; i += 64 * NW) dst[((i / (W * NQ)) * TW + 1) * NQ + i % (W * NQ)] =
        src[((i / (W * NQ)) * TW + 1) * NQ + i % (W * NQ)];
  };
  int nst = 0;  // vector-memory ops this wave issued after the DMA the next barrier waits for
  // residual of a band: x from its LDS tile (read after the band's conv)
  auto xres_read = [&](int buf, u32x2 (&xr)[RB][PT]) {
    if constexpr (EULER && !RESG) {
      const unsigned tb = lds_u32(lds + buf * TILE) + lxr;
#pragma unroll
      for (int r = 0; r < RB; ++r)
#pragma unroll
        for (int pt = 0; pt < PT; ++pt) xr[r][pt] = lds_rd64(tb + (unsigned)(r * BD::ROWB + pt * BD::PTB));
      lgkm_wait<0>();
    }
  };
  // RESG: every lane issues exactly RB*PT loads (rows past the image end
  // re-read its last row), so the barrier counts stay exact
  const unsigned lres = (unsigned)(2 * (lx * C + o0));
  auto xg_load = [&](const ItemCursor& c, u32x2 (&xr)[RB][PT]) {
    if constexpr (RESG) {
      const int y0 = c.b * BR, rows = min(BR, H - y0);
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        const int ur = __builtin_amdgcn_readfirstlane((c.n * H + y0 + min(r0 + r, rows - 1)) * W);
        const unsigned char* rb = (const unsigned char*)(resid + (long)ur * C);
#pragma unroll
        for (int pt = 0; pt < PT; ++pt) xr[r][pt] = *(const u32x2*)(rb + lres + (unsigned)(2 * 16 * pt * C));
      }
      nst += RB * PT;
    }
  };
  auto xg_consume = [&](u32x2 (&xr)[RB][PT]) {
    if constexpr (RESG) {
#pragma unroll
      for (int r = 0; r < RB; ++r)
#pragma unroll
        for (int pt = 0; pt < PT; ++pt) asm volatile("" : "+v"(xr[r][pt]));
    }
  };
  auto init = [&](f32x4 (&acc)[RB][PT]) {
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
      for (int pt = 0; pt < PT; ++pt) acc[r][pt] = f32x4{bz[0], bz[1], bz[2], bz[3]};
  };
  // y and the relu-mask word of output row r, pixel tile pt (every lane
  // ends with the 16-bit mask word of its pixel: OR over the 4 lane rows)
  auto epi_vals = [&](int r, int pt, const f32x4 (&acc)[RB][PT], const u32x2 (&xr)[RB][PT], u32x2& ov,
                      unsigned& mword) {
    bf16x4 o4;
    mword = 0;
    if constexpr (EULER) {
      const bf16x4 xv = *(const bf16x4*)&xr[r][pt];
      unsigned nib = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float z = acc[r][pt][e];
        const bool pos = z > 0.f;  // relu'(z) as TF's ReluGrad: z > 0
        nib |= (pos ? 1u : 0u) << e;
        const float rz = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, z) & (pos ? ~0u : 0u));
        o4[e] = (bf16)fmaf(h, rz, (float)xv[e]);
      }
      mword = nib << (4 * g);
      const auto s16 = __builtin_amdgcn_permlane16_swap(mword, mword, false, false);
      mword = s16[0] | s16[1];
      const auto s32 = __builtin_amdgcn_permlane32_swap(mword, mword, false, false);
      mword = s32[0] | s32[1];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) o4[e] = (bf16)acc[r][pt][e];
    }
    ov = *(const u32x2*)&o4;
  };
  // one epilogue unit of the band at cursor c
  auto epi_unit = [&](auto U, const f32x4 (&acc)[RB][PT], const u32x2 (&xr)[RB][PT], const ItemCursor& c) {
    constexpr int u = decltype(U)::value;
    const int y0 = c.b * BR;
    if constexpr (ST16) {
      // row r, both pixel tiles: a 16-lane row swap between the tiles gives
      // lane row g the 8 channels 16*ot + 8*(g>>1) of pixel 16*(g&1) + lx
      constexpr int r = u;
      if (r0 + r >= min(BR, H - y0)) return;
      const long row = ((long)c.n * H + y0 + r0 + r) * W;
      nst += (EULER && mask) ? 2 : 1;
      u32x2 ov[2];
      unsigned mw[2];
      epi_vals(r, 0, acc, xr, ov[0], mw[0]);
      epi_vals(r, 1, acc, xr, ov[1], mw[1]);
      const auto s0 = __builtin_amdgcn_permlane16_swap(ov[0][0], ov[1][0], false, false);
      const auto s1 = __builtin_amdgcn_permlane16_swap(ov[0][1], ov[1][1], false, false);
      *(u32x4*)(y + (row + 16 * (g & 1) + lx) * C + 16 * ot + 8 * (g >> 1)) = u32x4{s0[0], s1[0], s0[1], s1[1]};
      if (EULER && mask && g < 2) *(uint16_t*)(mask + (row + 16 * g) * (C / 8) + lm) = (uint16_t)(g ? mw[1] : mw[0]);
    } else {
      constexpr int r = u / PT, pt = u % PT;
      if (r0 + r >= min(BR, H - y0)) return;
      const long row = ((long)c.n * H + y0 + r0 + r) * W + 16 * pt;
      nst += (EULER && mask) ? 2 : 1;
      u32x2 ov;
      unsigned mword;
      epi_vals(r, pt, acc, xr, ov, mword);
      if (EULER && mask && g == 0) *(uint16_t*)(mask + row * (C / 8) + lm) = (uint16_t)mword;
      *(u32x2*)(y + row * C + ly) = ov;
    }
  };
  auto epi_all = [&](const f32x4 (&acc)[RB][PT], const u32x2 (&xr)[RB][PT], const ItemCursor& c) {
    epi_all_units<NU>(epi_unit, acc, xr, c);
  };

  f32x4 accA[RB][PT], accB[RB][PT];
  u32x2 xrA[RB][PT], xrB[RB][PT];
  // prologue: band i0 computed (its epilogue waits for the next band's MFMAs)
  dma(cur, 0);
  barrier_vm(0);
  if (i0 + 1 < i1) dma(nx1, 1);
  xg_load(cur, xrA);
  init(accA);
  conv_band<C, W, RB>(lds_u32(lds + r0 * BD::ROWB), lo, A, accA);
  xres_read(0, xrA);
  int it = i0;
  while (true) {
    // accA / xrA: band it.  In flight: DMA of band it+1 into buffer (it+1-i0)&1.
    if (it + 1 >= i1) {
      epi_all(accA, xrA, cur);
      break;
    }
    ASR_STAMP(it - i0, 0);
    barrier_vm(nst);  // band it+1 landed, every wave is done with band it's tile
    ASR_STAMP(it - i0, 1);
    nst = 0;
    xg_consume(xrA);
    if (it + 2 < i1) dma_next2(nx2, nx1, (it - i0) & 1);
    xg_load(nx1, xrB);
    ASR_STAMP(it - i0, 2);
    init(accB);
    {
      const ItemCursor c = cur;
      auto hook = [&](auto U) { epi_unit(U, accA, xrA, c); };
      conv_band<C, W, RB, NU>(lds_u32(lds + ((it + 1 - i0) & 1) * TILE + r0 * BD::ROWB), lo, A, accB, hook);
    }
    ASR_STAMP(it - i0, 3);
    xres_read((it + 1 - i0) & 1, xrB);
    ASR_STAMP(it - i0, 4);
    ++it;
    cur.next(nb);
    nx1.next(nb);
    nx2.next(nb);
    // the same with the roles of A and B swapped
    if (it + 1 >= i1) {
      epi_all(accB, xrB, cur);
      break;
    }
    ASR_STAMP(it - i0, 0);
    barrier_vm(nst);
    ASR_STAMP(it - i0, 1);
    nst = 0;
    xg_consume(xrB);
    if (it + 2 < i1) dma_next2(nx2, nx1, (it - i0) & 1);
    xg_load(nx1, xrA);
    ASR_STAMP(it - i0, 2);
    init(accA);
    {
      const ItemCursor c = cur;
      auto hook = [&](auto U) { epi_unit(U, accB, xrB, c); };
      conv_band<C, W, RB, NU>(lds_u32(lds + ((it + 1 - i0) & 1) * TILE + r0 * BD::ROWB), lo, A, accA, hook);
    }
    ASR_STAMP(it - i0, 3);
    xres_read((it + 1 - i0) & 1, xrA);
    ASR_STAMP(it - i0, 4);
    ++it;
    cur.next(nb);
    nx1.next(nb);
    nx2.next(nb);
  }
}

// Forward, band form at three waves per SIMD (C = 64; 3 WGs of 4 waves per
// CU, <= 168 VGPRs): no cross-band software pipeline.  Each wave runs its
// o-tile's band conv, then the band's epilogue; the other two workgroups on
// the CU keep the matrix pipe busy meanwhile.  The epilogue works on the
// regrouped accumulators (v_permlane16_swap: lane (lx, g) owns channels
// 16*ot + 8*(g>>1) + 0..7 of pixel lx + 16*(g&1)): the residual is one
// ds_read_b128 of the band's LDS tile, y one 16-B store, the relu bits one
// byte per lane (v_med3 + v_lshl_or, relu as an integer max on the bit
// pattern).  MFMA accumulation order and rounding equal k_fwd_pipe's, so both
// kernels give bitwise the same y and mask.
// RESG (second RK2 stage): the residual is `resid` (the step input), not the
// conv input x: 16-B global loads in the regrouped layout, issued before the conv.
template <int C, int W, int BR, int MODE, int WPE, bool RESG = false>
__global__ __launch_bounds__(256, WPE) void k_fwd3(const bf16* __restrict__ x, const bf16* __restrict__ resid,
                                                   bf16* __restrict__ y, uint8_t* __restrict__ mask,
                                                   const bf16* __restrict__ wpack, const float* __restrict__ bias,
                                                   float h, int N, int H) {
  using G = Geo<C>;
  constexpr int TW = W + 2, NQ = G::NQ, OT = C / 16, NW = 4, RB = BR;
  static_assert(OT == NW && W == 32, "one 16-channel o-tile per wave, two pixel tiles");
  using BD = Band<C, W, RB>;
  constexpr int TILE = (BR + 2) * BD::ROWB;
  constexpr bool EULER = MODE == FWD_EULER;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ot = wave, g = lane >> 4, lx = lane & 15;
  const int o0 = 16 * ot + 4 * g;
  const int px = lx + 16 * (g & 1), cg = 2 * ot + (g >> 1);  // after the regroup: pixel, 16-B channel chunk

  bf16x8 A[G::KS];
  load_A1<C>(wpack, ot, lane, A);
  unsigned lo[3 * BD::NCB];
  band_lane_offsets<C, W, RB>(g, lx, lo);
  float bz[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) bz[e] = bias ? bias[o0 + e] : 0.f;
  const unsigned lxr = (unsigned)toff<C>(1, px + 1, cg, TW);  // output row 0's residual chunk
  const unsigned ly = (unsigned)(px * C + 8 * cg) * 2u, lm = (unsigned)(px * (C / 8) + cg);

  zero_halo_cols<C, W>(lds, BR + 2, tid, 64 * NW);
  zero_halo_cols<C, W>(lds + TILE, BR + 2, tid, 64 * NW);
  const int nb = (H + BR - 1) / BR;
  int i0, i1;
  item_range(N * nb, &i0, &i1);
  if (i0 >= i1) return;
  ItemCursor cur(i0, nb), nxt(i0, nb);
  nxt.next(nb);
  {
    const int yy = cur.b * BR;
    dma_rows<C, W>(x, lds, cur.n, yy - 1, min(BR, H - yy) + 2, H, wave, NW, lane);
  }
  int nst = 0;  // vector-memory ops issued after the DMA the next barrier waits for
  ASR_BCLK(0, 0);
  for (int it = i0; it < i1; ++it, cur.next(nb), nxt.next(nb)) {
    const int buf = (it - i0) & 1;
    if (wave == 0) ASR_BTR(0, 0, it - i0, 0);
    barrier_vm_usual<2 * BR>(nst);  // band it landed; every wave is done with band it-1's tile
    if (wave == 0) ASR_BTR(0, 0, it - i0, 1);
    nst = 0;
    if (it + 1 < i1) {
      // the next band into the other buffer; its rows 0, 1 are this band's rows
      // BR, BR+1 when it continues the image (copied inside LDS, the rest by DMA)
      unsigned char* nt = lds + (buf ^ 1) * TILE;
      const int yy = nxt.b * BR;
      if (nxt.n == cur.n && nxt.b == cur.b + 1) {
        dma_rows<C, W>(x, nt + 2 * BD::ROWB, nxt.n, yy + 1, min(BR, H - yy), H, wave, NW, lane);
        const uint4* src = (const uint4*)(lds + buf * TILE + BR * BD::ROWB);
        uint4* dst = (uint4*)nt;
        constexpr int NCH = 2 * W * NQ;
        for (int i = tid; i < NCH; i += 64 * NW) {
          const int o = ((i / (W * NQ)) * TW + 1) * NQ + i % (W * NQ);
          dst[o] = src[o];
        }
      } else {
        dma_rows<C, W>(x, nt, nxt.n, yy - 1, min(BR, H - yy) + 2, H, wave, NW, lane);
      }
    }
    const unsigned tb = lds_u32(lds + buf * TILE);
    u32x4 xr[RB];
    if constexpr (RESG) {  // rows past the image end re-read its last row (never stored)
      const int y0 = cur.b * BR, rows = min(BR, H - y0);
      const unsigned char* rb = (const unsigned char*)(resid + ((long)cur.n * H + y0) * W * C) + ly;
#pragma unroll
      for (int r = 0; r < RB; ++r) xr[r] = *(const u32x4*)(rb + (long)min(r, rows - 1) * W * C * 2);
    }
    f32x4 acc[RB][2];
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
      for (int pt = 0; pt < 2; ++pt) acc[r][pt] = f32x4{bz[0], bz[1], bz[2], bz[3]};
    if (wave == 0) ASR_BTR(0, 0, it - i0, 2);
    conv_band<C, W, RB>(tb, lo, A, acc);
    if (wave == 0) ASR_BTR(0, 0, it - i0, 3);
    if constexpr (EULER && !RESG) {
#pragma unroll
      for (int r = 0; r < RB; ++r) xr[r] = lds_rd128(tb + lxr + (unsigned)(r * BD::ROWB));
      lgkm_wait<0>();
    }
    const int y0 = cur.b * BR, rows = min(BR, H - y0);
    const long rowb = ((long)cur.n * H + y0) * W;
    unsigned char* yb = (unsigned char*)(y + rowb * C) + ly;
    uint8_t* mb = mask ? mask + rowb * (C / 8) + lm : nullptr;
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      if (r >= rows) break;
      float z[8];
      regroup(acc[r][0], acc[r][1], z);
      u32x4 yw;
      if constexpr (EULER) {
        unsigned bits = 0;
        static_for<0, 4>([&](auto dc) {
          constexpr int d = decltype(dc)::value;
          const int ra = max(__float_as_int(z[2 * d]), 0), rb = max(__float_as_int(z[2 * d + 1]), 0);
          yw[d] = pk_bf16(fmaf(h, __int_as_float(ra), lo_f(xr[r][d])), fmaf(h, __int_as_float(rb), hi_f(xr[r][d])));
          bits = d == 0 ? bit01(ra) : lshl_or<2 * d>(bit01(ra), bits);
          bits = lshl_or<2 * d + 1>(bit01(rb), bits);
        });
        if (mb) {
          mb[r * W * (C / 8)] = (uint8_t)bits;
          ++nst;
        }
      } else {
#pragma unroll
        for (int d = 0; d < 4; ++d) yw[d] = pk_bf16(z[2 * d], z[2 * d + 1]);
      }
      *(u32x4*)(yb + r * W * C * 2) = yw;
      ++nst;
    }
    if (wave == 0) ASR_BTR(0, 0, it - i0, 4);
  }
  ASR_BCLK(0, 1);
}

}  // namespace blk
}  // namespace asr
