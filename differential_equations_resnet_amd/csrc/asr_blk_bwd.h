// Per-block fused backward of the bf16 Euler block at W = 32 (one launch per
// block: dgrad + wgrad + db in one pass; part of asr_block_mfma.hip's
// translation unit).  A persistent workgroup per CU walks 4-row bands; the dgrad
// waves hold the W fragments in VGPRs, the wgrad waves hold the dW tile set in
// accumulators for the workgroup's whole run and write one [dW | db] slab per
// workgroup at the end; both read the same LDS images of dz (from dy and the
// relu mask, once per band) and x.  launch_bwd (asr_block_mfma.hip) picks:
//   k_bwd   v1, 512 threads (8 waves): C = 16 and 32, and the C = 64
//           compositions k_bwd3 does not cover;
//   k_bwd3  v3, C = 64, 768 threads (12 waves) on the v2 band protocol (Bwd2Lds);
//           k_bwd3_stack (asr_blk_stack.h) runs the same protocol over all blocks.
// Each has its design above it.
#pragma once
#include <type_traits>

#include "asr_blk_common.h"
#include "asr_common.h"
#include "asr_device.h"

namespace asr {
namespace blk {

// ===========================================================================
// Backward v1 (k_bwd: C = 16 / 32, and the C = 64 compositions k_bwd3 leaves
// out).  One 512-thread workgroup per CU: waves 0-3 own the dgrad (W fragments
// resident in VGPRs), waves 4-7 the wgrad (the dW tile set resident in
// accumulators for the workgroup's whole run); both consume the same LDS
// images of dz (computed once per item from dy and the relu mask, by all 8
// waves between two barriers) and x.  kBwdDgradDmaPct of the next band's
// prefetch DMAs are issued by the dgrad waves inside their k-steps.
// ===========================================================================
template <int C, int W, int BR>
struct BwdLds {
  static constexpr int TW = W + 2;
  static constexpr int TILE = (BR + 2) * TW * (C / 8) * 16;
  static constexpr int RBM = W * C / 8;  // mask bytes per image row
  // mask bytes per buffer: the band's rows, or 2 copied rows + whole 1 KiB DMAs of the other BR
  static constexpr int MTB0 = ((BR + 2) * RBM + 1023) / 1024 * 1024;
  static constexpr int MTB1 = (2 * RBM + (BR * RBM + 1023) / 1024 * 1024 + 1023) / 1024 * 1024;
  static constexpr int MTB = MTB0 > MTB1 ? MTB0 : MTB1;
  static constexpr int DY = 0;                 // 2 x TILE (dy, halo rows)
  static constexpr int X = DY + 2 * TILE;      // 2 x TILE (x, halo rows)
  static constexpr int DZ = X + 2 * TILE;      // 1 x TILE (dz, halo rows)
  static constexpr int MSK = DZ + TILE;        // 2 x MTB
  static constexpr int TOTAL = MSK + 2 * MTB;
  // XT (RK2 first stage): per dgrad wave, a private copy of the extra dx
  // term for its MR rows x W pixels x its OTW o-tiles (NCH 16-B chunks/pixel)
  static constexpr int RS = 4 / Geo<C>::OSPLIT, MR = (BR + RS - 1) / RS;
  static constexpr int NCH = 2 * Geo<C>::OTW;
  static constexpr int ROWX = W * NCH * 16;    // bytes per private row
  static constexpr int EXT = TOTAL;            // 4 x MR x ROWX
  static constexpr int TOTAL_XT = EXT + 4 * MR * ROWX;
  static_assert(ROWX % 1024 == 0, "private extra rows are whole 1 KiB DMAs");
};

// DMA the extra dx term of one dgrad wave's rows (rg + k*RS) of the band at
// image row y0, its channels [16*OTW*oh, +16*OTW), into the wave's private
// rows: 16-B chunk j of pixel px sits in slot j ^ ((px / PXG) % NCH), PXG =
// the pixels one 64-bank span holds, so the epilogue's 8-B reads do not
// conflict.  Rows outside the band read the zero page.  Issues MR*ROWX/1024
// instructions.
template <int C, int W, int BR>
__device__ __forceinline__ void dma_extra(const bf16* __restrict__ extra, unsigned char* priv, int n, int y0, int rows,
                                          int H, int rg, int oh, int lane) {
  using L = BwdLds<C, W, BR>;
  constexpr int NCH = L::NCH, PXG = 64 / (NCH * 4);
#pragma unroll
  for (int k = 0; k < L::MR; ++k) {
    const int r = rg + k * L::RS;
#pragma unroll
    for (int q = 0; q < L::ROWX / 1024; ++q) {
      const int lb = q * 1024 + lane * 16;
      const int px = lb / (NCH * 16), slot = (lb / 16) % NCH;
      const int chunk = slot ^ ((px / PXG) % NCH);
      const void* src = (r < rows) ? (const void*)(extra + (((long)n * H + y0 + r) * W + px) * C +
                                                   16 * Geo<C>::OTW * oh + 8 * chunk)
                                   : (const void*)(g_zero_page + lane);
      dma16(src, priv + k * L::ROWX + q * 1024);
    }
  }
}

// The prefetch of the next band as one stream of 1 KiB DMA instructions
// [dy rows | x rows | mask chunks].  When the next band continues the same
// image, its two top tile rows are this band's two bottom rows: they are
// copied inside LDS (bwd_halo_copy) and the stream starts at tile row 2.
template <int C, int W, int BR, bool EULER>
struct BwdPrefetch {
  using L = BwdLds<C, W, BR>;
  static constexpr int IPR = W / Geo<C>::PPI, ROWB = (W + 2) * (C / 8) * 16;
  int n, gy0, nrows, ni, end;
  unsigned char *dyt, *xt, *mt;
  __device__ __forceinline__ void init(const ItemCursor& nx, bool active, bool reuse, unsigned char* lds, int buf, int H) {
    const int y0 = nx.b * BR, r0 = reuse ? 2 : 0;
    n = nx.n;
    gy0 = y0 - 1 + r0;
    nrows = min(BR, H - y0) + 2 - r0;
    ni = nrows * IPR;
    dyt = lds + L::DY + buf * L::TILE + r0 * ROWB;
    xt = lds + L::X + buf * L::TILE + r0 * ROWB;
    mt = lds + L::MSK + buf * L::MTB + r0 * L::RBM;
    end = active ? 2 * ni + (EULER ? (nrows * L::RBM + 1023) / 1024 : 0) : 0;
  }
  __device__ __forceinline__ void issue(int u, const bf16* dy, const bf16* x, const uint8_t* mask, int H, unsigned loff,
                                        int lane) const {
    if (u < ni)
      dma_row_instr<C, W>(dy, dyt, n, gy0, u, H, loff);
    else if (u < 2 * ni)
      dma_row_instr<C, W>(x, xt, n, gy0, u - ni, H, loff);
    else
      dma_mask_instr<C, W>(mask, mt, n, gy0, nrows, u - 2 * ni, H, lane);
  }
};

// tile rows BR, BR+1 of this band's dy/x tiles and mask rows -> rows 0, 1 of
// the next band's buffers (all threads; asm LDS accesses, see lds_rd128)
template <int C, int W, int BR, bool EULER>
__device__ __forceinline__ void bwd_halo_copy(unsigned char* lds, int buf, int tid, int nthreads) {
  using L = BwdLds<C, W, BR>;
  constexpr int ROWB = (W + 2) * (C / 8) * 16, NR = 2 * ROWB / 16, NM = EULER ? 2 * L::RBM / 16 : 0;
  constexpr int TOT = 2 * NR + NM, KB = (TOT + 511) / 512;
  const unsigned base = lds_u32(lds);
  u32x4 v[KB];
  unsigned dst[KB];
#pragma unroll
  for (int k = 0; k < KB; ++k) {
    const int c = tid + k * nthreads;
    const int cc = c < TOT ? c : 0;
    unsigned src;
    if (cc < NR) {
      src = L::DY + buf * L::TILE + BR * ROWB + cc * 16;
      dst[k] = L::DY + (buf ^ 1) * L::TILE + cc * 16;
    } else if (cc < 2 * NR) {
      src = L::X + buf * L::TILE + BR * ROWB + (cc - NR) * 16;
      dst[k] = L::X + (buf ^ 1) * L::TILE + (cc - NR) * 16;
    } else {
      src = L::MSK + buf * L::MTB + BR * L::RBM + (cc - 2 * NR) * 16;
      dst[k] = L::MSK + (buf ^ 1) * L::MTB + (cc - 2 * NR) * 16;
    }
    v[k] = lds_rd128(base + src);
  }
  lgkm_wait<0>();
#pragma unroll
  for (int k = 0; k < KB; ++k)
    if (tid + k * nthreads < TOT) lds_wr128(base + dst[k], v[k]);
}

template <int C, int W, int BR, bool EULER>
__device__ __forceinline__ void bwd_issue(const bf16* dy, const bf16* x, const uint8_t* mask, unsigned char* lds,
                                          int buf, int n, int y0, int H, int wave, int lane, int nwaves) {
  using L = BwdLds<C, W, BR>;
  const int nr = min(BR, H - y0) + 2;
  dma_rows<C, W>(dy, lds + L::DY + buf * L::TILE, n, y0 - 1, nr, H, wave, nwaves, lane);
  dma_rows<C, W>(x, lds + L::X + buf * L::TILE, n, y0 - 1, nr, H, wave, nwaves, lane);
  if constexpr (EULER) dma_mask_rows<C, W>(mask, lds + L::MSK + buf * L::MTB, n, y0 - 1, nr, H, wave, nwaves, lane);
}

// dzm = dy * mask for all staged rows, into the DZ tile: a bit operation on
// the bf16 values (the factor h of dz = h*dy*mask is applied in fp32 in the
// epilogues: dx, dW and db are linear in dz).  Interior columns only (the DZ
// tile's halo columns are zeroed once per launch), so chunk c of the band is
// (row, col, q) by shifts and its mask byte is byte c of the staged mask
// rows.  LDS accesses through asm (see lds_rd128): the dgrad waves run this
// with the next band's DMA in flight.
template <int C, int W, int BR, bool EULER>
__device__ __forceinline__ void bwd_convert(unsigned char* lds, int buf, int nr, int tid, int nthreads) {
  using L = BwdLds<C, W, BR>;
  constexpr int TW = W + 2, NQ = C / 8, KB = 4;
  static_assert((NQ & (NQ - 1)) == 0 && (W & (W - 1)) == 0, "power-of-two chunk decomposition");
  const unsigned dyt = lds_u32(lds + L::DY + buf * L::TILE);
  const unsigned mt = lds_u32(lds + L::MSK + buf * L::MTB);
  const unsigned dzt = lds_u32(lds + L::DZ);
  const int nch = nr * W * NQ;
  for (int c0 = tid; c0 < nch; c0 += KB * nthreads) {
    u32x4 v[KB];
    unsigned mb[KB];
    unsigned off[KB];
#pragma unroll
    for (int k = 0; k < KB; ++k) {  // all LDS reads first (latencies overlap)
      const int c = c0 + k * nthreads;
      const int cc = c < nch ? c : 0;
      const int q = cc & (NQ - 1), col = 1 + ((cc / NQ) & (W - 1)), r = cc / (NQ * W);
      off[k] = (unsigned)toff<C>(r, col, q, TW);
      v[k] = lds_rd128(dyt + off[k]);
      if constexpr (EULER) mb[k] = lds_rd_u8(mt + (unsigned)cc);
    }
    lgkm_wait<0>();
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      if (c0 + k * nthreads < nch) {
        u32x4 z = v[k];
        if constexpr (EULER) {
#pragma unroll
          for (int d = 0; d < 4; ++d) {  // element pair (2d, 2d+1) of this 16-byte chunk
            const unsigned lo = (unsigned)__builtin_amdgcn_sbfe((int)mb[k], 2 * d, 1);
            const unsigned hi = (unsigned)__builtin_amdgcn_sbfe((int)mb[k], 2 * d + 1, 1);
            z[d] &= __builtin_amdgcn_perm(hi, lo, 0x07060100u);  // bytes 0-1 of lo, 2-3 of hi
          }
        }
        lds_wr128(dzt + off[k], z);
      }
    }
  }
}

template <int C, int W, int BR, int MODE, bool XT>
__global__ __launch_bounds__(512) void k_bwd(const bf16* __restrict__ dy, const bf16* __restrict__ x,
                                             const uint8_t* __restrict__ mask, const bf16* __restrict__ wpack,
                                             float h, float two_gamma, int N, int H, bf16* __restrict__ dx,
                                             float* __restrict__ slabs, const bf16* __restrict__ extra,
                                             int skip_dy, int accum) {
  using G = Geo<C>;
  using L = BwdLds<C, W, BR>;
  constexpr int TW = W + 2, PT = W / 16, NQ = G::NQ, OTW = G::OTW, OT = G::OT, MTW = G::MTW;
  constexpr int KPR = W / 32;
  constexpr bool EULER = MODE == BWD_EULER;
  static_assert(W % 32 == 0, "wgrad k-steps are 32 pixels of one row");
  // XT: the RK2 variant (extra dx term and/or no +dy residual); compiled out
  // of the Euler block's kernel
  const bool has_extra = XT && extra != nullptr;
  const bool no_dy = XT && skip_dy != 0;
  // XT && accum: add to the slab this WG's slot already holds (the RK2 first
  // stage onto the second stage's slabs: same grid, so one slab set per block)
  const bool acc_slab = XT && accum != 0;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, lx = lane & 15;

  for (int b = 0; b < 2; ++b) {
    zero_halo_cols<C, W>(lds + L::DY + b * L::TILE, BR + 2, tid, 512);
    zero_halo_cols<C, W>(lds + L::X + b * L::TILE, BR + 2, tid, 512);
  }
  zero_halo_cols<C, W>(lds + L::DZ, BR + 2, tid, 512);
  const int nb = (H + BR - 1) / BR;
  int i0, i1;
  item_range(N * nb, &i0, &i1);
  if (i0 < i1) {
    const ItemCursor c0(i0, nb);
    bwd_issue<C, W, BR, EULER>(dy, x, mask, lds, 0, c0.n, c0.b * BR, H, wave, lane, 8);
  }

  float* slab = slabs + (long)blockIdx.x * (9 * C * C + C);
  const float hs = EULER ? h : 1.f;  // dz = hs * dzm (dzm = dy*mask in LDS)
  const float hs2g = hs * two_gamma;
  if (wave < 4) {
    // ---------------- dgrad waves ----------------
    constexpr int RS = 4 / G::OSPLIT;
    const int oh = wave % G::OSPLIT, rg = wave / G::OSPLIT;
    const int wv4 = __builtin_amdgcn_readfirstlane(wave);
    const unsigned loff = (unsigned)dma_lane_off<C, W>(lane) * 2u;
    bf16x8 A[OTW][G::KS];
    load_A<C>(wpack, oh, lane, A);
    Frag<C, W> boff;
    boff.init(g, lx);
    float dbacc[OTW][4];  // db partial for channels 16*(oh*OTW+t) + 4g + e over this lane's pixels
#pragma unroll
    for (int t = 0; t < OTW; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) dbacc[t][e] = 0.f;
    int nst = 0;
    // the extra dx term (RK2: the outer dy of the first stage): each dgrad
    // wave DMAs the rows it needs into its private LDS rows after its last
    // epilogue of the previous band (prologue: before the loop), so it is
    // older than the next band's prefetch and vm_wait(nd) covers it
    using LX = BwdLds<C, W, BR>;
    constexpr int MR = LX::MR, NEX = MR * LX::ROWX / 1024;
    unsigned char* priv = lds + LX::EXT + wave * MR * LX::ROWX;
    if (has_extra && i0 < i1) {
      const ItemCursor c0(i0, nb);
      dma_extra<C, W, BR>(extra, priv, c0.n, c0.b * BR, min(BR, H - c0.b * BR), H, rg, oh, lane);
      nst = NEX;
    }
    ItemCursor cur(i0, nb), nxt(i0, nb);
    nxt.next(nb);
    for (int it = i0; it < i1; ++it, cur.next(nb), nxt.next(nb)) {
      const int buf = (it - i0) & 1;
      const int n = cur.n, y0 = cur.b * BR;
      const int rows = min(BR, H - y0);
      ASR_STAMP(it - i0, 0);
      barrier_vm(nst);  // item's DMA landed; previous item fully consumed
      ASR_STAMP(it - i0, 1);
      nst = 0;
      // prefetch of band it+1: dy rows, x rows, mask chunks as one stream of
      // instructions dealt round-robin to all 8 waves; a dgrad wave issues
      // its share one per k-step of its first dgrad row (so the issue cost
      // overlaps MFMAs), the rest flushed before that row's epilogue
      int nd = 0;  // prefetch instructions this wave issued
      const bool reuse = it + 1 < i1 && nxt.n == cur.n;
      BwdPrefetch<C, W, BR, EULER> pf;
      pf.init(nxt, it + 1 < i1, reuse, lds, buf ^ 1, H);
      const int dsplit = (pf.end * kBwdDgradDmaPct) / 100;  // dgrad waves: [0, dsplit)
      int du = wv4;                                               // wave-uniform stream cursor
      const int dend = dsplit;
      auto dma_one = [&]() {
        if (du < dend) {
          pf.issue(du, dy, x, mask, H, loff, lane);
          du += 4;
          nst = 0;  // the next barrier waits for this prefetch; stores issued after it need not finish
          ++nd;
        }
      };
      bool ex_wait = has_extra;
      if (reuse) bwd_halo_copy<C, W, BR, EULER>(lds, buf, tid, 512);
      bwd_convert<C, W, BR, EULER>(lds, buf, rows + 2, tid, 512);
      ASR_STAMP(it - i0, 2);
      barrier_lds();  // dz ready
      ASR_STAMP(it - i0, 3);
      const unsigned char* dzt = lds + L::DZ;
      const unsigned char* dyt = lds + L::DY + buf * L::TILE;
#pragma unroll
      for (int k = 0; k < MR; ++k) {
        const int r = rg + k * RS;
        if (r >= rows) break;
        f32x4 acc[OTW][PT];
#pragma unroll
        for (int t = 0; t < OTW; ++t)
#pragma unroll
          for (int pt = 0; pt < PT; ++pt) acc[t][pt] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (k == 0) {
          conv_row<C, W>(dzt, r, A, boff, acc, dma_one);
          while (du < dend) dma_one();
          ASR_STAMP(it - i0, 4);
        } else {
          conv_row<C, W>(dzt, r, A, boff, acc);
        }
        const int gy = y0 + r;
        if (dx) nst += PT * OTW;
        u32x2 dzv[PT][OTW], dyv[PT][OTW];
#pragma unroll
        for (int pt = 0; pt < PT; ++pt)
#pragma unroll
          for (int t = 0; t < OTW; ++t) {
            const int px = 16 * pt + lx, o0 = 16 * (oh * OTW + t) + 4 * g;
            const int co = toff<C>(r + 1, px + 1, o0 >> 3, TW) + (o0 & 4) * 2;
            dzv[pt][t] = lds_rd64(lds_u32(dzt + co));
            if (EULER && !no_dy) dyv[pt][t] = lds_rd64(lds_u32(dyt + co));
          }
        lgkm_wait<0>();
        if (ex_wait) {
          vm_wait(nd);  // this wave's private extra rows (older than the next band's prefetch)
          ex_wait = false;
        }
#pragma unroll
        for (int pt = 0; pt < PT; ++pt) {
          const int px = 16 * pt + lx;
#pragma unroll
          for (int t = 0; t < OTW; ++t) {
            const int o0 = 16 * (oh * OTW + t) + 4 * g;
            const bf16x4 dzr = *(const bf16x4*)&dzv[pt][t];
            float dzf[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              dzf[e] = (float)dzr[e];
              dbacc[t][e] += dzf[e];
            }
            // residual terms: dy (unless skip_dy) + extra
            float res[4] = {0.f, 0.f, 0.f, 0.f};
            if (EULER && !no_dy) {
              const bf16x4 dyr = *(const bf16x4*)&dyv[pt][t];
#pragma unroll
              for (int e = 0; e < 4; ++e) res[e] = (float)dyr[e];
            }
            if (has_extra) {
              constexpr int PXG = 64 / (LX::NCH * 4);
              const int px = 16 * pt + lx;
              const unsigned a = lds_u32(priv + k * LX::ROWX + px * LX::NCH * 16 +
                                         (((2 * t + (g >> 1)) ^ ((px / PXG) % LX::NCH)) * 16) + (g & 1) * 8);
              u32x2 ev = lds_rd64(a);
              lgkm_wait<0>();
              const bf16x4 exr = *(const bf16x4*)&ev;
#pragma unroll
              for (int e = 0; e < 4; ++e) res[e] += (float)exr[e];
            }
            bf16x4 o4;
            if constexpr (EULER) {
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const float v = fmaf(-hs, acc[t][pt][e], res[e]);
                o4[e] = (bf16)(hs2g != 0.f ? fmaf(hs2g, dzf[e], v) : v);
              }
            } else {
#pragma unroll
              for (int e = 0; e < 4; ++e) o4[e] = (bf16)(fmaf(two_gamma, dzf[e], -acc[t][pt][e]) + res[e]);
            }
            if (dx) *(bf16x4*)(dx + (((long)n * H + gy) * W + px) * C + o0) = o4;
          }
        }
        ASR_STAMP(it - i0, 5 + k);
      }
      while (du < dend) dma_one();  // a wave without rows in this band
      if (has_extra && it + 1 < i1) {  // next band's extra rows into the (now read) private rows
        dma_extra<C, W, BR>(extra, priv, nxt.n, nxt.b * BR, min(BR, H - nxt.b * BR), H, rg, oh, lane);
        nst += NEX;
      }
    }
    // reduce db over the 16 pixel lanes, then over the row-group waves (LDS)
#pragma unroll
    for (int t = 0; t < OTW; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v = dbacc[t][e];
        v += __shfl_xor(v, 1);
        v += __shfl_xor(v, 2);
        v += __shfl_xor(v, 4);
        v += __shfl_xor(v, 8);
        dbacc[t][e] = v;
      }
    barrier_vm(0);  // matches the wgrad waves' end-of-loop barrier
    float* dbl = (float*)lds + 12288;  // [RS][C], past the K-split scratch
    if (lx == 0) {
#pragma unroll
      for (int t = 0; t < OTW; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) dbl[rg * C + 16 * (oh * OTW + t) + 4 * g + e] = hs * dbacc[t][e];
    }
    if constexpr (G::KSPLIT > 1) {
      __syncthreads();
      __syncthreads();
    }
  } else {
    // ---------------- wgrad waves ----------------
    const int w4 = wave - 4;
    const int tg = w4 % G::TG, kg = w4 / G::TG;
    const int tq = lx >> 2, tp = lx & 3;
    f32x4 acc[MTW][OT];
#pragma unroll
    for (int mi = 0; mi < MTW; ++mi)
#pragma unroll
      for (int ot = 0; ot < OT; ++ot) acc[mi][ot] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int wv8 = __builtin_amdgcn_readfirstlane(wave);
    const unsigned loff = (unsigned)dma_lane_off<C, W>(lane) * 2u;
    ItemCursor cur(i0, nb), nxt(i0, nb);
    nxt.next(nb);
    for (int it = i0; it < i1; ++it, cur.next(nb), nxt.next(nb)) {
      const int buf = (it - i0) & 1;
      const int y0 = cur.b * BR;
      const int rows = min(BR, H - y0);
      ASR_STAMP(it - i0, 0);
      barrier_vm(0);  // this wave's share of the band's prefetch landed (no stores in flight)
      ASR_STAMP(it - i0, 1);
      // this wave's share of band it+1's prefetch (see the dgrad waves),
      // issued after the dz barrier, while the dgrad wave on this SIMD runs
      // its MFMAs
      const bool reuse = it + 1 < i1 && nxt.n == cur.n;
      BwdPrefetch<C, W, BR, EULER> pf;
      pf.init(nxt, it + 1 < i1, reuse, lds, buf ^ 1, H);
      int du = (pf.end * kBwdDgradDmaPct) / 100 + wv8 - 4;  // wgrad waves: [dsplit, end)
      const int dend = pf.end;
      auto dma_one = [&]() {
        if (du < dend) {
          pf.issue(du, dy, x, mask, H, loff, lane);
          du += 4;
        }
      };
      if (reuse) bwd_halo_copy<C, W, BR, EULER>(lds, buf, tid, 512);
      bwd_convert<C, W, BR, EULER>(lds, buf, rows + 2, tid, 512);
      ASR_STAMP(it - i0, 2);
      barrier_lds();
      ASR_STAMP(it - i0, 3);
      while (du < dend) dma_one();
      ASR_STAMP(it - i0, 4);
      const unsigned char* dzt = lds + L::DZ;
      const unsigned char* xt = lds + L::X + buf * L::TILE;
      for (int kk = kg; kk < rows * KPR; kk += G::KSPLIT) {
        const int r = kk / KPR, kb = kk % KPR;
        const int pb = 32 * kb + 8 * g + tq;
        auto loadA = [&](int mi) {
          const int mt = tg * MTW + mi;
          const int tap = (16 * mt) / C, itile = ((16 * mt) % C) / 16;
          const int ky = tap / 3, kx = tap % 3;
          const int q = 2 * itile + (tp >> 1);
          return tr_pair(xt + toff<C>(r + ky, pb + kx, q, TW) + 8 * (tp & 1),
                         xt + toff<C>(r + ky, pb + 4 + kx, q, TW) + 8 * (tp & 1));
        };
        bf16x8 Bf[OT];
#pragma unroll
        for (int ot = 0; ot < OT; ++ot) {
          const int q = 2 * ot + (tp >> 1);
          Bf[ot] = tr_pair(dzt + toff<C>(r + 1, pb + 1, q, TW) + 8 * (tp & 1),
                           dzt + toff<C>(r + 1, pb + 5, q, TW) + 8 * (tp & 1));
        }
        bf16x8 Ac = loadA(0), An;
#pragma unroll
        for (int mi = 0; mi < MTW; ++mi) {
          if (mi + 1 < MTW) An = loadA(mi + 1);
#pragma unroll
          for (int ot = 0; ot < OT; ++ot)
            acc[mi][ot] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ac, Bf[ot], acc[mi][ot], 0, 0, 0);
          if (mi + 1 < MTW) Ac = An;
        }
      }
      ASR_STAMP(it - i0, 5);
    }
    barrier_vm(0);  // all items consumed: LDS reusable
    float* red = (float*)lds;
    if constexpr (G::KSPLIT > 1) {
      if (kg > 0) {
#pragma unroll
        for (int mi = 0; mi < MTW; ++mi)
#pragma unroll
          for (int ot = 0; ot < OT; ++ot)
#pragma unroll
            for (int e = 0; e < 4; ++e)
              red[((((kg - 1) * G::TG + tg) * MTW + mi) * OT + ot) * 256 + e * 64 + lane] = acc[mi][ot][e];
      }
      __syncthreads();
      if (kg == 0) {
        for (int k2 = 1; k2 < G::KSPLIT; ++k2)
#pragma unroll
          for (int mi = 0; mi < MTW; ++mi)
#pragma unroll
            for (int ot = 0; ot < OT; ++ot)
#pragma unroll
              for (int e = 0; e < 4; ++e)
                acc[mi][ot][e] += red[((((k2 - 1) * G::TG + tg) * MTW + mi) * OT + ot) * 256 + e * 64 + lane];
      }
      __syncthreads();
    }
    if (kg == 0) {
      // acc_slab: the old values of MC m-tiles loaded before their first
      // store (one latency per chunk, not one per element: the compiler keeps
      // load/store pairs to the slab in order)
      constexpr int MC = MTW % 3 == 0 ? 3 : 1;
#pragma unroll
      for (int m0 = 0; m0 < MTW; m0 += MC) {
        float prev[MC][OT][4];
#pragma unroll
        for (int mi = 0; mi < MC; ++mi)
#pragma unroll
          for (int ot = 0; ot < OT; ++ot)
#pragma unroll
            for (int e = 0; e < 4; ++e)
              prev[mi][ot][e] =
                  acc_slab ? slab[(long)(16 * (tg * MTW + m0 + mi) + 4 * g + e) * C + 16 * ot + lx] : 0.f;
#pragma unroll
        for (int mi = 0; mi < MC; ++mi)
#pragma unroll
          for (int ot = 0; ot < OT; ++ot)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int m = 16 * (tg * MTW + m0 + mi) + 4 * g + e;
              slab[(long)m * C + 16 * ot + lx] = fmaf(hs, acc[m0 + mi][ot][e], prev[mi][ot][e]);
            }
      }
    }
  }
  __syncthreads();
  if (tid < C) {
    const float* dbl = (const float*)lds + 12288;
    float s = 0.f;
    for (int q = 0; q < 4 / G::OSPLIT; ++q) s += dbl[q * C + tid];
    slab[9 * C * C + tid] = acc_slab ? slab[9 * C * C + tid] + s : s;
  }
}

// ===========================================================================
// The v2 band protocol (C=64, W=32, BR=4), which k_bwd3 and k_bwd3_stack run
// (the v2 kernel itself is gone).  The dz = dy*mask conversion of band it+1 runs on the
// dgrad waves at the end of band it, while the wgrad waves still run band
// it's MFMAs (v1 converts on all 8 waves between two barriers, with the MFMA
// pipe idle).  dy, x and dz tiles are double-buffered (6 tiles, 153 KiB);
// the relu mask goes to registers, not LDS.  Each dgrad wave owns whole
// tile rows of the next band: it DMAs their dy, loads their mask dwords and
// converts them, so its own vmcnt covers everything it converts and no
// cross-wave wait is needed before the band barrier.  The wgrad waves DMA
// the next band's x rows and, after their MFMAs, copy the halo rows of a
// band that continues the previous band's image (dz rows 0,1 already
// masked, x rows 0,1, dy row 1 = the residual's first interior row).
// ===========================================================================
template <int C, int W, int BR>
struct Bwd2Lds {
  static constexpr int ROWB = (W + 2) * (C / 8) * 16;
  static constexpr int TILE = (BR + 2) * ROWB;
  static constexpr int DY = 0, X = 2 * TILE, DZ = 4 * TILE;
  // 256 x 16 B: the 16-bit-lane AND masks of one 16-B chunk per mask byte
  static constexpr int MTAB = 6 * TILE, TOTAL = MTAB + 4096;
};

// tile rows of band `nx` owned by dgrad wave wv (0..3): reuse -> row 2+wv;
// else rows wv and wv+4 (wv < 2)
struct Bwd2Own {
  int ra, rb;  // rb < 0: one row
  __device__ __forceinline__ Bwd2Own(bool reuse, int wv) {
    ra = reuse ? 2 + wv : wv;
    rb = (!reuse && wv < 2) ? wv + 4 : -1;
  }
  __device__ __forceinline__ int count() const { return rb < 0 ? 1 : 2; }
  __device__ __forceinline__ int row(int k) const { return k == 0 ? ra : rb; }
};

// mask dword of lane (pixel lane&31, channel half lane>>5) of tile row r of
// band (n, y0): bytes 8*px + 4*h .. +3 of the image row (zeros outside)
template <int C, int W>
__device__ __forceinline__ unsigned bwd2_mask_word(const uint8_t* __restrict__ mask, int n, int y0, int r, int H,
                                                   int lane) {
  const int gy = y0 - 1 + r;
  if ((unsigned)gy >= (unsigned)H) return 0u;
  return *(const unsigned*)(mask + ((long)n * H + gy) * (W * C / 8) + (2 * (lane & 31) + (lane >> 5)) * 4);
}


// ===========================================================================
// Backward v3 (C=64, W=32, BR=4): the round-1 v2 backward's band protocol (double-buffered
// dy / x / dz tiles, the next band's dz converted by the dgrad waves from
// their own dy rows, x DMA + halo copy by the wgrad waves, the previous
// block's slab pass folded in) at three waves per SIMD (12 waves, <= 168
// VGPRs):
//   waves 0-3  dgrad, one 16-channel o-tile each over the whole band (the
//              forward's band conv on the dz tile: A 72 VGPRs), epilogue on
//              the regrouped accumulators (16-B dy / dz / x chunk reads, one
//              16-B dx store per row, db over 8 channels per lane);
//   waves 4-11 wgrad, m-tile group tg = (w-4)/2 (9 m-tiles) x o-tiles
//              2*((w-4)&1) + 0..1: 72 accumulator VGPRs, 18 MFMAs per k-step.
// dW sums the pixels of a row in a bank-conflict-free permutation, dx the taps
// in the band conv's order, db on MFMA.
// ===========================================================================
template <int C, int W, int BR, int MODE, bool RO, bool XT = false>
__global__ __launch_bounds__(768, 1) void k_bwd3(const bf16* __restrict__ dy, const bf16* __restrict__ x,
                                                 const uint8_t* __restrict__ mask, const bf16* __restrict__ wpack,
                                                 float h, float two_gamma, int N, int H, bf16* __restrict__ dx,
                                                 float* __restrict__ slabs, const float* __restrict__ pslabs, int pP,
                                                 float* __restrict__ pgrp, int skip_dy,
                                                 const bf16* __restrict__ extra = nullptr) {
  using G = Geo<C>;
  using L = Bwd2Lds<C, W, BR>;
  using BD = Band<C, W, BR>;
  constexpr int TW = W + 2, OT = G::OT, MTW = G::MTW, IPR = W / G::PPI, NQ = G::NQ;
  constexpr bool EULER = MODE == BWD_EULER;
  static_assert(C == 64 && W == 32 && BR == 4 && MTW == 9 && OT == 4, "v3 backward geometry");
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, lx = lane & 15;

  for (int b = 0; b < 2; ++b) {
    zero_halo_cols<C, W>(lds + L::DY + b * L::TILE, BR + 2, tid, 768);
    zero_halo_cols<C, W>(lds + L::X + b * L::TILE, BR + 2, tid, 768);
    zero_halo_cols<C, W>(lds + L::DZ + b * L::TILE, BR + 2, tid, 768);
  }
  if (EULER) {  // dword d of byte m's entry: 0xffff per set bit of (m >> 2d) & 3
    unsigned* tab = (unsigned*)(lds + L::MTAB);
    for (int i = tid; i < 1024; i += 768) {
      const unsigned m = (unsigned)i >> 2, d = (unsigned)i & 3;
      tab[i] = (((m >> (2 * d)) & 1u) ? 0xffffu : 0u) | (((m >> (2 * d + 1)) & 1u) ? 0xffff0000u : 0u);
    }
  }
  const int nb = (H + BR - 1) / BR;
  int i0, i1;
  item_range(N * nb, &i0, &i1);
  const unsigned loff = (unsigned)dma_lane_off<C, W>(lane) * 2u;
  float* slab = slabs + (long)blockIdx.x * (9 * C * C + C);
  const float hs = EULER ? h : 1.f;  // dz = hs * dzm (dzm = dy*mask in LDS)
  const float hs2g = hs * two_gamma;
  __syncthreads();  // halo columns zeroed before any convert / copy writes near them
  ASR_BCLK(1, 0);

  // pass 1 of the previous block's slab reduction (as in the round-1 v2 backward), on the wgrad
  // waves only: thread ft = tid - 256 owns one 16-B chunk of one group row
  constexpr int ES = 9 * C * C + C, ECH = ES / 4;
  const int ft = tid - 256;
  const long fT = (long)((pP + 31) / 32) * ECH;
  const long fc0 = (long)blockIdx.x * fT / gridDim.x, fc1 = (long)(blockIdx.x + 1) * fT / gridDim.x;
  const bool fold = pP > 0 && ft >= 0 && fc0 + ft < fc1;
  const int fg = fold ? (int)((fc0 + ft) / ECH) : 0;
  const int fpe = min(pP, 32 * fg + 32);
  int fp = 32 * fg;
  unsigned foff = fold ? (unsigned)fp * ES + (unsigned)((fc0 + ft) % ECH) * 4 : 0u;
  f32x4 facc = {0.f, 0.f, 0.f, 0.f}, fv[2];

  if (wave < 4) {
    // ---------------- dgrad waves ----------------
    const int ot = wave;
    bf16x8 A[G::KS];
    load_A1<C>(wpack, ot, lane, A);
    unsigned lo[3 * BD::NCB];
    band_lane_offsets<C, W, BR>(g, lx, lo);
    const int px = lx + 16 * (g & 1), cg = 2 * ot + (g >> 1);  // regrouped: pixel, 16-B channel chunk
    const unsigned lch = (unsigned)toff<C>(1, px + 1, cg, TW);  // output row 0's chunk in a tile
    const unsigned ldx = (unsigned)(px * C + 8 * cg) * 2u;
    int nst = 0;
    ItemCursor cur(i0, nb);
    for (int it = i0; it < i1; ++it, cur.next(nb)) {
      const int buf = (it - i0) & 1;
      const int n = cur.n, y0 = cur.b * BR;
      const int rows = min(BR, H - y0);
      if (wave == 0) ASR_BTR(1, 0, it - i0, 0);
      barrier_vm_usual<BR>(nst);  // band it staged everywhere; band it-1 fully consumed
      if (wave == 0) ASR_BTR(1, 0, it - i0, 1);
      // XT: the extra dx term of the band's rows (in flight during the conv)
      u32x4 exv[XT ? BR : 1];
      if constexpr (XT) {
        const bf16* eb = extra + ((long)n * H + y0) * W * C;
#pragma unroll
        for (int r = 0; r < BR; ++r) {
          const int rr = min(r, rows - 1);
          exv[r] = *(const u32x4*)((const unsigned char*)(eb + (long)rr * W * C) + ldx);
        }
      }
      const unsigned dzt = lds_u32(lds + L::DZ + buf * L::TILE), dyt = lds_u32(lds + L::DY + buf * L::TILE);
      const unsigned xt = lds_u32(lds + L::X + buf * L::TILE);
      f32x4 acc[BR][2];
#pragma unroll
      for (int r = 0; r < BR; ++r) acc[r][0] = acc[r][1] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (wave == 0) ASR_BTR(1, 0, it - i0, 2);
      conv_band<C, W, BR>(dzt, lo, A, acc);
      if (wave == 0) ASR_BTR(1, 0, it - i0, 3);
      // epilogue, LDS reads one row ahead: dy (the residual), dz only for the
      // 2*gamma*dz term (gamma != 0), x for RO; the flags are compile-time in
      // each instantiation (a runtime flag costs selects on every element)
      bf16* drow = dx ? dx + ((long)n * H + y0) * W * C : nullptr;
      int nld = 0;
      auto epilogue = [&](auto g2c, auto skc) {
        constexpr bool G2 = decltype(g2c)::value, SKIP = decltype(skc)::value;
        constexpr bool RDY = EULER && !SKIP;
        constexpr int NR = (RDY ? 1 : 0) + (G2 ? 1 : 0) + (RO ? 1 : 0);  // LDS reads per row
        u32x4 dyw[2], dzw[2], xw[2];
        auto issue = [&](int r, int sl) {
          const unsigned co = lch + (unsigned)(r * L::ROWB);
          if constexpr (RDY) dyw[sl] = lds_rd128(dyt + co);
          if constexpr (G2) dzw[sl] = lds_rd128(dzt + co);
          if constexpr (RO) xw[sl] = lds_rd128(xt + co);
        };
        // reads of all BR tile rows on a compile-time schedule (rows past the image
        // read tile rows that exist and are not used), each retired before the row
        // guard: no branch between a read and its wait (see k_bwd3_stack)
        if constexpr (NR > 0) issue(0, 0);
        static_for<0, BR>([&](auto rc) {
          constexpr int r = decltype(rc)::value, sl = r & 1;
          if constexpr (NR > 0) {
            if constexpr (r + 1 < BR) {
              issue(r + 1, sl ^ 1);
              lgkm_wait<NR>();  // row r's reads (row r+1's still in flight)
            } else {
              lgkm_wait<0>();
            }
          }
          if (r < rows) {
            float z[8];
            regroup(acc[r][0], acc[r][1], z);
            u32x4 ow;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
              float v0, v1;
              if constexpr (EULER) {
                float r0 = 0.f, r1 = 0.f;
                if constexpr (RDY) r0 = lo_f(dyw[sl][d]), r1 = hi_f(dyw[sl][d]);
                if constexpr (XT) {
                  r0 += lo_f(exv[r][d]);
                  r1 += hi_f(exv[r][d]);
                }
                v0 = fmaf(-hs, z[2 * d], r0);
                v1 = fmaf(-hs, z[2 * d + 1], r1);
                if constexpr (G2) {
                  v0 = fmaf(hs2g, lo_f(dzw[sl][d]), v0);
                  v1 = fmaf(hs2g, hi_f(dzw[sl][d]), v1);
                }
              } else {
                v0 = -z[2 * d];
                v1 = -z[2 * d + 1];
                if constexpr (G2) {
                  v0 = fmaf(two_gamma, lo_f(dzw[sl][d]), v0);
                  v1 = fmaf(two_gamma, hi_f(dzw[sl][d]), v1);
                }
              }
              ow[d] = pk_bf16(v0, v1);
              if constexpr (RO) {  // bf16 x > 0: positive as a signed 16-bit integer
                const unsigned xd = xw[sl][d];
                ow[d] &= ((int)(short)(xd & 0xffffu) > 0 ? 0xffffu : 0u) | ((int)xd > 0xffff ? 0xffff0000u : 0u);
              }
            }
            if (drow) {
              *(u32x4*)((unsigned char*)(drow + (long)r * W * C) + ldx) = ow;
              ++nld;
            }
          }
        });
      };
      using T_ = std::true_type;
      using F_ = std::false_type;
      const bool g2 = hs2g != 0.f;
      if (EULER && skip_dy) {
        if (g2) epilogue(T_{}, T_{});
        else epilogue(F_{}, T_{});
      } else {
        if (g2) epilogue(T_{}, F_{});
        else epilogue(F_{}, F_{});
      }
      if (wave == 0) ASR_BTR(1, 0, it - i0, 4);
      if (wave == 0) ASR_BTR(1, 0, it - i0, 5);
      nst = nld;
    }
    barrier_vm(0);  // matches the wgrad waves' end-of-loop barrier
  } else {
    // ---------------- wgrad waves ----------------
    const int w8 = __builtin_amdgcn_readfirstlane(wave) - 4;
    const int tg = w8 >> 1, oq = 2 * (w8 & 1);  // m-tiles tg*9 .. +8, o-tiles oq, oq+1
    const int tq = lx >> 2, tp = lx & 3;
    f32x4 acc[MTW][2];
#pragma unroll
    for (int mi = 0; mi < MTW; ++mi) acc[mi][0] = acc[mi][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    // per-lane byte offsets (tile row 0) of the transposed fragment reads:
    // A = x at tap (ky, kx) of m-tile tg*9 + mi, B = dz of o-tile oq + oi (output row 0 = tile row 1)
    // LDS byte addresses in the current band's buffer (row r's r * ROWB is an immediate).
    // K = the row's 32 pixels, lane group g reading pixels 4g + tq and 4g + 16 + tq
    // (any pixel permutation shared by A and B gives the same GEMM): each 32-lane
    // half then reads 8 consecutive tile columns, whose swizzled 8-B pieces cover
    // the 64 banks once (pixels 8g + tq, 8g + 4 + tq, as the round-1 v2 backward read them, put
    // columns c and c + 8 on the same banks: every read 2-way)
    unsigned offA[MTW], offB[2];  // pixel tile 1 sits 16 px = 2 KiB on (swizzle period 8 px)
    {
      const unsigned xb0 = lds_u32(lds + L::X), zb0 = lds_u32(lds + L::DZ);
      const int pb = 4 * g + tq;
#pragma unroll
      for (int mi = 0; mi < MTW; ++mi) {
        const int mt = tg * MTW + mi;
        const int tap = (16 * mt) / C, itile = ((16 * mt) % C) / 16;
        const int ky = tap / 3, kx = tap % 3, q = 2 * itile + (tp >> 1);
        offA[mi] = xb0 + (unsigned)(toff<C>(ky, pb + kx, q, TW) + 8 * (tp & 1));
      }
#pragma unroll
      for (int oi = 0; oi < 2; ++oi) {
        const int q = 2 * (oq + oi) + (tp >> 1);
        offB[oi] = zb0 + (unsigned)(toff<C>(1, pb + 1, q, TW) + 8 * (tp & 1));
      }
      // opaque to the compiler: kept in VGPRs, not recomputed per band
#pragma unroll
      for (int mi = 0; mi < MTW; ++mi) asm volatile("" : "+v"(offA[mi]));
      asm volatile("" : "+v"(offB[0]), "+v"(offB[1]));
    }
    // the next band's dz: wgrad wave w8 owns tile row 2 + w8 (w8 < 4) of a band that
    // continues the image, row w8 (w8 < 6) of one that starts an image; it DMAs
    // that row's dy, loads its mask dwords and converts it (its own vmcnt covers both)
    auto own_row = [&](bool reuse) { return reuse ? (w8 < 4 ? 2 + w8 : -1) : (w8 < 6 ? w8 : -1); };
    auto stage_own = [&](const ItemCursor& c, int row, int nbuf, unsigned& mwv) {
      if (row < 0) return;
      if constexpr (EULER) mwv = bwd2_mask_word<C, W>(mask, c.n, c.b * BR, row, H, lane);
      for (int j = 0; j < IPR; ++j)
        dma_row_instr<C, W>(dy, lds + L::DY + nbuf * L::TILE + row * L::ROWB, c.n, c.b * BR - 1 + row, j, H, loff);
    };
    // dz = dy & mask of the own row (lane = pixel lane&31, chunks 4*(lane>>5) + j),
    // two chunks at a time, compiler-visible LDS accesses (this role's live state
    // leaves little room: a spilled inline-asm read result would be garbage)
    auto convert_own = [&](int row, int nbuf, unsigned mwv) {
      if (row < 0) return;
      const unsigned base = lds_u32(lds);
      const int cpx = lane & 31, hh = lane >> 5;
#pragma unroll
      for (int jj = 0; jj < 4; jj += 2) {
        u32x4 v[2], mt[2];
        unsigned off[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          off[j] = (unsigned)toff<C>(row, cpx + 1, 4 * hh + jj + j, TW) + (unsigned)(nbuf * L::TILE);
          v[j] = lds_ld128(base + L::DY + off[j]);
          if (EULER) mt[j] = lds_ld128(base + L::MTAB + __builtin_amdgcn_ubfe(mwv, 8 * (jj + j), 8) * 16);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          u32x4 z = v[j];
          if constexpr (EULER) {
            z &= mt[j];
          } else if constexpr (EULER) {
#pragma unroll
            for (int d = 0; d < 4; ++d) {
              const unsigned lo = (unsigned)__builtin_amdgcn_sbfe((int)mwv, 8 * (jj + j) + 2 * d, 1);
              const unsigned hi = (unsigned)__builtin_amdgcn_sbfe((int)mwv, 8 * (jj + j) + 2 * d + 1, 1);
              z[d] &= __builtin_amdgcn_perm(hi, lo, 0x07060100u);
            }
          }
          lds_st128(base + L::DZ + off[j], z);
        }
      }
    };
    // db on MFMA (tile group 3): ones(16 x 32) x dz^T, every row of the result = db
    bf16x8 ones;
#pragma unroll
    for (int i = 0; i < 8; ++i) ones[i] = (bf16)1.0f;
    f32x4 accb[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    const bool dbw = tg == 3;
    if (i0 < i1) {  // prologue: dy rows (own) and x rows of band i0, its dz converted
      const ItemCursor c0(i0, nb);
      unsigned mw0 = 0u;
      const int row0 = own_row(false);
      stage_own(c0, row0, 0, mw0);
      for (int j = w8; j < (BR + 2) * IPR; j += 8) dma_row_instr<C, W>(x, lds + L::X, c0.n, c0.b * BR - 1, j, H, loff);
      // (the band loop's x DMA runs on waves w8 >= 4 only: waves 0-3 DMA the own dy rows)
      vm_wait(0);
      convert_own(row0, 0, mw0);
    }
    ItemCursor cur(i0, nb), nxt(i0, nb);
    nxt.next(nb);
    for (int it = i0; it < i1; ++it, cur.next(nb), nxt.next(nb)) {
      const int buf = (it - i0) & 1;
      const int y0 = cur.b * BR;
      const int rows = min(BR, H - y0);
      if (wave == 4) ASR_BTR(1, 1, it - i0, 0);
      barrier_vm(0);  // this wave's x rows of band it landed
      if (wave == 4) ASR_BTR(1, 1, it - i0, 1);
#pragma unroll
      for (int q = 0; q < 2; ++q)
        if (fold && fp + q < fpe) fv[q] = *(const f32x4*)(pslabs + foff + (unsigned)q * ES);
      const bool more = it + 1 < i1;
      const int orow = more ? own_row(nxt.n == cur.n) : -1;
      unsigned mwv = 0u;
      // the next band's DMA pieces of this wave: own dy row (waves 0-3, or 0-5 when
      // the next band starts an image), x rows (waves 4-7; rows 2.. when it
      // continues this band's image); the first kBwd3Dma0 pieces issued here, the
      // rest after the band's MFMAs (below; the per-row interleave among the MFMAs
      // went with the round-5 cleanup d41213d, and this per-block path's speed was
      // not re-measured: the networks run the stacked kernels)
      if constexpr (EULER) {
        if (orow >= 0) mwv = bwd2_mask_word<C, W>(mask, nxt.n, nxt.b * BR, orow, H, lane);
      }
      const int xr0 = nxt.n == cur.n ? 2 : 0;
      const int ndy = orow >= 0 ? IPR : 0;
      const int nx = (more && w8 >= 4) ? ((BR + 2 - xr0) * IPR - (w8 - 4) + 3) / 4 : 0;
      const int npc = ndy + nx;
      int ipc = 0;
      auto piece = [&]() {
        if (ipc < ndy) {
          dma_row_instr<C, W>(dy, lds + L::DY + (buf ^ 1) * L::TILE + orow * L::ROWB, nxt.n, nxt.b * BR - 1 + orow,
                              ipc, H, loff);
        } else {
          dma_row_instr<C, W>(x, lds + L::X + (buf ^ 1) * L::TILE + xr0 * L::ROWB, nxt.n, nxt.b * BR - 1 + xr0,
                              (w8 - 4) + 4 * (ipc - ndy), H, loff);
        }
        ++ipc;
      };
      while (ipc < npc && ipc < kBwd3Dma0) piece();
      bf16x8 Bf[2], Ar[3];
      if (wave == 4) ASR_BTR(1, 1, it - i0, 2);
      // A fragments two m-tiles ahead (ring of 3), as in the round-1 v2 backward
      auto mfma_band = [&](auto bo) {
        constexpr int BO = decltype(bo)::value;
        Ar[0] = tr_pair_px<BO>(offA[0]);
        static_for<0, BR>([&](auto rc) {
          constexpr int r = decltype(rc)::value, RO_ = BO + r * L::ROWB;
          __builtin_amdgcn_sched_barrier(0);  // no hoisting of later rows' reads (register pressure)
          if (r < rows) {
            const bool mr = r + 1 < rows;
#pragma unroll
            for (int oi = 0; oi < 2; ++oi) Bf[oi] = tr_pair_px<RO_>(offB[oi]);
            Ar[1] = tr_pair_px<RO_>(offA[1]);
            static_for<0, MTW>([&](auto mc) {
              constexpr int mi = decltype(mc)::value;
              if constexpr (mi + 2 < MTW) Ar[(mi + 2) % 3] = tr_pair_px<RO_>(offA[mi + 2]);
              else if constexpr (mi + 2 == MTW && r + 1 < BR) {
                if (mr) Ar[0] = tr_pair_px<RO_ + L::ROWB>(offA[0]);  // MTW % 3 == 0: slot 0 again
              }
#pragma unroll
              for (int oi = 0; oi < 2; ++oi)
                acc[mi][oi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ar[mi % 3], Bf[oi], acc[mi][oi], 0, 0, 0);
            });
            if (dbw) {
#pragma unroll
              for (int oi = 0; oi < 2; ++oi)
                accb[oi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, Bf[oi], accb[oi], 0, 0, 0);
            }
          }
        });
      };
      if (it > i0) {  // the offsets follow the buffer (in place: no second register set)
        const unsigned dlt = buf ? (unsigned)L::TILE : (unsigned)-L::TILE;
#pragma unroll
        for (int mi = 0; mi < MTW; ++mi) offA[mi] += dlt;
#pragma unroll
        for (int oi = 0; oi < 2; ++oi) offB[oi] += dlt;
      }
      mfma_band(std::integral_constant<int, 0>{});
      while (ipc < npc) piece();
      if (more) {
        vm_wait(0);  // own dy row and mask dwords of band it+1 (x DMA and fold loads too: long landed)
        convert_own(orow, buf ^ 1, mwv);
      }
      if (wave == 4) ASR_BTR(1, 1, it - i0, 3);
      // halo rows of a band that continues this band's image: dz rows BR, BR+1
      // -> 0, 1 (masked), x rows BR, BR+1 -> 0, 1, dy row BR+1 -> 1; 5 x 256
      // chunks over the 512 wgrad threads
      if (it + 1 < i1 && nxt.n == cur.n) {
        const unsigned base = lds_u32(lds);
        const int nbf = buf ^ 1;
        u32x4 cv[3];
        unsigned dst[3];
        int nc = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const int c = ft + 512 * k;
          if (c < 5 * 256) {
            const int which = c >> 8;
            const unsigned o = (unsigned)((c & 255) + NQ) * 16u;
            const unsigned sreg = which < 2 ? L::DZ : which < 4 ? L::X : L::DY;
            const int srow = which == 4 ? BR + 1 : BR + (which & 1);
            const int drow = which == 4 ? 1 : (which & 1);
            cv[k] = lds_rd128(base + sreg + buf * L::TILE + srow * L::ROWB + o);
            dst[k] = base + sreg + nbf * L::TILE + drow * L::ROWB + o;
            nc = k + 1;
          }
        }
        lgkm_wait<0>();
#pragma unroll
        for (int k = 0; k < 3; ++k)
          if (k < nc) lds_wr128(dst[k], cv[k]);
      }
#pragma unroll
      for (int q = 0; q < 2; ++q)
        if (fold && fp < fpe) {
          facc += fv[q];
          ++fp;
          foff += ES;
        }
      if (wave == 4) ASR_BTR(1, 1, it - i0, 4);
    }
    barrier_vm(0);  // all items consumed: LDS reusable
    if (dbw && g == 0) {
      float* dbl = (float*)lds + 12288;  // [C]
#pragma unroll
      for (int oi = 0; oi < 2; ++oi) dbl[16 * (oq + oi) + lx] = hs * accb[oi][0];
    }
    constexpr int MC = XT ? 3 : MTW;
#pragma unroll
    for (int m0 = 0; m0 < MTW; m0 += MC) {
      float prev[XT ? MC : 1][2][4];
      if constexpr (XT) {
#pragma unroll
        for (int mi = 0; mi < MC; ++mi)
#pragma unroll
          for (int oi = 0; oi < 2; ++oi)
#pragma unroll
            for (int e = 0; e < 4; ++e)
              prev[mi][oi][e] = slab[(long)(16 * (tg * MTW + m0 + mi) + 4 * g + e) * C + 16 * (oq + oi) + lx];
      }
#pragma unroll
      for (int mi = 0; mi < MC; ++mi)
#pragma unroll
        for (int oi = 0; oi < 2; ++oi)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int m = 16 * (tg * MTW + m0 + mi) + 4 * g + e;
            float v = hs * acc[m0 + mi][oi][e];
            if constexpr (XT) v += prev[mi][oi][e];
            slab[(long)m * C + 16 * (oq + oi) + lx] = v;
          }
    }
  }
  __syncthreads();
  if (tid < C) {
    const float* dbl = (const float*)lds + 12288;
    float s = dbl[tid];
    if constexpr (XT) s += slab[9 * C * C + tid];
    slab[9 * C * C + tid] = s;
  }
  if (fold) {  // slabs the bands did not cover (a WG with fewer than 16 bands)
    for (; fp < fpe; ++fp, foff += ES) facc += *(const f32x4*)(pslabs + foff);
    *(f32x4*)(pgrp + (long)fg * ES + (foff - (unsigned)fpe * ES)) = facc;
  }
  ASR_BCLK(1, 1);
}

}  // namespace blk
}  // namespace asr
