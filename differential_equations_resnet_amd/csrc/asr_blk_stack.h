// The C = 64 stacks (W = 32, 4-row bands; part of asr_block_mfma.hip's
// translation unit): all L blocks of a network in ONE launch, forward
// (k_fwd3_stack) and backward (k_bwd3_stack), Euler and RK2.  The images do not
// interact, so a workgroup owns a contiguous run of whole images and walks
// (block, image, band) items with the per-block kernels' band protocols:
//   k_fwd3_stack  256 threads, 2 workgroups per CU, k_fwd3's band conv and
//                 regrouped epilogue on a ring of three LDS tiles; no workgroup
//                 ever waits for another.
//   k_bwd3_stack  768 threads (waves 0-3 dgrad, 4-11 wgrad), one workgroup per
//                 CU, k_bwd3's band protocol (Bwd2Lds, asr_blk_bwd.h), blocks
//                 last to first.  Workgroups exchange only the weight-gradient
//                 slabs: published per block, pass 1 of block l's reduction
//                 folded into the bands of block l-2 behind a bounded poll
//                 (a wait that runs out: stack_bwd_reduce_rest after the launch,
//                 g_stack_degraded).  PAIR: the slab holds the 74 tiles of
//                 D = dW - mirror(dW)^T (PairSlabLayout), not the 144 of dW.
// The comment above each kernel gives its ordering argument in full.
#pragma once
#include <type_traits>

#include "asr_blk_bwd.h"
#include "asr_blk_common.h"
#include "asr_common.h"
#include "asr_device.h"

namespace asr {
namespace blk {

// ===========================================================================
// Stack forward (C=64, W=32, BR=4, Euler): all L blocks of a network in ONE
// launch.  The images do not interact (3x3 SAME conv per image, no batch
// statistics), so a workgroup owns a contiguous run of whole images and walks
// (layer, image, band) items: block l+1 of an image reads only what this
// workgroup wrote for block l, and no workgroup ever waits for another.  The
// per-band protocol is k_fwd3's (band conv + regrouped epilogue, next band's
// rows by LDS-DMA into the other buffer, halo rows copied within an image).
// Replaces L launches of k_fwd3: no per-launch fill and drain, and no tail of
// workgroups with one band more than the rest (whole images per workgroup).
// Ordering: the DMA of item it+1 is issued after the barrier of item it, when
// every wave's stores of items <= it-1 have been waited for (barrier_vm counts
// only the previous item's stores as still in flight), so the first band of
// block l+1 (it reads rows -1..4 of block l's output, written by the first
// two bands of the image) needs >= 4 bands per workgroup and block: the host
// checks nb >= 4.  Training: activations are distinct buffers per block,
// written once in this launch.  Inference (slots = 2): x_{l+1} goes to slot
// l % 2 of ys, so block l+1 overwrites x_l; a workgroup finishes every item of
// block l (whole images, its own) before it writes block l+1, and its own
// stores and DMA reads meet in its CU's L1, so no line can be stale either.
// ===========================================================================
// RK2 (BASELINE config 5): 2L stages, stage 2l = the first (x_l -> xmid_l, h/2,
// mask1), stage 2l+1 the second (xmid_l -> x_{l+1}, h, mask2) with the residual
// x_l from global memory (16-B loads in the regrouped layout, as k_fwd3<..., RESG>).
template <int C, int W, int BR, bool RK2 = false>
__global__ __launch_bounds__(256, 2) void k_fwd3_stack(const bf16* __restrict__ x0, bf16* __restrict__ ys,
                                                       long y_stride, uint8_t* __restrict__ masks, long mask_stride,
                                                       const bf16* __restrict__ wpack, long w_stride,
                                                       const float* __restrict__ bias, long bias_stride, float h,
                                                       int N, int H, int L, int slots,
                                                       bf16* __restrict__ xm = nullptr,
                                                       uint8_t* __restrict__ masks2 = nullptr) {
  using G = Geo<C>;
  constexpr int TW = W + 2, NQ = G::NQ, OT = C / 16, NW = 4, RB = BR;
  static_assert(OT == NW && W == 32, "one 16-channel o-tile per wave, two pixel tiles");
  using BD = Band<C, W, RB>;
  constexpr int TILE = (BR + 2) * BD::ROWB;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ot = wave, g = lane >> 4, lx = lane & 15;
  const int o0 = 16 * ot + 4 * g;
  const int px = lx + 16 * (g & 1), cg = 2 * ot + (g >> 1);

  // whole images per workgroup
  const int n0 = (int)((long)blockIdx.x * N / gridDim.x), n1 = (int)((long)(blockIdx.x + 1) * N / gridDim.x);
  if (n0 >= n1) return;
  const int nb = (H + BR - 1) / BR, per = (n1 - n0) * nb;  // items per block
  // items walk stages (blocks, or RK2 half steps): block, input, output, mask, step of stage st
  auto blk_of = [&](int st) { return RK2 ? st >> 1 : st; };
  // slots: 0 = one buffer per block (training), 2 = ping-pong (inference; Euler only)
  auto slot_of = [&](int l) -> long { return slots > 0 ? (long)(l % slots) : (long)l; };
  auto xin_of = [&](int l) -> const bf16* { return l == 0 ? x0 : ys + slot_of(l - 1) * y_stride; };
  auto src_of = [&](int st) -> const bf16* {
    if constexpr (RK2) return (st & 1) ? xm + (long)(st >> 1) * y_stride : xin_of(st >> 1);
    else return xin_of(st);
  };
  auto out_of = [&](int st) -> bf16* {
    if constexpr (RK2) return ((st & 1) ? ys : xm) + (long)(st >> 1) * y_stride;
    else return ys + slot_of(st) * y_stride;
  };
  auto mask_of = [&](int st) -> uint8_t* {
    uint8_t* m = (RK2 && (st & 1)) ? masks2 : masks;
    return m ? m + (long)blk_of(st) * mask_stride : nullptr;
  };

  // A and the bias by untracked loads, here and at every block switch: the
  // next item's barrier_vm retires them (tracked, hipcc would wait vmcnt(0)
  // before each band's first MFMA, i.e. for the next band's DMA as well)
  bf16x8 A[G::KS] = {};
  load_A1_untracked<C>(wpack, ot, lane, A);
  unsigned lo[3 * BD::NCB];
  band_lane_offsets<C, W, RB>(g, lx, lo);
  float bz[4] = {0.f, 0.f, 0.f, 0.f};
  load_bias4_untracked(bias ? bias + 16 * ot : nullptr, g, bz);
  const unsigned lxr = (unsigned)toff<C>(1, px + 1, cg, TW);
  const unsigned ly = (unsigned)(px * C + 8 * cg) * 2u, lm = (unsigned)(px * (C / 8) + cg);

  // A ring of three tiles: a band that continues the previous band's image
  // reads its two halo rows where that band's tile holds them (rows BR, BR+1), so only its
  // BR new rows are DMA'd and nothing is copied inside LDS.  The DMA of band it+1 goes to
  // the tile band it-2 used, which band it-1 read last (as its halo rows): free after
  // band it's barrier.  (2 tiles: the halo rows copied into the next tile.)
  constexpr int NT = 3;
#pragma unroll
  for (int k = 0; k < NT; ++k) zero_halo_cols<C, W>(lds + k * TILE, BR + 2, tid, 64 * NW);
  constexpr int IPR = W / G::PPI;  // DMA pieces per row
  const unsigned loff = (unsigned)dma_lane_off<C, W>(lane) * 2u;
  // cursor over (stage l, image n, band b) and the band's first row R within this
  // workgroup's images ((n - n0) H + b BR, 32-bit): every address of a band is a per-stage
  // 64-bit base (computed once per stage) plus R times a power of two, so a band costs a
  // few scalar adds instead of 64-bit multiplies (the r05f instruction mix: ~180 scalar
  // instructions per band and wave before, a wave issues one instruction per ~4 cycles)
  int cl = 0, cn = n0, cb = 0, cR = 0;
  int xl = 0, xn = n0, xb = 0, xR = 0;  // next item
  auto adv = [&](int& l, int& n, int& b, int& R) {
    if (++b == nb) {
      b = 0;
      if (++n == n1) {
        n = n0;
        ++l;
        R = 0;
      } else {
        R = (n - n0) * H;
      }
    } else {
      R += BR;
    }
  };
  constexpr unsigned ROWBYTES = W * C * 2, MROWBYTES = W * C / 8;
  static_assert(ROWBYTES == 4096 && MROWBYTES == 256, "row byte shifts");
  const long img0 = (long)n0 * H;  // this workgroup's first image row
  const unsigned region = (unsigned)((n1 - n0) * H);  // its image rows
  // per stage: the output / mask buffer descriptors (base = this workgroup's first row) and
  // the next stage's DMA source base
  auto out_rs = [&](int st) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)(out_of(st) + img0 * W * C), 0, region * ROWBYTES, 0x00020000);
  };
  auto mask_rs = [&](int st) {
    uint8_t* m = mask_of(st);
    return __builtin_amdgcn_make_buffer_rsrc((void*)(m ? m + img0 * MROWBYTES : m), 0, m ? region * MROWBYTES : 0u,
                                             0x00020000);
  };
  auto src_base = [&](int st) { return (const unsigned char*)(src_of(st) + img0 * W * C); };
  adv(xl, xn, xb, xR);
  dma_rows<C, W>(x0, lds, cn, -1, min(BR, H) + 2, H, wave, NW, lane);
  int nst = 0;
  const int total = (RK2 ? 2 : 1) * L * per;
  ASR_BCLK(0, 0);
  int buf = 0, nbuf = 1, pbuf = NT - 1;  // this band's tile, the next band's, the previous band's
  auto yrs = out_rs(0);
  auto mrs = mask_rs(0);
  bool hasm = mask_of(0) != nullptr;
  const unsigned char* nsrc = src_base(0);  // the next item's stage's source rows
  int nsrc_st = 0;
  for (int it = 0; it < total; ++it) {
    if (wave == 0) ASR_BTR(0, 0, it, 0);
    barrier_vm_usual<2 * BR>(nst);  // band it landed; every wave is done with band it-1's tile
    if (wave == 0) ASR_BTR(0, 0, it, 1);
    nst = 0;
    // the next band into the ring: rows 0, 1 are this band's rows BR, BR+1 when it
    // continues the image (read in place), the rest by DMA
    if (it + 1 < total) {
      if (xl != nsrc_st) {  // (once per stage)
        nsrc = src_base(xl);
        nsrc_st = xl;
      }
      const int yy = xb * BR;
      const bool ncont = xl == cl && xn == cn && xb == cb + 1;
      const int r0 = ncont ? 1 : -1;  // image row offset of the first DMA'd tile row
      const int nrows = min(BR, H - yy) + (ncont ? 0 : 2);
      const unsigned nt0 = lds_u32(lds + nbuf * TILE) + (ncont ? 2u * BD::ROWB : 0u);
      // whole rows, one dma16x4 each (wave w: rows w, w + 4)
      for (int r = __builtin_amdgcn_readfirstlane(wave); r < nrows; r += NW) {
        const int gy = yy + r0 + r;
        const unsigned char* rowp = (unsigned)gy < (unsigned)H
                                        ? nsrc + (size_t)((unsigned)(xR + r0 + r) * ROWBYTES)
                                        : (const unsigned char*)g_zero_page;
        dma16x4_at(rowp + loff, nt0 + (unsigned)(r * BD::ROWB) + (unsigned)(NQ * 16));
      }
    }
    if (wave == 0) ASR_BTR(0, 0, it, 2);
    const unsigned tb = lds_u32(lds + buf * TILE);
    // input rows 0, 1: the previous band's tile rows BR, BR+1 when this band continues its image
    const unsigned th = cb > 0 ? lds_u32(lds + pbuf * TILE) + (unsigned)(BR * BD::ROWB) : tb;
    f32x4 acc[RB][2];
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
      for (int pt = 0; pt < 2; ++pt) acc[r][pt] = f32x4{bz[0], bz[1], bz[2], bz[3]};
    u32x4 xr[RB];
    const bool resg = RK2 && (cl & 1);  // second RK2 stage: residual x_l from global memory
    if (resg) {  // rows past the image end re-read its last row (never stored)
      const int y0 = cb * BR, rows = min(BR, H - y0);
      const unsigned char* rb = (const unsigned char*)(xin_of(cl >> 1) + ((long)cn * H + y0) * W * C) + ly;
#pragma unroll
      for (int r = 0; r < RB; ++r) xr[r] = *(const u32x4*)(rb + (long)min(r, rows - 1) * W * C * 2);
    }
    conv_band2<C, W, RB>(tb, th, lo, A, acc);
    if (wave == 0) ASR_BTR(0, 0, it, 3);
    if (!resg) {  // tile rows 1..RB (row 1 a halo row)
#pragma unroll
      for (int r = 0; r < RB; ++r) xr[r] = lds_rd128((r == 0 ? th : tb) + lxr + (unsigned)(r * BD::ROWB));
    }
    const int l = cl;
    if (blk_of(xl) != blk_of(cl) && it + 1 < total) {  // the next item starts block l+1: its W and bias (L2 hits)
      load_A1_untracked<C>(wpack + (long)blk_of(xl) * w_stride, ot, lane, A);
      load_bias4_untracked(bias ? bias + (long)blk_of(xl) * bias_stride + 16 * ot : nullptr, g, bz);
    }
    lgkm_wait<0>();
    const int rows = min(BR, H - cb * BR);
    // the band's y rows and mask rows as buffer stores: the stage's descriptor, the lane's
    // 32-bit offset and the row (R + r) as the scalar offset
    const float hst = (RK2 && !(l & 1)) ? 0.5f * h : h;
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      if (r >= rows) break;
      float z[8];
      regroup(acc[r][0], acc[r][1], z);
      u32x4 yw;
      unsigned bits = 0;
      static_for<0, 4>([&](auto dc) {
        constexpr int d = decltype(dc)::value;
        const int ra = max(__float_as_int(z[2 * d]), 0), rb = max(__float_as_int(z[2 * d + 1]), 0);
        yw[d] = pk_bf16(fmaf(hst, __int_as_float(ra), lo_f(xr[r][d])), fmaf(hst, __int_as_float(rb), hi_f(xr[r][d])));
        // relu-mask bits two at a time: [ra > 0] at bit 2d, [rb > 0] at bit 16 + 2d
        const unsigned pw = bits01_pair(ra, rb);
        bits = d == 0 ? pw : lshl_or<2 * d>(pw, bits);
      });
      bits = pair_bits_to_byte(bits);
      if (hasm) {
        __builtin_amdgcn_raw_buffer_store_b8((unsigned char)bits, mrs, (int)lm, (int)((unsigned)(cR + r) * MROWBYTES), 0);
        ++nst;
      }
      __builtin_amdgcn_raw_buffer_store_b128(yw, yrs, (int)ly, (int)((unsigned)(cR + r) * ROWBYTES), 0);
      ++nst;
    }
    if (wave == 0) ASR_BTR(0, 0, it, 4);
    if (xl != cl && it + 1 < total) {  // the next item starts a new stage: its store descriptors
      yrs = out_rs(xl);
      mrs = mask_rs(xl);
      hasm = mask_of(xl) != nullptr;
    }
    cl = xl, cn = xn, cb = xb, cR = xR;
    adv(xl, xn, xb, xR);
    pbuf = buf, buf = nbuf, nbuf = nbuf + 1 == NT ? 0 : nbuf + 1;
  }
  ASR_BCLK(0, 1);
}

// ===========================================================================
// Stack backward (C=64, W=32, BR=4, Euler): the backward of all L blocks in
// ONE launch, k_bwd3's band protocol and roles on (block, image, band) items,
// blocks last to first.  A workgroup owns whole images (as k_fwd3_stack), so
// block l-1 of an image reads only the dx this workgroup wrote for block l
// (ping-pong buffers dbuf[0/1]: block L-1 reads dbuf[0]); the only exchange
// between workgroups is the weight-gradient reduction:
//   * at the end of its items of block l, every wgrad wave stores its dW
//     tiles as sc1 (write-through) 16-B stores in the tile-major slab layout
//       slab[((mt * 4 + ot) * 64 + lane) * 4 + e] = dW[16 mt + 4 (lane>>4) + e][16 ot + (lane&15)]
//     (db after the 9C^2 block); the next band barrier drains them (vmcnt(0))
//     and one lane adds 1 to done[l] (relaxed, agent scope: the Guideline-16
//     write-through publish);
//   * pass 1 of block l's reduction (32-slab group sums, as k_bwd3's fold) is
//     folded into this workgroup's bands of block l-2: one lane polls done[l]
//     == gridDim.x before the first of them and fences acquire at agent scope,
//     and the band barrier orders that before every slab load.  Blocks below
//     lfold (>= 2; L when a workgroup would own more than 512 chunks of the
//     group rows, one per wgrad thread) are reduced after the launch.
//   * the poll is bounded (kStackSpinLimit sleeps, ~1-2 ms): a missed hand-off
//     costs speed, never correctness.  A workgroup whose wait runs out sets
//     skipf[l] (its share of block l's group rows may be built from slabs not
//     yet published), counts the event in g_stack_degraded (asr_stack_status),
//     and stops waiting for the rest of the launch (a word in LDS): every later
//     block it folds is flagged too.  After the launch, stack_bwd_reduce_rest
//     recomputes the group rows of every flagged block from its slabs, which
//     are all published by then (same stream), before the projection reads them.
// Co-residency of the grid (one 768-thread workgroup per CU, grid <= CUs; the
// stacked path is used only when the occupancy query keeps one resident per
// CU) is therefore a speed matter: a grid that is not (another kernel or
// process on the device) degrades to the post-launch reduction of the blocks
// whose wait ran out.  At the switch to block l-1 the dgrad waves load its W
// after their last conv of block l; block 0 applies the stem's relu' to dx
// when ro0 (k_bwd3<..., RO>).
// ===========================================================================
typedef __attribute__((address_space(1))) unsigned gu32;  // global agent-scope words (never flat)
// bound of the stacked backward's slab wait, in polls of one relaxed L2 load
// + s_sleep 2 (~1-2 ms: about one whole launch, far above the skew between
// resident workgroups, which stay within a block of each other).  A
// compile-time constant: a run-time bound cost the kernel a spilled register
// (tests/test_isa.py)
constexpr unsigned kStackSpinLimit = 1u << 13;
// waits of k_bwd3_stack workgroups that ran out since the last reset
// (asr_stack_status): each one means a slower launch (post-launch reduction of
// the flagged blocks), not a wrong gradient
__device__ unsigned g_stack_degraded = 0u;
typedef __attribute__((address_space(1))) float gf32;

// Pair-local weight-gradient tiling of k_bwd3_stack<..., PAIR> (C = 64, an
// antisymmetric operator: W[8-t][o][i] = -W[t][i][o] for tap t = 3ky+kx,
// …3By3.py:115-141, 277-293).  Every theta then pulls back
// D(t,i,o) = dW[t][i][o] - dW[8-t][o][i] (one entry, a sign), so the slab
// stores D, not dW: 74 16x16 tiles instead of 144 (half the publish burst
// and half the fold's reads).  Wave w8 = 2p + h of the 8 wgrad waves owns tap
// pair (p, 8-p) for input tiles a = 0..3 and output tiles b in {2h, 2h+1}:
// X = dW[p] tiles (A = x(p, a), B = dz(b)) and the transposed dW[8-p] tiles
// (A = dz(a), B = x(8-p, b): the same fragments in the other operand slot
// give the transpose), D = X - Y^T in registers; plus 2 MFMAs of tap 4:
// waves p < 3 one cross pair (a', b') of tiles (D likewise), waves p = 3 the
// two self tiles of their b-set (raw, and transposed for the odd one; the
// projection forms X - X^T there).  perm(0..3) orders the tiles a wave walks
// (its b-set first) so that every accumulator and register index is
// compile-time: acc[a][b] / acc[4+a][b] hold tiles (perm(a), perm(b)).
using PairSlab = PairSlabLayout;
constexpr int cmin(int a, int b) { return a < b ? a : b; }
// the pipelined pair wgrad (k_bwd3_stack): the last of a row's 12 fragments MFMA group g uses
constexpr int pf_last(int g) { return g == 0 ? 2 : g == 1 ? 3 : g == 2 ? 5 : g + 3; }  // (asr_common.h: the layout and the projection's pair_encode)
struct PairRole {
  // one wave-uniform word (the wgrad role sits at the SGPR limit): bits 0-7 perm(0..3),
  // 8-9 t, 10 self, 11 (s1 == 2), 12-14 k4
  unsigned w;
  __device__ __forceinline__ explicit PairRole(int w8) {
    const int t = w8 >> 1, h = w8 & 1, self = t == 3;
    // tap-4 cross pair k4 = (a', b') with b' in the wave's b-set {2h, 2h+1}
    const int k4 = 3 * h + t;
    const int ap = pair_tap4_a(k4), bp = pair_tap4_b(k4);
    const int b0 = self ? 2 * h : bp, b1 = (4 * h + 1) - b0;  // the b-set, b0 first
    // perm(2): a' when a' is outside the b-set (the tap-4 transposed product reads dz(perm(s1)))
    const int o0 = h ? 0 : 2, o1 = h ? 1 : 3;  // the two tiles outside the b-set
    const bool ain = !self && (ap >> 1) == h;
    const int p2 = (!self && !ain) ? ap : o0, p3 = (p2 == o0) ? o1 : o0;
    const int s2 = (self || ain) ? 0 : 1;
    w = (unsigned)(b0 | (b1 << 2) | (p2 << 4) | (p3 << 6) | (t << 8) | (self << 10) | (s2 << 11) | (k4 << 12));
  }
  __device__ __forceinline__ int perm(int k) const { return (w >> (2 * k)) & 3; }
  __device__ __forceinline__ int t() const { return (w >> 8) & 3; }
  __device__ __forceinline__ bool self() const { return (w >> 10) & 1; }
  __device__ __forceinline__ bool s1_is_2() const { return (w >> 11) & 1; }
  __device__ __forceinline__ int k4() const { return (int)(w >> 12) & 7; }
  // tap-4 fragments: x(4, u0) (phase 2, with dz(perm 0)), x(4, v1) (phase 1, with dz(perm s1))
  __device__ __forceinline__ int u0() const { return self() ? perm(0) : pair_tap4_a(k4()); }
  __device__ __forceinline__ int v1() const { return self() ? perm(1) : pair_tap4_b(k4()); }
  // LDS address bits of tile perm(k) relative to tile 0 (wave-uniform: one v_xor per read)
  __device__ __forceinline__ unsigned sh(int k) const { return (unsigned)perm(k) << 5; }
  // slab tile of acc[a][b] (D of tap t, input tile perm(a), output tile perm(b))
  __device__ __forceinline__ int tile(int a, int b) const { return t() * 16 + perm(a) * 4 + perm(b); }
};

// RK2 (config 5): items walk 2L stages, per block l its second stage first
// (dy = dL/dx_{l+1}, x = xmid_l, mask2, h, no +dy residual: out g = A^T dz2 into
// gbuf) then its first (dy = g, x = x_l, mask1, h/2, plus the extra term
// dL/dx_{l+1} by 16-B global loads: out dx_l).  Both stages accumulate one dW:
// at the stage switch acc *= 2 (exact), and the block's slab is (h/2) acc.
template <int C, int W, int BR, bool RK2 = false, bool PAIR = false>
__global__ __launch_bounds__(768, 1) void k_bwd3_stack(bf16* __restrict__ dbuf0, bf16* __restrict__ dbuf1,
                                                       const bf16* __restrict__ xs, long x_stride,
                                                       const uint8_t* __restrict__ masks, long mask_stride,
                                                       const bf16* __restrict__ wpack, long w_stride, float h,
                                                       float two_gamma, int N, int H, int L, int ro0,
                                                       float* __restrict__ slabs, long slab_stride,
                                                       float* __restrict__ grp, long grp_stride,
                                                       unsigned* __restrict__ done, unsigned* __restrict__ skipf,
                                                       int lfold, const bf16* __restrict__ xm = nullptr,
                                                       const uint8_t* __restrict__ masks2 = nullptr,
                                                       bf16* __restrict__ gbuf = nullptr,
                                                       const bf16* __restrict__ gtop = nullptr) {
  using G = Geo<C>;
  using LL = Bwd2Lds<C, W, BR>;
  using BD = Band<C, W, BR>;
  constexpr int TW = W + 2, OT = G::OT, MTW = G::MTW, IPR = W / G::PPI, NQ = G::NQ;
  static_assert(C == 64 && W == 32 && BR == 4 && MTW == 9 && OT == 4, "v3 backward geometry");
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, lx = lane & 15;

  for (int b = 0; b < 2; ++b) {
    zero_halo_cols<C, W>(lds + LL::DY + b * LL::TILE, BR + 2, tid, 768);
    zero_halo_cols<C, W>(lds + LL::X + b * LL::TILE, BR + 2, tid, 768);
    zero_halo_cols<C, W>(lds + LL::DZ + b * LL::TILE, BR + 2, tid, 768);
  }
  {
    unsigned* tab = (unsigned*)(lds + LL::MTAB);
    for (int i = tid; i < 1024; i += 768) {
      const unsigned m = (unsigned)i >> 2, d = (unsigned)i & 3;
      tab[i] = (((m >> (2 * d)) & 1u) ? 0xffffu : 0u) | (((m >> (2 * d + 1)) & 1u) ? 0xffff0000u : 0u);
    }
  }
  // the LDS byte address of the allocation, taken here (uniform code): casting in the dgrad
  // role's code made hipcc (ROCm 7.2) emit the cast's null check as an illegal VALU compare
  const unsigned lds0 = lds_u32(lds);
  unsigned* late = (unsigned*)(lds + LL::TOTAL);  // a slab wait of this workgroup ran out: stop waiting
  if (tid == 0) *late = 0u;
  const int n0 = (int)((long)blockIdx.x * N / gridDim.x), n1 = (int)((long)(blockIdx.x + 1) * N / gridDim.x);
  // cursor index l is a STAGE: the block itself (Euler) or 2*block + (1: second RK2 stage, 0: first)
  constexpr int SPB = RK2 ? 2 : 1;
  const int nb = (H + BR - 1) / BR, per = (n1 - n0) * nb, total = SPB * L * per;
  const unsigned loff = (unsigned)dma_lane_off<C, W>(lane) * 2u;
  auto blk_of = [&](int st) { return RK2 ? st >> 1 : st; };
  auto s1_of = [&](int st) { return RK2 && !(st & 1); };  // first RK2 stage: h/2, extra term
  // block l reads dL/dx_{l+1} from dbuf[(L-1-l) & 1] and writes dL/dx_l to the other one
  auto din_of = [&](int l) -> bf16* { return ((L - 1 - l) & 1) ? dbuf1 : dbuf0; };
  auto dout_of = [&](int l) -> bf16* { return ((L - 1 - l) & 1) ? dbuf0 : dbuf1; };
  auto dy_of = [&](int st) -> bf16* {
    if constexpr (RK2) return (st & 1) ? din_of(st >> 1) : gbuf;
    else return din_of(st);
  };
  auto dx_of = [&](int st) -> bf16* {
    if constexpr (RK2) return (st & 1) ? gbuf : dout_of(st >> 1);
    else return dout_of(st);
  };
  auto x_of = [&](int st) -> const bf16* {
    if constexpr (RK2) return ((st & 1) ? xm : xs) + (long)(st >> 1) * x_stride;
    else return xs + (long)st * x_stride;
  };
  auto mask_of = [&](int st) -> const uint8_t* {
    if constexpr (RK2) return ((st & 1) ? masks2 : masks) + (long)(st >> 1) * mask_stride;
    else return masks + (long)st * mask_stride;
  };
  // (block, image, band) cursor, blocks last to first
  struct Cur {
    int l, n, b;
  };
  auto adv = [&](Cur& c) {
    if (++c.b == nb) {
      c.b = 0;
      if (++c.n == n1) {
        c.n = n0;
        --c.l;
      }
    }
  };
  __syncthreads();
  if (n0 >= n1) return;  // (uniform per workgroup: never with grid <= N)
  ASR_BCLK(1, 0);

  constexpr int ES = PAIR ? PairSlab::ES : 9 * C * C + C, ECH = ES / 4;
  if (wave < 4) {
    // ---------------- dgrad waves ----------------
    const int ot = wave;
    // W by untracked loads, here and at each block switch: the next item's
    // barrier_vm retires them (a tracked reload made hipcc wait vmcnt(0) before
    // every band's first MFMA, i.e. for the previous band's dx stores)
    bf16x8 A[G::KS] = {};
    load_A1_untracked<C>(wpack + (long)(L - 1) * w_stride, ot, lane, A);
    unsigned lo[3 * BD::NCB];
    band_lane_offsets<C, W, BR>(g, lx, lo);
    const int px = lx + 16 * (g & 1), cg = 2 * ot + (g >> 1);
    const unsigned lch = (unsigned)toff<C>(1, px + 1, cg, TW);
    const unsigned ldx = (unsigned)(px * C + 8 * cg) * 2u;
    int nst = 0;
    Cur cur{SPB * L - 1, n0, 0};
    for (int it = 0; it < total; ++it) {
      const int buf = it & 1;
      const int n = cur.n, y0 = cur.b * BR, l = cur.l;
      const int rows = min(BR, H - y0);
      if (wave == 0) ASR_BTR(1, 0, it, 0);
      const bool sw_ = !RK2 && cur.b == 0 && n == n0;  // (trace build: the first band of block l)
      if (wave == 0 && sw_) ASR_BSW(l, 3, false);
      barrier_vm_usual<BR>(nst);  // item it staged everywhere; item it-1 fully consumed
      if (wave == 0) ASR_BTR(1, 0, it, 1);
      if (wave == 0 && sw_) ASR_BSW(l, 4, false);
      const unsigned dzt = lds_u32(lds + LL::DZ + buf * LL::TILE), dyt = lds_u32(lds + LL::DY + buf * LL::TILE);
      const unsigned xt = lds_u32(lds + LL::X + buf * LL::TILE);
      const bool s1 = s1_of(l);
      const float hs = s1 ? 0.5f * h : h, hs2g = hs * two_gamma;
      // RK2 first stage: the extra dx term dL/dx_{l+1} of the band's rows (in flight during the conv)
      u32x4 exv[RK2 ? BR : 1];
      if (RK2 && s1) {
        const bf16* eb = din_of(blk_of(l)) + ((long)n * H + y0) * W * C;
#pragma unroll
        for (int r = 0; r < (RK2 ? BR : 1); ++r)
          exv[r] = *(const u32x4*)((const unsigned char*)(eb + (long)min(r, rows - 1) * W * C) + ldx);
      }
      f32x4 acc[BR][2];
#pragma unroll
      for (int r = 0; r < BR; ++r) acc[r][0] = acc[r][1] = f32x4{0.f, 0.f, 0.f, 0.f};
      conv_band<C, W, BR>(dzt, lo, A, acc);
      if (wave == 0) ASR_BTR(1, 0, it, 2);
      const bool last_of_stage = cur.b == nb - 1 && n == n1 - 1;
      if (last_of_stage && blk_of(l) > 0 && (!RK2 || s1))
        load_A1_untracked<C>(wpack + (long)(blk_of(l) - 1) * w_stride, ot, lane, A);
      bf16* drow = dx_of(l) + ((long)n * H + y0) * W * C;
      // dx rows as buffer stores (uniform base, the lane's 32-bit offset, the row as the scalar offset)
      const auto drs = __builtin_amdgcn_make_buffer_rsrc((void*)(RK2 ? nullptr : drow), 0, BR * W * C * 2, 0x00020000);
      int nld = 0;
      auto epilogue = [&](auto g2c, auto roc, auto kc) {
        // KIND 0: Euler (+dy), 1: second RK2 stage (no +dy), 2: first RK2 stage (+dy +extra)
        constexpr bool G2 = decltype(g2c)::value, RO = decltype(roc)::value;
        constexpr int KIND = decltype(kc)::value;
        constexpr bool RDY = KIND != 1;
        constexpr int NR = (RDY ? 1 : 0) + (G2 ? 1 : 0) + (RO ? 1 : 0);  // LDS reads per row
        u32x4 dyw[2], dzw[2], xw[2];
        auto issue = [&](int r, int sl) {
          const unsigned co = lch + (unsigned)(r * LL::ROWB);
          if constexpr (RDY) dyw[sl] = lds_rd128(dyt + co);
          if constexpr (G2) dzw[sl] = lds_rd128(dzt + co);
          if constexpr (RO) xw[sl] = lds_rd128(xt + co);
        };
        // the reads run on a compile-time schedule, each retired before the row guard,
        // so no branch sits between a read and the wait that retires it: with the
        // reads inside the guard hipcc merged a read's register at the join with a copy
        // placed before that wait (stale dy rows under LDS contention, tools/asm_lds_audit.py)
        if constexpr (NR > 0) issue(0, 0);
        static_for<0, BR>([&](auto rc) {
          constexpr int r = decltype(rc)::value, sl = r & 1;
          if constexpr (NR > 0) {
            if constexpr (r + 1 < BR) {
              issue(r + 1, sl ^ 1);
              lgkm_wait<NR>();
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
              float r0 = 0.f, r1 = 0.f;
              if constexpr (RDY) r0 = lo_f(dyw[sl][d]), r1 = hi_f(dyw[sl][d]);
              if constexpr (KIND == 2) {
                r0 += lo_f(exv[RK2 ? r : 0][d]);
                r1 += hi_f(exv[RK2 ? r : 0][d]);
              }
              float v0 = fmaf(-hs, z[2 * d], r0);
              float v1 = fmaf(-hs, z[2 * d + 1], r1);
              if constexpr (G2) {
                v0 = fmaf(hs2g, lo_f(dzw[sl][d]), v0);
                v1 = fmaf(hs2g, hi_f(dzw[sl][d]), v1);
              }
              ow[d] = pk_bf16(v0, v1);
              if constexpr (RO) {
                const unsigned xd = xw[sl][d];
                ow[d] &= ((int)(short)(xd & 0xffffu) > 0 ? 0xffffu : 0u) | ((int)xd > 0xffff ? 0xffff0000u : 0u);
              }
            }
            if constexpr (RK2)  // (its dgrad role has no SGPRs to spare for the descriptor)
              *(u32x4*)((unsigned char*)(drow + (long)r * W * C) + ldx) = ow;
            else
              __builtin_amdgcn_raw_buffer_store_b128(ow, drs, (int)ldx, r * W * C * 2, 0);
            ++nld;
          }
        });
      };
      using T_ = std::true_type;
      using F_ = std::false_type;
      using K0 = std::integral_constant<int, 0>;
      using K1 = std::integral_constant<int, 1>;
      using K2 = std::integral_constant<int, 2>;
      const bool g2 = hs2g != 0.f;
      if constexpr (RK2) {
        if (s1) {
          if (g2) epilogue(T_{}, F_{}, K2{});
          else epilogue(F_{}, F_{}, K2{});
        } else {
          if (g2) epilogue(T_{}, F_{}, K1{});
          else epilogue(F_{}, F_{}, K1{});
        }
      } else {
        const bool ro = ro0 && l == 0;
        if (ro) {
          if (g2) epilogue(T_{}, T_{}, K0{});
          else epilogue(F_{}, T_{}, K0{});
        } else {
          if (g2) epilogue(T_{}, F_{}, K0{});
          else epilogue(F_{}, F_{}, K0{});
        }
      }
      nst = nld;
      if (wave == 0) ASR_BTR(1, 0, it, 3);
      if (!RK2 && cur.b + 1 < nb) {  // (RK2: the wgrad waves copy them; its dgrad role has no registers to spare)
        // the next item continues this image: its tile rows 0, 1 are this band's rows BR, BR+1
        // (dz, x; dy row 1 only), copied here, where the dgrad waves would otherwise wait at
        // the band barrier for the wgrad waves.  Rows BR, BR+1 of this item's tiles were
        // complete at its barrier, and no wave touches rows 0, 1 of the other buffer before
        // the next one (its DMAs and the convert fill rows 2..).  Compiler-visible LDS
        // accesses: the epilogue's asm reads were retired by its last lgkm_wait<0>, and these
        // waves have no LDS-DMA in flight
        const unsigned base = lds0;
        const int nbf = buf ^ 1;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
          const int c = tid + 256 * k;  // 5 x 256 16-B chunks: dz rows, x rows, dy row
          const unsigned o = (unsigned)((c & 255) + NQ) * 16u;
          const unsigned sreg = k < 2 ? LL::DZ : k < 4 ? LL::X : LL::DY;
          const int srow = k == 4 ? BR + 1 : BR + (k & 1);
          const int drow = k == 4 ? 1 : (k & 1);
          lds_st128(base + sreg + nbf * LL::TILE + drow * LL::ROWB + o,
                    lds_ld128(base + sreg + buf * LL::TILE + srow * LL::ROWB + o));
        }
      }
      if (wave == 0) ASR_BTR(1, 0, it, 4);
      adv(cur);
    }
    barrier_vm(0);  // matches the wgrad waves' end-of-loop barrier
  } else {
    // ---------------- wgrad waves ----------------
    const int w8 = __builtin_amdgcn_readfirstlane(wave) - 4;
    const int tg = w8 >> 1, oq = 2 * (w8 & 1);
    const int tq = lx >> 2, tp = lx & 3;
    const int ft = tid - 256;
    f32x4 acc[MTW][2];
#pragma unroll
    for (int mi = 0; mi < MTW; ++mi) acc[mi][0] = acc[mi][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    // operand addresses: the full-dW tiling (PAIR false) reads 9 x fragments (offA) and 2 dz
    // fragments (offB) per row; the pair-local tiling (PairRole) 8 x and 4 dz fragments
    constexpr int NOA = PAIR ? 5 : MTW, NOB = PAIR ? 1 : 2;
    unsigned offA[NOA], offB[NOB];  // pixel tile 1 sits 16 px = 2 KiB on (swizzle period 8 px)
    const PairRole pr(w8);
    {
      const unsigned xb0 = lds_u32(lds + LL::X), zb0 = lds_u32(lds + LL::DZ);
      const int pb = 4 * g + tq;
      auto xoff = [&](int tap, int itile) {
        const int ky = tap / 3, kx = tap % 3, q = 2 * itile + (tp >> 1);
        return xb0 + (unsigned)(toff<C>(ky, pb + kx, q, TW) + 8 * (tp & 1));
      };
      auto zoff = [&](int otile) {
        return zb0 + (unsigned)(toff<C>(1, pb + 1, 2 * otile + (tp >> 1), TW) + 8 * (tp & 1));
      };
      if constexpr (PAIR) {
        // offA: x(t, tile 0), x(8-t, perm[0]), x(8-t, perm[1]), x(4, u0), x(4, v1); offB: dz(tile 0).
        // A 16-channel tile's fragment address differs from tile 0's only in address bits 5-6
        // (the chunk index 2*tile + h, XOR-swizzled by the column: (tile ^ (col&7)>>1) << 5; the
        // buffer bases and the tile-buffer step keep those bits clear), so x(t, a) and dz(a) are
        // read at offA[0] ^ (a << 5), offB[0] ^ (a << 5): one register each instead of four
        offA[0] = xoff(pr.t(), 0);
        offA[1] = xoff(8 - pr.t(), pr.perm(0));
        offA[2] = xoff(8 - pr.t(), pr.perm(1));
        offA[3] = xoff(4, pr.u0());
        offA[4] = xoff(4, pr.v1());
        offB[0] = zoff(0);
      } else {
#pragma unroll
        for (int mi = 0; mi < MTW; ++mi) {
          const int mt = tg * MTW + mi;
          offA[mi] = xoff((16 * mt) / C, ((16 * mt) % C) / 16);
        }
#pragma unroll
        for (int oi = 0; oi < 2; ++oi) offB[oi] = zoff(oq + oi);
      }
      // opaque to the compiler: kept in VGPRs, not recomputed per band
#pragma unroll
      for (int k = 0; k < NOA; ++k) asm volatile("" : "+v"(offA[k]));
#pragma unroll
      for (int k = 0; k < NOB; ++k) asm volatile("" : "+v"(offB[k]));
    }
    auto own_row = [&](bool reuse) { return reuse ? (w8 < 4 ? 2 + w8 : -1) : (w8 < 6 ? w8 : -1); };
    // gtop (Euler): the top block's dy = dL/dx_L is the GAP gradient, one row per image constant over the
    // pixels (tfkeras_resnets.py:595-597); its tile rows are written from that row (zeros outside the
    // image, as the DMA's zero page) instead of read from a full tensor
    auto synth = [&](const Cur& c) { return !RK2 && gtop != nullptr && c.l == L - 1; };
    auto synth_row = [&](const Cur& c, int row, int nbuf) {
      const int gy = c.b * BR - 1 + row, q = lane & 7, p0 = lane >> 3;
      u32x4 v = {0u, 0u, 0u, 0u};
      if ((unsigned)gy < (unsigned)H) {  // (buffer load: a 32-bit lane offset, no 64-bit per-lane pointer kept live)
        const auto rs = __builtin_amdgcn_make_buffer_rsrc((void*)(gtop + (long)c.n * C), 0, C * 2, 0x00020000);
        v = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, 16 * q, 0, 0));
      }
      const unsigned rb = lds_u32(lds + LL::DY + nbuf * LL::TILE + row * LL::ROWB);
#pragma unroll
      for (int k = 0; k < W / 8; ++k) lds_st128(rb + (unsigned)toff<C>(0, p0 + 8 * k + 1, q, TW), v);
    };
    auto stage_own = [&](const Cur& c, int row, int nbuf, unsigned& mwv) {
      if (row < 0) return;
      mwv = bwd2_mask_word<C, W>(mask_of(c.l), c.n, c.b * BR, row, H, lane);
      if (synth(c)) {
        synth_row(c, row, nbuf);
        return;
      }
      for (int j = 0; j < IPR; ++j)
        dma_row_instr_at<C, W>(dy_of(c.l), lds0 + (unsigned)(LL::DY + nbuf * LL::TILE + row * LL::ROWB), c.n, c.b * BR - 1 + row, j,
                            H, loff);
    };
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
          off[j] = (unsigned)toff<C>(row, cpx + 1, 4 * hh + jj + j, TW) + (unsigned)(nbuf * LL::TILE);
          v[j] = lds_ld128(base + LL::DY + off[j]);
          mt[j] = lds_ld128(base + LL::MTAB + __builtin_amdgcn_ubfe(mwv, 8 * (jj + j), 8) * 16);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          u32x4 z = v[j];
          z &= mt[j];
          lds_st128(base + LL::DZ + off[j], z);
        }
      }
    };
    bf16x8 ones;
#pragma unroll
    for (int i = 0; i < 8; ++i) ones[i] = (bf16)1.0f;
    f32x4 accb[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    const bool dbw = PAIR ? pr.self() : tg == 3;
    // fold state (pass 1 of block l+2's reduction while on block l)
    const long fT = (long)((gridDim.x + 31) / 32) * ECH;
    const long fc0 = (long)blockIdx.x * fT / gridDim.x, fc1 = (long)(blockIdx.x + 1) * fT / gridDim.x;
    const bool fmine = ft >= 0 && fc0 + ft < fc1;
    const int fg = fmine ? (int)((fc0 + ft) / ECH) : 0;
    const int fpe = min((int)gridDim.x, 32 * fg + 32);
    const unsigned fch = fmine ? (unsigned)((fc0 + ft) % ECH) * 4 : 0u;
    bool fold = false;
    int fp = 0;
    unsigned foff = 0u;
    const float* pslabs = slabs;
    f32x4 facc = {0.f, 0.f, 0.f, 0.f}, fv[2];
    auto fold_begin = [&](int l) {  // block l's slabs (published: done[l] == grid, acquired)
      fold = fmine;
      fp = 32 * fg;
      foff = (unsigned)fp * ES + fch;
      pslabs = slabs + (long)l * slab_stride;
      facc = f32x4{0.f, 0.f, 0.f, 0.f};
    };
    auto fold_end = [&](int l) {
      if (fold) {
        for (; fp < fpe; ++fp, foff += ES) facc += *(const f32x4*)(pslabs + foff);
        // (the group row's offset from live values: foff - fpe*ES is this thread's chunk)
        *(f32x4*)(grp + (long)l * grp_stride + ((unsigned)fg * ES + (foff - (unsigned)fpe * ES))) = facc;
      }
      fold = false;
    };
    const float hsb = RK2 ? 0.5f * h : h;  // the slab scale (RK2: acc doubled at the stage switch)
    {  // prologue: own dy rows and x rows of item 0, its dz converted
      const Cur c0{SPB * L - 1, n0, 0};
      unsigned mw0 = 0u;
      const int row0 = own_row(false);
      stage_own(c0, row0, 0, mw0);
      for (int j = w8; j < (BR + 2) * IPR; j += 8)
        dma_row_instr_at<C, W>(x_of(c0.l), lds0 + (unsigned)LL::X, c0.n, c0.b * BR - 1, j, H, loff);
      vm_wait(0);
      convert_own(row0, 0, mw0);
    }
    Cur cur{SPB * L - 1, n0, 0}, nxt{SPB * L - 1, n0, 0};
    adv(nxt);
    for (int it = 0; it < total; ++it) {
      const int buf = it & 1;
      const int y0 = cur.b * BR, l = blk_of(cur.l);  // (l: the block)
      const int rows = min(BR, H - y0);
      const bool first_of_block = cur.b == 0 && cur.n == n0 && (!RK2 || (cur.l & 1));
      if (wave == 4) ASR_BTR(1, 1, it, 0);
      if (wave == 4 && first_of_block && !RK2) {
        ASR_BSW(l, 0, false);
        ASR_BSW(l, 5, true);
      }
      if (first_of_block && l + 2 < L && l + 2 >= lfold && w8 == 0 && lane == 0) {
        // block l+2's slabs: every workgroup published them (bounded poll); once a
        // wait of this workgroup ran out, every later block it folds is flagged
        // for the post-launch reduction instead (stack_bwd_reduce_rest)
        bool ran_out = *(volatile unsigned*)late != 0u;
        if (!ran_out) {
          unsigned spins = 0;
          while (__hip_atomic_load((gu32*)(done + l + 2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < gridDim.x) {
            __builtin_amdgcn_s_sleep(2);
            if (++spins > kStackSpinLimit) {
              ran_out = true;
              *(volatile unsigned*)late = 1u;
              __hip_atomic_fetch_add((gu32*)&g_stack_degraded, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              break;
            }
          }
        }
        if (ran_out) __hip_atomic_store((gu32*)(skipf + l + 2), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      }
      if (wave == 4 && first_of_block && !RK2) ASR_BSW(l, 1, false);
      barrier_vm(0);  // this wave's x rows of item it landed (and its slab stores drained)
      if (wave == 4) ASR_BTR(1, 1, it, 1);
      if (wave == 4 && first_of_block && !RK2) {
        ASR_BSW(l, 2, false);
        ASR_BSW(l, 6, true);
      }
      if (first_of_block && l + 1 < L && l + 1 >= lfold && w8 == 0 && lane == 0)
        __hip_atomic_fetch_add((gu32*)(done + l + 1), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // published
      if (first_of_block && l + 2 < L && l + 2 >= lfold) fold_begin(l + 2);
#pragma unroll
      for (int q = 0; q < 2; ++q)
        if (fold && fp + q < fpe) fv[q] = *(const f32x4*)(pslabs + foff + (unsigned)q * ES);
      const bool more = it + 1 < total;
      const bool cont = more && nxt.l == cur.l && nxt.n == cur.n;
      const int orow = more ? own_row(cont) : -1;
      unsigned mwv = 0u;
      if (orow >= 0) mwv = bwd2_mask_word<C, W>(mask_of(nxt.l), nxt.n, nxt.b * BR, orow, H, lane);
      const int xr0 = cont ? 2 : 0;
      const bool syn = orow >= 0 && synth(nxt);
      if (syn) synth_row(nxt, orow, buf ^ 1);
      // the next band's rows, each by one whole-row DMA (4 pieces on one address): the own dy
      // row, and x rows 2..5 on waves 4..7 when the next band continues this image (rows 0, 1
      // are the halo copy), else rows 0..5 with row r on wave (r + 6) & 7.  (Measured and not
      // kept: the x rows DMA'd by the dgrad waves before their conv, -1.8 %, r05c)
      if (orow >= 0 && !syn)
        dma_row_whole_at<C, W>(dy_of(nxt.l), lds0 + (unsigned)(LL::DY + (buf ^ 1) * LL::TILE + orow * LL::ROWB), nxt.n,
                               nxt.b * BR - 1 + orow, H, loff);
      if (more) {
        const int xrow = cont ? (w8 >= 4 ? w8 - 2 : -1) : (((w8 + 2) & 7) < BR + 2 ? ((w8 + 2) & 7) : -1);
        if (xrow >= 0)
          dma_row_whole_at<C, W>(x_of(nxt.l), lds0 + (unsigned)(LL::X + (buf ^ 1) * LL::TILE + xrow * LL::ROWB), nxt.n,
                                 nxt.b * BR - 1 + xrow, H, loff);
      }
      if (wave == 4) ASR_BTR(1, 1, it, 2);
      bf16x8 Bf[2], Ar[3];
      auto mfma_band_full = [&](auto bo) {
        constexpr int BO = decltype(bo)::value;
        Ar[0] = tr_pair_px<BO>(offA[0]);
        static_for<0, BR>([&](auto rc) {
          constexpr int r = decltype(rc)::value, RO_ = BO + r * LL::ROWB;
          __builtin_amdgcn_sched_barrier(0);
          if (r < rows) {
            const bool mr = r + 1 < rows;
#pragma unroll
            for (int oi = 0; oi < 2; ++oi) Bf[oi] = tr_pair_px<RO_>(offB[oi]);
            Ar[1] = tr_pair_px<RO_>(offA[1]);
            static_for<0, MTW>([&](auto mc) {
              constexpr int mi = decltype(mc)::value;
              if constexpr (mi + 2 < MTW) Ar[(mi + 2) % 3] = tr_pair_px<RO_>(offA[mi + 2]);
              else if constexpr (mi + 2 == MTW && r + 1 < BR) {
                if (mr) Ar[0] = tr_pair_px<RO_ + LL::ROWB>(offA[0]);
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
      // pair-local tiling (PairRole): per row, phase 1 the transposed products of tap 8-t
      // (A = dz(perm[a]), B = -x(8-t, perm[b]): -dW[8-t]^T tiles) and the tap-4 partner's,
      // phase 2 the direct products of tap t (A = x(t, perm[a]), B = dz(perm[b])) and the
      // tap-4 tile, both into acc[a][b], which holds D = X - Y^T at the block's end.
      // The band's 4 x 12 operand fragments are one read stream, each read issued P = 3
      // fragments ahead of the MFMA group that first uses it, across the row boundaries
      // (the transposed reads are compiler-visible builtins: hipcc places their waits; a
      // version reading each row's fragments at the row's start ran its MFMA phase 0.5-0.6 k
      // cycles longer per band); row r's fragments in use order:
      //   0 dz(p0) 1 x(8-t, p0) 2 x(8-t, p1) 3 dz(p1) 4 dz(p2) 5 x(4, v1) 6 dz(p3)
      //   7..10 x(t, p0..p3) 11 x(4, u0)
      // The registers of the stream come from accumulating the transposed products into
      // acc[a][b] with the x(8-t) operand negated (bf16 sign flips, exact) instead of into
      // separate Y^T tiles: 40 accumulator VGPRs instead of 72 (acc[4..7] unused).  No row guard: rows past `rows` (the
      // image's last band when H % 4 != 0) are outside the image, where the dz tile is
      // zero (zero-page DMA, zero mask words), so their products add zeros.
      auto mfma_band_pair = [&](auto bo) {
        constexpr int BO = decltype(bo)::value, NF = 12, P = 3;
        bf16x8 F[BR * NF];  // compile-time indices only: registers, allocated by liveness
        auto rd = [&](auto jc) {
          constexpr int j = decltype(jc)::value, k = j % NF, R = BO + (j / NF) * LL::ROWB;
          if constexpr (k == 0 || k == 3 || k == 4 || k == 6)
            F[j] = tr_pair_px<R>(offB[0] ^ pr.sh(k == 0 ? 0 : k == 3 ? 1 : k == 4 ? 2 : 3));
          else if constexpr (k == 1 || k == 2) F[j] = tr_pair_px<R>(offA[k]);
          else if constexpr (k == 5) F[j] = tr_pair_px<R>(offA[4]);
          else if constexpr (k < 11) F[j] = tr_pair_px<R>(offA[0] ^ pr.sh(k - 7));
          else F[j] = tr_pair_px<R>(offA[3]);
        };
        // group g of a row first needs fragment pf_last(g); reads up to that + P are issued before it
        static_for<0, BR>([&](auto rc) {
          constexpr int r = decltype(rc)::value, b = r * NF;
          bf16x8 nxa, nxb;
          static_for<0, 9>([&](auto gc) {
            constexpr int g = decltype(gc)::value;
            constexpr int lo = g == 0 ? (r == 0 ? 0 : cmin(BR * NF, b - NF + pf_last(8) + 1 + P))
                                      : cmin(BR * NF, b + pf_last(g - 1) + 1 + P);
            constexpr int hi = cmin(BR * NF, b + pf_last(g) + 1 + P);
            static_for<lo, hi>(rd);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (g == 0) {
              nxa = neg_bf16x8(F[b + 1]);
              nxb = neg_bf16x8(F[b + 2]);
            }
            if constexpr (g < 4) {  // transposed products of tap 8-t (+ the tap-4 partner's)
              constexpr int dzk = g == 0 ? 0 : g == 1 ? 3 : g == 2 ? 4 : 6;
              acc[g][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(F[b + dzk], nxa, acc[g][0], 0, 0, 0);
              acc[g][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(F[b + dzk], nxb, acc[g][1], 0, 0, 0);
              if constexpr (g == 2) {  // dz(perm[s1]) x x(4, v1)
                const bf16x8 sel = pr.s1_is_2() ? F[b + 4] : F[b + 3];
                acc[8][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sel, F[b + 5], acc[8][1], 0, 0, 0);
              }
            } else if constexpr (g < 8) {  // direct products of tap t
              acc[g - 4][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(F[b + 3 + g], F[b], acc[g - 4][0], 0, 0, 0);
              acc[g - 4][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(F[b + 3 + g], F[b + 3], acc[g - 4][1], 0, 0, 0);
            } else {  // the tap-4 tile, db
              acc[8][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(F[b + 11], F[b], acc[8][0], 0, 0, 0);
              if (dbw) {
                accb[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, F[b], accb[0], 0, 0, 0);
                accb[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, F[b + 3], accb[1], 0, 0, 0);
              }
            }
          });
        });
      };
      auto convert_next = [&]() {  // the next band's dz of this wave's own row
        if (more) {
          vm_wait(0);  // own dy row and mask dwords of band it+1 (x DMA and fold loads too)
          if (wave == 4) ASR_BTR(1, 1, it, 4);
          convert_own(orow, buf ^ 1, mwv);
        }
      };
      auto mfma_band = [&](auto bo) {
        if constexpr (PAIR) mfma_band_pair(bo);
        else mfma_band_full(bo);
      };
      if (it > 0) {
        const unsigned dlt = buf ? (unsigned)LL::TILE : (unsigned)-LL::TILE;
#pragma unroll
        for (int k = 0; k < NOA; ++k) offA[k] += dlt;
#pragma unroll
        for (int k = 0; k < NOB; ++k) offB[k] += dlt;
      }
      mfma_band(std::integral_constant<int, 0>{});
      if (wave == 4) ASR_BTR(1, 1, it, 3);
      convert_next();
      if (wave == 4) ASR_BTR(1, 1, it, 5);
      if (RK2 && cont) {  // halo rows of the next band of this image (Euler: the dgrad waves copy them)
        // compiler-visible LDS accesses: the item's DMAs were retired by the vm_wait(0)
        // before the convert (cont implies more), so hipcc's own waits cost nothing
        // here, and a copied or spilled read result stays correct
        const unsigned base = lds_u32(lds);
        const int nbf = buf ^ 1;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const int c = ft + 512 * k;
          if (c < 5 * 256) {
            const int which = c >> 8;
            const unsigned o = (unsigned)((c & 255) + NQ) * 16u;
            const unsigned sreg = which < 2 ? LL::DZ : which < 4 ? LL::X : LL::DY;
            const int srow = which == 4 ? BR + 1 : BR + (which & 1);
            const int drow = which == 4 ? 1 : (which & 1);
            lds_st128(base + sreg + nbf * LL::TILE + drow * LL::ROWB + o,
                      lds_ld128(base + sreg + buf * LL::TILE + srow * LL::ROWB + o));
          }
        }
      }
#pragma unroll
      for (int q = 0; q < 2; ++q)
        if (fold && fp < fpe) {
          facc += fv[q];
          ++fp;
          foff += ES;
        }
      const bool last_of_stage = cur.b == nb - 1 && cur.n == n1 - 1;
      const bool last_of_block = last_of_stage && !(RK2 && (cur.l & 1));
      if (RK2 && last_of_stage && (cur.l & 1)) {  // second -> first RK2 stage of the block: acc *= 2 (exact)
#pragma unroll
        for (int mi = 0; mi < MTW; ++mi) acc[mi][0] *= 2.f, acc[mi][1] *= 2.f;
        accb[0] *= 2.f, accb[1] *= 2.f;
      }
      if (last_of_block) {
        if (l + 2 < L && l + 2 >= lfold) fold_end(l + 2);
        // publish block l's dW tiles and db (write-through; drained at the next band barrier)
        float* slab = slabs + (long)l * slab_stride + (long)blockIdx.x * ES;
        const auto rs = __builtin_amdgcn_make_buffer_rsrc(slab, 0, ES * 4, 0x00020000);
        auto put = [&](int tile, f32x4 v) {
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rs, ((tile * 64 + lane) * 4) * 4, 0, 16);
        };
        if constexpr (PAIR) {  // D = X - Y^T per pair tile: 8 (+1 or 2 tap-4) tiles of the 74
#pragma unroll
          for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
              put(pr.tile(a, b), acc[a][b] * hsb);
          if (pr.self()) {
            put(PairSlab::kSelf + pr.perm(0), acc[8][0] * hsb);  // raw X(4, c, c), c even
            put(PairSlab::kSelf + pr.perm(1), acc[8][1] * hsb);  // X(4, c, c)^T, c odd
          } else {
            put(PairSlab::kTap4 + pr.k4(), (acc[8][0] - acc[8][1]) * hsb);
          }
#pragma unroll
          for (int mi = 0; mi < MTW; ++mi) acc[mi][0] = acc[mi][1] = f32x4{0.f, 0.f, 0.f, 0.f};
        } else {
#pragma unroll
          for (int mi = 0; mi < MTW; ++mi)
#pragma unroll
            for (int oi = 0; oi < 2; ++oi) {
              const int mt = tg * MTW + mi;
              put(mt * 4 + oq + oi, acc[mi][oi] * hsb);
              acc[mi][oi] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
        if (dbw) {
          if (g == 0) {
#pragma unroll
            for (int oi = 0; oi < 2; ++oi) {
              const int ob = PAIR ? pr.perm(oi) : oq + oi;
              __hip_atomic_store((gf32*)(slab + (ES - C) + 16 * ob + lx), hsb * accb[oi][0], __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);
            }
          }
          accb[0] = accb[1] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
      }
      if (wave == 4) ASR_BTR(1, 1, it, 6);
      cur = nxt;
      adv(nxt);
    }
    barrier_vm(0);
  }
  ASR_BCLK(1, 1);
}

// asr_stack_status: read (and with reset, clear) the degraded-wait count in one
// device atomic, into the calling host thread's own result word
__global__ void k_stack_status_take(int reset, unsigned* out) {
  *out = reset ? __hip_atomic_exchange(&g_stack_degraded, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
               : __hip_atomic_load(&g_stack_degraded, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace blk
}  // namespace asr
