// The native single-stage network executor (asr_net_*, include/asr.h): stem, L Euler or RK2 blocks,
// head, loss and the backward of all of it, over one workspace.  (The layer-level C ABI is
// asr_api.hip; the multi-stage executor is asr_stages.hip.)
//
// One function, net_plan, decides which kernel path runs the weight materialisation, the stem and
// the blocks of a configuration.  net_layout sizes the workspace from that plan and both executors
// dispatch on it: nothing else in this file asks a *_supported predicate or reads a variant bit
// that chooses an arm.
//
// Reference call stack replaced: Training.train's
// sess.run(train_step) (training/training.py:578-597) over the graph built by
// get_single_block_resnet_build_function (models/tfkeras_resnets.py:547-602)
// and Training._build_optimizer (training/training.py:283-304).
#include <math.h>

#include <vector>

#include "asr_common.h"
#include "asr_internal.h"

namespace asr {

// ---------------------------------------------------------------------------
// the plan: which path runs a configuration
// ---------------------------------------------------------------------------
// how theta becomes W (and, for an operator that is not antisymmetric, W_bwd)
enum class WPack {
  kKxkF32,    // k x k blocks: the single-layer ABI's pack, all L layers per launch
  kKxkBf16,   // ... in bf16, rounded to nearest
  kBf16Bal,   // 3 x 3 bf16: balanced rounding of the antisymmetric pairs (k_theta_to_w_pack_bal)
  kBf16Near,  // 3 x 3 bf16 to nearest (a variant)
  kF32,       // 3 x 3 fp32
};
// normalisation + conv1 + relu
enum class StemFwd {
  kMfma,     // 3 x 3 conv1 on the matrix cores (stem_fwd_mfma)
  kKxk,      // 5 x 5 / 7 x 7 conv1 on the matrix cores (stem_fwd_kxk)
  kValu,     // stem_forward
  kGeneric,  // k_normalize into L.x0, then conv_f32
};
// conv1's weight gradient
enum class StemWgrad {
  kKxk,      // stem_wgrad_kxk, from dz1 in bf16
  kMfma,     // stem_wgrad_mfma, from dz1 in bf16
  kValu,     // stem_wgrad (applies relu' itself)
  kGeneric,  // make_dz + wgrad_f32 over the normalised input at L.x0
};
enum class BlocksFwd {
  kDeep16,      // C=16, 32 x 32: all L steps in one launch, images resident in LDS
  kStack64,     // C=64 Euler: all L blocks in one launch
  kStack64Rk2,  // C=64 RK2: all 2L stages in one launch
  kPerBlock,    // one launch (RK2: two) per block on BlockKernel
};
enum class BlockKernel {
  kRk2,      // rk2_forward_impl / rk2_backward_slabs (bf16 at W = 32, fp32)
  kKxkBf16,  // convk_bf16
  kKxkF32,   // conv_f32_k
  kConvb,    // bf16 off W = 32: the any-width kernels (column strips at W >= 48)
  kMfma,     // bf16 at W = 32: block_fwd_mfma / block_bwd_mfma
  kF32,      // conv_f32
};
enum class BlocksBwd {
  kDeep16,    // all L blocks in one launch (dx resident in LDS), one slab set per layer
  kStack64,   // C=64: all L blocks (Euler or RK2) in one launch, tile-major or pair-local slabs
  kKxk,       // k x k blocks: one dgrad and one weight-gradient launch per block
  kPerBlock,  // block_backward / rk2_backward_slabs per block
};

// What is requested.  Whether block 0's backward applied the stem's relu' and how many layers' slab
// reductions the stacked launch folded are the kernels' answers at run time (BwdOut, lfold).
struct NetPlan {
  bool inference;  // forward-only workspace (3 activation slots, no backward buffers)
  WPack w_pack;
  StemFwd stem_fwd;
  StemWgrad stem_wgrad;
  bool x0_from_forward;  // the forward leaves the normalised input at L.x0 (else kGeneric's wgrad normalises)
  bool x0_room;          // L.x0 is laid out: every conv1 off the shapes of stem_forward, whichever arm runs it
  BlocksFwd blocks_fwd;   // the training forward
  BlocksFwd blocks_eval;  // asr_net_forward: the C=64 Euler stack on an inference workspace only (two slots)
  BlockKernel blk_kernel;
  BlocksBwd blocks_bwd;
  // kStack64.  Its buffers and theta maps belong to the shape: the per-block variant of that shape keeps them
  bool stack_ws;       // the C=64 bf16 training workspace holds the stacked backward's slabs, counters and map
  bool stack_pair_ws;  // ... and the pull-back from pair-local slabs (antisymmetric operator)
  int stack_grid;      // its workgroups
  bool pair;           // pair-local slabs (the 74 D tiles); else tile-major dW
  bool grow;           // dL/dx_L as one bf16 row per image (the GAP gradient); else the full tensor
  // kStack64 and kPerBlock
  bool blk_fuses;  // the per-block kernel can fuse the stem's relu' and another block's slab reduction (not convb)
  int ro0;         // ask block 0's backward for dz1 = dx1 * [x1 > 0]: the stem's wgrad takes it in bf16
  bool fold;       // pass 1 of a slab reduction rides in the next kernel; else in launches of its own
};

// The stem's backward workspace (the network executor's bwdws area, shared with
// the blocks' BwdWs): dz1 in fp32, conv1's weight-gradient slabs, reduce_and_project's rows.
struct StemWs {
  size_t dz, slabs, red, total;
};

static StemWs stem_ws_layout(long P, int Cin, int C, int K = 3) {
  StemWs w{};
  const long ES1 = (long)K * K * Cin * C + C;
  WsCursor c;
  w.dz = c.take((size_t)P * 4);
  w.slabs = c.take((size_t)kMaxBlockSlabs * ES1 * 4);
  w.red = c.take(reduce_ws_bytes(kMaxBlockSlabs, ES1));
  w.total = c.off;
  return w;
}

struct NetLayout {
  NetPlan plan;
  long ntheta, P, E, wstride;  // wstride in elements of the W dtype
  long off_c1k, off_c1b, off_blk, blk_stride, off_fck, off_fcb, nparams;
  bool sep_bwd;  // operator not antisymmetric: dgrad uses W_bwd = -flip(W)^T
  bool rk2;      // RK2 midpoint blocks (x_mid activations, two masks per block)
  int stages;    // conv applications per block (1 Euler, 2 RK2)
  long grp_stride;  // floats of slab group sums per layer
  size_t grp;  // per-layer slab group sums, projected after the whole backward
  size_t slabs_all;  // fp32: every block's slabs, pass 1 of all blocks in one launch after the loop
  long slab_stride;
  size_t w_src, w_src_bwd, theta_dst, wbuf, wbuf_bwd, x0, acts, xmids, masks, dxa, dxb, dxg, bwdws, slabs2, slabs, red, probs,
      loss_per, dlogits, gap, total;
  long mask_bytes;
  int act_bytes;
  size_t deep_slabs;  // deep16's weight-gradient slabs [L][rows][E+C]
  size_t theta_dst_tm, stack_slabs, stack_done;  // tile-major projection map, [L][grid][E+C] slabs, counters
  size_t theta_dst_pr;  // the pull-back from the pair-local slabs (plan.stack_pair_ws)
  int f32_rows;         // fp32: slab rows of one block application's weight gradient (f32_block_slab_rows)
  size_t grow;        // stacked Euler backward: dL/dx_L as one bf16 row per image (the GAP gradient) [N][C]
  BwdWs bw;           // inside bwdws: one block's backward workspace (asr_conv_backward's layout) ...
  StemWs stem;        // ... and, after the blocks, the stem's
  int k1, kb;         // conv1's and the blocks' kernel size (3, 5 or 7)
  int kxk_rows;       // k x k blocks: the slab rows a block's weight gradient writes
};

// asr_net_config's kernel sizes: 0 means 3
static int net_k1(const asr_net_config* c) { return c->conv1_kernel_size ? c->conv1_kernel_size : 3; }
static int net_kb(const asr_net_config* c) { return c->kernel_size ? c->kernel_size : 3; }

static const char kNetKernelSizes[] =
    "kernel_size and conv1_kernel_size in {0 (= 3), 3, 5, 7}; kernel_size 5 / 7: ASR_PARAM_GENERAL or "
    "ASR_PARAM_REGULAR blocks, Euler integrator, float32 at any shape, bfloat16 at C in {16, 32, 64} and "
    "W in {8, 16, 32}; kernel_size 3 in bfloat16: C in {16, 32, 64, 128, 256} and W == 8 or W % 16 == 0 (RK2: W == 32, "
    "C <= 64)";

static int check_net_kernel_size(const char* field, int k) {
  if (k == 3 || k == 5 || k == 7) return ASR_OK;
  return fail((k < 1 || !(k & 1)) ? ASR_E_ARG : ASR_E_UNSUPPORTED, "%s %d: the network takes %s", field, k,
              kNetKernelSizes);
}

static int net_check(const asr_net_config* c) {
  if (!c) return fail(ASR_E_ARG, "null config");
  ASR_TRY(check_shape(c->N, c->H, c->W, c->C));
  if (c->L < 1 || c->Cin < 1 || c->num_classes < 1)
    return fail(ASR_E_ARG, "bad net config (L=%d Cin=%d K=%d C=%d)", c->L, c->Cin, c->num_classes, c->C);
  if (c->num_classes > 256 || c->C > 256)  // (as asr_stages_check: one workgroup of 256 threads per image)
    return fail(ASR_E_UNSUPPORTED, "the head takes C and num_classes <= 256 (C=%d K=%d)", c->C, c->num_classes);
  if (c->dtype != ASR_F32 && c->dtype != ASR_BF16) return fail(ASR_E_ARG, "bad dtype");
  if (param_is_antisymmetric(c->param_kind, c->antisymmetric) < 0) return ASR_E_ARG;
  if (c->param_kind == ASR_PARAM_3BY3 && !c->antisymmetric)
    return fail(ASR_E_ARG, "the 3by3 parametrisation is always antisymmetric");
  if (c->integrator != ASR_INTEGRATOR_EULER && c->integrator != ASR_INTEGRATOR_RK2)
    return fail(ASR_E_ARG, "bad integrator %d", c->integrator);
  if (c->variant & ~(ASR_VARIANT_NO_FOLD | ASR_VARIANT_STEM_FWD_VALU | ASR_VARIANT_STEM_WGRAD_VALU | ASR_VARIANT_PER_BLOCK_FWD |
                    ASR_VARIANT_PER_BLOCK_BWD | ASR_VARIANT_INFERENCE | ASR_VARIANT_TIMED | ASR_VARIANT_FULL_DXL |
                    ASR_VARIANT_FULL_SLABS | ASR_VARIANT_W_BF16))
    return fail(ASR_E_ARG, "bad variant bits 0x%x", c->variant);
  const int kb = net_kb(c);
  ASR_TRY(check_net_kernel_size("conv1_kernel_size", net_k1(c)));
  ASR_TRY(check_net_kernel_size("kernel_size", kb));
  if (kb != 3) {
    if (c->param_kind == ASR_PARAM_3BY3)
      return fail(ASR_E_ARG, "the 3by3 parametrisation has kernel_size 3 (kernel_size=%d): the network takes %s", kb,
                  kNetKernelSizes);
    if (c->integrator == ASR_INTEGRATOR_RK2)
      return fail(ASR_E_UNSUPPORTED, "RK2 blocks with kernel_size %d: the network takes %s", kb, kNetKernelSizes);
    if (c->dtype == ASR_BF16 && !convk_bf16_supported(kb, c->W, c->C))
      return fail(ASR_E_UNSUPPORTED, "bf16 network with kernel_size %d at C=%d W=%d: the network takes %s", kb, c->C,
                  c->W, kNetKernelSizes);
    return ASR_OK;
  }
  if (c->dtype == ASR_BF16 && !mfma_supported(c->C, c->W)) {
    // off W = 32 the blocks run one by one on the any-width kernels: plain Euler blocks only
    if (!convb_supported(c->W, c->C))
      return fail(ASR_E_UNSUPPORTED,
                  "bf16 network needs C in {16,32,64,128,256} and W == 8 or W %% 16 == 0 (C=%d W=%d)", c->C, c->W);
    if (c->integrator == ASR_INTEGRATOR_RK2)
      return fail(ASR_E_UNSUPPORTED, "bf16 network with RK2 blocks needs W == 32 and C in {16,32,64} (C=%d W=%d)", c->C,
                  c->W);
  }
  return ASR_OK;
}

// The one place that picks the paths of a (checked) configuration: every *_supported predicate and
// every variant bit that chooses an arm is read here.
static NetPlan net_plan(const asr_net_config* c) {
  NetPlan p{};
  const int N = c->N, H = c->H, W = c->W, C = c->C, k1 = net_k1(c);
  const bool bf = c->dtype == ASR_BF16, kxk = net_kb(c) != 3, rk2 = c->integrator == ASR_INTEGRATOR_RK2;
  const bool antisym = param_is_antisymmetric(c->param_kind, c->antisymmetric) != 0;
  const auto bit = [&](int v) { return (c->variant & v) != 0; };
  p.inference = bit(ASR_VARIANT_INFERENCE);

  p.w_pack = kxk  ? (bf ? WPack::kKxkBf16 : WPack::kKxkF32)
             : bf ? (bit(ASR_VARIANT_W_BF16) ? WPack::kBf16Near : WPack::kBf16Bal)
                  : WPack::kF32;

  // the stem: stem_forward's shapes (3 x 3) or the matrix-core k x k conv1 (bf16), else the generic arm
  const bool fast_stem = k1 == 3 && stem_supported(c->Cin, H, W, C);
  const bool stem_kxk = bf && k1 != 3 && stem_kxk_supported(k1, c->Cin, W, C);
  const bool fwd_valu = bit(ASR_VARIANT_STEM_FWD_VALU), wgrad_valu = bit(ASR_VARIANT_STEM_WGRAD_VALU);
  p.stem_fwd = fast_stem && bf && stem_fwd_mfma_supported(c->Cin, H, W, C) && !fwd_valu ? StemFwd::kMfma
               : stem_kxk && !fwd_valu                                                   ? StemFwd::kKxk
               : fast_stem                                                               ? StemFwd::kValu
                                                                                         : StemFwd::kGeneric;
  // (stem_wgrad_mfma's shapes have C in {16, 64}: relu_grad_bf16's n % 8 == 0 holds)
  p.stem_wgrad = stem_kxk && !wgrad_valu ? StemWgrad::kKxk
                 : fast_stem && bf && !wgrad_valu && stem_wgrad_mfma_supported(c->Cin, H, W, C) ? StemWgrad::kMfma
                 : fast_stem                                                                    ? StemWgrad::kValu
                                                                                                : StemWgrad::kGeneric;
  p.x0_from_forward = p.stem_fwd == StemFwd::kGeneric;
  p.x0_room = !fast_stem;
  // a bf16 stem on its own kernels takes dz1 in bf16: block 0's backward is asked to apply relu'
  const bool want_dz1 = (fast_stem || stem_kxk) && bf && !wgrad_valu;

  // the blocks
  const bool deep = !kxk && bf && !rk2 && deep16_supported(H, W, C);
  const bool stack_fwd = !kxk && bf && block_stack_fwd_supported(N, H, W, C) && !bit(ASR_VARIANT_PER_BLOCK_FWD);
  p.blocks_fwd = deep ? BlocksFwd::kDeep16
                 : stack_fwd ? (rk2 ? BlocksFwd::kStack64Rk2 : BlocksFwd::kStack64)
                             : BlocksFwd::kPerBlock;
  p.blocks_eval = deep ? BlocksFwd::kDeep16
                  : stack_fwd && !rk2 && p.inference ? BlocksFwd::kStack64
                                                     : BlocksFwd::kPerBlock;
  p.blk_kernel = rk2                          ? BlockKernel::kRk2
                 : kxk                        ? (bf ? BlockKernel::kKxkBf16 : BlockKernel::kKxkF32)
                 : bf && !mfma_supported(C, W) ? BlockKernel::kConvb
                 : bf                         ? BlockKernel::kMfma
                                              : BlockKernel::kF32;
  p.stack_ws = !kxk && !p.inference && bf && block_stack_bwd_supported(N, H, W, C);
  p.stack_pair_ws = p.stack_ws && antisym;
  p.stack_grid = p.stack_ws ? block_stack_bwd_grid(N) : 0;
  p.blocks_bwd = deep                                            ? BlocksBwd::kDeep16
                 : p.stack_ws && !bit(ASR_VARIANT_PER_BLOCK_BWD) ? BlocksBwd::kStack64
                 : kxk                                           ? BlocksBwd::kKxk
                                                                 : BlocksBwd::kPerBlock;
  const bool fold_on = !bit(ASR_VARIANT_NO_FOLD);
  if (p.blocks_bwd == BlocksBwd::kStack64) {
    p.pair = p.stack_pair_ws && !bit(ASR_VARIANT_FULL_SLABS);
    p.grow = !rk2 && !bit(ASR_VARIANT_FULL_DXL);
    // (RK2: the first block's first stage has the extra term, so the stem's relu' runs separately)
    p.ro0 = want_dz1 && !rk2;
    p.fold = fold_on;
  } else if (p.blocks_bwd == BlocksBwd::kPerBlock) {
    // bf16 off W = 32: convb_backward fuses neither the stem's relu' nor another block's slab reduction
    p.blk_fuses = p.blk_kernel != BlockKernel::kConvb;
    p.ro0 = want_dz1 && !rk2 && p.blk_fuses;
    p.fold = fold_on && p.blk_fuses;
  }
  return p;
}

static NetLayout net_layout(const asr_net_config* c) {
  NetLayout L{};
  const NetPlan& p = L.plan = net_plan(c);
  const int C = c->C, K = c->num_classes;
  L.k1 = net_k1(c);
  L.kb = net_kb(c);
  const bool kxk = L.kb != 3, f32 = c->dtype == ASR_F32;
  const bool deep = p.blocks_fwd == BlocksFwd::kDeep16;
  L.ntheta = theta_count_k(C, L.kb, c->param_kind, c->antisymmetric);
  L.sep_bwd = param_is_antisymmetric(c->param_kind, c->antisymmetric) == 0;
  L.rk2 = c->integrator == ASR_INTEGRATOR_RK2;
  L.stages = L.rk2 ? 2 : 1;
  L.P = (long)c->N * c->H * c->W * C;
  L.E = (long)L.kb * L.kb * C * C;
  L.act_bytes = f32 ? 4 : 2;
  L.wstride = f32 ? L.E : (long)(C / 16) * ((L.kb * L.kb * C + 31) / 32) * 512;
  L.off_c1k = 0;
  L.off_c1b = (long)L.k1 * L.k1 * c->Cin * C;
  L.off_blk = L.off_c1b + C;
  L.blk_stride = L.ntheta + C;
  L.off_fck = L.off_blk + (long)c->L * L.blk_stride;
  L.off_fcb = L.off_fck + (long)C * K;
  L.nparams = L.off_fcb + K;
  L.mask_bytes = asr_mask_bytes(c->N, c->H, c->W, C);
  const bool tr = !p.inference;  // training buffers
  WsCursor ws;
  L.w_src = ws.take((size_t)L.E * 4);
  L.w_src_bwd = ws.take(L.sep_bwd && tr ? (size_t)L.E * 4 : 0);
  L.theta_dst = ws.take((size_t)L.ntheta * 2 * 4);
  L.wbuf = ws.take((size_t)c->L * L.wstride * L.act_bytes);
  L.wbuf_bwd = ws.take(L.sep_bwd && tr ? (size_t)c->L * L.wstride * L.act_bytes : 0);
  L.x0 = ws.take(p.x0_room ? (size_t)c->N * c->H * c->W * c->Cin * 4 : 0);
  // training keeps x_0 .. x_L for the backward; inference ping-pongs (x_0 + 2 slots)
  L.acts = ws.take((size_t)(tr ? c->L + 1 : 3) * L.P * L.act_bytes);
  L.xmids = ws.take(L.rk2 ? (size_t)(tr ? c->L : 1) * L.P * L.act_bytes : 0);
  L.masks = ws.take(tr ? (size_t)L.stages * c->L * L.mask_bytes : 0);  // RK2: mask1 of every block, then mask2
  L.dxa = ws.take(tr ? (size_t)L.P * L.act_bytes : 0);
  L.dxb = ws.take(tr ? (size_t)L.P * L.act_bytes : 0);
  L.dxg = ws.take(L.rk2 && tr ? (size_t)L.P * L.act_bytes : 0);
  // per-block backward workspace (asr_conv_backward layout), reused by the stem.
  // fp32 keeps every block's slabs in slabs_all, sized by the grid its weight
  // gradient runs (not the 512-row maximum): no slab rows here, no slabs2
  // k x k blocks: one slab set in the backward workspace, reduced into the block's group sums right after its launch
  L.kxk_rows = !kxk ? 0 : f32 ? wgrad_f32_chunks(c->N, c->H) : wgradk_bf16_slab_rows(L.kb, c->N, c->H, c->W, C);
  L.f32_rows = f32 && !kxk ? f32_block_slab_rows(c->N, c->H, c->W, C) : 0;
  // bf16 blocks at C in {128, 256}: every slab area by the rows k_wgradbw writes (Euler only there: one stage)
  const int bf_rows = !f32 && !kxk && C > 64 ? bf16_block_slab_rows(c->N, c->H, c->W, C) : kMaxBlockSlabs;
  L.bw = bwd_ws_layout(c->N, c->H, c->W, C, c->dtype, L.stages, L.kb, kxk ? L.kxk_rows : f32 ? 0 : -1);
  L.stem = stem_ws_layout(L.P, c->Cin, C, L.k1);
  L.bwdws = ws.take(tr ? std::max(L.bw.total, L.stem.total) : 0);
  // odd Euler blocks' slabs (even ones use the backward workspace's): a
  // block's slabs stay readable while the next block's kernel reduces them
  L.slabs2 = ws.take(tr && !f32 && !kxk ? (size_t)L.stages * bf_rows * (L.E + C) * 4 : 0);  // every other block's slabs
  const int rows = kxk ? L.kxk_rows : f32 ? L.stages * L.f32_rows : L.stages * bf_rows;
  L.grp_stride = (long)reduce_groups(rows) * (L.E + C);
  L.grp = ws.take(tr ? (size_t)c->L * L.grp_stride * 4 : 0);
  L.slab_stride = (long)rows * (L.E + C);
  L.slabs_all = ws.take(tr && f32 && !kxk ? (size_t)c->L * L.slab_stride * 4 : 0);
  L.deep_slabs = ws.take(deep && tr ? deep16_slab_bytes(c->N, c->L) : 0);
  L.theta_dst_tm = ws.take(p.stack_ws ? (size_t)L.ntheta * 2 * 4 : 0);
  L.theta_dst_pr = ws.take(p.stack_pair_ws ? (size_t)L.ntheta * 2 * 4 : 0);
  L.stack_slabs = ws.take(p.stack_ws ? (size_t)c->L * p.stack_grid * (L.E + C) * 4 : 0);
  L.stack_done = ws.take(p.stack_ws ? (size_t)stack_done_words(c->L) * 4 : 0);
  L.grow = ws.take(p.stack_ws && !L.rk2 ? (size_t)c->N * C * 2 : 0);
  L.probs = ws.take((size_t)c->N * K * 4);
  L.loss_per = ws.take(tr ? (size_t)c->N * 4 : 0);
  L.dlogits = ws.take(tr ? (size_t)c->N * K * 4 : 0);
  L.gap = ws.take(tr ? (size_t)c->N * C * 4 : 0);
  L.total = ws.off;
  return L;
}

// ASR_VARIANT_TIMED: HIP events around the block launches of the last timed
// asr_net_forward / asr_net_forward_backward (asr_net_kernel_times): 0-1 the
// blocks' forward, 2-3 the stacked backward kernel, 3-4 its post-launch slab
// reductions and the projection onto theta.  Measurement only.  The events are
// kept per device (created on that device at its first timed call); on one
// device, timed calls from several host threads at once overwrite each
// other's times (one timing thread per device).
constexpr int kMaxTimedDevices = 64;
struct TimedEvents {
  hipEvent_t ev[5];
  bool made;
  unsigned rec;  // bit i: event i recorded by the last timed call on this device
};
static TimedEvents g_tev[kMaxTimedDevices];

static TimedEvents* timed_events_here() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxTimedDevices) return nullptr;
  return &g_tev[dev];
}

static int timed_event(const asr_net_config* c, int i, hipStream_t s) {
  if (!(c->variant & ASR_VARIANT_TIMED)) return ASR_OK;
  TimedEvents* t = timed_events_here();
  if (!t) return fail(ASR_E_HIP, "ASR_VARIANT_TIMED: no current device (or device id >= %d)", kMaxTimedDevices);
  if (!t->made) {
    for (auto& e : t->ev) ASR_TRY(hip_check(hipEventCreate(&e), "hipEventCreate"));
    t->made = true;
  }
  if (i == 0) t->rec = 0;
  ASR_TRY(hip_check(hipEventRecord(t->ev[i], s), "hipEventRecord"));
  t->rec |= 1u << i;
  return ASR_OK;
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
template <typename Tin>
__global__ void k_normalize(const Tin* __restrict__ img, long n, float mean, float inv_std, int use_norm,
                            float* __restrict__ out) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float v = (float)img[i];
    if (use_norm) v = (v - mean) * inv_std;
    out[i] = v;
  }
}

// the normalised input (v - mean) * inv_std as fp32, at L.x0: the generic stem arms' operand
static int net_normalize(const asr_net_config* c, const NetLayout& L, const void* images, unsigned char* ws,
                         hipStream_t s) {
  const float inv_std = c->use_norm ? 1.f / c->divide_by_stddev : 1.f;
  const long nin = (long)c->N * c->H * c->W * c->Cin;
  float* x0 = (float*)(ws + L.x0);
  const unsigned gn = (unsigned)std::min<long>((nin + 255) / 256, 4096);
  if (c->input_u8)
    hipLaunchKernelGGL(k_normalize<uint8_t>, dim3(gn), dim3(256), 0, s, (const uint8_t*)images, nin, c->subtract_mean,
                       inv_std, c->use_norm, x0);
  else
    hipLaunchKernelGGL(k_normalize<float>, dim3(gn), dim3(256), 0, s, (const float*)images, nin, c->subtract_mean,
                       inv_std, c->use_norm, x0);
  ASR_LAUNCH_CHECK("k_normalize");
  return ASR_OK;
}

// One forward's operands.  Training keeps every activation (x_l in slot l); evaluation ping-pongs: the per-block
// kernels and deep16 over slots 0-1 (x_l in slot l & 1), the C=64 stack over slots 1-2 of the inference layout.
struct NetFwd {
  const asr_net_config* c;
  const NetLayout& L;
  const float* params;
  bool training;
  unsigned char* ws;
  hipStream_t s;
  unsigned char* slot(int i) const { return ws + L.acts + (size_t)i * L.P * L.act_bytes; }
  unsigned char* act(int l) const { return slot(training ? l : (l & 1)); }
  const float* bias(int l) const { return params + L.off_blk + (long)l * L.blk_stride + L.ntheta; }
};

// 1. W for all L blocks, one launch; training with an operator that is not antisymmetric: W_bwd as well,
// from the transposed map and without the gamma term.  It is -flip(W)^T of the W just packed, entry for
// entry: round to nearest gives that by itself, the balanced pack as a mirror job (PackJob::mirror)
static int net_materialise_w(const NetFwd& f) {
  const asr_net_config* c = f.c;
  const NetLayout& L = f.L;
  const float* th = f.params + L.off_blk;
  for (int bwd = 0; bwd < (f.training && L.sep_bwd ? 2 : 1); ++bwd) {
    const int32_t* src = (const int32_t*)(f.ws + (bwd ? L.w_src_bwd : L.w_src));
    unsigned char* w = f.ws + (bwd ? L.wbuf_bwd : L.wbuf);
    const float gamma = bwd ? 0.f : c->gamma;
    switch (L.plan.w_pack) {
      case WPack::kKxkBf16:
        ASR_TRY(asr_theta_to_w_k_bf16(th, L.blk_stride, c->L, c->C, L.kb, src, gamma, w, L.wstride, f.s));
        break;
      case WPack::kKxkF32:
        ASR_TRY(asr_theta_to_w_k(th, L.blk_stride, c->L, c->C, L.kb, src, gamma, (float*)w, L.wstride, f.s));
        break;
      case WPack::kBf16Bal:
      case WPack::kBf16Near: {
        // (W of a map known to pair its entries: theta read coalesced through theta_dst, PackJob)
        const bool paired = !bwd && c->param_kind != ASR_PARAM_REGULAR;
        ASR_TRY(theta_to_w_bf16(th, L.blk_stride, c->L, c->C, src, gamma, w, L.wstride,
                                L.plan.w_pack == WPack::kBf16Bal, f.s,
                                paired ? (const int32_t*)(f.ws + L.theta_dst) : nullptr, bwd ? 0 : L.ntheta,
                                bwd != 0));
        break;
      }
      case WPack::kF32:
        ASR_TRY(asr_theta_to_w(th, L.blk_stride, c->L, c->C, src, gamma, w, L.wstride, c->dtype, f.s));
        break;
    }
  }
  return ASR_OK;
}

// 2. normalisation + conv1 + relu (tfkeras_resnets.py:555-572) -> x_0
static int net_stem_forward(const NetFwd& f, const void* images) {
  const asr_net_config* c = f.c;
  const NetLayout& L = f.L;
  const int C = c->C, N = c->N, H = c->H, W = c->W;
  const int out_bf16 = c->dtype == ASR_BF16 ? 1 : 0;
  const float inv_std = c->use_norm ? 1.f / c->divide_by_stddev : 1.f;
  const float *w1 = f.params + L.off_c1k, *b1 = f.params + L.off_c1b;
  switch (L.plan.stem_fwd) {
    case StemFwd::kMfma:
      return stem_fwd_mfma(images, c->input_u8, w1, b1, N, H, W, c->Cin, C, c->subtract_mean, inv_std, c->use_norm,
                           f.act(0), f.s);
    case StemFwd::kKxk:
      return stem_fwd_kxk(L.k1, images, c->input_u8, w1, b1, N, H, W, c->Cin, C, c->subtract_mean, inv_std,
                          c->use_norm, f.act(0), f.s);
    case StemFwd::kValu:
      return stem_forward(images, c->input_u8, w1, b1, N, H, W, c->Cin, C, c->subtract_mean, inv_std, c->use_norm,
                          f.act(0), out_bf16, f.s);
    case StemFwd::kGeneric:
      ASR_TRY(net_normalize(c, L, images, f.ws, f.s));
      return conv_f32(F_RELU, f.ws + L.x0, f.act(0), nullptr, w1, b1, 1.f, 0.f, nullptr, N, H, W, c->Cin, C, out_bf16,
                      f.s, nullptr, L.k1);
  }
  return fail(ASR_E_ARG, "net_stem_forward: bad plan");
}

// 3. the L blocks (tfkeras_resnets.py:579-582 -> :28-94), one function per arm; *xL: where x_L is
static int net_fwd_deep16(const NetFwd& f, unsigned char** xL) {
  const asr_net_config* c = f.c;
  const NetLayout& L = f.L;
  *xL = f.act(c->L);
  return deep16_forward(f.act(0), f.act(f.training ? 1 : c->L), L.P, f.training ? (uint8_t*)(f.ws + L.masks) : nullptr,
                        L.mask_bytes, f.ws + L.wbuf, f.bias(0), L.blk_stride, c->h, c->N, c->L, f.training, f.s);
}

// whole images per workgroup; evaluation ping-pongs x_l between slots 1 and 2 with no relu masks
static int net_fwd_stack64(const NetFwd& f, unsigned char** xL) {
  const asr_net_config* c = f.c;
  const NetLayout& L = f.L;
  if (f.training) {
    *xL = f.slot(c->L);
    return block_stack_fwd_mfma(f.slot(0), f.slot(1), (long)L.P, (uint8_t*)(f.ws + L.masks), (long)L.mask_bytes,
                                f.ws + L.wbuf, (long)L.wstride, f.bias(0), L.blk_stride, c->h, c->N, c->H, c->W, c->C,
                                c->L, f.s);
  }
  *xL = f.slot(1 + (c->L - 1) % 2);
  return block_stack_fwd_mfma(f.slot(0), f.slot(1), (long)L.P, nullptr, 0, f.ws + L.wbuf, (long)L.wstride, f.bias(0),
                              L.blk_stride, c->h, c->N, c->H, c->W, c->C, c->L, f.s, 2);
}

static int net_fwd_stack64_rk2(const NetFwd& f, unsigned char** xL) {  // (training only)
  const asr_net_config* c = f.c;
  const NetLayout& L = f.L;
  uint8_t* m1 = (uint8_t*)(f.ws + L.masks);
  *xL = f.slot(c->L);
  return block_stack_fwd_rk2_mfma(f.slot(0), f.slot(1), f.ws + L.xmids, (long)L.P, m1,
                                  m1 + (size_t)c->L * L.mask_bytes, (long)L.mask_bytes, f.ws + L.wbuf, (long)L.wstride,
                                  f.bias(0), L.blk_stride, c->h, c->N, c->H, c->W, c->C, c->L, f.s);
}

static int net_fwd_blocks(const NetFwd& f, unsigned char** xL) {
  const asr_net_config* c = f.c;
  const NetLayout& L = f.L;
  const int C = c->C, N = c->N, H = c->H, W = c->W;
  *xL = f.act(c->L);
  for (int l = 0; l < c->L; ++l) {
    const float* bias = f.bias(l);
    const unsigned char* wl = f.ws + L.wbuf + (size_t)l * L.wstride * L.act_bytes;
    uint8_t* mask = f.training ? (uint8_t*)(f.ws + L.masks) + (size_t)l * L.mask_bytes : nullptr;
    unsigned char *x = f.act(l), *y = f.act(l + 1);
    switch (L.plan.blk_kernel) {
      case BlockKernel::kRk2: {
        unsigned char* xm = f.ws + L.xmids + (f.training ? (size_t)l * L.P * L.act_bytes : 0);
        uint8_t* mask2 = f.training ? mask + (size_t)c->L * L.mask_bytes : nullptr;
        ASR_TRY(rk2_forward_impl(x, xm, y, mask, mask2, wl, bias, c->h, N, H, W, C, c->dtype, f.s));
        break;
      }
      case BlockKernel::kKxkBf16:
        ASR_TRY(convk_bf16(F_EULER, L.kb, x, y, mask, wl, bias, c->h, 0.f, nullptr, N, H, W, C, f.s));
        break;
      case BlockKernel::kKxkF32:
        ASR_TRY(conv_f32_k(F_EULER, L.kb, x, y, mask, (const float*)wl, bias, c->h, 0.f, nullptr, N, H, W, C, f.s,
                           nullptr));
        break;
      case BlockKernel::kConvb:
        ASR_TRY(convb_forward(x, y, mask, wl, bias, c->h, N, H, W, C, f.s));
        break;
      case BlockKernel::kMfma:
        ASR_TRY(block_fwd_mfma(0, x, nullptr, y, mask, wl, bias, c->h, N, H, W, C, f.s));
        break;
      case BlockKernel::kF32:
        ASR_TRY(conv_f32(F_EULER, x, y, mask, (const float*)wl, bias, c->h, 0.f, nullptr, N, H, W, C, C, 0, f.s));
        break;
    }
  }
  return ASR_OK;
}

static int net_forward_impl(const asr_net_config* c, const NetLayout& L, const float* params, const void* images,
                            bool training, unsigned char* ws, hipStream_t s, unsigned char** xL) {
  if (training && L.plan.inference)
    return fail(ASR_E_ARG, "an ASR_VARIANT_INFERENCE workspace has no training buffers");
  const NetFwd f{c, L, params, training, ws, s};
  ASR_TRY(net_materialise_w(f));
  ASR_TRY(net_stem_forward(f, images));
  ASR_TRY(timed_event(c, 0, s));
  switch (training ? L.plan.blocks_fwd : L.plan.blocks_eval) {
    case BlocksFwd::kDeep16: ASR_TRY(net_fwd_deep16(f, xL)); break;
    case BlocksFwd::kStack64: ASR_TRY(net_fwd_stack64(f, xL)); break;
    case BlocksFwd::kStack64Rk2: ASR_TRY(net_fwd_stack64_rk2(f, xL)); break;
    case BlocksFwd::kPerBlock: ASR_TRY(net_fwd_blocks(f, xL)); break;
  }
  return timed_event(c, 1, s);
}

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------
// What every backward arm is handed: d0 holds dL/dx_L (plan.grow: the row per image at L.grow instead) and d1 is
// the other dx buffer; the dgrad operator (W itself when it is antisymmetric, A^T = -A + 2 gamma I; else W_bwd
// without the gamma term); theta's map; where [dtheta | dbias] of the blocks go.
struct NetBwd {
  const asr_net_config* c;
  const NetLayout& L;
  unsigned char* b;
  hipStream_t s;
  unsigned char *d0, *d1;
  const unsigned char* w_bwd;
  float gamma, two_gamma;
  const int32_t* theta_dst;
  float* dblocks;
  unsigned char* act(int l) const { return b + L.acts + (size_t)l * L.P * L.act_bytes; }
  const uint8_t* mask(int l) const { return (const uint8_t*)(b + L.masks) + (size_t)l * L.mask_bytes; }
  const unsigned char* w(int l) const { return w_bwd + (size_t)l * L.wstride * L.act_bytes; }
};
// What it answers: the buffer that holds dx_1 (the gradient entering the stem's relu), and whether block 0's
// kernel already turned it into dz1 = dx1 * [x1 > 0]
struct BwdOut {
  unsigned char* dx;
  int relu_done;
};

// C=16: all L blocks in one launch (dx resident in LDS), one slab set per layer
// (fused_stage_backward's deep16 sequence written out: timed event 3 sits between the kernel and its reductions)
static int net_bwd_deep16(const NetBwd& a, BwdOut* out) {
  const asr_net_config* c = a.c;
  const NetLayout& L = a.L;
  int rows = 0, in_b = 0;
  float* slabs = (float*)(a.b + L.deep_slabs);
  float* grp = (float*)(a.b + L.grp);
  ASR_TRY(deep16_backward(a.d0, a.d1, a.act(0), L.P, a.mask(0), L.mask_bytes, a.w_bwd, c->h, a.two_gamma, c->N, c->L,
                          slabs, &rows, &in_b, a.s));
  ASR_TRY(timed_event(c, 3, a.s));
  const int G = reduce_groups(rows);
  ASR_TRY(reduce_slabs_to_groups(slabs, c->L * rows, L.E + c->C, grp, a.s));
  ASR_TRY(project_layers(grp, (long)G * (L.E + c->C), G, L.E, c->C, a.theta_dst, L.ntheta, c->L, a.dblocks,
                         L.blk_stride, a.s));
  *out = {in_b ? a.d1 : a.d0, 0};
  return timed_event(c, 4, a.s);
}

// C=64: all L blocks (Euler or RK2) in one launch, tile-major or pair-local slabs; dx_1 ends in the buffer L's
// parity picks
static int net_bwd_stack64(const NetBwd& a, BwdOut* out) {
  const asr_net_config* c = a.c;
  const NetLayout& L = a.L;
  const NetPlan& p = L.plan;
  const int grid = p.stack_grid;
  const long ES = stack_slab_floats(c->C, p.pair ? 1 : 0), sst = (long)grid * ES;
  float* slabs = (float*)(a.b + L.stack_slabs);
  float* grp = (float*)(a.b + L.grp);
  unsigned* done = (unsigned*)(a.b + L.stack_done);
  int lfold = c->L;
  ASR_TRY(block_stack_bwd_mfma(a.d0, a.d1, a.act(0), L.P, a.mask(0), L.mask_bytes, a.w_bwd, L.wstride, c->h,
                               a.two_gamma, c->N, c->H, c->W, c->C, c->L, p.ro0, slabs, sst, grp, L.grp_stride, done,
                               &lfold, a.s, L.rk2 ? a.b + L.xmids : nullptr, L.rk2 ? a.mask(c->L) : nullptr,
                               L.rk2 ? a.b + L.dxg : nullptr, p.grow ? a.b + L.grow : nullptr, p.fold ? 1 : 0,
                               p.pair ? 1 : 0));
  ASR_TRY(timed_event(c, 3, a.s));
  // pass 1 of the blocks below lfold, and of any block whose in-launch fold was
  // flagged (a workgroup's wait ran out), before the projection reads them
  ASR_TRY(stack_bwd_reduce_rest(slabs, sst, grid, ES, grp, L.grp_stride, c->L, lfold, done, a.s));
  ASR_TRY(project_layers(grp, L.grp_stride, reduce_groups(grid), ES - c->C, c->C,
                         (const int32_t*)(a.b + (p.pair ? L.theta_dst_pr : L.theta_dst_tm)), L.ntheta, c->L, a.dblocks,
                         L.blk_stride, a.s));
  *out = {(c->L & 1) ? a.d1 : a.d0, p.ro0};
  return timed_event(c, 4, a.s);
}

// pass 2 of every block's weight-gradient reduction (G group rows a layer) + projection onto theta, one launch
// (per-block kernels: their slab passes ride inside timed events 2-3)
static int net_project_blocks(const NetBwd& a, int G) {
  const NetLayout& L = a.L;
  ASR_TRY(timed_event(a.c, 3, a.s));
  ASR_TRY(project_layers((float*)(a.b + L.grp), L.grp_stride, G, L.E, a.c->C, a.theta_dst, L.ntheta, a.c->L, a.dblocks,
                         L.blk_stride, a.s));
  return timed_event(a.c, 4, a.s);
}

// k x k blocks: one dgrad and one weight-gradient launch per block, pass 1 of its slabs right behind
static int net_bwd_kxk(const NetBwd& a, BwdOut* out) {
  const asr_net_config* c = a.c;
  const NetLayout& L = a.L;
  const int C = c->C, N = c->N, H = c->H, W = c->W;
  float* slabs = (float*)(a.b + L.bwdws + L.bw.slabs);
  float* dz = (float*)(a.b + L.bwdws + L.bw.dz);
  unsigned char *dcur = a.d0, *dnext = a.d1;
  int nsl = 0;
  for (int l = c->L - 1; l >= 0; --l) {
    if (L.plan.blk_kernel == BlockKernel::kKxkBf16) {
      ASR_TRY(convk_bf16(B_EULER, L.kb, dcur, dnext, nullptr, a.w(l), nullptr, c->h, a.two_gamma, a.mask(l), N, H, W,
                         C, a.s));
      ASR_TRY(wgradk_bf16(L.kb, a.act(l), dcur, a.mask(l), c->h, N, H, W, C, slabs, &nsl, a.s));
    } else {
      ASR_TRY(make_dz(F_EULER, dcur, a.mask(l), nullptr, c->h, N, H, W, C, 0, dz, a.s));
      ASR_TRY(conv_f32_k(B_EULER, L.kb, dz, dnext, nullptr, (const float*)a.w(l), nullptr, c->h, a.two_gamma,
                         (const float*)dcur, N, H, W, C, a.s, nullptr));
      ASR_TRY(wgrad_f32(a.act(l), 0, dz, N, H, W, C, C, slabs, &nsl, a.s, L.kb));
    }
    if (nsl < 1 || nsl > L.kxk_rows)  // (the device differs from the one the workspace was sized on)
      return fail(ASR_E_WORKSPACE, "k x k block %d wrote %d slab rows, the workspace holds %d", l, nsl, L.kxk_rows);
    ASR_TRY(reduce_slabs_to_groups(slabs, nsl, L.E + C, (float*)(a.b + L.grp) + (size_t)l * L.grp_stride, a.s));
    std::swap(dcur, dnext);
  }
  *out = {dcur, 0};
  return net_project_blocks(a, reduce_groups(nsl));
}

// One launch (RK2: two) per block, last block first.  bf16: a block's slabs alternate between two buffers; pass 1
// of the previous (deeper) block's reduction rides in this block's (second-stage) kernel when it can (else it
// runs here), and this block's waits for the next block (or the end of the loop).  fp32: every block keeps its
// own slabs; one launch reduces them all after the loop.
static int net_bwd_blocks(const NetBwd& a, BwdOut* out) {
  const asr_net_config* c = a.c;
  const NetLayout& L = a.L;
  const NetPlan& p = L.plan;
  const int C = c->C, N = c->N, H = c->H, W = c->W;
  const bool bf = c->dtype == ASR_BF16;
  float* dz = (float*)(a.b + L.bwdws + L.bw.dz);
  unsigned char *dcur = a.d0, *dnext = a.d1;
  const float* pend_slabs = nullptr;  // the slabs whose pass-1 reduction is still pending
  int pend_P = 0;
  float* pend_grp = nullptr;
  int nsl = 0, relu_done = 0;
  for (int l = c->L - 1; l >= 0; --l) {
    float* slabs_l = !bf ? (float*)(a.b + L.slabs_all) + (size_t)l * L.slab_stride
                         : (float*)(a.b + ((l & 1) ? L.slabs2 : L.bwdws + L.bw.slabs));
    int folded = 0;
    if (p.blk_kernel == BlockKernel::kRk2) {
      const unsigned char* xm = a.b + L.xmids + (size_t)l * L.P * L.act_bytes;
      ASR_TRY(rk2_backward_slabs(dcur, a.act(l), xm, a.mask(l), a.mask(c->L + l), a.w(l), c->h, a.gamma, N, H, W, C,
                                 c->dtype, dnext, a.b + L.dxg, true, slabs_l, dz, &nsl, a.s,
                                 p.fold ? pend_slabs : nullptr, p.fold ? pend_P : 0, pend_grp, &folded));
    } else {
      ASR_TRY(block_backward(ASR_MODE_EULER, dcur, a.act(l), a.mask(l), a.w(l), c->h, a.gamma, N, H, W, C, c->dtype,
                             dnext, true, nullptr, false, slabs_l, dz, &nsl, a.s, l == 0 && p.ro0,
                             l == 0 ? &relu_done : nullptr, p.fold ? pend_slabs : nullptr, p.fold ? pend_P : 0,
                             pend_grp, &folded));
    }
    std::swap(dcur, dnext);
    if (!bf) {
      if (nsl > L.stages * L.f32_rows)  // (the device differs from the one the workspace was sized on)
        return fail(ASR_E_WORKSPACE, "fp32 block %d wrote %d slab rows, the workspace holds %d (sized on another device?)",
                    l, nsl, L.stages * L.f32_rows);
      continue;
    }
    if (pend_P > 0 && !folded) ASR_TRY(reduce_slabs_to_groups(pend_slabs, pend_P, L.E + C, pend_grp, a.s));
    pend_slabs = slabs_l;
    pend_P = nsl;
    pend_grp = (float*)(a.b + L.grp) + (size_t)l * L.grp_stride;
  }
  if (pend_P > 0) ASR_TRY(reduce_slabs_to_groups(pend_slabs, pend_P, L.E + C, pend_grp, a.s));
  if (!bf && nsl > 0)  // (every block of a network has the same slab count)
    ASR_TRY(reduce_slab_layers((const float*)(a.b + L.slabs_all), L.slab_stride, nsl, L.E + C, (float*)(a.b + L.grp),
                               L.grp_stride, c->L, a.s));
  *out = {dcur, relu_done};
  return net_project_blocks(a, reduce_groups(nsl));
}

// stem: dz1 = dx1 * [x1 > 0]; conv1 weight/bias gradient from the normalised input
static int net_stem_backward(const NetBwd& a, const BwdOut& d, const void* images, float* grads) {
  const asr_net_config* c = a.c;
  const NetLayout& L = a.L;
  const int C = c->C, N = c->N, H = c->H, W = c->W;
  const int bf = c->dtype == ASR_BF16 ? 1 : 0;
  float* dz = (float*)(a.b + L.bwdws + L.stem.dz);
  float* slabs = (float*)(a.b + L.bwdws + L.stem.slabs);
  float* red = (float*)(a.b + L.bwdws + L.stem.red);
  const float inv_std = c->use_norm ? 1.f / c->divide_by_stddev : 1.f;
  int nsl = 0;
  switch (L.plan.stem_wgrad) {
    case StemWgrad::kKxk:  // the k x k conv1 on the matrix cores, from dz1 in bf16
      if (!d.relu_done) ASR_TRY(relu_grad_bf16(d.dx, a.act(0), L.P, a.s));
      ASR_TRY(stem_wgrad_kxk(L.k1, images, c->input_u8, d.dx, N, H, W, c->Cin, C, c->subtract_mean, inv_std,
                             c->use_norm, slabs, &nsl, a.s));
      break;
    case StemWgrad::kMfma:
      if (!d.relu_done) ASR_TRY(relu_grad_bf16(d.dx, a.act(0), L.P, a.s));
      ASR_TRY(stem_wgrad_mfma(images, c->input_u8, d.dx, N, H, W, c->Cin, C, c->subtract_mean, inv_std, c->use_norm,
                              slabs, &nsl, a.s));
      break;
    case StemWgrad::kValu:  // (masking an already-masked dz1 again is exact)
      ASR_TRY(stem_wgrad(images, c->input_u8, d.dx, a.act(0), bf, N, H, W, c->Cin, C, c->subtract_mean, inv_std,
                         c->use_norm, slabs, &nsl, a.s));
      break;
    case StemWgrad::kGeneric:
      if (!L.plan.x0_from_forward) ASR_TRY(net_normalize(c, L, images, a.b, a.s));
      ASR_TRY(make_dz(F_RELU, d.dx, nullptr, a.act(0), 1.f, N, H, W, C, bf, dz, a.s));
      ASR_TRY(wgrad_f32(a.b + L.x0, 0, dz, N, H, W, c->Cin, C, slabs, &nsl, a.s, L.k1));
      break;
  }
  return reduce_and_project(slabs, nsl, (long)L.k1 * L.k1 * c->Cin * C, C, nullptr, 0, nullptr, grads + L.off_c1b,
                            grads + L.off_c1k, red, a.s);
}

}  // namespace asr

using namespace asr;

extern "C" {

long asr_net_param_count(const asr_net_config* cfg) {
  if (net_check(cfg) != ASR_OK) return -1;
  return net_layout(cfg).nparams;
}

size_t asr_net_workspace_bytes(const asr_net_config* cfg) {
  if (net_check(cfg) != ASR_OK) return 0;
  return net_layout(cfg).total;
}

int asr_net_prepare(const asr_net_config* cfg, void* ws, size_t ws_bytes) {
  ASR_TRY(net_check(cfg));
  const NetLayout L = net_layout(cfg);
  if (!ws || ws_bytes < L.total) return fail(ASR_E_WORKSPACE, "asr_net_prepare: workspace too small");
  ASR_TRY(check_ws_device(ws, "asr_net_prepare"));
  std::vector<int32_t> w_src((size_t)L.E), theta_dst((size_t)L.ntheta * 2);
  ASR_TRY(param_map_k(cfg->C, L.kb, cfg->param_kind, cfg->antisymmetric, w_src.data(), theta_dst.data()));
  unsigned char* b = (unsigned char*)ws;
  if (L.sep_bwd && !L.plan.inference) {
    std::vector<int32_t> w_bwd((size_t)L.E);
    ASR_TRY(param_map_transpose_k(cfg->C, L.kb, w_src.data(), w_bwd.data()));
    ASR_TRY(hip_check(hipMemcpy(b + L.w_src_bwd, w_bwd.data(), w_bwd.size() * 4, hipMemcpyHostToDevice), "hipMemcpy"));
  }
  ASR_TRY(hip_check(hipMemcpy(b + L.w_src, w_src.data(), w_src.size() * 4, hipMemcpyHostToDevice), "hipMemcpy"));
  ASR_TRY(hip_check(hipMemcpy(b + L.theta_dst, theta_dst.data(), theta_dst.size() * 4, hipMemcpyHostToDevice),
                    "hipMemcpy"));
  if (L.plan.stack_pair_ws) {  // the same pull-back from k_bwd3_stack's pair-local D slabs
    std::vector<int32_t> pr(theta_dst.size());
    ASR_TRY(theta_dst_pair_host(theta_dst.data(), L.ntheta, cfg->C, pr.data()));
    ASR_TRY(hip_check(hipMemcpy(b + L.theta_dst_pr, pr.data(), pr.size() * 4, hipMemcpyHostToDevice), "hipMemcpy"));
  }
  if (L.plan.stack_ws) {  // the same map into k_bwd3_stack's tile-major dW slabs (plan.pair off):
    // entry e = m*C + o of the row-major dW -> ((m/16 * C/16 + o/16) * 64 + 16*((m%16)/4) + o%16) * 4 + m%4
    const int C = cfg->C;
    std::vector<int32_t> tm(theta_dst);
    for (auto& v : tm) {
      if (v < 0) continue;
      const long e = v >> 1, m = e / C, o = e % C;
      const long et = (((m / 16) * (C / 16) + o / 16) * 64 + 16 * ((m % 16) / 4) + o % 16) * 4 + m % 4;
      v = (int32_t)((et << 1) | (v & 1));
    }
    ASR_TRY(hip_check(hipMemcpy(b + L.theta_dst_tm, tm.data(), tm.size() * 4, hipMemcpyHostToDevice), "hipMemcpy"));
  }
  return ASR_OK;
}

int asr_net_forward(const asr_net_config* cfg, const float* params, const void* images, float* probs, void* ws,
                    size_t ws_bytes, asr_stream_t stream) {
  ASR_TRY(net_check(cfg));
  const NetLayout L = net_layout(cfg);
  if (!params || !images || !probs) return fail(ASR_E_ARG, "asr_net_forward: null pointer");
  if (!ws || ws_bytes < L.total) return fail(ASR_E_WORKSPACE, "asr_net_forward: workspace too small");
  ASR_TRY(check_ws_device(ws, "asr_net_forward"));
  hipStream_t s = (hipStream_t)stream;
  unsigned char* b = (unsigned char*)ws;
  unsigned char* xL = nullptr;
  ASR_TRY(net_forward_impl(cfg, L, params, images, false, b, s, &xL));
  ASR_TRY(head(xL, cfg->dtype == ASR_BF16, params + L.off_fck, params + L.off_fcb, nullptr, cfg->N, cfg->H * cfg->W,
               cfg->C, cfg->num_classes, probs, nullptr, nullptr, nullptr, nullptr, s));
  return ASR_OK;
}

int asr_net_check_status(const asr_net_config* cfg, const void* ws, size_t ws_bytes, asr_stream_t stream) {
  ASR_TRY(net_check(cfg));
  const NetLayout L = net_layout(cfg);
  if (!ws || ws_bytes < L.total) return fail(ASR_E_WORKSPACE, "asr_net_check_status: workspace too small");
  ASR_TRY(check_ws_device(ws, "asr_net_check_status"));
  // the stream's own completion status only (hipGetLastError would report, and clear,
  // whatever error another HIP call on this thread left behind)
  return hip_check(hipStreamSynchronize((hipStream_t)stream), "hipStreamSynchronize");
}

int asr_net_kernel_times(float* us) {
  if (!us) return fail(ASR_E_ARG, "asr_net_kernel_times: null output");
  const TimedEvents* t = timed_events_here();
  if (!t || !t->made || !(t->rec & 3u))
    return fail(ASR_E_ARG, "asr_net_kernel_times: no ASR_VARIANT_TIMED call recorded on the current device");
  for (int i = 0; i < 3; ++i) us[i] = -1.f;
  for (int i = 0; i < 3; ++i) {
    const int a = i == 0 ? 0 : i + 1, e = a + 1;
    if ((t->rec >> a & 1u) && (t->rec >> e & 1u)) {
      ASR_TRY(hip_check(hipEventSynchronize(t->ev[e]), "hipEventSynchronize"));
      float ms = 0.f;
      ASR_TRY(hip_check(hipEventElapsedTime(&ms, t->ev[a], t->ev[e]), "hipEventElapsedTime"));
      us[i] = ms * 1e3f;
    }
  }
  return ASR_OK;
}

int asr_net_forward_backward(const asr_net_config* cfg, const float* params, const void* images, const float* targets,
                             float* grads, float* loss, float* probs, void* ws, size_t ws_bytes,
                             asr_stream_t stream) {
  ASR_TRY(net_check(cfg));
  const NetLayout L = net_layout(cfg);
  if (!params || !images || !targets || !grads || !loss) return fail(ASR_E_ARG, "asr_net_forward_backward: null");
  if (!ws || ws_bytes < L.total) return fail(ASR_E_WORKSPACE, "asr_net_forward_backward: workspace too small");
  // before any launch: an inference layout has no backward buffers (its maps for the
  // transposed operator and the training activations are absent)
  if (L.plan.inference)
    return fail(ASR_E_ARG, "asr_net_forward_backward: an ASR_VARIANT_INFERENCE workspace has no training buffers");
  ASR_TRY(check_ws_device(ws, "asr_net_forward_backward"));
  hipStream_t s = (hipStream_t)stream;
  unsigned char* b = (unsigned char*)ws;
  const int C = cfg->C, N = cfg->N, K = cfg->num_classes;
  unsigned char* xL = nullptr;
  ASR_TRY(net_forward_impl(cfg, L, params, images, true, b, s, &xL));
  // head: probabilities, per-image loss, dlogits, dL/dx_L
  const float gamma_bwd = L.sep_bwd ? 0.f : cfg->gamma;
  const NetBwd a{cfg, L, b, s, b + L.dxa, b + L.dxb, b + (L.sep_bwd ? L.wbuf_bwd : L.wbuf), gamma_bwd,
                 2.f * gamma_bwd, (const int32_t*)(b + L.theta_dst), grads + L.off_blk};
  float* probs_ws = probs ? probs : (float*)(b + L.probs);
  // the stacked Euler backward stages its top block's dy from one row per image (the GAP gradient is
  // constant over the pixels): the head writes N x C values instead of the full dL/dx_L tensor
  const bool grow = L.plan.grow;
  ASR_TRY(head(xL, cfg->dtype == ASR_BF16, params + L.off_fck, params + L.off_fcb, targets, N, cfg->H * cfg->W, C, K,
               probs_ws, (float*)(b + L.loss_per), (float*)(b + L.dlogits), (float*)(b + L.gap),
               grow ? nullptr : a.d0, s, grow ? b + L.grow : nullptr));
  ASR_TRY(head_param_grads((const float*)(b + L.gap), (const float*)(b + L.dlogits), N, C, K, grads + L.off_fck,
                           grads + L.off_fcb, (const float*)(b + L.loss_per), loss, s));
  // blocks, last to first
  BwdOut d{};
  ASR_TRY(timed_event(cfg, 2, s));  // (measurement) the blocks' backward starts
  switch (L.plan.blocks_bwd) {
    case BlocksBwd::kDeep16: ASR_TRY(net_bwd_deep16(a, &d)); break;
    case BlocksBwd::kStack64: ASR_TRY(net_bwd_stack64(a, &d)); break;
    case BlocksBwd::kKxk: ASR_TRY(net_bwd_kxk(a, &d)); break;
    case BlocksBwd::kPerBlock: ASR_TRY(net_bwd_blocks(a, &d)); break;
  }
  return net_stem_backward(a, d, images, grads);
}

}  // extern "C"
