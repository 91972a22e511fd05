// Device-side image augmentation (asr_augment_batch, include/asr.h): one launch
// turns rows of the HBM-resident dataset array into an augmented batch: gather
// by index, crop, bilinear resize (or resize with zero padding), left-right
// flip, brightness and saturation.  The per-image parameters come from a device
// table the host drew (asr_aug_item); the kernel is a pure function of it.
//
// The kernel is bandwidth-bound with no reuse worth staging in LDS.  The output
// is walked as one flat array in runs of 16 / sizeof(element) pixels per
// thread: with C channels a run is C 16-B stores at a 16-B aligned address
// whatever the row length (4 float pixels of 3 channels = 3 stores, 16 uint8
// pixels of 3 channels = 3 stores); the last npix % run pixels take scalar
// stores.  Sources are read with element-sized loads (1-B for uint8: 3-byte
// pixels and odd image sizes start anywhere), never with a vector load that
// assumes more than the element's alignment.  (The compiler pairs some
// neighbouring byte loads into global_load_ushort at odd addresses and a float32
// pixel's channels into global_load_dwordx3 at 4-B alignment: both rely on
// gfx950 serving unaligned global accesses; the odd-offset tests run them.)
#include "asr_internal.h"

#include <algorithm>

namespace asr {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct AugParams {
  const void* src;
  const asr_aug_item* items;
  void* dst;
  long n_src;
  unsigned npix;  // N * Ho * Wo (< 2^31, checked on the host)
  int Hs, Ws, Ho, Wo;
  int pad, rh, rw, pt, pl;  // pad != 0: the resized extent and its offsets in the output
  int flip_src, op0, op1;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// convert_image_dtype(float -> uint8, saturate=True): * 255.5, clamp, truncate
__device__ __forceinline__ float quant_u8(float v) { return truncf(fminf(fmaxf(v * 255.5f, 0.f), 255.f)); }

// adjust_saturation: RGB -> HSV, s <- clip(s * f, 0, 1), HSV -> RGB (asr.h states the formulas)
__device__ __forceinline__ void saturate_rgb(float& r, float& g, float& b, float f) {
  const float v = fmaxf(r, fmaxf(g, b)), range = v - fminf(r, fminf(g, b));
  float s = v > 0.f ? range / v : 0.f, h = 0.f;
  if (range > 0.f) {
    const float norm = 1.f / (6.f * range);
    h = r == v ? norm * (g - b) : g == v ? norm * (b - r) + 2.f / 6.f : norm * (r - g) + 4.f / 6.f;
    if (h < 0.f) h += 1.f;
  }
  s = fminf(fmaxf(s * f, 0.f), 1.f);
  const float c = s * v, m = v - c, dh = h * 6.f;
  const int cat = (int)dh % 6;  // h == 1 (a tiny negative hue wrapped in float32) is h == 0
  const float x = c * (1.f - fabsf(dh - 2.f * floorf(dh * 0.5f) - 1.f));
  r = m + ((cat == 0 || cat == 5) ? c : (cat == 1 || cat == 4) ? x : 0.f);
  g = m + ((cat == 1 || cat == 2) ? c : (cat == 0 || cat == 3) ? x : 0.f);
  b = m + ((cat == 3 || cat == 4) ? c : (cat == 2 || cat == 5) ? x : 0.f);
}

// One image's table row, read and clamped once per image a run touches (not per pixel).
template <typename TS>
struct AugImage {
  const TS* win;  // the crop window's first element
  int ch, cw;
  bool flip;
  float brightness, saturation;
};

template <typename TS, int C, bool RESIZE>
__device__ __forceinline__ AugImage<TS> aug_image(const AugParams& P, int n) {
  const asr_aug_item it = P.items[n];
  AugImage<TS> im;
  // a bad table cannot read outside the array: the row and the window are clamped into it
  const long row = std::min<long>(std::max<long>(it.src, 0), P.n_src - 1);
  im.ch = RESIZE ? clampi(it.ch, 1, P.Hs) : P.Ho;
  im.cw = RESIZE ? clampi(it.cw, 1, P.Ws) : P.Wo;
  const int y0 = clampi(it.y0, 0, P.Hs - im.ch), x0 = clampi(it.x0, 0, P.Ws - im.cw);
  im.win = (const TS*)P.src + ((size_t)(row * P.Hs + y0) * P.Ws + x0) * C;
  im.flip = it.flip != 0;
  im.brightness = it.brightness;
  im.saturation = it.saturation;
  return im;
}

// One output pixel (y, x) of image im: px[C] on the source's scale; for a uint8 output the values
// are whole numbers in 0..255.
template <typename TS, int C, bool RESIZE>
__device__ __forceinline__ void aug_pixel(const AugParams& P, const AugImage<TS>& im, int y, int x, float (&px)[C]) {
  constexpr bool U8OUT = sizeof(TS) == 1 && !RESIZE;
  const TS* win = im.win;
  const int ch = im.ch, cw = im.cw;
  const bool flip = im.flip;
  if constexpr (!RESIZE) {
    const TS* p = win + ((size_t)y * P.Ws + (flip ? P.Wo - 1 - x : x)) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) px[c] = (float)p[c];
  } else {
    const bool fsrc = flip && P.flip_src;
    int ry = y, rx = (flip && !P.flip_src) ? P.Wo - 1 - x : x, rh = P.Ho, rw = P.Wo;
    if (P.pad) {
      ry -= P.pt;
      rx -= P.pl;
      rh = P.rh;
      rw = P.rw;
    }
    if (ry < 0 || ry >= rh || rx < 0 || rx >= rw) {
#pragma unroll
      for (int c = 0; c < C; ++c) px[c] = 0.f;
    } else {
      // tf.image.resize_images, align_corners=False, legacy coordinates: source = d * (in / out)
      const float sy = (float)ry * ((float)ch / (float)rh), sx = (float)rx * ((float)cw / (float)rw);
      const int ylo = min((int)sy, ch - 1), yhi = min(ylo + 1, ch - 1);
      const int xlo = min((int)sx, cw - 1), xhi = min(xlo + 1, cw - 1);
      const float fy = sy - (float)ylo, fx = sx - (float)xlo;
      const size_t cl = (size_t)(fsrc ? cw - 1 - xlo : xlo) * C, chi = (size_t)(fsrc ? cw - 1 - xhi : xhi) * C;
      const TS* top = win + (size_t)ylo * P.Ws * C;
      const TS* bot = win + (size_t)yhi * P.Ws * C;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float tl = (float)top[cl + c], tr = (float)top[chi + c];
        const float bl = (float)bot[cl + c], br = (float)bot[chi + c];
        const float t = tl + (tr - tl) * fx, b = bl + (br - bl) * fx;
        px[c] = t + (b - t) * fy;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int op = k ? P.op1 : P.op0;
    if (op == ASR_AUG_BRIGHTNESS) {
#pragma unroll
      for (int c = 0; c < C; ++c)
        px[c] = U8OUT ? quant_u8(px[c] * (1.f / 255.f) + im.brightness) : px[c] + im.brightness;
    }
    if constexpr (C == 3) {
      if (op == ASR_AUG_SATURATION) {
        if constexpr (U8OUT) {
          float r = px[0] * (1.f / 255.f), g = px[1] * (1.f / 255.f), b = px[2] * (1.f / 255.f);
          saturate_rgb(r, g, b, im.saturation);
          px[0] = quant_u8(r);
          px[1] = quant_u8(g);
          px[2] = quant_u8(b);
        } else {
          saturate_rgb(px[0], px[1], px[2], im.saturation);
        }
      }
    }
  }
}

template <typename TS, int C, bool RESIZE>
__global__ __launch_bounds__(256) void k_augment(const AugParams P) {
  constexpr bool U8OUT = sizeof(TS) == 1 && !RESIZE;
  constexpr int PG = U8OUT ? 16 : 4;    // pixels of one run: PG * C elements = C 16-B stores
  constexpr int EPW = U8OUT ? 4 : 1;    // elements per 32-bit word
  constexpr int NW = PG * C / EPW;      // = 4 * C words
  const unsigned nruns = P.npix / PG;
  const unsigned tid = blockIdx.x * 256u + threadIdx.x, nthreads = gridDim.x * 256u;
  for (unsigned g = tid; g < nruns; g += nthreads) {
    const unsigned p0 = g * PG;
    int x = (int)(p0 % (unsigned)P.Wo);
    const unsigned q = p0 / (unsigned)P.Wo;
    int y = (int)(q % (unsigned)P.Ho), n = (int)(q / (unsigned)P.Ho);
    AugImage<TS> im = aug_image<TS, C, RESIZE>(P, n);
    uint32_t w[NW];
#pragma unroll
    for (int k = 0; k < NW; ++k) w[k] = 0u;
#pragma unroll
    for (int i = 0; i < PG; ++i) {
      float px[C];
      aug_pixel<TS, C, RESIZE>(P, im, y, x, px);
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const int e = i * C + c;
        if constexpr (U8OUT) w[e / 4] |= (uint32_t)px[c] << (8 * (e % 4));
        else w[e] = __float_as_uint(px[c]);
      }
      if (++x == P.Wo) {
        x = 0;
        if (++y == P.Ho) {  // the run crosses into the next image (the run's last pixel may be the batch's last)
          y = 0;
          if (i + 1 < PG) im = aug_image<TS, C, RESIZE>(P, ++n);
        }
      }
    }
    // 16-B stores of a vector type (one store in the IR from the start: HIP's uint4 is a struct whose members
    // the optimiser regroups by pixel, into 12-B stores).  Not nontemporal: the next kernel reads the batch,
    // and the wide shape measured 69 us with nt stores against 47 us without.
    u32x4* d = (u32x4*)((char*)P.dst + (size_t)g * (16 * C));
#pragma unroll
    for (int k = 0; k < C; ++k) {
      const u32x4 v = {w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]};
      d[k] = v;
    }
  }
  // the last npix % PG pixels, one per thread, scalar stores
  const unsigned p = nruns * PG + tid;
  if (p < P.npix) {
    const unsigned q = p / (unsigned)P.Wo;
    float px[C];
    const AugImage<TS> im = aug_image<TS, C, RESIZE>(P, (int)(q / (unsigned)P.Ho));
    aug_pixel<TS, C, RESIZE>(P, im, (int)(q % (unsigned)P.Ho), (int)(p % (unsigned)P.Wo), px);
#pragma unroll
    for (int c = 0; c < C; ++c) {
      if constexpr (U8OUT) ((uint8_t*)P.dst)[(size_t)p * C + c] = (uint8_t)px[c];
      else ((float*)P.dst)[(size_t)p * C + c] = px[c];
    }
  }
}

template <typename TS, int C, bool RESIZE>
void launch_augment(const AugParams& P, hipStream_t s) {
  const long pg = (sizeof(TS) == 1 && !RESIZE) ? 16 : 4;
  const long work = std::max<long>(P.npix / pg, P.npix % pg);
  const long grid = std::max<long>(1, std::min<long>((work + 255) / 256, 8L * launch_cus()));
  hipLaunchKernelGGL((k_augment<TS, C, RESIZE>), dim3((unsigned)grid), dim3(256), 0, s, P);
}

bool color_op_known(int op) { return op == ASR_AUG_NONE || op == ASR_AUG_BRIGHTNESS || op == ASR_AUG_SATURATION; }

}  // namespace

int augment_batch(const void* src, long n_src, const asr_aug_plan* plan, const asr_aug_item* items, int N, void* dst,
                  hipStream_t s) {
  if (!src || !plan || !items || !dst) return fail(ASR_E_ARG, "asr_augment_batch: null pointer");
  if (N < 1 || n_src < 1) return fail(ASR_E_ARG, "asr_augment_batch: N = %d, n_src = %ld (both >= 1)", N, n_src);
  const asr_aug_plan& p = *plan;
  if (p.Hs < 1 || p.Ws < 1 || p.Ho < 1 || p.Wo < 1)
    return fail(ASR_E_ARG, "asr_augment_batch: source %d x %d, output %d x %d (all >= 1)", p.Hs, p.Ws, p.Ho, p.Wo);
  if (p.src_dtype != ASR_U8 && p.src_dtype != ASR_F32)
    return fail(ASR_E_UNSUPPORTED, "asr_augment_batch: source dtype %d (ASR_U8 or ASR_F32)", p.src_dtype);
  if (p.dst_dtype != ASR_U8 && p.dst_dtype != ASR_F32)
    return fail(ASR_E_UNSUPPORTED, "asr_augment_batch: output dtype %d (ASR_U8 or ASR_F32)", p.dst_dtype);
  if (p.Cch != 1 && p.Cch != 3) return fail(ASR_E_UNSUPPORTED, "asr_augment_batch: %d channels (1 or 3)", p.Cch);
  if (p.resize != ASR_AUG_RESIZE_NONE && p.resize != ASR_AUG_RESIZE_BILINEAR && p.resize != ASR_AUG_RESIZE_PAD)
    return fail(ASR_E_ARG, "asr_augment_batch: resize mode %d", p.resize);
  if (!color_op_known(p.color[0]) || !color_op_known(p.color[1]) ||
      (p.color[0] != ASR_AUG_NONE && p.color[0] == p.color[1]))
    return fail(ASR_E_ARG, "asr_augment_batch: colour operations {%d, %d} (each of none, brightness, saturation once)",
                p.color[0], p.color[1]);
  if (p.Cch != 3 && (p.color[0] == ASR_AUG_SATURATION || p.color[1] == ASR_AUG_SATURATION))
    return fail(ASR_E_UNSUPPORTED, "asr_augment_batch: saturation on %d channel(s) (3 only)", p.Cch);
  const bool resize = p.resize != ASR_AUG_RESIZE_NONE;
  if (!resize && (p.Ho > p.Hs || p.Wo > p.Ws))
    return fail(ASR_E_ARG, "asr_augment_batch: a %d x %d window outside the %d x %d source", p.Ho, p.Wo, p.Hs, p.Ws);
  if (p.resize == ASR_AUG_RESIZE_PAD && (p.rh < 1 || p.rw < 1 || p.pad_top < 0 || p.pad_left < 0 ||
                                         p.pad_top + p.rh > p.Ho || p.pad_left + p.rw > p.Wo))
    return fail(ASR_E_ARG, "asr_augment_batch: resized extent %d x %d at (%d, %d) outside the %d x %d output", p.rh,
                p.rw, p.pad_top, p.pad_left, p.Ho, p.Wo);
  const int want_dst = (p.src_dtype == ASR_U8 && !resize) ? ASR_U8 : ASR_F32;
  if (p.dst_dtype != want_dst)
    return fail(ASR_E_ARG, "asr_augment_batch: output dtype %d, this plan writes %d (uint8 only from uint8 without "
                "a resize)", p.dst_dtype, want_dst);
  const long npix = (long)N * p.Ho * p.Wo;
  if (npix >= (1L << 31))
    return fail(ASR_E_UNSUPPORTED, "asr_augment_batch: %ld output pixels (fewer than 2^31)", npix);
  if (((uintptr_t)dst & 15) || (p.src_dtype == ASR_F32 && ((uintptr_t)src & 3)) || ((uintptr_t)items & 3))
    return fail(ASR_E_ARG, "asr_augment_batch: dst must be 16-B aligned, a float32 src and items 4-B aligned");
  AugParams P;
  P.src = src;
  P.items = items;
  P.dst = dst;
  P.n_src = n_src;
  P.npix = (unsigned)npix;
  P.Hs = p.Hs, P.Ws = p.Ws, P.Ho = p.Ho, P.Wo = p.Wo;
  P.pad = p.resize == ASR_AUG_RESIZE_PAD;
  P.rh = p.rh, P.rw = p.rw, P.pt = p.pad_top, P.pl = p.pad_left;
  P.flip_src = p.flip_src != 0;
  P.op0 = p.color[0], P.op1 = p.color[1];
  const bool u8 = p.src_dtype == ASR_U8;
  if (p.Cch == 3) {
    if (u8) resize ? launch_augment<uint8_t, 3, true>(P, s) : launch_augment<uint8_t, 3, false>(P, s);
    else resize ? launch_augment<float, 3, true>(P, s) : launch_augment<float, 3, false>(P, s);
  } else {
    if (u8) resize ? launch_augment<uint8_t, 1, true>(P, s) : launch_augment<uint8_t, 1, false>(P, s);
    else resize ? launch_augment<float, 1, true>(P, s) : launch_augment<float, 1, false>(P, s);
  }
  ASR_LAUNCH_CHECK("k_augment");
  return ASR_OK;
}

}  // namespace asr

extern "C" int asr_augment_batch(const void* src, long n_src, const asr_aug_plan* plan, const asr_aug_item* items,
                                 int N, void* dst, asr_stream_t stream) {
  return asr::augment_batch(src, n_src, plan, items, N, dst, (hipStream_t)stream);
}
