// Training augmentation on the device: the mmseg / mmcv transform chain of vfmseg_amd/datasets.py after the decode -
// Resize (bilinear) -> RandomCrop -> RandomFlip -> PhotoMetricDistortion - and SegDataPreProcessor's channel swap, normalisation and padding,
// one launch per sample.  The host draws every random number and hands the outcome over as a vfm_augment_plan; this file reproduces the
// host's arithmetic stage by stage, with the host's quantisation to uint8 after every stage, so that the result equals
// vfm_preprocess_u8(host chain's crop).
//
// This file is compiled with -ffp-contract=off (csrc/build.py, EXTRA): the host evaluates every expression below as separately rounded IEEE
// operations, and a contracted a * b + c would round once where numpy rounds twice.  Divisions are true divisions for the same reason.
#include "common.h"

namespace {

struct px3 {
  int c[3];
};

// PhotoMetricDistortion._convert: clip(x * alpha + beta, 0, 255).astype(uint8) - astype truncates.  The host computes it in float32, the
// parameters rounded to float32 first: np.random.uniform returns a Python float, which leaves a float32 array float32 under numpy 1 and 2.
// `wide` is the float64 form, for a host whose probe (datasets.convert_is_wide) finds numpy widening; both are tested.
__device__ __forceinline__ int convert_u8(int x, double alpha, double beta, int wide) {
  if (wide) {
    double v = (double)x * alpha + beta;
    v = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v);
    return (int)v;
  }
  float v = (float)x * (float)alpha + (float)beta;
  v = v < 0.f ? 0.f : (v > 255.f ? 255.f : v);
  return (int)v;
}

__device__ __forceinline__ int clip_u8(float v) { return (int)(v < 0.f ? 0.f : (v > 255.f ? 255.f : v)); }

// datasets.bgr2hsv_u8: float32, the same expressions in the same order; H in [0, 180)
__device__ __forceinline__ px3 bgr2hsv(px3 p) {
  const float b = (float)p.c[0], g = (float)p.c[1], r = (float)p.c[2];
  const float v = fmaxf(fmaxf(r, g), b), mn = fminf(fminf(r, g), b);
  const float diff = v - mn;
  const float s = v > 0.f ? diff / fmaxf(v, 1e-12f) * 255.0f : 0.f;
  const float safe = diff > 0.f ? diff : 1.0f;
  // the branch order of the host: v == r, then v == g.  One division: the three branches differ in the numerator and the offset only
  const float num = v == r ? 60.0f * (g - b) : (v == g ? 60.0f * (b - r) : 60.0f * (r - g));
  const float quo = num / safe;
  float h = v == r ? quo : (v == g ? 120.0f + quo : 240.0f + quo);
  h = diff > 0.f ? h : 0.f;
  h = (h < 0.f ? h + 360.0f : h) / 2.0f;
  float hr = rintf(h);          // half to even
  hr = hr >= 180.f ? hr - 180.f : hr;   // rint(h) is in [0, 180]: % 180
  px3 o;
  o.c[0] = clip_u8(hr);
  o.c[1] = clip_u8(rintf(s));
  o.c[2] = clip_u8(v);
  return o;
}

// datasets.hsv2bgr_u8
__device__ __forceinline__ px3 hsv2bgr(px3 p) {
  const float h = (float)p.c[0] * 2.0f, s = (float)p.c[1] / 255.0f, v = (float)p.c[2];
  const float hd = h / 60.0f;
  const float hf = floorf(hd);
  const float fr = hd - hf;
  const int hi = (int)hf % 6;
  const float pp = v * (1.f - s), q = v * (1.f - s * fr), t = v * (1.f - s * (1.f - fr));
  float r, g, b;
  switch (hi) {
    case 0: r = v, g = t, b = pp; break;
    case 1: r = q, g = v, b = pp; break;
    case 2: r = pp, g = v, b = t; break;
    case 3: r = pp, g = q, b = v; break;
    case 4: r = t, g = pp, b = v; break;
    default: r = v, g = pp, b = q; break;
  }
  px3 o;
  o.c[0] = clip_u8(rintf(b));
  o.c[1] = clip_u8(rintf(g));
  o.c[2] = clip_u8(rintf(r));
  return o;
}

// one axis of F.interpolate(mode="bilinear", align_corners=False) in float32: taps i0, i1 (both inside [0, n)) and the weight of i1
__device__ __forceinline__ void taps(int dst, float scale, int n, int& i0, int& i1, float& w1) {
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  src = src < 0.f ? 0.f : src;
  i0 = min((int)src, n - 1);
  i1 = min(i0 + 1, n - 1);
  const float l = src - (float)i0;
  w1 = l < 0.f ? 0.f : (l > 1.f ? 1.f : l);
}

// the host chain's uint8 BGR pixel at crop position (cy, cx): resize, crop offset, photometric distortion
__device__ __forceinline__ px3 sample(const uint8_t* __restrict__ src, int Hs, int Ws, const vfm_augment_plan& P, float sch, float scw,
                                      int cy, int cx) {
  const int ry = P.crop_y + cy, rx = P.crop_x + cx;   // position in the resized image
  px3 p;
  if (P.resize_h > 0) {
    int y0, y1, x0, x1;
    float wy, wx;
    taps(ry, sch, Hs, y0, y1, wy);
    taps(rx, scw, Ws, x0, x1, wx);
    const uint8_t *a = src + ((long)y0 * Ws + x0) * 3, *b = src + ((long)y0 * Ws + x1) * 3;
    const uint8_t *c = src + ((long)y1 * Ws + x0) * 3, *d = src + ((long)y1 * Ws + x1) * 3;
    const float wy0 = 1.f - wy, wx0 = 1.f - wx;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float top = wx0 * (float)a[k] + wx * (float)b[k];
      const float bot = wx0 * (float)c[k] + wx * (float)d[k];
      p.c[k] = clip_u8(rintf(wy0 * top + wy * bot));
    }
  } else {
    const int y = min(max(ry, 0), Hs - 1), x = min(max(rx, 0), Ws - 1);
    const uint8_t* a = src + ((long)y * Ws + x) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) p.c[k] = a[k];
  }
  // PhotoMetricDistortion.__call__, in its order
  if (P.brightness_on) {
#pragma unroll
    for (int k = 0; k < 3; ++k) p.c[k] = convert_u8(p.c[k], 1.0, P.brightness_beta, P.wide);
  }
  if (P.contrast_on == 1) {
#pragma unroll
    for (int k = 0; k < 3; ++k) p.c[k] = convert_u8(p.c[k], P.contrast_alpha, 0.0, P.wide);
  }
  if (P.saturation_on) {
    px3 h = bgr2hsv(p);
    h.c[1] = convert_u8(h.c[1], P.saturation_alpha, 0.0, P.wide);
    p = hsv2bgr(h);
  }
  if (P.hue_on) {
    px3 h = bgr2hsv(p);
    int t = (h.c[0] + P.hue_delta) % 180;   // Python's %: the result takes the divisor's sign
    h.c[0] = t < 0 ? t + 180 : t;
    p = hsv2bgr(h);
  }
  if (P.contrast_on == 2) {
#pragma unroll
    for (int k = 0; k < 3; ++k) p.c[k] = convert_u8(p.c[k], P.contrast_alpha, 0.0, P.wide);
  }
  return p;
}

// One thread per VEC horizontally adjacent output pixels, all three channels (the HSV steps need them together).
template <int VEC>
__global__ void __launch_bounds__(256) k_augment_u8(const uint8_t* __restrict__ src, int Hs, int Ws, vfm_augment_plan P, float* __restrict__ out,
                                                    int Hp, int Wp, float m0, float m1, float m2, float s0, float s1, float s2, int swap_rb,
                                                    float pad_val) {
  const int wv = Wp / VEC;
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= (long)Hp * wv) return;
  const int y = (int)(i / wv), xb = (int)(i % wv) * VEC;
  const float sch = P.resize_h > 0 ? (float)Hs / (float)P.resize_h : 1.f, scw = P.resize_w > 0 ? (float)Ws / (float)P.resize_w : 1.f;
  float v[3][VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    const int x = xb + j;
    if (y < P.crop_h && x < P.crop_w) {
      const int cy = P.flip == 2 ? P.crop_h - 1 - y : y, cx = P.flip == 1 ? P.crop_w - 1 - x : x;
      const px3 p = sample(src, Hs, Ws, P, sch, scw, cy, cx);
      v[0][j] = ((float)(swap_rb ? p.c[2] : p.c[0]) - m0) / s0;
      v[1][j] = ((float)p.c[1] - m1) / s1;
      v[2][j] = ((float)(swap_rb ? p.c[0] : p.c[2]) - m2) / s2;
    } else {
      v[0][j] = v[1][j] = v[2][j] = pad_val;
    }
  }
  const long plane = (long)Hp * Wp, o = (long)y * Wp + xb;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (VEC == 4) {
      *reinterpret_cast<float4*>(out + c * plane + o) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
    } else {
#pragma unroll
      for (int j = 0; j < VEC; ++j) out[c * plane + o + j] = v[c][j];
    }
  }
}

}  // namespace

extern "C" int vfm_augment_u8(const uint8_t* img, int Hs, int Ws, const vfm_augment_plan* plan, float* out, int Hp, int Wp,
                              const float* mean3, const float* std3, int bgr_to_rgb, float pad_val, void* stream) {
  VFM_CHECK(img && plan && out && mean3 && std3 && Hs > 0 && Ws > 0 && Hp >= 0 && Wp >= 0, VFM_E_SHAPE,
            "vfm_augment_u8: shape (plan / mean3 / std3 are HOST pointers)");
  const vfm_augment_plan P = *plan;
  VFM_CHECK((P.resize_h > 0) == (P.resize_w > 0) && P.resize_h >= 0, VFM_E_SHAPE, "vfm_augment_u8: resize target %d x %d", P.resize_h, P.resize_w);
  const int Hr = P.resize_h > 0 ? P.resize_h : Hs, Wr = P.resize_h > 0 ? P.resize_w : Ws;   // the image the crop box refers to
  VFM_CHECK(P.crop_y >= 0 && P.crop_x >= 0 && P.crop_h > 0 && P.crop_w > 0 && (long)P.crop_y + P.crop_h <= Hr && (long)P.crop_x + P.crop_w <= Wr,
            VFM_E_SHAPE, "vfm_augment_u8: crop box y %d + %d, x %d + %d outside the %d x %d image", P.crop_y, P.crop_h, P.crop_x, P.crop_w, Hr, Wr);
  VFM_CHECK(P.crop_h <= Hp && P.crop_w <= Wp, VFM_E_SHAPE, "vfm_augment_u8: crop %d x %d larger than the output %d x %d", P.crop_h, P.crop_w, Hp, Wp);
  VFM_CHECK(P.flip >= 0 && P.flip <= 2 && P.contrast_on >= 0 && P.contrast_on <= 2, VFM_E_INVAL, "vfm_augment_u8: flip %d / contrast position %d",
            P.flip, P.contrast_on);
  VFM_CHECK((long)Hs * Ws * 3 < (1L << 40) && 3L * Hp * Wp < (1L << 40), VFM_E_SHAPE, "vfm_augment_u8: image too large");
  if ((long)Hp * Wp == 0) return VFM_OK;
  const bool vec = Wp % 4 == 0 && ((uintptr_t)out & 15) == 0;
  const long threads = (long)Hp * (vec ? Wp / 4 : Wp);
  const long grid = (threads + 255) / 256;
  VFM_CHECK(grid < (1L << 31), VFM_E_SHAPE, "vfm_augment_u8: output too large");
  if (vec)
    hipLaunchKernelGGL(k_augment_u8<4>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, img, Hs, Ws, P, out, Hp, Wp, mean3[0], mean3[1],
                       mean3[2], std3[0], std3[1], std3[2], bgr_to_rgb, pad_val);
  else
    hipLaunchKernelGGL(k_augment_u8<1>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, img, Hs, Ws, P, out, Hp, Wp, mean3[0], mean3[1],
                       mean3[2], std3[0], std3[1], std3[2], bgr_to_rgb, pad_val);
  VFM_LAUNCH_CHECK();
  return VFM_OK;
}
