// HRDA multi-resolution fusion (rein/models/heads/hrda.py:149-191) on fp32 NHWC logits, forward and backward.
//
//   s     = sigmoid(a)                          a  [B,ha,wa,C]   AttentionHead logits at feature resolution
//   att   = mask * bilinear(s -> h x w)         lr [B,h,w,C]     LinearHead logits of the half-size image; mask = crop box / 8 (1 without a crop)
//   lr'   = (1 - att) * lr
//   F     = up2(att) * hr_ins + up2(lr')        hr [B,hc,wc,C]   placed at (Y0,X0) of the [2h,2w] grid, zero elsewhere
//
// Memory-bound and tiny per element: every thread owns ONE element of the flattened contiguous (b, y, x, c) index (c innermost, so
// a wave reads and writes whole 256-byte runs) and recomputes its small neighbourhood - the 2 x 2 low-resolution taps of an output
// pixel, each from the 2 x 2 taps of `a`.  The adjoint resizes are gathers: a low-resolution element visits the few outputs whose taps
// (clamped edges included) name it, in a fixed order.  No floating-point atomics: two runs are bit-identical.
// All arithmetic is fp32 in both builds of the library (the logits are fp32 in every precision mode).
#include "common.h"

namespace {

struct Tap {
  int i0, i1;
  float l0, l1;
};
// ATen area_pixel_compute_source_index (align_corners=False) + edge clamp, as k_resize_bilinear
__device__ __forceinline__ Tap tap_of(int dst, float scale, int in_size) {
  float src = scale * (dst + 0.5f) - 0.5f;
  if (src < 0.f) src = 0.f;
  Tap r;
  r.i0 = (int)src;
  if (r.i0 > in_size - 1) r.i0 = in_size - 1;
  r.i1 = r.i0 + (r.i0 < in_size - 1 ? 1 : 0);
  r.l1 = src - r.i0;
  r.l0 = 1.f - r.l1;
  return r;
}
// weight with which destination index `dst` of a resize reads source index `i`
__device__ __forceinline__ float tap_weight(int dst, float scale, int in_size, int i) {
  const Tap t = tap_of(dst, scale, in_size);
  return (t.i0 == i ? t.l0 : 0.f) + (t.i1 == i ? t.l1 : 0.f);
}
__device__ __forceinline__ float sigmoidf_(float v) { return 1.f / (1.f + expf(-v)); }

struct Geo {
  int B, h, w, C, ha, wa;      // lr grid, classes, attention grid
  int Y0, X0, hc, wc;          // hr map inside the [2h, 2w] output grid
  int my0, my1, mx0, mx1;      // rows / columns of the lr grid where the attention mask is 1
  float sya, sxa;              // source scales of the attention resize (ha / h, wa / w)
};

// att(y, x, c) = mask * bilinear(sigmoid(a))
__device__ __forceinline__ float att_at(const float* __restrict__ a, const Geo& g, long b, int y, int x, int c) {
  if (y < g.my0 || y >= g.my1 || x < g.mx0 || x >= g.mx1) return 0.f;
  const Tap ty = tap_of(y, g.sya, g.ha), tx = tap_of(x, g.sxa, g.wa);
  const float* ab = a + b * (long)g.ha * g.wa * g.C + c;
  const float s00 = sigmoidf_(ab[((long)ty.i0 * g.wa + tx.i0) * g.C]);
  const float s01 = sigmoidf_(ab[((long)ty.i0 * g.wa + tx.i1) * g.C]);
  const float s10 = sigmoidf_(ab[((long)ty.i1 * g.wa + tx.i0) * g.C]);
  const float s11 = sigmoidf_(ab[((long)ty.i1 * g.wa + tx.i1) * g.C]);
  return ty.l0 * (tx.l0 * s00 + tx.l1 * s01) + ty.l1 * (tx.l0 * s10 + tx.l1 * s11);
}

__global__ void k_hrda_fuse_fwd(const float* __restrict__ lr, const float* __restrict__ a, const float* __restrict__ hr, Geo g,
                                float* __restrict__ fused, float* __restrict__ att_out, float* __restrict__ lrs_out) {
  const int H2 = 2 * g.h, W2 = 2 * g.w;
  const long total = (long)g.B * H2 * W2 * g.C;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % g.C);
    long t = i / g.C;
    const int X = (int)(t % W2);
    t /= W2;
    const int Y = (int)(t % H2);
    const long b = t / H2;
    const Tap ty = tap_of(Y, 0.5f, g.h), tx = tap_of(X, 0.5f, g.w);
    const float* lb = lr + b * (long)g.h * g.w * g.C + c;
    const float a00 = att_at(a, g, b, ty.i0, tx.i0, c), a01 = att_at(a, g, b, ty.i0, tx.i1, c);
    const float a10 = att_at(a, g, b, ty.i1, tx.i0, c), a11 = att_at(a, g, b, ty.i1, tx.i1, c);
    const float l00 = (1.f - a00) * lb[((long)ty.i0 * g.w + tx.i0) * g.C], l01 = (1.f - a01) * lb[((long)ty.i0 * g.w + tx.i1) * g.C];
    const float l10 = (1.f - a10) * lb[((long)ty.i1 * g.w + tx.i0) * g.C], l11 = (1.f - a11) * lb[((long)ty.i1 * g.w + tx.i1) * g.C];
    const float up_att = ty.l0 * (tx.l0 * a00 + tx.l1 * a01) + ty.l1 * (tx.l0 * a10 + tx.l1 * a11);
    const float up_lr = ty.l0 * (tx.l0 * l00 + tx.l1 * l01) + ty.l1 * (tx.l0 * l10 + tx.l1 * l11);
    const int yc = Y - g.Y0, xc = X - g.X0;
    float hv = 0.f;
    if (yc >= 0 && yc < g.hc && xc >= 0 && xc < g.wc) hv = hr[((b * g.hc + yc) * (long)g.wc + xc) * g.C + c];
    fused[i] = up_att * hv + up_lr;
    // the odd output pixel (2y + 1, 2x + 1) has (y, x) as its first tap: it publishes the low-resolution maps, each element once
    if ((Y & 1) && (X & 1)) {
      const long o = ((b * g.h + ty.i0) * (long)g.w + tx.i0) * g.C + c;
      if (att_out) att_out[o] = a00;
      if (lrs_out) lrs_out[o] = l00;
    }
  }
}

// One index space for two independent jobs: [0, n_lr) the low-resolution gathers, [n_lr, n_lr + n_hr) d_hr.
__global__ void k_hrda_fuse_bwd_lr(const float* __restrict__ dF, const float* __restrict__ lr, const float* __restrict__ att,
                                   const float* __restrict__ hr, Geo g, float* __restrict__ d_lr, float* __restrict__ d_att,
                                   float* __restrict__ d_hr) {
  const int H2 = 2 * g.h, W2 = 2 * g.w;
  const long n_lr = (long)g.B * g.h * g.w * g.C, n_hr = (long)g.B * g.hc * g.wc * g.C;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n_lr + n_hr; i += (long)gridDim.x * blockDim.x) {
    if (i < n_lr) {
      const int c = (int)(i % g.C);
      long t = i / g.C;
      const int x = (int)(t % g.w);
      t /= g.w;
      const int y = (int)(t % g.h);
      const long b = t / g.h;
      // up2^T: the outputs 2y - 1 .. 2y + 2 are the only ones whose taps can name y (the clamped border rows name it twice)
      float g_lr = 0.f, g_hr = 0.f;
      for (int Y = max(2 * y - 1, 0); Y <= min(2 * y + 2, H2 - 1); ++Y) {
        const float wy = tap_weight(Y, 0.5f, g.h, y);
        if (wy == 0.f) continue;
        const int yc = Y - g.Y0;
        for (int X = max(2 * x - 1, 0); X <= min(2 * x + 2, W2 - 1); ++X) {
          const float wgt = wy * tap_weight(X, 0.5f, g.w, x);
          if (wgt == 0.f) continue;
          const float d = dF[((b * H2 + Y) * (long)W2 + X) * g.C + c];
          g_lr += wgt * d;
          const int xc = X - g.X0;
          if (yc >= 0 && yc < g.hc && xc >= 0 && xc < g.wc) g_hr += wgt * d * hr[((b * g.hc + yc) * (long)g.wc + xc) * g.C + c];
        }
      }
      const float at = att[i];
      const bool in_mask = y >= g.my0 && y < g.my1 && x >= g.mx0 && x < g.mx1;
      d_lr[i] = (1.f - at) * g_lr;
      d_att[i] = in_mask ? g_hr - lr[i] * g_lr : 0.f;
    } else {
      const long j = i - n_lr;
      const int c = (int)(j % g.C);
      long t = j / g.C;
      const int xc = (int)(t % g.wc);
      t /= g.wc;
      const int yc = (int)(t % g.hc);
      const long b = t / g.hc;
      const int Y = yc + g.Y0, X = xc + g.X0;
      const Tap ty = tap_of(Y, 0.5f, g.h), tx = tap_of(X, 0.5f, g.w);
      const float* ab = att + b * (long)g.h * g.w * g.C + c;
      const float a00 = ab[((long)ty.i0 * g.w + tx.i0) * g.C], a01 = ab[((long)ty.i0 * g.w + tx.i1) * g.C];
      const float a10 = ab[((long)ty.i1 * g.w + tx.i0) * g.C], a11 = ab[((long)ty.i1 * g.w + tx.i1) * g.C];
      const float up_att = ty.l0 * (tx.l0 * a00 + tx.l1 * a01) + ty.l1 * (tx.l0 * a10 + tx.l1 * a11);
      d_hr[j] = up_att * dF[((b * H2 + Y) * (long)W2 + X) * g.C + c];
    }
  }
}

// d_a = (attention resize)^T(d_att) * s (1 - s): an element of `a` visits the rows / columns of the lr grid whose taps can name it
__global__ void k_hrda_fuse_bwd_a(const float* __restrict__ d_att, const float* __restrict__ a, Geo g, float ry, float rx,
                                  float* __restrict__ d_a) {
  const long total = (long)g.B * g.ha * g.wa * g.C;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % g.C);
    long t = i / g.C;
    const int xa = (int)(t % g.wa);
    t /= g.wa;
    const int ya = (int)(t % g.ha);
    const long b = t / g.ha;
    // y reads ya when its source coordinate lies in (ya - 1, ya + 1) (or is clamped onto it): a generous range, exact weights
    int y_lo = (int)floorf((ya - 1.f + 0.5f) * ry - 0.5f) - 1, y_hi = (int)ceilf((ya + 1.f + 0.5f) * ry - 0.5f) + 1;
    int x_lo = (int)floorf((xa - 1.f + 0.5f) * rx - 0.5f) - 1, x_hi = (int)ceilf((xa + 1.f + 0.5f) * rx - 0.5f) + 1;
    if (ya == 0) y_lo = 0;
    if (xa == 0) x_lo = 0;
    if (ya == g.ha - 1) y_hi = g.h - 1;
    if (xa == g.wa - 1) x_hi = g.w - 1;
    y_lo = max(y_lo, max(g.my0, 0)), y_hi = min(y_hi, min(g.my1, g.h) - 1);   // d_att is zero outside the mask
    x_lo = max(x_lo, max(g.mx0, 0)), x_hi = min(x_hi, min(g.mx1, g.w) - 1);
    float acc = 0.f;
    for (int y = y_lo; y <= y_hi; ++y) {
      const float wy = tap_weight(y, g.sya, g.ha, ya);
      if (wy == 0.f) continue;
      const float* row = d_att + ((b * g.h + y) * (long)g.w) * g.C + c;
      float racc = 0.f;
      for (int x = x_lo; x <= x_hi; ++x) racc += tap_weight(x, g.sxa, g.wa, xa) * row[(long)x * g.C];
      acc += wy * racc;
    }
    const float s = sigmoidf_(a[i]);
    d_a[i] = acc * s * (1.f - s);
  }
}

int check_geo(const char* who, int B, int h, int w, int C, int ha, int wa, int hc, int wc, int Y0, int X0, int my0, int my1, int mx0,
              int mx1) {
  VFM_CHECK(B > 0 && h > 0 && w > 0 && C > 0 && ha > 0 && wa > 0 && hc > 0 && wc > 0, VFM_E_SHAPE, "%s: empty shape", who);
  VFM_CHECK(Y0 >= 0 && X0 >= 0 && Y0 + (long)hc <= 2L * h && X0 + (long)wc <= 2L * w, VFM_E_SHAPE,
            "%s: hr map %dx%d at (%d,%d) leaves the %dx%d output grid", who, hc, wc, Y0, X0, 2 * h, 2 * w);
  VFM_CHECK(my0 >= 0 && mx0 >= 0 && my1 <= h && mx1 <= w && my0 <= my1 && mx0 <= mx1, VFM_E_SHAPE, "%s: mask box outside the lr grid", who);
  VFM_CHECK(2L * h < (1L << 30) && 2L * w < (1L << 30), VFM_E_SHAPE, "%s: grid too large", who);
  return VFM_OK;
}
Geo make_geo(int B, int h, int w, int C, int ha, int wa, int hc, int wc, int Y0, int X0, int my0, int my1, int mx0, int mx1) {
  Geo g;
  g.B = B, g.h = h, g.w = w, g.C = C, g.ha = ha, g.wa = wa;
  g.Y0 = Y0, g.X0 = X0, g.hc = hc, g.wc = wc;
  g.my0 = my0, g.my1 = my1, g.mx0 = mx0, g.mx1 = mx1;
  g.sya = (float)ha / (float)h, g.sxa = (float)wa / (float)w;
  return g;
}
int grid_for(long total) { return (int)((total + 255) / 256 > 16384 ? 16384 : (total + 255) / 256); }

}  // namespace

extern "C" int vfm_hrda_fuse_fwd(const float* lr, const float* a, const float* hr, int B, int h, int w, int C, int ha, int wa, int hc,
                                 int wc, int Y0, int X0, int my0, int my1, int mx0, int mx1, float* fused, float* att_out,
                                 float* lr_scaled_out, void* stream) {
  VFM_CHECK(lr && a && hr && fused, VFM_E_INVAL, "vfm_hrda_fuse_fwd: null operand");
  const int rc = check_geo("vfm_hrda_fuse_fwd", B, h, w, C, ha, wa, hc, wc, Y0, X0, my0, my1, mx0, mx1);
  if (rc != VFM_OK) return rc;
  const Geo g = make_geo(B, h, w, C, ha, wa, hc, wc, Y0, X0, my0, my1, mx0, mx1);
  hipLaunchKernelGGL(k_hrda_fuse_fwd, dim3(grid_for(4L * B * h * w * C)), dim3(256), 0, (hipStream_t)stream, lr, a, hr, g, fused,
                     att_out, lr_scaled_out);
  VFM_LAUNCH_CHECK();
  return VFM_OK;
}

extern "C" int vfm_hrda_fuse_bwd(const float* d_fused, const float* lr, const float* a, const float* hr, const float* att, int B, int h,
                                 int w, int C, int ha, int wa, int hc, int wc, int Y0, int X0, int my0, int my1, int mx0, int mx1,
                                 float* d_lr, float* d_a, float* d_hr, float* d_att_ws, void* stream) {
  VFM_CHECK(d_fused && lr && a && hr && att && d_lr && d_a && d_hr && d_att_ws, VFM_E_INVAL, "vfm_hrda_fuse_bwd: null operand");
  const int rc = check_geo("vfm_hrda_fuse_bwd", B, h, w, C, ha, wa, hc, wc, Y0, X0, my0, my1, mx0, mx1);
  if (rc != VFM_OK) return rc;
  const Geo g = make_geo(B, h, w, C, ha, wa, hc, wc, Y0, X0, my0, my1, mx0, mx1);
  hipLaunchKernelGGL(k_hrda_fuse_bwd_lr, dim3(grid_for((long)B * C * ((long)h * w + (long)hc * wc))), dim3(256), 0, (hipStream_t)stream,
                     d_fused, lr, att, hr, g, d_lr, d_att_ws, d_hr);
  VFM_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_hrda_fuse_bwd_a, dim3(grid_for((long)B * ha * wa * C)), dim3(256), 0, (hipStream_t)stream, d_att_ws, a, g,
                     (float)h / (float)ha, (float)w / (float)wa, d_a);
  VFM_LAUNCH_CHECK();
  return VFM_OK;
}
