// Evaluation kernels: the confusion histogram behind mmseg IoUMetric.intersect_and_union (rein/dg_metrics.py:46-52 calls it per
// sample).  HBM-bound: 1 B prediction + 1 or 8 B label per pixel, read once with 16-byte loads; counts privatised per wave in LDS,
// one integer atomic per touched bin per block.  Below it, vfm_postprocess_argmax: mmseg's postprocess_result and those counts in one pass.
#include "common.h"

#define NC_MAX 64  // classes on the path: 19 (Cityscapes); rows = num_classes + 1 ("other" labels that are not ignore_index)

template <typename LT>
__global__ __launch_bounds__(256) void k_confusion_hist(const uint8_t* __restrict__ pred, const LT* __restrict__ label, long n, int nc,
                                                        int ignore, unsigned long long* __restrict__ hist) {
  // per-wave private copies: 4 waves x (nc+1) x nc 32-bit counters (19 classes: 4 x 380 x 4 B = 6 KiB)
  extern __shared__ unsigned int sh[];
  const int bins = (nc + 1) * nc;
  const int wave = threadIdx.x >> 6;
  unsigned int* mine = sh + wave * bins;
  for (int i = threadIdx.x; i < 4 * bins; i += 256) sh[i] = 0u;
  __syncthreads();
  // 16 pixels per thread-iteration: one 16-byte load of predictions (and the matching label loads)
  const long n16 = n >> 4;
  for (long v = blockIdx.x * 256L + threadIdx.x; v < n16; v += (long)gridDim.x * 256L) {
    const uint4 p4 = reinterpret_cast<const uint4*>(pred)[v];
    const uint32_t pw[4] = {p4.x, p4.y, p4.z, p4.w};
    int lab[16];
    if constexpr (sizeof(LT) == 1) {
      const uint4 l4 = reinterpret_cast<const uint4*>(label)[v];
      const uint32_t lw[4] = {l4.x, l4.y, l4.z, l4.w};
#pragma unroll
      for (int j = 0; j < 16; ++j) lab[j] = (lw[j >> 2] >> (8 * (j & 3))) & 0xff;
    } else {
      const longlong2* lp = reinterpret_cast<const longlong2*>(label + (v << 4));
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const longlong2 t = lp[j];
        lab[2 * j] = (int)t.x;
        lab[2 * j + 1] = (int)t.y;
      }
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int p = (pw[j >> 2] >> (8 * (j & 3))) & 0xff;
      const int l = lab[j];
      if (l != ignore && p < nc) atomicAdd(&mine[((l >= 0 && l < nc) ? l : nc) * nc + p], 1u);
    }
  }
  // tail pixels (n % 16) by the first threads of block 0
  if (blockIdx.x == 0) {
    for (long i = (n16 << 4) + threadIdx.x; i < n; i += 256) {
      const int p = pred[i];
      const int l = (int)label[i];
      if (l != ignore && p < nc) atomicAdd(&mine[((l >= 0 && l < nc) ? l : nc) * nc + p], 1u);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < bins; i += 256) {
    const unsigned int c = sh[i] + sh[bins + i] + sh[2 * bins + i] + sh[3 * bins + i];
    if (c) atomicAdd(&hist[i], (unsigned long long)c);
  }
}

extern "C" int vfm_confusion_hist(const uint8_t* pred, const void* label, int label_dt, long n, int num_classes, int ignore_index,
                                  int64_t* hist, void* stream) {
  VFM_CHECK(hist && n >= 0, VFM_E_INVAL, "vfm_confusion_hist: null histogram / negative size");
  if (n == 0) return VFM_OK;  // an empty map (its pointers may be null) adds nothing
  VFM_CHECK(pred && label, VFM_E_INVAL, "vfm_confusion_hist: null pointer");
  VFM_CHECK(num_classes > 0 && num_classes <= NC_MAX, VFM_E_SHAPE, "vfm_confusion_hist: num_classes %d not in [1, %d]", num_classes, NC_MAX);
  VFM_CHECK(label_dt == VFM_I64 || label_dt == VFM_U8, VFM_E_UNSUPPORTED, "vfm_confusion_hist: labels must be int64 or uint8");
  VFM_CHECK(((uintptr_t)pred & 15) == 0 && ((uintptr_t)label & 15) == 0, VFM_E_ALIGN, "vfm_confusion_hist: 16-byte aligned maps required");
  const int bins = (num_classes + 1) * num_classes;
  const size_t lds = 4u * bins * sizeof(unsigned int);
  long blocks = (n / 16 + 255) / 256;
  if (blocks < 1) blocks = 1;
  if (blocks > 2048) blocks = 2048;  // 8 blocks per CU: enough loads in flight for the HBM stream, few flush atomics
  if (label_dt == VFM_U8)
    hipLaunchKernelGGL(k_confusion_hist<uint8_t>, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, pred,
                       (const uint8_t*)label, n, num_classes, ignore_index, (unsigned long long*)hist);
  else
    hipLaunchKernelGGL(k_confusion_hist<int64_t>, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, pred,
                       (const int64_t*)label, n, num_classes, ignore_index, (unsigned long long*)hist);
  VFM_LAUNCH_CHECK();
  return VFM_OK;
}

// ---------------------------------------------------------------------------------------------------- fused post-processing
// mmseg postprocess_result + the confusion counts above in ONE pass over the output pixels of one image: un-pad (the window is
// addressed in place), un-flip, bilinear resize to ori_shape (align_corners=False), argmax over the classes, uint8 label map and
// (optionally) the (label, prediction) counts.  No full-resolution fp32 map exists: the unique traffic is the source window (read
// once from HBM, its 4-tap reuse served by the caches) plus 1 B prediction and one label per output pixel.
// Four consecutive output pixels (linear index, so a group may straddle two rows) per thread: one 4-byte prediction store and one
// 4-byte (uint8) or two 16-byte (int64) label loads per group; the last n % 4 pixels are a scalar tail of the same code.
struct PLerp {
  int i0, i1;
  float l0, l1;
};
// the source index arithmetic of vfm_resize_bilinear (vision.hip lerp_idx: ATen area_pixel_compute_source_index, align_corners=False),
// restated so that both kernels sample identically; in_size is the WINDOW's size: a tap is clamped to the window, never to the map
__device__ __forceinline__ PLerp plerp_idx(int dst, float scale, int in_size) {
  float src = scale * (dst + 0.5f) - 0.5f;
  if (src < 0.f) src = 0.f;
  PLerp r;
  r.i0 = (int)src;
  if (r.i0 > in_size - 1) r.i0 = in_size - 1;
  r.i1 = r.i0 + (r.i0 < in_size - 1 ? 1 : 0);
  r.l1 = src - r.i0;
  r.l0 = 1.f - r.l1;
  return r;
}

template <typename LT, bool IDENT>
__global__ __launch_bounds__(256) void k_postprocess_argmax(const float* __restrict__ lg, int C, long ps, int rs, int h, int w, int flip,
                                                            uint8_t* __restrict__ pred, int oh, int ow, float sy, float sx,
                                                            const LT* __restrict__ label, int nc, int ignore, int ncopy,
                                                            unsigned long long* __restrict__ hist) {
  extern __shared__ unsigned int sh[];  // ncopy (4, or 2 for the largest class counts) privatised copies of the counters
  const int bins = (nc + 1) * nc;
  unsigned int* mine = sh + ((threadIdx.x >> 6) & (ncopy - 1)) * bins;
  if (hist) {
    for (int i = threadIdx.x; i < ncopy * bins; i += 256) sh[i] = 0u;
    __syncthreads();
  }
  const long n = (long)oh * ow;
  const long ng = (n + 3) >> 2;
  for (long g = blockIdx.x * 256L + threadIdx.x; g < ng; g += (long)gridDim.x * 256L) {
    const long p0 = g << 2;
    const int cnt = n - p0 < 4 ? (int)(n - p0) : 4;
    // window-relative offsets of the four taps and their weights; a pixel past the end repeats the last one (valid reads, no store)
    int o00[4], o01[4], o10[4], o11[4];
    float wy0[4], wy1[4], wx0[4], wx1[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long p = p0 + j < n ? p0 + j : n - 1;
      const int y = (int)(p / ow), x = (int)(p - (long)y * ow);
      PLerp ly, lx;
      if constexpr (IDENT) {
        ly.i0 = ly.i1 = y, lx.i0 = lx.i1 = x;
        ly.l0 = lx.l0 = 1.f, ly.l1 = lx.l1 = 0.f;
      } else {
        ly = plerp_idx(y, sy, h), lx = plerp_idx(x, sx, w);
      }
      if (flip == 1) lx.i0 = w - 1 - lx.i0, lx.i1 = w - 1 - lx.i1;
      if (flip == 2) ly.i0 = h - 1 - ly.i0, ly.i1 = h - 1 - ly.i1;
      o00[j] = ly.i0 * rs + lx.i0, o01[j] = ly.i0 * rs + lx.i1, o10[j] = ly.i1 * rs + lx.i0, o11[j] = ly.i1 * rs + lx.i1;
      wy0[j] = ly.l0, wy1[j] = ly.l1, wx0[j] = lx.l0, wx1[j] = lx.l1;
    }
    float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    int bi[4] = {0, 0, 0, 0};
    for (int c = 0; c < C; ++c) {
      const float* pl = lg + c * ps;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float v;
        if constexpr (IDENT) {
          v = pl[o00[j]];  // same size: the value itself (no 0 * inf from a neighbour)
        } else {
          const float v00 = pl[o00[j]], v01 = pl[o01[j]], v10 = pl[o10[j]], v11 = pl[o11[j]];
          v = wy0[j] * (wx0[j] * v00 + wx1[j] * v01) + wy1[j] * (wx0[j] * v10 + wx1[j] * v11);
        }
        if (v > best[j]) {  // first maximum wins (vfm_slide_finalize)
          best[j] = v;
          bi[j] = c;
        }
      }
    }
    if (cnt == 4) {
      *reinterpret_cast<uint32_t*>(pred + p0) = (uint32_t)bi[0] | ((uint32_t)bi[1] << 8) | ((uint32_t)bi[2] << 16) | ((uint32_t)bi[3] << 24);
    } else {
      for (int j = 0; j < cnt; ++j) pred[p0 + j] = (uint8_t)bi[j];
    }
    if (hist) {
      int lab[4] = {ignore, ignore, ignore, ignore};
      if (cnt == 4) {
        if constexpr (sizeof(LT) == 1) {
          const uint32_t lw = *reinterpret_cast<const uint32_t*>(label + p0);
#pragma unroll
          for (int j = 0; j < 4; ++j) lab[j] = (lw >> (8 * j)) & 0xff;
        } else {
          const longlong2* lp = reinterpret_cast<const longlong2*>(label + p0);
          const longlong2 a = lp[0], b = lp[1];
          lab[0] = (int)a.x, lab[1] = (int)a.y, lab[2] = (int)b.x, lab[3] = (int)b.y;
        }
      } else {
        for (int j = 0; j < cnt; ++j) lab[j] = (int)label[p0 + j];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int l = lab[j];
        if (j < cnt && l != ignore && bi[j] < nc) atomicAdd(&mine[((l >= 0 && l < nc) ? l : nc) * nc + bi[j]], 1u);
      }
    }
  }
  if (hist) {
    __syncthreads();
    for (int i = threadIdx.x; i < bins; i += 256) {
      unsigned int c = 0;
      for (int k = 0; k < ncopy; ++k) c += sh[k * bins + i];
      if (c) atomicAdd(&hist[i], (unsigned long long)c);
    }
  }
}

extern "C" int vfm_postprocess_argmax(const float* logits, int C, long plane_stride, long row_stride, int Hm, int Wm, int y0, int x0,
                                      int h, int w, int flip, uint8_t* pred, int oh, int ow, const void* label, int label_dt,
                                      int num_classes, int ignore_index, int64_t* hist, void* stream) {
  VFM_CHECK(logits && pred, VFM_E_INVAL, "vfm_postprocess_argmax: null pointer");
  VFM_CHECK(C > 0 && C <= 32, VFM_E_SHAPE, "vfm_postprocess_argmax: C=%d not in [1, 32]", C);
  VFM_CHECK(h > 0 && w > 0, VFM_E_SHAPE, "vfm_postprocess_argmax: empty window %d x %d", h, w);
  VFM_CHECK(Hm > 0 && Wm > 0 && y0 >= 0 && x0 >= 0 && (long)y0 + h <= Hm && (long)x0 + w <= Wm, VFM_E_SHAPE,
            "vfm_postprocess_argmax: window (%d, %d, %d, %d) outside the %d x %d map", y0, x0, h, w, Hm, Wm);
  VFM_CHECK(row_stride >= Wm && (long)Hm * row_stride < (1L << 31) && plane_stride >= (long)(Hm - 1) * row_stride + Wm, VFM_E_SHAPE,
            "vfm_postprocess_argmax: strides (plane %ld, row %ld) do not hold a %d x %d map", plane_stride, row_stride, Hm, Wm);
  VFM_CHECK(flip >= 0 && flip <= 2, VFM_E_INVAL, "vfm_postprocess_argmax: flip %d (0 none, 1 horizontal, 2 vertical)", flip);
  VFM_CHECK(oh >= 0 && ow >= 0, VFM_E_SHAPE, "vfm_postprocess_argmax: negative output size");
  VFM_CHECK(((uintptr_t)pred & 15) == 0, VFM_E_ALIGN, "vfm_postprocess_argmax: 16-byte aligned pred required");
  int ncopy = 4, bins = 0;
  if (hist) {
    VFM_CHECK(label, VFM_E_INVAL, "vfm_postprocess_argmax: hist given without label");
    VFM_CHECK(num_classes > 0 && num_classes <= NC_MAX, VFM_E_SHAPE, "vfm_postprocess_argmax: num_classes %d not in [1, %d]", num_classes, NC_MAX);
    VFM_CHECK(label_dt == VFM_I64 || label_dt == VFM_U8, VFM_E_UNSUPPORTED, "vfm_postprocess_argmax: labels must be int64 or uint8");
    VFM_CHECK(((uintptr_t)label & 15) == 0, VFM_E_ALIGN, "vfm_postprocess_argmax: 16-byte aligned label required");
    bins = (num_classes + 1) * num_classes;
    if (4u * bins * sizeof(unsigned int) > 48u * 1024u) ncopy = 2;  // 64 classes: two copies of 16.25 KiB
  } else {
    num_classes = 1;
  }
  const long n = (long)oh * ow;
  if (n == 0) return VFM_OK;
  const size_t lds = hist ? (size_t)ncopy * bins * sizeof(unsigned int) : 0;
  long blocks = ((n + 3) / 4 + 255) / 256;
  if (blocks > 2048) blocks = 2048;  // 8 blocks per CU, grid-stride beyond
  const float sy = (float)h / (float)oh, sx = (float)w / (float)ow;
  const float* win = logits + (long)y0 * row_stride + x0;
  const bool ident = h == oh && w == ow;
  const bool l8 = hist && label_dt == VFM_U8;
#define PP_LAUNCH(LT, ID)                                                                                                        \
  hipLaunchKernelGGL((k_postprocess_argmax<LT, ID>), dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, win, C, plane_stride, \
                     (int)row_stride, h, w, flip, pred, oh, ow, sy, sx, (const LT*)label, num_classes, ignore_index, ncopy,       \
                     (unsigned long long*)hist)
  if (l8) {
    if (ident) PP_LAUNCH(uint8_t, true);
    else PP_LAUNCH(uint8_t, false);
  } else {
    if (ident) PP_LAUNCH(int64_t, true);
    else PP_LAUNCH(int64_t, false);
  }
#undef PP_LAUNCH
  VFM_LAUNCH_CHECK();
  return VFM_OK;
}
