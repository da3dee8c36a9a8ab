// The loss options of the fused cross-entropy as per-pixel weight maps: the OHEM pixel sampler (mmseg 1.2.2
// OHEMPixelSampler, thresh branch), class weights and avg_non_ignore.  Every option ends as one fp32 map [B,H,W] that vfm_upsample_ce_w
// consumes plus one device scalar that rescales its loss and gradient; k, n, t and the normaliser never leave the device.
//   1. k_ohem_prob        p = softmax(bilinear_up(logits))[label] per pixel in registers (the arithmetic of k_upsample_ce), the counters
//                         n and #(p < thresh), and the first radix histogram of the keys
//   2. k_ohem_pick<r> / k_ohem_hist<r>   the exact k-th smallest p from three integer histograms (ohem_select.h)
//   3. k_label_weight     w = [valid and p < t] * class_weight[label] * pixel weight, and the per-class label counts that give the
//                         normaliser (k_label_weight_finish, fixed order, double)
// Only integers are accumulated with atomics: every output is bitwise reproducible.
#include "common.h"
#include "ohem_select.h"

#define OHEM_CMAX 32  // = CE_CMAX of vision.hip
static_assert(OHEM_S_INTS == VFM_OHEM_STATE_INTS && OHEM_S_N == VFM_OHEM_N && OHEM_S_NLT == VFM_OHEM_NLT && OHEM_S_K == VFM_OHEM_K &&
                  OHEM_S_T == VFM_OHEM_T && OHEM_CMAX + 1 == VFM_LABEL_COUNT_INTS,
              "include/vfmseg_hip.h and ohem_select.h describe one state layout");

// the source index arithmetic of vision.hip lerp_idx (ATen area_pixel_compute_source_index, align_corners=False)
struct OLerp {
  int i0, i1;
  float l0, l1;
};
__device__ __forceinline__ OLerp olerp_idx(int dst, float scale, int in_size) {
  float src = scale * (dst + 0.5f) - 0.5f;
  if (src < 0.f) src = 0.f;
  OLerp r;
  r.i0 = (int)src;
  if (r.i0 > in_size - 1) r.i0 = in_size - 1;
  r.i1 = r.i0 + (r.i0 < in_size - 1 ? 1 : 0);
  r.l1 = src - r.i0;
  r.l0 = 1.f - r.l1;
  return r;
}

static inline int ohem_grid(long items, int cap) {
  const long blocks = (items + 255) / 256;
  return (int)(blocks < 1 ? 1 : (blocks > cap ? cap : blocks));
}

// One wave adds its lanes' bins to an LDS histogram.  Late in training nearly every p is close to 1 and all 64 lanes hold the same bin:
// 64 LDS atomics on one address would serialise.  So the wave first peels up to four bins off as "the first pending lane's bin, added once
// with the number of lanes that share it"; whatever is still pending after that (a spread input) goes out as one add per lane, which then
// hit different addresses.  Called by all lanes of the wave (the ballots), `has` false where a lane has nothing to add.
__device__ __forceinline__ void wave_hist_add(int* sh, bool has, int bin) {
  const int lane = threadIdx.x & 63;
  unsigned long long pending = __ballot(has);
  for (int it = 0; it < 4 && pending; ++it) {
    const int leader = __ffsll((long long)pending) - 1;
    const int lb = __shfl(bin, leader, 64);
    const unsigned long long same = __ballot(has && bin == lb);
    if (lane == leader) atomicAdd(&sh[lb], (int)__popcll(same));
    if (bin == lb) has = false;
    pending &= ~same;
  }
  if (has) atomicAdd(&sh[bin], 1);
}

// LDS histogram -> global histogram: one integer atomic per non-empty bin per block
__device__ __forceinline__ void flush_hist(const int* sh, int nbins, int32_t* hist) {
  for (int i = threadIdx.x; i < nbins; i += 256) {
    const int v = sh[i];
    if (v) atomicAdd(&hist[i], v);
  }
}

__global__ void __launch_bounds__(256) k_ohem_prob(const float* __restrict__ lg, const int64_t* __restrict__ label, int B, int h, int w,
                                                    int C, int H, int W, int ignore, float sy, float sx, float thresh,
                                                    float* __restrict__ p_out, int32_t* __restrict__ state) {
  __shared__ int sh[OHEM_BINS0];
  __shared__ int red[2][4];
  for (int i = threadIdx.x; i < OHEM_BINS0; i += 256) sh[i] = 0;
  __syncthreads();
  const long total = (long)B * H * W;
  int nv = 0, nlt = 0;
  for (long base = (long)blockIdx.x * 256; base < total; base += (long)gridDim.x * 256) {  // wave-uniform trip count
    const long i = base + threadIdx.x;
    bool has = false;
    int bin = 0;
    if (i < total) {
      const int64_t lab = label[i];
      float p = OHEM_SENTINEL;
      if (lab != ignore) {
        const int hx = (int)(i % W);
        const long t = i / W;
        const int hy = (int)(t % H);
        const long b = t / H;
        const OLerp ly = olerp_idx(hy, sy, h), lx = olerp_idx(hx, sx, w);
        const float* r0 = lg + (b * h + ly.i0) * (long)w * C;
        const float* r1 = lg + (b * h + ly.i1) * (long)w * C;
        const float *p00 = r0 + (long)lx.i0 * C, *p01 = r0 + (long)lx.i1 * C, *p10 = r1 + (long)lx.i0 * C, *p11 = r1 + (long)lx.i1 * C;
        float v[OHEM_CMAX];
        float m = -INFINITY, vl = 0.f;
#pragma unroll
        for (int c = 0; c < OHEM_CMAX; ++c) {
          if (c < C) {
            v[c] = ly.l0 * (lx.l0 * p00[c] + lx.l1 * p01[c]) + ly.l1 * (lx.l0 * p10[c] + lx.l1 * p11[c]);
            if (v[c] > m) m = v[c];
            if (c == (int)lab) vl = v[c];
          }
        }
        float se = 0.f;
#pragma unroll
        for (int c = 0; c < OHEM_CMAX; ++c)
          if (c < C) se += __expf(v[c] - m);
        p = __expf(vl - m) / se;
        const uint32_t bits = __float_as_uint(p);
        if (ohem_is_key(bits)) {
          has = true;
          bin = ohem_digit(bits, 0);
          nv += 1;
          nlt += p < thresh ? 1 : 0;
        } else {
          p = OHEM_SENTINEL;  // (a NaN with the sign bit set: out of the selection, as an ignored pixel)
        }
      }
      p_out[i] = p;
    }
    wave_hist_add(sh, has, bin);
  }
  for (int o = 32; o > 0; o >>= 1) {
    nv += __shfl_xor(nv, o, 64);
    nlt += __shfl_xor(nlt, o, 64);
  }
  if ((threadIdx.x & 63) == 0) red[0][threadIdx.x >> 6] = nv, red[1][threadIdx.x >> 6] = nlt;
  __syncthreads();
  if (threadIdx.x < 2) {  // one global tally per counter per block
    const int n = (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
    if (n) atomicAdd(&state[threadIdx.x == 0 ? OHEM_S_N : OHEM_S_NLT], n);
  }
  flush_hist(sh, OHEM_BINS0, state + OHEM_S_HIST0);
}

// rounds 1 and 2: the histogram of the next digit over the keys that share the prefix picked so far
template <int ROUND>
__global__ void __launch_bounds__(256) k_ohem_hist(const float* __restrict__ p, long total, int32_t* __restrict__ state) {
  __shared__ int sh[OHEM_BINS1];
  if (state[OHEM_S_DONE]) return;  // the threshold decided in round 0 (read on the device; the launch itself is unconditional)
  const uint32_t prefix = (uint32_t)state[OHEM_S_PREFIX];
  for (int i = threadIdx.x; i < OHEM_BINS1; i += 256) sh[i] = 0;
  __syncthreads();
  for (long base = (long)blockIdx.x * 256; base < total; base += (long)gridDim.x * 256) {
    const long i = base + threadIdx.x;
    bool has = false;
    int bin = 0;
    if (i < total) {
      const uint32_t bits = __float_as_uint(p[i]);
      if (ohem_is_key(bits) && ohem_prefix_match(bits, prefix, ROUND)) has = true, bin = ohem_digit(bits, ROUND);
    }
    wave_hist_add(sh, has, bin);
  }
  __syncthreads();
  flush_hist(sh, OHEM_BINS1, state + (ROUND == 1 ? OHEM_S_HIST1 : OHEM_S_HIST0));
}

// One block: walk round ROUND's histogram to the bin that holds the wanted rank.  256 threads sum a chunk of bins each, thread 0 walks
// the chunk sums and then the chunk (ohem_pick_bin both times).  Round 0 reads n and #(p < thresh), clamps k and may settle t = thresh.
template <int ROUND>
__global__ void __launch_bounds__(256) k_ohem_pick(int32_t* __restrict__ state, long k_request, float thresh) {
  __shared__ int chunk[256];
  constexpr int NB = ROUND == 0 ? OHEM_BINS0 : OHEM_BINS1, PER = NB / 256;
  const int tid = threadIdx.x;
  int rank;
  if (ROUND == 0) {
    const int n = state[OHEM_S_N], nlt = state[OHEM_S_NLT];
    const int k = n > 0 ? ohem_clamp_rank(k_request, n) : 0;
    const bool decided = ohem_thresh_decides(n, nlt, k);
    __syncthreads();  // everyone has read the counters before thread 0 writes next to them
    if (tid == 0) {
      state[OHEM_S_K] = k;
      if (decided) {
        state[OHEM_S_T] = (int32_t)__float_as_uint(thresh);
        state[OHEM_S_DONE] = 1;
      }
    }
    if (decided) return;
    rank = k;
  } else {
    if (state[OHEM_S_DONE]) return;
    rank = state[OHEM_S_RANK];
  }
  int32_t* hist = state + (ROUND == 1 ? OHEM_S_HIST1 : OHEM_S_HIST0);
  int s = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) s += hist[tid * PER + j];
  chunk[tid] = s;
  const uint32_t prefix = ROUND == 0 ? 0u : (uint32_t)state[OHEM_S_PREFIX];
  __syncthreads();
  if (tid == 0) {
    int c, r, b, r2;
    ohem_pick_bin(chunk, 256, rank, &c, &r);
    ohem_pick_bin(hist + c * PER, PER, r, &b, &r2);
    const uint32_t np = ohem_extend_prefix(prefix, ROUND, c * PER + b);
    state[OHEM_S_PREFIX] = (int32_t)np;
    state[OHEM_S_RANK] = r2;
    if (ROUND == 2) {
      const float v = __uint_as_float(np);  // the k-th smallest valid p, exactly
      state[OHEM_S_T] = (int32_t)__float_as_uint(v > thresh ? v : thresh);
      state[OHEM_S_DONE] = 1;
    }
  }
  // the next round's histogram starts empty (round 1 counts into HIST1, round 2 into HIST0, which round 0 is done with)
  if (ROUND == 0)
    for (int i = tid; i < OHEM_BINS1; i += 256) state[OHEM_S_HIST1 + i] = 0;
  if (ROUND == 1) {
    for (int i = tid; i < OHEM_BINS1; i += 256) state[OHEM_S_HIST0 + i] = 0;
  }
}

// w = [valid and p < t] * class_weight[label] * pixel weight (each factor optional) and the per-class counts of the valid labels
// (bin OHEM_CMAX: valid labels outside [0, C); they weigh 0 under class weights).  The counts are wave-uniform ballot sums in registers.
__global__ void __launch_bounds__(256) k_label_weight(const int64_t* __restrict__ label, const float* __restrict__ p,
                                                       const int32_t* __restrict__ state, const float* __restrict__ cw,
                                                       const float* __restrict__ pixw, int C, long total, int ignore,
                                                       float* __restrict__ weight, int32_t* __restrict__ counts) {
  __shared__ float scw[OHEM_CMAX + 1];
  __shared__ int shc[OHEM_CMAX + 1];
  if (threadIdx.x <= OHEM_CMAX) {
    scw[threadIdx.x] = cw ? (threadIdx.x < C ? cw[threadIdx.x] : 0.f) : 1.f;
    shc[threadIdx.x] = 0;
  }
  __syncthreads();
  const float t = p ? __uint_as_float((uint32_t)state[OHEM_S_T]) : 0.f;
  int acc[OHEM_CMAX + 1];
#pragma unroll
  for (int c = 0; c <= OHEM_CMAX; ++c) acc[c] = 0;
  for (long base = (long)blockIdx.x * 256; base < total; base += (long)gridDim.x * 256) {
    const long i = base + threadIdx.x;
    int cls = -1;  // -1: no pixel / ignored
    if (i < total) {
      const int64_t lab = label[i];
      if (lab != ignore) cls = (lab >= 0 && lab < C) ? (int)lab : OHEM_CMAX;
      if (weight) {
        float wv = 0.f;
        if (cls >= 0) {
          wv = scw[cls];
          if (p) wv = p[i] < t ? wv : 0.f;
          if (pixw) wv *= pixw[i];
        }
        weight[i] = wv;
      }
    }
    if (counts) {
#pragma unroll
      for (int c = 0; c <= OHEM_CMAX; ++c)
        if (c < C || c == OHEM_CMAX) acc[c] += (int)__popcll(__ballot(cls == c));
    }
  }
  if (counts) {
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int c = 0; c <= OHEM_CMAX; ++c)
        if (acc[c]) atomicAdd(&shc[c], acc[c]);
    }
    __syncthreads();
    if (threadIdx.x <= OHEM_CMAX && shc[threadIdx.x]) atomicAdd(&counts[threadIdx.x], shc[threadIdx.x]);
  }
}

// norm[0] = B*H*W / (avg_factor + eps): what the loss and gradient of vfm_upsample_ce_w (a mean over ALL pixels) are multiplied with;
// norm[1] = avg_factor.  mode 2: sum_c class_weight[c] * count[c]; 1: the number of valid pixels; 0: B*H*W.  Fixed order, double.
__global__ void k_label_weight_finish(const int32_t* __restrict__ counts, const float* __restrict__ cw, int C, int mode, long total,
                                      float* __restrict__ norm) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double avg = 0.0;
  if (mode == 2) {
    for (int c = 0; c < C; ++c) avg += (double)cw[c] * (double)counts[c];
  } else if (mode == 1) {
    long n = counts[OHEM_CMAX];
    for (int c = 0; c < C; ++c) n += counts[c];
    avg = (double)n;
  } else {
    avg = (double)total;
  }
  norm[0] = (float)((double)total / (avg + 1.1920928955078125e-07));
  norm[1] = (float)avg;
}

extern "C" int vfm_ohem_prob(const float* logits_low, const int64_t* label, int B, int h, int w, int C, int H, int W, int ignore_index,
                             float thresh, float* p, int32_t* state, void* stream) {
  VFM_CHECK(C > 0 && C <= OHEM_CMAX, VFM_E_SHAPE, "vfm_ohem_prob: C=%d > %d", C, OHEM_CMAX);
  VFM_CHECK(B > 0 && h > 0 && w > 0 && H > 0 && W > 0, VFM_E_SHAPE, "vfm_ohem_prob: empty map");
  const long total = (long)B * H * W;
  VFM_CHECK(total < (1L << 31), VFM_E_SHAPE, "vfm_ohem_prob: %ld pixels overflow the int32 counters", total);
  VFM_CHECK(logits_low && label && p && state, VFM_E_INVAL, "vfm_ohem_prob: null pointer");
  hipLaunchKernelGGL(k_ohem_prob, dim3(ohem_grid(total, 1024)), dim3(256), 0, (hipStream_t)stream, logits_low, label, B, h, w, C, H, W,
                     ignore_index, (float)h / (float)H, (float)w / (float)W, thresh, p, state);
  VFM_LAUNCH_CHECK();
  return VFM_OK;
}

extern "C" int vfm_ohem_threshold(const float* p, long n_pix, long k_request, float thresh, int32_t* state, void* stream) {
  VFM_CHECK(n_pix > 0 && n_pix < (1L << 31), VFM_E_SHAPE, "vfm_ohem_threshold: n_pix=%ld", n_pix);
  VFM_CHECK(k_request >= 0, VFM_E_INVAL, "vfm_ohem_threshold: negative rank");
  VFM_CHECK(p && state, VFM_E_INVAL, "vfm_ohem_threshold: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int grid = ohem_grid(n_pix, 512);
  hipLaunchKernelGGL(k_ohem_pick<0>, dim3(1), dim3(256), 0, s, state, k_request, thresh);
  hipLaunchKernelGGL(k_ohem_hist<1>, dim3(grid), dim3(256), 0, s, p, n_pix, state);
  hipLaunchKernelGGL(k_ohem_pick<1>, dim3(1), dim3(256), 0, s, state, k_request, thresh);
  hipLaunchKernelGGL(k_ohem_hist<2>, dim3(grid), dim3(256), 0, s, p, n_pix, state);
  hipLaunchKernelGGL(k_ohem_pick<2>, dim3(1), dim3(256), 0, s, state, k_request, thresh);
  VFM_LAUNCH_CHECK();
  return VFM_OK;
}

extern "C" int vfm_label_weight(const int64_t* label, const float* p, const int32_t* state, const float* class_weight,
                                const float* pix_weight, int C, long n_pix, int ignore_index, int avg_non_ignore, float* weight,
                                int32_t* counts, float* norm, void* stream) {
  VFM_CHECK(C > 0 && C <= OHEM_CMAX, VFM_E_SHAPE, "vfm_label_weight: C=%d > %d", C, OHEM_CMAX);
  VFM_CHECK(n_pix > 0 && n_pix < (1L << 31), VFM_E_SHAPE, "vfm_label_weight: n_pix=%ld", n_pix);
  VFM_CHECK(label && (weight || counts), VFM_E_INVAL, "vfm_label_weight: nothing to do");
  VFM_CHECK((p == nullptr) == (state == nullptr), VFM_E_INVAL, "vfm_label_weight: p and state come together");
  VFM_CHECK((counts == nullptr) == (norm == nullptr), VFM_E_INVAL, "vfm_label_weight: counts and norm come together");
  VFM_CHECK(weight || !(p || class_weight || pix_weight), VFM_E_INVAL, "vfm_label_weight: a weighted form needs the weight map");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_label_weight, dim3(ohem_grid(n_pix, 1024)), dim3(256), 0, s, label, p, state, class_weight, pix_weight, C, n_pix,
                     ignore_index, weight, counts);
  if (counts)
    hipLaunchKernelGGL(k_label_weight_finish, dim3(1), dim3(64), 0, s, counts, class_weight, C, class_weight ? 2 : (avg_non_ignore ? 1 : 0),
                       n_pix, norm);
  VFM_LAUNCH_CHECK();
  return VFM_OK;
}
