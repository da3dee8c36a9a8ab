// Gradient clipping on the device: the norm of the flat fp32 gradient buffer and torch's clip_grad_norm_ coefficient,
// neither of which the host ever reads in a train step - the fused AdamW launch takes the coefficient from the clip state (k_adamw,
// vision.hip) and, under the loss scaler, its skip flag from the non-finite flag formed in the same pass.
//   1. k_grad_norm<VEC,KIND>  each thread folds its grid-strided elements (|g|^2, |g| or max |g|) into ONE fp32 accumulator, the
//                             block adds its 256 accumulators in double in a fixed LDS tree -> partial[block], bad[block]
//   2. k_grad_norm_finish     one block adds the partials in double in a fixed order, applies the pre-scale (the norm is homogeneous:
//                             |s g| = |s| |g|, so the un-scale / the 1/world average is ONE multiply of the result), writes the clip state
// No float atomics, and the grid is a function of n alone: the same buffer gives the same bits on every call.
//
// Longest fp32 chain (what the test tolerance of tests/test_optim_clip_gpu.py rests on).  The float4 path runs min(2048, ceil(n/4/256))
// blocks of 256 threads; a thread adds 4 elements per grid stride of GN_GRID * 256 * 4 = 2^21 floats into its accumulator, plus at
// most one of the n % 4 tail elements:  chain = 4 * ceil(n / 2^21) + 1  (16.6 M gradients of dinov2_ms_masked: 33).  The scalar path
// (pointer not 16-byte aligned) adds one element per stride of 2^19: chain = ceil(n / 2^19) (32 for that buffer).  Every addend is >= 0,
// so the relative error of a chain of c additions is at most c * 2^-24; everything after it (8 + 11 levels of tree) is double.
// 1e-5 relative therefore holds while chain <= 167, i.e. up to n = 87 M on the float4 path, 2^-24 per element squared included.
#include "common.h"

#define GN_GRID 2048
static_assert(2 * GN_GRID == VFM_GRAD_NORM_WS_DOUBLES, "include/vfmseg_hip.h states the workspace size");

template <int KIND>
__device__ __forceinline__ void gn_fold(float& acc, int& bad, float x) {
  bad |= (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u;   // inf or NaN: the exponent field is all ones
  const float a = fabsf(x);
  if (KIND == VFM_NORM_L2) acc += a * a;
  else if (KIND == VFM_NORM_L1) acc += a;
  else acc = fmaxf(acc, a);   // (fmaxf drops a NaN: the finish kernel turns a flagged max into NaN)
}

template <int KIND>
__device__ __forceinline__ double gn_join(double a, double b) {
  return KIND == VFM_NORM_INF ? (a > b ? a : b) : a + b;
}

template <bool VEC, int KIND>
__global__ void __launch_bounds__(256) k_grad_norm(const float* __restrict__ g, long n, double* __restrict__ ws) {
  __shared__ double s_acc[256];
  float acc = 0.f;
  int bad = 0;
  const long stride = (long)gridDim.x * 256L;
  if constexpr (VEC) {
    const long nv = n >> 2;
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
#pragma unroll 4
    for (long iv = blockIdx.x * 256L + threadIdx.x; iv < nv; iv += stride) {
      const float4 x = g4[iv];
      gn_fold<KIND>(acc, bad, x.x);
      gn_fold<KIND>(acc, bad, x.y);
      gn_fold<KIND>(acc, bad, x.z);
      gn_fold<KIND>(acc, bad, x.w);
    }
    const long tail = (nv << 2) + threadIdx.x;   // the n % 4 elements behind the last whole vector: block 0, threads 0..2
    if (blockIdx.x == 0 && threadIdx.x < 3 && tail < n) gn_fold<KIND>(acc, bad, g[tail]);
  } else {
#pragma unroll 4
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += stride) gn_fold<KIND>(acc, bad, g[i]);
  }
  s_acc[threadIdx.x] = (double)acc;
  const int any_bad = __syncthreads_or(bad);   // (also the barrier behind the store above)
  for (int w = 128; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) s_acc[threadIdx.x] = gn_join<KIND>(s_acc[threadIdx.x], s_acc[threadIdx.x + w]);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    ws[blockIdx.x] = s_acc[0];
    ws[GN_GRID + blockIdx.x] = any_bad ? 1.0 : 0.0;
  }
}

// one block of 256 threads: thread t adds partials t, t + 256, ... in that order, then the LDS tree of k_grad_norm
template <int KIND>
__global__ void __launch_bounds__(256) k_grad_norm_finish(const double* __restrict__ ws, int n_part, float max_norm, float pre_scale,
                                                          const float* __restrict__ amp_state, float* __restrict__ clip_state,
                                                          int* __restrict__ nonfinite) {
  __shared__ double s_acc[256];
  double acc = 0.0;
  int bad = 0;
  for (int i = threadIdx.x; i < n_part; i += 256) {
    acc = gn_join<KIND>(acc, ws[i]);
    bad |= ws[GN_GRID + i] != 0.0;
  }
  s_acc[threadIdx.x] = acc;
  const int any_bad = __syncthreads_or(bad);
  for (int w = 128; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) s_acc[threadIdx.x] = gn_join<KIND>(s_acc[threadIdx.x], s_acc[threadIdx.x + w]);
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  double total = KIND == VFM_NORM_L2 ? sqrt(s_acc[0]) : s_acc[0];
  if (any_bad && total - total == 0.0) total = nan("");                    // a NaN that the max dropped, an inf the sum lost
  const float s = amp_state != nullptr ? pre_scale / amp_state[0] : pre_scale;   // as k_adamw forms its un-scale factor
  const float tn = (float)(total * (double)fabsf(s));
  // torch.nn.utils.clip_grad_norm_: clip_coef = max_norm / (total_norm + 1e-6), clamped to at most 1 (a NaN stays a NaN), in fp32
  const float r = max_norm / (tn + 1e-6f);
  clip_state[0] = tn;
  clip_state[1] = n_part == 0 ? 1.f : (r != r ? r : fminf(r, 1.f));
  clip_state[2] = 0.f;
  clip_state[3] = 0.f;
  if (nonfinite != nullptr) *nonfinite = any_bad ? 1 : 0;
}

template <int KIND>
static void gn_launch(const float* g, long n, float max_norm, float pre_scale, const float* amp_state, double* ws, float* clip_state,
                      int* nonfinite, hipStream_t st) {
  int grid = 0;
  if (n > 0) {
    const bool vec = ((uintptr_t)g & 15) == 0;
    const long work = vec ? (n + 3) / 4 : n;
    grid = (int)((work + 255) / 256 > GN_GRID ? GN_GRID : (work + 255) / 256);
    if (vec) hipLaunchKernelGGL((k_grad_norm<true, KIND>), dim3(grid), dim3(256), 0, st, g, n, ws);
    else hipLaunchKernelGGL((k_grad_norm<false, KIND>), dim3(grid), dim3(256), 0, st, g, n, ws);
  }
  hipLaunchKernelGGL((k_grad_norm_finish<KIND>), dim3(1), dim3(256), 0, st, ws, grid, max_norm, pre_scale, amp_state, clip_state, nonfinite);
}

extern "C" int vfm_grad_norm(const float* g, long n, int norm_kind, float max_norm, float pre_scale, const float* amp_state,
                             double* workspace, float* clip_state, int* nonfinite, void* stream) {
  VFM_CHECK(n >= 0 && (g != nullptr || n == 0) && workspace != nullptr && clip_state != nullptr, VFM_E_INVAL, "vfm_grad_norm: arguments");
  VFM_CHECK(((uintptr_t)g & 3) == 0 && ((uintptr_t)workspace & 7) == 0, VFM_E_ALIGN, "vfm_grad_norm: g / workspace alignment");
  VFM_CHECK(norm_kind == VFM_NORM_L2 || norm_kind == VFM_NORM_L1 || norm_kind == VFM_NORM_INF, VFM_E_UNSUPPORTED,
            "vfm_grad_norm: norm_kind %d (VFM_NORM_L2, VFM_NORM_L1, VFM_NORM_INF)", norm_kind);
  VFM_CHECK(max_norm == max_norm && max_norm >= 0.f, VFM_E_INVAL, "vfm_grad_norm: max_norm");
  hipStream_t st = (hipStream_t)stream;
  if (norm_kind == VFM_NORM_L2) gn_launch<VFM_NORM_L2>(g, n, max_norm, pre_scale, amp_state, workspace, clip_state, nonfinite, st);
  else if (norm_kind == VFM_NORM_L1) gn_launch<VFM_NORM_L1>(g, n, max_norm, pre_scale, amp_state, workspace, clip_state, nonfinite, st);
  else gn_launch<VFM_NORM_INF>(g, n, max_norm, pre_scale, amp_state, workspace, clip_state, nonfinite, st);
  VFM_LAUNCH_CHECK();
  return VFM_OK;
}
