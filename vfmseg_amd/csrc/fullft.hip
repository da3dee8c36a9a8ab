// Full fine-tuning of the backbone: the two memory-bound kernels that only a trained base needs (include/vfmseg_hip.h, ABI 12).
//   vfm_branch_param_grads : LayerScale / bias gradients of a residual branch and the dgrad operand, one read pass over dx and u
//   vfm_pack_weights       : per-step refresh of the packed GEMM operands (and their transposes) from the fp32 master, one launch
// Both are the same in the two builds (bf16_t = the half type of the build).
#include "common.h"

__device__ __forceinline__ uint32_t pack_h2(float a, float b) { return (uint32_t)f32_to_bf16(a) | ((uint32_t)f32_to_bf16(b) << 16); }

template <typename T>
__device__ __forceinline__ void ld8(const T* p, float (&v)[8]);
template <>
__device__ __forceinline__ void ld8<float>(const float* p, float (&v)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
}
template <>
__device__ __forceinline__ void ld8<bf16_t>(const bf16_t* p, float (&v)[8]) {
  const uint4 w = *reinterpret_cast<const uint4*>(p);
  v[0] = h16_lo(w.x), v[1] = h16_hi(w.x), v[2] = h16_lo(w.y), v[3] = h16_hi(w.y);
  v[4] = h16_lo(w.z), v[5] = h16_hi(w.z), v[6] = h16_lo(w.w), v[7] = h16_hi(w.w);
}
template <typename T>
__device__ __forceinline__ void st8(T* p, const float (&v)[8]);
template <>
__device__ __forceinline__ void st8<float>(float* p, const float (&v)[8]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}
template <>
__device__ __forceinline__ void st8<bf16_t>(bf16_t* p, const float (&v)[8]) {
  *reinterpret_cast<uint4*>(p) = make_uint4(pack_h2(v[0], v[1]), pack_h2(v[2], v[3]), pack_h2(v[4], v[5]), pack_h2(v[6], v[7]));
}

// ------------------------------------------------------------------------------------------------ branch parameter gradients
// stage 1: a block owns 64 columns (8 lanes x 8 columns: 16-byte loads of u, 2 x 16 of dx) and 32 row lanes; block (bx, by) walks the rows
// by*32 + lane, += gridDim.y*32.  The 32 row lanes of a column meet pairwise in LDS (fixed order); ws[by, 0 | 1, c] = (sum dx u, sum dx).
template <typename TU, typename TT>
__global__ void __launch_bounds__(256) k_branch1(const float* __restrict__ dx, long ld_dx, const TU* __restrict__ u, long ld_u,
                                                 const float* __restrict__ gamma, long M, long D, TT* __restrict__ t, long ld_t,
                                                 float* __restrict__ ws) {
  __shared__ float sh[2][32][65];
  const int tx = threadIdx.x & 7, ty = threadIdx.x >> 3;
  const long c = (long)blockIdx.x * 64 + tx * 8;
  float g[8];
  ld8<float>(gamma + c, g);
  float sdu[8], sdx[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) sdu[j] = 0.f, sdx[j] = 0.f;
  for (long r = (long)blockIdx.y * 32 + ty; r < M; r += (long)gridDim.y * 32) {
    float d[8];
    ld8<float>(dx + r * ld_dx + c, d);
    if (u) {
      float uv[8];
      ld8<TU>(u + r * ld_u + c, uv);
#pragma unroll
      for (int j = 0; j < 8; ++j) sdu[j] += d[j] * uv[j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) sdx[j] += d[j];
    if (t) {
      float tv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) tv[j] = d[j] * g[j];
      st8<TT>(t + r * ld_t + c, tv);
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) sh[0][ty][tx * 8 + j] = sdu[j], sh[1][ty][tx * 8 + j] = sdx[j];
  __syncthreads();
  if (threadIdx.x < 128) {
    const int which = threadIdx.x >> 6, col = threadIdx.x & 63;
    float v[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) v[i] = sh[which][i][col];
#pragma unroll
    for (int s = 16; s > 0; s >>= 1)
#pragma unroll
      for (int i = 0; i < s; ++i) v[i] += v[i + s];
    ws[((long)blockIdx.y * 2 + which) * D + (long)blockIdx.x * 64 + col] = v[0];
  }
}

// stage 2: one thread per column adds the parts in order, in double
__global__ void __launch_bounds__(256) k_branch2(const float* __restrict__ ws, int parts, long D, const float* __restrict__ gamma,
                                                 float* __restrict__ dgamma, float* __restrict__ dbias, int accumulate) {
  const long c = (long)blockIdx.x * 256 + threadIdx.x;
  if (c >= D) return;
  double a = 0.0, b = 0.0;
  for (int p = 0; p < parts; ++p) {
    a += (double)ws[((long)p * 2) * D + c];
    b += (double)ws[((long)p * 2 + 1) * D + c];
  }
  if (dgamma) dgamma[c] = accumulate ? dgamma[c] + (float)a : (float)a;
  if (dbias) {
    const float v = (float)((double)gamma[c] * b);
    dbias[c] = accumulate ? dbias[c] + v : v;
  }
}

extern "C" int vfm_branch_param_grads(const float* dx, long ld_dx, const void* u, int u_dt, long ld_u, const float* gamma, long M, long D,
                                      float* dgamma, float* dbias, int accumulate, void* t, int t_dt, long ld_t, float* ws, void* stream) {
  auto a16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  VFM_CHECK(dx && gamma && ws && M >= 0 && D > 0 && D % 64 == 0, VFM_E_SHAPE, "vfm_branch_param_grads: D must be a multiple of 64");
  VFM_CHECK(!dgamma || u, VFM_E_INVAL, "vfm_branch_param_grads: dgamma needs the saved branch output u");
  VFM_CHECK(ld_dx >= D && ld_dx % 8 == 0 && a16(dx) && a16(gamma) && (!u || (ld_u >= D && ld_u % 8 == 0 && a16(u))) &&
                (!t || (ld_t >= D && ld_t % 8 == 0 && a16(t))),
            VFM_E_SHAPE, "vfm_branch_param_grads: leading dimensions must be multiples of 8 elements and bases 16-byte aligned");
  const int udt = u ? u_dt : (t ? t_dt : VFM_F32), tdt = t ? t_dt : udt;
  VFM_CHECK((udt == VFM_F32 || udt == VFM_BF16) && udt == tdt, VFM_E_INVAL, "vfm_branch_param_grads: u and t share one dtype (fp32 or the half type)");
  hipStream_t s = (hipStream_t)stream;
  long parts = (M + 127) / 128;   // >= 4 rows per thread before another block is worth its reduction
  const long cap = 2048 / (D / 64) > 0 ? 2048 / (D / 64) : 1;
  if (parts > cap) parts = cap;
  if (parts > VFM_BRANCH_WS_PARTS) parts = VFM_BRANCH_WS_PARTS;
  if (parts < 1) parts = 1;
  dim3 grid((unsigned)(D / 64), (unsigned)parts);
  if (udt == VFM_F32)
    hipLaunchKernelGGL((k_branch1<float, float>), grid, dim3(256), 0, s, dx, ld_dx, (const float*)u, ld_u, gamma, M, D, (float*)t, ld_t, ws);
  else
    hipLaunchKernelGGL((k_branch1<bf16_t, bf16_t>), grid, dim3(256), 0, s, dx, ld_dx, (const bf16_t*)u, ld_u, gamma, M, D, (bf16_t*)t, ld_t, ws);
  if (dgamma || dbias)
    hipLaunchKernelGGL(k_branch2, dim3(cdiv(D, 256)), dim3(256), 0, s, ws, (int)parts, D, gamma, dgamma, dbias, accumulate);
  VFM_LAUNCH_CHECK();
  return VFM_OK;
}

// ------------------------------------------------------------------------------------------------ packed-weight refresh
// blockIdx.y = site; the blocks of a site walk its 64 x 64 tiles.  A tile is read once (16-byte loads along K), written to w along K and,
// through LDS, to wt along N (8- / 16-byte stores where the leading dimensions allow, elementwise otherwise).
template <typename TO>
__device__ __forceinline__ void st4(TO* p, const float (&v)[4]);
template <>
__device__ __forceinline__ void st4<float>(float* p, const float (&v)[4]) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
template <>
__device__ __forceinline__ void st4<bf16_t>(bf16_t* p, const float (&v)[4]) {
  *reinterpret_cast<uint2*>(p) = make_uint2(pack_h2(v[0], v[1]), pack_h2(v[2], v[3]));
}

template <typename TO>
__global__ void __launch_bounds__(256) k_pack_weights(const vfm_pack_site* __restrict__ tab) {
  __shared__ float tile[64][65];
  const vfm_pack_site s = tab[blockIdx.y];
  const long tk = (s.K + 63) / 64, tn = (s.N + 63) / 64, ntiles = tk * tn;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  constexpr uintptr_t AM = 4 * sizeof(TO) - 1;
  TO* w = (TO*)s.w;
  TO* wt = (TO*)s.wt;
  const bool vec_in = (s.K % 4 == 0) && ((reinterpret_cast<uintptr_t>(s.src) & 15) == 0);
  const bool vec_w = (s.ld_w % 4 == 0) && ((reinterpret_cast<uintptr_t>(w) & AM) == 0);
  const bool vec_t = wt && (s.ld_wt % 4 == 0) && ((reinterpret_cast<uintptr_t>(wt) & AM) == 0);
  for (long ti = blockIdx.x; ti < ntiles; ti += gridDim.x) {
    const long r0 = (ti / tk) * 64, c0 = (ti % tk) * 64;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = ty + 16 * j;
      const long r = r0 + i, c = c0 + tx * 4;
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (r < s.N) {
        const float* sp = s.src + r * s.K + c;
        if (vec_in && c + 3 < s.K) {
          const float4 f = *reinterpret_cast<const float4*>(sp);
          v[0] = f.x, v[1] = f.y, v[2] = f.z, v[3] = f.w;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (c + e < s.K) v[e] = sp[e];
        }
        TO* dp = w + r * s.ld_w + c;
        if (vec_w && c + 3 < s.K) {
          st4<TO>(dp, v);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (c + e < s.K) st_f32(dp + e, v[e]);
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) tile[i][tx * 4 + e] = v[e];
    }
    __syncthreads();
    if (wt) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int i = ty + 16 * j;
        const long k = c0 + i, n = r0 + tx * 4;
        if (k < s.K) {
          float v[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = tile[tx * 4 + e][i];
          TO* dp = wt + k * s.ld_wt + n;
          if (vec_t && n + 3 < s.N) {
            st4<TO>(dp, v);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (n + e < s.N) st_f32(dp + e, v[e]);
          }
        }
      }
    }
    __syncthreads();
  }
}

extern "C" int vfm_pack_weights(const vfm_pack_site* table_dev, int nsites, long max_tiles, int dt, void* stream) {
  VFM_CHECK(table_dev && nsites >= 0 && (dt == VFM_F32 || dt == VFM_BF16), VFM_E_INVAL, "vfm_pack_weights: bad args");
  if (nsites == 0 || max_tiles <= 0) return VFM_OK;
  VFM_CHECK(nsites <= 65535, VFM_E_SHAPE, "vfm_pack_weights: at most 65535 sites per table");
  int gx = (int)(max_tiles > 256 ? 256 : max_tiles);
  if (dt == VFM_F32) hipLaunchKernelGGL(k_pack_weights<float>, dim3(gx, nsites), dim3(256), 0, (hipStream_t)stream, table_dev);
  else hipLaunchKernelGGL(k_pack_weights<bf16_t>, dim3(gx, nsites), dim3(256), 0, (hipStream_t)stream, table_dev);
  VFM_LAUNCH_CHECK();
  return VFM_OK;
}
