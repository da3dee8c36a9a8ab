// LoRA down-projection of an adapter site whose input no LayerNorm kernel produces (attn.proj reads the attention output, fc2 the GELU
// output): ONE launch over x [M, K] (16 bit, strided) that writes
//     mask = the dropout multiplier (0 or 1/(1-p) in 16 bit), element index offset + row * K + c of the counter-based RNG: the bits
//            vfm_dropout_mask writes for a contiguous [M, K] map with the same seed and offset,
//     xd   = x * mask, the bits vfm_mul_mask writes,
//     T    = s * xd @ A^T  [M, 64] into the K tail of the operand ([x | T] @ [W | B]^T is the adapted projection),
// instead of three passes (vfm_dropout_mask, vfm_mul_mask, vfm_gemm): x is read once, xd goes from registers into LDS and into memory.
// p = 0 (no dropout / prediction): no mask, no xd, T = s * x @ A^T.
// A is [64, K] with zero rows past the rank, so all 64 columns of T are written for every row < M.
// Block = 32 rows, 256 threads = 4 waves; K runs in chunks of 128 staged through LDS (the next chunk travels while this one is multiplied).
// Wave w owns output columns 32 (w & 1) .. + 31 and the K half (w >> 1) of every chunk; the two halves meet in LDS in a fixed order
// (fp32 accumulation, plain vector stores, no atomics).  25.5 KiB of LDS.
#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef vfm_h bf16x8 __attribute__((ext_vector_type(8)));

#define LD_ROWS 32
#define LD_R 64     // R_PAD: the rank padded to one MFMA K-block of the projection that consumes T
#define LD_KC 128
#define LD_LD 136   // 16-bit LDS row pitch (272 B): 128 + 8 so that the 32 fragment rows of one ds_read_b128 spread over the banks

struct LoraDownArgs {
  const bf16_t* x; long ld_x;
  const bf16_t* a; long ld_a;
  bf16_t* mask; long ld_mask;
  bf16_t* xd; long ld_xd;
  bf16_t* t; long ld_t;
  long rows; int K; float s, p, keep_scale; uint64_t seed, offset;
};

template <bool DROP>
__global__ void __launch_bounds__(256) k_lora_down(LoraDownArgs g) {
  __shared__ __attribute__((aligned(16))) bf16_t As[LD_ROWS * LD_LD];
  __shared__ __attribute__((aligned(16))) bf16_t Bs[LD_R * LD_LD];
  float* Rs = reinterpret_cast<float*>(Bs);   // after the K loop: the partial sums of the second K half, [32, 64] fp32 (8 KiB of B's 17 KiB)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 31, fh = lane >> 5;
  const int ct = wave & 1, kh = wave >> 1;
  const long r0 = (long)blockIdx.x * LD_ROWS;
  const int K = g.K;
  // loader maps.  x: thread -> row tid / 8, two pieces of 8 columns at 64 i + 8 (tid % 8).  A: 1024 16-byte pieces of a [64, 128] chunk,
  // piece tid + 256 i: 16 threads = one 256-B row.
  const int arow = tid >> 3, ac = tid & 7;
  const bool live = r0 + arow < g.rows;
  const long grow = live ? r0 + arow : g.rows - 1;   // rows past the end read the last row (never stored)
  uint4 ah[2], bv[4];
  auto load = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) ah[i] = *reinterpret_cast<const uint4*>(g.x + grow * g.ld_x + k0 + 64 * i + 8 * ac);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int pc = tid + 256 * i;
      bv[i] = *reinterpret_cast<const uint4*>(g.a + (long)(pc >> 4) * g.ld_a + k0 + 8 * (pc & 15));
    }
  };
  const bf16_t ks = f32_to_bf16(g.keep_scale);
  const float ksf = bf16_to_f32(ks);
  auto store = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      uint4 v = ah[i];
      if constexpr (DROP) {
        const int c0 = k0 + 64 * i + 8 * ac;
        const uint64_t e0 = g.offset + (uint64_t)grow * (uint64_t)K + (uint64_t)c0;
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        uint32_t mo[4], xo[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool k0_ = (hash_u32(g.seed, e0 + 2 * j) >> 8) * (1.0f / 16777216.0f) >= g.p;
          const bool k1_ = (hash_u32(g.seed, e0 + 2 * j + 1) >> 8) * (1.0f / 16777216.0f) >= g.p;
          mo[j] = (k0_ ? (uint32_t)ks : 0u) | ((k1_ ? (uint32_t)ks : 0u) << 16);
          xo[j] = (uint32_t)f32_to_bf16(h16_lo(w[j]) * (k0_ ? ksf : 0.f)) | ((uint32_t)f32_to_bf16(h16_hi(w[j]) * (k1_ ? ksf : 0.f)) << 16);
        }
        v = make_uint4(xo[0], xo[1], xo[2], xo[3]);
        if (live) {
          *reinterpret_cast<uint4*>(g.mask + grow * g.ld_mask + c0) = make_uint4(mo[0], mo[1], mo[2], mo[3]);
          *reinterpret_cast<uint4*>(g.xd + grow * g.ld_xd + c0) = v;
        }
      }
      *reinterpret_cast<uint4*>(As + arow * LD_LD + 64 * i + 8 * ac) = v;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int pc = tid + 256 * i;
      *reinterpret_cast<uint4*>(Bs + (pc >> 4) * LD_LD + 8 * (pc & 15)) = bv[i];
    }
  };

  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  load(0);
  for (int k0 = 0; k0 < K; k0 += LD_KC) {
    store(k0);
    __syncthreads();
    if (k0 + LD_KC < K) load(k0 + LD_KC);
#pragma unroll
    for (int s = 0; s < LD_KC / 32; ++s) {
      const int kk = 64 * kh + 16 * s + 8 * fh;
      const bf16x8 a = *reinterpret_cast<const bf16x8*>(As + fr * LD_LD + kk);
      const bf16x8 b = *reinterpret_cast<const bf16x8*>(Bs + (32 * ct + fr) * LD_LD + kk);
      acc = VFM_MFMA16(a, b, acc);
    }
    __syncthreads();
  }
  // the second K half hands its sums over; the first adds them (one fixed order) and stores
  if (kh == 1) {
#pragma unroll
    for (int r = 0; r < 16; ++r) Rs[((r & 3) + 8 * (r >> 2) + 4 * fh) * LD_R + 32 * ct + fr] = acc[r];
  }
  __syncthreads();
  if (kh == 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * fh;
      const int col = 32 * ct + fr;
      const long gr = r0 + row;
      if (gr < g.rows) g.t[gr * g.ld_t + col] = f32_to_bf16(g.s * (acc[r] + Rs[row * LD_R + col]));
    }
  }
}

extern "C" int vfm_lora_down(const void* x, long ld_x, const void* a, long ld_a, void* mask, long ld_mask, void* xd, long ld_xd, void* t,
                             long ld_t, long rows, long K, float s, float p, uint64_t seed, uint64_t offset, void* stream) {
  VFM_CHECK(x && a && t, VFM_E_INVAL, "vfm_lora_down: null operand");
  VFM_CHECK(p >= 0.f && p < 1.f, VFM_E_INVAL, "vfm_lora_down: p");
  VFM_CHECK(rows >= 0 && K > 0 && K % LD_KC == 0 && K <= (1 << 24), VFM_E_SHAPE, "vfm_lora_down: K %% 128 == 0 (K=%ld)", K);
  VFM_CHECK(ld_x >= K && ld_a >= K && ld_t >= LD_R, VFM_E_SHAPE, "vfm_lora_down: leading dimensions >= the row widths");
  VFM_CHECK((uintptr_t)x % 16 == 0 && ld_x % 8 == 0 && (uintptr_t)a % 16 == 0 && ld_a % 8 == 0, VFM_E_ALIGN,
            "vfm_lora_down: x and a 16-byte aligned with ld %% 8 == 0");
  const bool drop = p > 0.f;
  if (drop) {
    VFM_CHECK(mask && xd, VFM_E_INVAL, "vfm_lora_down: p > 0 needs mask and xd");
    VFM_CHECK(ld_mask >= K && ld_xd >= K && (uintptr_t)mask % 16 == 0 && ld_mask % 8 == 0 && (uintptr_t)xd % 16 == 0 && ld_xd % 8 == 0, VFM_E_ALIGN,
              "vfm_lora_down: mask and xd 16-byte aligned with ld %% 8 == 0, >= K");
  }
  if (rows == 0) return VFM_OK;
  LoraDownArgs g = {};
  g.x = (const bf16_t*)x, g.ld_x = ld_x, g.a = (const bf16_t*)a, g.ld_a = ld_a, g.mask = (bf16_t*)mask, g.ld_mask = ld_mask;
  g.xd = (bf16_t*)xd, g.ld_xd = ld_xd, g.t = (bf16_t*)t, g.ld_t = ld_t, g.rows = rows, g.K = (int)K, g.s = s, g.p = p;
  g.keep_scale = 1.0f / (1.0f - p), g.seed = seed, g.offset = offset;
  if (drop) hipLaunchKernelGGL(k_lora_down<true>, dim3(cdiv(rows, LD_ROWS)), dim3(256), 0, (hipStream_t)stream, g);
  else hipLaunchKernelGGL(k_lora_down<false>, dim3(cdiv(rows, LD_ROWS)), dim3(256), 0, (hipStream_t)stream, g);
  VFM_LAUNCH_CHECK();
  return VFM_OK;
}
