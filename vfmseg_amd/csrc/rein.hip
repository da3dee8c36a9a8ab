// Rein adapter (rein/models/backbones/reins.py:84-116): the token attention between the fp32 residual stream and the m <= 128 learnable tokens
// of a layer, forward and backward, each as ONE launch.  Both directions have the same shape:
//     phase 1   R[32 rows, 128] = A[32 rows, D] @ B1[128, D]^T          (K = D, B1 staged through LDS in chunks of 128 columns)
//     row op    softmax (forward) / softmax backward (backward) on the 128-wide rows, in registers; result in 16 bit in LDS (+ global)
//     phase 2   O[32 rows, D]   = R16[32 rows, 128] @ B2[D, 128]^T + epilogue   (K = 128, B2 staged in chunks of 128 output columns)
//   forward : A = x (fp32 stream, converted on the way into LDS), B1 = T, row op = masked softmax of c * scores, B2 = V^T,
//             O = u = P V + x in the compute type (the A operand of the mlp_delta_f GEMM); P (and x in 16 bit) are kept for backward.
//   backward: A = du (16 bit), B1 = V, row op = dS = c * P * (dP - <P, dP>), B2 = T^T, O = dx += du + dS T (fp32 gradient stream).
// T / V are [128, D] with zero rows past the m tokens, V with a zero row 0 as well ("attend to nothing", reins.py:110-114: column 0 of P meets
// no value); the pad columns are masked out of the softmax (probability exactly 0), not merely zero scores.
// 256 threads = 4 waves; in phase 1 wave w owns score columns 32 w .. 32 w + 31, in phase 2 output columns d0 + 32 w ...  51 KiB of LDS (8704 + 34816 + 8704 B).
#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef vfm_h bf16x8 __attribute__((ext_vector_type(8)));

#define RN_ROWS 32
#define RN_TOK 128
#define RN_KC 128
#define RN_LD 136   // 16-bit LDS row pitch (272 B): 128 + 8 so that the 32 fragment rows of one ds_read_b128 spread over the banks

struct ReinArgs {
  const float* x; long ld_x;          // forward A operand (fp32) / backward: unused
  const bf16_t* a16; long ld_a;       // backward A operand du
  const bf16_t* b1; const bf16_t* b2; // [128, D] and [D, 128]
  bf16_t* p; long ld_p;               // forward: P out (may be null); backward: P in
  bf16_t* r16; long ld_r;             // backward: dS out [rows, 128]
  bf16_t* u; long ld_u;               // forward: u out
  bf16_t* x16; long ld_x16;           // forward: 16-bit copy of x (may be null)
  float* dx; long ld_dx;              // backward: gradient stream (+=)
  long rows; int D; int m; float c;
};

__device__ __forceinline__ uint32_t pack2(float a, float b) { return (uint32_t)f32_to_bf16(a) | ((uint32_t)f32_to_bf16(b) << 16); }

template <bool BWD>
__global__ void __launch_bounds__(256) k_rein_mix(ReinArgs g) {
  __shared__ __attribute__((aligned(16))) bf16_t As[RN_ROWS * RN_LD];
  __shared__ __attribute__((aligned(16))) bf16_t Bs[RN_TOK * RN_LD];
  __shared__ __attribute__((aligned(16))) bf16_t Ps[RN_ROWS * RN_LD];
  float* Ss = reinterpret_cast<float*>(Bs);   // the fp32 rows of the row op live in B's staging area between the two phases
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 31, fh = lane >> 5;
  const long r0 = (long)blockIdx.x * RN_ROWS;
  const int D = g.D;
  // ---- loader maps.  A: thread -> row tid / 8, four pieces of 4 columns at 32 i + 4 (tid % 8) (fp32: 8 threads = 128 B) or two pieces of
  // 8 columns at 64 i + 8 (tid % 8) (16 bit).  B: 2048 16-byte pieces of a [128, 128] chunk, piece tid + 256 i: 16 threads = one 256-B row.
  const int arow = tid >> 3, ac = tid & 7;
  long grow = r0 + arow;
  if (grow > g.rows - 1) grow = g.rows - 1;   // rows past the end read the last row (never stored)
  float4 ax[4];
  uint4 ah[2];
  uint4 bv[8];
  auto load_a = [&](int k0) {
    if constexpr (!BWD) {
#pragma unroll
      for (int i = 0; i < 4; ++i) ax[i] = *reinterpret_cast<const float4*>(g.x + grow * g.ld_x + k0 + 32 * i + 4 * ac);
    } else {
#pragma unroll
      for (int i = 0; i < 2; ++i) ah[i] = *reinterpret_cast<const uint4*>(g.a16 + grow * g.ld_a + k0 + 64 * i + 8 * ac);
    }
  };
  auto store_a = [&](int k0) {
    if constexpr (!BWD) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        uint2 w;
        w.x = pack2(ax[i].x, ax[i].y), w.y = pack2(ax[i].z, ax[i].w);
        *reinterpret_cast<uint2*>(As + arow * RN_LD + 32 * i + 4 * ac) = w;
        if (g.x16 && r0 + arow < g.rows) *reinterpret_cast<uint2*>(g.x16 + (r0 + arow) * g.ld_x16 + k0 + 32 * i + 4 * ac) = w;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 2; ++i) *reinterpret_cast<uint4*>(As + arow * RN_LD + 64 * i + 8 * ac) = ah[i];
    }
  };
  // B chunk: `nrow_ld` elements between the rows of the source, chunk origin `src`
  auto load_b = [&](const bf16_t* src, long ld) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int pc = tid + 256 * i;
      bv[i] = *reinterpret_cast<const uint4*>(src + (long)(pc >> 4) * ld + 8 * (pc & 15));
    }
  };
  auto store_b = [&]() {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int pc = tid + 256 * i;
      *reinterpret_cast<uint4*>(Bs + (pc >> 4) * RN_LD + 8 * (pc & 15)) = bv[i];
    }
  };

  // ---- phase 1: scores (forward) / dP (backward), K = D
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  load_a(0);
  load_b(g.b1, D);
  for (int k0 = 0; k0 < D; k0 += RN_KC) {
    store_a(k0);
    store_b();
    __syncthreads();
    if (k0 + RN_KC < D) {   // the next chunk travels while this one is multiplied
      load_a(k0 + RN_KC);
      load_b(g.b1 + k0 + RN_KC, D);
    }
#pragma unroll
    for (int s = 0; s < RN_KC / 16; ++s) {
      const bf16x8 a = *reinterpret_cast<const bf16x8*>(As + fr * RN_LD + 16 * s + 8 * fh);
      const bf16x8 b = *reinterpret_cast<const bf16x8*>(Bs + (32 * wave + fr) * RN_LD + 16 * s + 8 * fh);
      acc = VFM_MFMA16(a, b, acc);
    }
    __syncthreads();
  }
  // the first chunk of phase 2's B operand is on its way during the row op
  load_b(g.b2, RN_TOK);
#pragma unroll
  for (int r = 0; r < 16; ++r) Ss[((r & 3) + 8 * (r >> 2) + 4 * fh) * (RN_TOK + 4) + 32 * wave + fr] = acc[r];
  __syncthreads();
  // ---- row op: wave w owns rows 8 w .. 8 w + 7, a lane the columns lane and lane + 64
#pragma unroll
  for (int i = 0; i < RN_ROWS / 4; ++i) {
    const int row = 8 * wave + i;
    const long gr = r0 + row;
    const bool live = gr < g.rows;
    const float s0 = Ss[row * (RN_TOK + 4) + lane], s1 = Ss[row * (RN_TOK + 4) + lane + 64];
    float o0, o1;
    if constexpr (!BWD) {
      const float v0 = lane < g.m ? g.c * s0 : -INFINITY, v1 = lane + 64 < g.m ? g.c * s1 : -INFINITY;
      const float mx = wave_max(fmaxf(v0, v1));
      const float e0 = __expf(v0 - mx), e1 = __expf(v1 - mx);   // exp(-inf) = 0: the pad columns carry exactly zero probability
      const float inv = 1.f / wave_sum(e0 + e1);
      o0 = e0 * inv, o1 = e1 * inv;
      if (g.p && live) {
        g.p[gr * g.ld_p + lane] = f32_to_bf16(o0);
        g.p[gr * g.ld_p + lane + 64] = f32_to_bf16(o1);
      }
    } else {
      const long pr = live ? gr : g.rows - 1;
      const float p0 = bf16_to_f32(g.p[pr * g.ld_p + lane]), p1 = bf16_to_f32(g.p[pr * g.ld_p + lane + 64]);
      const float dot = wave_sum(p0 * s0 + p1 * s1);
      o0 = g.c * p0 * (s0 - dot), o1 = g.c * p1 * (s1 - dot);
      if (live) {
        g.r16[gr * g.ld_r + lane] = f32_to_bf16(o0);
        g.r16[gr * g.ld_r + lane + 64] = f32_to_bf16(o1);
      }
    }
    Ps[row * RN_LD + lane] = f32_to_bf16(o0);
    Ps[row * RN_LD + lane + 64] = f32_to_bf16(o1);
  }
  __syncthreads();
  // ---- phase 2: K = 128 tokens, the A fragments stay in registers
  bf16x8 af[RN_TOK / 16];
#pragma unroll
  for (int s = 0; s < RN_TOK / 16; ++s) af[s] = *reinterpret_cast<const bf16x8*>(Ps + fr * RN_LD + 16 * s + 8 * fh);
  for (int d0 = 0; d0 < D; d0 += RN_KC) {
    store_b();
    __syncthreads();
    if (d0 + RN_KC < D) load_b(g.b2 + (long)(d0 + RN_KC) * RN_TOK, RN_TOK);
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
    for (int s = 0; s < RN_TOK / 16; ++s) {
      const bf16x8 b = *reinterpret_cast<const bf16x8*>(Bs + (32 * wave + fr) * RN_LD + 16 * s + 8 * fh);
      acc = VFM_MFMA16(af[s], b, acc);
    }
    const int col = d0 + 32 * wave + fr;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const long gr = r0 + (r & 3) + 8 * (r >> 2) + 4 * fh;
      if (gr < g.rows) {
        if constexpr (!BWD) {
          g.u[gr * g.ld_u + col] = f32_to_bf16(acc[r] + g.x[gr * g.ld_x + col]);
        } else {
          g.dx[gr * g.ld_dx + col] += acc[r] + bf16_to_f32(g.a16[gr * g.ld_a + col]);
        }
      }
    }
    __syncthreads();
  }
}

static int rein_check(const void* b1, const void* b2, long rows, int D, int m, const char* who) {
  VFM_CHECK(rows >= 0 && D > 0 && D % RN_KC == 0 && m >= 2 && m <= RN_TOK, VFM_E_SHAPE, "%s: D %% 128 == 0 and 2 <= token_length <= 128 (D=%d m=%d)", who, D, m);
  VFM_CHECK((uintptr_t)b1 % 16 == 0 && (uintptr_t)b2 % 16 == 0, VFM_E_ALIGN, "%s: token operands must be 16-byte aligned", who);
  return VFM_OK;
}

extern "C" int vfm_rein_mix_fwd(const float* x, long ld_x, const void* t, const void* vt, void* u, long ld_u, void* p, long ld_p, void* x16,
                                long ld_x16, long rows, int D, int m, float c, void* stream) {
  VFM_CHECK(x && t && vt && u, VFM_E_INVAL, "vfm_rein_mix_fwd: null operand");
  const int rc = rein_check(t, vt, rows, D, m, "vfm_rein_mix_fwd");
  if (rc) return rc;
  VFM_CHECK((uintptr_t)x % 16 == 0 && ld_x % 4 == 0 && ld_x >= D && ld_u >= D && (!p || ld_p >= RN_TOK) &&
                (!x16 || ((uintptr_t)x16 % 8 == 0 && ld_x16 % 4 == 0 && ld_x16 >= D)),
            VFM_E_ALIGN, "vfm_rein_mix_fwd: x 16-byte aligned with ld %% 4 == 0; leading dimensions >= the row widths");
  if (rows == 0) return VFM_OK;
  ReinArgs g = {};
  g.x = x, g.ld_x = ld_x, g.b1 = (const bf16_t*)t, g.b2 = (const bf16_t*)vt, g.u = (bf16_t*)u, g.ld_u = ld_u, g.p = (bf16_t*)p, g.ld_p = ld_p;
  g.x16 = (bf16_t*)x16, g.ld_x16 = ld_x16, g.rows = rows, g.D = D, g.m = m, g.c = c;
  hipLaunchKernelGGL(k_rein_mix<false>, dim3(cdiv(rows, RN_ROWS)), dim3(256), 0, (hipStream_t)stream, g);
  VFM_LAUNCH_CHECK();
  return VFM_OK;
}

extern "C" int vfm_rein_mix_bwd(const void* du, long ld_du, const void* p, long ld_p, const void* v, const void* tt, void* ds, long ld_ds,
                                float* dx, long ld_dx, long rows, int D, int m, float c, void* stream) {
  VFM_CHECK(du && p && v && tt && ds && dx, VFM_E_INVAL, "vfm_rein_mix_bwd: null operand");
  const int rc = rein_check(v, tt, rows, D, m, "vfm_rein_mix_bwd");
  if (rc) return rc;
  VFM_CHECK((uintptr_t)du % 16 == 0 && ld_du % 8 == 0 && ld_du >= D && ld_p >= RN_TOK && ld_ds >= RN_TOK && ld_dx >= D, VFM_E_ALIGN,
            "vfm_rein_mix_bwd: du 16-byte aligned with ld %% 8 == 0; leading dimensions >= the row widths");
  if (rows == 0) return VFM_OK;
  ReinArgs g = {};
  g.a16 = (const bf16_t*)du, g.ld_a = ld_du, g.b1 = (const bf16_t*)v, g.b2 = (const bf16_t*)tt, g.p = (bf16_t*)p, g.ld_p = ld_p;
  g.r16 = (bf16_t*)ds, g.ld_r = ld_ds, g.dx = dx, g.ld_dx = ld_dx, g.rows = rows, g.D = D, g.m = m, g.c = c;
  hipLaunchKernelGGL(k_rein_mix<true>, dim3(cdiv(rows, RN_ROWS)), dim3(256), 0, (hipStream_t)stream, g);
  VFM_LAUNCH_CHECK();
  return VFM_OK;
}
