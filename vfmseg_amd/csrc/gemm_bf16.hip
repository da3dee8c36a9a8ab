// bf16 MFMA GEMM for gfx950:  C[M,N] = epilogue(alpha * A[M,K] * B[N,K]^T), fp32 accumulation.
//
//   tile BM x BN x 64, WAVES = WM_W x WN_W waves, each wave a (BM/WM_W) x (BN/WN_W) sub-tile of 32x32x16 MFMAs
//   operands staged by LDS-DMA (global_load_lds_dwordx4) into an NS-deep ring of LDS stages, prefetch distance NS-1,
//     ONE raw s_barrier per K-step, counted s_waitcnt vmcnt(N) so the prefetch stays in flight across the barrier
//   LDS image [rows][64] bf16 = 128-B rows; 16-B chunk c of row r lives at chunk c ^ ((r>>1)&7): the swizzle is applied
//     to the per-lane SOURCE address (the DMA destination is lane-linear) and again on the ds_read_b128 fragment reads
//   epilogue through LDS: accumulators -> row-major fp32 tile -> 16-byte vector loads/stores of bias / residual / aux / C
//   XCD-aware bijective tile mapping (blocks b, b+8 share an XCD's L2)
#include "gemm_launch.h"

template <int BM, int BN, int WM_W, int WN_W, int NS>
struct Cfg {
  static constexpr int WAVES = WM_W * WN_W;
  static constexpr int THREADS = WAVES * 64;
  static constexpr int A_BYTES = BM * BK * 2, B_BYTES = BN * BK * 2;
  static constexpr int STAGE_BYTES = A_BYTES + B_BYTES;
  static constexpr int A_PIECES = BM / 8 / WAVES, B_PIECES = BN / 8 / WAVES;  // 1-KiB LDS-DMA pieces per wave
  static constexpr int PIECES = A_PIECES + B_PIECES;
  static constexpr int WM = BM / WM_W, WN = BN / WN_W;
  static constexpr int MI = WM / 32, NI = WN / 32;
  static constexpr int EPI_LD = WN + 4;                       // fp32 row stride of the epilogue image
  static constexpr int EPI_BYTES = WAVES * 32 * EPI_LD * 4;   // one 32-row slab per wave at a time
  static constexpr int SMEM = (NS * STAGE_BYTES > EPI_BYTES) ? NS * STAGE_BYTES : EPI_BYTES;
  static_assert(BM % (8 * WAVES) == 0 && BN % (8 * WAVES) == 0, "tile rows must split into whole DMA pieces per wave");
  static_assert(WM % 32 == 0 && WN % 32 == 0, "wave tile must be a multiple of the 32x32 MFMA");
};

typedef short s16x4 __attribute__((ext_vector_type(4)));

// BT = true: B is given as [K, N] row-major (N contiguous) - weight-gradient GEMMs reduce over tokens, so the activation
// operand is consumed in place and its MFMA fragments come from transposed LDS reads (ds_read_b64_tr_b16); rows k >= kb_rows
// are clamped (the A operand is zero there).
// AT = true (with BT): A is given as [K, M] row-major too (M contiguous): C = A^T B with BOTH operands token-major, the form
// of a weight gradient dW = X^T dY - no transposed copy of either operand; k-rows past the valid tokens read a zero row.
__device__ __attribute__((aligned(16))) unsigned char g_zero_row[512];
template <int BM, int BN, int WM_W, int WN_W, int NS, bool VEC, bool BT, bool AT = false>
__global__ void __launch_bounds__(WM_W* WN_W * 64)
    k_gemm_bf16(const bf16_t* __restrict__ A, long lda, const bf16_t* __restrict__ B, long ldb, long M, long N, long K,
                long stride_a, long stride_b, long stride_c, int tiles_m, int tiles_n, long kb_rows, EpiParams e, SkinnyTail sk) {
  using C = Cfg<BM, BN, WM_W, WN_W, NS>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  if constexpr (!BT && C::THREADS == 512 && C::SMEM >= 65536) {
    if (sk.nblk > 0 && (int)blockIdx.x >= tiles_m * tiles_n) {  // tail rows of M ([cls] tokens): extra blocks at the end of the grid
      skinny_tile(sk.A, sk.lda, B, ldb, sk.M, N, K, (long)((int)blockIdx.x - tiles_m * tiles_n) * 32, sk.e, 0, smem);
      return;
    }
  }
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN_W, wn = wave % WN_W;

  // ---- XCD-aware tile mapping
  const int ntiles = tiles_m * tiles_n;
  int bid = blockIdx.x;
  {
    const int q = ntiles >> 3, r = ntiles & 7, xcd = bid & 7, idx = bid >> 3;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  constexpr int GM = 8;
  const int group = bid / (GM * tiles_n);
  const int first_m = group * GM;
  const int gsz = min(tiles_m - first_m, GM);
  const int tm = first_m + (bid % (GM * tiles_n)) % gsz;
  const int tn = (bid % (GM * tiles_n)) / gsz;
  const long m0 = (long)tm * BM, n0 = (long)tn * BN;
  const long z = blockIdx.y;
  const bf16_t* Ab = A + z * stride_a;
  const bf16_t* Bb = B + z * stride_b;
  // BT: valid B rows of this batch slice (split-K batches slice the token dimension; the last slice may be short)
  long kb_valid = K;
  if constexpr (BT) {
    if (kb_rows > 0) {  // split-K slices of ONE [kb_rows, N] matrix; kb_rows == 0: independent batches, all K rows valid
      kb_valid = kb_rows - (ldb > 0 ? z * (stride_b / ldb) : 0);
      if (kb_valid > K) kb_valid = K;
      if (kb_valid < 1) kb_valid = 1;
    } else if (kb_rows < 0) {  // independent batches (one per layer) of -kb_rows valid rows each
      kb_valid = -kb_rows;
      if (kb_valid > K) kb_valid = K;
    }
  }

  // ---- per-lane DMA sources (row clamp keeps every load in bounds; clamped rows are never stored)
  const int lr = lane >> 3, pc = lane & 7;
  const bf16_t* a_src[C::A_PIECES];
  const bf16_t* b_src[C::B_PIECES];
  int at_row[C::A_PIECES];
#pragma unroll
  for (int j = 0; j < C::A_PIECES; ++j) {
    if constexpr (!AT) {
      const int r = (wave * C::A_PIECES + j) * 8 + lr;
      long gm = m0 + r;
      if (gm > M - 1) gm = M - 1;
      a_src[j] = Ab + gm * lda + ((pc ^ ((r >> 1) & 7)) << 3);
    } else {
      static_assert(!AT || (BT && BM == 128), "transposed-A path: BM = 128 (256-byte LDS rows), together with transposed B");
      const int piece = wave * C::A_PIECES + j;          // 1 KiB = 4 k-rows x 256 B
      const int r = piece * 4 + (lane >> 4);
      const int c = (lane & 15) ^ ((r & 3) << 2);
      long gm = m0 + c * 8;
      if (gm > M - 8) gm = M - 8;                        // M % 8 == 0: clamped chunks are never stored
      at_row[j] = r;
      a_src[j] = Ab + gm;
    }
  }
  int bt_row[C::B_PIECES];  // BT: k-row of this lane inside the tile, per piece
#pragma unroll
  for (int j = 0; j < C::B_PIECES; ++j) {
    if constexpr (!BT) {
      const int r = (wave * C::B_PIECES + j) * 8 + lr;
      long gn = n0 + r;
      if (gn > N - 1) gn = N - 1;
      b_src[j] = Bb + gn * ldb + ((pc ^ ((r >> 1) & 7)) << 3);
    } else {
      static_assert(!BT || BN == 128, "transposed-B path is built for BN = 128 (256-byte LDS rows)");
      const int piece = wave * C::B_PIECES + j;          // 1 KiB = 4 k-rows x 256 B
      const int r = piece * 4 + (lane >> 4);
      const int c = (lane & 15) ^ ((r & 3) << 2);
      long gn = n0 + c * 8;
      if (gn > N - 8) gn = N - 8;                        // N % 8 == 0: clamped chunks are never stored
      bt_row[j] = r;
      b_src[j] = Bb + gn;
    }
  }
  auto stage = [&](int slot, long k0) {
    char* sa = smem + slot * C::STAGE_BYTES;
    char* sb = sa + C::A_BYTES;
#pragma unroll
    for (int j = 0; j < C::A_PIECES; ++j) {
      if constexpr (!AT) {
        glds16(a_src[j] + k0, sa + (wave * C::A_PIECES + j) * 1024);
      } else {
        const long kr = k0 + at_row[j];
        const bf16_t* src = kr < kb_valid ? a_src[j] + kr * lda : reinterpret_cast<const bf16_t*>(g_zero_row) + (lane & 15) * 8;
        glds16(src, sa + (wave * C::A_PIECES + j) * 1024);
      }
    }
#pragma unroll
    for (int j = 0; j < C::B_PIECES; ++j) {
      if constexpr (!BT) {
        glds16(b_src[j] + k0, sb + (wave * C::B_PIECES + j) * 1024);
      } else {
        long kr = k0 + bt_row[j];
        if (kr > kb_valid - 1) kr = kb_valid - 1;
        glds16(b_src[j] + kr * ldb, sb + (wave * C::B_PIECES + j) * 1024);
      }
    }
  };

  f32x16 acc[C::MI][C::NI];
#pragma unroll
  for (int i = 0; i < C::MI; ++i)
#pragma unroll
    for (int j = 0; j < C::NI; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int fr = lane & 31, fh = lane >> 5;
  int a_off[C::MI], a_sw[C::MI], b_off[C::NI], b_sw[C::NI];
#pragma unroll
  for (int i = 0; i < C::MI; ++i) {
    const int r = wm * C::WM + i * 32 + fr;
    a_off[i] = r * 128;
    a_sw[i] = (r >> 1) & 7;
  }
#pragma unroll
  for (int j = 0; j < C::NI; ++j) {
    const int r = wn * C::WN + j * 32 + fr;
    b_off[j] = r * 128;
    b_sw[j] = (r >> 1) & 7;
  }

  const int nk = (int)(K / BK);
  // ---- prologue: fill NS-1 stages
#pragma unroll
  for (int s = 0; s < NS - 1; ++s)
    if (s < nk) stage(s, (long)s * BK);

  for (int t = 0; t < nk; ++t) {
    // tile t must have landed: groups issued so far cover tiles t .. min(t+NS-2, nk-1)
    const int inflight = min(NS - 2, nk - 1 - t);  // younger groups allowed to stay in flight
    if (inflight >= NS - 2 && NS >= 2) wait_vmcnt<(NS - 2) * C::PIECES>();
    else if (NS >= 4 && inflight == NS - 3) wait_vmcnt<(NS >= 3 ? (NS - 3) : 0) * C::PIECES>();
    else if (NS >= 5 && inflight == NS - 4) wait_vmcnt<(NS >= 4 ? (NS - 4) : 0) * C::PIECES>();
    else wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();  // everyone's pieces of tile t are in LDS; everyone finished reading tile t-1
    if (t + NS - 1 < nk) stage((t + NS - 1) % NS, (long)(t + NS - 1) * BK);  // refills the slot tile t-1 used
    const char* sa = smem + (t % NS) * C::STAGE_BYTES;
    const char* sb = sa + C::A_BYTES;
    // fragment double buffering: the ds_reads of k-step s+1 are issued before the MFMAs of k-step s
    auto read_b = [&](int s2, int j) -> bf16x8 {
      if constexpr (!BT) {
        return *reinterpret_cast<const bf16x8*>(sb + b_off[j] + (((2 * s2 + fh) ^ b_sw[j]) << 4));
      } else {
        const int g = lane >> 4, i2 = lane & 15, q = i2 >> 2, p = i2 & 3, h2 = g >> 1;
        const int chunk = (wn * C::WN + j * 32) / 8 + 2 * (g & 1) + (p >> 1);
        const int r0 = 16 * s2 + 8 * h2 + q, r1 = r0 + 4;
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) s16x4*)(sb + r0 * 256 + ((chunk ^ ((r0 & 3) << 2)) << 4) + ((p & 1) << 3)));
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) s16x4*)(sb + r1 * 256 + ((chunk ^ ((r1 & 3) << 2)) << 4) + ((p & 1) << 3)));
        union { struct { s16x4 a, b; } st; bf16x8 v; } u;
        u.st.a = lo;
        u.st.b = hi;
        return u.v;
      }
    };
    auto read_a = [&](int s2, int i) -> bf16x8 {
      if constexpr (!AT) {
        return *reinterpret_cast<const bf16x8*>(sa + a_off[i] + (((2 * s2 + fh) ^ a_sw[i]) << 4));
      } else {
        const int g = lane >> 4, i2 = lane & 15, q = i2 >> 2, p = i2 & 3, h2 = g >> 1;
        const int chunk = (wm * C::WM + i * 32) / 8 + 2 * (g & 1) + (p >> 1);
        const int r0 = 16 * s2 + 8 * h2 + q, r1 = r0 + 4;
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) s16x4*)(sa + r0 * 256 + ((chunk ^ ((r0 & 3) << 2)) << 4) + ((p & 1) << 3)));
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) s16x4*)(sa + r1 * 256 + ((chunk ^ ((r1 & 3) << 2)) << 4) + ((p & 1) << 3)));
        union { struct { s16x4 a, b; } st; bf16x8 v; } u;
        u.st.a = lo;
        u.st.b = hi;
        return u.v;
      }
    };
    bf16x8 af[2][C::MI], bfr[2][C::NI];
#pragma unroll
    for (int i = 0; i < C::MI; ++i) af[0][i] = read_a(0, i);
#pragma unroll
    for (int j = 0; j < C::NI; ++j) bfr[0][j] = read_b(0, j);
#pragma unroll
    for (int s = 0; s < BK / 16; ++s) {
      const int cur = s & 1, nxt = cur ^ 1;
      if (s + 1 < BK / 16) {
#pragma unroll
        for (int i = 0; i < C::MI; ++i)
          af[nxt][i] = read_a(s + 1, i);
#pragma unroll
        for (int j = 0; j < C::NI; ++j) bfr[nxt][j] = read_b(s + 1, j);
      }
#pragma unroll
      for (int i = 0; i < C::MI; ++i)
#pragma unroll
        for (int j = 0; j < C::NI; ++j)
          acc[i][j] = VFM_MFMA16(af[cur][i], bfr[cur][j], acc[i][j]);
    }
  }

  // ---- epilogue
  const long zoff = z * stride_c;
  __syncthreads();  // all LDS reads of the last stage are done; the ring is reused as the epilogue image
  float* img = reinterpret_cast<float*>(smem) + wave * 32 * C::EPI_LD;
  if constexpr (VEC) epi_wave_tile<C::MI, C::NI, 1>(e, zoff, acc, img, lane, m0 + wm * C::WM, n0 + wn * C::WN, M, N);
  else epi_scalar<C::MI, C::NI, 1>(e, zoff, acc, img, lane, m0 + wm * C::WM, n0 + wn * C::WN, M, N);
}

// tail != null (the plan lets the <= 32 rows past the last full 128-row block ride along, GEMM_TAIL_BLOCKS): they run as extra blocks
// of the same launch.  Only a configuration that can host them (512 threads, >= 64 KiB LDS: hosts_tail in the config table) is given any.
template <int BM, int BN, int WM_W, int WN_W, int NS, bool VEC, bool BT, bool AT = false>
static void launch_one(const vfm_gemm_desc* d, hipStream_t s, const vfm_gemm_desc* tail = nullptr) {
  using C = Cfg<BM, BN, WM_W, WN_W, NS>;
  const int tiles_m = cdiv(d->M, BM), tiles_n = cdiv(d->N, BN);
  const long batch = d->batch > 0 ? d->batch : 1;
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)k_gemm_bf16<BM, BN, WM_W, WN_W, NS, VEC, BT, AT>, hipFuncAttributeMaxDynamicSharedMemorySize, C::SMEM);
    attr = true;
  }
  const SkinnyTail sk = skinny_tail(tail);
  dim3 grid(tiles_m * tiles_n + sk.nblk, (unsigned)batch), blk(C::THREADS);
  const long ldb = BT ? d->sb_k : d->sb_n;
  const long kb_rows = d->kb_rows;
  hipLaunchKernelGGL((k_gemm_bf16<BM, BN, WM_W, WN_W, NS, VEC, BT, AT>), grid, blk, C::SMEM, s, (const bf16_t*)d->A, AT ? d->sa_k : d->sa_m,
                     (const bf16_t*)d->B, ldb, d->M, d->N, d->K, d->stride_a, d->stride_b, d->stride_c, tiles_m, tiles_n, kb_rows,
                     make_epi(d), sk);
}

// the two-stage configs of the table: 10: 64x64 2x2 NS4   16: 256x256 4x4 NS2   17: 128x128 2x4 NS2   18: 64x128 2x2 NS2
template <int ID, int BM, int BN, int WM_W, int WN_W, int NS>
static void launch_two_stage(const vfm_gemm_desc* d, hipStream_t s, const GemmPlan& p, const vfm_gemm_desc* tail) {
  using C = Cfg<BM, BN, WM_W, WN_W, NS>;
  static_assert(kGemmConfigs[gemm_config_index(ID)].hosts_tail == (C::THREADS == 512 && C::SMEM >= 65536), "config table: hosts_tail");
  if (p.vec) launch_one<BM, BN, WM_W, WN_W, NS, true, false>(d, s, tail);
  else launch_one<BM, BN, WM_W, WN_W, NS, false, false>(d, s, tail);
}
void vfm_gemm_launch_10(const vfm_gemm_desc* d, hipStream_t s, const GemmPlan& p, const vfm_gemm_desc* tail) { launch_two_stage<10, 64, 64, 2, 2, 4>(d, s, p, tail); }
void vfm_gemm_launch_16(const vfm_gemm_desc* d, hipStream_t s, const GemmPlan& p, const vfm_gemm_desc* tail) { launch_two_stage<16, 256, 256, 4, 4, 2>(d, s, p, tail); }
void vfm_gemm_launch_17(const vfm_gemm_desc* d, hipStream_t s, const GemmPlan& p, const vfm_gemm_desc* tail) { launch_two_stage<17, 128, 128, 2, 4, 2>(d, s, p, tail); }
void vfm_gemm_launch_18(const vfm_gemm_desc* d, hipStream_t s, const GemmPlan& p, const vfm_gemm_desc* tail) { launch_two_stage<18, 64, 128, 2, 2, 2>(d, s, p, tail); }

template <int BM, int WM_W, int WN_W, int NS = 2>
static void launch_bt(const vfm_gemm_desc* d, hipStream_t s, bool vec) {
  if (vec) launch_one<BM, 128, WM_W, WN_W, NS, true, true>(d, s);
  else launch_one<BM, 128, WM_W, WN_W, NS, false, true>(d, s);
}

// ------------------------------------------------------------------------------------------------ skinny tail
__global__ void __launch_bounds__(512) k_gemm_bf16_skinny(const bf16_t* __restrict__ A, long lda, const bf16_t* __restrict__ B, long ldb,
                                                          long M, long N, long K, long stride_a, long stride_b, long stride_c,
                                                          EpiParams e) {
  __shared__ __attribute__((aligned(16))) char stg[65536];
  const long z = blockIdx.y;
  skinny_tile(A + z * stride_a, lda, B + z * stride_b, ldb, M, N, K, (long)blockIdx.x * 32, e, z * stride_c, stg);
}

static void launch_skinny(const vfm_gemm_desc* d, hipStream_t s) {
  const long batch = d->batch > 0 ? d->batch : 1;
  hipLaunchKernelGGL(k_gemm_bf16_skinny, dim3(cdiv(d->N, 32), (unsigned)batch), dim3(512), 0, s, (const bf16_t*)d->A, d->sa_m,
                     (const bf16_t*)d->B, d->sb_n, d->M, d->N, d->K, d->stride_a, d->stride_b, d->stride_c, make_epi(d));
}

// ------------------------------------------------------------------------------------------------ dispatch
GemmKnobs g_gemm_knobs;
long g_nt_bytes = 0;

// the launchers in the order of the rows of kGemmConfigs
typedef void (*GemmLaunch)(const vfm_gemm_desc*, hipStream_t, const GemmPlan&, const vfm_gemm_desc*);
#define VFM_GEMM_LAUNCHER(id, family, min_k, span, hosts, deep, msg) vfm_gemm_launch_##id,
static const GemmLaunch kGemmLaunch[] = {VFM_GEMM_CONFIGS(VFM_GEMM_LAUNCHER)};
#undef VFM_GEMM_LAUNCHER

// gemm_select (gemm_select.h) decides everything; this only builds the descriptors of a peeled tail and launches what the plan says
int vfm_gemm_bf16_impl(const vfm_gemm_desc* d0, hipStream_t s) {
  const GemmPlan p = gemm_select(*d0, g_gemm_knobs);
  if (p.err) VFM_FAIL(p.err, "vfm_gemm(bf16): %s (gemm_cfg %d)", kGemmMsgs[p.msg], g_gemm_knobs.force_cfg);
  vfm_gemm_desc dm, dt;
  const vfm_gemm_desc* d = d0;
  if (p.tail_rows > 0) {
    dm = *d0, dt = *d0;
    const long mm = d0->M - p.tail_rows;
    dm.M = mm;
    dt.M = p.tail_rows;
    auto adv = [&](const void* ptr, int dt_, long ld) -> const void* {
      return ptr ? (const void*)((const char*)ptr + mm * ld * (dt_ == VFM_BF16 || dt_ == VFM_SPLIT3 ? 2 : 4)) : nullptr;
    };
    dt.A = adv(d0->A, VFM_BF16, d0->sa_m);
    dt.C = (void*)adv(d0->C, d0->c_dt, d0->ldc);
    dt.residual = adv(d0->residual, d0->r_dt, d0->ldr);
    dt.aux = adv(d0->aux, d0->aux_dt, d0->ld_aux);
    dt.C2 = (void*)adv(d0->C2, d0->c2_dt, d0->ldc2);
    d = &dm;
  }
  const vfm_gemm_desc* ride = (p.tail_mode == GEMM_TAIL_BLOCKS || p.tail_mode == GEMM_TAIL_INSIDE) ? &dt : nullptr;
  switch (p.kind) {
    case GEMM_SKINNY: launch_skinny(d, s); break;
    case GEMM_BT64: launch_bt<64, 1, 4>(d, s, p.vec); break;
    case GEMM_BT128: launch_bt<128, 2, 4>(d, s, p.vec); break;
    case GEMM_ATBT:
      if (p.vec) launch_one<128, 128, 2, 4, 2, true, true, true>(d, s);
      else launch_one<128, 128, 2, 4, 2, false, true, true>(d, s);
      break;
    default: kGemmLaunch[gemm_config_index(p.cfg)](d, s, p, ride); break;
  }
  if (p.tail_mode == GEMM_TAIL_SEPARATE) launch_skinny(&dt, s);
  return VFM_OK;
}
