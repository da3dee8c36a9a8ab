// Host program of tests/test_gemm_dispatch_cpu.py: reads dispatch cases (rows of NCOL int64), runs the pure selector of
// vfmseg_amd/csrc/gemm_select.h on each and writes one row of NOUT int32 per case.  No HIP anywhere: plain g++.
//   gemm_dispatch_main cases.bin plans.bin     -> plans
//   gemm_dispatch_main --ids                   -> the ids of the config table, one line
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "gemm_select.h"

// case columns: M N K batch layout epi sa_m bias | gemm_cfg use_pp use_192 w44_k split_tail fold_tail bt64 batch_tiles deep_tail_k deep_sep_k use_ps
//   layout 0: A [M,K], B [N,K]   1: B given as [K,N]   2: A given as [K,M] as well
//   epi 0: every epilogue operand 16-byte aligned   1: ldc = N + 2 (scalar epilogue)
//   sa_m: row stride of A (0 = K)   bias: 1 = an aligned fp32 bias (what the persistent kernel's eligibility looks at)
enum { NCOL = 19, NOUT = 6 };

static vfm_gemm_desc make_desc(const int64_t* c) {
  vfm_gemm_desc d;
  memset(&d, 0, sizeof(d));
  const long M = c[0], N = c[1], K = c[2], batch = c[3];
  d.A = (const void*)(uintptr_t)0x10000000, d.B = (const void*)(uintptr_t)0x20000000, d.C = (void*)(uintptr_t)0x30000000;
  d.in_dt = VFM_BF16, d.c_dt = VFM_BF16, d.alpha = 1.f;
  d.M = M, d.N = N, d.K = K;
  d.sa_m = c[6] ? c[6] : K, d.sa_k = 1, d.sb_n = K, d.sb_k = 1;
  if (c[4] >= 1) d.sb_n = 1, d.sb_k = N;
  if (c[4] == 2) d.sa_m = 1, d.sa_k = M;
  d.ldc = c[5] ? N + 2 : N;
  if (c[7]) d.bias = (const float*)(uintptr_t)0x40000000;
  d.batch = batch;
  if (batch > 1) d.stride_a = M * K, d.stride_b = N * K, d.stride_c = M * d.ldc;
  return d;
}

static GemmKnobs make_knobs(const int64_t* c) {
  GemmKnobs k;
  k.force_cfg = (int)c[8], k.use_pp = (int)c[9], k.use_192 = (int)c[10], k.w44_k = (int)c[11], k.split_tail = (int)c[12];
  k.fold_tail = (int)c[13], k.bt64 = (int)c[14], k.batch_tiles = (int)c[15], k.deep_tail_k = (int)c[16], k.deep_sep_k = (int)c[17];
  k.use_ps = (int)c[18];
  return k;
}

int main(int argc, char** argv) {
  if (argc == 2 && strcmp(argv[1], "--ids") == 0) {
    for (const GemmConfig& g : kGemmConfigs) printf("%d ", g.id);
    printf("\n");
    return 0;
  }
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<int64_t> cases;
  int64_t row[NCOL];
  while (fread(row, sizeof(int64_t), NCOL, f) == NCOL) cases.insert(cases.end(), row, row + NCOL);
  fclose(f);
  const size_t n = cases.size() / NCOL;
  std::vector<int32_t> out(n * NOUT);
  for (size_t i = 0; i < n; ++i) {
    const vfm_gemm_desc d = make_desc(&cases[i * NCOL]);
    const GemmPlan p = gemm_select(d, make_knobs(&cases[i * NCOL]));
    int32_t* o = &out[i * NOUT];
    o[0] = p.err, o[1] = p.kind, o[2] = p.cfg, o[3] = p.vec, o[4] = (int32_t)p.tail_rows, o[5] = p.tail_mode;
  }
  f = fopen(argv[2], "wb");
  if (!f) return 2;
  fwrite(out.data(), sizeof(int32_t), out.size(), f);
  fclose(f);
  return 0;
}
