// Host side shared by the bf16 GEMM files: one launcher per row of the config table (gemm_select.h), defined next to its kernel.
//   d: the descriptor of the tile launch; p: its plan (p.vec, p.tail_mode)
//   tail: the descriptor of the peeled tail rows when the plan lets them ride along with this launch (GEMM_TAIL_BLOCKS / GEMM_TAIL_INSIDE),
//         nullptr otherwise
#pragma once
#include "gemm_dev.h"
#include "gemm_select.h"

#define VFM_GEMM_DECLARE(id, family, min_k, span, hosts, deep, msg) \
  void vfm_gemm_launch_##id(const vfm_gemm_desc* d, hipStream_t s, const GemmPlan& p, const vfm_gemm_desc* tail);
VFM_GEMM_CONFIGS(VFM_GEMM_DECLARE)
#undef VFM_GEMM_DECLARE

// the tail rows as the tile kernels take them: nblk skinny blocks of 32 columns (0: no tail rows in this launch)
static inline SkinnyTail skinny_tail(const vfm_gemm_desc* tail) {
  SkinnyTail sk;
  sk.nblk = 0;
  if (tail) sk.A = (const bf16_t*)tail->A, sk.lda = tail->sa_m, sk.M = tail->M, sk.nblk = cdiv(tail->N, 32), sk.e = make_epi(tail);
  return sk;
}
