// vfm_tune: the tuning / experiment knobs of the library by name (bench.py --tune KEY=INT, tools/ab_step.py, tools/ab_eval.py).
// Each knob lives in (and is documented by) the file that reads it; this is only the name -> variable table.
#include <limits.h>
#include "attn_common.h"
#include "gemm_select.h"

#ifndef VFM_EXPERIMENTAL_GEMM
int g_ps_burst = 0;   // gemm_ps.hip is not built: "ps_burst" is accepted and ignored
#endif

namespace {
int g_nt_mb = 0;      // "gemm_nt_mb": g_nt_bytes in MiB
struct Knob { const char* key; int* value; int lo, hi; };
const Knob kKnobs[] = {
    {"gemm_cfg", &g_gemm_knobs.force_cfg, INT_MIN, INT_MAX},
    {"gemm_use_pp", &g_gemm_knobs.use_pp, INT_MIN, INT_MAX},
    {"gemm_use_ps", &g_gemm_knobs.use_ps, INT_MIN, INT_MAX},
    {"gemm_use_192", &g_gemm_knobs.use_192, INT_MIN, INT_MAX},
    {"gemm_w44_k", &g_gemm_knobs.w44_k, 0, INT_MAX},
    {"gemm_deep_sep_k", &g_gemm_knobs.deep_sep_k, 0, INT_MAX},   // (a negative value used to mean "skip the tail rows": a timing diagnostic with wrong results)
    {"gemm_deep_tail_k", &g_gemm_knobs.deep_tail_k, INT_MIN, INT_MAX},
    {"gemm_batch_tiles", &g_gemm_knobs.batch_tiles, INT_MIN, INT_MAX},
    {"gemm_bt64", &g_gemm_knobs.bt64, INT_MIN, INT_MAX},
    {"gemm_fold_tail", &g_gemm_knobs.fold_tail, INT_MIN, INT_MAX},
    {"gemm_split_tail", &g_gemm_knobs.split_tail, INT_MIN, INT_MAX},
    {"gemm_nt_mb", &g_nt_mb, INT_MIN, INT_MAX},
    {"pp_dbg", &g_pp_dbg, INT_MIN, INT_MAX},
    {"ps_burst", &g_ps_burst, INT_MIN, INT_MAX},
    {"attn_short_grid", &g_attn_short_grid, INT_MIN, INT_MAX},
    {"attn_il", &g_attn_il, 0, 3},
    {"attn_xcd", &g_attn_xcd, INT_MIN, INT_MAX},
    {"attn_fwd64", &g_attn_fwd64, INT_MIN, INT_MAX},
    {"attn_lds_pad", &g_attn_lds_pad, INT_MIN, INT_MAX},
};
}  // namespace

extern "C" int vfm_tune(const char* key, int value) {
  for (const Knob& k : kKnobs) {
    if (!key || strcmp(key, k.key) != 0) continue;
    if (value < k.lo || value > k.hi) VFM_FAIL(VFM_E_INVAL, "vfm_tune(%s): %d is outside %d .. %d", k.key, value, k.lo, k.hi);
    *k.value = value;
    g_nt_bytes = (long)g_nt_mb << 20;
    return VFM_OK;
  }
  VFM_FAIL(VFM_E_INVAL, "vfm_tune: unknown key");
}
