// Which kernel a bf16 GEMM runs on: the knobs, the config table and the selector.  No HIP in here (plain C++17, compiled on the host by
// tests/test_gemm_dispatch_cpu.py, which pins every plan of a large case list): gemm_bf16.hip turns a GemmPlan into launches.
#pragma once
#include <stdint.h>
#include "../../include/vfmseg_hip.h"

// ------------------------------------------------------------------------------------------------ knobs (vfm_tune, tune.hip)
struct GemmKnobs {
  int force_cfg = -1;   // vfm_tune("gemm_cfg"): a config id of the table below instead of the rules (-1 = rules)
  int split_tail = 3;  // bit 0: peel the tail rows of M off; bit 1: ... except for shapes on the 64-row tiles
  int batch_tiles = 1;  // count the batch in the tile-count heuristics
  int bt64 = 1;       // transposed-B GEMMs with few tiles use 64-row tiles
  int fold_tail = 1;  // run the tail rows as extra blocks of the tile kernel's launch
  // bit 0: 256x256 ping-pong kernel instead of config 16; bit 1: 128x128 ping-pong kernel (gemm_pp.hip); bit 3: N >= 2048 stays
  // on the 128x128 tiles; bit 4: whole waves of 256x256 tiles go to the 8-wave 64-wide-K-tile kernel (gemm_w4.hip); bit 5: the
  // 128x128 tiles run through the five-chunk ring kernel (config 34) instead of the two-stage kernel (config 17).
  // Default 40, measured inside the train step (bench.py --tune gemm_use_pp=...): 128x128 tiles / 8 waves / two blocks per CU win
  // on every shape of the path - co-resident blocks overlap one tile's epilogue traffic (fc1 writes 64 MB per call) with another
  // tile's main loop, which a one-block-per-CU kernel cannot - and the 2.5-K-tile ring beats the two-stage pipeline by 5-18 %
  // per shape (+2.6 % images/s).  The big-tile kernels win on long-K / light-epilogue shapes (4096^3: 1.26 PF vs 1.0) and stay
  // selectable per call (vfm_tune gemm_cfg 30..33).
  int use_pp = 184;  // round 3: 40 -> 184 (bit 4: fc1 forward / fc2 input gradient on 256 x 256 tiles, +1.7 % images/s; bit 7: the qkv projection too, +1.0 %)
  // the persistent two-accumulator kernel (gemm_ps.hip) for whole rounds of 256 x 256 regions with a bf16 epilogue: OFF by default.  Round 3,
  // one-process A/B inside the train step (tools/ab_step.py, profiles/r03_ab_step_gemm.log): persistent kernel 132.7 images/s, 128 x 128 ring
  // kernel 133.1, 256 x 256 8-wave ring kernel (gemm_use_pp bit 4) 134.5 - the form with the fewest operand bytes per flop wins once its
  // epilogue is the cheap eight-column one; hiding half of the epilogue under the next sub-tile's loop does not pay
  int use_ps = 0;
  // 192 x 256 tiles (config 40) for the large-M GEMMs of the 1024^2 predictions (nine windows = 9216 rows) wherever they
  // fill the 256 CUs' rounds better than 256 x 256 tiles do.  tools/bench_gemm_step.py SHAPES=eval (profiles/r03_gemm_eval_shapes.log):
  // DINOv2 fc2 / proj / fc1 98.1 -> 83.8 / 33.2 -> 29.8 / 100.5 -> 94.8 us, SAM-H qkv / proj / fc2 106.3 -> 89.8 / 42.0 -> 37.0 / 127.5 -> 109.7 us;
  // bit 1: 256 x 256 tiles for the shapes they fill to >= 80 % (DINOv2 qkv [9216 x 3072]: 69.3 -> 64.1 us).  vfm_tune gemm_use_192.
  int use_192 = 3;
  int w44_k = 1024;     // vfm_tune("gemm_w44_k"): from this K on the 128 x 128 ring kernel runs as four waves of 64 x 64 (config 52) instead of eight of
                        // 64 x 32 (config 34): +0.6 % images/s inside the train step, one process, interleaved (profiles/r04_ab_step_w44.log); 0 = never
  int deep_sep_k = 0;   // K from which one-tile-per-CU launches WITH tail rows take the seven-chunk ring and leave the tail rows to a skinny
                        // launch of their own (vfm_tune gemm_deep_sep_k; 0 = never)
  int deep_tail_k = 0;  // K from which one-tile-per-CU launches WITH tail rows take the seven-chunk ring, the tail rows riding
                        // inside the regular blocks (gemm_w4.hip CLSIN); 0 = never (five-chunk ring + tail blocks).  Measured:
                        // with cold operands 62.8 -> 53.9 us at K = 4096 (19.8 -> 22.2 at K = 1024), inside the train step
                        // (operands warm in L2 / Infinity Cache) 127.1 -> 124.6 images/s with K >= 2048: off
};
extern GemmKnobs g_gemm_knobs;   // the process-wide instance (gemm_bf16.hip), written by vfm_tune
// the other knobs of the GEMM files that vfm_tune writes
extern long g_nt_bytes;   // gemm_bf16.hip, vfm_tune("gemm_nt_mb"): outputs of at least this many bytes are stored nontemporally (0 = never)
extern int g_pp_dbg;      // gemm_pp.hip, vfm_tune("pp_dbg"): timing-diagnostic instances of the ping-pong / ring kernels
extern int g_ps_burst;    // gemm_ps.hip (experimental builds), vfm_tune("ps_burst")

// ------------------------------------------------------------------------------------------------ config table
// experiment vehicles, built only with VFMSEG_EXPERIMENTAL=1 (vfmseg_amd/csrc/build.py EXPERIMENTAL): the persistent two-accumulator kernel
// (gemm_ps.hip, round 3) and the 4-wave 16x16x32 256x256 kernel (gemm_v5.hip, round 4).  Neither beat the ring kernels of gemm_w4.hip
// (DESIGN.md section 5.1); without them their configs answer VFM_E_UNSUPPORTED and the knobs that select them are ignored.
#ifdef VFM_EXPERIMENTAL_GEMM
constexpr bool kGemmExperimental = true;
#else
constexpr bool kGemmExperimental = false;
#endif

enum GemmFamily { GEMM_FAM_TWO_STAGE, GEMM_FAM_PP, GEMM_FAM_RING, GEMM_FAM_SPLITK, GEMM_FAM_PS, GEMM_FAM_V5 };
enum GemmMsg {
  GEMM_MSG_NONE, GEMM_MSG_UNKNOWN, GEMM_MSG_RETIRED, GEMM_MSG_EXPERIMENT, GEMM_MSG_PP256, GEMM_MSG_PP128, GEMM_MSG_RING256, GEMM_MSG_DEEP,
  GEMM_MSG_SPLITK, GEMM_MSG_W44, GEMM_MSG_T192, GEMM_MSG_V5, GEMM_MSG_PS2, GEMM_MSG_PS1
};
constexpr const char* kGemmMsgs[] = {
    "",
    "unknown config",
    "retired config: the two-stage sweep configs 0-9, 11-15 and 19-29 are no longer built (live: 10, 16, 17, 18)",
    "gemm_ps.hip / gemm_v5.hip (configs 37, 38, 50) are experiments: build with VFMSEG_EXPERIMENTAL=1",
    "the ping-pong kernel needs K >= 128",
    "the 128x128 ping-pong kernel needs K >= 256",
    "the 64-wide-K-tile ring kernels need K >= 128 and operands spanning < 4 GiB",
    "the deep-ring 128x128 kernels need K >= 256 and operands spanning < 4 GiB",
    "the split-K ring kernel needs K % 128 == 0, K >= 512, one batch, <= 512 tiles of 128 x 128, a 16-byte aligned epilogue",
    "the 4-wave 128x128 kernel needs K >= 128 and operands spanning < 4 GiB",
    "the 192x256 kernel needs K >= 128 and operands spanning < 4 GiB",
    "the 16x16x32 256x256 kernel needs K >= 128 and operands spanning < 4 GiB",
    "the persistent kernel needs M % 256 == 0, N % 256 == 0, K % 64 == 0, K >= 576 and a bf16 bias / GELU / multiply epilogue",
    "the persistent kernel needs M % 256 == 0, N % 128 == 0, K % 64 == 0, K >= 576 and a bf16 bias / GELU / multiply epilogue",
};

// One row per config id (also the sweep space of tools/bench_gemm.py); X(id, family, min K, span, hosts tail, deep ring, message).
//   launcher: vfm_gemm_launch_<id>, defined next to its kernel (gemm_bf16.hip / gemm_pp.hip / gemm_w4.hip / gemm_ps.hip / gemm_v5.hip)
//   min K   : shortest K of the kernel's pipeline
//   span    : rows past M / N that (M + span) * lda and (N + span) * ldb must keep under 2^31 elements (32-bit operand offsets); 0 = none
//   hosts   : can host skinny blocks for the tail rows: 512 threads and at least 64 KiB of LDS (two-stage family), a ring of at least
//             64 KiB (the other families) - each launcher static_asserts its row against its template's constants
//   deep    : deep ring, one block per CU: <= 8 tail rows ride inside the regular blocks (CLSIN) instead of in blocks of their own
//  10: 64x64 2x2 NS4    16: 256x256 4x4 NS2   17: 128x128 2x4 NS2  18: 64x128 2x2 NS2                    (two-stage kernel, gemm_bf16.hip)
//  30: 256x256 ping-pong   31: 128x128 ping-pong                                                         (gemm_pp.hip)
//  32 / 33: 256x256 ring, 4 / 8 waves   34: 128x128 five-chunk ring, 8 waves   35 / 36: seven- / nine-chunk ring (one block per CU)
//  39 / 40: 192x256 ring, 4 / 8 waves   52: 128x128 ring, 4 waves of 64x64 (1.0 fragment reads per MFMA instead of 1.5)   (gemm_w4.hip)
//  51: 128 x 128 ring kernel, two blocks per tile (one per half of K), in-kernel fix-up.  Never chosen by the rules: on the
//      shapes it was built for (the N = 1024 GEMMs of the coarse prediction pass, 128 tiles) the exchange of the partial sums costs
//      what the second half of the CUs gains (fc2 [2049 x 1024 x 4096] 38.6 -> 37.6 us, proj 14.0 -> 17.9: profiles/r04_gemm_splitk_eval.log)
//  37 / 38: persistent kernel, 256x256 / 256x128 regions (gemm_ps.hip)   50: 256x256, 4 waves, 16x16x32 MFMA (gemm_v5.hip)
#define VFM_GEMM_CONFIGS_SHIPPED(X)                                  \
  X(10, GEMM_FAM_TWO_STAGE, 0, 0, false, false, GEMM_MSG_NONE)       \
  X(16, GEMM_FAM_TWO_STAGE, 0, 0, false, false, GEMM_MSG_NONE)       \
  X(17, GEMM_FAM_TWO_STAGE, 0, 0, true, false, GEMM_MSG_NONE)        \
  X(18, GEMM_FAM_TWO_STAGE, 0, 0, false, false, GEMM_MSG_NONE)       \
  X(30, GEMM_FAM_PP, 128, 0, true, false, GEMM_MSG_PP256)            \
  X(31, GEMM_FAM_PP, 256, 0, true, false, GEMM_MSG_PP128)            \
  X(32, GEMM_FAM_RING, 128, 256, true, false, GEMM_MSG_RING256)      \
  X(33, GEMM_FAM_RING, 128, 256, true, false, GEMM_MSG_RING256)      \
  X(34, GEMM_FAM_RING, 128, 256, true, false, GEMM_MSG_RING256)      \
  X(35, GEMM_FAM_RING, 256, 256, true, true, GEMM_MSG_DEEP)          \
  X(36, GEMM_FAM_RING, 256, 256, true, true, GEMM_MSG_DEEP)          \
  X(39, GEMM_FAM_RING, 128, 256, true, false, GEMM_MSG_T192)         \
  X(40, GEMM_FAM_RING, 128, 256, true, false, GEMM_MSG_T192)         \
  X(51, GEMM_FAM_SPLITK, 512, 256, true, false, GEMM_MSG_SPLITK)     \
  X(52, GEMM_FAM_RING, 128, 256, true, false, GEMM_MSG_W44)
#ifdef VFM_EXPERIMENTAL_GEMM
#define VFM_GEMM_CONFIGS(X)                                          \
  VFM_GEMM_CONFIGS_SHIPPED(X)                                        \
  X(37, GEMM_FAM_PS, 576, 256, true, false, GEMM_MSG_PS2)            \
  X(38, GEMM_FAM_PS, 576, 256, true, false, GEMM_MSG_PS1)            \
  X(50, GEMM_FAM_V5, 128, 256, true, false, GEMM_MSG_V5)
#else
#define VFM_GEMM_CONFIGS(X) VFM_GEMM_CONFIGS_SHIPPED(X)
#endif

struct GemmConfig {
  int id, family, min_k, span;
  bool hosts_tail, deep_ring;
  int msg;
};
#define VFM_GEMM_ROW(id, family, min_k, span, hosts, deep, msg) {id, family, min_k, span, hosts, deep, msg},
constexpr GemmConfig kGemmConfigs[] = {VFM_GEMM_CONFIGS(VFM_GEMM_ROW)};
#undef VFM_GEMM_ROW
constexpr int kGemmConfigCount = (int)(sizeof(kGemmConfigs) / sizeof(kGemmConfigs[0]));
constexpr int gemm_config_index(int id) {   // row of the table, -1 if the id is not in it
  for (int i = 0; i < kGemmConfigCount; ++i)
    if (kGemmConfigs[i].id == id) return i;
  return -1;
}
constexpr bool gemm_config_retired(int id) { return id >= 0 && id <= 29 && gemm_config_index(id) < 0; }   // the round-1 sweep of the two-stage kernel
constexpr bool gemm_config_experimental(int id) { return id == 37 || id == 38 || id == 50; }

// ------------------------------------------------------------------------------------------------ plan
enum GemmKind { GEMM_SKINNY = 0, GEMM_BT64 = 1, GEMM_BT128 = 2, GEMM_ATBT = 3, GEMM_TILE = 4 };
enum GemmTail {
  GEMM_TAIL_NONE = 0,      // no tail rows
  GEMM_TAIL_BLOCKS = 1,    // extra skinny blocks of the same launch
  GEMM_TAIL_INSIDE = 2,    // rows inside the regular blocks (CLSIN)
  GEMM_TAIL_SEPARATE = 3,  // a skinny launch of their own behind the tile launch
  GEMM_TAIL_ROW_TILE = 4   // not peeled: one more row tile of the same launch (the 64-row shapes)
};
struct GemmPlan {
  int err = VFM_OK;            // VFM_E_*: nothing is launched, the other fields hold their defaults
  int msg = GEMM_MSG_NONE;     // index into kGemmMsgs
  int kind = GEMM_SKINNY;      // whole-skinny, transposed-B with BM 64 / 128, transposed-A+B, or a tile config
  int cfg = -1;                // GEMM_TILE: id of the config table
  int vec = 0;                 // the 16-byte vector epilogue (0: the scalar one)
  long tail_rows = 0;          // rows of M split off the tile launch (0 if none)
  int tail_mode = GEMM_TAIL_NONE;
};

// ------------------------------------------------------------------------------------------------ selector
inline int gemm_cdiv(long a, long b) { return (int)((a + b - 1) / b); }

inline bool gemm_vec_ok(const vfm_gemm_desc& d) {
  auto a16 = [](const void* p) { return ((uintptr_t)p % 16) == 0; };
  const long bm = d.bias_mod > 0 ? d.bias_mod : d.N;
  bool ok = (d.N % 4 == 0) && (d.ldc % 4 == 0) && a16(d.C) && (d.stride_c % 4 == 0);
  if (d.bias) ok = ok && a16(d.bias) && (bm % 4 == 0);
  if (d.colscale) ok = ok && a16(d.colscale);
  if (d.residual) ok = ok && a16(d.residual) && (d.ldr % 4 == 0);
  if (d.aux) ok = ok && a16(d.aux) && (d.ld_aux % 4 == 0);
  if (d.C2) ok = ok && a16(d.C2) && (d.ldc2 % 4 == 0);
  return ok;
}

// the split-K form of the 128 x 128 ring kernel: K % 128 == 0, K / 2 >= 128, one batch, at most GEMM_SPLITK_TILES tiles, the vector epilogue
constexpr int GEMM_SPLITK_TILES = 512;
inline bool gemm_splitk_ok(const vfm_gemm_desc& d, bool vec) {
  return vec && d.batch <= 1 && d.K % 128 == 0 && d.K >= 512 && (long)gemm_cdiv(d.M, 128) * gemm_cdiv(d.N, 128) <= GEMM_SPLITK_TILES;
}

// the persistent kernel (gemm_ps.hip): which epilogue instance serves this descriptor, or -1 (the caller then keeps the tile kernels)
enum { PS_BIAS = 0, PS_GELU_DGELU = 1, PS_MUL = 2, PS_GELU = 3 };   // epilogue kinds (all write bf16 C)
constexpr int PS_PEEL = 8;                            // slabs per wave tile = K-tiles the previous sub-tile's epilogue rides on
inline int gemm_ps_kind(const vfm_gemm_desc* d) {
  auto a16 = [](const void* p) { return ((uintptr_t)p % 16) == 0; };
  if (d->c_dt != VFM_BF16 || d->residual || d->colscale || !a16(d->C) || d->ldc % 8) return -1;
  const long bm = d->bias_mod > 0 ? d->bias_mod : d->N;
  if (d->bias && (!a16(d->bias) || bm % 4 || bm < d->N)) return -1;
  switch (d->ep_mode) {
    case VFM_EP_NONE: return (d->bias && !d->C2) ? PS_BIAS : -1;
    case VFM_EP_GELU: return (d->bias && !d->C2) ? PS_GELU : -1;
    case VFM_EP_GELU_DGELU: return (d->bias && d->C2 && d->c2_dt == VFM_BF16 && a16(d->C2) && d->ldc2 % 8 == 0) ? PS_GELU_DGELU : -1;
    case VFM_EP_MUL: return (!d->bias && !d->C2 && d->aux && d->aux_dt == VFM_BF16 && a16(d->aux) && d->ld_aux % 8 == 0) ? PS_MUL : -1;
    default: return -1;
  }
}
// per: sub-tiles of 256 x 128 per block (2: a 256 x 256 region).  Shapes: M % 256 == 0, N % (128 per) == 0, K % 64 == 0, K >= 64 * 8 + 64
// (the previous sub-tile's epilogue rides on the first eight K-tiles), operands contiguous in K, spans < 4 GiB, no batch.
inline bool gemm_ps_ok(const vfm_gemm_desc* d, int per) {
  if (!kGemmExperimental || gemm_ps_kind(d) < 0 || d->batch > 1 || per < 1 || per > 2) return false;
  if (d->sa_k != 1 || d->sb_k != 1 || d->M % 256 || d->N % (128 * per) || d->K % 64 || d->K < 64 * (PS_PEEL + 1)) return false;
  if ((d->M + 256) * d->sa_m >= (1l << 31) || (d->N + 256) * d->sb_n >= (1l << 31)) return false;
  if ((d->M + 8) * d->ldc >= (1l << 31) * 2 || (d->aux && (d->M + 8) * d->ld_aux >= (1l << 31))) return false;
  return ((uintptr_t)d->A % 16) == 0 && ((uintptr_t)d->B % 16) == 0 && d->sa_m % 8 == 0 && d->sb_n % 8 == 0;
}

inline bool gemm_span_ok(const vfm_gemm_desc& d, long span) {
  return (d.M + span) * d.sa_m < (1l << 31) && (d.N + span) * d.sb_n < (1l << 31);
}

inline GemmPlan gemm_plan_error(int err, int msg) {
  GemmPlan p;
  p.err = err, p.msg = msg;
  return p;
}

// The kernel of the [M, N] part `d` of a GEMM (all of it, or what is left once `tail_rows` rows were peeled off; has_tail: those rows
// may ride along with the tile launch).  Fills kind / cfg / vec / tail_mode.
inline GemmPlan gemm_select_main(const vfm_gemm_desc& d, const GemmKnobs& kn, long tail_rows, bool has_tail) {
  GemmPlan p;
  p.vec = gemm_vec_ok(d);
  p.tail_rows = tail_rows;
  if (d.sb_n == 1 && d.sb_k != 1) {  // B given as [K, N]: transposed-B kernels (BN = 128)
    if (d.sa_m == 1 && d.sa_k != 1) {  // ... and A given as [K, M]: C = A^T B, both operands consumed in place
      p.kind = GEMM_ATBT;
      return p;
    }
    // few 128-row tiles (decoder dgrads: 2048 x 256 outputs over K = 1024..2048): 64-row tiles double the blocks in flight
    const bool few = (long)gemm_cdiv(d.M, 128) * gemm_cdiv(d.N, 128) * (d.batch > 0 ? d.batch : 1) < 128;
    p.kind = (d.M <= 64 || (kn.bt64 && few)) ? GEMM_BT64 : GEMM_BT128;  // (a four-stage ring measured no faster: one wave per SIMD)
    return p;
  }
  const bool tail = has_tail;
  bool separate = tail_rows > 0 && !has_tail;
  int cfg = kn.force_cfg;
  if (cfg < 0) {
    // measured on MI355X (tools/bench_gemm.py): with ~one wave of tiles, occupancy (waves per SIMD) decides
    const long nbatch = d.batch > 0 ? d.batch : 1;  // batched launches (SAM's per-window products) fill the chip with their batch
    const long t128 = (long)gemm_cdiv(d.M, 128) * gemm_cdiv(d.N, 128) * (kn.batch_tiles ? nbatch : 1);
    const long t256 = (long)gemm_cdiv(d.M, 256) * gemm_cdiv(d.N, 256);
    const bool span31 = gemm_span_ok(d, 128);
    const bool span33 = gemm_span_ok(d, 256);
    // fill of the CUs' rounds by whole tiles (one block per CU for the 256-column forms)
    const long t192 = (long)gemm_cdiv(d.M, 192) * gemm_cdiv(d.N, 256);
    const double eff192 = (double)t192 / (256.0 * gemm_cdiv(t192, 256)), eff256 = (double)t256 / (256.0 * gemm_cdiv(t256, 256));
    const bool big_m = d.M >= 8192 && d.N >= 1024 && d.K >= 1024 && nbatch == 1 && span33 && !(kn.use_pp & 64);
    const long t64 = (long)gemm_cdiv(d.M, 64) * gemm_cdiv(d.N, 64);
    if (d.N <= 32) cfg = 10;                                        // 64x64 tiles: many rows, few columns
    else if ((kn.use_192 & 1) && big_m && eff192 >= eff256 + 0.08)
      cfg = 40;  // 192 x 256 tiles: [9216 x 1024 / 1280]: 192 / 240 tiles instead of 144 / 180; [9216 x 3840 / 4096]: 720 / 768 of 768 slots
    else if ((kn.use_192 & 2) && big_m && d.N >= 2048 && t256 > 256 && eff256 >= 0.8 && eff256 < 0.9)
      cfg = 33;  // [9216 x 3072]: 432 tiles of 256 x 256 = 84 % of two rounds (the 128 x 128 form: 1728 tiles, 3.4 rounds of 512 slots)
    else if ((kn.use_ps & 1) && d.N >= 2048 && t256 >= 224 && t256 % 256 == 0 && d.K >= 1024 && gemm_ps_ok(&d, 2))
      cfg = 37;  // whole rounds of 256 x 256 regions with a bf16 store-heavy epilogue (fc1 forward, fc2 input gradient [4096 x 4096 x 1024]):
                 // one persistent block per CU, the first half's epilogue under the second half's K loop
    else if (!(kn.use_pp & 64) && tail && t128 >= 96 && t128 <= 160 && d.N >= 512 && d.K >= 1024 && span31 && nbatch == 1)
      cfg = 31;  // half a wave of 128x128 tiles over a long K in a backbone GEMM (tail rows present: the coarse eval pass, 2049 tokens x
                 // 1024 columns): the ping-pong kernel beats the 64x64 tiles by 10-20 % (tools/scratch/_coarse_gemm.py: 15.9 / 36.3 us
                 // against 17.5 / 45.8 at K = 1024 / 4096).  The decoder's 2048-token GEMMs of the train step (no tail) keep the
                 // 64x64 tiles: 125.3 vs 124.9 images/s
    else if (!(kn.use_pp & 64) && d.N >= 1024 && d.N < 2048 && t256 >= 128 && t256 <= 200 && span33 && nbatch == 1 &&
             (d.K >= 2048 || (t256 >= 170 && d.K >= 1024)))
      cfg = 33;  // 130-200 tiles of 256x256 (eval: nine 1024-token windows at once - DINOv2 fc2 [9225 x 1024 x 4096] 104.5 -> 94.9 us,
                 // SAM-H proj / fc2 [9216 x 1280 x 1280 / 5120] 51.6 -> 46.9 / 142.5 -> 118.0 us): 576-720 tiles of 128x128 are 1.1-1.4
                 // rounds of the 512 resident slots
    else if (!(kn.use_pp & 64) && d.N >= 4096 && t256 >= 700 && t256 < 768 && d.K >= 1024 && span33 && nbatch == 1)
      cfg = 33;  // SAM-H fc1 over nine windows [9216 x 5120 x 1280]: 189.4 -> 160.5 us
    else if (!(kn.use_pp & 64) && d.N >= 2048 && t256 >= 224 && t256 <= 256 && d.K >= 1024 && span33 && nbatch == 1 && !tail)
      cfg = 33;  // one 256x256 tile on (almost) every CU - SAM-H qkv + LoRA in the train step [4096 x 3840 x 1344]: 866 -> 1016 TFLOP/s
    else if (t128 <= 160 && d.K >= 512 && t64 <= 544)
      cfg = 10;  // few tiles, long K (LoRA T GEMM 4096x64x1024, decoder projections): 64x64 tiles with the 4-stage ring
    else if (t128 <= 160) cfg = 18;                                  // small problems: 64x128 tiles fill more CUs
    else if ((kn.use_pp & 2) && t128 > 160 && t128 <= 272 && d.K >= 256 && span31)
      cfg = 31;  // about one 128x128 tile per CU: the ping-pong kernel (one block per CU, 4-slot DMA ring)
    else if ((kn.use_pp & 128) && d.N >= 2048 && t256 >= 176 && t256 < 256 && d.K >= 512 && span33 && nbatch == 1)
      cfg = 33;  // three quarters of a round of 256 x 256 tiles (qkv + LoRA forward [4096 x 3072 x 1088]: 192 tiles)
    else if ((kn.use_pp & 16) && d.N >= 2048 && (t256 % 256 == 0 || t256 >= 768) && d.K >= 128 && span33)
      cfg = 33;  // whole waves of 256x256 tiles: 8 waves, 64-wide K-tiles (whole-line LDS-DMA), 5-chunk ring
    else if (d.N >= 2048 && (t256 % 256 == 0 || t256 >= 768) && !(kn.use_pp & 8))
      cfg = ((kn.use_pp & 1) && d.K >= 128 && span33) ? 30 : 16;  // 256x256 tiles
    else cfg = 17;                                                   // 128x128, 8 waves, 2 blocks per CU
    if (cfg == 17 && (kn.use_pp & 32) && d.K >= 128 && span31)
      cfg = 34;  // same tile and wave layout, operands through the five-chunk (2.5 K-tile) LDS-DMA ring of gemm_w4.hip
    if (cfg == 34 && kn.w44_k > 0 && d.K >= kn.w44_k) cfg = 52;   // vfm_tune("gemm_w44_k"): the 4-wave form of the same tile from this K on (0 = never)
    // at most one tile per CU and no tail blocks to squeeze in: the second block's LDS buys a seven-chunk ring instead
    if (cfg == 34 && !tail && t128 <= 256 && d.K >= 256 && d.M % 128 == 0) cfg = 35;
    // ... and with tail blocks riding along when K is long: one tile per CU streams its operands latency-bound (bytes in flight /
    // latency), so the deeper ring wins more than the tail blocks lose by waiting for a CU (they cannot share the ring's LDS)
    if (cfg == 34 && tail && t128 <= 256 && d.M % 128 == 0 && d.K >= kn.deep_tail_k && kn.deep_tail_k > 0) cfg = 35;
    // ... or with the tail rows in a launch of their own behind this one (they cannot share a CU with the deep ring's LDS)
    if (cfg == 34 && tail && t128 <= 256 && d.M % 128 == 0 && d.K >= 256 && kn.deep_sep_k > 0 && d.K >= kn.deep_sep_k) cfg = 35, separate = true;
  }
  const int row = gemm_config_index(cfg);
  if (row < 0) {
    if (gemm_config_experimental(cfg)) return gemm_plan_error(VFM_E_UNSUPPORTED, GEMM_MSG_EXPERIMENT);
    if (gemm_config_retired(cfg)) return gemm_plan_error(VFM_E_UNSUPPORTED, GEMM_MSG_RETIRED);
    return gemm_plan_error(VFM_E_INVAL, GEMM_MSG_UNKNOWN);
  }
  const GemmConfig& c = kGemmConfigs[row];
  bool ok = d.K >= c.min_k && (c.span == 0 || (d.K % 64 == 0 && gemm_span_ok(d, c.span)));
  if (c.family == GEMM_FAM_SPLITK) ok = ok && gemm_splitk_ok(d, p.vec);
  if (c.family == GEMM_FAM_PS) ok = gemm_ps_ok(&d, cfg == 37 ? 2 : 1);
  if (!ok) return gemm_plan_error(VFM_E_UNSUPPORTED, c.msg);
  p.kind = GEMM_TILE, p.cfg = cfg;
  if (c.family == GEMM_FAM_SPLITK || c.family == GEMM_FAM_PS) p.vec = 1;   // (their checks ask for what the vector epilogue asks for)
  // where the tail rows go, from the config's properties
  if (tail_rows > 0) {
    if (separate || !c.hosts_tail) p.tail_mode = GEMM_TAIL_SEPARATE;
    else if (c.deep_ring && tail_rows <= 8 && d.sa_k == 1) p.tail_mode = GEMM_TAIL_INSIDE;
    else p.tail_mode = GEMM_TAIL_BLOCKS;
  }
  return p;
}

inline GemmPlan gemm_select(const vfm_gemm_desc& d0, const GemmKnobs& kn) {
  // A few rows past a 128-row boundary (M = B*1024 patch tokens + B [cls] tokens) would cost a whole extra row of
  // latency-bound tiles: peel them off into the skinny kernel.
  const long tail = d0.M % 128;
  const bool bt = (d0.sb_n == 1 && d0.sb_k != 1);
  if (bt) return gemm_select_main(d0, kn, 0, false);
  // shapes that go to the 64-row tiles (few column tiles, long K: the LoRA T GEMM [4100 x 64 x 1024]) take the tail as one
  // more row tile of the same launch - cheaper than a launch of its own
  // (a few tiles over the 512 resident slots still beat a second launch: the coarse 512 x 1024 inference pass, M = 2049, N = 1024,
  // has 33 x 16 tiles and paid 10 us per GEMM for its one [cls] row)
  // (... except where the ping-pong kernel with the tail folded in as skinny blocks is faster still: half a wave of 128 x 128 tiles,
  // N >= 512, K >= 1024 - the rule in gemm_select_main)
  const long t128m = (long)((d0.M - tail) / 128) * gemm_cdiv(d0.N, 128);
  const bool pp_coarse = !(kn.use_pp & 64) && tail > 0 && t128m >= 96 && t128m <= 160 && d0.N >= 512 && d0.K >= 1024 && d0.batch <= 1;
  const bool rows64 = !pp_coarse && d0.N > 32 && d0.K >= 512 && (long)gemm_cdiv(d0.M, 128) * gemm_cdiv(d0.N, 128) <= 160 &&
                      (long)gemm_cdiv(d0.M, 64) * gemm_cdiv(d0.N, 64) <= 544;
  const bool peelable = kn.split_tail && d0.M > 512 && tail > 0 && tail <= 32 && (d0.batch <= 1);
  if (peelable && !(rows64 && (kn.split_tail & 2))) {
    vfm_gemm_desc dm = d0;
    dm.M = d0.M - tail;
    return gemm_select_main(dm, kn, tail, kn.fold_tail != 0);
  }
  if (d0.M <= 32 && d0.N >= 32) return GemmPlan();   // whole-skinny
  GemmPlan p = gemm_select_main(d0, kn, 0, false);
  if (peelable && !p.err) p.tail_mode = GEMM_TAIL_ROW_TILE;
  return p;
}
