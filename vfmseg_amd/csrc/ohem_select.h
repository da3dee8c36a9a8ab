// The selection arithmetic of the OHEM pixel sampler (ohem.hip) as pure functions: no HIP in here, so the same code runs inside the
// kernels and in a host program (tests/ohem_select_main.cpp compiles it with plain g++ under the sanitizers).
//
// p = softmax(logits)[label] is a non-negative IEEE float, and non-negative floats order like their bit patterns.  The k-th smallest of
// the valid p is therefore the k-th smallest 31-bit key, found exactly by three rounds of integer histograms over 11 / 10 / 10 bits,
// most significant first: each round walks its histogram to the bin that holds the wanted rank, keeps the bin as the next piece of the
// key's prefix and the rank inside the bin as the next round's rank.  Ignored pixels carry a negative sentinel (sign bit set), which no
// round counts.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define OHEM_HD __host__ __device__ inline
#else
#define OHEM_HD inline
#endif

#define OHEM_ROUNDS 3
#define OHEM_BINS0 2048  // round 0: bits 30..20
#define OHEM_BINS1 1024  // rounds 1 and 2: bits 19..10 and 9..0
#define OHEM_SENTINEL (-1.0f)

// layout of the int32 device state of one selection (vfm_ohem_prob zero-initialised it; include/vfmseg_hip.h VFM_OHEM_STATE_INTS)
enum {
  OHEM_S_N = 0,       // valid pixels
  OHEM_S_NLT = 1,     // valid pixels with p < thresh
  OHEM_S_K = 2,       // the clamped rank k = min(k_request, n - 1)
  OHEM_S_PREFIX = 3,  // key bits fixed so far
  OHEM_S_RANK = 4,    // rank inside the bins that share the prefix
  OHEM_S_DONE = 5,    // t is final (n == 0, or the k-th value lies below thresh): the later rounds exit
  OHEM_S_T = 6,       // the threshold t (float bits)
  OHEM_S_HIST0 = 8,                         // rounds 0 and 2
  OHEM_S_HIST1 = OHEM_S_HIST0 + OHEM_BINS0, // round 1
  OHEM_S_INTS = OHEM_S_HIST1 + OHEM_BINS1
};

OHEM_HD int ohem_bins(int round) { return round == 0 ? OHEM_BINS0 : OHEM_BINS1; }

// is `bits` the pattern of a value that takes part (sign bit clear)?
OHEM_HD bool ohem_is_key(uint32_t bits) { return (bits >> 31) == 0; }

// float bits -> digit of round r
OHEM_HD int ohem_digit(uint32_t bits, int round) {
  return round == 0 ? (int)((bits >> 20) & 0x7ffu) : (round == 1 ? (int)((bits >> 10) & 0x3ffu) : (int)(bits & 0x3ffu));
}

// does `bits` lie in the bins picked by the rounds before `round`?  prefix = the digits of those rounds, most significant first
OHEM_HD bool ohem_prefix_match(uint32_t bits, uint32_t prefix, int round) {
  return round == 0 ? true : (round == 1 ? (bits >> 20) == prefix : (bits >> 10) == prefix);
}

OHEM_HD uint32_t ohem_extend_prefix(uint32_t prefix, int round, int bin) {
  return round == 0 ? (uint32_t)bin : ((prefix << 10) | (uint32_t)bin);
}

// k = min(k_request, n - 1) for n > 0 (mmseg: min_kept * batch clamped to the last valid pixel)
OHEM_HD int ohem_clamp_rank(long k_request, int n) {
  const long last = (long)n - 1;
  const long k = k_request < last ? k_request : last;
  return (int)(k < 0 ? 0 : k);
}

// t = thresh without a selection: nothing valid, or more than k values lie below thresh (then s[k] < thresh and max(s[k], thresh) = thresh)
OHEM_HD bool ohem_thresh_decides(int n, int n_lt, int k) { return n == 0 || n_lt > k; }

// (histogram, rank) -> bin, residual rank: the first bin whose running count exceeds `rank`; residual = rank minus the count before it.
// A rank beyond the histogram's total (it cannot happen when the counters agree) lands in the last non-empty bin with its last element.
OHEM_HD void ohem_pick_bin(const int32_t* hist, int nbins, int rank, int* bin, int* residual) {
  int before = 0, last = -1, last_before = 0;
  for (int i = 0; i < nbins; ++i) {
    const int c = hist[i];
    if (c <= 0) continue;
    if (rank < before + c) {
      *bin = i;
      *residual = rank - before;
      return;
    }
    last = i, last_before = before;
    before += c;
  }
  if (last < 0) {
    *bin = 0;
    *residual = 0;
  } else {
    *bin = last;
    *residual = before - last_before - 1;
  }
}
