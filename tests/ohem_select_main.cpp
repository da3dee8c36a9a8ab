// Host program around vfmseg_amd/csrc/ohem_select.h (no HIP in it): runs the three-round histogram selection of the OHEM sampler the way
// the kernels of ohem.hip do - counters and first histogram, then pick / histogram / pick / histogram / pick over one int32 state - and
// compares t = max(k-th smallest valid value, thresh) with std::sort, bit for bit.  tests/test_loss_options_cpu.py compiles it with
// g++ -fsanitize=undefined,address and expects "ok <cases>" and exit status 0.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "ohem_select.h"

static uint32_t bits_of(float v) {
  uint32_t b;
  std::memcpy(&b, &v, 4);
  return b;
}
static float float_of(uint32_t b) {
  float v;
  std::memcpy(&v, &b, 4);
  return v;
}

// the kernel's two-level walk: 256 chunk sums, then the chunk
static void pick_two_level(const int32_t* hist, int nbins, int rank, int* bin, int* residual) {
  const int per = nbins / 256;
  int32_t chunk[256];
  for (int t = 0; t < 256; ++t) {
    chunk[t] = 0;
    for (int j = 0; j < per; ++j) chunk[t] += hist[t * per + j];
  }
  int c, r, b;
  ohem_pick_bin(chunk, 256, rank, &c, &r);
  ohem_pick_bin(hist + c * per, per, r, &b, residual);
  *bin = c * per + b;
}

struct Result {
  float t;
  int n, n_lt, k;
};

static Result select_hist(const std::vector<float>& p, long k_request, float thresh) {
  std::vector<int32_t> state(OHEM_S_INTS, 0);
  for (float v : p) {  // k_ohem_prob
    const uint32_t b = bits_of(v);
    if (!ohem_is_key(b)) continue;
    state[OHEM_S_N] += 1;
    state[OHEM_S_NLT] += v < thresh ? 1 : 0;
    state[OHEM_S_HIST0 + ohem_digit(b, 0)] += 1;
  }
  const int n = state[OHEM_S_N], n_lt = state[OHEM_S_NLT];
  const int k = n > 0 ? ohem_clamp_rank(k_request, n) : 0;
  state[OHEM_S_K] = k;
  if (ohem_thresh_decides(n, n_lt, k)) return {thresh, n, n_lt, k};
  state[OHEM_S_RANK] = k;
  for (int round = 0; round < OHEM_ROUNDS; ++round) {
    int32_t* hist = state.data() + (round == 1 ? OHEM_S_HIST1 : OHEM_S_HIST0);
    const uint32_t prefix = (uint32_t)state[OHEM_S_PREFIX];
    if (round > 0) {  // k_ohem_hist<round>
      for (float v : p) {
        const uint32_t b = bits_of(v);
        if (ohem_is_key(b) && ohem_prefix_match(b, prefix, round)) hist[ohem_digit(b, round)] += 1;
      }
    }
    int bin, res, bin2, res2;  // k_ohem_pick<round>
    ohem_pick_bin(hist, ohem_bins(round), state[OHEM_S_RANK], &bin, &res);
    pick_two_level(hist, ohem_bins(round), state[OHEM_S_RANK], &bin2, &res2);
    if (bin != bin2 || res != res2) {
      std::printf("two-level pick differs: round %d bin %d/%d residual %d/%d\n", round, bin, bin2, res, res2);
      return {-2.f, n, n_lt, k};
    }
    state[OHEM_S_PREFIX] = (int32_t)ohem_extend_prefix(round == 0 ? 0u : prefix, round, bin);
    state[OHEM_S_RANK] = res;
    int32_t* next = state.data() + (round == 0 ? OHEM_S_HIST1 : OHEM_S_HIST0);
    if (round < 2) std::fill(next, next + OHEM_BINS1, 0);
  }
  const float v = float_of((uint32_t)state[OHEM_S_PREFIX]);
  return {v > thresh ? v : thresh, n, n_lt, k};
}

static Result select_sort(const std::vector<float>& p, long k_request, float thresh) {
  std::vector<float> s;
  for (float v : p)
    if (!(bits_of(v) >> 31)) s.push_back(v);
  std::sort(s.begin(), s.end());
  const int n = (int)s.size();
  int n_lt = 0;
  for (float v : s) n_lt += v < thresh ? 1 : 0;
  if (n == 0) return {thresh, 0, 0, 0};
  const long k = std::min<long>(k_request, n - 1);
  return {std::max(s[(size_t)k], thresh), n, n_lt, (int)k};
}

static int g_cases = 0, g_bad = 0;

static void check(const char* name, const std::vector<float>& p, long k_request, float thresh) {
  const Result a = select_hist(p, k_request, thresh), b = select_sort(p, k_request, thresh);
  ++g_cases;
  if (bits_of(a.t) != bits_of(b.t) || a.n != b.n || a.n_lt != b.n_lt || a.k != b.k) {
    ++g_bad;
    std::printf("MISMATCH %s k_request=%ld thresh=%g: t %.9g (bits %08x) vs sort %.9g (bits %08x), n %d/%d, n_lt %d/%d, k %d/%d\n", name,
                k_request, thresh, a.t, bits_of(a.t), b.t, bits_of(b.t), a.n, b.n, a.n_lt, b.n_lt, a.k, b.k);
  }
}

static void sweep(const char* name, const std::vector<float>& p) {
  const long n = (long)p.size();
  const long ks[] = {0, 1, n / 3, n / 2, n - 2 < 0 ? 0 : n - 2, n - 1 < 0 ? 0 : n - 1, n, n + 7, 1L << 40};
  const float ths[] = {0.f, 1e-30f, 0.05f, 0.5f, 0.7f, 1.f, 2.f};
  for (long k : ks)
    for (float th : ths) check(name, p, k, th);
}

int main() {
  std::mt19937 rng(1234);
  std::uniform_real_distribution<float> uni(0.f, 1.f);
  {  // random values in [0, 1], with and without sentinels
    std::vector<float> p(5000), q;
    for (float& v : p) v = uni(rng);
    p[17] = 0.f, p[18] = 1.f;
    sweep("uniform", p);
    q = p;
    for (size_t i = 0; i < q.size(); i += 3) q[i] = OHEM_SENTINEL;
    sweep("uniform+sentinels", q);
  }
  {  // saturated: nearly everything rounds near 1
    std::vector<float> p(4000);
    for (float& v : p) v = 1.f - 1e-6f * uni(rng);
    for (int i = 0; i < 40; ++i) p[(size_t)i * 97] = uni(rng);
    sweep("saturated", p);
  }
  sweep("all-equal", std::vector<float>(777, 0.25f));
  {
    std::vector<float> p(1000, 0.125f);
    for (size_t i = 0; i < p.size(); i += 2) p[i] = 0.875f;
    sweep("two-values", p);
  }
  {  // denormals and zeros
    std::vector<float> p;
    for (uint32_t b = 0; b < 600; ++b) p.push_back(float_of(b % 7 == 0 ? 0u : b * 13u));
    p.push_back(float_of(0x007fffffu));
    p.push_back(float_of(0x00800000u));
    std::shuffle(p.begin(), p.end(), rng);
    sweep("denormals", p);
  }
  {  // duplicates on both sides of the bin edges of every round
    std::vector<float> p;
    const uint32_t edges[] = {0x3f100000u, 0x3f000000u, 0x3f100400u, 0x3f1ffc00u, 0x3f100401u, 0x3f800000u};
    for (uint32_t e : edges)
      for (int r = 0; r < 9; ++r) p.push_back(float_of(e)), p.push_back(float_of(e - 1u));
    std::shuffle(p.begin(), p.end(), rng);
    sweep("bin-edges", p);
    for (long k = 0; k < (long)p.size() + 2; ++k) check("bin-edges-every-k", p, k, 0.f);
  }
  sweep("one", std::vector<float>(1, 0.3f));
  sweep("empty", std::vector<float>());
  sweep("only-sentinels", std::vector<float>(50, OHEM_SENTINEL));
  std::printf("%s %d\n", g_bad ? "FAILED" : "ok", g_cases);
  return g_bad ? 1 : 0;
}
