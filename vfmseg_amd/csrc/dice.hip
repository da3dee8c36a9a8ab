// Dice loss of the bilinearly up-sampled logits (mmseg 1.2.2 losses/dice_loss.py) without the [B,C,H,W] logits, their
// activation or either gradient in memory.  The loss of image n is a function of three sums over ALL of its pixels, so it takes two
// passes over the label map with a tiny finish between them:
//   1. k_dice_sums     every high-resolution pixel once: interpolated logits (the arithmetic of vision.hip k_upsample_ce), sigmoid or
//                      softmax in registers, the pixel's p.t, p^2 (naive: p), sum t and the accuracy counters; one row of sums per block
//   2. k_dice_finish   one block: the rows of every image in a fixed order, in double -> (alpha, beta, gamma) per image, loss, accuracy
//   3. k_dice_bwd      the gather of k_upsample_ce: the waves of a LOW-resolution pixel walk the high-resolution pixels whose footprint
//                      touches it, activate them again and add their share of d loss / d v (k_dice_bwd_tile: the x4 / x16 heads with 19
//                      classes, a block per tile of low-resolution pixels, every high-resolution pixel activated once per block)
// No floating-point atomics and no integer ones either: blocks never span two images and every sum has a fixed order.
#include "common.h"

#define DICE_CMAX 32  // = CE_CMAX of vision.hip

// the source index arithmetic of vision.hip lerp_idx (ATen area_pixel_compute_source_index, align_corners=False)
struct DLerp {
  int i0, i1;
  float l0, l1;
};
__device__ __forceinline__ DLerp dlerp_idx(int dst, float scale, int in_size) {
  float src = scale * (dst + 0.5f) - 0.5f;
  if (src < 0.f) src = 0.f;
  DLerp r;
  r.i0 = (int)src;
  if (r.i0 > in_size - 1) r.i0 = in_size - 1;
  r.i1 = r.i0 + (r.i0 < in_size - 1 ? 1 : 0);
  r.l1 = src - r.i0;
  r.l0 = 1.f - r.l1;
  return r;
}

// v[c] (c < C) -> p[c] in place: sigmoid, or softmax over the C classes.  Returns the arg-max of v (first maximum wins).
template <bool SIG>
__device__ __forceinline__ int dice_activate(float (&v)[DICE_CMAX], int C) {
  float m = -INFINITY;
  int am = 0;
#pragma unroll
  for (int c = 0; c < DICE_CMAX; ++c)
    if (c < C && v[c] > m) m = v[c], am = c;
  if constexpr (SIG) {
#pragma unroll
    for (int c = 0; c < DICE_CMAX; ++c)
      if (c < C) v[c] = 1.f / (1.f + __expf(-v[c]));
  } else {
    float se = 0.f;
#pragma unroll
    for (int c = 0; c < DICE_CMAX; ++c)
      if (c < C) v[c] = __expf(v[c] - m), se += v[c];
    const float inv = 1.f / se;
#pragma unroll
    for (int c = 0; c < DICE_CMAX; ++c)
      if (c < C) v[c] *= inv;
  }
  return am;
}

// the class whose row of t is one: clamp(label, 0, C), with C (and anything above, 255 included) meaning "none"
__device__ __forceinline__ int dice_class(int64_t lab, int C) { return lab < 0 ? 0 : (lab >= C ? C : (int)lab); }

template <bool SIG, bool NAIVE>
__global__ void __launch_bounds__(256) k_dice_sums(const float* __restrict__ lg, const int64_t* __restrict__ label, int h, int w, int C,
                                                    int H, int W, float sy, float sx, int drop, int ignore, int nblk,
                                                    float* __restrict__ fsum, int32_t* __restrict__ isum) {
  __shared__ float redf[2][4];
  __shared__ int redi[3][4];
  const long n = blockIdx.x / nblk;
  const int j = blockIdx.x % nblk;
  const long HW = (long)H * W;
  const float* lb = lg + n * (long)h * w * C;
  const int64_t* labn = label + n * HW;
  float a = 0.f, b = 0.f;
  int nt = 0, valid = 0, hits = 0;
  for (long i = (long)j * 256 + threadIdx.x; i < HW; i += (long)nblk * 256) {
    const int hy = (int)(i / W), hx = (int)(i % W);
    const int64_t lab = labn[i];
    const DLerp ly = dlerp_idx(hy, sy, h), lx = dlerp_idx(hx, sx, w);
    const float* r0 = lb + (long)ly.i0 * w * C;
    const float* r1 = lb + (long)ly.i1 * w * C;
    const float *p00 = r0 + (long)lx.i0 * C, *p01 = r0 + (long)lx.i1 * C, *p10 = r1 + (long)lx.i0 * C, *p11 = r1 + (long)lx.i1 * C;
    float v[DICE_CMAX];
#pragma unroll
    for (int c = 0; c < DICE_CMAX; ++c)
      v[c] = c < C ? ly.l0 * (lx.l0 * p00[c] + lx.l1 * p01[c]) + ly.l1 * (lx.l0 * p10[c] + lx.l1 * p11[c]) : -INFINITY;
    const int am = dice_activate<SIG>(v, C);
    const int cls = dice_class(lab, C);
    float pa = 0.f, pb = 0.f;
#pragma unroll
    for (int c = 0; c < DICE_CMAX; ++c) {
      if (c < C && c != drop) {
        pb += NAIVE ? v[c] : v[c] * v[c];
        if (c == cls) pa = v[c];
      }
    }
    a += pa, b += pb;
    nt += (cls < C && cls != drop) ? 1 : 0;
    if (lab != ignore) valid += 1, hits += (lab == (int64_t)am) ? 1 : 0;
  }
  a = wave_sum(a), b = wave_sum(b);
  for (int o = 32; o > 0; o >>= 1) {
    nt += __shfl_xor(nt, o, 64);
    valid += __shfl_xor(valid, o, 64);
    hits += __shfl_xor(hits, o, 64);
  }
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) redf[0][wv] = a, redf[1][wv] = b, redi[0][wv] = nt, redi[1][wv] = valid, redi[2][wv] = hits;
  __syncthreads();
  if (threadIdx.x < 2) fsum[(long)blockIdx.x * 2 + threadIdx.x] = (redf[threadIdx.x][0] + redf[threadIdx.x][1]) + (redf[threadIdx.x][2] + redf[threadIdx.x][3]);
  if (threadIdx.x < 3) isum[(long)blockIdx.x * 3 + threadIdx.x] = (redi[threadIdx.x][0] + redi[threadIdx.x][1]) + (redi[threadIdx.x][2] + redi[threadIdx.x][3]);
}

// One block.  Per image: thread t adds rows t, t + 256, ... in double, the 256 partials meet in an LDS tree; thread 0 closes the image.
__global__ void __launch_bounds__(256) k_dice_finish(const float* __restrict__ fsum, const int32_t* __restrict__ isum, int B, int nblk,
                                                      int naive, float eps, float acc_eps, float* __restrict__ coef,
                                                      float* __restrict__ sums, int32_t* __restrict__ counts, float* __restrict__ loss,
                                                      float* __restrict__ acc) {
  __shared__ double sd[2][256];
  __shared__ long long si[3][256];
  const int tid = threadIdx.x;
  double loss_sum = 0.0;
  long long hits_all = 0, valid_all = 0;
  for (int n = 0; n < B; ++n) {
    double a = 0.0, b = 0.0;
    long long nt = 0, valid = 0, hits = 0;
    for (int r = tid; r < nblk; r += 256) {
      const long row = (long)n * nblk + r;
      a += (double)fsum[row * 2], b += (double)fsum[row * 2 + 1];
      nt += isum[row * 3], valid += isum[row * 3 + 1], hits += isum[row * 3 + 2];
    }
    __syncthreads();  // the previous image's tree has been read
    sd[0][tid] = a, sd[1][tid] = b, si[0][tid] = nt, si[1][tid] = valid, si[2][tid] = hits;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) {
        sd[0][tid] += sd[0][tid + o], sd[1][tid] += sd[1][tid + o];
        si[0][tid] += si[0][tid + o], si[1][tid] += si[1][tid + o], si[2][tid] += si[2][tid + o];
      }
      __syncthreads();
    }
    if (tid == 0) {
      const double A = sd[0][0], Bs = sd[1][0], T = (double)si[0][0], e = (double)eps;
      double s, d, al, be, ga;
      if (naive) {
        s = Bs + T + e;
        d = (2.0 * A + e) / s;
        al = -2.0 / s, be = 0.0, ga = (2.0 * A + e) / (s * s);
      } else {
        s = (Bs + e) + (T + e);
        d = 2.0 * A / s;
        al = -2.0 / s, be = 4.0 * A / (s * s), ga = 0.0;
      }
      coef[n * 3 + 0] = (float)al, coef[n * 3 + 1] = (float)be, coef[n * 3 + 2] = (float)ga;
      if (sums) sums[n * 4 + 0] = (float)A, sums[n * 4 + 1] = (float)Bs, sums[n * 4 + 2] = (float)T, sums[n * 4 + 3] = (float)d;
      loss_sum += 1.0 - d;
      hits_all += si[2][0], valid_all += si[1][0];
    }
  }
  if (tid == 0) {
    loss[0] = (float)(loss_sum / (double)B);
    acc[0] = (float)hits_all * (100.0f / ((float)valid_all + acc_eps));  // the expression of k_ce_finish
    if (counts) counts[0] = (int32_t)hits_all, counts[1] = (int32_t)valid_all;
  }
}

// WPP = waves per low-resolution pixel, as in k_upsample_ce: 1 (small footprints, 4 pixels per block) or 4 (the block's four waves
// split one pixel's candidates and meet in LDS).  Every member pixel counts here, ignored ones too: they are part of the sums of p.
template <int WPP, bool SIG>
__global__ void __launch_bounds__(256) k_dice_bwd(const float* __restrict__ lg, const int64_t* __restrict__ label,
                                                   const float* __restrict__ coef, int B, int h, int w, int C, int H, int W, float sy,
                                                   float sx, int drop, float scale, int accumulate, float* __restrict__ dlogits) {
  __shared__ float red[4][DICE_CMAX];
  constexpr int PS = DICE_CMAX + 1;               // odd stride: the four corner vectors of a lane sit in different banks
  __shared__ float nb[WPP == 1 ? 4 : 1][9 * PS];  // the 3x3 low-res logit vectors a pixel's members interpolate from
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long pix_raw = WPP == 1 ? (long)blockIdx.x * 4 + wv : (long)blockIdx.x;
  const bool active = pix_raw < (long)B * h * w;  // tail waves of the WPP==1 form compute on the last pixel, write nothing
  const long pix = active ? pix_raw : (long)B * h * w - 1;
  const int x = (int)(pix % w);
  const long t = pix / w;
  const int y = (int)(t % h);
  const long b = t / h;
  const float al = coef[b * 3] * scale, be = coef[b * 3 + 1] * scale, ga = coef[b * 3 + 2] * scale;
  // conservative candidate window in the high-res grid
  int hy0 = (int)floorf((y - 1 + 0.5f) / sy - 0.5f) - 1, hy1 = (int)ceilf((y + 1 + 0.5f) / sy - 0.5f) + 1;
  int hx0 = (int)floorf((x - 1 + 0.5f) / sx - 0.5f) - 1, hx1 = (int)ceilf((x + 1 + 0.5f) / sx - 0.5f) + 1;
  if (y == 0) hy0 = 0;  // clamped sources
  if (x == 0) hx0 = 0;
  hy0 = max(hy0, 0), hx0 = max(hx0, 0), hy1 = min(hy1, H - 1), hx1 = min(hx1, W - 1);
  const int nx = hx1 - hx0 + 1, ny = hy1 - hy0 + 1;
  float acc[DICE_CMAX];
#pragma unroll
  for (int c = 0; c < DICE_CMAX; ++c) acc[c] = 0.f;
  const float* lb = lg + b * (long)h * w * C;
  float* Ls = nb[WPP == 1 ? wv : 0];
  for (int i = (WPP == 1 ? lane : (int)threadIdx.x); i < 9 * C; i += 64 * WPP) {
    const int c = i % C, p = i / C;
    const int yy = min(max(y - 1 + p / 3, 0), h - 1), xx = min(max(x - 1 + p % 3, 0), w - 1);
    Ls[p * PS + c] = lb[((long)yy * w + xx) * C + c];
  }
  __syncthreads();
  for (int i = (WPP == 1 ? lane : (int)threadIdx.x); i < nx * ny; i += 64 * WPP) {
    const int hy = hy0 + i / nx, hx = hx0 + i % nx;
    const DLerp ly = dlerp_idx(hy, sy, h), lx = dlerp_idx(hx, sx, w);
    const float wy = (ly.i0 == y ? ly.l0 : 0.f) + (ly.i1 == y ? ly.l1 : 0.f);
    const float wx = (lx.i0 == x ? lx.l0 : 0.f) + (lx.i1 == x ? lx.l1 : 0.f);
    const bool member = (ly.i0 == y || ly.i1 == y) && (lx.i0 == x || lx.i1 == x);
    if (!member) continue;
    const int cls = dice_class(label[(b * H + hy) * (long)W + hx], C);
    // members have i0 in {y-1, y} and i1 in {y, y+1}
    const float* p00 = Ls + ((ly.i0 - y + 1) * 3 + (lx.i0 - x + 1)) * PS;
    const float* p01 = Ls + ((ly.i0 - y + 1) * 3 + (lx.i1 - x + 1)) * PS;
    const float* p10 = Ls + ((ly.i1 - y + 1) * 3 + (lx.i0 - x + 1)) * PS;
    const float* p11 = Ls + ((ly.i1 - y + 1) * 3 + (lx.i1 - x + 1)) * PS;
    float v[DICE_CMAX];
#pragma unroll
    for (int c = 0; c < DICE_CMAX; ++c)
      v[c] = c < C ? ly.l0 * (lx.l0 * p00[c] + lx.l1 * p01[c]) + ly.l1 * (lx.l0 * p10[c] + lx.l1 * p11[c]) : -INFINITY;
    dice_activate<SIG>(v, C);
    const float g = wy * wx;
    if constexpr (SIG) {
#pragma unroll
      for (int c = 0; c < DICE_CMAX; ++c) {
        if (c < C && c != drop) {
          const float gp = (c == cls ? al : 0.f) + be * v[c] + ga;
          acc[c] += g * (gp * v[c] * (1.f - v[c]));
        }
      }
    } else {
      float dot = 0.f;  // sum_k p_k g_k over the kept channels
#pragma unroll
      for (int c = 0; c < DICE_CMAX; ++c)
        if (c < C && c != drop) dot += v[c] * ((c == cls ? al : 0.f) + be * v[c] + ga);
#pragma unroll
      for (int c = 0; c < DICE_CMAX; ++c) {
        if (c < C) {
          const float gp = c != drop ? (c == cls ? al : 0.f) + be * v[c] + ga : 0.f;
          acc[c] += g * (v[c] * (gp - dot));
        }
      }
    }
  }
  if constexpr (WPP == 1) {
#pragma unroll
    for (int c = 0; c < DICE_CMAX; ++c) {
      if (c < C) {
        const float s = wave_sum(acc[c]);
        if (lane == 0 && active) dlogits[pix * C + c] = accumulate ? dlogits[pix * C + c] + s : s;
      }
    }
  } else {
#pragma unroll
    for (int c = 0; c < DICE_CMAX; ++c) {
      if (c < C) {
        const float s = wave_sum(acc[c]);
        if (lane == 0) red[wv][c] = s;
      }
    }
    __syncthreads();
    if (threadIdx.x < C) {
      const float s = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
      dlogits[pix * C + threadIdx.x] = accumulate ? dlogits[pix * C + threadIdx.x] + s : s;
    }
  }
}

// Tiled gather for integer scale factors S and a compile-time class count (H = S*h, W = S*w: the x4 LinearHead / SegformerHead and the
// x16 VFMHead losses with 19 classes), after vision.hip k_upsample_ce_tile: a block owns T x T low-res pixels, i.e. a (T+1)S x (T+1)S
// high-res region walked in strips of RS rows.  Every high-res pixel of a strip is activated ONCE per block (operands from LDS) and leaves
// its d loss / d v in LDS (0 outside the image); the transpose of the up-sampling is then separable: a horizontal pass per strip and one
// vertical pass, each a sum of 2S terms in a fixed order.
template <int S, int T, int C, int RS, bool SIG>
__global__ void __launch_bounds__(256) k_dice_bwd_tile(const float* __restrict__ lg, const int64_t* __restrict__ label,
                                                        const float* __restrict__ coef, int B, int h, int w, int H, int W, int drop,
                                                        float scale, int accumulate, float* __restrict__ dlogits) {
  constexpr int R = (T + 1) * S, LT = T + 2, PS = C | 1;  // odd LDS stride: conflict-free per-pixel vectors
  constexpr int NSTRIP = R / RS, PPT = (RS * R + 255) / 256;
  static_assert(R % RS == 0, "strips tile the region");
  static_assert(C <= DICE_CMAX, "class count");
  __shared__ float Ls[LT * LT * PS];  // low-res logits
  __shared__ float Ds[RS * R * PS];   // d loss / d v per high-res pixel of the strip
  __shared__ float Hs[R * T * PS];    // horizontal pass
  __shared__ float Wy[T][2 * S], Wx[T][2 * S];
  const int tid = threadIdx.x;
  const int tiles_x = w / T, tiles_y = h / T;
  const int bx = blockIdx.x % tiles_x, by = (blockIdx.x / tiles_x) % tiles_y;
  const long b = blockIdx.x / (tiles_x * tiles_y);
  const int y0 = by * T, x0 = bx * T;
  const float sc = 1.0f / S;
  const int hy_base = S * y0 - S / 2, hx_base = S * x0 - S / 2;
  const float* lb = lg + b * (long)h * w * C;
  const float al = coef[b * 3] * scale, be = coef[b * 3 + 1] * scale, ga = coef[b * 3 + 2] * scale;
  int labs[NSTRIP * PPT];  // the pixel's class in [0, C] (C: none), -1: outside the image / no pixel
#pragma unroll
  for (int k = 0; k < NSTRIP * PPT; ++k) {
    const int i = tid + (k % PPT) * 256;
    const int hy = hy_base + (k / PPT) * RS + i / R, hx = hx_base + i % R;
    int lab = -1;
    if (i < RS * R && hy >= 0 && hy < H && hx >= 0 && hx < W) lab = dice_class(label[(b * H + hy) * (long)W + hx], C);
    labs[k] = lab;
  }
  for (int i = tid; i < LT * LT * C; i += 256) {
    const int c = i % C, p = i / C;
    const int yy = min(max(y0 - 1 + p / LT, 0), h - 1), xx = min(max(x0 - 1 + p % LT, 0), w - 1);
    Ls[p * PS + c] = lb[((long)yy * w + xx) * C + c];
  }
  for (int i = tid; i < 2 * T * 2 * S; i += 256) {  // the share of owned row / column t in member d (0 outside the image)
    const int d = i % (2 * S), t = (i / (2 * S)) % T, isx = i / (2 * S * T);
    const int hp = (isx ? hx_base : hy_base) + t * S + d, own = (isx ? x0 : y0) + t, lim = isx ? W : H;
    float wgt = 0.f;
    if (hp >= 0 && hp < lim) {
      const DLerp l = dlerp_idx(hp, sc, isx ? w : h);
      wgt = (l.i0 == own ? l.l0 : 0.f) + (l.i1 == own ? l.l1 : 0.f);
    }
    if (isx) Wx[t][d] = wgt;
    else Wy[t][d] = wgt;
  }
#pragma unroll
  for (int st = 0; st < NSTRIP; ++st) {
    __syncthreads();  // Ls / weights ready (st == 0); previous strip's horizontal pass done with Ds
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
      const int i = tid + j * 256;
      if (i >= RS * R) break;
      const int cls = labs[st * PPT + j];
      float v[C];
      if (cls >= 0) {
        const int hy = hy_base + st * RS + i / R, hx = hx_base + i % R;
        const DLerp ly = dlerp_idx(hy, sc, h), lx = dlerp_idx(hx, sc, w);
        const float* p00 = Ls + ((ly.i0 - y0 + 1) * LT + (lx.i0 - x0 + 1)) * PS;
        const float* p01 = Ls + ((ly.i0 - y0 + 1) * LT + (lx.i1 - x0 + 1)) * PS;
        const float* p10 = Ls + ((ly.i1 - y0 + 1) * LT + (lx.i0 - x0 + 1)) * PS;
        const float* p11 = Ls + ((ly.i1 - y0 + 1) * LT + (lx.i1 - x0 + 1)) * PS;
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = ly.l0 * (lx.l0 * p00[c] + lx.l1 * p01[c]) + ly.l1 * (lx.l0 * p10[c] + lx.l1 * p11[c]);
        if constexpr (SIG) {
#pragma unroll
          for (int c = 0; c < C; ++c) {
            const float p = 1.f / (1.f + __expf(-v[c]));
            const float gp = c != drop ? (c == cls ? al : 0.f) + be * p + ga : 0.f;
            v[c] = gp * p * (1.f - p);
          }
        } else {
          float m = -INFINITY, se = 0.f, dot = 0.f;
#pragma unroll
          for (int c = 0; c < C; ++c) m = fmaxf(m, v[c]);
#pragma unroll
          for (int c = 0; c < C; ++c) v[c] = __expf(v[c] - m), se += v[c];
          const float inv = 1.f / se;
#pragma unroll
          for (int c = 0; c < C; ++c) {
            v[c] *= inv;
            if (c != drop) dot += v[c] * ((c == cls ? al : 0.f) + be * v[c] + ga);
          }
#pragma unroll
          for (int c = 0; c < C; ++c) {
            const float gp = c != drop ? (c == cls ? al : 0.f) + be * v[c] + ga : 0.f;
            v[c] = v[c] * (gp - dot);
          }
        }
      }
#pragma unroll
      for (int c = 0; c < C; ++c) Ds[i * PS + c] = cls >= 0 ? v[c] : 0.f;
    }
    __syncthreads();
    for (int task = tid; task < RS * T * C; task += 256) {
      const int c = task % C, tx = (task / C) % T, ry = task / (C * T);
      const float* dp = Ds + (ry * R + tx * S) * PS + c;
      float acc = 0.f;
#pragma unroll
      for (int dx = 0; dx < 2 * S; ++dx) acc += Wx[tx][dx] * dp[dx * PS];
      Hs[((st * RS + ry) * T + tx) * PS + c] = acc;
    }
  }
  __syncthreads();
  for (int task = tid; task < T * T * C; task += 256) {
    const int c = task % C, tx = (task / C) % T, ty = task / (C * T);
    const float* hp = Hs + (ty * S * T + tx) * PS + c;
    float g = 0.f;
#pragma unroll
    for (int dy = 0; dy < 2 * S; ++dy) g += Wy[ty][dy] * hp[dy * T * PS];
    float* out = dlogits + ((b * h + y0 + ty) * (long)w + x0 + tx) * C + c;
    *out = accumulate ? *out + g : g;
  }
}

static int dice_shape_ok(const char* who, int B, int h, int w, int C, int H, int W) {
  VFM_CHECK(C > 0 && C <= DICE_CMAX, VFM_E_SHAPE, "%s: C=%d > %d", who, C, DICE_CMAX);
  VFM_CHECK(B > 0 && h > 0 && w > 0, VFM_E_SHAPE, "%s: empty map", who);
  VFM_CHECK(H >= h && W >= w, VFM_E_SHAPE, "%s: only up-sampling is supported", who);
  VFM_CHECK((long)H * W < (1L << 31), VFM_E_SHAPE, "%s: %ld pixels per image overflow the int32 counters", who, (long)H * W);
  return VFM_OK;
}

extern "C" int vfm_upsample_dice_sums(const float* logits_low, const int64_t* label, int B, int h, int w, int C, int H, int W,
                                      int use_sigmoid, int naive, int drop_class, int ignore_label, int nblk, float* fsum, int32_t* isum,
                                      void* stream) {
  const int rc = dice_shape_ok("vfm_upsample_dice_sums", B, h, w, C, H, W);
  if (rc != VFM_OK) return rc;
  VFM_CHECK(logits_low && label && fsum && isum, VFM_E_INVAL, "vfm_upsample_dice_sums: null pointer");
  VFM_CHECK(nblk >= 1 && (long)B * nblk < (1L << 31), VFM_E_INVAL, "vfm_upsample_dice_sums: nblk=%d", nblk);
  VFM_CHECK(drop_class >= -1 && drop_class < C, VFM_E_INVAL, "vfm_upsample_dice_sums: drop_class=%d is no class of %d", drop_class, C);
  const dim3 grid((unsigned)(B * nblk)), block(256);
  const float sy = (float)h / (float)H, sx = (float)w / (float)W;
  hipStream_t s = (hipStream_t)stream;
#define DICE_SUMS(SIG, NAIVE) \
  hipLaunchKernelGGL((k_dice_sums<SIG, NAIVE>), grid, block, 0, s, logits_low, label, h, w, C, H, W, sy, sx, drop_class, ignore_label, nblk, fsum, isum)
  if (use_sigmoid) {
    if (naive) DICE_SUMS(true, true);
    else DICE_SUMS(true, false);
  } else {
    if (naive) DICE_SUMS(false, true);
    else DICE_SUMS(false, false);
  }
#undef DICE_SUMS
  VFM_LAUNCH_CHECK();
  return VFM_OK;
}

extern "C" int vfm_dice_finish(const float* fsum, const int32_t* isum, int B, int nblk, int naive, float eps, float acc_eps, float* coef,
                               float* sums, int32_t* counts, float* loss, float* acc, void* stream) {
  VFM_CHECK(fsum && isum && coef && loss && acc, VFM_E_INVAL, "vfm_dice_finish: null pointer");
  VFM_CHECK(B > 0 && nblk >= 1, VFM_E_INVAL, "vfm_dice_finish: B=%d nblk=%d", B, nblk);
  hipLaunchKernelGGL(k_dice_finish, dim3(1), dim3(256), 0, (hipStream_t)stream, fsum, isum, B, nblk, naive, eps, acc_eps, coef, sums, counts,
                     loss, acc);
  VFM_LAUNCH_CHECK();
  return VFM_OK;
}

extern "C" int vfm_upsample_dice_bwd(const float* logits_low, const int64_t* label, const float* coef, int B, int h, int w, int C, int H,
                                     int W, int use_sigmoid, int drop_class, float scale, int accumulate, float* dlogits, void* stream) {
  const int rc = dice_shape_ok("vfm_upsample_dice_bwd", B, h, w, C, H, W);
  if (rc != VFM_OK) return rc;
  VFM_CHECK(logits_low && label && coef && dlogits, VFM_E_INVAL, "vfm_upsample_dice_bwd: null pointer");
  VFM_CHECK(drop_class >= -1 && drop_class < C, VFM_E_INVAL, "vfm_upsample_dice_bwd: drop_class=%d is no class of %d", drop_class, C);
  const long npix = (long)B * h * w;
  VFM_CHECK(npix < (1L << 31), VFM_E_SHAPE, "vfm_upsample_dice_bwd: %ld low-resolution pixels", npix);
  const bool big = ((long)H * W) >= 64L * h * w;  // footprint (2*scale)^2 >= 256 candidates per low-res pixel
  const float sy = (float)h / (float)H, sx = (float)w / (float)W;
  hipStream_t s = (hipStream_t)stream;
#define DICE_BWD(WPP, SIG, GRID) \
  hipLaunchKernelGGL((k_dice_bwd<WPP, SIG>), dim3((unsigned)(GRID)), dim3(256), 0, s, logits_low, label, coef, B, h, w, C, H, W, sy, sx, drop_class, scale, accumulate, dlogits)
#define DICE_BWD_TILE(S, T, RS, SIG, GRID) \
  hipLaunchKernelGGL((k_dice_bwd_tile<S, T, 19, RS, SIG>), dim3((unsigned)(GRID)), dim3(256), 0, s, logits_low, label, coef, B, h, w, H, W, drop_class, scale, accumulate, dlogits)
  if (H == 4 * h && W == 4 * w && h % 4 == 0 && w % 4 == 0 && C == 19) {  // the geometries of k_upsample_ce_tile
    if (use_sigmoid) DICE_BWD_TILE(4, 4, 20, true, B * (h / 4) * (w / 4));
    else DICE_BWD_TILE(4, 4, 20, false, B * (h / 4) * (w / 4));
  } else if (H == 16 * h && W == 16 * w && C == 19) {
    if (use_sigmoid) DICE_BWD_TILE(16, 1, 8, true, npix);
    else DICE_BWD_TILE(16, 1, 8, false, npix);
  } else if (big) {
    if (use_sigmoid) DICE_BWD(4, true, npix);
    else DICE_BWD(4, false, npix);
  } else {
    if (use_sigmoid) DICE_BWD(1, true, cdiv(npix, 4));
    else DICE_BWD(1, false, cdiv(npix, 4));
  }
#undef DICE_BWD
#undef DICE_BWD_TILE
  VFM_LAUNCH_CHECK();
  return VFM_OK;
}
