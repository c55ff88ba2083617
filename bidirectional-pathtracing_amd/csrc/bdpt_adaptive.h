// bdpt_adaptive.h — adaptive sampling under BDPT: the frame is rendered in rounds of m
// samples over a shrinking list of 8x8 pixel blocks; after each round the per-pixel eye and light
// records are updated, every block's variance is tested against its mean and the blocks that pass
// leave the list. BDPT_HD: k_adapt_moments, k_adapt_decide, k_adapt_compact and k_adapt_resolve
// (bdpt_adaptive.hip) and the host build (tests/native/core_cpu_adaptive.cpp) run the same code. Only
// + - x / and max on fp32, in the order written here, so the two builds agree bit for bit.

#pragma once

#include "bdpt_variance.h"

namespace bdpt {

// bdpt_adaptive_params' defaults: the reference's -a BATCH TOL defaults (application.h) and 4 rounds
// before the first decision.
constexpr int kAdaptSamplesPerRound = 32;
constexpr int kAdaptMinRounds = 4;
constexpr float kAdaptTolerance = 0.05f;
constexpr float kAdaptZ2 = 3.8416f;   // 1.96^2
constexpr int kAdaptBlock = 8;        // the megakernel's work item: 8x8 pixels, one wave

// The light record's update: moments_add on the light frame with the round's increment weighted by
// w = fl(1 / M_r), M_r the pixel-samples (= light subpaths) of the round.
BDPT_HD float4 moments_add_weighted(float4 rec, f3 f, float w) {
  const f3 b = sub(f, mk3(rec.x, rec.y, rec.z));
  float4 r;
  r.x = f.x; r.y = f.y; r.z = f.z;
  r.w = rec.w + ((b.x * b.x + b.y * b.y) + b.z * b.z) * w;
  return r;
}

// The scalars of a decision or a resolve after R rounds with N pixel-samples in all, computed on the
// host in double and rounded to fp32 once: g = S W H / N, vl = g^2 N / (R - 1), inv_n = 1 / N.
struct AdaptScal {
  float g, vl, inv_n;
};
inline AdaptScal adapt_scal(int W, int H, int S, int R, long long N) {
  AdaptScal s;
  const double g = (double)S * (double)W * (double)H / (double)N;
  s.g = (float)g;
  s.vl = R > 1 ? (float)(g * g * (double)N / (double)(R - 1)) : 0.0f;
  s.inv_n = (float)(1.0 / (double)N);
  return s;
}

// The factors of a block that was active for K rounds of m samples, in plain fp32 (K m and S are
// exact in fp32 below 2^24): a = S / (K m), inv_k = 1 / K, ve = a^2 K / (K - 1). K < 2 has no eye
// variance (ve = 0) and K == 0 no eye estimate (a = 0); a render never leaves such a block, the
// buffer entry points may be handed one.
struct AdaptBlockF {
  float a, ve, inv_k;
};
BDPT_HD AdaptBlockF adapt_block(int K, int S, int m) {
  AdaptBlockF f;
  const float kf = (float)K;
  f.a = K > 0 ? (float)S / (kf * (float)m) : 0.0f;
  f.inv_k = K > 0 ? 1.0f / kf : 0.0f;
  f.ve = K > 1 ? (f.a * f.a) * (kf / (kf - 1.0f)) : 0.0f;
  return f;
}

// A pixel's estimate from its two records (after a round's moments pass prev is the frame itself):
// c = fl(fl(a E) + fl(g L)), v = vE + vL with
//   vE = ve max(0, Q_E - |E|^2 inv_k),   vL = vl max(0, Q_L - |L|^2 inv_n).
struct AdaptPix {
  f3 c;
  float v;
};
BDPT_HD AdaptPix adapt_pixel(float4 re, float4 rl, AdaptBlockF bf, AdaptScal sc) {
  AdaptPix p;
  p.c = add(smul(bf.a, mk3(re.x, re.y, re.z)), smul(sc.g, mk3(rl.x, rl.y, rl.z)));
  const float se = (re.x * re.x + re.y * re.y) + re.z * re.z;
  const float sl = (rl.x * rl.x + rl.y * rl.y) + rl.z * rl.z;
  const float ve = bf.ve * fmaxf(0.0f, re.w - se * bf.inv_k);
  const float vl = sc.vl * fmaxf(0.0f, rl.w - sl * sc.inv_n);
  p.v = ve + vl;
  return p;
}

// A lane's addend of the block's second sum.
BDPT_HD float adapt_csum(f3 c) { return (c.x + c.y) + c.z; }

// The stopping rule on the block's sums over its n in-frame pixels: 1.96 e_b <= tol mu_b with
// e_b^2 = Sv / (3 n) and mu_b = Sc / (3 n), multiplied out. Sv and Sc are the xor-butterfly sums
// over the block's 64 lanes (lane = x + 8 y, out-of-frame lanes add +0): strides 32, 16, 8, 4, 2, 1,
// s = s + s[lane ^ stride] at each.
BDPT_HD bool adapt_stop(float Sv, float Sc, int n, float tol) {
  const float t = tol * Sc;
  return (kAdaptZ2 * Sv) * (float)(3 * n) <= t * t;
}

}  // namespace bdpt
