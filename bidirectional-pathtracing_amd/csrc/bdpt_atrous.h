// bdpt_atrous.h — the edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) over a frame,
// guided by the first-hit features of bdpt_features.h. BDPT_HD: k_atrous
// (bdpt_denoise.hip) and the host build (tests/native/core_cpu_denoise.cpp) run the same code.

#pragma once

#include "bdpt_math.h"

namespace bdpt {

// bdpt_denoise_params' defaults, chosen by the sweep of DESIGN.md §11
constexpr int kDenoiseLevels = 2;
constexpr float kDenoiseSigmaColor = 1.5f, kDenoiseSigmaNormal = 0.3f, kDenoiseSigmaDepth = 0.03f;
constexpr int kDenoiseDemodulate = 0;
constexpr int kDenoiseMaxLevels = 8;
constexpr float kDemodEps = 0.01f;

// A pixel's feature record as two 16-byte loads: {albedo.rgb, n.x} {n.y, n.z, depth, coverage}.
struct FeatRec {
  float4 a, b;
};
BDPT_HD FeatRec load_feat(const float* F, size_t k) {
  const float4* p = (const float4*)F + 2 * k;
  FeatRec r;
  r.a = p[0];
  r.b = p[1];
  return r;
}

// Demodulation: the filter runs on colour / (albedo + 0.01) and the result is multiplied back.
BDPT_HD f3 demod_in(f3 c, const FeatRec& f) {
  return mk3(c.x / (f.a.x + kDemodEps), c.y / (f.a.y + kDemodEps), c.z / (f.a.z + kDemodEps));
}
BDPT_HD f3 demod_out(f3 c, const FeatRec& f) {
  return mk3(c.x * (f.a.x + kDemodEps), c.y * (f.a.y + kDemodEps), c.z * (f.a.z + kDemodEps));
}

struct AtrousLevel {
  int W, H, step;          // step = 2^level
  float sc, sn, sd;        // sigma_color * 2^-level, sigma_normal, sigma_depth
};

// Level i of a filter with these sigmas (host side of both builds): step 2^i, sigma_color halved per level.
inline AtrousLevel atrous_level(int W, int H, int i, float sigma_color, float sigma_normal, float sigma_depth) {
  AtrousLevel L;
  L.W = W; L.H = H; L.step = 1 << i;
  L.sc = ldexpf(sigma_color, -i);
  L.sn = sigma_normal;
  L.sd = sigma_depth;
  return L;
}

// One level at pixel (x, y): the 5x5 B3 taps at distance `step`, those inside the frame only, each
// weighted by exp(-(e_c + e_n + e_d)); the centre tap's weight is 1, so the denominator is >= 9/64.
BDPT_HD f3 atrous_pixel(const float* c_in, const float* F, const AtrousLevel& L, int x, int y) {
  const float kk[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
  const size_t p = (size_t)x + (size_t)y * L.W;
  const f3 cp = mk3(c_in[3 * p], c_in[3 * p + 1], c_in[3 * p + 2]);
  const FeatRec fp = load_feat(F, p);
  const f3 np = mk3(fp.a.w, fp.b.x, fp.b.y);
  const float dp = fp.b.z;
  const float sc2 = L.sc * L.sc, sn2 = L.sn * L.sn;
  f3 num = splat3(0);
  float den = 0.0f;
  for (int dy = -2; dy <= 2; dy++) {
    const int qy = y + dy * L.step;
    if (qy < 0 || qy >= L.H) continue;
    for (int dx = -2; dx <= 2; dx++) {
      const int qx = x + dx * L.step;
      if (qx < 0 || qx >= L.W) continue;
      const size_t q = (size_t)qx + (size_t)qy * L.W;
      const f3 cq = mk3(c_in[3 * q], c_in[3 * q + 1], c_in[3 * q + 2]);
      float w = 1.0f;
      if (dx != 0 || dy != 0) {
        const FeatRec fq = load_feat(F, q);
        const float ec = norm2(sub(cp, cq)) / sc2;
        const float en = norm2(sub(np, mk3(fq.a.w, fq.b.x, fq.b.y))) / sn2;
        const float m = fmaxf(dp, fq.b.z);
        float ed = 0.0f;
        if (m != 0.0f) {
          const float r = (dp - fq.b.z) / (L.sd * m);
          ed = r * r;
        }
        w = expf(-((ec + en) + ed));
      }
      const float hw = (kk[dx + 2] * kk[dy + 2]) * w;
      num = add(num, smul(hw, cq));
      den += hw;
    }
  }
  return mk3(num.x / den, num.y / den, num.z / den);
}

}  // namespace bdpt
