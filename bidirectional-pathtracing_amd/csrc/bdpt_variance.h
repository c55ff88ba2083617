// bdpt_variance.h — per-pixel batch moments of a frame rendered in equal sample batches, the
// variance of the frame they estimate, and one level of the variance-guided a-trous filter
// (DESIGN.md §12). BDPT_HD: k_moments, k_variance and k_atrous_var (bdpt_variance.hip) and the host
// build (tests/native/core_cpu_variance.cpp) run the same code.

#pragma once

#include "bdpt_atrous.h"

namespace bdpt {

// bdpt_denoise_variance_params' defaults, chosen by the sweep of DESIGN.md §12
constexpr int kDenoiseVarLevels = 3;
constexpr float kDenoiseVarSigmaVariance = 4.0f, kDenoiseVarSigmaNormal = 0.3f, kDenoiseVarSigmaDepth = 0.03f;
constexpr float kVarEps = 1e-8f;

// The moments record of a pixel, one float4 {prev.r, prev.g, prev.b, Q}: the cumulative colour after
// the last batch and the sum over the batches of |increment|^2. f is the cumulative colour now.
BDPT_HD float4 moments_add(float4 rec, f3 f) {
  const f3 b = sub(f, mk3(rec.x, rec.y, rec.z));
  float4 r;
  r.x = f.x; r.y = f.y; r.z = f.z;
  r.w = rec.w + ((b.x * b.x + b.y * b.y) + b.z * b.z);
  return r;
}

// {1/K, K/(K-1)} of K batches, computed once on the host in fp32.
struct VarK {
  float inv_k, k_over_km1;
};
inline VarK var_k(int K) {
  VarK kf;
  kf.inv_k = 1.0f / (float)K;
  kf.k_over_km1 = (float)K / (float)(K - 1);
  return kf;
}

// The trace of the covariance of the pixel's colour as rendered: K equal batches with increments b_k,
// F = sum b_k, Q = sum |b_k|^2: K/(K-1) (Q - |F|^2/K), unbiased; clamped at 0.
BDPT_HD float variance_of(float4 rec, VarK kf) {
  const float s = (rec.x * rec.x + rec.y * rec.y) + rec.z * rec.z;
  return fmaxf(0.0f, (rec.w - s * kf.inv_k) * kf.k_over_km1);
}

// Level i of the variance-guided filter: atrous_level's, but sc = sigma_variance at every level (the
// variance shrinks as the filter proceeds; sigma does not).
inline AtrousLevel atrous_var_level(int W, int H, int i, float sigma_variance, float sigma_normal, float sigma_depth) {
  AtrousLevel L = atrous_level(W, H, i, sigma_variance, sigma_normal, sigma_depth);
  L.sc = sigma_variance;
  return L;
}

struct ColVar {
  f3 c;
  float v;
};

// The 3x3 Gaussian (1/4, 1/2, 1/4)^2 of v_in around (x, y) at unit distance, in-frame taps only,
// divided by the sum of the weights used.
BDPT_HD float var_prefilter(const float* v_in, int W, int H, int x, int y) {
  const float g[3] = {0.25f, 0.5f, 0.25f};
  float s = 0.0f, ws = 0.0f;
  for (int dy = -1; dy <= 1; dy++) {
    const int qy = y + dy;
    if (qy < 0 || qy >= H) continue;
    for (int dx = -1; dx <= 1; dx++) {
      const int qx = x + dx;
      if (qx < 0 || qx >= W) continue;
      const float w = g[dx + 1] * g[dy + 1];
      s += w * v_in[(size_t)qx + (size_t)qy * W];
      ws += w;
    }
  }
  return s / ws;
}

// One level at pixel (x, y): atrous_pixel's taps, kernel, in-frame rule, e_n and e_d; the colour term
// is e_c = |c(p) - c(q)|^2 / (sigma_v^2 v~(p) + 1e-8) with v~ the prefiltered variance. Colour:
// sum h w c(q) / sum h w, evaluated as c(p) + sum h w (c(q) - c(p)) / sum h w, so a pixel whose
// other taps all weigh 0 comes back bit for bit. Variance: sum (h w)^2 v(q) / (sum h w)^2, and not
// above the largest v(q) of the taps (which only rounding could make it).
BDPT_HD ColVar atrous_var_pixel(const float* c_in, const float* v_in, const float* F, const AtrousLevel& L, int x, int y) {
  const float kk[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
  const size_t p = (size_t)x + (size_t)y * L.W;
  const f3 cp = mk3(c_in[3 * p], c_in[3 * p + 1], c_in[3 * p + 2]);
  const FeatRec fp = load_feat(F, p);
  const f3 np = mk3(fp.a.w, fp.b.x, fp.b.y);
  const float dp = fp.b.z;
  const float sn2 = L.sn * L.sn;
  const float cden = (L.sc * L.sc) * var_prefilter(v_in, L.W, L.H, x, y) + kVarEps;
  f3 num = splat3(0);
  float den = 0.0f, vnum = 0.0f, vmax = 0.0f;
  for (int dy = -2; dy <= 2; dy++) {
    const int qy = y + dy * L.step;
    if (qy < 0 || qy >= L.H) continue;
    for (int dx = -2; dx <= 2; dx++) {
      const int qx = x + dx * L.step;
      if (qx < 0 || qx >= L.W) continue;
      const size_t q = (size_t)qx + (size_t)qy * L.W;
      const f3 dc = sub(mk3(c_in[3 * q], c_in[3 * q + 1], c_in[3 * q + 2]), cp);
      const float vq = v_in[q];
      float w = 1.0f;
      if (dx != 0 || dy != 0) {
        const FeatRec fq = load_feat(F, q);
        const float ec = norm2(dc) / cden;
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
      num = add(num, smul(hw, dc));
      den += hw;
      vnum += (hw * hw) * vq;
      vmax = fmaxf(vmax, vq);
    }
  }
  ColVar r;
  r.c = mk3(cp.x + num.x / den, cp.y + num.y / den, cp.z + num.z / den);
  r.v = fminf(vnum / (den * den), vmax);
  return r;
}

}  // namespace bdpt
