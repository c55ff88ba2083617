// tests/native/core_cpu_adaptive.cpp — TEST ONLY. The host build of the adaptive sampler's device code
// (bdpt_adaptive.h), in the shape of core_cpu_variance.cpp: the yardstick of
// k_adapt_moments, k_adapt_decide, k_adapt_compact and k_adapt_resolve. The kernels' sum order is
// restated here: the xor-butterfly over a block's 64 lanes, strides 32, 16, 8, 4, 2, 1. Never linked
// into the product.
#include <algorithm>
#include <cstring>

#include "bdpt_adaptive.h"

using namespace bdpt;

static float4 load4(const float* p) {
  float4 r;
  std::memcpy(&r, p, sizeof r);
  return r;
}

// s[lane] = s[lane] + s[lane ^ stride] for every lane at once, stride 32 .. 1: lane 0's value.
static float butterfly(float* s) {
  float t[64];
  for (int o = 32; o > 0; o >>= 1) {
    for (int l = 0; l < 64; l++) t[l] = s[l] + s[l ^ o];
    std::memcpy(s, t, sizeof t);
  }
  return s[0];
}

// One round into the two records (npix float4 each); round_samples = M_r.
extern "C" int core_cpu_adaptive_moments(const float* eye, const float* light, float* rec_e, float* rec_l, long long npix,
                                         long long round_samples) {
  if (!eye || !light || !rec_e || !rec_l || npix <= 0 || round_samples < 1) return -1;
  const float inv_m = (float)(1.0 / (double)round_samples);
  for (long long i = 0; i < npix; i++) {
    float4 r = moments_add(load4(rec_e + 4 * i), mk3(eye[3 * i], eye[3 * i + 1], eye[3 * i + 2]));
    std::memcpy(rec_e + 4 * i, &r, sizeof r);
    r = moments_add_weighted(load4(rec_l + 4 * i), mk3(light[3 * i], light[3 * i + 1], light[3 * i + 2]), inv_m);
    std::memcpy(rec_l + 4 * i, &r, sizeof r);
  }
  return 0;
}

// k_adapt_decide: K_b += 1 for the active blocks; with decide, the rule after R rounds and N
// pixel-samples. sums (may be null): per block {Sv, Sc} of the blocks that were evaluated.
extern "C" int core_cpu_adaptive_decide(const float* rec_e, const float* rec_l, int* rounds, int* active, int W, int H, int S, int m,
                                        int R, long long N, float tol, int decide, float* sums) {
  if (!rec_e || !rec_l || !rounds || !active || W <= 0 || H <= 0) return -1;
  if (decide && (R < 2 || N < 1 || S < 1 || m < 1)) return -1;
  AdaptScal sc = {0.0f, 0.0f, 0.0f};
  if (decide) sc = adapt_scal(W, H, S, R, N);
  const int nbx = (W + kAdaptBlock - 1) / kAdaptBlock, nby = (H + kAdaptBlock - 1) / kAdaptBlock;
  for (int b = 0; b < nbx * nby; b++) {
    if (active[b] == 0) continue;
    const int K = rounds[b] + 1;
    rounds[b] = K;
    if (!decide) continue;
    const int x0 = (b % nbx) * kAdaptBlock, y0 = (b / nbx) * kAdaptBlock;
    float sv[64], scol[64];
    for (int lane = 0; lane < 64; lane++) {
      const int x = x0 + (lane & 7), y = y0 + (lane >> 3);
      sv[lane] = scol[lane] = 0.0f;
      if (x < W && y < H) {
        const size_t p = (size_t)x + (size_t)y * W;
        const AdaptPix px = adapt_pixel(load4(rec_e + 4 * p), load4(rec_l + 4 * p), adapt_block(K, S, m), sc);
        sv[lane] = px.v;
        scol[lane] = adapt_csum(px.c);
      }
    }
    const float Sv = butterfly(sv), Sc = butterfly(scol);
    if (sums) { sums[2 * b] = Sv; sums[2 * b + 1] = Sc; }
    const int n = std::min(kAdaptBlock, W - x0) * std::min(kAdaptBlock, H - y0);
    if (adapt_stop(Sv, Sc, n, tol)) active[b] = 0;
  }
  return 0;
}

// k_adapt_compact: list4 (room for nbx * nby x 4 ints) in block order, counts = {blocks, pixels}.
extern "C" int core_cpu_adaptive_compact(const int* active, int W, int H, int* list4, int* counts) {
  if (!active || !list4 || !counts || W <= 0 || H <= 0) return -1;
  const int nbx = (W + kAdaptBlock - 1) / kAdaptBlock, nby = (H + kAdaptBlock - 1) / kAdaptBlock;
  int n = 0, pix = 0;
  for (int b = 0; b < nbx * nby; b++) {
    if (active[b] == 0) continue;
    const int x0 = (b % nbx) * kAdaptBlock, y0 = (b / nbx) * kAdaptBlock;
    const int bw = std::min(kAdaptBlock, W - x0), bh = std::min(kAdaptBlock, H - y0);
    list4[4 * n] = x0; list4[4 * n + 1] = y0; list4[4 * n + 2] = bw; list4[4 * n + 3] = bh;
    n++;
    pix += bw * bh;
  }
  counts[0] = n;
  counts[1] = pix;
  return 0;
}

// k_adapt_resolve: colour (npix * 3), variance (npix), counts (npix).
extern "C" int core_cpu_adaptive_resolve(const float* rec_e, const float* rec_l, const int* rounds, int W, int H, int S, int m, int R,
                                         long long N, float* color, float* var, int* count) {
  if (!rec_e || !rec_l || !rounds || !color || !var || !count || W <= 0 || H <= 0 || R < 2 || N < 1 || S < 1 || m < 1) return -1;
  const AdaptScal sc = adapt_scal(W, H, S, R, N);
  const int nbx = (W + kAdaptBlock - 1) / kAdaptBlock;
  for (int y = 0; y < H; y++)
    for (int x = 0; x < W; x++) {
      const size_t i = (size_t)x + (size_t)y * W;
      const int K = rounds[(y / kAdaptBlock) * nbx + x / kAdaptBlock];
      const AdaptPix px = adapt_pixel(load4(rec_e + 4 * i), load4(rec_l + 4 * i), adapt_block(K, S, m), sc);
      color[3 * i] = px.c.x; color[3 * i + 1] = px.c.y; color[3 * i + 2] = px.c.z;
      var[i] = px.v;
      count[i] = K * m;
    }
  return 0;
}

// The library's defaults (bdpt_adaptive.h): {samples_per_round, min_rounds}, tolerance.
extern "C" void core_cpu_adaptive_defaults(int* ints, float* tol) {
  ints[0] = kAdaptSamplesPerRound;
  ints[1] = kAdaptMinRounds;
  tol[0] = kAdaptTolerance;
}
