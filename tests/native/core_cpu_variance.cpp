// tests/native/core_cpu_variance.cpp — TEST ONLY. The host build of the variance-guided denoise's
// device code (bdpt_variance.h), in the shape of core_cpu_denoise.cpp: the yardstick
// of k_moments, k_variance and k_atrous_var. Never linked into the product.
#include <cstring>
#include <vector>

#include "bdpt_variance.h"

using namespace bdpt;

// One batch into the record (npix float4): the cumulative frame is a, or a + b when b is not null.
extern "C" int core_cpu_variance_moments(const float* a, const float* b, float* rec, long long npix) {
  if (!a || !rec || npix <= 0) return -1;
  for (long long i = 0; i < npix; i++) {
    f3 f = mk3(a[3 * i], a[3 * i + 1], a[3 * i + 2]);
    if (b) f = add(f, mk3(b[3 * i], b[3 * i + 1], b[3 * i + 2]));
    float4 r;
    std::memcpy(&r, rec + 4 * i, sizeof r);
    r = moments_add(r, f);
    std::memcpy(rec + 4 * i, &r, sizeof r);
  }
  return 0;
}

// The variance frame (npix floats) of a record of K batches.
extern "C" int core_cpu_variance_variance(const float* rec, int K, long long npix, float* var) {
  if (!rec || !var || K < 2 || npix <= 0) return -1;
  const VarK kf = var_k(K);
  for (long long i = 0; i < npix; i++) {
    float4 r;
    std::memcpy(&r, rec + 4 * i, sizeof r);
    var[i] = variance_of(r, kf);
  }
  return 0;
}

// The library's defaults (bdpt_variance.h): levels, {sigma_variance, sigma_normal, sigma_depth}.
extern "C" void core_cpu_variance_defaults(int* levels, float* sigmas) {
  levels[0] = kDenoiseVarLevels;
  sigmas[0] = kDenoiseVarSigmaVariance; sigmas[1] = kDenoiseVarSigmaNormal; sigmas[2] = kDenoiseVarSigmaDepth;
}

// The filter on host memory, in the pass order of bdpt_variance.hip's enqueue_filter. out may be
// color, var_out may be var or null.
extern "C" int core_cpu_variance_filter(const float* color, const float* var, const float* feat, int W, int H, int levels,
                                        float sigma_variance, float sigma_normal, float sigma_depth, float* out,
                                        float* var_out) {
  if (W <= 0 || H <= 0 || levels < 0 || levels > kDenoiseMaxLevels) return -1;
  const size_t npix = (size_t)W * H;
  // the feature records are read 16 bytes at a time: an aligned copy
  std::vector<float4> F4(2 * npix);
  std::memcpy(F4.data(), feat, npix * 8 * sizeof(float));
  const float* F = (const float*)F4.data();
  std::vector<float> a(color, color + 3 * npix), b(3 * npix), va(var, var + npix), vb(npix);
  for (int i = 0; i < levels; i++) {
    const AtrousLevel L = atrous_var_level(W, H, i, sigma_variance, sigma_normal, sigma_depth);
    for (int y = 0; y < H; y++)
      for (int x = 0; x < W; x++) {
        const ColVar r = atrous_var_pixel(a.data(), va.data(), F, L, x, y);
        const size_t p = (size_t)x + (size_t)y * W;
        b[3 * p] = r.c.x; b[3 * p + 1] = r.c.y; b[3 * p + 2] = r.c.z;
        vb[p] = r.v;
      }
    a.swap(b);
    va.swap(vb);
  }
  std::memcpy(out, a.data(), 3 * npix * sizeof(float));
  if (var_out) std::memcpy(var_out, va.data(), npix * sizeof(float));
  return 0;
}
