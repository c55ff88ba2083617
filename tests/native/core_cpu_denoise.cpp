// tests/native/core_cpu_denoise.cpp — TEST ONLY. The host build of the denoised-output device code
// (bdpt_features.h, bdpt_atrous.h) over the host scene preparation (bdpt_scene.cpp),
// in the shape of core_cpu_lens.cpp: the yardstick of k_features and k_atrous. Never linked into
// the product.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "bdpt_atrous.h"
#include "bdpt_features.h"
#include "bdpt_scene.h"
#include "core_cpu_host.h"

using namespace bdpt;

namespace {

// The scene and FeatParams of a context of these settings, as bdpt_create / bdpt_render_features
// set them up. integrator: 0 BDPT, 1 PathTracer.
struct Setup {
  HostScene hs;
  FeatParams fp;
};
int setup(const bdpt_scene_desc* d, int W, int H, int nsamp, uint64_t seed, int integrator, double lens_radius,
          double focal_distance, int infinite_lights, Setup& s) {
  std::string err;
  const bool pt = integrator == 1;
  const int rc = build_host_scene(d, s.hs, err, pt, infinite_lights != 0);
  if (rc) { fprintf(stderr, "core_cpu_denoise: %s\n", err.c_str()); return rc; }
  const bool lens = !pt && lens_radius > 0;
  s.hs.cam.lens_r = lens ? (float)lens_radius : 0.0f;
  s.fp.W = W; s.fp.H = H; s.fp.nsamp = nsamp; s.fp.seed = seed;
  if (pt) {
    s.fp.kind = FEAT_PT;
    s.fp.lens_r = (float)lens_radius;
    s.fp.focal = lens_focal(focal_distance);
  } else {
    s.fp.kind = kernel_flavour(s.hs, false, lens) == 3 ? FEAT_BDPT_LENS : FEAT_BDPT;
    s.fp.lens_r = 0.0f;
    s.fp.focal = lens_focal(focal_distance);
  }
  return 0;
}

template <int LM>
void render_lm(const Setup& s, float* out8) {
  const SceneView S = host_view(s.hs, LM);
  Counters cnt = {0, 0, 0, 0, 0, 0};
  for (int y = 0; y < s.fp.H; y++)
    for (int x = 0; x < s.fp.W; x++) feature_pixel<LM>(S, s.fp, cnt, x, y, out8 + 8 * ((size_t)x + (size_t)y * s.fp.W));
}

template <int LM>
void samples_lm(const Setup& s, int n, const int* xys, int* prim, float* t, float* albedo, float* normal) {
  const SceneView S = host_view(s.hs, LM);
  Counters cnt = {0, 0, 0, 0, 0, 0};
  for (int k = 0; k < n; k++) {
    const FeatSample f = feature_sample<LM>(S, s.fp, cnt, xys[3 * k], xys[3 * k + 1], (uint32_t)xys[3 * k + 2]);
    prim[k] = f.prim >= 0 ? s.hs.prim_ref[f.prim] : -1;
    t[k] = f.t;
    albedo[3 * k] = f.albedo.x; albedo[3 * k + 1] = f.albedo.y; albedo[3 * k + 2] = f.albedo.z;
    normal[3 * k] = f.n.x; normal[3 * k + 1] = f.n.y; normal[3 * k + 2] = f.n.z;
  }
}

void put_ray(float* r, f3 o, f3 d, float tmin, float tmax) {
  r[0] = o.x; r[1] = o.y; r[2] = o.z; r[3] = d.x; r[4] = d.y; r[5] = d.z; r[6] = tmin; r[7] = tmax;
}

// The first ray of BDPT's own eye walk: walk_begin (bdpt_paths.h) at flavour EXT.
template <int EXT>
void walk_begin_rays(const Setup& s, int n, const int* xys, float* rays) {
  const SceneView S = host_view(s.hs, 0);
  SampleParams sp;
  sp.W = s.fp.W; sp.H = s.fp.H; sp.spp = s.fp.nsamp; sp.max_depth = 5; sp.seed = s.fp.seed;
  sp.rr = 0;
  sp.focal = s.fp.focal;
  Paths<5>* P = new Paths<5>();
  Counters cnt = {0, 0, 0, 0, 0, 0};
  for (int k = 0; k < n; k++) {
    Rng g;
    WalkState<5> w;
    walk_begin<5, EXT>(S, sp, *P, cnt, g, w, xys[3 * k], xys[3 * k + 1], (uint32_t)xys[3 * k + 2]);
    put_ray(rays + 8 * k, w.ro, w.rd, w.rmin, w.rmax);
  }
  delete P;
}

}  // namespace

// The feature frame (W*H*8 floats) of samples [0, nsamp) of every pixel.
extern "C" int core_cpu_denoise_features(const bdpt_scene_desc* d, int W, int H, int nsamp, uint64_t seed, int integrator,
                                         double lens_radius, double focal_distance, int infinite_lights, int lds_mode,
                                         float* out8) {
  Setup s;
  const int rc = setup(d, W, H, nsamp, seed, integrator, lens_radius, focal_distance, infinite_lights, s);
  if (rc) return rc;
  return dispatch_lm(lds_mode, [&](auto LM) { render_lm<decltype(LM)::value>(s, out8); return 0; });
}

// The primary rays (n*8 floats: o, d, tmin, tmax) of the n samples xys = {x, y, s}.
extern "C" int core_cpu_denoise_primary_rays(const bdpt_scene_desc* d, int W, int H, uint64_t seed, int integrator,
                                             double lens_radius, double focal_distance, int n, const int* xys,
                                             float* rays) {
  Setup s;
  const int rc = setup(d, W, H, 1, seed, integrator, lens_radius, focal_distance, 0, s);
  if (rc) return rc;
  for (int k = 0; k < n; k++) {
    const PrimaryRay r = feature_primary_ray(s.hs.cam, s.fp, xys[3 * k], xys[3 * k + 1], (uint32_t)xys[3 * k + 2]);
    put_ray(rays + 8 * k, r.o, r.d, r.tmin, r.tmax);
  }
  return 0;
}

// Per sample: the scene index of the primitive the feature pass hits (-1: none), its distance, and
// the sample's albedo and normal (n*3 floats each).
extern "C" int core_cpu_denoise_sample_prims(const bdpt_scene_desc* d, int W, int H, uint64_t seed, int integrator,
                                             double lens_radius, double focal_distance, int lds_mode, int n,
                                             const int* xys, int* prim, float* t, float* albedo, float* normal) {
  Setup s;
  const int rc = setup(d, W, H, 1, seed, integrator, lens_radius, focal_distance, 0, s);
  if (rc) return rc;
  return dispatch_lm(lds_mode, [&](auto LM) { samples_lm<decltype(LM)::value>(s, n, xys, prim, t, albedo, normal); return 0; });
}

// The first ray of the BDPT eye walk of each sample, from walk_begin itself (the pinhole flavour,
// or flavour 3 with lens_radius > 0).
extern "C" int core_cpu_denoise_walk_begin_rays(const bdpt_scene_desc* d, int W, int H, uint64_t seed, double lens_radius,
                                                double focal_distance, int n, const int* xys, float* rays) {
  Setup s;
  const int rc = setup(d, W, H, 1, seed, 0, lens_radius, focal_distance, 0, s);
  if (rc) return rc;
  if (s.fp.kind == FEAT_BDPT_LENS) walk_begin_rays<3>(s, n, xys, rays);
  else walk_begin_rays<0>(s, n, xys, rays);
  return 0;
}

// The radiance of PathTracer samples (pt_sample, max_depth 1: emission + direct light of the first
// hit): on a scene whose materials all emit, the first hit's radiance.
extern "C" int core_cpu_denoise_pt_samples(const bdpt_scene_desc* d, int W, int H, uint64_t seed, double lens_radius,
                                           double focal_distance, int n, const int* xys, float* rgb) {
  Setup s;
  const int rc = setup(d, W, H, 1, seed, 1, lens_radius, focal_distance, 0, s);
  if (rc) return rc;
  const SceneView S = host_view(s.hs, 0);
  PtParams pp;
  pp.W = W; pp.H = H; pp.spp = 1; pp.max_depth = 1; pp.seed = seed;
  pp.ns_area_light = 1; pp.batch = 1; pp.hemisphere = 0; pp.tol = 0.0f;
  pp.lens_radius = s.fp.lens_r;
  pp.focal_distance = s.fp.focal;
  Counters cnt = {0, 0, 0, 0, 0, 0};
  for (int k = 0; k < n; k++) {
    const f3 v = pt_sample<0>(S, pp, cnt, xys[3 * k], xys[3 * k + 1], (uint32_t)xys[3 * k + 2]);
    rgb[3 * k] = v.x; rgb[3 * k + 1] = v.y; rgb[3 * k + 2] = v.z;
  }
  return 0;
}

// The library's defaults (bdpt_atrous.h): {levels, demodulate}, {sigma_color, sigma_normal, sigma_depth}.
extern "C" void core_cpu_denoise_defaults(int* levels_demod, float* sigmas) {
  levels_demod[0] = kDenoiseLevels; levels_demod[1] = kDenoiseDemodulate;
  sigmas[0] = kDenoiseSigmaColor; sigmas[1] = kDenoiseSigmaNormal; sigmas[2] = kDenoiseSigmaDepth;
}

// The filter on host memory, in the pass order of bdpt_denoise.hip's enqueue_filter. out may be color.
extern "C" int core_cpu_denoise_filter(const float* color, const float* feat, int W, int H, int levels,
                                       float sigma_color, float sigma_normal, float sigma_depth, int demodulate,
                                       float* out) {
  if (W <= 0 || H <= 0 || levels < 0 || levels > kDenoiseMaxLevels) return -1;
  const size_t npix = (size_t)W * H;
  // the feature records are read 16 bytes at a time: an aligned copy
  std::vector<float4> F4(2 * npix);
  std::memcpy(F4.data(), feat, npix * 8 * sizeof(float));
  const float* F = (const float*)F4.data();
  std::vector<float> a(color, color + 3 * npix), b(3 * npix);
  if (demodulate)
    for (size_t p = 0; p < npix; p++) {
      const f3 v = demod_in(mk3(a[3 * p], a[3 * p + 1], a[3 * p + 2]), load_feat(F, p));
      a[3 * p] = v.x; a[3 * p + 1] = v.y; a[3 * p + 2] = v.z;
    }
  for (int i = 0; i < levels; i++) {
    const AtrousLevel L = atrous_level(W, H, i, sigma_color, sigma_normal, sigma_depth);
    for (int y = 0; y < H; y++)
      for (int x = 0; x < W; x++) {
        const f3 v = atrous_pixel(a.data(), F, L, x, y);
        const size_t p = (size_t)x + (size_t)y * W;
        b[3 * p] = v.x; b[3 * p + 1] = v.y; b[3 * p + 2] = v.z;
      }
    a.swap(b);
  }
  for (size_t p = 0; p < npix; p++) {
    f3 v = mk3(a[3 * p], a[3 * p + 1], a[3 * p + 2]);
    if (demodulate) v = demod_out(v, load_feat(F, p));
    out[3 * p] = v.x; out[3 * p + 1] = v.y; out[3 * p + 2] = v.z;
  }
  return 0;
}
