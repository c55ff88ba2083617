// bdpt_features.h — first-hit feature buffers: per pixel the albedo, normal, depth
// and coverage of the first vertex of its eye paths, through the integrator's own primary rays.
// BDPT_HD: k_features (bdpt_denoise.hip) and the host build (tests/native/core_cpu_denoise.cpp) run
// the same code.

#pragma once

#include "bdpt_pt.h"

namespace bdpt {

// Which integrator's primary ray: BDPT's pinhole (walk_begin), BDPT's thin lens (walk_begin at
// EXT = 3: the lens point on sub-stream RNG_LENS_WALK), the PathTracer's (pt_sample: its lens draw
// follows the jitter on stream 0, at any lens radius).
enum { FEAT_BDPT = 0, FEAT_BDPT_LENS = 1, FEAT_PT = 2 };

struct FeatParams {
  int W, H;
  int nsamp;        // samples [0, nsamp) of every pixel
  int kind;         // FEAT_*
  uint64_t seed;
  float focal;      // FEAT_BDPT_LENS: SampleParams::focal; FEAT_PT: PtParams::focal_distance
  float lens_r;     // FEAT_PT: PtParams::lens_radius (FEAT_BDPT_LENS reads DCam::lens_r, as its kernels do)
};

struct PrimaryRay {
  f3 o, d;
  float tmin, tmax;
};

// The primary ray of sample s of pixel (x, y): the origin, direction and window of the integrator's
// first closest-hit query. The expressions are walk_begin's (bdpt_paths.h) and pt_sample's
// (bdpt_pt.h), restated here so that those two keep their instruction streams.
BDPT_HD PrimaryRay feature_primary_ray(const DCam& cam, const FeatParams& fp, int x, int y, uint32_t s) {
  Rng g;
  rng_init(g, fp.seed, (uint32_t)(x + y * fp.W), s);
  float px, py;
  grid2d(g, &px, &py);
  px = px + (float)x;
  py = py + (float)y;
  const float dx = px / (float)fp.W, dy = py / (float)fp.H;
  PrimaryRay r;
  r.tmin = cam.nclip;
  r.tmax = cam.fclip;
  if (fp.kind == FEAT_PT) {   // Camera::generate_ray_for_thin_lens (pt_sample)
    float lx, ly;
    grid2d(g, &lx, &ly);
    float lc, ls;
    cos_sin_2pi(ly, &lc, &ls);
    const f3 pLens = mk3(fp.lens_r * sqrtf(lx) * lc, fp.lens_r * sqrtf(lx) * ls, 0.0f);
    const f3 rdir = mk3((2 * dx - 1) * cam.tanh_, (2 * dy - 1) * cam.tanv_, -1.0f);
    const f3 rd0 = sub(muls(rdir, fp.focal), pLens);
    const f3 c0 = mk3(cam.c2w[0], cam.c2w[1], cam.c2w[2]), c1 = mk3(cam.c2w[3], cam.c2w[4], cam.c2w[5]),
             c2 = mk3(cam.c2w[6], cam.c2w[7], cam.c2w[8]);
    r.d = normalize(add(add(smul(rd0.x, c0), smul(rd0.y, c1)), smul(rd0.z, c2)));
    r.o = add(mk3(cam.pos[0], cam.pos[1], cam.pos[2]),
              add(add(smul(pLens.x, c0), smul(pLens.y, c1)), smul(pLens.z, c2)));
  } else if (fp.kind == FEAT_BDPT_LENS) {
    const f3 pl = lens_draw(cam, g, RNG_LENS_WALK);
    r.o = lens_world(cam, pl);
    r.d = lens_ray_dir(cam, fp.focal, pl, dx, dy);
  } else {
    r.o = mk3(cam.pos[0], cam.pos[1], cam.pos[2]);
    r.d = camera_dir(cam, dx, dy);
  }
  return r;
}

// The albedo a denoiser divides out, per material kind.
BDPT_HD f3 feature_albedo(const DMat& M) {
  const f3 a = mk3(M.a[0], M.a[1], M.a[2]), b = mk3(M.b[0], M.b[1], M.b[2]);
  switch (M.type) {
    case MAT_REFRACTION: return b;
    case MAT_GLASS: return mk3(fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z));
    case MAT_EMISSION: return mk3(fminf(a.x, 1.0f), fminf(a.y, 1.0f), fminf(a.z, 1.0f));
    case MAT_MICROFACET: return mf_F(M, mk3(0.0f, 0.0f, 1.0f));   // Fresnel reflectance at normal incidence
    default: return a;   // diffuse, mirror
  }
}

struct FeatSample {
  f3 albedo, n;
  float t;
  int prim;   // position in the device tree's leaf order, -1 = miss
};

// One sample's first hit: trace_closest + shade_hit on the primary ray; a miss is all zeros.
template <int LM>
BDPT_HD FeatSample feature_sample(const SceneView& S, const FeatParams& fp, Counters& cnt, int x, int y, uint32_t s) {
  const PrimaryRay r = feature_primary_ray(S.cam, fp, x, y, s);
  FeatSample f;
  f.albedo = splat3(0);
  f.n = splat3(0);
  f.t = 0.0f;
  f.prim = -1;
  Hit h;
  if (!trace_closest<LM, kWalkStack>(S, r.o, r.d, r.tmin, r.tmax, h, cnt)) return f;
  f3 n;
  int mat;
  shade_hit<LM>(S, h, r.o, r.d, &n, &mat);
  f.albedo = feature_albedo(S.mats[mat]);
  f.n = dot(n, r.d) > 0 ? neg(n) : n;   // facing the ray
  f.t = h.t;
  f.prim = h.prim;
  return f;
}

// The pixel's record: 8 floats {albedo.rgb, normal.xyz, depth, coverage}, sums over the samples in
// sample order. Albedo and normal are means over all samples (the normal is not renormalised), the
// depth is the mean over the hits, the coverage the fraction of samples that hit.
template <int LM>
BDPT_HD void feature_pixel(const SceneView& S, const FeatParams& fp, Counters& cnt, int x, int y, float* out8) {
  f3 alb = splat3(0), nrm = splat3(0);
  float depth = 0.0f;
  int hits = 0;
  for (int s = 0; s < fp.nsamp; s++) {
    const FeatSample f = feature_sample<LM>(S, fp, cnt, x, y, (uint32_t)s);
    alb = add(alb, f.albedo);
    nrm = add(nrm, f.n);
    depth += f.t;
    hits += f.prim >= 0 ? 1 : 0;
  }
  const float n = (float)fp.nsamp;
  out8[0] = alb.x / n; out8[1] = alb.y / n; out8[2] = alb.z / n;
  out8[3] = nrm.x / n; out8[4] = nrm.y / n; out8[5] = nrm.z / n;
  out8[6] = depth / (float)(hits > 0 ? hits : 1);
  out8[7] = (float)hits / n;
}

}  // namespace bdpt
