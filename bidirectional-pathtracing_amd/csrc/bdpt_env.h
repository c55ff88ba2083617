// bdpt_env.h — the environment light (environment_light.cpp) in the device semantics: table
// searches, radiance and pdf lookups, direction sampling.

#pragma once

#include "bdpt_sceneview.h"

namespace bdpt {

// ------------------------------------------------------------------------------------------------
// EnvironmentLight (environment_light.cpp) in the device semantics: w points from the scene toward
// the environment (sample_L's *wi, sample_dir's r.d).
BDPT_HD int upper_idx(const float* a, int n, float u) {   // std::upper_bound(a, a + n, u) - a, <= n - 1
  int lo = 0, cnt = n;
  while (cnt > 0) {
    const int st = cnt >> 1, m = lo + st;
    if (!(u < a[m])) { lo = m + 1; cnt -= st + 1; }
    else cnt = st;
  }
  return lo < n ? lo : n - 1;
}
// The same index through a guide table gd[0..G] (gd[k] = upper_bound(a, a + n, k / G), G a power of
// two, bdpt_scene.cpp): u * G is exact, so the answer lies in [gd[k], gd[k + 1]] for k = floor(u * G)
// and only that range is searched (one or two dependent loads instead of log2 n).
BDPT_HD int upper_idx_guided(const float* a, int n, const int* gd, int G, float u) {
  int k = (int)(u * (float)G);
  k = k < 0 ? 0 : k > G - 1 ? G - 1 : k;
  int lo = gd[k], cnt = gd[k + 1] - lo;
  while (cnt > 0) {
    const int st = cnt >> 1, m = lo + st;
    if (!(u < a[m])) { lo = m + 1; cnt -= st + 1; }
    else cnt = st;
  }
  return lo < n ? lo : n - 1;
}
BDPT_HD f3 env_texel(const EnvView& E, int k) {
  const float* p = E.rgb + 3 * (size_t)k;
  return mk3(p[0], p[1], p[2]);
}
BDPT_HD f3 env_bilerp(const EnvView& E, float x, float y) {   // bilerp (:106-123)
  int right = lround_pos(x), left, v = lround_pos(y);
  const float u1 = ((float)right - x) + 0.5f;
  float v1;
  if (right == 0 || right == E.w) { left = E.w - 1; right = 0; }
  else left = right - 1;
  if (v == 0) { v = 1; v1 = 1.0f; }
  else if (v == E.h) { v = E.h - 1; v1 = 0.0f; }
  else v1 = ((float)v - y) + 0.5f;
  const int bottom = E.w * v, top = bottom - E.w;
  const float u0 = 1 - u1;
  const f3 a = add(muls(env_texel(E, top + left), u1), muls(env_texel(E, top + right), u0));
  const f3 b = add(muls(env_texel(E, bottom + left), u1), muls(env_texel(E, bottom + right), u0));
  return add(muls(a, v1), muls(b, 1 - v1));
}
// theta_phi_to_dir(xy_to_theta_phi(x, y)) (:88-104): phi = 2 pi x / w, theta = pi y / h;
// (cos(phi - pi) sin t, cos t, -sin(phi - pi) sin t) = (-cos phi sin t, cos t, sin phi sin t).
BDPT_HD f3 env_xy_to_dir(const EnvView& E, float x, float y, float* sin_theta) {
  float cp, sp, ct, st;
  cos_sin_2pi(x / (float)E.w, &cp, &sp);
  cos_sin_2pi((y / (float)E.h) * 0.5f, &ct, &st);
  *sin_theta = st;
  return mk3(-cp * st, ct, sp * st);
}
// theta_phi_to_xy(dir_to_theta_phi(u)) (:81-86, 97-102) for a unit u: theta = acos(u.y),
// phi = atan2(-u.z, u.x) + pi; sin(theta) as sqrt((1 - y)(1 + y)).
BDPT_HD void env_dir_to_xy(const EnvView& E, f3 u, float* x, float* y, float* sin_theta) {
  const float st = sqrtf(fmaxf(0.0f, (1.0f - u.y) * (1.0f + u.y)));
  const float th = atan2_det(st, u.y);
  const float ph = atan2_det(-u.z, u.x) + BDPT_PI_F;
  *x = ph / 2.0f / BDPT_PI_F * (float)E.w;
  *y = th / BDPT_PI_F * (float)E.h;
  *sin_theta = st;
}
// sample_dir (:159-168): the radiance arriving along -u from direction u
BDPT_HD f3 env_radiance(const EnvView& E, f3 u) {
  float x, y, st;
  env_dir_to_xy(E, u, &x, &y, &st);
  return env_bilerp(E, x, y);
}
// Solid-angle density of sample_L choosing direction u (the pdf sample_L returns, :152, for the
// texel u falls in); 0 at the poles.
BDPT_HD float env_pdf_dir(const EnvView& E, f3 u) {
  float x, y, st;
  env_dir_to_xy(E, u, &x, &y, &st);
  if (!(st > 0.0f)) return 0.0f;
  const int xi = (int)x, yi = (int)y;
  const int i = xi < E.w - 1 ? xi : E.w - 1, j = yi < E.h - 1 ? yi : E.h - 1;
  return E.pdf[E.w * j + i] * (float)(E.w * E.h) / (2.0f * BDPT_PI_F * BDPT_PI_F * st);
}
// sample_L's direction sampling (:126-156): row by the marginal CDF, column by the row's CDF, then
// a uniform jitter inside the texel; returns bilerp(xy) (4 uniforms).
BDPT_HD f3 env_sample_dir(const EnvView& E, Rng& g, f3* w, float* pdf) {
  float ux, uy;
  grid2d(g, &ux, &uy);
  int y, x;
  if (E.gmarg) {
    y = upper_idx_guided(E.marg, E.h, E.gmarg, E.gm, uy);
    x = upper_idx_guided(E.cond + (size_t)E.w * y, E.w, E.gcond + (size_t)(E.gc + 1) * y, E.gc, ux);
  } else {
    y = upper_idx(E.marg, E.h, uy);
    x = upper_idx(E.cond + (size_t)E.w * y, E.w, ux);
  }
  const float xf = (float)x + rng_next(g);
  const float yf = (float)y + rng_next(g);
  float st;
  *w = env_xy_to_dir(E, xf, yf, &st);
  *pdf = E.pdf[E.w * y + x] * (float)(E.w * E.h) / (2.0f * BDPT_PI_F * BDPT_PI_F * st);
  return env_bilerp(E, xf, yf);
}

// ------------------------------------------------------------------------------------------------
// Hemisphere (ambient) and directional lights under BDPT: the environment light's
// machinery with a uniform hemisphere about +y, or one delta direction, in place of the tables.
// sample_L's direction w (toward the light), its pdf and radiance: InfiniteHemisphereLight
// (light.cpp:62-70, two uniforms, pdf 1/2pi) or DirectionalLight (light.cpp:17-23: dirToLight, no
// uniform; its pdf 1 stands for the delta, which cancels between the strategies that sample it).
BDPT_HD float hemi_pdf() { return (float)(1.0 / (2.0 * 3.14159265358979323)); }   // bdpt_pt.h light_sample_L's constant
BDPT_HD f3 inf_sample_dir(const DLight& L, Rng& g, f3* w, float* pdf) {
  if (L.type == LIGHT_DIR) {
    *w = mk3(L.dir[0], L.dir[1], L.dir[2]);
    *pdf = 1.0f;
  } else {
    const float Xi1 = rng_next(g);
    const float Xi2 = rng_next(g);
    float c, s;
    cos_sin_2pi(Xi2, &c, &s);
    const float st = sqrtf(fmaxf(0.0f, 1.0f - Xi1 * Xi1));
    *w = mk3(st * c, Xi1, -(st * s));
    *pdf = hemi_pdf();
  }
  return mk3(L.rad[0], L.rad[1], L.rad[2]);
}
// The hemisphere light seen along direction u (toward it): its radiance above the horizon
BDPT_HD f3 hemi_radiance(const DLight& L, f3 u) { return u.y > 0.0f ? mk3(L.rad[0], L.rad[1], L.rad[2]) : splat3(0); }

}  // namespace bdpt
