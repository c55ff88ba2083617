// bdpt_bsdf.h — samplers (sampler.cpp) and BSDFs (bsdf.cpp, advanced_bsdf.cpp) in the device
// semantics: sample_f, f and the pdfs of every material.

#pragma once

#include "bdpt_sceneview.h"

namespace bdpt {

// ------------------------------------------------------------------------------------------------
// Samplers (sampler.cpp) and BSDFs (bsdf.cpp, advanced_bsdf.cpp)
BDPT_HD void grid2d(Rng& g, float* x, float* y) {   // Vector2D(U(), U()): y is drawn first
  float b = rng_next(g);
  float a = rng_next(g);
  *x = a;
  *y = b;
}
BDPT_HD f3 cosine_hemi(Rng& g, float* pdf) {   // sampler.cpp:76-86
  float Xi1 = rng_next(g);
  float Xi2 = rng_next(g);
  float r = sqrtf(Xi1);
  *pdf = sqrtf(1 - Xi1) / BDPT_PI_F;
  float c, s;
  cos_sin_2pi(Xi2, &c, &s);
  return mk3(r * c, r * s, sqrtf(1 - Xi1));
}
BDPT_HD float cosine_pdf_z(float z) { return z > 0 ? z / BDPT_PI_F : 0.0f; }   // sampler.cpp:92-95

BDPT_HD bool is_delta(int type) { return type == MAT_MIRROR || type == MAT_GLASS || type == MAT_REFRACTION; }

BDPT_HD bool refract_dir(f3 wo, f3* wi, float ior) {   // advanced_bsdf.cpp:279-303
  bool enter = wo.z > 0;
  float eta = enter ? 1.0f / ior : ior;
  float z_sq = 1 - eta * eta * (1 - wo.z * wo.z);
  if (z_sq < 0) return false;
  float sgn = enter ? -1.0f : 1.0f;
  *wi = mk3(-eta * wo.x, -eta * wo.y, sgn * sqrtf(z_sq));
  return true;
}

// MicrofacetBSDF (advanced_bsdf.cpp:46-142, bsdf.h:176-184) in the device semantics (PathTracer
// only): cos(acos z) = z, tan(acos z) = sqrt(1 - z^2) / z, integer powers by products, erf / exp /
// log from the fp32 math library (oracle mode 2 restates it, oracle/bdpt_oracle.cpp mf_*).
BDPT_HD float mf_lambda(float alpha, f3 w) {
  const float c = fminf(fmaxf(w.z, (float)(-1.0 + 1e-5)), (float)(1.0 - 1e-5));
  const float t = sqrtf(1.0f - c * c) / c;
  const float a = 1.0f / (alpha * t);
  return 0.5f * (erff(a) - 1.0f + expf(-a * a) / (a * BDPT_PI_F));
}
BDPT_HD float mf_G(float alpha, f3 wo, f3 wi) { return 1.0f / (1.0f + mf_lambda(alpha, wi) + mf_lambda(alpha, wo)); }
BDPT_HD float mf_D(float alpha, f3 h) {
  const float c = h.z;
  const float t = sqrtf(fmaxf(0.0f, 1.0f - c * c)) / c;
  const float q = t / alpha;
  const float c2 = c * c;
  return expf(-(q * q)) / (BDPT_PI_F * alpha * alpha * (c2 * c2));
}
BDPT_HD f3 mf_F(const DMat& M, f3 wi) {   // (Rs + Rp) / 2, CGL operator order
  const f3 eta = mk3(M.a[0], M.a[1], M.a[2]), k = mk3(M.b[0], M.b[1], M.b[2]);
  const float c = fabsf(wi.z) / norm(wi);
  const float c2 = c * c;
  const f3 e2k2 = add(mul(eta, eta), mul(k, k));
  const f3 t = muls(smul(2.0f, eta), c);
  const f3 Rs = mk3((e2k2.x - t.x + c2) / (e2k2.x + t.x + c2), (e2k2.y - t.y + c2) / (e2k2.y + t.y + c2),
                    (e2k2.z - t.z + c2) / (e2k2.z + t.z + c2));
  const f3 e = muls(e2k2, c2);
  const f3 Rp = mk3((e.x - t.x + 1.0f) / (e.x + t.x + 1.0f), (e.y - t.y + 1.0f) / (e.y + t.y + 1.0f),
                    (e.z - t.z + 1.0f) / (e.z + t.z + 1.0f));
  return divs(add(Rs, Rp), 2.0f);
}
BDPT_HD f3 mf_f(const DMat& M, f3 wo, f3 wi) {
  if (wo.z <= BDPT_EPS_F || wi.z <= BDPT_EPS_F) return splat3(0);
  const f3 h = normalize(add(wo, wi));
  return divs(muls(muls(mf_F(M, wi), mf_G(M.alpha, wo, wi)), mf_D(M.alpha, h)), 4.0f * wo.z * wi.z);
}
BDPT_HD f3 mf_sample_f(const DMat& M, Rng& g, f3 wo, f3* wi, float* pdf) {
  float rx, ry;
  grid2d(g, &rx, &ry);
  const float alpha = M.alpha;
  const float tt = sqrtf(-alpha * alpha * logf(1.0f - rx));   // tan(theta)
  const float ct = 1.0f / sqrtf(1.0f + tt * tt);
  const float st = tt * ct;
  float cp, sp;
  cos_sin_2pi(ry, &cp, &sp);
  const f3 h = mk3(st * cp, st * sp, ct);
  const float costheta = dot(wo, h) / norm(wo);
  const f3 d = sub(wo, muls(muls(h, costheta), norm(wo)));
  *wi = normalize(sub(muls(muls(h, costheta), norm(wo)), d));
  if (wo.z <= BDPT_EPS_F || wi->z <= BDPT_EPS_F) {
    *pdf = 1;
    *wi = mk3(0, 0, 1);
    return splat3(0);
  }
  const float q = tt / alpha, c2 = ct * ct;
  const float p_theta = 2.0f * st * expf(-(q * q)) / (alpha * alpha * (c2 * ct));
  const float p_phi = 1.0f / (2.0f * BDPT_PI_F);
  const float pdf_h = p_theta * p_phi / st;
  *pdf = pdf_h / (4.0f * dot(*wi, h));
  return mf_f(M, wo, *wi);
}

BDPT_HD f3 sample_f(const DMat& M, Rng& g, f3 wo, f3* wi, float* pdf) {
  f3 A = mk3(M.a[0], M.a[1], M.a[2]);
  switch (M.type) {
    case MAT_MICROFACET: return mf_sample_f(M, g, wo, wi, pdf);
    case MAT_DIFFUSE: {
      *wi = cosine_hemi(g, pdf);
      if (wo.z < 0 || wi->z < 0) return splat3(0);
      return divs(A, BDPT_PI_F);
    }
    case MAT_EMISSION: {
      *pdf = 1.0f / BDPT_PI_F;
      *wi = cosine_hemi(g, pdf);
      return splat3(0);
    }
    case MAT_MIRROR: {
      *wi = mk3(-wo.x, -wo.y, wo.z);
      *pdf = 1;
      float ct = fabsf(wi->z) / norm(*wi);
      return divs(A, ct);
    }
    case MAT_REFRACTION: {
      f3 B = mk3(M.b[0], M.b[1], M.b[2]);
      if (!refract_dir(wo, wi, M.ior)) { *pdf = 1; return splat3(0); }
      *pdf = 1;
      float eta = wo.z > 0 ? 1.0f / M.ior : M.ior;
      float ct = fabsf(wi->z) / norm(*wi);
      return divs(divs(B, ct), eta * eta);
    }
    default: {   // glass (advanced_bsdf.cpp:198-237)
      f3 B = mk3(M.b[0], M.b[1], M.b[2]);
      f3 wr = mk3(-wo.x, -wo.y, wo.z), wt;
      bool tir = !refract_dir(wo, &wt, M.ior);
      if (tir) {
        *pdf = 1;
        *wi = wr;
        float ct = fabsf(wi->z) / norm(wo);
        return divs(A, ct);
      }
      float cref = fabsf(wt.z) / norm(wt);
      float eta = wo.z > 0 ? 1.0f / M.ior : M.ior;
      float x = (1 - eta) / (1 + eta);
      float R0 = x * x;
      float m = 1 - cref, m2 = m * m, m4 = m2 * m2;
      float Rf = R0 + (1 - R0) * (m4 * m);
      if (rng_next(g) < Rf) {
        *wi = wr;
        *pdf = Rf;
        float ct = fabsf(wi->z) / norm(*wi);
        return divs(smul(Rf, A), ct);
      }
      *wi = wt;
      *pdf = 1 - Rf;
      float ct = fabsf(wi->z) / norm(*wi);
      return divs(divs(smul(1 - Rf, B), ct), eta * eta);
    }
  }
}

// BSDF::sample_pdf with wo = 0 (as every MIS call site passes, bidirection.cpp:150,189,...).
// `n` is the vertex normal (the frame is rebuilt only for glass, which needs wi.x, wi.y).
BDPT_HD float pdf_b(const DMat& M, f3 n, f3 zh, f3 dw) {
  switch (M.type) {
    case MAT_DIFFUSE:
    case MAT_EMISSION: return cosine_pdf_z(lz(dw, zh));
    case MAT_MIRROR:
    case MAT_REFRACTION: return 1.0f;
    default: {
      Frame f = make_frame_hit(n);
      f3 wi = to_local(f, dw), wt;
      if (!refract_dir(wi, &wt, M.ior)) return 1.0f;
      float c = fabsf(wt.z) / norm(wt);
      float eta = M.ior;   // wo = 0: wo.z > 0 is false (advanced_bsdf.cpp:251)
      float x = (1 - eta) / (1 + eta);
      float R0 = x * x;
      float m = 1 - c, m2 = m * m, m4 = m2 * m2;
      float Rf = R0 + (1 - R0) * (m4 * m);
      if (wi.z > 0) return Rf;
      return 1 - Rf;
    }
  }
}

}  // namespace bdpt
