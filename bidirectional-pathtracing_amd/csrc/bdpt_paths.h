// bdpt_paths.h — the bidirectional estimator: path vertices and their store, MIS, the light and
// camera samples, the two walks, connection evaluation and the per-sample driver.

#pragma once

#include "bdpt_bvh.h"
#include "bdpt_bsdf.h"
#include "bdpt_env.h"

namespace bdpt {

// ------------------------------------------------------------------------------------------------
// Path vertices (PathVertex, bidirection.h:29-46) with the MIS path constants attached.
struct Vtx {
  f3 pos, n, zh, alpha;
  float fwd;   // MIS denominator of the step at this vertex (bidirection.cpp:194-211 / 257-280)
  float gp;    // MIS prefix: G of the vertex one step inward (see mis_horner), 0 at E[2] / L[1];
               // during the walk it holds the vertex's roulette probability q (PathVertex.q)
               // until the *_constants pass has consumed it
  int mat;     // -1: no BSDF (camera / light vertex); MAT_ENV_V: environment vertex
  float cq;    // > 0: can receive a connection — diffuse (the only BSDF with f != 0,
               // bsdf.cpp:52-62), seen from its front side (wo.z >= 0 toward the previous vertex),
               // alpha != 0 — and then equal to q; 0: cannot
};

struct LightSample {
  f3 pos, n, zh, alpha;
  float dir_pdf;
  float fwd;   // point_pdf / nL (the MIS denominator of the light end in environment scenes)
  bool env;    // environment (or, §9a, hemisphere / directional) light: n = zh = -w, pos unused
  bool delta;  // directional light: no escaped ray reaches it (read by the infinite-light kernels only)
};

// A vertex as the path store holds it: the shading axis zh is not stored (it is zaxis(n), or n
// itself for an environment vertex, and is recomputed where a connection reads it), and in the
// reference-only kernels (EXT = 0) the connectability flag rides in bit 16 of the material
// word, so a vertex is 12 dwords (48 B) instead of 16; EXT kernels keep cq (the roulette
// probability of a connectable vertex) as a 13th dword. The private segment is lane-interleaved
// per dword, so the dwords a kernel never touches cost no traffic.
// EXT is the kernel flavour: 0 reference-only; 1 environment map and / or roulette (§9); 2 the
// same plus hemisphere and directional lights (§9a); 3 flavour 2 plus the thin-lens camera (§9b).
// Code written `EXT ? ... : ...` serves 1, 2 and 3; what flavour 2 adds is behind `EXT >= 2` and
// what the lens adds behind `EXT >= 3`, so the lower flavours compile to what they were.
struct VtxS {
  f3 pos;
  float fwd;
  f3 n;
  float gp;
  f3 alpha;
  int mb;     // material id (low 16 bits, signed); EXT = false: bit 16 = can_connect
  float cq;   // EXT only
};
BDPT_HD int vs_mat(const VtxS& s) { return (int)(short)(s.mb & 0xffff); }
template <int EXT>
BDPT_HD void vtx_store(VtxS& s, const Vtx& v) {
  s.pos = v.pos; s.fwd = v.fwd; s.n = v.n; s.gp = v.gp; s.alpha = v.alpha;
  s.mb = (v.mat & 0xffff) | (!EXT && v.cq > 0.0f ? 0x10000 : 0);
  if (EXT) s.cq = v.cq;
}
template <int EXT>
BDPT_HD Vtx vtx_load(const VtxS& s) {
  Vtx v;
  v.pos = s.pos; v.fwd = s.fwd; v.n = s.n; v.gp = s.gp; v.alpha = s.alpha;
  v.mat = vs_mat(s);
  v.cq = EXT ? s.cq : ((s.mb >> 16) != 0 ? 1.0f : 0.0f);
  v.zh = v.n;   // hit vertices: make_frame_hit; environment vertices: n = zh = -w; L[1]'s zh is never read
  return v;
}

// Per-subpath bit masks indexed by the reference's vertex index k <= MAXV + 1: 32 bits up to the
// m = 16 kernels (unchanged code), 64 for the m <= 32 and m <= 62 ones.
template <int MAXV>
using DeltaMask = typename std::conditional<
    (MAXV > 62), unsigned __int128, typename std::conditional<(MAXV > 29), uint64_t, uint32_t>::type>::type;
static_assert(sizeof(DeltaMask<62>) * 8 >= 62 + 2, "delta mask holds vertex indices up to MAXV + 1");
static_assert(sizeof(DeltaMask<126>) * 8 >= 126 + 2, "delta mask holds vertex indices up to MAXV + 1");

template <int MAXV>
struct Paths {
  VtxS E[MAXV];       // E[k] at index k-2 (k >= 2): eye hits
  VtxS L[MAXV + 1];   // L[k] at index k-1 (k >= 1): L[1] = light vertex, then hits
  int nE, nL;        // path sizes including v0, v1 (reference's vector sizes)
  DeltaMask<MAXV> dE, dL;   // delta-BSDF bit masks: bit k set <=> E[k] / L[k] is_delta(); bit 0 of dL:
                            // L[1] is on a directional light (infinite-light kernels, §9a)
  DeltaMask<MAXV> cE, cL;   // connectable vertices: bit k set <=> E[k] / L[k] has cq > 0
  DeltaMask<MAXV> sE;       // s = 0 sources: bit k set <=> E[k] is on an emitter or the environment
  float l1_dir_pdf;
  f3 l1_d;           // the light walk's first direction and its pdf (read back when it starts)
  float l1_pdf;
};

struct SampleParams {
  int W, H, spp, max_depth;
  uint64_t seed;
  int rr;   // Russian roulette (bdpt_params.russian_roulette; honoured by EXT kernels only)
  float focal;   // the thin lens' focal distance (§9b; read by EXT = 3 only). It fills what was the
                 // struct's tail padding, so no kernel argument moves
};
static_assert(sizeof(SampleParams) == 32, "SampleParams: the focal distance takes the tail padding");

// Power-heuristic sums in Horner form. Along a subpath walked from the connection endpoint
// inward, the reference accumulates ratio_k = f_end * ... * f_k and adds ratio_k^2 when neither
// vertex of step k is delta (t_k). Innermost first, the same sum is G_k = f_k^2 (t_k + G_{k-1});
// every interior factor f_k is a path constant (rev/fwd pdf ratio), so G up to the vertex below
// the endpoint is cached per vertex (Vtx::gp) and a connection costs O(1) instead of O(i + j).
// A term whose inner sum is exactly zero stays zero (no inf * 0); the oracle's mode 2 evaluates
// the identical expression (oracle/bdpt_oracle.cpp horner_step).
BDPT_HD float mis_horner(float f, bool t, float g) {
  const float s = t ? 1.0f + g : g;
  return s == 0.0f ? 0.0f : (f * f) * s;
}

// MIS step quantities between a vertex `cur` and a neighbour `oth` whose BSDF/frame is used:
// d = normalize(cur - oth), g = |(w2o(oth)*d).z * dot(d, cur.n)| / dist^2 (bidirection.cpp:151-158).
BDPT_HD float step_g(f3 cur_pos, f3 cur_n, f3 oth_pos, f3 oth_zh, f3* dw_out) {
  f3 dw = sub(cur_pos, oth_pos);
  float dist = norm(dw);
  dw = normalize(dw);
  float wz = lz(dw, oth_zh);
  *dw_out = dw;
  return fabsf(wz * dot(dw, cur_n)) / (dist * dist);
}
// The same with environment vertices: an env vertex sits at infinity in direction
// w, with n = zh = -w. oth env: d = -w and g = |dot(d, cur.n)| (the emission disk's planar density
// projected onto cur); cur env: d = w and g = 1 (densities of an env vertex are solid-angle ones).
BDPT_HD float step_gx(f3 cur_pos, f3 cur_n, bool cur_env, f3 oth_pos, f3 oth_zh, bool oth_env, f3* dw_out) {
  if (cur_env) { *dw_out = neg(cur_n); return 1.0f; }
  if (oth_env) { *dw_out = oth_zh; return fabsf(dot(oth_zh, cur_n)); }
  return step_g(cur_pos, cur_n, oth_pos, oth_zh, dw_out);
}
BDPT_HD bool is_env(const Vtx& v) { return v.mat == MAT_ENV_V; }

// AreaLight/PointLight BDPT methods (light.cpp:115-153, 219-284).
BDPT_HD bool light_contains(const DLight& l, f3 p) {
  f3 lp = mk3(l.pos[0], l.pos[1], l.pos[2]);
  if (l.type == LIGHT_POINT) return norm(sub(p, lp)) < BDPT_EPS_F;
  f3 d = normalize(sub(lp, p));
  return fabsf(dot(d, mk3(l.dir[0], l.dir[1], l.dir[2]))) < BDPT_EPS_F;
}
// sample_pdf's dir_pdf for a point known to be on the light; wi = direction of travel.
BDPT_HD float light_dir_pdf(const DLight& l, f3 wi) {
  if (l.type == LIGHT_POINT) return 0.25f / BDPT_PI_F;
  if (l.type == LIGHT_ENV) return 1.0f / l.area;   // planar density of the emission disk (§9)
  Frame f;
  f.X = mk3(l.fx[0], l.fx[1], l.fx[2]);
  f.Y = mk3(l.fy[0], l.fy[1], l.fy[2]);
  f.Z = mk3(l.fz[0], l.fz[1], l.fz[2]);
  f3 wl = normalize(to_local(f, neg(wi)));
  return cosine_pdf_z(wl.z);
}

BDPT_HD LightSample light_sample_point(const DLight& l, int nlights, Rng& g, f3 p, float* lpp_out) {
  LightSample s;
  f3 rad = mk3(l.rad[0], l.rad[1], l.rad[2]);
  f3 dirv = mk3(l.dir[0], l.dir[1], l.dir[2]);
  float lpp;
  if (l.type == LIGHT_POINT) {
    f3 lp = mk3(l.pos[0], l.pos[1], l.pos[2]);
    f3 d = sub(lp, p);
    f3 wi = normalize(d);
    lpp = 1.0f;
    s.dir_pdf = 0.25f / BDPT_PI_F;
    s.n = neg(wi);
    s.pos = lp;
  } else {
    float sx, sy;
    grid2d(g, &sx, &sy);
    sx = sx - 0.5f;
    sy = sy - 0.5f;
    f3 pt = add(add(mk3(l.pos[0], l.pos[1], l.pos[2]), smul(sx, mk3(l.dx[0], l.dx[1], l.dx[2]))),
                smul(sy, mk3(l.dy[0], l.dy[1], l.dy[2])));
    f3 d = sub(pt, p);
    float cosT = dot(d, dirv);
    float dd = sqrtf(norm2(d));
    f3 wi = divs(d, dd);
    lpp = 1.0f / l.area;
    s.n = dirv;
    s.pos = pt;
    s.dir_pdf = cosine_pdf_z(lz(neg(wi), mk3(l.fz[0], l.fz[1], l.fz[2])));
    if (!(cosT < 0)) rad = splat3(0);
  }
  lpp = lpp / (float)nlights;
  s.alpha = divs(rad, lpp);
  s.zh = zaxis(s.n);
  s.fwd = lpp;
  s.env = false;
  s.delta = false;
  *lpp_out = lpp;
  return s;
}
// sample_Le_point of the environment light: a direction w from sample_L's
// importance sampling; point_pdf = its solid-angle pdf / nL, dir_pdf = the emission disk's planar
// density 1/(pi R^2); the vertex sits at infinity (n = zh = -w).
BDPT_HD LightSample env_sample_point(const SceneView& S, Rng& g, f3 p) {
  LightSample s;
  f3 w;
  float pw;
  const f3 rad = env_sample_dir(S.env, g, &w, &pw);
  const float lpp = pw / (float)S.nlights;
  s.pos = p;
  s.n = neg(w);
  s.zh = s.n;
  s.dir_pdf = 1.0f / S.lights[S.env.light].area;
  s.alpha = divs(rad, lpp);
  s.fwd = lpp;
  s.env = true;
  s.delta = false;
  return s;
}
// The same for a hemisphere or directional light L: w from inf_sample_dir.
BDPT_HD LightSample inf_sample_point(const SceneView& S, const DLight& L, Rng& g, f3 p) {
  LightSample s;
  f3 w;
  float pw;
  const f3 rad = inf_sample_dir(L, g, &w, &pw);
  const float lpp = pw / (float)S.nlights;
  s.pos = p;
  s.n = neg(w);
  s.zh = s.n;
  s.dir_pdf = 1.0f / L.area;
  s.alpha = divs(rad, lpp);
  s.fwd = lpp;
  s.env = true;
  s.delta = L.type == LIGHT_DIR;
  return s;
}

// Camera::generate_ray (camera.cpp:191-212)
BDPT_HD f3 camera_dir(const DCam& c, float x, float y) {
  float rx = (2 * x - 1) * c.tanh_;
  float ry = (2 * y - 1) * c.tanv_;
  float rz = -1;
  f3 w = add(add(smul(rx, mk3(c.c2w[0], c.c2w[1], c.c2w[2])), smul(ry, mk3(c.c2w[3], c.c2w[4], c.c2w[5]))),
             smul(rz, mk3(c.c2w[6], c.c2w[7], c.c2w[8])));
  return normalize(w);
}

struct EyeSample {
  f3 pos, n, zh, alpha;
  float dir_pdf;
  int x, y;
};
// Camera::sample_ray_pdf (camera.cpp:214-248) with cos(acos z) = z.
BDPT_HD EyeSample camera_sample(const DCam& c, int W, int H, f3 p) {
  EyeSample e;
  f3 cam = mk3(c.pos[0], c.pos[1], c.pos[2]);
  f3 wi = sub(cam, p);
  float dist = norm(wi);
  wi = normalize(wi);
  f3 mw = neg(wi);
  f3 wc = add(add(smul(mw.x, mk3(c.w2c[0], c.w2c[1], c.w2c[2])), smul(mw.y, mk3(c.w2c[3], c.w2c[4], c.w2c[5]))),
              smul(mw.z, mk3(c.w2c[6], c.w2c[7], c.w2c[8])));
  wc.z = -wc.z;
  float ct = wc.z;
  float c2 = ct * ct;
  float denom = 4 * c.tanh_ * c.tanv_ / (c2 * c2);
  e.dir_pdf = (dist * dist) / ct;
  e.n = neg(wi);
  float rz = 1.0f / wc.z;
  wc = mk3(wc.x * rz, wc.y * rz, wc.z * rz);
  float fx = ((wc.x / c.tanh_ + 1) * 0.5f) * (float)W;
  float fy = ((wc.y / c.tanv_ + 1) * 0.5f) * (float)H;
  e.x = (fx > -1.0f && fx < (float)W) ? (int)fx : -1;
  e.y = (fy > -1.0f && fy < (float)H) ? (int)fy : -1;
  e.alpha = divs(splat3(1.0f / denom), 1.0f);
  e.pos = cam;
  e.zh = zaxis(e.n);
  return e;
}

// ------------------------------------------------------------------------------------------------
// The thin lens (Camera::generate_ray_for_thin_lens, camera_lens.cpp:22-43), EXT = 3.
// Sub-streams of the lens uniforms: the walk's lens point, and one per camera connection (1, j).
// (0: eye walk, 1: light sample + walk, 2 + i: the fresh light sample of (i, 1), i <= 127.)
enum : uint32_t { RNG_LENS_WALK = 0x100u, RNG_LENS_CONN = 0x200u };
BDPT_HD f3 cam_to_world(const DCam& c, f3 v) {
  return add(add(smul(v.x, mk3(c.c2w[0], c.c2w[1], c.c2w[2])), smul(v.y, mk3(c.c2w[3], c.c2w[4], c.c2w[5]))),
             smul(v.z, mk3(c.c2w[6], c.c2w[7], c.c2w[8])));
}
// pLens = r sqrt(u1) (cos 2 pi u2, sin 2 pi u2, 0) in camera space
BDPT_HD f3 lens_plens(const DCam& c, float u1, float u2) {
  const float r = c.lens_r * sqrtf(u1);
  float cs, sn;
  cos_sin_2pi(u2, &cs, &sn);
  return mk3(r * cs, r * sn, 0.0f);
}
// The lens point of sub-stream `stream` of g's pixel-sample, in camera space. g is taken by value:
// Philox is counter-based, so the point is recomputed wherever it is needed and the caller's stream
// position stays where it was.
BDPT_HD f3 lens_draw(const DCam& c, Rng g, uint32_t stream) {
  rng_stream(g, stream);
  const float u1 = rng_next(g);
  const float u2 = rng_next(g);
  return lens_plens(c, u1, u2);
}
BDPT_HD f3 lens_world(const DCam& c, f3 pl) { return add(mk3(c.pos[0], c.pos[1], c.pos[2]), cam_to_world(c, pl)); }
// The eye ray through raster position (x, y) in [0, 1]^2 from lens point pl: toward the point
// pFocus = ((2x - 1) tanh, (2y - 1) tanv, -1) F of the focal plane. The direction pFocus - pLens is
// formed divided by F, as camera_dir's vector minus pLens / F: the same direction, and one that
// turns into the pinhole's bit for bit as the lens shrinks.
BDPT_HD f3 lens_ray_dir(const DCam& c, float F, f3 pl, float x, float y) {
  const f3 pf = mk3((2 * x - 1) * c.tanh_, (2 * y - 1) * c.tanv_, -1.0f);
  return normalize(cam_to_world(c, sub(pf, divs(pl, F))));
}
// camera_sample from the lens point pl: its expressions with cam -> x_l, the raster position
// taken through the focal plane (q = pLens + (wc / wc.z) F, used as q / F = pLens / F + wc / wc.z).
BDPT_HD EyeSample camera_sample_lens(const DCam& c, float F, int W, int H, f3 pl, f3 p) {
  EyeSample e;
  const f3 xl = lens_world(c, pl);
  f3 wi = sub(xl, p);
  float dist = norm(wi);
  wi = normalize(wi);
  f3 mw = neg(wi);
  f3 wc = add(add(smul(mw.x, mk3(c.w2c[0], c.w2c[1], c.w2c[2])), smul(mw.y, mk3(c.w2c[3], c.w2c[4], c.w2c[5]))),
              smul(mw.z, mk3(c.w2c[6], c.w2c[7], c.w2c[8])));
  wc.z = -wc.z;
  float ct = wc.z;
  float c2 = ct * ct;
  float denom = 4 * c.tanh_ * c.tanv_ / (c2 * c2);
  e.dir_pdf = (dist * dist) / ct;
  e.n = neg(wi);
  float rz = 1.0f / wc.z;
  wc = mk3(wc.x * rz, wc.y * rz, wc.z * rz);
  const float qx = pl.x / F + wc.x, qy = pl.y / F + wc.y;
  float fx = ((qx / c.tanh_ + 1) * 0.5f) * (float)W;
  float fy = ((qy / c.tanv_ + 1) * 0.5f) * (float)H;
  e.x = (fx > -1.0f && fx < (float)W) ? (int)fx : -1;
  e.y = (fy > -1.0f && fy < (float)H) ? (int)fy : -1;
  e.alpha = divs(splat3(1.0f / denom), 1.0f);
  e.pos = xl;
  e.zh = zaxis(e.n);
  return e;
}


// multiple_importance_sampling_weight (bidirection.cpp:121-293) with cached path constants.
// PA: path accessor — e(k) / l(k) return reference vertices E[k] (k >= 2) / L[k] (k >= 1) and
// dE / dL the delta masks; PathsInRegs below (one lane's Paths) or the wavefront vertex store.
// i, j: reference vertex indices; ls: fresh light sample (j == 1); es: camera sample (i == 1);
// dc, dist: normalize(vl - ve) and |vl - ve| of the connection (j >= 1), which are exactly the
// endpoint-step directions the reference recomputes (normalize(-v) == -normalize(v) in IEEE).
template <int EXT = 0, class PA>
BDPT_HD float mis_weight(const SceneView& S, const PA& P, const Vtx* ev, const Vtx* lv, int i, int j,
                         const LightSample& ls, const EyeSample& es, int eye_light, f3 dc, float dist) {
  float ge = 0.0f, gl = 0.0f;
  if (i >= 2) {
    const Vtx& cur = *ev;
    const bool cenv = EXT && is_env(cur);
    float nom;
    if (j == 0) {
      const DLight& EL = S.lights[eye_light];
      float p = EL.type == LIGHT_POINT ? 1.0f
                : (EXT && EL.type == LIGHT_ENV) ? env_pdf_dir(S.env, neg(cur.n)) / (float)S.nlights
                                                : 1.0f / EL.area;
      // §9a: a hemisphere light's density of this direction; and the light choice's 1 / nL on an
      // emitter too (the reference leaves it out, which only one-light scenes forgive), as every
      // other strategy of these kernels that samples the light carries it
      if (EXT >= 2) p = (EL.type == LIGHT_HEMI ? hemi_pdf() : p) / (EL.type == LIGHT_ENV ? 1.0f : (float)S.nlights);
      nom = p * 1.0f;
    } else {
      f3 pzh = j == 1 ? ls.zh : lv->zh;
      f3 dw = neg(dc);   // normalize(E[i] - vl)
      float g = (EXT && j == 1 && ls.env) ? fabsf(dot(dw, cur.n))
                                          : fabsf(lz(dw, pzh) * dot(dw, cur.n)) / (dist * dist);
      float p = j == 1 ? ls.dir_pdf * 1.0f : pdf_b(S.mats[lv->mat], lv->n, pzh, dw) * (EXT ? lv->cq : 1.0f);
      nom = p * g;
    }
    float below = cur.gp;   // G_{i-1}
    if (j == 0 && i >= 3) {  // the step below the emitter uses the light's dir_pdf (:224-232)
      const Vtx v = P.e(i - 1);
      f3 dr;
      const float revg = EXT ? step_gx(v.pos, v.n, false, cur.pos, cur.zh, cenv, &dr)
                             : step_g(v.pos, v.n, cur.pos, cur.zh, &dr);   // g of the step E[i-1] <- E[i]
      f3 dw = cenv ? cur.n : normalize(sub(v.pos, cur.pos));
      // (an env vertex's light — map or, §9a, hemisphere — emits from the disk: planar density 1 / area)
      float dp = (EXT >= 2 && cenv) ? 1.0f / S.lights[eye_light].area : light_dir_pdf(S.lights[eye_light], neg(dw));
      below = mis_horner(((dp * 1.0f) * revg) / v.fwd, !((P.dE >> (i - 2)) & 3u), v.gp);
    }
    // delta(E[i]) || delta(E[i-1]); an escaped camera ray (i = 2) has no camera-connection strategy
    const bool t = !((P.dE >> (i - 1)) & 3u) && !(cenv && i == 2);
    ge = mis_horner(nom / cur.fwd, t, below);
  }
  if (j >= 1) {
    if (EXT && j == 1 && (EXT >= 2 || S.env.light >= 0)) {
      // environment scenes: the light end of (i, 1) is the fresh sample itself; so it
      // is in every scene of the infinite-light kernels, where the term is off for a directional
      // light's sample: no eye subpath ends on a delta direction (§9a)
      f3 dw;
      float g;
      if (ls.env) { dw = dc; g = 1.0f; }
      else g = step_g(ls.pos, ls.n, i == 1 ? es.pos : ev->pos, i == 1 ? es.zh : ev->zh, &dw);
      float p = i <= 1 ? es.dir_pdf * 1.0f : pdf_b(S.mats[ev->mat], ev->n, ev->zh, dw) * ev->cq;
      gl = mis_horner((p * g) / ls.fwd, !(EXT >= 2 && ls.delta), 0.0f);
    } else {
      const Vtx& cur = *lv;   // j == 1: the original L[1], not the fresh sample (quirk 5)
      f3 pzh = i == 1 ? es.zh : ev->zh;
      f3 dw;
      float g;
      if (j >= 2) {   // cur = L[j] = vl: normalize(L[j] - ve) = dc
        dw = dc;
        g = fabsf(lz(dw, pzh) * dot(dw, cur.n)) / (dist * dist);
      } else {
        f3 ppos = i == 1 ? es.pos : ev->pos;
        g = step_g(cur.pos, cur.n, ppos, pzh, &dw);
      }
      float p = i <= 1 ? es.dir_pdf * 1.0f : pdf_b(S.mats[ev->mat], ev->n, pzh, dw) * (EXT ? ev->cq : 1.0f);
      gl = mis_horner((p * g) / cur.fwd, !((P.dL >> (j - 1)) & 3u), cur.gp);
    }
  }
  return 1.0f / ((1.0f + ge) + gl);
}

// Path accessor over one lane's Paths (megakernel, host tests).
template <int MAXV, int EXT>
struct PathsInRegs {
  const Paths<MAXV>& P;
  DeltaMask<MAXV> dE, dL;
  BDPT_HD explicit PathsInRegs(const Paths<MAXV>& p) : P(p), dE(p.dE), dL(p.dL) {}
  BDPT_HD DeltaMask<MAXV> conn_e() const { return P.cE; }   // connectable eye / light vertices
  BDPT_HD DeltaMask<MAXV> conn_l() const { return P.cL; }
  BDPT_HD DeltaMask<MAXV> src_e() const { return P.sE; }    // s = 0 sources
  BDPT_HD Vtx e(int k) const { return vtx_load<EXT>(P.E[k - 2]); }
  BDPT_HD Vtx l(int k) const { return vtx_load<EXT>(P.L[k - 1]); }
};

// The next vertex's throughput alpha = prev_alpha * |cos| * f / pdf (prepare_bidirectional_subpath
// :60-62), formed when its ray is: one f3 live across the traversal instead of alpha, f and pdf
BDPT_HD f3 walk_next_alpha(f3 pa, f3 pn, f3 d, f3 f, float pdf) { return divs(mul(muls(pa, fabsf(dot(pn, d))), f), pdf); }

// The state of one lane's fused eye + light walk between two iterations (walk_step).
template <int MAXV>
struct WalkState {
  f3 ro, rd, prev_n, nalpha;   // the next ray, the previous vertex's normal, the next vertex's throughput
  float rmin, rmax;
  float pv_fwd, pv_gp, pv_q;   // the previous vertex's fwd / prefix / roulette probability
  int i, count, pv_mat;        // reference vertex index, vertices stored on this subpath, previous material
  DeltaMask<MAXV> dm;          // delta mask of this subpath
  DeltaMask<MAXV> cm, em;      // its connectable vertices (cq > 0); the eye subpath's s = 0 sources
  uint32_t lpos;               // the light stream's position after L[1]
  bool light, l1env;           // walking the light subpath; its L[1] is an environment vertex
};

// Starts one pixel-sample's walk: the camera ray (raytrace_pixel's jitter, bidirection.cpp:515-524)
// and the light vertex L[1] with the light walk's first ray (sample_light_ray, :105-118).
template <int MAXV, int EXT = 0>
BDPT_HD void walk_begin(const SceneView& S, const SampleParams& sp, Paths<MAXV>& P, Counters& cnt, Rng& g,
                        WalkState<MAXV>& w, int x, int y, uint32_t sample) {
  rng_init(g, sp.seed, (uint32_t)(x + y * sp.W), sample);
  float px, py;
  grid2d(g, &px, &py);
  px = px + (float)x;
  py = py + (float)y;
  float dx = px / (float)sp.W, dy = py / (float)sp.H;
  const f3 cam = mk3(S.cam.pos[0], S.cam.pos[1], S.cam.pos[2]);
  f3 rd = camera_dir(S.cam, dx, dy);
  // sample_light_ray (bidirection.cpp:105-118), AreaLight/PointLight::sample_Le, on stream 1: the
  // light vertex L[1] and the light walk's first ray, drawn before the eye walk and kept in the path
  // store (read back when the light walk starts), so the ~17 registers of the light sample are not
  // live across the eye walk's traversals (drawing them at the switch instead spilled more).
  bool l1env = false, l1dir = false;   // l1dir: L[1] is on a directional light (§9a)
  float mis_p = 0.0f;  // L[1]'s MIS point density (differs from lpp only for the env light)
  auto sample_light = [&](Rng& gl, f3& lo, f3& ld, f3& ln, f3& alpha1, float& ldp) {
    rng_stream(gl, 1);
    int lid = (int)(rng_next(gl) * (float)S.nlights);
    if (lid >= S.nlights) lid = S.nlights - 1;
    const DLight& L0 = S.lights[lid];
    f3 lrad = mk3(L0.rad[0], L0.rad[1], L0.rad[2]);
    float lpp, mis_dir;
    if (EXT && (L0.type == LIGHT_ENV || (EXT >= 2 && L0.type >= LIGHT_HEMI))) {
      // sample_Le of the environment light: direction by sample_L's importance
      // sampling, origin uniform on the disk of radius R facing -w, tangent to the bounding sphere;
      // a hemisphere or directional light (§9a) the same with its own sample_L
      f3 w;
      float pw;
      if (EXT >= 2 && L0.type != LIGHT_ENV) {
        lrad = inf_sample_dir(L0, gl, &w, &pw);
        l1dir = L0.type == LIGHT_DIR;
      } else {
        lrad = env_sample_dir(S.env, gl, &w, &pw);
        cnt.env_s++;
      }
      const float u1 = rng_next(gl), u2 = rng_next(gl);
      const float r = S.env.rad * sqrtf(u1);
      float c, sn;
      cos_sin_2pi(u2, &c, &sn);
      const Frame wf = make_frame(w);
      lo = add(add(add(mk3(S.env.cx, S.env.cy, S.env.cz), smul(S.env.rad, w)), smul(r * c, wf.X)), smul(r * sn, wf.Y));
      ld = neg(w);
      ln = ld;
      lpp = 1.0f / L0.area;
      ldp = pw;
      mis_p = pw;
      mis_dir = 1.0f / L0.area;
      l1env = true;
    } else if (L0.type == LIGHT_POINT) {
      float z = rng_next(gl) * 2 - 1;
      float sinT = sqrtf(fmaxf(0.0f, 1.0f - z * z));
      float u = rng_next(gl);
      float c, s;
      cos_sin_2pi(u, &c, &s);
      ld = mk3(c * sinT, s * sinT, z);
      lo = mk3(L0.pos[0], L0.pos[1], L0.pos[2]);
      lpp = 1;
      ldp = 0.25f / BDPT_PI_F;
      ln = ld;
      mis_p = lpp;
      mis_dir = ldp;
    } else {
      float sx, sy;
      grid2d(gl, &sx, &sy);
      sx = sx - 0.5f;
      sy = sy - 0.5f;
      lo = add(add(mk3(L0.pos[0], L0.pos[1], L0.pos[2]), smul(sx, mk3(L0.dx[0], L0.dx[1], L0.dx[2]))),
               smul(sy, mk3(L0.dy[0], L0.dy[1], L0.dy[2])));
      f3 dl = cosine_hemi(gl, &ldp);
      Frame lf;
      lf.X = mk3(L0.fx[0], L0.fx[1], L0.fx[2]);
      lf.Y = mk3(L0.fy[0], L0.fy[1], L0.fy[2]);
      lf.Z = mk3(L0.fz[0], L0.fz[1], L0.fz[2]);
      ld = to_world(lf, dl);
      lpp = 1.0f / L0.area;
      ln = mk3(L0.dir[0], L0.dir[1], L0.dir[2]);
      mis_p = lpp;
      mis_dir = ldp;
    }
    lpp = lpp / (float)S.nlights;
    mis_p = mis_p / (float)S.nlights;
    alpha1 = divs(lrad, lpp);
    Vtx v1;
    v1.pos = lo;
    v1.n = ln;
    v1.zh = l1env ? ln : zaxis(ln);
    v1.alpha = alpha1;
    v1.mat = l1env ? ((EXT >= 2 && l1dir) ? (int)MAT_DIRL_V : (int)MAT_ENV_V) : -1;
    v1.gp = 0; v1.cq = 0;
    v1.fwd = mis_p;   // light_constants' L[1] value (set here for the fused walk)
    vtx_store<EXT>(P.L[0], v1);
    P.l1_dir_pdf = mis_dir;
  };
  Rng gl0 = g;
  f3 lo, ld, ln, la1;
  float ldp;
#if defined(BDPT_PHASE_PROF) && defined(__HIP_DEVICE_COMPILE__)
  const unsigned long long tl0 = __builtin_amdgcn_s_memtime();
#endif
  sample_light(gl0, lo, ld, ln, la1, ldp);
#if defined(BDPT_PHASE_PROF) && defined(__HIP_DEVICE_COMPILE__)
  BDPT_WAVE_CLK(cnt.clk_light, __builtin_amdgcn_s_memtime() - tl0);
#endif
  w.lpos = gl0.pos;
  P.l1_d = ld;
  P.l1_pdf = ldp;
  w.l1env = false;   // re-read with the rest when the light walk starts
  // the walk: eye first (camera ray on [nClip, fClip], alpha = 1, pdf = 1, n = d), then light
  w.ro = cam;
  if (EXT >= 3) {
    // §9b: E[1] is the lens point (its two uniforms on a sub-stream of their own: every other draw
    // of the sample is the pinhole kernels'), the ray runs to the focal plane's point of (dx, dy)
    const f3 pl = lens_draw(S.cam, g, RNG_LENS_WALK);
    w.ro = lens_world(S.cam, pl);
    rd = lens_ray_dir(S.cam, sp.focal, pl, dx, dy);
  }
  w.rmin = S.cam.nclip;
  w.rmax = S.cam.fclip;
  w.prev_n = rd;
  w.rd = rd;
  w.nalpha = walk_next_alpha(divs(splat3(1.0f), 1.0f), rd, rd, splat3(1.0f), 1.0f);
  w.i = 2;
  w.count = 0;
  w.dm = 0;
  w.cm = 0;
  w.em = 0;
  w.light = false;
  w.pv_mat = -1;
  w.pv_fwd = 1.0f; w.pv_gp = 0.0f; w.pv_q = 1.0f;
}
// One iteration of the fused walk: trace the next ray, store the vertex it hits (with its MIS
// constants), sample the continuation. Returns true once the light subpath has ended (both
// subpaths and P.nE / P.nL / P.dE / P.dL complete).
template <int MAXV, int LM = 0, int EXT = 0>
BDPT_HD bool walk_step(const SceneView& S, const SampleParams& sp, Paths<MAXV>& P, Counters& cnt, Rng& g,
                       WalkState<MAXV>& w) {
  f3 ro = w.ro, rd = w.rd, prev_n = w.prev_n, nalpha = w.nalpha;
  float rmin = w.rmin, rmax = w.rmax, pv_fwd = w.pv_fwd, pv_gp = w.pv_gp, pv_q = w.pv_q;
  int i = w.i, count = w.count, pv_mat = w.pv_mat;
  DeltaMask<MAXV> dm = w.dm, cm = w.cm, em = w.em;
  bool light = w.light, l1env = w.l1env;
  auto next_alpha = walk_next_alpha;
  bool done = false;
  {
    Hit h;
#if defined(BDPT_PHASE_PROF) && defined(__HIP_DEVICE_COMPILE__)
    const unsigned long long tq0 = __builtin_amdgcn_s_memtime();
#endif
    BDPT_LANE_PROF(cnt, LP_WALK);
    bool end = !trace_closest<LM, kWalkStack>(S, ro, rd, rmin, rmax, h, cnt);
#if defined(BDPT_PHASE_PROF) && defined(__HIP_DEVICE_COMPILE__)
    const unsigned long long tq1 = __builtin_amdgcn_s_memtime();
    BDPT_WAVE_CLK(cnt.clk_walk_trace, tq1 - tq0);
#endif
    if (EXT && end && !light && S.env.light >= 0) {
      // an escaped eye ray ends on the environment light: vertex at infinity in direction rd
      Vtx v;
      v.alpha = nalpha;
      v.pos = ro;
      v.n = neg(rd);
      v.zh = v.n;
      v.mat = MAT_ENV_V;
      v.fwd = 1; v.gp = 1; v.cq = 0;
      // eye_constants of an env vertex: g = 1 toward it, the previous vertex's BSDF density of rd
      // times its roulette probability; no prefix (the j = 0 weight recomputes this step)
      if (count > 0) {
        const f3 pn = EXT ? P.E[count - 1].n : prev_n;
        const int pm = EXT ? vs_mat(P.E[count - 1]) : pv_mat;
        v.fwd = pdf_b(S.mats[pm], pn, pn, rd) * pv_q * 1.0f;
      }
      v.gp = 0.0f;
      em |= DeltaMask<MAXV>(1) << i;   // an s = 0 source (vertex index i = count + 2)
      vtx_store<EXT>(P.E[count++], v);
    }
    if (!end) {
      BDPT_LANE_PROF(cnt, LP_SHADE);
      f3 n;
      int mat;
      shade_hit<LM>(S, h, ro, rd, &n, &mat);
      const DMat M = S.mats[mat];
      const Frame fr = make_frame_hit(n);
      const f3 hit_p = add(ro, muls(rd, h.t));
      Vtx v;
      v.alpha = nalpha;
      v.pos = hit_p;
      v.n = n;
      v.zh = fr.Z;
      v.mat = mat;
      v.fwd = 1; v.gp = EXT ? 1.0f : 0.0f; v.cq = 0;
      VtxS* slot = (light ? P.L + 1 : P.E) + count++;
      if (is_delta(M.type)) dm |= DeltaMask<MAXV>(1) << i;
      if (!light && M.type == MAT_EMISSION) em |= DeltaMask<MAXV>(1) << i;   // an s = 0 source
      // eye_constants / light_constants of this vertex at its creation. The previous vertex is the
      // one just below it on the same subpath (camera: no step; the light vertex L[1] for the
      // light's first hit) and is still in registers: position ro, normal prev_n (shading axis
      // normalize(prev_n), as make_frame / zaxis compute it; an environment L[1] keeps n itself),
      // material, fwd, prefix, roulette probability. The prefix and the connectability need this
      // vertex's own roulette probability, known after its sample_f below (EXT), so they are
      // finished there: gp = horner(((pp * q) * g) / fwd_prev, t, gp_prev), cq = conn ? q : 0.
      const bool conn = M.type == MAT_DIFFUSE && lz(normalize(sub(ro, v.pos)), v.zh) >= 0 && nonzero3(v.alpha);
      const bool first_eye = !light && count == 1;
      // the previous vertex. EXT kernels read it back from the path store (it was stored before
      // this traversal) rather than hold it in registers across the traversal: C5 +1.5%; the
      // reference-only kernels keep the registers (-0.3 .. -1.5% otherwise, profiles/r03_ab_pv_reload.log)
      f3 pn = prev_n;
      int pmat = pv_mat;
      float pfwd = pv_fwd, pgp = pv_gp;
      if (EXT) {
        if (first_eye) {
          pn = rd; pmat = -1; pfwd = 1.0f; pgp = 0.0f;
        } else {
          const VtxS& pvx = light ? P.L[count - 1] : P.E[count - 2];
          pn = pvx.n; pmat = vs_mat(pvx); pfwd = pvx.fwd; pgp = pvx.gp;
        }
      }
      float gp_pp = 0.0f, gp_g = 0.0f;
      if (first_eye) {
        v.fwd = 1.0f * 1.0f;
      } else {
        const bool nx_env = EXT && light && count == 1 && l1env;
        // the previous vertex's shading axis: a surface hit's is its normal (make_frame_hit), the
        // light vertex L[1]'s is zaxis(n) (an environment L[1] keeps n)
        const f3 nx_zh = (nx_env || !(light && count == 1)) ? pn : zaxis(pn);
        f3 dw;
        const float g2 = EXT ? step_gx(v.pos, v.n, false, ro, nx_zh, nx_env, &dw) : step_g(v.pos, v.n, ro, nx_zh, &dw);
        const float p = (light && count == 1) ? P.l1_dir_pdf
                                              : pdf_b(S.mats[pmat], pn, nx_zh, dw) * (EXT ? pv_q : 1.0f);
        v.fwd = p * g2;
        gp_g = EXT ? step_gx(ro, pn, nx_env, v.pos, v.zh, false, &dw) : step_g(ro, pn, v.pos, v.zh, &dw);
        gp_pp = pdf_b(M, v.n, v.zh, dw);
      }
      const bool gp_t = !((dm >> (i - 2)) & 3u);
      auto finish = [&](float q) {   // q: this vertex's roulette probability (1 without roulette)
        v.cq = conn ? (EXT ? q : 1.0f) : 0.0f;
        if (v.cq > 0.0f) cm |= DeltaMask<MAXV>(1) << i;   // connectable (i: this vertex's index)
        v.gp = first_eye ? 0.0f : mis_horner(((EXT ? gp_pp * q : gp_pp) * gp_g) / pfwd, gp_t, pgp);
        pv_mat = v.mat; pv_fwd = v.fwd; pv_gp = v.gp; pv_q = q;
      };
      if (!EXT) finish(1.0f);
      vtx_store<EXT>(*slot, v);
      if (i >= sp.max_depth + 1 || count >= MAXV) {
        end = true;
        if (EXT) {
          finish(1.0f);
          slot->gp = v.gp; slot->cq = v.cq;
        }
      } else {
        f3 wi;
        float pdf;
        const f3 fv = sample_f(M, g, to_local(fr, neg(rd)), &wi, &pdf);
        float q = 1.0f;
        if (EXT && sp.rr && i > BDPT_RR_MIN) {
          // p_keep = min(1, |f| / pdf), PathVertex.q, then coin_flip(p_keep) (bidirection.cpp:87-93)
          q = pdf > 0.0f ? fminf(1.0f, norm(fv) / pdf) : 0.0f;
          slot->gp = q;
          if (!(rng_next(g) < q)) end = true;
        }
        if (EXT) {
          finish(q);
          slot->gp = v.gp; slot->cq = v.cq;
        }
        ro = hit_p;
        rd = normalize(to_world(fr, wi));
        rmin = BDPT_EPS_F;
        rmax = INFINITY;
        prev_n = n;
        nalpha = next_alpha(v.alpha, n, rd, fv, pdf * q);
        i++;
        // A subpath whose throughput is exactly zero (the vertex's f = 0: an emitter, a diffuse
        // surface seen from behind, bsdf.cpp:56-58,99-110) would walk on to the depth cap with
        // alpha = 0: every later vertex has alpha = 0, so no
        // connection can use it (can_connect, make_conn's contrib gate) and no weight of another
        // connection reads it, and the walk's draws come from its own counter stream. Ending it
        // here is output-identical (tests/test_core_cpu.py vs the oracle, which walks on) and
        // saves 3-4% of the walk rays at the north star's 1080p FOV.
        if (!nonzero3(nalpha)) end = true;
      }
#if defined(BDPT_PHASE_PROF) && defined(__HIP_DEVICE_COMPILE__)
      BDPT_WAVE_CLK(cnt.clk_vertex, __builtin_amdgcn_s_memtime() - tq1);
#endif
    }
    if (end) {
      if (light) {
        P.nL = count + 2;
        P.dL = dm;
        P.cL = cm;
        done = true;
      } else {
      P.nE = count + 2;
      P.dE = dm;
      P.cE = cm;
      P.sE = em;
      light = true;
      // the light sample drawn before the eye walk, read back from the path store (not held in
      // registers across the eye walk)
      rng_stream(g, 1);
      g.pos = w.lpos;
      ro = P.L[0].pos; rd = P.l1_d; prev_n = P.L[0].n;
      nalpha = next_alpha(P.L[0].alpha, prev_n, rd, splat3(1.0f), P.l1_pdf);
      const float mis_p = P.L[0].fwd;
      l1env = EXT >= 2 ? vs_mat(P.L[0]) <= (int)MAT_ENV_V : vs_mat(P.L[0]) == (int)MAT_ENV_V;
      rmin = BDPT_EPS_F; rmax = INFINITY;
      i = 2; count = 0; dm = 0; cm = 0;
      // §9a: no eye subpath ends on a directional light. Bit 0 of the light mask (the step from
      // L[1] to the light's own sampling, which only L[2]'s prefix reads) switches that strategy
      // off the way a delta vertex would, and leaves the (i, 1) connections to L[2] alone.
      if (EXT >= 2 && vs_mat(P.L[0]) == (int)MAT_DIRL_V) dm = 1;
      pv_mat = -1; pv_fwd = mis_p; pv_gp = 0.0f; pv_q = 1.0f;   // the light vertex L[1]
      }
    }
  }
  w.ro = ro; w.rd = rd; w.prev_n = prev_n; w.nalpha = nalpha;
  w.rmin = rmin; w.rmax = rmax; w.pv_fwd = pv_fwd; w.pv_gp = pv_gp; w.pv_q = pv_q;
  w.i = i; w.count = count; w.pv_mat = pv_mat; w.dm = dm; w.cm = cm; w.em = em; w.light = light; w.l1env = l1env;
  return done;
}

// Eye and light subpaths of one pixel-sample plus their MIS constants
// (est_radiance_global_illumination, bidirection.cpp:472-488; raytrace_pixel :515-524;
// prepare_bidirectional_subpath :20-102 for both walks). The two walks run as ONE loop: a lane whose
// eye walk ends starts its light walk in the next iteration, so a wave iterates
// max(|E| + |L|) times instead of max |E| + max |L|. The RNG sub-streams (eye walk: 0, light
// sample + walk: 1) make the interleaving invisible in the results.
template <int MAXV, int LM = 0, int EXT = 0>
BDPT_HD void prepare_sample(const SceneView& S, const SampleParams& sp, Paths<MAXV>& P, Counters& cnt, Rng& g,
                            int x, int y, uint32_t sample) {
  WalkState<MAXV> w;
  walk_begin<MAXV, EXT>(S, sp, P, cnt, g, w, x, y, sample);
  while (!walk_step<MAXV, LM, EXT>(S, sp, P, cnt, g, w)) {
  }
}
// What estimate_bidirection_radiance (bidirection.cpp:296-469) computes for pair (i, j) up to its
// visibility test: either nothing (zero contribution), a direct eye-image value (s = 0, no ray),
// or a connection ray on [EPS_F, tmax] whose value (MIS-weighted) counts if it is unoccluded.
enum { CONN_NONE = 0, CONN_DIRECT = 1, CONN_RAY = 2 };
struct Conn {
  f3 o, d;
  float tmax;
  f3 val;      // eye image: ill; light image: ill / ns_aa
  int splat;   // -1: eye image of this sample's pixel; else x + y*W of the t = 1 splat
};

// A vertex that can receive a connection: diffuse (f != 0 only for DiffuseBSDF, bsdf.cpp:52-62),
// viewed from its front side (wo.z >= 0) and carrying throughput.
BDPT_HD bool can_connect(const Vtx& v) { return v.cq > 0.0f; }
// ev_pre / lv_pre: E[i] / L[j] already loaded by the caller (kept across the megakernel's inner
// connection loop), or null.
// ec: environment-table read counters (stats builds), or null.
template <int EXT = 0, class PA>
BDPT_HD int make_conn(const SceneView& S, const SampleParams& sp, const PA& P, Rng& g, int i, int j, Conn& cn,
                      const Vtx* ev_pre = nullptr, const Vtx* lv_pre = nullptr, Counters* ec = nullptr) {
  const f3 cam = mk3(S.cam.pos[0], S.cam.pos[1], S.cam.pos[2]);
  const bool eye_cam = i == 1;
  Vtx ev, lv;
  LightSample ls;
  ls.env = false;
  ls.delta = false;
  EyeSample es;
  es.x = -1; es.y = -1;
  cn.splat = -1;
  if (!eye_cam) ev = ev_pre ? *ev_pre : P.e(i);
  if (j == 0) {
    if (eye_cam) return CONN_NONE;
    if (EXT && is_env(ev)) {   // an escaped eye ray: the environment light contains it (§9)
      f3 c;
      const bool hemi = EXT >= 2 && S.lights[S.env.light].type == LIGHT_HEMI;
      if (hemi) {
        // §9a: the sky above the horizon; an escaped camera ray (i = 2) sees none of it, as the
        // reference's PathTracer looks up only the environment map there
        c = i >= 3 ? hemi_radiance(S.lights[S.env.light], neg(ev.n)) : splat3(0);
      } else {
        c = env_radiance(S.env, neg(ev.n));
        if (ec) ec->env_l++;
      }
      f3 contrib = mul(mul(ev.alpha, splat3(1.0f)), c);
      float w = 0;
      if (norm(contrib) > BDPT_EPS_F) {
        w = mis_weight<EXT>(S, P, &ev, &lv, i, 0, ls, es, S.env.light, splat3(0), 0);
        if (ec && !hemi) ec->env_p++;   // the j = 0 weight's env_pdf_dir
      }
      cn.val = muls(contrib, w);
      return CONN_DIRECT;
    }
    const DMat& M = S.mats[ev.mat];
    if (M.type != MAT_EMISSION) return CONN_NONE;
    f3 c = mk3(M.a[0], M.a[1], M.a[2]);
    if (!(norm(c) > BDPT_EPS_F)) return CONN_NONE;
    int eye_light = -1;
    for (int l = 0; l < S.nlights; l++)
      if ((!EXT || S.lights[l].type != LIGHT_ENV) && (EXT < 2 || S.lights[l].type < LIGHT_ENV) &&
          light_contains(S.lights[l], ev.pos)) { eye_light = l; break; }
    if (eye_light < 0) return CONN_NONE;
    f3 prevp = i == 2 ? cam : P.e(i - 1).pos;
    if (EXT >= 3 && i == 2) prevp = lens_world(S.cam, lens_draw(S.cam, g, RNG_LENS_WALK));   // this sample's walk lens point
    f3 wi = normalize(sub(ev.pos, prevp));
    const DLight& EL = S.lights[eye_light];
    if (!(light_dir_pdf(EL, wi) > 0)) return CONN_NONE;
    c = mk3(EL.rad[0], EL.rad[1], EL.rad[2]);
    f3 contrib = mul(mul(ev.alpha, splat3(1.0f)), c);
    float w = 0;
    if (norm(contrib) > BDPT_EPS_F) w = mis_weight<EXT>(S, P, &ev, &lv, i, 0, ls, es, eye_light, splat3(0), 0);
    cn.val = muls(contrib, w);
    return CONN_DIRECT;
  }
  // Zero-contribution connections (f_eye = 0 or f_light = 0 or zero throughput) end here.
  if (!eye_cam && !can_connect(ev)) return CONN_NONE;
  lv = lv_pre ? *lv_pre : P.l(j);   // j == 1: the original L[1] (MIS quirk); j >= 2: the light endpoint
  if (j >= 2 && !can_connect(lv)) return CONN_NONE;
  f3 vl_pos, vl_n, la;
  // §9b: a camera connection's own lens point (camera space), fresh per j and independent of the walk's
  f3 pl = splat3(0);
  if (EXT >= 3 && eye_cam) pl = lens_draw(S.cam, g, RNG_LENS_CONN + (uint32_t)j);
  if (j == 1) {   // fresh light sample (bidirection.cpp:332-358)
    const f3 epos = eye_cam ? (EXT >= 3 ? lens_world(S.cam, pl) : cam) : ev.pos;
    rng_stream(g, 2u + (uint32_t)i);
    int id = (int)(rng_next(g) * (float)S.nlights);
    if (id >= S.nlights) id = S.nlights - 1;
    if (EXT && S.lights[id].type == LIGHT_ENV) {
      if (eye_cam) return CONN_NONE;   // no camera connection to a vertex at infinity (§9)
      ls = env_sample_point(S, g, epos);
      if (ec) ec->env_s++;
    } else if (EXT >= 2 && S.lights[id].type >= LIGHT_HEMI) {   // hemisphere / directional (§9a)
      if (eye_cam) return CONN_NONE;
      ls = inf_sample_point(S, S.lights[id], g, epos);
    } else {
      float lp;
      ls = light_sample_point(S.lights[id], S.nlights, g, epos, &lp);
    }
    vl_pos = ls.pos; vl_n = ls.n; la = ls.alpha;
  } else {
    vl_pos = lv.pos; vl_n = lv.n; la = lv.alpha;
  }
  f3 ve_pos, ve_n, ea;
  if (eye_cam) {   // camera sample (bidirection.cpp:360-383)
    es = EXT >= 3 ? camera_sample_lens(S.cam, sp.focal, sp.W, sp.H, pl, vl_pos) : camera_sample(S.cam, sp.W, sp.H, vl_pos);
    if (!(es.x >= 0 && es.y >= 0 && es.x < sp.W && es.y < sp.H)) return CONN_NONE;   // not splatted
    ve_pos = es.pos; ve_n = es.n; ea = es.alpha;
  } else {
    ve_pos = ev.pos; ve_n = ev.n; ea = ev.alpha;
  }
  f3 eal = mul(ea, la);
  if (!nonzero3(eal)) return CONN_NONE;
  // One direction serves the f() hemisphere tests, the connection ray and both MIS endpoint steps.
  const bool lenv = EXT && ls.env;
  f3 dc;
  float dist;
  if (lenv) {
    dc = neg(ls.n);   // toward the environment, unbounded
    dist = INFINITY;
  } else {
    dc = sub(vl_pos, ve_pos);
    dist = norm(dc);
    dc = normalize(dc);
  }
  f3 f_eye = splat3(1.0f), f_light = splat3(1.0f);
  if (!eye_cam) {
    if (lz(dc, ev.zh) < 0) return CONN_NONE;   // f_eye = 0 (bsdf.cpp:56-58)
    const DMat& M = S.mats[ev.mat];
    f_eye = divs(mk3(M.a[0], M.a[1], M.a[2]), BDPT_PI_F);
  }
  if (j >= 2) {
    if (lz(neg(dc), lv.zh) < 0) return CONN_NONE;   // f_light = 0
    const DMat& M = S.mats[lv.mat];
    f_light = divs(mk3(M.a[0], M.a[1], M.a[2]), BDPT_PI_F);
  }
  float gg = lenv ? fabsf(dot(ve_n, dc)) : fabsf(dot(vl_n, dc) * dot(ve_n, dc)) / (dist * dist);
  f3 c = mul(muls(f_eye, gg), f_light);
  f3 contrib = mul(eal, c);
  if (!(norm(contrib) > BDPT_EPS_F)) return CONN_NONE;   // w = 0
  float w = mis_weight<EXT>(S, P, &ev, &lv, i, j, ls, es, -1, dc, dist);
  f3 ill = muls(contrib, w);
  cn.o = ve_pos;
  cn.d = dc;
  cn.tmax = dist - BDPT_EPS_F;
  if (eye_cam) {
    cn.val = divs(ill, (float)sp.spp);
    cn.splat = es.x + es.y * sp.W;
  } else {
    cn.val = ill;
  }
  return CONN_RAY;
}

// sink.eye(x, y, v, direct) of a sink that has one: a sink that only takes the light image's splats
// needs none and is not told.
template <class Sink>
BDPT_HD auto sink_eye(Sink& sink, int x, int y, f3 v, bool direct, int) -> decltype(sink.eye(x, y, v, direct), void()) {
  sink.eye(x, y, v, direct);
}
template <class Sink>
BDPT_HD void sink_eye(Sink&, int, int, f3, bool, long) {}

// One pixel-sample, connections resolved in the reference's (i, j) order (host/test use; the
// device kernel defers the connection rays to a wave-compacted queue instead). The sink sees every
// addend: splat(x, y, v) those of the light image, eye(x, y, v, direct), where it has that hook,
// those of eye_sum, as they are added; direct: an s = 0 contribution (CONN_DIRECT), else a
// connection ray that got through.
template <int MAXV, int LM = 0, int EXT = 0, class Sink>
BDPT_HD f3 render_sample(const SceneView& S, const SampleParams& sp, Paths<MAXV>& P, Counters& cnt,
                         int x, int y, uint32_t sample, Sink& sink) {
  Rng g;
  prepare_sample<MAXV, LM, EXT>(S, sp, P, cnt, g, x, y, sample);
  f3 eye_sum = splat3(0);
#if defined(BDPT_STEP_HIST) && !defined(__HIP_DEVICE_COMPILE__)
  if (anyhit_log()) {   // diagnostics: this pixel-sample's connection lists (tools/flush_sim.py)
    const int e[6] = {-1, (int)(uint32_t)P.cE, (int)(uint32_t)P.cL, -2, (int)(uint32_t)P.sE, P.nL};
    anyhit_log()->insert(anyhit_log()->end(), e, e + 6);
  }
#endif
  for (int i = 1; i < P.nE; i++) {
    for (int j = 0; j < P.nL; j++) {
      Conn cn;
      int kind = make_conn<EXT>(S, sp, PathsInRegs<MAXV, EXT>(P), g, i, j, cn);
      if (kind == CONN_DIRECT) {
        eye_sum = add(eye_sum, cn.val);
        sink_eye(sink, x, y, cn.val, true, 0);
      } else if (kind == CONN_RAY) {
#if defined(BDPT_STEP_HIST) && !defined(__HIP_DEVICE_COMPILE__)
        anyhit_tag() = i << 8 | j;
#endif
        if (trace_any<LM>(S, cn.o, cn.d, BDPT_EPS_F, cn.tmax, cnt)) continue;
        if (cn.splat >= 0) {
          sink.splat(cn.splat % sp.W, cn.splat / sp.W, cn.val);
        } else {
          eye_sum = add(eye_sum, cn.val);
          sink_eye(sink, x, y, cn.val, false, 0);
        }
      }
    }
  }
  return eye_sum;
}

}  // namespace bdpt
