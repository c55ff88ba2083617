// tests/native/core_cpu.cpp — TEST ONLY. Compiles the device-side pipeline (bdpt_core.h) and the
// host scene preparation (bdpt_scene.cpp) with g++ so the per-sample arithmetic can be checked
// against the oracle on the CPU before it runs on the GPU. Never linked into the product.
#include <cmath>
#include <cstdio>
#include <vector>

#include "bdpt_core.h"
#include "bdpt_ldsplan.h"
#include "bdpt_scene.h"

using namespace bdpt;

#ifndef CORE_CPU_TRACE_ONLY   // (stack_probe's sanitizer build takes the ray queries alone: a third of the compile time)
// A flat record of fp32 addends: entry k is (pix[k] = x + y * W, rgb[3k..3k+2]). n counts every
// entry offered; only the first cap are stored.
struct AddendRec {
  int* pix;
  float* rgb;
  long long cap, n;
  float vmin;   // the smallest component offered
  void put(int p, f3 v) {
    vmin = fminf(vmin, fminf(v.x, fminf(v.y, v.z)));
    if (pix && n < cap) { pix[n] = p; rgb[3 * n] = v.x; rgb[3 * n + 1] = v.y; rgb[3 * n + 2] = v.z; }
    n++;
  }
};

// What core_cpu_render_rec records beside the frames (tests/_pixelbound.py): the light image's
// splat count per pixel, and on request every splat, every eye-image addend (one connection's
// value, before the 1 / spp factor) and every per-sample eye value (after it).
struct Recorder {
  int* nsplat;   // W * H
  AddendRec splats, eye_addends, eye_samples;
};

struct HostSink {
  std::vector<double>* light;
  int W;
  Recorder* rec = nullptr;
  void splat(int x, int y, f3 v) {
    size_t k = 3 * ((size_t)x + (size_t)y * W);
    (*light)[k] += v.x; (*light)[k + 1] += v.y; (*light)[k + 2] += v.z;
    if (rec) {
      rec->nsplat[x + y * W]++;
      rec->splats.put(x + y * W, v);
    }
  }
};

// render_sample (bdpt_paths.h), statement for statement, with every eye-image addend recorded
// (tests/test_pixel_bounds.py holds the two bit-equal).
template <int MAXV, int LM, int EXT>
static f3 sample_recorded(const SceneView& S, const SampleParams& sp, Paths<MAXV>& P, Counters& cnt, int x, int y,
                          uint32_t sample, HostSink& sink) {
  Rng g;
  prepare_sample<MAXV, LM, EXT>(S, sp, P, cnt, g, x, y, sample);
  f3 eye_sum = splat3(0);
  for (int i = 1; i < P.nE; i++) {
    for (int j = 0; j < P.nL; j++) {
      Conn cn;
      int kind = make_conn<EXT>(S, sp, PathsInRegs<MAXV, EXT>(P), g, i, j, cn);
      if (kind == CONN_DIRECT) {
        eye_sum = add(eye_sum, cn.val);
        sink.rec->eye_addends.put(x + y * sp.W, cn.val);
      } else if (kind == CONN_RAY) {
        if (trace_any<LM>(S, cn.o, cn.d, BDPT_EPS_F, cn.tmax, cnt)) continue;
        if (cn.splat >= 0) sink.splat(cn.splat % sp.W, cn.splat / sp.W, cn.val);
        else {
          eye_sum = add(eye_sum, cn.val);
          sink.rec->eye_addends.put(x + y * sp.W, cn.val);
        }
      }
    }
  }
  return eye_sum;
}

template <int MAXV, int LM, bool EXT>
static int run(const HostScene& hs, int W, int H, int spp, int M, uint64_t seed, int s0, int count,
               const int* pixels, int npix, double* eye, double* light, double* stats, int rr,
               Recorder* rec = nullptr) {
  SceneView S;
  const HostBvh& T = hs.tree(lm_width(LM));
  S.nodes = (const float4*)T.nodes.data();
  S.geom = (const float4*)hs.geom.data();
  S.shade = (const float4*)hs.shade.data();
  S.mats = hs.mats.data();
  S.lights = hs.lights.data();
  S.nlights = (int)hs.lights.size();
  S.root = T.root;
  // LM 1 reads the "LDS copy": on the CPU the same arrays (exercises the LDS-mode tree)
  // LM 2 reads its BFS treelet [0, n_top) from the "LDS copy" (the same array on the CPU)
  S.lnodes = LM == 1 || LM == 2 ? S.nodes : nullptr;
  S.lgeom = LM == 1 || LM == 3 ? S.geom : nullptr;
  S.lshade = LM == 3 ? S.shade : nullptr;
  S.lleaves = hs.leaf_refs.data();
  S.nleaves = (int)hs.leaf_refs.size();
  S.fn = flat_prims(hs, &S.fsph);
  S.ntop = LM == 2 ? T.n_top : 0;
  S.lstack = nullptr;
  S.cam = hs.cam;
  const size_t np = (size_t)hs.env_w * hs.env_h;
  S.env.light = hs.env_light;
  S.env.w = hs.env_w;
  S.env.h = hs.env_h;
  S.env.marg = hs.env.data();
  S.env.cond = hs.env.data() + hs.env_h;
  S.env.pdf = hs.env.data() + hs.env_h + np;
  S.env.rgb = hs.env.data() + hs.env_h + 2 * np;
  S.env.gmarg = hs.env.empty() ? nullptr : (const int*)(hs.env.data() + hs.env_h + 5 * np);
  S.env.gcond = hs.env.empty() ? nullptr : S.env.gmarg + hs.env_gm + 1;
  S.env.gm = hs.env_gm;
  S.env.gc = hs.env_gc;
  S.env.cx = hs.env_c[0]; S.env.cy = hs.env_c[1]; S.env.cz = hs.env_c[2];
  S.env.rad = hs.env_rad;
  SampleParams sp;
  sp.W = W; sp.H = H; sp.spp = spp; sp.max_depth = M; sp.seed = seed;
  sp.rr = rr;
  std::vector<double> lb((size_t)W * H * 3, 0.0);
  HostSink sink{&lb, W, rec};
  Counters cnt = {0, 0, 0, 0, 0, 0};
  Paths<MAXV>* P = new Paths<MAXV>();
  float inv = 1.0f / (float)spp;
  int total = pixels ? npix : W * H;
  for (int q = 0; q < total; q++) {
    int x = pixels ? pixels[2 * q] : q % W, y = pixels ? pixels[2 * q + 1] : q / W;
    for (int s = s0; s < s0 + count; s++) {
      f3 v = rec ? sample_recorded<MAXV, LM, EXT>(S, sp, *P, cnt, x, y, (uint32_t)s, sink)
                 : render_sample<MAXV, LM, EXT>(S, sp, *P, cnt, x, y, (uint32_t)s, sink);
      size_t k = 3 * ((size_t)x + (size_t)y * W);
      if (rec) rec->eye_samples.put(x + y * W, mk3(v.x * inv, v.y * inv, v.z * inv));
      eye[k] += (double)(v.x * inv); eye[k + 1] += (double)(v.y * inv); eye[k + 2] += (double)(v.z * inv);
    }
  }
  delete P;
  for (size_t k = 0; k < lb.size(); k++) light[k] += lb[k];
  if (stats) {
    stats[0] = cnt.closest + cnt.shadow; stats[1] = cnt.closest; stats[2] = cnt.shadow;
    stats[3] = cnt.nodes; stats[4] = cnt.tris; stats[5] = cnt.sphs; stats[6] = cnt.hits;
  }
  return 0;
}

template <int LM, bool EXT>
static int render_maxv(const HostScene& hs, int W, int H, int spp, int M, uint64_t seed, int s0, int count,
                       const int* pixels, int npix, double* eye, double* light, double* stats, int rr,
                       Recorder* rec) {
  int need = M < 1 ? 1 : M;
  if (need <= 5) return run<5, LM, EXT>(hs, W, H, spp, M, seed, s0, count, pixels, npix, eye, light, stats, rr, rec);
  if (need <= 8) return run<8, LM, EXT>(hs, W, H, spp, M, seed, s0, count, pixels, npix, eye, light, stats, rr, rec);
  if (need <= 16) return run<16, LM, EXT>(hs, W, H, spp, M, seed, s0, count, pixels, npix, eye, light, stats, rr, rec);
  if (need <= 32) return run<32, LM, EXT>(hs, W, H, spp, M, seed, s0, count, pixels, npix, eye, light, stats, rr, rec);
  if (need <= 62) return run<62, LM, EXT>(hs, W, H, spp, M, seed, s0, count, pixels, npix, eye, light, stats, rr, rec);
  if (need <= 126) return run<126, LM, EXT>(hs, W, H, spp, M, seed, s0, count, pixels, npix, eye, light, stats, rr, rec);
  return BDPT_E_UNSUPPORTED;
}

template <int LM>
static int render_lm(const bdpt_scene_desc* d, int W, int H, int spp, int M, uint64_t seed, int s0,
                     int count, const int* pixels, int npix, double* eye, double* light, double* stats, int rr,
                     Recorder* rec = nullptr) {
  HostScene hs;
  std::string err;
  int rc = build_host_scene(d, hs, err);
  if (rc) { fprintf(stderr, "core_cpu: %s\n", err.c_str()); return rc; }
  // the kernel selection of bdpt_create: EXT kernels for an environment light or roulette
  if (hs.env_light >= 0 || rr)
    return render_maxv<LM, true>(hs, W, H, spp, M, seed, s0, count, pixels, npix, eye, light, stats, rr, rec);
  return render_maxv<LM, false>(hs, W, H, spp, M, seed, s0, count, pixels, npix, eye, light, stats, rr, rec);
}

// lds_mode 0: the HBM tree (lm_width(0) children per node); 1: the LDS-mode tree (lm_width(1));
// 2: the HBM tree with its BFS treelet read through the LDS path (same array on the CPU); 3: flat list
extern "C" int core_cpu_render(const bdpt_scene_desc* d, int W, int H, int spp, int M, uint64_t seed, int s0,
                               int count, const int* pixels, int npix, double* eye, double* light, double* stats,
                               int lds_mode, int rr) {
  if (lds_mode == 1) return render_lm<1>(d, W, H, spp, M, seed, s0, count, pixels, npix, eye, light, stats, rr);
  if (lds_mode == 2) return render_lm<2>(d, W, H, spp, M, seed, s0, count, pixels, npix, eye, light, stats, rr);
  if (lds_mode == 3) return render_lm<3>(d, W, H, spp, M, seed, s0, count, pixels, npix, eye, light, stats, rr);
  return render_lm<0>(d, W, H, spp, M, seed, s0, count, pixels, npix, eye, light, stats, rr);
}

// core_cpu_render with the addends on record (tests/_pixelbound.py; small frames): nsplat = W * H
// ints, the light image's splats per pixel (added to). Each of the three records is optional (null
// pix: only counted): splats, eye-image addends (a connection's value before the 1 / spp factor) and
// per-sample eye values (after it), as (pix = x + y * W, r, g, b) with room for cap[k] entries;
// n_out[k] = entries offered (> cap[k]: the record is cut short), vmin[k] = the smallest component
// among them (+inf for none): no addend may be negative.
extern "C" int core_cpu_render_rec(const bdpt_scene_desc* d, int W, int H, int spp, int M, uint64_t seed, int s0,
                                   int count, const int* pixels, int npix, double* eye, double* light, double* stats,
                                   int lds_mode, int rr, int* nsplat, int* splat_pix, float* splat_rgb,
                                   int* addend_pix, float* addend_rgb, int* sample_pix, float* sample_rgb,
                                   const long long* cap, long long* n_out, float* vmin) {
  Recorder rec = {nsplat, {splat_pix, splat_rgb, cap[0], 0, INFINITY}, {addend_pix, addend_rgb, cap[1], 0, INFINITY},
                  {sample_pix, sample_rgb, cap[2], 0, INFINITY}};
  int rc;
  if (lds_mode == 1) rc = render_lm<1>(d, W, H, spp, M, seed, s0, count, pixels, npix, eye, light, stats, rr, &rec);
  else if (lds_mode == 2) rc = render_lm<2>(d, W, H, spp, M, seed, s0, count, pixels, npix, eye, light, stats, rr, &rec);
  else if (lds_mode == 3) rc = render_lm<3>(d, W, H, spp, M, seed, s0, count, pixels, npix, eye, light, stats, rr, &rec);
  else rc = render_lm<0>(d, W, H, spp, M, seed, s0, count, pixels, npix, eye, light, stats, rr, &rec);
  n_out[0] = rec.splats.n; n_out[1] = rec.eye_addends.n; n_out[2] = rec.eye_samples.n;
  vmin[0] = rec.splats.vmin; vmin[1] = rec.eye_addends.vmin; vmin[2] = rec.eye_samples.vmin;
  return rc;
}

// What the LDS plan of a launch is chosen from (bdpt_ldsplan.h lds_plan), from the same
// build_host_scene: out8 = {primitive records, bytes of the whole-scene copy (binary tree + geometry),
// bytes of the flat-list copy, the 4-wide tree's BFS treelet candidates (n_top), bytes of one 4-wide
// node, materials, lights, the flat list's length or 0}. infinite_lights: bdpt_params.infinite_lights.
extern "C" int core_cpu_lds_facts(const bdpt_scene_desc* d, int infinite_lights, int* out8) {
  HostScene hs;
  std::string err;
  int rc = build_host_scene(d, hs, err, false, infinite_lights != 0);
  if (rc) return rc;
  const LdsPlan p = lds_plan(hs, -1, 0, 0);   // the two byte counts do not depend on the budget
  out8[0] = hs.nprim;
  out8[1] = (int)p.full_bytes;
  out8[2] = (int)p.flat_bytes;
  out8[3] = hs.tree(lm_width(2)).n_top;
  out8[4] = node_bytes(lm_width(2));
  out8[5] = (int)hs.mats.size();
  out8[6] = (int)hs.lights.size();
  uint32_t sph = 0;
  out8[7] = flat_prims(hs, &sph);
  return 0;
}

// lds_plan itself: out6 = {lm, ntop, n_node4, copy_bytes, flat_bytes, full_bytes}. forced_lm: -1 = none.
// d == null: the HostScene with no primitives (build_host_scene refuses a description of one).
extern "C" int core_cpu_lds_plan(const bdpt_scene_desc* d, int infinite_lights, int forced_lm, long long lds_max,
                                 long long treelet_max, long long* out6) {
  HostScene hs;
  std::string err;
  const int rc = d ? build_host_scene(d, hs, err, false, infinite_lights != 0) : 0;
  if (rc) return rc;
  const LdsPlan p = lds_plan(hs, forced_lm, (size_t)lds_max, (size_t)treelet_max);
  out6[0] = p.lm; out6[1] = p.ntop; out6[2] = p.n_node4;
  out6[3] = (long long)p.copy_bytes; out6[4] = (long long)p.flat_bytes; out6[5] = (long long)p.full_bytes;
  return 0;
}

extern "C" int core_cpu_scene_info(const bdpt_scene_desc* d, int* depth, int* ref_nodes, int* prim_ref) {
  HostScene hs;
  std::string err;
  int rc = build_host_scene(d, hs, err);
  if (rc) return rc;
  *depth = hs.depth;
  *ref_nodes = hs.ref_nodes;
  for (size_t i = 0; i < hs.ref_order.size(); i++) prim_ref[i] = hs.ref_order[i];
  return 0;
}

// The unidirectional PathTracer (bdpt_core.h pt_pixel) for the whole frame: image = W*H*3
// (sampleBuffer), counts = W*H (sampleCountBuffer).
// LDS mode 3's flat primitive run (flat_prims): its length, or 0 when the leaves are not one run
extern "C" int core_cpu_flat_prims(const bdpt_scene_desc* d, uint32_t* sph_mask) {
  HostScene hs;
  std::string err;
  if (build_host_scene(d, hs, err) != BDPT_OK) return -1;
  return flat_prims(hs, sph_mask);
}

extern "C" int core_cpu_pt_render(const bdpt_scene_desc* d, int W, int H, int spp, int M, uint64_t seed,
                                  int ns_area_light, int batch, float tol, int hemisphere, double lens,
                                  double focal, double* image, int* counts) {
  HostScene hs;
  std::string err;
  int rc = build_host_scene(d, hs, err, true);
  if (rc) { fprintf(stderr, "core_cpu: %s\n", err.c_str()); return rc; }
  SceneView S;
  const HostBvh& T = hs.tree(lm_width(0));
  S.nodes = (const float4*)T.nodes.data();
  S.geom = (const float4*)hs.geom.data();
  S.shade = (const float4*)hs.shade.data();
  S.mats = hs.mats.data();
  S.lights = hs.lights.data();
  S.nlights = (int)hs.lights.size();
  S.root = T.root;
  S.lnodes = nullptr;
  S.lgeom = nullptr;
  S.lshade = nullptr;
  S.lleaves = nullptr;
  S.nleaves = 0;
  S.fn = 0;
  S.fsph = 0;
  S.ntop = 0;
  S.lstack = nullptr;
  S.cam = hs.cam;
  const size_t np = (size_t)hs.env_w * hs.env_h;
  S.env.light = hs.env_light;
  S.env.w = hs.env_w;
  S.env.h = hs.env_h;
  S.env.marg = hs.env.data();
  S.env.cond = hs.env.data() + hs.env_h;
  S.env.pdf = hs.env.data() + hs.env_h + np;
  S.env.rgb = hs.env.data() + hs.env_h + 2 * np;
  S.env.gmarg = hs.env.empty() ? nullptr : (const int*)(hs.env.data() + hs.env_h + 5 * np);
  S.env.gcond = hs.env.empty() ? nullptr : S.env.gmarg + hs.env_gm + 1;
  S.env.gm = hs.env_gm;
  S.env.gc = hs.env_gc;
  S.env.cx = hs.env_c[0]; S.env.cy = hs.env_c[1]; S.env.cz = hs.env_c[2];
  S.env.rad = hs.env_rad;
  PtParams pp;
  pp.W = W; pp.H = H; pp.spp = spp; pp.max_depth = M; pp.seed = seed;
  pp.ns_area_light = ns_area_light; pp.batch = batch; pp.hemisphere = hemisphere; pp.tol = tol;
  pp.lens_radius = (float)lens; pp.focal_distance = (float)focal;
  Counters cnt = {0, 0, 0, 0, 0, 0};
  for (int y = 0; y < H; y++)
    for (int x = 0; x < W; x++) {
      const size_t k = (size_t)x + (size_t)y * W;
      const f3 v = pt_pixel<0>(S, pp, cnt, x, y, counts + k);
      image[3 * k] = v.x; image[3 * k + 1] = v.y; image[3 * k + 2] = v.z;
    }
  return 0;
}

// the device tree's depth and node count (binary tree before the 4-wide collapse), as built under
// the current BDPT_BVH / BDPT_SAH_* settings
extern "C" int core_cpu_dev_tree(const bdpt_scene_desc* d, int* depth, int* nodes) {
  HostScene hs;
  std::string err;
  int rc = build_host_scene(d, hs, err);
  if (rc) return rc;
  *depth = hs.dev_depth;
  *nodes = hs.dev_nodes;
  return 0;
}

#endif   // CORE_CPU_TRACE_ONLY

// Closest hits of the device traversal (lds_mode 0, 1 or 2) against a brute-force loop over every
// primitive with the same tests and tie rule, for n rays with origins spread over the scene's box and
// directions with exact zero (and -0) components: axis-aligned and in the coordinate planes (a zero
// component once gave an infinite inverse and NaN / -inf plane distances, bdpt_core.h safe_inv).
// Returns the number of rays whose hit (primitive, t) differs; *hits = rays that hit something.
template <int LM>
static SceneView trace_view(const HostScene& hs) {
  SceneView S = {};
  const HostBvh& T = hs.tree(lm_width(LM));
  S.nodes = (const float4*)T.nodes.data();
  S.geom = (const float4*)hs.geom.data();
  S.shade = (const float4*)hs.shade.data();
  S.root = T.root;
  S.lnodes = LM == 1 || LM == 2 ? S.nodes : nullptr;
  S.lgeom = LM == 1 ? S.geom : nullptr;
  S.ntop = LM == 2 ? T.n_top : 0;
  return S;
}

template <int LM>
static int trace_check_lm(const HostScene& hs, int n, uint64_t seed, int* hits) {
  const SceneView S = trace_view<LM>(hs);
  const int np = (int)(hs.geom.size() / 12);
  float lo[3] = {1e30f, 1e30f, 1e30f}, hi[3] = {-1e30f, -1e30f, -1e30f};
  for (int i = 0; i < np; i++) {
    const float* g = &hs.geom[12 * i];
    const bool sph = __float_as_int(hs.shade[12 * i + 10]) != 0;
    for (int v = 0; v < (sph ? 1 : 3); v++)
      for (int k = 0; k < 3; k++) {
        const float e = v == 0 ? 0.0f : (v == 1 ? g[3 + k] : g[6 + k]);
        const float x = g[k] + e;
        lo[k] = fminf(lo[k], x); hi[k] = fmaxf(hi[k], x);
      }
  }
  uint64_t st = seed;
  auto rnd = [&]() { st = st * 6364136223846793005ull + 1442695040888963407ull; return (float)((st >> 40) & 0xffffff) / 16777216.0f; };
  int bad = 0;
  *hits = 0;
  Counters cnt = {};
  for (int q = 0; q < n; q++) {
    f3 o = mk3(lo[0] + (hi[0] - lo[0]) * rnd(), lo[1] + (hi[1] - lo[1]) * rnd(), lo[2] + (hi[2] - lo[2]) * rnd());
    float dv[3] = {rnd() * 2 - 1, rnd() * 2 - 1, rnd() * 2 - 1};
    const int pat = q % 7;   // which components are zeroed: one axis (3), two axes (3), none
    if (pat < 3) dv[pat] = (q & 8) ? -0.0f : 0.0f;
    else if (pat < 6) { dv[(pat + 1) % 3] = 0.0f; dv[(pat + 2) % 3] = (q & 8) ? -0.0f : 0.0f; }
    f3 d = normalize(mk3(dv[0], dv[1], dv[2]));
    if (!(norm2(d) > 0.5f)) continue;
    Hit h;
    trace_closest<LM, kWalkStack>(S, o, d, 1e-5f, 1e30f, h, cnt);
    float bt = 1e30f;
    int bp = -1, bk = -1;
    for (int i = 0; i < np; i++) {
      const float4* g = S.geom + 3 * i;
      float t, b1, b2;
      bool ok;
      int key;
      if (__float_as_int(hs.shade[12 * i + 10]) != 0) {
        ok = sph_test(g[0], o, d, 1e-5f, bt, &t);
        key = __float_as_int(g[1].x);
      } else {
        ok = tri_test(g[0], g[1], g[2], o, d, 1e-5f, bt, &t, &b1, &b2);
        key = __float_as_int(g[2].y);
      }
      if (ok && (t < bt || key > bk)) { bt = t; bp = i; bk = key; }
    }
    if (bp >= 0) (*hits)++;
    // compared as scene primitives: a primitive that spatial splits reference from two leaves has a
    // record at two positions, and either may be the one a walk or the loop meets first
    const int sp = bp >= 0 ? hs.prim_ref[bp] : -1, hp = h.prim >= 0 ? hs.prim_ref[h.prim] : -1;
    if (sp != hp || (bp >= 0 && bt != h.t)) bad++;
  }
  return bad;
}

extern "C" int core_cpu_trace_check(const bdpt_scene_desc* d, int lds_mode, int n, uint64_t seed, int* hits) {
  HostScene hs;
  std::string err;
  if (build_host_scene(d, hs, err) != BDPT_OK) return -1;
  if (lds_mode == 1) return trace_check_lm<1>(hs, n, seed, hits);
  return lds_mode == 2 ? trace_check_lm<2>(hs, n, seed, hits) : trace_check_lm<0>(hs, n, seed, hits);
}

// bdpt_trace_rays (k_trace_rays) on the CPU: rays = n x (o, d, tmin, tmax); closest hit t and the
// primitive's scene index (-1: none), or for any_hit whether anything lies in [tmin, tmax]
template <int LM>
static void trace_rays_lm(const HostScene& hs, const float* rays, int n, int any_hit, float* out_t, int* out_prim,
                          unsigned* visits = nullptr) {
  const SceneView S = trace_view<LM>(hs);
  for (int i = 0; i < n; i++) {
    Counters c = {};
    const float* r = rays + 8 * (size_t)i;
    const f3 o = mk3(r[0], r[1], r[2]), d = mk3(r[3], r[4], r[5]);
    if (any_hit) {
      const bool h = trace_any<LM, kConnStack>(S, o, d, r[6], r[7], c);
      out_t[i] = h ? 0.0f : INFINITY;
      out_prim[i] = h ? 0 : -1;
    } else {
      Hit h;
      const bool ok = trace_closest<LM, kWalkStack>(S, o, d, r[6], r[7], h, c);
      out_t[i] = ok ? h.t : INFINITY;
      out_prim[i] = ok ? hs.prim_ref[h.prim] : -1;
    }
    if (visits) visits[i] = c.nodes;
  }
}

extern "C" int core_cpu_trace_rays(const bdpt_scene_desc* d, int lds_mode, const float* rays, int n, int any_hit,
                                   float* out_t, int* out_prim) {
  HostScene hs;
  std::string err;
  if (build_host_scene(d, hs, err) != BDPT_OK) return -1;
  if (lds_mode == 1) trace_rays_lm<1>(hs, rays, n, any_hit, out_t, out_prim);
  else if (lds_mode == 2) trace_rays_lm<2>(hs, rays, n, any_hit, out_t, out_prim);
  else trace_rays_lm<0>(hs, rays, n, any_hit, out_t, out_prim);
  return 0;
}

// The same over one scene build for LDS modes 0, 1, 2 and both query kinds, with each ray's node
// visits (Counters::nodes: a node step counts its W child slots): out_prim and visits hold n entries
// per (mode, query) at ((2 * mode + any_hit) * n), info 5 per mode = W, the nodes and wide-node
// levels of the tree that mode traverses, the traversal stack entries that tree needs, kStackMax
// (tests/native/stack_probe.cpp)
extern "C" int core_cpu_trace_visits(const bdpt_scene_desc* d, const float* rays, int n, int* out_prim,
                                     unsigned* visits, int* info) {
  HostScene hs;
  std::string err;
  if (build_host_scene(d, hs, err) != BDPT_OK) return -1;
  std::vector<float> t(n);
  for (int lm = 0; lm < 3; lm++) {
    const int W = lm_width(lm);
    const HostBvh& T = hs.tree(W);
    int* f = info + 5 * lm;
    f[0] = W;
    f[1] = (int)(T.nodes.size() / ((size_t)4 * node_f4(W)));
    f[2] = T.depth + 1;
    f[3] = (W - 1) * (T.depth + 1) + 2;
    f[4] = kStackMax;
    for (int any = 0; any < 2; any++) {
      const size_t at = (size_t)(2 * lm + any) * n;
      if (lm == 1) trace_rays_lm<1>(hs, rays, n, any, t.data(), out_prim + at, visits + at);
      else if (lm == 2) trace_rays_lm<2>(hs, rays, n, any, t.data(), out_prim + at, visits + at);
      else trace_rays_lm<0>(hs, rays, n, any, t.data(), out_prim + at, visits + at);
    }
  }
  return 0;
}

#if defined(BDPT_STEP_HIST)
// diagnostics (tools/anyhit_probe.py): collect the any-hit rays of the following renders (max_rays,
// 0 = stop), then copy up to max_rays of them out; returns the number collected
static std::vector<float> g_rays;
extern "C" void core_cpu_ray_dump(int on) {
  g_rays.clear();
  ray_dump() = on == 1 ? &g_rays : nullptr;
}
extern "C" long long core_cpu_ray_dump_get(float* out, long long max_rays) {
  const long long n = std::min<long long>(max_rays, (long long)g_rays.size() / 8);
  std::copy(g_rays.begin(), g_rays.begin() + 8 * n, out);
  return (long long)g_rays.size() / 8;
}
// diagnostics (tools/step_hist.py): node steps per closest-hit query since the last call
extern "C" void core_cpu_step_hist(unsigned long long* out1024) {
  for (int k = 0; k < 1024; k++) { out1024[k] = step_hist()[k]; step_hist()[k] = 0; }
}
#endif
