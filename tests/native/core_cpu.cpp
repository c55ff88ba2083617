// tests/native/core_cpu.cpp — TEST ONLY. Compiles the device-side pipeline (bdpt_core.h) and the
// host scene preparation (bdpt_scene.cpp) with g++ so the per-sample arithmetic can be checked
// against the oracle on the CPU before it runs on the GPU. Never linked into the product.
#include <cmath>
#include <cstdio>
#include <vector>

#include "core_cpu_host.h"

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

// What core_cpu_render_rec records beside the frames and the splat counts (tests/_pixelbound.py),
// each on request: every splat, every eye-image addend (one connection's value, before the 1 / spp
// factor) and every per-sample eye value (after it).
struct Recorder {
  AddendRec splats, eye_addends, eye_samples;
};

struct RecSink : HostSink {
  Recorder* rec = nullptr;
  void splat(int x, int y, f3 v) {
    HostSink::splat(x, y, v);
    rec->splats.put(x + y * W, v);
  }
  void eye(int x, int y, f3 v, bool s0) {
    HostSink::eye(x, y, v, s0);
    rec->eye_addends.put(x + y * W, v);
  }
  void sample(int x, int y, f3 v) { rec->eye_samples.put(x + y * W, v); }
};

// lds_mode: host_render's (core_cpu_host.h). stats: 7 doubles, the first of host_render's. One thread.
extern "C" int core_cpu_render(const bdpt_scene_desc* d, int W, int H, int spp, int M, uint64_t seed, int s0,
                               int count, const int* pixels, int npix, double* eye, double* light, double* stats,
                               int lds_mode, int rr) {
  const Job J = {W, H, spp, M, s0, count, rr, seed, pixels, npix, eye, light, stats, 7};
  return host_render<1>("core_cpu", d, 0, lds_mode, J, HostSink());
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
  Recorder rec = {{splat_pix, splat_rgb, cap[0], 0, INFINITY}, {addend_pix, addend_rgb, cap[1], 0, INFINITY},
                  {sample_pix, sample_rgb, cap[2], 0, INFINITY}};
  RecSink sink;
  sink.nsplat = nsplat;
  sink.rec = &rec;
  const Job J = {W, H, spp, M, s0, count, rr, seed, pixels, npix, eye, light, stats, 7};
  const int rc = host_render<1>("core_cpu", d, 0, lds_mode, J, sink);
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

// host_view (core_cpu_host.h) of the description at lds_mode, that is scene_view (bdpt_scene.h) plus
// the "LDS copies" (tests/test_scene_view.py). out19 = {the width of the tree S.nodes points into (2,
// 4, 0: neither), root, ntop, nleaves, fn, env.light, the offsets in floats from HostScene::env of
// env.marg, cond, pdf, rgb, gmarg, gcond (-1: null), whether lnodes, lgeom, lshade are set, and
// to hold them against: lm_width(lds_mode), and from the HostScene itself the root of the tree of
// that width, the n_top of LM 2's tree, its leaves}.
extern "C" int core_cpu_view_facts(const bdpt_scene_desc* d, int infinite_lights, int lds_mode, int* out19) {
  HostScene hs;
  std::string err;
  const int rc = build_host_scene(d, hs, err, false, infinite_lights != 0);
  if (rc) return rc;
  const SceneView S = host_view(hs, lds_mode);
  out19[0] = (const float*)S.nodes == hs.bvh2.nodes.data() ? 2 : (const float*)S.nodes == hs.bvh4.nodes.data() ? 4 : 0;
  out19[1] = S.root; out19[2] = S.ntop; out19[3] = S.nleaves; out19[4] = S.fn; out19[5] = S.env.light;
  const void* env[6] = {S.env.marg, S.env.cond, S.env.pdf, S.env.rgb, S.env.gmarg, S.env.gcond};
  for (int k = 0; k < 6; k++) out19[6 + k] = env[k] ? (int)((const float*)env[k] - hs.env.data()) : -1;
  out19[12] = S.lnodes != nullptr; out19[13] = S.lgeom != nullptr; out19[14] = S.lshade != nullptr;
  out19[15] = lm_width(lds_mode);
  out19[16] = hs.tree(lm_width(lds_mode)).root;
  out19[17] = hs.tree(lm_width(2)).n_top;
  out19[18] = (int)hs.leaf_refs.size();
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

// LDS mode 3's flat primitive run (flat_prims): its length, or 0 when the leaves are not one run
extern "C" int core_cpu_flat_prims(const bdpt_scene_desc* d, uint32_t* sph_mask) {
  HostScene hs;
  std::string err;
  if (build_host_scene(d, hs, err) != BDPT_OK) return -1;
  return flat_prims(hs, sph_mask);
}

// The unidirectional PathTracer (bdpt_core.h pt_pixel) for the whole frame: image = W*H*3
// (sampleBuffer), counts = W*H (sampleCountBuffer).
extern "C" int core_cpu_pt_render(const bdpt_scene_desc* d, int W, int H, int spp, int M, uint64_t seed,
                                  int ns_area_light, int batch, float tol, int hemisphere, double lens,
                                  double focal, double* image, int* counts) {
  HostScene hs;
  std::string err;
  int rc = build_host_scene(d, hs, err, true);
  if (rc) { fprintf(stderr, "core_cpu: %s\n", err.c_str()); return rc; }
  const SceneView S = host_view(hs, 0);
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
static int trace_check_lm(const HostScene& hs, int n, uint64_t seed, int* hits) {
  const SceneView S = host_view(hs, LM);
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
  const SceneView S = host_view(hs, LM);
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
