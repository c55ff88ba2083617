// tests/native/core_cpu_host.h — TEST ONLY. What the CPU builds of the device code (core_cpu*.cpp)
// share: the SceneView of a HostScene on the host and, unless CORE_CPU_TRACE_ONLY is defined (the
// ray-query builds: a third of the compile time), the render loop over render_sample
// (bdpt_paths.h). Never linked into the product.
#pragma once

#include "bdpt_core.h"
#include "bdpt_ldsplan.h"
#include "bdpt_scene.h"

namespace bdpt {

// scene_view (bdpt_scene.h) over the scene's own vectors. The "LDS copies" of mode LM are the same
// arrays on the CPU: LM 1 reads the whole LDS-mode tree and the geometry through them, LM 2 its BFS
// treelet [0, n_top), LM 3 the geometry and the shading records.
inline SceneView host_view(const HostScene& hs, int LM) {
  SceneView S = scene_view(hs, {hs.bvh2.nodes.data(), hs.bvh4.nodes.data(), hs.geom.data(), hs.shade.data(),
                                hs.mats.data(), hs.lights.data(), hs.leaf_refs.data(), hs.env.data()}, LM);
  S.lnodes = LM == 1 || LM == 2 ? S.nodes : nullptr;
  S.lgeom = LM == 1 || LM == 3 ? S.geom : nullptr;
  S.lshade = LM == 3 ? S.shade : nullptr;
  S.ntop = LM == 2 ? hs.tree(lm_width(LM)).n_top : 0;
  return S;
}

}  // namespace bdpt

#ifndef CORE_CPU_TRACE_ONLY
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

namespace bdpt {

// The sink of a host render (render_sample's Sink, plus sample() for the loop below): the light
// image of one thread, and on request the splats per pixel, the smallest component of any addend
// and the s = 0 contributions. A sink that records more derives from it (core_cpu.cpp RecSink).
struct HostSink {
  int* nsplat = nullptr;   // W * H, added to: the light image's splats per pixel (one thread only)
  float* vmin = nullptr;   // lowered to the smallest component of any eye or light addend (one thread only)
  std::vector<double>* light = nullptr;   // set by host_render: this thread's light frame, W wide
  int W = 0;
  double direct[2] = {0, 0};   // s = 0 strategies that returned a value, the sum of their components' magnitudes
  void note(f3 v) { if (vmin) *vmin = fminf(*vmin, fminf(v.x, fminf(v.y, v.z))); }
  void splat(int x, int y, f3 v) {
    size_t k = 3 * ((size_t)x + (size_t)y * W);
    (*light)[k] += v.x; (*light)[k + 1] += v.y; (*light)[k + 2] += v.z;
    if (nsplat) nsplat[x + y * W]++;
    note(v);
  }
  void eye(int, int, f3 v, bool s0) {
    note(v);
    if (s0) {
      direct[0] += 1;
      direct[1] += (double)fabsf(v.x) + (double)fabsf(v.y) + (double)fabsf(v.z);
    }
  }
  void sample(int, int, f3) {}   // a pixel-sample's eye value, after the 1 / spp factor
};

// One render: samples [s0, s0 + count) of the frame, or of the npix pixels (x, y) at pixels.
struct Job {
  int W, H, spp, M, s0, count, rr;
  uint64_t seed;
  const int* pixels;
  int npix;
  double *eye, *light;    // W * H * 3, added to
  double* stats;          // null, or nstats doubles of the ten below (host_render)
  int nstats;
  int threads = 1;
  float lens_r = 0.0f, focal = 4.7f;   // the thin lens (flavour 3 with lens_r > 0)
};

template <int MAXV, int LM, int EXT, class Sink>
int run(const HostScene& hs, const Job& J, const Sink& proto) {
  SceneView S = host_view(hs, LM);
  S.cam.lens_r = J.lens_r;
  SampleParams sp;
  sp.W = J.W; sp.H = J.H; sp.spp = J.spp; sp.max_depth = J.M; sp.seed = J.seed;
  sp.rr = J.rr;
  sp.focal = J.focal;
  const int total = J.pixels ? J.npix : J.W * J.H;
  const int nt = J.threads < 1 ? 1 : (J.threads > total ? (total > 0 ? total : 1) : J.threads);
  const float inv = 1.0f / (float)J.spp;
  // thread t renders the pixels [total * t / nt, total * (t + 1) / nt) in order into the shared eye
  // frame (a pixel belongs to one thread) and its own light frame; the light frames are added in
  // thread order, so one thread gives the summation order of a plain loop
  std::vector<std::vector<double>> lb(nt, std::vector<double>((size_t)J.W * J.H * 3, 0.0));
  std::vector<Counters> cnts(nt);
  std::vector<Sink> sinks(nt, proto);
  auto work = [&](int t) {
    Sink& sink = sinks[t];
    sink.light = &lb[t];
    sink.W = J.W;
    Counters cnt = {0, 0, 0, 0, 0, 0};
    Paths<MAXV>* P = new Paths<MAXV>();
    for (int q = (int)((long long)total * t / nt); q < (int)((long long)total * (t + 1) / nt); q++) {
      const int x = J.pixels ? J.pixels[2 * q] : q % J.W, y = J.pixels ? J.pixels[2 * q + 1] : q / J.W;
      for (int s = J.s0; s < J.s0 + J.count; s++) {
        const f3 v = render_sample<MAXV, LM, EXT>(S, sp, *P, cnt, x, y, (uint32_t)s, sink);
        const f3 vs = mk3(v.x * inv, v.y * inv, v.z * inv);
        sink.sample(x, y, vs);
        const size_t k = 3 * ((size_t)x + (size_t)y * J.W);
        J.eye[k] += (double)vs.x; J.eye[k + 1] += (double)vs.y; J.eye[k + 2] += (double)vs.z;
      }
    }
    delete P;
    cnts[t] = cnt;
  };
  if (nt == 1) {   // no std::thread: libcorecpu.so is linked without -lpthread
    work(0);
  } else {
    std::vector<std::thread> th;
    for (int t = 0; t < nt; t++) th.emplace_back(work, t);
    for (std::thread& t : th) t.join();
  }
  for (int t = 0; t < nt; t++)
    for (size_t k = 0; k < lb[t].size(); k++) J.light[k] += lb[t][k];
  if (J.stats) {
    double st[10] = {0};
    for (int t = 0; t < nt; t++) {
      const Counters& c = cnts[t];
      st[0] += (double)c.closest + c.shadow; st[1] += c.closest; st[2] += c.shadow; st[3] += c.nodes;
      st[4] += c.tris; st[5] += c.sphs; st[6] += c.hits;
      st[8] += sinks[t].direct[0]; st[9] += sinks[t].direct[1];
    }
    st[7] = EXT;   // the kernel flavour that rendered
    std::memcpy(J.stats, st, (size_t)J.nstats * sizeof(double));   // the caller's array may hold no more
  }
  return 0;
}

template <int LM, int EXT, class Sink>
int render_maxv(const HostScene& hs, const Job& J, const Sink& proto) {
  switch (maxv_class(J.M)) {
    case 5: return run<5, LM, EXT>(hs, J, proto);
    case 8: return run<8, LM, EXT>(hs, J, proto);
    case 16: return run<16, LM, EXT>(hs, J, proto);
    case 32: return run<32, LM, EXT>(hs, J, proto);
    case 62: return run<62, LM, EXT>(hs, J, proto);
    case 126: return run<126, LM, EXT>(hs, J, proto);
  }
  return BDPT_E_UNSUPPORTED;
}

// The render of a description as bdpt_create would set it up: the scene checks (a refusal goes to
// stderr as "who: message"), the kernel flavour (kernel_flavour; a library compiles those up to
// EXT_MAX), the depth class, and lds_mode: 0 the HBM tree (lm_width(0) children per node), 1 the
// LDS-mode tree (lm_width(1)), 2 the HBM tree with its BFS treelet read through the LDS path, 3 the
// flat list. Each thread's sink is a copy of proto. stats: {rays, closest-hit queries, any-hit
// queries, node steps, triangle tests, sphere tests, hits, the flavour that rendered, s = 0
// strategies that returned a value, the sum of those values' magnitudes}.
template <int EXT_MAX, class Sink>
int host_render(const char* who, const bdpt_scene_desc* d, int infinite_lights, int lds_mode, const Job& J,
                const Sink& proto) {
  HostScene hs;
  std::string err;
  const int rc = build_host_scene(d, hs, err, false, infinite_lights != 0);
  if (rc) { fprintf(stderr, "%s: %s\n", who, err.c_str()); return rc; }
  const int ext = kernel_flavour(hs, J.rr != 0, J.lens_r > 0.0f);
  return dispatch_lm(lds_mode, [&](auto LM) -> int {
    constexpr int lm = decltype(LM)::value;
    if constexpr (EXT_MAX >= 3) if (ext == 3) return render_maxv<lm, 3>(hs, J, proto);
    if constexpr (EXT_MAX >= 2) if (ext == 2) return render_maxv<lm, 2>(hs, J, proto);
    if (ext == 1) return render_maxv<lm, 1>(hs, J, proto);
    if (ext == 0) return render_maxv<lm, 0>(hs, J, proto);
    return BDPT_E_UNSUPPORTED;
  });
}

}  // namespace bdpt
#endif   // CORE_CPU_TRACE_ONLY
