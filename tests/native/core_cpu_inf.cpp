// tests/native/core_cpu_inf.cpp — TEST ONLY. The device-side BDPT pipeline (bdpt_core.h) and the
// host scene preparation (bdpt_scene.cpp) compiled with g++, like core_cpu.cpp, with the
// bdpt_params.infinite_lights opt-in: the yardstick of the GPU's infinite-light
// kernels and the renderer of the convergence tests. Never linked into the product.
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "bdpt_core.h"
#include "bdpt_scene.h"

using namespace bdpt;

namespace {

struct HostSink {
  std::vector<double>* light;
  int W;
  int* nsplat = nullptr;   // the light image's splats per pixel (core_cpu_inf_render_counts)
  float* vmin = nullptr;   // the smallest component of any addend so far
  void splat(int x, int y, f3 v) {
    size_t k = 3 * ((size_t)x + (size_t)y * W);
    (*light)[k] += v.x; (*light)[k + 1] += v.y; (*light)[k + 2] += v.z;
    if (nsplat) nsplat[x + y * W]++;
    note(v);
  }
  void note(f3 v) { if (vmin) *vmin = fminf(*vmin, fminf(v.x, fminf(v.y, v.z))); }
};

template <int LM>
SceneView view_of_host(const HostScene& hs) {
  SceneView S;
  const HostBvh& T = hs.tree(lm_width(LM));
  S.nodes = (const float4*)T.nodes.data();
  S.geom = (const float4*)hs.geom.data();
  S.shade = (const float4*)hs.shade.data();
  S.mats = hs.mats.data();
  S.lights = hs.lights.data();
  S.nlights = (int)hs.lights.size();
  S.root = T.root;
  // the "LDS copies" are the same arrays on the CPU (core_cpu.cpp)
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
  S.env.light = hs.esc_light;   // what bdpt_ctx.h view_of hands the kernels
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
  return S;
}

struct Job {
  int W, H, spp, M, s0, count, rr, threads;
  uint64_t seed;
  const int* pixels;
  int npix;
  double *eye, *light, *stats;
  int* nsplat = nullptr;   // with vmin: one thread only
  float* vmin = nullptr;
};

// render_sample (bdpt_paths.h) with the s = 0 contributions counted: direct[0] = how many (i, 0)
// strategies returned a value, direct[1] = the sum of their components' magnitudes
template <int MAXV, int LM, int EXT>
f3 sample_counted(const SceneView& S, const SampleParams& sp, Paths<MAXV>& P, Counters& cnt, int x, int y,
                  uint32_t sample, HostSink& sink, double* direct) {
  Rng g;
  prepare_sample<MAXV, LM, EXT>(S, sp, P, cnt, g, x, y, sample);
  f3 eye_sum = splat3(0);
  for (int i = 1; i < P.nE; i++) {
    for (int j = 0; j < P.nL; j++) {
      Conn cn;
      int kind = make_conn<EXT>(S, sp, PathsInRegs<MAXV, EXT>(P), g, i, j, cn);
      if (kind == CONN_DIRECT) {
        eye_sum = add(eye_sum, cn.val);
        sink.note(cn.val);
        direct[0] += 1;
        direct[1] += (double)fabsf(cn.val.x) + (double)fabsf(cn.val.y) + (double)fabsf(cn.val.z);
      } else if (kind == CONN_RAY) {
        if (trace_any<LM>(S, cn.o, cn.d, BDPT_EPS_F, cn.tmax, cnt)) continue;
        if (cn.splat >= 0) sink.splat(cn.splat % sp.W, cn.splat / sp.W, cn.val);
        else { eye_sum = add(eye_sum, cn.val); sink.note(cn.val); }
      }
    }
  }
  return eye_sum;
}

template <int MAXV, int LM, int EXT>
int run(const HostScene& hs, const Job& J) {
  const SceneView S = view_of_host<LM>(hs);
  SampleParams sp;
  sp.W = J.W; sp.H = J.H; sp.spp = J.spp; sp.max_depth = J.M; sp.seed = J.seed;
  sp.rr = J.rr;
  const int total = J.pixels ? J.npix : J.W * J.H;
  const int nt = J.threads < 1 ? 1 : (J.threads > total ? (total > 0 ? total : 1) : J.threads);
  const float inv = 1.0f / (float)J.spp;
  // thread t renders the pixels [total * t / nt, total * (t + 1) / nt) in order into the shared eye
  // frame (a pixel belongs to one thread) and its own light frame; the light frames are added in
  // thread order, so one thread gives core_cpu_render's summation order
  std::vector<std::vector<double>> lb(nt, std::vector<double>((size_t)J.W * J.H * 3, 0.0));
  std::vector<Counters> cnts(nt);
  std::vector<double> direct(2 * (size_t)nt, 0.0);
  auto work = [&](int t) {
    HostSink sink{&lb[t], J.W, J.nsplat, J.vmin};
    Counters cnt = {0, 0, 0, 0, 0, 0};
    Paths<MAXV>* P = new Paths<MAXV>();
    for (int q = (int)((long long)total * t / nt); q < (int)((long long)total * (t + 1) / nt); q++) {
      const int x = J.pixels ? J.pixels[2 * q] : q % J.W, y = J.pixels ? J.pixels[2 * q + 1] : q / J.W;
      for (int s = J.s0; s < J.s0 + J.count; s++) {
        const f3 v = sample_counted<MAXV, LM, EXT>(S, sp, *P, cnt, x, y, (uint32_t)s, sink, &direct[2 * t]);
        const size_t k = 3 * ((size_t)x + (size_t)y * J.W);
        J.eye[k] += (double)(v.x * inv); J.eye[k + 1] += (double)(v.y * inv); J.eye[k + 2] += (double)(v.z * inv);
      }
    }
    delete P;
    cnts[t] = cnt;
  };
  if (nt == 1) {
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
      st[8] += direct[2 * t]; st[9] += direct[2 * t + 1];
    }
    st[7] = EXT;   // the kernel flavour that rendered
    std::memcpy(J.stats, st, sizeof st);
  }
  return 0;
}

template <int LM, int EXT>
int render_maxv(const HostScene& hs, const Job& J) {
  const int need = J.M < 1 ? 1 : J.M;
  if (need <= 5) return run<5, LM, EXT>(hs, J);
  if (need <= 8) return run<8, LM, EXT>(hs, J);
  if (need <= 16) return run<16, LM, EXT>(hs, J);
  if (need <= 32) return run<32, LM, EXT>(hs, J);
  if (need <= 62) return run<62, LM, EXT>(hs, J);
  if (need <= 126) return run<126, LM, EXT>(hs, J);
  return BDPT_E_UNSUPPORTED;
}

template <int LM>
int render_lm(const bdpt_scene_desc* d, const Job& J, int infinite_lights) {
  HostScene hs;
  std::string err;
  const int rc = build_host_scene(d, hs, err, false, infinite_lights != 0);
  if (rc) { fprintf(stderr, "core_cpu_inf: %s\n", err.c_str()); return rc; }
  // the kernel selection of bdpt_create
  const int ext = kernel_flavour(hs, J.rr != 0);
  if (ext == 2) return render_maxv<LM, 2>(hs, J);
  if (ext == 1) return render_maxv<LM, 1>(hs, J);
  return render_maxv<LM, 0>(hs, J);
}

}  // namespace

// core_cpu_render (core_cpu.cpp) with bdpt_params.infinite_lights and a thread count. stats: 10
// doubles; [0..6] as core_cpu_render, [7] the kernel flavour (0 reference-only, 1 environment map /
// roulette, 2 infinite lights), [8] s = 0 strategies that returned a value, [9] the sum of those
// values' magnitudes.
extern "C" int core_cpu_inf_render(const bdpt_scene_desc* d, int W, int H, int spp, int M, uint64_t seed, int s0,
                                   int count, const int* pixels, int npix, double* eye, double* light,
                                   double* stats, int lds_mode, int rr, int infinite_lights, int threads) {
  Job J;
  J.W = W; J.H = H; J.spp = spp; J.M = M; J.s0 = s0; J.count = count; J.rr = rr; J.threads = threads;
  J.seed = seed; J.pixels = pixels; J.npix = npix; J.eye = eye; J.light = light; J.stats = stats;
  if (lds_mode == 1) return render_lm<1>(d, J, infinite_lights);
  if (lds_mode == 2) return render_lm<2>(d, J, infinite_lights);
  if (lds_mode == 3) return render_lm<3>(d, J, infinite_lights);
  return render_lm<0>(d, J, infinite_lights);
}

// The same on one thread, with the light image's splat count per pixel added to nsplat (W * H) and
// *vmin lowered to the smallest component of any eye or light addend (tests/_pixelbound.py: the
// addend counts of the per-pixel bound, and that no addend is negative).
extern "C" int core_cpu_inf_render_counts(const bdpt_scene_desc* d, int W, int H, int spp, int M, uint64_t seed,
                                          int s0, int count, const int* pixels, int npix, double* eye, double* light,
                                          double* stats, int lds_mode, int rr, int infinite_lights, int* nsplat,
                                          float* vmin) {
  Job J;
  J.W = W; J.H = H; J.spp = spp; J.M = M; J.s0 = s0; J.count = count; J.rr = rr; J.threads = 1;
  J.seed = seed; J.pixels = pixels; J.npix = npix; J.eye = eye; J.light = light; J.stats = stats;
  J.nsplat = nsplat; J.vmin = vmin;
  if (lds_mode == 1) return render_lm<1>(d, J, infinite_lights);
  if (lds_mode == 2) return render_lm<2>(d, J, infinite_lights);
  if (lds_mode == 3) return render_lm<3>(d, J, infinite_lights);
  return render_lm<0>(d, J, infinite_lights);
}

// bdpt_create's scene checks (build_host_scene under the BDPT integrator) without a device: the
// status, the message, and on success the kernel flavour (*flavour) and the index of the light an
// escaped ray can reach (*esc_light, -1: none).
extern "C" int core_cpu_inf_scene_check(const bdpt_scene_desc* d, int infinite_lights, int rr, char* msg, int msg_len,
                                        int* flavour, int* esc_light) {
  HostScene hs;
  std::string err;
  const int rc = build_host_scene(d, hs, err, false, infinite_lights != 0);
  if (msg && msg_len > 0) snprintf(msg, (size_t)msg_len, "%s", err.c_str());
  if (rc == BDPT_OK) {
    if (flavour) *flavour = kernel_flavour(hs, rr != 0);
    if (esc_light) *esc_light = hs.esc_light;
  }
  return rc;
}
