// tests/native/core_cpu_lens.cpp — TEST ONLY. The device-side BDPT pipeline (bdpt_core.h) and the
// host scene preparation (bdpt_scene.cpp) compiled with g++, in the shape of core_cpu_inf.cpp, with
// the thin lens (bdpt_params.lens_radius > 0): the yardstick of the GPU's lens
// kernels (flavour 3) and the renderer of the convergence tests. lens_radius <= 0 renders with the
// flavour bdpt_create picks for the pinhole. Never linked into the product.
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
  float lens_r = 0.0f, focal = 4.7f;
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
  SceneView S = view_of_host<LM>(hs);
  S.cam.lens_r = J.lens_r;
  SampleParams sp;
  sp.focal = J.focal;
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
  if (rc) { fprintf(stderr, "core_cpu_lens: %s\n", err.c_str()); return rc; }
  // the kernel selection of bdpt_create
  const int ext = kernel_flavour(hs, J.rr != 0, J.lens_r > 0.0f);
  if (ext == 3) return render_maxv<LM, 3>(hs, J);
  if (ext == 2) return render_maxv<LM, 2>(hs, J);
  if (ext == 1) return render_maxv<LM, 1>(hs, J);
  return render_maxv<LM, 0>(hs, J);
}

}  // namespace

// core_cpu_inf_render with the thin lens: lens_radius > 0 renders through flavour 3 with
// focal_distance (0 = 4.7), lens_radius <= 0 through the pinhole's flavour. stats: 10 doubles as
// core_cpu_inf_render's ([7] the kernel flavour that rendered).
extern "C" int core_cpu_lens_render(const bdpt_scene_desc* d, int W, int H, int spp, int M, uint64_t seed, int s0,
                                    int count, const int* pixels, int npix, double* eye, double* light,
                                    double* stats, int lds_mode, int rr, int infinite_lights, int threads,
                                    double lens_radius, double focal_distance) {
  Job J;
  J.W = W; J.H = H; J.spp = spp; J.M = M; J.s0 = s0; J.count = count; J.rr = rr; J.threads = threads;
  J.seed = seed; J.pixels = pixels; J.npix = npix; J.eye = eye; J.light = light; J.stats = stats;
  J.lens_r = (float)lens_radius;
  J.focal = lens_focal(focal_distance);
  if (lds_mode == 1) return render_lm<1>(d, J, infinite_lights);
  if (lds_mode == 2) return render_lm<2>(d, J, infinite_lights);
  if (lds_mode == 3) return render_lm<3>(d, J, infinite_lights);
  return render_lm<0>(d, J, infinite_lights);
}

// bdpt_create's kernel choice without a device: the status of the scene checks and, on success,
// the flavour for these settings.
extern "C" int core_cpu_lens_flavour(const bdpt_scene_desc* d, int infinite_lights, int rr, double lens_radius,
                                     int* flavour) {
  HostScene hs;
  std::string err;
  const int rc = build_host_scene(d, hs, err, false, infinite_lights != 0);
  if (rc == BDPT_OK && flavour) *flavour = kernel_flavour(hs, rr != 0, lens_radius > 0);
  return rc;
}

// The two halves of the round trip (tests/test_lens.py): the eye ray of raster position (x, y) in
// [0, 1]^2 from the lens point of uniforms (u1, u2), and the camera sampler from the same lens
// point toward the world point p. cam: the scene's camera; out: origin[3] dir[3] / pixel[2] pos[3].
static DCam lens_cam(const bdpt_scene_desc* d, double lens_radius, int* rc) {
  HostScene hs;
  std::string err;
  *rc = build_host_scene(d, hs, err, false, true);
  hs.cam.lens_r = (float)lens_radius;
  return hs.cam;
}
extern "C" int core_cpu_lens_eye_rays(const bdpt_scene_desc* d, double lens_radius, double focal_distance, int n,
                                      const float* u, const float* xy, float* origin, float* dir) {
  int rc;
  const DCam c = lens_cam(d, lens_radius, &rc);
  if (rc) return rc;
  for (int k = 0; k < n; k++) {
    const f3 pl = lens_plens(c, u[2 * k], u[2 * k + 1]);
    const f3 o = lens_world(c, pl), r = lens_ray_dir(c, lens_focal(focal_distance), pl, xy[2 * k], xy[2 * k + 1]);
    origin[3 * k] = o.x; origin[3 * k + 1] = o.y; origin[3 * k + 2] = o.z;
    dir[3 * k] = r.x; dir[3 * k + 1] = r.y; dir[3 * k + 2] = r.z;
  }
  return 0;
}
extern "C" int core_cpu_lens_camera_samples(const bdpt_scene_desc* d, double lens_radius, double focal_distance,
                                            int W, int H, int n, const float* u, const float* p, int* pixel,
                                            float* pos) {
  int rc;
  const DCam c = lens_cam(d, lens_radius, &rc);
  if (rc) return rc;
  for (int k = 0; k < n; k++) {
    const f3 pl = lens_plens(c, u[2 * k], u[2 * k + 1]);
    const EyeSample e = camera_sample_lens(c, lens_focal(focal_distance), W, H, pl, mk3(p[3 * k], p[3 * k + 1], p[3 * k + 2]));
    pixel[2 * k] = e.x; pixel[2 * k + 1] = e.y;
    pos[3 * k] = e.pos.x; pos[3 * k + 1] = e.pos.y; pos[3 * k + 2] = e.pos.z;
  }
  return 0;
}
