// tests/native/core_cpu_inf.cpp — TEST ONLY. The device-side BDPT pipeline (bdpt_core.h) and the
// host scene preparation (bdpt_scene.cpp) compiled with g++, like core_cpu.cpp, with the
// bdpt_params.infinite_lights opt-in: the yardstick of the GPU's infinite-light
// kernels and the renderer of the convergence tests. Never linked into the product.
#include <cstdio>

#include "core_cpu_host.h"

using namespace bdpt;

// core_cpu_render (core_cpu.cpp) with bdpt_params.infinite_lights and a thread count. stats: 10
// doubles; [0..6] as core_cpu_render, [7] the kernel flavour (0 reference-only, 1 environment map /
// roulette, 2 infinite lights), [8] s = 0 strategies that returned a value, [9] the sum of those
// values' magnitudes.
extern "C" int core_cpu_inf_render(const bdpt_scene_desc* d, int W, int H, int spp, int M, uint64_t seed, int s0,
                                   int count, const int* pixels, int npix, double* eye, double* light,
                                   double* stats, int lds_mode, int rr, int infinite_lights, int threads) {
  Job J = {W, H, spp, M, s0, count, rr, seed, pixels, npix, eye, light, stats, 10};
  J.threads = threads;
  return host_render<2>("core_cpu_inf", d, infinite_lights, lds_mode, J, HostSink());
}

// The same on one thread, with the light image's splat count per pixel added to nsplat (W * H) and
// *vmin lowered to the smallest component of any eye or light addend (tests/_pixelbound.py: the
// addend counts of the per-pixel bound, and that no addend is negative).
extern "C" int core_cpu_inf_render_counts(const bdpt_scene_desc* d, int W, int H, int spp, int M, uint64_t seed,
                                          int s0, int count, const int* pixels, int npix, double* eye, double* light,
                                          double* stats, int lds_mode, int rr, int infinite_lights, int* nsplat,
                                          float* vmin) {
  const Job J = {W, H, spp, M, s0, count, rr, seed, pixels, npix, eye, light, stats, 10};
  HostSink sink;
  sink.nsplat = nsplat;
  sink.vmin = vmin;
  return host_render<2>("core_cpu_inf", d, infinite_lights, lds_mode, J, sink);
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
