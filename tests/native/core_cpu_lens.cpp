// tests/native/core_cpu_lens.cpp — TEST ONLY. The device-side BDPT pipeline (bdpt_core.h) and the
// host scene preparation (bdpt_scene.cpp) compiled with g++, in the shape of core_cpu_inf.cpp, with
// the thin lens (bdpt_params.lens_radius > 0): the yardstick of the GPU's lens
// kernels (flavour 3) and the renderer of the convergence tests. lens_radius <= 0 renders with the
// flavour bdpt_create picks for the pinhole. Never linked into the product.
#include <cstdio>

#include "core_cpu_host.h"

using namespace bdpt;

// core_cpu_inf_render with the thin lens: lens_radius > 0 renders through flavour 3 with
// focal_distance (0 = 4.7), lens_radius <= 0 through the pinhole's flavour. stats: 10 doubles as
// core_cpu_inf_render's ([7] the kernel flavour that rendered).
extern "C" int core_cpu_lens_render(const bdpt_scene_desc* d, int W, int H, int spp, int M, uint64_t seed, int s0,
                                    int count, const int* pixels, int npix, double* eye, double* light,
                                    double* stats, int lds_mode, int rr, int infinite_lights, int threads,
                                    double lens_radius, double focal_distance) {
  Job J = {W, H, spp, M, s0, count, rr, seed, pixels, npix, eye, light, stats, 10};
  J.threads = threads;
  J.lens_r = (float)lens_radius;
  J.focal = lens_focal(focal_distance);
  return host_render<3>("core_cpu_lens", d, infinite_lights, lds_mode, J, HostSink());
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
