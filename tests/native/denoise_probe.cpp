// tests/native/denoise_probe.cpp — TEST ONLY. The host builds of the a-trous filter and of the
// feature pass (core_cpu_denoise.cpp) on the odd frame sizes of tests/_denoise.py, for a build with
// -fsanitize=address,undefined (tests/test_denoise.py): every buffer is allocated at exactly its
// size, so a tap or a record read or written outside the frame is reported. Loads a COLLADA scene
// for the feature renders. Exit 0 and "no sanitizer report" = every output was finite and the
// sanitizers stayed silent.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "bdpt/bdpt.h"

namespace bdpt { thread_local std::string g_err; }   // the loader's error text (the product's is in bdpt_hip.hip)

extern "C" int core_cpu_denoise_features(const bdpt_scene_desc* d, int W, int H, int nsamp, uint64_t seed, int integrator,
                                         double lens_radius, double focal_distance, int infinite_lights, int lds_mode,
                                         float* out8);
extern "C" int core_cpu_denoise_filter(const float* color, const float* feat, int W, int H, int levels,
                                       float sigma_color, float sigma_normal, float sigma_depth, int demodulate,
                                       float* out);

static bool finite_all(const std::vector<float>& v) {
  for (float x : v)
    if (!std::isfinite(x)) return false;
  return true;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: denoise_probe <scene.dae>\n");
    return 2;
  }
  const int frames[4][2] = {{37, 21}, {8, 8}, {1, 1}, {64, 3}};
  int bad = 0;
  for (const auto& fr : frames) {
    const int W = fr[0], H = fr[1];
    bdpt_dae* dae = nullptr;
    if (bdpt_dae_load(argv[1], W, H, &dae) != BDPT_OK) {
      fprintf(stderr, "denoise_probe: cannot load %s\n", argv[1]);
      return 3;
    }
    bdpt_scene_desc d;
    bdpt_dae_get_desc(dae, &d);
    const size_t npix = (size_t)W * H;
    for (int integrator = 0; integrator < 2; integrator++)
      for (int lm = 0; lm < 4; lm++) {
        std::vector<float> feat(npix * 8);
        const int rc = core_cpu_denoise_features(&d, W, H, 3, 5489, integrator, integrator ? 0.05 : 0.0, 4.7, 0, lm, feat.data());
        if (rc != 0 || !finite_all(feat)) { printf("features %dx%d integrator %d lm %d: rc %d or not finite\n", W, H, integrator, lm, rc); bad++; }
        if (lm != 0) continue;
        // a deterministic noisy colour; levels up to the cap, both demodulation settings, in place too
        std::vector<float> color(npix * 3);
        uint32_t s = 12345u + (uint32_t)W;
        for (float& c : color) { s = s * 1664525u + 1013904223u; c = (float)(s >> 8) * (2.0f / 16777216.0f); }
        for (int levels : {0, 1, 5, 8})
          for (int dm = 0; dm < 2; dm++) {
            std::vector<float> out(npix * 3);
            if (core_cpu_denoise_filter(color.data(), feat.data(), W, H, levels, 1.0f, 0.3f, 0.1f, dm, out.data()) != 0 || !finite_all(out)) {
              printf("filter %dx%d levels %d demodulate %d: failed or not finite\n", W, H, levels, dm);
              bad++;
            }
            std::vector<float> inplace(color);
            core_cpu_denoise_filter(inplace.data(), feat.data(), W, H, levels, 1.0f, 0.3f, 0.1f, dm, inplace.data());
            if (inplace != out) { printf("filter %dx%d levels %d demodulate %d: in place differs\n", W, H, levels, dm); bad++; }
          }
      }
    bdpt_dae_free(dae);
  }
  if (bad) return 1;
  printf("no sanitizer report\n");
  return 0;
}
