// tests/native/variance_probe.cpp — TEST ONLY. The host build of the batch moments, the variance and
// the variance-guided a-trous filter (core_cpu_variance.cpp) on the odd frame sizes of
// tests/_denoise.py, for a build with -fsanitize=address,undefined (tests/test_variance.py): every
// buffer is allocated at exactly its size, so a tap or a record read or written outside the frame
// is reported. Exit 0 and "no sanitizer report" = every output was finite and the sanitizers stayed
// silent.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" int core_cpu_variance_moments(const float* a, const float* b, float* rec, long long npix);
extern "C" int core_cpu_variance_variance(const float* rec, int K, long long npix, float* var);
extern "C" int core_cpu_variance_filter(const float* color, const float* var, const float* feat, int W, int H, int levels,
                                        float sigma_variance, float sigma_normal, float sigma_depth, float* out,
                                        float* var_out);

static bool finite_all(const std::vector<float>& v) {
  for (float x : v)
    if (!std::isfinite(x)) return false;
  return true;
}

static uint32_t g_s = 12345u;
static float rnd() {
  g_s = g_s * 1664525u + 1013904223u;
  return (float)(g_s >> 8) * (1.0f / 16777216.0f);
}

int main() {
  const int frames[4][2] = {{37, 21}, {8, 8}, {1, 1}, {64, 3}};
  int bad = 0;
  for (const auto& fr : frames) {
    const int W = fr[0], H = fr[1];
    const size_t npix = (size_t)W * H;
    // K batches into the record, with and without the second frame
    for (int K : {2, 3, 8})
      for (int second = 0; second < 2; second++) {
        std::vector<float> a(npix * 3, 0.0f), b(npix * 3, 0.0f), rec(npix * 4, 0.0f), var(npix);
        for (int k = 0; k < K; k++) {
          for (float& x : a) x += rnd();
          for (float& x : b) x += 0.5f * rnd();
          if (core_cpu_variance_moments(a.data(), second ? b.data() : nullptr, rec.data(), (long long)npix) != 0) bad++;
        }
        if (core_cpu_variance_variance(rec.data(), K, (long long)npix, var.data()) != 0 || !finite_all(rec) || !finite_all(var)) {
          printf("moments %dx%d K %d second %d: failed or not finite\n", W, H, K, second);
          bad++;
        }
        for (float v : var)
          if (v < 0) { printf("moments %dx%d K %d: negative variance\n", W, H, K); bad++; break; }
      }
    // the filter: a noisy colour, a variance with zeros, features of two normals and a depth ramp
    std::vector<float> color(npix * 3), var(npix), feat(npix * 8, 0.0f);
    for (float& c : color) c = 2.0f * rnd();
    for (size_t p = 0; p < npix; p++) {
      var[p] = p % 5 == 0 ? 0.0f : 0.5f * rnd();
      float* f = feat.data() + 8 * p;
      f[0] = f[1] = f[2] = 0.5f;
      if ((int)(p % W) < (W + 1) / 2) f[5] = 1.0f; else f[4] = 1.0f;
      f[6] = 1.0f + 0.1f * (float)(p % W);
      f[7] = 1.0f;
    }
    for (int levels : {0, 1, 5, 8}) {
      std::vector<float> out(npix * 3), vout(npix);
      if (core_cpu_variance_filter(color.data(), var.data(), feat.data(), W, H, levels, 2.0f, 0.3f, 0.1f, out.data(), vout.data()) != 0 ||
          !finite_all(out) || !finite_all(vout)) {
        printf("filter %dx%d levels %d: failed or not finite\n", W, H, levels);
        bad++;
      }
      std::vector<float> ic(color), iv(var);
      core_cpu_variance_filter(ic.data(), iv.data(), feat.data(), W, H, levels, 2.0f, 0.3f, 0.1f, ic.data(), iv.data());
      if (ic != out || iv != vout) { printf("filter %dx%d levels %d: in place differs\n", W, H, levels); bad++; }
      std::vector<float> oc(npix * 3);
      core_cpu_variance_filter(color.data(), var.data(), feat.data(), W, H, levels, 2.0f, 0.3f, 0.1f, oc.data(), nullptr);
      if (oc != out) { printf("filter %dx%d levels %d: without a variance output differs\n", W, H, levels); bad++; }
    }
  }
  if (bad) return 1;
  printf("no sanitizer report\n");
  return 0;
}
