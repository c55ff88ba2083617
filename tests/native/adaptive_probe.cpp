// tests/native/adaptive_probe.cpp — TEST ONLY. The host build of the adaptive sampler's records,
// decision, compaction and resolve (core_cpu_adaptive.cpp) on the odd frame sizes of tests/_denoise.py,
// for a build with -fsanitize=address,undefined (tests/test_adaptive.py): every buffer is allocated at
// exactly its size, so a record, a flag or a list entry read or written outside it is reported. Runs a
// synthetic render of 6 rounds in which the decisions shrink the block list. Exit 0 and "no sanitizer
// report" = every output was finite, the counts were consistent and the sanitizers stayed silent.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" int core_cpu_adaptive_moments(const float* eye, const float* light, float* rec_e, float* rec_l, long long npix,
                                         long long round_samples);
extern "C" int core_cpu_adaptive_decide(const float* rec_e, const float* rec_l, int* rounds, int* active, int W, int H, int S, int m,
                                        int R, long long N, float tol, int decide, float* sums);
extern "C" int core_cpu_adaptive_compact(const int* active, int W, int H, int* list4, int* counts);
extern "C" int core_cpu_adaptive_resolve(const float* rec_e, const float* rec_l, const int* rounds, int W, int H, int S, int m, int R,
                                         long long N, float* color, float* var, int* count);

static uint32_t g_s = 12345u;
static float rnd() {
  g_s = g_s * 1664525u + 1013904223u;
  return (float)(g_s >> 8) * (1.0f / 16777216.0f);
}

int main() {
  const int frames[4][2] = {{37, 21}, {8, 8}, {1, 1}, {64, 3}};
  const int S = 12, m = 2, rounds_max = 6, min_rounds = 2;
  int bad = 0;
  for (const auto& fr : frames) {
    const int W = fr[0], H = fr[1];
    const size_t npix = (size_t)W * H;
    const int nbx = (W + 7) / 8, nb = nbx * ((H + 7) / 8);
    std::vector<float> eye(npix * 3, 0.0f), light(npix * 3, 0.0f), rec_e(npix * 4, 0.0f), rec_l(npix * 4, 0.0f);
    std::vector<int> rounds(nb, 0), active(nb, 1), list(4 * (size_t)nb), counts(2);
    long long N = 0;
    int R = 0, nact = nb, pix = (int)npix;
    while (true) {
      // the round's samples land in the active blocks only; the noise grows with the block index
      for (size_t p = 0; p < npix; p++) {
        const int b = (int)((p / W) / 8) * nbx + (int)((p % W) / 8);
        if (!active[b]) continue;
        for (int c = 0; c < 3; c++) {
          eye[3 * p + c] += 0.1f + 0.05f * (float)(b % 5) * rnd();
          light[3 * p + c] += 0.01f + 0.0005f * (float)(b % 3) * rnd();
        }
      }
      const long long M = (long long)pix * m;
      N += M;
      R++;
      if (core_cpu_adaptive_moments(eye.data(), light.data(), rec_e.data(), rec_l.data(), (long long)npix, M) != 0) bad++;
      if (core_cpu_adaptive_decide(rec_e.data(), rec_l.data(), rounds.data(), active.data(), W, H, S, m, R, N, 0.05f, R >= min_rounds,
                                   nullptr) != 0)
        bad++;
      if (core_cpu_adaptive_compact(active.data(), W, H, list.data(), counts.data()) != 0) bad++;
      int want = 0;
      for (int a : active) want += a != 0;
      if (counts[0] != want || counts[1] < 0 || counts[1] > (int)npix || counts[0] > nact) {
        printf("%dx%d round %d: inconsistent counts %d %d\n", W, H, R, counts[0], counts[1]);
        bad++;
      }
      nact = counts[0];
      pix = counts[1];
      if (nact == 0 || R == rounds_max) break;
    }
    std::vector<float> color(npix * 3), var(npix);
    std::vector<int> count(npix);
    if (core_cpu_adaptive_resolve(rec_e.data(), rec_l.data(), rounds.data(), W, H, S, m, R, N, color.data(), var.data(), count.data()) != 0)
      bad++;
    for (float x : color)
      if (!std::isfinite(x)) { printf("%dx%d: colour not finite\n", W, H); bad++; break; }
    for (float x : var)
      if (!std::isfinite(x) || x < 0) { printf("%dx%d: variance negative or not finite\n", W, H); bad++; break; }
    for (int k : count)
      if (k < min_rounds * m || k > R * m) { printf("%dx%d: count %d outside the rounds run\n", W, H, k); bad++; break; }
    printf("%dx%d: %d rounds, %lld pixel-samples, %d blocks left of %d\n", W, H, R, N, nact, nb);
  }
  if (bad) return 1;
  printf("no sanitizer report\n");
  return 0;
}
