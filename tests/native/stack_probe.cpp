// tests/native/stack_probe.cpp — TEST ONLY. The traversal stack at its worst case, for a build with
// -fsanitize=address,undefined (tests/test_ray_queries.py): loads a COLLADA scene and sends rays that
// enter every child of every node through the closest-hit and any-hit traversals of LDS modes 0, 1
// and 2 (core_cpu.cpp). Such a ray holds every sibling of its path on the stack, (W - 1) per level:
// what the builder's (W-1)*(depth+1)+2 limit (bdpt_scene.cpp) is sized for. That the rays do enter
// every child is checked from the node-visit counter, not assumed. Two ray sets:
//   nan: NaN origin, [1e-5, inf). fmaxf / fminf drop the NaN plane distances, so every slab test
//        passes. The 4-wide closest-hit step sorts its children by an entry distance that is NaN
//        here and so takes them all for misses: that one combination visits the root alone.
//   inf: origin (+inf, +inf, +inf), direction (1, 1, 1) / sqrt 3, (-inf, +inf). Every plane distance
//        is -inf, every slab test passes with a key of -inf: every child is entered in all six
//        combinations, the 4-wide closest-hit step included.
// Exit 0 and "no sanitizer report" = every expectation held and the sanitizers stayed silent.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "bdpt/bdpt.h"

namespace bdpt { thread_local std::string g_err; }   // the loader's error text (the product's is in bdpt_hip.hip)

extern "C" int core_cpu_trace_visits(const bdpt_scene_desc* d, const float* rays, int n, int* out_prim,
                                     unsigned* visits, int* info);

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: stack_probe <scene.dae>\n");
    return 2;
  }
  bdpt_dae* dae = nullptr;
  if (bdpt_dae_load(argv[1], 32, 24, &dae) != BDPT_OK) {
    fprintf(stderr, "stack_probe: cannot load %s\n", argv[1]);
    return 3;
  }
  bdpt_scene_desc d;
  bdpt_dae_get_desc(dae, &d);
  const int n = 64;
  const float s3 = 0.577350269f;
  std::vector<float> nan_rays, inf_rays;
  for (int i = 0; i < n; i++) {
    // directions through all eight octants (the 4-wide fetch orders a node's rows by them)
    const float dx = (i & 1) ? -s3 : s3, dy = (i & 2) ? -s3 : s3, dz = (i & 4) ? -s3 : s3;
    const float a[8] = {NAN, NAN, NAN, dx, dy, dz, 1e-5f, INFINITY};
    const float b[8] = {dx > 0 ? INFINITY : -INFINITY, dy > 0 ? INFINITY : -INFINITY, dz > 0 ? INFINITY : -INFINITY,
                        dx, dy, dz, -INFINITY, INFINITY};
    nan_rays.insert(nan_rays.end(), a, a + 8);
    inf_rays.insert(inf_rays.end(), b, b + 8);
  }
  // one scene build: the nan rays first, then the inf rays, through every mode and query kind
  std::vector<float> rays = nan_rays;
  rays.insert(rays.end(), inf_rays.begin(), inf_rays.end());
  std::vector<int> prim(6 * 2 * n);
  std::vector<unsigned> visits(6 * 2 * n);
  int info[15];
  if (core_cpu_trace_visits(&d, rays.data(), 2 * n, prim.data(), visits.data(), info) != 0) {
    fprintf(stderr, "stack_probe: scene build failed\n");
    return 4;
  }
  int bad = 0;
  for (int lm = 0; lm < 3; lm++)
    for (int any = 0; any < 2; any++)
      for (int set = 0; set < 2; set++) {
        const int* f = info + 5 * lm;
        const unsigned W = (unsigned)f[0], all = W * (unsigned)f[1];
        const unsigned want = (set == 0 && !any && W == 4) ? W : all;
        unsigned lo = ~0u, hi = 0;
        int hits = 0;
        const int at = (2 * lm + any) * 2 * n + set * n;
        for (int i = at; i < at + n; i++) {
          lo = visits[i] < lo ? visits[i] : lo;
          hi = visits[i] > hi ? visits[i] : hi;
          hits += prim[i] >= 0;
        }
        const bool ok = lo == want && hi == want && hits == 0;
        printf("LM %d %s %-7s: W %u, %d nodes, %d levels, stack need %d, stack limit %d; visits per ray %u..%u, "
               "expected %u (%s), hits %d%s\n",
               lm, set ? "inf" : "nan", any ? "any" : "closest", W, f[1], f[2], f[3], f[4], lo, hi, want,
               want == all ? "every child of every node" : "the root alone", hits, ok ? "" : "  <-- FAILED");
        if (!ok) bad++;
      }
  bdpt_dae_free(dae);
  if (bad) {
    printf("stack_probe: %d expectations failed\n", bad);
    return 1;
  }
  printf("stack_probe: every expectation held, no sanitizer report\n");
  return 0;
}
