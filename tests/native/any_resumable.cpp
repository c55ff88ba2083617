// tests/native/any_resumable.cpp — TEST ONLY (tests/test_any_resumable.py). On the host (one lane)
// traverse_any_resumable must answer every any-hit query as trace_any does and visit the same nodes
// and primitives: per ray, both forms' answer and node / triangle / sphere counters are compared.
#define CORE_CPU_TRACE_ONLY
#include "core_cpu.cpp"

template <int LM>
static void resumable_check_lm(const HostScene& hs, const float* rays, int n, int* out) {
  const SceneView S = host_view(hs, LM);
  for (int i = 0; i < n; i++) {
    const float* r = rays + 8 * (size_t)i;
    const f3 o = mk3(r[0], r[1], r[2]), d = mk3(r[3], r[4], r[5]);
    Counters c1 = {}, c2 = {};
    const bool h1 = trace_any<LM, kConnStack>(S, o, d, r[6], r[7], c1);
    int stack_mem[kStackMax];
    TravStack<kConnStack> stk(stack_mem);
    AnyTrav<kConnStack> q = {};
    q.ref = kTravDone;
    // the caller still has rays to hand out (i odd) or not: one lane never reaches kRefillIdle
    traverse_any_resumable<LM, kConnStack>(S, q, stk, r[6], (i & 1) != 0, c2);   // nothing in flight: returns at once
    const bool idle_ok = q.ended() && c2.nodes == 0 && c2.tris == 0 && c2.sphs == 0;
    q.start(S, stk, o, d, r[7]);
    traverse_any_resumable<LM, kConnStack>(S, q, stk, r[6], (i & 1) != 0, c2);
    out[0] += h1 ? 1 : 0;
    out[1] += (q.ended() && idle_ok && q.hit == h1) ? 0 : 1;
    out[2] += c1.nodes == c2.nodes ? 0 : 1;
    out[3] += (c1.tris == c2.tris && c1.sphs == c2.sphs) ? 0 : 1;
    out[4] += (int)(c1.nodes / (uint32_t)lm_width(LM));
    out[5] += (int)(c1.tris + c1.sphs);
  }
}

// out (6, added to): rays that hit, rays whose answer differs (or whose query did not end), rays whose
// node count differs, rays whose primitive counts differ, trace_any's node steps, its primitive tests
extern "C" int any_resumable_check(const bdpt_scene_desc* d, int lds_mode, const float* rays, int n, int* out) {
  HostScene hs;
  std::string err;
  if (build_host_scene(d, hs, err) != BDPT_OK) return -1;
  if (lds_mode == 1) resumable_check_lm<1>(hs, rays, n, out);
  else if (lds_mode == 2) resumable_check_lm<2>(hs, rays, n, out);
  else resumable_check_lm<0>(hs, rays, n, out);
  return 0;
}
