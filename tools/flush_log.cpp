// tools/flush_log.cpp — DIAGNOSTICS ONLY (tools/flush_sim.py; never linked into the product). The CPU
// build of the device code (tests/native/core_cpu.cpp) compiled with -DBDPT_STEP_HIST, plus access
// to the any-hit query log that bdpt_bvh.h / bdpt_paths.h keep in such a build.
#include "../tests/native/core_cpu.cpp"

static std::vector<int> g_anyhit_log;
extern "C" void core_cpu_anyhit_log(int on) {
  g_anyhit_log.clear();
  anyhit_log() = on == 1 ? &g_anyhit_log : nullptr;
}
// copies up to max_ints ints of the log (triples, bdpt_bvh.h anyhit_log) and returns its length
extern "C" long long core_cpu_anyhit_log_get(int* out, long long max_ints) {
  const long long n = (long long)g_anyhit_log.size();
  for (long long k = 0; k < n && k < max_ints; k++) out[k] = g_anyhit_log[(size_t)k];
  return n;
}
