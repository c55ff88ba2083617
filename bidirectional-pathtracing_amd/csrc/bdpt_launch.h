// bdpt_launch.h — the host plumbing the C-ABI units share (bdpt_hip.hip, bdpt_denoise.hip,
// bdpt_variance.hip, bdpt_adaptive.hip): the LDS budgets, a plan (bdpt_ldsplan.h) applied to a launch,
// the persistent launch (dispatched over the LDS modes by bdpt_ldsplan.h dispatch_lm), the tile -> block list, and the small
// helpers of an entry point (ticket word, lazy allocation, read-back, argument checks).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "bdpt_ctx.h"
#include "bdpt_ldsplan.h"
#include "bdpt_megakernel.h"

namespace bdpt {

// LDS budget for the scene copy: 160 KB per CU shared by the blocks that the 4-waves/SIMD VGPR
// budget admits (16 waves per CU), minus their wave queues.
constexpr size_t kLdsPerCu = 160 * 1024;
constexpr size_t kBlocksPerCu = 4 * kMinWaves / kWavesPerBlock;
constexpr size_t kLdsSceneMax = kLdsPerCu / kBlocksPerCu - kWavesPerBlock * sizeof(WaveQ) - 256 - kStaticLds;
// LM 2's treelet gets kLdsSceneMax - kLdsStackBytes (an unsigned difference): it must hold at least
// one node, or the subtraction wraps and the treelet size is no longer capped by the LDS budget
static_assert(kLdsSceneMax > kLdsStackBytes + (size_t)node_bytes(lm_width(2)), "LDS budget: wave queues + stack slots leave no treelet");
// k_pt and k_features: their LDS holds the scene copy only
constexpr size_t kLdsCopyOnlyMax = kLdsPerCu / kBlocksPerCu - 256;

// Points a launch's parameters at the scene as the plan's mode sees it.
template <class KP>
void apply_plan(const Ctx* c, const LdsPlan& p, KP& kp) {
  kp.S = view_of(c, p.lm);
  kp.S.ntop = p.ntop;
  kp.n_node4 = p.n_node4;
}

// Persistent launch: as many blocks as are co-resident (occupancy query with this launch's LDS),
// never more waves than work items. *grid (when given) receives the block count before the launch.
template <class K, class KP>
int launch_persistent(Ctx* c, K kernel, const char* name, size_t lds, const KP& kp, long long items, int* grid_out = nullptr) {
  int per_cu = 0;
  HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kBlock, lds));
  if (per_cu <= 0) { g_err = std::string(name) + " cannot be resident (LDS/VGPR budget)"; return BDPT_E_DEVICE; }
  long long grid = std::min<long long>((long long)per_cu * c->ncu, (items + kWavesPerBlock - 1) / kWavesPerBlock);
  grid = std::max(1LL, grid);
  if (grid_out) *grid_out = (int)grid;
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(kBlock), lds, c->stream, kp);
  HIPCHK(hipGetLastError());
  return BDPT_OK;
}

// Tiles (raytrace_tile clips them to the frame, raytraced_renderer.cpp:600-604) -> 8x8 blocks
// {x, y, w, h}, appended to blk. The far edges are clipped in 64 bits: x0 + w may pass INT32_MAX.
inline void tiles_to_blocks(const bdpt_tile* tiles, int ntiles, int W, int H, std::vector<int4>& blk) {
  for (int t = 0; t < ntiles; t++) {
    const int x0 = std::max(0, tiles[t].x0), y0 = std::max(0, tiles[t].y0);
    const int x1 = (int)std::min<int64_t>(W, (int64_t)tiles[t].x0 + tiles[t].w);
    const int y1 = (int)std::min<int64_t>(H, (int64_t)tiles[t].y0 + tiles[t].h);
    for (int by = y0; by < y1; by += 8)
      for (int bx = x0; bx < x1; bx += 8) blk.push_back(make_int4(bx, by, std::min(8, x1 - bx), std::min(8, y1 - by)));
  }
}

// The ticket word of the render kernels: every use zeroes it first, in stream order. Null: the
// memset failed (g_err says how).
inline unsigned* reset_tickets(Ctx* c) {
  unsigned* work = (unsigned*)(c->d_stats + 15);
  const hipError_t e = hipMemsetAsync(work, 0, sizeof(unsigned), c->stream);
  if (e == hipSuccess) return work;
  g_err = std::string("hipMemsetAsync(kp.work, 0, sizeof(unsigned), c->stream): ") + hipGetErrorString(e);
  return nullptr;
}

// A buffer allocated on first use; with zero_on_stream, a fresh one is zeroed on that stream.
template <class T>
int ensure_alloc(T** p, size_t bytes, const hipStream_t* zero_on_stream = nullptr) {
  if (*p) return BDPT_OK;
  if (hipMalloc((void**)p, bytes) != hipSuccess) { g_err = "out of device memory"; return BDPT_E_NOMEM; }
  if (zero_on_stream) HIPCHK(hipMemsetAsync(*p, 0, bytes, *zero_on_stream));
  return BDPT_OK;
}

// The copy of a bdpt_read_* entry point: device memory to the caller's, complete on return.
inline int read_back(Ctx* c, void* dst, const void* src, size_t bytes) {
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return BDPT_OK;
}

// The body of a bdpt_read_* / *_device_ptr entry point over one per-pixel buffer of the context: under
// the lock, frame(c) is the buffer, or null (the error is `missing`); dptr receives it, dst a host copy.
template <class F>
int frame_out(void* ctx, F frame, const char* missing, size_t bytes_per_pixel, void* dst, void** dptr) {
  Ctx* c = (Ctx*)ctx;
  if (!c || (!dst && !dptr)) { g_err = "null argument"; return BDPT_E_INVALID; }
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  void* p = frame(c);
  if (!p) { g_err = missing; return BDPT_E_INVALID; }
  if (dptr) *dptr = p;
  return dst ? read_back(c, dst, p, c->npix * bytes_per_pixel) : BDPT_OK;
}

// The frame arguments of a *_buffers entry point.
inline int check_frame(int32_t device, int32_t w, int32_t h) {
  if (w <= 0 || h <= 0) { g_err = "invalid frame size"; return BDPT_E_INVALID; }
  if (device < 0) { g_err = "bad device ordinal"; return BDPT_E_INVALID; }
  return BDPT_OK;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// The PathTracer's focal distance (bdpt_params.focal_distance, 0 = its default), as k_pt and the
// feature pass of a PathTracer context take it.
inline float pt_focal(const bdpt_params& prm) { return lens_focal(prm.focal_distance); }

}  // namespace bdpt
