// bdpt_ctx.h — the device context behind the C-ABI handle (shared by the kernels' TU,
// bdpt_hip.hip, and the multi-GPU frame reduce, bdpt_reduce.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <mutex>
#include <string>

#include "bdpt/bdpt.h"
#include "bdpt_core.h"
#include "bdpt_err.h"
#include "bdpt_scene.h"

namespace bdpt {

// bdpt_last_error() text: bdpt_err.h

struct Ctx {
  HostScene hs;
  int ext = 0;                 // kernel flavour (kernel_flavour, bdpt_scene.h): 1 environment light or
                               // Russian roulette, 2 hemisphere / directional lights as well
  bdpt_params prm;
  int device = 0;
  hipStream_t own = nullptr, stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool timed = false;
  float* d_nodes2 = nullptr;   // HostScene::bvh2 / bvh4
  float* d_nodes4 = nullptr;
  float* d_geom = nullptr;
  float* d_shade = nullptr;
  DMat* d_mats = nullptr;
  DLight* d_lights = nullptr;
  int* d_prim_ref = nullptr;
  int* d_leaves = nullptr;     // HostScene::leaf_refs (LM 3 staging source)
  float* d_env = nullptr;      // HostScene::env (environment light tables + map)
  int* d_count = nullptr;      // PathTracer::sampleCountBuffer (W*H)
  unsigned* d_work8 = nullptr;  // 8 per-XCD-group ticket counters, 128 B apart
  bool pt = false;             // bdpt_params.integrator == BDPT_INTEGRATOR_PT
  float* d_eye = nullptr;
  float* d_light = nullptr;
  float* d_sample = nullptr;
  // [0..7] counters, [12..14] environment-table reads, [15] tickets, [16..31] phase profile,
  // [32..47] lane-use profile (BDPT_PHASE_PROF builds)
  static constexpr int kStatSlots = 48;
  unsigned long long* d_stats = nullptr;
  // Tile-block lists of bdpt_render: a ring of pinned staging + device buffers, each slot reused
  // only after the event recorded behind the launch that read it, so back-to-back tile renders
  // (raytrace_tile / raytrace_pixel callers) never wait for the GPU.
  struct BlockSlot {
    int4* h = nullptr;
    int4* d = nullptr;
    size_t cap = 0;
    hipEvent_t done = nullptr;
    bool pending = false;
  };
  static constexpr int kBlockSlots = 4;
  BlockSlot blk[kBlockSlots];
  int blk_next = 0;
  // Every entry point locks the ctx: the reference drives raytrace_pixel / raytrace_tile from N
  // worker threads (raytraced_renderer.cpp:325-327,610-615); calls on one ctx are serialised here.
  std::recursive_mutex mu;
  // Diagnostics read once at bdpt_create (BDPT_LDS_MODE, BDPT_NTOP_MAX, BDPT_BLOCK_MAJOR,
  // BDPT_XCD_GROUPS): -1 = not set.
  int env_lds_mode = -1, env_ntop_max = -1, block_major = 1, xcd = 0;
  int last_lm = -1;            // LDS mode of the last BDPT / PathTracer launch
  // The rest of the last launch's plan (bdpt_debug_launch_plan): {lstack_on, ntop, dynamic LDS bytes,
  // grid blocks, samples per lane, work items, materials / lights staged in LDS}; -1 = none yet,
  // and for what a PathTracer launch does not have (lstack_on, spl, staged).
  int last_plan[7] = {-1, -1, -1, -1, -1, -1, -1};
  int maxv = 5;
  int ncu = 256;
  size_t npix = 0;
  // Denoised output (bdpt_denoise.hip), all allocated on first use: the feature
  // frame (W*H*8), the denoised frame (W*H*3), the filter's two ping-pong frames, and the 8x8 block
  // list of a tiled feature pass.
  float* d_features = nullptr;
  float* d_denoised = nullptr;
  float* d_dn_scratch = nullptr;
  int4* d_feat_blocks = nullptr;
  size_t feat_blocks_cap = 0;
  bool denoised_valid = false;
  // Variance-guided denoise (bdpt_variance.hip), all allocated on first use: the
  // moments record (W*H float4 {prev.rgb, Q}), the variance frame (W*H) and the filter's two
  // variance ping-pong frames. var_batches: batches in the record (K); var_batch_spp: samples per
  // batch; var_unbatched: bdpt_render ran outside bdpt_render_batches since the last bdpt_clear;
  // in_batches: bdpt_render_batches is the caller of bdpt_render.
  float* d_moments = nullptr;
  float* d_variance = nullptr;
  float* d_var_scratch = nullptr;
  int var_batches = 0, var_batch_spp = 0;
  bool var_unbatched = false, in_batches = false, variance_valid = false;
  // Adaptive sampling (bdpt_adaptive.hip), all allocated by the first adaptive render:
  // the eye and the light records (2 x W*H float4), per 8x8 block the rounds it was active and its
  // active flag (2 x nblocks int), the compacted block list, its two counts {blocks, pixels} on the
  // device and in pinned memory with the event of the per-round wait, and the resolved frames
  // (colour W*H*3, variance W*H, counts W*H int32; allocated by the first resolve). frame_dirty: the
  // frame holds samples since the last bdpt_clear; adapt_valid: they are an adaptive render's, of
  // adapt_rounds rounds of adapt_m samples and adapt_n pixel-samples in all.
  float* d_adapt_rec = nullptr;
  int* d_adapt_rounds = nullptr;
  int4* d_adapt_list = nullptr;
  int* d_adapt_counts = nullptr;
  int* h_adapt_counts = nullptr;
  hipEvent_t adapt_ev = nullptr;
  float* d_adapt_out = nullptr;
  int adapt_rounds = 0, adapt_m = 0, adapt_active = 0;
  long long adapt_n = 0;
  bool frame_dirty = false, adapt_valid = false, adapt_resolved = false;
};

// The launch half of bdpt_render (bdpt_hip.hip): samples [spp_begin, spp_begin + spp_count) of the
// nblocks 8x8 pixel blocks {x, y, w, h} at d_blocks (device memory), or of the whole frame when
// d_blocks is null. The caller holds c->mu and has set the device.
int render_blocks(Ctx* c, const int4* d_blocks, int nblocks, int spp_begin, int spp_count);

#define HIPCHK(x)                                                                   \
  do {                                                                              \
    hipError_t e_ = (x);                                                            \
    if (e_ != hipSuccess) {                                                         \
      ::bdpt::g_err = std::string(#x) + ": " + hipGetErrorString(e_);               \
      return BDPT_E_DEVICE;                                                         \
    }                                                                               \
  } while (0)

// The scene as a kernel of LDS mode LM sees it (scene_view, bdpt_scene.h) over the device copies.
inline SceneView view_of(const Ctx* c, int LM) {
  return scene_view(c->hs, {c->d_nodes2, c->d_nodes4, c->d_geom, c->d_shade, c->d_mats, c->d_lights, c->d_leaves, c->d_env}, LM);
}

}  // namespace bdpt
