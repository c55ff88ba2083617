// bdpt_hip.hip — HIP kernels for gfx950 + the C-ABI of include/bdpt/bdpt.h (libbdpt_amd.so).
//
// k_bdpt_sample: one lane per (pixel, chunk of samples). Lanes of a wave cover an 8x8 pixel block
// at the same sample index (coherent primary rays and BVH paths). Each lane runs the reference's
// per-sample estimator (bdpt_core.h: eye walk, light walk, all s x t connections with MIS),
// accumulates its eye-image value in registers and adds it once per chunk to the fp32 eye frame;
// t = 1 light-tracing splats (bidirection.cpp:457-466) are fp32 atomics into the light frame —
// the device form of update_pixel under update_lock (bidirection.cpp:544-551).
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see __graft_entry__.build).

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>

#include "bdpt/bdpt.h"
#include "bdpt_core.h"
#include "bdpt_launch.h"   // bdpt_ctx.h, bdpt_megakernel.h, bdpt_ldsplan.h
#include "bdpt_scene.h"

using namespace bdpt;

thread_local std::string bdpt::g_err;

namespace {

// k_pt: the unidirectional PathTracer (bdpt_core.h pt_pixel). Persistent waves take 8x8 pixel
// blocks from a ticket counter; a lane owns one pixel and runs its adaptive batches to the end
// (PathTracer::raytrace_pixel), then stores the mean (update_pixel) and the sample count.
struct PtKParams {
  SceneView S;
  PtParams pp;
  float* eye;                 // the frame (sampleBuffer)
  int* count;                 // sampleCountBuffer
  unsigned long long* stats;
  const int4* blocks;
  int nblocks, nbx;
  unsigned* work;
  int n_node4, n_geom4;
};

template <bool STATS, int LM>
__global__ __launch_bounds__(kBlock, kMinWaves) void k_pt(PtKParams kp) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63;
  stage_lds_scene<LM>(kp.S, kp.n_node4, kp.n_geom4, (float4*)smem);   // no stack slots, no material / light copy
  Counters cnt = {0, 0, 0, 0, 0, 0};
  unsigned nsamp = 0;
  for (;;) {
    unsigned item = 0;
    if (lane == 0) item = atomicAdd(kp.work, 1u);
    item = __shfl(item, 0, 64);
    if (item >= (unsigned)kp.nblocks) break;
    int x, y;
    if (block_pixel(kp.blocks, kp.nbx, kp.pp.W, kp.pp.H, (int)item, lane, x, y)) {
      int n = 0;
      const f3 v = pt_pixel<LM>(kp.S, kp.pp, cnt, x, y, &n);
      const size_t k = (size_t)x + (size_t)y * kp.pp.W;
      kp.eye[3 * k] = v.x;
      kp.eye[3 * k + 1] = v.y;
      kp.eye[3 * k + 2] = v.z;
      kp.count[k] = n;
      nsamp += (unsigned)n;
    }
  }
  flush_stats<STATS, 8>(kp.stats, lane, nsamp, cnt);
}

__global__ void k_trace_rays(SceneView S, const float* rays, int n, int any_hit, float* out_t, int* out_prim,
                             const int* prim_ref) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* r = rays + 8 * (size_t)i;
  f3 o = mk3(r[0], r[1], r[2]), d = mk3(r[3], r[4], r[5]);
  Counters c = {0, 0, 0, 0, 0, 0};
  if (any_hit) {
    bool h = trace_any(S, o, d, r[6], r[7], c);
    out_t[i] = h ? 0.0f : INFINITY;
    out_prim[i] = h ? 0 : -1;
  } else {
    Hit h;
    bool ok = trace_closest(S, o, d, r[6], r[7], h, c);
    out_t[i] = ok ? h.t : INFINITY;
    out_prim[i] = ok ? prim_ref[h.prim] : -1;
  }
}

__global__ void k_combine(const float* a, const float* b, float* out, long long n) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = a[i] + b[i];
}

// The LDS mode of a BDPT launch and the dynamic LDS it needs (wave queues + the scene copy).
int pick_lm(Ctx* c, KParams& kp, size_t* lds) {
  size_t treelet_max = kLdsSceneMax - kLdsStackBytes;
  if (c->env_ntop_max >= 0)   // diagnostics: BDPT_NTOP_MAX caps the treelet's nodes
    treelet_max = std::min(treelet_max, (size_t)c->env_ntop_max * node_bytes(lm_width(2)));
  const LdsPlan p = lds_plan(c->hs, c->env_lds_mode, kLdsSceneMax, treelet_max);
  apply_plan(c, p, kp);
  // LM 2 always gives the stacks their LDS slots (the treelet makes room); LM 1 when the whole
  // scene and the slots fit together (CBgems: +0.5 .. +0.8 %, profiles/r04o_ab_stack_lm1.log)
  kp.lstack_on = p.lm == 2 || (p.lm == 1 && p.full_bytes + kLdsStackBytes <= kLdsSceneMax);
  *lds = kWavesPerBlock * sizeof(WaveQ) + (kp.lstack_on ? kLdsStackBytes : 0) + p.copy_bytes;
  return p.lm;
}

// Whether k_bdpt_sample copies the materials and lights to its static LDS arrays: the predicate
// stage_scene evaluates, on the host for bdpt_debug_launch_plan.
bool mats_lights_staged(const KParams& kp) { return kp.nmat <= kLdsMats && kp.S.nlights <= kLdsLights; }

// launch_persistent for the LDS mode lm, on record as the context's last launch
// (bdpt_debug_launch_plan, bdpt_stats.lds_mode). launch(LM, grid_out) is the launch_persistent call.
template <class F>
int launch_recorded(Ctx* c, int lm, size_t lds, long long items, F&& launch) {
  int grid = 0;
  c->last_lm = lm;
  const int rc = dispatch_lm(lm, [&](auto LM) { return launch(LM, &grid); });
  if (grid > 0) {
    c->last_plan[2] = (int)lds;
    c->last_plan[3] = grid;
    c->last_plan[5] = (int)items;
  }
  return rc;
}

template <int MAXV, bool STATS, int EXT>
int launch_lm(Ctx* c, KParams& kp) {
  size_t lds = 0;
  const int lm = pick_lm(c, kp, &lds);
  c->last_plan[0] = kp.lstack_on;
  c->last_plan[1] = kp.S.ntop;
  c->last_plan[4] = kp.spl;
  c->last_plan[6] = mats_lights_staged(kp) ? 1 : 0;
  return launch_recorded(c, lm, lds, kp.nitems, [&](auto LM, int* grid) {
    return launch_persistent(c, k_bdpt_sample<MAXV, STATS, decltype(LM)::value, EXT>, "k_bdpt_sample", lds, kp, kp.nitems, grid);
  });
}

template <int MAXV>
int launch_maxv(Ctx* c, KParams& kp) {
  // the thin-lens flavour (§9b): instantiated in bdpt_lens.hip
  if (c->ext == 3) return c->prm.collect_stats ? launch_lm<MAXV, true, 3>(c, kp) : launch_lm<MAXV, false, 3>(c, kp);
  if (c->ext == 2) return c->prm.collect_stats ? launch_lm<MAXV, true, 2>(c, kp) : launch_lm<MAXV, false, 2>(c, kp);
  if (c->ext) return c->prm.collect_stats ? launch_lm<MAXV, true, 1>(c, kp) : launch_lm<MAXV, false, 1>(c, kp);
  return c->prm.collect_stats ? launch_lm<MAXV, true, 0>(c, kp) : launch_lm<MAXV, false, 0>(c, kp);
}

template <bool STATS>
int launch_pt(Ctx* c, PtKParams& kp) {
  const LdsPlan p = lds_plan(c->hs, c->env_lds_mode, kLdsCopyOnlyMax, kLdsCopyOnlyMax);
  apply_plan(c, p, kp);
  kp.n_geom4 = (int)(c->hs.geom.size() / 4);
  c->last_plan[0] = c->last_plan[4] = c->last_plan[6] = -1;   // k_pt: no stack slots, chunks or material copy
  c->last_plan[1] = kp.S.ntop;
  return launch_recorded(c, p.lm, p.copy_bytes, kp.nblocks, [&](auto LM, int* grid) {
    return launch_persistent(c, k_pt<STATS, decltype(LM)::value>, "k_pt", p.copy_bytes, kp, kp.nblocks, grid);
  });
}

void free_ctx(Ctx* c) {
  if (!c) return;
  void* bufs[] = {c->d_nodes2, c->d_nodes4, c->d_geom, c->d_shade, c->d_mats, c->d_lights, c->d_prim_ref, c->d_env, c->d_count, c->d_work8, c->d_leaves,
                  c->d_eye, c->d_light, c->d_sample, c->d_stats, c->d_features, c->d_denoised, c->d_dn_scratch,
                  c->d_feat_blocks, c->d_moments, c->d_variance, c->d_var_scratch, c->d_adapt_rec, c->d_adapt_rounds,
                  c->d_adapt_list, c->d_adapt_counts, c->d_adapt_out};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  if (c->h_adapt_counts) (void)hipHostFree(c->h_adapt_counts);
  if (c->adapt_ev) (void)hipEventDestroy(c->adapt_ev);
  for (Ctx::BlockSlot& b : c->blk) {
    if (b.d) (void)hipFree(b.d);
    if (b.h) (void)hipHostFree(b.h);
    if (b.done) (void)hipEventDestroy(b.done);
  }
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  if (c->own) (void)hipStreamDestroy(c->own);
  delete c;
}

template <class T>
int upload(T** dst, const std::vector<T>& v) {
  size_t bytes = std::max<size_t>(sizeof(T), v.size() * sizeof(T));
  HIPCHK(hipMalloc((void**)dst, bytes));
  if (!v.empty()) HIPCHK(hipMemcpy(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return BDPT_OK;
}

}  // namespace

extern "C" {

int bdpt_abi_version(void) { return BDPT_ABI_VERSION; }
const char* bdpt_last_error(void) { return g_err.c_str(); }

int bdpt_create(const bdpt_scene_desc* scene, const bdpt_params* params, void** ctx_out) {
  if (!scene || !params || !ctx_out) { g_err = "null argument"; return BDPT_E_INVALID; }
  *ctx_out = nullptr;
  const bdpt_params& p = *params;
  if (p.width <= 0 || p.height <= 0 || p.spp <= 0 || p.max_depth < 0) {
    g_err = "invalid frame size / spp / max_depth";
    return BDPT_E_INVALID;
  }
  // the kernels hold a subpath in a fixed array: instantiations for m <= 5, 8, 16, 32, 62 and 126
  // (the reference's vectors have no cap, bidirection.cpp:84-86; deeper paths are rejected cleanly:
  // a subpath's vertex index must fit the 128-bit delta masks)
  int need = p.max_depth < 1 ? 1 : p.max_depth;
  if (need > kMaxDepth) {
    g_err = "max_depth " + std::to_string(p.max_depth) + " > " + std::to_string(kMaxDepth) +
            ": the deepest kernel holds subpaths of up to 126 bounces";
    return BDPT_E_UNSUPPORTED;
  }
  // 0 = auto = 1: the persistent megakernel. 2 was the wavefront pipeline (per-bounce kernels with
  // ballot-compacted ray queues), retired in round 5 after it had fallen to 0.32-0.50x of the
  // megakernel and never ran the environment light / roulette.
  if (p.integrator == BDPT_INTEGRATOR_PT && p.max_depth > kPtMaxVerts) {   // k_pt records <= 21 vertices
    g_err = "PathTracer max_depth " + std::to_string(p.max_depth) + " > " + std::to_string(kPtMaxVerts) +
            ": its walk records up to 21 vertices (the reference's own roulette cap, pathtracer.cpp:215)";
    return BDPT_E_UNSUPPORTED;
  }
  if (p.pipeline == 2) {
    g_err = "pipeline 2 (wavefront) was retired: it ran at 0.32-0.50x of the megakernel (DESIGN.md §5); use 0 or 1";
    return BDPT_E_UNSUPPORTED;
  }
  if (p.pipeline < 0 || p.pipeline > 2) { g_err = "bad pipeline (0 = auto, 1 = megakernel)"; return BDPT_E_INVALID; }
  Ctx* c = new Ctx();
  c->prm = p;
  c->maxv = maxv_class(p.max_depth);
  // diagnostics / A-B switches, read once per ctx (tests set them before bdpt_create)
  auto env_int = [](const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; };
  c->env_lds_mode = env_int("BDPT_LDS_MODE", -1);
  c->env_ntop_max = env_int("BDPT_NTOP_MAX", -1);
  c->block_major = env_int("BDPT_BLOCK_MAJOR", 1);
  c->xcd = env_int("BDPT_XCD_GROUPS", 0);
  if (c->env_lds_mode > 3) { g_err = "BDPT_LDS_MODE must be 0..3"; delete c; return BDPT_E_INVALID; }
  c->pt = p.integrator == BDPT_INTEGRATOR_PT;
  if (p.integrator != BDPT_INTEGRATOR_BDPT && !c->pt) { g_err = "unknown integrator"; delete c; return BDPT_E_INVALID; }
  if (c->pt && (p.ns_area_light < 0 || p.samples_per_batch < 0 || p.lens_radius < 0)) {
    g_err = "invalid PathTracer settings"; delete c; return BDPT_E_INVALID;
  }
  int rc = build_host_scene(scene, c->hs, g_err, c->pt, p.infinite_lights != 0);
  if (rc) { delete c; return rc; }
  // host-side shape check before anything runs: each tree holds whole nodes of the stride its
  // kernels read (hs.tree(lm_width(LM)) is what view_of hands the LDS mode LM)
  for (int lm = 0; lm < 3; lm++) {
    const int W = lm_width(lm);
    if (c->hs.tree(W).nodes.size() % (4 * (size_t)node_f4(W)) != 0) {
      g_err = "device tree layout does not match the kernels' node width";
      delete c;
      return BDPT_E_INVALID;
    }
  }
  // the speculative loop of traverse<LM 0 / 2> reaches a leaf only out of a node step: started on a
  // leaf reference it never ends, so the 4-wide tree's root must be a node (bdpt_scene.cpp emits a
  // one-slot node around a leaf root)
  if (c->hs.nprim > 0 && c->hs.bvh4.root < 0) {
    g_err = "device tree: the 4-wide tree's root is a leaf reference (the 4-wide traversal needs a node)";
    delete c;
    return BDPT_E_UNSUPPORTED;
  }
  // bdpt_params.lens_radius > 0 under BDPT: the thin lens (§9b); <= 0 the pinhole, as before
  const bool lens = !c->pt && p.lens_radius > 0;
  c->hs.cam.lens_r = lens ? (float)p.lens_radius : 0.0f;
  c->ext = kernel_flavour(c->hs, p.russian_roulette != 0, lens);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    g_err = "no HIP device";
    delete c;
    return BDPT_E_DEVICE;
  }
  if (p.device < 0 || p.device >= ndev) { g_err = "bad device ordinal"; delete c; return BDPT_E_INVALID; }
  c->device = p.device;
  auto fail = [&](int code) { free_ctx(c); return code; };
  if (hipSetDevice(c->device) != hipSuccess) { g_err = "hipSetDevice failed"; return fail(BDPT_E_DEVICE); }
  if (hipDeviceGetAttribute(&c->ncu, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || c->ncu <= 0)
    c->ncu = 256;
  if ((rc = upload(&c->d_nodes2, c->hs.bvh2.nodes))) return fail(rc);
  if ((rc = upload(&c->d_nodes4, c->hs.bvh4.nodes))) return fail(rc);
  if ((rc = upload(&c->d_geom, c->hs.geom))) return fail(rc);
  if ((rc = upload(&c->d_shade, c->hs.shade))) return fail(rc);
  if ((rc = upload(&c->d_mats, c->hs.mats))) return fail(rc);
  if ((rc = upload(&c->d_lights, c->hs.lights))) return fail(rc);
  if ((rc = upload(&c->d_prim_ref, c->hs.prim_ref))) return fail(rc);
  if ((rc = upload(&c->d_leaves, c->hs.leaf_refs))) return fail(rc);
  if (c->hs.env_light >= 0 && (rc = upload(&c->d_env, c->hs.env))) return fail(rc);
  c->npix = (size_t)p.width * p.height;
  size_t fb = c->npix * 3 * sizeof(float);
  if ((rc = ensure_alloc(&c->d_eye, fb)) || (rc = ensure_alloc(&c->d_light, fb)) || (rc = ensure_alloc(&c->d_sample, fb)) ||
      (rc = ensure_alloc(&c->d_count, c->npix * sizeof(int))) || (rc = ensure_alloc(&c->d_work8, 8 * 32 * sizeof(unsigned))) ||
      (rc = ensure_alloc(&c->d_stats, Ctx::kStatSlots * sizeof(unsigned long long))))
    return fail(rc);
  bool ev_ok = true;
  for (Ctx::BlockSlot& b : c->blk) ev_ok = ev_ok && hipEventCreateWithFlags(&b.done, hipEventDisableTiming) == hipSuccess;
  if (!ev_ok || hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess) {
    g_err = "stream/event creation failed";
    return fail(BDPT_E_DEVICE);
  }
  c->stream = c->own;
  // the frames, the sample counts and the stat slots start at zero, as after bdpt_clear
  if (bdpt_clear(c) != BDPT_OK || hipStreamSynchronize(c->stream) != hipSuccess) { g_err = "init sync failed"; return fail(BDPT_E_DEVICE); }
  *ctx_out = c;
  return BDPT_OK;
}

void bdpt_destroy(void* ctx) {
  Ctx* c = (Ctx*)ctx;
  if (!c) return;
  {
    std::lock_guard<std::recursive_mutex> lk(c->mu);   // waits for a call in flight on another thread
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
  }
  free_ctx(c);
}

int bdpt_set_stream(void* ctx, void* stream) {
  Ctx* c = (Ctx*)ctx;
  if (!c) { g_err = "null ctx"; return BDPT_E_INVALID; }
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  c->stream = stream ? (hipStream_t)stream : c->own;
  return BDPT_OK;
}

int bdpt_clear(void* ctx) {
  Ctx* c = (Ctx*)ctx;
  if (!c) { g_err = "null ctx"; return BDPT_E_INVALID; }
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  HIPCHK(hipSetDevice(c->device));
  size_t fb = c->npix * 3 * sizeof(float);
  HIPCHK(hipMemsetAsync(c->d_eye, 0, fb, c->stream));
  HIPCHK(hipMemsetAsync(c->d_light, 0, fb, c->stream));
  HIPCHK(hipMemsetAsync(c->d_count, 0, c->npix * sizeof(int), c->stream));
  HIPCHK(hipMemsetAsync(c->d_stats, 0, Ctx::kStatSlots * sizeof(unsigned long long), c->stream));
  if (c->d_features) HIPCHK(hipMemsetAsync(c->d_features, 0, c->npix * 8 * sizeof(float), c->stream));
  // the batch moments (bdpt_variance.hip) start over with the frame
  if (c->d_moments) HIPCHK(hipMemsetAsync(c->d_moments, 0, c->npix * 4 * sizeof(float), c->stream));
  c->var_batches = c->var_batch_spp = 0;
  c->var_unbatched = c->variance_valid = false;
  // the adaptive records, round counts and flags (bdpt_adaptive.hip) start over too
  if (c->d_adapt_rec) HIPCHK(hipMemsetAsync(c->d_adapt_rec, 0, 2 * c->npix * 4 * sizeof(float), c->stream));
  if (c->d_adapt_rounds)
    HIPCHK(hipMemsetAsync(c->d_adapt_rounds, 0, 2 * (size_t)((c->prm.width + 7) / 8) * ((c->prm.height + 7) / 8) * sizeof(int), c->stream));
  c->adapt_rounds = c->adapt_m = c->adapt_active = 0;
  c->adapt_n = 0;
  c->frame_dirty = c->adapt_valid = c->adapt_resolved = false;
  return BDPT_OK;
}

int bdpt_render(void* ctx, const bdpt_tile* tiles, int32_t ntiles, int32_t spp_begin, int32_t spp_count) {
  Ctx* c = (Ctx*)ctx;
  if (!c) { g_err = "null ctx"; return BDPT_E_INVALID; }
  if (spp_begin < 0 || spp_count < 0 || ntiles < 0) { g_err = "negative argument"; return BDPT_E_INVALID; }
  if ((int64_t)spp_begin + spp_count > INT32_MAX) { g_err = "spp_begin + spp_count overflows int32"; return BDPT_E_INVALID; }
  if (spp_count == 0) return BDPT_OK;
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  if (!c->in_batches) c->var_unbatched = true;   // samples outside bdpt_render_batches: no variance of this frame
  c->frame_dirty = true;                         // bdpt_render_adaptive starts from a cleared frame only,
  c->adapt_valid = false;                        // and its per-block estimate no longer describes this one
  HIPCHK(hipSetDevice(c->device));
  const int W = c->prm.width, H = c->prm.height;
  const int4* d_blocks = nullptr;
  int nblocks = 0;
  Ctx::BlockSlot* slot = nullptr;
  if (tiles && ntiles > 0) {
    std::vector<int4> blk;
    tiles_to_blocks(tiles, ntiles, W, H, blk);
    if (blk.empty()) return BDPT_OK;
    // next slot of the staging ring: wait only for the launch that last read it
    slot = &c->blk[c->blk_next];
    c->blk_next = (c->blk_next + 1) % Ctx::kBlockSlots;
    if (slot->pending) HIPCHK(hipEventSynchronize(slot->done));
    slot->pending = false;
    if (blk.size() > slot->cap) {
      if (slot->d) { (void)hipFree(slot->d); slot->d = nullptr; }
      if (slot->h) { (void)hipHostFree(slot->h); slot->h = nullptr; }
      slot->cap = 0;
      HIPCHK(hipMalloc((void**)&slot->d, blk.size() * sizeof(int4)));
      HIPCHK(hipHostMalloc((void**)&slot->h, blk.size() * sizeof(int4)));
      slot->cap = blk.size();
    }
    memcpy(slot->h, blk.data(), blk.size() * sizeof(int4));
    HIPCHK(hipMemcpyAsync(slot->d, slot->h, blk.size() * sizeof(int4), hipMemcpyHostToDevice, c->stream));
    d_blocks = slot->d;
    nblocks = (int)blk.size();
  }
  // the slot is free again once everything enqueued below has run (on every return path)
  struct SlotRelease {
    Ctx::BlockSlot* s;
    hipStream_t st;
    ~SlotRelease() {
      if (s && hipEventRecord(s->done, st) == hipSuccess) s->pending = true;
      else if (s) (void)hipStreamSynchronize(st);
    }
  } slot_release{slot, c->stream};
  return render_blocks(c, d_blocks, nblocks, spp_begin, spp_count);
}

}  // extern "C"

// The second half of bdpt_render: the launch over a device list of 8x8 pixel blocks (null: the frame).
int bdpt::render_blocks(Ctx* c, const int4* d_blocks, int nblocks, int spp_begin, int spp_count) {
  const int W = c->prm.width, H = c->prm.height;
  KParams kp;
  kp.S = view_of(c, 0);   // launch_lm sets the LDS mode's view
  kp.sp.W = W; kp.sp.H = H; kp.sp.spp = c->prm.spp; kp.sp.max_depth = c->prm.max_depth; kp.sp.seed = c->prm.seed;
  kp.sp.rr = c->prm.russian_roulette != 0;
  kp.sp.focal = lens_focal(c->prm.focal_distance);   // read by the lens kernels only (§9b)
  kp.eye = c->d_eye;
  kp.light = c->d_light;
  kp.stats = c->d_stats;
  kp.prof = c->d_stats + 16;
  kp.n_geom4 = (int)(c->hs.geom.size() / 4);
  kp.nmat = (int)c->hs.mats.size();
  kp.item_lo = 0;
  kp.lstack_on = 0;
  kp.blocks = d_blocks;
  kp.nbx = (W + 7) / 8;
  kp.nblocks = d_blocks ? nblocks : kp.nbx * ((H + 7) / 8);
  if (c->pt) {   // the PathTracer renders whole pixels (adaptive sampling decides per pixel)
    if (spp_begin != 0 || spp_count != c->prm.spp) {
      g_err = "the PathTracer renders whole pixels: spp_begin must be 0 and spp_count the ctx's spp";
      return BDPT_E_INVALID;
    }
    PtKParams pk;
    pk.pp.W = W; pk.pp.H = H; pk.pp.spp = c->prm.spp; pk.pp.max_depth = c->prm.max_depth;
    pk.pp.seed = c->prm.seed;
    pk.pp.ns_area_light = c->prm.ns_area_light > 0 ? c->prm.ns_area_light : 1;
    pk.pp.batch = c->prm.samples_per_batch > 0 ? c->prm.samples_per_batch : 32;
    pk.pp.hemisphere = c->prm.direct_hemisphere_sample != 0;
    pk.pp.tol = c->prm.max_tolerance;
    pk.pp.lens_radius = (float)c->prm.lens_radius;
    pk.pp.focal_distance = pt_focal(c->prm);
    pk.eye = c->d_eye;
    pk.count = c->d_count;
    pk.stats = c->d_stats;
    pk.blocks = kp.blocks;
    pk.nblocks = kp.nblocks;
    pk.nbx = kp.nbx;
    if (!(pk.work = reset_tickets(c))) return BDPT_E_DEVICE;
    HIPCHK(hipEventRecord(c->ev0, c->stream));
    int rc = c->prm.collect_stats ? launch_pt<true>(c, pk) : launch_pt<false>(c, pk);
    if (rc) return rc;
    HIPCHK(hipEventRecord(c->ev1, c->stream));
    c->timed = true;
    return BDPT_OK;
  }
  int spl = c->prm.samples_per_lane;
  if (spl <= 0) {
    // small work items (8x8 pixels x 2 samples): measured against the earlier "~16 items per
    // co-resident wave" rule (spl 6 on C2, 43 on the 1080p stand-in): C2 586 -> 591, Lucy stand-in
    // 1080p 532 -> 536-539 Msamples/s; with block-major order spl 2 vs 4: CBgems 313 vs 305, C2 and
    // the stand-in equal; spl 8 / 16 / 32 lose 1-14% (tools/gpu_spl.sh)
    spl = (int)std::min<long long>(spp_count, 2);
  }
  kp.spl = spl;
  kp.spp_begin = spp_begin;
  kp.spp_end = spp_begin + spp_count;
  const long long nchunks = (spp_count + spl - 1) / spl;
  const long long nitems = nchunks * kp.nblocks;
  if (nitems >= 0x7fffffffLL) { g_err = "launch too large; split spp"; return BDPT_E_INVALID; }
  kp.nitems = (unsigned)nitems;
  kp.nchunks = (unsigned)nchunks;
  // consecutive tickets take one pixel block's sample chunks in turn (measured: C2 +1.2%, CBgems
  // +2%, Lucy stand-in 1080p +-0 over chunk-major order); BDPT_BLOCK_MAJOR=0 restores chunk-major
  kp.block_major = c->block_major;
  if (!(kp.work = reset_tickets(c))) return BDPT_E_DEVICE;
  kp.work8 = c->d_work8;
  kp.region = (kp.nitems + 7u) / 8u;
  kp.xcd = c->xcd;
  if (kp.xcd) HIPCHK(hipMemsetAsync(kp.work8, 0, 8 * 32 * sizeof(unsigned), c->stream));
  HIPCHK(hipEventRecord(c->ev0, c->stream));
#ifdef BDPT_ONLY_MAXV   // A/B variant builds (tools/build_variants.sh): one depth class, a faster compile
  if (c->maxv != BDPT_ONLY_MAXV) { g_err = "variant build: only max_depth class " BDPT_STR(BDPT_ONLY_MAXV); return BDPT_E_UNSUPPORTED; }
  int rc = launch_maxv<BDPT_ONLY_MAXV>(c, kp);
#else
  int rc = c->maxv == 5 ? launch_maxv<5>(c, kp) : c->maxv == 8 ? launch_maxv<8>(c, kp)
           : c->maxv == 16 ? launch_maxv<16>(c, kp) : c->maxv == 32 ? launch_maxv<32>(c, kp)
           : c->maxv == 62 ? launch_maxv<62>(c, kp) : launch_maxv<126>(c, kp);
#endif
  if (rc) return rc;
  HIPCHK(hipEventRecord(c->ev1, c->stream));
  c->timed = true;
  return BDPT_OK;
}

extern "C" {

int bdpt_sync(void* ctx) {
  Ctx* c = (Ctx*)ctx;
  if (!c) { g_err = "null ctx"; return BDPT_E_INVALID; }
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  return BDPT_OK;
}

int bdpt_frame_device_ptr(void* ctx, int32_t which, void** dptr) {
  Ctx* c = (Ctx*)ctx;
  if (!c || !dptr) { g_err = "null argument"; return BDPT_E_INVALID; }
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  HIPCHK(hipSetDevice(c->device));
  if (which == BDPT_FRAME_EYE) { *dptr = c->d_eye; return BDPT_OK; }
  if (which == BDPT_FRAME_LIGHT) { *dptr = c->d_light; return BDPT_OK; }
  if (which != BDPT_FRAME_SAMPLE) { g_err = "bad frame id"; return BDPT_E_INVALID; }
  long long n = (long long)c->npix * 3;
  hipLaunchKernelGGL(k_combine, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->d_eye, c->d_light,
                     c->d_sample, n);
  HIPCHK(hipGetLastError());
  *dptr = c->d_sample;
  return BDPT_OK;
}

int bdpt_copy_frame(void* ctx, int32_t which, void* dst_device) {
  Ctx* c = (Ctx*)ctx;
  if (!c || !dst_device) { g_err = "null argument"; return BDPT_E_INVALID; }
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  void* p = nullptr;
  int rc = bdpt_frame_device_ptr(ctx, which, &p);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(dst_device, p, c->npix * 3 * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  return BDPT_OK;
}

int bdpt_read_frame(void* ctx, int32_t which, float* rgb) {
  Ctx* c = (Ctx*)ctx;
  if (!c || !rgb) { g_err = "null argument"; return BDPT_E_INVALID; }
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  void* p = nullptr;
  int rc = bdpt_frame_device_ptr(ctx, which, &p);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(rgb, p, c->npix * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return BDPT_OK;
}

int bdpt_read_frame_rect(void* ctx, int32_t which, int32_t x0, int32_t y0, int32_t w, int32_t h, float* rgb) {
  Ctx* c = (Ctx*)ctx;
  if (!c || !rgb) { g_err = "null argument"; return BDPT_E_INVALID; }
  const int W = c->prm.width, H = c->prm.height;
  if (x0 < 0 || y0 < 0 || w < 0 || h < 0 || (int64_t)x0 + w > W || (int64_t)y0 + h > H) {
    g_err = "rectangle outside the frame";
    return BDPT_E_INVALID;
  }
  if (w == 0 || h == 0) return BDPT_OK;
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  void* p = nullptr;
  int rc = bdpt_frame_device_ptr(ctx, which, &p);
  if (rc) return rc;
  const size_t row = (size_t)W * 3 * sizeof(float);
  HIPCHK(hipMemcpy2DAsync(rgb, (size_t)w * 3 * sizeof(float), (const char*)p + ((size_t)y0 * W + x0) * 3 * sizeof(float), row,
                          (size_t)w * 3 * sizeof(float), (size_t)h, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return BDPT_OK;
}

int bdpt_read_sample_counts(void* ctx, int32_t* counts) {
  Ctx* c = (Ctx*)ctx;
  if (!c || !counts) { g_err = "null argument"; return BDPT_E_INVALID; }
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (c->pt) {
    HIPCHK(hipMemcpy(counts, c->d_count, c->npix * sizeof(int), hipMemcpyDeviceToHost));
  } else {   // BidirectionalPathTracer::raytrace_pixel records ns_aa (bidirection.cpp:539)
    for (size_t k = 0; k < c->npix; k++) counts[k] = c->prm.spp;
  }
  return BDPT_OK;
}

int bdpt_get_stats(void* ctx, bdpt_stats* out) {
  Ctx* c = (Ctx*)ctx;
  if (!c || !out) { g_err = "null argument"; return BDPT_E_INVALID; }
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  unsigned long long s[16];
  HIPCHK(hipMemcpy(s, c->d_stats, sizeof s, hipMemcpyDeviceToHost));
  memset(out, 0, sizeof *out);
  out->samples = s[0];
  out->closest_rays = s[1];
  out->shadow_rays = s[2];
  out->rays = s[1] + s[2];
  out->node_visits = s[3];
  out->tri_tests = s[4];
  out->sph_tests = s[5];
  out->hits = s[6];
  float ms = 0;
  if (c->timed) HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
  out->last_kernel_ms = ms;
  out->bvh_nodes = (uint64_t)c->hs.ref_nodes;
  out->bvh_depth = (uint64_t)c->hs.depth;
  out->lds_node_visits = s[7];
  out->lds_mode = c->last_lm;
  out->env_samples = s[12];
  out->env_lookups = s[13];
  out->env_pdf_lookups = s[14];
  return BDPT_OK;
}

// 16 of the stat slots (Ctx::d_stats) from slot `first` on, once the stream has drained.
static int read_stat_slots(void* ctx, int first, uint64_t* out16) {
  Ctx* c = (Ctx*)ctx;
  if (!c || !out16) { g_err = "null argument"; return BDPT_E_INVALID; }
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy(out16, c->d_stats + first, 16 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return BDPT_OK;
}

int bdpt_debug_lane_counters(void* ctx, uint64_t* out16) { return read_stat_slots(ctx, 32, out16); }
int bdpt_debug_counters(void* ctx, uint64_t* out16) { return read_stat_slots(ctx, 16, out16); }

int bdpt_debug_launch_plan(void* ctx, int32_t* out8) {
  Ctx* c = (Ctx*)ctx;
  if (!c || !out8) { g_err = "null argument"; return BDPT_E_INVALID; }
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  out8[0] = c->last_lm;
  for (int k = 0; k < 7; k++) out8[1 + k] = c->last_plan[k];
  return BDPT_OK;
}

int bdpt_trace_rays(void* ctx, const float* rays, int32_t n, int32_t any_hit, float* out_t, int32_t* out_prim) {
  Ctx* c = (Ctx*)ctx;
  if (!c || (!rays && n) || n < 0) { g_err = "bad argument"; return BDPT_E_INVALID; }
  if (n == 0) return BDPT_OK;
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  HIPCHK(hipSetDevice(c->device));
  float *d_r = nullptr, *d_t = nullptr;
  int* d_p = nullptr;
  struct Frees {   // every exit path (HIPCHK returns early) releases the temporaries
    void** p[3];
    ~Frees() { for (void** q : p) if (*q) (void)hipFree(*q); }
  } frees{{(void**)&d_r, (void**)&d_t, (void**)&d_p}};
  HIPCHK(hipMalloc((void**)&d_r, (size_t)n * 8 * sizeof(float)));
  HIPCHK(hipMalloc((void**)&d_t, (size_t)n * sizeof(float)));
  HIPCHK(hipMalloc((void**)&d_p, (size_t)n * sizeof(int)));
  HIPCHK(hipMemcpy(d_r, rays, (size_t)n * 8 * sizeof(float), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_trace_rays, dim3((n + 127) / 128), dim3(128), 0, c->stream, view_of(c, 0), d_r, n, any_hit,
                     d_t, d_p, c->d_prim_ref);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy(out_t, d_t, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(out_prim, d_p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
  return BDPT_OK;
}

}  // extern "C"
