// bdpt_denoise.hip — denoised output: the first-hit feature pass (k_features,
// bdpt_features.h) and the edge-avoiding a-trous filter (k_atrous, bdpt_atrous.h), with their
// C-ABI (bdpt_render_features .. bdpt_denoise_buffers). A translation unit of its own, like
// bdpt_lens.hip: it reuses bdpt_megakernel.h's helpers and leaves the other kernels' code alone.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see __graft_entry__.build).

#include <hip/hip_runtime.h>

#include <mutex>
#include <string>

#include "bdpt/bdpt.h"
#include "bdpt_atrous.h"
#include "bdpt_features.h"
#include "bdpt_launch.h"   // bdpt_ctx.h, bdpt_megakernel.h, bdpt_ldsplan.h
#include "bdpt_tile.h"

using namespace bdpt;

namespace {

// ------------------------------------------------------------------------------------------------
// The feature pass. k_features is k_pt's shape (bdpt_hip.hip): persistent waves take 8x8 pixel
// blocks from a ticket counter, the block stages its LDS copy of the scene, a lane owns one pixel,
// loops over its samples and stores the record once (two 16-byte stores). No atomics on the frame.
struct FeatKParams {
  SceneView S;
  FeatParams fp;
  float* feat;                // W*H*8
  const int4* blocks;
  int nblocks, nbx;
  unsigned* work;
  int n_node4, n_geom4;
};

template <int LM>
__global__ __launch_bounds__(kBlock, kMinWaves) void k_features(FeatKParams kp) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63;
  stage_lds_scene<LM>(kp.S, kp.n_node4, kp.n_geom4, (float4*)smem);
  Counters cnt = {0, 0, 0, 0, 0, 0};
  for (;;) {
    unsigned item = 0;
    if (lane == 0) item = atomicAdd(kp.work, 1u);
    item = __shfl(item, 0, 64);
    if (item >= (unsigned)kp.nblocks) break;
    int x, y;
    if (block_pixel(kp.blocks, kp.nbx, kp.fp.W, kp.fp.H, (int)item, lane, x, y)) {
      float r[8];
      feature_pixel<LM>(kp.S, kp.fp, cnt, x, y, r);
      float4* out = (float4*)kp.feat + 2 * ((size_t)x + (size_t)y * kp.fp.W);
      out[0] = make_float4(r[0], r[1], r[2], r[3]);
      out[1] = make_float4(r[4], r[5], r[6], r[7]);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// The filter. One launch per level over the wave tiles of bdpt_tile.h. No LDS: from step 4 on
// neighbouring tiles share no taps, and the frames sit in L2 / the Infinity Cache.
__global__ __launch_bounds__(kAtrousBlock) void k_atrous(const float* c_in, const float* F, float* c_out, AtrousLevel L) {
  int x, y;
  if (!tile_pixel(L.W, L.H, x, y)) return;
  const f3 v = atrous_pixel(c_in, F, L, x, y);
  const size_t p = (size_t)x + (size_t)y * L.W;
  c_out[3 * p] = v.x;
  c_out[3 * p + 1] = v.y;
  c_out[3 * p + 2] = v.z;
}

// mode 0: copy, 1: demod_in (before level 0), 2: demod_out (after the last level)
__global__ __launch_bounds__(kAtrousBlock) void k_modulate(const float* c_in, const float* F, float* c_out, int W, int H, int mode) {
  int x, y;
  if (!tile_pixel(W, H, x, y)) return;
  const size_t p = (size_t)x + (size_t)y * W;
  f3 v = mk3(c_in[3 * p], c_in[3 * p + 1], c_in[3 * p + 2]);
  if (mode == 1) v = demod_in(v, load_feat(F, p));
  else if (mode == 2) v = demod_out(v, load_feat(F, p));
  c_out[3 * p] = v.x;
  c_out[3 * p + 1] = v.y;
  c_out[3 * p + 2] = v.z;
}

int check_denoise_params(const bdpt_denoise_params* p, bdpt_denoise_params* out) {
  bdpt_denoise_params d;
  d.levels = kDenoiseLevels;
  d.sigma_color = kDenoiseSigmaColor;
  d.sigma_normal = kDenoiseSigmaNormal;
  d.sigma_depth = kDenoiseSigmaDepth;
  d.demodulate = kDenoiseDemodulate;
  d.reserved[0] = d.reserved[1] = d.reserved[2] = 0;
  if (p) d = *p;
  if (d.levels < 0 || d.levels > kDenoiseMaxLevels) { g_err = "denoise levels must be 0..8"; return BDPT_E_INVALID; }
  if (!(d.sigma_color > 0) || !(d.sigma_normal > 0) || !(d.sigma_depth > 0)) { g_err = "denoise sigmas must be > 0"; return BDPT_E_INVALID; }
  if (d.demodulate != 0 && d.demodulate != 1) { g_err = "denoise demodulate must be 0 or 1"; return BDPT_E_INVALID; }
  if (d.reserved[0] || d.reserved[1] || d.reserved[2]) { g_err = "bdpt_denoise_params.reserved must be 0"; return BDPT_E_INVALID; }
  *out = d;
  return BDPT_OK;
}

// Enqueues the filter: color -> out through the two scratch frames s[0], s[1] (W*H*3 each). Level i
// reads the current frame and writes s[i & 1]; the last pass writes out, so out may be color.
int enqueue_filter(hipStream_t st, const float* color, const float* F, int W, int H, const bdpt_denoise_params& p,
                   float* out, float* s0, float* s1) {
  const dim3 grid = tile_grid(W, H), block(kAtrousBlock);
  float* s[2] = {s0, s1};
  const float* cur = color;
  if (p.demodulate) {
    hipLaunchKernelGGL(k_modulate, grid, block, 0, st, cur, F, s[1], W, H, 1);
    cur = s[1];
  }
  for (int i = 0; i < p.levels; i++) {
    const AtrousLevel L = atrous_level(W, H, i, p.sigma_color, p.sigma_normal, p.sigma_depth);
    hipLaunchKernelGGL(k_atrous, grid, block, 0, st, cur, F, s[i & 1], L);
    cur = s[i & 1];
  }
  if (cur != out) hipLaunchKernelGGL(k_modulate, grid, block, 0, st, cur, F, out, W, H, p.demodulate ? 2 : 0);
  HIPCHK(hipGetLastError());
  return BDPT_OK;
}

}  // namespace

extern "C" {

int bdpt_denoise_default_params(bdpt_denoise_params* p) {
  if (!p) { g_err = "null argument"; return BDPT_E_INVALID; }
  return check_denoise_params(nullptr, p);
}

int bdpt_render_features(void* ctx, const bdpt_tile* tiles, int32_t ntiles, int32_t spp_count) {
  Ctx* c = (Ctx*)ctx;
  if (!c) { g_err = "null ctx"; return BDPT_E_INVALID; }
  if (ntiles < 0 || (ntiles > 0 && !tiles)) { g_err = "bad tile list"; return BDPT_E_INVALID; }
  if (spp_count < 0 || spp_count > c->prm.spp) {
    g_err = "feature spp_count " + std::to_string(spp_count) + " outside 0.." + std::to_string(c->prm.spp) + " (the ctx's spp)";
    return BDPT_E_INVALID;
  }
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  HIPCHK(hipSetDevice(c->device));
  const int W = c->prm.width, H = c->prm.height;
  int rc = ensure_alloc(&c->d_features, c->npix * 8 * sizeof(float), &c->stream);
  if (rc) return rc;
  FeatKParams kp;
  kp.fp.W = W; kp.fp.H = H;
  kp.fp.nsamp = spp_count ? spp_count : c->prm.spp;
  kp.fp.seed = c->prm.seed;
  if (c->pt) {   // PtParams as bdpt_render fills them
    kp.fp.kind = FEAT_PT;
    kp.fp.lens_r = (float)c->prm.lens_radius;
    kp.fp.focal = pt_focal(c->prm);
  } else {
    kp.fp.kind = c->ext == 3 ? FEAT_BDPT_LENS : FEAT_BDPT;
    kp.fp.lens_r = 0.0f;
    kp.fp.focal = lens_focal(c->prm.focal_distance);
  }
  kp.feat = c->d_features;
  kp.blocks = nullptr;
  kp.nbx = (W + 7) / 8;
  kp.nblocks = kp.nbx * ((H + 7) / 8);
  if (ntiles > 0) {
    std::vector<int4> blk;
    tiles_to_blocks(tiles, ntiles, W, H, blk);
    if (blk.empty()) return BDPT_OK;
    // the list's device buffer may still be read by an earlier pass: wait, then upload
    HIPCHK(hipStreamSynchronize(c->stream));
    if (blk.size() > c->feat_blocks_cap) {
      if (c->d_feat_blocks) { (void)hipFree(c->d_feat_blocks); c->d_feat_blocks = nullptr; }
      c->feat_blocks_cap = 0;
      HIPCHK(hipMalloc((void**)&c->d_feat_blocks, blk.size() * sizeof(int4)));
      c->feat_blocks_cap = blk.size();
    }
    HIPCHK(hipMemcpy(c->d_feat_blocks, blk.data(), blk.size() * sizeof(int4), hipMemcpyHostToDevice));
    kp.blocks = c->d_feat_blocks;
    kp.nblocks = (int)blk.size();
  }
  // the plan k_pt gets (bdpt_hip.hip launch_pt), not on record as the context's last launch
  // (bdpt_debug_launch_plan, bdpt_stats.lds_mode)
  const LdsPlan p = lds_plan(c->hs, c->env_lds_mode, kLdsCopyOnlyMax, kLdsCopyOnlyMax);
  apply_plan(c, p, kp);
  kp.n_geom4 = (int)(c->hs.geom.size() / 4);
  if (!(kp.work = reset_tickets(c))) return BDPT_E_DEVICE;
  return dispatch_lm(p.lm, [&](auto LM) {
    return launch_persistent(c, k_features<decltype(LM)::value>, "k_features", p.copy_bytes, kp, kp.nblocks);
  });
}

static float* features_of(Ctx* c) { return c->d_features; }
static const char* const kNoFeatures = "no feature pass has run on this context (bdpt_render_features)";

int bdpt_read_features(void* ctx, float* out8) { return frame_out(ctx, features_of, kNoFeatures, 8 * sizeof(float), out8, nullptr); }
int bdpt_features_device_ptr(void* ctx, void** dptr) { return frame_out(ctx, features_of, kNoFeatures, 0, nullptr, dptr); }

int bdpt_denoise(void* ctx, int32_t which, const bdpt_denoise_params* p) {
  if (which != BDPT_FRAME_SAMPLE && which != BDPT_FRAME_EYE && which != BDPT_FRAME_LIGHT) { g_err = "bad frame id"; return BDPT_E_INVALID; }
  bdpt_denoise_params dp;
  int rc = check_denoise_params(p, &dp);
  if (rc) return rc;
  Ctx* c = (Ctx*)ctx;
  if (!c) { g_err = "null ctx"; return BDPT_E_INVALID; }
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  if (!c->d_features) { g_err = "bdpt_denoise needs a feature pass first (bdpt_render_features)"; return BDPT_E_INVALID; }
  HIPCHK(hipSetDevice(c->device));
  const size_t fb = c->npix * 3 * sizeof(float);
  if ((rc = ensure_alloc(&c->d_denoised, fb)) || (rc = ensure_alloc(&c->d_dn_scratch, 2 * fb))) return rc;
  void* src = nullptr;
  if ((rc = bdpt_frame_device_ptr(ctx, which, &src))) return rc;
  rc = enqueue_filter(c->stream, (const float*)src, c->d_features, c->prm.width, c->prm.height, dp, c->d_denoised,
                      c->d_dn_scratch, c->d_dn_scratch + c->npix * 3);
  if (rc) return rc;
  c->denoised_valid = true;
  return BDPT_OK;
}

static float* denoised_of(Ctx* c) { return c->denoised_valid ? c->d_denoised : nullptr; }
static const char* const kNoDenoised = "no denoised frame on this context (bdpt_denoise)";

int bdpt_read_denoised(void* ctx, float* rgb) { return frame_out(ctx, denoised_of, kNoDenoised, 3 * sizeof(float), rgb, nullptr); }
int bdpt_denoised_device_ptr(void* ctx, void** dptr) { return frame_out(ctx, denoised_of, kNoDenoised, 0, nullptr, dptr); }

int bdpt_denoise_buffers(int32_t device, const float* d_color, const float* d_features, int32_t w, int32_t h,
                         const bdpt_denoise_params* p, float* d_out, void* stream) {
  if (!d_color || !d_features || !d_out) { g_err = "null argument"; return BDPT_E_INVALID; }
  int rc = check_frame(device, w, h);
  if (rc) return rc;
  if (!aligned16(d_features)) { g_err = "d_features must be 16-byte aligned"; return BDPT_E_INVALID; }
  bdpt_denoise_params dp;
  if ((rc = check_denoise_params(p, &dp))) return rc;
  HIPCHK(hipSetDevice(device));
  const size_t n3 = (size_t)w * h * 3;
  float* scratch = nullptr;
  HIPCHK(hipMalloc((void**)&scratch, 2 * n3 * sizeof(float)));
  rc = enqueue_filter((hipStream_t)stream, d_color, d_features, w, h, dp, d_out, scratch, scratch + n3);
  const hipError_t e = hipStreamSynchronize((hipStream_t)stream);
  (void)hipFree(scratch);
  if (rc) return rc;
  HIPCHK(e);
  return BDPT_OK;
}

}  // extern "C"
