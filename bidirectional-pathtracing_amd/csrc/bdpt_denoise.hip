// bdpt_denoise.hip — denoised output: the first-hit feature pass (k_features,
// bdpt_features.h) and the edge-avoiding a-trous filter (k_atrous, bdpt_atrous.h), with their
// C-ABI (bdpt_render_features .. bdpt_denoise_buffers). A translation unit of its own, like
// bdpt_lens.hip: it reuses bdpt_megakernel.h's helpers and leaves the other kernels' code alone.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see __graft_entry__.build).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <mutex>
#include <string>
#include <vector>

#include "bdpt/bdpt.h"
#include "bdpt_atrous.h"
#include "bdpt_ctx.h"
#include "bdpt_features.h"
#include "bdpt_megakernel.h"

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

// The LDS plan k_pt gets (bdpt_hip.hip pick_lds_copy / launch_pt), restated: it must not record
// itself as the context's last launch (bdpt_debug_launch_plan, bdpt_stats.lds_mode).
constexpr size_t kLdsPerCu = 160 * 1024;
constexpr int kFlatMaxPrims = 24;
constexpr size_t kBlocksPerCu = 4 * kMinWaves / kWavesPerBlock;
constexpr size_t kFeatLdsMax = kLdsPerCu / kBlocksPerCu - 256;

int feature_lds_mode(const Ctx* c, FeatKParams& kp, size_t* lds) {
  const size_t full = (c->hs.tree(lm_width(1)).nodes.size() + c->hs.geom.size()) * sizeof(float);
  const size_t flat = 2 * c->hs.geom.size() * sizeof(float) + (c->hs.leaf_refs.size() + 3) / 4 * 16;
  const bool has_nodes = !c->hs.bvh2.nodes.empty();
  int lm = c->env_lds_mode >= 0 ? c->env_lds_mode
               : (c->hs.nprim <= kFlatMaxPrims && flat <= kFeatLdsMax) ? 3
               : (full <= kFeatLdsMax ? 1 : has_nodes ? 2 : 0);
  if (lm == 3 && flat > kFeatLdsMax) lm = 1;
  if (lm == 1 && full > kFeatLdsMax) lm = 2;
  if (lm == 2 && !has_nodes) lm = 0;
  kp.S = view_of(c, lm);
  kp.n_node4 = (int)(c->hs.tree(lm_width(lm)).nodes.size() / 4);
  kp.n_geom4 = (int)(c->hs.geom.size() / 4);
  if (lm == 2) kp.S.ntop = (int)std::min<size_t>((size_t)c->hs.tree(lm_width(2)).n_top, kFeatLdsMax / node_bytes(lm_width(2)));
  *lds = lm == 3 ? flat : lm == 1 ? full : lm == 2 ? (size_t)kp.S.ntop * node_bytes(lm_width(2)) : 0;
  return lm;
}

template <int LM>
int launch_features(Ctx* c, const FeatKParams& kp, size_t lds) {
  int per_cu = 0;
  HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_features<LM>, kBlock, lds));
  if (per_cu <= 0) { g_err = "k_features cannot be resident (LDS/VGPR budget)"; return BDPT_E_DEVICE; }
  long long grid = std::min<long long>((long long)per_cu * c->ncu, ((long long)kp.nblocks + kWavesPerBlock - 1) / kWavesPerBlock);
  grid = std::max(1LL, grid);
  hipLaunchKernelGGL(k_features<LM>, dim3((unsigned)grid), dim3(kBlock), lds, c->stream, kp);
  HIPCHK(hipGetLastError());
  return BDPT_OK;
}

// ------------------------------------------------------------------------------------------------
// The filter. One launch per level; a wave owns an 8x8 pixel tile (lane = pixel), so its taps fall
// in few cache lines at every step; four tiles per 256-thread block. No LDS: from step 4 on
// neighbouring tiles share no taps, and the frames sit in L2 / the Infinity Cache.
constexpr int kAtrousBlock = 256;

__device__ __forceinline__ bool tile_pixel(int W, int H, int& x, int& y) {
  const int ntx = (W + 7) / 8;
  const long long tile = (long long)blockIdx.x * (kAtrousBlock / 64) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  x = (int)(tile % ntx) * 8 + (lane & 7);
  y = (int)(tile / ntx) * 8 + (lane >> 3);
  return x < W && y < H;
}

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
  const long long tiles = (long long)((W + 7) / 8) * ((H + 7) / 8);
  const dim3 grid((unsigned)((tiles + kAtrousBlock / 64 - 1) / (kAtrousBlock / 64))), block(kAtrousBlock);
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
  if (!c->d_features) {
    if (hipMalloc((void**)&c->d_features, c->npix * 8 * sizeof(float)) != hipSuccess) { g_err = "out of device memory"; return BDPT_E_NOMEM; }
    HIPCHK(hipMemsetAsync(c->d_features, 0, c->npix * 8 * sizeof(float), c->stream));
  }
  FeatKParams kp;
  kp.fp.W = W; kp.fp.H = H;
  kp.fp.nsamp = spp_count ? spp_count : c->prm.spp;
  kp.fp.seed = c->prm.seed;
  if (c->pt) {   // PtParams as bdpt_render fills them
    kp.fp.kind = FEAT_PT;
    kp.fp.lens_r = (float)c->prm.lens_radius;
    kp.fp.focal = (float)(c->prm.focal_distance > 0 ? c->prm.focal_distance : 4.7);
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
    for (int t = 0; t < ntiles; t++) {
      const int x0 = std::max(0, tiles[t].x0), y0 = std::max(0, tiles[t].y0);
      const int x1 = (int)std::min<int64_t>(W, (int64_t)tiles[t].x0 + tiles[t].w), y1 = (int)std::min<int64_t>(H, (int64_t)tiles[t].y0 + tiles[t].h);
      for (int by = y0; by < y1; by += 8)
        for (int bx = x0; bx < x1; bx += 8) blk.push_back(make_int4(bx, by, std::min(8, x1 - bx), std::min(8, y1 - by)));
    }
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
  size_t lds = 0;
  const int lm = feature_lds_mode(c, kp, &lds);
  // the ticket word of the render kernels: every use zeroes it first, in stream order
  kp.work = (unsigned*)(c->d_stats + 15);
  HIPCHK(hipMemsetAsync(kp.work, 0, sizeof(unsigned), c->stream));
  if (lm == 3) return launch_features<3>(c, kp, lds);
  if (lm == 1) return launch_features<1>(c, kp, lds);
  if (lm == 2) return launch_features<2>(c, kp, lds);
  return launch_features<0>(c, kp, lds);
}

int bdpt_read_features(void* ctx, float* out8) {
  Ctx* c = (Ctx*)ctx;
  if (!c || !out8) { g_err = "null argument"; return BDPT_E_INVALID; }
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  if (!c->d_features) { g_err = "no feature pass has run on this context (bdpt_render_features)"; return BDPT_E_INVALID; }
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(out8, c->d_features, c->npix * 8 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return BDPT_OK;
}

int bdpt_features_device_ptr(void* ctx, void** dptr) {
  Ctx* c = (Ctx*)ctx;
  if (!c || !dptr) { g_err = "null argument"; return BDPT_E_INVALID; }
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  if (!c->d_features) { g_err = "no feature pass has run on this context (bdpt_render_features)"; return BDPT_E_INVALID; }
  *dptr = c->d_features;
  return BDPT_OK;
}

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
  if (!c->d_denoised && hipMalloc((void**)&c->d_denoised, fb) != hipSuccess) { g_err = "out of device memory"; return BDPT_E_NOMEM; }
  if (!c->d_dn_scratch && hipMalloc((void**)&c->d_dn_scratch, 2 * fb) != hipSuccess) { g_err = "out of device memory"; return BDPT_E_NOMEM; }
  void* src = nullptr;
  if ((rc = bdpt_frame_device_ptr(ctx, which, &src))) return rc;
  rc = enqueue_filter(c->stream, (const float*)src, c->d_features, c->prm.width, c->prm.height, dp, c->d_denoised,
                      c->d_dn_scratch, c->d_dn_scratch + c->npix * 3);
  if (rc) return rc;
  c->denoised_valid = true;
  return BDPT_OK;
}

int bdpt_read_denoised(void* ctx, float* rgb) {
  Ctx* c = (Ctx*)ctx;
  if (!c || !rgb) { g_err = "null argument"; return BDPT_E_INVALID; }
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  if (!c->denoised_valid) { g_err = "no denoised frame on this context (bdpt_denoise)"; return BDPT_E_INVALID; }
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(rgb, c->d_denoised, c->npix * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return BDPT_OK;
}

int bdpt_denoised_device_ptr(void* ctx, void** dptr) {
  Ctx* c = (Ctx*)ctx;
  if (!c || !dptr) { g_err = "null argument"; return BDPT_E_INVALID; }
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  if (!c->denoised_valid) { g_err = "no denoised frame on this context (bdpt_denoise)"; return BDPT_E_INVALID; }
  *dptr = c->d_denoised;
  return BDPT_OK;
}

int bdpt_denoise_buffers(int32_t device, const float* d_color, const float* d_features, int32_t w, int32_t h,
                         const bdpt_denoise_params* p, float* d_out, void* stream) {
  if (!d_color || !d_features || !d_out) { g_err = "null argument"; return BDPT_E_INVALID; }
  if (w <= 0 || h <= 0) { g_err = "invalid frame size"; return BDPT_E_INVALID; }
  if (((uintptr_t)d_features & 15u) != 0) { g_err = "d_features must be 16-byte aligned"; return BDPT_E_INVALID; }
  bdpt_denoise_params dp;
  int rc = check_denoise_params(p, &dp);
  if (rc) return rc;
  if (device < 0) { g_err = "bad device ordinal"; return BDPT_E_INVALID; }
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
