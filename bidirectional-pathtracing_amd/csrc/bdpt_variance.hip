// bdpt_variance.hip — variance-guided denoise: the per-pixel batch moments of a frame
// rendered in equal sample batches (k_moments), the variance frame they estimate (k_variance) and
// the variance-guided a-trous filter (k_atrous_var), all bdpt_variance.h, with their C-ABI
// (bdpt_render_batches .. bdpt_denoise_variance_buffers). A translation unit of its own, like
// bdpt_denoise.hip: it adds kernels and leaves the other units' device code alone.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see __graft_entry__.build).

#include <hip/hip_runtime.h>

#include <mutex>
#include <string>

#include "bdpt/bdpt.h"
#include "bdpt_launch.h"   // bdpt_ctx.h
#include "bdpt_tile.h"
#include "bdpt_variance.h"

using namespace bdpt;

namespace {

// One lane per pixel, linear over the frame: the record is one 16-byte load and one 16-byte store.
// b == nullptr: the cumulative colour is a alone; else a + b, added as k_combine adds them.
__global__ __launch_bounds__(kLinBlock) void k_moments(const float* a, const float* b, float4* rec, long long npix) {
  const long long i = (long long)blockIdx.x * kLinBlock + threadIdx.x;
  if (i >= npix) return;
  f3 f = mk3(a[3 * i], a[3 * i + 1], a[3 * i + 2]);
  if (b) f = add(f, mk3(b[3 * i], b[3 * i + 1], b[3 * i + 2]));
  rec[i] = moments_add(rec[i], f);
}

__global__ __launch_bounds__(kLinBlock) void k_variance(const float4* rec, float* var, long long npix, VarK kf) {
  const long long i = (long long)blockIdx.x * kLinBlock + threadIdx.x;
  if (i >= npix) return;
  var[i] = variance_of(rec[i], kf);
}

// The filter. k_atrous's shape (bdpt_denoise.hip): one launch per level over the wave tiles of
// bdpt_tile.h, no LDS: the 9 prefilter taps lie in the tile and its rim, which the level's own 25
// variance taps at step 1 read anyway, and from step 4 on neighbouring tiles share no taps; the
// frames sit in L2 / the Infinity Cache.
__global__ __launch_bounds__(kAtrousBlock) void k_atrous_var(const float* c_in, const float* v_in, const float* F,
                                                             float* c_out, float* v_out, AtrousLevel L) {
  int x, y;
  if (!tile_pixel(L.W, L.H, x, y)) return;
  const ColVar r = atrous_var_pixel(c_in, v_in, F, L, x, y);
  const size_t p = (size_t)x + (size_t)y * L.W;
  c_out[3 * p] = r.c.x;
  c_out[3 * p + 1] = r.c.y;
  c_out[3 * p + 2] = r.c.z;
  v_out[p] = r.v;
}

// The last pass: scratch -> out. v_out may be null (the caller does not want the filtered variance).
__global__ __launch_bounds__(kAtrousBlock) void k_copy_var(const float* c_in, const float* v_in, float* c_out, float* v_out,
                                                           int W, int H) {
  int x, y;
  if (!tile_pixel(W, H, x, y)) return;
  const size_t p = (size_t)x + (size_t)y * W;
  c_out[3 * p] = c_in[3 * p];
  c_out[3 * p + 1] = c_in[3 * p + 1];
  c_out[3 * p + 2] = c_in[3 * p + 2];
  if (v_out) v_out[p] = v_in[p];
}

int check_params(const bdpt_denoise_variance_params* p, bdpt_denoise_variance_params* out) {
  bdpt_denoise_variance_params d;
  d.levels = kDenoiseVarLevels;
  d.sigma_variance = kDenoiseVarSigmaVariance;
  d.sigma_normal = kDenoiseVarSigmaNormal;
  d.sigma_depth = kDenoiseVarSigmaDepth;
  d.reserved[0] = d.reserved[1] = d.reserved[2] = d.reserved[3] = 0;
  if (p) d = *p;
  if (d.levels < 0 || d.levels > kDenoiseMaxLevels) { g_err = "denoise levels must be 0..8"; return BDPT_E_INVALID; }
  if (!(d.sigma_variance > 0) || !(d.sigma_normal > 0) || !(d.sigma_depth > 0)) { g_err = "denoise sigmas must be > 0"; return BDPT_E_INVALID; }
  if (d.reserved[0] || d.reserved[1] || d.reserved[2] || d.reserved[3]) { g_err = "bdpt_denoise_variance_params.reserved must be 0"; return BDPT_E_INVALID; }
  *out = d;
  return BDPT_OK;
}

// Enqueues the filter: (color, var) -> (out, var_out or nowhere) through two scratch pairs (sc[k]
// W*H*3, sv[k] W*H). Level i reads the current pair and writes pair i & 1; the last pass copies to
// out, so out may be color (and var_out var). levels == 0 is that copy alone.
int enqueue_filter(hipStream_t st, const float* color, const float* var, const float* F, int W, int H,
                   const bdpt_denoise_variance_params& p, float* out, float* var_out, float* sc0, float* sc1, float* sv0,
                   float* sv1) {
  const dim3 grid = tile_grid(W, H), block(kAtrousBlock);
  float* sc[2] = {sc0, sc1};
  float* sv[2] = {sv0, sv1};
  const float* cur = color;
  const float* curv = var;
  for (int i = 0; i < p.levels; i++) {
    const AtrousLevel L = atrous_var_level(W, H, i, p.sigma_variance, p.sigma_normal, p.sigma_depth);
    hipLaunchKernelGGL(k_atrous_var, grid, block, 0, st, cur, curv, F, sc[i & 1], sv[i & 1], L);
    cur = sc[i & 1];
    curv = sv[i & 1];
  }
  float* vo = var_out == curv ? nullptr : var_out;
  if (cur != out || vo) hipLaunchKernelGGL(k_copy_var, grid, block, 0, st, cur, curv, out, vo, W, H);
  HIPCHK(hipGetLastError());
  return BDPT_OK;
}

// restores Ctx::in_batches on every return path of bdpt_render_batches
struct BatchScope {
  Ctx* c;
  explicit BatchScope(Ctx* c_) : c(c_) { c->in_batches = true; }
  ~BatchScope() { c->in_batches = false; }
};

}  // namespace

extern "C" {

int bdpt_denoise_variance_default_params(bdpt_denoise_variance_params* p) {
  if (!p) { g_err = "null argument"; return BDPT_E_INVALID; }
  return check_params(nullptr, p);
}

int bdpt_render_batches(void* ctx, int32_t spp_begin, int32_t spp_count, int32_t batches) {
  Ctx* c = (Ctx*)ctx;
  if (!c) { g_err = "null ctx"; return BDPT_E_INVALID; }
  if (c->pt) {
    g_err = "bdpt_render_batches: the PathTracer renders whole pixels and keeps its moments inside its kernel; batches need the BDPT integrator";
    return BDPT_E_UNSUPPORTED;
  }
  if (spp_begin < 0 || spp_count <= 0) { g_err = "bdpt_render_batches: spp_begin must be >= 0 and spp_count > 0"; return BDPT_E_INVALID; }
  if (batches < 2) { g_err = "bdpt_render_batches needs at least 2 batches"; return BDPT_E_INVALID; }
  if (spp_count % batches != 0) {
    g_err = "bdpt_render_batches: spp_count " + std::to_string(spp_count) + " is no multiple of " + std::to_string(batches) + " batches";
    return BDPT_E_INVALID;
  }
  const int per = spp_count / batches;
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  if (c->var_batches > 0 && c->var_batch_spp != per) {
    g_err = "bdpt_render_batches: the frame holds batches of " + std::to_string(c->var_batch_spp) + " samples; this call asks for " +
            std::to_string(per) + " (bdpt_clear starts over)";
    return BDPT_E_INVALID;
  }
  HIPCHK(hipSetDevice(c->device));
  int rc = ensure_alloc(&c->d_moments, c->npix * sizeof(float4), &c->stream);
  if (rc) return rc;
  BatchScope scope(c);
  for (int k = 0; k < batches; k++) {
    if ((rc = bdpt_render(ctx, nullptr, 0, spp_begin + k * per, per))) return rc;
    hipLaunchKernelGGL(k_moments, dim3(lin_grid(c->npix)), dim3(kLinBlock), 0, c->stream, c->d_eye, c->d_light,
                       (float4*)c->d_moments, (long long)c->npix);
    HIPCHK(hipGetLastError());
    c->var_batches++;
    c->var_batch_spp = per;
    c->variance_valid = false;
  }
  return BDPT_OK;
}

int bdpt_variance(void* ctx) {
  Ctx* c = (Ctx*)ctx;
  if (!c) { g_err = "null ctx"; return BDPT_E_INVALID; }
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  if (c->var_unbatched) { g_err = "bdpt_variance: the frame holds samples that were not rendered in batches"; return BDPT_E_INVALID; }
  if (c->var_batches < 2) { g_err = "bdpt_variance needs at least 2 batches (bdpt_render_batches)"; return BDPT_E_INVALID; }
  HIPCHK(hipSetDevice(c->device));
  const int rc = ensure_alloc(&c->d_variance, c->npix * sizeof(float));
  if (rc) return rc;
  hipLaunchKernelGGL(k_variance, dim3(lin_grid(c->npix)), dim3(kLinBlock), 0, c->stream, (const float4*)c->d_moments,
                     c->d_variance, (long long)c->npix, var_k(c->var_batches));
  HIPCHK(hipGetLastError());
  c->variance_valid = true;
  return BDPT_OK;
}

static float* variance_of(Ctx* c) { return c->variance_valid ? c->d_variance : nullptr; }
static float* moments_of(Ctx* c) { return c->d_moments; }
static const char* const kNoVariance = "no variance frame on this context (bdpt_variance)";

int bdpt_read_variance(void* ctx, float* var) { return frame_out(ctx, variance_of, kNoVariance, sizeof(float), var, nullptr); }
int bdpt_variance_device_ptr(void* ctx, void** dptr) { return frame_out(ctx, variance_of, kNoVariance, 0, nullptr, dptr); }
int bdpt_read_moments(void* ctx, float* rec4) {
  return frame_out(ctx, moments_of, "no moments record on this context (bdpt_render_batches)", sizeof(float4), rec4, nullptr);
}

int bdpt_denoise_variance(void* ctx, const bdpt_denoise_variance_params* p) {
  bdpt_denoise_variance_params dp;
  int rc = check_params(p, &dp);
  if (rc) return rc;
  Ctx* c = (Ctx*)ctx;
  if (!c) { g_err = "null ctx"; return BDPT_E_INVALID; }
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  if (!c->d_features) { g_err = "bdpt_denoise_variance needs a feature pass first (bdpt_render_features)"; return BDPT_E_INVALID; }
  if (!c->variance_valid) { g_err = "bdpt_denoise_variance needs a variance frame first (bdpt_variance)"; return BDPT_E_INVALID; }
  HIPCHK(hipSetDevice(c->device));
  const size_t fb = c->npix * 3 * sizeof(float);
  if ((rc = ensure_alloc(&c->d_denoised, fb)) || (rc = ensure_alloc(&c->d_dn_scratch, 2 * fb)) ||
      (rc = ensure_alloc(&c->d_var_scratch, 2 * c->npix * sizeof(float))))
    return rc;
  void* src = nullptr;
  if ((rc = bdpt_frame_device_ptr(ctx, BDPT_FRAME_SAMPLE, &src))) return rc;
  rc = enqueue_filter(c->stream, (const float*)src, c->d_variance, c->d_features, c->prm.width, c->prm.height, dp, c->d_denoised,
                      nullptr, c->d_dn_scratch, c->d_dn_scratch + c->npix * 3, c->d_var_scratch, c->d_var_scratch + c->npix);
  if (rc) return rc;
  c->denoised_valid = true;
  return BDPT_OK;
}

int bdpt_moments_buffers(int32_t device, const float* d_frame_a, const float* d_frame_b, float* d_record, int32_t w, int32_t h,
                         void* stream) {
  if (!d_frame_a || !d_record) { g_err = "null argument"; return BDPT_E_INVALID; }
  const int rc = check_frame(device, w, h);
  if (rc) return rc;
  if (!aligned16(d_record)) { g_err = "d_record must be 16-byte aligned"; return BDPT_E_INVALID; }
  HIPCHK(hipSetDevice(device));
  const size_t npix = (size_t)w * h;
  hipLaunchKernelGGL(k_moments, dim3(lin_grid(npix)), dim3(kLinBlock), 0, (hipStream_t)stream, d_frame_a, d_frame_b,
                     (float4*)d_record, (long long)npix);
  HIPCHK(hipGetLastError());
  return BDPT_OK;
}

int bdpt_variance_buffers(int32_t device, const float* d_record, int32_t batches, int32_t w, int32_t h, float* d_var,
                          void* stream) {
  if (!d_record || !d_var) { g_err = "null argument"; return BDPT_E_INVALID; }
  const int rc = check_frame(device, w, h);
  if (rc) return rc;
  if (batches < 2) { g_err = "a variance needs at least 2 batches"; return BDPT_E_INVALID; }
  if (!aligned16(d_record)) { g_err = "d_record must be 16-byte aligned"; return BDPT_E_INVALID; }
  HIPCHK(hipSetDevice(device));
  const size_t npix = (size_t)w * h;
  hipLaunchKernelGGL(k_variance, dim3(lin_grid(npix)), dim3(kLinBlock), 0, (hipStream_t)stream, (const float4*)d_record, d_var,
                     (long long)npix, var_k(batches));
  HIPCHK(hipGetLastError());
  return BDPT_OK;
}

int bdpt_denoise_variance_buffers(int32_t device, const float* d_color, const float* d_var, const float* d_features, int32_t w,
                                  int32_t h, const bdpt_denoise_variance_params* p, float* d_out, float* d_var_out,
                                  void* stream) {
  if (!d_color || !d_var || !d_features || !d_out) { g_err = "null argument"; return BDPT_E_INVALID; }
  int rc = check_frame(device, w, h);
  if (rc) return rc;
  if (!aligned16(d_features)) { g_err = "d_features must be 16-byte aligned"; return BDPT_E_INVALID; }
  bdpt_denoise_variance_params dp;
  if ((rc = check_params(p, &dp))) return rc;
  HIPCHK(hipSetDevice(device));
  const size_t n = (size_t)w * h;
  float* scratch = nullptr;
  HIPCHK(hipMalloc((void**)&scratch, 8 * n * sizeof(float)));
  rc = enqueue_filter((hipStream_t)stream, d_color, d_var, d_features, w, h, dp, d_out, d_var_out, scratch, scratch + 3 * n,
                      scratch + 6 * n, scratch + 7 * n);
  const hipError_t e = hipStreamSynchronize((hipStream_t)stream);
  (void)hipFree(scratch);
  if (rc) return rc;
  HIPCHK(e);
  return BDPT_OK;
}

}  // extern "C"
