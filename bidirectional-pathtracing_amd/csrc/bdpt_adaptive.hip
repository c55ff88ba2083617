// bdpt_adaptive.hip — adaptive sampling under BDPT: the frame is rendered in rounds over
// a shrinking list of 8x8 pixel blocks. After each round k_adapt_moments updates the per-pixel eye and
// light records, k_adapt_decide tests every active block's variance against its mean, and
// k_adapt_compact rebuilds the block list the megakernel reads; k_adapt_resolve turns the records into
// the colour, variance and sample-count frames. All four are bdpt_adaptive.h, with their C-ABI
// (bdpt_render_adaptive .. bdpt_adaptive_resolve_buffers). A translation unit of its own, like
// bdpt_variance.hip: it adds kernels and leaves the other units' device code alone.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see __graft_entry__.build).

#include <hip/hip_runtime.h>

#include <cmath>
#include <mutex>
#include <string>

#include "bdpt/bdpt.h"
#include "bdpt_adaptive.h"
#include "bdpt_launch.h"   // bdpt_ctx.h
#include "bdpt_tile.h"

using namespace bdpt;

namespace {

constexpr int kWaveBlock = 256;      // k_adapt_decide: four waves = four pixel blocks
constexpr int kCompactBlock = 1024;  // k_adapt_compact: one workgroup of 16 waves

// One lane per pixel, linear over the frame: two 16-byte loads and two 16-byte stores. An inactive
// block's pixel has a zero increment, so the update is unconditional.
__global__ __launch_bounds__(kLinBlock) void k_adapt_moments(const float* eye, const float* light, float4* rec_e, float4* rec_l,
                                                             long long npix, float inv_m) {
  const long long i = (long long)blockIdx.x * kLinBlock + threadIdx.x;
  if (i >= npix) return;
  rec_e[i] = moments_add(rec_e[i], mk3(eye[3 * i], eye[3 * i + 1], eye[3 * i + 2]));
  rec_l[i] = moments_add_weighted(rec_l[i], mk3(light[3 * i], light[3 * i + 1], light[3 * i + 2]), inv_m);
}

// One wave per pixel block (lane = x + 8 y inside it), four blocks per workgroup. The wave owns the
// block's round count and flag: no atomics. decide == 0: the round is counted and nothing else.
__global__ __launch_bounds__(kWaveBlock) void k_adapt_decide(const float4* rec_e, const float4* rec_l, int* rounds, int* active, int W,
                                                             int H, int S, int m, AdaptScal sc, float tol, int decide) {
  const int nbx = (W + kAdaptBlock - 1) / kAdaptBlock, nby = (H + kAdaptBlock - 1) / kAdaptBlock;
  const int b = (int)blockIdx.x * (kWaveBlock / 64) + (int)(threadIdx.x >> 6);
  if (b >= nbx * nby) return;   // the whole wave
  if (active[b] == 0) return;   // the whole wave: a stopped block never restarts
  const int lane = threadIdx.x & 63;
  const int K = rounds[b] + 1;
  const int x0 = (b % nbx) * kAdaptBlock, y0 = (b / nbx) * kAdaptBlock;
  const int x = x0 + (lane & 7), y = y0 + (lane >> 3);
  float sv = 0.0f, scol = 0.0f;
  if (decide && x < W && y < H) {
    const size_t p = (size_t)x + (size_t)y * W;
    const AdaptPix px = adapt_pixel(rec_e[p], rec_l[p], adapt_block(K, S, m), sc);
    sv = px.v;
    scol = adapt_csum(px.c);
  }
  for (int o = 32; o > 0; o >>= 1) {
    sv = sv + __shfl_xor(sv, o, 64);
    scol = scol + __shfl_xor(scol, o, 64);
  }
  if (lane == 0) {
    rounds[b] = K;
    const int n = min(kAdaptBlock, W - x0) * min(kAdaptBlock, H - y0);
    if (decide && adapt_stop(sv, scol, n, tol)) active[b] = 0;
  }
}

// The ordered compaction of the flags into the megakernel's block list {x, y, w, h}, in block-index
// order, by one workgroup that strides over the flags: a wave's ballot and popcount give the lane's
// place in its wave, the 16 wave totals go through LDS. counts = {active blocks, their in-frame
// pixels}.
__global__ __launch_bounds__(kCompactBlock) void k_adapt_compact(const int* active, int W, int H, int4* list, int* counts) {
  __shared__ int wtot[kCompactBlock / 64];
  __shared__ int wpix[kCompactBlock / 64];
  const int nbx = (W + kAdaptBlock - 1) / kAdaptBlock, nby = (H + kAdaptBlock - 1) / kAdaptBlock;
  const int nblocks = nbx * nby;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int base_out = 0, pix = 0;
  for (int base = 0; base < nblocks; base += kCompactBlock) {
    const int b = base + tid;
    const bool on = b < nblocks && active[b] != 0;
    const unsigned long long m = __ballot(on);
    if (lane == 0) wtot[wave] = (int)__popcll(m);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < kCompactBlock / 64; w++) {
      const int t = wtot[w];
      before += w < wave ? t : 0;
      total += t;
    }
    if (on) {
      const int x0 = (b % nbx) * kAdaptBlock, y0 = (b / nbx) * kAdaptBlock;
      const int bw = min(kAdaptBlock, W - x0), bh = min(kAdaptBlock, H - y0);
      const int at = base_out + before + (int)__popcll(m & ((1ull << lane) - 1ull));   // < nblocks: one slot per flag
      list[at] = make_int4(x0, y0, bw, bh);
      pix += bw * bh;
    }
    base_out += total;
    __syncthreads();   // wtot is rewritten by the next stride
  }
  for (int o = 32; o > 0; o >>= 1) pix += __shfl_xor(pix, o, 64);
  if (lane == 0) wpix[wave] = pix;
  __syncthreads();
  if (tid == 0) {
    int p = 0;
    for (int w = 0; w < kCompactBlock / 64; w++) p += wpix[w];
    counts[0] = base_out;
    counts[1] = p;
  }
}

// One lane per pixel: colour (W*H*3), variance (W*H) and the sample count K_b m (W*H int32).
__global__ __launch_bounds__(kLinBlock) void k_adapt_resolve(const float4* rec_e, const float4* rec_l, const int* rounds, int W, int H,
                                                             int S, int m, AdaptScal sc, float* color, float* var, int* count) {
  const long long i = (long long)blockIdx.x * kLinBlock + threadIdx.x;
  if (i >= (long long)W * H) return;
  const int x = (int)(i % W), y = (int)(i / W);
  const int K = rounds[(y / kAdaptBlock) * ((W + kAdaptBlock - 1) / kAdaptBlock) + x / kAdaptBlock];
  const AdaptPix px = adapt_pixel(rec_e[i], rec_l[i], adapt_block(K, S, m), sc);
  color[3 * i] = px.c.x;
  color[3 * i + 1] = px.c.y;
  color[3 * i + 2] = px.c.z;
  var[i] = px.v;
  count[i] = K * m;
}

int nblocks_of(int W, int H) { return ((W + kAdaptBlock - 1) / kAdaptBlock) * ((H + kAdaptBlock - 1) / kAdaptBlock); }
unsigned wave_grid(int nblocks) { return (unsigned)((nblocks + kWaveBlock / 64 - 1) / (kWaveBlock / 64)); }

void defaults(bdpt_adaptive_params* d, int spp) {
  d->samples_per_round = kAdaptSamplesPerRound;
  d->min_rounds = kAdaptMinRounds;
  d->max_rounds = spp > 0 ? spp / kAdaptSamplesPerRound : 0;
  d->tolerance = kAdaptTolerance;
  d->reserved[0] = d->reserved[1] = d->reserved[2] = d->reserved[3] = 0;
}

// max_rounds == 0 in a caller's struct: spp / samples_per_round.
int check_params(const bdpt_adaptive_params* p, int spp, bdpt_adaptive_params* out) {
  bdpt_adaptive_params d;
  defaults(&d, spp);
  if (p) {
    d = *p;
    if (d.samples_per_round >= 1 && d.max_rounds == 0) d.max_rounds = spp / d.samples_per_round;
  }
  if (d.samples_per_round < 1) { g_err = "bdpt_adaptive_params.samples_per_round must be >= 1"; return BDPT_E_INVALID; }
  if (d.min_rounds < 2) { g_err = "bdpt_adaptive_params.min_rounds must be >= 2 (a variance needs two rounds)"; return BDPT_E_INVALID; }
  if (d.max_rounds < d.min_rounds) {
    g_err = "bdpt_adaptive_params: max_rounds " + std::to_string(d.max_rounds) + " < min_rounds " + std::to_string(d.min_rounds);
    return BDPT_E_INVALID;
  }
  if ((int64_t)d.max_rounds * d.samples_per_round > spp) {
    g_err = "bdpt_adaptive_params: max_rounds x samples_per_round = " + std::to_string((int64_t)d.max_rounds * d.samples_per_round) +
            " exceeds the context's spp " + std::to_string(spp);
    return BDPT_E_INVALID;
  }
  if (!std::isfinite(d.tolerance) || d.tolerance < 0) { g_err = "bdpt_adaptive_params.tolerance must be finite and >= 0"; return BDPT_E_INVALID; }
  if (d.reserved[0] || d.reserved[1] || d.reserved[2] || d.reserved[3]) { g_err = "bdpt_adaptive_params.reserved must be 0"; return BDPT_E_INVALID; }
  *out = d;
  return BDPT_OK;
}

// The scalars of a decision or a resolve: what the callers of adapt_scal must hold.
int check_totals(int32_t spp, int32_t m, int32_t rounds, int64_t samples) {
  if (spp < 1 || m < 1) { g_err = "spp and samples_per_round must be >= 1"; return BDPT_E_INVALID; }
  if (rounds < 2) { g_err = "a variance needs at least 2 rounds"; return BDPT_E_INVALID; }
  if (samples < 1) { g_err = "the number of pixel-samples must be >= 1"; return BDPT_E_INVALID; }
  return BDPT_OK;
}

// The adaptive buffers of a context, allocated on the first adaptive render.
int alloc_state(Ctx* c) {
  const int nb = nblocks_of(c->prm.width, c->prm.height);
  int rc;
  if ((rc = ensure_alloc(&c->d_adapt_rec, 2 * c->npix * sizeof(float4), &c->stream)) ||
      (rc = ensure_alloc(&c->d_adapt_rounds, 2 * (size_t)nb * sizeof(int))) ||
      (rc = ensure_alloc(&c->d_adapt_list, (size_t)nb * sizeof(int4))) || (rc = ensure_alloc(&c->d_adapt_counts, 2 * sizeof(int))))
    return rc;
  if (!c->h_adapt_counts) HIPCHK(hipHostMalloc((void**)&c->h_adapt_counts, 2 * sizeof(int)));
  if (!c->adapt_ev) HIPCHK(hipEventCreateWithFlags(&c->adapt_ev, hipEventDisableTiming));
  return BDPT_OK;
}

}  // namespace

extern "C" {

int bdpt_adaptive_default_params(void* ctx, bdpt_adaptive_params* p) {
  if (!p) { g_err = "null argument"; return BDPT_E_INVALID; }
  const Ctx* c = (const Ctx*)ctx;
  defaults(p, c ? c->prm.spp : 0);
  return BDPT_OK;
}

int bdpt_render_adaptive(void* ctx, const bdpt_adaptive_params* params, bdpt_adaptive_info* out) {
  Ctx* c = (Ctx*)ctx;
  if (!c) { g_err = "null ctx"; return BDPT_E_INVALID; }
  if (c->pt) {
    g_err = "bdpt_render_adaptive: the PathTracer stops single pixels inside its own kernel (max_tolerance); "
            "block-adaptive rounds need the BDPT integrator";
    return BDPT_E_UNSUPPORTED;
  }
  bdpt_adaptive_params p;
  int rc = check_params(params, c->prm.spp, &p);
  if (rc) return rc;
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  if (c->frame_dirty) {
    g_err = "bdpt_render_adaptive: the frame already holds samples (bdpt_clear starts over)";
    return BDPT_E_INVALID;
  }
  HIPCHK(hipSetDevice(c->device));
  if ((rc = alloc_state(c))) return rc;
  const int W = c->prm.width, H = c->prm.height, S = c->prm.spp, m = p.samples_per_round;
  const int nb = nblocks_of(W, H);
  float4* rec_e = (float4*)c->d_adapt_rec;
  float4* rec_l = rec_e + c->npix;
  int* rounds = c->d_adapt_rounds;
  int* active = rounds + nb;
  HIPCHK(hipMemsetAsync(rounds, 0, (size_t)nb * sizeof(int), c->stream));
  HIPCHK(hipMemsetD32Async((hipDeviceptr_t)active, 1, (size_t)nb, c->stream));
  c->frame_dirty = true;
  c->var_unbatched = true;   // unequal sample counts: bdpt_variance's uniform batches do not describe this frame
  c->adapt_valid = c->adapt_resolved = false;
  long long N = 0, npix_active = (long long)c->npix;
  int nact = nb, R = 0;
  while (true) {
    // round R renders samples [R m, (R + 1) m) of the active blocks; round 0 is the whole frame
    rc = render_blocks(c, R == 0 ? nullptr : c->d_adapt_list, nact, R * m, m);
    if (rc) return rc;
    const long long M = npix_active * m;
    N += M;
    R++;
    hipLaunchKernelGGL(k_adapt_moments, dim3(lin_grid(c->npix)), dim3(kLinBlock), 0, c->stream, c->d_eye, c->d_light, rec_e, rec_l,
                       (long long)c->npix, (float)(1.0 / (double)M));
    const int decide = R >= p.min_rounds ? 1 : 0;
    AdaptScal sc = {0.0f, 0.0f, 0.0f};
    if (decide) sc = adapt_scal(W, H, S, R, N);
    hipLaunchKernelGGL(k_adapt_decide, dim3(wave_grid(nb)), dim3(kWaveBlock), 0, c->stream, rec_e, rec_l, rounds, active, W, H, S, m, sc,
                       p.tolerance, decide);
    hipLaunchKernelGGL(k_adapt_compact, dim3(1), dim3(kCompactBlock), 0, c->stream, active, W, H, c->d_adapt_list, c->d_adapt_counts);
    HIPCHK(hipGetLastError());
    // the one host wait of the round: the two counts
    HIPCHK(hipMemcpyAsync(c->h_adapt_counts, c->d_adapt_counts, 2 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipEventRecord(c->adapt_ev, c->stream));
    HIPCHK(hipEventSynchronize(c->adapt_ev));
    nact = c->h_adapt_counts[0];
    npix_active = c->h_adapt_counts[1];
    if (nact < 0 || nact > nb || npix_active < 0 || npix_active > (long long)c->npix) {
      g_err = "bdpt_render_adaptive: the compaction returned counts outside the frame";
      return BDPT_E_DEVICE;
    }
    if (nact == 0 || R == p.max_rounds) break;
  }
  c->adapt_rounds = R;
  c->adapt_m = m;
  c->adapt_n = N;
  c->adapt_active = nact;
  c->adapt_valid = true;
  if (out) {
    out->rounds = R;
    out->active_blocks = nact;
    out->samples = N;
    out->reserved[0] = out->reserved[1] = out->reserved[2] = out->reserved[3] = 0;
  }
  return BDPT_OK;
}

int bdpt_adaptive_resolve(void* ctx) {
  Ctx* c = (Ctx*)ctx;
  if (!c) { g_err = "null ctx"; return BDPT_E_INVALID; }
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  if (!c->adapt_valid) { g_err = "bdpt_adaptive_resolve needs an adaptive render of this frame first (bdpt_render_adaptive)"; return BDPT_E_INVALID; }
  HIPCHK(hipSetDevice(c->device));
  const int rc = ensure_alloc(&c->d_adapt_out, c->npix * 5 * sizeof(float));
  if (rc) return rc;
  const int W = c->prm.width, H = c->prm.height;
  const float4* rec_e = (const float4*)c->d_adapt_rec;
  hipLaunchKernelGGL(k_adapt_resolve, dim3(lin_grid(c->npix)), dim3(kLinBlock), 0, c->stream, rec_e, rec_e + c->npix,
                     (const int*)c->d_adapt_rounds, W, H, c->prm.spp, c->adapt_m, adapt_scal(W, H, c->prm.spp, c->adapt_rounds, c->adapt_n),
                     c->d_adapt_out, c->d_adapt_out + 3 * c->npix, (int*)(c->d_adapt_out + 4 * c->npix));
  HIPCHK(hipGetLastError());
  c->adapt_resolved = true;
  return BDPT_OK;
}

int bdpt_read_adaptive(void* ctx, float* rgb, float* var, int32_t* counts) {
  Ctx* c = (Ctx*)ctx;
  if (!c) { g_err = "null ctx"; return BDPT_E_INVALID; }
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  if (!c->adapt_valid || !c->adapt_resolved) { g_err = "no resolved adaptive frame on this context (bdpt_adaptive_resolve)"; return BDPT_E_INVALID; }
  HIPCHK(hipSetDevice(c->device));
  const float* o = c->d_adapt_out;
  if (rgb) HIPCHK(hipMemcpyAsync(rgb, o, c->npix * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (var) HIPCHK(hipMemcpyAsync(var, o + 3 * c->npix, c->npix * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (counts) HIPCHK(hipMemcpyAsync(counts, o + 4 * c->npix, c->npix * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return BDPT_OK;
}

int bdpt_adaptive_device_ptrs(void* ctx, void** d_color, void** d_var, void** d_counts) {
  Ctx* c = (Ctx*)ctx;
  if (!c) { g_err = "null ctx"; return BDPT_E_INVALID; }
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  if (!c->adapt_valid || !c->adapt_resolved) { g_err = "no resolved adaptive frame on this context (bdpt_adaptive_resolve)"; return BDPT_E_INVALID; }
  if (d_color) *d_color = c->d_adapt_out;
  if (d_var) *d_var = c->d_adapt_out + 3 * c->npix;
  if (d_counts) *d_counts = c->d_adapt_out + 4 * c->npix;
  return BDPT_OK;
}

// One half of Ctx::d_adapt_rounds: the blocks' round counts (half 0) or their active flags (half 1).
static int read_per_block(void* ctx, int half, int32_t* per_block) {
  Ctx* c = (Ctx*)ctx;
  if (!c || !per_block) { g_err = "null argument"; return BDPT_E_INVALID; }
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  if (!c->adapt_valid) { g_err = "no adaptive render on this context (bdpt_render_adaptive)"; return BDPT_E_INVALID; }
  const size_t nb = (size_t)nblocks_of(c->prm.width, c->prm.height);
  return read_back(c, per_block, c->d_adapt_rounds + half * nb, nb * sizeof(int32_t));
}

int bdpt_read_adaptive_rounds(void* ctx, int32_t* per_block) { return read_per_block(ctx, 0, per_block); }
int bdpt_read_adaptive_active(void* ctx, int32_t* per_block) { return read_per_block(ctx, 1, per_block); }

int bdpt_read_adaptive_records(void* ctx, float* eye_rec4, float* light_rec4) {
  Ctx* c = (Ctx*)ctx;
  if (!c) { g_err = "null ctx"; return BDPT_E_INVALID; }
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  if (!c->adapt_valid) { g_err = "no adaptive render on this context (bdpt_render_adaptive)"; return BDPT_E_INVALID; }
  HIPCHK(hipSetDevice(c->device));
  const size_t bytes = c->npix * sizeof(float4);
  if (eye_rec4) HIPCHK(hipMemcpyAsync(eye_rec4, c->d_adapt_rec, bytes, hipMemcpyDeviceToHost, c->stream));
  if (light_rec4) HIPCHK(hipMemcpyAsync(light_rec4, c->d_adapt_rec + 4 * c->npix, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return BDPT_OK;
}

int bdpt_adaptive_moments_buffers(int32_t device, const float* d_eye, const float* d_light, float* d_eye_record, float* d_light_record,
                                  int32_t w, int32_t h, int64_t round_samples, void* stream) {
  if (!d_eye || !d_light || !d_eye_record || !d_light_record) { g_err = "null argument"; return BDPT_E_INVALID; }
  int rc = check_frame(device, w, h);
  if (rc) return rc;
  if (round_samples < 1) { g_err = "the round's pixel-samples must be >= 1"; return BDPT_E_INVALID; }
  if (!aligned16(d_eye_record) || !aligned16(d_light_record)) { g_err = "the records must be 16-byte aligned"; return BDPT_E_INVALID; }
  HIPCHK(hipSetDevice(device));
  const size_t npix = (size_t)w * h;
  hipLaunchKernelGGL(k_adapt_moments, dim3(lin_grid(npix)), dim3(kLinBlock), 0, (hipStream_t)stream, d_eye, d_light,
                     (float4*)d_eye_record, (float4*)d_light_record, (long long)npix, (float)(1.0 / (double)round_samples));
  HIPCHK(hipGetLastError());
  return BDPT_OK;
}

int bdpt_adaptive_decide_buffers(int32_t device, const float* d_eye_record, const float* d_light_record, int32_t* d_rounds,
                                 int32_t* d_active, int32_t w, int32_t h, int32_t spp, int32_t samples_per_round, int32_t rounds,
                                 int64_t samples, float tolerance, int32_t decide, void* stream) {
  if (!d_eye_record || !d_light_record || !d_rounds || !d_active) { g_err = "null argument"; return BDPT_E_INVALID; }
  int rc = check_frame(device, w, h);
  if (rc) return rc;
  if (decide && (rc = check_totals(spp, samples_per_round, rounds, samples))) return rc;
  if (!std::isfinite(tolerance) || tolerance < 0) { g_err = "tolerance must be finite and >= 0"; return BDPT_E_INVALID; }
  if (!aligned16(d_eye_record) || !aligned16(d_light_record)) { g_err = "the records must be 16-byte aligned"; return BDPT_E_INVALID; }
  HIPCHK(hipSetDevice(device));
  AdaptScal sc = {0.0f, 0.0f, 0.0f};
  if (decide) sc = adapt_scal(w, h, spp, rounds, samples);
  hipLaunchKernelGGL(k_adapt_decide, dim3(wave_grid(nblocks_of(w, h))), dim3(kWaveBlock), 0, (hipStream_t)stream,
                     (const float4*)d_eye_record, (const float4*)d_light_record, d_rounds, d_active, w, h, spp, samples_per_round, sc,
                     tolerance, decide ? 1 : 0);
  HIPCHK(hipGetLastError());
  return BDPT_OK;
}

int bdpt_adaptive_compact_buffers(int32_t device, const int32_t* d_active, int32_t w, int32_t h, int32_t* d_list4, int32_t* d_counts2,
                                  void* stream) {
  if (!d_active || !d_list4 || !d_counts2) { g_err = "null argument"; return BDPT_E_INVALID; }
  int rc = check_frame(device, w, h);
  if (rc) return rc;
  if (!aligned16(d_list4)) { g_err = "d_list4 must be 16-byte aligned"; return BDPT_E_INVALID; }
  HIPCHK(hipSetDevice(device));
  hipLaunchKernelGGL(k_adapt_compact, dim3(1), dim3(kCompactBlock), 0, (hipStream_t)stream, d_active, w, h, (int4*)d_list4, d_counts2);
  HIPCHK(hipGetLastError());
  return BDPT_OK;
}

int bdpt_adaptive_resolve_buffers(int32_t device, const float* d_eye_record, const float* d_light_record, const int32_t* d_rounds,
                                  int32_t w, int32_t h, int32_t spp, int32_t samples_per_round, int32_t rounds, int64_t samples,
                                  float* d_color, float* d_var, int32_t* d_counts, void* stream) {
  if (!d_eye_record || !d_light_record || !d_rounds || !d_color || !d_var || !d_counts) { g_err = "null argument"; return BDPT_E_INVALID; }
  int rc = check_frame(device, w, h);
  if (rc) return rc;
  if ((rc = check_totals(spp, samples_per_round, rounds, samples))) return rc;
  if (!aligned16(d_eye_record) || !aligned16(d_light_record)) { g_err = "the records must be 16-byte aligned"; return BDPT_E_INVALID; }
  HIPCHK(hipSetDevice(device));
  hipLaunchKernelGGL(k_adapt_resolve, dim3(lin_grid((size_t)w * h)), dim3(kLinBlock), 0, (hipStream_t)stream,
                     (const float4*)d_eye_record, (const float4*)d_light_record, d_rounds, w, h, spp, samples_per_round,
                     adapt_scal(w, h, spp, rounds, samples), d_color, d_var, d_counts);
  HIPCHK(hipGetLastError());
  return BDPT_OK;
}

}  // extern "C"
