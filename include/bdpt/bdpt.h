/* include/bdpt/bdpt.h — C-ABI of the MI355X-native BDPT hot path (libbdpt_amd.so).
 *
 * Drop-in boundary for the reference's per-pixel BDPT loop:
 *   reference interface                          replaced by
 *   PathTracer::set_frame_size   pathtracer.h:36  -> bdpt_create (frame size in bdpt_params)
 *   PathTracer::clear            pathtracer.h:43  -> bdpt_clear
 *   PathTracer::raytrace_pixel   pathtracer.h:69  -> bdpt_render over a 1x1 tile
 *     (BidirectionalPathTracer::raytrace_pixel, src/pathtracer/bidirection.cpp:503-542)
 *   RaytracedRenderer::raytrace_tile             -> bdpt_render over a list of tiles
 *     (src/pathtracer/raytraced_renderer.cpp:595-620)
 *   BidirectionalPathTracer::{sampleBuffer, eyeBuffer, lightBuffer}
 *     (bidirection.h:81, pathtracer.h:90)         -> bdpt_read_frame (BDPT_FRAME_*)
 *   RaytracedRenderer::set_scene / build_accel    -> bdpt_create (scene desc; the BVH is built
 *     (raytraced_renderer.cpp:105-127,350-374)       inside: the reference's midpoint-split tree,
 *                                                    bvh.cpp:51-129, for its DFS leaf order (the
 *                                                    equal-t tie key), and a binned-SAH device tree
 *                                                    over the same primitives)
 *
 * Threading: one ctx per GPU. Every entry point taking a ctx locks it, so the reference's model of
 * N worker threads calling raytrace_pixel / raytrace_tile on one PathTracer
 * (raytraced_renderer.cpp:325-327,610-615) is safe; the calls are serialised per ctx.
 *
 * Plain C types only: no torch, no HIP types in any signature (a stream is passed as void*).
 * Every call returns 0 (BDPT_OK) or a negative BDPT_E_* code; bdpt_last_error() gives the text.
 * No C++ exception crosses this boundary. Unsupported features that the reference can only
 * assert(0) on under BDPT (microfacet sample_pdf, advanced_bsdf.cpp:144-148; ambient / directional /
 * spot / sphere / mesh lights, light.cpp:25-51,72-98,168-194) are rejected at bdpt_create with
 * BDPT_E_UNSUPPORTED instead of aborting (ambient and directional lights: unless
 * bdpt_params.infinite_lights is set, below).
 *
 * Extensions beyond what the reference can run (semantics in DESIGN.md §9):
 *   - the environment light under BDPT (the reference's EnvironmentLight has sample_L / sample_dir
 *     but asserts in sample_Le / sample_Le_point / sample_pdf / contain_point,
 *     environment_light.cpp:182-208): bdpt_scene_desc.envmap, loaded by bdpt_exr_load (-e);
 *   - Russian roulette on both subpaths through PathVertex.q (bidirection.h:36, the rule commented
 *     out at bidirection.cpp:87-93): bdpt_params.russian_roulette;
 *   - ambient (InfiniteHemisphereLight) and directional lights under BDPT (the reference's BDPT
 *     light API prints "not ready" and asserts for them, light.cpp:25-51,72-98), with the
 *     environment light's machinery: bdpt_params.infinite_lights. At most
 *     one light that an escaped ray can reach — the environment map or one ambient light — per
 *     scene; any number of directional lights.
 * Denoised output (new symbols only, the ABI version is unchanged): per-pixel first-hit
 * feature buffers through the integrator's own primary rays (bdpt_render_features) and a
 * feature-guided edge-avoiding a-trous filter over a frame (bdpt_denoise, bdpt_denoise_buffers).
 * Variance-guided denoise (new symbols only as well): a frame rendered in equal sample
 * batches keeps per-pixel moments (bdpt_render_batches), which give its per-pixel variance
 * (bdpt_variance) and guide the filter's colour weight (bdpt_denoise_variance, *_buffers).
 * Adaptive sampling under BDPT (new symbols only as well): the frame is rendered in
 * rounds and every 8x8 pixel block stops once its variance is within a tolerance of its mean
 * (bdpt_render_adaptive, bdpt_adaptive_resolve, bdpt_read_adaptive, bdpt_adaptive_*_buffers).
 * And the reference's second integrator: the unidirectional PathTracer
 * (pathtracer.cpp:47-340 — NEE, adaptive sampling, thin lens, roulette at -m 0, the environment
 * light, MicrofacetBSDF), selected by bdpt_params.integrator = BDPT_INTEGRATOR_PT (ABI v3).
 */
#ifndef BDPT_AMD_BDPT_H
#define BDPT_AMD_BDPT_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BDPT_ABI_VERSION 10

enum bdpt_status {
  BDPT_OK = 0,
  BDPT_E_INVALID = -1,      /* bad argument / malformed scene */
  BDPT_E_UNSUPPORTED = -2,  /* feature the reference BDPT cannot run (see header comment) */
  BDPT_E_DEVICE = -3,       /* HIP runtime error (no device, launch failure, ...) */
  BDPT_E_NOMEM = -4
};

/* Primitive kinds (src/scene/triangle.h, src/scene/sphere.h). */
enum bdpt_prim_type { BDPT_PRIM_TRIANGLE = 0, BDPT_PRIM_SPHERE = 1 };

/* BSDF kinds (src/pathtracer/bsdf.h:117-306). */
enum bdpt_mat_type {
  BDPT_MAT_DIFFUSE = 0,     /* a = reflectance                                  bsdf.cpp:52-85   */
  BDPT_MAT_EMISSION = 1,    /* a = radiance                                     bsdf.cpp:99-118  */
  BDPT_MAT_MIRROR = 2,      /* a = reflectance                          advanced_bsdf.cpp:17-35   */
  BDPT_MAT_GLASS = 3,       /* a = reflectance, b = transmittance, ior  advanced_bsdf.cpp:198-259 */
  BDPT_MAT_REFRACTION = 4,  /* b = transmittance, ior                   advanced_bsdf.cpp:163-184 */
  BDPT_MAT_MICROFACET = 5   /* rejected: sample_pdf asserts under BDPT  advanced_bsdf.cpp:144-148 */
};

/* Light kinds (src/scene/light.h). Only area and point lights have BDPT methods in the reference;
 * ambient and directional lights render under BDPT with bdpt_params.infinite_lights; the
 * environment light comes in through bdpt_scene_desc.envmap, never through this list. */
enum bdpt_light_type {
  BDPT_LIGHT_AREA = 0, BDPT_LIGHT_POINT = 1,
  BDPT_LIGHT_OTHER = 2,       /* spot: rejected (SpotLight::sample_L leaves its outputs unset,
                                 light.cpp:163-166)                                            */
  BDPT_LIGHT_HEMISPHERE = 3,  /* an ambient light = InfiniteHemisphereLight (light.cpp:55-70):
                                 the PathTracer, and BDPT with bdpt_params.infinite_lights
                                 (the reference's BDPT: sample_Le asserts, :72-77)              */
  BDPT_LIGHT_DIRECTIONAL = 4  /* DirectionalLight (light.cpp:11-23): `direction` = dirToLight, the
                                 unit world direction towards the light; the PathTracer, and
                                 BDPT with bdpt_params.infinite_lights                          */
};

typedef struct bdpt_material {
  int32_t type;
  double a[3];
  double b[3];
  double ior;
  double roughness;
} bdpt_material;

typedef struct bdpt_light {
  int32_t type;
  double radiance[3];
  double position[3];
  double direction[3];  /* area: unit emitting normal                                */
  double dim_x[3];      /* area: rectangle edge vectors (light.cpp:199-203)          */
  double dim_y[3];
  double area;          /* |dim_x| * |dim_y|                                         */
} bdpt_light;

/* Pinhole camera state after Camera::configure/place/set_screen_size (camera.cpp:29-147). */
typedef struct bdpt_camera {
  double pos[3];
  double c2w[9];        /* column-major: c2w[3*col + row] (CGL Matrix3x3 columns)     */
  double w2c[9];        /* = c2w.inv() as the reference computes it                    */
  double hfov_deg;
  double vfov_deg;
  double nclip;
  double fclip;
} bdpt_camera;

/* The HDRImageBuffer of an environment map (main.cpp:40-77 load_exr; data[w*j + i], row j = 0 at
 * theta = 0, i.e. +y): EnvironmentLight(envMap) (environment_light.cpp:6-62). */
typedef struct bdpt_envmap {
  int32_t width, height;
  const float* rgb;           /* width*height*3                                          */
} bdpt_envmap;

/* Scene in the reference's primitive order (objects in scene order, faces in mesh order:
 * RaytracedRenderer::build_accel, raytraced_renderer.cpp:350-374). The BVH is built from it. */
typedef struct bdpt_scene_desc {
  int32_t nprim;
  const int32_t* prim_type;   /* nprim, bdpt_prim_type                                   */
  const double* prim_geom;    /* nprim*18: triangle p1,p2,p3,n1,n2,n3; sphere c[3],r,... */
  const int32_t* prim_mat;    /* nprim, index into mats                                  */
  int32_t nmat;
  const bdpt_material* mats;
  int32_t nlight;
  const bdpt_light* lights;
  bdpt_camera camera;
  /* NULL = none. Otherwise an EnvironmentLight appended after `lights` (the renderer pushes
   * pt->envLight onto scene->lights last, raytraced_renderer.cpp:117-119). ABI v2. */
  const bdpt_envmap* envmap;
} bdpt_scene_desc;

/* Random-number semantics of the device path: Philox4x32-10 keyed by seed, counter
 * (pixel = x + y*W, global sample index, block, 0xB1D1). See DESIGN.md §RNG. */
typedef struct bdpt_params {
  int32_t width;              /* frame size (PathTracer::set_frame_size)                 */
  int32_t height;
  int32_t spp;                /* ns_aa: the 1/ns_aa weight of every sample                */
  int32_t max_depth;          /* max_ray_depth (-m); BDPT: 0..62, PathTracer: 0..21      */
  uint64_t seed;
  int32_t samples_per_lane;   /* 0 = auto                                                 */
  int32_t device;             /* HIP device ordinal                                       */
  int32_t collect_stats;      /* 1 = kernel also counts node/prim tests (roofline bytes)  */
  int32_t pipeline;           /* 0 = auto = 1, the megakernel; 2 (the wavefront pipeline) was
                                 retired in round 5: BDPT_E_UNSUPPORTED                      */
  int32_t russian_roulette;   /* 1 = PathVertex.q roulette on both subpaths (ABI v2)       */
  /* ABI v3: the integrator and the PathTracer's settings (PathTracer fields, pathtracer.h:73-85;
   * CLI -l -a -H -b -d, main.cpp:107-141; AppConfig defaults application.h:45-65) */
  int32_t integrator;         /* BDPT_INTEGRATOR_BDPT (0, the reference's) / _PT (1)         */
  int32_t ns_area_light;      /* -l: samples per area light (0 = 1)                          */
  int32_t samples_per_batch;  /* -a batch: adaptive sampling batch (0 = 32)                  */
  float max_tolerance;        /* -a tol: stop when 1.96 sigma / sqrt(n) <= tol * mean        */
  int32_t direct_hemisphere_sample;  /* -H: hemisphere instead of light sampling            */
  /* The thin lens (Camera::generate_ray_for_thin_lens). The PathTracer always honoured the two; under
   * BDPT_INTEGRATOR_BDPT lens_radius > 0 now selects the thin-lens kernels (a lens
   * point per eye walk and a fresh one per camera connection) and lens_radius <= 0 is the pinhole,
   * which a caller that zeroes the struct gets as before. Same layout, same ABI version. */
  double lens_radius;         /* -b (0: pinhole)                                             */
  double focal_distance;      /* -d (0 = 4.7)                                                */
  /* Was reserved[0]: the layout is unchanged and a caller that zeroes the reserved words gets the
   * rejection it always got, so the ABI version stays 9. BDPT only; the PathTracer ignores it. */
  int32_t infinite_lights;    /* 0: BDPT rejects BDPT_LIGHT_HEMISPHERE / _DIRECTIONAL with
                                 BDPT_E_UNSUPPORTED; 1: it renders them         */
  int32_t reserved[3];
} bdpt_params;

enum bdpt_integrator { BDPT_INTEGRATOR_BDPT = 0, BDPT_INTEGRATOR_PT = 1 };

typedef struct bdpt_tile {
  int32_t x0, y0, w, h;       /* clipped to the frame like raytrace_tile does            */
} bdpt_tile;

enum bdpt_frame { BDPT_FRAME_SAMPLE = 0, BDPT_FRAME_EYE = 1, BDPT_FRAME_LIGHT = 2 };

typedef struct bdpt_stats {
  uint64_t samples;           /* pixel-samples rendered since the last clear            */
  uint64_t rays;              /* closest-hit + connection queries                        */
  uint64_t closest_rays;      /* walk rays (closest hit)                                 */
  uint64_t shadow_rays;       /* connection rays (any hit)                               */
  uint64_t node_visits;       /* AABBs fetched                                            */
  uint64_t tri_tests;
  uint64_t sph_tests;
  uint64_t hits;              /* closest-hit queries that hit (shading record fetched)   */
  double last_kernel_ms;      /* duration of the last bdpt_render's kernels (hipEvents)  */
  uint64_t bvh_nodes;
  uint64_t bvh_depth;
  /* ABI v4: where the scene reads of the last launches were served from */
  uint64_t lds_node_visits;   /* of node_visits: AABBs read from the CU's LDS copy          */
  int32_t lds_mode;           /* 0 scene in HBM, 1 whole scene in LDS, 2 BFS treelet in LDS +
                                 HBM below it, 3 flat primitive list in LDS; -1 none yet     */
  int32_t reserved0;
  /* ABI v6: environment-light table reads, counted like the scene reads above */
  uint64_t env_samples;       /* importance-sampled directions: 2 guide cells + 2 CDF entries per
                                 axis, the texel pdf, 4 texels (76 B)                          */
  uint64_t env_lookups;       /* radiance lookups along a direction: 4 texels (48 B)          */
  uint64_t env_pdf_lookups;   /* texel pdf lookups (4 B)                                      */
} bdpt_stats;

int bdpt_abi_version(void);
const char* bdpt_last_error(void);

/* Builds the BVH, flattens it, deep-copies the scene to HBM. The caller may free its arrays
 * after this returns. */
int bdpt_create(const bdpt_scene_desc* scene, const bdpt_params* params, void** ctx_out);
void bdpt_destroy(void* ctx);

/* All later work is enqueued on `stream` (a hipStream_t; NULL = the ctx's own stream). */
int bdpt_set_stream(void* ctx, void* stream);

/* Zeroes the frame buffers and counters (PathTracer::clear / set_frame_size). Async. */
int bdpt_clear(void* ctx);

/* Renders global sample indices [spp_begin, spp_begin+spp_count) of every pixel of the tiles.
 * Asynchronous on the ctx stream. ntiles == 0 or tiles == NULL means the whole frame. The
 * PathTracer renders whole pixels (its adaptive sampling decides per pixel): spp_begin must be 0
 * and spp_count the ctx's spp; shard its work across GPUs by tiles. */
int bdpt_render(void* ctx, const bdpt_tile* tiles, int32_t ntiles, int32_t spp_begin,
                int32_t spp_count);

int bdpt_sync(void* ctx);

/* Copies a W*H*3 float frame (row 0 = bottom, as HDRImageBuffer) to host memory (sync). Under
 * the PathTracer, BDPT_FRAME_SAMPLE is its sampleBuffer (per-pixel means, update_pixel). */
int bdpt_read_frame(void* ctx, int32_t which, float* rgb);

/* ABI v8: the pixels [x0, x0 + w) x [y0, y0 + h) of a frame as w*h*3 floats, row 0 = y0 (sync):
 * what a per-tile caller copies into sampleBuffer after raytrace_tile (the renderer reads the
 * whole sampleBuffer through the non-virtual write_to_framebuffer after every tile,
 * raytraced_renderer.cpp:619, pathtracer.cpp:42-45). The rectangle must lie inside the frame. */
int bdpt_read_frame_rect(void* ctx, int32_t which, int32_t x0, int32_t y0, int32_t w, int32_t h, float* rgb);

/* PathTracer::sampleCountBuffer (pathtracer.h:94): W*H samples per pixel, row 0 = bottom (sync).
 * Under BDPT every rendered pixel reports the samples rendered for it. */
int bdpt_read_sample_counts(void* ctx, int32_t* counts);

/* Device pointer of a frame (W*H*3 float) for in-HBM consumers (RCCL reduce). */
int bdpt_frame_device_ptr(void* ctx, int32_t which, void** dptr);

/* Enqueues a device-to-device copy of a frame into caller device memory (W*H*3 floats) on the
 * ctx stream — e.g. into a torch tensor that RCCL then reduces. Async. */
int bdpt_copy_frame(void* ctx, int32_t which, void* dst_device);

int bdpt_get_stats(void* ctx, bdpt_stats* out);

/* ABI v9: the multi-GPU frame reduce. The reference renders with N CPU threads
 * into one shared frame (raytraced_renderer.cpp:325-327); here N contexts — one per GPU, each
 * rendering its own sample range of every pixel — hold partial W*H*3 frames, and because the t = 1
 * light splats land on any pixel (bidirection.cpp:457-466) the image is their whole-frame sum.
 * bdpt_reduce_create builds one RCCL communicator clique over the contexts' distinct devices
 * (ncclCommInitAll; contexts sharing a device are summed on it first). bdpt_reduce_frames then
 * enqueues one grouped ncclReduce (sum, fp32) of every context's eye and light frames into the
 * `root` context's frames, on the contexts' streams (under the PathTracer the sampleCountBuffer is
 * summed too); afterwards bdpt_read_frame(root, ...) returns the whole image. The other contexts'
 * frames are unchanged. Async; later work on any listed ctx is ordered after it. The contexts must
 * outlive the reducer and share the frame size and integrator. RCCL is loaded on first use
 * (librccl.so.1); without it these calls fail with BDPT_E_DEVICE. */
typedef struct bdpt_reducer bdpt_reducer;
int bdpt_reduce_create(void* const* ctxs, int32_t n, bdpt_reducer** out);
int bdpt_reduce_frames(bdpt_reducer* r, int32_t root);
/* RCCL ranks of the reducer's communicator (= distinct devices), or BDPT_E_INVALID. */
int bdpt_reduce_ranks(const bdpt_reducer* r);
/* ncclGetVersion of the RCCL that the reducer uses (loads it), or a negative BDPT_E_* code. */
int bdpt_reduce_rccl_version(void);
void bdpt_reduce_destroy(bdpt_reducer* r);

/* Test hook: closest-hit / any-hit queries for a batch of rays through the device BVH
 * (BVHAccel::intersect, bvh.cpp:161-188). rays: n*8 floats {o.xyz, d.xyz, min_t, max_t};
 * out_t[n] (INFINITY if no hit), out_prim[n] (reference primitive index or -1). Sync. */
int bdpt_trace_rays(void* ctx, const float* rays, int32_t n, int32_t any_hit, float* out_t,
                    int32_t* out_prim);

/* Diagnostic hook: the 16 phase-profile words of a BDPT_PHASE_PROF build (cycles of the walks,
 * connection generation and connection rays, walk traversal; walk iterations per wave / per lane;
 * connection-grid cells / pairs). Sync. */
int bdpt_debug_counters(void* ctx, uint64_t* out16);
/* Diagnostic hook (ABI v9): the lane-use profile of a BDPT_PHASE_PROF build — per phase k (closest-hit
 * node steps, closest-hit primitive tests, any-hit node steps, any-hit primitive tests, walk
 * shading, walk iterations, connection evaluations, connection-ray flushes) out16[2k] = wave-level
 * iterations and out16[2k+1] = active lanes summed over them. Sync. Zero in product builds. */
int bdpt_debug_lane_counters(void* ctx, uint64_t* out16);
/* Diagnostic hook (ABI v10): the plan of the ctx's last launch, as the host chose it — out8 = {LDS
 * mode (bdpt_stats.lds_mode), 1 if the traversal stacks have their LDS overflow slots, treelet
 * nodes staged in LDS (LDS mode 2, else 0), dynamic LDS bytes per block, blocks launched, samples
 * per lane and work item, work items (PathTracer: pixel blocks), 1 if the kernel copies the
 * materials and lights to LDS (0: it reads them from global memory)}. -1: no launch yet, or not
 * applicable to the PathTracer's kernel. Touches no device. */
int bdpt_debug_launch_plan(void* ctx, int32_t* out8);

/* Denoised output. New symbols only: no struct above changes and the ABI version
 * stays 10. A context that never calls them allocates nothing and runs nothing for them.
 *
 * The feature pass: per pixel 8 interleaved floats {albedo.rgb, normal.xyz, depth, coverage} of the
 * first hit of the context's integrator's own primary rays (the same origin, direction and clip
 * window as the first closest-hit query of every eye path at the context's seed, lens included), a
 * W*H*8 float frame, row 0 = bottom. Albedo and normal are means over the samples (a miss adds
 * zeros; the normal faces the ray and is not renormalised), depth is the mean hit distance over the
 * samples that hit, coverage the fraction that hit. Albedo by material: diffuse and mirror a,
 * refraction b, glass max(a, b), emission min(a, 1), microfacet its Fresnel reflectance at normal
 * incidence. Deterministic: one lane owns a pixel and sums in sample order.
 *
 * bdpt_render_features renders samples [0, spp_count) (0 = the ctx's spp; otherwise
 * 1 <= spp_count <= spp) of the pixels of the tiles (clipped as bdpt_render clips them; ntiles == 0:
 * the whole frame), overwriting their records. It allocates the feature frame on first use and
 * leaves the eye / light / sample frames, the sample counts and bdpt_stats alone. Async on the ctx
 * stream (a tile list is uploaded after the stream's earlier work has finished). bdpt_clear zeroes
 * the feature frame once it exists. */
int bdpt_render_features(void* ctx, const bdpt_tile* tiles, int32_t ntiles, int32_t spp_count);
/* The feature frame as W*H*8 floats (sync). BDPT_E_INVALID before the first feature pass. */
int bdpt_read_features(void* ctx, float* out8);
int bdpt_features_device_ptr(void* ctx, void** dptr);

/* The edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) of a W*H*3 colour frame C guided
 * by a feature frame: `levels` passes, pass i over the 5x5 taps q = p + 2^i (dx, dy) inside the frame
 * with the B3 kernel h = k[dx] k[dy], k = (1/16, 1/4, 3/8, 1/4, 1/16):
 *   c_{i+1}(p) = sum_q h w(p, q) c_i(q) / sum_q h w(p, q),   w = expf(-(e_c + e_n + e_d)),
 *   e_c = |c_i(p) - c_i(q)|^2 / (sigma_color 2^-i)^2,  e_n = |n(p) - n(q)|^2 / sigma_normal^2,
 *   e_d = ((d(p) - d(q)) / (sigma_depth max(d(p), d(q))))^2 (0 where both depths are 0),
 * the centre tap's w = 1. demodulate: c_0 = C / (albedo + 0.01), out = c_L (albedo + 0.01); off:
 * c_0 = C, out = c_L. levels = 0 with demodulate off returns the input bit for bit.
 * A NULL bdpt_denoise_params pointer means the defaults. levels 0..8, sigmas > 0,
 * reserved words 0. */
typedef struct bdpt_denoise_params {
  int32_t levels;
  float sigma_color, sigma_normal, sigma_depth;
  int32_t demodulate;
  int32_t reserved[3];
} bdpt_denoise_params;
/* Fills *p with the defaults. */
int bdpt_denoise_default_params(bdpt_denoise_params* p);
/* Filters frame `which` (BDPT_FRAME_SAMPLE = eye + light under BDPT) with the ctx's feature frame
 * into the ctx's denoised frame (allocated on first use). Async. BDPT_E_INVALID before the first
 * feature pass. */
int bdpt_denoise(void* ctx, int32_t which, const bdpt_denoise_params* p);
/* The denoised frame, W*H*3 floats, row 0 = bottom (sync). BDPT_E_INVALID before bdpt_denoise. */
int bdpt_read_denoised(void* ctx, float* rgb);
int bdpt_denoised_device_ptr(void* ctx, void** dptr);
/* The same filter on caller device memory of `device`, without a ctx: d_color w*h*3 floats,
 * d_features w*h*8 floats (16-byte aligned), d_out w*h*3 floats (may equal d_color), enqueued on
 * `stream` (a hipStream_t; NULL = the null stream). It allocates its two scratch frames and frees
 * them once the stream has run the filter, so it returns after the result is in d_out. */
int bdpt_denoise_buffers(int32_t device, const float* d_color, const float* d_features, int32_t w, int32_t h,
                         const bdpt_denoise_params* p, float* d_out, void* stream);

/* Variance-guided denoise. New symbols only: no struct above changes and the ABI
 * version stays 10. A context that never calls them allocates nothing and runs nothing for them.
 *
 * Batch moments. A frame rendered as K equal sample batches is the sum of the batches' increments
 * b_k (the 1/spp weight is per sample; disjoint sample ranges are independent). The moments record
 * keeps per pixel one float4 {prev.r, prev.g, prev.b, Q}: after each batch, with f the cumulative
 * colour (under BDPT eye + light, added as BDPT_FRAME_SAMPLE adds them), b = f - prev,
 * Q += (b.x^2 + b.y^2) + b.z^2, prev = f. The variance frame, one float per pixel, W*H floats, row 0
 * = bottom, with 1/K and K/(K-1) rounded to fp32 once:
 *   v = max(0, (Q - ((prev.x^2 + prev.y^2) + prev.z^2) (1/K)) K/(K-1)),
 * the trace of the covariance of the pixel's colour as rendered (the quantity |dc|^2 compares
 * with); an unbiased estimate of the frame's variance when the batches are equal. sqrt(v) is the
 * standard error of the pixel.
 *
 * bdpt_render_batches renders samples [spp_begin, spp_begin + spp_count) of the whole frame as
 * `batches` equal ranges: bdpt_render and a moments pass, `batches` times. batches >= 2,
 * spp_count > 0 and a multiple of batches; a later call adds further batches and must use the same
 * samples per batch. BDPT_E_UNSUPPORTED under the PathTracer (it renders whole pixels; its moments
 * live inside its kernel). Async. bdpt_clear zeroes the record and the batch count. A bdpt_render
 * outside this call marks the frame: bdpt_variance then returns BDPT_E_INVALID until bdpt_clear. */
int bdpt_render_batches(void* ctx, int32_t spp_begin, int32_t spp_count, int32_t batches);
/* Computes the variance frame from the record (allocated on first use). Async. BDPT_E_INVALID with
 * fewer than 2 batches in the record, or when the frame holds samples not rendered in batches. */
int bdpt_variance(void* ctx);
/* The variance frame, W*H floats (sync). BDPT_E_INVALID before bdpt_variance. */
int bdpt_read_variance(void* ctx, float* var);
int bdpt_variance_device_ptr(void* ctx, void** dptr);
/* The raw record, W*H*4 floats (sync). BDPT_E_INVALID before the first bdpt_render_batches. */
int bdpt_read_moments(void* ctx, float* rec4);

/* The variance-guided a-trous filter (after Schied et al. 2017) of a colour frame C with variance
 * frame V: bdpt_denoise's taps, kernel h, in-frame rule, e_n and e_d; per level i
 *   v~(p) = the 3x3 Gaussian (1/4, 1/2, 1/4)^2 of v_i at unit distance around p, in-frame taps only,
 *           divided by the sum of the weights used,
 *   e_c = |c_i(p) - c_i(q)|^2 / (sigma_variance^2 v~(p) + 1e-8),  w = expf(-((e_c + e_n) + e_d)),
 *   c_{i+1}(p) = sum_q h w c_i(q) / sum_q h w   (evaluated as c_i(p) + sum h w (c_i(q) - c_i(p)) / sum h w),
 *   v_{i+1}(p) = sum_q (h w)^2 v_i(q) / (sum_q h w)^2   (and not above the largest v_i(q) of the taps),
 * the centre tap's w = 1. sigma_variance is the same at every level: the variance shrinks instead.
 * No demodulation. levels = 0 returns colour and variance bit for bit.
 * A NULL params pointer means the defaults. levels 0..8, sigmas > 0, reserved 0. */
typedef struct bdpt_denoise_variance_params {
  int32_t levels;
  float sigma_variance, sigma_normal, sigma_depth;
  int32_t reserved[4];
} bdpt_denoise_variance_params;
/* Fills *p with the defaults. */
int bdpt_denoise_variance_default_params(bdpt_denoise_variance_params* p);
/* Filters BDPT_FRAME_SAMPLE with the ctx's variance and feature frames into the ctx's denoised
 * frame (bdpt_read_denoised). Async. BDPT_E_INVALID before a feature pass or before bdpt_variance. */
int bdpt_denoise_variance(void* ctx, const bdpt_denoise_variance_params* p);
/* The same three passes on caller device memory of `device`, without a ctx, enqueued on `stream`
 * (a hipStream_t; NULL = the null stream). d_record w*h*4 floats and d_features w*h*8 floats are
 * 16-byte aligned. bdpt_moments_buffers adds one batch to d_record (zero it before the first):
 * the cumulative frame is d_frame_a, or d_frame_a + d_frame_b when d_frame_b is not NULL (w*h*3
 * floats each); async. bdpt_variance_buffers writes w*h floats to d_var; async.
 * bdpt_denoise_variance_buffers filters d_color (w*h*3) with d_var (w*h) into d_out (may equal
 * d_color) and, when d_var_out is not NULL, the filtered variance into it (may equal d_var); it
 * allocates its scratch frames and returns after the result is in place. */
int bdpt_moments_buffers(int32_t device, const float* d_frame_a, const float* d_frame_b, float* d_record, int32_t w, int32_t h,
                         void* stream);
int bdpt_variance_buffers(int32_t device, const float* d_record, int32_t batches, int32_t w, int32_t h, float* d_var,
                          void* stream);
int bdpt_denoise_variance_buffers(int32_t device, const float* d_color, const float* d_var, const float* d_features, int32_t w,
                                  int32_t h, const bdpt_denoise_variance_params* p, float* d_out, float* d_var_out,
                                  void* stream);

/* Adaptive sampling under BDPT (new symbols, the ABI version stays 10). The frame is
 * rendered in rounds of m = samples_per_round samples over the 8x8 pixel blocks of bdpt_render's
 * whole-frame grid (nbx = (W+7)/8, edge blocks clipped). Round r renders samples [r m, (r+1) m) of the
 * pixels of the blocks still active; a block that has stopped never restarts, so a pixel of a block
 * that was active for K_b rounds holds samples [0, K_b m). With S the ctx's spp (every sample weighs
 * 1/S in the raw frames E and L), R rounds, M_r the pixel-samples of round r and N their sum:
 *   colour    c = fl(fl(a_b E) + fl(g L)),  a_b = S / (K_b m),  g = S W H / N
 *   records   eye   {E.rgb, Q_E}: b = E - prev, Q_E += (b.x^2 + b.y^2) + b.z^2
 *             light {L.rgb, Q_L}: b = L - prev, Q_L += ((b.x^2 + b.y^2) + b.z^2) fl(1 / M_r)
 *   variance  v = a_b^2 K_b/(K_b-1) max(0, Q_E - |E|^2/K_b) + g^2 N/(R-1) max(0, Q_L - |L|^2/N),
 * the trace of the covariance of c in bdpt_variance's units, without the eye-light covariance of a
 * pixel (only the pixel's own K_b m of the N light subpaths correlate with its eye samples).
 * After each round R >= min_rounds a block of n in-frame pixels stops iff
 *   3.8416 Sv (3 n) <= (tol Sc)^2,   Sv = sum v,   Sc = sum (c.x + c.y) + c.z,
 * i.e. 1.96 x the RMS per-channel standard error <= tol x the mean channel value; both sums are
 * xor-butterflies over the block's 64 lanes (lane = x + 8 y, strides 32 .. 1, out-of-frame lanes +0).
 * The render ends when no block is active or after max_rounds rounds. min_rounds == max_rounds
 * == S / m is a uniform render: a_b = g = 1 and c is BDPT_FRAME_SAMPLE bit for bit. */
typedef struct bdpt_adaptive_params {
  int32_t samples_per_round; /* m >= 1; default 32                                               */
  int32_t min_rounds;        /* rounds before the first decision, >= 2; default 4                 */
  int32_t max_rounds;        /* >= min_rounds, max_rounds x m <= spp; 0 = spp / m (the default)    */
  float tolerance;           /* tol >= 0, finite; default 0.05                                    */
  int32_t reserved[4];       /* 0                                                                 */
} bdpt_adaptive_params;
typedef struct bdpt_adaptive_info {
  int32_t rounds;            /* R: rounds run                                                     */
  int32_t active_blocks;     /* blocks still active at the end (they ran into max_rounds)          */
  int64_t samples;           /* N: pixel-samples (= light subpaths) rendered                      */
  int32_t reserved[4];
} bdpt_adaptive_info;
/* The defaults; ctx may be NULL (max_rounds stays 0 = spp / samples_per_round). No device is touched. */
int bdpt_adaptive_default_params(void* ctx, bdpt_adaptive_params* p);
/* Renders the whole frame adaptively (params NULL: the defaults) and returns when it is done (one host
 * wait per round); `out` may be NULL. BDPT_E_UNSUPPORTED under the PathTracer. BDPT_E_INVALID for
 * parameters outside the ranges above and for a frame that already holds samples (bdpt_render,
 * bdpt_render_batches or an earlier adaptive render since bdpt_clear). Afterwards the raw frames hold
 * unequal sample counts: read the image with bdpt_adaptive_resolve / bdpt_read_adaptive;
 * bdpt_variance refuses the frame; a bdpt_render invalidates the adaptive state until bdpt_clear,
 * which zeroes the records, the K_b, N and the flags. bdpt_read_sample_counts is unchanged. */
int bdpt_render_adaptive(void* ctx, const bdpt_adaptive_params* params, bdpt_adaptive_info* out);
/* Computes c, v and the per-pixel sample count K_b m from the records (frames allocated on first use).
 * Async. BDPT_E_INVALID before an adaptive render. */
int bdpt_adaptive_resolve(void* ctx);
/* The resolved frames: rgb W*H*3 floats, var W*H floats, counts W*H int32, row 0 = bottom (sync); any
 * pointer may be NULL. BDPT_E_INVALID before bdpt_adaptive_resolve. */
int bdpt_read_adaptive(void* ctx, float* rgb, float* var, int32_t* counts);
int bdpt_adaptive_device_ptrs(void* ctx, void** d_color, void** d_var, void** d_counts);
/* Per block, in block-index order (nbx x nby int32): K_b, and the active flag (1 = the block ran into
 * max_rounds) (sync). */
int bdpt_read_adaptive_rounds(void* ctx, int32_t* per_block);
int bdpt_read_adaptive_active(void* ctx, int32_t* per_block);
/* The raw records, W*H*4 floats each (sync); either pointer may be NULL. */
int bdpt_read_adaptive_records(void* ctx, float* eye_rec4, float* light_rec4);
/* The four kernels on caller device memory of `device`, without a ctx, enqueued on `stream`; all
 * async. The records (w*h*4 floats) and d_list4 are 16-byte aligned. d_rounds / d_active: one int32 per
 * block. bdpt_adaptive_moments_buffers: one round into the two records, round_samples = M_r.
 * bdpt_adaptive_decide_buffers: K_b += 1 for the active blocks and, when decide != 0, the stopping rule
 * after `rounds` rounds with `samples` pixel-samples in all (rounds >= 2). bdpt_adaptive_compact_buffers:
 * the active blocks as {x, y, w, h} in block order into d_list4 (room for every block) and
 * d_counts2 = {active blocks, their pixels}. bdpt_adaptive_resolve_buffers: c (w*h*3), v (w*h) and
 * K_b m (w*h int32). */
int bdpt_adaptive_moments_buffers(int32_t device, const float* d_eye, const float* d_light, float* d_eye_record, float* d_light_record,
                                  int32_t w, int32_t h, int64_t round_samples, void* stream);
int bdpt_adaptive_decide_buffers(int32_t device, const float* d_eye_record, const float* d_light_record, int32_t* d_rounds,
                                 int32_t* d_active, int32_t w, int32_t h, int32_t spp, int32_t samples_per_round, int32_t rounds,
                                 int64_t samples, float tolerance, int32_t decide, void* stream);
int bdpt_adaptive_compact_buffers(int32_t device, const int32_t* d_active, int32_t w, int32_t h, int32_t* d_list4, int32_t* d_counts2,
                                  void* stream);
int bdpt_adaptive_resolve_buffers(int32_t device, const float* d_eye_record, const float* d_light_record, const int32_t* d_rounds,
                                  int32_t w, int32_t h, int32_t spp, int32_t samples_per_round, int32_t rounds, int64_t samples,
                                  float* d_color, float* d_var, int32_t* d_counts, void* stream);

/* Host-side COLLADA loader: the reference CLI's scene path (ColladaParser::load,
 * collada.cpp:129-941, + Application::load, application.cpp:228-304). width/height > 0 apply
 * Camera::set_screen_size (-r W H). The desc returned by bdpt_dae_get_desc points into the
 * loaded scene and stays valid until bdpt_dae_free. No device is touched. */
typedef struct bdpt_dae bdpt_dae;
int bdpt_dae_load(const char* path, int32_t width, int32_t height, bdpt_dae** out);
int bdpt_dae_get_desc(const bdpt_dae* scene, bdpt_scene_desc* out);
/* Writes the scene in the JSON dump format of tests/golden/scenes (round-trip doubles). */
int bdpt_dae_dump_json(const bdpt_dae* scene, const char* path);
void bdpt_dae_free(bdpt_dae* scene);

/* ABI v5: the CLI's -c camera-settings file (main.cpp:120-121,177-178 -> Application::load_camera
 * -> Camera::load_settings, camera.cpp:172-186), read with the reference's stream extraction order
 * (hFov vFov ar nClip fClip, pos, targetPos, phi theta r minR maxR, c2w row by row, screenW
 * screenH screenDist, focalDistance lensRadius: the format Camera::dump_settings writes). It
 * replaces cam's hfov_deg, vfov_deg, nclip, fclip, pos and c2w. w2c is kept: load_settings does
 * not recompute it (w2c = c2w.inv() only happens in compute_position, camera.cpp:146), so the
 * reference's t = 1 camera connections keep using the placement's inverse — reproduced here.
 * A file that cannot be opened leaves cam unchanged (as the reference's ifstream does) and returns
 * BDPT_E_INVALID. */
int bdpt_camera_load_settings(const char* path, bdpt_camera* cam);
/* ABI v7: the same, also returning the file's focalDistance and lensRadius (its last line), which
 * Camera::load_settings writes over the thin-lens settings the renderer's config gave the camera
 * (raytraced_renderer.cpp:141-142 set_camera runs first, main.cpp:177 load_camera after, and
 * PathTracer::raytrace_pixel reads them in generate_ray_for_thin_lens, pathtracer.cpp:312).
 * *focal_distance / *lens_radius carry the current values in (a short file leaves or zeroes them
 * as the reference's extractions would). Either pointer may be null. */
int bdpt_camera_load_settings_lens(const char* path, bdpt_camera* cam, double* focal_distance, double* lens_radius);

/* Host-side OpenEXR reader for the -e environment map (main.cpp:40-77 load_exr, tinyexr):
 * scanline files with NONE / RLE / ZIPS / ZIP compression and HALF / FLOAT / UINT channels.
 * Like load_exr, the channels are taken in the file's (alphabetical) channel-list order and
 * r, g, b = channels 2, 1, 0 (an RGB file: R, G, B). *rgb_out (width*height*3 floats) is freed
 * with bdpt_exr_free. */
int bdpt_exr_load(const char* path, int32_t* width, int32_t* height, float** rgb_out);
void bdpt_exr_free(float* rgb);

#ifdef __cplusplus
}
#endif

#endif /* BDPT_AMD_BDPT_H */
