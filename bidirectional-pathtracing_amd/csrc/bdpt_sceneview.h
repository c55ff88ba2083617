// bdpt_sceneview.h — what a kernel sees of a scene: materials, lights, the environment map's
// tables, the camera, the leaf encoding and SceneView; the roofline counters and the lane-use
// profile of BDPT_PHASE_PROF builds.

#pragma once

#include "bdpt_math.h"

namespace bdpt {

// ------------------------------------------------------------------------------------------------
// Scene layout in HBM (see DESIGN.md §Data layout)
enum { MAT_DIFFUSE = 0, MAT_EMISSION = 1, MAT_MIRROR = 2, MAT_GLASS = 3, MAT_REFRACTION = 4, MAT_MICROFACET = 5 };
// Vtx::mat of a vertex without BSDF: -1 camera / area or point light vertex, MAT_ENV_V a vertex
// of the environment light (an escaped eye ray, or an env light subpath's first vertex).
// MAT_DIRL_V: the first vertex L[1] of a directional light's subpath (an env vertex whose light no
// escaped ray reaches); stored only, the walk turns it into MAT_ENV_V semantics.
enum { MAT_ENV_V = -2, MAT_DIRL_V = -3 };
// HEMI, DIR: the PathTracer, and BDPT's infinite-light kernels (bdpt_params.infinite_lights, §9a)
enum { LIGHT_AREA = 0, LIGHT_POINT = 1, LIGHT_ENV = 2, LIGHT_HEMI = 3, LIGHT_DIR = 4 };
// Russian roulette (bdpt_params.russian_roulette): vertices with index i > BDPT_RR_MIN continue
// with p_keep = min(1, |f| / pdf) (the rule commented out at bidirection.cpp:87-93).
#define BDPT_RR_MIN 3

struct DMat {
  int type;
  float a[3];    // microfacet: eta
  float b[3];    // microfacet: k
  float ior;
  float alpha;   // microfacet roughness (PathTracer only: BDPT rejects microfacet)
};
struct DLight {
  int type;
  float rad[3], pos[3], dir[3], dx[3], dy[3];
  float area;                 // LIGHT_ENV, and HEMI / DIR under BDPT: pi R^2 of the scene's bounding sphere (emission disk)
  float fx[3], fy[3], fz[3];  // make_coord_space(dir)
};

// Environment light (EnvironmentLight, environment_light.cpp): the map and its sampling tables
// (init(), :18-62) built in fp64 on the host and rounded to fp32, plus the scene's bounding
// sphere that sample_Le emits from.
struct EnvView {
  const float* marg;   // h: marginal_y (CDF over rows)
  const float* cond;   // w*h: conds_y (per-row CDFs)
  const float* pdf;    // w*h: pdf_envmap
  const float* rgb;    // w*h*3: data[w*j + i]
  const int* gmarg;    // gm+1: guide table of marg (null: plain binary search)
  const int* gcond;    // h*(gc+1): guide tables of the rows of cond
  int gm, gc;
  int w, h;
  int light;           // index of the light an escaped ray reaches (-1: none): the env light, or in the
                       // infinite-light kernels a hemisphere light (the tables are then empty)
  float cx, cy, cz, rad;
};
struct DCam {
  float pos[3];
  float c2w[9];  // column-major
  float w2c[9];
  float tanh_, tanv_;  // tan(hFov*PI/360) in fp64, rounded (camera.cpp:199-200)
  float nclip, fclip;
  float lens_r;        // thin-lens radius, read by the lens kernels (EXT = 3) only; it
                       // fills what was the struct's tail padding inside SceneView, so nothing moves
};
static_assert(sizeof(DCam) == 26 * sizeof(float), "DCam: 25 floats + the lens radius");

// Child reference: >= 0 internal node index; < 0 leaf: ~ref = start << 7 | sphere_mask << 3 | count.
BDPT_HD bool ref_is_leaf(int r) { return r < 0; }
BDPT_HD int leaf_start(int r) { return (int)(((uint32_t)~r) >> 7); }
BDPT_HD int leaf_count(int r) { return (int)((uint32_t)~r & 7u); }
BDPT_HD int leaf_sph_mask(int r) { return (int)((((uint32_t)~r) >> 3) & 15u); }

struct SceneView {
  const float4* nodes;   // node_f4(lm_width(LM)) float4 per node (layouts at node_step)
  const float4* geom;    // 3 x float4 per prim (DFS order): tri p0,e1,e2 | sphere c,r
  const float4* shade;   // 3 x float4 per prim: n1 n2 n3 (tri) ; w of the 3rd = material (bits)
  const DMat* mats;
  const DLight* lights;
  int nlights;
  int root;              // root child reference
  const float4* lnodes;  // LDS copy of nodes [0, ntop) (LM 1: all nodes; LM 2: BFS treelet)
  const float4* lgeom;   // LDS copy of the geometry (LM 1 and 3)
  const float4* lshade;  // LDS copy of the shading records (LM 3)
  const int* lleaves;    // LM 3: every leaf reference (LDS), nleaves of them
  int nleaves;
  int fn;                // LM 3: > 0 when the leaves hold primitives 0 .. fn-1 in order (flat_prims)
  uint32_t fsph;         // LM 3: sphere mask of those primitives
  int ntop;
  int* lstack;           // LM 1 / 2: the traversal stacks' first kLdsStack overflow slots in LDS (slot k of
                         // lane t at lstack[k * kLdsStackStride + t]); null: all overflow in scratch
  DCam cam;
  EnvView env;
};

// ------------------------------------------------------------------------------------------------
// Counters for the roofline (algorithmic bytes)
struct Counters {
  uint32_t nodes, tris, sphs, closest, shadow, hits;
  uint32_t lnodes = 0;   // of `nodes`: child AABBs read from the block's LDS copy (LM 1, LM 2 treelet)
  uint32_t env_s = 0, env_l = 0, env_p = 0;   // environment-light samples / radiance / pdf lookups
#ifdef BDPT_PHASE_PROF
  // wave-level cycles (each interval counted by the wave's lowest active lane, BDPT_WAVE_CLK; the
  // kernel sums its lanes): in the walk's closest-hit queries, drawing the light vertex L[1]
  // (sample_light_ray), and from a hit to the next ray (shading record, vertex, sample_f)
  unsigned long long clk_walk_trace = 0;
  unsigned long long clk_light = 0;
  unsigned long long clk_vertex = 0;
  // lane use per phase: [2k] wave-level iterations (counted by the wave's lowest active lane),
  // [2k + 1] active lanes summed over them (every active lane counts itself); k = LP_*
  uint32_t lp[2 * 8] = {};
#endif
};

// Phases of the lane-use profile (BDPT_PHASE_PROF builds, bdpt_debug_lane_counters).
enum {
  LP_CNODE = 0,   // closest-hit node steps (walk rays)
  LP_CPRIM = 1,   // closest-hit primitive tests
  LP_ANODE = 2,   // any-hit node steps (connection rays)
  LP_APRIM = 3,   // any-hit primitive tests
  LP_SHADE = 4,   // walk: hit -> next ray (shading record, vertex, MIS constants, sample_f)
  LP_WALK = 5,    // walk iterations (one closest-hit query each)
  LP_CONN = 6,    // connection evaluations (make_conn)
  LP_FLUSH = 7    // connection-ray flushes: wave-level flushes / rays traced
};
#if defined(BDPT_PHASE_PROF) && defined(__HIP_DEVICE_COMPILE__)
#define BDPT_LANE_PROF(c, k)                                                                      \
  do {                                                                                            \
    const unsigned long long m_ = __ballot(1);                                                    \
    if ((unsigned)__lane_id() == (unsigned)__builtin_ctzll(m_)) (c).lp[2 * (k)]++;                \
    (c).lp[2 * (k) + 1]++;                                                                        \
  } while (0)
// a wave-level interval of dt cycles (s_memtime is the wave's clock): added once, by the lowest
// active lane, so that an interval is counted whichever lanes take part in it
#define BDPT_WAVE_CLK(acc, dt)                                                                    \
  do {                                                                                            \
    const unsigned long long m_ = __ballot(1);                                                    \
    if ((unsigned)__lane_id() == (unsigned)__builtin_ctzll(m_)) (acc) += (dt);                    \
  } while (0)
#else
#define BDPT_LANE_PROF(c, k) \
  do {                       \
  } while (0)
#endif

}  // namespace bdpt
