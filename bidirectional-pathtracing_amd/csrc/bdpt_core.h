// bdpt_core.h — device-side BDPT per-sample pipeline for MI355X (gfx950), single-source so the
// host part of libbdpt_amd.so can precompute light frames with the same arithmetic.
//
// What it computes is the reference's per-pixel-sample estimator
//   BidirectionalPathTracer::raytrace_pixel / est_radiance_global_illumination
//   (src/pathtracer/bidirection.cpp:472-542)
// in the fp32 "device semantics" of DESIGN.md §fp32: every expression keeps the reference's
// operation order (CGL Vector3D semantics), uniforms come from Philox4x32-10 keyed by
// (seed, pixel, sample), sin/cos(2*pi*u) from a fixed polynomial, cos(acos z) = z, integer
// powers by products, and the sphere quadratic in fp64. The oracle's COUNTER32 mode
// (oracle/bdpt_oracle.cpp) restates the same semantics independently; parity is per sample.
//
// How it differs from the reference's *structure* (output-identical):
//  * BVH2 with both child boxes in the parent, near-first ordered traversal, t-culling against
//    conservatively padded fp32 boxes; ties in t resolved to the larger DFS leaf position, which
//    is what the reference's l->r exhaustive traversal with `t <= max_t` yields (bvh.cpp:161-188).
//  * Connection (shadow) rays use an any-hit traversal: only their boolean is consumed
//    (bidirection.cpp:428-433).
//  * The MIS walk (bidirection.cpp:121-293) is O(i+j) multiplies per connection: the per-vertex
//    ratios nom/denom of the non-endpoint steps are path constants, evaluated once per subpath
//    with the reference's exact operations and reused; only the two endpoint steps are evaluated
//    per connection.
//  * Connections whose contribution is identically zero (non-diffuse endpoint BSDF, f = 0
//    hemisphere test, zero throughput) skip their shadow ray (quirk 17).
//
// This header is the umbrella include; the code lives in bdpt_math.h, bdpt_sceneview.h, bdpt_bvh.h,
// bdpt_bsdf.h, bdpt_env.h, bdpt_paths.h (the estimator above) and bdpt_pt.h (the PathTracer).

#pragma once

#include "bdpt_paths.h"
#include "bdpt_pt.h"
