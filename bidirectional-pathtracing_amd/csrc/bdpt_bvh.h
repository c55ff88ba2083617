// bdpt_bvh.h — ray queries: the primitive tests, the traversal stack, the node step and the
// closest-hit / any-hit BVH traversals (replace BVHAccel::intersect), and a hit's shading record.

#pragma once

#include "bdpt_sceneview.h"

namespace bdpt {

struct Hit {
  float t;
  int prim;   // position in the device tree's leaf order, -1 = none
  int key;    // position in the reference tree's DFS leaf order (tie-break)
  float b1, b2;
};

// Both predicates with non-short-circuit & / |: each term a lane mask, combined without a branch.
// Written with && / || (and the early-outs joined by ||), the compiler emitted an exec-mask branch
// per term — ~40 scalar / vector instructions per check in the leaf loops; flat, the north-star
// kernel has 650 fewer static instructions and runs +3.3 % (CBspheres +14 %, CBgems m7 +5 %,
// profiles/r06v_ab_tri_flat.log). Same predicates, same results.
BDPT_HD bool quot_neg(float n, float d) {
  return (((n < 0) & (d > 0)) | ((n > 0) & (d < 0))) & (fabsf(n) >= fabsf(d) * 8.67361738e-19f);  // 2^-60
}
BDPT_HD bool quot_gt1(float n, float d) {
  return (((n > 0) & (d > 0)) | ((n < 0) & (d < 0))) & (fabsf(n) > fabsf(d));
}

// Möller–Trumbore exactly as Triangle::intersect (triangle.cpp:57-95), fp32.
BDPT_HD bool tri_test(const float4 g0, const float4 g1, const float4 g2, f3 o, f3 d, float tmin, float tmax,
                      float* t_out, float* b1_out, float* b2_out) {
  f3 p0 = mk3(g0.x, g0.y, g0.z);
  f3 e1 = mk3(g0.w, g1.x, g1.y);
  f3 e2 = mk3(g1.z, g1.w, g2.x);
  f3 s = sub(o, p0);
  f3 s1 = cross(d, e2);
  float denom = dot(s1, e1);
  float n1 = dot(s1, s);
  // Exact early-outs before the three correctly-rounded divisions: only when the rounded
  // quotient is certainly < 0 (opposite signs, |q| >= 2^-60 so it cannot round to -0) or > 1
  // (|n| > |denom| implies fl(n/denom) > 1), i.e. exactly when the reference test fails anyway.
  if (quot_neg(n1, denom) | quot_gt1(n1, denom)) return false;
  f3 s2 = cross(s, e1);
  float n2 = dot(s2, d);
  if (quot_neg(n2, denom) | quot_gt1(n2, denom)) return false;
  float nt = dot(s2, e2);
  if ((tmin >= 0) & quot_neg(nt, denom)) return false;
  float t = nt / denom;
  float b1 = n1 / denom;
  float b2 = n2 / denom;
  *t_out = t; *b1_out = b1; *b2_out = b2;
  return (t >= tmin) & (t <= tmax) & (b1 >= 0) & (b2 >= 0) & (b1 + b2 <= 1);
}

// Sphere::test + intersect (sphere.cpp:11-35,61-93) with the quadratic in fp64.
BDPT_HD bool sph_test(const float4 g0, f3 o, f3 d, float tmin, float tmax, float* t_out) {
  {
    // Conservative fp32 miss test: squared distance of the centre from the ray's line exceeds r^2
    // by far more than the fp32 error (~1e-6 |o-c|^2), so the fp64 discriminant is < 0 too.
    f3 f = sub(o, mk3(g0.x, g0.y, g0.z));
    float a = norm2(d), bh = dot(f, d), ff = norm2(f);
    float dl2a = ff * a - bh * bh;   // a * dist^2(centre, line)
    if (dl2a > a * (g0.w * g0.w * 1.001f + ff * 1e-5f)) return false;
  }
  double ox = o.x, oy = o.y, oz = o.z, dx = d.x, dy = d.y, dz = d.z;
  double cx = g0.x, cy = g0.y, cz = g0.z, r = g0.w;
  double r2 = r * r;
  double a = dx * dx + dy * dy + dz * dz;
  double fx = ox - cx, fy = oy - cy, fz = oz - cz;
  double b = 2 * (fx * dx + fy * dy + fz * dz);
  double c = (fx * fx + fy * fy + fz * fz) - r2;
  double delta = b * b - 4 * a * c;
  if (delta < 0) return false;
  double root = sqrt(delta);
  double t1 = (-b - root) / (2 * a);
  double t2 = (-b + root) / (2 * a);
  const bool in1 = (t1 >= (double)tmin) & (t1 <= (double)tmax), in2 = (t2 >= (double)tmin) & (t2 <= (double)tmax);
  const double t = in1 ? t1 : in2 ? t2 : -1.0;
  if (t > 0) {
    *t_out = (float)t;
    return true;
  }
  return false;
}

// ------------------------------------------------------------------------------------------------
// BVH traversal (replaces BVHAccel::intersect, bvh.cpp:161-188; see header comment).
#ifndef BDPT_STACK_MAX
#define BDPT_STACK_MAX 64
#endif
constexpr int kStackMax = BDPT_STACK_MAX;   // variant builds may override (-DBDPT_STACK_MAX=...)
// Register-stack entries of the megakernel's walk / connection-ray traversals (TravStack<K>).
// Measured (Lucy stand-in 1080p / CBspheres / CBgems, Msamples/s): K 0: 440 / 438 / 273,
// K 2: 465 / 452 / 284, K 4: 465 / 450 / 290 (walk 8 or connection 8: no further gain). Round 4,
// with 8 LDS slots behind them (kLdsStack): walk / connection 2/2, 3/3, 2/4, 4/2 lose 0.6 .. 1.7 %
// on the north star (profiles/r04k_ab_regstack.log). Round 5, with the LDS slots: 0 / 0 and 0 / 4
// -0.5 % on the north star, 4 / 0 +-0.2 %; with the tree in HBM (no LDS slots) 0 / 0 -10 %, and on
// CBgems (LM 1) -2 % (profiles/r05y_ab_regstack.log). Round 6, after the leaner node step: 3 / 3,
// 2 / 2, 4 / 2, 2 / 4 lose 0.4 .. 1 % on the north star, up to 2 % on CBgems (r06z3_ab_regstack.log).
#ifndef BDPT_WALK_STACK
#define BDPT_WALK_STACK 4
#endif
#ifndef BDPT_CONN_STACK
#define BDPT_CONN_STACK 4
#endif
constexpr int kWalkStack = BDPT_WALK_STACK;   // variant builds may override (-DBDPT_WALK_STACK=...)
constexpr int kConnStack = BDPT_CONN_STACK;
// Children per BVH node: 2 (64-B nodes) or 4 (128-B nodes: half the dependent node fetches per
// ray, four independent slab tests per fetch). The host emits both trees over the same leaves;
// a kernel traverses the one its LDS mode selects: scenes fetched from HBM (LM 0, LM 2's nodes below
// the treelet) gain from the shorter dependent chain, a scene held whole in LDS (LM 1) does not
// (its fetches are short, and the wider test costs instructions). Measured, DESIGN.md §5.
constexpr int kBvhWidth = 4;       // LM 0 / 2
constexpr int kLdsBvhWidth = 2;   // LM 1
static_assert((kBvhWidth == 2 || kBvhWidth == 4) && (kLdsBvhWidth == 2 || kLdsBvhWidth == 4),
              "BVH widths must be 2 or 4");
// Child visiting order of the 4-wide node step: 0 = slot order (any-hit connection rays),
// 1 = near-first by a sorting network (closest-hit queries).
constexpr int kAnyOrd = 0, kClosestOrd = 1;

// BVH leaves: the next primitive's record is loaded before the current one is tested, where the
// geometry comes from HBM (LM 0 / 2). Measured: Lucy stand-in 1080p 489 -> 516, CBbunny 800x600
// 351 -> 370 Msamples/s; with the geometry in LDS (LM 1, CBgems) 303 -> 299, so off there. LM 3
// walks its flat list the same way (S.fn > 0).
BDPT_HD constexpr bool leaf_prefetch(int LM) { return LM == 0 || LM == 2; }

// Speculative while-while (Aila & Laine 2009; trace_closest / trace_any): a lane holding a
// postponed leaf keeps descending while other lanes still look for theirs; leaves are tested once
// every lane holds one (or is done). Where the nodes come from HBM (LM 0 / 2) the extra node steps
// fill the lanes that would otherwise wait: Lucy stand-in 601 -> 631, C5-shaped 468 -> 485
// Msamples/s; with the whole tree in LDS (LM 1) the longer steps cost more than the latency they
// hide (CBgems m7 269 -> 247), so only LM 0 / 2. Variants measured and removed: two
// postponed leaves per lane, stopping the descent once fewer than 4 / 8 / 16 lanes still look.
BDPT_HD constexpr bool spec_trav(int LM) { return LM == 0 || LM == 2; }
// active lanes of the wave for which the predicate holds (the host build runs one lane)
BDPT_HD int wave_count(bool p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popcll(__ballot(p));
#else
  return p ? 1 : 0;
#endif
}
// LM 3 (flat): tiny scenes test every leaf in order, no node fetches, no stack, no divergence
// in the traversal loop (same hits and tie rule as a tree walk, bdpt_scene.cpp leaf_refs).
BDPT_HD constexpr int lm_width(int LM) { return LM == 1 || LM == 3 ? kLdsBvhWidth : kBvhWidth; }
BDPT_HD constexpr int node_f4(int W) { return W == 4 ? 8 : 4; }        // float4 per node (stride)
BDPT_HD constexpr int node_used_f4(int W) { return W == 4 ? 7 : 4; }   // float4 a traversal reads
BDPT_HD constexpr int node_bytes(int W) { return 16 * node_f4(W); }

// Traversal stack: the newest K entries in registers (shifted on push/pop, fully unrolled), older
// ones in a private array (K = 0: all of it). Near-first traversal of these trees rarely holds more
// than ~8 entries; a few register entries keep most pushes/pops off scratch.
// The overflow below the register entries: its first kLdsStack slots in LDS when the kernel gives
// the stack an LDS area (SceneView::lstack, LM 1 / 2; one lane's slot k at lstack[k * stride + lane], no
// bank conflicts), deeper ones in the private array. A pop from LDS puts the next node address on
// the critical path after an LDS read instead of a scratch (L1 / L2) read. The 32 KB come out of the
// LM-2 treelet (~430 -> ~180 nodes). Measured (profiles/r04i_ab_lds_stack.log, Msamples/s, 0 / 4 /
// 8 / 12 slots): north star 681 / 690 / 689 / 679, C5-shaped 580 / 586 / 590 / 579, C3 465 / 471 /
// 471 / 465, CBbunny 800x600 510 / 517 / 515 / 508.
constexpr int kLdsStack = 8;
constexpr int kLdsStackStride = 1024;   // lanes per block (bdpt_hip.hip kBlock)

// this lane's LDS overflow slots (device, LM 1 / 2 kernels that staged them), else null
BDPT_HD int* lane_stack(const SceneView& S) {
#if defined(__HIP_DEVICE_COMPILE__)
  return kLdsStack > 0 && S.lstack ? S.lstack + threadIdx.x : nullptr;
#else
  return nullptr;
#endif
}

#if defined(BDPT_STEP_HIST) && !defined(__HIP_DEVICE_COMPILE__)
}  // namespace bdpt
#include <vector>
namespace bdpt {
inline unsigned long long* step_hist() { static thread_local unsigned long long h[1024]; return h; }
inline int& step_hist_nested() { static thread_local int n = 0; return n; }
// diagnostics: the any-hit queries' rays (o, d, tmin, tmax) while a sink is set (tools/anyhit_probe.py)
inline std::vector<float>*& ray_dump() { static thread_local std::vector<float>* v = nullptr; return v; }
// diagnostics: while a sink is set, a log of int triples (tools/flush_sim.py). Every any-hit query
// adds (tag, node steps, primitive tests), tag = anyhit_tag() as render_sample set it (i << 8 | j);
// render_sample opens each pixel-sample with (-1, conn_e mask, conn_l mask) and (-2, src_e mask, nL),
// the lists the megakernel's connect_sample walks (masks cut to 32 bits: depths up to 30).
inline std::vector<int>*& anyhit_log() { static thread_local std::vector<int>* v = nullptr; return v; }
inline int& anyhit_tag() { static thread_local int t = 0; return t; }
#endif
template <int K>
struct TravStack {
  int s[K > 0 ? K : 1];
  int nreg, msp;
  int* mem;   // a separate private array, so that s[] / nreg / msp stay in registers
  int* lds;   // this lane's LDS overflow slots (stride kLdsStackStride), or null
  BDPT_HD explicit TravStack(int* m, int* l = nullptr) : nreg(0), msp(0), mem(m), lds(l) {}
  BDPT_HD void clear() { nreg = 0; msp = 0; }
  BDPT_HD int size() const { return nreg + msp; }
  BDPT_HD void put(int k, int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (kLdsStack > 0 && lds && k < kLdsStack) {
      *(__attribute__((address_space(3))) int*)(lds + k * kLdsStackStride) = v;
      return;
    }
#endif
    mem[k] = v;
  }
  BDPT_HD int get(int k) const {
#if defined(__HIP_DEVICE_COMPILE__)
    if (kLdsStack > 0 && lds && k < kLdsStack) return *(const __attribute__((address_space(3))) int*)(lds + k * kLdsStackStride);
#endif
    return mem[k];
  }
  BDPT_HD void push(int v) {
    if (K == 0) {
      put(msp++, v);
      return;
    }
    if (nreg == K) {
      put(msp++, s[K - 1]);
    } else {
      nreg++;
    }
#pragma unroll
    for (int k = K - 1; k > 0; k--) s[k] = s[k - 1];
    s[0] = v;
  }
  BDPT_HD bool pop(int& v) {
    if (K > 0 && nreg > 0) {
      v = s[0];
#pragma unroll
      for (int k = 0; k + 1 < K; k++) s[k] = s[k + 1];
      nreg--;
      return true;
    }
    if (msp == 0) return false;
    v = get(--msp);
    return true;
  }
};

struct RayInv {
  f3 o, d, inv, oi;   // oi = o * inv: slab planes are fma(p, inv, -oi)
  // 4-wide nodes: byte offset (0 or 16) of each axis' near plane row within its lo / hi row pair
  // (the hi row when the direction component is negative), so that a lane loads its near and far
  // rows directly and the per-axis min / max of the two plane distances disappears
  int nx, ny, nz;
};
// A zero direction component would give an infinite inverse and NaN / wrong-signed plane distances
// (inf - inf); it is replaced by +-2^-100, whose plane distances are huge and of the right sign, so a
// parallel ray is inside a slab exactly when its origin is (up to the boxes' padding).
BDPT_HD float safe_inv(float x) {
  const float tiny = 7.88860905e-31f;   // 2^-100
  return 1.0f / (fabsf(x) < tiny ? copysignf(tiny, x) : x);
}
BDPT_HD RayInv make_rayinv(f3 o, f3 d) {
  RayInv r;
  r.o = o; r.d = d;
  r.inv = mk3(safe_inv(d.x), safe_inv(d.y), safe_inv(d.z));
  r.oi = mk3(o.x * r.inv.x, o.y * r.inv.y, o.z * r.inv.z);
  r.nx = r.inv.x < 0.0f ? 16 : 0;
  r.ny = r.inv.y < 0.0f ? 16 : 0;
  r.nz = r.inv.z < 0.0f ? 16 : 0;
  return r;
}
// Slab test against a padded (conservative) box (2-wide nodes; 4-wide nodes load the near and far
// rows directly, node_step). The fused form rounds differently from (p - o) * inv by at most ulp(o * inv) in t, far inside
// the 2^-16 box padding, so it never culls a box a hit lies in (results do not depend on it).
BDPT_HD void slab(const RayInv& r, float lx, float ly, float lz_, float hx, float hy, float hz,
                  float* tn, float* tf) {
  const float t0x = fmaf(lx, r.inv.x, -r.oi.x), t1x = fmaf(hx, r.inv.x, -r.oi.x);
  const float t0y = fmaf(ly, r.inv.y, -r.oi.y), t1y = fmaf(hy, r.inv.y, -r.oi.y);
  const float t0z = fmaf(lz_, r.inv.z, -r.oi.z), t1z = fmaf(hz, r.inv.z, -r.oi.z);
  const float n = fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fminf(t0z, t1z));
  const float f = fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fmaxf(t0z, t1z));
  *tn = n;
  *tf = f * 1.00000024f;
}

// Traversal loops are "while-while" (Aila & Laine 2009): an inner loop descends internal nodes
// until this lane stands on a leaf (or its stack is empty), then the leaf's primitives are tested.
// In a wave, every lane runs node steps together and then leaf tests together, instead of each
// iteration paying for both code paths. Each lane visits nodes in the same near-first order as a
// plain loop, so hits and counters do not change.
constexpr int kTravDone = (int)0x80000000;   // not a valid leaf reference (start would be 2^24)

// Scene fetches with explicit address spaces on the device: the LDS copy is read with ds_read and
// the HBM arrays with global_load (through a generic pointer both would compile to flat_load).
BDPT_HD float4 ld_lds4(const float4* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return *(const __attribute__((address_space(3))) float4*)p;
#else
  return *p;
#endif
}
BDPT_HD float4 ld_glb4(const float4* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return *(const __attribute__((address_space(1))) float4*)p;
#else
  return *p;
#endif
}
// geometry record k (3 float4 per primitive): LDS copy in LDS mode 1, else HBM
template <int LM>
BDPT_HD float4 ld_geom(const SceneView& S, int k) {
  return LM == 1 || LM == 3 ? ld_lds4(S.lgeom + k) : ld_glb4(S.geom + k);
}
// primitive pi's whole record (3 float4). From HBM: the array's base as the scalar part of the
// address, a 32-bit per-lane offset, the rows' 0 / 16 / 32 in the immediate field.
template <int LM>
BDPT_HD void ld_rec3(const SceneView& S, int pi, float4& a0, float4& a1, float4& a2) {
  if (LM == 1 || LM == 3) {
    a0 = ld_lds4(S.lgeom + 3 * pi); a1 = ld_lds4(S.lgeom + 3 * pi + 1); a2 = ld_lds4(S.lgeom + 3 * pi + 2);
  } else {
    const char* b = (const char*)S.geom;
    const size_t o = (size_t)((uint32_t)pi * 48u);
    a0 = ld_glb4((const float4*)(b + o));
    a1 = ld_glb4((const float4*)(b + 16 + o));
    a2 = ld_glb4((const float4*)(b + 32 + o));
  }
}
BDPT_HD int ld_lds_i(const int* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return *(const __attribute__((address_space(3))) int*)p;
#else
  return *p;
#endif
}
// A 4-wide node's rows as the ray sees them: v[0] / v[1] = the x plane rows nearer / farther along
// the ray (lo.x / hi.x, swapped when the direction's x is negative), v[2] / v[3] y, v[4] / v[5] z,
// v[6] the child references. Byte offsets within node ref: near = 128 ref + 32 a + n_a, far =
// 128 ref + 32 a + 16 - n_a. The address is the node array's base (wave-uniform: the scalar part of
// a global load) plus a 32-bit per-lane byte offset, the row's constant part in the immediate field:
// against a 64-bit address per row (round 6, profiles/r06qrs_ab_lean_node.log) the per-ray offsets
// take 6 VGPRs instead of 12 and the north-star kernel's static scratch instructions fall 236 -> 187.
// 32-bit offsets suffice: a scene holds < 2^24 primitive references (bdpt_scene.cpp), so < 2^25 binary
// and fewer 4-wide nodes, 128 ref + 112 < 2^32; the records (ld_rec3) are < 48 * 2^24 bytes.
BDPT_HD void ld_node4_oct_glb(const float4* nodes, int ref, const RayInv& r, float4* v) {
  const char* b = (const char*)nodes;
  const uint32_t o = (uint32_t)ref * 128u;
  const uint32_t nx = (uint32_t)r.nx, ny = (uint32_t)r.ny, nz = (uint32_t)r.nz;
  v[0] = ld_glb4((const float4*)(b + (size_t)(o + nx)));
  v[1] = ld_glb4((const float4*)(b + (size_t)(o + (16u - nx))));
  v[2] = ld_glb4((const float4*)(b + 32 + (size_t)(o + ny)));
  v[3] = ld_glb4((const float4*)(b + 32 + (size_t)(o + (16u - ny))));
  v[4] = ld_glb4((const float4*)(b + 64 + (size_t)(o + nz)));
  v[5] = ld_glb4((const float4*)(b + 64 + (size_t)(o + (16u - nz))));
  v[6] = ld_glb4((const float4*)(b + 96 + (size_t)o));
}
// The same as one asm block: the seven loads issue back to back under one wait. LM 0 (every node from
// HBM) needs it: left to the compiler, its loads were spaced by waits and the reference row (needed
// only once a child is hit) sank behind the slab tests, a second dependent fetch per step (LM 0
// 703 -> 647). LM 2's HBM path (waves with a lane below the treelet) runs faster with the compiler's
// schedule (north star 782 asm vs 792), so it keeps the C++ form.
BDPT_HD void ld_node4_oct_glb_asm(const float4* nodes, int ref, const RayInv& r, float4* v) {
#if defined(__HIP_DEVICE_COMPILE__)
  const char* b = (const char*)nodes;
  const uint32_t o = (uint32_t)ref * 128u;
  const uint32_t nx = (uint32_t)r.nx, ny = (uint32_t)r.ny, nz = (uint32_t)r.nz;
  typedef float v4f __attribute__((ext_vector_type(4)));
  v4f t[7];
  asm volatile(
      "global_load_dwordx4 %0, %7, %14\n\t"
      "global_load_dwordx4 %1, %8, %14\n\t"
      "global_load_dwordx4 %2, %9, %14 offset:32\n\t"
      "global_load_dwordx4 %3, %10, %14 offset:32\n\t"
      "global_load_dwordx4 %4, %11, %14 offset:64\n\t"
      "global_load_dwordx4 %5, %12, %14 offset:64\n\t"
      "global_load_dwordx4 %6, %13, %14 offset:96\n\t"
      "s_waitcnt vmcnt(0)"
      : "=&v"(t[0]), "=&v"(t[1]), "=&v"(t[2]), "=&v"(t[3]), "=&v"(t[4]), "=&v"(t[5]), "=&v"(t[6])
      : "v"(o + nx), "v"(o + (16u - nx)), "v"(o + ny), "v"(o + (16u - ny)), "v"(o + nz), "v"(o + (16u - nz)),
        "v"(o), "s"(b));
#pragma unroll
  for (int k = 0; k < 7; k++) v[k] = make_float4(t[k].x, t[k].y, t[k].z, t[k].w);
#else
  ld_node4_oct_glb(nodes, ref, r, v);
#endif
}
// the same from the LDS copy
BDPT_HD void ld_node4_oct_lds(const float4* p, const RayInv& r, float4* v) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef float v4f __attribute__((ext_vector_type(4)));
  const uint32_t a = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) float4*)p;
  const int nx = r.nx, ny = r.ny, nz = r.nz;
  v4f t[7];
  // one asm block of ds_read_b128 and a single wait (a node fetch that may come from LDS or HBM, as in
  // the treelet mode, otherwise compiles to flat_load for both): near rows at a + n + 32 axis, far
  // rows at a - n + 32 axis + 16
  asm volatile(
      "ds_read_b128 %0, %7\n\t"
      "ds_read_b128 %1, %8 offset:16\n\t"
      "ds_read_b128 %2, %9 offset:32\n\t"
      "ds_read_b128 %3, %10 offset:48\n\t"
      "ds_read_b128 %4, %11 offset:64\n\t"
      "ds_read_b128 %5, %12 offset:80\n\t"
      "ds_read_b128 %6, %13 offset:96\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(t[0]), "=&v"(t[1]), "=&v"(t[2]), "=&v"(t[3]), "=&v"(t[4]), "=&v"(t[5]), "=&v"(t[6])
      : "v"(a + nx), "v"(a - nx), "v"(a + ny), "v"(a - ny), "v"(a + nz), "v"(a - nz), "v"(a));
#pragma unroll
  for (int k = 0; k < 7; k++) v[k] = make_float4(t[k].x, t[k].y, t[k].z, t[k].w);
#else
  ld_node4_oct_glb(p, 0, r, v);
#endif
}

// One node of the descent: slab-test the children, continue with the nearest hit child, push the
// other hit children (farther first, so they pop near-first); pop when none is hit.
// Width 2, 4 float4: lo_l.xyz hi_l.x | hi_l.yz lo_r.xy | lo_r.z hi_r.xyz | refs
// Width 4, 8 float4: lo.x[4] | hi.x[4] | lo.y[4] | hi.y[4] | lo.z[4] | hi.z[4] | refs[4] | pad,
// fetched in near / far order per axis (ld_node4_oct_*)
// ORD: visit hit children near-first (closest-hit queries); any-hit queries take them in slot order.
// A child is entered when its slab interval, clipped to [tmin, tmax], is non-empty.
template <int K, int LM, int ORD = 1>
BDPT_HD int node_step(const SceneView& S, const RayInv& r, int ref, float tmin, float tmax, TravStack<K>& stk,
                      Counters& c) {
  constexpr int W = lm_width(LM), NU = node_used_f4(W);
  float4 v[NU];
  if (W == 4) {
    // rows in near / far order (ld_node4_oct_*). LM 2: the treelet (LDS) and HBM lanes of one wave
    // would run a lane-divergent if / else over the same registers — the global loads, a wait for
    // them (the ds_reads would overwrite their registers), then the ds_reads: HBM latency + LDS
    // latency. So only a wave whose lanes are all in the treelet reads LDS; any other wave fetches
    // every lane's node from HBM (the treelet nodes are there too, and hot in L2).
    if (LM == 2) {
      const bool in_lds = ref < S.ntop;
#if defined(__HIP_DEVICE_COMPILE__)
      const bool all_lds = __ballot(in_lds) == __ballot(true);
#else
      const bool all_lds = in_lds;
#endif
      if (all_lds) {
        ld_node4_oct_lds(S.lnodes + node_f4(W) * ref, r, v);
        c.lnodes += W;
      } else {
        ld_node4_oct_glb(S.nodes, ref, r, v);
      }
    } else if (LM == 1) {
      ld_node4_oct_lds(S.lnodes + node_f4(W) * ref, r, v);
      c.lnodes += W;
    } else {
      ld_node4_oct_glb_asm(S.nodes, ref, r, v);
    }
  } else if (LM == 1) {   // 2-wide, all nodes in LDS: plain ds_reads the compiler schedules
#pragma unroll
    for (int k = 0; k < NU; k++) v[k] = ld_lds4(S.lnodes + node_f4(W) * ref + k);
    c.lnodes += W;
  } else {
#pragma unroll
    for (int k = 0; k < NU; k++) v[k] = ld_glb4(S.nodes + node_f4(W) * ref + k);
  }
  if (W == 2) {
    const float4 a = v[0], b = v[1], cc = v[2], e = v[3 % NU];
    c.nodes += 2;
    float tnl, tfl, tnr, tfr;
    slab(r, a.x, a.y, a.z, a.w, b.x, b.y, &tnl, &tfl);
    slab(r, b.z, b.w, cc.x, cc.y, cc.z, cc.w, &tnr, &tfr);
    const bool hl = fmaxf(tnl, tmin) <= fminf(tfl, tmax);
    const bool hr = fmaxf(tnr, tmin) <= fminf(tfr, tmax);
    const int lref = __float_as_int(e.x), rref = __float_as_int(e.y);
    if (hl && hr) {
      const bool lfirst = ORD == 0 || tnl <= tnr;
      stk.push(lfirst ? rref : lref);
      return lfirst ? lref : rref;
    }
    if (hl) return lref;
    if (hr) return rref;
    int nx;
    return stk.pop(nx) ? nx : kTravDone;
  } else {
    c.nodes += 4;
    int r0, r1, r2, r3;
    float tn0, tn1, tn2, tn3;
    bool h0, h1, h2, h3;
    const float4 lx = v[0], hx = v[1], ly = v[2 % NU], hy = v[3 % NU];
    const float4 lz = v[4 % NU], hz = v[5 % NU], e = v[6 % NU];
    r0 = __float_as_int(e.x); r1 = __float_as_int(e.y); r2 = __float_as_int(e.z); r3 = __float_as_int(e.w);
    float tf;
    // lx / ly / lz are the near rows, hx / hy / hz the far rows (ld_node4_oct_*): with a finite
    // inverse the near plane's distance is the smaller of the two (the fma is monotone in the plane
    // coordinate), so this is slab()'s test without its per-axis min / max — 6 fewer VALU per child,
    // the same visits. Measured against slab() (profiles/r05l_ab_oct_rows.log): north star +0.3 %,
    // C5-shaped +1.2 %, CBbunny +0.3 %, the stand-in with the tree in HBM (LM 0) +2.5 %.
#define BDPT_SLAB_OCT(C, TN, TF)                                                             \
  {                                                                                          \
    TN = fmaxf(fmaxf(fmaf(lx.C, r.inv.x, -r.oi.x), fmaf(ly.C, r.inv.y, -r.oi.y)),            \
               fmaf(lz.C, r.inv.z, -r.oi.z));                                                \
    TF = fminf(fminf(fmaf(hx.C, r.inv.x, -r.oi.x), fmaf(hy.C, r.inv.y, -r.oi.y)),            \
               fmaf(hz.C, r.inv.z, -r.oi.z)) * 1.00000024f;                                  \
  }
    // An empty slot (reference kTravDone) holds an inverted infinite box (bdpt_scene.cpp): its near
    // distance is +inf and its far one -inf, so its test fails without a look at the reference, and
    // the reference row is needed only once a child is hit (round 6: north star +1.7 % by itself).
    BDPT_SLAB_OCT(x, tn0, tf);
    h0 = fmaxf(tn0, tmin) <= fminf(tf, tmax);
    BDPT_SLAB_OCT(y, tn1, tf);
    h1 = fmaxf(tn1, tmin) <= fminf(tf, tmax);
    BDPT_SLAB_OCT(z, tn2, tf);
    h2 = fmaxf(tn2, tmin) <= fminf(tf, tmax);
    BDPT_SLAB_OCT(w, tn3, tf);
    h3 = fmaxf(tn3, tmin) <= fminf(tf, tmax);
#undef BDPT_SLAB_OCT
    if (ORD == 0) {
      // continue with the lowest hit slot, push the others
      int nx = kTravDone;
      if (h3) nx = r3;
      if (h2) { if (nx != kTravDone) stk.push(nx); nx = r2; }
      if (h1) { if (nx != kTravDone) stk.push(nx); nx = r1; }
      if (h0) { if (nx != kTravDone) stk.push(nx); nx = r0; }
      if (nx == kTravDone && !stk.pop(nx)) return kTravDone;
      return nx;
    }
    // sort key: entry distance of a hit child, +inf for a miss or an empty slot
    float k0 = h0 ? tn0 : INFINITY, k1 = h1 ? tn1 : INFINITY, k2 = h2 ? tn2 : INFINITY, k3 = h3 ? tn3 : INFINITY;
    // 5-comparator sorting network on (key, ref)
#define BDPT_CSWAP(ka, ra, kb, rb)                          \
  {                                                         \
    const bool sw = kb < ka;                                \
    const float tk = sw ? kb : ka; kb = sw ? ka : kb; ka = tk; \
    const int tr = sw ? rb : ra; rb = sw ? ra : rb; ra = tr;   \
  }
    BDPT_CSWAP(k0, r0, k1, r1);
    BDPT_CSWAP(k2, r2, k3, r3);
    BDPT_CSWAP(k0, r0, k2, r2);
    BDPT_CSWAP(k1, r1, k3, r3);
    BDPT_CSWAP(k1, r1, k2, r2);
#undef BDPT_CSWAP
    if (!(k0 < INFINITY)) {
      int nx;
      return stk.pop(nx) ? nx : kTravDone;
    }
    // the keys are sorted, so a later child is hit only if the earlier ones are: nested, a wave skips
    // the deeper pushes unless one of its lanes has that many hit children (against three flat
    // conditional pushes: north star +1.4 %, C5-shaped +1.8 %, profiles/r06z6_ab_push_nest.log)
    if (k1 < INFINITY) {
      if (k2 < INFINITY) {
        if (k3 < INFINITY) stk.push(r3);
        stk.push(r2);
      }
      stk.push(r1);
    }
    return r0;
  }
}

// Query policies of traverse(): what distinguishes a closest-hit query from an any-hit one.
//  kOrd: the child order given to node_step; kNode / kPrim: the lane-use profile slots;
//  kKey: a primitive's DFS key is needed (the non-prefetch leaf path then loads a hit sphere's);
//  bound(): the current upper end of the ray interval;
//  accept(): the step after a primitive test (ok: it passed); true ends the query.
struct ClosestQuery {
  static constexpr int kOrd = kClosestOrd, kNode = LP_CNODE, kPrim = LP_CPRIM;
  static constexpr bool kKey = true;
  Hit& h;
  BDPT_HD float bound() const { return h.t; }
  BDPT_HD bool accept(bool ok, int pi, int key, float t, float b1, float b2) {
    // t <= h.t here; an equal t replaces the hit only if it comes later in the reference's DFS
    // leaf order (the reference keeps the last of equal-t hits)
    if (ok & ((t < h.t) | (key > h.key))) {
      h.t = t; h.prim = pi; h.key = key; h.b1 = b1; h.b2 = b2;
    }
    return false;
  }
};
struct AnyQuery {
  static constexpr int kOrd = kAnyOrd, kNode = LP_ANODE, kPrim = LP_APRIM;
  static constexpr bool kKey = false;
  float tmax;
  BDPT_HD float bound() const { return tmax; }
  BDPT_HD bool accept(bool ok, int, int, float, float, float) { return ok; }
};

// The traversal of both query kinds, on [tmin, q.bound()]; true when q.accept ended the query.
// The ray set-up and the stack with its private array stay in the two entry points: built here,
// k_pt<LM 2> took 16 B more scratch per lane (every other instantiation the same or less).
template <int LM, int K, class Q>
BDPT_HD bool traverse(const SceneView& S, const RayInv& r, TravStack<K>& stk, float tmin, Q& q, Counters& c) {
  const f3 o = r.o, d = r.d;
  int ref = S.root;
  // primitive pi, its record (g0, g1, g2) already in registers
  auto test_rec = [&](int pi, bool sph, const float4 g0, const float4 g1, const float4 g2) -> bool {
    float t, b1 = 0, b2 = 0;
    bool ok;
    int key;
    if (sph) {
      c.sphs++;
      ok = sph_test(g0, o, d, tmin, q.bound(), &t);
      key = __float_as_int(g1.x);
    } else {
      c.tris++;
      ok = tri_test(g0, g1, g2, o, d, tmin, q.bound(), &t, &b1, &b2);
      key = __float_as_int(g2.y);
    }
    return q.accept(ok, pi, key, t, b1, b2);
  };
  int li = 0;
  if (LM == 3 && S.fn > 0) {
    // the flat list as one run of primitives, the next record's loads issued before this test
    float4 a0, a1, a2;
    ld_rec3<LM>(S, 0, a0, a1, a2);
    for (int pi = 0; pi < S.fn; pi++) {
      BDPT_LANE_PROF(c, Q::kPrim);
      const float4 g0 = a0, g1 = a1, g2 = a2;
      ld_rec3<LM>(S, pi + 1 < S.fn ? pi + 1 : pi, a0, a1, a2);
      if (test_rec(pi, (S.fsph >> pi) & 1u, g0, g1, g2)) return true;
    }
    return false;
  }
  float4 a0, a1, a2;
  // the primitives of leaf lf
  auto test_leaf = [&](int lf) -> bool {
    const int st = leaf_start(lf), cnt = leaf_count(lf), sm = leaf_sph_mask(lf);
    if constexpr (leaf_prefetch(LM)) {
      ld_rec3<LM>(S, st, a0, a1, a2);
    }
    for (int k = 0; k < cnt; k++) {
      BDPT_LANE_PROF(c, Q::kPrim);
      const int pi = st + k;
      if constexpr (leaf_prefetch(LM)) {
        // this record was loaded one test ahead; issue the next one's loads (if any) before testing it
        const float4 g0 = a0, g1 = a1, g2 = a2;
        if (k + 1 < cnt) ld_rec3<LM>(S, pi + 1, a0, a1, a2);
        if (test_rec(pi, (sm >> k) & 1, g0, g1, g2)) return true;
      } else {
        float t, b1 = 0, b2 = 0;
        bool ok;
        int key;
        if ((sm >> k) & 1) {
          c.sphs++;
          ok = sph_test(ld_geom<LM>(S, 3 * pi), o, d, tmin, q.bound(), &t);
          key = Q::kKey && ok ? __float_as_int(ld_geom<LM>(S, 3 * pi + 1).x) : 0;
        } else {
          c.tris++;
          const float4 g2 = ld_geom<LM>(S, 3 * pi + 2);
          ok = tri_test(ld_geom<LM>(S, 3 * pi), ld_geom<LM>(S, 3 * pi + 1), g2, o, d, tmin, q.bound(), &t, &b1, &b2);
          key = __float_as_int(g2.y);
        }
        if (q.accept(ok, pi, key, t, b1, b2)) return true;
      }
    }
    return false;
  };
  if constexpr (spec_trav(LM)) {
    // speculative while-while: a lane's first leaf is postponed and the lane goes on descending its
    // stack while other lanes still look for theirs; leaves are tested once every lane has one
    int pend = 0;
    for (;;) {
      while (ref >= 0) {
        BDPT_LANE_PROF(c, Q::kNode);
        ref = node_step<K, LM, Q::kOrd>(S, r, ref, tmin, q.bound(), stk, c);
        if ((ref < 0) & (ref != kTravDone) & (pend == 0)) {
          pend = ref;
          if (!stk.pop(ref)) ref = kTravDone;
        }
        if (wave_count((pend == 0) & (ref >= 0)) == 0) break;
      }
      while (pend != 0) {
        if (test_leaf(pend)) return true;
        pend = 0;
        if ((ref < 0) & (ref != kTravDone)) {
          pend = ref;
          if (!stk.pop(ref)) ref = kTravDone;
        }
      }
      if (ref == kTravDone) return false;
    }
  } else {
    for (;;) {
      if (LM == 3) {
        if (li >= S.nleaves) return false;
        ref = ld_lds_i(S.lleaves + li++);
      }
      while (ref >= 0) {
        BDPT_LANE_PROF(c, Q::kNode);
        ref = node_step<K, LM, Q::kOrd>(S, r, ref, tmin, q.bound(), stk, c);
      }
      if (ref == kTravDone) return false;
      if (test_leaf(ref)) return true;
      if (LM != 3 && !stk.pop(ref)) return false;
    }
  }
}

// Closest hit in [tmin, tmax]; ties in t go to the larger DFS position (reference order).
template <int LM = 0, int K = 0>
BDPT_HD bool trace_closest(const SceneView& S, f3 o, f3 d, float tmin, float tmax, Hit& h, Counters& c) {
  h.t = tmax;
  h.prim = -1;
  h.key = -1;
  h.b1 = 0; h.b2 = 0;
  c.closest++;
#if defined(BDPT_STEP_HIST) && !defined(__HIP_DEVICE_COMPILE__)
  // CPU diagnostics (tools/step_hist.py): the histogram of node steps per closest-hit query
  struct StepHist {
    const Counters& c;
    uint32_t n0;
    ~StepHist() {
      if (step_hist_nested()) return;
      const uint32_t s = (c.nodes - n0) / (uint32_t)lm_width(LM);
      step_hist()[s < 255 ? s : 255]++;
    }
  } step_hist_{c, c.nodes};
#endif
  ClosestQuery q{h};
  RayInv r = make_rayinv(o, d);
  int stack_mem[kStackMax];
  TravStack<K> stk(stack_mem, LM == 1 || LM == 2 ? lane_stack(S) : nullptr);
  traverse<LM, K>(S, r, stk, tmin, q, c);
  if (h.prim >= 0) c.hits++;
#if defined(BDPT_STEP_HIST) && !defined(__HIP_DEVICE_COMPILE__)
  // entries 512..767: node steps of the same query given its final hit distance up front (the
  // ordering-independent part); 768..1023: node steps of the queries that hit nothing (the flat
  // run takes no node steps and is left out)
  if (!step_hist_nested() && !(LM == 3 && S.fn > 0)) {
    step_hist_nested() = 1;
    Counters c2 = {};
    Hit h2;
    trace_closest<LM, K>(S, o, d, tmin, h.prim >= 0 ? h.t * 1.000001f : tmax, h2, c2);
    const uint32_t s2 = c2.nodes / (uint32_t)lm_width(LM);
    step_hist()[512 + (s2 < 255 ? s2 : 255)]++;
    if (h.prim < 0) step_hist()[768 + (s2 < 255 ? s2 : 255)]++;
    step_hist_nested() = 0;
  }
#endif
  return h.prim >= 0;
}

// Any hit in [tmin, tmax] (connection rays, bidirection.cpp:418-433).
template <int LM = 0, int K = 0>
BDPT_HD bool trace_any(const SceneView& S, f3 o, f3 d, float tmin, float tmax, Counters& c) {
  c.shadow++;
#if defined(BDPT_STEP_HIST) && !defined(__HIP_DEVICE_COMPILE__)
  struct StepHistAny {   // any-hit queries: histogram entries 256..511
    const Counters& c;
    uint32_t n0, p0;
    ~StepHistAny() {
      if (step_hist_nested()) return;
      const uint32_t s = (c.nodes - n0) / (uint32_t)lm_width(LM);
      step_hist()[256 + (s < 255 ? s : 255)]++;
      if (anyhit_log()) {
        const int e[3] = {anyhit_tag(), (int)s, (int)(c.tris + c.sphs - p0)};
        anyhit_log()->insert(anyhit_log()->end(), e, e + 3);
      }
    }
  } step_hist_{c, c.nodes, c.tris + c.sphs};
  if (ray_dump() && !step_hist_nested()) {
    const float rv[8] = {o.x, o.y, o.z, d.x, d.y, d.z, tmin, tmax};
    ray_dump()->insert(ray_dump()->end(), rv, rv + 8);
  }
#endif
  AnyQuery q{tmax};
  RayInv r = make_rayinv(o, d);
  int stack_mem[kStackMax];
  TravStack<K> stk(stack_mem, LM == 1 || LM == 2 ? lane_stack(S) : nullptr);
  return traverse<LM, K>(S, r, stk, tmin, q, c);
}

// ------------------------------------------------------------------------------------------------
// The resumable any-hit traversal (the megakernel's connection-ray flush, bdpt_megakernel.h): the
// query's state lives in a struct of the caller's, and the traversal hands the wave back at a phase
// boundary of the while-while loop (after a leaf batch) once enough lanes have ended their query for
// the caller to give them the next queued ray. A connection ray carries nothing but its ring slot,
// so a lane that ends early costs the wave one live register instead of idling until the slowest of
// the 64 rays ends (E[max of 64] is 27 node steps against a mean of 4.5 on the north star's tree).
// LM 3's flat list has no divergence to fill (round 2: -6 % on CBspheres), so it keeps trace_any.
BDPT_HD constexpr bool flush_refill(int LM) { return LM == 0 || LM == 2; }
// lanes of the wave that must have ended before the traversal returns for a refill
constexpr int kRefillIdle = 16;

template <int K>
struct AnyTrav {
  RayInv r;
  float tmax;
  int ref;    // the node / leaf to continue with; kTravDone: no query in flight (ended, or none taken yet)
  bool hit;   // of the query that ended last
  BDPT_HD bool ended() const { return ref == kTravDone; }
  BDPT_HD void start(const SceneView& S, TravStack<K>& stk, f3 o, f3 d, float tmax_) {
    r = make_rayinv(o, d);
    tmax = tmax_;
    ref = S.root;
    hit = false;
    stk.clear();
  }
};

// any-hit test of leaf lf's primitives (traverse()'s test_leaf under AnyQuery)
template <int LM>
BDPT_HD bool any_leaf(const SceneView& S, f3 o, f3 d, float tmin, float tmax, int lf, Counters& c) {
  const int st = leaf_start(lf), cnt = leaf_count(lf), sm = leaf_sph_mask(lf);
  float4 a0, a1, a2;
  if constexpr (leaf_prefetch(LM)) {
    ld_rec3<LM>(S, st, a0, a1, a2);
  }
  for (int k = 0; k < cnt; k++) {
    BDPT_LANE_PROF(c, LP_APRIM);
    const int pi = st + k;
    float4 g0, g1, g2;
    if constexpr (leaf_prefetch(LM)) {
      // this record was loaded one test ahead; issue the next one's loads (if any) before testing it
      g0 = a0; g1 = a1; g2 = a2;
      if (k + 1 < cnt) ld_rec3<LM>(S, pi + 1, a0, a1, a2);
    }
    float t, b1, b2;
    if ((sm >> k) & 1) {
      c.sphs++;
      if (!leaf_prefetch(LM)) g0 = ld_geom<LM>(S, 3 * pi);
      if (sph_test(g0, o, d, tmin, tmax, &t)) return true;
    } else {
      c.tris++;
      if (!leaf_prefetch(LM)) { g0 = ld_geom<LM>(S, 3 * pi); g1 = ld_geom<LM>(S, 3 * pi + 1); g2 = ld_geom<LM>(S, 3 * pi + 2); }
      if (tri_test(g0, g1, g2, o, d, tmin, tmax, &t, &b1, &b2)) return true;
    }
  }
  return false;
}

// Runs the wave's queries in flight (lanes with !q.ended()) on [tmin, q.tmax] in trace_any's visiting
// order, and returns at a phase boundary when every lane has ended, or, if the caller has more rays
// to hand out, when at least kRefillIdle lanes have. A lane that ended holds its answer in q.hit.
// The exit test is wave-uniform: every lane of the wave calls this together, ended ones included.
template <int LM, int K>
BDPT_HD void traverse_any_resumable(const SceneView& S, AnyTrav<K>& q, TravStack<K>& stk, float tmin, bool more,
                                    Counters& c) {
  static_assert(LM != 3, "the flat list has no resumable form");
  int ref = q.ref;
  bool hit = q.hit;
  for (;;) {
    if constexpr (spec_trav(LM)) {
      // speculative while-while, as in traverse(); no leaf is postponed across a phase boundary
      int pend = 0;
      while (ref >= 0) {
        BDPT_LANE_PROF(c, LP_ANODE);
        ref = node_step<K, LM, kAnyOrd>(S, q.r, ref, tmin, q.tmax, stk, c);
        if ((ref < 0) & (ref != kTravDone) & (pend == 0)) {
          pend = ref;
          if (!stk.pop(ref)) ref = kTravDone;
        }
        if (wave_count((pend == 0) & (ref >= 0)) == 0) break;
      }
      while (pend != 0) {
        if (any_leaf<LM>(S, q.r.o, q.r.d, tmin, q.tmax, pend, c)) {
          hit = true;
          ref = kTravDone;
          break;
        }
        pend = 0;
        if ((ref < 0) & (ref != kTravDone)) {
          pend = ref;
          if (!stk.pop(ref)) ref = kTravDone;
        }
      }
    } else {
      while (ref >= 0) {
        BDPT_LANE_PROF(c, LP_ANODE);
        ref = node_step<K, LM, kAnyOrd>(S, q.r, ref, tmin, q.tmax, stk, c);
      }
      if (ref != kTravDone) {
        if (any_leaf<LM>(S, q.r.o, q.r.d, tmin, q.tmax, ref, c)) {
          hit = true;
          ref = kTravDone;
        } else if (!stk.pop(ref)) {
          ref = kTravDone;
        }
      }
    }
    const int n_ended = wave_count(ref == kTravDone);
    if (n_ended == wave_count(true) || (more && n_ended >= kRefillIdle)) break;
  }
  q.ref = ref;
  q.hit = hit;
}

// Shading record of a closest hit: interpolated normal (triangle.cpp:80-82) or sphere normal
// (sphere.cpp:78-81), and the material.
template <int LM = 0>
BDPT_HD void shade_hit(const SceneView& S, const Hit& h, f3 o, f3 d, f3* n_out, int* mat_out) {
  float4 s0, s1, s2;
  if (LM == 3) {   // the flat list's shading records are staged in LDS with its geometry
    const float4* sh = S.lshade + 3 * h.prim;
    s0 = ld_lds4(sh); s1 = ld_lds4(sh + 1); s2 = ld_lds4(sh + 2);
  } else {
    const float4* sh = S.shade + 3 * h.prim;
    s0 = ld_glb4(sh); s1 = ld_glb4(sh + 1); s2 = ld_glb4(sh + 2);
  }
  *mat_out = __float_as_int(s2.y);
  if (__float_as_int(s2.z) != 0) {   // sphere: center in geom
    float4 g = ld_geom<LM>(S, 3 * h.prim);
    f3 p = add(o, smul(h.t, d));
    *n_out = normalize(sub(p, mk3(g.x, g.y, g.z)));
  } else {
    f3 n1 = mk3(s0.x, s0.y, s0.z), n2 = mk3(s0.w, s1.x, s1.y), n3 = mk3(s1.z, s1.w, s2.x);
    f3 n = add(add(muls(n1, 1 - h.b1 - h.b2), smul(h.b1, n2)), smul(h.b2, n3));
    *n_out = normalize(n);
  }
}

}  // namespace bdpt
