// bdpt_ldsplan.h — which copy of the scene a block stages in LDS (stage_lds_scene, bdpt_megakernel.h),
// chosen on the host from the scene alone: no context, no HIP types, so the CPU tests compile it too
// (tests/native/core_cpu.cpp). bdpt_launch.h holds the budgets and applies a plan to a launch.
#pragma once

#include <algorithm>
#include <cstddef>
#include <type_traits>

#include "bdpt_scene.h"

namespace bdpt {

// scenes up to this many primitives use the flat leaf-list traversal (LM 3)
constexpr int kFlatMaxPrims = 24;   // measured: CBspheres 488 -> 511 Msamples/s, CBspheres_lambertian +6%, CBempty -1%

struct LdsPlan {
  int lm;              // the LDS mode: 0 none, 1 the whole scene, 2 the BFS treelet, 3 the flat leaf list
  int ntop;            // LM 2: the treelet's nodes, else 0
  int n_node4;         // float4s of the tree of this mode's width
  size_t copy_bytes;   // the bytes of this mode's copy
  size_t flat_bytes;   // LM 3's copy: geometry, leaf list (padded to 16 B), shading records
  size_t full_bytes;   // LM 1's copy: the binary tree and the geometry
};

// The plan for a kernel with lds_max bytes for the copy, of which a treelet may take treelet_max:
// forced_lm (BDPT_LDS_MODE, -1 = none), else the flat list for tiny scenes, else the whole scene,
// else the treelet; a mode that does not fit or has nothing to stage falls back 3 -> 1 -> 2 -> 0.
inline LdsPlan lds_plan(const HostScene& hs, int forced_lm, size_t lds_max, size_t treelet_max) {
  LdsPlan p;
  p.full_bytes = (hs.tree(lm_width(1)).nodes.size() + hs.geom.size()) * sizeof(float);
  p.flat_bytes = 2 * hs.geom.size() * sizeof(float) + (hs.leaf_refs.size() + 3) / 4 * 16;
  const bool has_nodes = !hs.bvh2.nodes.empty();
  int lm = forced_lm >= 0 ? forced_lm
               : (hs.nprim <= kFlatMaxPrims && p.flat_bytes <= lds_max) ? 3
               : (p.full_bytes <= lds_max ? 1 : has_nodes ? 2 : 0);
  if (lm == 3 && p.flat_bytes > lds_max) lm = 1;
  if (lm == 1 && p.full_bytes > lds_max) lm = 2;
  if (lm == 2 && !has_nodes) lm = 0;
  p.lm = lm;
  p.n_node4 = (int)(hs.tree(lm_width(lm)).nodes.size() / 4);
  p.ntop = lm == 2 ? (int)std::min<size_t>((size_t)hs.tree(lm_width(2)).n_top, treelet_max / node_bytes(lm_width(2))) : 0;
  p.copy_bytes = lm == 3 ? p.flat_bytes : lm == 1 ? p.full_bytes : lm == 2 ? (size_t)p.ntop * node_bytes(lm_width(2)) : 0;
  return p;
}

// f(std::integral_constant<int, LM>) for the LDS mode lm: the kernels take it as a template argument.
template <class F>
int dispatch_lm(int lm, F&& f) {
  if (lm == 3) return f(std::integral_constant<int, 3>{});
  if (lm == 1) return f(std::integral_constant<int, 1>{});
  if (lm == 2) return f(std::integral_constant<int, 2>{});
  return f(std::integral_constant<int, 0>{});
}

}  // namespace bdpt
