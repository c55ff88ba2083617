// tests/native/tree_check.cpp — TEST ONLY. Builds a HostScene (bdpt_scene.cpp) and inspects the
// device tree it emitted, in both widths, from the flattened records alone: shape figures, the
// tree's SAH cost and a validity flag (tests/test_bvh_reinsert.py). Never linked into the product.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "bdpt_scene.h"

using namespace bdpt;

namespace {

struct FBox {
  float lo[3], hi[3];
};

double area(const FBox& b) {
  const double dx = (double)b.hi[0] - b.lo[0], dy = (double)b.hi[1] - b.lo[1], dz = (double)b.hi[2] - b.lo[2];
  return 2 * (dx * dy + dy * dz + dz * dx);
}

int f2i(float f) {
  int v;
  std::memcpy(&v, &f, 4);
  return v;
}

struct Child {
  int ref;
  FBox box;
};

// the children of node k of the W-wide tree (empty slots left out)
std::vector<Child> children(const HostBvh& B, int W, int k) {
  const float* N = &B.nodes[(size_t)4 * node_f4(W) * k];
  std::vector<Child> ch;
  if (W == 2) {
    for (int s = 0; s < 2; s++) {
      Child c;
      c.ref = f2i(N[12 + s]);
      for (int a = 0; a < 3; a++) { c.box.lo[a] = N[6 * s + a]; c.box.hi[a] = N[6 * s + 3 + a]; }
      ch.push_back(c);
    }
  } else {
    for (int s = 0; s < 4; s++) {
      Child c;
      c.ref = f2i(N[24 + s]);
      if (c.ref == kTravDone) continue;
      for (int a = 0; a < 3; a++) { c.box.lo[a] = N[8 * a + s]; c.box.hi[a] = N[8 * a + 4 + s]; }
      ch.push_back(c);
    }
  }
  return ch;
}

// Walks the W-wide tree from its root: false when a child reference is out of range, a child box
// leaves its parent's box, or the leaf ranges do not cover [0, nref) exactly once. For W == 2 also
// sums the SAH cost: every inner node's area + 0.5 x count x area per leaf, over the root's area
// (the root's box is the union of its children's: no record holds it).
bool walk(const HostScene& hs, int W, double* sah) {
  const HostBvh& B = hs.tree(W);
  const int nref = (int)hs.prim_ref.size();
  const int nnodes = (int)(B.nodes.size() / ((size_t)4 * node_f4(W)));
  std::vector<int> cover(nref, 0);
  auto leaf = [&](int ref) {
    const uint32_t u = ~(uint32_t)ref;
    const int st = (int)(u >> 7), cnt = (int)(u & 7u);
    if (cnt < 1 || cnt > 4 || st + cnt > nref) return -1;
    for (int k = 0; k < cnt; k++) cover[st + k]++;
    return cnt;
  };
  bool ok = true;
  double cost = 0, root_area = 0;
  if (B.root < 0) {
    const int cnt = leaf(B.root);
    if (cnt < 0) return false;
    cost = 0.5 * cnt;
    root_area = 1;
  } else {
    if (B.root >= nnodes) return false;
    std::vector<char> seen(nnodes, 0);
    struct Item { int node; FBox box; bool bounded; };
    std::vector<Item> st{{B.root, FBox(), false}};
    while (!st.empty()) {
      const Item it = st.back();
      st.pop_back();
      if (seen[it.node]) return false;   // a node reached twice: not a tree
      seen[it.node] = 1;
      const std::vector<Child> ch = children(B, W, it.node);
      // a node has two children or more; the 4-wide root around a leaf root has the one leaf
      if (ch.size() < 2 && !(W == 4 && !it.bounded && ch.size() == 1 && ch[0].ref < 0)) return false;
      FBox un = ch[0].box;
      for (const Child& c : ch) {
        for (int a = 0; a < 3; a++) {
          un.lo[a] = std::min(un.lo[a], c.box.lo[a]);
          un.hi[a] = std::max(un.hi[a], c.box.hi[a]);
          if (!(c.box.lo[a] <= c.box.hi[a])) ok = false;
          if (it.bounded && (c.box.lo[a] < it.box.lo[a] || c.box.hi[a] > it.box.hi[a])) ok = false;
        }
      }
      if (!it.bounded) root_area = area(un);
      cost += it.bounded ? area(it.box) : area(un);
      for (const Child& c : ch) {
        if (c.ref >= 0) {
          if (c.ref >= nnodes) return false;
          st.push_back({c.ref, c.box, true});
        } else {
          const int cnt = leaf(c.ref);
          if (cnt < 0) return false;
          cost += 0.5 * cnt * area(c.box);
        }
      }
    }
  }
  for (int k = 0; k < nref; k++)
    if (cover[k] != 1) ok = false;
  if (sah) *sah = root_area > 0 ? cost / root_area : 0;
  return ok;
}

}  // namespace

// info[0..7]: binary node count, binary depth, primitive references, validity flag, wide-node levels
// of the 2-wide and of the 4-wide tree, the traversal stack entries the trees need, kStackMax.
// Returns build_host_scene's code (info is filled only for BDPT_OK).
extern "C" int tree_check(const bdpt_scene_desc* d, int* info, double* sah) {
  HostScene hs;
  std::string err;
  const int rc = build_host_scene(d, hs, err);
  if (rc != BDPT_OK) return rc;
  bool ok = walk(hs, 2, sah);
  ok = walk(hs, 4, nullptr) && ok;
  // the 4-wide tree's root is a node: its speculative traversal never ends on a leaf reference
  if (hs.nprim > 0 && hs.bvh4.root < 0) ok = false;
  std::vector<char> used(hs.nprim, 0);
  for (int32_t p : hs.prim_ref) {
    if (p < 0 || p >= hs.nprim) { ok = false; continue; }
    used[p] = 1;
  }
  for (int i = 0; i < hs.nprim; i++)
    if (!used[i]) ok = false;
  info[0] = hs.dev_nodes;
  info[1] = hs.dev_depth;
  info[2] = (int)hs.prim_ref.size();
  info[3] = ok ? 1 : 0;
  info[4] = hs.bvh2.depth;
  info[5] = hs.bvh4.depth;
  info[6] = std::max(1 * (hs.bvh2.depth + 1) + 2, 3 * (hs.bvh4.depth + 1) + 2);
  info[7] = kStackMax;
  return BDPT_OK;
}
