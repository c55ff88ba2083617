// bdpt_megakernel.h — k_bdpt_sample, the persistent BDPT megakernel, with its launch parameters,
// wave queue and work distribution. A header so that the kernel's flavours can be instantiated in
// more than one translation unit: bdpt_hip.hip holds flavours 0-2 (and launches all of them),
// bdpt_lens.hip the thin-lens flavour 3, compiled in parallel.

#pragma once

#include <hip/hip_runtime.h>

#include "bdpt_core.h"

namespace bdpt {

struct KParams {
  SceneView S;
  SampleParams sp;
  float* eye;        // W*H*3
  float* light;      // W*H*3
  unsigned long long* stats;  // 8 counters
  unsigned long long* prof;   // phase cycle counters (BDPT_PHASE_PROF builds only)
  const int4* blocks;         // tile blocks (x0, y0, w, h) of <= 8x8 pixels; null = full frame
  int nblocks;
  int nbx;                    // full-frame: blocks per row
  int spp_begin, spp_end, spl;
  unsigned nitems;            // work items = nblocks * ceil(spp_count / spl)
  unsigned nchunks;           // ceil(spp_count / spl)
  int block_major;            // 1: consecutive tickets walk one pixel block's chunks
  unsigned* work;             // ticket counter (zeroed before each launch)
  unsigned* work8;            // XCD mode: 8 ticket counters, 128 B apart (zeroed before each launch)
  unsigned region;            // XCD mode: items per group, ceil(nitems / 8)
  int xcd;                    // 1: blocks b, b+8, ... (one XCD) take items from their own eighth first
  int n_node4, n_geom4;       // float4 counts of the node / geometry arrays (LDS staging)
  int nmat;
  unsigned item_lo;           // first item of this launch (tickets count from it)
  int lstack_on;              // the traversal stacks' LDS overflow slots are staged (LM 1 / 2)
};

__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int ctz_mask(uint32_t m) { return __builtin_ctz(m); }
__device__ __forceinline__ int ctz_mask(uint64_t m) { return __builtin_ctzll(m); }
__device__ __forceinline__ int ctz_mask(unsigned __int128 m) {   // the m <= 126 kernels' 128-bit masks
  const uint64_t lo = (uint64_t)m;
  return lo ? __builtin_ctzll(lo) : 64 + __builtin_ctzll((uint64_t)(m >> 64));
}
// number of set bits of m below this lane (ballot + mbcnt prefix sum)
__device__ __forceinline__ int lanes_below(unsigned long long m) {
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// Wave-local ring of deferred connection rays in LDS (SoA, 128 slots per wave).
constexpr int QCAP = 128;
struct WaveQ {
  float ox[QCAP], oy[QCAP], oz[QCAP], dx[QCAP], dy[QCAP], dz[QCAP], tmax[QCAP];
  float vx[QCAP], vy[QCAP], vz[QCAP];
  int tgt[QCAP];            // >= 0: light-image pixel (t = 1 splat); < 0: ~owner lane (eye image)
  float acc[3][64];         // eye-image accumulators of the wave's 64 lanes
};

__device__ __forceinline__ float wave_sumf(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The unoccluded connection rays of the lanes with vis set: each adds its value to the owner's eye
// accumulator (LDS atomic) or splats it (global atomic).
// Splats aimed at the round's most common kind of target — the first splatting lane's pixel — are
// summed across the wave first: a point light's own vertex projects to the same pixel for every
// sample (t = 1, s = 1), and unaggregated that one address serialises ~all global atomics.
__device__ __forceinline__ void resolve_rays(WaveQ& q, bool vis, float vx, float vy, float vz, int tgt, int lane,
                                             float* light) {
  if (vis && tgt < 0) {
    const int ow = ~tgt;
    atomicAdd(&q.acc[0][ow], vx);
    atomicAdd(&q.acc[1][ow], vy);
    atomicAdd(&q.acc[2][ow], vz);
  }
  const bool splat = vis && tgt >= 0;
  const unsigned long long m = __ballot(splat);
  if (m == 0) return;
  const int lead = __builtin_ctzll(m);
  const int t0 = __shfl(tgt, lead, 64);
  const bool same = splat && tgt == t0;
  const unsigned long long ms = __ballot(same);
  if (__popcll(ms) > 1) {
    const float sx = wave_sumf(same ? vx : 0.0f), sy = wave_sumf(same ? vy : 0.0f), sz = wave_sumf(same ? vz : 0.0f);
    if (lane == lead) {
      float* p = light + 3 * (size_t)t0;
      atomicAdd(p, sx);
      atomicAdd(p + 1, sy);
      atomicAdd(p + 2, sz);
    }
  } else if (same) {
    float* p = light + 3 * (size_t)t0;
    atomicAdd(p, vx);
    atomicAdd(p + 1, vy);
    atomicAdd(p + 2, vz);
  }
  if (splat && !same) {
    float* p = light + 3 * (size_t)tgt;
    atomicAdd(p, vx);
    atomicAdd(p + 1, vy);
    atomicAdd(p + 2, vz);
  }
}

// Resolve the n queued connection rays from ring position head on.
// LM 3 (n <= 64): one ray per lane, an any-hit test each, then resolve_rays.
// With refill (flush_refill(LM), any n <= QCAP): lanes 0-63 take the first rays; whenever the
// resumable traversal hands the wave back, the lanes whose ray ended resolve it (value and target
// re-read from the ring slot) and take the next slots in lane order from a wave-uniform cursor,
// until every ray queued at the start is traced. Across the traversal a lane holds, beyond the
// traversal's own state, its slot index alone. Nothing is pushed during a flush, so a slot stays
// valid until its lane has resolved it.
template <int LM>
__device__ __forceinline__ void flush_queue(const SceneView& S, WaveQ& q, int head, int n, int lane, float* light,
                                            Counters& cnt) {
#ifdef BDPT_PHASE_PROF
  if (lane == 0) cnt.lp[2 * LP_FLUSH]++;
#endif
  if constexpr (flush_refill(LM)) {
    AnyTrav<kConnStack> st = {};
    st.ref = kTravDone;
    int stack_mem[kStackMax];
    TravStack<kConnStack> stk(stack_mem, LM == 1 || LM == 2 ? lane_stack(S) : nullptr);
    int slot = -1;   // this lane's ring slot, -1: none
    int cur = head;  // wave-uniform: the next ring position to hand out
    const int end = head + n;
    for (;;) {
      const bool want = slot < 0;
      const unsigned long long mw = __ballot(want);
      const int pos = cur + lanes_below(mw);
      if (want && pos < end) {
        slot = pos & (QCAP - 1);
        st.start(S, stk, mk3(q.ox[slot], q.oy[slot], q.oz[slot]), mk3(q.dx[slot], q.dy[slot], q.dz[slot]),
                 q.tmax[slot]);
        cnt.shadow++;
#ifdef BDPT_PHASE_PROF
        cnt.lp[2 * LP_FLUSH + 1]++;
#endif
      }
      cur = __builtin_amdgcn_readfirstlane(min(end, cur + (int)__popcll(mw)));
      if (__ballot(slot >= 0) == 0) break;
      traverse_any_resumable<LM, kConnStack>(S, st, stk, BDPT_EPS_F, cur < end, cnt);
      const bool ended = (slot >= 0) & st.ended();
      const bool vis = ended & !st.hit;
      float vx = 0, vy = 0, vz = 0;
      int tgt = -1;
      if (vis) {
        vx = q.vx[slot]; vy = q.vy[slot]; vz = q.vz[slot];
        tgt = q.tgt[slot];
      }
      resolve_rays(q, vis, vx, vy, vz, tgt, lane, light);
      if (ended) slot = -1;
    }
  } else {
    bool vis = false;
    float vx = 0, vy = 0, vz = 0;
    int tgt = -1;
#ifdef BDPT_PHASE_PROF
    if (lane < n) cnt.lp[2 * LP_FLUSH + 1]++;
#endif
    if (lane < n) {
      const int k = (head + lane) & (QCAP - 1);
      f3 o = mk3(q.ox[k], q.oy[k], q.oz[k]), d = mk3(q.dx[k], q.dy[k], q.dz[k]);
      const float tmax = q.tmax[k];
      vx = q.vx[k]; vy = q.vy[k]; vz = q.vz[k];
      tgt = q.tgt[k];
      vis = !trace_any<LM, kConnStack>(S, o, d, BDPT_EPS_F, tmax, cnt);
    }
    resolve_rays(q, vis, vx, vy, vz, tgt, lane, light);
  }
}

// k_bdpt_sample: each lane owns one pixel and a chunk of its samples. Per sample the lane builds
// both subpaths (random walks, closest-hit traversal) and then enumerates its (i, j) connections
// in the reference's order; every connection that needs a visibility ray is pushed (ballot +
// mbcnt compaction) into the wave's LDS ring, and whenever 64 are queued the whole wave traces
// them together — all 64 lanes busy on shadow rays regardless of per-lane path lengths. Where the
// any-hit traversal diverges (LM 0 / 2, flush_refill) the wave instead lets the ring fill up and
// drains it whole, lanes whose ray ends early taking the next queued one (flush_queue).
// 4 waves per SIMD = 128 VGPRs: measured best (round 1: 2: 160, 3: 220, 4: 259, 5: 151 Msamples/s;
// round 4, with 0 instead of 38-51 spilled VGPRs at 3 waves: still -13..-16% on every workload,
// profiles/r04c_ab_waves.log)
constexpr int kMinWaves = 4;
constexpr int kBlock = 256 * kMinWaves;   // one block per CU: one LDS scene copy shared by its 16 waves
constexpr int kWavesPerBlock = kBlock / 64;

// Connections: every strategy from per-lane compacted lists (connect_sample) instead of the
// wave-uniform max|E| x max|L| grid. History: the general (i, j >= 2) pairs from lists, the special
// strategies wave-uniform, paid only for m > 5 (C5-shaped 446 -> 470, CBgems m7 +0.9 %; the m5 north
// star -1.7 %). Round 5 put the special strategies on lists too (the s = 0 list holds only the
// emitter / environment vertices), and the lists now win at m5 as well: north star 721.7 -> 730.4,
// CBspheres 674 -> 684 Msamples/s, C5-shaped and CBgems m7 unchanged (profiles/r05za_ab_conn_lists.log).
// Materials and lights copied to LDS (static arrays) when they fit: per-lane material / light
// reads in the walk and in every connection become ds_reads instead of vector-memory loads.
// (measured: C2 +3%, Lucy stand-in +1%, CBgems +1%)
constexpr int kLdsMats = 48, kLdsLights = 8;
constexpr size_t kLdsStackBytes = (size_t)kLdsStack * kBlock * sizeof(int);   // LM 1 (when it fits) and 2

constexpr size_t kStaticLds = kLdsMats * sizeof(DMat) + kLdsLights * sizeof(DLight);
constexpr int kMaxDepth = 126;   // the deepest k_bdpt_sample instantiation (MAXV = 126: vertex index <= 127, 128-bit delta masks)
#define BDPT_STR2(x) #x
#define BDPT_STR(x) BDPT_STR2(x)

#ifdef BDPT_PHASE_PROF
#define PH_STAMP(v) (v) = __builtin_amdgcn_s_memtime()
#else
#define PH_STAMP(v)
#endif

// Stages the block's LDS copy of the scene at sc (LM 1: whole tree + geometry; LM 2: the BFS
// treelet; LM 3: the flat leaf list with its geometry and shading records) and points S at it.
template <int LM>
__device__ __forceinline__ void stage_lds_scene(SceneView& S, int n_node4, int n_geom4, float4* sc) {
  if (LM != 0) {
    const int nn = LM == 1 ? n_node4 : LM == 3 ? 0 : node_f4(lm_width(LM)) * S.ntop;
    const int n4 = nn + (LM == 1 || LM == 3 ? n_geom4 : 0);
    for (int k = threadIdx.x; k < n4; k += blockDim.x)
      sc[k] = k < nn ? S.nodes[k] : S.geom[k - nn];
    if (LM == 3) {
      int* lv = (int*)(sc + n4);
      for (int k = threadIdx.x; k < S.nleaves; k += blockDim.x) lv[k] = S.lleaves[k];
      S.lleaves = lv;
      float4* ls = sc + n4 + (S.nleaves + 3) / 4;   // shading records after the leaf list
      for (int k = threadIdx.x; k < n_geom4; k += blockDim.x) ls[k] = S.shade[k];
      S.lshade = ls;
    }
    __syncthreads();
    S.lnodes = sc;
    S.lgeom = sc + nn;
  }
}

// k_bdpt_sample's LDS: the scene copy behind the wave queues and the traversal stacks' overflow
// slots, and the materials / lights; points kp.S at them.
template <int LM>
__device__ __forceinline__ void stage_scene(KParams& kp, unsigned char* smem, DMat* s_mats, DLight* s_lights) {
  static_assert(kLdsStackStride == kBlock, "LDS stack stride = lanes per block");
  const bool lst = (LM == 1 || LM == 2) && kLdsStack > 0 && kp.lstack_on;
  if (lst)   // the traversal stacks' LDS overflow slots, behind the wave queues
    kp.S.lstack = (int*)(smem + kWavesPerBlock * sizeof(WaveQ));
  stage_lds_scene<LM>(kp.S, kp.n_node4, kp.n_geom4,
                      (float4*)(smem + kWavesPerBlock * sizeof(WaveQ) + (lst ? kLdsStackBytes : 0)));
  if (kp.nmat <= kLdsMats && kp.S.nlights <= kLdsLights) {
    for (int k = threadIdx.x; k < kp.nmat; k += blockDim.x) s_mats[k] = kp.S.mats[k];
    for (int k = threadIdx.x; k < kp.S.nlights; k += blockDim.x) s_lights[k] = kp.S.lights[k];
    __syncthreads();
    kp.S.mats = s_mats;
    kp.S.lights = s_lights;
  }
}

// Persistent waves: each wave takes work items (8x8 pixel block, chunk of spl samples) from a
// global ticket counter until none are left, so per-item cost differences (path lengths, scene
// regions) never leave CUs idle at the tail of the launch. Returns false at the first ticket past
// the end (every wave reaches it). XCD mode: blocks b and b + 8 share an XCD (round-robin dealing,
// MI355X_MICROARCH.md), so group g = b % 8 works through its own contiguous eighth of the items (a
// contiguous band of pixel blocks, whose BVH region then stays in that XCD's L2) and only then
// helps the other groups. Items are numbered from kp.item_lo.
struct Item {
  int x, y, s0, my_n;   // this lane's pixel and sample range [s0, s0 + my_n)
  unsigned idx;         // item index relative to kp.item_lo
};
// Pixel block blk (<= 8x8: an entry of the tile block list, or a cell of the full frame's grid) and
// the lane's pixel in it; false (and pixel 0, 0) for a lane outside the block.
__device__ __forceinline__ bool block_pixel(const int4* blocks, int nbx, int W, int H, int blk, int lane, int& x,
                                            int& y) {
  int bx0, by0, bw, bh;
  if (blocks) {
    int4 bb = blocks[blk];
    bx0 = bb.x; by0 = bb.y; bw = bb.z; bh = bb.w;
  } else {
    bx0 = (blk % nbx) * 8;
    by0 = (blk / nbx) * 8;
    bw = min(8, W - bx0);
    bh = min(8, H - by0);
  }
  const int qx = lane & 7, qy = lane >> 3;
  const bool in = qx < bw && qy < bh;
  x = in ? bx0 + qx : 0;
  y = in ? by0 + qy : 0;
  return in;
}
__device__ __forceinline__ bool next_item(const KParams& kp, int lane, int grp, int& cur, Item& it) {
  unsigned item = 0;
  if (kp.xcd) {
    item = 0xffffffffu;
    if (lane == 0) {
      for (; cur < 8; cur++) {
        const unsigned gg = (unsigned)((grp + cur) & 7);
        const unsigned lo = gg * kp.region;
        if (lo >= kp.nitems) continue;
        const unsigned t = atomicAdd(kp.work8 + 32 * gg, 1u);
        if (t < kp.region && lo + t < kp.nitems) { item = lo + t; break; }
      }
    }
    item = __shfl(item, 0, 64);
    cur = __shfl(cur, 0, 64);
    if (item == 0xffffffffu) return false;
  } else {
    if (lane == 0) item = atomicAdd(kp.work, 1u);
    item = __shfl(item, 0, 64);
    if (item >= kp.nitems) return false;
  }
  it.idx = item;
  item += kp.item_lo;
  int chunk, blk;
  if (kp.block_major) {
    blk = (int)(item / kp.nchunks);
    chunk = (int)(item - (unsigned)blk * kp.nchunks);
  } else {
    chunk = (int)(item / (unsigned)kp.nblocks);
    blk = (int)(item - (unsigned)chunk * (unsigned)kp.nblocks);
  }
  int s0 = 0, s1 = 0;
  if (block_pixel(kp.blocks, kp.nbx, kp.sp.W, kp.sp.H, blk, lane, it.x, it.y)) {
    s0 = kp.spp_begin + chunk * kp.spl;
    s1 = min(s0 + kp.spl, kp.spp_end);
  }
  it.s0 = s0;
  it.my_n = max(0, s1 - s0);
  return true;
}

// Per-wave connection state of one work item: the wave-uniform ring indices (the eye accumulators,
// direct s = 0 contributions included, live in the ring's LDS).
struct ConnState {
  int head = 0, tail = 0;
#ifdef BDPT_PHASE_PROF
  unsigned long long ph_gen = 0, ph_flush = 0;
#endif
};

// The connections of one pixel-sample (est_radiance_global_illumination's s x t loop,
// bidirection.cpp:472-500): one strategy kind at a time, each lane walking its own list of usable
// vertices, so the j == 1 (fresh light sample) and i == 1 (camera connection) bodies run once per
// iteration for all lanes instead of interleaving with the general case; every connection that
// needs a visibility ray is pushed (ballot + mbcnt compaction) into the wave's LDS ring, and
// whenever a flush is due (conn_step) the wave traces them together. PA: the path accessor (PathsInRegs over the
// lane's private Paths).
template <int LM, int EXT, bool STATS, class PA>
__device__ __forceinline__ void connect_sample(const KParams& kp, WaveQ& q, const PA& PP, Rng& g, int nE, int nL,
                                               int lane, float inv, ConnState& cs, Counters& cnt) {
#ifdef BDPT_PHASE_PROF
  const unsigned long long tg0 = __builtin_amdgcn_s_memtime();
  unsigned long long tp0, tp1;
#endif
  // one (i, j) connection per lane (active lanes only), its ray pushed into the wave's ring, the
  // ring flushed when it is due: 64 rays queued (LM 3), or no room left for the next step's pushes,
  // of which there are at most next_max (wave-uniform)
  auto conn_step = [&](int i, int j, bool active, int next_max, const Vtx* ev_pre = nullptr,
                       const Vtx* lv_pre = nullptr) {
    int kind = CONN_NONE;
    Conn cn;
    if (active) {
      BDPT_LANE_PROF(cnt, LP_CONN);
      kind = make_conn<EXT>(kp.S, kp.sp, PP, g, i, j, cn, ev_pre, lv_pre, EXT && STATS ? &cnt : nullptr);
      if (kind == CONN_DIRECT) {
        // straight into this lane's accumulator in the wave's LDS (only this wave writes it, and
        // not while a flush runs): no registers held across the walks
        q.acc[0][lane] += cn.val.x * inv;
        q.acc[1][lane] += cn.val.y * inv;
        q.acc[2][lane] += cn.val.z * inv;
      }
    }
    const bool push = kind == CONN_RAY;
    const unsigned long long m = __ballot(push);
    if (push) {
      const int slot = (cs.tail + lanes_below(m)) & (QCAP - 1);
      q.ox[slot] = cn.o.x; q.oy[slot] = cn.o.y; q.oz[slot] = cn.o.z;
      q.dx[slot] = cn.d.x; q.dy[slot] = cn.d.y; q.dz[slot] = cn.d.z;
      q.tmax[slot] = cn.tmax;
      const bool eye_t = cn.splat < 0;
      q.vx[slot] = eye_t ? cn.val.x * inv : cn.val.x;
      q.vy[slot] = eye_t ? cn.val.y * inv : cn.val.y;
      q.vz[slot] = eye_t ? cn.val.z * inv : cn.val.z;
      q.tgt[slot] = eye_t ? ~lane : cn.splat;
    }
    cs.tail += __popcll(m);
    // With refill a flush drains the ring, and the later it runs the more rays it has to fill idle
    // lanes with: only when the next step's pushes (at most next_max) could overflow the ring. The
    // test stays behind the push, so that cn is never live across a flush.
    const int queued = cs.tail - cs.head;
    if (flush_refill(LM) ? queued + next_max > QCAP : queued >= 64) {
      const int n = flush_refill(LM) ? queued : 64;
      PH_STAMP(tp0);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      flush_queue<LM>(kp.S, q, cs.head, n, lane, kp.light, cnt);
      __builtin_amdgcn_wave_barrier();
      cs.head += n;
      PH_STAMP(tp1);
#ifdef BDPT_PHASE_PROF
      cs.ph_flush += tp1 - tp0;
#endif
    }
  };
  // Per-lane lists (bit masks, built by the walk as it stores the vertices) of the vertices each
  // strategy can use: connectable eye / light vertices (cq > 0), and the eye vertices an s = 0 path
  // ends on (an emitter, or the environment in EXT kernels) — the only ones make_conn does not
  // reject at once for these strategies
  using Mask = decltype(PP.dE);   // 32 bits, or 64 for the m <= 32 / 62 kernels
  // (a lane without a sample in this step, nE = 0, still holds its previous sample's paths)
  const bool has = nE > 0;
  Mask mE = has ? PP.conn_e() : Mask(0), mL = has ? PP.conn_l() : Mask(0), m0 = has ? PP.src_e() : Mask(0);
  // The special strategies one kind at a time (each iteration runs one make_conn body for all
  // lanes), every lane walking its own list in the reference's index order, so the wave iterates
  // the longest list instead of the longest subpath: s = 0 (j = 0), the fresh light sample (j = 1:
  // the camera, i = 1, and every connectable eye vertex), light tracing to the camera (i = 1, j >= 2)
  // The next step pushes at most one ray per lane whose list is not yet empty: the loops' own ballot
  // counts them. After a list's last step any strategy may follow, a new sample's included: 64.
  auto each = [&](Mask m, int fixed, bool fixed_is_j) {
    unsigned long long left = __ballot(m != 0);
    while (left) {
      const bool act = m != 0;
      const int k = act ? ctz_mask(m) : 0;
      if (act) m &= m - 1;
      left = __ballot(m != 0);
      conn_step(fixed_is_j ? k : fixed, fixed_is_j ? fixed : k, act, left ? (int)__popcll(left) : 64);
    }
  };
  each(m0, 0, true);
  each(nL > 1 ? Mask(mE | Mask(2u)) : Mask(0), 1, true);
  each(mL, 1, false);
  // ... then the general (i >= 2, j >= 2) pairs from the same lists: a lane walks its own (i, j)
  // pairs, so the wave iterates max(pairs) times instead of max|E| x max|L| (most cells of that
  // grid are empty for most lanes)
  if (mL == 0) mE = 0;
  Mask jm = mL;
  unsigned long long left = __ballot(mE != 0);
  while (left) {
    const bool act = mE != 0;
    const int ci = act ? ctz_mask(mE) : 0, cj = act ? ctz_mask(jm) : 0;
    if (act) {
      jm &= jm - 1;
      if (jm == 0) { mE &= mE - 1; jm = mL; }
    }
    left = __ballot(mE != 0);
    conn_step(ci, cj, act, left ? (int)__popcll(left) : 64);
  }
#ifdef BDPT_PHASE_PROF
  cs.ph_gen += __builtin_amdgcn_s_memtime() - tg0;
#endif
}

// End of a work item: the queued rays are traced and every lane adds its eye-image sum once.
template <int LM>
__device__ __forceinline__ void finish_item(const KParams& kp, WaveQ& q, const Item& it, int lane, ConnState& cs,
                                            Counters& cnt) {
  if (cs.tail > cs.head) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    flush_queue<LM>(kp.S, q, cs.head, cs.tail - cs.head, lane, kp.light, cnt);
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
  if (it.my_n > 0) {
    float ax = q.acc[0][lane], ay = q.acc[1][lane], az = q.acc[2][lane];
    float* e = kp.eye + 3 * ((size_t)it.x + (size_t)it.y * kp.sp.W);
    if (ax != 0) atomicAdd(e, ax);
    if (ay != 0) atomicAdd(e + 1, ay);
    if (az != 0) atomicAdd(e + 2, az);
  }
  __builtin_amdgcn_wave_barrier();
}

// The wave's counters added to the context's statistics; N: how many of them the kernel keeps (8:
// the scene counters, k_pt; 11: with the environment-table reads, k_bdpt_sample).
template <bool STATS, int N>
__device__ __forceinline__ void flush_stats(unsigned long long* stats, int lane, unsigned nsamp, const Counters& cnt) {
  if (STATS) {
    // slots 0..7 the scene counters, 12..14 the environment-table reads (15: tickets, 16..31: phase profile)
    unsigned v[11] = {nsamp, cnt.closest, cnt.shadow, cnt.nodes, cnt.tris, cnt.sphs, cnt.hits, cnt.lnodes,
                      cnt.env_s, cnt.env_l, cnt.env_p};
#pragma unroll
    for (int k = 0; k < N; k++) {
      unsigned s = wave_sum(v[k]);
      if (lane == 0 && s) atomicAdd(stats + (k < 8 ? k : k + 4), (unsigned long long)s);
    }
  }
}

// LM (LDS mode): 0 = scene read from HBM/L2; 1 = whole BVH + geometry staged in LDS by every
// block; 2 = the top n_top BFS-ordered nodes (the part every ray traverses) staged in LDS.
// EXT, the kernel flavour: 1 = environment light and/or Russian roulette; 0 is the
// reference-only path with no trace of either in the generated code; 2 = flavour 1 plus hemisphere
// and directional lights (bdpt_params.infinite_lights, §9a), of which 0 and 1 hold no trace.
// 3 = flavour 2 plus the thin-lens camera (bdpt_params.lens_radius > 0, §9b), of which 0-2 hold no trace.
template <int MAXV, bool STATS, int LM, int EXT>
__global__ __launch_bounds__(kBlock, kMinWaves) void k_bdpt_sample(KParams kp) {
  // One dynamic LDS array: [wave queues][optional scene / treelet copy]
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ DMat s_mats[kLdsMats];
  __shared__ DLight s_lights[kLdsLights];
  stage_scene<LM>(kp, smem, s_mats, s_lights);
  WaveQ* qs = (WaveQ*)smem;
  const int lane = threadIdx.x & 63;
  WaveQ& q = qs[threadIdx.x >> 6];
  Counters cnt = {0, 0, 0, 0, 0, 0};
  unsigned nsamp = 0;
  const float inv = 1.0f / (float)kp.sp.spp;
  Paths<MAXV> P;
#ifdef BDPT_PHASE_PROF
  unsigned long long ph_prep = 0, ph_gen = 0, ph_flush = 0, tp0, tp1;
  unsigned long long ph_walk_wave = 0, ph_walk_lane = 0;   // walk iterations: wave (max) / lane sums
  unsigned long long ph_cells = 0, ph_pairs = 0;           // connection grid cells / (i, j) pairs
#endif
  const int grp = blockIdx.x & 7;
  int cur = 0;   // wave-uniform: XCD groups exhausted so far
  Item it;
  while (next_item(kp, lane, grp, cur, it)) {
    const int wave_n = wave_max(it.my_n);
    q.acc[0][lane] = 0;
    q.acc[1][lane] = 0;
    q.acc[2][lane] = 0;
    ConnState cs;
    for (int t = 0; t < wave_n; t++) {
      Rng g;
      int nE = 0, nL = 0;
      PH_STAMP(tp0);
#ifdef BDPT_PHASE_PROF
      const uint32_t c0 = cnt.closest;
#endif
      if (t < it.my_n) {
        prepare_sample<MAXV, LM, EXT>(kp.S, kp.sp, P, cnt, g, it.x, it.y, (uint32_t)(it.s0 + t));
        nE = P.nE;
        nL = P.nL;
        nsamp++;
      }
      PH_STAMP(tp1);
#ifdef BDPT_PHASE_PROF
      ph_prep += tp1 - tp0;
      const int wi = (int)(cnt.closest - c0);
      ph_walk_wave += (unsigned)wave_max(wi);
      ph_walk_lane += (unsigned)wi;
      ph_cells += (unsigned)(max(wave_max(nE) - 1, 0) * wave_max(nL));
      ph_pairs += (unsigned)(max(nE - 1, 0) * nL);
#endif
      connect_sample<LM, EXT, STATS>(kp, q, PathsInRegs<MAXV, EXT>(P), g, nE, nL, lane, inv, cs, cnt);
    }
    finish_item<LM>(kp, q, it, lane, cs, cnt);
#ifdef BDPT_PHASE_PROF
    ph_gen += cs.ph_gen;
    ph_flush += cs.ph_flush;
#endif
  }
#ifdef BDPT_PHASE_PROF
  {
    // the wave-level clocks were added by whichever lane was the lowest active one (BDPT_WAVE_CLK)
    const unsigned long long ct = wave_sum64(cnt.clk_walk_trace), cl = wave_sum64(cnt.clk_light),
                             cv = wave_sum64(cnt.clk_vertex);
    if (lane == 0) {
      atomicAdd((unsigned long long*)kp.prof + 0, ph_prep);
      atomicAdd((unsigned long long*)kp.prof + 1, ph_gen - ph_flush);
      atomicAdd((unsigned long long*)kp.prof + 2, ph_flush);
      atomicAdd((unsigned long long*)kp.prof + 3, ct);
      atomicAdd((unsigned long long*)kp.prof + 4, ph_walk_wave);
      atomicAdd((unsigned long long*)kp.prof + 6, ph_cells);
      atomicAdd((unsigned long long*)kp.prof + 8, cl);
      atomicAdd((unsigned long long*)kp.prof + 9, cv);
    }
  }
#pragma unroll
  for (int k = 0; k < 16; k++) {   // lane-use profile: prof[16 + k]
    const unsigned long long s = (unsigned long long)wave_sum(cnt.lp[k]);
    if (lane == 0 && s) atomicAdd((unsigned long long*)kp.prof + 16 + k, s);
  }
  {
    const unsigned long long wl = (unsigned long long)wave_sum((unsigned)ph_walk_lane);
    const unsigned long long wp = (unsigned long long)wave_sum((unsigned)ph_pairs);
    if (lane == 0) {
      atomicAdd((unsigned long long*)kp.prof + 5, wl);
      atomicAdd((unsigned long long*)kp.prof + 7, wp);
    }
  }
#endif
  flush_stats<STATS, 11>(kp.stats, lane, nsamp, cnt);
}

// The thin-lens flavour's instantiations live in bdpt_lens.hip: every MAXV class, STATS value and
// LDS mode, as launch_maxv dispatches them.
#define BDPT_LENS_KERNELS_LM(X, MAXV, STATS) X(MAXV, STATS, 0) X(MAXV, STATS, 1) X(MAXV, STATS, 2) X(MAXV, STATS, 3)
#define BDPT_LENS_KERNELS_MAXV(X, MAXV) BDPT_LENS_KERNELS_LM(X, MAXV, false) BDPT_LENS_KERNELS_LM(X, MAXV, true)
#ifdef BDPT_ONLY_MAXV
#define BDPT_LENS_KERNELS(X) BDPT_LENS_KERNELS_MAXV(X, BDPT_ONLY_MAXV)
#else
#define BDPT_LENS_KERNELS(X)                                                                          \
  BDPT_LENS_KERNELS_MAXV(X, 5) BDPT_LENS_KERNELS_MAXV(X, 8) BDPT_LENS_KERNELS_MAXV(X, 16)             \
  BDPT_LENS_KERNELS_MAXV(X, 32) BDPT_LENS_KERNELS_MAXV(X, 62) BDPT_LENS_KERNELS_MAXV(X, 126)
#endif
#define BDPT_LENS_KERNEL_DECL(MAXV, STATS, LM) extern template __global__ void k_bdpt_sample<MAXV, STATS, LM, 3>(KParams);
BDPT_LENS_KERNELS(BDPT_LENS_KERNEL_DECL)
#undef BDPT_LENS_KERNEL_DECL

}  // namespace bdpt
