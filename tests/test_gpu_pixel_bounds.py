"""GPU: every pixel of the eye, light and sample frames within the derived fp32-reordering bound of
tests/_pixelbound.py of the CPU build of the same device code (bit-equal to oracle mode 2,
tests/test_core_cpu.py), with no pixel allowed outside — over the launch shapes, LDS plans, staging
branches and depth classes of k_bdpt_sample that only the GPU executes (bdpt_hip.hip: next_item /
block_pixel, connect_sample, flush_queue, finish_item, stage_scene, pick_lm; bdpt_launch.h:
launch_persistent, tiles_to_blocks), each case asserting the launch plan (bdpt_debug_launch_plan) or the
scene facts that prove it ran the branch it names. k_pt, which has no atomics, is held bit-exact.
The bound's soundness and sharpness: tests/test_pixel_bounds.py (CPU)."""
import functools
import os

import numpy as np
import pytest

import _pixelbound as PB
import bdpt_amd as B
from _util import MODE_C32, REPO, oracle_pt_render

pytestmark = pytest.mark.gpu

SEED = 5489


# ------------------------------------------------------------------------------------------------
def _scene(spec, W, H):
    kind = spec[0]
    if kind == "golden":
        return PB.full_view(spec[1], W, H)
    if kind == "box":      # ("box", N, nsph[, "env" | "dir"]): the relief box under CBspheres' area light
        sc = PB.box_scene(W, H, spec[1], spec[2], area_light=True)
        if "env" in spec:
            sc = PB.with_env(sc)
        if "dir" in spec:
            sc = PB.with_directional(sc)
        return sc
    if kind == "staging":  # ("staging", nmat, nlights[, "mat" | "light"])
        return PB.staging_scene(W, H, spec[1], spec[2], alter_last_mat="mat" in spec, alter_last_light="light" in spec)
    raise KeyError(spec)


@functools.lru_cache(maxsize=None)
def _ref(spec, W, H, S, M, rr=False, pixels=None):
    """The CPU build's frames and splat counts, computed once per case and shared; read-only."""
    sc = _scene(spec, W, H)
    if "dir" in spec:
        r = PB.inf_render_rec(sc, W, H, S, M, seed=SEED, rr=rr)
        assert r["stats"][7] == 2   # the infinite-light flavour, as bdpt_create chooses
    else:
        r = PB.render_rec(sc, W, H, S, M, seed=SEED, rr=rr, pixels=pixels)
    assert r["vmin"] >= 0, "a negative addend: the bound does not apply"
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def _gpu(sc, W, H, S, M, tiles=(), ranges=None, spl=0, rr=False, inf=False):
    pt = B.BidirectionalPathTracer(sc, W, H, S, M, seed=SEED, samples_per_lane=spl, russian_roulette=rr,
                                   infinite_lights=inf)
    try:
        plans = []
        for a, b in (ranges or [(0, S)]):
            pt.raytrace_tiles(list(tiles), a, b - a)
            plans.append(pt.launch_plan())
        out = {k: pt.read_frame(v).astype(np.float64)
               for k, v in (("sample", B.FRAME_SAMPLE), ("eye", B.FRAME_EYE), ("light", B.FRAME_LIGHT))}
        out["plan"], out["plans"] = plans[-1], plans
        return out
    finally:
        pt.close()


def _lit(ref, label):
    e, l = PB.lit_share(ref)
    assert e > 0.5 and l > 0.5, f"{label}: only {e:.2f} / {l:.2f} of the pixels are lit in the eye / light reference"


def _setenv(monkeypatch, env):
    for k in ("BDPT_LDS_MODE", "BDPT_NTOP_MAX", "BDPT_XCD_GROUPS", "BDPT_BLOCK_MAJOR"):
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)


def _blocks(W, H):
    return ((W + 7) // 8) * ((H + 7) // 8)


SPHERES = ("golden", "CBspheres")
ORDERS = [None, {"BDPT_XCD_GROUPS": "1"}, {"BDPT_BLOCK_MAJOR": "0"}, {"BDPT_XCD_GROUPS": "1", "BDPT_BLOCK_MAJOR": "0"}]
ORDER_IDS = ["default", "xcd", "chunk_major", "xcd_chunk_major"]


# ------------------------------------------------------------------------------------------------
# launch shapes

def _launch_case(monkeypatch, W, H, S, spl, env, label):
    M = 5
    ref = _ref(SPHERES, W, H, S, M)
    if W * H >= 64:
        _lit(ref, label)
    else:   # a frame of a few pixels: every one of them is lit
        assert (ref["eye"].sum(axis=2) > 0).mean() > 0.5 and ref["nsplat"].sum() > 0
    _setenv(monkeypatch, env)
    g = _gpu(_scene(SPHERES, W, H), W, H, S, M, spl=spl)
    p = g["plan"]
    print(f"{label}: plan {p}")
    want_spl = spl if spl > 0 else min(S, 2)
    assert p["lm"] == 3 and p["spl"] == want_spl
    assert p["nitems"] == _blocks(W, H) * -(-S // want_spl)
    assert p["grid"] == max(1, -(-p["nitems"] // 16))   # far fewer items than co-resident waves: 16 waves per block
    PB.check_frames(g, ref, S, M, label)
    return p


@pytest.mark.parametrize("W,H", [(1, 1), (7, 5), (8, 8), (9, 17), (20, 9), (64, 48)])
def test_frames(W, H, monkeypatch):
    """Frames narrower than a pixel block (1x1, 7x5), one full block, partial last columns and rows
    (9x17), 6 blocks (20x9: fewer than the 8 XCD groups), 48 blocks; s2 m5."""
    p = _launch_case(monkeypatch, W, H, 2, 0, None, f"frame {W}x{H}")
    if (W, H) == (20, 9):
        assert p["nitems"] == 6 and p["grid"] == 1


@pytest.mark.parametrize("S,spl", [(1, 0), (3, 2), (5, 2), (5, 3), (4, 1), (2, 16)])
def test_samples_per_lane(S, spl, monkeypatch):
    """Sample chunks: one sample, a ragged last chunk (3 / 2, 5 / 2, 5 / 3), one sample per item, a
    chunk longer than the launch (16 > 2), on a 9x17 frame (partial blocks in both directions)."""
    _launch_case(monkeypatch, 9, 17, S, spl, None, f"s{S} spl {spl or 'auto'}")


@pytest.mark.parametrize("env", ORDERS, ids=ORDER_IDS)
@pytest.mark.parametrize("W,H,S", [(8, 8, 1), (20, 9, 3), (64, 48, 5)])
def test_ticket_orders(W, H, S, env, monkeypatch):
    """Block- and chunk-major order, one ticket counter and the XCD groups' eight, at one work item
    (seven groups own nothing: the `lo >= nitems` skip, and every wave but one leaves at once), at
    12 items over 6 blocks (groups 6 and 7 own nothing, blocks of other groups hand over) and at 144."""
    p = _launch_case(monkeypatch, W, H, S, 0, env, f"tickets {W}x{H} s{S} {env}")
    if (W, H) == (8, 8):
        assert p["nitems"] == 1 and p["grid"] == 1
    if (W, H) == (20, 9):
        assert p["nitems"] == 12 and -(-p["nitems"] // 8) * 6 >= p["nitems"]   # region 2: groups 6, 7 start past the end


def test_sample_ranges_accumulate():
    """Three launches over the sample ranges [0, 1), [1, 3), [3, 5) add up to the one-launch frame's
    reference (a pixel's S_p is still 5)."""
    W, H, S, M = 20, 9, 5, 5
    ref = _ref(SPHERES, W, H, S, M)
    _lit(ref, "ranges")
    g = _gpu(_scene(SPHERES, W, H), W, H, S, M, ranges=[(0, 1), (1, 3), (3, 5)])
    assert [p["nitems"] for p in g["plans"]] == [6, 6, 6] and [p["spl"] for p in g["plans"]] == [1, 2, 2]
    PB.check_frames(g, ref, S, M, "ranges 20x9 s5")


TW, TH, TS = 37, 29, 3
TILES = {
    "unaligned": [(3, 5, 11, 7)],
    "clipped": [(30, 20, 32, 32)],
    "negative_origin": [(-4, -4, 10, 10)],
    "corners": [(0, 0, 1, 1), (TW - 1, 0, 1, 1), (0, TH - 1, 1, 1), (TW - 1, TH - 1, 1, 1)],
    "far_edge_past_int32": [(8, 0, 2**31 - 1, 8)],   # x0 + w > INT32_MAX: clipped to the frame like any other
}


def _tile_pixels(tiles):
    px = []
    for x0, y0, w, h in tiles:
        px += [(x, y) for y in range(max(0, y0), min(TH, y0 + h)) for x in range(max(0, x0), min(TW, x0 + w))]
    return tuple(px)


@pytest.mark.parametrize("key", list(TILES))
def test_tiles(key):
    """Tiles on a 37x29 frame cut into pixel blocks: unaligned, clipped at the right and top edges,
    with a negative origin, 1x1 tiles at the four corners, and one whose x0 + w passes INT32_MAX. Inside the tiles the eye frame obeys
    the bound, outside it is exactly 0 (the reference is 0 there); the light frame obeys the bound
    against a CPU-build render of the same pixel list."""
    M = 5
    tiles = TILES[key]
    px = _tile_pixels(tiles)
    assert len(set(px)) == len(px)
    whole = _ref(SPHERES, TW, TH, TS, M)
    _lit(whole, "tiles")
    ref = _ref(SPHERES, TW, TH, TS, M, pixels=px)
    samples = np.zeros((TH, TW), np.int64)
    for x, y in px:
        samples[y, x] = TS
    assert np.array_equal(ref["eye"][samples > 0], whole["eye"][samples > 0])   # a pixel's eye value is its own
    assert (ref["eye"][samples == 0] == 0).all()
    g = _gpu(_scene(SPHERES, TW, TH), TW, TH, TS, M, tiles=tiles)
    nblk = sum(-(-(min(TW, x0 + w) - max(0, x0)) // 8) * -(-(min(TH, y0 + h) - max(0, y0)) // 8) for x0, y0, w, h in tiles)
    print(f"tiles {key}: plan {g['plan']}")
    assert g["plan"]["nitems"] == nblk * 2
    PB.check_frames(g, ref, samples, M, f"tiles {key}")
    assert (g["eye"][samples == 0] == 0).all()


def test_tile_outside_the_frame_is_a_no_op():
    sc = _scene(SPHERES, TW, TH)
    g = _gpu(sc, TW, TH, TS, 5, tiles=[(40, 0, 8, 8)])
    assert g["plan"]["lm"] == -1 and g["plan"]["nitems"] == -1   # nothing was launched
    for k in ("eye", "light", "sample"):
        assert (g[k] == 0).all()


# ------------------------------------------------------------------------------------------------
# the LDS-plan ladder: default mode selection (no BDPT_LDS_MODE), frame 48x36, s2, m5

LW, LH, LS = 48, 36, 2


def _ladder_case(monkeypatch, spec, M, env, label, rr=False):
    sc = _scene(spec, LW, LH)
    f = PB.lds_facts(sc, "dir" in spec)
    ref = _ref(spec, LW, LH, LS, M, rr)
    _lit(ref, label)
    _setenv(monkeypatch, env)
    g = _gpu(sc, LW, LH, LS, M, rr=rr, inf="dir" in spec)
    p = g["plan"]
    print(f"{label}: facts {f} plan lm {p['lm']} lstack_on {p['lstack_on']} ntop {p['ntop']} "
          f"lds_bytes {p['lds_bytes']} staged {p['staged']} grid {p['grid']} nitems {p['nitems']}")
    PB.check_frames(g, ref, LS, M, label)
    return f, p


def _copy_bytes(f, p):
    return {3: f["flat"], 1: f["full"], 2: p["ntop"] * f["node_bytes"], 0: 0}[p["lm"]]


def _assert_lds(f, p):
    assert p["lds_bytes"] == PB.WAVEQ_BYTES + (PB.LDS_STACK_BYTES if p["lstack_on"] else 0) + _copy_bytes(f, p)
    assert p["staged"] == 1


@pytest.mark.parametrize("nsph,lm", [(4, 3), (5, 1)])
def test_ladder_flat_list_edge(nsph, lm, monkeypatch):
    """24 primitives run the flat leaf list (LM 3), 25 the whole scene in LDS (LM 1, stack slots on)."""
    f, p = _ladder_case(monkeypatch, ("box", 2, nsph), 5, None, f"ladder nprim {20 + nsph}")
    assert f["nprim"] == 20 + nsph and (f["nprim"] <= PB.FLAT_MAX_PRIMS) == (lm == 3)
    assert p["lm"] == lm and p["lstack_on"] == (1 if lm == 1 else 0) and p["ntop"] == 0
    _assert_lds(f, p)


def test_ladder_lm1_with_stack_slots(monkeypatch):
    f, p = _ladder_case(monkeypatch, ("box", 12, 6), 5, None, "ladder grid(12)")
    assert f["full"] + PB.LDS_STACK_BYTES <= PB.LDS_SCENE_MAX and f["nprim"] > PB.FLAT_MAX_PRIMS
    assert p["lm"] == 1 and p["lstack_on"] == 1
    _assert_lds(f, p)


@pytest.mark.parametrize("spec,M,rr", [(("box", 13, 6), 5, False), (("box", 16, 6), 5, False),
                                       (("box", 13, 6, "env"), 8, True), (("box", 13, 6, "dir"), 5, False)],
                         ids=["grid13", "grid16", "grid13_env_rr_m8", "grid13_infinite_lights"])
def test_ladder_lm1_without_stack_slots(spec, M, rr, monkeypatch):
    """The whole scene in LDS with no room left for the traversal stacks' overflow slots
    (LDS_SCENE_MAX - LDS_STACK_BYTES < full <= LDS_SCENE_MAX): every stack overflow goes to scratch. Also
    under the environment + roulette kernels (m8) and the infinite-light kernels."""
    f, p = _ladder_case(monkeypatch, spec, M, None, f"ladder no slots {spec[1:]}", rr=rr)
    assert PB.LDS_SCENE_MAX - PB.LDS_STACK_BYTES < f["full"] <= PB.LDS_SCENE_MAX
    assert p["lm"] == 1 and p["lstack_on"] == 0 and p["ntop"] == 0
    _assert_lds(f, p)


@pytest.mark.parametrize("ntop_max", [None, "1"])
def test_ladder_treelet_below_the_cap(ntop_max, monkeypatch):
    """A scene too large for LDS whose whole BFS treelet fits (n_top < the budget's cap): LM 2 stages
    exactly n_top nodes; and the same scene with a one-node treelet (BDPT_NTOP_MAX=1)."""
    f, p = _ladder_case(monkeypatch, ("box", 20, 6), 5, {"BDPT_NTOP_MAX": ntop_max} if ntop_max else None,
                        f"ladder grid(20) ntop_max {ntop_max}")
    assert f["full"] > PB.LDS_SCENE_MAX and 1 < f["n_top"] < f["cap"]
    assert p["lm"] == 2 and p["lstack_on"] == 1
    assert p["ntop"] == (1 if ntop_max else f["n_top"])
    _assert_lds(f, p)


# ------------------------------------------------------------------------------------------------
# materials / lights staging

@pytest.mark.parametrize("nmat,nlights,staged", [(48, 8, 1), (49, 8, 0), (48, 9, 0)])
def test_materials_and_lights_staging(nmat, nlights, staged, monkeypatch):
    """The 25-primitive box with 48 materials and 8 lights (the static LDS arrays full to the last
    entry), and one material or one light more: the kernel then reads both from global memory. The last
    material and the last light are in use: altering either changes the CPU reference."""
    spec = ("staging", nmat, nlights)
    for what in ("mat", "light"):
        alt = _ref(spec + (what,), LW, LH, LS, 5)
        base = _ref(spec, LW, LH, LS, 5)
        assert not np.array_equal(alt["eye"], base["eye"]), f"the last {what} is not reachable"
    f, p = _ladder_case(monkeypatch, spec, 5, None, f"staging {nmat} materials {nlights} lights")
    assert (f["nprim"], f["nmat"], f["nlights"]) == (25, nmat, nlights)
    assert (nmat <= PB.LDS_MATS and nlights <= PB.LDS_LIGHTS) == bool(staged)
    assert p["lm"] == 1 and p["staged"] == staged


# ------------------------------------------------------------------------------------------------
# depth classes: the edges of the MAXV = 5 / 8 / 16 / 32 / 62 / 126 kernels

@pytest.mark.parametrize("name,M", [("CBspheres", m) for m in (0, 6, 9, 16, 17, 33, 63, 126)] +
                         [("CBgems", 9), ("CBgems", 33)])
def test_depth_class_edges(name, M, monkeypatch):
    W, H, S = 16, 12, 1
    spec = ("golden", name)
    ref = _ref(spec, W, H, S, M)
    if M > 0:
        _lit(ref, f"{name} m{M}")
    else:   # no bounce: the light image holds the light's own projection only
        _lit(_ref(spec, W, H, S, 5), f"{name} m5")
        assert (ref["eye"].sum(axis=2) > 0).mean() > 0.5 and ref["nsplat"].sum() > 0
    _setenv(monkeypatch, None)
    g = _gpu(_scene(spec, W, H), W, H, S, M)
    print(f"{name} m{M}: plan {g['plan']}")
    assert g["plan"]["lm"] == (3 if name == "CBspheres" else 1)
    PB.check_frames(g, ref, S, M, f"depth {name} m{M}")


# ------------------------------------------------------------------------------------------------
def test_same_pixel_aggregation(monkeypatch):
    """CBempty's point light projects to one pixel, and every sample's light vertex splats there
    (t = 1, s = 1): the CPU build counts at least W H S splats on it, the frame's largest count. All 64
    lanes of a wave push that connection in the same step (it is the first entry of each lane's j = 1
    list), so 64 such rays sit in consecutive ring slots and any flush holds at least 32 of them:
    flush_queue's popcount(same) > 1 branch sums them over the wave and the lead lane adds once. The
    pixel's n makes its bound loose (2 (3080 + 2) u = 3.7e-4 relative) but still rigorous."""
    W, H, S, M = 32, 24, 4, 5
    spec = ("golden", "CBempty")
    ref = _ref(spec, W, H, S, M)
    _lit(ref, "aggregation")
    n = ref["nsplat"]
    y, x = np.unravel_index(n.argmax(), n.shape)
    assert n[y, x] >= W * H * S and n[y, x] > 100 * np.partition(n.reshape(-1), -2)[-2]
    _setenv(monkeypatch, None)
    g = _gpu(_scene(spec, W, H), W, H, S, M)
    print(f"aggregation: pixel ({x}, {y}) n {n[y, x]} G {g['light'][y, x]} R {ref['light'][y, x]}")
    PB.check_frames(g, ref, S, M, "aggregation CBempty 32x24 s4")


# ------------------------------------------------------------------------------------------------
# the unidirectional PathTracer: k_pt has no atomics, every pixel is bit-exact

@functools.lru_cache(maxsize=None)
def _pt_ref(name, W, H):
    sc = B.load_dae(os.path.join(REPO, "scenes", name + ".dae"), W, H)
    img, cnt, _ = oracle_pt_render(sc, W, H, 4, 5, MODE_C32, seed=31, batch=2, tol=0.05)
    img.setflags(write=False)
    cnt.setflags(write=False)
    return sc, img, cnt


@pytest.mark.parametrize("tiled", [False, True], ids=["frame", "tiles"])
@pytest.mark.parametrize("lds", ["0", "1", "2", "3"])
@pytest.mark.parametrize("W,H", [(13, 9), (64, 48)])
@pytest.mark.parametrize("name", ["CBspheres_lambertian", "CBspheres"])
def test_pathtracer_bit_exact(name, W, H, lds, tiled, monkeypatch):
    """Image and sample counts equal to oracle mode 2, whole frame, at every LDS mode; and rendered
    as two tiles whose edge is no multiple of the 8-pixel block."""
    sc, o_img, o_cnt = _pt_ref(name, W, H)
    _setenv(monkeypatch, {"BDPT_LDS_MODE": lds})
    pt = B.PathTracer(sc, W, H, 4, 5, seed=31, samples_per_batch=2, max_tolerance=0.05)
    try:
        cut = 5 if W == 13 else 27
        pt.raytrace_tiles([(0, 0, cut, H), (cut, 0, W - cut, H)] if tiled else [])
        img = pt.read_frame(B.FRAME_SAMPLE).astype(np.float64)
        cnt = pt.read_sample_counts()
        plan = pt.launch_plan()
    finally:
        pt.close()
    assert plan["lm"] == int(lds)
    assert o_img.mean() > 0 and len(np.unique(o_cnt)) > 1   # adaptive sampling stopped some pixels early
    assert np.array_equal(cnt, o_cnt), f"{int((cnt != o_cnt).sum())} sample counts differ"
    assert np.array_equal(img, o_img), f"{int((img != o_img).any(axis=2).sum())} pixels differ"
