"""The per-pixel bound of tests/_pixelbound.py is sound and sharp (CPU): on the recorded
fp32 addends of the CPU build of the device code, every fp32 re-summation stays inside the bound,
and a single missing, misplaced or spurious addend falls outside it — where the whole-frame
RMSE < 1e-4 criterion of the GPU parity tests lets most of them pass."""
import functools

import numpy as np
import pytest

import _pixelbound as PB
from _util import MODE_C32, golden_scene, oracle_render

W, H, S, M = 16, 12, 4, 5
SEED = 77
RMSE_TOL = 1e-4   # tests/test_gpu_parity.py
SCENES = ["CBspheres", "CBempty"]   # area light with mirror + glass; point light
F32 = np.float32


@functools.lru_cache(maxsize=None)
def _ref(name):
    sc = PB.full_view(name, W, H)
    r = PB.render_rec(sc, W, H, S, M, seed=SEED, record=True)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return sc, r


def _per_pixel(rec):
    """{pixel: (k, 3) float32 addends}"""
    pix, rgb = rec
    order = np.argsort(pix, kind="stable")
    pix, rgb = pix[order], rgb[order]
    cut = np.flatnonzero(np.diff(pix)) + 1
    return {int(p[0]): a for p, a in zip(np.split(pix, cut), np.split(rgb, cut)) if len(p)}


def _images(name):
    """Per image kind: (reference (H, W, 3), n (H, W), tol (H, W, 3), {pixel: addends as the GPU adds them})."""
    _, r = _ref(name)
    ne = np.full((H, W), PB.eye_n(S, M))
    inv = F32(1.0) / F32(S)
    eye_add = {p: a * inv for p, a in _per_pixel(r["eye_addends"]).items()}   # fl(value / spp), the GPU's addend
    return {"eye": (r["eye"], ne, PB.tol_of(r["eye"], ne), eye_add),
            "light": (r["light"], r["nsplat"], PB.tol_of(r["light"], r["nsplat"]), _per_pixel(r["splats"]))}


def _sum_seq(a):
    s = np.zeros(3, F32)
    for v in a:
        s = s + v
    return s


def _sum_pairwise(a):
    a = a.copy()
    while len(a) > 1:
        if len(a) & 1:
            a = np.concatenate([a, np.zeros((1, 3), F32)])
        a = a[0::2] + a[1::2]
    return a[0]


def _sum_grouped(a):
    """groups of up to 64 summed pairwise (a wave's butterfly), the group sums then in sequence (atomics)"""
    return _sum_seq([_sum_pairwise(a[k:k + 64]) for k in range(0, len(a), 64)])


@pytest.mark.parametrize("name", SCENES)
def test_recording_export_is_the_reference(name):
    """core_cpu_render_rec renders what core_cpu_render and oracle mode 2 render, bit for bit, its
    records are complete, the per-sample eye values sum to the eye image, and no pixel holds more
    addends than the bound's n."""
    from test_core_cpu import core_render
    sc, r = _ref(name)
    eye, light, _ = core_render(sc, W, H, S, M, seed=SEED)
    assert np.array_equal(r["eye"], eye) and np.array_equal(r["light"], light)
    _, oeye, olight, _ = oracle_render(sc, W, H, S, M, MODE_C32, seed=SEED, threads=1)
    assert np.array_equal(r["eye"], oeye) and np.array_equal(r["light"], olight)
    pix, rgb = r["eye_samples"]
    assert len(pix) == W * H * S
    acc = np.zeros((H * W, 3))
    np.add.at(acc, pix, rgb.astype(np.float64))
    assert np.array_equal(acc.reshape(H, W, 3), r["eye"])
    pix, rgb = r["splats"]
    assert np.array_equal(np.bincount(pix, minlength=W * H).reshape(H, W), r["nsplat"])
    acc = np.zeros((H * W, 3))
    np.add.at(acc, pix, rgb.astype(np.float64))
    assert np.allclose(acc.reshape(H, W, 3), r["light"], rtol=1e-14, atol=0)   # fp64 sums in another order
    counts = np.bincount(r["eye_addends"][0], minlength=W * H)
    assert counts.max() <= PB.eye_n(S, M) and counts.max() > S   # several strategies per sample do contribute
    e, l = PB.lit_share(r)
    assert e > 0.5 and l > 0.5


@pytest.mark.parametrize("name", SCENES)
def test_addends_are_non_negative(name):
    _, r = _ref(name)
    for key in ("splats", "eye_addends", "eye_samples"):
        rgb = r[key][1]
        assert len(rgb) > 0 and np.isfinite(rgb).all() and (rgb >= 0).all(), key


@pytest.mark.parametrize("name", SCENES)
def test_bound_is_sound(name):
    """Every pixel's addends re-summed in fp32 — in 20 random orders, and in groups of up to 64 summed
    pairwise whose sums are then added in sequence — land within tol of the reference: the reference
    alone stays within the bound, whatever order the GPU's scheduling picks."""
    rng = np.random.default_rng(3)
    worst = {}
    for kind, (R, n, tol, adds) in _images(name).items():
        Rf, tf = R.reshape(-1, 3), tol.reshape(-1, 3)
        seen = np.zeros(W * H, bool)
        for p, a in adds.items():
            seen[p] = True
            sums = [_sum_grouped(a), _sum_seq(a)] + [_sum_seq(a[rng.permutation(len(a))]) for _ in range(20)]
            sums.append(_sum_grouped(a[rng.permutation(len(a))]))
            for s in sums:
                d = np.abs(s.astype(np.float64) - Rf[p])
                assert (d <= tf[p]).all(), (kind, p, s, Rf[p], tf[p])
                with np.errstate(divide="ignore", invalid="ignore"):
                    worst[kind] = max(worst.get(kind, 0.0), float(np.where(tf[p] > 0, d / tf[p], 0).max()))
        assert (Rf[~seen] == 0).all()   # a pixel without addends is exactly 0
    print(name, "largest |resum - R| / tol:", worst)


def _flagged(G, R, tol):
    return PB.violations(G, R, tol).any(axis=2).reshape(-1)


def _rmse(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))


def _largest(a):
    return a[np.argmax(a.astype(np.float64).sum(axis=1))].astype(np.float64)


@pytest.mark.parametrize("name", SCENES)
def test_bound_is_sharp(name):
    """One wrong addend is flagged, for every pixel with 1 <= n <= 1000 addends (a / R >= 1 / n there,
    against a tolerance of 2 (n + 2) 2^-24 R):

    * its largest addend dropped;
    * its largest splat moved to the horizontally adjacent pixel: flagged at both pixels. (The one
      exception is a move into the pixel a point light projects to, which sums W H S splats: a
      neighbour's splat of 2e-6 of that sum is under the 9e-5 that fp32 summation orders of that
      pixel differ by, so no sound bound can see it there; it is flagged at the pixel it left.)
    * a value, however small, written to a pixel whose reference is 0.

    Against RMSE_TOL = 1e-4 (one value wrong by d gives an RMSE of d / 24 on this 16x12x3 frame, d / 720
    at 480x360, d / 2494 at 1080p), measured here, CBspheres / CBempty: a pixel's largest eye addend
    dropped gives an RMSE of 2.1e-4 .. 1.8e-1 / 9.9e-4 .. 1.6e-2 (none passes on this frame; at 480x360
    the criterion admits every d < 0.072, at 1080p every d < 0.25), its largest splat dropped
    3.4e-9 .. 5.5e-3 / 6.5e-8 .. 1.6e-2, of which 49 % / 57 % pass RMSE_TOL on this very frame; a moved
    splat 4.9e-9 .. 7.8e-3 / 9.2e-8 .. 2.3e-2; the value 1e-30 in a zero pixel 4e-32, always passing.
    The bound flags every one of them."""
    rmses = {"drop": [], "move": []}
    nzero = unresolved = 0
    for kind, (R, n, tol, adds) in _images(name).items():
        npx = 0
        for p, a in adds.items():
            y, x = divmod(p, W)
            if not 1 <= len(a) <= 1000:
                continue
            npx += 1
            big = _largest(a)
            G = R.copy()
            G[y, x] -= big
            assert _flagged(G, R, tol)[p], (kind, "dropped addend not flagged", p, big, R[y, x], tol[y, x])
            assert _flagged(G, R, tol).sum() == 1
            rmses["drop"].append(_rmse(G, R))
            rmses.setdefault("drop_" + kind, []).append(_rmse(G, R))
            if kind == "light":
                x2 = x + 1 if x + 1 < W else x - 1
                G[y, x2] += big
                f = _flagged(G, R, tol)
                assert f[p]
                if (big > tol[y, x2]).any():
                    assert f[y * W + x2], ("moved splat not flagged at the receiving pixel", p, big, R[y, x2])
                else:   # under what fp32 summation of the receiving pixel can resolve: only the light's own pixel
                    assert n[y, x2] == n.max() and n[y, x2] >= W * H * S, (p, big, n[y, x2])
                    unresolved += 1
                rmses["move"].append(_rmse(G, R))
        assert npx > W * H // 2, (kind, npx)
        zero = np.argwhere(R.sum(axis=2) == 0)
        nzero += len(zero)
        for y, x in zero:
            G = R.copy()
            G[y, x, 1] = 1e-30
            assert _flagged(G, R, tol)[y * W + x]
            assert _rmse(G, R) < RMSE_TOL
    drop = np.array(rmses["drop_light"])
    for kind in ("eye", "light"):
        d = np.array(rmses["drop_" + kind])
        print(f"{name}: {kind}: dropped addend RMSE {d.min():.1e} .. {d.max():.1e}, {np.mean(d < RMSE_TOL):.2f} pass")
    print(f"{name}: RMSE of a dropped addend {drop.min():.2e} .. {drop.max():.2e}, {np.mean(drop < RMSE_TOL):.2f} "
          f"of them pass RMSE_TOL; of a moved splat {min(rmses['move']):.2e} .. {max(rmses['move']):.2e}")
    assert nzero > 0 and unresolved <= 2
    # the gap this bound closes: mutations the old criterion accepts, every one flagged above
    assert (drop < RMSE_TOL).sum() >= 10


def test_zero_reference_admits_only_zero():
    R = np.zeros((2, 2, 3))
    G = R.copy()
    assert not PB.violations(G, R, PB.tol_of(R, 5)).any()
    G[1, 0, 2] = 1e-38
    assert PB.violations(G, R, PB.tol_of(R, 5)).sum() == 1
    G[1, 0, 2] = np.nan
    assert PB.violations(G, R, PB.tol_of(R, 5)).sum() == 1


def test_the_launch_plan_facts_of_the_suite_scenes():
    """core_cpu_lds_facts on the golden scenes whose plans DESIGN.md §5 documents: CBspheres is a flat
    list (14 <= 24 primitives), CBgems' whole-scene copy is 21,760 B and leaves room for the stack slots."""
    f = PB.lds_facts(golden_scene("CBspheres", 32, 24))
    assert f["nprim"] == 14 and f["flat_n"] == 14 and f["nprim"] <= PB.FLAT_MAX_PRIMS
    g = PB.lds_facts(golden_scene("CBgems", 32, 24))
    assert g["full"] == 21760 and g["full"] + PB.LDS_STACK_BYTES <= PB.LDS_SCENE_MAX
    assert g["cap"] == 202 and g["node_bytes"] == 128


# ------------------------------------------------------------------------------------------------
# the LDS plan (csrc/bdpt_ldsplan.h lds_plan), which the launches of k_bdpt_sample, k_pt and k_features share

def _plan_is(p, f, lm, ntop=0):
    """The plan is mode lm with the copy, the tree and the byte counts that belong to it."""
    copy = {3: f["flat"], 1: f["full"], 2: ntop * f["node_bytes"], 0: 0}[lm]
    assert (p["lm"], p["ntop"], p["copy_bytes"]) == (lm, ntop, copy), p
    assert (p["flat_bytes"], p["full_bytes"]) == (f["flat"], f["full"]), p


def test_lds_plan_flat_list_and_its_fallbacks():
    """CBspheres: the flat list unforced; a forced flat list that misses the budget by a byte falls to the
    whole scene; a forced whole scene that misses it by a byte falls to the treelet."""
    sc = golden_scene("CBspheres", 32, 24)
    f = PB.lds_facts(sc)
    assert f["nprim"] <= PB.FLAT_MAX_PRIMS and f["flat"] <= PB.LDS_SCENE_MAX and f["n_top"] >= 1
    _plan_is(PB.lds_plan(sc), f, 3)
    assert PB.lds_plan(sc)["copy_bytes"] == f["flat"]
    assert f["flat"] - 1 >= f["full"]   # or the next case would fall through mode 1 as well
    _plan_is(PB.lds_plan(sc, forced_lm=3, lds_max=f["flat"] - 1), f, 1)
    tmax = PB.LDS_SCENE_MAX - PB.LDS_STACK_BYTES
    want = min(f["n_top"], tmax // f["node_bytes"])
    assert want >= 1
    _plan_is(PB.lds_plan(sc, forced_lm=1, lds_max=f["full"] - 1, treelet_max=tmax), f, 2, want)
    # a treelet budget of one node and a bit: one node
    _plan_is(PB.lds_plan(sc, forced_lm=1, lds_max=f["full"] - 1, treelet_max=2 * f["node_bytes"] - 1), f, 2, 1)


def test_lds_plan_whole_scene():
    """CBgems: too many primitives for the flat list, 21,760 B of tree and geometry: the whole scene."""
    sc = golden_scene("CBgems", 32, 24)
    f = PB.lds_facts(sc)
    assert f["nprim"] > PB.FLAT_MAX_PRIMS and f["full"] == 21760
    p = PB.lds_plan(sc)
    _plan_is(p, f, 1)
    assert p["full_bytes"] == 21760


def test_lds_plan_treelet_capped_by_its_budget():
    """The relief box of 812 triangles is larger than the budget: the treelet, of every BFS candidate
    when they fit, of treelet_max // node_bytes nodes when they do not."""
    sc = PB.box_scene(48, 36, 20, 6, area_light=True)
    f = PB.lds_facts(sc)
    assert f["full"] > PB.LDS_SCENE_MAX and f["nprim"] > PB.FLAT_MAX_PRIMS and 3 < f["n_top"] < f["cap"]
    _plan_is(PB.lds_plan(sc), f, 2, f["n_top"])
    _plan_is(PB.lds_plan(sc, treelet_max=3 * f["node_bytes"] + 5), f, 2, 3)
    _plan_is(PB.lds_plan(sc, treelet_max=0), f, 2, 0)
    # k_pt's and k_features' budget (no wave queues, no stack slots): 160 KB / 4 blocks - 256 B
    copy_only = 160 * 1024 // 4 - 256
    assert f["full"] > copy_only
    _plan_is(PB.lds_plan(sc, lds_max=copy_only, treelet_max=copy_only), f, 2, min(f["n_top"], copy_only // f["node_bytes"]))


def test_lds_plan_with_nothing_to_stage():
    """No binary nodes: a forced treelet has nothing to stage and falls to mode 0. The host scene with no
    primitives (flat and whole-scene copies of 0 bytes) is a flat list when nothing is forced, as every
    scene of <= 24 primitives whose list fits; so is a one-leaf scene, whose device tree is its root."""
    zero = {"flat": 0, "full": 0, "node_bytes": 128}
    _plan_is(PB.lds_plan(None, forced_lm=2), zero, 0)
    _plan_is(PB.lds_plan(None), zero, 3)
    _plan_is(PB.lds_plan(None, forced_lm=1), zero, 1)
    assert PB.lds_plan(None)["n_node4"] == 0
    import _rayref as R
    sc = R.scene("render1")
    f = PB.lds_facts(sc)
    assert f["nprim"] == 1
    _plan_is(PB.lds_plan(sc, forced_lm=2), f, 0)
    _plan_is(PB.lds_plan(sc), f, 3)
    _plan_is(PB.lds_plan(sc, forced_lm=0), f, 0)
