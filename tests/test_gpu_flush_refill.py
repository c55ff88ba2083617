"""GPU: the connection-ray flush with refill (bdpt_megakernel.h flush_queue over
traverse_any_resumable, bdpt_bvh.h) and its later flush trigger, at the shapes where the ring's
bookkeeping can break: drains of more and of fewer than 64 rays, items of 2 + 1 samples, lists long
enough to wrap the 128-slot ring several times per sample, waves most of whose lanes own no pixel,
and the point light whose splats all land on one pixel. Every case holds the eye, light and sample
frames to the per-pixel bound of tests/_pixelbound.py against the CPU build of the same device code
(bit-equal to oracle mode 2, tests/test_core_cpu.py), and the `collect_stats` launch's closest-hit
and connection-ray counts equal to the CPU build's: no ray is lost or traced twice. LM 3 (the flat
list) keeps the 64-ray flush and runs the same checks."""
import functools
import os

import numpy as np
import pytest

import _pixelbound as PB
import bdpt_amd as B
from _util import REPO

pytestmark = pytest.mark.gpu

SEED = 5489
W, H = 64, 48


def _scene(name, w, h):
    """The scene with its own field of view on a w x h frame (PB.full_view)."""
    if name == "CBbunny":
        sc = B.load_dae(os.path.join(REPO, "scenes", "CBbunny.dae"))
        sc.width, sc.height = w, h
        return sc
    return PB.full_view(name, w, h)


@functools.lru_cache(maxsize=None)
def _ref(name, w, h, S, M, pixels=None):
    """The CPU build's frames, splat counts and ray counts, computed once per case; read-only."""
    r = PB.render_rec(_scene(name, w, h), w, h, S, M, seed=SEED, pixels=pixels)
    assert r["vmin"] >= 0, "a negative addend: the bound does not apply"
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def _gpu(sc, w, h, S, M, tiles=(), spl=0, stats=False):
    pt = B.BidirectionalPathTracer(sc, w, h, S, M, seed=SEED, samples_per_lane=spl, collect_stats=stats)
    try:
        pt.raytrace_tiles(list(tiles))
        out = {k: pt.read_frame(v).astype(np.float64)
               for k, v in (("sample", B.FRAME_SAMPLE), ("eye", B.FRAME_EYE), ("light", B.FRAME_LIGHT))}
        out["plan"] = pt.launch_plan()
        if stats:
            out["stats"] = pt.stats()
        return out
    finally:
        pt.close()


def _setenv(monkeypatch, lds):
    for k in ("BDPT_LDS_MODE", "BDPT_NTOP_MAX", "BDPT_XCD_GROUPS", "BDPT_BLOCK_MAJOR"):
        monkeypatch.delenv(k, raising=False)
    if lds is not None:
        monkeypatch.setenv("BDPT_LDS_MODE", lds)


def _case(monkeypatch, name, w, h, S, M, lds, lm, spl=0, tiles=(), pixels=None, samples=None):
    """Frames of the product kernel against the bound, then the ray counts of the STATS kernel."""
    label = f"{name} {w}x{h} s{S} m{M} lm {lm} spl {spl} tiles {list(tiles)}"
    ref = _ref(name, w, h, S, M, pixels)
    closest, shadow = int(ref["stats"][1]), int(ref["stats"][2])
    assert shadow > 0 and ref["nsplat"].sum() > 0 and (ref["eye"] > 0).any(), label
    _setenv(monkeypatch, lds)
    sc = _scene(name, w, h)
    g = _gpu(sc, w, h, S, M, tiles, spl)
    assert g["plan"]["lm"] == lm, (label, g["plan"])
    PB.check_frames(g, ref, S if samples is None else samples, M, label)
    gs = _gpu(sc, w, h, S, M, tiles, spl, stats=True)
    st = gs["stats"]
    print(f"{label}: items {g['plan']['nitems']} closest {st.closest_rays} / {closest} "
          f"connection rays {st.shadow_rays} / {shadow}, per item {shadow / max(1, g['plan']['nitems']):.1f}")
    assert (st.closest_rays, st.shadow_rays) == (closest, shadow), label
    PB.check_frames(gs, ref, S if samples is None else samples, M, label + " (stats kernel)")
    return g, ref


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2, 3])
@pytest.mark.parametrize("lds,lm", [(None, 2), ("0", 0)], ids=["lm2", "lm0"])
def test_bunny_items_of_two_and_one_samples(lds, lm, S, monkeypatch):
    """CBbunny (treelet in LDS, and the whole tree from HBM), m5, two samples per item: s1 is one
    short item, s3 an item of two samples and one of one. Some 300 rays per sample and wave: every
    item drains its ring several times, the last drain with what is left."""
    g, ref = _case(monkeypatch, "CBbunny", W, H, S, 5, lds, lm, spl=2)
    assert g["plan"]["spl"] == 2 and g["plan"]["nitems"] == 48 * -(-S // 2)
    assert ref["stats"][2] / (48 * S) > 128   # more rays per wave and sample than the ring holds


def test_gems_whole_scene_in_lds(monkeypatch):
    _case(monkeypatch, "CBgems", W, H, 2, 7, None, 1)


def test_spheres_flat_list_keeps_the_64_ray_flush(monkeypatch):
    _case(monkeypatch, "CBspheres", W, H, 2, 5, None, 3)


@pytest.mark.parametrize("lds,lm", [(None, 3), ("0", 0)], ids=["lm3", "lm0"])
def test_point_light_splats_on_one_pixel(lds, lm, monkeypatch):
    """CBempty: every sample's t = 1 splat of the point light's own vertex lands on one pixel; all 64
    lanes push it in the same step, so a drain's first round resolves dozens of them together and the
    same-target sum must cover exactly the lanes that ended in that round. Also with the tree walked
    from HBM, where the drains refill."""
    g, ref = _case(monkeypatch, "CBempty", W, H, 2, 5, lds, lm)
    n = ref["nsplat"]
    assert n.max() >= W * H * 2 and n.max() > 100 * np.partition(n.reshape(-1), -2)[-2]


@pytest.mark.parametrize("lds,lm", [(None, 3), ("0", 0)], ids=["lm3", "lm0"])
def test_long_lists_wrap_the_ring(lds, lm, monkeypatch):
    """m16 on CBspheres: well over a thousand rays per wave and sample, the ring positions pass
    slot 127 many times within one item."""
    g, ref = _case(monkeypatch, "CBspheres", 32, 24, 1, 16, lds, lm)
    assert ref["stats"][2] / g["plan"]["nitems"] > 8 * 128


# ------------------------------------------------------------------------------------------------
TILES = {"8x8": (16, 8, 8, 8), "3x5": (21, 9, 3, 5), "1x1": (30, 20, 1, 1)}


@pytest.mark.parametrize("lds,lm", [(None, 2), ("0", 0)], ids=["lm2", "lm0"])
@pytest.mark.parametrize("key", list(TILES))
def test_single_wave_tiles(key, lds, lm, monkeypatch):
    """One wave: a full 8x8 block; a 3x5 tile, whose 49 lanes outside the block never push a ray but
    take refills; one pixel, whose last drain holds fewer than 64 rays. Outside the tile the eye frame
    stays exactly 0."""
    x0, y0, w, h = TILES[key]
    px = tuple((x, y) for y in range(y0, y0 + h) for x in range(x0, x0 + w))
    samples = np.zeros((H, W), np.int64)
    samples[y0:y0 + h, x0:x0 + w] = 2
    g, ref = _case(monkeypatch, "CBbunny", W, H, 2, 5, lds, lm, tiles=[TILES[key]], pixels=px, samples=samples)
    assert g["plan"]["nitems"] == 1
    assert (g["eye"][samples == 0] == 0).all()
    if key == "1x1":
        assert 0 < ref["stats"][2] < 64


def test_tile_outside_the_frame_leaves_the_frames_zero(monkeypatch):
    _setenv(monkeypatch, None)
    g = _gpu(_scene("CBbunny", W, H), W, H, 2, 5, tiles=[(W + 8, 0, 8, 8)])
    for k in ("eye", "light", "sample"):
        assert (g[k] == 0).all()
