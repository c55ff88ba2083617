"""Depth of field under BDPT: the thin-lens kernels (k_bdpt_sample's flavour 3,
bdpt_params.lens_radius > 0). CPU: the device code compiled with g++
(tests/native/core_cpu_lens.cpp).

The reference's BDPT is pinhole only (its thin lens is commented out, bidirection.cpp:525-526), so
the semantics are pinned against the reference's own unidirectional PathTracer with its lens on the
same scenes (tests/golden/lens/*_lens_pt.npz, written by tools/make_lens_golden.py from
oracle/_ref/ref_driver -U -b 0.5 -d 2.5), the way tests/test_inflights.py pins the infinite lights.
GPU parity of the same code: tests/test_gpu_lens.py."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import bdpt_amd as B
from _inflights import fixture_scene, inf_render, threads
from _lens import FOCAL, GOLD, LENS, camera_samples, eye_rays, flavour, lens_render
from _util import REPO, golden_scene
from test_output_stage import CLI


def _blk(a, W, H):
    return a.reshape(4, H // 4, 4, W // 4, 3).mean(axis=(1, 3))


def _deviation(samp, ref, W, H):
    """test_inflights.py's measures: relative deviation of the image mean (worst channel) and of the
    4x4-block means (worst block, worst channel)"""
    dm = np.abs(samp.mean(axis=(0, 1)) / ref.mean(axis=(0, 1)) - 1).max()
    db = np.abs(_blk(samp, W, H) / _blk(ref, W, H) - 1).max()
    return dm, db


def _gold(key):
    g = np.load(os.path.join(GOLD, key + "_lens_pt.npz"))
    assert float(g["lens"]) == LENS and float(g["focal"]) == FOCAL
    return g["image"], int(g["W"]), int(g["H"]), int(g["depth"])


# Measured with this file's settings (256 spp, seed 7, the fixture's 64x48 frame and depth 12, lens
# radius 0.5, focal distance 2.5), roulette off / on, against the committed PathTracer lens images:
# relative deviation of the image mean (worst channel) and of the 4x4-block means (worst block,
# worst channel). Tolerance = 5 x the larger of the two measurements (DESIGN.md §9's margin).
#   hemi: mean 0.03 % / 0.09 %, blocks 1.91 % / 1.87 %
#   dir:  mean 0.44 % / 0.50 %, blocks 1.17 % / 1.20 %
# The mean tolerances (0.45 % and 2.5 %) stay below a third of the lens' own effect on the
# PathTracer's image mean (+14.3 % hemi, +9.5 % dir: 4.8 % and 3.2 %), so the test tells the lens from
# the pinhole; the pinhole BDPT image misses the fixtures by 13.5 % / 30 % (hemi) and 9.2 % / 92 % (dir).
# The light image (t = 1: the camera connection through a fresh lens point) carries 0.63 % of the
# image mean on hemi and 1.43 % on dir. On dir that is less than the mean tolerance: this test alone
# would not notice a missing t = 1 there; test_pinhole_limit (both frames per pixel) and
# test_round_trip (the camera sampler against the ray generator) carry that coverage.
CONVERGENCE_TOL = {"hemi": (5 * 0.0009, 5 * 0.0191), "dir": (5 * 0.0050, 5 * 0.0120)}
LENS_EFFECT_THIRD = {"hemi": 0.048, "dir": 0.032}


@functools.lru_cache(maxsize=None)
def _lens_image(key, rr):
    _, W, H, depth = _gold(key)
    eye, light, st = lens_render(fixture_scene(key, W, H), W, H, 256, depth, seed=7, rr=rr, threads=threads())
    assert st[7] == 3
    return eye, light


@pytest.mark.parametrize("rr", [False, True])
@pytest.mark.parametrize("key", ["hemi", "dir"])
def test_lens_bdpt_converges_to_reference_pathtracer(key, rr):
    """BDPT with the thin lens vs the reference's PathTracer with its lens, same scene, frame, depth,
    lens radius and focal distance. Measured (roulette off / on): hemi mean 0.03 % / 0.09 %, blocks
    1.91 % / 1.87 %; dir mean 0.44 % / 0.50 %, blocks 1.17 % / 1.20 %; tolerances five times the larger
    of each pair (CONVERGENCE_TOL). The light image carries 0.63 % (hemi) and 1.43 % (dir) of the mean."""
    ref, W, H, _ = _gold(key)
    eye, light = _lens_image(key, rr)
    samp = eye + light
    assert np.isfinite(samp).all()
    dm, db = _deviation(samp, ref, W, H)
    share = light.mean() / samp.mean()
    print(f"{key} rr {rr}: mean deviation {dm:.5f} block deviation {db:.5f} light-image share {share:.5f}")
    tol_m, tol_b = CONVERGENCE_TOL[key]
    assert tol_m < LENS_EFFECT_THIRD[key]
    assert dm < tol_m
    assert db < tol_b


@pytest.mark.parametrize("key", ["hemi", "dir"])
def test_pinhole_misses_the_lens_fixture(key):
    """Control: the pinhole BDPT image of the same scene, same settings, misses the lens fixture by
    more than the tolerances of the convergence test: the fixture discriminates."""
    ref, W, H, depth = _gold(key)
    eye, light, st = inf_render(fixture_scene(key, W, H), W, H, 256, depth, seed=7, threads=threads())
    assert st[7] == 2
    dm, db = _deviation(eye + light, ref, W, H)
    print(f"{key} pinhole vs lens fixture: mean deviation {dm:.5f} block deviation {db:.5f}")
    tol_m, tol_b = CONVERGENCE_TOL[key]
    assert dm > tol_m
    assert db > tol_b


@pytest.mark.parametrize("key", ["hemi", "dir", "mixed"])
def test_pinhole_limit(key):
    """lens_radius = 1e-7, focal_distance = 4.7 through flavour 3 against the pinhole through flavour
    2, same seed: both frames agree per pixel. Holds only if the lens draws live in sub-streams of
    their own (every other draw is the pinhole kernels') and every lens formula reduces to the
    pinhole's."""
    W, H, S, M = 32, 24, 4, 5
    sc = fixture_scene(key, W, H)
    e3, l3, st3 = lens_render(sc, W, H, S, M, seed=5489, lens_radius=1e-7, focal_distance=4.7)
    e2, l2, st2 = lens_render(sc, W, H, S, M, seed=5489, lens_radius=0.0)
    assert st3[7] == 3 and st2[7] == 2
    re_, rl = np.sqrt(np.mean((e3 - e2) ** 2)), np.sqrt(np.mean((l3 - l2) ** 2))
    print(f"{key}: pinhole-limit rmse eye {re_:.3e} light {rl:.3e}; means {e2.mean():.5f} {l2.mean():.3e}")
    assert e2.mean() > 0
    assert re_ < 1e-4 and rl < 1e-4


@pytest.mark.parametrize("focal", [1.0, 2.5, 4.7])
def test_round_trip(focal):
    """A lens point, a raster position and a distance t: the eye ray's point at t, given to the camera
    sampler with the same lens point, comes back as the same integer pixel with e.pos equal to the
    ray origin. 300 random cases per focal distance."""
    W, H, N = 64, 48, 300
    sc = fixture_scene("hemi", W, H)
    rng = np.random.default_rng(int(focal * 10))
    u = rng.random((N, 2)).astype(np.float32)
    pix = np.stack([rng.integers(0, W, N), rng.integers(0, H, N)], axis=1)
    # raster positions away from the pixel borders: fp32 rounding of the two directions must not
    # decide the pixel
    frac = 0.1 + 0.8 * rng.random((N, 2))
    xy = ((pix + frac) / np.array([W, H])).astype(np.float32)
    t = (0.5 + 9.5 * rng.random(N)).astype(np.float32)
    o, d = eye_rays(sc, LENS, focal, u, xy)
    assert np.allclose(np.linalg.norm(d, axis=1), 1.0, atol=1e-5)
    p = o + d * t[:, None]
    got, pos = camera_samples(sc, LENS, focal, W, H, u, p)
    assert np.array_equal(got, pix)
    assert np.array_equal(pos, o)
    # the lens points spread over the disk of radius LENS around the camera position
    cam = np.array(list(sc.desc().camera.pos))
    r = np.linalg.norm(o - cam, axis=1)
    assert r.max() <= LENS * (1 + 1e-5) and r.max() > 0.9 * LENS and np.allclose(r, LENS * np.sqrt(u[:, 0]), atol=1e-5)


def test_switch_off_is_bit_identical():
    """lens_radius = 0: the flavour is the one bdpt_create chose before the lens existed, and the
    frames are today's entry points' bit for bit (CBspheres: the reference-only kernels; hemi and
    mixed: flavour 2). bdpt_params keeps its layout."""
    from test_core_cpu import core_render
    W, H, S, M = 32, 24, 2, 5
    plain = golden_scene("CBspheres", W, H)
    assert flavour(plain, False, False, 0.0) == 0 and flavour(plain, False, True, 0.0) == 1
    assert flavour(plain, False, False, -1.0) == 0
    assert flavour(plain, False, False, LENS) == 3 and flavour(plain, True, True, LENS) == 3
    eye, light, _ = core_render(plain, W, H, S, M, seed=99)
    e, l, st = lens_render(plain, W, H, S, M, seed=99, lens_radius=0.0, infinite_lights=False)
    assert st[7] == 0 and np.array_equal(e, eye) and np.array_equal(l, light)
    for key in ("hemi", "mixed"):
        sc = fixture_scene(key, W, H)
        assert flavour(sc, True, False, 0.0) == 2 and flavour(sc, True, False, LENS) == 3
        eye, light, _ = inf_render(sc, W, H, S, M, seed=99, threads=1)
        e, l, st = lens_render(sc, W, H, S, M, seed=99, lens_radius=0.0, threads=1)
        assert st[7] == 2 and np.array_equal(e, eye) and np.array_equal(l, light)
    assert C.sizeof(B.Params) == 96
    assert B.Params.lens_radius.offset == 64 and B.Params.focal_distance.offset == 72
    assert B.Params.infinite_lights.offset == 80
    import inspect
    sig = inspect.signature(B.BidirectionalPathTracer.__init__).parameters
    assert sig["lens_radius"].default == 0.0 and sig["focal_distance"].default == 4.7


def test_cli_lens_needs_the_flag(tmp_path):
    """Without --thin-lens, -b 0.5 -d 2.5 parse as they always did and BDPT stays the pinhole; with
    it they select the lens; under --pt the flag changes nothing. (The CLI reports its camera before
    it creates the device context, so this runs without a GPU; the render itself is
    tests/test_gpu_lens.py's.)"""
    dae = os.path.join(REPO, "scenes", "CBspheres.dae")
    base = ["-s", "1", "-m", "1", "-r", "16", "12", "-b", "0.5", "-d", "2.5", "-f", str(tmp_path / "o.png"), dae]

    def run(extra):
        return subprocess.run([CLI] + extra + base, capture_output=True, text=True, timeout=300).stderr

    err = run([])
    assert "BDPT camera: pinhole" in err and "thin lens" not in err
    err = run(["--thin-lens"])
    assert "BDPT camera: thin lens, radius 0.5, focal distance 2.5" in err
    assert "BDPT camera" not in run(["--pt", "--thin-lens"])
    usage = subprocess.run([CLI, "-h"], capture_output=True, text=True).stdout
    assert "--thin-lens" in usage
