"""Ambient (hemisphere) and directional lights under BDPT: bdpt_params.infinite_lights, DESIGN.md
§9a. CPU: the device code compiled with g++ (tests/native/core_cpu_inf.cpp).

The reference's BDPT cannot render these lights (its light API for them prints "not ready" and
asserts, light.cpp:25-51,72-98), so the semantics are pinned against the reference's own
unidirectional PathTracer on the same scenes (tests/golden/inflights/*_pt.npz, written by
tools/make_inflights_golden.py from oracle/_ref/ref_driver -U), the way
test_env.py::test_env_bdpt_converges_to_reference_pathtracer pins the environment light.
GPU parity of the same code: tests/test_gpu_inflights.py."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import bdpt_amd as B
from _inflights import GOLD, fixture_scene, inf_render, scene_check, threads
from _util import MODE_C64, REPO, golden_scene, oracle_pt_render

ENV = os.path.join(REPO, "tests", "golden", "env")
TODAYS_TEXT = "InfiniteHemisphereLight"   # what tests/test_abi.py greps the rejection for


def _blk(a, W, H):
    return a.reshape(4, H // 4, 4, W // 4, 3).mean(axis=(1, 3))


def _with_lights(sc, lights):
    return B.Scene(sc.prim_type, sc.prim_geom, sc.prim_mat, [sc.mats[i] for i in range(sc.nmat)], lights,
                   sc.camera, sc.width, sc.height, sc.envmap)


def _synth_env():
    import sys
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from envmap import synth_envmap
    return synth_envmap(16, 8, seed=5)


def test_opt_in():
    """infinite_lights = 1 passes bdpt_create's scene checks for the ambient-lit bunny.dae and the
    directional-lit teapot.dae and selects the third kernel flavour; 0 is today's rejection with
    today's text. More than one light that an escaped ray can reach, and spot lights, stay rejected."""
    bunny = B.load_dae(os.path.join(REPO, "scenes", "bunny.dae"), 32, 24)
    teapot = B.load_dae(os.path.join(REPO, "scenes", "teapot.dae"), 32, 24)
    assert [l.type for l in bunny.lights] == [B.LIGHT_HEMISPHERE]
    assert [l.type for l in teapot.lights] == [B.LIGHT_DIRECTIONAL]
    for sc, esc in ((bunny, 0), (teapot, -1)):
        rc, msg, flavour, esc_light = scene_check(sc, True)
        assert rc == B.BDPT_OK, msg
        assert flavour == 2 and esc_light == esc
        rc, msg, _, _ = scene_check(sc, False)
        assert rc == B.BDPT_E_UNSUPPORTED and TODAYS_TEXT in msg and "use the PathTracer integrator" in msg
    # the switch does not touch scenes without these lights
    plain = golden_scene("CBspheres", 32, 24)
    assert scene_check(plain, True)[2] == 0 and scene_check(plain, True, rr=True)[2] == 1
    # an environment map plus a hemisphere light; two hemisphere lights
    bunny.set_envmap(_synth_env())
    rc, msg, _, _ = scene_check(bunny, True)
    assert rc == B.BDPT_E_UNSUPPORTED and "at most one light that an escaped ray can reach" in msg
    two = _with_lights(teapot, [bunny.lights[0], teapot.lights[0], bunny.lights[0]])
    rc, msg, _, _ = scene_check(two, True)
    assert rc == B.BDPT_E_UNSUPPORTED and "at most one light that an escaped ray can reach" in msg
    # an environment map plus directional lights is fine: the map is the escape-visible light
    teapot.set_envmap(_synth_env())
    many = _with_lights(teapot, [teapot.lights[0]] * 3)
    rc, msg, flavour, esc_light = scene_check(many, True)
    assert rc == B.BDPT_OK and flavour == 2 and esc_light == 3, msg
    # spot lights
    spot = B.Light()
    spot.type = B.LIGHT_OTHER
    for on in (False, True):
        rc, msg, _, _ = scene_check(_with_lights(plain, [plain.lights[0], spot]), on)
        assert rc == B.BDPT_E_UNSUPPORTED and "only area and point lights" in msg


def test_params_field_takes_a_reserved_slot():
    """bdpt_params keeps its layout: infinite_lights is the first of the four reserved words."""
    assert C.sizeof(B.Params) == 96
    assert B.Params.infinite_lights.offset == 80 and B.Params.reserved.offset == 84
    assert B.Params.reserved.size == 12


# Measured with this file's settings (256 spp, seed 7, the fixture's 64x48 frame and depth 12),
# roulette off / on, against the committed PathTracer images: relative deviation of the image mean
# (worst channel) and of the 4x4-block means (worst block, worst channel). Tolerance = 5 x the
# larger of the two measurements, the margin DESIGN.md §9 took for the environment light.
#   hemi: mean 0.27 % / 0.37 %, blocks 3.6 % / 3.7 %
#   dir:  mean 0.04 % / 0.09 %, blocks 1.5 % / 1.7 %
CONVERGENCE_TOL = {"hemi": (5 * 0.0037, 5 * 0.037), "dir": (5 * 0.0009, 5 * 0.017)}


@pytest.mark.parametrize("rr", [False, True])
@pytest.mark.parametrize("key", ["hemi", "dir"])
def test_bdpt_converges_to_reference_pathtracer(key, rr):
    """BDPT lit only by an ambient / a directional light (light subpaths from the emission disk,
    fresh direction samples, and for the ambient light escaped eye rays) vs the reference's own
    PathTracer on the same diffuse scene, same frame and depth. Measured (see CONVERGENCE_TOL):
    hemi mean 0.27 % / 0.37 % (roulette off / on) and blocks 3.6 % / 3.7 %; dir mean 0.04 % /
    0.09 % and blocks 1.5 % / 1.7 %; tolerances five times that."""
    g = np.load(os.path.join(GOLD, key + "_pt.npz"))
    W, H, depth = int(g["W"]), int(g["H"]), int(g["depth"])
    ref = g["image"]
    sc = fixture_scene(key, W, H)
    eye, light, st = inf_render(sc, W, H, 256, depth, seed=7, rr=rr, threads=threads())
    samp = eye + light
    assert st[7] == 2 and np.isfinite(samp).all()
    m, mr = samp.mean(axis=(0, 1)), ref.mean(axis=(0, 1))
    dm = np.abs(m / mr - 1).max()
    db = np.abs(_blk(samp, W, H) / _blk(ref, W, H) - 1).max()
    print(f"{key} rr {rr}: mean deviation {dm:.5f} block deviation {db:.5f}")
    tol_m, tol_b = CONVERGENCE_TOL[key]
    assert dm < tol_m, (m, mr)
    assert db < tol_b


@functools.lru_cache(maxsize=None)
def _pt_images():
    """The oracle's PathTracer (fp64 counter mode) on the mixed scene and on the same scene without
    its directional light (scenes/CBspheres_lambertian.dae)."""
    W, H, depth = 64, 48, 12
    mixed = fixture_scene("mixed", W, H)
    area = B.load_dae(os.path.join(REPO, "scenes", "CBspheres_lambertian.dae"), W, H)
    return tuple(oracle_pt_render(s, W, H, 512, depth, MODE_C64, seed=11, batch=64, tol=0.0)[0] for s in (mixed, area))


@pytest.mark.parametrize("rr", [False, True])
def test_mixed_lights(rr):
    """An area light and a directional light in one scene (nL = 2: the light choice's 1 / nL is in
    every strategy), BDPT against the PathTracer (oracle_pt_render, fp64 counter mode).

    The PathTracer is no yardstick for the area light's share: the reference divides an area
    light's radiance by dist^2 although its pdf is already a solid-angle one (pathtracer.cpp:147,
    DESIGN.md §10), so on scenes/CBspheres_lambertian.dae alone — no code of this feature — its mean
    is 21.5 % off BDPT's, and on the mixed scene 12.6 % (12.7 % with roulette). Both integrators are
    linear in the lights, so what is compared is each one's image minus its own image of the scene
    without the directional light (BDPT's by the reference-only kernels): the directional light's
    share in the two-light scene, which a wrong 1 / nL or light choice on either light changes.
    Measured (256 spp, seed 7, roulette off / on): mean 0.07 % / 0.06 %, 4x4 blocks 5.6 % / 6.0 %
    (the difference of two noisy images); tolerances five times the larger."""
    W, H, depth = 64, 48, 12
    ref_mixed, ref_area = _pt_images()
    mixed = fixture_scene("mixed", W, H)
    assert sorted(l.type for l in mixed.lights) == [B.LIGHT_AREA, B.LIGHT_DIRECTIONAL]
    area = B.load_dae(os.path.join(REPO, "scenes", "CBspheres_lambertian.dae"), W, H)
    e, l, st = inf_render(mixed, W, H, 256, depth, seed=7, rr=rr, threads=threads())
    ea, la, sta = inf_render(area, W, H, 256, depth, seed=7, rr=rr, threads=threads())
    assert st[7] == 2 and sta[7] == (1 if rr else 0)
    d, dref = (e + l) - (ea + la), ref_mixed - ref_area
    assert np.isfinite(d).all()
    m, mr = d.mean(axis=(0, 1)), dref.mean(axis=(0, 1))
    dm = np.abs(m / mr - 1).max()
    db = np.abs(_blk(d, W, H) / _blk(dref, W, H) - 1).max()
    lit = np.abs((e + l).mean(axis=(0, 1)) / ref_mixed.mean(axis=(0, 1)) - 1).max()
    print(f"mixed rr {rr}: share mean deviation {dm:.5f} block deviation {db:.5f}; whole image vs PathTracer {lit:.4f}")
    assert dm < 5 * 0.0007, (m, mr)
    assert db < 5 * 0.060


def test_switch_off_is_bit_identical():
    """Scenes without these lights: the new entry point, switch off and on, returns core_cpu_render's
    frames bit for bit (CBspheres: the reference-only kernels; the environment-map scene of
    test_env.py and roulette: flavour 1)."""
    from test_core_cpu import core_render
    W, H, S, M = 32, 24, 2, 5
    env = golden_scene("CBspheres_lambertian", W, H)
    env.set_envmap(B.load_exr(os.path.join(ENV, "sky_32x16_zip_half.exr")))
    for sc, rr, flavour in ((golden_scene("CBspheres", W, H), False, 0), (env, False, 1), (env, True, 1)):
        eye, light, _ = core_render(sc, W, H, S, M, seed=99, rr=rr)
        for on in (False, True):
            e, l, st = inf_render(sc, W, H, S, M, seed=99, rr=rr, infinite_lights=on, threads=1)
            assert st[7] == flavour
            assert np.array_equal(e, eye) and np.array_equal(l, light)


def test_directional_never_hit():
    """A scene lit only by a directional light, with a mirror sphere, at m = 5: no eye subpath ends
    on the light, so not one s = 0 strategy returns a value (the native entry point counts them),
    and the image is finite and lit."""
    W, H = 32, 24
    sc = fixture_scene("dir", W, H)
    mirror = B.Material()
    mirror.type = B.MAT_MIRROR
    mirror.a[:] = [0.9, 0.9, 0.9]
    mats = [sc.mats[i] for i in range(sc.nmat)] + [mirror]
    pm = sc.prim_mat.copy()
    sph = np.flatnonzero(sc.prim_type == B.PRIM_SPHERE)
    assert len(sph) == 2
    pm[sph[0]] = len(mats) - 1
    sc = B.Scene(sc.prim_type, sc.prim_geom, pm, mats, [sc.lights[0]], sc.camera, W, H)
    eye, light, st = inf_render(sc, W, H, 16, 5, seed=3, threads=threads())
    assert st[7] == 2
    assert st[8] == 0 and st[9] == 0.0
    assert np.isfinite(eye).all() and np.isfinite(light).all()
    assert eye.mean() > 0.01 and light.mean() > 0
    # the ambient light, for contrast, is reached by escaped rays
    _, _, sth = inf_render(fixture_scene("hemi", W, H), W, H, 4, 5, seed=3, threads=threads())
    assert sth[8] > 0 and sth[9] > 0
