"""GPU: k_features (bdpt_denoise.hip) against the host build of the same device code
(tests/native/core_cpu_denoise.cpp). Bit-equal: k_pt's frames already are, through the same
trace_closest / shade_hit, so a difference is a finding, not a tolerance. And the isolation of the
new passes from the beauty render's frames, counts, stats and launch plan."""
import ctypes as C
import os

import numpy as np
import pytest

import bdpt_amd as B
import _denoise as D
from _util import REPO, golden_scene

pytestmark = pytest.mark.gpu
SEED = 5489


def scene_of(name):
    if name == "CBbunny":
        return B.load_dae(os.path.join(REPO, "scenes", "CBbunny.dae"))
    return golden_scene(name)   # the file's own field of view: spheres, mirror and glass in frame


def gpu_features(sc, W, H, spp, feature_spp=0, pt=False, lens=0.0, tiles=()):
    if pt:
        r = B.PathTracer(sc, W, H, spp, 5, seed=SEED, lens_radius=lens)
    else:
        r = B.BidirectionalPathTracer(sc, W, H, spp, 5, seed=SEED, lens_radius=lens)
    try:
        r.render_features(tiles, feature_spp)
        return r.read_features_raw()
    finally:
        r.close()


@pytest.mark.parametrize("name,W,H,spp", [("CBspheres", 37, 21, 1), ("CBspheres", 37, 21, 5), ("CBbunny", 40, 30, 2),
                                          ("CBspheres", 8, 8, 2), ("CBspheres", 5, 3, 2)])
def test_features_bit_equal_to_host_build(name, W, H, spp):
    sc = scene_of(name)
    got = gpu_features(sc, W, H, spp)
    want = D.host_features(sc, W, H, spp, SEED)
    assert got[..., 7].max() > 0
    assert np.array_equal(got, want)


@pytest.mark.parametrize("lds", [0, 1, 2])
def test_features_in_every_lds_mode(lds, monkeypatch):
    """CBspheres takes the flat list (mode 3) by itself; BDPT_LDS_MODE forces the others."""
    monkeypatch.setenv("BDPT_LDS_MODE", str(lds))
    sc = scene_of("CBspheres")
    assert np.array_equal(gpu_features(sc, 37, 21, 3), D.host_features(sc, 37, 21, 3, SEED, lds_mode=lds))


def test_features_of_a_lens_context():
    sc = scene_of("CBspheres")
    got = gpu_features(sc, 37, 21, 3, lens=0.25)
    assert np.array_equal(got, D.host_features(sc, 37, 21, 3, SEED, lens_radius=0.25))
    assert not np.array_equal(got, D.host_features(sc, 37, 21, 3, SEED))


def test_features_of_a_pathtracer_context_with_microfacet():
    """The microfacet albedo (Fresnel at normal incidence) uses no transcendental: bit-equal."""
    sc = scene_of("CBspheres_microfacet_al_ag")
    got = gpu_features(sc, 37, 21, 3, pt=True, lens=0.05)
    assert np.array_equal(got, D.host_features(sc, 37, 21, 3, SEED, pt=True, lens_radius=0.05))


def test_feature_spp_below_the_context_s():
    sc = scene_of("CBspheres")
    assert np.array_equal(gpu_features(sc, 37, 21, 5, feature_spp=2), D.host_features(sc, 37, 21, 2, SEED))
    r = B.BidirectionalPathTracer(sc, 37, 21, 5, 5, seed=SEED)
    try:
        assert r.lib.bdpt_render_features(r.ctx, None, 0, 6) == B.BDPT_E_INVALID
        assert b"spp" in r.lib.bdpt_last_error()
        assert r.lib.bdpt_render_features(r.ctx, None, 0, -1) == B.BDPT_E_INVALID
        out = np.zeros((21, 37, 8), np.float32)
        assert r.lib.bdpt_read_features(r.ctx, out.ctypes.data_as(C.POINTER(C.c_float))) == B.BDPT_E_INVALID
        assert b"feature pass" in r.lib.bdpt_last_error()
        assert r.lib.bdpt_denoise(r.ctx, B.FRAME_SAMPLE, None) == B.BDPT_E_INVALID
        assert b"feature pass" in r.lib.bdpt_last_error()
        assert r.lib.bdpt_denoise(r.ctx, 3, None) == B.BDPT_E_INVALID
    finally:
        r.close()


def test_tiles_unaligned_clipped_and_off_frame():
    """One unaligned tile, one clipped at the frame's edge, one fully off the frame: the tiles'
    pixels get their records, every other pixel keeps its previous one (here: a spp-1 pass's)."""
    W, H = 37, 21
    sc = scene_of("CBspheres")
    tiles = [(3, 2, 13, 9), (30, 15, 20, 20), (40, 0, 8, 8), (-5, -5, 3, 3)]
    r = B.BidirectionalPathTracer(sc, W, H, 3, 5, seed=SEED)
    try:
        r.render_features((), 1)
        before = r.read_features_raw()
        r.render_features(tiles, 3)
        got = r.read_features_raw()
        r.clear()
        assert not r.read_features_raw().any()
    finally:
        r.close()
    inside = np.zeros((H, W), bool)
    inside[2:11, 3:16] = True
    inside[15:21, 30:37] = True
    full = D.host_features(sc, W, H, 3, SEED)
    assert np.array_equal(before, D.host_features(sc, W, H, 1, SEED))
    assert np.array_equal(got[inside], full[inside])
    assert np.array_equal(got[~inside], before[~inside])
    assert not np.array_equal(full[~inside], before[~inside])


@pytest.mark.parametrize("pt", [False, True])
def test_feature_pass_and_filter_leave_the_beauty_alone(pt):
    """Beauty, then the feature pass and the filter: the eye, light and sample frames, the sample
    counts, bdpt_stats and the launch plan are bit-identical to what the context held when it had
    run the beauty alone (one context, read before and after: the light image's atomics make two
    BDPT renders differ in their last bits, which is not what this is about)."""
    W, H, S = 40, 30, 4
    sc = scene_of("CBspheres")
    if pt:
        r = B.PathTracer(sc, W, H, S, 5, seed=SEED, samples_per_batch=2, collect_stats=True)
    else:
        r = B.BidirectionalPathTracer(sc, W, H, S, 5, seed=SEED, collect_stats=True)

    def state():
        st = r.stats()
        return ([r.read_frame(k) for k in (B.FRAME_EYE, B.FRAME_LIGHT, B.FRAME_SAMPLE)], r.read_sample_counts(),
                [getattr(st, f) for f, _ in B.Stats._fields_], r.launch_plan())

    try:
        r.raytrace_tiles()
        fa, ca, sa, pa = state()
        assert sa[0] > 0 and pa["lm"] >= 0
        r.render_features()
        out = r.denoise()
        r.render_features([(1, 1, 9, 9)], 2)
        r.denoise(B.FRAME_EYE, levels=2)
        fb, cb, sb, pb = state()
    finally:
        r.close()
    assert np.isfinite(out).all() and not np.array_equal(out, fa[2])
    assert all(np.array_equal(x, y) for x, y in zip(fa, fb))
    assert np.array_equal(ca, cb)
    assert sa == sb
    assert pa == pb
