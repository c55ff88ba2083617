"""The first-hit feature pass on the host build of csrc/bdpt_features.h: its primary
rays traced by an independent route (the oracle's fp32 BVH), the albedo table, the normals against a
float64 interpolation, the per-pixel accumulation, and the identity of its primary rays with the
integrators' own. No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import bdpt_amd as B
import _denoise as D
import _rayref
from _util import REPO, golden_scene

W, H = 24, 18
SEED = 5489


def scene_of(name):
    """The scene with its file's own field of view (a camera retargeted to a frame this small would
    see the back wall alone): the frame size is the render's."""
    if name == "grid":
        sc = _rayref.scene("grid")
        sc.camera = dict(golden_scene("CBempty").camera)
        return sc
    if name == "CBbunny":
        return B.load_dae(os.path.join(REPO, "scenes", "CBbunny.dae"))
    return golden_scene(name)


def diffuse_copy(sc):
    """The scene's geometry with one diffuse material: what the oracle's ray queries accept where
    the scene holds microfacet materials (the PathTracer's), which its BDPT scene checks refuse."""
    m = B.Material()
    m.type = B.MAT_DIFFUSE
    m.a[:] = [0.5, 0.5, 0.5]
    return B.Scene(sc.prim_type, sc.prim_geom, np.zeros(sc.nprim, np.int32), [m],
                   [sc.lights[i] for i in range(sc.nlight)], sc.camera, sc.width, sc.height)


# (scene, PathTracer context)
CASES = [("CBspheres", False), ("CBbunny", False), ("grid", False), ("CBspheres_microfacet_al_ag", True)]
_cache = {}


def case(name, pt):
    """The scene, its spp-1 samples, their primary rays, the feature frame and the per-sample
    primitive: computed once per scene."""
    if name not in _cache:
        sc = scene_of(name)
        xys = D.all_samples(W, H)
        rays = D.host_primary_rays(sc, W, H, xys, SEED, pt=pt)
        feat = D.host_features(sc, W, H, 1, SEED, pt=pt)
        prim, t, _, _ = D.host_samples(sc, W, H, xys, SEED, pt=pt)
        _cache[name] = (sc, xys, rays, feat, prim, t)
    return _cache[name]


def albedo_table(sc):
    """The albedo per material (include/bdpt/bdpt.h), restated in numpy on the fp32 material records."""
    out = np.zeros((sc.nmat, 3), np.float32)
    for i in range(sc.nmat):
        m = sc.mats[i]
        a, b = np.array(m.a[:], np.float32), np.array(m.b[:], np.float32)
        if m.type in (B.MAT_DIFFUSE, B.MAT_MIRROR):
            out[i] = a
        elif m.type == B.MAT_REFRACTION:
            out[i] = b
        elif m.type == B.MAT_GLASS:
            out[i] = np.maximum(a, b)
        elif m.type == B.MAT_EMISSION:
            out[i] = np.minimum(a, np.float32(1))
        elif m.type == B.MAT_MICROFACET:   # (Rs + Rp) / 2 at cos = 1, in mf_F's fp32 operation order
            one, two = np.float32(1), np.float32(2)
            e2k2 = a * a + b * b
            t = (two * a) * one
            rs = (e2k2 - t + one) / (e2k2 + t + one)
            e = e2k2 * one
            rp = (e - t + one) / (e + t + one)
            out[i] = (one / two) * (rs + rp)
    return out


@pytest.mark.parametrize("name,pt", CASES)
def test_first_hit_matches_the_oracle_trace(name, pt):
    """The exported primary rays traced by the oracle's fp32 BVH (oracle mode 2): the per-sample
    primitive and the depth are bit-equal, and the coverage is prim >= 0."""
    sc, xys, rays, feat, prim, t = case(name, pt)
    ot, op = _rayref.oracle_trace(diffuse_copy(sc) if pt else sc, rays)
    assert np.array_equal(prim, op)
    hit = op >= 0
    assert hit.any()
    assert np.array_equal(t[hit], ot[hit]) and np.all(t[~hit] == 0)
    assert np.array_equal(feat[..., 6].ravel(), np.where(hit, ot, np.float32(0)))
    assert np.array_equal(feat[..., 7].ravel(), hit.astype(np.float32))


@pytest.mark.parametrize("name,pt", CASES)
def test_albedo_is_the_material_table(name, pt):
    sc, xys, rays, feat, prim, t = case(name, pt)
    tab = albedo_table(sc)
    want = np.where((prim >= 0)[:, None], tab[sc.prim_mat[np.maximum(prim, 0)]], np.float32(0))
    assert np.array_equal(feat[..., 0:3].reshape(-1, 3), want)
    if pt:
        assert (np.array([sc.mats[i].type for i in range(sc.nmat)])[sc.prim_mat[prim[prim >= 0]]] == B.MAT_MICROFACET).any()


def normals_fp64(sc, rays, prim, t):
    """Float64 shading normals at the hits: the barycentric interpolation of the triangle's vertex
    normals at the hit point, (p - c) / r for a sphere; turned to face the ray."""
    r = rays.astype(np.float64)
    o, d = r[:, 0:3], r[:, 3:6]
    p = o + t.astype(np.float64)[:, None] * d
    n = np.zeros((len(prim), 3))
    g = sc.prim_geom
    for k in np.nonzero(prim >= 0)[0]:
        i = prim[k]
        if sc.prim_type[i] == B.PRIM_SPHERE:
            n[k] = (p[k] - g[i, 0:3]) / g[i, 3]
        else:
            p0, p1, p2 = g[i, 0:3], g[i, 3:6], g[i, 6:9]
            m = np.stack([p1 - p0, p2 - p0], 1)
            b, *_ = np.linalg.lstsq(m, p[k] - p0, rcond=None)
            v = (1 - b[0] - b[1]) * g[i, 9:12] + b[0] * g[i, 12:15] + b[1] * g[i, 15:18]
            n[k] = v / np.linalg.norm(v)
        if n[k] @ d[k] > 0:
            n[k] = -n[k]
    return n


NORMAL_DEV = 1.7e-6   # measured (below); asserted at 5x


@pytest.mark.parametrize("name,pt", CASES)
def test_normals_against_float64(name, pt):
    """The spp-1 normal is shade_hit's unit normal, facing the ray. Largest component deviation from
    the float64 normals, measured on the CPU build at 24x18: CBspheres 7.5e-7, CBbunny 1.7e-6 (small
    triangles: the fp32 hit point's rounding against their size), grid 1.3e-6,
    CBspheres_microfacet_al_ag 7.0e-7. Asserted: 5 x 1.7e-6."""
    sc, xys, rays, feat, prim, t = case(name, pt)
    n = feat[..., 3:6].reshape(-1, 3).astype(np.float64)
    hit = prim >= 0
    dev = float(np.abs(n[hit] - normals_fp64(sc, rays, prim, t)[hit]).max())
    print(f"{name}: largest normal component deviation {dev:.3e}")
    assert dev <= 5 * NORMAL_DEV
    assert np.all(n[~hit] == 0)
    assert np.all(np.einsum("ij,ij->i", n[hit], rays[hit, 3:6].astype(np.float64)) <= 0)
    assert np.abs(np.linalg.norm(n[hit], axis=1) - 1).max() < 1e-6


@pytest.mark.parametrize("name,pt,lens", [("CBspheres", False, 0.0), ("CBspheres", False, 0.25),
                                          ("CBspheres_microfacet_al_ag", True, 0.1)])
def test_accumulation_in_sample_order(name, pt, lens):
    """At spp 5 the record is the fp32 sum, in sample order, of the five single-sample results,
    divided as specified; bit-equal."""
    sc = scene_of(name)
    S = 5
    xys = D.all_samples(W, H, S)
    prim, t, alb, nrm = D.host_samples(sc, W, H, xys, SEED, pt=pt, lens_radius=lens)
    feat = D.host_features(sc, W, H, S, SEED, pt=pt, lens_radius=lens)
    hit = (prim >= 0).reshape(H, W, S)
    alb, nrm, t = alb.reshape(H, W, S, 3), nrm.reshape(H, W, S, 3), t.reshape(H, W, S)
    assert np.all(t[~hit] == 0) and np.all(alb[~hit] == 0) and np.all(nrm[~hit] == 0)
    asum, nsum = np.zeros((H, W, 3), np.float32), np.zeros((H, W, 3), np.float32)
    dsum, hits = np.zeros((H, W), np.float32), np.zeros((H, W), np.int32)
    for s in range(S):
        asum, nsum, dsum, hits = asum + alb[:, :, s], nsum + nrm[:, :, s], dsum + t[:, :, s], hits + hit[:, :, s]
    n = np.float32(S)
    assert np.array_equal(feat[..., 0:3], asum / n)
    assert np.array_equal(feat[..., 3:6], nsum / n)
    assert np.array_equal(feat[..., 6], dsum / np.maximum(hits, 1).astype(np.float32))
    assert np.array_equal(feat[..., 7], hits.astype(np.float32) / n)


@pytest.mark.parametrize("lens", [0.0, 0.25])
def test_primary_rays_are_walk_begin_s(lens):
    """BDPT, pinhole and thin lens: the exported primary rays are bit-equal to the first ray of the
    eye walk as walk_begin (bdpt_paths.h) itself starts it."""
    sc = scene_of("CBspheres")
    xys = D.all_samples(W, H, 3)
    a = D.host_primary_rays(sc, W, H, xys, SEED, lens_radius=lens, focal_distance=3.5)
    b = D.host_walk_begin_rays(sc, W, H, xys, SEED, lens_radius=lens, focal_distance=3.5)
    assert np.array_equal(a, b)
    pin = D.host_primary_rays(sc, W, H, xys, SEED)
    assert np.array_equal(a, pin) == (lens == 0.0)
    if lens:   # the lens moves origins off the pinhole, inside the lens disk
        off = np.linalg.norm(a[:, 0:3] - pin[:, 0:3], axis=1)
        assert off.max() > 0.1 * lens and off.max() <= lens * 1.0001


@pytest.mark.parametrize("lens", [0.0, 0.1])
def test_primary_rays_are_the_pathtracers(lens):
    """PathTracer: on a scene where every primitive has an emitting material of its own, pt_sample
    (bdpt_pt.h) at depth 1 returns the radiance of its first hit; the feature pass's albedo (min(a, 1),
    a < 1) is bit-equal to it on every sample, so both hit the same primitive through one ray. The
    feature ray differs from the BDPT pinhole's by the PathTracer's own normalisation and lens draw."""
    base = scene_of("CBspheres")
    rng = np.random.default_rng(5)
    mats = []
    for i in range(base.nprim):
        m = B.Material()
        m.type = B.MAT_EMISSION
        m.a[:] = [float(np.float32(v)) for v in rng.uniform(0.05, 0.95, 3)]
        mats.append(m)
    sc = B.Scene(base.prim_type, base.prim_geom, np.arange(base.nprim, dtype=np.int32), mats,
                 [base.lights[i] for i in range(base.nlight)], base.camera, W, H)
    xys = D.all_samples(W, H, 2)
    rgb = D.host_pt_samples(sc, W, H, xys, SEED, lens_radius=lens)
    prim, t, alb, _ = D.host_samples(sc, W, H, xys, SEED, pt=True, lens_radius=lens)
    tab = albedo_table(sc)
    want = np.where((prim >= 0)[:, None], tab[np.maximum(prim, 0)], np.float32(0))
    assert (prim >= 0).sum() > 0.9 * len(prim) and len(np.unique(prim)) > 8
    assert np.array_equal(alb, want) and np.array_equal(rgb, want)


def test_abi_rejects_before_touching_a_device():
    """The new entry points validate their arguments first and set bdpt_last_error."""
    lib = B.load_library()
    out = (C.c_float * 8)()
    p = C.c_void_p()
    assert lib.bdpt_render_features(None, None, 0, 0) == B.BDPT_E_INVALID and b"null" in lib.bdpt_last_error()
    assert lib.bdpt_read_features(None, out) == B.BDPT_E_INVALID and b"null" in lib.bdpt_last_error()
    assert lib.bdpt_features_device_ptr(None, C.byref(p)) == B.BDPT_E_INVALID
    assert lib.bdpt_read_denoised(None, out) == B.BDPT_E_INVALID
    assert lib.bdpt_denoised_device_ptr(None, C.byref(p)) == B.BDPT_E_INVALID
    assert lib.bdpt_denoise_default_params(None) == B.BDPT_E_INVALID
    assert lib.bdpt_denoise(None, 7, None) == B.BDPT_E_INVALID and b"frame id" in lib.bdpt_last_error()
    assert lib.bdpt_denoise(None, B.FRAME_SAMPLE, None) == B.BDPT_E_INVALID and b"null" in lib.bdpt_last_error()
    d = B.denoise_params()
    assert (d.levels, d.demodulate) == (D.defaults()["levels"], int(D.defaults()["demodulate"]))
    assert d.sigma_color == D.defaults()["sigma_color"] and tuple(d.reserved) == (0, 0, 0)
    buf = C.c_void_p(4096)   # never dereferenced: every call below is rejected first
    for kw, msg in ((dict(levels=9), b"levels"), (dict(levels=-1), b"levels"), (dict(sigma_color=0.0), b"sigmas")):
        q = B.denoise_params(**kw)
        assert lib.bdpt_denoise_buffers(0, buf, buf, 8, 8, C.byref(q), buf, None) == B.BDPT_E_INVALID
        assert msg in lib.bdpt_last_error()
        assert lib.bdpt_denoise(None, B.FRAME_SAMPLE, C.byref(q)) == B.BDPT_E_INVALID and msg in lib.bdpt_last_error()
    q = B.denoise_params()
    q.reserved[1] = 1
    assert lib.bdpt_denoise_buffers(0, buf, buf, 8, 8, C.byref(q), buf, None) == B.BDPT_E_INVALID
    assert b"reserved" in lib.bdpt_last_error()
    q = B.denoise_params()
    assert lib.bdpt_denoise_buffers(0, None, buf, 8, 8, C.byref(q), buf, None) == B.BDPT_E_INVALID
    assert lib.bdpt_denoise_buffers(0, buf, buf, 0, 8, C.byref(q), buf, None) == B.BDPT_E_INVALID
    assert lib.bdpt_denoise_buffers(0, buf, C.c_void_p(4100), 8, 8, C.byref(q), buf, None) == B.BDPT_E_INVALID
    assert b"aligned" in lib.bdpt_last_error()
