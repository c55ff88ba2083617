"""The per-pixel bound between the GPU's frames and the CPU build of the same device code
(tests/test_pixel_bounds.py, tests/test_gpu_pixel_bounds.py), derived, not measured.

Both sides compute every sample's fp32 addends with the same operations; they differ in how the
addends are added into a pixel. The reference (tests/native/core_cpu.cpp, bit-equal to oracle mode 2)
adds in fp64: the light image is the exact sum of its fp32 splats, the eye image the fp64 sum of the
per-sample values fl(fl(sum of the sample's connections) / spp). The GPU adds in fp32, in an order
that the scheduling decides: per-lane LDS partial sums, the wave butterfly of flush_queue, global
atomics; and it multiplies each eye addend by 1 / spp before adding where the CPU does so once per
sample; k_combine adds one more rounding.

With u = 2^-24, any fp32 summation order or grouping of n non-negative addends stays within
(n - 1) u sum(a) of the exact sum. Hence, for a pixel and channel with reference R, GPU value G and
at most n addends,

    |G - R| <= tol = 2 (n + 2) u R,        and        R == 0  =>  G == 0 exactly

(the factor 2 and the + 2 cover the per-addend 1 / spp product, the reference's own per-sample fp32
sum and the combine; they are not tuned against GPU output).

* eye image:    n = S_p (M + 2)^2, S_p = samples rendered for the pixel, (M + 2)^2 bounding the
                (i, j) strategies of one sample, M = max(max_depth, 1);
* light image:  n = the pixel's splat count, from the CPU build;
* sample image: tol_eye + tol_light + u R.

No pixel may violate the bound."""
import ctypes as C
import os
import sys

import numpy as np

import bdpt_amd as B
from _util import REPO, golden_scene

U = 2.0 ** -24


# ------------------------------------------------------------------------------------------------
# the bound

def eye_n(samples, M):
    """Upper bound on the fp32 addends of an eye-image pixel: samples (scalar or (H, W)) x (M + 2)^2."""
    return np.asarray(samples, np.int64) * (max(int(M), 1) + 2) ** 2


def tol_of(R, n):
    """2 (n + 2) u R per pixel and channel; R (H, W, 3), n scalar or (H, W)."""
    n = np.asarray(n, np.float64)
    if n.ndim == 2:
        n = n[..., None]
    return 2.0 * (n + 2.0) * U * np.asarray(R, np.float64)


def violations(G, R, tol):
    """Boolean (H, W, 3): |G - R| > tol, a non-finite G, or G != 0 where R == 0."""
    G, R = np.asarray(G, np.float64), np.asarray(R, np.float64)
    return ~np.isfinite(G) | (np.abs(G - R) > tol) | ((R == 0) & (G != 0))


def worst(G, R, n, tol, k=5):
    """The k worst entries as (x, y, channel, G, R, n, tol), by |G - R| / tol (inf where tol = 0 < |G - R|)."""
    G, R = np.asarray(G, np.float64), np.asarray(R, np.float64)
    n = np.broadcast_to(np.asarray(n)[..., None] if np.ndim(n) == 2 else np.asarray(n), R.shape)
    d = np.abs(G - R)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(d > 0, d / tol, 0.0)
    ratio = np.where(np.isfinite(G), ratio, np.inf)
    out = []
    for f in np.argsort(ratio, axis=None)[::-1][:k]:
        y, x, c = np.unravel_index(f, R.shape)
        out.append((int(x), int(y), int(c), float(G[y, x, c]), float(R[y, x, c]), int(n[y, x, c]), float(tol[y, x, c])))
    return out


def margin(G, R, tol):
    """The largest |G - R| / tol over the entries with tol > 0 (0.0 when there is none)."""
    d = np.abs(np.asarray(G, np.float64) - np.asarray(R, np.float64))
    ok = tol > 0
    return float((d[ok] / tol[ok]).max()) if ok.any() else 0.0


MARGINS = {"eye": 0.0, "light": 0.0, "sample": 0.0}   # the largest |G - R| / tol seen by check_frames


def check_image(kind, G, R, n, tol, label):
    bad = violations(G, R, tol)
    m = margin(G, R, tol)
    MARGINS[kind] = max(MARGINS[kind], m)
    print(f"{label}: {kind} max |G-R|/tol {m:.4f} (largest so far {MARGINS[kind]:.4f}), outside {int(bad.sum())}")
    if bad.any():
        print(f"{label}: {kind} worst (x, y, channel, G, R, n, tol):")
        for w in worst(G, R, n, tol):
            print("   ", w)
    assert not bad.any(), f"{label}: {int(bad.any(axis=2).sum())} {kind}-image pixels outside the per-pixel bound"


def check_eye(G, R, samples, M, label):
    """The eye image alone (what a test with only an oracle eye image can check)."""
    n = eye_n(samples, M)
    check_image("eye", G, R, n, tol_of(R, n), label)


def check_frames(g, ref, samples, M, label):
    """g: the GPU's "eye", "light" and "sample" frames; ref: a render_rec() result; samples: rendered
    per pixel (scalar or (H, W)). Asserts the bound on all three images."""
    ne = eye_n(samples, M)
    te, tl = tol_of(ref["eye"], ne), tol_of(ref["light"], ref["nsplat"])
    rs = ref["eye"] + ref["light"]
    check_image("eye", g["eye"], ref["eye"], ne, te, label)
    check_image("light", g["light"], ref["light"], ref["nsplat"], tl, label)
    ns = np.broadcast_to(ne, ref["nsplat"].shape) + ref["nsplat"]
    check_image("sample", g["sample"], rs, ns, te + tl + U * rs, label)


# ------------------------------------------------------------------------------------------------
# the CPU build with its addends on record

_IP, _FP, _DP = C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_double)
_rec_ready = False


def _core():
    global _rec_ready
    from test_core_cpu import core
    lib = core()
    if not _rec_ready:
        lib.core_cpu_render_rec.argtypes = [C.POINTER(B.SceneDesc), C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64,
                                            C.c_int, C.c_int, _IP, C.c_int, _DP, _DP, _DP, C.c_int, C.c_int,
                                            _IP, _IP, _FP, _IP, _FP, _IP, _FP, C.POINTER(C.c_longlong),
                                            C.POINTER(C.c_longlong), _FP]
        lib.core_cpu_lds_facts.argtypes = [C.POINTER(B.SceneDesc), C.c_int, _IP]
        lib.core_cpu_lds_plan.argtypes = [C.POINTER(B.SceneDesc), C.c_int, C.c_int, C.c_longlong, C.c_longlong,
                                          C.POINTER(C.c_longlong)]
        _rec_ready = True
    return lib


def render_rec(scene, W, H, spp, M, seed=5489, s0=0, count=None, pixels=None, lds_mode=0, rr=False, record=False):
    """core_cpu_render_rec: {"eye", "light"} float64 (H, W, 3), {"nsplat"} int (H, W), and with record
    the addends as (pix, rgb) arrays: "splats", "eye_addends" (a connection's value before the 1 / spp
    product) and "eye_samples" (per sample, after it); "vmin": the smallest component of any addend. pixels: a list of (x, y) instead of the frame."""
    lib = _core()
    count = spp - s0 if count is None else count
    eye, light, st = np.zeros((H, W, 3)), np.zeros((H, W, 3)), np.zeros(8)
    nsplat = np.zeros((H, W), np.int32)
    px, npx = None, 0
    if pixels is not None:
        px = np.ascontiguousarray(pixels, dtype=np.int32).reshape(-1, 2)
        npx = px.shape[0]
    total = npx if pixels is not None else W * H
    k = (max(M, 1) + 2) ** 2
    caps = [total * count * (max(M, 1) + 2), total * count * k, total * count] if record else [0, 0, 0]
    bufs = [(np.zeros(max(c, 1), np.int32), np.zeros(3 * max(c, 1), np.float32)) for c in caps]
    cap = (C.c_longlong * 3)(*caps)
    n_out = (C.c_longlong * 3)()
    vmin = (C.c_float * 3)()
    d = scene.desc()
    args = []
    for p, f in bufs:
        args += [p.ctypes.data_as(_IP) if record else None, f.ctypes.data_as(_FP) if record else None]
    rc = lib.core_cpu_render_rec(C.byref(d), W, H, spp, M, seed, s0, count,
                                 px.ctypes.data_as(_IP) if px is not None else None, npx, eye.ctypes.data_as(_DP),
                                 light.ctypes.data_as(_DP), st.ctypes.data_as(_DP), lds_mode, 1 if rr else 0,
                                 nsplat.ctypes.data_as(_IP), *args, cap, n_out, vmin)
    assert rc == 0, rc
    out = {"eye": eye, "light": light, "nsplat": nsplat, "stats": st, "vmin": float(min(vmin))}
    if record:
        for name, (p, f), c, n in zip(("splats", "eye_addends", "eye_samples"), bufs, caps, n_out):
            assert n <= c, (name, n, c)   # a record cut short would make every check on it vacuous
            out[name] = (p[:n].copy(), f[:3 * n].reshape(n, 3).copy())
        assert n_out[0] == nsplat.sum()
    return out


def inf_render_rec(scene, W, H, spp, M, seed=5489, rr=False, lds_mode=0):
    """core_cpu_inf_render_counts (the infinite_lights flavour): eye, light, nsplat and "vmin", the
    smallest component of any addend."""
    from _inflights import core_inf
    lib = core_inf()
    lib.core_cpu_inf_render_counts.argtypes = [C.POINTER(B.SceneDesc), C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64,
                                               C.c_int, C.c_int, _IP, C.c_int, _DP, _DP, _DP, C.c_int, C.c_int,
                                               C.c_int, _IP, _FP]
    eye, light, st = np.zeros((H, W, 3)), np.zeros((H, W, 3)), np.zeros(10)
    nsplat = np.zeros((H, W), np.int32)
    vmin = C.c_float(np.inf)
    d = scene.desc()
    rc = lib.core_cpu_inf_render_counts(C.byref(d), W, H, spp, M, seed, 0, spp, None, 0, eye.ctypes.data_as(_DP),
                                        light.ctypes.data_as(_DP), st.ctypes.data_as(_DP), lds_mode, 1 if rr else 0,
                                        1, nsplat.ctypes.data_as(_IP), C.byref(vmin))
    assert rc == 0, rc
    return {"eye": eye, "light": light, "nsplat": nsplat, "stats": st, "vmin": float(vmin.value)}


# What bdpt_hip.hip's launch plan is chosen from. The two byte limits follow from its constants (160 KB
# of LDS per CU and one 1024-lane block per CU, minus 16 wave queues of 6,400 B, 256 B and the 2,560 B
# of static material / light arrays; 8 overflow slots x 1024 lanes x 4 B): the GPU tests assert the plan
# the library reports, so a change of those constants shows as a failed plan, not as a silent miss.
LDS_SCENE_MAX = 58624
LDS_STACK_BYTES = 32768
FLAT_MAX_PRIMS = 24
LDS_MATS, LDS_LIGHTS = 48, 8
WAVEQ_BYTES = 16 * 6400


def lds_facts(scene, infinite_lights=False):
    """{"nprim", "full", "flat", "n_top", "node_bytes", "nmat", "nlights", "flat_n"} of build_host_scene, and
    "cap": the treelet nodes the LDS budget admits beside the stack slots."""
    out = (C.c_int * 8)()
    d = scene.desc()
    assert _core().core_cpu_lds_facts(C.byref(d), 1 if infinite_lights else 0, out) == 0
    f = dict(zip(("nprim", "full", "flat", "n_top", "node_bytes", "nmat", "nlights", "flat_n"), list(out)))
    f["cap"] = (LDS_SCENE_MAX - LDS_STACK_BYTES) // f["node_bytes"]
    return f


def lds_plan(scene, forced_lm=-1, lds_max=LDS_SCENE_MAX, treelet_max=LDS_SCENE_MAX - LDS_STACK_BYTES, infinite_lights=False):
    """lds_plan (csrc/bdpt_ldsplan.h) on build_host_scene's scene: {"lm", "ntop", "n_node4", "copy_bytes",
    "flat_bytes", "full_bytes"}. The default budgets are a BDPT launch's. scene None: the host scene with
    no primitives."""
    out = (C.c_longlong * 6)()
    d = scene.desc() if scene is not None else None
    assert _core().core_cpu_lds_plan(C.byref(d) if d is not None else None, 1 if infinite_lights else 0, forced_lm,
                                     lds_max, treelet_max, out) == 0
    return dict(zip(("lm", "ntop", "n_node4", "copy_bytes", "flat_bytes", "full_bytes"), list(out)))


# ------------------------------------------------------------------------------------------------
# scenes: generated geometry inside CBempty's box (x, z in [-1, 1], y in [0, 1.5]), its 12 wall
# triangles kept, so the golden camera sees it and the light reaches it

def full_view(name, W, H):
    """The golden scene with its own field of view on a W x H frame. (retarget_camera follows the
    reference's Camera::set_screen_size, which shrinks the view with the frame: a 16x12 frame then
    sees a hundredth of the box, and hardly any light-image splat lands in it.)"""
    sc = golden_scene(name)
    sc.width, sc.height = W, H
    return sc


def _mat(kind, a=(0, 0, 0), b=(0, 0, 0), ior=0.0):
    m = B.Material()
    m.type = kind
    m.a[:], m.b[:], m.ior = a, b, ior
    return m


def _copy_light(l, dx=0.0, dz=0.0, scale=1.0):
    out = B.Light.from_buffer_copy(l)
    out.position[0] += dx
    out.position[2] += dz
    for k in range(3):
        out.radiance[k] *= scale
    return out


def box_scene(W, H, N, nsph, area_light=False, seed=1):
    """CBempty's box with a relief of 2 N^2 triangles on its floor (_rayref.grid, scaled into the
    box) and nsph spheres above it that alternate CBspheres' mirror and glass materials; CBempty's
    point light, or CBspheres' area light."""
    from _rayref import grid
    base = full_view("CBempty", W, H)
    sph = full_view("CBspheres", W, H)
    g = grid(N, scale=0.9, offset=(0.0, 0.2, 0.0), nsph=nsph, seed=seed)
    mats = [base.mats[i] for i in range(base.nmat)]
    mirror = next(sph.mats[i] for i in range(sph.nmat) if sph.mats[i].type == B.MAT_MIRROR)
    glass = next(sph.mats[i] for i in range(sph.nmat) if sph.mats[i].type == B.MAT_GLASS)
    mats += [mirror, glass]
    relief = _mat(B.MAT_DIFFUSE, (0.6, 0.7, 0.5))
    mats.append(relief)
    ntri = 2 * N * N
    gm = np.concatenate([np.full(ntri, base.nmat + 2), base.nmat + (np.arange(nsph) % 2)]).astype(np.int32)
    lights = [sph.lights[0]] if area_light else [base.lights[i] for i in range(base.nlight)]
    return B.Scene(np.concatenate([base.prim_type, g.prim_type]), np.concatenate([base.prim_geom, g.prim_geom]),
                   np.concatenate([base.prim_mat, gm]), mats, lights, base.camera, W, H)


def staging_scene(W, H, nmat, nlights, alter_last_mat=False, alter_last_light=False):
    """The 25-primitive box (12 walls, a relief of 8 triangles, 5 spheres) with nmat diffuse materials
    of distinct albedos, primitive i using material i (nmat - 1) // 24 (the first and the last are in
    use, the last by the last sphere), and nlights copies of CBspheres' area light at shifted positions
    with radiance / nlights."""
    sc = box_scene(W, H, 2, 5, area_light=True)
    assert sc.nprim == 25
    mats = []
    for k in range(nmat):
        t = (k + 1) / (nmat + 1)
        mats.append(_mat(B.MAT_DIFFUSE, (0.25 + 0.6 * t, 0.85 - 0.5 * t, 0.3 + 0.5 * ((7 * k) % 11) / 11)))
    if alter_last_mat:
        mats[-1] = _mat(B.MAT_DIFFUSE, (0.05, 0.05, 0.05))
    pm = (np.arange(25) * (nmat - 1)) // 24
    lights = []
    for k in range(nlights):
        a = 2 * np.pi * k / nlights
        lights.append(_copy_light(sc.lights[0], 0.3 * np.cos(a), 0.15 * np.sin(a), 1.0 / nlights))
    if alter_last_light:
        lights[-1] = _copy_light(lights[-1], scale=3.0)
    return B.Scene(sc.prim_type, sc.prim_geom, pm.astype(np.int32), mats, lights, sc.camera, W, H)


def with_env(sc, w=32, h=16):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from envmap import synth_envmap
    sc.set_envmap(synth_envmap(w, h))
    return sc


def with_directional(sc):
    """sc plus a directional light: the infinite_lights kernel flavour."""
    l = B.Light()
    l.type = B.LIGHT_DIRECTIONAL
    l.radiance[:] = (1.5, 1.4, 1.2)
    l.direction[:] = (0.2, 0.9, 0.4)
    return B.Scene(sc.prim_type, sc.prim_geom, sc.prim_mat, [sc.mats[i] for i in range(sc.nmat)],
                   [sc.lights[i] for i in range(sc.nlight)] + [l], sc.camera, sc.width, sc.height, sc.envmap)


def lit_share(ref):
    """The shares of pixels that are non-zero in the eye and in the light reference."""
    return float((ref["eye"].sum(axis=2) > 0).mean()), float((ref["light"].sum(axis=2) > 0).mean())
