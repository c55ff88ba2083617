"""Ray-query conformance helper (tests/test_ray_queries.py, tests/test_gpu_ray_queries.py):
generated scenes away from the Cornell boxes, their ray sets, and brute_fp64, a float64 closest-hit
reference that loops over every primitive with no tree.

Run as a program it is the child process of the tests that must not stall the suite on a traversal
that never returns: `python _rayref.py trace|render <scene> <lds_mode> <in.npy|-> <out.npz>`."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

TESTS = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(TESTS)
for _p in (REPO, os.path.join(REPO, "bidirectional-pathtracing_amd"), TESTS):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import bdpt_amd as B   # noqa: E402
from _util import golden_scene, oracle   # noqa: E402

PF, PI = C.POINTER(C.c_float), C.POINTER(C.c_int)
FRAME = (16, 12)   # the frame of the leaf-root renders


# ------------------------------------------------------------------------------------------------
# scenes: B.Scene objects around CBempty's materials, light and camera

def _scene(tris, sphs=(), W=FRAME[0], H=FRAME[1]):
    """tris (n, 3, 3) vertices, sphs (m, 4) centre + radius; material 0, flat normals."""
    base = golden_scene("CBempty", W, H)
    tris = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    sphs = np.asarray(sphs, np.float64).reshape(-1, 4)
    n, m = len(tris), len(sphs)
    geom = np.zeros((n + m, 18))
    geom[:n, :9] = tris.reshape(n, 9)
    nrm = np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0])
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
    geom[:n, 9:18] = np.tile(nrm, (1, 3))
    geom[n:, :4] = sphs
    ptype = np.concatenate([np.zeros(n, np.int32), np.ones(m, np.int32)])
    return B.Scene(ptype, geom, np.zeros(n + m, np.int32), [base.mats[i] for i in range(base.nmat)],
                   [base.lights[i] for i in range(base.nlight)], base.camera, base.width, base.height)


def grid(N=12, scale=1.0, offset=(0.0, 0.0, 0.0), nsph=6, seed=1):
    """A height field of 2 N^2 triangles over [-1, 1]^2 (shared edges and vertices) and nsph spheres
    above it, scaled about the origin and then translated."""
    rng = np.random.default_rng(seed)
    xs = np.linspace(-1.0, 1.0, N + 1)
    h = 0.15 * rng.uniform(-1, 1, (N + 1, N + 1))
    P = np.stack(np.broadcast_arrays(xs[:, None], h, xs[None, :]), axis=-1)   # (N+1, N+1, 3), y up
    a, b, c, d = P[:-1, :-1], P[1:, :-1], P[1:, 1:], P[:-1, 1:]
    tris = np.concatenate([np.stack([a, b, c], 2).reshape(-1, 3, 3), np.stack([a, c, d], 2).reshape(-1, 3, 3)])
    sph = np.concatenate([rng.uniform(-0.7, 0.7, (nsph, 1)), rng.uniform(0.5, 0.9, (nsph, 1)),
                          rng.uniform(-0.7, 0.7, (nsph, 1)), rng.uniform(0.1, 0.25, (nsph, 1))], axis=1)
    off = np.asarray(offset, np.float64)
    sph[:, :3] = sph[:, :3] * scale + off
    sph[:, 3] *= scale
    return _scene(tris * scale + off, sph)


def fan(n=256, seed=2):
    """n large triangles through one centre (every box overlaps every other) and 3 spheres."""
    rng = np.random.default_rng(seed)
    c = np.array([0.0, 0.5, 0.0])
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    w = np.cross(u, rng.normal(size=(n, 3)))
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    r = rng.uniform(0.6, 1.0, (n, 1))
    tris = np.stack([c - 0.3 * r * u - 0.2 * r * w, c + r * u, c + r * w], axis=1)
    sph = [[0.6, 0.9, 0.3, 0.15], [-0.5, 0.2, 0.4, 0.2], [0.1, 0.4, -0.7, 0.1]]
    return _scene(tris, sph)


def slivers(n=200, seed=3):
    """n needles of aspect 1e4 (length 1, width 1e-4), randomly oriented, over a 2-triangle floor."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.6, 0.6, (n, 3)) + np.array([0.0, 0.7, 0.0])
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    w = np.cross(u, rng.normal(size=(n, 3)))
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    tris = np.stack([p - 0.5 * u, p + 0.5 * u, p - 0.5 * u + 1e-4 * w], axis=1)
    f = np.array([[-1.5, 0, -1.5], [1.5, 0, -1.5], [1.5, 0, 1.5], [-1.5, 0, 1.5]])
    floor = np.stack([f[[0, 1, 2]], f[[0, 2, 3]]])
    return _scene(np.concatenate([tris, floor]))


STACK_SPACING = 1e-2


def stack(layers=8, spacing=STACK_SPACING):
    """Parallel horizontal quads (2 triangles each) at y = 0.5 + k spacing."""
    tris = []
    for k in range(layers):
        y = 0.5 + k * spacing
        q = np.array([[-1, y, -1], [1, y, -1], [1, y, 1], [-1, y, 1]], np.float64)
        tris += [q[[0, 1, 2]], q[[0, 2, 3]]]
    return _scene(np.stack(tris))


_TINY = np.array([[[-0.9, 0.1, -0.6], [0.9, 0.1, -0.6], [0.0, 1.6, -0.5]],
                  [[0.9, 0.1, -0.6], [1.8, 1.6, -0.5], [0.0, 1.6, -0.5]]])   # shares an edge: one leaf


def same(n=64):
    """One triangle n times (coincident centroids: the oracle refuses it)."""
    return _scene(np.repeat(_TINY[:1], n, axis=0))


def tiny(k):
    """k in {1, 2} triangles, or "sphere": one sphere. The device tree's root is a leaf."""
    if k == "sphere":
        return _scene(np.zeros((0, 3, 3)), [[0.0, 0.7, -0.3, 0.45]])
    return _scene(_TINY[:int(k)])


def degenerate_render_scene(kind):
    """tiny(kind) out of CBempty's own last triangles (its back wall first), which the 16x12 frame's
    camera sees and the light reaches; kind "sphere": a sphere in the middle of the box."""
    base = golden_scene("CBempty", *FRAME)
    if kind == "sphere":
        return _scene(np.zeros((0, 3, 3)), [[0.0, 0.5, 0.0, 0.5]])
    k = int(kind)
    tri = base.prim_type == 0
    return B.Scene(np.zeros(k, np.int32), base.prim_geom[tri][::-1][:k], base.prim_mat[tri][::-1][:k],
                   [base.mats[i] for i in range(base.nmat)], [base.lights[i] for i in range(base.nlight)],
                   base.camera, base.width, base.height)


SCENES = {
    "grid": lambda: grid(12),
    "grid_1e3": lambda: grid(12, scale=1e3),
    "grid_off": lambda: grid(12, offset=(1000.0, 1000.0, 1000.0)),
    "fan": lambda: fan(256),
    "slivers": lambda: slivers(200),
    "stack": lambda: stack(8),
    "same": lambda: same(64),
    "tiny1": lambda: tiny(1),
    "tiny2": lambda: tiny(2),
    "tiny_sphere": lambda: tiny("sphere"),
    "odd": lambda: grid(6, nsph=4),
    "render1": lambda: degenerate_render_scene(1),
    "render2": lambda: degenerate_render_scene(2),
    "render_sphere": lambda: degenerate_render_scene("sphere"),
}
# (scale, offset) of a scene's coordinates: tmin and the ray origins follow them
PLACE = {"grid_1e3": (1e3, 0.0), "grid_off": (1.0, 1000.0)}
ORACLE_REFUSES = ("same",)


def scene(name):
    return SCENES[name]()


# ------------------------------------------------------------------------------------------------
# rays: (n, 8) float32 rows of o, d, tmin, tmax

def pack(o, d, tmin, tmax):
    n = len(o)
    r = np.empty((n, 8), np.float32)
    r[:, :3], r[:, 3:6] = o, d
    r[:, 6], r[:, 7] = tmin, tmax
    return r


def random_rays(name, n=2000, seed=17):
    """Origins uniform in a box around the scene, unit directions uniform on the sphere, tmin 1e-5
    (times the scene's scale), tmax infinite. The stack's rays come from above, steeply."""
    rng = np.random.default_rng(seed)
    s, off = PLACE.get(name, (1.0, 0.0))
    o = rng.uniform([-1.0, 0.0, -1.0], [1.0, 1.4, 1.0], (n, 3))
    d = rng.normal(size=(n, 3))
    if name == "stack":
        o = rng.uniform([-0.9, 0.9, -0.9], [0.9, 1.4, 0.9], (n, 3))
        d = np.stack([rng.uniform(-0.3, 0.3, n), -np.ones(n), rng.uniform(-0.3, 0.3, n)], axis=1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return pack(o * s + off, d, 1e-5 * s, np.inf)


ODD_KINDS = ("tmin_neg", "tmin_gt_tmax", "d_zero", "nan_origin", "tmin_inf", "d_1e-20", "d_1e18")


def odd_rays(kind, n=100, seed=23):
    r = random_rays("odd", n, seed)
    if kind == "tmin_neg":
        r[:, 6] = -10.0
    elif kind == "tmin_gt_tmax":
        r[:, 6], r[:, 7] = 2.0, 1.0
    elif kind == "d_zero":
        r[:, 3:6] = 0.0
    elif kind == "nan_origin":
        r[:, 0:3] = np.nan
    elif kind == "tmin_inf":
        r[:, 6] = np.inf
    elif kind == "d_1e-20":
        r[:, 3:6] *= np.float32(1e-20)
    elif kind == "d_1e18":
        r[:, 3:6] *= np.float32(1e18)
    else:
        raise KeyError(kind)
    return r


def nan_origin_rays(n):
    r = random_rays("grid", n, 29)
    r[:, 0:3] = np.nan
    return r


# ------------------------------------------------------------------------------------------------
# the float64 reference

BAND = 1e-4      # a relative quantity under this leaves the ray undecided
NEAR = 1e-3      # ... for a primitive this close to being accepted
GRAZE = 0.02     # |d.n| / (|d||n|) of the hit triangle under this: undecided


def canonical(sc):
    """Per primitive, the first primitive with the same record: coincident copies (same(64)) are one
    surface, and which copy a query names is the tie rule's business, not the geometry's."""
    first, canon = {}, np.empty(sc.nprim, np.int32)
    for i in range(sc.nprim):
        canon[i] = first.setdefault((int(sc.prim_type[i]), sc.prim_geom[i, :9].astype(np.float32).tobytes()), i)
    return canon


def brute_fp64(sc, rays):
    """Closest hit of every ray by Möller–Trumbore and the sphere quadratic in float64 over every
    primitive, on the inputs as the device holds them: vertices, edges (p2 - p1, p3 - p1) and the
    sphere record rounded to fp32, the rays as given (fp32). Returns (prim, t, decided): prim = the
    scene index or -1, t float64 (inf for none). A ray is undecided when a different rounding could
    change its answer: a primitive within NEAR of being accepted has a barycentric, 1 - b1 - b2 or
    the distance of t from a finite window end (relative to t) under BAND; a sphere's discriminant
    is under BAND b^2; the two closest accepted t are closer than BAND (relative); or the ray
    grazes the hit triangle. Coincident copies of a primitive count once, as canonical() numbers them."""
    rays = np.asarray(rays, np.float32).reshape(-1, 8).astype(np.float64)
    o, d, tmin, tmax = rays[:, :3], rays[:, 3:6], rays[:, 6], rays[:, 7]
    n = len(rays)
    g = sc.prim_geom.astype(np.float32)
    best_t, second_t = np.full(n, np.inf), np.full(n, np.inf)
    best_p = np.full(n, -1)
    graze = np.zeros(n, bool)
    decided = np.ones(n, bool)
    fin_min, fin_max = np.isfinite(tmin), np.isfinite(tmax)

    def window(t):
        """t's signed distance into the window, relative to |t| (inf at an infinite end)."""
        with np.errstate(invalid="ignore", divide="ignore"):
            mag = np.maximum(np.abs(t), 1e-300)
            lo = np.where(fin_min, (t - tmin) / mag, np.inf)
            hi = np.where(fin_max, (tmax - t) / mag, np.inf)
        return np.minimum(lo, hi)

    def take(i, ok, t, gz):
        nonlocal best_t, second_t, best_p, graze
        t = np.where(ok, t, np.inf)
        closer = t < best_t
        second_t = np.where(closer, best_t, np.minimum(second_t, t))
        best_p = np.where(closer, i, best_p)
        graze = np.where(closer, gz, graze)
        best_t = np.where(closer, t, best_t)

    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        dn = np.linalg.norm(d, axis=1)
        canon = canonical(sc)
        for i in range(sc.nprim):
            if canon[i] != i:
                continue
            if sc.prim_type[i] == 0:
                p0 = g[i, 0:3].astype(np.float64)
                e1 = (g[i, 3:6] - g[i, 0:3]).astype(np.float64)   # fp32 differences, as the device stores them
                e2 = (g[i, 6:9] - g[i, 0:3]).astype(np.float64)
                s = o - p0
                s1 = np.cross(d, e2)
                den = s1 @ e1
                b1 = np.einsum("ij,ij->i", s1, s) / den
                s2 = np.cross(s, e1)
                b2 = np.einsum("ij,ij->i", s2, d) / den
                t = (s2 @ e2) / den
                q = np.stack([b1, b2, 1.0 - b1 - b2, window(t)])
                qmin = q.min(axis=0)
                ok = (qmin >= 0) & np.isfinite(t)
                near = qmin > -NEAR
                decided &= ~(near & (np.abs(q).min(axis=0) < BAND))
                nr = np.cross(e1, e2)
                gz = np.abs(d @ nr) / (dn * np.linalg.norm(nr)) < GRAZE
                take(i, ok, t, gz)
            else:
                c, r = g[i, 0:3].astype(np.float64), float(g[i, 3])
                f = o - c
                a = np.einsum("ij,ij->i", d, d)
                b = 2 * np.einsum("ij,ij->i", f, d)
                cc = np.einsum("ij,ij->i", f, f) - r * r
                delta = b * b - 4 * a * cc
                decided &= ~(np.abs(delta) < BAND * b * b)
                root = np.sqrt(np.maximum(delta, 0))
                t1, t2 = (-b - root) / (2 * a), (-b + root) / (2 * a)
                w1, w2 = window(t1), window(t2)
                real = delta >= 0
                in1, in2 = real & (w1 >= 0) & (t1 > 0), real & (w2 >= 0) & (t2 > 0)
                for tt, w in ((t1, w1), (t2, w2)):
                    decided &= ~(real & (w > -NEAR) & (np.abs(w) < BAND))
                take(i, in1 | in2, np.where(in1, t1, t2), np.zeros(n, bool))
        gap = (second_t - best_t) / np.maximum(np.abs(best_t), 1e-300)
        decided &= ~(np.isfinite(second_t) & (gap < BAND))
    decided &= ~graze
    return best_p.astype(np.int32), best_t, decided


# ------------------------------------------------------------------------------------------------
# the tracers

def oracle_trace(sc, rays, any_hit=False):
    """oracle_trace_rays(mode 2): the reference's fp32 algorithm over its own BVH. None when the
    oracle refuses the scene."""
    rays = np.ascontiguousarray(rays, np.float32)
    n = len(rays)
    t, p = np.empty(n, np.float32), np.empty(n, np.int32)
    d = sc.desc()
    rc = oracle().oracle_trace_rays(C.byref(d), 2, rays.ctypes.data_as(PF), n, 1 if any_hit else 0,
                                    t.ctypes.data_as(PF), p.ctypes.data_as(PI))
    return None if rc != 0 else (t, p)


def core_trace(sc, lds_mode, rays, any_hit=False):
    """core_cpu_trace_rays: bdpt_trace_rays' traversal in the CPU build of the device code."""
    from test_core_cpu import core
    lib = core()
    lib.core_cpu_trace_rays.argtypes = [C.POINTER(B.SceneDesc), C.c_int, PF, C.c_int, C.c_int, PF, PI]
    rays = np.ascontiguousarray(rays, np.float32)
    n = len(rays)
    t, p = np.empty(n, np.float32), np.empty(n, np.int32)
    d = sc.desc()
    rc = lib.core_cpu_trace_rays(C.byref(d), lds_mode, rays.ctypes.data_as(PF), n, 1 if any_hit else 0,
                                 t.ctypes.data_as(PF), p.ctypes.data_as(PI))
    assert rc == 0
    return t, p


def binary_nodes(sc):
    """Nodes of the device's binary tree before the wide collapse: 1 = its root is a leaf."""
    from test_core_cpu import core
    lib = core()
    depth, nodes = C.c_int(), C.c_int()
    d = sc.desc()
    assert lib.core_cpu_dev_tree(C.byref(d), C.byref(depth), C.byref(nodes)) == 0
    return nodes.value


CHILD_LIMIT = 60   # seconds: a traversal that never returns fails its test instead of stalling the suite


def child(what, name, lds_mode, tmp_path, rays=None):
    """what = "trace": (t, prim, any) of `rays` on scene `name`; "render": (eye, light) of the
    16x12 s1 m5 frame — through the CPU library in a child process under CHILD_LIMIT."""
    inp, out = "-", str(tmp_path / f"{what}_{name}_{lds_mode}.npz")
    if rays is not None:
        inp = str(tmp_path / f"rays_{name}_{lds_mode}.npy")
        np.save(inp, np.ascontiguousarray(rays, np.float32))
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), what, name, str(lds_mode), inp, out],
                           capture_output=True, text=True, timeout=CHILD_LIMIT)
    except subprocess.TimeoutExpired:
        raise AssertionError(f"{what} of {name} in LDS mode {lds_mode} did not return within {CHILD_LIMIT} s")
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    z = np.load(out)
    return tuple(z[k] for k in (("t", "prim", "any") if what == "trace" else ("eye", "light")))


def _main(argv):
    what, name, lm, inp, out = argv[1], argv[2], int(argv[3]), argv[4], argv[5]
    sc = scene(name)
    if what == "trace":
        rays = np.load(inp)
        t, p = core_trace(sc, lm, rays)
        _, pa = core_trace(sc, lm, rays, any_hit=True)
        np.savez(out, t=t, prim=p, any=pa >= 0)
    else:
        from test_core_cpu import core_render
        eye, light, _ = core_render(sc, FRAME[0], FRAME[1], 1, 5, seed=3, lds_mode=lm)
        np.savez(out, eye=eye, light=light)
    return 0


if __name__ == "__main__":
    sys.exit(_main(sys.argv))
