"""Helpers of the thin-lens tests (tests/test_lens.py, tests/test_gpu_lens.py): the CPU build of the
device code at the thin-lens flavour (tests/native/core_cpu_lens.cpp -> libcorecpu_lens.so,
DESIGN.md §9b) and the fixtures of tests/golden/lens/."""
import ctypes as C
import os

import numpy as np

import bdpt_amd as B
from _util import REPO

GOLD = os.path.join(REPO, "tests", "golden", "lens")
LENS, FOCAL = 0.5, 2.5   # the fixtures' -b / -d

_lib = None


def core_lens():
    global _lib
    if _lib is None:
        import sys
        sys.path.insert(0, REPO)
        import __graft_entry__ as g
        g.build_core_cpu_lens()
        lib = C.CDLL(g.CORE_CPU_LENS_SO)
        P, F, I = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int)
        D = C.POINTER(B.SceneDesc)
        lib.core_cpu_lens_render.argtypes = [D, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int, C.c_int,
                                             I, C.c_int, P, P, P, C.c_int, C.c_int, C.c_int, C.c_int,
                                             C.c_double, C.c_double]
        lib.core_cpu_lens_flavour.argtypes = [D, C.c_int, C.c_int, C.c_double, I]
        lib.core_cpu_lens_eye_rays.argtypes = [D, C.c_double, C.c_double, C.c_int, F, F, F, F]
        lib.core_cpu_lens_camera_samples.argtypes = [D, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, F, F, I, F]
        _lib = lib
    return _lib


def lens_render(scene, W, H, spp, M, seed=5489, s0=0, count=None, lds_mode=0, rr=False, infinite_lights=True,
                threads=1, lens_radius=LENS, focal_distance=FOCAL):
    """(eye, light, stats): float64 frames (H, W, 3), row 0 = bottom; stats[7] = the kernel flavour
    that rendered (3 with lens_radius > 0). threads = 1 sums the light image in core_cpu_render's order."""
    count = spp - s0 if count is None else count
    eye = np.zeros((H, W, 3))
    light = np.zeros((H, W, 3))
    st = np.zeros(10)
    d = scene.desc()
    pd = C.POINTER(C.c_double)
    rc = core_lens().core_cpu_lens_render(C.byref(d), W, H, spp, M, seed, s0, count, None, 0,
                                          eye.ctypes.data_as(pd), light.ctypes.data_as(pd), st.ctypes.data_as(pd),
                                          lds_mode, 1 if rr else 0, 1 if infinite_lights else 0, threads,
                                          lens_radius, focal_distance)
    assert rc == 0, rc
    return eye, light, st


def flavour(scene, infinite_lights, rr, lens_radius):
    """bdpt_create's kernel flavour for these settings, without a device"""
    fl = C.c_int(-1)
    d = scene.desc()
    rc = core_lens().core_cpu_lens_flavour(C.byref(d), 1 if infinite_lights else 0, 1 if rr else 0, lens_radius,
                                           C.byref(fl))
    assert rc == 0, rc
    return fl.value


def _f(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def eye_rays(scene, lens_radius, focal_distance, u, xy):
    """Eye rays (origin, dir) of raster positions xy in [0, 1]^2 from the lens points of uniforms u"""
    u = np.ascontiguousarray(u, dtype=np.float32)
    xy = np.ascontiguousarray(xy, dtype=np.float32)
    n = len(u)
    o, dr = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    d = scene.desc()
    rc = core_lens().core_cpu_lens_eye_rays(C.byref(d), lens_radius, focal_distance, n, _f(u), _f(xy), _f(o), _f(dr))
    assert rc == 0, rc
    return o, dr


def camera_samples(scene, lens_radius, focal_distance, W, H, u, p):
    """The camera sampler from the lens points of uniforms u toward the points p: (pixel, e.pos)"""
    u = np.ascontiguousarray(u, dtype=np.float32)
    p = np.ascontiguousarray(p, dtype=np.float32)
    n = len(u)
    pix, pos = np.zeros((n, 2), np.int32), np.zeros((n, 3), np.float32)
    d = scene.desc()
    rc = core_lens().core_cpu_lens_camera_samples(C.byref(d), lens_radius, focal_distance, W, H, n, _f(u), _f(p),
                                                  pix.ctypes.data_as(C.POINTER(C.c_int)), _f(pos))
    assert rc == 0, rc
    return pix, pos
