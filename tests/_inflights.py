"""Helpers of the infinite-light tests (tests/test_inflights.py, tests/test_gpu_inflights.py): the
CPU build of the device code with the bdpt_params.infinite_lights opt-in
(tests/native/core_cpu_inf.cpp -> libcorecpu_inf.so) and the fixtures of tests/golden/inflights/."""
import ctypes as C
import os

import numpy as np

import bdpt_amd as B
from _util import REPO

GOLD = os.path.join(REPO, "tests", "golden", "inflights")

_lib = None


def core_inf():
    global _lib
    if _lib is None:
        import sys
        sys.path.insert(0, REPO)
        import __graft_entry__ as g
        g.build_core_cpu_inf()
        lib = C.CDLL(g.CORE_CPU_INF_SO)
        P = C.POINTER(C.c_double)
        lib.core_cpu_inf_render.argtypes = [C.POINTER(B.SceneDesc), C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int,
                                            P, P, P, C.c_int, C.c_int, C.c_int, C.c_int]
        lib.core_cpu_inf_scene_check.argtypes = [C.POINTER(B.SceneDesc), C.c_int, C.c_int, C.c_char_p, C.c_int,
                                                 C.POINTER(C.c_int), C.POINTER(C.c_int)]
        _lib = lib
    return _lib


def inf_render(scene, W, H, spp, M, seed=5489, s0=0, count=None, pixels=None, lds_mode=0, rr=False,
               infinite_lights=True, threads=1):
    """(eye, light, stats): float64 frames (H, W, 3), row 0 = bottom; stats[7] = kernel flavour,
    stats[8] / [9] = number / magnitude of the s = 0 contributions. threads = 1 sums the light
    image in core_cpu_render's order."""
    count = spp - s0 if count is None else count
    eye = np.zeros((H, W, 3))
    light = np.zeros((H, W, 3))
    st = np.zeros(10)
    d = scene.desc()
    pd = C.POINTER(C.c_double)
    px, npx = None, 0
    if pixels is not None:
        px = np.ascontiguousarray(pixels, dtype=np.int32).reshape(-1, 2)
        npx = px.shape[0]
    rc = core_inf().core_cpu_inf_render(C.byref(d), W, H, spp, M, seed, s0, count,
                                        px.ctypes.data_as(C.POINTER(C.c_int)) if px is not None else None, npx,
                                        eye.ctypes.data_as(pd), light.ctypes.data_as(pd), st.ctypes.data_as(pd),
                                        lds_mode, 1 if rr else 0, 1 if infinite_lights else 0, threads)
    assert rc == 0, rc
    return eye, light, st


def scene_check(scene, infinite_lights, rr=False):
    """bdpt_create's scene checks under BDPT, without a device: (status, message, flavour, esc_light)."""
    msg = C.create_string_buffer(512)
    fl, esc = C.c_int(-1), C.c_int(-1)
    d = scene.desc()
    rc = core_inf().core_cpu_inf_scene_check(C.byref(d), 1 if infinite_lights else 0, 1 if rr else 0, msg, 512,
                                             C.byref(fl), C.byref(esc))
    return rc, msg.value.decode(), fl.value, esc.value


def fixture_scene(key, W, H):
    """tests/golden/inflights/CBspheres_<key>.dae (hemi, dir, mixed) at W x H"""
    return B.load_dae(os.path.join(GOLD, "CBspheres_%s.dae" % key), W, H)


def threads():
    return min(16, os.cpu_count() or 1)
