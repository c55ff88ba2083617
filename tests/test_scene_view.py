"""The one place that turns a HostScene into a SceneView (csrc/bdpt_scene.h scene_view) and the host
view the CPU yardstick builds put over it (tests/native/core_cpu_host.h host_view): the tree a mode
traverses, the layout of HostScene::env behind the environment pointers, the light an escaped ray
reaches, and which "LDS copies" each mode reads. bdpt_ctx.h view_of is scene_view over the device
pointers, so what is pinned here is what the kernels are handed. CPU only."""
import ctypes as C

import numpy as np
import pytest

import bdpt_amd as B
from _inflights import fixture_scene
from _pixelbound import lds_facts
from _util import golden_scene
from test_core_cpu import core

W, H = 16, 12
LM_WIDTH = {0: 4, 1: 2, 2: 4, 3: 2}   # bdpt_bvh.h lm_width: kBvhWidth for LM 0 / 2, kLdsBvhWidth for LM 1 / 3
ENV_NAMES = ("marg", "cond", "pdf", "rgb", "gmarg", "gcond")


def view_facts(scene, infinite_lights, lds_mode):
    lib = core()
    lib.core_cpu_view_facts.argtypes = [C.POINTER(B.SceneDesc), C.c_int, C.c_int, C.POINTER(C.c_int)]
    out = (C.c_int * 19)()
    d = scene.desc()
    assert lib.core_cpu_view_facts(C.byref(d), 1 if infinite_lights else 0, lds_mode, out) == 0
    v = list(out)
    f = dict(zip(("tree", "root", "ntop", "nleaves", "fn", "env_light"), v[:6]))
    f["env"] = dict(zip(ENV_NAMES, v[6:12]))
    f["lnodes"], f["lgeom"], f["lshade"] = (bool(x) for x in v[12:15])
    f["lm_width"], f["hs_root"], f["hs_ntop"], f["hs_nleaves"] = v[15:19]
    return f


def _plain():
    sc = golden_scene("CBspheres", W, H)
    return sc, False, -1, dict.fromkeys(ENV_NAMES, -1)


def _mapped():
    sc = golden_scene("CBspheres", W, H)
    rgb = np.linspace(0.1, 2.0, 4 * 2 * 3, dtype=np.float32).reshape(2, 4, 3)   # w = 4, h = 2
    sc.set_envmap(rgb)
    # h = 2 rows, np = 8 texels, gm = 2 guide cells: marg[h] | cond[np] | pdf[np] | rgb[3 np] | gmarg[gm + 1] | gcond
    off = dict(zip(ENV_NAMES, (0, 2, 10, 18, 42, 45)))
    return sc, False, sc.nlight, off   # the environment light is appended after the scene's own


def _hemi():
    sc = fixture_scene("hemi", W, H)
    hemi = [i for i in range(sc.nlight) if sc.lights[i].type == B.LIGHT_HEMISPHERE]
    assert len(hemi) == 1
    return sc, True, hemi[0], dict.fromkeys(ENV_NAMES, -1)


@pytest.mark.parametrize("make", [_plain, _mapped, _hemi])
def test_scene_view_facts(make):
    sc, inf, esc_light, env_off = make()
    facts = lds_facts(sc, infinite_lights=inf)
    for lm in range(4):
        f = view_facts(sc, inf, lm)
        label = (make.__name__, lm)
        assert f["lm_width"] == LM_WIDTH[lm], label
        assert f["tree"] == LM_WIDTH[lm], label
        assert f["root"] == f["hs_root"], label
        assert f["hs_ntop"] == facts["n_top"] > 0, label
        assert f["ntop"] == (facts["n_top"] if lm == 2 else 0), label
        assert f["nleaves"] == f["hs_nleaves"] > 0, label
        assert f["fn"] == facts["flat_n"], label
        assert f["env_light"] == esc_light, label
        assert f["env"] == env_off, label
        assert (f["lnodes"], f["lgeom"], f["lshade"]) == (lm in (1, 2), lm in (1, 3), lm == 3), label
