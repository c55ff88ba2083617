"""CPU checks of the device tree after the reinsertion passes (bdpt_scene.cpp reinsert_optimise):
the flattened trees are valid and cheaper by the SAH than the top-down build's, BDPT_BVH=sah still
gives the tree from before the passes existed, renders stay bit-exact against oracle mode 2 and
closest hits equal brute force on every combination of {reinsertion, spatial splits}, degenerate
inputs build, and a tree too deep for the traversal stack falls back instead of failing.
tests/native/tree_check.cpp (compiled here with g++) inspects the trees."""
import ctypes as C
import glob
import os
import subprocess
import time

import numpy as np
import pytest

import bdpt_amd as B
from _util import MODE_C32, REPO, golden_scene, oracle_render
from test_core_cpu import core, core_render

CSRC = os.path.join(REPO, "bidirectional-pathtracing_amd", "csrc")
UNSUPPORTED = -2   # BDPT_E_UNSUPPORTED (include/bdpt/bdpt.h)

# BDPT_BVH=sah: (binary nodes, binary depth, primitive references) of the commit before the
# reinsertion passes, recorded there with this file's helper (spatial splits at their defaults of
# then: alpha 1e-5, budget 0.3)
PARENT_TREE = {"CBbunny": (34733, 19, 29250), "CBgems": (303, 10, 252)}
PARENT_SBVH = {"BDPT_SBVH": "1e-5", "BDPT_SBVH_BUDGET": "0.3"}

TREES = [pytest.param({}, id="default"), pytest.param({"BDPT_BVH": "sah"}, id="sah")]
SPLITS = [pytest.param({"BDPT_SBVH": "0"}, id="nosplit"), pytest.param({"BDPT_SBVH": "1e-5"}, id="split")]

_libs = {}


def checker(tmp_path_factory, stack_max=None):
    """tests/native/tree_check.cpp + bdpt_scene.cpp as a shared library, optionally with another
    traversal stack limit (-DBDPT_STACK_MAX)."""
    if stack_max not in _libs:
        so = str(tmp_path_factory.mktemp("tree_check") / "libtreecheck.so")
        cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-I" + os.path.join(REPO, "include"),
               "-I" + CSRC, "-o", so, os.path.join(REPO, "tests", "native", "tree_check.cpp"),
               os.path.join(CSRC, "bdpt_scene.cpp")]
        if stack_max is not None:
            cmd.insert(1, f"-DBDPT_STACK_MAX={stack_max}")
        subprocess.run(cmd, check=True)
        lib = C.CDLL(so)
        lib.tree_check.argtypes = [C.POINTER(B.SceneDesc), C.POINTER(C.c_int), C.POINTER(C.c_double)]
        _libs[stack_max] = lib
    return _libs[stack_max]


def tree_of(lib, sc):
    info = (C.c_int * 8)()
    sah = C.c_double()
    d = sc.desc()
    rc = lib.tree_check(C.byref(d), info, C.byref(sah))
    keys = ("nodes", "depth", "refs", "valid", "depth2", "depth4", "stack_need", "stack_max")
    return rc, dict(zip(keys, info), sah=sah.value)


def dae(name, W=32, H=24):
    return B.load_dae(os.path.join(REPO, "scenes", name + ".dae"), W, H)


def set_env(monkeypatch, *envs):
    for k in ("BDPT_BVH", "BDPT_SBVH", "BDPT_SBVH_BUDGET"):
        monkeypatch.delenv(k, raising=False)
    for env in envs:
        for k, v in env.items():
            monkeypatch.setenv(k, v)


@pytest.mark.parametrize("name", ["CBbunny", "CBgems"])
def test_valid_and_cheaper_than_top_down(name, tmp_path_factory, monkeypatch):
    lib = checker(tmp_path_factory)
    sc = dae(name)
    set_env(monkeypatch)
    rc, new = tree_of(lib, sc)
    set_env(monkeypatch, {"BDPT_BVH": "sah"})
    rc0, old = tree_of(lib, sc)
    print(name, "default", new, "BDPT_BVH=sah", old)
    assert rc == 0 and rc0 == 0
    assert new["valid"] == 1 and old["valid"] == 1
    assert new["sah"] < old["sah"]
    for split in ({"BDPT_SBVH": "0"}, {"BDPT_SBVH": "1e-5"}):
        set_env(monkeypatch, split)
        rc, a = tree_of(lib, sc)
        set_env(monkeypatch, split, {"BDPT_BVH": "sah"})
        rc0, b = tree_of(lib, sc)
        assert rc == 0 and rc0 == 0 and a["valid"] == 1 and b["valid"] == 1
        assert a["sah"] < b["sah"], (split, a, b)
        assert a["refs"] == b["refs"]   # the passes move subtrees; they add or drop no reference


def test_every_quick_scene_valid_and_not_costlier(tmp_path_factory, monkeypatch):
    """Every scene under scenes/ that loads in under a second."""
    lib = checker(tmp_path_factory)
    seen = 0
    for path in sorted(glob.glob(os.path.join(REPO, "scenes", "*.dae"))):
        t0 = time.time()
        try:
            sc = B.load_dae(path, 32, 24)
        except B.BDPTError:
            continue
        if time.time() - t0 >= 1.0:
            continue
        set_env(monkeypatch)
        rc, new = tree_of(lib, sc)
        set_env(monkeypatch, {"BDPT_BVH": "sah"})
        rc0, old = tree_of(lib, sc)
        assert rc == rc0, path
        if rc != 0:
            continue   # a scene the BDPT integrator does not take (its materials or lights)
        seen += 1
        assert new["valid"] == 1 and old["valid"] == 1, path
        assert new["sah"] <= old["sah"], (path, new, old)
    assert seen >= 5


@pytest.mark.parametrize("name", ["CBbunny", "CBgems"])
def test_bvh_sah_is_the_tree_from_before(name, tmp_path_factory, monkeypatch):
    lib = checker(tmp_path_factory)
    set_env(monkeypatch, {"BDPT_BVH": "sah"}, PARENT_SBVH)
    rc, t = tree_of(lib, dae(name))
    assert rc == 0
    assert (t["nodes"], t["depth"], t["refs"]) == PARENT_TREE[name]


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("scene,W,H,spp,M", [("CBgems", 32, 24, 1, 7), ("CBbunny", 40, 30, 1, 5)])
def test_trees_bit_exact(scene, W, H, spp, M, tree, split, monkeypatch):
    """The shapes of test_device_tree_knobs_bit_exact, in LDS modes 0 (4-wide tree) and 1 (binary)."""
    set_env(monkeypatch, tree, split)
    sc = dae(scene, W, H)
    _, oeye, olight, _ = oracle_render(sc, W, H, spp, M, MODE_C32, seed=5, threads=1)
    for lm in (0, 1):
        eye, light, _ = core_render(sc, W, H, spp, M, seed=5, lds_mode=lm)
        assert np.array_equal(eye, oeye) and np.array_equal(light, olight), (tree, split, lm)


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("tree", TREES)
def test_closest_hits_match_brute_force(tree, split, monkeypatch):
    """core_cpu_trace_check: closest hits of rays with zero direction components through the tree
    against a loop over every primitive, on CBbunny."""
    set_env(monkeypatch, tree, split)
    lib = core()
    lib.core_cpu_trace_check.argtypes = [C.POINTER(B.SceneDesc), C.c_int, C.c_int, C.c_uint64, C.POINTER(C.c_int)]
    sc = dae("CBbunny")
    for lm in (0, 1, 2):
        hits = C.c_int()
        assert lib.core_cpu_trace_check(C.byref(sc.desc()), lm, 1400, 12345, C.byref(hits)) == 0, lm
        assert hits.value > 500


def _with_prims(base, geom, mat):
    """base's materials, light and camera around the triangles `geom` (n, 18) of materials `mat`."""
    n = len(geom)
    return B.Scene(np.zeros(n, np.int32), np.asarray(geom, np.float64), np.asarray(mat, np.int32),
                   [base.mats[i] for i in range(base.nmat)], [base.lights[i] for i in range(base.nlight)],
                   base.camera, base.width, base.height)


def _degenerate(kind):
    """(scene, the scene the oracle renders, LDS modes). The triangles are CBempty's last ones
    (its back wall first), which this small frame's camera sees and the light reaches."""
    W, H = 16, 12
    base = golden_scene("CBempty", W, H)
    tris = base.prim_geom[base.prim_type == 0]
    tris, mats = tris[::-1], base.prim_mat[base.prim_type == 0][::-1]
    if kind == "CBspheres":   # 14 primitives: the product renders it from the flat list (mode 3)
        sc = golden_scene("CBspheres", W, H)
        return sc, sc, (0, 1)
    if kind == "same64":
        # the oracle (like the reference) refuses primitives without extent between their
        # centroids; 64 copies of one triangle render what the one triangle renders: the same t,
        # normal and material whichever copy is hit
        return (_with_prims(base, np.repeat(tris[:1], 64, axis=0), np.repeat(mats[:1], 64)),
                _with_prims(base, tris[:1], mats[:1]), (0, 1))
    # A tree whose root is a leaf (1 or 2 triangles): the 4-wide tree wraps the leaf in a one-slot
    # root node (emit_device_tree), so every mode renders it: the 4-wide tree with and without its
    # treelet (0, 2), the binary tree (1) and the flat list (3). Started on a bare leaf reference
    # the 4-wide traversal did not terminate; bdpt_trace_rays and BDPT_LDS_MODE=0 / 2 reach it.
    sc = _with_prims(base, tris[:int(kind)], mats[:int(kind)])
    return sc, sc, (0, 1, 2, 3) if int(kind) < 3 else (0, 1, 3)


@pytest.mark.parametrize("kind", ["1", "2", "3", "same64", "CBspheres"])
def test_degenerate_inputs(kind, tmp_path_factory, monkeypatch):
    """1, 2 and 3 triangles, 64 identical ones (coincident centroids) and CBspheres forced through
    the 4-wide and the binary tree (LDS modes 0 and 1)."""
    set_env(monkeypatch)
    W, H = 16, 12
    sc, osc, modes = _degenerate(kind)
    rc, t = tree_of(checker(tmp_path_factory), sc)
    assert rc == 0 and t["valid"] == 1, t
    _, oeye, olight, _ = oracle_render(osc, W, H, 1, 5, MODE_C32, seed=3, threads=1)
    assert oeye.mean() + olight.mean() > 0
    for lm in modes:
        eye, light, _ = core_render(sc, W, H, 1, 5, seed=3, lds_mode=lm)
        assert np.array_equal(eye, oeye) and np.array_equal(light, olight), (kind, lm)


def test_too_deep_tree_falls_back(tmp_path_factory, monkeypatch):
    """With the traversal stack limit just below what the optimised CBbunny tree needs the build
    succeeds through a fallback (the tree without the passes, then without spatial splits); below
    what any tree needs it is BDPT_E_UNSUPPORTED."""
    sc = dae("CBbunny")
    set_env(monkeypatch)
    rc, t = tree_of(checker(tmp_path_factory), sc)
    assert rc == 0
    need = t["stack_need"]
    rc, f = tree_of(checker(tmp_path_factory, need - 1), sc)
    print("optimised", t, "fallback", f)
    assert rc == 0 and f["valid"] == 1
    assert f["stack_need"] < need and f["stack_max"] == need - 1
    rc, _ = tree_of(checker(tmp_path_factory, 8), sc)
    assert rc == UNSUPPORTED
