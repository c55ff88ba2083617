"""GPU side of tests/test_ray_queries.py: the same generated scenes, ray sets and references
(tests/_rayref.py) through bdpt_trace_rays (k_trace_rays: the 4-wide tree in HBM, LDS mode 0) —
closest hits bit-equal to oracle mode 2, no wrong primitive against brute_fp64 among the rays it
decides, any-hit agreeing with closest-hit, also for finite [tmin, tmax] windows and odd rays — and
the scenes whose device tree is a single leaf through k_trace_rays, k_bdpt_sample in every LDS mode
and k_pt. Each case is one small context and at most 4000 rays or a 16x12 frame."""
import os

import numpy as np
import pytest

import _rayref as R
import bdpt_amd as B
import test_ray_queries as Q
from _util import MODE_C32, REPO, oracle_pt_render, oracle_render

pytestmark = pytest.mark.gpu

RMSE_TOL = 1e-4   # the suite's frame tolerance (tests/test_gpu_parity.py)


class Tracer:
    """One context on a scene; trace(rays, any_hit) -> (t, prim)."""

    def __init__(self, sc):
        self.pt = B.BidirectionalPathTracer(sc, R.FRAME[0], R.FRAME[1], 1, 5)

    def __call__(self, rays, any_hit=False):
        return self.pt.trace_rays(rays, any_hit=any_hit)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.pt.close()


@pytest.fixture(autouse=True)
def _default_modes(monkeypatch):
    for k in ("BDPT_LDS_MODE", "BDPT_NTOP_MAX", "BDPT_BVH", "BDPT_SBVH", "BDPT_SBVH_BUDGET"):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("name", Q.CASES)
def test_closest_and_any_hit(name):
    """Case (a); tiny1, tiny2 and tiny_sphere are the trees whose root is a leaf."""
    r = Q.ref(name)
    with Tracer(r["sc"]) as trace:
        t, p = trace(r["rays"])
        _, pa = trace(r["rays"], True)
    Q.check_against_references(name, t, p, pa >= 0)


@pytest.mark.parametrize("name", [c for c in Q.CASES if c not in R.ORACLE_REFUSES])
def test_windows_at_the_hit(name):
    with Tracer(Q.ref(name)["sc"]) as trace:
        Q.check_windows(name, trace)


def test_windows_between_layers():
    with Tracer(Q.ref("stack")["sc"]) as trace:
        Q.check_stack_windows(trace)


def test_odd_rays():
    sets = Q.odd_ray_sets()
    with Tracer(R.scene("odd")) as trace:
        out = {kind: (trace(rays), trace(rays, True)) for kind, rays in sets.items()}
    for kind, ((t, p), (_, pa)) in out.items():
        Q.check_odd(kind, sets[kind], t, p, pa >= 0)


def test_nan_origins_on_a_deep_tree():
    """256 rays with a NaN origin on CBbunny: no hit, as the oracle says. Their any-hit queries enter
    every child of every node (fmaxf / fminf drop the NaN plane distances): the deepest the stack
    gets (tests/native/stack_probe.cpp has the counters and the sanitizers, on the CPU)."""
    sc = B.load_dae(os.path.join(REPO, "scenes", "CBbunny.dae"), *R.FRAME)
    rays = R.nan_origin_rays(256)
    with Tracer(sc) as trace:
        t, p = trace(rays)
        _, pa = trace(rays, True)
    ot, op = R.oracle_trace(sc, rays)
    assert (op < 0).all()
    assert np.array_equal(p, op) and np.isinf(t).all() and (pa < 0).all()


def _rmse(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))


_renders = {}


def _oracle_frame(rname):
    if rname not in _renders:
        W, H = R.FRAME
        _renders[rname] = oracle_render(R.scene(rname), W, H, 1, 5, MODE_C32)
    return _renders[rname]


# BDPT_LDS_MODE -> the mode lds_plan (bdpt_ldsplan.h) runs a one-leaf scene in: unset = the flat
# list (<= 24 primitives); a forced 2 has no binary nodes to stage and falls to 0
LEAF_ROOT_MODES = [(None, 3), ("0", 0), ("1", 1), ("2", 0), ("3", 3)]


@pytest.mark.parametrize("lds,ran", LEAF_ROOT_MODES, ids=[f"lds_{m[0]}" for m in LEAF_ROOT_MODES])
@pytest.mark.parametrize("rname", [r for _, r in Q.LEAF_ROOTS])
def test_leaf_root_renders(rname, lds, ran, monkeypatch):
    W, H = R.FRAME
    if lds is not None:
        monkeypatch.setenv("BDPT_LDS_MODE", lds)
    pt = B.BidirectionalPathTracer(R.scene(rname), W, H, 1, 5, seed=5489, collect_stats=True)
    try:
        pt.raytrace_tiles([], 0, 1)
        g = {k: pt.read_frame(v).astype(np.float64)
             for k, v in (("sample", B.FRAME_SAMPLE), ("eye", B.FRAME_EYE), ("light", B.FRAME_LIGHT))}
        st = pt.stats()
    finally:
        pt.close()
    assert st.lds_mode == ran
    samp, eye, light, _ = _oracle_frame(rname)
    assert samp.mean() > 0 and np.isfinite(g["sample"]).all()
    r, re_, rl = _rmse(g["sample"], samp), _rmse(g["eye"], eye), _rmse(g["light"], light)
    print(f"{rname} BDPT_LDS_MODE={lds} (ran {st.lds_mode}): rmse sample {r:.3e} eye {re_:.3e} light {rl:.3e}")
    assert r < RMSE_TOL and re_ < RMSE_TOL and rl < RMSE_TOL


def test_leaf_root_pathtracer(monkeypatch):
    """Two triangles under the unidirectional PathTracer with the 4-wide tree forced (k_pt<LM 0>)."""
    W, H, S, M = R.FRAME[0], R.FRAME[1], 4, 5
    monkeypatch.setenv("BDPT_LDS_MODE", "0")
    sc = R.scene("render2")
    pt = B.PathTracer(sc, W, H, S, M, seed=31, samples_per_batch=4, collect_stats=True)
    try:
        pt.raytrace_tiles()
        img = pt.read_frame(B.FRAME_SAMPLE).astype(np.float64)
        cnt = pt.read_sample_counts()
        st = pt.stats()
    finally:
        pt.close()
    assert st.lds_mode == 0
    o_img, o_cnt, _ = oracle_pt_render(sc, W, H, S, M, MODE_C32, seed=31, batch=4)
    assert o_img.mean() > 0 and np.isfinite(img).all()
    r, mism = _rmse(img, o_img), float(np.mean(cnt != o_cnt))
    print(f"PT render2 LM 0: rmse {r:.3e} count mismatch {mism:.4f}")
    assert mism <= 0.01 and r < RMSE_TOL
