"""GPU checks of the device tree after the reinsertion passes (bdpt_scene.cpp reinsert_optimise):
the default tree and BDPT_BVH=sah (the top-down SAH tree without them) render the same frames as
oracle mode 2, also where the re-ordered nodes straddle the LDS treelet, and find the same closest
hits. The CPU side is tests/test_bvh_reinsert.py."""
import os

import numpy as np
import pytest

import bdpt_amd as B
from _util import MODE_C32, REPO, golden_scene, oracle_render

pytestmark = pytest.mark.gpu

RMSE_TOL = 1e-4   # the suite's frame tolerance (tests/test_gpu_parity.py)

_refs = {}


def _scene(name, W, H):
    if name == "CBbunny":
        return B.load_dae(os.path.join(REPO, "scenes", "CBbunny.dae"), W, H)
    return golden_scene(name, W, H)


def _oracle(name, W, H, S, M):
    """One oracle render per shape, shared by the cases and left unchanged."""
    key = (name, W, H, S, M)
    if key not in _refs:
        _refs[key] = oracle_render(_scene(name, W, H), W, H, S, M, MODE_C32)
    return _refs[key]


def _rmse(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))


@pytest.mark.parametrize("bvh", [None, "sah"], ids=["default", "sah"])
@pytest.mark.parametrize("name,M,lds,ntop", [("CBbunny", 5, "0", None), ("CBbunny", 5, "2", None),
                                             ("CBbunny", 5, "0", "5"), ("CBbunny", 5, "2", "5"),
                                             ("CBgems", 7, "1", None)])
def test_parity_vs_oracle(name, M, lds, ntop, bvh, monkeypatch):
    W, H, S = 64, 48, 1
    monkeypatch.setenv("BDPT_LDS_MODE", lds)
    if ntop:
        monkeypatch.setenv("BDPT_NTOP_MAX", ntop)
    if bvh:
        monkeypatch.setenv("BDPT_BVH", bvh)
    else:
        monkeypatch.delenv("BDPT_BVH", raising=False)
    sc = _scene(name, W, H)
    pt = B.BidirectionalPathTracer(sc, W, H, S, M, seed=5489, collect_stats=True)
    try:
        pt.raytrace_tiles([], 0, S)
        g = {k: pt.read_frame(v).astype(np.float64)
             for k, v in (("sample", B.FRAME_SAMPLE), ("eye", B.FRAME_EYE), ("light", B.FRAME_LIGHT))}
        st = pt.stats()
    finally:
        pt.close()
    assert st.lds_mode == int(lds)
    samp, eye, light, _ = _oracle(name, W, H, S, M)
    assert np.isfinite(g["sample"]).all()
    r, re_, rl = _rmse(g["sample"], samp), _rmse(g["eye"], eye), _rmse(g["light"], light)
    print(f"{name} LM {lds} ntop {ntop} BDPT_BVH={bvh}: rmse sample {r:.3e} eye {re_:.3e} light {rl:.3e}")
    assert samp.mean() > 0
    assert r < RMSE_TOL and re_ < RMSE_TOL and rl < RMSE_TOL


def test_traced_rays_equal_between_trees(monkeypatch):
    """bdpt_trace_rays' closest hits (primitive key and t) over 20,000 random rays on CBbunny are
    bit-equal between the default tree and BDPT_BVH=sah."""
    sc = _scene("CBbunny", 64, 48)
    rng = np.random.default_rng(7)
    n = 20000
    o = rng.uniform(-0.9, 0.9, (n, 3)).astype(np.float32)
    o[:, 1] = rng.uniform(0.05, 1.4, n)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([o, d, np.full((n, 1), 1e-5, np.float32),
                           np.full((n, 1), np.inf, np.float32)], axis=1).astype(np.float32)
    out = {}
    for bvh in (None, "sah"):
        if bvh:
            monkeypatch.setenv("BDPT_BVH", bvh)
        else:
            monkeypatch.delenv("BDPT_BVH", raising=False)
        pt = B.BidirectionalPathTracer(sc, 64, 48, 1, 5)
        try:
            out[bvh] = pt.trace_rays(rays, any_hit=False)
        finally:
            pt.close()
    (t0, p0), (t1, p1) = out[None], out["sah"]
    assert (p0 >= 0).sum() > n // 2
    assert np.array_equal(p0, p1)
    assert np.array_equal(t0[p0 >= 0], t1[p0 >= 0])
