"""GPU: the infinite-light kernels (k_bdpt_sample's third flavour, bdpt_params.infinite_lights,
DESIGN.md §9a) against the CPU build of the same device headers (tests/native/core_cpu_inf.cpp) at
the same seed, the route tests/test_core_cpu.py gives the other flavours; the oracle does not know
these lights. Tolerance: the project's mode-2 one, per-pixel RMSE < 1e-4 (the two differ by the
order of the fp32 additions into the frames). Semantics: tests/test_inflights.py (CPU)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import bdpt_amd as B
from _inflights import fixture_scene, inf_render, threads
from _util import REPO
from test_output_stage import CLI, read_png

pytestmark = pytest.mark.gpu

RMSE_TOL = 1e-4


def _scene(key, W, H):
    if key == "bunny":
        return B.load_dae(os.path.join(REPO, "scenes", "bunny.dae"), W, H)
    return fixture_scene(key, W, H)


def _gpu_render(sc, W, H, S, M, seed=5489, rr=False, tiles=(), ranges=None, stats=False):
    pt = B.BidirectionalPathTracer(sc, W, H, S, M, seed=seed, russian_roulette=rr, infinite_lights=True,
                                   collect_stats=stats)
    try:
        for a, b in (ranges or [(0, S)]):
            pt.raytrace_tiles(list(tiles), a, b - a)
        out = {k: pt.read_frame(v).astype(np.float64) for k, v in (("eye", B.FRAME_EYE), ("light", B.FRAME_LIGHT))}
        out["stats"] = pt.stats()
        return out
    finally:
        pt.close()


@functools.lru_cache(maxsize=None)
def _cpu_render(key, W, H, S, M, rr):
    """computed once per case and shared (the LDS-mode cases compare with one render)"""
    eye, light, st = inf_render(_scene(key, W, H), W, H, S, M, seed=5489, rr=rr, threads=threads())
    assert st[7] == 2   # the infinite-light flavour, as bdpt_create chooses
    return eye, light


def _rmse(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))


CASES = [
    ("hemi", 32, 24, 2, 5, False, None),
    ("dir", 32, 24, 2, 5, False, None),
    ("mixed", 32, 24, 2, 5, False, None),
    ("hemi", 32, 24, 2, 8, True, None),    # a second MAXV class, roulette: 13-dword vertices
    ("dir", 32, 24, 2, 1, False, None),    # the shortest paths: only (2, 1) and the light image
    ("mixed", 32, 24, 2, 5, False, "0"), ("mixed", 32, 24, 2, 5, False, "1"),
    ("mixed", 32, 24, 2, 5, False, "2"), ("mixed", 32, 24, 2, 5, False, "3"),   # every LDS mode
    ("bunny", 64, 48, 1, 5, False, None),  # 28k triangles: the treelet path
]


@pytest.mark.parametrize("key,W,H,S,M,rr,lds", CASES)
def test_gpu_matches_cpu_build(key, W, H, S, M, rr, lds, monkeypatch):
    if lds is not None:
        monkeypatch.setenv("BDPT_LDS_MODE", lds)
    g = _gpu_render(_scene(key, W, H), W, H, S, M, rr=rr)
    eye, light = _cpu_render(key, W, H, S, M, rr)
    assert np.isfinite(g["eye"]).all() and np.isfinite(g["light"]).all()
    re_, rl = _rmse(g["eye"], eye), _rmse(g["light"], light)
    print(f"{key} {W}x{H} s{S} m{M} rr {rr} lds {lds}: rmse eye {re_:.3e} light {rl:.3e} "
          f"mean gpu {g['eye'].mean():.6f} + {g['light'].mean():.6f} cpu {eye.mean():.6f} + {light.mean():.6f}")
    assert eye.mean() > 0   # (at these frame sizes few t = 1 splats land: the light image may be all zero)
    assert re_ < RMSE_TOL and rl < RMSE_TOL
    if lds is not None:
        assert g["stats"].lds_mode == int(lds)
    if key == "bunny":
        assert g["stats"].lds_mode == 2


def test_tiles_and_sample_ranges_compose():
    """Two sample ranges over two tiles sum to the whole-frame render (the tolerance of
    test_gpu_parity.py::test_tiles_and_sample_ranges_compose)."""
    W, H, S, M = 32, 24, 2, 5
    sc = _scene("hemi", W, H)
    full = _gpu_render(sc, W, H, S, M)
    tiled = _gpu_render(sc, W, H, S, M, tiles=[(0, 0, 16, H), (16, 0, 16, H)], ranges=[(0, 1), (1, 2)])
    assert _rmse(full["eye"] + full["light"], tiled["eye"] + tiled["light"]) < 1e-6


def test_cli_flag(tmp_path):
    """pathtracer --infinite-lights renders the directional-lit teapot.dae under BDPT; without the
    flag the CLI fails and its message names the flag and --pt."""
    out = tmp_path / "teapot.png"
    args = ["-s", "2", "-m", "5", "-r", "64", "48", "-f", str(out), os.path.join(REPO, "scenes", "teapot.dae")]
    r = subprocess.run([CLI, "--infinite-lights"] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    img = read_png(out)
    assert img.shape == (48, 64, 4) and img[..., :3].max() > 0
    os.remove(out)
    r = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "--infinite-lights" in r.stderr and "--pt" in r.stderr
    assert not os.path.exists(out)
