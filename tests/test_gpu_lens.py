"""GPU: the thin-lens kernels (k_bdpt_sample's flavour 3, bdpt_params.lens_radius > 0)
against the CPU build of the same device headers (tests/native/core_cpu_lens.cpp) at the same seed,
the route tests/test_gpu_inflights.py gives flavour 2. Tolerance: the project's, per-pixel RMSE <
1e-4 (the two differ by the order of the fp32 additions into the frames). Semantics:
tests/test_lens.py (CPU)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import bdpt_amd as B
from _inflights import fixture_scene, threads
from _lens import FOCAL, LENS, lens_render
from _util import REPO, golden_scene
from test_output_stage import CLI, read_png

pytestmark = pytest.mark.gpu

RMSE_TOL = 1e-4
SEED = 5489


def _scene(key, W, H):
    if key == "bunny":
        return B.load_dae(os.path.join(REPO, "scenes", "bunny.dae"), W, H)
    if key == "CBspheres":
        return golden_scene("CBspheres", W, H)
    return fixture_scene(key, W, H)


def _gpu_render(sc, W, H, S, M, rr=False, tiles=(), ranges=None):
    pt = B.BidirectionalPathTracer(sc, W, H, S, M, seed=SEED, russian_roulette=rr, infinite_lights=True,
                                   lens_radius=LENS, focal_distance=FOCAL)
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
    eye, light, st = lens_render(_scene(key, W, H), W, H, S, M, seed=SEED, rr=rr, threads=threads())
    assert st[7] == 3   # the thin-lens flavour, as bdpt_create chooses
    return eye, light


def _rmse(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))


CASES = [
    ("hemi", 32, 24, 2, 5, False, None),
    ("dir", 32, 24, 2, 5, False, None),
    ("mixed", 32, 24, 2, 5, False, None),
    ("hemi", 32, 24, 2, 8, True, None),    # a second MAXV class, roulette
    ("dir", 32, 24, 2, 1, False, None),    # the shortest paths: only (2, 1) and the light image
    ("CBspheres", 32, 24, 2, 5, False, None),   # delta BSDFs, an area light: flavour 3 on a scene of flavour 0
    ("mixed", 32, 24, 2, 5, False, "0"), ("mixed", 32, 24, 2, 5, False, "1"),
    ("mixed", 32, 24, 2, 5, False, "2"), ("mixed", 32, 24, 2, 5, False, "3"),   # every LDS mode
    ("bunny", 64, 48, 1, 5, False, None),  # 28k triangles: the treelet path
]
# the cases whose CPU light frame is not zero at these frame sizes (asserted below): there the camera
# connection through a lens point (t = 1) runs on the GPU
LIGHT_FRAME_CASES = {"mixed", "CBspheres"}


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
    assert eye.mean() > 0
    if key in LIGHT_FRAME_CASES:
        assert light.mean() > 0 and np.count_nonzero(light.sum(axis=2)) >= 4
    assert re_ < RMSE_TOL and rl < RMSE_TOL
    if lds is not None:
        assert g["stats"].lds_mode == int(lds)
    if key == "bunny":
        assert g["stats"].lds_mode == 2


def test_lens_differs_from_pinhole_on_the_gpu():
    """The lens reaches the kernels: the same scene and seed without it renders another image."""
    W, H, S, M = 32, 24, 2, 5
    sc = _scene("mixed", W, H)
    lens = _gpu_render(sc, W, H, S, M)
    pt = B.BidirectionalPathTracer(sc, W, H, S, M, seed=SEED, infinite_lights=True)
    try:
        pt.raytrace_tiles()
        pin = pt.read_frame(B.FRAME_EYE).astype(np.float64)
    finally:
        pt.close()
    assert _rmse(lens["eye"], pin) > 100 * RMSE_TOL


def test_tiles_and_sample_ranges_compose():
    """Two sample ranges over two tiles sum to the whole-frame render (the tolerance of
    test_gpu_parity.py::test_tiles_and_sample_ranges_compose)."""
    W, H, S, M = 32, 24, 2, 5
    sc = _scene("mixed", W, H)
    full = _gpu_render(sc, W, H, S, M)
    tiled = _gpu_render(sc, W, H, S, M, tiles=[(0, 0, 16, H), (16, 0, 16, H)], ranges=[(0, 1), (1, 2)])
    assert _rmse(full["eye"] + full["light"], tiled["eye"] + tiled["light"]) < 1e-6


def test_cli_thin_lens(tmp_path):
    """pathtracer --thin-lens -b 0.5 -d 2.5 writes the PNG of the Python render of the same settings
    (the same kernels; through the CLI's output stage, a step of one where a pixel sits on a
    quantisation boundary)."""
    W, H, S, M = 32, 24, 2, 5
    dae = os.path.join(REPO, "scenes", "CBspheres.dae")
    out = tmp_path / "lens.png"
    r = subprocess.run([CLI, "--thin-lens", "-b", str(LENS), "-d", str(FOCAL), "-s", str(S), "-m", str(M),
                        "-r", str(W), str(H), "-f", str(out), "--no-stats", dae], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    assert "thin lens, radius 0.5, focal distance 2.5" in r.stderr
    ours = read_png(out)
    g = _gpu_render(B.load_dae(dae, W, H), W, H, S, M)
    raw = tmp_path / "ref.f64"
    np.ascontiguousarray(g["eye"] + g["light"], dtype="<f8").tofile(raw)
    subprocess.run([CLI, "--tonemap", str(raw), str(W), str(H), str(tmp_path / "ref.png")], check=True)
    ref = read_png(tmp_path / "ref.png")
    d = np.abs(ours.astype(int) - ref.astype(int))
    assert d.max() <= 1 and np.count_nonzero(d) <= 0.002 * d.size
