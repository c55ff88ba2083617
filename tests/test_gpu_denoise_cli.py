"""GPU: the `pathtracer` CLI's --denoise / --features: the new PNGs, the unchanged
old ones, the denoised image against an equal Python render, and -g 2 against -g 1."""
import os
import subprocess

import numpy as np
import pytest

import bdpt_amd as B
from _util import REPO
from test_output_stage import CLI, read_png

pytestmark = pytest.mark.gpu
W, H, S, M = 64, 48, 4, 5
SCENE = os.path.join(REPO, "scenes", "CBspheres.dae")


def run_cli(out, *flags):
    r = subprocess.run([CLI, "-s", str(S), "-m", str(M), "-r", str(W), str(H), "--no-stats", "-f", str(out), *flags,
                        SCENE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "Job completed" in r.stdout
    return r


def tonemapped(hdr, tmp_path, name):
    raw = tmp_path / (name + ".f64")
    np.ascontiguousarray(hdr, dtype="<f8").tofile(raw)
    subprocess.run([CLI, "--tonemap", str(raw), str(W), str(H), str(tmp_path / (name + ".png"))], check=True)
    return read_png(tmp_path / (name + ".png"))


def close(a, b):
    """test_cli.py's tolerance for two BDPT renders of the same samples (the light image's atomics
    land in any order): one 8-bit step on at most 0.2 % of the values."""
    d = np.abs(a.astype(int) - b.astype(int))
    return d.max() <= 1 and np.count_nonzero(d) <= 0.002 * d.size


def test_cli_denoise_and_features_under_the_pathtracer(tmp_path):
    """--pt renders without atomics, so two runs repeat bit for bit: out.png and out_rate.png are
    byte-identical with and without the new flags, the four new PNGs exist at the frame size, and
    out_denoised.png is the tonemap of read_denoised of an equal Python render, exactly."""
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    pt = ("--pt", "-a", "2", "0.05")
    run_cli(tmp_path / "a" / "out.png", *pt)
    run_cli(tmp_path / "b" / "out.png", *pt, "--denoise", "--features")
    for n in ("out.png", "out_rate.png"):
        assert (tmp_path / "a" / n).read_bytes() == (tmp_path / "b" / n).read_bytes()
    for n in ("out_denoised.png", "out_albedo.png", "out_normal.png", "out_depth.png"):
        assert not (tmp_path / "a" / n).exists()
        assert read_png(tmp_path / "b" / n).shape[:2] == (H, W)
    r = B.PathTracer(B.load_dae(SCENE, W, H), W, H, S, M, samples_per_batch=2, max_tolerance=0.05)
    try:
        r.raytrace_tiles()
        r.render_features()
        den = r.denoise()
        f = r.read_features()
    finally:
        r.close()
    assert np.array_equal(read_png(tmp_path / "b" / "out_denoised.png"), tonemapped(den, tmp_path, "den"))
    # the feature images: linear, clamped, 8 bits by truncation; PNG rows run top to bottom
    alb = read_png(tmp_path / "b" / "out_albedo.png")[..., :3]
    assert np.array_equal(alb, (np.clip(f["albedo"], 0, 1) * np.float32(255)).astype(np.uint8)[::-1])
    nrm = read_png(tmp_path / "b" / "out_normal.png")[..., :3]
    want = (np.clip(np.float32(0.5) * f["normal"] + np.float32(0.5), 0, 1) * np.float32(255)).astype(np.uint8)[::-1]
    assert np.array_equal(nrm, want)
    dep = read_png(tmp_path / "b" / "out_depth.png")[..., 0]
    assert np.array_equal(dep, (np.clip(f["depth"] / f["depth"].max(), 0, 1) * np.float32(255)).astype(np.uint8)[::-1])


def test_cli_denoise_under_bdpt_and_two_workers(tmp_path):
    """BDPT: the flags leave out.png and out_rate.png as they are (to the splat-order tolerance:
    two BDPT renders differ in their last bits), --denoise-levels / --denoise-sigma / --feature-spp
    reach the library, and -g 2 --devices 0,0 (features and filter on context 0 after the reduce)
    gives the -g 1 image to the same tolerance."""
    for d in ("a", "b", "c", "g"):
        (tmp_path / d).mkdir()
    run_cli(tmp_path / "a" / "out.png")
    run_cli(tmp_path / "b" / "out.png", "--denoise")
    assert close(read_png(tmp_path / "a" / "out.png"), read_png(tmp_path / "b" / "out.png"))
    assert (tmp_path / "a" / "out_rate.png").read_bytes() == (tmp_path / "b" / "out_rate.png").read_bytes()
    assert not (tmp_path / "b" / "out_albedo.png").exists()
    den = read_png(tmp_path / "b" / "out_denoised.png")
    assert not close(den, read_png(tmp_path / "b" / "out.png"))
    run_cli(tmp_path / "g" / "out.png", "--denoise", "-g", "2", "--devices", "0,0")
    assert close(read_png(tmp_path / "g" / "out_denoised.png"), den)
    # levels 0 with any sigmas is the identity on the undemodulated default: the plain image again
    run_cli(tmp_path / "c" / "out.png", "--denoise", "--denoise-levels", "0", "--denoise-sigma", "2", "0.5", "0.2",
            "--feature-spp", "1")
    assert np.array_equal(read_png(tmp_path / "c" / "out_denoised.png"), read_png(tmp_path / "c" / "out.png"))
    r = subprocess.run([CLI, "-s", str(S), "-f", str(tmp_path / "c" / "x.png"), "-r", str(W), str(H), "--denoise",
                        "--feature-spp", str(S + 1), SCENE], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "spp" in r.stderr
