"""GPU: the `pathtracer` CLI's --denoise-batches / --denoise-sigma-variance: the
variance-guided denoised image against an equal Python render, the standard-error image, and the
unchanged outputs without the new flags."""
import subprocess

import numpy as np
import pytest

import bdpt_amd as B
from test_gpu_denoise_cli import H, M, S, SCENE, W, close, run_cli, tonemapped
from test_output_stage import CLI, read_png

pytestmark = pytest.mark.gpu
K = 4


def test_cli_batches_give_the_python_path_image(tmp_path):
    """--denoise --denoise-batches 4 --features: out_denoised.png is the tonemap of
    denoise_variance() of an equal Python render and out_stderr.png that of sqrt(read_variance())
    as a grey, to test_cli.py's tolerance for two BDPT renders of the same samples (one 8-bit step
    on at most 0.2 % of the values: the atomics land in any order); out.png is the plain run's to
    the same tolerance and out_rate.png byte for byte; --denoise-sigma-variance and
    --denoise-levels reach the library."""
    for d in ("a", "b", "c"):
        (tmp_path / d).mkdir()
    run_cli(tmp_path / "a" / "out.png", "--denoise", "--features")
    run_cli(tmp_path / "b" / "out.png", "--denoise", "--features", "--denoise-batches", str(K))
    assert not (tmp_path / "a" / "out_stderr.png").exists()
    assert close(read_png(tmp_path / "a" / "out.png"), read_png(tmp_path / "b" / "out.png"))
    assert (tmp_path / "a" / "out_rate.png").read_bytes() == (tmp_path / "b" / "out_rate.png").read_bytes()
    for n in ("out_albedo.png", "out_normal.png", "out_depth.png"):   # the feature pass has no atomics
        assert (tmp_path / "a" / n).read_bytes() == (tmp_path / "b" / n).read_bytes()
    r = B.BidirectionalPathTracer(B.load_dae(SCENE, W, H), W, H, S, M)
    try:
        r.render_batches(0, S, K)
        r.variance()
        var = r.read_variance()
        r.render_features()
        den = r.denoise_variance()
        wide = r.denoise_variance(levels=2, sigma_variance=16.0)
    finally:
        r.close()
    got = read_png(tmp_path / "b" / "out_denoised.png")
    assert close(got, tonemapped(den, tmp_path, "den"))
    assert not close(got, read_png(tmp_path / "a" / "out_denoised.png"))   # not the plain filter's image
    se = np.repeat(np.sqrt(var.astype(np.float64))[..., None], 3, axis=2)
    assert close(read_png(tmp_path / "b" / "out_stderr.png"), tonemapped(se, tmp_path, "se"))
    run_cli(tmp_path / "c" / "out.png", "--denoise", "--denoise-batches", str(K), "--denoise-levels", "2",
            "--denoise-sigma-variance", "16")
    got_wide = read_png(tmp_path / "c" / "out_denoised.png")
    assert close(got_wide, tonemapped(wide, tmp_path, "wide")) and not close(got_wide, got)
    assert not (tmp_path / "c" / "out_stderr.png").exists()   # --features was not given


def test_cli_without_the_new_flags_is_unchanged(tmp_path):
    """--pt renders without atomics, so runs repeat bit for bit: two runs without --denoise-batches
    write byte-identical PNGs, out_denoised.png included; and the flag is refused where batches do
    not apply (the PathTracer, K that does not divide -s, K = 1)."""
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    pt = ("--pt", "-a", "2", "0.05")
    run_cli(tmp_path / "a" / "out.png", *pt, "--denoise", "--features")
    run_cli(tmp_path / "b" / "out.png", *pt, "--denoise", "--features")
    names = ("out.png", "out_rate.png", "out_denoised.png", "out_albedo.png", "out_normal.png", "out_depth.png")
    for n in names:
        assert (tmp_path / "a" / n).read_bytes() == (tmp_path / "b" / n).read_bytes()
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == sorted(names)
    for flags in (("--pt", "--denoise-batches", "2"), ("--denoise-batches", "3"), ("--denoise-batches", "1")):
        r = subprocess.run([CLI, "-s", str(S), "-m", str(M), "-r", str(W), str(H), "--no-stats", "-f",
                            str(tmp_path / "x.png"), *flags, SCENE], capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "--denoise-batches" in r.stderr
        assert not (tmp_path / "x.png").exists()
