"""GPU: the `pathtracer` CLI's --adaptive: the resolved colour against an equal Python
render through the same output stage, the rate image against the counts, the variance-guided
denoise of the resolved frame, and the refused combinations."""
import os
import subprocess

import numpy as np
import pytest

import bdpt_amd as B
import _adaptive as A
from _util import REPO
from test_output_stage import CLI, read_png

pytestmark = pytest.mark.gpu
W, H, S, M, BATCH, TOL = 60, 44, 32, 5, 2, 0.3   # clipped blocks on both edges
SCENE = os.path.join(REPO, "scenes", "CBspheres.dae")
BASE = ["-s", str(S), "-m", str(M), "-r", str(W), str(H), "--no-stats"]


def run_cli(out, *flags):
    r = subprocess.run([CLI, *BASE, "-f", str(out), *flags, SCENE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "Job completed" in r.stdout
    return r


def tonemapped(hdr, tmp_path, name):
    raw = tmp_path / (name + ".f64")
    np.ascontiguousarray(hdr, dtype="<f8").tofile(raw)
    subprocess.run([CLI, "--tonemap", str(raw), str(W), str(H), str(tmp_path / (name + ".png"))], check=True)
    return read_png(tmp_path / (name + ".png"))


def rounds_of_rate_png(path):
    """K_b per pixel (H, W), row 0 = bottom, from the rate image's colours: a rate s = K m / S <= 1/2
    is written as green = 2 s, blue = 1 - 2 s, above it as red = 2 s - 1, green = 2 - 2 s (8 bits by
    truncation); the PNG's row i is the frame's row H - 1 - i. K / 16 steps are 32 grey levels apart."""
    px = read_png(path)[::-1].astype(np.float64) / 255.0
    s = np.where(px[..., 0] > 0, 0.5 + 0.5 * px[..., 0], 0.5 * px[..., 1])
    return np.rint(s * S / BATCH).astype(np.int32)


def test_cli_adaptive_gives_the_python_path_image(tmp_path):
    """--adaptive -a 2 0.3 -s 32: out_rate.png decodes to one K_b per 8x8 block (clipped blocks
    included), between min_rounds and 16, with several values; out.png is the tonemap of the Python
    path's resolved colour to test_cli.py's tolerance for two BDPT renders of the same samples (one
    8-bit step on at most 0.2 % of the values), on the blocks on which the two runs' schedules agree:
    two renders differ in the order of their atomic adds, so a block at the threshold may stop a round
    apart; at least 90 % of the blocks must agree (the agreement is printed). Without --adaptive, -a
    changes nothing under BDPT."""
    run = run_cli(tmp_path / "out.png", "--adaptive", "-a", str(BATCH), str(TOL), "--denoise", "--features")
    assert "adaptive:" in run.stderr
    K_cli = rounds_of_rate_png(tmp_path / "out_rate.png")
    bid = A.block_ids(W, H)
    nb = A.block_pixels(W, H).size
    per_block = [np.unique(K_cli[bid == b]) for b in range(nb)]
    assert all(u.size == 1 for u in per_block), per_block
    Kb_cli = np.array([u[0] for u in per_block])
    assert Kb_cli.min() >= 4 and Kb_cli.max() <= S // BATCH and np.unique(Kb_cli).size >= 3
    r = B.BidirectionalPathTracer(B.load_dae(SCENE, W, H), W, H, S, M)
    try:
        info = r.render_adaptive(samples_per_round=BATCH, tolerance=TOL)
        r.adaptive_resolve()
        py = r.read_adaptive()
        Kb_py = r.read_adaptive_rounds().ravel()
        r.render_features()
        ptrs = r.adaptive_device_ptrs()
        r.sync()
        B.denoise_variance_buffers(ptrs["color"], ptrs["variance"], r.features_device_ptr(), W, H, ptrs["color"])
        den = r.read_adaptive()["color"]
    finally:
        r.close()
    agree = Kb_cli == Kb_py
    print(f"CLI K_b {Kb_cli.tolist()}\nPython K_b {Kb_py.tolist()} {info}\nagreeing blocks {agree.mean():.3f}")
    assert agree.mean() >= 0.9
    mask = agree[bid][::-1]   # PNG rows run top-down
    got, want = read_png(tmp_path / "out.png"), tonemapped(py["color"], tmp_path, "py_out")
    d = np.abs(got.astype(int) - want.astype(int))[mask]
    print(f"out.png: max step {d.max()}, differing values {np.count_nonzero(d)} of {d.size}")
    assert d.max() <= 1 and np.count_nonzero(d) <= 0.002 * d.size
    # the filter reads its neighbours across block borders: where all blocks agree the denoised image
    # holds to the same tolerance; otherwise it is only required to exist at the frame size
    got_d = read_png(tmp_path / "out_denoised.png")
    assert got_d.shape[:2] == (H, W)
    if agree.all():
        d = np.abs(got_d.astype(int) - tonemapped(den, tmp_path, "py_den").astype(int))
        assert d.max() <= 1 and np.count_nonzero(d) <= 0.002 * d.size
    assert read_png(tmp_path / "out_stderr.png").shape[:2] == (H, W)   # --features with a variance at hand
    # -a without --adaptive: ignored under BDPT, as before
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    run_cli(tmp_path / "a" / "out.png")
    run_cli(tmp_path / "b" / "out.png", "-a", str(BATCH), str(TOL))
    assert (tmp_path / "a" / "out_rate.png").read_bytes() == (tmp_path / "b" / "out_rate.png").read_bytes()
    da = np.abs(read_png(tmp_path / "a" / "out.png").astype(int) - read_png(tmp_path / "b" / "out.png").astype(int))
    assert da.max() <= 1 and np.count_nonzero(da) <= 0.002 * da.size
    assert (rounds_of_rate_png(tmp_path / "a" / "out_rate.png") == S // BATCH).all()


@pytest.mark.parametrize("flags,message", [
    (("--pt",), "PathTracer"),
    (("-g", "2"), "-g 1"),
    (("-p", "0", "0", "16", "16"), "no -p"),
    (("--denoise-batches", "2"), "--denoise-batches"),
    (("-a", "5", "0.3"), "divide -s"),
])
def test_cli_refuses_what_adaptive_cannot_do(tmp_path, flags, message):
    args = [CLI, *BASE, "-f", str(tmp_path / "x.png"), "--adaptive"]
    if "-a" not in flags:
        args += ["-a", str(BATCH), str(TOL)]
    r = subprocess.run(args + list(flags) + [SCENE], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and message in r.stderr, r.stderr
    assert "--adaptive" in r.stderr
    assert not (tmp_path / "x.png").exists()
