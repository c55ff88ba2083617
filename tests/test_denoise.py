"""The edge-avoiding a-trous filter on the host build of csrc/bdpt_atrous.h: against
the float64 restatement of its definition (tests/_denoise.py), its exact properties, and a run of
both new host builds under ASan + UBSan. No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _denoise as D
from _util import REPO

BIG = 1e18
SIG = dict(sigma_color=1.0, sigma_normal=0.3, sigma_depth=0.1)


def rel_dev(a, b, color):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(color).max())


@pytest.mark.parametrize("W,H,levels,demod", D.CASES)
def test_filter_matches_float64_restatement(W, H, levels, demod):
    """fp32 host build vs the float64 numpy restatement on the synthetic inputs. Largest deviation
    relative to the input's maximum, measured over all cases: 5.2e-7 (37x21, levels 3 and 5, not
    demodulated). Asserted: 5 x that (D.FP32_VS_FP64)."""
    color, feat = D.synthetic(W, H)
    got = D.host_filter(color, feat, levels, demodulate=demod, **SIG)
    ref = D.ref_filter(color, feat, levels, demodulate=demod, **SIG)
    dev = rel_dev(got, ref, color)
    print(f"{W}x{H} levels {levels} demodulate {demod}: {dev:.3e}")
    assert np.isfinite(got).all()
    assert dev <= 5 * D.FP32_VS_FP64
    if levels >= 3 and W * H > 64:   # the filter does something: it is not the identity here
        assert rel_dev(got, color.astype(np.float64), color) > 0.05


@pytest.mark.parametrize("W,H", D.FRAMES)
def test_zero_levels_is_the_identity(W, H):
    color, feat = D.synthetic(W, H)
    assert np.array_equal(D.host_filter(color, feat, 0, demodulate=False, **SIG), color)


@pytest.mark.parametrize("W,H", D.FRAMES)
@pytest.mark.parametrize("levels", [1, 3, 5])
def test_constant_in_constant_out(W, H, levels):
    """A constant colour stays constant within 32 * 2^-24 * levels relative: per level the 25
    products and sums of numerator and denominator and one division."""
    _, feat = D.synthetic(W, H)
    for v in (0.7, 123.456):
        color = np.full((H, W, 3), v, np.float32)
        out = D.host_filter(color, feat, levels, demodulate=False, **SIG)
        assert np.abs(out.astype(np.float64) - float(np.float32(v))).max() <= 32 * 2.0 ** -24 * levels * v


def b3_blur(color, levels):
    """The plain 5x5 B3 a-trous blur with clipped, renormalised borders, float64."""
    c = np.asarray(color, np.float64)
    H, W = c.shape[:2]
    for i in range(levels):
        step = 1 << i
        num, den = np.zeros_like(c), np.zeros((H, W))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                ox, oy = dx * step, dy * step
                x0, x1, y0, y1 = max(0, -ox), min(W, W - ox), max(0, -oy), min(H, H - oy)
                if x0 >= x1 or y0 >= y1:
                    continue
                h = D.KERNEL[dx + 2] * D.KERNEL[dy + 2]
                num[y0:y1, x0:x1] += h * c[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
                den[y0:y1, x0:x1] += h
        c = num / den[..., None]
    return c


@pytest.mark.parametrize("W,H", D.FRAMES)
@pytest.mark.parametrize("levels", [1, 3, 5])
def test_huge_sigmas_give_the_plain_b3_blur(W, H, levels):
    """With all three sigmas 1e18 every weight is 1: the plain B3 a-trous blur, to the tolerance of
    the float64 comparison. The zero-coverage band's depth 0 against its neighbours' gives
    e_d = (1 / 1e18)^2, still 0 in the exponent."""
    color, feat = D.synthetic(W, H)
    got = D.host_filter(color, feat, levels, BIG, BIG, BIG, False)
    assert rel_dev(got, b3_blur(color, levels), color) <= 5 * D.FP32_VS_FP64


@pytest.mark.parametrize("W,H", D.FRAMES)
@pytest.mark.parametrize("demod", [False, True])
def test_opposite_normals_do_not_leak(W, H, demod):
    """sigma_normal 1e-3 across two half-planes of opposite normals: e_n = 4e6, expf gives exactly
    0, so every output pixel lies within [min, max] of the input on its own side, per channel
    (demodulated: of the demodulated input, then multiplied back: compared before that)."""
    color, feat = D.synthetic(W, H, opposite=True)
    feat[..., 0:3] = 0.5 if demod else feat[..., 0:3]   # one albedo: the bound survives the round trip
    feat[..., 6] = 1.0                                    # one depth, so only the normals separate
    feat[..., 3:6][feat[..., 7] == 0] = (0, 0, 1)         # the band keeps normals: two sides only
    left = np.arange(W) < (W + 1) // 2
    feat[:, ~left, 3:6] = (0, 0, -1)
    for x in range(3):
        color[:, left, x] = np.clip(color[:, left, x], 0.0, 0.5)
        color[:, ~left, x] = np.clip(color[:, ~left, x], 1.5, 2.0)
    out = D.host_filter(color, feat, 5, 1e3, 1e-3, BIG, demod)
    slack = 4 * 2.0 ** -24 * 2.0 if demod else 0.0   # the division and multiplication by albedo + 0.01
    for side in (left, ~left):
        if not side.any():
            continue
        lo, hi = color[:, side].min((0, 1)), color[:, side].max((0, 1))
        assert np.all(out[:, side] >= lo - slack) and np.all(out[:, side] <= hi + slack)


@pytest.mark.parametrize("W,H", D.FRAMES)
def test_finite_in_finite_out(W, H):
    """Zero-coverage pixels (all-zero records) with finite colour stay finite, demodulated or not,
    at every level count up to the cap."""
    color, feat = D.synthetic(W, H)
    for levels in (0, 1, 5, 8):
        for demod in (False, True):
            assert np.isfinite(D.host_filter(color, feat, levels, demodulate=demod, **SIG)).all()
    feat[...] = 0
    assert np.isfinite(D.host_filter(color, feat, 5, demodulate=True, **SIG)).all()


def test_defaults_are_the_documented_ones():
    """DESIGN.md §11 names the defaults the sweep chose; the library and the host build agree."""
    d = D.defaults()
    text = open(os.path.join(REPO, "DESIGN.md")).read()
    line = f"levels {d['levels']}, sigma_color {d['sigma_color']:g}, sigma_normal {d['sigma_normal']:g}, " \
           f"sigma_depth {d['sigma_depth']:g}, demodulate {'on' if d['demodulate'] else 'off'}"
    assert line in text, line


CSRC = os.path.join(REPO, "bidirectional-pathtracing_amd", "csrc")
NATIVE = os.path.join(REPO, "tests", "native")
SAN_FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-omit-frame-pointer",
             "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-I" + os.path.join(REPO, "include"), "-I" + CSRC]


@pytest.mark.slow
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_host_builds_under_asan_ubsan(tmp_path):
    """tests/native/denoise_probe.cpp: the host filter (levels up to 8, in place too) and the host
    feature render (both integrators, every LDS mode's traversal) on the odd frame sizes, every
    buffer at exactly its size, built with ASan + UBSan and run as a child process."""
    from concurrent.futures import ThreadPoolExecutor
    srcs = [os.path.join(NATIVE, "denoise_probe.cpp"), os.path.join(NATIVE, "core_cpu_denoise.cpp"),
            os.path.join(CSRC, "bdpt_scene.cpp"), os.path.join(CSRC, "dae_loader.cpp")]
    objs = [str(tmp_path / (os.path.basename(s) + ".o")) for s in srcs]
    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(lambda so: subprocess.run(["g++"] + SAN_FLAGS + ["-c", so[0], "-o", so[1]], check=True,
                                              capture_output=True, text=True, timeout=600), zip(srcs, objs)))
    exe = str(tmp_path / "denoise_probe")
    subprocess.run(["g++", "-fsanitize=address,undefined", "-static-libasan", "-o", exe] + objs + ["-lz"],
                   check=True, capture_output=True, text=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, os.path.join(REPO, "scenes", "CBspheres.dae")], capture_output=True,
                       text=True, timeout=600, env=env)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "no sanitizer report" in r.stdout
