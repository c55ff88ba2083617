"""Helpers of the variance-guided denoise tests: the host build of
csrc/bdpt_variance.h (tests/native/libcorecpu_variance.so), synthetic batch frames and variance
frames, and float64 numpy restatements of the moments, the variance and the filter."""
import ctypes as C
import os

import numpy as np

import _denoise as D
from _util import REPO

SO = os.path.join(REPO, "tests", "native", "libcorecpu_variance.so")
PF = C.POINTER(C.c_float)
FRAMES = D.FRAMES
BATCHES = (2, 3, 8)
U = 2.0 ** -24
VAR_EPS = float(np.float32(1e-8))

# Largest |host fp32 filter - float64 restatement| / max|input| over FRAMES x levels (0, 1, 3, 5),
# colour and variance each against its own input's maximum, measured on the CPU build
# (2.12e-7: 37x21, 1 level, the variance; test_variance.py prints every case and asserts 5x).
FP32_VS_FP64 = 2.2e-7

SIG = dict(sigma_variance=2.0, sigma_normal=0.3, sigma_depth=0.1)   # the sigmas of the comparisons
LEAK = dict(levels=5, sigma_variance=1e3, sigma_normal=1e-3, sigma_depth=1e18)
CASES = [(W, H, L) for (W, H) in FRAMES for L in (0, 1, 3, 5)]
CTX = dict(W=16, H=12, S=8, M=5, K=4, seed=5489)   # the context-path case of the GPU tests (CBspheres)

_lib = None


def lib():
    global _lib
    if _lib is None:
        import __graft_entry__ as ge
        ge.build_core_cpu_variance()
        L = C.CDLL(SO)
        L.core_cpu_variance_moments.argtypes = [PF, PF, PF, C.c_longlong]
        L.core_cpu_variance_variance.argtypes = [PF, C.c_int, C.c_longlong, PF]
        L.core_cpu_variance_defaults.argtypes = [C.POINTER(C.c_int), PF]
        L.core_cpu_variance_defaults.restype = None
        L.core_cpu_variance_filter.argtypes = [PF, PF, PF, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float,
                                               PF, PF]
        _lib = L
    return _lib


def _f(a):
    return a.ctypes.data_as(PF)


def defaults():
    lv, sg = (C.c_int * 1)(), (C.c_float * 3)()
    lib().core_cpu_variance_defaults(lv, sg)
    return dict(levels=lv[0], sigma_variance=sg[0], sigma_normal=sg[1], sigma_depth=sg[2])


def host_moments(frames_a, frames_b=None):
    """The record (H, W, 4) after the cumulative frames frames_a[k] (+ frames_b[k]) in turn."""
    H, W = frames_a[0].shape[:2]
    rec = np.zeros((H, W, 4), np.float32)
    for k, a in enumerate(frames_a):
        a = np.ascontiguousarray(a, np.float32)
        b = None if frames_b is None else np.ascontiguousarray(frames_b[k], np.float32)
        rc = lib().core_cpu_variance_moments(_f(a), None if b is None else _f(b), _f(rec), W * H)
        assert rc == 0, rc
    return rec


def host_variance(rec, K):
    rec = np.ascontiguousarray(rec, np.float32)
    H, W = rec.shape[:2]
    var = np.empty((H, W), np.float32)
    rc = lib().core_cpu_variance_variance(_f(rec), K, W * H, _f(var))
    assert rc == 0, rc
    return var


def host_filter(color, var, feat, levels, sigma_variance, sigma_normal, sigma_depth):
    """(colour (H, W, 3), variance (H, W)) of the host build."""
    color = np.ascontiguousarray(color, np.float32)
    var = np.ascontiguousarray(var, np.float32)
    feat = np.ascontiguousarray(feat, np.float32)
    H, W = color.shape[:2]
    out, vout = np.empty_like(color), np.empty_like(var)
    rc = lib().core_cpu_variance_filter(_f(color), _f(var), _f(feat), W, H, levels, sigma_variance, sigma_normal,
                                        sigma_depth, _f(out), _f(vout))
    assert rc == 0, rc
    return out, vout


# ------------------------------------------------------------------------------------------------
# synthetic inputs

def batch_frames(W, H, K, seed=11, identical=False):
    """(a, b): K cumulative fp32 frame pairs (H, W, 3) each, as two frames that are added per pixel
    (the eye and the light frame): the fp32 running sums of random increments in [0, 1) and
    [0, 0.5). identical: every batch adds the same increment, a multiple of 2^-20, so that every
    cumulative frame k * increment (k <= 8) is exact in fp32 (fl(3 b) of a full 24-bit b is not, and
    the batches a renderer would then see are no longer identical)."""
    rng = np.random.default_rng(seed + 1000 * W + 10 * H + K)
    a, b = [], []
    ca, cb = np.zeros((H, W, 3), np.float32), np.zeros((H, W, 3), np.float32)
    ia, ib = rng.uniform(0, 1, (H, W, 3)).astype(np.float32), rng.uniform(0, 0.5, (H, W, 3)).astype(np.float32)
    if identical:
        ia, ib = np.floor(ia * 2.0 ** 20) / np.float32(2.0 ** 20), np.floor(ib * 2.0 ** 20) / np.float32(2.0 ** 20)
    for k in range(K):
        if not identical and k > 0:
            ia, ib = rng.uniform(0, 1, (H, W, 3)).astype(np.float32), rng.uniform(0, 0.5, (H, W, 3)).astype(np.float32)
        ca, cb = ca + ia, cb + ib
        a.append(ca.copy())
        b.append(cb.copy())
    return a, b


def ref_moments(frames):
    """float64 over the fp32 cumulative frames: (F (H, W, 3), Q (H, W))."""
    prev = np.zeros(frames[0].shape, np.float64)
    Q = np.zeros(frames[0].shape[:2])
    for f in frames:
        f = np.asarray(f, np.float64)
        Q += ((f - prev) ** 2).sum(-1)
        prev = f
    return prev, Q


def ref_variance(F, Q, K):
    return np.maximum(0.0, (Q - (F ** 2).sum(-1) / K) * (K / (K - 1.0)))


def variance_scale(F, Q, K):
    """(Q + |F|^2 / K) K / (K - 1): what the rounding errors of the variance are relative to."""
    return (Q + (F ** 2).sum(-1) / K) * (K / (K - 1.0))


def synthetic(W, H, seed=7):
    """_denoise.synthetic's colour and features, and a variance frame (H, W) in [0, 0.5) with a
    block of exact zeros where the frame has room for it."""
    color, feat = D.synthetic(W, H, seed)
    rng = np.random.default_rng(seed + 77 + 1000 * W + H)
    var = rng.uniform(0.0, 0.5, (H, W)).astype(np.float32)
    if W >= 8 and H >= 8:
        var[2:6, 1:5] = 0.0
    return color, var, feat


def leak_inputs(W, H):
    color, feat, left = D.leak_inputs(W, H)
    var = np.full((H, W), 0.25, np.float32)
    return color, var, feat, left


def distinct_colors(W, H):
    """Colours of which any two pixels differ by more than 0.01 in a channel: pixel k has red 0.02 k."""
    c = np.zeros((H, W, 3), np.float32)
    c[..., 0] = (0.02 * np.arange(W * H)).reshape(H, W)
    c[..., 1] = 0.5
    c[..., 2] = 0.25
    return c


# ------------------------------------------------------------------------------------------------
# the float64 restatement

def _shifts(W, H, step, r):
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            ox, oy = dx * step, dy * step
            x0, x1, y0, y1 = max(0, -ox), min(W, W - ox), max(0, -oy), min(H, H - oy)
            if x0 >= x1 or y0 >= y1:
                continue
            yield dx, dy, (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))


def ref_prefilter(v):
    H, W = v.shape
    g = np.array([0.25, 0.5, 0.25])
    s, ws = np.zeros((H, W)), np.zeros((H, W))
    for dx, dy, P, Q in _shifts(W, H, 1, 1):
        w = g[dx + 1] * g[dy + 1]
        s[P] += w * v[Q]
        ws[P] += w
    return s / ws


def ref_filter(color, var, feat, levels, sigma_variance, sigma_normal, sigma_depth):
    """The filter's definition (include/bdpt/bdpt.h) in float64 over the fp32 inputs:
    c = sum h w c(q) / sum h w, v = sum (h w)^2 v(q) / (sum h w)^2."""
    c = np.asarray(color, np.float64)
    v = np.asarray(var, np.float64)
    f = np.asarray(feat, np.float64)
    H, W = v.shape
    n, d = f[..., 3:6], f[..., 6]
    sv, sn, sd = (float(np.float32(s)) for s in (sigma_variance, sigma_normal, sigma_depth))
    for i in range(levels):
        cden = sv ** 2 * ref_prefilter(v) + VAR_EPS
        num, den, vnum = np.zeros_like(c), np.zeros((H, W)), np.zeros((H, W))
        for dx, dy, P, Q in _shifts(W, H, 1 << i, 2):
            h = D.KERNEL[dx + 2] * D.KERNEL[dy + 2]
            if dx == 0 and dy == 0:
                w = np.ones((H, W))[P]
            else:
                ec = ((c[P] - c[Q]) ** 2).sum(-1) / cden[P]
                en = ((n[P] - n[Q]) ** 2).sum(-1) / sn ** 2
                m = np.maximum(d[P], d[Q])
                with np.errstate(invalid="ignore", divide="ignore"):
                    ed = np.where(m != 0, ((d[P] - d[Q]) / (sd * m)) ** 2, 0.0)
                w = np.exp(-(ec + en + ed))
            num[P] += (h * w)[..., None] * c[Q]
            den[P] += h * w
            vnum[P] += (h * w) ** 2 * v[Q]
        c, v = num / den[..., None], vnum / den ** 2
    return c, v


def tap_max(v, levels):
    """Per pixel the largest value of v over the in-frame taps of every level up to `levels`, applied
    level by level (an upper bound of the filtered variance)."""
    v = np.asarray(v, np.float64).copy()
    H, W = v.shape
    for i in range(levels):
        m = np.full((H, W), -np.inf)
        for dx, dy, P, Q in _shifts(W, H, 1 << i, 2):
            m[P] = np.maximum(m[P], v[Q])
        v = m
    return v
