"""Helpers of the denoised-output tests: the host build of the feature pass and the
a-trous filter (tests/native/libcorecpu_denoise.so), synthetic filter inputs, and ref_filter, a
float64 numpy restatement of the filter's definition."""
import ctypes as C
import os

import numpy as np

import bdpt_amd as B
from _util import REPO

SO = os.path.join(REPO, "tests", "native", "libcorecpu_denoise.so")
PF, PI = C.POINTER(C.c_float), C.POINTER(C.c_int)
FRAMES = ((37, 21), (8, 8), (1, 1), (64, 3))   # (W, H)
KERNEL = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])
EPS = float(np.float32(0.01))

# Largest |host fp32 filter - float64 restatement| / max|input| over FRAMES x levels (0, 1, 3, 5) x
# demodulation on / off, measured on the CPU build: 5.2e-7 (test_denoise.py asserts 5x).
FP32_VS_FP64 = 5.2e-7

_lib = None


def lib():
    global _lib
    if _lib is None:
        import __graft_entry__ as ge
        ge.build_core_cpu_denoise()
        L = C.CDLL(SO)
        D = C.POINTER(B.SceneDesc)
        L.core_cpu_denoise_features.argtypes = [D, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int, C.c_double,
                                                C.c_double, C.c_int, C.c_int, PF]
        L.core_cpu_denoise_primary_rays.argtypes = [D, C.c_int, C.c_int, C.c_uint64, C.c_int, C.c_double, C.c_double,
                                                    C.c_int, PI, PF]
        L.core_cpu_denoise_sample_prims.argtypes = [D, C.c_int, C.c_int, C.c_uint64, C.c_int, C.c_double, C.c_double,
                                                    C.c_int, C.c_int, PI, PI, PF, PF, PF]
        L.core_cpu_denoise_walk_begin_rays.argtypes = [D, C.c_int, C.c_int, C.c_uint64, C.c_double, C.c_double,
                                                       C.c_int, PI, PF]
        L.core_cpu_denoise_pt_samples.argtypes = [D, C.c_int, C.c_int, C.c_uint64, C.c_double, C.c_double, C.c_int,
                                                  PI, PF]
        L.core_cpu_denoise_defaults.argtypes = [PI, PF]
        L.core_cpu_denoise_defaults.restype = None
        L.core_cpu_denoise_filter.argtypes = [PF, PF, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float,
                                              C.c_int, PF]
        _lib = L
    return _lib


def defaults():
    ld, sg = (C.c_int * 2)(), (C.c_float * 3)()
    lib().core_cpu_denoise_defaults(ld, sg)
    return dict(levels=ld[0], demodulate=bool(ld[1]), sigma_color=sg[0], sigma_normal=sg[1], sigma_depth=sg[2])


def _f(a):
    return a.ctypes.data_as(PF)


def all_samples(W, H, spp=1):
    """(n, 3) int32 rows {x, y, s} of every sample of the frame, pixel-major."""
    y, x, s = np.meshgrid(np.arange(H), np.arange(W), np.arange(spp), indexing="ij")
    return np.ascontiguousarray(np.stack([x, y, s], -1).reshape(-1, 3).astype(np.int32))


def host_features(sc, W, H, spp, seed=5489, pt=False, lens_radius=0.0, focal_distance=4.7, lds_mode=0):
    out = np.zeros((H, W, 8), np.float32)
    d = sc.desc()
    rc = lib().core_cpu_denoise_features(C.byref(d), W, H, spp, seed, 1 if pt else 0, lens_radius, focal_distance, 0,
                                         lds_mode, _f(out))
    assert rc == 0, rc
    return out


def host_primary_rays(sc, W, H, xys, seed=5489, pt=False, lens_radius=0.0, focal_distance=4.7):
    rays = np.zeros((len(xys), 8), np.float32)
    d = sc.desc()
    rc = lib().core_cpu_denoise_primary_rays(C.byref(d), W, H, seed, 1 if pt else 0, lens_radius, focal_distance,
                                             len(xys), xys.ctypes.data_as(PI), _f(rays))
    assert rc == 0, rc
    return rays


def host_samples(sc, W, H, xys, seed=5489, pt=False, lens_radius=0.0, focal_distance=4.7, lds_mode=0):
    """Per sample: (prim, t, albedo (n, 3), normal (n, 3))."""
    prim, t = np.zeros(len(xys), np.int32), np.zeros(len(xys), np.float32)
    alb, nrm = np.zeros((len(xys), 3), np.float32), np.zeros((len(xys), 3), np.float32)
    d = sc.desc()
    rc = lib().core_cpu_denoise_sample_prims(C.byref(d), W, H, seed, 1 if pt else 0, lens_radius, focal_distance,
                                             lds_mode, len(xys), xys.ctypes.data_as(PI), prim.ctypes.data_as(PI), _f(t),
                                             _f(alb), _f(nrm))
    assert rc == 0, rc
    return prim, t, alb, nrm


def host_walk_begin_rays(sc, W, H, xys, seed=5489, lens_radius=0.0, focal_distance=4.7):
    rays = np.zeros((len(xys), 8), np.float32)
    d = sc.desc()
    rc = lib().core_cpu_denoise_walk_begin_rays(C.byref(d), W, H, seed, lens_radius, focal_distance, len(xys),
                                                xys.ctypes.data_as(PI), _f(rays))
    assert rc == 0, rc
    return rays


def host_pt_samples(sc, W, H, xys, seed=5489, lens_radius=0.0, focal_distance=4.7):
    rgb = np.zeros((len(xys), 3), np.float32)
    d = sc.desc()
    rc = lib().core_cpu_denoise_pt_samples(C.byref(d), W, H, seed, lens_radius, focal_distance, len(xys),
                                           xys.ctypes.data_as(PI), _f(rgb))
    assert rc == 0, rc
    return rgb


def host_filter(color, feat, levels, sigma_color, sigma_normal, sigma_depth, demodulate):
    color = np.ascontiguousarray(color, np.float32)
    feat = np.ascontiguousarray(feat, np.float32)
    H, W = color.shape[:2]
    out = np.empty_like(color)
    rc = lib().core_cpu_denoise_filter(_f(color), _f(feat), W, H, levels, sigma_color, sigma_normal, sigma_depth,
                                       1 if demodulate else 0, _f(out))
    assert rc == 0, rc
    return out


# ------------------------------------------------------------------------------------------------
# synthetic inputs

def synthetic(W, H, seed=7, opposite=False):
    """(color (H, W, 3), features (H, W, 8)) float32: random colour in [0, 2); random albedo; two
    normal half-planes (left / right of W / 2; `opposite`: +z / -z, else +z / +y); a depth ramp; a
    band of zero-coverage rows (all-zero records) at H // 3 where the frame has the rows for it."""
    rng = np.random.default_rng(seed + 1000 * W + H)
    color = rng.uniform(0.0, 2.0, (H, W, 3)).astype(np.float32)
    feat = np.zeros((H, W, 8), np.float32)
    feat[..., 0:3] = rng.uniform(0.1, 0.9, (H, W, 3))
    left = np.arange(W) < (W + 1) // 2
    feat[:, left, 3:6] = (0, 0, 1)
    feat[:, ~left, 3:6] = (0, 0, -1) if opposite else (0, 1, 0)
    feat[..., 6] = 1.0 + 0.1 * np.arange(W)[None, :] + 0.05 * np.arange(H)[:, None]
    feat[..., 7] = 1.0
    if H >= 6:
        feat[H // 3:H // 3 + 2] = 0.0
    return color, feat


CASES = [(W, H, L, dm) for (W, H) in FRAMES for L in (0, 1, 3, 5) for dm in (False, True)]
SIG = dict(sigma_color=1.0, sigma_normal=0.3, sigma_depth=0.1)   # the sigmas of the comparisons


def leak_inputs(W, H):
    """Two half-planes of opposite normals at one depth, colours in [0, 0.5] left and [1.5, 2] right:
    (color, features, left columns)."""
    color, feat = synthetic(W, H, opposite=True)
    feat[..., 6] = 1.0
    left = np.arange(W) < (W + 1) // 2
    feat[:, left, 3:6] = (0, 0, 1)
    feat[:, ~left, 3:6] = (0, 0, -1)
    color[:, left] = np.clip(color[:, left], 0.0, 0.5)
    color[:, ~left] = np.clip(color[:, ~left], 1.5, 2.0)
    return color, feat, left


LEAK = dict(levels=5, sigma_color=1e3, sigma_normal=1e-3, sigma_depth=1e18, demodulate=False)


# ------------------------------------------------------------------------------------------------
# the float64 restatement

def ref_filter(color, feat, levels, sigma_color, sigma_normal, sigma_depth, demodulate):
    """The filter's definition (include/bdpt/bdpt.h) in float64 over the fp32 inputs."""
    c = np.asarray(color, np.float64)
    f = np.asarray(feat, np.float64)
    H, W = c.shape[:2]
    alb, n, d = f[..., 0:3], f[..., 3:6], f[..., 6]
    sn, sd = float(np.float32(sigma_normal)), float(np.float32(sigma_depth))
    if demodulate:
        c = c / (alb + EPS)
    for i in range(levels):
        step = 1 << i
        sc = float(np.float32(sigma_color)) * 2.0 ** -i
        num, den = np.zeros_like(c), np.zeros((H, W))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                ox, oy = dx * step, dy * step
                x0, x1, y0, y1 = max(0, -ox), min(W, W - ox), max(0, -oy), min(H, H - oy)
                if x0 >= x1 or y0 >= y1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                h = KERNEL[dx + 2] * KERNEL[dy + 2]
                if dx == 0 and dy == 0:
                    w = np.ones((y1 - y0, x1 - x0))
                else:
                    ec = ((c[P] - c[Q]) ** 2).sum(-1) / sc ** 2
                    en = ((n[P] - n[Q]) ** 2).sum(-1) / sn ** 2
                    m = np.maximum(d[P], d[Q])
                    with np.errstate(invalid="ignore", divide="ignore"):
                        ed = np.where(m != 0, ((d[P] - d[Q]) / (sd * m)) ** 2, 0.0)
                    w = np.exp(-(ec + en + ed))
                num[P] += (h * w)[..., None] * c[Q]
                den[P] += h * w
        c = num / den[..., None]
    if demodulate:
        c = c * (alb + EPS)
    return c


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))
