"""GPU: k_moments, k_variance and k_atrous_var (bdpt_variance.hip) against the host build of the same
arithmetic (tests/native/core_cpu_variance.cpp) on the CPU tests' synthetic inputs, the filter's
exact properties, the context path (bdpt_render_batches .. bdpt_denoise_variance) against a one-shot
render, the host build, the float64 estimator and the buffer path, the error paths, and that the
defaults denoise a low-spp render."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import bdpt_amd as B
import _denoise as D
import _pixelbound as PB
import _variance as V
from _util import golden_scene

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))
BIG = 1e18
CTX = V.CTX
PF = C.POINTER(C.c_float)

# Largest |GPU - host build| / max|input| over the cases of test_filter_matches_host_build, colour and
# variance each against its own input's maximum, measured on an MI355X: the device's expf against
# glibc's, nothing else. Asserted at 5x.
GPU_VS_HOST = 1.2e-7


@pytest.fixture(scope="module")
def torch_side(tmp_path_factory):
    """tests/_variance_gpu.py, once: the buffer entry points on torch-allocated device memory (a
    process of its own, where torch's HIP runtime initialises first)."""
    out = str(tmp_path_factory.mktemp("variance_gpu") / "out.npz")
    r = subprocess.run([sys.executable, os.path.join(TESTS, "_variance_gpu.py"), out], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return np.load(out)


@pytest.mark.parametrize("K", V.BATCHES)
@pytest.mark.parametrize("W,H", V.FRAMES)
def test_moments_and_variance_equal_the_host_build(W, H, K, torch_side):
    """k_moments and k_variance through bdpt_moments_buffers / bdpt_variance_buffers, with both
    frames and with the second frame pointer null: +, -, x and max only, so bit-equal."""
    a, b = V.batch_frames(W, H, K)
    for tag, bb in (("2", b), ("1", None)):
        rec = V.host_moments(a, bb)
        assert np.array_equal(torch_side[f"{W}x{H}_K{K}_rec{tag}"], rec)
        assert np.array_equal(torch_side[f"{W}x{H}_K{K}_var{tag}"], V.host_variance(rec, K))


def _dev(got, want, inp):
    return float(np.abs(got.astype(np.float64) - want).max() / np.abs(inp).max())


@pytest.mark.parametrize("W,H", V.FRAMES)
def test_filter_matches_host_build(W, H, torch_side):
    """Levels 0, 1, 3, 5, colour and variance, and d_out == d_color with d_var_out == d_var. Measured
    on the GPU, the largest deviation relative to the input's maximum: 1.192e-7 (37x21; GPU_VS_HOST;
    the two builds differ by expf only). Asserted: 5 x that."""
    color, var, feat = V.synthetic(W, H)
    worst = 0.0
    for levels in (0, 1, 3, 5):
        wc, wv = V.host_filter(color, var, feat, levels, **V.SIG)
        gc, gv = torch_side[f"{W}x{H}_L{levels}_c"], torch_side[f"{W}x{H}_L{levels}_v"]
        dc, dv = _dev(gc, wc, color), _dev(gv, wv, var)
        print(f"{W}x{H} levels {levels}: colour {dc:.3e} variance {dv:.3e}")
        worst = max(worst, dc, dv)
        assert np.array_equal(torch_side[f"{W}x{H}_L{levels}_inplace_c"], gc)
        assert np.array_equal(torch_side[f"{W}x{H}_L{levels}_inplace_v"], gv)
    print(f"{W}x{H}: worst {worst:.3e}")
    assert worst <= 5 * GPU_VS_HOST


@pytest.mark.parametrize("W,H", V.FRAMES)
def test_exact_properties_hold_on_the_gpu(W, H, torch_side):
    """They do not depend on expf's last bit: the levels-0 identity of colour and variance, constant
    in / constant out, v_out <= the largest tap, zero variance with distinct colours returns the
    colour bit for bit, huge sigmas give the plain B3 blur and sum h^2 v / (sum h)^2, and no leak
    across opposite normals."""
    from test_denoise import b3_blur
    from test_variance import b3_variance
    color, var, feat = V.synthetic(W, H)
    for tag in ("L0", "L0_inplace"):
        assert np.array_equal(torch_side[f"{W}x{H}_{tag}_c"], color)
        assert np.array_equal(torch_side[f"{W}x{H}_{tag}_v"], var)
    for levels in (1, 5):
        out = torch_side[f"{W}x{H}_const_L{levels}_c"]
        assert np.abs(out.astype(np.float64) - float(np.float32(0.7))).max() <= 32 * 2.0 ** -24 * levels * 0.7
    big_var = var + np.float32(0.1)
    for levels in (1, 3, 5):
        assert (torch_side[f"{W}x{H}_L{levels}_v"].astype(np.float64) <= V.tap_max(var, levels)).all()
        assert (torch_side[f"{W}x{H}_big_L{levels}_v"].astype(np.float64) <= V.tap_max(big_var, levels)).all()
        assert np.array_equal(torch_side[f"{W}x{H}_zero_L{levels}_c"], V.distinct_colors(W, H))
        assert (torch_side[f"{W}x{H}_zero_L{levels}_v"] == 0).all()
        assert _dev(torch_side[f"{W}x{H}_big_L{levels}_c"], b3_blur(color, levels), color) <= 5 * V.FP32_VS_FP64
        assert _dev(torch_side[f"{W}x{H}_big_L{levels}_v"], b3_variance(big_var, levels), big_var) <= 5 * V.FP32_VS_FP64
    lc, _, _, left = V.leak_inputs(W, H)
    out = torch_side[f"{W}x{H}_leak_c"]
    assert np.isfinite(out).all()
    for side in (left, ~left):
        if side.any():
            lo, hi = lc[:, side].min((0, 1)), lc[:, side].max((0, 1))
            assert np.all(out[:, side] >= lo) and np.all(out[:, side] <= hi)


# ------------------------------------------------------------------------------------------------
# the context path: CBspheres 16x12, 8 spp, m5, 4 batches

def _ctx_scene():
    return PB.full_view("CBspheres", CTX["W"], CTX["H"])


@pytest.fixture(scope="module")
def batch_refs():
    """The CPU build of the device code (bit-equal to oracle mode 2) on the context's four sample
    ranges and on all eight samples: float64 frames and splat counts. Computed once, read-only."""
    W, H, S, M, K = (CTX[k] for k in ("W", "H", "S", "M", "K"))
    per = S // K
    refs = [PB.render_rec(_ctx_scene(), W, H, S, M, seed=CTX["seed"], s0=k * per, count=per) for k in range(K)]
    one = PB.render_rec(_ctx_scene(), W, H, S, M, seed=CTX["seed"])
    for r in refs + [one]:
        assert r["vmin"] >= 0
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return refs, one


def test_batched_frames_obey_the_one_shot_bound(torch_side, batch_refs):
    """render_batches changes only the order of the atomic adds: the eye, light and sample frames
    lie within _pixelbound's per-pixel bound of the one-shot reference, no pixel outside. The
    batches' references add up to the one-shot reference to 1e-12."""
    refs, one = batch_refs
    assert np.abs(sum(r["eye"] + r["light"] for r in refs) - (one["eye"] + one["light"])).max() <= 1e-12
    e, l = PB.lit_share(one)
    assert e > 0.5 and l > 0.5
    g = {k: torch_side["ctx_" + k].astype(np.float64) for k in ("sample", "eye", "light")}
    PB.check_frames(g, one, CTX["S"], CTX["M"], "render_batches 16x12 s8 K4")


def test_record_and_variance_equal_the_host_build(torch_side):
    """read_moments()[..., :3] is read_frame(FRAME_SAMPLE) bit for bit (moments_add adds eye + light
    as k_combine does), and read_variance() is the host build's variance_of on that record."""
    rec = torch_side["ctx_moments"]
    assert np.array_equal(rec[..., :3], torch_side["ctx_sample"])
    assert (rec[..., 3] > 0).mean() > 0.5
    var = torch_side["ctx_variance"]
    assert np.array_equal(var, V.host_variance(rec, CTX["K"]))
    assert (var >= 0).all() and (var > 0).mean() > 0.5


def test_variance_matches_the_float64_estimator(torch_side, batch_refs):
    """The GPU's variance against v64 = K / (K - 1) (Q - |R|^2 / K) in float64 over the reference's
    batch increments r_k (R_k their running sum). Per channel, with u = 2^-24 and T_k
    _pixelbound's sample-frame bound of the cumulative frame after k batches (tol_eye at k S / K
    samples + tol_light at the cumulative splat count + u R_k; T_0 = 0): the GPU's cumulative
    frame F_k is within T_k of R_k, so its increment b_k = fl(F_k - F_{k-1}) is within
    d_k = T_k + T_{k-1} + u (r_k + T_k + T_{k-1}) of r_k, and |b_k|^2 within
    sum_c d (2 r + d) of |r_k|^2. The fp32 squares and sums add (K + 2) u Qh (a product, two adds,
    K - 1 adds of the running sum) with Qh = sum_k sum_c (r + d)^2; |F|^2 is within
    sum_c T_K (2 R + T_K) + 3 u Sh, Sh = sum_c (R + T_K)^2, times fl(1 / K): 2 u Sh / K more; the
    subtraction u (Qh + Sh / K); fl(K / (K - 1)) and its product 2u of the result. In total
        |v - v64| <= K / (K - 1) [dQ + dS / K + 2 u Sh / K + 3 u (Qh + Sh / K)],
    asserted with a factor 1.01 for the second-order terms. The clamp at 0 moves v towards
    v64 >= 0 only."""
    refs, _ = batch_refs
    S, M, K = CTX["S"], CTX["M"], CTX["K"]
    u = PB.U
    H, W = refs[0]["nsplat"].shape
    Re, Rl, N = np.zeros((H, W, 3)), np.zeros((H, W, 3)), np.zeros((H, W), np.int64)
    T_prev = np.zeros((H, W, 3))
    Q64, dQ, Qh = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W))
    for k, r in enumerate(refs):
        Re, Rl, N = Re + r["eye"], Rl + r["light"], N + r["nsplat"]
        T = PB.tol_of(Re, PB.eye_n((k + 1) * (S // K), M)) + PB.tol_of(Rl, N) + u * (Re + Rl)
        rk = r["eye"] + r["light"]
        d = T + T_prev + u * (rk + T + T_prev)
        Q64 += (rk ** 2).sum(-1)
        dQ += (d * (2 * rk + d)).sum(-1)
        Qh += ((rk + d) ** 2).sum(-1)
        T_prev = T
    R = Re + Rl
    dQ += (K + 2) * u * Qh
    Sh = ((R + T_prev) ** 2).sum(-1)
    dS = (T_prev * (2 * R + T_prev)).sum(-1) + 3 * u * Sh
    kk = K / (K - 1.0)
    bound = 1.01 * kk * (dQ + dS / K + 2 * u * Sh / K + 3 * u * (Qh + Sh / K))
    v64 = V.ref_variance(R, Q64, K)
    err = np.abs(torch_side["ctx_variance"].astype(np.float64) - v64)
    lit = v64 > 0
    print(f"variance vs float64 estimator: max err / bound {(err[lit] / bound[lit]).max():.4f}, "
          f"median bound / v64 {np.median(bound[lit] / v64[lit]):.3e}, lit {lit.mean():.2f}")
    assert lit.mean() > 0.5
    assert (err <= bound).all()
    assert (torch_side["ctx_variance"][v64 == 0] == 0).all()


def test_context_path_equals_buffer_path(torch_side):
    """bdpt_denoise_variance(ctx) = bdpt_denoise_variance_buffers on that context's own sample,
    variance and feature frames (raw device pointers, torch's stream): bit-equal; and both are the
    host build's result to the filter's GPU tolerance."""
    got = torch_side["ctx_denoised"]
    assert np.array_equal(got, torch_side["ctx_buffers"])
    assert not np.array_equal(got, torch_side["ctx_sample"])
    want, _ = V.host_filter(torch_side["ctx_sample"], torch_side["ctx_variance"], torch_side["ctx_features"], **V.defaults())
    assert np.abs(got - want).max() <= 5 * GPU_VS_HOST * np.abs(torch_side["ctx_sample"]).max()


# ------------------------------------------------------------------------------------------------
# error paths

def _err(r):
    return r.lib.bdpt_last_error()


def test_error_paths():
    W, H = 16, 12
    sc = golden_scene("CBspheres")
    buf = np.zeros((H, W, 4), np.float32)
    p = r = None
    try:
        p = B.PathTracer(sc, W, H, 4, 5, seed=3, max_tolerance=0.0, samples_per_batch=4)
        assert p.lib.bdpt_render_batches(p.ctx, 0, 4, 2) == B.BDPT_E_UNSUPPORTED
        assert b"PathTracer" in _err(p)
        r = B.BidirectionalPathTracer(sc, W, H, 8, 5, seed=3)
        L = r.lib
        assert L.bdpt_render_batches(r.ctx, 0, 8, 1) == B.BDPT_E_INVALID and b"2 batches" in _err(r)
        assert L.bdpt_render_batches(r.ctx, 0, 7, 2) == B.BDPT_E_INVALID and b"multiple" in _err(r)
        assert L.bdpt_read_moments(r.ctx, buf.ctypes.data_as(PF)) == B.BDPT_E_INVALID
        assert L.bdpt_variance(r.ctx) == B.BDPT_E_INVALID and b"2 batches" in _err(r)
        # a plain render marks the frame
        r.raytrace_tiles()
        assert L.bdpt_variance(r.ctx) == B.BDPT_E_INVALID and b"not rendered in batches" in _err(r)
        r.render_batches(0, 8, 4)
        assert L.bdpt_variance(r.ctx) == B.BDPT_E_INVALID and b"not rendered in batches" in _err(r)
        # bdpt_clear re-arms everything
        r.clear()
        assert L.bdpt_variance(r.ctx) == B.BDPT_E_INVALID and b"2 batches" in _err(r)
        assert (r.read_moments() == 0).all()
        r.render_batches(0, 4, 2)
        # filtering before a feature pass, and before a variance
        assert L.bdpt_denoise_variance(r.ctx, None) == B.BDPT_E_INVALID and b"feature pass" in _err(r)
        r.render_features()
        assert L.bdpt_denoise_variance(r.ctx, None) == B.BDPT_E_INVALID and b"variance" in _err(r)
        assert L.bdpt_read_variance(r.ctx, buf.ctypes.data_as(PF)) == B.BDPT_E_INVALID
        # another batch size
        assert L.bdpt_render_batches(r.ctx, 4, 4, 4) == B.BDPT_E_INVALID and b"batches of 2" in _err(r)
        r.render_batches(4, 4, 2)   # the same size: four batches now
        r.variance()
        assert np.array_equal(r.read_variance(), V.host_variance(r.read_moments(), 4))
        assert np.isfinite(r.denoise_variance()).all()
        bad = B.denoise_variance_params()
        bad.reserved[3] = 1
        assert L.bdpt_denoise_variance(r.ctx, C.byref(bad)) == B.BDPT_E_INVALID
        bad = B.denoise_variance_params(levels=9)
        assert L.bdpt_denoise_variance(r.ctx, C.byref(bad)) == B.BDPT_E_INVALID
        r.clear()
        assert L.bdpt_read_variance(r.ctx, buf.ctypes.data_as(PF)) == B.BDPT_E_INVALID
        r.render_batches(0, 8, 2)   # another batch size after a clear
        r.variance()
        assert (r.read_variance() >= 0).all()
    finally:
        for x in (p, r):
            if x is not None:
                x.close()


# ------------------------------------------------------------------------------------------------
RHO_VAR = 0.510   # measured on the GPU (docstring below)


def test_it_denoises():
    """test_gpu_denoise.py::test_it_denoises' setup under BDPT: CBspheres_lambertian 96x72 at depth
    5, R = 512 spp at seed 77, A = 8 spp at seed 5489 rendered as 4 batches, D = A through the
    variance-guided filter at its defaults. Measured on an MI355X: rho_var = RMSE(D, R) / RMSE(A, R)
    = 0.510 (RMSE 0.0638 -> 0.0325; the plain filter on the same frame: 0.588), the mean v 1.259e-2
    against a mean squared error to R of 1.222e-2. Asserted: RMSE(D, R) <= RMSE(A, R) (1 + rho_var) / 2,
    half the measured gain, so another seed's noise does not flip it. The plain filter's rho is
    printed beside it."""
    W, H = 96, 72
    sc = golden_scene("CBspheres_lambertian")
    r = B.BidirectionalPathTracer(sc, W, H, 512, 5, seed=77)
    try:
        r.raytrace_tiles()
        ref = r.read_frame(B.FRAME_SAMPLE)
    finally:
        r.close()
    r = B.BidirectionalPathTracer(sc, W, H, 8, 5, seed=5489)
    try:
        r.render_batches(0, 8, 4)
        a = r.read_frame(B.FRAME_SAMPLE)
        r.variance()
        var = r.read_variance()
        r.render_features()
        d = r.denoise_variance()
        plain = r.denoise()
    finally:
        r.close()
    ea, ed, ep = D.rmse(a, ref), D.rmse(d, ref), D.rmse(plain, ref)
    mse = float(np.mean(((a.astype(np.float64) - ref) ** 2).sum(-1)))
    print(f"BDPT: RMSE(A, R) {ea:.4f} RMSE(D, R) {ed:.4f} rho_var {ed / ea:.3f}; plain filter rho {ep / ea:.3f}; "
          f"mean v {var.mean():.4e} against the squared error to R {mse:.4e}")
    assert np.isfinite(d).all()
    assert ed <= ea * (1 + RHO_VAR) / 2
