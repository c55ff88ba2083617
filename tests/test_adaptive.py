"""Adaptive sampling under BDPT on the host build of csrc/bdpt_adaptive.h: the records
and the estimate against float64 within derived bounds, the stopping rule against a float64
evaluation, the compaction against its definition, the adaptive loop over the CPU build of the
device code (schedule, uniform case, estimator), the C-ABI's error paths that touch no device, and a
run under ASan + UBSan. No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import bdpt_amd as B
import _adaptive as A
import _pixelbound as PB
from _util import REPO

S_SYN, M_SYN, R_SYN = 24, 2, 7   # the synthetic renders: 7 rounds of 2 samples of a 24-spp context


@pytest.mark.parametrize("W,H", A.FRAMES)
def test_records_and_estimate_match_float64(W, H):
    """fp32 host build vs float64 on the same fp32 cumulative frames, K_b spread over 2 .. 7 and M_r
    unequal. Records: prev is the frame; Q_E within (R + 4) u Q_E (DESIGN.md §12's count with the
    rounds for the batches), Q_L within (R + 5) u Q_L (one more product per term, by the stored
    fl(1 / M_r)). Estimate: colour within 3u (|a E| + |g L|) (asserted with 4), variance within
    _adaptive.v_bound's u [(R + 17) scaleE + (R + 14) scaleL + v]; v >= 0; counts = K_b m."""
    run = A.synthetic_run(W, H, S_SYN, M_SYN, R_SYN)
    K, N = run["K"], run["N"]
    if K.size > 2:
        assert len(set(K.tolist())) >= 3 and len(set(run["M"])) >= 3   # unequal K_b and M_r
    re, rl = A.host_records(run)
    assert np.array_equal(re[..., :3], run["eye"][-1]) and np.array_equal(rl[..., :3], run["light"][-1])
    QE, QL = A.ref_records(run)
    assert (np.abs(re[..., 3] - QE) <= (R_SYN + 4) * A.U * QE).all()
    assert (np.abs(rl[..., 3] - QL) <= (R_SYN + 5) * A.U * QL).all()
    c, v, cnt = A.host_resolve(re, rl, K, S_SYN, M_SYN, R_SYN, N)
    re64, rl64 = re.astype(np.float64), rl.astype(np.float64)
    re64[..., 3], rl64[..., 3] = QE, QL
    est = A.ref_estimate(re64, rl64, K, W, H, S_SYN, M_SYN, R_SYN, N)
    ev, ec = np.abs(v - est["v"]), np.abs(c - est["c"])
    print(f"{W}x{H}: v max err / bound {(ev / A.v_bound(est, R_SYN)).max():.3f}, "
          f"c max err / bound {(ec / A.c_bound(est)).max():.3f}")
    assert (v >= 0).all() and v.max() > 0
    assert (ev <= A.v_bound(est, R_SYN)).all()
    assert (ec <= A.c_bound(est)).all()
    assert np.array_equal(cnt, (K[A.block_ids(W, H)] * M_SYN).astype(np.int32))


@pytest.mark.parametrize("W,H", A.FRAMES)
def test_identical_increments_have_zero_eye_variance(W, H):
    """K_b = 4 and 2 copies of one 20-bit increment per pixel, weight m / S = 1 / 4 (exact cumulative
    frames), the stopped blocks adding 0 afterwards: Q_E = K q and |E|^2 / K = K q exactly (DESIGN.md
    §12's argument at K = 2 and 4), so vE == 0 exactly and v is the light term alone."""
    S, m, R = 8, 2, 4
    run = A.synthetic_run(W, H, S, m, R, pattern="k24", identical=True)
    K, N = run["K"], run["N"]
    re, rl = A.host_records(run)
    _, v, _ = A.host_resolve(re, rl, K, S, m, R, N)
    zero_l = rl.copy()
    zero_l[..., 3] = 0   # Q_L = 0 clamps vL to 0: what is left is vE
    _, ve, _ = A.host_resolve(re, zero_l, K, S, m, R, N)
    assert (ve == 0).all()
    assert (re[..., 3] > 0).all() and (v > 0).any()


def _decision_cases():
    """Synthetic renders whose blocks differ in eye noise by a factor of 30 (their threshold tolerances
    spread over 0.14 .. 0.85), at tolerances that stop a quarter to three quarters of them:
    (W, H, tol, seed)."""
    return [(W, H, tol, seed) for (W, H) in ((64, 40), (37, 21), (64, 3), (8, 8), (1, 1))
            for tol in (0.15, 0.2, 0.35) for seed in (1, 2, 3)]


def test_decision_matches_float64():
    """Every active block of every case: the fp32 decision equals the float64 evaluation of the rule
    wherever the float64 margin |LHS - RHS| exceeds the fp32 error bound of the two sums
    (_adaptive.ref_decide derives it). The blocks inside that margin are counted and are at most 5 % of
    the cases; both outcomes occur; K_b is counted for the active blocks only; a stopped block is left
    alone (its K_b in the records' estimate is the one it stopped at)."""
    total = unclear = stops = 0
    for W, H, tol, seed in _decision_cases():
        nb = A.block_pixels(W, H).size
        noise = 0.05 * 30.0 ** (np.arange(nb) % 7 / 6.0)
        run = A.synthetic_run(W, H, S_SYN, M_SYN, R_SYN, seed=seed, noise=noise)
        re, rl = A.host_records(run)
        K, N = run["K"], run["N"]
        # every block is asked, as if this had been its K_b-th round; every third one was stopped
        # before and must be left alone
        active = (np.arange(nb) % 3 != 2).astype(np.int32)
        before = K - active
        k2, a2, sums = A.host_decide(re, rl, before, active, S_SYN, M_SYN, R_SYN, N, tol)
        assert np.array_equal(k2, K)
        assert (a2[active == 0] == 0).all() and np.isnan(sums[active == 0]).all()
        est = A.ref_estimate(re, rl, K, W, H, S_SYN, M_SYN, R_SYN, N)
        stop64, clear, lhs, rhs = A.ref_decide(est, W, H, tol, R_SYN)
        on = active != 0
        got_stop = a2 == 0
        assert np.array_equal(got_stop[on & clear], stop64[on & clear]), (W, H, tol, seed)
        total += int(on.sum())
        unclear += int((on & ~clear).sum())
        stops += int((on & got_stop).sum())
        # the sums themselves against float64
        Sv = np.bincount(A.block_ids(W, H).ravel(), est["v"].ravel(), nb)
        assert np.allclose(sums[on, 0], Sv[on], rtol=1e-4, atol=0)
    print(f"decisions: {total} blocks, {stops} stopped, {unclear} inside the fp32 margin")
    assert total >= 100 and 0.2 * total <= stops <= 0.8 * total
    assert unclear <= 0.05 * total


def test_without_decide_only_the_rounds_are_counted():
    W, H = 37, 21
    nb = A.block_pixels(W, H).size
    rec = np.zeros((H, W, 4), np.float32)
    active = (np.arange(nb) % 2).astype(np.int32)
    k, a, _ = A.host_decide(rec, rec, np.full(nb, 3), active, 8, 2, 1, 1, 0.3, decide=False)
    assert np.array_equal(a, active) and np.array_equal(k, 3 + active)


@pytest.mark.parametrize("W,H", A.FRAMES)
def test_a_block_of_zeros_stops(W, H):
    """Sv = Sc = 0: 0 <= 0 holds, the block stops (nothing arrives in it, nothing ever will)."""
    nb = A.block_pixels(W, H).size
    rec = np.zeros((H, W, 4), np.float32)
    k, a, sums = A.host_decide(rec, rec, np.full(nb, 3), np.ones(nb), 8, 2, 4, 4 * W * H * 2, 0.3)
    assert (a == 0).all() and (k == 4).all() and (sums == 0).all()


def test_clipped_blocks_use_their_own_pixel_count():
    """37x21 with the same record in every pixel: Sv = n v and Sc = n s, so with its own n every block's
    LHS / RHS = 3.8416 x 3 v / (tol s)^2, whatever n. tol is set for LHS / RHS = 1 / 2: every block
    stops, the clipped ones too. With n = 64 in place of a clipped block's 5 x 5 pixels its ratio
    would be 64 / 25 x as large and it would go on. At tol / 2 (ratio 2) no block stops."""
    W, H, S, m, R = 37, 21, 8, 2, 4
    rng = np.random.default_rng(5)
    pat = rng.uniform(0.2, 1.0, (R, 3))          # one increment per round and channel, the same in every pixel
    re, rl = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32)
    E = np.zeros((H, W, 3), np.float32)
    for r in range(R):
        E = E + (pat[r] * (m / S)).astype(np.float32)
        re, rl = A.host_moments(E, np.zeros_like(E), re, rl, W * H * m)
    nb = A.block_pixels(W, H).size
    N = R * W * H * m
    est = A.ref_estimate(re, rl, np.full(nb, R), W, H, S, m, R, N)
    ratio = A.Z2 * est["v"][0, 0] * 3 / (est["c"][0, 0].sum() ** 2)   # LHS / RHS at tol 1, any n: n v 3n / (n c)^2
    tol = float(np.sqrt(2 * ratio))
    for t, stopped in ((tol, True), (tol / 2, False)):
        _, a, _ = A.host_decide(re, rl, np.full(nb, R - 1), np.ones(nb), S, m, R, N, t)
        assert ((a == 0) == stopped).all(), (t, a)


GRIDS = [(1, 1), (20, 20), (263, 250)]   # 1 block; 3x3 clipped; 33 x 32 = 1056 blocks, clipped


@pytest.mark.parametrize("W,H", GRIDS)
@pytest.mark.parametrize("pattern", ["all", "none", "one", "alternating", "random"])
def test_compaction(W, H, pattern):
    """The list is the active blocks in block order, clipped to the frame; the counts are the blocks
    and their in-frame pixels; nothing is written past the count."""
    active = compaction_flags(W, H, pattern)
    lst, cnt = A.host_compact(active, W, H)
    want, wcnt = A.expected_list(active, W, H)
    assert np.array_equal(lst, want) and cnt == wcnt
    if pattern == "all":
        assert cnt == (active.size, W * H)


def compaction_flags(W, H, pattern):
    nb = A.block_pixels(W, H).size
    if pattern == "all":
        return np.ones(nb, np.int32)
    if pattern == "none":
        return np.zeros(nb, np.int32)
    if pattern == "one":
        a = np.zeros(nb, np.int32)
        a[nb - 1] = 1          # the clipped corner block
        return a
    if pattern == "alternating":
        return (np.arange(nb) % 2).astype(np.int32)
    return (np.random.default_rng(nb).uniform(size=nb) < 0.3).astype(np.int32) * 7   # any non-zero flag counts


# ------------------------------------------------------------------------------------------------
# the adaptive loop over the CPU build of the device code

@pytest.fixture(scope="module")
def conf_run():
    c = A.CONF
    sc = PB.full_view("CBspheres", c["W"], c["H"])
    return A.cpu_adaptive(sc, c["W"], c["H"], c["S"], c["m"], c["min_rounds"], c["max_rounds"], c["tol"], c["seed"], c["M"])


def test_conformance_schedule(conf_run):
    """CBspheres 20x20, S 32, m 2, min 4, max 16, tol 0.3, seed 5489 on the CPU build: the K_b and N
    recorded in DESIGN.md §13 (blocks stop at once, at later rounds, and three run to the cap)."""
    r = conf_run
    print("K_b", r["K"].tolist(), "N", r["N"], "active per round", r["nactive"])
    assert r["K"].tolist() == A.CONF_KB
    assert r["N"] == A.CONF_N
    assert r["nactive"] == [9, 9, 9, 9, 7, 7, 6, 6, 6, 5, 5, 4, 3, 3, 3, 3]
    assert r["R"] == 16 and int(r["active"].sum()) == 3
    assert np.array_equal(r["counts"], (r["K"][A.block_ids(20, 20)] * 2).astype(np.int32))


def test_uniform_rounds_give_the_plain_frame():
    """min_rounds == max_rounds == S / m: a_b = g = 1 exactly, so c == fl(E + L) bit for bit, counts
    are S and N = W H S. And v against DESIGN.md §12's batch variance of the same rounds (the moments
    of E + L): the two differ by the eye-light covariance of a pixel alone, which §13 leaves out;
    the ratio of the frame means is recorded there (measured 1.029 here; asserted within 10 %, the
    band of the estimator tests)."""
    import _variance as V
    W, H, S, m, M = 20, 20, 8, 2, 5
    sc = PB.full_view("CBspheres", W, H)
    r = A.cpu_adaptive(sc, W, H, S, m, S // m, S // m, 0.3, 5489, M, keep=True)
    assert r["R"] == S // m and r["N"] == W * H * S and (r["counts"] == S).all()
    e32, l32 = r["eye"].astype(np.float32), r["light"].astype(np.float32)
    assert np.array_equal(r["color"], e32 + l32)
    # §12 on the same rounds: the cumulative frames are the records' prev after each round
    cum = [(re[..., :3] + rl[..., :3]) for re, rl, _, _, _ in r["per_round"]]
    v12 = V.host_variance(V.host_moments(cum), S // m)
    ratio = float(r["variance"].mean() / v12.mean())
    print(f"mean v (no eye-light covariance) / mean v of DESIGN.md §12: {ratio:.4f}")
    assert 0.9 <= ratio <= 1.1


@pytest.mark.parametrize("S,min_rounds,tol", [(8, 4, 0.3), (32, 4, 0.3)], ids=["uniform", "tol0.3"])
def test_estimator_against_the_empirical_variance(S, min_rounds, tol):
    """CBspheres_lambertian 20x20 m5, m 2, seeds 1000..1063: the mean over pixels and seeds of v over
    the mean over pixels of the empirical trace variance of the 64 resolved frames lies in
    [0.9, 1.1], DESIGN.md §12's band. Uniform: S 8 in 4 rounds, every block active throughout;
    adaptive: S 32, min 4, max 16, tol 0.3."""
    W, H, m = 20, 20, 2
    sc = PB.full_view("CBspheres_lambertian", W, H)
    cols, vs, Ns = [], [], []
    for seed in range(1000, 1064):
        r = A.cpu_adaptive(sc, W, H, S, m, min_rounds, S // m, tol, seed)
        cols.append(r["color"].astype(np.float64))
        vs.append(r["variance"].astype(np.float64))
        Ns.append(r["N"])
    empirical = np.stack(cols).var(axis=0, ddof=1).sum(-1).mean()
    ratio = float(np.mean(vs) / empirical)
    print(f"S {S} min {min_rounds} tol {tol}: mean v / mean empirical variance {ratio:.4f}, mean N {np.mean(Ns):.0f}")
    if S == 8:
        assert all(n == W * H * S for n in Ns)
    else:
        assert np.mean(Ns) < 0.9 * W * H * S   # the rule does stop blocks
    assert 0.9 <= ratio <= 1.1


# ------------------------------------------------------------------------------------------------
# the C-ABI's error paths that touch no device

def _err(lib):
    return lib.bdpt_last_error()


def test_defaults_are_the_documented_ones():
    lib = B.load_library()
    p = B.AdaptiveParams()
    assert lib.bdpt_adaptive_default_params(None, C.byref(p)) == B.BDPT_OK
    d = A.defaults()
    assert (p.samples_per_round, p.min_rounds, p.max_rounds) == (d["samples_per_round"], d["min_rounds"], 0)
    assert (p.samples_per_round, p.min_rounds) == (32, 4) and abs(p.tolerance - 0.05) < 1e-9
    assert list(p.reserved) == [0, 0, 0, 0]
    assert lib.bdpt_adaptive_default_params(None, None) == B.BDPT_E_INVALID and b"null" in _err(lib)
    text = open(os.path.join(REPO, "DESIGN.md")).read()
    assert "samples_per_round 32, min_rounds 4, tolerance 0.05" in text


def test_error_paths_without_a_device():
    lib = B.load_library()
    INV = B.BDPT_E_INVALID
    one = C.c_void_p(16)   # a non-null, aligned stand-in: every call below fails before it is read
    odd = C.c_void_p(20)
    assert lib.bdpt_render_adaptive(None, None, None) == INV and b"null ctx" in _err(lib)
    assert lib.bdpt_adaptive_resolve(None) == INV
    assert lib.bdpt_read_adaptive(None, None, None, None) == INV
    assert lib.bdpt_adaptive_device_ptrs(None, None, None, None) == INV
    assert lib.bdpt_read_adaptive_rounds(None, None) == INV
    assert lib.bdpt_read_adaptive_active(None, None) == INV
    assert lib.bdpt_read_adaptive_records(None, None, None) == INV
    # moments
    assert lib.bdpt_adaptive_moments_buffers(0, None, one, one, one, 8, 8, 64, None) == INV and b"null" in _err(lib)
    assert lib.bdpt_adaptive_moments_buffers(0, one, one, one, one, 0, 8, 64, None) == INV and b"frame size" in _err(lib)
    assert lib.bdpt_adaptive_moments_buffers(-1, one, one, one, one, 8, 8, 64, None) == INV and b"ordinal" in _err(lib)
    assert lib.bdpt_adaptive_moments_buffers(0, one, one, one, one, 8, 8, 0, None) == INV and b"pixel-samples" in _err(lib)
    assert lib.bdpt_adaptive_moments_buffers(0, one, one, odd, one, 8, 8, 64, None) == INV and b"aligned" in _err(lib)
    # decide
    assert lib.bdpt_adaptive_decide_buffers(0, one, one, None, one, 8, 8, 8, 2, 4, 512, 0.3, 1, None) == INV
    assert lib.bdpt_adaptive_decide_buffers(0, one, one, one, one, 8, -1, 8, 2, 4, 512, 0.3, 1, None) == INV
    assert lib.bdpt_adaptive_decide_buffers(0, one, one, one, one, 8, 8, 8, 2, 1, 512, 0.3, 1, None) == INV and b"2 rounds" in _err(lib)
    assert lib.bdpt_adaptive_decide_buffers(0, one, one, one, one, 8, 8, 8, 0, 4, 512, 0.3, 1, None) == INV
    assert lib.bdpt_adaptive_decide_buffers(0, one, one, one, one, 8, 8, 8, 2, 4, 0, 0.3, 1, None) == INV
    assert lib.bdpt_adaptive_decide_buffers(0, one, one, one, one, 8, 8, 8, 2, 4, 512, -0.1, 1, None) == INV and b"tolerance" in _err(lib)
    assert lib.bdpt_adaptive_decide_buffers(0, one, one, one, one, 8, 8, 8, 2, 4, 512, float("nan"), 1, None) == INV
    assert lib.bdpt_adaptive_decide_buffers(0, one, odd, one, one, 8, 8, 8, 2, 4, 512, 0.3, 1, None) == INV and b"aligned" in _err(lib)
    # compact
    assert lib.bdpt_adaptive_compact_buffers(0, one, 8, 8, one, None, None) == INV and b"null" in _err(lib)
    assert lib.bdpt_adaptive_compact_buffers(0, one, 8, 0, one, one, None) == INV
    assert lib.bdpt_adaptive_compact_buffers(0, one, 8, 8, odd, one, None) == INV and b"aligned" in _err(lib)
    # resolve
    assert lib.bdpt_adaptive_resolve_buffers(0, one, one, one, 8, 8, 8, 2, 4, 512, one, one, None, None) == INV
    assert lib.bdpt_adaptive_resolve_buffers(0, one, one, one, 8, 8, 8, 2, 1, 512, one, one, one, None) == INV and b"2 rounds" in _err(lib)
    assert lib.bdpt_adaptive_resolve_buffers(0, one, one, one, 8, 8, 0, 2, 4, 512, one, one, one, None) == INV
    assert lib.bdpt_adaptive_resolve_buffers(-2, one, one, one, 8, 8, 8, 2, 4, 512, one, one, one, None) == INV


CSRC = os.path.join(REPO, "bidirectional-pathtracing_amd", "csrc")
NATIVE = os.path.join(REPO, "tests", "native")
SAN_FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-omit-frame-pointer",
             "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-I" + os.path.join(REPO, "include"), "-I" + CSRC]


@pytest.mark.slow
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_host_build_under_asan_ubsan(tmp_path):
    """tests/native/adaptive_probe.cpp: a synthetic render in rounds through the host moments, decision,
    compaction and resolve on the four frame sizes, every buffer at exactly its size, built with
    ASan + UBSan and run as a child process."""
    exe = str(tmp_path / "adaptive_probe")
    srcs = [os.path.join(NATIVE, "adaptive_probe.cpp"), os.path.join(NATIVE, "core_cpu_adaptive.cpp")]
    subprocess.run(["g++"] + SAN_FLAGS + ["-static-libasan", "-o", exe] + srcs, check=True, capture_output=True, text=True,
                   timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "no sanitizer report" in r.stdout
