"""Helpers of the adaptive-sampling tests: the host build of csrc/bdpt_adaptive.h
(tests/native/libcorecpu_adaptive.so), synthetic renders in rounds with unequal K_b and M_r, float64
restatements of the records, the estimate and the stopping rule with their derived fp32 error
bounds, and a driver that runs the adaptive loop over the CPU build of the device code."""
import ctypes as C
import os

import numpy as np

from _util import REPO

SO = os.path.join(REPO, "tests", "native", "libcorecpu_adaptive.so")
PF, PI = C.POINTER(C.c_float), C.POINTER(C.c_int)
FRAMES = [(37, 21), (8, 8), (1, 1), (64, 3)]
U = 2.0 ** -24
Z2 = float(np.float32(3.8416))
# the GPU conformance configuration (CBspheres, the golden camera's full view)
CONF = dict(W=20, H=20, S=32, m=2, min_rounds=4, max_rounds=16, tol=0.3, seed=5489, M=5)
# its schedule on the CPU build: K_b over the 3x3 blocks, and N
CONF_KB = [16, 16, 11, 6, 4, 9, 12, 4, 16]
CONF_N = 8192

_lib = None


def lib():
    global _lib
    if _lib is None:
        import __graft_entry__ as ge
        ge.build_core_cpu_adaptive()
        L = C.CDLL(SO)
        L.core_cpu_adaptive_moments.argtypes = [PF, PF, PF, PF, C.c_longlong, C.c_longlong]
        L.core_cpu_adaptive_decide.argtypes = [PF, PF, PI, PI, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong,
                                               C.c_float, C.c_int, PF]
        L.core_cpu_adaptive_compact.argtypes = [PI, C.c_int, C.c_int, PI, PI]
        L.core_cpu_adaptive_resolve.argtypes = [PF, PF, PI, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong,
                                                PF, PF, PI]
        L.core_cpu_adaptive_defaults.argtypes = [PI, PF]
        L.core_cpu_adaptive_defaults.restype = None
        _lib = L
    return _lib


def _f(a):
    return a.ctypes.data_as(PF)


def _i(a):
    return a.ctypes.data_as(PI)


def grid(W, H):
    """(nbx, nby)."""
    return (W + 7) // 8, (H + 7) // 8


def block_ids(W, H):
    """(H, W) int: the 8x8 block of every pixel, in bdpt_render's whole-frame order."""
    nbx, _ = grid(W, H)
    return (np.arange(H)[:, None] // 8) * nbx + (np.arange(W)[None, :] // 8)


def block_pixels(W, H):
    """In-frame pixels of every block."""
    nbx, nby = grid(W, H)
    return np.bincount(block_ids(W, H).ravel(), minlength=nbx * nby)


def defaults():
    n, t = (C.c_int * 2)(), (C.c_float * 1)()
    lib().core_cpu_adaptive_defaults(n, t)
    return dict(samples_per_round=n[0], min_rounds=n[1], tolerance=t[0])


# ------------------------------------------------------------------------------------------------
# the host build

def host_moments(eye, light, rec_e, rec_l, round_samples):
    """One round into copies of the records (H, W, 4): returns (rec_e, rec_l)."""
    eye, light = np.ascontiguousarray(eye, np.float32), np.ascontiguousarray(light, np.float32)
    rec_e, rec_l = np.array(rec_e, np.float32, order="C"), np.array(rec_l, np.float32, order="C")
    H, W = eye.shape[:2]
    rc = lib().core_cpu_adaptive_moments(_f(eye), _f(light), _f(rec_e), _f(rec_l), W * H, int(round_samples))
    assert rc == 0, rc
    return rec_e, rec_l


def host_decide(rec_e, rec_l, rounds, active, S, m, R, N, tol, decide=True):
    """(rounds, active, sums (nblocks, 2) = {Sv, Sc} of the evaluated blocks, nan elsewhere)."""
    rec_e, rec_l = np.ascontiguousarray(rec_e, np.float32), np.ascontiguousarray(rec_l, np.float32)
    H, W = rec_e.shape[:2]
    rounds, active = np.array(rounds, np.int32).ravel(), np.array(active, np.int32).ravel()
    sums = np.full((rounds.size, 2), np.nan, np.float32)
    rc = lib().core_cpu_adaptive_decide(_f(rec_e), _f(rec_l), _i(rounds), _i(active), W, H, S, m, R, int(N), tol,
                                        1 if decide else 0, _f(sums))
    assert rc == 0, rc
    return rounds, active, sums


def host_compact(active, W, H):
    """(list (n, 4) int32 {x, y, w, h}, (blocks, pixels))."""
    active = np.ascontiguousarray(active, np.int32).ravel()
    nbx, nby = grid(W, H)
    assert active.size == nbx * nby
    lst, cnt = np.full((nbx * nby, 4), -1, np.int32), np.zeros(2, np.int32)
    rc = lib().core_cpu_adaptive_compact(_i(active), W, H, _i(lst), _i(cnt))
    assert rc == 0, rc
    assert (lst[cnt[0]:] == -1).all()   # nothing written past the count
    return lst[:cnt[0]].copy(), (int(cnt[0]), int(cnt[1]))


def host_resolve(rec_e, rec_l, rounds, S, m, R, N):
    """(colour (H, W, 3), variance (H, W), counts (H, W) int32)."""
    rec_e, rec_l = np.ascontiguousarray(rec_e, np.float32), np.ascontiguousarray(rec_l, np.float32)
    rounds = np.ascontiguousarray(rounds, np.int32).ravel()
    H, W = rec_e.shape[:2]
    c, v, n = np.empty((H, W, 3), np.float32), np.empty((H, W), np.float32), np.empty((H, W), np.int32)
    rc = lib().core_cpu_adaptive_resolve(_f(rec_e), _f(rec_l), _i(rounds), W, H, S, m, R, int(N), _f(c), _f(v), _i(n))
    assert rc == 0, rc
    return c, v, n


def expected_list(active, W, H):
    """The compaction's definition in numpy: the active blocks in block order, clipped."""
    nbx, _ = grid(W, H)
    out = []
    for b in np.flatnonzero(np.asarray(active).ravel()):
        x0, y0 = (b % nbx) * 8, (b // nbx) * 8
        out.append((x0, y0, min(8, W - x0), min(8, H - y0)))
    lst = np.array(out, np.int32).reshape(-1, 4)
    return lst, (len(out), int((lst[:, 2] * lst[:, 3]).sum()))


# ------------------------------------------------------------------------------------------------
# synthetic renders in rounds

def schedule(W, H, R, pattern="mixed"):
    """K_b per block for a render of R rounds: 'mixed' spreads 2 .. R over the blocks with block 0 at R
    (a 1-block frame runs all R rounds); 'k24' alternates 2 and 4 (R >= 4)."""
    nbx, nby = grid(W, H)
    b = np.arange(nbx * nby)
    if pattern == "k24":
        return np.where(b % 2 == 0, 4, 2).astype(np.int32)
    return (R - (b * 5) % (R - 1)).astype(np.int32)


def synthetic_run(W, H, S, m, R, seed=3, pattern="mixed", identical=False, noise=None):
    """A render of R rounds with the prescribed schedule: per round the cumulative fp32 eye and light
    frames (the eye frame grows in the active blocks only, the light frame everywhere, in proportion to
    the round's pixel-samples), M_r and the active flags. identical: every round adds one 20-bit
    increment per pixel to the eye frame (exact cumulative frames). noise (nblocks,): the eye
    increments' spread per block, default 1. Returns dict(eye, light, M, active, K, N)."""
    rng = np.random.default_rng(seed + 1000 * W + 10 * H + R)
    K = schedule(W, H, R, pattern)
    bid, npx = block_ids(W, H), block_pixels(W, H)
    noise = np.ones(K.size) if noise is None else np.asarray(noise, np.float64)
    E, L = np.zeros((H, W, 3), np.float32), np.zeros((H, W, 3), np.float32)
    inc = np.floor(rng.uniform(0, 1, (H, W, 3)) * 2.0 ** 20) / 2.0 ** 20
    out = dict(eye=[], light=[], M=[], active=[], K=K)
    for r in range(R):
        act = K > r
        M = int(npx[act].sum()) * m
        if not identical:
            inc = 0.5 + noise[bid][..., None] * (rng.uniform(0, 1, (H, W, 3)) - 0.5)
        E = (E + np.where(act[bid][..., None], inc * (m / S), 0.0).astype(np.float32)).astype(np.float32)
        L = (L + (rng.uniform(0, 0.5, (H, W, 3)) * (M / (S * W * H))).astype(np.float32)).astype(np.float32)
        out["eye"].append(E.copy())
        out["light"].append(L.copy())
        out["M"].append(M)
        out["active"].append(act.astype(np.int32))
    out["N"] = int(sum(out["M"]))
    return out


def host_records(run):
    """The two records after every round of a synthetic_run()."""
    H, W = run["eye"][0].shape[:2]
    re, rl = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32)
    for e, l, M in zip(run["eye"], run["light"], run["M"]):
        re, rl = host_moments(e, l, re, rl, M)
    return re, rl


# ------------------------------------------------------------------------------------------------
# float64

def ref_records(run):
    """float64 over the fp32 cumulative frames: (Q_E, Q_L) (H, W); the weight is fl(1 / M_r) as stored
    (the host rounds it once: a given of the definition, not an error of the record)."""
    pe, pl = np.zeros(run["eye"][0].shape), np.zeros(run["eye"][0].shape)
    QE, QL = np.zeros(pe.shape[:2]), np.zeros(pe.shape[:2])
    for e, l, M in zip(run["eye"], run["light"], run["M"]):
        e, l = np.asarray(e, np.float64), np.asarray(l, np.float64)
        QE += ((e - pe) ** 2).sum(-1)
        QL += ((l - pl) ** 2).sum(-1) * float(np.float32(1.0 / M))
        pe, pl = e, l
    return QE, QL


def ref_estimate(rec_e, rec_l, K, W, H, S, m, R, N):
    """The definition in float64 over fp32 records: dict(c, vE, vL, v, scaleE, scaleL, cabs) with
    scaleE = (Q_E + |E|^2 / K) a^2 K / (K - 1) and scaleL = (Q_L + |L|^2 / N) g^2 N / (R - 1), what the
    rounding errors of vE and vL are relative to, and cabs = |a E| + |g L| per channel."""
    re, rl = np.asarray(rec_e, np.float64), np.asarray(rec_l, np.float64)
    Kp = np.asarray(K, np.float64).ravel()[block_ids(W, H)]
    a = S / (Kp * m)
    g = S * W * H / N
    sE, sL = (re[..., :3] ** 2).sum(-1), (rl[..., :3] ** 2).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        fe = np.where(Kp > 1, a * a * Kp / (Kp - 1), 0.0)
    fl = g * g * N / (R - 1)
    return dict(c=a[..., None] * re[..., :3] + g * rl[..., :3],
                vE=fe * np.maximum(0.0, re[..., 3] - sE / Kp), vL=fl * np.maximum(0.0, rl[..., 3] - sL / N),
                v=fe * np.maximum(0.0, re[..., 3] - sE / Kp) + fl * np.maximum(0.0, rl[..., 3] - sL / N),
                scaleE=fe * (re[..., 3] + sE / Kp), scaleL=fl * (rl[..., 3] + sL / N),
                cabs=np.abs(a[..., None] * re[..., :3]) + np.abs(g * rl[..., :3]), K=Kp)


def v_bound(est, R=None):
    """|v_fp32 - v_64| per pixel, u = 2^-24, first-order counts. Given the fp32 records (R None):
    |E|^2 is a product and two adds, 3u, times fl(1 / K) (u) by one product (u): 5u |E|^2 / K; the
    subtraction adds u (Q_E + |E|^2 / K): at most 6u (Q_E + |E|^2 / K). The factor: a = fl(S / (K m))
    u (K m is exact), a a 3u, fl(K / (K - 1)) u, their product u, the last product u: 6u of the result.
    vE: 12u scaleE. vL: 5u |L|^2 / N as before (1 / N is rounded once on the host), the subtraction u,
    g^2 N / (R - 1) rounded once (u) and its product (u): 8u scaleL. The sum: u (vE + vL). Asserted
    with 13 and 9 for the second-order terms. From the frames (R given) the records' own errors come
    on top: Q_E as DESIGN.md §12's Q with the rounds for the batches, (R + 4) u Q_E; Q_L with one more
    product per term, (R + 5) u Q_L. The clamps at 0 move v towards v_64 >= 0 only."""
    ke, kl = (13, 9) if R is None else (13 + R + 4, 9 + R + 5)
    return U * (ke * est["scaleE"] + kl * est["scaleL"] + est["v"])


def c_bound(est):
    """|c_fp32 - c_64| per channel: fl(a) u, its product u, fl(g) u, its product u, the add u:
    at most 3 u (|a E| + |g L|) to first order; asserted with 4."""
    return 4 * U * est["cabs"]


def ref_decide(est, W, H, tol, R):
    """Per block: (stop64 (bool), clear (bool)): the rule in float64 over the float64 estimate, and
    whether its margin exceeds the fp32 error bound of the two sums. Sv: the per-pixel bound of v plus
    the butterfly's six adds of non-negative terms, 6 u Sv. Sc: per pixel the three channels' c bounds
    plus the two adds of (c.x + c.y) + c.z, 2 u, and the butterfly's 6 u, on sums of non-negative
    terms. LHS = fl(fl(Z2 Sv) fl(3 n)): 2 u more; RHS = fl(t t), t = fl(tol Sc): 3 u more."""
    bid, npx = block_ids(W, H).ravel(), block_pixels(W, H)
    nb = npx.size
    tol = float(np.float32(tol))
    Sv = np.bincount(bid, est["v"].ravel(), nb)
    dSv = np.bincount(bid, v_bound(est).ravel(), nb) + 6 * U * Sv
    Sc = np.bincount(bid, est["c"].sum(-1).ravel(), nb)
    Sabs = np.bincount(bid, est["cabs"].sum(-1).ravel(), nb)
    dSc = np.bincount(bid, c_bound(est).sum(-1).ravel(), nb) + 8 * U * Sabs
    lhs, rhs = Z2 * Sv * (3 * npx), (tol * Sc) ** 2
    dl = Z2 * (3 * npx) * dSv + 2 * U * lhs
    dr = 2 * tol * tol * np.abs(Sc) * dSc + (tol * dSc) ** 2 + 3 * U * rhs
    return lhs <= rhs, np.abs(lhs - rhs) > 1.01 * (dl + dr), lhs, rhs


# ------------------------------------------------------------------------------------------------
# the adaptive loop over the CPU build of the device code

def cpu_adaptive(scene, W, H, S, m, min_rounds, max_rounds, tol, seed, M=5, keep=False):
    """bdpt_render_adaptive's loop with _pixelbound.render_rec as the renderer (round r renders samples
    [r m, (r + 1) m) of the active blocks' pixels) and the host build for the records, the decision and
    the resolve. The cumulative frames are float64 sums of the rounds' frames, rounded to fp32 for the
    records. Returns dict(eye, light (float64), nsplat, K, N, R, active, nactive (per round), color,
    variance, counts, rec_e, rec_l[, per_round: the records and flags after every round])."""
    import _pixelbound as PB
    nbx, nby = grid(W, H)
    bid = block_ids(W, H)
    K, active = np.zeros(nbx * nby, np.int32), np.ones(nbx * nby, np.int32)
    E, L, ns = np.zeros((H, W, 3)), np.zeros((H, W, 3)), np.zeros((H, W), np.int64)
    re, rl = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32)
    N, R, nactive, per_round = 0, 0, [], []
    while True:
        nactive.append(int(active.sum()))
        on = active[bid] != 0
        pix = [(x, y) for y in range(H) for x in range(W) if on[y, x]]
        r = PB.render_rec(scene, W, H, S, M, seed=seed, s0=R * m, count=m, pixels=pix)
        assert r["vmin"] >= 0
        E, L, ns = E + r["eye"], L + r["light"], ns + r["nsplat"]
        Mr = len(pix) * m
        N += Mr
        R += 1
        re, rl = host_moments(E.astype(np.float32), L.astype(np.float32), re, rl, Mr)
        K, active, _ = host_decide(re, rl, K, active, S, m, R, N, tol, decide=R >= min_rounds)
        if keep:
            per_round.append((re.copy(), rl.copy(), K.copy(), active.copy(), N))
        if not active.any() or R == max_rounds:
            break
    c, v, cnt = host_resolve(re, rl, K, S, m, R, N)
    return dict(eye=E, light=L, nsplat=ns, K=K, N=N, R=R, active=active, nactive=nactive, color=c, variance=v, counts=cnt,
                rec_e=re, rec_l=rl, per_round=per_round)


def replay(scene, W, H, S, m, K, seed, M=5, render=None):
    """The CPU build on a given schedule: round r renders the pixels of {b : K_b > r} with s0 = r m,
    count = m. render(s0, count, pixels) -> {"eye", "light"[, "nsplat"]} replaces
    _pixelbound.render_rec (the thin-lens build). Returns a render_rec()-shaped dict of float64 sums
    and N."""
    import _pixelbound as PB
    K = np.asarray(K).ravel()
    bid = block_ids(W, H)
    E, L, ns, N = np.zeros((H, W, 3)), np.zeros((H, W, 3)), np.zeros((H, W), np.int64), 0
    for r in range(int(K.max())):
        on = K[bid] > r
        pix = [(x, y) for y in range(H) for x in range(W) if on[y, x]]
        if render is None:
            rr = PB.render_rec(scene, W, H, S, M, seed=seed, s0=r * m, count=m, pixels=pix)
            assert rr["vmin"] >= 0
        else:
            rr = render(r * m, m, pix)
        E, L = E + rr["eye"], L + rr["light"]
        ns = ns + rr.get("nsplat", 0)
        N += len(pix) * m
    return {"eye": E, "light": L, "nsplat": ns}, N


def lens_render_pixels(scene, W, H, S, M, seed, s0, count, pixels, lens_radius, focal_distance):
    """tests/native/core_cpu_lens.cpp on a pixel list: {"eye", "light"} float64 (no splat counts)."""
    import _lens
    px = np.ascontiguousarray(pixels, dtype=np.int32).reshape(-1, 2)
    eye, light, st = np.zeros((H, W, 3)), np.zeros((H, W, 3)), np.zeros(10)
    d = scene.desc()
    pd = C.POINTER(C.c_double)
    rc = _lens.core_lens().core_cpu_lens_render(C.byref(d), W, H, S, M, seed, s0, count, px.ctypes.data_as(PI), px.shape[0],
                                                eye.ctypes.data_as(pd), light.ctypes.data_as(pd), st.ctypes.data_as(pd), 0, 0, 1,
                                                1, lens_radius, focal_distance)
    assert rc == 0 and st[7] == 3, (rc, st[7])
    return {"eye": eye, "light": light}


def block_rel_error(D, ref):
    """Per 8x8 block the RMS per-channel error of D against ref over the block's mean channel value
    of ref."""
    H, W = ref.shape[:2]
    bid, npx = block_ids(W, H).ravel(), block_pixels(W, H)
    D, ref = np.asarray(D, np.float64), np.asarray(ref, np.float64)
    e = np.bincount(bid, ((D - ref) ** 2).sum(-1).ravel(), npx.size)
    mu = np.bincount(bid, ref.sum(-1).ravel(), npx.size) / (3 * npx)
    return np.sqrt(e / (3 * npx)) / np.maximum(mu, 1e-9)
