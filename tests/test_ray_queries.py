"""Ray queries on generated geometry, CPU build of the device traversal (core_cpu_trace_rays, LDS
modes 0 / 1 / 2: the 4-wide tree, the binary tree, the 4-wide tree with its treelet) against two
references: oracle mode 2 (the reference's fp32 algorithm over its own BVH; bit-equal primitive and
t) and tests/_rayref.py brute_fp64 (float64, no tree; no wrong primitive among the rays it decides,
t within a bound). Scenes away from the Cornell boxes — other scales and offsets, overlapping
boxes, slivers, coincident copies, trees whose root is a leaf — finite [tmin, tmax] windows, odd
rays, and the traversal stack at its bound under ASan + UBSan (tests/native/stack_probe.cpp).
The GPU side is tests/test_gpu_ray_queries.py.

The bound on |t - t64| / t64 per scene is 4 x the largest deviation of ORACLE MODE 2 (not of the
code under test) from brute_fp64 on the same decided rays, the 4 for another libm and rounding
order. Measured with this file's ray sets (random_rays(name): 2000 rays, seed 17) by
test_closest_and_any_hit's own oracle pass, x86-64 g++ -O2 -ffp-contract=off:

    scene        undecided   oracle max |t - t64| / t64   bound (4 x)
    grid           0.05 %            8.608e-07             3.443e-06
    grid_1e3       0.05 %            2.436e-06             9.744e-06
    grid_off       0.05 %            5.730e-07             2.292e-06
    fan            1.35 %            8.982e-04             3.593e-03
    slivers        0.05 %            1.926e-07             7.704e-07
    stack          0.35 %            5.817e-08             2.327e-07
    same           0.00 %            7.965e-07 (tiny1)     3.186e-06
    tiny1          0.00 %            7.965e-07             3.186e-06
    tiny2          0.00 %            5.886e-06             2.354e-05
    tiny_sphere    0.00 %            5.333e-08             2.133e-07

(the deviations rounded up in their last digit). The oracle refuses same(64) (no extent between its
centroids); its triangle is tiny1's and its rays are tiny1's, so tiny1's oracle pass is its
reference: the same t, whichever copy is named.
Each test re-measures the oracle's deviation and asserts it is no larger than the table's."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _rayref as R
from _util import MODE_C32, REPO, oracle_render

CASES = ["grid", "grid_1e3", "grid_off", "fan", "slivers", "stack", "same", "tiny1", "tiny2", "tiny_sphere"]
LDS_MODES = [0, 1, 2]
UNDECIDED_MAX = 0.05
# oracle mode 2's largest |t - t64| / t64 on the decided rays (the table above)
ORACLE_DEV = {"grid": 8.608e-07, "grid_1e3": 2.436e-06, "grid_off": 5.730e-07, "fan": 8.982e-04,
              "slivers": 1.926e-07, "stack": 5.817e-08, "same": 7.965e-07, "tiny1": 7.965e-07,
              "tiny2": 5.886e-06, "tiny_sphere": 5.333e-08}

_refs = {}


def ref(name):
    """Scene, rays and both references of a case: computed once, shared, left unchanged."""
    if name not in _refs:
        sc, rays = R.scene(name), R.random_rays(name)
        p64, t64, dec = R.brute_fp64(sc, rays)
        osc = R.scene("tiny1") if name in R.ORACLE_REFUSES else sc
        ot, op = R.oracle_trace(osc, rays)
        if name in R.ORACLE_REFUSES:
            assert R.oracle_trace(sc, rays) is None
        _refs[name] = dict(sc=sc, rays=rays, p64=p64, t64=t64, dec=dec, ot=ot, op=op, canon=R.canonical(sc))
    return _refs[name]


def rel_dev(t, t64, m):
    return float((np.abs(t[m].astype(np.float64) - t64[m]) / t64[m]).max()) if m.any() else 0.0


def check_against_references(name, t, p, hit_any):
    """The assertions of case (a) on one tracer's closest hits (t, p) and any-hit flags."""
    r = ref(name)
    p64, t64, dec, ot, op = r["p64"], r["t64"], r["dec"], r["ot"], r["op"]
    und = float((~dec).mean())
    print(f"{name}: {len(dec)} rays, hits {(p64 >= 0).mean():.2f}, undecided {100 * und:.2f} %")
    assert und <= UNDECIDED_MAX
    assert (p64 >= 0).sum() >= len(dec) // 10 and (p64 < 0).sum() >= 10
    # the oracle itself against float64: no wrong primitive, and the deviation the bound comes from
    oc = r["canon"][np.maximum(op, 0)] if name not in R.ORACLE_REFUSES else op
    assert np.array_equal(np.where(op >= 0, oc, -1)[dec], p64[dec])
    odev = rel_dev(ot, t64, dec & (p64 >= 0))
    bound = 4 * ORACLE_DEV[name]
    print(f"{name}: oracle max dev {odev:.3e} (table {ORACLE_DEV[name]:.3e}), bound {bound:.3e}")
    assert odev <= ORACLE_DEV[name]
    # the tracer: bit-equal to the oracle ...
    if name in R.ORACLE_REFUSES:
        assert np.array_equal(p >= 0, op >= 0)
    else:
        assert np.array_equal(p, op)
    assert np.array_equal(t[op >= 0], ot[op >= 0])
    assert np.isinf(t[op < 0]).all()
    # ... and against float64
    pc = np.where(p >= 0, r["canon"][np.maximum(p, 0)], -1)
    wrong = int((pc[dec] != p64[dec]).sum())
    dev = rel_dev(t, t64, dec & (p64 >= 0) & (pc == p64))
    print(f"{name}: wrong primitives {wrong}, max dev {dev:.3e}")
    assert wrong == 0
    assert dev < bound
    assert np.array_equal(hit_any, p >= 0)


@pytest.mark.parametrize("lm", LDS_MODES)
@pytest.mark.parametrize("name", CASES)
def test_closest_and_any_hit(name, lm):
    r = ref(name)
    t, p = R.core_trace(r["sc"], lm, r["rays"])
    _, pa = R.core_trace(r["sc"], lm, r["rays"], any_hit=True)
    check_against_references(name, t, p, pa >= 0)


def window_sets(name):
    """The re-queries of case (b) from the oracle's hits of case (a): {label: (rays, t0, p0)}."""
    r = ref(name)
    hit = r["op"] >= 0
    rays, t0, p0 = r["rays"][hit], r["ot"][hit], r["op"][hit]
    at, below, above = rays.copy(), rays.copy(), rays.copy()
    at[:, 7] = t0
    below[:, 7] = np.nextafter(t0, np.float32(0))
    above[:, 6] = np.nextafter(t0, np.float32(np.inf))
    return {"tmax=t": (at, t0, p0), "tmax<t": (below, t0, p0), "tmin>t": (above, t0, p0)}


def check_windows(name, trace):
    """Case (b) with trace(rays, any_hit) -> (t, prim)."""
    sc = ref(name)["sc"]
    for label, (rays, t0, p0) in window_sets(name).items():
        t, p = trace(rays, False)
        _, pa = trace(rays, True)
        ot, op = R.oracle_trace(sc, rays)
        assert np.array_equal(p, op), (name, label)
        assert np.array_equal(t[op >= 0], ot[op >= 0]), (name, label)
        assert np.array_equal(pa >= 0, p >= 0), (name, label)
        same = (p == p0) & (t == t0)
        if label == "tmax=t":
            # t <= tmax is inclusive: a triangle hit stays (a sphere's float64 root may lie above its
            # own fp32 rounding, so about half of those drop: the oracle decides)
            tri = sc.prim_type[p0] == 0
            assert same[tri].all(), (name, label)
        else:
            assert not same.any(), (name, label)


@pytest.mark.parametrize("lm", LDS_MODES)
@pytest.mark.parametrize("name", [c for c in CASES if c not in R.ORACLE_REFUSES])
def test_windows_at_the_hit(name, lm):
    sc = ref(name)["sc"]
    check_windows(name, lambda rays, any_hit: R.core_trace(sc, lm, rays, any_hit))


def stack_windows():
    """Rays through all 8 layers with windows that begin and end between two layers (layer j + 1 is
    the first inside), or lie wholly between two layers (nothing inside)."""
    r = ref("stack")
    rays = r["rays"][:1000].copy()
    rng = np.random.default_rng(31)
    o, d = rays[:, :3].astype(np.float64), rays[:, 3:6].astype(np.float64)
    layers = 8
    tk = (0.5 + R.STACK_SPACING * np.arange(layers)[None, :] - o[:, 1:2]) / d[:, 1:2]   # (n, 8), decreasing in k
    tk = tk[:, ::-1]                                                                      # along the ray
    mid = 0.5 * (tk[:, :-1] + tk[:, 1:])                                                  # 7 gaps
    n = len(rays)
    j = rng.integers(0, 6, n)
    k = j + 1 + rng.integers(0, 6 - j)   # j < k <= 6
    empty = np.arange(n) % 4 == 0
    rays[:, 6] = mid[np.arange(n), j]
    rays[:, 7] = np.where(empty, mid[np.arange(n), j] * (1 + 1e-3), mid[np.arange(n), k])
    return rays, empty


def check_stack_windows(trace):
    sc = ref("stack")["sc"]
    rays, empty = stack_windows()
    p64, t64, dec = R.brute_fp64(sc, rays)
    assert (~dec).mean() <= UNDECIDED_MAX
    # what the windows are meant to select, from float64: nothing in an empty one, else one layer
    # (a ray that leaves the quads' sides hits nothing)
    assert (p64[empty] < 0).all() and (p64[~empty] >= 0).mean() > 0.9
    t, p = trace(rays, False)
    _, pa = trace(rays, True)
    ot, op = R.oracle_trace(sc, rays)
    assert np.array_equal(p, op) and np.array_equal(t[op >= 0], ot[op >= 0])
    assert np.array_equal(p[dec], p64[dec])
    assert rel_dev(t, t64, dec & (p64 >= 0)) < 4 * ORACLE_DEV["stack"]
    assert np.array_equal(pa >= 0, p >= 0)


@pytest.mark.parametrize("lm", LDS_MODES)
def test_windows_between_layers(lm):
    sc = ref("stack")["sc"]
    check_stack_windows(lambda rays, any_hit: R.core_trace(sc, lm, rays, any_hit))


def odd_ray_sets():
    return {kind: R.odd_rays(kind) for kind in R.ODD_KINDS}


def check_odd(kind, rays, t, p, hit_any):
    ot, op = R.oracle_trace(R.scene("odd"), rays)
    assert np.array_equal(p, op), kind
    assert np.array_equal(t[op >= 0], ot[op >= 0]), kind
    assert np.isinf(t[op < 0]).all(), kind
    assert np.array_equal(hit_any, p >= 0), kind
    if kind in ("tmin_gt_tmax", "d_zero", "nan_origin", "tmin_inf"):
        assert (op < 0).all(), kind    # nothing to hit: the oracle agrees with the plain reading
    if kind in ("tmin_neg", "d_1e-20"):   # (t is in units of |d|: at |d| = 1e18 every t lies under tmin)
        assert (op >= 0).sum() >= 10, kind


@pytest.mark.parametrize("lm", LDS_MODES)
def test_odd_rays(lm, tmp_path):
    """Negative tmin, tmin > tmax, d = 0, NaN origin, infinite tmin, |d| of 1e-20 and 1e18, 100 rays
    each on grid(6) + 4 spheres, in a child process under a time limit."""
    sets = odd_ray_sets()
    t, p, a = R.child("trace", "odd", lm, tmp_path, np.concatenate(list(sets.values())))
    for k, (kind, rays) in enumerate(sets.items()):
        s = slice(100 * k, 100 * (k + 1))
        check_odd(kind, rays, t[s], p[s], a[s])


LEAF_ROOTS = [("tiny1", "render1"), ("tiny2", "render2"), ("tiny_sphere", "render_sphere")]


@pytest.mark.parametrize("lm", LDS_MODES)
@pytest.mark.parametrize("name,rname", LEAF_ROOTS)
def test_leaf_roots_terminate(name, rname, lm, tmp_path):
    """A device tree whose root is a leaf: rays and a 16x12 s1 m5 render return, bit-equal to oracle
    mode 2. Before emit_device_tree gave the 4-wide tree a root node, LDS modes 0 and 2 never
    returned (this test then fails by its child's time limit); mode 1 did."""
    r = ref(name)
    assert R.binary_nodes(r["sc"]) == 1 and R.binary_nodes(R.scene(rname)) == 1   # the root is a leaf
    t, p, a = R.child("trace", name, lm, tmp_path, r["rays"])
    check_against_references(name, t, p, a)
    eye, light = R.child("render", rname, lm, tmp_path)
    W, H = R.FRAME
    _, oeye, olight, _ = oracle_render(R.scene(rname), W, H, 1, 5, MODE_C32, seed=3, threads=1)
    assert oeye.mean() + olight.mean() > 0
    assert np.array_equal(eye, oeye) and np.array_equal(light, olight)


# ------------------------------------------------------------------------------------------------
# (e) the traversal stack at its bound, under ASan + UBSan

CSRC = os.path.join(REPO, "bidirectional-pathtracing_amd", "csrc")
NATIVE = os.path.join(REPO, "tests", "native")
SAN_FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-omit-frame-pointer",
             "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-I" + os.path.join(REPO, "include"), "-I" + CSRC]


def build_probes(tmp, stack_maxes):
    """stack_probe with the flags of tests/test_sanitizers.py's driver, once per traversal stack
    limit (None = the default); the units are compiled side by side. core_cpu.cpp gives its ray
    queries alone (CORE_CPU_TRACE_ONLY): its renders are not run here and take minutes to compile."""
    from concurrent.futures import ThreadPoolExecutor
    jobs, exes = [], []
    loader = str(tmp / "dae_loader.o")   # does not see BDPT_STACK_MAX: shared
    jobs.append(["g++"] + SAN_FLAGS + ["-c", os.path.join(CSRC, "dae_loader.cpp"), "-o", loader])
    for sm in stack_maxes:
        defs = ["-DCORE_CPU_TRACE_ONLY"] + ([f"-DBDPT_STACK_MAX={sm}"] if sm is not None else [])
        objs = []
        for src in (os.path.join(NATIVE, "stack_probe.cpp"), os.path.join(NATIVE, "core_cpu.cpp"),
                    os.path.join(CSRC, "bdpt_scene.cpp")):
            objs.append(str(tmp / f"{os.path.basename(src)}.{sm}.o"))
            jobs.append(["g++"] + SAN_FLAGS + defs + ["-c", src, "-o", objs[-1]])
        exes.append((str(tmp / f"stack_probe_{sm}"), objs + [loader]))
    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(lambda c: subprocess.run(c, check=True, capture_output=True, text=True, timeout=600), jobs))
    for exe, objs in exes:
        subprocess.run(["g++", "-fsanitize=address,undefined", "-static-libasan", "-o", exe] + objs + ["-lz"],
                       check=True, capture_output=True, text=True, timeout=600)
    return [exe for exe, _ in exes]


def run_probe(exe, **env):
    e = {k: v for k, v in os.environ.items() if k not in ("BDPT_BVH", "BDPT_SBVH", "BDPT_SBVH_BUDGET")}
    e.update(env, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, os.path.join(REPO, "scenes", "CBbunny.dae")], capture_output=True, text=True,
                       timeout=600, env=e)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "no sanitizer report" in r.stdout
    return r.stdout


@pytest.mark.slow
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_stack_bound_under_asan_ubsan(tmp_path, tmp_path_factory, monkeypatch):
    """Rays that enter every child of every node of CBbunny's trees (the probe verifies that from
    the counters) fill the traversal stack as far as any ray can: (W - 1) entries per level. With
    the default limit on the default tree, the tree with spatial splits and the reference's
    midpoint tree; then with BDPT_STACK_MAX at exactly what the default tree needs, where one
    entry more than the (W-1)*(depth+1)+2 bound admits would write past the stack array."""
    from test_bvh_reinsert import checker, dae, set_env, tree_of
    set_env(monkeypatch)
    rc, t = tree_of(checker(tmp_path_factory), dae("CBbunny"))
    assert rc == 0
    need = t["stack_need"]
    exe, tight = build_probes(tmp_path, [None, need])
    run_probe(exe)
    run_probe(exe, BDPT_SBVH="1e-5")
    run_probe(exe, BDPT_BVH="ref")
    out = run_probe(tight)
    assert f"stack limit {need}" in out and f"stack need {need}" in out
