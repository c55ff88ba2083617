#!/usr/bin/env python3
"""CPU screen (no GPU) of the connection-ray flush policies of k_bdpt_sample (bdpt_megakernel.h).

The CPU build of the device code (-DBDPT_STEP_HIST, tools/flush_log.cpp) renders chosen 8x8 pixel
blocks of a full frame and logs, per pixel-sample, the lists connect_sample walks and, per any-hit
query, its node steps and primitive tests (one lane: the same tree and visiting order as the GPU,
no speculation). This tool rebuilds each work item's push order from that log — 64 lanes stepping
through their lists together, one ballot-compacted push per step — and replays the flush policies
on it:

  current        flush 64 rays as soon as 64 are queued, one ray per lane, the wave waits for the
                 slowest; the item's end flushes what is left
  refill         the same trigger, but a flush drains every queued ray: once `idle` lanes have
                 ended their ray they take the next queued ones (a refill round, priced one step)
  refill+late    drain only when queued + B > 128, B = lanes whose list is not yet empty after the
                 step (64 after a list's last step)

A ray's work is its node steps (first figure) or its node steps + primitive tests (second figure,
equal weight); a lane works through its rays serially, a wave step advances every busy lane by one.
The model ignores how speculative descent couples the lanes, the phase boundaries a refill has to
wait for, and the cost of the extra ballots: it bounds what refill can gain, it does not predict it.

  python3 tools/flush_sim.py [scene ...] [blocks=150] [idle=8,16,32] [seed=1]
scenes: standin, CBbunny, CBgems (default: all three), 1920x1080, 2 samples per item
"""
import os
import sys

QCAP = 128


# ------------------------------------------------------------------------------------------------
# the arithmetic (tests/test_flush_sim.py)

def parse_log(ints):
    """The log's int triples -> one record per pixel-sample, in log order:
    {"cE", "cL", "sE", "nL", "rays": {(i, j): (node steps, primitive tests)}}."""
    out = []
    for k in range(0, len(ints), 3):
        a, b, c = int(ints[k]), int(ints[k + 1]), int(ints[k + 2])
        if a == -1:
            out.append({"cE": b & 0xffffffff, "cL": c & 0xffffffff, "sE": 0, "nL": 0, "rays": {}})
        elif a == -2:
            out[-1]["sE"], out[-1]["nL"] = b & 0xffffffff, c
        else:
            out[-1]["rays"][(a >> 8, a & 255)] = (b, c)
    return out


def _bits(m):
    return [k for k in range(32) if m >> k & 1]


def lane_steps(rec):
    """A lane's connection steps in connect_sample's order, as four lists (one per loop: s = 0, the
    fresh light sample j = 1, light tracing i = 1, the general pairs) of (i, j)."""
    if rec is None:
        return [[], [], [], []]
    cE, cL = _bits(rec["cE"]), _bits(rec["cL"])
    return [[(k, 0) for k in _bits(rec["sE"])],
            [(k, 1) for k in _bits(rec["cE"] | 2)] if rec["nL"] > 1 else [],
            [(1, k) for k in cL],
            [(i, j) for i in cE for j in cL]]


def item_pushes(samples):
    """samples: per sample of the item, the 64 lanes' records (None: a lane without a pixel).
    Returns the item's steps in order, each (rays pushed in lane order as (node steps, primitive
    tests), B = the wave-uniform bound of the next step's pushes)."""
    steps = []
    for lanes in samples:
        lists = [lane_steps(r) for r in lanes]
        for phase in range(4):
            n = max(len(l[phase]) for l in lists)
            for s in range(n):
                pushed = [r["rays"][l[phase][s]] for r, l in zip(lanes, lists)
                          if r is not None and s < len(l[phase]) and l[phase][s] in r["rays"]]
                left = sum(1 for l in lists if len(l[phase]) > s + 1)
                steps.append((pushed, left if left else 64))
    return steps


def drain(works, idle=None):
    """Wave steps to resolve the rays whose per-ray work is `works`, in order. idle = None: one ray
    per lane (at most 64), the wave waits for the slowest. Otherwise lanes 0-63 take the first rays,
    and whenever at least `idle` lanes are out of work while rays are left, they take the next
    ones: one step per refill round."""
    if idle is None:
        assert len(works) <= 64
        return max(works) if works else 0
    busy, rest, t = list(works[:64]), list(works[64:]), 0
    while True:
        busy = [w for w in busy if w > 0]
        if rest and 64 - len(busy) >= idle:
            take = min(64 - len(busy), len(rest))
            busy += rest[:take]
            rest = rest[take:]
            t += 1
            continue
        if not busy:
            return t
        t += 1
        busy = [w - 1 for w in busy]


def replay(steps, policy, idle=16):
    """One work item under a policy ("current", "refill", "late"): {"flushes", "rays", "node": wave
    steps with a ray's work = its node steps, "both": = node steps + primitive tests}."""
    out = {"flushes": 0, "rays": 0, "node": 0, "both": 0}
    queue = []

    def flush(n):
        batch = queue[:n]
        del queue[:n]
        out["flushes"] += 1
        out["rays"] += len(batch)
        th = None if policy == "current" else idle
        out["node"] += drain([b[0] for b in batch], th)
        out["both"] += drain([b[0] + b[1] for b in batch], th)

    for pushed, nxt in steps:
        queue.extend(pushed)
        assert len(queue) <= QCAP, "the ring would overflow"
        if policy == "late":
            if len(queue) + nxt > QCAP:
                flush(len(queue))
        elif len(queue) >= 64:
            flush(64 if policy == "current" else len(queue))
    if queue:
        flush(len(queue))
    return out


def summarise(items, policy, idle=16):
    """Per-item means over the items' replays: (flushes, mean batch, node wave-steps, node + primitive
    wave-iterations)."""
    tot = {"flushes": 0, "rays": 0, "node": 0, "both": 0}
    for steps in items:
        for k, v in replay(steps, policy, idle).items():
            tot[k] += v
    n = max(1, len(items))
    return tot["flushes"] / n, tot["rays"] / max(1, tot["flushes"]), tot["node"] / n, tot["both"] / n


# ------------------------------------------------------------------------------------------------
def main(argv):
    import ctypes as C
    import subprocess

    import numpy as np

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(repo, "bidirectional-pathtracing_amd"), os.path.join(repo, "tests")]
    import bdpt_amd as B
    from _util import golden_scene

    opts = {"blocks": "150", "idle": "8,16,32", "seed": "1"}
    only = []
    for a in argv:
        if "=" in a:
            k, v = a.split("=", 1)
            opts[k] = v
        else:
            only.append(a)
    nblk, idles, seed = int(opts["blocks"]), [int(x) for x in opts["idle"].split(",")], int(opts["seed"])
    cs = os.path.join(repo, "bidirectional-pathtracing_amd", "csrc")
    so = "/tmp/libcore_flushlog.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-DBDPT_STEP_HIST",
                    "-I" + os.path.join(repo, "include"), "-I" + cs, "-o", so,
                    os.path.join(repo, "tools", "flush_log.cpp"), os.path.join(cs, "bdpt_scene.cpp")], check=True)
    lib = C.CDLL(so)
    lib.core_cpu_anyhit_log_get.restype = C.c_longlong
    W, H, spp = 1920, 1080, 2
    for name, M, lm in [("standin", 5, 2), ("CBbunny", 5, 2), ("CBgems", 7, 1)]:
        if only and name not in only:
            continue
        if name == "CBgems":
            sc = golden_scene(name, W, H)
        else:
            sc = B.load_dae(os.path.join(repo, "scenes", "CBlucy_standin.dae" if name == "standin" else name + ".dae"), W, H)
        rng = np.random.RandomState(seed)
        blocks = rng.choice((W // 8) * (H // 8), nblk, replace=False)
        px = np.array([((b % (W // 8)) * 8 + (l & 7), (b // (W // 8)) * 8 + (l >> 3)) for b in blocks for l in range(64)],
                      dtype=np.int32)
        eye, light, st = np.zeros((H, W, 3)), np.zeros((H, W, 3)), np.zeros(8)
        pd, d = C.POINTER(C.c_double), sc.desc()
        lib.core_cpu_anyhit_log(1)
        rc = lib.core_cpu_render(C.byref(d), W, H, spp, M, C.c_uint64(5489), 0, spp, px.ctypes.data_as(C.POINTER(C.c_int)),
                                 len(px), eye.ctypes.data_as(pd), light.ctypes.data_as(pd), st.ctypes.data_as(pd), lm, 0)
        assert rc == 0
        n = lib.core_cpu_anyhit_log_get(None, C.c_longlong(0))
        log = np.zeros(n, np.int32)
        lib.core_cpu_anyhit_log_get(log.ctypes.data_as(C.POINTER(C.c_int)), C.c_longlong(n))
        lib.core_cpu_anyhit_log(0)
        recs = parse_log(log)
        assert len(recs) == nblk * 64 * spp and sum(len(r["rays"]) for r in recs) == int(st[2])
        # record (block, lane, sample) is recs[(block * 64 + lane) * spp + sample]; one item per block
        items = [item_pushes([[recs[(b * 64 + l) * spp + s] for l in range(64)] for s in range(spp)]) for b in range(nblk)]
        rays = [w for it in items for pushed, _ in it for w in pushed]
        assert len(rays) == int(st[2])   # every logged ray is pushed exactly once
        print(f"{name} {W}x{H} m{M} LM {lm}: {nblk} items of {spp} samples, {len(rays) / nblk:.1f} rays per item, "
              f"node steps per ray mean {np.mean([r[0] for r in rays]):.2f} max {max(r[0] for r in rays)}, "
              f"primitive tests per ray mean {np.mean([r[1] for r in rays]):.2f}", flush=True)
        base = summarise(items, "current")
        print(f"  {'policy':<28} flushes/item  mean batch  node wave-steps/item  node+prim wave-iterations/item")
        print(f"  {'current':<28} {base[0]:12.2f} {base[1]:11.1f} {base[2]:21.1f} {base[3]:31.1f}")
        for pol in ("refill", "late"):
            for idle in idles:
                r = summarise(items, pol, idle)
                label = f"{'refill' if pol == 'refill' else 'refill+late trigger'} idle {idle}"
                print(f"  {label:<28} {r[0]:12.2f} {r[1]:11.1f} {r[2]:12.1f} ({r[2] / base[2] - 1:+6.1%}) "
                      f"{r[3]:22.1f} ({r[3] / base[3] - 1:+6.1%})", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
