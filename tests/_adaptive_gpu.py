"""The torch side of tests/test_gpu_adaptive.py, run once as a child process:
`python _adaptive_gpu.py out.npz`. torch brings a HIP runtime of its own, which has to initialise
before the library's does (bench.py's order); a pytest process has long loaded the library by then.
Runs bdpt_adaptive_moments_buffers, bdpt_adaptive_decide_buffers, bdpt_adaptive_compact_buffers and
bdpt_adaptive_resolve_buffers on torch-allocated device memory over the CPU tests' synthetic inputs
and saves every result."""
import os
import sys

import numpy as np
import torch   # before bdpt_amd loads libbdpt_amd.so

TESTS = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(TESTS)
for _p in (REPO, os.path.join(REPO, "bidirectional-pathtracing_amd"), TESTS):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import bdpt_amd as B   # noqa: E402
import _adaptive as A   # noqa: E402

S, M, R = 24, 2, 7          # test_adaptive.py's synthetic renders
TOL = 0.2
GRIDS = [(1, 1), (20, 20), (263, 250)]
PATTERNS = ["all", "none", "one", "alternating", "random"]


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def decide_inputs(W, H, seed=1):
    """test_adaptive.py::test_decision_matches_float64's case at this size."""
    nb = A.block_pixels(W, H).size
    noise = 0.05 * 30.0 ** (np.arange(nb) % 7 / 6.0)
    run = A.synthetic_run(W, H, S, M, R, seed=seed, noise=noise)
    active = (np.arange(nb) % 3 != 2).astype(np.int32)
    return run, active


def compaction_flags(W, H, pattern):
    from test_adaptive import compaction_flags as f
    return f(W, H, pattern)


def main(out_path):
    torch.cuda.init()
    st = torch.cuda.current_stream().cuda_stream
    res = {}
    for (W, H) in A.FRAMES + [(64, 40)]:
        key = f"{W}x{H}"
        run, active = decide_inputs(W, H)
        nb = active.size
        rec_e = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        rec_l = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        for e, l, Mr in zip(run["eye"], run["light"], run["M"]):
            te, tl = dev(e), dev(l)
            B.adaptive_moments_buffers(te.data_ptr(), tl.data_ptr(), rec_e.data_ptr(), rec_l.data_ptr(), W, H, Mr, stream=st)
            torch.cuda.synchronize()   # te / tl go out of scope
        res[key + "_rec_e"], res[key + "_rec_l"] = rec_e.cpu().numpy(), rec_l.cpu().numpy()
        # the decision on the host build's records, so that a last-bit difference of the records
        # (there is none: asserted by the test) cannot hide in it
        he, hl = A.host_records(run)
        de, dl = dev(he), dev(hl)
        rounds, flags = dev(run["K"] - active, np.int32), dev(active, np.int32)
        B.adaptive_decide_buffers(de.data_ptr(), dl.data_ptr(), rounds.data_ptr(), flags.data_ptr(), W, H, S, M, R, run["N"], TOL,
                                  decide=True, stream=st)
        torch.cuda.synchronize()
        res[key + "_rounds"], res[key + "_active"] = rounds.cpu().numpy(), flags.cpu().numpy()
        r2, f2 = dev(run["K"] - active, np.int32), dev(active, np.int32)
        B.adaptive_decide_buffers(de.data_ptr(), dl.data_ptr(), r2.data_ptr(), f2.data_ptr(), W, H, S, M, 1, 1, TOL, decide=False, stream=st)
        torch.cuda.synchronize()
        res[key + "_rounds_nodecide"], res[key + "_active_nodecide"] = r2.cpu().numpy(), f2.cpu().numpy()
        # a frame of zeros stops
        z = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        r3, f3 = dev(np.full(nb, 3), np.int32), dev(np.ones(nb), np.int32)
        B.adaptive_decide_buffers(z.data_ptr(), z.data_ptr(), r3.data_ptr(), f3.data_ptr(), W, H, 8, 2, 4, 4 * W * H * 2, 0.3, stream=st)
        torch.cuda.synchronize()
        res[key + "_zero_rounds"], res[key + "_zero_active"] = r3.cpu().numpy(), f3.cpu().numpy()
        # the resolve
        col = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        var = torch.empty((H, W), dtype=torch.float32, device="cuda")
        cnt = torch.empty((H, W), dtype=torch.int32, device="cuda")
        kb = dev(run["K"], np.int32)
        B.adaptive_resolve_buffers(de.data_ptr(), dl.data_ptr(), kb.data_ptr(), W, H, S, M, R, run["N"], col.data_ptr(), var.data_ptr(),
                                   cnt.data_ptr(), stream=st)
        torch.cuda.synchronize()
        res[key + "_color"], res[key + "_var"], res[key + "_counts"] = col.cpu().numpy(), var.cpu().numpy(), cnt.cpu().numpy()
    for (W, H) in GRIDS:
        nb = A.block_pixels(W, H).size
        for pattern in PATTERNS:
            flags = dev(compaction_flags(W, H, pattern), np.int32)
            lst = torch.full((nb, 4), -1, dtype=torch.int32, device="cuda")
            cnt = torch.full((2,), -1, dtype=torch.int32, device="cuda")
            B.adaptive_compact_buffers(flags.data_ptr(), W, H, lst.data_ptr(), cnt.data_ptr(), stream=st)
            torch.cuda.synchronize()
            res[f"{W}x{H}_{pattern}_list"], res[f"{W}x{H}_{pattern}_cnt"] = lst.cpu().numpy(), cnt.cpu().numpy()
    np.savez(out_path, **res)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
