"""The torch side of tests/test_gpu_variance.py, run once as a child process:
`python _variance_gpu.py out.npz`. torch brings a HIP runtime of its own, which has to initialise
before the library's does (bench.py's order); a pytest process has long loaded the library by then.
Runs bdpt_moments_buffers, bdpt_variance_buffers and bdpt_denoise_variance_buffers on
torch-allocated device memory over the CPU tests' synthetic inputs, and the context path against
the buffer path, and saves every result."""
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
import _pixelbound as PB   # noqa: E402
import _variance as V   # noqa: E402

BIG = 1e18
CTX = V.CTX


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def gpu_moments(a, b, K):
    """(record, variance) through the buffer entry points on torch's current stream."""
    H, W = a[0].shape[:2]
    st = torch.cuda.current_stream().cuda_stream
    rec = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    for k in range(K):
        ta = dev(a[k])
        tb = dev(b[k]) if b is not None else None
        B.moments_buffers(ta.data_ptr(), tb.data_ptr() if tb is not None else 0, rec.data_ptr(), W, H, stream=st)
        torch.cuda.synchronize()   # ta / tb go out of scope
    var = torch.empty((H, W), dtype=torch.float32, device="cuda")
    B.variance_buffers(rec.data_ptr(), K, W, H, var.data_ptr(), stream=st)
    torch.cuda.synchronize()
    return rec.cpu().numpy(), var.cpu().numpy()


def gpu_filter(color, var, feat, in_place=False, **params):
    c, v, f = dev(color), dev(var), dev(feat)
    out, vout = B.denoise_variance_tensor(c, v, f, out=c if in_place else None, var_out=v if in_place else None, **params)
    torch.cuda.synchronize()
    if not in_place:   # the inputs are left alone
        assert torch.equal(c.cpu(), torch.from_numpy(np.ascontiguousarray(color, np.float32)))
        assert torch.equal(v.cpu(), torch.from_numpy(np.ascontiguousarray(var, np.float32)))
    return out.cpu().numpy(), vout.cpu().numpy()


def main(out_path):
    torch.cuda.init()
    res = {}

    def put(key, cv):
        res[key + "_c"], res[key + "_v"] = cv

    for (W, H) in V.FRAMES:
        for K in V.BATCHES:
            a, b = V.batch_frames(W, H, K)
            res[f"{W}x{H}_K{K}_rec2"], res[f"{W}x{H}_K{K}_var2"] = gpu_moments(a, b, K)
            res[f"{W}x{H}_K{K}_rec1"], res[f"{W}x{H}_K{K}_var1"] = gpu_moments(a, None, K)
        color, var, feat = V.synthetic(W, H)
        for levels in (0, 1, 3, 5):
            put(f"{W}x{H}_L{levels}", gpu_filter(color, var, feat, levels=levels, **V.SIG))
            put(f"{W}x{H}_L{levels}_inplace", gpu_filter(color, var, feat, in_place=True, levels=levels, **V.SIG))
        for levels in (1, 3, 5):
            put(f"{W}x{H}_big_L{levels}", gpu_filter(color, var + np.float32(0.1), feat, levels=levels, sigma_variance=BIG,
                                                      sigma_normal=BIG, sigma_depth=BIG))
            put(f"{W}x{H}_zero_L{levels}", gpu_filter(V.distinct_colors(W, H), np.zeros((H, W), np.float32), feat,
                                                       levels=levels, **V.SIG))
        const = np.full((H, W, 3), 0.7, np.float32)
        for levels in (1, 5):
            put(f"{W}x{H}_const_L{levels}", gpu_filter(const, var, feat, levels=levels, **V.SIG))
        lc, lv, lf, _ = V.leak_inputs(W, H)
        put(f"{W}x{H}_leak", gpu_filter(lc, lv, lf, **V.LEAK))
    # the context path, and the buffer path on the context's own pointers, on a stream of torch's
    W, H, S, M, K = (CTX[k] for k in ("W", "H", "S", "M", "K"))
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        r = B.BidirectionalPathTracer(PB.full_view("CBspheres", W, H), W, H, S, M, seed=CTX["seed"])
        r.set_stream(st.cuda_stream)
        r.render_batches(0, S, K)
        for name, which in (("sample", B.FRAME_SAMPLE), ("eye", B.FRAME_EYE), ("light", B.FRAME_LIGHT)):
            res["ctx_" + name] = r.read_frame(which)
        res["ctx_moments"] = r.read_moments()
        r.variance()
        res["ctx_variance"] = r.read_variance()
        r.render_features()
        res["ctx_features"] = r.read_features_raw()
        res["ctx_denoised"] = r.denoise_variance()
        dst = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        B.denoise_variance_buffers(r.frame_device_ptr(B.FRAME_SAMPLE), r.variance_device_ptr(), r.features_device_ptr(), W, H,
                                   dst.data_ptr(), stream=st.cuda_stream)
        st.synchronize()
        res["ctx_buffers"] = dst.cpu().numpy()
        r.close()
    np.savez(out_path, **res)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
