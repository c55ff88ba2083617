"""The torch side of tests/test_gpu_denoise.py, run once as a child process:
`python _denoise_gpu.py out.npz`. torch brings a HIP runtime of its own, which has to initialise
before the library's does (bench.py's order); a pytest process has long loaded the library by then.
Runs bdpt_denoise_buffers on torch-allocated device memory (bdpt_amd.denoise_tensor) over the CPU
tests' synthetic inputs, and the context path against the buffer path, and saves every result."""
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
import _denoise as D   # noqa: E402
from _util import golden_scene   # noqa: E402


def gpu_filter(color, feat, in_place=False, **params):
    c = torch.from_numpy(np.ascontiguousarray(color, np.float32)).cuda()
    f = torch.from_numpy(np.ascontiguousarray(feat, np.float32)).cuda()
    out = B.denoise_tensor(c, f, out=c if in_place else None, **params)
    torch.cuda.synchronize()
    if not in_place:   # the input is left alone
        assert torch.equal(c.cpu(), torch.from_numpy(np.ascontiguousarray(color, np.float32)))
    return out.cpu().numpy()


def main(out_path):
    torch.cuda.init()
    res = {}
    for (W, H) in D.FRAMES:
        color, feat = D.synthetic(W, H)
        for levels in (0, 1, 3, 5):
            for demod in (False, True):
                k = f"{W}x{H}_L{levels}_d{int(demod)}"
                res[k] = gpu_filter(color, feat, levels=levels, demodulate=demod, **D.SIG)
                res[k + "_inplace"] = gpu_filter(color, feat, in_place=True, levels=levels, demodulate=demod, **D.SIG)
        const = np.full((H, W, 3), 0.7, np.float32)
        for levels in (1, 5):
            res[f"{W}x{H}_const_L{levels}"] = gpu_filter(const, feat, levels=levels, demodulate=False, **D.SIG)
        lc, lf, _ = D.leak_inputs(W, H)
        res[f"{W}x{H}_leak"] = gpu_filter(lc, lf, **D.LEAK)
    # the context path against the buffer path, on a stream of torch's
    W, H = 37, 21
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        r = B.BidirectionalPathTracer(golden_scene("CBspheres"), W, H, 4, 5, seed=3)
        r.set_stream(st.cuda_stream)
        r.raytrace_tiles()
        r.render_features()
        res["ctx_denoised"] = r.denoise()
        res["ctx_features"] = r.read_features_raw()
        res["ctx_sample"] = r.read_frame(B.FRAME_SAMPLE)
        dst = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        B.denoise_buffers(r.frame_device_ptr(B.FRAME_SAMPLE), r.features_device_ptr(), W, H, dst.data_ptr(),
                          stream=st.cuda_stream)
        st.synchronize()
        res["ctx_buffers"] = dst.cpu().numpy()
        res["ctx_ptr_ok"] = np.array([r.denoised_device_ptr() != 0])
        r.close()
    np.savez(out_path, **res)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
