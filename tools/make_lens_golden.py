#!/usr/bin/env python3
"""Generates tests/golden/lens/ (run where the reference tree and oracle/_ref/ exist; the GPU box
only reads the committed outputs).

  * hemi_lens_pt.npz / dir_lens_pt.npz: the reference's unidirectional PathTracer with its thin
    lens (oracle/_ref/ref_driver -U -b 0.5 -d 2.5, Camera::generate_ray_for_thin_lens) on
    tests/golden/inflights/CBspheres_hemi.dae and CBspheres_dir.dae: the converged images that BDPT
    with the thin lens (bdpt_params.lens_radius > 0) is checked against
    (tests/test_lens.py; the reference's BDPT is pinhole only). Frame size and depth as
    tests/golden/inflights/*_pt.npz; 1024 spp. Lens radius and focal distance are chosen so that
    the lens shows in the image mean and in the 4x4 block means at this frame size.

usage: python tools/make_lens_golden.py
"""
import os
import subprocess
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "lens")
SCENES = os.path.join(REPO, "tests", "golden", "inflights")
DRV = os.path.join(REPO, "oracle", "_ref", "ref_driver")
PT = dict(W=64, H=48, spp=1024, depth=12, threads=8, lens=0.5, focal=2.5)


def main():
    os.makedirs(OUT, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        for key in ("hemi", "dir"):
            dae = os.path.join(SCENES, "CBspheres_%s.dae" % key)
            pre = os.path.join(tmp, key)
            cmd = [DRV, "-U", "-a", "64", "0", "-s", str(PT["spp"]), "-m", str(PT["depth"]),
                   "-t", str(PT["threads"]), "-r", str(PT["W"]), str(PT["H"]),
                   "-b", str(PT["lens"]), "-d", str(PT["focal"]), "-o", pre, dae]
            subprocess.run(cmd, cwd=tmp, check=True, stdout=subprocess.DEVNULL)
            img = np.load(pre + "_sample.npy", allow_pickle=False)
            np.savez_compressed(os.path.join(OUT, key + "_lens_pt.npz"), image=img,
                                cmd=np.array(" ".join(os.path.basename(c) if os.path.isabs(c) else c for c in cmd)),
                                **{k: np.array(v) for k, v in PT.items()})
            print("wrote %s_lens_pt.npz mean" % key, img.mean(axis=(0, 1)), flush=True)


if __name__ == "__main__":
    main()
