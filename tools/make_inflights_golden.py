#!/usr/bin/env python3
"""Generates tests/golden/inflights/ (run where the reference tree and oracle/_ref/ exist; the GPU
box only reads the committed outputs).

  * CBspheres_hemi.dae: scenes/CBspheres_lambertian.dae (the reference's scene) with its area light
    and emissive quad replaced by one ambient light (InfiniteHemisphereLight: uniform about world
    +y, up; its light enters through the box's open side);
  * CBspheres_dir.dae: the same with one directional light whose direction enters the open side;
  * CBspheres_mixed.dae: the scene with its area light kept and the directional light added;
  * hemi_pt.npz / dir_pt.npz: the reference's unidirectional PathTracer (oracle/_ref/ref_driver -U)
    on the first two: the converged images that BDPT with bdpt_params.infinite_lights is checked
    against (tests/test_inflights.py; the reference's BDPT cannot render these lights). Frame size,
    depth and sample budget as tests/golden/env/envonly_pt.npz.

usage: python tools/make_inflights_golden.py
"""
import os
import re
import subprocess
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "inflights")
DRV = os.path.join(REPO, "oracle", "_ref", "ref_driver")
SRC = os.path.join(REPO, "scenes", "CBspheres_lambertian.dae")
PT = dict(W=64, H=48, spp=512, depth=12, threads=8)

AMBIENT = """    <light id="Hemi-light" name="Hemi">
      <technique_common>
        <ambient>
          <color>1 1 1</color>
        </ambient>
      </technique_common>
    </light>
"""
DIRECTIONAL = """    <light id="Sun-light" name="Sun">
      <technique_common>
        <directional>
          <color sid="color">3 3 3</color>
        </directional>
      </technique_common>
    </light>
"""
# The loader transforms the COLLADA direction (0, 0, -1) as a point (w = 1), so the node's
# translation steers it: normalize((0, 0, -1) + (0.3, 1, 1.4)) = normalize(0.3, 1, 0.4) in the file's
# Z-up axes, which the scene's up-axis conversion turns into dirToLight = (-0.268, 0.358, 0.894) in
# world space: from the camera's side (the box's open side faces +z there), above and to the side.
SUN_NODE = """      <node id="Sun" name="Sun" type="NODE">
        <matrix sid="transform">1 0 0 0.3 0 1 0 1 0 0 1 1.4 0 0 0 1</matrix>
        <instance_light url="#Sun-light"/>
      </node>
"""
HEMI_NODE = """      <node id="Hemi" name="Hemi" type="NODE">
        <matrix sid="transform">1 0 0 0 0 1 0 0 0 0 1 0 0 0 0 1</matrix>
        <instance_light url="#Hemi-light"/>
      </node>
"""


def without_area_light(s):
    s, n = re.subn(r'    <light id="Area-light" name="Light">.*?</light>\n', "", s, flags=re.S)
    assert n == 1
    for node in ("Area", "light"):
        s, n = re.subn(r'\s*<node id="%s" name="%s" type="NODE">.*?</node>' % (node, node), "", s, flags=re.S)
        assert n == 1, node
    return s


def with_light(s, light, node):
    s, n = re.subn(r"(  <library_lights>\n)", lambda m: m.group(1) + light, s)
    assert n == 1
    s, n = re.subn(r'(    <visual_scene id="Scene" name="Scene">\n)', lambda m: m.group(1) + node, s)
    assert n == 1
    return s


def main():
    os.makedirs(OUT, exist_ok=True)
    src = open(SRC).read()
    scenes = {"CBspheres_hemi.dae": with_light(without_area_light(src), AMBIENT, HEMI_NODE),
              "CBspheres_dir.dae": with_light(without_area_light(src), DIRECTIONAL, SUN_NODE),
              "CBspheres_mixed.dae": with_light(src, DIRECTIONAL, SUN_NODE)}
    for name, text in scenes.items():
        open(os.path.join(OUT, name), "w").write(text)
        print("wrote", name, flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        for key in ("hemi", "dir"):
            dae = os.path.join(OUT, "CBspheres_%s.dae" % key)
            pre = os.path.join(tmp, key)
            cmd = [DRV, "-U", "-a", "64", "0", "-s", str(PT["spp"]), "-m", str(PT["depth"]),
                   "-t", str(PT["threads"]), "-r", str(PT["W"]), str(PT["H"]), "-o", pre, dae]
            subprocess.run(cmd, cwd=tmp, check=True, stdout=subprocess.DEVNULL)
            img = np.load(pre + "_sample.npy", allow_pickle=False)
            np.savez_compressed(os.path.join(OUT, key + "_pt.npz"), image=img,
                                cmd=np.array(" ".join(os.path.basename(c) if os.path.isabs(c) else c for c in cmd)),
                                **{k: np.array(v) for k, v in PT.items()})
            print("wrote %s_pt.npz mean" % key, img.mean(axis=(0, 1)), flush=True)


if __name__ == "__main__":
    main()
