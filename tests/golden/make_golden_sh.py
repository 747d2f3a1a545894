#!/usr/bin/env python3
"""
Regenerates tests/golden/sh_golden.npz.  BUILD CONTAINER ONLY: imports the reference's pure-numpy
deep3dmap/core/renderer/renderer_demo/mesh/texture.py by file path (under the reference checkout given) and stores only
the outputs of its fit_illumination on the scenes of tests/smooth_shading_scenes.py (inputs are regenerated from the seeds,
not stored).  The reference clamps vertices[:2] in place: every call gets copies.

Usage:  python tests/golden/make_golden_sh.py <reference checkout>
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import smooth_shading_scenes as S  # noqa: E402


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref_root = sys.argv[1]
    path = os.path.join(ref_root, "deep3dmap/core/renderer/renderer_demo/mesh/texture.py")
    spec = importlib.util.spec_from_file_location("reference_mesh_texture", path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {}
    for name in S.FIT_SCENES:
        s = S.fit_scene(name)
        out[name] = ref.fit_illumination(s["image"].copy(), s["vertices"].copy(), s["texture"].copy(), s["triangles"].copy(),
                                         s["vis_ind"].copy())
        out[name + "/iter1_lamb2"] = ref.fit_illumination(s["image"].copy(), s["vertices"].copy(), s["texture"].copy(),
                                                          s["triangles"].copy(), s["vis_ind"].copy(), lamb=2, max_iter=1)
    dst = os.path.join(HERE, "sh_golden.npz")
    np.savez_compressed(dst, **out)
    print(f"wrote {dst}: {len(out)} arrays, {os.path.getsize(dst) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
