#!/usr/bin/env python3
"""
Regenerates tests/golden/light_golden.npz.  BUILD CONTAINER ONLY: needs /root/reference.

The reference's lighting (NR/lighting.py:5-57), imported by file path and run on the CPU under autograd: lit textures
and the gradients of every light parameter, of the faces and of the textures for one upstream gradient, in three cases --
a shared light, per-batch colours and direction ([bs,3]), and 0-d intensity tensors.  Only inputs and numeric outputs are
stored (tests/test_gpu_light_params.py).

Usage:  python tests/golden/make_golden_light.py
"""
import importlib.util
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
NR = "/root/reference/pnpmodules/neural_renderer/neural_renderer"
NAMES = ("intensity_ambient", "intensity_directional", "color_ambient", "color_directional", "direction")


def main():
    spec = importlib.util.spec_from_file_location("ref_lighting", os.path.join(NR, "lighting.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.manual_seed(11)
    bs, nf, ts = 3, 40, 2
    faces = torch.randn(bs, nf, 3, 3)
    textures = torch.rand(bs, nf, ts, ts, ts, 3)
    upstream = torch.randn(bs, nf, ts, ts, ts, 3)
    cases = {
        "shared": (torch.tensor(0.4), torch.tensor(0.7), torch.tensor([0.9, 0.8, 1.0]), torch.tensor([1.0, 0.7, 0.6]),
                   torch.tensor([0.3, 0.8, -0.5])),
        "per_batch": (torch.tensor(0.5), torch.tensor(0.6), torch.rand(bs, 3) * 0.5 + 0.5, torch.rand(bs, 3) * 0.5 + 0.5,
                      torch.randn(bs, 3)),
        "zero_dim": (torch.tensor(0.3), torch.tensor(0.9), torch.tensor([1.0, 1.0, 1.0]), torch.tensor([0.8, 0.9, 1.0]),
                     torch.tensor([0.0, 0.6, 0.8])),
    }
    out = {"faces": faces.numpy(), "textures": textures.numpy(), "upstream": upstream.numpy()}
    for name, params in cases.items():
        p = [x.clone().requires_grad_(True) for x in params]
        f = faces.clone().requires_grad_(True)
        t = textures.clone().requires_grad_(True)
        lit = mod.lighting(f, t * 1.0, *p)          # (the reference multiplies its argument in place)
        (lit * upstream).sum().backward()
        out[f"{name}/lit"] = lit.detach().numpy()
        out[f"{name}/grad_faces"] = f.grad.numpy()
        out[f"{name}/grad_textures"] = t.grad.numpy()
        for n, x in zip(NAMES, p):
            out[f"{name}/{n}"] = x.detach().numpy()
            out[f"{name}/grad_{n}"] = x.grad.numpy()
    np.savez_compressed(os.path.join(HERE, "light_golden.npz"), **out)
    print("wrote", os.path.join(HERE, "light_golden.npz"), len(out), "arrays")


if __name__ == "__main__":
    main()
