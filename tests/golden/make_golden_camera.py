#!/usr/bin/env python3
"""
Regenerates tests/golden/camera_golden.npz.  BUILD CONTAINER ONLY: needs /root/reference.

The reference's cameras (NR/look_at.py, look.py, perspective.py, projection.py), imported by file path and run on the CPU
under autograd: transformed vertices and the gradients of every camera parameter and of the vertices for one upstream
gradient -- look_at and look each followed by perspective (as NR/renderer.py applies them) and projection, each with
shared ([3] / [1,...]) and per-batch ([bs,...]) parameters.  The vertices stay off the optical axis (projection.py's
sqrt(x^2 + y^2)**2 has no finite derivative there).  Only inputs and numeric outputs are stored
(tests/test_gpu_camera_params.py).

Usage:  python tests/golden/make_golden_camera.py
"""
import importlib.util
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
NR = "/root/reference/pnpmodules/neural_renderer/neural_renderer"


def _load(name):
    spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(NR, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return getattr(mod, name)


def main():
    look_at, look, perspective, projection = (_load(n) for n in ("look_at", "look", "perspective", "projection"))
    torch.manual_seed(5)
    bs, nv = 2, 50  # (bs != 3: the reference's torch.cross without dim crosses along the first axis of size 3)
    vertices = torch.rand(bs, nv, 3) * torch.tensor([0.8, 0.8, 0.6]) + torch.tensor([0.15, 0.1, -0.3])
    upstream = torch.randn(bs, nv, 3)
    rot = torch.linalg.qr(torch.randn(bs, 3, 3))[0]
    rot = rot * torch.sign(torch.linalg.det(rot))[:, None, None]
    kmat = torch.tensor([[300., 2., 128.], [0., 310., 120.], [0., 0., 1.]])
    cases = {
        "look_at_shared": ("look_at", [torch.tensor([0.3, 0.6, -2.5]), torch.tensor([0.1, 0.0, 0.2]),
                                       torch.tensor([0.05, 1.0, 0.1])]),
        "look_at_per_batch": ("look_at", [torch.tensor([[0.3, 0.6, -2.5], [-0.8, 0.2, -2.2]]),
                                          torch.tensor([[0.1, 0.0, 0.2], [0.0, 0.1, 0.0]]),
                                          torch.tensor([[0.05, 1.0, 0.1], [0.0, 1.0, 0.0]])]),
        "look_shared": ("look", [torch.tensor([0.3, 0.6, -2.5]), torch.tensor([0.05, -0.1, 1.0]),
                                 torch.tensor([0.0, 1.0, 0.1])]),
        "look_per_batch": ("look", [torch.tensor([[0.3, 0.6, -2.5], [-0.8, 0.2, -2.2]]),
                                    torch.tensor([[0.05, -0.1, 1.0], [0.2, 0.0, 1.0]]),
                                    torch.tensor([[0.0, 1.0, 0.1], [0.1, 1.0, 0.0]])]),
        "projection_shared": ("projection", [kmat[None], rot[:1], torch.tensor([[[0.1, -0.2, 3.0]]]),
                                             torch.tensor([[0.05, -0.02, 0.001, 0.002, 0.01]])]),
        "projection_per_batch": ("projection", [kmat[None].repeat(bs, 1, 1) + torch.randn(bs, 3, 3) * torch.tensor(
                                                    [[5., 1., 3.], [0., 5., 3.], [0., 0., 0.]]), rot,
                                                torch.tensor([[[0.1, -0.2, 3.0]], [[0.0, 0.1, 2.5]]]),
                                                torch.tensor([[0.05, -0.02, 0.001, 0.002, 0.01],
                                                              [0.02, 0.01, -0.002, 0.001, 0.0]])]),
    }
    out = {"vertices": vertices.numpy(), "upstream": upstream.numpy(), "orig_size": np.float32(256.0),
           "angle": np.float32(30.0)}
    for name, (kind, params) in cases.items():
        p = [x.clone().requires_grad_(True) for x in params]
        v = vertices.clone().requires_grad_(True)
        if kind == "look_at":
            o = perspective(look_at(v, p[0], p[1], p[2]), angle=30.)
        elif kind == "look":
            o = perspective(look(v, p[0], p[1], p[2]), angle=30.)
        else:
            o = projection(v, p[0], p[1], p[2], p[3], 256.)
        (o * upstream).sum().backward()
        out[f"{name}/out"] = o.detach().numpy()
        out[f"{name}/grad_vertices"] = v.grad.numpy()
        for k, x in enumerate(p):
            out[f"{name}/p{k}"] = x.detach().numpy()
            out[f"{name}/grad_p{k}"] = x.grad.numpy()
    np.savez_compressed(os.path.join(HERE, "camera_golden.npz"), **out)
    print("wrote", os.path.join(HERE, "camera_golden.npz"), len(out), "arrays")


if __name__ == "__main__":
    main()
