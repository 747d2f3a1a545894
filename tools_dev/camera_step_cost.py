#!/usr/bin/env python3
"""Cost of a learnable camera in the render nodes, each step captured (graph.CapturedStep), median of --steps replays:
(a) the benchmark's render_fit_loss step -- 32 look_at views of grid_mesh(225), 512x512, texture size 2 -- with constant
eyes and with learnable per-view eyes [32,3]; (b) an example-4-shaped step (neural_renderer's examples/example4.py:
constant vertices, a learnable [3] eye, silhouettes, squared error against a reference image) at 1 view @256 and 32 views
@512, in the node against the route the parent took for it -- the camera as a torch composition (look_at + perspective),
the [B,F',3,3] face gather and the reference-shaped silhouette rasterizer -- composed inline here.  Prints one JSON line."""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deep3dmap_amd import neural_renderer as nr, synthetic  # noqa: E402
from deep3dmap_amd.graph import CapturedStep  # noqa: E402
from deep3dmap_amd.neural_renderer import mesh_ops  # noqa: E402
from deep3dmap_amd.neural_renderer.rasterize import rasterize_silhouettes  # noqa: E402


def _median_ms(step, steps):
    run = CapturedStep(step).capture()
    times = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    run.release()
    times.sort()
    return times[len(times) // 2]


def _unit(x):
    return x / x.norm(dim=-1, keepdim=True).clamp_min(1e-5)


_WIDTH = float(torch.tan(torch.tensor(30.0 / 180 * math.pi, dtype=torch.float32)))       # perspective.py:15-17


def _parent_silhouettes(v, tri, eye, up, size):
    """the parent's route for a learnable eye: NR/look_at.py + perspective.py in torch operators, then the face gather and
    the reference-shaped rasterizer (`up` [B,3] on the device: nothing is uploaded inside the captured step)"""
    B = eye.shape[0]
    z = _unit(-eye)                 # (at = 0)
    x = _unit(torch.linalg.cross(up, z, dim=-1))
    y = _unit(torch.linalg.cross(z, x, dim=-1))
    sv = torch.einsum('bvk,bjk->bvj', v.expand(B, -1, -1) - eye[:, None, :], torch.stack((x, y, z), dim=1))
    zc = sv[..., 2]
    sv = torch.stack((sv[..., 0] / zc / _WIDTH, sv[..., 1] / zc / _WIDTH, zc), dim=-1)
    return rasterize_silhouettes(mesh_ops.gather_faces(sv, tri, True), size, True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--views", type=int, default=32)
    args = ap.parse_args()
    B, s = args.views, 512
    v, tri = synthetic.grid_mesh(225)
    tex = synthetic.random_textures(tri.shape[0], 2)
    v = torch.from_numpy(v)[None].cuda()
    tri = torch.from_numpy(tri)[None].cuda()
    tex = torch.from_numpy(tex)[None].cuda().requires_grad_(True)
    ang = torch.arange(B, dtype=torch.float32) * (2 * math.pi / B)
    eyes0 = torch.stack([2.5 * torch.sin(ang), 0.4 * torch.ones(B), -2.5 * torch.cos(ang)], 1).cuda()
    g = torch.Generator().manual_seed(0)
    targets = (torch.rand(B, 3, s, s, generator=g).cuda(), torch.rand(B, s, s, generator=g).cuda() + 2,
               (torch.rand(B, s, s, generator=g) > 0.5).float().cuda(), torch.ones(B, s, s).cuda())
    out = {"views": B, "image_size": s, "faces": int(tri.shape[1])}
    # (a) the headline fit step
    vg = v.clone().requires_grad_(True)
    for name in ("constant_eyes", "learnable_eyes"):
        r = nr.Renderer(camera_mode="look_at", image_size=s, anti_aliasing=False)
        r.eye = eyes0.clone().requires_grad_(name != "constant_eyes")
        params = [vg, tex] + ([r.eye] if r.eye.requires_grad else [])

        def step(r=r, params=params):
            for p in params:
                p.grad = None
            loss = r.render_fit_loss(vg, tri, tex, targets)
            loss.backward()
            return loss.detach()
        out["fit_" + name + "_ms"] = _median_ms(step, args.steps)
    out["fit_ratio"] = out["fit_learnable_eyes_ms"] / out["fit_constant_eyes_ms"]
    # (b) example 4's shape: constant vertices, one learnable eye, silhouettes, squared error
    for nv, size in ((1, 256), (B, 512)):
        ref = (torch.rand(nv, size, size, generator=g) > 0.5).float().cuda()
        vv = v.expand(nv, -1, -1).contiguous() if nv > 1 else v
        for route in ("node", "parent"):
            r = nr.Renderer(camera_mode="look_at", image_size=size)
            eye = torch.tensor([0.6, 1.0, -2.8], device="cuda", requires_grad=True)
            r.eye = eye
            up = torch.tensor([[0.0, 1.0, 0.0]], device="cuda").expand(nv, 3)

            def step(r=r, eye=eye, route=route, vv=vv, ref=ref, size=size, nv=nv, up=up):
                eye.grad = None
                if route == "node":
                    image = r(vv, tri, mode="silhouettes")
                else:
                    image = _parent_silhouettes(vv, tri, eye[None].expand(nv, 3), up, size)
                loss = torch.sum((image - ref) ** 2)
                loss.backward()
                return loss.detach()
            out[f"example4_{nv}x{size}_{route}_ms"] = _median_ms(step, args.steps)
        out[f"example4_{nv}x{size}_speedup"] = out[f"example4_{nv}x{size}_parent_ms"] / out[f"example4_{nv}x{size}_node_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
