#!/usr/bin/env python3
"""Cost of a per-view learnable light in the fit step: one render_fit_loss step (+ backward) at the benchmark's shape --
32 look_at views of grid_mesh(225), 512x512, texture size 2 -- with the constant light and with a [32]-view light whose five
parameters require grad, each as a captured step (graph.CapturedStep), median of --steps replays.  Prints one JSON line."""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deep3dmap_amd import neural_renderer as nr, synthetic  # noqa: E402
from deep3dmap_amd.graph import CapturedStep  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--views", type=int, default=32)
    args = ap.parse_args()
    B, s = args.views, 512
    v, tri = synthetic.grid_mesh(225)
    tex = synthetic.random_textures(tri.shape[0], 2)
    v = torch.from_numpy(v)[None].cuda().requires_grad_(True)
    tri = torch.from_numpy(tri)[None].cuda()
    tex = torch.from_numpy(tex)[None].cuda().requires_grad_(True)
    ang = torch.arange(B, dtype=torch.float32) * (2 * math.pi / B)
    eyes = torch.stack([2.5 * torch.sin(ang), 0.4 * torch.ones(B), -2.5 * torch.cos(ang)], 1).cuda()
    g = torch.Generator().manual_seed(0)
    targets = (torch.rand(B, 3, s, s, generator=g).cuda(), torch.rand(B, s, s, generator=g).cuda() + 2,
               (torch.rand(B, s, s, generator=g) > 0.5).float().cuda(), torch.ones(B, s, s).cuda())
    out = {"views": B, "image_size": s, "faces": int(tri.shape[1])}
    for name in ("constant", "per_view_learnable"):
        r = nr.Renderer(camera_mode="look_at", image_size=s, anti_aliasing=False)
        r.eye = eyes
        params = [v, tex]
        if name != "constant":
            lp = [torch.full((B,), 0.5), torch.full((B,), 0.5), torch.ones(B, 3), torch.ones(B, 3),
                  torch.tensor([0.0, 1.0, 0.0]).repeat(B, 1)]
            lp = [x.cuda().requires_grad_(True) for x in lp]
            for a, x in zip(("light_intensity_ambient", "light_intensity_directional", "light_color_ambient",
                             "light_color_directional", "light_direction"), lp):
                setattr(r, a, x)
            params += lp

        def step(r=r, params=params):
            for p in params:
                p.grad = None
            loss = r.render_fit_loss(v, tri, tex, targets)
            loss.backward()
            return loss.detach()
        run = CapturedStep(step).capture()
        times = []
        for _ in range(args.steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b))
        times.sort()
        out[name + "_ms"] = times[len(times) // 2]
        run.release()
    out["ratio"] = out["per_view_learnable_ms"] / out["constant_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
