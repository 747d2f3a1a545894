#!/usr/bin/env python3
"""Cost of learnable uv images (neural_renderer/uv_textures.py) at the benchmark's mesh, grid_mesh(225) (F = 100,352) with
grid uv coordinates: (a) the forward (image -> cubes), the adjoint (cube gradient -> image gradient) and the one-time
transpose build, for texture size 2 / 4, 1024^2 / 2048^2 images, bilinear / nearest, with the transpose's size; (b) the
headline fit step -- render_fit_loss + backward, 32 look_at views, 512x512, texture size 2 -- with learnable cubes and with
a learnable 1024^2 image sampled into them, each captured (graph.CapturedStep), median of --steps replays, the way
light_step_cost.py times it.  Prints one JSON line."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deep3dmap_amd import neural_renderer as nr, synthetic  # noqa: E402
from deep3dmap_amd.graph import CapturedStep  # noqa: E402
from deep3dmap_amd.neural_renderer import uv_textures  # noqa: E402


def grid_uv(n):
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    uv = np.stack([j, i], -1).reshape(-1, 2).astype(np.float32) / (n - 1)
    return torch.from_numpy(uv[synthetic.grid_topology(n)]).cuda()


def median_ms(fn, reps):
    for _ in range(3):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2]


def captured_median_ms(step, steps):
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


def kernels(uv, reps):
    out = []
    F = uv.shape[0]
    for ts in (2, 4):
        for size in (1024, 2048):
            for bilinear in (True, False):
                img = torch.rand(size, size, 3, device="cuda")
                fwd = median_ms(lambda: nr.textures_from_image(img, uv, ts, 'REPEAT', bilinear), reps)
                builds = []
                for _ in range(3):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    T = uv_textures.build_transpose(uv, None, ts, size, size, 0, bilinear)
                    torch.cuda.synchronize()
                    builds.append((time.perf_counter() - t0) * 1e3)
                g = torch.randn(1, F * ts ** 3 * 3, device="cuda")
                adj = median_ms(lambda: uv_textures.uv_texture_adjoint(T, g), reps)
                sweep = {str(L): median_ms(lambda: uv_textures.uv_texture_adjoint(T._replace(lanes_per_row=L), g), reps)
                         for L in (1, 2, 4, 8, 16)}
                nnz = int(T.csr.items.shape[0])
                csr_bytes = 4 * (T.csr.offsets.numel() + T.csr.items.numel())
                out.append({"ts": ts, "image": size, "bilinear": bilinear, "forward_ms": fwd, "adjoint_ms": adj,
                            "build_ms": sorted(builds)[1], "entries": nnz, "csr_bytes": csr_bytes,
                            "long_rows": int(T.csr.num_long_rows), "chunks": int(T.csr.num_chunks),
                            "lanes_per_row": T.lanes_per_row, "adjoint_ms_by_lanes": sweep,
                            "mean_row": nnz / max(1, int((T.csr.offsets[1:] > T.csr.offsets[:-1]).sum())),
                            "adjoint_bytes_model": csr_bytes + 4 * g.numel() + 12 * size * size})
                del T
    return out


def fit_steps(steps, B=32, s=512, image=1024):
    v, tri = synthetic.grid_mesh(225)
    uv = grid_uv(225)
    F = tri.shape[0]
    v = torch.from_numpy(v)[None].cuda().requires_grad_(True)
    tri = torch.from_numpy(tri)[None].cuda()
    ang = torch.arange(B, dtype=torch.float32) * (2 * math.pi / B)
    eyes = torch.stack([2.5 * torch.sin(ang), 0.4 * torch.ones(B), -2.5 * torch.cos(ang)], 1).cuda()
    g = torch.Generator().manual_seed(0)
    targets = (torch.rand(B, 3, s, s, generator=g).cuda(), torch.rand(B, s, s, generator=g).cuda() + 2,
               (torch.rand(B, s, s, generator=g) > 0.5).float().cuda(), torch.ones(B, s, s).cuda())
    img = torch.rand(image, image, 3, generator=g).cuda().requires_grad_(True)
    cubes = nr.textures_from_image(img.detach(), uv, 2)[None].contiguous().requires_grad_(True)
    out = {"views": B, "image_size": s, "faces": F, "uv_image": image, "texture_size": 2}
    for name in ("cubes", "uv_image"):
        r = nr.Renderer(camera_mode="look_at", image_size=s, anti_aliasing=False)
        r.eye = eyes
        params = [v, cubes] if name == "cubes" else [v, img]

        def step(r=r, params=params, name=name):
            for p in params:
                p.grad = None
            tex = cubes if name == "cubes" else nr.textures_from_image(img, uv, 2)[None]
            loss = r.render_fit_loss(v, tri, tex, targets)
            loss.backward()
            return loss.detach()
        out[name + "_step_ms"] = captured_median_ms(step, steps)
    out["ratio"] = out["uv_image_step_ms"] / out["cubes_step_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    uv = grid_uv(225)
    out = {"faces": int(uv.shape[0]), "kernels": kernels(uv, args.reps)}
    out["fit_step"] = fit_steps(args.steps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
