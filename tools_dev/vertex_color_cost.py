#!/usr/bin/env python3
"""Cost of learnable per-vertex colours (neural_renderer/vertex_colors.py) at the benchmark's mesh, grid_mesh(225)
(V = 50,625, F = 100,352): (a) the node's forward (colours -> cubes) and adjoint (cube gradient -> colour gradient) beside
the same two of the eager-torch composition colors[faces] -> vcolor_to_texture_cube -> autograd -- the two forms alternate
in one call, device events around synchronised work, after warm-up, medians of --reps -- and the one-time adjacency build;
(b) a MultiViewFit step (32 views, 512x512, one rank, captured) with vertex_colors and with cube textures, alternating,
median of --steps, and the bytes each form's step exchanges (its flat all-reduce buffer).  Writes one JSON object to --out
and prints it."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deep3dmap_amd import neural_renderer as nr, synthetic  # noqa: E402
from deep3dmap_amd.core.renderer_utils import vcolor_to_texture_cube  # noqa: E402
from deep3dmap_amd.multiview import MultiViewFit  # noqa: E402
from deep3dmap_amd.neural_renderer import vertex_colors  # noqa: E402


def timed_ms(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def median(xs):
    return sorted(xs)[len(xs) // 2]


def eager_cubes(colors, faces_long):
    """the composition a caller writes without the node: [V,3] -> [1,F,2,2,2,3]"""
    return vcolor_to_texture_cube(colors[faces_long].permute(2, 0, 1)[None])


def kernels(reps, n=225):
    v, tri = synthetic.grid_mesh(n)
    V, F = v.shape[0], tri.shape[0]
    faces = torch.from_numpy(tri).cuda()
    faces_long = faces.long()
    gen = torch.Generator().manual_seed(0)
    colors = torch.rand(V, 3, generator=gen).cuda().requires_grad_(True)
    g = torch.randn(1, F, 2, 2, 2, 3, generator=gen).cuda()
    builds = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        A = vertex_colors.build_adjacency(faces, V)
        torch.cuda.synchronize()
        builds.append((time.perf_counter() - t0) * 1e3)
    forms = {"hip": lambda: nr.textures_from_vertex_colors(colors, faces), "eager": lambda: eager_cubes(colors, faces_long)}
    times = {f"{name}_{part}_ms": [] for name in forms for part in ("forward", "adjoint")}
    for rep in range(reps + 3):
        for name, fwd in forms.items():
            t_f, out = timed_ms(fwd)
            t_a, _ = timed_ms(lambda: torch.autograd.grad(out, colors, g))
            if rep >= 3:                                    # (the first three rounds warm up)
                times[f"{name}_forward_ms"].append(t_f)
                times[f"{name}_adjoint_ms"].append(t_a)
    res = {k: median(x) for k, x in times.items()}
    same = torch.equal(forms["hip"]().detach(), forms["eager"]().detach())
    res.update(vertices=V, faces=F, adjacency_build_ms=median(builds), long_rows=int(A.csr.num_long_rows),
               max_valence=int((A.csr.offsets[1:] - A.csr.offsets[:-1]).max()), forward_equals_eager_bitwise=bool(same),
               timing="events around each call (eager launch, host time included), forms alternating, median")
    return res


def fit_steps(steps, B=32, s=512, n=225):
    v, tri = synthetic.grid_mesh(n)
    colors = np.random.default_rng(1).random((v.shape[0], 3), dtype=np.float32)
    eyes = synthetic.camera_ring(B)
    with torch.no_grad():
        cubes = nr.textures_from_vertex_colors(torch.from_numpy(colors).cuda(), torch.from_numpy(tri).cuda())[0].cpu().numpy()
    fits = {"vertex_colors": MultiViewFit(v, tri, None, eyes, image_size=s, vertex_colors=colors),
            "cubes": MultiViewFit(v, tri, cubes, eyes, image_size=s)}
    out = {"views": B, "image_size": s, "faces": int(tri.shape[0]), "vertices": int(v.shape[0])}
    for name, fit in fits.items():
        fit.set_targets_from(synthetic.perturb(v))
        fit.step()
        fit.capture_graph()
        out[name + "_exchange_bytes_per_step"] = 4 * fit._flat.numel()
    times = {name: [] for name in fits}
    for rep in range(steps + 3):
        for name, fit in fits.items():
            t, _ = timed_ms(fit.step)
            if rep >= 3:
                times[name].append(t)
    for name in fits:
        out[name + "_step_ms"] = median(times[name])
    out["ratio"] = out["vertex_colors_step_ms"] / out["cubes_step_ms"]
    out["multi_gpu_effect_of_the_smaller_exchange"] = "unmeasured on hardware"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vertex_color_cost.json"))
    args = ap.parse_args()
    out = {"kernels": kernels(args.reps), "fit_step": fit_steps(args.steps)}
    line = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
