#!/usr/bin/env python3
"""Cost of the smooth-shading node (neural_renderer/smooth_shading.py) at the benchmark's mesh, grid_mesh(225) (V = 50,625,
F = 100,352), for B = 1 and 32 sets of vertices and colours under one light each: nr.sh_vertex_colors beside the eager-torch
composition a caller writes without it -- face normals by cross product, index_add_ into the vertices (float atomics), the
norm, the clamp, nr.sh_basis and an einsum -- forward alone and forward + backward (vertices, colours and sh all require
grad).  The two forms alternate in one call; a timed region is --iters calls between two device events; after warm-up, the
median of --regions regions, per call (eager launches, host time included).  Also the kernels' own times (the library's
d3m_timing events around each launch, mean of 5; not a profiler trace) and the largest difference between the two forms.

Writes one JSON object to --out and prints it."""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deep3dmap_amd import _lib, neural_renderer as nr, synthetic  # noqa: E402
from deep3dmap_amd.build import LOAD_PATH  # noqa: E402


def region_ms(fn, iters):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def median(xs):
    return sorted(xs)[len(xs) // 2]


def alternate(forms, regions, iters, warmup=2):
    times = {name: [] for name in forms}
    for rep in range(regions + warmup):
        for name, fn in forms.items():
            t = region_ms(fn, iters)
            if rep >= warmup:
                times[name].append(t)
    return {name: median(t) for name, t in times.items()}


def eager_shade(x, faces_long, colors, sh):
    """the composition without the node: [B,V,3], [F,3] i64, [B,V,3], [B,3,9] -> [B,V,3]"""
    x0, x1, x2 = (x[:, faces_long[:, c]] for c in range(3))
    face_normals = torch.linalg.cross(x1 - x0, x2 - x0)
    s = torch.zeros_like(x)
    for c in range(3):
        s = s.index_add(1, faces_long[:, c], face_normals)
    n = s / torch.linalg.vector_norm(s, dim=-1, keepdim=True).clamp(min=1e-6)
    return colors * torch.einsum("bkj,bvj->bvk", sh, nr.sh_basis(n))


def case(B, regions, iters, n=225):
    v, tri = synthetic.grid_mesh(n)
    V, F = v.shape[0], tri.shape[0]
    faces = torch.from_numpy(tri).cuda()
    faces_long = faces.long()
    gen = torch.Generator().manual_seed(B)
    x = (torch.from_numpy(v)[None] + 0.001 * torch.randn(B, V, 3, generator=gen)).cuda().requires_grad_(True)
    colors = (0.2 + 0.7 * torch.rand(B, V, 3, generator=gen)).cuda().requires_grad_(True)
    sh = (torch.rand(B, 3, 9, generator=gen) - 0.5 + torch.tensor([2.0] + [0.0] * 8)).cuda().requires_grad_(True)
    g = torch.randn(B, V, 3, generator=gen).cuda()
    leaves = (x, colors, sh)
    forms = {"node": lambda: nr.sh_vertex_colors(x, faces, colors, sh), "eager": lambda: eager_shade(x, faces_long, colors, sh)}

    def both(forward):
        def run():
            return torch.autograd.grad(forward(), leaves, g)
        return run

    def no_grad(forward):
        def run():
            with torch.no_grad():
                return forward()
        return run

    with torch.no_grad():
        out = {name: f() for name, f in forms.items()}
    grads = {name: both(f)() for name, f in forms.items()}
    rel = lambda a, b: float((a - b).abs().max()) / float(b.abs().max())       # noqa: E731
    diff = dict(shaded=rel(out["node"], out["eager"]),
                **{k: rel(a, b) for k, a, b in zip(("grad_vertices", "grad_colors", "grad_sh"), grads["node"], grads["eager"])})
    fwd = alternate({name: no_grad(f) for name, f in forms.items()}, regions, iters)
    fb = alternate({name: both(f) for name, f in forms.items()}, regions, iters)
    _lib.collect_kernel_times()
    _lib.kernel_timing(True)
    for _ in range(5):
        both(forms["node"])()
    kernels = {k: ms / c for k, (c, ms) in _lib.collect_kernel_times().items()}
    _lib.kernel_timing(False)
    return dict(V=V, F=F, B=B, node_forward_ms=fwd["node"], eager_forward_ms=fwd["eager"],
                node_forward_backward_ms=fb["node"], eager_forward_backward_ms=fb["eager"],
                eager_over_node_forward=fwd["eager"] / fwd["node"], eager_over_node_forward_backward=fb["eager"] / fb["node"],
                kernel_ms=kernels, node_kernels_sum_ms=sum(kernels.values()), relative_difference_to_eager=diff)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth_shading_cost.json"))
    args = ap.parse_args()
    out = {"library_sha256_16": hashlib.sha256(open(LOAD_PATH, "rb").read()).hexdigest()[:16],
           "cases": [case(B, args.regions, args.iters) for B in (1, 32)],
           "timing": f"device events around {args.iters} calls (eager launches, host time included), forms alternating, "
                     f"median of {args.regions} regions after 2 warm-up regions, per call"}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
