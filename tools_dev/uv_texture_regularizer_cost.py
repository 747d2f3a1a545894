#!/usr/bin/env python3
"""Cost of the UV texture regularisers (neural_renderer/uv_texture_regularizers.py) at the headline scene's layout.

nr.uv_texture_regularizer beside the composed route a caller writes without the node, on the same inputs: a texture
[B,T,T,C] at T = 512, C = 3, B = 1 and B = 8, all four terms (smoothness with smooth_eps, symmetry, flatness, anchor with
reference weights), the mask nr.uv_layout_mask of a lat-long uv layout of grid_mesh(225) (100,352 triangles).  The composed
route: slices, a flip, masked sums and `where` in eager torch, differentiable in the texture like the node.  Forward alone
and forward + backward; the two forms alternate; a timed region is --iters calls between two device events; after warm-up,
the median of --regions regions, per call (eager launches, host time included).  Also the node's kernels' own times (the
library's d3m_timing events around each launch, mean of 5; not a rocprofv3 trace).

Writes one JSON object to --out and prints it."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deep3dmap_amd import _lib, neural_renderer as nr, synthetic  # noqa: E402
from deep3dmap_amd.build import LOAD_PATH  # noqa: E402
from tools_dev.uv_bake_cost import alternate  # noqa: E402

WEIGHTS = dict(smooth=0.7, smooth_eps=0.05, symmetry=1.3, flat=0.4, anchor=2.0)


def composed(x, mask, reference, reference_weights, smooth, smooth_eps, symmetry, flat, anchor):
    """value [B] of x [B,T,T,C] with a shared mask [T,T], reference [T,T,C] and weights [T,T]"""
    C, W = x.shape[-1], x.shape[2]
    a = mask > 0
    rho = lambda d: torch.sqrt(d * d + smooth_eps * smooth_eps) - smooth_eps
    mean = lambda s, n: torch.where(n > 0, s / (n.clamp(min=1e-30) * C), torch.zeros_like(s))
    ph, pv = a[:, :-1] & a[:, 1:], a[:-1] & a[1:]
    s = (rho(x[:, :, :-1] - x[:, :, 1:]) * ph[..., None]).sum((1, 2, 3)) + (rho(x[:, :-1] - x[:, 1:]) * pv[..., None]).sum((1, 2, 3))
    value = smooth * mean(s, (ph.sum() + pv.sum()).float())
    half = W // 2
    m = a[:, :half] & a.flip(1)[:, :half]
    value = value + symmetry * mean((((x[:, :, :half] - x.flip(2)[:, :, :half]) ** 2) * m[..., None]).sum((1, 2, 3)), m.sum().float())
    n = a.sum().float()
    mu = (x * a[..., None]).sum((1, 2), keepdim=True) / n.clamp(min=1)
    value = value + flat * mean((((x - mu) ** 2) * a[..., None]).sum((1, 2, 3)), n)
    r = torch.where((reference_weights > 0) & a, reference_weights, torch.zeros_like(reference_weights))
    return value + anchor * mean((r[..., None] * (x - reference) ** 2).sum((1, 2, 3)), r.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--mesh-n", type=int, default=225)
    ap.add_argument("--texture-size", type=int, default=512)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    T, C, n = args.texture_size, args.channels, args.mesh_n
    _, tri_np = synthetic.grid_mesh(n)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    vertex_uv = np.stack([0.02 + 0.96 * j / (n - 1), 0.02 + 0.96 * i / (n - 1)], -1).reshape(-1, 2).astype(np.float32)
    faces_uv = torch.from_numpy(vertex_uv[tri_np]).cuda().contiguous()
    mask = nr.uv_layout_mask(faces_uv, T)
    gen = torch.Generator().manual_seed(1)
    reference = torch.rand(T, T, C, generator=gen).cuda()
    weights = torch.rand(T, T, generator=gen).cuda()
    out = {"library_sha256_16": hashlib.sha256(open(LOAD_PATH, "rb").read()).hexdigest()[:16],
           "scene": dict(triangles=int(tri_np.shape[0]), texture_size=T, channels=C, active_texels=int((mask > 0).sum()),
                         texels=T * T, terms=WEIGHTS),
           "timing": f"device events around {args.iters} calls (eager launches, host time included), forms alternating, "
                     f"median of {args.regions} regions after 2 warm-up regions, per call"}
    for B in args.batches:
        x = torch.rand(B, T, T, C, generator=gen).cuda().requires_grad_(True)
        g = torch.randn(B, generator=gen).cuda()
        forwards = {"node": lambda: nr.uv_texture_regularizer(x, mask, reference=reference, reference_weights=weights, **WEIGHTS),
                    "composed": lambda: composed(x, mask, reference, weights, **WEIGHTS)}

        def both(forward):
            def run():
                x.grad = None
                forward().backward(g)
                return (x.grad,)
            return run

        def no_grad(forward):
            def run():
                with torch.no_grad():
                    return (forward(),)
            return run

        values = {k: f().detach().clone() for k, f in forwards.items()}
        grads = {k: both(f)()[0].clone() for k, f in forwards.items()}
        rel = lambda p, q: float((p - q).abs().max()) / float(q.abs().max())
        fwd = alternate({k: no_grad(f) for k, f in forwards.items()}, args.regions, args.iters)
        fb = alternate({k: both(f) for k, f in forwards.items()}, args.regions, args.iters)
        _lib.collect_kernel_times()
        _lib.kernel_timing(True)
        for _ in range(5):
            both(forwards["node"])()
        kernels = {k: dict(launches_per_call=c / 5, ms_per_launch=ms / c) for k, (c, ms) in _lib.collect_kernel_times().items()}
        _lib.kernel_timing(False)
        out[f"B{B}"] = {"node_forward_ms": fwd["node"], "composed_forward_ms": fwd["composed"],
                        "node_forward_backward_ms": fb["node"], "composed_forward_backward_ms": fb["composed"],
                        "composed_over_node_forward": fwd["composed"] / fwd["node"],
                        "composed_over_node_forward_backward": fb["composed"] / fb["node"], "node_kernels": kernels,
                        "relative_difference_to_composed": dict(value=rel(values["node"], values["composed"]),
                                                                grad_texture=rel(grads["node"], grads["composed"]))}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
