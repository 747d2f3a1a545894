#!/usr/bin/env python3
"""Cost of the linear morphable-model node (neural_renderer/morphable.py).

--part kernels: forward + backward of nr.morphable_vertices beside the reference's own formulation in eager torch
(param2points_bfm's matmuls and add, and their autograd) on the same hashed inputs: at Basel size (R = 159,645, K = 228) for
B in {1, 16, 32} and at the benchmark's mesh (R = 151,875) with K = 64, B = 1.  The two forms alternate; a timed region is
--iters forward + backward pairs between two device events; after warm-up, the median of --regions regions, per pair.  Also
each direction alone, the kernels' own times (d3m_timing), and the byte floor 2 * 4 * R * K * ceil(B / 16) at 8 TB/s.

--part fit: a one-rank MultiViewFit(morphable=...) step beside the plain step (free vertices) on grid_mesh(9) (4 views,
64x64, K = 7) and on the benchmark's mesh grid_mesh(225) (32 views, 512x512, K = 64), captured, alternating, median of
--steps; the exchange sizes follow from the shapes.

Writes one JSON object per part to --out and prints it."""
import argparse
import hashlib
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deep3dmap_amd import _lib, neural_renderer as nr, synthetic  # noqa: E402
from deep3dmap_amd.build import LOAD_PATH  # noqa: E402
from deep3dmap_amd.multiview import MultiViewFit  # noqa: E402
from deep3dmap_amd.neural_renderer import morphable as mb  # noqa: E402

HBM_BYTES_PER_S = 8e12


def hashed(rows, cols, salt, lo=-1.0, hi=1.0):
    r = np.arange(rows, dtype=np.int64)[:, None]
    k = np.arange(cols, dtype=np.int64)[None, :]
    h = (r * 1315423911 + k * 2654435761 + salt * 97531) % 65521
    return (lo + (hi - lo) * (h / 65520.0)).astype(np.float32)


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


def kernel_case(R, K, B, regions, iters):
    basis = torch.from_numpy(hashed(R, K, 1)).cuda()
    mean = torch.from_numpy(hashed(R, 1, 2, -100.0, 100.0)[:, 0]).cuda()
    scale = torch.from_numpy(hashed(1, K, 3, 0.5, 1.5)[0]).cuda()
    coeffs = torch.from_numpy(hashed(B, K, 4)).cuda().requires_grad_(True)
    grad = torch.from_numpy(hashed(B, R, 5)).cuda()
    split = K - max(1, K // 8)          # the reference multiplies two bases (identity | expression) and adds
    w, w_exp = basis[:, :split].contiguous(), basis[:, split:].contiguous()

    def node():
        coeffs.grad = None
        nr.morphable_vertices(coeffs, basis, mean, scale).backward(grad.view(B, -1, 3))
        return coeffs.grad

    def eager():
        coeffs.grad = None
        alpha = coeffs[:, :split].view(-1, split, 1) * scale[:split].view(1, split, 1)
        beta = coeffs[:, split:].view(-1, K - split, 1) * scale[split:].view(1, K - split, 1)
        face = torch.matmul(w[None], alpha) + torch.matmul(w_exp[None], beta) + mean.view(1, R, 1)
        face.reshape(-1, R // 3, 3).backward(grad.view(B, -1, 3))
        return coeffs.grad

    c2 = coeffs.detach()
    g_node, g_eager = node().clone(), eager().clone()
    res = alternate({"node": node, "eager": eager}, regions, iters)
    alone = alternate({"forward": lambda: mb.forward(c2, basis, mean, scale),
                       "backward": lambda: mb.backward(grad, basis, scale)}, regions, iters)
    _lib.collect_kernel_times()
    _lib.kernel_timing(True)
    for _ in range(5):
        node()
    kernels = {k: ms / c for k, (c, ms) in _lib.collect_kernel_times().items()}
    _lib.kernel_timing(False)
    floor = 2 * 4 * R * K * math.ceil(B / mb.SETS_PER_PASS) / HBM_BYTES_PER_S * 1e3
    return dict(R=R, K=K, B=B, node_forward_backward_ms=res["node"], eager_forward_backward_ms=res["eager"],
                node_forward_alone_ms=alone["forward"], node_backward_alone_ms=alone["backward"], kernel_ms=kernels,
                byte_floor_ms=floor, node_over_floor=res["node"] / floor,
                gradient_relative_difference=float((g_node - g_eager).abs().max()) / float(g_eager.abs().max()))


def kernels_part(args):
    cases = [(159645, 228, 1), (159645, 228, 16), (159645, 228, 32), (151875, 64, 1)]
    return {"cases": [kernel_case(R, K, B, args.regions, args.iters) for R, K, B in cases],
            "timing": f"device events around {args.iters} forward + backward pairs (eager launches, host time included), "
                      f"forms alternating, median of {args.regions} regions after 2 warm-up regions, per pair"}


def fit_case(n, views, size, K, steps):
    v, tri = synthetic.grid_mesh(n)
    cubes = hashed(tri.shape[0], 24, 6, 0.0, 1.0).reshape(-1, 2, 2, 2, 3)
    eyes = synthetic.camera_ring(views)
    basis, c0 = hashed(v.size, K, 7, -0.02, 0.02), hashed(1, K, 8)[0]
    model = nr.MorphableModel(v.reshape(-1), basis)
    fits = {"morphable": MultiViewFit(None, tri, cubes, eyes, image_size=size, morphable=model, coeffs=c0)}
    fits["plain"] = MultiViewFit(fits["morphable"].vertices.detach().cpu().numpy(), tri, cubes, eyes, image_size=size)
    out = dict(views=views, image_size=size, vertices=int(v.shape[0]), faces=int(tri.shape[0]), components=K)
    for name, fit in fits.items():
        fit.set_targets_from(synthetic.perturb(v))
        fit.step()
        fit.capture_graph()
        out[name + "_exchange_bytes_per_step"] = 4 * fit._flat.numel()
    res = alternate({name: fit.step for name, fit in fits.items()}, steps, 1, warmup=3)
    for name in fits:
        out[name + "_step_ms"] = res[name]
    out["added_ms"] = out["morphable_step_ms"] - out["plain_step_ms"]
    return out


def fit_part(args):
    return {"cases": [fit_case(9, 4, 64, 7, args.steps), fit_case(225, 32, 512, 64, args.steps)],
            "timing": f"device events around each captured step, forms alternating, median of {args.steps}",
            "multi_gpu": "exchange sizes from shapes only; no exchange between GPUs was measured"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["kernels", "fit"], required=True)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    out = {"library_sha256_16": hashlib.sha256(open(LOAD_PATH, "rb").read()).hexdigest()[:16], "part": args.part}
    out.update(kernels_part(args) if args.part == "kernels" else fit_part(args))
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
