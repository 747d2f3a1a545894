#!/usr/bin/env python3
"""Cost of the chamfer distance between point sets (neural_renderer/point_sets.py) at the headline mesh's size.

nr.chamfer_distance (squared, both directions) beside the composed route a caller writes without the node, on the same
inputs, at three sizes: N = M = 50,625 (the vertices of grid_mesh(225) against a scan of the same size) with B = 1 and B = 8,
and N = 5,000 against M = 1,000,000 (few queries against a large scan: the targets are split over workgroups).  The composed
route: per batch element and direction torch.cdist in chunks of at most 2^26 distances (--cdist-mode: torch's default
compute mode; "donot_use_mm_for_euclid_dist" forms the distances from the differences as the node does, but its `min` named
the k-d tree's neighbour for a quarter of the points only on the build this was measured with), `min` per chunk, then the
squared distances to the gathered neighbours, whose backward is an index_add_.  Forward alone and forward + backward; the two forms alternate; a timed region is --iters calls
between two device events; after warm-up, the median of --regions regions, per call (eager launches, host time included).
Also the node's kernels' own times (the library's d3m_timing events around each launch, mean of 3; not a rocprofv3 trace)
and the split counts the node chose.

Writes one JSON object to --out and prints it."""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deep3dmap_amd import _lib, neural_renderer as nr  # noqa: E402
from deep3dmap_amd.build import LOAD_PATH  # noqa: E402
from deep3dmap_amd.neural_renderer import point_sets  # noqa: E402
from tools_dev.uv_bake_cost import alternate  # noqa: E402

SIZES = {"N50625_M50625_B1": (1, 50625, 50625), "N50625_M50625_B8": (8, 50625, 50625), "N5000_M1000000_B1": (1, 5000, 1000000)}
CHUNK_DISTANCES = 1 << 26
CDIST_MODE = "use_mm_for_euclid_dist_if_necessary"


def nearest_composed(p, q, mode):
    """index [n] of every point of p [n,3] in q [m,3]: chunked cdist and min"""
    rows = max(1, CHUNK_DISTANCES // q.shape[0])
    with torch.no_grad():
        return torch.cat([torch.cdist(p[r:r + rows], q, compute_mode=mode).min(1).indices for r in range(0, p.shape[0], rows)])


def composed(a, b, mode):
    """value [B] of the squared chamfer distance of a [B,N,3] and b [B,M,3], both directions"""
    values = []
    for x, y in zip(a, b):
        ab, ba = nearest_composed(x, y, mode), nearest_composed(y, x, mode)
        values.append(((x - y[ab]) ** 2).sum(-1).mean() + ((y - x[ba]) ** 2).sum(-1).mean())
    return torch.stack(values)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=list(SIZES), choices=list(SIZES))
    ap.add_argument("--regions", type=int, default=3)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--cdist-mode", default=CDIST_MODE, help="torch.cdist's compute_mode in the composed route")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    out = {"library_sha256_16": hashlib.sha256(open(LOAD_PATH, "rb").read()).hexdigest()[:16],
           "options": dict(squared=True, weight_ab=1.0, weight_ba=1.0), "cdist_compute_mode": args.cdist_mode, "tile": point_sets.TILE,
           "queries_per_workgroup": 256 * point_sets.QUERIES_PER_LANE,
           "timing": f"device events around {args.iters} calls (eager launches, host time included), forms alternating, "
                     f"median of {args.regions} regions after 2 warm-up regions, per call"}
    gen = torch.Generator().manual_seed(1)
    for name in args.sizes:
        B, N, M = SIZES[name]
        a = (torch.rand(B, N, 3, generator=gen) * 2 - 1).cuda().requires_grad_(True)
        b = (torch.rand(B, M, 3, generator=gen) * 2 - 1).cuda().requires_grad_(True)
        g = torch.randn(B, generator=gen).cuda()
        forwards = {"node": lambda: nr.chamfer_distance(a, b), "composed": lambda: composed(a, b, args.cdist_mode)}

        def both(forward):
            def run():
                a.grad = b.grad = None
                forward().backward(g)
                return (a.grad, b.grad)
            return run

        def no_grad(forward):
            def run():
                with torch.no_grad():
                    return (forward(),)
            return run

        values = {k: f().detach().clone() for k, f in forwards.items()}
        grads = {k: [t.clone() for t in both(f)()] for k, f in forwards.items()}
        rel = lambda p, q: float((p - q).abs().max()) / float(q.abs().max())
        fwd = alternate({k: no_grad(f) for k, f in forwards.items()}, args.regions, args.iters)
        fb = alternate({k: both(f) for k, f in forwards.items()}, args.regions, args.iters)
        _lib.collect_kernel_times()
        _lib.kernel_timing(True)
        for _ in range(3):
            both(forwards["node"])()
        kernels = {k: dict(launches_per_call=c / 3, ms_per_launch=ms / c) for k, (c, ms) in _lib.collect_kernel_times().items()}
        _lib.kernel_timing(False)
        out[name] = {"B": B, "N": N, "M": M,
                     "splits": dict(a_to_b=point_sets.auto_splits(B, N, M), b_to_a=point_sets.auto_splits(B, M, N)),
                     "node_forward_ms": fwd["node"], "composed_forward_ms": fwd["composed"],
                     "node_forward_backward_ms": fb["node"], "composed_forward_backward_ms": fb["composed"],
                     "composed_over_node_forward": fwd["composed"] / fwd["node"],
                     "composed_over_node_forward_backward": fb["composed"] / fb["node"], "node_kernels": kernels,
                     "relative_difference_to_composed": dict(value=rel(values["node"], values["composed"]),
                                                             grad_a=rel(grads["node"][0], grads["composed"][0]),
                                                             grad_b=rel(grads["node"][1], grads["composed"][1]))}
        torch.cuda.empty_cache()
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
