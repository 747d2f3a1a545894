#!/usr/bin/env python3
"""Cost of fusing baked view textures and filling their unseen texels (neural_renderer/uv_fill.py) at the headline scene.

nr.fuse_uv_textures beside the composed route a caller writes without the node, on the same inputs: the bake outputs
(texture [B,T,T,C], mask [B,T,T]) of --views look_at cameras on a ring at 512 x 512 around grid_mesh(225) (100,352 triangles),
a lat-long uv layout at T = 512, C = 3.  The composed route: the torch fusion sum(mask texture) / sum(mask), then a push-pull
with one avg_pool2d of the sums and of the counts per level on the way up and one bilinear interpolate (scale 2,
align_corners=False: the node's taps on a side that is a power of two) and one select per level on the way down --
differentiable in the textures like the node.  Forward alone and forward + backward; the two forms alternate; a timed region is
--iters calls between two device events; after warm-up, the median of --regions regions, per call (eager launches, host time
included).  Also the node's kernels' own times (the library's d3m_timing events around each launch, mean of 5; not a rocprofv3
trace).

Writes one JSON object to --out and prints it."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deep3dmap_amd import _lib, neural_renderer as nr, synthetic  # noqa: E402
from deep3dmap_amd.build import LOAD_PATH  # noqa: E402
from tools_dev.uv_bake_cost import alternate  # noqa: E402


def composed(textures, weights):
    """(texture [T,T,C], valid [T,T]) of the composed route; T a power of two, background zeros"""
    w = weights.clamp(min=0)
    m = w.sum(0)
    valid = m > 0
    v0 = (w[..., None] * textures).sum(0) / m.clamp(min=1e-30)[..., None]
    sums = [(v0 * valid[..., None]).permute(2, 0, 1)[None]]
    counts = [valid.float()[None, None]]
    while sums[-1].shape[-1] > 1:
        sums.append(F.avg_pool2d(sums[-1], 2) * 4)
        counts.append(F.avg_pool2d(counts[-1], 2) * 4)
    mean = lambda l: sums[l] / counts[l].clamp(min=1)
    f = mean(len(sums) - 1)
    for l in range(len(sums) - 2, -1, -1):
        f = torch.where(counts[l] > 0, mean(l), F.interpolate(f, scale_factor=2, mode="bilinear", align_corners=False))
    return f[0].permute(1, 2, 0), valid.float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--mesh-n", type=int, default=225)
    ap.add_argument("--image-size", type=int, default=512)
    ap.add_argument("--texture-size", type=int, default=512)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    B, s, T, C, n = args.views, args.image_size, args.texture_size, args.channels, args.mesh_n
    if T & (T - 1):
        raise SystemExit("--texture-size must be a power of two (the composed route's interpolate)")
    v_np, tri_np = synthetic.grid_mesh(n)
    r = nr.Renderer(image_size=s, anti_aliasing=False, camera_mode="look_at", fill_back=True)
    r.eye = torch.from_numpy(synthetic.camera_ring(B)).float().cuda()
    faces = torch.from_numpy(tri_np).int().cuda()[None]
    v = torch.from_numpy(v_np).float().cuda()[None].repeat(B, 1, 1)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    vertex_uv = np.stack([0.02 + 0.96 * j / (n - 1), 0.02 + 0.96 * i / (n - 1)], -1).reshape(-1, 2).astype(np.float32)
    faces_uv = torch.from_numpy(vertex_uv[tri_np]).cuda().contiguous()
    gen = torch.Generator().manual_seed(1)
    images = torch.rand(B, C, s, s, generator=gen).cuda()
    with torch.no_grad():
        baked, mask = r.bake_uv_texture(v, faces, images, faces_uv, T)
    textures = baked.clone().requires_grad_(True)
    g = torch.randn(T, T, C, generator=gen).cuda()

    forwards = {"node": lambda: nr.fuse_uv_textures(textures, mask), "composed": lambda: composed(textures, mask)}

    def both(forward):
        def run():
            textures.grad = None
            forward()[0].backward(g)
            return (textures.grad,)
        return run

    def no_grad(forward):
        def run():
            with torch.no_grad():
                return forward()
        return run

    results = {k: [t.detach().clone() for t in f()] for k, f in forwards.items()}
    grads = {k: [t.clone() for t in both(f)()] for k, f in forwards.items()}
    rel = lambda a, b: float((a - b).abs().max()) / float(b.abs().max())
    diff = dict(valid_disagreements=int((results["node"][1] != results["composed"][1]).sum()), texels=T * T,
                valid_texels=int(results["node"][1].sum()), texture=rel(results["node"][0], results["composed"][0]),
                grad_textures=rel(grads["node"][0], grads["composed"][0]))
    fwd = alternate({k: no_grad(f) for k, f in forwards.items()}, args.regions, args.iters)
    fb = alternate({k: both(f) for k, f in forwards.items()}, args.regions, args.iters)
    _lib.collect_kernel_times()
    _lib.kernel_timing(True)
    for _ in range(5):
        both(forwards["node"])()
    kernels = {k: dict(launches_per_call=c / 5, ms_per_launch=ms / c) for k, (c, ms) in _lib.collect_kernel_times().items()}
    _lib.kernel_timing(False)
    out = {"library_sha256_16": hashlib.sha256(open(LOAD_PATH, "rb").read()).hexdigest()[:16],
           "scene": dict(triangles=int(tri_np.shape[0]), views=B, image_size=s, texture_size=T, channels=C),
           "node_forward_ms": fwd["node"], "composed_forward_ms": fwd["composed"],
           "node_forward_backward_ms": fb["node"], "composed_forward_backward_ms": fb["composed"],
           "composed_over_node_forward": fwd["composed"] / fwd["node"],
           "composed_over_node_forward_backward": fb["composed"] / fb["node"],
           "node_kernels": kernels, "relative_difference_to_composed": diff,
           "timing": f"device events around {args.iters} calls (eager launches, host time included), forms alternating, "
                     f"median of {args.regions} regions after 2 warm-up regions, per call"}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
