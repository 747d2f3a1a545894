#!/usr/bin/env python3
"""Cost of baking view images into a uv texture (neural_renderer/uv_bake.py) at the headline scene.

nr.bake_uv_texture beside the composed route a caller must write without the node, on the same inputs: grid_mesh(225) (100,352
triangles), --views look_at cameras on a ring at 512 x 512, a lat-long uv layout at T = 512, C = 3.  The composed route:
nr.interpolate_vertex_attributes of the unrolled corners' (x z, y z, z) over the layout record, the perspective division, a
z-buffer test in torch (the pixel's owner and depth gathered from the view record), torch.nn.functional.grid_sample
(align_corners=False, border padding) and a masked select -- differentiable in the images and the screen vertices like the node.
Forward alone and forward + backward; the two forms alternate; a timed region is --iters calls between two device events;
after warm-up, the median of --regions regions, per call (eager launches, host time included).  Also the node's kernels' own
times (the library's d3m_timing events around each launch, mean of 5; not a rocprofv3 trace).

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


def composed(images, uv_fr, fr, sv, corners, depth_tolerance):
    """(texture [B,T,T,C], mask [B,T,T]) of the composed route, perspective"""
    B, T, S = sv.shape[0], int(uv_fr.image_size), fr.raster_size
    Ft = fr.tri.shape[0]
    p = sv[:, corners]                                                # [B,3F,3]: the unrolled mesh
    attr = torch.stack((p[..., 0] * p[..., 2], p[..., 1] * p[..., 2], p[..., 2]), -1).permute(1, 0, 2).reshape(-1, 3 * B)
    maps, _ = nr.interpolate_vertex_attributes(attr.contiguous(), uv_fr)
    maps = maps[0].flip(1).reshape(B, 3, T, T)
    Z = maps[:, 2]
    x, y = maps[:, 0] / Z, maps[:, 1] / Z
    with torch.no_grad():
        owner = uv_fr.face_index_map[0].long()
        gx, gy = (x * S + S) * 0.5, (y * S + S) * 0.5
        inside = (gx >= 0) & (gx < S) & (gy >= 0) & (gy < S) & (owner >= 0)[None]
        q = gy.clamp(0, S - 1).long() * S + gx.clamp(0, S - 1).long()
        o = fr.face_index_map.view(B, -1).gather(1, q.view(B, -1)).view(B, T, T).long()
        d = fr.depth_map.view(B, -1).gather(1, q.view(B, -1)).view(B, T, T)
        visible = inside & (o >= 0) & ((o % Ft == (owner % Ft)[None]) | (Z <= d + depth_tolerance))
    grid = torch.stack((torch.nan_to_num(x), -torch.nan_to_num(y)), -1)
    tex = torch.nn.functional.grid_sample(images, grid, mode="bilinear", padding_mode="border", align_corners=False)
    return tex.permute(0, 2, 3, 1) * visible[..., None], visible.float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--mesh-n", type=int, default=225)
    ap.add_argument("--image-size", type=int, default=512)
    ap.add_argument("--texture-size", type=int, default=512)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    B, s, T, C, n = args.views, args.image_size, args.texture_size, args.channels, args.mesh_n
    v_np, tri_np = synthetic.grid_mesh(n)
    r = nr.Renderer(image_size=s, anti_aliasing=False, camera_mode="look_at", fill_back=True)
    r.eye = torch.from_numpy(synthetic.camera_ring(B)).float().cuda()
    faces = torch.from_numpy(tri_np).int().cuda()[None]
    v = torch.from_numpy(v_np).float().cuda()[None].repeat(B, 1, 1)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    vertex_uv = np.stack([0.02 + 0.96 * j / (n - 1), 0.02 + 0.96 * i / (n - 1)], -1).reshape(-1, 2).astype(np.float32)
    faces_uv = torch.from_numpy(vertex_uv[tri_np]).cuda().contiguous()
    sv = r._transform(v, None, None, None, None, None).detach().contiguous().requires_grad_(True)
    fr = nr.rasterize_fragments(sv.detach(), faces, s, False, True, r.near, r.far)
    uv_fr = nr.uv_layout_fragments(faces_uv, T)
    gen = torch.Generator().manual_seed(1)
    images = torch.rand(B, C, s, s, generator=gen).cuda().requires_grad_(True)
    g = torch.randn(B, T, T, C, generator=gen).cuda()
    corners = faces[0].reshape(-1).long()
    tol = 1e-2

    forwards = {"node": lambda: nr.bake_uv_texture(images, uv_fr, fr, sv, True, tol),
                "composed": lambda: composed(images, uv_fr, fr, sv, corners, tol)}

    def both(forward):
        def run():
            images.grad = sv.grad = None
            forward()[0].backward(g)
            return images.grad, sv.grad
        return run

    def no_grad(forward):
        def run():
            with torch.no_grad():
                return forward()
        return run

    results = {k: [t.detach().clone() for t in f()] for k, f in forwards.items()}
    # the two routes round differently: a texel-view on a threshold may be decided either way; its output gradient is taken out
    agree = (results["node"][1] == results["composed"][1])
    g = g * agree[..., None]
    grads = {k: [t.clone() for t in both(f)()] for k, f in forwards.items()}
    rel = lambda a, b: float((a - b).abs().max()) / float(b.abs().max())
    diff = dict(mask_disagreements=int((~agree).sum()), texels=int(agree.numel()),
                visible_texel_views=int(results["node"][1].sum()),
                texture=rel(results["node"][0] * agree[..., None], results["composed"][0] * agree[..., None]),
                grad_images=rel(grads["node"][0], grads["composed"][0]), grad_screen_vertices=rel(grads["node"][1], grads["composed"][1]))
    fwd = alternate({k: no_grad(f) for k, f in forwards.items()}, args.regions, args.iters)
    fb = alternate({k: both(f) for k, f in forwards.items()}, args.regions, args.iters)
    _lib.collect_kernel_times()
    _lib.kernel_timing(True)
    for _ in range(5):
        both(forwards["node"])()
    kernels = {k: ms / c for k, (c, ms) in _lib.collect_kernel_times().items()}
    _lib.kernel_timing(False)
    out = {"library_sha256_16": hashlib.sha256(open(LOAD_PATH, "rb").read()).hexdigest()[:16],
           "scene": dict(triangles=int(tri_np.shape[0]), views=B, image_size=s, texture_size=T, channels=C),
           "node_forward_ms": fwd["node"], "composed_forward_ms": fwd["composed"],
           "node_forward_backward_ms": fb["node"], "composed_forward_backward_ms": fb["composed"],
           "composed_over_node_forward": fwd["composed"] / fwd["node"],
           "composed_over_node_forward_backward": fb["composed"] / fb["node"],
           "node_kernel_ms": kernels, "relative_difference_to_composed": diff,
           "timing": f"device events around {args.iters} calls (eager launches, host time included), forms alternating, "
                     f"median of {args.regions} regions after 2 warm-up regions, per call"}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
