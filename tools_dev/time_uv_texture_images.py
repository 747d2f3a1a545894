#!/usr/bin/env python3
"""Forward plus backward (with respect to the image) of a per-pixel uv texture image at the benchmark's headline scene:
grid_mesh(225) (V = 50,625, F = 100,352), 32 ring cameras, 512x512, anti-aliasing off, a shared RGB texture of
  (a) 64 x 64     (magnification: many lanes of a wave add to the same texel), and
  (b) 1024 x 1024,
beside Renderer.render_attributes at C = 3 (forward plus backward with respect to the attributes), the yardstick, in the
same loop.  Every form is the whole call, coverage included.  The forms alternate within one loop (device events around each
eager call after warm-up, at least 50 timed iterations, the median); the loop is repeated three times and the spread is the
largest difference between the repeats' medians.  Per kernel of the node: the mean time over the timed iterations of a
separate pass (the library's launch timer), and for the scatter the atomic bytes per second it achieved -- 8 bytes per
(covered pixel, tap of non-zero weight, channel): the rate of 64-bit integer atomic adds, which nobody had measured.  Nothing
is judged: the figures are recorded.  Writes one JSON object to --out and prints it.  Needs a GPU."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deep3dmap_amd import _lib, neural_renderer as nr, synthetic  # noqa: E402

KERNELS = ("k_uv_texture_images", "k_uv_texture_images_clear_max", "k_uv_texture_images_scatter", "k_uv_texture_images_convert")


def timed_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--mesh-n", type=int, default=225)
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--image-size", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uv_texture_images_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_uv_texture_images.py needs a GPU")
    if args.iters < 50:
        sys.exit("at least 50 timed iterations")
    B, s, n = args.views, args.image_size, args.mesh_n
    v_np, tri_np = synthetic.grid_mesh(n)
    V = v_np.shape[0]
    vertices = torch.from_numpy(v_np).cuda()[None].repeat(B, 1, 1)
    faces = torch.from_numpy(tri_np).cuda()[None]
    r = nr.Renderer(image_size=s, anti_aliasing=False, camera_mode="look_at", fill_back=True, background_color=[0, 0, 0])
    r.eye = torch.from_numpy(synthetic.camera_ring(B)).float().cuda()
    # the grid's own layout as the uv: vertex (i, j) at (j, i) / (n - 1)
    i, j = torch.meshgrid(torch.arange(n), torch.arange(n), indexing="ij")
    uv = (torch.stack([j, i], -1).reshape(V, 2).float() / (n - 1)).cuda()
    faces_uv = uv[faces[0].long()].contiguous()
    gen = torch.Generator().manual_seed(0)
    images = {size: torch.rand(size, size, 3, generator=gen).cuda().requires_grad_(True) for size in (64, 1024)}
    attributes = torch.rand(V, 3, generator=gen).cuda().requires_grad_(True)
    grad = torch.randn(B, 3, s, s, generator=gen).cuda()

    def texture_route(size):
        def run():
            a = images[size]
            a.grad = None
            r.render_uv_texture(vertices, faces, a, faces_uv, "CLAMP_TO_EDGE")[0].backward(grad)
        return run

    def attribute_route():
        attributes.grad = None
        r.render_attributes(vertices, faces, attributes)[0].backward(grad)

    forms = {"uv_texture_64": texture_route(64), "uv_texture_1024": texture_route(1024), "attributes_c3": attribute_route}
    repeats = []
    for _ in range(args.repeats):
        times = {name: [] for name in forms}
        for it in range(args.warmup + args.iters):
            for name, fn in forms.items():
                torch.cuda.synchronize()
                t = timed_ms(fn)
                if it >= args.warmup:
                    times[name].append(t)
        repeats.append({name: median(x) for name, x in times.items()})
    med = {name: median([rep[name] for rep in repeats]) for name in forms}
    spread = {name: max(rep[name] for rep in repeats) - min(rep[name] for rep in repeats) for name in forms}
    # per kernel, and the scatter's atomic rate
    fr = r.fragments(vertices, faces)
    covered = int((fr.face_index_map >= 0).sum())
    kernels = {}
    for size in (64, 1024):
        _lib.collect_kernel_times()
        _lib.kernel_timing(True)
        for _ in range(args.iters):
            a = images[size]
            a.grad = None
            nr.sample_uv_texture(a, faces_uv, fr, "CLAMP_TO_EDGE")[0].backward(grad)
        got = _lib.collect_kernel_times()
        _lib.kernel_timing(False)
        per = {k: got[k][1] / got[k][0] * 1e3 for k in KERNELS}
        atomic_bytes = covered * 4 * 3 * 8
        kernels[f"uv_texture_{size}"] = {
            "mean_us": per, "scatter_atomic_bytes_upper": atomic_bytes,
            "scatter_atomic_bytes_per_s_upper": atomic_bytes / (per["k_uv_texture_images_scatter"] * 1e-6)}
    out = {"scene": {"mesh_n": n, "vertices": V, "faces": int(tri_np.shape[0]), "views": B, "image_size": s,
                     "anti_aliasing": False, "covered_pixels": covered, "channels": 3, "wrapping": "CLAMP_TO_EDGE"},
           "timing": "forward + backward, eager calls with coverage, device events, forms alternating, median of "
                     f"{args.iters} after {args.warmup} warm-up, {args.repeats} repeats; kernels: the library's launch timer, "
                     f"mean of {args.iters} calls over one coverage record; atomic bytes: 8 per (covered pixel, tap, channel), "
                     "an upper figure (taps of weight 0 are skipped)",
           "median_ms": med, "repeat_medians_ms": repeats, "spread_ms": spread, "kernels": kernels}
    line = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
