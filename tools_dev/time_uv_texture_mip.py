#!/usr/bin/env python3
"""Forward plus backward (with respect to the image) of a mip-mapped per-pixel uv texture image beside the bilinear node at
the benchmark's headline scene: grid_mesh(225) (V = 50,625, F = 100,352), 32 ring cameras, 512x512, anti-aliasing off, a
shared RGB texture of 2048 x 2048 -- minification, the case mip-mapping is for.  Both forms are the whole call, coverage
included, and alternate within one loop (device events around each eager call after warm-up, at least 50 timed iterations,
the median); the loop is repeated three times and the spread is the largest difference between the repeats' medians.  Per
kernel of the mip-mapped node: the mean time over the timed iterations of a separate pass (the library's launch timer), and
for the scatter the atomic bytes per second it achieved -- 8 bytes per (covered pixel, tap, channel), eight taps: an upper
figure, taps of weight 0 are skipped.  The levels of detail met are recorded with them.  Nothing is judged: the figures are
recorded.  Writes one JSON object to --out and prints it.  Needs a GPU."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deep3dmap_amd import _lib, neural_renderer as nr, synthetic  # noqa: E402

KERNELS = ("k_texture_mip_tile", "k_texture_mip_tail", "k_uv_texture_mip_images", "k_uv_texture_images_clear_max",
           "k_uv_texture_mip_images_scatter", "k_uv_texture_mip_images_convert")
BILINEAR_KERNELS = ("k_uv_texture_images", "k_uv_texture_images_clear_max", "k_uv_texture_images_scatter",
                    "k_uv_texture_images_convert")


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
    ap.add_argument("--texture-size", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uv_texture_mip_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_uv_texture_mip.py needs a GPU")
    if args.iters < 50:
        sys.exit("at least 50 timed iterations")
    B, s, n, size = args.views, args.image_size, args.mesh_n, args.texture_size
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
    image = torch.rand(size, size, 3, generator=gen).cuda().requires_grad_(True)
    grad = torch.randn(B, 3, s, s, generator=gen).cuda()
    levels = nr.uv_texture_images.mip_levels(size, size, True)

    def route(mipmap):
        def run():
            image.grad = None
            r.render_uv_texture(vertices, faces, image, faces_uv, "CLAMP_TO_EDGE", mipmap=mipmap)[0].backward(grad)
        return run

    forms = {"mip": route(True), "bilinear": route(None)}
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
    cov = fr.face_index_map >= 0
    covered = int(cov.sum())
    lod = nr.uv_texture_lod(faces_uv, fr, (size, size), "CLAMP_TO_EDGE", 0.0, levels)[cov]
    kernels = {}
    for name, mipmap, names, taps in (("mip", True, KERNELS, 8), ("bilinear", None, BILINEAR_KERNELS, 4)):
        _lib.collect_kernel_times()
        _lib.kernel_timing(True)
        for _ in range(args.iters):
            image.grad = None
            nr.sample_uv_texture(image, faces_uv, fr, "CLAMP_TO_EDGE", mipmap=mipmap)[0].backward(grad)
        got = _lib.collect_kernel_times()
        _lib.kernel_timing(False)
        per = {k: got[k][1] / got[k][0] * 1e3 for k in names if k in got}
        scatter = [k for k in names if k.endswith("_scatter")][0]
        atomic_bytes = covered * taps * 3 * 8
        kernels[name] = {"mean_us": per, "scatter_atomic_bytes_upper": atomic_bytes,
                         "scatter_atomic_bytes_per_s_upper": atomic_bytes / (per[scatter] * 1e-6)}
    out = {"scene": {"mesh_n": n, "vertices": V, "faces": int(tri_np.shape[0]), "views": B, "image_size": s,
                     "anti_aliasing": False, "covered_pixels": covered, "channels": 3, "wrapping": "CLAMP_TO_EDGE",
                     "texture_size": size, "levels": levels,
                     "lod": {"min": float(lod.min()), "median": float(lod.median()), "max": float(lod.max())}},
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
