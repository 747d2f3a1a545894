#!/usr/bin/env python3
"""Forward plus backward (with respect to the colours) of a per-vertex attribute image beside the existing C = 3 route, at the
benchmark's headline scene: grid_mesh(225) (V = 50,625, F = 100,352), 32 ring cameras, 512x512, anti-aliasing off.
  (a) Renderer.render_rgb(vertices, faces, nr.textures_from_vertex_colors(colors, faces)), ambient 1, directional 0;
  (b) Renderer.render_attributes(vertices, faces, attributes) at C = 3 and at C = 16 (coverage included: the whole call).
The forms alternate within one loop (device events around each eager call after warm-up, at least 50 timed iterations, the
median); the loop is repeated three times and the spread is the largest difference between the repeats' medians.  The
condition: (b) at C = 3 is not slower than (a) beyond that spread.  Writes one JSON object to --out and prints it.  Needs a
GPU."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deep3dmap_amd import neural_renderer as nr, synthetic  # noqa: E402


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vertex_attributes_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_vertex_attributes.py needs a GPU")
    if args.iters < 50:
        sys.exit("at least 50 timed iterations")
    B, s = args.views, args.image_size
    v_np, tri_np = synthetic.grid_mesh(args.mesh_n)
    V = v_np.shape[0]
    vertices = torch.from_numpy(v_np).cuda()[None].repeat(B, 1, 1)
    faces = torch.from_numpy(tri_np).cuda()[None]
    r = nr.Renderer(image_size=s, anti_aliasing=False, camera_mode="look_at", fill_back=True, background_color=[0, 0, 0],
                    light_intensity_ambient=1.0, light_intensity_directional=0.0)
    r.eye = torch.from_numpy(synthetic.camera_ring(B)).float().cuda()
    gen = torch.Generator().manual_seed(0)
    attrs = {C: torch.rand(V, C, generator=gen).cuda().requires_grad_(True) for C in (3, 16)}
    grads = {C: torch.randn(B, C, s, s, generator=gen).cuda() for C in (3, 16)}

    def cube_route():
        a = attrs[3]
        a.grad = None
        r.render_rgb(vertices, faces, nr.textures_from_vertex_colors(a, faces)).backward(grads[3])

    def attribute_route(C):
        def run():
            a = attrs[C]
            a.grad = None
            r.render_attributes(vertices, faces, a)[0].backward(grads[C])
        return run

    forms = {"cube_route_c3": cube_route, "attributes_c3": attribute_route(3), "attributes_c16": attribute_route(16)}
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
    # the two C = 3 routes draw the same picture
    with torch.no_grad():
        a = r.render_rgb(vertices, faces, nr.textures_from_vertex_colors(attrs[3], faces))
        b = r.render_attributes(vertices, faces, attrs[3])[0]
    allowed = max(spread["cube_route_c3"], spread["attributes_c3"])
    out = {"scene": {"mesh_n": args.mesh_n, "vertices": V, "faces": int(tri_np.shape[0]), "views": B, "image_size": s,
                     "anti_aliasing": False},
           "timing": "forward + backward wrt the colours, eager calls, device events, forms alternating, median of "
                     f"{args.iters} after {args.warmup} warm-up, {args.repeats} repeats",
           "median_ms": med, "repeat_medians_ms": repeats, "spread_ms": spread,
           "attributes_c3_minus_cube_route_ms": med["attributes_c3"] - med["cube_route_c3"],
           "condition_attributes_c3_not_slower_beyond_spread": bool(med["attributes_c3"] <= med["cube_route_c3"] + allowed),
           "largest_difference_of_the_c3_images": float((a - b).abs().max())}
    line = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)
    if not out["condition_attributes_c3_not_slower_beyond_spread"]:
        sys.exit("attributes at C = 3 are slower than the texture-cube route beyond the measured spread")


if __name__ == "__main__":
    main()
