#!/usr/bin/env python3
"""Forward, and forward plus backward, of nr.shade_uv_texture beside the composed route it replaces, with gradients to the
albedo image, the normals and the light, at the benchmark's headline scene: grid_mesh(225) (V = 50,625, F = 100,352), 32 ring
cameras, 512x512, anti-aliasing off (the one setting at which the two routes draw the same picture), a shared T x T albedo
(T = 512) with a seamless per-vertex uv layout, over ONE coverage record made beforehand (coverage is not timed: both routes
read the same record).
  (a) node      nr.shade_uv_texture(image, faces_uv, normals, sh, fragments)
  (b) composed  nr.shade_fragments(normals, sh, fragments, background=1.0)[0] * nr.sample_uv_texture(image, faces_uv, fragments)[0]
The forms alternate within one loop (device events around each eager call after warm-up, at least 20 timed iterations, the
median); the loop is repeated three times and the spread is the largest difference between the repeats' medians.  Reported, not
gated: the reason for the node is the supersampled record, where (b) is not the same function.  The launch counts and
per-kernel milliseconds are the library's kernels (d3m_timing_collect: events around every launch, so the step is slower
while they are collected) of one forward plus backward; torch's own multiply of (b) and its backward are not among them.
Writes one JSON object to --out and prints it.  Needs a GPU."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deep3dmap_amd import _lib, neural_renderer as nr, synthetic  # noqa: E402


def timed_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def median(xs):
    return sorted(xs)[len(xs) // 2]


def library_launches(fn):
    _lib.collect_kernel_times()
    _lib.kernel_timing(True)
    try:
        fn()
        torch.cuda.synchronize()
        return {k: {"launches": v[0], "ms": round(v[1], 4)} for k, v in _lib.collect_kernel_times().items()}
    finally:
        _lib.kernel_timing(False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--mesh-n", type=int, default=225)
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--image-size", type=int, default=512)
    ap.add_argument("--texture-size", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shade_uv_texture_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_shade_uv_texture.py needs a GPU")
    if args.iters < 20:
        sys.exit("at least 20 timed iterations")
    B, s, T = args.views, args.image_size, args.texture_size
    v_np, tri_np = synthetic.grid_mesh(args.mesh_n)
    V = v_np.shape[0]
    vertices = torch.from_numpy(v_np).cuda()[None].repeat(B, 1, 1)
    faces = torch.from_numpy(tri_np).cuda()[None]
    r = nr.Renderer(image_size=s, anti_aliasing=False, camera_mode="look_at", fill_back=True)
    r.eye = torch.from_numpy(synthetic.camera_ring(B)).float().cuda()
    fr = r.fragments(vertices, faces)
    gen = torch.Generator().manual_seed(0)
    xy = vertices[0, :, :2]
    vertex_uv = (xy - xy.min(0).values) / (xy.max(0).values - xy.min(0).values)
    faces_uv = vertex_uv[faces[0].long()].contiguous()
    with torch.no_grad():
        normals = nr.vertex_normals(vertices[0], faces).clone().requires_grad_(True)
    image = (0.5 + 0.5 * torch.rand(T, T, 3, generator=gen)).cuda().requires_grad_(True)
    sh = nr.SHLight().sh.detach().clone()
    sh[:, 1:] = 0.3 * torch.randn(3, 8, generator=gen)
    sh = sh.cuda().requires_grad_(True)
    g = torch.randn(B, 3, s, s, generator=gen).cuda()
    leaves = (image, normals, sh)

    def node_image():
        return nr.shade_uv_texture(image, faces_uv, normals, sh, fr)[0]

    def composed_image():
        return nr.shade_fragments(normals, sh, fr, background=1.0)[0] * nr.sample_uv_texture(image, faces_uv, fr)[0]

    def forward(image_of):
        def run():
            with torch.no_grad():
                image_of()
        return run

    def step(image_of):
        def run():
            for t in leaves:
                t.grad = None
            image_of().backward(g)
        return run

    forms = {"node_forward": forward(node_image), "composed_forward": forward(composed_image),
             "node_step": step(node_image), "composed_step": step(composed_image)}
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
    launches = {name: library_launches(forms[name]) for name in ("node_step", "composed_step")}
    # without supersampling the two routes draw the same picture on covered pixels and give the same gradients, up to
    # float32 rounding
    results = {}
    for name in ("node_step", "composed_step"):
        forms[name]()
        results[name] = [t.grad.clone() for t in leaves]
    with torch.no_grad():
        a, b = node_image(), composed_image()
    differences = {"image": float((a - b).abs().max() / b.abs().max())}
    for key, x, y in zip(("albedo", "normals", "sh"), results["node_step"], results["composed_step"]):
        differences[key] = float((x - y).abs().max() / y.abs().max())
    out = {"scene": {"mesh_n": args.mesh_n, "vertices": V, "faces": int(tri_np.shape[0]), "views": B, "image_size": s,
                     "texture_size": T, "anti_aliasing": False},
           "timing": "forward (no_grad) and forward + backward wrt albedo image, normals and light over one record, eager "
                     f"calls, device events, forms alternating, median of {args.iters} after {args.warmup} warm-up, "
                     f"{args.repeats} repeats",
           "median_ms": med, "repeat_medians_ms": repeats, "spread_ms": spread,
           "library_launches": launches, "library_launches_total": {k: sum(x["launches"] for x in v.values()) for k, v in launches.items()},
           "node_not_slower_than_composed": {"forward": bool(med["node_forward"] <= med["composed_forward"]),
                                             "step": bool(med["node_step"] <= med["composed_step"])},
           "largest_difference_over_largest_entry": differences}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
