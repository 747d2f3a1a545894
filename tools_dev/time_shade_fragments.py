#!/usr/bin/env python3
"""Forward plus backward of nr.shade_fragments beside the composed route it replaces, with gradients to the normals, the
colours and the light, at the benchmark's headline scene: grid_mesh(225) (V = 50,625, F = 100,352), 32 ring cameras, 512x512,
anti-aliasing off, over ONE coverage record made beforehand (coverage is not timed: both routes read the same record).
  (a) fused     nr.shade_fragments(normals, sh, fragments, colors)
  (b) composed  nr.interpolate_vertex_attributes of the normals, torch's normalisation, nr.sh_basis, the contraction with sh,
                times nr.interpolate_vertex_attributes of the colours, times alpha
The forms alternate within one loop (device events around each eager call after warm-up, at least 20 timed iterations, the
median); the loop is repeated three times and the spread is the largest difference between the repeats' medians.  The
condition: (a) is not slower than (b).  The launch counts are the library's kernels (d3m_timing_collect) of one step; torch's
own element-wise and reduction kernels of (b) are not among them.  Writes one JSON object to --out and prints it.  Needs a GPU."""
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
        return {k: v[0] for k, v in _lib.collect_kernel_times().items()}
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shade_fragments_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_shade_fragments.py needs a GPU")
    if args.iters < 20:
        sys.exit("at least 20 timed iterations")
    B, s = args.views, args.image_size
    v_np, tri_np = synthetic.grid_mesh(args.mesh_n)
    V = v_np.shape[0]
    vertices = torch.from_numpy(v_np).cuda()[None].repeat(B, 1, 1)
    faces = torch.from_numpy(tri_np).cuda()[None]
    r = nr.Renderer(image_size=s, anti_aliasing=False, camera_mode="look_at", fill_back=True)
    r.eye = torch.from_numpy(synthetic.camera_ring(B)).float().cuda()
    fr = r.fragments(vertices, faces)
    gen = torch.Generator().manual_seed(0)
    with torch.no_grad():
        normals = nr.vertex_normals(vertices[0], faces).clone().requires_grad_(True)
    colors = (0.5 + 0.5 * torch.rand(V, 3, generator=gen)).cuda().requires_grad_(True)
    sh = nr.SHLight().sh.detach().clone()
    sh[:, 1:] = 0.3 * torch.randn(3, 8, generator=gen)
    sh = sh.cuda().requires_grad_(True)
    g = torch.randn(B, 3, s, s, generator=gen).cuda()
    leaves = (normals, colors, sh)

    def fused_image():
        return nr.shade_fragments(normals, sh, fr, colors)[0]

    def composed_image():
        m, alpha = nr.interpolate_vertex_attributes(normals, fr)
        m = m.permute(0, 2, 3, 1)
        length = torch.sqrt((m[..., 0] * m[..., 0] + m[..., 1] * m[..., 1]) + m[..., 2] * m[..., 2])
        H = nr.sh_basis(m / length.clamp(min=1e-6)[..., None])
        shade = torch.einsum("kj,byxj->bkyx", sh, H)
        return shade * nr.interpolate_vertex_attributes(colors, fr)[0] * alpha[:, None]

    def step(image):
        def run():
            for t in leaves:
                t.grad = None
            image().backward(g)
        return run

    forms = {"fused": step(fused_image), "composed": step(composed_image)}
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
    launches = {name: library_launches(fn) for name, fn in forms.items()}
    # the two routes draw the same picture and give the same gradients, up to float32 rounding
    results = {}
    for name, fn in forms.items():
        fn()
        results[name] = [t.grad.clone() for t in leaves]
    with torch.no_grad():
        a, b = fused_image(), composed_image()
    differences = {"image": float((a - b).abs().max() / b.abs().max())}
    for key, x, y in zip(("normals", "colors", "sh"), results["fused"], results["composed"]):
        differences[key] = float((x - y).abs().max() / y.abs().max())
    out = {"scene": {"mesh_n": args.mesh_n, "vertices": V, "faces": int(tri_np.shape[0]), "views": B, "image_size": s,
                     "anti_aliasing": False},
           "timing": "forward + backward wrt normals, colours and light over one record, eager calls, device events, forms "
                     f"alternating, median of {args.iters} after {args.warmup} warm-up, {args.repeats} repeats",
           "median_ms": med, "repeat_medians_ms": repeats, "spread_ms": spread,
           "library_launches": launches, "library_launches_total": {k: sum(v.values()) for k, v in launches.items()},
           "condition_fused_not_slower_than_composed": bool(med["fused"] <= med["composed"]),
           "largest_difference_over_largest_entry": differences}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)
    if not out["condition_fused_not_slower_than_composed"]:
        sys.exit("the fused node is slower than the composed route")


if __name__ == "__main__":
    main()
