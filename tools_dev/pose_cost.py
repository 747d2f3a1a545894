#!/usr/bin/env python3
"""Cost of the weak-perspective pose node (neural_renderer/pose.py) at Basel size.

nr.pose_vertices beside the same arithmetic in eager torch -- the restatement of deep3dmap/models/frameworks/imgs2mesh.py
:111-118 and :194-197 that a caller must write without the node (clamp, six trig calls, three matrix stacks, two 3x3
products, a batched matmul, permutes, slices, the y flip, an index for the landmarks) -- on the same hashed inputs, at
V = 53,215 for B in {1, 3, 16}, in two configurations: `posed` (the posed points alone) and `full` (posed points, uv at the
reference's image size, and 68 landmarks).  Forward alone and forward + backward (a gradient arrives at every output,
vertices and pose both require grad).  The two forms alternate; a timed region is --iters calls between two device events;
after warm-up, the median of --regions regions, per call (eager launches, host time included).  Also the kernels' own times
(the library's d3m_timing events around each launch, mean of 5; not a rocprofv3 trace) and the byte floor of the node at
8 TB/s: forward reads 12 V B bytes and writes 12 V B (+ 8 V B for uv); backward reads the vertices and the gradients and
writes the vertex gradient.

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
from deep3dmap_amd import _lib, neural_renderer as nr  # noqa: E402
from deep3dmap_amd.build import LOAD_PATH  # noqa: E402
from deep3dmap_amd.core.renderer_pt3d import euler_xyz_to_matrix  # noqa: E402

HBM_BYTES_PER_S = 8e12
V_BASEL, IMAGE_SIZE, LIMIT = 53215, 224.0, 3.1415


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


def eager_pose(points, pose, full, lm_idx):
    """the operations of imgs2mesh.py:111-118 and :194-197 in eager torch: clamp, Euler matrix, a batched matmul on the
    transposed points, scale, translation, transpose back, slice, divide, flip y, gather"""
    rot = euler_xyz_to_matrix(pose[:, 1:4].clamp(-LIMIT, LIMIT))
    turned = torch.matmul(rot, points.transpose(1, 2))
    posed = (pose[:, 0].view(-1, 1, 1) * turned + IMAGE_SIZE * pose[:, 4:7].view(-1, 3, 1)).transpose(1, 2)
    if not full:
        return (posed,)
    xy = posed[:, :, :2] / IMAGE_SIZE
    return posed, torch.stack([xy[:, :, 0], 1 - xy[:, :, 1]], 2), posed[:, lm_idx]


def case(B, full, regions, iters):
    V = V_BASEL
    points = torch.from_numpy(hashed(B * V, 3, 1, -100.0, 100.0)).view(B, V, 3).cuda().requires_grad_(True)
    pose_np = hashed(B, 7, 2, -1.0, 1.0)
    pose_np[:, 0] += 1.5
    pose = torch.from_numpy(pose_np).cuda().requires_grad_(True)
    lm_idx = torch.from_numpy((np.arange(68, dtype=np.int64) * 7919 + 13) % V).cuda()
    grads = [torch.from_numpy(hashed(B * V, 3, 3)).view(B, V, 3).cuda()]
    if full:
        grads += [torch.from_numpy(hashed(B * V, 2, 4)).view(B, V, 2).cuda(), torch.from_numpy(hashed(B * 68, 3, 5)).view(B, 68, 3).cuda()]

    def node_forward():
        out = nr.pose_vertices(points, pose, IMAGE_SIZE, LIMIT, IMAGE_SIZE if full else None, lm_idx if full else None)
        return [t for t in out if t is not None]

    def eager_forward():
        return list(eager_pose(points, pose, full, lm_idx))

    def both(forward):
        def run():
            points.grad = pose.grad = None
            torch.autograd.backward(forward(), grads)
            return points.grad, pose.grad
        return run

    gn = [g.clone() for g in both(node_forward)()]
    ge = [g.clone() for g in both(eager_forward)()]
    with torch.no_grad():
        fn, fe = node_forward(), eager_forward()
    diff = dict(outputs=max(float((a - b).abs().max()) / float(b.abs().max()) for a, b in zip(fn, fe)),
                grad_vertices=float((gn[0] - ge[0]).abs().max()) / float(ge[0].abs().max()),
                grad_pose=float((gn[1] - ge[1]).abs().max()) / float(ge[1].abs().max()))

    def no_grad(f):
        def run():
            with torch.no_grad():
                return f()
        return run

    fwd = alternate({"node": no_grad(node_forward), "eager": no_grad(eager_forward)}, regions, iters)
    fb = alternate({"node": both(node_forward), "eager": both(eager_forward)}, regions, iters)
    _lib.collect_kernel_times()
    _lib.kernel_timing(True)
    for _ in range(5):
        both(node_forward)()
    kernels = {k: ms / c for k, (c, ms) in _lib.collect_kernel_times().items()}
    _lib.kernel_timing(False)
    out_bytes = 12 * V * B + ((8 * V * B + 12 * 68 * B) if full else 0)
    floor_f = (12 * V * B + out_bytes) / HBM_BYTES_PER_S * 1e3
    floor_b = (12 * V * B + out_bytes + 12 * V * B) / HBM_BYTES_PER_S * 1e3
    return dict(V=V, B=B, outputs="full" if full else "posed", node_forward_ms=fwd["node"], eager_forward_ms=fwd["eager"],
                node_forward_backward_ms=fb["node"], eager_forward_backward_ms=fb["eager"],
                eager_over_node_forward=fwd["eager"] / fwd["node"], eager_over_node_forward_backward=fb["eager"] / fb["node"],
                kernel_ms=kernels, byte_floor_forward_ms=floor_f, byte_floor_backward_ms=floor_b,
                relative_difference_to_eager=diff)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    out = {"library_sha256_16": hashlib.sha256(open(LOAD_PATH, "rb").read()).hexdigest()[:16],
           "cases": [case(B, full, args.regions, args.iters) for B in (1, 3, 16) for full in (False, True)],
           "timing": f"device events around {args.iters} calls (eager launches, host time included), forms alternating, "
                     f"median of {args.regions} regions after 2 warm-up regions, per call"}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
