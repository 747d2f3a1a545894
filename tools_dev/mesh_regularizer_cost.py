#!/usr/bin/env python3
"""Cost of the mesh shape regularisers (neural_renderer/mesh_regularizers.py) at the benchmark's mesh, grid_mesh(225)
(V = 50,625, F = 100,352): (a) value + gradient of the three terms by nr.mesh_regularizer beside the same three terms
composed from eager torch operators on the device (index_add_, cross, norm: what a caller runs without the node) -- the two
forms alternate in one call, device events around synchronised work, after warm-up, medians of --reps --, the launches of
each form's value + gradient, and the one-time topology build; (b) a MultiViewFit step (32 views, 512x512, one rank,
captured) with and without regularizer=, alternating, median of --steps.  Writes one JSON object to --out and prints it."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deep3dmap_amd import _lib, neural_renderer as nr, synthetic  # noqa: E402
from deep3dmap_amd.build import LOAD_PATH  # noqa: E402
from deep3dmap_amd.multiview import MultiViewFit  # noqa: E402
from deep3dmap_amd.neural_renderer import mesh_regularizers  # noqa: E402

WEIGHTS = dict(laplacian=0.5, edge=1.0, edge_target=0.01, normal=0.2)


def timed_ms(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def median(xs):
    return sorted(xs)[len(xs) // 2]


def eager_terms(x, edges, wings, V):
    """the composition a caller writes without the node, on the device"""
    a, b = edges[:, 0], edges[:, 1]
    deg = torch.zeros(V, device=x.device).index_add_(0, a, torch.ones_like(a, dtype=x.dtype)).index_add_(
        0, b, torch.ones_like(b, dtype=x.dtype))
    total = torch.zeros_like(x).index_add_(0, a, x[b]).index_add_(0, b, x[a])
    delta = torch.where((deg > 0)[:, None], x - total / deg.clamp(min=1)[:, None], torch.zeros_like(x))
    lap = (delta ** 2).sum() / V
    edge = (((x[a] - x[b]).norm(dim=-1) - WEIGHTS["edge_target"]) ** 2).mean()
    xa = x[wings[:, 0]]
    e = x[wings[:, 1]] - xa
    n0 = torch.cross(e, x[wings[:, 2]] - xa, dim=-1)
    n1 = -torch.cross(e, x[wings[:, 3]] - xa, dim=-1)
    cos = (n0 * n1).sum(-1) / (n0.norm(dim=-1) * n1.norm(dim=-1))
    return WEIGHTS["laplacian"] * lap + WEIGHTS["edge"] * edge + WEIGHTS["normal"] * (1 - cos).mean()


def kernels(reps, n=225):
    v, tri = synthetic.grid_mesh(n)
    v = synthetic.perturb(v)                                 # (no flat pair: the eager form has no zero-normal guard)
    V, F = v.shape[0], tri.shape[0]
    faces = torch.from_numpy(tri).cuda()
    x = torch.as_tensor(v, dtype=torch.float32).cuda().requires_grad_(True)
    builds = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        T = mesh_regularizers.build_topology(faces, V)
        torch.cuda.synchronize()
        builds.append((time.perf_counter() - t0) * 1e3)
    edges, wings = T.edges.long(), T.wings.long()

    def both(loss_fn):
        x.grad = None
        loss = loss_fn()
        loss.backward()
        return loss.detach(), x.grad

    forms = {"hip": lambda: both(lambda: nr.mesh_regularizer(x, faces, **WEIGHTS)),
             "eager": lambda: both(lambda: eager_terms(x, edges, wings, V))}
    times = {name: [] for name in forms}
    for rep in range(reps + 3):
        for name, fn in forms.items():
            t, _ = timed_ms(fn)
            if rep >= 3:                                    # (the first three rounds warm up)
                times[name].append(t)
    res = {f"{name}_value_and_gradient_ms": median(t) for name, t in times.items()}
    (l_h, g_h), (l_e, g_e) = forms["hip"](), forms["eager"]()
    g_h, g_e = g_h.clone(), g_e.clone()
    _lib.collect_kernel_times()
    _lib.kernel_timing(True)
    forms["hip"]()
    launched = {k: c for k, (c, _) in _lib.collect_kernel_times().items()}
    _lib.kernel_timing(False)
    try:                                                    # (the profiler's device rows: one per kernel name)
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            forms["eager"]()
            torch.cuda.synchronize()
        eager_launches = sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)
    except Exception as exc:                                # noqa: BLE001 -- a count that cannot be taken is reported as such
        eager_launches = f"not counted: {exc!r}"
    res.update(vertices=V, faces=F, edges=T.num_edges, wing_records=T.num_wings, topology_build_ms=median(builds),
               hip_launches_forward_and_backward=launched, hip_launches=sum(launched.values()),
               eager_device_launches=eager_launches,
               value_relative_difference=abs(float(l_h) - float(l_e)) / abs(float(l_e)),
               gradient_relative_difference=float((g_h - g_e).abs().max()) / float(g_e.abs().max()),
               timing="events around each call (eager launch, host time included), forms alternating, median")
    return res


def fit_steps(steps, B=32, s=512, n=225):
    v, tri = synthetic.grid_mesh(n)
    cubes = np.random.default_rng(1).random((tri.shape[0], 2, 2, 2, 3), dtype=np.float32)
    eyes = synthetic.camera_ring(B)
    fits = {"regularized": MultiViewFit(v, tri, cubes, eyes, image_size=s, regularizer=WEIGHTS),
            "plain": MultiViewFit(v, tri, cubes, eyes, image_size=s)}
    out = {"views": B, "image_size": s, "faces": int(tri.shape[0]), "vertices": int(v.shape[0])}
    for name, fit in fits.items():
        fit.set_targets_from(synthetic.perturb(v))
        fit.step()
        fit.capture_graph()
        out[name + "_exchange_bytes_per_step"] = 4 * fit._flat.numel()
    times = {name: [] for name in fits}
    for rep in range(steps + 3):
        for name, fit in fits.items():
            t, _ = timed_ms(fit.step)
            if rep >= 3:
                times[name].append(t)
    for name in fits:
        out[name + "_step_ms"] = median(times[name])
    out["added_ms"] = out["regularized_step_ms"] - out["plain_step_ms"]
    out["multi_gpu"] = "from shapes only: rank 0 runs the extra passes, no exchange bytes are added; unmeasured on hardware"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_regularizer_cost.json"))
    args = ap.parse_args()
    out = {"library_sha256_16": hashlib.sha256(open(LOAD_PATH, "rb").read()).hexdigest()[:16],
           "kernels": kernels(args.reps), "fit_step": fit_steps(args.steps)}
    line = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
