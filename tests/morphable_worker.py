"""One rank of a small camera-sharded fit of a morphable model's coefficients, run as a child process by
tests/test_gpu_morphable.py: grid_mesh(9), 4 cameras at 64x64 shared among the ranks, K = 7 hashed basis, the captured step.
Every rank uses cuda:0 and the collective runs over gloo.  Writes what the rank holds after the exchange -- the loss and the
gradients of the objective over ALL cameras, the shape gradient as [K] -- to --out.  Exit code != 0 on any failure."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def fit_scene():
    """(vertices, triangles, cubes, eyes, basis [3V,7], scale [7], c0 [7]) of the morphable fit tests, from the hash"""
    import numpy as np
    import morphable_scenes as ms
    from deep3dmap_amd import synthetic
    v, tri = synthetic.grid_mesh(9)
    K = 7
    basis = ms.hashed_floats(v.size, K, 31, -0.04, 0.04)
    scale = ms.hashed_floats(1, K, 32, 0.5, 1.5)[0]
    c0 = ms.hashed_floats(1, K, 33, -1.0, 1.0)[0]
    cubes = ms.hashed_floats(tri.shape[0], 24, 34, 0.0, 1.0).reshape(-1, 2, 2, 2, 3)
    return v.astype(np.float32), tri, cubes, synthetic.camera_ring(4), basis, scale, c0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    import numpy as np
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    torch.cuda.set_device(0)
    if world > 1:
        dist.init_process_group(backend="gloo")
    from deep3dmap_amd import neural_renderer as nr, synthetic
    from deep3dmap_amd.multiview import MultiViewFit
    v, tri, cubes, eyes, basis, scale, c0 = fit_scene()
    model = nr.MorphableModel(v.reshape(-1), basis, scale)
    fit = MultiViewFit(None, tri, cubes, eyes, image_size=64, rank=rank, world_size=world, morphable=model, coeffs=c0,
                       regularizer=dict(laplacian=0.5))
    assert not fit.split_exchange
    fit.set_targets_from(synthetic.perturb(v))
    loss, gc, gt = fit.step()
    eager = (float(loss), gc.clone(), gt.clone())
    fit.capture_graph()
    assert fit.graph_captured
    for i in range(2):
        loss, gc, gt = fit.step()
        torch.cuda.synchronize()
        assert abs(float(loss) - eager[0]) <= 1e-5 * abs(eager[0]), (i, float(loss), eager[0])
        for got, want in ((gc, eager[1]), (gt, eager[2])):
            assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max()), i
    np.savez(args.out + f".rank{rank}.npz", loss=float(loss), gc=gc.cpu().numpy(), gt=gt.cpu().numpy(),
             flat_numel=fit._flat.numel())
    print(f"rank {rank}/{world}: loss {float(loss):.7f} ok", flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
