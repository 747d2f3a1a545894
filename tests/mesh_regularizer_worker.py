"""One rank of a small camera-sharded fit with a shape regulariser, run as a child process by
tests/test_gpu_mesh_regularizers.py: icosphere(1), 4 cameras at 64x64 shared among the ranks, the eager and the captured
step.  Every rank uses cuda:0 and the collective runs over gloo.  Writes what the rank holds after the exchange -- the loss
and the vertex gradient of the objective over ALL cameras plus the prior, once -- and whether this rank launched the
regulariser's kernels (rank 0 alone does) to --out.  Exit code != 0 on any failure."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    from deep3dmap_amd import _lib, synthetic
    from deep3dmap_amd.multiview import MultiViewFit
    v, tri = synthetic.icosphere(1)
    textures = np.random.default_rng(3).random((tri.shape[0], 2, 2, 2, 3), dtype=np.float32)
    fit = MultiViewFit(v, tri, textures, synthetic.camera_ring(4), image_size=64, rank=rank, world_size=world,
                       regularizer=dict(laplacian=0.5, edge=1.0, edge_target=0.3, normal=0.2))
    fit.set_targets_from(synthetic.perturb(v))
    _lib.collect_kernel_times()
    _lib.kernel_timing(True)
    loss, gv, gt = fit.step()
    torch.cuda.synchronize()
    launched = any(name.startswith("k_mesh_reg") for name in _lib.collect_kernel_times())
    _lib.kernel_timing(False)
    assert launched == (rank == 0), (rank, launched)
    eager = (float(loss), gv.clone(), gt.clone())
    fit.capture_graph()
    assert fit.graph_captured
    for i in range(2):
        loss, gv, gt = fit.step()
        torch.cuda.synchronize()
        assert abs(float(loss) - eager[0]) <= 1e-5 * abs(eager[0]), (i, float(loss), eager[0])
        for got, want in ((gv, eager[1]), (gt, eager[2])):
            assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max()), i
    np.savez(args.out + f".rank{rank}.npz", loss=float(loss), gv=gv.cpu().numpy(), prior=float(fit.regularizer_loss()),
             launched_regularizer=launched)
    print(f"rank {rank}/{world}: loss {float(loss):.7f} ok", flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
