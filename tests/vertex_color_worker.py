"""One rank of a small camera-sharded fit with per-vertex colours, run as a child process by
tests/test_gpu_vertex_colors.py: grid_mesh(9), 4 cameras at 64x64 shared among the ranks, the captured step.  Every rank
uses cuda:0 and the collective runs over gloo.  Writes what the rank holds after the exchange -- the loss and the gradients
of the objective over ALL cameras, the colour gradient as [V,3] -- to --out.  Exit code != 0 on any failure."""
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
    from deep3dmap_amd import synthetic
    from deep3dmap_amd.multiview import MultiViewFit
    v, tri = synthetic.grid_mesh(9)
    colors = np.random.default_rng(3).random((v.shape[0], 3), dtype=np.float32)
    fit = MultiViewFit(v, tri, None, synthetic.camera_ring(4), image_size=64, rank=rank, world_size=world,
                       vertex_colors=colors)
    assert not fit.split_exchange
    fit.set_targets_from(synthetic.perturb(v))
    loss, gv, gc = fit.step()
    eager = (float(loss), gv.clone(), gc.clone())
    fit.capture_graph()
    assert fit.graph_captured
    for i in range(2):
        loss, gv, gc = fit.step()
        torch.cuda.synchronize()
        assert abs(float(loss) - eager[0]) <= 1e-5 * abs(eager[0]), (i, float(loss), eager[0])
        for got, want in ((gv, eager[1]), (gc, eager[2])):
            assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max()), i
    np.savez(args.out + f".rank{rank}.npz", loss=float(loss), gv=gv.cpu().numpy(), gc=gc.cpu().numpy(),
             flat_numel=fit._flat.numel())
    print(f"rank {rank}/{world}: loss {float(loss):.7f} ok", flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
