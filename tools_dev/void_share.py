"""The share of void tiles of the fused fit objective's pass (docs/EXPERIMENTS.md K) in the headline scene, its 8-view shard
and config 5, counted on the CPU from the fit's targets and its rendered coverage (the images of one step).  One JSON
object; written to dev_out/void_tiles_share.json (profiles/void_tiles_share.json is a copy of one run).  Needs a GPU."""
import json, sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from deep3dmap_amd import synthetic
from deep3dmap_amd.multiview import MultiViewFit
out = {}
for name, mesh_n, S, views in (("headline", 225, 512, 32), ("8-view shard", 225, 512, 8), ("config 5", 709, 1024, 8)):
    v, tri = synthetic.grid_mesh(mesh_n)
    tex = synthetic.random_textures(tri.shape[0], 2)
    fit = MultiViewFit(v, tri, tex, synthetic.camera_ring(views), image_size=S, anti_aliasing=False, rank=0, world_size=1,
                       device="cuda:0", objective_in_renderer=True)
    fit.set_targets_from(synthetic.perturb(v))
    fit.keep_images = True
    fit.step()
    torch.cuda.synchronize()
    rgb_t, depth_t, alpha_t = (t.cpu().numpy() for t in fit.targets[:3])
    alpha = fit.images[2].cpu().numpy()
    ok = (alpha_t == 0) & np.isfinite(depth_t) & np.isfinite(rgb_t).all(1)
    r = {"covered_pixels": float((alpha > 0).mean()), "target_live_pixels": float((alpha_t != 0).mean())}
    for T in (16, 32):
        n = S // T
        tv = ok.reshape(views, n, T, n, T).all((2, 4))
        cov = (alpha > 0).reshape(views, n, T, n, T).any((2, 4))
        r[f"tile{T}"] = {"target_void": float(tv.mean()), "void": float((tv & ~cov).mean())}
    out[name] = r
    del fit
os.makedirs("dev_out", exist_ok=True)
json.dump(out, open("dev_out/void_tiles_share.json", "w"), indent=1)
print(json.dumps(out))
