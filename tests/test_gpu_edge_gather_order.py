"""k_edge_gather adds a lane's results in ONE documented order (d3m_edge_grad.h): lane_partial first when the plan is
incomplete, then the lane's crossings ascending, each as outward (.x/.y) then inward (.z/.w), the six lanes of a face in
order into the two vertices of their edge.  The yardstick is independent of the kernel: lane_cross, lane_block, xpos and
results are read out of the plan blob K4 left (as tools_dev/plan_stats.py reads it), added in numpy in float32 in that
order, and grad_faces must equal the sums BIT FOR BIT -- however the kernel fetches the results."""
import numpy as np
import pytest
import torch

import edge_chain_scenes as E

pytestmark = pytest.mark.gpu


def _check(faces, S, seed=0, plan_bytes=None, form=None):
    B, F = faces.shape[:2]
    maps = E.product_maps(faces, S, seed)
    _, g_rgb, g_alpha = E.random_inputs(B, F, S, seed)
    gf, plan, vis, ws = E.run_k4(faces, maps, g_rgb, g_alpha, S, plan_bytes=plan_bytes, form=form)
    pv = E.PlanView(plan, vis, ws, B, F, S)
    want = E.gather_in_numpy(pv)
    assert pv.n_visible > 0 and np.abs(want[np.isfinite(want)]).max() > 0
    E.assert_bit_equal(gf.cpu().numpy(), want)
    return pv


@pytest.mark.parametrize("B", [1, 3])
def test_grid_mesh_views(B):
    pv = _check(E.grid_views(10, B, 32), 32, seed=B)
    assert pv.complete and pv.n_visible % 42 != 0


@pytest.mark.parametrize("n,S,B", [(14, 48, 2), (20, 64, 1)])
def test_visible_counts_off_the_block_size(n, S, B):
    """more than one block of 42 listed faces, the last one partial"""
    pv = _check(E.grid_views(n, B, S, seed=2), S, seed=n)
    assert pv.complete and pv.n_visible > 42 and pv.n_visible % 42 != 0


def test_one_visible_face():
    S = 16
    faces = torch.from_numpy(E.pixel_triangles([[(2.5, 3.5), (12.5, 4.5), (5.5, 13.5)]], S))[None].cuda()
    pv = _check(faces, S)
    assert pv.n_visible == 1 and pv.complete


@pytest.mark.parametrize("S", [16, 33, 64])
def test_hand_placed_lane_lengths(S):
    """lanes of 0, 1, 3, 4, 5, 8 and 9 crossings (a round of four, its remainders, two rounds, two and one more)"""
    sizes = [(1, 5), (3, 4), (4, 3), (5, 9), (8, 1), (9, 8)]
    tris, x, y = [], 1.5, 1.5
    for w, h in sizes:                      # left to right, a new row of triangles where the image ends
        if x + w + 1 > S - 1:
            x, y = 1.5, y + 11.0
        if y + h + 1 > S - 1:
            break
        tris.append(E.corner_triangle(x, y, w, h))
        x += w + 2.0
    faces = torch.from_numpy(E.pixel_triangles(tris, S))[None].cuda()
    pv = _check(faces, S, seed=S)
    counts = set(pv.lane_cross[:pv.n_visible * 6, 1].tolist())
    assert pv.complete and pv.n_visible == len(tris)
    if S == 64:
        assert len(tris) == len(sizes) and {0, 1, 3, 4, 5, 8, 9} <= counts, sorted(counts)
    else:
        assert {0, 1, 3, 4} <= counts, sorted(counts)


def _large_triangles(S):
    """8 triangles across most of the raster, stacked in depth: lanes of hundreds of crossings"""
    rng = np.random.default_rng(5)
    tris = [[(rng.uniform(2, 0.3 * S), rng.uniform(2, 0.3 * S)), (rng.uniform(0.7 * S, S - 3), rng.uniform(2, 0.5 * S)),
             (rng.uniform(0.2 * S, 0.8 * S), rng.uniform(0.7 * S, S - 3))] for _ in range(8)]
    return torch.from_numpy(E.pixel_triangles(tris, S, z=1.0 + 0.1 * np.arange(8)))[None].cuda()


def test_large_triangles_many_chunks():
    """a block of more crossings than one LDS chunk of the gather pass (1024); so few faces that the plan's scatter pass
    deals the block's rounds to several workgroups"""
    S = 256
    pv = _check(_large_triangles(S), S, seed=7)
    first, end = pv.lane_runs()
    assert pv.complete and not pv.one_pass
    assert int((end - first).sum()) > 2 * 1024 and int((end - first).max()) > 100


@pytest.mark.parametrize("scene", ["grid", "large"])
def test_workspace_too_small_for_the_records(scene):
    """a blob without room for the batch's crossings: no record is used, k_edge_overflow walks every crossing and the
    lanes' sums come from lane_partial"""
    S = 32 if scene == "grid" else 256
    faces = E.grid_views(10, 3, S) if scene == "grid" else _large_triangles(S)
    B, F = faces.shape[:2]
    pv = _check(faces, S, seed=11, plan_bytes=E.plan_bytes_for(B, F, S, 100))
    assert not pv.records and not pv.complete and pv.total > pv.cap
    assert np.abs(pv.lane_partial[:pv.n_visible * 6]).max() > 0
