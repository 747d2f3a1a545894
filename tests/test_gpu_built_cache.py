"""A captured step keeps what its kernels read after the cache has evicted it (neural_renderer/built_cache.py): the raw
addresses of the faces' adjacency (the deterministic mode's per-vertex gathers), of pose_vertices' int32 landmarks and of
param2points_bfm's concatenated basis are baked into the step's HIP graph, so they must live as long as the graph, whatever the
bounded cache does with its entry.  Every test: two eager steps (the bits), a capture, the entry evicted by `size` other keys,
every local reference dropped -- then, BEFORE any replay, the tensor must be alive and among the step's `_scratch_refs`; only
then is the graph replayed and compared bit for bit.  (A regression fails the assertion; it never replays over freed memory.)"""
import gc
import weakref

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _holds(r, t):
    return r is t or (isinstance(r, tuple) and any(_holds(x, t) for x in r))


def _kept(refs, alive):
    """`alive()` (a tensor) is, or is a field (of a field: Adjacency.csr.items) of, one of the objects the captured step holds."""
    return any(_holds(r, alive()) for r in refs)


def _replays_equal(captured, eager):
    for _ in range(2):
        got = captured()
        got = got if isinstance(got, (tuple, list)) else (got,)
        torch.cuda.synchronize()
        assert len(got) == len(eager) and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, eager))


def _evict_adjacency():
    from deep3dmap_amd.neural_renderer import row_gather as rg
    for i in range(rg._cache.size):                        # `size` other tiny topologies
        rg.vertex_adjacency(torch.tensor([[[0, 1, 2]]], dtype=torch.int32, device="cuda"), 3 + i)


def test_deterministic_lit_step_keeps_its_adjacency_after_eviction():
    from deep3dmap_amd import _lib, synthetic
    from deep3dmap_amd.multiview import MultiViewFit
    from deep3dmap_amd.neural_renderer import row_gather as rg
    v, tri = synthetic.grid_mesh(9)                        # 81 vertices, 128 faces
    fit = MultiViewFit(v, tri, synthetic.random_textures(tri.shape[0], 2), synthetic.camera_ring(2), image_size=32)
    fit.set_targets_from(synthetic.perturb(v, 0.03))
    with _lib.deterministic():
        eager = [[t.clone() for t in fit.step()] for _ in range(2)]
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(*eager))
        assert float(eager[0][1].abs().max()) > 0 and float(eager[0][2].abs().max()) > 0
        fit.capture_graph()
        adjacency = rg.vertex_adjacency(fit.triangles[None], v.shape[0])       # (a hit: what the node's state holds)
        assert adjacency.num_faces == tri.shape[0]
        items = weakref.ref(adjacency.csr.items)
        _evict_adjacency()
        del adjacency
        gc.collect()
        assert rg._faces_key(fit.triangles[None], v.shape[0]) not in rg._cache
        assert items() is not None and _kept(fit._runner._scratch_refs, items)
        for _ in range(2):
            got = fit.step()
            torch.cuda.synchronize()
            assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, eager[0]))
        fit.release_graph()


@pytest.mark.parametrize("node", ["silhouettes", "depth", "gather_faces"])
def test_deterministic_step_keeps_its_adjacency_after_eviction(node):
    """... the silhouette / depth node (its forward fetches the adjacency) and vertices_to_faces' adjoint (its backward does)."""
    from deep3dmap_amd import _lib, neural_renderer as nr, synthetic
    from deep3dmap_amd.graph import CapturedStep
    from deep3dmap_amd.neural_renderer import mesh_ops, row_gather as rg
    v_np, tri_np = synthetic.grid_mesh(9)
    V = v_np.shape[0]
    tri = torch.from_numpy(tri_np).int().cuda()[None]
    v = torch.from_numpy(v_np).float().cuda()[None].requires_grad_(True)
    if node == "gather_faces":
        w = torch.linspace(0.5, 1.5, 9, device="cuda").view(3, 3)
        loss = lambda: (mesh_ops.gather_faces(v, tri, True) ** 2 * w).sum()            # noqa: E731
    else:
        r = nr.Renderer(image_size=32, anti_aliasing=False, camera_mode="look_at", fill_back=True)
        r.eye = torch.from_numpy(synthetic.camera_ring(2)).float().cuda()
        render = getattr(r, "render_" + node)
        with torch.no_grad():
            target = torch.roll(render(v, tri), shifts=(3, -2), dims=(1, 2)).clamp(max=10.0)
        loss = lambda: ((render(v, tri).clamp(max=10.0) - target) ** 2).sum()          # noqa: E731

    def step():
        v.grad = None
        loss().backward()
        return v.grad

    with _lib.deterministic():
        eager = [step().clone() for _ in range(2)]
        assert float(eager[0].abs().max()) > 0 and torch.equal(_bits(eager[0]), _bits(eager[1]))
        captured = CapturedStep(step).capture()
        adjacency = rg.vertex_adjacency(tri, V)
        items = weakref.ref(adjacency.csr.items)
        _evict_adjacency()
        del adjacency
        gc.collect()
        assert rg._faces_key(tri, V) not in rg._cache
        assert items() is not None and _kept(captured._scratch_refs, items)
        _replays_equal(captured, eager[:1])
        captured.release()


def test_pose_step_keeps_its_landmarks_after_eviction():
    from deep3dmap_amd import neural_renderer as nr
    from deep3dmap_amd.graph import CapturedStep
    from deep3dmap_amd.neural_renderer import pose as po
    B, V = 2, 300                                           # two chunks of vertices
    rng = np.random.default_rng(11)
    x = torch.from_numpy(rng.standard_normal((V, 3)).astype(np.float32)).cuda().requires_grad_(True)
    pose = torch.tensor([[1.1, 0.2, -0.3, 0.1, 0.5, -0.2, 0.3], [0.8, -0.4, 0.1, 0.6, -0.1, 0.4, 0.2]]).cuda().requires_grad_(True)
    landmarks = torch.tensor([0, 7, 7, 299, 12], dtype=torch.int64).cuda()     # int64: the int32 form is the cache's alone
    w = [torch.from_numpy(rng.standard_normal(s).astype(np.float32)).cuda() for s in ((B, V, 3), (B, V, 2), (B, 5, 3))]

    def step():
        x.grad = pose.grad = None
        out = nr.pose_vertices(x, pose, translation_scale=2.0, uv_size=4.0, landmarks=landmarks)
        (((out.posed ** 2) * w[0]).sum() + (out.uv * w[1]).sum() + ((out.landmarks ** 2) * w[2]).sum()).backward()
        return x.grad, pose.grad

    eager = [[t.clone() for t in step()] for _ in range(2)]
    assert all(float(t.abs().max()) > 0 for t in eager[0])
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(*eager))
    captured = CapturedStep(step).capture()
    int32_form = po._landmarks_in_range(landmarks, V)
    assert int32_form.dtype == torch.int32 and int32_form.data_ptr() != landmarks.data_ptr()
    alive = weakref.ref(int32_form)
    others = [torch.tensor([i], device="cuda") for i in range(po._checked_landmarks.size)]
    for t in others:
        po._landmarks_in_range(t, V)
    del int32_form
    gc.collect()
    assert po.tensor_key(landmarks) + (V,) not in po._checked_landmarks
    assert alive() is not None and _kept(captured._scratch_refs, alive)
    _replays_equal(captured, eager[0])
    captured.release()


def test_param2points_bfm_step_keeps_its_basis_after_eviction():
    from deep3dmap_amd.core import bfm_tools
    from deep3dmap_amd.graph import CapturedStep
    gen = torch.Generator().manual_seed(5)
    rand = lambda *s: torch.rand(*s, generator=gen).cuda()                     # noqa: E731
    sp = {"w": rand(120, 5) - 0.5, "sigma": rand(5) + 0.5, "mu_shape": rand(120, 1)}
    ep, op = {"w_exp": rand(120, 3) - 0.5}, {"sigma_exp": rand(3) + 0.5}
    preds = (rand(2, 15) - 0.5).requires_grad_(True)
    w = rand(2, 40, 3)

    def step():
        preds.grad = None
        face, pose = bfm_tools.param2points_bfm(sp, ep, op, preds)
        ((face ** 2) * w).sum().backward()
        return face.detach(), preds.grad           # (no grad_fn leaves the step: nothing else holds the basis)

    eager = [[t.clone() for t in step()] for _ in range(2)]
    assert float(eager[0][1][:, :8].abs().max()) > 0
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(*eager))
    captured = CapturedStep(step).capture()
    basis, scale = weakref.ref(bfm_tools._basis(sp["w"], ep["w_exp"])), weakref.ref(bfm_tools._scale(sp["sigma"], op["sigma_exp"]))
    assert basis().shape == (120, 8)
    for _ in range(bfm_tools._bases.size):                 # `size` other pairs
        bfm_tools._basis(rand(3, 1), rand(3, 1))
        bfm_tools._scale(rand(1) + 1, rand(1) + 1)
    gc.collect()
    assert len(bfm_tools._bases) == len(bfm_tools._scales) == bfm_tools.CACHE_SIZE
    assert (bfm_tools.tensor_key(sp["w"]), bfm_tools.tensor_key(ep["w_exp"])) not in bfm_tools._bases
    assert basis() is not None and _kept(captured._scratch_refs, basis)
    assert scale() is not None and _kept(captured._scratch_refs, scale)
    _replays_equal(captured, eager[0])
    captured.release()
