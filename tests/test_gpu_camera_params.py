"""Learnable cameras inside the render nodes: the camera's parameter tensors are autograd inputs of the lit node and of the
silhouette / depth node, read from device memory by their kernels, and receive their gradients
(d3m_camera_params_backward); MultiViewFit(optimise_cameras=True) returns this rank's eye gradient."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import kernels_launched

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "camera_golden.npz")
NEW_KERNELS = {"k_camera_params_partial", "k_camera_params_finish"}
D3M_OK, D3M_ERR_INVALID = 0, 1          # include/d3m_raster.h


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def _cam_grad(grads):
    from deep3dmap_amd import _lib
    return _lib.D3MCameraGrad(*[_lib.ptr(g) for g in grads])


def _raw_params_backward(p, v, g, grads):
    from deep3dmap_amd import _lib
    from deep3dmap_amd.neural_renderer import cameras
    L = _lib.lib()
    cam, _keep = cameras._camera_struct(p, v.device)
    basis, _bk = cameras.basis_struct(p, "vectors")
    ws = torch.empty(int(L.d3m_camera_params_backward_workspace_bytes(p["batch"], v.shape[1], p["mode"])),
                     dtype=torch.uint8, device=v.device)
    rc = L.d3m_camera_params_backward(_lib.ptr(v), v.shape[0], ctypes.byref(cam),
                                      ctypes.byref(basis) if basis is not None else None, _lib.ptr(g),
                                      ctypes.byref(_cam_grad(grads)), p["batch"], v.shape[1], _lib.ptr(ws), ws.numel(),
                                      _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _oracle_camera(kind, v, params, orig_size=256.0, angle=30.0):
    """float64 torch autograd form of the oracle's restatement of NR/look_at.py, look.py, perspective.py, projection.py"""
    from oracle import nr_oracle as O
    B = v.shape[0]
    if kind == "projection":
        K, R, t, d = params
        return O._projection_torch(v, K.expand(B, 3, 3), R.expand(B, 3, 3), t.reshape(-1, 1, 3), d.expand(B, 5), orig_size)
    e, a, u = (x.reshape(-1, 3).expand(B, 3) for x in params)
    out = O._look_at_torch(v, e, a, u) if kind == "look_at" else O._look_torch(v, e, a, u)
    return O.perspective(out, angle=angle)


# ---- 1. the kernel against the reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["look_at_shared", "look_at_per_batch", "look_shared", "look_per_batch",
                                  "projection_shared", "projection_per_batch"])
def test_params_backward_matches_reference_golden_and_oracle(case):
    from deep3dmap_amd import _lib
    from deep3dmap_amd.neural_renderer import cameras
    z = np.load(GOLDEN)
    kind = case.rsplit("_", 2)[0] if "per_batch" in case else case.rsplit("_", 1)[0]
    v = torch.from_numpy(z["vertices"]).cuda()
    up = torch.from_numpy(z["upstream"]).cuda()
    n = 4 if kind == "projection" else 3
    ps = [torch.from_numpy(z[f"{case}/p{k}"]) for k in range(n)]
    if kind == "projection":
        K, R, t, d = (x.cuda() for x in ps)
        p = cameras.projection_params(v, K, R, t, d, float(z["orig_size"]))
        grads = [torch.empty_like(p["eye_or_t"]), None, None, torch.empty_like(p["rot"]), torch.empty_like(p["K"]),
                 torch.empty_like(p["dist"])]
        mine = [grads[4], grads[3], grads[0], grads[5]]
    else:
        fn = cameras.look_at_params if kind == "look_at" else cameras.look_params
        p = fn(v, *(x.cuda() for x in ps), _perspective_angle=float(z["angle"]))
        grads = [torch.empty_like(t) for t in cameras.camera_inputs(p)[:3]] + [None] * 3
        mine = grads[:3]
    assert _raw_params_backward(p, v, up, grads) == D3M_OK
    for k in range(n):
        ref = torch.from_numpy(z[f"{case}/grad_p{k}"])
        got = mine[k].cpu().reshape(ref.shape)
        assert torch.allclose(got, ref, rtol=2e-4, atol=2e-5), (case, k, float((got - ref).abs().max()))
    # float64 autograd of the oracle
    p64 = [x.double().requires_grad_(True) for x in ps]
    out = _oracle_camera(kind, torch.from_numpy(z["vertices"]).double(), p64, float(z["orig_size"]), float(z["angle"]))
    g64 = torch.autograd.grad(out, p64, torch.from_numpy(z["upstream"]).double())
    for k in range(n):
        assert _rel(mine[k].cpu().reshape(g64[k].shape), g64[k]) <= 1e-5, (case, k)
    # the public function: the same gradients through autograd, and the vertices' gradient
    vv = v.clone().requires_grad_(True)
    pp = [x.cuda().requires_grad_(True) for x in ps]
    if kind == "projection":
        o = cameras.projection(vv, *pp, float(z["orig_size"]))
    else:
        o = (cameras.look_at if kind == "look_at" else cameras.look)(vv, *pp, _perspective_angle=float(z["angle"]))
    (o * up).sum().backward()
    assert torch.allclose(o.detach().cpu(), torch.from_numpy(z[f"{case}/out"]), rtol=2e-4, atol=2e-5)
    assert torch.allclose(vv.grad.cpu(), torch.from_numpy(z[f"{case}/grad_vertices"]), rtol=2e-4, atol=2e-5)
    for k in range(n):
        assert torch.allclose(pp[k].grad.cpu(), torch.from_numpy(z[f"{case}/grad_p{k}"]), rtol=2e-4, atol=2e-5)


# ---- 2. the render nodes against the chain rule ---------------------------------------------------------------------------
def _scene(B, shared, n=12, size=32):
    from deep3dmap_amd import synthetic
    v, tri = synthetic.grid_mesh(n)
    tex = synthetic.random_textures(tri.shape[0], 2)
    v, tri, tex = torch.from_numpy(v).cuda()[None], torch.from_numpy(tri).int().cuda()[None], \
        torch.from_numpy(tex).float().cuda()[None]
    if not shared:
        v = v.repeat(B, 1, 1) + 0.02 * torch.arange(B, dtype=torch.float32, device="cuda")[:, None, None]
    return v.contiguous(), tri, tex


def _camera(kind, B, per_view, size):
    """(Renderer attributes, oracle parameter list, per-call kwargs)"""
    if kind == "projection":
        K = torch.tensor([[[size * 1.2, 0, size / 2], [0, size * 1.2, size / 2], [0, 0, 1]]], dtype=torch.float32)
        R = torch.eye(3)[None]
        t = torch.tensor([[[0.05, -0.03, 2.5]]])
        d = torch.tensor([[0.02, -0.01, 0.001, 0.002, 0.0]])
        if per_view:
            K, R, t, d = K.repeat(B, 1, 1), R.repeat(B, 1, 1), t.repeat(B, 1, 1), d.repeat(B, 1)
            t = t + 0.05 * torch.arange(B, dtype=torch.float32)[:, None, None]
        return [K, R, t, d]
    eye = torch.tensor([0.4, 0.7, -2.4])
    if per_view:
        eye = torch.stack([eye + torch.tensor([0.1 * b, -0.05 * b, 0.0]) for b in range(B)])
    if kind == "look":
        direction = -eye / eye.norm(dim=-1, keepdim=True)
        return [eye, direction]
    return [eye]


def _renderer(kind, size, aa, params):
    from deep3dmap_amd import neural_renderer as nr
    r = nr.Renderer(camera_mode=kind, image_size=size, anti_aliasing=aa, orig_size=size)
    kw = {}
    if kind == "projection":
        kw = dict(K=params[0], R=params[1], t=params[2], dist_coeffs=params[3])
    else:
        r.eye = params[0]
        if kind == "look":
            r.camera_direction = params[1]
    return r, kw


def _targets(B, size, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rgb = torch.rand(B, 3, size, size, device="cuda", generator=g)
    depth = torch.rand(B, size, size, device="cuda", generator=g) * 3
    alpha = (torch.rand(B, size, size, device="cuda", generator=g) > 0.5).float()
    return rgb, depth, alpha, alpha


def _run_inside(method, kind, v, tri, tex, params, size, aa, targets, weights):
    """method's scalar with the camera inside the node: (images, scalar, camera parameter gradients)"""
    ps = [x.cuda().requires_grad_(True) for x in params]
    r, kw = _renderer(kind, size, aa, ps)
    assert r._camera_in_node(v, **kw) is not None
    if method == "render":
        rgb, depth, alpha = r.render(v, tri, tex, **kw)
        imgs = (rgb, depth, alpha)
        s = (rgb * weights[0]).sum() + (depth * weights[1]).sum() + (alpha * weights[2]).sum()
    elif method == "render_fit_loss":
        s = r.render_fit_loss(v, tri, tex, targets, **kw)
        imgs = (s.detach().clone(),)
    elif method == "silhouettes":
        a = r.render_silhouettes(v, tri, **kw)
        imgs, s = (a,), (a * weights[2]).sum()
    else:
        d = r.render_depth(v, tri, **kw)
        imgs, s = (d,), (d * weights[1]).sum()
    grads = torch.autograd.grad(s, ps)
    return [x.detach() for x in imgs], s.detach(), grads


def _run_outside(method, kind, v, tri, tex, params, size, aa, targets, weights):
    """the same with the camera outside: HIP screen vertices as a leaf, then float64 oracle autograd of the camera"""
    from deep3dmap_amd.neural_renderer import cameras, mesh_ops
    from deep3dmap_amd.neural_renderer.rasterize import (rasterize_depth, rasterize_lit, rasterize_lit_fit,
                                                         rasterize_silhouettes)
    r, kw = _renderer(kind, size, aa, [x.cuda() for x in params])
    sv = r._transform(v, kw.get("K"), kw.get("R"), kw.get("t"), kw.get("dist_coeffs"), None).detach().requires_grad_(True)
    light = r._light_cfg()
    if method == "render":
        out = rasterize_lit(sv, v, tri, tex, light, True, size, aa, r.near, r.far, r.rasterizer_eps, r.background_color)
        imgs = (out["rgb"], out["depth"], out["alpha"])
        s = (imgs[0] * weights[0]).sum() + (imgs[1] * weights[1]).sum() + (imgs[2] * weights[2]).sum()
    elif method == "render_fit_loss":
        s = rasterize_lit_fit(sv, v, tri, tex, light, True, targets, size, r.near, r.far, r.rasterizer_eps,
                              r.background_color, anti_aliasing=aa)
        imgs = (s.detach().clone(),)
    elif method == "silhouettes":
        a = rasterize_silhouettes(mesh_ops.gather_faces(sv, tri, True), size, aa)
        imgs, s = (a,), (a * weights[2]).sum()
    else:
        d = rasterize_depth(mesh_ops.gather_faces(sv, tri, True), size, aa)
        imgs, s = (d,), (d * weights[1]).sum()
    (g_sv,) = torch.autograd.grad(s, [sv])
    p64 = [x.double().requires_grad_(True) for x in params]
    if kind == "look":
        p64c = [p64[0], p64[1], torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64)]
    elif kind == "look_at":
        p64c = [p64[0], torch.zeros(3, dtype=torch.float64), torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64)]
    else:
        p64c = p64
    B = sv.shape[0]
    o = _oracle_camera(kind, v.detach().cpu().double().expand(B, -1, -1), p64c, float(size))
    grads = torch.autograd.grad(o, p64, g_sv.cpu().double())
    return [x.detach() for x in imgs], s.detach(), grads


CASES = [  # (method, kind, B, per_view, aa, shared mesh)
    ("render", "look_at", 3, True, False, True), ("render", "look", 1, False, True, True),
    ("render", "projection", 3, False, False, False),
    ("render_fit_loss", "look_at", 3, True, False, True), ("render_fit_loss", "look_at", 1, False, True, False),
    ("render_fit_loss", "projection", 3, True, True, True), ("render_fit_loss", "look", 3, True, False, True),
    ("silhouettes", "look_at", 1, False, False, True), ("silhouettes", "look", 3, True, True, False),
    ("silhouettes", "projection", 3, True, False, True),
    ("depth", "look_at", 3, True, True, True), ("depth", "projection", 1, False, False, True),
    ("depth", "look", 3, False, False, False),
]


@pytest.mark.parametrize("method,kind,B,per_view,aa,shared", CASES)
def test_render_nodes_match_the_chain_rule(method, kind, B, per_view, aa, shared):
    size = 32
    v, tri, tex = _scene(B, shared)
    vb = v if not shared or B == 1 else v          # (a shared mesh: the camera makes the batch)
    params = _camera(kind, B, per_view, size)
    if shared and B > 1 and not per_view:
        vb = v.expand(B, -1, -1).contiguous()        # (shared parameters of B views need B from the vertices)
    targets = _targets(B, size)
    g = torch.Generator(device="cuda").manual_seed(1)
    weights = (torch.randn(B, 3, size, size, device="cuda", generator=g), torch.randn(B, size, size, device="cuda", generator=g),
               torch.randn(B, size, size, device="cuda", generator=g))
    im_in, s_in, g_in = _run_inside(method, kind, vb, tri, tex, params, size, aa, targets, weights)
    im_out, s_out, g_out = _run_outside(method, kind, vb, tri, tex, params, size, aa, targets, weights)
    for a, b in zip(im_in, im_out):
        if method == "render_fit_loss":     # (the objective's value: its partial sums arrive in any order)
            assert torch.allclose(a, b, rtol=1e-5, atol=0)
        else:
            assert torch.equal(a, b)
    for a, b in zip(g_in, g_out):
        assert a.shape == b.shape
        if float(b.abs().max()) > 0:
            assert _rel(a.cpu(), b) <= 1e-4, (method, kind, _rel(a.cpu(), b))


# ---- 3. end to end against the oracle renderer ----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["silhouettes", "depth"])
def test_learnable_eye_end_to_end_matches_oracle(mode):
    from deep3dmap_amd import neural_renderer as nr, synthetic
    from oracle import nr_oracle as O
    v, tri = synthetic.grid_mesh(10)
    v, tri = torch.from_numpy(v)[None], torch.from_numpy(tri).int()[None]
    eye0 = torch.tensor([[0.5, 0.8, -2.6], [-0.4, 0.3, -2.3]])
    g = torch.Generator().manual_seed(2)
    w = torch.randn(2, 40, 40, generator=g)
    res = []
    for mod, dev in ((nr, "cuda"), (O, "cpu")):
        r = mod.Renderer(camera_mode="look_at", image_size=40, anti_aliasing=False)
        r.eye = eye0.clone().to(dev).requires_grad_(True)
        img = r(v.to(dev).expand(2, -1, -1), tri.to(dev), mode=mode)
        (img * w.to(dev)).sum().backward()
        res.append((img.detach().cpu(), r.eye.grad.cpu()))
    assert torch.allclose(res[0][0], res[1][0], rtol=1e-4, atol=1e-5)
    assert _rel(res[0][1], res[1][1]) <= 1e-3, (res[0][1], res[1][1])


# ---- 4. the route -----------------------------------------------------------------------------------------------------------
def test_learnable_eye_runs_in_the_node_and_constant_cameras_never_launch_the_new_kernels():
    from deep3dmap_amd import neural_renderer as nr
    from deep3dmap_amd.neural_renderer import cameras
    assert not hasattr(cameras, "_frame_torch") and not hasattr(cameras, "_view_torch")
    v, tri, tex = _scene(3, True)
    for learnable in (True, False):
        r = nr.Renderer(camera_mode="look_at", image_size=32, anti_aliasing=False)
        r.eye = torch.tensor([[0.4, 0.7, -2.4], [0.2, 0.5, -2.5], [0.0, 0.6, -2.2]], device="cuda").requires_grad_(learnable)
        vv = v.clone().requires_grad_(True)
        blk = r._camera_in_node(vv)
        assert blk is not None and cameras.camera_learnable(blk) == learnable
        with kernels_launched() as k:
            rgb, depth, alpha = r.render(vv, tri, tex)
            (rgb.sum() + alpha.sum()).backward()
            r.render_silhouettes(vv, tri).sum().backward()
            torch.cuda.synchronize()
        assert "k_camera_forward" not in k.names and "k_camera_basis" not in k.names
        if learnable:
            assert NEW_KERNELS <= k.names, k.names
            assert r.eye.grad is not None and float(r.eye.grad.abs().sum()) > 0
        else:
            assert not (NEW_KERNELS & k.names), k.names


# ---- 5. example 4's shape ------------------------------------------------------------------------------------------------
def test_example4_shape_constant_vertices_learnable_eye_silhouettes():
    from deep3dmap_amd import neural_renderer as nr, synthetic
    v, tri = synthetic.grid_mesh(16)

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.register_buffer("vertices", torch.from_numpy(v)[None])
            self.register_buffer("faces", torch.from_numpy(tri).int()[None])
            self.renderer = nr.Renderer(camera_mode="look_at", image_size=64)
            self.renderer.eye = torch.nn.Parameter(torch.tensor([0.6, 1.0, -2.8]))

        def forward(self, ref):
            image = self.renderer(self.vertices, self.faces, mode="silhouettes")
            return torch.sum((image - ref) ** 2)

    m = Model().cuda()
    m.renderer.eye = torch.nn.Parameter(m.renderer.eye.detach().cuda())
    ref = torch.zeros(1, 64, 64, device="cuda")
    ref[:, 16:48, 20:44] = 1
    with kernels_launched() as k:
        loss = m(ref)
        loss.backward()
        torch.cuda.synchronize()
    assert NEW_KERNELS <= k.names
    assert m.renderer.eye.grad is not None and torch.isfinite(m.renderer.eye.grad).all()
    assert float(m.renderer.eye.grad.abs().sum()) > 0
    assert m.vertices.grad is None


# ---- 6. capture ---------------------------------------------------------------------------------------------------------
def _det(on):
    from deep3dmap_amd import _lib
    old = _lib.lib().d3m_get_deterministic()
    _lib.lib().d3m_set_deterministic(1 if on else 0)
    return old


@pytest.mark.parametrize("kind", ["look_at", "projection"])
def test_captured_step_reads_in_place_camera_updates(kind):
    from deep3dmap_amd import _lib
    size, B = 32, 3
    v, tri, tex = _scene(B, True)
    params = [x.cuda().requires_grad_(True) for x in _camera(kind, B, True, size)]
    r, kw = _renderer(kind, size, False, params)
    targets = _targets(B, size)

    def step():
        if kind == "look_at":
            s = r.render_fit_loss(v, tri, tex, targets, **kw)
        else:
            s = r.render_silhouettes(v, tri, **kw).square().sum()
        return (s.detach(),) + torch.autograd.grad(s, params)

    old = _det(True)
    try:
        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            for _ in range(2):
                step()
        cur.wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = step()
        for it in range(3):
            with torch.no_grad():
                for p in params:
                    p.add_(0.01 * (it + 1) * torch.ones_like(p) * (1 if p.dim() < 3 else 0.001))
            graph.replay()
            torch.cuda.synchronize()
            replayed = [x.clone() for x in out]
            eager = step()
            assert torch.allclose(replayed[0], eager[0], rtol=1e-6, atol=0)
            for a, b in zip(replayed[1:], eager[1:]):
                assert torch.equal(a, b)
        del graph
    finally:
        _lib.lib().d3m_set_deterministic(old)


# ---- 7. deterministic mode -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,kind", [("render_fit_loss", "look_at"), ("silhouettes", "projection"),
                                         ("depth", "look")])
def test_deterministic_learnable_camera_is_bit_reproducible(method, kind):
    size, B = 32, 3
    v, tri, tex = _scene(B, True)
    params = _camera(kind, B, True, size)
    targets = _targets(B, size)
    g = torch.Generator(device="cuda").manual_seed(1)
    weights = tuple(torch.randn(B, *s, device="cuda", generator=g) for s in ((3, size, size), (size, size), (size, size)))
    from deep3dmap_amd import _lib
    old = _det(True)
    try:
        runs = [_run_inside(method, kind, v, tri, tex, params, size, False, targets, weights)[2] for _ in range(3)]
    finally:
        _lib.lib().d3m_set_deterministic(old)
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)
    out = _run_outside(method, kind, v, tri, tex, params, size, False, targets, weights)[2]
    for a, b in zip(runs[0], out):
        if float(b.abs().max()) > 0:
            assert _rel(a.cpu(), b) <= 1e-5, _rel(a.cpu(), b)


# ---- 8. bad shapes ---------------------------------------------------------------------------------------------------------
def test_bad_shapes_raise_before_any_launch_and_raw_calls_are_refused():
    from deep3dmap_amd import _lib, neural_renderer as nr
    from deep3dmap_amd.neural_renderer import cameras
    v, tri, tex = _scene(3, False)
    bad = [("look_at", dict(eye=torch.ones(2, 3, device="cuda", requires_grad=True))),
           ("look_at", dict(eye=torch.ones(3, 2, device="cuda", requires_grad=True))),
           ("look", dict(eye=torch.ones(3, device="cuda"), camera_direction=torch.ones(4, 3, device="cuda", requires_grad=True))),
           ("projection", dict(t=torch.ones(4, 1, 3, device="cuda", requires_grad=True)))]
    for kind, attrs in bad:
        r = nr.Renderer(camera_mode=kind, image_size=32, anti_aliasing=False,
                        K=torch.eye(3, device="cuda")[None], R=torch.eye(3, device="cuda")[None],
                        t=torch.tensor([[0.0, 0.0, 2.5]], device="cuda"))
        for a, x in attrs.items():
            setattr(r, a, x)
        with kernels_launched() as k:
            for fn in (lambda: r.render(v, tri, tex), lambda: r.render_silhouettes(v, tri),
                       lambda: r.render_fit_loss(v, tri, tex, _targets(3, 32))):
                with pytest.raises(ValueError):
                    fn()
            torch.cuda.synchronize()
        assert not k.names, k.names
    # raw C calls
    L = _lib.lib()
    p = cameras.look_at_params(v, torch.tensor([0.4, 0.7, -2.4], device="cuda"), _perspective_angle=30)
    g = torch.ones_like(v)
    e = torch.empty(1, 3, device="cuda")
    assert _raw_params_backward(p, v, g, [e, None, None, None, None, None]) == D3M_OK
    assert _raw_params_backward(p, v, g, [e, None, None, None, torch.empty(1, 3, 3, device="cuda"), None]) == D3M_ERR_INVALID
    cam, _keep = cameras._camera_struct(p, v.device)
    ws = torch.empty(int(L.d3m_camera_params_backward_workspace_bytes(3, v.shape[1], p["mode"])), dtype=torch.uint8,
                     device="cuda")
    gs = _cam_grad([e, torch.empty(1, 3, device="cuda"), None, None, None, None])
    for args in ((v, 3, None, g, gs, 3),              # at without the basis
                 (v, 3, None, None, _cam_grad([e] + [None] * 5), 3),      # no grad_screen
                 (v, 2, None, g, _cam_grad([e] + [None] * 5), 3),         # vertices batch 2 of 3 views
                 (v, 3, None, g, _cam_grad([e] + [None] * 5), 0)):        # no views
        vv, vb, basis, gg, gstruct, B = args
        rc = L.d3m_camera_params_backward(_lib.ptr(vv), vb, ctypes.byref(cam), basis, _lib.ptr(gg), ctypes.byref(gstruct), B,
                                          vv.shape[1], _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
        assert rc == D3M_ERR_INVALID
    bs, _bk = cameras.basis_struct(p, "vectors")
    bs.eye_batch = 2
    rc = L.d3m_camera_params_backward(_lib.ptr(v), 3, ctypes.byref(cam), ctypes.byref(bs), _lib.ptr(g), ctypes.byref(gs), 3,
                                      v.shape[1], _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
    assert rc == D3M_ERR_INVALID


# ---- 9. MultiViewFit(optimise_cameras=True) ---------------------------------------------------------------------------------
def _fit(optimise_cameras, rank=0, world_size=1, n_views=4, size=48, **kw):
    from deep3dmap_amd import synthetic
    from deep3dmap_amd.multiview import MultiViewFit
    v, tri = synthetic.grid_mesh(14)
    tex = synthetic.random_textures(tri.shape[0], 2)
    eyes = synthetic.camera_ring(n_views)
    fit = MultiViewFit(v, tri, tex, eyes, image_size=size, rank=rank, world_size=world_size,
                       optimise_cameras=optimise_cameras, **kw)
    fit.set_targets_from(v * 1.05)
    return fit


def test_multiview_fit_optimise_cameras():
    from deep3dmap_amd import _lib
    with pytest.raises(ValueError):
        _fit(True, split_exchange=True)
    fit = _fit(True)
    assert fit.split_exchange is False
    out = fit.step()
    assert len(out) == 4
    loss, gv, gt, ge = (x.clone() if x is not None else None for x in out)
    assert ge.shape == fit.eyes.shape and float(ge.abs().sum()) > 0
    # against render_fit_loss + autograd on the same scene
    r = fit.renderer
    eyes = fit.eyes.detach().clone().requires_grad_(True)
    r.eye = eyes
    s = r.render_fit_loss(fit.vertices.detach()[None], fit.triangles[None], fit.textures.detach()[None], tuple(fit.targets) +
                          (fit.targets[2], fit.mask_sum))
    (g_ref,) = torch.autograd.grad(s, [eyes])
    del s               # (the fit's leaves take no part in it: their AccumulateGrad nodes stay on the fit's stream)
    r.eye = fit.eyes
    assert _rel(ge, g_ref) <= 1e-4
    # captured: replays read in-place updates of the eyes; replayed == eager (an uncaptured fit with the same eyes)
    fit.capture_graph()
    other = _fit(True)
    for f in (fit, other):
        with torch.no_grad():
            f.eyes.add_(0.01)
    rep = fit.step()[3].clone()
    ref = other.step()[3].clone()
    assert _rel(rep, ref) <= 1e-4 and not torch.equal(rep, ge)
    fit.release_graph()
    # deterministic: bit for bit against render_fit_loss + autograd; mesh gradients as with constant cameras
    old = _det(True)
    try:
        fit_d, fit_c = _fit(True), _fit(False)
        ld, gvd, gtd, ged = (x.clone() for x in fit_d.step())
        lc, gvc, gtc = (x.clone() for x in fit_c.step())
        assert torch.equal(gvd, gvc) and torch.equal(gtd, gtc) and torch.equal(ld, lc)
        r = fit_d.renderer
        eyes = fit_d.eyes.detach().clone().requires_grad_(True)
        r.eye = eyes
        s = r.render_fit_loss(fit_d.vertices.detach()[None], fit_d.triangles[None], fit_d.textures.detach()[None], tuple(fit_d.targets) +
                              (fit_d.targets[2], fit_d.mask_sum))
        (g_ref,) = torch.autograd.grad(s, [eyes])
        assert torch.equal(ged, g_ref)
        r.eye = fit_d.eyes
        fit_d.capture_graph()
        for _ in range(2):
            assert torch.equal(fit_d.step()[3], ged)
        with torch.no_grad():
            fit_d.eyes.add_(0.01)
            fit_c.eyes.add_(0.01)
        other = _fit(True)
        with torch.no_grad():
            other.eyes.add_(0.01)
        assert torch.equal(fit_d.step()[3], other.step()[3])
        fit_d.release_graph()
    finally:
        _lib.lib().d3m_set_deterministic(old)


def test_multiview_fit_two_ranks_eye_gradients_concatenate_to_one_ranks():
    one = _fit(True)
    ge_one = one.step()[3].clone()
    parts = []
    for rank in range(2):
        f = _fit(True, rank=rank, world_size=2)
        f.mask_sum = one.mask_sum.clone()           # (the global normaliser: what set_targets_from all-reduces)
        parts.append(f.step()[3].clone())
    both = torch.cat(parts)
    assert _rel(both, ge_one) <= 1e-5, _rel(both, ge_one)
