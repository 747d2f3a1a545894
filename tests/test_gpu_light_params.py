"""Learnable and per-view lights in the lit render node (rasterize.light_on_device): the light's parameters are autograd
inputs of the node, read from device memory by its kernels, and receive their gradients (d3m_light_params_backward)."""
import os

import numpy as np
import pytest
import torch

from conftest import kernels_launched

pytestmark = pytest.mark.gpu

NAMES = ("intensity_ambient", "intensity_directional", "color_ambient", "color_directional", "direction")
ATTRS = ("light_intensity_ambient", "light_intensity_directional", "light_color_ambient", "light_color_directional",
         "light_direction")
NEW_KERNELS = {"k_lit_front_dev", "k_lit_back_dev", "k_face_light_backward_dev", "k_face_light_backward_gather_dev",
               "k_light_params_partial", "k_light_params_finish", "k_face_light_dev"}


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _scene(B, n=12, shared=False):
    from deep3dmap_amd import synthetic
    v, tri = synthetic.grid_mesh(n)
    tex = synthetic.random_textures(tri.shape[0], 2)
    v, tri, tex = torch.from_numpy(v)[None], torch.from_numpy(tri)[None], torch.from_numpy(tex)[None]
    if not shared:
        v = v.repeat(B, 1, 1) + 0.02 * torch.arange(B, dtype=torch.float32)[:, None, None]
        tri, tex = tri.repeat(B, 1, 1), tex.repeat(B, 1, 1, 1, 1, 1)
    return v, tri, tex


def _eyes(B):
    return torch.tensor([[0.4 + 0.1 * b, 0.7 - 0.05 * b, -2.4] for b in range(B)], dtype=torch.float32)


def _light(B, per_view):
    g = torch.Generator().manual_seed(3)
    if per_view:
        return [torch.rand(B, generator=g) * 0.4 + 0.3, torch.rand(B, generator=g) * 0.4 + 0.4,
                torch.rand(B, 3, generator=g) * 0.4 + 0.6, torch.rand(B, 3, generator=g) * 0.4 + 0.6,
                torch.tensor([0.3, 0.8, -0.5]) + 0.2 * torch.rand(B, 3, generator=g)]
    return [torch.tensor(0.45), torch.tensor(0.6), torch.tensor([0.9, 0.8, 1.0]), torch.tensor([1.0, 0.7, 0.6]),
            torch.tensor([0.3, 0.8, -0.5])]


def _render(mod, dev, v, tri, tex, light, eyes, size, aa, views=None, mode=None):
    """rgb, depth, alpha and the gradients of vertices, textures and the five light parameters"""
    r = mod.Renderer(camera_mode="look_at", image_size=size, anti_aliasing=aa)
    r.eye = eyes.to(dev) if views is None else eyes[views].to(dev)
    vv, tt = v.clone().to(dev).requires_grad_(True), tex.clone().to(dev).requires_grad_(True)
    lp = [x.clone().to(dev).requires_grad_(True) for x in light]
    for a, x in zip(ATTRS, lp):
        setattr(r, a, x)
    if mode == "rgb":
        rgb = r(vv, tri.to(dev), tt, mode="rgb")
        depth = alpha = torch.zeros(1, device=dev)
    else:
        rgb, depth, alpha = r(vv, tri.to(dev), tt)
    w = torch.linspace(0.5, 1.5, rgb[0].numel(), device=dev).reshape(rgb.shape[1:])     # (the same weights in every view)
    (rgb * w).sum().add(alpha.sum()).add(depth.clamp(max=5).sum()).backward()
    return [x.detach().cpu() for x in (rgb, depth, alpha)] + [vv.grad.cpu(), tt.grad.cpu()] + [x.grad.cpu() for x in lp]


# ---- 1. the materialised route against the reference's lighting (tests/golden/make_golden_light.py) -----------------------
@pytest.mark.parametrize("case", ["shared", "per_batch", "zero_dim"])
def test_mesh_ops_lighting_matches_reference_golden(case):
    from deep3dmap_amd.neural_renderer import mesh_ops
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "light_golden.npz"))
    g = lambda k: torch.from_numpy(z[k]).cuda()      # noqa: E731
    f, t = g("faces").requires_grad_(True), g("textures").requires_grad_(True)
    p = [g(f"{case}/{n}").requires_grad_(True) for n in NAMES]
    lit = mesh_ops.lighting(f, t, *p)
    (lit * g("upstream")).sum().backward()
    assert _rel(lit.detach(), g(f"{case}/lit")) < 1e-6
    assert _rel(f.grad, g(f"{case}/grad_faces")) < 1e-4
    assert _rel(t.grad, g(f"{case}/grad_textures")) < 1e-6
    for n, x in zip(NAMES, p):
        assert x.grad is not None, n
        assert _rel(x.grad, g(f"{case}/grad_{n}")) < 1e-5, n


# ---- 2. a learnable shared light through render() against the oracle under CPU autograd ------------------------------------
@pytest.mark.parametrize("aa", [False, True])
@pytest.mark.parametrize("B,size", [(2, 40), (4, 64)])
def test_learnable_shared_light_matches_oracle(aa, B, size):
    from deep3dmap_amd import neural_renderer as nr
    from oracle import nr_oracle as O
    v, tri, tex = _scene(B)
    light = _light(B, False)
    ref = _render(O, "cpu", v, tri, tex, light, _eyes(B), size, aa)
    got = _render(nr, "cuda", v, tri, tex, light, _eyes(B), size, aa)
    for k, (a, b) in enumerate(zip(got, ref)):
        assert _rel(a, b) < (1e-5 if k < 3 else 1e-3), k


# ---- 3. per-view light against the sum of single-view oracle renders ------------------------------------------------------
@pytest.mark.parametrize("shared", [False, True])
def test_per_view_light_matches_single_view_oracle_renders(shared):
    from deep3dmap_amd import neural_renderer as nr
    from oracle import nr_oracle as O
    B = 4
    v, tri, tex = _scene(B, shared=shared)
    light = _light(B, True)
    got = _render(nr, "cuda", v, tri, tex, light, _eyes(B), 48, False)
    parts = []
    for b in range(B):
        vb = v if shared else v[b:b + 1]
        tb, xb = (tri, tex) if shared else (tri[b:b + 1], tex[b:b + 1])
        parts.append(_render(O, "cpu", vb, tb, xb, [x[b] for x in light], _eyes(B), 48, False, views=[b]))
    for k in range(3):
        assert _rel(got[k], torch.cat([p[k] for p in parts])) < 1e-5, k
    cat_or_sum = (lambda xs: sum(xs)) if shared else (lambda xs: torch.cat(xs))
    assert _rel(got[3], cat_or_sum([p[3] for p in parts])) < 1e-3
    assert _rel(got[4], cat_or_sum([p[4] for p in parts])) < 1e-3
    for j in range(5):
        assert _rel(got[5 + j], torch.stack([p[5 + j] for p in parts])) < 1e-3, NAMES[j]


# ---- 4. finite differences of the light's parameters (the light does not move geometry) ------------------------------------
def test_light_gradients_match_finite_differences():
    from deep3dmap_amd import neural_renderer as nr
    B = 2
    v, tri, tex = (x.cuda() for x in _scene(B, n=8))
    light = [x.double().cuda() for x in _light(B, True)]
    r = nr.Renderer(camera_mode="look_at", image_size=32, anti_aliasing=False)
    r.eye = _eyes(B).cuda()
    w = torch.rand(B, 3, 32, 32, generator=torch.Generator().manual_seed(5)).cuda()

    def f(params):
        for a, x in zip(ATTRS, params):
            setattr(r, a, x.float())
        return (r(v, tri, tex, mode="rgb") * w).sum().double()
    lp = [x.clone().requires_grad_(True) for x in light]
    f(lp).backward()
    h = 1e-2
    for j, x in enumerate(light):
        flat = x.reshape(-1)
        for e in range(flat.numel()):
            up, dn = [y.clone() for y in light], [y.clone() for y in light]
            up[j].reshape(-1)[e] += h
            dn[j].reshape(-1)[e] -= h
            with torch.no_grad():
                fd = float((f(up) - f(dn)) / (2 * h))
            an = float(lp[j].grad.reshape(-1)[e])
            assert abs(an - fd) <= 2e-3 * max(1.0, abs(fd)), (NAMES[j], e, an, fd)


# ---- 5. render_fit_loss with a per-view learnable light equals render() + multiview_fit_loss -------------------------------
@pytest.mark.parametrize("aa", [False, True])
@pytest.mark.parametrize("groups", [1, 2])
def test_render_fit_loss_per_view_light_matches_composition(aa, groups):
    from deep3dmap_amd import neural_renderer as nr
    from deep3dmap_amd.core.losses import multiview_fit_loss
    B, s = 4, 32
    v, tri, tex = (x.cuda() for x in _scene(B, shared=True))
    gen = torch.Generator().manual_seed(9)
    targets = (torch.rand(B, 3, s, s, generator=gen).cuda(), torch.rand(B, s, s, generator=gen).cuda() + 2,
               (torch.rand(B, s, s, generator=gen) > 0.5).float().cuda(), (torch.rand(B, s, s, generator=gen) > 0.3).float().cuda())
    outs = []
    for fused in (True, False):
        r = nr.Renderer(camera_mode="look_at", image_size=s, anti_aliasing=aa)
        r.eye, r.view_groups = _eyes(B).cuda(), groups
        vv, tt = v.clone().requires_grad_(True), tex.clone().requires_grad_(True)
        lp = [x.clone().cuda().requires_grad_(True) for x in _light(B, True)]
        for a, x in zip(ATTRS, lp):
            setattr(r, a, x)
        if fused:
            images = tuple(torch.empty_like(t) for t in targets[:3])
            loss = r.render_fit_loss(vv, tri, tt, targets, images_out=images)
        else:
            rgb, depth, alpha = r(vv, tri, tt)
            loss = multiview_fit_loss(rgb, depth, alpha, *targets, link=False)
        loss.backward()
        outs.append([loss.detach(), vv.grad, tt.grad] + [x.grad for x in lp])
    for k, (a, b) in enumerate(zip(*outs)):
        assert _rel(a, b) < 1e-4, k


# ---- 6. routes -----------------------------------------------------------------------------------------------------------
def test_per_view_light_runs_in_the_lit_node_and_constant_light_keeps_its_kernels():
    from deep3dmap_amd import neural_renderer as nr
    B = 3
    v, tri, tex = (x.cuda() for x in _scene(B, shared=True))
    r = nr.Renderer(camera_mode="look_at", image_size=32, anti_aliasing=False)
    r.eye = _eyes(B).cuda()
    vv = v.clone().requires_grad_(True)
    for a, x in zip(ATTRS, _light(B, True)):
        setattr(r, a, x.cuda().requires_grad_(True))
    with kernels_launched() as k:
        rgb, depth, alpha = r(vv, tri, tex)
        rgb.sum().backward()
        torch.cuda.synchronize()
    assert {"k_lit_front_dev", "k_light_params_partial", "k_light_params_finish"} <= k.names, sorted(k.names)
    assert not any(n.startswith("k_lighting_") for n in k.names), sorted(k.names)
    r2 = nr.Renderer(camera_mode="look_at", image_size=32, anti_aliasing=False)
    r2.eye = _eyes(B).cuda()
    with kernels_launched() as k2:
        rgb, depth, alpha = r2(v.clone().requires_grad_(True), tri, tex)
        rgb.sum().backward()
        torch.cuda.synchronize()
    assert "k_lit_front" in k2.names and not (NEW_KERNELS & k2.names), sorted(k2.names)


# ---- 7. deterministic mode -----------------------------------------------------------------------------------------------
def test_deterministic_shared_learnable_light_is_bit_reproducible_and_per_view_is_refused():
    from deep3dmap_amd import _lib, neural_renderer as nr
    B = 3
    v, tri, tex = (x.cuda() for x in _scene(B, shared=True))
    old = _lib.lib().d3m_get_deterministic()
    _lib.lib().d3m_set_deterministic(1)
    try:
        runs = []
        for _ in range(2):
            r = nr.Renderer(camera_mode="look_at", image_size=40, anti_aliasing=False)
            r.eye = _eyes(B).cuda()
            vv, tt = v.clone().requires_grad_(True), tex.clone().requires_grad_(True)
            lp = [x.cuda().requires_grad_(True) for x in _light(B, False)]
            for a, x in zip(ATTRS, lp):
                setattr(r, a, x)
            rgb, depth, alpha = r(vv, tri, tt)
            (rgb.square().sum() + alpha.sum()).backward()
            runs.append([rgb, vv.grad, tt.grad] + [x.grad for x in lp])
        for a, b in zip(*runs):
            assert torch.equal(a, b)
        r = nr.Renderer(camera_mode="look_at", image_size=40, anti_aliasing=False)
        r.eye = _eyes(B).cuda()
        for a, x in zip(ATTRS, _light(B, True)):
            setattr(r, a, x.cuda().requires_grad_(True))
        with pytest.raises(NotImplementedError):
            r(v.clone().requires_grad_(True), tri, tex)
    finally:
        _lib.lib().d3m_set_deterministic(old)


# ---- 8. capture: the light is read when the graph replays ----------------------------------------------------------------
def test_captured_step_reads_the_per_view_light_at_replay():
    from deep3dmap_amd import neural_renderer as nr
    from deep3dmap_amd.graph import CapturedStep
    B = 3
    v, tri, tex = (x.cuda() for x in _scene(B, shared=True))
    r = nr.Renderer(camera_mode="look_at", image_size=32, anti_aliasing=False)
    r.eye = _eyes(B).cuda()
    vv = v.clone().requires_grad_(True)
    lp = [x.cuda().requires_grad_(True) for x in _light(B, True)]
    for a, x in zip(ATTRS, lp):
        setattr(r, a, x)

    def step():
        for x in lp + [vv]:
            x.grad = None
        rgb, depth, alpha = r(vv, tri, tex)
        rgb.square().sum().backward()
        return rgb.detach(), lp[4].grad
    run = CapturedStep(step).capture()
    with torch.no_grad():
        lp[0].mul_(0.5)
        lp[3].add_(0.1)
        lp[4].copy_(torch.tensor([[0.1, 0.9, -0.3]], device="cuda").expand(B, 3))
    rgb, _ = run()
    torch.cuda.synchronize()
    r2 = nr.Renderer(camera_mode="look_at", image_size=32, anti_aliasing=False)
    r2.eye = _eyes(B).cuda()
    for a, x in zip(ATTRS, lp):
        setattr(r2, a, x.detach().clone())
    with torch.no_grad():
        ref = r2(v, tri, tex, mode="rgb")
    assert torch.equal(rgb, ref)


# ---- 9. bad shapes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("attr,value", [("light_color_ambient", torch.ones(2, 3)), ("light_direction", torch.ones(3, 4)),
                                        ("light_intensity_ambient", torch.ones(5)),
                                        ("light_intensity_directional", torch.ones(3, 1))])
def test_bad_light_shapes_raise_before_any_launch(attr, value):
    from deep3dmap_amd import neural_renderer as nr
    B = 3
    v, tri, tex = (x.cuda() for x in _scene(B, shared=True))
    r = nr.Renderer(camera_mode="look_at", image_size=32, anti_aliasing=False)
    r.eye = _eyes(B).cuda()
    setattr(r, attr, value.cuda())
    with kernels_launched() as k:
        with pytest.raises(ValueError):
            r(v.clone().requires_grad_(True), tri, tex)
    assert not k.names
