"""Fused and push-pull filled uv textures on the device (neural_renderer/uv_fill.py, csrc/d3m_uv_fill.h) against the float64
restatement of tests/uv_fill_scenes.py; tolerances: uv_fill_scenes.DEVICE_TOLERANCE, 8 x the float32 yardstick of each kind
(tests/test_uv_fill_host.py holds the figures).  `valid` rests on w > 0 alone and must be the reference's exactly."""
import pytest
import torch

import uv_bake_scenes as UB
import uv_fill_scenes as UF
from conftest import kernels_launched
from vertex_attribute_scenes import VIEWING_ANGLE, image_size_of, scene

pytestmark = pytest.mark.gpu
FORWARD = {"k_uv_fill_fuse_tile", "k_uv_fill_top", "k_uv_fill_push_tile"}
TILE, VIEWS = "k_uv_fill_adjoint_tile", "k_uv_fill_adjoint_views"


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _device_inputs(case):
    a = UF.case_inputs(case)
    return a["textures"].cuda(), a["weights"].cuda(), a["grad"].cuda(), a["background"].cuda()


def _check(result, ref, kind, what):
    assert result.shape == ref.shape and bool(torch.isfinite(result).all()), what
    err, allowed = UF.relative_error(result, ref), UF.DEVICE_TOLERANCE[kind]
    print(what, kind, "error / largest entry: %.2e" % err, "allowed: %.2e" % allowed)
    assert float(ref.abs().max()) > 0 and err <= allowed, (what, kind, err)


# ---- 1. texture, valid and the gradient, every case, with and without the fill ---------------------------------------------------
@pytest.mark.parametrize("fill", (True, False), ids=("fill", "plain"))
@pytest.mark.parametrize("case", UF.CASES, ids=UF.case_id)
def test_texture_valid_and_gradient_against_the_float64_reference(case, fill):
    from deep3dmap_amd import neural_renderer as nr
    name, H, W, B, C = case
    what = UF.case_id(case) + (" fill" if fill else " plain")
    ref = UF.reference(case, fill)
    x, w, g, bg = _device_inputs(case)
    x.requires_grad_(True)
    texture, valid = nr.fuse_uv_textures(x, w, fill, bg)
    assert texture.shape == (H, W, C) and valid.shape == (H, W) and not valid.requires_grad
    assert torch.equal(valid.cpu(), ref["valid"].float())
    texture.backward(g)
    _check(texture, ref["texture"], "texture", what)
    _check(x.grad, ref["textures_grad"], "textures_grad", what)
    # exactly +0 where a view does not count
    absent = ~(w > 0)
    assert not bool(_bits(x.grad)[absent].any())
    # without the fill: the torch formula on the device
    if not fill:
        wv = torch.where(w > 0, w, torch.zeros_like(w))
        want = (wv[..., None] * x.detach()).sum(0) / wv.sum(0).clamp(min=2.0 ** -100)[..., None]
        want = torch.where((valid > 0)[..., None], want, bg.expand_as(want))
        assert UF.relative_error(texture, want.cpu()) <= UF.DEVICE_TOLERANCE["texture"]
        assert torch.equal(_bits(texture)[valid == 0], _bits(bg.expand_as(texture))[valid == 0])


# ---- 2. what is exact on the device ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", UF.CASES, ids=UF.case_id)
def test_valid_texels_pass_through_bit_for_bit(case):
    from deep3dmap_amd import neural_renderer as nr
    x, w, g, bg = _device_inputs(case)
    filled, valid = nr.fuse_uv_textures(x, w, True, bg)
    plain, valid2 = nr.fuse_uv_textures(x, w, False, bg)
    on = valid > 0
    assert torch.equal(_bits(valid), _bits(valid2)) and torch.equal(_bits(filled)[on], _bits(plain)[on])


@pytest.mark.parametrize("case", (UF.CASES[0], UF.CASES[2]), ids=UF.case_id)
def test_one_view_of_weight_one_returns_the_input(case):
    from deep3dmap_amd import neural_renderer as nr
    x = _device_inputs(case)[0][:1].clone()
    x.view(-1)[::7] = -0.0
    for fill in (True, False):
        out, valid = nr.fuse_uv_textures(x, torch.ones_like(x[..., 0]), fill)
        assert bool((valid == 1).all()) and torch.equal(_bits(out), _bits(x[0]))


def test_no_valid_texel_gives_the_background_and_zero_gradients():
    from deep3dmap_amd import neural_renderer as nr
    x, w, g, bg = _device_inputs(UF.CASES[2])
    x.requires_grad_(True)
    texture, valid = nr.fuse_uv_textures(x, -w.abs(), True, bg)
    texture.backward(g)
    assert not bool(valid.any()) and torch.equal(_bits(texture), _bits(bg.expand_as(texture))) and not bool(_bits(x.grad).any())


def test_zero_and_non_finite_output_gradients():
    """g = 0: +0 everywhere.  A non-finite g at a valid texel reaches that texel's views only."""
    from deep3dmap_amd import neural_renderer as nr
    case = UF.CASES[2]
    x, w, g, bg = _device_inputs(case)
    x.requires_grad_(True)
    texture, valid = nr.fuse_uv_textures(x, w)
    grad, = torch.autograd.grad(texture, x, torch.zeros_like(g), retain_graph=True)
    assert not bool(_bits(grad).any())
    y, xx = (int(v) for v in (valid > 0).nonzero()[0])
    g = g.clone()
    g[y, xx, 0] = float("inf")
    grad, = torch.autograd.grad(texture, x, g)
    bad = ~torch.isfinite(grad)
    assert bool(bad[:, y, xx, 0][w[:, y, xx] > 0].all())
    bad[:, y, xx, 0] = False
    assert not bool(bad.any())


# ---- 3. the same bits on every run, eager and captured ---------------------------------------------------------------------------
def _step(nr, x, w, g, bg):
    texture, valid = nr.fuse_uv_textures(x, w, True, bg)
    return (texture, valid) + torch.autograd.grad(texture, (x,), g)


@pytest.mark.parametrize("case", (UF.CASES[2], UF.CASES[4]), ids=UF.case_id)
def test_two_runs_have_the_same_bits(case):
    from deep3dmap_amd import neural_renderer as nr
    x, w, g, bg = _device_inputs(case)
    runs = [_step(nr, x.clone().requires_grad_(True), w, g, bg) for _ in range(3)]
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(_bits(a), _bits(b))


def test_captured_forward_and_backward():
    from deep3dmap_amd import neural_renderer as nr
    from deep3dmap_amd.graph import CapturedStep
    case = UF.CASES[2]
    x, w, g, bg = _device_inputs(case)
    values = [x, torch.rand(x.shape, generator=torch.Generator().manual_seed(11)).cuda()]
    twin, live = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    eager = []
    for i in (0, 1):
        with torch.no_grad():
            twin.copy_(values[i])
        eager.append([t.clone() for t in _step(nr, twin, w, g, bg)])
    assert not torch.equal(eager[0][0], eager[1][0]) and float(eager[1][2].abs().max()) > 0
    torch.cuda.synchronize()
    cs = CapturedStep(lambda: _step(nr, live, w, g, bg)).capture()
    for i in (1, 0, 1):
        with torch.no_grad():
            live.copy_(values[i])
        got = [t.clone() for t in cs()]
        torch.cuda.synchronize()
        for a, b in zip(got, eager[i]):
            assert torch.equal(_bits(a), _bits(b)), i
    cs.release()


# ---- 4. launches ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,B,C,tiles", (((1, 1), 1, 1, 0), ((5, 7), 2, 3, 1), ((32, 32), 1, 9, 1), ((37, 50), 3, 9, 2),
                                            ((256, 256), 1, 1, 2), ((264, 300), 1, 2, 3), ((2048, 2048), 2, 1, 3)))
def test_launch_counts(size, B, C, tiles):
    """Forward 3, backward k_uv_fill_adjoint_tile once per three levels while a level exceeds 32 x 32 and once for the levels
    above, then k_uv_fill_adjoint_views: at most 4 either way up to 2048 x 2048, whatever B and C; without the fill 1 and 1."""
    from deep3dmap_amd import neural_renderer as nr
    H, W = size
    x = torch.rand(B, H, W, C, device="cuda").requires_grad_(True)
    w = (torch.rand(B, H, W, device="cuda") < 0.5).float()
    for fill in (True, False):
        with kernels_launched() as kf:
            texture, _ = nr.fuse_uv_textures(x, w, fill)
        assert {k: v[0] for k, v in kf.times.items()} == dict.fromkeys(FORWARD if fill else {"k_uv_fill_fuse_tile"}, 1)
        with kernels_launched() as kb:
            texture.backward(torch.ones_like(texture))
        want = {VIEWS: 1}
        if fill and tiles:
            want[TILE] = tiles
        got = {k: v[0] for k, v in kb.times.items()}
        assert got == want and sum(got.values()) <= 4, (got, want)
    with kernels_launched() as k:
        nr.fuse_uv_textures(x.detach(), w)
    assert sum(v[0] for v in k.times.values()) == 3


# ---- 5. the wrapper and the renderer -----------------------------------------------------------------------------------------------
def test_fill_uv_texture_is_the_node_with_one_view():
    from deep3dmap_amd import neural_renderer as nr
    x, w, g, bg = _device_inputs(UF.CASES[4])
    a = x[0].clone().requires_grad_(True)
    b = x.clone().requires_grad_(True)
    out = nr.fill_uv_texture(a, w[0], bg)
    want, _ = nr.fuse_uv_textures(b, w, True, bg)
    assert torch.equal(_bits(out), _bits(want))
    out.backward(g)
    want.backward(g)
    assert torch.equal(_bits(a.grad), _bits(b.grad[0]))


def _renderer_scene():
    from deep3dmap_amd import neural_renderer as nr
    case = UB.CASES[0]
    name, layout, T, S, aa, H, W, C, persp = case
    sc = scene(name)
    eyes = torch.from_numpy(sc["eyes"]).cuda()
    B = eyes.shape[0]
    r = nr.Renderer(camera_mode="look_at", image_size=image_size_of(S, aa), anti_aliasing=aa, viewing_angle=VIEWING_ANGLE,
                    perspective=persp)
    r.eye = eyes
    v = torch.from_numpy(sc["vertices"]).cuda()[None].repeat(B, 1, 1)
    faces = torch.from_numpy(sc["tri"]).cuda()[None]
    a = UB.case_inputs(case)
    return r, v, faces, a["images"].cuda(), a["faces_uv"].cuda(), T, B, C


def test_renderer_bake_fused_uv_texture():
    from deep3dmap_amd import neural_renderer as nr
    r, v, faces, images, faces_uv, T, B, C = _renderer_scene()
    baked, mask = r.bake_uv_texture(v, faces, images, faces_uv, T, background=0.5)
    assert 0 < int(mask.sum()) < mask.numel() and int(mask.sum(0).clamp(max=1).sum()) < T * T      # texels no view saw
    for fill in (True, False):
        texture, valid = r.bake_fused_uv_texture(v, faces, images, faces_uv, T, background=0.5, fill=fill)
        want, want_valid = nr.fuse_uv_textures(baked, mask, fill, 0.5)
        assert texture.shape == (T, T, C) and valid.shape == (T, T)
        assert torch.equal(_bits(texture), _bits(want)) and torch.equal(_bits(valid), _bits(want_valid))
    baked, mask = r.bake_uv_texture(v, faces, images, faces_uv, T)
    view_weights = torch.tensor([0.25, 1.0], device="cuda")[:B]
    texture, valid = r.bake_fused_uv_texture(v, faces, images, faces_uv, T, view_weights=view_weights)
    want, _ = nr.fuse_uv_textures(baked, mask * view_weights[:, None, None])
    assert torch.equal(_bits(texture), _bits(want))
    per_texel = torch.rand(B, T, T, device="cuda")
    texture, _ = r.bake_fused_uv_texture(v, faces, images, faces_uv, T, view_weights=per_texel)
    want, _ = nr.fuse_uv_textures(baked, mask * per_texel)
    assert torch.equal(_bits(texture), _bits(want))
    with pytest.raises(ValueError, match="view_weights"):
        r.bake_fused_uv_texture(v, faces, images, faces_uv, T, view_weights=torch.rand(B + 1, device="cuda"))


def test_photographs_to_a_mip_mapped_picture_end_to_end():
    """photographs -> bake -> fuse and fill -> sample_uv_texture(mipmap=True): the photographs' gradient is finite and not zero"""
    from deep3dmap_amd import neural_renderer as nr
    r, v, faces, images, faces_uv, T, B, C = _renderer_scene()
    images = images.clone().requires_grad_(True)
    texture, valid = r.bake_fused_uv_texture(v, faces, images, faces_uv, T)
    fr = r.fragments(v, faces)
    pictures, alpha = nr.sample_uv_texture(texture, faces_uv, fr, mipmap=True)
    assert bool(torch.isfinite(pictures).all()) and float(alpha.sum()) > 0
    pictures.square().sum().backward()
    assert bool(torch.isfinite(images.grad).all()) and float(images.grad.abs().max()) > 0
