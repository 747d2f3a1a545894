"""The lit sampler's texture_size == 2 branch (csrc/d3m_lit.h, sample_pixel_lit) on a scene where originals and fill_back
copies own neighbouring pixels, so that one wave samples both kinds: corner pn of an original reads texel rev(pn) (bits 0
and 2 of pn change places), corner pn of a copy reads texel pn.  The kernel places a face's eight texels in corner order once
per pixel; a wrong placement shows only where the two kinds meet in one wave, which the closed meshes of the other tests
(every owner an original) never produce.

Scene: synthetic.grid_mesh(12) with the vertex order of every second triangle reversed -- with fill_back the owner of a pixel
is then an original (face index < F) or a copy (>= F) from one triangle to the next -- eight distinct texels per face, a
directional light with coloured parts (the per-face light differs per channel and per face), three cameras on a ring.

Yardstick of the images: render() with lighting_on_the_fly against the materialised sequence cat -> lighting -> the generic
sampler, BIT-equal (DESIGN.md section 4.4 claims it; the parent of the commit that added this file is bit-equal at these
inputs too).  Yardstick of the fused objective (k_render_lit_fit_records<16>, <32> and _pooled): multiview_fit_loss on
render()'s images, at the tolerances of tests/test_gpu_renderer.py's fused-against-images tests."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 3
LIGHT = dict(light_direction=[0.3, 0.8, -0.5], light_color_directional=[1.0, 0.8, 0.6], light_color_ambient=[0.9, 1.0, 0.8],
             light_intensity_ambient=0.4, light_intensity_directional=0.6, background_color=[0.1, 0.2, 0.3])


def _scene(per_view):
    """(vertices [V,3], triangles [F,3] with every second one reversed, textures [1 or B,F,2,2,2,3], eyes [B,3]) on the GPU"""
    from deep3dmap_amd import synthetic
    v, tri = synthetic.grid_mesh(12)
    tri = tri.copy()
    tri[1::2] = tri[1::2, ::-1]
    tex = np.stack([synthetic.random_textures(tri.shape[0], 2, seed=1 + k) for k in range(B if per_view else 1)])
    assert all(len(np.unique(t.reshape(8, 3)[:, 0])) == 8 for t in tex[0][:16])
    eyes = torch.from_numpy(synthetic.camera_ring(B)).float().cuda()
    return torch.from_numpy(v).cuda(), torch.from_numpy(np.ascontiguousarray(tri)).int().cuda(), torch.from_numpy(tex).cuda(), eyes


def _renderer(size, eyes, aa=False):
    import deep3dmap_amd.neural_renderer as nr
    r = nr.Renderer(image_size=size, anti_aliasing=aa, camera_mode="look_at", fill_back=True, **LIGHT)
    r.eye = eyes
    return r


def _assert_both_kinds_own_pixels(r, v, tri):
    """a condition on the scene: originals and copies own at least 10 % of the covered pixels each"""
    fr = r.fragments(v[None].repeat(B, 1, 1), tri[None])
    fi = fr.face_index_map
    covered = int((fi >= 0).sum())
    F = tri.shape[0]
    originals, copies = int(((fi >= 0) & (fi < F)).sum()), int((fi >= F).sum())
    assert covered > 0 and originals >= 0.1 * covered and copies >= 0.1 * covered, (covered, originals, copies)
    # ... and they meet inside a wave's 64 consecutive pixels: neighbours in a row with owners of different kinds
    own, back = fi >= 0, fi >= F
    mixed = own[:, :, 1:] & own[:, :, :-1] & (back[:, :, 1:] != back[:, :, :-1])
    assert int(mixed.sum()) >= 0.05 * covered, (covered, int(mixed.sum()))


@pytest.mark.parametrize("per_view", [False, True])
@pytest.mark.parametrize("size", [16, 40])
def test_images_bit_equal_to_the_materialised_sequence(size, per_view):
    """render() through the fused sampler (k_render_lit_epilogue) == cat -> lighting -> k_texture_sampling, bit for bit"""
    v, tri, tex, eyes = _scene(per_view)
    _assert_both_kinds_own_pixels(_renderer(size, eyes), v, tri)
    res = []
    for fly in (False, True):
        r = _renderer(size, eyes)
        r.lighting_on_the_fly = fly
        n = 1 if (fly and not per_view) else B                   # the materialised sequence has no shared form
        vv = v[None].repeat(n, 1, 1)
        tt = tex if tex.shape[0] == n else tex.repeat(n, 1, 1, 1, 1, 1)
        with torch.no_grad():
            res.append(r(vv, tri[None].repeat(n, 1, 1), tt))
    (rgb0, depth0, alpha0), (rgb1, depth1, alpha1) = res
    assert 0.1 < float(alpha0.mean()) < 0.9
    assert torch.equal(alpha0, alpha1) and torch.equal(depth0, depth1)
    diff = (rgb0 - rgb1).abs()
    print("rgb: differing words", int((rgb0 != rgb1).sum()), "of", rgb0.numel(), "largest", float(diff.max()))
    assert torch.equal(rgb0, rgb1)


class _TileForm:
    """d3m_set_fit_tile_form for the block: -1 = by the launch's size, 0 = 16 x 16 tiles, 1 = 32 x 32"""
    def __init__(self, form):
        self.form = form

    def __enter__(self):
        from deep3dmap_amd import _lib
        self.old = _lib.lib().d3m_get_fit_tile_form()
        _lib.check(_lib.lib().d3m_set_fit_tile_form(self.form), "d3m_set_fit_tile_form")

    def __exit__(self, *exc):
        from deep3dmap_amd import _lib
        _lib.lib().d3m_set_fit_tile_form(self.old)


@pytest.mark.parametrize("per_view", [False, True])
@pytest.mark.parametrize("form", ["tile16", "tile32", "pooled"])
@pytest.mark.parametrize("size", [16, 40])
def test_fused_objective_matches_the_objective_of_the_images(size, form, per_view):
    """render_fit_loss (k_render_lit_fit_records<16> / <32>, and _pooled with anti-aliasing) against multiview_fit_loss on
    render()'s images: value to rtol 2e-6, vertex and texture gradients to 2e-5 of their largest entry"""
    from deep3dmap_amd.core import multiview_fit_loss
    from deep3dmap_amd import synthetic
    aa = form == "pooled"
    v, tri, tex, eyes = _scene(per_view)
    r = _renderer(size, eyes, aa)
    _assert_both_kinds_own_pixels(r, v, tri)
    n = B if per_view else 1
    tri_d = tri[None].repeat(n, 1, 1)
    with torch.no_grad():
        tv = torch.from_numpy(synthetic.perturb(v.cpu().numpy(), 0.04)).cuda()
        rgb_t, depth_t, alpha_t = r(tv[None].repeat(n, 1, 1), tri_d, tex)

    def run(inside):
        vv = v[None].repeat(n, 1, 1).requires_grad_(True)
        tt = tex.clone().requires_grad_(True)
        if inside:
            loss = r.render_fit_loss(vv, tri_d, tt, (rgb_t, depth_t, alpha_t, alpha_t))
        else:
            loss = multiview_fit_loss(*r(vv, tri_d, tt), rgb_t, depth_t, alpha_t, alpha_t)
        loss.backward()
        return loss.detach(), vv.grad, tt.grad

    with _TileForm({"tile16": 0, "tile32": 1, "pooled": -1}[form]):
        a, b = run(True), run(False)
    print("loss", float(a[0]), float(b[0]), "gradient deviations / largest entry",
          [float((ga - gb).abs().max() / gb.abs().max()) for ga, gb in zip(a[1:], b[1:])])
    assert float(b[0]) > 0 and torch.allclose(a[0], b[0], rtol=2e-6, atol=0)
    for ga, gb in zip(a[1:], b[1:]):
        assert float(gb.abs().max()) > 0
        assert float((ga - gb).abs().max()) <= 2e-5 * float(gb.abs().max())
