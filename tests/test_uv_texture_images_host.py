"""Per-pixel uv texture images (neural_renderer/uv_texture_images.py), host side, on the CPU oracle's maps: the element-wise
restatement (tests/uv_texture_image_scenes.py) pinned analytically -- an affine texture is an attribute image, a constant
texture a constant --, the adjoint's number format emulated in numpy (order independence, the error bound, exact scaling by
powers of two), every refusal that needs no device, and the new kernels' resource usage."""
import numpy as np
import pytest
import torch

from uv_texture_image_scenes import (WRAPS, adjoint64, fixed_point_sum, restate_uv_texture_images, seeded_faces_uv,
                                     seeded_image, wrap_uv)
from vertex_attribute_scenes import U32, oracle_maps, restate_attribute_images, scene


def _maps_with_exact_depth(maps):
    """The maps with depth_map recomputed in float64 as 1 / sum_c (w_c / z_c): the u_c = w_c (d / z_c) then sum to 1 to
    float64 rounding (the float32 depth_map leaves 1 +- 1e-7, which an affine texture's constant term would show)."""
    fi = maps["face_index_map"].long()
    B, S = fi.shape[:2]
    cov = fi >= 0
    bidx = torch.arange(B)[:, None, None].expand(B, S, S)
    z = maps["faces"][bidx, fi.clamp(min=0)][..., 2].double()
    z = torch.where(cov[..., None], z, torch.ones_like(z))
    d = 1.0 / (maps["weight_map"].double() / z).sum(-1)
    return dict(maps, depth_map=torch.where(cov, d, torch.ones_like(d)))


# ---- 1. the analytic pins of the restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S2", "planar"])
@pytest.mark.parametrize("anti_aliasing", [False, True])
def test_affine_texture_is_an_attribute_image(name, anti_aliasing):
    """image[y, x, :] = a + b x + c y with seamless uv under CLAMP_TO_EDGE: bilinear lookup reproduces an affine function, so
    the picture is the attribute image of the per-vertex attribute a + b u (W - 1) + c v (H - 1)."""
    S = 32 if anti_aliasing else 16
    sc = scene(name)
    maps = _maps_with_exact_depth(oracle_maps(name, S, perspective=name != "planar"))
    faces_uv, vertex_uv = seeded_faces_uv(name, "seamless")
    H, W = 7, 4
    a = torch.tensor([0.5, -1.25, 2.0], dtype=torch.float64)
    b = torch.tensor([0.25, 1.5, -0.75], dtype=torch.float64)
    c = torch.tensor([-1.0, 0.125, 0.5], dtype=torch.float64)
    x = torch.arange(W, dtype=torch.float64)[None, :, None]
    y = torch.arange(H, dtype=torch.float64)[:, None, None]
    image = a + b * x + c * y
    bg = torch.tensor([0.25, 0.5, 0.75], dtype=torch.float64)
    got, got_alpha = restate_uv_texture_images(maps, sc["tri"], faces_uv, image, bg, anti_aliasing, "CLAMP_TO_EDGE",
                                               torch.float64)
    uv = vertex_uv.double()
    attributes = a + b * (uv[:, 0:1] * (W - 1)) + c * (uv[:, 1:2] * (H - 1))
    want, want_alpha = restate_attribute_images(maps, sc["tri"], attributes, bg, anti_aliasing, torch.float64)
    scale = float((a.abs() + b.abs() * (W - 1) + c.abs() * (H - 1)).max())
    assert got.shape == want.shape and int((want_alpha > 0).sum()) > 50
    assert float((got - want).abs().max()) <= 1e-12 * scale
    assert torch.equal(got_alpha, want_alpha)


@pytest.mark.parametrize("wrapping", WRAPS)
def test_constant_texture(wrapping):
    sc = scene("S2")
    for S, aa in ((16, False), (32, True)):
        maps = oracle_maps("S2", S)
        faces_uv, _ = seeded_faces_uv("S2", "corners")
        value, bg = torch.tensor([0.75, -2.0]), torch.tensor([0.125, 4.0])
        image = value.expand(5, 3, 2)
        got, alpha = restate_uv_texture_images(maps, sc["tri"], faces_uv, image, bg, False, wrapping, torch.float64)
        cov = (maps["face_index_map"] >= 0).flip(1)
        assert torch.equal(alpha, cov.double()) and 0 < int(cov.sum()) < cov.numel()
        want = torch.where(cov[:, None], value.double()[None, :, None, None], bg.double()[None, :, None, None])
        assert float((got - want).abs().max()) <= 1e-12
        pooled, pooled_alpha = restate_uv_texture_images(maps, sc["tri"], faces_uv, image, bg, aa, wrapping, torch.float64)
        if aa:
            assert pooled.shape[-1] == S // 2 and float((pooled_alpha - cov.double().reshape(2, 16, 2, 16, 2).mean((2, 4))).abs().max()) == 0


def test_wrap_uv_folds_into_the_unit_interval():
    v = torch.tensor([-0.75, -0.25, 0.0, 0.25, 1.0, 1.25, 1.75])
    assert wrap_uv(v, "REPEAT").tolist() == [0.25, 0.75, 1.0, 0.25, 0.0, 0.25, 0.75]
    assert wrap_uv(v, "MIRRORED_REPEAT").tolist() == [0.75, 0.25, 0.0, 0.25, 1.0, 0.75, 0.25]
    assert wrap_uv(v, "CLAMP_TO_EDGE").tolist() == [0.0, 0.0, 0.0, 0.25, 1.0, 1.0, 1.0]


def test_adjoint_reference_is_the_adjoint_of_the_restatement():
    sc = scene("S2")
    maps = oracle_maps("S2", 16)
    faces_uv, _ = seeded_faces_uv("S2", "corners")
    g = torch.randn(2, 3, 16, 16, generator=torch.Generator().manual_seed(1))
    for batch in (None, 2):
        image = seeded_image(7, 4, 3, batch)
        ref = adjoint64(maps, sc["tri"], faces_uv, image, g, False, "REPEAT")
        assert ref.shape == image.shape and float(ref.abs().max()) > 0
        out, _ = restate_uv_texture_images(maps, sc["tri"], faces_uv, image.double(), None, False, "REPEAT", torch.float64)
        assert abs(float((out * g.double()).sum()) - float((image.double() * ref).sum())) <= 1e-9       # the map is linear


# ---- 2. the adjoint's number format, emulated -----------------------------------------------------------------------------
def test_fraction_bits():
    from deep3dmap_amd.neural_renderer.uv_texture_images import uv_adjoint_fraction_bits as frac
    assert frac(1, 1) == 62 and frac(1, 2) == 60 and frac(3, 1) == 60 and frac(5, 1) == 59
    assert frac(32, 512) == 39 and frac(32, 1024) == 37 and frac(2, 16) == 53 and frac(1, 128) == 48
    assert frac(65535, 256) == 30 and frac(65536, 256) == 30 and frac(4, 32768) == 30
    for B, S in ((65537, 256), (5, 32768), (65535, 16385)):
        with pytest.raises(ValueError, match="2\\^32"):
            frac(B, S)
    with pytest.raises(ValueError):
        frac(0, 4)


@pytest.mark.parametrize("n", [10, 1000, 200000])
def test_emulated_sum_is_order_independent_and_within_its_bound(n):
    """frac = 37 (32 views at S = 1024): terms w (scale g) with w in [0, 1] and |g| spread over six decades."""
    frac = 37
    rng = np.random.default_rng(n)
    g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 0, n)).astype(np.float32)
    w = rng.uniform(0, 1, n).astype(np.float32)
    terms = (w * g).astype(np.float32)
    gmax = float(np.abs(g).max())
    total, result = fixed_point_sum(terms, gmax, frac)
    for seed in range(3):
        shuffled = terms[np.random.default_rng(seed).permutation(n)]
        assert fixed_point_sum(shuffled, gmax, frac)[0] == total                      # the same integer
    exact = float(terms.astype(np.float64).sum())
    q = np.ldexp(1.0, int(np.floor(np.log2(gmax))) + 1 - frac)
    bound = n * q / 2 + U32 * float(np.abs(terms.astype(np.float64)).sum()) + U32 * abs(float(result))
    err = abs(float(result) - exact)
    assert err <= bound
    sequential = abs(float(np.cumsum(terms, dtype=np.float32)[-1]) - exact)          # (cumsum adds in sequence, in float32)
    print(n, "error:", err, "bound:", bound, "sequential float32 sum:", sequential)
    if sequential > n * q / 2 + U32 * abs(float(result)):            # (beyond the format's own quantisation and final rounding)
        assert err <= sequential                                     # smaller than a sequential float32 sum's
    assert abs(total) < 2 ** 62 and np.abs(terms).max() <= gmax
    # scaling g by 2^3 scales the result by exactly 2^3, with the same integer
    total8, result8 = fixed_point_sum((w * (g * np.float32(8))).astype(np.float32), 8 * gmax, frac)
    assert total8 == total and result8 == np.float32(8) * result


# ---- 3. refusals that need no device --------------------------------------------------------------------------------------
def _host_fragments(B=2, V=6, F=2, s=4, anti_aliasing=False, fill_back=True, device="cpu"):
    from deep3dmap_amd import neural_renderer as nr
    S = 2 * s if anti_aliasing else s
    Fp = 2 * F if fill_back else F
    e = dict(device=device)
    return nr.Fragments(torch.empty(B, S, S, dtype=torch.int32, **e), torch.empty(B, S, S, 3, **e), torch.empty(B, S, S, **e),
                        torch.empty(B, Fp, 3, 3, **e), torch.empty(64, dtype=torch.uint8, **e),
                        torch.empty(F, 3, dtype=torch.int32, **e), fill_back, s, anti_aliasing, V)


def test_argument_errors():
    from deep3dmap_amd import neural_renderer as nr
    from deep3dmap_amd.neural_renderer import uv_texture_images as ut
    assert nr.sample_uv_texture is ut.sample_uv_texture and ut.CHANNEL_CHUNK == 8 and ut.MAX_CHANNELS == 64
    assert hasattr(nr.Renderer, "render_uv_texture")
    fr = _host_fragments()
    image, uv = torch.rand(5, 4, 3), torch.rand(2, 3, 2)
    for bad in (torch.rand(5, 4), torch.rand(1, 2, 5, 4, 3), torch.rand(5, 4, 0), torch.rand(5, 4, 65), torch.rand(0, 4, 3),
                torch.rand(5, 0, 3), torch.rand(3, 5, 4, 3), torch.rand(1, 5, 4, 3)):
        with pytest.raises(ValueError):
            nr.sample_uv_texture(bad, uv, fr)
    for bad in (image.double(), image.half(), image.numpy()):
        with pytest.raises(TypeError):
            nr.sample_uv_texture(bad, uv, fr)
    with pytest.raises(TypeError):
        nr.sample_uv_texture(image, uv.double(), fr)
    for bad in (torch.rand(3, 3, 2), torch.rand(1, 3, 2), torch.rand(2, 3, 3), torch.rand(2, 6), torch.rand(4, 3, 2)):
        with pytest.raises(ValueError, match="faces_uv"):
            nr.sample_uv_texture(image, bad, fr)
    with pytest.raises(ValueError, match="CLAMP_TO_BORDER"):
        nr.sample_uv_texture(image, uv, fr, "CLAMP_TO_BORDER")
    with pytest.raises(ValueError, match="CLAMP_TO_BORDER"):
        nr.sample_uv_texture(image, uv, fr, 3)
    for bad in ("NEAREST", 4, -1):
        with pytest.raises(ValueError, match="texture_wrapping"):
            nr.sample_uv_texture(image, uv, fr, bad)
    with pytest.raises(ValueError, match="Fragments"):
        nr.sample_uv_texture(image, uv, tuple(fr))
    with pytest.raises(ValueError, match="fit"):
        nr.sample_uv_texture(image, uv, fr._replace(anti_aliasing=True))
    for bg in (torch.rand(3, requires_grad=True), torch.rand(2), torch.rand(3).double(), [1.0, 2.0]):
        with pytest.raises(ValueError, match="background"):
            nr.sample_uv_texture(image, uv, fr, "REPEAT", bg)
    with pytest.raises(NotImplementedError, match="faces_uv"):
        nr.sample_uv_texture(image, uv.clone().requires_grad_(True), fr)
    with pytest.raises(ValueError, match="GPU"):                     # everything on the host: nothing to run on
        nr.sample_uv_texture(image, uv, fr, "MIRRORED_REPEAT", 0.5)
    # B S S beyond 2^32: a record of 5 views at S = 32768 (shapes only: the meta device allocates nothing)
    big = _host_fragments(B=5, s=16384, anti_aliasing=True, device="meta")
    with pytest.raises(ValueError, match="2\\^32"):
        nr.sample_uv_texture(image, uv, big)


def test_entry_points_return_invalid_before_any_launch():
    import ctypes
    from deep3dmap_amd import _lib
    L = _lib.lib()
    p, q = ctypes.c_void_p(256), 256                                 # never dereferenced
    INVALID = 1
    fr_ok = dict(face_index_map=q, weight_map=q, depth_map=q, faces=q, tri=q, visibility=None, visibility_size=0,
                 batch_size=2, num_tri=2, fill_back=1, image_size=4, anti_aliasing=0)
    fwd_ok = dict(fr=True, faces_uv=p, image=p, image_batch=1, H=5, W=4, C=3, wrapping=0, background=None, images=p, alpha=p)
    bwd_ok = dict(fr=True, faces_uv=p, grad_images=p, image_batch=1, H=5, W=4, C=3, wrapping=0, scratch=p,
                  scratch_bytes=1 << 30, grad_image=p)
    bad_fr = [dict(face_index_map=None), dict(weight_map=None), dict(depth_map=None), dict(faces=None), dict(tri=None),
              dict(batch_size=0), dict(num_tri=0), dict(image_size=0), dict(image_size=16385)]
    bad = [dict(fr=None), dict(faces_uv=None), dict(image_batch=3), dict(image_batch=0), dict(H=0), dict(W=0), dict(H=32769),
           dict(W=32769), dict(C=0), dict(C=65), dict(wrapping=3), dict(wrapping=-1), dict(wrapping=4)]
    bad_fwd = [dict(image=None), dict(images=None), dict(alpha=None), dict(image=ctypes.c_void_p(258))]
    bad_bwd = [dict(grad_images=None), dict(scratch=None), dict(grad_image=None), dict(scratch=ctypes.c_void_p(260)),
               dict(batch_size=5, image_size=16384, anti_aliasing=1)]                   # (B S S = 5 * 2^30)
    for ok, fn, more in ((fwd_ok, L.d3m_uv_texture_images, bad_fwd), (bwd_ok, L.d3m_uv_texture_images_backward, bad_bwd)):
        for change in bad_fr + bad + more:
            a = dict(ok, **{k: v for k, v in change.items() if k in ok})
            if a["fr"]:
                a["fr"] = ctypes.byref(_lib.D3MFragments(**dict(fr_ok, **{k: v for k, v in change.items() if k in fr_ok})))
            assert fn(*a.values(), None) == INVALID, change
    need = L.d3m_uv_texture_images_scratch_bytes(1, 5, 4, 3, 2, 4)
    assert need == 5 * 4 * 3 * 8 + 1024 * 4
    assert L.d3m_uv_texture_images_scratch_bytes(2, 5, 4, 3, 2, 4) == 2 * 5 * 4 * 3 * 8 + 1024 * 4
    for args in ((3, 5, 4, 3, 2, 4), (1, 0, 4, 3, 2, 4), (1, 5, 4, 65, 2, 4), (1, 5, 4, 3, 5, 32768), (1, 5, 4, 3, 0, 4)):
        assert L.d3m_uv_texture_images_scratch_bytes(*args) == 0, args
    a = dict(bwd_ok, scratch_bytes=need - 1)
    a["fr"] = ctypes.byref(_lib.D3MFragments(**fr_ok))
    assert L.d3m_error_string(L.d3m_uv_texture_images_backward(*a.values(), None)) == b"workspace missing or too small"


# ---- 4. resource usage ----------------------------------------------------------------------------------------------------
def test_new_kernels_use_no_scratch():
    from deep3dmap_amd.resource_usage import kernel_resource_usage
    import re
    short = {re.sub(r"^(void )?(d3m::)?", "", re.sub(r"\(.*$", "", k)): v for k, v in kernel_resource_usage().items()}
    table = {k: v for k, v in short.items() if k.startswith("k_uv_texture")}
    names = set(table)
    assert {"k_uv_texture_images", "k_uv_texture_images_clear_max", "k_uv_texture_images_scatter",
            "k_uv_texture_images_convert"} <= names, names
    assert all(v["scratch"] == 0 and not v["vgpr_spill"] for v in table.values()), table
