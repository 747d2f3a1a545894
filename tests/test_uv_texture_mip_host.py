"""Mip-mapped per-pixel uv texture images (neural_renderer/uv_texture_images.py with mipmap=, csrc/d3m_uv_texture_mip.h), host
side, on the CPU oracle's maps: the restatement (tests/uv_texture_mip_scenes.py) pinned analytically -- a constant image, an
affine image at every level of detail, the one level of detail of a planar scene --, its adjoint, the bound shown not to be
vacuous on every case, the adjoint's number format emulated in numpy, the level count mipmap=True picks, every refusal that
needs no device, and the new kernels' resource usage."""
import math

import numpy as np
import pytest
import torch

import uv_texture_mip_scenes as M
from test_uv_texture_images_host import _host_fragments
from uv_texture_image_scenes import restate_uv_texture_images, seeded_faces_uv, seeded_image
from vertex_attribute_scenes import oracle_maps, scene


def _case_inputs(name, S, size, spread, C=3, batch=None):
    return oracle_maps(name, S), scene(name)["tri"], seeded_faces_uv(name, spread)[0], seeded_image(size[0], size[1], C, batch)


# ---- 1. the analytic pins of the restatement ------------------------------------------------------------------------------
def test_constant_image():
    """A constant gives that constant at every level exactly (float32 and float64: c + c, 2c + c, 3c + c and the quarter are
    exact for c = 0.75, -2) and in the picture to the float64 roundings of the eight weights (they sum to 1 to 1e-15)."""
    sc, maps = scene("S2"), oracle_maps("S2", 16)
    faces_uv, _ = seeded_faces_uv("S2", "corners")
    value, bg = torch.tensor([0.75, -2.0]), torch.tensor([0.125, 4.0])
    image = value.expand(16, 8, 2).contiguous()
    for dtype in (torch.float32, torch.float64):
        levels = M.pyramid_levels(image.to(dtype), 3)
        assert [tuple(lv.shape) for lv in levels] == [(16, 8, 2), (8, 4, 2), (4, 2, 2), (2, 1, 2)]
        assert all(torch.equal(lv, value.to(dtype).expand_as(lv)) for lv in levels)
    cov = (maps["face_index_map"] >= 0).flip(1)
    want = torch.where(cov[:, None], value.double()[None, :, None, None], bg.double()[None, :, None, None])
    for bias in (-8.0, 0.0, 1.5, 8.0):
        got, alpha = M.restate_mip_images(maps, sc["tri"], faces_uv, image, bg, False, "REPEAT", 3, bias)
        assert torch.equal(alpha, cov.double()) and 0 < int(cov.sum()) < cov.numel()
        assert float((got - want).abs().max()) <= 1e-12


@pytest.mark.parametrize("anti_aliasing", [False, True])
def test_affine_image_at_every_level_of_detail(anti_aliasing):
    """image = a + b x + c y on 64 x 64 with every corner uv in [0.25, 0.75] and L = 5: pos lies in [15.75, 47.25], so no
    level's position meets its clamp ((pos + 0.5) 2^-5 - 0.5 >= 0.0078) and every level reproduces the affine function (a
    texel of level l sits at the centre of the block it averages): whatever lambda_c is, the picture is the bilinear one's.
    This checks the level positions: half a texel off at level 1 would show as |b| / 2."""
    S = 32 if anti_aliasing else 16
    sc, maps = scene("S2"), oracle_maps("S2", S)
    F = sc["tri"].shape[0]
    faces_uv = (0.25 + 0.5 * torch.rand(F, 3, 2, generator=torch.Generator().manual_seed(3))).contiguous()
    a = torch.tensor([0.5, -1.25, 2.0], dtype=torch.float64)
    b = torch.tensor([0.25, 1.5, -0.75], dtype=torch.float64)
    c = torch.tensor([-1.0, 0.125, 0.5], dtype=torch.float64)
    x = torch.arange(64, dtype=torch.float64)[None, :, None]
    y = torch.arange(64, dtype=torch.float64)[:, None, None]
    image = a + b * x + c * y
    bg = torch.tensor([0.25, 0.5, 0.75], dtype=torch.float64)
    want, want_alpha = restate_uv_texture_images(maps, sc["tri"], faces_uv, image, bg, anti_aliasing, "CLAMP_TO_EDGE",
                                                 torch.float64)
    seen = set()
    for bias in (-8.0, -2.0, 0.0, 1.5, 3.0, 8.0):
        lam = M.restate_lod(maps, sc["tri"], faces_uv, (64, 64), "CLAMP_TO_EDGE", bias, 5)
        seen |= set(lam[maps["face_index_map"] >= 0].floor().long().tolist())
        got, alpha = M.restate_mip_images(maps, sc["tri"], faces_uv, image, bg, anti_aliasing, "CLAMP_TO_EDGE", 5, bias)
        bound = M.forward_bound(maps, sc["tri"], faces_uv, image.float(), bg, anti_aliasing, "CLAMP_TO_EDGE", 5, bias)
        assert torch.equal(alpha, want_alpha)
        assert bool(((got - want).abs() <= bound).all()), (bias, float(((got - want).abs() / bound.clamp(min=1e-300)).max()))
        assert float(bound.max()) < 1e-2 * float(b.abs().max())      # (far below half a texel's step)
    assert seen == {0, 1, 2, 3, 4, 5}, seen


@pytest.mark.parametrize("S,size", [(16, (64, 64)), (32, (64, 64)), (16, (8, 8))])
def test_planar_scene_has_one_level_of_detail(S, size):
    """perspective=False, a flat patch seen along z, u = (x + 0.8) / 1.6 and v = (y + 0.8) / 1.6 of the vertex: the patch spans
    0.8 S pixels (NDC x is the world's; a pixel is 2 / S of NDC), so a pixel steps (size - 1) / (0.8 S) texels on both axes
    and lambda = log2((size - 1) / (0.8 S)) at every covered pixel."""
    sc = scene("planar")
    maps = oracle_maps("planar", S, perspective=False)
    tri = torch.from_numpy(sc["tri"]).long()
    vertex_uv = torch.from_numpy((sc["vertices"][:, :2] + 0.8) / 1.6).float()
    faces_uv = vertex_uv[tri].contiguous()
    L = 3
    lam = M.restate_lod(maps, sc["tri"], faces_uv, size, "CLAMP_TO_EDGE", 0.0, L)
    cov = maps["face_index_map"] >= 0
    want = math.log2((size[0] - 1) / (0.8 * S))
    assert int(cov.sum()) > 50
    assert float((lam[cov] - min(max(want, 0.0), L)).abs().max()) <= 1e-5, (want, lam[cov].min(), lam[cov].max())
    assert bool((lam[~cov] == 0).all())
    raw = 0.5 * torch.log2(M._rho2(maps, sc["tri"], faces_uv, size[0], size[1], "CLAMP_TO_EDGE", torch.float64)[0])
    assert float((raw[cov] - want).abs().max()) <= 1e-5             # (the float32 maps' own rounding)
    assert float(M.lod_bound(maps, sc["tri"], faces_uv, size, "CLAMP_TO_EDGE", 0.0, L)[cov].max()) < 2.0 ** -10


def test_level_of_detail_rules():
    """a constant uv: rho2 is 0 or the rounding noise of the weights' sum, its log2 -inf or far below -8, lambda_c = 0 under
    a bias of 8; a huge bias on spread uv: lambda_c = L"""
    sc, maps = scene("S1"), oracle_maps("S1", 16)
    F = sc["tri"].shape[0]
    cov = maps["face_index_map"] >= 0
    point = torch.full((F, 3, 2), 0.5)
    assert bool((M.restate_lod(maps, sc["tri"], point, (4, 4), "REPEAT", 8.0, 2) == 0).all())
    uv = seeded_faces_uv("S1", "corners")[0]
    assert bool((M.restate_lod(maps, sc["tri"], uv, (4, 4), "REPEAT", 64.0, 2)[cov] == 2).all())
    assert bool((M.restate_lod(maps, sc["tri"], uv, (4, 4), "REPEAT", -64.0, 2) == 0).all())


# ---- 2. the bound is not vacuous ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lod_bias", M.LOD_BIASES)
@pytest.mark.parametrize("name,S,size,spread,L", M.CASES)
def test_a_shift_of_the_level_of_detail_violates_the_forward_bound(name, S, size, spread, L, lod_bias):
    """lambda shifted by 2^-6 in the float64 restatement leaves the forward bound at more than half of the covered pixels with
    0 < lambda_c < L, on every case that has such pixels."""
    maps, tri, faces_uv, image = _case_inputs(name, S, size, spread)
    inside = M.interior_lod(maps, tri, faces_uv, size, "REPEAT", lod_bias, L)
    n = int(inside.sum())
    assert n > 0, "every case of the table has interior pixels at both biases"
    out = M.restate_mip_images(maps, tri, faces_uv, image, None, False, "REPEAT", L, lod_bias)[0]
    shifted = M.restate_mip_images(maps, tri, faces_uv, image, None, False, "REPEAT", L, lod_bias, lod_shift=2.0 ** -6)[0]
    bound = M.forward_bound(maps, tri, faces_uv, image, None, False, "REPEAT", L, lod_bias)
    violated = ((out - shifted).abs() > bound).any(1).flip(1)       # back in map orientation
    share = int((violated & inside).sum()) / n
    print(name, S, size, lod_bias, "interior pixels:", n, "of", int((maps["face_index_map"] >= 0).sum()), "violating:", share)
    assert share > 0.5


# ---- 3. the adjoint -------------------------------------------------------------------------------------------------------
def test_adjoint_reference_is_the_adjoint_of_the_restatement():
    maps, tri, faces_uv, _ = _case_inputs("S2", 16, (64, 32), "corners")
    g = torch.randn(2, 3, 16, 16, generator=torch.Generator().manual_seed(1))
    for batch in (None, 2):
        image = seeded_image(64, 32, 3, batch)
        ref = M.adjoint64(maps, tri, faces_uv, image, g, False, "REPEAT", 5, 0.0)
        assert ref.shape == image.shape and float(ref.abs().max()) > 0
        out = M.restate_mip_images(maps, tri, faces_uv, image.double(), None, False, "REPEAT", 5, 0.0)[0]
        assert abs(float((out * g.double()).sum()) - float((image.double() * ref).sum())) <= 1e-9       # the map is linear


@pytest.mark.parametrize("name,S,size,spread,L,aa,batched", [("S1", 16, (64, 64), "corners", 6, False, False),
                                                             ("S2", 32, (64, 32), "corners", 5, True, True),
                                                             ("S1", 32, (8, 8), "corners", 3, False, False)])
def test_emulated_adjoint_is_order_independent_and_within_its_bound(name, S, size, spread, L, aa, batched):
    """quantise per term, integer sums per level, the conversion in level order: the same integers and the same float32 bits
    for every order of the pixels, within adjoint_bound of the float64 autograd; g 2^5 gives the result 2^5 exactly."""
    maps, tri, faces_uv, _ = _case_inputs(name, S, size, spread)
    B = maps["face_index_map"].shape[0]
    image = seeded_image(size[0], size[1], 3, B if batched else None)
    s = S // 2 if aa else S
    g = torch.randn(B, 3, s, s, generator=torch.Generator().manual_seed(7))
    for bias in M.LOD_BIASES:
        acc, result = M.emulate_adjoint(maps, tri, faces_uv, tuple(image.shape), g, aa, "MIRRORED_REPEAT", L, bias)
        for seed in range(2):
            order = np.random.default_rng(seed).permutation(B * S * S)
            acc2, result2 = M.emulate_adjoint(maps, tri, faces_uv, tuple(image.shape), g, aa, "MIRRORED_REPEAT", L, bias, order)
            assert np.array_equal(acc, acc2) and np.array_equal(result.view(np.int32), result2.view(np.int32))
        ref = M.adjoint64(maps, tri, faces_uv, image, g, aa, "MIRRORED_REPEAT", L, bias)
        bound = M.adjoint_bound(maps, tri, faces_uv, tuple(image.shape), g, aa, "MIRRORED_REPEAT", L, bias, ref)
        err = (torch.from_numpy(result).double() - ref).abs()
        assert float(ref.abs().max()) > 0 and bool((err <= bound).all()), float((err / bound.clamp(min=1e-300)).max())
        reach = M.reach_counts(maps, tri, faces_uv, tuple(image.shape), aa, "MIRRORED_REPEAT", L, bias)
        assert bool((torch.from_numpy(result)[reach == 0] == 0).all())
        acc32, result32 = M.emulate_adjoint(maps, tri, faces_uv, tuple(image.shape), g * 32.0, aa, "MIRRORED_REPEAT", L, bias)
        assert np.array_equal(acc, acc32) and np.array_equal(result32, result * np.float32(32))


# ---- 4. the level count and the refusals that need no device ----------------------------------------------------------------
def test_mipmap_true_picks_the_largest_level_count():
    from deep3dmap_amd.neural_renderer import uv_texture_images as ut
    assert ut.MAX_LEVEL == 15
    for (H, W), want in (((64, 64), 6), ((64, 32), 5), ((8, 8), 3), ((1024, 1024), 10), ((96, 64), 5), ((2, 6), 1),
                         ((32768, 32768), 15), ((12, 20), 2)):
        assert ut.mip_levels(H, W, True) == want == min((H & -H).bit_length() - 1, (W & -W).bit_length() - 1, 15)
    for H, W in ((7, 4), (4, 7), (1, 1)):
        with pytest.raises(ValueError, match="odd"):
            ut.mip_levels(H, W, True)
    assert ut.mip_levels(7, 4, None) == 0 and ut.mip_levels(7, 4, 0) == 0 and ut.mip_levels(7, 4, False) == 0
    assert ut.mip_levels(64, 32, 2) == 2 and ut.mip_levels(64, 32, 5) == 5
    for bad in (6, 16, -1):
        with pytest.raises(ValueError):
            ut.mip_levels(64, 32, bad)
    with pytest.raises(TypeError):
        ut.mip_levels(64, 32, 2.0)


def test_argument_errors():
    from deep3dmap_amd import neural_renderer as nr
    from deep3dmap_amd.neural_renderer import uv_texture_images as ut
    assert nr.texture_mip_pyramid is ut.texture_mip_pyramid and nr.uv_texture_lod is ut.uv_texture_lod
    fr = _host_fragments()
    image, uv = torch.rand(8, 4, 3), torch.rand(2, 3, 2)
    with pytest.raises(ValueError, match="odd"):
        nr.sample_uv_texture(torch.rand(5, 4, 3), uv, fr, mipmap=True)
    for bad in (3, 16, -1):
        with pytest.raises(ValueError, match="mipmap"):
            nr.sample_uv_texture(image, uv, fr, mipmap=bad)
    for bad in (1.0, "2"):
        with pytest.raises(TypeError, match="mipmap"):
            nr.sample_uv_texture(image, uv, fr, mipmap=bad)
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="lod_bias"):
            nr.sample_uv_texture(image, uv, fr, mipmap=2, lod_bias=bad)
    for bad in ("1", None, torch.zeros(()), True):
        with pytest.raises(TypeError, match="lod_bias"):
            nr.sample_uv_texture(image, uv, fr, mipmap=2, lod_bias=bad)
    # what the bilinear node refuses, the mip-mapped one refuses
    with pytest.raises(ValueError, match="CLAMP_TO_BORDER"):
        nr.sample_uv_texture(image, uv, fr, "CLAMP_TO_BORDER", mipmap=True)
    with pytest.raises(ValueError, match="faces_uv"):
        nr.sample_uv_texture(image, torch.rand(3, 3, 2), fr, mipmap=True)
    with pytest.raises(NotImplementedError, match="faces_uv"):
        nr.sample_uv_texture(image, uv.clone().requires_grad_(True), fr, mipmap=True)
    with pytest.raises(ValueError, match="background"):
        nr.sample_uv_texture(image, uv, fr, "REPEAT", torch.rand(2), mipmap=True)
    with pytest.raises(ValueError, match="GPU"):                     # everything on the host: nothing to run on
        nr.sample_uv_texture(image, uv, fr, mipmap=True, lod_bias=1.5)
    with pytest.raises(ValueError, match="GPU"):
        nr.sample_uv_texture(image, uv, fr, mipmap=2, lod_bias=-1)
    # texture_mip_pyramid
    for bad in (torch.rand(8, 4), torch.rand(8, 4, 65), torch.rand(8, 4, 0), torch.rand(0, 8, 4, 3)):
        with pytest.raises(ValueError):
            nr.texture_mip_pyramid(bad, 2)
    for bad in (image.double(), image.numpy()):
        with pytest.raises(TypeError):
            nr.texture_mip_pyramid(bad, 2)
    for bad in (0, 3, 16):
        with pytest.raises(ValueError):
            nr.texture_mip_pyramid(image, bad)
    for bad in (True, 2.0, None):
        with pytest.raises(TypeError):
            nr.texture_mip_pyramid(image, bad)
    with pytest.raises(ValueError, match="GPU"):
        nr.texture_mip_pyramid(image, 2)
    # uv_texture_lod
    with pytest.raises(TypeError):
        nr.uv_texture_lod(uv.double(), fr, (8, 4))
    with pytest.raises(ValueError, match="size"):
        nr.uv_texture_lod(uv, fr, 8)
    with pytest.raises(ValueError, match="size"):
        nr.uv_texture_lod(uv, fr, (8, 0))
    with pytest.raises(ValueError, match="odd"):
        nr.uv_texture_lod(uv, fr, (8, 5))
    with pytest.raises(ValueError):
        nr.uv_texture_lod(uv, fr, (8, 4), levels=3)
    with pytest.raises(ValueError):
        nr.uv_texture_lod(uv, fr, (8, 4), levels=0)
    with pytest.raises(ValueError, match="CLAMP_TO_BORDER"):
        nr.uv_texture_lod(uv, fr, (8, 4), "CLAMP_TO_BORDER")
    with pytest.raises(ValueError, match="faces_uv"):
        nr.uv_texture_lod(torch.rand(3, 3, 2), fr, (8, 4))
    with pytest.raises(ValueError, match="lod_bias"):
        nr.uv_texture_lod(uv, fr, (8, 4), lod_bias=float("nan"))
    with pytest.raises(ValueError, match="Fragments"):
        nr.uv_texture_lod(uv, tuple(fr), (8, 4))
    with pytest.raises(ValueError, match="GPU"):
        nr.uv_texture_lod(uv, fr, (8, 4), levels=2)
    import inspect
    sig = inspect.signature(nr.Renderer.render_uv_texture).parameters
    assert sig["mipmap"].default is None and sig["lod_bias"].default == 0.0


def test_entry_points_return_invalid_before_any_launch():
    import ctypes
    from deep3dmap_amd import _lib
    L = _lib.lib()
    p, q = ctypes.c_void_p(256), 256                                 # never dereferenced
    INVALID = 1
    fr_ok = dict(face_index_map=q, weight_map=q, depth_map=q, faces=q, tri=q, visibility=None, visibility_size=0,
                 batch_size=2, num_tri=2, fill_back=1, image_size=4, anti_aliasing=0)
    lod_ok = dict(fr=True, faces_uv=p, H=8, W=4, wrapping=0, levels=2, lod_bias=0.0, lod=p)
    fwd_ok = dict(fr=True, faces_uv=p, pyramid=p, image_batch=1, H=8, W=4, C=3, wrapping=0, levels=2, lod_bias=0.0,
                  background=None, images=p, alpha=p)
    bwd_ok = dict(fr=True, faces_uv=p, grad_images=p, image_batch=1, H=8, W=4, C=3, wrapping=0, levels=2, lod_bias=0.0,
                  scratch=p, scratch_bytes=1 << 30, grad_image=p)
    bad_fr = [dict(face_index_map=None), dict(weight_map=None), dict(depth_map=None), dict(faces=None), dict(tri=None),
              dict(batch_size=0), dict(num_tri=0), dict(image_size=0), dict(image_size=16385)]
    bad = [dict(fr=None), dict(faces_uv=None), dict(image_batch=3), dict(image_batch=0), dict(H=0), dict(W=0), dict(H=32769),
           dict(W=32769), dict(C=0), dict(C=65), dict(wrapping=3), dict(wrapping=-1), dict(wrapping=4), dict(levels=0),
           dict(levels=3), dict(levels=16), dict(levels=-1), dict(H=6), dict(W=6), dict(lod_bias=float("nan")),
           dict(lod_bias=float("inf"))]
    bad_lod = [dict(lod=None), dict(lod=ctypes.c_void_p(258))]
    bad_fwd = [dict(pyramid=None), dict(images=None), dict(alpha=None), dict(pyramid=ctypes.c_void_p(258))]
    need = L.d3m_uv_texture_mip_images_scratch_bytes(1, 8, 4, 3, 2, 2, 4)
    assert need == (32 + 8 + 2) * 3 * 8 + 1024 * 4
    bad_bwd = [dict(grad_images=None), dict(scratch=None), dict(grad_image=None), dict(scratch=ctypes.c_void_p(260)),
               dict(batch_size=5, image_size=16384, anti_aliasing=1), dict(scratch_bytes=need - 1), dict(scratch_bytes=0)]
    for ok, fn, more in ((lod_ok, L.d3m_uv_texture_lod, bad_lod), (fwd_ok, L.d3m_uv_texture_mip_images, bad_fwd),
                         (bwd_ok, L.d3m_uv_texture_mip_images_backward, bad_bwd)):
        for change in bad_fr + bad + more:
            if not (set(change) & (set(ok) | set(fr_ok))):
                continue                                             # (the level-of-detail entry takes no image batch or C)
            a = dict(ok, **{k: v for k, v in change.items() if k in ok})
            if a["fr"]:
                a["fr"] = ctypes.byref(_lib.D3MFragments(**dict(fr_ok, **{k: v for k, v in change.items() if k in fr_ok})))
            assert fn(*a.values(), None) == INVALID, (fn.__name__, change)
    pyr_ok = dict(image=p, image_batch=1, H=8, W=4, C=3, levels=2, pyramid=p)
    for change in (dict(image=None), dict(pyramid=None), dict(image=ctypes.c_void_p(258)), dict(image_batch=0), dict(H=0),
                   dict(W=0), dict(H=32769), dict(C=0), dict(C=65), dict(levels=0), dict(levels=3), dict(levels=16), dict(H=6)):
        assert L.d3m_texture_mip_pyramid(*dict(pyr_ok, **change).values(), None) == INVALID, change
    assert L.d3m_uv_texture_mip_images_scratch_bytes(2, 8, 4, 3, 2, 2, 4) == 2 * 42 * 3 * 8 + 1024 * 4
    assert L.d3m_uv_texture_mip_images_scratch_bytes(1, 64, 32, 1, 5, 2, 4) == (2048 + 512 + 128 + 32 + 8 + 2) * 8 + 1024 * 4
    for args in ((3, 8, 4, 3, 2, 2, 4), (1, 0, 4, 3, 2, 2, 4), (1, 8, 4, 65, 2, 2, 4), (1, 8, 4, 3, 2, 5, 32768),
                 (1, 8, 4, 3, 2, 0, 4), (1, 8, 4, 3, 3, 2, 4), (1, 8, 4, 3, 0, 2, 4), (1, 8, 4, 3, 16, 2, 4)):
        assert L.d3m_uv_texture_mip_images_scratch_bytes(*args) == 0, args


# ---- 5. resource usage ----------------------------------------------------------------------------------------------------
def test_new_kernels_use_no_scratch():
    from deep3dmap_amd.resource_usage import kernel_resource_usage
    import re
    short = {re.sub(r"^(void )?(d3m::)?", "", re.sub(r"\(.*$", "", k)): v for k, v in kernel_resource_usage().items()}
    new = {"k_texture_mip_tile", "k_texture_mip_tail", "k_uv_texture_lod", "k_uv_texture_mip_images",
           "k_uv_texture_mip_images_scatter", "k_uv_texture_mip_images_convert"}
    assert new <= set(short), set(short)
    table = {k: short[k] for k in new}
    assert all(v["scratch"] == 0 and not v["vgpr_spill"] for v in table.values()), table
    assert table["k_texture_mip_tile"]["lds"] == (1024 + 256 + 64 + 16 + 4 + 1) * 8 * 4
