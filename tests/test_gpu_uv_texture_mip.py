"""Mip-mapped per-pixel uv texture images on the device (neural_renderer/uv_texture_images.py with mipmap=,
csrc/d3m_uv_texture_mip.h): the forward and the level of detail against the float64 restatement evaluated on the device's own
maps, the pyramid bit for bit, the adjoint against float64 autograd within the derived bound, bit properties, neutrality
against the bilinear node, exact counts, the reach of the gradient, a captured step and the pass-through of the Renderer.
Restatement and bounds: tests/uv_texture_mip_scenes.py."""
import pytest
import torch

import uv_texture_mip_scenes as M
from conftest import kernels_launched
from test_gpu_uv_texture_images import _background, _bits, _case, _channels, _gradient
from uv_texture_image_scenes import seeded_image

pytestmark = pytest.mark.gpu
PYRAMID = {"k_texture_mip_tile"}
TAIL = {"k_texture_mip_tail"}                                        # levels above 5
LOOKUP = {"k_uv_texture_mip_images"}
BACKWARD = {"k_uv_texture_images_clear_max", "k_uv_texture_mip_images_scatter", "k_uv_texture_mip_images_convert"}
# the issue's cases with, taken together, each wrap, shared and per-view images, C in {1, 3, CHANNEL_CHUNK + 1}, aa off and on:
# (wrap, per view, index into _channels(), anti-aliasing)
SETTINGS = [("REPEAT", False, 1, False), ("MIRRORED_REPEAT", True, 2, True), ("CLAMP_TO_EDGE", False, 0, False),
            ("REPEAT", False, 1, False), ("CLAMP_TO_EDGE", True, 2, True), ("MIRRORED_REPEAT", True, 0, False)]
IDS = [f"{c[0]}-{c[1]}-{c[2][0]}x{c[2][1]}" for c in M.CASES]


def _forward_names(L):
    return PYRAMID | LOOKUP | (TAIL if L > 5 else set())


def _inputs(i):
    name, S, (H, W), spread, L = M.CASES[i]
    wrap, per_view, ci, aa = SETTINGS[i]
    c = _case(name, S, aa)
    C = _channels()[ci]
    uv = c["uv_seamless"] if spread == "seamless" else c["uv"]
    image = seeded_image(H, W, C, c["B"] if per_view else None)
    return c, uv, image, wrap, aa, L, C


# ---- 1. forward, level of detail, pyramid ---------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(M.CASES)), ids=IDS)
def test_forward_against_the_restatement(i):
    from deep3dmap_amd import neural_renderer as nr
    c, uv, image, wrap, aa, L, C = _inputs(i)
    fr, B, s = c["fr"], c["B"], c["s"]
    bg = _background(C)
    plain_alpha = nr.sample_uv_texture(image.cuda(), uv.cuda(), fr, wrap, bg.cuda())[1]
    runs = [(True, L, bias) for bias in M.LOD_BIASES] + ([(2, 2, 0.0)] if i == 0 else [])      # (mipmap=2: lambda_c = L, t = 1)
    for mipmap, levels, bias in runs:
        with kernels_launched() as k:
            images, alpha = nr.sample_uv_texture(image.cuda(), uv.cuda(), fr, wrap, bg.cuda(), mipmap=mipmap, lod_bias=bias)
        assert k.names == _forward_names(levels), k.names
        assert images.shape == (B, C, s, s) and alpha.shape == (B, s, s) and not alpha.requires_grad
        want, want_alpha = M.restate_mip_images(c["maps"], c["tri"], uv, image, bg, aa, wrap, levels, bias)
        bound = M.forward_bound(c["maps"], c["tri"], uv, image, bg, aa, wrap, levels, bias)
        err = (images.double().cpu() - want).abs()
        print(M.CASES[i], mipmap, bias, "largest error / bound:", float((err / bound.clamp(min=1e-300)).max()))
        assert bool((err <= bound).all()), (mipmap, bias, float((err / bound.clamp(min=1e-300)).max()))
        assert torch.equal(alpha.double().cpu(), want_alpha) and torch.equal(_bits(alpha), _bits(plain_alpha))
    if i == 0:
        lam = M.restate_lod(c["maps"], c["tri"], uv, tuple(image.shape[:2]), wrap, 0.0, 2)
        assert float((lam[c["maps"]["face_index_map"] >= 0] == 2).double().mean()) > 0.75    # mostly clamped at L: t = 1


@pytest.mark.parametrize("i", range(len(M.CASES)), ids=IDS)
def test_level_of_detail_against_the_restatement(i):
    from deep3dmap_amd import neural_renderer as nr
    c, uv, image, wrap, aa, L, C = _inputs(i)
    size = tuple(image.shape[-3:-1])
    S = c["maps"]["face_index_map"].shape[1]
    cov = c["maps"]["face_index_map"] >= 0
    for bias in M.LOD_BIASES:
        with kernels_launched() as k:
            lod = nr.uv_texture_lod(uv.cuda(), c["fr"], size, wrap, bias, levels=L)
        assert k.names == {"k_uv_texture_lod"}, k.names
        assert lod.shape == (c["B"], S, S) and not lod.requires_grad
        want = M.restate_lod(c["maps"], c["tri"], uv, size, wrap, bias, L)
        bound = M.lod_bound(c["maps"], c["tri"], uv, size, wrap, bias, L)
        err = (lod.double().cpu() - want).abs()
        print(M.CASES[i], bias, "lambda_c:", float(want[cov].min()), "...", float(want[cov].max()), "largest error:",
              float(err.max()), "largest bound:", float(bound.max()))
        assert bool((err <= bound).all()), float((err / bound.clamp(min=1e-300)).max())
        assert bool((_bits(lod).cpu()[~cov] == 0).all()) and float(bound[cov].median()) < 2.0 ** -10
    assert torch.equal(nr.uv_texture_lod(uv.cuda(), c["fr"], size, wrap), nr.uv_texture_lod(uv.cuda(), c["fr"], size, wrap, 0.0, L))


@pytest.mark.parametrize("H,W,C,L,batch", [(64, 64, 3, 6, None), (64, 64, 3, 2, None), (64, 32, 9, 5, 2), (8, 8, 1, 3, None),
                                           (48, 80, 3, 4, 2), (2, 6, 9, 1, None), (96, 160, 1, 5, None),
                                           (1024, 1024, 3, 10, None), (128, 64, 64, 6, 2)])
def test_pyramid_bit_for_bit(H, W, C, L, batch):
    """against float32 torch operators in the stated order: whole and clipped tiles, one and several channel chunks, levels
    inside the tile kernel only and beyond it"""
    from deep3dmap_amd import neural_renderer as nr
    image = seeded_image(H, W, C, batch)
    with kernels_launched() as k:
        levels = nr.texture_mip_pyramid(image.cuda().requires_grad_(True), L)
    assert k.names == PYRAMID | (TAIL if L > 5 else set()), k.names
    want = M.pyramid_levels(image, L)
    assert len(levels) == L + 1
    for got, ref in zip(levels, want):
        assert got.shape == ref.shape and not got.requires_grad
        assert torch.equal(_bits(got).cpu(), _bits(ref))


# ---- 2. adjoint -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(M.CASES)), ids=IDS)
def test_adjoint_against_float64_autograd(i):
    from deep3dmap_amd import neural_renderer as nr
    c, uv, image, wrap, aa, L, C = _inputs(i)
    fr, B, s = c["fr"], c["B"], c["s"]
    g = _gradient(C, B, s)
    runs = [(True, L, bias) for bias in M.LOD_BIASES] + ([(2, 2, 0.0)] if i == 0 else [])
    for mipmap, levels, bias in runs:
        a = image.cuda().requires_grad_(True)
        images, alpha = nr.sample_uv_texture(a, uv.cuda(), fr, wrap, _background(C).cuda(), mipmap=mipmap, lod_bias=bias)
        with kernels_launched() as k:
            images.backward(g.cuda())
        assert k.names == BACKWARD, k.names
        ref = M.adjoint64(c["maps"], c["tri"], uv, image, g, aa, wrap, levels, bias)
        assert float(ref.abs().max()) > 0 and a.grad.shape == image.shape
        bound = M.adjoint_bound(c["maps"], c["tri"], uv, tuple(image.shape), g, aa, wrap, levels, bias, ref)
        err = (a.grad.double().cpu() - ref).abs()
        print(M.CASES[i], mipmap, bias, "largest error / bound:", float((err / bound.clamp(min=1e-300)).max()))
        assert bool((err <= bound).all()), (mipmap, bias, float((err / bound.clamp(min=1e-300)).max()))
        reach = M.reach_counts(c["maps"], c["tri"], uv, tuple(image.shape), aa, wrap, levels, bias)
        assert bool((_bits(a.grad).cpu()[reach == 0] == 0).all())                             # +0 under no footprint


# ---- 3. bit properties ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [0, 1, 2], ids=IDS[:3])
def test_bit_properties(i):
    from deep3dmap_amd import neural_renderer as nr
    c, uv, _, wrap, aa, L, _ = _inputs(i)
    (H, W), C = M.CASES[i][2], _channels()[2]
    fr, B, s = c["fr"], c["B"], c["s"]
    uv = uv.cuda()
    g = _gradient(C, B, s).cuda()

    def grad_of(image, fragments, grad):
        a = image.cuda().requires_grad_(True)
        nr.sample_uv_texture(a, uv, fragments, wrap, mipmap=True, lod_bias=0.5)[0].backward(grad)
        return a.grad

    for per_view in (False, True):
        image = seeded_image(H, W, C, B if per_view else None)
        first = grad_of(image, fr, g)
        assert float(first.abs().max()) > 0
        assert torch.equal(_bits(first), _bits(grad_of(image, fr, g)))                    # two runs: the same bits
        assert torch.equal(_bits(grad_of(image, fr, g * 32.0)), _bits(first * 32.0))      # g 2^5: the result 2^5, exactly
        assert bool((_bits(grad_of(image, fr, torch.zeros_like(g))) == 0).all())          # g = 0: +0 everywhere
        poisoned = g.clone()
        poisoned[B - 1, C - 1, s // 2, s // 3] = float("inf")
        assert bool(torch.isnan(grad_of(image, fr, poisoned)).all())                     # one inf: NaN everywhere, no error
    if B > 1:                                                        # a shared image, the views in reverse order: the same bits
        image = seeded_image(H, W, C)
        rev = fr._replace(face_index_map=fr.face_index_map.flip(0).contiguous(), weight_map=fr.weight_map.flip(0).contiguous(),
                          depth_map=fr.depth_map.flip(0).contiguous(), faces=fr.faces.flip(0).contiguous())
        assert torch.equal(_bits(grad_of(image, rev, g.flip(0).contiguous())), _bits(grad_of(image, fr, g)))
    else:
        assert i == 2


# ---- 4. neutrality, exact counts, reach -------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [0, 4, 5], ids=[IDS[0], IDS[4], IDS[5]])
def test_level_zero_everywhere_is_the_bilinear_node(i):
    """lambda_c = 0 at every covered pixel -- a very negative lod_bias; a constant uv, whose rho2 is 0 or rounding noise, under
    any moderate bias --: l0 = 0, t = 0, level 1 is not read, and images and gradient have the bits of mipmap=None"""
    from deep3dmap_amd import neural_renderer as nr
    c, uv, image, wrap, aa, L, C = _inputs(i)
    fr, B, s = c["fr"], c["B"], c["s"]
    g, bg = _gradient(C, B, s).cuda(), _background(C).cuda()
    size = tuple(image.shape[-3:-1])
    point = torch.full_like(uv, 0.3125)
    for faces_uv, bias in ((uv, -64.0), (point, 8.0), (point, 0.0)):
        assert bool((nr.uv_texture_lod(faces_uv.cuda(), fr, size, wrap, bias) == 0).all())
        out = []
        for mipmap in (None, True):
            a = image.cuda().requires_grad_(True)
            images, alpha = nr.sample_uv_texture(a, faces_uv.cuda(), fr, wrap, bg, mipmap=mipmap, lod_bias=bias)
            images.backward(g)
            out.append((images, alpha, a.grad))
        assert float(out[0][2].abs().max()) > 0
        for plain, mip in zip(*out):
            assert torch.equal(_bits(plain), _bits(mip))


@pytest.mark.parametrize("aa", [False, True])
def test_exact_counts(aa):
    """g = 1 with lambda_c = L everywhere (spread uv under lod_bias = 64; with every uv at one point rho2 is 0 and the stated
    rule sends lambda to 0, the case of the test above): l0 = L - 1, t = 1, and level L is one texel whose single tap has
    weight 1, so every term is 1 (or 1/4), the top accumulator counts the covered pixels and every level-0 texel receives
    covered scale / 4^L exactly: / 16 on a 4 x 4 texture, / 4 on 2 x 2, / 256 on 16 x 16."""
    from deep3dmap_amd import neural_renderer as nr
    c = _case("S3", 128, aa)
    fr, B, s = c["fr"], c["B"], c["s"]
    covered = int((c["maps"]["face_index_map"] >= 0).sum())
    want = covered * (0.25 if aa else 1.0)
    g = torch.ones(B, 3, s, s).cuda()
    for (H, W), L, wrap in (((4, 4), 2, "REPEAT"), ((2, 2), 1, "MIRRORED_REPEAT"), ((16, 16), 4, "REPEAT")):
        assert bool((nr.uv_texture_lod(c["uv"].cuda(), fr, (H, W), wrap, 64.0, levels=L)[fr.face_index_map >= 0] == L).all())
        a = torch.rand(H, W, 3).cuda().requires_grad_(True)
        nr.sample_uv_texture(a, c["uv"].cuda(), fr, wrap, mipmap=L, lod_bias=64.0)[0].backward(g)
        assert a.grad.cpu().flatten().tolist() == [want / 4 ** L] * (H * W * 3)


def test_gradient_reaches_the_footprint():
    """S3 at S = 128 with the 1024 x 1024 seamless texture (lambda between 2.2 and 3.2): the bilinear node's gradient is
    non-zero at four texels per pixel at most, the mip-mapped one's at every texel under the eight taps' ancestors' blocks --
    no fewer than 3 x as many (on the CPU oracle's maps: 196 992 against 39 015)."""
    from deep3dmap_amd import neural_renderer as nr
    c = _case("S3", 128, False)
    fr, B, s = c["fr"], c["B"], c["s"]
    image, uv = seeded_image(1024, 1024, 1), c["uv_seamless"].cuda()
    g = _gradient(1, B, s).cuda()
    counts = []
    for mipmap in (None, True):
        a = image.cuda().requires_grad_(True)
        nr.sample_uv_texture(a, uv, fr, "REPEAT", mipmap=mipmap)[0].backward(g)
        counts.append(int((a.grad != 0).sum()))
    print("texels with a non-zero gradient: bilinear", counts[0], "mip-mapped", counts[1])
    assert counts[0] > 0 and counts[1] >= 3 * counts[0]


# ---- 5. capture, pass-through, refusals -------------------------------------------------------------------------------------
def test_captured_forward_and_backward():
    """Forward plus backward under torch.cuda.graph (CapturedStep: the step's own stream), replayed with the image and the
    gradient rewritten in place; the replay has the bits of the eager run (test_gpu_uv_texture_images.py's, with a pyramid of
    six levels: both pyramid kernels are in the graph)."""
    from deep3dmap_amd import neural_renderer as nr
    from deep3dmap_amd.graph import CapturedStep
    c = _case("S1", 32, True)
    fr, C, (H, W) = c["fr"], _channels()[2], (64, 64)
    uv, bg = c["uv"].cuda(), _background(C).cuda()
    images_in = [seeded_image(H, W, C, seed=sd).cuda() for sd in (31, 32)]
    grads_in = [_gradient(C, c["B"], c["s"], seed=sd).cuda() for sd in (17, 18)]
    twin = images_in[0].clone().requires_grad_(True)
    live = images_in[0].clone().requires_grad_(True)
    g_twin, g_live = grads_in[0].clone(), grads_in[0].clone()

    def step(image, g):
        images, alpha = nr.sample_uv_texture(image, uv, fr, "MIRRORED_REPEAT", bg, mipmap=True, lod_bias=1.5)
        grad, = torch.autograd.grad(images, image, g)
        return images, alpha, grad

    eager = []
    for i in (0, 1):
        with torch.no_grad():
            twin.copy_(images_in[i])
            g_twin.copy_(grads_in[i])
        with kernels_launched() as k:
            eager.append([t.clone() for t in step(twin, g_twin)])
        assert k.names == _forward_names(6) | BACKWARD, k.names      # nothing but the node's own kernels
    assert not torch.equal(eager[0][0], eager[1][0]) and not torch.equal(eager[0][2], eager[1][2])
    assert float(eager[1][2].abs().max()) > 0
    torch.cuda.synchronize()
    cs = CapturedStep(lambda: step(live, g_live)).capture()
    for i in (1, 0):
        with torch.no_grad():
            live.copy_(images_in[i])
            g_live.copy_(grads_in[i])
        got = [t.clone() for t in cs()]
        torch.cuda.synchronize()
        for a, b in zip(got, eager[i]):
            assert torch.equal(_bits(a), _bits(b)), i
    cs.release()


def test_renderer_passes_mipmap_through():
    from deep3dmap_amd import neural_renderer as nr
    c = _case("S2", 32, True)
    image, uv = seeded_image(64, 32, 3).cuda(), c["uv"].cuda()
    fr = c["r"].fragments(c["v"], c["faces"])
    for mipmap, bias in ((True, 0.0), (2, 1.5), (None, 0.0)):
        via = c["r"].render_uv_texture(c["v"], c["faces"], image, uv, "MIRRORED_REPEAT", 0.5, mipmap=mipmap, lod_bias=bias)
        direct = nr.sample_uv_texture(image, uv, fr, "MIRRORED_REPEAT", 0.5, mipmap=mipmap, lod_bias=bias)
        assert torch.equal(_bits(via[0]), _bits(direct[0])) and torch.equal(_bits(via[1]), _bits(direct[1]))
    plain = nr.sample_uv_texture(image, uv, fr, "MIRRORED_REPEAT", 0.5)[0]
    assert torch.equal(_bits(plain), _bits(direct[0]))              # (mipmap=None: the bilinear node)
    assert not torch.equal(plain, c["r"].render_uv_texture(c["v"], c["faces"], image, uv, "MIRRORED_REPEAT", 0.5, mipmap=True)[0])


def test_refusals():
    from deep3dmap_amd import neural_renderer as nr
    c = _case("S1", 16, False)
    fr = c["fr"]
    image, uv = torch.rand(8, 4, 3).cuda(), c["uv"].cuda()
    with kernels_launched() as k:
        with pytest.raises(ValueError, match="odd"):
            nr.sample_uv_texture(torch.rand(7, 4, 3).cuda(), uv, fr, mipmap=True)
        with pytest.raises(ValueError, match="mipmap"):
            nr.sample_uv_texture(image, uv, fr, mipmap=3)
        with pytest.raises(ValueError, match="lod_bias"):
            nr.sample_uv_texture(image, uv, fr, mipmap=True, lod_bias=float("nan"))
        with pytest.raises(NotImplementedError, match="faces_uv"):
            nr.sample_uv_texture(image, uv.clone().requires_grad_(True), fr, mipmap=True)
        with pytest.raises(ValueError, match="device"):
            nr.sample_uv_texture(image.cpu(), uv, fr, mipmap=True)
        with pytest.raises(ValueError, match="device"):
            nr.uv_texture_lod(uv.cpu(), fr, (8, 4))
        with pytest.raises(ValueError):
            nr.texture_mip_pyramid(image, 3)
        with pytest.raises(ValueError, match="GPU"):
            nr.texture_mip_pyramid(image.cpu(), 2)
    assert not k.names, k.names
