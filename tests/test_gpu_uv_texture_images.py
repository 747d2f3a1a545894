"""Per-pixel uv texture images on the device (neural_renderer/uv_texture_images.py, csrc/d3m_uv_texture.h): the forward against
the float64 restatement evaluated on the device's own maps, alpha against interpolate_vertex_attributes' bit for bit, the
order-independent adjoint against float64 autograd within the derived bound, exact cases, bit properties, a captured step
and the refusals.  Scenes, restatement and bounds: tests/uv_texture_image_scenes.py."""
import itertools

import pytest
import torch

from conftest import kernels_launched
from uv_texture_image_scenes import (WRAPS, adjoint64, adjoint_bound, forward_bound, reach_counts, restate_uv_texture_images,
                                     seeded_faces_uv, seeded_image)
from vertex_attribute_scenes import VIEWING_ANGLE, fragment_maps, image_size_of, scene

pytestmark = pytest.mark.gpu
FM_MAX_BBOX_AREA = 4096     # csrc/d3m_face_major.h
FORWARD = {"k_uv_texture_images"}
BACKWARD = {"k_uv_texture_images_clear_max", "k_uv_texture_images_scatter", "k_uv_texture_images_convert"}
SCENE_CASES = [(n, S, aa) for n in ("S1", "S2", "S3") for S in scene(n)["sizes"] for aa in (False, True)]
TEXTURES = ((1, 1), (1, 5), (7, 4), (32, 32))


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _channels():
    from deep3dmap_amd.neural_renderer.uv_texture_images import CHANNEL_CHUNK
    return (1, 3, CHANNEL_CHUNK + 1)


def _combinations():
    """every texture size x channel count x wrap x (shared | per view)"""
    return itertools.product(TEXTURES, _channels(), WRAPS, (False, True))


_built = {}


def _case(name, S, aa):
    """The scene on the device, computed once: renderer, vertices [B,V,3], faces [1,F,3], the Fragments, its maps on the host."""
    from deep3dmap_amd import neural_renderer as nr
    key = (name, S, aa)
    if key not in _built:
        sc = scene(name)
        eyes = torch.from_numpy(sc["eyes"]).cuda()
        B = eyes.shape[0]
        r = nr.Renderer(camera_mode="look_at", image_size=image_size_of(S, aa), anti_aliasing=aa, viewing_angle=VIEWING_ANGLE)
        r.eye = eyes
        v = torch.from_numpy(sc["vertices"]).cuda()[None].repeat(B, 1, 1)
        faces = torch.from_numpy(sc["tri"]).cuda()[None]
        fr = r.fragments(v, faces)
        torch.cuda.synchronize()
        maps = fragment_maps(fr)
        _assert_scene_property(name, maps, sc["tri"].shape[0])
        _built[key] = dict(r=r, v=v, faces=faces, fr=fr, maps=maps, tri=sc["tri"], B=B, V=v.shape[1], s=image_size_of(S, aa),
                           uv=seeded_faces_uv(name, "corners")[0], uv_seamless=seeded_faces_uv(name, "seamless")[0])
    return _built[key]


def _assert_scene_property(name, maps, F):
    """what each scene is there for, on the device's own maps"""
    fi = maps["face_index_map"]
    owners = fi[fi >= 0]
    assert owners.numel() > 0 and int(owners.max()) < 2 * F
    if name == "S1":
        assert bool((owners >= F).all())                              # every owner is a reversed copy
    if name == "S2":
        assert bool((fi[0][fi[0] >= 0] < F).all()) and bool((fi[1][fi[1] >= 0] >= F).all())      # both owner kinds
    if name == "S3":
        assert int(torch.bincount(owners.long()).max()) > FM_MAX_BBOX_AREA                      # one face owns thousands


def _background(C):
    return torch.linspace(0.25, 1.5, C)


def _gradient(C, B, s, seed=17):
    return torch.randn(B, C, s, s, generator=torch.Generator().manual_seed(seed + C))


# ---- 1. forward -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,S,aa", SCENE_CASES)
def test_forward_against_the_restatement(name, S, aa):
    from deep3dmap_amd import neural_renderer as nr
    c = _case(name, S, aa)
    fr, B, s = c["fr"], c["B"], c["s"]
    attribute_alpha = nr.interpolate_vertex_attributes(torch.rand(c["V"], 1).cuda(), fr)[1]
    worst = 0.0
    for (H, W), C, wrap, per_view in _combinations():
        uv = c["uv_seamless"] if (wrap == "CLAMP_TO_EDGE" and C == 3) else c["uv"]
        image, bg = seeded_image(H, W, C, B if per_view else None), _background(C)
        with kernels_launched() as k:
            images, alpha = nr.sample_uv_texture(image.cuda(), uv.cuda(), fr, wrap, bg.cuda())
        assert k.names == FORWARD, k.names
        assert images.shape == (B, C, s, s) and alpha.shape == (B, s, s) and not alpha.requires_grad
        want, want_alpha = restate_uv_texture_images(c["maps"], c["tri"], uv, image, bg, aa, wrap, torch.float64)
        bound = forward_bound(c["maps"], c["tri"], uv, image, bg, aa, wrap)
        err = (images.double().cpu() - want).abs()
        worst = max(worst, float((err / bound.clamp(min=1e-300)).max()))
        assert bool((err <= bound).all()), (H, W, C, wrap, per_view, float((err / bound.clamp(min=1e-300)).max()))
        assert torch.equal(alpha.double().cpu(), want_alpha)
        assert torch.equal(_bits(alpha), _bits(attribute_alpha))
    print(name, S, aa, "largest error / bound:", worst)
    # Renderer.render_uv_texture is sample_uv_texture over Renderer.fragments; no background: zeros; a float: every channel
    image, uv = seeded_image(7, 4, 3).cuda(), c["uv"].cuda()
    via, via_alpha = c["r"].render_uv_texture(c["v"], c["faces"], image, uv, "MIRRORED_REPEAT", 0.5)
    direct, direct_alpha = nr.sample_uv_texture(image, uv, c["r"].fragments(c["v"], c["faces"]), "MIRRORED_REPEAT", 0.5)
    assert torch.equal(_bits(via), _bits(direct)) and torch.equal(_bits(via_alpha), _bits(direct_alpha))
    zero = nr.sample_uv_texture(image, uv, fr, "MIRRORED_REPEAT")[0]
    uncovered = (via_alpha == 0)[:, None].expand_as(zero)
    assert bool((zero[uncovered] == 0).all()) and bool((via[uncovered] == 0.5).all())


# ---- 2. adjoint -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,S,aa", SCENE_CASES)
def test_adjoint_against_float64_autograd(name, S, aa):
    from deep3dmap_amd import neural_renderer as nr
    c = _case(name, S, aa)
    fr, B, s = c["fr"], c["B"], c["s"]
    worst = 0.0
    for (H, W), C, wrap, per_view in _combinations():
        uv = c["uv_seamless"] if (wrap == "CLAMP_TO_EDGE" and C == 3) else c["uv"]
        image = seeded_image(H, W, C, B if per_view else None)
        g = _gradient(C, B, s)
        a = image.cuda().requires_grad_(True)
        images, alpha = nr.sample_uv_texture(a, uv.cuda(), fr, wrap, _background(C).cuda())
        with kernels_launched() as k:
            images.backward(g.cuda())
        assert k.names == BACKWARD, k.names
        ref = adjoint64(c["maps"], c["tri"], uv, image, g, aa, wrap)
        assert float(ref.abs().max()) > 0
        bound = adjoint_bound(c["maps"], c["tri"], uv, tuple(image.shape), g, aa, wrap, ref)
        err = (a.grad.double().cpu() - ref).abs()
        worst = max(worst, float((err / bound.clamp(min=1e-300)).max()))
        assert a.grad.shape == image.shape
        assert bool((err <= bound).all()), (H, W, C, wrap, per_view, float((err / bound.clamp(min=1e-300)).max()))
    print(name, S, aa, "largest error / bound:", worst)


# ---- 3. exact cases -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aa", [False, True])
def test_exact_counts(aa):
    """g = 1 everywhere: on a (1,1) texture every term is 1 (or 1/4), on a (1,5) texture with every uv at u = 0 likewise and
    all of them land on texel 0 -- small multiples of a power of two, so the sums are exact."""
    from deep3dmap_amd import neural_renderer as nr
    c = _case("S3", 128, aa)
    fr, B, s = c["fr"], c["B"], c["s"]
    covered = int((c["maps"]["face_index_map"] >= 0).sum())
    assert covered > FM_MAX_BBOX_AREA
    want = covered * (0.25 if aa else 1.0)
    g = torch.ones(B, 3, s, s).cuda()
    a = torch.rand(1, 1, 3).cuda().requires_grad_(True)
    nr.sample_uv_texture(a, c["uv"].cuda(), fr)[0].backward(g)
    assert a.grad.cpu().flatten().tolist() == [want] * 3
    a = torch.rand(1, 5, 3).cuda().requires_grad_(True)
    uv0 = torch.cat([torch.zeros_like(c["uv"][..., :1]), c["uv"][..., 1:]], -1)
    nr.sample_uv_texture(a, uv0.cuda(), fr, "CLAMP_TO_EDGE")[0].backward(g)
    assert a.grad[0, 0].cpu().tolist() == [want] * 3
    assert bool((_bits(a.grad[0, 1:]) == 0).all())


# ---- 4. bit properties ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,S,aa", [("S1", 16, False), ("S2", 32, True), ("S3", 128, False)])
def test_bit_properties(name, S, aa):
    from deep3dmap_amd import neural_renderer as nr
    c = _case(name, S, aa)
    fr, B, s = c["fr"], c["B"], c["s"]
    C, (H, W), wrap = _channels()[2], (32, 32), "REPEAT"
    uv = c["uv"].cuda()
    g = _gradient(C, B, s).cuda()

    def grad_of(image, fragments, grad):
        a = image.cuda().requires_grad_(True)
        nr.sample_uv_texture(a, uv, fragments, wrap)[0].backward(grad)
        return a.grad

    for per_view in (False, True):
        image = seeded_image(H, W, C, B if per_view else None)
        first = grad_of(image, fr, g)
        assert torch.equal(_bits(first), _bits(grad_of(image, fr, g)))                    # two runs: the same bits
        scaled = grad_of(image, fr, g * 32.0)                                            # g 2^5: the result 2^5, exactly
        assert torch.equal(_bits(scaled), _bits(first * 32.0))
        reach = reach_counts(c["maps"], c["tri"], c["uv"], tuple(image.shape), aa, wrap)
        unreached = (reach == 0).cuda()
        if name != "S3":
            assert int(unreached.sum()) > 0
        assert bool((_bits(first)[unreached] == 0).all())                                 # +0 where no sample reaches
        zero = grad_of(image, fr, torch.zeros_like(g))
        assert bool((_bits(zero) == 0).all())                                             # g = 0: +0 everywhere
        poisoned = g.clone()
        poisoned[B - 1, C - 1, s // 2, s // 3] = float("inf")
        assert bool(torch.isnan(grad_of(image, fr, poisoned)).all())                     # one inf: NaN everywhere, no error
    # a shared image, the views in reverse order: the same bits
    if B > 1:
        image = seeded_image(H, W, C)
        rev = fr._replace(face_index_map=fr.face_index_map.flip(0).contiguous(), weight_map=fr.weight_map.flip(0).contiguous(),
                          depth_map=fr.depth_map.flip(0).contiguous(), faces=fr.faces.flip(0).contiguous())
        assert torch.equal(_bits(grad_of(image, rev, g.flip(0).contiguous())), _bits(grad_of(image, fr, g)))


# ---- 5. capture -----------------------------------------------------------------------------------------------------------
def test_captured_forward_and_backward():
    """Forward plus backward under torch.cuda.graph (CapturedStep: the step's own stream), replayed with the image and the
    gradient rewritten in place; the replay has the bits of the eager run.  The captured step has a leaf of its own that no
    eager call touches (graph.py); the eager runs use a twin."""
    from deep3dmap_amd import neural_renderer as nr
    from deep3dmap_amd.graph import CapturedStep
    c = _case("S1", 32, True)
    fr, C, (H, W) = c["fr"], _channels()[2], (7, 4)
    uv, bg = c["uv"].cuda(), _background(C).cuda()
    images_in = [seeded_image(H, W, C, seed=sd).cuda() for sd in (31, 32)]
    grads_in = [_gradient(C, c["B"], c["s"], seed=sd).cuda() for sd in (17, 18)]
    twin = images_in[0].clone().requires_grad_(True)
    live = images_in[0].clone().requires_grad_(True)
    g_twin, g_live = grads_in[0].clone(), grads_in[0].clone()

    def step(image, g):
        images, alpha = nr.sample_uv_texture(image, uv, fr, "MIRRORED_REPEAT", bg)
        grad, = torch.autograd.grad(images, image, g)
        return images, alpha, grad

    eager = []
    for i in (0, 1):
        with torch.no_grad():
            twin.copy_(images_in[i])
            g_twin.copy_(grads_in[i])
        with kernels_launched() as k:
            eager.append([t.clone() for t in step(twin, g_twin)])
        assert k.names == FORWARD | BACKWARD, k.names                # nothing but the node's own kernels
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


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals():
    from deep3dmap_amd import neural_renderer as nr
    c = _case("S1", 16, False)
    fr, F = c["fr"], c["tri"].shape[0]
    image, uv = torch.rand(7, 4, 3).cuda(), c["uv"].cuda()
    with kernels_launched() as k:
        with pytest.raises(ValueError, match="CLAMP_TO_BORDER"):
            nr.sample_uv_texture(image, uv, fr, "CLAMP_TO_BORDER")
        for bad in (uv[:F - 1], torch.cat([uv, uv[:1]]), uv[:, :2], uv.reshape(F, 6)):
            with pytest.raises(ValueError, match="faces_uv"):
                nr.sample_uv_texture(image, bad, fr)
        with pytest.raises(NotImplementedError, match="faces_uv"):
            nr.sample_uv_texture(image, uv.clone().requires_grad_(True), fr)
        with pytest.raises(ValueError, match="device"):
            nr.sample_uv_texture(image.cpu(), uv, fr)
        with pytest.raises(ValueError, match="device"):
            nr.sample_uv_texture(image, uv.cpu(), fr)
        for bad in (image.double(), image.half()):
            with pytest.raises(TypeError):
                nr.sample_uv_texture(bad, uv, fr)
        for bad in (torch.rand(7, 4, 0).cuda(), torch.rand(7, 4, 65).cuda(), torch.rand(3, 7, 4, 3).cuda(), torch.rand(7, 4).cuda()):
            with pytest.raises(ValueError):
                nr.sample_uv_texture(bad, uv, fr)
        with pytest.raises(ValueError, match="background"):
            nr.sample_uv_texture(image, uv, fr, "REPEAT", torch.rand(3))                  # on the host
        with pytest.raises(ValueError):                                                  # per-view topology
            c["r"].render_uv_texture(c["v"], c["faces"].repeat(2, 1, 1), image, uv)
        with pytest.raises(NotImplementedError, match="detach them"):
            c["r"].render_uv_texture(c["v"].clone().requires_grad_(True), c["faces"], image, uv)
    assert not {n for n in k.names if n.startswith("k_uv_texture")}, k.names
