"""The interior geometry gradient on the device (neural_renderer/fragment_geometry.py, csrc/d3m_fragment_geometry.h):
fragment_weights' forward bit for bit and its adjoint against the float64 reference, the attribute and the uv texture node
with screen_vertices (the same bits of everything they returned before, and the vertices' gradient against the reference),
determinism, the Renderer's geometry_grad plumbing, and a captured step.  Reference, tolerance (DEVICE_TOLERANCE: 8 x the
float32 yardstick measured on the CPU) and the near-integer exclusion: tests/fragment_geometry_scenes.py."""
import pytest
import torch

import fragment_geometry_scenes as FG
from conftest import kernels_launched
from uv_texture_image_scenes import seeded_faces_uv, seeded_image
from vertex_attribute_scenes import (VIEWING_ANGLE, fragment_maps, image_size_of, pixel_weights, scene, seeded_attributes,
                                     seeded_background)

pytestmark = pytest.mark.gpu
FM_MAX_BBOX_AREA = 4096     # csrc/d3m_face_major.h
ADJOINT = {"k_fragment_geometry_face_sums", "k_fragment_geometry_large_face_sums", "k_vertex_attribute_adjoint_rows"}
CHUNKS = "k_vertex_attribute_adjoint_chunks"


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


_built = {}


def _case(name, S, aa):
    """The scene on the device, computed once: renderer, vertices [B,V,3], faces [1,F,3], the screen vertices the record was
    made from, the Fragments, its maps on the host."""
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
        sv = r._transform(v, None, None, None, None, None).detach().contiguous()
        fr = nr.rasterize_fragments(sv, faces, r.image_size, aa, r.fill_back, r.near, r.far)
        torch.cuda.synchronize()
        maps = fragment_maps(fr)
        if name == "S3B":                                             # the workgroup route, in both views
            assert B == 2
            for b in range(B):
                fi = maps["face_index_map"][b]
                assert int(torch.bincount(fi[fi >= 0].long()).max()) > FM_MAX_BBOX_AREA
        _built[key] = dict(r=r, v=v, faces=faces, sv=sv, fr=fr, maps=maps, tri=sc["tri"], B=B, V=v.shape[1],
                           s=image_size_of(S, aa), S=S)
    return _built[key]


def _check(grad, reference, what):
    """every element, per view in units of the view's largest reference entry"""
    assert grad.shape == reference.shape and bool(torch.isfinite(grad).all())
    errors = FG.view_errors(grad, reference)
    print(what, "per-view error / largest entry:", ["%.2e" % e for e in errors], "allowed: %.2e" % FG.DEVICE_TOLERANCE)
    assert float(reference.abs().max()) > 0 and max(errors) <= FG.DEVICE_TOLERANCE, (what, errors)


def _adjoint_names_ok(names, name, extra=frozenset()):
    want = ADJOINT | set(extra)
    return want <= names <= want | {CHUNKS} and (CHUNKS in names) == (name == "S4")


# ---- 1. fragment_weights, forward ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,S,aa", FG.scene_cases())
def test_fragment_weights_forward_is_the_maps_expression_bit_for_bit(name, S, aa):
    from deep3dmap_amd import neural_renderer as nr
    c = _case(name, S, aa)
    fr, B = c["fr"], c["B"]
    with kernels_launched() as k:
        u = nr.fragment_weights(fr, c["sv"])
    assert k.names == {"k_fragment_weights"}, k.names
    assert u.shape == (B, S, S, 3) and u.dtype == torch.float32 and not u.requires_grad
    cov = fr.face_index_map >= 0
    fn = fr.face_index_map.long().clamp(min=0)
    z = fr.faces[torch.arange(B, device="cuda")[:, None, None], fn][..., 2]                # [B,S,S,3]
    want = fr.weight_map * (fr.depth_map[..., None] / z)                                    # float32, element-wise
    assert int(cov.sum()) > 0 and torch.equal(_bits(u[cov]), _bits(want[cov]))
    assert bool((_bits(u[~cov]) == 0).all())                                                # an exact +0
    # the C entry point on a NaN-filled output: every element is written
    import ctypes
    from deep3dmap_amd import _lib
    raw = torch.full((B, S, S, 3), float("nan"), device="cuda")
    c_fr = fr.c_struct()
    _lib.check(_lib.lib().d3m_fragment_weights(ctypes.byref(c_fr), _lib.ptr(raw), _lib.stream_ptr()), "d3m_fragment_weights")
    assert torch.equal(_bits(raw), _bits(u))


# ---- 2. fragment_weights, backward --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,S,aa", FG.scene_cases())
def test_fragment_weights_backward_against_the_float64_reference(name, S, aa):
    from deep3dmap_amd import neural_renderer as nr
    c = _case(name, S, aa)
    fr, B = c["fr"], c["B"]
    gu = FG.seeded_grad_weights(B, S)
    sv = c["sv"].clone().requires_grad_(True)
    u = nr.fragment_weights(fr, sv)
    assert u.requires_grad
    with kernels_launched() as k:
        u.backward(gu.cuda())
    assert _adjoint_names_ok(k.names, name), k.names
    ref = FG.weights_reference(c["maps"], c["tri"], c["sv"], gu)
    _check(sv.grad, ref, f"{name} {S} weights")
    # a vertex of no visible face gets an exact +0
    _, cov, corners = pixel_weights(c["maps"], c["tri"])
    for b in range(B):
        seen = torch.zeros(c["V"], dtype=torch.bool)
        seen[corners[b][cov[b]].reshape(-1)] = True
        assert bool((_bits(sv.grad[b].cpu()[~seen]) == 0).all())


# ---- 3. the attribute node ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,S,aa", FG.scene_cases())
def test_attribute_node_with_screen_vertices(name, S, aa):
    from deep3dmap_amd import neural_renderer as nr
    c = _case(name, S, aa)
    fr, B, s = c["fr"], c["B"], c["s"]
    for C in (1, 3, 11):
        g = FG.seeded_grad_images(B, C, s)
        bg = seeded_background(C).cuda()
        for batched in (False, True):
            attr = seeded_attributes(name, C, batched)
            a0 = attr.cuda().requires_grad_(True)
            images0, alpha0 = nr.interpolate_vertex_attributes(a0, fr, bg)
            images0.backward(g.cuda())
            a1 = attr.cuda().requires_grad_(True)
            sv = c["sv"].clone().requires_grad_(True)
            images1, alpha1 = nr.interpolate_vertex_attributes(a1, fr, bg, screen_vertices=sv)
            with kernels_launched() as k:
                images1.backward(g.cuda())
            assert _adjoint_names_ok(k.names, name, {"k_vertex_attribute_face_sums", "k_vertex_attribute_large_face_sums",
                                                     "k_vertex_attribute_pixel_grads"}), k.names
            assert torch.equal(_bits(images1), _bits(images0)) and torch.equal(_bits(alpha1), _bits(alpha0))
            assert torch.equal(_bits(a1.grad), _bits(a0.grad))
            ref = FG.attribute_reference(c["maps"], c["tri"], c["sv"], attr, g, aa)
            _check(sv.grad, ref, f"{name} {S} aa={aa} attributes C={C} batched={batched}")
    # vertices that do not require grad: nothing extra is launched
    a = seeded_attributes(name, 3, False).cuda().requires_grad_(True)
    images, _ = nr.interpolate_vertex_attributes(a, fr, screen_vertices=c["sv"])
    with kernels_launched() as k:
        images.backward(FG.seeded_grad_images(B, 3, s).cuda())
    assert not {n for n in k.names if "geometry" in n or "pixel_grads" in n}, k.names


# ---- 4. the uv texture node ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,S,aa", FG.scene_cases())
def test_uv_node_with_screen_vertices(name, S, aa):
    """(a) an image affine in (x, y): every element compared.  (b) a seeded random image: output pixels fed by an internal
    pixel whose float64 position lies within 2^-12 of an integer get a zero image gradient (the taps are chosen from the
    float32 position); at most 2 % of the covered output pixels."""
    from deep3dmap_amd import neural_renderer as nr
    c = _case(name, S, aa)
    fr, B, s = c["fr"], c["B"], c["s"]
    g = FG.seeded_grad_images(B, 3, s)
    for spread, wrap in FG.UV_CASES:
        fuv = seeded_faces_uv(name, spread, FG.UV_SEED)[0]
        for H, W in FG.UV_SIZES:
            keep, share = FG.near_integer_mask(c["maps"], c["tri"], fuv, H, W, aa, wrap)
            print(name, S, aa, spread, wrap, H, W, "share of zeroed output pixels:", share)
            assert share <= FG.MAX_ZEROED_SHARE
            for kind, image, gi in (("affine", FG.affine_image(H, W, 3), g), ("random", seeded_image(H, W, 3), g * keep)):
                i0 = image.cuda().requires_grad_(True)
                images0, alpha0 = nr.sample_uv_texture(i0, fuv.cuda(), fr, wrap)
                images0.backward(gi.cuda())
                i1 = image.cuda().requires_grad_(True)
                sv = c["sv"].clone().requires_grad_(True)
                images1, alpha1 = nr.sample_uv_texture(i1, fuv.cuda(), fr, wrap, screen_vertices=sv)
                with kernels_launched() as k:
                    images1.backward(gi.cuda())
                assert _adjoint_names_ok({n for n in k.names if not n.startswith("k_uv_texture_images_")},
                                         name, {"k_uv_texture_pixel_grads"}), k.names
                assert torch.equal(_bits(images1), _bits(images0)) and torch.equal(_bits(alpha1), _bits(alpha0))
                assert torch.equal(_bits(i1.grad), _bits(i0.grad))
                ref = FG.uv_reference(c["maps"], c["tri"], c["sv"], fuv, image, gi, aa, wrap)
                _check(sv.grad, ref, f"{name} {S} aa={aa} uv {spread} {wrap} {H}x{W} {kind}")
    # vertices that do not require grad: nothing extra is launched
    image = seeded_image(8, 8, 3).cuda().requires_grad_(True)
    images, _ = nr.sample_uv_texture(image, seeded_faces_uv(name, "seamless", FG.UV_SEED)[0].cuda(), fr, screen_vertices=c["sv"])
    with kernels_launched() as k:
        images.backward(g.cuda())
    assert k.names and not {n for n in k.names if "geometry" in n or "pixel_grads" in n or "vertex_attribute" in n}, k.names


def test_uv_node_refuses_mipmap_with_screen_vertices():
    from deep3dmap_amd import neural_renderer as nr
    c = _case("S1", 16, False)
    fuv = seeded_faces_uv("S1", "seamless", FG.UV_SEED)[0].cuda()
    with kernels_launched() as k:
        with pytest.raises(NotImplementedError, match="mipmap"):
            nr.sample_uv_texture(torch.rand(8, 8, 3).cuda(), fuv, c["fr"], mipmap=True, screen_vertices=c["sv"].clone().requires_grad_(True))
    assert not k.names, k.names


# ---- 5. determinism -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,S,aa", [("S1", 32, True), ("S3B", 128, False), ("S4", 32, False)])
def test_the_same_bits_on_every_run(name, S, aa):
    from deep3dmap_amd import neural_renderer as nr
    c = _case(name, S, aa)
    fr, B, s = c["fr"], c["B"], c["s"]
    fuv = seeded_faces_uv(name, "corners", FG.UV_SEED)[0]
    attr, image = seeded_attributes(name, 11, True), seeded_image(32, 16, 3)
    g11, g3, gu = FG.seeded_grad_images(B, 11, s).cuda(), FG.seeded_grad_images(B, 3, s).cuda(), FG.seeded_grad_weights(B, S).cuda()

    def run(order):
        made = {}
        for what in order:                                            # (the operands' order of creation: other addresses)
            made[what] = {"sv": lambda: c["sv"].clone().requires_grad_(True), "attr": lambda: attr.cuda(),
                          "image": lambda: image.cuda(), "pad": lambda: torch.empty(12345, device="cuda")}[what]()
        out = []
        for f in (lambda sv: (nr.fragment_weights(fr, sv), gu),
                  lambda sv: (nr.interpolate_vertex_attributes(made["attr"], fr, screen_vertices=sv)[0], g11),
                  lambda sv: (nr.sample_uv_texture(made["image"], fuv.cuda(), fr, "MIRRORED_REPEAT", screen_vertices=sv)[0], g3)):
            sv = made["sv"].detach().clone().requires_grad_(True)
            y, gy = f(sv)
            y.backward(gy)
            out.append(sv.grad)
        return out
    first = run(("sv", "attr", "image"))
    for other in (run(("sv", "attr", "image")), run(("pad", "image", "attr", "pad", "sv"))):
        for a, b in zip(first, other):
            assert float(a.abs().max()) > 0 and torch.equal(_bits(a), _bits(b))


# ---- 6. the Renderer ----------------------------------------------------------------------------------------------------------
def test_renderer_geometry_grad_is_the_hand_written_composition():
    from deep3dmap_amd import neural_renderer as nr
    name, S, aa = "S2", 32, True
    c = _case(name, S, aa)
    r, faces, B, s = c["r"], c["faces"], c["B"], c["s"]
    attr = seeded_attributes(name, 3, False).cuda()
    image = seeded_image(32, 16, 3).cuda()
    fuv = seeded_faces_uv(name, "seamless", FG.UV_SEED)[0].cuda()
    g = FG.seeded_grad_images(B, 3, s).cuda()
    eyes = r.eye
    try:
        for node in ("attributes", "uv"):
            grads = []
            for by_hand in (False, True):
                v = c["v"].clone().requires_grad_(True)
                r.eye = eyes.clone().requires_grad_(True)
                if not by_hand:
                    images = (r.render_attributes(v, faces, attr, geometry_grad=True) if node == "attributes" else
                              r.render_uv_texture(v, faces, image, fuv, geometry_grad=True))[0]
                else:
                    sv = r._transform(v, None, None, None, None, None)
                    fr = nr.rasterize_fragments(sv.detach(), faces, r.image_size, r.anti_aliasing, r.fill_back, r.near, r.far)
                    images = (nr.interpolate_vertex_attributes(attr, fr, screen_vertices=sv) if node == "attributes" else
                              nr.sample_uv_texture(image, fuv, fr, screen_vertices=sv))[0]
                images.backward(g)
                grads.append((v.grad, r.eye.grad))
            (gv, ge), (hv, he) = grads
            assert torch.equal(_bits(gv), _bits(hv)) and torch.equal(_bits(ge), _bits(he))
            assert bool(torch.isfinite(gv).all()) and float(gv.abs().max()) > 0
            assert ge.shape == eyes.shape and bool(torch.isfinite(ge).all()) and float(ge.abs().max()) > 0
        # the defaults still refuse vertices that require grad
        r.eye = eyes
        v = c["v"].clone().requires_grad_(True)
        with pytest.raises(NotImplementedError, match="detach them: an attribute image carries no geometry gradient"):
            r.render_attributes(v, faces, attr)
        with pytest.raises(NotImplementedError, match="detach them"):
            r.render_uv_texture(v, faces, image, fuv, geometry_grad=False)
        with kernels_launched() as k:                                # (known from the arguments: before the rasteriser runs)
            with pytest.raises(NotImplementedError, match="mipmap"):
                r.render_uv_texture(v, faces, image, fuv, mipmap=True, geometry_grad=True)
        assert not k.names, k.names
    finally:
        r.eye = eyes


# ---- 7. capture ---------------------------------------------------------------------------------------------------------------
def test_captured_forward_and_backward():
    """fragment_weights forward plus backward captured (CapturedStep: torch.cuda.graph on the step's own stream) with the
    Fragments and the adjacency built beforehand; the replay has the bits of the eager run.  The captured step has a leaf of
    its own that no eager call ever touches; the eager runs use a twin."""
    from deep3dmap_amd import neural_renderer as nr
    from deep3dmap_amd.graph import CapturedStep
    name, S, aa = "S4", 32, False
    c = _case(name, S, aa)
    fr = c["fr"]
    values = [FG.seeded_grad_weights(c["B"], S, seed=sd).cuda() for sd in (41, 42)]
    gu = values[0].clone()
    twin = c["sv"].clone().requires_grad_(True)
    live = c["sv"].clone().requires_grad_(True)

    def step(sv):
        u = nr.fragment_weights(fr, sv)
        grad, = torch.autograd.grad(u, sv, gu)
        return u, grad

    step(twin)                                                       # (the adjacency exists before the capture)
    eager = []
    for i in (0, 1):
        gu.copy_(values[i])
        with kernels_launched() as k:
            eager.append([t.clone() for t in step(twin)])
        assert k.names == {"k_fragment_weights", CHUNKS} | ADJOINT, k.names     # nothing but the node's own kernels
    assert not torch.equal(eager[0][1], eager[1][1]) and float(eager[1][1].abs().max()) > 0
    torch.cuda.synchronize()
    cs = CapturedStep(lambda: step(live)).capture()
    for i in (1, 0, 1):
        gu.copy_(values[i])
        got = [t.clone() for t in cs()]
        torch.cuda.synchronize()
        for a, b in zip(got, eager[i]):
            assert torch.equal(_bits(a), _bits(b)), i
    cs.release()
