"""The interior geometry gradient without a device (neural_renderer/fragment_geometry.py, csrc/d3m_fragment_geometry.h): the
float64 reference of tests/fragment_geometry_scenes.py against central finite differences at fixed ownership and against the
closed form the kernels evaluate; the float32 yardstick behind the device tolerance; the near-integer exclusion's cap on the
oracle's maps; the argument checks of every new argument; the C entry points' refusals."""
import ctypes

import pytest
import torch

import fragment_geometry_scenes as FG
from uv_texture_image_scenes import seeded_faces_uv, seeded_image
from vertex_attribute_scenes import oracle_maps, scene, seeded_attributes

FD_STEP = 1e-6
FD_AGREEMENT = 1e-6       # of the largest gradient entry; truncation and round-off are both below 1e-9 at this step


def _central_differences(loss, sv):
    """d loss / d sv by central differences in float64, every entry"""
    base = sv.double()
    out = torch.zeros_like(base)
    flat = out.view(-1)
    for i in range(base.numel()):
        lo, hi = base.clone(), base.clone()
        lo.view(-1)[i] -= FD_STEP
        hi.view(-1)[i] += FD_STEP
        flat[i] = (float(loss(hi)) - float(loss(lo))) / (2 * FD_STEP)
    return out


def _agree(reference, fd, what):
    err = float((reference - fd).abs().max()) / float(reference.abs().max())
    print(what, "largest |reference - finite differences| / largest entry:", err)
    assert float(reference.abs().max()) > 0 and err <= FD_AGREEMENT, (what, err)


# ---- 1. the reference itself ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S1", "S2"])
def test_reference_against_finite_differences(name):
    S, dt = 16, torch.float64
    maps, tri, sv = oracle_maps(name, S), scene(name)["tri"], FG.screen_vertices(name)
    B = sv.shape[0]
    gu = FG.seeded_grad_weights(B, S).double()
    ref = FG.weights_reference(maps, tri, sv, gu)
    _agree(ref, _central_differences(lambda s: (FG.weights_of(maps, tri, s, dt)[0] * gu).sum(), sv), name + " weights")
    # the closed form the kernels evaluate is the same gradient
    assert max(FG.view_errors(FG.adjoint_identities(maps, tri, sv, gu), ref)) <= 1e-12
    for aa in (False, True):
        s = S // 2 if aa else S
        attr = seeded_attributes(name, 3, False)
        g = FG.seeded_grad_images(B, 3, s).double()
        ref = FG.attribute_reference(maps, tri, sv, attr, g, aa)
        fd = _central_differences(lambda v: (FG.attribute_images_of(maps, tri, v, attr, aa, dt) * g).sum(), sv)
        _agree(ref, fd, f"{name} attributes aa={aa}")
        # the uv image, value and derivative from the expression alone (what finite differences see), near-integer
        # positions excluded: the lookup is piecewise bilinear
        fuv = seeded_faces_uv(name, "seamless", FG.UV_SEED)[0]
        image = seeded_image(8, 8, 3)
        keep = _expression_mask(maps, tri, sv, fuv, 8, 8, aa).double()
        ref = FG.uv_reference(maps, tri, sv, fuv, image, g * keep, aa, "REPEAT", values_from_maps=False)
        fd = _central_differences(
            lambda v: (FG.uv_images_of(maps, tri, v, fuv, image, aa, "REPEAT", dt, values_from_maps=False) * g * keep).sum(), sv)
        _agree(ref, fd, f"{name} uv aa={aa}")


def _expression_mask(maps, tri, sv, faces_uv, H, W, aa):
    """near_integer_mask on the maps whose u is the expression's own (so that the excluded pixels are those of the function
    the finite differences evaluate)"""
    u = FG.weights_of(maps, tri, sv.double(), torch.float64)[0]
    z = torch.ones_like(maps["faces"])
    own = dict(maps, weight_map=u.float(), depth_map=torch.ones_like(maps["depth_map"]), faces=z)
    return FG.near_integer_mask(own, tri, faces_uv, H, W, aa, "REPEAT")[0]


# ---- 2. the yardstick of the device tolerance ---------------------------------------------------------------------------------
def test_float32_yardstick_is_the_recorded_one():
    """The error of the expression in float32 against float64 per scene, measured here again: within a factor 2 of the
    recorded figures either way (torch's float32 kernels may associate differently from build to build), and the device
    tolerance is 8 x the largest recorded one."""
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)                         # (a fixed order of torch's float32 scatter-add)
    try:
        for key, recorded in FG.YARDSTICK.items():
            name, S = key.split("/")
            maps, tri, sv = oracle_maps(name, int(S)), scene(name)["tri"], FG.screen_vertices(name)
            gu = FG.seeded_grad_weights(sv.shape[0], int(S))
            measured = max(FG.view_errors(FG.weights_reference(maps, tri, sv, gu, torch.float32),
                                          FG.weights_reference(maps, tri, sv, gu)))
            print(key, "float32 yardstick:", measured, "recorded:", recorded)
            assert recorded / 2 <= measured <= recorded * 2, (key, measured)
    finally:
        torch.use_deterministic_algorithms(was)
    assert set(FG.YARDSTICK) == {"%s/%d" % (n, S) for n, S, _ in FG.scene_cases()}      # every scene case has its figure
    assert FG.DEVICE_TOLERANCE == 8 * FG.YARDSTICK["S3B/128"] == 8 * max(FG.YARDSTICK.values())


def test_near_integer_exclusion_stays_within_its_cap_on_the_oracle_maps():
    worst = 0.0
    for name, S, aa in FG.scene_cases():
        maps, tri = oracle_maps(name, S), scene(name)["tri"]
        for spread, wrap in FG.UV_CASES:
            fuv = seeded_faces_uv(name, spread, FG.UV_SEED)[0]
            for H, W in FG.UV_SIZES:
                keep, share = FG.near_integer_mask(maps, tri, fuv, H, W, aa, wrap)
                assert share <= FG.MAX_ZEROED_SHARE, (name, S, aa, spread, wrap, H, W, share)
                worst = max(worst, share)
    print("largest share of zeroed output pixels:", worst)


# ---- 3. argument checks -------------------------------------------------------------------------------------------------------
def _host_fragments(B=2, V=6, F=2, s=4, anti_aliasing=False, fill_back=True):
    from deep3dmap_amd import neural_renderer as nr
    S = 2 * s if anti_aliasing else s
    Fp = 2 * F if fill_back else F
    return nr.Fragments(torch.full((B, S, S), -1, dtype=torch.int32), torch.zeros(B, S, S, 3), torch.zeros(B, S, S),
                        torch.zeros(B, Fp, 3, 3), torch.zeros(64, dtype=torch.uint8),
                        torch.tensor([[0, 1, 2], [3, 4, 5]], dtype=torch.int32)[:F], fill_back, s, anti_aliasing, V)


def _bad_screen_vertices():
    ok = torch.rand(2, 6, 3)
    return [torch.rand(6, 3), torch.rand(2, 6, 2), torch.rand(1, 2, 6, 3), ok.double(), ok.half(), ok.numpy(), torch.rand(2, 5, 3),
            torch.rand(2, 7, 3), torch.rand(3, 6, 3), torch.rand(1, 6, 3), ok.to("meta")]


def test_argument_errors_of_the_new_arguments():
    from deep3dmap_amd import neural_renderer as nr
    from deep3dmap_amd.neural_renderer import fragment_geometry
    assert nr.fragment_weights is fragment_geometry.fragment_weights
    fr = _host_fragments()
    attr, image, fuv = torch.rand(6, 3), torch.rand(8, 8, 3), torch.rand(2, 3, 2)
    sv = torch.rand(2, 6, 3, requires_grad=True)
    for bad in _bad_screen_vertices():
        with pytest.raises(ValueError, match="screen_vertices"):
            nr.fragment_weights(fr, bad)
        with pytest.raises(ValueError, match="screen_vertices"):
            nr.interpolate_vertex_attributes(attr, fr, screen_vertices=bad)
        with pytest.raises(ValueError, match="screen_vertices"):
            nr.sample_uv_texture(image, fuv, fr, screen_vertices=bad)
    with pytest.raises(ValueError, match="Fragments"):
        nr.fragment_weights(tuple(fr), sv)
    with pytest.raises(ValueError, match="fit"):
        nr.fragment_weights(fr._replace(weight_map=torch.zeros(2, 4, 4, 2)), sv)
    # well-formed arguments on the host end at the device check, behind every other check
    for call in (lambda: nr.fragment_weights(fr, sv), lambda: nr.fragment_weights(fr, sv.detach()),
                 lambda: nr.interpolate_vertex_attributes(attr, fr, screen_vertices=sv),
                 lambda: nr.sample_uv_texture(image, fuv, fr, screen_vertices=sv),
                 lambda: nr.sample_uv_texture(image, fuv, fr, screen_vertices=sv, mipmap=0)):
        with pytest.raises(ValueError, match="GPU"):
            call()
    # no geometry gradient through a mip-mapped lookup, whether or not the vertices require grad
    for v in (sv, sv.detach()):
        for mipmap in (1, 3, True):
            with pytest.raises(NotImplementedError, match="mipmap"):
                nr.sample_uv_texture(image, fuv, fr, screen_vertices=v, mipmap=mipmap)
    with pytest.raises(ValueError):                                  # (mipmap's own checks come first)
        nr.sample_uv_texture(image, fuv, fr, screen_vertices=sv, mipmap=4)
    # an index of tri outside [0, V) is refused where the adjacency is built
    with pytest.raises(ValueError, match="indices"):
        nr.fragment_weights(fr._replace(num_vertices=5), torch.rand(2, 5, 3))


def test_defaults_keep_the_existing_refusals():
    """screen_vertices=None and geometry_grad=False are today's paths: vertices that require grad still raise."""
    from deep3dmap_amd import neural_renderer as nr
    fr = _host_fragments()
    with pytest.raises(ValueError, match="GPU"):
        nr.interpolate_vertex_attributes(torch.rand(6, 3), fr, screen_vertices=None)
    with pytest.raises(ValueError, match="GPU"):
        nr.sample_uv_texture(torch.rand(8, 8, 3), torch.rand(2, 3, 2), fr, screen_vertices=None)
    r = object.__new__(nr.Renderer)                                  # (the constructor puts its camera on the device)
    r.camera_mode, r.image_size, r.anti_aliasing, r.fill_back, r.near, r.far = "none", 8, True, True, 0.1, 100
    v = torch.rand(2, 6, 3, requires_grad=True)
    faces = torch.tensor([[[0, 1, 2], [3, 4, 5]]])
    for geometry_grad in ({}, dict(geometry_grad=False)):
        with pytest.raises(NotImplementedError, match="detach them: an attribute image carries no geometry gradient"):
            r.render_attributes(v, faces, torch.rand(6, 3), **geometry_grad)
        with pytest.raises(NotImplementedError, match="detach them"):
            r.render_uv_texture(v, faces, torch.rand(8, 8, 3), torch.rand(2, 3, 2), **geometry_grad)
    # geometry_grad=True detaches for the record: the call gets as far as the device check
    with pytest.raises(ValueError, match="GPU"):
        r.render_attributes(v, faces, torch.rand(6, 3), geometry_grad=True)
    with pytest.raises(ValueError, match="GPU"):
        r.render_uv_texture(v, faces, torch.rand(8, 8, 3), torch.rand(2, 3, 2), geometry_grad=True)
    # ... but not with mipmap: known from the arguments, refused before the camera operators and the rasteriser
    for mipmap in (1, True):
        with pytest.raises(NotImplementedError, match="mipmap"):
            r.render_uv_texture(v, faces, torch.rand(8, 8, 3), torch.rand(2, 3, 2), mipmap=mipmap, geometry_grad=True)
    with pytest.raises(ValueError, match="GPU"):
        r.render_uv_texture(v, faces, torch.rand(8, 8, 3), torch.rand(2, 3, 2), mipmap=0, geometry_grad=True)


# ---- 4. the C entry points refuse bad arguments before any launch ---------------------------------------------------------------
def test_entry_points_return_invalid_before_any_launch():
    from deep3dmap_amd import _lib
    L = _lib.lib()
    p, q = ctypes.c_void_p(256), 256                                 # never dereferenced
    INVALID = 1
    fr_ok = dict(face_index_map=q, weight_map=q, depth_map=q, faces=q, tri=q, visibility=q, visibility_size=1 << 20,
                 batch_size=2, num_tri=2, fill_back=1, image_size=4, anti_aliasing=0)
    csr_ok = dict(offsets=q, items=q, chunks=None, long_rows=None, long_chunk_ptr=None, num_rows=6, num_chunks=0,
                  num_long_rows=0, long_row=64)
    bad_fr = [dict(face_index_map=None), dict(weight_map=None), dict(depth_map=None), dict(faces=None), dict(tri=None),
              dict(batch_size=0), dict(batch_size=65536), dict(num_tri=0), dict(image_size=0), dict(image_size=16385),
              dict(batch_size=40000, num_tri=40000), dict(batch_size=65535, image_size=16384)]

    def run(fn, ok, changes):
        for change in changes:
            a = dict(ok, **{k: v for k, v in change.items() if k in ok})
            if a.get("fr"):
                a["fr"] = ctypes.byref(_lib.D3MFragments(**dict(fr_ok, **{k: v for k, v in change.items() if k in fr_ok})))
            if a.get("csr"):
                a["csr"] = ctypes.byref(_lib.D3MCsr(**dict(csr_ok, **{k: v for k, v in change.items() if k in csr_ok})))
            assert fn(*a.values(), None) == INVALID, (fn.__name__, change)

    misaligned = ctypes.c_void_p(258)
    run(L.d3m_fragment_weights, dict(fr=True, weights=p), bad_fr + [dict(fr=None), dict(weights=None), dict(weights=misaligned)])
    run(L.d3m_vertex_attribute_pixel_grads,
        dict(fr=True, attributes=p, attributes_batch=1, V=6, C=3, grad_images=p, h=p),
        bad_fr + [dict(fr=None), dict(attributes=None), dict(grad_images=None), dict(h=None), dict(attributes_batch=3),
                  dict(V=0), dict(C=0), dict(C=1025)])
    run(L.d3m_uv_texture_pixel_grads,
        dict(fr=True, faces_uv=p, image=p, image_batch=1, H=8, W=8, C=3, wrapping=0, grad_images=p, h=p),
        bad_fr + [dict(fr=None), dict(faces_uv=None), dict(image=None), dict(grad_images=None), dict(h=None),
                  dict(h=misaligned), dict(image_batch=3), dict(H=0), dict(W=32769), dict(C=65), dict(wrapping=3)])
    bwd_ok = dict(fr=True, h=p, csr=True, scratch=p, scratch_floats=1 << 30, grad=p, V=6)
    run(L.d3m_fragment_geometry_backward, bwd_ok,
        bad_fr + [dict(fr=None), dict(h=None), dict(csr=None), dict(scratch=None), dict(grad=None), dict(h=misaligned), dict(V=0),
                  dict(visibility=None), dict(visibility_size=16), dict(offsets=None), dict(items=None), dict(num_rows=5),
                  dict(num_chunks=1, chunks=q), dict(num_long_rows=1, long_rows=q, long_chunk_ptr=q)])
    # the scratch: B F' 9 sums, 3 B num_chunks chunk sums, and 3 B S S with the pixel_grads map; too little has its own code
    csr = _lib.D3MCsr(**csr_ok)
    assert L.d3m_fragment_geometry_scratch_floats(2, 4, 4, ctypes.byref(csr), 0) == 2 * 4 * 9
    assert L.d3m_fragment_geometry_scratch_floats(2, 4, 4, ctypes.byref(csr), 1) == 2 * 4 * 9 + 2 * 4 * 4 * 3
    assert L.d3m_fragment_geometry_scratch_floats(2, 4, 0, ctypes.byref(csr), 1) == 0
    assert L.d3m_fragment_geometry_scratch_floats(0, 4, 4, ctypes.byref(csr), 0) == 0
    assert L.d3m_fragment_geometry_scratch_floats(65535, 4, 32768, ctypes.byref(csr), 0) == 0
    a = dict(bwd_ok, scratch_floats=2 * 4 * 9 - 1)
    a["fr"], a["csr"] = ctypes.byref(_lib.D3MFragments(**fr_ok)), ctypes.byref(csr)
    assert L.d3m_error_string(L.d3m_fragment_geometry_backward(*a.values(), None)) == b"workspace missing or too small"
