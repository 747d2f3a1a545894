"""Per-pixel spherical-harmonic shading of a UV albedo texture without a device (neural_renderer/sh_uv_fragments.py,
csrc/d3m_sh_uv_fragments.h): the two conditions of tests/sh_uv_fragment_scenes.py and the float32 yardsticks behind the device
tolerances; the float64 restatement against central finite differences in every argument; the composed route the node
replaces, which differs from it on a supersampled record; every error of the arguments; the C entry points' refusals."""
import ctypes

import pytest
import torch

import fragment_geometry_scenes as FG
import sh_fragment_scenes as SF
import sh_uv_fragment_scenes as SU
from deep3dmap_amd.neural_renderer import sh_uv_fragments      # the node every check in this file is about
from vertex_attribute_scenes import oracle_maps, scene

FD_STEP = 1e-6
FD_AGREEMENT = 1e-6       # of the largest gradient entry; truncation and round-off are both below 1e-9 at this step


# ---- 1. the conditions and the yardsticks of the device tolerances -------------------------------------------------------------
def test_conditions_hold_and_float32_yardsticks_are_the_recorded_ones():
    """Per case: min r >= 0.7 over covered pixels; the share of covered output pixels whose image gradient near_integer_mask
    zeroes for the geometry gradient stays within MAX_ZEROED_SHARE; the error of the expression in float32 against float64
    per kind, measured here again, is within a factor 2 of the recorded figure either way.  The device tolerance of a kind is
    8 x the largest recorded one, the light's 8 x the figure at S3B/128."""
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        for key, recorded in SU.YARDSTICK.items():
            name, S = key.split("/")
            measured, share, min_r = SU.measure_yardstick(name, int(S))
            print(key, "smallest r: %.3f" % min_r, "largest zeroed share: %.4f" % share)
            assert min_r >= SU.MIN_R, (key, min_r)
            assert share <= SU.MAX_ZEROED_SHARE, (key, share)
            for kind in SU.KINDS:
                print(key, kind, "float32 yardstick:", "%.2e" % measured[kind], "recorded:", recorded[kind])
                assert recorded[kind] / 2 <= measured[kind] <= recorded[kind] * 2, (key, kind, measured[kind])
    finally:
        torch.use_deterministic_algorithms(was)
    assert set(SU.YARDSTICK) == {"%s/%d" % (n, S) for n, S, _ in SU.CASES}
    for kind in SU.KINDS:
        largest = max(y[kind] for y in SU.YARDSTICK.values())
        assert SU.DEVICE_TOLERANCE[kind] == 8 * (SU.YARDSTICK["S3B/128"]["sh"] if kind == "sh" else largest)
    assert FG.UV_SEED == 24 and len(SU.uv_combos()) == 8 and len(SU.layouts()) == 8


def test_the_fixed_point_term_is_far_below_the_yardstick():
    """frac >= 47 at every case's size, and the derived bound on the fixed-point sum is below 1e-7 of the largest entry of
    the albedo image's float64 gradient in the case that has the most pixels (S3B/128)."""
    from deep3dmap_amd.neural_renderer.uv_texture_images import uv_adjoint_fraction_bits
    assert min(uv_adjoint_fraction_bits(2, S) for _, S, _ in SU.CASES) >= 47
    name, S = "S3B", 128
    maps, tri, sv = oracle_maps(name, S), scene(name)["tri"], FG.screen_vertices(name)
    g = SF.seeded_grad_out(2, S)
    (H, W), spread, wrapping = SU.uv_combos()[0]
    image, normals, sh = SU.inputs_of(name, "cone", (False, False, False), H, W, 2)
    ref = SU.reference(maps, tri, image, SU.faces_uv_of(name, spread), normals, sh, sv, g, False, wrapping)
    bound = SU.fixed_point_bound(maps, tri, normals, sh, g, False)
    print("fixed-point bound %.2e of the largest entry %.2e" % (bound, float(ref["albedo"].abs().max())))
    assert 0 < bound <= 1e-7 * float(ref["albedo"].abs().max())


# ---- 2. the restatement against central finite differences, in every argument ------------------------------------------------
def test_restatement_against_finite_differences():
    """S1/16 with anti-aliasing, an 8 x 8 texture, per-corner uv that MIRRORED_REPEAT folds.  The image gradient is zeroed
    where near_integer_mask says a lookup position sits on a texel boundary: the slope along pos jumps there, and a finite
    difference across the jump is not the derivative."""
    name, S, aa, dt = "S1", 16, True, torch.float64
    (H, W), spread, wrapping = (8, 8), "corners", "MIRRORED_REPEAT"
    maps, tri = oracle_maps(name, S), scene(name)["tri"]
    B = FG.screen_vertices(name).shape[0]
    uv = SU.faces_uv_of(name, spread)
    keep = FG.near_integer_mask(maps, tri, uv, H, W, aa, wrapping)[0].double()
    g = SF.seeded_grad_out(B, S // 2).double() * keep
    base = dict(image=SU.albedo_of(H, W).double(), normals=SF.cone_normals(name, False).double(), sh=SF.seeded_sh(B).double(),
                screen_vertices=FG.screen_vertices(name).double())

    def images(a):
        return SU.shade_uv_images_of(maps, tri, a["image"], uv, a["normals"], a["sh"], 0.5, aa, wrapping, dt,
                                     a["screen_vertices"], values_from_maps=False)[0]

    def loss(**changed):
        return float((images(dict(base, **changed)) * g).sum())

    leaves = {k: v.clone().requires_grad_(True) for k, v in base.items()}
    grads = dict(zip(leaves, torch.autograd.grad((images(leaves) * g).sum(), list(leaves.values()))))
    for key, value in base.items():
        fd = torch.zeros_like(value)
        for i in range(value.numel()):
            lo, hi = value.clone(), value.clone()
            lo.view(-1)[i] -= FD_STEP
            hi.view(-1)[i] += FD_STEP
            fd.view(-1)[i] = (loss(**{key: hi}) - loss(**{key: lo})) / (2 * FD_STEP)
        err = float((grads[key] - fd).abs().max()) / float(grads[key].abs().max())
        print(key, "largest |autograd - finite differences| / largest entry:", err)
        assert float(grads[key].abs().max()) > 0 and err <= FD_AGREEMENT, (key, err)
    # value from the maps, derivative from the expression: the images are the maps'
    ref = SU.reference(maps, tri, base["image"], uv, base["normals"], base["sh"], base["screen_vertices"], g, aa, wrapping, 0.5)
    plain = SU.shade_uv_images_of(maps, tri, base["image"], uv, base["normals"], base["sh"], 0.5, aa, wrapping, dt)[0]
    assert torch.equal(ref["image"], plain)


# ---- 3. the reason for the node ------------------------------------------------------------------------------------------------
def test_the_composed_route_differs_on_a_supersampled_record():
    """S1/32 with anti-aliasing: pool(a, background 0) * pool(s, background 1) -- shade_fragments' picture times
    sample_uv_texture's -- against pool(a s), in float64, per view in units of the view's largest entry: far beyond the
    image tolerance, in the interior (the product of two means is not the mean of the products) and at the silhouette."""
    name, S, aa = "S1", 32, True
    maps, tri = oracle_maps(name, S), scene(name)["tri"]
    worst = 0.0
    for (H, W), spread, wrapping in SU.uv_combos():
        image, normals, sh = SU.inputs_of(name, "cone", (False, False, False), H, W, 2)
        args = (maps, tri, image, SU.faces_uv_of(name, spread), normals, sh, None, aa, wrapping, torch.float64)
        node, composed = SU.shade_uv_images_of(*args)[0], SU.shade_uv_images_of(*args, composed=True)[0]
        errors = SU.errors_of(composed, node)
        print(f"{H}x{W} {spread} {wrapping}: |composed - node| / largest entry per view:", ["%.3f" % e for e in errors])
        assert min(errors) > SU.DEVICE_TOLERANCE["image"] > 0, (spread, wrapping, errors)
        worst = max(worst, max(errors))
        plain = (SU.shade_uv_images_of(*args[:7], False, *args[8:])[0], SU.shade_uv_images_of(*args[:7], False, *args[8:], composed=True)[0])
        assert torch.equal(*plain)                                    # without supersampling (background 0) the two are one
    print("largest difference: %.3f of the largest entry" % worst)


# ---- 4. argument checks ---------------------------------------------------------------------------------------------------------
def _host_fragments(B=2, V=6, F=2, s=4, anti_aliasing=False, fill_back=True):
    from deep3dmap_amd import neural_renderer as nr
    S = 2 * s if anti_aliasing else s
    Fp = 2 * F if fill_back else F
    return nr.Fragments(torch.full((B, S, S), -1, dtype=torch.int32), torch.zeros(B, S, S, 3), torch.zeros(B, S, S),
                        torch.zeros(B, Fp, 3, 3), torch.zeros(64, dtype=torch.uint8),
                        torch.tensor([[0, 1, 2], [3, 4, 5]], dtype=torch.int32)[:F], fill_back, s, anti_aliasing, V)


def test_argument_errors_are_raised_before_the_device():
    from deep3dmap_amd import neural_renderer as nr
    assert nr.shade_uv_texture is sh_uv_fragments.shade_uv_texture
    fr = _host_fragments()
    img, uv, n, sh = torch.rand(5, 7, 3), torch.rand(2, 3, 2), torch.rand(6, 3), torch.rand(3, 9)
    for bad in (img.numpy(), None):
        with pytest.raises(TypeError, match="tensors"):
            nr.shade_uv_texture(bad, uv, n, sh, fr)
    for bad_img, bad_uv in ((img.double(), uv), (img, uv.double()), (img.half(), uv)):
        with pytest.raises(TypeError, match="float32"):
            nr.shade_uv_texture(bad_img, bad_uv, n, sh, fr)
    for bad in (torch.rand(7, 3), torch.rand(1, 2, 5, 7, 3), torch.rand(0, 7, 3), torch.rand(5, 0, 3)):
        with pytest.raises(ValueError, match="image must be"):
            nr.shade_uv_texture(bad, uv, n, sh, fr)
    for bad in (torch.rand(5, 7, 1), torch.rand(5, 7, 4), torch.rand(2, 5, 7, 2)):
        with pytest.raises(ValueError, match="3 channels"):
            nr.shade_uv_texture(bad, uv, n, sh, fr)
    for bad in (torch.rand(3, 5, 7, 3), torch.rand(1, 5, 7, 3)):
        with pytest.raises(ValueError, match="views"):
            nr.shade_uv_texture(bad, uv, n, sh, fr)
    for shape in ((32769, 1, 3), (1, 32769, 3)):
        with pytest.raises(ValueError, match="at most 32768"):
            nr.shade_uv_texture(torch.empty(shape, device="meta"), uv, n, sh, fr)
    for bad in (torch.rand(3, 3, 2), torch.rand(2, 3), torch.rand(2, 2, 3), torch.rand(1, 3, 2)):
        with pytest.raises(ValueError, match="faces_uv"):
            nr.shade_uv_texture(img, bad, n, sh, fr)
    with pytest.raises(NotImplementedError, match="faces_uv"):
        nr.shade_uv_texture(img, uv.clone().requires_grad_(True), n, sh, fr)
    with pytest.raises(ValueError, match="CLAMP_TO_BORDER"):
        nr.shade_uv_texture(img, uv, n, sh, fr, texture_wrapping="CLAMP_TO_BORDER")
    with pytest.raises((ValueError, TypeError)):
        nr.shade_uv_texture(img, uv, n, sh, fr, texture_wrapping="NO_SUCH_WRAPPING")
    with pytest.raises(ValueError, match="device"):
        nr.shade_uv_texture(img.to("meta"), uv, n, sh, fr)
    for bad in (torch.rand(6), torch.rand(6, 2), n.double(), n.numpy(), torch.rand(5, 3), torch.rand(3, 6, 3), n.to("meta")):
        with pytest.raises(ValueError, match="normals"):
            nr.shade_uv_texture(img, uv, bad, sh, fr)
    for bad in (torch.rand(9), torch.rand(3, 8), sh.double(), sh.numpy(), torch.rand(3, 3, 9), sh.to("meta"), None):
        with pytest.raises(ValueError, match="sh"):
            nr.shade_uv_texture(img, uv, n, bad, fr)
    for bad in (torch.rand(6, 3), torch.rand(2, 6, 2), torch.rand(2, 6, 3).double(), torch.rand(2, 5, 3), torch.rand(3, 6, 3)):
        with pytest.raises(ValueError, match="screen_vertices"):
            nr.shade_uv_texture(img, uv, n, sh, fr, screen_vertices=bad)
    with pytest.raises(ValueError, match="Fragments"):
        nr.shade_uv_texture(img, uv, n, sh, tuple(fr))
    with pytest.raises(ValueError, match="fit"):
        nr.shade_uv_texture(img, uv, n, sh, fr._replace(weight_map=torch.zeros(2, 4, 4, 2)))
    with pytest.raises(ValueError, match="background"):
        nr.shade_uv_texture(img, uv, n, sh, fr, background=torch.rand(3, requires_grad=True))
    with pytest.raises(ValueError, match="background"):
        nr.shade_uv_texture(img, uv, n, sh, fr, background=[0.1, 0.2])
    with pytest.raises(ValueError, match="2\\^32"):                   # B S S beyond 2^32 (meta maps: nothing is allocated)
        meta = lambda shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device="meta")
        big = nr.Fragments(meta((5, 32768, 32768), torch.int32), meta((5, 32768, 32768, 3)), meta((5, 32768, 32768)),
                           meta((5, 4, 3, 3)), meta(64, torch.uint8), fr.tri.to("meta"), True, 32768, False, 6)
        nr.shade_uv_texture(img.to("meta"), uv.to("meta"), n.to("meta"), sh.to("meta"), big)
    with pytest.raises(TypeError):                                    # mipmap and colors are not offered
        nr.shade_uv_texture(img, uv, n, sh, fr, mipmap=True)
    with pytest.raises(TypeError):
        nr.shade_uv_texture(img, uv, n, sh, fr, colors=torch.rand(6, 3))
    # well-formed arguments on the host end at the device check, behind every other check
    sv = torch.rand(2, 6, 3, requires_grad=True)
    light = nr.SHLight()
    for call in (lambda: nr.shade_uv_texture(img, uv, n, sh, fr),
                 lambda: nr.shade_uv_texture(torch.rand(2, 5, 7, 3), uv, torch.rand(2, 6, 3), torch.rand(2, 3, 9), fr,
                                             "MIRRORED_REPEAT", [0.1, 0.2, 0.3], screen_vertices=sv),
                 lambda: light.shade_uv_texture(img, uv, n, fr), lambda: light.shade_uv_texture(img, uv, n, fr, background=1.0)):
        with pytest.raises(ValueError, match="GPU"):
            call()
    with pytest.raises(ValueError, match="sh"):                       # a per-set light of another count than the record's views
        nr.SHLight(per_set=3).shade_uv_texture(img, uv, n, fr)


def test_render_uv_shaded_refuses_antialias_on_a_supersampling_renderer_before_any_launch():
    from deep3dmap_amd import neural_renderer as nr
    r = object.__new__(nr.Renderer)                                  # (the constructor puts its camera on the device)
    r.camera_mode, r.image_size, r.anti_aliasing, r.fill_back, r.near, r.far = "none", 8, True, True, 0.1, 100
    v, faces = torch.rand(2, 6, 3), torch.tensor([[[0, 1, 2], [3, 4, 5]]])
    with pytest.raises(ValueError, match="anti_aliasing=False"):
        r.render_uv_shaded(v, faces, torch.rand(3, 9), torch.rand(4, 4, 3), torch.rand(2, 3, 2), normals=torch.rand(6, 3),
                           antialias=True)


def test_shade_fragments_no_longer_recommends_the_multiplication():
    from deep3dmap_amd import neural_renderer as nr
    doc = " ".join(nr.shade_fragments.__doc__.split())
    assert "shade_uv_texture" in doc and "multiplies the result with" not in doc


# ---- 5. the C entry points refuse bad arguments before any launch ---------------------------------------------------------------
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
              dict(batch_size=65535, image_size=16384), dict(fr=None)]
    misaligned = ctypes.c_void_p(258)
    bad_inputs = [dict(normals=None), dict(normals=misaligned), dict(sh=None), dict(sh=misaligned), dict(nb=3), dict(nb=0),
                  dict(sb=3), dict(V=0), dict(faces_uv=None), dict(faces_uv=misaligned), dict(image=None),
                  dict(image=misaligned), dict(ib=3), dict(ib=0), dict(H=0), dict(W=0), dict(H=32769), dict(W=32769),
                  dict(wrapping=3), dict(wrapping=-1)]

    def run(fn, ok, changes):
        for change in changes:
            a = dict(ok, **{k: v for k, v in change.items() if k in ok})
            if a.get("fr"):
                a["fr"] = ctypes.byref(_lib.D3MFragments(**dict(fr_ok, **{k: v for k, v in change.items() if k in fr_ok})))
            if a.get("csr"):
                a["csr"] = ctypes.byref(_lib.D3MCsr(**dict(csr_ok, **{k: v for k, v in change.items() if k in csr_ok})))
            assert fn(*a.values(), None) == INVALID, (fn.__name__, change)

    inputs = dict(fr=True, normals=p, nb=1, sh=p, sb=1, V=6, faces_uv=p, image=p, ib=1, H=5, W=7, wrapping=0)
    run(L.d3m_sh_uv_fragment_images, dict(inputs, background=None, images=p, alpha=p),
        bad_fr + bad_inputs + [dict(images=None), dict(alpha=None), dict(images=misaligned), dict(alpha=misaligned),
                               dict(background=misaligned)])
    run(L.d3m_sh_uv_fragment_pixel_grads, dict(inputs, grad_images=p, h=p),
        bad_fr + bad_inputs + [dict(grad_images=None), dict(h=None), dict(grad_images=misaligned), dict(h=misaligned)])
    bwd_ok = dict(inputs, grad_images=p, csr=True, scratch=p, scratch_bytes=1 << 30, grad_normals=p, grad_sh=p, grad_image=p,
                  pixel_grads=p)
    run(L.d3m_sh_uv_fragment_images_backward, bwd_ok,
        bad_fr + bad_inputs + [dict(grad_images=None), dict(grad_images=misaligned), dict(csr=None), dict(scratch=None),
                               dict(scratch=ctypes.c_void_p(260)), dict(grad_normals=None, grad_sh=None, grad_image=None, pixel_grads=None),
                               dict(grad_normals=misaligned), dict(grad_sh=misaligned), dict(grad_image=misaligned),
                               dict(pixel_grads=misaligned), dict(visibility=None), dict(visibility_size=16),
                               dict(offsets=None), dict(items=None), dict(num_rows=5), dict(num_chunks=1, chunks=q),
                               dict(num_long_rows=1, long_rows=q, long_chunk_ptr=q)])
    # the scratch: the image adjoint's accumulators and 1024 block maxima, then floats: the gather's B F' 3 3 sums, the two
    # gradient images 2 B 3 S S, the light's partials B parts 27
    csr = _lib.D3MCsr(**csr_ok)
    fixed = lambda ib, H, W: ib * H * W * 3 * 8 + 1024 * 4
    floats = lambda B, Fp, S, parts: B * Fp * 3 * 3 + 2 * B * 3 * S * S + B * parts * 27
    assert L.d3m_sh_uv_fragment_scratch_bytes(2, 4, 4, 1, 5, 7, ctypes.byref(csr)) == fixed(1, 5, 7) + 4 * floats(2, 4, 4, 1)
    assert L.d3m_sh_uv_fragment_scratch_bytes(2, 4, 128, 2, 5, 7, ctypes.byref(csr)) == fixed(2, 5, 7) + 4 * floats(2, 4, 128, 16)
    for bad in ((0, 4, 4, 1, 5, 7), (2, 0, 4, 1, 5, 7), (2, 4, 0, 1, 5, 7), (2, 4, 4, 3, 5, 7), (2, 4, 4, 1, 0, 7),
                (2, 4, 4, 1, 5, 32769), (65535, 4, 32768, 1, 5, 7)):
        assert L.d3m_sh_uv_fragment_scratch_bytes(*bad, ctypes.byref(csr)) == 0, bad
    assert L.d3m_sh_uv_fragment_scratch_bytes(2, 4, 4, 1, 5, 7, None) == 0
    a = dict(bwd_ok, scratch_bytes=fixed(1, 5, 7) + 4 * floats(2, 4, 4, 1) - 1)
    a["fr"], a["csr"] = ctypes.byref(_lib.D3MFragments(**fr_ok)), ctypes.byref(csr)
    assert L.d3m_error_string(L.d3m_sh_uv_fragment_images_backward(*a.values(), None)) == b"workspace missing or too small"
