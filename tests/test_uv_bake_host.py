"""View images baked into a uv texture without a device (neural_renderer/uv_bake.py, csrc/d3m_uv_bake.h): the float64
restatement of tests/uv_bake_scenes.py against central finite differences in the images and the screen vertices; the float32
yardsticks behind the device tolerances and the margin of the decisions; the share of texel-views near a threshold in every
case; the round trip through the restatement of sample_uv_texture; the layout's vertices; every ValueError; the C entry
points' refusals."""
import ctypes

import numpy as np
import pytest
import torch

import uv_bake_scenes as UB
import uv_texture_image_scenes as UT
from deep3dmap_amd.neural_renderer import uv_bake      # the node every check in this file is about
from vertex_attribute_scenes import scene

FD_STEP = 1e-6
FD_AGREEMENT = 1e-6       # of the largest gradient entry (test_sh_fragments_host.py's step and rule)


# ---- 1. the restatement against central finite differences ---------------------------------------------------------------------
@pytest.mark.parametrize("perspective", (True, False))
def test_restatement_against_finite_differences(perspective):
    name, T, S, dt = "S1", 20, 16, torch.float64
    uv_maps, view_maps = UB.oracle_layout_maps(name, "atlas", T), UB.oracle_view_maps(name, S, perspective)
    tri = scene(name)["tri"]
    base = dict(sv=UB.screen_vertices(name, perspective).double(), images=UB.seeded_images(2, 2, 6, 10).double())
    g = UB.seeded_grad_texture(2, T, 2).double()
    ref = UB.reference(uv_maps, view_maps, tri, base["sv"], base["images"], g, perspective)
    frozen = UB.decisions_of(ref["info"])                             # the decisions are constants: a step must not move them
    assert int(ref["mask"].sum()) > 50

    def loss(**changed):
        a = dict(base, **changed)
        tex = UB.bake_of(uv_maps, view_maps, tri, a["sv"], a["images"], perspective, UB.DEPTH_TOLERANCE, None, dt, frozen)[0]
        return float((tex * g).sum())

    for key, kind in (("sv", "screen_vertices"), ("images", "images")):
        value, grad = base[key], ref[kind]
        fd = torch.zeros_like(value)
        for i in range(value.numel()):
            lo, hi = value.clone(), value.clone()
            lo.view(-1)[i] -= FD_STEP
            hi.view(-1)[i] += FD_STEP
            fd.view(-1)[i] = (loss(**{key: hi}) - loss(**{key: lo})) / (2 * FD_STEP)
        err = float((grad - fd).abs().max()) / float(grad.abs().max())
        print(key, "largest |autograd - finite differences| / largest entry:", err)
        assert float(grad.abs().max()) > 0 and err <= FD_AGREEMENT, (key, err)
    if not perspective:
        assert float(ref["screen_vertices"][..., 2].abs().max()) == 0.0      # orthographic: no gradient to z


# ---- 2. the yardsticks, the margin and the share of texel-views near a threshold -----------------------------------------------
def test_float32_yardsticks_are_the_recorded_ones():
    """Measured here again: within a factor 2 of the recorded figures either way (torch's float32 kernels may associate
    differently from build to build).  The device tolerance of a kind is 8 x the largest recorded one; the margins M_POS and
    M_Z are 8 x the largest recorded error of the decision quantities."""
    assert set(UB.YARDSTICK) == {UB.case_id(c) for c in UB.CASES}
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        for case in UB.CASES:
            measured, recorded = UB.measure_yardstick(case), UB.YARDSTICK[UB.case_id(case)]
            for kind, value in measured.items():
                print(UB.case_id(case), kind, "float32 yardstick:", "%.2e" % value, "recorded:", recorded[kind])
                assert recorded[kind] / 2 <= value <= recorded[kind] * 2, (UB.case_id(case), kind, value)
    finally:
        torch.use_deterministic_algorithms(was)
    for kind in UB.KINDS:
        assert UB.DEVICE_TOLERANCE[kind] == 8 * max(y[kind] for y in UB.YARDSTICK.values())
    assert UB.M_POS == 8 * max(y["position"] for y in UB.YARDSTICK.values())
    assert UB.M_Z == 8 * max(y["depth"] for y in UB.YARDSTICK.values())


@pytest.mark.parametrize("case", UB.CASES, ids=UB.case_id)
def test_few_texel_views_lie_near_a_threshold(case):
    """At most 1 % of the covered texel-views of a case lie within the margin of a threshold, and every case exercises what it
    is there for: visible texels, texels hidden behind another triangle, texels outside every uv triangle."""
    uv_maps, view_maps = UB.case_oracle_maps(case)
    a = UB.case_inputs(case)
    ref = UB.reference(uv_maps, view_maps, a["tri"], a["sv"], a["images"], a["grad_texture"], case[8])
    info = ref["info"]
    share = UB.near_share(info, UB.M_POS, UB.M_Z)
    hidden = info["other"] & ~info["visible"]
    print(UB.case_id(case), "covered texel-views:", int(info["covered"].sum()), "visible:", int(info["visible"].sum()),
          "hidden behind another triangle:", int(hidden.sum()), "share near a threshold: %.4f" % share)
    assert share <= UB.MAX_NEAR_SHARE, share
    assert int(info["visible"].sum()) > 0 and int((~info["covered"]).sum()) > 0
    if case[1] == "planar" and case[0] in ("S1", "S4"):
        assert int(hidden.sum()) > 0                                  # the closed meshes: owners that the view does not see
    owners = uv_maps["face_index_map"][0]
    F = a["tri"].shape[0]
    if case[1] == "atlas" or case[0] == "S1":                         # (a planar quad has one winding)
        assert int((owners >= F).sum()) > 0 and int(((owners >= 0) & (owners < F)).sum()) > 0      # both windings own texels
    if case[2] == 128:
        counts = torch.bincount(owners[owners >= 0].flatten())
        assert int(counts.max()) > 4096                               # the workgroup route of stage 1


# ---- 3. the round trip through sample_uv_texture's restatement -------------------------------------------------------------------
def _round_trip(texture, T, S):
    """(baked, texture, interior) at the visible texels whose four taps are covered pixels: the planar patch seen straight on
    without perspective, drawn by the float64 restatement of sample_uv_texture and baked back"""
    name = "planar"
    tri = scene(name)["tri"]
    faces_uv = UB.planar_layout(name)
    uv_maps, view_maps = UB.oracle_layout_maps(name, "planar", T), UB.oracle_view_maps(name, S, False)
    image, alpha = UT.restate_uv_texture_images(view_maps, tri, faces_uv, texture.double(), None, False, "REPEAT", torch.float64)
    sv = UB.screen_vertices(name, False)
    baked, mask, info = UB.bake_of(uv_maps, view_maps, tri, sv, image, False, UB.DEPTH_TOLERANCE, None, torch.float64)
    cov = alpha[0] > 0                                                # [S,S], output orientation
    yi, xi = info["yi"][0], info["xi"][0]
    y1, x1 = (yi + 1).clamp(max=S - 1), (xi + 1).clamp(max=S - 1)
    interior = mask[0] & cov[yi, xi] & cov[yi, x1] & cov[y1, xi] & cov[y1, x1]
    return baked[0], texture.double(), interior


def test_round_trip_returns_the_texture_at_visible_texels():
    """Bilinear interpolation reproduces affine functions, and on the planar patch without perspective uv is an affine function
    of the screen position: an AFFINE texture comes back up to the float32 rounding of the two records' maps and of the layout's
    vertices (a handful of roundings in each record's weights, each moving a lookup by 2^-24 of the texture's range: 32 x 2^-24
    of the largest texel allowed).  A smooth texture A (sin(w u) + sin(w v))
    comes back within the two interpolations' errors, (1/8) h^2 max|f''| per axis each: A w^2 / 8 (2 / (T - 1)^2 + 2 s^2), s the
    uv step of one pixel.  Measured: 1.7e-7 (affine), 8.4e-3 against a bound of 9.8e-3 (smooth), T = 20, S = 32."""
    T, S = 20, 32
    u = torch.linspace(0, 1, T, dtype=torch.float64)
    vv, uu = torch.meshgrid(u, u, indexing="ij")                      # texture row j is v, column i is u
    affine = (0.3 + 0.5 * uu - 0.2 * vv)[..., None]
    baked, tex, interior = _round_trip(affine, T, S)
    assert int(interior.sum()) > 100
    err = float((baked - tex)[interior].abs().max())
    print("round trip of an affine texture, largest error at", int(interior.sum()), "interior texels:", err)
    assert err <= 32 * 2.0 ** -24 * float(affine.abs().max())
    A, w = 0.25, 2 * np.pi
    smooth = (A * (torch.sin(w * uu) + torch.sin(w * vv)))[..., None]
    baked, tex, interior = _round_trip(smooth, T, S)
    # the patch spans uv 0.88 over the screen width it covers: x from -0.8 to 0.8 of a look_at camera without perspective
    sv = UB.screen_vertices("planar", False)[0]
    step = 0.88 / (float(sv[:, 0].max() - sv[:, 0].min()) * S / 2)
    bound = A * w * w / 8 * (2 / (T - 1) ** 2 + 2 * step ** 2)
    err = float((baked - tex)[interior].abs().max())
    print("round trip of a smooth texture: largest error", err, "bound", bound)
    assert err <= bound


# ---- 4. the layout's vertices ----------------------------------------------------------------------------------------------------
def test_layout_vertices_put_texel_centres_on_sample_uv_textures_grid():
    T = 20
    uv = torch.tensor([[[0.0, 1.0], [3 / 19, 7 / 19], [1.25, -0.5]]])
    v, tri = uv_bake.uv_layout_vertices(uv, T, "CLAMP_TO_EDGE")
    assert v.shape == (1, 3, 3) and v.dtype == torch.float32 and tri.dtype == torch.int32 and tri.tolist() == [[0, 1, 2]]
    centre = lambda i: (2 * i + 1 - T) / T                           # pixel_center of the rasteriser
    expect = torch.tensor([[centre(0), centre(19), 1.0], [centre(3), centre(7), 1.0], [centre(19), centre(0), 1.0]])
    assert torch.allclose(v[0], expect, atol=1e-6, rtol=0)
    wrapped = uv_bake.wrap_uv(torch.tensor([-0.25, 0.0, 1.5, 2.25]), 0)
    assert torch.equal(wrapped, UT.wrap_uv(torch.tensor([-0.25, 0.0, 1.5, 2.25]), "REPEAT"))
    for code, name in enumerate(UT.WRAPS):
        x = torch.linspace(-2.3, 2.9, 53)
        assert torch.equal(uv_bake.wrap_uv(x, code), UT.wrap_uv(x, name))
    for bad in (torch.rand(4, 3), torch.rand(4, 2, 3), torch.rand(0, 3, 2), torch.rand(4, 3, 2).double(), None):
        with pytest.raises(ValueError, match="faces_uv"):
            uv_bake.uv_layout_fragments(bad, T)
    for bad in (0, -3, 16385, 2.5, True):
        with pytest.raises(ValueError, match="texture_size"):
            uv_bake.uv_layout_fragments(torch.rand(4, 3, 2), bad)
    with pytest.raises(ValueError, match="CLAMP_TO_BORDER"):
        uv_bake.uv_layout_fragments(torch.rand(4, 3, 2), T, "CLAMP_TO_BORDER")
    with pytest.raises(ValueError, match="GPU"):
        uv_bake.uv_layout_fragments(torch.rand(4, 3, 2), T)
    assert uv_bake.bake_adjoint_fraction_bits(20) == 62 - 9 and uv_bake.bake_adjoint_fraction_bits(512) == 44
    with pytest.raises(ValueError):
        uv_bake.bake_adjoint_fraction_bits(16385)


# ---- 5. argument checks ---------------------------------------------------------------------------------------------------------
def _host_fragments(B=2, V=6, F=2, s=4, anti_aliasing=False, fill_back=True):
    from deep3dmap_amd import neural_renderer as nr
    S = 2 * s if anti_aliasing else s
    Fp = 2 * F if fill_back else F
    return nr.Fragments(torch.full((B, S, S), -1, dtype=torch.int32), torch.zeros(B, S, S, 3), torch.zeros(B, S, S),
                        torch.zeros(B, Fp, 3, 3), torch.zeros(64, dtype=torch.uint8),
                        torch.tensor([[0, 1, 2], [3, 4, 5], [0, 2, 4]], dtype=torch.int32)[:F], fill_back, s, anti_aliasing, V)


def test_argument_errors_are_raised_before_the_device():
    from deep3dmap_amd import neural_renderer as nr
    assert nr.bake_uv_texture is uv_bake.bake_uv_texture and nr.uv_layout_fragments is uv_bake.uv_layout_fragments
    fr, uv = _host_fragments(), _host_fragments(B=1, s=8)
    img, sv = torch.rand(2, 3, 5, 7), torch.rand(2, 6, 3)
    for bad in (torch.rand(3, 5, 7), torch.rand(2, 3, 5, 7, 1), img.double(), img.numpy(), torch.rand(2, 0, 5, 7),
                torch.rand(2, 65, 5, 7), torch.rand(2, 3, 0, 7), torch.rand(3, 3, 5, 7), torch.rand(1, 3, 5, 7), img.to("meta")):
        with pytest.raises(ValueError, match="images"):
            nr.bake_uv_texture(bad, uv, fr, sv)
    for bad in (torch.rand(6, 3), torch.rand(2, 6, 2), sv.double(), torch.rand(2, 5, 3), torch.rand(3, 6, 3), sv.to("meta")):
        with pytest.raises(ValueError, match="screen_vertices"):
            nr.bake_uv_texture(img, uv, fr, bad)
    with pytest.raises(ValueError, match="Fragments"):
        nr.bake_uv_texture(img, uv, tuple(fr), sv)
    with pytest.raises(ValueError, match="uv_fragments"):
        nr.bake_uv_texture(img, tuple(uv), fr, sv)
    with pytest.raises(ValueError, match="one view"):
        nr.bake_uv_texture(img, _host_fragments(B=2, s=8), fr, sv)
    with pytest.raises(ValueError, match="anti_aliasing"):
        nr.bake_uv_texture(img, _host_fragments(B=1, s=8, anti_aliasing=True), fr, sv)
    with pytest.raises(ValueError, match="triangles"):
        nr.bake_uv_texture(img, _host_fragments(B=1, s=8, F=3), fr, sv)
    with pytest.raises(ValueError, match="fit"):
        nr.bake_uv_texture(img, uv._replace(weight_map=torch.zeros(1, 8, 8, 2)), fr, sv)
    with pytest.raises(ValueError, match="device"):
        nr.bake_uv_texture(img, uv._replace(**{k: getattr(uv, k).to("meta") for k in
                                               ("face_index_map", "weight_map", "depth_map", "faces", "tri", "visibility")}), fr, sv)
    for bad in (-1e-3, float("nan"), float("inf"), None, "0.1", True):
        with pytest.raises(ValueError, match="depth_tolerance"):
            nr.bake_uv_texture(img, uv, fr, sv, depth_tolerance=bad)
    with pytest.raises(ValueError, match="background"):
        nr.bake_uv_texture(img, uv, fr, sv, background=[0.1, 0.2])
    with pytest.raises(ValueError, match="background"):
        nr.bake_uv_texture(img, uv, fr, sv, background=torch.rand(3, requires_grad=True))
    with pytest.raises(ValueError, match="indices"):                  # an index of tri outside [0, V)
        nr.bake_uv_texture(img, uv, fr._replace(num_vertices=5), torch.rand(2, 5, 3))
    # well-formed arguments on the host end at the device check, behind every other check
    for call in (lambda: nr.bake_uv_texture(img, uv, fr, sv),
                 lambda: nr.bake_uv_texture(img.requires_grad_(True), uv, fr, sv.requires_grad_(True), perspective=False,
                                            depth_tolerance=0, background=[0.1, 0.2, 0.3])):
        with pytest.raises(ValueError, match="GPU"):
            call()


# ---- 6. the C entry points refuse bad arguments before any launch ---------------------------------------------------------------
def test_entry_points_return_invalid_before_any_launch():
    from deep3dmap_amd import _lib
    L = _lib.lib()
    p, q = ctypes.c_void_p(256), 256                                 # never dereferenced
    INVALID = 1
    fr_ok = dict(face_index_map=q, weight_map=q, depth_map=q, faces=q, tri=q, visibility=q, visibility_size=1 << 20,
                 batch_size=2, num_tri=2, fill_back=1, image_size=4, anti_aliasing=0)
    uv_ok = dict(fr_ok, batch_size=1, image_size=8)
    csr_ok = dict(offsets=q, items=q, chunks=None, long_rows=None, long_chunk_ptr=None, num_rows=6, num_chunks=0,
                  num_long_rows=0, long_row=64)
    bad_record = [dict(face_index_map=None), dict(weight_map=None), dict(depth_map=None), dict(faces=None), dict(tri=None),
                  dict(batch_size=0), dict(num_tri=0), dict(image_size=0), dict(image_size=16385)]
    misaligned = ctypes.c_void_p(258)

    def run(fn, ok, changes):
        for change in changes:
            a = dict(ok, **{k: v for k, v in change.items() if k in ok})
            a["uv"] = ctypes.byref(_lib.D3MFragments(**dict(uv_ok, **change.get("uv_change", {})))) if a["uv"] else None
            a["fr"] = ctypes.byref(_lib.D3MFragments(**dict(fr_ok, **change.get("fr_change", {})))) if a["fr"] else None
            if a.get("csr"):
                a["csr"] = ctypes.byref(_lib.D3MCsr(**dict(csr_ok, **change.get("csr_change", {}))))
            assert fn(*a.values(), None) == INVALID, (fn.__name__, change)

    records = ([dict(uv_change=c) for c in bad_record] + [dict(fr_change=c) for c in bad_record] +
               [dict(uv=None), dict(fr=None), dict(uv_change=dict(batch_size=2)), dict(uv_change=dict(anti_aliasing=1)),
                dict(uv_change=dict(num_tri=3)), dict(fr_change=dict(batch_size=65536))])
    sizes = [dict(C=0), dict(C=65), dict(H=0), dict(W=0), dict(H=32769), dict(W=32769), dict(sv=None), dict(sv=misaligned),
             dict(V=0), dict(tol=-1.0), dict(tol=float("nan")), dict(tol=float("inf"))]
    fwd = dict(uv=True, fr=True, images=p, C=3, H=5, W=7, sv=p, V=6, persp=1, tol=ctypes.c_float(0.01), background=None,
               texture=p, mask=p)
    run(L.d3m_uv_bake_texture, fwd, records + sizes + [dict(images=None), dict(images=misaligned), dict(texture=None),
                                                       dict(mask=None), dict(texture=misaligned), dict(mask=misaligned),
                                                       dict(background=misaligned)])
    img_bwd = dict(uv=True, fr=True, C=3, H=5, W=7, sv=p, V=6, persp=1, tol=ctypes.c_float(0.01), grad_texture=p, scratch=p,
                   scratch_bytes=1 << 30, grad_images=p)
    run(L.d3m_uv_bake_images_backward, img_bwd,
        records + sizes + [dict(grad_texture=None), dict(grad_texture=misaligned), dict(scratch=None),
                           dict(scratch=ctypes.c_void_p(260)), dict(grad_images=None), dict(grad_images=misaligned)])
    assert L.d3m_uv_bake_images_scratch_bytes(2, 3, 5, 7) == 2 * 3 * 5 * 7 * 8 + 1024 * 4
    assert L.d3m_uv_bake_images_scratch_bytes(0, 3, 5, 7) == 0 == L.d3m_uv_bake_images_scratch_bytes(2, 65, 5, 7)
    a = dict(img_bwd, scratch_bytes=2 * 3 * 5 * 7 * 8 + 1024 * 4 - 1)
    a["uv"], a["fr"] = ctypes.byref(_lib.D3MFragments(**uv_ok)), ctypes.byref(_lib.D3MFragments(**fr_ok))
    assert L.d3m_error_string(L.d3m_uv_bake_images_backward(*a.values(), None)) == b"workspace missing or too small"
    sv_bwd = dict(uv=True, fr=True, images=p, C=3, H=5, W=7, sv=p, V=6, persp=1, tol=ctypes.c_float(0.01), grad_texture=p, csr=True,
                  scratch=p, scratch_floats=1 << 30, grad_sv=p)
    run(L.d3m_uv_bake_vertices_backward, sv_bwd,
        records + sizes + [dict(images=None), dict(images=misaligned), dict(grad_texture=None), dict(grad_texture=misaligned),
                           dict(scratch=None), dict(scratch=misaligned), dict(grad_sv=None), dict(grad_sv=misaligned),
                           dict(csr=None), dict(uv_change=dict(visibility=None)), dict(uv_change=dict(visibility_size=16)),
                           dict(csr_change=dict(offsets=None)), dict(csr_change=dict(items=None)),
                           dict(csr_change=dict(num_rows=5)), dict(csr_change=dict(num_chunks=1, chunks=q)),
                           dict(csr_change=dict(num_long_rows=1, long_rows=q, long_chunk_ptr=q))])
    csr = _lib.D3MCsr(**csr_ok)
    assert L.d3m_uv_bake_scratch_floats(2, 4, ctypes.byref(csr)) == 2 * 4 * 9 + 2 * 4
    assert L.d3m_uv_bake_scratch_floats(0, 4, ctypes.byref(csr)) == 0 == L.d3m_uv_bake_scratch_floats(2, 4, None)
    a = dict(sv_bwd, scratch_floats=2 * 4 * 9 + 2 * 4 - 1)
    a["uv"], a["fr"], a["csr"] = (ctypes.byref(_lib.D3MFragments(**uv_ok)), ctypes.byref(_lib.D3MFragments(**fr_ok)),
                                  ctypes.byref(csr))
    assert L.d3m_error_string(L.d3m_uv_bake_vertices_backward(*a.values(), None)) == b"workspace missing or too small"
