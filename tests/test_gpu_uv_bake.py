"""View images baked into a uv texture on the device (neural_renderer/uv_bake.py, csrc/d3m_uv_bake.h) against the float64
restatement of tests/uv_bake_scenes.py on the two records' own maps and the device's own screen vertices; tolerances:
uv_bake_scenes.DEVICE_TOLERANCE, 8 x the float32 yardstick of each kind (tests/test_uv_bake_host.py holds the figures).  The
mask must be the reference's wherever the reference's decision is at least the margin away from its thresholds; within the
margin the device's decision is accepted and the reference is evaluated with it (uv_bake_scenes, NEAR A THRESHOLD)."""
import pytest
import torch

import fragment_geometry_scenes as FG
import uv_bake_scenes as UB
from conftest import kernels_launched
from vertex_attribute_scenes import VIEWING_ANGLE, image_size_of, scene

pytestmark = pytest.mark.gpu
FORWARD = "k_uv_bake_texture"
IMAGES = {"k_uv_texture_images_clear_max", "k_uv_bake_images_scatter", "k_uv_texture_images_convert"}
VERTICES = {"k_uv_bake_view_flags", "k_uv_bake_face_sums", "k_uv_bake_large_face_sums", "k_vertex_attribute_adjoint_rows"}
CHUNKS = "k_vertex_attribute_adjoint_chunks"


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


_built = {}


def _case(case):
    """The case on the device, computed once: the view record and the screen vertices it was made from, the layout record,
    both records' maps on the host, the inputs."""
    from deep3dmap_amd import neural_renderer as nr
    if case not in _built:
        name, layout, T, S, aa, H, W, C, persp = case
        sc = scene(name)
        eyes = torch.from_numpy(sc["eyes"]).cuda()
        B = eyes.shape[0]
        r = nr.Renderer(camera_mode="look_at", image_size=image_size_of(S, aa), anti_aliasing=aa, viewing_angle=VIEWING_ANGLE,
                        perspective=persp)
        r.eye = eyes
        v = torch.from_numpy(sc["vertices"]).cuda()[None].repeat(B, 1, 1)
        faces = torch.from_numpy(sc["tri"]).cuda()[None]
        sv = r._transform(v, None, None, None, None, None).detach().contiguous()
        fr = nr.rasterize_fragments(sv, faces, r.image_size, aa, r.fill_back, r.near, r.far)
        a = UB.case_inputs(case)
        faces_uv = a["faces_uv"].cuda()
        uv_fr = nr.uv_layout_fragments(faces_uv, T)
        torch.cuda.synchronize()
        _built[case] = dict(a, r=r, v=v, faces=faces, sv=sv, fr=fr, uv_fr=uv_fr, faces_uv_dev=faces_uv, B=B,
                            background_dev=a["background"].cuda(),
                            view_maps=UB.record_maps(fr), uv_maps=UB.record_maps(uv_fr))
    return _built[case]


def _check(result, ref, kind, what):
    assert result.shape == ref.shape and bool(torch.isfinite(result).all()), what
    errors, allowed = FG.view_errors(result, ref), UB.DEVICE_TOLERANCE[kind]
    print(what, kind, "error / largest entry:", ["%.2e" % e for e in errors], "allowed: %.2e" % allowed)
    assert float(ref.abs().max()) > 0 and max(errors) <= allowed, (what, kind, errors)


# ---- 1. texture, mask and both gradients, every case ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", UB.CASES, ids=UB.case_id)
def test_texture_mask_and_gradients_against_the_float64_reference(case):
    from deep3dmap_amd import neural_renderer as nr
    c = _case(case)
    name, layout, T, S, aa, H, W, C, persp = case
    B, what = c["B"], UB.case_id(case)
    args = (c["uv_maps"], c["view_maps"], c["tri"], c["sv"], c["images"], c["grad_texture"], persp, UB.DEPTH_TOLERANCE,
            c["background"])
    first = UB.reference(*args)
    near_v, near_c = UB.near_threshold(first["info"], UB.M_POS, UB.M_Z)
    share = float((near_v | near_c).sum()) / float(first["info"]["covered"].sum())
    print(what, "share of covered texel-views near a threshold: %.4f" % share)
    assert share <= UB.MAX_NEAR_SHARE, share

    images, sv = c["images"].cuda().requires_grad_(True), c["sv"].clone().requires_grad_(True)
    texture, mask = nr.bake_uv_texture(images, c["uv_fr"], c["fr"], sv, persp, UB.DEPTH_TOLERANCE, c["background"].cuda())
    assert texture.shape == (B, T, T, C) and mask.shape == (B, T, T) and not mask.requires_grad
    got_mask = mask.cpu()
    assert bool(((got_mask == 0) | (got_mask == 1)).all())
    got_visible = got_mask > 0
    differ = got_visible != first["mask"]
    assert not bool((differ & ~near_v).any()), int((differ & ~near_v).sum())
    # within the margin the device's decision stands; near a cell boundary the output gradient is taken out
    decisions = dict(UB.decisions_of(first["info"]), visible=torch.where(near_v, got_visible, first["mask"]))
    g = c["grad_texture"] * (~near_c)[..., None]
    ref = UB.reference(*args[:5], g, *args[6:], decisions=decisions)
    texture.backward(g.cuda())
    assert int(got_visible.sum()) > 0
    _check(texture, ref["texture"], "texture", what)
    _check(images.grad, ref["images"], "images", what)
    _check(sv.grad, ref["screen_vertices"], "screen_vertices", what)
    if not persp:
        assert float(sv.grad[..., 2].abs().max()) == 0.0
    # a texel outside every uv triangle: the background, mask 0
    outside = ~first["info"]["covered"]
    assert int(outside.sum()) > 0 and not bool(got_visible[outside].any())
    assert torch.equal(texture.detach().cpu()[outside], c["background"].expand(int(outside.sum()), C))


# ---- 2. an independent composition on the device --------------------------------------------------------------------------------
def test_values_against_interpolated_positions_and_grid_sample():
    """Orthographic: the surface point is the barycentric mix of the corners' x, y -- interpolate_vertex_attributes of the
    unrolled screen vertices over the layout record -- and the lookup is torch's grid_sample at (x, -y) with
    align_corners=False and border padding."""
    from deep3dmap_amd import neural_renderer as nr
    case = UB.CASES[2]
    assert not case[8]
    c = _case(case)
    name, layout, T, S, aa, H, W, C, persp = case
    B = c["B"]
    images = c["images"].cuda()
    texture, mask = nr.bake_uv_texture(images, c["uv_fr"], c["fr"], c["sv"], False, UB.DEPTH_TOLERANCE)
    corners = c["faces"][0].reshape(-1).long()                        # the unrolled mesh: vertex 3 f + c of the layout
    attr = c["sv"][:, corners, :2].permute(1, 0, 2).reshape(-1, 2 * B).contiguous()
    xy, _ = nr.interpolate_vertex_attributes(attr, c["uv_fr"])        # [1, 2B, T, T], rows reversed
    xy = xy[0].flip(1).reshape(B, 2, T, T)
    grid = torch.stack((xy[:, 0], -xy[:, 1]), -1)
    want = torch.nn.functional.grid_sample(images, grid, mode="bilinear", padding_mode="border", align_corners=False)
    want = want.permute(0, 2, 3, 1)
    visible = mask > 0
    assert int(visible.sum()) > 50
    sel = visible[..., None].expand_as(want)
    errors = FG.view_errors(torch.where(sel, texture, torch.zeros_like(want)), torch.where(sel, want, torch.zeros_like(want)).cpu())
    print("against grid_sample, error / largest entry:", ["%.2e" % e for e in errors])
    assert max(errors) <= UB.DEVICE_TOLERANCE["texture"], errors


# ---- 3. the same bits on every run, eager and captured ----------------------------------------------------------------------------
def _step(nr, c, case, images, sv, g):
    texture, mask = nr.bake_uv_texture(images, c["uv_fr"], c["fr"], sv, case[8], UB.DEPTH_TOLERANCE, c["background_dev"])
    return (texture, mask) + torch.autograd.grad(texture, (images, sv), g)


@pytest.mark.parametrize("case", [UB.CASES[1], UB.CASES[3], UB.CASES[4]], ids=UB.case_id)
def test_two_runs_have_the_same_bits(case):
    from deep3dmap_amd import neural_renderer as nr
    c = _case(case)
    g = c["grad_texture"].cuda()
    runs = [_step(nr, c, case, c["images"].cuda().requires_grad_(True), c["sv"].clone().requires_grad_(True), g) for _ in range(3)]
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(_bits(a), _bits(b))
    # the images' gradient asked for alone has the bits it has beside the vertices'
    images = c["images"].cuda().requires_grad_(True)
    nr.bake_uv_texture(images, c["uv_fr"], c["fr"], c["sv"], case[8], UB.DEPTH_TOLERANCE)[0].backward(g)
    assert torch.equal(_bits(images.grad), _bits(runs[0][2]))


def test_captured_forward_and_backward():
    from deep3dmap_amd import neural_renderer as nr
    from deep3dmap_amd.graph import CapturedStep
    case = UB.CASES[0]
    c = _case(case)
    B, C, H, W = c["images"].shape
    g = c["grad_texture"].cuda()
    values = [UB.seeded_images(B, C, H, W, seed=sd).cuda() for sd in (83, 84)]
    twin = [values[0].clone().requires_grad_(True), c["sv"].clone().requires_grad_(True)]
    live = [values[0].clone().requires_grad_(True), c["sv"].clone().requires_grad_(True)]
    _step(nr, c, case, twin[0], twin[1], g)                           # (the adjacency exists before the capture)
    eager = []
    for i in (0, 1):
        with torch.no_grad():
            twin[0].copy_(values[i])
        eager.append([t.clone() for t in _step(nr, c, case, twin[0], twin[1], g)])
    assert not torch.equal(eager[0][0], eager[1][0]) and float(eager[1][3].abs().max()) > 0
    torch.cuda.synchronize()
    cs = CapturedStep(lambda: _step(nr, c, case, live[0], live[1], g)).capture()
    for i in (1, 0, 1):
        with torch.no_grad():
            live[0].copy_(values[i])
        got = [t.clone() for t in cs()]
        torch.cuda.synchronize()
        for a, b in zip(got, eager[i]):
            assert torch.equal(_bits(a), _bits(b)), i
    cs.release()


def test_zero_and_non_finite_output_gradients():
    from deep3dmap_amd import neural_renderer as nr
    case = UB.CASES[0]
    c = _case(case)
    for fill, check in ((0.0, lambda t: torch.equal(_bits(t), torch.zeros_like(_bits(t)))),
                        (float("inf"), lambda t: bool(torch.isnan(t).all()))):
        images = c["images"].cuda().requires_grad_(True)
        texture, _ = nr.bake_uv_texture(images, c["uv_fr"], c["fr"], c["sv"], case[8])
        g = torch.zeros_like(texture)
        g[0, 3, 4, 0] = fill
        texture.backward(g)
        assert check(images.grad), fill


# ---- 4. launches -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [UB.CASES[0], UB.CASES[4]], ids=UB.case_id)
def test_launch_counts(case):
    from deep3dmap_amd import neural_renderer as nr
    c = _case(case)
    g = c["grad_texture"].cuda()
    hubs = {CHUNKS} if case[0] == "S4" else set()

    def run(images_grad, sv_grad):
        images, sv = c["images"].cuda().requires_grad_(images_grad), c["sv"].clone().requires_grad_(sv_grad)
        with kernels_launched() as kf:
            texture, _ = nr.bake_uv_texture(images, c["uv_fr"], c["fr"], sv, case[8])
        assert {k: v[0] for k, v in kf.times.items()} == {FORWARD: 1}, kf.times
        if not (images_grad or sv_grad):
            assert not texture.requires_grad
            return {}
        with kernels_launched() as kb:
            texture.backward(g)
        return {k: v[0] for k, v in kb.times.items()}

    assert run(False, False) == {}
    assert run(True, False) == dict.fromkeys(IMAGES, 1)               # vertices that need no gradient: nothing extra
    assert run(False, True) == dict.fromkeys(VERTICES | hubs, 1)
    assert run(True, True) == dict.fromkeys(IMAGES | VERTICES | hubs, 1)


# ---- 5. the renderer ---------------------------------------------------------------------------------------------------------------
def test_renderer_bake_uv_texture():
    from deep3dmap_amd import neural_renderer as nr
    case = UB.CASES[0]
    c = _case(case)
    name, layout, T, S, aa, H, W, C, persp = case
    r, v, faces = c["r"], c["v"], c["faces"]
    images, g = c["images"].cuda(), c["grad_texture"].cuda()
    texture, mask = r.bake_uv_texture(v, faces, images, c["faces_uv_dev"], T, background=0.5)
    want, want_mask = nr.bake_uv_texture(images, c["uv_fr"], c["fr"], c["sv"], True, 1e-2, 0.5)
    assert torch.equal(_bits(texture), _bits(want)) and torch.equal(_bits(mask), _bits(want_mask))
    vv, im = v.clone().requires_grad_(True), images.clone().requires_grad_(True)
    out, _ = r.bake_uv_texture(vv, faces, im, c["faces_uv_dev"], T, geometry_grad=True)
    out.backward(g)
    assert bool(torch.isfinite(vv.grad).all()) and float(vv.grad.abs().max()) > 0
    assert bool(torch.isfinite(im.grad).all()) and float(im.grad.abs().max()) > 0
    vv = v.clone().requires_grad_(True)
    out, _ = r.bake_uv_texture(vv, faces, images, c["faces_uv_dev"], T)
    assert not out.requires_grad                                      # without geometry_grad the vertices are constants
    # fusing the views: sum mask texture / sum mask
    fused = (mask[..., None] * texture).sum(0) / mask.sum(0).clamp(min=1)[..., None]
    assert fused.shape == (T, T, C) and bool(torch.isfinite(fused).all())
