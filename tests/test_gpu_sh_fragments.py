"""Per-pixel spherical-harmonic shading of fragment images on the device (neural_renderer/sh_fragments.py,
csrc/d3m_sh_fragments.h) against the float64 restatement of tests/sh_fragment_scenes.py on the record's own maps; tolerances:
sh_fragment_scenes.DEVICE_TOLERANCE, 8 x the float32 yardstick of each kind (tests/test_sh_fragments_host.py holds the figures).

The light's sum tree (N = 27, 1024 pixels a part, at most 256 parts): S1 / S2 / S4 at 16 reach ONE PARTLY FILLED part (256 of
1024 elements; at 32 the part is full), S3B/128 reaches SEVERAL parts (16, every lane striding over four elements).  The cap of
256 parts lies at S = 512, beyond these cases: tests/test_sh_fragments_host.py walks the striding loop beyond the cap in the
numpy replay of tests/set_sums_replay.py.  S3B/128 also has faces that own more than 4096 pixels in both views (the gather's
workgroup route), S4 has hub vertices (the long-row chunks)."""
import pytest
import torch

import sh_fragment_scenes as SF
import vertex_attribute_scenes as VA
from conftest import kernels_launched
from vertex_attribute_scenes import VIEWING_ANGLE, fragment_maps, image_size_of, scene

pytestmark = pytest.mark.gpu
FM_MAX_BBOX_AREA = 4096     # csrc/d3m_face_major.h
PIXELS, FINISH = "k_sh_fragment_backward_pixels", "k_sh_fragment_finish"
GATHER = {"k_vertex_attribute_face_sums", "k_vertex_attribute_large_face_sums", "k_vertex_attribute_adjoint_rows"}
GEOMETRY = {"k_fragment_geometry_face_sums", "k_fragment_geometry_large_face_sums"}
CHUNKS = "k_vertex_attribute_adjoint_chunks"


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


_built = {}


def _case(name, S, aa):
    """The scene on the device, computed once: renderer, vertices, faces, the screen vertices the record was made from, the
    Fragments, its maps on the host."""
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
            for b in range(B):
                fi = maps["face_index_map"][b]
                assert int(torch.bincount(fi[fi >= 0].long()).max()) > FM_MAX_BBOX_AREA
        _built[key] = dict(r=r, v=v, faces=faces, sv=sv, fr=fr, maps=maps, tri=sc["tri"], B=B, V=v.shape[1],
                           s=image_size_of(S, aa), S=S)
    return _built[key]


def _inputs(name, kind, config, B):
    nb, sb, col = config
    return (SF.normals_of(name, kind, nb), SF.seeded_sh(B if sb else None),
            None if col is None else SF.seeded_colors(name, col == "batched"))


def _leaf(t):
    return None if t is None else t.cuda().requires_grad_(True)


def _check(result, ref, kind, what):
    assert result.shape == ref.shape and bool(torch.isfinite(result).all()), what
    errors, allowed = SF.errors_of(result, ref), SF.DEVICE_TOLERANCE[kind]
    print(what, kind, "error / largest entry:", ["%.2e" % e for e in errors], "allowed: %.2e" % allowed)
    assert float(ref.abs().max()) > 0 and max(errors) <= allowed, (what, kind, errors)


def _backward_names(name, sh=True, vertex=True, geometry=False):
    want = {PIXELS} | ({FINISH} if sh else set()) | (GATHER if vertex else set()) | \
        (GEOMETRY | {"k_vertex_attribute_adjoint_rows"} if geometry else set())
    return want | ({CHUNKS} if name == "S4" and (vertex or geometry) else set())


# ---- 1. the image and the four gradients, every case and every layout of the inputs ------------------------------------------
@pytest.mark.parametrize("name,S,aa", SF.CASES)
def test_image_and_gradients_against_the_float64_reference(name, S, aa):
    from deep3dmap_amd import neural_renderer as nr
    c = _case(name, S, aa)
    fr, B, s = c["fr"], c["B"], c["s"]
    g = SF.seeded_grad_out(B, s)
    bg = VA.seeded_background(3)
    for kind in SF.NORMAL_KINDS[name]:
        for config in SF.input_configs():
            normals, sh, colors = _inputs(name, kind, config, B)
            n, l, col, sv = _leaf(normals), _leaf(sh), _leaf(colors), c["sv"].clone().requires_grad_(True)
            images, alpha = nr.shade_fragments(n, l, fr, col, bg.cuda(), screen_vertices=sv)
            images.backward(g.cuda())
            ref = SF.reference(c["maps"], c["tri"], normals, sh, colors, c["sv"], g, aa, bg)
            what = f"{name}/{S} aa={aa} {kind} {config}"
            assert images.shape == (B, 3, s, s) and alpha.shape == (B, s, s) and not alpha.requires_grad
            _check(images, ref["image"], "image", what)
            _check(n.grad, ref["normals"], "normals", what)
            _check(l.grad, ref["sh"], "sh", what)
            if colors is not None:
                _check(col.grad, ref["colors"], "colors", what)
            _check(sv.grad, ref["screen_vertices"], "screen_vertices", what)


# ---- 2. alpha ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,S,aa", SF.CASES)
def test_alpha_has_the_bits_of_the_attribute_images_alpha(name, S, aa):
    from deep3dmap_amd import neural_renderer as nr
    c = _case(name, S, aa)
    normals = SF.cone_normals(name, False).cuda()
    _, alpha = nr.shade_fragments(normals, SF.seeded_sh().cuda(), c["fr"], background=0.25)
    _, want = nr.interpolate_vertex_attributes(normals, c["fr"])
    assert torch.equal(_bits(alpha), _bits(want)) and float(alpha.sum()) > 0


# ---- 3. white ambient light: the picture is the interpolated albedo -----------------------------------------------------------------
@pytest.mark.parametrize("name,S,aa", [("S1", 32, True), ("S2", 16, False), ("S4", 32, False)])
def test_white_ambient_light_gives_the_attribute_image_of_the_colours(name, S, aa):
    from deep3dmap_amd import neural_renderer as nr
    c = _case(name, S, aa)
    colors = SF.seeded_colors(name, True).cuda()
    images, _ = nr.shade_fragments(SF.cone_normals(name, True).cuda(), SF.white_ambient().cuda(), c["fr"], colors)
    want, _ = nr.interpolate_vertex_attributes(colors, c["fr"])
    _check(images, want.cpu().double(), "image", f"{name}/{S} white ambient")


# ---- 4. the clamp branch: a known answer -------------------------------------------------------------------------------------------
def test_all_zero_normals_take_the_clamp_branch():
    """m = 0: n = 0 / 1e-6 = 0, so s_k = a0 sh[k,0] exactly, and dL/dm = dL/dn / 1e-6 with dL/dn = sum_k g_k a1 (sh[k,1],
    sh[k,2], sh[k,3]): the normals' gradient is the attribute adjoint of that gradient image."""
    from deep3dmap_amd import neural_renderer as nr
    from deep3dmap_amd.neural_renderer.smooth_shading import SH_A
    name, S = "S1", 32
    c = _case(name, S, False)
    fr, B, V = c["fr"], c["B"], c["V"]
    sh = SF.seeded_sh(B)
    n = torch.zeros(V, 3, device="cuda", requires_grad=True)
    images, alpha = nr.shade_fragments(n, sh.cuda(), fr)
    want = (torch.tensor(SH_A[0], dtype=torch.float32) * sh[:, :, 0])[:, :, None, None].expand(B, 3, S, S)     # one float32 product
    cov = (alpha.cpu() > 0)[:, None].expand(B, 3, S, S)
    assert int(cov.sum()) > 0 and torch.equal(_bits(images.cpu()[cov]), _bits(want[cov]))
    assert bool((_bits(images.cpu()[~cov]) == 0).all())
    g = SF.seeded_grad_out(B, S)
    images.backward(g.cuda())
    G = torch.einsum("bkyx,bki->biyx", g.double(), sh[:, :, 1:4].double()) * SH_A[1] / 1e-6
    ref = VA.adjoint64(c["maps"], c["tri"], torch.zeros(V, 3), G, False)[0]
    _check(n.grad, ref, "normals", "zero normals")


# ---- 5. the composed route -------------------------------------------------------------------------------------------------------
def _composed(nr, normals, sh, colors, fr):
    """interpolate_vertex_attributes of the normals, torch's normalisation, nr.sh_basis, the contraction with sh -- that
    contraction in float64, so that the light's gradient of THIS side (a library matrix product over all pixels otherwise)
    adds no float32 summation error of its own and the fused node is held to the device tolerance"""
    m, alpha = nr.interpolate_vertex_attributes(normals, fr)
    m = m.permute(0, 2, 3, 1)
    r = torch.sqrt((m[..., 0] * m[..., 0] + m[..., 1] * m[..., 1]) + m[..., 2] * m[..., 2])
    H = nr.sh_basis(m / r.clamp(min=1e-6)[..., None])                 # [B,s,s,9]
    shb = sh if sh.dim() == 3 else sh[None].expand(m.shape[0], 3, 9)
    shade = torch.einsum("bkj,byxj->bkyx", shb.double(), H.double()).float()
    if colors is not None:
        shade = shade * nr.interpolate_vertex_attributes(colors, fr)[0]
    return shade * alpha[:, None]


@pytest.mark.parametrize("name,S", [("S1", 32), ("S3B", 128), ("S4", 32)])
def test_against_the_composed_route(name, S):
    from deep3dmap_amd import neural_renderer as nr
    c = _case(name, S, False)
    fr, B = c["fr"], c["B"]
    g = SF.seeded_grad_out(B, S).cuda()
    for config in ((False, False, "shared"), (True, True, "batched"), (True, False, None)):
        normals, sh, colors = _inputs(name, "cone", config, B)
        fused = [_leaf(t) for t in (normals, sh, colors)]
        got = nr.shade_fragments(fused[0], fused[1], fr, fused[2])[0]
        got.backward(g)
        comp = [_leaf(t) for t in (normals, sh, colors)]
        image = _composed(nr, comp[0], comp[1], comp[2], fr)
        image.backward(g)
        _check(got, image.detach().cpu().double(), "image", f"{name}/{S} composed {config}")
        for a, b, kind in zip(fused, comp, ("normals", "sh", "colors")):
            if a is not None:
                _check(a.grad, b.grad.cpu().double(), kind, f"{name}/{S} composed {config}")


# ---- 6. determinism and capture ----------------------------------------------------------------------------------------------------
def _step(nr, fr, n, l, col, sv, bg, g):
    images, alpha = nr.shade_fragments(n, l, fr, col, bg, screen_vertices=sv)
    return (images, alpha) + torch.autograd.grad(images, (n, l, col, sv), g)


@pytest.mark.parametrize("name,S,aa", [("S3B", 128, False), ("S4", 32, False), ("S1", 32, True)])
def test_two_runs_have_the_same_bits(name, S, aa):
    from deep3dmap_amd import neural_renderer as nr
    c = _case(name, S, aa)
    B = c["B"]
    g, bg = SF.seeded_grad_out(B, c["s"]).cuda(), VA.seeded_background(3).cuda()
    for config in ((False, False, "shared"), (True, True, "batched"), (False, True, "batched")):
        runs = []
        for _ in range(2):
            n, l, col = [_leaf(t) for t in _inputs(name, "cone", config, B)]
            runs.append(_step(nr, c["fr"], n, l, col, c["sv"].clone().requires_grad_(True), bg, g))
        for a, b in zip(*runs):
            assert torch.equal(_bits(a), _bits(b)), config
        # a gradient asked for alone (its own gather of three channels) has the bits it has beside the others
        for alone in (2, 4):                                          # index into _step's results: normals, colours
            n, l, col = [t.cuda() for t in _inputs(name, "cone", config, B)]
            (n if alone == 2 else col).requires_grad_(True)
            images, _ = nr.shade_fragments(n, l, c["fr"], col, bg)
            images.backward(g)
            assert torch.equal(_bits((n if alone == 2 else col).grad), _bits(runs[0][alone])), (config, alone)


def test_captured_forward_and_backward():
    """Forward plus backward captured (CapturedStep) with the record and the adjacency built beforehand: the replay has the
    bits of the eager step.  The captured step has leaves of its own that no eager call touches; the eager runs use twins."""
    from deep3dmap_amd import neural_renderer as nr
    from deep3dmap_amd.graph import CapturedStep
    name, S, aa = "S1", 32, True
    c = _case(name, S, aa)
    fr, B = c["fr"], c["B"]
    g, bg = SF.seeded_grad_out(B, c["s"]).cuda(), VA.seeded_background(3).cuda()
    values = [[SF.cone_normals(name, False, seed=sd).cuda(), SF.seeded_sh(B, seed=sd).cuda(),
               SF.seeded_colors(name, False, seed=sd).cuda(), c["sv"].clone()] for sd in (71, 72)]
    twin = [t.clone().requires_grad_(True) for t in values[0]]
    live = [t.clone().requires_grad_(True) for t in values[0]]

    def step(leaves):
        return _step(nr, fr, leaves[0], leaves[1], leaves[2], leaves[3], bg, g)

    step(twin)                                                       # (the adjacency exists before the capture)
    eager = []
    for i in (0, 1):
        with torch.no_grad():
            for t, v in zip(twin[:3], values[i][:3]):
                t.copy_(v)
        eager.append([t.clone() for t in step(twin)])
    assert not torch.equal(eager[0][0], eager[1][0]) and float(eager[1][3].abs().max()) > 0
    torch.cuda.synchronize()
    cs = CapturedStep(lambda: step(live)).capture()
    for i in (1, 0, 1):
        with torch.no_grad():
            for t, v in zip(live[:3], values[i][:3]):
                t.copy_(v)
        got = [t.clone() for t in cs()]
        torch.cuda.synchronize()
        for a, b in zip(got, eager[i]):
            assert torch.equal(_bits(a), _bits(b)), i
    cs.release()


# ---- 7. launches -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S1", "S4"])
def test_launch_counts(name):
    from deep3dmap_amd import neural_renderer as nr
    S = 32
    c = _case(name, S, False)
    fr, B = c["fr"], c["B"]
    g = SF.seeded_grad_out(B, S).cuda()
    hubs = 1 if name == "S4" else 0

    def run(config, grads, sv=None):
        """the kernels of the forward and of the backward; grads: which of normals, sh, colors require grad"""
        n, l, col = [None if t is None else t.cuda().requires_grad_(need) for t, need in zip(_inputs(name, "cone", config, B), grads)]
        with kernels_launched() as kf:
            images, _ = nr.shade_fragments(n, l, fr, col, screen_vertices=sv)
        with kernels_launched() as kb:
            images.backward(g)
        assert {k: v[0] for k, v in kf.times.items()} == {"k_sh_fragment_images": 1}, kf.times
        return {k: v[0] for k, v in kb.times.items()}

    # everything requires grad, one batch size: the per-pixel launch, the finish, one gather
    counts = run((True, True, "batched"), (True, True, True))
    assert set(counts) == _backward_names(name) and sum(counts.values()) == 5 + hubs and set(counts.values()) == {1}, counts
    assert run((False, False, None), (True, True, True)) == counts
    # colours of another batch size than the normals': a second gather
    counts = run((False, True, "batched"), (True, True, True))
    assert set(counts) == _backward_names(name) and sum(counts.values()) == 8 + 2 * hubs, counts
    assert counts[PIXELS] == counts[FINISH] == 1
    # the light alone: no gather; the normals alone, beside colours that need none: no finish, one gather of three channels
    assert run((True, True, "batched"), (False, True, False)) == {PIXELS: 1, FINISH: 1}
    for grads in ((True, False, False), (False, False, True)):
        counts = run((True, True, "batched"), grads)
        assert set(counts) == _backward_names(name, sh=False) and sum(counts.values()) == 4 + hubs, counts
    # screen vertices that do not require grad: nothing extra; that do: the shared adjoint alone -- the node's pixel_grads
    # come out of the same per-pixel launch
    assert run((True, True, "batched"), (False, True, False), sv=c["sv"]) == {PIXELS: 1, FINISH: 1}
    counts = run((True, True, "batched"), (True, True, True), sv=c["sv"].clone().requires_grad_(True))
    assert set(counts) == _backward_names(name, geometry=True), counts
    assert counts[PIXELS] == 1 and counts["k_vertex_attribute_adjoint_rows"] == 2 and sum(counts.values()) == 8 + 2 * hubs, counts
    counts = run((True, True, "batched"), (False, False, False), sv=c["sv"].clone().requires_grad_(True))
    assert set(counts) == _backward_names(name, sh=False, vertex=False, geometry=True), counts
    assert sum(counts.values()) == 4 + hubs and set(counts.values()) == {1}, counts


# ---- 8. the renderer ---------------------------------------------------------------------------------------------------------------
def test_render_sh_shaded():
    from deep3dmap_amd import neural_renderer as nr
    c = _case("S1", 32, False)
    r, v, faces, B = c["r"], c["v"], c["faces"], c["B"]
    sh, colors = SF.seeded_sh(B).cuda(), SF.seeded_colors("S1", False).cuda()
    images, alpha = r.render_sh_shaded(v, faces, sh, colors, background=0.5)
    fr = r.fragments(v, faces)
    want, want_alpha = nr.shade_fragments(nr.vertex_normals(v, faces), sh, fr, colors, 0.5)
    assert torch.equal(_bits(images), _bits(want)) and torch.equal(_bits(alpha), _bits(want_alpha))
    g = SF.seeded_grad_out(B, 32).cuda()
    # the light's gradient reaches the vertices through the normals; geometry_grad and antialias each add their own
    grads = {}
    for key, kw in (("normals", {}), ("geometry", dict(geometry_grad=True)), ("antialias", dict(antialias=True))):
        vv = v.clone().requires_grad_(True)
        out, _ = r.render_sh_shaded(vv, faces, sh, colors, **kw)
        out.backward(g)
        grads[key] = vv.grad
        assert bool(torch.isfinite(vv.grad).all()) and float(vv.grad.abs().max()) > 0, key
    assert not torch.equal(grads["geometry"], grads["normals"]) and not torch.equal(grads["antialias"], grads["normals"])
    # given normals: the vertices get a gradient from geometry_grad / antialias alone
    n = SF.cone_normals("S1", False).cuda()
    for kw in (dict(geometry_grad=True), dict(antialias=True)):
        vv = v.clone().requires_grad_(True)
        r.render_sh_shaded(vv, faces, sh, colors, normals=n, **kw)[0].backward(g)
        assert bool(torch.isfinite(vv.grad).all()) and float(vv.grad.abs().max()) > 0, kw
    ra = _case("S1", 32, True)["r"]
    with kernels_launched() as k:
        with pytest.raises(ValueError, match="anti_aliasing=False"):
            ra.render_sh_shaded(v, faces, sh, colors, antialias=True)
    assert not k.names, k.names


# ---- 9. a small fit ----------------------------------------------------------------------------------------------------------------
def test_fitting_the_light_is_reproducible():
    """30 Adam steps on the light from white ambient toward the picture of a seeded light: the loss falls below a tenth of
    its start, and two fits have the same loss history bit for bit."""
    from deep3dmap_amd import neural_renderer as nr
    c = _case("S1", 32, False)
    fr = c["fr"]
    normals, colors = SF.smooth_normals("S1", False).cuda(), SF.seeded_colors("S1", False).cuda()
    with torch.no_grad():
        target, _ = nr.shade_fragments(normals, SF.seeded_sh().cuda(), fr, colors)
    histories = []
    for _ in range(2):
        light = nr.SHLight().cuda()
        opt = torch.optim.Adam(light.parameters(), lr=0.2)         # (the float32 restatement on the CPU reaches 0.02 of the start)
        losses = []
        for _ in range(30):
            opt.zero_grad()
            images, _ = light.shade(normals, fr, colors)
            loss = ((images - target) ** 2).mean()
            loss.backward()
            opt.step()
            losses.append(loss.detach())
        histories.append(torch.stack(losses))
    print("loss: start %.3e end %.3e" % (float(histories[0][0]), float(histories[0][-1])))
    assert float(histories[0][-1]) < 0.1 * float(histories[0][0])
    assert torch.equal(_bits(histories[0]), _bits(histories[1]))
