"""Per-pixel spherical-harmonic shading of a UV albedo texture on the device (neural_renderer/sh_uv_fragments.py,
csrc/d3m_sh_uv_fragments.h) against the float64 restatement of tests/sh_uv_fragment_scenes.py on the record's own maps;
tolerances: sh_uv_fragment_scenes.DEVICE_TOLERANCE, 8 x the float32 yardstick of each kind (tests/test_sh_uv_fragments_host.py
holds the figures), the albedo image's gradient with the derived fixed-point term on top.

S3B/128 is the one case on the workgroup-per-face route of the normals' gather and has a view owned by fill_back copies; S4 has
slivers and hub vertices (the long-row chunks); the 32 x 16 texture catches swapped H and W; the pooled cases catch a product
taken after the pooling."""
import pytest
import torch

import fragment_geometry_scenes as FG
import sh_fragment_scenes as SF
import sh_uv_fragment_scenes as SU
import uv_texture_image_scenes as UV
import vertex_attribute_scenes as VA
from conftest import kernels_launched
from vertex_attribute_scenes import VIEWING_ANGLE, fragment_maps, image_size_of, scene

pytestmark = pytest.mark.gpu
FM_MAX_BBOX_AREA = 4096     # csrc/d3m_face_major.h
FORWARD, PIXELS, FINISH = "k_sh_uv_fragment_images", "k_sh_uv_fragment_backward_pixels", "k_sh_fragment_finish"
GATHER = {"k_vertex_attribute_face_sums", "k_vertex_attribute_large_face_sums", "k_vertex_attribute_adjoint_rows"}
SCATTER = {"k_uv_texture_images_clear_max", "k_uv_texture_images_scatter", "k_uv_texture_images_convert"}
GEOMETRY = {"k_fragment_geometry_face_sums", "k_fragment_geometry_large_face_sums", "k_vertex_attribute_adjoint_rows"}
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
        if name == "S3B":                                             # the workgroup route in both views, back copies in one
            for b in range(B):
                fi = maps["face_index_map"][b]
                assert int(torch.bincount(fi[fi >= 0].long()).max()) > FM_MAX_BBOX_AREA
            assert bool((maps["face_index_map"] >= sc["tri"].shape[0]).any())
        _built[key] = dict(r=r, v=v, faces=faces, sv=sv, fr=fr, maps=maps, tri=sc["tri"], B=B, V=v.shape[1],
                           s=image_size_of(S, aa), S=S)
    return _built[key]


def _leaf(t):
    return t.cuda().requires_grad_(True)


def _check(result, ref, kind, what, absolute=0.0):
    """per view: max |result - ref| <= DEVICE_TOLERANCE[kind] x the view's largest |ref| entry (+ absolute)"""
    assert result.shape == ref.shape and bool(torch.isfinite(result).all()), what
    r, f = result.detach().cpu().double(), ref.double()
    if f.dim() < 3 or kind == "albedo" and f.dim() == 3:              # a shared [V,3], [3,9] or [H,W,3]: as one view
        r, f = r[None], f[None]
    n = f.shape[0]
    scale = f.abs().reshape(n, -1).max(1).values
    diff = (r - f).abs().reshape(n, -1).max(1).values
    allowed = SU.DEVICE_TOLERANCE[kind] * scale + absolute
    print(what, kind, "error / largest entry:", ["%.2e" % e for e in (diff / scale).tolist()],
          "allowed: %.2e" % SU.DEVICE_TOLERANCE[kind])
    assert float(scale.min()) > 0 and bool((diff <= allowed).all()), (what, kind, (diff / scale).tolist())


# ---- 1. the image and the four gradients, every case, texture, uv case and normal kind; the layouts rotate ---------------------
@pytest.mark.parametrize("name,S,aa", SU.CASES)
def test_image_and_gradients_against_the_float64_reference(name, S, aa):
    from deep3dmap_amd import neural_renderer as nr
    c = _case(name, S, aa)
    fr, B, s, maps, tri = c["fr"], c["B"], c["s"], c["maps"], c["tri"]
    g, bg = SF.seeded_grad_out(B, s), VA.seeded_background(3)
    layouts, seen, i = SU.layouts(), set(), SU.CASES.index((name, S, aa))
    for (H, W), spread, wrapping in SU.uv_combos():
        uv = SU.faces_uv_of(name, spread)
        keep, share = FG.near_integer_mask(maps, tri, uv, H, W, aa, wrapping)
        assert share <= SU.MAX_ZEROED_SHARE, share
        for kind in SF.NORMAL_KINDS[name]:
            layout = layouts[i % len(layouts)]
            i += 1
            seen.add(layout)
            image, normals, sh = SU.inputs_of(name, kind, layout, H, W, B)
            a, n, l, sv = _leaf(image), _leaf(normals), _leaf(sh), c["sv"].clone().requires_grad_(True)
            images, alpha = nr.shade_uv_texture(a, uv.cuda(), n, l, fr, wrapping, bg.cuda(), screen_vertices=sv)
            # everything from one backward with the image gradient zeroed near texel boundaries (the vertices' is checked),
            # then the three that are continuous there from the whole image gradient
            masked = torch.autograd.grad(images, (a, n, l, sv), (g * keep).cuda(), retain_graph=True)
            ga, gn, gl = torch.autograd.grad(images, (a, n, l), g.cuda())
            ref = SU.reference(maps, tri, image, uv, normals, sh, c["sv"], g, aa, wrapping, bg, keep=keep)
            what = f"{name}/{S} aa={aa} {H}x{W} {spread} {wrapping} {kind} {layout}"
            assert images.shape == (B, 3, s, s) and alpha.shape == (B, s, s) and not alpha.requires_grad
            _check(images, ref["image"], "image", what)
            _check(gn, ref["normals"], "normals", what)
            _check(gl, ref["sh"], "sh", what)
            _check(ga, ref["albedo"], "albedo", what, SU.fixed_point_bound(maps, tri, normals, sh, g, aa))
            _check(masked[3], ref["screen_vertices"], "screen_vertices", what)
    assert len(seen) == len(layouts)


# ---- 2. alpha ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,S,aa", SU.CASES)
def test_alpha_has_the_bits_of_the_attribute_images_alpha(name, S, aa):
    from deep3dmap_amd import neural_renderer as nr
    c = _case(name, S, aa)
    normals = SF.cone_normals(name, False).cuda()
    _, alpha = nr.shade_uv_texture(SU.albedo_of(8, 8).cuda(), SU.faces_uv_of(name, "seamless").cuda(), normals,
                                   SF.seeded_sh().cuda(), c["fr"], background=0.25)
    _, want = nr.interpolate_vertex_attributes(normals, c["fr"])
    assert torch.equal(_bits(alpha), _bits(want)) and float(alpha.sum()) > 0


# ---- 3. the two nodes it joins ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,S,aa", [case for case in SU.CASES if not case[2]])
def test_without_supersampling_the_image_is_the_product_of_the_two_nodes(name, S, aa):
    from deep3dmap_amd import neural_renderer as nr
    c = _case(name, S, aa)
    fr, B = c["fr"], c["B"]
    for i, ((H, W), spread, wrapping) in enumerate(SU.uv_combos()):
        image, normals, sh = [t.cuda() for t in SU.inputs_of(name, "cone", SU.layouts()[i], H, W, B)]
        uv = SU.faces_uv_of(name, spread).cuda()
        got, alpha = nr.shade_uv_texture(image, uv, normals, sh, fr, wrapping)
        want = nr.shade_fragments(normals, sh, fr, colors=None, background=1.0)[0] * nr.sample_uv_texture(image, uv, fr, wrapping)[0]
        cov = (alpha > 0)[:, None].expand_as(got)
        assert int(cov.sum()) > 0
        zero = torch.zeros_like(got)
        _check(torch.where(cov, got, zero), torch.where(cov, want, zero).cpu().double(), "image", f"{name}/{S} {H}x{W} {spread} {wrapping}")


@pytest.mark.parametrize("name,S,aa", [("S1", 32, True), ("S2", 16, False), ("S3B", 128, False), ("S4", 32, False)])
def test_white_ambient_light_gives_the_picture_of_sample_uv_texture(name, S, aa):
    from deep3dmap_amd import neural_renderer as nr
    c = _case(name, S, aa)
    for (H, W), spread, wrapping in SU.uv_combos():
        image, uv = SU.albedo_of(H, W, c["B"]).cuda(), SU.faces_uv_of(name, spread).cuda()
        images, _ = nr.shade_uv_texture(image, uv, SF.cone_normals(name, True).cuda(), SF.white_ambient().cuda(), c["fr"], wrapping,
                                        background=0.5)
        want, _ = nr.sample_uv_texture(image, uv, c["fr"], wrapping, background=0.5)
        _check(images, want.cpu().double(), "image", f"{name}/{S} aa={aa} {H}x{W} {spread} {wrapping} white ambient")


# ---- 4. the rules of the image's gradient ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,S,aa", [("S1", 32, True), ("S4", 16, False)])
@pytest.mark.parametrize("batched", [False, True])
def test_image_gradient_rules(name, S, aa, batched):
    from deep3dmap_amd import neural_renderer as nr
    c = _case(name, S, aa)
    fr, B, s = c["fr"], c["B"], c["s"]
    (H, W), spread, wrapping = (32, 16), "seamless", "REPEAT"
    uv = SU.faces_uv_of(name, spread)
    normals, sh = SF.cone_normals(name, False).cuda(), SF.seeded_sh(B).cuda()

    def grad_for(g):
        a = _leaf(SU.albedo_of(H, W, B if batched else None))
        images, _ = nr.shade_uv_texture(a, uv.cuda(), normals, sh, fr, wrapping)
        images.backward(g.cuda())
        return a.grad

    zero = grad_for(torch.zeros(B, 3, s, s))
    assert bool((_bits(zero) == 0).all())                             # an exact +0, not -0
    g = SF.seeded_grad_out(B, s)
    g[B - 1, 1, s // 2, s // 3] = float("nan")
    assert bool(torch.isnan(grad_for(g)).all())
    # a texel that no pixel can reach, in float32 or float64: +0; one that some pixel reaches: touched
    reach = UV.reach_counts(c["maps"], c["tri"], uv, (B, H, W, 3) if batched else (H, W, 3), aa, wrapping)
    grad = grad_for(SF.seeded_grad_out(B, s)).cpu()
    untouched = (reach == 0)[..., None].expand_as(grad)
    assert int(untouched.sum()) > 0 and bool((_bits(grad[untouched]) == 0).all())
    assert bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0


# ---- 5. determinism and capture ----------------------------------------------------------------------------------------------------
def _step(nr, fr, uv, wrapping, a, n, l, sv, bg, g):
    images, alpha = nr.shade_uv_texture(a, uv, n, l, fr, wrapping, bg, screen_vertices=sv)
    return (images, alpha) + torch.autograd.grad(images, (a, n, l, sv), g)


@pytest.mark.parametrize("name,S,aa", [("S3B", 128, False), ("S4", 32, False), ("S1", 32, True)])
def test_two_runs_have_the_same_bits(name, S, aa):
    from deep3dmap_amd import neural_renderer as nr
    c = _case(name, S, aa)
    B = c["B"]
    g, bg = SF.seeded_grad_out(B, c["s"]).cuda(), VA.seeded_background(3).cuda()
    (H, W), spread, wrapping = (32, 16), "corners", "MIRRORED_REPEAT"
    uv = SU.faces_uv_of(name, spread).cuda()
    for layout in ((False, False, False), (True, True, True), (True, False, True)):
        runs = []
        for _ in range(2):
            a, n, l = [_leaf(t) for t in SU.inputs_of(name, "cone", layout, H, W, B)]
            runs.append(_step(nr, c["fr"], uv, wrapping, a, n, l, c["sv"].clone().requires_grad_(True), bg, g))
        for x, y in zip(*runs):
            assert torch.equal(_bits(x), _bits(y)), layout
        # a gradient asked for alone has the bits it has beside the others (the vertices alone: the pixel_grads entry point)
        for alone in (2, 3, 4, 5):                                    # index into _step's results
            leaves = [t.cuda() for t in SU.inputs_of(name, "cone", layout, H, W, B)] + [c["sv"].clone()]
            leaves[alone - 2].requires_grad_(True)
            images, _ = nr.shade_uv_texture(leaves[0], uv, leaves[1], leaves[2], c["fr"], wrapping, bg, screen_vertices=leaves[3])
            images.backward(g)
            assert torch.equal(_bits(leaves[alone - 2].grad), _bits(runs[0][alone])), (layout, alone)


def test_captured_forward_and_backward():
    """Forward plus backward captured (CapturedStep) with the record and the adjacency built beforehand: the replay has the
    bits of the eager step.  The captured step has leaves of its own that no eager call touches; the eager runs use twins."""
    from deep3dmap_amd import neural_renderer as nr
    from deep3dmap_amd.graph import CapturedStep
    name, S, aa = "S1", 32, True
    c = _case(name, S, aa)
    fr, B = c["fr"], c["B"]
    g, bg = SF.seeded_grad_out(B, c["s"]).cuda(), VA.seeded_background(3).cuda()
    (H, W), wrapping = (32, 16), "REPEAT"
    uv = SU.faces_uv_of(name, "corners").cuda()
    values = [[UV.seeded_image(H, W, 3, seed=sd).cuda(), SF.cone_normals(name, False, seed=sd).cuda(),
               SF.seeded_sh(B, seed=sd).cuda(), c["sv"].clone()] for sd in (71, 72)]
    twin = [t.clone().requires_grad_(True) for t in values[0]]
    live = [t.clone().requires_grad_(True) for t in values[0]]

    def step(leaves):
        return _step(nr, fr, uv, wrapping, leaves[0], leaves[1], leaves[2], leaves[3], bg, g)

    step(twin)                                                       # (the adjacency exists before the capture)
    eager = []
    for i in (0, 1):
        with torch.no_grad():
            for t, v in zip(twin[:3], values[i][:3]):
                t.copy_(v)
        eager.append([t.clone() for t in step(twin)])
    assert not torch.equal(eager[0][0], eager[1][0]) and float(eager[1][2].abs().max()) > 0
    torch.cuda.synchronize()
    cs = CapturedStep(lambda: step(live)).capture()
    for i in (1, 0, 1):
        with torch.no_grad():
            for t, v in zip(live[:3], values[i][:3]):
                t.copy_(v)
        got = [t.clone() for t in cs()]
        torch.cuda.synchronize()
        for x, y in zip(got, eager[i]):
            assert torch.equal(_bits(x), _bits(y)), i
    cs.release()


# ---- 6. launches -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S1", "S4"])
def test_launch_counts(name):
    from deep3dmap_amd import neural_renderer as nr
    S = 32
    c = _case(name, S, False)
    fr, B = c["fr"], c["B"]
    g = SF.seeded_grad_out(B, S).cuda()
    uv = SU.faces_uv_of(name, "seamless").cuda()
    hubs = 1 if name == "S4" else 0
    chunks = {CHUNKS} if hubs else set()

    def run(grads, sv=None, layout=(True, True, True)):
        """the kernels of the backward; grads: which of image, normals, sh require grad"""
        a, n, l = [t.cuda().requires_grad_(need) for t, need in zip(SU.inputs_of(name, "cone", layout, 32, 16, B), grads)]
        with kernels_launched() as kf:
            images, _ = nr.shade_uv_texture(a, uv, n, l, fr, screen_vertices=sv)
        with kernels_launched() as kb:
            images.backward(g)
        assert {k: v[0] for k, v in kf.times.items()} == {FORWARD: 1}, kf.times
        return {k: v[0] for k, v in kb.times.items()}

    for layout in ((True, True, True), (False, False, False)):
        # everything requires grad: the per-pixel launch, the finish, the normals' gather, the image's scatter
        counts = run((True, True, True), layout=layout)
        assert set(counts) == {PIXELS, FINISH} | GATHER | SCATTER | chunks and set(counts.values()) == {1}, counts
        assert sum(counts.values()) == 8 + hubs
    # one at a time: only what is wanted is written and gathered
    assert run((False, False, True)) == {PIXELS: 1, FINISH: 1}
    assert run((True, False, False)) == dict.fromkeys({PIXELS} | SCATTER, 1)
    assert run((False, True, False)) == dict.fromkeys({PIXELS} | GATHER | chunks, 1)
    assert run((True, False, True)) == dict.fromkeys({PIXELS, FINISH} | SCATTER, 1)
    # screen vertices that do not require grad: nothing extra; that do: the shared adjoint alone -- the node's pixel_grads
    # come out of the same per-pixel launch
    assert run((False, False, True), sv=c["sv"]) == {PIXELS: 1, FINISH: 1}
    counts = run((True, True, True), sv=c["sv"].clone().requires_grad_(True))
    assert set(counts) == {PIXELS, FINISH} | GATHER | SCATTER | GEOMETRY | chunks, counts
    assert counts[PIXELS] == 1 and counts["k_vertex_attribute_adjoint_rows"] == 2 and sum(counts.values()) == 11 + 2 * hubs, counts
    counts = run((False, False, False), sv=c["sv"].clone().requires_grad_(True))
    assert set(counts) == {PIXELS} | GEOMETRY | chunks and set(counts.values()) == {1} and sum(counts.values()) == 4 + hubs, counts


# ---- 7. the renderer and the light module --------------------------------------------------------------------------------------------
def test_render_uv_shaded_and_the_light_module():
    from deep3dmap_amd import neural_renderer as nr
    g = SF.seeded_grad_out(2, 32).cuda()
    for aa in (False, True):
        c = _case("S1", 32 if not aa else 64, aa)
        r, v, faces, B = c["r"], c["v"], c["faces"], c["B"]
        sh, image, uv = SF.seeded_sh(B).cuda(), SU.albedo_of(32, 16).cuda(), SU.faces_uv_of("S1", "corners").cuda()
        images, alpha = r.render_uv_shaded(v, faces, sh, image, uv, texture_wrapping="MIRRORED_REPEAT", background=0.5)
        fr = r.fragments(v, faces)
        want, want_alpha = nr.shade_uv_texture(image, uv, nr.vertex_normals(v, faces), sh, fr, "MIRRORED_REPEAT", 0.5)
        assert torch.equal(_bits(images), _bits(want)) and torch.equal(_bits(alpha), _bits(want_alpha))
        # geometry_grad: the pieces by hand -- the camera in the graph, the record of the detached vertices, screen_vertices=
        n = SF.cone_normals("S1", False).cuda()
        vv, vh = v.clone().requires_grad_(True), v.clone().requires_grad_(True)
        r.render_uv_shaded(vv, faces, sh, image, uv, normals=n, geometry_grad=True)[0].backward(g)
        svh = r._transform(vh, None, None, None, None, None)
        nr.shade_uv_texture(image, uv, n, sh, r.fragments(v, faces), screen_vertices=svh)[0].backward(g)
        assert float(vv.grad.abs().max()) > 0 and torch.equal(_bits(vv.grad), _bits(vh.grad))
        # normals=None: the light's gradient reaches the vertices through the smooth normals
        vv = v.clone().requires_grad_(True)
        r.render_uv_shaded(vv, faces, sh, image, uv)[0].backward(g)
        assert bool(torch.isfinite(vv.grad).all()) and float(vv.grad.abs().max()) > 0
        light = nr.SHLight(per_set=B).cuda()
        assert torch.equal(_bits(light.shade_uv_texture(image, uv, n, fr, background=0.5)[0]),
                           _bits(nr.shade_uv_texture(image, uv, n, light.sh, fr, background=0.5)[0]))
        if aa:
            with kernels_launched() as k:
                with pytest.raises(ValueError, match="anti_aliasing=False"):
                    r.render_uv_shaded(v, faces, sh, image, uv, antialias=True)
            assert not k.names, k.names
        else:                                                         # antialias: one nr.antialias call on the node's picture
            vv, vh = v.clone().requires_grad_(True), v.clone().requires_grad_(True)
            out, out_alpha = r.render_uv_shaded(vv, faces, sh, image, uv, normals=n, antialias=True)
            out.backward(g)
            svh = r._transform(vh, None, None, None, None, None)
            frh = r.fragments(v, faces)
            plain, plain_alpha = nr.shade_uv_texture(image, uv, n, sh, frh)
            by_hand = nr.antialias(torch.cat((plain, plain_alpha[:, None]), 1), frh, svh)
            by_hand[:, :3].backward(g)
            assert torch.equal(_bits(out), _bits(by_hand[:, :3])) and torch.equal(_bits(out_alpha), _bits(by_hand[:, 3]))
            assert float(vv.grad.abs().max()) > 0 and torch.equal(_bits(vv.grad), _bits(vh.grad))
