"""The analytic edge antialiasing on the device (neural_renderer/antialias.py, csrc/d3m_antialias.h): forward and both
gradients against the float64 restatement of tests/antialias_scenes.py on the record's own maps, a closed-form known answer,
the paths that do nothing, determinism, launch counts, a captured step, the refusals, the Renderer's option and a small fit.
Tolerances (8 x the float32 yardstick measured on the CPU) and the fragile-pair rule: tests/antialias_scenes.py."""
import pytest
import torch

import antialias_scenes as AS
import fragment_geometry_scenes as FG
from conftest import kernels_launched
from vertex_attribute_scenes import VIEWING_ANGLE, fragment_maps, scene, seeded_attributes

pytestmark = pytest.mark.gpu
FORWARD = "k_antialias_images"
BACKWARD = "k_antialias_images_backward"
GATHER = {"k_antialias_face_sums", "k_antialias_large_face_sums", "k_vertex_attribute_adjoint_rows"}
CHUNKS = "k_vertex_attribute_adjoint_chunks"
U32 = 2.0 ** -24


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


_built = {}


def _case(name, S):
    """The scene on the device, computed once: renderer, vertices, faces, the screen vertices the record was made from, the
    Fragments (no anti-aliasing), its maps on the host."""
    from deep3dmap_amd import neural_renderer as nr
    if (name, S) not in _built:
        sc = scene(name)
        eyes = torch.from_numpy(sc["eyes"]).cuda()
        B = eyes.shape[0]
        r = nr.Renderer(camera_mode="look_at", image_size=S, anti_aliasing=False, viewing_angle=VIEWING_ANGLE)
        r.eye = eyes
        v = torch.from_numpy(sc["vertices"]).cuda()[None].repeat(B, 1, 1)
        faces = torch.from_numpy(sc["tri"]).cuda()[None]
        sv = r._transform(v, None, None, None, None, None).detach().contiguous()
        fr = nr.rasterize_fragments(sv, faces, S, False, r.fill_back, r.near, r.far)
        torch.cuda.synchronize()
        _built[(name, S)] = dict(r=r, v=v, faces=faces, sv=sv, fr=fr, maps=fragment_maps(fr), tri=sc["tri"], B=B, V=v.shape[1])
    return _built[(name, S)]


def _run(c, images, grad_out, image_grad=True, vertex_grad=True):
    """(out, grad_images, grad_sv) of the device node"""
    from deep3dmap_amd import neural_renderer as nr
    im = images.cuda().requires_grad_(image_grad)
    sv = c["sv"].clone().requires_grad_(vertex_grad)
    out = nr.antialias(im, c["fr"], sv)
    out.backward(grad_out.cuda())
    return out.detach(), im.grad, sv.grad


# ---- 1. forward and both gradients against the float64 reference -----------------------------------------------------------------
@pytest.mark.parametrize("name,S", AS.CASES)
def test_forward_and_gradients_against_the_float64_reference(name, S):
    c = _case(name, S)
    B = c["B"]
    if name == "S3B":                                                 # the workgroup route of stage 1, in both views
        for b in range(B):
            fi = c["maps"]["face_index_map"][b]
            assert int(torch.bincount(fi[fi >= 0].long()).max()) > 4096
    side = AS.side_opposite_of(c["tri"])
    for C in (1, 3, 9):
        images, g = AS.seeded_images(B, C, S), AS.seeded_grad_out(B, C, S)
        ref_out, keep, ref_gi, ref_gs = AS.reference(c["maps"], c["tri"], c["sv"], images, g, side=side)
        share = AS.left_out_share(keep)
        out, gi, gs = _run(c, images, g * keep)
        forward = float(((out.cpu().double() - ref_out).abs() * keep).max())
        e_gi, e_gs = FG.view_errors(gi, ref_gi), FG.view_errors(gs, ref_gs)
        print(name, S, "C =", C, "left out: %.4f" % share, "forward error: %.2e allowed: %.2e" % (forward, AS.FORWARD_TOLERANCE),
              "gradient errors / largest entry, image:", ["%.2e" % e for e in e_gi], "vertices:", ["%.2e" % e for e in e_gs],
              "allowed: %.2e" % AS.GRADIENT_TOLERANCE)
        assert share <= AS.MAX_LEFT_OUT
        assert float((ref_out - images.double()).abs().max()) > 0.05 and float(ref_gs.abs().max()) > 0
        assert bool(torch.isfinite(out).all()) and forward <= AS.FORWARD_TOLERANCE
        assert bool(torch.isfinite(gi).all()) and max(e_gi) <= AS.GRADIENT_TOLERANCE
        assert bool(torch.isfinite(gs).all()) and max(e_gs) <= AS.GRADIENT_TOLERANCE
        assert bool((_bits(gs[..., 2]) == 0).all())                   # the z gradient: an exact +0


# ---- 2. a closed-form known answer -------------------------------------------------------------------------------------------------
S_RECT = 16
PX = 2.0 / S_RECT


def _centre(i):
    return (2 * i + 1 - S_RECT) / S_RECT


def _rectangle(dx=0.0, right=0.3):
    """Screen vertices [1,7,3] and faces [1,3,3] of an axis-aligned rectangle of two triangles (diagonal from top left to
    bottom right: the triangle with the right and the top edge owns every pixel next to those edges) covering pixel columns
    and rows 4..11: left edge 0.4 pixel left of centre 4, right edge `right` pixel right of centre 11, bottom 0.4 below
    centre 4, top 0.3 above centre 11, shifted by dx pixels in x; and a sub-pixel triangle that covers no centre."""
    x0, x1 = _centre(4) - 0.4 * PX + dx * PX, _centre(11) + right * PX + dx * PX
    y0, y1 = _centre(4) - 0.4 * PX, _centre(11) + 0.3 * PX
    e = _centre(1) + 0.1 * PX
    sv = torch.tensor([[[x0, y0, 1.0], [x1, y0, 1.0], [x1, y1, 1.0], [x0, y1, 1.0],
                        [e, e, 1.0], [e + 0.3 * PX, e, 1.0], [e, e + 0.3 * PX, 1.0]]], dtype=torch.float32)
    faces = torch.tensor([[[0, 1, 3], [1, 2, 3], [4, 5, 6]]], dtype=torch.int32)
    return sv.cuda(), faces.cuda()


def _alpha_of(fr, sv):
    from deep3dmap_amd import neural_renderer as nr
    return nr.interpolate_vertex_attributes(torch.ones(sv.shape[1], 1, device="cuda"), fr)[1][:, None]


def test_rectangle_known_answer():
    from deep3dmap_amd import neural_renderer as nr
    base, faces = _rectangle()
    fr = nr.rasterize_fragments(base, faces, S_RECT, False)
    alpha = _alpha_of(fr, base)
    assert float(alpha.sum()) == 64.0                                 # columns and rows 4..11
    sv = base.clone().requires_grad_(True)
    out = nr.antialias(alpha, fr, sv)
    # coverage of the edge pixels: 1/2 + the edge's distance from the centre (0.3 right and top, 0.4 left and bottom)
    img = out.detach()[0, 0].flip(0)                                           # the maps' orientation: [y, x]
    assert abs(float(img[7, 11]) - 0.8) < 1e-5 and abs(float(img[11, 7]) - 0.8) < 1e-5
    assert abs(float(img[7, 4]) - 0.9) < 1e-5 and abs(float(img[4, 7]) - 0.9) < 1e-5
    assert float(img[7, 7]) == 1.0 and float(img[7, 12]) == 0.0 and float(img[7, 3]) == 0.0
    out.sum().backward()
    g = sv.grad[0]
    want = (S_RECT / 2) * 8                                          # (S / 2) R, R = 8 rows
    tol = 8 * U32 * want
    print("d sum / dx right edge:", float(g[1, 0] + g[2, 0]), "d sum / dy top edge:", float(g[2, 1] + g[3, 1]), "want:", want)
    assert abs(float(g[1, 0] + g[2, 0]) - want) <= tol                # the right edge's two vertices, in x
    assert abs(float(g[2, 1] + g[3, 1]) - want) <= tol                # the top edge's, in y
    assert bool((_bits(g[:, 2]) == 0).all())                          # z: an exact +0
    assert bool((_bits(g[4:]) == 0).all())                            # vertices on no silhouette pair: an exact +0


# ---- 3. paths that do nothing ---------------------------------------------------------------------------------------------------------
def _isolated_pairs(fi, F):
    """Horizontal pairs p = (x, y), q = (x + 1, y) of one view's face_index_map [S,S] whose tids differ while the three
    other neighbours of p have p's tid and those of q have q's: nothing but this pair can change either pixel."""
    S = fi.shape[0]
    tid = torch.where(fi >= 0, fi % F, torch.full_like(fi, -1)).tolist()
    found = []
    for y in range(1, S - 1):
        for x in range(1, S - 2):
            p, q = tid[y][x], tid[y][x + 1]
            if p != q and p >= 0 and q >= 0 and tid[y][x - 1] == tid[y - 1][x] == tid[y + 1][x] == p \
                    and tid[y][x + 2] == tid[y - 1][x + 1] == tid[y + 1][x + 1] == q:
                found.append((x, y))
    return found


def _wedge(third, z):
    """Triangles on the near-vertical edge P Q with the given third vertices (x, y) at depths z; P, Q at depth 2"""
    pts = [[0.003, -0.9, 2.0], [-0.003, 0.9, 2.0]] + [[x, y, zz] for (x, y), zz in zip(third, z)]
    tri = [[0, 2 + i, 1] if x > 0 else [0, 1, 2 + i] for i, ((x, y), _) in enumerate(zip(third, z))]
    return torch.tensor([pts], dtype=torch.float32).cuda(), torch.tensor([tri], dtype=torch.int32).cuda()


NOTHING = {
    # a flat quad of two triangles: the shared edge is interior
    "interior": lambda: _wedge([(-0.8, 0.0), (0.8, 0.05)], [2.0, 2.0]),
    # a fin: three triangles on one edge (-2 in the side table)
    "fin": lambda: _wedge([(-0.8, 0.0), (0.8, 0.05), (0.85, 0.6)], [2.0, 1.0, 3.0]),
    # two interpenetrating triangles: along their intersection the far pixel lies inside the near triangle
    "intersection": lambda: (torch.tensor([[[-0.8, -0.7, 1.0], [0.8, -0.6, 3.0], [0.0, 0.8, 2.0],
                                            [-0.8, -0.6, 3.0], [0.8, -0.7, 1.0], [0.0, 0.75, 2.0]]]).cuda(),
                             torch.tensor([[[0, 1, 2], [3, 4, 5]]], dtype=torch.int32).cuda()),
}


@pytest.mark.parametrize("what", sorted(NOTHING))
def test_pairs_that_do_nothing_keep_their_bits(what):
    from deep3dmap_amd import neural_renderer as nr
    from deep3dmap_amd.neural_renderer.antialias import build_side_opposite
    S = 16
    sv, faces = NOTHING[what]()
    table = build_side_opposite(faces, sv.shape[1]).tolist()
    if what == "interior":
        assert sorted(sum(table, [])) == [-1, -1, -1, -1, 2, 3]
    if what == "fin":
        assert sum(row.count(-2) for row in table) == 3
    fr = nr.rasterize_fragments(sv, faces, S, False)
    fi = fr.face_index_map[0].cpu().long()
    pairs = _isolated_pairs(fi, faces.shape[1])
    assert len(pairs) >= 2, (what, fi)
    images = AS.seeded_images(1, 3, S).cuda().requires_grad_(True)
    leaf = sv.clone().requires_grad_(True)
    out = nr.antialias(images, fr, leaf)
    assert not torch.equal(out.detach(), images.detach())             # the outline does blend
    for x, y in pairs:
        for xx in (x, x + 1):
            assert torch.equal(_bits(out[0, :, S - 1 - y, xx]), _bits(images[0, :, S - 1 - y, xx])), (what, x, y)
    # and such a pair passes the gradient straight through and gives the vertices none
    g = torch.zeros(1, 3, S, S, device="cuda")
    for x, y in pairs:
        g[0, :, S - 1 - y, x:x + 2] = torch.randn(3, 2, device="cuda")
    out.backward(g)
    assert torch.equal(_bits(images.grad), _bits(g)) and bool((_bits(leaf.grad) == 0).all())


# ---- 4. the same bits on every run ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,S", [("S4", 32), ("S3B", 128)])
def test_the_same_bits_on_every_run(name, S):
    c = _case(name, S)
    images, g = AS.seeded_images(c["B"], 9, S), AS.seeded_grad_out(c["B"], 9, S)
    first = _run(c, images, g)
    pad = torch.empty(12345, device="cuda")                          # (other addresses for the second run's buffers)
    second = _run(c, images, g)
    del pad
    for a, b in zip(first, second):
        assert float(a.abs().max()) > 0 and torch.equal(_bits(a), _bits(b))


# ---- 5. launch counts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,S", [("S2", 16), ("S4", 32)])
def test_launch_counts(name, S):
    from deep3dmap_amd import neural_renderer as nr
    c = _case(name, S)
    images, g = AS.seeded_images(c["B"], 3, S).cuda(), AS.seeded_grad_out(c["B"], 3, S).cuda()
    nr.antialias(images, c["fr"], c["sv"])                            # (the side table and the adjacency exist)
    with kernels_launched() as k:
        out = nr.antialias(images, c["fr"], c["sv"])
    assert {n: t[0] for n, t in k.times.items()} == {FORWARD: 1} and not out.requires_grad
    want = GATHER | ({CHUNKS} if name == "S4" else set())             # S4: a mesh with long rows
    for image_grad, vertex_grad in ((True, True), (False, True), (True, False)):
        im = images.clone().requires_grad_(image_grad)
        sv = c["sv"].clone().requires_grad_(vertex_grad)
        with kernels_launched() as k:
            out = nr.antialias(im, c["fr"], sv)
        assert {n: t[0] for n, t in k.times.items()} == {FORWARD: 1}
        with kernels_launched() as k:
            out.backward(g)
        counts = {n: t[0] for n, t in k.times.items()}
        assert counts == {n: 1 for n in ({BACKWARD} | want if vertex_grad else {BACKWARD})}, counts
        assert (im.grad is not None) == image_grad and (sv.grad is not None) == vertex_grad


# ---- 6. capture ----------------------------------------------------------------------------------------------------------------------
def test_captured_forward_and_backward(monkeypatch):
    from deep3dmap_amd import neural_renderer as nr
    from deep3dmap_amd.graph import CapturedStep
    from deep3dmap_amd.neural_renderer.antialias import SideOppositeCache
    from deep3dmap_amd.neural_renderer.row_gather import vertex_adjacency
    name, S = "S4", 32
    c = _case(name, S)
    fr, B = c["fr"], c["B"]
    values = [AS.seeded_grad_out(B, 3, S, seed=sd).cuda() for sd in (71, 72)]
    g = values[0].clone()
    images = AS.seeded_images(B, 3, S).cuda()
    twin = (images.clone().requires_grad_(True), c["sv"].clone().requires_grad_(True))
    live = (images.clone().requires_grad_(True), c["sv"].clone().requires_grad_(True))

    def step(im, sv):
        out = nr.antialias(im, fr, sv)
        return (out,) + torch.autograd.grad(out, (im, sv), g)

    step(*twin)                                                       # (the side table and the adjacency exist before the capture)
    eager = []
    for i in (0, 1):
        g.copy_(values[i])
        with kernels_launched() as k:
            eager.append([t.clone() for t in step(*twin)])
        assert k.names == {FORWARD, BACKWARD, CHUNKS} | GATHER, k.names
    assert not torch.equal(eager[0][2], eager[1][2]) and float(eager[1][2].abs().max()) > 0
    torch.cuda.synchronize()
    cs = CapturedStep(lambda: step(*live)).capture()
    for i in (1, 0, 1):
        g.copy_(values[i])
        got = [t.clone() for t in cs()]
        torch.cuda.synchronize()
        for a, b in zip(got, eager[i]):
            assert torch.equal(_bits(a), _bits(b)), i
    cs.release()
    # a first call under a capture with a tri the cache has not seen: refused, nothing launched
    unseen = fr._replace(tri=fr.tri.clone())
    vertex_adjacency(unseen.tri, c["V"])
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with kernels_launched() as k:
        with pytest.raises(RuntimeError, match="side table"):
            nr.antialias(images, unseen, c["sv"], cache=SideOppositeCache())
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    assert not k.names


# ---- 7. refusals before any launch ---------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    from deep3dmap_amd import neural_renderer as nr
    name, S = "S1", 16
    c = _case(name, S)
    fr, sv, B, V = c["fr"], c["sv"], c["B"], c["V"]
    images = AS.seeded_images(B, 3, S).cuda()
    r = nr.Renderer(camera_mode="look_at", image_size=S // 2, anti_aliasing=True, viewing_angle=VIEWING_ANGLE)
    r.eye = c["r"].eye
    pooled = r.fragments(c["v"], c["faces"])
    attr = seeded_attributes(name, 3, False).cuda()
    torch.cuda.synchronize()
    with kernels_launched() as k:
        with pytest.raises(ValueError, match="anti_aliasing"):
            nr.antialias(images[:, :, :S // 2, :S // 2].contiguous(), pooled, sv)
        for bad in (torch.rand(B, 0, S, S).cuda(), torch.rand(B, 1025, S, S).cuda(), images[:1], images[:, :, :-1], images[..., :-1],
                    images.double(), images.cpu(), images[0]):
            with pytest.raises(ValueError, match="images"):
                nr.antialias(bad, fr, sv)
        for bad in (sv[:, :-1], sv[:1], sv.double(), sv.cpu(), sv[..., :2]):
            with pytest.raises(ValueError, match="screen_vertices"):
                nr.antialias(images, fr, bad)
        with pytest.raises(ValueError, match="anti_aliasing=False"):
            r.render_attributes(c["v"], c["faces"], attr, antialias=True)
    assert not k.names, k.names


# ---- 8. the Renderer -------------------------------------------------------------------------------------------------------------------
def test_renderer_antialias_is_the_hand_written_composition():
    from deep3dmap_amd import neural_renderer as nr
    name, S = "S2", 32
    c = _case(name, S)
    r, faces, B = c["r"], c["faces"], c["B"]
    attr = seeded_attributes(name, 3, False).cuda()
    g, ga = FG.seeded_grad_images(B, 3, S).cuda(), FG.seeded_grad_images(B, 1, S)[:, 0].cuda()
    eyes = r.eye
    try:
        got = []
        for by_hand in (False, True):
            v = c["v"].clone().requires_grad_(True)
            r.eye = eyes.clone().requires_grad_(True)
            if not by_hand:
                images, alpha = r.render_attributes(v, faces, attr, antialias=True, geometry_grad=True)
            else:
                sv = r._transform(v, None, None, None, None, None)
                fr = nr.rasterize_fragments(sv.detach(), faces, r.image_size, r.anti_aliasing, r.fill_back, r.near, r.far)
                images, alpha = nr.interpolate_vertex_attributes(attr, fr, screen_vertices=sv)
                out = nr.antialias(torch.cat((images, alpha[:, None]), 1), fr, sv)
                images, alpha = out[:, :-1], out[:, -1]
            ((images * g).sum() + (alpha * ga).sum()).backward()
            got.append((images.detach(), alpha.detach(), v.grad, r.eye.grad))
        for a, b in zip(*got):
            assert torch.equal(_bits(a), _bits(b))
        images, alpha, gv, ge = got[0]
        assert images.shape == (B, 3, S, S) and alpha.shape == (B, S, S)
        assert bool(((alpha > 0) & (alpha < 1)).any())               # an antialiased silhouette
        assert bool(torch.isfinite(gv).all()) and float(gv.abs().max()) > 0 and float(ge.abs().max()) > 0
        # the silhouette gradient is there on top of the interior one
        v = c["v"].clone().requires_grad_(True)
        r.eye = eyes
        plain = r.render_attributes(v, faces, attr, geometry_grad=True)
        (plain[0] * g).sum().backward()
        assert not torch.equal(v.grad, gv)
        # the defaults: today's bits, and vertices that require grad are still refused
        with torch.no_grad():
            a = r.render_attributes(c["v"], faces, attr)
            b = nr.interpolate_vertex_attributes(attr, r.fragments(c["v"], faces))
        assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))
        assert torch.equal(_bits(plain[0]), _bits(a[0]))
        with pytest.raises(NotImplementedError, match="detach them"):
            r.render_attributes(v, faces, attr)
    finally:
        r.eye = eyes


# ---- 9. a small fit ------------------------------------------------------------------------------------------------------------------
def test_fitting_a_shifted_rectangle_through_the_silhouette():
    """A rectangle offset by 0.3 pixel from the target alpha image (the unshifted rectangle, antialiased by the node): twenty
    plain gradient steps on the silhouette L2 loss bring the offset below 0.05 pixel.  One translation d (in NDC) moves the
    four corners.  Step size: each of the R = 8 rows has a left and a right edge pixel whose value moves by S / 2 per unit of d,
    so the loss's curvature is 2 * 2 R (S / 2)^2 = R S^2 in the regime where one pixel per edge changes; half the Newton step."""
    from deep3dmap_amd import neural_renderer as nr
    target_sv, faces = _rectangle(right=0.35)
    fr = nr.rasterize_fragments(target_sv, faces, S_RECT, False)
    target = nr.antialias(_alpha_of(fr, target_sv), fr, target_sv)
    base, _ = _rectangle(dx=-0.3, right=0.35)
    d = torch.zeros(2, device="cuda", requires_grad=True)
    lr = 0.5 / (8 * S_RECT ** 2)
    move = torch.zeros(7, 3, device="cuda")
    move[:4, 0] = 1.0
    for step in range(20):
        sv = base + move[None] * d[0]
        fr = nr.rasterize_fragments(sv.detach(), faces, S_RECT, False)
        alpha = _alpha_of(fr, sv)
        assert not alpha.requires_grad                                # without the node: no gradient reaches the vertices
        loss = ((nr.antialias(alpha, fr, sv) - target) ** 2).sum()
        grad, = torch.autograd.grad(loss, d)
        with torch.no_grad():
            d -= lr * grad
        offset = abs(float(d[0]) / PX - 0.3)
        print("step", step, "loss %.5f" % float(loss), "offset in pixels %.4f" % offset)
    assert offset < 0.05
