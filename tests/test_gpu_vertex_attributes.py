"""Per-vertex attribute images on the device (neural_renderer/attributes.py, csrc/d3m_attributes.h): the forward against the
float64 restatement evaluated on the device's own maps, alpha against render_silhouettes bit for bit, the fixed-order adjoint
against float64 autograd within the derived bound, bit identities, C = 3 against the texture-cube route, the UV position-map
recipe, a captured step, and the refusals.  Scenes, restatement and bounds: tests/vertex_attribute_scenes.py."""
import ctypes

import pytest
import torch

from conftest import kernels_launched
from vertex_attribute_scenes import (FORWARD_ROUNDINGS, U32, VIEWING_ANGLE, adjoint64, adjoint_bound, attribute_term_magnitude,
                                     cube_route_colors, fragment_maps, image_size_of, restate_attribute_images, scene,
                                     scene_cases, seeded_attributes, seeded_background)

pytestmark = pytest.mark.gpu
FM_MAX_BBOX_AREA = 4096     # csrc/d3m_face_major.h
FORWARD = {"k_vertex_attribute_images"}
BACKWARD = {"k_vertex_attribute_face_sums", "k_vertex_attribute_large_face_sums", "k_vertex_attribute_adjoint_rows"}
CHUNKS = "k_vertex_attribute_adjoint_chunks"


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _channels():
    from deep3dmap_amd.neural_renderer.attributes import CHANNEL_CHUNK
    return (1, CHANNEL_CHUNK, CHANNEL_CHUNK + 1, 2 * CHANNEL_CHUNK + 1)


_built = {}


def _case(name, S, aa, view=None):
    """The scene on the device, computed once: renderer, vertices [B,V,3], faces [1,F,3], the Fragments, its maps on the host;
    `view`: that view alone."""
    from deep3dmap_amd import neural_renderer as nr
    key = (name, S, aa, view)
    if key not in _built:
        sc = scene(name)
        eyes = torch.from_numpy(sc["eyes"] if view is None else sc["eyes"][view:view + 1]).cuda()
        B = eyes.shape[0]
        r = nr.Renderer(camera_mode="look_at", image_size=image_size_of(S, aa), anti_aliasing=aa, viewing_angle=VIEWING_ANGLE)
        r.eye = eyes
        v = torch.from_numpy(sc["vertices"]).cuda()[None].repeat(B, 1, 1)
        faces = torch.from_numpy(sc["tri"]).cuda()[None]
        fr = r.fragments(v, faces)
        torch.cuda.synchronize()
        _built[key] = dict(r=r, v=v, faces=faces, fr=fr, maps=fragment_maps(fr), tri=sc["tri"], B=B, V=v.shape[1],
                           s=image_size_of(S, aa))
    return _built[key]


def _assert_scene_property(name, c):
    """what each scene is there for, on the device's own maps"""
    fi, F = c["maps"]["face_index_map"], c["tri"].shape[0]
    owners = fi[fi >= 0]
    assert owners.numel() > 0 and int(owners.max()) < 2 * F
    if name == "S1":
        assert bool((owners >= F).all())                              # every owner is a reversed copy
    if name == "S2":
        assert bool((fi[0][fi[0] >= 0] < F).all()) and bool((fi[1][fi[1] >= 0] >= F).all())      # both owner kinds
    if name == "S3":
        assert int(torch.bincount(owners.long()).max()) > FM_MAX_BBOX_AREA                      # the large-face form
    if name == "S4":
        from deep3dmap_amd.neural_renderer.row_gather import CHUNK, LONG_ROW, vertex_adjacency
        A = vertex_adjacency(c["fr"].tri, c["V"])
        counts = (A.csr.offsets[1:] - A.csr.offsets[:-1]).cpu()
        assert {int(counts[h]) for h in scene(name)["notes"]["hubs"]} == {LONG_ROW, LONG_ROW + 1, 2 * CHUNK + 1}
        assert A.csr.num_chunks == 4


# ---- 1. forward -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,S,aa", scene_cases())
def test_forward_against_the_restatement(name, S, aa):
    from deep3dmap_amd import _lib, neural_renderer as nr
    c = _case(name, S, aa)
    _assert_scene_property(name, c)
    fr, B, V, s = c["fr"], c["B"], c["V"], c["s"]
    silhouettes = c["r"].render_silhouettes(c["v"], c["faces"])
    for C in _channels():
        bg = seeded_background(C)
        for batched in (False, True):
            attr = seeded_attributes(name, C, batched)
            with kernels_launched() as k:
                images, alpha = nr.interpolate_vertex_attributes(attr.cuda(), fr, bg.cuda())
            assert k.names == FORWARD, k.names
            assert images.shape == (B, C, s, s) and alpha.shape == (B, s, s) and not alpha.requires_grad
            want, want_alpha = restate_attribute_images(c["maps"], c["tri"], attr, bg, aa, torch.float64)
            mag = attribute_term_magnitude(c["maps"], c["tri"], attr, bg, aa)
            err = (images.double().cpu() - want).abs()
            print(name, S, aa, C, batched, "largest error / (U32 sum|terms|):", float((err / (U32 * mag)).max()))
            assert bool((err <= FORWARD_ROUNDINGS * U32 * mag).all())
            assert torch.equal(alpha.double().cpu(), want_alpha)
            assert torch.equal(_bits(alpha), _bits(silhouettes))
            # the C entry point, raw, on NaN-filled outputs: every element is written
            raw = torch.full((B, C, s, s), float("nan"), device="cuda")
            raw_alpha = torch.full((B, s, s), float("nan"), device="cuda")
            a_dev, bg_dev, c_fr = attr.cuda(), bg.cuda(), fr.c_struct()
            _lib.check(_lib.lib().d3m_vertex_attribute_images(ctypes.byref(c_fr), _lib.ptr(a_dev), B if batched else 1, V, C,
                                                              _lib.ptr(bg_dev), _lib.ptr(raw), _lib.ptr(raw_alpha),
                                                              _lib.stream_ptr()), "d3m_vertex_attribute_images")
            assert torch.equal(_bits(raw), _bits(images)) and torch.equal(_bits(raw_alpha), _bits(alpha))
    # no background: zeros; a float: every channel
    attr = seeded_attributes(name, 3, False).cuda()
    zero = nr.interpolate_vertex_attributes(attr, fr)[0]
    flat = nr.interpolate_vertex_attributes(attr, fr, 0.5)[0]
    same = nr.interpolate_vertex_attributes(attr, fr, torch.full((3,), 0.5).cuda())[0]
    assert torch.equal(_bits(flat), _bits(same))
    uncovered = (alpha == 0)[:, None].expand_as(zero)
    assert bool((zero[uncovered] == 0).all()) and bool((flat[uncovered] == 0.5).all())


# ---- 2. adjoint -----------------------------------------------------------------------------------------------------------
def _gradient(name, C, B, s):
    return torch.randn(B, C, s, s, generator=torch.Generator().manual_seed(17 + C))


@pytest.mark.parametrize("name,S,aa", scene_cases())
def test_adjoint_against_float64_autograd(name, S, aa):
    from deep3dmap_amd import neural_renderer as nr
    c = _case(name, S, aa)
    _assert_scene_property(name, c)
    fr, B, s = c["fr"], c["B"], c["s"]
    for C in _channels():
        g = _gradient(name, C, B, s)
        for batched in (False, True):
            attr = seeded_attributes(name, C, batched)
            a = attr.cuda().requires_grad_(True)
            images, alpha = nr.interpolate_vertex_attributes(a, fr, seeded_background(C).cuda())
            with kernels_launched() as k:
                images.backward(g.cuda())
            assert BACKWARD <= k.names <= BACKWARD | {CHUNKS} and (CHUNKS in k.names) == (name == "S4"), k.names
            ref, mag, count = adjoint64(c["maps"], c["tri"], attr, g, aa)
            assert float(ref.abs().max()) > 0
            if name == "S4":                                        # the hubs' long rows carry terms
                assert int(count[..., 0].max()) > 0 and int(count[..., 2].max()) > 0
            err = (a.grad.double().cpu() - ref).abs()
            bound = adjoint_bound(mag, count)
            print(name, S, aa, C, batched, "largest error / bound:", float((err / bound.clamp(min=1e-300)).max()))
            assert a.grad.shape == attr.shape and bool((err <= bound).all()), float((err - bound).max())


# ---- 3. bit properties ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,S,aa", [("S1", 32, True), ("S3", 128, False), ("S4", 32, False), ("S4", 32, True)])
def test_bit_properties(name, S, aa):
    from deep3dmap_amd import _lib, neural_renderer as nr
    from deep3dmap_amd.neural_renderer.row_gather import vertex_adjacency
    c = _case(name, S, aa)
    fr, B, V, s = c["fr"], c["B"], c["V"], c["s"]
    C = _channels()[2]
    g = _gradient(name, C, B, s).cuda()

    def grad_of(attr, fragments, grad):
        a = attr.cuda().requires_grad_(True)
        nr.interpolate_vertex_attributes(a, fragments)[0].backward(grad)
        return a.grad

    for batched in (False, True):
        attr = seeded_attributes(name, C, batched)
        first = grad_of(attr, fr, g)
        assert torch.equal(_bits(first), _bits(grad_of(attr, fr, g)))                     # two runs: the same bits
        # the C entry point, raw, on NaN-filled output and scratch: every element is written; a vertex that no pixel term
        # reaches (in no face, or in no visible face) gets an exact +0.0
        A = vertex_adjacency(fr.tri, V)
        n = int(_lib.lib().d3m_vertex_attribute_scratch_floats(B, fr.faces.shape[1], C, ctypes.byref(A.csr.c)))
        scratch = torch.full((n,), float("nan"), device="cuda")
        raw = torch.full(tuple(attr.shape), float("nan"), device="cuda")
        c_fr = fr.c_struct()
        _lib.check(_lib.lib().d3m_vertex_attribute_images_backward(
            ctypes.byref(c_fr), _lib.ptr(g), ctypes.byref(A.csr.c), _lib.ptr(scratch), n, _lib.ptr(raw), B if batched else 1,
            V, C, _lib.stream_ptr()), "d3m_vertex_attribute_images_backward")
        assert torch.equal(_bits(raw), _bits(first))
        count = adjoint64(c["maps"], c["tri"], attr, g, aa)[2]
        unreached = (count == 0).cuda()
        if name != "S3" and (batched or name == "S4"):              # (S4: the unused vertex; per view: the far side)
            assert int(unreached.sum()) > 0
        assert bool((_bits(raw)[unreached] == 0).all())
        if name == "S4":
            assert bool(unreached[..., scene(name)["notes"]["unused"]].all())
    # per-view attributes: the gradient of view b computed in the batch has the bits of the same view rendered alone
    if B > 1:
        attr = seeded_attributes(name, C, True)
        batch = grad_of(attr, fr, g)
        for b in range(B):
            alone = _case(name, S, aa, view=b)
            assert torch.equal(alone["maps"]["face_index_map"], c["maps"]["face_index_map"][b:b + 1])
            one = grad_of(attr[b:b + 1], alone["fr"], g[b:b + 1])
            assert torch.equal(_bits(one[0]), _bits(batch[b])), b


# ---- 4. C = 3 against the texture-cube route ------------------------------------------------------------------------------
@pytest.mark.parametrize("name,S,aa", [c for c in scene_cases() if c[0] in ("S1", "S2")])
def test_three_channels_against_the_texture_cube_route(name, S, aa):
    """Renderer.render_rgb over nr.textures_from_vertex_colors cubes with ambient light 1, directional 0 and the same
    background draws the same picture: every pixel within 64 U32 sum|terms|, the bound measured against the reference's
    sampler (tests/test_vertex_attributes_host.py), not against this code."""
    from deep3dmap_amd import neural_renderer as nr
    c = _case(name, S, aa)
    bg = [0.25, 0.5, 0.75]
    colors = cube_route_colors(c["V"])
    r = nr.Renderer(camera_mode="look_at", image_size=c["s"], anti_aliasing=aa, viewing_angle=VIEWING_ANGLE,
                    background_color=bg, light_intensity_ambient=1.0, light_intensity_directional=0.0)
    r.eye = c["r"].eye
    with torch.no_grad():
        want = r.render_rgb(c["v"], c["faces"], nr.textures_from_vertex_colors(colors.cuda(), c["faces"]))
        got, _ = r.render_attributes(c["v"], c["faces"], colors.cuda(), torch.tensor(bg).cuda())
    mag = attribute_term_magnitude(c["maps"], c["tri"], colors, torch.tensor(bg), aa)
    err = (got.double().cpu() - want.double().cpu()).abs()
    print(name, S, aa, "largest error / (U32 sum|terms|):", float((err / (U32 * mag)).max()))
    assert got.shape == want.shape == (c["B"], 3, c["s"], c["s"])
    assert bool((err <= 64 * U32 * mag).all())


# ---- 5. the UV position map (INTEGRATION.md's recipe) ---------------------------------------------------------------------
def test_uv_position_map_recipe():
    from deep3dmap_amd import neural_renderer as nr, synthetic
    n, B, s = 6, 2, 32
    v_np, tri_np = synthetic.grid_mesh(n)
    V = v_np.shape[0]
    vertices, tri = torch.from_numpy(v_np).cuda(), torch.from_numpy(tri_np).cuda()
    # the UV layout of the grid mesh: vertex (i, j) at (j, i) / (n - 1); rasterised ONCE as (u, v, const - z)
    i, j = torch.meshgrid(torch.arange(n), torch.arange(n), indexing="ij")
    uv = torch.stack([j, i], -1).reshape(V, 2).float().cuda() / (n - 1)
    layout = torch.cat([uv * 1.8 - 0.9, 3.0 - vertices[:, 2:3]], 1)
    fr = nr.rasterize_fragments(layout[None].repeat(B, 1, 1), tri, s, anti_aliasing=False)
    maps = fragment_maps(fr)
    covered = int((maps["face_index_map"] >= 0).sum())
    assert covered > B * 0.7 * s * s
    # every step: pose -> position image -> loss
    pose = torch.tensor([[1.1, 0.2, -0.3, 0.1, 0.05, -0.02, 0.03], [0.9, -0.4, 0.5, 0.2, -0.1, 0.04, 0.0]]).cuda().requires_grad_(True)
    with kernels_launched() as k:
        posed = nr.pose_vertices(vertices, pose)[0]
        image, alpha = nr.interpolate_vertex_attributes(posed, fr)
    assert FORWARD <= k.names and not {"k_bid_faces", "k_bin_count"} & k.names, k.names      # coverage is not run again
    want, _ = restate_attribute_images(maps, tri_np, posed.detach().cpu(), None, False, torch.float64)
    mag = attribute_term_magnitude(maps, tri_np, posed.detach().cpu(), None, False)
    at_covered = (alpha > 0)[:, None].expand_as(image).cpu()
    err = (image.double().cpu() - want).abs()
    assert image.shape == (B, 3, s, s) and bool((err <= FORWARD_ROUNDINGS * U32 * mag)[at_covered].all())
    target = torch.rand(B, 3, s, s, generator=torch.Generator().manual_seed(4)).cuda()
    posed.retain_grad()
    loss = (((image - target) ** 2) * alpha[:, None]).sum()
    loss.backward()
    g = (2 * (image - target) * alpha[:, None]).detach()
    ref, mag, count = adjoint64(maps, tri_np, posed.detach(), g, False)
    err = (posed.grad.double().cpu() - ref).abs()
    assert posed.grad.shape == (B, V, 3) and bool((err <= adjoint_bound(mag, count)).all())
    assert pose.grad.shape == (B, 7) and bool(torch.isfinite(pose.grad).all()) and bool((pose.grad.abs().amax(1) > 0).all())


# ---- 6. capture -----------------------------------------------------------------------------------------------------------
def test_captured_forward_and_backward():
    """Forward plus backward captured (CapturedStep: torch.cuda.graph on the step's own stream) with the Fragments and the
    adjacency built beforehand; the replay has the bits of the eager run.  The captured step has a leaf of its own that no
    eager call ever touches (graph.py: a leaf used on another stream first makes autograd wait across streams inside the
    capture); the eager runs use a twin."""
    from deep3dmap_amd import neural_renderer as nr
    from deep3dmap_amd.graph import CapturedStep
    name, S, aa = "S1", 32, True
    c = _case(name, S, aa)
    fr, C = c["fr"], _channels()[2]
    values = [seeded_attributes(name, C, True, seed=sd).cuda() for sd in (5, 6)]
    twin = values[0].clone().requires_grad_(True)
    live = values[0].clone().requires_grad_(True)
    g = _gradient(name, C, c["B"], c["s"]).cuda()
    bg = seeded_background(C).cuda()

    def step(attr):
        images, alpha = nr.interpolate_vertex_attributes(attr, fr, bg)
        grad, = torch.autograd.grad(images, attr, g)
        return images, alpha, grad

    step(twin)                                                       # (the adjacency exists before the capture)
    with kernels_launched() as k:
        eager = [[t.clone() for t in step(twin)]]
    assert k.names == FORWARD | BACKWARD, k.names                    # nothing but the node's own kernels
    with torch.no_grad():
        twin.copy_(values[1])
    eager.append([t.clone() for t in step(twin)])
    assert not torch.equal(eager[0][0], eager[1][0]) and float(eager[1][2].abs().max()) > 0
    torch.cuda.synchronize()
    cs = CapturedStep(lambda: step(live)).capture()
    for i in (1, 0, 1):
        with torch.no_grad():
            live.copy_(values[i])
        got = [t.clone() for t in cs()]
        torch.cuda.synchronize()
        for a, b in zip(got, eager[i]):
            assert torch.equal(_bits(a), _bits(b)), i
    cs.release()


# ---- 7. errors ------------------------------------------------------------------------------------------------------------
def test_refusals():
    from deep3dmap_amd import neural_renderer as nr
    c = _case("S1", 16, False)
    fr, r, v, faces, V = c["fr"], c["r"], c["v"], c["faces"], c["V"]
    ok = torch.rand(V, 3).cuda()
    with kernels_launched() as k:
        for bad in (torch.rand(V - 1, 3).cuda(), torch.rand(V + 1, 3).cuda(), ok.cpu(), ok.double(), ok.half(),
                    torch.rand(V, 0).cuda(), torch.rand(V, 1025).cuda(), torch.rand(3, V, 3).cuda(), torch.rand(V).cuda()):
            with pytest.raises(ValueError):
                nr.interpolate_vertex_attributes(bad, fr)
        with pytest.raises(ValueError, match="background"):
            nr.interpolate_vertex_attributes(ok, fr, torch.rand(3, device="cuda", requires_grad=True))
        with pytest.raises(ValueError, match="background"):
            nr.interpolate_vertex_attributes(ok, fr, torch.rand(3))                       # on the host
        with pytest.raises(ValueError):                                                  # per-view topology
            r.fragments(v, faces.repeat(2, 1, 1))
        with pytest.raises(ValueError):
            r.render_attributes(v, faces.repeat(2, 1, 1), ok)
        with pytest.raises(NotImplementedError, match="detach them: an attribute image carries no geometry gradient"):
            r.fragments(v.clone().requires_grad_(True), faces)
        with pytest.raises(NotImplementedError, match="detach them"):
            r.render_attributes(v.clone().requires_grad_(True), faces, ok)
        with pytest.raises(NotImplementedError, match="detach them"):
            nr.rasterize_fragments(v.clone().requires_grad_(True), faces, 16)
        # a record whose maps do not belong together never reaches a launch
        with pytest.raises(ValueError):
            nr.interpolate_vertex_attributes(ok, fr._replace(face_index_map=fr.face_index_map[:1]))
        with pytest.raises(ValueError):
            nr.interpolate_vertex_attributes(ok, fr._replace(fill_back=False))
    assert not {n for n in k.names if n.startswith("k_vertex_attribute")}, k.names
    with torch.no_grad():                                            # no gradient is asked for: a plain render
        images, alpha = r.render_attributes(v.clone().requires_grad_(True), faces, ok, 1.0)
    assert images.shape == (2, 3, 16, 16) and float(alpha.sum()) == 2 * 88
