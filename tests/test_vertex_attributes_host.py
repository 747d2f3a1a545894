"""Per-vertex attribute images (neural_renderer/attributes.py), host side: the scenes' coverage through the CPU oracle with
the properties the GPU tests rely on, the element-wise restatement (tests/vertex_attribute_scenes.py) pinned analytically on
an orthographic planar patch and cross-checked against the reference rasterizer's render of vcolor_to_texture_cube cubes,
argument errors that need no device, and the adjacency's reuse through the cache."""
import numpy as np
import pytest
import torch

from vertex_attribute_scenes import (U32, adjoint64, adjoint_bound, attribute_term_magnitude, cube_route_colors, oracle_maps,
                                     pixel_weights,
                                     restate_attribute_images, scene, seeded_attributes)

FM_MAX_BBOX_AREA = 4096     # csrc/d3m_face_major.h


def _owned(maps):
    fi = maps["face_index_map"]
    return [int((fi[b] >= 0).sum()) for b in range(fi.shape[0])]


# ---- 1. the scenes have the properties the tests rely on ------------------------------------------------------------------
def test_scene_properties():
    F1 = scene("S1")["tri"].shape[0]
    for S, covered in ((16, 88), (32, 344)):
        m = oracle_maps("S1", S)
        fi = m["face_index_map"]
        assert _owned(m) == [covered, covered]
        assert bool((fi[fi >= 0] >= F1).all())                       # every owner is a reversed copy
    per_view = [torch.unique(fi[b][fi[b] >= 0]) for b in range(2)]
    assert len(per_view[0]) + len(per_view[1]) == 44 and 2 * F1 == 160
    F2 = scene("S2")["tri"].shape[0]
    for S, covered in ((16, [64, 64]), (32, [256, 250])):
        m = oracle_maps("S2", S)
        fi = m["face_index_map"]
        assert _owned(m) == covered
        assert bool((fi[0][fi[0] >= 0] < F2).all()) and bool((fi[1][fi[1] >= 0] >= F2).all())    # both owner kinds
    assert len(torch.unique(fi[fi >= 0])) == 36
    m = oracle_maps("S3", 128)
    counts = torch.bincount(m["face_index_map"][m["face_index_map"] >= 0].reshape(-1))
    assert int(counts.max()) == 7508 and int(counts.max()) > FM_MAX_BBOX_AREA
    sc = scene("S4")
    from deep3dmap_amd.neural_renderer.row_gather import CHUNK, LONG_ROW
    valence = np.bincount(sc["tri"].reshape(-1), minlength=257)
    assert {int(valence[h]) for h in sc["notes"]["hubs"]} == {LONG_ROW, LONG_ROW + 1, 2 * CHUNK + 1}
    assert valence[sc["notes"]["unused"]] == 0 and sc["vertices"].shape == (257, 3)
    m = oracle_maps("S4", 32)
    assert min(_owned(m)) > 100


# ---- 2. the analytic pin of the restatement -------------------------------------------------------------------------------
@pytest.mark.parametrize("anti_aliasing", [False, True])
def test_restatement_is_affine_on_an_orthographic_planar_patch(anti_aliasing):
    """A flat patch in z = 0 seen along the z axis without perspective: screen (x, y) = world (x, y), every corner has the
    same depth, so an image of the 3D positions holds, at each covered pixel, the NDC coordinates of its centre and z = 0."""
    S = 32 if anti_aliasing else 16
    sc = scene("planar")
    maps = oracle_maps("planar", S, perspective=False)
    pos = torch.from_numpy(sc["vertices"]).double()
    img, alpha = restate_attribute_images(maps, sc["tri"], pos, None, anti_aliasing, torch.float64)
    s = 16
    centre = (2.0 * torch.arange(s, dtype=torch.float64) + 1.0 - s) / s          # NDC centre of output column / row (from the bottom)
    want_x = centre[None, :].expand(s, s)
    want_y = centre.flip(0)[:, None].expand(s, s)                                # (row 0 is the top)
    inside = alpha[0] == 1.0                                                     # (pooled: all four internal pixels covered)
    assert int(inside.sum()) >= 100
    assert float((img[0, 0] - want_x)[inside].abs().max()) <= 1e-6
    assert float((img[0, 1] - want_y)[inside].abs().max()) <= 1e-6
    assert float(img[0, 2][inside].abs().max()) <= 1e-6


# ---- 3. the restatement against the reference rasterizer on the CPU -------------------------------------------------------
@pytest.mark.parametrize("name,S", [("S1", 16), ("S1", 32), ("S2", 16), ("S2", 32), ("S3", 128)])
def test_restatement_matches_the_reference_render_of_colour_cubes(name, S):
    """C = 3: the restatement in float32 against the oracle's sampler (reference kernels restated in C, fill_back, eps 1e-3)
    on vcolor_to_texture_cube cubes of the same colours (cube_route_colors: why they stay away from 0).  Figures: at most
    16 U32 sum_c|u_c a_c| when the bound was set; 8.7 U32 sum|terms| with these colours (S1: 5.5 and 5.4, S2: 5.3 and 6.6,
    S3: 8.7); no pixel has a u_c above 1 - 1e-3 (asserted: the sampler's clamp never fires).  Allowed: 64 U32 sum|terms|,
    four times the 16, because the device sampler contracts FMAs."""
    from oracle import nr_oracle as O
    from test_vertex_colors_host import restate_cubes
    sc = scene(name)
    B, tri = sc["eyes"].shape[0], torch.from_numpy(sc["tri"]).long()
    colors = cube_route_colors(sc["vertices"].shape[0])
    maps = oracle_maps(name, S)
    u, cov, _ = pixel_weights(maps, tri)
    assert float(u[cov].max()) <= 1.0 - 1e-3
    cubes = restate_cubes(colors[None], tri).repeat(B, 1, 1, 1, 1, 1)
    cubes = torch.cat((cubes, cubes.permute(0, 1, 4, 3, 2, 5)), 1)
    bg = (0.25, 0.5, 0.75)
    m = O.raster_forward(maps["faces"].numpy(), cubes.numpy(), S, 0.1, 100, 1e-3, bg, True, True, False)
    want = torch.from_numpy(m["rgb_map"]).permute(0, 3, 1, 2).flip(2)
    got, _ = restate_attribute_images(maps, tri, colors, torch.tensor(bg), False, torch.float32)
    mag = attribute_term_magnitude(maps, tri, colors, torch.tensor(bg), False)
    err = (got.double() - want.double()).abs()
    print(name, S, "largest error / (U32 sum|terms|):", float((err / (U32 * mag).clamp(min=1e-300)).max()))
    assert bool((err <= 64 * U32 * mag).all())


# ---- 4. the adjoint's reference is the adjoint of the restatement ---------------------------------------------------------
def test_adjoint_reference_and_bound_shapes():
    sc = scene("S2")
    maps = oracle_maps("S2", 16)
    for batched in (False, True):
        a = seeded_attributes("S2", 3, batched)
        g = torch.randn(2, 3, 16, 16, generator=torch.Generator().manual_seed(1))
        ref, mag, count = adjoint64(maps, sc["tri"], a, g, False)
        assert ref.shape == mag.shape == a.shape and count.shape == a.shape[:-1]
        assert int(count.sum()) == 3 * 128 and bool((mag >= ref.abs() - 1e-12).all())
        assert adjoint_bound(mag, count).shape == a.shape
        # <images(a), g> = <a, adjoint(g)>: the map is linear in the attributes
        img, _ = restate_attribute_images(maps, sc["tri"], a.double(), None, False, torch.float64)
        assert abs(float((img * g.double()).sum()) - float((a.double() * ref).sum())) <= 1e-9


# ---- 5. argument errors that need no device -------------------------------------------------------------------------------
def _host_fragments(B=2, V=6, F=2, s=4, anti_aliasing=False, fill_back=True):
    from deep3dmap_amd import neural_renderer as nr
    S = 2 * s if anti_aliasing else s
    Fp = 2 * F if fill_back else F
    return nr.Fragments(torch.full((B, S, S), -1, dtype=torch.int32), torch.zeros(B, S, S, 3), torch.zeros(B, S, S),
                        torch.zeros(B, Fp, 3, 3), torch.zeros(64, dtype=torch.uint8),
                        torch.tensor([[0, 1, 2], [3, 4, 5]], dtype=torch.int32)[:F], fill_back, s, anti_aliasing, V)


def test_argument_errors():
    from deep3dmap_amd import neural_renderer as nr
    from deep3dmap_amd.neural_renderer import attributes as at
    assert at.CHANNEL_CHUNK == 8 and nr.interpolate_vertex_attributes is at.interpolate_vertex_attributes
    fr = _host_fragments()
    ok = torch.rand(6, 3)
    bad = [torch.rand(6), torch.rand(1, 2, 6, 3), ok.double(), ok.half(), ok.numpy(), torch.rand(6, 0), torch.rand(6, 1025),
           torch.rand(5, 3), torch.rand(7, 3), torch.rand(3, 6, 3), torch.rand(1, 6, 3)]
    for a in bad:
        with pytest.raises(ValueError):
            nr.interpolate_vertex_attributes(a, fr)
    with pytest.raises(ValueError, match="vertices"):
        nr.interpolate_vertex_attributes(torch.rand(5, 3), fr)
    with pytest.raises(ValueError, match="Fragments"):
        nr.interpolate_vertex_attributes(ok, tuple(fr))
    with pytest.raises(ValueError, match="fit"):                     # maps that do not fit one another
        nr.interpolate_vertex_attributes(ok, fr._replace(weight_map=torch.zeros(2, 4, 4, 2)))
    with pytest.raises(ValueError, match="fit"):
        nr.interpolate_vertex_attributes(ok, fr._replace(anti_aliasing=True))
    with pytest.raises(ValueError, match="fit"):
        nr.interpolate_vertex_attributes(ok, fr._replace(tri=fr.tri.long()))
    for bg in (torch.rand(3, requires_grad=True), torch.rand(2), torch.rand(3).double(), [1.0, 2.0]):
        with pytest.raises(ValueError, match="background"):
            nr.interpolate_vertex_attributes(ok, fr, bg)
    with pytest.raises(ValueError, match="GPU"):                     # everything on the host: nothing to run on
        nr.interpolate_vertex_attributes(ok, fr, 0.5)
    # rasterize_fragments
    sv, faces = torch.rand(2, 6, 3), torch.tensor([[0, 1, 2], [3, 4, 5]])
    for v, f in ((torch.rand(6, 3), faces), (torch.rand(2, 6, 2), faces), (sv.double(), faces), (sv, faces.float()),
                 (sv, faces[None].repeat(2, 1, 1)), (sv, faces[:, :2]), (sv.numpy(), faces)):
        with pytest.raises(ValueError):
            nr.rasterize_fragments(v, f, 8)
    with pytest.raises(ValueError, match="image_size"):
        nr.rasterize_fragments(sv, faces, 0)
    with pytest.raises(NotImplementedError, match="detach them: an attribute image carries no geometry gradient"):
        nr.rasterize_fragments(sv.clone().requires_grad_(True), faces, 8)
    with pytest.raises(ValueError, match="GPU"):
        nr.rasterize_fragments(sv, faces, 8)
    with torch.no_grad():                                           # grad disabled: not a gradient request
        with pytest.raises(ValueError, match="GPU"):
            nr.rasterize_fragments(sv.clone().requires_grad_(True), faces, 8)


def test_fragments_c_struct_points_at_the_record():
    from deep3dmap_amd import _lib
    fr = _host_fragments(anti_aliasing=True, fill_back=False)
    c = fr.c_struct()
    assert isinstance(c, _lib.D3MFragments)
    assert (c.face_index_map, c.weight_map, c.depth_map, c.faces, c.tri, c.visibility) == tuple(
        t.data_ptr() for t in (fr.face_index_map, fr.weight_map, fr.depth_map, fr.faces, fr.tri, fr.visibility))
    assert (c.visibility_size, c.batch_size, c.num_tri, c.fill_back, c.image_size, c.anti_aliasing) == (64, 2, 2, 0, 4, 1)
    assert fr.raster_size == 8


# ---- 6. the adjacency is the cached one -----------------------------------------------------------------------------------
def test_adjacency_is_built_once_and_shared_with_the_vertex_colour_node(monkeypatch):
    """interpolate_vertex_attributes asks row_gather.vertex_adjacency for (tri, V, cache): the object
    textures_from_vertex_colors and the deterministic mode use, built on the first call and reused afterwards."""
    from deep3dmap_amd.neural_renderer import attributes as at, row_gather
    fr = _host_fragments()
    cache = row_gather.AdjacencyCache()
    built = []
    real = row_gather.build_adjacency
    monkeypatch.setattr(row_gather, "build_adjacency", lambda faces, V: built.append(real(faces, V)) or built[-1])
    for _ in range(2):                                               # (on the host the call ends at the device check, behind it)
        with pytest.raises(ValueError, match="GPU"):
            at.interpolate_vertex_attributes(torch.rand(6, 3), fr, None, cache)
    assert len(cache) == 1 and len(built) == 1
    assert row_gather.vertex_adjacency(fr.tri, 6, cache) is built[0] and len(built) == 1
    assert built[0].csr.items.tolist() == [0, 1, 2, 3, 4, 5] and built[0].num_vertices == 6
    # an index outside [0, V): refused where the adjacency is built
    with pytest.raises(ValueError, match="indices"):
        at.interpolate_vertex_attributes(torch.rand(5, 3), fr._replace(num_vertices=5), None, cache)


# ---- 7. the C entry points refuse bad arguments before any launch ---------------------------------------------------------
def test_entry_points_return_invalid_before_any_launch():
    import ctypes
    from deep3dmap_amd import _lib
    L = _lib.lib()
    p, q = ctypes.c_void_p(256), 256                                 # never dereferenced
    INVALID = 1
    fr_ok = dict(face_index_map=q, weight_map=q, depth_map=q, faces=q, tri=q, visibility=q, visibility_size=1 << 20,
                 batch_size=2, num_tri=2, fill_back=1, image_size=4, anti_aliasing=0)
    fwd_ok = dict(fr=True, attributes=p, attributes_batch=1, V=6, C=3, background=None, images=p, alpha=p)
    bad_fr = [dict(face_index_map=None), dict(weight_map=None), dict(depth_map=None), dict(faces=None), dict(tri=None),
              dict(batch_size=0), dict(batch_size=65536), dict(num_tri=0), dict(image_size=0), dict(image_size=16385),
              dict(batch_size=40000, num_tri=40000)]
    bad_fwd = [dict(fr=None), dict(attributes=None), dict(images=None), dict(alpha=None), dict(attributes_batch=3),
               dict(attributes_batch=0), dict(V=0), dict(C=0), dict(C=1025)]
    for change in bad_fr + bad_fwd:
        a = dict(fwd_ok, **{k: v for k, v in change.items() if k in fwd_ok})
        if a["fr"]:
            a["fr"] = ctypes.byref(_lib.D3MFragments(**dict(fr_ok, **{k: v for k, v in change.items() if k in fr_ok})))
        assert L.d3m_vertex_attribute_images(*a.values(), None) == INVALID, change
    csr_ok = dict(offsets=q, items=q, chunks=None, long_rows=None, long_chunk_ptr=None, num_rows=6, num_chunks=0,
                  num_long_rows=0, long_row=64)
    bwd_ok = dict(fr=True, grad_images=p, csr=True, scratch=p, scratch_floats=1 << 30, grad=p, attributes_batch=1, V=6, C=3)
    bad_bwd = [dict(fr=None), dict(grad_images=None), dict(csr=None), dict(scratch=None), dict(grad=None),
               dict(attributes_batch=3), dict(V=0), dict(C=0), dict(C=1025), dict(visibility=None), dict(visibility_size=16),
               dict(offsets=None), dict(items=None), dict(num_rows=5), dict(num_chunks=1, chunks=q),
               dict(num_long_rows=1, long_rows=q, long_chunk_ptr=q)]
    for change in bad_fr + bad_bwd:
        a = dict(bwd_ok, **{k: v for k, v in change.items() if k in bwd_ok})
        if a["fr"]:
            a["fr"] = ctypes.byref(_lib.D3MFragments(**dict(fr_ok, **{k: v for k, v in change.items() if k in fr_ok})))
        if a["csr"]:
            a["csr"] = ctypes.byref(_lib.D3MCsr(**dict(csr_ok, **{k: v for k, v in change.items() if k in csr_ok})))
        assert L.d3m_vertex_attribute_images_backward(*a.values(), None) == INVALID, change
    # too little scratch: its own code; and the size itself
    csr = _lib.D3MCsr(**csr_ok)
    assert L.d3m_vertex_attribute_scratch_floats(2, 4, 3, ctypes.byref(csr)) == 2 * 4 * 3 * 3
    assert L.d3m_vertex_attribute_scratch_floats(2, 4, 0, ctypes.byref(csr)) == 0
    a = dict(bwd_ok, scratch_floats=2 * 4 * 3 * 3 - 1)
    a["fr"], a["csr"] = ctypes.byref(_lib.D3MFragments(**fr_ok)), ctypes.byref(csr)
    assert L.d3m_error_string(L.d3m_vertex_attribute_images_backward(*a.values(), None)) == b"workspace missing or too small"
