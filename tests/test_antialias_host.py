"""The analytic edge antialiasing without a device (neural_renderer/antialias.py, csrc/d3m_antialias.h): the float64
restatement of tests/antialias_scenes.py against central differences of itself, the fragile-pair rule's cap and the float32
yardstick on the oracle's maps (measured here, recorded there), the side table on a hand-written mesh, the argument checks
and the C entry points' refusals, and the new kernels' register budget."""
import ctypes
import re

import pytest
import torch

import antialias_scenes as AS
import fragment_geometry_scenes as FG

FD_STEP = 1e-6
FD_AGREEMENT = 1e-6       # of the largest gradient entry: t is a ratio of expressions bilinear in the corners


# ---- 1. the restatement itself --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S1", "S2"])
def test_restatement_gradient_against_central_differences(name):
    S = 16
    maps, tri, sv = AS.oracle_case(name, S)
    B = sv.shape[0]
    images, g = AS.seeded_images(B, 3, S), AS.seeded_grad_out(B, 3, S)
    side = AS.side_opposite_of(tri)
    out, keep, gi, gs = AS.reference(maps, tri, sv, images, g, side=side)
    gk = g.double() * keep

    def loss(s):
        return float((AS.antialias_of(maps, tri, s, images, side=side)[0] * gk).sum())
    base = sv.double()
    fd = torch.zeros_like(base)
    for i in range(base.numel()):
        lo, hi = base.clone(), base.clone()
        lo.view(-1)[i] -= FD_STEP
        hi.view(-1)[i] += FD_STEP
        fd.view(-1)[i] = (loss(hi) - loss(lo)) / (2 * FD_STEP)
    err = float((gs - fd).abs().max()) / float(gs.abs().max())
    print(name, "largest |autograd - central differences| / largest entry:", err)
    assert float(gs.abs().max()) > 0 and err <= FD_AGREEMENT
    assert bool((gs[..., 2] == 0).all())                              # nothing depends on z
    # the image gradient is the transpose of a linear map: <g, A x> = <A^T g, x>
    x = torch.randn(images.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    Ax = AS.antialias_of(maps, tri, base, x, side=side)[0]
    assert abs(float((Ax * gk).sum()) - float((gi * x).sum())) <= 1e-12 * float((Ax * gk).abs().sum())
    assert float((out - images.double()).abs().max()) > 0.05          # the scene has silhouette pairs that blend


# ---- 2. the cap and the yardstick -------------------------------------------------------------------------------------------------
def test_left_out_shares_and_float32_yardstick_are_the_recorded_ones():
    """Measured here again on the oracle's maps (C = 3): every case within the cap and at its recorded share; the float32
    yardstick within a factor 2 of the recorded figures either way (torch's float32 kernels may associate differently from
    build to build); the device tolerances are 8 x the largest recorded ones."""
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        for name, S in AS.CASES:
            k = AS.key(name, S)
            maps, tri, sv = AS.oracle_case(name, S)
            B = sv.shape[0]
            images, g = AS.seeded_images(B, 3, S), AS.seeded_grad_out(B, 3, S)
            side = AS.side_opposite_of(tri)
            out, keep, gi, gs = AS.reference(maps, tri, sv, images, g, side=side)
            o32, _, gi32, gs32 = AS.reference(maps, tri, sv, images, g, torch.float32, side=side, keep=keep)
            share = AS.left_out_share(keep)
            forward = float(((o32.double() - out).abs() * keep).max())
            gradient = max(max(FG.view_errors(gi32, gi)), max(FG.view_errors(gs32, gs)))
            print(k, "left out: %.4f" % share, "float32 yardstick forward: %.2e gradient: %.2e" % (forward, gradient),
                  "recorded:", AS.LEFT_OUT[k], AS.YARDSTICK["forward"][k], AS.YARDSTICK["gradient"][k])
            assert share <= AS.MAX_LEFT_OUT and abs(share - AS.LEFT_OUT[k]) < 1e-4, (k, share)
            assert AS.YARDSTICK["forward"][k] / 2 <= forward <= AS.YARDSTICK["forward"][k] * 2, (k, forward)
            assert AS.YARDSTICK["gradient"][k] / 2 <= gradient <= AS.YARDSTICK["gradient"][k] * 2, (k, gradient)
            assert float(gs.abs().max()) > 0 and float((out - images.double()).abs().max()) > 0
    finally:
        torch.use_deterministic_algorithms(was)
    keys = {AS.key(n, S) for n, S in AS.CASES}
    assert keys == set(AS.LEFT_OUT) == set(AS.YARDSTICK["forward"]) == set(AS.YARDSTICK["gradient"])
    assert AS.FORWARD_TOLERANCE == 8 * max(AS.YARDSTICK["forward"].values())
    assert AS.GRADIENT_TOLERANCE == 8 * max(AS.YARDSTICK["gradient"].values())


# ---- 3. the side table --------------------------------------------------------------------------------------------------------
HAND_MESH = [[0, 1, 2],      # side 0: a boundary; side 1: manifold with the next; side 2: manifold with the last
             [2, 1, 3],      # side 1 (1-3): the fin
             [1, 4, 3], [3, 1, 5],                                     # the fin's other two triangles (one of them reversed)
             [6, 6, 7],      # a triangle that repeats an index
             [6, 7, 8],      # its neighbour: the shared edge counts for this one alone
             [0, 2, 9]]
HAND_TABLE = [[-1, 3, 9], [0, -2, -1], [-1, -1, -2], [-2, -1, -1], [-2, -2, -2], [-1, -1, -1], [1, -1, -1]]


def test_side_opposite_on_a_hand_written_mesh():
    from deep3dmap_amd.neural_renderer.antialias import SIDE_BOUNDARY, SIDE_IGNORED, build_side_opposite
    assert (SIDE_BOUNDARY, SIDE_IGNORED) == (-1, -2)
    for dtype in (torch.int32, torch.int64):
        faces = torch.tensor(HAND_MESH, dtype=dtype)
        for f in (faces, faces[None]):
            table = build_side_opposite(f, 10)
            assert table.dtype == torch.int32 and table.is_contiguous() and table.tolist() == HAND_TABLE
    assert AS.side_opposite_of(HAND_MESH).tolist() == HAND_TABLE
    # and on every scene of the device tests the operator form agrees with the dictionary form
    for name in ("S1", "S2", "S3B", "S4"):
        tri = torch.as_tensor(AS.scene(name)["tri"])
        assert torch.equal(build_side_opposite(tri, int(tri.max()) + 1).long(), AS.side_opposite_of(tri)), name


def test_side_table_cache_is_a_built_cache_of_its_own():
    import importlib
    from deep3dmap_amd.neural_renderer import built_cache, row_gather
    antialias = importlib.import_module("deep3dmap_amd.neural_renderer.antialias")     # (the package's attribute is the function)
    assert issubclass(antialias.SideOppositeCache, built_cache.BuiltCache)
    assert not issubclass(antialias.SideOppositeCache, row_gather.AdjacencyCache)
    cache = antialias.SideOppositeCache(size=2)
    faces = torch.tensor(HAND_MESH)
    first = antialias.side_opposite(faces, 10, cache)
    assert antialias.side_opposite(faces, 10, cache) is first and len(cache) == 1
    faces[0, 0] = 0                                                   # a new version of the tensor: built again
    assert antialias.side_opposite(faces, 10, cache) is not first and len(cache) == 2


def test_side_table_is_not_built_under_a_capture(monkeypatch):
    """As the other caches: a hit is handed out (and registered with the captured step), a miss raises."""
    import importlib
    from deep3dmap_amd.neural_renderer import rasterize_ops
    antialias = importlib.import_module("deep3dmap_amd.neural_renderer.antialias")
    rasterize_ops.take_captured_refs()
    cache = antialias.SideOppositeCache()
    faces = torch.tensor(HAND_MESH)
    built = antialias.side_opposite(faces, 10, cache)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    assert antialias.side_opposite(faces, 10, cache) is built
    with pytest.raises(RuntimeError, match="side table"):
        antialias.side_opposite(faces.clone(), 10, cache)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    assert any(ref is built for ref in rasterize_ops.take_captured_refs())


# ---- 4. argument checks ---------------------------------------------------------------------------------------------------------
def _host_fragments(B=2, V=6, s=4, anti_aliasing=False):
    from deep3dmap_amd import neural_renderer as nr
    S = 2 * s if anti_aliasing else s
    return nr.Fragments(torch.full((B, S, S), -1, dtype=torch.int32), torch.zeros(B, S, S, 3), torch.zeros(B, S, S),
                        torch.zeros(B, 4, 3, 3), torch.zeros(64, dtype=torch.uint8),
                        torch.tensor([[0, 1, 2], [3, 4, 5]], dtype=torch.int32), True, s, anti_aliasing, V)


def test_argument_errors():
    from deep3dmap_amd import neural_renderer as nr
    from deep3dmap_amd.neural_renderer.antialias import antialias
    assert nr.antialias is antialias
    fr, sv, images = _host_fragments(), torch.rand(2, 6, 3, requires_grad=True), torch.rand(2, 3, 4, 4)
    with pytest.raises(ValueError, match="anti_aliasing"):
        nr.antialias(torch.rand(2, 3, 4, 4), _host_fragments(anti_aliasing=True), sv)
    with pytest.raises(ValueError, match="Fragments"):
        nr.antialias(images, tuple(fr), sv)
    with pytest.raises(ValueError, match="fit"):
        nr.antialias(images, fr._replace(depth_map=torch.zeros(2, 4, 5)), sv)
    ok = torch.rand(2, 3, 4, 4)
    for bad in (torch.rand(3, 4, 4), torch.rand(2, 3, 4, 4, 1), ok.double(), ok.half(), ok.numpy(), torch.rand(2, 0, 4, 4),
                torch.rand(2, 1025, 4, 4), torch.rand(1, 3, 4, 4), torch.rand(3, 3, 4, 4), torch.rand(2, 3, 4, 5),
                torch.rand(2, 3, 8, 8), ok.to("meta")):
        with pytest.raises(ValueError, match="images"):
            nr.antialias(bad, fr, sv)
    for bad in (torch.rand(6, 3), torch.rand(2, 6, 2), sv.detach().double(), torch.rand(2, 5, 3), torch.rand(2, 7, 3),
                torch.rand(3, 6, 3), torch.rand(2, 6, 3).to("meta")):
        with pytest.raises(ValueError, match="screen_vertices"):
            nr.antialias(images, fr, bad)
    # well-formed arguments on the host end at the device check, behind every other check
    for v in (sv, sv.detach()):
        with pytest.raises(ValueError, match="GPU"):
            nr.antialias(images, fr, v)
    with pytest.raises(ValueError, match="indices"):                 # an index of tri outside [0, V)
        nr.antialias(images, fr._replace(num_vertices=5), torch.rand(2, 5, 3))


def test_renderer_options():
    """antialias=True on a renderer with anti_aliasing is refused before anything else; on one without it the call detaches
    for the record and gets as far as the device check; the defaults still refuse vertices that require grad."""
    from deep3dmap_amd import neural_renderer as nr
    r = object.__new__(nr.Renderer)                                  # (the constructor puts its camera on the device)
    r.camera_mode, r.image_size, r.anti_aliasing, r.fill_back, r.near, r.far = "none", 8, True, True, 0.1, 100
    v = torch.rand(2, 6, 3, requires_grad=True)
    faces = torch.tensor([[[0, 1, 2], [3, 4, 5]]])
    attr, image, fuv = torch.rand(6, 3), torch.rand(8, 8, 3), torch.rand(2, 3, 2)
    for geometry_grad in (False, True):
        with pytest.raises(ValueError, match="anti_aliasing=False"):
            r.render_attributes(v, faces, attr, antialias=True, geometry_grad=geometry_grad)
        with pytest.raises(ValueError, match="anti_aliasing=False"):
            r.render_uv_texture(v, faces, image, fuv, antialias=True, geometry_grad=geometry_grad)
    r.anti_aliasing = False
    for geometry_grad in (False, True):
        with pytest.raises(ValueError, match="GPU"):
            r.render_attributes(v, faces, attr, antialias=True, geometry_grad=geometry_grad)
        with pytest.raises(ValueError, match="GPU"):
            r.render_uv_texture(v, faces, image, fuv, antialias=True, geometry_grad=geometry_grad)
    with pytest.raises(NotImplementedError, match="mipmap"):
        r.render_uv_texture(v, faces, image, fuv, mipmap=True, antialias=True, geometry_grad=True)
    with pytest.raises(NotImplementedError, match="detach them"):
        r.render_attributes(v, faces, attr, antialias=False)
    with pytest.raises(NotImplementedError, match="detach them"):
        r.render_uv_texture(v, faces, image, fuv)


# ---- 5. the C entry points refuse bad arguments before any launch -----------------------------------------------------------------
def test_entry_points_return_invalid_before_any_launch():
    from deep3dmap_amd import _lib
    L = _lib.lib()
    p, q, r2 = ctypes.c_void_p(256), 256, ctypes.c_void_p(512)       # never dereferenced
    INVALID = 1
    fr_ok = dict(face_index_map=q, weight_map=q, depth_map=q, faces=q, tri=q, visibility=q, visibility_size=1 << 20,
                 batch_size=2, num_tri=2, fill_back=1, image_size=4, anti_aliasing=0)
    csr_ok = dict(offsets=q, items=q, chunks=None, long_rows=None, long_chunk_ptr=None, num_rows=6, num_chunks=0,
                  num_long_rows=0, long_row=64)
    bad_fr = [dict(face_index_map=None), dict(weight_map=None), dict(depth_map=None), dict(faces=None), dict(tri=None),
              dict(batch_size=0), dict(batch_size=65536), dict(num_tri=0), dict(image_size=0), dict(image_size=16385),
              dict(batch_size=65535, image_size=16384), dict(anti_aliasing=1), dict(fr=None)]

    def run(fn, ok, changes):
        for change in changes:
            a = dict(ok, **{k: v for k, v in change.items() if k in ok})
            if a.get("fr"):
                a["fr"] = ctypes.byref(_lib.D3MFragments(**dict(fr_ok, **{k: v for k, v in change.items() if k in fr_ok})))
            if a.get("csr"):
                a["csr"] = ctypes.byref(_lib.D3MCsr(**dict(csr_ok, **{k: v for k, v in change.items() if k in csr_ok})))
            assert fn(*a.values(), None) == INVALID, (fn.__name__, change)

    misaligned = ctypes.c_void_p(258)
    run(L.d3m_antialias_images, dict(fr=True, images=p, C=3, sv=p, V=6, side=p, out=r2),
        bad_fr + [dict(images=None), dict(sv=None), dict(side=None), dict(out=None), dict(out=p), dict(images=misaligned),
                  dict(sv=misaligned), dict(side=misaligned), dict(out=misaligned), dict(C=0), dict(C=1025), dict(V=0)])
    r3, r4 = ctypes.c_void_p(768), ctypes.c_void_p(1024)
    run(L.d3m_antialias_images_backward, dict(fr=True, images=p, C=3, sv=p, V=6, side=p, g=r2, gi=r3, pg=r4),
        bad_fr + [dict(images=None), dict(sv=None), dict(side=None), dict(g=None), dict(gi=None, pg=None), dict(gi=p),
                  dict(gi=r2), dict(g=misaligned), dict(gi=misaligned), dict(pg=misaligned), dict(C=0), dict(C=1025), dict(V=0)])
    bwd_ok = dict(fr=True, pg=p, csr=True, scratch=p, scratch_floats=1 << 30, grad=p, V=6)
    run(L.d3m_antialias_geometry_backward, bwd_ok,
        bad_fr + [dict(pg=None), dict(csr=None), dict(scratch=None), dict(grad=None), dict(pg=misaligned), dict(V=0),
                  dict(visibility=None), dict(visibility_size=16), dict(offsets=None), dict(items=None), dict(num_rows=5),
                  dict(num_chunks=1, chunks=q), dict(num_long_rows=1, long_rows=q, long_chunk_ptr=q)])
    # the scratch: B F' 9 sums, 3 B num_chunks chunk sums, and 4 B S S with the pair_grads map; too little has its own code
    csr = _lib.D3MCsr(**csr_ok)
    assert L.d3m_antialias_scratch_floats(2, 4, 4, ctypes.byref(csr), 0) == 2 * 4 * 9
    assert L.d3m_antialias_scratch_floats(2, 4, 4, ctypes.byref(csr), 1) == 2 * 4 * 9 + 2 * 4 * 4 * 4
    assert L.d3m_antialias_scratch_floats(2, 4, 0, ctypes.byref(csr), 1) == 0
    assert L.d3m_antialias_scratch_floats(0, 4, 4, ctypes.byref(csr), 0) == 0
    a = dict(bwd_ok, scratch_floats=2 * 4 * 9 - 1)
    a["fr"], a["csr"] = ctypes.byref(_lib.D3MFragments(**fr_ok)), ctypes.byref(csr)
    assert L.d3m_error_string(L.d3m_antialias_geometry_backward(*a.values(), None)) == b"workspace missing or too small"


# ---- 6. the kernels' budget ---------------------------------------------------------------------------------------------------------
def test_kernels_use_no_scratch():
    from deep3dmap_amd.resource_usage import kernel_resource_usage
    short = {re.sub(r"^(void )?(d3m::)?", "", re.sub(r"\(.*$", "", k)): v for k, v in kernel_resource_usage().items()}
    for name in ("k_antialias_images", "k_antialias_images_backward", "k_antialias_face_sums", "k_antialias_large_face_sums"):
        assert name in short, name
        assert short[name]["scratch"] == 0 and not short[name]["vgpr_spill"] and not short[name]["sgpr_spill"], (name, short[name])
