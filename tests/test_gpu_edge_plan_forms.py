"""The edge gradient's plan in its two forms (d3m_edge_grad.h, struct EdgePlan): the one-pass form (fixed record slice per
line) and the counted form (count -> allocate -> scatter).  Both must give the same gradients where every crossing has a
record; a one-pass plan whose lines outgrow their slices (or whose crossings outgrow the blob) walks what has no record
through k_edge_overflow and still matches the reference's kernels; the deterministic mode stays bit-identical."""
import numpy as np
import pytest
import torch

from conftest import kernels_launched
from oracle import nr_ref_hip as RH

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not RH.available(), reason="oracle/_ref/libnr_ref_hip.so not built (make -C oracle ref_hip)")]

GRAD_RTOL = 1e-3        # as tests/test_gpu_reference.py: backward gradients to 1e-3 of the tensor's largest entry
EPS = 1e-3
COUNT_KERNELS = {"k_edge_count", "k_alloc_plan"}


def _scene(B, S, n, seed=0, distance=2.732):
    """the headline's mesh family (tools_dev/plan_stats.py) at B views of S^2; n x n vertices: 2 (n-1)^2 faces per view;
    a camera farther away than the headline's crowds the crossings onto fewer lines"""
    from deep3dmap_amd import neural_renderer as nr, synthetic
    from deep3dmap_amd.neural_renderer.mesh_ops import gather_faces
    v, tri = synthetic.grid_mesh(n, seed=seed)
    eyes = torch.from_numpy(synthetic.camera_ring(32, distance=distance)[:B]).cuda()
    vt = torch.from_numpy(v).cuda()[None].expand(B, -1, -1).contiguous()
    ft = torch.from_numpy(tri).cuda()[None].expand(B, -1, -1).contiguous()
    faces = gather_faces(nr.look_at(vt, eyes, _perspective_angle=30), ft, True).contiguous()
    gen = torch.Generator(device="cuda").manual_seed(1234 + seed)
    tex = torch.rand(B, faces.shape[1], 2, 2, 2, 3, device="cuda", generator=gen)
    ref = RH.forward(faces, tex, S, 0.1, 100.0, EPS, (0.1, 0.2, 0.3))
    g_rgb = torch.randn(B, S, S, 3, device="cuda", generator=gen)
    g_alpha = torch.randn(B, S, S, device="cuda", generator=gen)
    return faces, ref, g_rgb, g_alpha


def _plan_bytes(B, F, S, cap):
    """a plan blob that holds exactly `cap` crossings (edge_plan_view's arithmetic)"""
    from deep3dmap_amd import _lib
    fixed = int(_lib.lib().d3m_edge_plan_min_bytes(B, F, S)) - 1024
    return fixed + 512 + (cap + 32) * 36


def _flags(plan, B, S):
    """(records per line, EG_ALLOC_SPILL, EG_ALLOC_FULL, EG_ALLOC_TOTAL) of a built plan"""
    nl = B * 2 * S
    raw = plan.cpu().numpy()
    off_alloc = (nl * 4 + 255) // 256 * 256
    alloc = raw[off_alloc:off_alloc + 256].view(np.int32)
    return raw[:nl * 4].view(np.int32).copy(), int(alloc[3]), int(alloc[4]), int(alloc[0])


def _spill_cap(faces, ref, g_rgb, g_alpha, B, S, margin=1.3):
    """a crossing capacity with room for every crossing's index (`margin` x the batch's crossings, counted by the counted
    form), and the records per line"""
    _, plan, _ = _edge_grad(faces, ref, g_rgb, g_alpha, S, form=1)
    counts, _, _, total = _flags(plan, B, S)
    return int(margin * total) + 16 * 1024, counts


def _edge_grad(faces, ref, g_rgb, g_alpha, S, plan_bytes=None, form=None):
    """K4 alone through the product's operator, with a plan built by d3m_edge_plan in a blob of `plan_bytes`
    (None: the default size); `form`: d3m_set_edge_plan_form for the build and the use of the plan."""
    from deep3dmap_amd import _lib
    from deep3dmap_amd.neural_renderer import rasterize_ops as ops
    B, F = faces.shape[:2]
    L = _lib.lib()
    old = L.d3m_get_edge_plan_form()
    if form is not None:
        _lib.check(L.d3m_set_edge_plan_form(form), "d3m_set_edge_plan_form")
    try:
        vis = ops.visibility(ref["face_index_map"], F)
        n = plan_bytes if plan_bytes is not None else int(_lib.lib().d3m_edge_plan_bytes(B, F, S))
        plan = torch.empty(n, dtype=torch.uint8, device="cuda")
        gf = torch.zeros_like(faces)
        with kernels_launched() as k:
            ops.edge_plan(faces, ref["face_index_map"], vis, S, out=plan)
            ops.backward_pixel_map(faces, ref["face_index_map"], ref["rgb_map"], ref["alpha_map"], g_rgb, g_alpha, gf, S,
                                   EPS, True, True, visibility=vis, edge_plan=plan)
        torch.cuda.synchronize()
    finally:
        L.d3m_set_edge_plan_form(old)
    return gf, plan, set(k.names)


def _assert_matches_reference(gf, faces, ref, g_rgb, g_alpha):
    gf_ref, _ = RH.backward(ref, g_rgb, g_alpha, None, True, True, False)
    ok = torch.isfinite(gf_ref)
    assert torch.equal(ok, torch.isfinite(gf))
    scale = float(gf_ref[ok].abs().max())
    assert scale > 0
    assert float((gf[ok] - gf_ref[ok]).abs().max()) <= GRAD_RTOL * scale


@pytest.fixture(scope="module")
def scene():
    B, S = 2, 128            # 2 x 44.5 k faces: 2120 blocks of faces, the one-pass form's range
    faces, ref, g_rgb, g_alpha = _scene(B, S, 150)
    return B, S, faces, ref, g_rgb, g_alpha


@pytest.fixture(scope="module")
def far_scene():
    B, S = 2, 128
    faces, ref, g_rgb, g_alpha = _scene(B, S, 150, seed=1, distance=6.0)
    return B, S, faces, ref, g_rgb, g_alpha


def test_forms_bit_equal_without_spill(scene):
    B, S, faces, ref, g_rgb, g_alpha = scene
    gf1, plan1, k1 = _edge_grad(faces, ref, g_rgb, g_alpha, S)
    gf2, plan2, k2 = _edge_grad(faces, ref, g_rgb, g_alpha, S, form=1)
    assert not (COUNT_KERNELS & k1) and "k_edge_scatter" in k1, sorted(k1)          # the default blob: one pass
    assert COUNT_KERNELS <= k2, sorted(k2)
    counts, spill, full, _ = _flags(plan1, B, S)
    assert spill == 0 and full == 0 and counts.max() > 0
    counts2, _, _, _ = _flags(plan2, B, S)
    assert np.array_equal(counts, counts2)          # the same records per line, in any order
    assert torch.equal(gf1, gf2)
    _assert_matches_reference(gf1, faces, ref, g_rgb, g_alpha)


def test_one_pass_lines_spill_to_overflow(far_scene):
    """slices of 1.3x the mean crossings per line: the fuller lines spill, the rest keep their records"""
    B, S, faces, ref, g_rgb, g_alpha = far_scene
    F = faces.shape[1]
    cap, counts = _spill_cap(faces, ref, g_rgb, g_alpha, B, S)
    cap_line = cap // (B * 2 * S)
    assert int((counts > cap_line).sum()) > 0, (counts.max(), cap_line)
    gf, plan_s, names = _edge_grad(faces, ref, g_rgb, g_alpha, S, plan_bytes=_plan_bytes(B, F, S, cap), form=2)
    assert not (COUNT_KERNELS & names)
    counts_s, spill, full, _ = _flags(plan_s, B, S)
    assert np.array_equal(counts_s, counts)
    assert full == 0 and spill == 1 and 0 < int((counts_s > cap_line).sum()) < int((counts_s > 0).sum())
    _assert_matches_reference(gf, faces, ref, g_rgb, g_alpha)
    gf_full, _, _ = _edge_grad(faces, ref, g_rgb, g_alpha, S)
    ok = torch.isfinite(gf_full)
    assert float((gf[ok] - gf_full[ok]).abs().max()) <= GRAD_RTOL * float(gf_full[ok].abs().max())


def test_one_pass_blob_too_small_walks_everything(scene):
    """slices of a few records: the crossings' indices outgrow the blob, no record is used, every crossing is walked"""
    B, S, faces, ref, g_rgb, g_alpha = scene
    F = faces.shape[1]
    nl = B * 2 * S
    gf, plan, names = _edge_grad(faces, ref, g_rgb, g_alpha, S, plan_bytes=_plan_bytes(B, F, S, 4 * nl), form=2)
    assert not (COUNT_KERNELS & names)
    assert _flags(plan, B, S)[2] == 1
    _assert_matches_reference(gf, faces, ref, g_rgb, g_alpha)
    # the counted form in the same blob: all or nothing as well
    gf2, _, names2 = _edge_grad(faces, ref, g_rgb, g_alpha, S, plan_bytes=_plan_bytes(B, F, S, 4 * nl))
    assert COUNT_KERNELS <= names2
    assert torch.equal(gf, gf2)


def test_dense_mesh_small_image_lines_outgrow_slices():
    """a dense mesh at a small raster: slices smaller than the fullest lines.  Most of such a mesh's crossings are idle (no
    record), so the blob that makes the slices this small cannot index every crossing either: nothing is recorded and
    every crossing is walked (EG_ALLOC_FULL) -- or, with room for the indices, the fullest lines spill"""
    B, S = 2, 32
    faces, ref, g_rgb, g_alpha = _scene(B, S, 150, seed=3, distance=4.0)
    F = faces.shape[1]
    nl = B * 2 * S
    _, counts = _spill_cap(faces, ref, g_rgb, g_alpha, B, S)
    cap_line = max(int(counts.max()) - 8, 1)
    gf, plan_s, names = _edge_grad(faces, ref, g_rgb, g_alpha, S, plan_bytes=_plan_bytes(B, F, S, cap_line * nl), form=2)
    assert not (COUNT_KERNELS & names)
    _, spill, full, _ = _flags(plan_s, B, S)
    assert spill == 1 or full == 1
    _assert_matches_reference(gf, faces, ref, g_rgb, g_alpha)


@pytest.mark.parametrize("spilling", [False, True])
def test_deterministic_one_pass_bit_identical(far_scene, spilling):
    from deep3dmap_amd import _lib
    B, S, faces, ref, g_rgb, g_alpha = far_scene
    F = faces.shape[1]
    kw = {}
    if spilling:
        kw = dict(plan_bytes=_plan_bytes(B, F, S, _spill_cap(faces, ref, g_rgb, g_alpha, B, S)[0]), form=2)
    with _lib.deterministic():
        gf1, plan1, names = _edge_grad(faces, ref, g_rgb, g_alpha, S, **kw)
        gf2, _, _ = _edge_grad(faces, ref, g_rgb, g_alpha, S, **kw)
    assert not (COUNT_KERNELS & names)
    assert _flags(plan1, B, S)[1] == (1 if spilling else 0)
    assert torch.equal(gf1, gf2)
