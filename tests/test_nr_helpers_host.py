"""NrRenderer's helper kernels without a device: the restatement of tests/nr_helper_scenes.py is pinned against the oracle
(oracle/nr_oracle.py: square maps and shared K, all it can express), against torch.nn.functional.grid_sample in float64,
against central differences and against known answers; every case tagged `exact` is proven exact (the float32 evaluation, one
operation at a time, gives the float64 bits at every element, and every reduction is exact in any order); every float case's
tolerance is proven sharp against six wrong variants of the restatement; the launcher arithmetic is restated and the path of
every case asserted; and every D3M_ERR_INVALID branch of the eleven entry points is driven with pointers that are never
dereferenced.  test_gpu_nr_helpers.py takes its expectations from the reference functions below."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nr_helper_scenes as S

GRID_KEYS = ("depth", "inv_K", "A", "t")


# ---- what the GPU file expects of a case: (dict of float64 arrays, dict of tolerances or None for "these bits") -------------------
def _ar(c):
    return "f64" if c.kind in ("exact", "zoom", "zero") else "err"


def _split(x, exact):
    """an evaluated result -> (values, tolerance or None)"""
    if x is None:
        return None, None
    if exact:
        return np.asarray(x, np.float64), None
    x = S.Err.lift(x)
    return x.v, S.tolerance(x.e)


def grid_forward(c, threeD, ar=None, variant=None):
    ar = ar or _ar(c)
    inp = S.grid_inputs(c)
    a = S.in_arith(inp, ar, GRID_KEYS + ("K",))
    return S.grid_warp(a["depth"], a["inv_K"], a["A"], a["t"], inp["cz"], None if threeD else a["K"], c.crop, c.H, c.W, variant)


def grid_forward_reference(c, threeD):
    return _split(grid_forward(c, threeD), c.kind == "exact")


def grid_backward(c, threeD, ar=None, variant=None):
    """(g_depth, g_A [B,9], g_t [B,3]) in the arithmetic"""
    ar = ar or _ar(c)
    inp = S.grid_inputs(c)
    a = S.in_arith(inp, ar, GRID_KEYS + ("K", "g3", "g2"))
    gd, terms = S.grid_warp_backward(a["depth"], a["inv_K"], a["A"], a["t"], inp["cz"], None if threeD else a["K"],
                                     a["g3"] if threeD else a["g2"], c.H, c.W, None if variant == "skip_run" else variant)
    HW = c.H * c.W
    skip = slice(256 * ((HW // 256) // 2), min(HW, 256 * ((HW // 256) // 2) + 256)) if variant == "skip_run" else None
    sums = S.reduce_terms(terms, S.reduce_chain(HW, S.grid_warp_split(c.B, HW)), skip)
    return gd, sums[:, :9], sums[:, 9:], terms


def grid_backward_reference(c, threeD):
    gd, gA, gt, _ = grid_backward(c, threeD)
    exact = c.kind == "exact"
    return {k: _split(v, exact) for k, v in (("g_depth", gd), ("g_A", gA), ("g_t", gt))}


def normals_forward(c, ar="err"):
    inp = S.normal_inputs(c)
    a = S.in_arith(inp, ar, ("depth", "inv_K"))
    return S.depth_normals(a["depth"], a["inv_K"], c.H, c.W)


def normals_backward(c, ar="err", variant=None):
    inp = S.normal_inputs(c)
    a = S.in_arith(inp, ar, ("depth", "inv_K", "g"))
    return S.depth_normals_backward(a["depth"], a["inv_K"], a["g"], c.H, c.W, variant)


def normals_reference(c):
    return _split(normals_forward(c), False), _split(normals_backward(c), False)


BORDER_NORMAL_Z = np.float32(1.0) / (np.sqrt(np.float32(1.0)) + np.float32(1e-7))        # the bits of (0, 0, 1) / (1 + 1e-7)


def tex_reference(c):
    inp = S.tex_inputs(c)
    return S.textures_from_im(inp["im"], c.ts), S.textures_from_im_backward(inp["g"], c.B, c.C, c.H, c.W, c.ts)


def view_forward(c, ar=None):
    a = S.in_arith(S.view_inputs(c), ar or _ar(c), ("view",))
    return S.view_transform(a["view"])


def view_backward(c, with_rot=True, with_trans=True, ar=None):
    a = S.in_arith(S.view_inputs(c), ar or _ar(c), ("view", "g_rot", "g_trans"))
    return S.view_transform_backward(a["view"], a["g_rot"] if with_rot else None, a["g_trans"] if with_trans else None)


def view_reference(c, with_rot=True, with_trans=True):
    R, t = view_forward(c)
    exact = c.kind == "zero"
    return _split(R, exact), _split(t, exact), _split(view_backward(c, with_rot, with_trans), exact)


RES_KEYS = ("depth", "inv_K", "K", "A", "t", "src", "g")


def resample_forward(c, ar=None, variant=None):
    inp = S.resample_inputs(c)
    a = S.in_arith(inp, ar or _ar(c), RES_KEYS)
    return S.warp_resample(a["depth"], a["inv_K"], a["K"], a["A"], a["t"], inp["cz"], a["src"], inp["src_n"], c.h, c.w, c.H, c.W,
                           variant)


def resample_backward(c, ar=None, variant=None):
    """(g_src added to the pre-filled integers [B,C,HW] and its tolerance, g_depth, partials [B,parts,12]) in the arithmetic"""
    ar = ar or _ar(c)
    inp = S.resample_inputs(c)
    a = S.in_arith(inp, ar, RES_KEYS)
    contrib, gd, terms = S.warp_resample_backward(a["depth"], a["inv_K"], a["K"], a["A"], a["t"], inp["cz"], a["src"], a["g"],
                                                  c.h, c.w, c.H, c.W, variant)
    return contrib, gd, S.resample_partials(terms, S.resample_parts(c.h, c.w)), terms


@functools.lru_cache(maxsize=None)
def partials_exact(c):
    """the (A, t) partial sums of an exact case are compared bit for bit where one workgroup of at most 256 pixels forms them (the
    host file proves those sums exact in any order); the sums of a larger map's products of dyadic fractions do not stay within
    24 bits, and are compared with the bound of the float cases"""
    if c.kind != "exact" or c.h * c.w > 256:
        return False
    a, b = resample_backward(c, "f32"), resample_backward(c, "f64")
    return bool(S.same_bits(a[2], b[2]) and all(S.exact_sum_proven(t, 1) for t in b[3]))


def src_tolerance(contrib, mag):
    """of grad_src: the bound of every contribution w g, and the atomic adds: as many roundings as contributions meet in a texel"""
    offs, ok, vals = contrib
    e, count = np.zeros_like(mag), np.zeros_like(mag)
    rows = np.arange(mag.shape[0])[:, None]
    for ch in range(mag.shape[1]):
        for k in range(4):
            np.add.at(e[:, ch], (rows, offs[k]), np.where(ok[k], vals[ch][k].e, 0))
            np.add.at(count[:, ch], (rows, offs[k]), ok[k] * 1.0)
    return S.tolerance(e + (count + 1) * mag)


def resample_reference(c):
    """forward: (out, out_nearest); backward: g_src (with the pre-fill), g_depth, partials"""
    exact = c.kind in ("exact", "zoom")
    out, near, _ = resample_forward(c)
    contrib, gd, parts, _ = resample_backward(c)
    inp = S.resample_inputs(c)
    g_src, mag = S.scatter_src(contrib, c.B, c.C, c.H * c.W, inp["prefill"])
    src_tol = None if exact else src_tolerance(contrib, mag)
    if exact and not partials_exact(c):
        parts = resample_backward(c, "err")[2]
    return dict(out=_split(out, exact), near=near, g_src=(g_src, src_tol), g_depth=_split(gd, exact),
                partials=_split(parts, partials_exact(c)))


# ---- the restatement against known answers ---------------------------------------------------------------------------------------
IDENTITY = np.array([[1, 0, 0, 0, 1, 0, 0, 0, 1.]])


def test_identity_motion_and_identity_K_reproduce_the_pixel_grid():
    B, H, W = 2, 5, 9
    depth = np.ones((B, H * W))
    A, t = np.repeat(IDENTITY, B, 0), np.zeros((B, 3))
    pts = S.grid_warp(depth, IDENTITY, A, t, 1.0, None, None, H, W)
    ys, xs = np.mgrid[0:H, 0:W]
    assert np.array_equal(pts[0], np.stack([xs, ys, np.ones_like(xs)], -1).reshape(-1, 3))
    uv = S.grid_warp(depth, IDENTITY, A, t, 1.0, IDENTITY, None, H, W).reshape(B, H, W, 2)
    assert np.array_equal(uv[1, :, :, 0], xs / (W - 1) * 2.0 - 1.0) and np.array_equal(uv[1, :, :, 1], ys / (H - 1) * 2.0 - 1.0)
    # ... which grid_sample reads as the image itself when the source is sampled at its own pixel centres (align_corners = False
    # stretches it by W / (W-1): the centre pixel stays)
    ix, iy = S.pixel_position([uv[..., 0].reshape(B, -1), uv[..., 1].reshape(B, -1)], H, W)
    assert ix.reshape(B, H, W)[0, 2, 4] == 4.0 and iy.reshape(B, H, W)[0, 2, 4] == 2.0


def test_a_quarter_turn_about_each_axis():
    q = math.pi / 2
    eye = np.eye(3)
    # R = Rz (Ry Rx) with the reference's signs: Rx: y -> z, Ry: z -> x, Rz: x -> y
    for axis, image in ((0, [[1, 0, 0], [0, 0, 1], [0, -1, 0]]), (1, [[0, 0, -1], [0, 1, 0], [1, 0, 0]]), (2, [[0, 1, 0], [-1, 0, 0], [0, 0, 1]])):
        v = np.zeros((1, 6))
        v[0, axis] = q
        v[0, 3:] = (1, 2, 3)
        R, t = S.view_transform(v)
        assert np.allclose(R.reshape(3, 3) @ eye, np.array(image, float).T, rtol=0, atol=1e-15), axis
        assert t.tolist() == [[1, 2, 3]]
    # the order: Rx first.  y -Rx-> z -Ry-> x -Rz-> y
    R, _ = S.view_transform(np.array([[q, q, q]]))
    assert np.allclose(R.reshape(3, 3) @ np.array([0, 1, 0.]), [0, 1, 0], rtol=0, atol=1e-15)
    assert S.view_transform(np.zeros((2, 5)))[1].shape == (2, 3) and S.view_transform(np.array([[0, 0, 0, 4, 5.]]))[1].tolist() == [[4, 5, 0]]
    # the moved grid: a quarter turn about z of the point (1, 0, cz + 1) about c = (0, 0, cz)
    pts = S.grid_warp(np.full((1, 9), 2.0), np.array([[1, 0, -1, 0, 1, -1, 0, 0, 1.]]), S.view_transform(np.array([[0, 0, q]]))[0],
                      np.array([[0, 0, 0.5]]), 1.0, None, None, 3, 3)
    assert np.allclose(pts[0, 5], [-0.0, 2.0, 2.5], rtol=0, atol=1e-15)          # pixel (1, 2): ray (1, 0, 1), p = (2, 0, 2)


@pytest.mark.parametrize("crop", [(1, 0, 0, 0), (0, 2, 0, 0), (0, 0, 1, 0), (0, 0, 0, 3), (1, 2, 2, 1), (4, 0, 0, 6), (0, 4, 6, 0)])
def test_crop_is_crop_mesh_slicing(crop):
    B, H, W = 2, 5, 7
    c = S.GridCase(B, H, W, B, crop, "float")
    inp = S.grid_inputs(c)
    g = S.grid_warp(inp["depth"], inp["inv_K"], np.repeat(IDENTITY, B, 0), np.zeros((B, 3)), 0.0, None, None, H, W).reshape(B, H, W, 3).copy()
    top, bottom, left, right = crop
    # render_yaw's crop_mesh, statement for statement (renderer_nr.py:145-158 of the reference, as oracle/nr_oracle.py restates it)
    if top > 0:
        g[:, :top, :, 1] = np.repeat(g[:, top:top + 1, :, 1], top, 1)
        g[:, :top, :, 2] = np.repeat(g[:, top:top + 1, :, 2], top, 1)
    if bottom > 0:
        g[:, -bottom:, :, 1] = np.repeat(g[:, -bottom - 1:-bottom, :, 1], bottom, 1)
        g[:, -bottom:, :, 2] = np.repeat(g[:, -bottom - 1:-bottom, :, 2], bottom, 1)
    if left > 0:
        g[:, :, :left, 0] = np.repeat(g[:, :, left:left + 1, 0], left, 2)
        g[:, :, :left, 2] = np.repeat(g[:, :, left:left + 1, 2], left, 2)
    if right > 0:
        g[:, :, -right:, 0] = np.repeat(g[:, :, -right - 1:-right, 0], right, 2)
        g[:, :, -right:, 2] = np.repeat(g[:, :, -right - 1:-right, 2], right, 2)
    A = inp["A"]
    moved = np.einsum("bij,bnj->bni", A.reshape(B, 3, 3), g.reshape(B, -1, 3) - [0, 0, 1.0]) + [0, 0, 1.0] + inp["t"][:, None]
    got = S.grid_warp(inp["depth"], inp["inv_K"], A, inp["t"], 1.0, None, crop, H, W)
    assert np.allclose(got, moved, rtol=0, atol=1e-14)


def test_the_cube_coefficients():
    # utils.py:84-94 of the reference: the corners of the 2x2x2 cube in barycentric terms of the face's three colours
    assert S.CUBE.shape == (8, 3) and S.CUBE.tolist() == [[.5, .5, .5], [0, 0, 1], [0, 1, 0], [-.5, .5, .5], [1, 0, 0], [.5, -.5, .5],
                                                            [.5, .5, -.5], [0, 0, 0]]
    from deep3dmap_amd.core.renderer_utils import _CUBE
    assert _CUBE == S.CUBE.tolist()
    im = np.arange(12.0).reshape(1, 1, 3, 4)
    t2 = S.textures_from_im(im, 2)
    assert t2.shape == (1, 12, 8, 1)
    assert t2[0, 0, :, 0].tolist() == [2.5, 4, 1, 2.5, 0, 1.5, -1.5, 0]               # cell (0, 0), first face: colours (0, 1, 4)
    assert t2[0, 6 + 5, :, 0].tolist() == [(10 + 7 + 11) / 2, 11, 7, (-10 + 7 + 11) / 2, 10, (10 - 7 + 11) / 2, (10 + 7 - 11) / 2, 0]
    t1 = S.textures_from_im(im, 1)
    assert t1[0, :, 0, 0].tolist() == [0, 1, 2, 4, 5, 6, 5, 6, 7, 9, 10, 11]


ONE_ROW = dict(depth=np.full((1, 5), 2.0), inv_K=np.array([[1, 0, -2, 0, 1, 0, 0, 0, 1.]]), K=np.array([[2, 1, 1, -1, 4, 2, 0, 0, 1.]]),
               A=IDENTITY, t=np.array([[0.5, -1, 0.]]), cz=1.0)


def one_row_grid(ar="f64"):
    """a 1 x 5 map projected: gw_project divides by H - 1 = 0, as the reference's grid_3d_to_2d does (renderer_nr.py:82-88)"""
    a = S.in_arith(ONE_ROW, ar, GRID_KEYS + ("K",))
    with np.errstate(divide="ignore", invalid="ignore"):
        return S.grid_warp(a["depth"], a["inv_K"], a["A"], a["t"], 1.0, a["K"], None, 1, 5)


def test_a_map_of_one_row_projects_to_infinities_as_the_reference_does():
    uv = one_row_grid()
    assert np.isfinite(uv[..., 0]).all() and np.isinf(uv[..., 1]).all() and len(set(np.sign(uv[0, :, 1]))) == 2
    assert S.same_bits(one_row_grid("f32")[..., 0], uv[..., 0]) and np.array_equal(one_row_grid("f32")[..., 1], uv[..., 1])
    from oracle import nr_oracle as ora
    r = ora.NrRenderer({}, 5)
    r.K = torch.from_numpy(ONE_ROW["K"]).float().reshape(1, 3, 3)
    pts = S.grid_warp(ONE_ROW["depth"], ONE_ROW["inv_K"], ONE_ROW["A"], ONE_ROW["t"], 1.0, None, None, 1, 5)
    want = r.grid_3d_to_2d(torch.from_numpy(pts).float().reshape(1, 1, 5, 3)).numpy().reshape(1, 5, 2)
    assert np.array_equal(want[..., 1], uv[..., 1]) and np.allclose(want[..., 0], uv[..., 0], rtol=0, atol=1e-6)


# ---- against the oracle (square maps, one shared K) --------------------------------------------------------------------------------
def _oracle(size, view):
    from oracle import nr_oracle as ora
    r = ora.NrRenderer({}, size)
    r.set_transform_matrices(torch.from_numpy(view).float())
    return r


def test_restatement_against_the_oracle():
    from oracle import nr_oracle as ora
    B, s = 2, 9
    view = S.hashed_floats(B, 6, 61, -0.5, 0.5)
    view[:, 3:] *= 0.2
    r = _oracle(s, view)
    depth = torch.from_numpy(S.hashed_floats(B, s * s, 62, 0.9, 1.1)).reshape(B, s, s)
    iK, K = r.inv_K.double().numpy().reshape(1, 9), r.K.double().numpy().reshape(1, 9)
    R, t = S.view_transform(view.astype(np.float64))
    assert np.allclose(R.reshape(B, 3, 3), r.rot_mat.numpy(), rtol=0, atol=1e-6) and np.allclose(t, r.trans_xyz.numpy()[:, 0], rtol=0, atol=0)
    d = depth.double().numpy().reshape(B, -1)
    cz = r.rot_center_depth
    was, ora.EXACT = ora.EXACT, False
    try:
        want3, want2 = r.get_warped_3d_grid(depth).numpy(), r.get_warped_2d_grid(depth).numpy()
        inv2 = r.get_inv_warped_2d_grid(depth).numpy()
    finally:
        ora.EXACT = was
    assert np.allclose(S.grid_warp(d, iK, R, t, cz, None, None, s, s), want3.reshape(B, -1, 3), rtol=0, atol=2e-6)
    assert np.allclose(S.grid_warp(d, iK, R, t, cz, K, None, s, s), want2.reshape(B, -1, 2), rtol=0, atol=2e-5)
    # the inverse motion composed as Rigid.inverse() does: A' = R^T, t' = -(t R)
    Rm = R.reshape(B, 3, 3)
    Ai, ti = Rm.transpose(0, 2, 1).reshape(B, 9), -np.einsum("bk,bki->bi", t, Rm)
    assert np.allclose(S.grid_warp(d, iK, Ai, ti, cz, K, None, s, s), inv2.reshape(B, -1, 2), rtol=0, atol=2e-5)
    assert np.allclose(S.depth_normals(d, iK, s, s), r.get_normal_from_depth(depth).numpy(), rtol=0, atol=2e-4)
    im = torch.from_numpy(S.hashed_floats(B * 3, s * s, 63)).reshape(B, 3, s, s)
    for ts in (1, 2):
        want = ora.get_textures_from_im(im, ts).numpy().reshape(B, 2 * (s - 1) ** 2, ts ** 3, 3)
        assert np.allclose(S.textures_from_im(im.double().numpy(), ts), want, rtol=0, atol=1e-6)
    # the resampled frame: F.grid_sample of the oracle's own grid
    want = F.grid_sample(im, torch.from_numpy(inv2), mode="bilinear", align_corners=False).numpy()
    got, _, _ = S.warp_resample(d, iK, K, Ai, ti, cz, im.double().numpy().reshape(B, 3, -1), None, s, s, s, s)
    assert np.allclose(got, want.reshape(B, 3, -1), rtol=0, atol=3e-4)


# ---- against torch.nn.functional.grid_sample, float64 -------------------------------------------------------------------------------
def _positions(H, W):
    """normalised positions whose pixel coordinates cover (-1, 0), below -1, at and above W and H, halves and interior"""
    px = np.array([-2.5, -1.25, -1.0, -0.75, -0.5, -0.25, 0.0, 0.5, 1.5, W - 1.5, W - 1.0, W - 0.5, W - 0.25, float(W), W + 0.75, 2.25])
    py = np.array([-1.5, -0.6, 0.0, 0.5, 1.5, H - 1.0, H - 0.5, float(H), H + 1.5, 2.4])
    gx, gy = np.meshgrid((2 * px + 1) / W - 1, (2 * py + 1) / H - 1)
    return gx.reshape(1, -1), gy.reshape(1, -1)


@pytest.mark.parametrize("H,W", [(3, 3), (5, 9), (4, 6)])
def test_lookups_against_grid_sample(H, W):
    C = 2
    src = S.hashed_floats(C, H * W, 71).astype(np.float64).reshape(1, C, H * W)
    gx, gy = _positions(H, W)
    ix, iy = S.pixel_position([gx, gy], H, W)
    assert (ix < -1).any() and ((ix > -1) & (ix < 0)).any() and (ix >= W).any() and (iy >= H).any() and (iy < -1).any()
    grid = torch.from_numpy(np.stack([gx, gy], -1)).reshape(1, 1, -1, 2).requires_grad_(True)
    s = torch.from_numpy(src).reshape(1, C, H, W).requires_grad_(True)
    want = F.grid_sample(s, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    assert np.allclose(S.lookup_bilinear(src, ix, iy, H, W), want.detach().numpy().reshape(1, C, -1), rtol=0, atol=1e-14)
    # nearest: half to even, as torch's nearbyint; positions whose float64 pixel coordinate is exactly k + 1/2 are in the list
    assert (np.abs(ix - np.floor(ix) - 0.5) == 0).any()
    want_n = F.grid_sample(s.detach(), grid.detach(), mode="nearest", padding_mode="zeros", align_corners=False)
    assert np.array_equal(S.lookup_nearest(src, ix, iy, H, W), want_n.numpy().reshape(1, C, -1))
    assert not np.array_equal(S.lookup_nearest(src, ix, iy, H, W, rounding=lambda v: np.floor(v + 0.5)), want_n.numpy().reshape(1, C, -1))
    # the adjoint of the lookup for the source and the position, against torch's
    g = S.hashed_floats(C, gx.size, 72).astype(np.float64).reshape(1, C, -1)
    (want * torch.from_numpy(g).reshape(want.shape)).sum().backward()
    one = np.ones((1, 9))
    # (drive the restated backward with a grid that is the identity in uv: depth 1, inv_K = K = I would tie uv to the pixel; the
    #  lookup's part is checked here, the rest by central differences)
    offs, ok, fx, fy = S._taps(ix, iy, H, W)
    wts = [(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy]
    g_src, _ = S.scatter_src((offs, ok, [[wts[k] * g[:, c] for k in range(4)] for c in range(C)]), 1, C, H * W)
    assert np.allclose(g_src, s.grad.numpy().reshape(1, C, -1), rtol=0, atol=1e-14) and one.size == 9
    tap = [[np.where(ok[k], np.take_along_axis(src[:, c], offs[k], 1), 0) for k in range(4)] for c in range(C)]
    gix = sum(g[:, c] * ((tap[c][1] - tap[c][0]) * (1 - fy) + (tap[c][3] - tap[c][2]) * fy) for c in range(C))
    giy = sum(g[:, c] * ((tap[c][2] - tap[c][0]) * (1 - fx) + (tap[c][3] - tap[c][1]) * fx) for c in range(C))
    tg = grid.grad.numpy().reshape(-1, 2)
    smooth = (np.abs(ix - np.round(ix)) > 1e-9) & (np.abs(iy - np.round(iy)) > 1e-9)       # (at a cell boundary the one-sided slopes differ)
    assert np.allclose((gix * W / 2)[smooth], tg[:, 0][smooth[0]], rtol=0, atol=1e-13)
    assert np.allclose((giy * H / 2)[smooth], tg[:, 1][smooth[0]], rtol=0, atol=1e-13)


def test_positions_that_are_not_finite_read_zero():
    """every tap is out of bounds and the output is 0, bilinear and nearest.  torch's CPU grid_sample propagates a NaN position
    into its output (its weights are NaN and its bounds test passes for no tap only in some builds): not compared."""
    src = np.ones((1, 1, 12))
    bad = np.array([[np.nan, np.inf, -np.inf, 1e30, -1e30, 0.5]])
    ok = np.full((1, 6), 1.0)
    for ix, iy in ((bad, ok), (ok, bad)):
        out = S.lookup_bilinear(src, ix, iy, 3, 4)
        assert out[0, 0, :5].tolist() == [0, 0, 0, 0, 0] and out[0, 0, 5] > 0
        assert S.lookup_nearest(src, ix, iy, 3, 4)[0, 0].tolist() == [0, 0, 0, 0, 0, 1]


# ---- every adjoint against central differences, float64 ------------------------------------------------------------------------------
def _central(f, x, h=1e-6):
    g = np.zeros_like(x)
    flat, gf = x.reshape(-1), g.reshape(-1)
    for i in range(flat.size):
        keep = flat[i]
        flat[i] = keep + h
        hi = f()
        flat[i] = keep - h
        lo = f()
        flat[i] = keep
        gf[i] = (hi - lo) / (2 * h)
    return g


def _near(a, b, tol=1e-7):
    return bool((np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b))).all())


def test_view_transform_adjoint_equals_central_differences():
    for n in (3, 5, 6):
        c = S.ViewCase(3, n, "hashed")
        inp = S.view_inputs(c)
        v, gr, gt = inp["view"].copy(), inp["g_rot"], inp["g_trans"]

        def value():
            R, t = S.view_transform(v)
            return (R * gr).sum() + (t * gt).sum()
        assert _near(S.view_transform_backward(v, gr, gt), _central(value, v))
        assert np.array_equal(S.view_transform_backward(v, None, gt)[:, :3], np.zeros((3, 3)))
        assert np.array_equal(S.view_transform_backward(v, gr, None)[:, 3:], np.zeros((3, n - 3)))


@pytest.mark.parametrize("kind", ["float", "general"])
@pytest.mark.parametrize("threeD", [True, False])
def test_grid_warp_adjoint_equals_central_differences(kind, threeD):
    c = S.GridCase(2, 3, 5, 2, None, kind)
    inp = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in S.grid_inputs(c).items()}
    if kind == "general":
        assert (inp["K"][:, [1, 3]] != 0).all() and (inp["inv_K"] != 0).all() and not np.array_equal(inp["K"][0], inp["K"][1])
    K, g = (None, inp["g3"]) if threeD else (inp["K"], inp["g2"])

    def value():
        return (S.grid_warp(inp["depth"], inp["inv_K"], inp["A"], inp["t"], inp["cz"], K, None, c.H, c.W) * g).sum()
    gd, terms = S.grid_warp_backward(inp["depth"], inp["inv_K"], inp["A"], inp["t"], inp["cz"], K, g, c.H, c.W)
    sums = S.reduce_terms(terms, 0)
    assert _near(gd, _central(value, inp["depth"]))
    assert _near(sums[:, :9], _central(value, inp["A"])) and _near(sums[:, 9:], _central(value, inp["t"]))


def test_depth_normals_adjoint_equals_central_differences():
    c = S.NormalCase(2, 5, 4, "float")
    inp = S.normal_inputs(c)
    d = inp["depth"].copy()
    assert not np.array_equal(inp["inv_K"][0], inp["inv_K"][1])
    assert _near(S.depth_normals_backward(d, inp["inv_K"], inp["g"], c.H, c.W),
                 _central(lambda: (S.depth_normals(d, inp["inv_K"], c.H, c.W) * inp["g"]).sum(), d, 1e-7), 2e-6)


def test_depth_normals_where_the_normal_vanishes():
    """c = 0 where |n| = 0: the gradient is that of n / eps there (torch autograd of n / (|n| + eps) gives NaN: 0 / 0 in d|n|/dn)"""
    c = S.NormalCase(2, 9, 5, "zero_patch")
    inp = S.normal_inputs(c)
    n = S.depth_normals(inp["depth"], inp["inv_K"], c.H, c.W)
    vanish = (n[:, 1:-1, 1:-1] == 0).all(-1)
    assert vanish.sum() >= 3
    g = S.depth_normals_backward(inp["depth"], inp["inv_K"], inp["g"], c.H, c.W)
    assert np.isfinite(g).all() and np.abs(g).max() > 1e5          # (the 1 / eps of a vanishing normal reaches its neighbours)
    d = torch.from_numpy(inp["depth"]).reshape(c.B, c.H, c.W).requires_grad_(True)
    x, y = (torch.from_numpy(v).double() for v in S.pixel_xy(c.H, c.W, inp["depth"]))
    iK = torch.from_numpy(inp["inv_K"])
    P = torch.stack([(x * iK[:, 3 * k:3 * k + 1] + y * iK[:, 3 * k + 1:3 * k + 2] + iK[:, 3 * k + 2:3 * k + 3]).reshape(c.B, c.H, c.W) * d for k in range(3)], -1)
    nn = torch.linalg.cross(P[:, 1:-1, 2:] - P[:, 1:-1, :-2], P[:, 2:, 1:-1] - P[:, :-2, 1:-1], dim=3)
    out = nn / ((nn ** 2).sum(3, keepdim=True) ** 0.5 + S.DN_EPS)
    (out * torch.from_numpy(inp["g"][:, 1:-1, 1:-1])).sum().backward()
    assert bool(torch.isnan(d.grad).any())
    ok = ~torch.isnan(d.grad).numpy().reshape(c.B, -1)
    assert ok.sum() > 20 and _near(g[ok], d.grad.numpy().reshape(c.B, -1)[ok], 1e-9)       # elsewhere they agree


def test_textures_adjoint_is_the_transpose():
    for c in S.tex_cases():
        inp = S.tex_inputs(c)
        tex, g_im = tex_reference(c)
        assert tex.shape == inp["g"].shape and (tex * inp["g"]).sum() == (inp["im"] * g_im).sum()


@pytest.mark.parametrize("kind", ["float", "general"])
def test_warp_resample_adjoint_equals_central_differences(kind):
    c = S.ResampleCase(2, 3, 5, 4, 6, 2, 0, 2, kind)
    inp = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in S.resample_inputs(c).items()}
    inp["A"] = S.rotations_of(S.hashed_floats(2, 3, 81, -0.05, 0.05))           # (most samples inside)

    def value():
        return (S.warp_resample(inp["depth"], inp["inv_K"], inp["K"], inp["A"], inp["t"], inp["cz"], inp["src"], None, c.h, c.w, c.H, c.W)[0]
                * inp["g"]).sum()
    _, _, (ix, iy) = S.warp_resample(inp["depth"], inp["inv_K"], inp["K"], inp["A"], inp["t"], inp["cz"], inp["src"], None, c.h, c.w, c.H, c.W)
    assert ((ix > 0) & (ix < c.W - 1)).sum() > 10 and np.abs(ix - np.round(ix)).min() > 1e-4 and np.abs(iy - np.round(iy)).min() > 1e-4
    contrib, gd, terms = S.warp_resample_backward(inp["depth"], inp["inv_K"], inp["K"], inp["A"], inp["t"], inp["cz"], inp["src"],
                                                  inp["g"], c.h, c.w, c.H, c.W)
    sums = S.reduce_terms(terms, 0)
    assert _near(S.scatter_src(contrib, c.B, c.C, c.H * c.W)[0], _central(value, inp["src"]))
    assert _near(gd, _central(value, inp["depth"]), 1e-6)
    assert _near(sums[:, :9], _central(value, inp["A"]), 1e-6) and _near(sums[:, 9:], _central(value, inp["t"]), 1e-6)
    assert np.abs(sums).min() > 1e-3


# ---- exact cases: the float32 evaluation gives the float64 bits ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in S.grid_forward_cases() if c.kind == "exact"], ids=S.case_id)
def test_exact_grid_warp_forward_cases_are_exact(c):
    for threeD in (True, False):
        assert S.same_bits(grid_forward(c, threeD, "f32"), grid_forward(c, threeD, "f64")), threeD
    assert math.log2(c.W - 1).is_integer() and math.log2(c.H - 1).is_integer()
    q = grid_forward(c, True, "f64")[:, :, 2]
    assert (np.frexp(q)[0] == 0.5).all()                  # q.z is a power of two
    if c.crop:
        assert c.crop[0] + c.crop[1] < c.H and c.crop[2] + c.crop[3] < c.W


def test_the_extreme_crops_keep_one_row_and_one_column():
    crops = [c.crop for c in S.grid_forward_cases() if c.crop]
    assert any(c.crop and c.crop[0] + c.crop[1] == c.H - 1 and c.crop[2] + c.crop[3] == c.W - 1 for c in S.grid_forward_cases())
    for side in range(4):
        assert any(cr[side] > 0 and sum(cr) == cr[side] for cr in crops), side
    assert any(all(v > 0 for v in cr) for cr in crops)


@pytest.mark.parametrize("c", [c for c in S.grid_backward_cases() if c.kind == "exact"], ids=S.case_id)
def test_exact_grid_warp_backward_cases_are_exact(c):
    for threeD in (True, False):
        a, b = grid_backward(c, threeD, "f32"), grid_backward(c, threeD, "f64")
        for k in range(3):
            assert S.same_bits(a[k], b[k]), (threeD, k)
        for x, y in zip(a[3], b[3]):
            assert S.same_bits(x, y), threeD
        assert all(S.exact_sum_proven(t, 1) for t in b[3]), threeD            # any order of the sum gives these bits
        assert all(np.abs(t).sum() > 0 for t in b[3][:2] + b[3][9:11]), threeD
        if not threeD and c.H * c.W > 600:
            assert (S.grid_inputs(c)["g2"][:, -1] != 0).any()       # the last pixel: the last strided pass carries a term


def test_textures_are_exact_for_integers():
    for c in S.tex_cases():
        inp = S.tex_inputs(c)
        tex, g_im = tex_reference(c)
        assert S.same_bits(S.textures_from_im(inp["im"].astype(np.float32), c.ts), tex)
        assert S.same_bits(S.textures_from_im_backward(inp["g"].astype(np.float32), c.B, c.C, c.H, c.W, c.ts), g_im)
        assert np.abs(g_im).max() * 2 < 2 ** 24


def test_zero_views_are_exact():
    for c in S.view_cases():
        if c.kind == "zero":
            R, t = view_forward(c, "f32")
            assert S.same_bits(R, np.repeat(IDENTITY, c.B, 0)) and S.same_bits(t, view_forward(c, "f64")[1])
            assert S.same_bits(view_backward(c, ar="f32"), view_backward(c, ar="f64"))


def _regions(ix, iy, H, W):
    rx = np.where(ix < -0.5, 0, np.where(ix > W - 0.5, 2, 1))
    ry = np.where(iy < -0.5, 0, np.where(iy > H - 0.5, 2, 1))
    return set((3 * ry + rx).reshape(-1).tolist())


@pytest.mark.parametrize("c", [c for c in S.resample_cases() if c.kind in ("exact", "zoom")], ids=S.case_id)
def test_exact_warp_resample_cases_are_exact(c):
    out32, near32, (ix32, iy32) = resample_forward(c, "f32")
    out, near, (ix, iy) = resample_forward(c, "f64")
    assert S.same_bits(ix32, ix) and S.same_bits(iy32, iy) and S.same_bits(out32, out)
    assert near is None or np.array_equal(near32, near)
    a, b = resample_backward(c, "f32"), resample_backward(c, "f64")
    assert S.same_bits(a[1], b[1]) and all(S.same_bits(x, y) for x, y in zip(a[3], b[3]))
    # one workgroup's sums are proven exact in any order at the maps of up to 153 pixels
    assert partials_exact(c) == (c.kind == "exact" and c.h * c.w <= 153)
    for ch in range(c.C):
        for k in range(4):
            assert S.same_bits(a[0][2][ch][k], b[0][2][ch][k])
    inp = S.resample_inputs(c)
    g_src, mag = S.scatter_src(b[0], c.B, c.C, c.H * c.W, inp["prefill"])
    vals = np.concatenate([np.where(b[0][1][k], b[0][2][ch][k], 0).reshape(-1) for ch in range(c.C) for k in range(4)])
    assert S.exact_sum_proven(np.concatenate([vals, inp["prefill"].reshape(-1)]), total=mag.max()) and S.same_bits(
        S.scatter_src(a[0], c.B, c.C, c.H * c.W, inp["prefill"], np.float32)[0], g_src)
    if c.kind == "zoom":
        hits = np.zeros(c.H * c.W)
        np.add.at(hits, b[0][0][0][0][b[0][1][0][0]], 1)
        assert hits.max() >= 8                     # many outputs add into one source texel
        return
    assert (ix - np.floor(ix) == 0.5).any() and (iy - np.floor(iy) == 0.5).any()
    # positions exactly at k + 1/2 in both axes at once, where half-to-even and half-away-from-zero disagree
    half = (ix - np.floor(ix) == 0.5) & (iy - np.floor(iy) == 0.5)
    assert half.any()
    if near is not None:
        away = S.lookup_nearest(inp["src_n"], ix, iy, c.H, c.W, rounding=lambda v: np.sign(v) * np.floor(np.abs(v) + 0.5))
        assert not np.array_equal(away, near)
    if (c.h, c.w) != (2, 2):
        assert _regions(ix, iy, c.H, c.W) == set(range(9))
        x0, y0 = np.floor(ix), np.floor(iy)
        for v, n in ((x0, c.W), (y0, c.H)):
            assert (v == -1).any() and (v == n - 1).any() and (v <= -2).any() and (v > n).any()       # partial taps, the clamp


# ---- float cases: the tolerance is small, and it is sharp -----------------------------------------------------------------------------
def _exceeds(wrong, right, tol):
    with np.errstate(invalid="ignore"):
        return bool((np.abs(np.asarray(wrong, np.float64) - right) > tol).any())


def _small(tol, ref, what):
    """the tolerance is a small part of the result's scale"""
    assert np.isfinite(tol).all() and float(np.median(tol)) < 1e-2 * max(1.0, float(np.abs(ref).max())), what


@pytest.mark.parametrize("c", [c for c in S.grid_forward_cases() if c.kind != "exact"], ids=S.case_id)
def test_grid_warp_forward_float_cases_are_sharp(c):
    ref3, tol3 = grid_forward_reference(c, True)
    ref2, tol2 = grid_forward_reference(c, False)
    _small(tol3, ref3, "3-D")
    _small(tol2, ref2, "2-D")
    if c.H != c.W:
        assert _exceeds(grid_forward(c, False, "f64", "swap_wh"), ref2, tol2)
    if c.kb > 1:
        assert _exceeds(grid_forward(c, True, "f64", "entry0"), ref3, tol3) and _exceeds(grid_forward(c, False, "f64", "entry0"), ref2, tol2)


@pytest.mark.parametrize("c", [c for c in S.grid_backward_cases() if c.kind != "exact"], ids=S.case_id)
def test_grid_warp_backward_float_cases_are_sharp(c):
    for threeD in (True, False):
        ref = grid_backward_reference(c, threeD)
        _small(ref["g_depth"][1], ref["g_depth"][0], "g_depth")
        assert all(np.isfinite(tol).all() for _, tol in ref.values())
        variants = ["skip_run"] if c.H * c.W >= 512 else []
        if not threeD:
            variants += (["swap_wh"] if c.H != c.W else []) + (["drop_K13"] if c.kind == "general" else [])
        if c.kb > 1:
            variants.append("entry0")
        for v in variants:
            gd, gA, gt, _ = grid_backward(c, threeD, "f64", v)
            missed = [k for k, x in (("g_depth", gd), ("g_A", gA), ("g_t", gt)) if _exceeds(x, *ref[k])]
            # (a left-out run does not touch g_depth; with a 3-D gradient g_t is the sum of the incoming gradient alone)
            want = ["g_A", "g_t"] if v == "skip_run" else (["g_depth", "g_A"] if threeD else ["g_depth", "g_A", "g_t"])
            assert missed == want, (threeD, v, missed)


@pytest.mark.parametrize("c", S.normal_cases(), ids=S.case_id)
def test_depth_normals_float_cases_are_sharp(c):
    (n, ntol), (g, gtol) = normals_reference(c)
    assert np.isfinite(ntol).all() and np.isfinite(gtol).all() and (ntol < 1e-4).all()
    interior = c.H > 2 and c.W > 2
    assert interior == ((c.B, c.H, c.W) not in ((1, 1, 7), (1, 7, 2), (2, 2, 2)))
    if not interior:
        assert np.array_equal(g, np.zeros_like(g)) and (gtol == 0).all() and (n[..., :2] == 0).all()
        assert (np.abs(n[..., 2] - float(BORDER_NORMAL_Z)) <= ntol[..., 2]).all()
        return
    assert _exceeds(normals_backward(c, "f64", "flip_sign"), g, gtol)
    if c.B > 1:
        inp = S.normal_inputs(c)
        assert _exceeds(S.depth_normals(inp["depth"], inp["inv_K"][:1], c.H, c.W), n, ntol)
        assert _exceeds(S.depth_normals_backward(inp["depth"], inp["inv_K"][:1], inp["g"], c.H, c.W), g, gtol)
    # each element has its own bound: the border's is exactly zero, the interior's relative to its own size
    assert (gtol.reshape(c.B, c.H, c.W)[:, 0, 0] == 0).all()
    if c.kind == "float":
        rel = float((gtol / np.maximum(np.abs(g), 1e-30))[np.abs(g) > 0.1 * np.abs(g).max()].max())
        print("NORMALS", S.case_id(c), "largest tolerance / |g| among the large elements", rel)
        assert rel < 0.05


@pytest.mark.parametrize("c", [c for c in S.view_cases() if c.kind != "zero"], ids=S.case_id)
def test_view_transform_float_cases(c):
    (R, Rtol), (t, ttol), (g, gtol) = view_reference(c)
    assert (Rtol <= S.MARGIN * S.U * 120).all() and (ttol == 0).all() and (gtol[:, 3:] == 0).all()
    assert (gtol[:, :3] < 1e-4).all()
    if c.kind == "quarter":
        assert np.abs(R - np.round(R)).max() < 1e-7          # exact zeros and ones, up to the float32 rounding of pi / 2
    # sharp: Ry Rx multiplied in the other order
    inp = S.view_inputs(c)
    v = inp["view"].copy()
    v[:, [0, 1]] = v[:, [1, 0]]
    if c.kind == "hashed":
        assert _exceeds(S.view_transform(v)[0], R, Rtol)


@pytest.mark.parametrize("c", [c for c in S.resample_cases() if c.kind in ("float", "general")], ids=S.case_id)
def test_warp_resample_float_cases_are_sharp(c):
    ref = resample_reference(c)
    for k in ("out", "g_depth"):
        _small(ref[k][1], ref[k][0], k)
    assert np.isfinite(ref["partials"][1]).all()
    assert np.isfinite(ref["g_src"][1]).all()
    variants = (["swap_wh"] if c.h != c.w else []) + (["W_for_w"] if c.W != c.w else []) + (["entry0"] if c.kb > 1 else []) + (["drop_K13"] if c.kind == "general" else [])
    for v in variants:
        if v != "drop_K13":
            assert _exceeds(resample_forward(c, "f64", v)[0], *ref["out"]), v
        _, gd, parts, _ = resample_backward(c, "f64", v)
        assert _exceeds(gd, *ref["g_depth"]) and _exceeds(parts, *ref["partials"]), v
    # a 256-pixel run left out: one workgroup's partial sums change
    if c.h * c.w >= 512:
        _, _, _, terms = resample_backward(c, "f64")
        parts = S.resample_parts(c.h, c.w)
        cut = [t.copy() for t in terms]
        for t in cut:
            t[:, 256:512] = 0
        assert _exceeds(S.resample_partials(cut, parts), *ref["partials"])


@pytest.mark.parametrize("c", [c for c in S.resample_cases() if c.kind in ("float", "general") and c.Cn], ids=S.case_id)
def test_nearest_positions_keep_clear_of_every_rounding_boundary(c):
    """so that the float32 position rounds to the same texel: no mask difference is allowed on the device"""
    _, _, (ix, iy) = resample_forward(c, "err")
    for p, n in ((ix, c.W), (iy, c.H)):
        away = np.abs(p.v - np.floor(p.v) - 0.5)           # distance to k + 1/2; the image's edges -1/2 and n - 1/2 are among them
        assert (away > S.tolerance(p.e)).all(), float((S.tolerance(p.e) / away).max())
    _, near, _ = resample_forward(c, "f64")
    assert S.nearest_clearance(c, S.resample_inputs(c)) < 1
    assert c.h * c.w < 20 or ((near != 0).sum() > 5 and (near == 0).sum() > 5)            # inside and outside both occur


# ---- the launcher arithmetic ---------------------------------------------------------------------------------------------------------
def test_every_case_takes_the_path_it_is_there_for():
    gw = {(c.B, c.H, c.W): (S.grid_warp_split(c.B, c.H * c.W), S.strided_passes(c.H * c.W, S.grid_warp_split(c.B, c.H * c.W)))
          for c in S.grid_backward_cases()}
    assert gw[(1, 5, 9)] == (1, (0, 1)) and gw[(3, 17, 33)] == (1, (2, 3))               # a plain store
    assert gw[(2, 32, 32)] == (2, (2, 2))                                                  # two workgroups, no tail
    assert gw[(2, 17, 65)] == (2, (2, 3))                                                  # lanes of 2 and 3 passes
    assert gw[(2, 65, 129)][0] == 16 and gw[(129, 65, 129)][0] == 8 and 129 * 16 > 2048 >= 129 * 8
    assert gw[(2049, 17, 65)][0] == 1 and min(16, 1105 // 512) == 2 and 2049 * 2 > 2048    # halved to a plain store
    assert S.grid_warp_path(2049, 1105) == "store" and S.grid_warp_path(2, 1024) == "atomics"
    # forward, one lane per pixel: (3, 9, 17) spans two workgroups with a batch boundary inside one and a ragged tail
    assert S.blocks_for(3 * 9 * 17) == 2 and 153 < 256 < 2 * 153 and (3 * 153) % 256 != 0
    assert S.blocks_for(3 * 17 * 33) > 3                                                    # normals over several workgroups
    assert [S.blocks_for(B, 64) for B in (1, 64, 65)] == [1, 1, 2]                          # the view kernels' workgroups of 64
    rs = {(c.h, c.w): S.resample_parts(c.h, c.w) for c in S.resample_cases()}
    assert rs[(2, 2)] == 1 and rs[(16, 16)] == 1 and rs[(3, 129)] == 2 and rs[(9, 17)] == 1 and rs[(17, 5)] == 1
    assert rs[(65, 129)] == 32 and S.blocks_for(65 * 129) == 33 and S.strided_passes(65 * 129, 32) == (1, 2)      # the cap, a second pass
    assert S.resample_parts(0, 8) == 0
    assert any((c.H, c.W) != (c.h, c.w) for c in S.resample_cases()) and {c.C for c in S.resample_cases()} == {1, 3}
    assert {c.Cn for c in S.resample_cases()} == {0, 1, 2} and {c.kb for c in S.resample_cases() if c.B > 1} == {1, 2, 3}


def test_the_library_sizes_the_partials_as_restated():
    from deep3dmap_amd import _lib
    f = _lib.lib().d3m_warp_resample_partials
    for h, w in ((2, 2), (16, 16), (16, 17), (3, 129), (65, 129), (64, 128), (2000, 2000), (0, 5), (5, 0), (-1, 4)):
        assert f(h, w) == S.resample_parts(h, w), (h, w)


# ---- the C entry points' refusals (nothing is launched; the pointers are never dereferenced) --------------------------------------------
P = 0x10000


def _call(name, defaults, **over):
    from deep3dmap_amd import _lib
    args = dict(defaults, **over)
    return getattr(_lib.lib(), name)(*args.values(), None)


def _crop(*v):
    return (ctypes.c_int * 4)(*v)


VIEW_F = dict(view=P, n=6, rot=P, trans=P, B=2)
VIEW_B = dict(view=P, n=6, g_rot=P, g_trans=P, g_view=P, B=2)
GW_F = dict(depth=P, inv_K=P, iKb=1, rot=P, trans=P, cz=1.0, K=P, Kb=1, crop=None, out=P, B=2, H=5, W=9)
GW_B = dict(depth=P, inv_K=P, iKb=1, rot=P, trans=P, cz=1.0, K=P, Kb=1, g_out=P, g_depth=P, g_rot=P, g_trans=P, B=2, H=5, W=9)
DN_F = dict(depth=P, inv_K=P, iKb=1, normal=P, B=2, H=5, W=9)
DN_B = dict(depth=P, inv_K=P, iKb=1, g_normal=P, g_depth=P, B=2, H=5, W=9)
TX_F = dict(im=P, tex=P, B=2, C=3, H=5, W=9, ts=2)
TX_B = dict(g_tex=P, g_im=P, B=2, C=3, H=5, W=9, ts=2)
WR_F = dict(depth=P, inv_K=P, iKb=1, K=P, Kb=1, rot=P, trans=P, cz=1.0, src=P, C=3, src_n=P, Cn=1, out=P, out_n=P, B=2, h=5, w=9, H=4, W=6)
WR_B = dict(depth=P, inv_K=P, iKb=1, K=P, Kb=1, rot=P, trans=P, cz=1.0, src=P, C=3, g_out=P, g_src=P, g_depth=P, partials=P, B=2, h=5, w=9,
            H=4, W=6)

REFUSALS = {
    "d3m_view_transform": (VIEW_F, [dict(view=None), dict(rot=None), dict(trans=None), dict(B=0), dict(B=-1)] +
                           [dict(n=n) for n in (0, 2, 4, 7, -3)]),
    "d3m_view_transform_backward": (VIEW_B, [dict(view=None), dict(g_view=None), dict(B=0), dict(B=-2)] + [dict(n=n) for n in (0, 2, 4, 7)]),
    "d3m_grid_warp": (GW_F, [dict(depth=None), dict(inv_K=None), dict(rot=None), dict(trans=None), dict(out=None), dict(B=0), dict(H=0),
                             dict(W=0), dict(W=-9), dict(iKb=0), dict(iKb=3), dict(Kb=0), dict(Kb=3), dict(crop=_crop(-1, 0, 0, 0)),
                             dict(crop=_crop(0, -1, 0, 0)), dict(crop=_crop(0, 0, -1, 0)), dict(crop=_crop(0, 0, 0, -1)),
                             dict(crop=_crop(3, 2, 0, 0)), dict(crop=_crop(5, 0, 0, 0)), dict(crop=_crop(0, 0, 4, 5)),
                             dict(crop=_crop(0, 0, 0, 9)), dict(crop=_crop(0, 0, 9, 0))]),
    "d3m_grid_warp_backward": (GW_B, [dict(depth=None), dict(inv_K=None), dict(rot=None), dict(trans=None), dict(g_out=None), dict(B=0),
                                      dict(H=0), dict(W=0), dict(iKb=3), dict(iKb=0), dict(Kb=3), dict(Kb=0)]),
    "d3m_depth_normals": (DN_F, [dict(depth=None), dict(inv_K=None), dict(normal=None), dict(B=0), dict(H=0), dict(W=0), dict(iKb=0), dict(iKb=3)]),
    "d3m_depth_normals_backward": (DN_B, [dict(depth=None), dict(inv_K=None), dict(g_normal=None), dict(g_depth=None), dict(B=0), dict(H=0),
                                          dict(W=-1), dict(iKb=0), dict(iKb=3)]),
    "d3m_textures_from_im": (TX_F, [dict(im=None), dict(tex=None), dict(B=0), dict(C=0), dict(H=1), dict(W=1), dict(H=0), dict(ts=0), dict(ts=3),
                                    dict(ts=-2)]),
    "d3m_textures_from_im_backward": (TX_B, [dict(g_tex=None), dict(g_im=None), dict(B=0), dict(C=0), dict(H=1), dict(W=1), dict(ts=0),
                                             dict(ts=3)]),
    "d3m_warp_resample": (WR_F, [dict(depth=None), dict(inv_K=None), dict(K=None), dict(rot=None), dict(trans=None), dict(src=None),
                                 dict(out=None), dict(B=0), dict(h=1), dict(w=1), dict(h=0), dict(H=0), dict(W=0), dict(C=0),
                                 dict(B=2, h=2 ** 14, w=2 ** 15), dict(B=1, h=2 ** 15, w=2 ** 15), dict(iKb=0), dict(iKb=3), dict(Kb=0),
                                 dict(Kb=3), dict(out_n=None), dict(Cn=0), dict(Cn=-1)]),
    "d3m_warp_resample_backward": (WR_B, [dict(depth=None), dict(inv_K=None), dict(K=None), dict(rot=None), dict(trans=None), dict(src=None),
                                          dict(g_out=None), dict(partials=None), dict(B=0), dict(h=1), dict(w=1), dict(H=0), dict(W=0),
                                          dict(C=0), dict(B=2, h=2 ** 14, w=2 ** 15), dict(iKb=3), dict(Kb=3)]),
}
# accepted forms next to the refused ones (driven on the device only: they launch)
ACCEPTED = {
    "d3m_grid_warp": [dict(K=None, Kb=7), dict(crop=_crop(4, 0, 0, 8)), dict(crop=_crop(2, 2, 4, 4)), dict(iKb=2, Kb=2)],
    "d3m_warp_resample": [dict(src_n=None, out_n=None, Cn=0), dict(src_n=None, out_n=None, Cn=-1), dict(iKb=2, Kb=2)],
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals(name):
    defaults, cases = REFUSALS[name]
    for over in cases:
        assert set(over) <= set(defaults), over
        assert _call(name, defaults, **over) == 1, over
    assert (2 * 2 ** 14 * 2 ** 15) > 0x3FFFFFFF >= 2 ** 15 * 2 ** 15 - 1 and 2 ** 15 * 2 ** 15 > 0x3FFFFFFF
