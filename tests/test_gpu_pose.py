"""The weak-perspective pose node on the device (neural_renderer/pose.py, core/pose_tools.py): forward and adjoint bit for bit
on integer inputs at every shape where the kernels take another path, float inputs against the float64 restatement within the
derived bounds (tests/pose_scenes.py), two runs and a captured step bit for bit, and the chain param2points_bfm ->
face_project -> Pt3dRenderer.sample with landmarks68 and supervised_losses beside it."""
import functools
import math
from collections import Counter

import numpy as np
import pytest
import torch

import pose_scenes as ps
from conftest import kernels_launched

pytestmark = pytest.mark.gpu
KERNELS = {"k_pose_forward", "k_pose_backward_chunks", "k_pose_backward_finish"}
LIMIT = float(np.float32(ps.ANGLE_LIMIT))       # what the kernels clamp at: the f32 nearest 3.1415


def _po():
    from deep3dmap_amd.neural_renderer import pose as po
    return po


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _sizes():
    po = _po()
    chunk = po.VERTICES_PER_CHUNK
    return ([1, 63, 64, 65, chunk - 1, chunk, 2 * chunk + 3, chunk * po.MAX_PARTS + 5], [1, 3, po.FINISH_SETS + 1],
            [0, 1, 68, 300])


# ---- 1. exact integers ----------------------------------------------------------------------------------------------------
TAU, UV = 4, 1


@functools.lru_cache(maxsize=2)
def _integer_inputs(V, B, shared):
    """s in {-2..2}, x in {-3..3}, t in {-5..5}, angles 0, incoming gradients in {-2..2}: int64 arrays (shared, never written)"""
    x = ps.hashed_ints((1 if shared else B) * V, 3, 101, -3, 3).reshape(-1, V, 3)
    pose = np.zeros((B, 7), np.int64)
    pose[:, 0] = ps.hashed_ints(B, 1, 102, -2, 2)[:, 0]
    pose[:, 4:7] = ps.hashed_ints(B, 3, 103, -5, 5)
    g_posed = ps.hashed_ints(B * V, 3, 104, -2, 2).reshape(B, V, 3)
    g_uv = ps.hashed_ints(B * V, 2, 105, -2, 2).reshape(B, V, 2)
    return x, pose, g_posed, g_uv


def _integer_answers(x, pose, G):
    """the int64 adjoint at angles 0 (R = 1, dR/da_k the generators of the rotations about x, y, z) for G [B,V,3]:
    (grad_pose [B,7], grad_vertices [1 or B,V,3], the largest absolute sum)"""
    B = pose.shape[0]
    M = np.einsum("bvj,bvc->bjc", G, np.broadcast_to(x, (B,) + x.shape[1:]))
    s = pose[:, 0]
    gp = np.zeros((B, 7), np.int64)
    gp[:, 0] = M[:, 0, 0] + M[:, 1, 1] + M[:, 2, 2]
    gp[:, 1] = s * (M[:, 2, 1] - M[:, 1, 2])
    gp[:, 2] = s * (M[:, 0, 2] - M[:, 2, 0])
    gp[:, 3] = s * (M[:, 1, 0] - M[:, 0, 1])
    gp[:, 4:7] = TAU * G.sum(1)
    gx = s[:, None, None] * G
    if x.shape[0] == 1:             # shared vertices (or one set)
        gx = gx.sum(0, keepdims=True)
    return gp, gx, int(max(np.abs(M).max(), np.abs(gp).max(), np.abs(gx).max()))


def _integer_case(V, B, L, shared, mode):
    """The inputs of one case, which outputs it asks for, and its exact answers (host only)."""
    x, pose, g_posed, g_uv = _integer_inputs(V, B, shared)
    idx = ps.landmark_indices(L, V, repeats=L == 300) if L else None
    use = {"posed": mode in ("posed", "all"), "uv": mode in ("uv", "all"), "lm": L > 0 and mode in ("lm", "all")}
    posed = pose[:, None, 0:1] * np.broadcast_to(x, (B, V, 3)) + TAU * pose[:, None, 4:7]
    want, grads = {}, {}
    G = np.zeros((B, V, 3), np.int64)
    if use["posed"]:
        want["posed"], grads["posed"] = posed, g_posed
        G += g_posed
    if use["uv"]:
        want["uv"], grads["uv"] = np.stack([posed[..., 0], 1 - posed[..., 1]], -1), g_uv
        G[..., 0] += g_uv[..., 0]
        G[..., 1] -= g_uv[..., 1]
    if use["lm"]:
        want["landmarks"], grads["landmarks"] = posed[:, idx], ps.hashed_ints(B * L, 3, 106, -2, 2).reshape(B, L, 3)
        np.add.at(G, (slice(None), idx), grads["landmarks"])
    gp, gx, largest = _integer_answers(x, pose, G)
    assert largest < 2 ** 24 and np.abs(posed).max() < 2 ** 24
    return x, pose, idx, use, want, grads, gp, gx, largest


def _equal(got, want, what):
    assert got is not None and torch.equal(got.detach().cpu().double(), torch.from_numpy(np.ascontiguousarray(want)).double()), what


def _check_integers(V, B, L, shared, mode, strided_pose=False, misaligned=False):
    """One case through nr.pose_vertices; returns the largest sum behind its answers."""
    from deep3dmap_amd import neural_renderer as nr
    x, pose, idx, use, want, grads, gp, gx, largest = _integer_case(V, B, L, shared, mode)
    if misaligned:          # the same vertices 4 bytes off a 16-byte boundary
        room = torch.zeros(x.size + 1, device="cuda")
        room[1:] = _dev(x).reshape(-1)
        d_x = room[1:].view(x.shape)
        assert d_x.data_ptr() % 16 == 4
    else:
        d_x = _dev(x)
    d_x = (d_x[0] if shared else d_x).detach().requires_grad_(True)
    if strided_pose:        # the pose as param2points_bfm hands it back: columns 228:235 of rows of 235
        preds = torch.zeros(B, 235, device="cuda")
        preds[:, 228:] = _dev(pose)
        preds.requires_grad_(True)
        d_pose = preds[:, 228:235]
        assert d_pose.stride() == (235, 1)
    else:
        d_pose = preds = _dev(pose).requires_grad_(True)
    out = nr.pose_vertices(d_x, d_pose, TAU, None, UV if use["uv"] else None, _dev(idx, torch.int64) if use["lm"] else None,
                           posed=use["posed"])
    for name in ("posed", "uv", "landmarks"):
        if name in want:
            _equal(getattr(out, name), want[name], (name, V, B, L, shared, mode))
        else:
            assert getattr(out, name) is None
    torch.autograd.backward([getattr(out, name) for name in want], [_dev(grads[name]) for name in want])
    _equal(preds.grad[:, 228:] if strided_pose else preds.grad, gp, ("grad_pose", V, B, L, shared, mode))
    _equal(d_x.grad, gx[0] if shared else gx, ("grad_vertices", V, B, L, shared, mode))
    if strided_pose:
        assert float(preds.grad[:, :228].abs().max()) == 0
    return largest


def _integer_cases(V):
    """The cross product of B, L, shared or per-set vertices and the outputs asked for (each alone and all together; the
    landmark output exists from L = 1 on, and `posed` / `uv` alone do not depend on L, so they run once, at L = 0)."""
    _, Bs, Ls = _sizes()
    return [(V, B, L, shared, mode) for B in Bs for shared in (True, False) for L in Ls
            for mode in (("posed", "uv", "all") if L == 0 else ("lm", "all"))]


@pytest.mark.parametrize("V", [1, 63, 64, 65, 255, 256, 515, 16389])
def test_integer_inputs_are_exact_at_every_shape(V):
    po = _po()
    Vs, Bs, Ls = _sizes()
    assert V in Vs and 16389 == po.VERTICES_PER_CHUNK * po.MAX_PARTS + 5 and Vs[4:7] == [255, 256, 515]
    largest, cases = 0, 0
    with kernels_launched() as k:
        for case in _integer_cases(V):
            largest = max(largest, _check_integers(*case))
            cases += 1
        if V == 515:
            largest = max(largest, _check_integers(V, 3, 68, False, "all", strided_pose=True))
            largest = max(largest, _check_integers(V, 3, 68, True, "all", misaligned=True))
            cases += 2
    # one launch forward, at most two backward, and nothing else of the library
    assert set(k.names) == KERNELS, k.names
    assert k.times["k_pose_forward"][0] == cases
    assert k.times["k_pose_backward_chunks"][0] == cases and k.times["k_pose_backward_finish"][0] == cases
    # the sums are neither trivial nor inexact (a sum over fewer than a chunk of terms of size <= 12 does not reach 1000)
    assert largest < 2 ** 24
    if V >= po.VERTICES_PER_CHUNK - 1:
        assert largest > 1000, largest


def test_an_unused_output_costs_nothing_and_unneeded_gradients_are_not_computed():
    from deep3dmap_amd import neural_renderer as nr
    V, B, L = 515, 3, 68
    x, pose, g_posed, g_uv = _integer_inputs(V, B, False)
    idx = ps.landmark_indices(L, V)
    g_lm = ps.hashed_ints(B * L, 3, 106, -2, 2).reshape(B, L, 3)
    G = np.zeros((B, V, 3), np.int64)
    np.add.at(G, (slice(None), idx), g_lm)
    gp, gx, _ = _integer_answers(x, pose, G)
    head = nr.PoseHead(idx, translation_scale=TAU, uv_size=UV).cuda()
    d_x, d_pose = _dev(x).requires_grad_(True), _dev(pose).requires_grad_(True)
    out = head(d_x, d_pose)                     # all three outputs, a gradient from the landmarks only
    with kernels_launched() as k:
        out.landmarks.backward(_dev(g_lm))
    assert k.times["k_pose_backward_chunks"][0] == 1 and k.times["k_pose_backward_finish"][0] == 1
    _equal(d_pose.grad, gp, "grad_pose")
    _equal(d_x.grad, gx, "grad_vertices")
    # only the pose requires grad and only the landmarks carry one: the finish launch alone, O(B L)
    p2 = _dev(pose).requires_grad_(True)
    out = head(_dev(x), p2)
    with kernels_launched() as k:
        out.landmarks.backward(_dev(g_lm))
    assert set(k.names) == {"k_pose_backward_finish"}
    _equal(p2.grad, gp, "grad_pose alone")
    # only the vertices require grad
    x2 = _dev(x).requires_grad_(True)
    out = head(x2, _dev(pose))
    out.landmarks.backward(_dev(g_lm))
    _equal(x2.grad, gx, "grad_vertices alone")
    # a pose [7] and vertices [V,3]: outputs and gradients without the leading B
    x1, p1 = _dev(x[0]).requires_grad_(True), _dev(pose[0]).requires_grad_(True)
    out = head(x1, p1)
    assert out.posed.shape == (V, 3) and out.uv.shape == (V, 2) and out.landmarks.shape == (L, 3)
    out.landmarks.backward(_dev(g_lm[0]))
    gp1, gx1, _ = _integer_answers(x[:1], pose[:1], G[:1])
    _equal(p1.grad, gp1[0], "grad_pose [7]")
    _equal(x1.grad, gx1[0], "grad_vertices [V,3]")
    # landmark indices outside [0, V) raise on the first call with that tensor
    with pytest.raises(ValueError, match=r"landmarks must lie in \[0, 515\)"):
        nr.pose_vertices(_dev(x), _dev(pose), landmarks=_dev(np.array([0, 515]), torch.int64))
    with pytest.raises(ValueError, match=r"landmarks must lie in \[0, 64\)"):
        head(_dev(x[:, :64]), _dev(pose))


# ---- 2. float inputs against float64 --------------------------------------------------------------------------------------
def _float_case(V, B, L, shared, salt):
    x = ps.hashed_floats((1 if shared else B) * V, 3, salt, -3.0, 3.0).reshape(-1, V, 3)
    pose = ps.float_pose(B, salt + 1, LIMIT)
    idx = ps.landmark_indices(L, V, salt, repeats=True)
    g = [ps.hashed_floats(B * n, c, salt + 5 + c, -1.0, 1.0).reshape(B, n, c) for n, c in ((V, 3), (V, 2))]
    g.append(ps.hashed_floats(B * L, 3, salt + 9, -1.0, 1.0).reshape(B, L, 3))
    return (x[0] if shared else x), pose, idx, g


def _run_float(V, B, L, shared, salt, tau=224.0, uv_size=224.0):
    """(device outputs and gradients, float64 restatement's, the inputs as float64 tensors) of one float case"""
    from deep3dmap_amd import neural_renderer as nr
    x, pose, idx, g = _float_case(V, B, L, shared, salt)
    d_x, d_pose = _dev(x).requires_grad_(True), _dev(pose).requires_grad_(True)
    out = nr.pose_vertices(d_x, d_pose, tau, LIMIT, uv_size, _dev(idx, torch.int64))
    torch.autograd.backward(list(out), [_dev(a) for a in g])
    t = lambda a: torch.from_numpy(a).double()      # noqa: E731
    r_x, r_pose = t(x).requires_grad_(True), t(pose).requires_grad_(True)
    ref = ps.restate_node(r_x, r_pose, tau, LIMIT, uv_size, torch.from_numpy(idx))
    torch.autograd.backward(list(ref), [t(a) for a in g])
    return out, (d_x.grad, d_pose.grad), ref, (r_x.grad, r_pose.grad), (t(x), t(pose), torch.from_numpy(idx), [t(a) for a in g])


@pytest.mark.parametrize("V,B,L,shared", [(515, 3, 68, True), (16389, 2, 300, False), (65, 65, 1, False), (515, 65, 68, True)])
def test_float_inputs_within_the_derived_bounds(V, B, L, shared):
    po = _po()
    tau = uv_size = 224.0
    out, (gx, gp), ref, (rx, rp), (x, pose, idx, g) = _run_float(V, B, L, shared, 200 + V % 7)
    # the angles span (-pi, pi): the first set's lie beyond the limit (clamped, no gradient), the second's exactly at it
    assert float(pose[0, 1]) > LIMIT and float(pose[0, 2]) < -LIMIT and (B == 1 or float(pose[1, 1]) == LIMIT)
    assert float(rp[0, 1]) == 0 and float(rp[0, 2]) == 0 and float(rp[0, 3]) != 0 and (B == 1 or float(rp[1, 1]) != 0)
    assert float(gp[0, 1]) == 0 and float(gp[0, 2]) == 0
    bound = ps.posed_bound(x, pose, tau)
    frac = {"posed": (out.posed.detach().cpu().double() - ref[0].detach()).abs() / bound,
            "uv": (out.uv.detach().cpu().double() - ref[1].detach()).abs() / ps.uv_bound(x, pose, tau, uv_size),
            "landmarks": (out.landmarks.detach().cpu().double() - ref[2].detach()).abs() / bound[:, idx]}
    hits = max(Counter(idx.tolist()).values())
    absG = ps.abs_gradient(B, V, uv_size, idx, *g)
    bp, bv = ps.gradient_bounds(x, pose, tau, absG, po.pose_chain(V, L), po.vertex_chain(B if shared else 1, hits), shared, LIMIT)
    frac["grad_pose"] = (gp.cpu().double() - rp).abs() / bp
    frac["grad_vertices"] = (gx.cpu().double() - rx).abs() / bv.reshape(rx.shape)
    print(f"V={V} B={B} L={L} shared={shared}: err/bound " + ", ".join(f"{n} {float(f.max()):.3f}" for n, f in frac.items()))
    assert hits > 1 or L == 1
    for name, f in frac.items():
        assert bool((f <= 1).all()), (name, float(f.max()))
    assert bool(torch.equal(_bits(out.landmarks), _bits(out.posed[:, idx.cuda()])))       # the rows of posed, bit for bit


# ---- 3. reproducibility ---------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical_and_a_captured_step_equals_its_eager_twin():
    from deep3dmap_amd import neural_renderer as nr
    from deep3dmap_amd.graph import CapturedStep
    po = _po()
    V, B, L = 2 * po.VERTICES_PER_CHUNK + 3, 3, 68
    x, pose, idx, g = _float_case(V, B, L, True, 300)
    assert max(Counter(idx.tolist()).values()) > 1
    head = nr.PoseHead(idx, translation_scale=224.0, angle_limit=LIMIT, uv_size=224.0).cuda()
    w = [_dev(a) for a in g]

    def make():
        return _dev(x).requires_grad_(True), _dev(pose).requires_grad_(True)

    def run(vx, vp):
        vx.grad = vp.grad = None
        out = head(vx, vp)
        # (gradients that depend on the inputs)
        (((out.posed ** 2) * w[0]).sum() + (out.uv * w[1]).sum() + ((out.landmarks ** 2) * w[2]).sum()).backward()
        return torch.cat([vx.grad.reshape(-1), vp.grad.reshape(-1)])

    twin = make()
    first = run(*twin).clone()
    assert float(first.abs().max()) > 0 and torch.equal(_bits(run(*twin)), _bits(first))
    again = make()
    assert torch.equal(_bits(run(*again)), _bits(first))
    live = make()
    cs = CapturedStep(lambda: run(*live)).capture()
    for i in range(2):
        dx, dp = _dev(ps.hashed_floats(V, 3, 310 + i, -0.5, 0.5)), _dev(ps.hashed_floats(B, 7, 320 + i, -0.1, 0.1))
        with torch.no_grad():
            for t, d in ((live[0], dx), (live[1], dp), (twin[0], dx), (twin[1], dp)):
                t.add_(d)
        got = cs().clone()
        torch.cuda.synchronize()
        want = run(*twin)
        assert float(want.abs().max()) > 0 and torch.equal(_bits(got), _bits(want)), i
    cs.release()


# ---- 4. the chain ---------------------------------------------------------------------------------------------------------
def _sheet(n=6):
    """an n x n sheet over [-1, 1]^2 at z = 1 (tests/test_gpu_pt3d.py's quad): vertices, triangles, normals"""
    ys, xs = torch.meshgrid(torch.linspace(-1, 1, n), torch.linspace(-1, 1, n), indexing="ij")
    verts = torch.stack((xs, ys, torch.ones_like(xs)), -1).reshape(-1, 3)
    i = torch.arange(n * n).reshape(n, n)
    a, b, c, d = i[:-1, :-1], i[:-1, 1:], i[1:, :-1], i[1:, 1:]
    tri = torch.cat([torch.stack((a, b, c), -1).reshape(-1, 3), torch.stack((b, d, c), -1).reshape(-1, 3)], 0).int()
    return verts, tri, torch.tensor([0., 0., 1.]).repeat(n * n, 1)


def _bfm(V, B, image_size):
    """a model of V vertices in param2points_bfm's dictionaries and preds [B,235] whose pose part turns the sheet away from
    the view (so that Pt3dRenderer.sample keeps its triangles) and lands it inside the image"""
    t = lambda a: torch.from_numpy(a)       # noqa: E731
    verts = _sheet(int(round(math.sqrt(V))))[0]
    sp = {'w': t(ps.hashed_floats(3 * V, 199, 401, -0.005, 0.005)), 'sigma': t(ps.hashed_floats(1, 199, 402, 0.5, 1.5)[0]),
          'mu_shape': verts.reshape(-1, 1).clone()}
    ep = {'w_exp': t(ps.hashed_floats(3 * V, 29, 403, -0.005, 0.005))}
    op = {'sigma_exp': t(ps.hashed_floats(1, 29, 404, 0.0005, 0.0015)[0])}
    preds = t(ps.hashed_floats(B, 235, 405, -1.0, 1.0)).clone()
    preds[:, 199:228] *= 0.001
    preds[:, 228] = t(ps.hashed_floats(B, 1, 406, 0.15, 0.25)[:, 0]) * image_size
    preds[:, 229:232] = torch.tensor([0.2, math.pi - 0.3, 0.1]) + 0.05 * preds[:, 229:232]
    preds[:, 232:235] = 0.5 + 0.05 * preds[:, 232:235]
    return sp, ep, op, preds


def test_coefficients_to_uv_unwrap_and_losses_in_one_graph():
    from deep3dmap_amd import core
    po = _po()
    B, n, S, T = 2, 6, 32, 24
    V = n * n
    verts, tri, normals = _sheet(n)
    sp, ep, op, preds0 = _bfm(V, B, S)
    cuda = lambda d: {k: v.cuda() for k, v in d.items()}     # noqa: E731
    d_sp, d_ep, d_op = cuda(sp), cuda(ep), cuda(op)
    preds = preds0.clone().cuda().requires_grad_(True)
    imgs = _dev(ps.hashed_floats(B * 3 * S, S, 410, 0.0, 1.0)).view(B, 3, S, S)
    r = core.Pt3dRenderer("cuda", T, lookview=torch.tensor([0., 0., 1.]).cuda())
    with kernels_launched() as k:
        face, pose = core.param2points_bfm(d_sp, d_ep, d_op, preds)
        fp, angles = core.face_project(face, pose, S)
        img, mask = r.sample(normals.cuda(), angles, tri.cuda(), imgs, verts.cuda(), fp)
        (img[..., :3] * _dev(ps.hashed_floats(B * T * T, 3, 411)).view(B, T, T, 3)).sum().backward()
    assert KERNELS <= set(k.names) and "k_morphable_adjoint_chunks" in k.names
    assert pose.stride() == (235, 1) and fp.shape == (B, V, 2) and angles.shape == (B, 3)
    assert float(fp.detach().min()) > 0 and float(fp.detach().max()) < 1 and float(img.detach()[..., 3].mean()) > 0.5
    g = preds.grad
    assert g.shape == (B, 235) and float(g[:, :228].abs().max()) > 0
    assert bool((g[:, [228, 229, 230, 231, 232, 233]].abs().max(0).values > 0).all()) and float(g[:, 234].abs().max()) == 0
    # face_project is the restatement's within the bound of case 2
    t64 = preds0.double()
    face64 = face.detach().cpu().double()
    fp64, ang64 = ps.image_coordinates64(face64, t64[:, 228:235], float(S), LIMIT)
    assert bool(((fp.detach().cpu().double() - fp64).abs() <= ps.uv_bound(face64, t64[:, 228:235], float(S), float(S))).all())
    assert torch.equal(angles.detach().cpu().double(), ang64)

    # grad_pose from landmarks68 against the float64 restatement
    lm_idx = torch.from_numpy(ps.landmark_indices(68, V, 2, repeats=True))
    pose_leaf = preds0[:, 228:235].clone().cuda().requires_grad_(True)
    lm = core.landmarks68(face.detach(), pose_leaf, lm_idx.cuda(), S)
    g_lm = ps.hashed_floats(B * 68, 2, 412).reshape(B, 68, 2)
    lm.backward(_dev(g_lm))
    p64 = t64[:, 228:235].clone().requires_grad_(True)
    lm64 = ps.landmarks64(face64, p64, lm_idx, float(S), LIMIT)
    lm64.backward(torch.from_numpy(g_lm).double())
    assert lm.shape == (B, 68, 2)
    assert bool(((lm.detach().cpu().double() - lm64.detach()).abs() <= ps.posed_bound(face64, t64[:, 228:235], float(S))[:, lm_idx, :2]).all())
    g3 = torch.cat([torch.from_numpy(g_lm).double(), torch.zeros(B, 68, 1, dtype=torch.float64)], 2)
    absG = ps.abs_gradient(B, V, None, lm_idx, None, None, g3)
    bp, _ = ps.gradient_bounds(face64, t64[:, 228:235], float(S), absG, po.pose_chain(V, 68), po.vertex_chain(1, 3), False, LIMIT)
    err = (pose_leaf.grad.cpu().double() - p64.grad).abs()
    print(f"landmarks68 grad_pose err/bound {float((err / bp.clamp_min(1e-300)).max()):.3f}")
    assert float(p64.grad[:, :6].abs().min()) > 0 and bool((err <= bp).all())

    # supervised_losses against its CPU float64 value
    views = 2
    gtobj = face64 + torch.from_numpy(ps.hashed_floats(B * V, 3, 413, -0.1, 0.1, np.float64)).reshape(B, V, 3)
    gtaux = torch.from_numpy(ps.hashed_floats(B * views, 152, 414, -1.0, 1.0, np.float64)).reshape(B, views, 152)
    gtaux[:, :, :136] = gtaux[:, :, :136] * 8 + 16
    pts = [face.detach(), face.detach() + 0.01]
    poses = [preds.detach()[:, 228:235], preds.detach()[:, 228:235] * 1.01]
    got = core.supervised_losses(pts, poses, gtaux.float().cuda(), gtobj.float().cuda(), lm_idx.cuda(), S)
    c64 = lambda ts: [a.cpu().double() for a in ts]          # noqa: E731
    want = ps.losses64(c64(pts), c64(poses), gtaux.float().double(), gtobj.float().double(), lm_idx, S)
    # every loss is a weighted L1 mean of n values: an f32 mean in any order is within (n + 2) u of the mean of the absolute
    # values (here the value itself), and the landmarks add the weighted mean of their own bound
    lm_slack = sum(0.02 * float(ps.posed_bound(x, p, float(S))[:, lm_idx, :2].mean()) for x, p in zip(c64(pts), c64(poses)))
    # (+ 4: the subtraction, the weight, the sum over the views, the sum of the three pose terms)
    for name, count, slack in (("ptsloss", B * V * 3, 0.0), ("poseloss", B * 3, 0.0), ("lm68loss", B * 68 * 2, lm_slack)):
        err = abs(float(got[name]) - float(want[name]))
        assert float(want[name]) > 0 and err <= (count + 4) * ps.U * float(want[name]) + slack, (name, err)
