"""The weak-perspective pose node without a device: the float64 restatement of tests/pose_scenes.py (known answers, autograd
against central differences, the clamp), every argument error of nr.pose_vertices, nr.PoseHead and core.pose_tools that needs
no device, every D3M_ERR_INVALID of the three C entry points with pointers that are never dereferenced, and
core.supervised_losses through the restatement against the losses stated from their definitions."""
import ctypes
import math

import numpy as np
import pytest
import torch

import pose_scenes as ps

F64 = torch.float64


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(F64)


def _pose(s=1.0, a=(0.0, 0.0, 0.0), t=(0.0, 0.0, 0.0)):
    return torch.tensor([[s, *a, *t]], dtype=F64)


def _small(B=3, V=5, per_set=False, salt=0):
    pts = _t(ps.hashed_floats(B * V if per_set else V, 3, 11 + salt, -2.0, 2.0, np.float64))
    pose = _t(ps.float_pose(B, 12 + salt)).clone()
    pose[:, 1:4] = _t(ps.hashed_floats(B, 3, 13 + salt, -1.5, 1.5, np.float64))      # (away from the clamp)
    return (pts.reshape(B, V, 3) if per_set else pts), pose


# ---- the restatement ------------------------------------------------------------------------------------------------------
def test_restatement_known_answers():
    pts, _ = _small()
    # zero angles: s x + tau t
    posed, uv, lm = ps.restate_node(pts, _pose(2.0, t=(1.0, -2.0, 3.0)), translation_scale=4.0)
    assert uv is None and lm is None and torch.equal(posed[0], 2.0 * pts + torch.tensor([4.0, -8.0, 12.0], dtype=F64))
    # a quarter turn about each axis moves the unit vectors where Rx Ry Rz says: Rx: y -> z, Ry: z -> x, Rz: x -> y
    eye = torch.eye(3, dtype=F64)
    q = math.pi / 2
    for axis, image in ((0, [[1, 0, 0], [0, 0, 1], [0, -1, 0]]), (1, [[0, 0, -1], [0, 1, 0], [1, 0, 0]]),
                        (2, [[0, 1, 0], [-1, 0, 0], [0, 0, 1]])):
        a = [0.0, 0.0, 0.0]
        a[axis] = q
        got = ps.restate_posed(eye, _pose(a=a))[0]      # row v = R e_v
        assert torch.allclose(got, torch.tensor(image, dtype=F64), rtol=0, atol=1e-15), axis
    # the product order: R = Rx Ry Rz applies Rz first; x -Rz-> y -Ry-> y -Rx-> z
    got = ps.restate_posed(eye[:1], _pose(a=(q, q, q)))[0, 0]
    assert torch.allclose(got, torch.tensor([0.0, 0.0, 1.0], dtype=F64), rtol=0, atol=1e-15)
    # uv flips y; landmarks are rows of posed (repeats allowed)
    pose = _pose(1.5, (0.3, -0.2, 0.1), (0.1, 0.2, 0.3))
    idx = torch.tensor([4, 0, 4])
    posed, uv, lm = ps.restate_node(pts, pose, 8.0, None, 16.0, idx)
    assert torch.equal(uv[..., 0], posed[..., 0] / 16.0) and torch.equal(uv[..., 1], 1 - posed[..., 1] / 16.0)
    assert torch.equal(lm, posed[:, [4, 0, 4]]) and lm.shape == (1, 3, 3)
    # the image coordinates and the landmark xy are outputs of the node's restatement
    fp, ang = ps.image_coordinates64(pts, pose, 16.0)
    assert torch.equal(fp, ps.restate_node(pts, pose, 16.0, ps.ANGLE_LIMIT, 16.0)[1]) and torch.equal(ang, pose[:, 1:4])
    assert torch.equal(ps.landmarks64(pts, pose, idx, 16.0), ps.restate_posed(pts, pose, 16.0, ps.ANGLE_LIMIT)[:, [4, 0, 4], :2])
    # the rotation matches core.renderer_pt3d.euler_xyz_to_matrix
    from deep3dmap_amd.core.renderer_pt3d import euler_xyz_to_matrix
    ang = _t(ps.hashed_floats(4, 3, 19, -3.0, 3.0, np.float64))
    assert torch.equal(ps.euler_xyz(ang), euler_xyz_to_matrix(ang))


@pytest.mark.parametrize("per_set", [False, True])
def test_restatement_gradient_equals_central_differences(per_set):
    B, V = 3, 5
    pts, pose = _small(B, V, per_set)
    idx = torch.tensor([1, 3, 1, 0])        # a repeated landmark
    g_posed, g_uv, g_lm = (_t(ps.hashed_floats(B * n, c, 20 + c + n, dtype=np.float64)).reshape(B, n, c)
                           for n, c in ((V, 3), (V, 2), (4, 3)))

    def value(x, p):
        posed, uv, lm = ps.restate_node(x, p, 4.0, ps.ANGLE_LIMIT, 7.0, idx)
        return (posed * g_posed).sum() + (uv * g_uv).sum() + (lm * g_lm).sum()

    x, p = pts.clone().requires_grad_(True), pose.clone().requires_grad_(True)
    value(x, p).backward()
    h = 1e-5
    for b in range(B):
        for k in range(7):
            d = torch.zeros_like(pose)
            d[b, k] = h
            fd = float(value(pts, pose + d) - value(pts, pose - d)) / (2 * h)
            assert abs(fd - float(p.grad[b, k])) <= 1e-7 * max(1.0, abs(fd)), (b, k)
    flat = pts.reshape(-1)
    for i in range(flat.numel()):
        d = torch.zeros_like(flat)
        d[i] = h
        fd = float(value((flat + d).reshape(pts.shape), pose) - value((flat - d).reshape(pts.shape), pose)) / (2 * h)
        assert abs(fd - float(x.grad.reshape(-1)[i])) <= 1e-7 * max(1.0, abs(fd)), i
    # and they are the sums the kernels form: M = sum G (x) x, n = sum G, g_x = s R^T G
    G = g_posed.clone()
    G[..., 0] += g_uv[..., 0] / 7.0
    G[..., 1] -= g_uv[..., 1] / 7.0
    G.index_add_(1, idx, g_lm)
    xb = pts if per_set else pts[None].expand(B, -1, -1)
    R = ps.euler_xyz(pose[:, 1:4])
    M = torch.einsum("bvj,bvc->bjc", G, xb)
    assert torch.allclose(p.grad[:, 0], (M * R).sum((1, 2)), rtol=0, atol=1e-12)
    assert torch.allclose(p.grad[:, 4:7], 4.0 * G.sum(1), rtol=0, atol=1e-12)
    gx = pose[:, 0].reshape(B, 1, 1) * torch.einsum("bij,bvi->bvj", R, G)
    assert torch.allclose(x.grad, gx if per_set else gx.sum(0), rtol=0, atol=1e-12)


def test_the_clamp_is_inclusive():
    pts, _ = _small(1, 5)
    limit = float(np.float32(ps.ANGLE_LIMIT))
    beyond = float(np.nextafter(np.float32(limit), np.float32(np.inf)))
    assert beyond > limit
    for sign in (1.0, -1.0):
        at = _pose(1.3, (sign * limit, 0.4, -0.3), (0.1, 0.2, 0.3)).requires_grad_(True)
        past = _pose(1.3, (sign * beyond, 0.4, -0.3), (0.1, 0.2, 0.3)).requires_grad_(True)
        w = _t(ps.hashed_floats(5, 3, 31, dtype=np.float64))
        va = ps.restate_posed(pts, at, 2.0, limit)
        vp = ps.restate_posed(pts, past, 2.0, limit)
        (va * w).sum().backward()
        (vp * w).sum().backward()
        assert torch.equal(va, vp)                                     # one float beyond: the forward uses the limit
        assert float(at.grad[0, 1]) != 0 and float(past.grad[0, 1]) == 0     # at the limit the gradient flows
        assert torch.equal(at.grad[0, 2:], past.grad[0, 2:]) and float(at.grad[0, 0]) == float(past.grad[0, 0])
        free = ps.restate_posed(pts, past.detach(), 2.0, None)
        assert not torch.equal(free, vp)


def test_bounds_follow_their_formulas():
    pts, pose = _small(2, 4)
    b = ps.posed_bound(pts, pose, 4.0)
    want = ps.C_POSED * ps.U * (abs(float(pose[1, 0])) * float(pts[2].abs().sum()) + abs(4.0 * float(pose[1, 5])))
    assert b.shape == (2, 4, 3) and abs(float(b[1, 2, 1]) - want) <= 1e-18 and ps.C_POSED == 36 and ps.C_TERM == 6 and ps.E_R == 30 * ps.U
    ub = ps.uv_bound(pts, pose, 4.0, 8.0)
    assert abs(float(ub[1, 2, 1]) - (ps.C_POSED + 2) * ps.U * (want / (ps.C_POSED * ps.U) / 8.0 + 1)) <= 1e-18
    idx = torch.tensor([3, 3])
    g = torch.ones(2, 2, 3, dtype=F64)
    G = ps.abs_gradient(2, 4, 8.0, idx, torch.ones(2, 4, 3, dtype=F64), -torch.ones(2, 4, 2, dtype=F64), -g)
    assert G[0, 3].tolist() == [1 + 1 / 8 + 2, 1 + 1 / 8 + 2, 3] and G[0, 0].tolist() == [1.125, 1.125, 1]
    bp, bv = ps.gradient_bounds(pts, pose, 4.0, G, 10, 5, shared=True)
    assert bp.shape == (2, 7) and bv.shape == (1, 4, 3)
    assert abs(float(bp[0, 4]) - (10 + ps.C_TERM) * ps.U * 4.0 * float(G[0, :, 0].sum())) <= 1e-18
    R = ps.euler_xyz(pose[:, 1:4]).abs()
    dR = [d.abs() for d in ps.euler_xyz_derivatives(pose[:, 1:4])]
    absM = torch.einsum("vj,vc->jc", G[0], pts.abs())
    want_s = (10 + 8 + ps.C_TERM) * ps.U * float((absM * R[0]).sum()) + ps.E_R * float(absM.sum())
    want_a = abs(float(pose[0, 0])) * ((10 + 8 + ps.C_TERM) * ps.U * float((absM * dR[1][0]).sum()) + ps.E_R * float(absM.sum()))
    assert abs(float(bp[0, 0]) - want_s) <= 1e-15 * want_s and abs(float(bp[0, 2]) - want_a) <= 1e-15 * want_a
    want_v = sum(abs(float(pose[b, 0])) * ((5 + ps.C_TERM) * ps.U * float((R[b, :, 0] * G[b, 3]).sum()) + ps.E_R * float(G[b, 3].sum()))
                 for b in range(2))
    assert abs(float(bv[0, 3, 0]) - want_v) <= 1e-15 * want_v
    # the derivative factors are the derivatives: central differences of the rotation
    ang = pose[:, 1:4]
    for k, d in enumerate(ps.euler_xyz_derivatives(ang)):
        e = torch.zeros_like(ang)
        e[:, k] = 1e-6
        assert torch.allclose(d, (ps.euler_xyz(ang + e) - ps.euler_xyz(ang - e)) / 2e-6, rtol=0, atol=1e-9)


# ---- argument errors that need no device -------------------------------------------------------------------------------
def test_node_argument_errors():
    from deep3dmap_amd import neural_renderer as nr
    v, p = torch.zeros(5, 3), torch.zeros(2, 7)
    idx = torch.tensor([0, 4])
    with pytest.raises(ValueError, match="vertices must be a tensor"):
        nr.pose_vertices(v.numpy(), p)
    with pytest.raises(ValueError, match="pose must be a tensor"):
        nr.pose_vertices(v, p.numpy())
    with pytest.raises(ValueError, match="vertices must be float32"):
        nr.pose_vertices(v.double(), p)
    with pytest.raises(ValueError, match="pose must be float32"):
        nr.pose_vertices(v, p.half())
    for bad in (torch.zeros(2, 6), torch.zeros(8), torch.zeros(1, 2, 7), torch.zeros(())):
        with pytest.raises(ValueError, match=r"pose must be \[7\] or \[B, 7\]"):
            nr.pose_vertices(v, bad)
    with pytest.raises(ValueError, match="poses per call"):
        nr.pose_vertices(v, torch.zeros(4097, 7))
    with pytest.raises(ValueError, match="poses per call"):
        nr.pose_vertices(v, torch.zeros(0, 7))
    for bad in (torch.zeros(5), torch.zeros(5, 2), torch.zeros(0, 3), torch.zeros(2, 2, 5, 3)):
        with pytest.raises(ValueError, match=r"vertices must be \[V, 3\] or \[B, V, 3\]"):
            nr.pose_vertices(bad, p)
    with pytest.raises(ValueError, match=r"need a pose \[B, 7\]"):
        nr.pose_vertices(torch.zeros(1, 5, 3), p[0])
    with pytest.raises(ValueError, match="vertices has 3 sets, pose 2"):
        nr.pose_vertices(torch.zeros(3, 5, 3), p)
    with pytest.raises(ValueError, match="2\\^31"):
        nr.pose_vertices(torch.zeros(1, 3).expand(2 ** 18, 3), torch.zeros(4096, 7))
    for name in ("angle_limit", "uv_size"):
        for bad in (0.0, -1.0, float("nan")):
            with pytest.raises(ValueError, match=f"{name} must be positive or None"):
                nr.pose_vertices(v, p, **{name: bad})
    with pytest.raises(ValueError, match="landmarks must be a tensor"):
        nr.pose_vertices(v, p, landmarks=[0, 1])
    for bad in (torch.tensor([0.0, 1.0]), torch.tensor([True]), torch.tensor([[0, 1]]), torch.tensor(3)):
        with pytest.raises(ValueError, match="landmarks must be an integer vector"):
            nr.pose_vertices(v, p, landmarks=bad)
    with pytest.raises(ValueError, match="1 to 1024 landmarks"):
        nr.pose_vertices(v, p, landmarks=torch.zeros(1025, dtype=torch.int64))
    with pytest.raises(ValueError, match="1 to 1024 landmarks"):
        nr.pose_vertices(v, p, landmarks=torch.zeros(0, dtype=torch.int64))
    # everything else in order: host tensors are refused (there is no CPU path), before the landmark range is looked at
    with pytest.raises(ValueError, match="vertices must be on the GPU"):
        nr.pose_vertices(v, p, 4.0, 3.1415, 8.0, torch.tensor([0, 99]))
    with pytest.raises(ValueError, match="vertices must be on the GPU"):
        nr.pose_vertices(v, p[0], posed=False, uv_size=2.0)
    assert nr.PosedPoints._fields == ("posed", "uv", "landmarks")


def test_pose_head_construction_and_errors():
    from deep3dmap_amd import neural_renderer as nr
    head = nr.PoseHead([3, 1, 3], translation_scale=224, angle_limit=3.1415, uv_size=224)
    assert dict(head.named_buffers())["landmarks"].dtype == torch.int32 and head.landmarks.tolist() == [3, 1, 3]
    assert not list(head.parameters()) and head.translation_scale == 224.0 and head.uv_size == 224.0
    src = torch.tensor([2, 0], dtype=torch.int64)
    assert nr.PoseHead(src).landmarks.data_ptr() != src.data_ptr() and nr.PoseHead(np.array([1, 2], np.int32)).landmarks.tolist() == [1, 2]
    plain = nr.PoseHead()
    assert plain.landmarks is None and plain.angle_limit is None and plain.uv_size is None and plain.translation_scale == 1.0
    with pytest.raises(ValueError, match="must not be negative"):
        nr.PoseHead([0, -1])
    with pytest.raises(ValueError, match="integer vector"):
        nr.PoseHead([0.5, 1.0])
    with pytest.raises(ValueError, match="integer vector"):
        nr.PoseHead([[0, 1]])
    with pytest.raises(ValueError, match="1 to 1024 landmarks"):
        nr.PoseHead(list(range(1025)))
    with pytest.raises(ValueError, match="1 to 1024 landmarks"):
        nr.PoseHead(torch.zeros(0, dtype=torch.int64))
    with pytest.raises(ValueError, match="int32"):
        nr.PoseHead([2 ** 31])
    with pytest.raises(ValueError, match="uv_size must be positive"):
        nr.PoseHead(uv_size=0)
    with pytest.raises(ValueError, match="angle_limit must be positive"):
        nr.PoseHead(angle_limit=-3.0)
    with pytest.raises(ValueError, match="must be on the GPU"):
        head(torch.zeros(5, 3), torch.zeros(7))


def test_pose_tools_argument_errors():
    from deep3dmap_amd import core
    v, p = torch.zeros(2, 5, 3), torch.zeros(2, 7)
    idx = torch.tensor([0, 1])
    for bad in (torch.zeros(7), torch.zeros(2, 6), [0.0] * 7):
        with pytest.raises(ValueError, match=r"face_project: pose must be \[B, 7\]"):
            core.face_project(v, bad, 224)
        with pytest.raises(ValueError, match=r"landmarks68: pose must be \[B, 7\]"):
            core.landmarks68(v, bad, idx, 224)
    with pytest.raises(ValueError, match="image_size must be positive"):
        core.face_project(v, p, 0)
    with pytest.raises(ValueError, match="must be on the GPU"):
        core.face_project(v, p, 224)
    with pytest.raises(ValueError, match="integer vector"):
        core.landmarks68(v, p, idx.float(), 224)
    with pytest.raises(ValueError, match="must be on the GPU"):
        core.landmarks68(v, p, idx, 224)
    gtaux, gtobj = torch.zeros(2, 1, 152), torch.zeros(2, 5, 3)
    with pytest.raises(ValueError, match="one entry per view"):
        core.supervised_losses([v], [p, p], gtaux, gtobj, idx, 224)
    with pytest.raises(ValueError, match="one entry per view"):
        core.supervised_losses([], [], gtaux, gtobj, idx, 224)
    with pytest.raises(ValueError, match="gtaux must be"):
        core.supervised_losses([v], [p], gtaux[:, :, :151], gtobj, idx, 224)
    with pytest.raises(ValueError, match="gtaux must be"):
        core.supervised_losses([v, v], [p, p], gtaux, gtobj, idx, 224)
    with pytest.raises(ValueError, match=r"supervised_losses: pose must be \[B, 7\]"):
        core.supervised_losses([v], [p[0]], gtaux, gtobj, idx, 224)
    with pytest.raises(ValueError, match="must be on the GPU"):
        core.supervised_losses([v], [p], gtaux, gtobj, idx, 224)


# ---- supervised_losses through the restatement ----------------------------------------------------------------------------
def test_supervised_losses_equal_their_definitions():
    from deep3dmap_amd import core
    B, V, views = 2, 90, 3
    lm_idx = torch.from_numpy(ps.landmark_indices(68, V, 1))
    gtobj = _t(ps.hashed_floats(B * V, 3, 41, -90.0, 90.0, np.float64)).reshape(B, V, 3)
    gtaux = _t(ps.hashed_floats(B * views, 152, 42, -1.0, 1.0, np.float64)).reshape(B, views, 152)
    gtaux[:, :, :136] *= 200.0
    pts, poses = [], []
    for k in range(views):
        x = gtobj + _t(ps.hashed_floats(B * V, 3, 43 + k, -5.0, 5.0, np.float64)).reshape(B, V, 3)
        x[0, 0, 0], x[1, 3, 2] = 2.0e5, -1.3e5             # beyond the reference's +-125000 clamp
        pose = _t(ps.float_pose(B, 50 + 3 * k))            # (angles beyond and at the limit among them)
        pts.append(x.requires_grad_(True))
        poses.append(pose.requires_grad_(True))
    got = core.supervised_losses(pts, poses, gtaux, gtobj, lm_idx, 224, landmarks_fn=ps.landmarks64)
    want = ps.losses64([x.detach() for x in pts], [p.detach() for p in poses], gtaux, gtobj, lm_idx, 224)
    assert set(got) == {"ptsloss", "poseloss", "lm68loss"}
    for name in got:
        assert got[name].dtype == F64 and float(want[name]) > 0
        assert abs(float(got[name].detach()) - float(want[name])) <= 1e-13 * float(want[name]), name
    # the gradient reaches points and pose, and not through a clamped point
    (got["ptsloss"] + got["poseloss"] + got["lm68loss"]).backward()
    assert float(poses[0].grad.abs().min()) >= 0 and float(poses[2].grad[:, 0].abs().min()) > 0
    assert float(pts[0].grad[0, 0, 0]) == 0 and float(pts[1].grad.abs().max()) > 0


# ---- the C entry points' refusals (nothing is launched; the pointers are never dereferenced) ------------------------------
P, ODD = 0x10000, 0x10002        # an aligned and a misaligned address


def _fwd(vertices=P, vb=2, pose=P, stride=7, tau=1.0, limit=3.0, uv_size=8.0, landmarks=P, L=4, posed=P, uv=P, lm=P, B=2, V=30):
    from deep3dmap_amd import _lib
    return _lib.lib().d3m_pose_forward(vertices, vb, pose, stride, tau, limit, uv_size, landmarks, L, posed, uv, lm, B, V, None)


def _bwd(vertices=P, vb=2, pose=P, stride=7, tau=1.0, limit=3.0, uv_size=8.0, landmarks=P, L=4, g_posed=P, g_uv=P, g_lm=P,
         scratch=P, n=None, g_v=P, g_p=P, B=2, V=30):
    from deep3dmap_amd import _lib
    lib = _lib.lib()
    n = lib.d3m_pose_scratch_floats(B, V) if n is None else n
    return lib.d3m_pose_backward(vertices, vb, pose, stride, tau, limit, uv_size, landmarks, L, g_posed, g_uv, g_lm, scratch, n,
                                 g_v, g_p, B, V, None)


SIZES = [dict(B=0, vb=0), dict(B=-1, vb=-1), dict(B=4097, vb=4097), dict(B=4097, vb=1), dict(V=0), dict(V=-5),
         dict(B=4096, vb=1, V=2 ** 18), dict(V=2 ** 31 - 1, B=1, vb=1), dict(vb=3), dict(vb=0), dict(stride=6), dict(stride=0),
         dict(L=-1), dict(L=1025), dict(landmarks=None)]


def test_forward_refusals():
    for name in ("vertices", "pose"):
        assert _fwd(**{name: None}) == 1, name
    for name in ("vertices", "pose", "landmarks", "posed", "uv", "lm"):
        assert _fwd(**{name: ODD}) == 1, name
    for sizes in SIZES:
        assert _fwd(**sizes) == 1, sizes
    assert _fwd(posed=None, uv=None, lm=None) == 1                      # nothing to compute
    assert _fwd(uv_size=0.0) == 1 and _fwd(uv_size=-2.0) == 1           # uv without its size
    assert _fwd(L=0, landmarks=None) == 1                               # landmark points without landmarks


def test_backward_refusals():
    for name in ("vertices", "pose", "scratch"):
        assert _bwd(**{name: None}) == 1, name
    for name in ("vertices", "pose", "landmarks", "g_posed", "g_uv", "g_lm", "scratch", "g_v", "g_p"):
        assert _bwd(**{name: ODD}) == 1, name
    for sizes in SIZES:
        assert _bwd(n=1 << 40, **sizes) == 1, sizes
    assert _bwd(g_v=None, g_p=None) == 1                                # nothing to compute
    assert _bwd(uv_size=0.0) == 1 and _bwd(L=0, landmarks=None) == 1
    assert _bwd(n=0) == 1 and _bwd(n=2 * 12 - 1) == 1                   # one part of 2 sets x 12 sums
    assert _bwd(V=257, n=2 * 2 * 12 - 1) == 1


def test_scratch_floats_and_the_exposed_constants():
    from deep3dmap_amd import _lib
    from deep3dmap_amd.neural_renderer import pose as po
    f = _lib.lib().d3m_pose_scratch_floats
    assert f(1, 1) == po.SUMS == 12 and f(2, 30) == 24
    assert f(1, po.VERTICES_PER_CHUNK) == 12 and f(1, po.VERTICES_PER_CHUNK + 1) == 24
    cap = po.VERTICES_PER_CHUNK * po.MAX_PARTS
    assert f(3, cap) == f(3, cap + 1) == f(3, 53215) == 3 * po.MAX_PARTS * 12
    assert f(po.MAX_SETS, 3) == po.MAX_SETS * 12
    for B, V in ((0, 5), (4097, 5), (2, 0), (4096, 2 ** 18)):
        assert f(B, V) == 0, (B, V)
    assert [po.num_parts(v) for v in (1, 256, 257, cap, cap + 1, 10 ** 6)] == [1, 1, 2, po.MAX_PARTS, po.MAX_PARTS, po.MAX_PARTS]
    # the exported constants are the library's
    c = (ctypes.c_int * 4)()
    _lib.lib().d3m_pose_tree_constants(c)
    assert list(c) == [po.VERTICES_PER_CHUNK, po.MAX_PARTS, po.FINISH_SETS, po.SUMS] and po.WAVES_PER_CHUNK * 64 == po.VERTICES_PER_CHUNK
    # a lane's vertices, the butterfly, the waves, the parts, the landmarks
    assert po.pose_chain(1) == 1 + 6 + 4 + 1 and po.pose_chain(cap + 1, 68) == 2 + 6 + 4 + po.MAX_PARTS + 68
    assert po.pose_chain(53215) == 4 + 6 + 4 + 64
    assert po.vertex_chain() == 5 and po.vertex_chain(3) == 7 and po.vertex_chain(1, 2) == 7 and po.vertex_chain(3, 2) == 15
