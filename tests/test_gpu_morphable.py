"""The linear morphable-model node on the device (neural_renderer/morphable.py, core/bfm_tools.py): forward and adjoint bit
for bit on integer inputs at every shape where the kernels take another path, one-hot inputs, float inputs against float64
within the derived bound (tests/morphable_scenes.py: bound), the reference's param2points_bfm at Basel size through the
golden file, the node's gradients, graph capture, and MultiViewFit(morphable=...) on one rank and on two."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import morphable_scenes as ms
from conftest import kernels_launched
from morphable_worker import fit_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mb():
    from deep3dmap_amd.neural_renderer import morphable as mb
    return mb


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _shapes():
    mb = _mb()
    rows = [1, mb.ROWS_PER_CHUNK - 1, mb.ROWS_PER_CHUNK, 2 * mb.ROWS_PER_CHUNK + 3]
    comps = [1, 5, 64, 65, 228, 2 * mb.COMPONENTS_PER_WORKGROUP + 1]
    sets = [1, 3, mb.SETS_PER_PASS, mb.SETS_PER_PASS + 1]
    return rows, comps, sets


def _integer_case(R, K, B):
    """basis in {-3..3}, coeffs and grad_out in {-2..2}, an integer mean: (int64 arrays, their exact forward and adjoint)"""
    basis = ms.hashed_ints(R, K, 41, -3, 3)
    coeffs = ms.hashed_ints(B, K, 42, -2, 2)
    grad = np.ascontiguousarray(ms.hashed_ints(R, B, 43, -2, 2).T)      # (the basis' own phase along the rows)
    mean = ms.hashed_ints(R, 1, 44, -4000, 4000)[:, 0]
    return basis, coeffs, grad, mean, coeffs @ basis.T + mean[None], grad @ basis


def _check_integers(R, K, B, misalign=False):
    mb = _mb()
    basis, coeffs, grad, mean, want_f, want_a = _integer_case(R, K, B)
    assert max(np.abs(want_f).max(), np.abs(want_a).max()) < 2 ** 24
    if misalign:        # the same basis 4 bytes off a 16-byte boundary
        room = torch.zeros(R * K + 1, device="cuda")
        room[1:] = _dev(basis).reshape(-1)
        d_basis = room[1:].view(R, K)
        assert d_basis.data_ptr() % 16 == 4
    else:
        d_basis = _dev(basis)
    out = torch.full((B, R), float("nan"), device="cuda")
    mb.forward(_dev(coeffs), d_basis, _dev(mean), None, out=out)
    gc = torch.full((B, K), float("nan"), device="cuda")
    mb.backward(_dev(grad), d_basis, None, out=gc)
    assert torch.equal(out.cpu().double(), torch.from_numpy(want_f).double()), ("forward", R, K, B)
    assert torch.equal(gc.cpu().double(), torch.from_numpy(want_a).double()), ("adjoint", R, K, B)
    return int(np.abs(want_f).max()), int(np.abs(want_a).max()), int(np.abs(want_f - mean[None]).max())


# ---- 1. exact integers --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 5, 64, 65, 228, 129])
def test_integer_inputs_are_exact_at_every_shape(K):
    rows, comps, sets = _shapes()
    assert K in comps
    largest = np.zeros(3, np.int64)         # forward, adjoint, forward without the mean
    with kernels_launched() as k:
        for R in rows:
            for B in sets:
                largest = np.maximum(largest, _check_integers(R, K, B))
        if K % 4 == 0:
            _check_integers(rows[-1], K, 3, misalign=True)
    assert {"k_morphable_forward", "k_morphable_adjoint_chunks", "k_morphable_adjoint_finish"} <= k.names, k.names
    # the sums are not small: the adjoint's (over up to 2 chunks + 3 rows) and the forward's with its mean exceed 1000; the
    # forward's sum alone cannot exceed 6 K (1000 only from K = 167), so it is held to a third of that ceiling
    assert largest[0] > 1000 and largest[1] > 1000 and largest[2] > 2 * K, largest


def test_integer_inputs_are_exact_at_basel_size():
    f, a, f_sum = _check_integers(ms.BFM_R, ms.BFM_K, 2)
    assert 6 * ms.BFM_R < 2 ** 24 and f > 1000 and a > 1000 and f_sum > 2 * ms.BFM_K


# ---- 2. one-hot ---------------------------------------------------------------------------------------------------------
def test_one_hot_inputs_pick_single_terms():
    mb = _mb()
    R, K, B = 2 * mb.ROWS_PER_CHUNK + 3, 228, 3
    basis = _dev(ms.hashed_floats(R, K, 51))
    scale = _dev(ms.hashed_floats(1, K, 52, 0.5, 1.5)[0])
    mean = _dev(ms.hashed_floats(R, 1, 53, -3.0, 3.0)[:, 0])
    # the adjoint of a one-hot grad_out is scale[k] * basis[r, k], bit for bit
    hot_rows = [0, R - 1, mb.ROWS_PER_CHUNK - 1, mb.ROWS_PER_CHUNK]
    for r in hot_rows:
        g = torch.zeros(B, R, device="cuda")
        g[1, r] = 1.0
        got = mb.backward(g, basis, scale)
        want = torch.zeros(B, K, device="cuda")
        want[1] = scale * basis[r]
        assert torch.equal(_bits(got), _bits(want)), r
    # a one-hot coefficient gives mean + basis[:, k] * (scale * c), the same f32 expression in torch (the kernel's fused
    # multiply-add starts from an exact 0 here, so its single rounding is the product's)
    for kk in (0, 63, 64, 227):
        c = torch.zeros(B, K, device="cuda")
        c[2, kk] = 1.7
        got = mb.forward(c, basis, mean, scale)
        want = mean[None].repeat(B, 1)
        want[2] = mean + basis[:, kk] * (scale[kk] * c[2, kk])
        assert torch.equal(_bits(got), _bits(want)), kk
        got = mb.forward(c, basis, None, None)
        want = torch.zeros(B, R, device="cuda")
        want[2] = basis[:, kk] * c[2, kk]
        assert torch.equal(_bits(got), _bits(want)), kk


# ---- 3. float inputs against float64 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,B", [(228, 3), (65, 17), (1, 1)])
def test_float_inputs_within_the_derived_bound(K, B):
    mb = _mb()
    R = 2 * mb.ROWS_PER_CHUNK + 3
    basis, coeffs = ms.hashed_floats(R, K, 61), ms.hashed_floats(B, K, 62, -2.0, 2.0)
    scale, mean = ms.hashed_floats(1, K, 63, 0.5, 1.5)[0], ms.hashed_floats(R, 1, 64, -50.0, 50.0)[:, 0]
    grad = ms.hashed_floats(B, R, 65)
    t = torch.from_numpy
    out = mb.forward(_dev(coeffs), _dev(basis), _dev(mean), _dev(scale)).cpu().double()
    gc = mb.backward(_dev(grad), _dev(basis), _dev(scale)).cpu().double()
    ref_f = ms.restate_rows(t(coeffs), t(basis), t(mean), t(scale))      # (R is not a multiple of 3 here: the C level's rows)
    ref_a = (t(grad).double() @ t(basis).double()) * t(scale).double()
    bound_f = ms.bound(K + 1, ms.abs_terms(t(coeffs), t(basis), t(mean), t(scale)))
    bound_a = ms.bound(mb.adjoint_chain(R), (t(grad).double().abs() @ t(basis).double().abs()) * t(scale).double())
    err_f, err_a = (out - ref_f).abs(), (gc - ref_a).abs()
    print(f"K={K} B={B}: forward err/bound {float((err_f / bound_f).max()):.3f}, adjoint {float((err_a / bound_a).max()):.3f}")
    assert bool((err_f <= bound_f).all()) and bool((err_a <= bound_a).all())
    assert mb.adjoint_chain(R) < R
    # <J c, g> = <c, J^T g> in float64 of the two outputs, within what the two bounds allow
    lhs = ((out - t(mean).double()) * t(grad).double()).sum()
    rhs = (t(coeffs).double() * gc).sum()
    slack = (bound_f * t(grad).double().abs()).sum() + (bound_a * t(coeffs).double().abs()).sum()
    assert abs(float(lhs - rhs)) <= float(slack) and abs(float(lhs)) > 0


# ---- 4. the golden: the reference's param2points_bfm at Basel size -------------------------------------------------------
@pytest.fixture(scope="module")
def bfm():
    sp, ep, op, preds = ms.bfm_inputs()
    return sp, ep, op, preds


def test_param2points_bfm_against_the_reference(bfm):
    from deep3dmap_amd import core
    z = np.load(os.path.join(ROOT, "tests", "golden", "bfm_golden.npz"))
    sp, ep, op, preds = bfm
    assert np.array_equal(preds.numpy(), z["preds"])
    cuda = lambda d: {k: v.cuda() for k, v in d.items()}     # noqa: E731
    d_sp, d_ep, d_op = cuda(sp), cuda(ep), cuda(op)
    with kernels_launched() as k:
        face, pose = core.param2points_bfm(d_sp, d_ep, d_op, preds.cuda())
    assert "k_morphable_forward" in k.names
    assert face.shape == (2, ms.BFM_V, 3) and torch.equal(pose.cpu(), torch.from_numpy(z["pose"]))
    # the concatenated basis is built once per (w, w_exp) pair
    from deep3dmap_amd.core import bfm_tools
    n = len(bfm_tools._bases)
    again = core.param2points_bfm(d_sp, d_ep, d_op, preds.cuda())[0]
    assert len(bfm_tools._bases) == n and torch.equal(_bits(again), _bits(face))
    idx = z["vertices"].astype(np.int64)
    rows = torch.from_numpy((idx[:, None] * 3 + np.arange(3)).reshape(-1))
    basis = torch.cat([sp['w'], ep['w_exp']], 1)[rows]
    scale = torch.cat([sp['sigma'].double(), 1.0 / (1000.0 * op['sigma_exp'].double())])
    S = ms.abs_terms(preds[:, :ms.BFM_K], basis, sp['mu_shape'].reshape(-1)[rows], scale).reshape(2, -1, 3)
    limit = ms.bound(ms.BFM_K, S)
    err = (face[:, idx].cpu().double() - torch.from_numpy(z["face64"])).abs()
    ref_err = (torch.from_numpy(z["face32"]).double() - torch.from_numpy(z["face64"])).abs()
    print(f"err/bound: node {float((err / limit).max()):.4f}, the reference's own f32 run {float((ref_err / limit).max()):.4f}")
    assert bool((ref_err <= limit).all()) and bool((err <= limit).all())


# ---- 5. node gradients --------------------------------------------------------------------------------------------------
def test_grad_scale_accumulate_and_strided_coefficients():
    from deep3dmap_amd import neural_renderer as nr
    mb = _mb()
    R, K, B = 3 * 200, 65, 3
    basis, scale = _dev(ms.hashed_floats(R, K, 71)), _dev(ms.hashed_floats(1, K, 72, 0.5, 1.5)[0])
    grad = _dev(ms.hashed_floats(B, R, 73))
    plain = mb.backward(grad, basis, scale)
    gs = _dev(np.array([2.0, -0.5, 0.0], np.float32))       # (powers of two and 0: the product is exact)
    assert torch.equal(_bits(mb.backward(grad, basis, scale, grad_scale=gs)), _bits(gs[:, None] * plain))
    start = _dev(ms.hashed_floats(B, K, 74))
    dst = start.clone()
    mb.backward(grad, basis, scale, out=dst, accumulate=True)
    assert torch.equal(_bits(dst), _bits(start + plain))
    mb.backward(grad, basis, scale, out=dst, grad_scale=gs, accumulate=True)
    assert torch.equal(_bits(dst), _bits((start + plain) + gs[:, None] * plain))
    # coefficients that are a strided view; [K] and [B,K]; basis as [V,3,K], mean as [V,3]
    wide = _dev(ms.hashed_floats(B, 2 * K, 75)).requires_grad_(True)
    mean = _dev(ms.hashed_floats(R, 1, 76)[:, 0])
    v = nr.morphable_vertices(wide[:, ::2], basis.view(R // 3, 3, K), mean.view(-1, 3), scale)
    assert v.shape == (B, R // 3, 3) and not wide[:, ::2].is_contiguous()
    v.backward(grad.view(B, -1, 3))
    assert torch.equal(_bits(v.reshape(B, R)), _bits(mb.forward(wide.detach()[:, ::2].contiguous(), basis, mean, scale)))
    assert torch.equal(_bits(wide.grad[:, ::2]), _bits(plain)) and float(wide.grad[:, 1::2].abs().max()) == 0
    one = wide.detach()[1, ::2].clone().requires_grad_(True)
    v1 = nr.morphable_vertices(one, basis, mean, scale)
    assert v1.shape == (R // 3, 3) and torch.equal(_bits(v1), _bits(v[1]))
    v1.backward(grad[1].view(-1, 3))
    assert one.grad.shape == (K,) and torch.equal(_bits(one.grad), _bits(mb.backward(grad[1:2], basis, scale)[0]))


def test_gradient_flows_through_a_render():
    from deep3dmap_amd import _lib, neural_renderer as nr, synthetic
    mb = _mb()
    v_np, tri_np = synthetic.icosphere(1)
    V, K = v_np.shape[0], 7
    basis = ms.hashed_floats(3 * V, K, 81, -0.1, 0.1)
    scale = ms.hashed_floats(1, K, 82, 0.5, 1.5)[0]
    model = nr.MorphableModel(v_np.astype(np.float32).reshape(-1), basis, scale).cuda()
    faces = torch.from_numpy(tri_np.astype(np.int32))[None].cuda()
    c = _dev(ms.hashed_floats(1, K, 83)[0]).requires_grad_(True)
    target = _dev(ms.hashed_floats(3 * 32, 32, 84, 0.0, 1.0)).view(3, 32, 32)
    r = nr.Renderer(camera_mode="look_at", image_size=32, anti_aliasing=False)
    r.eye = torch.tensor([[0.0, 0.0, -2.7], [1.6, 0.9, -2.0], [-1.9, -0.6, 1.8]]).cuda()
    with _lib.deterministic():
        verts = model(c)
        verts.retain_grad()
        sil = r.render_silhouettes(verts[None], faces)
        ((sil - target) ** 2).sum().backward()
    gv = verts.grad.reshape(-1).cpu().double()
    assert sil.shape == (3, 32, 32) and float(gv.abs().max()) > 0
    t = torch.from_numpy
    ref = (gv @ t(basis).double()) * t(scale).double()
    limit = ms.bound(mb.adjoint_chain(3 * V), (gv.abs() @ t(basis).double().abs()) * t(scale).double())
    err = (c.grad.cpu().double() - ref).abs()
    assert float(ref.abs().max()) > 0 and bool((err <= limit).all()), float((err / limit).max())


# ---- 6. capture and replay ----------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical_and_a_captured_step_equals_its_eager_twin():
    from deep3dmap_amd import neural_renderer as nr
    from deep3dmap_amd.graph import CapturedStep
    R, K = 3 * 700, 228
    model = nr.MorphableModel(ms.hashed_floats(R, 1, 91, -3.0, 3.0)[:, 0], ms.hashed_floats(R, K, 92),
                              ms.hashed_floats(1, K, 93, 0.5, 1.5)[0]).cuda()
    w = _dev(ms.hashed_floats(R, 1, 94, 0.0, 1.0)[:, 0]).view(-1, 3)
    c = _dev(ms.hashed_floats(1, K, 95)[0]).requires_grad_(True)
    twin = c.detach().clone().requires_grad_(True)

    def run(x):
        x.grad = None
        ((model(x) ** 2) * w).sum().backward()            # (a gradient that depends on the coefficients)
        return x.grad

    first = run(twin).clone()
    assert torch.equal(_bits(run(twin)), _bits(first))
    # captured from the first call: the node builds nothing and never synchronises
    cs = CapturedStep(lambda: run(c)).capture()
    for i in range(3):
        delta = _dev(ms.hashed_floats(1, K, 96 + i, -0.5, 0.5)[0])
        with torch.no_grad():
            c.add_(delta)
            twin.add_(delta)
        got = cs().clone()
        torch.cuda.synchronize()
        want = run(twin)
        assert float(want.abs().max()) > 0 and torch.equal(_bits(got), _bits(want)), i
    cs.release()


# ---- 7. MultiViewFit(morphable=...), one rank ---------------------------------------------------------------------------
def _close(got, want, what):
    scale = float(want.abs().max())
    assert scale > 0 and float((got - want).abs().max()) <= 1e-5 * scale, what


def _jt_check(gc, gv_plain, basis, scale):
    """grad_coeffs against the float64 J^T of the plain fit's vertex gradient: bound 3 plus 1e-5 of scale"""
    mb = _mb()
    t = torch.from_numpy
    g = gv_plain.reshape(-1).cpu().double()
    ref = (g @ t(basis).double()) * t(scale).double()
    limit = ms.bound(mb.adjoint_chain(g.numel()), (g.abs() @ t(basis).double().abs()) * t(scale).double()) \
        + 1e-5 * float(ref.abs().max())
    err = (gc.cpu().double() - ref).abs()
    assert float(ref.abs().max()) > 0 and bool((err <= limit).all()), float((err / limit).max())


def test_multiview_fit_with_a_morphable_model():
    from deep3dmap_amd import neural_renderer as nr, synthetic
    from deep3dmap_amd.multiview import MultiViewFit
    v, tri, cubes, eyes, basis, scale, c0 = fit_scene()
    V, F, K = v.shape[0], tri.shape[0], 7
    model = nr.MorphableModel(v.reshape(-1), basis, scale)
    fit = MultiViewFit(None, tri, cubes, eyes, image_size=64, morphable=model, coeffs=c0)
    assert fit._flat.numel() == 1 + K + 24 * F and not fit.split_exchange
    fit.set_targets_from(synthetic.perturb(v))
    with kernels_launched() as k:
        loss, gc, gt = fit.step()
    assert {"k_morphable_forward", "k_morphable_adjoint_chunks", "k_morphable_adjoint_finish"} <= k.names, k.names
    assert gc.shape == (K,) and gc.data_ptr() == fit._flat[1:].data_ptr() and gt.shape == cubes.shape
    verts = model.cuda()(_dev(c0)).detach()
    assert torch.equal(_bits(fit.vertices), _bits(verts))
    plain = MultiViewFit(verts.cpu().numpy(), tri, cubes, eyes, image_size=64)
    plain.set_targets_from(synthetic.perturb(v))
    loss_p, gv_p, gt_p = plain.step()
    torch.cuda.synchronize()
    assert abs(float(loss) - float(loss_p)) <= 1e-5 * abs(float(loss_p))
    _close(gt, gt_p, "texture gradient")
    _jt_check(gc, gv_p, basis, scale)
    # captured, then replayed after an in-place update of the coefficients: the step reads them at replay
    fit.capture_graph()
    assert fit.graph_captured
    delta = _dev(ms.hashed_floats(1, K, 35, -0.3, 0.3)[0])
    with torch.no_grad():
        fit.coeffs.add_(delta)
    for _ in range(2):
        loss, gc, gt = fit.step()
    torch.cuda.synchronize()
    fresh = MultiViewFit(None, tri, cubes, eyes, image_size=64, morphable=model, coeffs=fit.coeffs.cpu().numpy())
    fresh.set_targets_from(synthetic.perturb(v))
    loss_f, gc_f, gt_f = fresh.step()
    torch.cuda.synchronize()
    assert abs(float(loss) - float(loss_f)) <= 1e-5 * abs(float(loss_f)) and float(loss_f) != float(loss_p)
    _close(gc, gc_f, "replayed grad_coeffs")
    _close(gt, gt_f, "replayed texture gradient")
    fit.release_graph()


def test_multiview_fit_morphable_with_regularizer_and_vertex_colors():
    from deep3dmap_amd import neural_renderer as nr, synthetic
    from deep3dmap_amd.multiview import MultiViewFit
    v, tri, cubes, eyes, basis, scale, c0 = fit_scene()
    V, K = v.shape[0], 7
    colors = ms.hashed_floats(V, 3, 36, 0.0, 1.0)
    reg = dict(laplacian=0.5, edge=0.2, edge_target=0.1, normal=0.3)
    model = nr.MorphableModel(v.reshape(-1), basis, scale)
    fit = MultiViewFit(None, tri, None, eyes, image_size=64, morphable=model, coeffs=c0, vertex_colors=colors, regularizer=reg)
    assert fit._flat.numel() == 1 + K + 3 * V
    fit.set_targets_from(synthetic.perturb(v))
    loss, gc, gcol = fit.step()
    plain = MultiViewFit(fit.vertices.detach().cpu().numpy(), tri, None, eyes, image_size=64, vertex_colors=colors,
                         regularizer=reg)
    plain.set_targets_from(synthetic.perturb(v))
    loss_p, gv_p, gcol_p = plain.step()
    torch.cuda.synchronize()
    assert abs(float(loss) - float(loss_p)) <= 1e-5 * abs(float(loss_p)) and float(plain.regularizer_loss()) > 0
    _close(gcol, gcol_p, "colour gradient")
    _jt_check(gc, gv_p, basis, scale)
    eager = (float(loss), gc.clone(), gcol.clone())
    fit.capture_graph()
    for _ in range(2):
        loss, gc, gcol = fit.step()
    torch.cuda.synchronize()
    assert abs(float(loss) - eager[0]) <= 1e-5 * abs(eager[0])
    _close(gc, eager[1], "replayed grad_coeffs")
    _close(gcol, eager[2], "replayed colour gradient")
    fit.release_graph()


def test_multiview_fit_morphable_argument_errors_on_the_device():
    from deep3dmap_amd import neural_renderer as nr
    from deep3dmap_amd.multiview import MultiViewFit
    v, tri, cubes, eyes, basis, scale, c0 = fit_scene()
    model = nr.MorphableModel(v.reshape(-1), basis, scale).cuda()
    with pytest.raises(ValueError, match="either vertices, or morphable"):
        MultiViewFit(v, tri, cubes, eyes, image_size=64, morphable=model, coeffs=c0)
    with pytest.raises(ValueError, match="split_exchange"):
        MultiViewFit(None, tri, cubes, eyes, image_size=64, morphable=model, coeffs=c0, split_exchange=True)
    with pytest.raises(ValueError, match="optimise_cameras"):
        MultiViewFit(None, tri, cubes, eyes, image_size=64, morphable=model, coeffs=c0, optimise_cameras=True)
    with pytest.raises(ValueError, match="vertex_colors must be"):
        MultiViewFit(None, tri, None, eyes, image_size=64, morphable=model, coeffs=c0, vertex_colors=np.zeros((3, 3), np.float32))


# ---- 8. two ranks on one device -----------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_ranks(world, out):
    """`world` child processes of tests/morphable_worker.py (ranks of one job: they run together), each under a time
    limit; every exit status is asserted before this returns."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), WORLD_SIZE=str(world),
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, os.path.join(ROOT, "tests", "morphable_worker.py"), "--out", out]
    procs = [subprocess.Popen(cmd, env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(world)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=240)[0])
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    log = "\n".join(f"--- world {world} rank {r} (exit {p.returncode}) ---\n{o}" for r, (p, o) in enumerate(zip(procs, outs)))
    assert all(p.returncode == 0 for p in procs), log
    return [np.load(f"{out}.rank{r}.npz") for r in range(world)]


def test_two_ranks_equal_one_rank(tmp_path):
    one = _run_ranks(1, str(tmp_path / "w1"))[0]            # (finished and checked before the two ranks start)
    two = _run_ranks(2, str(tmp_path / "w2"))
    K, F = 7, one["gt"].shape[0]
    assert one["gc"].shape == (K,) and int(one["flat_numel"]) == 1 + K + 24 * F
    for r in range(2):
        assert int(two[r]["flat_numel"]) == 1 + K + 24 * F
        assert abs(float(two[r]["loss"]) - float(one["loss"])) <= 1e-5 * abs(float(one["loss"]))
        for key in ("gc", "gt"):
            a, b = two[r][key], one[key]
            assert np.abs(b).max() > 0 and np.abs(a - b).max() <= 1e-5 * np.abs(b).max(), (r, key)
