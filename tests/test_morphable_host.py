"""The linear morphable-model node without a device: the float64 restatements of tests/morphable_scenes.py (known answers,
autograd against central differences, the reference's own param2points_bfm where its checkout exists), every argument error
of nr.morphable_vertices, nr.MorphableModel, core.param2points_bfm and MultiViewFit(morphable=...) that needs no device, and
every D3M_ERR_INVALID of the C entry points with pointers that are never dereferenced."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import morphable_scenes as ms

REF = "/root/reference/deep3dmap/core/all3dmm/bfm_tools.py"


def _small(R=12, K=5, B=3, dtype=torch.float64):
    t = lambda a: torch.from_numpy(a).to(dtype)     # noqa: E731
    return (t(ms.hashed_floats(B, K, 11, dtype=np.float64)), t(ms.hashed_floats(R, K, 12, dtype=np.float64)),
            t(ms.hashed_floats(R, 1, 13, -3.0, 3.0, np.float64)[:, 0]), t(ms.hashed_floats(1, K, 14, 0.5, 2.0, np.float64)[0]))


# ---- the restatements ---------------------------------------------------------------------------------------------------
def test_restatement_known_answers():
    coeffs, basis, mean, scale = _small()
    # K = 1: every vertex moves along one direction
    one = ms.restate_node(torch.tensor([[2.0]], dtype=torch.float64), basis[:, :1], mean, torch.tensor([3.0], dtype=torch.float64))
    assert torch.equal(one, (mean + 6.0 * basis[:, 0]).reshape(1, 4, 3))
    # zero coefficients give the mean
    assert torch.equal(ms.restate_node(torch.zeros_like(coeffs), basis, mean, scale), mean.reshape(1, 4, 3).expand(3, 4, 3))
    # scale=None is scale = 1, mean=None is mean = 0
    assert torch.equal(ms.restate_node(coeffs, basis, mean), ms.restate_node(coeffs, basis, mean, torch.ones(5, dtype=torch.float64)))
    assert torch.equal(ms.restate_node(coeffs, basis), ms.restate_node(coeffs, basis, torch.zeros(12, dtype=torch.float64)))
    # element by element
    want = torch.zeros(3, 12, dtype=torch.float64)
    for b in range(3):
        for r in range(12):
            want[b, r] = mean[r] + sum(basis[r, k] * (scale[k] * coeffs[b, k]) for k in range(5))
    assert torch.allclose(ms.restate_node(coeffs, basis, mean, scale).reshape(3, 12), want, rtol=0, atol=1e-14)
    # [K] -> [V,3]
    assert ms.restate_node(coeffs[0], basis, mean, scale).shape == (4, 3)
    # the sum of absolute terms bounds the value
    assert bool((ms.abs_terms(coeffs, basis, mean, scale) >= want.abs() - 1e-14).all())


def test_restatement_gradient_equals_central_differences():
    coeffs, basis, mean, scale = _small()
    g = torch.from_numpy(ms.hashed_floats(3, 12, 15, dtype=np.float64)).reshape(3, 4, 3)
    c = coeffs.clone().requires_grad_(True)
    (ms.restate_node(c, basis, mean, scale) * g).sum().backward()
    h = 1e-3
    for b in range(3):
        for k in range(5):
            d = torch.zeros_like(coeffs)
            d[b, k] = h
            fd = ((ms.restate_node(coeffs + d, basis, mean, scale) - ms.restate_node(coeffs - d, basis, mean, scale)) * g).sum() / (2 * h)
            assert abs(float(fd) - float(c.grad[b, k])) <= 1e-9 * max(1.0, abs(float(fd)))
    # and it is J^T g
    want = (g.reshape(3, 12) @ basis) * scale
    assert torch.allclose(c.grad, want, rtol=0, atol=1e-13)


def test_param2points_restatement_is_the_node_restatement():
    t = lambda a: torch.from_numpy(a)       # noqa: E731
    R = 30
    sp = {'w': t(ms.hashed_floats(R, 199, 1, dtype=np.float64)), 'sigma': t(ms.hashed_floats(1, 199, 2, 0.5, 1.5, np.float64)[0]),
          'mu_shape': t(ms.hashed_floats(R, 1, 3, -9.0, 9.0, np.float64))}
    ep = {'w_exp': t(ms.hashed_floats(R, 29, 4, dtype=np.float64))}
    op = {'sigma_exp': t(ms.hashed_floats(1, 29, 5, 0.0005, 0.0015, np.float64)[0])}
    preds = t(ms.hashed_floats(2, 235, 6, -2.0, 2.0, np.float64))
    face, pose = ms.restate_param2points(sp, ep, op, preds)
    assert face.shape == (2, 10, 3) and torch.equal(pose, preds[:, 228:235])
    node = ms.restate_node(preds[:, :228], torch.cat([sp['w'], ep['w_exp']], 1), sp['mu_shape'],
                           torch.cat([sp['sigma'], 1.0 / (1000.0 * op['sigma_exp'])]))
    assert torch.allclose(face, node, rtol=0, atol=1e-11 * float(face.abs().max()))


@pytest.mark.skipif(not os.path.exists(REF), reason="the reference checkout is not on this machine")
def test_restatement_equals_the_reference_at_basel_size():
    spec = importlib.util.spec_from_file_location("ref_bfm_tools", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    sp, ep, op, preds = ms.bfm_inputs(torch.float64)
    face, pose = mod.param2points_bfm(sp, ep, op, preds)
    mine, mine_pose = ms.restate_param2points(sp, ep, op, preds)
    assert face.shape == (2, ms.BFM_V, 3) and face.dtype == torch.float64
    assert torch.equal(mine, face) and torch.equal(mine_pose, pose)


def test_the_golden_file_matches_its_description():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bfm_golden.npz")
    assert os.path.getsize(path) < 160 * 1024       # (2 x 2048 x 3 float64 values alone are 96 KiB)
    z = np.load(path)
    assert z["preds"].shape == (2, 235) and z["vertices"].shape == (2048,) and z["pose"].shape == (2, 7)
    assert z["face64"].shape == z["face32"].shape == (2, 2048, 3) and z["face64"].dtype == np.float64
    assert np.array_equal(z["vertices"], ms.bfm_sample_vertices()) and np.array_equal(z["pose"], z["preds"][:, 228:235])
    assert np.array_equal(z["preds"], ms.hashed_floats(2, 235, 6, -2.0, 2.0))


# ---- argument errors that need no device -------------------------------------------------------------------------------
def test_node_argument_errors():
    from deep3dmap_amd import neural_renderer as nr
    coeffs, basis, mean, scale = _small(dtype=torch.float32)
    with pytest.raises(ValueError, match="tensor"):
        nr.morphable_vertices(coeffs.numpy(), basis)
    with pytest.raises(ValueError, match="float32"):
        nr.morphable_vertices(coeffs.double(), basis)
    with pytest.raises(ValueError, match="float32"):
        nr.morphable_vertices(coeffs, basis.half())
    with pytest.raises(ValueError, match="float32"):
        nr.morphable_vertices(coeffs, basis, mean.double())
    with pytest.raises(ValueError, match="float32"):
        nr.morphable_vertices(coeffs, basis, mean, scale.long())
    with pytest.raises(ValueError, match=r"coeffs must be \[K\]"):
        nr.morphable_vertices(coeffs[None], basis)
    with pytest.raises(ValueError, match="basis must be"):
        nr.morphable_vertices(coeffs, basis.reshape(-1))
    with pytest.raises(ValueError, match="basis must be"):
        nr.morphable_vertices(coeffs, basis.reshape(2, 6, 5))
    with pytest.raises(ValueError, match="3 per vertex"):
        nr.morphable_vertices(coeffs, basis[:11])
    with pytest.raises(ValueError, match="components"):
        nr.morphable_vertices(coeffs[:, :4], basis)
    with pytest.raises(ValueError, match="1 to 1024 components"):
        nr.morphable_vertices(torch.zeros(1025), torch.zeros(3, 1025))
    with pytest.raises(ValueError, match="coefficient sets"):
        nr.morphable_vertices(torch.zeros(4097, 5), basis)
    with pytest.raises(ValueError, match="mean must be"):
        nr.morphable_vertices(coeffs, basis, mean[:-1])
    with pytest.raises(ValueError, match="mean must be"):
        nr.morphable_vertices(coeffs, basis, mean.reshape(3, 4))
    with pytest.raises(ValueError, match="scale must be"):
        nr.morphable_vertices(coeffs, basis, mean, scale[:-1])
    for name in ("basis", "mean", "scale"):
        args = dict(basis=basis, mean=mean, scale=scale)
        args[name] = args[name].clone().requires_grad_(True)
        with pytest.raises(NotImplementedError, match=name):
            nr.morphable_vertices(coeffs, **args)
    # everything else in order: host tensors are refused (there is no CPU path)
    with pytest.raises(ValueError, match="must be on the GPU"):
        nr.morphable_vertices(coeffs, basis, mean, scale)
    with pytest.raises(ValueError, match="must be on the GPU"):
        nr.morphable_vertices(coeffs[0], basis.reshape(4, 3, 5), mean.reshape(4, 3))


def test_model_construction_and_errors():
    from deep3dmap_amd import neural_renderer as nr
    coeffs, basis, mean, scale = _small(dtype=torch.float32)
    m = nr.MorphableModel(mean, basis, scale)
    assert m.num_components == 5 and m.num_vertices == 4
    assert set(dict(m.named_buffers())) == {"mean", "basis", "scale"} and not list(m.parameters())
    assert torch.equal(m.basis, basis) and m.basis.data_ptr() != basis.data_ptr()
    # several bases are concatenated along K once, at construction; [V,3,K] and numpy are taken
    two = nr.MorphableModel(mean.reshape(4, 3).numpy(), [basis[:, :2].reshape(4, 3, 2), basis[:, 2:].numpy()], [scale[:2], scale[2:]])
    assert torch.equal(two.basis, basis) and torch.equal(two.scale, scale) and torch.equal(two.mean, mean)
    assert nr.MorphableModel(mean, basis).scale is None
    with pytest.raises(ValueError, match="same V"):
        nr.MorphableModel(mean, [basis, basis[:9]])
    with pytest.raises(ValueError, match="3 per vertex"):
        nr.MorphableModel(mean[:11], basis[:11])
    with pytest.raises(ValueError, match="mean must hold"):
        nr.MorphableModel(mean[:9], basis)
    with pytest.raises(ValueError, match="scale must hold"):
        nr.MorphableModel(mean, basis, scale[:4])
    with pytest.raises(ValueError, match="components"):
        nr.MorphableModel(torch.zeros(3), torch.zeros(3, 1025))
    with pytest.raises(ValueError, match="must be on the GPU"):
        m(coeffs)


def test_param2points_bfm_argument_errors():
    from deep3dmap_amd import core
    sp = {'w': torch.zeros(12, 199), 'sigma': torch.ones(199), 'mu_shape': torch.zeros(12, 1)}
    ep = {'w_exp': torch.zeros(12, 29)}
    op = {'sigma_exp': torch.ones(29)}
    with pytest.raises(ValueError, match="same rows"):
        core.param2points_bfm(sp, {'w_exp': torch.zeros(9, 29)}, op, torch.zeros(2, 235))
    with pytest.raises(ValueError, match="preds must be"):
        core.param2points_bfm(sp, ep, op, torch.zeros(2, 200))
    with pytest.raises(ValueError, match="preds must be"):
        core.param2points_bfm(sp, ep, op, torch.zeros(235))
    with pytest.raises(ValueError, match="float32"):
        core.param2points_bfm(sp, ep, op, torch.zeros(2, 235, dtype=torch.float64))
    with pytest.raises(ValueError, match="must be on the GPU"):
        core.param2points_bfm(sp, ep, op, torch.zeros(2, 235))
    with pytest.raises(KeyError):
        core.param2points_bfm(sp, ep, {}, torch.zeros(2, 235))
    # a model tensor that requires grad: refused, never silently detached
    for d, key in ((sp, 'w'), (sp, 'sigma'), (sp, 'mu_shape'), (ep, 'w_exp'), (op, 'sigma_exp')):
        learn = dict(d, **{key: d[key].clone().requires_grad_(True)})
        args = [learn if x is d else x for x in (sp, ep, op)]
        with pytest.raises(NotImplementedError, match=key):
            core.param2points_bfm(*args, torch.zeros(2, 235))


def test_multiview_fit_morphable_argument_errors():
    from deep3dmap_amd import neural_renderer as nr, synthetic
    from deep3dmap_amd.multiview import MultiViewFit
    v, tri = synthetic.grid_mesh(3)
    V, F = v.shape[0], tri.shape[0]
    model = nr.MorphableModel(v.reshape(-1), ms.hashed_floats(3 * V, 4, 21))
    cubes = np.zeros((F, 2, 2, 2, 3), np.float32)
    eyes = synthetic.camera_ring(4)
    c0 = np.zeros(4, np.float32)
    with pytest.raises(ValueError, match="either vertices, or morphable"):
        MultiViewFit(v, tri, cubes, eyes, image_size=64, morphable=model, coeffs=c0)
    with pytest.raises(ValueError, match="either vertices, or morphable"):
        MultiViewFit(None, tri, cubes, eyes, image_size=64, morphable=model)
    with pytest.raises(ValueError, match="either vertices, or morphable"):
        MultiViewFit(None, tri, cubes, eyes, image_size=64, coeffs=c0)
    with pytest.raises(ValueError, match="either vertices, or morphable"):
        MultiViewFit(v, tri, cubes, eyes, image_size=64, coeffs=c0)
    with pytest.raises(ValueError, match="either vertices, or morphable"):
        MultiViewFit(None, tri, cubes, eyes, image_size=64)
    with pytest.raises(ValueError, match="split_exchange"):
        MultiViewFit(None, tri, cubes, eyes, image_size=64, morphable=model, coeffs=c0, split_exchange=True)
    with pytest.raises(ValueError, match="optimise_cameras"):
        MultiViewFit(None, tri, cubes, eyes, image_size=64, morphable=model, coeffs=c0, optimise_cameras=True)
    with pytest.raises(ValueError, match=r"coeffs must be \[4\]"):
        MultiViewFit(None, tri, cubes, eyes, image_size=64, morphable=model, coeffs=np.zeros(5, np.float32))
    with pytest.raises(ValueError, match=r"coeffs must be \[4\]"):
        MultiViewFit(None, tri, cubes, eyes, image_size=64, morphable=model, coeffs=np.zeros((1, 4), np.float32))


# ---- the C entry points' refusals (nothing is launched; the pointers are never dereferenced) ------------------------------
P, ODD = 0x10000, 0x10002        # an aligned and a misaligned address


def _fwd(basis=P, coeffs=P, mean=P, scale=P, out=P, B=2, R=30, K=5):
    from deep3dmap_amd import _lib
    return _lib.lib().d3m_morphable_forward(basis, coeffs, mean, scale, out, B, R, K, None)


def _bwd(basis=P, grad_out=P, scale=P, grad_scale=P, scratch=P, n=None, grad_coeffs=P, B=2, R=30, K=5, accumulate=0):
    from deep3dmap_amd import _lib
    L = _lib.lib()
    n = L.d3m_morphable_scratch_floats(B, R, K) if n is None else n
    return L.d3m_morphable_backward(basis, grad_out, scale, grad_scale, scratch, n, grad_coeffs, B, R, K, accumulate, None)


SIZES = [dict(B=0), dict(B=-1), dict(B=4097), dict(K=0), dict(K=1025), dict(R=0), dict(R=-3),
         dict(R=2 ** 21, K=1024), dict(R=2 ** 31 - 1, K=2)]


def test_forward_refusals():
    for name in ("basis", "coeffs", "out"):
        assert _fwd(**{name: None}) == 1, name
    for name in ("basis", "coeffs", "mean", "scale", "out"):
        assert _fwd(**{name: ODD}) == 1, name
    for sizes in SIZES:
        assert _fwd(**sizes) == 1, sizes


def test_backward_refusals():
    for name in ("basis", "grad_out", "scratch", "grad_coeffs"):
        assert _bwd(**{name: None}) == 1, name
    for name in ("basis", "grad_out", "scale", "grad_scale", "scratch", "grad_coeffs"):
        assert _bwd(**{name: ODD}) == 1, name
    assert _bwd(scratch=P + 4) == 1             # scratch: 16-byte aligned
    for sizes in SIZES:
        assert _bwd(n=1 << 40, **sizes) == 1, sizes
    assert _bwd(n=0) == 1 and _bwd(n=2 * 5 - 1) == 1        # one chunk of 2 sets x 5 components: 10 floats
    assert _bwd(R=257, n=2 * 2 * 5 - 1) == 1


def test_scratch_floats_and_the_exposed_constants():
    from deep3dmap_amd import _lib
    from deep3dmap_amd.neural_renderer import morphable as mb
    f = _lib.lib().d3m_morphable_scratch_floats
    assert f(1, 1, 1) == 1 and f(2, 30, 5) == 10
    # one partial per (chunk of ROWS_PER_CHUNK rows, set, component)
    assert f(1, mb.ROWS_PER_CHUNK, 1) == 1 and f(1, mb.ROWS_PER_CHUNK + 1, 1) == 2
    assert f(3, 2 * mb.ROWS_PER_CHUNK + 3, 7) == 3 * 3 * 7
    assert f(2, ms.BFM_R, ms.BFM_K) == mb.num_chunks(ms.BFM_R) * 2 * ms.BFM_K == 624 * 2 * 228
    assert f(mb.MAX_SETS, 3, mb.MAX_COMPONENTS) == mb.MAX_SETS * mb.MAX_COMPONENTS
    for sizes in SIZES:
        args = dict(B=2, R=30, K=5)
        args.update(sizes)
        assert f(args["B"], args["R"], args["K"]) == 0, sizes
    assert mb.ROWS_PER_CHUNK == mb.ROWS_PER_WAVE * mb.WAVES_PER_CHUNK and mb.SETS_PER_PASS == 16
    assert mb.adjoint_chain(1) == 1 + 4 + 1 + 16 and mb.adjoint_chain(ms.BFM_R) == 64 + 4 + 39 + 16
    assert mb.forward_chain(228) == 16 * 4 + 5
