"""Mesh shape regularisers on the device (neural_renderer/mesh_regularizers.py): value and gradient of every term against
the float64 restatement of tests/test_mesh_regularizers_host.py within a bound measured on the same restatement in float32,
determinism, the raw entry point (every element written, the accumulate form, grad_scale), graph capture, and
MultiViewFit(regularizer=...) on one rank (both step forms) and on two."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import kernels_launched
from test_mesh_regularizers_host import _grid, loop_topology, regularizer_mesh, restate

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONFIGS = {"laplacian": dict(laplacian=1.0), "edge": dict(edge=1.0, edge_target=0.05), "normal": dict(normal=1.0),
           "all": dict(laplacian=0.7, edge=1.3, edge_target=0.05, normal=0.4)}
REG_KERNELS = {"k_mesh_reg_mean_chunks", "k_mesh_reg_delta", "k_mesh_reg_row_chunks", "k_mesh_reg_rows", "k_mesh_reg_finish"}
FIT_WEIGHTS = dict(laplacian=0.5, edge=1.0, edge_target=0.3, normal=0.2)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def case():
    """The test mesh, three jittered vertex sets in float32, and per configuration the restatement's value and gradient in
    float64 (the reference) and in float32 on the host (the yardstick), computed once."""
    vertices, faces, notes = regularizer_mesh()
    edges, wings = loop_topology(faces)
    gen = torch.Generator().manual_seed(11)
    x = (vertices[None] + 0.01 * torch.randn(3, *vertices.shape, generator=gen, dtype=torch.float64)).float()
    refs = {name: (restate(x, edges, wings, dtype=torch.float64, **w), restate(x, edges, wings, dtype=torch.float32, **w))
            for name, w in CONFIGS.items()}
    return dict(x=x, faces=faces, notes=notes, refs=refs, V=vertices.shape[0])


def _bound(ref64, ref32):
    """max(4 max|f32 - f64|, 64 2^-24 max|f64|): the kernel may associate differently than the float32 restatement (chunked
    rows, one pass for two terms), and a single-seed yardstick moves by small factors; the floor covers a float32 run that
    happens to land within a few dozen roundings."""
    yard = float((ref32.double() - ref64).abs().max())
    return max(4.0 * yard, 64.0 * 2.0 ** -24 * float(ref64.abs().max())), yard


# ---- 1. value and gradient ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_value_and_gradient_against_float64(case, config, batch):
    from deep3dmap_amd import neural_renderer as nr
    weights = CONFIGS[config]
    faces = case["faces"].cuda()
    # batch 1 goes in as [V,3], batch 3 as [3,V,3]
    x = (case["x"][0] if batch == 1 else case["x"]).cuda().requires_grad_(True)
    with kernels_launched() as k:
        loss = nr.mesh_regularizer(x, faces, **weights)
        loss.sum().backward()
    assert loss.shape == (() if batch == 1 else (3,)) and x.grad.shape == x.shape
    lap_kernels = {"k_mesh_reg_mean_chunks", "k_mesh_reg_delta"}
    want = REG_KERNELS if "laplacian" in weights else REG_KERNELS - lap_kernels
    assert k.names == want, k.names                         # (a term of weight 0 is not evaluated)
    # value (forward) + value and gradient (backward): 3 launches each, 2 more for the long rows
    # (the Laplacian's value alone needs no gathered row: its forward skips the row chunks)
    counts = {n: k.times[n][0] for n in want}
    assert counts == dict({n: 2 for n in want}, k_mesh_reg_row_chunks=1 if config == "laplacian" else 2), counts
    (l64, g64), (l32, g32) = case["refs"][config]
    l64, g64, l32, g32 = l64[:batch], g64[:batch], l32[:batch], g32[:batch]
    got_l, got_g = loss.detach().double().cpu().reshape(batch), x.grad.double().cpu().reshape(batch, -1, 3)
    bound_g, yard_g = _bound(g64, g32)
    bound_l, yard_l = _bound(l64, l32)
    err_g, err_l = float((got_g - g64).abs().max()), float((got_l - l64).abs().max())
    print(f"mesh_regularizer {config} B={batch}: gradient error {err_g:.3e} (f32 restatement {yard_g:.3e}, ratio "
          f"{err_g / max(yard_g, 1e-300):.2f}, of max|g| {err_g / float(g64.abs().max()):.2e}); value error {err_l:.3e} "
          f"(f32 restatement {yard_l:.3e}, of |L| {err_l / float(l64.abs().max()):.2e})")
    assert float(g64.abs().max()) > 0 and err_g <= bound_g, (err_g, bound_g)
    assert err_l <= bound_l, (err_l, bound_l)


def test_one_term_calls_and_a_mesh_without_long_rows():
    from deep3dmap_amd import neural_renderer as nr
    x64, faces = _grid(7)
    x64 = x64 + 0.1 * torch.randn(x64.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    edges, wings = loop_topology(faces)
    x, f = x64.float().cuda(), faces.int().cuda()
    for call, weights in ((lambda: nr.laplacian_loss(x, f), dict(laplacian=1.0)),
                          (lambda: nr.edge_length_loss(x, f, edge_target=0.9), dict(edge=1.0, edge_target=0.9)),
                          (lambda: nr.normal_consistency_loss(x, f), dict(normal=1.0))):
        want = float(restate(x[None], edges, wings, **weights)[0])
        assert abs(float(call()) - want) <= 1e-5 * abs(want), weights
    # value + gradient of all three terms: three launches
    xg = x.clone().requires_grad_(True)
    loss = nr.mesh_regularizer(xg, f, **CONFIGS["all"])
    with kernels_launched() as k:
        loss.backward()
    assert {n: c for n, (c, _) in k.times.items()} == {"k_mesh_reg_delta": 1, "k_mesh_reg_rows": 1, "k_mesh_reg_finish": 1}
    _, g64 = restate(x[None], edges, wings, **CONFIGS["all"])
    assert float((xg.grad.double().cpu() - g64[0]).abs().max()) <= 1e-5 * float(g64.abs().max())


def test_two_runs_give_the_same_bits(case):
    from deep3dmap_amd import neural_renderer as nr
    faces = case["faces"].cuda()
    runs = []
    for _ in range(2):
        x = case["x"].cuda().requires_grad_(True)
        loss = nr.mesh_regularizer(x, faces, **CONFIGS["all"])
        loss.sum().backward()
        runs.append((loss.detach().clone(), x.grad.clone()))
    assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])) and torch.equal(_bits(runs[0][1]), _bits(runs[1][1]))


# ---- 2. the raw entry point -----------------------------------------------------------------------------------------------
def test_entry_point_writes_every_element_accumulates_and_scales(case):
    from deep3dmap_amd.neural_renderer import mesh_regularizers as mr
    V, notes = case["V"], case["notes"]
    x = case["x"].cuda()
    T = mr.mesh_topology(case["faces"].cuda(), V)
    weights = mr._checked_weights(**CONFIGS["all"])
    nan = float("nan")
    loss, grad = mr.evaluate(x, T, weights, loss_out=torch.full((3,), nan, device="cuda"),
                             grad_out=torch.full((3, V, 3), nan, device="cuda"))
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(grad).all())
    isolated = grad[:, notes["isolated"]]
    assert torch.equal(_bits(isolated), torch.zeros_like(_bits(isolated)))
    # the value-only form: the same value, the gradient untouched
    only, none = mr.evaluate(x, T, weights, want_grad=False)
    assert none is None and torch.equal(_bits(only), _bits(loss))
    # accumulate: prefill + plain result, to one rounding per element
    gen = torch.Generator().manual_seed(5)
    pre_l, pre_g = torch.randn(3, generator=gen).cuda(), torch.randn(3, V, 3, generator=gen).cuda()
    acc_l, acc_g = mr.evaluate(x, T, weights, loss_out=pre_l.clone(), grad_out=pre_g.clone(), accumulate=True)
    for got, want in ((acc_l, pre_l.double() + loss.double()), (acc_g, pre_g.double() + grad.double())):
        assert bool(((got.double() - want).abs() <= 2.0 ** -24 * want.abs()).all())
    # grad_scale: a device factor per vertex set, one rounding per element
    scale = torch.tensor([0.37, -2.0, 1.5], device="cuda")
    _, scaled = mr.evaluate(x, T, weights, grad_scale=scale)
    want = grad.double() * scale.double()[:, None, None]
    assert bool(((scaled.double() - want).abs() <= 2.0 ** -24 * want.abs()).all())


def test_backward_with_a_device_grad_output(case):
    from deep3dmap_amd import neural_renderer as nr
    faces = case["faces"].cuda()
    x = case["x"][0].cuda().requires_grad_(True)
    nr.mesh_regularizer(x, faces, **CONFIGS["all"]).backward()
    unit = x.grad.clone()
    x.grad = None
    factor = torch.tensor(0.37, device="cuda")
    (nr.mesh_regularizer(x, faces, **CONFIGS["all"]) * factor).backward()
    want = unit.double() * factor.double()
    assert float(unit.abs().max()) > 0 and bool(((x.grad.double() - want).abs() <= 2.0 ** -24 * want.abs()).all())


# ---- 3. capture -----------------------------------------------------------------------------------------------------------
def _render_scene():
    from deep3dmap_amd import neural_renderer as nr, synthetic
    v_np, tri_np = synthetic.icosphere(1)
    gen = torch.Generator().manual_seed(2)
    tex = torch.rand(1, tri_np.shape[0], 2, 2, 2, 3, generator=gen).cuda()
    target = torch.rand(3, 3, 32, 32, generator=gen).cuda()
    r = nr.Renderer(camera_mode="look_at", image_size=32, anti_aliasing=False)
    r.eye = torch.tensor([[0.0, 0.0, -2.7], [1.6, 0.9, -2.0], [-1.9, -0.6, 1.8]]).cuda()
    return torch.as_tensor(v_np, dtype=torch.float32), torch.from_numpy(tri_np), tex, target, r


def test_captured_step_over_the_module_and_a_render():
    from deep3dmap_amd import _lib, neural_renderer as nr
    from deep3dmap_amd.graph import CapturedStep
    v0, tri, tex, target, r = _render_scene()
    reg, twin_reg = (nr.MeshRegularizer(tri, **FIT_WEIGHTS).cuda() for _ in range(2))
    v, twin_v = (v0.clone().cuda().requires_grad_(True) for _ in range(2))
    tri_r = tri[None].int().cuda()
    out = {}

    def run(module, x, key):
        x.grad = None
        prior = module(x)
        rgb = r.render(x[None], tri_r, tex)[0]
        (((rgb - target) ** 2).mean() + prior).backward()
        out[key] = prior.detach()
        return x.grad

    gen = torch.Generator().manual_seed(9)
    with _lib.deterministic():
        cs = CapturedStep(lambda: run(reg, v, "captured")).capture()
        for i in range(3):
            delta = 0.02 * (torch.rand(v0.shape, generator=gen).cuda() - 0.5)
            with torch.no_grad():
                v.add_(delta)
                twin_v.add_(delta)
            got = cs().clone()
            torch.cuda.synchronize()
            prior = out["captured"].clone()
            want = run(twin_reg, twin_v, "eager")
            torch.cuda.synchronize()
            assert float(out["eager"]) > 0 and torch.equal(_bits(prior), _bits(out["eager"])), i
            assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max()), i
        cs.release()
    assert len(reg._topology) == 1


def test_first_call_inside_a_capture_raises_and_launches_nothing():
    from deep3dmap_amd import neural_renderer as nr
    from deep3dmap_amd.graph import CapturedStep
    v0, tri, *_ = _render_scene()
    reg = nr.MeshRegularizer(tri, **FIT_WEIGHTS).cuda()
    v = v0.cuda()
    torch.cuda.synchronize()
    with kernels_launched() as k:
        with pytest.raises(RuntimeError, match="topology.*capture"):
            CapturedStep(lambda: reg(v)).capture(warmup=0)
    assert not k.names, k.names
    assert len(reg._topology) == 0
    assert reg(v).shape == ()                               # eager: builds it


# ---- 4. MultiViewFit(regularizer=...), one rank ---------------------------------------------------------------------------
def fit_scene():
    from deep3dmap_amd import synthetic
    v, tri = synthetic.icosphere(1)
    textures = np.random.default_rng(3).random((tri.shape[0], 2, 2, 2, 3), dtype=np.float32)
    return v, tri, textures, synthetic.camera_ring(4)


def _close(got, want):
    return float((got - want).abs().max()) <= 1e-5 * float(want.abs().max())


def _check_fit_against_twin(split):
    from deep3dmap_amd import neural_renderer as nr, synthetic
    from deep3dmap_amd.multiview import MultiViewFit
    v, tri, textures, eyes = fit_scene()
    fit = MultiViewFit(v, tri, textures, eyes, image_size=64, regularizer=FIT_WEIGHTS)
    twin = MultiViewFit(v, tri, textures, eyes, image_size=64)
    assert fit.split_exchange == twin.split_exchange == split
    for f in (fit, twin):
        f.set_targets_from(synthetic.perturb(v))
    x = torch.as_tensor(v, dtype=torch.float32).cuda().requires_grad_(True)
    prior = nr.mesh_regularizer(x, torch.from_numpy(tri).cuda(), **FIT_WEIGHTS)
    prior.backward()
    loss_t, gv_t, gt_t = twin.step()
    torch.cuda.synchronize()
    want_loss, want_gv, want_gt = float(loss_t) + float(prior), gv_t + x.grad, gt_t.clone()
    # the prior is a visible part of both
    assert float(prior) > 1e-3 * abs(want_loss) and float(x.grad.abs().max()) > 1e-3 * float(want_gv.abs().max())
    assert torch.equal(_bits(fit.regularizer_loss()), _bits(prior)) and twin.regularizer_loss() is None

    def check(step):
        assert len(step) == 3
        loss, gv, gt = step
        torch.cuda.synchronize()
        assert abs(float(loss) - want_loss) <= 1e-5 * abs(want_loss)
        assert gv.data_ptr() == fit._flat[1:].data_ptr() and _close(gv, want_gv) and _close(gt, want_gt)
    check(fit.step())
    fit.capture_graph()
    assert fit.graph_captured and len(fit._reg_cache) == 1
    for _ in range(2):
        check(fit.step())
    fit.release_graph()


def test_multiview_fit_with_a_regularizer():
    _check_fit_against_twin(split=False)


def test_multiview_fit_with_a_regularizer_split_exchange(monkeypatch):
    """The step in two parts, reached on one rank through the debug switches (collectives issued in a group of one; without
    a process group they do nothing): the prior is added at the end of the geometry side."""
    from deep3dmap_amd import multiview
    monkeypatch.setattr(multiview, "COLLECTIVES_WITH_ONE_RANK", True)
    monkeypatch.setenv("D3M_SPLIT_EXCHANGE", "force")
    _check_fit_against_twin(split=True)


def test_multiview_fit_regularizer_forms_and_determinism():
    from deep3dmap_amd import _lib, neural_renderer as nr, synthetic
    from deep3dmap_amd.multiview import MultiViewFit
    v, tri, textures, eyes = fit_scene()
    with pytest.raises(ValueError, match="no weight"):
        MultiViewFit(v, tri, textures, eyes, image_size=64, regularizer=dict(laplace=1.0))
    with pytest.raises(ValueError, match=">= 0"):
        MultiViewFit(v, tri, textures, eyes, image_size=64, regularizer=dict(edge=-1.0))
    with pytest.raises(ValueError, match="triangles"):
        MultiViewFit(v, tri, textures, eyes, image_size=64, regularizer=nr.MeshRegularizer(torch.from_numpy(tri[:-1])))
    with _lib.deterministic():
        fit = MultiViewFit(v, tri, textures, eyes, image_size=64,
                           regularizer=nr.MeshRegularizer(torch.from_numpy(tri), **FIT_WEIGHTS))
        assert fit._reg_weights == (0.5, 1.0, 0.3, 0.2)
        fit.set_targets_from(synthetic.perturb(v))
        steps = []
        for _ in range(3):
            loss, gv, gt = fit.step()
            steps.append((loss.clone(), gv.clone(), gt.clone()))
        torch.cuda.synchronize()
    for other in steps[1:]:
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(steps[0], other))


# ---- 5. two ranks on one device -------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_ranks(world, out):
    """`world` child processes of tests/mesh_regularizer_worker.py (ranks of one job: they run together), each under a
    time limit; every exit status is asserted before this returns."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), WORLD_SIZE=str(world),
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, os.path.join(ROOT, "tests", "mesh_regularizer_worker.py"), "--out", out]
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
    assert float(one["prior"]) > 1e-3 * abs(float(one["loss"]))
    for r in range(2):
        assert abs(float(two[r]["loss"]) - float(one["loss"])) <= 1e-5 * abs(float(one["loss"]))
        a, b = two[r]["gv"], one["gv"]
        assert np.abs(b).max() > 0 and np.abs(a - b).max() <= 1e-5 * np.abs(b).max(), r
        assert bool(two[r]["launched_regularizer"]) == (r == 0)
