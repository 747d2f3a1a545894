"""Learnable per-vertex colours on the device (neural_renderer/vertex_colors.py): the forward bit for bit against
get_textures_from_im on a grid mesh and against the element-wise restatement on an irregular mesh with hubs, the fixed-order
adjoint against float64 within the derived bound (tests/test_vertex_colors_host.py: adjoint_bound), determinism, the chain
through a render, graph capture, and MultiViewFit(vertex_colors=...) on one rank and on two."""
import ctypes
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import kernels_launched
from test_vertex_colors_host import adjoint64, adjoint_bound, image_grid_faces, irregular_mesh, restate_cubes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _within_bound(got, ref, mag, valence):
    err = (got.detach().double().cpu() - ref).abs()
    bound = adjoint_bound(mag, valence)
    assert bool((err <= bound).all()), float((err - bound).max())


# ---- 1. grid parity, forward --------------------------------------------------------------------------------------------
def test_forward_equals_get_textures_from_im_on_the_grid_mesh():
    from deep3dmap_amd import neural_renderer as nr
    from deep3dmap_amd.core.renderer_utils import get_textures_from_im
    h, w = 5, 7
    im = torch.rand(2, 3, h, w, generator=torch.Generator().manual_seed(1)).cuda()
    colors = im.permute(0, 2, 3, 1).reshape(2, h * w, 3).contiguous()
    faces = image_grid_faces(h, w).cuda()
    got = nr.textures_from_vertex_colors(colors, faces)
    want = get_textures_from_im(im, 2)
    assert got.shape == want.shape == (2, 2 * (h - 1) * (w - 1), 2, 2, 2, 3)
    assert torch.equal(_bits(got), _bits(want))
    one = nr.textures_from_vertex_colors(colors[1].contiguous(), faces[None].int().contiguous())
    assert one.shape == (1,) + want.shape[1:] and torch.equal(_bits(one[0]), _bits(want[1]))


# ---- 2. irregular mesh --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def irregular():
    """The mesh, colours and two cube gradients (random; integers in [-8, 8]) with their float64 adjoints, computed once."""
    faces, V, notes = irregular_mesh()
    F = faces.shape[0]
    gen = torch.Generator().manual_seed(7)
    colors = torch.randn(3, V, 3, generator=gen)
    g = torch.randn(3, F, 2, 2, 2, 3, generator=gen)
    g_int = torch.randint(-8, 9, (3, F, 2, 2, 2, 3), generator=gen).float()
    return dict(faces=faces, V=V, notes=notes, colors=colors, g=g, g_int=g_int, cubes=restate_cubes(colors, faces),
                ref=adjoint64(g, faces, V), ref_int=adjoint64(g_int, faces, V))


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_irregular_mesh_forward_and_adjoint(irregular, batch, dtype):
    from deep3dmap_amd import _lib, neural_renderer as nr
    from deep3dmap_amd.neural_renderer import vertex_colors as vc
    c = irregular
    V, notes = c["V"], c["notes"]
    faces = c["faces"].to(dtype).cuda()
    # batch 1 goes in as [V,3], batch 3 as [3,V,3]
    colors = (c["colors"][0] if batch == 1 else c["colors"]).cuda().requires_grad_(True)
    g, g_int = c["g"][:batch].cuda(), c["g_int"][:batch].cuda()
    with kernels_launched() as k:
        out = nr.textures_from_vertex_colors(colors, faces)
        out.backward(g)
    assert {"k_vertex_color_textures", "k_vertex_color_adjoint_chunks", "k_vertex_color_adjoint_rows"} <= k.names, k.names
    assert out.shape == (batch, faces.shape[0], 2, 2, 2, 3)
    assert torch.equal(_bits(out).cpu(), _bits(c["cubes"][:batch]))
    got = colors.grad.reshape(batch, V, 3).clone()
    ref, mag, valence = c["ref"]
    assert {int(valence[h]) for h in notes["hubs"]} == {vc.LONG_ROW, vc.LONG_ROW + 1, 2 * vc.CHUNK + 1}
    _within_bound(got, ref[:batch], mag[:batch], valence)
    # two runs: the same bits
    colors.grad = None
    nr.textures_from_vertex_colors(colors, faces).backward(g)
    assert torch.equal(_bits(colors.grad.reshape(batch, V, 3)), _bits(got))
    # integer gradients: every partial sum is a multiple of 1/2 far below 2^23, so ANY order gives the exact sum
    colors.grad = None
    nr.textures_from_vertex_colors(colors, faces).backward(g_int)
    got_int = colors.grad.reshape(batch, V, 3)
    assert torch.equal(got_int.double().cpu(), c["ref_int"][0][:batch])
    # the C entry point, raw, on a NaN-filled output: every element is written, the unused vertex gets an exact 0
    A = vc.vertex_adjacency(faces, V)
    raw = torch.full((batch, V, 3), float("nan"), device="cuda")
    partials = torch.full((batch, A.csr.num_chunks, 3), float("nan"), device="cuda")
    _lib.check(_lib.lib().d3m_vertex_color_textures_backward(
        _lib.ptr(g_int), ctypes.byref(A.csr.c), _lib.ptr(partials), _lib.ptr(raw), batch, V, faces.shape[0],
        _lib.stream_ptr()), "d3m_vertex_color_textures_backward")
    assert torch.equal(_bits(raw), _bits(got_int))
    unused = raw[:, notes["unused"]]
    assert torch.equal(_bits(unused), torch.zeros_like(_bits(unused)))


def test_adjoint_has_the_bits_of_the_shared_order(irregular):
    """grad_colors bit for bit against the numpy replay of the order csrc/d3m_row_gather.h states (tests/
    row_gather_replay.py): the rows of LONG_ROW items (the short path), LONG_ROW + 1 (one chunk) and 2 CHUNK + 1 (three
    chunks, the last of one item) are where a moved addition shows.  An item's term is t = 0; t += C[idx][c] g[f, idx, k]
    for idx ascending, in float32 (the products are exact)."""
    from deep3dmap_amd.core.renderer_utils import _CUBE
    from deep3dmap_amd.neural_renderer import vertex_colors as vc
    from row_gather_replay import replay_gather
    c = irregular
    V, B = c["V"], 3
    A = vc.vertex_adjacency(c["faces"].cuda(), V)
    got = vc.vertex_color_adjoint(A, c["g"].cuda())
    counts = (A.csr.offsets[1:] - A.csr.offsets[:-1]).cpu()
    assert {int(counts[h]) for h in c["notes"]["hubs"]} == {vc.LONG_ROW, vc.LONG_ROW + 1, 2 * vc.CHUNK + 1}
    assert A.csr.long_rows.shape[0] == 2 and A.csr.chunks.shape[0] == 4
    items = A.csr.items.cpu().numpy()
    f, corner = items // 3, items % 3
    C = np.array(_CUBE, np.float32)
    g = c["g"].numpy().reshape(B, -1, 8, 3)
    t = np.zeros((items.shape[0], B, 3), np.float32)
    for idx in range(8):
        t = t + C[idx, corner][:, None, None] * g[:, f, idx, :].transpose(1, 0, 2)
    want = replay_gather(t.reshape(-1, B * 3), A.csr.offsets.cpu().numpy(), A.csr.chunks.cpu().numpy(), A.csr.long_rows.cpu().numpy(),
                         A.csr.long_chunk_ptr.cpu().numpy(), vc.LONG_ROW)
    want = torch.from_numpy(np.ascontiguousarray(want.reshape(V, B, 3).transpose(1, 0, 2)))
    assert torch.equal(_bits(got).cpu(), _bits(want))


# ---- 3. through the renderer --------------------------------------------------------------------------------------------
def test_colour_gradient_through_a_render():
    from deep3dmap_amd import _lib, neural_renderer as nr, synthetic
    v_np, tri_np = synthetic.icosphere(1)
    V = v_np.shape[0]
    v, tri = torch.from_numpy(v_np)[None].cuda(), torch.from_numpy(tri_np)[None].cuda()
    gen = torch.Generator().manual_seed(2)
    colors = torch.rand(V, 3, generator=gen).cuda().requires_grad_(True)
    target = torch.rand(3, 3, 32, 32, generator=gen).cuda()
    r = nr.Renderer(camera_mode="look_at", image_size=32, anti_aliasing=False)
    r.eye = torch.tensor([[0.0, 0.0, -2.7], [1.6, 0.9, -2.0], [-1.9, -0.6, 1.8]]).cuda()
    runs = []
    with _lib.deterministic():
        for _ in range(2):
            colors.grad = None
            tex = nr.textures_from_vertex_colors(colors, tri[0])
            tex.retain_grad()
            rgb = r.render(v, tri, tex)[0]
            ((rgb - target) ** 2).sum().backward()
            runs.append((rgb.detach().clone(), tex.grad.clone(), colors.grad.clone()))
    assert torch.equal(_bits(runs[0][2]), _bits(runs[1][2]))
    rgb, gt, gc = runs[0]
    assert rgb.shape == (3, 3, 32, 32) and float(gc.abs().max()) > 0
    ref, mag, valence = adjoint64(gt, tri[0], V)
    _within_bound(gc[None], ref, mag, valence)
    # the images are those of the restatement's cubes
    cubes = restate_cubes(colors.detach().cpu()[None], tri[0].cpu()).cuda()
    with torch.no_grad():
        want = r.render(v, tri, cubes)[0]
    assert torch.equal(_bits(rgb), _bits(want))


# ---- 4. capture ---------------------------------------------------------------------------------------------------------
def test_captured_step_over_the_module():
    from deep3dmap_amd import _lib, neural_renderer as nr
    from deep3dmap_amd.graph import CapturedStep
    faces, V, _ = irregular_mesh(seed=4)
    gen = torch.Generator().manual_seed(9)
    colors0 = torch.rand(V, 3, generator=gen)
    w = torch.rand(1, faces.shape[0], 2, 2, 2, 3, generator=gen).cuda()
    m = nr.VertexColors(colors0, faces).cuda()
    twin = nr.VertexColors(colors0, faces).cuda()          # eager, outside the step's stream

    def run(mod):
        mod.colors.grad = None
        ((mod() ** 2) * w).sum().backward()                # (a gradient that depends on the colours)
        return mod.colors.grad

    with _lib.deterministic():
        cs = CapturedStep(lambda: run(m)).capture()
        for i in range(3):
            delta = torch.rand(V, 3, generator=gen).cuda() - 0.5
            with torch.no_grad():
                m.colors.add_(delta)
                twin.colors.add_(delta)
            got = cs().clone()
            torch.cuda.synchronize()
            want = run(twin)
            assert float(want.abs().max()) > 0 and torch.equal(_bits(got), _bits(want)), i
        cs.release()
    assert len(m._adjacency) == 1


def test_first_call_inside_a_capture_raises_and_launches_nothing():
    from deep3dmap_amd import neural_renderer as nr
    from deep3dmap_amd.graph import CapturedStep
    faces, V, _ = irregular_mesh(seed=5)
    m = nr.VertexColors(torch.rand(V, 3), faces).cuda()
    torch.cuda.synchronize()
    with kernels_launched() as k:
        with pytest.raises(RuntimeError, match="adjacency.*capture"):
            CapturedStep(lambda: m()).capture(warmup=0)
    assert not k.names, k.names
    assert len(m._adjacency) == 0
    assert m().shape == (1, faces.shape[0], 2, 2, 2, 3)    # eager: builds it


# ---- 5. MultiViewFit(vertex_colors=...), one rank -----------------------------------------------------------------------
def _fit_scene():
    from deep3dmap_amd import synthetic
    v, tri = synthetic.grid_mesh(9)
    colors = np.random.default_rng(3).random((v.shape[0], 3), dtype=np.float32)
    return v, tri, colors, synthetic.camera_ring(4)


def test_multiview_fit_with_vertex_colors():
    from deep3dmap_amd import synthetic
    from deep3dmap_amd.multiview import MultiViewFit
    v, tri, colors, eyes = _fit_scene()
    V = v.shape[0]
    fit = MultiViewFit(v, tri, None, eyes, image_size=64, vertex_colors=colors)
    assert fit._flat.numel() == 1 + 6 * V and not fit.split_exchange and fit._sink[1] is None
    fit.set_targets_from(synthetic.perturb(v))
    loss, gv, gc = fit.step()
    assert gc.shape == (V, 3) and gc.data_ptr() == fit._flat[1 + 3 * V:].data_ptr()
    cubes = restate_cubes(torch.from_numpy(colors)[None], torch.from_numpy(tri))[0]
    twin = MultiViewFit(v, tri, cubes, eyes, image_size=64)
    twin.set_targets_from(synthetic.perturb(v))
    loss_t, gv_t, gt_t = twin.step()
    torch.cuda.synchronize()
    ref, mag, valence = adjoint64(gt_t[None], torch.from_numpy(tri), V)
    err = (gc.double().cpu()[None] - ref).abs()
    bound = adjoint_bound(mag, valence) + 1e-5 * float(ref.abs().max())
    assert float(ref.abs().max()) > 0 and bool((err <= bound).all()), float((err - bound).max())
    assert abs(float(loss) - float(loss_t)) <= 1e-5 * abs(float(loss_t))
    assert float((gv - gv_t).abs().max()) <= 1e-5 * float(gv_t.abs().max())
    # captured and replayed: the same step
    eager = (float(loss), gv.clone(), gc.clone())
    fit.capture_graph()
    assert fit.graph_captured and len(fit._color_adjacency) == 1
    for _ in range(2):
        loss, gv, gc = fit.step()
    torch.cuda.synchronize()
    assert abs(float(loss) - eager[0]) <= 1e-5 * abs(eager[0])
    assert float((gv - eager[1]).abs().max()) <= 1e-5 * float(eager[1].abs().max())
    assert float((gc - eager[2]).abs().max()) <= 1e-5 * float(eager[2].abs().max())
    fit.release_graph()
    # colours that do not learn: nothing of them in the buffer
    frozen = MultiViewFit(v, tri, None, eyes, image_size=64, vertex_colors=colors, optimise_textures=False)
    frozen.set_targets_from(synthetic.perturb(v))
    assert frozen._flat.numel() == 1 + 3 * V and frozen.step()[2] is None


def test_multiview_fit_vertex_color_argument_errors():
    from deep3dmap_amd.multiview import MultiViewFit
    v, tri, colors, eyes = _fit_scene()
    cubes = np.zeros((tri.shape[0], 2, 2, 2, 3), np.float32)
    with pytest.raises(ValueError, match="either"):
        MultiViewFit(v, tri, cubes, eyes, image_size=64, vertex_colors=colors)
    with pytest.raises(ValueError, match="either"):
        MultiViewFit(v, tri, None, eyes, image_size=64)
    with pytest.raises(ValueError, match="split_exchange"):
        MultiViewFit(v, tri, None, eyes, image_size=64, vertex_colors=colors, split_exchange=True)
    with pytest.raises(ValueError, match="vertex_colors must be"):
        MultiViewFit(v, tri, None, eyes, image_size=64, vertex_colors=colors[:-1])


# ---- 6. two ranks on one device -----------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_ranks(world, out):
    """`world` child processes of tests/vertex_color_worker.py (ranks of one job: they run together), each under a
    time limit; every exit status is asserted before this returns."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), WORLD_SIZE=str(world),
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, os.path.join(ROOT, "tests", "vertex_color_worker.py"), "--out", out]
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
    V = one["gv"].shape[0]
    assert one["gc"].shape == (V, 3) and int(one["flat_numel"]) == 1 + 6 * V
    for r in range(2):
        assert abs(float(two[r]["loss"]) - float(one["loss"])) <= 1e-5 * abs(float(one["loss"]))
        for key in ("gv", "gc"):
            a, b = two[r][key], one[key]
            assert np.abs(b).max() > 0 and np.abs(a - b).max() <= 1e-5 * np.abs(b).max(), (r, key)
