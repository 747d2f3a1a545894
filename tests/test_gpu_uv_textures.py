"""Learnable uv images on the device (neural_renderer/uv_textures.py): the forward against load_textures_from_image bit for
bit, the fixed-order adjoint against a float64 restatement of the sampling map (tests/test_uv_textures_host.py), the
dot-product identity, determinism (eager, replayed, through the renderer), the chain rule through a render, UVTextures
.from_obj against load_obj, and a short fit."""
import numpy as np
import pytest
import torch

from test_uv_textures_host import load_case, load_cases, restate_cubes64

pytestmark = pytest.mark.gpu

WRAPS = ["REPEAT", "MIRRORED_REPEAT", "CLAMP_TO_EDGE", "CLAMP_TO_BORDER"]


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def tex_golden():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                                "tex_golden.npz"))


def _random_layout(rng, F, scale=2.0):
    """uv corners well outside [0,1]: negative, and a block of integer corners (REPEAT's 0 -> 1 case)"""
    uv = (rng.standard_normal((F, 3, 2)) * scale).astype(np.float32)
    uv[: F // 8] = np.round(uv[: F // 8])
    uv[F // 8: F // 4] = rng.integers(0, 2, (F // 4 - F // 8, 3, 2)).astype(np.float32)   # exactly 0 and 1: last row / column
    return uv


def _grid_uv(n):
    """faces_uv [F,3,2] of synthetic.grid_mesh(n): vertex (i, j) at uv (j, i) / (n - 1)"""
    from deep3dmap_amd import synthetic
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    uv = np.stack([j, i], -1).reshape(-1, 2).astype(np.float32) / (n - 1)
    return uv[synthetic.grid_topology(n)]


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


# ---- 1. forward -----------------------------------------------------------------------------------------------------
def test_forward_equals_load_textures_on_every_golden_case(tex_golden):
    from deep3dmap_amd.neural_renderer import obj_io, textures_from_image
    names = load_cases(tex_golden)
    assert len(names) == 8
    for name in names:
        c = load_case(tex_golden, name)
        ts, wrap, bil = c["textures_in"].shape[1], int(c["wrapping"]), bool(c["bilinear"])
        img, uv, tin, upd = _dev(c["image"]), _dev(c["faces_uv"]), _dev(c["textures_in"]), _dev(c["is_update"])
        got = textures_from_image(img, uv, ts, wrap, bil, faces_mask=upd, base=tin)
        assert torch.equal(_bits(got), _bits(_dev(c["textures_out"]))), name
        want = obj_io.load_textures_from_image(img, uv, torch.zeros_like(tin), torch.ones_like(upd), wrap, bil)
        assert torch.equal(_bits(textures_from_image(img, uv, ts, wrap, bil)), _bits(want)), name


@pytest.mark.parametrize("wrapping", WRAPS)
@pytest.mark.parametrize("bilinear", [True, False])
def test_forward_equals_load_textures_on_random_layouts(wrapping, bilinear):
    from deep3dmap_amd.neural_renderer import obj_io, textures_from_image
    rng = np.random.default_rng(WRAPS.index(wrapping) * 2 + int(bilinear))
    code = obj_io.texture_wrapping_dict[wrapping]
    for ts, (H, W) in ((2, (23, 41)), (3, (40, 17)), (4, (8, 8)), (5, (1, 9))):
        F = 300
        uv = _dev(_random_layout(rng, F))
        img = _dev(rng.random((H, W, 3), dtype=np.float32))
        base = _dev(rng.random((F, ts, ts, ts, 3), dtype=np.float32))
        mask = _dev((rng.random(F) > 0.4).astype(np.int32))
        want = obj_io.load_textures_from_image(img, uv, torch.zeros_like(base), torch.ones_like(mask), code, bilinear)
        assert torch.equal(_bits(textures_from_image(img, uv, ts, wrapping, bilinear)), _bits(want))
        want = obj_io.load_textures_from_image(img, uv, base.clone(), mask, code, bilinear)
        assert torch.equal(_bits(textures_from_image(img, uv, ts, wrapping, bilinear, faces_mask=mask, base=base)),
                           _bits(want))
        assert torch.equal(_bits(textures_from_image(img, uv, ts, wrapping, bilinear, faces_mask=mask.bool(), base=base)),
                           _bits(want))
        # masked-out faces without a base are zeros
        got = textures_from_image(img, uv, ts, wrapping, bilinear, faces_mask=mask)
        assert torch.equal(got[mask == 0], torch.zeros_like(got[mask == 0]))
        # a batch of images is B single calls; base shared or per image
        B = 3
        imgs = _dev(rng.random((B, H, W, 3), dtype=np.float32))
        bases = _dev(rng.random((B, F, ts, ts, ts, 3), dtype=np.float32))
        got = textures_from_image(imgs, uv, ts, wrapping, bilinear, faces_mask=mask, base=base)
        got_b = textures_from_image(imgs, uv, ts, wrapping, bilinear, faces_mask=mask, base=bases)
        assert got.shape == (B, F, ts, ts, ts, 3)
        for b in range(B):
            one = textures_from_image(imgs[b], uv, ts, wrapping, bilinear, faces_mask=mask, base=base)
            assert torch.equal(_bits(got[b]), _bits(one))
            one = textures_from_image(imgs[b], uv, ts, wrapping, bilinear, faces_mask=mask, base=bases[b].contiguous())
            assert torch.equal(_bits(got_b[b]), _bits(one))


def test_argument_errors_on_the_device():
    from deep3dmap_amd.neural_renderer import textures_from_image
    img, uv = torch.rand(5, 6, 3).cuda(), torch.rand(4, 3, 2).cuda()
    with pytest.raises(RuntimeError, match="contiguous"):
        textures_from_image(img.transpose(0, 1), uv)
    with pytest.raises(RuntimeError, match="CUDA"):
        textures_from_image(img, uv, faces_mask=torch.ones(4, dtype=torch.int32))
    with pytest.raises(NotImplementedError):
        textures_from_image(img, uv.clone().requires_grad_(True))


# ---- 2. the adjoint against float64 ------------------------------------------------------------------------------------
def _check_adjoint(uv_np, H, W, ts, wrapping, bilinear, mask_np=None, seed=0):
    from deep3dmap_amd.neural_renderer import obj_io, textures_from_image
    code = obj_io.texture_wrapping_dict[wrapping]
    rng = np.random.default_rng(seed)
    F = uv_np.shape[0]
    img = _dev(rng.random((H, W, 3), dtype=np.float32)).requires_grad_(True)
    g = rng.standard_normal((F, ts, ts, ts, 3)).astype(np.float32)
    mask = None if mask_np is None else _dev(mask_np)
    out = textures_from_image(img, _dev(uv_np), ts, wrapping, bilinear, faces_mask=mask)
    out.backward(_dev(g))
    got = img.grad.double().cpu()
    x64 = img.detach().double().cpu().requires_grad_(True)
    g64 = torch.from_numpy(g).double()
    # (+ 0 * sum: under CLAMP_TO_BORDER the map is zero and the image would leave the graph)
    ((restate_cubes64(x64, uv_np, ts, code, bilinear, mask_np) * g64).sum() + 0 * x64.sum()).backward()
    a64 = torch.zeros_like(x64, requires_grad=True)
    ((restate_cubes64(a64, uv_np, ts, code, bilinear, mask_np) * g64.abs()).sum() + 0 * a64.sum()).backward()
    ref, bound = x64.grad, a64.grad                 # bound: sum of |w g| over each pixel's entries (w >= 0)
    err = (got - ref).abs()
    assert bool((err <= 1e-5 * bound).all()), (wrapping, bilinear, ts, float((err - 1e-5 * bound).max()))
    return got, ref, bound


@pytest.mark.parametrize("wrapping", WRAPS)
@pytest.mark.parametrize("bilinear", [True, False])
@pytest.mark.parametrize("ts", [2, 3, 4])
def test_adjoint_matches_float64_per_pixel(wrapping, bilinear, ts):
    rng = np.random.default_rng(ts * 7 + int(bilinear))
    F, H, W = 700, 29, 37
    uv = _random_layout(rng, F)
    mask = (rng.random(F) > 0.25).astype(np.int32)
    got, ref, bound = _check_adjoint(uv, H, W, ts, wrapping, bilinear, mask, seed=ts)
    if wrapping == "CLAMP_TO_BORDER":
        assert float(got.abs().max()) == 0.0
    else:
        assert float(bound[0, 0].sum()) > 0 and float(bound[-1].abs().sum() + bound[:, -1].abs().sum()) > 0
        # the hot spot really is long: it goes through the chunked reduction
        assert int(mask.sum()) > 64


def test_adjoint_at_the_hot_spot_of_a_large_grid():
    """pixel (0,0) holds one entry per face (~20k, 20 chunks), and so do its zero-weight neighbours before dropping"""
    uv = _grid_uv(100)
    got, ref, bound = _check_adjoint(uv, 96, 160, 4, "REPEAT", True, seed=1)
    assert float(bound[0, 0].sum()) > 0


# ---- 3. dot-product identity -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bilinear", [True, False])
def test_dot_product_identity(bilinear):
    from deep3dmap_amd.neural_renderer import textures_from_image
    from deep3dmap_amd.neural_renderer.uv_textures import uv_texture_adjoint, uv_transpose
    rng = np.random.default_rng(11)
    F, H, W, ts = 500, 31, 53, 3              # H != W: swapped axes show
    uv = _dev(_random_layout(rng, F, 0.7))
    x = _dev(rng.random((H, W, 3), dtype=np.float32))
    y = _dev(rng.random((F, ts, ts, ts, 3), dtype=np.float32))
    Tx = textures_from_image(x, uv, ts, "MIRRORED_REPEAT", bilinear)
    T = uv_transpose(uv, ts, H, W, "MIRRORED_REPEAT", bilinear)
    lhs = float((Tx.double() * y.double()).sum())
    for lanes in (1, 2, 4, 8, 16):            # every walk of the short rows
        Ty = uv_texture_adjoint(T._replace(lanes_per_row=lanes), y.reshape(1, -1))[0]
        rhs = float((x.double() * Ty.double()).sum())
        assert abs(lhs - rhs) <= 1e-6 * abs(lhs), lanes


@pytest.fixture(scope="module")
def hot_pixel_layout():
    """2100 random faces on a 29 x 37 image, ts = 2, bilinear, REPEAT, no mask: texel 0 of every face samples pixel (0,0), a
    row of three chunks.  The transpose, a cube gradient for two images and the per-entry terms float32(weight) * g[texel]
    (one rounding: what the kernels add), computed once."""
    from deep3dmap_amd.neural_renderer.uv_textures import uv_transpose
    rng = np.random.default_rng(21)
    F, H, W, ts, B = 2100, 29, 37, 2, 2
    uv = _dev(_random_layout(rng, F))
    T = uv_transpose(uv, ts, H, W, "REPEAT", True)
    g = rng.standard_normal((B, F * ts ** 3, 3)).astype(np.float32)
    entries = T.csr.items.cpu().numpy()
    weight = np.ascontiguousarray(entries[:, 1]).view(np.float32)
    terms = weight[:, None, None] * g[:, entries[:, 0], :].transpose(1, 0, 2)          # [nnz, B, 3]
    return dict(T=T, uv=uv, g=g, terms=terms.reshape(-1, B * 3), B=B, H=H, W=W)


@pytest.mark.parametrize("lanes", [1, 2, 4, 8, 16])
def test_adjoint_has_the_bits_of_the_shared_order(hot_pixel_layout, lanes):
    """grad_image bit for bit against the numpy replay of the order csrc/d3m_row_gather.h states (tests/
    row_gather_replay.py), for every walk of the short rows and the three chunks of pixel (0,0)."""
    from deep3dmap_amd.neural_renderer import uv_textures
    from row_gather_replay import replay_gather
    c = hot_pixel_layout
    T, B, H, W = c["T"], c["B"], c["H"], c["W"]
    row_ptr = T.csr.offsets.cpu().numpy()
    assert int(row_ptr[1] - row_ptr[0]) > 2 * uv_textures.CHUNK and int(T.csr.long_chunk_ptr[1]) >= 3
    got = uv_textures.uv_texture_adjoint(T._replace(lanes_per_row=lanes), _dev(c["g"]).reshape(B, -1))
    want = replay_gather(c["terms"], row_ptr, T.csr.chunks.cpu().numpy(), T.csr.long_rows.cpu().numpy(),
                         T.csr.long_chunk_ptr.cpu().numpy(), uv_textures.LONG_ROW, lanes_per_row=lanes)
    want = torch.from_numpy(np.ascontiguousarray(want.reshape(H, W, B, 3).transpose(2, 0, 1, 3)))
    assert torch.equal(_bits(got).cpu(), _bits(want))


# ---- 4. determinism ----------------------------------------------------------------------------------------------------
def test_image_gradient_is_bit_identical_eager_and_replayed():
    from deep3dmap_amd.graph import CapturedStep
    from deep3dmap_amd.neural_renderer import textures_from_image
    rng = np.random.default_rng(4)
    uv = _dev(_grid_uv(120))
    F, ts = uv.shape[0], 4
    img = _dev(rng.random((2, 200, 300, 3), dtype=np.float32)).requires_grad_(True)
    g = _dev(rng.standard_normal((2, F, ts, ts, ts, 3)).astype(np.float32))

    def step():
        img.grad = None
        (textures_from_image(img, uv, ts) * g).sum().backward()
        return img.grad

    cs = CapturedStep(step)                   # every run on the step's stream (graph.py: one stream per leaf)
    runs = [cs().clone() for _ in range(2)]
    cs.capture()
    runs += [cs().clone() for _ in range(2)]
    cs.release()
    for r in runs[1:]:
        assert torch.equal(_bits(r), _bits(runs[0]))
    assert float(runs[0][:, 0, 0].abs().min()) > 0


@pytest.mark.parametrize("ts", [2, 3, 4])
def test_deterministic_render_chain_is_bit_identical(ts):
    from deep3dmap_amd import _lib, neural_renderer as nr, synthetic
    v, tri = synthetic.grid_mesh(40)
    v, tri = torch.from_numpy(v)[None].cuda(), torch.from_numpy(tri)[None].cuda()
    faces_uv = _dev(_grid_uv(40))
    F = faces_uv.shape[0]
    rng = np.random.default_rng(ts)
    m = nr.UVTextures(faces_uv, [_dev(rng.random((64, 48, 3), dtype=np.float32))], [torch.ones(F, dtype=torch.int32).cuda()],
                      torch.zeros(F, ts, ts, ts, 3).cuda(), texture_size=ts).cuda()
    r = nr.Renderer(camera_mode="look_at", image_size=96, anti_aliasing=False)
    r.eye = [0.4, 0.7, -2.4]
    w = torch.rand(1, 3, 96, 96, generator=torch.Generator().manual_seed(ts)).cuda()
    grads = []
    with _lib.deterministic():
        for _ in range(3):
            m.zero_grad(set_to_none=True)
            rgb, _, _ = r.render(v, tri, m()[None])
            (rgb * w).sum().backward()
            grads.append(m.images[0].grad.clone())
    for gr in grads[1:]:
        assert torch.equal(_bits(gr), _bits(grads[0]))
    assert float(grads[0].abs().max()) > 0


# ---- 5. chain rule through a render ------------------------------------------------------------------------------------
def test_image_gradient_equals_adjoint_of_the_cube_gradient():
    from deep3dmap_amd import _lib, neural_renderer as nr, synthetic
    from deep3dmap_amd.neural_renderer.uv_textures import uv_texture_adjoint, uv_transpose
    v, tri = synthetic.grid_mesh(50)
    v, tri = torch.from_numpy(v)[None].cuda(), torch.from_numpy(tri)[None].cuda()
    uv = _dev(_grid_uv(50))
    ts = 3
    img = torch.rand(80, 120, 3, generator=torch.Generator().manual_seed(2)).cuda().requires_grad_(True)
    r = nr.Renderer(camera_mode="look_at", image_size=128, anti_aliasing=False)
    r.eye = [0.3, 0.9, -2.2]
    w = torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(3)).cuda()
    with _lib.deterministic():
        tex = nr.textures_from_image(img, uv, ts, 'REPEAT', True)
        (r.render(v, tri, tex[None])[0] * w).sum().backward()
        cubes = tex.detach().clone().requires_grad_(True)
        (r.render(v, tri, cubes[None])[0] * w).sum().backward()
    want = uv_texture_adjoint(uv_transpose(uv, ts, 80, 120, 'REPEAT', True), cubes.grad.reshape(1, -1))[0]
    assert torch.equal(_bits(img.grad), _bits(want))
    assert float(want.abs().max()) > 0


# ---- 6. UVTextures.from_obj --------------------------------------------------------------------------------------------
def _write_scene(tmp_path):
    """two image materials, a Kd-only material and faces before any usemtl, on a 4x4 vertex grid"""
    from PIL import Image
    rng = np.random.default_rng(8)
    for name, shape in (("a.png", (12, 10, 3)), ("b.png", (9, 16, 3))):
        Image.fromarray((rng.random(shape) * 255).astype(np.uint8)).save(tmp_path / name)
    (tmp_path / "s.mtl").write_text("newmtl pa\nKd 0.2 0.4 0.6\nmap_Kd a.png\n\nnewmtl plain\nKd 0.9 0.1 0.3\n\n"
                                    "newmtl pb\nmap_Kd b.png\n")
    lines = ["mtllib s.mtl"]
    for i in range(4):
        for j in range(4):
            lines.append(f"v {j} {i} {0.1 * ((i * j) % 3)}")
            lines.append(f"vt {j / 3 * 1.3 - 0.1:.4f} {i / 3 * 1.2 - 0.05:.4f}")
    quads = [(i * 4 + j + 1, i * 4 + j + 2, i * 4 + j + 6, i * 4 + j + 5) for i in range(3) for j in range(3)]
    groups = [None, "pa", "plain", "pb", "pa"]
    for k, q in enumerate(quads):
        g = groups[min(k // 2, 4)]
        if g is not None and (k % 2 == 0):
            lines.append(f"usemtl {g}")
        lines.append("f " + " ".join(f"{a}/{a}" for a in q))
    (tmp_path / "s.obj").write_text("\n".join(lines) + "\n")
    return str(tmp_path / "s.obj")


@pytest.mark.parametrize("wrapping", WRAPS)
@pytest.mark.parametrize("bilinear", [True, False])
def test_from_obj_equals_load_obj(tmp_path, wrapping, bilinear):
    from deep3dmap_amd import neural_renderer as nr
    path = _write_scene(tmp_path)
    for ts in (2, 4):
        _, _, want = nr.load_obj(path, load_texture=True, texture_size=ts, texture_wrapping=wrapping,
                                 use_bilinear=bilinear)
        m = nr.UVTextures.from_obj(path, texture_size=ts, texture_wrapping=wrapping, use_bilinear=bilinear)
        assert len(m.images) == 2 and m.names == ["pa", "pb"]
        assert torch.equal(_bits(m()), _bits(want))


def test_from_obj_images_get_gradient_only_through_their_faces(tmp_path):
    from deep3dmap_amd import neural_renderer as nr
    m = nr.UVTextures.from_obj(_write_scene(tmp_path), texture_size=3)
    masks = m.masks()
    out = m()
    for i in range(2):
        own = masks[i].bool()
        for sel, expect_nonzero in ((own, True), (~own, False)):
            m.zero_grad(set_to_none=False)
            g = torch.zeros_like(out)
            g[sel] = 1.0
            m().backward(g)
            assert (float(m.images[i].grad.abs().sum()) > 0) == expect_nonzero, (i, expect_nonzero)


# ---- 7. a short fit ----------------------------------------------------------------------------------------------------
def test_twenty_adam_steps_halve_the_loss():
    from deep3dmap_amd import neural_renderer as nr, synthetic
    v, tri = synthetic.grid_mesh(30)
    v, tri = torch.from_numpy(v)[None].cuda(), torch.from_numpy(tri)[None].cuda()
    uv = _dev(_grid_uv(30))
    gen = torch.Generator().manual_seed(6)
    r = nr.Renderer(camera_mode="look_at", image_size=64, anti_aliasing=False)
    r.eye = [0.3, 0.8, -2.4]
    target_img = torch.rand(16, 16, 3, generator=gen).cuda()
    with torch.no_grad():
        target = r.render(v, tri, nr.textures_from_image(target_img, uv, 2)[None])[0]
    img = torch.full((16, 16, 3), 0.5).cuda().requires_grad_(True)
    opt = torch.optim.Adam([img], lr=0.05)
    losses = []
    for _ in range(20):
        opt.zero_grad()
        loss = ((r.render(v, tri, nr.textures_from_image(img, uv, 2)[None])[0] - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert losses[-1] <= 0.5 * losses[0], losses
