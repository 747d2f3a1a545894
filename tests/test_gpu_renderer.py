"""GPU tests of the Python mirror (deep3dmap_amd.neural_renderer) against the oracle's torch-CPU
restatement of the reference wrappers and against the reference's own known-answer tests."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _nr():
    import deep3dmap_amd.neural_renderer as nr
    return nr


def _t(golden, key):
    return torch.from_numpy(golden[key]).cuda()


# ---- the reference's own tests, run against the HIP path ---------------------------------------------
@pytest.mark.parametrize("which", ["sil1", "sil2"])
@pytest.mark.parametrize("mode", ["sil", "rgb"])
def test_reference_known_answer_gradients(golden, which, mode):
    """tests/test_rasterize_silhouettes.py:37-99, tests/test_rasterize.py:84-156 (rtol 1e-2), including
    the to_minibatch fixture: sample in slot 2 of a zero batch of 4."""
    nr = _nr()
    v = golden[f"known/{which}/vertices"]
    pxi, pyi = (int(t) for t in golden[f"known/{which}/pxy"])
    vert = torch.zeros(4, 3, 3)
    vert[2] = torch.from_numpy(v)
    vert = vert.cuda().requires_grad_(True)
    faces = torch.zeros(4, 1, 3, dtype=torch.int32)
    faces[2] = torch.tensor([[0, 1, 2]], dtype=torch.int32)
    faces = faces.cuda()
    renderer = nr.Renderer(camera_mode='look_at')
    renderer.image_size = 64
    renderer.anti_aliasing = False
    renderer.perspective = False
    if mode == "sil":
        images = renderer(vert, faces, mode='silhouettes')
    else:
        renderer.light_intensity_ambient = 1.0
        renderer.light_intensity_directional = 0.0
        tex = torch.zeros(4, 1, 4, 4, 4, 3)
        tex[2] = 1
        images, _, _ = renderer(vert, faces, tex.cuda())
        images = torch.mean(images, dim=1)
    target = 1 if which == "sil1" else 0
    loss = torch.sum(torch.abs(images[:, pyi, pxi] - target))
    loss.backward()
    g = vert.grad.cpu().numpy()
    assert np.allclose(g[2], golden[f"known/{which}/grad"], rtol=1e-2, atol=1e-8)
    assert np.abs(g[[0, 1, 3]]).max() == 0


def test_look_at_and_perspective_known_answers(golden):
    nr = _nr()
    v = torch.tensor([[[1., 0., 0.]]]).cuda()
    for eye, ans in zip(golden["known/look_at/eyes"], golden["known/look_at/answers"]):
        assert np.allclose(nr.look_at(v, eye).squeeze().cpu().numpy(), ans, atol=1e-6)
    out = nr.perspective(torch.from_numpy(golden["known/perspective/in"])[None, None].cuda())
    assert np.allclose(out.squeeze().cpu().numpy(), golden["known/perspective/out"])


def test_depth_backward_finite_differences():
    """The intent of tests/test_rasterize_depth.py:56-89 (vacuous there: it reads batch slot 0): analytic
    depth gradient vs central finite differences, atol 1e-3."""
    nr = _nr()
    v0 = torch.tensor([[[-0.9, -0.9, 2.], [-0.8, 0.8, 1.], [0.8, 0.8, 0.5]]]).cuda()
    faces = torch.tensor([[[0, 1, 2]]], dtype=torch.int32).cuda()
    renderer = nr.Renderer(camera_mode='look_at')
    renderer.image_size, renderer.anti_aliasing, renderer.perspective, renderer.camera_mode = 64, False, False, 'none'

    def loss_of(v):
        return torch.sum((renderer(v, faces, mode='depth')[0, 15, 20] - 1) ** 2)

    v = v0.clone().requires_grad_(True)
    loss_of(v).backward()
    g = v.grad[0].cpu().numpy()
    fd = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            e = torch.zeros_like(v0)
            e[0, i, j] = 1e-3
            fd[i, j] = ((loss_of(v0 + e) - loss_of(v0 - e)) / 2e-3).item()
    assert np.abs(g).max() > 1e-3
    assert np.allclose(g, fd, atol=1e-3)


# ---- camera / gather / lighting kernels against vectors made from the reference's python modules ------
def test_camera_kernels_match_reference_modules(golden):
    nr = _nr()
    g = golden
    v = _t(g, "cam/projection/vertices").requires_grad_(True)
    out = nr.projection(v, _t(g, "cam/projection/K"), _t(g, "cam/projection/R"), _t(g, "cam/projection/t"),
                        _t(g, "cam/projection/dist"), int(g["cam/projection/orig_size"]))
    assert torch.allclose(out.cpu(), torch.from_numpy(g["cam/projection/out"]), rtol=1e-5, atol=2e-6)
    out.backward(_t(g, "cam/projection/grad_out"))
    assert torch.allclose(v.grad.cpu(), torch.from_numpy(g["cam/projection/grad_vertices"]), rtol=1e-3, atol=1e-4)
    v = _t(g, "cam/look_at/vertices").requires_grad_(True)
    la = nr.look_at(v, _t(g, "cam/look_at/eyes"))
    assert torch.allclose(la.cpu(), torch.from_numpy(g["cam/look_at/out"]), rtol=1e-5, atol=2e-6)
    pp = nr.perspective(la, float(g["cam/look_at/persp_angle"]))
    assert torch.allclose(pp.cpu(), torch.from_numpy(g["cam/look_at/persp_out"]), rtol=1e-5, atol=2e-6)
    pp.backward(_t(g, "cam/look_at/grad_out"))
    assert torch.allclose(v.grad.cpu(), torch.from_numpy(g["cam/look_at/grad_vertices"]), rtol=1e-3, atol=1e-5)
    la1 = nr.look_at(_t(g, "cam/look_at/vertices"), [0, 0, -2.732])
    assert torch.allclose(la1.cpu(), torch.from_numpy(g["cam/look_at/single_eye_out"]), rtol=1e-5, atol=2e-6)
    for (d, e, a), ref in zip(g["cam/points_from_angles/in"], g["cam/points_from_angles/out"]):
        assert np.allclose(nr.get_points_from_angles(float(d), float(e), float(a)), ref, rtol=1e-6)


def test_gather_and_lighting_match_reference_modules(golden):
    nr = _nr()
    g = golden
    verts = _t(g, "cam/projection/vertices").requires_grad_(True)
    f = nr.vertices_to_faces(verts, _t(g, "cam/v2f/faces"))
    assert torch.equal(f.cpu(), torch.from_numpy(g["cam/v2f/out"]))
    p = g["cam/lighting/params"]
    tex = _t(g, "cam/lighting/textures").requires_grad_(True)
    lit = nr.lighting(f, tex, float(p[0]), float(p[1]), tuple(p[2:5]), tuple(p[5:8]), tuple(p[8:11]))
    assert torch.allclose(lit.cpu(), torch.from_numpy(g["cam/lighting/out"]), rtol=1e-5, atol=1e-6)
    # gradients of the whole gather+lighting chain against torch autograd on the oracle's restatement
    from oracle import nr_oracle as O
    go = torch.randn(lit.shape, generator=torch.Generator().manual_seed(5))
    lit.backward(go.cuda())
    vc = torch.from_numpy(g["cam/projection/vertices"]).requires_grad_(True)
    tc = torch.from_numpy(g["cam/lighting/textures"]).requires_grad_(True)
    lc = O.lighting(O.vertices_to_faces(vc, torch.from_numpy(g["cam/v2f/faces"])), tc, float(p[0]), float(p[1]),
                    tuple(p[2:5]), tuple(p[5:8]), tuple(p[8:11]))
    lc.backward(go)
    assert torch.allclose(tex.grad.cpu(), tc.grad, rtol=1e-4, atol=1e-6)
    assert torch.allclose(verts.grad.cpu(), vc.grad, rtol=1e-3, atol=1e-4)


# ---- end to end: Renderer on a small mesh, every mode / camera, against the oracle renderer ----------
def _scene(B=2, n=14):
    from deep3dmap_amd import synthetic
    v, tri = synthetic.grid_mesh(n)
    tex = synthetic.random_textures(tri.shape[0], 2)
    return (torch.from_numpy(v)[None].repeat(B, 1, 1), torch.from_numpy(tri)[None].repeat(B, 1, 1),
            torch.from_numpy(tex)[None].repeat(B, 1, 1, 1, 1, 1))


def _rel_l2(a, b):
    return float(torch.linalg.norm(a - b) / (torch.linalg.norm(b) + 1e-12))


def _rel_max(a, b):
    """largest deviation relative to the reference tensor's largest entry (north_star: 1e-3 on backward gradients)"""
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


# The oracle's cameras produce their forward VALUES in the same f32 association as the HIP kernels (oracle/nr_oracle.py
# "EXACT"), so both rasterize bit-identical screen-space vertices: silhouettes must be EQUAL, images agree to rounding of
# the shading arithmetic, gradients to north_star's 1e-3.
IMG_TOL, GRAD_TOL = 2e-6, 1e-3


def _record_association(name, info):
    """one case's numbers into gpurun_out/camera_association.json (copied to profiles/ by hand)"""
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out", "camera_association.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    data = json.load(open(path)) if os.path.exists(path) else {}
    data[name] = info
    json.dump(data, open(path, "w"), indent=1, sort_keys=True)


class _association:
    """The oracle's cameras in the product's f32 association ("product": oracle.nr_oracle.EXACT, the default -- both
    sides rasterize bit-identical vertices) or in torch's = the reference modules' own (NR/look_at.py:48-60,
    NR/projection.py:19-42: "reference") -- the independent end-to-end pin of the camera stage (missing 3)."""

    def __init__(self, which):
        self.exact = which == "product"

    def __enter__(self):
        from oracle import nr_oracle as O
        self.saved, O.EXACT = O.EXACT, self.exact

    def __exit__(self, *exc):
        from oracle import nr_oracle as O
        O.EXACT = self.saved
        return False


FLIP_FRAC, AWAY_IMG_TOL = 5e-4, 1e-4       # reference association: flipped pixels, and image error away from them


def _compare_end_to_end(ref, got, association, name):
    """ref / got = [rgb, depth, alpha, loss, grad_vertices, grad_textures] of the oracle / the product."""
    if association == "product":
        assert torch.equal(ref[2], got[2])
        assert _rel_max(got[0], ref[0]) < IMG_TOL and _rel_max(got[1], ref[1]) < IMG_TOL
        assert abs(float(got[3] - ref[3])) / float(ref[3]) < 1e-5
        assert _rel_max(got[5], ref[5]) < GRAD_TOL
        assert _rel_max(got[4], ref[4]) < GRAD_TOL
        return
    # The reference's own association: vertices differ in the last bit, so a pixel centre within an ulp of an edge may
    # change owner.  Count those (silhouette: alpha differs; interior: another face's texels), and hold everything
    # else to 1e-4 (images) / 1e-3 (gradients; of a case in which no pixel flipped -- a flipped pixel's whole
    # contribution moves, which is not an error of either side).
    sil = ref[2] != got[2]
    rgb_d = (got[0] - ref[0]).abs().amax(1)
    interior = (~sil) & (rgb_d > 1e-3 * float(ref[0].abs().max()))
    flipped = sil | interior
    away = ~flipped
    info = {"pixels": int(sil.numel()), "flipped_silhouette": int(sil.sum()), "flipped_interior": int(interior.sum()),
            "rgb_err_away": float(rgb_d[away].max() / ref[0].abs().max()),
            "depth_err_away": float(((got[1] - ref[1]).abs() / ref[1].abs().clamp_min(1e-6))[away].max()),
            "loss_rel": abs(float(got[3] - ref[3])) / float(ref[3]),
            "grad_vertices_rel_max": _rel_max(got[4], ref[4]), "grad_textures_rel_max": _rel_max(got[5], ref[5])}
    _record_association(name, info)
    assert int(flipped.sum()) <= max(2, FLIP_FRAC * flipped.numel()), info
    assert info["rgb_err_away"] <= AWAY_IMG_TOL and info["depth_err_away"] <= AWAY_IMG_TOL, info
    if not int(flipped.sum()):
        assert info["grad_vertices_rel_max"] < GRAD_TOL and info["grad_textures_rel_max"] < GRAD_TOL, info
    else:
        assert info["grad_vertices_rel_max"] < 0.2 and info["grad_textures_rel_max"] < 0.2, info


@pytest.mark.parametrize("association", ["product", "reference"])
@pytest.mark.parametrize("camera", ["look_at", "look", "projection"])
@pytest.mark.parametrize("aa", [False, True])
def test_renderer_end_to_end_against_oracle(camera, aa, association):
    nr = _nr()
    from oracle import nr_oracle as O
    v, tri, tex = _scene()
    kw = dict(image_size=48, anti_aliasing=aa, camera_mode=camera, background_color=[0.2, 0.3, 0.4],
              light_direction=[0.3, 0.8, -0.5])
    if camera == "projection":
        K = torch.tensor([[[60., 0., 24.], [0., 60., 24.], [0., 0., 1.]]])
        R = O.get_rotation_matrix(torch.tensor([0.2]), torch.tensor([-0.3]), torch.tensor([0.1]))
        t = torch.tensor([[[0.05, -0.02, 2.6]]])
        kw.update(K=K, R=R, t=t, orig_size=48)
    ro = O.Renderer(**kw)
    kw_g = dict(kw)
    for k in ("K", "R", "t"):
        if k in kw_g:
            kw_g[k] = kw_g[k].cuda()
    rg = nr.Renderer(**kw_g)
    if camera != "projection":
        ro.eye = rg.eye = [0.6, 0.9, -2.3]
    gen = torch.Generator().manual_seed(11)
    targets = (torch.rand(2, 3, 48, 48, generator=gen), torch.rand(2, 48, 48, generator=gen),
               torch.rand(2, 48, 48, generator=gen))

    def run(renderer, dev):
        vv = v.detach().clone().to(dev).requires_grad_(True)
        tt = tex.detach().clone().to(dev).requires_grad_(True)
        rgb, depth, alpha = renderer(vv, tri.to(dev), tt)
        loss = ((rgb - targets[0].to(dev)) ** 2).sum() + ((alpha - targets[1].to(dev)) ** 2).sum() + \
               (depth.clamp(max=5.0) - targets[2].to(dev)).abs().sum() * 0.1
        loss.backward()
        return [x.detach().cpu() for x in (rgb, depth, alpha, loss, vv.grad, tt.grad)]

    with _association(association):
        ref = run(ro, "cpu")
    got = run(rg, "cuda")
    _compare_end_to_end(ref, got, association, f"end_to_end[{camera},aa={int(aa)}]")


@pytest.mark.parametrize("association", ["product", "reference"])
@pytest.mark.parametrize("seed", range(12))
def test_renderer_differential_fuzz(seed, association):
    """Random meshes, cameras and settings through Renderer.render + a loss + backward on the lit path (fill_back and
    lighting on the fly, rasterization from the indexed mesh, side-stream branches, vertex-target gradients) against
    the oracle's Renderer: shared or per-view mesh, anti-aliasing on/off, several views, odd image sizes."""
    nr = _nr()
    from oracle import nr_oracle as O
    from deep3dmap_amd import synthetic
    rng = np.random.default_rng(500 + seed)
    n = int(rng.integers(5, 16))
    S = int(rng.choice([24, 30, 40, 56]))
    aa = bool(seed % 2)
    B = int(rng.integers(1, 4))
    shared = bool((seed // 2) % 2)
    vnp, tnp = synthetic.grid_mesh(n, seed=seed)
    ts = int(rng.choice([1, 2, 2, 3]))
    tex = torch.from_numpy(synthetic.random_textures(tnp.shape[0], ts))
    eyes = torch.tensor([nr.get_points_from_angles(float(rng.uniform(2.2, 3.2)), float(rng.uniform(-40, 40)),
                                                   float(rng.uniform(0, 360))) for _ in range(B)], dtype=torch.float32)
    kw = dict(image_size=S, anti_aliasing=aa, camera_mode="look_at", background_color=[0.2, 0.3, 0.4],
              light_direction=[0.3, 0.8, -0.5], fill_back=bool(seed % 3))
    gen = torch.Generator().manual_seed(seed)
    tg = (torch.rand(B, 3, S, S, generator=gen), torch.rand(B, S, S, generator=gen), torch.rand(B, S, S, generator=gen))

    def run(mod, dev, use_shared):
        r = mod.Renderer(**kw)
        r.eye = eyes.to(dev)
        nb = 1 if use_shared else B
        vv = torch.from_numpy(vnp)[None].repeat(nb, 1, 1).to(dev).requires_grad_(True)
        tt = tex[None].repeat(nb, 1, 1, 1, 1, 1).to(dev).requires_grad_(True)
        tri = torch.from_numpy(tnp)[None].repeat(nb, 1, 1).to(dev)
        rgb, depth, alpha = r(vv, tri, tt)
        loss = ((rgb - tg[0].to(dev)) ** 2).sum() + ((alpha - tg[1].to(dev)) ** 2).sum() + \
               (depth.clamp(max=5.0) - tg[2].to(dev)).abs().sum() * 0.1
        loss.backward()
        gv, gt = vv.grad, tt.grad
        if not use_shared:                        # compare like with like: sum the per-view copies
            gv, gt = gv.sum(0, keepdim=True), gt.sum(0, keepdim=True)
        return [x.detach().cpu() for x in (rgb, depth, alpha, loss, gv, gt)]

    with _association(association):
        ref = run(O, "cpu", False)
    got = run(nr, "cuda", shared)
    _compare_end_to_end(ref, got, association, f"fuzz[{seed}]")


@pytest.mark.parametrize("mode", ["silhouettes", "depth", "rgb"])
def test_single_output_modes_against_oracle(mode):
    nr = _nr()
    from oracle import nr_oracle as O
    v, tri, tex = _scene(B=1)
    ro, rg = O.Renderer(camera_mode="look_at", image_size=40), nr.Renderer(camera_mode="look_at", image_size=40)
    outs = []
    for renderer, dev in ((ro, "cpu"), (rg, "cuda")):
        vv = v.detach().clone().to(dev).requires_grad_(True)
        args = (vv, tri.to(dev)) + ((tex.to(dev),) if mode == "rgb" else ())
        img = renderer(*args, mode=mode)
        img.clamp(max=5.0).sum().backward()
        outs.append((img.detach().cpu(), vv.grad.cpu()))
    assert outs[0][0].shape == outs[1][0].shape
    assert _rel_max(outs[1][0].clamp(max=5.0), outs[0][0].clamp(max=5.0)) < IMG_TOL
    assert _rel_max(outs[1][1], outs[0][1]) < GRAD_TOL


def test_rasterize_module_matches_reference_layout():
    """Rasterize(...)(faces, textures): internal-resolution, unflipped maps; empty tensors for disabled outputs
    (NR/rasterize.py:91-98); TypeError for CPU tensors (:247-248)."""
    nr = _nr()
    from oracle import nr_oracle as O
    rng = np.random.default_rng(3)
    xy = rng.uniform(-1, 1, (1, 20, 1, 2)) + rng.uniform(-0.5, 0.5, (1, 20, 3, 2))
    faces = np.concatenate([xy, rng.uniform(0.5, 3, (1, 20, 3, 1))], -1).astype(np.float32)
    tex = rng.uniform(0, 1, (1, 20, 2, 2, 2, 3)).astype(np.float32)
    m = O.raster_forward(faces, tex, 32, 0.1, 100.0, 1e-3, (0.5, 0.5, 0.5), True, True, True)
    rgb, alpha, depth = nr.Rasterize(32, 0.1, 100.0, 1e-3, [0.5, 0.5, 0.5], True, True, True)(
        torch.from_numpy(faces).cuda(), torch.from_numpy(tex).cuda())
    assert np.allclose(rgb.cpu().numpy(), m["rgb_map"], atol=1e-6)
    assert np.array_equal(alpha.cpu().numpy(), m["alpha_map"]) and np.array_equal(depth.cpu().numpy(), m["depth_map"])
    r2 = nr.Rasterize(32, 0.1, 100.0, 1e-3, [0, 0, 0], False, True, False)(torch.from_numpy(faces).cuda(), None)
    assert r2[0].numel() == 0 and r2[2].numel() == 0 and r2[1].shape == (1, 32, 32)
    with pytest.raises(TypeError):
        nr.Rasterize(32, 0.1, 100.0, 1e-3, [0, 0, 0], False, True, False)(torch.from_numpy(faces), None)


def test_loss_kernels_match_reference_losses(golden):
    """photometric_loss / silhouette loss kernels vs vectors produced by the reference's utils.py."""
    from deep3dmap_amd.core import photometric_loss, silhouette_loss
    g = golden
    a, b, m, s = (_t(g, k) for k in ("loss/a", "loss/b", "loss/mask", "loss/sigma"))
    assert np.allclose(photometric_loss(a, b).item(), g["loss/photometric"], rtol=1e-5)
    assert np.allclose(photometric_loss(a, b, mask=m).item(), g["loss/photometric_mask"], rtol=1e-5)
    assert np.allclose(photometric_loss(a, b, mask=m, conf_sigma=s).item(), g["loss/photometric_mask_sigma"], rtol=1e-5)
    # gradients against torch autograd of the oracle's restatement
    from oracle import nr_oracle as O
    ag = a.clone().requires_grad_(True)
    (photometric_loss(ag, b, mask=m, conf_sigma=s) * 3.0).backward()
    ac = a.cpu().clone().requires_grad_(True)
    (O.photometric_loss(ac, b.cpu(), mask=m.cpu(), conf_sigma=s.cpu()) * 3.0).backward()
    assert torch.allclose(ag.grad.cpu(), ac.grad, rtol=1e-4, atol=1e-7)
    ag = a.clone().requires_grad_(True)
    silhouette_loss(ag[:, 0], b[:, 0]).backward()
    assert np.allclose(silhouette_loss(a[:, 0], b[:, 0]).item(), ((a[:, 0] - b[:, 0]) ** 2).sum().item(), rtol=1e-5)
    assert torch.allclose(ag.grad, 2 * (a - b) * torch.tensor([1., 0, 0], device="cuda").view(1, 3, 1, 1), atol=1e-6)


@pytest.mark.parametrize("shape", [(2, 8, 8), (3, 17, 5), (16, 64, 64), (1, 3, 3)])
def test_fused_smooth_loss_matches_reference_vectors_and_oracle_autograd(golden, shape):
    """smooth_loss as three kernels per pyramid level: the reference's own values (tests/golden: loss/smooth*), and
    value + gradient against torch autograd of the oracle's restatement of utils.py:82-102, incl. a pyramid, a 4-D
    input, an upstream gradient != 1 and plateaus (sign(0) = 0)."""
    from deep3dmap_amd.core import smooth_loss
    from oracle import nr_oracle as O
    a, b = _t(golden, "loss/a"), _t(golden, "loss/b")
    assert np.allclose(smooth_loss(a[:, 0]).item(), golden["loss/smooth"], rtol=1e-5)
    assert np.allclose(smooth_loss([a[:, 0], b[:, 0, ::2, ::2]]).item(), golden["loss/smooth_pyramid"], rtol=1e-5)
    B, H, W = shape
    gen = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(B, H, W, generator=gen)
    x[:, : H // 2, : W // 2] = 0.25                      # a plateau: exact zeros among the second differences
    res = []
    for fn, dev in ((smooth_loss, "cuda"), (O.smooth_loss, "cpu")):
        xx = x.clone().to(dev).requires_grad_(True)
        pyr = [xx, xx[:, ::2, ::2].contiguous()] if min(H, W) >= 6 else xx
        loss = fn(pyr)
        (loss * 1.7).backward()
        res.append((loss.detach().cpu(), xx.grad.cpu()))
    assert torch.allclose(res[0][0], res[1][0], rtol=1e-5)
    assert torch.allclose(res[0][1], res[1][1], rtol=1e-5, atol=1e-8)
    x4 = x[:, None].cuda()
    assert torch.allclose(smooth_loss(x4), smooth_loss(x.cuda()))


def test_camera_parameter_gradients_match_oracle_autograd():
    """eye (look_at, look) and K / R / t / dist_coeffs (projection) as learnable parameters: values and gradients of a
    scalar of the transformed vertices against torch autograd of the oracle's restatement of NR/look_at.py, look.py,
    projection.py (camera optimisation as in neural_renderer's example4); then a silhouette render whose loss moves
    the eye."""
    nr = _nr()
    from oracle import nr_oracle as O
    gen = torch.Generator().manual_seed(4)
    v = torch.randn(2, 30, 3, generator=gen) * 0.4
    wgt = torch.randn(2, 30, 3, generator=gen)

    def both(fn_gpu, fn_cpu, params):
        res = []
        for fn, dev in ((fn_gpu, "cuda"), (fn_cpu, "cpu")):
            ps = [p.clone().to(dev).requires_grad_(True) for p in params]
            vv = v.clone().to(dev).requires_grad_(True)
            out = fn(vv, *ps)
            (out * wgt.to(dev)).sum().backward()
            res.append([out.detach().cpu(), vv.grad.cpu()] + [p.grad.cpu() for p in ps])
        for a, b in zip(*res):
            assert torch.allclose(a, b, rtol=2e-4, atol=2e-5), float((a - b).abs().max())

    eye = torch.tensor([[0.3, 0.6, -2.5], [-1.0, 0.2, -2.0]])
    both(lambda vv, e: nr.perspective(nr.look_at(vv, e), angle=30), lambda vv, e: O.perspective(O.look_at(vv, e), angle=30), [eye])
    both(lambda vv, e: nr.look(vv, e, direction=[0.1, 0.2, 1.0]), lambda vv, e: O.look(vv, e, direction=[0.1, 0.2, 1.0]), [eye])
    K = torch.tensor([[[300., 0, 128], [0, 310., 120], [0, 0, 1]]]).repeat(2, 1, 1)
    R = torch.linalg.qr(torch.randn(2, 3, 3, generator=gen))[0]
    t = torch.tensor([[[0.1, -0.2, 3.0]], [[0.0, 0.1, 2.5]]])
    dist = torch.tensor([[0.05, -0.02, 0.001, 0.002, 0.01]]).repeat(2, 1)
    both(lambda vv, K_, R_, t_, d_: nr.projection(vv, K_, R_, t_, d_, 256),
         lambda vv, K_, R_, t_, d_: O.projection(vv, K_, R_, t_, d_, 256), [K, R, t, dist])
    # end to end: the silhouette loss reaches the eye through the rasterizer
    from deep3dmap_amd import synthetic
    mv, mt = synthetic.grid_mesh(10)
    mv, mt = torch.from_numpy(mv).cuda()[None], torch.from_numpy(mt).cuda()[None]
    r = nr.Renderer(camera_mode="look_at", image_size=48, anti_aliasing=False)
    r.eye = torch.tensor([0.5, 0.8, -2.6], device="cuda", requires_grad=True)
    sil = r(mv, mt, mode="silhouettes")
    (sil[:, :, :24].sum() - sil[:, :, 24:].sum()).backward()
    assert r.eye.grad is not None and torch.isfinite(r.eye.grad).all() and float(r.eye.grad.abs().sum()) > 0


@pytest.mark.parametrize("shape", [(2, 8, 8), (3, 20, 12), (1, 64, 64)])
def test_fused_fit_loss_matches_composed_losses_and_oracle(shape):
    """multiview_fit_loss (3 launches) against photometric + silhouette/P + photometric composed from the loss
    operators, and against torch autograd of the oracle's restatement of utils.py:105-114; a non-unit upstream
    gradient exercises the in-kernel scaling."""
    from deep3dmap_amd.core import multiview_fit_loss, photometric_loss, silhouette_loss
    from oracle import nr_oracle as O
    B, H, W = shape
    gen = torch.Generator().manual_seed(B * 1000 + H)
    rgb, rgb_t = torch.rand(B, 3, H, W, generator=gen), torch.rand(B, 3, H, W, generator=gen)
    depth, depth_t = torch.rand(B, H, W, generator=gen) + 1, torch.rand(B, H, W, generator=gen) + 1
    alpha = (torch.rand(B, H, W, generator=gen) > 0.4).float()
    alpha_t = (torch.rand(B, H, W, generator=gen) > 0.5).float()
    rgb[0, 1, 0, 0] = rgb_t[0, 1, 0, 0]                       # a zero difference: sign() must give 0 there

    def run(fn, dev):
        xs = [x.to(dev).clone().requires_grad_(True) for x in (rgb, depth, alpha)]
        ts_ = [x.to(dev) for x in (rgb_t, depth_t, alpha_t)]
        loss = fn(*xs, *ts_)
        (loss * 2.5).backward()
        return loss.detach().cpu(), [x.grad.cpu() for x in xs]

    fused = run(lambda r, d, a, rt, dt, at: multiview_fit_loss(r, d, a, rt, dt, at, at), "cuda")
    composed = run(lambda r, d, a, rt, dt, at: photometric_loss(r, rt, mask=at[:, None]) + silhouette_loss(a, at) / (H * W) +
                   photometric_loss(d[:, None], dt[:, None], mask=at[:, None]), "cuda")
    oracle = run(lambda r, d, a, rt, dt, at: O.photometric_loss(r, rt, mask=at[:, None]) + ((a - at) ** 2).sum() / (H * W) +
                 O.photometric_loss(d[:, None], dt[:, None], mask=at[:, None]), "cpu")
    for other in (composed, oracle):
        assert torch.allclose(fused[0], other[0], rtol=1e-5)
        for g, go in zip(fused[1], other[1]):
            assert torch.allclose(g, go, rtol=1e-5, atol=1e-8)
    with pytest.raises(ValueError):
        multiview_fit_loss(rgb.cuda()[:, :2], depth.cuda(), alpha.cuda(), rgb_t.cuda()[:, :2], depth_t.cuda(),
                           alpha_t.cuda(), alpha_t.cuda())


@pytest.mark.parametrize("ts", [2, 3])
def test_fit_objective_inside_the_rendering_node(ts):
    """Renderer.render_fit_loss (objective summed where the images are produced, gradient written straight into the
    internal maps) against multiview_fit_loss on the rendered images: same value, same vertex / texture gradients,
    with a non-unit upstream gradient."""
    nr = _nr()
    from deep3dmap_amd import synthetic
    from deep3dmap_amd.core import multiview_fit_loss
    v, tri = synthetic.grid_mesh(14)
    tex = synthetic.random_textures(tri.shape[0], ts)
    eyes = torch.from_numpy(synthetic.camera_ring(3)).float().cuda()
    r = nr.Renderer(image_size=56, anti_aliasing=False, camera_mode="look_at", fill_back=True)
    r.eye = eyes
    tri_d = torch.from_numpy(tri).int().cuda()[None]
    with torch.no_grad():
        tv = torch.from_numpy(synthetic.perturb(v, 0.04)).float().cuda()
        rgb_t, depth_t, alpha_t = r(tv[None], tri_d, torch.from_numpy(tex).float().cuda()[None])

    def run(inside):
        vv = torch.from_numpy(v).float().cuda().requires_grad_(True)
        tt = torch.from_numpy(tex).float().cuda().requires_grad_(True)
        if inside:
            loss = r.render_fit_loss(vv[None], tri_d, tt[None], (rgb_t, depth_t, alpha_t, alpha_t))
        else:
            rgb, depth, alpha = r(vv[None], tri_d, tt[None])
            loss = multiview_fit_loss(rgb, depth, alpha, rgb_t, depth_t, alpha_t, alpha_t)
        (loss * 1.75).backward()
        return loss.detach(), vv.grad, tt.grad

    a, b = run(True), run(False)
    assert torch.allclose(a[0], b[0], rtol=2e-6)
    assert float(a[1].abs().max()) > 0 and float(a[2].abs().max()) > 0
    # the two paths differ only in the order the four sums are added up (a factor 1/den on every gradient)
    for ga, gb in zip(a[1:], b[1:]):
        assert float((ga - gb).abs().max()) <= 1e-5 * float(gb.abs().max())


@pytest.mark.parametrize("ts", [1, 4])
@pytest.mark.parametrize("aa", [False, True])
def test_step_finishes_its_objective_at_every_texture_size(ts, aa):
    """A MultiViewFit step defers the objective's finish (partial sums -> value) to the backward pass
    (D3M_FIT_FINISH_DEFERRED).  Only the texture_size == 2 form of that pass has a kernel for it to ride in; at other
    sizes it must still happen (round 5 shipped a step whose loss stayed 0 there until this test)."""
    from deep3dmap_amd import synthetic
    from deep3dmap_amd.multiview import MultiViewFit
    v, tri = synthetic.grid_mesh(12)
    tex = synthetic.random_textures(tri.shape[0], ts)
    fit = MultiViewFit(v, tri, tex, synthetic.camera_ring(3), image_size=48, anti_aliasing=aa)
    fit.set_targets_from(synthetic.perturb(v, 0.04))
    l0, gv0, gt0 = fit.step()
    l0, gv0, gt0 = float(l0), gv0.clone(), gt0.clone()
    fit2 = MultiViewFit(v, tri, tex, synthetic.camera_ring(3), image_size=48, anti_aliasing=aa, objective_in_renderer=False)
    fit2.targets, fit2.mask_sum, fit2._mask_sum_local = fit.targets, fit.mask_sum, fit._mask_sum_local
    l1, gv1, gt1 = fit2.step()
    assert l0 > 0 and abs(l0 - float(l1)) <= 2e-6 * abs(float(l1))
    assert float((gv0 - gv1).abs().max()) <= 2e-5 * float(gv1.abs().max())
    assert float((gt0 - gt1).abs().max()) <= 2e-5 * float(gt1.abs().max())


@pytest.mark.parametrize("ts,frozen_tex", [(2, False), (1, False), (2, True)])
def test_fit_objective_inside_the_rendering_node_with_anti_aliasing(ts, frozen_tex):
    """The same with anti-aliasing (SURVEY C2 is AA-on): the objective of the 2x2-pooled images, evaluated in the pass that
    pools them; its gradient leaves as unscaled maps at the internal size.  MultiViewFit.fit_loss never changes path
    behind the caller's back."""
    nr = _nr()
    from deep3dmap_amd import synthetic
    from deep3dmap_amd.core import multiview_fit_loss
    v, tri = synthetic.grid_mesh(14)
    tex = synthetic.random_textures(tri.shape[0], ts)
    eyes = torch.from_numpy(synthetic.camera_ring(3)).float().cuda()
    r = nr.Renderer(image_size=40, anti_aliasing=True, camera_mode="look_at", fill_back=True)
    r.eye = eyes
    tri_d = torch.from_numpy(tri).int().cuda()[None]
    with torch.no_grad():
        tv = torch.from_numpy(synthetic.perturb(v, 0.04)).float().cuda()
        rgb_t, depth_t, alpha_t = r(tv[None], tri_d, torch.from_numpy(tex).float().cuda()[None])
    assert rgb_t.shape[-1] == 40
    mask = (alpha_t > 0.5).float()

    def run(inside):
        vv = torch.from_numpy(v).float().cuda().requires_grad_(True)
        tt = torch.from_numpy(tex).float().cuda().requires_grad_(not frozen_tex)
        if inside:
            loss = r.render_fit_loss(vv[None], tri_d, tt[None], (rgb_t, depth_t, alpha_t, mask))
        else:
            rgb, depth, alpha = r(vv[None], tri_d, tt[None])
            loss = multiview_fit_loss(rgb, depth, alpha, rgb_t, depth_t, alpha_t, mask)
        (loss * 0.6).backward()
        return loss.detach(), vv.grad, tt.grad

    a, b = run(True), run(False)
    assert torch.allclose(a[0], b[0], rtol=2e-6)
    for ga, gb in zip(a[1:], b[1:]):
        if gb is None:
            assert ga is None
            continue
        assert float(gb.abs().max()) > 0 and float((ga - gb).abs().max()) <= 2e-5 * float(gb.abs().max())
    # the camera-sharded fit takes the fused path with anti-aliasing too, and a captured step replays it
    from deep3dmap_amd.multiview import MultiViewFit
    fit = MultiViewFit(v, tri, tex, synthetic.camera_ring(3), image_size=40, anti_aliasing=True)
    fit.set_targets_from(synthetic.perturb(v, 0.04))
    l0, gv0, gt0 = fit.step()
    l0, gv0, gt0 = float(l0), gv0.clone(), gt0.clone()
    fit2 = MultiViewFit(v, tri, tex, synthetic.camera_ring(3), image_size=40, anti_aliasing=True, objective_in_renderer=False)
    fit2.targets, fit2.mask_sum, fit2._mask_sum_local = fit.targets, fit.mask_sum, fit._mask_sum_local
    l1, gv1, gt1 = fit2.step()
    assert abs(l0 - float(l1)) <= 2e-6 * abs(float(l1))
    assert float((gv0 - gv1).abs().max()) <= 2e-5 * float(gv1.abs().max())
    assert float((gt0 - gt1).abs().max()) <= 2e-5 * float(gt1.abs().max())
    fit.capture_graph()
    for _ in range(3):
        l2, gv2, _ = fit.step()
    assert abs(float(l2) - l0) <= 1e-6 * abs(l0) and float((gv2 - gv0).abs().max()) <= 1e-4 * float(gv0.abs().max())
    fit.release_graph()


@pytest.mark.parametrize("n", [3, 5, 6])
def test_view_transform_kernel_matches_reference_tensor_algebra(n):
    """get_transform_matrices on the device (one HIP launch each way) against the reference's tensor algebra
    (utils.py:34-71: stacked Euler factors, Rz (Ry Rx), zero-padded translation) evaluated by torch on the host:
    values and the gradient of the view through both outputs."""
    from deep3dmap_amd.core.renderer_utils import get_transform_matrices
    gen = torch.Generator().manual_seed(n)
    view = (torch.rand(7, n, generator=gen) - 0.5) * torch.tensor([3.0, 3.0, 3.0, 0.4, 0.4, 0.1][:n])
    w_r, w_t = torch.randn(7, 3, 3, generator=gen), torch.randn(7, 1, 3, generator=gen)

    def run(dev):
        v = view.to(dev).clone().requires_grad_(True)
        rot, trans = get_transform_matrices(v)
        ((rot * w_r.to(dev)).sum() + (trans * w_t.to(dev)).sum()).backward()
        return rot.detach().cpu(), trans.detach().cpu(), v.grad.cpu()

    (ra, ta, ga), (rb, tb, gb) = run("cuda"), run("cpu")
    assert ra.shape == (7, 3, 3) and ta.shape == (7, 1, 3)
    assert torch.allclose(ra, rb, atol=2e-6) and torch.equal(ta, tb)
    assert torch.allclose(ga, gb, rtol=1e-5, atol=2e-6)
    with pytest.raises(ValueError):
        get_transform_matrices(torch.zeros(2, 4, device="cuda"))


def test_fit_objective_inside_the_rendering_node_large_faces():
    """The same comparison on a mesh of a few screen-filling triangles: their bounding boxes exceed the gathered
    pass's limit, so the texture / depth gradients go through the per-pixel fallback kernels, which must apply the
    scalar factors of the unscaled gradient maps too."""
    nr = _nr()
    from deep3dmap_amd.core import multiview_fit_loss
    v = np.array([[-0.9, -0.8, 0.1], [0.9, -0.7, -0.1], [0.0, 0.9, 0.2], [0.8, 0.8, -0.2], [-0.8, 0.7, 0.0]], np.float32)
    tri = np.array([[0, 1, 2], [1, 3, 2], [0, 2, 4]], np.int32)
    tex = np.random.default_rng(5).uniform(0.1, 1, (3, 2, 2, 2, 3)).astype(np.float32)
    r = nr.Renderer(image_size=96, anti_aliasing=False, camera_mode="look_at", fill_back=True)
    r.eye = torch.tensor([[0.3, 0.2, -2.2], [-0.4, 0.5, -2.0]], device="cuda")
    tri_d = torch.from_numpy(tri).cuda()[None]
    with torch.no_grad():
        rgb_t, depth_t, alpha_t = r(torch.from_numpy(v * 0.93).cuda()[None], tri_d, torch.from_numpy(tex).cuda()[None])

    def run(inside):
        vv = torch.from_numpy(v).cuda().requires_grad_(True)
        tt = torch.from_numpy(tex).cuda().requires_grad_(True)
        if inside:
            loss = r.render_fit_loss(vv[None], tri_d, tt[None], (rgb_t, depth_t, alpha_t, alpha_t))
        else:
            loss = multiview_fit_loss(*r(vv[None], tri_d, tt[None]), rgb_t, depth_t, alpha_t, alpha_t)
        (loss * 0.5).backward()
        return loss.detach(), vv.grad, tt.grad

    a, b = run(True), run(False)
    assert torch.allclose(a[0], b[0], rtol=2e-6)
    for ga, gb in zip(a[1:], b[1:]):
        assert float(gb.abs().max()) > 0
        assert float((ga - gb).abs().max()) <= 2e-5 * float(gb.abs().max())


@pytest.mark.parametrize("size", [40, 160])
@pytest.mark.parametrize("ts", [1, 2, 3, 4])
@pytest.mark.parametrize("shared", [False, True])
def test_on_the_fly_lighting_matches_materialised_path(ts, shared, size):
    """render() with fill_back + lighting applied inside the sampler (shared or per-view mesh/textures) against the
    reference's sequence cat -> lighting -> rasterize on materialised arrays: same images, same gradients.  At 160^2 the
    242-triangle mesh is COARSE (more than 48 raster pixels per triangle): a wave per face in the gathered passes of
    every texture size (k_backward_textures_lit_faces<64>, k_backward_textures_lit_faces_any<64>)."""
    nr = _nr()
    from deep3dmap_amd import synthetic
    v, tri = synthetic.grid_mesh(12)
    tex = synthetic.random_textures(tri.shape[0], ts)
    eyes = torch.from_numpy(synthetic.camera_ring(3)).cuda()
    B = 3
    res = []
    for fly in (False, True):
        r = nr.Renderer(image_size=size, anti_aliasing=False, camera_mode="look_at", light_direction=[0.3, 0.8, -0.5],
                        background_color=[0.1, 0.2, 0.3])
        r.eye = eyes
        r.lighting_on_the_fly = fly
        use_shared = shared and fly
        vv = torch.from_numpy(v).cuda()[None].repeat(1 if use_shared else B, 1, 1).requires_grad_(True)
        tt = torch.from_numpy(tex).cuda()[None].repeat(1 if use_shared else B, 1, 1, 1, 1, 1).requires_grad_(True)
        ff = torch.from_numpy(tri).cuda()[None].repeat(1 if use_shared else B, 1, 1)
        rgb, depth, alpha = r(vv, ff, tt)
        w = torch.linspace(0.5, 1.5, rgb.numel(), device="cuda").view_as(rgb)
        ((rgb * w).sum() + alpha.sum() + depth.clamp(max=5).sum()).backward()
        gv = vv.grad if vv.shape[0] == 1 else vv.grad.sum(0, keepdim=True)
        gt = tt.grad if tt.shape[0] == 1 else tt.grad.sum(0, keepdim=True)
        res.append((rgb.detach(), depth.detach(), alpha.detach(), gv, gt))
    a, b = res
    assert torch.equal(a[2], b[2]) and torch.equal(a[1], b[1])
    assert torch.allclose(a[0], b[0], rtol=0, atol=1e-6)
    assert float((a[4] - b[4]).abs().max()) <= 1e-3 * max(1.0, float(a[4].abs().max()))
    assert float((a[3] - b[3]).abs().max()) <= 1e-3 * max(1.0, float(a[3].abs().max()))


def test_obj_round_trip_tetrahedron(tmp_path):
    """tests/test_load_obj.py:15-37 and tests/test_save_obj.py on a tetrahedron written by this test (the
    reference's tests/data directory is not in its tree): load with and without normalisation, save, reload,
    and render the loaded mesh."""
    nr = _nr()
    vertices_ref = np.array([[1., 0., 0.], [0., 1., 0.], [0., 0., 1.], [0., 0., 0.]], 'float32')
    faces_ref = np.array([[1, 3, 2], [3, 1, 0], [2, 0, 1], [0, 2, 3]], 'int32')
    path = tmp_path / "tetrahedron.obj"
    path.write_text("# tetrahedron\n" + "".join("v %g %g %g\n" % tuple(v) for v in vertices_ref) +
                    "".join("f %d/1/1 %d/2/2 %d/3/3\n" % tuple(f + 1) for f in faces_ref))
    vertices, faces = nr.load_obj(str(path), False)
    assert torch.allclose(torch.from_numpy(vertices_ref).cuda(), vertices) and torch.equal(torch.from_numpy(faces_ref).cuda(), faces)
    vertices, faces = nr.load_obj(str(path), True)
    assert torch.allclose(torch.from_numpy(vertices_ref).cuda() * 2 - 1.0, vertices)
    out = tmp_path / "out.obj"
    nr.save_obj(str(out), vertices, faces)
    v2, f2 = nr.load_obj(str(out), False)
    assert torch.allclose(v2, vertices, atol=1e-6) and torch.equal(f2, faces)
    quad = tmp_path / "quad.obj"                      # polygons are fanned into triangles
    quad.write_text("v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nf 1 2 3 4\n")
    _, fq = nr.load_obj(str(quad), False)
    assert fq.cpu().tolist() == [[0, 1, 2], [0, 2, 3]]
    mesh = nr.Mesh.fromobj(str(path), texture_size=2)
    assert mesh.num_faces == 4 and mesh.textures.shape == (4, 2, 2, 2, 3)
    r = nr.Renderer(camera_mode="look_at", image_size=32)
    sil = r(mesh.vertices[None], mesh.faces[None], mode="silhouettes")
    assert sil.shape == (1, 32, 32) and 0.01 < float(sil.mean()) < 0.9
    with pytest.raises(Exception, match="Failed to load textures"):      # no mtllib line (load_obj.py:150-151)
        nr.load_obj(str(path), load_texture=True)


def test_fit_objective_with_frozen_textures_and_ambient_light_only():
    """render_fit_loss when neither the textures nor the light need a gradient (textures frozen, directional intensity
    0): the depth term then goes through d3m_backward_depth_map on its own, whose gradient map must carry the
    objective's 1 / sum(mask) like every other reader -- against the materialised objective on the same renderer."""
    from deep3dmap_amd import synthetic
    from deep3dmap_amd.multiview import MultiViewFit
    v, tri = synthetic.grid_mesh(16)
    tex = synthetic.random_textures(tri.shape[0], 2)
    res = []
    for inside in (True, False):
        fit = MultiViewFit(v, tri, tex, synthetic.camera_ring(3), image_size=64, optimise_textures=False,
                           objective_in_renderer=inside)
        fit.renderer.light_intensity_directional = 0.0
        fit.renderer.light_intensity_ambient = 1.0
        fit.set_targets_from(synthetic.perturb(v, 0.03))
        loss, gv, gt = fit.step()
        assert gt is None
        res.append((float(loss), gv.clone()))
    (la, ga), (lb, gb) = res
    assert abs(la - lb) <= 1e-5 * abs(lb) and float(gb.abs().max()) > 0
    assert _rel_max(ga, gb) < 1e-4


def test_per_batch_lights_fall_back_to_the_materialised_sequence():
    """NR/lighting.py:25-30 accepts one colour / direction per batch entry; the fused sampler takes one light, so such
    renderers go through cat -> lighting -> rasterize, against the oracle."""
    nr = _nr()
    from oracle import nr_oracle as O
    v, tri, tex = _scene()
    ca = torch.tensor([[1.0, 0.9, 0.8], [0.6, 0.7, 1.0]])
    dr = torch.tensor([[0.0, 1.0, 0.0], [0.5, 0.5, -0.7]])
    outs = []
    for mod, dev in ((O, "cpu"), (nr, "cuda")):
        r = mod.Renderer(camera_mode="look_at", image_size=40, anti_aliasing=False, light_color_ambient=ca.to(dev),
                         light_direction=dr.to(dev))
        vv = v.clone().to(dev).requires_grad_(True)
        rgb = r(vv, tri.to(dev), tex.to(dev), mode="rgb")
        rgb.square().sum().backward()
        outs.append((rgb.detach().cpu(), vv.grad.cpu()))
    assert _rel_max(outs[1][0], outs[0][0]) < IMG_TOL * 5 and _rel_max(outs[1][1], outs[0][1]) < GRAD_TOL


def test_losses_refuse_gradients_they_do_not_compute():
    from deep3dmap_amd.core import photometric_loss, silhouette_loss
    a = torch.rand(1, 3, 8, 8, device="cuda", requires_grad=True)
    b = torch.rand(1, 3, 8, 8, device="cuda", requires_grad=True)
    sig = torch.rand(1, 1, 8, 8, device="cuda", requires_grad=True)
    with pytest.raises(NotImplementedError):
        photometric_loss(a, b)
    with pytest.raises(NotImplementedError):
        photometric_loss(a, b.detach(), conf_sigma=sig)
    with pytest.raises(NotImplementedError):
        silhouette_loss(a[:, 0], b[:, 0])
    photometric_loss(a, b.detach(), conf_sigma=sig.detach()).backward()
    assert a.grad is not None


def test_fit_objective_can_leave_the_images_behind():
    """render_fit_loss(images_out=...): the pass that evaluates the objective also writes the images render() returns
    (bit for bit), and value and gradients of the objective do not change."""
    from deep3dmap_amd import synthetic
    from deep3dmap_amd.multiview import MultiViewFit
    v, tri = synthetic.grid_mesh(18)
    tex = synthetic.random_textures(tri.shape[0], 2)
    fit = MultiViewFit(v, tri, tex, synthetic.camera_ring(3), image_size=64)
    fit.set_targets_from(synthetic.perturb(v, 0.03))
    loss0, gv0, gt0 = (t.clone() for t in fit.step())
    fit.keep_images = True
    loss1, gv1, gt1 = fit.step()
    assert float(loss0) == float(loss1) and _rel_max(gv1, gv0) < 1e-5 and _rel_max(gt1, gt0) < 1e-5
    with torch.no_grad():
        rgb, depth, alpha = fit.render()
    for got, ref in zip(fit.images, (rgb, depth, alpha)):
        assert torch.equal(got, ref)


def test_dropin_render_plus_fit_loss_takes_the_records_route():
    """The reference-shaped composition -- images = Renderer.render(...) (NR/renderer.py:200-246), then
    multiview_fit_loss(images, targets) -- under autograd: the loss node finds that its three images are the outputs of
    one lit render node, evaluates the objective and leaves its gradient as the edge gradient's per-pixel records in ONE
    pass (k_fit_loss_records), and backward runs without gradient images (no k_fit_loss_grad, no k_pack_maps).  Images
    bit-equal to render(), loss and gradients equal to Renderer.render_fit_loss (the fused objective) and to the plain
    loss node on detached copies of the images."""
    from conftest import kernels_launched
    from deep3dmap_amd import synthetic
    from deep3dmap_amd.core.losses import _MultiViewFitLoss, multiview_fit_loss
    from deep3dmap_amd.multiview import MultiViewFit
    v, tri = synthetic.grid_mesh(20)
    tex = synthetic.random_textures(tri.shape[0], 2)
    fit = MultiViewFit(v, tri, tex, synthetic.camera_ring(4), image_size=96)
    fit.set_targets_from(synthetic.perturb(v, 0.03))
    loss0, gv0, gt0 = (t.clone() for t in fit.step())                # the fused objective (render_fit_loss)
    rgb_t, depth_t, alpha_t = fit.targets
    with torch.no_grad():
        ref_images = fit.render()
    fit.vertices.grad = fit.textures.grad = None
    with kernels_launched() as k:
        rgb, depth, alpha = fit.render()
        loss = multiview_fit_loss(rgb, depth, alpha, rgb_t, depth_t, alpha_t, alpha_t, fit.mask_sum)
        loss.backward()
    assert "k_fit_loss_records" in k.names and not ({"k_fit_loss_grad", "k_fit_loss_reduce", "k_pack_maps"} & k.names), sorted(k.names)
    for got, ref in zip((rgb, depth, alpha), ref_images):
        assert torch.equal(got.detach(), ref)
    assert abs(float(loss) - float(loss0)) <= 1e-6 * abs(float(loss0))
    assert _rel_max(fit.vertices.grad, gv0) < 1e-5 and _rel_max(fit.textures.grad, gt0) < 1e-5
    # a scaled loss (the scalar gradient travels through the link) and a second backward over the same graph
    fit.vertices.grad = fit.textures.grad = None
    rgb, depth, alpha = fit.render()
    loss = multiview_fit_loss(rgb, depth, alpha, rgb_t, depth_t, alpha_t, alpha_t, fit.mask_sum)
    (loss * 2.5).backward(retain_graph=True)
    assert _rel_max(fit.vertices.grad, 2.5 * gv0) < 1e-5 and _rel_max(fit.textures.grad, 2.5 * gt0) < 1e-5
    fit.vertices.grad = fit.textures.grad = None
    loss.backward()
    assert _rel_max(fit.vertices.grad, gv0) < 1e-5 and _rel_max(fit.textures.grad, gt0) < 1e-5
    # a NEGATIVE gradient of the loss: the edge gradient is not linear in it (a pixel counts iff its diff_grad > 0,
    # KCU:401/:481), so the comparison is with the plain loss node on gradient images
    neg = []
    for linked in (True, False):
        fit.vertices.grad = fit.textures.grad = None
        rgb, depth, alpha = fit.render()
        node = multiview_fit_loss if linked else (lambda *a: _MultiViewFitLoss.apply(*a))
        (node(rgb, depth, alpha, rgb_t, depth_t, alpha_t, alpha_t, fit.mask_sum) * -1.5).backward()
        neg.append((fit.vertices.grad.clone(), fit.textures.grad.clone()))
    assert _rel_max(neg[0][0], neg[1][0]) < 1e-5 and _rel_max(neg[0][1], neg[1][1]) < 1e-5
    assert _rel_max(neg[0][0], -1.5 * gv0) > 1e-2
    # ANOTHER consumer of the images beside the objective: the objective's gradient images are materialised after all
    # and added to the other's (same result as the plain loss node + the other term on one graph)
    w = torch.randn_like(rgb_t)
    grads = []
    for linked in (True, False):
        fit.vertices.grad = fit.textures.grad = None
        rgb, depth, alpha = fit.render()
        node = multiview_fit_loss if linked else (lambda *a: _MultiViewFitLoss.apply(*a))
        total = node(rgb, depth, alpha, rgb_t, depth_t, alpha_t, alpha_t, fit.mask_sum) + (rgb * w).mean() + depth.clamp(max=4).mean()
        total.backward()
        grads.append((fit.vertices.grad.clone(), fit.textures.grad.clone()))
    assert _rel_max(grads[0][0], grads[1][0]) < 1e-5 and _rel_max(grads[0][1], grads[1][1]) < 1e-5
    # the other consumer ALONE, after an objective was linked and never back-propagated: nothing of it may leak in
    fit.vertices.grad = fit.textures.grad = None
    rgb, depth, alpha = fit.render()
    multiview_fit_loss(rgb, depth, alpha, rgb_t, depth_t, alpha_t, alpha_t, fit.mask_sum)
    (rgb * w).mean().backward()
    only = fit.vertices.grad.clone()
    fit.vertices.grad = fit.textures.grad = None
    rgb, depth, alpha = fit.render()
    (rgb * w).mean().backward()
    assert _rel_max(only, fit.vertices.grad) < 1e-5
    # the captured drop-in step (MultiViewFit(objective_in_renderer=False)) replays the same numbers
    fit2 = MultiViewFit(v, tri, tex, synthetic.camera_ring(4), image_size=96, objective_in_renderer=False)
    fit2.targets, fit2.mask_sum, fit2._mask_sum_local = fit.targets, fit.mask_sum, fit._mask_sum_local
    fit2.capture_graph()
    for _ in range(3):
        loss2, gv2, gt2 = fit2.step()
    assert abs(float(loss2) - float(loss0)) <= 1e-6 * abs(float(loss0)) and _rel_max(gv2, gv0) < 1e-5 and _rel_max(gt2, gt0) < 1e-5
    fit2.release_graph()


def test_linked_fit_loss_with_observed_image_gradients():
    """the linked objective returns zero-stride ZERO gradient images and sends the real gradient through the
    link -- so nobody may be looking at those images' gradients.  retain_grad() / register_hook (before OR after the loss
    is built) get the objective's real gradient images; torch.autograd.grad(loss, rgb) -- a pass that stops at the images --
    fails loudly instead of returning zeros, needs link=False, and leaves NOTHING behind for a later backward through
    the render node."""
    from deep3dmap_amd import synthetic
    from deep3dmap_amd.core.losses import _MultiViewFitLoss, multiview_fit_loss
    from deep3dmap_amd.multiview import MultiViewFit
    v, tri = synthetic.grid_mesh(16)
    tex = synthetic.random_textures(tri.shape[0], 2)
    fit = MultiViewFit(v, tri, tex, synthetic.camera_ring(3), image_size=64)
    fit.set_targets_from(synthetic.perturb(v, 0.03))
    rgb_t, depth_t, alpha_t = fit.targets
    args = (rgb_t, depth_t, alpha_t, alpha_t, fit.mask_sum)

    def reference():
        fit.vertices.grad = fit.textures.grad = None
        rgb, depth, alpha = fit.render()
        for t in (rgb, depth, alpha):
            t.retain_grad()
        _MultiViewFitLoss.apply(rgb, depth, alpha, *args).backward()
        return [t.grad.clone() for t in (rgb, depth, alpha)], fit.vertices.grad.clone(), fit.textures.grad.clone()
    g_img, gv0, gt0 = reference()
    assert all(float(g.abs().max()) > 0 for g in g_img)

    # retain_grad BEFORE the loss is built: no link, real gradient images
    fit.vertices.grad = fit.textures.grad = None
    rgb, depth, alpha = fit.render()
    rgb.retain_grad()
    multiview_fit_loss(rgb, depth, alpha, *args).backward()
    assert _rel_max(rgb.grad, g_img[0]) < 1e-6 and _rel_max(fit.vertices.grad, gv0) < 1e-5

    # retain_grad / a hook AFTER the loss is built (the link exists): the loss node's backward hands out real images
    for observe in ("retain", "hook"):
        fit.vertices.grad = fit.textures.grad = None
        rgb, depth, alpha = fit.render()
        loss = multiview_fit_loss(rgb, depth, alpha, *args)
        seen = []
        if observe == "retain":
            depth.retain_grad()
        else:
            depth.register_hook(lambda g: seen.append(g.clone()))
        loss.backward()
        got = depth.grad if observe == "retain" else seen[0]
        assert _rel_max(got, g_img[1]) < 1e-6, observe
        assert _rel_max(fit.vertices.grad, gv0) < 1e-5 and _rel_max(fit.textures.grad, gt0) < 1e-5, observe

    # a pass that stops at the images: loud, not zeros; link=False is the way; and the next backward is clean
    w = torch.randn_like(rgb_t)
    fit.vertices.grad = fit.textures.grad = None
    rgb, depth, alpha = fit.render()
    loss = multiview_fit_loss(rgb, depth, alpha, *args)
    with pytest.raises(RuntimeError, match="link=False"):
        torch.autograd.grad(loss, rgb, retain_graph=True)
    (rgb * w).mean().backward()                    # unrelated to the objective: nothing of it may be added
    polluted = fit.vertices.grad.clone()
    fit.vertices.grad = fit.textures.grad = None
    rgb, depth, alpha = fit.render()
    (rgb * w).mean().backward()
    assert _rel_max(polluted, fit.vertices.grad) < 1e-5
    rgb, depth, alpha = fit.render()
    (g,) = torch.autograd.grad(multiview_fit_loss(rgb, depth, alpha, *args, link=False), rgb)
    assert _rel_max(g, g_img[0]) < 1e-6


@pytest.mark.parametrize("aa", [False, True])
def test_registered_objective_rides_in_the_render_pass(aa):
    """the reference-shaped composition with the objective REGISTERED on the renderer (Renderer.fit_targets):
    render() returns the same images bit for bit, the pass that writes them has evaluated the objective and left walk
    records, and multiview_fit_loss on those images with those targets launches NOTHING (no k_fit_loss_records) -- value
    and gradients equal to the fused objective; other targets, other consumers and observed image gradients fall back to
    the ordinary routes and stay correct."""
    from conftest import kernels_launched
    from deep3dmap_amd import synthetic
    from deep3dmap_amd.core.losses import _MultiViewFitLoss, multiview_fit_loss
    from deep3dmap_amd.multiview import MultiViewFit
    v, tri = synthetic.grid_mesh(20)
    tex = synthetic.random_textures(tri.shape[0], 2)
    fit = MultiViewFit(v, tri, tex, synthetic.camera_ring(4), image_size=96, anti_aliasing=aa)     # (aa: the pooled records)
    fit.set_targets_from(synthetic.perturb(v, 0.03))
    loss0, gv0, gt0 = (t.clone() for t in fit.step())                # the fused objective (render_fit_loss)
    rgb_t, depth_t, alpha_t = fit.targets
    args = (rgb_t, depth_t, alpha_t, alpha_t, fit.mask_sum)
    with torch.no_grad():
        ref_images = fit.render()
    r = fit.renderer

    def render_registered():
        fit.vertices.grad = fit.textures.grad = None
        r.fit_targets = args
        try:
            return r(fit.vertices[None], fit.triangles[None], fit.textures[None])
        finally:
            r.fit_targets = None

    with kernels_launched() as k:
        rgb, depth, alpha = render_registered()
        loss = multiview_fit_loss(rgb, depth, alpha, *args)
        loss.backward()
    assert "k_render_lit_fit_records" in k.names and not ({"k_fit_loss_records", "k_fit_loss_grad", "k_pack_maps"} & k.names), sorted(k.names)
    for got, ref in zip((rgb, depth, alpha), ref_images):
        assert torch.equal(got.detach(), ref)
    assert abs(float(loss.detach()) - float(loss0)) <= 1e-6 * abs(float(loss0))
    assert _rel_max(fit.vertices.grad, gv0) < 1e-5 and _rel_max(fit.textures.grad, gt0) < 1e-5
    # OTHER targets than the registered ones: the ordinary linked objective (its own pass over the images)
    other = (rgb_t * 0.5, depth_t, alpha_t, alpha_t, fit.mask_sum)
    grads = []
    for registered in (True, False):
        if registered:
            rgb, depth, alpha = render_registered()
        else:
            fit.vertices.grad = fit.textures.grad = None
            rgb, depth, alpha = fit.render()
        multiview_fit_loss(rgb, depth, alpha, *other).backward()
        grads.append((fit.vertices.grad.clone(), fit.textures.grad.clone()))
    assert _rel_max(grads[0][0], grads[1][0]) < 1e-5 and _rel_max(grads[0][1], grads[1][1]) < 1e-5
    # another consumer beside the objective, and an observed image gradient: gradient images after all
    w = torch.randn_like(rgb_t)
    fit.vertices.grad = fit.textures.grad = None
    rgb, depth, alpha = fit.render()
    (_MultiViewFitLoss.apply(rgb, depth, alpha, *args) + (rgb * w).mean()).backward()
    want = (fit.vertices.grad.clone(), fit.textures.grad.clone())
    rgb, depth, alpha = render_registered()
    (multiview_fit_loss(rgb, depth, alpha, *args) + (rgb * w).mean()).backward()
    assert _rel_max(fit.vertices.grad, want[0]) < 1e-5 and _rel_max(fit.textures.grad, want[1]) < 1e-5
    rgb, depth, alpha = render_registered()
    loss = multiview_fit_loss(rgb, depth, alpha, *args)
    depth.retain_grad()
    loss.backward()
    assert float(depth.grad.abs().max()) > 0 and _rel_max(fit.vertices.grad, gv0) < 1e-5
    # the images alone, objective registered and never asked for: ordinary image gradients
    rgb, depth, alpha = render_registered()
    (rgb * w).mean().backward()
    only = fit.vertices.grad.clone()
    fit.vertices.grad = fit.textures.grad = None
    rgb, depth, alpha = fit.render()
    (rgb * w).mean().backward()
    assert _rel_max(only, fit.vertices.grad) < 1e-5


@pytest.mark.parametrize("mode", ["silhouettes", "depth"])
@pytest.mark.parametrize("aa", [False, True])
@pytest.mark.parametrize("per_view_mesh", [False, True])
def test_silhouette_and_depth_modes_over_the_indexed_mesh(mode, aa, per_view_mesh, coverage):
    """Renderer.render_silhouettes / render_depth (NR/renderer.py:114-183) with a look_at camera run as ONE node over the
    indexed mesh (rasterize._RasterizeMeshModes: camera inside, coverage through the index tensor, K4 / K6 straight into the
    vertices' gradient) -- against the reference's operator sequence, which the same Renderer runs with mesh_modes off
    (look_at -> vertices_to_faces -> rasterize_* -> scatter-add; itself pinned to the oracle by the tests above): images bit
    for bit, vertex gradients to the order of their float atomics; no gather / scatter pass in the new step.  Both forms of coverage."""
    from conftest import kernels_launched
    from deep3dmap_amd import neural_renderer as nr, synthetic
    v_np, tri_np = synthetic.grid_mesh(24)
    B = 3
    eyes = torch.from_numpy(synthetic.camera_ring(B)).float().cuda()
    tri = torch.from_numpy(tri_np).int().cuda()[None]
    base = torch.from_numpy(v_np).float().cuda()[None]
    if per_view_mesh:
        base = base.repeat(B, 1, 1) * torch.linspace(0.9, 1.1, B, device="cuda")[:, None, None]
        tri = tri.repeat(B, 1, 1)
    gen = torch.Generator(device="cuda").manual_seed(3)
    out = {}
    for on in (True, False):
        r = nr.Renderer(image_size=64, anti_aliasing=aa, camera_mode="look_at", fill_back=True)
        r.eye, r.mesh_modes = eyes, on
        v = base.clone().requires_grad_(True)
        with kernels_launched() as k:
            image = getattr(r, "render_" + mode)(v, tri)
            if on:
                w = torch.rand(image.shape, device="cuda", generator=gen) - 0.3
            (image * w).sum().backward(retain_graph=on)
        out[on] = (image.detach(), v.grad.clone(), set(k.names))
        if on:      # a second backward over the same graph (the first used the accumulator the forward pass had zeroed)
            v.grad = None
            (image * w).sum().backward()
            assert float((v.grad - out[on][1]).abs().max()) <= 2e-5 * float(v.grad.abs().max())
    assert out[True][0].shape == (B, 64, 64) and torch.equal(out[True][0], out[False][0])
    assert 0.05 < float((out[True][0] > 0).float().mean()) < 1.0 if mode == "silhouettes" else True
    g1, g0 = out[True][1], out[False][1]
    assert float(g0.abs().max()) > 0 and float((g1 - g0).abs().max()) <= 2e-5 * float(g0.abs().max())
    assert {"k_gather_faces", "k_scatter_face_grads", "k_mark_visible"} & out[False][2]
    assert not ({"k_gather_faces", "k_scatter_face_grads", "k_mark_visible", "k_output_epilogue_backward"} & out[True][2]) \
        or mode == "depth", sorted(out[True][2])
    assert not ({"k_gather_faces", "k_scatter_face_grads", "k_mark_visible"} & out[True][2]), sorted(out[True][2])
    if mode == "silhouettes":      # round 6: the walks read the image's gradient where it is -- no pass packing records
        assert "k_pack_maps" not in out[True][2] and "k_pack_maps" not in out[False][2], sorted(out[True][2])


def _projection_camera(size, batch):
    fx = 1.25 * size
    K = torch.tensor([[fx, 0.0, size / 2.0], [0.0, fx, size / 2.0], [0.0, 0.0, 1.0]], device="cuda")[None]
    ang = torch.linspace(-0.4, 0.4, batch)
    R = torch.stack([torch.tensor([[float(torch.cos(a)), 0.0, float(torch.sin(a))], [0.0, 1.0, 0.0],
                                   [-float(torch.sin(a)), 0.0, float(torch.cos(a))]]) for a in ang]).cuda()
    t = torch.tensor([[0.05, -0.02, 2.8]], device="cuda").repeat(batch, 1)[:, None, :]
    dist = torch.tensor([[0.05, 0.01, 0.001, -0.002, 0.0]], device="cuda")
    return dict(K=K, R=R, t=t, dist_coeffs=dist, orig_size=size)


@pytest.mark.parametrize("camera_mode", ["look", "projection"])
def test_look_and_projection_cameras_run_inside_the_render_nodes(camera_mode):
    """Round 5: not only look_at -- `look` and `projection` cameras with constant parameters also run inside the render
    nodes (Renderer._camera_in_node: the lit node of render / render_rgb / render_fit_loss and the mesh node of
    render_silhouettes / render_depth).  Against the same Renderer driven the reference's way (camera transform as a node of
    its own, NR/renderer.py:88-112, then the rasterizer on the transformed vertices): images bit for bit, gradients to the
    order of their float atomics."""
    from deep3dmap_amd import neural_renderer as nr, synthetic
    from deep3dmap_amd.neural_renderer.rasterize import rasterize_lit
    v_np, tri_np = synthetic.grid_mesh(20)
    B, size = 3, 64
    tri = torch.from_numpy(tri_np).int().cuda()[None]
    tex = torch.from_numpy(synthetic.random_textures(tri_np.shape[0], 2)).float().cuda()[None]
    r = nr.Renderer(image_size=size, anti_aliasing=False, camera_mode=camera_mode, fill_back=True)
    kw = {}
    if camera_mode == "look":
        r.eye = torch.from_numpy(synthetic.camera_ring(B)).float().cuda()
        r.camera_direction = (-r.eye / r.eye.norm(dim=1, keepdim=True)).contiguous()
    else:
        kw = _projection_camera(size, B)
    assert r._camera_in_node(torch.zeros(1, 4, 3, device="cuda"), **kw) is not None
    gen = torch.Generator(device="cuda").manual_seed(11)
    # silhouettes and depth: the mesh node against the operator sequence
    for mode in ("silhouettes", "depth"):
        res = []
        for on in (True, False):
            r.mesh_modes = on
            v = torch.from_numpy(v_np).float().cuda()[None].requires_grad_(True)
            image = getattr(r, "render_" + mode)(v, tri, **kw)
            if on:
                w = torch.rand(image.shape, device="cuda", generator=gen) - 0.3
            (image * w).sum().backward()
            res.append((image.detach(), v.grad.clone()))
        assert torch.equal(res[0][0], res[1][0]) and float((res[0][0] != res[0][0][0, 0, 0]).float().mean()) > 0.02
        assert float((res[0][1] - res[1][1]).abs().max()) <= 2e-5 * float(res[1][1].abs().max()) > 0
    # render(): the lit node with the camera inside against the lit node behind the camera's own node
    v = torch.from_numpy(v_np).float().cuda()[None].requires_grad_(True)
    t1 = tex.clone().requires_grad_(True)
    rgb, depth, alpha = r.render(v, tri, t1, **kw)
    w3 = torch.rand(rgb.shape, device="cuda", generator=gen)
    (rgb * w3).sum().backward()
    v2 = torch.from_numpy(v_np).float().cuda()[None].requires_grad_(True)
    t2 = tex.clone().requires_grad_(True)
    sv = r._transform(v2, kw.get("K"), kw.get("R"), kw.get("t"), kw.get("dist_coeffs"), kw.get("orig_size"))
    out = rasterize_lit(sv, v2, tri, t2, r._light_cfg(), r.fill_back, r.image_size, r.anti_aliasing, r.near, r.far,
                        r.rasterizer_eps, r.background_color)
    (out["rgb"] * w3).sum().backward()
    assert torch.equal(rgb.detach(), out["rgb"].detach()) and torch.equal(depth.detach(), out["depth"].detach())
    assert float((v.grad - v2.grad).abs().max()) <= 2e-5 * float(v2.grad.abs().max()) > 0
    assert float((t1.grad - t2.grad).abs().max()) <= 2e-5 * float(t2.grad.abs().max())


@pytest.mark.parametrize("mode", ["silhouettes", "depth"])
def test_mesh_modes_without_fill_back_and_without_gradients(mode):
    """The same node with fill_back off (front faces only) and under no_grad (no visibility list, no plan): images bit for
    bit as the operator sequence's, gradients equal where they are asked for."""
    from deep3dmap_amd import neural_renderer as nr, synthetic
    v_np, tri_np = synthetic.grid_mesh(24)
    eyes = torch.from_numpy(synthetic.camera_ring(3)).float().cuda()
    tri = torch.from_numpy(tri_np).int().cuda()[None]
    res = []
    for on in (True, False):
        r = nr.Renderer(image_size=48, anti_aliasing=True, camera_mode="look_at", fill_back=False)
        r.eye, r.mesh_modes = eyes, on
        v = torch.from_numpy(v_np).float().cuda()[None].requires_grad_(True)
        with torch.no_grad():
            plain = getattr(r, "render_" + mode)(v, tri)
        image = getattr(r, "render_" + mode)(v, tri)
        assert torch.equal(plain, image.detach())
        (image * image).sum().backward()
        res.append((image.detach(), v.grad.clone()))
    assert torch.equal(res[0][0], res[1][0])
    assert float((res[0][1] - res[1][1]).abs().max()) <= 2e-5 * float(res[1][1].abs().max()) > 0


@pytest.mark.parametrize("size,aa,views", [(37, False, 1), (33, True, 2), (130, False, 3), (65, True, 1)])
def test_silhouette_node_reads_the_image_gradient_in_place_at_odd_sizes(size, aa, views):
    """Round 6: the silhouette node's edge gradient reads the OUTPUT image's gradient where it is -- through the row flip and,
    with anti-aliasing, the 2x2 pooling's adjoint -- instead of packing per-pixel records (d3m_edge_grad.h "DIRECT";
    d3m_fit_targets.flags = D3M_GRAD_OF_OUTPUT_IMAGE [| D3M_FIT_POOLED]).  Image sizes that are odd, not a multiple of the
    staging loops' four pixels per thread, and above one round of the two-wave line kernel; a random (dense) gradient and a
    band-shaped one: against the reference's operator sequence (mesh_modes off: rasterize_silhouettes' own flip / pooling
    nodes in front of the reference-shaped K4)."""
    from deep3dmap_amd import neural_renderer as nr, synthetic
    v_np, tri_np = synthetic.grid_mesh(14)
    eyes = torch.from_numpy(synthetic.camera_ring(max(views, 2))[:views]).float().cuda()
    tri = torch.from_numpy(tri_np).int().cuda()[None]
    gen = torch.Generator(device="cuda").manual_seed(size)
    for kind in ("dense", "band"):
        res = []
        for on in (True, False):
            r = nr.Renderer(image_size=size, anti_aliasing=aa, camera_mode="look_at", fill_back=True)
            r.eye, r.mesh_modes = eyes, on
            v = torch.from_numpy(v_np).float().cuda()[None].requires_grad_(True)
            image = r.render_silhouettes(v, tri)
            if on:
                if kind == "dense":
                    w = torch.rand(image.shape, device="cuda", generator=gen) - 0.4
                else:       # the gradient of a squared error against a shifted silhouette: two thin bands
                    w = 2.0 * (image.detach() - torch.roll(image.detach(), shifts=(2, -3), dims=(1, 2))) / image[0].numel()
            (image * w).sum().backward()
            res.append((image.detach(), v.grad.clone()))
        assert res[0][0].shape == (views, size, size) and torch.equal(res[0][0], res[1][0])
        assert 0.02 < float((res[0][0] > 0).float().mean()) < 0.98
        scale = float(res[1][1].abs().max())
        assert scale > 0 and float((res[0][1] - res[1][1]).abs().max()) <= 2e-5 * scale, (kind, scale)


def test_mesh_depth_mode_with_large_faces():
    """Faces whose pixel box exceeds the gathered pass's limit are left to the per-pixel pass (counted, so that it leaves at
    once in the ordinary case): an 8-triangle mesh in a 384x384 image (boxes of ~7 000 pixels) takes that route in d3m_backward_depth_map_mesh --
    with the output image's gradient read through the flip -- and must agree with the operator sequence."""
    from conftest import kernels_launched
    from deep3dmap_amd import neural_renderer as nr, synthetic
    v_np, tri_np = synthetic.grid_mesh(3)
    eyes = torch.from_numpy(synthetic.camera_ring(2)).float().cuda()
    tri = torch.from_numpy(tri_np).int().cuda()[None]
    res = []
    for on in (True, False):
        r = nr.Renderer(image_size=384, anti_aliasing=False, camera_mode="look_at", fill_back=True)
        r.eye, r.mesh_modes = eyes, on
        v = torch.from_numpy(v_np).float().cuda()[None].requires_grad_(True)
        image = r.render_depth(v, tri)
        w = torch.linspace(0.2, 1.3, 384, device="cuda")[None, :, None] * torch.linspace(1.0, 0.5, 384, device="cuda")[None, None, :]
        (image.clamp(max=10) * w).sum().backward()
        res.append((image.detach(), v.grad.clone()))
    assert torch.equal(res[0][0], res[1][0])
    # the mean face owns more than 2 048 pixels, i.e. its box exceeds the limit of 4 096 (D3M_FM_MAX_BBOX_AREA)
    assert float((res[0][0] < 50).float().sum(dim=(1, 2)).min()) / 8 > 2048
    assert float((res[0][1] - res[1][1]).abs().max()) <= 2e-5 * float(res[1][1].abs().max()) > 0


@pytest.mark.parametrize("n,size", [(7, 96), (12, 160)])
def test_mesh_depth_mode_on_a_coarse_mesh(n, size):
    """More than 48 raster pixels per triangle: d3m_backward_depth_map_mesh gives a face a whole wave instead of eight lanes
    (k_backward_depth_faces<DenseFaces, 64>), the faces still below the box limit of the per-pixel pass.  Same gradient as
    the operator sequence's."""
    from deep3dmap_amd import neural_renderer as nr, synthetic
    v_np, tri_np = synthetic.grid_mesh(n)
    assert size * size > 48 * tri_np.shape[0]
    eyes = torch.from_numpy(synthetic.camera_ring(3)).float().cuda()
    tri = torch.from_numpy(tri_np).int().cuda()[None]
    res = []
    for on in (True, False):
        r = nr.Renderer(image_size=size, anti_aliasing=False, camera_mode="look_at", fill_back=True)
        r.eye, r.mesh_modes = eyes, on
        v = torch.from_numpy(v_np).float().cuda()[None].requires_grad_(True)
        image = r.render_depth(v, tri)
        w = torch.linspace(0.3, 1.1, size, device="cuda")[None, :, None] * torch.linspace(1.0, 0.4, size, device="cuda")[None, None, :]
        (image.clamp(max=10) * w).sum().backward()
        res.append((image.detach(), v.grad.clone()))
    assert torch.equal(res[0][0], res[1][0]) and float((res[0][0] < 50).float().mean()) > 0.05
    assert float((res[0][1] - res[1][1]).abs().max()) <= 2e-5 * float(res[1][1].abs().max()) > 0


@pytest.mark.parametrize("aa", [False, True])
def test_renderer_end_to_end_on_a_coarse_mesh_against_oracle(aa):
    """More than 48 raster pixels per triangle (72 triangles @48^2, or @96^2 with anti-aliasing): the gathered texture /
    depth pass gives a face a whole wave instead of eight lanes (k_backward_textures_lit_faces<64>), and small batches of
    such meshes take the per-tile lists.  Images, loss and both gradients against the oracle, as the test above."""
    nr = _nr()
    from oracle import nr_oracle as O
    v, tri, tex = _scene(n=7)
    assert 48 * 48 > 24 * tri.shape[1]
    kw = dict(image_size=48, anti_aliasing=aa, camera_mode="look_at", background_color=[0.2, 0.3, 0.4],
              light_direction=[0.3, 0.8, -0.5])
    ro, rg = O.Renderer(**kw), nr.Renderer(**kw)
    ro.eye = rg.eye = [0.6, 0.9, -2.3]
    gen = torch.Generator().manual_seed(5)
    targets = (torch.rand(2, 3, 48, 48, generator=gen), torch.rand(2, 48, 48, generator=gen), torch.rand(2, 48, 48, generator=gen))

    def run(renderer, dev):
        vv = v.detach().clone().to(dev).requires_grad_(True)
        tt = tex.detach().clone().to(dev).requires_grad_(True)
        rgb, depth, alpha = renderer(vv, tri.to(dev), tt)
        loss = ((rgb - targets[0].to(dev)) ** 2).sum() + ((alpha - targets[1].to(dev)) ** 2).sum() + \
               (depth.clamp(max=5.0) - targets[2].to(dev)).abs().sum() * 0.1
        loss.backward()
        return [x.detach().cpu() for x in (rgb, depth, alpha, loss, vv.grad, tt.grad)]

    with _association("product"):
        ref = run(ro, "cpu")
    got = run(rg, "cuda")
    _compare_end_to_end(ref, got, "product", f"coarse[aa={int(aa)}]")


def _needles(count):
    """`count` thin triangles, each the height of the image, side by side: at 1024^2 every one's pixel box exceeds the gathered
    passes' limit (5 x 1024 pixels), and half an image row crosses a hundred of them."""
    xs = np.linspace(-0.9, 0.9, count + 1).astype(np.float32)
    v = np.zeros((3 * count, 3), np.float32)
    for i in range(count):
        v[3 * i] = (xs[i], -0.9, 0.02 * (i % 5))
        v[3 * i + 1] = (xs[i + 1], -0.9, 0.02 * (i % 3))
        v[3 * i + 2] = (xs[i], 0.9, 0.01 * (i % 7))
    tri = np.arange(3 * count, dtype=np.int32).reshape(count, 3)
    return v, tri


def test_large_face_fallbacks_with_more_faces_than_a_workgroup_table_holds():
    """The per-pixel fallbacks of the gathered passes collect a workgroup's sums per face in a 64-slot LDS table (WgSums) and
    add the rest directly: 200 needle triangles @1024^2 are all over the box limit, and a workgroup's run of pixels crosses a
    hundred of them -- the table overflows in every workgroup (150 needles, each owning ~2 300 pixels in a box of ~5 000).  Depth mode against the operator sequence, and the lit
    render (textures, light, depth) against the materialised sequence."""
    nr = _nr()
    v_np, tri_np = _needles(150)
    tri = torch.from_numpy(tri_np).cuda()[None]
    eye = [0.0, 0.0, -1.9]
    res = []
    for on in (True, False):
        r = nr.Renderer(image_size=1024, anti_aliasing=False, camera_mode="look_at", fill_back=True)
        r.eye, r.mesh_modes = eye, on
        v = torch.from_numpy(v_np).cuda()[None].requires_grad_(True)
        image = r.render_depth(v, tri)
        w = torch.linspace(0.3, 1.2, 1024, device="cuda")[None, :, None] * torch.linspace(1.0, 0.5, 1024, device="cuda")[None, None, :]
        (image.clamp(max=10) * w).sum().backward()
        res.append((image.detach(), v.grad.clone()))
    assert torch.equal(res[0][0], res[1][0])
    covered = float((res[0][0] < 50).float().sum())
    assert 2 * covered / 150 > 4096, covered          # (a needle's box = twice its area: over the limit of 4 096 pixels)
    assert float((res[0][1] - res[1][1]).abs().max()) <= 5e-5 * float(res[1][1].abs().max()) > 0
    tex = torch.rand(1, tri_np.shape[0], 2, 2, 2, 3, device="cuda")
    out = []
    for fly in (True, False):
        r = nr.Renderer(image_size=1024, anti_aliasing=False, camera_mode="look_at", light_direction=[0.3, 0.8, -0.5])
        r.eye, r.lighting_on_the_fly = eye, fly
        vv = torch.from_numpy(v_np).cuda()[None].requires_grad_(True)
        tt = tex.clone().requires_grad_(True)
        rgb, depth, alpha = r(vv, tri, tt)
        w3 = torch.linspace(0.5, 1.5, 1024, device="cuda")[None, None, :, None]
        ((rgb * w3).sum() + depth.clamp(max=5).sum()).backward()
        out.append((rgb.detach(), vv.grad.clone(), tt.grad.clone()))
    assert torch.allclose(out[0][0], out[1][0], rtol=0, atol=1e-6)
    for k in (1, 2):
        assert float((out[0][k] - out[1][k]).abs().max()) <= 1e-3 * float(out[1][k].abs().max()) > 0


@pytest.mark.parametrize("route", ["render", "fit_loss"])
def test_texture_only_optimisation_skips_the_geometry_side(route):
    """with the camera inside the node, a mesh that wants no gradient (texture-only optimisation) used to pay for
    the whole geometry side -- screen-space accumulator, plan, line walk, K6, camera adjoint -- to produce a gradient
    autograd throws away.  Now: no k_edge_* launch at all, grad_vertices None, and the texture gradient equal to the one the
    full backward pass produces."""
    from conftest import kernels_launched
    from deep3dmap_amd import synthetic
    from deep3dmap_amd.core.losses import multiview_fit_loss
    from deep3dmap_amd.multiview import MultiViewFit
    v, tri = synthetic.grid_mesh(18)
    tex = synthetic.random_textures(tri.shape[0], 2)
    fit = MultiViewFit(v, tri, tex, synthetic.camera_ring(3), image_size=64, anti_aliasing=False)
    fit.set_targets_from(synthetic.perturb(v, 0.03))
    rgb_t, depth_t, alpha_t = fit.targets
    r = fit.renderer

    def run(vertices_grad):
        vtx = fit.vertices.detach().clone().requires_grad_(vertices_grad)
        txt = fit.textures.detach().clone().requires_grad_(True)
        with kernels_launched() as k:
            if route == "render":
                rgb, depth, alpha = r(vtx[None], fit.triangles[None], txt[None])
                loss = multiview_fit_loss(rgb, depth, alpha, rgb_t, depth_t, alpha_t, alpha_t)
            else:
                loss = r.render_fit_loss(vtx[None], fit.triangles[None], txt[None], (rgb_t, depth_t, alpha_t, alpha_t))
            loss.backward()
        return float(loss.detach()), vtx.grad, txt.grad, k.names

    loss_full, gv_full, gt_full, names_full = run(True)
    loss_tex, gv_tex, gt_tex, names_tex = run(False)
    assert gv_full is not None and gv_tex is None
    assert loss_tex == loss_full
    assert _rel_max(gt_tex, gt_full) < 1e-6
    assert "k_edge_lines" in names_full and "k_edge_scatter" in names_full
    geometry = {n for n in names_tex if n.startswith("k_edge_") or n.startswith("k_camera_backward") or n == "k_lit_back"}
    assert not geometry, sorted(names_tex)


def test_registered_objective_that_does_not_fit_the_call_is_ignored():
    """Renderer.fit_targets is sticky; a later render() with another batch or image size must not raise on it --
    the call is a plain render (and multiview_fit_loss on its images takes the ordinary routes).  And a registered objective
    WITH a global mask_sum is not silently used for a call that asks for the local normaliser (mask_sum=None)."""
    from conftest import kernels_launched
    from deep3dmap_amd import synthetic
    from deep3dmap_amd.core.losses import multiview_fit_loss
    from deep3dmap_amd.multiview import MultiViewFit
    v, tri = synthetic.grid_mesh(16)
    tex = synthetic.random_textures(tri.shape[0], 2)
    fit = MultiViewFit(v, tri, tex, synthetic.camera_ring(2), image_size=48, anti_aliasing=False)
    fit.set_targets_from(synthetic.perturb(v, 0.03))
    rgb_t, depth_t, alpha_t = fit.targets
    r = fit.renderer
    r.fit_targets = (rgb_t, depth_t, alpha_t, alpha_t, fit.mask_sum)
    try:
        with torch.no_grad():
            want = [t.clone() for t in r(fit.vertices[None], fit.triangles[None], fit.textures[None])]
        r.image_size = 32                                   # the registration no longer fits: ignored, not an error
        with kernels_launched() as k:
            small = r(fit.vertices[None], fit.triangles[None], fit.textures[None])
        assert tuple(small[0].shape) == (2, 3, 32, 32) and "k_render_lit_fit_records" not in k.names
        r.image_size = 48
        # the registered objective carries the GLOBAL normaliser (here: twice the local one)
        double = (fit.mask_sum * 2.0).reshape(1)
        r.fit_targets = (rgb_t, depth_t, alpha_t, alpha_t, double)
        fit.vertices.grad = fit.textures.grad = None
        rgb, depth, alpha = r(fit.vertices[None], fit.triangles[None], fit.textures[None])
        assert all(torch.equal(a.detach(), b) for a, b in zip((rgb, depth, alpha), want))
        local = multiview_fit_loss(rgb, depth, alpha, rgb_t, depth_t, alpha_t, alpha_t)         # mask_sum=None: sum(mask)
        glob = multiview_fit_loss(rgb, depth, alpha, rgb_t, depth_t, alpha_t, alpha_t, double)
    finally:
        r.fit_targets = None
    rgb2, depth2, alpha2 = fit.render()
    ref_local = multiview_fit_loss(rgb2, depth2, alpha2, rgb_t, depth_t, alpha_t, alpha_t, link=False)
    ref_glob = multiview_fit_loss(rgb2, depth2, alpha2, rgb_t, depth_t, alpha_t, alpha_t, double, link=False)
    assert abs(float(local) - float(ref_local)) <= 1e-6 * abs(float(ref_local))
    assert abs(float(glob) - float(ref_glob)) <= 1e-6 * abs(float(ref_glob))
    assert abs(float(ref_local) - float(ref_glob)) > 1e-3 * abs(float(ref_local))          # (the two really differ)


@pytest.mark.parametrize("scene", ["fine_mesh_32_views_graph", "coarse_mesh_large_faces", "anti_aliased_dropin"])
def test_deterministic_mode_is_bit_reproducible(scene):
    """d3m_set_deterministic(1) / D3M_DETERMINISTIC=1.  The default backward pass adds its vertex gradients
    with float atomics in arrival order: grad_vertices differs by ~1e-7 of its largest entry from run to run (an ascending
    visibility list alone does not change that -- measured in round 6: 1 of 12 runs bit-identical either way).  In the
    deterministic mode the lit render node produces every term per (view, face) and sums per vertex in a fixed order:
    loss, grad_vertices and grad_textures are BIT-identical over repeated steps -- eager and replayed from a HIP graph --
    and agree with the default mode to the order of its own spread."""
    from deep3dmap_amd import _lib, synthetic
    from deep3dmap_amd.core.losses import multiview_fit_loss
    from deep3dmap_amd.multiview import MultiViewFit
    if scene == "fine_mesh_32_views_graph":
        n, views, size, aa = 120, 32, 256, False
    elif scene == "coarse_mesh_large_faces":
        n, views, size, aa = 4, 3, 256, False            # 18 triangles filling a 256^2 raster: boxes far beyond 4096 pixels
    else:
        n, views, size, aa = 40, 4, 96, True
    v, tri = synthetic.grid_mesh(n)
    tex = synthetic.random_textures(tri.shape[0], 2)
    fit = MultiViewFit(v, tri, tex, synthetic.camera_ring(views), image_size=size, anti_aliasing=aa,
                       objective_in_renderer=scene != "anti_aliased_dropin")
    fit.set_targets_from(synthetic.perturb(v, 0.03))
    ref = [t.clone() for t in fit.step()]                # default mode
    runs = []
    with _lib.deterministic():
        assert _lib.lib().d3m_get_deterministic() == 1
        for _ in range(3):
            runs.append([t.clone() for t in fit.step()])
        if scene == "fine_mesh_32_views_graph":
            fit.capture_graph()
            for _ in range(3):
                runs.append([t.clone() for t in fit.step()])
            fit.release_graph()
    assert _lib.lib().d3m_get_deterministic() == 0
    for r in runs[1:]:
        for name, a, b in zip(("loss", "grad_vertices", "grad_textures"), r, runs[0]):
            assert torch.equal(a, b), (scene, name, float((a - b).abs().max()))
    assert float(runs[0][1].abs().max()) > 0 and float(runs[0][2].abs().max()) > 0
    assert abs(float(runs[0][0]) - float(ref[0])) <= 1e-6 * abs(float(ref[0]))
    assert _rel_max(runs[0][1], ref[1]) < 1e-5 and _rel_max(runs[0][2], ref[2]) < 1e-5


@pytest.mark.parametrize("aa", [False, True])
@pytest.mark.parametrize("mode,n", [("silhouettes", 60), ("depth", 60), ("depth", 4)])
def test_deterministic_mode_covers_the_silhouette_and_depth_nodes(mode, n, aa):
    """... and the silhouette / depth node (render_silhouettes, render_depth over one shared topology): K4 -- or K6, gathered
    per face whatever the face's size (n = 4: 18 triangles, boxes far beyond the gathered pass's usual limit) -- into a
    per-face array, summed per vertex over the index tensor's CSR adjacency: bit-identical gradients over repeated backward
    passes, eager and replayed from a HIP graph, and equal to the default mode's to the order of its float atomics."""
    from deep3dmap_amd import _lib, neural_renderer as nr, synthetic
    from deep3dmap_amd.graph import CapturedStep
    v_np, tri_np = synthetic.grid_mesh(n)
    B = 6
    r = nr.Renderer(image_size=128, anti_aliasing=aa, camera_mode="look_at", fill_back=True)
    r.eye = torch.from_numpy(synthetic.camera_ring(B)).float().cuda()
    tri = torch.from_numpy(tri_np).int().cuda()[None]
    v = torch.from_numpy(v_np).float().cuda()[None].requires_grad_(True)
    render = getattr(r, "render_" + mode)
    with torch.no_grad():
        target = torch.roll(render(v, tri), shifts=(3, -2), dims=(1, 2)).clamp(max=10.0)

    def step():
        v.grad = None
        ((render(v, tri).clamp(max=10.0) - target) ** 2).sum().backward()
        return v.grad

    ref = step().clone()
    default_runs = [step().clone() for _ in range(4)]
    with _lib.deterministic():
        runs = [step().clone() for _ in range(3)]
        captured = CapturedStep(step).capture()
        for _ in range(3):
            runs.append(captured().clone())
        torch.cuda.synchronize()
        captured.release()
    for g in runs[1:]:
        assert torch.equal(g, runs[0]), float((g - runs[0]).abs().max())
    assert float(ref.abs().max()) > 0 and _rel_max(runs[0], ref) < 1e-5
    assert all(_rel_max(g, ref) < 1e-5 for g in default_runs)


def test_deterministic_mode_refuses_what_it_does_not_cover():
    """... and the shapes its fixed-order sums do not cover (per-view index tensors, view groups) raise instead of silently
    running the unordered pass; the reference-shaped gather's adjoint (vertices_to_faces) is gathered in order too."""
    from deep3dmap_amd import _lib
    from deep3dmap_amd.neural_renderer import mesh_ops
    vs, tris, texs = (t.cuda() for t in _scene(B=2, n=10))          # faces of batch 2
    vs.requires_grad_(True)
    r = _nr().Renderer(camera_mode="look_at", image_size=32, anti_aliasing=False)
    r.eye = [0.3, 0.4, -2.5]
    with _lib.deterministic():
        with pytest.raises(NotImplementedError):
            r(vs, tris, texs)[0].sum().backward()
        grads = []
        for _ in range(3):
            vv = vs.detach()[:1].clone().requires_grad_(True)
            (mesh_ops.gather_faces(vv, tris[:1], True) * torch.linspace(0.5, 1.5, 9, device="cuda").view(3, 3)).sum().backward()
            grads.append(vv.grad.clone())
        assert torch.equal(grads[0], grads[1]) and torch.equal(grads[0], grads[2])
    vv = vs.detach()[:1].clone().requires_grad_(True)
    (mesh_ops.gather_faces(vv, tris[:1], True) * torch.linspace(0.5, 1.5, 9, device="cuda").view(3, 3)).sum().backward()
    assert _rel_max(grads[0], vv.grad) < 1e-6


@pytest.mark.parametrize("node", ["lit", "silhouettes"])
def test_deterministic_switch_must_enclose_backward(node):
    """... and the switch must hold from a node's forward pass to its backward pass: forward builds the ascending visibility
    list and the CSR adjacency (or not), and the library reads the switch again at launch time, so a backward pass outside
    the deterministic() block that enclosed its forward pass -- or inside one that did not -- raises instead of running
    half deterministic.  A pass with both inside still runs."""
    from deep3dmap_amd import _lib
    vs, tris, texs = (t.cuda() for t in _scene(B=1, n=10))            # one shared mesh: what the mode covers
    r = _nr().Renderer(camera_mode="look_at", image_size=32, anti_aliasing=False)
    r.eye = [0.3, 0.4, -2.5]

    def forward():
        v = vs.clone().requires_grad_(True)
        return v, (r(v, tris, texs)[0] if node == "lit" else r.render_silhouettes(v, tris)).sum()

    with _lib.deterministic():
        _, loss = forward()
    with pytest.raises(RuntimeError, match="must enclose backward"):
        loss.backward()
    _, loss = forward()
    with _lib.deterministic():
        with pytest.raises(RuntimeError, match="must enclose backward"):
            loss.backward()
        v, loss = forward()
        loss.backward()
    assert float(v.grad.abs().max()) > 0


def test_second_backward_over_one_forward_result():
    """One render(), two backward passes (retain_graph): the plan built in forward is walked twice, and whatever the first
    walk leaves in the plan's blob and the node's buffers must not reach the second.  Both passes give the same gradients."""
    vs, tris, texs = (t.cuda() for t in _scene(B=2, n=16))
    r = _nr().Renderer(camera_mode="look_at", image_size=64, anti_aliasing=False)
    r.eye = [0.3, 0.5, -2.6]
    w = torch.randn(2, 3, 64, 64, device="cuda")
    vv = vs.clone().requires_grad_(True)
    tt = texs.clone().requires_grad_(True)
    rgb, depth, alpha = r(vv, tris, tt)
    loss = (rgb * w).sum() + (alpha * w[:, 0]).sum() + (depth.clamp(max=4) * w[:, 1]).sum()
    first = torch.autograd.grad(loss, (vv, tt), retain_graph=True)
    second = torch.autograd.grad(loss, (vv, tt))
    for a, b in zip(first, second):
        assert float(a.abs().max()) > 0 and _rel_max(b, a) < 1e-5
