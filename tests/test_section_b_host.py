"""CPU side of the section-B operator tests (tests/section_b_scenes.py, tests/test_gpu_section_b.py): it proves what the GPU file
relies on.

  * the float32 restatements reproduce the committed reference vectors (tests/golden/nr_golden.npz, cam/*) and the float64 ones
    agree with oracle.nr_oracle's torch forms and their autograd;
  * the inputs are as well conditioned as the issue states (vertices in the unit ball, z >= 1, projection depths in [1.5, 3.5],
    `up` 30 degrees off the view, faces 1.25 LIGHT_MARGIN off the light's horizon) -- no case is dropped for conditioning: the
    re-draw loop raises;
  * the integer cases of the gather's adjoints are exact in any order (exact_sum_proven);
  * E32 and the bound of every float case (`*_reference`, printed once by test_print_e32_of_every_float_case);
  * every named wrong variant is rejected by the comparison the GPU test makes.

perspective() alone (the identity frame, eye 0) is NOT taken as exact: v - 0, v 1 + 0 + 0 and the copy of z are exact (z is compared
bit for bit), x / z / width rounds twice and is held to the tolerance like any other float case."""
import functools
import os

import numpy as np
import pytest
import torch

import section_b_scenes as S
from test_param_reductions_host import LIGHT_MARGIN, light_values

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "nr_golden.npz")


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float64)))


# ---- references: (float64 value, per-element tolerance or None = bit for bit, E32) --------------------------------------------------
def _ref(f64, f32, bnd, D):
    e = S.e32_of(f32, f64, bnd)
    return np.asarray(f64, np.float64), S.tolerance(D, e, bnd), e


@functools.lru_cache(maxsize=None)
def camera_reference(c):
    """dict(forward, adjoint): each (ref, tol | None, E32); adjoint is [vb,V,3] -- the per-view terms, or their sum over the views
    in the shared route's own order for E32; terms32: the float32 terms [B,V,3] (the needles' expectation)"""
    inp = S.camera_inputs(c)
    Df, Da = S.CAM_D[c.mode]
    f64, f32, fab = (S.camera_forward(c, inp, ar) for ar in ("f64", "f32", "abs"))
    t64, t32, tab = (S.camera_adjoint_terms(c, inp, ar) for ar in ("f64", "f32", "abs"))
    out = dict(terms32=t32)
    out["forward"] = (f64, None, 0.0) if c.mode == "none" else _ref(f64, f32, fab.a, Df)
    if c.vb > 1:
        out["adjoint"] = (t64, None, 0.0) if c.mode == "none" else _ref(t64, t32 + np.float32(0), tab.a, Da)
    else:
        out["adjoint"] = _ref(t64.sum(0, keepdims=True), S.shared_sum32(t32)[None], tab.a.sum(0, keepdims=True), S.shared_D(c.B))
    return out


@functools.lru_cache(maxsize=None)
def basis_reference(c):
    args = S.basis_inputs(c)
    f64, f32, ab = (S.camera_basis(*args, c.is_look_at, c.B, ar) for ar in ("f64", "f32", "abs"))
    return _ref(f64, f32, ab.a, S.BASIS_D)


@functools.lru_cache(maxsize=None)
def light_reference(c):
    """dict(forward, grad_textures, grad_faces): each (ref, tol, E32); f32: the float32 restatement of the three (the exact cases'
    expectation)"""
    inp = S.light_inputs(c)
    f = {ar: (S.lighting_forward(c, inp, ar),) + S.lighting_backward(c, inp, ar) for ar in ("f64", "f32", "abs")}
    D = (S.LIGHT_FWD_D, S.LIGHT_FWD_D, S.light_grad_faces_D(c.ts))
    out = {name: _ref(f["f64"][k], f["f32"][k], f["abs"][k].a, D[k]) for k, name in enumerate(("forward", "grad_textures", "grad_faces"))}
    out["f32"] = f["f32"]
    return out


# ---- 1. the restatements against the reference's vectors and the oracle ------------------------------------------------------------
def test_float32_camera_restatement_reproduces_the_reference_golden():
    z = np.load(GOLDEN)
    v, eyes = z["cam/look_at/vertices"].astype(np.float64), z["cam/look_at/eyes"].astype(np.float64)
    B, V = v.shape[:2]
    at, up = np.zeros((1, 3)), np.array([[0.0, 1.0, 0.0]])
    inp = dict(v=v, g=z["cam/look_at/grad_out"].astype(np.float64), eye=eyes, K=None, dist=None,
               rot=S.f32v(S.camera_basis(eyes, at, up, True, B, "f32")), width=S.tan_width(float(z["cam/look_at/persp_angle"])))
    plain, persp = S.CamCase("look_at", 0, B, V, B, (0, 0)), S.CamCase("look_at", 1, B, V, B, (0, 0))
    assert np.allclose(S.camera_forward(plain, inp, "f32"), z["cam/look_at/out"], rtol=1e-5, atol=2e-6)
    assert np.allclose(S.camera_forward(persp, inp, "f32"), z["cam/look_at/persp_out"], rtol=1e-5, atol=2e-6)
    assert np.allclose(S.camera_adjoint_terms(persp, inp, "f64"), z["cam/look_at/grad_vertices"], rtol=1e-4, atol=1e-6)
    pv = z["cam/projection/vertices"].astype(np.float64)
    inp = dict(v=pv, g=z["cam/projection/grad_out"].astype(np.float64), rot=z["cam/projection/R"].reshape(-1, 9).astype(np.float64),
               eye=z["cam/projection/t"].reshape(-1, 3).astype(np.float64), K=z["cam/projection/K"].reshape(-1, 9).astype(np.float64),
               dist=z["cam/projection/dist"].astype(np.float64), orig=float(z["cam/projection/orig_size"]))
    c = S.CamCase("projection", 0, pv.shape[0], pv.shape[1], pv.shape[0], (0, 0, 0, 0))
    assert np.allclose(S.camera_forward(c, inp, "f32"), z["cam/projection/out"], rtol=1e-5, atol=2e-6)
    assert np.allclose(S.camera_adjoint_terms(c, inp, "f64"), z["cam/projection/grad_vertices"], rtol=1e-4, atol=1e-5)
    # vertices_to_faces and lighting of the same file
    faces, tex, p = z["cam/v2f/out"], z["cam/lighting/textures"], z["cam/lighting/params"].astype(np.float64)
    gc = S.GatherCase(3, pv.shape[1], faces.shape[1], 0, 3)
    assert np.array_equal(S.gather_faces(gc, dict(v=pv, tri=z["cam/v2f/faces"])), faces)
    n = faces.shape[0] * faces.shape[1]
    linp = dict(faces=faces.reshape(n, 3, 3).astype(np.float64), tex=tex.reshape(n, 8, 3).astype(np.float64),
                light=dict(ia=float(p[0]), id=float(p[1]), ca=p[2:5], cd=p[5:8], dir=p[8:11]))
    assert np.allclose(S.lighting_forward(S.LightCase(n, 2, "float"), linp, "f32").reshape(tex.shape), z["cam/lighting/out"], rtol=1e-5, atol=1e-6)


ORACLE_CASES = [c for c in S.camera_cases() if not any(c.pb) and c.mode in ("look_at", "look", "projection") and c.V == 33 and c.B in (3, 9)]


@pytest.mark.parametrize("c", ORACLE_CASES, ids=S.case_id)
def test_float64_camera_restatement_is_the_oracle_and_its_autograd(c):
    from oracle import nr_oracle as O
    inp = S.camera_inputs(c)
    v = _t(S._entry(inp["v"], c.B)).requires_grad_(True)
    if c.mode == "projection":
        out = O._projection_torch(v, _t(inp["K"]).reshape(-1, 3, 3), _t(inp["rot"]).reshape(-1, 3, 3), _t(inp["eye"]).reshape(-1, 1, 3),
                                  _t(inp["dist"]), S.ORIG_SIZE)
    else:
        e, a, u = (_t(x) for x in inp["vectors"])
        out = (O._look_at_torch if c.mode == "look_at" else O._look_torch)(v, e, a, u)
        if c.persp:
            z = out[:, :, 2]
            out = torch.stack([out[:, :, 0] / z / S.tan_width(), out[:, :, 1] / z / S.tan_width(), z], 2)
    (gv,) = torch.autograd.grad(out, v, _t(inp["g"]))
    # (the frame handed to the kernels is a float32 one: the oracle's float64 frame differs from it by float32 rounding)
    assert np.allclose(S.camera_forward(c, inp, "f64"), out.detach().numpy(), rtol=0, atol=2e-4 if c.mode == "projection" else 2e-6)
    assert np.allclose(S.camera_adjoint_terms(c, inp, "f64"), gv.numpy(), rtol=1e-5, atol=2e-4 if c.mode == "projection" else 2e-6)


@pytest.mark.parametrize("mode,persp", [("look_at", 1), ("projection", 0), ("perspective", 1)])
def test_float64_camera_adjoint_matches_central_differences_of_the_forward(mode, persp):
    """the analytic adjoint against finite differences of the forward restatement, in float64 on the very same inputs (frame
    included): central differences of step 1e-6 agree to 1e-7 of the gradient's scale"""
    c = next(c for c in S.camera_cases() if c.mode == mode and c.persp == persp and c.vb > 1)
    inp = dict(S.camera_inputs(c))
    gv = S.camera_adjoint_terms(c, inp, "f64")
    h, fd = 1e-6, np.zeros_like(gv)
    for k in range(3):
        lo, hi = dict(inp), dict(inp)
        step = np.zeros(3)
        step[k] = h
        lo["v"], hi["v"] = inp["v"] - step, inp["v"] + step
        d = (_fwd64(c, hi) - _fwd64(c, lo)) / (2 * h)
        fd[:, :, k] = (d * inp["g"]).sum(2)
    assert np.abs(fd - gv).max() <= 1e-6 * max(1.0, np.abs(gv).max())


def _fwd64(c, inp):
    """camera_forward in float64 on inputs that need not be float32 values (finite differences)"""
    saved = S.lift
    try:
        S.lift = lambda a, ar: np.asarray(a, np.float64)
        return S.camera_forward(c, inp, "f64")
    finally:
        S.lift = saved


@pytest.mark.parametrize("c", [c for c in S.light_cases() if c.kind in ("float", "near_degenerate", "twin", "ia0", "id0") and c.n <= 257],
                         ids=S.case_id)
def test_float64_lighting_restatement_is_the_reference_form_and_its_autograd(c):
    inp, p = S.light_inputs(c), S.light_of(c)
    faces, tex = _t(inp["faces"]).requires_grad_(True), _t(inp["tex"]).requires_grad_(True)
    light = light_values(faces, torch.tensor(p["ia"], dtype=torch.float64), torch.tensor(p["id"], dtype=torch.float64), _t(p["ca"]),
                         _t(p["cd"]), _t(p["dir"]))
    out = tex * light[:, None, :]
    g_faces, g_tex = torch.autograd.grad(out, [faces, tex], _t(inp["g"]))
    want_f, (want_gt, want_gf) = S.lighting_forward(c, inp, "f64"), S.lighting_backward(c, inp, "f64")
    scale = lambda x: float(np.abs(x).max()) + 1e-30          # noqa: E731
    # (F.normalize's eps is 1e-5, the kernels' is float32(1e-5): 2.5e-8 apart, which the clamped branch shows)
    assert np.abs(want_f - out.detach().numpy()).max() <= 1e-7 * scale(want_f)
    assert np.abs(want_gt - g_tex.numpy()).max() <= 1e-7 * scale(want_gt)
    assert np.abs(want_gf - g_faces.numpy()).max() <= 1e-7 * scale(want_gf)


def test_float64_basis_restatement_is_f_normalize():
    from oracle import nr_oracle as O
    for c in S.basis_cases():
        e, a, u = (_t(S._entry(x, c.B)) for x in S.basis_inputs(c))
        want = O._camera_basis(a - e if c.is_look_at else a, u).reshape(c.B, 9).numpy()
        got = S.camera_basis(*S.basis_inputs(c), c.is_look_at, c.B, "f64")
        assert np.isfinite(got).all() and np.allclose(got, want, rtol=1e-6, atol=1e-12), c
        if c.kind == "zero_z":
            assert not got.any()
        if c.kind == "up_parallel":
            assert not got[:, :6].any() and (np.abs(got[:, 6:]).max(1) == 1).all()


# ---- 2. conditioning ----------------------------------------------------------------------------------------------------------------
def test_camera_inputs_are_well_conditioned():
    for c in S.camera_cases():
        inp = S.camera_inputs(c)
        radius = np.linalg.norm(inp["v"] - (np.array([0, 0, 2.5]) if c.mode == "perspective" else 0), axis=-1)
        assert radius.max() <= 1.0, c
        if c.mode == "none":
            continue
        z = S.camera_forward(S.CamCase(c.mode, 0, *c[2:]), inp, "f64")[..., 2]
        if c.mode == "projection":
            assert 1.5 <= z.min() and z.max() <= 3.5, (c, z.min(), z.max())
            assert (inp["dist"] != 0).all() and (inp["K"][:, 1] != 0).all()          # five coefficients and a skew
        else:
            assert z.min() >= 1.0, (c, z.min())
        if c.mode in ("look_at", "look"):
            assert (np.linalg.norm(inp["eye"], axis=1) >= 2).all()
    for c in S.basis_cases():
        if c.kind != "float":
            continue
        e, a, u = (S._entry(x, c.B) for x in S.basis_inputs(c))
        zdir = a - e if c.is_look_at else a
        cos = np.abs((zdir * u).sum(1)) / (np.linalg.norm(zdir, axis=1) * np.linalg.norm(u, axis=1))
        assert cos.max() <= np.cos(np.radians(30)), c
    # every pairing of an eye with another view's target and `up` (a parameter of batch 1 meets every view)
    eye, at, direction, up = S._views(33, S._rng(1))
    for tgt in (at[:, None] - eye[None], np.repeat(direction[:, None], 33, 1)):
        cos = np.abs((tgt * up[:, None]).sum(2)) / (np.linalg.norm(tgt, axis=2) * np.linalg.norm(up, axis=1)[:, None])
        assert cos.max() <= np.cos(np.radians(30))


def test_cases_cover_what_the_issue_lists():
    cams = S.camera_cases()
    assert {c.B for c in cams if c.vb == 1} >= set(S.SHARED_B) and {c.V for c in cams} >= set(S.CAM_V)
    for mode in ("look_at", "look", "projection"):
        n = len(S.CAM_PARAMS[mode])
        for vb in (1, 3):
            assert {c.pb for c in cams if c.mode == mode and (c.vb == 1) == (vb == 1)} >= {tuple(int(j == k) for j in range(n)) for k in range(n)}
    assert {(c.mode, c.persp) for c in cams} == {("look_at", 1), ("look_at", 0), ("look", 1), ("look", 0), ("projection", 0), ("none", 0),
                                                 ("perspective", 1)}
    assert {(c.B, c.V) for c in S.needle_cases()} >= {(B, 33) for B in S.SHARED_B} | {(9, V) for V in S.CAM_V}
    assert {tuple(c.pb) for c in S.basis_cases() if c.B > 1} >= {(1, 0, 0), (0, 1, 0), (0, 0, 1)}
    assert {S.lanes_of(c) for c in S.gather_cases()} >= {252, 261, 513, 5580}
    assert {(c.B, c.tb, c.fb) for c in S.gather_cases()} >= {(1, 1, 1), (1, 1, 0), (3, 1, 0), (3, 3, 0), (3, 1, 1)}
    floats = [c for c in S.light_cases() if c.kind == "float"]
    assert {c.n for c in floats} == set(S.LIGHT_N) and {c.ts for c in floats} == set(S.LIGHT_TS)
    assert {(c.n, c.ts) for c in floats} >= {(n, ts) for n in (257, 513) for ts in S.LIGHT_TS}
    epi = S.epilogue_cases()
    assert {(c.S, c.aa) for c in epi} == {(2, 1), (6, 1), (10, 1), (34, 1), (1, 0), (5, 0), (17, 0), (33, 0)}
    assert {(c.B, c.bb) for c in epi} == {(1, 1), (3, 1), (3, 3)}
    sizes = sorted(c.B * (c.S // (2 if c.aa else 1)) ** 2 for c in epi)
    assert sizes[0] < 256 < sizes[-1]


def test_light_faces_are_off_the_horizon_and_no_case_is_dropped():
    """light_inputs re-draws until every face passes and raises otherwise: building every case IS the cap"""
    for c in S.light_cases():
        inp = S.light_inputs(c)
        assert inp["faces"].shape == (c.n, 3, 3)
        a, b = inp["faces"][:, 0] - inp["faces"][:, 1], inp["faces"][:, 2] - inp["faces"][:, 1]
        cr = np.cross(a, b)
        length = np.linalg.norm(cr, axis=1)
        twin = (np.arange(c.n) % 3 == 0) if c.kind == "twin" else np.zeros(c.n, bool)
        assert (length[twin] == 0).all() and (np.cross(a.astype(np.float32), b.astype(np.float32))[twin] == 0).all()
        ok = ~twin
        shape = length[ok] / (np.linalg.norm(a[ok], axis=1) * np.linalg.norm(b[ok], axis=1))
        lit = np.abs(cr[ok] @ S.LIGHT["dir"]) / (length[ok] * np.linalg.norm(S.LIGHT["dir"]))
        assert shape.min() >= LIGHT_MARGIN and lit.min() >= LIGHT_MARGIN, (c, shape.min(), lit.min())
        if c.kind == "near_degenerate":
            assert (length > 1e-7).all() and (length < 1e-5).all() and (cr @ S.LIGHT["dir"] > 0).all()
        if c.kind == "back_ia0":
            assert (cr @ S.LIGHT["dir"] < 0).all()
        if c.kind not in ("twin", "near_degenerate"):
            sh, lt = S.conditioning(inp["faces"], S.LIGHT["dir"])          # the project's own measure
            assert sh.min() >= LIGHT_MARGIN and lt.min() >= LIGHT_MARGIN
        # a tail block's values differ from every other face's
        lo, hi = inp["tex"].min((1, 2)), inp["tex"].max((1, 2))
        assert c.kind == "ones" or (lo[1:] > hi[:-1]).all()
        assert (np.abs(inp["g"]).min((1, 2))[1:] > np.abs(inp["g"]).max((1, 2))[:-1]).all()


# ---- 3. the exact cases ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", S.gather_cases(), ids=S.case_id)
def test_gather_adjoints_are_exact_in_any_order(c):
    inp = S.gather_inputs(c)
    for g in (inp["g_a"], inp["g_b"]):
        assert np.abs(g).max() <= 8 and np.array_equal(g, np.round(g))
    mag = S.scatter_face_grads(c, inp, np.abs(inp["g_a"]) + np.abs(inp["g_b"]), absolute=True)
    assert S.exact_sum_proven(np.concatenate([inp["g_a"].ravel(), inp["g_b"].ravel(), inp["prefill"].ravel()]), total=mag.max())
    got32, got64 = (S.scatter_face_grads(c, inp, inp["g_a"], dt) for dt in (np.float32, np.float64))
    assert S.same_bits(got32, got64)
    assert (inp["g_a"] == 0).any() and np.signbit(inp["g_a"][inp["g_a"] == 0]).any()          # zeros and -0.0 are among the entries
    if c.tb == 1:
        v32, v64 = (S.vertex_gather(c, inp, inp["g_a"], inp["g_b"], inp["flags"], dt) for dt in (np.float32, np.float64))
        assert np.array_equal(v32.astype(np.float64), v64) and not v64[:, -1].any()          # the unused vertex: zeros
        # without flags the ordered gather is the scatter onto zeros
        plain = S.vertex_gather(c, inp, inp["g_a"], None, None)
        assert np.array_equal(plain, S.scatter_face_grads(c, dict(inp, prefill=np.zeros_like(inp["prefill"])), inp["g_a"]))


@pytest.mark.parametrize("c", [c for c in S.light_cases() if c.kind not in ("float", "near_degenerate")], ids=S.case_id)
def test_exact_lighting_cases_are_what_the_issue_says(c):
    """why each is exact: the light is a constant or zero -- no rounding of the normal reaches the result"""
    inp, p = S.light_inputs(c), S.light_of(c)
    out, g_tex, g_faces = (np.asarray(x, np.float64) for x in light_reference(c)["f32"])
    ambient = (np.float32(p["ia"]) * p["ca"].astype(np.float32)).astype(np.float64)
    if c.kind == "ones":            # 1 * light = light: the output repeats the face's light on every texel
        light = np.stack(S.face_light(inp["faces"], p, "f32")[0], 1)
        assert np.array_equal(out, np.repeat(light[:, None], c.ts ** 3, 1))
    if c.kind == "back_ia0":        # relu = 0 and no ambient term: 0 + id (cd 0)
        assert not out.any() and not np.asarray(g_tex).any() and not np.asarray(g_faces).any()
    if c.kind == "twin":            # cross = 0 exactly: n = 0 / 1e-5 = 0, relu(0) = 0, light = ia ca + 0; cs > 0 is false
        twin = np.arange(c.n) % 3 == 0
        assert np.array_equal(out[twin], inp["tex"].astype(np.float32)[twin] * ambient.astype(np.float32)) and not np.asarray(g_faces)[twin].any()
        assert np.asarray(g_faces)[~twin].any()
    if c.kind == "id0":             # the ambient term alone; no gradient reaches the normal
        assert np.array_equal(out, (inp["tex"].astype(np.float32) * ambient.astype(np.float32)).astype(np.float64)) and not np.asarray(g_faces).any()
    if c.kind == "ia0":             # no ambient term: the light is id (cd relu)
        light, _, _, cs, _ = S.face_light(inp["faces"], p, "f32")
        want = np.stack([np.float32(p["id"]) * (np.float32(p["cd"][k]) * np.maximum(cs, np.float32(0))) for k in range(3)], 1)
        assert np.array_equal(np.stack(light, 1), want)


def test_perspective_alone_copies_z():
    c = next(c for c in S.camera_cases() if c.mode == "perspective")
    inp = S.camera_inputs(c)
    assert np.array_equal(S.camera_forward(c, inp, "f32")[..., 2].astype(np.float64), S._entry(inp["v"], c.B)[..., 2])


# ---- 4. E32 and the bounds ----------------------------------------------------------------------------------------------------------------
def test_print_e32_of_every_float_case():
    """printed once (`pytest -s`); the largest per operator is in docs/EXPERIMENTS.md next to what the kernels achieved"""
    worst = {}
    for c in S.camera_cases():
        r = camera_reference(c)
        for name in ("forward", "adjoint"):
            key = f"camera_{name}" + ("_shared" if c.vb == 1 and name == "adjoint" else "") + ("_projection" if c.mode == "projection" else "")
            worst[key] = max(worst.get(key, 0.0), r[name][2])
            print(f"SECTIONB-E32 {S.case_id(c)} {name} E32={r[name][2]:.3e}")
            assert np.isfinite(r[name][0]).all() and (r[name][1] is None or np.isfinite(r[name][1]).all())
            assert r[name][2] < 64 * S.U, (c, name, r[name][2])          # a float32 evaluation of a well conditioned case
    for c in S.basis_cases():
        r = basis_reference(c)
        worst["camera_basis"] = max(worst.get("camera_basis", 0.0), r[2])
        print(f"SECTIONB-E32 {S.case_id(c)} basis E32={r[2]:.3e}")
        assert r[2] < 64 * S.U
    for c in S.light_cases():
        r = light_reference(c)
        for name in ("forward", "grad_textures", "grad_faces"):
            key = "lighting_" + name + ("_near_degenerate" if c.kind == "near_degenerate" else "")
            worst[key] = max(worst.get(key, 0.0), r[name][2])
            print(f"SECTIONB-E32 {S.case_id(c)} {name} E32={r[name][2]:.3e}")
            assert np.isfinite(r[name][1]).all() and r[name][2] < 64 * S.U, (c, name, r[name][2])
    for k, v in sorted(worst.items()):
        print(f"SECTIONB-E32-WORST {k} {v:.3e} = {v / S.U:.2f} u")


# ---- 5. every wrong variant is rejected by the comparison the GPU test makes ----------------------------------------------------------
def _outside(got, ref):
    """the GPU test's float comparison: some element off by more than its tolerance"""
    want, tol, _ = ref
    return bool((np.abs(np.asarray(got, np.float64) - want) > tol).any())


@pytest.mark.parametrize("c", S.needle_cases(), ids=S.case_id)
def test_needles_pin_every_view_exactly_once(c):
    """adding zeros is exact: the shared route on a gradient that is zero outside view b gives the per-view route's row b, bit for
    bit, in the kernel's own order of additions -- and the two wrong reductions do not"""
    inp = S.camera_inputs(c)
    wrong = {"skip_views_ge_8": False, "view0_twice": False}
    for b in range(c.B):
        t32 = S.camera_adjoint_terms(c, inp, "f32", g=S.needle(inp["g"], b))
        want = camera_reference(c)["terms32"][b] + np.float32(0)
        assert np.array_equal(S.bits(S.shared_sum32(t32)), S.bits(want)), (c, b)
        for v in wrong:
            wrong[v] |= not np.array_equal(S.bits(S.shared_sum32(t32, v)), S.bits(want))
    assert wrong["view0_twice"] and wrong["skip_views_ge_8"] == (c.B > 8), (c, wrong)
    t32 = camera_reference(c)["terms32"]
    if c.B > 8:
        assert _outside(S.shared_sum32(t32, "skip_views_ge_8")[None], camera_reference(c)["adjoint"])
    assert _outside(S.shared_sum32(t32, "view0_twice")[None], camera_reference(c)["adjoint"])
    assert not _outside(S.shared_sum32(t32)[None], camera_reference(c)["adjoint"])


def test_add_that_stores_is_rejected():
    c = S.needle_cases()[0]
    inp = S.camera_inputs(c)
    plain = S.shared_sum32(camera_reference(c)["terms32"])[None]
    assert not np.array_equal(S.bits(S.add_onto(inp["prefill"], plain)), S.bits(S.add_onto(inp["prefill"], plain, "add_stores")))


@pytest.mark.parametrize("c", [c for c in S.camera_cases() if c.mode == "projection" or c.persp], ids=S.case_id)
def test_wrong_camera_adjoints_are_rejected(c):
    inp = S.camera_inputs(c)
    variant = "proj_4p2" if c.mode == "projection" else "persp_no_z"
    t = S.camera_adjoint_terms(c, inp, "f64", variant)
    assert _outside(t if c.vb > 1 else t.sum(0, keepdims=True), camera_reference(c)["adjoint"]), c
    t32 = camera_reference(c)["terms32"]
    assert not _outside(t32 if c.vb > 1 else S.shared_sum32(t32)[None], camera_reference(c)["adjoint"]), c


@pytest.mark.parametrize("c", [c for c in S.gather_cases() if c.tb == 1], ids=S.case_id)
def test_wrong_ordered_gathers_are_rejected(c):
    inp = S.gather_inputs(c)
    right = S.vertex_gather(c, inp, inp["g_a"], inp["g_b"], inp["flags"])
    assert not np.array_equal(right, S.vertex_gather(c, inp, inp["g_a"], inp["g_b"], inp["flags"], variant="flags_ignored"))
    hidden = S.vertex_gather(c, inp, inp["g_a"], None, inp["flags"]) - S.vertex_gather(c, inp, inp["g_a"], None, inp["flags"], variant="flags_ignored")
    assert hidden[:, inp["tri"][0, 0]].any()                  # face 0: flag 0, entries 7 and -5
    if c.fb:
        pin = S.corner_pin(c)
        assert not np.array_equal(S.vertex_gather(c, inp, pin, None, None), S.vertex_gather(c, inp, pin, None, None, variant="back_unreversed"))


def test_wrong_lighting_sweeps_are_rejected():
    for c in S.light_cases():
        assert S.sweep_stays_inside(c)
        assert S.sweep_stays_inside(c, "tail_256") == (c.n % 256 == 0), c
        if c.kind == "float" and c.n > 1:
            assert _outside(S.lighting_forward(c, S.light_inputs(c), "f64", "face_index_by_third"), light_reference(c)["forward"]), c
        if c.kind == "near_degenerate":
            wrong = S.lighting_backward(c, S.light_inputs(c), "f64", "degenerate_by_len")[1]
            assert _outside(wrong, light_reference(c)["grad_faces"]), c
        r = light_reference(c)
        for k, name in enumerate(("forward", "grad_textures", "grad_faces")):
            assert not _outside(r["f32"][k], r[name]), (c, name)


def test_wrong_epilogues_are_rejected():
    flipped = 0
    for c in S.epilogue_cases():
        inp = S.epilogue_inputs(c)
        right = S.output_epilogue(c, inp)
        if c.aa:
            wrong = S.output_epilogue(c, inp, "pool_before_flip")
            flipped += not np.array_equal(S.bits(right["rgb_out"]), S.bits(wrong["rgb_out"]))
            assert np.array_equal(right["alpha_out"], wrong["alpha_out"])          # (small integers: any order)
        if c.bb > 1:
            wrong = S.output_epilogue(c, inp, "bg_row0")
            assert not np.array_equal(S.bits(right["rgb_out"]), S.bits(wrong["rgb_out"])), c
        # covered: rgb, uncovered: the background, exactly
        cov = inp["fim"] >= 0
        bg = np.broadcast_to(inp["bg"][:, None, None, :] if c.bb > 1 else inp["bg"][None, None], inp["rgb"].shape)
        assert np.array_equal(S.bits(right["rgb_blended"]), S.bits(np.where(cov[..., None], inp["rgb"], bg)))
        # the adjoint of the restatement is the restatement of the adjoint: <forward(x), g> = <x, backward(g)> in float64
        g_rgb, g_alpha, g_depth = S.output_epilogue_backward(c, inp)
        assert np.isclose((right["depth_out"].astype(np.float64) * inp["g_depth"]).sum(), (inp["depth"].astype(np.float64) * g_depth).sum(), rtol=1e-5)
        assert np.isclose((right["rgb_out"].astype(np.float64) * inp["g_rgb"]).sum(), (right["rgb_blended"].astype(np.float64) * g_rgb).sum(), rtol=1e-5)
    assert flipped >= 4          # the pairing order shows in the bits wherever three of four addends round differently
