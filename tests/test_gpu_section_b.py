"""The section-B operators of include/d3m_raster.h through the C ABI at every shape: the cameras (d3m_camera_basis, _forward,
_backward, _backward_add), the gather, its scatter and the ordered gather (d3m_gather_faces, d3m_scatter_face_grads,
d3m_vertex_gather), lighting (d3m_lighting_forward, _backward, d3m_face_light) and the output epilogue (d3m_output_epilogue,
_backward), against the predictions of tests/test_section_b_host.py -- the cases, the bit-for-bit expectations of the exact
cases, the float64 restatements and the per-element tolerance (D 2^-24 + 4 E32) bound are defined and proven there -- then the
public wrappers.

Every output sits between guard words and is itself filled with the guard pattern (a NaN): an element that is not written is a
NaN in the result, a word written outside is seen afterwards.  Every call runs twice and the bits must agree, except grad_faces of
d3m_lighting_backward at texture size >= 2 (LDS float atomics order a face's sum), unless it is all zeros.

Each float case prints its achieved err / tolerance (`pytest -s`); the largest per operator is in docs/EXPERIMENTS.md, section N,
and profiles/section_b_operator_errors.json."""
import ctypes

import numpy as np
import pytest
import torch

import section_b_scenes as S
import test_section_b_host as H
from conftest import kernels_launched
from test_gpu_loss_reductions import Check as _Check, _bits, _untouched
from test_gpu_param_reductions import GUARD_BITS, Guarded

pytestmark = pytest.mark.gpu

D3M_OK = 0
WORST = {}          # operator -> the largest err / tolerance of the session


@pytest.fixture(scope="module", autouse=True)
def _print_worst():
    """the session's largest err / tolerance per operator, printed once at the end (`pytest -s`)"""
    yield
    for operator, worst in sorted(WORST.items()):
        print(f"SECTIONB-WORST {operator} err/tolerance={worst:.3e}")


class Check(_Check):
    """the loss tests' collector, with a per-element tolerance that prints what was achieved"""

    def bounded(self, operator, what, got, ref):
        want, tol = ref[0], ref[1]
        if tol is None:
            return self.exact(what, got, want)
        got, want, tol = (np.asarray(x, np.float64).reshape(-1) for x in (got, want, tol))
        if got.shape != want.shape:
            return self.failures.append((what, "shape", got.shape, want.shape))
        err = np.abs(got - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(tol > 0, err / np.where(tol > 0, tol, 1), np.where(err == 0, 0.0, np.inf))
        worst = float(np.nanmax(ratio)) if ratio.size else 0.0
        print(f"SECTIONB {operator} {S.case_id(self.c)} {what} E32={ref[2]:.3e} err/tolerance={worst:.3e}")
        WORST[operator] = max(WORST.get(operator, 0.0), worst)
        if not bool((err <= tol).all()):             # (a NaN fails)
            self.failures.append((what, "largest err / tolerance", worst, "at", int(np.nanargmax(ratio)), "NaN" * bool(np.isnan(err).any())))


def _dev(x, dtype=torch.float32):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dtype).cuda().contiguous()


def _run(name, *args, expect=D3M_OK):
    """the entry point on the current stream; every Guarded among the arguments is checked afterwards"""
    from deep3dmap_amd import _lib
    conv = [_lib.ptr(a.inner if isinstance(a, Guarded) else a) if isinstance(a, (Guarded, torch.Tensor)) or a is None else a for a in args]
    rc = getattr(_lib.lib(), name)(*conv, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, (name, rc)
    for a in args:
        assert not isinstance(a, Guarded) or a.intact(), (name, "guard words were written")


def _np(g):
    return None if g is None else g.inner.cpu().numpy()


def _launched(names, fn):
    with kernels_launched() as k:
        out = fn()
    assert k.names == names, (names, k.names)
    return out


def _vec3(x):
    return (ctypes.c_float * 3)(*[float(v) for v in x])


# ==== 1. cameras ===================================================================================================================
class Camera:
    """the d3m_camera block of a case on the device"""

    def __init__(self, c, inp=None):
        from deep3dmap_amd import _lib
        inp = S.camera_inputs(c) if inp is None else inp
        self.c, self.inp = c, inp
        self.keep = {k: _dev(inp[k]) for k in ("rot", "eye", "K", "dist")}
        cam = _lib.D3MCamera()
        cam.mode = {"none": _lib.CAMERA_NONE, "look_at": _lib.CAMERA_LOOK_AT, "perspective": _lib.CAMERA_LOOK_AT, "look": _lib.CAMERA_LOOK,
                    "projection": _lib.CAMERA_PROJECTION}[c.mode]
        cam.perspective, cam.tan_half_width, cam.orig_size = int(c.persp), S.tan_width(), S.ORIG_SIZE
        for field, key in (("rot", "rot"), ("eye_or_t", "eye"), ("K", "K"), ("dist", "dist")):
            t = self.keep[key]
            setattr(cam, field, None if t is None else t.data_ptr())
            setattr(cam, "eye_batch" if key == "eye" else field + "_batch", 1 if t is None else t.shape[0])
        self.cam = cam
        self.v, self.g = _dev(inp["v"]), _dev(inp["g"])

    def forward(self):
        out = Guarded((self.c.B, self.c.V, 3))
        _run("d3m_camera_forward", self.v, self.c.vb, ctypes.byref(self.cam), out, self.c.B, self.c.V)
        return _np(out)

    def backward(self, g=None, per_view=False, onto=None):
        """per_view: the same mesh handed over once per view (the per-view route); onto: d3m_camera_backward_add onto this prefill"""
        c = self.c
        vb = c.B if per_view else c.vb
        v = self.v.expand(c.B, c.V, 3).contiguous() if per_view and c.vb == 1 else self.v
        out = Guarded((vb, c.V, 3))
        if onto is not None:
            out.inner.copy_(_dev(onto))
        _run("d3m_camera_backward" if onto is None else "d3m_camera_backward_add", v, vb, ctypes.byref(self.cam), self.g if g is None else g,
             out, c.B, c.V)
        return _np(out)


@pytest.mark.parametrize("c", S.camera_cases(), ids=S.case_id)
def test_camera_at_shape(c):
    chk, ref, cam = Check(c), H.camera_reference(c), Camera(c)
    suffix = ("_projection" if c.mode == "projection" else "")
    got = _launched({"k_camera_forward"}, cam.forward)
    chk.twice("forward", [got], [cam.forward()])
    chk.bounded("camera_forward" + suffix, "forward", got, ref["forward"])
    if c.mode == "perspective":           # the identity frame copies z
        chk.exact("z", got[..., 2], S._entry(cam.inp["v"], c.B)[..., 2])
    grad = _launched({"k_camera_backward"}, cam.backward)
    chk.twice("backward", [grad], [cam.backward()])
    chk.bounded("camera_backward" + ("_shared" if c.vb == 1 else "") + suffix, "backward", grad, ref["adjoint"])
    added = _launched({"k_camera_backward"}, lambda: cam.backward(onto=cam.inp["prefill"]))
    chk.twice("backward_add", [added], [cam.backward(onto=cam.inp["prefill"])])
    chk.exact("backward_add = float32(prefill + plain)", added, S.add_onto(cam.inp["prefill"], grad))
    chk.done()


@pytest.mark.parametrize("c", S.needle_cases(), ids=S.case_id)
def test_shared_route_takes_every_view_exactly_once(c):
    """a gradient that is zero outside view b: the shared route returns the per-view route's row b bit for bit"""
    chk, cam = Check(c), Camera(c)
    rows = cam.backward(per_view=True) if c.B > 1 else cam.backward()
    for b in range(c.B):
        got = cam.backward(g=_dev(S.needle(cam.inp["g"], b)))
        chk.exact(f"needle {b}", got[0], rows[b])
    chk.done()


@pytest.mark.parametrize("c", S.basis_cases(), ids=S.case_id)
def test_camera_basis_at_shape(c):
    chk = Check(c)
    eye, tgt, up = (_dev(x) for x in S.basis_inputs(c))

    def basis():
        rot = Guarded((c.B, 9))
        _run("d3m_camera_basis", eye, eye.shape[0], tgt, tgt.shape[0], up, up.shape[0], c.is_look_at, rot, c.B)
        return _np(rot)
    got = _launched({"k_camera_basis"}, basis)
    chk.twice("basis", [got], [basis()])
    assert np.isfinite(got).all()
    chk.bounded("camera_basis", "rows", got, H.basis_reference(c))
    chk.done()


@pytest.mark.parametrize("mode", ["look_at", "projection"])
def test_camera_wrappers_reach_the_shared_route(mode):
    """nr.look_at(vertices [1,V,3], eyes [B,3]) and nr.projection with one mesh: k_camera_backward's shared route, and a gradient
    of the vertices' own shape"""
    from deep3dmap_amd import neural_renderer as nr
    c = next(c for c in S.camera_cases() if c.mode == mode and c.vb == 1 and c.B == 9 and c.V == 33 and not any(c.pb) and c.persp == 0)
    chk, inp, ref = Check(c), S.camera_inputs(c), H.camera_reference(c)
    v = _dev(inp["v"]).requires_grad_(True)
    with kernels_launched() as k:
        if mode == "look_at":
            out = nr.look_at(v, _dev(inp["vectors"][0]), _dev(inp["vectors"][1]), _dev(inp["vectors"][2]))
        else:
            out = nr.projection(v, _dev(inp["K"]).reshape(-1, 3, 3), _dev(inp["rot"]).reshape(-1, 3, 3), _dev(inp["eye"]).reshape(-1, 1, 3),
                                _dev(inp["dist"]), S.ORIG_SIZE)
        out.backward(_dev(inp["g"]))
    assert k.names == {"k_camera_forward", "k_camera_backward"} | ({"k_camera_basis"} if mode == "look_at" else set()), k.names
    assert out.shape == (c.B, c.V, 3) and v.grad.shape == (1, c.V, 3)
    chk.bounded("camera_forward" + ("_projection" if mode == "projection" else ""), "wrapper forward", out.detach().cpu().numpy(), ref["forward"])
    chk.bounded("camera_backward_shared" + ("_projection" if mode == "projection" else ""), "wrapper backward", v.grad.cpu().numpy(), ref["adjoint"])
    chk.done()


# ==== 2. gather, scatter, ordered gather ================================================================================================
@pytest.mark.parametrize("c", S.gather_cases(), ids=S.case_id)
def test_gather_and_its_adjoints_at_shape(c):
    from deep3dmap_amd import _lib
    chk, inp = Check(c), S.gather_inputs(c)
    Fp = (2 if c.fb else 1) * c.Ft
    v, tri = _dev(inp["v"]), _dev(inp["tri"], torch.int32)
    g_a, g_b, nil = _dev(inp["g_a"]), _dev(inp["g_b"]), torch.zeros(c.B, Fp, 3, 3, device="cuda")

    def gather():
        out = Guarded((c.B, Fp, 3, 3))
        _run("d3m_gather_faces", v, tri, c.tb, out, c.B, c.V, c.Ft, c.fb)
        return _np(out)

    def scatter(g):
        out = Guarded((c.B, c.V, 3))
        out.inner.copy_(_dev(inp["prefill"]))
        _run("d3m_scatter_face_grads", g, tri, c.tb, out, c.B, c.V, c.Ft, c.fb)
        return _np(out)
    got = _launched({"k_gather_faces"}, gather)
    chk.twice("gather", [got], [gather()])
    chk.exact("gather", got, S.gather_faces(c, inp))
    got = _launched({"k_scatter_face_grads"}, lambda: scatter(g_a))
    chk.twice("scatter", [got], [scatter(g_a)])
    chk.exact("scatter onto the prefill", got, S.scatter_face_grads(c, inp, inp["g_a"]))
    chk.exact("scatter of zeros leaves the prefill", scatter(nil), inp["prefill"])
    chk.exact("scatter of -0.0 leaves the prefill", scatter(-nil), inp["prefill"])
    if c.tb == 1:
        offsets, items = _dev(inp["offsets"], torch.int32), _dev(inp["items"], torch.int32)
        blob = torch.zeros(int(_lib.lib().d3m_visibility_bytes(c.B, Fp)) // 4 + 1, dtype=torch.int32, device="cuda")
        blob[:c.B * Fp] = _dev(inp["flags"], torch.int32).reshape(-1)

        def ordered(a, b, flags):
            out = Guarded((c.B, c.V, 3))
            _run("d3m_vertex_gather", a, b, offsets, items, out, c.B, c.V, c.Ft, c.fb, blob if flags else None)
            return _np(out)
        for what, a, b, na, nb in (("one array", g_a, None, inp["g_a"], None), ("two arrays", g_a, g_b, inp["g_a"], inp["g_b"]),
                                   ("the second array alone", None, g_b, None, inp["g_b"])):
            for flags in (False, True):
                got = _launched({"k_vertex_gather"}, lambda: ordered(a, b, flags))      # (a NaN-filled output comes back fully written)
                chk.twice(f"ordered gather, {what}, flags={flags}", [got], [ordered(a, b, flags)])
                chk.exact(f"ordered gather, {what}, flags={flags}", got, S.vertex_gather(c, inp, na, nb, inp["flags"] if flags else None))
                chk.exact("the unused vertex is written: zeros", got[:, -1], np.zeros((c.B, 3)))
        if c.fb:
            pin = S.corner_pin(c)
            chk.exact("the back copy's corners are reversed", ordered(_dev(pin), None, False), S.vertex_gather(c, inp, pin, None, None))
    chk.done()


@pytest.mark.parametrize("c", [c for c in S.gather_cases() if c.tb == 1], ids=S.case_id)
def test_gather_faces_wrapper_in_both_modes(c):
    """gather_faces + backward in the default (scatter) and the deterministic (ordered gather) mode: the same bits on integers"""
    from deep3dmap_amd import _lib
    from deep3dmap_amd.neural_renderer.mesh_ops import gather_faces
    chk, inp = Check(c), S.gather_inputs(c)
    grads = []
    for on, kernel in ((False, "k_scatter_face_grads"), (True, "k_vertex_gather")):
        v = _dev(inp["v"]).requires_grad_(True)
        with _lib.deterministic(on), kernels_launched() as k:
            faces = gather_faces(v, _dev(inp["tri"], torch.int32), bool(c.fb))
            faces.backward(_dev(inp["g_a"]))
        assert {"k_gather_faces", kernel} <= k.names and not ({"k_scatter_face_grads", "k_vertex_gather"} - {kernel}) & k.names, k.names
        chk.exact("faces", faces.detach().cpu().numpy(), S.gather_faces(c, inp))
        grads.append(v.grad.cpu().numpy())
    chk.exact("default mode", grads[0], S.vertex_gather(c, inp, inp["g_a"], None, None))
    chk.twice("the two modes", [grads[0]], [grads[1]])
    chk.done()


# ==== 3. lighting ==================================================================================================================
@pytest.mark.parametrize("c", S.light_cases(), ids=S.case_id)
def test_lighting_at_shape(c):
    chk, inp, ref, p = Check(c), S.light_inputs(c), H.light_reference(c), S.light_of(c)
    per = c.ts ** 3
    faces, tex, g = _dev(inp["faces"]), _dev(inp["tex"]), _dev(inp["g"])
    light = (p["ia"], p["id"], _vec3(p["ca"]), _vec3(p["cd"]), _vec3(p["dir"]))

    def forward():
        out = Guarded((c.n, per, 3))
        _run("d3m_lighting_forward", faces, tex, out, *light, c.n, c.ts)
        return _np(out)

    def backward(with_tex=True, with_faces=True):
        g_tex, g_faces = Guarded((c.n, per, 3)) if with_tex else None, Guarded((c.n, 3, 3)) if with_faces else None
        _run("d3m_lighting_backward", faces, tex, g, g_tex, g_faces, *light, c.n, c.ts)
        return _np(g_tex), _np(g_faces)
    # LDS float atomics order a face's sum at ts >= 2: grad_faces is exempt from the run-twice rule there, unless it is all zeros
    ordered = c.ts == 1 or c.kind in ("back_ia0", "id0")
    out = _launched({"k_lighting_forward"}, forward)
    chk.twice("forward", [out], [forward()])
    g_tex, g_faces = _launched({"k_lighting_backward"}, backward)
    again = backward()
    chk.twice("backward", [g_tex, g_faces] if ordered else [g_tex], list(again) if ordered else [again[0]])
    near = "_near_degenerate" if c.kind == "near_degenerate" else ""
    chk.bounded("lighting_forward" + near, "forward", out, ref["forward"])
    chk.bounded("lighting_grad_textures" + near, "grad_textures", g_tex, ref["grad_textures"])
    chk.bounded("lighting_grad_faces" + near, "grad_faces", g_faces, ref["grad_faces"])
    # each output alone: the bits of the call that wrote both
    chk.twice("grad_textures alone", [g_tex], [backward(True, False)[0]])
    if ordered:
        chk.twice("grad_faces alone", [g_faces], [backward(False, True)[1]])
    else:
        chk.bounded("lighting_grad_faces" + near, "grad_faces alone", backward(False, True)[1], ref["grad_faces"])
    f32 = ref["f32"]
    if c.kind == "ones":            # the output is the light itself: d3m_face_light's, bit for bit ("the same f32 product")
        sv, st = S.soup(inp["faces"])
        fl = Guarded((1, c.n, 3))
        _launched({"k_face_light"}, lambda: _run("d3m_face_light", _dev(sv), 1, _dev(st, torch.int32), 1, fl, *light, 1, 3 * c.n, c.n, 0))
        chk.exact("textures of ones: the light of d3m_face_light", out, np.repeat(_np(fl)[0][:, None], per, 1))
    if c.kind in ("back_ia0", "id0"):
        chk.exact("forward", out, f32[0])
        chk.exact("grad_textures", g_tex, f32[1])
        chk.exact("grad_faces: zeros", g_faces, np.zeros((c.n, 3, 3)))
        assert c.kind == "id0" or (not out.any() and not g_tex.any())
    if c.kind == "twin":
        twin = np.arange(c.n) % 3 == 0
        chk.exact("twin vertices: light = ia ca", out[twin], f32[0][twin])
        chk.exact("twin vertices: grad_faces zero", g_faces[twin], np.zeros((int(twin.sum()), 3, 3)))
    if c.kind == "ia0":             # no ambient term: the light of d3m_face_light with ia = 0 on textures of ones
        ones = torch.ones_like(tex)
        lit = Guarded((c.n, per, 3))
        _run("d3m_lighting_forward", faces, ones, lit, *light, c.n, c.ts)
        sv, st = S.soup(inp["faces"])
        fl = Guarded((1, c.n, 3))
        _run("d3m_face_light", _dev(sv), 1, _dev(st, torch.int32), 1, fl, *light, 1, 3 * c.n, c.n, 0)
        chk.exact("ia = 0: the directional term alone", _np(lit), np.repeat(_np(fl)[0][:, None], per, 1))
    chk.done()


def test_lighting_wrapper_matches_the_entry_points():
    from deep3dmap_amd import neural_renderer as nr
    c = S.LightCase(257, 2, "float")
    chk, inp, ref, p = Check(c), S.light_inputs(c), H.light_reference(c), S.LIGHT
    faces = _dev(inp["faces"]).reshape(1, c.n, 3, 3).requires_grad_(True)
    tex = _dev(inp["tex"]).reshape(1, c.n, 2, 2, 2, 3).requires_grad_(True)
    with kernels_launched() as k:
        out = nr.lighting(faces, tex, p["ia"], p["id"], tuple(p["ca"]), tuple(p["cd"]), tuple(p["dir"]))
        out.backward(_dev(inp["g"]).reshape(out.shape))
    assert k.names == {"k_lighting_forward", "k_lighting_backward"}, k.names
    chk.bounded("lighting_forward", "wrapper forward", out.detach().cpu().numpy(), ref["forward"])
    chk.bounded("lighting_grad_textures", "wrapper grad_textures", tex.grad.cpu().numpy(), ref["grad_textures"])
    chk.bounded("lighting_grad_faces", "wrapper grad_faces", faces.grad.cpu().numpy(), ref["grad_faces"])
    chk.done()


# ==== 4. output epilogue ===============================================================================================================
@pytest.mark.parametrize("c", S.epilogue_cases(), ids=S.case_id)
def test_output_epilogue_at_shape(c):
    chk, inp = Check(c), S.epilogue_inputs(c)
    s = c.S // 2 if c.aa else c.S
    want = S.output_epilogue(c, inp)
    fim, rgb, depth, bg = _dev(inp["fim"], torch.int32), _dev(inp["rgb"]), _dev(inp["depth"]), _dev(inp["bg"])
    shapes = dict(rgb_blended=(c.B, c.S, c.S, 3), alpha_map=(c.B, c.S, c.S), rgb_out=(c.B, 3, s, s), alpha_out=(c.B, s, s), depth_out=(c.B, s, s))
    full = None
    for name, (w_rgb, w_depth, *w_out) in S.EPI_POINTERS.items():
        def forward():
            outs = {k: Guarded(shapes[k]) if on else None for k, on in zip(shapes, w_out)}
            _run("d3m_output_epilogue", fim, rgb if w_rgb else None, depth if w_depth else None, bg if w_rgb else None, c.bb, *outs.values(),
                 c.B, c.S, c.aa)
            return {k: _np(o) for k, o in outs.items()}
        got = _launched({"k_output_epilogue"}, forward)
        chk.twice(name, list(got.values()), list(forward().values()))
        for k, o in got.items():
            if o is not None:
                chk.exact(f"{name}: {k}", o, want[k])
                if full is not None:
                    chk.twice(f"{name}: {k} as with every pointer", [o], [full[k]])
        full = got if full is None else full
    g_out = [_dev(inp[k]) for k in ("g_rgb", "g_alpha", "g_depth")]
    g_shapes = ((c.B, c.S, c.S, 3), (c.B, c.S, c.S), (c.B, c.S, c.S))
    g_want = S.output_epilogue_backward(c, inp)
    for on in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 1, 1)):
        def backward():
            outs = [Guarded(sh) if o else None for sh, o in zip(g_shapes, on)]
            _run("d3m_output_epilogue_backward", *[g if o else None for g, o in zip(g_out, on)], *outs, c.B, c.S, c.aa)
            return [_np(o) for o in outs]
        got = _launched({"k_output_epilogue_backward"}, backward)
        chk.twice(f"backward {on}", got, backward())
        for k, o in enumerate(got):
            if o is not None:
                chk.exact(f"backward {on}: output {k}", o, g_want[k])
    chk.done()


def test_the_guard_pattern_is_a_nan():
    assert np.isnan(np.array([GUARD_BITS], np.int32).view(np.float32)[0]) and _untouched(np.array([GUARD_BITS], np.int32).view(np.float32))
    assert not np.array_equal(_bits(np.float32(0.0)), _bits(np.float32(-0.0)))
