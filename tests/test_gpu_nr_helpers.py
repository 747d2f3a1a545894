"""NrRenderer's helper kernels through the C ABI, off the square and at every launch shape: d3m_view_transform, d3m_grid_warp,
d3m_depth_normals, d3m_textures_from_im and d3m_warp_resample, each with its _backward (and d3m_warp_resample_partials),
against the predictions of tests/test_nr_helpers_host.py -- the cases, the path each takes, the bit-for-bit expectations of the
exact cases, the float64 restatement and the per-element tolerance MARGIN x bound x 2^-24 of the float cases are defined and
proven there -- then the Python wrappers of core/renderer_nr.py and core/renderer_utils.py.

Every output and scratch buffer sits between guard words and is itself filled with the guard pattern (a NaN): an element that is
not written is a NaN in the result, a word written outside is seen afterwards.  Every call runs twice and the bits must agree,
except where float atomics order the sum: the (A, t) gradients of d3m_grid_warp_backward's float cases with more than one workgroup
per entry, and grad_src of d3m_warp_resample_backward's float cases.

Each float case prints the largest achieved |got - ref| / bound per output (`pytest -s`); the figures of record are in
docs/EXPERIMENTS.md, section I."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import nr_helper_scenes as S
import test_nr_helpers_host as H
from conftest import kernels_launched
from test_gpu_loss_reductions import Check as _Check, _bits, _untouched
from test_gpu_param_reductions import GUARD_BITS, Guarded

pytestmark = pytest.mark.gpu

D3M_OK, D3M_ERR_INVALID = 0, 1          # include/d3m_raster.h


class Check(_Check):
    """the loss tests' collector, with a per-element tolerance that prints what was achieved"""

    def bounded(self, entry, what, got, want, tol):
        if tol is None:
            return self.exact(what, got, want)
        got, want, tol = (np.asarray(x, np.float64).reshape(-1) for x in (got, want, tol))
        if got.shape != want.shape:
            return self.failures.append((what, "shape", got.shape, want.shape))
        err = np.abs(got - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(tol > 0, err / np.where(tol > 0, tol, 1), np.where(err == 0, 0.0, np.inf))
        worst = float(np.nanmax(ratio)) if ratio.size else 0.0
        print(f"NRHELPER {entry} {S.case_id(self.c)} {what} err/bound={worst * S.MARGIN:.3e}")
        if not bool((err <= tol).all()):             # (a NaN fails)
            self.failures.append((what, "largest err / tolerance", worst, "at", int(np.nanargmax(ratio)), "NaN" * bool(np.isnan(err).any())))


def _dev(x, dtype=torch.float32):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dtype).cuda().contiguous()


def _p(x):
    from deep3dmap_amd import _lib
    return _lib.ptr(x.inner if isinstance(x, Guarded) else x)


def _run(name, *args, expect=D3M_OK):
    """the entry point on the current stream; every Guarded among the arguments is checked afterwards"""
    from deep3dmap_amd import _lib
    rc = getattr(_lib.lib(), name)(*[_p(a) if isinstance(a, (Guarded, torch.Tensor)) or a is None else a for a in args],
                                   _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, (name, rc)
    for a in args:
        assert not isinstance(a, Guarded) or a.intact(), (name, "guard words were written")


def _np(g):
    return None if g is None else g.inner.cpu().numpy()


def _same(a, b):
    return all((x is None and y is None) or np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


# ---- d3m_view_transform / _backward ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", S.view_cases(), ids=S.case_id)
def test_view_transform_at_size(c):
    chk = Check(c)
    inp = S.view_inputs(c)
    view, g_rot, g_trans = _dev(inp["view"]), _dev(inp["g_rot"]), _dev(inp["g_trans"])

    def forward():
        rot, trans = Guarded((c.B, 9)), Guarded((c.B, 3))
        _run("d3m_view_transform", view, c.n, rot, trans, c.B)
        return _np(rot), _np(trans)

    def backward(with_rot, with_trans):
        g_view = Guarded((c.B, c.n))
        _run("d3m_view_transform_backward", view, c.n, g_rot if with_rot else None, g_trans if with_trans else None, g_view, c.B)
        return (_np(g_view),)
    with kernels_launched() as k:
        got = forward()
    assert k.names == {"k_view_transform"}, k.names
    chk.twice("forward", got, forward())
    (R, Rtol), (t, ttol), _ = H.view_reference(c)
    chk.bounded("view_transform", "rot", got[0], R, Rtol)
    chk.exact("trans", got[1], t)
    for with_rot, with_trans in ((True, True), (False, True), (True, False), (False, False)):
        what = f"backward rot={int(with_rot)} trans={int(with_trans)}"
        gv = backward(with_rot, with_trans)
        chk.twice(what, gv, backward(with_rot, with_trans))
        want, tol = H.view_reference(c, with_rot, with_trans)[2]
        chk.bounded("view_transform_backward", what + " angles", gv[0][:, :3], want[:, :3], None if tol is None else tol[:, :3])
        chk.exact(what + " translation", gv[0][:, 3:], want[:, 3:])
        if not with_rot:
            chk.exact(what + " zero angles", gv[0][:, :3], np.zeros((c.B, 3)))
    chk.done()


# ---- d3m_grid_warp / _backward -----------------------------------------------------------------------------------------------------------
def _grid_dev(c):
    inp = S.grid_inputs(c)
    return inp, {k: _dev(inp[k]) for k in ("depth", "inv_K", "K", "A", "t", "g3", "g2")}


@pytest.mark.parametrize("c", S.grid_forward_cases(), ids=S.case_id)
def test_grid_warp_at_shape(c):
    chk = Check(c)
    inp, d = _grid_dev(c)
    crop = None if c.crop is None else (ctypes.c_int * 4)(*c.crop)
    for threeD in (True, False):
        def forward():
            out = Guarded((c.B, c.H * c.W, 3 if threeD else 2))
            _run("d3m_grid_warp", d["depth"], d["inv_K"], c.kb, d["A"], d["t"], inp["cz"], None if threeD else d["K"], c.kb, crop,
                 out, c.B, c.H, c.W)
            return (_np(out),)
        what = "3-D" if threeD else "2-D"
        with kernels_launched() as k:
            got = forward()
        assert k.names == {"k_grid_warp"}, k.names
        chk.twice(what, got, forward())
        chk.bounded("grid_warp", what, got[0], *H.grid_forward_reference(c, threeD))
    chk.done()


def test_grid_warp_of_a_one_row_map_divides_by_zero_as_the_reference_does():
    """H = 1 with K: v / (H - 1) is an infinity of v's sign (pinned as the reference's behaviour, not a defect); u is exact"""
    r = H.ONE_ROW
    out = Guarded((1, 5, 2))
    _run("d3m_grid_warp", _dev(r["depth"]), _dev(r["inv_K"]), 1, _dev(r["A"]), _dev(r["t"]), r["cz"], _dev(r["K"]), 1, None, out, 1, 1, 5)
    got, want = _np(out), H.one_row_grid()
    assert np.array_equal(_bits(got[..., 0]), _bits(want[..., 0])) and np.array_equal(got[..., 1], want[..., 1].astype(np.float32))


NULL_COMBINATION_SHAPES = ((3, 17, 33), (2, 17, 65))          # a plain store and two workgroups per entry


@pytest.mark.parametrize("c", S.grid_backward_cases(), ids=S.case_id)
def test_grid_warp_backward_at_shape(c):
    chk = Check(c)
    inp, d = _grid_dev(c)
    HW = c.H * c.W
    atomics = S.grid_warp_path(c.B, HW) == "atomics"
    combos = list(itertools.product((True, False), repeat=3)) if (c.B, c.H, c.W) in NULL_COMBINATION_SHAPES else [(True, True, True)]
    for threeD in (True, False):
        ref = H.grid_backward_reference(c, threeD)

        def backward(wd, wr, wt):
            outs = [Guarded((c.B, HW)) if wd else None, Guarded((c.B, 9)) if wr else None, Guarded((c.B, 3)) if wt else None]
            _run("d3m_grid_warp_backward", d["depth"], d["inv_K"], c.kb, d["A"], d["t"], inp["cz"], None if threeD else d["K"], c.kb,
                 d["g3"] if threeD else d["g2"], *outs, c.B, c.H, c.W)
            return [_np(o) for o in outs]
        for wd, wr, wt in combos:
            what = f"{'3-D' if threeD else '2-D'} depth={int(wd)} rot={int(wr)} trans={int(wt)}"
            with kernels_launched() as k:
                got = backward(wd, wr, wt)
            # the (A, t) sums of more than one workgroup per entry are atomics into arrays zeroed first; one workgroup stores
            zeroed = {"k_zero_fill"} if atomics and (wr or wt) else set()
            assert k.names == {"k_grid_warp_backward"} | zeroed, (what, k.names)
            again = backward(wd, wr, wt)
            # float atomics order the (A, t) sums of a float case with more than one workgroup per entry: exempt
            chk.twice(what, got[:1] if atomics and c.kind != "exact" else got, again[:1] if atomics and c.kind != "exact" else again)
            for name, g in zip(("g_depth", "g_A", "g_t"), got):
                if g is not None:
                    chk.bounded("grid_warp_backward", f"{what} {name}", g, *ref[name])
    chk.done()


# ---- d3m_depth_normals / _backward -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", S.normal_cases(), ids=S.case_id)
def test_depth_normals_at_shape(c):
    chk = Check(c)
    inp = S.normal_inputs(c)
    depth, inv_K, g = _dev(inp["depth"]), _dev(inp["inv_K"]), _dev(inp["g"])

    def forward():
        out = Guarded((c.B, c.H, c.W, 3))
        _run("d3m_depth_normals", depth, inv_K, c.B, out, c.B, c.H, c.W)
        return (_np(out),)

    def backward():
        out = Guarded((c.B, c.H * c.W))
        _run("d3m_depth_normals_backward", depth, inv_K, c.B, g, out, c.B, c.H, c.W)
        return (_np(out),)
    (n, ntol), (gd, gtol) = H.normals_reference(c)
    with kernels_launched() as k:
        got, grad = forward(), backward()
    assert k.names == {"k_depth_normals", "k_depth_normals_backward"}, k.names
    chk.twice("forward", got, forward())
    chk.twice("backward", grad, backward())
    chk.bounded("depth_normals", "normal", got[0], n, ntol)                      # every element against its own bound
    chk.bounded("depth_normals_backward", "g_depth", grad[0], gd, gtol)
    border = np.ones((c.H, c.W), bool)
    border[1:-1, 1:-1] = False
    want = np.zeros((c.B, int(border.sum()), 3), np.float32)
    want[..., 2] = H.BORDER_NORMAL_Z
    chk.exact("the border is (0, 0, 1) / (1 + 1e-7)", got[0][:, border], want)
    if not (c.H > 2 and c.W > 2):
        chk.exact("no interior: the gradient is zero", grad[0], np.zeros((c.B, c.H * c.W)))
    chk.done()


# ---- d3m_textures_from_im / _backward -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", S.tex_cases(), ids=S.case_id)
def test_textures_from_im_at_shape(c):
    chk = Check(c)
    inp = S.tex_inputs(c)
    im, g = _dev(inp["im"]), _dev(inp["g"])
    faces, per = 2 * (c.H - 1) * (c.W - 1), 8 if c.ts == 2 else 1

    def forward():
        out = Guarded((c.B, faces, per, c.C))
        _run("d3m_textures_from_im", im, out, c.B, c.C, c.H, c.W, c.ts)
        return (_np(out),)

    def backward():
        out = Guarded((c.B, c.C, c.H, c.W))
        _run("d3m_textures_from_im_backward", g, out, c.B, c.C, c.H, c.W, c.ts)
        return (_np(out),)
    tex, g_im = H.tex_reference(c)
    with kernels_launched() as k:
        got, grad = forward(), backward()
    assert k.names == {"k_textures_from_im", "k_textures_from_im_backward"}, k.names
    chk.twice("forward", got, forward())
    chk.twice("backward", grad, backward())
    chk.exact("textures", got[0], tex)
    chk.exact("g_im", grad[0], g_im)
    chk.done()


# ---- d3m_warp_resample / _backward ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", S.resample_cases(), ids=S.case_id)
def test_warp_resample_at_shape(c):
    from deep3dmap_amd import _lib
    chk = Check(c)
    inp = S.resample_inputs(c)
    d = {k: _dev(inp[k]) for k in ("depth", "inv_K", "K", "A", "t", "src", "src_n", "g", "prefill")}
    hw, HW, exact = c.h * c.w, c.H * c.W, c.kind in ("exact", "zoom")
    parts = int(_lib.lib().d3m_warp_resample_partials(c.h, c.w))
    assert parts == S.resample_parts(c.h, c.w)
    head = (d["depth"], d["inv_K"], c.kb, d["K"], c.kb, d["A"], d["t"], inp["cz"], d["src"], c.C)

    def forward():
        out, out_n = Guarded((c.B, c.C, hw)), Guarded((c.B, c.Cn, hw)) if c.Cn else None
        _run("d3m_warp_resample", *head, d["src_n"], c.Cn, out, out_n, c.B, c.h, c.w, c.H, c.W)
        return _np(out), _np(out_n)

    def backward(with_src=True, with_depth=True):
        g_src = Guarded((c.B, c.C, HW)) if with_src else None
        if with_src:
            g_src.inner.copy_(d["prefill"])               # integers: the kernel adds to what is there
        g_depth, partials = Guarded((c.B, hw)) if with_depth else None, Guarded((c.B * parts * 12,))      # exactly the stated size
        _run("d3m_warp_resample_backward", *head, d["g"], g_src, g_depth, partials, c.B, c.h, c.w, c.H, c.W)
        return _np(g_src), _np(g_depth), _np(partials)
    ref = H.resample_reference(c)
    with kernels_launched() as k:
        got = forward()
    assert k.names == {"k_warp_resample"}, k.names
    chk.twice("forward", got, forward())
    chk.bounded("warp_resample", "bilinear", got[0], *ref["out"])
    if c.Cn:
        chk.exact("nearest (no texel may differ)", got[1], ref["near"])
    for with_src, with_depth in ((True, True), (False, True), (True, False), (False, False)):
        what = f"backward src={int(with_src)} depth={int(with_depth)}"
        with kernels_launched() as k:
            grads = backward(with_src, with_depth)
        assert k.names == {"k_warp_resample_backward"}, k.names
        again = backward(with_src, with_depth)
        # float atomics order grad_src of a float case: exempt; grad_depth and the partial sums have one order
        chk.twice(what, grads if exact else grads[1:], again if exact else again[1:])
        if with_src:
            chk.bounded("warp_resample_backward", what + " g_src", grads[0], *ref["g_src"])
        if with_depth:
            chk.bounded("warp_resample_backward", what + " g_depth", grads[1], *ref["g_depth"])
        chk.bounded("warp_resample_backward", what + " partials", grads[2], *ref["partials"])
    chk.done()


# ---- refusals: D3M_ERR_INVALID, nothing launched, nothing written ----------------------------------------------------------------------------
def _buffers(name, defaults):
    """a device buffer for every pointer of the entry point, sized for the default (accepted) arguments; outputs are Guarded"""
    B = defaults["B"]
    HW = defaults.get("H", 1) * defaults.get("W", 1)
    hw = defaults.get("h", 1) * defaults.get("w", 1)
    C = defaults.get("C", 1)
    sizes = dict(view=B * 6, rot=B * 9, trans=B * 3, g_rot=B * 9, g_trans=B * 3, g_view=B * 6, depth=B * max(HW, hw), inv_K=B * 9, K=B * 9,
                 out=B * max(HW * 3, hw * C), g_out=B * max(HW * 3, hw * C), g_depth=B * max(HW, hw), normal=B * HW * 3, g_normal=B * HW * 3,
                 im=B * C * HW, tex=B * 2 * HW * 8 * C, g_tex=B * 2 * HW * 8 * C, g_im=B * C * HW, src=B * C * HW, src_n=B * HW,
                 out_n=B * hw, g_src=B * C * HW, partials=B * 32 * 12)
    outputs = {"d3m_view_transform": ("rot", "trans"), "d3m_view_transform_backward": ("g_view",), "d3m_grid_warp": ("out",),
               "d3m_grid_warp_backward": ("g_depth", "g_rot", "g_trans"), "d3m_depth_normals": ("normal",),
               "d3m_depth_normals_backward": ("g_depth",), "d3m_textures_from_im": ("tex",), "d3m_textures_from_im_backward": ("g_im",),
               "d3m_warp_resample": ("out", "out_n"), "d3m_warp_resample_backward": ("g_src", "g_depth", "partials")}[name]
    bufs = {}
    for k, v in defaults.items():
        if v == H.P:
            bufs[k] = Guarded((sizes[k],)) if k in outputs else torch.ones(sizes[k], dtype=torch.float32, device="cuda")
    return bufs, outputs


@pytest.mark.parametrize("name", sorted(H.REFUSALS))
def test_refusals_launch_nothing_and_write_nothing(name):
    defaults, cases = H.REFUSALS[name]
    bufs, outputs = _buffers(name, defaults)
    for over in cases:
        args = dict(defaults, **bufs)
        args.update(over)
        with kernels_launched() as k:
            _run(name, *args.values(), expect=D3M_ERR_INVALID)
        assert not k.names, (over, k.names)
        for o in outputs:
            assert bufs[o].intact() and _untouched(_np(bufs[o])), (over, o)
    # the accepted forms next to them run
    for over in [{}] + H.ACCEPTED.get(name, []):
        args = dict(defaults, **bufs)
        args.update(over)
        with kernels_launched() as k:
            _run(name, *args.values())
        assert len(k.names) == 1, (over, k.names)


# ---- the Python wrappers -------------------------------------------------------------------------------------------------------------------
def _t(x, shape=None, grad=False):
    t = _dev(x)
    return (t if shape is None else t.reshape(shape)).requires_grad_(grad)


def _sum_tolerance(ref, tol, B):
    """of a gradient summed over the batch by the wrapper: the entries' tolerances and B roundings of their absolute sum"""
    return tol.sum(0, keepdims=True) + S.tolerance(B * np.abs(ref).sum(0, keepdims=True))


@pytest.mark.parametrize("threeD", [True, False], ids=["3-D", "2-D"])
def test_grid_warp_wrapper_with_a_shared_motion(threeD):
    """A [1,3,3] and t [1,1,3] with B = 3 on a 17 x 33 map, a depth map that is not contiguous: the summed gradient keeps the input's
    shape; then every needs_input_grad subset"""
    from deep3dmap_amd.core.renderer_nr import _GridWarp
    c = S.GridCase(3, 17, 33, 1, None, "float")
    chk = Check(c)
    inp = dict(S.grid_inputs(c))
    inp["A"], inp["t"] = np.repeat(inp["A"][:1], c.B, 0), np.repeat(inp["t"][:1], c.B, 0)
    a = S.in_arith(inp, "err", H.GRID_KEYS + ("K", "g3", "g2"))
    K = None if threeD else a["K"]
    want = S.grid_warp(a["depth"], a["inv_K"], a["A"], a["t"], inp["cz"], K, None, c.H, c.W)
    gd, terms = S.grid_warp_backward(a["depth"], a["inv_K"], a["A"], a["t"], inp["cz"], K, a["g3"] if threeD else a["g2"], c.H, c.W)
    sums = S.reduce_terms(terms, S.reduce_chain(c.H * c.W, S.grid_warp_split(c.B, c.H * c.W)))
    wide = torch.zeros(c.B, c.H, 2 * c.W, device="cuda")
    wide[:, :, ::2] = _t(inp["depth"], (c.B, c.H, c.W))
    g = _t(inp["g3"]) if threeD else _t(inp["g2"], (c.B, c.H, c.W, 2))
    for need in itertools.product((True, False), repeat=3):
        if not any(need):
            continue
        depth = wide[:, :, ::2].detach().requires_grad_(need[0])
        assert not depth.is_contiguous()
        A, t = _t(inp["A"][:1], (1, 3, 3), need[1]), _t(inp["t"][:1], (1, 1, 3), need[2])
        out = _GridWarp.apply(depth, _t(inp["inv_K"], (1, 3, 3)), A, t, inp["cz"], None if threeD else _t(inp["K"], (1, 3, 3)), None)
        assert out.shape == ((c.B, c.H * c.W, 3) if threeD else (c.B, c.H, c.W, 2))
        out.backward(g)
        what = f"need={need}"
        if all(need):
            chk.bounded("_GridWarp", "forward", out.detach().cpu().numpy(), want.v, S.tolerance(want.e))
        for x, on in zip((depth, A, t), need):
            assert (x.grad is not None) == on, what
        if need[0]:
            chk.bounded("_GridWarp", what + " g_depth", depth.grad.cpu().numpy(), gd.v, S.tolerance(gd.e))
        if need[1]:
            assert A.grad.shape == (1, 3, 3)
            chk.bounded("_GridWarp", what + " g_A", A.grad.cpu().numpy(), sums.v[:, :9].sum(0),
                        _sum_tolerance(sums.v[:, :9], S.tolerance(sums.e[:, :9]), c.B))
        if need[2]:
            assert t.grad.shape == (1, 1, 3)
            chk.bounded("_GridWarp", what + " g_t", t.grad.cpu().numpy(), sums.v[:, 9:].sum(0),
                        _sum_tolerance(sums.v[:, 9:], S.tolerance(sums.e[:, 9:]), c.B))
    chk.done()


def test_depth_normals_and_textures_wrappers_off_the_square():
    from deep3dmap_amd.core.renderer_nr import _DepthNormals
    from deep3dmap_amd.core.renderer_utils import get_textures_from_im, get_transform_matrices
    c = S.NormalCase(2, 9, 5, "float")
    chk = Check(c)
    inp = S.normal_inputs(c)
    (n, ntol), (gd, gtol) = H.normals_reference(c)
    wide = torch.zeros(c.B, 2 * c.H, c.W, device="cuda")
    wide[:, ::2] = _t(inp["depth"], (c.B, c.H, c.W))
    depth = wide[:, ::2].detach().requires_grad_(True)
    assert not depth.is_contiguous()
    out = _DepthNormals.apply(depth, _t(inp["inv_K"], (c.B, 3, 3)))
    out.backward(_t(inp["g"]))
    chk.bounded("_DepthNormals", "normal", out.detach().cpu().numpy(), n, ntol)
    chk.bounded("_DepthNormals", "g_depth", depth.grad.cpu().numpy(), gd, gtol)
    for tc in (S.TexCase(2, 3, 7, 2, 1), S.TexCase(3, 4, 6, 7, 2)):
        ti = S.tex_inputs(tc)
        tex, g_im = H.tex_reference(tc)
        im = _t(ti["im"], grad=True)
        got = get_textures_from_im(im, tx_size=tc.ts)
        assert got.shape == (tc.B, 2 * (tc.H - 1) * (tc.W - 1), tc.ts, tc.ts, tc.ts, tc.C)
        got.backward(_t(ti["g"]).reshape(got.shape))
        chk.exact(f"get_textures_from_im {tc}", got.detach().cpu().numpy(), tex)
        chk.exact(f"get_textures_from_im {tc} gradient", im.grad.cpu().numpy(), g_im)
    with pytest.raises(NotImplementedError):
        get_textures_from_im(im, tx_size=3)
    vc = S.ViewCase(65, 5, "hashed")
    vi = S.view_inputs(vc)
    (R, Rtol), (t, _), (gv, gvtol) = H.view_reference(vc)
    view = _t(vi["view"], grad=True)
    rot, trans = get_transform_matrices(view)
    assert rot.shape == (65, 3, 3) and trans.shape == (65, 1, 3)
    torch.autograd.backward([rot, trans], [_t(vi["g_rot"], (65, 3, 3)), _t(vi["g_trans"], (65, 1, 3))])
    chk.bounded("get_transform_matrices", "rot", rot.detach().cpu().numpy(), R, Rtol)
    chk.exact("get_transform_matrices trans", trans.detach().cpu().numpy(), t)
    chk.bounded("get_transform_matrices", "g_view", view.grad.cpu().numpy(), gv, gvtol)
    # only the rotation is used: the translation's gradient is absent, not garbage
    view2 = _t(vi["view"], grad=True)
    get_transform_matrices(view2)[0].backward(_t(vi["g_rot"], (65, 3, 3)))
    chk.bounded("get_transform_matrices", "g_view, rot alone", view2.grad.cpu().numpy()[:, :3], H.view_reference(vc, True, False)[2][0][:, :3],
                gvtol[:, :3])
    chk.exact("g_view, rot alone: translation", view2.grad.cpu().numpy()[:, 3:], np.zeros((65, 2)))
    chk.done()


def test_warp_resample_wrapper_off_the_square():
    """a 5 x 33 source looked up from a 9 x 17 map with a shared motion, a mask for the nearest lookup, and needs_input_grad subsets"""
    from deep3dmap_amd.core.renderer_nr import _WarpResample
    c = S.ResampleCase(2, 9, 17, 5, 33, 1, 2, 2, "general")
    chk = Check(c)
    inp = dict(S.resample_inputs(c))
    inp["A"], inp["t"] = np.repeat(inp["A"][:1], c.B, 0), np.repeat(inp["t"][:1], c.B, 0)
    a = S.in_arith(inp, "err", H.RES_KEYS)
    args = (a["depth"], a["inv_K"], a["K"], a["A"], a["t"], inp["cz"], a["src"])
    out, near, _ = S.warp_resample(*args, inp["src_n"], c.h, c.w, c.H, c.W)
    assert S.nearest_clearance(c, inp) < 1
    contrib, gd, terms = S.warp_resample_backward(*args, a["g"], c.h, c.w, c.H, c.W)
    parts = S.resample_partials(terms, S.resample_parts(c.h, c.w))
    g_src, mag = S.scatter_src(contrib, c.B, c.C, c.H * c.W)
    for need in ((True, True, True, True), (True, False, False, False), (False, True, False, False), (False, False, True, False),
                 (False, False, False, True)):
        depth, src = _t(inp["depth"], (c.B, c.h, c.w), need[0]), _t(inp["src"], (c.B, c.C, c.H, c.W), need[1])
        A, t = _t(inp["A"][:1], (1, 3, 3), need[2]), _t(inp["t"][:1], (1, 1, 3), need[3])
        got, got_n = _WarpResample.apply(depth, src, _t(inp["src_n"], (c.B, c.Cn, c.H, c.W)), _t(inp["inv_K"], (c.B, 3, 3)),
                                         _t(inp["K"], (c.B, 3, 3)), A, t, inp["cz"])
        assert got.shape == (c.B, c.C, c.h, c.w) and got_n.shape == (c.B, c.Cn, c.h, c.w) and not got_n.requires_grad
        got.backward(_t(inp["g"], (c.B, c.C, c.h, c.w)))
        what = f"need={need}"
        for x, on in zip((depth, src, A, t), need):
            assert (x.grad is not None) == on, what
        if all(need):
            chk.bounded("_WarpResample", "bilinear", got.detach().cpu().numpy(), out.v, S.tolerance(out.e))
            chk.exact("nearest", got_n.cpu().numpy(), near)
        if need[0]:
            chk.bounded("_WarpResample", what + " g_depth", depth.grad.cpu().numpy(), gd.v, S.tolerance(gd.e))
        if need[1]:
            chk.bounded("_WarpResample", what + " g_src", src.grad.cpu().numpy(), g_src, H.src_tolerance(contrib, mag))
        total, tol = parts.v.sum((0, 1)), S.tolerance(parts.e.sum((0, 1)) + (c.B + parts.shape[1]) * np.abs(parts.v).sum((0, 1)))
        if need[2]:
            assert A.grad.shape == (1, 3, 3)
            chk.bounded("_WarpResample", what + " g_A", A.grad.cpu().numpy(), total[:9], tol[:9])
        if need[3]:
            assert t.grad.shape == (1, 1, 3)
            chk.bounded("_WarpResample", what + " g_t", t.grad.cpu().numpy(), total[9:], tol[9:])
    chk.done()


def test_the_guard_pattern_is_a_nan():
    assert np.isnan(np.array([GUARD_BITS], np.int32).view(np.float32)[0])
