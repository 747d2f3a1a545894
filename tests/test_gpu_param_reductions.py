"""The fixed-order parameter reductions beyond one workgroup: k_camera_params_partial / _finish (csrc/d3m_camera_grad.h) and
k_light_params_partial / _finish (csrc/d3m_light_grad.h) driven through the C ABI at 1 ... 300 001 elements, 1 ... 300 views,
against the float64 references of tests/test_param_reductions_host.py (cases, inputs, references and the tolerance
(D 2^-24 + 4 E32) * bound are defined and proven sharp there), and through the render nodes at the benchmark's mesh.

Every call runs with guard words around the workspace and around every output (NaN bit patterns: an entry that is read
before it is written, or not written at all, is a NaN in the result; a word written outside is seen afterwards).

Each case prints D 2^-24, E32 and the achieved |got - ref| / bound of every parameter (`pytest -s`); the figures of record are
in docs/EXPERIMENTS.md, section G."""
import ctypes
import math

import pytest
import torch

import test_gpu_light_params as light_tests
import test_param_reductions_host as H
from conftest import kernels_launched
from test_gpu_camera_params import (D3M_ERR_INVALID, D3M_OK, NEW_KERNELS as CAMERA_KERNELS, _cam_grad, _rel, _run_inside,
                                    _run_outside, _targets)

pytestmark = pytest.mark.gpu

LIGHT_KERNELS = {"k_light_params_partial", "k_light_params_finish"}
GUARD_WORDS = 1024                  # 4 KiB either side
GUARD_BITS = 0x7FC5A5A5             # a quiet NaN


class Guarded:
    """A float32 device buffer of `shape` between two runs of guard words, itself filled with the guard pattern"""

    def __init__(self, shape):
        self.n = int(math.prod(shape))
        self.raw = torch.full((self.n + 2 * GUARD_WORDS,), GUARD_BITS, dtype=torch.int32, device="cuda")
        self.inner = self.raw[GUARD_WORDS:GUARD_WORDS + self.n].view(torch.float32).view(*shape)

    def intact(self):
        lo, hi = self.raw[:GUARD_WORDS], self.raw[GUARD_WORDS + self.n:]
        return bool((lo == GUARD_BITS).all()) and bool((hi == GUARD_BITS).all())


def _finish_call(rc, outs, ws, expect_rc):
    torch.cuda.synchronize()
    assert rc == expect_rc, rc
    assert ws.intact(), "the workspace's guard words were written"
    for o in outs:
        assert o is None or o.intact(), "an output's guard words were written"
    return [None if o is None else o.inner.cpu() for o in outs]


# ---- the two entry points ---------------------------------------------------------------------------------------------------
class CameraCall:
    def __init__(self, c, inp):
        from deep3dmap_amd import _lib
        from deep3dmap_amd.neural_renderer import cameras
        self.c, self.v = c, inp["vertices"].cuda()
        ps = [p.cuda() for p in inp["params"]]
        if c.kind == "projection":
            self.p = cameras.projection_params(self.v, ps[0], ps[1], ps[2], ps[3], H.ORIG_SIZE)
            self.pick = (4, 3, 0, 5)                          # K, R, t, dist among d3m_camera_grad's fields
        else:
            fn = cameras.look_at_params if c.kind == "look_at" else cameras.look_params
            self.p = fn(self.v, *ps, _perspective_angle=H.ANGLE)
            self.pick = (0, 1, 2)
        self.need = int(_lib.lib().d3m_camera_params_backward_workspace_bytes(c.views, c.n, self.p["mode"]))
        assert self.need == 4 * c.views * (H.parts_of(c.n) * H.CAM_SUMS + H.CAM_ROW)

    def __call__(self, g, workspace_bytes=None, expect_rc=D3M_OK):
        from deep3dmap_amd import _lib
        from deep3dmap_amd.neural_renderer import cameras
        cam, _keep = cameras._camera_struct(self.p, self.v.device)
        basis, _bk = cameras.basis_struct(self.p, "vectors")
        outs = [None if t is None else Guarded(t.shape) for t in cameras.camera_inputs(self.p)]
        ws = Guarded((self.need // 4,))
        grads = _cam_grad([None if o is None else o.inner for o in outs])
        rc = _lib.lib().d3m_camera_params_backward(
            _lib.ptr(self.v), self.v.shape[0], ctypes.byref(cam), ctypes.byref(basis) if basis is not None else None,
            _lib.ptr(g), ctypes.byref(grads), self.c.views, self.c.n, _lib.ptr(ws.inner),
            self.need if workspace_bytes is None else workspace_bytes, _lib.stream_ptr())
        res = _finish_call(rc, outs, ws, expect_rc)
        return [res[k].reshape(res[k].shape[0], -1) for k in self.pick]


class LightCall:
    def __init__(self, c, inp):
        from deep3dmap_amd import _lib
        self.c, self.v = c, inp["vertices"].cuda()
        self.tri = inp["tri"].cuda() if c.grid is None else None
        self.tri_batch = 1 if c.grid is None else -c.grid[1]
        self.num_tri = inp["num_tri"]
        self.light = [p.cuda() for p in inp["light"]]
        self.need = int(_lib.lib().d3m_light_params_backward_workspace_bytes(c.views, self.num_tri, c.fill_back))
        assert self.need == 4 * c.views * (H.parts_of(c.n) * H.LIGHT_SUMS + H.LIGHT_ROW)

    def __call__(self, g, workspace_bytes=None, expect_rc=D3M_OK):
        from deep3dmap_amd import _lib
        from deep3dmap_amd.neural_renderer.rasterize import _light_struct
        outs = [Guarded(t.shape) for t in self.light]
        ws = Guarded((self.need // 4,))
        rc = _lib.lib().d3m_light_params_backward(
            _lib.ptr(self.v), self.v.shape[0], _lib.ptr(self.tri), self.tri_batch, _lib.ptr(g), self.c.views,
            ctypes.byref(_light_struct(self.light)), ctypes.byref(_light_struct([o.inner for o in outs], self.light)),
            self.v.shape[1], self.num_tri, self.c.fill_back, _lib.ptr(ws.inner),
            self.need if workspace_bytes is None else workspace_bytes, _lib.stream_ptr())
        res = _finish_call(rc, outs, ws, expect_rc)
        return [r.reshape(r.shape[0], -1) for r in res]


# ---- checks 1, 2, 3 and 5 of a case (4, the guard words, rides on every call) ---------------------------------------------------
def _bits_equal(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def _check_case(what, c, call, inp, ref, names):
    g = inp["upstream"].cuda()
    failures = []
    # 1. dense and 2. sparse upstream against float64; 5. a second call gives the same bits
    for mode in ("dense", "sparse"):
        gm = g if mode == "dense" else (g * inp["keep"].cuda()[:, :, None]).contiguous()
        got = call(gm)
        if not _bits_equal(got, call(gm)):
            failures.append((mode, "two calls differ"))
        for k, name in enumerate(names):
            want, bound, tol = ref.ref[mode][k], ref.bound[mode][k], ref.tolerance(mode, k)
            assert got[k].shape == want.shape, (name, got[k].shape, want.shape)
            err = (got[k].double() - want).abs()
            achieved = float((err / bound.clamp_min(1e-300))[bound > 0].max()) if bool((bound > 0).any()) else 0.0
            D = H.chain_length(c.n, c.views, ref.summed[k])
            print(f"REDUCTION {what} {H.case_id(c)} {name} {mode} D*2^-24={D * H.EPS32:.3e} E32={ref.e32[mode][k]:.3e} "
                  f"achieved={achieved:.3e}")
            if not bool((err <= tol).all()):            # (a NaN fails)
                failures.append((mode, name, "largest |got - ref| / tol", float((err / tol.clamp_min(1e-300)).max())))
    # 3. one-hot upstream in the last view: that term alone, and exact zeros in every other view
    one = torch.zeros_like(g)
    for j, i in enumerate(ref.onehot):
        one[-1, i] = g[-1, i]
        got = call(one)
        one[-1, i] = 0
        for k, name in enumerate(names):
            tol, e = ref.term_tolerance(k)
            row = got[k][-1].double()
            err = (row - ref.term[k][j]).abs()
            if j == 0:
                print(f"REDUCTION {what} {H.case_id(c)} {name} one-hot 8*2^-24={8 * H.EPS32:.3e} E32_term={e:.3e}")
            if not bool((err <= tol[j]).all()):
                failures.append(("one-hot", i, name, float((err / tol[j].clamp_min(1e-300)).max())))
            if got[k].shape[0] > 1 and not bool((got[k][:-1].view(torch.int32) << 1 == 0).all()):
                failures.append(("one-hot", i, name, "another view's gradient is not zero"))
    assert not failures, "\n".join(" ".join(map(str, f)) for f in failures)


@pytest.mark.parametrize("c", H.camera_cases(), ids=H.case_id)
def test_camera_params_backward_at_size(c):
    inp = H.camera_inputs(c)
    _check_case("camera", c, CameraCall(c, inp), inp, H.camera_reference(c, inp), H.CAMERA_NAMES[c.kind])


@pytest.mark.parametrize("c", H.light_cases(), ids=H.case_id)
def test_light_params_backward_at_size(c):
    inp = H.light_inputs(c)
    _check_case("light", c, LightCall(c, inp), inp, H.light_reference(c, inp), H.LIGHT_NAMES)


# ---- 4. a workspace one byte short is refused before anything is launched ---------------------------------------------------------
@pytest.mark.parametrize("n", [1, 1025, 131072, 300001])
def test_short_workspace_is_refused_and_launches_nothing(n):
    cc = H.CameraCase("projection", n, 3, False, True)
    lc = H.LightCase(n, 3, 0, None, True, True)
    for c, make, Call in ((cc, H.camera_inputs, CameraCall), (lc, H.light_inputs, LightCall)):
        inp = make(c)
        call = Call(c, inp)
        g = inp["upstream"].cuda()
        with kernels_launched() as k:
            got = call(g, workspace_bytes=call.need - 1, expect_rc=D3M_ERR_INVALID)
            torch.cuda.synchronize()
        assert not k.names, k.names
        for x in got:          # nothing was written: the outputs still hold the guard pattern
            assert bool((x.view(torch.int32) == GUARD_BITS).all())
        with kernels_launched() as k:
            call(g)
            torch.cuda.synchronize()
        assert (CAMERA_KERNELS if Call is CameraCall else LIGHT_KERNELS) <= k.names, k.names


# ---- 6, 7. through the render nodes at the benchmark's mesh ----------------------------------------------------------------------
BENCH_GRID, BENCH_VIEWS, BENCH_SIZE = 225, 2, 128


def _bench_scene():
    from deep3dmap_amd import synthetic
    v, tri = synthetic.grid_mesh(BENCH_GRID)
    tex = synthetic.random_textures(tri.shape[0], 2)
    assert v.shape[0] == 50625 and 2 * tri.shape[0] == 200704
    return (torch.from_numpy(v)[None], torch.from_numpy(tri)[None], torch.from_numpy(tex)[None],
            torch.from_numpy(synthetic.camera_ring(BENCH_VIEWS)))


@pytest.mark.parametrize("method", ["render", "render_fit_loss", "silhouettes"])
def test_learnable_eye_in_the_render_nodes_at_the_benchmarks_mesh(method):
    v, tri, tex, eyes = _bench_scene()
    v, tri, tex = v.cuda(), tri.int().cuda(), tex.float().cuda()
    B, size = BENCH_VIEWS, BENCH_SIZE
    targets = _targets(B, size)
    gen = torch.Generator(device="cuda").manual_seed(1)
    weights = tuple(torch.randn(B, *s, device="cuda", generator=gen) for s in ((3, size, size), (size, size), (size, size)))
    with kernels_launched() as k:
        im_in, s_in, g_in = _run_inside(method, "look_at", v, tri, tex, [eyes], size, False, targets, weights)
        torch.cuda.synchronize()
    assert CAMERA_KERNELS <= k.names, sorted(k.names)
    im_out, s_out, g_out = _run_outside(method, "look_at", v, tri, tex, [eyes], size, False, targets, weights)
    for a, b in zip(im_in, im_out):
        if method == "render_fit_loss":
            assert torch.allclose(a, b, rtol=1e-5, atol=0)
        else:
            assert torch.equal(a, b)
    assert g_in[0].shape == g_out[0].shape == (B, 3) and float(g_out[0].abs().max()) > 0
    rel = _rel(g_in[0].cpu(), g_out[0])
    print(f"REDUCTION node {method} eye gradient: largest deviation / largest entry = {rel:.3e}")
    assert rel <= 1e-4, (method, rel)


@pytest.mark.parametrize("per_view", [False, True])
def test_learnable_light_in_the_lit_node_at_the_benchmarks_mesh(per_view):
    from deep3dmap_amd import neural_renderer as nr
    from oracle import nr_oracle as O
    v, tri, tex, eyes = _bench_scene()
    B, size = BENCH_VIEWS, BENCH_SIZE
    light = light_tests._light(B, per_view)
    if per_view:        # one shared mesh; the oracle renders one view at a time (its light is one for the batch)
        with kernels_launched() as k:
            got = light_tests._render(nr, "cuda", v, tri, tex, light, eyes, size, False)
            torch.cuda.synchronize()
        parts = [light_tests._render(O, "cpu", v, tri, tex, [x[b] for x in light], eyes, size, False, views=[b])
                 for b in range(B)]
        ref = [torch.cat([p[j] for p in parts]) for j in range(3)] + [sum(p[3] for p in parts), sum(p[4] for p in parts)] + \
            [torch.stack([p[5 + j] for p in parts]) for j in range(5)]
    else:
        vb, tb, xb = v.repeat(B, 1, 1), tri.repeat(B, 1, 1), tex.repeat(B, 1, 1, 1, 1, 1)
        with kernels_launched() as k:
            got = light_tests._render(nr, "cuda", vb, tb, xb, light, eyes, size, False)
            torch.cuda.synchronize()
        ref = light_tests._render(O, "cpu", vb, tb, xb, light, eyes, size, False)
    assert LIGHT_KERNELS <= k.names, sorted(k.names)
    for j, (a, b) in enumerate(zip(got, ref)):
        rel = light_tests._rel(a, b.reshape(a.shape))
        print(f"REDUCTION node light per_view={int(per_view)} output {j}: largest deviation / largest entry = {rel:.3e}")
        assert rel < (1e-5 if j < 3 else 1e-3), (j, rel)
