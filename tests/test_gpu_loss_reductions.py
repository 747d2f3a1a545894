"""The loss reductions at every grid shape and input layout: d3m_photometric_loss, d3m_sum_squared_error,
d3m_smooth_loss_forward/_backward and d3m_fit_loss_forward/_backward driven through the C ABI against the predictions of
tests/test_loss_reductions_host.py (cases, inputs, the path each case takes, the bit-for-bit expectations of the integer
cases and the float64 references, tolerance (D 2^-24 + 4 E32) * bound and sharpness proof of the float cases are there),
then the Python wrappers of core/losses.py at the shapes they broadcast or refuse.

Every output and the scratch buffer sit between guard words and are themselves filled with the guard pattern (a NaN): an
element that is not written is a NaN in the result, a word written outside is seen afterwards.  The scratch has exactly the
size the wrapper allocates.  Every call runs twice and the bits must agree.

Each float case prints D 2^-24, E32 and the achieved |loss - ref| / tolerance (`pytest -s`); the figures of record are in
docs/EXPERIMENTS.md, section H."""
import math

import numpy as np
import pytest
import torch

import test_loss_reductions_host as H
from conftest import kernels_launched
from test_gpu_param_reductions import GUARD_BITS, GUARD_WORDS, Guarded

pytestmark = pytest.mark.gpu

D3M_OK, D3M_ERR_INVALID = 0, 1          # include/d3m_raster.h
FIT_GRAD_OUT = 1.7


class Shifted(Guarded):
    """a Guarded buffer whose first element lies 4 bytes past a 16-byte boundary"""

    def __init__(self, shape):
        self.n = int(math.prod(shape))
        self.lo = GUARD_WORDS + 1
        self.raw = torch.full((self.n + 2 * GUARD_WORDS + 1,), GUARD_BITS, dtype=torch.int32, device="cuda")
        self.inner = self.raw[self.lo:self.lo + self.n].view(torch.float32).view(*shape)
        assert self.inner.data_ptr() % 16 == 4

    def intact(self):
        lo, hi = self.raw[:self.lo], self.raw[self.lo + self.n:]
        return bool((lo == GUARD_BITS).all()) and bool((hi == GUARD_BITS).all())


def _dev(x, off=False):
    """x as a flat float32 device buffer on a 16-byte boundary, or 4 bytes past one"""
    if x is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(x).astype(np.float32).reshape(-1))
    buf = torch.empty(t.numel() + 4, dtype=torch.float32, device="cuda")
    v = buf[1:1 + t.numel()] if off else buf[:t.numel()]
    v.copy_(t)
    assert v.data_ptr() % 16 == (4 if off else 0)
    return v


def _finish(rc, expect_rc, scratch, outs):
    torch.cuda.synchronize()
    assert rc == expect_rc, rc
    assert scratch is None or scratch.intact(), "the scratch buffer's guard words were written"
    for o in outs:
        assert o is None or o.intact(), "an output's guard words were written"
    return [None if o is None else o.inner.cpu().numpy() for o in outs]


def _ptr(x):
    from deep3dmap_amd import _lib
    return _lib.ptr(x.inner if isinstance(x, Guarded) else x)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def _same_bits(a, b):
    return all((x is None and y is None) or np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _untouched(x):
    return bool((_bits(x) == GUARD_BITS).all())


class Check:
    """collects what a case misses, so that one failure does not hide the next; asserts at the end"""

    def __init__(self, c):
        self.c, self.failures = c, []

    def exact(self, what, got, want):
        got, want = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
        if got.shape != want.shape or not np.array_equal(_bits(got), _bits(want)):
            bad = np.flatnonzero(_bits(got) != _bits(want)) if got.shape == want.shape else []
            first = int(bad[0]) if len(bad) else -1
            self.failures.append((what, "bits differ at", len(bad), "elements, first", first,
                                  None if first < 0 else (float(got[first]), float(want[first]))))

    def close(self, what, got, want, tol):
        if tol is None:
            return self.exact(what, got, want)
        err = np.abs(np.asarray(got, np.float64).reshape(-1) - np.asarray(want, np.float64).reshape(-1))
        tol = np.broadcast_to(np.asarray(tol, np.float64).reshape(-1), err.shape)
        if not bool((err <= tol).all()):             # (a NaN fails)
            with np.errstate(divide="ignore", invalid="ignore"):
                self.failures.append((what, "largest err / tol", float(np.nanmax(err / tol)), "NaN" * bool(np.isnan(err).any())))

    def loss(self, what, variant, got, ref):
        err = abs(float(got) - float(ref.loss))
        print(f"LOSS {H.case_id(self.c)} {variant} {what} D*2^-24={ref.D * H.EPS32:.3e} E32={ref.e32:.3e} "
              f"err/bound={err / float(ref.bound):.3e} err/tol={err / ref.tol:.3e}")
        if not err <= ref.tol:
            self.failures.append((what, variant, "loss err / tol", err / ref.tol, float(got), float(ref.loss)))

    def twice(self, what, a, b):
        if not _same_bits(a, b):
            self.failures.append((what, "two calls differ"))

    def done(self):
        assert not self.failures, "\n".join(" ".join(map(str, f)) for f in self.failures)


# ---- d3m_photometric_loss ------------------------------------------------------------------------------------------------------
def _photometric(c, dev, with_grad, expect_rc=D3M_OK):
    from deep3dmap_amd import _lib
    loss, scratch = Guarded((1,)), Guarded((H.SCRATCH_FLOATS["photometric"],))
    grad = (Shifted if c.off == "grad" else Guarded)((c.B * c.C, c.H * c.W)) if with_grad else None
    rc = _lib.lib().d3m_photometric_loss(_ptr(dev["im1"]), _ptr(dev["im2"]), _ptr(dev["mask"]), _ptr(dev["sigma"]), _ptr(loss),
                                         None if grad is None else _ptr(grad), _ptr(scratch), c.B, c.C, c.H, c.W,
                                         _lib.stream_ptr())
    return _finish(rc, expect_rc, scratch, [loss, grad])


@pytest.mark.parametrize("c", H.photo_cases(), ids=H.case_id)
def test_photometric_loss_at_shape(c):
    chk = Check(c)
    for variant in H.variants(c):
        inp = H.inputs(c, variant)
        dev = {k: _dev(inp[k], c.off == k) for k in ("im1", "im2", "mask", "sigma")}
        ref = H.float_reference(c, variant, inp) if H.is_float(variant) else None
        want = None if ref else H.exact_expected(c, inp)
        for with_grad in (False, True):
            what = f"{variant} grad={int(with_grad)}"
            got = _photometric(c, dev, with_grad)
            chk.twice(what, got, _photometric(c, dev, with_grad))
            if ref:
                chk.loss(what, variant, got[0][0], ref)
                if with_grad:
                    chk.close(what + " gradient", got[1], ref.grad["grad"], ref.grad_tol["grad"])
            else:
                chk.exact(what + " loss", got[0], want["loss"])
                if with_grad:
                    chk.exact(what + " gradient", got[1], want["grad"])
    chk.done()


@pytest.mark.parametrize("shape", H.PHOTO_REFUSED, ids=str)
def test_photometric_loss_refuses_more_than_1024_planes_and_launches_nothing(shape):
    c = H.PhotoCase(*shape, 1, 1, None)
    n = c.B * c.C * c.H * c.W
    dev = dict(im1=_dev(np.zeros(n)), im2=_dev(np.zeros(n)), mask=_dev(np.ones(c.B * c.H * c.W)),
               sigma=_dev(np.ones(c.B * c.H * c.W)))
    for with_grad in (False, True):
        with kernels_launched() as k:
            loss, grad = _photometric(c, dev, with_grad, expect_rc=D3M_ERR_INVALID)
        assert not k.names, k.names
        assert _untouched(loss) and (grad is None or _untouched(grad))


# ---- d3m_sum_squared_error -------------------------------------------------------------------------------------------------------
def _sse(c, dev, with_grad, n=None, expect_rc=D3M_OK):
    from deep3dmap_amd import _lib
    loss, scratch = Guarded((1,)), Guarded((H.SCRATCH_FLOATS["sse"],))
    grad = (Shifted if c.off == "grad" else Guarded)((c.n,)) if with_grad else None
    rc = _lib.lib().d3m_sum_squared_error(_ptr(dev["a"]), _ptr(dev["b"]), _ptr(loss), None if grad is None else _ptr(grad),
                                          _ptr(scratch), c.n if n is None else n, _lib.stream_ptr())
    return _finish(rc, expect_rc, scratch, [loss, grad])


@pytest.mark.parametrize("c", H.sse_cases(), ids=H.case_id)
def test_sum_squared_error_at_size(c):
    chk = Check(c)
    for variant in H.variants(c):
        inp = H.inputs(c, variant)
        dev = {k: _dev(inp[k], c.off == k) for k in ("a", "b")}
        ref = H.float_reference(c, variant, inp) if H.is_float(variant) else None
        want = None if ref else H.exact_expected(c, inp)
        for with_grad in (False, True):
            what = f"{variant} grad={int(with_grad)}"
            got = _sse(c, dev, with_grad)
            chk.twice(what, got, _sse(c, dev, with_grad))
            if ref:
                chk.loss(what, variant, got[0][0], ref)
            else:
                chk.exact(what + " loss", got[0], want["loss"])
            if with_grad:           # (2 (a - b) is a prediction of bits for float inputs too)
                chk.exact(what + " gradient", got[1], ref.grad["grad"] if ref else want["grad"])
    chk.done()


def test_sum_squared_error_refuses_no_elements_and_launches_nothing():
    c = H.SseCase(5, None)
    dev = dict(a=_dev(np.ones(5)), b=_dev(np.zeros(5)))
    with kernels_launched() as k:
        loss, grad = _sse(c, dev, True, n=0, expect_rc=D3M_ERR_INVALID)
    assert not k.names, k.names
    assert _untouched(loss) and _untouched(grad)


# ---- d3m_smooth_loss_forward / _backward ------------------------------------------------------------------------------------------
def _smooth(c, pred, grad_loss, expect_rc=D3M_OK):
    from deep3dmap_amd import _lib
    L = _lib.lib()
    loss, scratch, grad = Guarded((1,)), Guarded((H.SCRATCH_FLOATS["smooth"],)), Guarded((c.B, c.H, c.W))
    rc = L.d3m_smooth_loss_forward(_ptr(pred), _ptr(loss), _ptr(scratch), c.B, c.H, c.W, _lib.stream_ptr())
    out = _finish(rc, expect_rc, scratch, [loss])
    rc = L.d3m_smooth_loss_backward(_ptr(pred), _ptr(grad_loss), _ptr(grad), c.B, c.H, c.W, _lib.stream_ptr())
    return out + _finish(rc, expect_rc, None, [grad])


@pytest.mark.parametrize("c", H.smooth_cases(), ids=H.case_id)
def test_smooth_loss_at_shape(c):
    chk = Check(c)
    grad_loss = _dev(np.array([H.GRAD_LOSS]))
    for variant in H.variants(c):
        inp = H.inputs(c, variant)
        pred = _dev(inp["pred"])
        got = _smooth(c, pred, grad_loss)
        chk.twice(variant, got, _smooth(c, pred, grad_loss))
        if H.is_float(variant):
            ref = H.float_reference(c, variant, inp)
            chk.loss("forward", variant, got[0][0], ref)
            chk.exact(variant + " gradient", got[1], ref.grad["grad"])       # (signs and counts: bits for float inputs too)
        else:
            want = H.exact_expected(c, inp)
            chk.exact(variant + " loss", got[0], want["loss"])
            chk.exact(variant + " gradient", got[1], want["grad"])
    chk.done()


@pytest.mark.parametrize("shape", H.SMOOTH_REFUSED, ids=str)
def test_smooth_loss_refuses_maps_without_second_differences_and_launches_nothing(shape):
    c = H.SmoothCase(*shape)
    with kernels_launched() as k:
        loss, grad = _smooth(c, _dev(np.zeros(shape)), _dev(np.ones(1)), expect_rc=D3M_ERR_INVALID)
    assert not k.names, k.names
    assert _untouched(loss) and _untouched(grad)


# ---- d3m_fit_loss_forward / _backward ------------------------------------------------------------------------------------------------
def _fit_forward(c, dev, scratch, mask_sum, expect_rc=D3M_OK):
    from deep3dmap_amd import _lib
    loss = Guarded((1,))
    rc = _lib.lib().d3m_fit_loss_forward(*[_ptr(dev[k]) for k in H.FIT_NAMES], _ptr(loss), _ptr(scratch), _ptr(mask_sum),
                                         c.B, c.H, c.W, _lib.stream_ptr())
    return _finish(rc, expect_rc, scratch, [loss])


def _fit_backward(c, dev, scratch, grad_loss, which, expect_rc=D3M_OK):
    from deep3dmap_amd import _lib
    hw = c.H * c.W
    outs = [Guarded(s) if k in which else None for k, s in (("g_rgb", (c.B, 3, hw)), ("g_depth", (c.B, hw)), ("g_alpha", (c.B, hw)))]
    rc = _lib.lib().d3m_fit_loss_backward(*[_ptr(dev[k]) for k in H.FIT_NAMES], _ptr(scratch), _ptr(grad_loss),
                                          *[None if o is None else _ptr(o) for o in outs], c.B, c.H, c.W, _lib.stream_ptr())
    return _finish(rc, expect_rc, scratch, outs)


FIT_GRADS = ("g_rgb", "g_depth", "g_alpha")


@pytest.mark.parametrize("c", H.fit_cases(), ids=H.case_id)
def test_fit_loss_at_shape(c):
    chk = Check(c)
    grad_loss = _dev(np.array([FIT_GRAD_OUT]))
    for variant in H.variants(c):
        inp = H.inputs(c, variant)
        dev = {k: _dev(inp[k]) for k in H.FIT_NAMES}
        for given in (None, H.foreign_mask_sum(inp)):
            what = f"{variant} mask_sum={'own' if given is None else 'given'}"
            mask_sum = None if given is None else _dev(np.array([given]))
            scratch, again = (Guarded((H.SCRATCH_FLOATS["fit"],)) for _ in range(2))
            got = _fit_forward(c, dev, scratch, mask_sum)
            chk.twice(what, got, _fit_forward(c, dev, again, mask_sum))
            # NULL and non-unit incoming gradient with all three outputs, then each output alone
            for go, which in ((None, FIT_GRADS), (FIT_GRAD_OUT, FIT_GRADS)) + tuple((FIT_GRAD_OUT, (k,)) for k in FIT_GRADS):
                grads = _fit_backward(c, dev, scratch, None if go is None else grad_loss, which)
                if len(which) == 3:
                    chk.twice(f"{what} backward go={go}", grads, _fit_backward(c, dev, again, None if go is None else grad_loss,
                                                                               which))
                if H.is_float(variant):
                    ref = H.float_reference(c, variant, inp, mask_sum=given, grad_out=go)
                    if go is None:
                        chk.loss(what, variant, got[0][0], ref)
                    want, tols = ref.grad, ref.grad_tol
                else:
                    want = H.exact_expected(c, inp, mask_sum=given, grad_out=go)
                    tols = dict.fromkeys(FIT_GRADS)
                    if go is None:
                        chk.exact(what + " loss", got[0], want["loss"])
                for k, g in zip(FIT_GRADS, grads):
                    assert (g is None) == (k not in which)
                    if g is not None:
                        chk.close(f"{what} go={go} {k}{' alone' if len(which) == 1 else ''}", g, want[k], tols[k])
    chk.done()


def test_fit_loss_refuses_more_than_1024_views_and_launches_nothing():
    c = H.FitCase(*H.FIT_REFUSED[0])
    hw = c.H * c.W
    dev = {k: _dev(np.ones(c.B * hw * (3 if k.startswith("rgb") else 1))) for k in H.FIT_NAMES}
    scratch = Guarded((H.SCRATCH_FLOATS["fit"],))
    with kernels_launched() as k:
        (loss,) = _fit_forward(c, dev, scratch, None, expect_rc=D3M_ERR_INVALID)
        grads = _fit_backward(c, dev, scratch, None, FIT_GRADS, expect_rc=D3M_ERR_INVALID)
    assert not k.names, k.names
    assert _untouched(loss) and all(_untouched(g) for g in grads) and _untouched(scratch.inner.cpu().numpy())


# ---- through the wrappers of core/losses.py -------------------------------------------------------------------------------------------
WRAPPER_SHAPE = (3, 3, 17, 15)


def _wrapper_operands():
    c = H.PhotoCase(*WRAPPER_SHAPE, 1, 1, None)
    inp = H.photo_inputs(c, "sigma_below_one")
    B, C, Hh, W = WRAPPER_SHAPE
    t = lambda x, ch: torch.from_numpy(x).reshape(B, ch, Hh, W)      # noqa: E731
    return c, t(inp["im1"], C), t(inp["im2"], C), t(inp["mask"], 1), t(inp["sigma"], 1)


@pytest.mark.parametrize("which", ["im2", "mask_1_1_H_W", "mask_B_1_1_1", "sigma", "all"])
def test_photometric_loss_broadcasts_as_the_reference_does(which):
    from deep3dmap_amd.core import photometric_loss
    c, im1, im2, mask, sigma = _wrapper_operands()
    B = im1.shape[0]
    if which in ("im2", "all"):
        im2 = im2[:1]
    if which in ("mask_1_1_H_W", "all"):
        mask = mask[:1]
    if which == "mask_B_1_1_1":
        mask = mask[:, :, :1, :1]
    if which in ("sigma", "all"):
        sigma = sigma[:1]
    full = [im2.expand_as(im1).contiguous(), mask.expand(B, 1, *im1.shape[2:]).contiguous(),
            sigma.expand(B, 1, *im1.shape[2:]).contiguous()]
    assert any(f.shape != s.shape for f, s in zip(full, (im2, mask, sigma)))

    def run(b, m, s):
        a = im1.cuda().requires_grad_(True)
        with kernels_launched() as k:
            loss = photometric_loss(a, b.cuda(), mask=m.cuda(), conf_sigma=s.cuda())
            (loss * 3.0).backward()
            torch.cuda.synchronize()
        assert {"k_photometric_reduce", "k_photometric_finish"} <= k.names, k.names
        return loss.detach().cpu(), a.grad.cpu()
    got, by_hand = run(im2, mask, sigma), run(*full)
    assert torch.equal(got[0].view(torch.int32), by_hand[0].view(torch.int32))
    assert torch.equal(got[1].view(torch.int32), by_hand[1].view(torch.int32))
    # the reference's formula (utils.py:105-114) with torch's own broadcasting, float64
    a64, b64, m64, s64 = (x.double() for x in (im1, im2, mask, sigma))
    l64 = (a64 - b64).abs() * 2 ** 0.5 / (s64 + H.SIGMA_EPS) + (s64 + H.SIGMA_EPS).log()
    m64 = m64.expand_as(l64)
    want = float((l64 * m64).sum() / m64.sum())
    ref = H.FloatReference(c, dict(im1=im1.reshape(B * 3, -1).numpy(), im2=full[0].reshape(B * 3, -1).numpy(),
                                   mask=full[1].reshape(B, -1).numpy(), sigma=full[2].reshape(B, -1).numpy()))
    assert abs(want - float(ref.loss)) <= 1e-12 * abs(want)
    err = abs(float(got[0]) - want)
    print(f"LOSS wrapper photometric {which} D*2^-24={ref.D * H.EPS32:.3e} E32={ref.e32:.3e} err/tol={err / ref.tol:.3e}")
    assert err <= ref.tol, (err, ref.tol)
    g = got[1].double().reshape(B * 3, -1).numpy()
    assert bool((np.abs(g - 3.0 * ref.grad["grad"]) <= 3.0 * ref.grad_tol["grad"] + 2.0 ** -24 * np.abs(g)).all())


def test_photometric_loss_refuses_what_it_cannot_broadcast_and_launches_nothing():
    from deep3dmap_amd.core import photometric_loss
    _, im1, im2, mask, sigma = _wrapper_operands()
    im1, im2, mask, sigma = (x.cuda() for x in (im1, im2, mask, sigma))
    with kernels_launched() as k:
        with pytest.raises(NotImplementedError):
            photometric_loss(im1, im2, mask=mask, conf_sigma=sigma.expand(-1, 3, -1, -1))
        with pytest.raises(ValueError):
            photometric_loss(im1, im2, mask=mask[:, :, :-1])
        with pytest.raises(ValueError):
            photometric_loss(im1, im2[:2], mask=mask)
        torch.cuda.synchronize()
    assert not k.names, k.names


def test_silhouette_loss_with_a_broadcast_reference():
    from deep3dmap_amd.core import silhouette_loss
    c = H.SseCase(3 * 23 * 19, None)
    inp = H.sse_inputs(c, "dense")
    ref_image = inp["b"][:23 * 19]
    b = np.tile(ref_image, 3)
    want = H.exact_expected(c, dict(a=inp["a"], b=b))
    image = torch.from_numpy(inp["a"].astype(np.float32)).reshape(3, 23, 19).cuda().requires_grad_(True)
    with kernels_launched() as k:
        loss = silhouette_loss(image, torch.from_numpy(ref_image.astype(np.float32)).reshape(1, 23, 19).cuda())
        loss.backward()
        torch.cuda.synchronize()
    assert {"k_sum_squared_error", "k_sum_partials"} <= k.names, k.names
    assert np.array_equal(_bits(loss.item()), _bits(want["loss"]))
    assert np.array_equal(_bits(image.grad.cpu().numpy().reshape(-1)), _bits(want["grad"]))


def test_smooth_loss_on_a_four_dimensional_map_and_a_pyramid():
    from deep3dmap_amd.core import smooth_loss
    c0, c1 = H.SmoothCase(2, 33, 31), H.SmoothCase(2, 17, 16)
    p0, p1 = (H.smooth_inputs(c, "dense")["pred"] for c in (c0, c1))
    w0, w1 = (H.exact_expected(c, dict(pred=p)) for c, p in ((c0, p0), (c1, p1)))
    t0, t1 = (torch.from_numpy(p.astype(np.float32)).cuda() for p in (p0, p1))
    # [1, 2, H, W] is the two maps of [2, H, W]
    a = t0[None].clone().requires_grad_(True)
    with kernels_launched() as k:
        loss = smooth_loss(a)
        (loss * float(H.GRAD_LOSS)).backward()
        torch.cuda.synchronize()
    assert {"k_smooth_reduce", "k_smooth_finish", "k_smooth_grad"} <= k.names, k.names
    assert np.array_equal(_bits(loss.item()), _bits(w0["loss"]))
    assert a.grad.shape == a.shape and np.array_equal(_bits(a.grad.cpu().numpy().reshape(-1)), _bits(w0["grad"].reshape(-1)))
    # two levels: the second weighs 1 / 2.3 (utils.py:82-102)
    a, b = t0.clone().requires_grad_(True), t1.clone().requires_grad_(True)
    loss = smooth_loss([a, b])
    (loss * float(H.GRAD_LOSS)).backward()
    weight = 1.0 / 2.3
    want = float(w0["loss"]) + float(w1["loss"]) * weight
    assert abs(loss.item() - want) <= 3 * 2.0 ** -24 * want          # (one product and one sum of the eager glue, in float32)
    assert np.array_equal(_bits(a.grad.cpu().numpy().reshape(-1)), _bits(w0["grad"].reshape(-1)))
    g1 = b.grad.cpu().double().numpy()
    want1 = w1["grad"].astype(np.float64) * weight
    assert bool((np.abs(g1 - want1) <= 3 * 2.0 ** -24 * np.abs(want1)).all())


def test_multiview_fit_loss_without_the_link_at_900_partials():
    from deep3dmap_amd.core import multiview_fit_loss
    c = H.FitCase(300, 7, 439)
    inp = H.fit_inputs(c, "dense")
    want = H.exact_expected(c, inp, grad_out=FIT_GRAD_OUT)
    t = {k: torch.from_numpy(inp[k].astype(np.float32)).reshape(c.B, *((3,) if k.startswith("rgb") else ()), c.H, c.W).cuda()
         for k in H.FIT_NAMES}
    rgb, depth, alpha = (t[k].requires_grad_(True) for k in ("rgb", "depth", "alpha"))
    with kernels_launched() as k:
        loss = multiview_fit_loss(rgb, depth, alpha, t["rgb_t"], t["depth_t"], t["alpha_t"], t["mask"], link=False)
        (loss * FIT_GRAD_OUT).backward()
        torch.cuda.synchronize()
    assert {"k_fit_loss_reduce", "k_fit_loss_finish", "k_fit_loss_grad"} <= k.names, k.names
    assert np.array_equal(_bits(loss.item()), _bits(want["loss"]))
    for x, name in ((rgb, "g_rgb"), (depth, "g_depth"), (alpha, "g_alpha")):
        assert np.array_equal(_bits(x.grad.cpu().numpy().reshape(-1)), _bits(want[name].reshape(-1))), name
