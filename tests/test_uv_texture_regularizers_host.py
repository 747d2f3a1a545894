"""The UV texture regularisers without a device (neural_renderer/uv_texture_regularizers.py, csrc/d3m_uv_texture_reg.h): the
float64 restatement of tests/uv_texture_regularizer_scenes.py against central finite differences; the closed form of the flat
term's gradient; known answers by hand; what the cases are there for; the float32 yardsticks behind the device tolerances;
every argument error; the C entry points' refusals."""
import ctypes

import pytest
import torch

import uv_texture_regularizer_scenes as S
from deep3dmap_amd.neural_renderer import uv_texture_regularizers as R      # the node every check in this file is about

FD_STEP = 1e-6
FD_AGREEMENT = 1e-6       # of the largest gradient entry (test_uv_fill_host.py's step and rule)
ODD = S.CASES[3]


# ---- 1. the restatement against central finite differences ---------------------------------------------------------------------
@pytest.mark.parametrize("config", S.CONFIGS)
def test_restatement_against_finite_differences(config):
    a = S.case_inputs(ODD)
    kw = dict(S.CONFIGS[config])
    if kw.get("anchor", 0) > 0:
        kw.update(reference=a["reference"].double(), reference_weights=a["reference_weights"].double())
    x, g = a["texture"].double(), a["upstream"].double()
    grad = S.reference(ODD, config)["texture_grad"]
    loss = lambda v: float((S.value_of(v, a["mask"], **kw) * g).sum())
    fd = torch.zeros_like(x)
    for i in range(x.numel()):
        lo, hi = x.clone(), x.clone()
        lo.view(-1)[i] -= FD_STEP
        hi.view(-1)[i] += FD_STEP
        fd.view(-1)[i] = (loss(hi) - loss(lo)) / (2 * FD_STEP)
    err = float((grad - fd).abs().max()) / float(grad.abs().max())
    print(config, "largest |autograd - finite differences| / largest entry:", err)
    assert float(grad.abs().max()) > 0 and err <= FD_AGREEMENT, err


# ---- 2. the flat term's closed form ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.CASES[3:7], ids=S.case_id)
def test_flat_gradient_is_the_closed_form(case):
    """2 (x - mu) / (N C) on the active texels, exactly 0 elsewhere: the mean's own derivative sums to zero."""
    name, H, W, B, C = case
    a = S.case_inputs(case)
    x, g = a["texture"].double(), a["upstream"].double()
    grad = S.reference(case, "flat")["texture_grad"]
    for b in range(B):
        active = S._plane(a["mask"], b, 2) > 0
        N = int(active.sum())
        if N == 0:
            assert not bool(grad[b].any())
            continue
        mu = x[b][active].mean(0)
        closed = torch.where(active[..., None], 2 * (x[b] - mu) / (N * C), torch.zeros_like(x[b])) * g[b]
        assert torch.allclose(grad[b], closed, rtol=0, atol=1e-15), float((grad[b] - closed).abs().max())


# ---- 3. known answers by hand -----------------------------------------------------------------------------------------------------
def test_known_answers_on_one_row():
    """1 x 6, C = 1: x = 0 1 3 6 10 15, texel 2 absent.  Pairs (0,1), (3,4), (4,5): (1 + 16 + 25) / 3 = 14.  Mirror pairs 0-5
    and 1-4 (2-3 lacks texel 2): (225 + 81) / 2 = 153.  Flat: mu = 32 / 5, sum (x - mu)^2 = 157.2, / 5 = 31.44.  Anchor to 0
    with weights 1 2 1 0 -1 0.5: R = 3.5 (texel 2 absent, -1 counts as 0), (2 * 1 + 0.5 * 225) / 3.5 = 229 / 7."""
    x = torch.tensor([0., 1., 3., 6., 10., 15.], dtype=torch.float64).reshape(1, 1, 6, 1)
    mask = torch.tensor([[1., 1., 0., 1., 1., 1.]])
    rw = torch.tensor([[1., 2., 1., 0., -1., 0.5]])
    assert S.counts(mask, 1, 6, rw) == (3, 2, 5, 3.5)
    t = S.image_terms(x[0], mask, None, torch.zeros(1, 6, 1), rw)
    want = dict(smooth=14.0, symmetry=153.0, flat=31.44, anchor=229 / 7)
    for k, v in want.items():
        assert abs(float(t[k]) - v) <= 1e-12 * v, (k, float(t[k]), v)
    tv = S.image_terms(x[0], mask, 0.05, which=("smooth",))["smooth"]             # Charbonnier: nearly |d|
    exact = sum((d * d + 0.0025) ** 0.5 - 0.05 for d in (1, 4, 5)) / 3
    assert abs(float(tv) - exact) <= 1e-12
    value = S.value_of(x, mask, smooth=0.5, symmetry=2.0, flat=1.0, anchor=3.0, reference=torch.zeros(1, 6, 1),
                       reference_weights=rw)
    assert abs(float(value[0]) - (7.0 + 306.0 + 31.44 + 3 * 229 / 7)) <= 1e-10


def test_known_answers_on_an_odd_width():
    """5 x 7, C = 3, every texel active, x[i,j,k] = j + 10 i + 100 k.  30 horizontal pairs of d = 1 and 28 vertical ones of
    d = 10: (30 + 2800) / 58.  Mirror pairs j = 0, 1, 2 of d = 6, 4, 2 in 5 rows, the centre column unpaired: M = 15,
    5 (36 + 16 + 4) / 15 = 56 / 3.  Switching the centre column off changes neither."""
    i, j, k = torch.meshgrid(torch.arange(5.), torch.arange(7.), torch.arange(3.), indexing="ij")
    x = (j + 10 * i + 100 * k).double()
    assert S.counts(None, 5, 7) == (58, 15, 35, 35.0)
    t = S.image_terms(x, None, which=("smooth", "symmetry"))
    assert abs(float(t["smooth"]) - 2830 / 58) <= 1e-12 and abs(float(t["symmetry"]) - 56 / 3) <= 1e-12
    mask = torch.ones(5, 7)
    mask[:, 3] = 0
    assert S.counts(mask, 5, 7)[:3] == (5 * 4 + 4 * 6, 15, 30)
    assert abs(float(S.image_terms(x, mask, which=("symmetry",))["symmetry"]) - 56 / 3) <= 1e-12


def test_terms_of_count_zero_are_zero_with_zero_gradient():
    one = S.CASES[0]
    for config in S.CONFIGS:
        r = S.reference(one, config)
        if "anchor" in config or "all" in config or config == "flat":
            continue                                                   # N = R = 1 there; the flat term of one texel is 0 too
        assert not bool(r["value"].any()) and not bool(r["texture_grad"].any())
    column = S.reference(S.CASES[2], "symmetry")
    assert not bool(column["value"].any()) and not bool(column["texture_grad"].any())


# ---- 4. the cases and the yardsticks -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_cases_have_what_they_are_there_for(case):
    name, H, W, B, C = case
    a = S.case_inputs(case)
    assert float(a["texture"].min()) >= 0 and float(a["texture"].max()) <= 1
    up = a["upstream"]
    assert up.shape == (B,) and (B == 1 or (bool((up > 0).any()) and bool((up < 0).any())))
    per_image = S.image_counts(case)
    if name in S.DEGENERATE:
        assert per_image == [(0, 0, 1, float(a["reference_weights"].clamp(min=0).sum()))]
        return
    for b, (P, M, N, Rsum) in enumerate(per_image):
        if name == "per_image" and b == S.ABSENT_IMAGE:
            assert (P, M, N, Rsum) == (0, 0, 0, 0.0)
            continue
        share = N / (H * W)
        print(S.case_id(case), "image", b, "active share %.2f" % share, "P", P, "M", M, "N", N, "R %.1f" % Rsum)
        assert 0.3 <= share <= 0.7
        assert P > 0 and N > 0 and Rsum > 0 and (M > 0) == (W > 1)
    if name == "row":
        assert H == 1
    if name == "column":
        assert W == 1 and all(c[1] == 0 for c in per_image)
    if name == "odd":
        assert W % 2 == 1
    if name == "shared":
        assert a["mask"].dim() == 2 and a["reference"].dim() == 3 and a["reference_weights"].dim() == 2
    if name == "per_image":
        m = a["mask"]
        assert m.dim() == 3 and bool(torch.isnan(m).any()) and bool((m < 0).any()) and bool((a["reference_weights"] < 0).any())
        assert float(up[S.ZERO_UPSTREAM_IMAGE]) == 0.0 and S.ZERO_UPSTREAM_IMAGE != S.ABSENT_IMAGE
    if name == "parts":
        assert 1 < S.parts_of(case) < R.MAX_PARTS
    if name == "stride":
        assert H * W > R.MAX_PARTS * R.PER_PART and S.parts_of(case) == R.MAX_PARTS
    else:
        assert H * W <= R.MAX_PARTS * R.PER_PART


def test_float32_yardsticks_are_the_recorded_ones():
    """Measured here again: within a factor 2 of the recorded figures either way.  The device tolerance of a kind is 8 x the
    largest recorded one."""
    assert set(S.YARDSTICK) == {S.case_id(c) for c in S.CASES}
    for case in S.CASES:
        measured, recorded = S.measure_yardstick(case), S.YARDSTICK[S.case_id(case)]
        for kind, value in measured.items():
            print(S.case_id(case), kind, "float32 yardstick:", "%.2e" % value, "recorded:", recorded[kind])
            assert recorded[kind] / 2 <= value <= recorded[kind] * 2, (S.case_id(case), kind, value)
    for kind in S.KINDS:
        assert S.DEVICE_TOLERANCE[kind] == 8 * max(y[kind] for y in S.YARDSTICK.values()) > 0


# ---- 5. argument checks --------------------------------------------------------------------------------------------------------------
def test_argument_errors_are_raised_before_the_device():
    from deep3dmap_amd import neural_renderer as nr
    for name in ("uv_texture_regularizer", "UvTextureRegularizer", "uv_texture_smoothness", "uv_texture_symmetry",
                 "uv_texture_flatness", "uv_texture_anchor", "uv_layout_mask"):
        assert getattr(nr, name) is getattr(R, name)
    x, m = torch.rand(2, 5, 7, 3), torch.ones(2, 5, 7)
    with pytest.raises(TypeError, match="texture"):
        nr.uv_texture_regularizer(x.numpy(), smooth=1.0)
    for bad in (torch.rand(5, 7), torch.rand(2, 5, 7, 3, 1), x.double(), torch.rand(0, 5, 7, 3), torch.rand(2, 0, 7, 3),
                torch.rand(2, 5, 0, 3), torch.rand(2, 5, 7, 0), torch.rand(2, 5, 7, 5), torch.empty(1, 32769, 1, 1, device="meta"),
                torch.empty(1, 1, 32769, 1, device="meta"), torch.empty(65536, 1, 1, 1, device="meta")):
        with pytest.raises(ValueError, match="texture"):
            nr.uv_texture_regularizer(bad, smooth=1.0)
    for kw in (dict(), dict(smooth=-1.0), dict(smooth=1.0, flat=-0.5), dict(symmetry=float("nan")), dict(anchor=float("inf"))):
        with pytest.raises(ValueError, match="smooth, symmetry, flat and anchor"):
            nr.uv_texture_regularizer(x, m, **kw)
    for eps in (0.0, -0.05, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="smooth_eps"):
            nr.uv_texture_regularizer(x, m, smooth=1.0, smooth_eps=eps)
    for bad in (torch.ones(7, 5), torch.ones(1, 5, 7), torch.ones(2, 5, 7, 1), m.double(), m.numpy(), m.to("meta"),
                m.clone().requires_grad_(True)):
        with pytest.raises(ValueError, match="mask"):
            nr.uv_texture_regularizer(x, bad, smooth=1.0)
    with pytest.raises(ValueError, match="mask"):
        nr.uv_texture_regularizer(x[0], m, smooth=1.0)                   # a per-image mask for an unbatched texture
    with pytest.raises(ValueError, match="reference"):
        nr.uv_texture_regularizer(x, m, anchor=1.0)
    for bad in (torch.rand(5, 7), torch.rand(2, 5, 7, 4), torch.rand(3, 5, 7, 3), x.double(), x.to("meta"),
                x.clone().requires_grad_(True)):
        with pytest.raises(ValueError, match="reference"):
            nr.uv_texture_regularizer(x, m, anchor=1.0, reference=bad)
    for bad in (torch.ones(7, 5), torch.ones(2, 5, 7, 3), m.double(), m.clone().requires_grad_(True)):
        with pytest.raises(ValueError, match="reference_weights"):
            nr.uv_texture_regularizer(x, m, anchor=1.0, reference=x.clone(), reference_weights=bad)
    with pytest.raises(ValueError, match="reference"):
        nr.UvTextureRegularizer(anchor=1.0)
    with pytest.raises(ValueError, match="must be > 0"):
        nr.UvTextureRegularizer(mask=m)
    # well-formed arguments on the host end at the device check, behind every other check; a term of weight 0 is not checked
    for call in (lambda: nr.uv_texture_regularizer(x, m, smooth=1.0), lambda: nr.uv_texture_regularizer(x[0], m[0], flat=1.0),
                 lambda: nr.uv_texture_regularizer(x, None, symmetry=1.0, reference=torch.rand(3)),
                 lambda: nr.uv_texture_anchor(x.clone().requires_grad_(True), x[0].clone(), m[0], m),
                 lambda: nr.UvTextureRegularizer(m[0], smooth=1.0, smooth_eps=0.05, anchor=2.0, reference=x)(x)):
        with pytest.raises(ValueError, match="GPU"):
            call()


# ---- 6. the C entry points refuse bad arguments before any launch ---------------------------------------------------------------
def test_entry_points_return_invalid_before_any_launch():
    from deep3dmap_amd import _lib
    L = _lib.lib()
    p, misaligned, by8 = ctypes.c_void_p(256), ctypes.c_void_p(258), ctypes.c_void_p(264)       # never dereferenced
    INVALID = 1
    B, H, W, C = 3, 33, 65, 3
    parts = R.num_parts(H, W)
    assert parts == 9 and R.num_parts(1, 1) == 1 and R.num_parts(300, 260) == R.MAX_PARTS == R.num_parts(32768, 32768)
    query = L.d3m_uv_texture_regularizer_scratch_bytes
    assert query(B, H, W) == (B * parts * (5 + 4 + 4) + B * 8) * 4
    assert query(0, H, W) == 0 == query(65536, H, W) == query(B, 0, W) == query(B, H, 32769)

    def run(fn, ok, changes):
        for change in changes:
            assert fn(*dict(ok, **change).values(), None) == INVALID, (fn.__name__, change)

    nan, inf = float("nan"), float("inf")
    common = [dict(B=0), dict(B=65536), dict(H=0), dict(W=0), dict(H=32769), dict(W=32769), dict(C=0), dict(C=5),
              dict(texture=None), dict(texture=misaligned), dict(mask=misaligned), dict(mask_batch=2), dict(smooth=-1.0),
              dict(smooth=nan), dict(symmetry=-0.5), dict(flat=inf), dict(anchor=-2.0),
              dict(smooth=0.0, symmetry=0.0, flat=0.0, anchor=0.0), dict(eps=0.0), dict(eps=-0.5), dict(eps=nan),
              dict(reference=None), dict(reference=misaligned), dict(reference_batch=2), dict(reference_weights=misaligned),
              dict(rw_batch=2), dict(C=4, texture=by8), dict(C=2, reference=ctypes.c_void_p(260)), dict(scratch=None),
              dict(scratch=misaligned)]
    inputs = dict(texture=p, B=B, H=H, W=W, C=C, mask=p, mask_batch=B, smooth=1.0, eps=R.NO_EPS, symmetry=1.0, flat=1.0,
                  anchor=1.0, reference=p, reference_batch=1, reference_weights=p, rw_batch=B)
    fwd = dict(inputs, scratch=p, scratch_bytes=1 << 30, stats=p, value=p)
    run(L.d3m_uv_texture_regularizer, fwd,
        common + [dict(stats=None), dict(stats=misaligned), dict(value=None), dict(value=misaligned)])
    both = dict(inputs, stats=None, grad_scale=p, scratch=p, scratch_bytes=1 << 30, value=p, grad=p)
    run(L.d3m_uv_texture_regularizer_grad, both,
        common + [dict(stats=misaligned), dict(grad_scale=misaligned), dict(value=misaligned), dict(grad=misaligned),
                  dict(value=None, grad=None), dict(C=4, grad=by8)])
    need = query(B, H, W)
    for fn, ok in ((L.d3m_uv_texture_regularizer, fwd), (L.d3m_uv_texture_regularizer_grad, both)):
        rc = fn(*dict(ok, scratch_bytes=need - 1).values(), None)
        assert L.d3m_error_string(rc) == b"workspace missing or too small"
