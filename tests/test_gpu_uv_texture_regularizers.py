"""The UV texture regularisers on the device (neural_renderer/uv_texture_regularizers.py, csrc/d3m_uv_texture_reg.h) against
the float64 restatement of tests/uv_texture_regularizer_scenes.py; tolerances: its DEVICE_TOLERANCE, 8 x the largest float32
yardstick of each kind (tests/test_uv_texture_regularizers_host.py holds the figures).  Everything the header calls exact is
compared by bits."""
import pytest
import torch

import sh_fragment_scenes as SF
import sh_uv_fragment_scenes as SU
import uv_bake_scenes as UB
import uv_texture_regularizer_scenes as S
from conftest import kernels_launched
from deep3dmap_amd.neural_renderer import uv_texture_regularizers as R
from vertex_attribute_scenes import VIEWING_ANGLE, image_size_of, scene

pytestmark = pytest.mark.gpu
FORWARD = dict.fromkeys(R.KERNELS_FORWARD, 1)
BACKWARD = dict.fromkeys(R.KERNELS_BACKWARD, 1)
CASE = {c[0]: c for c in S.CASES}


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _run(case, config, texture=None, upstream=None, **override):
    """(value [B], gradient [B,H,W,C]) of the node on a case's inputs under a configuration, on the device"""
    from deep3dmap_amd import neural_renderer as nr
    a = S.case_inputs(case)
    x = (a["texture"] if texture is None else texture).cuda().requires_grad_(True)
    kw = S.node_arguments(a, S.CONFIGS[config] if isinstance(config, str) else config, "cuda")
    kw.update(override)
    value = nr.uv_texture_regularizer(x, **kw)
    grad, = torch.autograd.grad(value, x, (a["upstream"] if upstream is None else upstream).cuda())
    return value.detach(), grad


# ---- 1. value and gradient of every case and configuration -------------------------------------------------------------------------
@pytest.mark.parametrize("config", S.CONFIGS)
@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_value_and_gradient_against_the_float64_reference(case, config):
    ref = S.reference(case, config)
    value, grad = _run(case, config)
    assert bool(torch.isfinite(value).all()) and bool(torch.isfinite(grad).all())
    for kind, got in (("value", value), ("texture_grad", grad)):
        err = S.relative_error(got, ref[kind])
        print(S.case_id(case), config, kind, "error / largest entry: %.2e" % err, "allowed: %.2e" % S.DEVICE_TOLERANCE[kind])
        assert got.shape == ref[kind].shape and err <= S.DEVICE_TOLERANCE[kind], (kind, err)
    name, H, W = case[:3]
    nothing = name in S.DEGENERATE or (config == "symmetry" and W == 1)
    if not nothing:
        assert float(ref["texture_grad"].abs().max()) > 0 and float(ref["value"].abs().max()) > 0


# ---- 2. exact things -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", S.CONFIGS)
def test_inactive_texels_absent_images_and_zero_upstream_get_plus_zero(config):
    case = CASE["per_image"]
    a = S.case_inputs(case)
    value, grad = _run(case, config)
    inactive = ~(a["mask"] > 0)
    assert int(inactive[0].sum()) > 0 and bool(inactive[S.ABSENT_IMAGE].all())
    bits = _bits(grad).cpu()
    assert bool((bits[inactive] == 0).all())
    assert bool((bits[S.ABSENT_IMAGE] == 0).all()) and int(_bits(value)[S.ABSENT_IMAGE]) == 0        # every count is 0 there
    assert bool((bits[S.ZERO_UPSTREAM_IMAGE] == 0).all()) and float(value[S.ZERO_UPSTREAM_IMAGE]) > 0
    assert float(grad[0].abs().max()) > 0


def test_terms_of_count_zero_are_plus_zero():
    for config in ("smooth", "charbonnier", "symmetry"):                  # 1 x 1: P = M = 0
        value, grad = _run(CASE["one"], config)
        assert not bool(_bits(value).any()) and not bool(_bits(grad).any()), config
    value, grad = _run(CASE["column"], "symmetry")                         # W = 1: no mirror pair
    assert not bool(_bits(value).any()) and not bool(_bits(grad).any())
    a = S.case_inputs(CASE["odd"])                                        # R = 0: no reference weight is > 0
    value, grad = _run(CASE["odd"], "anchor", reference_weights=-a["reference_weights"].cuda())
    assert not bool(_bits(value).any()) and not bool(_bits(grad).any())


@pytest.mark.parametrize("case", (CASE["odd"], CASE["per_image"], CASE["stride"]), ids=S.case_id)
def test_a_mirror_symmetric_texture_has_symmetry_plus_zero(case):
    a = S.case_inputs(case)
    x, m = a["texture"], torch.nan_to_num(a["mask"], nan=-1.0)
    x, m = torch.maximum(x, x.flip(2)), torch.maximum(m, m.flip(-1))
    value, grad = _run(case, "symmetry", texture=x, mask=m.cuda())
    assert not bool(_bits(value).any()) and not bool(_bits(grad).any())
    value, grad = _run(case, "symmetry", mask=m.cuda())                  # (the case's own texture is not symmetric)
    assert float(value.abs().max()) > 0 and float(grad.abs().max()) > 0


@pytest.mark.parametrize("config", ("smooth", "charbonnier"))
def test_a_constant_texture_has_smoothness_plus_zero(config):
    for case in (CASE["odd"], CASE["per_image"]):
        name, H, W, B, C = case
        x = torch.linspace(0.1, 0.9, B * C).reshape(B, 1, 1, C).expand(B, H, W, C).contiguous()
        value, grad = _run(case, config, texture=x)
        assert not bool(_bits(value).any()) and not bool(_bits(grad).any())


@pytest.mark.parametrize("case", (CASE["column"], CASE["shared"], CASE["per_image"]), ids=S.case_id)
def test_an_image_of_a_batch_has_the_bits_of_its_own_call(case):
    """The order of an image's sums does not depend on B; nor on whether the texture has a batch dimension."""
    from deep3dmap_amd import neural_renderer as nr
    a = S.case_inputs(case)
    B = case[3]
    value, grad = _run(case, "all_charbonnier")
    for b in range(B):
        kept = {k: (a[k].dim() == rank, a[k].cuda()) for k, rank in (("mask", 2), ("reference", 3), ("reference_weights", 2))}
        kw = {k: (t if shared else t[b:b + 1]) for k, (shared, t) in kept.items()}
        v1, g1 = _run(case, "all_charbonnier", texture=a["texture"][b:b + 1], upstream=a["upstream"][b:b + 1], **kw)
        assert torch.equal(_bits(v1), _bits(value[b:b + 1])) and torch.equal(_bits(g1), _bits(grad[b:b + 1])), b
        x = a["texture"][b].cuda().requires_grad_(True)                   # [H,W,C]: a 0-d value
        kw = {k: (t if shared else t[b]) for k, (shared, t) in kept.items()}
        v0 = nr.uv_texture_regularizer(x, **kw, **S.CONFIGS["all_charbonnier"])
        g0, = torch.autograd.grad(v0, x, a["upstream"][b].cuda())
        assert v0.dim() == 0 and torch.equal(_bits(v0), _bits(value[b])) and torch.equal(_bits(g0), _bits(grad[b])), b


def test_a_shared_mask_has_the_bits_of_the_mask_repeated():
    case = CASE["shared"]
    a, B = S.case_inputs(case), case[3]
    for config in ("all", "all_charbonnier"):
        shared = _run(case, config)
        repeated = _run(case, config, mask=a["mask"][None].repeat(B, 1, 1).cuda(),
                        reference=a["reference"][None].repeat(B, 1, 1, 1).cuda(),
                        reference_weights=a["reference_weights"][None].repeat(B, 1, 1).cuda())
        assert torch.equal(_bits(shared[0]), _bits(repeated[0])) and torch.equal(_bits(shared[1]), _bits(repeated[1]))
        none = _run(case, config, mask=None, reference_weights=None)
        ones = _run(case, config, mask=torch.ones_like(a["mask"]).cuda(), reference_weights=torch.ones_like(a["mask"]).cuda())
        assert torch.equal(_bits(none[0]), _bits(ones[0])) and torch.equal(_bits(none[1]), _bits(ones[1]))


# ---- 3. determinism and capture ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", (CASE["per_image"], CASE["stride"]), ids=S.case_id)
def test_two_runs_have_the_same_bits(case):
    for config in ("all", "all_charbonnier"):
        first, second = _run(case, config), _run(case, config)
        assert torch.equal(_bits(first[0]), _bits(second[0])) and torch.equal(_bits(first[1]), _bits(second[1]))


def test_captured_forward_and_backward():
    """Forward plus backward under torch.cuda.graph (CapturedStep: the step's own stream), replayed twice after the texture, the
    mask and the upstream gradient are rewritten in place -- the counts are taken on the device on every call --; a replay has
    the bits of the eager run.  The captured step has a leaf of its own that no eager call touches; the eager runs use a twin."""
    from deep3dmap_amd import neural_renderer as nr
    from deep3dmap_amd.graph import CapturedStep
    case = CASE["per_image"]
    a = S.case_inputs(case)
    config = S.CONFIGS["all_charbonnier"]
    reference, rw = a["reference"].cuda(), a["reference_weights"].cuda()
    textures = [a["texture"].cuda(), a["texture"].flip(1).cuda() * 0.5]
    masks = [a["mask"].cuda(), a["mask"].flip(0).contiguous().cuda()]
    upstreams = [a["upstream"].cuda(), torch.tensor([0.3, -0.2, 1.1]).cuda()]
    twin, live = textures[0].clone().requires_grad_(True), textures[0].clone().requires_grad_(True)
    m_twin, m_live, g_twin, g_live = masks[0].clone(), masks[0].clone(), upstreams[0].clone(), upstreams[0].clone()

    def step(x, m, g):
        value = nr.uv_texture_regularizer(x, m, reference=reference, reference_weights=rw, **config)
        grad, = torch.autograd.grad(value, x, g)
        return value, grad

    eager = []
    for i in (0, 1):
        with torch.no_grad():
            for dst, src in ((twin, textures), (m_twin, masks), (g_twin, upstreams)):
                dst.copy_(src[i])
        with kernels_launched() as k:
            eager.append([t.clone() for t in step(twin, m_twin, g_twin)])
        assert k.names == set(FORWARD) | set(BACKWARD), k.names          # nothing but the node's own kernels
    assert not torch.equal(eager[0][0], eager[1][0]) and not torch.equal(eager[0][1], eager[1][1])
    torch.cuda.synchronize()
    cs = CapturedStep(lambda: step(live, m_live, g_live)).capture()
    for i in (1, 0):
        with torch.no_grad():
            for dst, src in ((live, textures), (m_live, masks), (g_live, upstreams)):
                dst.copy_(src[i])
        got = [t.clone() for t in cs()]
        torch.cuda.synchronize()
        for x, y in zip(got, eager[i]):
            assert torch.equal(_bits(x), _bits(y)), i


# ---- 4. launches -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_launch_counts_are_the_docstrings(case):
    """Forward 4, backward 1, whatever B, H, W, C and the weights (the module's docstring)."""
    from deep3dmap_amd import neural_renderer as nr
    a = S.case_inputs(case)
    for config in S.CONFIGS:
        x = a["texture"].cuda().requires_grad_(True)
        kw = S.node_arguments(a, S.CONFIGS[config], "cuda")
        with kernels_launched() as kf:
            value = nr.uv_texture_regularizer(x, **kw)
        with kernels_launched() as kb:
            value.backward(a["upstream"].cuda())
        forward, backward = ({k: v[0] for k, v in t.times.items()} for t in (kf, kb))
        assert forward == FORWARD and sum(forward.values()) <= 4, (config, forward)
        assert backward == BACKWARD and sum(backward.values()) <= 4, (config, backward)
    for name in R.KERNELS_FORWARD + R.KERNELS_BACKWARD:
        assert name in R.__doc__


# ---- 5. the raw entry points ------------------------------------------------------------------------------------------------------------
def test_entry_point_writes_every_element_and_takes_null_pointers():
    from deep3dmap_amd import _lib
    L = _lib.lib()
    case = CASE["per_image"]
    name, H, W, B, C = case
    a = S.case_inputs(case)
    x, mask, ref, rw, up = (a[k].cuda() for k in ("texture", "mask", "reference", "reference_weights", "upstream"))
    scratch = torch.full((int(L.d3m_uv_texture_regularizer_scratch_bytes(B, H, W)) // 4,), float("nan"), device="cuda")
    w = S.CONFIGS["all_charbonnier"]
    inputs = lambda anchor, reference, weights: (
        _lib.ptr(x), B, H, W, C, _lib.ptr(mask), B, w["smooth"], w["smooth_eps"], w["symmetry"], w["flat"], anchor,
        _lib.ptr(reference), B, _lib.ptr(weights), B)
    full = inputs(w["anchor"], ref, rw)
    tail = (_lib.ptr(scratch), scratch.numel() * 4)
    value, grad = _run(case, "all_charbonnier")
    # value and gradient in one call, over poisoned buffers, the statistics computed into scratch: at most four launches
    poison = float("nan")
    v1, g1 = torch.full((B,), float("nan"), device="cuda"), torch.full((B, H, W, C), poison, device="cuda")
    with kernels_launched() as k:
        _lib.check(L.d3m_uv_texture_regularizer_grad(*full, None, _lib.ptr(up), *tail, _lib.ptr(v1), _lib.ptr(g1), None), "both")
    assert {n: v[0] for n, v in k.times.items()} == FORWARD
    assert torch.equal(_bits(v1), _bits(value)) and torch.equal(_bits(g1), _bits(grad))
    assert not bool(torch.isnan(g1).any())
    # a null gradient pointer: the value alone
    v2 = torch.full((B,), float("nan"), device="cuda")
    _lib.check(L.d3m_uv_texture_regularizer_grad(*full, None, None, *tail, _lib.ptr(v2), None, None), "value alone")
    assert torch.equal(_bits(v2), _bits(value))
    # a null value pointer and the forward's statistics: the gradient alone, one launch; a null grad_scale is 1
    stats, v3 = torch.empty(B, 4 + C, device="cuda"), torch.empty(B, device="cuda")
    _lib.check(L.d3m_uv_texture_regularizer(*full, *tail, _lib.ptr(stats), _lib.ptr(v3), None), "forward")
    assert torch.equal(_bits(v3), _bits(value))
    g3 = torch.full((B, H, W, C), poison, device="cuda")
    with kernels_launched() as k:
        _lib.check(L.d3m_uv_texture_regularizer_grad(*full, _lib.ptr(stats), None, None, 0, None, _lib.ptr(g3), None), "gradient")
    assert {n: v[0] for n, v in k.times.items()} == BACKWARD
    ones = _run(case, "all_charbonnier", upstream=torch.ones(B))[1]
    assert torch.equal(_bits(g3), _bits(ones))
    # a term of weight 0 is not evaluated: anchor = 0 with a null reference
    v4 = torch.empty(B, device="cuda")
    _lib.check(L.d3m_uv_texture_regularizer_grad(*inputs(0.0, None, None), None, None, *tail, _lib.ptr(v4), None, None), "no anchor")
    want = _run(case, dict(w, anchor=0.0))[0]
    assert torch.equal(_bits(v4), _bits(want))
    # the statistics: the coefficients weight / (count C) and the channel means
    for b, (P, M, N, Rsum) in enumerate(S.image_counts(case)):
        coefficients = [wt / (n * C) if n > 0 else 0.0 for wt, n in
                        ((w["smooth"], P), (w["symmetry"], M), (w["flat"], N), (w["anchor"], Rsum))]
        assert torch.allclose(stats[b, :4].cpu().double(), torch.tensor(coefficients, dtype=torch.float64), rtol=1e-6, atol=0), b
        if N > 0:
            mu = a["texture"][b][a["mask"][b] > 0].double().mean(0)
            assert torch.allclose(stats[b, 4:].cpu().double(), mu, rtol=1e-6, atol=0)


# ---- 6. the module, the helpers and the layout mask -----------------------------------------------------------------------------------
def test_module_and_helpers_equal_the_function():
    from deep3dmap_amd import neural_renderer as nr
    case = CASE["shared"]
    a = S.case_inputs(case)
    x, mask, ref, rw, up = (a[k].cuda() for k in ("texture", "mask", "reference", "reference_weights", "upstream"))

    def both(fn):
        leaf = x.clone().requires_grad_(True)
        value = fn(leaf)
        return value, torch.autograd.grad(value, leaf, up)[0]

    same = lambda p, q: torch.equal(_bits(p[0]), _bits(q[0])) and torch.equal(_bits(p[1]), _bits(q[1]))
    config = S.CONFIGS["all_charbonnier"]
    module = nr.UvTextureRegularizer(a["mask"], reference=a["reference"], reference_weights=a["reference_weights"], **config).cuda()
    assert set(dict(module.named_buffers())) == {"mask", "reference", "reference_weights"} and not list(module.parameters())
    assert same(both(module), _run(case, "all_charbonnier"))
    assert same(both(nr.UvTextureRegularizer(smooth=2.0).cuda()), both(lambda t: nr.uv_texture_regularizer(t, smooth=2.0)))
    assert same(both(lambda t: nr.uv_texture_smoothness(t, mask)), _run(case, "smooth"))
    assert same(both(lambda t: nr.uv_texture_smoothness(t, mask, 0.05)), _run(case, "charbonnier"))
    assert same(both(lambda t: nr.uv_texture_symmetry(t, mask)), _run(case, "symmetry"))
    assert same(both(lambda t: nr.uv_texture_flatness(t, mask)), _run(case, "flat"))
    assert same(both(lambda t: nr.uv_texture_anchor(t, ref, mask, rw)), _run(case, "anchor"))
    # inputs that are not contiguous are made so by the node
    wide = torch.zeros(case[3], case[1], case[2], 5, device="cuda")
    wide[..., 1:4] = x
    view = wide[..., 1:4].detach().requires_grad_(True)
    value = nr.uv_texture_regularizer(view, mask.t().contiguous().t(), smooth=1.0)
    grad, = torch.autograd.grad(value, view, up)
    assert same((value, grad), _run(case, "smooth"))


def test_uv_layout_mask_is_the_layout_records_coverage():
    from deep3dmap_amd import neural_renderer as nr
    T = 20
    uv = UB.layout_of("S1", "atlas").cuda()
    mask = nr.uv_layout_mask(uv, T)
    want = nr.uv_layout_fragments(uv, T).face_index_map[0] >= 0
    assert mask.shape == (T, T) and mask.dtype == torch.float32 and torch.equal(mask, want.float())
    assert 0 < int(want.sum()) < T * T
    x = torch.rand(T, T, 3, device="cuda").requires_grad_(True)
    nr.uv_texture_regularizer(x, mask, smooth=1.0, flat=1.0).backward()
    assert bool((_bits(x.grad)[~want] == 0).all()) and float(x.grad[want].abs().min()) > 0


# ---- 7. end to end ---------------------------------------------------------------------------------------------------------------------
def test_the_regulariser_moves_the_texels_no_pixel_reaches():
    """A few Adam steps on a learnable albedo and SH light through shade_uv_texture on the S1 scene.  Without the regulariser
    the texels outside every pixel's taps get a gradient of exactly 0 and keep their initial bits; with smooth and anchor they
    move.  No optimisation quality is asserted."""
    from deep3dmap_amd import neural_renderer as nr
    name, size, aa, (H, W) = "S1", 16, False, (32, 16)
    sc = scene(name)
    eyes = torch.from_numpy(sc["eyes"]).cuda()
    B = eyes.shape[0]
    r = nr.Renderer(camera_mode="look_at", image_size=image_size_of(size, aa), anti_aliasing=aa, viewing_angle=VIEWING_ANGLE)
    r.eye = eyes
    v = torch.from_numpy(sc["vertices"]).cuda()[None].repeat(B, 1, 1)
    sv = r._transform(v, None, None, None, None, None).detach().contiguous()
    fr = nr.rasterize_fragments(sv, torch.from_numpy(sc["tri"]).cuda()[None], r.image_size, aa, r.fill_back, r.near, r.far)
    uv, normals = SU.faces_uv_of(name, "seamless").cuda(), SF.cone_normals(name, False).cuda()
    start, light = SU.albedo_of(H, W).cuda(), SF.seeded_sh().cuda()
    target = torch.rand(B, 3, image_size_of(size, aa), image_size_of(size, aa), generator=torch.Generator().manual_seed(5)).cuda()

    def fit(regularised):
        albedo, sh = start.clone().requires_grad_(True), light.clone().requires_grad_(True)
        opt = torch.optim.Adam([albedo, sh], lr=0.05)
        untouched = None
        for _ in range(3):
            opt.zero_grad()
            images, _ = nr.shade_uv_texture(albedo, uv, normals, sh, fr)
            loss = ((images - target) ** 2).mean()
            if regularised:
                loss = loss + nr.uv_texture_regularizer(albedo, smooth=1.0, anchor=1.0, reference=start)
            loss.backward()
            zero = (albedo.grad == 0).all(-1)
            untouched = zero if untouched is None else untouched & zero
            opt.step()
        return albedo.detach(), untouched

    plain, untouched = fit(False)
    assert 0 < int(untouched.sum()) < H * W
    assert torch.equal(_bits(plain)[untouched], _bits(start)[untouched]) and not torch.equal(plain[~untouched], start[~untouched])
    moved, none_untouched = fit(True)
    assert not bool(none_untouched.any())
    assert bool((moved[untouched] != start[untouched]).any(-1).all())
