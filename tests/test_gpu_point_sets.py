"""Nearest points and chamfer distances on the device (neural_renderer/point_sets.py, csrc/d3m_point_sets.h, core/mesh_eval.py)
against the float64 brute-force restatement of tests/point_set_scenes.py.  Lattice cases: index and squared distance bit for
bit.  Random cases: the scenes file's rounding BOUND.  Value and gradients: its DEVICE_TOLERANCE, 8 x the largest float32
yardstick of each kind (tests/test_point_sets_host.py holds the figures), plus the quantum bound where a gradient holds
scattered terms.  Everything the header calls exact is compared by bits."""
import numpy as np
import pytest
import torch

import point_set_scenes as S
from conftest import kernels_launched
from deep3dmap_amd.neural_renderer import point_sets as PS

pytestmark = pytest.mark.gpu
CASE = {S.case_id(c): c for c in S.CASES}
LATTICE = tuple(c for c in S.CASES if c[0] == "lattice")
RANDOM = tuple(c for c in S.CASES if c[0] == "random")


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _cuda(t):
    return None if t is None else t.cuda()


def _search(case, splits=None, swap=False):
    """(index, dist2) of nr.nearest_points on a case's sets (swap: b's points in a)"""
    from deep3dmap_amd import neural_renderer as nr
    i = S.case_inputs(case)
    sets = (i["b"], i["a"], i["b_lengths"], i["a_lengths"]) if swap else (i["a"], i["b"], i["a_lengths"], i["b_lengths"])
    return nr.nearest_points(*(_cuda(t) for t in sets), _splits=splits)


def _run(case, option, splits=None, a=None, b=None, upstream=None):
    """(value [B], grad_a, grad_b) of nr.chamfer_distance on a case's inputs under an option, on the device"""
    from deep3dmap_amd import neural_renderer as nr
    i = S.case_inputs(case)
    x = (i["a"] if a is None else a).cuda().requires_grad_(True)
    y = (i["b"] if b is None else b).cuda().requires_grad_(True)
    kw = S.options_of(case, option) if isinstance(option, str) else option
    value = nr.chamfer_distance(x, y, _cuda(i["a_lengths"]), _cuda(i["b_lengths"]), _splits=splits, **kw)
    ga, gb = torch.autograd.grad(value, (x, y), (i["upstream"] if upstream is None else upstream).cuda())
    return value.detach(), ga, gb


# ---- 1. the search ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LATTICE, ids=S.case_id)
def test_lattice_index_and_distance_bit_for_bit(case):
    """Exact arithmetic, many exact ties: the lowest index wins, for every split count and in both directions."""
    ref = S.reference(case, "squared")
    for swap, (want_index, want_d2) in ((False, (ref["index_ab"], ref["dist2_ab"])), (True, (ref["index_ba"], ref["dist2_ba"]))):
        for splits in (None,) + S.SPLITS:
            index, dist2 = _search(case, splits, swap)
            assert index.dtype == torch.int32 and index.shape == want_index.shape and dist2.shape == want_d2.shape
            assert torch.equal(index.cpu(), want_index), (swap, splits)
            assert torch.equal(_bits(dist2).cpu(), _bits(want_d2.float())), (swap, splits)


@pytest.mark.parametrize("case", RANDOM, ids=S.case_id)
def test_random_distance_within_the_rounding_bound(case):
    """dist2 and the float64 distance to the returned index, both within BOUND of the float64 minimum; -1 and +0 where the node
    says so.  No index is compared."""
    ref = S.reference(case, "squared")
    inputs = S.case_inputs(case)
    la, lb = S.lengths_of(inputs)
    for splits in (None,) + S.SPLITS:
        index, dist2 = (t.cpu() for t in _search(case, splits))
        worst = 0.0
        for e in range(index.shape[0]):
            n, m = la[e], lb[e]
            used = n if m > 0 else 0
            assert bool((index[e, used:] == -1).all()) and not bool(_bits(dist2[e, used:]).any())
            if used == 0:
                continue
            j = index[e, :n].long()
            assert bool((j >= 0).all()) and bool((j < m).all())
            best = ref["dist2_ab"][e, :n]
            d = inputs["a"][e, :n].double() - inputs["b"][e, :m].double()[j]
            to_index = (d * d).sum(-1)
            worst = max(worst, float(((dist2[e, :n].double() - best).abs() / best).max()),
                        float(((to_index - best).abs() / best).max()))
        print(S.case_id(case), "splits", splits, "largest relative deviation from the float64 minimum: %.2e" % worst,
              "allowed: %.2e" % S.BOUND)
        assert worst <= S.BOUND, (splits, worst)


# ---- 2. value and gradients of every case and option -------------------------------------------------------------------------------
@pytest.mark.parametrize("option", S.OPTIONS)
@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_value_and_gradients_against_the_float64_reference(case, option):
    ref = S.reference(case, option)
    inputs = S.case_inputs(case)
    value, ga, gb = _run(case, option)
    kw = S.options_of(case, option)
    q = S.quantum(ref, inputs)
    # a gradient holds scattered terms iff the OTHER set's points are queries
    scattered = dict(grad_a=kw.get("weight_ba", 1.0) > 0, grad_b=kw.get("weight_ab", 1.0) > 0)
    counts = dict(grad_a=S.sources(ref["index_ba"], ga.shape[1]), grad_b=S.sources(ref["index_ab"], gb.shape[1]))
    for kind, got in (("value", value), ("grad_a", ga), ("grad_b", gb)):
        want = ref[kind]
        assert got.shape == want.shape and bool(torch.isfinite(got).all())
        scale = float(want.abs().max()) or 1.0
        allowed = torch.full(want.shape, S.DEVICE_TOLERANCE[kind] * scale, dtype=torch.float64)
        if kind != "value" and scattered[kind]:
            allowed = allowed + ((counts[kind].double() / 2 + 1) * q)[..., None]
        err = (got.cpu().double() - want).abs()
        print(S.case_id(case), option, kind, "error / largest entry: %.2e" % (float(err.max()) / scale),
              "allowed: %.2e" % S.DEVICE_TOLERANCE[kind], "quantum: %.1e" % q)
        assert bool((err <= allowed).all()), (kind, float(err.max()) / scale)


# ---- 3. exact things -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", (CASE["lattice-blocks-B1-N1025-M1027"], CASE["random-blocks-B1-N1025-M1027"],
                                  CASE["random-ragged-B3-N65-M1027"], CASE["lattice-empty-B3-N1025-M513"]), ids=S.case_id)
def test_the_same_bits_on_two_runs_and_for_every_split_count(case):
    for option in ("distance", "truncated", "weighted"):
        first = _run(case, option)
        for splits in (None,) + S.SPLITS:
            again = _run(case, option, splits)
            for x, y in zip(first, again):
                assert torch.equal(_bits(x), _bits(y)), (option, splits)
    for swap in (False, True):
        first = _search(case, None, swap)
        for splits in (None,) + S.SPLITS:
            again = _search(case, splits, swap)
            assert torch.equal(first[0], again[0]) and torch.equal(_bits(first[1]), _bits(again[1])), (swap, splits)


@pytest.mark.parametrize("family", S.FAMILIES)
def test_unused_points_and_truncated_terms_get_plus_zero(family):
    case = CASE["%s-empty-B3-N1025-M513" % family]
    inputs = S.case_inputs(case)
    la, lb = S.lengths_of(inputs)
    e0 = S.EMPTY_TARGET_ELEMENT
    assert lb[e0] == 0 and la[e0] > 1
    for option in S.OPTIONS:
        value, ga, gb = _run(case, option)
        for e in range(3):
            assert not bool(_bits(ga[e, la[e]:]).any()) and not bool(_bits(gb[e, lb[e]:]).any()), (option, e)
        assert not bool(_bits(ga[e0]).any()) and not bool(_bits(gb[e0]).any()) and int(_bits(value)[e0]) == 0, option
        assert float(ga[0].abs().max()) > 0 and float(gb[0].abs().max()) > 0
    # one direction with truncation: the truncated queries' gradients are direct terms only, exactly +0
    ref = S.reference(case, "squared")
    tau = S.TAU[family]
    tau2 = float(np.float32(tau) * np.float32(tau))
    value, ga, gb = _run(case, dict(truncate=tau, weight_ba=0.0))
    cut = ref["dist2_ab"] > tau2
    assert 0 < int(cut[0, :la[0]].sum()) < la[0]
    assert not bool(_bits(ga).cpu()[cut].any()) and bool((ga.cpu()[0, :la[0]][~cut[0, :la[0]]] != 0).any())
    index, dist2 = _search(case)
    assert bool((index[e0] == -1).all()) and not bool(_bits(dist2[e0]).any())


def test_zero_upstream_gives_plus_zero_everywhere():
    case = CASE["random-ragged-B3-N65-M1027"]
    value, ga, gb = _run(case, "weighted", upstream=torch.zeros(3))
    assert not bool(_bits(ga).any()) and not bool(_bits(gb).any()) and float(value.abs().min()) > 0


def test_nan_in_gives_nan_out_and_the_process_goes_on():
    from deep3dmap_amd import neural_renderer as nr
    case = CASE["random-ragged-B3-N65-M1027"]
    inputs = S.case_inputs(case)
    a = inputs["a"].clone()
    a[0, 3, 1] = float("nan")
    index, dist2 = nr.nearest_points(a.cuda(), inputs["b"].cuda(), _cuda(inputs["a_lengths"]), _cuda(inputs["b_lengths"]))
    clean = _search(case)
    assert int(index[0, 3]) == -1 and bool(torch.isnan(dist2[0, 3]))
    keep = torch.ones_like(index, dtype=torch.bool)
    keep[0, 3] = False
    assert torch.equal(index[keep], clean[0][keep]) and torch.equal(_bits(dist2)[keep], _bits(clean[1])[keep])
    for option in ("squared", "distance", "truncated"):
        value, ga, gb = _run(case, option, a=a)
        assert bool(torch.isnan(value[0])) and bool(torch.isfinite(value[1:]).all())
        assert bool(torch.isnan(ga).all()) and bool(torch.isnan(gb).all())
    b = inputs["b"].clone()
    b[0, 7] = float("inf")                                   # an infinite target is never the nearest: nothing else changes
    index, dist2 = nr.nearest_points(inputs["a"].cuda(), b.cuda(), _cuda(inputs["a_lengths"]), _cuda(inputs["b_lengths"]))
    assert bool(torch.isfinite(dist2).all()) and not bool((index[0] == 7).any())
    torch.cuda.synchronize()
    assert torch.equal(_search(case)[0], clean[0])          # the device still answers


def test_nearest_points_is_differentiable_through_the_same_adjoint():
    """sum(dist2 w) / n through nearest_points equals chamfer_distance of one direction: the same direct terms (2 w (a - b_nn)),
    the same scatter."""
    from deep3dmap_amd import neural_renderer as nr
    case = CASE["random-above-B1-N65-M513"]
    inputs = S.case_inputs(case)
    a = inputs["a"].cuda().requires_grad_(True)
    b = inputs["b"].cuda().requires_grad_(True)
    index, dist2 = nr.nearest_points(a, b)
    assert not index.requires_grad and dist2.requires_grad
    w = torch.linspace(-1.0, 2.0, a.shape[1]).cuda()[None]
    ga, gb = torch.autograd.grad((dist2 * w).sum(), (a, b))
    j = index[0].long()
    direct = 2 * w[0, :, None].double() * (a.detach()[0].double() - b.detach()[0].double()[j])
    want_b = torch.zeros_like(direct[:1].expand(b.shape[1], 3)).index_add(0, j, -direct)
    scale = float(direct.abs().max())
    assert float((ga[0].double() - direct).abs().max()) <= 4 * S.U * scale
    counts = torch.bincount(j, minlength=b.shape[1]).double()
    assert bool(((gb[0].double() - want_b).abs() <= (4 * S.U * scale) * (counts[:, None] + 1)).all())
    # unbatched sets: the same bits without the batch dimension
    a2, b2 = inputs["a"][0].cuda().requires_grad_(True), inputs["b"][0].cuda().requires_grad_(True)
    index2, dist22 = nr.nearest_points(a2, b2)
    g2 = torch.autograd.grad((dist22 * w[0]).sum(), (a2, b2))
    assert index2.shape == (65,) and torch.equal(index2, index[0]) and torch.equal(_bits(dist22), _bits(dist2[0]))
    assert torch.equal(_bits(g2[0]), _bits(ga[0])) and torch.equal(_bits(g2[1]), _bits(gb[0]))


# ---- 4. capture and launches -----------------------------------------------------------------------------------------------------------
def test_captured_forward_and_backward():
    """Forward plus backward under torch.cuda.graph (CapturedStep), replayed after the sets, the lengths and the upstream
    gradient are rewritten in place; a replay has the bits of the eager run."""
    from deep3dmap_amd import neural_renderer as nr
    from deep3dmap_amd.graph import CapturedStep
    case = CASE["random-ragged-B3-N65-M1027"]
    i = S.case_inputs(case)
    sets_a = [i["a"].cuda(), (i["a"].flip(1) * 0.5).cuda()]
    sets_b = [i["b"].cuda(), (i["b"].flip(0) + 0.25).cuda()]
    lens = [i["b_lengths"].cuda(), torch.tensor([7, 1027, 600], dtype=torch.int32).cuda()]
    ups = [i["upstream"].cuda(), torch.tensor([0.3, -0.2, 1.1]).cuda()]
    la = i["a_lengths"].cuda()
    kw = dict(squared=False, truncate=0.25, weight_ab=0.7, weight_ba=1.3)

    def step(x, y, lb, g):
        value = nr.chamfer_distance(x, y, la, lb, **kw)
        return (value,) + torch.autograd.grad(value, (x, y), g)

    def fresh():
        return (sets_a[0].clone().requires_grad_(True), sets_b[0].clone().requires_grad_(True), lens[0].clone(), ups[0].clone())

    twin, live = fresh(), fresh()
    eager = []
    for k in (0, 1):
        with torch.no_grad():
            for dst, src in zip(twin, (sets_a, sets_b, lens, ups)):
                dst.copy_(src[k])
        with kernels_launched() as kl:
            eager.append([t.clone() for t in step(*twin)])
        assert kl.names == set(PS.KERNELS_FORWARD) | set(PS.KERNELS_BACKWARD), kl.names
    assert not torch.equal(eager[0][0], eager[1][0]) and not torch.equal(eager[0][1], eager[1][1])
    torch.cuda.synchronize()
    cs = CapturedStep(lambda: step(*live)).capture()
    for k in (1, 0):
        with torch.no_grad():
            for dst, src in zip(live, (sets_a, sets_b, lens, ups)):
                dst.copy_(src[k])
        got = [t.clone() for t in cs()]
        torch.cuda.synchronize()
        for x, y in zip(got, eager[k]):
            assert torch.equal(_bits(x), _bits(y)), k


@pytest.mark.parametrize("case", (CASE["lattice-one-B1-N1-M1"], CASE["random-blocks-B1-N1025-M1027"],
                                  CASE["random-few_many-B1-N1-M1027"], CASE["lattice-empty-B3-N1025-M513"]), ids=S.case_id)
def test_launch_counts_are_the_headers(case):
    """nearest_points 3, chamfer_distance 4 forward, 3 backward, whatever the shapes, the lengths, the options and the splits."""
    from deep3dmap_amd import neural_renderer as nr
    i = S.case_inputs(case)
    for option in S.OPTIONS:
        for splits in (None, 5):
            x, y = i["a"].cuda().requires_grad_(True), i["b"].cuda().requires_grad_(True)
            with kernels_launched() as kf:
                value = nr.chamfer_distance(x, y, _cuda(i["a_lengths"]), _cuda(i["b_lengths"]), _splits=splits,
                                            **S.options_of(case, option))
            with kernels_launched() as kb:
                value.backward(i["upstream"].cuda())
            forward, backward = ({k: v[0] for k, v in t.times.items()} for t in (kf, kb))
            assert forward == dict.fromkeys(PS.KERNELS_FORWARD, 1) and sum(forward.values()) <= 5, (option, forward)
            assert backward == dict.fromkeys(PS.KERNELS_BACKWARD, 1) and sum(backward.values()) <= 4, (option, backward)
    x, y = i["a"].cuda().requires_grad_(True), i["b"].cuda().requires_grad_(True)
    with kernels_launched() as kf:
        index, dist2 = nr.nearest_points(x, y, _cuda(i["a_lengths"]), _cuda(i["b_lengths"]))
    with kernels_launched() as kb:
        dist2.sum().backward()
    assert {k: v[0] for k, v in kf.times.items()} == dict.fromkeys(PS.KERNELS_NEAREST, 1)
    assert {k: v[0] for k, v in kb.times.items()} == dict.fromkeys(PS.KERNELS_BACKWARD, 1)
    for name in PS.KERNELS_FORWARD + PS.KERNELS_BACKWARD:
        assert name in PS.__doc__


# ---- 5. the module, unbatched sets, the entry point ---------------------------------------------------------------------------------------
def test_module_and_unbatched_sets_equal_the_function():
    from deep3dmap_amd import neural_renderer as nr
    case = CASE["random-above-B1-N65-M513"]
    i = S.case_inputs(case)
    kw = dict(squared=False, truncate=0.25, weight_ab=0.7, weight_ba=1.3)
    want = _run(case, kw)
    module = nr.ChamferTarget(i["b"][0], **kw).cuda()
    assert set(dict(module.named_buffers())) == {"target_points"} and not list(module.parameters())
    for x in (i["a"][0], i["a"]):                          # [N,3] -> 0-d; [B,N,3] with the [M,3] target repeated
        leaf = x.cuda().requires_grad_(True)
        value = module(leaf)
        grad, = torch.autograd.grad(value, leaf, i["upstream"].cuda()[0] if x.dim() == 2 else i["upstream"].cuda())
        assert value.dim() == x.dim() - 2 and torch.equal(_bits(value).reshape(-1), _bits(want[0]))
        assert torch.equal(_bits(grad).reshape(-1), _bits(want[1]).reshape(-1))
    # sets that are not contiguous are made so by the node
    wide = torch.zeros(1, 65, 5, device="cuda")
    wide[..., 1:4] = i["a"].cuda()
    view = wide[..., 1:4].detach().requires_grad_(True)
    value = nr.chamfer_distance(view, i["b"].cuda(), **kw)
    grad, = torch.autograd.grad(value, view, i["upstream"].cuda())
    assert torch.equal(_bits(value), _bits(want[0])) and torch.equal(_bits(grad), _bits(want[1]))


def test_entry_point_writes_every_element_over_poisoned_buffers():
    from deep3dmap_amd import _lib
    L = _lib.lib()
    case = CASE["random-empty-B3-N1025-M513"]
    i = S.case_inputs(case)
    B, N, M = case[2:]
    a, b, la, lb, up = (i[k].cuda() for k in ("a", "b", "a_lengths", "b_lengths", "upstream"))
    want = _run(case, "weighted")
    nan = float("nan")
    words = int(L.d3m_chamfer_distance_scratch_bytes(B, N, M)) // 8 + 1
    scratch = torch.full((words,), -1, dtype=torch.int64, device="cuda")
    ints = lambda n: torch.full((B, n), -7, dtype=torch.int32, device="cuda")
    floats = lambda *s: torch.full(s, nan, device="cuda")
    iab, dab, iba, dba, coef, value = ints(N), floats(B, N), ints(M), floats(B, M), floats(B, 2), floats(B)
    _lib.check(L.d3m_chamfer_distance(_lib.ptr(a), _lib.ptr(b), B, N, M, _lib.ptr(la), _lib.ptr(lb), 1, -1.0, 0.7, 1.3, 0,
                                      _lib.ptr(scratch), words * 8, _lib.ptr(iab), _lib.ptr(dab), _lib.ptr(iba), _lib.ptr(dba),
                                      _lib.ptr(coef), _lib.ptr(value), None), "forward")
    assert torch.equal(_bits(value), _bits(want[0]))
    assert not bool(torch.isnan(dab).any()) and not bool(torch.isnan(dba).any()) and int(iab.min()) >= -1 and int(iba.min()) >= -1
    lengths = S.lengths_of(i)
    for e in range(B):
        n, m = lengths[0][e], lengths[1][e]
        expect = [0.7 / n if n else 0.0, 1.3 / m if m else 0.0]
        assert torch.allclose(coef[e].cpu().double(), torch.tensor(expect, dtype=torch.float64), rtol=1e-7, atol=0)
    scratch.fill_(-1)
    ga, gb = floats(B, N, 3), floats(B, M, 3)
    _lib.check(L.d3m_chamfer_distance_backward(_lib.ptr(a), _lib.ptr(b), B, N, M, _lib.ptr(la), _lib.ptr(lb), _lib.ptr(iab),
                                               _lib.ptr(dab), _lib.ptr(iba), _lib.ptr(dba), _lib.ptr(coef), _lib.ptr(up), 0, 1,
                                               -1.0, _lib.ptr(scratch), words * 8, _lib.ptr(ga), _lib.ptr(gb), None), "backward")
    assert torch.equal(_bits(ga), _bits(want[1])) and torch.equal(_bits(gb), _bits(want[2]))


# ---- 6. mesh_eval -----------------------------------------------------------------------------------------------------------------------
def test_eval_points_against_the_restatement():
    from deep3dmap_amd import core
    case = CASE["random-blocks-B1-N1025-M1027"]
    i = S.case_inputs(case)
    pred, trgt = i["a"][0], i["b"][0]
    ref = S.reference(case, "squared")
    to_trgt, to_pred = ref["dist2_ab"][0].sqrt(), ref["dist2_ba"][0].sqrt()          # per predicted point; per target point
    threshold = float(to_trgt.median())
    got = core.eval_points(pred.numpy(), trgt, threshold)
    want = dict(dist1=float(to_trgt.mean()), dist2=float(to_pred.mean()), prec=float((to_trgt < threshold).double().mean()),
                recal=float((to_pred < threshold).double().mean()))
    want["fscore"] = 2 * want["prec"] * want["recal"] / (want["prec"] + want["recal"])
    assert set(got) == set(want) and 0.3 < want["prec"] < 0.7
    # a distance within 13 u of the threshold may fall on either side of it: at most one point of each set here
    for k in ("dist1", "dist2"):
        assert abs(got[k] - want[k]) <= 1e-6 * want[k], k
    assert abs(got["prec"] - want["prec"]) <= 1 / 1025 and abs(got["recal"] - want["recal"]) <= 1 / 1027
    assert abs(got["fscore"] - 2 * got["prec"] * got["recal"] / (got["prec"] + got["recal"])) <= 1e-12
    far = core.eval_points(pred, trgt + 100.0, 0.05)
    assert far["prec"] == 0.0 and far["recal"] == 0.0 and np.isnan(far["fscore"])
    index, distance = core.nn_correspondance(trgt, pred.numpy())                        # for each point of pred, the nearest of trgt
    assert torch.equal(index.cpu(), ref["index_ab"][0]) and float((distance.cpu().double() - to_trgt).abs().max()) <= 1e-6
    assert core.nn_correspondance(np.zeros((0, 3)), pred) == ([], []) and core.nn_correspondance(pred, []) == ([], [])


# ---- 7. end to end -----------------------------------------------------------------------------------------------------------------------
def test_points_move_onto_a_sphere():
    """200 points moved onto 300 points of the unit sphere by Adam steps of chamfer_distance: the fit of
    point_set_scenes.restatement_fit, whose own run in float64 on the CPU brings the loss down by a factor of
    RESTATEMENT_FIT_FACTOR (tests/test_point_sets_host.py measures it again); half of that is asked for here."""
    from deep3dmap_amd import neural_renderer as nr
    start, target = S.fit_points()
    first, last = S.adam_fit(start.cuda(), lambda x: nr.chamfer_distance(x, target.cuda()))
    print("loss %.4f -> %.5f: a factor of %.1f; the restatement's: %.1f" % (first, last, first / last, S.RESTATEMENT_FIT_FACTOR))
    assert first / last >= S.RESTATEMENT_FIT_FACTOR / 2


def test_a_closed_mesh_moves_onto_a_sphere_with_the_regulariser():
    """The same fit on the 66 vertices of an octahedron subdivided twice, shrunk, with nr.MeshRegularizer beside
    nr.ChamferTarget: the data term falls by at least half the factor that the restatement's fit with a restated Laplacian
    term reaches."""
    from deep3dmap_amd import neural_renderer as nr
    vertices, faces, target = S.fit_mesh()
    data = nr.ChamferTarget(target).cuda()
    prior = nr.MeshRegularizer(faces, laplacian=S.FIT_LAPLACIAN).cuda()
    first, last = S.adam_fit(vertices.cuda(), data, prior)
    print("data term %.4f -> %.5f: a factor of %.1f; the restatement's: %.1f" % (first, last, first / last, S.RESTATEMENT_MESH_FIT_FACTOR))
    assert first / last >= S.RESTATEMENT_MESH_FIT_FACTOR / 2
