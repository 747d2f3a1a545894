"""Nearest points and chamfer distances without a device (neural_renderer/point_sets.py, csrc/d3m_point_sets.h,
core/mesh_eval.py): the float64 restatement of tests/point_set_scenes.py against central finite differences, against known
answers by hand and against scipy's k-d tree; what the cases are there for (exact ties in every lattice case, no near-ties in
the random ones); eval_points' metrics by hand; the float32 yardsticks behind the device tolerances; the restatement's own
end-to-end fits; every argument error; the C entry points' refusals."""
import ctypes

import numpy as np
import pytest
import torch

import point_set_scenes as S
from deep3dmap_amd.neural_renderer import point_sets as PS

FD_STEP = 1e-6
FD_AGREEMENT = 1e-6       # of the largest gradient entry (test_uv_texture_regularizers_host.py's step and rule)
FD_TAU = 0.5              # the truncation distance of the finite-difference case: 7 points against 9


# ---- 1. the restatement against central finite differences ---------------------------------------------------------------------
def _fd_inputs():
    gen = torch.Generator().manual_seed(3)
    a, b = torch.rand(1, 7, 3, generator=gen) * 2 - 1, torch.rand(1, 9, 3, generator=gen) * 2 - 1
    return dict(a=a, b=b, a_lengths=None, b_lengths=None, upstream=torch.tensor([0.7]))


def test_the_finite_difference_case_is_clear_of_every_kink():
    """The nn is a constant of differentiation: a step must not change it.  Moving one point by h changes a distance by at most
    h, so a gap of more than 4 h between the best and the second-best distance of every point, in both directions, keeps every
    nn; likewise no distance is within 4 h of the truncation distance, and none is 0."""
    i = _fd_inputs()
    for p, q in ((i["a"][0], i["b"][0]), (i["b"][0], i["a"][0])):
        D = S.pair_distances(p, q).sqrt().sort(1).values
        assert float((D[:, 1] - D[:, 0]).min()) > 4 * FD_STEP
        assert float((D[:, 0] - FD_TAU).abs().min()) > 4 * FD_STEP and float(D[:, 0].min()) > 4 * FD_STEP
        assert bool((D[:, 0] > FD_TAU).any()) and bool((D[:, 0] < FD_TAU).any())          # both sides of the truncation occur


@pytest.mark.parametrize("option", S.OPTIONS)
def test_restatement_against_finite_differences(option):
    i = _fd_inputs()
    kw = dict(S.OPTIONS[option])
    if kw.get("truncate"):
        kw["truncate"] = FD_TAU
    ref = S.evaluate(i, kw)
    la, lb = S.lengths_of(i)

    def loss(a, b):
        ab, ba = S.nearest_points(a, b, la, lb)[0], S.nearest_points(b, a, lb, la)[0]          # found anew at every step
        return float((S.value_of(a, b, la, lb, ab, ba, **kw) * i["upstream"].double()).sum())

    for name, grad in (("a", ref["grad_a"]), ("b", ref["grad_b"])):
        fd = torch.zeros_like(grad)
        for k in range(grad.numel()):
            sets = {"a": [i["a"].double().clone(), i["a"].double().clone()], "b": [i["b"].double().clone(), i["b"].double().clone()]}
            sets[name][0].view(-1)[k] -= FD_STEP
            sets[name][1].view(-1)[k] += FD_STEP
            fd.view(-1)[k] = (loss(sets["a"][1], sets["b"][1]) - loss(sets["a"][0], sets["b"][0])) / (2 * FD_STEP)
        err = float((grad - fd).abs().max()) / float(grad.abs().max())
        print(option, name, "largest |autograd - finite differences| / largest entry:", err)
        assert float(grad.abs().max()) > 0 and err <= FD_AGREEMENT, (name, err)


# ---- 2. known answers by hand ----------------------------------------------------------------------------------------------------------
def test_known_answers_on_a_line():
    """a = 0, 1, 3 and b = 0.5, 4 on the x axis.  a -> b: 0 and 1 go to 0.5 (d = 0.5), 3 goes to 4 (d = 1).  b -> a: 0.5 is as
    far from 0 as from 1 -- the lower index, 0 --, 4 goes to 3.  Squared: L_ab = (0.25 + 0.25 + 1) / 3 = 0.5, L_ba = 1.25 / 2.
    Distances: L_ab = 2 / 3, L_ba = 0.75.  tau = 0.75 truncates the terms of d = 1 to 0.5625 and 0.75; tau = 1 truncates
    nothing (equality).  Gradients of L_ab squared: a gets 2 (a - b_nn) / 3 = -1/3, 1/3, -2/3; b gets minus the sums: 0, 2/3."""
    line = lambda xs: torch.tensor([[[x, 0.0, 0.0] for x in xs]])
    i = dict(a=line([0.0, 1.0, 3.0]), b=line([0.5, 4.0]), a_lengths=None, b_lengths=None, upstream=torch.tensor([1.0]))
    r = S.evaluate(i, dict())
    assert r["index_ab"].tolist() == [[0, 0, 1]] and r["index_ba"].tolist() == [[0, 2]]
    assert r["dist2_ab"].tolist() == [[0.25, 0.25, 1.0]] and r["dist2_ba"].tolist() == [[0.25, 1.0]]
    near = lambda v, w: abs(float(v) - w) <= 1e-14
    assert near(r["value"][0], 0.5 + 0.625)
    assert near(S.evaluate(i, dict(weight_ba=0.0))["value"][0], 0.5) and near(S.evaluate(i, dict(weight_ab=0.0))["value"][0], 0.625)
    assert near(S.evaluate(i, dict(squared=False, weight_ba=0.0))["value"][0], 2 / 3)
    assert near(S.evaluate(i, dict(squared=False, weight_ab=0.0, weight_ba=2.0))["value"][0], 1.5)
    assert near(S.evaluate(i, dict(truncate=0.75))["value"][0], (0.25 + 0.25 + 0.5625) / 3 + (0.25 + 0.5625) / 2)
    assert near(S.evaluate(i, dict(truncate=0.75, squared=False))["value"][0], (0.5 + 0.5 + 0.75) / 3 + (0.5 + 0.75) / 2)
    assert near(S.evaluate(i, dict(truncate=1.0))["value"][0], 0.5 + 0.625)
    g = S.evaluate(i, dict(weight_ba=0.0))
    assert torch.allclose(g["grad_a"][0, :, 0], torch.tensor([-1 / 3, 1 / 3, -2 / 3], dtype=torch.float64), rtol=0, atol=1e-15)
    assert torch.allclose(g["grad_b"][0, :, 0], torch.tensor([0.0, 2 / 3], dtype=torch.float64), rtol=0, atol=1e-15)
    assert not bool(g["grad_a"][..., 1:].any()) and abs(g["gmax"] - 2 / 3) <= 1e-15
    cut = S.evaluate(i, dict(weight_ba=0.0, truncate=0.75))                     # the truncated term has no gradient
    assert cut["grad_a"][0, :, 0].tolist() == g["grad_a"][0, :2, 0].tolist() + [0.0] and not bool(cut["grad_b"][0, 1].any())
    d = S.evaluate(i, dict(weight_ba=0.0, squared=False))                       # rho' = 1 / d: unit vectors / 3
    assert torch.allclose(d["grad_a"][0, :, 0], torch.tensor([-1 / 3, 1 / 3, -1 / 3], dtype=torch.float64), rtol=0, atol=1e-15)
    same = dict(i, b=line([0.0, 4.0]))                                          # a_0 == b_0: rho'(0) is 0, not infinite
    z = S.evaluate(same, dict(squared=False))
    assert bool(torch.isfinite(z["grad_a"]).all()) and not bool(z["grad_a"][0, 0].any())


def test_lengths_and_empty_sets_in_the_restatement():
    line = lambda xs: torch.tensor([[x, 0.0, 0.0] for x in xs])
    i = dict(a=torch.stack([line([0.0, 1.0, 9.0])] * 3), b=torch.stack([line([0.5, 4.0])] * 3),
             a_lengths=torch.tensor([3, 2, 2], dtype=torch.int32), b_lengths=torch.tensor([2, 1, 0], dtype=torch.int32),
             upstream=torch.ones(3))
    r = S.evaluate(i, dict())
    assert r["index_ab"].tolist() == [[0, 0, 1], [0, 0, -1], [-1, -1, -1]] and r["index_ba"].tolist() == [[0, 1], [0, -1], [-1, -1]]
    assert r["dist2_ab"][1].tolist() == [0.25, 0.25, 0.0] and not bool(r["dist2_ab"][2].any())
    assert abs(float(r["value"][1]) - 0.5) <= 1e-15 and float(r["value"][2]) == 0.0
    assert not bool(r["grad_a"][1, 2].any()) and not bool(r["grad_a"][2].any()) and not bool(r["grad_b"][1, 1].any())


def test_eval_points_metrics_by_hand():
    """Four predicted points at distances 0.01, 0.02, 0.2, 0.3 from the target, two target points at 0.04 and 0.5 from the
    prediction, threshold 0.05: prec = 2/4, recal = 1/2, fscore = 0.5; the reference's dict calls the mean over the
    PREDICTION's points dist1 and the mean over the target's dist2 (its locals are numbered the other way)."""
    from deep3dmap_amd import core
    from deep3dmap_amd.core import mesh_eval
    assert core.eval_points is mesh_eval.eval_points and core.nn_correspondance is mesh_eval.nn_correspondance
    to_trgt, to_pred = torch.tensor([0.01, 0.02, 0.2, 0.3]), torch.tensor([0.04, 0.5])
    m = mesh_eval.metrics_of(to_pred, to_trgt, 0.05)
    assert list(m) == ["dist1", "dist2", "prec", "recal", "fscore"]
    assert abs(m["dist1"] - 0.1325) <= 1e-7 and abs(m["dist2"] - 0.27) <= 1e-7
    assert m["prec"] == 0.5 and m["recal"] == 0.5 and abs(m["fscore"] - 0.5) <= 1e-15
    m = mesh_eval.metrics_of(to_pred, to_trgt, 0.005)                        # nothing within the threshold: 0 / 0
    assert m["prec"] == 0.0 and m["recal"] == 0.0 and np.isnan(m["fscore"])
    assert mesh_eval.metrics_of(torch.tensor([0.05]), torch.tensor([0.05]), 0.05)["prec"] == 0.0      # strictly below, as the reference's `<`
    assert core.nn_correspondance(np.zeros((0, 3)), np.zeros((4, 3))) == ([], [])
    assert core.nn_correspondance(torch.zeros(4, 3), []) == ([], [])
    assert all(np.isnan(v) for v in core.eval_points(np.zeros((0, 3)), np.zeros((4, 3))).values())
    with pytest.raises(ValueError, match="num_points, 3"):
        core.nn_correspondance(np.zeros((4, 2)), np.zeros((4, 3)))
    if not torch.cuda.is_available():
        with pytest.raises(ValueError, match="GPU"):
            core.eval_points(np.zeros((4, 3)), np.ones((4, 3)))
    assert "voxel_down_sample" in mesh_eval.__doc__ and "OUT OF SCOPE" in mesh_eval.__doc__


def test_restatement_against_scipys_tree():
    spatial = pytest.importorskip("scipy.spatial")
    for case in (c for c in S.CASES if c[0] == "random" and c[1] in ("above", "blocks", "few_many")):
        i = S.case_inputs(case)
        ref = S.reference(case, "squared")
        for p, q, index, d2 in ((i["a"][0], i["b"][0], ref["index_ab"][0], ref["dist2_ab"][0]),
                                (i["b"][0], i["a"][0], ref["index_ba"][0], ref["dist2_ba"][0])):
            distance, j = spatial.cKDTree(q.double().numpy()).query(p.double().numpy())
            assert np.array_equal(j, index.numpy()) and np.allclose(distance ** 2, d2.numpy(), rtol=1e-12, atol=0)


# ---- 3. the cases and the yardsticks ---------------------------------------------------------------------------------------------------
def test_the_shapes_follow_the_kernels_tile_and_queries_per_lane():
    from deep3dmap_amd import _lib
    L = _lib.lib()
    assert (S.T, S.Q) == (PS.TILE, PS.QUERIES_PER_LANE) == (L.d3m_point_set_tile(), L.d3m_point_set_queries_per_lane())
    T, Q = S.T, S.Q
    assert {c[3] for c in S.CASES} == {1, 63, 64, 65, 256 * Q + 1} and {c[4] for c in S.CASES} == {1, T - 1, T, T + 1, 2 * T + 3}
    assert {c[2] for c in S.CASES} == {1, 3} and S.SPLITS == (1, 2, 5) and (2 * T + 3 + T - 1) // T == 3 and 3 % 2
    assert PS.auto_splits(1, 1, 1) == 1 and PS.auto_splits(1, 1, 2 * T + 3) == 3 and PS.auto_splits(1, 256 * Q + 1, 1) == 1
    assert PS.auto_splits(1, 50625, 50625) == 21 and PS.auto_splits(8, 50625, 50625) == 3
    assert PS.auto_splits(1, 5000, 1000000) == 205 and PS.auto_splits(1, 1000000, 5000) == 2
    assert PS.auto_splits(0, 1, 1) == 0 == PS.auto_splits(1, (1 << 30) + 1, 1)


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_cases_have_what_they_are_there_for(case):
    family, name, B, N, M = case
    i = S.case_inputs(case)
    la, lb = S.lengths_of(i)
    assert i["a"].shape == (B, N, 3) and i["b"].shape == (B, M, 3) and i["a"].dtype == i["b"].dtype == torch.float32
    up = i["upstream"]
    assert up.shape == (B,) and (B == 1 or (bool((up > 0).any()) and bool((up < 0).any())))
    if B == 3:
        assert 1 in la and max(la) == N and max(lb) == M and min(la) < N
        assert (0 in lb) == (name == "empty") and (name != "empty" or lb[S.EMPTY_TARGET_ELEMENT] == 0)
    ties = near_ties = 0
    for e in range(B):
        for p, q in ((i["a"][e, :la[e]], i["b"][e, :lb[e]]), (i["b"][e, :lb[e]], i["a"][e, :la[e]])):
            if p.shape[0] == 0 or q.shape[0] < 2:
                continue
            D = S.pair_distances(p, q).sort(1).values
            ties += int((D[:, 1] == D[:, 0]).sum())
            near_ties += int((D[:, 1] - D[:, 0] <= 4 * S.BOUND * D[:, 0]).sum())
    if family == "lattice":
        k = torch.cat((i["a"].reshape(-1), i["b"].reshape(-1))) * 8
        assert bool((k == k.round()).all()) and float(k.abs().max()) <= 64               # coordinates k / 8, |k| <= 64
        # exact ties between candidates need two candidates: every lattice case with M > 1 has them (every target has a duplicate)
        print(S.case_id(case), "points whose best two candidates tie exactly:", ties)
        assert ties > 0 or M == 1, ties
        ref = S.reference(case, "truncated")
        tau2 = S.TAU[family] ** 2
        if N > 256 * S.Q and M > 1:                       # the big lattice cases hold every kind of term of a truncated sum
            d2 = ref["dist2_ab"][0, :la[0]]
            assert bool((d2 == tau2).any()) and bool((d2 > tau2).any()) and bool((d2 < tau2).any()) and bool((d2 == 0).any())
    else:
        # no point's two best candidates are within 4 BOUND of each other: the device's index is the restatement's, and the
        # gradients can be compared although no index is
        assert near_ties == 0 and float(i["a"].abs().max()) <= 1 and float(i["b"].abs().max()) <= 1


def test_the_rounding_bound_is_what_the_scenes_file_derives():
    u = S.U
    assert u == 2.0 ** -24 and (1 + u) ** 5 - 1 <= S.PAIR_ERROR == 6 * u
    assert (1 + S.PAIR_ERROR) / (1 - S.PAIR_ERROR) - 1 <= S.BOUND == 13 * u
    # the f32 difference form on a random case, formed as the kernel forms it, stays within PAIR_ERROR of float64
    i = S.case_inputs(next(c for c in S.CASES if c[0] == "random" and c[1] == "above"))
    p, q = i["a"][0], i["b"][0]
    d = p[:, None, :] - q[None, :, :]
    low = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    exact = S.pair_distances(p, q)
    assert float(((low.double() - exact).abs() / exact).max()) <= S.PAIR_ERROR


def test_float32_yardsticks_are_the_recorded_ones():
    """Measured here again: within a factor 2 of the recorded figures either way (the lattice cases' sums are exact up to the
    means' divisions: whatever is recorded as 0 must measure 0).  The device tolerance of a kind is 8 x the largest recorded
    one."""
    assert set(S.YARDSTICK) == {S.case_id(c) for c in S.CASES}
    for case in S.CASES:
        measured, recorded = S.measure_yardstick(case), S.YARDSTICK[S.case_id(case)]
        for kind, value in measured.items():
            print(S.case_id(case), kind, "float32 yardstick:", "%.2e" % value, "recorded:", recorded[kind])
            assert recorded[kind] / 2 <= value <= recorded[kind] * 2, (S.case_id(case), kind, value)
    for kind in S.KINDS:
        assert S.DEVICE_TOLERANCE[kind] == 8 * max(y[kind] for y in S.YARDSTICK.values()) > 0


def test_the_restatements_fits():
    """The factors the device's end-to-end fits are held to, measured again: within 10 % of the recorded ones."""
    for mesh, recorded in ((False, S.RESTATEMENT_FIT_FACTOR), (True, S.RESTATEMENT_MESH_FIT_FACTOR)):
        factor = S.restatement_fit(mesh)
        print("mesh" if mesh else "points", "the restatement's fit brings the data term down by a factor of %.2f" % factor,
              "recorded: %.2f" % recorded)
        assert recorded > 4 and abs(factor - recorded) <= 0.1 * recorded
    vertices, faces = S.subdivided_octahedron()
    assert vertices.shape == (66, 3) and faces.shape == (128, 3)
    edges = torch.cat((faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]])).long().sort(1).values
    assert bool((torch.unique(edges, dim=0, return_counts=True)[1] == 2).all())           # closed: every edge has two faces


# ---- 4. argument checks -----------------------------------------------------------------------------------------------------------------
def test_argument_errors_are_raised_before_the_device():
    from deep3dmap_amd import neural_renderer as nr
    for name in ("nearest_points", "chamfer_distance", "ChamferTarget"):
        assert getattr(nr, name) is getattr(PS, name)
    a, b = torch.rand(2, 5, 3), torch.rand(2, 7, 3)
    calls = {"nearest_points": lambda x, y, **kw: nr.nearest_points(x, y, **kw),
             "chamfer_distance": lambda x, y, **kw: nr.chamfer_distance(x, y, **kw)}
    for name, call in calls.items():
        first = "points" if name == "nearest_points" else "a"
        for bad in (a.numpy(), torch.rand(5), torch.rand(1, 2, 5, 3), torch.rand(2, 5, 2), a.double(), a.long(),
                    torch.rand(2, 0, 3), torch.rand(0, 3)):
            with pytest.raises(ValueError, match=name):
                call(bad, b)
            with pytest.raises(ValueError, match=name):
                call(a, bad)
        with pytest.raises(ValueError, match="both"):
            call(a[0], b)                                                     # ranks differ
        with pytest.raises(ValueError, match="batch sizes"):
            call(a, torch.rand(3, 7, 3))
        with pytest.raises(ValueError, match="one device"):
            call(a, b.to("meta"))
        with pytest.raises(ValueError, match="65535"):
            call(torch.empty(65536, 1, 3, device="meta"), torch.empty(65536, 1, 3, device="meta"))
        with pytest.raises(ValueError, match="2\\^30"):
            call(torch.empty(1, (1 << 30) + 1, 3, device="meta"), torch.empty(1, 1, 3, device="meta"))
        with pytest.raises(ValueError, match="_splits"):
            call(a, b, _splits=-1)
        lengths = "lengths" if name == "nearest_points" else "a_lengths"
        targets = "target_lengths" if name == "nearest_points" else "b_lengths"
        for key in (lengths, targets):
            for bad in ([5, 5], torch.tensor([5.0, 5.0]), torch.tensor([5]), torch.tensor([[5, 5]]),
                        torch.tensor([5, 5]).to("meta")):
                with pytest.raises(ValueError, match=key):
                    call(a, b, **{key: bad})
        # well-formed arguments on the host end at the device check, behind every other check
        for ok in (lambda: call(a, b), lambda: call(a[0], b[0]),
                   lambda: call(a, b, **{lengths: torch.tensor([5, 0]), targets: torch.tensor([7, 1], dtype=torch.int32)})):
            with pytest.raises(ValueError, match="GPU"):
                ok()
    nan, inf = float("nan"), float("inf")
    for kw in (dict(weight_ab=-1.0), dict(weight_ba=-0.5), dict(weight_ab=nan), dict(weight_ba=inf)):
        with pytest.raises(ValueError, match="weight_ab and weight_ba must be >= 0"):
            nr.chamfer_distance(a, b, **kw)
        with pytest.raises(ValueError, match="weight_ab and weight_ba must be >= 0"):
            nr.ChamferTarget(b, **kw)
    with pytest.raises(ValueError, match="must be > 0"):
        nr.chamfer_distance(a, b, weight_ab=0.0, weight_ba=0.0)
    for tau in (-0.5, nan, inf):
        with pytest.raises(ValueError, match="truncate"):
            nr.chamfer_distance(a, b, truncate=tau)
        with pytest.raises(ValueError, match="truncate"):
            nr.ChamferTarget(b, truncate=tau)
    for bad in (torch.rand(5), torch.rand(7, 2), torch.rand(0, 3)):
        with pytest.raises(ValueError, match="target_points"):
            nr.ChamferTarget(bad)
    module = nr.ChamferTarget(b[0].numpy(), torch.tensor([4]), squared=False, truncate=0.0, weight_ba=0.0)
    assert module.target_points.dtype == torch.float32 and module.target_lengths.dtype == torch.int32
    assert module.options == dict(squared=False, truncate=0.0, weight_ab=1.0, weight_ba=0.0)
    for x in (a[0], a):
        with pytest.raises(ValueError, match="GPU"):
            module(x)


# ---- 5. the C entry points refuse bad arguments before any launch ---------------------------------------------------------------
def test_entry_points_return_invalid_before_any_launch():
    from deep3dmap_amd import _lib
    L = _lib.lib()
    p, misaligned, by4 = ctypes.c_void_p(256), ctypes.c_void_p(258), ctypes.c_void_p(260)        # never dereferenced
    INVALID = 1
    B, N, M = 3, 1025, 513
    query = L.d3m_chamfer_distance_scratch_bytes
    forward = B * N * 8 + B * M * 8 + B * 2 * 4 + B * 1 * 4              # the keys; the value's parts: 2 and 1 per set
    backward = (B * N + B * M) * 3 * 8 + 1024 * 4                       # the accumulators; the block maxima
    assert query(B, N, M) == max(forward, backward) == backward and query(1, 1, 1) == 48 + 4096
    assert query(0, N, M) == 0 == query(65536, N, M) == query(B, 0, M) == query(B, N, 0) == query(B, (1 << 30) + 1, M)
    assert query(1, 1 << 30, 1 << 30) == 2 * 3 * 8 * (1 << 30) + 4096

    def run(fn, ok, changes):
        assert set().union(*changes) <= set(ok)
        for change in changes:
            assert fn(*dict(ok, **change).values(), None) == INVALID, (fn.__name__, change)

    nan, inf = float("nan"), float("inf")
    sizes = [dict(B=0), dict(B=65536), dict(N=0), dict(M=0), dict(N=(1 << 30) + 1), dict(M=(1 << 30) + 1), dict(N=-1)]
    common = sizes + [dict(a=None), dict(b=None), dict(a=misaligned), dict(b=misaligned), dict(la=misaligned), dict(lb=misaligned),
                      dict(scratch=None), dict(scratch=misaligned), dict(scratch=by4)]
    sets = dict(a=p, b=p, B=B, N=N, M=M, la=p, lb=None)
    nearest = dict(sets, splits=0, scratch=p, scratch_bytes=1 << 40, index=p, dist2=p)
    run(L.d3m_nearest_points, nearest,
        common + [dict(splits=-1), dict(index=None), dict(dist2=None), dict(index=misaligned), dict(dist2=misaligned)])
    fwd = dict(sets, squared=1, truncate=-1.0, weight_ab=1.0, weight_ba=1.0, splits=0, scratch=p, scratch_bytes=1 << 40,
               index_ab=p, dist2_ab=p, index_ba=p, dist2_ba=p, coef=p, value=p)
    run(L.d3m_chamfer_distance, fwd,
        common + [dict(splits=-1), dict(truncate=nan), dict(truncate=inf), dict(weight_ab=-1.0), dict(weight_ba=-0.5),
                  dict(weight_ab=nan), dict(weight_ba=inf), dict(weight_ab=0.0, weight_ba=0.0), dict(index_ab=None),
                  dict(dist2_ab=None), dict(index_ba=None), dict(dist2_ba=None), dict(coef=None), dict(value=None),
                  dict(index_ab=misaligned), dict(dist2_ba=misaligned), dict(coef=misaligned), dict(value=misaligned)])
    bwd = dict(sets, index_ab=p, dist2_ab=p, index_ba=p, dist2_ba=p, coef=p, upstream=p, per_query=0, squared=1, truncate=-1.0,
               scratch=p, scratch_bytes=1 << 40, grad_a=p, grad_b=p)
    run(L.d3m_chamfer_distance_backward, bwd,
        common + [dict(truncate=nan), dict(upstream=None), dict(grad_a=None), dict(grad_b=None), dict(index_ab=None, index_ba=None),
                  dict(dist2_ab=None), dict(dist2_ba=None), dict(coef=None), dict(per_query=1), dict(per_query=1, coef=None),
                  dict(per_query=1, coef=None, index_ba=None, index_ab=None), dict(index_ab=misaligned), dict(dist2_ba=misaligned),
                  dict(coef=misaligned), dict(upstream=misaligned), dict(grad_a=misaligned), dict(grad_b=misaligned)])
    need = query(B, N, M)
    for fn, ok in ((L.d3m_nearest_points, nearest), (L.d3m_chamfer_distance, fwd), (L.d3m_chamfer_distance_backward, bwd)):
        rc = fn(*dict(ok, scratch_bytes=need - 1).values(), None)
        assert L.d3m_error_string(rc) == b"workspace missing or too small"
