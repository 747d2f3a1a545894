"""Nearest points and chamfer distances between point sets (neural_renderer/point_sets.py, csrc/d3m_point_sets.h): the cases,
the options, the seeded inputs, a brute-force restatement in float64 (the reference) and float32 (the yardstick) and the
recorded float32 yardsticks.

THE FUNCTION, restated from the module text.  Per batch element with n points of a and m points of b (the lengths):
    nn(i)  = the lowest j < m that minimises d2(i, j) = |a_i - b_j|^2 formed from the coordinate differences
    L_ab   = (1/n) sum_{i<n} rho(d2(i, nn(i))),  rho(d2) = d2 (squared) or sqrt(d2); truncate = tau: a term with d2 > tau^2
             contributes rho(tau^2) and has no gradient (tau^2 as the f32 product, as the kernel forms it)
    value  = weight_ab L_ab + weight_ba L_ba, L_ba with the roles swapped; an empty query or target set contributes 0
The gradient is autograd's of these operators with nn held constant (sqrt'(0) taken as 0), of sum_b value[b] upstream[b].

THE ROUNDING BOUND of the random family, u = 2^-24.  The kernel forms dx = fl(a.x - b.x) and so on, each with relative error
<= u, then fma(dz, dz, fma(dy, dy, fl(dx dx))): three more roundings.  Every term is >= 0, so relative errors do not amplify:
the computed d2 is within (1 + u)^2 (1 + u)^3 - 1 <= PAIR_ERROR = 6 u of the exact one (5 u / (1 - 5 u) < 6 u; the same holds
without the fused forms, which round five times too).  The f32 minimum is therefore within 6 u of the float64 minimum D*, and
the float64 distance D_j to the returned index j obeys D_j (1 - 6 u) <= d2_j <= D* (1 + 6 u), so D_j <= D* (1 + 6 u) / (1 - 6 u)
<= D* (1 + 13 u).  BOUND = 13 u covers both checks.  (Coordinates in [-1, 1] as seeded here: no square underflows.)

YARDSTICKS.  Per case and kind the largest |float32 restatement - float64 restatement| over the options, in units of the float64
result's largest entry, the float32 restatement taking the float64 one's nn; recorded below and measured again by
tests/test_point_sets_host.py within a factor 2.  DEVICE_TOLERANCE of a kind is 8 x the largest recorded yardstick of that
kind, the margin of tests/test_gpu_uv_texture_regularizers.py: the kernel associates its sums differently from the float32
restatement, and a single-seed yardstick moves by small factors."""
import numpy as np
import torch

from deep3dmap_amd.neural_renderer import point_sets as PS

T, Q = PS.TILE, PS.QUERIES_PER_LANE
U = 2.0 ** -24
PAIR_ERROR = 6 * U
BOUND = 13 * U
KINDS = ("value", "grad_a", "grad_b")
FAMILIES = ("lattice", "random")
SPLITS = (1, 2, 5)              # 2 does not divide the 3 tiles of M = 2 T + 3; 5 exceeds them

# (name, B, N, M): every N of {1, 63, 64, 65, 256 Q + 1} and every M of {1, T - 1, T, T + 1, 2 T + 3}
SHAPES = (
    ("one", 1, 1, 1),
    ("below", 1, 63, T - 1),
    ("wave", 1, 64, T),
    ("above", 1, 65, T + 1),
    ("blocks", 1, 256 * Q + 1, 2 * T + 3),          # two query blocks against three tiles
    ("few_many", 1, 1, 2 * T + 3),
    ("many_one", 1, 256 * Q + 1, 1),
    ("ragged", 3, 65, 2 * T + 3),                   # ragged lengths, a set of length 1
    ("empty", 3, 256 * Q + 1, T + 1),               # ragged lengths, a set of length 1, an empty target set
)
CASES = tuple((family,) + shape for family in FAMILIES for shape in SHAPES)
TAU = {"lattice": 1.0, "random": 0.125}             # lattice: d2 == tau^2 occurs (not truncated) beside larger and smaller ones

OPTIONS = {
    "squared": dict(),
    "distance": dict(squared=False),
    "truncated": dict(truncate=True),
    "truncated_distance": dict(squared=False, truncate=True),
    "ab_only": dict(weight_ba=0.0),
    "ba_only": dict(weight_ab=0.0, weight_ba=0.7, squared=False),
    "weighted": dict(weight_ab=0.7, weight_ba=1.3),
}


def case_id(case):
    return "%s-%s-B%d-N%d-M%d" % case


def options_of(case, option):
    """the keyword arguments of chamfer_distance for OPTIONS[option] on a case (truncate=True -> the family's tau)"""
    kw = dict(OPTIONS[option])
    if kw.get("truncate"):
        kw["truncate"] = TAU[case[0]]
    return kw


# measured by measure_yardstick (tests/test_point_sets_host.py prints them again)
YARDSTICK = {
    "lattice-one-B1-N1-M1": dict(value=3.6e-08, grad_a=6.3e-08, grad_b=6.3e-08),
    "lattice-below-B1-N63-M511": dict(value=9.8e-08, grad_a=1.1e-07, grad_b=1.1e-07),
    "lattice-wave-B1-N64-M512": dict(value=6.8e-08, grad_a=2.0e-07, grad_b=1.1e-07),
    "lattice-above-B1-N65-M513": dict(value=6.0e-08, grad_a=2.4e-07, grad_b=1.0e-07),
    "lattice-blocks-B1-N1025-M1027": dict(value=9.6e-08, grad_a=1.2e-07, grad_b=2.0e-07),
    "lattice-few_many-B1-N1-M1027": dict(value=8.9e-08, grad_a=1.1e-06, grad_b=9.3e-08),
    "lattice-many_one-B1-N1025-M1": dict(value=1.4e-07, grad_a=6.5e-08, grad_b=4.0e-06),
    "lattice-ragged-B3-N65-M1027": dict(value=1.3e-07, grad_a=1.3e-06, grad_b=8.6e-08),
    "lattice-empty-B3-N1025-M513": dict(value=5.1e-08, grad_a=4.2e-07, grad_b=2.0e-07),
    "random-one-B1-N1-M1": dict(value=4.8e-08, grad_a=3.2e-08, grad_b=3.2e-08),
    "random-below-B1-N63-M511": dict(value=1.6e-07, grad_a=1.5e-07, grad_b=2.0e-07),
    "random-wave-B1-N64-M512": dict(value=1.1e-07, grad_a=1.3e-07, grad_b=1.2e-07),
    "random-above-B1-N65-M513": dict(value=9.9e-08, grad_a=1.7e-07, grad_b=1.4e-07),
    "random-blocks-B1-N1025-M1027": dict(value=6.6e-08, grad_a=1.1e-07, grad_b=1.2e-07),
    "random-few_many-B1-N1-M1027": dict(value=4.5e-08, grad_a=6.2e-07, grad_b=1.2e-07),
    "random-many_one-B1-N1025-M1": dict(value=9.9e-08, grad_a=7.9e-08, grad_b=7.9e-07),
    "random-ragged-B3-N65-M1027": dict(value=1.1e-07, grad_a=9.3e-07, grad_b=1.3e-07),
    "random-empty-B3-N1025-M513": dict(value=6.4e-08, grad_a=4.1e-07, grad_b=1.3e-07),
}
DEVICE_TOLERANCE = {k: 8 * max(y[k] for y in YARDSTICK.values()) for k in KINDS}


# ---- the cases' inputs --------------------------------------------------------------------------------------------------------
UPSTREAM = {1: (0.7,), 3: (-1.3, 0.7, 0.5)}
EMPTY_TARGET_ELEMENT = 2                            # of the `empty` shape
_inputs = {}


def _lattice(gen, B, N, M):
    """Coordinates k / 8, |k| <= 64: every difference, square and sum is exact in f32 (and in f64) under any contraction.
    Targets: integers in [-6, 6]; the second quarter mirrors the first in x, the second half repeats the first half (an odd
    one out repeats target 0): every target has an exact duplicate.  Queries: multiples of 1/2 in [-8, 8], every third one
    on the mirror plane x = 0: equidistant from distinct targets, too."""
    h = max(M // 2, 1)
    b = torch.randint(-6, 7, (B, M, 3), generator=gen).float()
    if h >= 2:
        b[:, h // 2:2 * (h // 2)] = b[:, :h // 2] * torch.tensor([-1.0, 1.0, 1.0])
    if M > 1:
        b[:, h:2 * h] = b[:, :h]
        b[:, 2 * h:] = b[:, :1]
    a = torch.randint(-16, 17, (B, N, 3), generator=gen).float() / 2
    a[:, ::3, 0] = 0.0
    return a, b


def case_inputs(case):
    """dict(a [B,N,3], b [B,M,3], a_lengths, b_lengths (int32 [B] or None), upstream [B]) in float32, seeded, computed once"""
    if case not in _inputs:
        family, name, B, N, M = case
        gen = torch.Generator().manual_seed(7 + 1000 * N + 10 * M + B + (500 if family == "random" else 0))
        if family == "lattice":
            a, b = _lattice(gen, B, N, M)
        else:
            a, b = torch.rand(B, N, 3, generator=gen) * 2 - 1, torch.rand(B, M, 3, generator=gen) * 2 - 1
        la = lb = None
        if B == 3:
            la = torch.tensor([N, 1, N // 2 + 1], dtype=torch.int32)
            lb = torch.tensor([M, M // 2 + 3, 0] if name == "empty" else [M - 5, M, 1], dtype=torch.int32)
        _inputs[case] = dict(a=a, b=b, a_lengths=la, b_lengths=lb, upstream=torch.tensor(UPSTREAM[B]))
    return _inputs[case]


def lengths_of(inputs):
    B, N, M = inputs["a"].shape[0], inputs["a"].shape[1], inputs["b"].shape[1]
    la = [N] * B if inputs["a_lengths"] is None else [int(v) for v in inputs["a_lengths"]]
    lb = [M] * B if inputs["b_lengths"] is None else [int(v) for v in inputs["b_lengths"]]
    return la, lb


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def pair_distances(p, q):
    """[n, m] squared distances of p [n,3] and q [m,3] in float64, from the coordinate differences"""
    d = p.double()[:, None, :] - q.double()[None, :, :]
    return (d * d).sum(-1)


def nearest(p, q):
    """(index [n] int64, d2 [n] float64) of every point of p in q: the lowest index among equal distances (numpy's argmin
    returns the first occurrence); a row of NaN only: -1 and NaN"""
    D = pair_distances(p, q).numpy()
    safe = np.where(np.isnan(D), np.inf, D)
    index = safe.argmin(1)
    d2 = D[np.arange(D.shape[0]), index]
    none = np.isnan(D).all(1)
    return torch.from_numpy(np.where(none, -1, index)), torch.from_numpy(np.where(none, np.nan, d2))


def nearest_points(a, b, la, lb):
    """(index [B,N] int32, dist2 [B,N] float64) as the node defines them: -1 and 0 beyond a set's length and without targets"""
    B, N = a.shape[:2]
    index, dist2 = torch.full((B, N), -1, dtype=torch.int32), torch.zeros(B, N, dtype=torch.float64)
    for e in range(B):
        n, m = la[e], lb[e]
        if n > 0 and m > 0:
            j, d2 = nearest(a[e, :n], b[e, :m])
            index[e, :n], dist2[e, :n] = j.to(torch.int32), d2
    return index, dist2


def rho(d2, squared, tau):
    """rho of d2 (a tensor of any float dtype); tau None or the truncation distance"""
    if tau is not None:
        tau2 = float(np.float32(tau) * np.float32(tau))
        d2 = torch.where(d2 > tau2, torch.full_like(d2, tau2), d2)
    if squared:
        return d2
    positive = d2 > 0
    return torch.where(positive, torch.sqrt(torch.where(positive, d2, torch.ones_like(d2))), torch.zeros_like(d2))


def direction_mean(p, q, index, squared, tau, direct_only=False):
    """L of one direction of one element: p [n,3] against q [m,3] with nn = index [n] (long); 0 for an empty set.
    direct_only: the targets are constants, so that the gradient is the queries' direct terms alone"""
    if p.shape[0] == 0 or q.shape[0] == 0:
        return p.sum() * 0
    d = p - (q.detach() if direct_only else q)[index]
    return rho((d * d).sum(-1), squared, tau).mean()


def value_of(a, b, la, lb, index_ab, index_ba, squared=True, truncate=None, weight_ab=1.0, weight_ba=1.0, direct_only=False):
    """value [B] in a's dtype; index_ab [B,N], index_ba [B,M]: the nn (held constant)"""
    values = []
    for e in range(a.shape[0]):
        n, m = la[e], lb[e]
        p, q = a[e, :n], b[e, :m]
        v = p.sum() * 0
        if weight_ab > 0:
            v = v + weight_ab * direction_mean(p, q, index_ab[e, :n].long(), squared, truncate, direct_only)
        if weight_ba > 0:
            v = v + weight_ba * direction_mean(q, p, index_ba[e, :m].long(), squared, truncate, direct_only)
        values.append(v)
    return torch.stack(values)


def evaluate(inputs, kw, dtype=torch.float64, index=None):
    """dict(value [B], grad_a, grad_b, gmax, index_ab, dist2_ab, index_ba, dist2_ba) of the restatement in `dtype`; the gradient
    is that of sum(value upstream); gmax: the largest |direct term| of the call.  index: (index_ab, index_ba) to hold constant
    instead of the restatement's own."""
    la, lb = lengths_of(inputs)
    ab = nearest_points(inputs["a"], inputs["b"], la, lb)
    ba = nearest_points(inputs["b"], inputs["a"], lb, la)
    index_ab, index_ba = (ab[0], ba[0]) if index is None else index
    a = inputs["a"].to(dtype).clone().requires_grad_(True)
    b = inputs["b"].to(dtype).clone().requires_grad_(True)
    value = value_of(a, b, la, lb, index_ab, index_ba, **kw)
    grad_a, grad_b = torch.autograd.grad((value * inputs["upstream"].to(dtype)).sum(), (a, b), allow_unused=True)
    zero = lambda g, t: torch.zeros_like(t) if g is None else g
    direct = value_of(a, b, la, lb, index_ab, index_ba, direct_only=True, **kw)
    direct = torch.autograd.grad((direct * inputs["upstream"].to(dtype)).sum(), (a, b), allow_unused=True)
    gmax = max(float(zero(g, t).abs().max()) for g, t in zip(direct, (a, b)))
    return dict(value=value.detach(), grad_a=zero(grad_a, a), grad_b=zero(grad_b, b), gmax=gmax, index_ab=ab[0], dist2_ab=ab[1],
                index_ba=ba[0], dist2_ba=ba[1])


_references = {}


def reference(case, option):
    """the float64 restatement of a case under OPTIONS[option], computed once and shared"""
    if (case, option) not in _references:
        _references[(case, option)] = evaluate(case_inputs(case), options_of(case, option))
    return _references[(case, option)]


def relative_error(result, ref):
    """max |result - ref| in units of ref's largest entry (of 1 where ref is all zero)"""
    scale = float(ref.abs().max())
    return float((result.detach().cpu().double() - ref.double()).abs().max()) / (scale if scale > 0 else 1.0)


def measure_yardstick(case):
    inputs = case_inputs(case)
    worst = dict.fromkeys(KINDS, 0.0)
    for option in OPTIONS:
        ref = reference(case, option)
        low = evaluate(inputs, options_of(case, option), torch.float32, (ref["index_ab"], ref["index_ba"]))
        for k in KINDS:
            worst[k] = max(worst[k], relative_error(low[k], ref[k]))
    return worst


# ---- what the scattered gradient may add: the quantum bound ----------------------------------------------------------------------
def sources(index, count):
    """[B, count] how many points name each target as their nearest neighbour; index [B,n] with -1 for none"""
    out = torch.zeros(index.shape[0], count, dtype=torch.int64)
    for e in range(index.shape[0]):
        j = index[e][index[e] >= 0].long()
        out[e] = torch.bincount(j, minlength=count)
    return out


def quantum(ref, inputs):
    """2^(E - frac) of a call whose restatement is ref: E = ilogb(gmax) + 1 and frac = 62 - ceil(log2(max(N, M))); 0 for
    gmax == 0"""
    N, M = inputs["a"].shape[1], inputs["b"].shape[1]
    if ref["gmax"] == 0:
        return 0.0
    E = int(np.floor(np.log2(ref["gmax"]))) + 1
    frac = 62 - int(np.ceil(np.log2(max(N, M))))
    return 2.0 ** (E - frac)


def relative_gaps(p, q):
    """(second-best d2 - best d2) / best d2 of every point of p in q [m >= 2], float64: how far the nn is from a tie"""
    D = pair_distances(p, q).sort(1).values
    return (D[:, 1] - D[:, 0]) / D[:, 0]


# ---- the end-to-end fits ------------------------------------------------------------------------------------------------------------
FIT_STEPS, FIT_RATE, FIT_LAPLACIAN = 60, 0.05, 0.05
# the factors by which restatement_fit brings the data term down (tests/test_point_sets_host.py measures them again); the device
# tests ask for half of them
RESTATEMENT_FIT_FACTOR = 98.3
RESTATEMENT_MESH_FIT_FACTOR = 42.4


def sphere_points(n, seed):
    p = torch.randn(n, 3, generator=torch.Generator().manual_seed(seed))
    return p / p.norm(dim=1, keepdim=True)


def fit_points():
    """(200 points in a small ball off the centre, 300 points of the unit sphere), float32"""
    return sphere_points(200, 2) * 0.3 + torch.tensor([0.2, 0.0, -0.1]), sphere_points(300, 1)


def subdivided_octahedron(levels=2):
    """(vertices [V,3] on the unit sphere, faces [F,3] int32) of a closed mesh: V = 66, F = 128 at two levels"""
    v = [(1., 0., 0.), (-1., 0., 0.), (0., 1., 0.), (0., -1., 0.), (0., 0., 1.), (0., 0., -1.)]
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    for _ in range(levels):
        mid, out = {}, []

        def middle(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                m = np.add(v[i], v[j]) / 2
                v.append(tuple(m / np.linalg.norm(m)))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            out += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        f = out
    return torch.tensor(v, dtype=torch.float32), torch.tensor(f, dtype=torch.int32)


def fit_mesh():
    """(the subdivided octahedron's vertices shrunk to 0.3, its faces, 300 points of the unit sphere)"""
    vertices, faces = subdivided_octahedron()
    return vertices * 0.3, faces, sphere_points(300, 1)


def adam_fit(start, data, prior=None):
    """FIT_STEPS Adam steps on a copy of `start` of data(x) (+ prior(x)): (the data term at the first step, at the last)"""
    x = start.clone().requires_grad_(True)
    opt = torch.optim.Adam([x], lr=FIT_RATE)
    first = last = None
    for _ in range(FIT_STEPS):
        opt.zero_grad()
        term = data(x)
        (term if prior is None else term + prior(x)).backward()
        opt.step()
        first, last = (float(term.detach()) if first is None else first), float(term.detach())
    return first, last


def restated_chamfer(x, target):
    """the squared chamfer distance of x [N,3] and target [M,3] in x's dtype, both directions, the nn found anew"""
    ab, ba = nearest(x.detach(), target)[0], nearest(target, x.detach())[0]
    return direction_mean(x, target, ab, True, None) + direction_mean(target, x, ba, True, None)


def restated_laplacian(x, faces):
    """the mean squared distance of a vertex from the mean of its neighbours (mesh_regularizer's L_lap)"""
    V = x.shape[0]
    f = faces.long()
    adjacency = torch.zeros(V, V, dtype=x.dtype)
    for i, j in ((0, 1), (1, 2), (2, 0)):
        adjacency[f[:, i], f[:, j]] = 1
        adjacency[f[:, j], f[:, i]] = 1
    mean = adjacency @ x / adjacency.sum(1, keepdim=True)
    return ((x - mean) ** 2).sum(-1).mean()


def restatement_fit(mesh):
    """the fit of the device tests with the restatement in float64 on the CPU: the factor first / last of the data term"""
    if mesh:
        vertices, faces, target = fit_mesh()
        first, last = adam_fit(vertices.double(), lambda x: restated_chamfer(x, target.double()),
                               lambda x: FIT_LAPLACIAN * restated_laplacian(x, faces))
    else:
        start, target = fit_points()
        first, last = adam_fit(start.double(), lambda x: restated_chamfer(x, target.double()))
    return first / last
