"""The fixed-order parameter reductions (csrc/d3m_camera_grad.h, csrc/d3m_light_grad.h) beyond one workgroup, host side:
the float64 references of both, in the per-term form that gives every (view, vertex) or (view, face) contribution to every
parameter entry, the inputs of every case of tests/test_gpu_param_reductions.py and the proof that they are sharp (no 256-
element chunk of a view can go missing inside the tolerance), and the workspace size arithmetic through the library.  No GPU.

The tolerance of an entry is (D 2^-24 + 4 E32) * bound:
  bound  sum of |term| over everything that is added into the entry (float64);
  D      the longest chain of additions an entry goes through, from the kernels' constants (chain_length);
  E32    the per-term rounding share, max |ref32 - ref| / bound over the parameter's entries, ref32 being this file's
         reference evaluated in float32 (torch sums pairwise, so what is left is the arithmetic of the terms); the factor 4
         because the kernels associate a term differently (camera_point_grad_cam's order, the sums the finish kernel forms).
Nothing in it comes from the kernels' output.

Sharpness is proven for the chunks of the last view of a case (the issue's "of one view"); the upstream gradient gives that
view most of the weight so that this holds for parameters that are summed over the views too.  A chunk lost in another view
of such a parameter can hide inside the tolerance at the largest sizes; those views are covered by the cases whose
parameters are per view."""
import collections
import itertools
import math
import os
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_camera_params import _oracle_camera

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_CAMERA = os.path.join(ROOT, "tests", "golden", "camera_golden.npz")
GOLDEN_LIGHT = os.path.join(ROOT, "tests", "golden", "light_golden.npz")

# ---- the kernels' constants (d3m_camera_grad.h, d3m_light_grad.h) ------------------------------------------------------------
PER_PART, MAX_PARTS, LANES = 1024, 128, 256
CAM_SUMS, CAM_ROW, LIGHT_SUMS, LIGHT_ROW = 23, 23, 9, 11
EPS32 = 2.0 ** -24
ANGLE, ORIG_SIZE = 30.0, 256.0

CAMERA_SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 50625, 131072, 131073, 300001)
LIGHT_SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 200704, 131072, 131073, 300001)
VIEWS = (1, 3, 32)
LONG_VIEWS, LONG_SIZES = 300, (5, 1025)          # the finish kernels' b += 256 / e += 256 loops
KINDS = ("look_at", "look", "projection")
CAMERA_NAMES = {"look_at": ("eye", "at", "up"), "look": ("eye", "direction", "up"), "projection": ("K", "R", "t", "dist")}
LIGHT_NAMES = ("intensity_ambient", "intensity_directional", "color_ambient", "color_directional", "direction")
ROWS_PER_GROUP = 1 << 19        # (view, element) pairs differentiated at a time


def parts_of(n):
    """camera_parts / light_parts: 1024 elements per workgroup, at most 128 workgroups"""
    return min(max(-(-n // PER_PART), 1), MAX_PARTS)


def chain_length(n, views, summed):
    """The longest chain of additions behind one entry: a lane's elements (stride parts*256), the wave's 6 butterfly steps,
    the 3 additions of the 4 waves, the finish kernel's `parts` partials -- and the views of a parameter of batch 1."""
    parts = parts_of(n)
    return -(-n // (parts * LANES)) + 6 + 3 + parts + (views if summed else 0)


def onehot_indices(n):
    parts = parts_of(n)
    return sorted({i for i in (0, 63, 64, 255, 256, parts * LANES - 1, parts * LANES, n - 257, n - 1) if 0 <= i < n})


# ---- cases -------------------------------------------------------------------------------------------------------------------
CameraCase = collections.namedtuple("CameraCase", "kind n views shared_params shared_vertices")
LightCase = collections.namedtuple("LightCase", "n views fill_back grid shared_params shared_vertices")


def _sizes_and_views(sizes):
    return [(n, b) for n in sizes for b in VIEWS] + [(n, LONG_VIEWS) for n in LONG_SIZES]


# (shared_params, shared_vertices): the cases of a kernel take them in turn
BATCH_SHAPES = ((False, False), (True, False), (False, True), (True, True))


def camera_cases():
    """Every size with 1, 3 and 32 views in every mode, the four combinations of the parameters' and the vertices' batch
    shapes taken in turn by each mode; 300 views at 5 and 1025 vertices in every mode with the parameters in BOTH shapes (the finish
    kernel's second trip through b += 256 feeds both the per-view rows and the sum over the views)."""
    cases, turns = [], {kind: itertools.cycle(BATCH_SHAPES) for kind in KINDS}        # (each mode takes its own turns)
    for n, b in _sizes_and_views(CAMERA_SIZES):
        for kind in KINDS:
            shapes = turns[kind]
            if b == LONG_VIEWS:
                sv = next(shapes)[1]
                cases += [CameraCase(kind, n, b, False, sv), CameraCase(kind, n, b, True, not sv)]
            else:
                cases.append(CameraCase(kind, n, b, *next(shapes)))
    return cases


def _grid_of(cells):
    """(H, W) of the grid mesh with `cells` cells (2 triangles each) that is nearest to a square"""
    h = next(h for h in range(math.isqrt(cells), 0, -1) if cells % h == 0)
    return (h + 1, cells // h + 1)


def light_variants(n):
    """(fill_back, grid) of F' = n faces: explicit indices without fill_back always; with fill_back where n is even; the
    implicit grid (tri == NULL, tri_batch = -W) where n (or n/2 with fill_back) is twice a number of cells"""
    out = [(0, None)]
    if n % 2 == 0:
        out.append((1, None))
        out.append((0, _grid_of(n // 2)))
        if n % 4 == 0:
            out.append((1, _grid_of(n // 4)))
    return out


def light_cases():
    """Every size with 1, 3 and 32 views in every variant light_variants allows, the four combinations of the batch shapes
    taken in turn by each variant; 300 views
    at 5 and 1025 faces with the parameters in BOTH shapes, as camera_cases."""
    cases, turns = [], collections.defaultdict(lambda: itertools.cycle(BATCH_SHAPES))   # (each variant takes its own turns)
    for n, b in _sizes_and_views(LIGHT_SIZES):
        for fill_back, grid in light_variants(n):
            shapes = turns[fill_back, grid is None]
            if b == LONG_VIEWS:
                sv = next(shapes)[1]
                cases += [LightCase(n, b, fill_back, grid, False, sv), LightCase(n, b, fill_back, grid, True, not sv)]
            else:
                cases.append(LightCase(n, b, fill_back, grid, *next(shapes)))
    return cases


def case_id(c):
    short = {"n": "n", "views": "b", "fill_back": "fb", "grid": "grid", "shared_params": "sp", "shared_vertices": "sv"}
    parts = []
    for f, v in zip(c._fields, c):
        if f == "kind":
            parts.append(v)
        elif f == "grid":
            parts.append("indexed" if v is None else f"grid{v[0]}x{v[1]}")
        else:
            parts.append(f"{short[f]}{int(v)}")
    return "-".join(parts)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def _generator(c):
    return torch.Generator().manual_seed(zlib.crc32(case_id(c).encode()))


def _wobble(nb, freq, phase):
    """a bounded offset per view (zero for view 0 of a shared parameter only by chance): sin(freq b + phase)"""
    return torch.sin(freq * torch.arange(nb, dtype=torch.float32) + phase)


def _vec(base, nb, scale, phase):
    base = torch.tensor(base, dtype=torch.float32)
    w = torch.stack([_wobble(nb, 1.0 + 0.7 * k, phase + k) for k in range(base.numel())], 1).reshape(nb, *base.shape)
    return (base[None] + scale * w).contiguous()


def upstream_weights(n, views):
    """[views, n, 1]: the last view carries 4*views times the weight of the others and the elements of a last, partial
    256-chunk 256/len times the weight of the rest, so that every chunk of the last view -- the tail's single element
    included -- holds a share of a shared parameter's bound that the tolerance cannot hide (the sharpness test)."""
    w = torch.ones(views, n, 1)
    tail = n % LANES
    if tail:
        w[:, n - tail:] = LANES / tail
    if views > 1:
        w[-1] *= 4 * views
    return w


def sparse_rows(n, views, gen):
    """[views, n] bool: one row in ten kept, in every 256-chunk (the renders leave zero rows for unseen vertices)"""
    keep = torch.zeros(views, n, dtype=torch.bool)
    for lo in range(0, n, LANES):
        m = min(LANES, n - lo)
        k = max(1, round(0.1 * m))
        order = torch.rand(views, m, generator=gen).argsort(1)
        keep[:, lo:lo + m] = order < k
    return keep


def camera_inputs(c):
    """float32 inputs of a camera case: vertices [1 or B,n,3] off the optical axis and in front of the camera, the mode's
    parameters ([1,...] or [B,...]), the dense upstream gradient [B,n,3] (z-heavy, so that the terms of the translation do
    not cancel) and the rows the sparse one keeps."""
    gen = _generator(c)
    B, n = c.views, c.n
    vb, nb = (1 if c.shared_vertices else B), (1 if c.shared_params else B)
    v = torch.rand(vb, n, 3, generator=gen) * torch.tensor([0.8, 0.8, 0.6]) + torch.tensor([0.15, 0.1, -0.3])
    if c.kind == "projection":
        K = _vec([[300., 2., 128.], [0., 310., 120.], [0., 0., 1.]], nb, 1.0, 0.3) * \
            torch.tensor([[1., 1., 1.], [0., 1., 1.], [0., 0., 0.]]) + torch.tensor([[0., 0., 0.], [0., 0., 0.], [0., 0., 1.]])
        ax, ay = 0.05 * _wobble(nb, 1.3, 0.5), 0.05 * _wobble(nb, 0.9, 1.5)
        one, zero = torch.ones(nb), torch.zeros(nb)
        Rx = torch.stack([one, zero, zero, zero, ax.cos(), -ax.sin(), zero, ax.sin(), ax.cos()], 1).reshape(nb, 3, 3)
        Ry = torch.stack([ay.cos(), zero, ay.sin(), zero, one, zero, -ay.sin(), zero, ay.cos()], 1).reshape(nb, 3, 3)
        dist = torch.tensor([0.05, -0.02, 0.001, 0.002, 0.01]) * \
            (1 + 0.2 * torch.stack([_wobble(nb, 1.0 + k, 1.1 * k) for k in range(5)], 1))
        params = [K.contiguous(), (Rx @ Ry).contiguous(), _vec([0.1, -0.2, 3.0], nb, 0.05, 0.7), dist.contiguous()]
    else:
        # A camera in general position, about 2.7 from the vertices, that looks PAST them (they sit 0.1-0.6 rad off the
        # optical axis): no entry of a gradient is small by alignment.  The gradient of `direction` (or `at`) is the part
        # of sum gc (x) (v - eye) perpendicular to the axis and that of `up` is parallel to the frame's x: with the axis or
        # `up` along an axis of the world, or the vertices on the optical axis, an entry is the difference of two sums and
        # its bound a tiny fraction of them -- a property of that pose, not of the reduction.
        if c.kind == "look_at":
            eye, second = _vec([-0.9, 1.2, -2.2], nb, 0.1, 0.0), _vec([1.39, 0.5, -0.55], nb, 0.05, 0.4)
        else:
            eye, second = _vec([-1.51, 1.43, -1.63], nb, 0.1, 0.0), _vec([0.45, -0.35, 0.8], nb, 0.03, 0.4)
        params = [eye, second, _vec([0.3, 0.9, -0.25], nb, 0.05, 0.9)]
    g = (torch.randn(B, n, 3, generator=gen) + torch.tensor([0.0, 0.0, 2.0])) * upstream_weights(n, B)
    return dict(vertices=v.contiguous(), params=params, upstream=g.contiguous(), keep=sparse_rows(n, B, gen))


def grid_triangles(H, W):
    """[2(H-1)(W-1), 3] int32: the implicit topology of tri_ids (d3m_device.h): (tl, bl, tr) of every cell, then (tr, bl, br)"""
    idx = torch.arange(H * W, dtype=torch.int32).reshape(H, W)
    f1 = torch.stack([idx[:-1, :-1], idx[1:, :-1], idx[:-1, 1:]], -1).reshape(-1, 3)
    f2 = torch.stack([idx[:-1, 1:], idx[1:, :-1], idx[1:, 1:]], -1).reshape(-1, 3)
    return torch.cat([f1, f2], 0)


def gather_faces(vertices, tri, fill_back):
    """[vb,V,3], [F,3] -> [vb,F',3,3]: vertices_to_faces, with the back faces as Renderer._fill_back makes them (reversed
    winding, appended)"""
    tri = tri.long()
    if fill_back:
        tri = torch.cat([tri, tri.flip(-1)], 0)
    return vertices[:, tri]


# Every face is well shaped and well off the horizon of every light that reads it: |cross(a, b)| >= LIGHT_MARGIN |a| |b| and
# |n . d| >= LIGHT_MARGIN |d|.  relu(n . d) of a sliver nearly edge-on to the light is a difference of products of the edges'
# size (measured: |a||b| / |cross| = 18 and n . d = 0.05 |d| gave a term of 42 * 2^-24 relative error in float32): the rounding
# of such a term belongs to the face, not to the reduction, and [n . d > 0] has to be the same decision in every precision.
LIGHT_MARGIN = 0.4


def face_conditioning(faces, direction):
    """faces [B,F',3,3], direction [B,3] (float64) -> (|cross| / (|a| |b|), |n . d| / |d|), each [B,F']"""
    a, b = faces[:, :, 0] - faces[:, :, 1], faces[:, :, 2] - faces[:, :, 1]
    cr = torch.cross(a, b, dim=-1)
    cs = (F.normalize(cr, eps=1e-5, dim=-1) * direction[:, None]).sum(-1)
    return cr.norm(dim=-1) / (a.norm(dim=-1) * b.norm(dim=-1)), cs.abs() / direction.norm(dim=-1)[:, None]


def _light_parameters(nb, grid):
    if grid is None:
        direction = _vec([0.3, 0.8, -0.5], nb, 0.05, 0.2)
    else:        # a height field's normals point along +z: lit from the front in even views, from behind in odd ones
        direction = _vec([0.2, 0.1, 0.0], nb, 0.1, 0.2)
        direction[:, 2] = 1.0 - 2.0 * (torch.arange(nb) % 2)
    return [0.45 + 0.1 * _wobble(nb, 1.1, 0.1), 0.6 + 0.1 * _wobble(nb, 0.8, 1.0), _vec([0.9, 0.8, 1.0], nb, 0.05, 0.3),
            _vec([1.0, 0.7, 0.6], nb, 0.05, 0.6), direction]


def light_inputs(c):
    """float32 inputs of a light case: vertices [1 or B,V,3], triangles [F,3] int32 (the grid's own for an implicit case:
    what the kernel derives from tri_batch = -W), the five parameters ([1,...] or [B,...]), the dense upstream gradient
    [B,F',3] (positive, so that the ambient sums do not cancel) and the rows the sparse one keeps.  No face is a sliver or
    near the horizon of a light that reads it (LIGHT_MARGIN)."""
    gen = _generator(c)
    B, n = c.views, c.n
    vb, nb = (1 if c.shared_vertices else B), (1 if c.shared_params else B)
    num_tri = n // 2 if c.fill_back else n
    light = _light_parameters(nb, c.grid)
    if c.grid is not None:
        H, W = c.grid
        step = 0.05          # (cells far above normalize's eps = 1e-5 in area)
        y, x = torch.meshgrid(step * torch.arange(H), step * torch.arange(W), indexing="ij")
        z = 0.1 * torch.sin(0.3 * x[None] + torch.arange(vb)[:, None, None]) * torch.cos(0.4 * y[None]) + \
            0.3 * step * torch.rand(vb, H, W, generator=gen)
        v = torch.stack([x[None].expand(vb, H, W), y[None].expand(vb, H, W), z], -1).reshape(vb, H * W, 3)
        tri = grid_triangles(H, W)
    else:
        V = 1024
        v = torch.rand(1, V, 3, generator=gen) * 2 - 1
        if vb > 1:          # one mesh, displaced a little in every view
            v = v + 0.02 * torch.randn(vb, V, 3, generator=gen)
        tri = torch.randint(0, V, (num_tri, 3), generator=gen, dtype=torch.int32)
        d64 = light[4].double().expand(B, 3)
        v64 = v.double().expand(B, V, 3)
        todo = torch.arange(num_tri)
        for _ in range(100):         # re-draw the slivers and the faces near the horizon of a light that reads them
            shape, lit = face_conditioning(v64[:, tri[todo].long()], d64)
            todo = todo[((shape < 1.25 * LIGHT_MARGIN) | (lit < 1.25 * LIGHT_MARGIN)).any(0)]
            if todo.numel() == 0:
                break
            tri[todo] = torch.randint(0, V, (todo.numel(), 3), generator=gen, dtype=torch.int32)
        else:
            raise AssertionError("light_inputs: could not place every face off the lights' horizons")
    g = (torch.rand(B, n, 3, generator=gen) + 0.5) * upstream_weights(n, B)
    return dict(vertices=v.contiguous(), tri=tri.contiguous(), light=[t.contiguous() for t in light],
                upstream=g.contiguous(), keep=sparse_rows(n, B, gen), num_tri=num_tri)


# ---- the references ------------------------------------------------------------------------------------------------------------
def camera_oracle(kind, vertices, params):
    """[B,V,3] -> [B,V,3] in the dtype of its arguments: oracle.nr_oracle's look_at / look + perspective, or projection"""
    return _oracle_camera(kind, vertices, params, ORIG_SIZE, ANGLE)


def camera_terms(kind, vertices, params, upstream, dtype):
    """Per-term form: vertices / upstream [nb,n,3] and parameters [nb,...] of nb views -> each parameter's [nb,n,P]: the
    contribution of (view, vertex) to each of its P entries.  One row per (view, vertex), every parameter a leaf per row."""
    nb, n = upstream.shape[:2]
    rows = nb * n
    leaves = [p.to(dtype)[:, None].expand(nb, n, *p.shape[1:]).reshape(rows, *p.shape[1:]).clone().requires_grad_(True)
              for p in params]
    out = camera_oracle(kind, vertices.to(dtype).reshape(rows, 1, 3), leaves)
    grads = torch.autograd.grad(out, leaves, upstream.to(dtype).reshape(rows, 1, 3))
    return [x.reshape(nb, n, -1) for x in grads]


def light_values(faces, ia, idr, ca, cd, direction):
    """lighting.py's per-face light in the dtype of its arguments: faces [...,3,3], intensities [...], colours and direction
    [...,3] -> [...,3].  ia*ca + id*cd*relu(n . d), n = normalize(cross(v0-v1, v2-v1), eps=1e-5); a term whose intensity is
    0 is skipped (it gives its parameters no gradient)."""
    normal = F.normalize(torch.cross(faces[..., 0, :] - faces[..., 1, :], faces[..., 2, :] - faces[..., 1, :], dim=-1),
                         eps=1e-5, dim=-1)
    cos = F.relu((normal * direction).sum(-1))
    zero = torch.zeros((), dtype=faces.dtype)
    ambient = torch.where((ia.detach() != 0)[..., None], ia[..., None] * ca, zero)
    directional = torch.where((idr.detach() != 0)[..., None], idr[..., None] * (cd * cos[..., None]), zero)
    return ambient + directional


def light_oracle(faces, light):
    """faces [Bl,F',3,3] and the five parameters ([1 or Bl], [1 or Bl,3]) -> the per-face light [Bl,F',3]"""
    ia, idr, ca, cd, dr = light
    return light_values(faces, ia.reshape(-1, 1), idr.reshape(-1, 1), ca.reshape(-1, 1, 3), cd.reshape(-1, 1, 3),
                        dr.reshape(-1, 1, 3)).expand(faces.shape[0], faces.shape[1], 3)


def light_terms(faces, light, upstream, dtype):
    """Per-term form: faces [nb,F',3,3], parameters [nb], [nb,3], upstream [nb,F',3] -> each parameter's [nb,F',P]"""
    nb, n = upstream.shape[:2]
    rows = nb * n
    leaves = [p.to(dtype)[:, None].expand(nb, n, *p.shape[1:]).reshape(rows, *p.shape[1:]).clone().requires_grad_(True)
              for p in light]
    out = light_values(faces.to(dtype).reshape(rows, 3, 3), *leaves)
    grads = torch.autograd.grad(out, leaves, upstream.to(dtype).reshape(rows, 3))
    return [x.reshape(nb, n, -1) for x in grads]


class Reference:
    """What the checks need of one case, per parameter k (entries flattened to P):
    ref[mode][k], bound[mode][k], ref32[mode][k]   [1 or B, P]   mode "dense" | "sparse" (float64; ref32 float32 sums)
    e32[mode][k]                                    max |ref32 - ref| / bound over the parameter's entries
    term[k], term32[k]                              [len(onehot), P]: the last view's terms at `onehot`
    chunks[mode][k]                                 [chunks, P]: the sum of each 256-chunk of the last view
    summed[k]                                       the parameter has batch 1 and the views' gradients are added"""

    def __init__(self, terms, n, views, keep, summed):
        self.n, self.views, self.summed = n, views, summed
        self.onehot = onehot_indices(n)
        group = max(1, ROWS_PER_GROUP // n)
        acc = {m: {"s": [], "a": [], "s32": []} for m in ("dense", "sparse")}
        nk = None
        for lo in range(0, views, group):
            hi = min(views, lo + group)
            t64, t32 = terms(lo, hi, torch.float64), terms(lo, hi, torch.float32)
            nk = len(t64)
            mask = keep[lo:hi, :, None]
            for m in ("dense", "sparse"):
                a64 = t64 if m == "dense" else [t * mask for t in t64]
                a32 = t32 if m == "dense" else [t * mask for t in t32]
                acc[m]["s"].append([t.sum(1) for t in a64])
                acc[m]["a"].append([t.abs().sum(1) for t in a64])
                acc[m]["s32"].append([t.sum(1) for t in a32])
                if hi == views:
                    pad = (-n) % LANES
                    setattr(self, "_chunks_" + m, [F.pad(t[-1], (0, 0, 0, pad)).reshape(-1, LANES, t.shape[-1]).sum(1)
                                                   for t in a64])
            if hi == views:
                self.term = [t[-1, self.onehot] for t in t64]
                self.term32 = [t[-1, self.onehot] for t in t32]
        self.ref, self.bound, self.ref32, self.e32 = {}, {}, {}, {}
        for m in ("dense", "sparse"):
            per_view = {q: [torch.cat([g[k] for g in acc[m][q]], 0) for k in range(nk)] for q in ("s", "a", "s32")}
            fold = lambda xs: [x.sum(0, keepdim=True) if s else x for x, s in zip(xs, summed)]      # noqa: E731
            self.ref[m], self.bound[m], self.ref32[m] = fold(per_view["s"]), fold(per_view["a"]), fold(per_view["s32"])
            self.e32[m] = [float(((r32.double() - r).abs() / b.clamp_min(1e-300))[b > 0].max()) if bool((b > 0).any()) else 0.0
                           for r, b, r32 in zip(self.ref[m], self.bound[m], self.ref32[m])]
        self.chunks = {m: getattr(self, "_chunks_" + m) for m in ("dense", "sparse")}

    def tolerance(self, mode, k):
        D = chain_length(self.n, self.views, self.summed[k])
        return (D * EPS32 + 4 * self.e32[mode][k]) * self.bound[mode][k]

    def term_tolerance(self, k):
        """of the one-hot check, per index: (8 2^-24 + 4 E32_term) |t|, with |t| the largest entry of the parameter's term
        and E32_term the largest |t32 - t| / |t| of the float32 terms in the same norm.  Per parameter and not per entry:
        an entry of a term is a difference of products of the size of the whole vector (the cross product of a face's
        normal, the projection in the adjoint of a normalisation), so its rounding error scales with the vector, and an
        entry can be arbitrarily small beside it (a normal perpendicular to an axis) -- per entry, two float32 evaluations
        of the same term that associate differently miss each other's 4x bound about one time in six there.  8: the
        additions a lone term still goes through are with zeros; what is left is its own arithmetic."""
        t, t32 = self.term[k], self.term32[k].double()
        size = t.abs().max(1).values
        e = float(((t32 - t).abs().max(1).values / size.clamp_min(1e-300))[size > 0].max()) if bool((size > 0).any()) else 0.0
        return (8 * EPS32 + 4 * e) * size, e


def _per_view(x, lo, hi):
    return x[lo:hi] if x.shape[0] > 1 else x.expand(hi - lo, *x.shape[1:])


def camera_reference(c, inp=None):
    inp = camera_inputs(c) if inp is None else inp

    def terms(lo, hi, dtype):
        return camera_terms(c.kind, _per_view(inp["vertices"], lo, hi), [_per_view(p, lo, hi) for p in inp["params"]],
                            inp["upstream"][lo:hi], dtype)
    summed = [c.shared_params or c.views == 1] * len(inp["params"])
    return Reference(terms, c.n, c.views, inp["keep"], summed)


def light_reference(c, inp=None):
    inp = light_inputs(c) if inp is None else inp

    def terms(lo, hi, dtype):
        faces = gather_faces(_per_view(inp["vertices"], lo, hi), inp["tri"], c.fill_back)
        return light_terms(faces, [_per_view(p, lo, hi) for p in inp["light"]], inp["upstream"][lo:hi], dtype)
    summed = [c.shared_params or c.views == 1] * 5
    return Reference(terms, c.n, c.views, inp["keep"], summed)


# ---- the references against autograd of the shared parameter and against the reference project's own numbers ------------------
def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("c", [c for c in camera_cases() if c.n * c.views <= 200000 and c.n in (65, 1025, 50625)], ids=case_id)
def test_camera_per_term_reference_sums_to_plain_autograd(c):
    inp = camera_inputs(c)
    ref = camera_reference(c, inp)
    p64 = [p.double().requires_grad_(True) for p in inp["params"]]
    out = camera_oracle(c.kind, inp["vertices"].double().expand(c.views, -1, -1), p64)
    for mode, g in (("dense", inp["upstream"]), ("sparse", inp["upstream"] * inp["keep"][:, :, None])):
        grads = torch.autograd.grad(out, p64, g.double(), retain_graph=True)
        for k, (a, b) in enumerate(zip(ref.ref[mode], grads)):
            assert _rel(a.reshape(b.shape), b) <= 1e-12, (mode, CAMERA_NAMES[c.kind][k])
            assert bool((ref.bound[mode][k] >= a.abs()).all())


@pytest.mark.parametrize("case", ["look_at_shared", "look_at_per_batch", "look_shared", "look_per_batch",
                                  "projection_shared", "projection_per_batch"])
def test_camera_oracle_reproduces_the_reference_golden(case):
    z = np.load(GOLDEN_CAMERA)
    kind = case.rsplit("_", 2)[0] if "per_batch" in case else case.rsplit("_", 1)[0]
    n = 4 if kind == "projection" else 3
    p64 = [torch.from_numpy(z[f"{case}/p{k}"]).double().requires_grad_(True) for k in range(n)]
    out = _oracle_camera(kind, torch.from_numpy(z["vertices"]).double(), p64, float(z["orig_size"]), float(z["angle"]))
    assert torch.allclose(out.detach().float(), torch.from_numpy(z[f"{case}/out"]), rtol=2e-4, atol=2e-5)
    grads = torch.autograd.grad(out, p64, torch.from_numpy(z["upstream"]).double())
    for k in range(n):
        want = torch.from_numpy(z[f"{case}/grad_p{k}"])
        assert torch.allclose(grads[k].float(), want, rtol=2e-4, atol=2e-5), (case, k)
    # ... and the per-term form gives the same sums
    B, V = z["vertices"].shape[:2]
    rows = [p.detach().reshape(-1, *p.shape[(p.dim() - (2 if kind == "projection" and k < 2 else 1)):])
            for k, p in enumerate(p64)]
    rows = [r.reshape(-1, 3) if kind == "projection" and k == 2 else r for k, r in enumerate(rows)]
    terms = camera_terms(kind, torch.from_numpy(z["vertices"]), [r.expand(B, *r.shape[1:]) for r in rows],
                         torch.from_numpy(z["upstream"]), torch.float64)
    for k in range(n):
        total = terms[k].sum(1) if rows[k].shape[0] > 1 else terms[k].sum((0, 1))
        assert _rel(total.reshape(grads[k].shape), grads[k]) <= 1e-12, (case, k)


@pytest.mark.parametrize("case", ["shared", "per_batch", "zero_dim"])
def test_light_oracle_reproduces_the_reference_golden(case):
    z = np.load(GOLDEN_LIGHT)
    faces = torch.from_numpy(z["faces"]).double()
    grad_light = torch.from_numpy((z["upstream"].astype(np.float64) * z["textures"]).sum((2, 3, 4)))     # [bs,nf,3]
    p64 = [torch.from_numpy(z[f"{case}/{n}"]).double().requires_grad_(True) for n in LIGHT_NAMES]
    light = light_oracle(faces, p64)
    lit = torch.from_numpy(z["textures"]).double() * light[:, :, None, None, None, :]
    assert _rel(lit.detach(), torch.from_numpy(z[f"{case}/lit"])) < 1e-6
    grads = torch.autograd.grad(light, p64, grad_light)
    for n, g in zip(LIGHT_NAMES, grads):
        assert _rel(g, torch.from_numpy(z[f"{case}/grad_{n}"])) < 1e-5, n
    bs = faces.shape[0]
    rows = [p.detach().reshape(-1) if k < 2 else p.detach().reshape(-1, 3) for k, p in enumerate(p64)]
    terms = light_terms(faces, [r.expand(bs, *r.shape[1:]) for r in rows], grad_light, torch.float64)
    for k, n in enumerate(LIGHT_NAMES):
        total = terms[k].sum(1) if rows[k].shape[0] > 1 else terms[k].sum((0, 1))
        assert _rel(total.reshape(grads[k].shape), grads[k]) <= 1e-12, n


def test_light_oracle_skips_a_term_of_intensity_zero():
    faces = torch.randn(2, 7, 3, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    for zero in (0, 1):
        p = [torch.tensor([0.4]), torch.tensor([0.7]), torch.tensor([[0.9, 0.8, 1.0]]), torch.tensor([[1.0, 0.7, 0.6]]),
             torch.tensor([[0.3, 0.8, -0.5]])]
        p[zero] = torch.zeros(1)
        p = [x.double().requires_grad_(True) for x in p]
        grads = torch.autograd.grad(light_oracle(faces, p), p, torch.ones(2, 7, 3, dtype=torch.float64))
        skipped = (0, 2) if zero == 0 else (1, 3, 4)
        for k in range(5):
            assert (float(grads[k].abs().sum()) == 0) == (k in skipped), (zero, k)


@pytest.mark.parametrize("c", [c for c in light_cases() if c.n * c.views <= 200000 and c.n in (64, 1024, 4097)], ids=case_id)
def test_light_per_term_reference_sums_to_plain_autograd(c):
    inp = light_inputs(c)
    ref = light_reference(c, inp)
    p64 = [p.double().requires_grad_(True) for p in inp["light"]]
    faces = gather_faces(inp["vertices"].double().expand(c.views, -1, -1), inp["tri"], c.fill_back)
    assert faces.shape[1] == c.n
    out = light_oracle(faces, p64)
    for mode, g in (("dense", inp["upstream"]), ("sparse", inp["upstream"] * inp["keep"][:, :, None])):
        grads = torch.autograd.grad(out, p64, g.double(), retain_graph=True)
        for k, (a, b) in enumerate(zip(ref.ref[mode], grads)):
            assert _rel(a.reshape(b.shape), b) <= 1e-12, (mode, LIGHT_NAMES[k])


# ---- the cases cover what the issue lists, and their inputs are sharp ------------------------------------------------------------
def test_cases_cover_every_size_view_count_mode_and_shape():
    cam, lit = camera_cases(), light_cases()
    assert {(c.n, c.views) for c in cam} == set(_sizes_and_views(CAMERA_SIZES))
    assert {(c.n, c.views) for c in lit} == set(_sizes_and_views(LIGHT_SIZES))
    # the whole product: every mode / variant at every size and number of views
    assert {(c.kind, c.n, c.views) for c in cam} == {(k, n, b) for n, b in _sizes_and_views(CAMERA_SIZES) for k in KINDS}
    assert {(c.n, c.views, c.fill_back, c.grid) for c in lit} == \
        {(n, b, fb, g) for n, b in _sizes_and_views(LIGHT_SIZES) for fb, g in light_variants(n)}
    regimes = lambda n: 0 if parts_of(n) == 1 else (1 if parts_of(n) < MAX_PARTS else 2)  # noqa: E731
    # every mode with every combination of batch shapes at one part, between, and at the cap (more than one view)
    seen = {(c.kind, c.shared_params, c.shared_vertices, regimes(c.n)) for c in cam if c.views > 1}
    for kind in KINDS:
        for sp, sv in BATCH_SHAPES:
            for r in (0, 1, 2):
                assert (kind, sp, sv, r) in seen, (kind, sp, sv, r)
    seen = {(c.fill_back, c.grid is not None, c.shared_params, regimes(c.n)) for c in lit if c.views > 1}
    for fb in (0, 1):
        for grid in (False, True):
            for sp in (False, True):
                for r in (0, 2):       # (between one part and the cap the listed sizes are odd: indexed, no fill_back)
                    assert (fb, grid, sp, r) in seen, (fb, grid, sp, r)
    assert {sp for (fb, grid, sp, r) in seen if r == 1} == {False, True}
    # 300 views: both parameter shapes, for both kernels, at both sizes, in every mode
    for n in LONG_SIZES:
        for kind in KINDS:
            assert {c.shared_params for c in cam if (c.kind, c.n, c.views) == (kind, n, LONG_VIEWS)} == {False, True}
        assert {c.shared_params for c in lit if (c.n, c.views) == (n, LONG_VIEWS)} == {False, True}
    assert {c.shared_vertices for c in lit} == {False, True}
    for c in lit:           # the grids are ones tri_source_ok accepts
        if c.grid is not None:
            H, W = c.grid
            assert H >= 2 and W >= 2 and 2 * (H - 1) * (W - 1) * (2 if c.fill_back else 1) == c.n
    # the benchmark's own: 32 views of the 225 x 225 grid with fill_back, F' = 200 704; 50 625 vertices
    assert any(c[:4] == (200704, 32, 1, (225, 225)) for c in lit) and any((c.n, c.views) == (50625, 32) for c in cam)


def _assert_sharp(ref, names, what):
    """(a) the float32 evaluation passes the check the kernel has to pass; (b) no 256-chunk of the LAST view can be removed
    without moving some entry by more than ten times its tolerance; (c) the one-hot tolerance stays far below the term.
    (b) holds for the last view only, which the inputs are built for (upstream_weights): in a parameter of batch 1 summed
    over 32 views of 131 072 elements or more, a chunk of another view is about 5e-6 of the bound and below the tolerance.
    The other views' partial slots rest on the cases with per-view parameters, where every view has its own bound."""
    for mode in ("dense", "sparse"):
        worst = None
        for k, name in enumerate(names):
            tol = ref.tolerance(mode, k)
            assert bool(((ref.ref32[mode][k].double() - ref.ref[mode][k]).abs() <= tol).all()), (what, mode, name)
            t = tol[-1]                      # (the last view's row, or the only one)
            moved = torch.where(t > 0, ref.chunks[mode][k].abs() / (10 * t.clamp_min(1e-300)), torch.zeros(()).double())
            worst = moved.max(1).values if worst is None else torch.maximum(worst, moved.max(1).values)
        assert float(worst.min()) > 1.0, (what, mode, "chunk", int(worst.argmin()), float(worst.min()))
    for k, name in enumerate(names):        # the one-hot terms: the float32 term passes its own check
        tol, e = ref.term_tolerance(k)
        assert bool(((ref.term32[k].double() - ref.term[k]).abs().max(1).values <= tol).all()), (what, "one-hot", name)
        assert 8 * EPS32 + 4 * e < 0.1, (what, "one-hot", name, e)       # a dropped or doubled term misses by |t|


@pytest.mark.parametrize("c", camera_cases(), ids=case_id)
def test_camera_case_inputs_are_sharp(c):
    inp = camera_inputs(c)
    if c.kind == "projection":       # off the optical axis, in front of the camera
        v = inp["vertices"].double().expand(c.views, -1, -1)
        K, R, t, d = (p.double().expand(c.views, *p.shape[1:]) for p in inp["params"])
        cam = torch.matmul(v, R.transpose(1, 2)) + t[:, None]
        assert float(cam[..., 2].min()) > 2.0 and float((cam[..., :2] / cam[..., 2:]).norm(dim=-1).min()) > 1e-2
    else:                            # in front of the camera and beside its axis
        v = inp["vertices"].double().expand(c.views, -1, -1)
        eye, second, up = (p.double().expand(c.views, 3) for p in inp["params"])
        z = F.normalize(second - eye if c.kind == "look_at" else second, dim=-1)
        d = v - eye[:, None]
        depth = (d * z[:, None]).sum(-1)
        assert float(depth.min()) > 1.5 and float(torch.atan2((d - depth[..., None] * z[:, None]).norm(dim=-1), depth).min()) > 0.05
    _assert_sharp(camera_reference(c, inp), CAMERA_NAMES[c.kind], c)


@pytest.mark.parametrize("c", light_cases(), ids=case_id)
def test_light_case_inputs_are_sharp(c):
    inp = light_inputs(c)
    faces = gather_faces(inp["vertices"].double().expand(c.views, -1, -1), inp["tri"], c.fill_back)
    shape, lit = face_conditioning(faces, inp["light"][4].double().expand(c.views, 3))
    assert float(shape.min()) > LIGHT_MARGIN and float(lit.min()) > LIGHT_MARGIN, (float(shape.min()), float(lit.min()))
    a = faces[:, :, 0] - faces[:, :, 1]
    assert float(torch.cross(a, faces[:, :, 2] - faces[:, :, 1], dim=-1).norm(dim=-1).min()) > 1e-3      # (normalize's eps: 1e-5)
    _assert_sharp(light_reference(c, inp), LIGHT_NAMES, c)


# ---- size arithmetic through the library -------------------------------------------------------------------------------------
def test_workspace_bytes_follow_the_documented_rule():
    from deep3dmap_amd import _lib
    L = _lib.lib()
    assert [parts_of(n) for n in (1, 1024, 1025, 4097, 50625, 131072, 131073, 200704, 300001)] == \
        [1, 1, 2, 5, 50, 128, 128, 128, 128]
    modes = (_lib.CAMERA_LOOK_AT, _lib.CAMERA_LOOK, _lib.CAMERA_PROJECTION)
    for B in VIEWS + (LONG_VIEWS,):
        for n in sorted(set(CAMERA_SIZES + LIGHT_SIZES)):
            for mode in modes:
                assert L.d3m_camera_params_backward_workspace_bytes(B, n, mode) == 4 * B * (parts_of(n) * CAM_SUMS + CAM_ROW)
            assert L.d3m_light_params_backward_workspace_bytes(B, n, 0) == 4 * B * (parts_of(n) * LIGHT_SUMS + LIGHT_ROW)
            assert L.d3m_light_params_backward_workspace_bytes(B, n, 1) == 4 * B * (parts_of(2 * n) * LIGHT_SUMS + LIGHT_ROW)
    for B, n in ((0, 5), (-1, 5), (3, 0), (3, -7)):
        assert L.d3m_camera_params_backward_workspace_bytes(B, n, _lib.CAMERA_LOOK_AT) == 0
        assert L.d3m_light_params_backward_workspace_bytes(B, n, 0) == 0
        assert L.d3m_light_params_backward_workspace_bytes(B, n, 1) == 0
    assert L.d3m_camera_params_backward_workspace_bytes(3, 5, _lib.CAMERA_NONE) == 0
    assert L.d3m_camera_params_backward_workspace_bytes(3, 5, 7) == 0
