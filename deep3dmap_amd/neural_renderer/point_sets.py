"""Nearest points and chamfer distances between point sets: the data term of a fit of a mesh to a 3D target (a scan, a fused
depth point cloud, another mesh's vertices), beside mesh_regularizer's priors.  Exact brute force; csrc/d3m_point_sets.h states
the distance, the tie rule, the order of every sum and the adjoint.

    nearest_points(points [B,N,3], targets [B,M,3]) -> index [B,N] (int32), dist2 [B,N]
        for every point the target j that minimises (the f32 squared distance, j): the lowest index among equal distances; the
        squared distance is formed from the coordinate differences.  -1 and +0 for a point at or beyond its set's length and
        for every point of an element without targets; -1 and NaN where every candidate distance is NaN.
    chamfer_distance(a [B,N,3], b [B,M,3]) -> value [B]
        value[b] = weight_ab L_ab + weight_ba L_ba,  L_ab = (1/n_b) sum over a's points of rho(dist2 to the nearest point of b),
        rho(d2) = d2 (squared=True: pytorch3d's chamfer) or sqrt(d2) (the distance mesh_eval averages); truncate = tau: a term
        with d2 > tau^2 contributes rho(tau^2) and has no gradient (at equality it is not truncated).  A direction of weight 0 is
        not evaluated; an empty query set contributes 0.

Both are differentiable in both sets with the argmin held constant: a point as a query receives c rho' (a_i - b_nn(i)), a plain
store; a point as somebody's nearest neighbour receives minus those terms through a 64-bit fixed-point integer scatter -- no
float atomics, the same bits on every run and for every split count, every element written, exactly +0 at points beyond a
set's length and at truncated terms.  A NaN in the inputs gives a NaN value and NaN gradients.  No host synchronisation:
forward and backward can be captured.

Launches, whatever B, N, M, the lengths and the options: nearest_points 3 (k_pset_init, k_pset_nearest, k_pset_resolve);
chamfer_distance forward 4 (k_pset_init, k_pset_nearest, k_pset_resolve, k_pset_value_finish); either backward 3 (k_pset_direct,
k_pset_scatter, k_pset_convert)."""
import torch
import torch.nn as nn

from .. import _lib

TILE = 512                  # PSET_TILE of csrc/d3m_point_sets.h: targets a workgroup stages at a time (d3m_point_set_tile)
QUERIES_PER_LANE = 4        # PSET_Q (d3m_point_set_queries_per_lane); a workgroup takes 256 times as many queries
MAX_SETS = 65535
MAX_POINTS = 1 << 30
KERNELS_NEAREST = ("k_pset_init", "k_pset_nearest", "k_pset_resolve")
KERNELS_FORWARD = KERNELS_NEAREST + ("k_pset_value_finish",)
KERNELS_BACKWARD = ("k_pset_direct", "k_pset_scatter", "k_pset_convert")


def auto_splits(batch_size, num_queries, num_targets):
    """The number of workgroups the kernel splits the targets over per query block at these shapes (d3m_point_set_splits)."""
    return int(_lib.lib().d3m_point_set_splits(int(batch_size), int(num_queries), int(num_targets)))


def _scratch(B, N, M, device):
    n = int(_lib.lib().d3m_chamfer_distance_scratch_bytes(B, N, M))
    return torch.empty(max((n + 7) // 8, 1), dtype=torch.int64, device=device)


def _backward(a, b, la, lb, ab, ba, coef, upstream, per_query, squared, truncate):
    """d3m_chamfer_distance_backward: (grad_a [B,N,3], grad_b [B,M,3]); ab / ba: (index, dist2) or (None, None)."""
    B, N, M = int(a.shape[0]), int(a.shape[1]), int(b.shape[1])
    scratch = _scratch(B, N, M, a.device)
    grad_a, grad_b = torch.empty_like(a), torch.empty_like(b)
    _lib.check(_lib.lib().d3m_chamfer_distance_backward(
        _lib.ptr(a), _lib.ptr(b), B, N, M, _lib.ptr(la), _lib.ptr(lb), _lib.ptr(ab[0]), _lib.ptr(ab[1]), _lib.ptr(ba[0]),
        _lib.ptr(ba[1]), _lib.ptr(coef), _lib.ptr(upstream), int(per_query), int(squared), truncate, _lib.ptr(scratch),
        scratch.numel() * 8, _lib.ptr(grad_a), _lib.ptr(grad_b), _lib.stream_ptr()), "d3m_chamfer_distance_backward")
    return grad_a, grad_b


class _NearestPoints(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, targets, lengths, target_lengths, splits):
        a, b = points.contiguous(), targets.contiguous()
        B, N, M = int(a.shape[0]), int(a.shape[1]), int(b.shape[1])
        scratch = _scratch(B, N, M, a.device)
        index = torch.empty(B, N, dtype=torch.int32, device=a.device)
        dist2 = torch.empty(B, N, dtype=torch.float32, device=a.device)
        _lib.check(_lib.lib().d3m_nearest_points(_lib.ptr(a), _lib.ptr(b), B, N, M, _lib.ptr(lengths), _lib.ptr(target_lengths),
                                                 splits, _lib.ptr(scratch), scratch.numel() * 8, _lib.ptr(index),
                                                 _lib.ptr(dist2), _lib.stream_ptr()), "d3m_nearest_points")
        ctx.save_for_backward(a, b, index, dist2, *(t for t in (lengths, target_lengths) if t is not None))
        ctx.have = (lengths is not None, target_lengths is not None)
        ctx.mark_non_differentiable(index)
        return index, dist2

    @staticmethod
    def backward(ctx, _grad_index, grad_dist2):
        a, b, index, dist2, *rest = ctx.saved_tensors
        rest = iter(rest)
        la, lb = (next(rest) if have else None for have in ctx.have)
        upstream = grad_dist2.to(torch.float32).contiguous()                # stays on the device
        grad_a, grad_b = _backward(a, b, la, lb, (index, dist2), (None, None), None, upstream, True, True, -1.0)
        return grad_a, grad_b, None, None, None


class _ChamferDistance(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, la, lb, options):
        squared, truncate, weight_ab, weight_ba, splits = options
        a, b = a.contiguous(), b.contiguous()
        B, N, M = int(a.shape[0]), int(a.shape[1]), int(b.shape[1])
        dev = a.device
        scratch = _scratch(B, N, M, dev)
        pair = lambda n, on: ((torch.empty(B, n, dtype=torch.int32, device=dev), torch.empty(B, n, dtype=torch.float32, device=dev))
                              if on else (None, None))
        ab, ba = pair(N, weight_ab > 0.0), pair(M, weight_ba > 0.0)
        coef = torch.empty(B, 2, dtype=torch.float32, device=dev)
        value = torch.empty(B, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().d3m_chamfer_distance(
            _lib.ptr(a), _lib.ptr(b), B, N, M, _lib.ptr(la), _lib.ptr(lb), int(squared), truncate, weight_ab, weight_ba, splits,
            _lib.ptr(scratch), scratch.numel() * 8, _lib.ptr(ab[0]), _lib.ptr(ab[1]), _lib.ptr(ba[0]), _lib.ptr(ba[1]),
            _lib.ptr(coef), _lib.ptr(value), _lib.stream_ptr()), "d3m_chamfer_distance")
        saved = (a, b, coef) + tuple(t for t in ab + ba + (la, lb) if t is not None)
        ctx.save_for_backward(*saved)
        ctx.have = (weight_ab > 0.0, weight_ba > 0.0, la is not None, lb is not None)
        ctx.options = options
        return value

    @staticmethod
    def backward(ctx, grad_value):
        a, b, coef, *rest = ctx.saved_tensors
        rest = iter(rest)
        have_ab, have_ba, have_la, have_lb = ctx.have
        ab = (next(rest), next(rest)) if have_ab else (None, None)
        ba = (next(rest), next(rest)) if have_ba else (None, None)
        la = next(rest) if have_la else None
        lb = next(rest) if have_lb else None
        squared, truncate = ctx.options[:2]
        upstream = grad_value.reshape(-1).to(torch.float32).contiguous()    # stays on the device
        grad_a, grad_b = _backward(a, b, la, lb, ab, ba, coef, upstream, False, squared, truncate)
        return grad_a, grad_b, None, None, None


def _checked_sets(name, a, b, a_name, b_name):
    """(batched, a [B,N,3], b [B,M,3]) of two point sets of rank 2 (both) or 3 (both)"""
    for t, n in ((a, a_name), (b, b_name)):
        if not torch.is_tensor(t):
            raise ValueError(f"{name}: {n} must be a tensor")
        if t.dim() not in (2, 3) or t.shape[-1] != 3:
            raise ValueError(f"{name}: {n} must be [num_points, 3] or [B, num_points, 3]")
        if t.dtype != torch.float32:
            raise ValueError(f"{name}: {n} must be float32")
        if t.shape[-2] < 1 or t.shape[-2] > MAX_POINTS:
            raise ValueError(f"{name}: {n}: 1 to 2^30 points (N = 0 and M = 0 are refused: give lengths for empty sets)")
    if a.dim() != b.dim():
        raise ValueError(f"{name}: {a_name} and {b_name} must both be [num_points, 3] or both [B, num_points, 3]")
    batched = a.dim() == 3
    if batched and a.shape[0] != b.shape[0]:
        raise ValueError(f"{name}: {a_name} and {b_name} have different batch sizes")
    if batched and not 1 <= a.shape[0] <= MAX_SETS:
        raise ValueError(f"{name}: {a_name}: 1 to {MAX_SETS} sets per call")
    if a.device != b.device:
        raise ValueError(f"{name}: {a_name} and {b_name} must be on one device")
    return batched, (a if batched else a[None]), (b if batched else b[None])


def _checked_lengths(name, lengths, what, like):
    """lengths [B] as int32 on the sets' device, or None"""
    if lengths is None:
        return None
    B = int(like.shape[0])
    if not torch.is_tensor(lengths) or lengths.dim() != 1 or lengths.shape[0] != B:
        raise ValueError(f"{name}: {what} must be a tensor [B] with the sets' batch size")
    if lengths.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{name}: {what} must be int32 or int64")
    if lengths.device != like.device:
        raise ValueError(f"{name}: {what} must be on the sets' device")
    return lengths.to(torch.int32).contiguous()


def _checked_splits(name, splits):
    splits = 0 if splits is None else int(splits)
    if splits < 0:
        raise ValueError(f"{name}: _splits must be positive")
    return splits


def _on_gpu(name, t):
    if not t.is_cuda:
        raise ValueError(f"{name}: the point sets must be on a GPU device")


def nearest_points(points, targets, lengths=None, target_lengths=None, _splits=None):
    """(index, dist2) of every point's nearest target (the module text).  points [N,3] or [B,N,3], targets [M,3] or [B,M,3], f32 on
    one GPU; lengths / target_lengths [B] (int32 or int64 on that device): the ragged set sizes, clamped to 0 .. N and 0 .. M;
    None: N and M.  index is int32 of shape [N] or [B,N] and not differentiable; dist2 is differentiable in points and targets,
    the index held constant.  ValueError, before anything is launched, for a wrong rank, dtype, last dimension, batch size, device
    or no points.  _splits forces the kernel's split count (no result depends on it by a bit)."""
    name = "nearest_points"
    batched, a, b = _checked_sets(name, points, targets, "points", "targets")
    la = _checked_lengths(name, lengths, "lengths", a)
    lb = _checked_lengths(name, target_lengths, "target_lengths", a)
    splits = _checked_splits(name, _splits)
    _on_gpu(name, a)
    index, dist2 = _NearestPoints.apply(a, b, la, lb, splits)
    return (index, dist2) if batched else (index[0], dist2[0])


def _checked_options(name, squared, truncate, weight_ab, weight_ba, splits):
    w = (float(weight_ab), float(weight_ba))
    if not all(0.0 <= v < float("inf") for v in w):                 # (NaN fails too)
        raise ValueError(f"{name}: weight_ab and weight_ba must be >= 0 and finite")
    if not any(v > 0.0 for v in w):
        raise ValueError(f"{name}: one of weight_ab and weight_ba must be > 0")
    tau = -1.0
    if truncate is not None:
        tau = float(truncate)
        if not 0.0 <= tau < float("inf"):
            raise ValueError(f"{name}: truncate must be None or >= 0 and finite")
    return (bool(squared), tau, w[0], w[1], _checked_splits(name, splits))


def chamfer_distance(a, b, a_lengths=None, b_lengths=None, squared=True, truncate=None, weight_ab=1.0, weight_ba=1.0,
                     _splits=None):
    """weight_ab L_ab + weight_ba L_ba between the point sets a and b (the module text), differentiable in both: one autograd
    node.  a [N,3] or [B,N,3], b [M,3] or [B,M,3], f32 on one GPU; a_lengths / b_lengths [B] as nearest_points takes them.
    Returns [B], or a 0-d tensor for unbatched sets.  ValueError, before anything is launched, for what nearest_points refuses, a
    negative or non-finite weight, both weights 0, or a negative or non-finite truncate."""
    name = "chamfer_distance"
    batched, a3, b3 = _checked_sets(name, a, b, "a", "b")
    la = _checked_lengths(name, a_lengths, "a_lengths", a3)
    lb = _checked_lengths(name, b_lengths, "b_lengths", a3)
    options = _checked_options(name, squared, truncate, weight_ab, weight_ba, _splits)
    _on_gpu(name, a3)
    value = _ChamferDistance.apply(a3, b3, la, lb, options)
    return value if batched else value[0]


class ChamferTarget(nn.Module):
    """The data term of a fit to one target: `target_points` [M,3] or [B,M,3] and `target_lengths` as buffers, and
    chamfer_distance's options; forward(points) returns chamfer_distance(points, target_points, ...).  A target of [M,3] serves
    points [N,3], and points [B,N,3] of any B (it is repeated).  Stands beside MeshRegularizer."""

    def __init__(self, target_points, target_lengths=None, squared=True, truncate=None, weight_ab=1.0, weight_ba=1.0):
        super().__init__()
        _checked_options("ChamferTarget", squared, truncate, weight_ab, weight_ba, None)
        target = torch.as_tensor(target_points)
        if target.dim() not in (2, 3) or target.shape[-1] != 3 or target.shape[-2] < 1:
            raise ValueError("ChamferTarget: target_points must be [num_points, 3] or [B, num_points, 3]")
        self.squared, self.truncate = bool(squared), None if truncate is None else float(truncate)
        self.weight_ab, self.weight_ba = float(weight_ab), float(weight_ba)
        self.register_buffer("target_points", target.detach().to(torch.float32).contiguous().clone())
        self.register_buffer("target_lengths", None if target_lengths is None else
                             torch.as_tensor(target_lengths).detach().to(torch.int32).reshape(-1).contiguous().clone())

    @property
    def options(self):
        return dict(squared=self.squared, truncate=self.truncate, weight_ab=self.weight_ab, weight_ba=self.weight_ba)

    def forward(self, points, lengths=None):
        target, target_lengths = self.target_points, self.target_lengths
        if torch.is_tensor(points) and points.dim() == 3 and target.dim() == 2:
            target = target[None].expand(points.shape[0], -1, -1)
            if target_lengths is not None:
                target_lengths = target_lengths.expand(points.shape[0])
        return chamfer_distance(points, target, lengths, target_lengths, **self.options)
