"""Shape regularisers of an indexed mesh: the uniform Laplacian, the edge-length and the normal-consistency term of a vertex
fit, value and gradient in one autograd node (`mesh_regularizer`, `MeshRegularizer`).

    L_lap  = (1/V) sum_v |x_v - mean of N(v)|^2                      (a vertex of no face adds 0)
    L_edge = (1/E) sum over the unique edges of (|x_a - x_b| - edge_target)^2
    L_nc   = (1/P) sum over the wing records of (1 - cos(n0, n1)),   n0 = (b-a) x (c-a), n1 = -(b-a) x (d-a)

A wing record (a, b, c, d) is an edge a < b with the third vertices of two of its faces; the sign of n1 makes a flat pair
give cos = 1 whatever the faces' winding.  d3m_mesh_regularizer evaluates all three as gathers over the topology of the faces
-- no float atomics, the same bits on every run.  The topology (unique edges as a neighbour CSR, the wing records, the wing
CSR, the chunk tables of the rows above LONG_ROW items: row_gather.py) is built once per (faces tensor, version, V) with torch operators and kept
in a bounded LRU cache of its own, like vertex_colors' adjacency."""
import ctypes
from collections import namedtuple

import torch
import torch.nn as nn

from .. import _lib
from .row_gather import BuiltCache, build_csr, checked_faces as _checked_faces, tensor_key

MAX_FACES_PER_EDGE = 16     # an edge of n faces gives n (n - 1) / 2 wing records

MeshTopology = namedtuple("MeshTopology", "edges wings nbr wing num_vertices num_edges num_wings c")
MeshTopology.__doc__ = """The faces of one mesh as d3m_mesh_regularizer reads them (all i32): edges [E,2] (a < b, sorted),
wings [P,4] = (a, b, c, d) ordered by (edge, i, j), nbr: the neighbour Csr of V rows (items [2E]: a vertex's distinct
neighbours, ascending), wing: the wing Csr of V rows (items [4P]: item = 4 p + role, ascending per vertex; row_gather.Csr),
and `c`: the d3m_mesh_topology that points at them."""


class TopologyCache(BuiltCache):
    """BuiltCache for mesh topologies: an entry also holds the caller's faces tensor."""
    what = "mesh_regularizer: the faces' topology"


_cache = TopologyCache()


def build_topology(faces, num_vertices):
    """The MeshTopology of faces [F,3] (int32 or int64, any device) over num_vertices vertices.  ValueError for an index
    outside [0, num_vertices) and for an edge of more than MAX_FACES_PER_EDGE faces.  Synchronises: never inside a capture."""
    V = int(num_vertices)
    dev = faces.device
    tri = faces.reshape(-1, 3).long()
    F = tri.shape[0]
    lo, hi = int(tri.min()), int(tri.max())
    if lo < 0 or hi >= V:
        raise ValueError(f"faces: vertex indices must be in [0, {V}) (found {lo if lo < 0 else hi})")
    i32 = dict(dtype=torch.int32, device=dev)
    # the three sides of every face, side s opposite corner (s + 2) % 3: (a, b) = (min, max), key a V + b
    src, dst, third = tri[:, [0, 1, 2]].reshape(-1), tri[:, [1, 2, 0]].reshape(-1), tri[:, [2, 0, 1]].reshape(-1)
    a, b = torch.minimum(src, dst), torch.maximum(src, dst)
    side_key = a * V + b
    keys = torch.unique(side_key[a != b])                       # sorted: by (min, max)
    E = int(keys.numel())
    ea, eb = torch.div(keys, V, rounding_mode="floor"), keys % V
    # neighbour CSR: both directions of every edge, sorted by (vertex, neighbour)
    directed = torch.sort(torch.cat([keys, eb * V + ea]))[0]
    nbr_rows, nbr_items = torch.div(directed, V, rounding_mode="floor"), directed % V
    # wings: the sides of the faces that repeat no index, sorted by (edge, face)
    proper = (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 2] != tri[:, 0])
    keep = proper[:, None].expand(F, 3).reshape(-1)
    side_edge = torch.searchsorted(keys, side_key[keep])
    side_face = torch.arange(F, device=dev)[:, None].expand(F, 3).reshape(-1)[keep]
    order = torch.argsort(side_edge * F + side_face)
    side_edge, side_third = side_edge[order], third[keep][order]
    per_edge = torch.bincount(side_edge, minlength=E)
    if E and int(per_edge.max()) > MAX_FACES_PER_EDGE:
        raise ValueError(f"faces: an edge of {int(per_edge.max())} faces (at most {MAX_FACES_PER_EDGE}: its wing records "
                         "grow with the square)")
    first_of_edge = torch.cumsum(per_edge, 0) - per_edge
    n_sides = side_edge.numel()
    rank = torch.arange(n_sides, device=dev) - first_of_edge[side_edge]
    later = per_edge[side_edge] - 1 - rank                       # records side i opens: one per j > i, in j order
    i_side = torch.repeat_interleave(torch.arange(n_sides, device=dev), later)
    P = int(i_side.numel())
    j_side = i_side + 1 + (torch.arange(P, device=dev) - (torch.cumsum(later, 0) - later)[i_side])
    e_of = side_edge[i_side]
    wings = torch.stack([ea[e_of], eb[e_of], side_third[i_side], side_third[j_side]], 1).reshape(-1, 4)
    nbr = build_csr(nbr_rows, V, nbr_items)
    # item = 4 p + role; stable: ascending per vertex
    wing = build_csr(wings.reshape(-1), V, torch.argsort(wings.reshape(-1), stable=True))
    edges, wings = torch.stack([ea, eb], 1).to(**i32).contiguous(), wings.to(**i32).contiguous()
    c = _lib.D3MMeshTopology(nbr.c, wing.c, wings.data_ptr() if P else None, E, P)
    return MeshTopology(edges, wings, nbr, wing, V, E, P, c)


def mesh_topology(faces, num_vertices, cache=None):
    """The cached MeshTopology of a faces tensor [F,3] or [1,F,3], int32 or int64 (built on the first call with this tensor
    at its current version, outside any stream capture); `cache`: the TopologyCache to keep it in (default: the module's)."""
    faces = _checked_faces(faces)
    cache = _cache if cache is None else cache
    return cache.get(tensor_key(faces) + (int(num_vertices),), lambda: build_topology(faces, num_vertices), holders=(faces,))


def _checked_weights(laplacian, edge, edge_target, normal):
    w = tuple(float(x) for x in (laplacian, edge, edge_target, normal))
    if not all(x >= 0.0 for x in w):           # (NaN fails too)
        raise ValueError("laplacian, edge, edge_target and normal must be >= 0")
    return w


def evaluate(vertices, topology, weights, loss_out=None, grad_out=None, grad_scale=None, accumulate=False, want_grad=True):
    """d3m_mesh_regularizer on vertices [B,V,3] (f32, contiguous, on the topology's device): returns (loss [B], gradient
    [B,V,3] or None).  loss_out / grad_out: where to write (allocated when None); accumulate: add to them instead;
    grad_scale [B]: a device factor of the gradient.  No host synchronisation."""
    T = topology
    vertices = vertices.contiguous()
    B = vertices.shape[0]
    if loss_out is None:
        loss_out = torch.empty(B, dtype=torch.float32, device=vertices.device)
    if grad_out is None and want_grad:
        grad_out = torch.empty_like(vertices)
    L = _lib.lib()
    n = L.d3m_mesh_regularizer_scratch_floats(B, ctypes.byref(T.c))
    scratch = torch.empty(max(int(n), 1), dtype=torch.float32, device=vertices.device)
    lap, edge, edge_target, normal = weights
    _lib.check(L.d3m_mesh_regularizer(_lib.ptr(vertices), B, ctypes.byref(T.c), lap, edge, edge_target, normal,
                                      _lib.ptr(scratch), scratch.numel(), _lib.ptr(grad_scale), _lib.ptr(loss_out),
                                      _lib.ptr(grad_out) if want_grad else None, int(bool(accumulate)), _lib.stream_ptr()),
               "d3m_mesh_regularizer")
    return loss_out, (grad_out if want_grad else None)


class _MeshRegularizer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vertices, topology, weights, batched):
        x = (vertices if batched else vertices[None]).contiguous()
        loss, _ = evaluate(x, topology, weights, want_grad=False)
        ctx.save_for_backward(x)
        ctx.topology, ctx.weights, ctx.batched = topology, weights, batched
        return loss if batched else loss[0]

    @staticmethod
    def backward(ctx, grad_loss):
        (x,) = ctx.saved_tensors
        scale = grad_loss.reshape(-1).to(torch.float32).contiguous()        # stays on the device
        _, grad = evaluate(x, ctx.topology, ctx.weights, grad_scale=scale)
        return (grad if ctx.batched else grad[0]), None, None, None


def _checked_vertices(vertices, faces):
    if not torch.is_tensor(vertices) or vertices.dim() not in (2, 3) or vertices.shape[-1] != 3 or vertices.shape[-2] < 1:
        raise ValueError("vertices must be [num_vertices, 3] or [B, num_vertices, 3]")
    if vertices.dtype != torch.float32:
        raise ValueError("vertices must be float32")
    faces = _checked_faces(faces)
    if vertices.dim() == 3 and not 1 <= vertices.shape[0] <= 65535:
        raise ValueError("1 to 65535 vertex sets per call")
    if not vertices.is_cuda or faces.device != vertices.device:
        raise ValueError("vertices and faces must be on one GPU device")
    return faces


def mesh_regularizer(vertices, faces, laplacian=0., edge=0., edge_target=0., normal=0., cache=None):
    """laplacian * L_lap + edge * L_edge + normal * L_nc of a mesh (the module text), differentiable with respect to
    `vertices`: one autograd node, value and gradient by d3m_mesh_regularizer in a fixed order.

    vertices [V,3] or [B,V,3] f32 on the device (every set on its own); faces [F,3] or [1,F,3] int32 / int64 on the same
    device, a constant.  Returns a 0-d tensor for [V,3], [B] for [B,V,3].  A term of weight 0 is not evaluated.  The first
    call with a faces tensor builds its topology (outside any stream capture; ValueError for an index outside [0, V) or an
    edge of more than 16 faces) and later calls reuse it; `cache`: the TopologyCache to keep it in (default: the module's)."""
    weights = _checked_weights(laplacian, edge, edge_target, normal)
    faces = _checked_vertices(vertices, faces)
    topology = mesh_topology(faces, vertices.shape[-2], cache)
    return _MeshRegularizer.apply(vertices, topology, weights, vertices.dim() == 3)


def laplacian_loss(vertices, faces, cache=None):
    """L_lap: the mean squared distance of a vertex from the mean of its neighbours."""
    return mesh_regularizer(vertices, faces, laplacian=1.0, cache=cache)


def edge_length_loss(vertices, faces, edge_target=0., cache=None):
    """L_edge: the mean squared deviation of the unique edges' lengths from edge_target."""
    return mesh_regularizer(vertices, faces, edge=1.0, edge_target=edge_target, cache=cache)


def normal_consistency_loss(vertices, faces, cache=None):
    """L_nc: the mean of 1 - cos between the normals of two faces across an edge (winding does not matter)."""
    return mesh_regularizer(vertices, faces, normal=1.0, cache=cache)


class MeshRegularizer(nn.Module):
    """The regulariser of one mesh: `faces` [F,3] (buffer) and the weights; forward(vertices) returns the weighted sum.  The
    module keeps the topology of its faces itself, so whatever holds the module (a captured step) keeps the topology."""

    def __init__(self, faces, laplacian=0., edge=0., edge_target=0., normal=0.):
        super().__init__()
        faces = _checked_faces(torch.as_tensor(faces))
        self.laplacian, self.edge, self.edge_target, self.normal = _checked_weights(laplacian, edge, edge_target, normal)
        self.register_buffer("faces", faces.detach().reshape(-1, 3).contiguous().clone())
        self._topology = TopologyCache(1)

    @property
    def weights(self):
        return dict(laplacian=self.laplacian, edge=self.edge, edge_target=self.edge_target, normal=self.normal)

    def forward(self, vertices):
        return mesh_regularizer(vertices, self.faces, cache=self._topology, **self.weights)
