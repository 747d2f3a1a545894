"""The interior geometry gradient of what is drawn over a coverage record: the derivative of the perspective-correct weights
u_c of every owned pixel with respect to the owner's three screen-space corners.

For internal pixel p of view b with owner fn, corners (x_c, y_c, z_c) = screen_vertices[b, vertex(fn, c)] and centre (xp, yp):
b = M^-1 (xp, yp, 1)^T with M = [[x0,x1,x2],[y0,y1,y2],[1,1,1]], u_c = (b_c / z_c) / sum_k (b_k / z_k) -- what weight_map *
depth_map / z_c evaluates, with the rasteriser's clamp-and-renormalise of b taken as the identity.  `fragment_weights` returns
that map and is differentiable in the screen vertices; `interpolate_vertex_attributes(..., screen_vertices=)` and
`sample_uv_texture(..., screen_vertices=)` send their images' gradient through the same adjoint (csrc/d3m_fragment_geometry.h
states it and the order of every sum: per visible face over the pixels it owns, then per vertex over the faces' CSR adjacency;
no float atomics, nothing cleared, the same bits on every run).

What is NOT differentiated: coverage.  Which face owns which pixel is a constant of the graph, so nothing here sees a pixel
changing its owner or the silhouette moving: that gradient is render_silhouettes' / render's, or antialias' (antialias.py)
over the drawn image.  The caller passes the vertices
the record was rasterised from; only their shape, dtype, device and V can be checked."""
import ctypes

import torch

from .. import _lib
from .attributes import _checked_fragments, _checked_screen_vertices, _geometry_adjoint, _geometry_scratch
from .row_gather import vertex_adjacency


def _weights_launch(fr):
    B, S = fr.face_index_map.shape[0], fr.raster_size
    u = torch.empty(B, S, S, 3, dtype=torch.float32, device=fr.face_index_map.device)
    c_fr = fr.c_struct()
    _lib.check(_lib.lib().d3m_fragment_weights(ctypes.byref(c_fr), _lib.ptr(u), _lib.stream_ptr()), "d3m_fragment_weights")
    return u


class _FragmentWeights(torch.autograd.Function):
    @staticmethod
    def forward(ctx, screen_vertices, fragments, adjacency):
        ctx.fragments, ctx.adjacency = fragments, adjacency
        return _weights_launch(fragments)

    @staticmethod
    def backward(ctx, grad_u):
        fr, A = ctx.fragments, ctx.adjacency
        h = grad_u.to(torch.float32).contiguous()
        _, scratch = _geometry_scratch(fr, A, False)
        return _geometry_adjoint(fr, A, h, scratch), None, None


def fragment_weights(fragments, screen_vertices, cache=None):
    """u [B,S,S,3] of a Fragments record (S its raster size, the maps' orientation: row 0 = bottom): the perspective-correct
    weights weight_map * (depth_map / z_c) of every owned pixel, an exact 0 where uncovered.  Differentiable in
    screen_vertices [B,V,3] (f32, on the record's device, V = fragments.num_vertices): the vertices the record was rasterised
    from -- their values cannot be checked.  The backward is the shared interior adjoint with dL/du = the incoming gradient;
    coverage is a constant.  One launch forward; three backward, four on a mesh with hub vertices.  The first call with the
    record's tri builds the faces' adjacency (outside any stream capture); `cache`: the AdjacencyCache to keep it in.
    ValueError, before anything is launched, for a malformed record or a wrong rank, dtype, device or V."""
    _checked_fragments(fragments)
    _checked_screen_vertices(screen_vertices, fragments, "fragment_weights")
    adjacency = vertex_adjacency(fragments.tri, fragments.num_vertices, cache)
    if not screen_vertices.is_cuda:
        raise ValueError("screen_vertices and fragments must be on one GPU device")
    if screen_vertices.requires_grad and torch.is_grad_enabled():
        return _FragmentWeights.apply(screen_vertices, fragments, adjacency)
    return _weights_launch(fragments)
