"""Analytic edge antialiasing of an image drawn over a coverage record, with the SILHOUETTE gradient: the fourth stage of
the coverage-record family (rasterize_fragments makes the record, interpolate_vertex_attributes / sample_uv_texture draw over
it, fragment_weights and screen_vertices= give the interior geometry gradient).

`antialias` blends the two pixels on either side of a silhouette edge by how far the edge sits between their centres.  For
every pair of 4-neighbours p, q owned by different triangles: n is the nearer covered pixel, o the other; the exit edge is the
side of n's triangle that the segment from n's centre to o's leaves through first, at parameter t in [0, 1); the edge counts
when it is a silhouette -- a boundary side, or a side whose one neighbouring triangle folds back onto the same side of it
(`side_opposite`) --; then t > 1/2 adds (t - 1/2)(c(n) - c(o)) to o and t < 1/2 adds (1/2 - t)(c(o) - c(n)) to n.  An interior
edge, a side shared by three or more triangles, a triangle that repeats an index, and a pair whose far pixel lies inside the
near triangle (two surfaces intersecting) leave both pixels alone.  csrc/d3m_antialias.h states every step and the order of
every sum: gathers in a fixed order, no float atomics, nothing cleared, the same bits on every run.

Image values near the outline thereby become continuous functions of the vertex positions, and the node is differentiable in
the image and in the screen vertices (x and y; the z gradient is an exact +0).  What is NOT differentiated: the choices -- which
pixel is the near one, which side is the exit edge, which pixel receives the blend; only t is.  Interior gradients
(screen_vertices= of the drawing nodes) and this one add in autograd."""
import ctypes

import torch

from .. import _lib
from .attributes import MAX_CHANNELS, _checked_fragments, _checked_screen_vertices
from .built_cache import BuiltCache, tensor_key
from .row_gather import vertex_adjacency

SIDE_BOUNDARY = -1      # side_opposite: only this triangle has the side (always a silhouette)
SIDE_IGNORED = -2       # side_opposite: three or more triangles share the side, or the triangle repeats an index


def build_side_opposite(faces, num_vertices):
    """side_opposite [F,3] i32 of faces [F,3] or [1,F,3] (any integer dtype, any device; indices in [0, num_vertices)), with
    torch operators: for side j of triangle f (corner j to corner (j + 1) mod 3) the third vertex of the other triangle when
    exactly two proper triangles (three distinct indices) share the undirected edge, SIDE_BOUNDARY when only this one has
    it, SIDE_IGNORED when three or more share it or when triangle f repeats an index."""
    tri = faces.reshape(-1, 3).long()
    V = int(num_vertices)
    a, c, third = tri, tri.roll(-1, 1), tri.roll(-2, 1)
    proper = (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])
    key = (torch.minimum(a, c) * V + torch.maximum(a, c)).reshape(-1)
    out = torch.full((tri.shape[0] * 3,), SIDE_IGNORED, dtype=torch.int64, device=tri.device)
    sides = torch.nonzero(proper[:, None].expand(-1, 3).reshape(-1)).flatten()        # the sides of proper triangles
    _, group, counts = torch.unique(key[sides], return_inverse=True, return_counts=True)
    shared_by = counts[group]
    out[sides[shared_by == 1]] = SIDE_BOUNDARY
    two = sides[shared_by == 2]
    two = two[torch.argsort(group[shared_by == 2], stable=True)]                      # the two sides of an edge, adjacent
    out[two] = third.reshape(-1)[two.view(-1, 2).flip(1).reshape(-1)]
    return out.view(-1, 3).to(torch.int32).contiguous()


class SideOppositeCache(BuiltCache):
    """BuiltCache for antialias' side tables: an entry also holds the caller's faces tensor."""
    what = "the silhouette side table (antialias)"


_cache = SideOppositeCache()


def side_opposite(faces, num_vertices, cache=None):
    """The cached build_side_opposite of a faces tensor (built on the first call with this tensor at its current version,
    outside any stream capture); `cache`: the SideOppositeCache to keep it in (default: the module's)."""
    cache = _cache if cache is None else cache
    return cache.get(tensor_key(faces) + (int(num_vertices),), lambda: build_side_opposite(faces, num_vertices),
                     holders=(faces,))


def _forward_launch(fr, images, sv, side):
    out = torch.empty_like(images)
    c_fr = fr.c_struct()
    _lib.check(_lib.lib().d3m_antialias_images(ctypes.byref(c_fr), _lib.ptr(images), images.shape[1], _lib.ptr(sv),
                                               int(fr.num_vertices), _lib.ptr(side), _lib.ptr(out), _lib.stream_ptr()),
               "d3m_antialias_images")
    return out


class _Antialias(torch.autograd.Function):
    @staticmethod
    def forward(ctx, images, screen_vertices, fragments, adjacency, side):
        img, sv = images.contiguous(), screen_vertices.detach().contiguous()
        ctx.save_for_backward(img, sv)
        ctx.fragments, ctx.adjacency, ctx.side = fragments, adjacency, side
        return _forward_launch(fragments, img, sv, side)

    @staticmethod
    def backward(ctx, grad_out):
        fr, A, side = ctx.fragments, ctx.adjacency, ctx.side
        img, sv = ctx.saved_tensors
        L = _lib.lib()
        B, S, V = img.shape[0], fr.raster_size, int(fr.num_vertices)
        g = grad_out.to(torch.float32).contiguous()
        grad_images = torch.empty_like(img) if ctx.needs_input_grad[0] else None
        pair_grads = scratch = None
        if ctx.needs_input_grad[1]:
            n = int(L.d3m_antialias_scratch_floats(B, fr.faces.shape[1], S, ctypes.byref(A.csr.c), 1))
            buf = torch.empty(n, dtype=torch.float32, device=img.device)      # (pair_grads and the adjoint's scratch: one buffer)
            pair_grads, scratch = buf[:B * S * S * 4], buf[B * S * S * 4:]
        c_fr = fr.c_struct()
        _lib.check(L.d3m_antialias_images_backward(ctypes.byref(c_fr), _lib.ptr(img), img.shape[1], _lib.ptr(sv), V,
                                                   _lib.ptr(side), _lib.ptr(g), _lib.ptr(grad_images), _lib.ptr(pair_grads),
                                                   _lib.stream_ptr()), "d3m_antialias_images_backward")
        grad_sv = None
        if pair_grads is not None:
            grad_sv = torch.empty(B, V, 3, dtype=torch.float32, device=img.device)
            _lib.check(L.d3m_antialias_geometry_backward(ctypes.byref(c_fr), _lib.ptr(pair_grads), ctypes.byref(A.csr.c),
                                                         _lib.ptr(scratch), scratch.numel(), _lib.ptr(grad_sv), V,
                                                         _lib.stream_ptr()), "d3m_antialias_geometry_backward")
        return grad_images, grad_sv, None, None, None


def antialias(images, fragments, screen_vertices, cache=None):
    """images_aa [B,C,s,s] of images [B,C,s,s] (f32 on the record's device, the nodes' output orientation: row 0 = top; 1 <=
    C <= 1024 -- what interpolate_vertex_attributes / sample_uv_texture return, their alpha concatenated as one more channel
    when an antialiased silhouette is wanted) over a Fragments record made WITHOUT anti-aliasing (a supersampled record is
    refused: its 2x2 pooling already does this job) and screen_vertices [B,V,3] f32, THE vertices the record was rasterised
    from (their values cannot be checked; shape, dtype, device and V are).  The module's docstring states the function.

    Differentiable in `images` and in `screen_vertices` (x and y; the z gradient is an exact +0, and so is the gradient of a
    vertex on no silhouette edge); the choices of near pixel, edge and recipient are constants.  One launch forward; backward
    one launch for the image gradient and the per-pair dL/dt, and, when the vertices require grad, three more (four on a
    mesh with hub vertices) for the fixed-order gather to the vertices.  Without requires_grad on either input the call is
    the forward launch only.

    The first call with the record's tri builds the silhouette side table and the faces' adjacency (outside any stream
    capture; inside one a missing table raises RuntimeError); `cache`: the SideOppositeCache to keep the table in (default:
    the module's; the adjacency lives in row_gather's).  ValueError, before anything is launched, for a malformed or
    supersampled record or a wrong rank, dtype, device, size, C, batch or V."""
    B, Ft, Fp = _checked_fragments(fragments)
    if fragments.anti_aliasing:
        raise ValueError("antialias: the fragments were made with anti_aliasing=True; their 2x2 pooling already antialiases -- "
                         "make the record with anti_aliasing=False")
    s = int(fragments.image_size)
    if not torch.is_tensor(images) or images.dim() != 4:
        raise ValueError("antialias: images must be [B, C, image_size, image_size]")
    if images.dtype != torch.float32:
        raise ValueError("antialias: images must be float32")
    if not 1 <= images.shape[1] <= MAX_CHANNELS:
        raise ValueError(f"antialias: images: 1 to {MAX_CHANNELS} channels")
    if images.shape[0] != B or tuple(images.shape[2:]) != (s, s):
        raise ValueError(f"antialias: images must be [{B}, C, {s}, {s}] for these fragments")
    if images.device != fragments.face_index_map.device:
        raise ValueError("antialias: images must be on the fragments' device")
    _checked_screen_vertices(screen_vertices, fragments, "antialias")
    V = int(fragments.num_vertices)
    adjacency = vertex_adjacency(fragments.tri, V)                  # (where tri's indices are checked against V)
    side = side_opposite(fragments.tri, V, cache)
    if not images.is_cuda:
        raise ValueError("antialias: images and fragments must be on one GPU device")
    if torch.is_grad_enabled() and (images.requires_grad or screen_vertices.requires_grad):
        return _Antialias.apply(images, screen_vertices, fragments, adjacency, side)
    return _forward_launch(fragments, images.contiguous(), screen_vertices.detach().contiguous(), side)
