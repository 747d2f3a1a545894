"""Learnable per-vertex colours: `textures_from_vertex_colors` (colours [V,3] of an indexed mesh -> per-face 2x2x2 texture
cubes, differentiable with respect to the colours) and `VertexColors` (the colours as a parameter).

The cube of a face is core.renderer_utils.vcolor_to_texture_cube of its three corner colours, evaluated by
d3m_vertex_color_textures in the association of get_textures_from_im (the same bits on an image's grid mesh).  On the
plane w0 + w1 + w2 = 1 its trilinear sample is the barycentric mix of the corner colours, so the render nodes draw smooth,
Gouraud-like colour through the sampler they have.

The adjoint is a gather over the CSR adjacency of the faces (a vertex's items 3 f + c in ascending order: what
d3m_vertex_gather walks), reduced by d3m_vertex_color_textures_backward in a fixed order -- no float atomics, the same bits
on every run.  A hub vertex (a fan apex, a pole) must not make one lane walk thousands of items: rows longer than LONG_ROW
items go through the chunked reduction that row_gather.py describes.  The adjacency is built once per (faces tensor,
version, V) with torch operators -- where the indices are checked against V -- and kept in row_gather's bounded LRU cache,
the one the deterministic mode's per-vertex gathers read theirs from."""
import ctypes

import torch
import torch.nn as nn

from .. import _lib
# (the adjacency, its cache and the constants stay importable from here)
from .row_gather import (CACHE_SIZE, CHUNK, LONG_ROW, Adjacency, AdjacencyCache, BuiltCache, Csr, _cache, _faces_key,  # noqa: F401
                         build_adjacency, build_csr, checked_faces as _checked_faces, csr_offsets, long_row_chunks, tensor_key,
                         vertex_adjacency)


def vertex_color_adjoint(adjacency, grad_textures):
    """grad_colors [B,V,3] of grad_textures [B,F,2,2,2,3] through the adjacency (d3m_vertex_color_textures_backward)."""
    A = adjacency
    g = grad_textures.to(torch.float32).contiguous()
    if g.dim() != 6 or tuple(g.shape[1:]) != (A.num_faces, 2, 2, 2, 3) or g.device != A.tri.device:
        raise ValueError(f"grad_textures must be [B, {A.num_faces}, 2, 2, 2, 3] on {A.tri.device}")
    B = g.shape[0]
    grad_colors = torch.empty(B, A.num_vertices, 3, dtype=torch.float32, device=g.device)
    partials = torch.empty(B, A.csr.num_chunks, 3, dtype=torch.float32, device=g.device) if A.csr.num_chunks else None
    _lib.check(_lib.lib().d3m_vertex_color_textures_backward(
        _lib.ptr(g), ctypes.byref(A.csr.c), _lib.ptr(partials), _lib.ptr(grad_colors), B, A.num_vertices, A.num_faces,
        _lib.stream_ptr()), "d3m_vertex_color_textures_backward")
    return grad_colors


class _VertexColorTextures(torch.autograd.Function):
    @staticmethod
    def forward(ctx, colors, adjacency, batched):
        cols = (colors if batched else colors[None]).contiguous()
        B, A = cols.shape[0], adjacency
        out = torch.empty(B, A.num_faces, 2, 2, 2, 3, dtype=torch.float32, device=cols.device)
        _lib.check(_lib.lib().d3m_vertex_color_textures(_lib.ptr(cols), B, _lib.ptr(A.tri), _lib.ptr(out), A.num_vertices,
                                                        A.num_faces, _lib.stream_ptr()), "d3m_vertex_color_textures")
        ctx.adjacency, ctx.batched = adjacency, batched
        return out

    @staticmethod
    def backward(ctx, grad_out):
        grad_colors = vertex_color_adjoint(ctx.adjacency, grad_out)
        return (grad_colors if ctx.batched else grad_colors[0]), None, None


def textures_from_vertex_colors(colors, faces, cache=None):
    """Per-face texture cubes of per-vertex colours, differentiable with respect to `colors`.

    colors [V,3] or [B,V,3] f32 on the device; faces [F,3] or [1,F,3] int32 / int64 on the same device, a constant.
    Returns [1,F,2,2,2,3] (or [B,F,2,2,2,3]): the cube of face f is vcolor_to_texture_cube of its corner colours, and
    rendering it draws the barycentric mix of the three colours.  The first call with a faces tensor builds its adjacency
    (outside any stream capture; a ValueError for an index outside [0, V)) and later calls reuse it; `cache`: the
    AdjacencyCache to keep it in (default: the module's)."""
    if not torch.is_tensor(colors) or colors.dim() not in (2, 3) or colors.shape[-1] != 3 or colors.shape[-2] < 1:
        raise ValueError("colors must be [num_vertices, 3] or [B, num_vertices, 3]")
    if colors.dtype != torch.float32:
        raise ValueError("colors must be float32")
    faces = _checked_faces(faces)
    batched = colors.dim() == 3
    if batched and not 1 <= colors.shape[0] <= 65535:
        raise ValueError("1 to 65535 colour sets per call")
    if not colors.is_cuda or faces.device != colors.device:
        raise ValueError("colors and faces must be on one GPU device")
    adjacency = vertex_adjacency(faces, colors.shape[-2], cache)
    return _VertexColorTextures.apply(colors, adjacency, batched)


class VertexColors(nn.Module):
    """The colours of a mesh's vertices as a learnable parameter: `colors` [V,3] (parameter), `faces` [F,3] (buffer);
    forward() returns the texture cubes [1,F,2,2,2,3].  The module keeps the adjacency of its faces itself, so whatever
    holds the module (a captured step) keeps the adjacency."""

    def __init__(self, colors, faces):
        super().__init__()
        colors = torch.as_tensor(colors)
        if colors.dim() != 2 or colors.shape[1] != 3 or colors.shape[0] < 1:
            raise ValueError("colors must be [num_vertices, 3]")
        faces = _checked_faces(torch.as_tensor(faces))
        self.colors = nn.Parameter(colors.detach().to(torch.float32).contiguous().clone())
        self.register_buffer("faces", faces.detach().reshape(-1, 3).contiguous().clone())
        self._adjacency = AdjacencyCache(1)

    @classmethod
    def from_textures(cls, textures, faces, num_vertices):
        """Colours read off texture cubes [F,ts,ts,ts,3] (or [1,F,...]; any ts >= 2, e.g. load_obj(load_texture=True)'s):
        a vertex's colour is the mean, over its incident faces, of the corner texel the cube gives that corner -- (ts-1,0,0),
        (0,ts-1,0), (0,0,ts-1) for slot 0, 1, 2; a vertex of no face gets 0.  A one-off in eager torch."""
        textures = torch.as_tensor(textures)
        faces = _checked_faces(torch.as_tensor(faces)).reshape(-1, 3)
        if textures.dim() == 6 and textures.shape[0] == 1:
            textures = textures[0]
        F, V = faces.shape[0], int(num_vertices)
        ts = textures.shape[1] if textures.dim() == 5 else 0
        if ts < 2 or tuple(textures.shape) != (F, ts, ts, ts, 3):
            raise ValueError(f"textures must be [{F}, ts, ts, ts, 3] with ts >= 2")
        flat = faces.reshape(-1).long().to(textures.device)
        if int(flat.min()) < 0 or int(flat.max()) >= V:
            raise ValueError(f"faces: vertex indices must be in [0, {V})")
        t = textures.detach().to(torch.float32)
        corners = torch.stack([t[:, ts - 1, 0, 0], t[:, 0, ts - 1, 0], t[:, 0, 0, ts - 1]], 1).reshape(-1, 3)
        total = torch.zeros(V, 3, dtype=torch.float32, device=t.device).index_add_(0, flat, corners)
        count = torch.bincount(flat, minlength=V).clamp(min=1).to(torch.float32)
        return cls(total / count[:, None], faces.to(t.device))

    def forward(self):
        return textures_from_vertex_colors(self.colors, self.faces, cache=self._adjacency)
