"""Per-pixel spherical-harmonic shading of fragment images: per-vertex normals (and, optionally, per-vertex albedo) interpolated
over a coverage record, the normal normalised PER PIXEL and lit by the 9-term light of smooth_shading.py -- the picture model
albedo times SH of the surface normal, as one node of the fragment family (attributes.py, uv_texture_images.py, antialias.py).

For internal pixel p of view b with owner fn, corner vertices v_c and weights u_c = weight_map[p,c] * (depth_map[p] / z_c):

    m   = (u_0 n_0 + u_1 n_1) + u_2 n_2        r = sqrt((m_x^2 + m_y^2) + m_z^2)        n = m / max(r, 1e-6)
    s_k = sum_j sh[b,k,j] H_j(n)               (H: sh_basis; j ascending; no clamp, no ReLU)
    a   = (u_0 c_0 + u_1 c_1) + u_2 c_2        value_k = a_k s_k                        (colors=None: value_k = s_k)

An uncovered pixel takes the background; the image is that map with its rows reversed and, with anti-aliasing, 2x2-averaged --
the shading is evaluated at every internal pixel BEFORE the pooling.  The normal is not flipped for a pixel a fill_back copy
owns (sh_vertex_colors does not flip either).  csrc/d3m_sh_fragments.h states the function and the order of every sum: the 27
sums of the light's gradient per view through the tree of csrc/d3m_set_sums.h (a set is a view, an element an internal pixel,
1024 pixels per part, at most 256 parts), the normals' and colours' gradients through the attribute adjoint's own gather
kernels over a per-pixel gradient image at the internal size, shared inputs summed over the views in ascending order.  No
float atomics, nothing cleared, the same bits on every run; forward and backward capture.

LAUNCHES.  Forward 1 (k_sh_fragment_images).  Backward: 1 per-pixel launch (k_sh_fragment_backward_pixels: recomputes m, n, H
from the record and the inputs, writes the per-pixel gradients of whatever requires grad -- normals, colors, screen_vertices --
and the light's partial sums), + 1 when sh requires grad (k_sh_fragment_finish), + a gather when normals or colors require
grad: 3 launches (the attribute adjoint's two face-sum kernels and its rows), 4 on a mesh with hub vertices (the long-row
chunks); only the gradient that is wanted is gathered, and normals AND colors whose batches differ ([V,3] with [B,V,3]) take a
gather each.  So 5 (6 with hubs) when normals, colors and sh require grad, 2 for the light alone.  screen_vertices that
require grad add the shared geometry adjoint's 3 (4 with hubs), nothing else."""
import ctypes

import torch

from .. import _lib
from .attributes import (_checked_background, _checked_fragments, _checked_pixel_lanes, _checked_screen_vertices,
                         _geometry_adjoint, _geometry_scratch, _node_geometry_adjoint)
from .row_gather import vertex_adjacency


def _batch_of(t):
    return t.shape[0] if t.dim() == 3 else 1


def _args(normals, sh, colors):
    """the C entry points' (normals, nb, sh, sb, colors, cb) of contiguous tensors"""
    return (_lib.ptr(normals), _batch_of(normals), _lib.ptr(sh), _batch_of(sh), _lib.ptr(colors),
            1 if colors is None else _batch_of(colors))


class _ShadeFragments(torch.autograd.Function):
    """colors and screen_vertices may be None.  The backward keeps the inputs only (nothing of the forward's arithmetic)."""
    @staticmethod
    def forward(ctx, normals, sh, colors, screen_vertices, fragments, adjacency, background):
        n, s = normals.contiguous(), sh.contiguous()
        c = None if colors is None else colors.contiguous()
        B, size, V = fragments.face_index_map.shape[0], int(fragments.image_size), n.shape[-2]
        images = torch.empty(B, 3, size, size, dtype=torch.float32, device=n.device)
        alpha = torch.empty(B, size, size, dtype=torch.float32, device=n.device)
        c_fr = fragments.c_struct()
        _lib.check(_lib.lib().d3m_sh_fragment_images(ctypes.byref(c_fr), *_args(n, s, c), V, _lib.ptr(background),
                                                     _lib.ptr(images), _lib.ptr(alpha), _lib.stream_ptr()),
                   "d3m_sh_fragment_images")
        ctx.save_for_backward(n, s, c)
        ctx.fragments, ctx.adjacency = fragments, adjacency
        ctx.mark_non_differentiable(alpha)
        return images, alpha

    @staticmethod
    def backward(ctx, grad_images, _grad_alpha):
        fr, A = ctx.fragments, ctx.adjacency
        n, s, c = ctx.saved_tensors
        need_n, need_sh, need_c, need_sv = ctx.needs_input_grad[:4]
        need_c = need_c and c is not None
        L = _lib.lib()
        g = grad_images.to(torch.float32).contiguous()
        B, V, Fp, dev = fr.face_index_map.shape[0], n.shape[-2], fr.faces.shape[1], g.device
        args = _args(n, s, c)
        grad_n = grad_c = grad_sh = grad_sv = None
        if not (need_n or need_c or need_sh):
            if need_sv:                                               # the vertices alone: the node's pixel_grads, nothing else
                grad_sv = _node_geometry_adjoint(fr, A, lambda c_fr, h: _lib.check(L.d3m_sh_fragment_pixel_grads(
                    c_fr, *args, V, _lib.ptr(g), h, _lib.stream_ptr()), "d3m_sh_fragment_pixel_grads"))
            return None, None, None, grad_sv, None, None, None
        n_scratch = int(L.d3m_sh_fragment_scratch_floats(B, Fp, fr.raster_size, int(c is not None), ctypes.byref(A.csr.c)))
        scratch = torch.empty(n_scratch, dtype=torch.float32, device=dev)
        grad_v = None
        if need_n and need_c and _batch_of(c) == _batch_of(n):        # one gather of six channels
            grad_v = torch.empty(n.shape[:-1] + (6,), dtype=torch.float32, device=dev)
            grad_n, grad_c = grad_v[..., :3], grad_v[..., 3:]
        elif need_n or need_c:                                        # what is wanted, the normals' first
            sizes = [t.numel() if need else 0 for t, need in ((n, need_n), (c, need_c))]
            grad_v = torch.empty(sum(sizes), dtype=torch.float32, device=dev)
            grad_n = grad_v[:sizes[0]].view(n.shape) if need_n else None
            grad_c = grad_v[sizes[0]:].view(c.shape) if need_c else None
        if need_sh:
            grad_sh = torch.empty(s.shape, dtype=torch.float32, device=dev)
        # the vertices' pixel_grads come out of the same per-pixel launch
        h, geometry_scratch = _geometry_scratch(fr, A, True) if need_sv else (None, None)
        c_fr = fr.c_struct()
        _lib.check(L.d3m_sh_fragment_images_backward(ctypes.byref(c_fr), *args, V, _lib.ptr(g), ctypes.byref(A.csr.c),
                                                     _lib.ptr(scratch), n_scratch, _lib.ptr(grad_v),
                                                     int(need_n) + 2 * int(need_c), _lib.ptr(grad_sh), _lib.ptr(h),
                                                     _lib.stream_ptr()), "d3m_sh_fragment_images_backward")
        if need_sv:
            grad_sv = _geometry_adjoint(fr, A, h, geometry_scratch)
        return grad_n, grad_sh, grad_c, grad_sv, None, None, None


def _checked_per_vertex(t, name, B, V, device):
    if not torch.is_tensor(t) or t.dim() not in (2, 3) or t.shape[-1] != 3:
        raise ValueError(f"{name} must be [num_vertices, 3] or [B, num_vertices, 3]")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32")
    if t.shape[-2] != V:
        raise ValueError(f"{name} have {t.shape[-2]} vertices, the fragments were rasterised from {V}")
    if t.dim() == 3 and t.shape[0] != B:
        raise ValueError(f"{name} must be [V, 3] or [{B}, V, 3] for fragments of {B} views")
    if t.device != device:
        raise ValueError(f"{name} must be on the fragments' device")


def _checked_sh(sh, B, device):
    """The 9-term light of the per-pixel shading nodes: f32 [3,9] or [B,3,9] on the record's device."""
    if not torch.is_tensor(sh) or sh.dim() not in (2, 3) or tuple(sh.shape[-2:]) != (3, 9):
        raise ValueError("sh must be [3, 9] or [B, 3, 9]")
    if sh.dtype != torch.float32:
        raise ValueError("sh must be float32")
    if sh.dim() == 3 and sh.shape[0] != B:
        raise ValueError(f"sh must be [3, 9] or [{B}, 3, 9] for fragments of {B} views")
    if sh.device != device:
        raise ValueError("sh must be on the fragments' device")


def shade_fragments(normals, sh, fragments, colors=None, background=None, cache=None, screen_vertices=None):
    """(images [B,3,s,s], alpha [B,s,s]): per-vertex `normals` f32 [V,3] (shared by the views) or [B,V,3] -- one per vertex
    of the record's topology, any length, in whatever frame the light lives in -- interpolated over the Fragments record,
    normalised per pixel and lit by `sh` f32 [3,9] or [B,3,9] (channel, basis term: sh_vertex_colors' layout, SH_A's
    constants); `colors` None or per-vertex albedo f32 [V,3] / [B,V,3] interpolated alike and multiplied in.  background: None
    (zeros), a float or [3], as interpolate_vertex_attributes takes it; an uncovered pixel takes it.  With a supersampled
    record the shading is evaluated at every internal pixel and then pooled 2x2.  A caller who fits a uv albedo calls
    shade_uv_texture (sh_uv_fragments.py), which multiplies the looked-up albedo in at every internal pixel: this node's picture
    times sample_uv_texture's is that product only without supersampling and away from the silhouette.

    One autograd node, differentiable in normals, sh and colors; alpha has the bits of interpolate_vertex_attributes' alpha
    and is not differentiable.  Every sum of the backward has a fixed order, no float atomics are used, nothing is cleared
    (the module docstring counts the launches); the gradient of an input without B is summed over the views in ascending
    order.  `cache`: the AdjacencyCache of interpolate_vertex_attributes.  screen_vertices: as in
    interpolate_vertex_attributes -- THE vertices [B,V,3] the record was rasterised from, still attached to the graph, get
    the INTERIOR geometry gradient through the shared adjoint of csrc/d3m_fragment_geometry.h; coverage stays a constant;
    vertices that do not require grad launch nothing extra.  ValueError, before the device is touched, for a wrong dtype,
    rank, V, batch or device, and for a background that requires grad; 1 <= B <= 65535."""
    B, Ft, Fp = _checked_fragments(fragments)
    V, device = fragments.num_vertices, fragments.face_index_map.device
    _checked_per_vertex(normals, "normals", B, V, device)
    _checked_sh(sh, B, device)
    if colors is not None:
        _checked_per_vertex(colors, "colors", B, V, device)
    if screen_vertices is not None:
        _checked_screen_vertices(screen_vertices, fragments, "shade_fragments")
    _checked_pixel_lanes(fragments, "shade_fragments")
    background = _checked_background(background, 3, normals)
    adjacency = vertex_adjacency(fragments.tri, V, cache)          # (where tri's indices are checked against V)
    if not normals.is_cuda:
        raise ValueError("normals and fragments must be on one GPU device")
    return _ShadeFragments.apply(normals, sh, colors, screen_vertices, fragments, adjacency, background)
