"""Per-pixel spherical-harmonic shading of a UV albedo texture: the albedo image [H,W,3] looked up bilinearly at every internal
pixel of a coverage record (uv_texture_images.py) times the 9-term light of the per-pixel normalised interpolated normal
(sh_fragments.py) -- the picture model of face reconstruction, UV albedo times SH of the surface normal, as ONE node of the
fragment family.

For internal pixel p of view b with owner fn, with shade_fragments' m, r, n, s_k and sample_uv_texture's four taps and weights:

    a_k = sum_j image[tap_j][k] * w_j        value_k = a_k s_k

An uncovered pixel takes the background; the image is that map with its rows reversed and, with anti-aliasing, 2x2-averaged
AFTER the product.  That is what multiplying shade_fragments' picture with sample_uv_texture's cannot give on a supersampled
record: both pool after their own evaluation, the product of two pooled images is not the pooled product, and at a silhouette
the two backgrounds are averaged separately and then multiplied.  csrc/d3m_sh_uv_fragments.h states the function and the order
of every sum; it calls the device functions of the two nodes it joins and restates none.

The adjoint recomputes everything per covered internal pixel in one launch and leaves what is wanted: the light's partial sums
(the tree of csrc/d3m_set_sums.h, as in shade_fragments), dL/dm as a gradient image for the attribute adjoint's own gather
kernels (normals), dL/da as a second gradient image for sample_uv_texture's own order-independent fixed-point scatter (image),
and dL/du for the shared interior geometry adjoint (screen vertices).  No float atomics, nothing assumed of the scratch, the
same bits on every run; forward and backward capture.

LAUNCHES.  Forward 1 (k_sh_uv_fragment_images).  Backward: 1 per-pixel launch (k_sh_uv_fragment_backward_pixels), + 1 when sh
requires grad (k_sh_fragment_finish), + 3 when normals require grad (4 on a mesh with hub vertices: the long-row chunks), + 3
when the image requires grad (clear and maxima, scatter, convert), + the shared geometry adjoint's 3 (4 with hubs) when
screen_vertices require grad.  Only what is wanted is written and gathered.

NOT OFFERED.  mipmap: the level of detail depends on the geometry, and this node carries the geometry gradient.  Per-vertex
colors together with an image: multiply the albedo into the image, or use shade_fragments."""
import ctypes

import torch

from .. import _lib
from .attributes import (_checked_background, _checked_screen_vertices, _geometry_adjoint, _geometry_scratch,
                         _node_geometry_adjoint)
from .row_gather import vertex_adjacency
from .sh_fragments import _batch_of, _checked_per_vertex, _checked_sh
from .uv_texture_images import _checked_uv_image


class _ShadeUvTexture(torch.autograd.Function):
    """screen_vertices may be None.  The backward keeps the inputs only (nothing of the forward's arithmetic)."""
    @staticmethod
    def forward(ctx, image, normals, sh, screen_vertices, faces_uv, fragments, adjacency, wrapping, background):
        img, n, s = image.contiguous(), normals.contiguous(), sh.contiguous()
        B, size, V = fragments.face_index_map.shape[0], int(fragments.image_size), n.shape[-2]
        images = torch.empty(B, 3, size, size, dtype=torch.float32, device=n.device)
        alpha = torch.empty(B, size, size, dtype=torch.float32, device=n.device)
        ctx.fragments, ctx.adjacency, ctx.faces_uv, ctx.wrapping = fragments, adjacency, faces_uv, wrapping
        c_fr = fragments.c_struct()
        _lib.check(_lib.lib().d3m_sh_uv_fragment_images(ctypes.byref(c_fr), *_ShadeUvTexture._args(ctx, n, s, img),
                                                        _lib.ptr(background), _lib.ptr(images), _lib.ptr(alpha),
                                                        _lib.stream_ptr()), "d3m_sh_uv_fragment_images")
        ctx.save_for_backward(img, n, s)
        ctx.mark_non_differentiable(alpha)
        return images, alpha

    @staticmethod
    def _args(ctx, n, s, img):
        """the C entry points' (normals, nb, sh, sb, V, faces_uv, image, ib, H, W, wrapping) of contiguous tensors"""
        H, W = img.shape[-3:-1]
        return (_lib.ptr(n), _batch_of(n), _lib.ptr(s), _batch_of(s), n.shape[-2], _lib.ptr(ctx.faces_uv), _lib.ptr(img),
                img.shape[0] if img.dim() == 4 else 1, H, W, ctx.wrapping)

    @staticmethod
    def backward(ctx, grad_images, _grad_alpha):
        fr, A = ctx.fragments, ctx.adjacency
        img, n, s = ctx.saved_tensors
        need_img, need_n, need_sh, need_sv = ctx.needs_input_grad[:4]
        L = _lib.lib()
        g = grad_images.to(torch.float32).contiguous()
        B, Fp, dev = fr.face_index_map.shape[0], fr.faces.shape[1], g.device
        args = _ShadeUvTexture._args(ctx, n, s, img)
        grad_img = grad_n = grad_sh = grad_sv = None
        if not (need_img or need_n or need_sh):
            if need_sv:                                               # the vertices alone: the node's pixel_grads, nothing else
                grad_sv = _node_geometry_adjoint(fr, A, lambda c_fr, h: _lib.check(L.d3m_sh_uv_fragment_pixel_grads(
                    c_fr, *args, _lib.ptr(g), h, _lib.stream_ptr()), "d3m_sh_uv_fragment_pixel_grads"))
            return None, None, None, grad_sv, None, None, None, None, None
        n_bytes = int(L.d3m_sh_uv_fragment_scratch_bytes(B, Fp, fr.raster_size, args[7], args[8], args[9], ctypes.byref(A.csr.c)))
        scratch = torch.empty((n_bytes + 7) // 8, dtype=torch.int64, device=dev)
        if need_img:
            grad_img = torch.empty(img.shape, dtype=torch.float32, device=dev)
        if need_n:
            grad_n = torch.empty(n.shape, dtype=torch.float32, device=dev)
        if need_sh:
            grad_sh = torch.empty(s.shape, dtype=torch.float32, device=dev)
        # the vertices' pixel_grads come out of the same per-pixel launch
        h, geometry_scratch = _geometry_scratch(fr, A, True) if need_sv else (None, None)
        c_fr = fr.c_struct()
        _lib.check(L.d3m_sh_uv_fragment_images_backward(ctypes.byref(c_fr), *args, _lib.ptr(g), ctypes.byref(A.csr.c),
                                                        _lib.ptr(scratch), scratch.numel() * 8, _lib.ptr(grad_n),
                                                        _lib.ptr(grad_sh), _lib.ptr(grad_img), _lib.ptr(h),
                                                        _lib.stream_ptr()), "d3m_sh_uv_fragment_images_backward")
        if need_sv:
            grad_sv = _geometry_adjoint(fr, A, h, geometry_scratch)
        return grad_img, grad_n, grad_sh, grad_sv, None, None, None, None, None


def shade_uv_texture(image, faces_uv, normals, sh, fragments, texture_wrapping='REPEAT', background=None, cache=None,
                     screen_vertices=None):
    """(images [B,3,s,s], alpha [B,s,s]): the albedo `image` f32 [H,W,3] (shared by the views) or [B,H,W,3], in the texture
    space of sample_uv_texture, looked up at every internal pixel of the Fragments record through faces_uv [F,3,2] (a constant,
    wrapped per corner by texture_wrapping 'REPEAT', 'MIRRORED_REPEAT' or 'CLAMP_TO_EDGE'; CLAMP_TO_BORDER is refused) and
    multiplied THERE with the light of shade_fragments: per-vertex `normals` f32 [V,3] or [B,V,3] interpolated and normalised
    per pixel, lit by `sh` f32 [3,9] or [B,3,9].  background: None (zeros), a float or [3]; an uncovered pixel takes it.  With
    a supersampled record the product is formed at every internal pixel and then pooled 2x2.

    One autograd node, differentiable in image, normals and sh; alpha has the bits of interpolate_vertex_attributes' alpha and
    is not differentiable.  The normals' and the light's gradients have a fixed order, the image's is a 64-bit fixed-point
    sum that is independent of order (sample_uv_texture's rules: an all-zero image gradient gives an exact +0, an Inf or NaN
    in it makes every element NaN, a texel that no pixel reaches gets +0); no float atomics (the module docstring counts the
    launches).  `cache`: the AdjacencyCache of interpolate_vertex_attributes.  screen_vertices: as in shade_fragments -- THE
    vertices [B,V,3] the record was rasterised from, still attached to the graph, get the INTERIOR geometry gradient through
    the shared adjoint of csrc/d3m_fragment_geometry.h (the normals' mix and the lookup's slope along the position); coverage
    and faces_uv stay constants.

    Not offered: mipmap (the level of detail depends on the geometry, and the node carries the geometry gradient) and
    per-vertex colors together with an image.  faces_uv that requires grad raises NotImplementedError.  ValueError /
    TypeError, before the device is touched, for a wrong rank, dtype, device, a channel count other than 3, F, V, batch,
    wrapping, a background that requires grad, B S S beyond 2^32, H or W beyond 32768."""
    B, Ft, H, W, C, wrapping = _checked_uv_image(image, faces_uv, texture_wrapping, fragments, "shade_uv_texture", channels=3)
    V, device = fragments.num_vertices, fragments.face_index_map.device
    _checked_per_vertex(normals, "normals", B, V, device)
    _checked_sh(sh, B, device)
    if screen_vertices is not None:
        _checked_screen_vertices(screen_vertices, fragments, "shade_uv_texture")
    background = _checked_background(background, 3, image)
    adjacency = vertex_adjacency(fragments.tri, V, cache)          # (where tri's indices are checked against V)
    if not image.is_cuda:
        raise ValueError("image and fragments must be on one GPU device")
    return _ShadeUvTexture.apply(image, normals, sh, screen_vertices, faces_uv.detach().contiguous(), fragments, adjacency,
                                 wrapping, background)
