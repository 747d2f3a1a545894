"""Per-vertex attribute images: any C-channel per-vertex quantity (3D positions -- a UV position map --, PNCC codes, smooth
normals, uv coordinates, feature vectors) drawn as an image [B,C,s,s], differentiable with respect to the attributes.

`rasterize_fragments` runs coverage once and returns the record, `Fragments`: a constant of the graph (an attribute image
carries no geometry gradient).  `interpolate_vertex_attributes` reads a record and attributes [V,C] or [B,V,C]: internal
pixel p with owner fn takes (u_0 a_0 + u_1 a_1) + u_2 a_2 of the owner's corner attributes, u_c = weight_map[p,c] *
(depth_map[p] / z_c) the perspective-correct weights of the texture sampler, an uncovered pixel the background; the image is
that map with its rows reversed and, with anti-aliasing, 2x2-averaged -- what rasterize_rgbad makes of a map.  One launch.

The adjoint is a gather in a fixed order (csrc/d3m_attributes.h states it): per visible face the sums over the pixels it owns
(scan_owned_pixels; a workgroup for a face whose box exceeds 4096 pixels), stored plainly in a per-face scratch, then per
vertex over the CSR adjacency of the faces (row_gather.vertex_adjacency: the one textures_from_vertex_colors walks), hub
vertices through the long-row chunks.  No float atomics, nothing cleared, the same bits on every run.

The record stays a constant, but with `screen_vertices=` the node also returns the INTERIOR geometry gradient -- the
derivative of the weights u_c with respect to the owner's screen-space corners -- through the shared adjoint of
csrc/d3m_fragment_geometry.h (fragment_geometry.py); the helpers of that adjoint live here, next to the record."""
import ctypes
from typing import NamedTuple

import torch

from .. import _lib
from . import rasterize_ops as ops
from ._util import const_tensor
from .row_gather import checked_faces, vertex_adjacency

CHANNEL_CHUNK = 8       # VA_CHUNK of csrc/d3m_attributes.h: the channels a lane keeps in registers at a time
MAX_CHANNELS = 1024
MAX_VIEWS = 65535


class Fragments(NamedTuple):
    """A coverage record, a constant of the graph.  Maps in the internal order (row 0 = bottom) at the raster size S =
    image_size, or 2 image_size with anti-aliasing: face_index_map [B,S,S] i32 (-1: uncovered), weight_map [B,S,S,3],
    depth_map [B,S,S]; faces [B,F',3,3], the dense screen-space copy coverage leaves (only owners' entries are defined, only
    those are read); visibility, the finished d3m_visibility blob; tri [F,3] i32; fill_back (F' = 2 F), image_size (of the
    output), anti_aliasing; num_vertices, the V of the vertices that were rasterised."""
    face_index_map: torch.Tensor
    weight_map: torch.Tensor
    depth_map: torch.Tensor
    faces: torch.Tensor
    visibility: torch.Tensor
    tri: torch.Tensor
    fill_back: bool
    image_size: int
    anti_aliasing: bool
    num_vertices: int

    @property
    def raster_size(self):
        return int(self.image_size) * (2 if self.anti_aliasing else 1)

    def c_struct(self):
        """The d3m_fragments (include/d3m_raster.h) that points at the record's tensors; whoever holds the record keeps them."""
        return _lib.D3MFragments(self.face_index_map.data_ptr(), self.weight_map.data_ptr(), self.depth_map.data_ptr(),
                                 self.faces.data_ptr(), self.tri.data_ptr(), self.visibility.data_ptr(),
                                 self.visibility.numel(), self.face_index_map.shape[0], self.tri.shape[0],
                                 int(bool(self.fill_back)), int(self.image_size), int(bool(self.anti_aliasing)))


def rasterize_fragments(screen_vertices, faces, image_size, anti_aliasing=True, fill_back=True, near=0.1, far=100):
    """The coverage record of screen-space vertices [B,V,3] f32 over ONE topology faces [F,3] or [1,F,3] (int32 / int64):
    d3m_forward_face_index_map_mesh, then the visibility blob is finished -- nothing else is launched.  The record is a
    constant: vertices that require grad raise NotImplementedError (no silent zero gradient); per-view topology raises
    ValueError."""
    if not torch.is_tensor(screen_vertices) or screen_vertices.dim() != 3 or screen_vertices.shape[-1] != 3 \
            or screen_vertices.shape[1] < 1:
        raise ValueError("screen_vertices must be [B, num_vertices, 3]")
    if screen_vertices.dtype != torch.float32:
        raise ValueError("screen_vertices must be float32")
    faces = checked_faces(faces)
    B, V = screen_vertices.shape[:2]
    if not 1 <= B <= MAX_VIEWS:
        raise ValueError(f"1 to {MAX_VIEWS} views per call")
    s = int(image_size)
    if s < 1:
        raise ValueError("image_size must be positive")
    if torch.is_grad_enabled() and screen_vertices.requires_grad:
        raise NotImplementedError("rasterize_fragments: the screen vertices require grad; detach them: an attribute image "
                                  "carries no geometry gradient")
    if not screen_vertices.is_cuda or faces.device != screen_vertices.device:
        raise ValueError("screen_vertices and faces must be on one GPU device")
    L = _lib.lib()
    dev = screen_vertices.device
    sv = screen_vertices.detach().contiguous()
    tri = faces.reshape(-1, 3).to(torch.int32).contiguous()
    Ft = tri.shape[0]
    Fp = 2 * Ft if fill_back else Ft
    S = 2 * s if anti_aliasing else s
    dense = torch.empty(B, Fp, 3, 3, dtype=torch.float32, device=dev)
    fi = torch.empty(B, S, S, dtype=torch.int32, device=dev)
    wm = torch.empty(B, S, S, 3, dtype=torch.float32, device=dev)
    dm = torch.empty(B, S, S, dtype=torch.float32, device=dev)
    vis = torch.empty(int(L.d3m_visibility_bytes(B, Fp)), dtype=torch.uint8, device=dev)
    ws = ops._workspace("fwd", L.d3m_forward_workspace_bytes(B, Fp, S), dev)
    _lib.check(L.d3m_forward_face_index_map_mesh(
        _lib.ptr(sv), _lib.ptr(tri), 1, V, Ft, int(bool(fill_back)), _lib.ptr(dense), _lib.ptr(fi), _lib.ptr(wm), _lib.ptr(dm),
        None, B, S, float(near), float(far), _lib.ptr(ws), ws.numel(), _lib.ptr(vis), vis.numel(), 0, _lib.stream_ptr()),
        "d3m_forward_face_index_map_mesh")
    # (its first step -- which faces own a pixel -- was left by the coverage pass)
    _lib.check(L.d3m_visibility(None, _lib.ptr(vis), vis.numel(), B, Fp, S, _lib.stream_ptr()), "d3m_visibility")
    return Fragments(fi, wm, dm, dense, vis, tri, bool(fill_back), s, bool(anti_aliasing), int(V))


def _checked_fragments(fr):
    if not isinstance(fr, Fragments):
        raise ValueError("fragments must be a Fragments record (rasterize_fragments, Renderer.fragments)")
    fi, S = fr.face_index_map, fr.raster_size
    if not all(torch.is_tensor(t) for t in fr[:6]) or fi.dim() != 3 or fr.tri.dim() != 2 or fr.tri.shape[1] != 3:
        raise ValueError("fragments: malformed record")
    B, Ft = fi.shape[0], fr.tri.shape[0]
    Fp = 2 * Ft if fr.fill_back else Ft
    shapes = ((fi, (B, S, S), torch.int32), (fr.weight_map, (B, S, S, 3), torch.float32),
              (fr.depth_map, (B, S, S), torch.float32), (fr.faces, (B, Fp, 3, 3), torch.float32), (fr.tri, (Ft, 3), torch.int32))
    for t, shape, dtype in shapes:
        if tuple(t.shape) != shape or t.dtype != dtype or t.device != fi.device or not t.is_contiguous():
            raise ValueError("fragments: the maps do not fit one another (shape, dtype, device or layout)")
    if not 1 <= B <= MAX_VIEWS or Ft < 1 or S < 1:
        raise ValueError("fragments: empty record")
    if fr.visibility.dtype != torch.uint8 or fr.visibility.device != fi.device or not fr.visibility.is_contiguous():
        raise ValueError("fragments: malformed visibility blob")
    return B, Ft, Fp


def _checked_background(background, C, attributes):
    """None, or the [C] f32 device tensor of a background given as a float or as [C] values."""
    if background is None:
        return None
    if torch.is_tensor(background):
        if background.requires_grad:
            raise ValueError("background must not require grad: the node is differentiable in the attributes only")
        if background.dim() == 0:
            background = float(background)
        elif tuple(background.shape) != (C,) or background.dtype != torch.float32 or background.device != attributes.device:
            raise ValueError(f"background must be None, a float or [{C}] float32 on the attributes' device")
        else:
            return background.contiguous()
    if isinstance(background, (int, float)):
        return const_tensor([float(background)] * C, attributes.device)
    values = list(background)
    if len(values) != C:
        raise ValueError(f"background must be None, a float or [{C}] values")
    return const_tensor([float(x) for x in values], attributes.device)


def _attribute_images_launch(fr, attr, background):
    """(images, alpha) of contiguous attributes: the forward's one launch"""
    batched = attr.dim() == 3
    V, C = attr.shape[-2:]
    B, s = fr.face_index_map.shape[0], int(fr.image_size)
    images = torch.empty(B, C, s, s, dtype=torch.float32, device=attr.device)
    alpha = torch.empty(B, s, s, dtype=torch.float32, device=attr.device)
    c_fr = fr.c_struct()
    _lib.check(_lib.lib().d3m_vertex_attribute_images(ctypes.byref(c_fr), _lib.ptr(attr), B if batched else 1, V, C,
                                                      _lib.ptr(background), _lib.ptr(images), _lib.ptr(alpha),
                                                      _lib.stream_ptr()), "d3m_vertex_attribute_images")
    return images, alpha


def _attribute_images_adjoint(fr, A, g, batched, sizes):
    """grad_attributes of the contiguous f32 image gradient g: the fixed-order gather"""
    B, V, C = sizes
    L = _lib.lib()
    Fp = fr.faces.shape[1]
    n = int(L.d3m_vertex_attribute_scratch_floats(B, Fp, C, ctypes.byref(A.csr.c)))
    scratch = torch.empty(n, dtype=torch.float32, device=g.device)
    grad = torch.empty((B, V, C) if batched else (V, C), dtype=torch.float32, device=g.device)
    c_fr = fr.c_struct()
    _lib.check(L.d3m_vertex_attribute_images_backward(ctypes.byref(c_fr), _lib.ptr(g), ctypes.byref(A.csr.c),
                                                      _lib.ptr(scratch), n, _lib.ptr(grad), B if batched else 1, V, C,
                                                      _lib.stream_ptr()), "d3m_vertex_attribute_images_backward")
    return grad


# ---- the interior geometry gradient (csrc/d3m_fragment_geometry.h) ----------------------------------------------------------
MAX_PIXEL_TERMS = 1 << 32  # B S S: one lane per internal pixel


def _checked_pixel_lanes(fragments, who):
    """What every node with one lane per internal pixel refuses: a record with B S S beyond 2^32."""
    n = fragments.face_index_map.shape[0] * fragments.raster_size ** 2
    if n > MAX_PIXEL_TERMS:
        raise ValueError(f"{who}: B S S = {n} is beyond 2^32")


def _checked_screen_vertices(screen_vertices, fragments, who):
    """The screen vertices a node differentiates in: [B,V,3] f32 on the record's device, V the record's.  That they are the
    vertices the record was rasterised from cannot be checked: the caller's business."""
    B = fragments.face_index_map.shape[0]
    if not torch.is_tensor(screen_vertices) or screen_vertices.dim() != 3 or screen_vertices.shape[-1] != 3:
        raise ValueError(f"{who}: screen_vertices must be [B, num_vertices, 3]")
    if screen_vertices.dtype != torch.float32:
        raise ValueError(f"{who}: screen_vertices must be float32")
    if screen_vertices.shape[0] != B:
        raise ValueError(f"{who}: screen_vertices must be [{B}, V, 3] for fragments of {B} views")
    if screen_vertices.shape[1] != fragments.num_vertices:
        raise ValueError(f"{who}: screen_vertices have {screen_vertices.shape[1]} vertices, the fragments were rasterised "
                         f"from {fragments.num_vertices}")
    if screen_vertices.device != fragments.face_index_map.device:
        raise ValueError(f"{who}: screen_vertices must be on the fragments' device")
    _checked_pixel_lanes(fragments, who)


def _geometry_scratch(fr, A, with_pixel_grads):
    """(pixel_grads [B,S,S,3] or None, the adjoint's scratch): one uninitialised buffer"""
    B, S, Fp = fr.face_index_map.shape[0], fr.raster_size, fr.faces.shape[1]
    n = int(_lib.lib().d3m_fragment_geometry_scratch_floats(B, Fp, S, ctypes.byref(A.csr.c), int(with_pixel_grads)))
    scratch = torch.empty(n, dtype=torch.float32, device=fr.face_index_map.device)
    if not with_pixel_grads:
        return None, scratch
    n_h = B * S * S * 3
    return scratch[:n_h].view(B, S, S, 3), scratch[n_h:]


def _geometry_adjoint(fr, A, pixel_grads, scratch):
    """grad_screen_vertices [B,V,3] of contiguous f32 pixel_grads [B,S,S,3] = dL/du: the shared fixed-order adjoint"""
    B, V = fr.face_index_map.shape[0], int(fr.num_vertices)
    grad = torch.empty(B, V, 3, dtype=torch.float32, device=pixel_grads.device)
    c_fr = fr.c_struct()
    _lib.check(_lib.lib().d3m_fragment_geometry_backward(ctypes.byref(c_fr), _lib.ptr(pixel_grads), ctypes.byref(A.csr.c),
                                                         _lib.ptr(scratch), scratch.numel(), _lib.ptr(grad), V,
                                                         _lib.stream_ptr()), "d3m_fragment_geometry_backward")
    return grad


def _node_geometry_adjoint(fr, A, launch_pixel_grads):
    """grad_screen_vertices of a node: launch_pixel_grads(c_fr, h) writes the node's dL/du into h [B,S,S,3], then the shared
    adjoint; h and the adjoint's scratch are one uninitialised buffer"""
    h, scratch = _geometry_scratch(fr, A, True)
    c_fr = fr.c_struct()
    launch_pixel_grads(ctypes.byref(c_fr), _lib.ptr(h))
    return _geometry_adjoint(fr, A, h, scratch)


class _VertexAttributeImages(torch.autograd.Function):
    """screen_vertices: None, or the vertices the record was rasterised from as a second differentiable input -- the same
    forward launch and the same adjoint for the attributes; the vertices' gradient through the node's pixel_grads and the
    shared adjoint.  The attributes are kept for the backward only when the vertices need a gradient."""
    @staticmethod
    def forward(ctx, attributes, screen_vertices, fragments, adjacency, background):
        attr = attributes.contiguous()
        images, alpha = _attribute_images_launch(fragments, attr, background)
        if ctx.needs_input_grad[1]:
            ctx.save_for_backward(attr)
        ctx.fragments, ctx.adjacency, ctx.batched = fragments, adjacency, attr.dim() == 3
        ctx.sizes = (images.shape[0],) + tuple(attr.shape[-2:])
        ctx.mark_non_differentiable(alpha)
        return images, alpha

    @staticmethod
    def backward(ctx, grad_images, _grad_alpha):
        fr, A = ctx.fragments, ctx.adjacency
        B, V, C = ctx.sizes
        g = grad_images.to(torch.float32).contiguous()
        grad_attr = _attribute_images_adjoint(fr, A, g, ctx.batched, ctx.sizes) if ctx.needs_input_grad[0] else None
        grad_sv = None
        if ctx.needs_input_grad[1]:
            attr, = ctx.saved_tensors
            grad_sv = _node_geometry_adjoint(fr, A, lambda c_fr, h: _lib.check(_lib.lib().d3m_vertex_attribute_pixel_grads(
                c_fr, _lib.ptr(attr), B if ctx.batched else 1, V, C, _lib.ptr(g), h, _lib.stream_ptr()),
                "d3m_vertex_attribute_pixel_grads"))
        return grad_attr, grad_sv, None, None, None


def interpolate_vertex_attributes(attributes, fragments, background=None, cache=None, screen_vertices=None):
    """(images [B,C,s,s], alpha [B,s,s]) of attributes [V,C] (shared by the views) or [B,V,C], f32 on the record's device,
    1 <= C <= 1024, over a Fragments record; background: None (zeros), a float, or [C].  Differentiable in `attributes`
    only; alpha is the coverage (the bits of render_silhouettes), not differentiable.  The first call with the record's tri
    builds the faces' adjacency (outside any stream capture; a ValueError for an index outside [0, V)) and later calls reuse
    it; `cache`: the AdjacencyCache to keep it in (default: row_gather's).  ValueError, before anything is launched, for a
    wrong rank, dtype, device, V, C, batch or background.

    screen_vertices None: as above.  screen_vertices [B,V,3] f32 on the record's device -- THE vertices the record was
    rasterised from, still attached to the graph (their values cannot be checked; shape, dtype, device and V are): the same
    forward launch and the same bits of images, alpha and the attributes' gradient, and in addition the INTERIOR geometry
    gradient reaches screen_vertices.grad: the derivative of the weights u_c of every owned pixel with respect to the
    owner's corners (csrc/d3m_fragment_geometry.h), in a fixed order.  Coverage stays a constant -- no gradient from a
    pixel changing its owner or from the silhouette, which render_silhouettes / render give, and antialias (antialias.py)
    for the drawn image itself.  Vertices that do not require grad launch nothing extra."""
    if not torch.is_tensor(attributes) or attributes.dim() not in (2, 3):
        raise ValueError("attributes must be [num_vertices, C] or [B, num_vertices, C]")
    if attributes.dtype != torch.float32:
        raise ValueError("attributes must be float32")
    V, C = attributes.shape[-2:]
    if not 1 <= C <= MAX_CHANNELS:
        raise ValueError(f"attributes: 1 to {MAX_CHANNELS} channels")
    B, Ft, Fp = _checked_fragments(fragments)
    if V != fragments.num_vertices:
        raise ValueError(f"attributes have {V} vertices, the fragments were rasterised from {fragments.num_vertices}")
    if attributes.dim() == 3 and attributes.shape[0] != B:
        raise ValueError(f"attributes must be [V, C] or [{B}, V, C] for fragments of {B} views")
    if attributes.device != fragments.face_index_map.device:
        raise ValueError("attributes must be on the fragments' device")
    if screen_vertices is not None:
        _checked_screen_vertices(screen_vertices, fragments, "interpolate_vertex_attributes")
    background = _checked_background(background, C, attributes)
    adjacency = vertex_adjacency(fragments.tri, V, cache)          # (where tri's indices are checked against V)
    if not attributes.is_cuda:
        raise ValueError("attributes and fragments must be on one GPU device")
    return _VertexAttributeImages.apply(attributes, screen_vertices, fragments, adjacency, background)
