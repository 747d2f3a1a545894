"""Learnable uv texture images: `textures_from_image` (image -> per-face texture cubes, differentiable with respect to the
image) and `UVTextures` (the images of a textured .obj as parameters).

The map image -> cubes is d3m_load_textures's sampling (obj_io.load_textures_from_image), which is linear in the image.
Its adjoint is the transpose of that map, walked as a gather: a CSR with one row per image pixel whose entries are
(texel, weight) in ascending texel order (d3m_uv_texture_taps + a stable sort by pixel, built once per layout and cached),
reduced by d3m_uv_texture_adjoint in a fixed order -- no float atomics, the same bits on every run.  Texel 0 of every face
samples pixel (0,0) with weight 1, so that row holds one entry per face: rows longer than LONG_ROW entries go through the
chunked reduction that row_gather.py describes.

The layout (faces_uv, face mask, texture size, image size, wrapping, filter) is a constant: a gradient with respect to
faces_uv raises NotImplementedError."""
import ctypes
from collections import namedtuple

import torch
import torch.nn as nn

from .. import _lib
from . import obj_io
from .row_gather import CACHE_SIZE, CHUNK, LONG_ROW, BuiltCache, build_csr, csr_offsets, long_row_chunks, tensor_key  # noqa: F401 (the constants stay importable from here)

Transpose = namedtuple("Transpose", "csr lanes_per_row num_texels height width")
Transpose.__doc__ = """The transpose of one layout's sampling map: csr, the row_gather.Csr of H*W rows whose items [nnz,2] are
(texel, weight bits), and the lanes that walk each row that is not long (a power of two, about a quarter of the mean length
of a non-empty row)."""


def _wrapping_code(texture_wrapping):
    if isinstance(texture_wrapping, str):
        if texture_wrapping not in obj_io.texture_wrapping_dict:
            raise ValueError(f"texture_wrapping must be one of {sorted(obj_io.texture_wrapping_dict)}")
        return obj_io.texture_wrapping_dict[texture_wrapping]
    code = int(texture_wrapping)
    if not 0 <= code <= 3:
        raise ValueError("texture_wrapping must be 0..3 or its name")
    return code


# ---- the transpose's cache --------------------------------------------------------------------------------------------
class TransposeCache(BuiltCache):
    """BuiltCache for transposes: an entry also holds the caller's faces_uv and mask tensors."""
    what = "textures_from_image: the uv layout's transpose"


_cache = TransposeCache()


def _layout_key(faces_uv, mask, texture_size, height, width, wrapping, use_bilinear):
    return (tensor_key(faces_uv), tensor_key(mask), int(texture_size), int(height), int(width), int(wrapping), bool(use_bilinear))


def build_transpose(faces_uv, mask32, texture_size, height, width, wrapping, use_bilinear):
    """The CSR of the map's transpose (see the module text).  Synchronises (the entry count): never inside a capture."""
    dev = faces_uv.device
    F, ts = faces_uv.shape[0], int(texture_size)
    taps = 4 if use_bilinear else 1
    n_texels = F * ts ** 3
    n_pix = height * width
    pixel = torch.empty(n_texels * taps, dtype=torch.int32, device=dev)
    weight = torch.empty(n_texels * taps, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().d3m_uv_texture_taps(
        _lib.ptr(faces_uv), _lib.ptr(mask32), F, ts, height, width, int(wrapping), int(bool(use_bilinear)),
        _lib.ptr(pixel), _lib.ptr(weight), _lib.stream_ptr()), "d3m_uv_texture_taps")
    # stable: a pixel's entries keep ascending entry order = ascending (texel, tap); dropped entries (pixel H*W) sort last
    keys, order = torch.sort(pixel, stable=True)
    nnz = int((keys < n_pix).sum())
    order = order[:nnz]
    entries = torch.stack([torch.div(order, taps, rounding_mode="floor").to(torch.int32),
                           weight[order].view(torch.int32)], 1)
    # (the long rows are few: pixel (0,0) and whatever a layout piles up)
    csr = build_csr(keys[:nnz].long(), n_pix, entries)
    # a row's walk is a chain of dependent loads: split the typical row over a few lanes (fixed per layout)
    mean = nnz / max(1, int((csr.offsets[1:] > csr.offsets[:-1]).sum()))
    lanes = 1
    while lanes < 16 and lanes * 4 < mean:
        lanes *= 2
    return Transpose(csr, lanes, n_texels, height, width)


def uv_transpose(faces_uv, texture_size, height, width, texture_wrapping='REPEAT', use_bilinear=True, faces_mask=None):
    """The cached transpose of a layout (built on the first call with these tensors, at their current versions)."""
    wrapping = _wrapping_code(texture_wrapping)
    key = _layout_key(faces_uv, faces_mask, texture_size, height, width, wrapping, use_bilinear)

    def build():
        mask32 = None if faces_mask is None else faces_mask.to(torch.int32).contiguous()
        return build_transpose(faces_uv, mask32, texture_size, height, width, wrapping, use_bilinear)
    return _cache.get(key, build, holders=(faces_uv, faces_mask))


def uv_texture_adjoint(transpose, grad_textures):
    """grad_image [B,H,W,3] of grad_textures [B, F*ts^3*3 floats] through the transpose (d3m_uv_texture_adjoint)."""
    T = transpose
    B = grad_textures.shape[0]
    g = grad_textures.to(torch.float32).contiguous()
    if g.dim() != 2 or g.shape[1] != T.num_texels * 3 or g.device != T.csr.offsets.device:
        raise ValueError(f"grad_textures must be [B, {T.num_texels * 3}] on {T.csr.offsets.device}")
    grad_image = torch.empty(B, T.height, T.width, 3, dtype=torch.float32, device=g.device)
    partials = torch.empty(B, T.csr.num_chunks, 3, dtype=torch.float32, device=g.device) if T.csr.num_chunks else None
    _lib.check(_lib.lib().d3m_uv_texture_adjoint(
        ctypes.byref(T.csr.c), T.lanes_per_row, _lib.ptr(g), _lib.ptr(partials), _lib.ptr(grad_image), B, T.num_texels,
        T.height, T.width, _lib.stream_ptr()), "d3m_uv_texture_adjoint")
    return grad_image


# ---- the autograd function ---------------------------------------------------------------------------------------------
class _TexturesFromImage(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, base, faces_uv, mask32, transpose, ts, wrapping, use_bilinear, batched):
        images = image if batched else image[None]
        B, H, W = images.shape[:3]
        F = faces_uv.shape[0]
        out = torch.empty(B, F, ts, ts, ts, 3, dtype=torch.float32, device=image.device)
        base_batch = 0 if base is None else (base.shape[0] if base.dim() == 6 else 1)
        _lib.check(_lib.lib().d3m_textures_from_image(
            _lib.ptr(images), B, _lib.ptr(faces_uv), _lib.ptr(mask32), _lib.ptr(base), base_batch, _lib.ptr(out), F, ts, H,
            W, wrapping, int(use_bilinear), _lib.stream_ptr()), "d3m_textures_from_image")
        ctx.transpose, ctx.batched = transpose, batched
        ctx.base_shape = None if base is None else base.shape
        ctx.save_for_backward(mask32)
        return out if batched else out[0]

    @staticmethod
    def backward(ctx, grad_out):
        mask32, = ctx.saved_tensors
        g = grad_out if ctx.batched else grad_out[None]
        B = g.shape[0]
        grad_image = grad_base = None
        if ctx.needs_input_grad[0]:
            grad_image = uv_texture_adjoint(ctx.transpose, g.reshape(B, -1))
            if not ctx.batched:
                grad_image = grad_image[0]
        if ctx.needs_input_grad[1]:
            # the faces outside the mask pass base through (no mask: every face samples the image)
            if mask32 is None:
                gb = torch.zeros_like(g)
            else:
                gb = torch.where((mask32 == 0).reshape(1, -1, 1, 1, 1, 1), g, torch.zeros((), dtype=g.dtype, device=g.device))
            if len(ctx.base_shape) == 5:
                gb = gb.sum(0)
            grad_base = gb.reshape(ctx.base_shape)
        return grad_image, grad_base, None, None, None, None, None, None, None


def textures_from_image(image, faces_uv, texture_size=4, texture_wrapping='REPEAT', use_bilinear=True, faces_mask=None,
                        base=None):
    """Per-face texture cubes sampled from a uv image, differentiable with respect to `image` and `base`.

    image [H,W,3] or [B,H,W,3] f32, texture space (row 0 = bottom, as obj_io's image reader returns it); faces_uv [F,3,2]
    f32, a constant.  Returns [F,ts,ts,ts,3] (or [B,F,ts,ts,ts,3]): what obj_io.load_textures_from_image writes for the
    faces with faces_mask != 0 (every face when None), bit for bit; the other faces copy base ([F,ts,ts,ts,3], or
    [B,F,ts,ts,ts,3] with a batch of images; zeros when None) and pass its gradient through.  texture_wrapping: 'REPEAT',
    'MIRRORED_REPEAT', 'CLAMP_TO_EDGE', 'CLAMP_TO_BORDER' (or 0..3).  The image's gradient needs the layout's transpose:
    the first call with a layout builds it (outside any stream capture) and later calls reuse it."""
    if image.dtype != torch.float32 or faces_uv.dtype != torch.float32 or (base is not None and base.dtype != torch.float32):
        raise TypeError("image, faces_uv and base must be float32")
    if image.dim() not in (3, 4) or image.shape[-1] != 3 or image.shape[-3] < 1 or image.shape[-2] < 1:
        raise ValueError("image must be [H, W, 3] or [B, H, W, 3]")
    if faces_uv.dim() != 3 or tuple(faces_uv.shape[1:]) != (3, 2) or faces_uv.shape[0] < 1:
        raise ValueError("faces_uv must be [num_faces, 3, 2]")
    ts = int(texture_size)
    if ts < 2:
        raise ValueError("texture_size must be at least 2")
    wrapping = _wrapping_code(texture_wrapping)
    batched = image.dim() == 4
    F = faces_uv.shape[0]
    B = image.shape[0] if batched else 1
    if batched and B > 65535:
        raise ValueError("at most 65535 images per call")
    cube = (F, ts, ts, ts, 3)
    if base is not None and tuple(base.shape) != cube and not (batched and tuple(base.shape) == (B,) + cube):
        raise ValueError(f"base must be {list(cube)}" + (f" or {[B] + list(cube)}" if batched else ""))
    if faces_mask is not None:
        if tuple(faces_mask.shape) != (F,):
            raise ValueError("faces_mask must be [num_faces]")
        if faces_mask.dtype not in (torch.bool, torch.int32, torch.int64, torch.uint8):
            raise TypeError("faces_mask must be bool or integer")
    if faces_uv.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError("textures_from_image: no gradient with respect to faces_uv (it is a constant; detach it)")
    _lib.require_device(image, faces_uv, faces_mask, base, names=("image", "faces_uv", "faces_mask", "base"))
    if any(t is not None and t.device != image.device for t in (faces_uv, faces_mask, base)):
        raise ValueError("image, faces_uv, faces_mask and base must be on one device")
    mask32 = None if faces_mask is None else faces_mask.to(torch.int32).contiguous()
    transpose = None
    if image.requires_grad and torch.is_grad_enabled():
        transpose = uv_transpose(faces_uv, ts, image.shape[-3], image.shape[-2], wrapping, use_bilinear, faces_mask)
    return _TexturesFromImage.apply(image, base, faces_uv, mask32, transpose, ts, wrapping, bool(use_bilinear), batched)


# ---- the images of an .obj as parameters -------------------------------------------------------------------------------
class UVTextures(nn.Module):
    """The texture images of a scene as learnable parameters: forward() returns the per-face cubes [F,ts,ts,ts,3] --
    `base` (buffer), then each image (parameter `images[i]`) sampled over the faces of its mask (buffer), in order."""

    def __init__(self, faces_uv, images, masks, base, texture_size=4, texture_wrapping='REPEAT', use_bilinear=True,
                 names=None):
        super().__init__()
        if len(images) != len(masks):
            raise ValueError("one face mask per image")
        self.texture_size = int(texture_size)
        self.texture_wrapping = texture_wrapping
        self.use_bilinear = bool(use_bilinear)
        self.names = list(names) if names is not None else [str(i) for i in range(len(images))]
        self.register_buffer("faces_uv", faces_uv.detach().to(torch.float32).contiguous())
        self.register_buffer("base", base.detach().to(torch.float32).contiguous())
        for i, m in enumerate(masks):
            self.register_buffer(f"mask_{i}", m.detach().to(torch.int32).contiguous())
        self.images = nn.ParameterList([nn.Parameter(im.detach().to(torch.float32).contiguous()) for im in images])

    @classmethod
    def from_obj(cls, filename_obj, filename_mtl=None, texture_size=4, texture_wrapping='REPEAT', use_bilinear=True):
        """The textures load_obj(filename_obj, load_texture=True, ...) returns, with one learnable image per map_Kd
        material (its `mtllib` unless filename_mtl is given): forward() equals that array bit for bit at construction."""
        import os
        scene = obj_io._ObjScene(filename_obj)
        obj_dir = os.path.dirname(filename_obj)
        if filename_mtl is None:
            if scene.mtllib is None:
                raise Exception('Failed to load textures.')
            filename_mtl = os.path.join(obj_dir, scene.mtllib)
        faces_uv, base, layers = obj_io._scene_layers(scene, obj_dir, filename_mtl, texture_size)
        return cls(faces_uv, [im for _, im, _ in layers], [m for _, _, m in layers], base, texture_size, texture_wrapping,
                   use_bilinear, names=[n for n, _, _ in layers])

    def masks(self):
        return [getattr(self, f"mask_{i}") for i in range(len(self.images))]

    def forward(self):
        tex = self.base
        for image, mask in zip(self.images, self.masks()):
            tex = textures_from_image(image, self.faces_uv, self.texture_size, self.texture_wrapping, self.use_bilinear,
                                      faces_mask=mask, base=tex)
        return tex
