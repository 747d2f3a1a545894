"""Per-pixel uv texture images: a texture image [H,W,C] (or [B,H,W,C], channels last like textures_from_image's [H,W,3])
looked up bilinearly at the interpolated uv of every pixel of a coverage record, differentiable with respect to the image.

The render nodes colour a pixel through per-face texture cubes, so the detail that reaches the picture is bounded by faces x
texture_size^3; here it is bounded by the image.  `sample_uv_texture` reads a `Fragments` record (rasterize_fragments,
Renderer.fragments), faces_uv [F,3,2] -- the per-corner uv that textures_from_image and UVTextures take, wrapped per corner
as load_textures wraps it -- and the image: internal pixel p takes the four bilinear taps at pos = clamp(sum_c u_c uv_c *
(size - 1)), u_c the perspective-correct weights of interpolate_vertex_attributes, an uncovered pixel the background; the
output is that map with its rows reversed and, with anti-aliasing, 2x2-averaged.  One launch.  csrc/d3m_uv_texture.h states
every step.

The adjoint is a scatter whose destinations change with every coverage.  It is independent of order by construction: every
term w_j * (scale * g) is rounded to a multiple of the quantum q = 2^(E - frac), E = ilogb(max |scale g|) + 1, frac =
uv_adjoint_fraction_bits(B, S), and added to an int64 accumulator per element of the image's gradient with an INTEGER atomic.
Integer sums are associative: the same bits on every run, for every arrival order and launch shape; no float atomics; the
maximum is found on the device, so nothing is read back and a stream capture is not broken.  Three launches.  A gradient
that is all zeros gives an exact +0 everywhere; an Inf or NaN anywhere in it makes every element NaN; a texel that no sample
reaches gets +0."""
import ctypes

import torch

from .. import _lib
from .attributes import _checked_background, _checked_fragments
from .uv_textures import _wrapping_code

MAX_CHANNELS = 64          # UVT_MAX_CHANNELS of csrc/d3m_uv_texture.h
CHANNEL_CHUNK = 8          # UVT_CHUNK: the channels a lane of the forward keeps in registers at a time
MAX_IMAGE_SIZE = 32768     # UVT_MAX_SIZE
MAX_PIXEL_TERMS = 1 << 32  # B S S: beyond it fewer than 30 fraction bits would be left
CLAMP_TO_BORDER = 3


def uv_adjoint_fraction_bits(B, S):
    """frac = 62 - ceil(log2(B S S)): the bits below 2^E (the power of two above the largest |scale g|) that a term keeps in
    the adjoint's int64 accumulators.  B S S terms of at most 2^frac each cannot overflow.  ValueError beyond B S S = 2^32."""
    n = int(B) * int(S) * int(S)
    if n < 1:
        raise ValueError("B and S must be positive")
    if n > MAX_PIXEL_TERMS:
        raise ValueError(f"sample_uv_texture: B S S = {n} is beyond 2^32 (fewer than 30 fraction bits in the adjoint)")
    return 62 - (n - 1).bit_length()


class _UvTextureImages(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, faces_uv, fragments, wrapping, background):
        fr = fragments
        img = image.contiguous()
        batched = img.dim() == 4
        H, W, C = img.shape[-3:]
        B, s = fr.face_index_map.shape[0], int(fr.image_size)
        images = torch.empty(B, C, s, s, dtype=torch.float32, device=img.device)
        alpha = torch.empty(B, s, s, dtype=torch.float32, device=img.device)
        c_fr = fr.c_struct()
        _lib.check(_lib.lib().d3m_uv_texture_images(ctypes.byref(c_fr), _lib.ptr(faces_uv), _lib.ptr(img), B if batched else 1,
                                                    H, W, C, wrapping, _lib.ptr(background), _lib.ptr(images), _lib.ptr(alpha),
                                                    _lib.stream_ptr()), "d3m_uv_texture_images")
        ctx.fragments, ctx.faces_uv, ctx.wrapping, ctx.batched, ctx.sizes = fr, faces_uv, wrapping, batched, (B, H, W, C)
        ctx.mark_non_differentiable(alpha)
        return images, alpha

    @staticmethod
    def backward(ctx, grad_images, _grad_alpha):
        fr = ctx.fragments
        B, H, W, C = ctx.sizes
        L = _lib.lib()
        g = grad_images.to(torch.float32).contiguous()
        ib = B if ctx.batched else 1
        n = int(L.d3m_uv_texture_images_scratch_bytes(ib, H, W, C, B, fr.raster_size))
        scratch = torch.empty((n + 7) // 8, dtype=torch.int64, device=g.device)
        grad = torch.empty((B, H, W, C) if ctx.batched else (H, W, C), dtype=torch.float32, device=g.device)
        c_fr = fr.c_struct()
        _lib.check(L.d3m_uv_texture_images_backward(ctypes.byref(c_fr), _lib.ptr(ctx.faces_uv), _lib.ptr(g), ib, H, W, C,
                                                    ctx.wrapping, _lib.ptr(scratch), scratch.numel() * 8, _lib.ptr(grad),
                                                    _lib.stream_ptr()), "d3m_uv_texture_images_backward")
        return grad, None, None, None, None


def sample_uv_texture(image, faces_uv, fragments, texture_wrapping='REPEAT', background=None):
    """(images [B,C,s,s], alpha [B,s,s]) of a texture image [H,W,C] (shared by the views) or [B,H,W,C], f32 on the record's
    device, 1 <= C <= 64, texture space as textures_from_image reads it; faces_uv [F,3,2] f32 for the record's F faces, a
    constant; texture_wrapping 'REPEAT', 'MIRRORED_REPEAT' or 'CLAMP_TO_EDGE' (or 0..2), applied to the corners; background:
    None (zeros), a float, or [C].  Differentiable in `image` only: faces_uv that requires grad raises NotImplementedError;
    alpha is the coverage (the bits of interpolate_vertex_attributes' alpha), not differentiable.  ValueError / TypeError,
    before anything is launched, for a wrong rank, dtype, device, C, F, batch, wrapping or background, and for a record with
    B S S beyond 2^32."""
    if not torch.is_tensor(image) or not torch.is_tensor(faces_uv):
        raise TypeError("image and faces_uv must be tensors")
    if image.dtype != torch.float32 or faces_uv.dtype != torch.float32:
        raise TypeError("image and faces_uv must be float32")
    if image.dim() not in (3, 4) or image.shape[-3] < 1 or image.shape[-2] < 1:
        raise ValueError("image must be [H, W, C] or [B, H, W, C]")
    H, W, C = image.shape[-3:]
    if not 1 <= C <= MAX_CHANNELS:
        raise ValueError(f"image: 1 to {MAX_CHANNELS} channels")
    if H > MAX_IMAGE_SIZE or W > MAX_IMAGE_SIZE:
        raise ValueError(f"image: at most {MAX_IMAGE_SIZE} rows and columns")
    wrapping = _wrapping_code(texture_wrapping)
    if wrapping == CLAMP_TO_BORDER:
        raise ValueError("sample_uv_texture: CLAMP_TO_BORDER is not offered (REPEAT, MIRRORED_REPEAT or CLAMP_TO_EDGE)")
    B, Ft, Fp = _checked_fragments(fragments)
    if faces_uv.dim() != 3 or tuple(faces_uv.shape) != (Ft, 3, 2):
        raise ValueError(f"faces_uv must be [{Ft}, 3, 2] for fragments of {Ft} faces")
    if image.dim() == 4 and image.shape[0] != B:
        raise ValueError(f"image must be [H, W, C] or [{B}, H, W, C] for fragments of {B} views")
    uv_adjoint_fraction_bits(B, fragments.raster_size)
    if faces_uv.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError("sample_uv_texture: no gradient with respect to faces_uv (it is a constant; detach it)")
    dev = fragments.face_index_map.device
    if image.device != dev or faces_uv.device != dev:
        raise ValueError("image and faces_uv must be on the fragments' device")
    background = _checked_background(background, C, image)
    if not image.is_cuda:
        raise ValueError("image and fragments must be on one GPU device")
    return _UvTextureImages.apply(image, faces_uv.detach().contiguous(), fragments, wrapping, background)
