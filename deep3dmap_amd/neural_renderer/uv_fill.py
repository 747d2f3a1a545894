"""Baked view textures fused into one and completed by push-pull: the step between bake_uv_texture and
sample_uv_texture(mipmap=True).  A bake gives one texture and one 0/1 mask per view; fused in torch the result still holds the
background wherever no view saw the surface and everywhere outside the layout's triangles, and the lookup's bilinear taps at
chart borders and every level of its box pyramid average that background into the picture.

`fuse_uv_textures` takes textures [B,H,W,C] and weights [B,H,W].  A view counts at a texel iff its weight is > 0; a texel is
valid iff some view counts; a valid texel is the weighted mean of the counting views (ascending b, f32).  With `fill` the
invalid texels are filled: the valid texels are summed and counted 2 x 2 up to a 1 x 1 level (levels of (h + 1) >> 1 rows, any
H and W), and on the way back down a texel with valid texels under it is their mean and every other one the bilinear value of
the level above at its centre; the top falls back to the background.  Valid texels pass through bit for bit.
csrc/d3m_uv_fill.h states every step and the order of every sum.

Differentiable in the textures; the weights and the set of valid texels are constants, `valid` is not differentiable.  The
adjoint is a chain of gathers in a fixed order: no atomics, the same bits on every run.  Forward three launches (one without
the fill), backward two to four up to 2048 x 2048 (one without the fill), independent of B, C and the number of levels."""
import ctypes

import torch

from .. import _lib
from .attributes import _checked_background
from .uv_texture_images import MAX_CHANNELS, MAX_IMAGE_SIZE

MAX_VIEWS = 65535


class _FuseUvTextures(torch.autograd.Function):
    @staticmethod
    def forward(ctx, textures, weights, fill, background):
        L = _lib.lib()
        x, w = textures.contiguous(), weights.contiguous()
        B, H, W, C = (int(v) for v in x.shape)
        texture = torch.empty(H, W, C, dtype=torch.float32, device=x.device)
        valid = torch.empty(H, W, dtype=torch.float32, device=x.device)
        n_counts = int(L.d3m_uv_fill_pyramid_texels(H, W)) if fill else 0
        counts = torch.empty(max(n_counts, 1), dtype=torch.int32, device=x.device)
        n = int(L.d3m_uv_fill_scratch_bytes(H, W, C)) if fill else 4
        scratch = torch.empty((n + 3) // 4, dtype=torch.float32, device=x.device)
        _lib.check(L.d3m_uv_fill_textures(_lib.ptr(x), _lib.ptr(w), B, H, W, C, fill, _lib.ptr(background), _lib.ptr(scratch),
                                          scratch.numel() * 4, _lib.ptr(counts), counts.numel(), _lib.ptr(texture),
                                          _lib.ptr(valid), _lib.stream_ptr()), "d3m_uv_fill_textures")
        ctx.save_for_backward(w, valid, counts)
        ctx.fill, ctx.sizes = fill, (B, H, W, C)
        ctx.mark_non_differentiable(valid)
        return texture, valid

    @staticmethod
    def backward(ctx, grad_texture, _grad_valid):
        L = _lib.lib()
        B, H, W, C = ctx.sizes
        w, valid, counts = ctx.saved_tensors
        g = grad_texture.to(torch.float32).contiguous()
        n = int(L.d3m_uv_fill_backward_scratch_bytes(H, W, C)) if ctx.fill else 4
        scratch = torch.empty((n + 3) // 4, dtype=torch.float32, device=g.device)
        grad = torch.empty(B, H, W, C, dtype=torch.float32, device=g.device)
        _lib.check(L.d3m_uv_fill_textures_backward(_lib.ptr(w), _lib.ptr(valid), _lib.ptr(counts), counts.numel(), _lib.ptr(g), B,
                                                   H, W, C, ctx.fill, _lib.ptr(scratch), scratch.numel() * 4, _lib.ptr(grad),
                                                   _lib.stream_ptr()), "d3m_uv_fill_textures_backward")
        return grad, None, None, None


def fuse_uv_textures(textures, weights, fill=True, background=None):
    """(texture [H,W,C], valid [H,W]) of textures [B,H,W,C] (f32 on a GPU, channels last, row j = texture row j: what
    bake_uv_texture returns and sample_uv_texture takes) and weights [B,H,W] (f32; a bake's mask, or a mask times a view-angle
    weight).  1 <= B <= 65535, 1 <= C <= 64, H and W at most 32768, any H and W.  A weight that is negative or NaN counts as
    absent.  fill=True: invalid texels are filled by push-pull (the module's docstring); fill=False: they are the background.
    background: None (zeros), a float or [C]: the value of an invalid texel without the fill, and of every texel when none is
    valid.  valid is 1.0 or 0.0.

    Differentiable in `textures`; `weights` are constants (a weights tensor that requires grad raises), and so is the set of
    valid texels.  ValueError, before anything is launched, for a wrong rank, dtype, device, B, size, C or background."""
    if not torch.is_tensor(textures) or textures.dim() != 4 or textures.shape[1] < 1 or textures.shape[2] < 1:
        raise ValueError("fuse_uv_textures: textures must be [B, H, W, C]")
    if textures.dtype != torch.float32:
        raise ValueError("fuse_uv_textures: textures must be float32")
    B, H, W, C = (int(v) for v in textures.shape)
    if not 1 <= B <= MAX_VIEWS:
        raise ValueError(f"fuse_uv_textures: textures: 1 to {MAX_VIEWS} views")
    if not 1 <= C <= MAX_CHANNELS:
        raise ValueError(f"fuse_uv_textures: textures: 1 to {MAX_CHANNELS} channels")
    if H > MAX_IMAGE_SIZE or W > MAX_IMAGE_SIZE:
        raise ValueError(f"fuse_uv_textures: textures: at most {MAX_IMAGE_SIZE} rows and columns")
    if not torch.is_tensor(weights) or tuple(weights.shape) != (B, H, W):
        raise ValueError(f"fuse_uv_textures: weights must be [{B}, {H}, {W}] for these textures")
    if weights.dtype != torch.float32:
        raise ValueError("fuse_uv_textures: weights must be float32")
    if weights.device != textures.device:
        raise ValueError("fuse_uv_textures: weights must be on the textures' device")
    if weights.requires_grad:
        raise ValueError("fuse_uv_textures: weights must not require grad: the node is differentiable in the textures only")
    background = _checked_background(background, C, textures)
    if not textures.is_cuda:
        raise ValueError("fuse_uv_textures: textures and weights must be on one GPU device")
    return _FuseUvTextures.apply(textures, weights, int(bool(fill)), background)


def fill_uv_texture(texture, mask, background=None):
    """texture [H,W,C] with the texels whose mask [H,W] is not > 0 filled by push-pull: fuse_uv_textures with B = 1, the texture
    only.  Texels with mask > 0 pass through bit for bit.  Differentiable in `texture`."""
    if not torch.is_tensor(texture) or texture.dim() != 3:
        raise ValueError("fill_uv_texture: texture must be [H, W, C]")
    if not torch.is_tensor(mask) or mask.dim() != 2:
        raise ValueError("fill_uv_texture: mask must be [H, W]")
    return fuse_uv_textures(texture[None], mask[None], True, background)[0]
