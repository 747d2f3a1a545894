"""Regularisers of a learnable UV texture: smoothness, left-right symmetry, flatness and an anchor to a reference texture,
value and gradient in one autograd node (`uv_texture_regularizer`, `UvTextureRegularizer`) -- the texture half's counterpart
of mesh_regularizer.  Per image, with a texel ACTIVE iff its mask is > 0 (negative and NaN: absent; no mask: every texel):

    L_smooth = (1/(P C)) sum over the P pairs of 4-neighbours (i,j)-(i,j+1), (i,j)-(i+1,j) that are both active, and the
               channels k, of rho(x_a[k] - x_b[k]);  rho(d) = d^2, or sqrt(d^2 + eps^2) - eps with smooth_eps = eps > 0
    L_sym    = (1/(M C)) sum over the M active texels with j < W-1-j whose mirror texel (i, W-1-j) is active, and k, of
               (x[i,j,k] - x[i,W-1-j,k])^2                       (the centre column of an odd W pairs with nothing)
    L_flat   = (1/(N C)) sum over the N active texels and k of (x[k] - mu_k)^2,  mu_k the channel's mean over the active texels
    L_anchor = (1/(R C)) sum over the active texels t of r_t sum_k (x_t[k] - ref_t[k])^2,  r = reference_weights where they are
               > 0, else 0 (None: 1), R = the sum of r_t over the active texels

A term whose count (P, M, N, R) is 0 is exactly +0 with a gradient of exactly +0.  The counts are taken on the device on every
call -- a bake's `valid` changes every step -- and are constants of the graph.  csrc/d3m_uv_texture_reg.h states the order of
every sum.  Differentiable in the texture only.  The gradient of a texel is a gather (its neighbours, its mirror texel, its own
flat and anchor terms): no float atomics, nothing cleared, every element written, an inactive texel exactly +0, the same bits
on every run.  No host synchronisation: forward and backward can be captured.

Launches, whatever B, H, W, C and the weights: forward 4 (k_uv_texture_reg_stats, k_uv_texture_reg_stats_finish,
k_uv_texture_reg_terms, k_uv_texture_reg_value_finish); backward 1 (k_uv_texture_reg_terms: the forward leaves its
[B, 4 + C] coefficients and channel means for it)."""
import torch
import torch.nn as nn

from .. import _lib
from .uv_bake import cached_uv_layout_fragments
from .uv_texture_images import MAX_IMAGE_SIZE

MAX_CHANNELS = 4            # UVR_MAX_CHANNELS of csrc/d3m_uv_texture_reg.h
MAX_IMAGES = 65535
PER_PART = 256              # UVR_PER_PART: texels per part of an image's sums
MAX_PARTS = 256             # UVR_MAX_PARTS: beyond PER_PART * MAX_PARTS texels the lanes stride
NO_EPS = -1.0               # D3M_UV_TEXTURE_REG_NO_EPS
KERNELS_FORWARD = ("k_uv_texture_reg_stats", "k_uv_texture_reg_stats_finish", "k_uv_texture_reg_terms",
                   "k_uv_texture_reg_value_finish")
KERNELS_BACKWARD = ("k_uv_texture_reg_terms",)


def num_parts(height, width):
    """Parts (workgroups) per image of the node's sums: uvr_parts of csrc/d3m_uv_texture_reg.h."""
    return max(1, min(MAX_PARTS, (int(height) * int(width) + PER_PART - 1) // PER_PART))


def _aligned(t, channels):
    """t, contiguous and with texels of `channels` floats aligned as the kernels' vector loads need them."""
    t = t.contiguous()
    need = 16 if channels == 4 else (8 if channels == 2 else 4)
    return t.clone() if t.data_ptr() % need else t


def _call(x, mask, weights, reference, reference_weights, stats, grad_scale, want_value, want_grad):
    """The entry points on x [B,H,W,C]: (value [B] or None, stats [B, 4 + C], grad [B,H,W,C] or None).  stats None: the value
    entry point (the forward), which computes them."""
    L = _lib.lib()
    B, H, W, C = (int(v) for v in x.shape)
    smooth, eps, symmetry, flat, anchor = weights
    dev = x.device
    f32 = dict(dtype=torch.float32, device=dev)
    scratch = torch.empty(max(int(L.d3m_uv_texture_regularizer_scratch_bytes(B, H, W)) // 4, 1), **f32)
    value = torch.empty(B, **f32) if want_value else None
    inputs = (_lib.ptr(x), B, H, W, C, _lib.ptr(mask), 0 if mask is None else (B if mask.dim() == 3 else 1), smooth, eps,
              symmetry, flat, anchor, _lib.ptr(reference), 0 if reference is None else (B if reference.dim() == 4 else 1),
              _lib.ptr(reference_weights), 0 if reference_weights is None else (B if reference_weights.dim() == 3 else 1))
    if stats is None:
        stats = torch.empty(B, 4 + C, **f32)
        _lib.check(L.d3m_uv_texture_regularizer(*inputs, _lib.ptr(scratch), scratch.numel() * 4, _lib.ptr(stats),
                                                _lib.ptr(value), _lib.stream_ptr()), "d3m_uv_texture_regularizer")
        return value, stats, None
    grad = torch.empty_like(x) if want_grad else None
    _lib.check(L.d3m_uv_texture_regularizer_grad(*inputs, _lib.ptr(stats), _lib.ptr(grad_scale), _lib.ptr(scratch),
                                                 scratch.numel() * 4, _lib.ptr(value), _lib.ptr(grad), _lib.stream_ptr()),
               "d3m_uv_texture_regularizer_grad")
    return value, stats, grad


class _UvTextureRegularizer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, texture, mask, weights, reference, reference_weights):
        batched = texture.dim() == 4
        C = int(texture.shape[-1])
        x = _aligned(texture if batched else texture[None], C)
        mask = None if mask is None else mask.contiguous()
        anchor = weights[4] > 0.0
        reference = _aligned(reference, C) if anchor else None
        reference_weights = reference_weights.contiguous() if anchor and reference_weights is not None else None
        value, stats, _ = _call(x, mask, weights, reference, reference_weights, None, None, True, False)
        ctx.save_for_backward(x, stats, *(t for t in (mask, reference, reference_weights) if t is not None))
        ctx.have = (mask is not None, reference is not None, reference_weights is not None)
        ctx.weights, ctx.batched = weights, batched
        return value if batched else value[0]

    @staticmethod
    def backward(ctx, grad_value):
        x, stats, *rest = ctx.saved_tensors
        rest = iter(rest)
        mask, reference, reference_weights = (next(rest) if have else None for have in ctx.have)
        scale = grad_value.reshape(-1).to(torch.float32).contiguous()           # stays on the device
        _, _, grad = _call(x, mask, ctx.weights, reference, reference_weights, stats, scale, False, True)
        return (grad if ctx.batched else grad[0]), None, None, None, None


def _checked_weights(smooth, smooth_eps, symmetry, flat, anchor):
    w = tuple(float(v) for v in (smooth, symmetry, flat, anchor))
    if not all(0.0 <= v < float("inf") for v in w):           # (NaN fails too)
        raise ValueError("uv_texture_regularizer: smooth, symmetry, flat and anchor must be >= 0 and finite")
    if not any(v > 0.0 for v in w):
        raise ValueError("uv_texture_regularizer: one of smooth, symmetry, flat and anchor must be > 0")
    eps = NO_EPS
    if smooth_eps is not None:
        eps = float(smooth_eps)
        if not 0.0 < eps < float("inf"):
            raise ValueError("uv_texture_regularizer: smooth_eps must be None or > 0")
    return (w[0], eps, w[1], w[2], w[3])


def _checked_plane(t, name, lead, sizes, channels, texture):
    """A constant of the node: [H,W(,C)] or [B,H,W(,C)] f32 on the texture's device, not requiring grad."""
    H, W = sizes
    tail = (H, W) + ((channels,) if channels else ())
    shapes = [tail] + ([(lead,) + tail] if lead is not None else [])
    if not torch.is_tensor(t) or tuple(t.shape) not in shapes:
        raise ValueError(f"uv_texture_regularizer: {name} must be " + " or ".join(str(list(s)) for s in shapes) +
                         " for this texture")
    if t.dtype != torch.float32:
        raise ValueError(f"uv_texture_regularizer: {name} must be float32")
    if t.device != texture.device:
        raise ValueError(f"uv_texture_regularizer: {name} must be on the texture's device")
    if t.requires_grad:
        raise ValueError(f"uv_texture_regularizer: {name} must not require grad: the node is differentiable in the texture only")
    return t


def uv_texture_regularizer(texture, mask=None, smooth=0.0, smooth_eps=None, symmetry=0.0, flat=0.0, anchor=0.0, reference=None,
                           reference_weights=None):
    """smooth * L_smooth + symmetry * L_sym + flat * L_flat + anchor * L_anchor of a UV texture (the module text),
    differentiable with respect to `texture`: one autograd node, value and gradient by d3m_uv_texture_regularizer in a fixed
    order.

    texture [H,W,C] or [B,H,W,C] (f32 on a GPU, channels last, row j = texture row j: what sample_uv_texture and
    shade_uv_texture take and fuse_uv_textures returns); 1 <= C <= 4, 1 <= B <= 65535, H and W at most 32768.  mask [H,W]
    (shared by the images) or [B,H,W], f32: a texel is active iff its mask is > 0; None: every texel.  reference [H,W,C] or
    [B,H,W,C] and reference_weights [H,W] or [B,H,W] (None: 1; a weight that is not > 0 counts as 0): the anchor's.  Returns a
    0-d tensor for [H,W,C], [B] for [B,H,W,C]: every image on its own.  A term of weight 0 is not evaluated and its inputs
    are not read.

    mask, reference and reference_weights are constants (one that requires grad raises).  ValueError / TypeError, before
    anything is launched, for a wrong rank, dtype, device, shape, C, B or size, a negative weight, all weights 0, a
    smooth_eps that is not > 0, or anchor > 0 without a reference."""
    if not torch.is_tensor(texture):
        raise TypeError("uv_texture_regularizer: texture must be a tensor")
    if texture.dim() not in (3, 4) or any(int(v) < 1 for v in texture.shape):
        raise ValueError("uv_texture_regularizer: texture must be [H, W, C] or [B, H, W, C]")
    if texture.dtype != torch.float32:
        raise ValueError("uv_texture_regularizer: texture must be float32")
    batched = texture.dim() == 4
    H, W, C = (int(v) for v in texture.shape[-3:])
    B = int(texture.shape[0]) if batched else None
    if batched and not 1 <= B <= MAX_IMAGES:
        raise ValueError(f"uv_texture_regularizer: texture: 1 to {MAX_IMAGES} images")
    if not 1 <= C <= MAX_CHANNELS:
        raise ValueError(f"uv_texture_regularizer: texture: 1 to {MAX_CHANNELS} channels")
    if H > MAX_IMAGE_SIZE or W > MAX_IMAGE_SIZE:
        raise ValueError(f"uv_texture_regularizer: texture: at most {MAX_IMAGE_SIZE} rows and columns")
    weights = _checked_weights(smooth, smooth_eps, symmetry, flat, anchor)
    if mask is not None:
        mask = _checked_plane(mask, "mask", B, (H, W), 0, texture)
    if weights[4] > 0.0:
        if reference is None:
            raise ValueError("uv_texture_regularizer: anchor > 0 needs a reference")
        reference = _checked_plane(reference, "reference", B, (H, W), C, texture)
        if reference_weights is not None:
            reference_weights = _checked_plane(reference_weights, "reference_weights", B, (H, W), 0, texture)
    else:
        reference = reference_weights = None
    if not texture.is_cuda:
        raise ValueError("uv_texture_regularizer: the texture must be on a GPU device")
    return _UvTextureRegularizer.apply(texture, mask, weights, reference, reference_weights)


def uv_texture_smoothness(texture, mask=None, smooth_eps=None):
    """L_smooth: the mean of rho over the active 4-neighbour pairs and the channels."""
    return uv_texture_regularizer(texture, mask, smooth=1.0, smooth_eps=smooth_eps)


def uv_texture_symmetry(texture, mask=None):
    """L_sym: the mean squared difference of a texel and its mirror texel (u -> 1 - u) where both are active."""
    return uv_texture_regularizer(texture, mask, symmetry=1.0)


def uv_texture_flatness(texture, mask=None):
    """L_flat: the variance of the active texels about their channel means (the reflectance-constancy loss)."""
    return uv_texture_regularizer(texture, mask, flat=1.0)


def uv_texture_anchor(texture, reference, mask=None, reference_weights=None):
    """L_anchor: the weighted mean squared difference from `reference` over the active texels."""
    return uv_texture_regularizer(texture, mask, anchor=1.0, reference=reference, reference_weights=reference_weights)


def uv_layout_mask(faces_uv, texture_size, texture_wrapping='REPEAT', cache=None):
    """The [T,T] f32 mask (1 or 0) of the texels that a triangle of the layout faces_uv [F,3,2] owns at T = texture_size: the
    mask of a learnable albedo that no bake gave one.  face_index_map[0] >= 0 of cached_uv_layout_fragments (internal row j is
    texture row j there): no kernel of its own; `cache`: the UvLayoutCache to keep the layout record in."""
    fragments = cached_uv_layout_fragments(faces_uv, texture_size, texture_wrapping, cache)
    return (fragments.face_index_map[0] >= 0).to(torch.float32)


class UvTextureRegularizer(nn.Module):
    """The regulariser of one texture layout: the weights, and `mask`, `reference` and `reference_weights` as buffers (each
    may be None); forward(texture) returns the weighted sum.  Mirrors MeshRegularizer."""

    def __init__(self, mask=None, smooth=0.0, smooth_eps=None, symmetry=0.0, flat=0.0, anchor=0.0, reference=None,
                 reference_weights=None):
        super().__init__()
        _checked_weights(smooth, smooth_eps, symmetry, flat, anchor)
        if float(anchor) > 0.0 and reference is None:
            raise ValueError("uv_texture_regularizer: anchor > 0 needs a reference")
        self.smooth, self.symmetry, self.flat, self.anchor = (float(v) for v in (smooth, symmetry, flat, anchor))
        self.smooth_eps = None if smooth_eps is None else float(smooth_eps)
        for name, t in (("mask", mask), ("reference", reference), ("reference_weights", reference_weights)):
            self.register_buffer(name, None if t is None else torch.as_tensor(t).detach().to(torch.float32).contiguous().clone())

    @property
    def weights(self):
        return dict(smooth=self.smooth, smooth_eps=self.smooth_eps, symmetry=self.symmetry, flat=self.flat, anchor=self.anchor)

    def forward(self, texture):
        return uv_texture_regularizer(texture, self.mask, reference=self.reference, reference_weights=self.reference_weights,
                                      **self.weights)
