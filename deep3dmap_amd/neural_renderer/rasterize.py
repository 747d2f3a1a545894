"""Differentiable rasterization: RasterizeFunction / Rasterize / rasterize_rgbad and friends, same
signatures and semantics as pnpmodules/neural_renderer/neural_renderer/rasterize.py (NR/rasterize.py),
running on the HIP operators of libd3m_raster.so.  CUDA(=HIP)-device tensors only, like the reference."""
import collections
import ctypes
import dataclasses
import os
from typing import Any, NamedTuple, Optional

import torch
import torch.nn as nn

from .. import _lib
from . import rasterize_ops as ops
from ._util import const_tensor, deterministic as _deterministic, f32c
from .built_cache import BuiltCache, tensor_key
from .row_gather import vertex_adjacency

DEFAULT_IMAGE_SIZE = 256
DEFAULT_ANTI_ALIASING = True
DEFAULT_NEAR = 0.1
DEFAULT_FAR = 100
DEFAULT_EPS = 1e-4
DEFAULT_BACKGROUND_COLOR = (0, 0, 0)


def _background_tensor(background_color, device):
    """[1,3] or [B,3] device tensor (NR/rasterize.py:189-194 accepts a colour or one colour per batch entry)."""
    if background_color is None:
        background_color = DEFAULT_BACKGROUND_COLOR
    if torch.is_tensor(background_color):
        t = background_color.to(device=device, dtype=torch.float32)
    else:
        t = const_tensor(background_color, device)
    return (t[None, :] if t.dim() == 1 else t).contiguous()


def _raster_forward(faces, textures, image_size, near, far, eps, background, return_rgb, return_alpha,
                    return_depth, keep_reference_maps):
    """Kernels 1+2 (+3), background blend and alpha: the body of NR/rasterize.py:50-84.
    keep_reference_maps: also materialise the reference's face_inv_map / faces_inv scratch."""
    dev = faces.device
    B, F = faces.shape[:2]
    S = int(image_size)
    m = {}
    # the reference pre-fills these (-1 / 0 / far / 0, rasterize.py:50-58); d3m_forward_face_index_map writes every
    # pixel, covered or not, so they are only allocated here
    m["face_index_map"] = torch.empty((B, S, S), dtype=torch.int32, device=dev)
    m["weight_map"] = torch.empty(B, S, S, 3, dtype=torch.float32, device=dev)
    m["depth_map"] = torch.empty((B, S, S), dtype=torch.float32, device=dev)
    dummy = torch.zeros(1, dtype=torch.float32, device=dev)
    want_finv = return_depth and keep_reference_maps
    face_inv_map = torch.empty(B, S, S, 3, 3, dtype=torch.float32, device=dev) if want_finv else dummy
    faces_inv = torch.zeros_like(faces) if keep_reference_maps else dummy
    ops.forward_face_index_map(faces, m["face_index_map"], m["weight_map"], m["depth_map"], face_inv_map, faces_inv,
                               S, near, far, return_rgb, return_alpha, want_finv)
    m["face_inv_map"] = face_inv_map
    m["faces_inv"] = faces_inv
    rgb_sampled = None
    if return_rgb:
        rgb_sampled = torch.zeros(B, S, S, 3, dtype=torch.float32, device=dev)
        m["sampling_index_map"] = torch.zeros(B, S, S, 8, dtype=torch.int32, device=dev)
        m["sampling_weight_map"] = torch.zeros(B, S, S, 8, dtype=torch.float32, device=dev)
        ops.forward_texture_sampling(faces, textures, m["face_index_map"], m["weight_map"], m["depth_map"],
                                     rgb_sampled, m["sampling_index_map"], m["sampling_weight_map"], S, eps)
    return m, rgb_sampled


def _epilogue(m, rgb_sampled, background, B, S, anti_aliasing, return_rgb, return_alpha, return_depth, outputs):
    """d3m_output_epilogue: blend + alpha at internal resolution and, when `outputs`, the flipped / pooled
    CHW output images of rasterize_rgbad in the same pass."""
    dev = m["face_index_map"].device
    s = S // 2 if anti_aliasing else S
    m["rgb_map"] = torch.empty(B, S, S, 3, dtype=torch.float32, device=dev) if return_rgb else None
    m["alpha_map"] = torch.empty(B, S, S, dtype=torch.float32, device=dev) if return_alpha else None
    rgb_out = alpha_out = depth_out = None
    if outputs:
        rgb_out = torch.empty(B, 3, s, s, dtype=torch.float32, device=dev) if return_rgb else None
        alpha_out = torch.empty(B, s, s, dtype=torch.float32, device=dev) if return_alpha else None
        depth_out = torch.empty(B, s, s, dtype=torch.float32, device=dev) if return_depth else None
    rc = _lib.lib().d3m_output_epilogue(
        _lib.ptr(m["face_index_map"]), _lib.ptr(rgb_sampled), _lib.ptr(m["depth_map"] if (outputs and return_depth) else None),
        _lib.ptr(background if return_rgb else None), background.shape[0] if return_rgb else 1,
        _lib.ptr(m["rgb_map"]), _lib.ptr(m["alpha_map"]), _lib.ptr(rgb_out), _lib.ptr(alpha_out), _lib.ptr(depth_out),
        B, S, int(bool(anti_aliasing and outputs)), _lib.stream_ptr())
    _lib.check(rc, "d3m_output_epilogue")
    return rgb_out, alpha_out, depth_out


def _raster_backward(faces, textures, m, S, eps, grad_rgb_map, grad_alpha_map, grad_depth_map, return_rgb,
                     return_alpha, return_depth, need_textures_grad):
    """NR/rasterize.py:109-156: K4 (overwrite) -> K5 -> K6 (add)."""
    dev = faces.device
    dummy = torch.zeros(1, dtype=torch.float32, device=dev)
    grad_faces = torch.zeros_like(faces, dtype=torch.float32)
    grad_textures = None
    if return_rgb or return_alpha:
        ops.backward_pixel_map(faces, m["face_index_map"], m["rgb_map"] if return_rgb else dummy,
                               m["alpha_map"] if return_alpha else dummy, grad_rgb_map if return_rgb else dummy,
                               grad_alpha_map if return_alpha else dummy, grad_faces, S, eps, return_rgb, return_alpha)
    if return_rgb and need_textures_grad:
        grad_textures = torch.zeros_like(textures, dtype=torch.float32)
        ops.backward_textures(m["face_index_map"], m["sampling_weight_map"], m["sampling_index_map"], grad_rgb_map,
                              grad_textures, faces.shape[1], faces=faces)
    if return_depth:
        ops.backward_depth_map(faces, m["depth_map"], m["face_index_map"], m["face_inv_map"], m["weight_map"],
                               grad_depth_map, grad_faces, S)
    return grad_faces, grad_textures


class RasterizeFunction(torch.autograd.Function):
    '''
    Definition of differentiable rasterize operation (NR/rasterize.py:15-226): internal-resolution maps,
    row 0 = bottom of the image.  Returns (rgb_map [B,S,S,3], alpha_map [B,S,S], depth_map [B,S,S]);
    disabled outputs are empty tensors.
    '''
    @staticmethod
    def forward(ctx, faces, textures, image_size, near, far, eps, background_color,
                return_rgb=False, return_alpha=False, return_depth=False):
        faces = f32c(faces)
        if return_rgb:
            textures = f32c(textures)
        dev = faces.device
        B = faces.shape[0]
        S = int(image_size)
        background = _background_tensor(background_color, dev) if return_rgb else None
        m, rgb_sampled = _raster_forward(faces, textures if return_rgb else None, S, float(near), float(far), float(eps),
                                         background, return_rgb, return_alpha, return_depth, True)
        if return_rgb or return_alpha:
            _epilogue(m, rgb_sampled, background, B, S, False, return_rgb, return_alpha, return_depth, False)
        ctx.cfg = (S, float(eps), bool(return_rgb), bool(return_alpha), bool(return_depth))
        ctx.maps = m
        ctx.save_for_backward(faces, textures if return_rgb else None)
        ctx.tex_needs_grad = bool(return_rgb and ctx.needs_input_grad[1])
        rgb_r = m["rgb_map"] if return_rgb else torch.tensor([])
        alpha_r = m["alpha_map"].clone() if return_alpha else torch.tensor([])
        depth_r = m["depth_map"].clone() if return_depth else torch.tensor([])
        return rgb_r, alpha_r, depth_r

    @staticmethod
    def backward(ctx, grad_rgb_map, grad_alpha_map, grad_depth_map):
        faces, textures = ctx.saved_tensors
        S, eps, rr, ra, rd = ctx.cfg
        g_rgb = f32c(grad_rgb_map) if rr else None
        g_alpha = f32c(grad_alpha_map) if ra else None
        g_depth = f32c(grad_depth_map) if rd else None
        gf, gt = _raster_backward(faces, textures, ctx.maps, S, eps, g_rgb, g_alpha, g_depth, rr, ra, rd,
                                  ctx.tex_needs_grad)
        return gf, gt, None, None, None, None, None, None, None, None


class Rasterize(nn.Module):
    '''
    Wrapper around the autograd function RasterizeFunction (NR/rasterize.py:228-251).
    '''
    def __init__(self, image_size, near, far, eps, background_color,
                 return_rgb=False, return_alpha=False, return_depth=False):
        super(Rasterize, self).__init__()
        self.image_size = image_size
        self.near = near
        self.far = far
        self.eps = eps
        self.background_color = background_color
        self.return_rgb = return_rgb
        self.return_alpha = return_alpha
        self.return_depth = return_depth

    def forward(self, faces, textures):
        if not faces.is_cuda or (textures is not None and not textures.is_cuda):
            raise TypeError('Rasterize module supports only cuda Tensors')
        return RasterizeFunction.apply(faces, textures, self.image_size, self.near, self.far,
                                       self.eps, self.background_color,
                                       self.return_rgb, self.return_alpha, self.return_depth)


class _RasterizeImages(torch.autograd.Function):
    """rasterize_rgbad in one autograd node: RasterizeFunction + vertical flip + CHW + 2x2 pooling
    (NR/rasterize.py:297-326), with the epilogue and its adjoint as single kernels."""

    @staticmethod
    def forward(ctx, faces, textures, image_size, anti_aliasing, near, far, eps, background_color, return_rgb,
                return_alpha, return_depth):
        faces = f32c(faces)
        if return_rgb:
            textures = f32c(textures)
        dev = faces.device
        B = faces.shape[0]
        S = int(image_size) * 2 if anti_aliasing else int(image_size)
        background = _background_tensor(background_color, dev) if return_rgb else None
        m, rgb_sampled = _raster_forward(faces, textures if return_rgb else None, S, float(near), float(far), float(eps),
                                         background, return_rgb, return_alpha, return_depth, False)
        rgb, alpha, depth = _epilogue(m, rgb_sampled, background, B, S, anti_aliasing, return_rgb, return_alpha,
                                      return_depth, True)
        ctx.cfg = (S, float(eps), bool(anti_aliasing), bool(return_rgb), bool(return_alpha), bool(return_depth))
        ctx.maps = m
        ctx.save_for_backward(faces, textures if return_rgb else None)
        ctx.tex_needs_grad = bool(return_rgb and ctx.needs_input_grad[1])
        empty = torch.tensor([])
        return (rgb if return_rgb else empty, alpha if return_alpha else empty, depth if return_depth else empty)

    @staticmethod
    def backward(ctx, g_rgb, g_alpha, g_depth):
        faces, textures = ctx.saved_tensors
        S, eps, aa, rr, ra, rd = ctx.cfg
        dev, B = faces.device, faces.shape[0]
        g_rgb_map = torch.empty(B, S, S, 3, dtype=torch.float32, device=dev) if rr else None
        g_alpha_map = torch.empty(B, S, S, dtype=torch.float32, device=dev) if ra else None
        g_depth_map = torch.empty(B, S, S, dtype=torch.float32, device=dev) if rd else None
        rc = _lib.lib().d3m_output_epilogue_backward(
            _lib.ptr(f32c(g_rgb) if rr else None), _lib.ptr(f32c(g_alpha) if ra else None),
            _lib.ptr(f32c(g_depth) if rd else None), _lib.ptr(g_rgb_map), _lib.ptr(g_alpha_map), _lib.ptr(g_depth_map),
            B, S, int(aa), _lib.stream_ptr())
        _lib.check(rc, "d3m_output_epilogue_backward")
        gf, gt = _raster_backward(faces, textures, ctx.maps, S, eps, g_rgb_map, g_alpha_map, g_depth_map, rr, ra, rd,
                                  ctx.tex_needs_grad)
        return (gf, gt) + (None,) * 9


_vec3_cache = {}


def _vec3_host(x):
    """A light colour / direction as three host floats (the C ABI takes them by value).  A device tensor costs a
    device-to-host copy -- a synchronisation -- so its value is remembered per tensor OBJECT and version (a weak reference:
    an address alone may be a new tensor in a freed one's place): the copy happens once per in-place change, not per call."""
    import weakref
    import numpy as np
    cacheable = torch.is_tensor(x) and x.is_cuda
    if cacheable:
        hit = _vec3_cache.get(id(x))
        if hit is not None and hit[0]() is x and hit[1] == x._version:
            return np.ctypeslib.as_ctypes(hit[2])
    a = x.detach().cpu().numpy() if torch.is_tensor(x) else x
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1))
    if a.size != 3:
        raise NotImplementedError("lighting: per-batch colours / directions are not supported by the HIP path")
    if cacheable:
        if len(_vec3_cache) >= 64:
            _vec3_cache.clear()
        _vec3_cache[id(x)] = (weakref.ref(x), x._version, a)
    return np.ctypeslib.as_ctypes(a)


LIGHT_FIELDS = ("intensity_ambient", "intensity_directional", "color_ambient", "color_directional", "direction")


def _light_param_batch(name, x):
    """The batch of one light parameter, from its shape alone: colours / direction [3] (1) or [n,3] (n), intensities a
    number, 0-d or [n] (n).  Anything else raises ValueError."""
    import numpy as np
    shape = tuple(x.shape) if torch.is_tensor(x) else np.shape(x)
    if name.startswith("intensity"):
        if len(shape) <= 1:
            return shape[0] if shape else 1
        raise ValueError(f"light {name} must be a number, a 0-d tensor or one value per view [B]; got shape {shape}")
    if len(shape) == 1 and shape[0] == 3:
        return 1
    if len(shape) == 2 and shape[1] == 3:
        return shape[0]
    raise ValueError(f"light {name} must be [3] or one row per view [B,3]; got shape {shape}")


def light_on_device(light_cfg):
    """The lit node's route rule: its light is read from device memory (d3m_light) and is an autograd input of the node
    when any parameter is a tensor that requires grad or is given per view; every other light is passed by value."""
    return any((torch.is_tensor(x) and x.requires_grad) or _light_param_batch(name, x) > 1
               for name, x in zip(LIGHT_FIELDS, light_cfg))


def normalize_light(light_cfg, batch, device):
    """(intensity_ambient, intensity_directional, color_ambient, color_directional, direction) -> five float32 device
    tensors [n], [n], [n,3], [n,3], [n,3] with n = 1 or `batch` each; differentiable (reshapes of the caller's tensors).
    Each may be a number, list, tuple, numpy array or tensor: colours and direction [3] or [B,3] (NR/lighting.py:25-30),
    intensities a number, a 0-d tensor or -- an extension of this library; the reference takes one intensity for the
    batch -- one per view, [B].  A batch other than 1 or `batch`, or a wrong last dimension, raises ValueError."""
    out = []
    for name, x in zip(LIGHT_FIELDS, light_cfg):
        n = _light_param_batch(name, x)
        if n not in (1, batch):
            raise ValueError(f"light {name} has batch {n}; the render has {batch} views (1 or {batch} expected)")
        t = x.to(device=device, dtype=torch.float32) if torch.is_tensor(x) else const_tensor(x, device)
        out.append(t.reshape(n) if name.startswith("intensity") else t.reshape(n, 3))
    return tuple(t.contiguous() for t in out)


def _light_struct(tensors, like=None):
    """d3m_light of five device tensors (gradient buffers: None = skipped) with the batches of `like` (default: themselves)"""
    return _lib.D3MLight(*[_lib.ptr(t) for t in tensors], *[int(t.shape[0]) for t in (like or tensors)])


def _host_zero(x):
    """a light intensity known on the host to be 0 (a tensor is never looked at: that would synchronise)"""
    import numpy as np
    return not torch.is_tensor(x) and bool(np.all(np.asarray(x, dtype=np.float32) == 0))


_side_streams = ops.StreamKeyedCache(max_per_kind=64)     # ((device index, which), forking stream handle) -> torch.cuda.Stream


def _serial_branches(batch, num_tri, image_size):
    """Whether a lit render node keeps its side branches (visibility list + edge plan beside the sampling pass; the
    gathered texture / depth pass beside the line walk) on the forking stream.  Default: never -- the branches win at every
    size measured in round 6 (32 views of the headline mesh 1.555-1.568 -> 1.506-1.522 ms on one box, 64 views -2.5 %, the
    anti-aliased step -3 %, 8 views at 1024x1024 -4.5 %, config 5 -1 to -4 %: tools_dev/branches_ab.sh).
    Rounds 4 and 5 ran the big batches (d3m_forward_big_batch) on one stream: with the kernels of that time the cross-queue
    waits cost what the filled tails bought (-1.5 % to +0 %); every kernel that got shorter since left a longer tail to fill.
    D3M_SERIAL_BRANCHES=1 / 0 forces / forbids (measurements); the deterministic mode and LitFitManual run on one stream."""
    env = os.environ.get("D3M_SERIAL_BRANCHES")
    if env is not None and env != "":
        return env != "0"
    return False


def _side_stream(device, which=0, serial=False):
    """Extra streams per (device, forking stream) for the branches a lit render node runs beside its main line: the
    visibility list / the gathered texture pass of every view group, and the main line of every group but the first.
    serial: the forking stream itself (see _serial_branches)."""
    if serial:
        return torch.cuda.current_stream(device)
    index = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
    key = ((index, which), torch.cuda.current_stream(device).cuda_stream)     # one set per stream that forks
    stream = _side_streams.get(key)
    if stream is None:
        stream = torch.cuda.Stream(device=device)
        _side_streams.put(key, stream)
    return stream


MAX_VIEW_GROUPS = 3       # every group brings two streams; a captured step with ten concurrent branches made hipGraphLaunch
                          # segfault on ROCm 7.2 (2 and 3 groups replay fine), and more groups were slower anyway


def _group_bounds(B, groups):
    g = max(1, min(int(groups), B, MAX_VIEW_GROUPS))
    return [(B * k // g, B * (k + 1) // g) for k in range(g)]


def _bslice(t, lo, hi):
    """views lo..hi of a tensor whose leading axis is the batch, or the tensor itself when it is shared (batch 1)"""
    if t is None:
        return None
    return t if t.shape[0] == 1 else t[lo:hi]


class _Records(NamedTuple):
    """A gradient as the edge gradient reads it: per-pixel records at the internal size S (what d3m_backward_pixel_map
    would pack from gradient maps), the lines' non-zero extents and, for a fused objective, its depth gradient as a map."""
    edge_grad: torch.Tensor                 # [B,S,S,4]
    edge_dot: torch.Tensor                  # [B,S,S,2]
    extents: Any                            # (nz_lo_inv, nz_hi1), each [B,2,S] int32: a [2,B,2,S] tensor or two views
    grad_depth: Optional[torch.Tensor]      # [B,S,S] (a fused objective's records only)

    def fields(self, lo, hi):
        """the records' fields of d3m_fit_targets for views lo..hi"""
        p = lambda t: _lib.ptr(None if t is None else t[lo:hi])     # noqa: E731
        return dict(grad_depth_map=p(self.grad_depth), edge_grad=p(self.edge_grad), edge_dot=p(self.edge_dot),
                    edge_nz_lo_inv=p(self.extents[0]), edge_nz_hi1=p(self.extents[1]))

    def struct(self, lo, hi):
        """d3m_fit_targets of final records (views lo..hi): no scratch, no scalars to apply"""
        return _lib.D3MFitTargets(**self.fields(lo, hi), flags=0)


def _pixel_records(B, S, dev, grad_depth=False, extents=None, zero_extents=False):
    """The records' buffers.  `extents`: where the caller keeps them (inside the edge plan's blob); else a [2,B,2,S] tensor,
    UNINITIALISED (the lit node zeroes it in its first launch; the epilogue's adjoint writes it) or zeroed (zero_extents)."""
    eg = torch.empty(B, S, S, 4, dtype=torch.float32, device=dev)
    ed = torch.empty(B, S, S, 2, dtype=torch.float32, device=dev)
    if extents is None:
        extents = (torch.zeros if zero_extents else torch.empty)(2, B, 2, S, dtype=torch.int32, device=dev)
    gd = torch.empty(B, S, S, dtype=torch.float32, device=dev) if grad_depth else None
    return _Records(eg, ed, extents, gd)


def _image_grad_struct(g_img, pooled):
    """d3m_fit_targets of the DIRECT read: the edge gradient reads the output (alpha) image's gradient in place"""
    return _lib.D3MFitTargets(grad_alpha_map=_lib.ptr(g_img), flags=_lib.GRAD_OF_OUTPUT_IMAGE | (_lib.FIT_POOLED if pooled else 0))


class _FitState(NamedTuple):
    """A fit objective evaluated in the lit render node's pass (or on its finished images, core.losses): targets, scratch
    and value per view group and, with a backward pass to come, its gradient (minus the loss's gradient) as records."""
    rgb_t: torch.Tensor                     # [B,3,s,s]
    depth_t: torch.Tensor                   # [B,s,s]
    alpha_t: torch.Tensor                   # [B,s,s]
    mask: torch.Tensor                      # [B,s,s]
    scratch: list                           # per view group: d3m_render_fit_scratch_floats
    loss: torch.Tensor                      # [G]: the value of each view group
    mask_sum: Optional[torch.Tensor]        # [1]: the photometric normaliser (None: sum(mask), no gradient wanted)
    pooled: bool                            # an objective on the 2x2-pooled images (anti-aliasing)
    records: Optional[_Records]
    tile_void: Optional[torch.Tensor] = None    # [B,n16,n16] uint8: the targets' void tiles (target_void_summary) or None

    def struct(self, k, lo, hi, grad_loss=None, flags=0):
        """d3m_fit_targets of view group k (views lo..hi): forward's `fit` (grad_loss None) / backward's `unscaled`."""
        rec = self.records.fields(lo, hi) if self.records is not None else {}   # (the gradient as per-pixel records)
        if self.records is not None and self.pooled:
            flags = int(flags) | _lib.FIT_POOLED
        return _lib.D3MFitTargets(
            rgb_target=_lib.ptr(self.rgb_t[lo:hi]), depth_target=_lib.ptr(self.depth_t[lo:hi]),
            alpha_target=_lib.ptr(self.alpha_t[lo:hi]), mask=_lib.ptr(self.mask[lo:hi]), scratch=_lib.ptr(self.scratch[k]),
            loss=_lib.ptr(self.loss[k:k + 1]), grad_loss=_lib.ptr(grad_loss), mask_sum=_lib.ptr(self.mask_sum), **rec,
            flags=int(flags), tile_void=_lib.ptr(None if self.tile_void is None else self.tile_void[lo:hi]))


class _TargetVoidCache(BuiltCache):
    what = "the fit targets' void-tile summary"


# Two sets of targets at most: an entry holds its four target tensors (at the headline's size about 200 MB) to keep their
# addresses taken, and a caller whose targets are new tensors every step (a tracker; targets f32c has to copy) should pin no
# more than that.  Such a caller also pays the summary's kernel every step (61 us at the headline's size, more than void
# tiles save there): D3M_FIT_VOID_TILES=0 is for it.
_target_void_cache = _TargetVoidCache(size=2)


def fit_void_tiles_enabled():
    """D3M_FIT_VOID_TILES=0 keeps d3m_fit_targets.tile_void NULL: the fused objective's pass does all of its work in every
    tile (A/B runs and the parity tests)."""
    return os.environ.get("D3M_FIT_VOID_TILES", "1") != "0"


def _build_target_void(rgb_t, depth_t, alpha_t, mask):
    B, S = mask.shape[0], mask.shape[-1]
    n16 = (S + 15) // 16
    out = torch.empty(B, n16, n16, dtype=torch.uint8, device=mask.device)
    _lib.check(_lib.lib().d3m_fit_target_summary(_lib.ptr(rgb_t), _lib.ptr(depth_t), _lib.ptr(alpha_t), _lib.ptr(mask),
                                                 _lib.ptr(out), B, S, _lib.stream_ptr()), "d3m_fit_target_summary")
    return out


def target_void_summary(rgb_t, depth_t, alpha_t, mask, build=_build_target_void, capturing=None):
    """One byte per (view, 16 x 16 tile of the output image): 1 where the targets ask nothing of the fit objective (alpha
    target 0, mask 0, finite rgb / depth targets at every pixel of the tile) -- d3m_fit_targets.tile_void.  The targets of a
    fit are constants (MultiViewFit.set_targets_from, Renderer.fit_targets), so the summary is built ONCE per set of target
    tensors -- keyed by their addresses and versions -- on the first eager step, and never inside a stream capture: a
    capture that finds none takes the pass without void tiles (None), it does not raise.  None as well under
    D3M_FIT_VOID_TILES=0.
    Like _vec3_host, the key only sees writes that bump a tensor's `_version`: after a write that does not (through
    `.data`, a raw pointer, another library), call invalidate_target_void_summaries().
    A CAPTURED step replays with the summary it was captured with -- no check can run at replay: after ANY write to the
    targets of a captured step (a `copy_` into persistent target buffers included) the step must be captured again, or such a
    caller runs under D3M_FIT_VOID_TILES=0.  Without the summary the kernels read the targets at replay and need neither."""
    if not fit_void_tiles_enabled():
        return None
    targets = (rgb_t, depth_t, alpha_t, mask)
    key = tuple(tensor_key(t) for t in targets)
    if capturing is None:
        capturing = torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()
    if capturing and key not in _target_void_cache:
        return None
    return _target_void_cache.get(key, lambda: build(*targets), holders=targets)


def invalidate_target_void_summaries():
    """Forget every cached summary of fit targets (target_void_summary): the next eager step rebuilds its own."""
    _target_void_cache.clear()


def _front_clears(clears):
    """[(device pointer, bytes)] -> the (pointers, sizes, count) arguments of d3m_lit_front"""
    assert len(clears) <= _lib.FRONT_RANGES
    n = max(1, len(clears))
    return (ctypes.c_void_p * n)(*[c[0] for c in clears]), (ctypes.c_size_t * n)(*[c[1] for c in clears]), len(clears)


def _check_deterministic(det):
    """The deterministic switch a node's forward pass ran with (`det`) must hold for its backward pass too: forward has
    built the ascending visibility list and the CSR adjacency for it (or not), and the library reads the switch again at
    launch time (the large-face fallback), so following either one alone would give a half-deterministic pass."""
    if _deterministic() != det:
        raise RuntimeError("the deterministic mode (D3M_DETERMINISTIC, d3m_set_deterministic) was %s for this render node's "
                           "forward pass and is %s for its backward pass: the deterministic() block must enclose backward "
                           "as well as forward" % (("on", "off") if det else ("off", "on")))


class LitImagesLink:
    """What a fit objective evaluated on the finished images of ONE lit render node (core.losses.multiview_fit_loss on
    the outputs of Renderer.render) shares with that node's backward: the objective's gradient as the edge gradient's
    per-pixel records (`fit_state`, a _FitState as _RasterizeLit keeps for its own fused objective), the scalar gradient of
    the loss, and the zero-stride zero images the loss node returns instead of gradient images.  Created on the node's state."""

    def __init__(self, state, fit_state, shapes, zero):
        self.fit_state, self.shapes, self.zero = fit_state, shapes, zero
        state.link = self
        self.grad_loss = None
        self.finish_pending = False     # the objective's totals are still partial sums (D3M_FIT_FINISH_DEFERRED)
        self.pending = False            # the loss node's backward ran and the render node's has not consumed it yet
        # The images themselves are NOT kept here: the render node's context holds this link, and an image holds that
        # context as its grad_fn -- a reference cycle through the autograd graph.  The loss node (which saved them) lends
        # them for the time between its backward and the render node's.
        self.images = None

    def dummies(self):
        return tuple(self.zero.expand(s) for s in self.shapes)

    def end_of_pass(self):
        """Queued by the loss node's backward on the autograd engine (queue_callback): runs when that backward pass ends.
        `pending` still set = the render node was not part of the pass, so whoever asked for the images' gradients got
        the zero-stride zeros: fail loudly, and never leave the flag (or the lent images) for a later, unrelated pass."""
        stale, self.pending, self.images = self.pending, False, None
        if stale:
            raise RuntimeError(
                "multiview_fit_loss was linked to the lit render node that produced its images, but this backward pass "
                "stopped at the images (torch.autograd.grad(loss, images) / backward(inputs=images)): their gradient only "
                "exists as the render node's walk records.  Build the loss with multiview_fit_loss(..., link=False) to "
                "differentiate with respect to the images themselves.")

    def is_dummy(self, g):
        return g is not None and g.data_ptr() == self.zero.data_ptr() and all(st == 0 for st in g.stride())

    def add_gradient_images(self, g_rgb, g_alpha, g_depth):
        """other consumers of the images sent gradients too: the objective's own gradient images after all
        (d3m_fit_loss_backward), added to what arrived"""
        rgb, depth, alpha = self.images
        fs = self.fit_state
        B, _, H, W = rgb.shape
        if self.finish_pending:         # (a registered objective whose finish was left to the records route: do it now)
            self.finish_pending = False
            fit_c = fs.struct(0, 0, B)
            # (the pass ran at the INTERNAL size: twice the images' with anti-aliasing)
            _lib.check(_lib.lib().d3m_fit_finish(ctypes.byref(fit_c), B, H * (2 if fs.pooled else 1),
                                                 _lib.stream_ptr()), "d3m_fit_finish")
        own = [torch.empty_like(t) for t in (rgb, depth, alpha)]
        t = (rgb, fs.rgb_t, depth, fs.depth_t, alpha, fs.alpha_t, fs.mask)
        _lib.check(_lib.lib().d3m_fit_loss_backward(*[_lib.ptr(x) for x in t], _lib.ptr(fs.scratch[0]), _lib.ptr(self.grad_loss),
                                                    _lib.ptr(own[0]), _lib.ptr(own[1]), _lib.ptr(own[2]), B, H, W,
                                                    _lib.stream_ptr()), "d3m_fit_loss_backward")
        add = lambda g, o: o if (g is None or self.is_dummy(g)) else g + o
        return add(g_rgb, own[0]), add(g_alpha, own[2]), add(g_depth, own[1])


def lit_images_link(rgb, depth, alpha):
    """The lit render node (its autograd context) whose three output images these are -- rgb, depth and alpha exactly as
    rasterize_lit() / Renderer.render() returned them, one pipeline, gradients wanted, no objective linked yet (with
    anti-aliasing only a node that was given the objective's targets up front: fit_hint) -- or None."""
    fn = rgb.grad_fn
    if fn is None or fn is not depth.grad_fn or fn is not alpha.grad_fn or not isinstance(fn, _RasterizeLit._backward_cls):
        return None
    if (rgb.output_nr, alpha.output_nr, depth.output_nr) != (0, 1, 2):
        return None
    st = fn.state
    if st.fit is not None or st.link is not None:
        return None
    if (st.aa and st.hint is None) or not (st.ra and st.rd) or len(st.groups) != 1 or fn.maps.get("visibility") is None:
        return None
    return fn


def _checked_sink(grad_sink, vertices, textures):
    """`grad_sink` = (grad_vertices, grad_textures | None, loss [1]): caller-owned buffers the lit node writes its results
    into in place (MultiViewFit: views of the flat all-reduce buffer).  They are RAW destinations of kernels that write
    vertices.numel() / textures.numel() floats, so they are used only when they fit this call exactly -- shape, float32,
    contiguous, same device; anything else (a per-view mesh [B,V,3], another V or F, a sink left over from another fit)
    gets fresh buffers instead of an out-of-bounds write."""
    if grad_sink is None:
        return None
    gv, gt, loss = grad_sink

    def fits(buf, like):
        return (torch.is_tensor(buf) and buf.dtype == torch.float32 and buf.is_contiguous() and buf.device == like.device
                and tuple(buf.shape) == tuple(like.shape))
    if not fits(gv, vertices) or (gt is not None and not fits(gt, textures)):
        return None
    if not (torch.is_tensor(loss) and loss.dtype == torch.float32 and loss.numel() == 1 and loss.device == vertices.device):
        return None
    return grad_sink


@dataclasses.dataclass(eq=False)
class _LitState:
    """What the lit render node's forward pass decided, kept on its context for backward -- which decides none of it again
    -- and for the fit objectives linked to the node (core.losses)."""
    S: int                                  # the internal size (twice the output's with anti-aliasing)
    eps: float
    aa: bool
    ra: bool                                # alpha and depth returned (rgb always is)
    rd: bool
    fill_back: bool
    light: tuple                            # (ia, idr, colour_ambient, colour_directional, direction) by value, or None
    Bl: int                                 # batch of the per-face light (1: one shared mesh)
    groups: list                            # the view groups' (lo, hi)
    need_grad: bool
    need_geom: bool                         # a gradient for the mesh: edge gradient, depth gradient, light / camera adjoints
    need_tex: bool
    need_vert: bool                         # the light's adjoint reaches the world-space vertices
    gathered: bool                          # backward runs the gathered texture / depth pass
    det: bool                               # the deterministic backward pass (checked against the switch in backward)
    serial: bool                            # every branch on the forking stream (_serial_branches)
    plan_open: bool                         # forward left the visibility list / plan branch open (defer_plan_join)
    camera: Any                             # the camera inside the node (its parameter block) or None
    cam_keep: Any
    grad_sink: Any                          # _checked_sink
    fit: Optional[_FitState]                # the node's own fused objective (rasterize_lit_fit)
    hint: Optional[_FitState]               # a registered objective (fit_hint), evaluated in the pass that wrote the images
    hint_mask_sum_given: bool               # ... with the caller's normaliser (else the node took sum(mask))
    finish_deferred: bool = False           # the objective's finish is left to backward's gathered pass (FIT_FINISH_DEFERRED)
    pre: Any = None                         # backward's buffers, allocated and zeroed by forward (_backward_buffers; one use)
    link: Optional[LitImagesLink] = None    # a fit objective evaluated on the finished images (set by LitImagesLink)
    dlight: Any = None                      # the light read from device memory (normalize_light's five tensors) or None
    need_lp: tuple = (False,) * 5           # which of them want a gradient (autograd inputs of the node)
    need_mesh: bool = False                 # the mesh (vertices or screen vertices) wants a gradient
    need_cp: tuple = (False,) * 6           # which of the camera's parameters want one (cameras.camera_inputs order)
    adjacency: Any = None                   # det with a gradient for the mesh: the index tensor's row_gather.Adjacency


# _backward_buffers: the vertex accumulators, the texture / light gradients of batch B and where each view group's gathered
# pass writes them (gt_g / gl_g; batch 1: the groups' sums, added up behind the join), the gathered pass's workspace (one
# pipeline: PRECLEARED), the ranges to zero, and the deterministic mode's per-view light, its gradient, K4's / K6's arrays.
_BackwardBuffers = collections.namedtuple("_BackwardBuffers", "grad_sv grad_vertices grad_textures gt_g grad_light gl_g lit_ws "
                                                              "clears det_light det_gl det_k4 det_k6")


def _backward_buffers(st, vertices, textures, light, B, V, Ft, ts, ws_stream=None):
    """The lit node's backward accumulators, the gathered pass's workspace and the ranges of them to zero before its
    kernels run (`clears`).  Called by backward (ws_stream: the stream of its gathered pass, whose cached workspace it
    takes) or, for a caller that runs backward right behind forward, by forward (a workspace of its own)."""
    L = _lib.lib()
    dev, groups, sink = vertices.device, st.groups, st.grad_sink
    G = len(groups)
    grad_sv = torch.empty(B, V, 3, dtype=torch.float32, device=dev) if st.need_geom else None
    grad_vertices = grad_textures = gt_g = grad_light = gl_g = lit_ws = None
    det_light = det_gl = det_k4 = det_k6 = None
    if st.need_vert:
        grad_vertices = sink[0] if (sink is not None and st.camera is not None) else torch.empty_like(vertices)
    if st.gathered:
        if textures.shape[0] == 1:
            gt_g = [sink[1] if (sink is not None and sink[1] is not None and G == 1) else torch.empty_like(textures)
                    for _ in groups]
        else:
            grad_textures = torch.empty_like(textures)
            gt_g = [grad_textures[lo:hi] for lo, hi in groups]
        if st.need_vert or any(st.need_lp):
            if st.Bl == 1:
                gl_g = [torch.empty_like(light) for _ in groups]
            else:
                grad_light = torch.empty_like(light)
                gl_g = [grad_light[lo:hi] for lo, hi in groups]
    clears = [_lib.tensor_range(t) for t in (grad_sv, grad_vertices) if t is not None]
    if st.det:
        # per-VIEW light gradients (one contribution per entry), the two per-face arrays of K4 and K6
        Fp = 2 * Ft if st.fill_back else Ft
        if st.need_vert or any(st.need_lp):
            det_light = light.expand(B, Fp, 3).contiguous() if st.Bl == 1 else light
            det_gl = torch.empty(B, Fp, 3, dtype=torch.float32, device=dev)
        if st.need_geom:
            det_k4 = torch.empty(B, Fp, 3, 3, dtype=torch.float32, device=dev)
            clears.append(_lib.tensor_range(det_k4))
            if st.rd:
                det_k6 = torch.empty(B, Fp, 3, 3, dtype=torch.float32, device=dev)
                clears.append(_lib.tensor_range(det_k6))
    if st.gathered and G == 1:
        nbytes = int(L.d3m_backward_textures_lit_workspace_bytes(B, Ft, int(st.fill_back), ts))
        if ws_stream is None:
            lit_ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        else:
            with torch.cuda.stream(ws_stream):     # (scratch is cached per stream: the stream the pass will run on)
                lit_ws = ops._workspace("lit", nbytes, dev)
        # what d3m_backward_textures_lit (with a visibility blob) zeroes in front of its kernels
        gl = det_gl if det_gl is not None else (gl_g[0] if gl_g is not None else None)
        ptrs, sizes = (ctypes.c_void_p * 4)(), (ctypes.c_size_t * 4)()
        n = L.d3m_backward_textures_lit_clear_ranges(
            _lib.ptr(grad_textures if grad_textures is not None else gt_g[0]), textures.shape[0], _lib.ptr(gl),
            B if det_gl is not None else st.Bl, B, Ft, int(st.fill_back), ts, _lib.ptr(lit_ws), 1, ptrs, sizes)
        clears += [(ptrs[i], sizes[i]) for i in range(n)]
    return _BackwardBuffers(grad_sv, grad_vertices, grad_textures, gt_g, grad_light, gl_g, lit_ws, clears, det_light,
                            det_gl, det_k4, det_k6)


class _RasterizeLit(torch.autograd.Function):
    """render / render_rgb in one autograd node with fill_back and lighting applied on the fly
    (d3m_face_light + d3m_render_lit_epilogue / d3m_backward_textures_lit): the per-view
    cat(textures, permuted) * light array of NR/renderer.py:155-167 is never materialised and textures /
    mesh may be shared by all views (batch 1).  The node starts from the SCREEN-space vertices: the face gather
    (vertices_to_faces + fill_back) happens inside, and backward accumulates the face gradients straight into the
    gradient of those vertices (d3m_vertex_target) instead of filling a [B,F',3,3] array for a scatter pass.

    VIEW GROUPS.  Nothing couples the views of a batch (KCU:92,263), so the node may run them as `view_groups`
    contiguous groups, each a complete pipeline (binning -> tile pass -> epilogue; edge gradient beside the gathered
    texture / depth pass) on streams of its own, forked from and joined to the current stream inside this one node --
    inside a captured step: parallel branches of the graph.  The passes of a pipeline alternate between latency-bound
    (binning, crossing emit) and issue-bound (tile pass, line walk) kernels; two pipelines out of phase fill each other's
    gaps.  With a fused fit objective the groups are shards of it: each normalises by the mask sum of ALL views
    (mask_sum), so the group values and gradients add up exactly as ranks do (multiview.py)."""

    @staticmethod
    def forward(ctx, screen_vertices, vertices, tri, textures, light_cfg, fill_back, image_size, anti_aliasing, near,
                far, eps, background_color, return_rgb, return_alpha, return_depth, fit=None, view_groups=1,
                defer_plan_join=False, camera=None, grad_sink=None, fit_hint=None, l_ia=None, l_idr=None, l_ca=None,
                l_cd=None, l_dir=None, c_eye_or_t=None, c_at_or_direction=None, c_up=None, c_rot=None, c_K=None,
                c_dist=None):
        # l_*: the light read from device memory (normalize_light; light_on_device) -- autograd inputs, so that backward
        # can return their gradients; None: the light of light_cfg, passed to the kernels by value.  c_*: the parameter
        # tensors of `camera` (cameras.camera_inputs), autograd inputs likewise: the block's own tensors, read by the kernels
        L = _lib.lib()
        vertices, textures = f32c(vertices), f32c(textures)
        tri = tri.to(torch.int32).contiguous()
        dev = vertices.device
        grad_sink = _checked_sink(grad_sink, vertices, textures)
        cam = cam_keep = basis = None
        if camera is not None:
            # THE CAMERA INSIDE THE NODE (`camera` = the parameter block of cameras._camera_struct, screen_vertices None):
            # the mesh is both projected and lit, i.e. `vertices` would receive two gradients that autograd then adds
            # with a kernel of its own; here the camera's adjoint is accumulated onto the light's (d3m_camera_backward_add)
            # and the node returns ONE gradient.  `grad_sink` = (grad_vertices [1,V,3], grad_textures, loss [1]) buffers
            # of the caller (MultiViewFit's flat all-reduce buffer): the results are produced in place, no packing copy.
            # The transform itself is part of the step's first launch (d3m_lit_front, below).
            from . import cameras
            cam, cam_keep = cameras._camera_struct(camera, dev)
            basis, basis_keep = cameras.basis_struct(camera)
            cam_keep = list(cam_keep) + basis_keep
            sv = torch.empty(camera["batch"], vertices.shape[1], 3, dtype=torch.float32, device=dev)
        else:
            sv = f32c(screen_vertices)
        B = sv.shape[0]
        Ft, V, ts = tri.shape[1], vertices.shape[1], textures.shape[2]
        Fp = 2 * Ft if fill_back else Ft
        if sv.shape[1] != V or tri.shape[0] not in (1, B):
            raise ValueError("screen_vertices must be [B, V, 3] and faces [1 or B, F, 3]")
        if textures.shape[0] not in (1, B) or textures.shape[1] != Ft:
            raise ValueError("textures must be [1 or B, num_faces, ts, ts, ts, 3] for the given faces")
        S = int(image_size) * 2 if anti_aliasing else int(image_size)
        ia, idr, ca, cd, direction = light_cfg
        dlight = None if l_ia is None else tuple(f32c(t) for t in (l_ia, l_idr, l_ca, l_cd, l_dir))
        need_lp = tuple(bool(x) for x in (tuple(ctx.needs_input_grad) + (False,) * 5)[21:26]) if dlight is not None \
            else (False,) * 5
        if dlight is None:
            cca, ccd, cdir = _vec3_host(ca), _vec3_host(cd), _vec3_host(direction)
        elif any(t.shape[0] not in (1, B) for t in dlight):
            raise ValueError("light parameters must have batch 1 or the number of views")
        # (a light given per view makes the per-face light per view, even for one shared mesh)
        light_per_view = dlight is not None and any(t.shape[0] > 1 for t in dlight)
        Bl = 1 if (vertices.shape[0] == 1 and tri.shape[0] == 1 and not light_per_view) else B
        light = torch.empty(Bl, Fp, 3, dtype=torch.float32, device=dev)        # (filled by the first launch, below)
        background = _background_tensor(background_color, dev)
        # which of the camera's parameters want a gradient (the camera inside the node only)
        need_cp = tuple(bool(x) for x in (tuple(ctx.needs_input_grad) + (False,) * 6)[26:32]) if camera is not None \
            else (False,) * 6
        need_grad = any(ctx.needs_input_grad[:4]) or any(need_lp) or any(need_cp)
        # the GEOMETRY side of backward (edge gradient K4, depth gradient K6, the light's and the camera's adjoints) only
        # exists for a mesh or a camera that wants a gradient: a texture-only optimisation builds no plan and walks no line
        need_mesh = bool(ctx.needs_input_grad[0] or ctx.needs_input_grad[1])
        need_geom = need_mesh or any(need_cp)
        need_tex = bool(ctx.needs_input_grad[3])
        need_vert = bool(ctx.needs_input_grad[1]) and (not _host_zero(idr) if dlight is not None else idr != 0)
        groups = _group_bounds(B, view_groups)
        G = len(groups)
        # Everything the branches write is allocated here, on the current stream: no tensor changes its owning stream.
        # Coverage comes straight from the indexed mesh: the binning pass reads the faces through `tri` and leaves the
        # dense copy of those that can own a pixel in `faces` (no vertices_to_faces pass); every other entry stays
        # UNINITIALISED (torch.empty: possibly NaN) and is never read -- later passes only touch pixel owners.
        faces = torch.empty(B, Fp, 3, 3, dtype=torch.float32, device=dev)
        m = {"face_index_map": torch.empty((B, S, S), dtype=torch.int32, device=dev),
             "weight_map": torch.empty(B, S, S, 3, dtype=torch.float32, device=dev),
             "depth_map": torch.empty((B, S, S), dtype=torch.float32, device=dev),
             "face_inv_map": const_tensor([0.0], dev),       # the 1-element stand-in of a disabled map (no fill launch)
             "rgb_map": torch.empty(B, S, S, 3, dtype=torch.float32, device=dev),
             "alpha_map": torch.empty(B, S, S, dtype=torch.float32, device=dev) if return_alpha else None}
        # which faces own a pixel is only needed by the backward pass: one blob per group (this node's backward may run
        # late, so they are its own buffers), built beside the sampling / epilogue pass
        vis = [torch.empty(int(L.d3m_visibility_bytes(hi - lo, Fp)), dtype=torch.uint8, device=dev) for lo, hi in groups] \
            if need_grad else None
        # ... and so is the edge gradient's plan (where the visible faces' edges cross the pixel grid, by image line):
        # geometry only, so it is built on the same branch and the backward pass starts with the line walk
        plan = [torch.empty(int(L.d3m_edge_plan_bytes(hi - lo, Fp, S)), dtype=torch.uint8, device=dev) for lo, hi in groups] \
            if need_geom else None
        s_out = S // 2 if anti_aliasing else S
        rgb = alpha = depth = loss_g = fit_state = None
        # A REGISTERED objective (Renderer.fit_targets -> `fit_hint`): the node returns the IMAGES, as render() does, and the
        # pass that writes them also evaluates the objective the caller is about to evaluate on them and leaves its gradient
        # as walk records (the fused objective's pass with images_out): core.losses.multiview_fit_loss, handed these very
        # images and targets, then finds value and records here instead of re-reading the images (`_LitState.hint`).
        hinted = fit is None and fit_hint is not None and return_alpha and return_depth and need_grad and G == 1
        if fit is None:
            rgb = torch.empty(B, 3, s_out, s_out, dtype=torch.float32, device=dev)
            alpha = torch.empty(B, s_out, s_out, dtype=torch.float32, device=dev) if return_alpha else None
            depth = torch.empty(B, s_out, s_out, dtype=torch.float32, device=dev) if return_depth else None
        mask_sum_given = False
        objective = (fit_hint, (rgb, depth, alpha)) if hinted else fit      # (targets, images_out | None)
        if objective is not None:
            # the fit objective is evaluated where the images are produced: they are never written (rasterize_lit_fit)
            if not (return_alpha and return_depth):
                raise ValueError("the fused fit objective needs rgb, alpha and depth")
            targets, images_out = objective         # targets = (rgb_t, depth_t, alpha_t, mask[, mask_sum])
            *targets, mask_sum = (tuple(targets) + (None,))[:5]
            rgb_t, depth_t, alpha_t, mask = (f32c(t) for t in targets)
            mask_sum_given = mask_sum is not None
            mask_sum = f32c(mask_sum).reshape(1) if mask_sum is not None else None
            if images_out is not None:
                # the images as a by-product of the same pass (caller's buffers, not differentiable outputs)
                rgb, depth, alpha = images_out
                for t, shape in ((rgb, (B, 3, s_out, s_out)), (depth, (B, s_out, s_out)), (alpha, (B, s_out, s_out))):
                    if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
                        raise ValueError("images_out must be contiguous float32 (rgb [B,3,s,s], depth [B,s,s], alpha [B,s,s])")
            if tuple(rgb_t.shape) != (B, 3, s_out, s_out) or any(tuple(t.shape) != (B, s_out, s_out) for t in (depth_t, alpha_t, mask)):
                raise ValueError("fit targets must be rgb [B,3,s,s] and depth / alpha / mask [B,s,s] at the output size")
            if mask_sum is None and (G > 1 or need_grad):
                # view groups are shards of the objective and need the normaliser of the whole batch; and with it known
                # up front the pass below can leave the gradient as the edge gradient's per-pixel records
                mask_sum = mask.sum().reshape(1)
            loss_g = grad_sink[2] if (grad_sink is not None and G == 1) else torch.empty(G, dtype=torch.float32, device=dev)
            scratch = [torch.empty(int(L.d3m_render_fit_scratch_floats(hi - lo, S)), dtype=torch.float32, device=dev)
                       for lo, hi in groups]
        cur = torch.cuda.current_stream()
        det = need_grad and _deterministic()
        adjacency = None
        if det:
            _RasterizeLit._deterministic_supported(G, tri, vertices, ts, 0.0 if _host_zero(idr) else 1.0,
                                                   ctx.needs_input_grad[1], light_per_view)
            if need_geom:       # (both of backward's gathers: need_vert implies it)
                adjacency = vertex_adjacency(tri, V)
        # (LitFitManual: every kernel on the caller's stream -- the step is cut BETWEEN kernels of one stream)
        manual = isinstance(ctx, _ManualContext)
        serial = G == 1 and (det or manual or _serial_branches(B, Ft, S))
        mains = [cur] + [_side_stream(dev, k) for k in range(1, G)]
        auxs = [_side_stream(dev, G + k, serial) for k in range(G)]
        own_extents = False
        if objective is not None:
            # with a backward pass to come, the same pass leaves the objective's gradient behind -- minus the gradient of the
            # loss, only known later -- in the form its readers want: the edge gradient's per-pixel records at the internal
            # size (what d3m_backward_pixel_map would otherwise pack from gradient maps: no pixel pass in backward at all),
            # the lines' non-zero extents, and the depth gradient as a map.  With anti-aliasing an output pixel is the mean
            # of four internal ones: each gets a quarter of its gradient (D3M_FIT_POOLED; round 4 left unscaled maps here
            # and packed them in backward).
            records = None
            if need_grad:
                # the lines' non-zero extents (zero before the objective's pass fills them): when the plan is built in front
                # of that pass on the same stream, inside the plan's blob, cleared by the plan's own clear; else a tensor of
                # their own, zeroed by the first launch (below)
                extents = None
                if serial and plan is not None:
                    each = ctypes.c_size_t(0)
                    off = int(L.d3m_edge_plan_extents_offset(B, Fp, S, ctypes.byref(each)))
                    extents = tuple(plan[0][off + j * each.value: off + j * each.value + B * 2 * S * 4].view(torch.int32)
                                    .view(B, 2, S) for j in range(2))
                own_extents = extents is None
                records = _pixel_records(B, S, dev, grad_depth=True, extents=extents)
            # VOID TILES: where neither the targets nor the mesh ask anything of a tile, the pass does no memory work there
            # (d3m_fit_targets.tile_void).  Records form without anti-aliasing only; not for a REGISTERED objective, whose
            # backward pass may turn out to be the images' after all and then reads rgb_map / alpha_map at every pixel
            # (d3m_output_epilogue_backward_records).  Backward hands the library the same struct, so both passes agree.
            tile_void = None
            if records is not None and not anti_aliasing and not hinted:
                tile_void = target_void_summary(rgb_t, depth_t, alpha_t, mask)
            fit_state = _FitState(rgb_t, depth_t, alpha_t, mask, scratch, loss_g, mask_sum, bool(anti_aliasing), records,
                                  tile_void)
        st = _LitState(S=S, eps=float(eps), aa=bool(anti_aliasing), ra=bool(return_alpha), rd=bool(return_depth),
                       fill_back=bool(fill_back), light=(float(ia), float(idr), ca, cd, direction) if dlight is None else None,
                       Bl=Bl, groups=groups, need_grad=need_grad, need_geom=need_geom, need_tex=need_tex,
                       need_vert=need_vert, gathered=need_tex or need_vert or any(need_lp) or any(need_cp), det=det,
                       serial=serial,
                       plan_open=bool(plan is not None and defer_plan_join and G == 1),   # (G > 1: capture crashes, as above)
                       camera=camera, cam_keep=cam_keep, grad_sink=grad_sink,
                       fit=None if hinted else fit_state, hint=fit_state if hinted else None,
                       # (whether the registered objective brought its normaliser or the node took sum(mask):
                       #  multiview_fit_loss only rides on the node's result when it is asked for the same one)
                       hint_mask_sum_given=hinted and mask_sum_given, dlight=dlight, need_lp=need_lp,
                       need_mesh=need_mesh, need_cp=need_cp, adjacency=adjacency)
        # THE STEP'S FIRST LAUNCH (d3m_lit_front): the camera transform (with its look_at basis), the per-face light and
        # every clear the operators below would otherwise each launch for themselves -- the forward workspace's counters (or
        # z-buffer), the plan's, the objective's arrival tickets, the lines' extents -- and, for a caller that runs backward
        # right behind forward (defer_plan_join: MultiViewFit's step; LitFitManual), the backward pass's accumulators and
        # masks too, allocated here for that purpose (`_LitState.pre`): five launches of round 4's step are block ranges of
        # one.  One pipeline only: view groups keep their own clears.
        clears, pre = [], None
        flags_fwd = flags_plan = flags_fit = 0
        ws0 = ops._workspace("fwd", L.d3m_forward_workspace_bytes(groups[0][1] - groups[0][0], Fp, S), dev)
        if G == 1:
            nb = int(L.d3m_forward_clear_bytes(B, Ft, int(bool(fill_back)), S, ws0.numel()))
            if nb:
                clears.append((ws0.data_ptr(), nb))
                flags_fwd = _lib.PRECLEARED
            if plan is not None:
                clears.append((plan[0].data_ptr(), int(L.d3m_edge_plan_clear_bytes(B, Fp, S))))
                flags_plan = _lib.PRECLEARED
            if fit_state is not None:
                off = ctypes.c_size_t(0)
                nfl = int(L.d3m_render_fit_scratch_clear_range(B, S, ctypes.byref(off)))
                clears.append((fit_state.scratch[0].data_ptr() + 4 * off.value, 4 * nfl))
                flags_fit = _lib.PRECLEARED
        if own_extents:
            clears.append(_lib.tensor_range(fit_state.records.extents))
        if G == 1 and need_grad and (defer_plan_join or manual) and not det:
            pre = _backward_buffers(st, vertices, textures, light, B, V, Ft, ts)
            if len(clears) + len(pre.clears) <= _lib.FRONT_RANGES:
                clears += pre.clears
            else:
                pre = None
        # ... and the objective's finish (partial sums -> value) is left to a kernel that backward pass launches anyway
        if pre is not None and st.gathered and fit_state is not None and fit_state.records is not None:
            flags_fit |= _lib.FIT_FINISH_DEFERRED
        st.pre, st.finish_deferred = pre, bool(flags_fit & _lib.FIT_FINISH_DEFERRED)
        zp, zb, nz = _front_clears(clears)
        if dlight is None:
            _lib.check(L.d3m_lit_front(_lib.ptr(vertices), vertices.shape[0], ctypes.byref(cam) if cam is not None else None,
                                       ctypes.byref(basis) if basis is not None else None,
                                       _lib.ptr(sv) if cam is not None else None, B, V, _lib.ptr(tri), tri.shape[0], Ft,
                                       int(bool(fill_back)), _lib.ptr(light), Bl, float(ia), float(idr), cca, ccd, cdir,
                                       zp, zb, nz, _lib.stream_ptr()), "d3m_lit_front")
        else:       # (the light's rows are read by the kernel: a captured step reads the light at replay)
            _lib.check(L.d3m_lit_front_dev(_lib.ptr(vertices), vertices.shape[0], ctypes.byref(cam) if cam is not None else None,
                                           ctypes.byref(basis) if basis is not None else None,
                                           _lib.ptr(sv) if cam is not None else None, B, V, _lib.ptr(tri), tri.shape[0], Ft,
                                           int(bool(fill_back)), _lib.ptr(light), Bl, ctypes.byref(_light_struct(dlight)),
                                           zp, zb, nz, _lib.stream_ptr()), "d3m_lit_front_dev")
        # The visibility list and the plan are only read by backward.  A caller that runs backward right behind forward,
        # on the same stream and (if captured) in the same capture, may leave that branch open at the end of forward
        # (defer_plan_join): backward waits for the plan where it first needs it and joins the branch, which runs on
        # under the loss and the first backward passes.  The outputs are then only valid after backward.
        plan_ready = [] if st.plan_open else None
        for k in range(G):
            if mains[k] is not cur:
                mains[k].wait_stream(cur)
            # every branch enters (a capture) from the ORIGIN stream: a stream that joins through another branch's
            # event -- a fork of a fork -- crashes hipStreamEndCapture on ROCm 7.2
            if vis is not None and auxs[k] is not cur and auxs[k] is not mains[k]:
                auxs[k].wait_stream(cur)
        for k, (lo, hi) in enumerate(groups):
            Bg = hi - lo
            with torch.cuda.stream(mains[k]):
                tri_g, tex_g, light_g, bg_g = (_bslice(t, lo, hi) for t in (tri, textures, light, background))
                fi_g, wm_g, dm_g = m["face_index_map"][lo:hi], m["weight_map"][lo:hi], m["depth_map"][lo:hi]
                ws = ws0 if k == 0 else ops._workspace("fwd", L.d3m_forward_workspace_bytes(Bg, Fp, S), dev)
                _lib.check(L.d3m_forward_face_index_map_mesh(
                    _lib.ptr(sv[lo:hi]), _lib.ptr(tri_g), tri_g.shape[0], V, Ft, int(bool(fill_back)), _lib.ptr(faces[lo:hi]),
                    _lib.ptr(fi_g), _lib.ptr(wm_g), _lib.ptr(dm_g), None, Bg, S, float(near), float(far), _lib.ptr(ws),
                    ws.numel(), _lib.ptr(vis[k]) if vis is not None else None, vis[k].numel() if vis is not None else 0,
                    flags_fwd, _lib.stream_ptr()), "d3m_forward_face_index_map_mesh")
                if vis is not None and plan is None:
                    # (texture-only: the list is all backward needs -- on this stream, no branch)
                    _lib.check(L.d3m_visibility(None, _lib.ptr(vis[k]), vis[k].numel(), Bg, Fp, S, _lib.stream_ptr()),
                               "d3m_visibility")
                elif vis is not None:
                    # ONE FORK, BEHIND THE VISIBILITY LIST (round 5).  The list has two readers -- the plan (side branch) and
                    # backward's gathered pass (this stream) -- and the coverage pass two as well (the list, the sampling
                    # pass).  Forked behind coverage, a replayed graph's critical chain (coverage -> list -> plan -> line
                    # walk) carried two kernels with a second successor each, and each cost it ~5 us (trace of the 4-view
                    # shard: 5.8 us between k_bid_resolve and the list, 5.1 behind the list).  With the list on this
                    # stream, in front of the fork, only it has two successors; the sampling pass starts 5 us later on a
                    # chain that has 40 us to spare.  4 views 0.2747 -> 0.2709 ms, 8 views 0.4687 -> 0.4660 (same box).
                    vis_first = plan_ready is not None and auxs[k] is not mains[k]
                    if vis_first:
                        _lib.check(L.d3m_visibility(None, _lib.ptr(vis[k]), vis[k].numel(), Bg, Fp, S,
                                                    _lib.stream_ptr()), "d3m_visibility")
                    if auxs[k] is not mains[k]:
                        auxs[k].wait_stream(mains[k])
                    with torch.cuda.stream(auxs[k]):
                        # (its first step -- which faces own a pixel -- was left by the tile pass above)
                        if not vis_first:
                            _lib.check(L.d3m_visibility(None, _lib.ptr(vis[k]), vis[k].numel(), Bg, Fp, S,
                                                        _lib.stream_ptr()), "d3m_visibility")
                        _lib.check(L.d3m_edge_plan(_lib.ptr(faces[lo:hi]), _lib.ptr(fi_g), _lib.ptr(vis[k]), _lib.ptr(plan[k]),
                                                   plan[k].numel(), Bg, Fp, S, flags_plan, _lib.stream_ptr()), "d3m_edge_plan")
                        if plan_ready is not None:
                            plan_ready.append(torch.cuda.Event())
                            plan_ready[k].record(auxs[k])
                # (the objective's value is completed by the pass's own last workgroups: no finishing launch)
                fit_c = fit_state.struct(k, lo, hi, flags=flags_fit) if fit_state is not None else None
                # texture sampling + background blend + alpha + flip / pooling in one pass (no rgb_sampled round trip)
                _lib.check(L.d3m_render_lit_epilogue(
                    _lib.ptr(faces[lo:hi]), _lib.ptr(tex_g), tex_g.shape[0], _lib.ptr(light_g), light_g.shape[0],
                    _lib.ptr(fi_g), _lib.ptr(wm_g), _lib.ptr(dm_g), _lib.ptr(bg_g), bg_g.shape[0],
                    _lib.ptr(m["rgb_map"][lo:hi]), _lib.ptr(_bslice(m["alpha_map"], lo, hi)),
                    _lib.ptr(_bslice(rgb, lo, hi)), _lib.ptr(_bslice(alpha, lo, hi)), _lib.ptr(_bslice(depth, lo, hi)), Bg, Ft,
                    int(bool(fill_back)), S, ts, float(eps), int(bool(anti_aliasing)),
                    ctypes.byref(fit_c) if fit_c is not None else None, _lib.stream_ptr()), "d3m_render_lit_epilogue")
        for k in range(G):
            if mains[k] is not cur:
                cur.wait_stream(mains[k])
            if vis is not None and plan_ready is None:
                cur.wait_stream(auxs[k])
        m["visibility"] = vis
        m["edge_plan"] = plan
        m["plan_ready"] = plan_ready
        m["plan_stream"] = auxs[0]
        ctx.state = st
        ctx.maps = m
        ctx.save_for_backward(faces, vertices, tri, textures, light)
        if fit is not None:
            return loss_g.sum() if G > 1 else loss_g.reshape(())
        empty = torch.tensor([])
        return (rgb, alpha if return_alpha else empty, depth if return_depth else empty)

    @staticmethod
    def _deterministic_supported(G, tri, vertices, ts, idr, vertices_need_grad, light_per_view=False):
        """The deterministic backward pass covers one pipeline over ONE shared index tensor (and, for the light's adjoint,
        one shared mesh) with gathered texture passes (texture_size 2, 3 or 4) and one light for all views: anything else
        would silently fall back to float atomics in arrival order, so it raises instead."""
        if G != 1 or tri.shape[0] != 1 or ts not in (2, 3, 4) or (vertices_need_grad and idr != 0 and vertices.shape[0] != 1) \
                or light_per_view:
            raise NotImplementedError(
                "D3M_DETERMINISTIC / d3m_set_deterministic(1): the lit render node's reproducible backward pass needs "
                "view_groups == 1, faces of batch 1 (one shared topology), texture_size 2..4, one light for all views "
                "and, with directional light, vertices of batch 1")

    @staticmethod
    def backward(ctx, g_rgb, g_alpha=None, g_depth=None):
        halves = _RasterizeLit._backward_halves(ctx, g_rgb, g_alpha, g_depth)
        next(halves)                    # ... up to the point where the texture gradient is final
        try:
            next(halves)                # ... the edge gradient, the light's and the camera's adjoints
        except StopIteration as done:
            return done.value
        raise RuntimeError("_backward_halves yields once")

    @staticmethod
    def _backward_halves(ctx, g_rgb, g_alpha=None, g_depth=None):
        """The node's backward as a generator with ONE cut: it yields when everything on the TEXTURE side has been
        issued (the gathered texture / depth pass and the sum over views: grad_textures is final in stream order), and
        returns the gradients after the GEOMETRY side (edge gradient, light and camera adjoints).  Autograd runs both
        halves back to back (backward() above); LitFitManual stops in between, so that a camera-sharded fit can send the
        texture gradient on its way while the geometry side still runs (deep3dmap_amd/multiview.py).  With more than one
        view group the cut comes after the last group's passes have been issued (nothing to overlap)."""
        L = _lib.lib()
        st, m = ctx.state, ctx.maps
        _check_deterministic(st.det)
        faces, vertices, tri, textures, light = ctx.saved_tensors
        S, eps, ra, rd, fill_back, Bl, groups = st.S, st.eps, st.ra, st.rd, st.fill_back, st.Bl, st.groups
        dlight = st.dlight
        if dlight is None:
            ia, idr, ca, cd, direction = st.light
            by_value = (ia, idr, _vec3_host(ca), _vec3_host(cd), _vec3_host(direction))
        else:
            dl_c = _light_struct(dlight)
        need_geom, need_tex, need_vert, gathered, det = st.need_geom, st.need_tex, st.need_vert, st.gathered, st.det
        dev, B, G = faces.device, faces.shape[0], len(groups)
        Ft, V, ts = tri.shape[1], vertices.shape[1], textures.shape[2]
        # a caller that runs backward right behind forward had its buffers allocated AND zeroed by the forward's first
        # launch (`pre`: one use -- a second backward over the same graph allocates and clears its own).  (No gradient for
        # the mesh wanted -- a texture-only optimisation: no screen-space accumulator, no edge gradient, no depth gradient,
        # no camera adjoint; the node returns None for the vertices.)
        bufs, st.pre = st.pre, None
        grad_loss = records = None
        # A fit objective evaluated on this node's finished images (core.losses.multiview_fit_loss -> LitImagesLink) has left
        # its gradient as per-pixel records and sends zero-stride ZERO images back: if those are all that arrived, backward
        # is the fused objective's (no gradient images exist); if other consumers of the images added theirs, the
        # objective's gradient images are materialised after all and added.
        fit, link = st.fit, st.link
        if fit is None and link is not None and link.pending:
            link.pending = False
            if link.is_dummy(g_rgb) and link.is_dummy(g_alpha) and link.is_dummy(g_depth):
                fit, g_rgb = link.fit_state, link.grad_loss
            else:
                g_rgb, g_alpha, g_depth = link.add_gradient_images(g_rgb, g_alpha, g_depth)
            link.images = None
        if fit is None:
            # the adjoint of the output epilogue (un-pool, un-flip, CHW -> HWC) writes the rgb / alpha gradients straight
            # as the edge gradient's per-pixel records (what d3m_backward_pixel_map would pack from gradient maps: one
            # pass over the pixels instead of two, no [B,S,S,3] / [B,S,S] gradient maps); the depth gradient as a map
            g_depth_map = torch.empty(B, S, S, dtype=torch.float32, device=dev) if rd else None
            records = _pixel_records(B, S, dev)
            _lib.check(L.d3m_output_epilogue_backward_records(
                _lib.ptr(f32c(g_rgb)), _lib.ptr(f32c(g_alpha) if ra else None), _lib.ptr(f32c(g_depth) if rd else None),
                _lib.ptr(m["face_index_map"]), _lib.ptr(m["rgb_map"]), _lib.ptr(m["alpha_map"] if ra else None),
                _lib.ptr(records.edge_grad), _lib.ptr(records.edge_dot), _lib.ptr(records.extents[0]),
                _lib.ptr(records.extents[1]), _lib.ptr(g_depth_map), B, S, int(st.aa), _lib.stream_ptr()),
                "d3m_output_epilogue_backward_records")
        else:       # g_rgb is the gradient of the scalar objective; the maps were left by forward, minus their scalars
            g_depth_map = fit.records.grad_depth        # (the rgb / alpha gradients exist as per-pixel records)
            grad_loss = f32c(g_rgb).reshape(1)
        # K4 -> textures (separate buffers) -> K6, as NR/rasterize.py:141-151; both face gradients land in grad_sv,
        # and both passes run over the compacted list of the faces that own a pixel.  The edge gradient (K4: ~8
        # latency-bound launches) and the gathered texture / depth pass (K5+K6) are independent -- they only meet in
        # the float atomics on grad_sv -- so the second runs on a stream of its own, per view group.
        vis = m["visibility"]
        tex_shared, light_shared = textures.shape[0] == 1, Bl == 1
        sink = st.grad_sink
        # DETERMINISTIC (d3m_set_deterministic / D3M_DETERMINISTIC=1; one pipeline, one shared topology).  Everything the
        # pass adds up with float atomics in arrival order is produced per (view, face) by the lanes that own it and then
        # summed in a FIXED order instead:
        #   K4 -> its own dense [B,F',3,3] array (k_edge_gather's plain stores: the reference's layout), K6 -> another one
        #   (k_backward_textures_lit_faces with grad_faces and NO large-face fallback: a face's lanes own its sums whatever
        #   its size), both gathered per vertex over a CSR adjacency of the index tensor (d3m_vertex_gather);
        #   the light's gradient per VIEW ([B,F',3]: one contribution per entry), summed over the views by torch's ordered
        #   reduction, its adjoint gathered per vertex (d3m_face_light_backward_gather);
        #   the visibility list in ascending order (the library, same switch); every kernel on one stream.
        # The camera's adjoint and the sum of the per-view texel gradients already add in view order.  What stays
        # unordered: the plan's fallback for an undersized workspace (k_edge_overflow) -- see DESIGN.md section 6.
        # Forward decided it (st.det, checked above against the switch) and, with it, one stream and no `pre`.
        cur = torch.cuda.current_stream()
        mains = [cur] + [_side_stream(dev, k) for k in range(1, G)]
        auxs = [_side_stream(dev, G + k, st.serial) for k in range(G)]
        plan_ready = m["plan_ready"]
        # THE EDGE GRADIENT STAYS ON THE PLAN'S STREAM (round 4).  With the forward's branch left open (plan_ready), the
        # step's critical chain is coverage -> visibility list -> plan -> line walk -> gather: all but the first on the side
        # stream if the line walk is issued there too, right behind the plan's last kernel, instead of on the forking stream
        # behind an event -- a replayed graph pays ~9 us for every cross-queue edge whose producer has only just finished
        # (trace of the 4-view shard: scatter ends 190.0, the line walk starts 198.6).  The gathered texture / depth pass
        # takes the forking stream then; it only needs the visibility list, which forward built on that stream in front of
        # the fork (ONE FORK, BEHIND THE VISIBILITY LIST): no event.
        swap = st.plan_open and G == 1 and auxs[0] is not cur
        s_edges = [auxs[0]] if swap else mains
        s_gath = [mains[0]] if swap else auxs
        # The backward pass's clears -- the two vertex accumulators and what the gathered pass needs zeroed -- as ONE launch
        # in front of the branches (round 4: one here and one inside d3m_backward_textures_lit), or none at all (`pre`).
        if bufs is None:
            bufs = _backward_buffers(st, vertices, textures, light, B, V, Ft, ts, ws_stream=s_gath[0])
            _lib.zero_raw(bufs.clears)
        grad_sv, grad_vertices, grad_textures, grad_light = bufs.grad_sv, bufs.grad_vertices, bufs.grad_textures, bufs.grad_light
        gt_g, gl_g, det_gl, det_k4, det_k6 = bufs.gt_g, bufs.gl_g, bufs.det_gl, bufs.det_k4, bufs.det_k6
        lit_flags = _lib.PRECLEARED if bufs.lit_ws is not None else 0
        for k in range(G):
            if mains[k] is not cur:
                mains[k].wait_stream(cur)
            if gathered or st.plan_open:
                auxs[k].wait_stream(cur)
            if swap:
                # the line walk reads the plan.  Backward normally runs under the stream forward forked from (autograd
                # restores it), so auxs[k] IS the stream the plan was recorded on and needs no edge -- and must not get
                # one: a wait on an event of the waiting stream itself inside a capture makes hipStreamEndCapture segfault
                # (ROCm 7.2).  Driven under another current stream the side stream is another object: then it waits.
                if auxs[k].cuda_stream != m["plan_stream"].cuda_stream:
                    auxs[k].wait_event(plan_ready[k])
            elif st.plan_open:
                mains[k].wait_event(plan_ready[k])       # the forward's open branch: visibility + plan of this group
        for k, (lo, hi) in enumerate(groups):
            Bg = hi - lo
            tri_g, tex_g, light_g = (_bslice(t, lo, hi) for t in (tri, textures, light))
            fi_g, wm_g, dm_g = m["face_index_map"][lo:hi], m["weight_map"][lo:hi], m["depth_map"][lo:hi]
            target = _lib.D3MVertexTarget(_lib.ptr(grad_sv[lo:hi]), _lib.ptr(tri_g), V, Ft, tri_g.shape[0], int(fill_back)) \
                if need_geom else None
            rd_geom = rd and need_geom              # the depth gradient (K6) is the mesh's
            unscaled = None
            if fit is not None:
                # (the deferred finish belongs to the objective THIS node evaluated -- its own or the registered one -- not to
                #  a foreign state a linked loss built on the finished images)
                deferred = st.finish_deferred and (fit is st.fit or fit is st.hint)
                unscaled = fit.struct(k, lo, hi, grad_loss, flags=_lib.FIT_FINISH_DEFERRED if deferred else 0)
            elif records is not None:
                unscaled = records.struct(lo, hi)
            if gathered:
                with torch.cuda.stream(s_gath[k]):
                    ws = bufs.lit_ws if bufs.lit_ws is not None else \
                        ops._workspace("lit", L.d3m_backward_textures_lit_workspace_bytes(Bg, Ft, int(fill_back), ts), dev)
                    # the depth gradient (K6, add) rides along in the same pass over the faces' pixels.  Deterministic:
                    # per-view light gradient, K6 into its own per-face array, no vertex target (see DETERMINISTIC)
                    light_d = bufs.det_light if bufs.det_light is not None else light_g
                    gl_k = det_gl if det else (gl_g[k] if gl_g is not None else None)
                    _lib.check(L.d3m_backward_textures_lit(
                        _lib.ptr(faces[lo:hi]), _lib.ptr(tex_g), tex_g.shape[0], _lib.ptr(light_d), light_d.shape[0],
                        _lib.ptr(fi_g), _lib.ptr(wm_g), _lib.ptr(dm_g), None, _lib.ptr(gt_g[k]), _lib.ptr(gl_k),
                        _lib.ptr(g_depth_map[lo:hi]) if rd_geom else None, _lib.ptr(det_k6), Bg, Ft, int(fill_back), S, ts,
                        eps, _lib.ptr(ws), ws.numel(), ctypes.byref(target) if (rd_geom and not det) else None,
                        _lib.ptr(vis[k]), ctypes.byref(unscaled) if unscaled is not None else None, lit_flags,
                        _lib.stream_ptr()), "d3m_backward_textures_lit")
            if G == 1:
                yield "textures"        # (one pipeline: the texture side is complete in the order of its stream)
            if need_geom:
                with torch.cuda.stream(s_edges[k]):
                    ops.backward_pixel_map(faces[lo:hi], fi_g, m["rgb_map"][lo:hi], m["alpha_map"][lo:hi] if ra else None,
                                           None, None, det_k4, S, eps, True, ra,
                                           vertex_target=None if det else target, visibility=vis[k], unscaled=unscaled,
                                           edge_plan=m["edge_plan"][k])
                    if det:     # K4's and K6's per-face arrays -> the screen-space gradient, per vertex in a fixed order
                        _lib.check(L.d3m_vertex_gather(_lib.ptr(det_k4), _lib.ptr(det_k6), _lib.ptr(st.adjacency.csr.offsets),
                                                       _lib.ptr(st.adjacency.csr.items), _lib.ptr(grad_sv), B, V, Ft,
                                                       int(fill_back), _lib.ptr(vis[k]), _lib.stream_ptr()),
                                   "d3m_vertex_gather")
        if G > 1:
            yield "textures"
        def light_to_vertices(grad_light):
            # the light gradient -> world-space vertices through the face normals
            if det:     # the views' gradients summed in view order (torch's reduction), the adjoint gathered per vertex
                total = det_gl.sum(0)           # (one shared mesh, one light: _deterministic_supported)
                head = (_lib.ptr(vertices), _lib.ptr(tri), _lib.ptr(st.adjacency.csr.offsets), _lib.ptr(st.adjacency.csr.items),
                        _lib.ptr(total), _lib.ptr(grad_vertices))
                if dlight is None:
                    _lib.check(L.d3m_face_light_backward_gather(*head, *by_value, V, Ft, int(fill_back), _lib.stream_ptr()),
                               "d3m_face_light_backward_gather")
                else:
                    _lib.check(L.d3m_face_light_backward_gather_dev(*head, ctypes.byref(dl_c), V, Ft, int(fill_back),
                                                                    _lib.stream_ptr()), "d3m_face_light_backward_gather_dev")
                return
            head = (_lib.ptr(vertices), vertices.shape[0], _lib.ptr(tri), tri.shape[0], _lib.ptr(grad_light),
                    _lib.ptr(grad_vertices))
            if dlight is None:
                _lib.check(L.d3m_face_light_backward(*head, *by_value, Bl, V, Ft, int(fill_back), _lib.stream_ptr()),
                           "d3m_face_light_backward")
            else:
                _lib.check(L.d3m_face_light_backward_dev(*head, ctypes.byref(dl_c), Bl, V, Ft, int(fill_back),
                                                         _lib.stream_ptr()), "d3m_face_light_backward_dev")

        # One pipeline on one stream with the camera inside the node: the light's adjoint and the camera's are the step's last
        # two kernels -- ONE launch then (d3m_lit_back: both add into the zeroed grad_vertices with float atomics).  With
        # branches the light's adjoint runs beside the line walk instead (below), where it costs the step nothing.
        fused_tail = st.serial and G == 1 and gathered and need_vert and st.camera is not None and not det
        light_done = fused_tail
        if gathered and need_vert and G == 1 and not fused_tail:
            # one pipeline: straight behind the gathered pass on its branch, beside the line walk, not behind the join
            with torch.cuda.stream(s_gath[0]):
                light_to_vertices(gl_g[0] if light_shared else grad_light)
            light_done = True
        # ... and so does the camera's adjoint, the step's last kernel, behind the gather: the side stream waits for the
        # forking stream's (shorter, by then finished) chain instead of the other way round, and the final join is the
        # end of the step
        tail_on_side = swap and gathered and st.camera is not None
        for k in range(G):
            if mains[k] is not cur:
                cur.wait_stream(mains[k])
            if tail_on_side:
                auxs[k].wait_stream(cur)
            elif gathered or st.plan_open:
                cur.wait_stream(auxs[k])
        if gathered:
            # shared textures / light: the groups' sums add up (a group's pass already summed over its views)
            if tex_shared:
                grad_textures = gt_g[0] if G == 1 else torch.stack(gt_g).sum(0)
            if need_vert and not light_done:
                if light_shared:
                    grad_light = gl_g[0] if G == 1 else torch.stack(gl_g).sum(0)
                light_to_vertices(grad_light)
            if not need_tex:
                grad_textures = None
        elif rd and need_geom:              # textures and lighting need no gradient: the depth term on its own
            if fit is not None:
                # d3m_backward_depth_map takes final maps: the fused objective left sign(depth - target) * mask, which
                # still lacks grad_loss / sum(mask) (GradScale::get, d3m_device.h); totals[2] of the scratch holds that
                # sum (the same in every group: with more than one the normaliser is the batch's mask_sum)
                g_depth_map = g_depth_map * (grad_loss / fit.mask_sum)              # mask_sum: set whenever gradients are wanted
            grad_faces = torch.zeros_like(faces)
            ops.backward_depth_map(faces, m["depth_map"], m["face_index_map"], m["face_inv_map"], m["weight_map"],
                                   g_depth_map, grad_faces, S)
            _lib.check(L.d3m_scatter_face_grads(_lib.ptr(grad_faces), _lib.ptr(tri), tri.shape[0], _lib.ptr(grad_sv), B, V,
                                                Ft, int(fill_back), _lib.stream_ptr()), "d3m_scatter_face_grads")
        grad_lp = [None] * 5
        if any(st.need_lp):
            # the light's parameters: one fixed-order reduction of the per-face light's gradient (per view in the
            # deterministic pass: summed over the views in view order by the same kernel)
            if det:
                gl_all, nbl = det_gl, B
            elif light_shared:
                gl_all = grad_light if grad_light is not None else (gl_g[0] if G == 1 else torch.stack(gl_g).sum(0))
                nbl = 1
            else:
                gl_all, nbl = grad_light, Bl
            grad_lp = [torch.empty_like(t) if need else None for t, need in zip(dlight, st.need_lp)]
            ws = torch.empty(int(L.d3m_light_params_backward_workspace_bytes(nbl, Ft, int(fill_back))), dtype=torch.uint8,
                             device=dev)
            _lib.check(L.d3m_light_params_backward(
                _lib.ptr(vertices), vertices.shape[0], _lib.ptr(tri), tri.shape[0], _lib.ptr(gl_all), nbl, ctypes.byref(dl_c),
                ctypes.byref(_light_struct(grad_lp, dlight)), V, Ft, int(fill_back), _lib.ptr(ws), ws.numel(),
                _lib.stream_ptr()), "d3m_light_params_backward")
        # the camera's parameters (a learnable camera inside the node): one fixed-order reduction of the final grad_sv,
        # beside the camera's adjoint on the same stream
        grad_cp = (None,) * 6
        if fused_tail:
            from . import cameras
            cam, _keep = cameras._camera_struct(st.camera, dev)
            head = (_lib.ptr(vertices), vertices.shape[0], ctypes.byref(cam), _lib.ptr(grad_sv), _lib.ptr(grad_vertices), B, V,
                    _lib.ptr(tri), tri.shape[0], Ft, int(fill_back), _lib.ptr(gl_g[0] if light_shared else grad_light), Bl)
            if dlight is None:
                _lib.check(L.d3m_lit_back(*head, *by_value, _lib.stream_ptr()), "d3m_lit_back")
            else:
                _lib.check(L.d3m_lit_back_dev(*head, ctypes.byref(dl_c), _lib.stream_ptr()), "d3m_lit_back_dev")
            grad_cp = cameras.params_backward(st.camera, vertices, grad_sv, st.need_cp)
            grad_sv = None
        elif st.camera is not None and need_geom:
            # the camera's adjoint joins the light's in the same buffer (or writes it, when there is none)
            from . import cameras
            cam, _keep = cameras._camera_struct(st.camera, dev)
            tail = auxs[0] if tail_on_side else cur
            if st.need_mesh:
                if grad_vertices is None:
                    grad_vertices = sink[0] if sink is not None else torch.empty_like(vertices)
                    fn, what = L.d3m_camera_backward, "d3m_camera_backward"
                else:
                    fn, what = L.d3m_camera_backward_add, "d3m_camera_backward_add"
                with torch.cuda.stream(tail):
                    _lib.check(fn(_lib.ptr(vertices), vertices.shape[0], ctypes.byref(cam), _lib.ptr(grad_sv),
                                  _lib.ptr(grad_vertices), B, V, _lib.stream_ptr()), what)
            grad_cp = cameras.params_backward(st.camera, vertices, grad_sv, st.need_cp, stream=tail)
            grad_sv = None
        if tail_on_side:
            cur.wait_stream(auxs[0])
        return (grad_sv if need_geom else None, grad_vertices if need_geom else None, None, grad_textures) + (None,) * 17 + \
            tuple(grad_lp) + tuple(grad_cp)


# What _RasterizeMeshModes' forward decided and left for backward: configuration, the deterministic switch (checked in backward),
# the camera (+ what its structs point into), the pass's maps and backward's accumulator, zeroed by forward (pre; one use)
_MeshModesState = dataclasses.make_dataclass("_MeshModesState", (
    "aa eps fill_back ra rd det camera keep faces face_index_map weight_map depth_map alpha_map visibility plan pre need_mesh "
    "need_cp adjacency").split(),
    eq=False)


class _RasterizeMeshModes(torch.autograd.Function):
    """render_silhouettes / render_depth (NR/renderer.py:114-183) of an indexed mesh as ONE node, camera inside: the
    reference's sequence for these modes -- look_at / look / projection, vertices_to_faces (+ the fill_back copy), the
    rasterizer with alpha or depth output, its backward and the gather's scatter-add adjoint -- run through the pipeline the
    lit node uses: the step's first launch transforms the vertices (d3m_lit_front), coverage reads the faces through the
    index tensor and leaves the dense copy, the visibility list and the edge plan behind, and backward adds the edge
    gradient (K4, alpha) and the depth gradient (K6, over the listed faces) straight into the screen-space gradient of
    the VERTICES (d3m_vertex_target), which the camera's adjoint takes to the mesh.  No [B,F',3,3] gather, no dense
    grad_faces, no scatter-add pass, no pass over face_index_map for the visibility flags, no epilogue pass without
    anti-aliasing: the 32-view silhouette step 1.57 -> 1.21 ms, the depth step 1.12 -> 0.66, same images bit for bit
    (tests/test_gpu_renderer.py; docs/EXPERIMENTS.md C)."""

    @staticmethod
    def forward(ctx, vertices, tri, camera, fill_back, image_size, anti_aliasing, near, far, eps, return_alpha, return_depth,
                c_eye_or_t=None, c_at_or_direction=None, c_up=None, c_rot=None, c_K=None, c_dist=None):
        # c_*: the parameter tensors of `camera` (cameras.camera_inputs) as autograd inputs: backward returns their gradients
        from . import cameras
        L = _lib.lib()
        vertices = f32c(vertices)
        tri = tri.to(torch.int32).contiguous()
        dev = vertices.device
        cam, cam_keep = cameras._camera_struct(camera, dev)
        basis, basis_keep = cameras.basis_struct(camera)
        B, V, Ft = camera["batch"], vertices.shape[1], tri.shape[1]
        Fp = 2 * Ft if fill_back else Ft
        if vertices.shape[0] not in (1, B) or tri.shape[0] not in (1, B):
            raise ValueError("vertices must be [1 or B, V, 3] and faces [1 or B, F, 3]")
        S = int(image_size) * 2 if anti_aliasing else int(image_size)
        s_out = int(image_size)
        need_cp = tuple(bool(x) for x in (tuple(ctx.needs_input_grad) + (False,) * 6)[11:17])
        need_grad = ctx.needs_input_grad[0] or any(need_cp)
        sv = torch.empty(B, V, 3, dtype=torch.float32, device=dev)
        faces = torch.empty(B, Fp, 3, 3, dtype=torch.float32, device=dev)      # (the dense copy of faces that can own a pixel)
        fi = torch.empty(B, S, S, dtype=torch.int32, device=dev)
        wm = torch.empty(B, S, S, 3, dtype=torch.float32, device=dev)
        dm = torch.empty(B, S, S, dtype=torch.float32, device=dev)
        alpha_map = torch.empty(B, S, S, dtype=torch.float32, device=dev) if return_alpha else None
        alpha = torch.empty(B, s_out, s_out, dtype=torch.float32, device=dev) if return_alpha else None
        depth = torch.empty(B, s_out, s_out, dtype=torch.float32, device=dev) if return_depth else None
        vis = torch.empty(int(L.d3m_visibility_bytes(B, Fp)), dtype=torch.uint8, device=dev) if need_grad else None
        plan = torch.empty(int(L.d3m_edge_plan_bytes(B, Fp, S)), dtype=torch.uint8, device=dev) \
            if (need_grad and return_alpha) else None
        ws = ops._workspace("fwd", L.d3m_forward_workspace_bytes(B, Fp, S), dev)
        # the first launch: camera (+ basis) and the clears of the operators behind it
        clears, flags_fwd, flags_plan = [], 0, 0
        nb = int(L.d3m_forward_clear_bytes(B, Ft, int(bool(fill_back)), S, ws.numel()))
        if nb:
            clears.append((ws.data_ptr(), nb))
            flags_fwd = _lib.PRECLEARED
        if plan is not None:
            clears.append((plan.data_ptr(), int(L.d3m_edge_plan_clear_bytes(B, Fp, S))))
            flags_plan = _lib.PRECLEARED
        # ... and of the backward pass: its accumulator (and the large faces' counter behind it) is allocated here and zeroed
        # by the same launch -- a fill of 12 B per (view, vertex) less in backward (one use: a second backward over the same
        # graph allocates and clears its own)
        pre = None
        if need_grad:
            pre = torch.empty(B * V * 3 + 64, dtype=torch.float32, device=dev)
            clears.append(_lib.tensor_range(pre))
        zero3 = _vec3_host((0.0, 0.0, 0.0))
        _lib.check(L.d3m_lit_front(_lib.ptr(vertices), vertices.shape[0], ctypes.byref(cam),
                                   ctypes.byref(basis) if basis is not None else None, _lib.ptr(sv), B, V, _lib.ptr(tri),
                                   tri.shape[0], Ft, int(bool(fill_back)), None, 0, 0.0, 0.0, zero3, zero3, zero3,
                                   *_front_clears(clears), _lib.stream_ptr()), "d3m_lit_front")
        # without anti-aliasing the output images are the maps with their rows reversed: coverage's last pass writes them too
        # (no epilogue pass); with it, the 2x2 pooling is a pass of its own
        in_pass = not anti_aliasing
        _lib.check(L.d3m_forward_face_index_map_mesh_modes(
            _lib.ptr(sv), _lib.ptr(tri), tri.shape[0], V, Ft, int(bool(fill_back)), _lib.ptr(faces), _lib.ptr(fi), _lib.ptr(wm),
            _lib.ptr(dm), None, B, S, float(near), float(far), _lib.ptr(ws), ws.numel(), _lib.ptr(vis),
            vis.numel() if vis is not None else 0, _lib.ptr(alpha_map if in_pass else None),
            _lib.ptr(alpha if in_pass else None), _lib.ptr(depth if in_pass else None), flags_fwd, _lib.stream_ptr()),
            "d3m_forward_face_index_map_mesh_modes")
        if not in_pass:
            _lib.check(L.d3m_output_epilogue(_lib.ptr(fi), None, _lib.ptr(dm if return_depth else None), None, 1, None,
                                             _lib.ptr(alpha_map), None, _lib.ptr(alpha), _lib.ptr(depth), B, S,
                                             int(bool(anti_aliasing)), _lib.stream_ptr()), "d3m_output_epilogue")
        if need_grad:
            # (the first step of the visibility list -- which faces own a pixel -- was left by the coverage pass)
            _lib.check(L.d3m_visibility(None, _lib.ptr(vis), vis.numel(), B, Fp, S, _lib.stream_ptr()), "d3m_visibility")
            if plan is not None:
                _lib.check(L.d3m_edge_plan(_lib.ptr(faces), _lib.ptr(fi), _lib.ptr(vis), _lib.ptr(plan), plan.numel(), B, Fp, S,
                                           flags_plan, _lib.stream_ptr()), "d3m_edge_plan")
        det = bool(need_grad) and _deterministic()
        # (the deterministic backward pass's CSR adjacency: one shared topology, silhouettes alone or depth alone)
        adjacency = vertex_adjacency(tri, V) if (det and (return_alpha != return_depth) and tri.shape[0] == 1) else None
        ctx.state = _MeshModesState(aa=bool(anti_aliasing), eps=float(eps), fill_back=bool(fill_back), ra=bool(return_alpha), rd=bool(return_depth), det=det,
                                    camera=camera, keep=(cam_keep, basis_keep), faces=faces, face_index_map=fi,
                                    weight_map=wm, depth_map=dm, alpha_map=alpha_map, visibility=vis, plan=plan, pre=pre,
                                    need_mesh=bool(ctx.needs_input_grad[0]), need_cp=need_cp, adjacency=adjacency)
        ctx.save_for_backward(vertices, tri)
        empty = torch.tensor([])
        return (alpha if return_alpha else empty, depth if return_depth else empty)

    @staticmethod
    def backward(ctx, g_alpha, g_depth):
        from . import cameras
        L = _lib.lib()
        st = ctx.state
        _check_deterministic(st.det)
        vertices, tri = ctx.saved_tensors
        aa, eps, fill_back, ra, rd = st.aa, st.eps, st.fill_back, st.ra, st.rd
        faces, fi, wm, dm, alpha_map = st.faces, st.face_index_map, st.weight_map, st.depth_map, st.alpha_map
        vis, plan = st.visibility, st.plan
        (B, Fp), S, V, Ft = faces.shape[:2], fi.shape[1], vertices.shape[1], tri.shape[1]
        dev = vertices.device
        # (the fixed-order sums cover one shared topology; per-view topologies keep their float atomics: DESIGN.md section 6)
        ordered = st.det and tri.shape[0] == 1
        acc, st.pre = st.pre, None
        if acc is None:
            acc = torch.empty(B * V * 3 + 64, dtype=torch.float32, device=dev)
            _lib.zero_raw([_lib.tensor_range(acc)])
        grad_sv, counter = acc[:B * V * 3].view(B, V, 3), acc[B * V * 3:]
        target = _lib.D3MVertexTarget(_lib.ptr(grad_sv), _lib.ptr(tri), V, Ft, tri.shape[0], int(fill_back))
        g_depth_map = torch.empty(B, S, S, dtype=torch.float32, device=dev) if (rd and (ra or aa)) else None
        if ra and not rd:
            # silhouettes only: the edge gradient reads the image's gradient where it is -- through the row flip and the
            # pooling's adjoint -- and the owners from face_index_map; no per-pixel records (d3m_edge_grad.h, "DIRECT")
            g_img = f32c(g_alpha)
            unscaled = _image_grad_struct(g_img, aa)
            if ordered:
                # DETERMINISTIC (as the lit node's): K4 into its own per-face array (plain stores), summed per vertex in a
                # fixed order over the index tensor's CSR adjacency -- bit-identical runs.
                det_k4 = torch.empty(B, Fp, 3, 3, dtype=torch.float32, device=dev)
                _lib.zero_raw([_lib.tensor_range(det_k4)])
                ops.backward_pixel_map(faces, fi, None, alpha_map, None, None, det_k4, S, eps, False, True,
                                       visibility=vis, unscaled=unscaled, edge_plan=plan)
                _lib.check(L.d3m_vertex_gather(_lib.ptr(det_k4), None, _lib.ptr(st.adjacency.csr.offsets),
                                               _lib.ptr(st.adjacency.csr.items), _lib.ptr(grad_sv), B, V, Ft, int(fill_back),
                                               _lib.ptr(vis), _lib.stream_ptr()), "d3m_vertex_gather")
            else:
                ops.backward_pixel_map(faces, fi, None, alpha_map, None, None, None, S, eps, False, True, vertex_target=target,
                                       visibility=vis, unscaled=unscaled, edge_plan=plan)
        elif ra:
            # the adjoint of the output epilogue writes the alpha gradient straight as the edge gradient's per-pixel records
            # (and the depth gradient as the map K6 reads)
            records = _pixel_records(B, S, dev)
            _lib.check(L.d3m_output_epilogue_backward_records(
                None, _lib.ptr(f32c(g_alpha)), _lib.ptr(f32c(g_depth) if rd else None), _lib.ptr(fi), None, _lib.ptr(alpha_map),
                _lib.ptr(records.edge_grad), _lib.ptr(records.edge_dot), _lib.ptr(records.extents[0]),
                _lib.ptr(records.extents[1]), _lib.ptr(g_depth_map), B, S, int(aa), _lib.stream_ptr()),
                "d3m_output_epilogue_backward_records")
            unscaled = records.struct(0, B)
            ops.backward_pixel_map(faces, fi, None, alpha_map, None, None, None, S, eps, False, True, vertex_target=target,
                                   visibility=vis, unscaled=unscaled, edge_plan=plan)
        k6_flags = _lib.PRECLEARED
        det_depth = rd and not ra and ordered
        if det_depth:
            # DETERMINISTIC, depth mode: the adjoint of the output epilogue as a map, K6 gathered per face into its own array by
            # the reference-shaped operator (in this mode without its per-pixel fallback for large faces: d3m_backward_depth_map),
            # summed per vertex over the CSR adjacency
            g_depth_map = torch.empty(B, S, S, dtype=torch.float32, device=dev)
            _lib.check(L.d3m_output_epilogue_backward(None, None, _lib.ptr(f32c(g_depth)), None, None, _lib.ptr(g_depth_map),
                                                      B, S, int(aa), _lib.stream_ptr()), "d3m_output_epilogue_backward")
            det_k6 = torch.empty(B, Fp, 3, 3, dtype=torch.float32, device=dev)
            _lib.zero_raw([_lib.tensor_range(det_k6)])
            ops.backward_depth_map(faces, dm, fi, const_tensor((0.0,), dev), wm, g_depth_map, det_k6, S)
            _lib.check(L.d3m_vertex_gather(_lib.ptr(det_k6), None, _lib.ptr(st.adjacency.csr.offsets),
                                           _lib.ptr(st.adjacency.csr.items), _lib.ptr(grad_sv), B, V, Ft, int(fill_back),
                                           _lib.ptr(vis), _lib.stream_ptr()), "d3m_vertex_gather")
        elif rd and not ra:
            if aa:
                _lib.check(L.d3m_output_epilogue_backward(None, None, _lib.ptr(f32c(g_depth)), None, None, _lib.ptr(g_depth_map),
                                                          B, S, int(aa), _lib.stream_ptr()), "d3m_output_epilogue_backward")
            else:   # the output image is the depth map with its rows reversed: K6 reads the gradient through the flip
                g_depth_map, k6_flags = f32c(g_depth), k6_flags | _lib.GRAD_OF_OUTPUT_IMAGE
        if rd and not det_depth:
            _lib.check(L.d3m_backward_depth_map_mesh(_lib.ptr(faces), _lib.ptr(dm), _lib.ptr(fi), _lib.ptr(wm),
                                                     _lib.ptr(g_depth_map), B, Fp, S, ctypes.byref(target), _lib.ptr(vis),
                                                     _lib.ptr(counter), k6_flags, _lib.stream_ptr()),
                       "d3m_backward_depth_map_mesh")
        grad_vertices = None
        if st.need_mesh:
            cam, _keep = cameras._camera_struct(st.camera, dev)
            grad_vertices = torch.empty_like(vertices)
            _lib.check(L.d3m_camera_backward(_lib.ptr(vertices), vertices.shape[0], ctypes.byref(cam), _lib.ptr(grad_sv),
                                             _lib.ptr(grad_vertices), B, V, _lib.stream_ptr()), "d3m_camera_backward")
        # a learnable camera: its parameters' gradient from the same grad_sv (d3m_camera_params_backward)
        return (grad_vertices,) + (None,) * 10 + cameras.params_backward(st.camera, vertices, grad_sv, st.need_cp)


def rasterize_mesh_modes(vertices, tri, camera, fill_back, image_size, anti_aliasing, return_alpha, return_depth,
                         near=DEFAULT_NEAR, far=DEFAULT_FAR, eps=DEFAULT_EPS):
    """(alpha, depth) images -- either may be left out -- of an indexed mesh seen through `camera` (the parameter block of
    cameras.look_at_params & co): the silhouette / depth modes of the renderer as one node.  See _RasterizeMeshModes."""
    alpha, depth = _RasterizeMeshModes.apply(vertices, tri, camera, bool(fill_back), int(image_size), bool(anti_aliasing),
                                             float(near), float(far), float(eps), bool(return_alpha), bool(return_depth),
                                             *_camera_tensors(camera))
    return (alpha if return_alpha else None), (depth if return_depth else None)


class _ManualContext:
    """What _RasterizeLit.forward / _backward_halves use of an autograd context, for calling them WITHOUT the autograd
    engine (LitFitManual): needs_input_grad, save_for_backward / saved_tensors, the node's state.  Forward runs every kernel
    of a node given this context on one stream."""

    def __init__(self, needs_input_grad):
        self.needs_input_grad = tuple(needs_input_grad)
        self.saved_tensors = ()
        self.state = self.maps = None

    def save_for_backward(self, *tensors):
        self.saved_tensors = tuple(tensors)


class LitFitManual:
    """The fused fit objective of the lit render node (rasterize_lit_fit) driven by hand instead of by the autograd
    engine: forward(), then the two halves of backward as separate calls on the CALLER's thread and stream --

        loss = m.forward(...)                 # as rasterize_lit_fit(...)
        m.backward_texture_side(grad_loss)    # grad_textures final (in the grad_sink, if one was given)
        gv, gt = m.backward_geometry_side()   # grad_vertices final

    -- so that a step can be captured as TWO HIP graphs with a collective issued between them (a capture cannot be ended
    on autograd's worker thread, and one autograd node cannot be split).  Same kernels, same numbers as the autograd
    node: it is that node's code (tests/test_gpu_multirank.py)."""

    def __init__(self, vertices_grad=True, textures_grad=True):
        self._needs = (False, bool(vertices_grad), False, bool(textures_grad)) + (False,) * 22
        self._ctx = self._halves = None

    def forward(self, vertices, tri, textures, light_cfg, fill_back, targets, image_size, near, far, eps, background_color,
                camera, grad_sink=None, images_out=None, anti_aliasing=False):
        if light_on_device(light_cfg):
            raise ValueError("LitFitManual takes one constant light for all views (no per-view light, no light that requires grad)")
        self._ctx = _ManualContext(self._needs)
        with torch.no_grad():
            return _RasterizeLit.forward(self._ctx, None, vertices, tri, textures, light_cfg, fill_back, image_size,
                                         bool(anti_aliasing), near, far, eps, background_color, True, True, True,
                                         (targets, images_out), 1, False, camera, grad_sink)

    def backward_texture_side(self, grad_loss):
        with torch.no_grad():
            self._halves = _RasterizeLit._backward_halves(self._ctx, grad_loss)
            next(self._halves)

    def backward_geometry_side(self):
        with torch.no_grad():
            try:
                next(self._halves)
            except StopIteration as done:
                grads = done.value
                self._ctx = self._halves = None
                return grads[1], grads[3]           # (grad_vertices, grad_textures)
        raise RuntimeError("_backward_halves yields once")


def _device_light(light_cfg, screen_vertices, vertices, camera):
    """The five light tensors the lit node takes as autograd inputs (normalize_light) when the light goes by device memory
    (light_on_device), else five None: the light of light_cfg by value, today's route.  Shapes are checked here, in front of
    any launch."""
    if not light_on_device(light_cfg):
        return (None,) * 5
    batch = camera["batch"] if camera is not None else screen_vertices.shape[0]
    return normalize_light(light_cfg, batch, vertices.device)


def _camera_tensors(camera):
    """The six parameter tensors of a camera inside a node (cameras.camera_inputs), autograd inputs of the node: a
    parameter that requires grad receives its gradient from the node's backward pass."""
    from . import cameras
    return cameras.camera_inputs(camera) if camera is not None else (None,) * 6


def rasterize_lit(screen_vertices, vertices, tri, textures, light_cfg, fill_back, image_size=DEFAULT_IMAGE_SIZE,
                  anti_aliasing=DEFAULT_ANTI_ALIASING, near=DEFAULT_NEAR, far=DEFAULT_FAR, eps=DEFAULT_EPS,
                  background_color=DEFAULT_BACKGROUND_COLOR, return_alpha=True, return_depth=True, view_groups=1,
                  camera=None, fit_hint=None, defer_plan_join=False):
    """rgb (+alpha, depth) images of the mesh (`screen_vertices` [B,V,3] after the camera transform, triangles
    `tri` [1|B,F,3]) textured with the ORIGINAL `textures` [1|B,F,ts,ts,ts,3]; the fill_back copy and the per-face
    light (computed from world-space `vertices`) are applied on the fly.  Same outputs as vertices_to_faces() +
    lighting() + rasterize_rgbad() on the materialised arrays.  `camera` (with screen_vertices None): the fused camera
    kernels' parameter block (cameras.look_at_params) -- the transform then runs inside the node.  `fit_hint` = the targets
    (rgb, depth, alpha, mask[, mask_sum]) of a multi-view fit objective the caller is about to evaluate on the returned
    images: see _RasterizeLit.forward, "a REGISTERED objective".  `light_cfg` = (intensity_ambient, intensity_directional,
    color_ambient, color_directional, direction): see normalize_light; a light that requires grad or is given per view is
    read from device memory and receives its gradient (light_on_device)."""
    rgb, alpha, depth = _RasterizeLit.apply(screen_vertices, vertices, tri, textures, light_cfg, fill_back, image_size,
                                            anti_aliasing, near, far, eps, background_color, True, return_alpha,
                                            return_depth, None, view_groups, defer_plan_join, camera, None, fit_hint,
                                            *_device_light(light_cfg, screen_vertices, vertices, camera),
                                            *_camera_tensors(camera))
    return {'rgb': rgb, 'alpha': alpha if return_alpha else None, 'depth': depth if return_depth else None}


def rasterize_lit_image_grid(screen_vertices, vertices, grid_hw, image, light_cfg, image_size=DEFAULT_IMAGE_SIZE,
                             anti_aliasing=DEFAULT_ANTI_ALIASING, near=DEFAULT_NEAR, far=DEFAULT_FAR, eps=DEFAULT_EPS,
                             background_color=DEFAULT_BACKGROUND_COLOR):
    """rgb [B,3,s,s] of a depth map's grid mesh textured by an image -- what NrRenderer's view-synthesis frames render
    (deep3dmap/core/renderer/renderer_nr.py:196-198: get_face_idx + get_textures_from_im(tx_size=2) + render_rgb with
    fill_back) -- with NEITHER array: the triangles are the implicit topology of the (h, w) grid (`grid_hw`), their texture
    cubes are evaluated from `image` [B,3,h,w] inside the sampler.  Same pixels as rasterize_lit() on the materialised
    arrays.  Forward only (visualisation frames): with gradients, the cube array is backward's intermediate anyway and the
    caller takes the materialised route."""
    if torch.is_grad_enabled() and any(t.requires_grad for t in (screen_vertices, vertices, image)):
        raise RuntimeError("rasterize_lit_image_grid is a forward-only path")
    L = _lib.lib()
    sv, vertices, im = f32c(screen_vertices), f32c(vertices), f32c(image)
    h, w = grid_hw
    B, V, dev = sv.shape[0], sv.shape[1], sv.device
    if V != h * w or tuple(im.shape) != (B, 3, h, w) or vertices.shape[1] != V:
        raise ValueError("vertices must be [B,h*w,3] and the image [B,3,h,w]")
    Ft = 2 * (h - 1) * (w - 1)
    Fp = 2 * Ft
    S = int(image_size) * 2 if anti_aliasing else int(image_size)
    s_out = int(image_size)
    ia, idr, ca, cd, direction = light_cfg
    light = torch.empty(vertices.shape[0], Fp, 3, dtype=torch.float32, device=dev)
    _lib.check(L.d3m_face_light(_lib.ptr(vertices), vertices.shape[0], None, -w, _lib.ptr(light), float(ia), float(idr),
                                _vec3_host(ca), _vec3_host(cd), _vec3_host(direction), vertices.shape[0], V, Ft, 1,
                                _lib.stream_ptr()), "d3m_face_light")
    faces = torch.empty(B, Fp, 3, 3, dtype=torch.float32, device=dev)
    fim = torch.empty((B, S, S), dtype=torch.int32, device=dev)
    wm = torch.empty(B, S, S, 3, dtype=torch.float32, device=dev)
    dm = torch.empty((B, S, S), dtype=torch.float32, device=dev)
    ws = ops._workspace("fwd", L.d3m_forward_workspace_bytes(B, Fp, S), dev)
    _lib.check(L.d3m_forward_face_index_map_mesh(_lib.ptr(sv), None, -w, V, Ft, 1, _lib.ptr(faces), _lib.ptr(fim), _lib.ptr(wm),
                                                 _lib.ptr(dm), None, B, S, float(near), float(far), _lib.ptr(ws), ws.numel(),
                                                 None, 0, 0, _lib.stream_ptr()), "d3m_forward_face_index_map_mesh")
    background = _background_tensor(background_color, dev)
    rgb_map = torch.empty(B, S, S, 3, dtype=torch.float32, device=dev)
    rgb = torch.empty(B, 3, s_out, s_out, dtype=torch.float32, device=dev)
    _lib.check(L.d3m_render_lit_epilogue(
        _lib.ptr(faces), _lib.ptr(im), -w, _lib.ptr(light), light.shape[0], _lib.ptr(fim), _lib.ptr(wm), _lib.ptr(dm),
        _lib.ptr(background), background.shape[0], _lib.ptr(rgb_map), None, _lib.ptr(rgb), None, None, B, Ft, 1, S, 2,
        float(eps), int(bool(anti_aliasing)), None, _lib.stream_ptr()), "d3m_render_lit_epilogue")
    return rgb


def rasterize_lit_fit(screen_vertices, vertices, tri, textures, light_cfg, fill_back, targets, image_size=DEFAULT_IMAGE_SIZE,
                      near=DEFAULT_NEAR, far=DEFAULT_FAR, eps=DEFAULT_EPS, background_color=DEFAULT_BACKGROUND_COLOR,
                      view_groups=1, defer_plan_join=False, images_out=None, camera=None, grad_sink=None,
                      anti_aliasing=False):
    """The multi-view fit objective of the images rasterize_lit() would return (targets at the output size; with
    anti_aliasing the objective of the 2x2-pooled images),

        photometric_loss(rgb, rgb_t, mask) + sum((alpha - alpha_t)^2) / S^2 + photometric_loss(depth, depth_t, mask),

    `targets` = (rgb_t [B,3,S,S], depth_t [B,S,S], alpha_t [B,S,S], mask [B,S,S][, mask_sum]), evaluated inside the
    rendering node (the optional device scalar `mask_sum` replaces sum(mask) as the photometric normaliser: the sum over
    ALL ranks' views when these views are one shard of a camera-sharded fit, so that values and gradients add up): the sums are taken where the images are produced and the gradient is written straight into the
    internal-resolution maps, so the images and their gradients never exist in memory.  Same value and gradients as
    core.losses.multiview_fit_loss(*rasterize_lit(...), ...)."""
    # (images_out: (rgb, depth, alpha) buffers the same pass fills with the images render() returns)
    return _RasterizeLit.apply(screen_vertices, vertices, tri, textures, light_cfg, fill_back, image_size,
                               bool(anti_aliasing), near, far, eps, background_color, True, True, True,
                               (targets, images_out), view_groups, defer_plan_join, camera, grad_sink, None,
                               *_device_light(light_cfg, screen_vertices, vertices, camera), *_camera_tensors(camera))


def rasterize_rgbad(
        faces,
        textures=None,
        image_size=DEFAULT_IMAGE_SIZE,
        anti_aliasing=DEFAULT_ANTI_ALIASING,
        near=DEFAULT_NEAR,
        far=DEFAULT_FAR,
        eps=DEFAULT_EPS,
        background_color=DEFAULT_BACKGROUND_COLOR,
        return_rgb=True,
        return_alpha=True,
        return_depth=True,
):
    """
    Generate RGB, alpha channel, and depth images from faces and textures (NR/rasterize.py:253-334).

    Args:
        faces (torch.Tensor): [batch size, number of faces, 3 (vertices), 3 (XYZ)].
        textures (torch.Tensor): [batch size, number of faces, ts, ts, ts, 3 (RGB)].
        image_size (int): width and height of rendered images.
        anti_aliasing (bool): 2x super-sampling.
        near, far (float): depth range that is drawn.
        eps (float): epsilon of the approximate edge gradient.
        background_color: colour (3) or one colour per batch entry (B, 3).

    Returns:
        dict: 'rgb' [B,3,s,s], 'alpha' [B,s,s], 'depth' [B,s,s] (None for disabled outputs); row 0 is the
        TOP of the image.
    """
    if not faces.is_cuda or (textures is not None and not textures.is_cuda):
        raise TypeError('Rasterize module supports only cuda Tensors')
    rgb, alpha, depth = _RasterizeImages.apply(faces, textures, image_size, anti_aliasing, near, far, eps,
                                               background_color, return_rgb, return_alpha, return_depth)
    return {
        'rgb': rgb if return_rgb else None,
        'alpha': alpha if return_alpha else None,
        'depth': depth if return_depth else None,
    }


def rasterize(faces, textures, image_size=DEFAULT_IMAGE_SIZE, anti_aliasing=DEFAULT_ANTI_ALIASING,
              near=DEFAULT_NEAR, far=DEFAULT_FAR, eps=DEFAULT_EPS, background_color=DEFAULT_BACKGROUND_COLOR):
    """RGB images [B,3,s,s] (NR/rasterize.py:367-394)."""
    return rasterize_rgbad(
        faces, textures, image_size, anti_aliasing, near, far, eps, background_color, True, False, False)['rgb']


def rasterize_silhouettes(faces, image_size=DEFAULT_IMAGE_SIZE, anti_aliasing=DEFAULT_ANTI_ALIASING,
                          near=DEFAULT_NEAR, far=DEFAULT_FAR, eps=DEFAULT_EPS):
    """Alpha channels [B,s,s] (NR/rasterize.py:397-420)."""
    return rasterize_rgbad(faces, None, image_size, anti_aliasing, near, far, eps, None, False, True, False)['alpha']


def rasterize_depth(faces, image_size=DEFAULT_IMAGE_SIZE, anti_aliasing=DEFAULT_ANTI_ALIASING,
                    near=DEFAULT_NEAR, far=DEFAULT_FAR, eps=DEFAULT_EPS):
    """Depth images [B,s,s] (NR/rasterize.py:423-446)."""
    return rasterize_rgbad(faces, None, image_size, anti_aliasing, near, far, eps, None, False, False, True)['depth']
