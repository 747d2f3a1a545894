"""View images baked into a uv texture: the inverse of sample_uv_texture, over the same Fragments records and with the same
conventions.  Where sample_uv_texture draws a texture into a view, `bake_uv_texture` pulls the colours a view shows back into
the texture that node samples, texel by texel, and the view record's z-buffer decides which texels the view sees.

`uv_layout_fragments` rasterises the layout faces_uv [F,3,2] itself into a coverage record (B = 1, raster size T, every vertex
at z = 1), so a texel knows the triangle that owns it and its barycentrics b_c there, and the walks of csrc/d3m_fragments.h
serve texels as they serve pixels.  `bake_uv_texture` reads that record, the view record and the screen vertices the view
record was rasterised from.  Per texel and view: the owner's three screen-space corners; the surface point (x, y, Z) -- with
`perspective` Z = sum b_c z_c, x = sum b_c x_c z_c / Z, the point that the rasteriser's perspective-correct weights assume,
without it x = sum b_c x_c --; visible iff the internal pixel of the view record that holds (x, y) is covered and either owned by
the same triangle or not nearer than Z by more than depth_tolerance; a visible texel takes the four bilinear taps of the
view's image at (x, y), every other texel the background.  csrc/d3m_uv_bake.h states every step.  One launch.

Differentiable in the images -- the order-independent fixed-point scatter of sample_uv_texture's adjoint, three launches --
and in the screen vertices (x, y and z) through the taps' slope and the closed-form derivative of the surface point, summed
per layout face in the fixed order of csrc/d3m_fragments.h and gathered over the mesh's vertex adjacency: no float atomics,
the same bits on every run.  Visibility and the choice of taps are constants of the graph; the mask is not differentiable.

Fusing the views and filling the texels none of them saw: fuse_uv_textures (uv_fill.py)."""
import ctypes
import math

import torch

from .. import _lib
from .attributes import (Fragments, _checked_background, _checked_fragments, _checked_screen_vertices, rasterize_fragments)
from .built_cache import BuiltCache, tensor_key
from .row_gather import vertex_adjacency
from .uv_texture_images import CLAMP_TO_BORDER, MAX_CHANNELS, MAX_IMAGE_SIZE
from .uv_textures import _wrapping_code

MAX_TEXTURE_SIZE = 16384   # the rasteriser's largest image
_WRAP_REPEAT, _WRAP_MIRRORED_REPEAT, _WRAP_CLAMP_TO_EDGE = 0, 1, 2


def wrap_uv(uv, wrapping):
    """wrap_uv of csrc/d3m_textures.h on a float32 tensor, bit for bit (fmod is exact): wrapping 0 REPEAT, 1 MIRRORED_REPEAT,
    2 CLAMP_TO_EDGE."""
    def tex_mod(x, y):
        r = torch.fmod(x, y)
        return torch.where(x > 0, r, y + r)
    if wrapping == _WRAP_REPEAT:
        return tex_mod(uv, 1.0)
    if wrapping == _WRAP_MIRRORED_REPEAT:
        m = tex_mod(uv, 1.0)
        return torch.where(tex_mod(uv, 2.0) < 1, m, 1 - m)
    return uv.clamp(max=1.0).clamp(min=0.0)


def _checked_layout(faces_uv, texture_size, texture_wrapping):
    if not torch.is_tensor(faces_uv) or faces_uv.dim() != 3 or tuple(faces_uv.shape[1:]) != (3, 2) or faces_uv.shape[0] < 1:
        raise ValueError("faces_uv must be [F, 3, 2]")
    if faces_uv.dtype != torch.float32:
        raise ValueError("faces_uv must be float32")
    if isinstance(texture_size, bool) or not isinstance(texture_size, int) or not 1 <= texture_size <= MAX_TEXTURE_SIZE:
        raise ValueError(f"texture_size must be an int in 1..{MAX_TEXTURE_SIZE} (the texture is square: the rasteriser is)")
    wrapping = _wrapping_code(texture_wrapping)
    if wrapping == CLAMP_TO_BORDER:
        raise ValueError("uv_layout_fragments: CLAMP_TO_BORDER is not offered (REPEAT, MIRRORED_REPEAT or CLAMP_TO_EDGE)")
    return wrapping


def uv_layout_vertices(faces_uv, texture_size, texture_wrapping='REPEAT'):
    """(vertices [1,3F,3] f32, tri [F,3] i32) that uv_layout_fragments rasterises, with torch operators on faces_uv's device:
    the corners wrapped as sample_uv_texture wraps them, the mesh unrolled to 3F vertices (tri = arange(3F).view(F,3): seams
    are allowed, triangle f of the layout is triangle f of the mesh), x = (2 u (T - 1) + 1 - T) / T and y likewise from v
    (formed in float64, rounded once) so that the centre of texel (i, j) is the uv sample_uv_texture maps to texel (i, j),
    z = 1."""
    wrapping = _checked_layout(faces_uv, texture_size, texture_wrapping)
    T = int(texture_size)
    uv = wrap_uv(faces_uv.detach().reshape(-1, 2), wrapping).double()
    xy = ((2.0 * uv * (T - 1) + (1 - T)) / T).float()
    vertices = torch.cat((xy, torch.ones_like(xy[:, :1])), 1)[None].contiguous()
    tri = torch.arange(3 * faces_uv.shape[0], dtype=torch.int32, device=faces_uv.device).view(-1, 3)
    return vertices, tri


def uv_layout_fragments(faces_uv, texture_size, texture_wrapping='REPEAT'):
    """The layout faces_uv [F,3,2] (f32, on a GPU; per-corner uv with seams, as sample_uv_texture takes it) as a Fragments
    record with B = 1 at raster size T = texture_size: rasterize_fragments of uv_layout_vertices with fill_back=True (a uv
    triangle may have either winding) and anti_aliasing=False -- no kernel of its own.  Internal row j is texture row j.
    Because z is constant, weight_map holds a texel's barycentrics in its owner; an owner f >= F is the copy of triangle
    f - F and reads corners 2 - c, as everywhere else.  ValueError for a wrong shape, dtype, size or wrapping."""
    vertices, tri = uv_layout_vertices(faces_uv, texture_size, texture_wrapping)
    return rasterize_fragments(vertices, tri, int(texture_size), anti_aliasing=False, fill_back=True)


class UvLayoutCache(BuiltCache):
    """BuiltCache for layout records: an entry also holds the caller's faces_uv tensor."""
    what = "the uv layout's coverage record (bake_uv_texture)"


_cache = UvLayoutCache()


def cached_uv_layout_fragments(faces_uv, texture_size, texture_wrapping='REPEAT', cache=None):
    """The cached uv_layout_fragments of a faces_uv tensor at its current version (built on the first call, outside any
    stream capture); `cache`: the UvLayoutCache to keep it in (default: the module's)."""
    wrapping = _checked_layout(faces_uv, texture_size, texture_wrapping)
    cache = _cache if cache is None else cache
    return cache.get(tensor_key(faces_uv) + (int(texture_size), wrapping),
                     lambda: uv_layout_fragments(faces_uv, texture_size, wrapping), holders=(faces_uv,))


def bake_adjoint_fraction_bits(T):
    """frac = 62 - ceil(log2(T T)): the bits below 2^E that a term keeps in the image adjoint's int64 accumulators.  A view's
    image receives only from its own T^2 texels, of at most 2^frac each: no overflow."""
    n = int(T) * int(T)
    if not 1 <= n <= MAX_TEXTURE_SIZE ** 2:
        raise ValueError(f"bake_uv_texture: a texture of side 1 to {MAX_TEXTURE_SIZE}")
    return 62 - (n - 1).bit_length()


def _sizes(images):
    return tuple(int(v) for v in images.shape[1:])


class _BakeUvTexture(torch.autograd.Function):
    @staticmethod
    def forward(ctx, images, screen_vertices, uv_fragments, fragments, adjacency, perspective, depth_tolerance, background):
        img, sv = images.contiguous(), screen_vertices.detach().contiguous()
        B, T = img.shape[0], int(uv_fragments.image_size)
        C, H, W = _sizes(img)
        texture = torch.empty(B, T, T, C, dtype=torch.float32, device=img.device)
        mask = torch.empty(B, T, T, dtype=torch.float32, device=img.device)
        c_uv, c_fr = uv_fragments.c_struct(), fragments.c_struct()
        _lib.check(_lib.lib().d3m_uv_bake_texture(ctypes.byref(c_uv), ctypes.byref(c_fr), _lib.ptr(img), C, H, W, _lib.ptr(sv),
                                                  sv.shape[1], perspective, depth_tolerance, _lib.ptr(background),
                                                  _lib.ptr(texture), _lib.ptr(mask), _lib.stream_ptr()), "d3m_uv_bake_texture")
        ctx.save_for_backward(sv, *((img,) if ctx.needs_input_grad[1] else ()))
        ctx.uv_fragments, ctx.fragments, ctx.adjacency = uv_fragments, fragments, adjacency
        ctx.perspective, ctx.depth_tolerance, ctx.sizes = perspective, depth_tolerance, (B, C, H, W)
        ctx.mark_non_differentiable(mask)
        return texture, mask

    @staticmethod
    def backward(ctx, grad_texture, _grad_mask):
        L = _lib.lib()
        B, C, H, W = ctx.sizes
        sv = ctx.saved_tensors[0]
        V = sv.shape[1]
        g = grad_texture.to(torch.float32).contiguous()
        c_uv, c_fr = ctx.uv_fragments.c_struct(), ctx.fragments.c_struct()
        grad_images = grad_sv = None
        if ctx.needs_input_grad[0]:
            n = int(L.d3m_uv_bake_images_scratch_bytes(B, C, H, W))
            scratch = torch.empty((n + 7) // 8, dtype=torch.int64, device=g.device)
            grad_images = torch.empty(B, C, H, W, dtype=torch.float32, device=g.device)
            _lib.check(L.d3m_uv_bake_images_backward(ctypes.byref(c_uv), ctypes.byref(c_fr), C, H, W, _lib.ptr(sv), V,
                                                     ctx.perspective, ctx.depth_tolerance, _lib.ptr(g), _lib.ptr(scratch),
                                                     scratch.numel() * 8, _lib.ptr(grad_images), _lib.stream_ptr()),
                       "d3m_uv_bake_images_backward")
        if ctx.needs_input_grad[1]:
            img, A = ctx.saved_tensors[1], ctx.adjacency
            n = int(L.d3m_uv_bake_scratch_floats(B, ctx.uv_fragments.faces.shape[1], ctypes.byref(A.csr.c)))
            scratch = torch.empty(n, dtype=torch.float32, device=g.device)
            grad_sv = torch.empty(B, V, 3, dtype=torch.float32, device=g.device)
            _lib.check(L.d3m_uv_bake_vertices_backward(ctypes.byref(c_uv), ctypes.byref(c_fr), _lib.ptr(img), C, H, W,
                                                       _lib.ptr(sv), V, ctx.perspective, ctx.depth_tolerance, _lib.ptr(g),
                                                       ctypes.byref(A.csr.c), _lib.ptr(scratch), n, _lib.ptr(grad_sv),
                                                       _lib.stream_ptr()), "d3m_uv_bake_vertices_backward")
        return grad_images, grad_sv, None, None, None, None, None, None


def bake_uv_texture(images, uv_fragments, fragments, screen_vertices, perspective=True, depth_tolerance=1e-2, background=None,
                    cache=None):
    """(texture [B,T,T,C], mask [B,T,T]) of images [B,C,H,W] (f32 on the records' device, output orientation: row 0 = top; any
    H, W -- the photograph may be finer than the record --; 1 <= C <= 64): what each of the B views of `fragments` shows of
    every texel of the layout record `uv_fragments` (uv_layout_fragments; its triangles are the view record's, one for one).
    screen_vertices [B,V,3] f32: THE vertices `fragments` was rasterised from (their values cannot be checked; shape, dtype,
    device and V are).  perspective: whether they come from a perspective camera (the surface point is then the
    perspective-correct one).  depth_tolerance >= 0: a texel whose pixel belongs to another triangle is visible iff its depth
    is at most the z-buffer's plus this.  background: None (zeros), a float or [C], the value of an invisible texel.  The
    texture is channels last, texture row j = row j of the layout: what sample_uv_texture takes.  mask is 1 or 0.  The module's
    docstring states the function; the triangle's orientation in the view is not tested (no backface culling).

    Differentiable in `images` and in `screen_vertices` (x, y and z); visibility and the choice of taps are constants, the
    mask is not differentiable.  One launch forward; backward three launches for the images and, when the vertices require
    grad, four more (five on a mesh with hub vertices) -- vertices that do not require grad launch nothing extra.  The first
    call with the view record's tri builds the faces' adjacency (outside any stream capture; `cache`: the AdjacencyCache to
    keep it in).  ValueError, before anything is launched, for a wrong rank, dtype, device, B, V, number of triangles, C,
    an anti-aliased layout record, a negative depth_tolerance or a wrong background."""
    if not torch.is_tensor(images) or images.dim() != 4 or images.shape[2] < 1 or images.shape[3] < 1:
        raise ValueError("bake_uv_texture: images must be [B, C, H, W]")
    if images.dtype != torch.float32:
        raise ValueError("bake_uv_texture: images must be float32")
    C, H, W = _sizes(images)
    if not 1 <= C <= MAX_CHANNELS:
        raise ValueError(f"bake_uv_texture: images: 1 to {MAX_CHANNELS} channels")
    if H > MAX_IMAGE_SIZE or W > MAX_IMAGE_SIZE:
        raise ValueError(f"bake_uv_texture: images: at most {MAX_IMAGE_SIZE} rows and columns")
    B, Ft, _ = _checked_fragments(fragments)
    if not isinstance(uv_fragments, Fragments):
        raise ValueError("bake_uv_texture: uv_fragments must be the Fragments record of uv_layout_fragments")
    uv_B, uv_Ft, _ = _checked_fragments(uv_fragments)
    if uv_B != 1:
        raise ValueError("bake_uv_texture: uv_fragments must be a layout record of one view (uv_layout_fragments)")
    if uv_fragments.anti_aliasing:
        raise ValueError("bake_uv_texture: uv_fragments were made with anti_aliasing=True; a layout record has one texel per "
                         "raster pixel (uv_layout_fragments)")
    if uv_Ft != Ft:
        raise ValueError(f"bake_uv_texture: uv_fragments have {uv_Ft} triangles, fragments {Ft}: the layout's triangles must "
                         "be the mesh's, one for one")
    if images.shape[0] != B:
        raise ValueError(f"bake_uv_texture: images must be [{B}, C, H, W] for fragments of {B} views")
    dev = fragments.face_index_map.device
    if images.device != dev or uv_fragments.face_index_map.device != dev:
        raise ValueError("bake_uv_texture: images and uv_fragments must be on the fragments' device")
    _checked_screen_vertices(screen_vertices, fragments, "bake_uv_texture")
    if isinstance(depth_tolerance, bool) or not isinstance(depth_tolerance, (int, float)):
        raise ValueError("bake_uv_texture: depth_tolerance must be a float")
    depth_tolerance = float(depth_tolerance)
    if not (depth_tolerance >= 0.0 and math.isfinite(depth_tolerance)):
        raise ValueError("bake_uv_texture: depth_tolerance must be finite and >= 0")
    bake_adjoint_fraction_bits(uv_fragments.image_size)
    background = _checked_background(background, C, images)
    adjacency = vertex_adjacency(fragments.tri, fragments.num_vertices, cache)     # (where tri's indices are checked against V)
    if not images.is_cuda:
        raise ValueError("bake_uv_texture: images and fragments must be on one GPU device")
    return _BakeUvTexture.apply(images, screen_vertices, uv_fragments, fragments, adjacency, int(bool(perspective)),
                                depth_tolerance, background)
