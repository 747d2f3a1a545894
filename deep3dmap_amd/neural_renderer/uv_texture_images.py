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
reaches gets +0.

With `mipmap` the lookup is trilinear in a box pyramid of the image at a level of detail per pixel, and the adjoint keeps one
int64 accumulator per element of every level, gathered back down the pyramid by the conversion in a fixed order: the same
guarantees, at most three launches forward and three backward.  csrc/d3m_uv_texture_mip.h states every step;
`texture_mip_pyramid` and `uv_texture_lod` show the pyramid and the level of detail on their own."""
import ctypes

import torch

from .. import _lib
from .attributes import (_checked_background, _checked_fragments, _checked_pixel_lanes, _checked_screen_vertices,
                         _node_geometry_adjoint)
from .row_gather import vertex_adjacency
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


def _checked_faces_uv(faces_uv, texture_wrapping, fragments, who):
    """(B, Ft, the wrapping's code) of a record and the faces_uv [Ft,3,2] that belong to its faces"""
    wrapping = _wrapping_code(texture_wrapping)
    if wrapping == CLAMP_TO_BORDER:
        raise ValueError(f"{who}: CLAMP_TO_BORDER is not offered (REPEAT, MIRRORED_REPEAT or CLAMP_TO_EDGE)")
    B, Ft, Fp = _checked_fragments(fragments)
    if faces_uv.dim() != 3 or tuple(faces_uv.shape) != (Ft, 3, 2):
        raise ValueError(f"faces_uv must be [{Ft}, 3, 2] for fragments of {Ft} faces")
    return B, Ft, wrapping


def _checked_uv_image(image, faces_uv, texture_wrapping, fragments, who, channels=None):
    """(B, Ft, H, W, C, the wrapping's code) of what every node that looks a texture image up over a record takes: the image
    [H,W,C] or [B,H,W,C] -- channels None: 1 <= C <= 64, else exactly `channels` --, faces_uv, the wrapping, the record with
    B S S within 2^32, all on the record's device.  The errors, in the order the nodes document."""
    if not torch.is_tensor(image) or not torch.is_tensor(faces_uv):
        raise TypeError("image and faces_uv must be tensors")
    if image.dtype != torch.float32 or faces_uv.dtype != torch.float32:
        raise TypeError("image and faces_uv must be float32")
    c = "C" if channels is None else channels
    if image.dim() not in (3, 4) or image.shape[-3] < 1 or image.shape[-2] < 1:
        raise ValueError(f"image must be [H, W, {c}] or [B, H, W, {c}]")
    H, W, C = image.shape[-3:]
    if channels is None and not 1 <= C <= MAX_CHANNELS:
        raise ValueError(f"image: 1 to {MAX_CHANNELS} channels")
    if channels is not None and C != channels:
        raise ValueError(f"image: an albedo has {channels} channels, not {C}")
    if H > MAX_IMAGE_SIZE or W > MAX_IMAGE_SIZE:
        raise ValueError(f"image: at most {MAX_IMAGE_SIZE} rows and columns")
    B, Ft, wrapping = _checked_faces_uv(faces_uv, texture_wrapping, fragments, who)
    if image.dim() == 4 and image.shape[0] != B:
        raise ValueError(f"image must be [H, W, {c}] or [{B}, H, W, {c}] for fragments of {B} views")
    if channels is None:
        uv_adjoint_fraction_bits(B, fragments.raster_size)            # (sample_uv_texture's own wording of the bound)
    else:
        _checked_pixel_lanes(fragments, who)
    if faces_uv.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError(f"{who}: no gradient with respect to faces_uv (it is a constant; detach it)")
    dev = fragments.face_index_map.device
    if image.device != dev or faces_uv.device != dev:
        raise ValueError("image and faces_uv must be on the fragments' device")
    return B, Ft, H, W, C, wrapping


def _uv_outputs(fr, img):
    """(images [B,C,s,s], alpha [B,s,s], the image's batch) of a contiguous image, uninitialised"""
    B, s = fr.face_index_map.shape[0], int(fr.image_size)
    images = torch.empty(B, img.shape[-1], s, s, dtype=torch.float32, device=img.device)
    alpha = torch.empty(B, s, s, dtype=torch.float32, device=img.device)
    return images, alpha, B if img.dim() == 4 else 1


def _uv_images_launch(fr, img, faces_uv, wrapping, background):
    """(images, alpha) of a contiguous image: the plain bilinear forward's one launch"""
    H, W, C = img.shape[-3:]
    images, alpha, ib = _uv_outputs(fr, img)
    c_fr = fr.c_struct()
    _lib.check(_lib.lib().d3m_uv_texture_images(ctypes.byref(c_fr), _lib.ptr(faces_uv), _lib.ptr(img), ib, H, W, C, wrapping,
                                                _lib.ptr(background), _lib.ptr(images), _lib.ptr(alpha), _lib.stream_ptr()),
               "d3m_uv_texture_images")
    return images, alpha


def _uv_images_adjoint(fr, g, batched, sizes, scratch_bytes, backward):
    """grad_image of the contiguous f32 image gradient g, the fixed-point scatter: backward(c_fr, ib, scratch, bytes, grad)
    is the plain or the mip-mapped entry point, scratch_bytes its scratch size for the image's batch ib"""
    B, H, W, C = sizes
    ib = B if batched else 1
    scratch = torch.empty((int(scratch_bytes(ib)) + 7) // 8, dtype=torch.int64, device=g.device)
    grad = torch.empty((B, H, W, C) if batched else (H, W, C), dtype=torch.float32, device=g.device)
    c_fr = fr.c_struct()
    backward(ctypes.byref(c_fr), ib, _lib.ptr(scratch), scratch.numel() * 8, _lib.ptr(grad))
    return grad


class _UvTextureImages(torch.autograd.Function):
    """screen_vertices: None, or the vertices the record was rasterised from as a second differentiable input -- the same
    forward launch and the same adjoint for the image; the vertices' gradient through the node's pixel_grads and the shared
    interior adjoint (csrc/d3m_fragment_geometry.h).  The image is kept for the backward only when the vertices need a
    gradient."""
    @staticmethod
    def forward(ctx, image, screen_vertices, faces_uv, fragments, adjacency, wrapping, background):
        img = image.contiguous()
        images, alpha = _uv_images_launch(fragments, img, faces_uv, wrapping, background)
        if ctx.needs_input_grad[1]:
            ctx.save_for_backward(img)
        ctx.fragments, ctx.faces_uv, ctx.wrapping, ctx.batched = fragments, faces_uv, wrapping, img.dim() == 4
        ctx.adjacency, ctx.sizes = adjacency, (images.shape[0],) + tuple(img.shape[-3:])
        ctx.mark_non_differentiable(alpha)
        return images, alpha

    @staticmethod
    def backward(ctx, grad_images, _grad_alpha):
        fr, L = ctx.fragments, _lib.lib()
        B, H, W, C = ctx.sizes
        uv, wrapping = _lib.ptr(ctx.faces_uv), ctx.wrapping
        g = grad_images.to(torch.float32).contiguous()
        grad_image = None
        if ctx.needs_input_grad[0]:
            grad_image = _uv_images_adjoint(
                fr, g, ctx.batched, ctx.sizes, lambda ib: L.d3m_uv_texture_images_scratch_bytes(ib, H, W, C, B, fr.raster_size),
                lambda c_fr, ib, scratch, n, grad: _lib.check(L.d3m_uv_texture_images_backward(
                    c_fr, uv, _lib.ptr(g), ib, H, W, C, wrapping, scratch, n, grad, _lib.stream_ptr()),
                    "d3m_uv_texture_images_backward"))
        grad_sv = None
        if ctx.needs_input_grad[1]:
            img, = ctx.saved_tensors
            grad_sv = _node_geometry_adjoint(fr, ctx.adjacency, lambda c_fr, h: _lib.check(L.d3m_uv_texture_pixel_grads(
                c_fr, uv, _lib.ptr(img), B if ctx.batched else 1, H, W, C, wrapping, _lib.ptr(g), h, _lib.stream_ptr()),
                "d3m_uv_texture_pixel_grads"))
        return grad_image, grad_sv, None, None, None, None, None


# ---- mip-mapping (csrc/d3m_uv_texture_mip.h) --------------------------------------------------------------------------------
MAX_LEVEL = 15             # UVT_MAX_LEVEL


def _trailing_zeros(n):
    return (n & -n).bit_length() - 1


def mip_levels(H, W, mipmap):
    """L, the number of pyramid levels above level 0, of `mipmap` for an H x W image: None, False or 0 -> 0 (no mip-mapping);
    True -> min(ctz H, ctz W, 15), the most the sizes allow (ValueError when that is 0: an odd side); an int L in 1..15 -> L
    (ValueError unless 2^L divides H and W)."""
    if mipmap is None or mipmap is False:
        return 0
    if mipmap is True:
        L = min(_trailing_zeros(int(H)), _trailing_zeros(int(W)), MAX_LEVEL)
        if L < 1:
            raise ValueError(f"mipmap=True: a {H} x {W} image has an odd side, so no level above 0")
        return L
    if not isinstance(mipmap, int):
        raise TypeError("mipmap must be None, a bool or an int")
    if mipmap == 0:
        return 0
    if not 1 <= mipmap <= MAX_LEVEL:
        raise ValueError(f"mipmap: 1 to {MAX_LEVEL} levels")
    if H % (1 << mipmap) or W % (1 << mipmap):
        raise ValueError(f"mipmap={mipmap}: H = {H} and W = {W} must be divisible by {1 << mipmap}")
    return mipmap


def _checked_lod_bias(lod_bias):
    if isinstance(lod_bias, bool) or not isinstance(lod_bias, (int, float)):
        raise TypeError("lod_bias must be a float")
    lod_bias = float(lod_bias)
    if lod_bias != lod_bias or lod_bias in (float("inf"), float("-inf")):
        raise ValueError("lod_bias must be finite")
    return lod_bias


def _level_sizes(H, W, L):
    return [(H >> l, W >> l) for l in range(L + 1)]


def _build_pyramid(img, L):
    """[n_img, T, C]: every level of a contiguous image [H,W,C] or [B,H,W,C], one buffer (at most two launches)."""
    H, W, C = img.shape[-3:]
    n_img = img.shape[0] if img.dim() == 4 else 1
    T = sum(h * w for h, w in _level_sizes(H, W, L))
    pyramid = torch.empty(n_img, T, C, dtype=torch.float32, device=img.device)
    _lib.check(_lib.lib().d3m_texture_mip_pyramid(_lib.ptr(img), n_img, H, W, C, L, _lib.ptr(pyramid), _lib.stream_ptr()),
               "d3m_texture_mip_pyramid")
    return pyramid


class _UvTextureMipImages(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, faces_uv, fragments, wrapping, background, levels, lod_bias):
        fr = fragments
        img = image.contiguous()
        H, W, C = img.shape[-3:]
        pyramid = _build_pyramid(img, levels)                         # transient: the backward does not read it
        images, alpha, ib = _uv_outputs(fr, img)
        c_fr = fr.c_struct()
        _lib.check(_lib.lib().d3m_uv_texture_mip_images(ctypes.byref(c_fr), _lib.ptr(faces_uv), _lib.ptr(pyramid), ib, H, W, C,
                                                        wrapping, levels, lod_bias, _lib.ptr(background), _lib.ptr(images),
                                                        _lib.ptr(alpha), _lib.stream_ptr()), "d3m_uv_texture_mip_images")
        ctx.fragments, ctx.faces_uv, ctx.wrapping, ctx.batched = fr, faces_uv, wrapping, img.dim() == 4
        ctx.sizes, ctx.levels, ctx.lod_bias = (images.shape[0], H, W, C), levels, lod_bias
        ctx.mark_non_differentiable(alpha)
        return images, alpha

    @staticmethod
    def backward(ctx, grad_images, _grad_alpha):
        fr, L = ctx.fragments, _lib.lib()
        B, H, W, C = ctx.sizes
        g = grad_images.to(torch.float32).contiguous()
        grad = _uv_images_adjoint(
            fr, g, ctx.batched, ctx.sizes,
            lambda ib: L.d3m_uv_texture_mip_images_scratch_bytes(ib, H, W, C, ctx.levels, B, fr.raster_size),
            lambda c_fr, ib, scratch, n, grad: _lib.check(L.d3m_uv_texture_mip_images_backward(
                c_fr, _lib.ptr(ctx.faces_uv), _lib.ptr(g), ib, H, W, C, ctx.wrapping, ctx.levels, ctx.lod_bias, scratch, n, grad,
                _lib.stream_ptr()), "d3m_uv_texture_mip_images_backward"))
        return grad, None, None, None, None, None, None


def sample_uv_texture(image, faces_uv, fragments, texture_wrapping='REPEAT', background=None, mipmap=None, lod_bias=0.0,
                      screen_vertices=None, cache=None):
    """(images [B,C,s,s], alpha [B,s,s]) of a texture image [H,W,C] (shared by the views) or [B,H,W,C], f32 on the record's
    device, 1 <= C <= 64, texture space as textures_from_image reads it; faces_uv [F,3,2] f32 for the record's F faces, a
    constant; texture_wrapping 'REPEAT', 'MIRRORED_REPEAT' or 'CLAMP_TO_EDGE' (or 0..2), applied to the corners; background:
    None (zeros), a float, or [C].  Differentiable in `image` only: faces_uv that requires grad raises NotImplementedError;
    alpha is the coverage (the bits of interpolate_vertex_attributes' alpha), not differentiable.

    mipmap None or 0: four bilinear taps per pixel, right when the texture is magnified.  mipmap = L (an int, 2^L dividing H
    and W) or True (the largest such L, at most 15; an odd side is a ValueError): a box pyramid of L levels above the image is
    built and every pixel takes eight taps, trilinearly, at its own level of detail lambda_c = clamp(log2(texels per pixel
    step) + lod_bias, 0, L) -- no aliasing when the texture is minified, and the image's gradient reaches every texel under a
    pixel's footprint instead of four (csrc/d3m_uv_texture_mip.h).  lod_bias: a finite float.

    screen_vertices None: as above.  screen_vertices [B,V,3] f32 on the record's device -- THE vertices the record was
    rasterised from, still attached to the graph (their values cannot be checked; shape, dtype, device and V are): the same
    forward launch and the same bits of images, alpha and the image's gradient, and in addition the INTERIOR geometry
    gradient reaches screen_vertices.grad: the four taps' slope along pos times the derivative of the weights u_c with
    respect to the owner's corners (csrc/d3m_fragment_geometry.h), in a fixed order.  Coverage stays a constant (the
    silhouette gradient is render_silhouettes' / render's) and so does faces_uv.  Plain bilinear lookup only: with mipmap
    the level of detail depends on the geometry, and NotImplementedError is raised.  Vertices that do not require grad
    launch nothing extra; the first call with the record's tri builds the faces' adjacency (outside any stream capture;
    `cache`: the AdjacencyCache to keep it in).

    ValueError / TypeError, before anything is launched, for a wrong rank, dtype, device, C, F, batch, wrapping, background,
    mipmap, lod_bias or screen_vertices, and for a record with B S S beyond 2^32."""
    B, Ft, H, W, C, wrapping = _checked_uv_image(image, faces_uv, texture_wrapping, fragments, "sample_uv_texture")
    levels = mip_levels(H, W, mipmap)
    lod_bias = _checked_lod_bias(lod_bias)
    adjacency = None
    if screen_vertices is not None:
        _checked_screen_vertices(screen_vertices, fragments, "sample_uv_texture")
        if levels != 0:
            raise NotImplementedError("sample_uv_texture: no geometry gradient with mipmap (the level of detail depends on "
                                      "the geometry); pass mipmap=None or screen_vertices=None")
        if screen_vertices.requires_grad and torch.is_grad_enabled():
            adjacency = vertex_adjacency(fragments.tri, fragments.num_vertices, cache)
    background = _checked_background(background, C, image)
    if not image.is_cuda:
        raise ValueError("image and fragments must be on one GPU device")
    if levels == 0:
        return _UvTextureImages.apply(image, screen_vertices if adjacency is not None else None, faces_uv.detach().contiguous(),
                                      fragments, adjacency, wrapping, background)
    return _UvTextureMipImages.apply(image, faces_uv.detach().contiguous(), fragments, wrapping, background, levels, lod_bias)


def texture_mip_pyramid(image, levels):
    """The box pyramid of image [H,W,C] or [B,H,W,C] (f32, on a GPU, 2^levels dividing H and W, 1 <= levels <= 15) as a list of
    levels + 1 detached tensors, level l of shape [..., H >> l, W >> l, C]: level 0 is the image, a texel of level l + 1 is
    (((a00 + a01) + a10) + a11) * 0.25 of level l's (2y, 2x), (2y, 2x+1), (2y+1, 2x), (2y+1, 2x+1)."""
    if not torch.is_tensor(image):
        raise TypeError("image must be a tensor")
    if image.dtype != torch.float32:
        raise TypeError("image must be float32")
    if image.dim() not in (3, 4) or image.shape[-3] < 1 or image.shape[-2] < 1 or (image.dim() == 4 and image.shape[0] < 1):
        raise ValueError("image must be [H, W, C] or [B, H, W, C]")
    H, W, C = image.shape[-3:]
    if not 1 <= C <= MAX_CHANNELS:
        raise ValueError(f"image: 1 to {MAX_CHANNELS} channels")
    if H > MAX_IMAGE_SIZE or W > MAX_IMAGE_SIZE:
        raise ValueError(f"image: at most {MAX_IMAGE_SIZE} rows and columns")
    if isinstance(levels, bool) or not isinstance(levels, int):
        raise TypeError("levels must be an int")
    L = mip_levels(H, W, levels)
    if L < 1:
        raise ValueError(f"levels: 1 to {MAX_LEVEL}")
    if not image.is_cuda:
        raise ValueError("image must be on a GPU device")
    pyramid = _build_pyramid(image.detach().contiguous(), L)
    out, first = [], 0
    for h, w in _level_sizes(H, W, L):
        level = pyramid[:, first:first + h * w].reshape(-1, h, w, C)
        out.append(level if image.dim() == 4 else level[0])
        first += h * w
    return out


def uv_texture_lod(faces_uv, fragments, size, texture_wrapping='REPEAT', lod_bias=0.0, levels=None):
    """lambda_c [B,S,S] (S the record's raster size) of sample_uv_texture(..., mipmap=levels, lod_bias=lod_bias) for a texture of
    size = (H, W): the level of detail of every internal pixel, in [0, levels], 0 where uncovered, in the orientation of the
    record's maps (row 0 = bottom).  levels None: the largest the sizes allow.  Not differentiable."""
    if not torch.is_tensor(faces_uv):
        raise TypeError("faces_uv must be a tensor")
    if faces_uv.dtype != torch.float32:
        raise TypeError("faces_uv must be float32")
    try:
        H, W = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError("size must be (H, W)")
    if not (1 <= H <= MAX_IMAGE_SIZE and 1 <= W <= MAX_IMAGE_SIZE):
        raise ValueError(f"size: 1 to {MAX_IMAGE_SIZE} rows and columns")
    B, Ft, wrapping = _checked_faces_uv(faces_uv, texture_wrapping, fragments, "uv_texture_lod")
    L = mip_levels(H, W, True if levels is None else levels)
    if L < 1:
        raise ValueError(f"levels: 1 to {MAX_LEVEL}")
    lod_bias = _checked_lod_bias(lod_bias)
    dev = fragments.face_index_map.device
    if faces_uv.device != dev:
        raise ValueError("faces_uv must be on the fragments' device")
    if not faces_uv.is_cuda:
        raise ValueError("faces_uv and fragments must be on one GPU device")
    S = int(fragments.raster_size)
    lod = torch.empty(B, S, S, dtype=torch.float32, device=dev)
    c_fr = fragments.c_struct()
    uv = faces_uv.detach().contiguous()
    _lib.check(_lib.lib().d3m_uv_texture_lod(ctypes.byref(c_fr), _lib.ptr(uv), H, W, wrapping, L, lod_bias, _lib.ptr(lod),
                                             _lib.stream_ptr()), "d3m_uv_texture_lod")
    return lod
