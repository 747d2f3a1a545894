"""Inputs, the float64 restatement and the references of the per-pixel spherical-harmonic shading of a UV albedo texture
(neural_renderer/sh_uv_fragments.py, csrc/d3m_sh_uv_fragments.h), shared by tests/test_sh_uv_fragments_host.py and
tests/test_gpu_sh_uv_fragments.py.  Built on tests/sh_fragment_scenes.py (cases, cone / smooth normals, seeded_sh, the light's
restatement, errors_of), tests/uv_texture_image_scenes.py (seeded_faces_uv, seeded_image, wrap_uv, _taps) and
tests/fragment_geometry_scenes.py (weights_of, _clamp_flat, near_integer_mask, UV_SEED, UV_CASES, UV_SIZES).

THE FUNCTION (shade_uv_images_of), element-wise torch operators on given maps, in any dtype: u_c = weight_map * (depth_map /
z_c); s_k of sh_fragment_scenes.shade_images_of without colours (m, r, n = m / max(r, 1e-6), the nine terms ascending); pos =
clamp(((u_0 uv_0 + u_1 uv_1) + u_2 uv_2) (size - 1), 0, size - 1) with the corners wrapped in float32 and a fill_back copy
reading corners 2 - c, the derivative of the clamp 0 AT a limit; the four taps of _taps CHOSEN FROM THE DETACHED POSITION, their
weights differentiable in it; a_k = the four products added in tap order; value_k = a_k s_k; background where uncovered; rows
reversed; with anti-aliasing ((p00 + p01) + p10) + p11, times 1/4, AFTER the product.  The gradients are torch autograd's of
that expression; with screen vertices u takes its VALUE from the maps and its DERIVATIVE from
fragment_geometry_scenes.weights_of (what the kernels do).

THE CASES: sh_fragment_scenes.CASES (S1, S2 at 16 and 32 with and without anti-aliasing, S3B at 128, S4 at 16 and 32; B = 2)
crossed with UV_SIZES (8 x 8, 32 x 16) and UV_CASES (seamless and per-corner uv, the three wrappings), faces_uv seeded with
UV_SEED, and with the normal kinds of sh_fragment_scenes.NORMAL_KINDS.

TWO CONDITIONS (tests/test_sh_uv_fragments_host.py asserts both on the CPU): min r >= 0.7 over covered pixels (the inputs are
sh_fragment_scenes'); the geometry gradient is compared with the image gradient zeroed at the output pixels
near_integer_mask names (float32 and float64 may choose different taps there and the slope along pos jumps across a texel
boundary), at most MAX_ZEROED_SHARE = 2 % of the covered output pixels of a case.  The image and the other gradients are
continuous across a texel boundary and are compared everywhere.

THE DEVICE TOLERANCE (measured on the CPU, docs/EXPERIMENTS.md "SH shading of a UV albedo: the float32 yardstick").  The
yardstick is the error of this very expression evaluated by torch in float32 against float64 on the oracle's maps, under
torch.use_deterministic_algorithms(True), with per-view inputs ([B,H,W,3] image, [B,V,3] normals, [B,3,9] light); per view in
units of the view's largest float64 entry; the larger of a case's views, normal kinds, anti-aliasing settings, texture sizes
and uv cases.  YARDSTICK holds the figures per case and kind; the host test measures them again and holds them within a factor
2.  The device gets 8 x the largest of a kind (the light's: 8 x the figure at S3B/128): the family's margin for another
association, FMA contraction and the kernels' own summation order.  The albedo image's gradient gets the fixed-point term on
top (fixed_point_bound): every term is rounded to a multiple of the quantum q = 2^(E - frac) once, so a texel is off by at
most (terms reaching it) q / 2 <= 4 B S^2 q / 2; E - 1 = ilogb(max |Qa|) and |Qa| <= max |scale g| max |s|, taken from the
float64 restatement and doubled (one binade of room for rounding); frac = uv_adjoint_fraction_bits(B, S) >= 47 at these sizes,
so the term is below 1e-7 of the largest entry everywhere -- derived, not measured."""
import math

import torch

import fragment_geometry_scenes as FG
import sh_fragment_scenes as SF
import uv_texture_image_scenes as UV
import vertex_attribute_scenes as VA
from deep3dmap_amd.neural_renderer.uv_texture_images import uv_adjoint_fraction_bits
from fragment_geometry_scenes import UV_CASES, UV_SEED, UV_SIZES
from vertex_attribute_scenes import _pool, scene

KINDS = ("image", "normals", "sh", "albedo", "screen_vertices")
CASES = SF.CASES
MIN_R = SF.MIN_R
MAX_ZEROED_SHARE = FG.MAX_ZEROED_SHARE

# per case "scene/S": the float32 yardstick of each kind (the larger of everything the case is crossed with)
YARDSTICK = {
    "S1/16": dict(image=3.57e-06, normals=2.81e-06, sh=3.64e-06, albedo=2.49e-06, screen_vertices=2.33e-06),
    "S1/32": dict(image=4.77e-06, normals=3.32e-06, sh=4.53e-06, albedo=3.58e-06, screen_vertices=4.99e-06),
    "S2/16": dict(image=4.05e-06, normals=4.65e-06, sh=7.75e-06, albedo=2.49e-06, screen_vertices=2.93e-06),
    "S2/32": dict(image=3.58e-06, normals=2.65e-06, sh=8.29e-06, albedo=2.96e-06, screen_vertices=2.65e-06),
    "S3B/128": dict(image=7.15e-06, normals=4.89e-06, sh=2.97e-06, albedo=2.03e-06, screen_vertices=5.95e-06),
    "S4/16": dict(image=3.56e-06, normals=2.82e-06, sh=4.68e-06, albedo=3.11e-06, screen_vertices=4.46e-06),
    "S4/32": dict(image=4.65e-06, normals=3.30e-06, sh=4.79e-06, albedo=3.13e-06, screen_vertices=2.75e-06),
}
DEVICE_TOLERANCE = {k: 8 * max(y[k] for y in YARDSTICK.values()) for k in KINDS if k != "sh"}
DEVICE_TOLERANCE["sh"] = 8 * YARDSTICK["S3B/128"]["sh"]


# ---- the inputs -----------------------------------------------------------------------------------------------------------
def uv_combos():
    """((H, W), spread, wrapping): the textures and uv cases every scene case is crossed with"""
    return [(size, spread, wrapping) for size in UV_SIZES for spread, wrapping in UV_CASES]


def faces_uv_of(name, spread):
    return UV.seeded_faces_uv(name, spread, seed=UV_SEED)[0]


def albedo_of(H, W, B=None):
    """a seeded albedo image [H,W,3] or [B,H,W,3]"""
    return UV.seeded_image(H, W, 3, B)


def layouts():
    """(image batched, normals batched, sh batched): the full product"""
    return [(ib, nb, sb) for ib in (False, True) for nb in (False, True) for sb in (False, True)]


def inputs_of(name, kind, layout, H, W, B):
    ib, nb, sb = layout
    return albedo_of(H, W, B if ib else None), SF.normals_of(name, kind, nb), SF.seeded_sh(B if sb else None)


# ---- the restatement ------------------------------------------------------------------------------------------------------
def _weights(maps, tri, V, dtype, screen_vertices, values_from_maps):
    u, cov = VA._restate(maps, tri, torch.zeros(V, 1, dtype=dtype), None, False, dtype, False)[2:4]
    if screen_vertices is not None:
        ue = FG.weights_of(maps, tri, screen_vertices, dtype)[0]
        u = u + (ue - ue.detach()) if values_from_maps else ue
    return u, cov


def albedo_of_pixels(maps, tri, image, faces_uv, wrapping, dtype, u, cov):
    """a [B,S,S,3] in dtype: the lookup at every internal pixel (0 where uncovered), differentiable in image and u"""
    fn = maps["face_index_map"].long().clamp(min=0)
    B, S = cov.shape[:2]
    img = image.to(dtype)
    H, W = img.shape[-3:-1]
    F = torch.as_tensor(tri).reshape(-1, 3).shape[0]
    cuv = UV.wrap_uv(faces_uv, wrapping).to(dtype)[fn % F]            # [B,S,S,3,2]
    cuv = torch.where((fn >= F)[..., None, None], cuv.flip(-2), cuv)  # a fill_back copy reads corners 2 - c
    pu = (u[..., 0] * cuv[..., 0, 0] + u[..., 1] * cuv[..., 1, 0]) + u[..., 2] * cuv[..., 2, 0]
    pv = (u[..., 0] * cuv[..., 0, 1] + u[..., 1] * cuv[..., 1, 1]) + u[..., 2] * cuv[..., 2, 1]
    zero = torch.zeros((), dtype=dtype)
    pos_x = torch.where(cov, FG._clamp_flat(pu * (W - 1), float(W - 1)), zero)
    pos_y = torch.where(cov, FG._clamp_flat(pv * (H - 1), float(H - 1)), zero)
    pix, w = UV._taps(pos_x, pos_y, H, W)                             # (.long(): the taps are chosen from the detached position)
    bidx = torch.arange(B)[:, None, None].expand(B, S, S)
    val = None
    for (y, x), wj in zip(pix, w):
        term = (img[y, x] if img.dim() == 3 else img[bidx, y, x]) * wj[..., None]
        val = term if val is None else val + term
    return val


def shade_uv_images_of(maps, tri, image, faces_uv, normals, sh, background, anti_aliasing, wrapping, dtype,
                       screen_vertices=None, values_from_maps=True, composed=False):
    """(images [B,3,s,s] in dtype, r [B,S,S] of the covered pixels (1 elsewhere), covered [B,S,S]).  values_from_maps=False: u
    is the expression's in the screen vertices alone, value and derivative (what finite differences see).  composed=True:
    NOT this node but the route it replaces -- pool(a, background 0) * pool(s, background 1), each pooled on its own."""
    V = normals.shape[-2]
    # s_k at the internal pixels, in the maps' orientation: the light's restatement without colours, background or pooling
    shade, r, cov = SF.shade_images_of(maps, tri, normals, sh, None, None, False, dtype, screen_vertices, values_from_maps)
    s = shade.flip(2).permute(0, 2, 3, 1)
    u, _ = _weights(maps, tri, V, dtype, screen_vertices, values_from_maps)
    a = albedo_of_pixels(maps, tri, image, faces_uv, wrapping, dtype, u, cov)

    def finish(val, bg):
        bg = torch.zeros(3, dtype=dtype) if bg is None else torch.as_tensor(bg, dtype=dtype).expand(3)
        img = torch.where(cov[..., None], val, bg.expand_as(val)).permute(0, 3, 1, 2).flip(2)
        return _pool(img) if anti_aliasing else img

    if composed:
        return finish(a, 0.0) * finish(s, 1.0), r, cov
    return finish(a * s, background), r, cov


def reference(maps, tri, image, faces_uv, normals, sh, screen_vertices, grad_out, anti_aliasing, wrapping, background=None,
              dtype=torch.float64, keep=None):
    """dict(image, albedo, normals, sh, screen_vertices) in dtype: the restatement and its autograd gradients for the image
    gradient grad_out -- screen_vertices' for grad_out * keep (near_integer_mask's), the others' for grad_out everywhere"""
    leaf = lambda t: t.detach().cpu().to(dtype).requires_grad_(True)
    a, n, s, sv = leaf(image), leaf(normals), leaf(sh), leaf(screen_vertices)
    img = shade_uv_images_of(maps, tri, a, faces_uv, n, s, background, anti_aliasing, wrapping, dtype, sv)[0]
    g = grad_out.detach().cpu().to(dtype)
    ga, gn, gs = torch.autograd.grad((img * g).sum(), (a, n, s), retain_graph=True)
    gsv, = torch.autograd.grad((img * (g if keep is None else g * keep.to(dtype))).sum(), sv)
    return dict(image=img.detach(), albedo=ga, normals=gn, sh=gs, screen_vertices=gsv)


errors_of = SF.errors_of


def fixed_point_bound(maps, tri, normals, sh, grad_out, anti_aliasing):
    """the most the fixed-point sum moves an element of the albedo image's gradient (absolute): 4 B S^2 q / 2 with q from
    twice the float64 bound max |scale g| max |s| on the gradient image's largest entry (the module docstring)"""
    B, S = maps["face_index_map"].shape[:2]
    shade = SF.shade_images_of(maps, tri, normals.double(), sh.double(), None, None, False, torch.float64)[0]
    gmax = 2.0 * float(grad_out.abs().max()) * (0.25 if anti_aliasing else 1.0) * float(shade.abs().max())
    q = math.ldexp(1.0, math.floor(math.log2(gmax)) + 1 - uv_adjoint_fraction_bits(B, S))
    return 4.0 * B * S * S * q / 2.0


def measure_yardstick(name, S):
    """({kind: the float32 yardstick of case name/S}, the largest zeroed share, the smallest r): the larger of the views, the
    normal kinds, the anti-aliasing settings, the texture sizes and the uv cases the case runs with (call under
    torch.use_deterministic_algorithms(True))"""
    maps, tri, sv = VA.oracle_maps(name, S), scene(name)["tri"], FG.screen_vertices(name)
    B = sv.shape[0]
    worst, share, min_r = dict.fromkeys(KINDS, 0.0), 0.0, 1.0
    for aa in sorted({aa for n, s, aa in CASES if (n, s) == (name, S)}):
        g = SF.seeded_grad_out(B, S // 2 if aa else S)
        for (H, W), spread, wrapping in uv_combos():
            uv = faces_uv_of(name, spread)
            keep, zeroed = FG.near_integer_mask(maps, tri, uv, H, W, aa, wrapping)
            share = max(share, zeroed)
            for kind in SF.NORMAL_KINDS[name]:
                args = (maps, tri, albedo_of(H, W, B), uv, SF.normals_of(name, kind, True), SF.seeded_sh(B), sv, g, aa, wrapping)
                r64, r32 = reference(*args, keep=keep), reference(*args, dtype=torch.float32, keep=keep)
                for k in KINDS:
                    worst[k] = max(worst[k], max(errors_of(r32[k], r64[k])))
                r, cov = shade_uv_images_of(maps, tri, args[2], uv, args[4], args[5], None, aa, wrapping, torch.float64)[1:]
                min_r = min(min_r, float(r[cov].min()))
    return worst, share, min_r
