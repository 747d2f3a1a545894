"""Scenes, the element-wise restatement, the adjoint's reference, the bounds and the numpy emulation of the adjoint's number
format for the per-pixel uv texture images (neural_renderer/uv_texture_images.py, csrc/d3m_uv_texture.h), shared by
tests/test_uv_texture_images_host.py and tests/test_gpu_uv_texture_images.py.  Built on tests/vertex_attribute_scenes.py: its
scenes, its maps (oracle_maps on the host, fragment_maps of a device record), its weights u_c and U32."""
import numpy as np
import torch

from deep3dmap_amd.neural_renderer.uv_texture_images import uv_adjoint_fraction_bits
from vertex_attribute_scenes import U32, _pool, _restate, scene

WRAPS = ("REPEAT", "MIRRORED_REPEAT", "CLAMP_TO_EDGE")

# ROUNDINGS of the expressions as written (csrc/d3m_uv_texture.h), evaluated in float32 on float32 maps and on corner uv that
# are wrapped in float32 in BOTH evaluations (wrap_uv is part of the input's definition, restated bit for bit):
#   pos:   u_c carries 2 (its division and its product), u_c uv_c 1, the two additions 2, the product with size - 1 one more:
#          6, relative to sum_c |u_c uv_c| (size - 1) <= size - 1 (the u_c are in [0, 1] and sum to 1, the wrapped uv lie in
#          [0, 1]); the clamp is exact.  delta = n_pos U32 (size - 1) bounds |pos_f32 - pos_f64|.
#   value, GIVEN pos: pos - (int)pos is exact; 1 - wx1 and 1 - wy1 round once each, the tap weight's product once (3 on
#          w_00), texel * weight 1, the additions from 0 three (0 + x is exact): 7; pooling adds three additions (the factor
#          1/4 is exact): 10, relative to sum_j |w_j texel_j|.  A background term is exact or meets the three additions.
#   an adjoint term w_j (scale g): 3 on the weight, 1 product (scale g is exact): 4, relative to |scale g| (w_j <= 1).
# The tests allow 1.5 x the derived count, the margin FORWARD_ROUNDINGS of the attribute node has (8 -> 12), nothing looser.
POS_ROUNDINGS = 9          # 1.5 x 6
VALUE_ROUNDINGS = 15       # 1.5 x 10
TERM_ROUNDINGS = 6         # 1.5 x 4


def seeded_faces_uv(name, spread, seed=23):
    """faces_uv [F,3,2] f32 of a scene.  spread 'seamless': per-vertex uv in [0, 1] gathered per corner (returns (faces_uv,
    vertex_uv [V,2])); 'corners': independent per-corner uv in [-0.75, 1.75], which every wrap has to fold (returns (faces_uv,
    None))."""
    sc = scene(name)
    tri = torch.from_numpy(sc["tri"]).long()
    gen = torch.Generator().manual_seed(seed)
    if spread == "seamless":
        uv = torch.rand(sc["vertices"].shape[0], 2, generator=gen)
        return uv[tri].contiguous(), uv
    assert spread == "corners"
    return (torch.rand(tri.shape[0], 3, 2, generator=gen) * 2.5 - 0.75).contiguous(), None


def seeded_image(H, W, C, batch=None, seed=31):
    gen = torch.Generator().manual_seed(seed + 1000 * H + 10 * W + C)
    return torch.randn((H, W, C) if batch is None else (batch, H, W, C), generator=gen)


def wrap_uv(v, wrapping):
    """wrap_uv of csrc/d3m_textures.h on a float32 tensor, bit for bit (fmod is exact, every other step rounds in float32)."""
    v = v.float()

    def tex_mod(x, y):
        r = torch.fmod(x, y)
        return torch.where(x > 0, r, y + r)
    if wrapping == "REPEAT":
        return tex_mod(v, 1.0)
    if wrapping == "MIRRORED_REPEAT":
        m = tex_mod(v, 1.0)
        return torch.where(tex_mod(v, 2.0) < 1, m, 1 - m)
    assert wrapping == "CLAMP_TO_EDGE"
    return v.clamp(max=1.0).clamp(min=0.0)


def _positions(maps, tri, faces_uv, H, W, wrapping, dtype):
    """(pos_x, pos_y [B,S,S] in dtype -- 0 where uncovered --, covered [B,S,S]) of the maps."""
    fi = maps["face_index_map"].long()
    dummy = torch.zeros(int(torch.as_tensor(tri).max()) + 1, 1, dtype=dtype)
    u, cov = _restate(maps, tri, dummy, None, False, dtype, False)[2:4]
    F = torch.as_tensor(tri).reshape(-1, 3).shape[0]
    fn = fi.clamp(min=0)
    cuv = wrap_uv(faces_uv, wrapping).to(dtype)[fn % F]               # [B,S,S,3,2]
    cuv = torch.where((fn >= F)[..., None, None], cuv.flip(-2), cuv)  # a fill_back copy reads corners 2 - c
    pu = (u[..., 0] * cuv[..., 0, 0] + u[..., 1] * cuv[..., 1, 0]) + u[..., 2] * cuv[..., 2, 0]
    pv = (u[..., 0] * cuv[..., 0, 1] + u[..., 1] * cuv[..., 1, 1]) + u[..., 2] * cuv[..., 2, 1]
    pos_x = (pu * (W - 1)).clamp(min=0.0).clamp(max=float(W - 1))
    pos_y = (pv * (H - 1)).clamp(min=0.0).clamp(max=float(H - 1))
    zero = torch.zeros((), dtype=dtype)
    return torch.where(cov, pos_x, zero), torch.where(cov, pos_y, zero), cov


def _taps(pos_x, pos_y, H, W):
    """texel_taps from pos on: ((y, x) of p00, p10, p01, p11, their weights)."""
    xi, yi = pos_x.long(), pos_y.long()
    wx1, wy1 = pos_x - xi.to(pos_x.dtype), pos_y - yi.to(pos_y.dtype)
    wx0, wy0 = 1 - wx1, 1 - wy1
    y1 = (pos_y + 1).long().clamp(max=H - 1)
    x1 = (xi + 1).clamp(max=W - 1)
    return ((yi, xi), (y1, xi), (yi, x1), (y1, x1)), (wx0 * wy0, wx0 * wy1, wx1 * wy0, wx1 * wy1)


def _restate_uv(maps, tri, faces_uv, image, background, anti_aliasing, wrapping, dtype, absolute=False):
    B, S = maps["face_index_map"].shape[:2]
    img = image.to(dtype)
    H, W, C = img.shape[-3:]
    pos_x, pos_y, cov = _positions(maps, tri, faces_uv, H, W, wrapping, dtype)
    pix, w = _taps(pos_x, pos_y, H, W)
    bidx = torch.arange(B)[:, None, None].expand(B, S, S)
    val = None
    for (y, x), wj in zip(pix, w):
        texel = img[y, x] if img.dim() == 3 else img[bidx, y, x]      # [B,S,S,C]
        term = texel * wj[..., None]
        if absolute:
            term = term.abs()
        val = term if val is None else val + term                    # (0 + the first term is exact)
    bg = torch.zeros(C, dtype=dtype) if background is None else torch.as_tensor(background, dtype=dtype).expand(C)
    if absolute:
        bg = bg.abs()
    val = torch.where(cov[..., None], val, bg.expand_as(val))
    out = val.permute(0, 3, 1, 2).flip(2)
    alpha = cov.to(dtype).flip(1)
    if anti_aliasing:
        out, alpha = _pool(out), _pool(alpha)
    return out, alpha, (pos_x, pos_y, cov, pix)


def restate_uv_texture_images(maps, tri, faces_uv, image, background, anti_aliasing, wrapping, dtype):
    """(images [B,C,s,s], alpha [B,s,s]) in `dtype`, element-wise torch operators only, of the semantics
    csrc/d3m_uv_texture.h states, on given maps: corners wrapped (in float32, as the input is defined), a fill_back copy
    reading corners 2 - c; pos = clamp(((u_0 uv_0 + u_1 uv_1) + u_2 uv_2) (size - 1), 0, size - 1); the four taps and weights
    of texel_taps; value = the four products added in the order p00, p10, p01, p11; background where uncovered; rows reversed;
    with anti-aliasing ((p00 + p01) + p10) + p11, times 1/4.  The rounding counts: the top of this file."""
    return _restate_uv(maps, tri, faces_uv, image, background, anti_aliasing, wrapping, dtype)[:2]


def _neighbourhood_max(d):
    """max of d [..,H,W,C] over the texels (y - 1 .. y + 2, x - 1 .. x + 2) (indices clamped): the differences that the 3 x 3
    cells around cell (y, x) interpolate"""
    H, W = d.shape[-3:-1]
    out = d
    for dy in (-1, 0, 1, 2):
        ys = (torch.arange(H) + dy).clamp(0, H - 1)
        for dx in (-1, 0, 1, 2):
            xs = (torch.arange(W) + dx).clamp(0, W - 1)
            out = torch.maximum(out, d[..., ys, :, :][..., xs, :])
    return out


def forward_bound(maps, tri, faces_uv, image, background, anti_aliasing, wrapping):
    """The allowed |device - float64 restatement| per output element [B,C,s,s].  Value and tap weights are continuous in pos
    (bilinear lookup, wrapping on the corners), so a different (int)pos in float64 costs nothing beyond this and no pixel is
    excluded.  Per internal pixel: VALUE_ROUNDINGS U32 sum_j |w_j texel_j| + delta_x max|D_x| + delta_y max|D_y|, delta =
    POS_ROUNDINGS U32 (size - 1), max|D| the largest difference of axis-neighbours among the texels of the 3 x 3 cells around
    the float64 cell (delta < 1: the float32 position lies in one of them); an uncovered pixel: VALUE_ROUNDINGS U32
    |background|.  Through the same flip and (linear) pooling."""
    img = image.double()
    H, W, C = img.shape[-3:]
    mag, _, (pos_x, pos_y, cov, pix) = _restate_uv(maps, tri, faces_uv, image, background, False, wrapping, torch.float64, True)
    B, S = cov.shape[:2]
    ys, xs = (torch.arange(H) + 1).clamp(max=H - 1), (torch.arange(W) + 1).clamp(max=W - 1)
    dx = _neighbourhood_max((img[..., xs, :] - img).abs())
    dy = _neighbourhood_max((img[..., ys, :, :] - img).abs())
    (yi, xi) = pix[0]
    bidx = torch.arange(B)[:, None, None].expand(B, S, S)
    mx = dx[yi, xi] if img.dim() == 3 else dx[bidx, yi, xi]
    my = dy[yi, xi] if img.dim() == 3 else dy[bidx, yi, xi]
    slope = POS_ROUNDINGS * U32 * ((W - 1) * mx + (H - 1) * my)
    slope = torch.where(cov[..., None], slope, torch.zeros_like(slope)).permute(0, 3, 1, 2).flip(2)
    bound = VALUE_ROUNDINGS * U32 * mag + slope
    return _pool(bound) if anti_aliasing else bound


# ---- the adjoint's reference and bound ------------------------------------------------------------------------------------
def adjoint64(maps, tri, faces_uv, image, grad_images, anti_aliasing, wrapping):
    """float64 autograd of the restatement with respect to `image` ([H,W,C] or [B,H,W,C]) for the image gradient grad_images."""
    g = grad_images.detach().double().cpu()
    a = image.detach().double().cpu().requires_grad_(True)
    out = _restate_uv(maps, tri, faces_uv, a, None, anti_aliasing, wrapping, torch.float64)[0]
    ref, = torch.autograd.grad((out * g).sum(), a)
    return ref


def quantum(grad_images, anti_aliasing, B, S):
    """q = 2^(E - frac) of a call (0.0 when the gradient is all zeros)."""
    scale = np.float32(0.25 if anti_aliasing else 1.0)
    gmax = float(np.abs(grad_images.detach().cpu().numpy().astype(np.float32) * scale).max())
    if gmax == 0.0:
        return 0.0
    return float(np.ldexp(1.0, int(np.floor(np.log2(gmax))) + 1 - uv_adjoint_fraction_bits(B, S)))


def _reach(maps, tri, faces_uv, image_shape, grad_images, anti_aliasing, wrapping):
    """Per element of grad_image: (the sum of |scale g| over the pixels whose float64 pos lies within 1 + delta of the texel
    on both axes [n_img H W, C], the number of those pixels [n_img H W])."""
    shared = len(image_shape) == 3
    H, W, C = image_shape[-3:]
    B, S = maps["face_index_map"].shape[:2]
    pos_x, pos_y, cov = _positions(maps, tri, faces_uv, H, W, wrapping, torch.float64)
    g = grad_images.detach().double().cpu().abs() * (0.25 if anti_aliasing else 1.0)
    if anti_aliasing:
        g = g.repeat_interleave(2, -1).repeat_interleave(2, -2)
    sg = g.flip(2).permute(0, 2, 3, 1)                               # [B,S,S,C] at the internal pixels
    delta_x, delta_y = POS_ROUNDINGS * U32 * (W - 1), POS_ROUNDINGS * U32 * (H - 1)
    n_img = 1 if shared else B
    acc = torch.zeros(n_img * H * W, C, dtype=torch.float64)
    cnt = torch.zeros(n_img * H * W, dtype=torch.float64)
    base = torch.zeros(B, S, S, dtype=torch.long) if shared else (torch.arange(B) * H * W)[:, None, None].expand(B, S, S)
    fx, fy = pos_x.floor().long(), pos_y.floor().long()
    for oy in (-1, 0, 1, 2):
        ty = fy + oy
        for ox in (-1, 0, 1, 2):
            tx = fx + ox
            ok = cov & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H) & ((pos_x - tx).abs() < 1 + delta_x) & \
                ((pos_y - ty).abs() < 1 + delta_y)
            idx = (base + ty * W + tx)[ok]
            acc.index_add_(0, idx, sg[ok])
            cnt.index_add_(0, idx, torch.ones(idx.shape[0], dtype=torch.float64))
    return acc, cnt


def reach_counts(maps, tri, faces_uv, image_shape, anti_aliasing, wrapping):
    """The number of pixels that can reach each texel in either evaluation, in image_shape without the channels."""
    B, S = maps["face_index_map"].shape[:2]
    s = S // 2 if anti_aliasing else S
    cnt = _reach(maps, tri, faces_uv, image_shape, torch.zeros(B, image_shape[-1], s, s), anti_aliasing, wrapping)[1]
    return cnt.reshape(tuple(image_shape[:-1]))


def adjoint_bound(maps, tri, faces_uv, image_shape, grad_images, anti_aliasing, wrapping, result):
    """The allowed |device - adjoint64| per element of grad_image (`result`: the reference, in image_shape).  The weight of a
    pixel on texel (ty, tx) is hat(pos_x - tx) hat(pos_y - ty): continuous, at most 1, Lipschitz 1 in each axis.  Per element:
      the sum over the pixels whose float64 pos lies within 1 + delta of the texel on both axes (every pixel that reaches it
      in either evaluation) of (TERM_ROUNDINGS U32 + delta_x + delta_y) |scale g|;
      n_taps q / 2, n_taps = 4 x the number of those pixels (each term is rounded to a multiple of q once);
      U32 |result| (the conversion to float32)."""
    H, W = image_shape[-3:-1]
    B, S = maps["face_index_map"].shape[:2]
    acc, cnt = _reach(maps, tri, faces_uv, image_shape, grad_images, anti_aliasing, wrapping)
    coef = TERM_ROUNDINGS * U32 + POS_ROUNDINGS * U32 * (W - 1) + POS_ROUNDINGS * U32 * (H - 1)
    q = quantum(grad_images, anti_aliasing, B, S)
    bound = coef * acc + (4.0 * cnt * q / 2.0)[:, None]
    return bound.reshape(tuple(image_shape)) + U32 * result.abs()


# ---- the adjoint's number format in numpy ---------------------------------------------------------------------------------
def fixed_point_sum(terms, gmax, frac):
    """(the int64 sum, the float32 result) of float32 terms as the adjoint adds them: E = ilogb(gmax) + 1; each term becomes
    rint((double)t 2^(frac - E)) (round to nearest even, __double2ll_rn); int64 sum; (float)((double)sum 2^(E - frac))."""
    terms = np.asarray(terms, np.float32)
    E = int(np.floor(np.log2(float(gmax)))) + 1
    fixed = np.rint(terms.astype(np.float64) * np.ldexp(1.0, frac - E)).astype(np.int64)
    total = int(fixed.sum(dtype=np.int64))
    return total, np.float32(np.float64(total) * np.ldexp(1.0, E - frac))
