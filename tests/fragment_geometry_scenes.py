"""The float64 reference of the interior geometry gradient (neural_renderer/fragment_geometry.py,
csrc/d3m_fragment_geometry.h), shared by tests/test_fragment_geometry_host.py and tests/test_gpu_fragment_geometry.py.  Built
on tests/vertex_attribute_scenes.py (scenes, maps, the corner vertices of every pixel, flip and pooling) and
tests/uv_texture_image_scenes.py (wrapped corner uv, taps).

The function that is differentiated, by torch autograd, with OWNERSHIP TAKEN FROM THE MAPS (face_index_map is a constant):
internal pixel p = (xi, yi) of view b with owner fn has corners (x_c, y_c, z_c) = screen_vertices[b, vertex(fn, c)], centre
xp = (2 xi + 1 - S) / S, yp likewise, raw barycentrics b = M^-1 (xp, yp, 1)^T and u_c = (b_c / z_c) / sum_k (b_k / z_k).  The
attribute image is sum_c u_c a_c and the uv image the four taps at pos = clamp(sum_c u_c uv_c (size - 1)), both through the
flip and the 2x2 pooling of _restate / _restate_uv.  The taps are chosen from the (detached) position, their weights are
differentiable in it; the derivative of the clamp is 0 AT a limit (pos <= 0 or pos >= size - 1), as the kernel defines it.

THE DEVICE TOLERANCE (measured on the CPU, docs/EXPERIMENTS.md "Interior geometry gradient: the float32 yardstick").  The
yardstick is the error of this very expression evaluated by torch in float32 against float64 on the oracle's maps, for
fragment_weights' adjoint with the seeded grad_u of the tests, per view in units of the view's largest float64 entry:
    S1/16 1.47e-07   S1/32 1.81e-07   S2/16 2.04e-07   S2/32 4.50e-07   S3B/128 1.51e-06   S4/16 4.62e-07   S4/32 7.08e-07
(the larger of a scene's views, under torch.use_deterministic_algorithms(True): without it torch's float32 scatter-add over
the ~7500 pixels of an S3 vertex runs in thread order and the figure wanders from run to run; S3B's first view, the one eye
of S3, has 6.21e-07, its second, from behind, 1.51e-06; tests/test_fragment_geometry_host.py measures them again and holds
them to these figures).
The device gets 8 x the largest (S3B/128), 1.21e-05: the margin covers another association, FMA contraction and sums over
some hundreds of pixels per vertex in the kernel's order instead of torch's.

The uv image's reference takes the VALUE of the lookup position from the maps' u and only its derivative from the expression
(uv_images_of): the forward evaluates the maps, so its taps and fractions are those of the maps' position, and the derived
|pos_f32 - pos_f64| <= 9 2^-24 (size - 1) behind the near-integer exclusion holds for that position only (the expression's u
is up to 1.4e-05 away from the maps' on the slivers of S4)."""
import torch

from uv_texture_image_scenes import _positions, _taps, wrap_uv
import numpy as np

import vertex_attribute_scenes as _VA
from vertex_attribute_scenes import VIEWING_ANGLE, _pool, pixel_weights, scene

YARDSTICK = {"S1/16": 1.47e-07, "S1/32": 1.81e-07, "S2/16": 2.04e-07, "S2/32": 4.50e-07, "S3B/128": 1.51e-06, "S4/16": 4.62e-07,
             "S4/32": 7.08e-07}
DEVICE_TOLERANCE = 8 * max(YARDSTICK.values())      # per view, in units of the view's largest reference entry

NEAR_INTEGER = 2.0 ** -12     # uv case (b): |pos - round(pos)| below this zeroes the image gradient of the fed output pixel
MAX_ZEROED_SHARE = 0.02
UV_SEED = 24                  # seeded_faces_uv's seed: with it every case of scene_cases() stays within MAX_ZEROED_SHARE on the
                              # oracle's maps (worst 1.63 %, S1/32 pooled; the host test checks it) -- one pixel of a pooled
                              # 16^2 case is 1.6 % (S1) to 3.1 % (S2), so the cap means "no such pixel" there
UV_CASES = (("seamless", "REPEAT"), ("corners", "REPEAT"), ("corners", "MIRRORED_REPEAT"), ("corners", "CLAMP_TO_EDGE"))
UV_SIZES = ((8, 8), (32, 16))


# ---- the scene cases ------------------------------------------------------------------------------------------------------
def _s3_two_eyes():
    """S3 (two faces of more than FM_MAX_BBOX_AREA box pixels each at S = 128: the workgroup route) from two eyes, the second
    behind the quad, so that the route runs on a second view's offsets and on fill_back copies"""
    sc = dict(_VA.SCENES["S3"]())
    sc["eyes"] = np.array([[0.3, 0.2, -2.732], [-0.25, 0.15, 2.732]], np.float32)
    return sc


_VA._OTHER.setdefault("S3B", _s3_two_eyes)        # (scene(), oracle_maps() and the seeded_* helpers know it by this name)
_SIZES = (("S1", (16, 32)), ("S2", (16, 32)), ("S3B", (128,)), ("S4", (16, 32)))


def scene_cases():
    """(scene, internal size S, anti_aliasing): S1, S2 and S4 at 16 and 32, the two-eyed S3 at 128, both settings; B = 2
    everywhere.  (vertex_attribute_scenes.scene_cases() has S4 at 32 only and S3 from one eye.)"""
    return [(n, S, aa) for n, sizes in _SIZES for S in sizes for aa in (False, True)]


def screen_vertices(name):
    """[B,V,3] f32: the scene's vertices through the oracle's look_at -- what oracle_maps rasterises."""
    from oracle import nr_oracle as O
    sc = scene(name)
    B = sc["eyes"].shape[0]
    v = torch.from_numpy(sc["vertices"])[None].repeat(B, 1, 1)
    return O.look_at(v, torch.from_numpy(sc["eyes"]), _perspective_angle=VIEWING_ANGLE).float().contiguous()


def seeded_grad_weights(B, S, seed=41):
    return torch.randn(B, S, S, 3, generator=torch.Generator().manual_seed(seed + S))


def seeded_grad_images(B, C, s, seed=43):
    return torch.randn(B, C, s, s, generator=torch.Generator().manual_seed(seed + 100 * C + s))


# ---- the expression -------------------------------------------------------------------------------------------------------
def weights_of(maps, tri, sv, dtype):
    """(u [B,S,S,3] in dtype, differentiable in sv [B,V,3]; covered [B,S,S]; fn [B,S,S] clamped at 0): the expression above,
    0 where uncovered."""
    fi = maps["face_index_map"].long()
    B, S = fi.shape[:2]
    _, cov, corners = pixel_weights(maps, tri)
    bidx = torch.arange(B)[:, None, None, None].expand(B, S, S, 3)
    p = sv.to(dtype)[bidx, corners]                                   # [B,S,S,3 corners,3]
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    centre = (2 * torch.arange(S) + 1 - S).to(dtype) / S
    xp, yp = centre[None, None, :].expand(B, S, S), centre[None, :, None].expand(B, S, S)
    x0, x1, x2 = x.unbind(-1)
    y0, y1, y2 = y.unbind(-1)
    den = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
    den = torch.where(cov, den, torch.ones_like(den))
    b0 = ((y1 - y2) * (xp - x2) + (x2 - x1) * (yp - y2)) / den
    b1 = ((y2 - y0) * (xp - x2) + (x0 - x2) * (yp - y2)) / den
    b2 = (1 - b0) - b1
    t = torch.stack((b0, b1, b2), -1) / torch.where(cov[..., None], z, torch.ones_like(z))
    u = t / torch.where(cov, t.sum(-1), torch.ones_like(den))[..., None]
    return torch.where(cov[..., None], u, torch.zeros_like(u)), cov, fi.clamp(min=0)


def _finish(val, cov, anti_aliasing):
    """[B,S,S,C] internal values (0 where uncovered: the background carries no gradient) -> the output image"""
    img = torch.where(cov[..., None], val, torch.zeros_like(val)).permute(0, 3, 1, 2).flip(2)
    return _pool(img) if anti_aliasing else img


def attribute_images_of(maps, tri, sv, attributes, anti_aliasing, dtype):
    u, cov, _ = weights_of(maps, tri, sv, dtype)
    B, S = cov.shape[:2]
    corners = pixel_weights(maps, tri)[2]
    attr = attributes.to(dtype)
    bidx = torch.arange(B)[:, None, None, None].expand(B, S, S, 3)
    a = attr[corners] if attr.dim() == 2 else attr[bidx, corners]     # [B,S,S,3,C]
    val = (u[..., 0, None] * a[..., 0, :] + u[..., 1, None] * a[..., 1, :]) + u[..., 2, None] * a[..., 2, :]
    return _finish(val, cov, anti_aliasing)


def _clamp_flat(raw, hi):
    """clamp(raw, 0, hi) whose derivative is 0 AT a limit"""
    inside = (raw > 0) & (raw < hi)
    return torch.where(inside, raw, raw.detach().clamp(min=0.0).clamp(max=hi))


def uv_images_of(maps, tri, sv, faces_uv, image, anti_aliasing, wrapping, dtype, values_from_maps=True):
    """values_from_maps: the lookup position takes its VALUE from the maps' u (weight_map * depth_map / z_c in dtype: what
    the forward evaluates, so taps and fractions are the forward's up to rounding) and its DERIVATIVE from the expression
    (u_maps + (u - u.detach())); False: the expression alone, value and derivative (what finite differences see)."""
    u, cov, fn = weights_of(maps, tri, sv, dtype)
    if values_from_maps:
        u = pixel_weights(maps, tri)[0].to(dtype) + (u - u.detach())
    B, S = cov.shape[:2]
    img = image.to(dtype)
    H, W, C = img.shape[-3:]
    F = torch.as_tensor(tri).reshape(-1, 3).shape[0]
    cuv = wrap_uv(faces_uv, wrapping).to(dtype)[fn % F]               # [B,S,S,3,2]
    cuv = torch.where((fn >= F)[..., None, None], cuv.flip(-2), cuv)
    pu = (u[..., 0] * cuv[..., 0, 0] + u[..., 1] * cuv[..., 1, 0]) + u[..., 2] * cuv[..., 2, 0]
    pv = (u[..., 0] * cuv[..., 0, 1] + u[..., 1] * cuv[..., 1, 1]) + u[..., 2] * cuv[..., 2, 1]
    pos_x, pos_y = _clamp_flat(pu * (W - 1), float(W - 1)), _clamp_flat(pv * (H - 1), float(H - 1))
    pix, w = _taps(pos_x, pos_y, H, W)
    bidx = torch.arange(B)[:, None, None].expand(B, S, S)
    val = None
    for (y, x), wj in zip(pix, w):
        term = (img[y, x] if img.dim() == 3 else img[bidx, y, x]) * wj[..., None]
        val = term if val is None else val + term
    return _finish(val, cov, anti_aliasing)


# ---- the references: the gradient with respect to sv, [B,V,3] in dtype ------------------------------------------------------
def _grad(build, sv, weights, dtype):
    s = sv.detach().cpu().to(dtype).requires_grad_(True)
    out = build(s)
    g, = torch.autograd.grad((out * weights.detach().cpu().to(dtype)).sum(), s)
    return g


def weights_reference(maps, tri, sv, grad_u, dtype=torch.float64):
    return _grad(lambda s: weights_of(maps, tri, s, dtype)[0], sv, grad_u, dtype)


def attribute_reference(maps, tri, sv, attributes, grad_images, anti_aliasing, dtype=torch.float64):
    a = attributes.detach().cpu()
    return _grad(lambda s: attribute_images_of(maps, tri, s, a, anti_aliasing, dtype), sv, grad_images, dtype)


def uv_reference(maps, tri, sv, faces_uv, image, grad_images, anti_aliasing, wrapping, dtype=torch.float64,
                 values_from_maps=True):
    uv, im = faces_uv.detach().cpu(), image.detach().cpu()
    return _grad(lambda s: uv_images_of(maps, tri, s, uv, im, anti_aliasing, wrapping, dtype, values_from_maps), sv,
                 grad_images, dtype)


def adjoint_identities(maps, tri, sv, h):
    """grad [B,V,3] float64 of the closed form csrc/d3m_fragment_geometry.h evaluates (no autograd): per owned pixel, with
    e_c = h_c - hbar, A_c = (d / z_c) e_c, dL/dz_k = -(u_k / z_k) e_k, dL/dx_k = -b_k sum_c N[c][0] A_c, dL/dy_k likewise,
    scattered to the corner vertices."""
    dt = torch.float64
    fi = maps["face_index_map"].long()
    B, S = fi.shape[:2]
    _, cov, corners = pixel_weights(maps, tri)
    s = sv.detach().cpu().to(dt)
    bidx = torch.arange(B)[:, None, None, None].expand(B, S, S, 3)
    p = s[bidx, corners]
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    centre = (2 * torch.arange(S) + 1 - S).to(dt) / S
    xp, yp = centre[None, None, :].expand(B, S, S), centre[None, :, None].expand(B, S, S)
    (x0, x1, x2), (y0, y1, y2) = x.unbind(-1), y.unbind(-1)
    den = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
    den = torch.where(cov, den, torch.ones_like(den))
    nx = torch.stack((y1 - y2, y2 - y0, y0 - y1), -1) / den[..., None]
    ny = torch.stack((x2 - x1, x0 - x2, x1 - x0), -1) / den[..., None]
    b = nx * (xp - x2)[..., None] + ny * (yp - y2)[..., None]
    b = torch.stack((b[..., 0], b[..., 1], (1 - b[..., 0]) - b[..., 1]), -1)
    z = torch.where(cov[..., None], z, torch.ones_like(z))
    d = 1 / (b / z).sum(-1, keepdim=True)
    u = (b / z) * d
    hh = h.detach().cpu().to(dt)
    e = hh - (u * hh).sum(-1, keepdim=True)
    A = (d / z) * e
    px, py = (nx * A).sum(-1, keepdim=True), (ny * A).sum(-1, keepdim=True)
    g = torch.stack((-b * px, -b * py, -(u / z) * e), -1)            # [B,S,S,3 corners,3 coordinates]
    g = torch.where(cov[..., None, None], g, torch.zeros_like(g))
    out = torch.zeros(B, s.shape[1], 3, dtype=dt)
    for v in range(B):
        out[v].index_add_(0, corners[v].reshape(-1), g[v].reshape(-1, 3))
    return out


def view_errors(result, reference):
    """per view: max |result - reference| in units of the view's largest |reference| entry"""
    r, ref = result.detach().cpu().double(), reference.double()
    B = ref.shape[0]
    scale = ref.abs().reshape(B, -1).max(1).values
    return ((r - ref).abs().reshape(B, -1).max(1).values / scale).tolist()


# ---- uv case (b): the near-integer exclusion --------------------------------------------------------------------------------
def near_integer_mask(maps, tri, faces_uv, H, W, anti_aliasing, wrapping):
    """(keep [B,1,s,s] of 0 / 1 to multiply the image gradient with, the share of covered output pixels that were zeroed): an
    output pixel is zeroed when an internal pixel that feeds it has a float64 pos_x or pos_y within NEAR_INTEGER of an
    integer -- there float32 and float64 may choose different taps (|pos_f32 - pos_f64| <= 9 2^-24 (size - 1) is far less).
    An axis on which the owner's three wrapped corner coordinates COINCIDE (whole faces folded onto the image's edge by
    CLAMP_TO_EDGE: pos is the integer 0 or size - 1 all over them) excludes nothing and the pixel is compared: there h_c is
    the same for the three corners, only h_c - hbar enters the adjoint, and the other axis' slope is continuous across the
    cell boundary."""
    pos_x, pos_y, cov = _positions(maps, tri, faces_uv, H, W, wrapping, torch.float64)
    F = torch.as_tensor(tri).reshape(-1, 3).shape[0]
    cuv = wrap_uv(faces_uv, wrapping)[maps["face_index_map"].long().clamp(min=0) % F]       # [B,S,S,3,2]

    def near_axis(pos, k):
        flat = (cuv[..., 0, k] == cuv[..., 1, k]) & (cuv[..., 1, k] == cuv[..., 2, k])
        return ((pos - pos.round()).abs() < NEAR_INTEGER) & ~flat
    near = cov & (near_axis(pos_x, 0) | near_axis(pos_y, 1))
    near, cov = near.flip(1), cov.flip(1)
    if anti_aliasing:
        def any4(m):
            return m[:, 0::2, 0::2] | m[:, 0::2, 1::2] | m[:, 1::2, 0::2] | m[:, 1::2, 1::2]
        near, cov = any4(near), any4(cov)
    share = float(near.sum()) / max(float(cov.sum()), 1.0)
    return (~near)[:, None].to(torch.float32), share


def affine_image(H, W, C, batch=None):
    """an image affine in (x, y) per channel: value[k] = a_k + b_k x + c_k y, so every cell has the same slope"""
    gen = torch.Generator().manual_seed(53 + C)
    coef = torch.randn(C, 3, generator=gen, dtype=torch.float64)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    img = coef[:, 0] + coef[:, 1] * xx[..., None] / max(W - 1, 1) + coef[:, 2] * yy[..., None] / max(H - 1, 1)
    img = img.float()
    return img if batch is None else img[None].repeat(batch, 1, 1, 1).contiguous()
