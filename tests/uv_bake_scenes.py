"""Scenes, layouts, the float64 restatement and the references of view images baked into a uv texture
(neural_renderer/uv_bake.py, csrc/d3m_uv_bake.h), shared by tests/test_uv_bake_host.py and tests/test_gpu_uv_bake.py.  Built on
tests/vertex_attribute_scenes.py (scenes, the oracle's maps) and tests/fragment_geometry_scenes.py (S3B, view_errors).

THE FUNCTION (bake_of), element-wise torch operators on given maps of the layout record and of the view record, in any dtype.
Texel p of the layout with owner f, triangle t = f mod F, b_c = the layout's weight_map (z is 1 there), view b:
  corners (x_c, y_c, z_c) = screen_vertices[b, tri[t][c]] (an owner f >= F: tri[t][2 - c]);
  perspective:  t_c = b_c z_c, Z = (t_0 + t_1) + t_2, x = ((t_0 x_0 + t_1 x_1) + t_2 x_2) / Z, y likewise;
  orthographic: x = (b_0 x_0 + b_1 x_1) + b_2 x_2, y likewise, Z as above;
  gx = (x S + S) / 2, gy likewise; visible iff 0 <= gx, gy < S, the internal pixel (floor gx, floor gy) of the view record is
  covered and (its owner mod F == t or Z <= depth + depth_tolerance);
  col = clamp((x W + W - 1) / 2, 0, W - 1), row = clamp((H - 1) - (y H + H - 1) / 2, 0, H - 1), both with derivative 0 at a limit;
  xi = floor col, fx = col - xi, x1 = min(xi + 1, W - 1), rows likewise; value = ((t00 w00 + t01 w01) + t10 w10) + t11 w11 with
  t00 = (yi, xi), t01 = (yi, x1), t10 = (y1, xi), t11 = (y1, x1) and weights (1 - fx)(1 - fy), fx (1 - fy), (1 - fx) fy, fx fy;
  texture = value where visible, else the background; mask = visible.
The DECISIONS -- visible, (xi, yi) and whether col / row sit strictly inside their clamp -- are constants of the graph.
bake_of returns them with their distances from the thresholds, and takes them back (`decisions=`) in the place of its own:
that is how finite differences, a float32 evaluation and the device's own visibility are compared with the float64 one.

NEAR A THRESHOLD (the GPU test's rule).  A texel-view whose gx or gy lies within M_POS of an integer, or whose Z - depth -
depth_tolerance lies within M_Z of 0 while its pixel is covered by ANOTHER triangle, may be decided either way in float32: the
device's mask is accepted there and the reference is evaluated with it.  A texel-view whose col or row lies within M_POS of an
integer may take the neighbouring cell's taps: value and weights are continuous, so texture and the images' gradient are
compared as they are, and the output gradient is zeroed at such a texel-view (in the device run and in the reference alike) so
that the vertices' gradient, which reads the cell's slope, stays comparable -- the rule of fragment_geometry_scenes'
near_integer_mask.  M = 8 x the float32 yardstick of the decision quantities; at most MAX_NEAR_SHARE of the covered texel-views
of a case may be near a threshold (the host test checks it on the oracle's maps, the GPU test on the device's).

THE DEVICE TOLERANCE.  The yardstick of a kind is the error of this very expression evaluated by torch in float32 against
float64 on the oracle's maps with the float64 decisions, per view in units of the view's largest float64 entry
(fragment_geometry_scenes.view_errors), the larger of a case's views; the device gets 8 x the largest of a kind over the cases:
the family's margin for another association and the kernels' own summation order.  tests/test_uv_bake_host.py measures the
figures again and holds them to YARDSTICK."""
import numpy as np
import torch

import fragment_geometry_scenes as FG      # (registers S3B)
from vertex_attribute_scenes import VIEWING_ANGLE, scene

KINDS = ("texture", "images", "screen_vertices")
DEPTH_TOLERANCE = 1e-2
MAX_NEAR_SHARE = 0.01

# (scene, layout, T, view raster size S, anti_aliasing of the view record, H, W, C, perspective); B is the scene's eyes
CASES = (
    ("S1", "planar", 20, 16, False, 24, 40, 3, True),       # B = 2; front and back overlap in uv: owners hidden in the view
    ("S1", "atlas", 20, 32, True, 24, 40, 9, True),         # seams, both windings, an anti-aliased view record, two chunks
    ("S1", "atlas", 20, 16, False, 24, 40, 3, False),       # orthographic
    ("S3B", "planar", 128, 32, False, 24, 40, 3, True),     # a uv triangle's box beyond 4096 texels: the workgroup route
    ("S4", "atlas", 100, 32, False, 24, 40, 1, True),       # hub vertices: the long-row chunks; one channel (2500 triangles,
                                                            # two texels a cell: the smallest T at which dozens are visible)
    ("S3", "planar", 20, 16, False, 24, 40, 3, False),      # B = 1
)


def case_id(case):
    name, layout, T, S, aa, H, W, C, persp = case
    return "%s-%s-T%d-S%d%s-%dx%d-C%d-%s" % (name, layout, T, S, "aa" if aa else "", H, W, C, "persp" if persp else "ortho")


# per case: the float32 yardstick of each kind, and of the decision quantities (gx, gy in pixels; Z - depth - tolerance)
YARDSTICK = {
    'S1-planar-T20-S16-24x40-C3-persp': dict(texture=1.98e-06, images=2.38e-06, screen_vertices=1.47e-06, position=1.20e-06, depth=5.98e-06),
    'S1-atlas-T20-S32aa-24x40-C9-persp': dict(texture=2.68e-06, images=1.61e-06, screen_vertices=1.30e-06, position=2.27e-06, depth=5.55e-06),
    'S1-atlas-T20-S16-24x40-C3-ortho': dict(texture=2.05e-06, images=1.41e-06, screen_vertices=2.61e-06, position=8.01e-07, depth=5.55e-06),
    'S3B-planar-T128-S32-24x40-C3-persp': dict(texture=4.92e-06, images=2.95e-06, screen_vertices=4.46e-06, position=3.49e-06, depth=6.16e-06),
    'S4-atlas-T100-S32-24x40-C1-persp': dict(texture=1.63e-06, images=2.13e-06, screen_vertices=1.59e-06, position=2.69e-06, depth=5.11e-06),
    'S3-planar-T20-S16-24x40-C3-ortho': dict(texture=2.44e-06, images=1.75e-06, screen_vertices=2.73e-06, position=1.55e-06, depth=3.23e-07),
}
DEVICE_TOLERANCE = {k: 8 * max(y[k] for y in YARDSTICK.values()) for k in KINDS}
M_POS = 8 * max(y["position"] for y in YARDSTICK.values())       # pixels (of the view record, and of the image's cells)
M_Z = 8 * max(y["depth"] for y in YARDSTICK.values())            # depth units


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def screen_vertices(name, perspective):
    """[B,V,3] f32: the scene's vertices through the oracle's look_at, with or without its perspective division"""
    from oracle import nr_oracle as O
    sc = scene(name)
    B = sc["eyes"].shape[0]
    v = torch.from_numpy(sc["vertices"])[None].repeat(B, 1, 1)
    return O.look_at(v, torch.from_numpy(sc["eyes"]), _perspective_angle=VIEWING_ANGLE if perspective else None).float().contiguous()


def planar_layout(name):
    """faces_uv [F,3,2] f32: the object-space x, y of every vertex, scaled into [0.06, 0.94] -- one uv per vertex, no seams; on
    a closed mesh the front and the back overlap in uv"""
    sc = scene(name)
    xy = torch.from_numpy(sc["vertices"])[:, :2].double()
    lo, hi = xy.min(0).values, xy.max(0).values
    uv = (0.06 + 0.88 * (xy - lo) / (hi - lo)).float()
    return uv[torch.from_numpy(sc["tri"]).long()].contiguous()


def atlas_layout(name, seed=71):
    """faces_uv [F,3,2] f32: a per-triangle atlas -- triangle f alone in cell f of an n x n grid, a seeded triangle inside the
    cell, odd triangles with their corners in the opposite winding: seams everywhere, both windings"""
    F = scene(name)["tri"].shape[0]
    n = int(np.ceil(np.sqrt(F)))
    gen = torch.Generator().manual_seed(seed)
    base = torch.tensor([[0.08, 0.08], [0.92, 0.12], [0.3, 0.9]], dtype=torch.float64)
    local = (base[None] + 0.06 * (torch.rand(F, 3, 2, generator=gen, dtype=torch.float64) - 0.5))
    local[1::2] = local[1::2].flip(1)
    cell = torch.stack((torch.arange(F) % n, torch.arange(F) // n), -1).double()
    return ((cell[:, None, :] + local) / n).float().contiguous()


def layout_of(name, layout):
    return planar_layout(name) if layout == "planar" else atlas_layout(name)


def seeded_images(B, C, H, W, seed=83):
    return torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(seed + 100 * C + H))


def seeded_grad_texture(B, T, C, seed=89):
    return torch.randn(B, T, T, C, generator=torch.Generator().manual_seed(seed + 100 * C + T))


def seeded_background(C):
    return torch.linspace(0.25, 1.5, C)


# ---- the oracle's maps ------------------------------------------------------------------------------------------------------
_map_cache = {}


def _oracle_record(sv, tri, S):
    from oracle import nr_oracle as O
    B = sv.shape[0]
    faces = O.vertices_to_faces(sv, torch.as_tensor(tri).long()[None].repeat(B, 1, 1))
    faces = torch.cat((faces, faces.flip(-2)), 1)
    m = O.raster_forward(faces.numpy(), None, S, 0.1, 100, 1e-3, None, False, True, False)
    return {k: torch.from_numpy(np.ascontiguousarray(m[k])) for k in ("face_index_map", "weight_map", "depth_map", "faces")}


def oracle_layout_maps(name, layout, T):
    """the layout record's maps from the CPU oracle: uv_layout_vertices rasterised with fill_back at size T"""
    from deep3dmap_amd.neural_renderer import uv_bake
    key = ("layout", name, layout, T)
    if key not in _map_cache:
        v, tri = uv_bake.uv_layout_vertices(layout_of(name, layout), T)
        _map_cache[key] = _oracle_record(v, tri, T)
    return _map_cache[key]


def oracle_view_maps(name, S, perspective):
    key = ("view", name, S, perspective)
    if key not in _map_cache:
        _map_cache[key] = _oracle_record(screen_vertices(name, perspective), scene(name)["tri"], S)
    return _map_cache[key]


def record_maps(fr):
    """the same dict from a device Fragments record"""
    return dict(face_index_map=fr.face_index_map.cpu(), weight_map=fr.weight_map.cpu(), depth_map=fr.depth_map.cpu(),
                faces=fr.faces.cpu())


# ---- the restatement ------------------------------------------------------------------------------------------------------
def bake_of(uv_maps, view_maps, tri, sv, images, perspective, depth_tolerance, background, dtype, decisions=None):
    """(texture [B,T,T,C], mask [B,T,T] bool, info) in dtype, differentiable in sv [B,V,3] and images [B,C,H,W].  info:
    visible, xi, yi, inner_x, inner_y (the decisions that were used), covered [B,T,T] (the texel has an owner), gx, gy,
    zq = Z - depth - depth_tolerance (dtype, detached), other [B,T,T] (the point's pixel is covered by ANOTHER triangle: where
    zq decides), d_pixel, d_depth, d_cell [B,T,T] float64: the distance of gx, gy from the nearest integer, |zq| where it
    decides (inf elsewhere), the distance of col, row from the nearest integer (beyond the clamp: from the limit), where the point is inside the view.  decisions: a dict with any of visible, xi,
    yi, inner_x, inner_y to use in the place of this evaluation's own."""
    decisions = decisions or {}
    fi = uv_maps["face_index_map"].long()[0]
    T = fi.shape[0]
    tri = torch.as_tensor(tri).long().reshape(-1, 3)
    F = tri.shape[0]
    cov = fi >= 0
    fn = fi.clamp(min=0)
    t = fn % F
    corners = torch.where((fn >= F)[..., None], tri[t].flip(-1), tri[t])           # [T,T,3]
    bw = uv_maps["weight_map"][0].to(dtype)                                       # [T,T,3]
    bw = torch.where(cov[..., None], bw, torch.full_like(bw, 1.0 / 3))            # (an uncovered texel: no 0 / 0 in the graph)
    img = images.to(dtype)
    B, C, H, W = img.shape
    p = sv.to(dtype)[:, corners]                                                  # [B,T,T,3 corners,3]
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    tc = bw[None] * z
    Z = (tc[..., 0] + tc[..., 1]) + tc[..., 2]
    if perspective:
        px = ((tc[..., 0] * x[..., 0] + tc[..., 1] * x[..., 1]) + tc[..., 2] * x[..., 2]) / Z
        py = ((tc[..., 0] * y[..., 0] + tc[..., 1] * y[..., 1]) + tc[..., 2] * y[..., 2]) / Z
    else:
        px = (bw[None, ..., 0] * x[..., 0] + bw[None, ..., 1] * x[..., 1]) + bw[None, ..., 2] * x[..., 2]
        py = (bw[None, ..., 0] * y[..., 0] + bw[None, ..., 1] * y[..., 1]) + bw[None, ..., 2] * y[..., 2]
    # visibility
    vfi = view_maps["face_index_map"].long()
    S = vfi.shape[1]
    gx, gy = ((px * S + S) * 0.5).detach(), ((py * S + S) * 0.5).detach()
    inside = (gx >= 0) & (gx < S) & (gy >= 0) & (gy < S)
    ix, iy = gx.floor().long().clamp(0, S - 1), gy.floor().long().clamp(0, S - 1)
    bidx = torch.arange(B)[:, None, None].expand(B, T, T)
    o = vfi[bidx, iy, ix]
    depth = view_maps["depth_map"].to(dtype)[bidx, iy, ix]
    zq = Z.detach() - depth - depth_tolerance
    same = (o % F) == t[None]
    covb = cov[None].expand(B, T, T)
    other = covb & inside & (o >= 0) & ~same
    visible = covb & inside & (o >= 0) & (same | (zq <= 0))
    visible = decisions.get("visible", visible)
    # lookup
    raw_c, raw_r = (px * W + (W - 1)) * 0.5, (H - 1) - (py * H + (H - 1)) * 0.5
    inner_x = decisions.get("inner_x", ((raw_c > 0) & (raw_c < W - 1)).detach())
    inner_y = decisions.get("inner_y", ((raw_r > 0) & (raw_r < H - 1)).detach())
    col = torch.where(inner_x, raw_c, raw_c.detach().clamp(min=0.0).clamp(max=float(W - 1)))
    row = torch.where(inner_y, raw_r, raw_r.detach().clamp(min=0.0).clamp(max=float(H - 1)))
    col, row = torch.nan_to_num(col, nan=0.0), torch.nan_to_num(row, nan=0.0)
    xi = decisions.get("xi", col.detach().floor().long().clamp(0, W - 1))
    yi = decisions.get("yi", row.detach().floor().long().clamp(0, H - 1))
    fx, fy = col - xi.to(dtype), row - yi.to(dtype)
    x1, y1 = (xi + 1).clamp(max=W - 1), (yi + 1).clamp(max=H - 1)
    b4 = bidx

    def tap(yy, xx):
        return img[b4, :, yy, xx]                                                 # [B,T,T,C]
    w00, w01, w10, w11 = (1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy
    val = ((tap(yi, xi) * w00[..., None] + tap(yi, x1) * w01[..., None]) + tap(y1, xi) * w10[..., None]) + \
        tap(y1, x1) * w11[..., None]
    bg = torch.zeros(C, dtype=dtype) if background is None else torch.as_tensor(background, dtype=dtype).expand(C)
    texture = torch.where(visible[..., None], val, bg.expand_as(val))

    def to_integer(v):
        v = v.double()
        return (v - v.round()).abs()

    def to_decision(raw, inner, hi):
        """inside the clamp: the distance from the nearest integer (another cell); outside: from the limit it passed"""
        raw = torch.nan_to_num(raw.double(), nan=0.0)
        return torch.where(inner, (raw - raw.round()).abs(), torch.minimum(raw.abs(), (raw - hi).abs()))
    inf = torch.full((B, T, T), float("inf"), dtype=torch.float64)
    info = dict(visible=visible, xi=xi, yi=yi, inner_x=inner_x, inner_y=inner_y, covered=covb, gx=gx, gy=gy, zq=zq, other=other,
                d_pixel=torch.where(covb, torch.minimum(to_integer(gx), to_integer(gy)), inf),
                d_depth=torch.where(other, zq.double().abs(), inf),
                d_cell=torch.where(covb & inside, torch.minimum(to_decision(raw_c.detach(), inner_x, W - 1),
                                                                to_decision(raw_r.detach(), inner_y, H - 1)), inf))
    return texture, visible, info


def decisions_of(info):
    return {k: info[k] for k in ("visible", "xi", "yi", "inner_x", "inner_y")}


def near_threshold(info, m_pos, m_z):
    """(near_visibility, near_cell) [B,T,T] bool of covered texel-views: the visibility decision / the choice of taps may go
    either way in float32"""
    return (info["d_pixel"] <= m_pos) | (info["d_depth"] <= m_z), info["covered"] & (info["d_cell"] <= m_pos)


def reference(uv_maps, view_maps, tri, sv, images, grad_texture, perspective, depth_tolerance=DEPTH_TOLERANCE, background=None,
              dtype=torch.float64, decisions=None):
    """dict(texture, mask, images, screen_vertices, info) in dtype: the restatement and its autograd gradients for the output
    gradient grad_texture [B,T,T,C]"""
    s = sv.detach().cpu().to(dtype).requires_grad_(True)
    im = images.detach().cpu().to(dtype).requires_grad_(True)
    texture, mask, info = bake_of(uv_maps, view_maps, tri, s, im, perspective, depth_tolerance, background, dtype, decisions)
    loss = (texture * grad_texture.detach().cpu().to(dtype)).sum()
    g_im, g_sv = torch.autograd.grad(loss, [im, s], allow_unused=True)
    zero = lambda g, like: torch.zeros_like(like) if g is None else g
    return dict(texture=texture.detach(), mask=mask, images=zero(g_im, im), screen_vertices=zero(g_sv, s), info=info)


def case_inputs(case):
    """dict(tri, faces_uv, sv, images, grad_texture, background) of a case"""
    name, layout, T, S, aa, H, W, C, persp = case
    sv = screen_vertices(name, persp)
    B = sv.shape[0]
    return dict(tri=scene(name)["tri"], faces_uv=layout_of(name, layout), sv=sv, images=seeded_images(B, C, H, W),
                grad_texture=seeded_grad_texture(B, T, C), background=seeded_background(C))


def case_oracle_maps(case):
    name, layout, T, S, aa, H, W, C, persp = case
    return oracle_layout_maps(name, layout, T), oracle_view_maps(name, S, persp)


def measure_yardstick(case):
    """{kind: the float32 yardstick, position, depth: the largest float32 error of gx, gy / of Z - depth - tolerance over the
    covered texel-views} of a case on the oracle's maps, the float32 evaluation with the float64 decisions"""
    uv_maps, view_maps = case_oracle_maps(case)
    a = case_inputs(case)
    args = (uv_maps, view_maps, a["tri"], a["sv"], a["images"], a["grad_texture"], case[8])
    r64 = reference(*args)
    r32 = reference(*args, dtype=torch.float32, decisions=decisions_of(r64["info"]))
    out = {k: max(FG.view_errors(r32[k], r64[k])) for k in KINDS}
    cov = r64["info"]["covered"] & torch.isfinite(r64["info"]["gx"])
    i64, i32 = r64["info"], r32["info"]
    out["position"] = float(torch.maximum((i32["gx"].double() - i64["gx"]).abs(), (i32["gy"].double() - i64["gy"]).abs())[cov].max())
    out["depth"] = float((i32["zq"].double() - i64["zq"]).abs()[cov].max())
    return out


def near_share(info, m_pos, m_z):
    near_v, near_c = near_threshold(info, m_pos, m_z)
    return float((near_v | near_c).sum()) / max(float(info["covered"].sum()), 1.0)
