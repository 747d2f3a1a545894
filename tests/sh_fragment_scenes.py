"""Inputs, the float64 restatement and the references of the per-pixel spherical-harmonic shading of fragment images
(neural_renderer/sh_fragments.py, csrc/d3m_sh_fragments.h), shared by tests/test_sh_fragments_host.py and
tests/test_gpu_sh_fragments.py.  Built on tests/vertex_attribute_scenes.py (scenes, maps, the pixels' weights and corner
vertices, flip and pooling) and tests/fragment_geometry_scenes.py (S3B, the expression of u in the screen vertices, view_errors).

THE FUNCTION (shade_images_of), element-wise torch operators on given maps, in any dtype: u_c = weight_map * (depth_map / z_c);
m = (u_0 n_0 + u_1 n_1) + u_2 n_2; r = sqrt((m_x^2 + m_y^2) + m_z^2); n = m / max(r, 1e-6); s_k = sum_j sh[b,k,j] H_j(n), j
ascending (H: nr.sh_basis); a = (u_0 c_0 + u_1 c_1) + u_2 c_2; value_k = a_k s_k (no colours: s_k); background where uncovered;
rows reversed; with anti-aliasing ((p00 + p01) + p10) + p11, times 1/4.  The gradients are torch autograd's of that expression;
with screen vertices u takes its VALUE from the maps and its DERIVATIVE from fragment_geometry_scenes.weights_of (what the
kernels do: the forward reads the maps, the shared adjoint differentiates the expression).

THE INPUTS keep the normalisation well conditioned (a condition, checked on the CPU by the host test: min r >= 0.7 over the
covered pixels of every case):
  cone     n_v = normalize(a + 0.4 xi_v), a = normalize((0.3, 0.2, 1)), xi_v seeded uniform in [-1, 1]^3: |0.4 xi| <= 0.693,
           every n_v within 44 degrees of a, so every convex mix has r >= 0.72.  Every scene.
  smooth   the scene's own smooth normals, area-weighted in float64 as nr.vertex_normals states them: S1, S2, S3B only (min r
           over the faces' whole simplex 0.934 / 0.996 / 0.9997); on S4 three vertices have a zero normal and r reaches 0.

THE DEVICE TOLERANCE (measured on the CPU, docs/EXPERIMENTS.md "Per-pixel SH shading: the float32 yardstick").  The yardstick
is the error of this very expression evaluated by torch in float32 against float64 on the oracle's maps, under
torch.use_deterministic_algorithms(True), with per-view inputs ([B,V,3] normals and colours, [B,3,9] light) so that every
result has a view dimension; per view in units of the view's largest float64 entry; the larger of a case's views, the larger
of its normal kinds.  YARDSTICK holds the figures per case and kind; tests/test_sh_fragments_host.py measures them again and
holds them to these figures.  The device gets 8 x the largest of a kind (the light's: the figure at S3B/128, up to 16 384 terms
per view): the family's margin for another association, FMA contraction and the kernels' own summation order."""
import torch

import fragment_geometry_scenes as FG
import vertex_attribute_scenes as VA
from vertex_attribute_scenes import _pool, cube_route_colors, scene

KINDS = ("image", "normals", "sh", "colors", "screen_vertices")
# (scene, internal size S, anti_aliasing)
CASES = ([(n, S, aa) for n in ("S1", "S2") for S in (16, 32) for aa in (False, True)] + [("S3B", 128, False)] +
         [("S4", S, False) for S in (16, 32)])
NORMAL_KINDS = {"S1": ("cone", "smooth"), "S2": ("cone", "smooth"), "S3B": ("cone", "smooth"), "S4": ("cone",)}
MIN_R = 0.7

# per case "scene/S" (the larger of aa False / True where both run): the float32 yardstick of each kind
YARDSTICK = {
    "S1/16": dict(image=2.36e-07, normals=2.34e-07, sh=1.85e-07, colors=1.96e-07, screen_vertices=3.61e-07),
    "S1/32": dict(image=2.20e-07, normals=5.11e-07, sh=2.11e-07, colors=2.94e-07, screen_vertices=6.03e-07),
    "S2/16": dict(image=1.98e-07, normals=1.81e-07, sh=2.54e-07, colors=2.28e-07, screen_vertices=3.67e-07),
    "S2/32": dict(image=2.31e-07, normals=2.72e-07, sh=1.49e-07, colors=3.63e-07, screen_vertices=4.14e-07),
    "S3B/128": dict(image=3.58e-07, normals=1.76e-06, sh=4.68e-07, colors=2.44e-06, screen_vertices=3.14e-06),
    "S4/16": dict(image=1.88e-07, normals=3.37e-07, sh=2.02e-07, colors=2.12e-07, screen_vertices=8.01e-07),
    "S4/32": dict(image=2.11e-07, normals=2.02e-07, sh=1.47e-07, colors=2.06e-07, screen_vertices=8.84e-07),
}
DEVICE_TOLERANCE = {k: 8 * max(y[k] for y in YARDSTICK.values()) for k in KINDS if k != "sh"}
DEVICE_TOLERANCE["sh"] = 8 * YARDSTICK["S3B/128"]["sh"]


# ---- the inputs -----------------------------------------------------------------------------------------------------------
def _sizes(name):
    sc = scene(name)
    return sc["eyes"].shape[0], sc["vertices"].shape[0]


def cone_normals(name, batched, seed=61):
    B, V = _sizes(name)
    a = torch.tensor([0.3, 0.2, 1.0], dtype=torch.float64)
    a = a / a.norm()
    xi = torch.rand((B, V, 3) if batched else (V, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 2 - 1
    n = a + 0.4 * xi
    return (n / n.norm(dim=-1, keepdim=True)).float()


def smooth_normals(name, batched):
    """area-weighted in float64: the normalised sum of (x1 - x0) x (x2 - x0) over the vertex's faces"""
    sc = scene(name)
    v, tri = torch.from_numpy(sc["vertices"]).double(), torch.from_numpy(sc["tri"]).long()
    nf = torch.cross(v[tri[:, 1]] - v[tri[:, 0]], v[tri[:, 2]] - v[tri[:, 0]], dim=-1)
    s = torch.zeros_like(v)
    for c in range(3):
        s.index_add_(0, tri[:, c], nf)
    n = (s / s.norm(dim=-1, keepdim=True).clamp(min=1e-6)).float()
    return n[None].repeat(_sizes(name)[0], 1, 1).contiguous() if batched else n


def normals_of(name, kind, batched):
    return cone_normals(name, batched) if kind == "cone" else smooth_normals(name, batched)


def seeded_sh(B=None, seed=67):
    """every term non-zero: magnitude in [0.2, 0.8), seeded sign; term 0 positive (a lit picture)"""
    gen = torch.Generator().manual_seed(seed)
    shape = (3, 9) if B is None else (B, 3, 9)
    sh = (0.2 + 0.6 * torch.rand(shape, generator=gen)) * (torch.randint(0, 2, shape, generator=gen) * 2 - 1).float()
    sh[..., 0] = sh[..., 0].abs() + 1.0
    return sh


def white_ambient():
    from deep3dmap_amd.neural_renderer.smooth_shading import SH_A
    sh = torch.zeros(3, 9)
    sh[:, 0] = 1.0 / SH_A[0]
    return sh


def seeded_colors(name, batched, seed=3):
    B, V = _sizes(name)
    return torch.stack([cube_route_colors(V, seed + 10 * b) for b in range(B)]) if batched else cube_route_colors(V, seed)


def seeded_grad_out(B, s):
    return FG.seeded_grad_images(B, 3, s)


def input_configs():
    """(normals batched, sh batched, colours: None / 'shared' / 'batched'): the full product"""
    return [(nb, sb, col) for nb in (False, True) for sb in (False, True) for col in (None, "shared", "batched")]


# ---- the restatement ------------------------------------------------------------------------------------------------------
def shade_images_of(maps, tri, normals, sh, colors, background, anti_aliasing, dtype, screen_vertices=None,
                    values_from_maps=True):
    """(images [B,3,s,s] in dtype, r [B,S,S] of the covered pixels (1 elsewhere), covered [B,S,S]).  values_from_maps=False:
    u is the expression's in the screen vertices alone, value and derivative (what finite differences see)."""
    from deep3dmap_amd import neural_renderer as nr
    V = normals.shape[-2]
    u, cov, corners = VA._restate(maps, tri, torch.zeros(V, 1, dtype=dtype), None, False, dtype, False)[2:]
    if screen_vertices is not None:
        ue = FG.weights_of(maps, tri, screen_vertices, dtype)[0]
        u = u + (ue - ue.detach()) if values_from_maps else ue
    B, S = cov.shape[:2]
    bidx = torch.arange(B)[:, None, None, None].expand(B, S, S, 3)

    def mix(x):
        x = x.to(dtype)
        xc = x[corners] if x.dim() == 2 else x[bidx, corners]         # [B,S,S,3 corners,3]
        return (u[..., 0, None] * xc[..., 0, :] + u[..., 1, None] * xc[..., 1, :]) + u[..., 2, None] * xc[..., 2, :]

    m = mix(normals)
    m = torch.where(cov[..., None], m, torch.tensor([0.0, 0.0, 1.0], dtype=dtype).expand_as(m))
    r = torch.sqrt((m[..., 0] * m[..., 0] + m[..., 1] * m[..., 1]) + m[..., 2] * m[..., 2])
    n = m / r.clamp(min=1e-6)[..., None]
    H = nr.sh_basis(n)                                                # [B,S,S,9]
    shb = sh.to(dtype)
    shb = shb[None].expand(B, 3, 9) if shb.dim() == 2 else shb
    val = None
    for j in range(9):
        term = shb[:, None, None, :, j] * H[..., None, j]
        val = term if val is None else val + term                     # [B,S,S,3]
    if colors is not None:
        val = mix(colors) * val
    bg = torch.zeros(3, dtype=dtype) if background is None else torch.as_tensor(background, dtype=dtype).expand(3)
    val = torch.where(cov[..., None], val, bg.expand_as(val))
    img = val.permute(0, 3, 1, 2).flip(2)
    return (_pool(img) if anti_aliasing else img), r, cov


def reference(maps, tri, normals, sh, colors, screen_vertices, grad_out, anti_aliasing, background=None, dtype=torch.float64):
    """dict(image, normals, sh, colors (None without colours), screen_vertices) in dtype: the restatement and its autograd
    gradients for the image gradient grad_out"""
    leaf = lambda t: None if t is None else t.detach().cpu().to(dtype).requires_grad_(True)
    n, s, c, sv = leaf(normals), leaf(sh), leaf(colors), leaf(screen_vertices)
    img = shade_images_of(maps, tri, n, s, c, background, anti_aliasing, dtype, sv)[0]
    wanted = [t for t in (n, s, c, sv) if t is not None]
    grads = list(torch.autograd.grad((img * grad_out.detach().cpu().to(dtype)).sum(), wanted))
    out = dict(image=img.detach())
    for key, t in (("normals", n), ("sh", s), ("colors", c), ("screen_vertices", sv)):
        out[key] = grads.pop(0) if t is not None else None
    return out


def errors_of(result, ref):
    """per view (a tensor without a view dimension: as one view) max |result - ref| in units of the largest |ref| entry"""
    r, ref = result.detach().cpu().double(), ref.double()
    if ref.dim() < 3:                                                 # a shared [V,3] or [3,9]
        r, ref = r[None], ref[None]
    return FG.view_errors(r, ref)


def measure_yardstick(name, S):
    """{kind: the float32 yardstick of case name/S}: the larger of the views, of the normal kinds and of the anti-aliasing
    settings the case runs with (call under torch.use_deterministic_algorithms(True))"""
    maps, tri, sv = VA.oracle_maps(name, S), scene(name)["tri"], FG.screen_vertices(name)
    B = sv.shape[0]
    worst = dict.fromkeys(KINDS, 0.0)
    for aa in sorted({aa for n, s, aa in CASES if (n, s) == (name, S)}):
        g = seeded_grad_out(B, S // 2 if aa else S)
        for kind in NORMAL_KINDS[name]:
            args = (maps, tri, normals_of(name, kind, True), seeded_sh(B), seeded_colors(name, True), sv, g, aa)
            r64, r32 = reference(*args), reference(*args, dtype=torch.float32)
            for k in KINDS:
                worst[k] = max(worst[k], max(errors_of(r32[k], r64[k])))
    return worst
