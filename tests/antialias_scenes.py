"""The float64 restatement of the analytic edge antialiasing (neural_renderer/antialias.py, csrc/d3m_antialias.h), shared by
tests/test_antialias_host.py and tests/test_gpu_antialias.py.  Built on tests/vertex_attribute_scenes.py and
tests/fragment_geometry_scenes.py (scenes, maps, screen vertices, view_errors).

`antialias_of` evaluates the function of csrc/d3m_antialias.h with element-wise torch operators on given maps: owners and
depths are taken FROM THE MAPS, every choice (near pixel, qualifying sides, exit edge, silhouette test, recipient) is made on
detached values, and t = E(P_n) / (E(P_n) - E(P_o)) -- the plain subtraction, not the kernel's closed form -- is differentiable
in the screen vertices through autograd.  `side_opposite_of` restates the side table with a dictionary.

THE FRAGILE-PAIR RULE (tau = 2^-10).  A pair of neighbours with different triangles is fragile when
  - it has an exit edge and |t - 1/2| < tau, or two qualifying sides have t within tau of each other;
  - for any side of the near triangle |E(P_n)| or |E(P_o)| < tau (|X_c - X_a| + |Y_c - Y_a|) 2 / S;
  - the exit edge has an opposite vertex O and |E(O)| < tau (|X_c - X_a| + |Y_c - Y_a|)(|O_x - X_a| + |O_y - Y_a|);
  - both pixels are covered and their depths differ by less than tau times the larger.
Both pixels of a fragile pair are left out of the forward comparison and get a zero seeded grad_out; at most MAX_LEFT_OUT of
a case's pixels may be left out.  LEFT_OUT records the shares on the oracle's maps and YARDSTICK the float32 yardstick --
this very expression evaluated by torch in float32 against float64 on the oracle's maps: forward the largest absolute
difference at compared pixels for image values in [0, 1); gradient per view in units of the view's largest float64 entry,
the larger of the image's and the vertices' gradient --; tests/test_antialias_host.py measures both again and holds them to
these figures.  The device gets 8 x the largest of each: another association, the closed-form denominator and sums over a
face's pixels in the kernel's order instead of torch's."""
import torch

import fragment_geometry_scenes as FG
from vertex_attribute_scenes import scene

TAU = 2.0 ** -10
MAX_LEFT_OUT = 0.08
CASES = [(n, S) for n, S, aa in FG.scene_cases() if not aa]          # S1, S2, S4 at 16 and 32, S3B at 128

# measured by tests/test_antialias_host.py (it prints them) on the oracle's maps
LEFT_OUT = {"S1/16": 0.0625, "S1/32": 0.0352, "S2/16": 0.0, "S2/32": 0.0039, "S3B/128": 0.0148, "S4/16": 0.0312, "S4/32": 0.0332}
YARDSTICK = {"forward": {"S1/16": 8.85e-08, "S1/32": 2.06e-07, "S2/16": 6.68e-08, "S2/32": 7.22e-08, "S3B/128": 6.20e-06,
                         "S4/16": 4.16e-07, "S4/32": 3.30e-06},
             "gradient": {"S1/16": 1.11e-07, "S1/32": 1.50e-07, "S2/16": 3.03e-07, "S2/32": 1.17e-07, "S3B/128": 6.75e-06,
                          "S4/16": 2.63e-07, "S4/32": 2.22e-06}}
FORWARD_TOLERANCE = 8 * max(YARDSTICK["forward"].values(), default=0.0)      # absolute, image values in [0, 1)
GRADIENT_TOLERANCE = 8 * max(YARDSTICK["gradient"].values(), default=0.0)    # per view, of the view's largest reference entry


def key(name, S):
    return "%s/%d" % (name, S)


def seeded_images(B, C, S, seed=61):
    """[B,C,S,S] in [0, 1)"""
    return torch.rand(B, C, S, S, generator=torch.Generator().manual_seed(seed + 100 * C + S))


def seeded_grad_out(B, C, S, seed=67):
    return torch.randn(B, C, S, S, generator=torch.Generator().manual_seed(seed + 100 * C + S))


def side_opposite_of(tri):
    """[F,3] int64, by a dictionary over the undirected edges of the proper triangles"""
    tri = torch.as_tensor(tri).reshape(-1, 3).tolist()
    users = {}
    for f, t in enumerate(tri):
        if len(set(t)) == 3:
            for j in range(3):
                users.setdefault(frozenset((t[j], t[(j + 1) % 3])), []).append((f, j))
    out = [[-2] * 3 for _ in tri]
    for sides in users.values():
        if len(sides) == 1:
            f, j = sides[0]
            out[f][j] = -1
        elif len(sides) == 2:
            (f, j), (g, i) = sides
            out[f][j], out[g][i] = tri[g][(i + 2) % 3], tri[f][(j + 2) % 3]
    return torch.tensor(out, dtype=torch.int64)


def _pairs(maps, tri, side, sv, c, axis, dtype):
    """The pairs p, q = p + one step along `axis` (0: x, 1: y) in the maps' orientation: (delta_p, delta_q [B,C,h,w] -- what
    the pair adds to its two pixels --, fragile [B,h,w])."""
    fi, depth = maps["face_index_map"].long(), maps["depth_map"].to(dtype)
    B, S = fi.shape[:2]
    tri = torch.as_tensor(tri).long().reshape(-1, 3)
    F = tri.shape[0]
    cut = (lambda a, lo: a[..., :, lo:S - 1 + lo]) if axis == 0 else (lambda a, lo: a[..., lo:S - 1 + lo, :])
    fp, fq, dp, dq, cp, cq = cut(fi, 0), cut(fi, 1), cut(depth, 0), cut(depth, 1), cut(c, 0), cut(c, 1)
    centre = (2 * torch.arange(S) + 1 - S).to(dtype) / S
    gx, gy = centre[None, None, :].expand(B, S, S), centre[None, :, None].expand(B, S, S)
    pxp, pxq, pyp, pyq = cut(gx, 0), cut(gx, 1), cut(gy, 0), cut(gy, 1)
    tid = lambda f: torch.where(f >= 0, f % F, torch.full_like(f, -1))
    differ = tid(fp) != tid(fq)
    inf = torch.full_like(dp, float("inf"))
    dp, dq = torch.where(fp >= 0, dp, inf), torch.where(fq >= 0, dq, inf)
    p_near = dp <= dq
    fn = torch.where(p_near, fp, fq).clamp(min=0)
    pnx, pny = torch.where(p_near, pxp, pxq), torch.where(p_near, pyp, pyq)
    pox, poy = torch.where(p_near, pxq, pxp), torch.where(p_near, pyq, pyp)
    back = fn >= F
    corners = tri[fn % F]
    corners = torch.where(back[..., None], corners.flip(-1), corners)               # [B,h,w,3]
    bidx = torch.arange(B)[:, None, None].expand(fn.shape)
    P = sv.to(dtype)[bidx[..., None], corners]                                      # [B,h,w,3 corners,3]
    X, Y = P[..., 0], P[..., 1]
    den = ((X[..., 1] - X[..., 0]) * (Y[..., 2] - Y[..., 0]) - (X[..., 2] - X[..., 0]) * (Y[..., 1] - Y[..., 0])).detach()
    w = torch.sign(den)
    # per side k: corner a = k to c = (k + 1) mod 3
    ex, ey = X.roll(-1, -1) - X, Y.roll(-1, -1) - Y                                 # [B,h,w,3]
    N = ex * (pny[..., None] - Y) - ey * (pnx[..., None] - X)
    Eo = ex * (poy[..., None] - Y) - ey * (pox[..., None] - X)
    qual = (N.detach() * w[..., None] >= 0) & (Eo.detach() * w[..., None] < 0)
    D = torch.where(qual, N - Eo, torch.ones_like(N))
    tk = N / D
    tsel = torch.where(qual, tk.detach(), torch.full_like(tk, float("inf")))
    k = tsel.argmin(-1)                                                            # (the first of equal minima: the lowest k)
    has_edge = qual.any(-1)
    pick = lambda a: a.gather(-1, k[..., None])[..., 0]
    t = pick(tk)
    j = torch.where(back, (4 - k) % 3, k)
    opp = side[fn % F, j]
    O = sv.to(dtype)[bidx, opp.clamp(min=0)]
    EO = pick(ex) * (O[..., 1] - pick(Y)) - pick(ey) * (O[..., 0] - pick(X))
    silhouette = (opp == -1) | ((opp >= 0) & (EO.detach() * w >= 0))
    active = differ & has_edge & silhouette
    to_far, to_near = active & (t.detach() > 0.5), active & (t.detach() < 0.5)
    cn, co = torch.where(p_near[:, None], cp, cq), torch.where(p_near[:, None], cq, cp)
    zero = torch.zeros_like(cn)
    delta_o = torch.where(to_far[:, None], (t - 0.5)[:, None] * (cn - co), zero)
    delta_n = torch.where(to_near[:, None], (0.5 - t)[:, None] * (co - cn), zero)
    delta_p = torch.where(p_near[:, None], delta_n, delta_o)
    delta_q = torch.where(p_near[:, None], delta_o, delta_n)
    # the fragile-pair rule, on detached float64-or-dtype values
    with torch.no_grad():
        size = ex.abs() + ey.abs()
        two = torch.where(qual, tk, torch.full_like(tk, float("inf"))).sort(-1).values
        close = (qual.sum(-1) >= 2) & ((two[..., 1] - two[..., 0]).abs() < TAU)
        near_side = ((N.abs() < TAU * size * 2 / S) | (Eo.abs() < TAU * size * 2 / S)).any(-1)
        near_o = (opp >= 0) & has_edge & (EO.abs() < TAU * pick(size) * ((O[..., 0] - pick(X)).abs() + (O[..., 1] - pick(Y)).abs()))
        both = (fp >= 0) & (fq >= 0)
        dmax = torch.where(both, torch.maximum(dp, dq), torch.ones_like(dp))
        near_depth = both & ((torch.where(both, dp - dq, torch.ones_like(dp))).abs() < TAU * dmax)
        fragile = differ & ((has_edge & ((t - 0.5).abs() < TAU)) | close | near_side | near_o | near_depth)
    return delta_p, delta_q, fragile


def antialias_of(maps, tri, sv, images, dtype=torch.float64, side=None):
    """(out [B,C,S,S] in `dtype`, output orientation, differentiable in sv [B,V,3] and in images; keep [B,1,S,S] bool, output
    orientation: False at both pixels of every fragile pair)."""
    side = side_opposite_of(tri) if side is None else side
    c = images.to(dtype).flip(2)                                                   # the maps' orientation
    dpx, dqx, frx = _pairs(maps, tri, side, sv, c, 0, dtype)
    dpy, dqy, fry = _pairs(maps, tri, side, sv, c, 1, dtype)
    pad = torch.nn.functional.pad
    # a pixel adds its pairs in the order -x (it is q), +x (it is p), -y, +y
    out = c + pad(dqx, (1, 0)) + pad(dpx, (0, 1)) + pad(dqy, (0, 0, 1, 0)) + pad(dpy, (0, 0, 0, 1))
    frx, fry = frx.to(torch.uint8), fry.to(torch.uint8)
    fragile = (pad(frx, (1, 0)) | pad(frx, (0, 1)) | pad(fry, (0, 0, 1, 0)) | pad(fry, (0, 0, 0, 1))).bool()
    return out.flip(2), ~fragile.flip(1)[:, None]


def reference(maps, tri, sv, images, grad_out, dtype=torch.float64, side=None, keep=None):
    """(out, keep, grad_images, grad_sv) in `dtype` with grad_out zeroed at the pixels left out; keep: the mask to use
    instead of this evaluation's own (a float32 evaluation takes the float64 one's)"""
    s = sv.detach().cpu().to(dtype).requires_grad_(True)
    im = images.detach().cpu().to(dtype).requires_grad_(True)
    out, own = antialias_of(maps, tri, s, im, dtype, side)
    keep = own if keep is None else keep
    g = grad_out.detach().cpu().to(dtype) * keep
    gi, gs = torch.autograd.grad((out * g).sum(), (im, s))
    return out.detach(), keep, gi, gs


def left_out_share(keep):
    return 1.0 - float(keep.float().mean())


def oracle_case(name, S):
    """(maps, tri, sv) of a scene at raster size S on the CPU oracle"""
    from vertex_attribute_scenes import oracle_maps
    return oracle_maps(name, S), scene(name)["tri"], FG.screen_vertices(name)
