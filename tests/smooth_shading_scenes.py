"""Scenes and restatements for the smooth-shading tests (neural_renderer/smooth_shading.py, mesh_cython.fit_illumination),
shared by tests/test_smooth_shading_host.py, tests/test_gpu_smooth_shading.py and tests/golden/make_golden_sh.py."""
import math

import numpy as np
import torch

import mesh_scenes

A0, A1 = math.sqrt(1 / (4 * math.pi)), math.sqrt(3 / (4 * math.pi))
A2, A3, A4 = 0.5 * A1, 3 * math.sqrt(5 / (12 * math.pi)), 1.5 * math.sqrt(5 / (12 * math.pi))
EPS = 1e-6
RIM = 12


# ---- meshes -----------------------------------------------------------------------------------------------------------------
def fan_mesh(seed=0):
    """(vertices [V,3] f64 numpy, faces [F,3] int64 numpy, notes).  Three fans whose apexes have exactly LONG_ROW, LONG_ROW + 1
    and 2 CHUNK + 1 faces: each fan's triangles cycle round a ring of 12 jittered rim vertices (a ring of n slivers would lose
    four digits in f32; this keeps every normal well conditioned) and the apex takes corner slot k % 3 of triangle k, the
    orientation kept.  Then a 17 x 17 jittered height-field grid (V > 256), one face [a, a, b] on two grid vertices, and a last
    vertex that is in no face."""
    from deep3dmap_amd.neural_renderer.row_gather import CHUNK, LONG_ROW
    rng = np.random.default_rng(seed)
    verts, faces, hubs = [], [], {}
    for i, count in enumerate((LONG_ROW, LONG_ROW + 1, 2 * CHUNK + 1)):
        base = len(verts)
        centre = np.array([3.0 * i, 0.0, 0.0])
        verts.append(centre + np.array([0.0, 0.0, 0.6]) + rng.uniform(-0.05, 0.05, 3))
        for j in range(RIM):
            a = 2 * math.pi * j / RIM
            verts.append(centre + np.array([math.cos(a), math.sin(a), 0.0]) + rng.uniform(-0.05, 0.05, 3))
        hubs[base] = count
        for k in range(count):
            tri = [base, base + 1 + k % RIM, base + 1 + (k + 1) % RIM]
            faces.append(tri[-(k % 3):] + tri[:-(k % 3)] if k % 3 else tri)          # the apex at slot k % 3
    n, base = 17, len(verts)
    for y in range(n):
        for x in range(n):
            verts.append(np.array([0.25 * x, 2.0 + 0.25 * y, 0.3 * math.sin(0.7 * x) * math.cos(0.5 * y)]) +
                         rng.uniform(-0.04, 0.04, 3))
    idx = base + np.arange(n * n).reshape(n, n)
    tl, tr, bl, br = idx[:-1, :-1], idx[:-1, 1:], idx[1:, :-1], idx[1:, 1:]
    faces += np.stack([tl, tr, bl], -1).reshape(-1, 3).tolist() + np.stack([bl, tr, br], -1).reshape(-1, 3).tolist()
    doubled = (int(idx[3, 3]), int(idx[9, 11]))
    faces.append([doubled[0], doubled[0], doubled[1]])
    verts.append(np.array([-2.0, -2.0, 1.0]))
    v, f = np.stack(verts), np.array(faces, np.int64)
    return v, f, dict(hubs=hubs, unused=len(verts) - 1, doubled=doubled, doubled_face=len(faces) - 1)


def grid_mesh(n, seed=0):
    """A jittered n x n height field without long rows: (vertices [n n, 3] f64 numpy, faces int64 numpy)."""
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v = np.stack([xs * 0.1, ys * 0.1, 0.2 * np.sin(0.3 * xs) * np.cos(0.2 * ys)], -1).reshape(-1, 3)
    v = v + rng.uniform(-0.02, 0.02, v.shape)
    idx = np.arange(n * n).reshape(n, n)
    tl, tr, bl, br = idx[:-1, :-1], idx[:-1, 1:], idx[1:, :-1], idx[1:, 1:]
    f = np.concatenate([np.stack([tl, tr, bl], -1).reshape(-1, 3), np.stack([bl, tr, br], -1).reshape(-1, 3)], 0)
    return v, f.astype(np.int64)


def case_inputs(vertices, B, seed):
    """float64 torch inputs for `B` sets over `vertices` [V,3]: x [B,V,3] (the mesh, jittered per set), colors [B,V,3] in
    (0.2, 0.9), sh [B,3,9], and the output gradients g [B,V,3], g_normals [B,V,3]."""
    gen = torch.Generator().manual_seed(seed)
    V = vertices.shape[0]
    x = torch.from_numpy(vertices)[None] + 0.01 * (torch.rand(B, V, 3, generator=gen, dtype=torch.float64) - 0.5)
    colors = 0.2 + 0.7 * torch.rand(B, V, 3, generator=gen, dtype=torch.float64)
    sh = torch.rand(B, 3, 9, generator=gen, dtype=torch.float64) - 0.5
    sh[:, :, 0] += 2.0
    g = torch.rand(B, V, 3, generator=gen, dtype=torch.float64) - 0.5
    g_normals = torch.rand(B, V, 3, generator=gen, dtype=torch.float64) - 0.5
    # (values exactly representable in float32, so every dtype starts from the same numbers)
    return tuple(t.float().double() for t in (x, colors, sh, g, g_normals))


# ---- the restatement of the node: forward and manual adjoint, in the inputs' dtype -----------------------------------------
def basis(n):
    nx, ny, nz = n.unbind(-1)
    return torch.stack([torch.full_like(nx, A0), A1 * nx, A1 * ny, A1 * nz, A2 * (2 * nz * nz - nx * nx - ny * ny),
                        A3 * (ny * nz), A3 * (nx * nz), A3 * (nx * ny), A4 * (nx * nx - ny * ny)], -1)


def basis_gradient(n):
    """[..., 9, 3]: d H_j / d n_c"""
    nx, ny, nz = n.unbind(-1)
    z, o = torch.zeros_like(nx), torch.ones_like(nx)
    rows = [(z, z, z), (A1 * o, z, z), (z, A1 * o, z), (z, z, A1 * o), (-2 * A2 * nx, -2 * A2 * ny, 4 * A2 * nz),
            (z, A3 * nz, A3 * ny), (A3 * nz, z, A3 * nx), (A3 * ny, A3 * nx, z), (2 * A4 * nx, -2 * A4 * ny, z)]
    return torch.stack([torch.stack(r, -1) for r in rows], -2)


def _scatter(faces, per_corner, V):
    """sum over the corners: per_corner [3][B,F,3] -> [B,V,3]"""
    out = torch.zeros(per_corner[0].shape[0], V, 3, dtype=per_corner[0].dtype)
    for c in range(3):
        out = out.index_add(1, faces[:, c], per_corner[c])
    return out


def restate_forward(x, faces, colors, sh):
    """x [B,V,3], faces [F,3] int64, colors [B,V,3], sh [B,3,9] -> (shaded [B,V,3], n [B,V,3], r [B,V]); differentiable."""
    x0, x1, x2 = (x[:, faces[:, c]] for c in range(3))
    N = torch.linalg.cross(x1 - x0, x2 - x0)
    s = _scatter(faces, [N, N, N], x.shape[1])
    r = torch.linalg.vector_norm(s, dim=-1)
    n = s / r.clamp(min=EPS)[..., None]
    L = torch.einsum("bkj,bvj->bvk", sh, basis(n))
    return colors * L, n, r


def restate_adjoint(x, faces, colors, sh, g, g_normals=None):
    """(g_x, g_colors, g_sh) of the formulas of csrc/d3m_smooth_shade.h, every set on its own."""
    _, n, r = restate_forward(x, faces, colors, sh)
    H = basis(n)
    L = torch.einsum("bkj,bvj->bvk", sh, H)
    gL = g * colors
    g_sh = torch.einsum("bvk,bvj->bkj", gL, H)
    g_n = torch.einsum("bvk,bkj,bvjc->bvc", gL, sh, basis_gradient(n))
    if g_normals is not None:
        g_n = g_n + g_normals
    proj = (g_n - n * (n * g_n).sum(-1, keepdim=True)) / r.clamp(min=EPS)[..., None]
    g_s = torch.where((r >= EPS)[..., None], proj, g_n / EPS)
    gN = (g_s[:, faces[:, 0]] + g_s[:, faces[:, 1]]) + g_s[:, faces[:, 2]]
    a, b = x[:, faces[:, 1]] - x[:, faces[:, 0]], x[:, faces[:, 2]] - x[:, faces[:, 0]]
    t1, t2 = torch.linalg.cross(b, gN), torch.linalg.cross(gN, a)
    return _scatter(faces, [-(t1 + t2), t1, t2], x.shape[1]), g * L, g_sh


def reference(x, faces, colors, sh, g, g_normals):
    """dict of the five checked tensors (normals, shaded, g_x, g_colors, g_sh) in the inputs' dtype"""
    shaded, n, _ = restate_forward(x, faces, colors, sh)
    g_x, g_c, g_sh = restate_adjoint(x, faces, colors, sh, g, g_normals)
    return dict(normals=n, shaded=shaded, g_x=g_x, g_colors=g_c, g_sh=g_sh)


def tolerances(ref64, ref32):
    """Per tensor max(8 E32, 16 2^-24 max|ref|), E32 the largest deviation of the float32 restatement from the float64 one."""
    out = {}
    for name, r in ref64.items():
        e32 = float((ref32[name].double() - r).abs().max())
        out[name] = (max(8 * e32, 16 * 2.0 ** -24 * float(r.abs().max())), e32)
    return out


# ---- fit_illumination -------------------------------------------------------------------------------------------------------
FIT_SCENES = {"g12_40x48": (12, 40, 48, 11, 0.0), "g20_64x56": (20, 64, 56, 12, 0.0), "g12_outside": (12, 40, 48, 13, 9.0)}


def fit_scene(name):
    """dict(image [h,w,3], vertices [3,nver], texture [3,nver] ~ U(0.2, 0.9), triangles [3,ntri] int32, vis_ind: every second
    vertex) of float64 numpy arrays; `push` > 0 spreads the vertices beyond the image so the clamp and the rounding run."""
    n, h, w, seed, push = FIT_SCENES[name]
    s = mesh_scenes.grid_scene(n, h, w, seed, big=False)
    rng = np.random.default_rng(1000 + seed)
    v = s["vertices"].copy()
    if push:
        centre = np.array([[w / 2.0], [h / 2.0]])
        v[:2] = centre + (v[:2] - centre) * 1.5 + rng.uniform(-push, push, v[:2].shape)
    texture = rng.uniform(0.2, 0.9, (3, v.shape[1]))
    return dict(image=s["src_image"], vertices=v, texture=texture, triangles=s["triangles"],
                vis_ind=np.arange(0, v.shape[1], 2))


def norm_direction64(vertices, triangles):
    """get_norm_direction's definition in float64 numpy: the normals cross(p0 - p1, p0 - p2) of a vertex's triangles added in
    triangle order, normalised; a vertex whose sum is zero gets (1, 0, 0).  ([3,nver], [3,ntri] -> [3,nver])"""
    p0, p1, p2 = (vertices[:, triangles[c]].T for c in range(3))
    tri_norm = np.cross(p0 - p1, p0 - p2)
    norm = np.zeros((vertices.shape[1], 3))
    np.add.at(norm, triangles.T.reshape(-1), np.repeat(tri_norm, 3, axis=0))
    mag = (norm ** 2).sum(1)
    zero = mag == 0
    norm[zero] = (1.0, 0.0, 0.0)
    mag[zero] = 1.0
    return (norm / np.sqrt(mag)[:, None]).T
