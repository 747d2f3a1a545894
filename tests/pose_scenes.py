"""Shared by the pose tests (test_pose_host.py, test_gpu_pose.py): the hashed input generators of morphable_scenes.py, a
float64 statement of what deep3dmap/models/frameworks/imgs2mesh.py:111-118, :194-197 and :165-200 compute (written here from
the formulas, in the dtype of its inputs), and the derived error bounds of the node.

THE BOUNDS.  u = 2^-24.  The device's sinf / cosf are ASSUMED to be within TRIG_ULP = 4 ulp (no HIP math accuracy table is
installed beside the compiler to take the figure from), that is a relative error of at most 2 TRIG_ULP u each.

  R.  An entry of Rx Ry Rz is a sum of at most two terms, each a product of at most three trig values; the sum of the terms'
  absolute values is at most 1 (|cx sz| + |sx sy cz| <= |cx||sz| + |sx||cz| <= 1 by Cauchy-Schwarz, and likewise for the
  others).  The kernel forms it with two 3x3 products of (a0 b0 + a1 b1) + a2 b2: at most 3 roundings per product and entry.
  So |fl(R_jk) - R_jk| <= E_R = (3 * 2 TRIG_ULP + 6) u.  The same holds for an entry of dR/da_k (one factor is
  differentiated: cos and sin swap, the same shapes).  This is the TRIG ALLOWANCE; it is absolute, not relative to |R_jk|.

  posed.  r_j = (R_j0 x_0 + R_j1 x_1) + R_j2 x_2: 3 roundings; s r_j: 1; tau t_j: 1; their sum: 1.  With |R_jk| <= 1:
      |fl(posed_j) - posed_j| <= C_POSED u (|s| sum_k |x_k| + |tau t_j|),   C_POSED = 6 TRIG_ULP + 6 + 3 + 1 + 1 + 1 = 36,
  the last 1 covering the products of two relative errors (C_POSED^2 u^2 against u).
  uv adds a division, and its y a subtraction from 1 (one rounding of a value of at most 1 + |y| / uv_size):
      |fl(uv) - uv| <= (C_POSED + 2) u ((|s| sum_k |x_k| + |tau t_j|) / uv_size + 1).

  gradients.  Every gradient is a sum of terms.  A chain of n additions in ANY order gives at most n u sum|terms| (Higham,
  Accuracy and Stability of Numerical Algorithms, 4.2, first order): the issue's bound, with the chain from the constants
  neural_renderer/pose.py exports and the absolute terms taken with the true |R_jc| and |dR_jc|.  To the chain come the
  roundings inside one term, and beside it the trig allowance on the sum WITHOUT |R| (the error of R is absolute):
      G = g_posed + g_uv / uv_size: 2;  G x: 1;  M R (or M dR): 1;  s times: 1;  second order: 1   ->  C_TERM = 6,
      and the sum of the nine products adds 8 to the chain of g_s and g_a.
      |fl(g_s) - g_s|     <= (pose_chain + 8 + C_TERM) u sum_jc absM_jc |R_jc|      + E_R sum_jc absM_jc
      |fl(g_a_k) - g_a_k| <= (pose_chain + 8 + C_TERM) u |s| sum_jc absM_jc |dR_jc| + E_R |s| sum_jc absM_jc   (0: clamped)
      |fl(g_t_j) - g_t_j| <= (pose_chain + C_TERM) u |tau| absn_j
      |fl(g_x_j) - g_x_j| <= (vertex_chain + C_TERM) u sum_b |s_b| sum_i |R_ij| |G_i| + E_R sum_b |s_b| sum_i |G_i|
  with absM_jc = sum_v |G_j| |x_c|, absn_j = sum_v |G_j|, |G| = |g_posed| + |g_uv| / uv_size + the |landmark gradients| that
  point at the vertex, and b over the sets that share x.  Nothing here is fitted to what the kernels return."""
import numpy as np
import torch

from morphable_scenes import hash_grid, hashed_floats, hashed_ints      # noqa: F401  (the generators, re-exported)

U = 2.0 ** -24
TRIG_ULP = 4            # assumed: see above
C_POSED = 6 * TRIG_ULP + 12
C_TERM = 6                      # the roundings inside one term of a gradient
E_R = (6 * TRIG_ULP + 6) * U    # the trig allowance: the absolute error of an entry of R or dR/da_k
ANGLE_LIMIT = 3.1415


def euler_factors(angles):
    """([Rx, Ry, Rz], [Rx', Ry', Rz']) for angles [B,3], each [B,3,3]: the factors of pytorch3d's
    euler_angles_to_matrix(angles, "XYZ") = Rx(a0) Ry(a1) Rz(a2) and their derivatives"""
    c, s = torch.cos(angles), torch.sin(angles)
    one, nil = torch.ones_like(c[:, 0]), torch.zeros_like(c[:, 0])

    def grid(*rows):
        return torch.stack([torch.stack(r, -1) for r in rows], -2)

    f = [grid((one, nil, nil), (nil, c[:, 0], -s[:, 0]), (nil, s[:, 0], c[:, 0])),
         grid((c[:, 1], nil, s[:, 1]), (nil, one, nil), (-s[:, 1], nil, c[:, 1])),
         grid((c[:, 2], -s[:, 2], nil), (s[:, 2], c[:, 2], nil), (nil, nil, one))]
    d = [grid((nil, nil, nil), (nil, -s[:, 0], -c[:, 0]), (nil, c[:, 0], -s[:, 0])),
         grid((-s[:, 1], nil, c[:, 1]), (nil, nil, nil), (-c[:, 1], nil, -s[:, 1])),
         grid((-s[:, 2], -c[:, 2], nil), (c[:, 2], -s[:, 2], nil), (nil, nil, nil))]
    return f, d


def euler_xyz(angles):
    """Rx(a0) Ry(a1) Rz(a2) for angles [B,3]: [B,3,3]"""
    f, _ = euler_factors(angles)
    return f[0] @ f[1] @ f[2]


def euler_xyz_derivatives(angles):
    """[dR/da0, dR/da1, dR/da2], each [B,3,3]"""
    f, d = euler_factors(angles)
    return [d[0] @ f[1] @ f[2], f[0] @ d[1] @ f[2], f[0] @ f[1] @ d[2]]


def _batched(points, B):
    return points if points.dim() == 3 and points.shape[0] == B else points.reshape(-1, 3)[None].expand(B, -1, -1)


def clamped_angles(pose, angle_limit=None):
    return pose[:, 1:4] if angle_limit is None else pose[:, 1:4].clamp(-angle_limit, angle_limit)


def restate_posed(points, pose, translation_scale=1.0, angle_limit=None):
    """scale * R(clamped angles) x + translation_scale * translation: points [V,3] or [B,V,3], pose [B,7] -> [B,V,3]"""
    B = pose.shape[0]
    turned = torch.einsum("bij,bvj->bvi", euler_xyz(clamped_angles(pose, angle_limit)), _batched(points, B))
    return pose[:, 0].reshape(B, 1, 1) * turned + translation_scale * pose[:, 4:7].reshape(B, 1, 3)


def restate_node(points, pose, translation_scale=1.0, angle_limit=None, uv_size=None, landmarks=None):
    """nr.pose_vertices: (posed [B,V,3], uv [B,V,2] or None, landmark points [B,L,3] or None)"""
    posed = restate_posed(points, pose, translation_scale, angle_limit)
    uv = lm = None
    if uv_size is not None:
        uv = torch.stack([posed[..., 0] / uv_size, 1 - posed[..., 1] / uv_size], -1)
    if landmarks is not None:
        lm = posed.index_select(1, landmarks.long())
    return posed, uv, lm


def image_coordinates64(points, pose, image_size, angle_limit=ANGLE_LIMIT):
    """what imgs2mesh.py:111-118 hands to Pt3dRenderer.sample: ((x / size, 1 - y / size) of the posed points [B,V,2], the
    clamped angles [B,3])"""
    return restate_node(points, pose, image_size, angle_limit, image_size)[1], clamped_angles(pose, angle_limit)


def landmarks64(points, pose, lm_idx, image_size, angle_limit=ANGLE_LIMIT):
    """what imgs2mesh.py:194-197 compares with the reference landmarks: x and y of the posed landmark points, [B,L,2]"""
    return restate_node(points, pose, image_size, angle_limit, None, lm_idx)[2][..., :2]


def mean_abs(a, b):
    return (a - b).abs().mean()


def losses64(points_per_view, pose_per_view, gtaux, gtobj, lm_idx, image_size):
    """The three supervised losses of imgs2mesh.py:165-200, stated from their definitions: per view, with the points clamped
    to +-125000, ptsloss = 0.0001 mean|points - gtobj|; poseloss = 20 mean|scale - aux[136]| + mean|angles - aux[149:152]| +
    mean|translation_xy - aux[146:148]|; lm68loss = 0.02 mean|landmarks_xy - aux[:136] as [68,2]|; each summed over the views."""
    total = {"ptsloss": 0.0, "poseloss": 0.0, "lm68loss": 0.0}
    for view, (points, pose) in enumerate(zip(points_per_view, pose_per_view)):
        aux = gtaux[:, view]
        points = points.clamp(-125000.0, 125000.0)
        total["ptsloss"] = total["ptsloss"] + 1e-4 * mean_abs(points, gtobj)
        total["poseloss"] = total["poseloss"] + (20.0 * mean_abs(pose[:, 0], aux[:, 136]) + mean_abs(pose[:, 1:4], aux[:, 149:152])
                                                 + mean_abs(pose[:, 4:6], aux[:, 146:148]))
        wanted = aux[:, :136].reshape(aux.shape[0], 68, 2)
        total["lm68loss"] = total["lm68loss"] + 0.02 * mean_abs(landmarks64(points, pose, lm_idx, image_size), wanted)
    return total


# ---- the bounds (float64 torch tensors in, float64 out) --------------------------------------------------------------------
def posed_bound(points, pose, translation_scale=1.0):
    """[B,V,3]: C_POSED u (|s| sum_k |x_k| + |tau t_j|)"""
    B = pose.shape[0]
    reach = pose[:, 0].abs().reshape(B, 1, 1) * _batched(points, B).abs().sum(2, keepdim=True)
    return C_POSED * U * (reach + (translation_scale * pose[:, 4:7]).abs().reshape(B, 1, 3))


def uv_bound(points, pose, translation_scale, uv_size):
    """[B,V,2]: (C_POSED + 2) u ((|s| sum_k |x_k| + |tau t_j|) / uv_size + 1)"""
    return (C_POSED + 2) / C_POSED * (posed_bound(points, pose, translation_scale)[:, :, :2] / uv_size + C_POSED * U)


def abs_gradient(B, V, uv_size=None, landmarks=None, g_posed=None, g_uv=None, g_lm=None):
    """|G| [B,V,3]: |g_posed| + |g_uv| / uv_size + the |landmark gradients| pointing at each vertex"""
    G = torch.zeros(B, V, 3, dtype=torch.float64)
    if g_posed is not None:
        G = G + g_posed.abs()
    if g_uv is not None:
        G[:, :, :2] += g_uv.abs() / uv_size
    if g_lm is not None:
        G.index_add_(1, landmarks.long(), g_lm.abs())
    return G


def gradient_bounds(points, pose, translation_scale, absG, pose_chain, vertex_chain, shared, angle_limit=None):
    """(bound of grad_pose [B,7], bound of grad_vertices [1 or B,V,3]) from |G| = abs_gradient(...) and the two chains"""
    B = pose.shape[0]
    x = _batched(points, B).abs()
    angles = clamped_angles(pose, angle_limit)
    R = euler_xyz(angles).abs()
    absM = torch.einsum("bvj,bvc->bjc", absG, x)            # sum_v |G_j| |x_c|
    absn = absG.sum(1)
    s = pose[:, 0].abs()
    chain = (pose_chain + 8 + C_TERM) * U
    bp = torch.empty(B, 7, dtype=torch.float64)
    bp[:, 0] = chain * (absM * R).sum((1, 2)) + E_R * absM.sum((1, 2))
    for k, dR in enumerate(euler_xyz_derivatives(angles)):
        bp[:, 1 + k] = s * (chain * (absM * dR.abs()).sum((1, 2)) + E_R * absM.sum((1, 2)))
    bp[:, 4:7] = (pose_chain + C_TERM) * U * abs(translation_scale) * absn
    bv = s.reshape(B, 1, 1) * ((vertex_chain + C_TERM) * U * torch.einsum("bij,bvi->bvj", R, absG)
                               + E_R * absG.sum(2, keepdim=True))
    if shared:
        bv = bv.sum(0, keepdim=True)
    return bp, bv


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def landmark_indices(L, V, salt=0, repeats=False):
    """L vertex indices in [0, V) from the hash; with repeats, every third entry repeats the one three before it"""
    idx = (hash_grid(L, 1, 300 + salt)[:, 0] * 31 + np.arange(L) * 7919) % V
    if repeats:
        idx[3::3] = idx[:-3:3]
    return idx.astype(np.int64)


def float_pose(B, salt, limit=ANGLE_LIMIT):
    """[B,7] f32: scale in [0.5, 2], angles across (-pi, pi) with the first set's beyond +-limit and the second's exactly at
    it, translation in [-1, 1]"""
    p = np.empty((B, 7), np.float32)
    p[:, 0] = hashed_floats(B, 1, salt, 0.5, 2.0)[:, 0]
    p[:, 1:4] = hashed_floats(B, 3, salt + 1, -3.1, 3.1)
    p[:, 4:7] = hashed_floats(B, 3, salt + 2, -1.0, 1.0)
    p[0, 1:4] = (3.3, -3.1416, 0.7)
    if B > 1:
        p[1, 1:4] = (np.float32(limit), -np.float32(limit), -2.9)
    return p
