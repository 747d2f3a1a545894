"""Mirror of the weak-perspective pose lines of deep3dmap/models/frameworks/imgs2mesh.py on nr.pose_vertices: `face_project`
(:111-118, the argument Pt3dRenderer.sample takes), `landmarks68` (:194-197) and `supervised_losses` (:165-200)."""
import torch

from ..neural_renderer.pose import pose_vertices

ANGLE_LIMIT = 3.1415        # imgs2mesh.py:112 and :194
POINT_LIMIT = 125000.0      # imgs2mesh.py:80
W_POINTS, W_SCALE, W_ANGLES, W_TRANSLATION, W_LANDMARKS = 0.0001, 20.0, 1.0, 1.0, 0.02    # imgs2mesh.py:172, :192, :198


def _pose_rows(pose, what):
    if not torch.is_tensor(pose) or pose.dim() != 2 or pose.shape[1] != 7:
        raise ValueError(f"{what}: pose must be [B, 7] (scale, three angles, translation)")


def face_project(points, pose, image_size):
    """imgs2mesh.py:111-118: points [B,V,3] (or [V,3], shared), pose [B,7] = param2points_bfm's second element, read in
    place.  Returns (face_project [B,V,2], outangles [B,3]):

        outangles    = clamp(pose[:, 1:4], -3.1415, 3.1415)
        p            = pose[:, 0] * (euler_angles_to_matrix(outangles, "XYZ") points) + pose[:, 4:7] * image_size
        face_project = (p_x / image_size, 1 - p_y / image_size)

    as ONE pose_vertices node that writes only the [B,V,2] output; both go straight into Pt3dRenderer.sample."""
    _pose_rows(pose, "face_project")
    if not float(image_size) > 0:
        raise ValueError("face_project: image_size must be positive")
    out = pose_vertices(points, pose, translation_scale=float(image_size), angle_limit=ANGLE_LIMIT, uv_size=float(image_size),
                        posed=False)
    return out.uv, torch.clamp(pose[:, 1:4], min=-ANGLE_LIMIT, max=ANGLE_LIMIT)


def landmarks68(points, pose, lm_idx, image_size):
    """imgs2mesh.py:194-197: the image-plane landmarks [B,L,2] = (s R points + T image_size)[:, lm_idx, :2], as one
    pose_vertices node that computes the L landmark points only."""
    _pose_rows(pose, "landmarks68")
    out = pose_vertices(points, pose, translation_scale=float(image_size), angle_limit=ANGLE_LIMIT, landmarks=lm_idx,
                        posed=False)
    return out.landmarks[:, :, :2]


def supervised_losses(outpts_list, outpose_list, gtaux, gtobj, lm_idx, image_size, landmarks_fn=landmarks68):
    """imgs2mesh.py:165-200 (with the clamp of :80 on the points): {'ptsloss', 'poseloss', 'lm68loss'} of the views k.

    outpts_list[k] [B,V,3] and outpose_list[k] [B,7] are param2points_bfm's outputs for view k; gtaux [B,n_views,>=152] holds
    per view the 68 reference landmarks (:136 as [68,2]), the scale (136), the rotation (137:146, not used here), the
    translation (146:149) and the angles (149:152); gtobj [B,V,3] the reference points.  Weights 0.0001 (points), 20 / 1 / 1
    (scale, angles, translation xy) and 0.02 (landmarks); every loss is an L1 mean, left to torch.  landmarks_fn(points,
    pose, lm_idx, image_size) -> [B,L,2] is landmarks68 unless a restatement is passed (the host tests do)."""
    if len(outpts_list) != len(outpose_list) or not outpts_list:
        raise ValueError("supervised_losses: outpts_list and outpose_list must hold one entry per view")
    n_views = len(outpts_list)
    if gtaux.dim() != 3 or gtaux.shape[1] < n_views or gtaux.shape[2] < 152:
        raise ValueError(f"supervised_losses: gtaux must be [B, >= {n_views}, >= 152]")
    l1 = torch.nn.functional.l1_loss
    ptsloss = poseloss = lm68loss = 0
    for k in range(n_views):
        outpts = torch.clamp(outpts_list[k], min=-POINT_LIMIT, max=POINT_LIMIT)
        pose = outpose_list[k]
        _pose_rows(pose, "supervised_losses")
        ptsloss = ptsloss + W_POINTS * l1(outpts, gtobj)
        aux = gtaux[:, k]
        want_lm, want_s, want_t, want_angles = aux[:, :136].reshape(-1, 68, 2), aux[:, 136], aux[:, 146:148], aux[:, 149:152]
        poseloss = poseloss + (W_SCALE * l1(pose[:, 0], want_s) + W_ANGLES * l1(pose[:, 1:4], want_angles)
                               + W_TRANSLATION * l1(pose[:, 4:6], want_t))
        lm68loss = lm68loss + W_LANDMARKS * l1(landmarks_fn(outpts, pose, lm_idx, image_size), want_lm)
    return {'ptsloss': ptsloss, 'poseloss': poseloss, 'lm68loss': lm68loss}
