"""Mirror of deep3dmap/core/evaluation/mesh_eval.py on the device: nn_correspondance (each point's nearest neighbour in the
other set, Euclidean) and the metrics of eval_fscore -- mean distances both ways, precision, recall and F-score at a threshold
-- on top of neural_renderer.nearest_points (csrc/d3m_point_sets.h: exact brute force, the lowest index among equal
distances) instead of one k-d tree query per point on the CPU.

The reference's eval_fscore reads two point-cloud files with Open3D and thins them with voxel_down_sample before it measures.
Both steps are OUT OF SCOPE here: neither can be checked against Open3D where it is not installed.  eval_points takes the
point arrays that eval_fscore has after those steps; read and thin the clouds with whatever the caller has."""
import numpy as np
import torch

from ..neural_renderer.point_sets import nearest_points


def _points(points, name):
    """points as a detached f32 tensor [n,3] where it is; None for an empty set"""
    t = torch.as_tensor(np.asarray(points) if not torch.is_tensor(points) else points)
    if t.numel() == 0:
        return None
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"mesh_eval: {name} must be [num_points, 3]")
    return t.detach().to(torch.float32)


def _on_device(*sets):
    """the sets on one GPU: the first one's if it is on one, else the current one"""
    if not torch.cuda.is_available():
        raise ValueError("mesh_eval: the nearest-point search needs a GPU device")
    device = next((t.device for t in sets if t.is_cuda), torch.device("cuda"))
    return [t.to(device) for t in sets]


def _nearest(verts1, verts2):
    """(index [n2] int32, distance [n2]) on the device of each point of verts2 to its nearest point of verts1"""
    index, dist2 = nearest_points(verts2, verts1)
    return index, torch.sqrt(dist2)


def nn_correspondance(verts1, verts2):
    """For each point of verts2 the nearest point of verts1 (mesh_eval.py:46-72): (indices, distances), the distance being
    the Euclidean one (the square root, as the reference).  verts1, verts2: [n,3] tensors or numpy arrays, moved to the GPU as
    f32.  Returns two lists ([], []) when either set is empty, as the reference does; else an int32 and an f32 tensor of
    length len(verts2) on the device."""
    v1, v2 = _points(verts1, "verts1"), _points(verts2, "verts2")
    if v1 is None or v2 is None:
        return [], []
    return _nearest(*_on_device(v1, v2))


def eval_points(verts_pred, verts_trgt, threshold=.05):
    """The metrics of the reference's eval_fscore (mesh_eval.py:28-43) on two point arrays: a dict of floats with the
    reference's names -- its local dist1 holds, per TARGET point, the distance to the nearest predicted point and its local
    dist2, per PREDICTED point, the distance to the nearest target point, and its dict swaps them: 'dist1' is mean(dist2), the
    mean over the prediction's points, and 'dist2' is mean(dist1), the mean over the target's; 'prec' the share of the prediction's points within
    `threshold` of the target, 'recal' the share of the target's points within it of the prediction, 'fscore' their harmonic
    mean: nan when prec + recal is 0, as the reference's division gives.  The threshold counts are integer sums on the
    device.  An empty set gives the means of empty arrays: nan."""
    pred, trgt = _points(verts_pred, "verts_pred"), _points(verts_trgt, "verts_trgt")
    if pred is None or trgt is None:
        nan = float("nan")
        return {'dist1': nan, 'dist2': nan, 'prec': nan, 'recal': nan, 'fscore': nan}
    pred, trgt = _on_device(pred, trgt)
    _, to_pred = _nearest(pred, trgt)           # the reference's dist1: per target point
    _, to_trgt = _nearest(trgt, pred)           # the reference's dist2: per predicted point
    return metrics_of(to_pred, to_trgt, threshold)


def metrics_of(to_pred, to_trgt, threshold):
    """eval_points' dict from the two distance arrays (tensors on any device): to_pred per target point, to_trgt per predicted
    point."""
    counts = torch.stack(((to_trgt < threshold).sum(), (to_pred < threshold).sum()))        # int64: exact in any order
    means = torch.stack((to_trgt.double().mean(), to_pred.double().mean()))
    within_trgt, within_pred = (int(v) for v in counts.cpu())
    mean_to_trgt, mean_to_pred = (float(v) for v in means.cpu())
    precision, recal = within_trgt / to_trgt.numel(), within_pred / to_pred.numel()
    with np.errstate(invalid="ignore", divide="ignore"):
        fscore = float(np.float64(2 * precision * recal) / np.float64(precision + recal))
    return {'dist1': mean_to_trgt, 'dist2': mean_to_pred, 'prec': precision, 'recal': recal, 'fscore': fscore}
