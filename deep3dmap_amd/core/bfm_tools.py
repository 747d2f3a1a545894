"""Mirror of deep3dmap/core/all3dmm/bfm_tools.py: `param2points_bfm`, the face vertices of Basel-face-model coefficients
(models/frameworks/imgs2mesh.py:78 calls it right before Pt3dRenderer.sample), on nr.morphable_vertices."""
import torch

from ..neural_renderer.built_cache import BuiltCache, tensor_key
from ..neural_renderer.morphable import morphable_vertices

N_SHAPE, N_EXP, N_POSE = 199, 29, 7     # the columns of preds: identity | expression | pose
CACHE_SIZE = 4


class _BasisCache(BuiltCache):
    what = "param2points_bfm: the basis w | w_exp"


class _ScaleCache(BuiltCache):
    what = "param2points_bfm: the scale sigma | 1 / (1000 sigma_exp)"


# (w, w_exp) / (sigma, sigma_exp) by address and version -> what the node reads, built once per pair; an entry holds the pair
_bases, _scales = _BasisCache(CACHE_SIZE), _ScaleCache(CACHE_SIZE)


def _basis(w, w_exp):
    return _bases.get((tensor_key(w), tensor_key(w_exp)), lambda: torch.cat([w, w_exp], 1).contiguous(), holders=(w, w_exp))


def _scale(sigma, sigma_exp):
    return _scales.get((tensor_key(sigma), tensor_key(sigma_exp)),
                       lambda: torch.cat([sigma.reshape(-1), 1.0 / (1000.0 * sigma_exp.reshape(-1))]).contiguous(),
                       holders=(sigma, sigma_exp))


def param2points_bfm(shape_param, exp_param, other_param, preds):
    """bfm_tools.py:4-20 with the same dictionaries and keys: shape_param['w'] [3V,199], ['sigma'] [199], ['mu_shape']
    [3V,1]; exp_param['w_exp'] [3V,29]; other_param['sigma_exp'] [29]; preds [B, >= 228] (f32, on the device).  Returns
    [face_shape [B,V,3], preds[:, 228:235]] with

        face_shape = w (preds[:, :199] sigma) + w_exp (preds[:, 199:228] / (1000 sigma_exp)) + mu_shape

    as ONE morphable_vertices node: basis w | w_exp and scale sigma | 1 / (1000 sigma_exp), each built once per pair of
    tensors (their address and version) and kept in a BuiltCache (a captured step keeps what it reads), mean mu_shape.
    The gradient reaches preds only: a model tensor that requires grad raises NotImplementedError, as the node does.  The
    reference hard-codes reshape(-1, 53215, 3); this uses V = w.shape[0] // 3, the same number for the Basel model."""
    w, w_exp = shape_param['w'], exp_param['w_exp']
    sigma, mu_shape, sigma_exp = shape_param['sigma'], shape_param['mu_shape'], other_param['sigma_exp']
    if w.dim() != 2 or w_exp.dim() != 2 or w.shape[0] != w_exp.shape[0]:
        raise ValueError("param2points_bfm: w [3V, n] and w_exp [3V, m] must have the same rows")
    n, m = w.shape[1], w_exp.shape[1]
    if preds.dim() != 2 or preds.shape[1] < n + m:
        raise ValueError(f"param2points_bfm: preds must be [B, >= {n + m}]")
    for name, t in (("w", w), ("w_exp", w_exp), ("sigma", sigma), ("mu_shape", mu_shape), ("sigma_exp", sigma_exp)):
        if t.requires_grad:
            raise NotImplementedError(f"param2points_bfm: the gradient with respect to {name} is not computed (detach it; "
                                      "only preds is differentiable)")
    if preds.dtype != torch.float32 or w.dtype != torch.float32 or w_exp.dtype != torch.float32:
        raise ValueError("param2points_bfm: preds, w and w_exp must be float32")
    if not (preds.is_cuda and w.device == preds.device and w_exp.device == preds.device):
        raise ValueError("param2points_bfm: preds, w and w_exp must be on the GPU device, all on one")
    face_shape = morphable_vertices(preds[:, :n + m], _basis(w, w_exp), mu_shape.reshape(-1), _scale(sigma, sigma_exp))
    return [face_shape, preds[:, n + m:n + m + N_POSE]]
