"""Shared by the morphable-model tests (test_morphable_host.py, test_gpu_morphable.py, morphable_worker.py,
golden/make_bfm_golden.py): inputs from a closed-form integer hash (identical on every machine, nothing large committed), the
float64 restatements of the node and of param2points_bfm, and the derived error bound."""
import numpy as np
import torch

BFM_V, BFM_SHAPE, BFM_EXP, BFM_POSE = 53215, 199, 29, 7
BFM_R, BFM_K = 3 * BFM_V, BFM_SHAPE + BFM_EXP


def hash_grid(rows, cols, salt):
    """[rows, cols] int64 in [0, 65521): ((r 1315423911 + k 2654435761 + salt 97531) mod 65521)"""
    r = np.arange(rows, dtype=np.int64)[:, None]
    k = np.arange(cols, dtype=np.int64)[None, :]
    return (r * 1315423911 + k * 2654435761 + np.int64(salt) * 97531) % 65521


def hashed_ints(rows, cols, salt, lo, hi):
    """int64 [rows, cols] in [lo, hi]: which of the hi - lo + 1 equal parts of [0, 65521) the hash falls in (a staircase of
    the hash, so that two such arrays along one axis correlate and their sums of products grow with the length)"""
    return hash_grid(rows, cols, salt) * (hi - lo + 1) // 65521 + lo


def hashed_floats(rows, cols, salt, lo=-1.0, hi=1.0, dtype=np.float32):
    """[rows, cols] in [lo, hi]: the hash as a fraction of 65520, computed in float64 and rounded once"""
    return (lo + (hi - lo) * (hash_grid(rows, cols, salt).astype(np.float64) / 65520.0)).astype(dtype)


def restate_rows(coeffs, basis, mean=None, scale=None):
    """d3m_morphable_forward in float64 torch: coeffs [B,K] (or [K]), basis [R,K], any R -> [B,R] (or [R])"""
    c = coeffs.double()
    if scale is not None:
        c = c * scale.double().reshape(-1)
    out = c @ basis.double().reshape(-1, basis.shape[-1]).T
    if mean is not None:
        out = out + mean.double().reshape(-1)
    return out


def restate_node(coeffs, basis, mean=None, scale=None):
    """morphable_vertices in float64 torch: coeffs [B,K] (or [K]), basis [3V,K] -> [B,V,3] (or [V,3])"""
    return restate_rows(coeffs, basis, mean, scale).reshape(*coeffs.shape[:-1], -1, 3)


def restate_param2points(shape_param, exp_param, other_param, preds):
    """param2points_bfm (deep3dmap/core/all3dmm/bfm_tools.py:4-20) term for term, in the dtype of its inputs, with the
    vertex count from w instead of the literal 53215"""
    alpha = preds[:, :199].reshape(-1, 199, 1) * shape_param['sigma'].reshape(1, 199, 1)
    beta = preds[:, 199:228].reshape(-1, 29, 1) * 1.0 / (1000.0 * other_param['sigma_exp'].reshape(1, 29, 1))
    w, w_exp, mu = shape_param['w'], exp_param['w_exp'], shape_param['mu_shape']
    face = torch.matmul(w[None], alpha) + torch.matmul(w_exp[None], beta) + mu.reshape(1, -1, 1)
    return [face.reshape(-1, w.shape[0] // 3, 3), preds[:, 228:235]]


def abs_terms(coeffs, basis, mean=None, scale=None):
    """sum of the absolute terms behind every output of the node, float64: [B,R]"""
    c = coeffs.double().reshape(-1, coeffs.shape[-1]).abs()
    if scale is not None:
        c = c * scale.double().reshape(-1).abs()
    s = c @ basis.double().reshape(-1, basis.shape[-1]).abs().T
    if mean is not None:
        s = s + mean.double().reshape(-1).abs()
    return s


def bound(n, abs_sum):
    """|fl(sum of n terms) - sum| <= (n + 3) 2^-24 sum|terms| for ANY order of the additions: a chain of at most n additions
    gives gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms, 4.2), every term is a product
    that carries at most three more roundings (scale * coeff, the product with the basis, grad_scale), u = 2^-24, and the
    (n + 3)^2 u^2 remainder is below the slack of counting three roundings where the kernels spend one or two."""
    return (n + 3) * 2.0 ** -24 * abs_sum


def bfm_inputs(dtype=torch.float32, device="cpu", batch=2):
    """The dictionaries of param2points_bfm at Basel size from the hash, and preds [batch, 235]."""
    t = lambda a: torch.from_numpy(a).to(dtype).to(device)       # noqa: E731
    shape_param = {'w': t(hashed_floats(BFM_R, BFM_SHAPE, 1, dtype=np.float64)),
                   'sigma': t(hashed_floats(1, BFM_SHAPE, 2, 0.5, 1.5, np.float64)[0]),
                   'mu_shape': t(hashed_floats(BFM_R, 1, 3, -100.0, 100.0, np.float64))}
    exp_param = {'w_exp': t(hashed_floats(BFM_R, BFM_EXP, 4, dtype=np.float64))}
    other_param = {'sigma_exp': t(hashed_floats(1, BFM_EXP, 5, 0.0005, 0.0015, np.float64)[0])}
    preds = t(hashed_floats(batch, BFM_K + BFM_POSE, 6, -2.0, 2.0, np.float64))
    return shape_param, exp_param, other_param, preds


def bfm_sample_vertices(n=2048):
    """n vertex indices in [0, BFM_V) from the hash (ascending, distinct)"""
    picks = np.unique((hash_grid(4 * n, 1, 7)[:, 0] * 7919 + np.arange(4 * n) * 104729) % BFM_V)
    assert picks.size >= n
    step = picks.size / n
    return picks[(np.arange(n) * step).astype(np.int64)]
