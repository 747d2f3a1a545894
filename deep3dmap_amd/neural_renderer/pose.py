"""The weak-perspective pose of a point set: `pose_vertices` (one autograd node, differentiable with respect to the vertices
and the pose) and `PoseHead` (the landmark indices and the constants as a module).

    a = clamp(pose[b, 1:4], -angle_limit, +angle_limit)        R_b = Rx(a0) Ry(a1) Rz(a2)   (core.renderer_pt3d.euler_xyz_to_matrix)
    posed[b, v] = pose[b, 0] * (R_b vertices[v]) + translation_scale * pose[b, 4:7]
    uv[b, v]    = (posed_x / uv_size, 1 - posed_y / uv_size)
    landmarks[b, l] = posed[b, landmark_index[l]]

d3m_pose_forward is one launch, d3m_pose_backward at most two, with no float atomics and a fixed tree for the 12 sums per set
(M_b = sum_v G (x) x, n_b = sum_v G) behind grad_pose: workgroup p of a set's num_parts(V) takes the vertices
VERTICES_PER_CHUNK * p + lane, then every VERTICES_PER_CHUNK * parts further, in ascending order per lane; the 64 lanes of a
wave are added as a butterfly, the four waves in wave order; a second launch adds a set's partials in ascending p, then the
landmark terms in ascending l, and applies the Euler adjoint, FINISH_SETS sets per workgroup.  The landmark gradients reach
grad_vertices in ascending l (with shared vertices: summed over the sets in ascending order first), so repeated indices are
neither a race nor an order left open.  The one thing cached is a landmark tensor's range-checked int32 form, in a
built_cache.BuiltCache (so a captured step keeps the form it reads), and nothing synchronises after that check: the node can
be captured once its landmark tensor has been seen."""
from collections import namedtuple

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from .. import _lib
from .built_cache import BuiltCache, tensor_key

# the constants of csrc/d3m_pose.h that fix the summation tree
VERTICES_PER_CHUNK = 256        # lanes of a workgroup, one vertex each per stride (PS_BLOCK)
MAX_PARTS = 64                  # workgroups per set; beyond VERTICES_PER_CHUNK * MAX_PARTS vertices the lanes stride (PS_MAX_PARTS)
FINISH_SETS = 64                # sets per workgroup of the second launch, one per lane (PS_FINISH_SETS)
SUMS = 12                       # M_b row-major (9) and n_b (3) (PS_SUMS)
WAVES_PER_CHUNK = VERTICES_PER_CHUNK // 64
MAX_SETS, MAX_LANDMARKS = 4096, 1024
CACHE_SIZE = 8

PosedPoints = namedtuple("PosedPoints", ["posed", "uv", "landmarks"])


class LandmarkCache(BuiltCache):
    """BuiltCache of range-checked landmark tensors: the payload is the int32 form the kernels read, the holder the tensor."""
    what = "pose_vertices: the landmark tensor's range check (its int32 form)"


_checked_landmarks = LandmarkCache(CACHE_SIZE)


def num_parts(num_vertices):
    return max(1, min(MAX_PARTS, (int(num_vertices) + VERTICES_PER_CHUNK - 1) // VERTICES_PER_CHUNK))


def pose_chain(num_vertices, num_landmarks=0):
    """The longest chain of additions behind one of a set's 12 sums: a lane's vertices, the butterfly of a wave (6 levels),
    the waves of a workgroup, the set's partials, the landmark terms."""
    parts = num_parts(num_vertices)
    per_lane = (int(num_vertices) + parts * VERTICES_PER_CHUNK - 1) // (parts * VERTICES_PER_CHUNK)
    return per_lane + 6 + WAVES_PER_CHUNK + parts + int(num_landmarks)


def vertex_chain(sets_summed=1, landmark_hits=0):
    """The same for one element of grad_vertices: the three gradients into G, the three products of R^T G, the sets of
    shared vertices, the landmark gradients that point at the vertex (each itself summed over the sets when shared)."""
    return 2 + 2 + int(sets_summed) + int(landmark_hits) * (1 + (int(sets_summed) if sets_summed > 1 else 0))


def forward(vertices, pose, translation_scale=1.0, angle_limit=None, uv_size=None, landmarks=None, posed=True):
    """d3m_pose_forward on checked device tensors: vertices [1 or B,V,3] contiguous, pose [B,7] with unit column stride,
    landmarks int32 [L] or None.  Returns (posed [B,V,3] or None, uv [B,V,2] or None, landmark points [B,L,3] or None)."""
    vb, V = vertices.shape[0], vertices.shape[1]
    B = pose.shape[0]
    dev = vertices.device
    L = 0 if landmarks is None else landmarks.numel()
    o_posed = torch.empty(B, V, 3, dtype=torch.float32, device=dev) if posed else None
    o_uv = torch.empty(B, V, 2, dtype=torch.float32, device=dev) if uv_size else None
    o_lm = torch.empty(B, L, 3, dtype=torch.float32, device=dev) if L else None
    _lib.check(_lib.lib().d3m_pose_forward(_lib.ptr(vertices), vb, _lib.ptr(pose), pose.stride(0) if B > 1 else 7,
                                           float(translation_scale), float(angle_limit or 0.0), float(uv_size or 0.0),
                                           _lib.ptr(landmarks), L, _lib.ptr(o_posed), _lib.ptr(o_uv), _lib.ptr(o_lm), B, V,
                                           _lib.stream_ptr()), "d3m_pose_forward")
    return o_posed, o_uv, o_lm


def backward(vertices, pose, grad_posed=None, grad_uv=None, grad_landmarks=None, translation_scale=1.0, angle_limit=None,
             uv_size=None, landmarks=None, need_vertices=True, need_pose=True):
    """d3m_pose_backward on the tensors of `forward` and contiguous f32 gradients of its outputs (None: zeros).  Returns
    (grad_vertices [1 or B,V,3] or None, grad_pose [B,7] or None)."""
    vb, V = vertices.shape[0], vertices.shape[1]
    B = pose.shape[0]
    dev = vertices.device
    L = 0 if landmarks is None else landmarks.numel()
    g_v = torch.empty(vb, V, 3, dtype=torch.float32, device=dev) if need_vertices else None
    g_p = torch.empty(B, 7, dtype=torch.float32, device=dev) if need_pose else None
    lib = _lib.lib()
    n = int(lib.d3m_pose_scratch_floats(B, V)) if need_pose else 0
    scratch = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
    _lib.check(lib.d3m_pose_backward(_lib.ptr(vertices), vb, _lib.ptr(pose), pose.stride(0) if B > 1 else 7,
                                     float(translation_scale), float(angle_limit or 0.0), float(uv_size or 0.0),
                                     _lib.ptr(landmarks), L, _lib.ptr(grad_posed), _lib.ptr(grad_uv), _lib.ptr(grad_landmarks),
                                     _lib.ptr(scratch), n, _lib.ptr(g_v), _lib.ptr(g_p), B, V, _lib.stream_ptr()),
               "d3m_pose_backward")
    return g_v, g_p


def _landmark_vector(landmarks, what="landmarks"):
    if not torch.is_tensor(landmarks):
        raise ValueError(f"{what} must be a tensor")
    if landmarks.dtype not in (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8) or landmarks.dim() != 1:
        raise ValueError(f"{what} must be an integer vector [L] (found {landmarks.dtype}, {tuple(landmarks.shape)})")
    if not 1 <= landmarks.numel() <= MAX_LANDMARKS:
        raise ValueError(f"1 to {MAX_LANDMARKS} landmarks (found {landmarks.numel()})")


def _landmarks_in_range(landmarks, num_vertices):
    """The int32 form of a landmark tensor whose entries lie in [0, V): looked at once per (tensor, V), by address and
    version, and the only step of the node that reads device memory on the host."""
    def check():
        lo, hi = int(landmarks.min()), int(landmarks.max())
        if lo < 0 or hi >= num_vertices:
            raise ValueError(f"landmarks must lie in [0, {num_vertices}) (found {lo} to {hi})")
        return landmarks.detach().to(torch.int32).contiguous()
    return _checked_landmarks.get(tensor_key(landmarks) + (int(num_vertices),), check, holders=(landmarks,))


def _positive_or_none(value, name):
    if value is None:
        return None
    value = float(value)
    if not value > 0.0:
        raise ValueError(f"{name} must be positive or None (found {value})")
    return value


def _checked(vertices, pose, angle_limit, uv_size, landmarks):
    """The arguments as the kernels read them: (vertices [1 or B,V,3], pose [B,7], angle_limit, uv_size, landmarks int32 or
    None, batched).  Dtypes, ranks and shapes are judged before the device, so those errors show without one."""
    for name, t in (("vertices", vertices), ("pose", pose)):
        if not torch.is_tensor(t):
            raise ValueError(f"{name} must be a tensor")
        if t.dtype != torch.float32:
            raise ValueError(f"{name} must be float32 (found {t.dtype})")
    if pose.dim() not in (1, 2) or pose.shape[-1] != 7:
        raise ValueError(f"pose must be [7] or [B, 7] (found {tuple(pose.shape)})")
    batched = pose.dim() == 2
    B = pose.shape[0] if batched else 1
    if not 1 <= B <= MAX_SETS:
        raise ValueError(f"1 to {MAX_SETS} poses per call (found {B})")
    if vertices.dim() not in (2, 3) or vertices.shape[-1] != 3 or vertices.shape[-2] < 1:
        raise ValueError(f"vertices must be [V, 3] or [B, V, 3] (found {tuple(vertices.shape)})")
    if vertices.dim() == 3 and not batched:
        raise ValueError("vertices [B, V, 3] need a pose [B, 7]")
    if vertices.dim() == 3 and vertices.shape[0] not in (1, B):
        raise ValueError(f"vertices has {vertices.shape[0]} sets, pose {B}")
    V = vertices.shape[-2]
    if B * V * 3 >= 2 ** 31:
        raise ValueError("B * V * 3 must stay below 2^31")
    angle_limit, uv_size = _positive_or_none(angle_limit, "angle_limit"), _positive_or_none(uv_size, "uv_size")
    if landmarks is not None:
        _landmark_vector(landmarks)
    for name, t in (("vertices", vertices), ("pose", pose), ("landmarks", landmarks)):
        if t is not None and not t.is_cuda:
            raise ValueError(f"{name} must be on the GPU device (found {t.device})")
        if t is not None and t.device != vertices.device:
            raise ValueError(f"{name} is on {t.device}, vertices on {vertices.device}")
    if landmarks is not None:
        landmarks = _landmarks_in_range(landmarks, V)
    return vertices, pose, angle_limit, uv_size, landmarks, batched


def _rows(pose):
    """pose [B,7] as the kernels read it in place: unit column stride, rows at least 7 floats apart (else a copy)"""
    if pose.stride(1) != 1 or (pose.shape[0] > 1 and pose.stride(0) < 7):
        return pose.contiguous()
    return pose


def _grad(g, shape):
    return None if g is None else g.to(torch.float32).reshape(shape).contiguous()


class _Pose(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vertices, pose, landmarks, translation_scale, angle_limit, uv_size, want_posed, batched):
        ctx.set_materialize_grads(False)
        v = (vertices if vertices.dim() == 3 else vertices[None]).contiguous()
        p = _rows(pose if batched else pose[None])
        posed, uv, lm = forward(v, p, translation_scale, angle_limit, uv_size, landmarks, want_posed)
        ctx.save_for_backward(v, p, landmarks)
        ctx.consts = (translation_scale, angle_limit, uv_size)
        ctx.shapes = (tuple(vertices.shape), batched)
        if not batched:
            posed, uv, lm = (None if t is None else t[0] for t in (posed, uv, lm))
        return posed, uv, lm

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_posed, grad_uv, grad_landmarks):
        need_v, need_p = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if (grad_posed is None and grad_uv is None and grad_landmarks is None) or not (need_v or need_p):
            return (None,) * 8
        v, p, landmarks = ctx.saved_tensors
        tau, limit, uv_size = ctx.consts
        shape, batched = ctx.shapes
        B, V = p.shape[0], v.shape[1]
        L = 0 if landmarks is None else landmarks.numel()
        g_v, g_p = backward(v, p, _grad(grad_posed, (B, V, 3)), _grad(grad_uv, (B, V, 2)), _grad(grad_landmarks, (B, L, 3)),
                            tau, limit, uv_size, landmarks, need_v, need_p)
        if g_v is not None:
            g_v = g_v.reshape(shape)
        if g_p is not None and not batched:
            g_p = g_p[0]
        return (g_v, g_p) + (None,) * 6


def pose_vertices(vertices, pose, translation_scale=1.0, angle_limit=None, uv_size=None, landmarks=None, posed=True):
    """The weak-perspective pose of `vertices` as the named tuple PosedPoints(posed, uv, landmarks).

    vertices f32 [V,3] (shared by every pose) or [B,V,3]; pose f32 [7] or [B,7] = (scale, three XYZ Euler angles, translation),
    read in place when its rows are a strided view such as preds[:, 228:235]; translation_scale multiplies the translation
    (the reference passes its image size); angle_limit clamps the angles to +-angle_limit (None: no clamp; the gradient
    flows at the limit itself, as torch.clamp's); uv_size adds uv [B,V,2] = (x / uv_size, 1 - y / uv_size) (None: uv is
    None); landmarks, an integer vector [L] of vertex indices that may repeat, adds the rows posed[:, landmarks] [B,L,3]
    (None: None); posed=False leaves posed [B,V,3] out (None) -- with only landmarks the work is O(B L).  A pose [7] gives
    outputs without the leading B.

    One autograd node, differentiable in vertices and pose (grad_pose is dense [B,7]); an output nobody used costs nothing
    in backward, a gradient nobody needs is not computed, and the sums have the fixed order the module text describes.
    ValueError, before the device is touched, for a wrong dtype, rank, device or shape; landmark indices outside [0, V) raise
    ValueError on the first call with that tensor (the one host read; inside a stream capture a RuntimeError)."""
    vertices, pose, angle_limit, uv_size, landmarks, batched = _checked(vertices, pose, angle_limit, uv_size, landmarks)
    if not posed and uv_size is None and landmarks is None:
        raise ValueError("posed=False leaves nothing to compute without uv_size or landmarks")
    return PosedPoints(*_Pose.apply(vertices, pose, landmarks, float(translation_scale), angle_limit, uv_size, bool(posed),
                                    batched))


class PoseHead(nn.Module):
    """pose_vertices with its constants and landmark indices held: `landmarks` (an integer vector, list or array, or None)
    becomes an int32 buffer, checked for negative entries here and against the vertex count on the first call.
    forward(vertices, pose) returns PosedPoints(posed, uv, landmarks)."""

    def __init__(self, landmarks=None, translation_scale=1.0, angle_limit=None, uv_size=None):
        super().__init__()
        if landmarks is not None:
            landmarks = torch.as_tensor(landmarks).detach()
            _landmark_vector(landmarks, "PoseHead: landmarks")
            if int(landmarks.min()) < 0:
                raise ValueError(f"PoseHead: landmarks must not be negative (found {int(landmarks.min())})")
            if int(landmarks.max()) >= 2 ** 31:
                raise ValueError("PoseHead: landmarks beyond int32")
            landmarks = landmarks.to(torch.int32).contiguous().clone()
        self.register_buffer("landmarks", landmarks)
        self.translation_scale = float(translation_scale)
        self.angle_limit = _positive_or_none(angle_limit, "PoseHead: angle_limit")
        self.uv_size = _positive_or_none(uv_size, "PoseHead: uv_size")

    def forward(self, vertices, pose):
        return pose_vertices(vertices, pose, self.translation_scale, self.angle_limit, self.uv_size, self.landmarks)
