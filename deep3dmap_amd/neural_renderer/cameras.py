"""Camera / viewpoint transforms of neural_renderer, each a single HIP pass with an analytic adjoint
(d3m_camera_forward / d3m_camera_backward in include/d3m_raster.h).

Reference (NR = pnpmodules/neural_renderer/neural_renderer): NR/look_at.py:6-62, NR/look.py:6-53,
NR/perspective.py:6-21, NR/projection.py:6-43, NR/get_points_from_angles.py:6-24.
"""
import ctypes
import math

import torch

from .. import _lib
from ._util import as_device_f32, const_tensor, f32c


class _CameraFunction(torch.autograd.Function):
    """vertices [Bv,V,3] -> [B,V,3].  `params` is a parameter block (look_at_params & co); the block's parameter tensors
    (camera_inputs) follow as autograd inputs, so that backward returns their gradients (d3m_camera_params_backward) beside
    the vertices' (d3m_camera_backward)."""

    @staticmethod
    def forward(ctx, vertices, params, *inputs):
        v = f32c(vertices)
        B = params["batch"]
        cam, keep = _camera_struct(params, v.device)
        out = torch.empty(B, v.shape[1], 3, dtype=torch.float32, device=v.device)
        rc = _lib.lib().d3m_camera_forward(_lib.ptr(v), v.shape[0], ctypes.byref(cam), _lib.ptr(out), B, v.shape[1],
                                           _lib.stream_ptr())
        _lib.check(rc, "d3m_camera_forward")
        ctx.save_for_backward(v)
        ctx.params, ctx.keep = params, keep
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (v,) = ctx.saved_tensors
        params = ctx.params
        g = f32c(grad_out)
        cam, keep = _camera_struct(params, v.device)
        gv = None
        if ctx.needs_input_grad[0]:
            gv = torch.empty_like(v)
            rc = _lib.lib().d3m_camera_backward(_lib.ptr(v), v.shape[0], ctypes.byref(cam), _lib.ptr(g), _lib.ptr(gv),
                                                params["batch"], v.shape[1], _lib.stream_ptr())
            _lib.check(rc, "d3m_camera_backward")
        n = len(ctx.needs_input_grad) - 2          # (perspective() has no parameter tensors)
        return (gv, None) + (params_backward(params, v, g, ctx.needs_input_grad[2:])[:n] if n else ())


def _camera_struct(p, device):
    cam = _lib.D3MCamera()
    cam.mode = p["mode"]
    cam.perspective = int(bool(p.get("perspective", False)))
    cam.tan_half_width = float(p.get("width", 1.0))
    cam.orig_size = float(p.get("orig_size", 1.0))
    keep = []
    for field, key in (("rot", "rot"), ("eye_or_t", "eye_or_t"), ("K", "K"), ("dist", "dist")):
        t = p.get(key)
        if t is not None:
            keep.append(t)
            setattr(cam, field, t.data_ptr())
            setattr(cam, field + "_batch" if field != "eye_or_t" else "eye_batch", t.shape[0])
    return cam, keep


# The parameter tensors of a block in the order of d3m_camera_grad's fields: the autograd inputs of _CameraFunction and of
# the render nodes that run the camera inside (rasterize._RasterizeLit, _RasterizeMeshModes).
CAMERA_INPUTS = ("eye_or_t", "at_or_direction", "up", "rot", "K", "dist")


def camera_inputs(p):
    """the six parameter tensors of block `p` (CAMERA_INPUTS; None where the mode has none).  look / look_at: eye, at or
    direction, up (the basis rows are computed from them); projection: t, R, K, dist."""
    if p["mode"] == _lib.CAMERA_PROJECTION:
        return (p["eye_or_t"], None, None, p["rot"], p["K"], p["dist"])
    eye, at_or_dir, up, _ = p["vectors"]
    return (eye, at_or_dir, up, None, None, None)


def camera_learnable(p):
    """whether any parameter of block `p` requires grad"""
    return p is not None and any(t is not None and t.requires_grad for t in camera_inputs(p))


def params_backward(p, vertices, grad_screen, needs, stream=None):
    """the gradients of block `p`'s parameters (camera_inputs order; None where `needs` is False) from grad_screen [B,V,3],
    the gradient of the camera's output, on vertices [Bv,V,3] (one fixed-order reduction: d3m_camera_params_backward).  The
    block's basis rows must hold the basis of its vectors (the forward pass left them there).  Allocated on the current
    stream; launched on `stream` (default: the current one)."""
    needs = tuple(bool(n) for n in tuple(needs)[:6]) + (False,) * max(0, 6 - len(needs))
    if not any(needs):
        return (None,) * 6
    ins = camera_inputs(p)
    grads = [torch.empty_like(t) if (t is not None and need) else None for t, need in zip(ins, needs)]
    L = _lib.lib()
    dev = vertices.device
    cam, keep = _camera_struct(p, dev)
    basis, bkeep = basis_struct(p, "vectors")
    gs = _lib.D3MCameraGrad(*[_lib.ptr(g) for g in grads])
    B, V = p["batch"], vertices.shape[1]
    ws = torch.empty(int(L.d3m_camera_params_backward_workspace_bytes(B, V, p["mode"])), dtype=torch.uint8, device=dev)
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(dev)):
        _lib.check(L.d3m_camera_params_backward(_lib.ptr(vertices), vertices.shape[0], ctypes.byref(cam),
                                                ctypes.byref(basis) if basis is not None else None, _lib.ptr(grad_screen),
                                                ctypes.byref(gs), B, V, _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
                   "d3m_camera_params_backward")
    return tuple(grads)


def _projection_torch(vertices, K, R, t, dist, orig_size, eps):
    """projection.py:19-43 as one differentiable device-side composition: projection() with a non-default eps (the fused
    kernels have the reference's 1e-9 built in)."""
    cam = torch.einsum('bvk,bjk->bvj', vertices, R) + t.reshape(-1, 1, 3)
    z = cam[..., 2]
    xn, yn = cam[..., 0] / (z + eps), cam[..., 1] / (z + eps)
    k1, k2, p1, p2, k3 = (dist[:, None, i] for i in range(5))
    r2 = torch.sqrt(xn ** 2 + yn ** 2) ** 2
    radial = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    xd = xn * radial + 2 * p1 * xn * yn + p2 * (r2 + 2 * xn ** 2)
    yd = yn * radial + p1 * (r2 + 2 * yn ** 2) + 2 * p2 * xn * yn
    pix = torch.einsum('bvk,bjk->bvj', torch.stack((xd, yd, torch.ones_like(z)), dim=-1), K)
    u, v = pix[..., 0], orig_size - pix[..., 1]
    return torch.stack((2 * (u - orig_size / 2.) / orig_size, 2 * (v - orig_size / 2.) / orig_size, z), dim=-1)


def _tan_width(angle):
    # perspective.py:15-17: the angle is rounded to f32 before tan
    return float(torch.tan(torch.tensor(angle / 180 * math.pi, dtype=torch.float32)))


def _basis(eye, at_or_dir, up, is_look_at, batch, device):
    """rows (x, y, z) of the camera frame, computed on the device (d3m_camera_basis)."""
    rot = torch.empty(batch, 3, 3, dtype=torch.float32, device=device)
    rc = _lib.lib().d3m_camera_basis(_lib.ptr(eye), eye.shape[0], _lib.ptr(at_or_dir), at_or_dir.shape[0],
                                     _lib.ptr(up), up.shape[0], int(is_look_at), _lib.ptr(rot), batch,
                                     _lib.stream_ptr())
    _lib.check(rc, "d3m_camera_basis")
    return rot


def camera_param(name, x, inner, device):
    """One camera parameter as a float32 device tensor [n, *inner] -- a differentiable reshape of the caller's tensor, so
    that its gradient comes back in the caller's shape.  Accepted: [*inner] (n = 1), [n, *inner], and [n, 1, *inner] (t of
    projection.py); anything else raises ValueError."""
    t = as_device_f32(x, device)
    k = len(inner)
    shape = tuple(t.shape)
    ok = shape[len(shape) - k:] == tuple(inner) and (len(shape) == k or len(shape) == k + 1
                                                     or (len(shape) == k + 2 and shape[1] == 1))
    if not ok:
        raise ValueError(f"camera {name} must be {list(inner)} or one per view [B,{','.join(map(str, inner))}]; "
                         f"got shape {list(shape)}")
    return t.reshape(-1, *inner).contiguous()


def _batch_of(vertices, named):
    """the batch of a camera: the vertices' or the parameters' (1 or B each); another batch raises ValueError"""
    B = max([vertices.shape[0]] + [t.shape[0] for t in named.values()])
    for name, t in list(named.items()) + [("vertices", vertices)]:
        if t.shape[0] not in (1, B):
            raise ValueError(f"camera: {name} has batch {t.shape[0]}; the others make {B} views (1 or {B} expected)")
    return B


def _look_block(vertices, mode, eye, target, up, is_look_at, _perspective_angle, defer_basis):
    device = vertices.device
    eye_t = camera_param("eye", eye, (3,), device)
    tgt_t = camera_param("at" if is_look_at else "direction", target, (3,), device)
    up_t = camera_param("up", up, (3,), device)
    batch = _batch_of(vertices, {"eye": eye_t, "at" if is_look_at else "direction": tgt_t, "up": up_t})
    nb = max(eye_t.shape[0], tgt_t.shape[0], up_t.shape[0])
    p = dict(mode=mode, batch=batch, eye_or_t=eye_t, perspective=_perspective_angle is not None,
             width=_tan_width(_perspective_angle) if _perspective_angle is not None else 1.0,
             vectors=(eye_t, tgt_t, up_t, is_look_at))
    if defer_basis:
        p["rot"] = torch.empty(nb, 3, 3, dtype=torch.float32, device=device)
        p["basis"] = p["vectors"]
    else:
        with torch.no_grad():
            p["rot"] = _basis(eye_t, tgt_t, up_t, is_look_at, nb, device)
    return p


def look_at_params(vertices, eye, at=[0, 0, 0], up=[0, 1, 0], _perspective_angle=None, defer_basis=False):
    """The fused camera kernels' parameter block of look_at(vertices, eye, at, up) -- for callers that run
    d3m_camera_forward / _backward inside a larger node (rasterize._RasterizeLit).  Parameters that require grad stay
    differentiable (camera_inputs; their gradient: params_backward).  defer_basis: the frame is NOT computed here
    (d3m_camera_basis, a launch of its own) but by the caller's d3m_lit_front, which leaves it in `rot`: the block then
    carries the vectors it is made of (`basis`).  Shapes [3] or [B,3]; another batch raises ValueError."""
    return _look_block(vertices, _lib.CAMERA_LOOK_AT, eye, at, up, True, _perspective_angle, defer_basis)


def basis_struct(p, key="basis"):
    """(D3MBasis, tensors to keep alive) of a parameter block made with defer_basis (key "basis"), or of the vectors of any
    look / look_at block (key "vectors"), else (None, [])"""
    b = p.get(key)
    if b is None:
        return None, []
    eye, at, up, is_look_at = b
    return _lib.D3MBasis(eye.data_ptr(), at.data_ptr(), up.data_ptr(), eye.shape[0], at.shape[0], up.shape[0],
                         int(bool(is_look_at))), [eye, at, up]


def look_at(vertices, eye, at=[0, 0, 0], up=[0, 1, 0], _perspective_angle=None):
    """"Look at" transformation of vertices (NR/look_at.py:6-62).
    `eye`, `at`, `up`: list / tuple / ndarray / tensor of shape [3] or [batch, 3]; tensors that require grad get it."""
    if vertices.ndimension() != 3:
        raise ValueError('vertices Tensor should have 3 dimensions')
    params = look_at_params(vertices, eye, at, up, _perspective_angle)
    return _CameraFunction.apply(vertices, params, *camera_inputs(params))


def look(vertices, eye, direction=[0, 1, 0], up=None, _perspective_angle=None):
    """"Look" transformation of vertices (NR/look.py:6-53); `up` defaults to [0, 1, 0]."""
    if vertices.ndimension() != 3:
        raise ValueError('vertices Tensor should have 3 dimensions')
    params = look_params(vertices, eye, direction, up, _perspective_angle)
    return _CameraFunction.apply(vertices, params, *camera_inputs(params))


def look_params(vertices, eye, direction=[0, 1, 0], up=None, _perspective_angle=None, defer_basis=False):
    """look()'s parameter block (see look_at_params)."""
    return _look_block(vertices, _lib.CAMERA_LOOK, eye, direction, [0, 1, 0] if up is None else up, False,
                       _perspective_angle, defer_basis)


def perspective(vertices, angle=30.):
    """Perspective distortion x,y /= z*tan(angle) (NR/perspective.py:6-21)."""
    if vertices.ndimension() != 3:
        raise ValueError('vertices Tensor should have 3 dimensions')
    device = vertices.device
    params = dict(mode=_lib.CAMERA_LOOK_AT, batch=vertices.shape[0],
                  rot=const_tensor([[1, 0, 0], [0, 1, 0], [0, 0, 1]], device, (1, 3, 3)),
                  eye_or_t=const_tensor([0, 0, 0], device, (1, 3)), perspective=True, width=_tan_width(angle))
    return _CameraFunction.apply(vertices, params)


def projection(vertices, K, R, t, dist_coeffs, orig_size, eps=1e-9):
    """Projective transformation with lens distortion (NR/projection.py:6-43).
    K [b,3,3], R [b,3,3], t [b,1,3] (or [b,3]), dist_coeffs [b,5]; b is 1 or the batch size."""
    params = projection_params(vertices, K, R, t, dist_coeffs, orig_size)
    if eps != 1e-9:      # the fused kernels have the reference's default eps built in
        batch = params["batch"]
        return _projection_torch(vertices.float().expand(batch, -1, -1), params["K"].expand(batch, 3, 3),
                                 params["rot"].expand(batch, 3, 3), params["eye_or_t"].expand(batch, 3),
                                 params["dist"].expand(batch, 5), float(orig_size), eps)
    return _CameraFunction.apply(vertices, params, *camera_inputs(params))


def projection_params(vertices, K, R, t, dist_coeffs, orig_size):
    """projection()'s parameter block (default eps).  Parameters that require grad stay differentiable (camera_inputs);
    K / R [3,3] or [B,3,3], t [3], [B,3] or [B,1,3], dist_coeffs [5] or [B,5]; another batch raises ValueError."""
    device = vertices.device
    tt = camera_param("t", t, (3,), device)
    rot, Kt, dist = (camera_param("R", R, (3, 3), device), camera_param("K", K, (3, 3), device),
                     camera_param("dist_coeffs", dist_coeffs, (5,), device))
    batch = _batch_of(vertices, {"t": tt, "R": rot, "K": Kt, "dist_coeffs": dist})
    return dict(mode=_lib.CAMERA_PROJECTION, batch=batch, rot=rot, eye_or_t=tt, K=Kt, dist=dist, orig_size=float(orig_size))


def get_points_from_angles(distance, elevation, azimuth, degrees=True):
    """Spherical -> cartesian eye position (NR/get_points_from_angles.py:6-24).  Host-side scalar form, or
    tensor form ([n] tensors -> [n,3])."""
    if isinstance(distance, (float, int)):
        if degrees:
            elevation, azimuth = math.radians(elevation), math.radians(azimuth)
        return (distance * math.cos(elevation) * math.sin(azimuth), distance * math.sin(elevation),
                -distance * math.cos(elevation) * math.cos(azimuth))
    if degrees:
        elevation, azimuth = math.pi / 180. * elevation, math.pi / 180. * azimuth
    return torch.stack([distance * torch.cos(elevation) * torch.sin(azimuth), distance * torch.sin(elevation),
                        -distance * torch.cos(elevation) * torch.cos(azimuth)]).transpose(1, 0)
