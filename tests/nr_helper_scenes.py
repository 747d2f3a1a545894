"""Shared by the tests of NrRenderer's helper kernels (test_nr_helpers_host.py, test_gpu_nr_helpers.py): the case tables, the
hashed inputs (no RNG state) and ONE statement of each operation, written from the comments above each kernel in
csrc/d3m_aux.h and at the end of csrc/d3m_g2s.h, in the kernel's order and association, generic over the arithmetic:

  F64   numpy float64: the restatement the float cases are compared with;
  F32   numpy float32 arrays, one operation at a time: the library is built with -ffp-contract=off, so where no intermediate
        rounds (inputs that are small integers and dyadic fractions) this gives the same bits as F64 -- that agreement, asserted
        at every output element by the host file, DEFINES an exact case, and the GPU test then demands equal bits;
  ERR   float64 values that carry a bound of |fl32(v) - v| in units of u = 2^-24 (class Err).

THE BOUND.  Every operation of the restatement rounds once: it adds |v| to the bound of its result, and the bounds of its
operands reach the result through the absolute values of the operation's partial derivatives (first order; Higham, Accuracy
and Stability of Numerical Algorithms, 3.3).  Summed over the path of an element this is "the absolute values of the terms that
enter the element, once per rounding on their way", term by term and never more than (number of roundings) x (sum of the
absolute terms).  A sum of n terms in ANY order (lanes, waves, LDS, atomics) adds chain x sum|terms| (Higham 4.2), with the chain
from the restated launcher arithmetic.  The device's sinf / cosf are ASSUMED to be within TRIG_ULP = 4 ulp (no HIP math accuracy
table is installed beside the compiler to take the figure from), that is a relative error of at most 2 TRIG_ULP u each -- the
assumption and the wording of tests/pose_scenes.py.  The tolerance of an element is MARGIN x bound x u with MARGIN = 4, the
integer factor of tests/test_param_reductions_host.py (FloatReference.tolerance: "4 * e32"); it covers the second-order
terms.  Nothing here is fitted to what the kernels return.

Conventions the kernels state and the restatement keeps: the normals' adjoint uses c = 0 where |n| = 0 (torch autograd of
n / (|n| + eps) gives NaN there: d|n|/dn is 0/0); a sampling position that is not finite makes every tap out of bounds and the
output 0 (torch.nn.functional.grid_sample returns NaN for a NaN position on the CPU: not compared)."""
import functools
import math
from collections import namedtuple

import numpy as np

from morphable_scenes import hash_grid, hashed_floats, hashed_ints      # noqa: F401

U = 2.0 ** -24
TRIG_ULP = 4            # assumed: see above
MARGIN = 4              # tests/test_param_reductions_host.py, FloatReference.tolerance
DN_EPS = float(np.float32(1e-7))        # csrc/d3m_aux.h
CUBE = np.array([[0.5, 0.5, 0.5], [0., 0., 1.], [0., 1., 0.], [-0.5, 0.5, 0.5],
                 [1., 0., 0.], [0.5, -0.5, 0.5], [0.5, 0.5, -0.5], [0., 0., 0.]])


# ---- the three arithmetics --------------------------------------------------------------------------------------------------
class Err:
    """v (float64) with e >= |fl32(v) - v| / u to first order; an input that float32 holds exactly has e = 0"""
    __array_ufunc__ = None

    def __init__(self, v, e=None):
        self.v = np.asarray(v, np.float64)
        self.e = np.zeros_like(self.v) if e is None else np.broadcast_to(np.asarray(e, np.float64), self.v.shape)

    @staticmethod
    def lift(x):
        return x if isinstance(x, Err) else Err(x)

    @staticmethod
    def _rounded(v, e):
        return Err(v, e + np.abs(v))

    def __add__(self, o):
        o = Err.lift(o)
        return Err._rounded(self.v + o.v, self.e + o.e)

    __radd__ = __add__

    def __sub__(self, o):
        o = Err.lift(o)
        return Err._rounded(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return Err.lift(o) - self

    def __mul__(self, o):
        o = Err.lift(o)
        return Err._rounded(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Err.lift(o)
        with np.errstate(divide="ignore", invalid="ignore"):
            v = self.v / o.v
            return Err._rounded(v, (self.e + np.abs(v) * o.e) / np.abs(o.v))

    def __rtruediv__(self, o):
        return Err.lift(o) / self

    def __neg__(self):
        return Err(-self.v, self.e)

    def __getitem__(self, i):
        return Err(self.v[i], self.e[i])

    @property
    def shape(self):
        return self.v.shape

    def reshape(self, *s):
        return Err(self.v.reshape(*s), self.e.reshape(*s))


def val(x):
    return x.v if isinstance(x, Err) else np.asarray(x)


def lift(a, ar):
    """an input array in the arithmetic `ar` ("f64", "f32", "err"); float32 must hold it exactly"""
    a = np.asarray(a, np.float64)
    assert np.array_equal(a.astype(np.float32).astype(np.float64), a, equal_nan=True), "an input is not a float32"
    return Err(a) if ar == "err" else a.astype(np.float32 if ar == "f32" else np.float64)


def _like(x, a):
    """the constant array `a` in the arithmetic of x"""
    return Err(a) if isinstance(x, Err) else np.asarray(a, val(x).dtype)


def sqrt_(x):
    if isinstance(x, Err):
        v = np.sqrt(x.v)
        with np.errstate(divide="ignore", invalid="ignore"):
            return Err._rounded(v, np.where(v > 0, x.e / (2 * np.where(v > 0, v, 1)), np.sqrt(x.e * U) / U))
    return np.sqrt(x)


def trig_(x):
    """(cos, sin): float64 and Err only (the bits of sinf / cosf are not predicted)"""
    if isinstance(x, Err):
        c, s = np.cos(x.v), np.sin(x.v)
        return Err(c, 2 * TRIG_ULP * np.abs(c) + np.abs(s) * x.e), Err(s, 2 * TRIG_ULP * np.abs(s) + np.abs(c) * x.e)
    return np.cos(x), np.sin(x)


def where_(cond, a, b):
    if isinstance(a, Err) or isinstance(b, Err):
        a, b = Err.lift(a), Err.lift(b)
        return Err(np.where(cond, a.v, b.v), np.where(cond, a.e, b.e))
    return np.where(cond, a, np.asarray(b, a.dtype) if isinstance(a, np.ndarray) else b)


def stack_(xs, axis=-1):
    if any(isinstance(x, Err) for x in xs):
        xs = [Err.lift(x) for x in xs]
        return Err(np.stack([x.v for x in xs], axis), np.stack([x.e for x in xs], axis))
    return np.stack(xs, axis)


def pad_(x, axes):
    """one zero either side of each axis of `axes`"""
    width = [(1, 1) if a in axes else (0, 0) for a in range(len(x.shape))]
    return Err(np.pad(x.v, width), np.pad(x.e, width)) if isinstance(x, Err) else np.pad(x, width)


def take_(x, idx):
    """x [B, N] gathered at idx [B, M] along the last axis"""
    if isinstance(x, Err):
        return Err(np.take_along_axis(x.v, idx, 1), np.take_along_axis(x.e, idx, 1))
    return np.take_along_axis(x, idx, 1)


def sum_(x, axis, chain):
    """a sum whose order is not stated: exact arithmetic for F64; for Err `chain` roundings of the sum of the absolute terms;
    for F32 numpy's own order (only meaningful where the terms make every order exact: exact_sum_proven)"""
    if isinstance(x, Err):
        return Err(x.v.sum(axis), x.e.sum(axis) + chain * np.abs(x.v).sum(axis))
    return x.sum(axis, dtype=x.dtype)


def exact_sum_proven(terms, axis=None, total=None):
    """every partial sum of `terms`, in any order, is a float32: the terms are multiples of one power of two q and the sum of
    their absolute values (`total`, where the terms fall into groups that are summed apart: the largest group's) stays below
    2^24 q"""
    t = np.asarray(terms, np.float64)
    nz = np.abs(t[t != 0])
    if nz.size == 0:
        return True
    q = 2.0 ** (np.frexp(nz)[1].min() - 25)          # 24 bits below the smallest term's leading bit: every f32 term is a multiple
    for k in range(60):                               # the coarsest grid all terms lie on
        if not np.array_equal(np.round(t / (q * 2)), t / (q * 2)):
            break
        q *= 2
    return bool((np.asarray(np.abs(t).sum(axis) if total is None else total) / q < 2 ** 24).all())


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def same_bits(a, b):
    """a (float32) and b (float64) agree bit for bit once b is rounded -- and b does not round"""
    a, b = np.asarray(a), np.asarray(b, np.float64)
    b32 = b.astype(np.float32)
    return a.dtype == np.float32 and a.shape == b.shape and np.array_equal(b32.astype(np.float64), b, equal_nan=True) and \
        np.array_equal(bits(a), bits(b32))


def tolerance(e):
    return MARGIN * U * np.asarray(e, np.float64)


# ---- pieces shared by the kernels (gw_ray, gw_rigid, gw_project, cam_ptr) ---------------------------------------------------------
def _entry(M, B):
    """cam_ptr: the matrix of every batch entry [B, n] from [B, n] or [1, n]"""
    assert M.shape[0] in (1, B)
    return M if M.shape[0] == B else M[np.zeros(B, np.int64)]


def _col(M, k):
    return M[:, k:k + 1]


def ray_(iK, x, y):
    """gw_ray: x * iK[3k] + y * iK[3k+1] + iK[3k+2]; iK [B,9], x / y [N] or [B,N]"""
    return [x * _col(iK, 3 * k) + y * _col(iK, 3 * k + 1) + _col(iK, 3 * k + 2) for k in range(3)]


def rigid_(p, R, t, cz):
    """gw_rigid: p is shifted to the rotation centre (returned), q = R p' + (0, 0, cz) + t"""
    p = [p[0], p[1], p[2] - cz]
    q = [p[0] * _col(R, 0) + p[1] * _col(R, 1) + p[2] * _col(R, 2) + _col(t, 0),
         p[0] * _col(R, 3) + p[1] * _col(R, 4) + p[2] * _col(R, 5) + _col(t, 1),
         p[0] * _col(R, 6) + p[1] * _col(R, 7) + p[2] * _col(R, 8) + cz + _col(t, 2)]
    return p, q


def project_(q, K, W, H, swap_wh=False):
    """gw_project: normalised coordinates of a W x H image"""
    if swap_wh:
        W, H = H, W
    xn, yn = q[0] / q[2], q[1] / q[2]
    u = xn * _col(K, 0) + yn * _col(K, 1) + _col(K, 2)
    v = xn * _col(K, 3) + yn * _col(K, 4) + _col(K, 5)
    return [u / float(W - 1) * 2.0 - 1.0, v / float(H - 1) * 2.0 - 1.0]


def pixel_xy(H, W, like):
    pix = np.arange(H * W)
    return _like(like, pix % W), _like(like, pix // W)


def project_adjoint_(g_u, g_v, q, K, W, H, variant=None):
    """the adjoint of gw_project as both backward kernels write it: (g_u, g_v) are the gradients of (uv0, uv1) already
    divided as the kernel divides them -> g_q"""
    if variant == "swap_wh":
        W, H = H, W
    gu, gv = g_u / float(W - 1), g_v / float(H - 1)
    if variant == "drop_K13":
        gxn, gyn = gu * _col(K, 0), gv * _col(K, 4)
    else:
        gxn, gyn = gu * _col(K, 0) + gv * _col(K, 3), gu * _col(K, 1) + gv * _col(K, 4)
    iz = 1.0 / q[2]
    return [gxn * iz, gyn * iz, -(gxn * q[0] + gyn * q[1]) * iz * iz]


def motion_adjoint_(gq, p, ray, R):
    """g_q -> (g_depth [B,N], the twelve per-pixel terms of (g_A, g_t) [12][B,N])"""
    gp = [gq[0] * _col(R, j) + gq[1] * _col(R, 3 + j) + gq[2] * _col(R, 6 + j) for j in range(3)]
    g_depth = gp[0] * ray[0] + gp[1] * ray[1] + gp[2] * ray[2]
    terms = [gq[k] * p[j] for k in range(3) for j in range(3)] + [gq[k] for k in range(3)]
    return g_depth, terms


# ---- d3m_view_transform / _backward -----------------------------------------------------------------------------------------------
def _mat3_mul(a, b):
    """(a0 b0 + a1 b1) + a2 b2 per entry; a, b lists of nine [B]"""
    return [(a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j] for i in range(3) for j in range(3)]


def _euler(view):
    (cx, sx), (cy, sy), (cz, sz) = (trig_(view[:, k]) for k in range(3))
    one, nil = _like(view, np.ones(view.shape[0])), _like(view, np.zeros(view.shape[0]))
    mx = [one, nil, nil, nil, cx, -sx, nil, sx, cx]
    my = [cy, nil, sy, nil, one, nil, -sy, nil, cy]
    mz = [cz, -sz, nil, sz, cz, nil, nil, nil, one]
    dx = [nil, nil, nil, nil, -sx, -cx, nil, cx, -sx]
    dy = [-sy, nil, cy, nil, nil, nil, -cy, nil, -sy]
    dz = [-sz, -cz, nil, cz, -sz, nil, nil, nil, nil]
    return (mx, my, mz), (dx, dy, dz)


def view_transform(view):
    """view [B, 3|5|6] -> (R = Rz (Ry Rx) [B,9], t [B,3] padded with zeros)"""
    B, n = view.shape
    (mx, my, mz), _ = _euler(view)
    R = _mat3_mul(mz, _mat3_mul(my, mx))
    nil = _like(view, np.zeros(B))
    return stack_(R, 1), stack_([view[:, 3 + k] if 3 + k < n else nil for k in range(3)], 1)


def view_transform_backward(view, g_rot, g_trans):
    """g_view [B, n]: <g_rot, dR/d(rx, ry, rz)>, then g_trans; None stands for zeros"""
    B, n = view.shape
    (mx, my, mz), (dx, dy, dz) = _euler(view)
    nil = _like(view, np.zeros(B))
    g = [g_rot[:, k] if g_rot is not None else nil for k in range(9)]
    out = []
    for d in (_mat3_mul(mz, _mat3_mul(my, dx)), _mat3_mul(mz, _mat3_mul(dy, mx)), _mat3_mul(dz, _mat3_mul(my, mx))):
        acc = nil
        for k in range(9):
            acc = acc + g[k] * d[k]
        out.append(acc)
    out += [g_trans[:, k - 3] if g_trans is not None else nil for k in range(3, n)]
    return stack_(out, 1)


# ---- d3m_grid_warp / _backward -------------------------------------------------------------------------------------------------------
def grid_warp(depth, inv_K, A, t, cz, K=None, crop=None, H=None, W=None, variant=None):
    """depth [B,HW], inv_K / K [1|B,9], A [B,9], t [B,3] -> [B,HW,3], or with K [B,HW,2]; crop (top, bottom, left, right)"""
    B = depth.shape[0]
    stride = (lambda M: M[:1]) if variant == "entry0" else (lambda M: M)
    iK = _entry(stride(inv_K), B)
    x, y = pixel_xy(H, W, depth)
    top, bottom, left, right = crop or (0, 0, 0, 0)
    xi, yi = np.arange(H * W) % W, np.arange(H * W) // W
    ry, cx = np.clip(yi, top, H - 1 - bottom), np.clip(xi, left, W - 1 - right)
    fry, fcx = _like(depth, ry), _like(depth, cx)
    # x from (y, cx), y from (ry, x), z from (ry, cx)
    p = [ray_(iK, fcx, y)[0] * depth[:, yi * W + cx], ray_(iK, x, fry)[1] * depth[:, ry * W + xi],
         ray_(iK, fcx, fry)[2] * depth[:, ry * W + cx]]
    _, q = rigid_(p, A, t, cz)
    if K is None:
        return stack_(q, 2)
    return stack_(project_(q, _entry(stride(K), B), W, H, variant == "swap_wh"), 2)


def grid_warp_backward(depth, inv_K, A, t, cz, K, g_out, H, W, variant=None):
    """(g_depth [B,HW], per-pixel terms of g_A (nine) and g_t (three), each [B,HW]); g_out [B,HW,3] or [B,HW,2]"""
    B = depth.shape[0]
    stride = (lambda M: M[:1]) if variant == "entry0" else (lambda M: M)
    iK = _entry(stride(inv_K), B)
    x, y = pixel_xy(H, W, depth)
    ray = ray_(iK, x, y)
    p, q = rigid_([ray[k] * depth for k in range(3)], A, t, cz)
    if K is None:
        gq = [g_out[:, :, k] for k in range(3)]
    else:
        gq = project_adjoint_(g_out[:, :, 0] * 2.0, g_out[:, :, 1] * 2.0, q, _entry(stride(K), B), W, H, variant)
    return motion_adjoint_(gq, p, ray, A)


def reduce_terms(terms, chain, skip=None):
    """the sums over the pixels of the twelve terms -> [B,12]; `skip` = a slice of pixels left out (a wrong variant)"""
    keep = slice(None) if skip is None else np.r_[0:skip.start, skip.stop:terms[0].shape[1]]
    return stack_([sum_(x[:, keep], 1, chain) for x in terms], 1)


# ---- d3m_depth_normals / _backward --------------------------------------------------------------------------------------------------
def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _tangents(depth, inv_K, H, W):
    B = depth.shape[0]
    x, y = pixel_xy(H, W, depth)
    ray = ray_(_entry(inv_K, B), x, y)
    P = [(ray[k] * depth).reshape(B, H, W) for k in range(3)]
    tu = [c[:, 1:-1, 2:] - c[:, 1:-1, :-2] for c in P]
    tv = [c[:, 2:, 1:-1] - c[:, :-2, 1:-1] for c in P]
    return ray, tu, tv


def depth_normals(depth, inv_K, H, W):
    """depth [B,HW] -> normals [B,H,W,3]: n / (|n| + eps) inside, (0, 0, 1) / (1 + eps) on the one-pixel border"""
    B = depth.shape[0]
    one, nil = _like(depth, np.ones((B, H, W))), _like(depth, np.zeros((B, H, W)))
    n = [nil, nil, one]
    if H > 2 and W > 2:
        _, tu, tv = _tangents(depth, inv_K, H, W)
        inside = np.zeros((B, H, W), bool)
        inside[:, 1:-1, 1:-1] = True
        n = [where_(inside, pad_(c, (1, 2)), b) for c, b in zip(_cross(tu, tv), n)]
    length = sqrt_(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]) + DN_EPS
    return stack_([c / length for c in n], 3)


def depth_normals_backward(depth, inv_K, g_normal, H, W, variant=None):
    """g_normal [B,H,W,3] -> g_depth [B,HW], gathered from the four neighbours; c = 0 where |n| = 0"""
    B = depth.shape[0]
    x, y = pixel_xy(H, W, depth)
    ray = ray_(_entry(inv_K, B), x, y)
    nil = _like(depth, np.zeros((B, H, W)))
    if not (H > 2 and W > 2):
        gp = [nil + nil, nil + nil, nil + nil]
    else:
        _, tu, tv = _tangents(depth, inv_K, H, W)
        n = _cross(tu, tv)
        norm = sqrt_(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
        length = norm + DN_EPS
        go = [g_normal[:, 1:-1, 1:-1, k] for k in range(3)]
        dot = go[0] * n[0] + go[1] * n[1] + go[2] * n[2]
        some = val(norm) > 0
        c = where_(some, dot / where_(some, length * length * norm, 1.0), 0.0)
        gn = [go[k] / length - n[k] * c for k in range(3)]
        # zero where the neighbour is on the border or outside the map: two cells of padding around the interior
        g_tu = [pad_(pad_(v, (1, 2)), (1, 2)) for v in _cross(tv, gn)]
        g_tv = [pad_(pad_(v, (1, 2)), (1, 2)) for v in _cross(gn, tu)]
        sl = lambda dy, dx: (slice(None), slice(1 + dy, 1 + dy + H), slice(1 + dx, 1 + dx + W))      # noqa: E731
        gp = []
        for k in range(3):
            acc = nil + g_tu[k][sl(0, -1)]                       # the right point of (y, x-1)
            acc = (acc + g_tu[k][sl(0, 1)]) if variant == "flip_sign" else (acc - g_tu[k][sl(0, 1)])     # the left point of (y, x+1)
            acc = acc + g_tv[k][sl(-1, 0)]                       # the lower point of (y-1, x)
            acc = acc - g_tv[k][sl(1, 0)]                        # the upper point of (y+1, x)
            gp.append(acc)
    gp = [c.reshape(B, H * W) for c in gp]
    return gp[0] * ray[0] + gp[1] * ray[1] + gp[2] * ray[2]


# ---- d3m_textures_from_im / _backward --------------------------------------------------------------------------------------------------
def textures_from_im(im, ts):
    """im [B,C,H,W] -> [B, 2 (H-1)(W-1), ts^3, C]: cell (y, x) holds the faces (im[y,x], im[y,x+1], im[y+1,x]) at
    n = y (W-1) + x and (im[y+1,x], im[y,x+1], im[y+1,x+1]) at n + (H-1)(W-1)"""
    B, C, H, W = im.shape
    tl, tr, bl, br = im[:, :, :-1, :-1], im[:, :, :-1, 1:], im[:, :, 1:, :-1], im[:, :, 1:, 1:]
    faces = [(tl, tr, bl), (bl, tr, br)]
    out = []
    for v in faces:
        if ts == 2:
            tex = [(float(CUBE[i][0]) * v[0] + float(CUBE[i][1]) * v[1]) + float(CUBE[i][2]) * v[2] for i in range(8)]
        else:
            tex = [v[0] if v is faces[0] else v[2]]
        out.append(np.stack(tex, -1).reshape(B, C, (H - 1) * (W - 1), len(tex)))         # [B,C,cells,per]
    return np.concatenate(out, 2).transpose(0, 2, 3, 1)


def textures_from_im_backward(g_tex, B, C, H, W, ts):
    """g_tex [B, 2 cells, per, C] -> g_im [B,C,H,W], gathered per pixel in the kernel's order of its (up to) six faces"""
    per = 8 if ts == 2 else 1
    g = g_tex.reshape(B, 2, H - 1, W - 1, per, C)
    g = np.pad(g, [(0, 0), (0, 0), (1, 1), (1, 1), (0, 0), (0, 0)])
    acc = np.zeros((B, C, H, W), g_tex.dtype)
    ys, xs = np.arange(H)[:, None], np.arange(W)[None, :]
    for second, dy, dx, slot in ((0, 0, 0, 0), (0, 0, -1, 1), (0, -1, 0, 2), (1, -1, 0, 0), (1, 0, -1, 1), (1, -1, -1, 2)):
        cell = g[:, second, ys + dy + 1, xs + dx + 1]             # [B,H,W,per,C]
        if ts == 2:
            for i in range(8):
                acc = acc + g_tex.dtype.type(CUBE[i][slot]) * cell[:, :, :, i].transpose(0, 3, 1, 2)
        elif slot == (2 if second else 0):
            acc = acc + cell[:, :, :, 0].transpose(0, 3, 1, 2)
    return acc


# ---- d3m_warp_resample / _backward ------------------------------------------------------------------------------------------------------
def resample_grid(depth, inv_K, K, A, t, cz, h, w, variant=None, W=None):
    """wr_grid of every output pixel: (ray, p, q, uv), lists of [B, h w]; the wrong variant "W_for_w" normalises by the source's
    width"""
    B = depth.shape[0]
    stride = (lambda M: M[:1]) if variant == "entry0" else (lambda M: M)
    x, y = pixel_xy(h, w, depth)
    ray = ray_(_entry(stride(inv_K), B), x, y)
    p, q = rigid_([ray[k] * depth for k in range(3)], A, t, cz)
    return ray, p, q, project_(q, _entry(stride(K), B), W if variant == "W_for_w" else w, h, variant == "swap_wh")


def pixel_position(uv, H, W):
    """F.grid_sample's pixel coordinates (align_corners = False) of the normalised position in an H x W source"""
    return ((uv[0] + 1.0) * float(W) - 1.0) / 2.0, ((uv[1] + 1.0) * float(H) - 1.0) / 2.0


def _taps(ix, iy, H, W):
    """the four taps (nw, ne, sw, se): plane offsets [4][B,N], validity, and the fractions; a position that is not finite or far
    outside has no valid tap"""
    with np.errstate(invalid="ignore"):
        flx, fly = np.floor(val(ix)), np.floor(val(iy))
        x0 = np.where((flx >= -2) & (flx <= W), flx, -2).astype(np.int64)
        y0 = np.where((fly >= -2) & (fly <= H), fly, -2).astype(np.int64)
    with np.errstate(invalid="ignore"):
        fx, fy = ix - _like(ix, flx), iy - _like(iy, fly)
    offs, ok = [], []
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        xx, yy = x0 + dx, y0 + dy
        v = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        ok.append(v)
        offs.append(np.where(v, yy * W + xx, 0))
    return offs, ok, fx, fy


def lookup_bilinear(src, ix, iy, H, W):
    """src [B,C,HW] at pixel positions [B,N] -> [B,C,N], zeros padding"""
    offs, ok, fx, fy = _taps(ix, iy, H, W)
    wts = [(1.0 - fx) * (1.0 - fy), fx * (1.0 - fy), (1.0 - fx) * fy, fx * fy]
    out = []
    for c in range(src.shape[1]):
        v = _like(ix, np.zeros(val(ix).shape))
        for k in range(4):
            v = v + where_(ok[k], take_(src[:, c], offs[k]) * wts[k], 0.0)
        out.append(v)
    return stack_(out, 1)


def lookup_nearest(src, ix, iy, H, W, rounding=np.rint):
    """half to even; zero outside the image and for a position that is not finite"""
    with np.errstate(invalid="ignore"):
        rx, ry = rounding(val(ix)), rounding(val(iy))
        inside = (rx >= 0) & (rx <= W - 1) & (ry >= 0) & (ry <= H - 1)
    off = np.where(inside, ry * W + rx, 0).astype(np.int64)
    return np.stack([np.where(inside, np.take_along_axis(val(src[:, c]), off, 1), 0) for c in range(src.shape[1])], 1)


def warp_resample(depth, inv_K, K, A, t, cz, src, src_nearest, h, w, H, W, variant=None):
    """-> (out [B,C,hw], out_nearest [B,Cn,hw] or None, (ix, iy))"""
    _, _, _, uv = resample_grid(depth, inv_K, K, A, t, cz, h, w, variant, W)
    ix, iy = pixel_position(uv, H, W)
    return lookup_bilinear(src, ix, iy, H, W), None if src_nearest is None else lookup_nearest(src_nearest, ix, iy, H, W), (ix, iy)


def warp_resample_backward(depth, inv_K, K, A, t, cz, src, g_out, h, w, H, W, variant=None):
    """-> (g_src contributions (offs [4][B,N], ok, values [C][4][B,N]), g_depth [B,hw], the twelve per-pixel terms)"""
    ray, p, q, uv = resample_grid(depth, inv_K, K, A, t, cz, h, w, variant, W)
    ix, iy = pixel_position(uv, H, W)
    offs, ok, fx, fy = _taps(ix, iy, H, W)
    wts = [(1.0 - fx) * (1.0 - fy), fx * (1.0 - fy), (1.0 - fx) * fy, fx * fy]
    gix = giy = _like(ix, np.zeros(val(ix).shape))
    contrib = []
    for c in range(src.shape[1]):
        gc = g_out[:, c]
        tap = [where_(ok[k], take_(src[:, c], offs[k]), 0.0) for k in range(4)]
        contrib.append([wts[k] * gc for k in range(4)])
        gix = gix + gc * ((tap[1] - tap[0]) * (1.0 - fy) + (tap[3] - tap[2]) * fy)
        giy = giy + gc * ((tap[2] - tap[0]) * (1.0 - fx) + (tap[3] - tap[1]) * fx)
    w_norm = W if variant == "W_for_w" else w
    g_u, g_v = gix * float(W) / 2.0 * 2.0, giy * float(H) / 2.0 * 2.0
    gq = project_adjoint_(g_u, g_v, q, _entry(K[:1] if variant == "entry0" else K, depth.shape[0]), w_norm, h, variant)
    g_depth, terms = motion_adjoint_(gq, p, ray, A)
    return (offs, ok, contrib), g_depth, terms


def scatter_src(contrib, B, C, HW, prefill=None, dtype=np.float64):
    """grad_src += : the contributions added into [B,C,HW] (numpy's order: only for terms that make every order exact, or in
    float64); returns (sum, sum of the absolute values)"""
    offs, ok, vals = contrib
    out = np.zeros((B, C, HW), dtype) if prefill is None else np.array(prefill, dtype).reshape(B, C, HW)
    mag = np.abs(out).astype(np.float64)
    rows = np.arange(B)[:, None]
    for c in range(C):
        for k in range(4):
            v = np.where(ok[k], val(vals[c][k]), 0)
            np.add.at(out[:, c], (rows, offs[k]), v.astype(dtype))
            np.add.at(mag[:, c], (rows, offs[k]), np.abs(v).astype(np.float64))
    return out, mag


def resample_partials(terms, parts):
    """the per-workgroup sums [B, parts, 12]: workgroup j owns the pixels j 256 + lane + m 256 parts"""
    N = val(terms[0]).shape[1]
    owner = (np.arange(N) // 256) % parts
    chain = strided_passes(N, parts)[1] + 6 + 3
    return stack_([stack_([sum_(x[:, owner == j], 1, chain) for x in terms], 1) for j in range(parts)], 1)


# ---- the launcher arithmetic (csrc/d3m_raster.hip), restated ------------------------------------------------------------------------------
def blocks_for(n, per=256):
    return (n + per - 1) // per


def grid_warp_split(B, HW):
    """workgroups per batch entry of k_grid_warp_backward: min(16, max(1, HW / 512)), halved while B split > 2048"""
    split = min(16, max(1, HW // 512))
    while split > 1 and B * split > 2048:
        split //= 2
    return split


def grid_warp_path(B, HW):
    split = grid_warp_split(B, HW)
    return "store" if split == 1 else "atomics"


def strided_passes(HW, split):
    """(fewest, most) passes of a lane of the backward kernels' strided loop"""
    per = 256 * split
    return HW // per, -(-HW // per)


def resample_parts(h, w):
    """d3m_warp_resample_partials: workgroups per batch entry, at most 32"""
    return min(32, max(1, blocks_for(h * w))) if h > 0 and w > 0 else 0


def reduce_chain(N, split):
    """the additions on the path of one of the (A, t) sums: a lane's strided passes, 6 DPP steps, 3 of the four waves, and the
    atomics of the other workgroups"""
    return strided_passes(N, split)[1] + 6 + 3 + (split - 1)


# ---- cases and inputs ---------------------------------------------------------------------------------------------------------------
GridCase = namedtuple("GridCase", "B H W kb crop kind")             # kb: batch count of inv_K and K; kind: exact | float | general
NormalCase = namedtuple("NormalCase", "B H W kind")                 # kind: float | zero_patch
TexCase = namedtuple("TexCase", "B C H W ts")
ViewCase = namedtuple("ViewCase", "B n kind")                       # kind: zero | quarter | hashed
ResampleCase = namedtuple("ResampleCase", "B h w H W C Cn kb kind")  # kind: exact | zoom | float | general


def case_id(c):
    return type(c).__name__[:-4].lower() + "-" + "-".join("x".join(map(str, v)) if isinstance(v, tuple) else str(v) for v in c)


GRID_SHAPES = ((1, 3, 3), (3, 5, 9), (3, 9, 17), (2, 17, 5))
GRID_CROPS = {(3, 5, 9): ((1, 0, 0, 0), (0, 2, 0, 0), (0, 0, 3, 0), (0, 0, 0, 2), (1, 1, 2, 3), (4, 0, 0, 8), (0, 4, 8, 0), (2, 2, 4, 4)),
              (2, 17, 5): ((3, 13, 1, 3),), (1, 3, 3): ((1, 1, 1, 1),)}
GRID_BACKWARD_SHAPES = ((1, 5, 9), (3, 17, 33), (2, 32, 32), (2, 17, 65), (2, 65, 129))       # HW = 45, 561, 1024, 1105, 8385
GRID_BACKWARD_LARGE_B = ((129, 65, 129), (2049, 17, 65))                                      # integer-exact only


def grid_forward_cases():
    out = []
    for s in GRID_SHAPES:
        for kb in sorted({1, s[0]}):
            out += [GridCase(*s, kb, None, kind) for kind in ("exact", "float")]
        out += [GridCase(*s, s[0], crop, "exact") for crop in GRID_CROPS.get(s, ())]
        out.append(GridCase(*s, s[0], None, "general"))
    return out


def grid_backward_cases():
    out = []
    for s in GRID_BACKWARD_SHAPES:
        out += [GridCase(*s, 1, None, "exact"), GridCase(*s, s[0], None, "float"), GridCase(*s, s[0], None, "general")]
    return out + [GridCase(*s, 1, None, "exact") for s in GRID_BACKWARD_LARGE_B]


NORMAL_SHAPES = ((1, 1, 7), (1, 7, 2), (2, 2, 2), (1, 3, 3), (2, 5, 9), (2, 9, 5), (3, 17, 33))


def normal_cases():
    return [NormalCase(*s, "float") for s in NORMAL_SHAPES] + [NormalCase(2, 9, 5, "zero_patch")]


def tex_cases():
    return [TexCase(*s, ts) for s in ((1, 1, 2, 2), (2, 3, 2, 7), (2, 3, 7, 2), (3, 4, 6, 7), (2, 3, 17, 9)) for ts in (1, 2)]


def view_cases():
    return [ViewCase(B, n, kind) for n in (3, 5, 6) for B in (1, 64, 65) for kind in ("zero", "quarter", "hashed")
            if kind == "hashed" or B == 65]


RESAMPLE_SHAPES = ((1, 2, 2, 3, 3), (2, 9, 17, 9, 17), (2, 9, 17, 5, 33), (3, 17, 5, 17, 5), (2, 16, 16, 16, 16), (2, 3, 129, 9, 9),
                   (1, 65, 129, 33, 33))


def resample_cases():
    out = []
    for i, s in enumerate(RESAMPLE_SHAPES):
        C, Cn = (1, 0) if i % 3 == 0 else ((3, 1) if i % 3 == 1 else (3, 2))
        out.append(ResampleCase(*s, C, Cn, 1, "exact"))
        out.append(ResampleCase(*s, 3 if C == 1 else 1, 2 if Cn == 0 else Cn, s[0], "float"))
    out.append(ResampleCase(2, 9, 17, 9, 17, 3, 1, 2, "zoom"))
    out.append(ResampleCase(2, 9, 17, 5, 33, 3, 1, 2, "general"))
    return out


def fov_matrices(H, W, fov=10.0):
    """NrRenderer's K and its inverse for a W x H image (renderer_nr.py:24-46), float32 values in float64"""
    fx = (W - 1) / 2 / math.tan(fov / 2 * math.pi / 180)
    fy = (H - 1) / 2 / math.tan(fov / 2 * math.pi / 180)
    K = np.array([[fx, 0, (W - 1) / 2], [0, fy, (H - 1) / 2], [0, 0, 1]], np.float32).astype(np.float64)
    return K.reshape(1, 9), np.linalg.inv(K).astype(np.float32).astype(np.float64).reshape(1, 9)


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def rotations_of(views):
    """float32 values of R = Rz (Ry Rx) for hashed views [B,3] (inputs of the kernels under test, not results of one)"""
    return _f32(view_transform(np.asarray(views, np.float64))[0])


SIGNED_PERMUTATIONS = (np.array([1, 0, 0, 0, 1, 0, 0, 0, 1.]), np.array([0, -1, 0, 1, 0, 0, 0, 0, 1.]), np.array([0, 0, 1, 0, -1, 0, 1, 0, 0.]),
                       np.array([1, 0.5, 0, 0, 1, 0, 0, -0.25, 1.]))


def grid_inputs(c, salt=0, threeD=True):
    """dict(depth [B,HW], inv_K, K [kb,9], A [B,9], t [B,3], cz, g3 [B,HW,3], g2 [B,HW,2]) as float64 arrays of float32 values"""
    B, H, W, HW = c.B, c.H, c.W, c.H * c.W
    if c.kind == "exact":
        # inv_K, K, A, t: small integers and dyadic fractions.  ray.z is 1 or 2, A's third row and column are (0, 0, 1) and t.z = 0, so
        # q.z = ray.z d is a power of two.  Gradients: small integers, the 2-D ones times the odd part of (W-1, H-1) so that
        # g 2 / (W-1) is exact; above 600 pixels the 2-D gradient is non-zero at the ends of the first 256-pixel runs and at the last
        # pixel only: a dense one's sums of gq p products are not multiples of one power of two within 24 bits (the 3-D gradient
        # and the float cases are dense at every shape)
        dense = HW <= 600
        depth = 2.0 ** hashed_ints(B, HW, 3 + salt, 0, 1)
        inv_K = np.array([[1, 0, -2, 0, 1, -1, 0, 0, 1.], [0.5, 0.5, 1, -0.5, 1, 0, 0, 0, 2.], [1, 0.5, 0, 0, 0.5, -3, 0, 0, 1.]])[np.arange(c.kb) % 3]
        K = np.array([[2, 1, 1, -1, 4, 2, 0, 0, 1.], [4, -2, 3, 1, 2, -1, 0, 0, 1.], [1, 2, 0, 3, -1, 4, 0, 0, 1.]])[np.arange(c.kb) % 3]
        A = np.array([[1, 0, 0, 0, 1, 0, 0, 0, 1.], [0, -1, 0, 1, 0, 0, 0, 0, 1.], [1, 0.5, 0, -0.25, 1, 0, 0, 0, 1.]])[np.arange(B) % 3]
        t = np.array([[0.5, -1, 0.], [-2, 0.25, 0.], [1, 1, 0.]])[np.arange(B) % 3]
        lim = 3 if dense else 1
        g3 = hashed_ints(B * HW, 3, 5 + salt, -lim, lim).reshape(B, HW, 3).astype(np.float64)
        odd = lambda n: n // (n & -n)          # noqa: E731
        g2 = hashed_ints(B * HW, 2, 6 + salt, -2, 2).reshape(B, HW, 2).astype(np.float64) * np.array([odd(W - 1), odd(H - 1)], np.float64)
        if not dense:
            keep = np.zeros(HW, bool)
            keep[[0, 255, 256, HW - 1]] = True
            g2 = g2 * keep[None, :, None]
        return dict(depth=depth, inv_K=inv_K, K=K, A=A, t=t, cz=1.0, g3=g3, g2=g2)
    depth = hashed_floats(B, HW, 3 + salt, 0.9, 1.1).astype(np.float64)
    K, inv_K = fov_matrices(H, W)
    if c.kind == "general" or c.kb > 1:
        # per-entry matrices; "general": skew and a full inverse (inv_K need not invert K for the kernels: they are two inputs)
        K = np.repeat(K, c.kb, 0) * (1 + 0.1 * hashed_floats(c.kb, 9, 7 + salt).astype(np.float64))
        inv_K = np.repeat(inv_K, c.kb, 0) * (1 + 0.1 * hashed_floats(c.kb, 9, 8 + salt).astype(np.float64))
        if c.kind == "general":
            K[:, 1], K[:, 3] = 0.3 * K[:, 0] * (1 + np.arange(c.kb)), -0.2 * K[:, 4] * (1 + np.arange(c.kb))
            inv_K[:, [1, 3]] = 0.4 * inv_K[:, [0, 4]] * np.array([1, -1])
            inv_K[:, 6:8] = 0.02 * hashed_floats(c.kb, 2, 9 + salt).astype(np.float64) / max(H, W)
    K, inv_K = _f32(K), _f32(inv_K)
    A = rotations_of(hashed_floats(B, 3, 10 + salt, -1.0, 1.0))
    t = hashed_floats(B, 3, 11 + salt, -0.1, 0.1).astype(np.float64)
    g3 = hashed_floats(B * HW, 3, 12 + salt).reshape(B, HW, 3).astype(np.float64)
    g2 = hashed_floats(B * HW, 2, 13 + salt).reshape(B, HW, 2).astype(np.float64)
    return dict(depth=depth, inv_K=inv_K, K=K, A=A, t=t, cz=float(np.float32(1.0)), g3=g3, g2=g2)


def normal_inputs(c):
    B, H, W = c.B, c.H, c.W
    depth = hashed_floats(B, H * W, 21, 0.9, 1.1).astype(np.float64)
    if c.kind == "zero_patch":
        d = depth.reshape(B, H, W)
        d[0, 2:5, 1:3] = 0.0            # (3, 1) and (3, 2): upper and lower point are zero, the left or right one is not: tv = 0, n = 0
        d[1, 4:7, 2] = 0.0
    _, inv_K = fov_matrices(max(H, 3), max(W, 3))
    inv_K = _f32(np.repeat(inv_K, B, 0) * (1 + 0.1 * hashed_floats(B, 9, 22).astype(np.float64)))
    inv_K[:, 6:8] = _f32(0.02 * hashed_floats(B, 2, 23) / max(H, W))
    g = hashed_floats(B * H * W, 3, 24).reshape(B, H, W, 3).astype(np.float64)
    return dict(depth=depth, inv_K=inv_K, g=g)


def tex_inputs(c):
    per = 8 if c.ts == 2 else 1
    im = hashed_ints(c.B * c.C, c.H * c.W, 31, -7, 7).reshape(c.B, c.C, c.H, c.W).astype(np.float64)
    g = hashed_ints(c.B * 2 * (c.H - 1) * (c.W - 1), per * c.C, 32, -5, 5).reshape(c.B, -1, per, c.C).astype(np.float64)
    return dict(im=im, g=g)


def view_inputs(c):
    if c.kind == "zero":
        view = np.zeros((c.B, c.n))
    elif c.kind == "quarter":
        q = float(np.float32(math.pi / 2))
        view = np.array([[0, q, -q][(b + k) % 3] for b in range(c.B) for k in range(c.n)]).reshape(c.B, c.n)
    else:
        view = hashed_floats(c.B, c.n, 41, -math.pi, math.pi).astype(np.float64)
    if c.n > 3:
        view[:, 3:] = hashed_ints(c.B, c.n - 3, 42, -4, 4) / 4.0
    g_rot = hashed_ints(c.B, 9, 43, -3, 3).astype(np.float64)
    g_trans = hashed_ints(c.B, 3, 44, -3, 3).astype(np.float64)
    return dict(view=view, g_rot=g_rot, g_trans=g_trans)


def nearest_clearance(c, inp):
    """the largest (tolerance of a pixel coordinate) / (its distance to the nearest k + 1/2): below 1, float32 rounds every
    position to the texel float64 does"""
    a = in_arith(inp, "err", ("depth", "inv_K", "K", "A", "t"))
    _, _, _, uv = resample_grid(a["depth"], a["inv_K"], a["K"], a["A"], a["t"], inp["cz"], c.h, c.w)
    worst = 0.0
    for p, n in zip(pixel_position(uv, c.H, c.W), (c.W, c.H)):
        worst = max(worst, float((tolerance(p.e) / np.abs(p.v - np.floor(p.v) - 0.5)).max()))
    return worst


@functools.lru_cache(maxsize=None)
def resample_inputs(c):
    """as _resample_inputs; the float cases with a nearest lookup take the first of the hashed inputs (salt 0, 1, ...) that keep
    every position clear of a rounding boundary"""
    for salt in range(16):
        inp = _resample_inputs(c, salt)
        if c.kind in ("exact", "zoom") or not c.Cn or nearest_clearance(c, inp) < 1:
            return inp
    raise AssertionError("no salt keeps the positions clear")


@functools.lru_cache(maxsize=None)
def _resample_inputs(c, salt):
    """dict(depth [B,hw], inv_K, K, A, t, cz, src [B,C,HW], src_n [B,Cn,HW] or None, g [B,C,hw], prefill [B,C,HW])"""
    B, h, w, H, W = c.B, c.h, c.w, c.H, c.W
    src_n = None if c.Cn == 0 else hashed_ints(B * c.Cn, H * W, 52, 1, 9).reshape(B, c.Cn, H * W).astype(np.float64)
    prefill = hashed_ints(B * c.C, H * W, 53, -3, 3).reshape(B, c.C, H * W).astype(np.float64)
    if c.kind in ("exact", "zoom"):
        # A = I, a dyadic translation, a constant power-of-two depth: u = s (x - cx + tx) + cu lands on a grid of quarters
        cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
        s = 0.25 if c.kind == "zoom" else 2.0
        odd = lambda n: n // (n & -n)          # noqa: E731
        depth = np.full((B, h * w), 2.0)
        inv_K = np.array([[1, 0, -cx, 0, 1, -cy, 0, 0, 1.]])
        # u = sx (x - cx + tx / 2) + cx with sx = s (w-1) / (the next power of two): u / (w-1) is dyadic whatever w is;
        # ix = u W / (w-1) - 1/2
        up = lambda n: n / 2.0 ** math.ceil(math.log2(n))          # noqa: E731
        K = np.array([[s * up(w - 1), 0, cx, 0, s * up(h - 1), cy, 0, 0, 1.]])
        A = np.repeat(SIGNED_PERMUTATIONS[0][None], B, 0)
        # entry 0 is not shifted (by a whole source row where h = 3): u W / (w-1) is then an integer at some pixels in both axes at
        # once, the positions exactly at k + 1/2; the other entries are shifted by dyadic fractions
        t = np.array([[0.0, 1.0 if h == 3 else 0.0, 0.0], [-1.0, 0.5, 0.0], [0.5, -0.25, 0.0]])[np.arange(B) % 3]
        if (h, w) == (2, 2):
            K, t = np.array([[1, 0, cx, 0, 1, cy, 0, 0, 1.]]), np.zeros((B, 3))       # u in {0, 1}: ix in {-1/2, W - 1/2}
        # the source: integers times the odd parts of (w-1, h-1), so that the adjoint's division by them is exact
        src = hashed_ints(B * c.C, H * W, 51, -8, 8).reshape(B, c.C, H * W).astype(np.float64) * (odd(w - 1) * odd(h - 1))
        g = hashed_ints(B * c.C, h * w, 54, -2, 2).reshape(B, c.C, h * w).astype(np.float64)
        inv_K, K = np.repeat(inv_K, c.kb, 0), np.repeat(K, c.kb, 0)
        return dict(depth=depth, inv_K=inv_K, K=K, A=A, t=t, cz=1.0, src=src, src_n=src_n, g=g, prefill=prefill)
    gc = GridCase(B, h, w, c.kb, None, c.kind)
    gi = grid_inputs(gc, salt=50 + 100 * salt)
    A = rotations_of(hashed_floats(B, 3, 55 + 100 * salt, -0.3, 0.3))
    src = hashed_floats(B * c.C, H * W, 51).reshape(B, c.C, H * W).astype(np.float64)
    g = hashed_floats(B * c.C, h * w, 54).reshape(B, c.C, h * w).astype(np.float64)
    return dict(depth=gi["depth"], inv_K=gi["inv_K"], K=gi["K"], A=A, t=gi["t"], cz=gi["cz"], src=src, src_n=src_n, g=g,
                prefill=prefill)


def in_arith(inp, ar, keys):
    return {k: (None if inp[k] is None else lift(inp[k], ar)) for k in keys}
