"""Shared by the tests of the section-B operators of include/d3m_raster.h (test_section_b_host.py, test_gpu_section_b.py): the
cameras (d3m_camera_basis / _forward / _backward / _backward_add), the gather, its scatter and the ordered gather
(d3m_gather_faces, d3m_scatter_face_grads, d3m_vertex_gather), lighting (d3m_lighting_forward / _backward, d3m_face_light) and the
output epilogue (d3m_output_epilogue / _backward).  The case tables, the seeded inputs and ONE statement of each operation,
written from csrc/d3m_aux.h in the kernel's order and association, generic over the arithmetic:

  "f64"  numpy float64: what the float cases are compared with;
  "f32"  numpy float32, one operation at a time (the library is built with -ffp-contract=off): E32 is measured on it, and it is the
         expectation of the exact cases;
  "abs"  class Abs: the float64 value together with the same expression with every term of every sum taken in absolute value -- the
         `bound` of the project's tolerance rule.

THE TOLERANCE is tests/test_param_reductions_host.py's (FloatReference.tolerance): (D 2^-24 + 4 E32) bound per element, with D the
longest chain of additions behind the element (stated beside each operator below), E32 the largest |f32 - f64| / bound of the
same case, and 4 the margin DESIGN section 2, pin 6 grants a kernel that associates a three-term dot product differently.  A
quotient's bound carries the divisor's own bound over its value (the amplification of a cancelled divisor).  Nothing is fitted
to what the kernels return.

Every named wrong variant (`variant=`) is one defect class of the issue; the host file shows that the comparison the GPU test
makes rejects each."""
import functools
import math
from collections import namedtuple

import numpy as np

from nr_helper_scenes import bits, exact_sum_proven, same_bits                       # noqa: F401

U = 2.0 ** -24
MARGIN = 4
EPS_N = float(np.float32(1e-5))          # F.normalize's eps as the kernels hold it (1e-5f)
ANGLE, ORIG_SIZE = 30.0, 256.0


# ---- the arithmetics ---------------------------------------------------------------------------------------------------------------
class Abs:
    """v (float64) and a >= |v|: the same expression with every term of every sum in absolute value"""
    __array_ufunc__ = None

    def __init__(self, v, a=None):
        self.v = np.asarray(v, np.float64)
        self.a = np.abs(self.v) if a is None else np.broadcast_to(np.asarray(a, np.float64), self.v.shape)

    @staticmethod
    def lift(x):
        return x if isinstance(x, Abs) else Abs(x)

    def __add__(self, o):
        o = Abs.lift(o)
        return Abs(self.v + o.v, self.a + o.a)

    __radd__ = __add__

    def __sub__(self, o):
        o = Abs.lift(o)
        return Abs(self.v - o.v, self.a + o.a)

    def __rsub__(self, o):
        return Abs.lift(o) - self

    def __mul__(self, o):
        o = Abs.lift(o)
        return Abs(self.v * o.v, self.a * o.a)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Abs.lift(o)
        with np.errstate(divide="ignore", invalid="ignore"):
            return Abs(self.v / o.v, np.where(o.v != 0, self.a * o.a / (o.v * o.v), np.inf))

    def __rtruediv__(self, o):
        return Abs.lift(o) / self

    def __neg__(self):
        return Abs(-self.v, self.a)

    def __getitem__(self, i):
        return Abs(self.v[i], self.a[i])

    @property
    def shape(self):
        return self.v.shape


def val(x):
    return x.v if isinstance(x, Abs) else np.asarray(x)


def lift(a, ar):
    """an input (float64 array of float32 values) in the arithmetic `ar`"""
    a = np.asarray(a, np.float64)
    assert np.array_equal(a.astype(np.float32).astype(np.float64), a), "an input is not a float32"
    return Abs(a) if ar == "abs" else a.astype(np.float32 if ar == "f32" else np.float64)


def sqrt_(x):
    return Abs(np.sqrt(x.v), np.sqrt(x.a)) if isinstance(x, Abs) else np.sqrt(x)


def fmax_(x, c):
    """max(x, c) for a constant c > 0"""
    if isinstance(x, Abs):
        return Abs(np.maximum(x.v, c), np.maximum(x.a, c))
    return np.maximum(x, x.dtype.type(c))


def where_(cond, a, b):
    if isinstance(a, Abs) or isinstance(b, Abs):
        a, b = Abs.lift(a), Abs.lift(b)
        return Abs(np.where(cond, a.v, b.v), np.where(cond, a.a, b.a))
    return np.where(cond, a, np.asarray(b, a.dtype))


def stack_(xs, axis=-1):
    if any(isinstance(x, Abs) for x in xs):
        xs = [Abs.lift(x) for x in xs]
        return Abs(np.stack(np.broadcast_arrays(*[x.v for x in xs]), axis), np.stack(np.broadcast_arrays(*[x.a for x in xs]), axis))
    return np.stack(np.broadcast_arrays(*xs), axis)


def sum_(x, axis):
    """a sum whose order the restatement does not state: exact in "f64"; sequential in "f32" (only E32 is taken from it)"""
    if isinstance(x, Abs):
        return Abs(x.v.sum(axis), x.a.sum(axis))
    if x.dtype == np.float32:
        x = np.moveaxis(x, axis, 0)
        acc = np.zeros(x.shape[1:], np.float32)
        for t in x:
            acc = acc + t
        return acc
    return x.sum(axis)


def tolerance(D, e32, bnd):
    return (D * U + MARGIN * e32) * np.asarray(bnd, np.float64)


def e32_of(f32, f64, bnd):
    """the largest |f32 - f64| / bound over the elements with a bound; an element without one must agree exactly"""
    f32, f64, bnd = (np.asarray(x, np.float64).reshape(-1) for x in (f32, f64, bnd))
    assert np.array_equal(f32[bnd == 0], f64[bnd == 0]), "an element without a bound differs between float32 and float64"
    return float((np.abs(f32 - f64)[bnd > 0] / bnd[bnd > 0]).max()) if (bnd > 0).any() else 0.0


def _rng(*seed):
    return np.random.default_rng([int(s) for s in seed])


def f32v(a):
    """float32 values, held in float64"""
    return np.asarray(a, np.float32).astype(np.float64)


def _entry(M, B):
    """cam_ptr: row b of a parameter of batch B, row 0 of one of batch 1"""
    M = np.asarray(M)
    assert M.shape[0] in (1, B), (M.shape, B)
    return M if M.shape[0] == B else np.repeat(M[:1], B, 0)


def case_id(c):
    return type(c).__name__[:-4].lower() + "-" + "-".join("".join(map(str, v)) if isinstance(v, tuple) else str(v) for v in c)


# ==== 1. cameras ====================================================================================================================
# mode: look_at | look | projection | none | perspective (perspective() alone: the identity frame, eye 0)
# vb: 1 = shared vertices; pb: the batch of each parameter (1 = batch 1, 0 stands for B) in the order of CAM_PARAMS[mode]
CamCase = namedtuple("CamCase", "mode persp B V vb pb")
CAM_PARAMS = {"look_at": ("rot", "eye"), "look": ("rot", "eye"), "perspective": ("rot", "eye"), "none": (),
              "projection": ("rot", "eye", "K", "dist")}
SHARED_B = (1, 2, 7, 8, 9, 16, 17, 33)
CAM_V = (1, 31, 32, 33, 257)
# D, the additions behind an element.  forward: v - e and a three-term dot (3), and for the projection the dot + t, + 1e-9, r2, the
# radial polynomial (3), the tangential terms (3), K (2), orig - v, u - orig / 2 (16).  adjoint: the forward's chain to z or to
# (x_, y_), then the products' sums and the transposed rotation (look 3 + 1 + 2; projection 16 + 4 + 1 + 1 + 2).
CAM_D = {"look_at": (3, 6), "look": (3, 6), "perspective": (3, 6), "none": (0, 0), "projection": (16, 24)}
BASIS_D = 9         # at - eye (1), three norms (2 each), two cross products (1 each)


def shared_D(B):
    """the shared route: a lane's ceil(B / 8) views, three DPP steps (the issue's figure)"""
    return -(-B // 8) + 3


def _all(n):
    return (0,) * n


def camera_cases():
    """per-view and shared vertices; every parameter alone at batch 1; every B and V of the issue for the shared route"""
    out = []
    for mode, persp in (("look_at", 1), ("look_at", 0), ("look", 1), ("look", 0), ("projection", 0), ("none", 0), ("perspective", 1)):
        n = len(CAM_PARAMS[mode])
        fixed = (1,) * n if mode == "perspective" else _all(n)
        out += [CamCase(mode, persp, 3, 33, 3, fixed), CamCase(mode, persp, 9, 33, 1, fixed)]
        if mode not in ("none", "perspective"):
            for k in range(n):          # parameter k alone at batch 1, per-view and shared vertices
                pb = tuple(int(j == k) for j in range(n))
                out += [CamCase(mode, persp, 3, 31, 3, pb), CamCase(mode, persp, 9, 32, 1, pb)]
            out.append(CamCase(mode, persp, 9, 33, 1, (1,) * n))
    for mode, persp in (("look_at", 1), ("projection", 0)):
        n = len(CAM_PARAMS[mode])
        out += [CamCase(mode, persp, B, 33, 1, _all(n)) for B in SHARED_B if B != 9]
        out += [CamCase(mode, persp, 9, V, 1, _all(n)) for V in CAM_V if V != 33]
        out += [CamCase(mode, persp, 2, V, 2, _all(n)) for V in (1, 257)]
    return list(dict.fromkeys(out))


def needle_cases():
    """the shared route's "every view exactly once": every B at V = 33, every V at B = 9"""
    return [c for c in camera_cases() if c.vb == 1 and c.mode in ("look_at", "projection") and c.persp == (c.mode == "look_at")
            and not any(c.pb) and (c.V == 33 or c.B == 9)]


def tan_width(angle=ANGLE):
    return float(np.tan(np.float32(angle / 180 * math.pi), dtype=np.float32))      # perspective.py:15-17


def _views(B, rng):
    """eyes at distance >= 2 in a cone about one direction (so that a parameter of batch 1 serves every view: z >= 1 whichever
    eye meets whichever axis), `at` near the origin, `up` within 0.1 of +y: at least 30 degrees off every viewing direction"""
    e0 = np.array([0.3, 0.2, -0.9]) / np.linalg.norm([0.3, 0.2, -0.9])
    eye = f32v(2.6 * e0 + 0.25 * rng.uniform(-1, 1, (B, 3)))
    at = f32v(0.05 * rng.uniform(-1, 1, (B, 3)))
    direction = f32v(-e0 + 0.05 * rng.uniform(-1, 1, (B, 3)))
    up = f32v(np.array([0.0, 1.0, 0.0]) + 0.1 * rng.uniform(-1, 1, (B, 3)))
    return eye, at, direction, up


def unit_ball(n, rng, radius=1.0):
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return f32v(0.98 * radius * d * rng.uniform(0, 1, (n, 1)) ** (1 / 3))


@functools.lru_cache(maxsize=None)
def camera_inputs(c):
    """dict(v [vb,V,3], g [B,V,3], prefill [vb,V,3], rot, eye, K, dist (each [1|B,...] or None), vectors (eye, at|direction, up)).
    The frame `rot` is the float32 restatement of d3m_camera_basis on the vectors: an input of the kernels under test."""
    rng = _rng(11, c.B, c.V, c.vb, *c.pb, len(c.mode), c.persp)
    B = c.B
    v = unit_ball(c.vb * c.V, rng, 0.95 if c.mode == "projection" else 1.0).reshape(c.vb, c.V, 3)
    g = f32v(rng.uniform(-1, 1, (B, c.V, 3)))
    prefill = f32v(rng.uniform(-1, 1, (c.vb, c.V, 3)))
    out = dict(v=v, g=g, prefill=prefill, rot=None, eye=None, K=None, dist=None, vectors=None)
    nb = dict(zip(CAM_PARAMS[c.mode], (1 if one else B for one in c.pb)))
    if c.mode in ("look_at", "look"):
        eye, at, direction, up = _views(B, rng)
        tgt = at if c.mode == "look_at" else direction
        out["vectors"] = (eye[:nb["eye"]], tgt[:nb["rot"]], up[:nb["rot"]])
        # the frame of view b from eye b (or 0) and target / up b (or 0): a frame of batch 1 is view 0's
        out["rot"] = f32v(camera_basis(eye[:nb["rot"]], tgt[:nb["rot"]], up[:nb["rot"]], c.mode == "look_at", nb["rot"], "f32"))
        out["eye"] = eye[:nb["eye"]]
    elif c.mode == "perspective":
        out["rot"], out["eye"] = np.eye(3).reshape(1, 9), np.zeros((1, 3))
        out["v"] = f32v(v + np.array([0.0, 0.0, 2.5]))          # z in [1.5, 3.5]
    elif c.mode == "projection":
        w = 0.2 * rng.uniform(-1, 1, (B, 3))
        th = np.linalg.norm(w, axis=1)[:, None, None]
        k = w / th[:, 0]
        Kx = np.zeros((B, 3, 3))
        Kx[:, 0, 1], Kx[:, 0, 2], Kx[:, 1, 0], Kx[:, 1, 2], Kx[:, 2, 0], Kx[:, 2, 1] = -k[:, 2], k[:, 1], k[:, 2], -k[:, 0], -k[:, 1], k[:, 0]
        R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)
        out["rot"] = f32v(R.reshape(B, 9))[:nb["rot"]]
        out["eye"] = f32v(np.array([0.0, 0.0, 2.5]) + rng.uniform(-1, 1, (B, 3)) * np.array([0.1, 0.1, 0.04]))[:nb["eye"]]
        K = np.array([200.0, 3.0, 128.0, 0.0, 210.0, 120.0, 0.0, 0.0, 1.0]) + rng.uniform(-1, 1, (B, 9)) * np.array([5, 1, 4, 0, 5, 4, 0, 0, 0.])
        out["K"] = f32v(K)[:nb["K"]]
        out["dist"] = f32v(np.array([-0.1, 0.05, 0.01, -0.02, 0.03]) * (1 + 0.2 * rng.uniform(-1, 1, (B, 5))))[:nb["dist"]]
    return out


def _normalize3(v):
    """normalize3: v / max(sqrt(v0 v0 + v1 v1 + v2 v2), 1e-5)"""
    d = fmax_(sqrt_(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), EPS_N)
    return [v[0] / d, v[1] / d, v[2] / d]


def _cross3(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def camera_basis(eye, at_or_dir, up, is_look_at, B, ar):
    """k_camera_basis: rows (x, y, z) [B,9]"""
    e, a, u = (lift(_entry(x, B), ar) for x in (eye, at_or_dir, up))
    z = _normalize3([a[:, k] - e[:, k] if is_look_at else a[:, k] for k in range(3)])
    x = _normalize3(_cross3([u[:, k] for k in range(3)], z))
    y = _normalize3(_cross3(z, x))
    return stack_(x + y + z, 1)


def _cam_cols(c, inp, ar):
    B = c.B
    col = lambda M, n: None if M is None else [lift(_entry(M, B), ar)[:, k:k + 1] for k in range(n)]        # noqa: E731
    return col(inp["rot"], 9), col(inp["eye"], 3), col(inp["K"], 9), col(inp["dist"], 5)


def _proj_chain(x, r, e, K, dc, orig):
    """camera_point's projection branch: (o, the intermediate values the adjoint needs)"""
    cx = x[0] * r[0] + x[1] * r[1] + x[2] * r[2] + e[0]
    cy = x[0] * r[3] + x[1] * r[4] + x[2] * r[5] + e[1]
    cz = x[0] * r[6] + x[1] * r[7] + x[2] * r[8] + e[2]
    zz = cz + 1e-9
    x_, y_ = cx / zz, cy / zz
    k1, k2, p1, p2, k3 = dc
    rr = sqrt_(x_ * x_ + y_ * y_)
    r2 = rr * rr
    r4 = r2 * r2
    r6 = r4 * r2
    radial = 1 + k1 * r2 + k2 * r4 + k3 * r6
    x__ = x_ * radial + 2 * p1 * x_ * y_ + p2 * (r2 + 2 * x_ * x_)
    y__ = y_ * radial + p1 * (r2 + 2 * y_ * y_) + 2 * p2 * x_ * y_
    u = x__ * K[0] + y__ * K[1] + K[2]
    vv = x__ * K[3] + y__ * K[4] + K[5]
    vv = orig - vv
    o = [2 * (u - orig / 2.0) / orig, 2 * (vv - orig / 2.0) / orig, cz]
    return o, dict(zz=zz, x_=x_, y_=y_, radial=radial, dr=k1 + 2 * k2 * r2 + 3 * k3 * r4)


def camera_forward(c, inp, ar):
    """k_camera_forward: [B,V,3]"""
    v = lift(_entry(inp["v"], c.B), ar)
    x = [v[:, :, k] for k in range(3)]
    if c.mode == "none":
        return stack_(x, 2)
    r, e, K, dc = _cam_cols(c, inp, ar)
    if c.mode == "projection":
        return stack_(_proj_chain(x, r, e, K, dc, inp.get("orig", ORIG_SIZE))[0], 2)
    d = [x[k] - e[k] for k in range(3)]
    o = [d[0] * r[3 * j] + d[1] * r[3 * j + 1] + d[2] * r[3 * j + 2] for j in range(3)]
    if c.persp:
        w = inp.get("width", tan_width())
        o = [o[0] / o[2] / w, o[1] / o[2] / w, o[2]]
    return stack_(o, 2)


def camera_adjoint_terms(c, inp, ar, variant=None, g=None):
    """camera_point_adjoint of every (view, vertex): [B,V,3], the terms both routes of k_camera_backward add up"""
    v = lift(_entry(inp["v"], c.B), ar)
    gg = lift(inp["g"] if g is None else g, ar)
    x, g = [v[:, :, k] for k in range(3)], [gg[:, :, k] for k in range(3)]
    if c.mode == "none":
        return stack_(g, 2)
    r, e, K, dc = _cam_cols(c, inp, ar)
    if c.mode == "projection":
        orig = inp.get("orig", ORIG_SIZE)
        _, t = _proj_chain(x, r, e, K, dc, orig)
        p1, p2 = dc[2], dc[3]
        gu, gvp = g[0] * 2.0 / orig, -g[1] * 2.0 / orig
        gx2, gy2 = K[0] * gu + K[3] * gvp, K[1] * gu + K[4] * gvp
        x_, y_ = t["x_"], t["y_"]
        six = 4 if variant == "proj_4p2" else 6
        dxx = t["radial"] + 2 * x_ * x_ * t["dr"] + 2 * p1 * y_ + six * p2 * x_
        dxy = 2 * x_ * y_ * t["dr"] + 2 * p1 * x_ + 2 * p2 * y_
        dyx = 2 * x_ * y_ * t["dr"] + 2 * p1 * x_ + 2 * p2 * y_
        dyy = t["radial"] + 2 * y_ * y_ * t["dr"] + 6 * p1 * y_ + 2 * p2 * x_
        gx1, gy1 = gx2 * dxx + gy2 * dyx, gx2 * dxy + gy2 * dyy
        gc = [gx1 / t["zz"], gy1 / t["zz"], g[2] - (gx1 * x_ + gy1 * y_) / t["zz"]]
    elif c.persp:
        d = [x[k] - e[k] for k in range(3)]
        o = [d[0] * r[3 * j] + d[1] * r[3 * j + 1] + d[2] * r[3 * j + 2] for j in range(3)]
        izw = 1.0 / (o[2] * inp.get("width", tan_width()))
        depth = (g[0] * o[0] + g[1] * o[1]) * izw
        gc = [g[0] * izw, g[1] * izw, g[2] - (depth if variant == "persp_no_z" else depth / o[2])]
    else:
        gc = g
    return stack_([r[k] * gc[0] + r[3 + k] * gc[1] + r[6 + k] * gc[2] for k in range(3)], 2)


def shared_sum32(terms, variant=None):
    """k_camera_backward's shared route on float32 terms [B,V,3], in its order: lane s adds views s, s + 8, ... to zero, then
    ((l0 + l1) + (l2 + l3)) + ((l7 + l6) + (l5 + l4)) -- quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror on lane 0"""
    assert terms.dtype == np.float32
    B = terms.shape[0]
    lanes = []
    for s in range(8):
        acc = np.zeros(terms.shape[1:], np.float32)
        for b in range(s, min(B, 8) if variant == "skip_views_ge_8" else B, 8):
            acc = acc + terms[b]
        if variant == "view0_twice" and s == 0:
            acc = acc + terms[0]
        lanes.append(acc)
    return ((lanes[0] + lanes[1]) + (lanes[2] + lanes[3])) + ((lanes[7] + lanes[6]) + (lanes[5] + lanes[4]))


def needle(g, b):
    """grad_out that is zero outside view b"""
    out = np.zeros_like(g)
    out[b] = g[b]
    return out


def add_onto(prefill, plain, variant=None):
    """d3m_camera_backward_add: float32(prefill + plain result); the wrong variant stores"""
    plain = np.asarray(plain, np.float32)
    return plain if variant == "add_stores" else np.asarray(prefill, np.float32) + plain


BasisCase = namedtuple("BasisCase", "is_look_at B pb kind")          # kind: float | zero_z | up_parallel


def basis_cases():
    out = [BasisCase(la, B, pb, "float") for la in (1, 0) for B in (1, 9, 65)
           for pb in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)) if B > 1 or not any(pb)]
    return out + [BasisCase(1, 3, (0, 0, 0), "zero_z"), BasisCase(0, 3, (0, 0, 0), "up_parallel")]


def basis_inputs(c):
    eye, at, direction, up = _views(c.B, _rng(12, c.B, *c.pb, c.is_look_at))
    tgt = at if c.is_look_at else direction
    if c.kind == "zero_z":
        tgt = eye.copy()                                    # at - eye = 0: every row 0 / 1e-5
    if c.kind == "up_parallel":
        tgt = np.array([[0, 0, 2.0], [0, 0, -0.5], [0, 4.0, 0]])
        up = np.array([[0, 0, 1.0], [0, 0, 3.0], [0, -1.0, 0]])          # cross(up, z) = 0 exactly
    n = [1 if one else c.B for one in c.pb]
    return eye[:n[0]], tgt[:n[1]], up[:n[2]]


# ==== 2. gather, scatter, ordered gather ================================================================================================
GatherCase = namedtuple("GatherCase", "B V Ft fb tb")          # tb: tri_batch; B (fb ? 2 : 1) Ft 9 = 252, 252, 261, 513, 513, 5580, ...


def gather_cases():
    return [GatherCase(1, 20, 14, 1, 1), GatherCase(1, 20, 28, 0, 1), GatherCase(1, 20, 29, 0, 1), GatherCase(3, 20, 19, 0, 1),
            GatherCase(3, 20, 19, 0, 3), GatherCase(1, 200, 310, 1, 1), GatherCase(3, 200, 310, 1, 1), GatherCase(3, 200, 310, 0, 3)]


def lanes_of(c):
    return c.B * (2 if c.fb else 1) * c.Ft * 9


HUB_DEGREE = 300


@functools.lru_cache(maxsize=None)
def gather_inputs(c):
    """dict(v [B,V,3], tri [tb,Ft,3] int32, g_a, g_b [B,F',3,3] integers (|g| <= 8, zeros and -0.0 among them), prefill [B,V,3]
    integers, flags [B,F'] int32, offsets [V+1], items [3 Ft] (the CSR of tri[0])).  Vertex 0 is a hub (degree 300 in the large
    meshes, every other face in the small ones), vertex V - 1 is used by no face, one face repeats a vertex."""
    rng = _rng(21, *c)
    Fp = (2 if c.fb else 1) * c.Ft
    tri = rng.integers(1, c.V - 1, (c.tb, c.Ft, 3))
    hub = np.arange(c.Ft) < HUB_DEGREE if c.Ft >= HUB_DEGREE else np.arange(c.Ft) % 2 == 0
    tri[:, hub, rng.integers(0, 3, int(hub.sum()))] = 0
    rep = int(np.flatnonzero(~hub)[-1])                                     # the last face without the hub repeats a vertex
    tri[:, rep, 1] = tri[:, rep, 0]
    tri = tri.astype(np.int32)
    assert (tri != c.V - 1).all() and (tri[:, rep, 0] == tri[:, rep, 1]).all()
    g_a, g_b = (rng.integers(-8, 9, (c.B, Fp, 3, 3)).astype(np.float64) for _ in range(2))
    g_a = np.where(rng.uniform(size=g_a.shape) < 0.1, -0.0, g_a)          # skipped by the scatter, harmless in the gather
    flags = (rng.uniform(size=(c.B, Fp)) < 0.6).astype(np.int32)
    flags[:, 0] = 0                                                          # a hidden face whose entries are not zero
    g_a[:, 0], g_b[:, 0] = 7.0, -5.0
    order = np.argsort(tri[0].reshape(-1), kind="stable")                   # items 3 f + c, ascending per vertex
    offsets = np.concatenate([[0], np.cumsum(np.bincount(tri[0].reshape(-1), minlength=c.V))]).astype(np.int32)
    assert offsets[1] == (HUB_DEGREE if c.Ft >= HUB_DEGREE else (c.Ft + 1) // 2) and offsets[-1] - offsets[-2] == 0
    return dict(v=f32v(rng.uniform(-1, 1, (c.B, c.V, 3))), tri=tri, g_a=g_a, g_b=g_b, flags=flags, offsets=offsets,
                items=order.astype(np.int32), prefill=rng.integers(-4, 5, (c.B, c.V, 3)).astype(np.float64))


def face_ids(c, tri):
    """IndexedFaces::vertex_ids of every (view, face): [B,F',3]; face Ft + f is face f with its corners reversed"""
    t = _entry(tri, c.B).astype(np.int64)
    return np.concatenate([t, t[:, :, ::-1]], 1) if c.fb else t


def gather_faces(c, inp):
    """k_gather_faces: [B,F',3,3], a copy"""
    ids = face_ids(c, inp["tri"])
    return np.asarray(inp["v"], np.float32)[np.arange(c.B)[:, None, None], ids]


def scatter_face_grads(c, inp, g, dtype=np.float64, absolute=False):
    """k_scatter_face_grads onto the prefill: entries that compare equal to zero are skipped (a sum's order does not matter for
    the integers of these cases: exact_sum_proven)"""
    ids = face_ids(c, inp["tri"])
    out = np.abs(inp["prefill"]).astype(dtype) if absolute else inp["prefill"].astype(dtype)
    g = np.abs(g) if absolute else g
    keep = g != 0
    b, f, n, k = np.nonzero(keep)
    np.add.at(out, (b, ids[b, f, n], k), g[keep].astype(dtype))
    return out


def vertex_gather(c, inp, g_a, g_b, flags, dtype=np.float64, variant=None, absolute=False):
    """k_vertex_gather: per (view, vertex) the items of the CSR in order; the back copy's corner is 2 - c"""
    assert c.tb == 1
    out = np.zeros((c.B, c.V, 3), dtype)
    if variant == "flags_ignored":
        flags = None
    for v in range(c.V):
        for item in inp["items"][inp["offsets"][v]:inp["offsets"][v + 1]]:
            f, cn = divmod(int(item), 3)
            for copy in range(2 if c.fb else 1):
                ff = c.Ft + f if copy else f
                cc = (cn if variant == "back_unreversed" else 2 - cn) if copy else cn
                on = np.ones(c.B, bool) if flags is None else flags[:, ff] != 0
                for arr in (g_a, g_b):
                    if arr is not None:
                        t = np.abs(arr[:, ff, cc]) if absolute else arr[:, ff, cc]
                        out[:, v] = out[:, v] + np.where(on[:, None], t, 0).astype(dtype)
    return out


def corner_pin(c):
    """a gradient that is non-zero in corners 0 and 2 of the back copies only, and differs between them"""
    g = np.zeros((c.B, 2 * c.Ft, 3, 3))
    g[:, c.Ft:, 0], g[:, c.Ft:, 2] = 1.0, 2.0
    return g


# ==== 3. lighting ==================================================================================================================
LightCase = namedtuple("LightCase", "n ts kind")
# kind: float | ones | back_ia0 | twin | id0 | ia0 | near_degenerate
LIGHT_N = (1, 255, 256, 257, 513)
LIGHT_TS = (1, 2, 3, 5)
LIGHT = dict(ia=float(np.float32(0.5)), id=float(np.float32(0.7)), ca=f32v([0.9, 0.8, 1.0]), cd=f32v([1.0, 0.7, 0.6]),
             dir=f32v([0.3, 0.8, -0.5]))
LIGHT_FWD_D = 7          # two differences, a cross product (1), the norm (2), n . d (2), ia ca + id cd r (1)


def light_grad_faces_D(ts):
    return ts ** 3 + 6      # the issue's figure: a face's ts^3 texels per channel, then the chain through the normal


def light_cases():
    out = [LightCase(n, ts, "float") for n in LIGHT_N for ts in LIGHT_TS if n in (257, 513) or ts == 2 or (n, ts) in ((1, 5), (256, 1), (255, 3))]
    out += [LightCase(257, 2, k) for k in ("ones", "back_ia0", "twin", "id0", "ia0", "near_degenerate")]
    return out + [LightCase(1, 1, "near_degenerate"), LightCase(513, 1, "ones")]


def light_of(c, inp=None):
    p = dict(LIGHT if inp is None else inp.get("light", LIGHT))
    if c.kind in ("back_ia0", "ia0"):
        p["ia"] = 0.0
    if c.kind == "id0":
        p["id"] = 0.0
    return p


def conditioning(faces, direction):
    """tests/test_param_reductions_host.py's face_conditioning on numpy faces [N,3,3]: (|cross| / (|a| |b|), |n . d| / |d|)"""
    import torch
    from test_param_reductions_host import face_conditioning
    shape, lit = face_conditioning(torch.from_numpy(np.asarray(faces, np.float64))[None], torch.from_numpy(np.asarray(direction, np.float64))[None])
    return shape[0].numpy(), lit[0].numpy()


REDRAW_ROUNDS = 100


@functools.lru_cache(maxsize=None)
def light_inputs(c):
    """dict(faces [N,3,3], tex, g [N,ts^3,3]): faces well shaped and off the light's horizon by 1.25 LIGHT_MARGIN (re-drawn until
    they are: raises otherwise, no case is dropped); face f's textures lie in (f + 1/4, f + 3/4) and its gradients in
    +-(f + 1/4, f + 3/4): those of a tail block differ from every other face's"""
    from test_param_reductions_host import LIGHT_MARGIN
    rng = _rng(31, c.n, c.ts, len(c.kind))
    faces = f32v(rng.uniform(-1, 1, (c.n, 3, 3)))
    todo = np.arange(c.n)
    for _ in range(REDRAW_ROUNDS):
        shape, lit = conditioning(faces[todo], LIGHT["dir"])
        todo = todo[(shape < 1.25 * LIGHT_MARGIN) | (lit < 1.25 * LIGHT_MARGIN)]
        if todo.size == 0:
            break
        faces[todo] = f32v(rng.uniform(-1, 1, (todo.size, 3, 3)))
    else:
        raise AssertionError("light_inputs: could not place every face off the light's horizon")
    a, b = faces[:, 0] - faces[:, 1], faces[:, 2] - faces[:, 1]
    facing = (np.cross(a, b) * LIGHT["dir"]).sum(1) > 0
    if c.kind == "back_ia0":                    # every face turned away from the light: swap v0 and v2 of the lit ones
        faces[facing] = faces[facing][:, ::-1]
    elif c.kind == "near_degenerate":           # the same shapes with edges of 1e-3 and facing the light: |cross| ~ 1e-6
        faces[~facing] = faces[~facing][:, ::-1]
        a, b = faces[:, 0] - faces[:, 1], faces[:, 2] - faces[:, 1]
        unit = lambda e: e / np.linalg.norm(e, axis=1, keepdims=True)          # noqa: E731
        # (v1 at the origin: the edges are the vertices themselves, and their bound is not that of a cancelled difference)
        faces = f32v(np.stack([1e-3 * unit(a), np.zeros_like(a), 1e-3 * unit(b)], 1))
    elif c.kind == "twin":
        faces[::3, 0] = faces[::3, 1]           # v0 = v1: the cross product is exactly zero
    per = c.ts ** 3
    f = np.arange(c.n)[:, None, None]
    tex = np.ones((c.n, per, 3)) if c.kind == "ones" else f32v(f + rng.uniform(0.25, 0.75, (c.n, per, 3)))
    sign = np.where(rng.uniform(size=(c.n, per, 3)) < 0.5, -1.0, 1.0)
    g = f32v(sign * (f + rng.uniform(0.25, 0.75, (c.n, per, 3))))
    return dict(faces=faces, tex=tex, g=g)


def face_light(faces, p, ar):
    """face_light (csrc/d3m_aux.h): (light [3][N], the normal [3][N], |cross| [N], n . d [N])"""
    f = lift(faces, ar)
    a = [f[:, 0, k] - f[:, 1, k] for k in range(3)]
    b = [f[:, 2, k] - f[:, 1, k] for k in range(3)]
    cr = _cross3(a, b)
    n = sqrt_(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2])
    d = fmax_(n, EPS_N)
    nrm = [cr[k] / d for k in range(3)]
    dr = [float(x) for x in p["dir"]]
    cs = nrm[0] * dr[0] + nrm[1] * dr[1] + nrm[2] * dr[2]
    r = where_(val(cs) > 0, cs, cs * 0.0) if isinstance(cs, Abs) else np.maximum(cs, cs.dtype.type(0))
    light = []
    for k in range(3):
        lk = _const(0.0, r)
        if p["ia"] != 0:
            lk = lk + _const(p["ia"], r) * float(p["ca"][k])
        if p["id"] != 0:
            lk = lk + p["id"] * (float(p["cd"][k]) * r)
        light.append(lk)
    return light, nrm, n, cs, (a, b)


def _const(x, like):
    """the constant x in the arithmetic (and shape) of `like`, so that a product of two constants rounds as the kernel's does"""
    return Abs(np.full(like.shape, x)) if isinstance(like, Abs) else np.full(like.shape, x, like.dtype)


def lighting_forward(c, inp, ar, variant=None):
    """k_lighting_forward: tex * light of the face that owns the texel -> [N,ts^3,3]"""
    light = stack_(face_light(inp["faces"], light_of(c, inp), ar)[0], 1)          # [N,3]
    tex = lift(inp["tex"], ar)
    if variant == "face_index_by_third":      # lf = e / (texels3 / 3): three faces' worth of lights per face, inside the block
        per3 = c.ts ** 3
        e = np.arange(c.n * per3 * 3).reshape(c.n, per3, 3)
        blk = e // (256 * per3 * 3)
        lf = np.minimum(blk * 256 + ((e - blk * 256 * per3 * 3) // per3) % 256, c.n - 1)
        return tex * light[lf, e % 3]
    return tex * light[:, None, :]


def sweep_stays_inside(c, variant=None):
    """whether the tail block's sweep ends with the array: min(256, n - f0) faces' texels; the wrong variant sweeps 256"""
    tail = 256 if variant == "tail_256" else min(256, c.n - (c.n - 1) // 256 * 256)
    return (c.n - 1) // 256 * 256 + tail == c.n


def lighting_backward(c, inp, ar, variant=None):
    """k_lighting_backward: (grad_textures [N,ts^3,3], grad_faces [N,3,3])"""
    p = light_of(c, inp)
    light, nrm, length, cs, (a, b) = face_light(inp["faces"], p, ar)
    g, tex = lift(inp["g"], ar), lift(inp["tex"], ar)
    g_tex = g * stack_(light, 1)[:, None, :]
    s_gl = sum_(g * tex, 1)                                                # [N,3]: LDS float atomics, any order
    cd, dr = [float(x) for x in p["cd"]], [float(x) for x in p["dir"]]
    g_cos = p["id"] * (cd[0] * s_gl[:, 0] + cd[1] * s_gl[:, 1] + cd[2] * s_gl[:, 2])
    gn = [g_cos * dr[k] for k in range(3)]
    dot = nrm[0] * gn[0] + nrm[1] * gn[1] + nrm[2] * gn[2]
    lv = val(length)
    safe = where_(lv > 0, length, length * 0.0 + 1.0)
    clamped = [gn[k] / safe if variant == "degenerate_by_len" else gn[k] / EPS_N for k in range(3)]
    gc = [where_(lv > np.float32(1e-5), (gn[k] - nrm[k] * dot) / safe, clamped[k]) for k in range(3)]
    ga, gb = _cross3(b, gc), _cross3(gc, a)
    on = (p["id"] != 0) & (val(cs) > 0)
    nil = _const(0.0, ga[0])
    rows = [where_(on, ga[k], nil) for k in range(3)] + [where_(on, -(ga[k] + gb[k]), nil) for k in range(3)] + \
        [where_(on, gb[k], nil) for k in range(3)]
    gf = stack_(rows, 1)
    if isinstance(gf, Abs):
        return g_tex, Abs(gf.v.reshape(-1, 3, 3), gf.a.reshape(-1, 3, 3))
    return g_tex, gf.reshape(-1, 3, 3)


def soup(faces):
    """faces [N,3,3] as a triangle soup for d3m_face_light: (vertices [1,3N,3], tri [1,N,3] int32)"""
    n = faces.shape[0]
    return np.asarray(faces, np.float32).reshape(1, 3 * n, 3), np.arange(3 * n, dtype=np.int32).reshape(1, n, 3)


# ==== 4. output epilogue ===============================================================================================================
EpiCase = namedtuple("EpiCase", "B S aa bb")            # bb: the background's batch


def epilogue_cases():
    return [EpiCase(B, S, aa, bb) for aa, sizes in ((1, (2, 6, 10, 34)), (0, (1, 5, 17, 33))) for S in sizes for B in (1, 3)
            for bb in sorted({1, B})]


# (rgb_map, depth_map, rgb_blended, alpha_map, rgb_out, alpha_out, depth_out) given: the combinations the header allows
EPI_POINTERS = {"all": (1, 1, 1, 1, 1, 1, 1), "no_rgb": (0, 1, 0, 1, 0, 1, 1), "no_depth": (1, 0, 1, 1, 1, 1, 0),
                "no_internal": (1, 1, 0, 0, 1, 1, 1), "silhouette": (0, 0, 0, 1, 0, 1, 0), "rgb_out_only": (1, 0, 0, 0, 1, 0, 0)}


@functools.lru_cache(maxsize=None)
def epilogue_inputs(c):
    """seeded, non-symmetric maps: face_index_map [B,S,S] int32 (about 40 % uncovered), rgb_map [B,S,S,3], depth_map [B,S,S],
    background [bb,3] with rows that differ, and the gradients of the three output images"""
    rng = _rng(41, *c)
    s = c.S // 2 if c.aa else c.S
    fim = rng.integers(0, 6, (c.B, c.S, c.S)).astype(np.int32)
    fim[rng.uniform(size=fim.shape) < 0.4] = -1
    fim[:, -1, -1] = 0
    fim[1::2 if c.S == 1 else 1, 0, 0] = -1          # every view shows its background (S = 1: the odd views do)
    return dict(fim=fim, rgb=rng.uniform(0.1, 1, (c.B, c.S, c.S, 3)).astype(np.float32), depth=rng.uniform(1, 9, (c.B, c.S, c.S)).astype(np.float32),
                bg=(0.1 + 0.2 * np.arange(c.bb * 3).reshape(c.bb, 3)).astype(np.float32),
                g_rgb=rng.uniform(-1, 1, (c.B, 3, s, s)).astype(np.float32), g_alpha=rng.uniform(-1, 1, (c.B, s, s)).astype(np.float32),
                g_depth=rng.uniform(-1, 1, (c.B, s, s)).astype(np.float32))


def output_epilogue(c, inp, variant=None):
    """k_output_epilogue in float32, bit for bit: dict(rgb_blended [B,S,S,3], alpha_map [B,S,S], rgb_out [B,3,s,s], alpha_out,
    depth_out [B,s,s]).  rgb mask + (1 - mask) bg; pooled ((p00 + p01) + p10) + p11 over internal rows S - 1 - (2 yo + dy), x 0.25"""
    one = np.float32(1)
    mask = (inp["fim"] >= 0).astype(np.float32)
    bg = inp["bg"][np.zeros(c.B, np.int64)] if (variant == "bg_row0" or c.bb == 1) else inp["bg"]
    blended = inp["rgb"] * mask[..., None] + (one - mask)[..., None] * bg[:, None, None, :]
    n = 2 if c.aa else 1
    s = c.S // n

    def pooled(m):          # m [B,S,S,...] internal -> [B,s,s,...]
        acc = None
        for dy in range(n):
            for dx in range(n):
                if variant == "pool_before_flip":          # rows paired in internal order, the pooled image flipped afterwards
                    rows = 2 * (s - 1 - np.arange(s)) + dy
                else:
                    rows = c.S - 1 - (np.arange(s) * n + dy)
                t = m[:, rows][:, :, np.arange(s) * n + dx]
                acc = (np.zeros_like(t) + t) if acc is None else acc + t
        return acc * np.float32(0.25 if c.aa else 1.0)
    return dict(rgb_blended=blended, alpha_map=mask, rgb_out=np.ascontiguousarray(pooled(blended).transpose(0, 3, 1, 2)),
                alpha_out=pooled(mask), depth_out=pooled(inp["depth"]))


def output_epilogue_backward(c, inp):
    """k_output_epilogue_backward: a copy times 1 or 0.25 -> (g_rgb_map [B,S,S,3], g_alpha_map, g_depth_map [B,S,S])"""
    n = 2 if c.aa else 1
    yo, xo = (c.S - 1 - np.arange(c.S)) // n, np.arange(c.S) // n
    sc = np.float32(0.25 if c.aa else 1.0)
    up = lambda m: m[..., yo, :][..., xo] * sc          # noqa: E731
    return np.ascontiguousarray(up(inp["g_rgb"]).transpose(0, 2, 3, 1)), up(inp["g_alpha"]), up(inp["g_depth"])
