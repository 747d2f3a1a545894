"""Smooth lighting of a mesh: `vertex_normals` (area-weighted per-vertex normals), `sh_vertex_colors` (per-vertex albedo lit
by the 9-term spherical-harmonic basis of those normals: one autograd node, differentiable in vertices, colours and sh),
`sh_basis` (the nine terms in plain torch) and `SHLight` (the coefficients as a parameter).

    N_f    = (x1 - x0) x (x2 - x0)                     (core.renderer_pt3d.vertex_normals, mesh_cython.get_norm_direction)
    s[b,v] = sum over v's adjacency items (f, c), ascending, of N_f[b]       r = |s|       n = s / max(r, 1e-6)
    shaded[b,v,k] = colors[b,v,k] * sum_j sh[b,k,j] H_j(n[b,v])              (H: sh_basis; no clamp, no ReLU)

This normal is the opposite of nr.lighting's face normal (x0 - x1) x (x2 - x1): a caller who wants the other side passes
faces.flip(-1).  A vertex of no face gets n = 0.  The output feeds textures_from_vertex_colors; a smooth-lit render sets the
renderer's own flat light to ambient 1, directional 0.

d3m_smooth_shade_forward is at most three launches and d3m_smooth_shade_backward at most five, with no float atomics and a
fixed order for every sum (csrc/d3m_smooth_shade.h states it): rows of the faces' adjacency in ascending item order, hub
vertices through the chunks of row_gather.py, the 27 sums of grad_sh through the tree of pose.py, shared inputs summed over
the sets in ascending order.  The adjacency is built once per faces tensor (vertex_adjacency: the one host read, outside
any capture) and after that the node never synchronises."""
import ctypes
import math

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from .. import _lib
from .row_gather import LONG_ROW, AdjacencyCache, checked_faces, vertex_adjacency  # noqa: F401 (LONG_ROW stays importable from here)

MAX_SETS = 65535
# the constants of the reference's fit_illumination (renderer_demo/mesh_cython/render.py:59-67)
SH_A = (math.sqrt(1 / (4 * math.pi)), math.sqrt(3 / (4 * math.pi)), 0.5 * math.sqrt(3 / (4 * math.pi)),
        3 * math.sqrt(5 / (12 * math.pi)), 1.5 * math.sqrt(5 / (12 * math.pi)))


def sh_basis(normals):
    """The nine spherical-harmonic terms H_j of unit normals [..., 3] -> [..., 9], in the normals' dtype and on their device
    (plain torch, differentiable)."""
    if not torch.is_tensor(normals) or normals.shape[-1:] != (3,) or not normals.is_floating_point():
        raise ValueError("normals must be a floating-point tensor [..., 3]")
    a0, a1, a2, a3, a4 = SH_A
    nx, ny, nz = normals.unbind(-1)
    return torch.stack([torch.full_like(nx, a0), a1 * nx, a1 * ny, a1 * nz, a2 * (2 * nz * nz - nx * nx - ny * ny),
                        a3 * (ny * nz), a3 * (nx * nz), a3 * (nx * ny), a4 * (nx * nx - ny * ny)], -1)


def _scratch(B, vb, A, device):
    n = int(_lib.lib().d3m_smooth_shade_scratch_floats(B, vb, A.num_vertices, A.num_faces, A.csr.num_chunks))
    if n == 0:
        raise ValueError("sets * vertices * 3 must stay below 2^31")
    return torch.empty(n, dtype=torch.float32, device=device), n


def forward(vertices, colors, sh, adjacency):
    """d3m_smooth_shade_forward on checked contiguous device tensors: vertices [1 or B,V,3], colors [1 or B,V,3] or None, sh
    [1 or B,3,9] or None.  Returns (shaded [B,V,3] or None, normals [vb,V,3], lengths [vb,V])."""
    A, vb, V, dev = adjacency, vertices.shape[0], vertices.shape[1], vertices.device
    B = vb if colors is None else max(vb, colors.shape[0], sh.shape[0])
    scratch, n = _scratch(B, vb, A, dev)
    shaded = None if colors is None else torch.empty(B, V, 3, dtype=torch.float32, device=dev)
    normals = torch.empty(vb, V, 3, dtype=torch.float32, device=dev)
    lengths = torch.empty(vb, V, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().d3m_smooth_shade_forward(
        _lib.ptr(vertices), vb, _lib.ptr(colors), 1 if colors is None else colors.shape[0], _lib.ptr(sh),
        1 if sh is None else sh.shape[0], _lib.ptr(A.tri), ctypes.byref(A.csr.c), _lib.ptr(scratch), n, _lib.ptr(shaded),
        _lib.ptr(normals), _lib.ptr(lengths), B, V, A.num_faces, _lib.stream_ptr()), "d3m_smooth_shade_forward")
    return shaded, normals, lengths


def backward(vertices, colors, sh, normals, lengths, adjacency, grad_shaded=None, grad_normals=None, need_vertices=True,
             need_colors=True, need_sh=True):
    """d3m_smooth_shade_backward on the tensors of `forward` and contiguous f32 gradients of its outputs (None: zeros).
    Returns (grad_vertices [vb,V,3], grad_colors [cb,V,3], grad_sh [sb,3,9]), each None where it is not needed."""
    A, vb, V, dev = adjacency, vertices.shape[0], vertices.shape[1], vertices.device
    B = vb if colors is None else max(vb, colors.shape[0], sh.shape[0])
    scratch, n = _scratch(B, vb, A, dev)
    lit = colors is not None and grad_shaded is not None
    g_v = torch.empty(vb, V, 3, dtype=torch.float32, device=dev) if need_vertices else None
    g_c = torch.empty(colors.shape[0], V, 3, dtype=torch.float32, device=dev) if lit and need_colors else None
    g_sh = torch.empty(sh.shape[0], 3, 9, dtype=torch.float32, device=dev) if lit and need_sh else None
    if g_v is None and g_c is None and g_sh is None:
        return None, None, None
    _lib.check(_lib.lib().d3m_smooth_shade_backward(
        _lib.ptr(vertices), vb, _lib.ptr(colors), 1 if colors is None else colors.shape[0], _lib.ptr(sh),
        1 if sh is None else sh.shape[0], _lib.ptr(normals), _lib.ptr(lengths), _lib.ptr(grad_shaded), _lib.ptr(grad_normals),
        _lib.ptr(A.tri), ctypes.byref(A.csr.c), _lib.ptr(scratch), n, _lib.ptr(g_v), _lib.ptr(g_c), _lib.ptr(g_sh), B, V,
        A.num_faces, _lib.stream_ptr()), "d3m_smooth_shade_backward")
    return g_v, g_c, g_sh


def _sets(t):
    return t.shape[0] if t is not None and t.dim() == 3 else 1


def _checked(vertices, faces, colors, sh, cache):
    """(the adjacency, whether any input has a set dimension) after the argument checks: dtypes, ranks and shapes are judged
    before the device, so those errors show without one."""
    given = [("vertices", vertices, (3,), "[V, 3] or [B, V, 3]")]
    if colors is not None or sh is not None:
        given += [("colors", colors, (3,), "[V, 3] or [B, V, 3]"), ("sh", sh, (3, 9), "[3, 9] or [B, 3, 9]")]
    for name, t, tail, form in given:
        if not torch.is_tensor(t):
            raise ValueError(f"{name} must be a tensor")
        if t.dtype != torch.float32:
            raise ValueError(f"{name} must be float32 (found {t.dtype})")
        if t.dim() not in (2, 3) or tuple(t.shape[-len(tail):]) != tail or t.shape[-2] < 1:
            raise ValueError(f"{name} must be {form} (found {tuple(t.shape)})")
    faces = checked_faces(faces)
    V = vertices.shape[-2]
    if colors is not None and colors.shape[-2] != V:
        raise ValueError(f"colors has {colors.shape[-2]} vertices, vertices {V}")
    counts = {_sets(t) for _, t, _, _ in given if t.dim() == 3}
    B = max(counts | {1})
    if not 1 <= B <= MAX_SETS or 0 in counts:
        raise ValueError(f"1 to {MAX_SETS} sets per call")
    if len(counts - {1}) > 1:
        raise ValueError(f"the inputs' set counts differ: {sorted(counts)}")
    if B * V * 3 >= 2 ** 31:
        raise ValueError("sets * vertices * 3 must stay below 2^31")
    for name, t, _, _ in given + [("faces", faces, None, None)]:
        if not t.is_cuda or t.device != vertices.device:
            raise ValueError(f"vertices, colors, sh and faces must be on one GPU device ({name} is on {t.device})")
    return vertex_adjacency(faces, V, cache), bool(counts)


def _batch(t):
    return None if t is None else (t if t.dim() == 3 else t[None]).contiguous()


def _grad(g, shape):
    return None if g is None else g.to(torch.float32).reshape(shape).contiguous()


class _SmoothShade(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vertices, colors, sh, adjacency, batched):
        ctx.set_materialize_grads(False)
        v, c, s = _batch(vertices), _batch(colors), _batch(sh)
        shaded, normals, lengths = forward(v, c, s, adjacency)
        ctx.save_for_backward(v, c, s, normals, lengths)
        ctx.adjacency = adjacency
        ctx.shapes = tuple(None if t is None else tuple(t.shape) for t in (vertices, colors, sh))
        if vertices.dim() == 2:
            normals = normals[0]
        if shaded is not None and not batched:
            shaded = shaded[0]
        return shaded, normals

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_shaded, grad_normals):
        need = ctx.needs_input_grad[:3]
        if (grad_shaded is None and grad_normals is None) or not any(need):
            return (None,) * 5
        v, c, s, normals, lengths = ctx.saved_tensors
        B = v.shape[0] if c is None else max(v.shape[0], c.shape[0], s.shape[0])
        grads = backward(v, c, s, normals, lengths, ctx.adjacency, _grad(grad_shaded, (B,) + tuple(v.shape[1:])),
                         _grad(grad_normals, tuple(v.shape)), *need)
        return tuple(None if g is None else g.reshape(shape) for g, shape in zip(grads, ctx.shapes)) + (None, None)


def sh_vertex_colors(vertices, faces, colors, sh, cache=None, return_normals=False):
    """Per-vertex albedo `colors` lit by the spherical-harmonic light `sh` at the smooth vertex normals of the mesh.

    vertices f32 [V,3] or [B,V,3]; faces [F,3] or [1,F,3] int32 / int64, a constant; colors f32 [V,3] or [B,V,3]; sh f32
    [3,9] or [B,3,9] (channel, basis term), all on one GPU device.  An input without B is shared by every set.  Returns shaded
    [B,V,3] ([V,3] when all three inputs are shared) = colors * sum_j sh[k,j] H_j(n), n the normalised sum of the normals
    (x1 - x0) x (x2 - x0) of the vertex's faces (pass faces.flip(-1) for the other side; a vertex of no face has n = 0);
    with return_normals=True, (shaded, normals), normals shaped like vertices.  No clamp is applied.

    One autograd node, differentiable in vertices, colors and sh; the gradient of a shared input is summed over the sets in
    ascending order, every sum has a fixed order and no float atomics are used.  The first call with a faces tensor builds its
    adjacency (outside any stream capture; a ValueError for an index outside [0, V)); `cache`: the AdjacencyCache to keep it
    in (default: the module's).  ValueError, before the device is touched, for a wrong dtype, rank, shape or device."""
    if colors is None or sh is None:
        raise ValueError("colors and sh must be tensors (vertex_normals gives the normals alone)")
    adjacency, batched = _checked(vertices, faces, colors, sh, cache)
    shaded, normals = _SmoothShade.apply(vertices, colors, sh, adjacency, batched)
    return (shaded, normals) if return_normals else shaded


def vertex_normals(vertices, faces, cache=None):
    """The smooth vertex normals sh_vertex_colors lights with, [V,3] or [B,V,3] like `vertices`: the same node without
    colours, differentiable in the vertices."""
    adjacency, _ = _checked(vertices, faces, None, None, cache)
    return _SmoothShade.apply(vertices, None, None, adjacency, vertices.dim() == 3)[1]


class SHLight(nn.Module):
    """A spherical-harmonic light as a learnable parameter: `sh` [3,9], or [per_set,3,9] with per_set sets, initialised to
    white ambient (sh[..., 0] = 1 / a0, the rest 0: shaded = colors up to rounding).  forward(vertices, faces, colors) returns
    sh_vertex_colors' shaded colours; the module keeps the adjacency of the faces it last saw itself, so whatever holds the
    module (a captured step) keeps the adjacency.  shade(normals, fragments, colors=None) lights a Fragments record per pixel
    with the same coefficients (sh_fragments.py)."""

    def __init__(self, per_set=None):
        super().__init__()
        if per_set is not None and not 1 <= int(per_set) <= MAX_SETS:
            raise ValueError(f"per_set must be None or 1 to {MAX_SETS}")
        sh = torch.zeros((3, 9) if per_set is None else (int(per_set), 3, 9), dtype=torch.float32)
        sh[..., 0] = 1.0 / SH_A[0]
        self.sh = nn.Parameter(sh)
        self._adjacency = AdjacencyCache(1)

    def forward(self, vertices, faces, colors, return_normals=False):
        return sh_vertex_colors(vertices, faces, colors, self.sh, cache=self._adjacency, return_normals=return_normals)

    def shade(self, normals, fragments, colors=None, **kw):
        """(images [B,3,s,s], alpha [B,s,s]) of this light PER PIXEL over a Fragments record: sh_fragments.shade_fragments
        with the module's coefficients (per_set must then be None or the record's views); kw: its background, cache and
        screen_vertices."""
        from .sh_fragments import shade_fragments
        return shade_fragments(normals, self.sh, fragments, colors=colors, **kw)

    def shade_uv_texture(self, image, faces_uv, normals, fragments, **kw):
        """(images [B,3,s,s], alpha [B,s,s]) of this light PER PIXEL on the UV albedo `image` over a Fragments record:
        sh_uv_fragments.shade_uv_texture with the module's coefficients (per_set must then be None or the record's views);
        kw: its texture_wrapping, background, cache and screen_vertices."""
        from .sh_uv_fragments import shade_uv_texture
        return shade_uv_texture(image, faces_uv, normals, self.sh, fragments, **kw)
