"""The vertices of a linear morphable model (a 3DMM such as the Basel face model): `morphable_vertices` (one autograd node,
differentiable with respect to the coefficients) and `MorphableModel` (mean, basis and scale as buffers).

    vertices[b] = mean + basis (scale * coeffs[b])            basis [3V, K] row-major, the rows in (vertex, xyz) order

d3m_morphable_forward and d3m_morphable_backward stream the basis once per SETS_PER_PASS coefficient sets.  The adjoint
grad_coeffs[b, k] = scale[k] * sum_r basis[r, k] * grad[b, r] is a sum over 3V rows with no float atomics and a fixed tree:
a workgroup takes ROWS_PER_CHUNK consecutive rows and COMPONENTS_PER_WORKGROUP components, each of its four waves adds
ROWS_PER_WAVE rows in ascending order, the waves' sums are added in wave order into one partial per (chunk, set, component),
and a second launch adds the chunks in FINISH_GROUPS groups of consecutive chunks, ascending, then the groups in order.  There
is no cache and no host synchronisation: the node can be captured from its first call."""
import torch
import torch.nn as nn

from .. import _lib

# the constants of csrc/d3m_morphable.h that fix the summation trees
ROWS_PER_CHUNK = 256            # adjoint: consecutive rows of one workgroup (MB_ROWS)
ROWS_PER_WAVE = 64              # adjoint: rows one accumulator adds in ascending order (MB_WAVE_ROWS)
WAVES_PER_CHUNK = ROWS_PER_CHUNK // ROWS_PER_WAVE
COMPONENTS_PER_WORKGROUP = 64   # adjoint: components of one workgroup, one per lane (MB_KW)
FINISH_GROUPS = 16              # adjoint: groups of consecutive chunks in the second launch (MB_FINISH_GROUPS)
SETS_PER_PASS = 16              # coefficient sets per pass over the basis, both directions (MB_SETS)
FORWARD_COMPONENTS_PER_STEP = 64    # forward: components per LDS step (MB_FWD_KC), 16 per wave
MAX_SETS, MAX_COMPONENTS = 4096, 1024


def num_chunks(num_rows):
    return (int(num_rows) + ROWS_PER_CHUNK - 1) // ROWS_PER_CHUNK


def adjoint_chain(num_rows):
    """The longest chain of additions behind one element of the adjoint over num_rows rows: a wave's rows, the waves of a
    chunk, a group's chunks, the groups."""
    n = num_chunks(num_rows)
    return min(ROWS_PER_WAVE, int(num_rows)) + WAVES_PER_CHUNK + (n + FINISH_GROUPS - 1) // FINISH_GROUPS + FINISH_GROUPS


def forward_chain(num_components):
    """The same for the forward over num_components components: a wave's 16 components of every step, the four waves, the mean."""
    steps = (int(num_components) + FORWARD_COMPONENTS_PER_STEP - 1) // FORWARD_COMPONENTS_PER_STEP
    return 16 * steps + 4 + 1


def forward(coeffs, basis, mean=None, scale=None, out=None):
    """d3m_morphable_forward on checked, contiguous device tensors: coeffs [B,K], basis [R,K], mean [R] / scale [K] or None.
    Returns out [B,R] (allocated when None).  No host synchronisation."""
    B, K = coeffs.shape
    R = basis.shape[0]
    if out is None:
        out = torch.empty(B, R, dtype=torch.float32, device=coeffs.device)
    _lib.check(_lib.lib().d3m_morphable_forward(_lib.ptr(basis), _lib.ptr(coeffs), _lib.ptr(mean), _lib.ptr(scale),
                                                _lib.ptr(out), B, R, K, _lib.stream_ptr()), "d3m_morphable_forward")
    return out


def backward(grad_out, basis, scale=None, out=None, grad_scale=None, accumulate=False):
    """d3m_morphable_backward: grad_out [B,R] -> grad_coeffs [B,K], written to `out` (allocated when None; accumulate: added
    to it), times the device factor grad_scale [B] when given.  No host synchronisation."""
    B, R = grad_out.shape
    K = basis.shape[1]
    if out is None:
        if accumulate:
            raise ValueError("accumulate needs the destination `out`")
        out = torch.empty(B, K, dtype=torch.float32, device=grad_out.device)
    L = _lib.lib()
    n = int(L.d3m_morphable_scratch_floats(B, R, K))
    scratch = torch.empty(max(n, 1), dtype=torch.float32, device=grad_out.device)
    _lib.check(L.d3m_morphable_backward(_lib.ptr(basis), _lib.ptr(grad_out), _lib.ptr(scale), _lib.ptr(grad_scale),
                                        _lib.ptr(scratch), n, _lib.ptr(out), B, R, K, int(bool(accumulate)),
                                        _lib.stream_ptr()), "d3m_morphable_backward")
    return out


def _checked(coeffs, basis, mean, scale):
    """The arguments as the kernels read them: (coeffs [B,K], basis [R,K], mean [R] or None, scale [K] or None, batched).
    Dtypes, ranks and shapes are judged before the device, so those errors show without one."""
    for name, t in (("coeffs", coeffs), ("basis", basis), ("mean", mean), ("scale", scale)):
        if t is None and name in ("mean", "scale"):
            continue
        if not torch.is_tensor(t):
            raise ValueError(f"{name} must be a tensor")
        if t.dtype != torch.float32:
            raise ValueError(f"{name} must be float32 (found {t.dtype})")
        if name != "coeffs" and t.requires_grad:
            raise NotImplementedError(f"morphable_vertices: the gradient with respect to {name} is not computed "
                                      "(detach it; only coeffs is differentiable)")
    if coeffs.dim() not in (1, 2):
        raise ValueError("coeffs must be [K] or [B, K]")
    if basis.dim() == 3:
        if basis.shape[1] != 3:
            raise ValueError("basis must be [3V, K] or [V, 3, K]")
        basis = basis.reshape(-1, basis.shape[-1])
    elif basis.dim() != 2:
        raise ValueError("basis must be [3V, K] or [V, 3, K]")
    R, K = basis.shape
    if R < 3 or R % 3:
        raise ValueError(f"basis: {R} rows are not 3 per vertex")
    if not 1 <= K <= MAX_COMPONENTS:
        raise ValueError(f"1 to {MAX_COMPONENTS} components (found {K})")
    if R * K >= 2 ** 31:
        raise ValueError("basis: 2^31 elements or more")
    if coeffs.shape[-1] != K:
        raise ValueError(f"coeffs has {coeffs.shape[-1]} components, basis {K}")
    batched = coeffs.dim() == 2
    if batched and not 1 <= coeffs.shape[0] <= MAX_SETS:
        raise ValueError(f"1 to {MAX_SETS} coefficient sets per call")
    if mean is not None:
        if mean.numel() != R or (mean.dim() > 1 and tuple(mean.shape) not in ((R // 3, 3), (R, 1))):
            raise ValueError(f"mean must be [{R}], [{R}, 1] or [{R // 3}, 3]")
        mean = mean.reshape(-1).contiguous()
    if scale is not None:
        if scale.numel() != K or scale.dim() > 2 or (scale.dim() == 2 and 1 not in scale.shape):
            raise ValueError(f"scale must be [{K}]")
        scale = scale.reshape(-1).contiguous()
    for name, t in (("coeffs", coeffs), ("basis", basis), ("mean", mean), ("scale", scale)):
        if t is not None and not t.is_cuda:
            raise ValueError(f"{name} must be on the GPU device (found {t.device})")
        if t is not None and t.device != coeffs.device:
            raise ValueError(f"{name} is on {t.device}, coeffs on {coeffs.device}")
    return coeffs, basis.contiguous(), mean, scale, batched


class _Morphable(torch.autograd.Function):
    @staticmethod
    def forward(ctx, coeffs, basis, mean, scale, batched):
        c = (coeffs if batched else coeffs[None]).contiguous()
        out = forward(c, basis, mean, scale)
        ctx.basis, ctx.scale, ctx.batched = basis, scale, batched
        out = out.view(c.shape[0], -1, 3)
        return out if batched else out[0]

    @staticmethod
    def backward(ctx, grad_vertices):
        g = grad_vertices.reshape(1 if not ctx.batched else grad_vertices.shape[0], -1).to(torch.float32).contiguous()
        grad = backward(g, ctx.basis, ctx.scale)
        return (grad if ctx.batched else grad[0]), None, None, None, None


def morphable_vertices(coeffs, basis, mean=None, scale=None):
    """mean + basis (scale * coeffs) as vertices: coeffs [K] -> [V,3], coeffs [B,K] -> [B,V,3].

    coeffs f32 on the device (need not be contiguous); basis [3V,K] or [V,3,K] (row 3 v + j is coordinate j of vertex v);
    mean [3V], [3V,1] or [V,3] or None (0); scale [K] or None (1).  One autograd node; the gradient reaches coeffs only, in
    the fixed order the module text describes: basis, mean or scale that require grad raise NotImplementedError.  ValueError
    for a wrong dtype, rank, device or shape.  No host synchronisation, nothing cached."""
    coeffs, basis, mean, scale, batched = _checked(coeffs, basis, mean, scale)
    return _Morphable.apply(coeffs, basis, mean, scale, batched)


class MorphableModel(nn.Module):
    """A linear morphable model: `mean` [3V] ([3V,1], [V,3]), `basis` [3V,K] ([V,3,K]) or a list of such bases, concatenated
    along K here, once (identity | expression), and `scale` [K] (or a list matching the bases; None: 1), held as buffers.
    forward(coeffs [K] or [B,K]) returns the vertices [V,3] or [B,V,3]."""

    def __init__(self, mean, basis, scale=None):
        super().__init__()
        bases = list(basis) if isinstance(basis, (list, tuple)) else [basis]
        bases = [torch.as_tensor(b).detach().to(torch.float32) for b in bases]
        bases = [b.reshape(-1, b.shape[-1]) if b.dim() == 3 else b for b in bases]
        if not bases or any(b.dim() != 2 or b.shape[0] != bases[0].shape[0] for b in bases):
            raise ValueError("MorphableModel: every basis must be [3V, K_i] (or [V, 3, K_i]) with the same V")
        full = torch.cat(bases, 1).contiguous()
        R, K = full.shape
        if R < 3 or R % 3:
            raise ValueError(f"MorphableModel: {R} rows are not 3 per vertex")
        if not 1 <= K <= MAX_COMPONENTS:
            raise ValueError(f"MorphableModel: 1 to {MAX_COMPONENTS} components (found {K})")
        mean = torch.as_tensor(mean).detach().to(torch.float32).reshape(-1).contiguous().to(full.device)
        if mean.numel() != R:
            raise ValueError(f"MorphableModel: mean must hold {R} values")
        if scale is not None:
            scales = list(scale) if isinstance(scale, (list, tuple)) else [scale]
            scale = torch.cat([torch.as_tensor(s).detach().to(torch.float32).reshape(-1) for s in scales]).contiguous()
            if scale.numel() != K:
                raise ValueError(f"MorphableModel: scale must hold {K} values")
            scale = scale.to(full.device)
        self.register_buffer("mean", mean.clone())
        self.register_buffer("basis", full.clone() if len(bases) == 1 else full)
        self.register_buffer("scale", None if scale is None else scale.clone())

    @property
    def num_components(self):
        return self.basis.shape[1]

    @property
    def num_vertices(self):
        return self.basis.shape[0] // 3

    def forward(self, coeffs):
        return morphable_vertices(coeffs, self.basis, self.mean, self.scale)
