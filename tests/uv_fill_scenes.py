"""Fused and push-pull filled uv textures (neural_renderer/uv_fill.py, csrc/d3m_uv_fill.h): the restatement with torch
operators in float64 (the reference) and float32 (the yardstick), the cases, the seeded inputs and the recorded float32
yardsticks.

THE FUNCTION, restated from the header.  View b counts at texel t iff w_b[t] > 0; t is valid iff some view counts;
v0 = (sum w_b x_b) / (sum w_b) over the counting views in ascending b, the sums starting at the first counting view's term.
Pull: s_0 = v0 on valid texels, 0 elsewhere, n_0 = 1 / 0; level l + 1 has (h + 1) >> 1 rows and (w + 1) >> 1 columns and
s_{l+1}(y, x) = ((s_l(2y, 2x) + s_l(2y, 2x + 1)) + s_l(2y + 1, 2x)) + s_l(2y + 1, 2x + 1), a child outside the level 0; n
likewise; up to the 1 x 1 level L.  Push: f_L = n_L > 0 ? s_L / n_L : background, f_l = n_l > 0 ? s_l / n_l : the bilinear value
of f_{l+1} at the texel's centre, per axis p = clamp(0.5 i - 0.25, 0, N2 - 1), i0 = min(floor p, max(N2 - 2, 0)),
i1 = min(i0 + 1, N2 - 1), t = p - i0.  The output is f_0; without the fill, v0 on valid texels and the background elsewhere.
The gradient with respect to the textures is autograd's of these operators; weights and validity are constants.

YARDSTICKS.  Per case and kind the largest |float32 restatement - float64 restatement| in units of the float64 result's
largest entry, recorded below and measured again by tests/test_uv_fill_host.py within a factor 2.  DEVICE_TOLERANCE of a kind
is 8 x the largest recorded yardstick of that kind."""
import torch

KINDS = ("texture", "textures_grad")

# (name, H, W, B, C): the smallest shapes that can break the kernels
CASES = (
    ("one", 1, 1, 1, 1),            # the smallest input: L = 0
    ("odd", 5, 7, 2, 3),            # odd sizes at every level, clamped taps; a negative and a NaN weight
    ("tiles", 37, 50, 3, 9),        # partial tiles, H != W, more than one channel chunk
    ("row", 33, 32, 2, 2),          # one tile plus one row
    ("tall", 80, 70, 1, 1),         # three levels above the tile levels, none square
    ("disc", 64, 64, 1, 1),         # an affine function inside a disc of radius 24: the seam figure
    ("levels", 264, 300, 1, 2),     # level 3 is 33 x 38: the adjoint's second launch runs over several tiles too
)


def case_id(case):
    return "%s-%dx%d-B%d-C%d" % case


# measured by measure_yardstick (tests/test_uv_fill_host.py prints them again)
YARDSTICK = {
    "one-1x1-B1-C1": dict(texture=0.0, textures_grad=0.0),
    "odd-5x7-B2-C3": dict(texture=9.6e-08, textures_grad=5.5e-08),
    "tiles-37x50-B3-C9": dict(texture=1.4e-07, textures_grad=9.1e-08),
    "row-33x32-B2-C2": dict(texture=1.7e-07, textures_grad=5.8e-08),
    "tall-80x70-B1-C1": dict(texture=1.4e-07, textures_grad=1.1e-07),
    "disc-64x64-B1-C1": dict(texture=2e-07, textures_grad=5.4e-08),
    "levels-264x300-B1-C2": dict(texture=1.7e-07, textures_grad=1.0e-07),
}
DEVICE_TOLERANCE = {k: 8 * max(y[k] for y in YARDSTICK.values()) for k in KINDS}


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def fuse(x, w):
    """(v0 [H,W,C] with 0 at invalid texels, valid [H,W] bool, counting [B,H,W] bool, sum of the counting weights [H,W])"""
    ok = w > 0
    wv = torch.where(ok, w, torch.zeros_like(w))
    a = torch.zeros_like(x[0])
    m = torch.zeros_like(wv[0])
    started = torch.zeros_like(ok[0])
    for b in range(x.shape[0]):
        term = wv[b][..., None] * x[b]
        a = torch.where(ok[b][..., None], torch.where(started[..., None], a + term, term), a)
        m = torch.where(ok[b], torch.where(started, m + wv[b], wv[b]), m)
        started = started | ok[b]
    v0 = torch.where(started[..., None], a / torch.where(started, m, torch.ones_like(m))[..., None], torch.zeros_like(a))
    return v0, started, ok, m


def pull(s, n):
    h, w = s.shape[:2]
    ph, pw = (h + 1) // 2 * 2, (w + 1) // 2 * 2
    S = torch.zeros(ph, pw, s.shape[2], dtype=s.dtype)
    S[:h, :w] = s
    N = torch.zeros(ph, pw, dtype=n.dtype)
    N[:h, :w] = n
    s2 = ((S[0::2, 0::2] + S[0::2, 1::2]) + S[1::2, 0::2]) + S[1::2, 1::2]
    n2 = ((N[0::2, 0::2] + N[0::2, 1::2]) + N[1::2, 0::2]) + N[1::2, 1::2]
    return s2, n2


def taps(n, n2, dtype):
    p = (torch.arange(n, dtype=dtype) * 0.5 - 0.25).clamp(0, n2 - 1)
    i0 = p.floor().long().clamp(max=max(n2 - 2, 0))
    i1 = (i0 + 1).clamp(max=n2 - 1)
    return i0, i1, p - i0.to(dtype)


def up(c, h, w):
    """the bilinear value of the coarse level c at the centres of an (h, w) level"""
    y0, y1, ty = taps(h, c.shape[0], c.dtype)
    x0, x1, tx = taps(w, c.shape[1], c.dtype)
    ty, tx = ty[:, None, None], tx[None, :, None]
    return (1 - ty) * ((1 - tx) * c[y0][:, x0] + tx * c[y0][:, x1]) + ty * ((1 - tx) * c[y1][:, x0] + tx * c[y1][:, x1])


def fuse_fill(x, w, fill=True, background=None):
    """(texture [H,W,C], valid [H,W] bool) of textures x [B,H,W,C] and weights w [B,H,W] in x's dtype"""
    C = x.shape[-1]
    bg = torch.zeros(C, dtype=x.dtype) if background is None else background.to(x.dtype)
    v0, valid, _, _ = fuse(x, w)
    if not fill:
        return torch.where(valid[..., None], v0, bg.expand_as(v0)), valid
    s, n = [v0], [valid.to(x.dtype)]
    while s[-1].shape[:2] != (1, 1):
        s2, n2 = pull(s[-1], n[-1])
        s.append(s2)
        n.append(n2)
    mean = lambda l: s[l] / n[l].clamp(min=1)[..., None]
    f = torch.where((n[-1] > 0)[..., None], mean(len(s) - 1), bg.expand_as(s[-1]))
    for l in range(len(s) - 2, -1, -1):
        f = torch.where((n[l] > 0)[..., None], mean(l), up(f, *s[l].shape[:2]))
    return f, valid


def evaluate(x, w, g, fill=True, background=None, dtype=torch.float64):
    """dict(texture, valid, textures_grad) of the restatement in `dtype`, the gradient of sum(texture g)"""
    xx = x.to(dtype).clone().requires_grad_(True)
    texture, valid = fuse_fill(xx, w.to(dtype), fill, background)
    grad, = torch.autograd.grad((texture * g.to(dtype)).sum(), xx)
    return dict(texture=texture.detach(), valid=valid, textures_grad=grad)


# ---- the cases' inputs --------------------------------------------------------------------------------------------------------
def seeded_background(C):
    return torch.linspace(0.25, 1.5, C)


def disc_scene(T=64, radius=24.0, dtype=torch.float64):
    """(the affine function [T,T,1], the disc's mask [T,T] bool)"""
    yy, xx = torch.meshgrid(torch.arange(T, dtype=dtype), torch.arange(T, dtype=dtype), indexing="ij")
    f = (0.2 + 0.5 * xx / T + 0.3 * yy / T)[..., None]
    c = (T - 1) / 2
    return f, ((xx - c) ** 2 + (yy - c) ** 2) < radius ** 2


_inputs = {}


def case_inputs(case):
    """dict(textures [B,H,W,C], weights [B,H,W], grad [H,W,C], background [C]) in float32, seeded, computed once.  Weights are
    0 or drawn from [2^-6, 1]: per view a coarse pattern of 5 x 5 cells (2 x 2 on a small texture; so that holes cross tile
    borders and survive several levels) times a per-texel one, with probabilities that leave about half the texels valid for every B."""
    if case not in _inputs:
        name, H, W, B, C = case
        gen = torch.Generator().manual_seed(97 + 1000 * H + 10 * W + B)
        x = torch.rand(B, H, W, C, generator=gen) * 0.8 + 0.2
        g = torch.randn(H, W, C, generator=gen)
        if name == "disc":
            f, mask = disc_scene(H)
            x, w = (f * mask[..., None]).float()[None].contiguous(), mask.float()[None].contiguous()
        elif name == "one":
            w = torch.full((1, 1, 1), 0.5)
        else:
            q = 1 - 0.5 ** (1 / B)                                     # a view's share, for a union of about one half
            cell = 5 if min(H, W) >= 10 else 2
            coarse = torch.rand(B, (H + cell - 1) // cell, (W + cell - 1) // cell, generator=gen) < q / 0.8
            coarse = coarse.repeat_interleave(cell, 1).repeat_interleave(cell, 2)[:, :H, :W]
            on = coarse & (torch.rand(B, H, W, generator=gen) < 0.8)
            w = torch.where(on, 2.0 ** -6 + torch.rand(B, H, W, generator=gen) * (1 - 2.0 ** -6), torch.zeros(B, H, W))
            if name == "odd":
                w[0, 0, 0], w[1, 2, 3] = -0.5, float("nan")           # both count as absent
        _inputs[case] = dict(textures=x, weights=w, grad=g, background=seeded_background(C))
    return _inputs[case]


_references = {}


def reference(case, fill=True):
    """the float64 restatement of a case with its seeded background, computed once and shared"""
    if (case, fill) not in _references:
        a = case_inputs(case)
        _references[(case, fill)] = evaluate(a["textures"], a["weights"], a["grad"], fill, a["background"])
    return _references[(case, fill)]


def relative_error(result, ref):
    """max |result - ref| in units of ref's largest entry"""
    return float((result.detach().cpu().double() - ref.double()).abs().max()) / float(ref.abs().max())


def measure_yardstick(case):
    a = case_inputs(case)
    ref = reference(case)
    low = evaluate(a["textures"], a["weights"], a["grad"], True, a["background"], torch.float32)
    return {k: relative_error(low[k], ref[k]) for k in KINDS}


# ---- the seam figure -------------------------------------------------------------------------------------------------------------
def box(a, levels):
    for _ in range(levels):
        a = 0.25 * (a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2])
    return a


def seam_errors(texture, level):
    """(unfilled, filled): the largest error against the affine function of the disc scene at the level's box-pyramid texels
    that straddle the disc's border, of the masked function itself and of `texture` [64,64,1]"""
    f, mask = disc_scene()
    share = box(mask.double()[..., None], level)[..., 0]
    straddle = (share > 0) & (share < 1)
    true = box(f, level)
    unfilled = float((box(f * mask[..., None], level) - true)[straddle].abs().max())
    filled = float((box(texture.double(), level) - true)[straddle].abs().max())
    return unfilled, filled
