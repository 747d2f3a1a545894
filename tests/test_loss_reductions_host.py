"""The loss reductions (csrc/d3m_aux.h: k_photometric_reduce/_finish, k_sum_squared_error + k_sum_partials,
k_smooth_reduce/_finish/_grad, k_fit_loss_reduce/_finish/_grad) at every grid shape and input layout, host side: the
launchers' grid arithmetic restated, the cases of tests/test_gpu_loss_reductions.py with the path each of them takes, their
inputs (position hashes), their references, and the proof that the float cases are sharp.  No GPU.

Integer cases.  Inputs are small integers, masks small non-negative integers; every term that is summed is a non-negative
integer and every total is asserted below 2^24 (int64), so every partial sum is exact in float32 in any order.  What the
kernels must give is then formed here in np.float32 with their own final expressions -- the library is compiled with
-ffp-contract=off, so these are predictions of bits.

Float cases (photometric with conf_sigma: a division and a logf per term; one plain float case per kernel family).  The
reference is float64 and the tolerance (D 2^-24 + 4 E32) * bound:
  bound  the float64 sum of |term| behind the loss (the two summands of the sigma form taken separately), through the
         loss's own final expression;
  D      the longest chain of additions behind a sum: a lane's passes (4 additions per pass on the float4 path, 3 for the
         fit objective's colour sum), the 6 butterfly steps of wave_sum, the 3 additions of block_sum_256, the finish
         kernel's ceil(partials / 256) passes and 6 + 3 again.  A quotient of two such sums takes the chain twice and one
         rounding of the division (2 D + 1); the sums of several quotients the roundings of their final expression on top
         (SMOOTH_FINAL, FIT_FINAL);
  E32    |loss32 - loss| / bound, loss32 being the same reference evaluated in np.float32 (numpy sums pairwise: what is
         left is the arithmetic of the terms); the factor 4 because the kernels associate the sums differently.
Nothing in it comes from the kernels' output.

Sharpness.  Removing any aligned group of 4 consecutive elements of any plane from the sums moves a float case's loss by
more than its tolerance (test_float_cases_are_sharp).  A dropped element leaves the numerator and the denominator of a mean
together, so the terms of a group must not average to the loss itself: every group's terms lie in one of two bands, [2, 3]
or [5, 7], and the loss between them.  Four photometric shapes hold 1.8 to 4.2 million elements (all of them on the capped
grid); four elements are about 2e-6 of their bound and cannot show beside D 2^-24.  For those the granularity is one
workgroup pass, 1024 consecutive elements (a plane's last, shorter run counted with the pass before it); the element-level
coverage of the same loops comes from the integer cases, which are exact at every size."""
import collections
import math
import os
import re
import zlib

import numpy as np
import pytest

from pose_scenes import hashed_floats, hashed_ints

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = 2.0 ** -24
LANES = 256
EXACT_LIMIT = 1 << 24
SQRT2_F32 = np.float32(1.41421356237309515)        # the kernels' constant
SIGMA_EPS = 1e-7                                    # utils.py's EPS
# what core/losses.py allocates for each entry point: exactly the launchers' caps
SCRATCH_FLOATS = {"photometric": 2048, "sse": 1024, "smooth": 4096, "fit": 4104}
GRAD_LOSS = np.float32(0.3)                         # not a power of two
SHARP_ELEMENTS = 20000                              # above: sharpness per workgroup pass, not per 4 elements
SMOOTH_FINAL, FIT_FINAL = 6, 4                      # roundings of the final expressions beside the quotients' own


def ceil_div(a, b):
    return -(-a // b)


# ---- the launchers' grid arithmetic (csrc/d3m_raster.hip, section C and fit_loss_grid) -----------------------------------------
def photometric_gx(planes, hw):
    """workgroups per plane, or None where the launcher refuses"""
    if planes > 65535:
        return None
    gx = min(ceil_div(hw, 2048), 1 if planes >= 1024 else 1024 // planes)
    return gx if planes * gx <= 1024 else None


def photometric_grid(planes, hw):
    gx = photometric_gx(planes, hw)
    return None if gx is None else planes * gx


def sse_grid(n):
    return min(ceil_div(n, 2048), 1024)


def smooth_grid(n):
    return min(ceil_div(n, 1024), 1024)


def fit_gx(B, hw):
    return None if B > 1024 else max(1, min(ceil_div(hw, 1024), 1024 // B))


def fit_grid(B, hw):
    gx = fit_gx(B, hw)
    return None if gx is None else B * gx


def finish_chain(partials):
    """the finish kernel: a lane's i += 256 passes, wave_sum, block_sum_256"""
    return ceil_div(partials, LANES) + 6 + 3


def photometric_chain(planes, hw, vector):
    gx = photometric_gx(planes, hw)
    lane = 4 * ceil_div(hw // 4, gx * LANES) if vector else ceil_div(hw, gx * LANES)
    return lane + 6 + 3 + finish_chain(planes * gx)


def sse_chain(n, vector):
    g = sse_grid(n)
    lane = 4 * ceil_div(n // 4, g * LANES) + (1 if n % 4 else 0) if vector else ceil_div(n, g * LANES)
    return lane + 6 + 3 + finish_chain(g)


def smooth_chain(n):
    g = smooth_grid(n)
    return ceil_div(n, g * LANES) + 6 + 3 + finish_chain(g)


def fit_chain(B, hw):
    gx = fit_gx(B, hw)
    return 3 * ceil_div(hw, gx * LANES) + 6 + 3 + finish_chain(B * gx)


def _grid_kind(grid, wanted):
    """"one" workgroup (per plane), "many" (as many as the size asks for) or "capped" (fewer: lanes take more passes)"""
    return "capped" if grid < wanted else ("one" if grid == 1 else "many")


# ---- cases ---------------------------------------------------------------------------------------------------------------------
PhotoCase = collections.namedtuple("PhotoCase", "B C H W mask sigma off")
SseCase = collections.namedtuple("SseCase", "n off")
SmoothCase = collections.namedtuple("SmoothCase", "B H W")
FitCase = collections.namedtuple("FitCase", "B H W")

PHOTO_SHAPES = ((1, 1, 1, 1), (1, 3, 5, 7), (2, 3, 17, 15), (1, 1, 16, 16), (1, 1, 257, 1),
                (1, 2, 32, 64), (1, 2, 1, 2049), (1, 2, 1, 2052),
                (16, 3, 208, 208),
                (100, 3, 1, 6148), (100, 3, 1, 6149),
                (1024, 1, 1, 5), (1024, 1, 41, 100))
PHOTO_REFUSED = ((1025, 1, 1, 5), (342, 3, 1, 1))
PHOTO_OFF_SHAPES = ((2, 3, 16, 16), (1, 2, 1, 2052))
PHOTO_FLOAT_PLAIN = (2, 3, 17, 15)
SSE_SIZES = (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 2097152, 2099203)
SSE_OFF_SIZES = (1025, 2049)
SSE_FLOAT = 2049
SMOOTH_SHAPES = ((1, 3, 3), (1, 3, 4), (1, 4, 3), (3, 17, 5), (2, 3, 400), (2, 400, 3), (1, 32, 32), (1, 41, 25), (2, 33, 31),
                 (1, 513, 512), (1, 1025, 1024))
SMOOTH_REFUSED = ((1, 2, 5), (1, 5, 2))
SMOOTH_FLOAT = (2, 33, 31)
FIT_SHAPES = ((1, 1, 1), (1, 31, 33), (1, 32, 32), (1, 25, 41), (3, 20, 12), (32, 182, 181), (300, 7, 439), (1024, 1, 5))
FIT_REFUSED = ((1025, 1, 5),)
FIT_FLOAT = (3, 20, 12)


def photo_cases():
    """Every shape with mask and conf_sigma in all four combinations; at PHOTO_OFF_SHAPES each operand in turn 4 bytes off a
    16-byte boundary, with a mask, without and with conf_sigma"""
    cases = [PhotoCase(*s, m, sg, None) for s in PHOTO_SHAPES for m in (0, 1) for sg in (0, 1)]
    for s in PHOTO_OFF_SHAPES:
        for sg in (0, 1):
            for off in ("im1", "im2", "mask") + (("sigma",) if sg else ()) + ("grad",):
                cases.append(PhotoCase(*s, 1, sg, off))
    return cases


def sse_cases():
    return [SseCase(n, None) for n in SSE_SIZES] + [SseCase(n, off) for n in SSE_OFF_SIZES for off in ("a", "b", "grad")]


def smooth_cases():
    return [SmoothCase(*s) for s in SMOOTH_SHAPES]


def fit_cases():
    return [FitCase(*s) for s in FIT_SHAPES]


def case_id(c):
    return type(c).__name__[:-4].lower() + "-" + "-".join(str(v) if v is not None else "aligned" for v in c)


def _salt(c):
    return zlib.crc32(case_id(c).encode()) % 9973


def variants(c):
    """the input variants a case runs with: two integer-exact ones, or the float ones"""
    if isinstance(c, PhotoCase):
        if c.sigma:
            return ("sigma_above_one", "sigma_below_one")
        plain = tuple(c[:4]) == PHOTO_FLOAT_PLAIN and c.mask and c.off is None
        return ("dense", "zeros") + (("float",) if plain else ())
    floats = {SseCase: c == SseCase(SSE_FLOAT, None), SmoothCase: tuple(c) == SMOOTH_FLOAT, FitCase: tuple(c) == FIT_FLOAT}
    return ("dense", "zeros") + (("float",) if floats[type(c)] else ())


def is_float(variant):
    return variant not in ("dense", "zeros")


def float_cases():
    return [(c, v) for c in photo_cases() + sse_cases() + smooth_cases() + fit_cases() for v in variants(c) if is_float(v)]


# ---- which path a case takes -----------------------------------------------------------------------------------------------------
def photo_vector(c, kernel):
    """whether k_photometric_reduce ("reduce") / the gradient loop of k_photometric_finish ("finish") stream float4"""
    reads = ("im1", "im2", "mask", "sigma") + (("grad",) if kernel == "finish" else ())
    return (c.H * c.W) % 4 == 0 and c.off not in reads


def sse_vector(c):
    return c.off is None


def paths(c):
    """(vector path, grid kind, the finish kernel adds more than 256 partials)"""
    if isinstance(c, PhotoCase):
        planes, hw = c.B * c.C, c.H * c.W
        gx = photometric_gx(planes, hw)
        return photo_vector(c, "reduce"), _grid_kind(gx, ceil_div(hw, 2048)), planes * gx > LANES
    if isinstance(c, SseCase):
        return sse_vector(c), _grid_kind(sse_grid(c.n), ceil_div(c.n, 2048)), sse_grid(c.n) > LANES
    if isinstance(c, SmoothCase):
        n = c.B * c.H * c.W
        return False, _grid_kind(smooth_grid(n), ceil_div(n, 1024)), smooth_grid(n) > LANES
    hw = c.H * c.W
    gx = fit_gx(c.B, hw)
    return False, _grid_kind(gx, ceil_div(hw, 1024)), c.B * gx > LANES


def chain(c):
    if isinstance(c, PhotoCase):
        return photometric_chain(c.B * c.C, c.H * c.W, photo_vector(c, "reduce"))
    if isinstance(c, SseCase):
        return sse_chain(c.n, sse_vector(c))
    if isinstance(c, SmoothCase):
        return smooth_chain(c.B * c.H * c.W)
    return fit_chain(c.B, c.H * c.W)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def _flat(fn, n, salt, *args, cols=4099):
    """n hashed values as the rows of a [.., 4099] grid laid end to end (a single row would repeat after 65 521 positions)"""
    return fn(ceil_div(n, cols), cols, salt, *args).reshape(-1)[:n]


def _signed_ints(rows, cols, salt):
    """+-1, +-2, +-3 from two hashes: no zero, and neighbours differ in size, so that an element dropped and another taken
    twice do not cancel"""
    return hashed_ints(rows, cols, salt, 1, 3) * (2 * hashed_ints(rows, cols, salt + 1, 0, 1) - 1)


def _int_mask(rows, cols, salt, zeros):
    m = hashed_ints(rows, cols, salt, 1, 2)
    if zeros:
        m = m * (hashed_ints(rows, cols, salt + 1, 0, 3) != 0)
        if not m.any():
            m[0, 0] = 1            # (a mean over an empty mask is 0 / 0)
    return m


def _bands(rows, cols, salt, span):
    """[rows, cols] float64: every aligned run of `span` columns in one of two bands, [2, 3] or [5, 7]"""
    mode = np.repeat(hashed_ints(rows, ceil_div(cols, span), salt, 0, 1), span, axis=1)[:, :cols]
    u = hashed_floats(rows, cols, salt + 1, 0.0, 1.0, np.float64)
    return np.where(mode == 0, 2.0 + u, 5.0 + 2.0 * u)


def _float_signs(rows, cols, salt):
    return (2 * hashed_ints(rows, cols, salt, 0, 1) - 1).astype(np.float64)


def sharp_span(c):
    """elements per group of the sharpness statement"""
    return 1024 if isinstance(c, PhotoCase) and c.B * c.C * c.H * c.W > SHARP_ELEMENTS else 4


def photo_inputs(c, variant):
    """im1, im2 [B*C, H*W], mask, sigma [B, H*W] or None: int64 for the integer variants, float32 for the float ones"""
    planes, hw, salt = c.B * c.C, c.H * c.W, _salt(c)
    if not is_float(variant):
        d = _signed_ints(planes, hw, salt + 1)
        if variant == "zeros":
            d = d * (hashed_ints(planes, hw, salt + 3, 0, 2) != 0)
        im2 = hashed_ints(planes, hw, salt + 4, -4, 4)
        mask = _int_mask(c.B, hw, salt + 5, variant == "zeros") if c.mask else None
        return dict(im1=im2 + d, im2=im2, mask=mask, sigma=None)
    target = _bands(planes, hw, salt + 7, sharp_span(c))              # the term of every element
    mask = hashed_floats(c.B, hw, salt + 9, 0.5, 1.5) if c.mask else None
    sigma = None
    if c.sigma:
        lo, hi = (1.5, 3.0) if variant == "sigma_above_one" else (0.1, 0.6)
        sigma = hashed_floats(c.B, hw, salt + 10, lo, hi)
        sg = np.repeat(sigma.astype(np.float64) + SIGMA_EPS, c.C, axis=0)
        target = (target - np.log(sg)) * sg / math.sqrt(2.0)          # |im1 - im2| that gives the term
    im2 = hashed_floats(planes, hw, salt + 4)
    im1 = (im2.astype(np.float64) + _float_signs(planes, hw, salt + 11) * target).astype(np.float32)
    return dict(im1=im1, im2=im2, mask=mask, sigma=sigma)


def sse_inputs(c, variant):
    n, salt = c.n, _salt(c)
    if not is_float(variant):
        d = _flat(_signed_ints, n, salt + 1)
        if variant == "zeros":
            d = d * (_flat(hashed_ints, n, salt + 3, 0, 2) != 0)
        b = _flat(hashed_ints, n, salt + 4, -4, 4)
        return dict(a=b + d, b=b)
    b = _flat(hashed_floats, n, salt + 4)
    d = _flat(hashed_floats, n, salt + 5, 0.5, 1.0, np.float64) * _flat(_float_signs, n, salt + 6)
    return dict(a=(b.astype(np.float64) + d).astype(np.float32), b=b)


def smooth_inputs(c, variant):
    """pred [B, H, W]; the rows of the B images are hashed as one column of B*H rows, so every image differs.  "zeros": a
    plateau of at least 2 x 2 in every image, whose second differences are exactly zero"""
    salt = _salt(c)
    if is_float(variant):
        # (a hash is linear in the position between its wrap-arounds: the product of two has second differences)
        a, b = (hashed_floats(c.B * c.H, c.W, salt + s, -1.0, 1.0, np.float64) for s in (1, 2))
        return dict(pred=(a * b).astype(np.float32).reshape(c.B, c.H, c.W))
    p = hashed_ints(c.B * c.H, c.W, salt + 1, 0, 3).reshape(c.B, c.H, c.W)
    if variant == "zeros":
        y0, x0 = c.H // 3, c.W // 3
        p[:, y0:y0 + ceil_div(c.H, 2), x0:x0 + ceil_div(c.W, 2)] = 2
    return dict(pred=p)


FIT_NAMES = ("rgb", "rgb_t", "depth", "depth_t", "alpha", "alpha_t", "mask")


def fit_inputs(c, variant):
    """rgb, rgb_t [B, 3, H*W]; depth, alpha, their targets and the mask [B, H*W]"""
    B, hw, salt = c.B, c.H * c.W, _salt(c)
    if not is_float(variant):
        zeros = variant == "zeros"
        keep = (lambda rows, s: hashed_ints(rows, hw, s, 0, 2) != 0) if zeros else (lambda rows, s: 1)
        rgb_t, depth_t, alpha_t = (hashed_ints(r, hw, salt + s, -4, 4) for r, s in ((3 * B, 1), (B, 2), (B, 3)))
        return dict(rgb=(rgb_t + _signed_ints(3 * B, hw, salt + 4) * keep(3 * B, salt + 6)).reshape(B, 3, hw),
                    rgb_t=rgb_t.reshape(B, 3, hw), depth=depth_t + _signed_ints(B, hw, salt + 7) * keep(B, salt + 9),
                    depth_t=depth_t, alpha=alpha_t + _signed_ints(B, hw, salt + 10) * keep(B, salt + 12), alpha_t=alpha_t,
                    mask=_int_mask(B, hw, salt + 13, zeros))
    # the colour and depth terms of a group of 4 pixels in the same band; the silhouette term small beside them
    mode = np.repeat(hashed_ints(B, ceil_div(hw, 4), salt + 15, 0, 1), 4, axis=1)[:, :hw]

    def band(rows, s):
        u = hashed_floats(rows, hw, s, 0.0, 1.0, np.float64)
        return np.where(np.repeat(mode, rows // B, axis=0) == 0, 2.0 + u, 5.0 + 2.0 * u) * _float_signs(rows, hw, s + 1)
    rgb_t, depth_t, alpha_t = (hashed_floats(r, hw, salt + s) for r, s in ((3 * B, 1), (B, 2), (B, 3)))
    d_alpha = hashed_floats(B, hw, salt + 20, 0.1, 0.2, np.float64) * _float_signs(B, hw, salt + 21)
    f32 = lambda t, d: (t.astype(np.float64) + d).astype(np.float32)      # noqa: E731
    return dict(rgb=f32(rgb_t, band(3 * B, salt + 16)).reshape(B, 3, hw), rgb_t=rgb_t.reshape(B, 3, hw),
                depth=f32(depth_t, band(B, salt + 18)), depth_t=depth_t, alpha=f32(alpha_t, d_alpha), alpha_t=alpha_t,
                mask=hashed_floats(B, hw, salt + 13, 0.5, 1.5))


def foreign_mask_sum(inp):
    """a `mask_sum` as the other shards' masks would make it: about one and a half times the mask's own sum (float32; far
    enough from it to show in a loss that the silhouette term dominates)"""
    own = np.float32(inp["mask"].astype(np.float64).sum())
    return np.float32(own + np.float32(np.floor(own / np.float32(2.0))) + np.float32(7.0))


# ---- what the kernels must give -----------------------------------------------------------------------------------------------------
def _exact(total):
    total = int(total)
    assert 0 <= total < EXACT_LIMIT, total
    return np.float32(total)


def _plane_rows(x, C):
    """[B, hw] -> [B*C, hw]: plane b*C + c reads row b"""
    return np.repeat(x, C, axis=0)


def smooth_counts(c):
    n_xx, n_xy, n_yy = c.B * c.H * (c.W - 2), c.B * (c.H - 1) * (c.W - 1), c.B * (c.H - 2) * c.W
    assert max(n_xx, n_xy, n_yy) < EXACT_LIMIT
    return np.float32(n_xx), np.float32(n_xy), np.float32(n_yy)


def smooth_differences(p):
    """the reference's nested first differences in p's dtype, the kernels' order of subtractions: dxx, dxy, dyx, dyy"""
    dxx = (p[:, :, 2:] - p[:, :, 1:-1]) - (p[:, :, 1:-1] - p[:, :, :-2])
    dxy = (p[:, 1:, 1:] - p[:, 1:, :-1]) - (p[:, :-1, 1:] - p[:, :-1, :-1])
    dyx = (p[:, 1:, 1:] - p[:, :-1, 1:]) - (p[:, 1:, :-1] - p[:, :-1, :-1])
    dyy = (p[:, 2:, :] - p[:, 1:-1, :]) - (p[:, 1:-1, :] - p[:, :-2, :])
    return dxx, dxy, dyx, dyy


def smooth_gradient(c, diffs, grad_loss):
    """k_smooth_grad in np.float32 from the differences' signs: the sums of signed coefficients are small integers"""
    sxx, sxy, syx, syy = (np.sign(d).astype(np.int64) for d in diffs)
    gxx, gxy, gyy = (np.zeros((c.B, c.H, c.W), np.int64) for _ in range(3))
    gxx[:, :, :-2] += sxx
    gxx[:, :, 1:-1] -= 2 * sxx
    gxx[:, :, 2:] += sxx
    gyy[:, :-2] += syy
    gyy[:, 1:-1] -= 2 * syy
    gyy[:, 2:] += syy
    s = sxy + syx
    gxy[:, :-1, :-1] += s
    gxy[:, :-1, 1:] -= s
    gxy[:, 1:, :-1] -= s
    gxy[:, 1:, 1:] += s
    n_xx, n_xy, n_yy = smooth_counts(c)
    f = lambda g: g.astype(np.float32)      # noqa: E731
    return np.float32(grad_loss) * ((f(gxx) / n_xx + f(gxy) / n_xy) + f(gyy) / n_yy)


def exact_expected(c, inp, mask_sum=None, grad_out=None):
    """loss and gradients of an integer case, float32, bit for bit"""
    if isinstance(c, PhotoCase):
        d = inp["im1"] - inp["im2"]
        m = _plane_rows(inp["mask"], c.C) if c.mask else np.ones_like(d)
        den = _exact(m.sum())
        # (sign and mask multiplied in float32, as the kernel does: -1 * 0 is -0)
        return dict(loss=_exact((np.abs(d) * m).sum()) / den, grad=np.sign(d).astype(np.float32) * m.astype(np.float32) / den)
    if isinstance(c, SseCase):
        d = inp["a"] - inp["b"]
        return dict(loss=_exact((d * d).sum()), grad=(2 * d).astype(np.float32))
    if isinstance(c, SmoothCase):
        diffs = smooth_differences(inp["pred"])
        a = [_exact(np.abs(d).sum()) for d in diffs]
        n_xx, n_xy, n_yy = smooth_counts(c)
        return dict(loss=((a[0] / n_xx + a[1] / n_xy) + a[2] / n_xy) + a[3] / n_yy,
                    grad=smooth_gradient(c, diffs, GRAD_LOSS))
    m = inp["mask"]
    d_rgb, d_depth, d_alpha = inp["rgb"] - inp["rgb_t"], inp["depth"] - inp["depth_t"], inp["alpha"] - inp["alpha_t"]
    a0, a1 = _exact((np.abs(d_rgb) * m[:, None]).sum()), _exact((np.abs(d_depth) * m).sum())
    a2, a3 = _exact(m.sum()), _exact((d_alpha * d_alpha).sum())
    if mask_sum is not None:
        a2 = np.float32(mask_sum)
    pixels, go = np.float32(c.H * c.W), np.float32(1.0 if grad_out is None else grad_out)
    f = lambda x: x.astype(np.float32)      # noqa: E731
    return dict(loss=(a0 / (np.float32(3.0) * a2) + a3 / pixels) + a1 / a2,
                g_rgb=f(np.sign(d_rgb)) * f(m[:, None]) / (np.float32(3.0) * a2) * go,
                g_depth=f(np.sign(d_depth)) * f(m) / a2 * go, g_alpha=f(2 * d_alpha) / pixels * go)


class FloatReference:
    """loss (float64), bound, loss32, e32, D, tol of a float case; `moves`: how far the loss goes when one group of
    sharp_span(c) consecutive elements of a plane is left out of every sum; the gradients and their tolerances.

    A gradient entry is a few roundings of its own and the relative error of the denominator it divides by, a sum of
    positive inputs with a chain of `chain(c)` additions: (chain + GRAD_OWN) 2^-24 |entry|.  Where no summed denominator
    enters (sum of squares, smooth, a given mask_sum) the float32 arithmetic of the entry is reproduced here and the
    gradient is a prediction of bits (tolerance None)."""
    GRAD_OWN = 8

    def __init__(self, c, inp, mask_sum=None, grad_out=None):
        self.c, span = c, sharp_span(c)
        f64 = {k: None if v is None else v.astype(np.float64) for k, v in inp.items()}

        def groups(x):          # [planes, hw] -> [planes, groups]: the sum of every aligned group of a plane
            pad = (-x.shape[1]) % span
            g = np.pad(x, ((0, 0), (0, pad))).reshape(x.shape[0], -1, span).sum(2)
            if span > 4 and pad and g.shape[1] > 1:       # a plane's last, shorter run of a pass goes with the pass before it
                g = np.concatenate([g[:, :-2], g[:, -2:].sum(1, keepdims=True)], 1)
            return g
        if isinstance(c, PhotoCase):
            self.D = 2 * chain(c) + 1
            d = f64["im1"] - f64["im2"]
            m = _plane_rows(f64["mask"], c.C) if c.mask else np.ones_like(d)
            scale = np.ones_like(d)
            term = bound = np.abs(d)
            if c.sigma:
                sg = _plane_rows(f64["sigma"], c.C) + SIGMA_EPS
                scale = math.sqrt(2.0) / sg
                term, bound = np.abs(d) * scale + np.log(sg), np.abs(d) * scale + np.abs(np.log(sg))
            num, den = (term * m).sum(), m.sum()
            self.loss, self.bound = num / den, (bound * m).sum() / den
            with np.errstate(divide="ignore", invalid="ignore"):
                self.moves = np.abs((num - groups(term * m)) / (den - groups(m)) - self.loss)
            self.grad = dict(grad=np.sign(d) * scale * m / den)
            self.grad_tol = dict(grad=(chain(c) + self.GRAD_OWN) * EPS32 * np.abs(self.grad["grad"]))
            a, b = inp["im1"], inp["im2"]
            l32 = np.abs(a - b)
            if c.sigma:
                sg32 = _plane_rows(inp["sigma"], c.C) + np.float32(SIGMA_EPS)
                l32 = l32 * SQRT2_F32 / sg32 + np.log(sg32)
            m32 = _plane_rows(inp["mask"], c.C) if c.mask else np.ones_like(a)
            self.loss32 = (l32 * m32).sum(dtype=np.float32) / m32.sum(dtype=np.float32)
        elif isinstance(c, SseCase):
            self.D = chain(c)
            d = (f64["a"] - f64["b"])[None]
            self.loss = self.bound = (d * d).sum()
            self.moves = groups(d * d)
            d32 = inp["a"] - inp["b"]
            self.loss32 = (d32 * d32).sum(dtype=np.float32)
            self.grad, self.grad_tol = dict(grad=np.float32(2.0) * d32), dict(grad=None)
        elif isinstance(c, SmoothCase):
            self.D = 2 * chain(c) + SMOOTH_FINAL        # (the counts are exact: the chain once would do; kept uniform)
            counts = [float(x) for x in smooth_counts(c)]
            weights = (counts[0], counts[1], counts[1], counts[2])

            def evaluate(p, dtype):
                total, per_element = dtype(0), np.zeros((c.B, c.H, c.W), dtype)
                for d, w, (hy, hx) in zip(smooth_differences(p), weights, ((c.H, c.W - 2), (c.H - 1, c.W - 1),
                                                                          (c.H - 1, c.W - 1), (c.H - 2, c.W))):
                    total = total + np.abs(d).sum(dtype=dtype) / dtype(w)
                    per_element[:, :hy, :hx] += np.abs(d) / dtype(w)       # (the lane of element (y, x) adds the term)
                return total, per_element
            self.loss, per_element = evaluate(f64["pred"], np.float64)
            self.bound = self.loss
            self.moves = groups(per_element.reshape(c.B, -1))
            self.loss32, _ = evaluate(inp["pred"], np.float32)
            self.grad = dict(grad=smooth_gradient(c, smooth_differences(inp["pred"]), GRAD_LOSS))
            self.grad_tol = dict(grad=None)
        else:
            self.D = 2 * chain(c) + FIT_FINAL
            pixels, go = float(c.H * c.W), 1.0 if grad_out is None else float(np.float32(grad_out))

            def evaluate(x, dtype, grouped):
                m = x["mask"]
                d_rgb, d_depth, d_alpha = x["rgb"] - x["rgb_t"], x["depth"] - x["depth_t"], x["alpha"] - x["alpha_t"]
                t = [(np.abs(d_rgb) * m[:, None]).sum(1), np.abs(d_depth) * m, m, d_alpha * d_alpha]
                a = [v.sum(dtype=dtype) for v in t]
                own = a[2]
                if mask_sum is not None:
                    a[2] = dtype(mask_sum)
                loss = (a[0] / (dtype(3.0) * a[2]) + a[3] / dtype(pixels)) + a[1] / a[2]
                if not grouped:
                    return loss
                g = [groups(v) for v in t]
                den = a[2] - (g[2] if mask_sum is None else 0.0)
                with np.errstate(divide="ignore", invalid="ignore"):
                    moved = ((a[0] - g[0]) / (3.0 * den) + (a[3] - g[3]) / pixels) + (a[1] - g[1]) / den
                return loss, np.abs(moved - loss), a, own, (d_rgb, d_depth, d_alpha, m)
            self.loss, self.moves, a, own, (d_rgb, d_depth, d_alpha, m) = evaluate(f64, np.float64, True)
            self.bound, self.own_mask_sum = self.loss, own            # (every term is non-negative)
            self.loss32 = evaluate(inp, np.float32, False)
            self.grad = dict(g_rgb=np.sign(d_rgb) * m[:, None] / (3.0 * a[2]) * go, g_depth=np.sign(d_depth) * m / a[2] * go,
                             g_alpha=2.0 * d_alpha / pixels * go)
            rel = ((0 if mask_sum is not None else chain(c)) + self.GRAD_OWN) * EPS32
            self.grad_tol = {k: rel * np.abs(v) for k, v in self.grad.items()}
        self.e32 = abs(float(self.loss32) - float(self.loss)) / float(self.bound)
        self.tol = (self.D * EPS32 + 4 * self.e32) * float(self.bound)


def inputs(c, variant):
    return {PhotoCase: photo_inputs, SseCase: sse_inputs, SmoothCase: smooth_inputs, FitCase: fit_inputs}[type(c)](c, variant)


def float_reference(c, variant, inp=None, **kw):
    return FloatReference(c, inputs(c, variant) if inp is None else inp, **kw)


# ---- the grid arithmetic and the caps ----------------------------------------------------------------------------------------------
def test_grids_of_the_listed_shapes():
    assert [photometric_gx(b * ch, h * w) for b, ch, h, w in PHOTO_SHAPES] == [1, 1, 1, 1, 1, 1, 2, 2, 21, 3, 3, 1, 1]
    assert [photometric_grid(b * ch, h * w) for b, ch, h, w in PHOTO_SHAPES[8:]] == [1008, 900, 900, 1024, 1024]
    assert [photometric_grid(b * ch, h * w) for b, ch, h, w in PHOTO_REFUSED] == [None, None]
    assert [sse_grid(n) for n in SSE_SIZES] == [1] * 12 + [2, 1024, 1024]
    assert [smooth_grid(b * h * w) for b, h, w in SMOOTH_SHAPES] == [1, 1, 1, 1, 3, 3, 1, 2, 2, 257, 1024]
    assert [fit_gx(b, h * w) for b, h, w in FIT_SHAPES] == [1, 1, 1, 2, 1, 32, 3, 1]
    assert [fit_grid(b, h * w) for b, h, w in FIT_SHAPES] == [1, 1, 1, 2, 3, 1024, 900, 1024]
    assert fit_grid(*FIT_REFUSED[0][:1], 5) is None
    # lanes' passes where the grid is capped: more than the two (photometric, float4) or four (fit, smooth) of a free grid
    assert ceil_div(208 * 208 // 4, 21 * LANES) == 3 and ceil_div(6149, 3 * LANES) == 9 and ceil_div(4100 // 4, LANES) == 5
    assert ceil_div(182 * 181, 32 * LANES) == 5 and ceil_div(1025 * 1024, 1024 * LANES) == 5
    assert ceil_div(2099203 // 4, 1024 * LANES) == 3 and ceil_div(2097152 // 4, 1024 * LANES) == 2


def test_no_grid_outgrows_the_scratch_the_wrappers_allocate():
    for planes in range(1, 1100):
        for hw in (1, 5, 2048, 2049, 4100, 43264, 2 ** 31 - 1):
            g = photometric_grid(planes, hw)
            assert (g is None) == (planes > 1024), (planes, hw)
            assert g is None or 2 * g <= SCRATCH_FLOATS["photometric"]
            f = fit_grid(planes, hw)
            assert (f is None) == (planes > 1024)
            assert f is None or 8 + 4 * f <= SCRATCH_FLOATS["fit"]
    for n in (1, 2048, 2049, 2097152, 2097153, 2 ** 31 - 1):
        assert sse_grid(n) <= SCRATCH_FLOATS["sse"] and 4 * smooth_grid(n) <= SCRATCH_FLOATS["smooth"]
    # ... and the caps are reached: the scratch is not larger than a case needs
    assert 2 * photometric_grid(1024, 5) == SCRATCH_FLOATS["photometric"] and sse_grid(2097152) == SCRATCH_FLOATS["sse"]
    assert 4 * smooth_grid(1025 * 1024) == SCRATCH_FLOATS["smooth"] and 8 + 4 * fit_grid(1024, 5) == SCRATCH_FLOATS["fit"]


def test_the_wrappers_allocate_the_scratch_sizes_assumed_here():
    with open(os.path.join(ROOT, "deep3dmap_amd", "core", "losses.py")) as f:
        src = f.read()
    sizes = [int(n) for n in re.findall(r"scratch = torch\.empty\((\d+),", src)]
    assert sizes == [SCRATCH_FLOATS[k] for k in ("photometric", "sse", "fit", "smooth")], sizes


def test_every_listed_shape_takes_the_path_it_is_listed_for():
    """(float4 loop, grid kind, the finish kernel adds more than 256 partials) of every aligned case, shape by shape"""
    T, F = True, False
    photo = [(F, "one", F), (F, "one", F), (F, "one", F), (T, "one", F), (F, "one", F),
             (T, "one", F), (F, "many", F), (T, "many", F),
             (T, "capped", T),
             (T, "capped", T), (F, "capped", T),
             (F, "one", T), (T, "capped", T)]
    for shape, want in zip(PHOTO_SHAPES, photo):
        for m in (0, 1):
            for sg in (0, 1):
                assert paths(PhotoCase(*shape, m, sg, None)) == want, shape
    sse = [(T, "one", F)] * 12 + [(T, "many", F), (T, "many", T), (T, "capped", T)]
    assert [paths(SseCase(n, None)) for n in SSE_SIZES] == sse
    assert [paths(c) for c in sse_cases() if c.off] == [(F, "one", F)] * 3 + [(F, "many", F)] * 3
    smooth = [("one", F)] * 4 + [("many", F)] * 2 + [("one", F), ("many", F), ("many", F), ("many", T), ("capped", T)]
    assert [paths(c)[1:] for c in smooth_cases()] == smooth
    fit = [("one", F)] * 3 + [("many", F), ("one", F), ("capped", T), ("capped", T), ("one", T)]
    assert [paths(c)[1:] for c in fit_cases()] == fit


def test_cases_cover_every_path():
    photo = {(paths(c), bool(c.mask), bool(c.sigma)) for c in photo_cases() if c.off is None}
    for vector in (False, True):
        for grid in ("one", "many", "capped"):
            for m in (False, True):
                for s in (False, True):
                    assert any(p[:2] == (vector, grid) and (pm, ps) == (m, s) for p, pm, ps in photo), (vector, grid, m, s)
    for long_finish in (False, True):
        assert {p[0] for p, _, _ in photo if p[2] == long_finish} == {False, True}
    assert {(b * ch) for b, ch, _, _ in PHOTO_SHAPES} >= {1024} and photometric_grid(1024, 4100) == 1024
    # misaligned: the scalar loops at a size that is a multiple of 4, for every operand in turn
    for shape in PHOTO_OFF_SHAPES:
        assert (shape[2] * shape[3]) % 4 == 0
        for sg in (0, 1):
            offs = {c.off for c in photo_cases() if tuple(c[:4]) == shape and c.sigma == sg and c.off}
            assert offs == {"im1", "im2", "mask", "grad"} | ({"sigma"} if sg else set())
    for c in photo_cases():
        if c.off:
            assert not photo_vector(c, "finish") and photo_vector(c, "reduce") == (c.off == "grad")
    sse = {paths(c) for c in sse_cases()}
    assert {(True, "one", False), (True, "many", False), (True, "many", True), (True, "capped", True), (False, "one", False),
            (False, "many", False)} <= sse
    assert any(c.n % 4 and c.n > 4 for c in sse_cases()) and any(c.n < 4 for c in sse_cases())      # the scalar tail, alone too
    smooth = {paths(c)[1:] for c in smooth_cases()}
    assert smooth == {("one", False), ("many", False), ("many", True), ("capped", True)}
    fit = {paths(c)[1:] for c in fit_cases()}
    assert fit == {("one", False), ("many", False), ("capped", True), ("one", True)}
    # every family has its float case, the photometric one both sigma ranges at every shape
    fl = float_cases()
    assert {type(c) for c, _ in fl} == {PhotoCase, SseCase, SmoothCase, FitCase}
    for shape in PHOTO_SHAPES:
        for m in (0, 1):
            assert {v for c, v in fl if c == PhotoCase(*shape, m, 1, None)} == {"sigma_above_one", "sigma_below_one"}


# ---- the integer cases are exact and say something ------------------------------------------------------------------------------------
def _all_cases():
    return photo_cases() + sse_cases() + smooth_cases() + fit_cases()


@pytest.mark.parametrize("c", _all_cases(), ids=case_id)
def test_integer_inputs_are_exact_and_dense(c):
    for variant in ("dense", "zeros"):
        if variant not in variants(c):
            continue
        inp = inputs(c, variant)
        want = exact_expected(c, inp)          # (asserts every total below 2^24)
        assert all(v is None or v.dtype == np.int64 for v in inp.values())
        assert np.isfinite(want["loss"])
        if isinstance(c, PhotoCase):
            d, m = inp["im1"] - inp["im2"], inp["mask"]
            if variant == "dense":
                assert d.all() and (m is None or m.all()) and {1, 2, 3} >= set(np.unique(np.abs(d)))
            elif d.size >= 64:
                assert not d.all() and d.any() and (m is None or (not m.all() and m.any()))
        elif isinstance(c, SseCase):
            d = inp["a"] - inp["b"]
            assert d.all() if variant == "dense" else (c.n < 64 or (not d.all() and d.any()))
        elif isinstance(c, SmoothCase):
            diffs = smooth_differences(inp["pred"])
            if variant == "zeros":      # the plateau: a zero of every kind of difference
                assert all((d == 0).any() for d in diffs)
            if c.B > 1:
                assert all(not np.array_equal(inp["pred"][0], inp["pred"][b]) for b in range(1, c.B))
            if c.H * c.W >= 64 and variant == "dense":
                assert all(len(np.unique(d)) >= 5 for d in diffs)
        else:
            ms = foreign_mask_sum(inp)
            assert ms != np.float32(inp["mask"].sum())
            other = exact_expected(c, inp, mask_sum=ms, grad_out=1.7)
            assert other["loss"] != want["loss"] and not np.array_equal(other["g_depth"], want["g_depth"])


# ---- the float cases are sharp --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,variant", float_cases(), ids=lambda x: case_id(x) if isinstance(x, tuple) else x)
def test_float_cases_are_sharp(c, variant):
    inp = inputs(c, variant)
    refs = [float_reference(c, variant, inp)]
    if isinstance(c, FitCase):
        refs.append(float_reference(c, variant, inp, mask_sum=foreign_mask_sum(inp), grad_out=1.7))
    for ref in refs:
        assert abs(float(ref.loss32) - float(ref.loss)) <= ref.tol
        assert ref.D * EPS32 + 4 * ref.e32 < 1e-4            # the tolerance is a small part of the bound
        moves = ref.moves[np.isfinite(ref.moves)]            # (leaving out the only group of a one-element case: 0 / 0)
        if isinstance(c, SmoothCase):                        # the last elements of an image's last row carry no term
            assert (ref.moves == 0).sum() <= 1
            moves = moves[moves > 0]
        assert moves.size == 0 or float(moves.min()) > ref.tol, (float(moves.min()), ref.tol)
        assert moves.size > 0 or c.B * c.C * c.H * c.W == 1
    if isinstance(c, PhotoCase) and c.sigma:
        sg = inp["sigma"].astype(np.float64) + SIGMA_EPS
        assert (sg.min() > 1.0) if variant == "sigma_above_one" else (sg.min() >= 0.1 and sg.max() <= 0.6 + 1e-6)


# ---- the broadcasting rules of photometric_loss, before any launch ----------------------------------------------------------------------
def test_photometric_loss_refuses_shapes_it_cannot_broadcast_before_any_launch():
    import torch
    from deep3dmap_amd.core import photometric_loss
    a, b = torch.zeros(3, 2, 4, 5), torch.zeros(3, 2, 4, 5)
    with pytest.raises(NotImplementedError):
        photometric_loss(a, b, conf_sigma=torch.ones(3, 2, 4, 5))
    with pytest.raises(NotImplementedError):
        photometric_loss(a, b, mask=torch.ones(3, 2, 4, 5))
    for kw in (dict(mask=torch.ones(3, 1, 6, 5)), dict(mask=torch.ones(2, 1, 4, 5)), dict(conf_sigma=torch.ones(3, 1, 4, 4)),
               dict(mask=torch.ones(1, 3, 1, 4, 5))):
        with pytest.raises(ValueError):
            photometric_loss(a, b, **kw)
    with pytest.raises(ValueError):
        photometric_loss(a, torch.zeros(2, 2, 4, 5))
    with pytest.raises(ValueError):
        photometric_loss(a, torch.zeros(3, 3, 4, 5))
