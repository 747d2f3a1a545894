"""Learnable uv images (neural_renderer/uv_textures.py), host side: a torch restatement of k_load_textures's sampling map
(pinned bit for bit to the oracle on the golden vectors; tests/test_gpu_uv_textures.py uses it in float64 as the adjoint's
reference), the hot-spot fact the adjoint is built around, and argument errors (the transpose's cache:
tests/test_built_cache_host.py)."""
import os

import numpy as np
import pytest
import torch

from oracle import nr_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement -----------------------------------------------------------------------------------------------
def _tex_mod(x, y):
    f = torch.fmod(x, y)
    return torch.where(x > 0, f, y + f)


def _wrap(v, wrapping):
    if wrapping == 0:
        return _tex_mod(v, 1.0)
    if wrapping == 1:
        m1 = _tex_mod(v, 1.0)
        return torch.where(_tex_mod(v, 2.0) < 1, m1, 1 - m1)
    if wrapping == 2:
        return torch.clamp(torch.clamp(v, max=1.0), min=0.0)
    return v


def sampling_map(faces_uv, ts, height, width, wrapping, bilinear):
    """k_load_textures's coefficients in its f32 arithmetic: pixel [F*ts^3, taps] int64 (y*W+x) and weight [F*ts^3, taps]
    f32 of every texel f*ts^3 + r, taps in the kernel's accumulation order (4 bilinear, 1 nearest); None under
    CLAMP_TO_BORDER (zeros).  Zero weights are kept."""
    if wrapping == 3:
        return None
    uv = torch.as_tensor(np.asarray(faces_uv, np.float32)).reshape(-1, 6)
    F = uv.shape[0]
    r = torch.arange(ts ** 3)
    d = [((r // (ts * ts)).double() / (ts - 1.)).float(), (((r // ts) % ts).double() / (ts - 1.)).float(),
         ((r % ts).double() / (ts - 1.)).float()]
    s = (d[0] + d[1]) + d[2]
    d = [torch.where(s > 0, x / torch.where(s > 0, s, torch.ones_like(s)), x) for x in d]
    u = _wrap(uv, wrapping)
    pos_x = (((u[:, None, 0] * d[0]) + (u[:, None, 2] * d[1])) + (u[:, None, 4] * d[2])) * float(width - 1)
    pos_y = (((u[:, None, 1] * d[0]) + (u[:, None, 3] * d[1])) + (u[:, None, 5] * d[2])) * float(height - 1)
    pos_x, pos_y = pos_x.reshape(-1), pos_y.reshape(-1)
    if bilinear:
        xi, yi = pos_x.to(torch.int64), pos_y.to(torch.int64)
        wx1 = pos_x - xi.float()
        wx0 = 1 - wx1
        wy1 = pos_y - yi.float()
        wy0 = 1 - wy1
        y1 = torch.clamp((pos_y + 1).to(torch.int64), max=height - 1)
        x1 = torch.clamp(xi + 1, max=width - 1)
        pix = torch.stack([yi * width + xi, y1 * width + xi, yi * width + x1, y1 * width + x1], 1)
        w = torch.stack([wx0 * wy0, wx0 * wy1, wx1 * wy0, wx1 * wy1], 1)
    else:
        # roundf (half away from zero) of a position >= 0, exact in double
        xr = torch.floor(pos_x.double() + 0.5).to(torch.int64)
        yr = torch.floor(pos_y.double() + 0.5).to(torch.int64)
        pix = (yr * width + xr)[:, None]
        w = torch.ones(pix.shape, dtype=torch.float32)
    return pix, w


def restate_load_textures(image, faces_uv, textures, is_update, wrapping, bilinear):
    """load_textures in f32, k_load_textures's association: c = 0, c += image[tap] * w in tap order."""
    image = torch.as_tensor(np.asarray(image, np.float32))
    H, W = image.shape[:2]
    out = torch.as_tensor(np.array(textures, np.float32, copy=True))
    F, ts = out.shape[0], out.shape[1]
    flat = out.reshape(F * ts ** 3, 3)
    m = sampling_map(faces_uv, ts, H, W, wrapping, bilinear)
    if m is None:
        new = torch.zeros_like(flat)
    else:
        pix, w = m
        img = image.reshape(-1, 3)
        if bilinear:
            new = torch.zeros_like(flat)
            for j in range(4):
                new = new + img[pix[:, j]] * w[:, j:j + 1]
        else:
            new = img[pix[:, 0]].clone()
    upd = torch.as_tensor(np.asarray(is_update) != 0).repeat_interleave(ts ** 3)
    flat[upd] = new[upd]
    return out.numpy()


def restate_cubes64(image64, faces_uv, ts, wrapping, bilinear, mask=None, base64=None):
    """The same linear map applied in float64 (differentiable in image64 [H,W,3] and base64): the adjoint's reference."""
    H, W = image64.shape[:2]
    F = int(np.asarray(faces_uv).shape[0])
    m = sampling_map(faces_uv, ts, H, W, wrapping, bilinear)
    if m is None:
        new = torch.zeros(F * ts ** 3, 3, dtype=torch.float64)
    else:
        pix, w = m
        img = image64.reshape(-1, 3)
        new = (img[pix] * w.double()[..., None]).sum(1)
    new = new.reshape(F, ts, ts, ts, 3)
    if mask is None:
        return new
    base64 = torch.zeros_like(new) if base64 is None else base64
    keep = torch.as_tensor(np.asarray(mask) != 0).reshape(F, 1, 1, 1, 1)
    return torch.where(keep, new, base64)


# ---- the restatement against the oracle --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tex_golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "tex_golden.npz"))


def load_cases(g):
    return sorted({k.split("/")[1] for k in g.files if k.startswith("load/")})


def load_case(g, name):
    pre = f"load/{name}/"
    return {k[len(pre):]: g[k] for k in g.files if k.startswith(pre)}


def test_restatement_is_bit_exact_against_the_oracle_on_every_golden_case(tex_golden):
    names = load_cases(tex_golden)
    assert len(names) == 8
    for name in names:
        c = load_case(tex_golden, name)
        args = (c["image"], c["faces_uv"], c["textures_in"], c["is_update"], int(c["wrapping"]), bool(c["bilinear"]))
        want = O.load_textures_np(c["image"], c["faces_uv"], c["textures_in"].copy(), c["is_update"], int(c["wrapping"]),
                                  bool(c["bilinear"]))
        got = restate_load_textures(*args)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
        assert np.array_equal(got.view(np.uint32), c["textures_out"].view(np.uint32)), name


@pytest.mark.parametrize("wrapping", [0, 1, 2])
@pytest.mark.parametrize("bilinear", [True, False])
def test_restatement_matches_the_oracle_off_the_unit_square(wrapping, bilinear):
    rng = np.random.default_rng(3 + wrapping)
    F, ts, H, W = 40, 3, 9, 14
    image = rng.random((H, W, 3), dtype=np.float32)
    uv = (rng.standard_normal((F, 3, 2)) * 2).astype(np.float32)
    uv[:6] = np.round(uv[:6])                                  # integer and negative integer corners
    tin = rng.random((F, ts, ts, ts, 3), dtype=np.float32)
    upd = (rng.random(F) > 0.3).astype(np.int32)
    want = O.load_textures_np(image, uv, tin.copy(), upd, wrapping, bilinear)
    got = restate_load_textures(image, uv, tin, upd, wrapping, bilinear)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("ts", [2, 3, 4, 5])
@pytest.mark.parametrize("wrapping", [0, 1, 2])
def test_texel_zero_of_every_face_samples_pixel_zero_with_weight_one(ts, wrapping):
    """The adjoint's hot spot: pixel (0,0) receives one entry per face (and zero-weight taps on its neighbours)."""
    rng = np.random.default_rng(ts)
    F, H, W = 200, 11, 13
    uv = (rng.standard_normal((F, 3, 2)) * 3).astype(np.float32)
    pix, w = sampling_map(uv, ts, H, W, wrapping, True)
    t0 = torch.arange(F) * ts ** 3
    assert torch.equal(pix[t0, 0], torch.zeros(F, dtype=torch.int64))
    assert torch.equal(w[t0, 0], torch.ones(F))
    assert torch.equal(w[t0, 1:], torch.zeros(F, 3))
    pix_n, w_n = sampling_map(uv, ts, H, W, wrapping, False)
    assert torch.equal(pix_n[t0, 0], torch.zeros(F, dtype=torch.int64))
    nz = w.reshape(-1) != 0
    assert int(torch.bincount(pix.reshape(-1)[nz], minlength=H * W)[0]) >= F


def test_restatement_float64_is_linear_in_the_image():
    rng = np.random.default_rng(0)
    F, ts, H, W = 12, 3, 7, 6
    uv = rng.random((F, 3, 2), dtype=np.float32) * 1.5
    a, b = (torch.from_numpy(rng.random((H, W, 3))) for _ in range(2))
    lhs = restate_cubes64(2 * a - 3 * b, uv, ts, 0, True)
    rhs = 2 * restate_cubes64(a, uv, ts, 0, True) - 3 * restate_cubes64(b, uv, ts, 0, True)
    assert torch.allclose(lhs, rhs, rtol=0, atol=1e-12)


# ---- the product's host logic ------------------------------------------------------------------------------------------
def test_argument_errors_raise_before_any_launch():
    from deep3dmap_amd.neural_renderer import textures_from_image
    img = torch.rand(5, 6, 3)
    uv = torch.rand(4, 3, 2)
    with pytest.raises(TypeError):
        textures_from_image(img.double(), uv)
    with pytest.raises(TypeError):
        textures_from_image(img, uv.double())
    with pytest.raises(ValueError):
        textures_from_image(img[..., :2], uv)
    with pytest.raises(ValueError):
        textures_from_image(img[0], uv)
    with pytest.raises(ValueError):
        textures_from_image(img, uv[:, :2])
    with pytest.raises(ValueError):
        textures_from_image(img, uv, texture_size=1)
    with pytest.raises(ValueError):
        textures_from_image(img, uv, texture_wrapping='WRAP')
    with pytest.raises(ValueError):
        textures_from_image(img, uv, texture_wrapping=4)
    with pytest.raises(ValueError):
        textures_from_image(img, uv, texture_size=2, base=torch.zeros(4, 3, 3, 3, 3))
    with pytest.raises(ValueError):
        textures_from_image(img, uv, texture_size=2, base=torch.zeros(2, 4, 2, 2, 2, 3))   # a batch base needs a batch
    with pytest.raises(ValueError):
        textures_from_image(img, uv, faces_mask=torch.ones(5, dtype=torch.int32))
    with pytest.raises(TypeError):
        textures_from_image(img, uv, faces_mask=torch.ones(4))
    with pytest.raises(RuntimeError, match="CUDA"):
        textures_from_image(img, uv)                                       # host tensors never reach the library


def test_faces_uv_gradient_raises():
    from deep3dmap_amd.neural_renderer import textures_from_image
    with pytest.raises(NotImplementedError, match="faces_uv"):
        textures_from_image(torch.rand(5, 6, 3), torch.rand(4, 3, 2, requires_grad=True))


# (the transpose cache: tests/test_built_cache_host.py, once for every cache of the package)


# ---- the C entry point refuses bad arguments before any launch -----------------------------------------------------------
def test_adjoint_entry_point_returns_invalid_before_any_launch():
    import ctypes
    from deep3dmap_amd import _lib
    L = _lib.lib()
    p, q = ctypes.c_void_p(256), 256                        # never dereferenced: every call below returns before a launch
    INVALID = 1
    csr = dict(offsets=q, items=q, chunks=None, long_rows=None, long_chunk_ptr=None, num_rows=6, num_chunks=0, num_long_rows=0,
               long_row=64)
    ok = dict(csr=True, lanes=4, g=p, partials=None, out=p, batch=1, texels=32, H=2, W=3)
    chunked = dict(num_chunks=1, num_long_rows=1, chunks=q, long_rows=q, long_chunk_ptr=q, partials=p)
    bad = [dict(g=None), dict(out=None), dict(offsets=None), dict(batch=0), dict(batch=65536), dict(texels=0), dict(H=0),
           dict(W=-1), dict(H=1 << 16, W=1 << 15), dict(lanes=0), dict(lanes=3), dict(lanes=32), dict(long_row=-1),
           dict(num_chunks=-1), dict(num_long_rows=-1),
           dict(num_long_rows=1, long_rows=q, long_chunk_ptr=q),        # long rows without chunks
           dict(num_chunks=1, chunks=q, partials=p),                    # chunks without long rows
           dict(chunked, items=None), dict(chunked, partials=None),     # chunks without entries or partials
           dict(chunked, chunks=None), dict(chunked, long_rows=None), dict(chunked, long_chunk_ptr=None),
           dict(csr=None), dict(num_rows=7), dict(num_rows=5)]          # no d3m_csr; not the H * W rows the entry point walks
    for change in bad:
        assert set(change) <= set(ok) | set(csr), change
        a = dict(ok, **{k: v for k, v in change.items() if k in ok})
        if a["csr"]:
            a["csr"] = ctypes.byref(_lib.D3MCsr(**dict(csr, **{k: v for k, v in change.items() if k in csr})))
        assert L.d3m_uv_texture_adjoint(*a.values(), None) == INVALID, change
