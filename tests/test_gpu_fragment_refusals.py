"""What the fragment family's backward entry points refuse on the device (csrc/d3m_raster.hip: gather_ok and the scratch
checks behind it), called raw on one valid record: the six gathering backwards -- attribute images, the interior
geometry adjoint, SH fragments, SH x uv albedo, antialias, the uv bake's vertices -- with (a) no visibility blob, (b) a blob
one byte short, (c) an adjacency without items, (d) a scratch one element short, (e) (b) and (d) together, and the two
fixed-point image adjoints (plain uv, mip) with (d): they read neither the blob nor an adjacency, so (a), (b), (c) and (e)
do not apply to them.  The expected codes are read off the entry points' code, not measured: a malformed argument is
D3M_ERR_INVALID and wins over a scratch that is too small, which is D3M_ERR_WORKSPACE -- except for the mip adjoint, which
answers D3M_ERR_INVALID for its scratch too.  Nothing is launched by a refusal, and the device works afterwards."""
import ctypes

import pytest
import torch

from conftest import kernels_launched

pytestmark = pytest.mark.gpu
INVALID, WORKSPACE = 1, 2                 # D3M_ERR_INVALID, D3M_ERR_WORKSPACE of include/d3m_raster.h
B, V, S, C, H, W = 1, 6, 4, 3, 4, 4       # one view of two triangles at 4 x 4, no anti-aliasing; a 4 x 4 texture, 3 channels
ROWS = (("a", INVALID), ("b", INVALID), ("c", INVALID), ("d", WORKSPACE), ("e", INVALID))


def _record():
    from deep3dmap_amd import neural_renderer as nr
    sv = torch.tensor([[[-0.8, -0.8, 1.0], [0.6, -0.7, 1.0], [-0.5, 0.7, 1.0],
                        [0.7, 0.8, 2.0], [-0.3, 0.6, 2.0], [0.6, -0.4, 2.0]]], device="cuda")
    faces = torch.tensor([[0, 1, 2], [3, 4, 5]], dtype=torch.int32, device="cuda")
    fr = nr.rasterize_fragments(sv, faces, S, anti_aliasing=False, fill_back=True)
    torch.cuda.synchronize()
    assert int((fr.face_index_map >= 0).sum()) > 0
    return sv, fr


def _attribute_gradient(fr, attributes):
    from deep3dmap_amd import neural_renderer as nr
    a = attributes.clone().requires_grad_(True)
    images, _alpha = nr.interpolate_vertex_attributes(a, fr)
    (images * images).sum().backward()
    torch.cuda.synchronize()
    return images.detach(), a.grad


def test_backward_entry_points_refuse_with_their_codes_and_launch_nothing():
    from deep3dmap_amd import _lib
    from deep3dmap_amd.neural_renderer.row_gather import vertex_adjacency
    from deep3dmap_amd.neural_renderer.uv_textures import _wrapping_code
    L = _lib.lib()
    sv, fr = _record()
    Fp = fr.faces.shape[1]
    csr = vertex_adjacency(fr.tri, V).csr.c
    assert Fp == 4 and csr.num_chunks == 0 and fr.visibility.numel() == L.d3m_visibility_bytes(B, Fp)
    attributes = torch.rand(V, C, device="cuda")
    images_before, grad_before = _attribute_gradient(fr, attributes)

    # operands that are large enough for every entry point; a refusal reads none of them
    buf = {k: torch.zeros(B * 16 * S * S, device="cuda") for k in ("g", "out", "normals", "sh", "image", "uv")}
    p = {k: _lib.ptr(t) for k, t in buf.items()}
    p["sv"] = _lib.ptr(sv)
    scratch = torch.zeros(1 << 16, dtype=torch.int64, device="cuda")
    wrap, tol = _wrapping_code("REPEAT"), 0.01
    csr_ref = ctypes.byref(csr)
    floats = dict(attribute=L.d3m_vertex_attribute_scratch_floats(B, Fp, C, csr_ref),
                  geometry=L.d3m_fragment_geometry_scratch_floats(B, Fp, S, csr_ref, 0),
                  sh=L.d3m_sh_fragment_scratch_floats(B, Fp, S, 0, csr_ref),
                  antialias=L.d3m_antialias_scratch_floats(B, Fp, S, csr_ref, 0),
                  bake=L.d3m_uv_bake_scratch_floats(B, Fp, csr_ref))
    nbytes = dict(sh_uv=L.d3m_sh_uv_fragment_scratch_bytes(B, Fp, S, 1, H, W, csr_ref),
                  uv=L.d3m_uv_texture_images_scratch_bytes(1, H, W, C, B, S),
                  mip=L.d3m_uv_texture_mip_images_scratch_bytes(1, H, W, C, 1, B, S))
    sizes = dict(floats, **nbytes)
    assert all(0 < n <= scratch.numel() for n in floats.values()) and all(0 < n <= scratch.numel() * 8 for n in nbytes.values())
    sp = _lib.ptr(scratch)

    # fn(f, a, n): the call with the record f, the adjacency a and the scratch size n (floats, or bytes where the ABI says so)
    gathering = {
        "attribute": lambda f, a, n: L.d3m_vertex_attribute_images_backward(f, p["g"], a, sp, n, p["out"], 1, V, C, None),
        "geometry": lambda f, a, n: L.d3m_fragment_geometry_backward(f, p["g"], a, sp, n, p["out"], V, None),
        "sh": lambda f, a, n: L.d3m_sh_fragment_images_backward(f, p["normals"], 1, p["sh"], 1, None, 1, V, p["g"], a, sp, n,
                                                                p["out"], 1, None, None, None),
        "sh_uv": lambda f, a, n: L.d3m_sh_uv_fragment_images_backward(f, p["normals"], 1, p["sh"], 1, V, p["uv"], p["image"], 1,
                                                                      H, W, wrap, p["g"], a, sp, n, p["out"], None, None,
                                                                      None, None),
        "antialias": lambda f, a, n: L.d3m_antialias_geometry_backward(f, p["g"], a, sp, n, p["out"], V, None),
        # (the record is its own uv layout: one view, no anti-aliasing, the same triangles)
        "bake": lambda f, a, n: L.d3m_uv_bake_vertices_backward(f, f, p["image"], C, H, W, p["sv"], V, 1, tol, p["g"], a, sp, n,
                                                                p["out"], None),
    }
    image_adjoints = {
        "uv": (lambda f, n: L.d3m_uv_texture_images_backward(f, p["uv"], p["g"], 1, H, W, C, wrap, sp, n, p["out"], None),
               WORKSPACE),
        "mip": (lambda f, n: L.d3m_uv_texture_mip_images_backward(f, p["uv"], p["g"], 1, H, W, C, wrap, 1, 0.0, sp, n,
                                                                  p["out"], None), INVALID),
    }

    def record(**changes):
        c = fr.c_struct()
        for k, v in changes.items():
            setattr(c, k, v)
        return ctypes.byref(c)

    no_items = _lib.D3MCsr(**dict({k: getattr(csr, k) for k, _ in _lib.D3MCsr._fields_}, items=None))
    short_blob = dict(visibility_size=fr.visibility.numel() - 1)
    with kernels_launched() as k:
        for name, fn in gathering.items():
            n = sizes[name]
            got = (("a", fn(record(visibility=None), csr_ref, n)), ("b", fn(record(**short_blob), csr_ref, n)),
                   ("c", fn(record(), ctypes.byref(no_items), n)), ("d", fn(record(), csr_ref, n - 1)),
                   ("e", fn(record(**short_blob), csr_ref, n - 1)))
            assert got == ROWS, (name, got)
        for name, (fn, code) in image_adjoints.items():
            assert fn(record(), sizes[name] - 1) == code, name
        torch.cuda.synchronize()
    assert not k.names, sorted(k.names)

    # the refusals left the device alone: the same node, forward and backward, gives the bits it gave before
    images_after, grad_after = _attribute_gradient(fr, attributes)
    assert bool(torch.isfinite(grad_after).all()) and float(grad_after.abs().max()) > 0
    assert torch.equal(images_before, images_after) and torch.equal(grad_before, grad_after)
