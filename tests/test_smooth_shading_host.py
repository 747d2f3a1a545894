"""Smooth shading (neural_renderer/smooth_shading.py, mesh_cython.fit_illumination), host side: the manual adjoint of
tests/smooth_shading_scenes.py against float64 autograd, sh_basis through the reference's fit_illumination outputs, argument
errors, SHLight's initial light, the adjacency cache, and the C entry points' refusals."""
import ctypes
import os

import numpy as np
import pytest
import torch

import smooth_shading_scenes as S
from deep3dmap_amd.neural_renderer import smooth_shading as ss

# The largest deviation of illumination_fit on CPU tensors from tests/golden/sh_golden.npz measured here is 8.9e-16 (values
# in [0, 1]; the scenes of S.FIT_SCENES with the default and with lamb=2, max_iter=1): only the order of the 9x9
# normal-equation sums differs.  The GPU test allows 16 times this bound.
FIT_TOL = 1e-15
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sh_golden.npz")


def _nr():
    from deep3dmap_amd import neural_renderer as nr
    return nr


# ---- 1. the restatement's manual adjoint is autograd's ----------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
def test_manual_adjoint_equals_float64_autograd(B):
    v, f, notes = S.fan_mesh()
    faces = torch.from_numpy(f)
    x, colors, sh, g, g_normals = S.case_inputs(v, B, 5)
    leaves = [t.clone().requires_grad_(True) for t in (x, colors, sh)]
    shaded, n, r = S.restate_forward(leaves[0], faces, leaves[1], leaves[2])
    ((shaded * g).sum() + (n * g_normals).sum()).backward()
    manual = S.restate_adjoint(x, faces, colors, sh, g, g_normals)
    for leaf, m, name in zip(leaves, manual, ("g_x", "g_colors", "g_sh")):
        scale = float(m.abs().max())
        assert scale > 0 and float((leaf.grad - m).abs().max()) <= 1e-12 * scale, name
    # the scene is what it says: hubs of 64, 65 and 2049 items, a vertex of no face with n = 0, well-conditioned normals
    from deep3dmap_amd.neural_renderer.row_gather import CHUNK, LONG_ROW
    counts = np.bincount(f.reshape(-1), minlength=v.shape[0])
    assert sorted(notes["hubs"].values()) == [LONG_ROW, LONG_ROW + 1, 2 * CHUNK + 1] and v.shape[0] > 256
    assert all(counts[h] == c and all(int(np.sum(f[:, s] == h)) >= c // 3 for s in range(3)) for h, c in notes["hubs"].items())
    assert counts[notes["unused"]] == 0 and notes["unused"] == v.shape[0] - 1
    assert bool((n[:, notes["unused"]] == 0).all()) and float(r.detach()[:, :-1].min()) > 0.05
    a, b = notes["doubled"]
    assert f[notes["doubled_face"]].tolist() == [a, a, b]


def test_sh_basis_is_the_restatement_and_differentiable():
    nr = _nr()
    n = torch.nn.functional.normalize(torch.randn(50, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(1)), dim=-1)
    assert torch.equal(nr.sh_basis(n), S.basis(n)) and nr.sh_basis(n.float()[None]).shape == (1, 50, 9)
    assert nr.sh_basis(n.float()).dtype == torch.float32
    leaf = n.clone().requires_grad_(True)
    w = torch.randn(50, 9, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    (nr.sh_basis(leaf) * w).sum().backward()
    assert float((leaf.grad - torch.einsum("vj,vjc->vc", w, S.basis_gradient(n))).abs().max()) <= 1e-14
    # the terms are orthonormal over the sphere up to the quadrature: H_0^2 integrates to 1
    assert abs(4 * np.pi * S.A0 ** 2 - 1) < 1e-15
    for bad in (torch.zeros(4, 2), torch.zeros(4, 3, dtype=torch.int32), np.zeros((4, 3))):
        with pytest.raises(ValueError):
            nr.sh_basis(bad)


# ---- 2. fit_illumination's device-agnostic part reproduces the reference ----------------------------------------------------
@pytest.mark.parametrize("name", sorted(S.FIT_SCENES))
def test_illumination_fit_on_cpu_tensors_reproduces_the_golden(name):
    """mesh_cython.render.illumination_fit (everything of fit_illumination after the normals, nr.sh_basis included) on CPU
    tensors against the reference's outputs.  Measured largest deviation over the scenes: 8.9e-16 (g20_64x56, lamb=2,
    max_iter=1); the bound FIT_TOL = 1e-15 is that figure rounded up, and the GPU test allows 16 FIT_TOL."""
    from deep3dmap_amd.mesh_cython import render as R
    golden = np.load(GOLDEN)
    s = S.fit_scene(name)
    before = s["vertices"].copy()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))     # noqa: E731
    norm = S.norm_direction64(s["vertices"], s["triangles"])
    for key, kw in ((name, {}), (name + "/iter1_lamb2", dict(lamb=2, max_iter=1))):
        got = R.illumination_fit(t(s["image"]), t(s["vertices"]), t(s["texture"]), t(norm), t(s["vis_ind"]), **kw)
        assert got.dtype == torch.float64 and tuple(got.shape) == golden[key].shape == s["texture"].shape
        dev = float(np.abs(got.numpy() - golden[key]).max())
        print(f"{key}: largest deviation {dev:.2e}")
        assert dev <= FIT_TOL, (key, dev)
        assert 0.02 < golden[key].min() and golden[key].max() <= 1.0
    assert np.array_equal(before, s["vertices"])                # the caller's vertices are not clamped in place
    if name == "g12_outside":
        h, w, _ = s["image"].shape
        assert (before[0] < 0).any() and (before[0] > w - 1).any() and (before[1] < 0).any() and (before[1] > h - 1).any()
        assert golden[name].max() == 1.0                        # the clamp to [0, 1] runs too
    with pytest.raises(ValueError):
        R.illumination_fit(t(s["image"]), t(s["vertices"]), t(s["texture"]), t(norm), t(s["vis_ind"]), max_iter=0)


# ---- 3. argument errors (none needs a device) -------------------------------------------------------------------------------
def test_argument_errors():
    nr = _nr()
    x, faces, colors, sh = torch.rand(6, 3), torch.tensor([[0, 1, 2], [3, 4, 5]]), torch.rand(6, 3), torch.rand(3, 9)
    bad = [dict(vertices=torch.rand(6, 4)), dict(vertices=torch.rand(6)), dict(vertices=torch.rand(2, 2, 6, 3)),
           dict(vertices=torch.rand(0, 3)), dict(vertices=x.double()), dict(vertices=x.half()), dict(vertices=x.numpy()),
           dict(colors=torch.rand(6, 4)), dict(colors=torch.rand(5, 3)), dict(colors=colors.double()), dict(colors=None),
           dict(colors=torch.rand(2, 6, 3), vertices=torch.rand(3, 6, 3)), dict(colors=colors.numpy()),
           dict(sh=torch.rand(9, 3)), dict(sh=torch.rand(3, 8)), dict(sh=torch.rand(27)), dict(sh=sh.double()), dict(sh=None),
           dict(sh=torch.rand(2, 3, 9), colors=torch.rand(3, 6, 3)), dict(sh=torch.rand(0, 3, 9)),
           dict(faces=faces.float()), dict(faces=faces.to(torch.int16)), dict(faces=faces.reshape(-1)),
           dict(faces=faces[None].repeat(2, 1, 1)), dict(faces=faces[:, :2]), dict(faces=faces[:0]), dict(faces=faces.numpy())]
    for change in bad:
        a = dict(dict(vertices=x, faces=faces, colors=colors, sh=sh), **change)
        with pytest.raises(ValueError):
            nr.sh_vertex_colors(a["vertices"], a["faces"], a["colors"], a["sh"])
    with pytest.raises(ValueError, match="device"):            # all on the host: nothing to run on
        nr.sh_vertex_colors(x, faces, colors, sh)
    with pytest.raises(ValueError, match="device"):
        nr.vertex_normals(x, faces)
    for v, f in ((x.double(), faces), (torch.rand(6, 2), faces), (x, faces.float())):
        with pytest.raises(ValueError):
            nr.vertex_normals(v, f)
    for per_set in (0, 65536, -1):
        with pytest.raises(ValueError):
            nr.SHLight(per_set)


# ---- 4. SHLight -----------------------------------------------------------------------------------------------------------
def test_shlight_starts_as_white_ambient():
    nr = _nr()
    for per_set, shape in ((None, (3, 9)), (4, (4, 3, 9))):
        m = nr.SHLight(per_set)
        assert isinstance(m.sh, torch.nn.Parameter) and tuple(m.sh.shape) == shape and m.sh.dtype == torch.float32
        assert [n for n, _ in m.named_parameters()] == ["sh"]
        sh = m.sh.detach()
        assert bool((sh[..., 1:] == 0).all()) and bool((sh[..., 0] == np.float32(1.0 / S.A0)).all())
        # L = sh . H(n) = 1 for any normal: shaded = colors
        n = torch.nn.functional.normalize(torch.randn(7, 3, generator=torch.Generator().manual_seed(3)), dim=-1)
        L = torch.einsum("...kj,vj->...vk", sh, nr.sh_basis(n))
        assert float((L - 1).abs().max()) <= 2.0 ** -23


# ---- 5. the adjacency is built once per faces tensor -------------------------------------------------------------------------
def test_the_adjacency_is_reused(monkeypatch):
    from deep3dmap_amd.neural_renderer import row_gather
    faces = torch.tensor([[0, 1, 2], [2, 1, 3]])
    x = torch.rand(4, 3)
    built = []
    real = row_gather.build_adjacency
    monkeypatch.setattr(row_gather, "build_adjacency", lambda *a: built.append(1) or real(*a))
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))      # (past the device check, on the host)
    cache = row_gather.AdjacencyCache(2)
    first, batched = ss._checked(x, faces, x, torch.rand(3, 9), cache)
    again, _ = ss._checked(x[None], faces, x, torch.rand(2, 3, 9), cache)
    assert first is again and built == [1] and not batched
    assert first.csr.offsets.tolist() == [0, 1, 3, 5, 6] and (first.num_vertices, first.num_faces) == (4, 2)
    other, _ = ss._checked(x, faces.clone(), None, None, cache)
    assert other is not first and built == [1, 1]
    with pytest.raises(ValueError, match="indices"):
        ss._checked(torch.rand(3, 3), faces, None, None, cache)
    light = _nr().SHLight()
    assert isinstance(light._adjacency, row_gather.AdjacencyCache) and light._adjacency is not row_gather._cache


# ---- 6. the C entry points refuse bad arguments before any launch -----------------------------------------------------------
def test_entry_points_return_invalid_before_any_launch():
    from deep3dmap_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(256)                                # never dereferenced: every call below returns before a launch
    INVALID = 1
    assert L.d3m_error_string(INVALID) == b"invalid argument"
    assert L.d3m_smooth_shade_scratch_floats(3, 3, 300, 500, 2) == 3 * (900 + 4500 + 6) + 3 * 2 * 27
    assert L.d3m_smooth_shade_scratch_floats(3, 1, 300, 500, 0) == 900 + 4500 + 3 * 2 * 27
    assert L.d3m_smooth_shade_scratch_floats(1, 1, 256 * 64 + 1, 1, 0) == 3 * (256 * 64 + 1) + 9 + 64 * 27
    for args in ((0, 1, 4, 2, 0), (65536, 1, 4, 2, 0), (3, 2, 4, 2, 0), (1, 1, 0, 2, 0), (1, 1, 4, 0, 0), (1, 1, 4, 2, -1),
                 (1, 1, 4, 2 ** 30, 0), (4, 4, 2 ** 28, 2, 0)):
        assert L.d3m_smooth_shade_scratch_floats(*args) == 0, args
    big = 1 << 20
    q = 256                                                 # the same address as a field of the d3m_csr
    csr = dict(offsets=q, items=q, chunks=None, long_rows=None, long_chunk_ptr=None, num_rows=4, num_chunks=0, num_long_rows=0,
               long_row=64)

    def refused(entry, ok, change):
        assert set(change) <= set(ok) | set(csr), change
        a = dict(ok, **{k: v for k, v in change.items() if k in ok})
        if a["csr"]:
            a["csr"] = ctypes.byref(_lib.D3MCsr(**dict(csr, **{k: v for k, v in change.items() if k in csr})))
        return entry(*a.values(), None) == INVALID
    fwd_ok = dict(x=p, vb=1, col=p, cb=1, sh=p, sb=1, tri=p, csr=True, scratch=p, floats=big, shaded=p, normals=p, lengths=p,
                  B=1, V=4, F=2)
    common = [dict(x=None), dict(tri=None), dict(offsets=None), dict(items=None), dict(scratch=None), dict(B=0), dict(B=65536),
              dict(V=0), dict(F=0), dict(F=-3), dict(F=2 ** 30), dict(vb=2), dict(cb=2), dict(sb=2), dict(vb=0),
              dict(B=3, vb=3, cb=2), dict(long_row=-1), dict(num_chunks=-1), dict(num_long_rows=-1),
              dict(num_long_rows=1, long_rows=q, long_chunk_ptr=q),    # long rows without chunks
              dict(num_chunks=1, chunks=q),                            # chunks without their rows
              dict(floats=5), dict(x=ctypes.c_void_p(258)), dict(col=p, sh=None),
              dict(csr=None), dict(num_rows=5), dict(num_rows=3)]      # no d3m_csr; not the V rows the entry point walks
    fwd_bad = common + [dict(normals=None), dict(lengths=None), dict(shaded=None), dict(col=None, sh=None),
                        dict(col=None, sh=None, shaded=None, B=2, vb=1)]
    for change in fwd_bad:
        assert refused(L.d3m_smooth_shade_forward, fwd_ok, change), change
    bwd_ok = dict(x=p, vb=1, col=p, cb=1, sh=p, sb=1, normals=p, lengths=p, g=p, gn=None, tri=p, csr=True, scratch=p, floats=big,
                  gx=p, gc=p, gsh=p, B=1, V=4, F=2)
    bwd_bad = common + [dict(normals=None), dict(lengths=None), dict(gx=None, gc=None, gsh=None), dict(g=None, gn=p),
                        dict(g=None, gn=p, gx=p, gc=None, gsh=p), dict(col=None, sh=None, gc=None, gsh=None)]
    for change in bwd_bad:
        assert refused(L.d3m_smooth_shade_backward, bwd_ok, change), change
