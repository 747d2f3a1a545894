"""Learnable per-vertex colours (neural_renderer/vertex_colors.py), host side: an element-wise torch restatement of the map
colours -> cubes (pinned to this repo's vcolor_to_texture_cube and, bit for bit, to the grid mesh of get_textures_from_im;
tests/test_gpu_vertex_colors.py uses it in float32 as the forward's reference and in float64 for the adjoint's), the CSR
builder, argument errors, and VertexColors.from_textures (the adjacency's cache: tests/test_built_cache_host.py)."""

import numpy as np
import pytest
import torch

from deep3dmap_amd.core.renderer_utils import _CUBE, vcolor_to_texture_cube


# ---- the restatement and the adjoint's reference (shared with the GPU tests) --------------------------------------------
def restate_cubes(colors, faces):
    """[B,V,3] colours, [F,3] indices -> [B,F,2,2,2,3] in the colours' dtype, element-wise operators only: texel idx, channel
    k = (C[idx][0] c0 + C[idx][1] c1) + C[idx][2] c2 (one rounding per operator: what the kernel computes)."""
    C = torch.tensor(_CUBE, dtype=colors.dtype)
    c = colors[:, faces.long()]                                     # [B,F,3 corners,3 channels]
    c0, c1, c2 = (c[:, :, j, None, :] for j in range(3))            # [B,F,1,3]
    w0, w1, w2 = (C[None, None, :, j, None] for j in range(3))      # [1,1,8,1]
    out = (w0 * c0 + w1 * c1) + w2 * c2
    return out.reshape(colors.shape[0], faces.shape[0], 2, 2, 2, 3)


def adjoint64(grad_textures, faces, num_vertices):
    """(reference, sum of |terms|, valence) of the adjoint in float64 on the host: reference[b,v,k] = sum over the vertex's
    (face, corner) items and idx of C[idx][corner] g[b,f,idx,k] (index_add_), the same sum of absolute values, and the
    number of items per vertex."""
    g = grad_textures.detach().double().cpu().reshape(grad_textures.shape[0], -1, 8, 3)
    faces = faces.detach().cpu().long().reshape(-1, 3)
    C = torch.tensor(_CUBE, dtype=torch.float64)
    ref = torch.zeros(g.shape[0], num_vertices, 3, dtype=torch.float64)
    mag = torch.zeros_like(ref)
    for c in range(3):
        ref.index_add_(1, faces[:, c], (C[None, None, :, c, None] * g).sum(2))
        mag.index_add_(1, faces[:, c], (C[None, None, :, c, None] * g).abs().sum(2))
    return ref, mag, torch.bincount(faces.reshape(-1), minlength=num_vertices)


def adjoint_bound(mag, valence):
    """gamma_n * sum|terms| with n = 8 * valence: the products are exact (coefficients 0, +-1/2, 1), so a float32 sum of n
    terms in ANY order is within gamma_n = n u / (1 - n u), u = 2^-24, of the exact sum, relative to the sum of |terms|."""
    nu = 8.0 * valence.double() * 2.0 ** -24
    return (nu / (1.0 - nu))[None, :, None] * mag


def image_grid_faces(h, w):
    """[2(h-1)(w-1), 3] faces of an h x w image's grid mesh in get_textures_from_im's corner order: (tl, tr, bl) of every
    cell, then (bl, tr, br) of every cell."""
    idx = torch.arange(h * w).reshape(h, w)
    tl, tr, bl, br = idx[:-1, :-1], idx[:-1, 1:], idx[1:, :-1], idx[1:, 1:]
    return torch.cat([torch.stack([tl, tr, bl], -1).reshape(-1, 3), torch.stack([bl, tr, br], -1).reshape(-1, 3)], 0)


def restate_textures_from_im(im):
    """get_textures_from_im(im, 2) of im [b,c,h,w] on the host: the three corner images of the two faces of every cell,
    sliced (no index tensor), through the kernel's expression."""
    b, c, h, w = im.shape
    C = torch.tensor(_CUBE, dtype=im.dtype)
    tl, tr, bl, br = im[:, :, :-1, :-1], im[:, :, :-1, 1:], im[:, :, 1:, :-1], im[:, :, 1:, 1:]
    halves = []
    for c0, c1, c2 in ((tl, tr, bl), (bl, tr, br)):
        c0, c1, c2 = (x.reshape(b, c, -1).transpose(1, 2)[:, :, None, :] for x in (c0, c1, c2))      # [b,cells,1,c]
        halves.append((C[None, None, :, 0, None] * c0 + C[None, None, :, 1, None] * c1) + C[None, None, :, 2, None] * c2)
    return torch.cat(halves, 1).reshape(b, -1, 2, 2, 2, c)


def irregular_mesh(seed=0):
    """(faces [F,3] int64, V = 257, notes): about 2,500 faces over one vertex more than a 256-lane workgroup, with vertex
    256 in no face, one face [a, a, b], and three hubs whose item counts are LONG_ROW exactly, LONG_ROW + 1 and 2 CHUNK + 1
    (two full chunks and one item)."""
    from deep3dmap_amd.neural_renderer.vertex_colors import CHUNK, LONG_ROW
    rng = np.random.default_rng(seed)
    V, hubs = 257, {0: 2 * CHUNK + 1, 1: LONG_ROW, 2: LONG_ROW + 1}
    plain = np.arange(5, 256)                                        # (3, 4: the repeated-corner face; 256: unused)
    faces = []
    for hub, count in hubs.items():
        for i in range(count):
            face = list(rng.choice(plain, 3, replace=False))
            face[i % 3] = hub                                        # the hub sits at every corner slot
            faces.append(face)
    faces.append([3, 3, 4])
    for _ in range(2500 - len(faces)):
        faces.append(list(rng.choice(plain, 3, replace=False)))
    faces = np.array(faces, np.int64)[rng.permutation(len(faces))]
    return torch.from_numpy(faces), V, dict(hubs=hubs, unused=256, doubled=3)


# ---- 1. the cube map ----------------------------------------------------------------------------------------------------
def test_restatement_equals_vcolor_to_texture_cube():
    gen = torch.Generator().manual_seed(0)
    colors = torch.randn(2, 40, 3, generator=gen)
    faces = torch.randint(0, 40, (90, 3), generator=gen)
    got = restate_cubes(colors, faces)
    # vcolor_to_texture_cube takes [b, channels, faces, 3 corners]
    want = vcolor_to_texture_cube(colors[:, faces].permute(0, 3, 1, 2).contiguous())
    assert got.shape == want.shape == (2, 90, 2, 2, 2, 3)
    assert float((got - want).abs().max()) <= 2.0 ** -23 * float(want.abs().max())


def test_restatement_equals_textures_from_im_on_the_grid_mesh():
    h, w = 5, 7
    im = torch.rand(2, 3, h, w, generator=torch.Generator().manual_seed(1))
    faces = image_grid_faces(h, w)
    assert faces.shape == (2 * (h - 1) * (w - 1), 3)
    colors = im.permute(0, 2, 3, 1).reshape(2, h * w, 3)
    got = restate_cubes(colors, faces)
    want = restate_textures_from_im(im)
    assert torch.equal(got.view(torch.int32), want.contiguous().view(torch.int32))
    # the corner texels are the corner colours themselves
    assert torch.equal(got[:, :, 1, 0, 0], colors[:, faces[:, 0]]) and torch.equal(got[:, :, 0, 0, 1], colors[:, faces[:, 2]])


# ---- 2. the CSR builder -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_adjacency_rows(dtype):
    from deep3dmap_amd.neural_renderer.vertex_colors import CHUNK, LONG_ROW, build_adjacency
    faces, V, notes = irregular_mesh()
    A = build_adjacency(faces.to(dtype), V)
    F = faces.shape[0]
    off, items = A.csr.offsets.long(), A.csr.items.long()
    assert A.csr.offsets.dtype == A.csr.items.dtype == A.tri.dtype == torch.int32
    assert off.shape == (V + 1,) and items.shape == (3 * F,) and int(off[0]) == 0 and int(off[-1]) == 3 * F
    assert torch.equal(A.tri.long(), faces) and (A.num_vertices, A.num_faces) == (V, F)
    flat = faces.reshape(-1)
    for v in range(V):
        row = items[off[v]:off[v + 1]]
        assert bool((flat[row] == v).all()) and bool((row[1:] > row[:-1]).all()), v
    assert sorted(items.tolist()) == list(range(3 * F))
    assert int(off[notes["unused"] + 1] - off[notes["unused"]]) == 0
    # the face [a, a, b] gives a two items, 3 f and 3 f + 1
    f = int(torch.nonzero((faces[:, 0] == 3) & (faces[:, 1] == 3))[0])
    a_row = items[off[3]:off[4]].tolist()
    assert a_row == [3 * f, 3 * f + 1]
    # the long rows: only the two hubs above the limit, cut into chunks of CHUNK items in row order
    counts = (off[1:] - off[:-1])
    for hub, n in notes["hubs"].items():
        assert int(counts[hub]) == n
    assert A.csr.long_rows.tolist() == [0, 2] and A.csr.long_chunk_ptr.tolist() == [0, 3, 4]
    assert int(counts[1]) == LONG_ROW and 1 not in A.csr.long_rows.tolist()
    ch = A.csr.chunks.tolist()
    assert ch[:3] == [[0, CHUNK], [CHUNK, 2 * CHUNK], [2 * CHUNK, 2 * CHUNK + 1]]
    assert ch[3] == [int(off[2]), int(off[3])]


def test_adjacency_without_long_rows_and_index_errors():
    from deep3dmap_amd.neural_renderer.vertex_colors import build_adjacency
    A = build_adjacency(torch.tensor([[0, 1, 2], [2, 1, 3]]), 5)
    assert A.csr.offsets.tolist() == [0, 1, 3, 5, 6, 6] and A.csr.items.tolist() == [0, 1, 4, 2, 3, 5]
    assert A.csr.chunks.shape == (0, 2) and A.csr.long_rows.numel() == 0 and A.csr.long_chunk_ptr.tolist() == [0]
    with pytest.raises(ValueError, match="indices"):
        build_adjacency(torch.tensor([[0, 1, 5]]), 5)
    with pytest.raises(ValueError, match="indices"):
        build_adjacency(torch.tensor([[0, -1, 2]]), 5)


# ---- 3. argument errors (none needs a device) ---------------------------------------------------------------------------
def test_argument_errors():
    from deep3dmap_amd import neural_renderer as nr
    colors, faces = torch.rand(6, 3), torch.tensor([[0, 1, 2], [3, 4, 5]])
    bad = [(torch.rand(6, 4), faces), (torch.rand(6), faces), (torch.rand(2, 2, 6, 3), faces), (torch.rand(0, 3), faces),
           (colors.double(), faces), (colors.half(), faces), (colors, faces.float()), (colors, faces.to(torch.int16)),
           (colors, faces.reshape(-1)), (colors, faces[None].repeat(2, 1, 1)), (colors, faces[:, :2]),
           (colors, faces[:0]), (colors.numpy(), faces), (colors, faces.numpy())]
    for c, f in bad:
        with pytest.raises(ValueError):
            nr.textures_from_vertex_colors(c, f)
    with pytest.raises(ValueError, match="device"):        # both on the host: nothing to run on
        nr.textures_from_vertex_colors(colors, faces)
    with pytest.raises(ValueError):
        nr.VertexColors(torch.rand(6, 2), faces)
    with pytest.raises(ValueError):
        nr.VertexColors(colors, faces.float())
    with pytest.raises(ValueError):
        nr.VertexColors.from_textures(torch.rand(3, 2, 2, 2, 3), faces, 6)          # three cubes, two faces
    with pytest.raises(ValueError):
        nr.VertexColors.from_textures(torch.rand(2, 1, 1, 1, 3), faces, 6)          # ts < 2
    with pytest.raises(ValueError, match="indices"):
        nr.VertexColors.from_textures(torch.rand(2, 2, 2, 2, 3), faces, 5)


# (4. the cache: tests/test_built_cache_host.py, once for every cache of the package)


# ---- 5. VertexColors.from_textures ----------------------------------------------------------------------------------------
def test_from_textures_returns_the_colours_the_cubes_were_made_from():
    from deep3dmap_amd import neural_renderer as nr
    faces, V, notes = irregular_mesh(seed=3)
    gen = torch.Generator().manual_seed(5)
    colors = torch.randint(-8, 9, (V, 3), generator=gen).float() / 2           # a 1/2-grid: every sum below is exact
    cubes = restate_cubes(colors[None], faces)
    m = nr.VertexColors.from_textures(cubes, faces, V)
    want = colors.clone()
    want[notes["unused"]] = 0                                                  # no face: no colour to read
    assert m.colors.shape == (V, 3) and isinstance(m.colors, torch.nn.Parameter) and torch.equal(m.faces, faces)
    assert torch.equal(m.colors.detach(), want)
    assert torch.equal(nr.VertexColors.from_textures(cubes[0], faces[None], V).colors.detach(), want)
    # any texture size: the corner texels are (ts-1,0,0), (0,ts-1,0), (0,0,ts-1)
    ts = 4
    big = torch.rand(faces.shape[0], ts, ts, ts, 3, generator=gen)
    big[:, ts - 1, 0, 0], big[:, 0, ts - 1, 0], big[:, 0, 0, ts - 1] = (colors[faces[:, j]] for j in range(3))
    assert torch.equal(nr.VertexColors.from_textures(big, faces, V).colors.detach(), want)


# ---- 6. the C entry points refuse bad arguments before any launch ---------------------------------------------------------
def test_entry_points_return_invalid_before_any_launch():
    import ctypes
    from deep3dmap_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(256)                                # never dereferenced: every call below returns before a launch
    INVALID = 1
    assert L.d3m_error_string(INVALID) == b"invalid argument"
    fwd = L.d3m_vertex_color_textures
    for args in ((None, 1, p, p, 4, 2), (p, 1, None, p, 4, 2), (p, 1, p, None, 4, 2), (p, 0, p, p, 4, 2),
                 (p, 65536, p, p, 4, 2), (p, 1, p, p, 0, 2), (p, 1, p, p, 4, 0), (p, 1, p, p, 4, -1)):
        assert fwd(*args, None) == INVALID, args
    bwd = L.d3m_vertex_color_textures_backward
    q = 256                                                 # the same address as a field of the d3m_csr
    csr = dict(offsets=q, items=q, chunks=None, long_rows=None, long_chunk_ptr=None, num_rows=4, num_chunks=0, num_long_rows=0,
               long_row=64)
    ok = dict(g=p, csr=True, partials=None, out=p, batch=1, V=4, F=2)
    bad = [dict(g=None), dict(offsets=None), dict(items=None), dict(out=None), dict(batch=0), dict(batch=65536), dict(V=0),
           dict(F=0), dict(F=-3), dict(long_row=-1), dict(num_chunks=-1), dict(num_long_rows=-1),
           dict(num_long_rows=1, long_rows=q, long_chunk_ptr=q),        # long rows without chunks
           dict(num_chunks=1, chunks=q),                                # chunks without partials
           dict(num_chunks=1, partials=p),                              # ... or without their ranges
           dict(num_long_rows=1, num_chunks=1, chunks=q, partials=p), dict(F=2 ** 30),
           dict(csr=None), dict(num_rows=5), dict(num_rows=3)]          # no d3m_csr; not the V rows the entry point walks
    for change in bad:
        assert set(change) <= set(ok) | set(csr), change
        a = dict(ok, **{k: v for k, v in change.items() if k in ok})
        if a["csr"]:
            a["csr"] = ctypes.byref(_lib.D3MCsr(**dict(csr, **{k: v for k, v in change.items() if k in csr})))
        assert bwd(*a.values(), None) == INVALID, change
