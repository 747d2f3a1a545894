"""Mesh shape regularisers (neural_renderer/mesh_regularizers.py), host side: a plain-torch restatement of the three terms
over edges and wing records this file builds with Python loops (tests/test_gpu_mesh_regularizers.py runs it in float64 as
the reference and in float32 as the yardstick of the tolerance), known answers, the topology builder against the loop-built
one, argument errors, and the entry points' D3M_ERR_INVALID (the topology's cache: tests/test_built_cache_host.py)."""
import ctypes
import math

import numpy as np
import pytest
import torch


# ---- the loop-built topology and the restatement (shared with the GPU tests) ----------------------------------------------
def loop_topology(faces):
    """(edges [E,2], wings [P,4]) int64 of faces [F,3], by the definition: the distinct unordered sides {a,b}, a != b, sorted
    by (min, max); per edge, every pair i < j of its incident faces that repeat no index, in ascending face order, gives
    (a, b, third vertex of face i, third vertex of face j)."""
    incident = {}
    for f, (i, j, k) in enumerate(faces.reshape(-1, 3).tolist()):
        proper = len({i, j, k}) == 3
        for s, t, o in ((i, j, k), (j, k, i), (k, i, j)):
            if s == t:
                continue
            at = incident.setdefault((min(s, t), max(s, t)), [])
            if proper:
                at.append((f, o))
    edges = sorted(incident)
    wings = []
    for a, b in edges:
        inc = sorted(incident[(a, b)])
        for i in range(len(inc)):
            for j in range(i + 1, len(inc)):
                wings.append((a, b, inc[i][1], inc[j][1]))
    return (torch.tensor(edges, dtype=torch.int64).reshape(-1, 2), torch.tensor(wings, dtype=torch.int64).reshape(-1, 4))


def restate_terms(x, edges, wings, edge_target=0.0, which=(True, True, True)):
    """(L_lap, L_edge, L_nc), each [B] (None where `which` is off), of x [B,V,3] in x's dtype: index_add_, cross, norm."""
    B, V, _ = x.shape
    a, b = edges[:, 0], edges[:, 1]
    E, P = edges.shape[0], wings.shape[0]
    lap = edge = nc = None
    if which[0]:
        one = torch.ones(E, dtype=x.dtype)
        deg = torch.zeros(V, dtype=x.dtype).index_add_(0, a, one).index_add_(0, b, one)
        total = torch.zeros_like(x).index_add_(1, a, x[:, b]).index_add_(1, b, x[:, a])
        delta = torch.where((deg > 0)[None, :, None], x - total / deg.clamp(min=1)[None, :, None], torch.zeros_like(x))
        lap = (delta ** 2).sum((1, 2)) / V
    if which[1]:
        length = (x[:, a] - x[:, b]).norm(dim=-1)
        edge = ((length - edge_target) ** 2).sum(1) / E if E else x.sum((1, 2)) * 0
    if which[2]:
        xa = x[:, wings[:, 0]]
        e = x[:, wings[:, 1]] - xa
        n0 = torch.cross(e, x[:, wings[:, 2]] - xa, dim=-1)
        n1 = -torch.cross(e, x[:, wings[:, 3]] - xa, dim=-1)
        den = n0.norm(dim=-1) * n1.norm(dim=-1)
        ok = den > 0
        cos = (n0 * n1).sum(-1) / torch.where(ok, den, torch.ones_like(den))
        nc = torch.where(ok, 1 - cos, torch.zeros_like(cos)).sum(1) / P if P else x.sum((1, 2)) * 0
    return lap, edge, nc


def restate(x, edges, wings, laplacian=0.0, edge=0.0, edge_target=0.0, normal=0.0, dtype=torch.float64):
    """(value [B], gradient [B,V,3]) of the weighted sum in `dtype` on the host: the restatement and its autograd gradient.
    A term of weight 0 is not evaluated."""
    x = x.detach().cpu().to(dtype).requires_grad_(True)
    terms = restate_terms(x, edges, wings, edge_target, (laplacian > 0, edge > 0, normal > 0))
    value = sum(w * t for w, t in zip((laplacian, edge, normal), terms) if t is not None)
    value.sum().backward()
    return value.detach(), x.grad


def regularizer_mesh(seed=0):
    """(vertices [V,3] f64, faces [F,3] i64, notes): a UV sphere of 2 CHUNK + 1 meridians x 3 rings (both poles have valence
    2 CHUNK + 1: two full chunks and one item), an open fan of LONG_ROW rim vertices and one of LONG_ROW + 1, three triangles
    on one edge (mixed winding), one face [a, a, b] and one vertex in no face; faces shuffled, positions jittered in 3-D."""
    from deep3dmap_amd.neural_renderer.vertex_colors import CHUNK, LONG_ROW
    rng = np.random.default_rng(seed)
    M, R = 2 * CHUNK + 1, 3
    theta = np.pi * (np.arange(R) + 1) / (R + 1)
    phi = 2 * np.pi * np.arange(M) / M
    rings = np.stack([np.sin(theta)[:, None] * np.cos(phi), np.sin(theta)[:, None] * np.sin(phi),
                      np.cos(theta)[:, None] * np.ones(M)], -1).reshape(-1, 3)
    sphere = np.concatenate([[[0, 0, 1.0], [0, 0, -1.0]], rings])
    sphere *= 1 + 0.05 * rng.standard_normal((len(sphere), 1))
    verts, faces = [sphere], []

    def ring(r, m):
        return 2 + r * M + m % M
    for m in range(M):
        faces.append([0, ring(0, m), ring(0, m + 1)])
        for r in range(R - 1):
            faces.append([ring(r, m), ring(r + 1, m), ring(r + 1, m + 1)])
            faces.append([ring(r, m), ring(r + 1, m + 1), ring(r, m + 1)])
        faces.append([1, ring(R - 1, m + 1), ring(R - 1, m)])
    at = len(sphere)
    notes = dict(poles=(0, 1), sphere_vertices=at, sphere_faces=len(faces), sphere_edges=9 * M)
    for name, rim, centre in (("fan_at_limit", LONG_ROW, 3.0), ("fan_above_limit", LONG_ROW + 1, -3.0)):
        ang = 1.5 * np.pi * np.arange(rim) / rim
        radius = 1 + 0.05 * rng.standard_normal(rim)
        fan = np.stack([centre + radius * np.cos(ang), radius * np.sin(ang), 0.2 * rng.standard_normal(rim)], -1)
        verts.append(np.concatenate([[[centre, 0, 0.3]], fan]))
        faces += [[at, at + 1 + k, at + 2 + k] for k in range(rim - 1)]
        notes[name] = at
        at += rim + 1
    verts.append(rng.standard_normal((5, 3)) + [0, 3.0, 0])
    p, q = at, at + 1
    faces += [[p, q, at + 2], [q, p, at + 3], [p, q, at + 4]]
    notes["shared_edge"] = (p, q)
    at += 5
    verts.append(rng.standard_normal((2, 3)) + [0, -3.0, 0])
    faces.append([at, at, at + 1])
    notes["doubled"] = (at, at + 1)
    at += 2
    verts.append(np.array([[0.5, 0.5, 4.0]]))
    notes["isolated"] = at
    at += 1
    faces = np.array(faces, np.int64)[rng.permutation(len(faces))]
    vertices = np.concatenate(verts)
    assert len(vertices) == at and at % 256 != 0
    return torch.from_numpy(vertices), torch.from_numpy(faces), notes


def _rel(a, b):
    return float((a - b).abs().max()) / float(b.abs().max())


# ---- 1. known answers -----------------------------------------------------------------------------------------------------
def test_regular_tetrahedron():
    x = torch.tensor([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=torch.float64) / math.sqrt(8)   # unit edges
    faces = torch.tensor([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])
    edges, wings = loop_topology(faces)
    assert edges.shape == (6, 2) and wings.shape == (6, 4)
    lap, edge, nc = restate_terms(x[None], edges, wings, edge_target=1.0)
    assert abs(float(lap) - 2 / 3) < 1e-14 and abs(float(edge)) < 1e-28 and abs(float(nc) - 4 / 3) < 1e-14
    # winding does not matter
    flipped = faces.clone()
    flipped[1] = flipped[1, [0, 2, 1]]
    assert abs(float(restate_terms(x[None], *loop_topology(flipped))[2]) - 4 / 3) < 1e-14


def _grid(n):
    idx = torch.arange(n * n).reshape(n, n)
    tl, tr, bl, br = idx[:-1, :-1], idx[:-1, 1:], idx[1:, :-1], idx[1:, 1:]
    faces = torch.cat([torch.stack([tl, tr, bl], -1).reshape(-1, 3), torch.stack([bl, tr, br], -1).reshape(-1, 3)], 0)
    ys, xs = torch.meshgrid(torch.arange(n, dtype=torch.float64), torch.arange(n, dtype=torch.float64), indexing="ij")
    return torch.stack([xs, ys, torch.zeros_like(xs)], -1).reshape(-1, 3), faces


def test_flat_grid():
    x, faces = _grid(5)
    edges, wings = loop_topology(faces)
    assert edges.shape == (56, 2) and wings.shape == (40, 4)
    assert float(restate_terms(x[None], edges, wings)[2]) == 0.0
    value, grad = restate(x[None], edges, wings, normal=1.0)
    assert float(value) == 0.0 and float(grad.abs().max()) < 1e-15


def test_restatement_gradient_equals_central_differences():
    x, faces = _grid(4)
    x = x + 0.2 * torch.randn(x.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    edges, wings = loop_topology(faces)
    for weights in (dict(laplacian=1.0), dict(edge=1.0, edge_target=0.7), dict(normal=1.0),
                    dict(laplacian=0.3, edge=0.5, edge_target=0.7, normal=0.2)):
        _, grad = restate(x[None], edges, wings, **weights)
        h, fd = 1e-6, torch.zeros_like(x)
        for v in range(x.shape[0]):
            for k in range(3):
                step = torch.zeros_like(x)
                step[v, k] = h
                fd[v, k] = (restate(x[None] + step, edges, wings, **weights)[0] -
                            restate(x[None] - step, edges, wings, **weights)[0]) / (2 * h)
        assert _rel(grad[0], fd) < 1e-7, weights


def test_degenerate_records_and_edges_contribute_nothing():
    # vertices 0 and 1 coincide: the edge (0,1) has length 0, and both faces on it have a zero normal
    x = torch.tensor([[0, 0, 0], [0, 0, 0], [1, 0, 0], [0, 1, 0.5]], dtype=torch.float64)
    faces = torch.tensor([[0, 1, 2], [1, 0, 3]])
    edges, wings = loop_topology(faces)
    value, grad = restate(x[None], edges, wings, edge=1.0, normal=1.0)
    assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(value).all())
    assert float(restate(x[None], edges, wings, normal=1.0)[1].abs().max()) == 0.0


# ---- 2. the topology builder ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mesh():
    vertices, faces, notes = regularizer_mesh()
    edges, wings = loop_topology(faces)
    return dict(vertices=vertices, faces=faces, notes=notes, edges=edges, wings=wings)


def test_the_test_mesh(mesh):
    from deep3dmap_amd.neural_renderer.vertex_colors import CHUNK
    n = mesh["notes"]
    assert n["sphere_vertices"] == 6149 and n["sphere_faces"] == 12294 and n["sphere_edges"] == 18441 == 9 * (2 * CHUNK + 1)
    sphere_edges = int((mesh["edges"][:, 1] < n["sphere_vertices"]).sum())
    sphere_wings = int((mesh["wings"][:, 1] < n["sphere_vertices"]).sum())
    assert sphere_edges == sphere_wings == 18441
    assert mesh["vertices"].shape[0] % 256 != 0
    # no normal of a wing record vanishes
    xa = mesh["vertices"][mesh["wings"][:, 0]]
    e = mesh["vertices"][mesh["wings"][:, 1]] - xa
    for role in (2, 3):
        assert float(torch.cross(e, mesh["vertices"][mesh["wings"][:, role]] - xa, dim=-1).norm(dim=-1).min()) > 0


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_topology_equals_the_loop_built_one(mesh, dtype):
    from deep3dmap_amd.neural_renderer.mesh_regularizers import build_topology
    from deep3dmap_amd.neural_renderer.vertex_colors import CHUNK, LONG_ROW
    faces, notes, edges, wings = mesh["faces"], mesh["notes"], mesh["edges"], mesh["wings"]
    V = mesh["vertices"].shape[0]
    T = build_topology(faces.to(dtype), V)
    E, P = edges.shape[0], wings.shape[0]
    assert (T.num_vertices, T.num_edges, T.num_wings) == (V, E, P) == (V, 18705, 18569)
    for t in (T.edges, T.wings, *T.nbr[:5], *T.wing[:5]):
        assert t.dtype == torch.int32
    assert torch.equal(T.edges.long(), edges) and torch.equal(T.wings.long(), wings)
    # the neighbour CSR: both directions of every edge, rows ascending
    both = torch.cat([edges, edges.flip(1)])
    both = both[torch.argsort(both[:, 0] * V + both[:, 1])]
    counts = torch.bincount(both[:, 0], minlength=V)
    off = T.nbr.offsets.long()
    assert off.shape == (V + 1,) and int(off[0]) == 0 and torch.equal(off[1:] - off[:-1], counts)
    assert torch.equal(T.nbr.items.long(), both[:, 1])
    same_row = both[1:, 0] == both[:-1, 0]
    assert bool((both[1:, 1] > both[:-1, 1])[same_row].all())
    # the wing CSR: items 4 p + role of the row's vertex, ascending per row, every item once
    woff, items = T.wing.offsets.long(), T.wing.items.long()
    wcounts = woff[1:] - woff[:-1]
    row_of = torch.repeat_interleave(torch.arange(V), wcounts)
    assert items.shape == (4 * P,) and torch.equal(wings.reshape(-1)[items], row_of)
    assert bool((items[1:] > items[:-1])[row_of[1:] == row_of[:-1]].all())
    assert torch.equal(torch.sort(items)[0], torch.arange(4 * P))
    # hubs: the poles' rows are two full chunks and one item; the fan apexes sit at the limit and one above it
    north, south = notes["poles"]
    at_limit, above = notes["fan_at_limit"], notes["fan_above_limit"]
    assert int(counts[north]) == int(counts[south]) == 2 * CHUNK + 1
    assert int(counts[at_limit]) == LONG_ROW and int(counts[above]) == LONG_ROW + 1
    assert T.nbr.long_rows.tolist() == [north, south, above] and T.nbr.long_chunk_ptr.tolist() == [0, 3, 6, 7]
    ch = T.nbr.chunks.tolist()
    assert ch[:3] == [[0, CHUNK], [CHUNK, 2 * CHUNK], [2 * CHUNK, 2 * CHUNK + 1]]
    assert ch[3][0] == int(off[south]) and ch[5] == [int(off[south]) + 2 * CHUNK, int(off[south + 1])]
    assert ch[6] == [int(off[above]), int(off[above + 1])]
    # (a pole's wing row: an endpoint of 2 CHUNK + 1 spokes, the third vertex across 2 CHUNK + 1 ring edges)
    assert int(wcounts[north]) == int(wcounts[south]) == 2 * (2 * CHUNK + 1)
    assert int(wcounts[at_limit]) == LONG_ROW - 2 and int(wcounts[above]) == LONG_ROW - 1
    assert T.wing.long_rows.tolist() == [north, south] and T.wing.long_chunk_ptr.tolist() == [0, 5, 10]
    wch = T.wing.chunks.tolist()
    assert wch[0] == [0, CHUNK] and wch[4] == [4 * CHUNK, 4 * CHUNK + 2] and wch[9][1] == int(woff[south + 1])
    # the isolated vertex: empty rows
    iso = notes["isolated"]
    assert int(counts[iso]) == 0 and int(wcounts[iso]) == 0
    # boundary edges (the fans' rims) give no record; the three-face edge gives three; [a, a, b] one edge and no record
    ab = T.wings[:, :2].long()
    rim = torch.tensor([at_limit + 1, at_limit + 2])
    assert bool((edges == rim).all(1).any()) and not bool((ab == rim).all(1).any())
    shared = torch.tensor(notes["shared_edge"])
    assert int((ab == shared).all(1).sum()) == 3
    doubled = torch.tensor(notes["doubled"])
    assert int((edges == doubled).all(1).sum()) == 1 and not bool((ab == doubled).all(1).any())
    assert int(counts[doubled[0]]) == 1 and T.nbr.items[off[doubled[0]]] == doubled[1]


def test_topology_errors_and_small_cases():
    from deep3dmap_amd.neural_renderer.mesh_regularizers import MAX_FACES_PER_EDGE, build_topology
    T = build_topology(torch.tensor([[0, 1, 2], [2, 1, 3]]), 5)
    assert T.edges.tolist() == [[0, 1], [0, 2], [1, 2], [1, 3], [2, 3]] and T.wings.tolist() == [[1, 2, 0, 3]]
    assert T.nbr.offsets.tolist() == [0, 2, 5, 8, 10, 10] and T.nbr.items.tolist() == [1, 2, 0, 2, 3, 0, 1, 3, 1, 2]
    assert T.wing.offsets.tolist() == [0, 1, 2, 3, 4, 4] and T.wing.items.tolist() == [2, 0, 1, 3]
    assert T.nbr.chunks.shape == (0, 2) and T.wing.long_rows.numel() == 0 and T.wing.long_chunk_ptr.tolist() == [0]
    only_doubled = build_topology(torch.tensor([[1, 1, 1], [0, 0, 2]]), 3)
    assert only_doubled.edges.tolist() == [[0, 2]] and only_doubled.num_wings == 0 and only_doubled.wings.shape == (0, 4)
    with pytest.raises(ValueError, match="indices"):
        build_topology(torch.tensor([[0, 1, 5]]), 5)
    with pytest.raises(ValueError, match="indices"):
        build_topology(torch.tensor([[0, -1, 2]]), 5)
    assert MAX_FACES_PER_EDGE == 16
    book = torch.tensor([[0, 1, 2 + k] for k in range(17)])
    assert build_topology(book[:16], 19).num_wings == 16 * 15 // 2
    with pytest.raises(ValueError, match="17 faces"):
        build_topology(book, 19)


# (3. the cache: tests/test_built_cache_host.py, once for every cache of the package)


# ---- 4. argument errors (none needs a device) -----------------------------------------------------------------------------
def test_argument_errors():
    from deep3dmap_amd import neural_renderer as nr
    x, faces = torch.rand(6, 3), torch.tensor([[0, 1, 2], [3, 4, 5]])
    bad = [(torch.rand(6, 4), faces), (torch.rand(6), faces), (torch.rand(2, 2, 6, 3), faces), (torch.rand(0, 3), faces),
           (x.double(), faces), (x.half(), faces), (x, faces.float()), (x, faces.to(torch.int16)), (x, faces.reshape(-1)),
           (x, faces[None].repeat(2, 1, 1)), (x, faces[:, :2]), (x, faces[:0]), (x.numpy(), faces), (x, faces.numpy())]
    for v, f in bad:
        with pytest.raises(ValueError):
            nr.mesh_regularizer(v, f, laplacian=1.0)
    for call in (nr.mesh_regularizer, nr.laplacian_loss, nr.edge_length_loss, nr.normal_consistency_loss):
        with pytest.raises(ValueError, match="device"):        # both on the host: nothing to run on
            call(x, faces)
    for weights in (dict(laplacian=-1.0), dict(edge=-0.5), dict(edge=1.0, edge_target=-1.0), dict(normal=-2.0),
                    dict(normal=float("nan"))):
        with pytest.raises(ValueError, match=">= 0"):
            nr.mesh_regularizer(x, faces, **weights)
        with pytest.raises(ValueError, match=">= 0"):
            nr.MeshRegularizer(faces, **weights)
    with pytest.raises(ValueError):
        nr.MeshRegularizer(faces.float())
    m = nr.MeshRegularizer(faces[None], laplacian=0.5, edge_target=0.1)
    assert m.faces.shape == (2, 3) and m.weights == dict(laplacian=0.5, edge=0.0, edge_target=0.1, normal=0.0)
    assert len(m._topology) == 0


# ---- 5. the C entry points refuse bad arguments before any launch ---------------------------------------------------------
def test_entry_points_return_invalid_before_any_launch():
    from deep3dmap_amd import _lib
    L = _lib.lib()
    p = 256                                                 # never dereferenced: every call below returns before a launch
    INVALID = 1
    assert L.d3m_error_string(INVALID) == b"invalid argument"
    csr = dict(offsets=p, items=p, chunks=None, long_rows=None, long_chunk_ptr=None, num_rows=8, num_chunks=0, num_long_rows=0,
               long_row=64)

    def topo(nbr={}, wing={}, both={}, **change):
        return _lib.D3MMeshTopology(**dict(dict(nbr=_lib.D3MCsr(**dict(csr, **both, **nbr)),
                                                wing=_lib.D3MCsr(**dict(csr, **both, **wing)), wings=p, num_edges=12, num_wings=10),
                                           **change))
    need = L.d3m_mesh_regularizer_scratch_floats
    assert need(1, ctypes.byref(topo())) == 8 * 4 + 1 and need(3, ctypes.byref(topo())) == 3 * (8 * 4 + 1)
    assert need(2, ctypes.byref(topo(nbr=dict(num_chunks=2, num_long_rows=1), wing=dict(num_chunks=1, num_long_rows=1)))) == \
        2 * (8 * 4 + 3 * 4 + 2 * 3 + 1)
    for b, t in ((0, topo()), (65536, topo()), (1, topo(both=dict(num_rows=0))), (1, topo(num_edges=-1)),
                 (1, topo(both=dict(long_row=-1)))):
        assert need(b, ctypes.byref(t)) == 0
    assert need(1, None) == 0
    ok = dict(x=p, batch=1, topo=topo(), lap=1.0, edge=1.0, target=0.5, normal=1.0, scratch=p, floats=1 << 20, scale=None,
              loss=p, grad=p, accumulate=0)
    chunked = dict(num_chunks=1, num_long_rows=1, chunks=p, long_rows=p, long_chunk_ptr=p)
    bad = [dict(x=None), dict(topo=None), dict(scratch=None), dict(loss=None), dict(batch=0), dict(batch=65536),
           dict(lap=-1.0), dict(edge=-1.0), dict(target=-0.1), dict(normal=-1.0), dict(lap=float("nan")),
           dict(floats=8 * 4), dict(scratch=260),                       # too small; not 16-byte aligned
           dict(topo=topo(both=dict(num_rows=0))), dict(topo=topo(both=dict(num_rows=-4))), dict(topo=topo(num_edges=-1)),
           dict(topo=topo(num_wings=-1)), dict(topo=topo(num_edges=1 << 30)), dict(topo=topo(num_wings=1 << 29)),
           dict(topo=topo(both=dict(long_row=-1))), dict(topo=topo(nbr=dict(offsets=None))), dict(topo=topo(nbr=dict(items=None))),
           dict(topo=topo(wings=None)), dict(topo=topo(wing=dict(offsets=None))), dict(topo=topo(wing=dict(items=None))),
           dict(topo=topo(nbr=dict(num_long_rows=1, long_rows=p, long_chunk_ptr=p))),         # long rows without chunks
           dict(topo=topo(wing=dict(num_long_rows=1, long_rows=p, long_chunk_ptr=p))),
           dict(topo=topo(nbr=dict(chunked, chunks=None))),                                    # chunks without their ranges
           dict(topo=topo(nbr=dict(chunked, long_rows=None))),
           dict(topo=topo(nbr=chunked), floats=8 * 4 + 1),                                     # chunks without partials
           dict(topo=topo(wing=dict(num_chunks=1, chunks=p))),                                 # chunks without long rows
           dict(topo=topo(wing=dict(num_rows=7))), dict(topo=topo(wing=dict(num_rows=9))),     # not the V rows of nbr
           dict(topo=topo(nbr=dict(long_row=-1))), dict(topo=topo(wing=dict(long_row=-1)))]
    for change in bad:
        a = dict(ok, **change)
        topo_arg = None if a["topo"] is None else ctypes.byref(a["topo"])
        args = [a["x"], a["batch"], topo_arg, a["lap"], a["edge"], a["target"], a["normal"], a["scratch"], a["floats"],
                a["scale"], a["loss"], a["grad"], a["accumulate"]]
        assert L.d3m_mesh_regularizer(*args, None) == INVALID, change
