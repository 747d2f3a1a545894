"""Shared by the tests of the texel, light and depth adjoints (test_texel_depth_host.py, test_gpu_texel_depth.py): K5 and K6 of
include/d3m_raster.h, section A (d3m_backward_textures, d3m_backward_depth_map, d3m_backward_depth_map_mesh) and the lit node's fused
form of them (d3m_backward_textures_lit).  The scenes, the seeded inputs and ONE statement of each operation, written from
csrc/d3m_backward.h, d3m_face_major.h and d3m_lit.h in the kernels' order and association, generic over the arithmetics of
section_b_scenes ("f64", "f32", "abs").

THE INPUTS OF ALL FOUR OPERATORS ARE MAPS.  face_index_map, weight_map, depth_map, face_inv_map and the sampling maps come from the
CPU oracle's forward (oracle.nr_oracle.raster_forward, port backend), so the owner of every pixel is known on the host and a float64
restatement over the same float32 maps takes no discrete decision -- but one: the integer part of a sample position at texture
sizes >= 3, which test_texel_depth_host.py keeps 2^-18 (ts - 1) away from every interior integer on every scene.

THE TOLERANCE is section_b_scenes.tolerance: (D 2^-24 + 4 E32) bound per element, D the longest chain of roundings behind the
element:

    D = n + TREE + CHAIN (+ B for a sum over the views) (+ SCALE_D with an unscaled gradient)

  n      the number of per-pixel terms behind the element.  A sum of n terms in ANY association -- a lane's sequential sum, the DPP
         tree of its 8 or 64 lanes, LDS atomics of a workgroup's waves, float atomics of the workgroups -- has a chain of at most
         n - 1 additions, so n covers every route's order;
  TREE   8: the 4 DPP steps and 2 additions of wave_sum, one addition into the workgroup's table, one into memory -- counted ON
         TOP of n, as the issue asks;
  CHAIN  the roundings of one term.  K5 (12): depth / z (1; as rcp and a product 3), x (ts - 1) (1), x weight (1), - floor (1),
         1 - fr (1), the corner's two products (2), x grad (1), x light (1), and 1 spare for the lit form's other association of the
         position.  The light's gradient adds x texel and its ts^3 terms.  K6 (22): to_pixel (3), a difference (1), a product (1), the
         denominator's two additions (2), the quotient (1; rcp and a product 3), / z (1; 3), KCU:582's three additions (3), depth^2
         in parallel, the four products and x S of KCU:588 (5);
  a v_rcp_f32 counts as two roundings.

An element whose bound is 0 has no term: it must be exactly zero.  Nothing is fitted to what the kernels return.

Every named wrong variant (`variant=`) is one defect class of the issue (VARIANTS); the host file shows that the comparison the GPU
test makes rejects each."""
import functools
from collections import namedtuple

import numpy as np

import test_gpu_owned_scan as T
from section_b_scenes import Abs, U, _rng, e32_of, f32v, fmax_, lift, sum_, tolerance, val      # noqa: F401

NEAR, FAR, EPS = 0.1, 100.0, 1e-3           # NR/renderer.py:63: the rasterizer's eps of the lit node
MAX_BOX, CHUNK = T.MAX_BOX, T.CHUNK
TREE, CHAIN_K5, CHAIN_K6, SCALE_D = 8, 12, 22, 3
STENCIL = 2.0 ** -18
GO, DEN = 0.75, 37.5                        # grad_out and mask_sum of the unscaled forms
Z_SEED = {"counts": 1, "holes": 1, "one_of_eight": 1, "limit": 2}      # (the first seeds that meet the stencil condition)
VARIANTS = ("chunk_last_dropped", "pixel_twice", "back_untransposed", "light_row_front", "light_view_ignored", "view32_missing",
            "view_twice", "large_not_zeroed", "back_vertices_unreversed", "flip_ignored", "scales_exchanged", "light_grad_lit",
            "corner_reversed", "bleed_dropped", "finv_transposed")


def fmin_(x, c):
    """min(x, c) for a constant c"""
    if isinstance(x, Abs):
        return Abs(np.minimum(x.v, c), np.where(x.v < c, x.a, abs(c)))
    return np.minimum(x, x.dtype.type(c))


def cat_(xs):
    if isinstance(xs[0], Abs):
        return Abs(np.concatenate([x.v for x in xs]), np.concatenate([x.a for x in xs]))
    return np.concatenate(xs)


def take_(x, idx):
    return Abs(x.v[idx], x.a[idx]) if isinstance(x, Abs) else x[idx]


def ints_(a, like):
    """an integer array in the arithmetic of `like`"""
    return Abs(a) if isinstance(like, Abs) else np.asarray(a).astype(like.dtype)


def scatter_(n, index, terms):
    """out[index[i]] += terms[i] in ascending i: exact in "f64", sequential float32 in "f32" (only E32 is taken from it)"""
    if isinstance(terms, Abs):
        v, a = np.zeros((n,) + terms.shape[1:]), np.zeros((n,) + terms.shape[1:])
        np.add.at(v, index, terms.v)
        np.add.at(a, index, terms.a)
        return Abs(v, a)
    out = np.zeros((n,) + terms.shape[1:], terms.dtype)
    np.add.at(out, index, terms)
    return out


def reshape_(x, shape):
    return Abs(x.v.reshape(shape), x.a.reshape(shape)) if isinstance(x, Abs) else x.reshape(shape)


# ==== scenes ========================================================================================================================
def _pad(S, tris, lanes):
    """off-screen triangles until the launch rule -- a wave per face above 48 raster pixels per triangle -- picks `lanes`"""
    tris = list(tris)
    while (S * S > 48 * len(tris)) != (lanes == 64):
        assert lanes == 8, "too many triangles for a wave per face"
        k = len(tris)
        tris.append([(S * T.OFF_SCREEN + k, 1.0, 1.0), (S * T.OFF_SCREEN + k + 3.0, 1.0, 1.0), (S * T.OFF_SCREEN + k, 4.0, 1.0)])
    return tris


def _views_triangles(B, lanes):
    """S = 24, six triangles a view, shifted from view to view; faces 1 and 4 wound the other way (their back copies own their pixels);
    faces 0-2 leave every third view, face 3 is on screen in views 5 and 32 alone (one view of the second mask word), face 4 in the
    last view alone -- without padding its back copy is among the last three faces of the array, where the ts = 1 reach meets the
    guard --, face 5 in none"""
    S, views = 24, []
    for b in range(B):
        tris = []
        for j in range(6):
            X, Y = 1.0 + 7 * (j % 3) + 0.37 * (b % 5), 1.0 + 10 * (j // 3) + 0.41 * (b % 3)
            on = [(b + j) % 3 != 0, (b + j) % 3 != 0, (b + j) % 3 != 0, b in (5, 32), b == B - 1, False][j]
            X += 0.0 if on else 3.0 * S
            z = 1.0 + 0.13 * j + 0.01 * (b % 7)
            t = [(X - 0.4, Y - 0.3, z), (X + 5.4, Y - 0.3, z + 0.3), (X - 0.4, Y + 5.3, z + 0.55)]
            tris.append(t[::-1] if j in (1, 4) else t)
        views.append(_pad(S, tris, lanes))
    return S, views, 6


def _slivers_triangles(lanes):
    """S = 128: eighty slivers 1.2 pixels wide on rows 0 and 1, each leaning 64 columns over 70 rows -- a box above FM_MAX_BBOX_AREA
    for a handful of pixels: every 64-pixel run of the first rows holds dozens of LARGE faces, a workgroup's run more than its table"""
    S, tris = 128, []
    for k in range(80):
        X = 1.5 * k
        lean = 64.0 if X < 64 else -64.0
        z = 1.0 + 0.01 * k
        tris.append([(X, -0.3, z), (X + 1.2, -0.3, z + 0.2), (X + 0.6 + lean, 70.3, z + 0.5)])
    return S, [_pad(S, tris, lanes)], 80


def _hub_triangles(lanes):
    """S = 32: a fan of twelve triangles about one hub vertex"""
    S, n = 32, 12
    ring = [(15.5 + 12.3 * np.cos(2 * np.pi * i / n + 0.1), 15.5 + 12.3 * np.sin(2 * np.pi * i / n + 0.1), 1.0 + 0.05 * i) for i in range(n)]
    hub = (15.4, 15.6, 1.5)
    return S, hub, ring


def _finish(S, v, tri, lanes, n_real, fill_back=True, **extra):
    """the oracle's forward of the mesh: everything the device will see"""
    from oracle import nr_oracle as O
    v = np.ascontiguousarray(v, np.float32)
    tri = np.ascontiguousarray(tri, np.int32)
    B, F = v.shape[0], tri.shape[0]
    faces = v[:, tri]
    faces2 = np.ascontiguousarray(np.concatenate([faces, faces[:, :, ::-1]], 1) if fill_back else faces)
    m = O.raster_forward(faces2, None, S, NEAR, FAR, EPS, None, False, True, True)
    fim = m["face_index_map"]
    Fp = faces2.shape[1]
    b, y, x = np.nonzero(fim >= 0)
    fn = fim[b, y, x].astype(np.int64)
    box = {}
    for key in np.unique(b * Fp + fn):
        bb = T._pixel_bbox(faces2[key // Fp, key % Fp], S)
        assert bb is not None
        box[int(key)] = bb
    sc = dict(S=S, B=B, F=F, Fp=Fp, V=v.shape[1], v=v, tri=tri, faces=faces2.astype(np.float64), fim=fim, wmap=m["weight_map"],
              dmap=m["depth_map"], finv=m["face_inv_map"], lanes=lanes, n_real=n_real, fill_back=fill_back, px=(b, y, x, fn), box=box)
    sc.update(extra)
    # every index a kernel can form: the owned pixels lie inside the face's (clamped) box, the box inside the image
    for key, (x0, x1, y0, y1) in box.items():
        sel = b * Fp + fn == key
        assert 0 <= x0 <= x[sel].min() and x[sel].max() <= x1 <= S - 1 and 0 <= y0 <= y[sel].min() and y[sel].max() <= y1 <= S - 1
    assert tri.min() >= 0 and tri.max() < v.shape[1]
    assert (sc["dmap"][fim >= 0] > NEAR).all() and (sc["dmap"][fim >= 0] < FAR).all()
    return sc


def _from_pixel_triangles(S, views, lanes, n_real, **extra):
    t = np.asarray(views, np.float64)                                          # [B, F, 3, 3]
    v = np.concatenate([T._ndc(t[..., :2], S), t[..., 2:]], -1).reshape(t.shape[0], -1, 3)
    tri = np.arange(v.shape[1], dtype=np.int32).reshape(-1, 3)
    return _finish(S, v, tri, lanes, n_real, **extra)


@functools.lru_cache(maxsize=None)
def scene(name, lanes, B=1):
    """dict(S, B, F, Fp, V, v [B,V,3], tri [F,3], faces [B,Fp,3,3], fim, wmap, dmap, finv, px = (b, y, x, fn) of the covered pixels
    in ascending order, box {b Fp + fn: (x0, x1, y0, y1)} of the faces that own a pixel)"""
    if name in T.SCENES:                            # the owned-scan scenes: chunk edges, holes, the box limit (their properties are
        assert B == 1                               # asserted there, on the same face_index_map)
        sc = T._scene(name, lanes)
        # their faces are flat in z, which puts sample positions on integers (w = 1/2 at ts = 3): every vertex moves up to 0.3
        # away from the eye -- less than the gap between overlapping faces, so that every pixel keeps its owner (asserted)
        v = sc["v"].numpy().copy()
        v[..., 2] += _rng(Z_SEED[name], len(name)).uniform(0, 0.3, v.shape[:2]).astype(np.float32)
        out = _finish(sc["S"], v, sc["tri"][0].numpy(), lanes, len(T._scene_triangles(name)[1]))
        assert np.array_equal(out["fim"][0], sc["fim"])
        return out
    if name in ("views", "views_front"):            # (views_front: without fill_back -- faces 1 and 4 are culled)
        S, views, n_real = _views_triangles(B, lanes)
        return _from_pixel_triangles(S, views, lanes, n_real, fill_back=name == "views")
    if name == "slivers":
        assert B == 1
        S, views, n_real = _slivers_triangles(lanes)
        return _from_pixel_triangles(S, views, lanes, n_real)
    if name == "hub":
        assert B == 1
        S, hub, ring = _hub_triangles(lanes)
        n = len(ring)
        pts = np.asarray([hub] + ring, np.float64)
        tri = [(0, 1 + i, 1 + (i + 1) % n) if i % 2 else (0, 1 + (i + 1) % n, 1 + i) for i in range(n)]    # (every other one by its back copy)
        pad = _pad(S, [None] * n, lanes)[n:]
        for t in pad:
            k = len(pts)
            pts = np.concatenate([pts, np.asarray(t, np.float64)], 0)
            tri.append((k, k + 1, k + 2))
        v = np.concatenate([T._ndc(pts[:, :2], S), pts[:, 2:]], -1)[None]
        return _finish(S, v, np.asarray(tri, np.int32), lanes, n)
    if name == "grid":                              # the implicit topology of a depth map's grid mesh: H x W vertices
        assert B == 1
        S, H, W = 32, 5, 6
        rng = _rng(5, H, W)
        gy, gx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        pts = np.stack([2.3 + 5.3 * gx + rng.uniform(-0.4, 0.4, gx.shape), 28.6 - 6.1 * gy + rng.uniform(-0.4, 0.4, gx.shape),
                        1.0 + rng.uniform(0, 0.8, gx.shape)], -1).reshape(-1, 3)
        first, second = [], []
        for yy in range(H - 1):                     # deep3dmap/core/renderer/utils.py:74-78 as tri_ids() restates it
            for xx in range(W - 1):
                tl = yy * W + xx
                first.append((tl, tl + W, tl + 1))
                second.append((tl + 1, tl + W, tl + W + 1))
        v = np.concatenate([T._ndc(pts[:, :2], S), pts[:, 2:]], -1)[None]
        assert (S * S > 48 * len(first + second)) == (lanes == 64)
        return _finish(S, v, np.asarray(first + second, np.int32), lanes, len(first + second), grid_w=W)
    raise KeyError(name)


def large_faces(sc):
    """keys b Fp + fn of the faces whose box exceeds FM_MAX_BBOX_AREA and that own a pixel"""
    return sorted(k for k, (x0, x1, y0, y1) in sc["box"].items() if (x1 - x0 + 1) * (y1 - y0 + 1) > MAX_BOX)


def px_runs(n):
    """csrc/d3m_raster.hip px_grid(n, sparse) and the kernels' split restated: (pixels per workgroup, workgroups) -- the same below
    either cap for every n of these tests"""
    blocks = (n + 255) // 256
    assert blocks <= 2048
    chunk = ((n + blocks - 1) // blocks + 255) // 256 * 256
    return chunk, blocks


@functools.lru_cache(maxsize=None)
def inputs(name, lanes, B, ts, tb, lb):
    """textures [tb,F,ts^3,3], light [lb,Fp,3], grad_rgb [B,S,S,3], grad_depth [B,S,S]: float32 values held in float64"""
    sc = scene(name, lanes, B)
    rng = _rng(23, len(name), lanes, B, ts, tb, lb)
    S, F, Fp = sc["S"], sc["F"], sc["Fp"]
    return dict(tex=f32v(rng.uniform(0.1, 1.0, (tb, F, ts ** 3, 3))), light=f32v(rng.uniform(0.2, 1.2, (lb, Fp, 3))),
                g_rgb=f32v(rng.uniform(-1, 1, (B, S, S, 3))), g_depth=f32v(rng.uniform(-1, 1, (B, S, S))), go=f32v(GO), den=f32v(DEN))


@functools.lru_cache(maxsize=None)
def sampling_maps(name, lanes, B, ts):
    """the oracle's forward_texture_sampling on the scene: dict(fim, sw [B,S,S,8], si [B,S,S,8], ts, F = the dense array's faces)"""
    from oracle import nr_oracle as O
    sc = scene(name, lanes, B)
    tex = np.ones((B, sc["Fp"], ts, ts, ts, 3), np.float32)
    m = O.raster_forward(sc["faces"].astype(np.float32), tex, sc["S"], NEAR, FAR, EPS, (0, 0, 0), True, True, False)
    assert np.array_equal(m["face_index_map"], sc["fim"])
    return dict(fim=sc["fim"], sw=m["sampling_weight_map"], si=m["sampling_index_map"], ts=ts, F=sc["Fp"])


def tri_views(sc):
    """an index tensor of its own for every view (tri_batch = B): view b's vertex i is stored at (i + 3 b) mod V.
    -> (vertices [B,V,3], tri [B,F,3]) giving the same faces"""
    B, V = sc["B"], sc["V"]
    v, tri = np.empty_like(sc["v"]), np.empty((B,) + sc["tri"].shape, np.int32)
    for b in range(B):
        v[b, (np.arange(V) + 3 * b) % V] = sc["v"][b]
        tri[b] = (sc["tri"] + 3 * b) % V
    assert np.array_equal(np.stack([v[b][tri[b]] for b in range(B)]), sc["v"][:, sc["tri"]])
    return v, tri


# ==== the cases ====================================================================================================================
# tb, lb: textures_batch, light_batch (1 = shared, 0 stands for B); vis: "list" (a d3m_visibility blob) | "flags" (none: the operator
# marks the faces itself); depth: where the depth rider goes ("none" | "faces" | "vertex"); form: the gradient maps (None = final,
# "maps" = unscaled maps, "records" = the edge gradient's float4 records); glight: grad_light given; off: bytes grad_textures is
# offset from 16-byte alignment; det: the deterministic mode
LitCase = namedtuple("LitCase", "scene lanes B ts tb lb vis depth form glight off det")
PlainCase = namedtuple("PlainCase", "scene lanes B ts ws")              # ws: the flags workspace and `faces` given
DepthCase = namedtuple("DepthCase", "scene lanes B ws finv det")        # finv: face_inv_map given
MeshCase = namedtuple("MeshCase", "scene lanes B tb implicit flip")     # tb: tri_batch (1 | 0 = B); implicit: tri = NULL
VIEW_COUNTS = (1, 31, 32, 33, 64, 65)


def _lit(scene_, lanes, ts, B=1, tb=1, lb=1, vis="list", depth="none", form=None, glight=1, off=0, det=0):
    return LitCase(scene_, lanes, B, ts, tb, lb, vis, depth, form, glight, off, det)


def lit_cases():
    out = []
    # textures: ts = 2 with flags and with a list, 8 and 64 lanes; ts = 3, 4 over a list (LDS form); without visibility, ts = 1, 5
    out += [_lit(s, lanes, 2) for s in ("counts", "holes", "one_of_eight") for lanes in (8, 64)]
    out += [_lit(s, 8, 2, vis="flags") for s in ("counts", "holes")]
    out += [_lit(s, lanes, ts) for ts in (3, 4) for s, lanes in (("counts", 8), ("counts", 64), ("holes", 8), ("holes", 64))]
    out += [_lit("one_of_eight", 8, ts, vis="flags") for ts in (3, 4)]
    out += [_lit("counts", 8, 1), _lit("counts", 8, 5), _lit("views", 64, 1, B=3, vis="flags"), _lit("views", 64, 5, B=3, vis="flags")]
    # textures_batch and light_batch 1 and B, grad_light NULL and not
    out += [_lit("views", 8, 2, B=2, tb=0, lb=0), _lit("views", 64, 4, B=3, tb=0, lb=0), _lit("views", 64, 3, B=2, tb=0, lb=1, vis="flags"),
            _lit("views", 8, 2, B=3, tb=1, lb=0), _lit("views", 64, 1, B=3, tb=0, lb=0, vis="flags"), _lit("views", 64, 2, B=3, tb=0, lb=1, vis="flags"),
            _lit("views", 8, 2, B=3, glight=0), _lit("views", 64, 4, B=2, tb=0, glight=0), _lit("views", 64, 5, B=2, glight=0)]
    # the depth rider: into grad_faces and into a vertex target, on every route
    out += [_lit("counts", lanes, 2, depth=d) for lanes in (8, 64) for d in ("faces", "vertex")]
    out += [_lit("holes", 8, 4, depth="faces"), _lit("holes", 64, 3, depth="vertex"), _lit("views", 64, 5, B=2, depth="faces", vis="flags"),
            _lit("views", 64, 5, B=2, depth="vertex"), _lit("hub", 8, 2, depth="vertex"), _lit("hub", 64, 2, depth="vertex")]
    # the input forms: unscaled maps, and the records (stride 4) with grad_out and mask_sum
    out += [_lit("counts", 8, 2, depth="vertex", form=f) for f in ("maps", "records")]
    out += [_lit("views", 64, 3, B=2, depth="vertex", form="records"), _lit("views", 64, 5, B=2, depth="vertex", form="maps", vis="flags")]
    # the view counts on shared textures: the mask's second word, the aligned and the generic sum over the views
    out += [_lit("views", 8 if off == 0 else 64, ts, B=B, lb=0, off=off) for B in VIEW_COUNTS for ts in (2, 4) for off in (0, 4)]
    # LARGE faces: the three branches of the per-pixel fallbacks
    out += [_lit("limit", lanes, 2, depth="faces") for lanes in (8, 64)]
    out += [_lit("limit", 64, 4, depth="vertex"), _lit("slivers", 8, 2, depth="vertex"), _lit("slivers", 64, 2, depth="faces")]
    # the deterministic mode: a box of any size stays in the gathered pass
    out += [_lit("limit", 64, 2, depth="faces", det=1), _lit("views", 8, 2, B=33, lb=0, depth="vertex", det=1)]
    assert len(set(out)) == len(out)
    return out


def plain_cases():
    return [PlainCase("counts", 8, 1, 2, 1), PlainCase("limit", 8, 1, 2, 1), PlainCase("views", 64, 2, 2, 1), PlainCase("counts", 8, 1, 2, 0),
            PlainCase("views", 64, 2, 1, 0), PlainCase("views", 64, 1, 1, 1), PlainCase("counts", 8, 1, 3, 1), PlainCase("holes", 8, 1, 5, 0)]


def depth_cases():
    return [DepthCase("counts", 8, 1, 1, 1, 0), DepthCase("counts", 8, 1, 0, 0, 0), DepthCase("holes", 8, 1, 1, 0, 0),
            DepthCase("limit", 8, 1, 1, 1, 0), DepthCase("limit", 8, 1, 1, 0, 1), DepthCase("views", 64, 2, 1, 0, 0),
            DepthCase("views", 64, 2, 0, 1, 0), DepthCase("slivers", 64, 1, 1, 0, 0), DepthCase("slivers", 64, 1, 0, 1, 0)]


def mesh_cases():
    return [MeshCase("counts", 8, 1, 1, 0, 0), MeshCase("counts", 64, 1, 1, 0, 1), MeshCase("holes", 8, 1, 1, 0, 1),
            MeshCase("views", 8, 3, 1, 0, 0), MeshCase("views", 64, 3, 0, 0, 0), MeshCase("views_front", 8, 3, 0, 0, 1),
            MeshCase("views_front", 64, 2, 1, 0, 0), MeshCase("grid", 8, 1, 1, 1, 0), MeshCase("grid", 8, 1, 1, 1, 1),
            MeshCase("hub", 8, 1, 1, 0, 0), MeshCase("hub", 64, 1, 1, 0, 1), MeshCase("limit", 64, 1, 1, 0, 0),
            MeshCase("slivers", 8, 1, 1, 0, 0), MeshCase("slivers", 64, 1, 1, 0, 1)]


def case_id(c):
    return type(c).__name__[:-4].lower() + "-" + "-".join(str(v) for v in c)


def batch_of(n, B):
    return n if n else B


# ==== the restatements ==============================================================================================================
def pixel_list(sc, variant=None):
    """(b, y, x, fn) of the owned pixels.  chunk_last_dropped: every face loses the last owned pixel of the first chunk of its box's
    scan (scan_owned_pixels: chunks of CHUNK[lanes] box pixels, row-major) in which it owns one; pixel_twice: its first counts twice"""
    b, y, x, fn = sc["px"]
    if variant not in ("chunk_last_dropped", "pixel_twice"):
        return b, y, x, fn
    keep = np.ones(b.size, np.int64)
    key = b * sc["Fp"] + fn
    for k, (x0, x1, y0, y1) in sc["box"].items():
        idx = np.nonzero(key == k)[0]
        off = (y[idx] - y0) * (x1 - x0 + 1) + (x[idx] - x0)
        order = idx[np.argsort(off)]
        chunk = np.sort(off) // CHUNK[sc["lanes"]]
        if variant == "pixel_twice":
            keep[order[0]] = 2
        else:
            keep[order[chunk == chunk[0]][-1]] = 0
    rep = np.repeat(np.arange(b.size), keep)
    return b[rep], y[rep], x[rep], fn[rep]


def scales(inp, form, ar, variant=None):
    """GradScale::get (csrc/d3m_device.h): (s_rgb, s_depth) of final maps (None), unscaled maps ("maps": go / (3 den), go / den) and the
    records form ("records": go, go / den)"""
    if form is None:
        return None, None
    go, den = lift(inp["go"], ar), lift(inp["den"], ar)
    s_rgb, s_depth = (go if form == "records" else go / (3.0 * den)), go / den
    return (s_depth, s_rgb) if variant == "scales_exchanged" else (s_rgb, s_depth)


def back_perm(ts):
    """texel (a, b, c) -> (c, b, a): NR/renderer.py:156; its own inverse"""
    t = np.arange(ts ** 3)
    return (t % ts) * ts * ts + ((t // ts) % ts) * ts + t // (ts * ts)


def sample_positions(sc, ts, ar, px=None):
    """sample_setup (csrc/d3m_lit.h:217, KCU:209-231): the clamped sample positions [P,3] of the owned pixels"""
    b, y, x, fn = sc["px"] if px is None else px
    w, d = lift(sc["wmap"][b, y, x], ar), lift(sc["dmap"][b, y, x], ar)
    z = lift(sc["faces"][b, fn, :, 2], ar)
    t = (w * float(ts - 1)) * (d[:, None] / z)
    return fmin_(fmax_(t, 0.0), float(np.float32(ts - 1) - np.float32(EPS)))


def corner_terms(t, g, ts, variant=None):
    """sample_corner (csrc/d3m_lit.h:228): the eight (weight x gradient [P,3], texel index [P]) of every pixel; weight = ((1 a0) a1) a2"""
    fl = np.trunc(val(t)).astype(np.int64)                  # f2i(): towards zero (ts = 1: the position is -eps, its integer part 0)
    fr = t - ints_(fl, t)
    out = []
    for pn in range(8):
        w, tii = None, []
        for k in range(3):
            bit = (pn >> k) & 1
            a = fr[:, k] if bit else 1.0 - fr[:, k]
            w = a if w is None else w * a
            tii.append(fl[:, k] + bit)
        if variant == "corner_reversed":
            tii = tii[::-1]
        out.append((w[:, None] * g, tii[0] * ts * ts + tii[1] * ts + tii[2]))
    return out


def lit_adjoint(sc, inp, ts, ar, variant=None, form=None):
    """d3m_backward_textures_lit's texels and light.  acc[b,f',texel,c] = sum over the owned pixels of corner weight x grad_rgb x s_rgb
    -- the gradient of the VIRTUAL lit array, with the ts = 1 reach into the following faces (lit_texel, KCU:229-233) and its guard at
    the array's end; gtex[b,f,texel] = acc x light of the front copy + the same of the back copy at texel (c,b,a), summed over the
    views in ascending order for shared textures; grad_light[row,c] = sum over the texels of acc x the PLAIN texel.
    -> dict(acc, gtex [tb,F,ts^3,3], glight [lb,Fp,3], n_tex, n_light: the per-pixel terms behind each element)"""
    B, F, Fp, ts3 = sc["B"], sc["F"], sc["Fp"], ts ** 3
    tb, lb = inp["tex"].shape[0], inp["light"].shape[0]
    px = pixel_list(sc, variant)
    b, y, x, fn = px
    g = lift(inp["g_rgb"][b, y, x], ar)
    s_rgb = scales(inp, form, ar, variant)[0]
    if s_rgb is not None:
        g = g * s_rgb
    corners = corner_terms(sample_positions(sc, ts, ar, px), g, ts, variant)
    terms, isc = cat_([c[0] for c in corners]), np.concatenate([c[1] for c in corners])
    vf = np.tile(b * Fp + fn, 8) + isc // ts3                # the face reached in the virtual [B,F'] array
    ok = vf < B * Fp
    if variant == "bleed_dropped":
        ok &= isc < ts3
    assert isc.min() >= 0 and (ts == 1 or isc.max() < ts3), "a corner outside the face's cube"
    e = (vf * ts3 + isc % ts3)[ok]
    acc = reshape_(scatter_(B * Fp * ts3, e, take_(terms, ok)), (B, Fp, ts3, 3))
    cnt = np.bincount(e, minlength=B * Fp * ts3).reshape(B, Fp, ts3)
    perm = np.arange(ts3) if variant == "back_untransposed" else back_perm(ts)
    light = lift(np.broadcast_to(inp["light"], (B, Fp, 3)) if lb == 1 else inp["light"], ar)
    if variant == "light_view_ignored":
        light = lift(np.broadcast_to(inp["light"][:1], (B, Fp, 3)), ar)
    if variant == "light_row_front" and sc["fill_back"]:
        light = _cat_axis1(light[:, :F], light[:, :F])
    tex = lift(np.broadcast_to(inp["tex"], (B, F, ts3, 3)) if tb == 1 else inp["tex"], ar)
    lit = acc * light[:, :, None, :]
    if sc["fill_back"]:
        gview = lit[:, :F] + take_(lit[:, F:], (slice(None), slice(None), perm))
        n_view = cnt[:, :F] + cnt[:, F:][:, :, perm]
        texp = take_(tex, (slice(None), slice(None), perm))
        tex2 = _cat_axis1(tex, texp)
    else:
        gview, n_view, tex2 = lit, cnt, tex
    if variant == "large_not_zeroed":                       # the per-pixel pass adds onto what the entry held: its own sums, twice
        for k in large_faces(sc):
            gview = _double(gview, k // Fp, (k % Fp) % F)
    prod = acc * tex2
    if variant == "light_grad_lit":
        prod = prod * light[:, :, None, :]
    rows = sum_(prod, 2)                                     # [B,Fp,3]
    n_rows = cnt.sum(2)
    if lb == 1:
        rows, n_rows = sum_(rows, 0)[None], n_rows.sum(0)[None]
    if tb == 1:
        views = list(range(B))
        if variant == "view32_missing":
            views = [v for v in views if v != 32]
        if variant == "view_twice":
            views.append(B - 1)
        gtex = sum_(take_(gview, (views,)), 0)[None]
        n_tex = n_view.sum(0)[None]
    else:
        gtex, n_tex = gview, n_view
    return dict(acc=acc, gtex=gtex, glight=rows, n_tex=n_tex[..., None], n_light=n_rows[..., None] + ts3)


def _cat_axis1(a, b):
    if isinstance(a, Abs):
        return Abs(np.concatenate([a.v, b.v], 1), np.concatenate([a.a, b.a], 1))
    return np.concatenate([a, b], 1)


def _double(x, b, f):
    if isinstance(x, Abs):
        v, a = x.v.copy(), x.a.copy()
        v[b, f] *= 2
        return Abs(v, a)
    x = x.copy()
    x[b, f] *= 2
    return x


def plain_texels(m, g_rgb, ar, variant=None):
    """d3m_backward_textures (KCU:506-540): grad_textures[b,f,...] += sampling weight x grad_rgb at the flat offset the sampling index
    names, past the own face at ts = 1, inside the array (the tex_total guard).  m: face_index_map, sampling_weight_map,
    sampling_index_map, ts, F.  -> (grad_textures [B,F,ts^3,3], terms per element)"""
    fim, ts3, F = m["fim"], m["ts"] ** 3, m["F"]
    B = fim.shape[0]
    b, y, x = np.nonzero(fim >= 0)
    fn = fim[b, y, x].astype(np.int64)
    if variant == "pixel_twice":
        b, y, x, fn = (np.concatenate([a, a[:1]]) for a in (b, y, x, fn))
    sw, si = lift(m["sw"][b, y, x], ar), m["si"][b, y, x].astype(np.int64)
    g = lift(g_rgb[b, y, x], ar)
    e = ((b * F + fn) * ts3)[:, None] + si
    ok = e < B * F * ts3
    if variant == "bleed_dropped":
        ok &= si < ts3
    assert e.min() >= 0
    terms = sw[:, :, None] * g[:, None, :]
    out = scatter_(B * F * ts3, e[ok], take_(terms, ok))
    return reshape_(out, (B, F, ts3, 3)), np.bincount(e[ok], minlength=B * F * ts3).reshape(B, F, ts3, 1)


def depth_adjoint(sc, g_depth, ar, variant=None, finv_map=False, flip=False, s_depth=None):
    """d3m_backward_depth_map (KCU:543-592): the nine values of every face, summed over the pixels it owns.
      tmp[k] = sum_l -finv[l][k] / z_l  (KCU:582; finv: the face inverse in pixel space, face_inverse(), or the forward's face_inv_map)
      v[k][0|1] = -g tmp[0|1] w_k depth^2 S / 2  (KCU:588)      v[k][2] = g w_k depth^2 / z_k^2  (KCU:575)
    flip: g is the gradient of the OUTPUT image, whose row S-1-y is the map's row y.  -> (grad_faces [B,Fp,3,3], terms per face)"""
    S, B, Fp = sc["S"], sc["B"], sc["Fp"]
    b, y, x, fn = pixel_list(sc, variant)
    face = lift(sc["faces"][b, fn], ar)                      # [P,3,3]
    z = face[:, :, 2]
    if finv_map:
        finv = lift(sc["finv"][b, y, x], ar)
        cols = [finv[:, :, 0], finv[:, :, 1], finv[:, :, 2]]
    else:
        px = [((face[:, n, 0] * float(S) + float(S)) - 1.0) * 0.5 for n in range(3)]
        py = [((face[:, n, 1] * float(S) + float(S)) - 1.0) * 0.5 for n in range(3)]
        den = (px[2] * (py[0] - py[1]) + px[0] * (py[1] - py[2])) + px[1] * (py[2] - py[0])
        c0 = [(py[(l + 1) % 3] - py[(l + 2) % 3]) / den for l in range(3)]
        c1 = [(px[(l + 2) % 3] - px[(l + 1) % 3]) / den for l in range(3)]
        c2 = [(px[(l + 1) % 3] * py[(l + 2) % 3] - px[(l + 2) % 3] * py[(l + 1) % 3]) / den for l in range(3)]
        cols = [_stack1(c0), _stack1(c1), _stack1(c2)]      # cols[k][:, l] = finv[l][k]
    tmp = []
    for k in range(2):
        acc = None
        for l in range(3):
            f = cols[l][:, k] if variant == "finv_transposed" else cols[k][:, l]
            term = (-f) / z[:, l]
            acc = term if acc is None else acc + term
        tmp.append(acc)
    g = lift(g_depth[b, (S - 1 - y) if (flip and variant != "flip_ignored") else y, x], ar)
    if s_depth is not None:
        g = g * s_depth
    w, d = lift(sc["wmap"][b, y, x], ar), lift(sc["dmap"][b, y, x], ar)
    d2 = d * d
    vals = []
    for k in range(3):
        for c in range(2):
            vals.append(((((-g) * tmp[c]) * w[:, k]) * d2) * float(S) / 2.0)
        vals.append(((g * w[:, k]) * d2) / (z[:, k] * z[:, k]))
    key = b * Fp + fn
    out = scatter_(B * Fp, key, _stack1(vals))
    return reshape_(out, (B, Fp, 3, 3)), np.bincount(key, minlength=B * Fp).reshape(B, Fp, 1, 1)


def _stack1(xs):
    if isinstance(xs[0], Abs):
        return Abs(np.stack([x.v for x in xs], 1), np.stack([x.a for x in xs], 1))
    return np.stack(xs, 1)


def to_vertices(sc, gf, n, variant=None, tri=None):
    """VertexTarget::vertex (csrc/d3m_device.h): corner n of virtual face f' goes to vertex tri[f][n], of the back copy to tri[f][2 - n].
    Only the faces that own a pixel add.  -> (grad_vertices [B,V,3], terms per vertex)"""
    B, F, Fp, V = sc["B"], sc["F"], sc["Fp"], sc["V"]
    tri = np.broadcast_to(np.asarray(sc["tri"] if tri is None else tri, np.int64).reshape(-1, F, 3), (B, F, 3))     # (tri_batch 1 | B)
    keys = np.asarray(sorted(sc["box"]), np.int64)
    b, fn = keys // Fp, keys % Fp
    back = fn >= F
    idx, rows, cnt = [], [], []
    for c in range(3):
        m = np.where(back & (variant != "back_vertices_unreversed"), 2 - c, c)
        idx.append(b * V + tri[b, fn % F, m])
        rows.append(take_(gf, (b, fn, c)))
        cnt.append(n[b, fn, 0, 0] + 1)
    idx = np.concatenate(idx)
    out = scatter_(B * V, idx, cat_(rows))
    terms = np.zeros(B * V, np.int64)
    np.add.at(terms, idx, np.concatenate(cnt))
    return reshape_(out, (B, V, 3)), terms.reshape(B, V, 1)


# ==== references: (float64 value, per-element tolerance, E32) ======================================================================
def D_k5(n, views=0, scaled=False):
    return n + TREE + CHAIN_K5 + views + (SCALE_D if scaled else 0)


def D_k6(n, scaled=False):
    return n + TREE + CHAIN_K6 + (SCALE_D if scaled else 0)


def lit_reference(sc, inp, ts, form=None):
    """dict(gtex, glight): each (ref, tol, E32)"""
    r = {ar: lit_adjoint(sc, inp, ts, ar, form=form) for ar in ("f64", "f32", "abs")}
    B, tb, lb = sc["B"], inp["tex"].shape[0], inp["light"].shape[0]
    out = {}
    for name, nk, shared in (("gtex", "n_tex", tb == 1), ("glight", "n_light", lb == 1)):
        bnd = r["abs"][name].a
        e = e32_of(r["f32"][name], r["f64"][name], bnd)
        D = D_k5(r["f64"][nk], B if shared else 0, form is not None) + (1 if name == "glight" else 0)
        out[name] = (np.asarray(r["f64"][name], np.float64), tolerance(D, e, bnd), e)
    return out


def depth_reference(sc, inp, form=None, finv_map=False, flip=False, vertices=False, tri=None):
    """(ref, tol, E32) of grad_faces [B,Fp,3,3], or of grad_vertices [B,V,3]"""
    def run(ar):
        s = scales(inp, form, ar)[1]
        gf, n = depth_adjoint(sc, inp["g_depth"], ar, finv_map=finv_map, flip=flip, s_depth=s)
        return to_vertices(sc, gf, n, tri=tri) if vertices else (gf, n)
    f64, n = run("f64")
    f32, ab = run("f32")[0], run("abs")[0]
    e = e32_of(f32, f64, ab.a)
    return np.asarray(f64, np.float64), tolerance(D_k6(n, form is not None), e, ab.a), e


def outside(got, ref):
    """the GPU test's float comparison: some element off by more than its tolerance (a NaN is outside)"""
    want, tol, _ = ref
    return not bool((np.abs(np.asarray(got, np.float64) - want) <= tol).all())
