"""The gathered texture / depth backward scans a face's box for owner indices alone and runs its arithmetic for the pixels
the face owns (csrc/d3m_face_major.h, scan_owned_pixels).  These tests hold the compaction to the EXACT pixel set on the
smallest scenes at which it can go wrong -- hand-placed triangles, every property checked on the CPU from the oracle's
face_index_map before anything runs on the device -- through the lit node at ts = 2, 3, 4 and the depth mode, with eight
lanes per face and with a wave per face, with and without the deterministic mode."""
import functools

import numpy as np
import pytest
import torch

from conftest import kernels_launched
from test_gpu_renderer import GRAD_TOL, _association, _compare_end_to_end, _rel_max

pytestmark = pytest.mark.gpu

CHUNK = {8: 32, 64: 64}         # box pixels per chunk of the scan: LANES * K
MAX_BOX = 4096                  # FM_MAX_BBOX_AREA
OFF_SCREEN = 3.0                # NDC x of the padding triangles: no pixel box at all


def _ndc(px, S):
    """pixel coordinate (pixel centres at the integers) -> NDC: the inverse of csrc/d3m_device.h to_pixel()"""
    return (2.0 * np.asarray(px, np.float64) + 1.0 - S) / S


def _row(X, Y, n, z, back=False):
    """One image row tall: box n x 1 from (X, Y); the hypotenuse crosses the row of centres at X + n / 2 - 0.5 (n even)
    or - 0.4 (n odd), so the face owns the first ceil(n / 2) of them."""
    t = [(X - 0.4, Y - 0.3, z), (X + n - (0.4 if n % 2 else 0.6), Y - 0.3, z), (X - 0.4, Y + 0.3, z)]
    return t[::-1] if back else t


def _tri(p0, p1, p2, z, back=False):
    t = [(p0[0], p0[1], z), (p1[0], p1[1], z), (p2[0], p2[1], z)]
    return t[::-1] if back else t


def _quad(x0, y0, x1, y1, z):
    return [_tri((x0, y0), (x1, y0), (x0, y1), z), _tri((x1, y0), (x1, y1), (x0, y1), z)]


def _scene_triangles(name):
    """(image size, triangles in pixel coordinates [(x, y, z) * 3], names of the faces the properties are about)"""
    if name == "counts":
        # faces owning exactly 1, 7, 8, 9, 16, 17 pixels; boxes of one chunk (32 / 64 pixels) and one chunk + 1 (33 / 65);
        # two of them wound the other way, so that the fill_back copy owns their pixels
        S, tris, tag = 96, [], {}
        for i, (c, n, back) in enumerate([(1, 2, False), (7, 14, False), (8, 16, False), (9, 18, False), (16, 32, False),
                                          (17, 33, False), (17, 34, False), (32, 64, False), (33, 65, False),
                                          (7, 14, True), (9, 18, True)]):
            tag[f"row{n}{'b' if back else ''}"] = (len(tris), c, n)
            tris.append(_row(5 + i, 4 + 8 * i, n, 1.0 + 0.1 * i, back))
        return S, tris, tag
    if name == "holes":
        S, tris, tag = 48, [], {}
        # a 12 x 12 box (five chunks of 32, three of 64) whose rows but the last lie behind a nearer quad
        tag["last"] = (len(tris),)
        tris.append(_tri((4 - 0.4, 15 + 0.3), (15 + 0.4, 15 + 0.3), (9.5, 4 - 0.3), 2.0))
        tris += _quad(2.6, 2.6, 17.4, 14.4, 1.0)
        # a 10 x 9 box crossed by a needle in front: whole box rows of foreign pixels between the face's own
        tag["needle"] = (len(tris),)
        tris.append(_tri((24 - 0.4, 20 - 0.3), (33 + 0.4, 20 - 0.3), (24 - 0.4, 28 + 0.3), 2.0, back=True))
        tris += _quad(20.6, 22.6, 40.4, 25.4, 1.0)
        return S, tris, tag
    if name == "one_of_eight":
        # the only eight faces that own a pixel: seven boxes within the first chunk, one that owns pixels in its second
        S, tris, tag = 32, [], {}
        for i in range(8):
            if i == 5:
                tag["second"] = (len(tris),)
                tris.append(_tri((20 - 0.4, 14 - 0.3), (20 - 0.4, 19 + 0.3), (27 + 0.4, 19 + 0.3), 1.5))
            else:
                tris.append(_row(2, 2 + 3 * i, 4 + 2 * i, 1.5))
        return S, tris, tag
    if name == "limit":
        # a box of exactly FM_MAX_BBOX_AREA pixels, and one just above it: handed to the per-pixel kernel, except in the
        # deterministic mode, where a box of any size stays in the gathered pass
        S, tag = 96, {"at": (0,), "above": (1,)}
        tris = [_tri((10 - 0.3, 10 - 0.3), (73 + 0.3, 10 - 0.3), (10 - 0.3, 73 + 0.3), 2.0),
                _tri((84 + 0.3, 88 + 0.3), (20 - 0.3, 88 + 0.3), (84 + 0.3, 25 - 0.3), 1.5)]
        return S, tris, tag
    raise KeyError(name)


SCENES = ("counts", "holes", "one_of_eight", "limit")


def _pixel_bbox(face, S):
    """csrc/d3m_forward.h pixel_bbox() restated: the box the gathered passes scan"""
    x, y = face[:, 0].astype(np.float64), face[:, 1].astype(np.float64)
    m = 4e-6 * (max(np.abs(x).max(), np.abs(y).max()) + 1.0)
    lx, hx = np.ceil(((x.min() - m) * S + S - 1) * 0.5), np.floor(((x.max() + m) * S + S - 1) * 0.5)
    ly, hy = np.ceil(((y.min() - m) * S + S - 1) * 0.5), np.floor(((y.max() + m) * S + S - 1) * 0.5)
    if lx > S - 1 or hx < 0 or ly > S - 1 or hy < 0 or lx > hx or ly > hy:
        return None
    return int(max(lx, 0)), int(min(hx, S - 1)), int(max(ly, 0)), int(min(hy, S - 1))


@functools.lru_cache(maxsize=None)
def _scene(name, lanes):
    """The mesh (every triangle has its own three vertices), padded with off-screen triangles until the launch rule --
    a wave per face above 48 raster pixels per triangle -- picks `lanes`; the oracle's face_index_map of it; each
    face's box and the box offsets of the pixels it owns.  The scene's properties are asserted here, on the CPU."""
    from oracle import nr_oracle as O
    S, tris, tag = _scene_triangles(name)
    n_real = len(tris)
    while (S * S > 48 * len(tris)) != (lanes == 64):
        assert lanes == 8
        k = len(tris)
        tris.append([(S * OFF_SCREEN + k, 1.0, 1.0), (S * OFF_SCREEN + k + 3.0, 1.0, 1.0), (S * OFF_SCREEN + k, 4.0, 1.0)])
    t = np.asarray(tris, np.float64)
    v = np.concatenate([_ndc(t[..., :2], S), t[..., 2:]], -1).reshape(-1, 3).astype(np.float32)
    tri = np.arange(v.shape[0], dtype=np.int32).reshape(-1, 3)
    F = tri.shape[0]
    faces = v[tri]
    faces2 = np.concatenate([faces, faces[:, ::-1]], 0)[None]                    # fill_back (NR/renderer.py:86)
    fim = O.raster_forward(faces2, None, S, 0.1, 100, 1e-3, None, False, True, False)["face_index_map"][0]
    box, owned = {}, {}
    for fn in np.unique(fim[fim >= 0]):
        b = _pixel_bbox(faces2[0, fn], S)
        ys, xs = np.nonzero(fim == fn)
        assert b and xs.min() >= b[0] and xs.max() <= b[1] and ys.min() >= b[2] and ys.max() <= b[3]
        box[int(fn)] = b
        owned[int(fn)] = np.sort((ys - b[2]) * (b[1] - b[0] + 1) + (xs - b[0]))
    area = {fn: (b[1] - b[0] + 1) * (b[3] - b[2] + 1) for fn, b in box.items()}
    ch = CHUNK[lanes]
    assert all(fn % F < n_real for fn in owned)                                   # the padding owns nothing

    def fn_of(key):                 # the copy of the face that owns its pixels
        f = tag[key][0]
        got = [fn for fn in (f, f + F) if fn in owned]
        assert len(got) == 1, key
        return got[0]
    if name == "counts":
        for key, (f, c, n) in tag.items():
            fn = fn_of(key)
            assert len(owned[fn]) == c and area[fn] == n and (fn >= F) == key.endswith("b"), (key, len(owned[fn]), area[fn])
        assert {len(owned[fn_of(k)]) for k in tag} >= {1, 7, 8, 9, 16, 17}
        assert {area[fn_of(k)] for k in tag} >= {ch, ch + 1}
        assert any(fn >= F for fn in owned)                                        # back copies of fill_back
    elif name == "holes":
        fn = fn_of("last")
        assert area[fn] > 2 * ch and len(owned[fn]) >= 8 and owned[fn].min() >= (area[fn] - 1) // ch * ch
        fn = fn_of("needle")
        bw = box[fn][1] - box[fn][0] + 1
        rows = np.unique(owned[fn] // bw)
        assert fn >= F and np.diff(rows).max() >= 3 and len(rows) >= 4            # whole foreign rows between its own
    elif name == "one_of_eight":
        assert len(owned) == 8
        second = fn_of("second")
        assert owned[second].max() >= CHUNK[8] and all(area[fn] <= CHUNK[8] for fn in owned if fn != second)
    elif name == "limit":
        assert area[fn_of("at")] == MAX_BOX and MAX_BOX < area[fn_of("above")] <= MAX_BOX + 64
        assert len(owned[fn_of("at")]) > 1000 and len(owned[fn_of("above")]) > 1000
    return dict(S=S, F=F, v=torch.from_numpy(v)[None], tri=torch.from_numpy(tri)[None], fim=fim)


def _maps(S):
    """per-pixel gradient weights, different for every pixel and strictly positive (uniform in [0.5, 1])"""
    gen = torch.Generator().manual_seed(S)
    return (torch.rand(1, 3, S, S, generator=gen) * 0.5 + 0.5, torch.rand(1, S, S, generator=gen) * 0.5 + 0.5,
            torch.rand(1, S, S, generator=gen))


def _run_lit(mod, dev, sc, ts):
    """unit light (ambient 1, directional 0): [rgb, depth, alpha, loss, grad_vertices, grad_textures]"""
    from deep3dmap_amd import synthetic
    S = sc["S"]
    r = mod.Renderer(image_size=S, anti_aliasing=False, camera_mode="look_at", perspective=False, fill_back=True,
                     light_intensity_ambient=1.0, light_intensity_directional=0.0, background_color=[0.2, 0.3, 0.4])
    r.camera_mode = "none"              # the vertices as they are: the triangles are placed in pixel coordinates
    g_rgb, g_depth, t_alpha = (m.to(dev) for m in _maps(S))
    vv = sc["v"].clone().to(dev).requires_grad_(True)
    tt = torch.from_numpy(synthetic.random_textures(sc["F"], ts))[None].to(dev).requires_grad_(True)
    rgb, depth, alpha = r(vv, sc["tri"].to(dev), tt)
    loss = (rgb * g_rgb).sum() + (depth.clamp(max=5.0) * g_depth).sum() * 0.1 + ((alpha - t_alpha) ** 2).sum()
    loss.backward()
    return [x.detach().cpu() for x in (rgb, depth, alpha, loss, vv.grad, tt.grad)]


def _run_depth(mod, dev, sc):
    S = sc["S"]
    r = mod.Renderer(image_size=S, anti_aliasing=False, camera_mode="look_at", perspective=False, fill_back=True)
    r.camera_mode = "none"
    vv = sc["v"].clone().to(dev).requires_grad_(True)
    depth = r(vv, sc["tri"].to(dev), mode="depth")
    (depth.clamp(max=5.0) * _maps(S)[1].to(dev)).sum().backward()
    return depth.detach().cpu(), vv.grad.detach().cpu()


@functools.lru_cache(maxsize=None)
def _oracle_lit(name, lanes, ts):
    from oracle import nr_oracle as O
    with _association("product"):
        return _run_lit(O, "cpu", _scene(name, lanes), ts)


@functools.lru_cache(maxsize=None)
def _oracle_depth(name, lanes):
    from oracle import nr_oracle as O
    with _association("product"):
        return _run_depth(O, "cpu", _scene(name, lanes))


def _check_owned_sums(sc, grad_textures):
    """The eight trilinear corner weights of a pixel sum to 1, so with unit light the texel gradients of a face, summed
    over its texels, are the sum of grad_rgb over EXACTLY the pixels its two copies own: a dropped or doubled pixel is off
    by >= 0.5 in a sum of at most n.  Tolerance: summation rounding, n * 2^-23 * sum |terms|.  Every face is checked."""
    S, F = sc["S"], sc["F"]
    g_map = _maps(S)[0][0].flip(1).numpy().astype(np.float64)                 # the map's row y is the image's row S-1-y
    covered = sc["fim"] >= 0
    owner = sc["fim"][covered] % F
    n = np.bincount(owner, minlength=F)
    got = grad_textures[0].double().reshape(F, -1, 3).sum(1).numpy()
    assert n.max() > 0
    for c in range(3):
        want = np.bincount(owner, weights=g_map[c][covered], minlength=F)
        tol = n * 2.0 ** -23 * want
        bad = np.nonzero(np.abs(got[:, c] - want) > tol)[0]
        assert bad.size == 0, [(int(f), int(n[f]), float(got[f, c]), float(want[f])) for f in bad[:8]]


@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("ts", [2, 3, 4])
@pytest.mark.parametrize("lanes", [8, 64])
@pytest.mark.parametrize("name", SCENES)
def test_lit_node_sums_exactly_the_owned_pixels(name, lanes, ts, deterministic):
    from deep3dmap_amd import _lib, neural_renderer as nr
    sc = _scene(name, lanes)
    ref = _oracle_lit(name, lanes, ts)
    with _lib.deterministic(deterministic):
        with kernels_launched() as k:
            got = _run_lit(nr, "cuda", sc, ts)
        assert "k_backward_textures_lit_faces" in k.names, sorted(k.names)
        if deterministic:                                   # run to run: bit-identical
            again = _run_lit(nr, "cuda", sc, ts)
            assert torch.equal(got[4], again[4]) and torch.equal(got[5], again[5])
    assert torch.equal((torch.from_numpy(sc["fim"]) >= 0).flip(0)[None].float(), got[2])
    _check_owned_sums(sc, got[5])
    _compare_end_to_end(ref, got, "product", f"owned_scan[{name},{lanes},{ts}]")


@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("lanes", [8, 64])
@pytest.mark.parametrize("name", SCENES)
def test_depth_mode_sums_exactly_the_owned_pixels(name, lanes, deterministic):
    from deep3dmap_amd import _lib, neural_renderer as nr
    sc = _scene(name, lanes)
    ref = _oracle_depth(name, lanes)
    with _lib.deterministic(deterministic):
        with kernels_launched() as k:
            got = _run_depth(nr, "cuda", sc)
        assert "k_backward_depth_faces" in k.names, sorted(k.names)
        if deterministic:
            assert torch.equal(got[1], _run_depth(nr, "cuda", sc)[1])
    assert torch.equal(ref[0] < 50, got[0] < 50)
    assert _rel_max(got[1], ref[1]) < GRAD_TOL and float(ref[1].abs().max()) > 0
