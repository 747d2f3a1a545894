"""The fused fit objective's VOID TILES (d3m_fit_targets.tile_void): a tile of the objective's pass of which neither the
targets nor the mesh ask anything does no memory work, and the line walk stages its pixels as constants.  Every scene runs
with the summary and, under D3M_FIT_VOID_TILES=0, without it, in both tile sizes of the pass (d3m_set_fit_tile_form): the
loss must be bit-equal and the gradients equal (-0 == 0); and against the oracle's kernels fed with the objective's
gradient maps, at the tolerance of tests/test_gpu_ops.py (1e-3 of a gradient's own scale).

Scenes are hand-placed in OUTPUT pixel coordinates (row 0 = top), two views, quads of two triangles; the light is ambient
white (lit texture = texture) and the screen vertices are given directly (no camera)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GRAD_RTOL = 1e-3            # tests/test_gpu_ops.py: north_star's bound on backward gradients, of the tensor's own scale
FWD_ATOL = 1e-6             # ... and its bound on forward floats
NEAR, FAR, EPS = 0.1, 100.0, 1e-3
LIGHT = (1.0, 0.0, [1, 1, 1], [1, 1, 1], [0, 1, 0])


# ---------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------
def _mesh(quads_per_view, S):
    """quads_per_view: per view a list of (x0, y0, x1, y1, z) in output pixels -> screen vertices [B,V,3], tri [F,3]"""
    B, nq = len(quads_per_view), len(quads_per_view[0])
    sv = np.zeros((B, 4 * nq, 3), np.float32)
    tri = np.zeros((2 * nq, 3), np.int32)
    for b, quads in enumerate(quads_per_view):
        assert len(quads) == nq
        for q, (x0, y0, x1, y1, z) in enumerate(quads):
            for c, (x, y) in enumerate(((x0, y0), (x1, y0), (x1, y1), (x0, y1))):
                sv[b, 4 * q + c] = (2.0 * x / S - 1.0, 1.0 - 2.0 * y / S, z)
    for q in range(nq):
        tri[2 * q] = (4 * q, 4 * q + 2, 4 * q + 1)         # (the winding the rasterizer keeps)
        tri[2 * q + 1] = (4 * q, 4 * q + 3, 4 * q + 2)
    return sv, tri


def _box(B, S, x0, y0, x1, y1):
    m = np.zeros((B, S, S), np.float32)
    m[:, int(y0):int(y1), int(x0):int(x1)] = 1.0
    return m


def _targets(S, alpha_t, mask, seed):
    """finite, non-zero rgb / depth targets EVERYWHERE (a target-void tile must give the same result whatever they hold)"""
    rng = np.random.default_rng(seed)
    B = alpha_t.shape[0]
    rgb_t = rng.uniform(0.05, 0.95, (B, 3, S, S)).astype(np.float32)
    depth_t = rng.uniform(0.5, 3.0, (B, S, S)).astype(np.float32)
    return rgb_t, depth_t, alpha_t.astype(np.float32), mask.astype(np.float32)


def _scene(name, S):
    """-> dict(sv [B,V,3], tri, tex, targets (rgb_t, depth_t, alpha_t, mask), bg)"""
    f = S / 64.0
    bg = (0.0, 0.0, 0.0)
    if name in ("classes", "classes_bg", "classes_bg_views", "mask_only", "nonfinite"):
        # a quad in the upper left and one in the lower right; the targets live in the right part of the image only:
        # upper left = covered with void targets, upper right = live targets without coverage, lower right = both,
        # lower left = void
        quads = [[(5.3 * f, 6.2 * f, 25.6 * f, 24.7 * f, 1.5), (38.4 * f, 37.3 * f, 58.7 * f, 57.6 * f, 2.0)],
                 [(8.6 * f, 4.4 * f, 27.2 * f, 22.3 * f, 1.2), (36.7 * f, 40.2 * f, 56.3 * f, 59.4 * f, 1.8)]]
        sv, tri = _mesh(quads, S)
        alpha_t = _box(2, S, 36 * f, 3 * f, 61 * f, 61 * f)
        mask = _box(2, S, 34 * f, 8 * f, 60 * f, 55 * f)
        if name == "mask_only":                     # the mask is non-zero only in a tile without coverage; no silhouette target
            sv, tri = _mesh([q[:1] for q in quads], S)
            alpha_t = np.zeros((2, S, S), np.float32)
            mask = _box(2, S, 40 * f, 38 * f, 52 * f, 50 * f)
        t = _targets(S, alpha_t, mask, 11)
        if name == "nonfinite":
            # mask 0 and alpha_t 0 there, but an inf / a NaN among the targets: 0 * inf is NaN, the tile must NOT be flagged
            t[0][0, 1, S - 5, 3] = np.inf           # rgb_t, lower left
            t[1][0, S - 20, 7] = np.nan             # depth_t, lower left, another tile of 16 x 16 (view 1 keeps its void tiles)
        if name == "classes_bg":
            bg = (0.2, 0.45, 0.7)
        if name == "classes_bg_views":
            bg = np.array([[0.2, 0.45, 0.7], [0.9, 0.1, 0.35]], np.float32)
    elif name in ("ring", "ring_plug"):
        # four quads around a hole; the targets are the same ring shifted: the hole holds whole void tiles of the pass (16 x 16
        # at every size, 32 x 32 at S = 80 and S = 96) INSIDE the non-zero extent of every line that crosses them
        lo, hi, o_lo, o_hi = {64: (13.6, 50.3, 4.2, 60.6), 80: (13.6, 66.3, 5.2, 75.6), 96: (29.6, 66.3, 12.2, 84.6)}[S]
        quads = []
        for dx, dy in ((0.0, 0.0), (1.7, -1.2)):
            quads.append([(o_lo + dx, o_lo + dy, o_hi + dx, lo + dy, 1.5), (o_lo + dx, hi + dy, o_hi + dx, o_hi + dy, 1.6),
                          (o_lo + dx, lo + dy, lo + dx, hi + dy, 1.7), (hi + dx, lo + dy, o_hi + dx, hi + dy, 1.8)])
        if name == "ring_plug":                     # a fifth quad in front that covers the whole hole (moved away by the test)
            for q, (dx, dy) in zip(quads, ((0.0, 0.0), (1.7, -1.2))):
                q.append((lo - 1.5 + dx, lo - 1.5 + dy, hi + 1.5 + dx, hi + 1.5 + dy, 1.0))
        sv, tri = _mesh(quads, S)
        alpha_t = _box(2, S, o_lo + 3, o_lo - 2, o_hi + 3, o_hi - 2) - _box(2, S, int(lo) + 2, int(lo) + 2, int(hi) - 1, int(hi) - 1)
        t = _targets(S, alpha_t, alpha_t, 12)
    else:
        raise ValueError(name)
    rng = np.random.default_rng(5)
    tex = rng.uniform(0.1, 0.9, (1, tri.shape[0], 2, 2, 2, 3)).astype(np.float32)
    return dict(sv=sv, tri=tri, tex=tex, targets=t, bg=bg, S=S)


# ---------------------------------------------------------------------------------------------------------------------
# the three evaluations: the library with / without void tiles, the oracle
# ---------------------------------------------------------------------------------------------------------------------
def _target_void_cpu(targets, S):
    """the summary from its definition: per (view, 16 x 16 output tile), tiles past the edge count their pixels inside"""
    rgb_t, depth_t, alpha_t, mask = targets
    ok = (alpha_t == 0) & (mask == 0) & np.isfinite(depth_t) & np.isfinite(rgb_t).all(1)
    n16 = (S + 15) // 16
    pad = np.ones((ok.shape[0], n16 * 16, n16 * 16), bool)
    pad[:, :S, :S] = ok
    return pad.reshape(-1, n16, 16, n16, 16).all((2, 4))


def _pass_tiles(c, tile, face_index_map):
    """the pass's tiles (internal rows: row 0 = bottom) -> (view, y0, y1, x0, x1, targets void, covered) each"""
    S = c["S"]
    tv16 = _target_void_cpu(c["targets"], S)
    n = (S + tile - 1) // tile
    for b in range(tv16.shape[0]):
        for j in range(n):
            for i in range(n):
                y0, y1, x0, x1 = j * tile, min((j + 1) * tile, S), i * tile, min((i + 1) * tile, S)
                yo0, yo1 = S - y1, S - 1 - y0
                tvoid = bool(tv16[b, yo0 // 16: yo1 // 16 + 1, x0 // 16: (x1 - 1) // 16 + 1].all())
                yield b, y0, y1, x0, x1, tvoid, bool((face_index_map[b, y0:y1, x0:x1] >= 0).any())


def _tile_classes(c, tile, face_index_map):
    """counts of (void, covered + void targets, live targets + uncovered, both)"""
    counts = np.zeros(4, int)
    for *_, tvoid, covered in _pass_tiles(c, tile, face_index_map):
        counts[(0 if tvoid else 2) + (1 if covered else 0)] += 1
    return counts


def _void_tile_between_coverage(c, tile, face_index_map):
    """some void tile of the pass has covered pixels on BOTH sides of it on the row line and the column line through it"""
    for b, y0, y1, x0, x1, tvoid, covered in _pass_tiles(c, tile, face_index_map):
        fi, y, x = face_index_map[b] >= 0, (y0 + y1) // 2, (x0 + x1) // 2
        if tvoid and not covered and fi[y, :x0].any() and fi[y, x1:].any() and fi[:y0, x].any() and fi[y1:, x].any():
            return True
    return False


def _sign(x):
    return (x > 0).astype(np.float32) - (x < 0).astype(np.float32)      # (0 for NaN, as the objective's kernels)


_ORACLE = {}


def _oracle(c, key=None):
    """loss, d/d(screen vertices), d/d(textures), images and the face index map from the oracle's kernels: once per scene"""
    if key is not None and key in _ORACLE:
        return _ORACLE[key]
    from oracle import nr_oracle as O
    sv, tri, S = c["sv"], c["tri"], c["S"]
    B = sv.shape[0]
    faces = sv[:, tri.astype(np.int64)]
    tex = np.broadcast_to(c["tex"], (B,) + c["tex"].shape[1:]).copy()
    m = O.raster_forward(faces, tex, S, NEAR, FAR, EPS, c["bg"], True, True, True)
    rgb_t, depth_t, alpha_t, mask = c["targets"]
    to_map = lambda t: np.ascontiguousarray(t[:, ::-1])                  # output rows -> internal rows
    rt, dt, at, mk = to_map(np.transpose(rgb_t, (0, 2, 3, 1))), to_map(depth_t), to_map(alpha_t), to_map(mask)
    den = np.float32(mask.sum())
    with np.errstate(invalid="ignore"):
        loss = (np.abs(m["rgb_map"] - rt) * mk[..., None]).sum(dtype=np.float64) / (3.0 * den) + \
            ((m["alpha_map"] - at) ** 2).sum(dtype=np.float64) / (S * S) + (np.abs(m["depth_map"] - dt) * mk).sum(dtype=np.float64) / den
        g_rgb = _sign(m["rgb_map"] - rt) * mk[..., None] / (3.0 * den)
        g_alpha = 2.0 * (m["alpha_map"] - at) / np.float32(S * S)
        g_depth = _sign(m["depth_map"] - dt) * mk / den
    gf, gt = O.raster_backward(m, g_rgb.astype(np.float32), g_alpha.astype(np.float32), g_depth.astype(np.float32), True, True, True)
    gsv = np.zeros_like(sv)
    np.add.at(gsv, (np.arange(B)[:, None], tri.astype(np.int64).reshape(1, -1)), gf.reshape(B, -1, 3))
    out = dict(loss=float(loss), gsv=gsv, gtex=gt.sum(0, keepdims=True), face_index_map=m["face_index_map"],
               rgb=np.transpose(m["rgb_map"][:, ::-1], (0, 3, 1, 2)), alpha=m["alpha_map"][:, ::-1], depth=m["depth_map"][:, ::-1])
    if key is not None:
        _ORACLE[key] = out
    return out


class _Form:
    """both tile sizes of the objective's pass: d3m_set_fit_tile_form(0 = 16 | 1 = 32) for forward AND backward"""

    def __init__(self, form):
        self.form = form

    def __enter__(self):
        from deep3dmap_amd import _lib
        self.old = _lib.lib().d3m_get_fit_tile_form()
        _lib.check(_lib.lib().d3m_set_fit_tile_form(self.form), "d3m_set_fit_tile_form")

    def __exit__(self, *exc):
        from deep3dmap_amd import _lib
        _lib.lib().d3m_set_fit_tile_form(self.old)


def _device_scene(c):
    sv = torch.from_numpy(c["sv"]).cuda().requires_grad_(True)
    tex = torch.from_numpy(c["tex"]).cuda().requires_grad_(True)
    tri = torch.from_numpy(c["tri"]).cuda()[None]
    targets = tuple(torch.from_numpy(t).cuda() for t in c["targets"])
    bg = torch.from_numpy(c["bg"]).cuda() if isinstance(c["bg"], np.ndarray) else c["bg"]
    return sv, tex, tri, targets, bg


def _expected_flags(c, tile):
    """what the pass must leave in its scratch: [B, tiles_y, tiles_x] (internal rows), 1 = void targets and no coverage"""
    fi = _oracle(c)["face_index_map"] if "fi" not in c else c["fi"]
    n = (c["S"] + tile - 1) // tile
    return np.array([tvoid and not covered for *_, tvoid, covered in _pass_tiles(c, tile, fi)], np.uint8).reshape(-1, n, n)


def _fit(c, images=False, dev=None, flags_of_tile=None):
    """one step of the fused objective -> [loss, grad_sv, grad_tex[, images]] as numpy.  flags_of_tile (16 | 32): also
    asserts ON THE DEVICE's data that the pass flagged exactly the void tiles (its bytes in the objective's scratch)."""
    from deep3dmap_amd import _lib
    from deep3dmap_amd.neural_renderer.rasterize import rasterize_lit_fit
    sv, tex, tri, targets, bg = dev if dev is not None else _device_scene(c)
    sv.grad = tex.grad = None
    S, B = c["S"], c["sv"].shape[0]
    out = (torch.empty(B, 3, S, S, device="cuda"), torch.empty(B, S, S, device="cuda"), torch.empty(B, S, S, device="cuda")) \
        if images else None
    loss = rasterize_lit_fit(sv, sv.detach()[:1], tri, tex, LIGHT, False, targets, S, NEAR, FAR, EPS, bg, images_out=out)
    if flags_of_tile:
        state = loss.grad_fn.state.fit
        assert state.tile_void is not None, "the pass ran without the targets' summary"
        n, off = (S + flags_of_tile - 1) // flags_of_tile, int(_lib.lib().d3m_render_fit_scratch_tile_void_offset(B, S))
        got = state.scratch[0][off:].view(torch.uint8)[:B * n * n].reshape(B, n, n).cpu().numpy()
        want = _expected_flags(c, flags_of_tile)
        assert np.array_equal(got, want), (got, want)
    loss.backward()
    r = [loss.detach().cpu().numpy(), sv.grad.cpu().numpy(), tex.grad.cpu().numpy()]
    if images:
        r.append(tuple(t.cpu().numpy() for t in out))       # (rgb, depth, alpha)
    return r


def _hostile_step(c, images=False):
    """Leaves HOSTILE stale data where the next step's uninitialised buffers will lie (the same allocation sequence: the
    caching allocator hands the same blocks back): the same mesh with every quad blown up over the whole image and a
    target that is live everywhere, through the pass that writes every tile -- records with large gradients, an owner and
    T != 0, alpha 1, texture colours and a depth gradient at EVERY pixel.  A void tile whose reader looked at memory instead
    of the tile's byte would read these."""
    d = dict(c)
    sv = c["sv"].copy()
    corners = np.array([(-1.3, 1.3), (1.3, 1.3), (1.3, -1.3), (-1.3, -1.3)], np.float32)
    for q in range(sv.shape[1] // 4):
        sv[:, 4 * q:4 * q + 4, :2] = corners
    rgb_t, depth_t, alpha_t, mask = c["targets"]
    d["sv"], d["targets"] = sv, (np.where(np.isfinite(rgb_t), 1.0 - rgb_t, 0.5).astype(np.float32),
                                np.full_like(depth_t, 7.0), np.zeros_like(alpha_t), np.ones_like(mask))
    old = os.environ.get("D3M_FIT_VOID_TILES")
    os.environ["D3M_FIT_VOID_TILES"] = "0"
    try:
        r = _fit(d, images)
    finally:
        if old is None:
            del os.environ["D3M_FIT_VOID_TILES"]
        else:
            os.environ["D3M_FIT_VOID_TILES"] = old
    assert np.abs(r[1]).max() > 0
    torch.cuda.synchronize()


def _assert_same(got, ref):
    """loss bit-equal (NaN included), gradients equal as numbers (-0 == 0)"""
    assert got[0].tobytes() == ref[0].tobytes(), (got[0], ref[0])
    assert np.array_equal(got[1], ref[1], equal_nan=True), np.nanmax(np.abs(got[1] - ref[1]))
    assert np.array_equal(got[2], ref[2], equal_nan=True), np.nanmax(np.abs(got[2] - ref[2]))


def _assert_oracle(got, ref):
    if np.isnan(ref["loss"]):
        assert np.isnan(got[0])
    else:
        assert abs(float(got[0]) - ref["loss"]) <= 2e-6 * abs(ref["loss"]), (float(got[0]), ref["loss"])
    for g, r in ((got[1], ref["gsv"]), (got[2], ref["gtex"])):
        scale = float(np.abs(r).max())              # (0: the texture gradient of a mask that lies on no face)
        assert np.abs(g - r).max() <= GRAD_RTOL * scale, (np.abs(g - r).max(), scale)


def _flagged_share(c, monkeypatch):
    """the share of flagged tiles, asserted on the CPU from the targets -- and the kernel's summary is that very array"""
    import importlib
    R = importlib.import_module("deep3dmap_amd.neural_renderer.rasterize")      # (the package exports a function of that name)
    want = _target_void_cpu(c["targets"], c["S"])
    monkeypatch.delenv("D3M_FIT_VOID_TILES", raising=False)
    got = R.target_void_summary(*(torch.from_numpy(t).cuda() for t in c["targets"]))
    assert np.array_equal(got.cpu().numpy().astype(bool), want)
    share = float(want.mean())
    assert 0.0 < share < 1.0, share
    return want


def _assert_same_to_atomics(got, ref):
    """the default mode: the loss is a sum in a fixed order (bit-equal); a vertex's gradient is added up by float atomics in
    arrival order -- equal to a few ulp of the largest addend, 1e-5 of the tensor's scale (as tests/test_gpu_renderer.py)"""
    assert got[0].tobytes() == ref[0].tobytes(), (got[0], ref[0])
    for g, r in ((got[1], ref[1]), (got[2], ref[2])):
        assert np.abs(g - r).max() <= 1e-5 * float(np.abs(r).max())


def _run_both(c, monkeypatch, form, images=False):
    """-> (with void tiles, without) in the DETERMINISTIC mode -- the gradients are sums in a fixed order there, so "equal"
    is meaningful (the default mode adds a vertex's contributions with float atomics in arrival order: two runs of ONE
    library may differ in the last bit) -- and with void tiles in the default mode (side streams).  Each run with void
    tiles comes right behind a HOSTILE step (_hostile_step), so what its void tiles leave unwritten is wrong data, and
    asserts the pass's flags as the device holds them."""
    from deep3dmap_amd import _lib
    tile = 32 if form else 16
    with _Form(form):
        with _lib.deterministic():
            monkeypatch.setenv("D3M_FIT_VOID_TILES", "0")
            ref = _fit(c, images)
            monkeypatch.delenv("D3M_FIT_VOID_TILES")
            _hostile_step(c, images)
            got = _fit(c, images, flags_of_tile=tile)
        _hostile_step(c, images)
        default = _fit(c, images, flags_of_tile=tile)
    return got, ref, default


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
SCENES = [("classes", 64), ("classes", 80), ("ring", 64), ("ring", 80), ("ring", 96), ("mask_only", 64), ("mask_only", 80),
          ("nonfinite", 64), ("nonfinite", 80), ("classes_bg", 64), ("classes_bg_views", 64), ("classes_bg_views", 80)]


@pytest.mark.parametrize("form", [0, 1], ids=["tile16", "tile32"])
@pytest.mark.parametrize("name,S", SCENES)
def test_void_tiles_change_nothing(name, S, form, monkeypatch):
    """Cases 1-5: all four classes of tile in one image; a ring whose hole is a void tile inside every crossing line's extent
    (at S = 96 a whole 32 x 32 tile); a mask that is non-zero only where nothing is covered; non-finite targets under a zero
    mask (NOT flagged: the loss is NaN either way); non-zero and per-view backgrounds."""
    c = _scene(name, S)
    tv = _flagged_share(c, monkeypatch)
    ref_o = _oracle(c, (name, S))
    counts = _tile_classes(c, 32 if form else 16, ref_o["face_index_map"])
    small_ring = name == "ring" and S == 64 and form == 1      # (64 = two tiles of 32 a side: no room for a ring around one)
    assert counts[0] > 0 or small_ring, counts       # some tile of the pass IS void
    if name.startswith("classes"):
        assert (counts > 0).all(), counts
    if name == "ring" and not small_ring:
        assert _void_tile_between_coverage(c, 32 if form else 16, ref_o["face_index_map"])
    if name == "nonfinite":
        assert not tv[0, (S - 5) // 16, 0] and not tv[0, (S - 20) // 16, 0]
    got, ref, default = _run_both(c, monkeypatch, form)
    _assert_same(got, ref)
    _assert_oracle(got, ref_o)
    _assert_same_to_atomics(default, ref)
    _assert_oracle(default, ref_o)


@pytest.mark.parametrize("form", [0, 1], ids=["tile16", "tile32"])
@pytest.mark.parametrize("S", [64, 80])
def test_void_tiles_with_images(S, form, monkeypatch):
    """Case 7: the form that also writes the images (images_out): they are bit-equal, void tiles included, and the oracle's."""
    c = _scene("classes_bg_views", S)
    _flagged_share(c, monkeypatch)
    got, ref, default = _run_both(c, monkeypatch, form, images=True)
    _assert_same(got, ref)
    for a, b, d in zip(got[3], ref[3], default[3]):
        assert a.tobytes() == b.tobytes() and d.tobytes() == b.tobytes()
    o = _oracle(c, ("classes_bg_views", S))
    rgb, depth, alpha = got[3]
    assert np.array_equal(alpha, o["alpha"]) and np.abs(rgb - o["rgb"]).max() <= FWD_ATOL and np.abs(depth - o["depth"]).max() <= FWD_ATOL
    _assert_oracle(got, o)


@pytest.mark.parametrize("det", [True, False], ids=["deterministic", "default"])
@pytest.mark.parametrize("form", [0, 1], ids=["tile16", "tile32"])
@pytest.mark.parametrize("name,S", [("classes", 64), ("classes", 96), ("ring_plug", 80), ("ring_plug", 96)])
def test_void_tiles_over_three_steps_on_one_workspace(name, S, form, det, monkeypatch):
    """Case 6: three steps, eager and replayed from ONE captured step (one memory pool: the very same records, maps and
    flags every step), the mesh moved in place between them so that a tile goes covered -> void -> covered: the upper left
    quad of the four classes, and -- `ring_plug` -- a quad that covers the ring's hole, so that in the second step the hole's
    void tiles lie INSIDE the non-zero extent of every line through them and hold the first step's records (non-zero
    gradients, an owner, alpha 1).  Nothing is carried from step to step: every step equals the step without void tiles
    (exactly in the deterministic mode; in the default mode, with its side streams, to the order of its float atomics) and
    the oracle's."""
    import contextlib
    from deep3dmap_amd import _lib
    from deep3dmap_amd.graph import CapturedStep
    from deep3dmap_amd.neural_renderer.rasterize import rasterize_lit_fit
    base = _scene(name, S)
    t = 32 if form else 16
    shift = np.zeros_like(base["sv"])
    if name == "classes":
        shift[:, :4, 0] = 2.0 * (S // 2) / S          # the upper left quad moves half an image to the right, and back
    else:
        shift[:, -4:, 0] = 4.0                        # the plug leaves the image, and comes back
    positions = [base["sv"], base["sv"] + shift, base["sv"]]
    scenes = [dict(base, sv=p) for p in positions]
    oracles = [_oracle(s, ("three_steps", name, S, k)) for k, s in enumerate(scenes)]
    for s, o in zip(scenes, oracles):
        s["fi"] = o["face_index_map"]
    if name == "classes":
        first = [bool((o["face_index_map"][:, S - t:, :t] >= 0).any()) for o in oracles]     # the pass's tile at the upper left corner
        assert first == [True, False, True]
    else:
        assert [_void_tile_between_coverage(s, t, s["fi"]) for s in scenes] == [False, True, False]
    _flagged_share(base, monkeypatch)
    same = _assert_same if det else _assert_same_to_atomics
    with _Form(form), (_lib.deterministic() if det else contextlib.nullcontext()):
        monkeypatch.setenv("D3M_FIT_VOID_TILES", "0")
        refs = [_fit(s) for s in scenes]
        monkeypatch.delenv("D3M_FIT_VOID_TILES")
        dev = _device_scene(base)
        eager = []
        for p in positions:
            with torch.no_grad():
                dev[0].copy_(torch.from_numpy(p))
            eager.append(_fit(scenes[len(eager)], dev=dev, flags_of_tile=t))
        sv, tex, tri, targets, bg = dev
        grads = (torch.zeros_like(sv), torch.zeros_like(tex))

        def step():
            sv.grad = tex.grad = None
            loss = rasterize_lit_fit(sv, sv.detach()[:1], tri, tex, LIGHT, False, targets, S, NEAR, FAR, EPS, bg)
            loss.backward()
            grads[0].copy_(sv.grad)
            grads[1].copy_(tex.grad)
            return loss, grads[0], grads[1]

        captured = CapturedStep(step).capture()
        replayed = []
        for p in positions:
            with torch.no_grad():
                sv.copy_(torch.from_numpy(p))
            replayed.append([x.detach().cpu().numpy().copy() for x in captured()])
        torch.cuda.synchronize()
        captured.release()
    for k in range(3):
        same(eager[k], refs[k])
        same(replayed[k], refs[k])
        _assert_oracle(eager[k], oracles[k])
        _assert_oracle(replayed[k], oracles[k])
