"""Scenes, launches and plan-blob readers shared by tests/test_gpu_edge_gather_order.py and tests/test_gpu_edge_scan_batch.py
(K4, the edge gradient: deep3dmap_amd/csrc/d3m_edge_grad.h).  Not a test module."""
import numpy as np
import torch

EPS = 1e-3
NEAR, FAR = 0.1, 100.0
BACKGROUND = (0.1, 0.2, 0.3)


def _al(x):
    return (x + 255) // 256 * 256


# ---- scenes ------------------------------------------------------------------------------------------------------------
def pixel_triangles(tris, S, z=None):
    """[F,3,3] f32 faces in the rasteriser's coordinates from triangles given in PIXEL coordinates (x, y of the pixel grid
    whose integer points are the pixel centres: the inverse of to_pixel), turned counter-clockwise (front-facing); z per
    triangle (default 1)."""
    tris = np.asarray(tris, np.float64).reshape(-1, 3, 2).copy()
    for t in tris:
        if (t[1, 0] - t[0, 0]) * (t[2, 1] - t[0, 1]) - (t[2, 0] - t[0, 0]) * (t[1, 1] - t[0, 1]) < 0:
            t[[1, 2]] = t[[2, 1]]
    f = np.zeros((len(tris), 3, 3), np.float32)
    f[:, :, :2] = ((2.0 * tris + 1.0 - S) / S).astype(np.float32)
    f[:, :, 2] = 1.0 if z is None else np.asarray(z, np.float32)[:, None]
    return f


def corner_triangle(x, y, w, h):
    """(x, y), (x + w, y + 0.4), (x + 0.3, y + h): from x = k + 0.5 its first edge crosses floor(w + 0.5) columns, its
    last one none; from y = m + 0.5 its last edge crosses floor(h + 0.5) rows"""
    return [(x, y), (x + w, y + 0.4), (x + 0.3, y + h)]


def grid_views(n, B, S, seed=0, distance=2.732):
    """B views of grid_mesh(n) on the camera ring: faces [B,F,3,3] on the device"""
    from deep3dmap_amd import neural_renderer as nr, synthetic
    from deep3dmap_amd.neural_renderer.mesh_ops import gather_faces
    v, tri = synthetic.grid_mesh(n, seed=seed)
    eyes = torch.from_numpy(synthetic.camera_ring(32, distance=distance)[:B]).cuda()
    vt = torch.from_numpy(v).cuda()[None].expand(B, -1, -1).contiguous()
    ft = torch.from_numpy(tri).cuda()[None].expand(B, -1, -1).contiguous()
    return gather_faces(nr.look_at(vt, eyes, _perspective_angle=30), ft, True).contiguous()


def random_inputs(B, F, S, seed):
    """(textures, grad_rgb_map, grad_alpha_map) on the device"""
    gen = torch.Generator(device="cuda").manual_seed(4321 + seed)
    tex = torch.rand(B, F, 2, 2, 2, 3, device="cuda", generator=gen)
    g_rgb = torch.randn(B, S, S, 3, device="cuda", generator=gen)
    g_alpha = torch.randn(B, S, S, device="cuda", generator=gen)
    return tex, g_rgb, g_alpha


# ---- the reference: its own kernels compiled for the device where they were built, the oracle's C port otherwise ---------
def reference_k4(faces, tex, S, g_rgb, g_alpha):
    """(maps for K4 on the device: face_index_map / rgb_map / alpha_map, the reference's grad_faces of K4 alone on the
    device, which oracle ran)"""
    from oracle import nr_oracle as O
    from oracle import nr_ref_hip as RH
    if RH.available():
        ref = RH.forward(faces, tex, S, NEAR, FAR, EPS, BACKGROUND)
        gf_ref, _ = RH.backward(ref, g_rgb, g_alpha, None, True, True, False)
        return ref, gf_ref, "reference kernels"
    m = O.raster_forward(faces.cpu().numpy(), tex.cpu().numpy(), S, NEAR, FAR, EPS, BACKGROUND, True, True, False,
                         backend="port", bbox=True)
    gf_ref, _ = O.raster_backward(m, g_rgb.cpu().numpy(), g_alpha.cpu().numpy(), None, True, True, False, backend="port")
    ref = {k: torch.from_numpy(np.ascontiguousarray(m[k])).cuda() for k in ("face_index_map", "rgb_map", "alpha_map")}
    return ref, torch.from_numpy(gf_ref).cuda(), "C port"


def product_maps(faces, S, seed=0):
    """face_index_map / alpha_map of the product's own forward pass and an arbitrary rgb_map (K4 reads it as values, whatever
    they are): a scene for tests that need no reference"""
    from deep3dmap_amd.neural_renderer.rasterize import _raster_forward
    m, _ = _raster_forward(faces, None, S, NEAR, FAR, EPS, None, False, True, True, False)
    B = faces.shape[0]
    gen = torch.Generator(device="cuda").manual_seed(99 + seed)
    return {"face_index_map": m["face_index_map"].contiguous(),
            "alpha_map": (m["face_index_map"] >= 0).float().contiguous(),
            "rgb_map": torch.rand(B, S, S, 3, device="cuda", generator=gen)}


# ---- K4 through the C ABI ------------------------------------------------------------------------------------------------
def plan_bytes_for(B, F, S, cap):
    """a plan blob that holds exactly `cap` crossings (edge_plan_view's arithmetic)"""
    from deep3dmap_amd import _lib
    fixed = int(_lib.lib().d3m_edge_plan_min_bytes(B, F, S)) - 1024
    return fixed + 512 + (cap + 32) * 36


def run_k4(faces, maps, g_rgb, g_alpha, S, plan_bytes=None, form=None):
    """K4 alone with grad_faces stored (no vertex target), on a plan built by d3m_edge_plan in a blob of `plan_bytes`
    (None: the default size) and a workspace of this call's own.  Returns (grad_faces, plan blob, visibility blob,
    workspace) -- all as the launch left them."""
    import ctypes
    from deep3dmap_amd import _lib
    from deep3dmap_amd.neural_renderer import rasterize_ops as ops
    B, F = faces.shape[:2]
    L = _lib.lib()
    old = L.d3m_get_edge_plan_form()
    if form is not None:
        _lib.check(L.d3m_set_edge_plan_form(form), "d3m_set_edge_plan_form")
    try:
        fi = maps["face_index_map"]
        vis = ops.visibility(fi, F)
        n = plan_bytes if plan_bytes is not None else int(L.d3m_edge_plan_bytes(B, F, S))
        plan = torch.zeros(n, dtype=torch.uint8, device="cuda")
        ops.edge_plan(faces, fi, vis, S, out=plan)
        ws = torch.zeros(int(L.d3m_backward_pixel_map_workspace_bytes(B, F, S)), dtype=torch.uint8, device="cuda")
        gf = torch.zeros_like(faces)
        rc = L.d3m_backward_pixel_map(
            _lib.ptr(faces), _lib.ptr(fi), _lib.ptr(maps["rgb_map"]), _lib.ptr(maps["alpha_map"]), _lib.ptr(g_rgb),
            _lib.ptr(g_alpha), _lib.ptr(gf), B, F, int(S), float(EPS), 1, 1, _lib.ptr(ws), ws.numel(), None, _lib.ptr(vis),
            _lib.ptr(plan), plan.numel(), None, _lib.stream_ptr())
        _lib.check(rc, "backward_pixel_map")
        torch.cuda.synchronize()
    finally:
        L.d3m_set_edge_plan_form(old)
    return gf, plan, vis, ws


class PlanView:
    """The arrays of a plan blob (edge_plan_layout / edge_plan_view), of the visibility blob (visibility_view) and the
    lanes' overflow sums in K4's workspace (edge_layout), as numpy arrays -- read the way tools_dev/plan_stats.py reads them."""
    CURSORS, CURSOR_STRIDE, FIRST_CURSOR = 32, 64, 64      # EG_PLAN_CURSORS, EG_CURSOR_STRIDE, EG_ALLOC_CURSORS

    def __init__(self, plan, vis, ws, B, F, S):
        raw = plan.cpu().numpy()
        nl, nf = B * 2 * S, B * F
        self.B, self.F, self.S = B, F, S
        alloc_ints = self.FIRST_CURSOR + self.CURSORS * self.CURSOR_STRIDE
        o = 0
        self.line_cursor = raw[o:o + nl * 4].view(np.int32); o += _al(nl * 4)
        self.alloc = raw[o:o + alloc_ints * 4].view(np.int32); o += _al(alloc_ints * 4)
        o += 2 * _al(nl * 4)                                                                    # the extents
        self.lane_cross = raw[o:o + nf * 6 * 8].view(np.int32).reshape(-1, 2); o += _al(nf * 6 * 8)
        self.lane_block = raw[o:o + (nf // 42 + 2) * 4].view(np.int32); o += _al((nf // 42 + 2) * 4)
        self.line_slice = raw[o:o + nl * 8].view(np.int32).reshape(-1, 2); o += _al(nl * 8)
        cap = (len(raw) - o - 512) // 36
        cap = cap - 32 if cap > 64 else 0
        self.cap = cap = min(cap, 0x3FFFFF00)
        self.xrec = raw[o:o + cap * 16].view(np.uint32).reshape(-1, 4)
        o_res = _al(o + cap * 16)
        self.results = raw[o_res:o_res + cap * 16].view(np.float32).reshape(-1, 4)           # (outward.xy, inward.xy)
        o_pos = _al(o_res + cap * 16)
        self.xpos = raw[o_pos:o_pos + cap * 4].view(np.int32)
        cursors = self.alloc[self.FIRST_CURSOR::self.CURSOR_STRIDE][:self.CURSORS]
        self.one_pass = int(cursors.sum()) > 0
        self.cap_line = cap // nl if self.one_pass else 0
        self.total = int(cursors.sum()) if self.one_pass else int(self.alloc[0])
        self.spill, self.full = int(self.alloc[3]), int(self.alloc[4])
        self.records = (self.full == 0) if self.one_pass else (self.total <= cap)               # plan_records
        self.complete = self.records and (not self.one_pass or self.spill == 0)               # plan_complete
        v = vis.cpu().numpy()
        self.visible_list = v[_al(nf * 4):_al(nf * 4) + nf * 4].view(np.int32)
        o_count = 2 * _al(nf * 4) + _al((nf // 1024 + 2) * 4)
        self.n_visible = int(v[o_count:o_count + 4].view(np.int32)[0])
        w = ws.cpu().numpy()
        px = B * S * S
        o_partial = _al(px * 16) + _al(px * 8) + 2 * _al(nl * 4)
        self.lane_partial = w[o_partial:o_partial + nf * 6 * 8].view(np.float32).reshape(-1, 2)

    def lane_runs(self):
        """(first crossing index, end) of every lane of the listed faces [6 * n_visible], as k_edge_gather takes them"""
        n = self.n_visible * 6
        if not self.records:
            return np.zeros(n, np.int64), np.zeros(n, np.int64)
        lc = self.lane_cross[:n].astype(np.int64)
        first = self.lane_block[np.arange(n) // (42 * 6)].astype(np.int64) + lc[:, 0]
        return first, np.minimum(first + lc[:, 1], self.cap)

    def crossings(self, faces):
        """(crossing index, line) of every crossing of the listed faces' lanes, the line from the GEOMETRY: lane (face, edge,
        axis) crosses the lines d0_from .. d0_to of its axis (crossing_range, on to_pixel's f32 arithmetic), its k-th
        crossing is index first + k on line d0_from + k.  Checks the lanes' counts against lane_cross on the way."""
        f32 = np.float32
        S, n = self.S, self.n_visible * 6
        gi = self.visible_list[:self.n_visible].astype(np.int64)
        fc = faces.detach().cpu().numpy().reshape(-1, 3, 3)[gi]
        px = f32(0.5) * (fc[:, :, :2] * f32(S) + f32(S) - f32(1.0))            # [n_vis, vertex, (x, y)]
        lane = np.arange(n)
        edge, axis = (lane % 6) >> 1, lane % 2
        p00 = px[lane // 6, edge, axis]
        p10 = px[lane // 6, (edge + 1) % 3, axis]
        d0_from = np.maximum(np.ceil(np.minimum(p00, p10)), 0).astype(np.int64)
        d0_to = np.minimum(np.maximum(p00, p10), f32(S - 1)).astype(np.int64)      # (f2i: truncation towards zero)
        count = np.maximum(d0_to - d0_from + 1, 0)
        assert np.array_equal(count, self.lane_cross[:n, 1])
        first = self.lane_block[lane // (42 * 6)].astype(np.int64) + self.lane_cross[:n, 0]
        line0 = ((gi[lane // 6] // self.F) * 2 + axis) * S + d0_from
        k = np.arange(int(count.sum())) - np.repeat(np.cumsum(count) - count, count)
        return np.repeat(first, count) + k, np.repeat(line0, count) + k


def gather_in_numpy(pv, go_abs=1.0):
    """grad_faces [B*F,3,3] f32 as k_edge_gather documents it: per lane of a listed face lane_partial first when the plan is
    incomplete, then its crossings in ascending order, each as .x/.y (outward) then .z/.w (inward) of its results, found
    through xpos (none: nothing); per face the six lanes in order into the two vertices of their edge, times |go|."""
    f32 = np.float32
    n = pv.n_visible * 6
    g = np.zeros((n, 2), f32) if pv.complete else pv.lane_partial[:n].copy()
    first, end = pv.lane_runs()
    for j in range(int((end - first).max()) if n else 0):
        sel = np.nonzero(first + j < end)[0]
        at = pv.xpos[first[sel] + j].astype(np.int64)
        r = np.where((at >= 0)[:, None], pv.results[np.maximum(at, 0)], f32(0))
        g[sel, 0] += r[:, 0]; g[sel, 1] += r[:, 1]
        g[sel, 0] += r[:, 2]; g[sel, 1] += r[:, 3]
    g = g.reshape(-1, 6, 2)
    acc = np.zeros((pv.n_visible, 6), f32)
    for e in range(6):
        edge, axis = e >> 1, e & 1
        acc[:, edge * 2 + (1 - axis)] += g[:, e, 0] * f32(go_abs)
        acc[:, ((edge + 1) % 3) * 2 + (1 - axis)] += g[:, e, 1] * f32(go_abs)
    out = np.zeros((pv.B * pv.F, 3, 3), f32)
    out[pv.visible_list[:pv.n_visible], :, :2] = acc.reshape(-1, 3, 2)
    return out


def assert_bit_equal(got, want):
    got, want = np.ascontiguousarray(got, np.float32).ravel(), np.ascontiguousarray(want, np.float32).ravel()
    nan = np.isnan(want)
    assert np.array_equal(nan, np.isnan(got))
    a, b = got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]
    bad = np.nonzero(a != b)[0]
    assert bad.size == 0, (bad.size, got[~nan][bad[:4]], want[~nan][bad[:4]])
