"""The texel, light and depth adjoints through the C ABI on every route: d3m_backward_textures, d3m_backward_depth_map,
d3m_backward_depth_map_mesh and the lit node's fused d3m_backward_textures_lit, element by element against the float64 restatements
of tests/texel_depth_scenes.py with the per-element tolerance (D 2^-24 + 4 E32) bound -- the cases, their properties, the
references and the rejected wrong variants are proven on the CPU by tests/test_texel_depth_host.py.

Call protocol: every call goes through _lib.lib(); every output and workspace sits between guard words and is filled with the guard
pattern (a NaN) wherever the operator is documented to write, not add -- an element that is not written is a NaN in the result,
a word written outside is seen afterwards; where the operator ADDS (grad_faces, a vertex target, d3m_backward_textures) the entries
with a term start at zero and every other entry keeps the guard pattern, bit for bit.  Every call runs twice, the second time with
D3M_PRECLEARED where the entry point has clear ranges.  Which kernels ran is read with kernels_launched(); a LARGE face is also seen
as FLAG_LARGE in the flags afterwards.  Visibility blobs come from d3m_visibility and are compared with numpy before use.

An element whose bound is 0 must be +0.0.  Each case's achieved error / tolerance goes to texel_depth_adjoint_errors.json in the
records folder -- $D3M_RECORDS_DIR, by default dev_out/ in the repository root, which git ignores -- (a copy is committed as
profiles/texel_depth_adjoint_errors.json; docs/EXPERIMENTS.md has the largest per entry point)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import test_texel_depth_host as H
import texel_depth_scenes as X
from conftest import kernels_launched
from test_gpu_loss_reductions import Shifted
from test_gpu_param_reductions import GUARD_BITS, Guarded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESULTS = {}            # entry point -> {case: {output: err / tolerance, "E32 " + output: E32}}
FLAG_LARGE = 2


@pytest.fixture(scope="module", autouse=True)
def _write_results():
    yield
    out = {k: dict(worst=max([r for c in v.values() for o, r in c.items() if not o.startswith("E32")] + [0.0]), cases=v)
           for k, v in sorted(RESULTS.items())}
    records = os.environ.get("D3M_RECORDS_DIR") or os.path.join(ROOT, "dev_out")
    os.makedirs(records, exist_ok=True)
    with open(os.path.join(records, "texel_depth_adjoint_errors.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    for k, v in out.items():
        print(f"TEXELDEPTH-WORST {k} err/tolerance={v['worst']:.3e}")


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


class Check:
    """collects what a case misses, so that one failure does not hide the next; asserts at the end"""

    def __init__(self, entry, c):
        self.entry, self.c, self.failures = entry, c, []
        self.ratios = RESULTS.setdefault(entry, {}).setdefault(X.case_id(c), {})

    def bounded(self, what, got, ref, untouched=None):
        """|got - ref| <= tol per element; an element without a bound is +0.0; `untouched` (a mask) keeps the guard pattern"""
        want, tol, e32 = ref
        got = np.asarray(got, np.float32).reshape(want.shape)
        live = np.ones(want.shape, bool) if untouched is None else ~np.broadcast_to(untouched, want.shape)
        if untouched is not None and not (_bits(got)[~live] == GUARD_BITS).all():
            self.failures.append((what, "an entry without a term was written", int((_bits(got)[~live] != GUARD_BITS).sum())))
        g, w, t = got[live].astype(np.float64), want[live], tol[live]
        err = np.abs(g - w)
        if not (_bits(got[live])[t == 0] == 0).all():
            self.failures.append((what, "an element without a bound is not +0.0", int((_bits(got[live])[t == 0] != 0).sum())))
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(t > 0, err / np.where(t > 0, t, 1), 0.0)
        worst = float(np.nanmax(ratio)) if ratio.size else 0.0
        print(f"TEXELDEPTH {self.entry} {X.case_id(self.c)} {what} E32={e32:.3e} err/tolerance={worst:.3e}")
        key = what.split(",")[0]
        self.ratios[key] = max(self.ratios.get(key, 0.0), worst)
        self.ratios["E32 " + key] = e32
        if not bool((err <= t).all()):                # (a NaN fails)
            self.failures.append((what, "largest err / tolerance", worst, "at", int(np.nanargmax(ratio)), "NaN" * bool(np.isnan(err).any())))

    def same_bits(self, what, a, b):
        if not np.array_equal(_bits(a), _bits(b)):
            self.failures.append((what, "two runs differ in", int((_bits(a) != _bits(b)).sum()), "elements"))

    def kernels(self, names, required, forbidden=()):
        if not set(required) <= names or set(forbidden) & names:
            self.failures.append(("kernels", sorted(names), "required", sorted(required), "forbidden", sorted(forbidden)))

    def done(self):
        assert not self.failures, "\n".join(" ".join(map(str, f)) for f in self.failures)


def _dev(x, dtype=torch.float32):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dtype).cuda().contiguous()


def _p(x):
    from deep3dmap_amd import _lib
    return _lib.ptr(x.inner if isinstance(x, Guarded) else x)


def _call(name, *args):
    """the entry point on the current stream; every Guarded among the arguments is checked afterwards"""
    from deep3dmap_amd import _lib
    conv = [_p(a) if isinstance(a, (Guarded, torch.Tensor)) or a is None else a for a in args]
    rc = getattr(_lib.lib(), name)(*conv, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, (name, rc)
    for a in args:
        assert not isinstance(a, Guarded) or a.intact(), (name, "guard words were written")


def _words(nbytes):
    return Guarded(((int(nbytes) + 3) // 4,))


def _visible(sc):
    vis = np.zeros((sc["B"], sc["Fp"]), bool)
    for k in sc["box"]:
        vis[k // sc["Fp"], k % sc["Fp"]] = True
    return vis


class Scene:
    """a scene's maps on the device, and its visibility blob: built by d3m_visibility, compared with numpy"""

    def __init__(self, name, lanes, B):
        self.sc = sc = X.scene(name, lanes, B)
        self.faces = _dev(sc["faces"])
        self.fim, self.wmap, self.dmap, self.finv = _dev(sc["fim"], torch.int32), _dev(sc["wmap"]), _dev(sc["dmap"]), _dev(sc["finv"])
        self.vis = _visible(sc)

    def blob(self, deterministic=False):
        """a fresh blob: the flags and the ascending list as numpy predicts them.  (Beyond one chunk of 1024 faces the list is
        ascending in the deterministic mode only -- include/d3m_raster.h -- so such a blob is built in that mode.)"""
        from deep3dmap_amd import _lib
        sc = self.sc
        nf = sc["B"] * sc["Fp"]
        blob = _words(_lib.lib().d3m_visibility_bytes(sc["B"], sc["Fp"]))
        with _lib.deterministic(deterministic or nf > 1024):
            _call("d3m_visibility", self.fim, blob, blob.n * 4, sc["B"], sc["Fp"], sc["S"])
        flags, lst, count = self.read_blob(blob)
        want = np.flatnonzero(self.vis.reshape(-1))
        assert np.array_equal(flags, self.vis.reshape(-1).astype(np.int32)) and count == want.size and np.array_equal(lst[:count], want)
        return blob

    def read_blob(self, blob):
        nf = self.sc["B"] * self.sc["Fp"]
        al = (nf * 4 + 255) // 256 * 256                # csrc/d3m_edge_grad.h visibility_view: flags | list | blocks | count
        words = blob.inner.view(torch.int32).cpu().numpy()
        at = (2 * al + ((nf // 1024 + 2) * 4 + 255) // 256 * 256) // 4
        return words[:nf].copy(), words[al // 4:al // 4 + nf].copy(), int(words[at])


def _vertex_target(sc, gv, tri, tri_batch):
    from deep3dmap_amd import _lib
    vt = _lib.D3MVertexTarget()
    vt.grad_vertices, vt.tri = gv.inner.data_ptr(), None if tri is None else tri.data_ptr()
    vt.num_vertices, vt.num_tri, vt.tri_batch, vt.fill_back = sc["V"], sc["F"], tri_batch, int(sc["fill_back"])
    return vt


def _prefill(g, live):
    """zeros where the operator adds its terms, the guard pattern elsewhere"""
    g.inner[torch.from_numpy(np.ascontiguousarray(np.broadcast_to(live, tuple(g.inner.shape)))).cuda()] = 0.0
    return g


def _touched_vertices(sc, tri=None):
    B, F, V = sc["B"], sc["F"], sc["V"]
    tri = np.broadcast_to(np.asarray(sc["tri"] if tri is None else tri).reshape(-1, F, 3), (B, F, 3))
    live = np.zeros((B, V, 1), bool)
    for k in sc["box"]:
        live[k // sc["Fp"], tri[k // sc["Fp"], (k % sc["Fp"]) % F]] = True
    return live


# ==== d3m_backward_textures_lit ========================================================================================================
def _lit_run(c, dv, inp, dev, blob, precleared):
    """one call: dict(gtex, glight, depth) as numpy"""
    from deep3dmap_amd import _lib
    L, sc = _lib.lib(), dv.sc
    B, F, Fp, S, ts3 = sc["B"], sc["F"], sc["Fp"], sc["S"], c.ts ** 3
    tb, lb = X.batch_of(c.tb, B), X.batch_of(c.lb, B)
    gtex = (Shifted if c.off else Guarded)((tb, F, ts3, 3))
    assert gtex.inner.data_ptr() % 16 == c.off
    glight = Guarded((lb, Fp, 3)) if c.glight else None
    ws = _words(L.d3m_backward_textures_lit_workspace_bytes(B, F, 1, c.ts))
    gfaces = gverts = vt = None
    if c.depth == "faces":
        gfaces = _prefill(Guarded((B, Fp, 3, 3)), dv.vis[:, :, None, None])
    if c.depth == "vertex":
        gverts = _prefill(Guarded((B, sc["V"], 3)), _touched_vertices(sc))
        vt = _vertex_target(sc, gverts, dev["tri"], 1)
    fit, keep = None, []
    if c.form is not None:
        fit = _lib.D3MFitTargets()
        scratch = torch.zeros(int(L.d3m_render_fit_scratch_floats(B, S)) + 8, device="cuda")
        scratch[2] = X.DEN
        go = torch.tensor([X.GO], device="cuda")
        keep += [scratch, go]
        fit.scratch, fit.grad_loss = scratch.data_ptr(), go.data_ptr()
        if c.form == "records":                     # float4 records: (alpha's, rgb's): the operator reads yzw
            den = torch.tensor([X.DEN], device="cuda")
            scratch[2] = float("nan")               # (mask_sum is given: the totals are not read)
            keep += [den]
            fit.mask_sum, fit.edge_grad = den.data_ptr(), dev["records"].data_ptr()
    if precleared:
        ptrs, sizes = (ctypes.c_void_p * 4)(), (ctypes.c_size_t * 4)()
        n = L.d3m_backward_textures_lit_clear_ranges(_p(gtex), tb, _p(glight), lb, B, F, 1, c.ts, _p(ws), int(blob is not None), ptrs, sizes)
        assert 1 <= n <= 4
        _lib.zero_raw([(ptrs[i], sizes[i]) for i in range(n)])
    _call("d3m_backward_textures_lit", dv.faces, dev["tex"], tb, dev["light"], lb, dv.fim, dv.wmap, dv.dmap,
          None if c.form == "records" else dev["g_rgb"], gtex, glight, dev["g_depth"] if c.depth != "none" else None, gfaces, B, F, 1, S,
          c.ts, X.EPS, ws, ws.n * 4, None if vt is None else ctypes.byref(vt), blob, None if fit is None else ctypes.byref(fit),
          _lib.PRECLEARED if precleared else 0)
    depth = gfaces if gfaces is not None else gverts
    return dict(gtex=gtex.inner.cpu().numpy(), glight=None if glight is None else glight.inner.cpu().numpy(),
                depth=None if depth is None else depth.inner.cpu().numpy())


@pytest.mark.parametrize("c", X.lit_cases(), ids=X.case_id)
def test_lit_adjoint_at_route(c):
    from deep3dmap_amd import _lib
    chk, ref, dv, inp = Check("d3m_backward_textures_lit", c), H.lit_reference(c), Scene(c.scene, c.lanes, c.B), H.lit_inputs(c)
    sc = dv.sc
    assert sc["fill_back"]
    dev = dict(tex=_dev(inp["tex"]), light=_dev(inp["light"]), g_rgb=_dev(inp["g_rgb"]), g_depth=_dev(inp["g_depth"]),
               tri=_dev(sc["tri"], torch.int32))
    if c.form == "records":
        rec = np.concatenate([X._rng(7, c.B).uniform(-1, 1, inp["g_rgb"].shape[:3] + (1,)), inp["g_rgb"]], -1)
        dev["records"] = _dev(rec)
    gathered = c.ts == 2 or (c.vis == "list" and c.ts in (3, 4))
    large = X.large_faces(sc) if gathered and not c.det else []
    runs = []
    with _lib.deterministic(bool(c.det)):
        for precleared in (False, True):
            blob = dv.blob(bool(c.det)) if c.vis == "list" else None
            with kernels_launched() as k:
                runs.append(_lit_run(c, dv, inp, dev, blob, precleared))
            need = {"k_backward_textures_lit_faces", "k_lit_large_faces"} if gathered else {"k_backward_textures_lit_pixels"}
            deny = {"k_backward_textures_lit_pixels"} if gathered else {"k_backward_textures_lit_faces", "k_lit_large_faces"}
            if not gathered and c.depth != "none":
                need |= {"k_backward_depth_map"} | ({"k_backward_depth_faces", "k_mark_visible"} if c.depth == "faces" else set())
            if c.ts == 2 and c.vis == "flags":
                need |= {"k_mark_visible"}
            (need if c.tb == 1 else deny).add("k_sum_over_views")
            chk.kernels(k.names, need, deny)
            if blob is not None and gathered:       # the faces the gathered pass left to the per-pixel pass, and no others
                flags = dv.read_blob(blob)[0]
                want = dv.vis.reshape(-1).astype(np.int32)
                want[large] = FLAG_LARGE
                if not np.array_equal(flags, want):
                    chk.failures.append(("flags after the call", int((flags != want).sum()), "differ"))
    live_depth = None if c.depth == "none" else (~dv.vis[:, :, None, None] if c.depth == "faces" else ~_touched_vertices(sc))
    for i, r in enumerate(runs):
        tag = "" if i == 0 else ", precleared"
        chk.bounded("grad_textures" + tag, r["gtex"], ref["gtex"])
        if c.glight:
            chk.bounded("grad_light" + tag, r["glight"], ref["glight"])
        if c.depth != "none":
            chk.bounded("depth" + tag, r["depth"], ref["depth"], untouched=live_depth)
    # fixed-order routes: the gathered ts = 2 texels (registers, a DPP tree, the views in ascending order) without a LARGE face
    if c.ts == 2 and not large:
        chk.same_bits("grad_textures", runs[0]["gtex"], runs[1]["gtex"])
    if c.det:                                       # one add per light row and per vertex: the two runs agree bit for bit
        chk.same_bits("grad_light", runs[0]["glight"], runs[1]["glight"])
        chk.same_bits("depth", runs[0]["depth"], runs[1]["depth"])
    chk.done()


# ==== d3m_backward_textures ===============================================================================================================
@pytest.mark.parametrize("c", X.plain_cases(), ids=X.case_id)
def test_backward_textures_at_route(c):
    from deep3dmap_amd import _lib
    chk, ref, dv = Check("d3m_backward_textures", c), H.plain_reference(c), Scene(c.scene, c.lanes, c.B)
    sc, m, inp = dv.sc, X.sampling_maps(c.scene, c.lanes, c.B, c.ts), X.inputs(c.scene, c.lanes, c.B, c.ts, 1, 1)
    sw, si, g = _dev(m["sw"]), _dev(m["si"], torch.int32), _dev(inp["g_rgb"])
    B, Fp, S = sc["B"], sc["Fp"], sc["S"]
    live = X.plain_texels(m, inp["g_rgb"], "f64")[1] > 0
    runs = []
    for _ in range(2):
        out = _prefill(Guarded((B, Fp, c.ts ** 3, 3)), live)
        ws = _words(_lib.lib().d3m_backward_faces_workspace_bytes(B, Fp)) if c.ws else None
        with kernels_launched() as k:
            _call("d3m_backward_textures", dv.faces if c.ws else None, dv.fim, sw, si, g, out, B, Fp, S, c.ts, ws, ws.n * 4 if c.ws else 0)
        gathered = {"k_mark_visible", "k_backward_textures_faces"}
        chk.kernels(k.names, {"k_backward_textures"} | (gathered if c.ws and c.ts == 2 else set()), () if c.ws and c.ts == 2 else gathered)
        if c.ws and c.ts == 2:
            want = dv.vis.reshape(-1).astype(np.int32)
            want[X.large_faces(sc)] = FLAG_LARGE
            if not np.array_equal(ws.inner.view(torch.int32).cpu().numpy()[:B * Fp], want):
                chk.failures.append(("flags after the call differ",))
        runs.append(out.inner.cpu().numpy())
        chk.bounded("grad_textures", runs[-1], ref, untouched=~live)
    if c.ws and c.ts == 2 and not X.large_faces(sc):
        chk.same_bits("grad_textures", *runs)
    chk.done()


# ==== d3m_backward_depth_map ==============================================================================================================
@pytest.mark.parametrize("c", X.depth_cases(), ids=X.case_id)
def test_backward_depth_map_at_route(c):
    from deep3dmap_amd import _lib
    chk, ref, dv = Check("d3m_backward_depth_map", c), H.depth_reference(c), Scene(c.scene, c.lanes, c.B)
    sc, inp = dv.sc, X.inputs(c.scene, c.lanes, c.B, 2, 1, 1)
    B, Fp, S = sc["B"], sc["Fp"], sc["S"]
    g = _dev(inp["g_depth"])
    live = dv.vis[:, :, None, None]
    runs = []
    with _lib.deterministic(bool(c.det)):
        for _ in range(2):
            out = _prefill(Guarded((B, Fp, 3, 3)), live)
            ws = _words(_lib.lib().d3m_backward_faces_workspace_bytes(B, Fp)) if c.ws else None
            with kernels_launched() as k:
                _call("d3m_backward_depth_map", dv.faces, dv.dmap, dv.fim, dv.finv if c.finv else None, dv.wmap, g, out, B, Fp, S, ws,
                      ws.n * 4 if c.ws else 0)
            gathered = {"k_mark_visible", "k_backward_depth_faces"}
            chk.kernels(k.names, {"k_backward_depth_map"} | (gathered if c.ws else set()), () if c.ws else gathered)
            if c.ws:
                want = dv.vis.reshape(-1).astype(np.int32)
                want[[] if c.det else X.large_faces(sc)] = FLAG_LARGE
                if not np.array_equal(ws.inner.view(torch.int32).cpu().numpy()[:B * Fp], want):
                    chk.failures.append(("flags after the call differ",))
            runs.append(out.inner.cpu().numpy())
            chk.bounded("grad_faces", runs[-1], ref, untouched=~live)
    if c.ws and (c.det or not X.large_faces(sc)):   # the gathered pass alone: a face's lanes own its sums
        chk.same_bits("grad_faces", *runs)
    chk.done()


# ==== d3m_backward_depth_map_mesh =========================================================================================================
@pytest.mark.parametrize("c", X.mesh_cases(), ids=X.case_id)
def test_backward_depth_map_mesh_at_route(c):
    from deep3dmap_amd import _lib
    chk, ref, dv = Check("d3m_backward_depth_map_mesh", c), H.mesh_reference(c), Scene(c.scene, c.lanes, c.B)
    sc, inp = dv.sc, X.inputs(c.scene, c.lanes, c.B, 2, 1, 1)
    B, Fp, S = sc["B"], sc["Fp"], sc["S"]
    g = _dev(inp["g_depth"])
    tri_np = None if c.tb else X.tri_views(sc)[1]
    tri = None if c.implicit else _dev(sc["tri"] if c.tb else tri_np, torch.int32)
    live = _touched_vertices(sc, tri_np)
    for precleared in (False, True):
        blob = dv.blob()
        out = _prefill(Guarded((B, sc["V"], 3)), live)
        vt = _vertex_target(sc, out, tri, -sc["grid_w"] if c.implicit else (1 if c.tb else B))
        counter = _words(256)
        if precleared:
            _lib.zero_raw([(counter.inner.data_ptr(), 256)])
        with kernels_launched() as k:
            _call("d3m_backward_depth_map_mesh", dv.faces, dv.dmap, dv.fim, dv.wmap, g, B, Fp, S, ctypes.byref(vt), blob, counter,
                  (_lib.PRECLEARED if precleared else 0) | (_lib.GRAD_OF_OUTPUT_IMAGE if c.flip else 0))
        chk.kernels(k.names, {"k_backward_depth_faces", "k_backward_depth_map"}, {"k_mark_visible"})
        large = X.large_faces(sc)
        want = dv.vis.reshape(-1).astype(np.int32)
        want[large] = FLAG_LARGE
        if not np.array_equal(dv.read_blob(blob)[0], want) or int(counter.inner.view(torch.int32)[0]) != len(large):
            chk.failures.append(("flags or the LARGE counter after the call differ",))
        chk.bounded("grad_vertices" + (", precleared" if precleared else ""), out.inner.cpu().numpy(), ref, untouched=~live)
    chk.done()
