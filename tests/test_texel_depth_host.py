"""CPU side of the texel / light / depth adjoint tests (tests/texel_depth_scenes.py, tests/test_gpu_texel_depth.py): it proves what the
GPU file relies on.

  * the float32 restatements reproduce the committed reference vectors of K5 and K6 (tests/golden/kern_golden.npz, the vectors of
    test_backward_ops_match_reference_vectors), the oracle's raster_backward on every scene within the tolerance the GPU test uses,
    and torch autograd of the oracle's lit sequence (fill_back's texel transposition, the light's product) for grad_textures and
    grad_light;
  * the scenes have the properties the routes need, read from the oracle's face_index_map: boxes at and just above
    FM_MAX_BBOX_AREA, boxes of one scan chunk and one more pixel for 8 and 64 lanes, the 48-pixels-per-triangle launch rule on both
    sides, a wave's run with more than four LARGE faces, a workgroup's run with more than its table holds, faces in exactly one
    view of the mask's second word, a face in no view, the ts = 1 reach at the array's end;
  * no sample position of a ts >= 3 case lies within 2^-18 (ts - 1) of an interior integer, so the float32 and the float64
    restatement take the same integer parts;
  * every named wrong variant is rejected by the comparison the GPU test makes, and the float32 restatement is not;
  * E32 of every case (test_print_e32_of_every_case, `pytest -s`)."""
import functools

import numpy as np
import pytest
import torch

import texel_depth_scenes as X
from conftest import golden_case
from test_oracle import CASES as GOLDEN_CASES


# ---- references of the cases: (float64 value, per-element tolerance, E32) --------------------------------------------------------
def lit_inputs(c):
    return X.inputs(c.scene, c.lanes, c.B, c.ts, X.batch_of(c.tb, c.B), X.batch_of(c.lb, c.B))


@functools.lru_cache(maxsize=None)
def lit_reference(c):
    """dict(gtex, glight, depth): depth is grad_faces [B,Fp,3,3] or grad_vertices [B,V,3] (None without the rider)"""
    sc, inp = X.scene(c.scene, c.lanes, c.B), lit_inputs(c)
    out = X.lit_reference(sc, inp, c.ts, c.form)
    out["depth"] = None if c.depth == "none" else X.depth_reference(sc, inp, c.form, vertices=c.depth == "vertex")
    return out


@functools.lru_cache(maxsize=None)
def plain_reference(c):
    m, inp = X.sampling_maps(c.scene, c.lanes, c.B, c.ts), X.inputs(c.scene, c.lanes, c.B, c.ts, 1, 1)
    f64, n = X.plain_texels(m, inp["g_rgb"], "f64")
    f32, ab = X.plain_texels(m, inp["g_rgb"], "f32")[0], X.plain_texels(m, inp["g_rgb"], "abs")[0]
    e = X.e32_of(f32, f64, ab.a)
    return np.asarray(f64), X.tolerance(n + X.TREE + 1, e, ab.a), e          # (one product per term)


@functools.lru_cache(maxsize=None)
def depth_reference(c):
    return X.depth_reference(X.scene(c.scene, c.lanes, c.B), X.inputs(c.scene, c.lanes, c.B, 2, 1, 1), finv_map=bool(c.finv))


@functools.lru_cache(maxsize=None)
def mesh_reference(c):
    sc = X.scene(c.scene, c.lanes, c.B)
    tri = None if c.tb else X.tri_views(sc)[1]
    return X.depth_reference(sc, X.inputs(c.scene, c.lanes, c.B, 2, 1, 1), flip=bool(c.flip), vertices=True, tri=tri)


# ---- 1. the restatements against the reference's vectors, the oracle and autograd -------------------------------------------------
def _close(got, ref):
    """tests/test_oracle.py's comparison of the oracle with the same vectors"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    ok = np.isfinite(ref)
    return np.array_equal(np.isfinite(got), ok) and np.abs(got[ok] - ref[ok]).max() <= 2e-6 * max(np.abs(ref[ok]).max(), 1e-30)


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_float32_restatements_reproduce_the_reference_vectors(golden, name):
    c = golden_case(golden, name)
    fim, faces = c["face_index_map"], c["faces"]
    B, F = faces.shape[:2]
    m = dict(fim=fim, sw=c["sampling_weight_map"], si=c["sampling_index_map"], ts=c["textures"].shape[2], F=F)
    gt = X.plain_texels(m, c["grad_rgb_map"].astype(np.float64), "f32")[0]
    assert _close(gt.reshape(c["grad_textures"].shape), c["grad_textures"])
    b, y, x = np.nonzero(fim >= 0)
    sc = dict(S=int(c["image_size"]), B=B, Fp=F, faces=faces.astype(np.float64), wmap=c["weight_map"], dmap=c["depth_map"],
              finv=c["face_inv_map"], px=(b, y, x, fim[b, y, x].astype(np.int64)))
    for finv_map in (True, False):
        gf = X.depth_adjoint(sc, c["grad_depth_map"].astype(np.float64), "f32", finv_map=finv_map)[0]
        assert _close(gf, c["grad_faces_depth"]), finv_map


ORACLE_SCENES = [("counts", 8, 1), ("holes", 64, 1), ("one_of_eight", 8, 1), ("limit", 64, 1), ("views", 64, 3), ("views", 8, 33),
                 ("slivers", 64, 1), ("hub", 8, 1), ("grid", 8, 1), ("views_front", 8, 3)]


@pytest.mark.parametrize("name,lanes,B", ORACLE_SCENES)
def test_restatements_are_the_oracle_backward(name, lanes, B):
    """the oracle (float32, per pixel in ascending order) lies within the GPU test's own tolerance of the float64 restatement: the
    virtual lit array's gradient (acc), K5 from the sampling maps, K6 with the forward's face_inv_map"""
    from oracle import nr_oracle as O
    sc = X.scene(name, lanes, B)
    for ts in (1, 2, 3, 4):
        inp = X.inputs(name, lanes, B, ts, 1, 1)
        tex = np.ones((B, sc["Fp"], ts, ts, ts, 3), np.float32)
        m = O.raster_forward(sc["faces"].astype(np.float32), tex, sc["S"], X.NEAR, X.FAR, X.EPS, (0, 0, 0), True, True, True)
        assert np.array_equal(m["face_index_map"], sc["fim"]) and np.array_equal(m["weight_map"], sc["wmap"])
        _, gt = O.raster_backward(m, inp["g_rgb"], None, None, True, False, False)
        r = {ar: X.lit_adjoint(sc, inp, ts, ar) for ar in ("f64", "f32", "abs")}
        e = X.e32_of(r["f32"]["acc"], r["f64"]["acc"], r["abs"]["acc"].a)
        n = sc["px"][0].size                                                      # (no element has more terms than there are pixels)
        ref = (r["f64"]["acc"], X.tolerance(X.D_k5(n), e, r["abs"]["acc"].a), e)
        assert not X.outside(gt.reshape(ref[0].shape), ref), (ts, "acc")
        # K5 from the oracle's sampling maps is the same sum
        plain = X.plain_texels(dict(fim=sc["fim"], sw=m["sampling_weight_map"], si=m["sampling_index_map"], ts=ts, F=sc["Fp"]), inp["g_rgb"], "f64")[0]
        assert np.abs(plain - r["f64"]["acc"]).max() <= 8 * X.U * max(r["abs"]["acc"].a.max(), 1e-30), ts
    inp = X.inputs(name, lanes, B, 2, 1, 1)
    gf, _ = O.raster_backward(m, None, None, inp["g_depth"], False, False, True)
    for finv_map in (True, False):
        assert not X.outside(gf, X.depth_reference(sc, inp, finv_map=finv_map)), finv_map


@pytest.mark.parametrize("ts,tb,lb", [(1, 1, 1), (2, 1, 0), (2, 0, 1), (3, 0, 0), (4, 1, 1)])
def test_texels_and_light_are_autograd_of_the_lit_sequence(ts, tb, lb):
    """NR/renderer.py:156 (cat(textures, textures.permute(0,1,4,3,2,5))) and NR/lighting.py:55 (x light per face), as oracle.nr_oracle
    restates them: the gradient of <lit array, acc> wrt the textures and the light is grad_textures and grad_light"""
    from oracle import nr_oracle as O
    B = 3
    sc = X.scene("views", 64, B)
    inp = X.inputs("views", 64, B, ts, X.batch_of(tb, B), X.batch_of(lb, B))
    r = X.lit_adjoint(sc, inp, ts, "f64")
    F, Fp = sc["F"], sc["Fp"]
    tex = torch.from_numpy(inp["tex"].reshape(-1, F, ts, ts, ts, 3)).requires_grad_(True)
    light = torch.from_numpy(inp["light"]).requires_grad_(True)
    _, both = O.Renderer(fill_back=True)._fill_back(torch.zeros(B, F, 3, dtype=torch.int64), tex.expand(B, F, ts, ts, ts, 3))
    lit = both * light.expand(B, Fp, 3)[:, :, None, None, None, :]
    (lit * torch.from_numpy(r["acc"].reshape(B, Fp, ts, ts, ts, 3))).sum().backward()
    assert np.allclose(tex.grad.numpy().reshape(r["gtex"].shape), r["gtex"], rtol=1e-12, atol=1e-15)
    assert np.allclose(light.grad.numpy(), r["glight"], rtol=1e-12, atol=1e-15)
    assert np.abs(r["gtex"]).max() > 0.1 and np.abs(r["glight"]).max() > 0.1


# ---- 2. the scenes' properties ----------------------------------------------------------------------------------------------------------
def _areas(sc):
    return {k: (x1 - x0 + 1) * (y1 - y0 + 1) for k, (x0, x1, y0, y1) in sc["box"].items()}


def _visible(sc):
    vis = np.zeros((sc["B"], sc["Fp"]), bool)
    for k in sc["box"]:
        vis[k // sc["Fp"], k % sc["Fp"]] = True
    return vis


def test_every_case_scene_follows_the_launch_rule_and_keeps_its_indices_inside():
    cases = X.lit_cases() + X.plain_cases() + X.depth_cases() + X.mesh_cases()
    seen = set()
    for c in cases:
        sc = X.scene(c.scene, c.lanes, c.B)
        assert (sc["S"] * sc["S"] > 48 * sc["F"]) == (c.lanes == 64), c               # a wave per face above 48 pixels per triangle
        assert sc["S"] <= 128 and sc["F"] <= 400, c
        seen.add((c.scene, c.lanes))
        vis = _visible(sc)
        if sc["fill_back"]:                         # a face's two copies never own pixels of the same view: the gathered store is the sum
            assert not (vis[:, :sc["F"]] & vis[:, sc["F"]:]).any(), c
    assert {(s, lanes) for s in ("counts", "holes", "limit", "slivers", "views", "hub") for lanes in (8, 64)} <= seen


@pytest.mark.parametrize("lanes", [8, 64])
def test_boxes_at_the_limit_and_at_the_chunk_edges(lanes):
    sc = X.scene("limit", lanes)
    areas = sorted(_areas(sc).values())
    assert areas[0] == X.MAX_BOX and X.MAX_BOX < areas[1] <= X.MAX_BOX + 64 and len(X.large_faces(sc)) == 1
    sc = X.scene("counts", lanes)
    assert {X.CHUNK[lanes], X.CHUNK[lanes] + 1} <= set(_areas(sc).values())
    assert any(k % sc["Fp"] >= sc["F"] for k in sc["box"])                         # back copies own pixels


@pytest.mark.parametrize("lanes", [8, 64])
def test_slivers_crowd_a_wave_and_overflow_a_workgroup_table(lanes):
    sc = X.scene("slivers", lanes)
    large = set(X.large_faces(sc))
    assert len(large) == 80 and len(sc["box"]) == 80
    fim = sc["fim"].reshape(-1)
    chunk, blocks = X.px_runs(fim.size)
    per_wave = [len(set(fim[i:i + 64][fim[i:i + 64] >= 0]) & large) for i in range(0, fim.size, 64)]
    per_group = [len(set(fim[i:i + chunk][fim[i:i + chunk] >= 0]) & large) for i in range(0, fim.size, chunk)]
    assert max(per_wave) > 4 and min(p for p in per_wave if p) <= 4                 # the leftover branch and the merged one
    assert max(per_group) > 64 + 8 and chunk == 256 and blocks == 64               # more faces than the 64-slot table's probes reach


@pytest.mark.parametrize("B", X.VIEW_COUNTS)
def test_view_scene_covers_the_mask_words(B):
    for lanes in (8, 64):
        sc = X.scene("views", lanes, B)
        vis, F = _visible(sc), sc["F"]
        both = vis[:, :F] | vis[:, F:]
        assert not both[:, 5].any()                                                 # a face visible in no view
        assert both[:, 4].sum() == 1 and both[B - 1, 4] and vis[B - 1, F + 4]       # one view, through its back copy
        assert [b for b in range(B) if both[b, 3]] == [b for b in (5, 32) if b < B]
        if B > 32:                                                                  # exactly one view of the second mask word
            assert both[32:64, 3].sum() == 1 and both[32].sum() >= 3
        assert vis[:, F + 1].any() and not vis[:, 1].any()
    sc = X.scene("views", 64, B)                   # unpadded: the ts = 1 reach of face F + 4 passes the end of the last view
    assert sc["Fp"] == 12 and (sc["fim"][B - 1] == 10).any()


def test_hub_vertex_is_shared_by_every_real_face():
    for lanes in (8, 64):
        sc = X.scene("hub", lanes)
        assert (sc["tri"][:sc["n_real"]] == 0).any(1).all() and len(sc["box"]) == sc["n_real"]


# ---- 3. the stencil distance ------------------------------------------------------------------------------------------------------------
def _stencil_count(sc, ts):
    t = X.sample_positions(sc, ts, "f64")
    near = np.abs(t - np.round(t)) < X.STENCIL * (ts - 1)
    interior = (np.round(t) >= 1) & (np.round(t) <= ts - 2)
    t32 = X.sample_positions(sc, ts, "f32")
    return int((near & interior).sum()), bool(np.array_equal(np.trunc(t), np.trunc(t32.astype(np.float64))))


def test_no_sample_position_sits_on_an_interior_integer():
    cases = {(c.scene, c.lanes, c.B, c.ts) for c in X.lit_cases() + X.plain_cases() if c.ts >= 3}
    assert len(cases) > 10
    for name, lanes, B, ts in sorted(cases):
        count, same = _stencil_count(X.scene(name, lanes, B), ts)
        assert count == 0 and same, (name, lanes, B, ts, count)
    for c in X.plain_cases():                       # the sampling maps' indices stay inside the array where they are not guarded
        m = X.sampling_maps(c.scene, c.lanes, c.B, c.ts)
        assert m["si"].min() >= 0 and (c.ts == 1 or m["si"].max() < c.ts ** 3)


# ---- 4. every wrong variant is rejected by the comparison the GPU test makes ------------------------------------------------------------
def _case(cases, **kw):
    return next(c for c in cases if all(getattr(c, k) == v for k, v in kw.items()))


def _lit_variant(c, variant):
    return X.lit_adjoint(X.scene(c.scene, c.lanes, c.B), lit_inputs(c), c.ts, "f64", variant, c.form)


def _depth_variant(c, variant, **kw):
    sc, inp = X.scene(c.scene, c.lanes, c.B), X.inputs(c.scene, c.lanes, c.B, getattr(c, "ts", 2), 1, 1)
    s = X.scales(lit_inputs(c), c.form, "f64", variant)[1] if hasattr(c, "form") else None
    gf, n = X.depth_adjoint(sc, inp["g_depth"], "f64", variant, s_depth=s, **kw)
    return gf, X.to_vertices(sc, gf, n, variant)[0]


LIT = X.lit_cases()
REJECTED_ON = {         # variant -> [(case, output)]
    "chunk_last_dropped": [(_case(LIT, scene="counts", lanes=8, ts=2, vis="list", depth="faces"), o) for o in ("gtex", "glight", "depth")]
                          + [(_case(LIT, scene="counts", lanes=64, ts=3), "gtex")],
    "pixel_twice": [(_case(LIT, scene="counts", lanes=64, ts=2, depth="faces"), o) for o in ("gtex", "glight", "depth")]
                   + [(_case(LIT, scene="limit", lanes=8, ts=2), "gtex")],
    "back_untransposed": [(_case(LIT, scene="counts", lanes=8, ts=2, vis="list", depth="none"), "gtex"), (_case(LIT, scene="holes", lanes=64, ts=4), "gtex")],
    "light_row_front": [(_case(LIT, scene="counts", lanes=8, ts=2, vis="list", depth="none"), "gtex"), (_case(LIT, scene="counts", lanes=8, ts=5), "gtex")],
    "light_view_ignored": [(_case(LIT, scene="views", B=2, ts=2, tb=0, lb=0), "gtex"), (_case(LIT, scene="views", B=33, ts=4, off=0), "gtex")],
    "view32_missing": [(_case(LIT, scene="views", B=B, ts=ts, off=off), "gtex") for B in (33, 64, 65) for ts in (2, 4) for off in (0, 4)],
    "view_twice": [(_case(LIT, scene="views", B=B, ts=ts, off=off), "gtex") for B in X.VIEW_COUNTS for ts in (2, 4) for off in (0, 4)],
    "large_not_zeroed": [(_case(LIT, scene="limit", lanes=lanes, ts=2, det=0), "gtex") for lanes in (8, 64)] + [(_case(LIT, scene="slivers", lanes=8), "gtex")],
    "back_vertices_unreversed": [(_case(LIT, scene="counts", lanes=8, ts=2, depth="vertex", form=None), "depth"), (_case(LIT, scene="hub", lanes=64), "depth")],
    "scales_exchanged": [(_case(LIT, scene="counts", form="records"), o) for o in ("gtex", "depth")] + [(_case(LIT, scene="counts", form="maps"), "gtex")],
    "light_grad_lit": [(_case(LIT, scene="counts", lanes=8, ts=2, vis="list", depth="none"), "glight"), (_case(LIT, scene="counts", lanes=8, ts=1), "glight")],
    "corner_reversed": [(_case(LIT, scene="counts", lanes=8, ts=2, vis="list", depth="none"), "gtex"), (_case(LIT, scene="counts", lanes=8, ts=3), "gtex")],
    "bleed_dropped": [(_case(LIT, scene="counts", lanes=8, ts=1), "gtex"), (_case(LIT, scene="views", ts=1, tb=0), "gtex")],
    "finv_transposed": [(_case(LIT, scene="counts", lanes=8, ts=2, depth="faces"), "depth"), (_case(LIT, scene="holes", ts=3, depth="vertex"), "depth")],
}


@pytest.mark.parametrize("variant", [v for v in X.VARIANTS if v != "flip_ignored"])
def test_wrong_lit_variants_are_rejected(variant):
    assert REJECTED_ON[variant]
    for c, output in REJECTED_ON[variant]:
        ref = lit_reference(c)[output]
        if output == "depth":
            gf, gv = _depth_variant(c, variant)
            wrong = gv if c.depth == "vertex" else gf
        else:
            wrong = _lit_variant(c, variant)[output]
        assert X.outside(wrong, ref), (variant, c, output)


def test_wrong_variants_of_the_plain_operators_are_rejected():
    for c in X.mesh_cases():
        sc, inp = X.scene(c.scene, c.lanes, c.B), X.inputs(c.scene, c.lanes, c.B, 2, 1, 1)
        tri = None if c.tb else X.tri_views(sc)[1]
        for variant in ("chunk_last_dropped", "pixel_twice", "finv_transposed", "back_vertices_unreversed", "flip_ignored"):
            if (variant == "flip_ignored" and not c.flip) or (variant == "back_vertices_unreversed" and not any(k % sc["Fp"] >= sc["F"] for k in sc["box"])):
                continue                            # (no back copy owns a pixel there)
            gf, n = X.depth_adjoint(sc, inp["g_depth"], "f64", variant, flip=bool(c.flip))
            assert X.outside(X.to_vertices(sc, gf, n, variant, tri=tri)[0], mesh_reference(c)), (c, variant)
    for c in X.depth_cases():
        sc, inp = X.scene(c.scene, c.lanes, c.B), X.inputs(c.scene, c.lanes, c.B, 2, 1, 1)
        for variant in ("chunk_last_dropped", "pixel_twice", "finv_transposed"):
            if variant == "finv_transposed" and c.finv:
                continue                            # (the map is an input)
            assert X.outside(X.depth_adjoint(sc, inp["g_depth"], "f64", variant, finv_map=bool(c.finv))[0], depth_reference(c)), (c, variant)
    for c in X.plain_cases():
        m, inp = X.sampling_maps(c.scene, c.lanes, c.B, c.ts), X.inputs(c.scene, c.lanes, c.B, c.ts, 1, 1)
        assert X.outside(X.plain_texels(m, inp["g_rgb"], "f64", "pixel_twice")[0], plain_reference(c)), c
        if c.ts == 1:
            assert X.outside(X.plain_texels(m, inp["g_rgb"], "f64", "bleed_dropped")[0], plain_reference(c)), c


def test_float32_restatement_is_inside_every_tolerance():
    for c in LIT:
        sc, ref = X.scene(c.scene, c.lanes, c.B), lit_reference(c)
        r = X.lit_adjoint(sc, lit_inputs(c), c.ts, "f32", form=c.form)
        assert not X.outside(r["gtex"], ref["gtex"]) and not X.outside(r["glight"], ref["glight"]), c
        assert np.isfinite(ref["gtex"][1]).all() and np.isfinite(ref["glight"][1]).all(), c
        # an element without a term has no bound: the GPU test then asks for an exact zero
        assert ((ref["gtex"][1] == 0) == (ref["gtex"][0] == 0)).all() or c.ts == 1, c
        if ref["depth"] is not None:
            assert np.isfinite(ref["depth"][1]).all() and np.abs(ref["depth"][0]).max() > 0, c


# ---- 5. E32 ---------------------------------------------------------------------------------------------------------------------------------
def test_print_e32_of_every_case():
    """printed once (`pytest -s`); the largest per entry point is in docs/EXPERIMENTS.md next to what the kernels achieved"""
    worst = {}

    def note(key, c, e):
        print(f"TEXELDEPTH-E32 {X.case_id(c)} {key} E32={e:.3e}")
        assert e < 64 * X.U, (c, key, e)            # a float32 evaluation of a well conditioned case
        worst[key] = max(worst.get(key, 0.0), e)
    for c in LIT:
        r = lit_reference(c)
        note("lit_textures", c, r["gtex"][2])
        note("lit_light", c, r["glight"][2])
        if r["depth"] is not None:
            note("lit_depth", c, r["depth"][2])
    for c in X.plain_cases():
        note("backward_textures", c, plain_reference(c)[2])
    for c in X.depth_cases():
        note("backward_depth_map", c, depth_reference(c)[2])
    for c in X.mesh_cases():
        note("backward_depth_map_mesh", c, mesh_reference(c)[2])
    for k, v in sorted(worst.items()):
        print(f"TEXELDEPTH-E32-WORST {k} {v:.3e} = {v / X.U:.2f} u")
