"""The owner look-ups of a crossing (d3m_edge_grad.h: crossing_shape / crossing_owners / crossing_decide) decide whether its
outward walk exists (the in-pixel is the face's) and whether a short inward range holds a pixel of the face at all (none:
no record).  K4's grad_faces against the reference's K4 -- its own kernels compiled for the device where they were built,
the oracle's C port otherwise; gradients to 1e-3 of the tensor's largest entry, as tests/test_gpu_reference.py -- on scenes
that sit on that rule's edges: inward ranges around XG_DEAD_SCAN pixels, ranges clipped at pixel 0 and S - 1, in-pixels on
the image border, in-pixels a nearer face owns; S = 33 and 64, one view and three, both forms of the plan.  And exactly:
every line's record count is the number of its crossings with a record, and two builds give the same plan."""
import numpy as np
import pytest
import torch

import edge_chain_scenes as E

pytestmark = pytest.mark.gpu

GRAD_RTOL = 1e-3
XG_DEAD_SCAN = 6
ONE_PASS_FACES = 2048 * 42 + 84          # blocks of 42 faces from which the plan takes the one-pass form (edge_plan_form)


def _view_triangles(S, seed):
    """(triangles in pixel coordinates, depths) of one view"""
    rng = np.random.default_rng(100 + seed)
    u = rng.uniform
    tris, z = [], []
    for k in range(6):                      # thin wedges: lines of every inward length up to ~10 pixels
        a0, b0 = u(3, S - 16), u(2, 6)
        t = [(a0, b0), (a0 + u(8, 11), b0 + u(0, 2)), (a0 + u(2, 8), S - u(3, 6))]
        tris.append(t if k % 2 == 0 else [(y, x) for x, y in t])
        z.append(1.0 + 0.05 * k)
    for k in range(4):                      # nearer faces over parts of them: in-pixels that belong to another face
        cx, cy = u(8, S - 8), u(8, S - 8)
        tris.append([(cx - u(3, 9), cy - u(3, 9)), (cx + u(3, 9), cy - u(0, 6)), (cx + u(-3, 3), cy + u(3, 9))])
        z.append(0.5 + 0.05 * k)
    m = S / 2.0
    border = [
        # strips that reach one pixel into the image: in-pixels on the border, inward ranges clipped at 0 / S - 1
        [(-9.3, 4.4), (0.6, 6.2), (-7.1, S - 5.3)], [(S - 1.6, 5.2), (S + 8.3, 7.7), (S + 6.1, S - 4.2)],
        [(5.5, -8.2), (S - 6.3, -7.4), (m + 0.2, 0.7)], [(4.4, S + 7.3), (m + 1.3, S - 1.6), (S - 5.2, S + 8.8)],
        # wedges across the border: in-pixels inside, ranges clipped
        [(-6.2, m - 3.3), (12.4, m + 0.4), (-5.5, m + 4.6)], [(S + 5.2, m - 4.3), (S - 11.6, m - 0.7), (S + 6.4, m + 3.9)],
        [(m - 4.1, -5.3), (m + 0.6, 11.7), (m + 3.8, -6.6)], [(m - 3.6, S + 5.1), (m - 0.3, S - 12.2), (m + 4.4, S + 6.3)],
    ]
    border = [[(x + u(-0.2, 0.2), y + u(-0.2, 0.2)) for x, y in t] for t in border]
    tris += border
    z += [0.8] * len(border)
    return tris, z


def _faces(S, B, pad):
    """[B,F,3,3]; `pad`: front-facing faces far outside the raster up to ONE_PASS_FACES per view (no pixel, no crossing)"""
    views = []
    for b in range(B):
        tris, z = _view_triangles(S, 10 * S + b)
        f = E.pixel_triangles(tris, S, z=z)
        if pad:
            n = ONE_PASS_FACES - len(f)
            o = S + 100.0 + 3.0 * (np.arange(n) % 64)
            far = [[(a, a), (a + 2.0, a + 0.5), (a + 0.5, a + 2.0)] for a in o]
            f = np.concatenate([f[:len(f) // 2], E.pixel_triangles(far, S), f[len(f) // 2:]])
        views.append(f)
    return torch.from_numpy(np.stack(views)).cuda().contiguous()


_cache = {}


def _scene(S, B, pad):
    """faces, the reference's maps and its K4, shared by the cases of one shape and left unchanged"""
    key = (S, B, pad)
    if key not in _cache:
        faces = _faces(S, B, pad)
        tex, g_rgb, g_alpha = E.random_inputs(B, faces.shape[1], S, S + B)
        maps, gf_ref, _ = E.reference_k4(faces, tex, S, g_rgb, g_alpha)
        _cache[key] = (faces, maps, g_rgb, g_alpha, gf_ref)
    return _cache[key]


def _canonical(pv):
    """the plan without what depends on arrival order (the list's chunks, the crossing bases, a record's rank under its line):
    per crossing, lanes by (face, edge, axis), whether it has a record and the record"""
    first, end = pv.lane_runs()
    lanes = np.argsort(np.repeat(pv.visible_list[:pv.n_visible].astype(np.int64), 6) * 6 + np.arange(first.size) % 6)
    first, end = first[lanes], end[lanes]
    count = end - first
    idx = np.repeat(first, count) + np.arange(int(count.sum())) - np.repeat(np.cumsum(count) - count, count)
    at = pv.xpos[idx].astype(np.int64)
    return at >= 0, np.where((at >= 0)[:, None], pv.xrec[np.maximum(at, 0)], 0)


# (padded, forced form): the counted form of a small batch, the one-pass form the padded batch takes by itself, and the
# counted form forced on that batch
FORMS = [(False, None), (True, None), (True, 1)]


@pytest.mark.parametrize("pad,form", FORMS, ids=["counted-small", "one-pass", "counted-forced"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("S", [33, 64])
def test_k4_against_reference_on_the_rules_edges(S, B, pad, form):
    faces, maps, g_rgb, g_alpha, gf_ref = _scene(S, B, pad)
    F = faces.shape[1]
    gf, plan, vis, ws = E.run_k4(faces, maps, g_rgb, g_alpha, S, form=form)
    pv = E.PlanView(plan, vis, ws, B, F, S)
    assert pv.one_pass == (pad and form is None) and pv.complete
    ok = torch.isfinite(gf_ref)
    assert torch.equal(ok, torch.isfinite(gf))
    scale = float(gf_ref[ok].abs().max())
    assert scale > 0
    err = float((gf[ok] - gf_ref[ok]).abs().max())
    print(f"S {S} B {B} pad {pad} form {form}: max |d| {err:.3e} of {scale:.3e} ({err / scale:.2e})")
    assert err <= GRAD_RTOL * scale
    # exactly: a line's records are its crossings that have one
    c, line = pv.crossings(faces)
    has = pv.xpos[c] >= 0
    assert np.array_equal(np.bincount(line[has], minlength=B * 2 * S), pv.line_cursor)
    assert 0 < int(has.sum()) < has.size                 # some crossings are idle: no record
    # ... and a second build of the same scene gives the same plan, and the same gradient
    gf2, plan2, vis2, ws2 = E.run_k4(faces, maps, g_rgb, g_alpha, S, form=form)
    pv2 = E.PlanView(plan2, vis2, ws2, B, F, S)
    assert np.array_equal(pv.line_cursor, pv2.line_cursor) and pv.total == pv2.total
    m1, r1 = _canonical(pv)
    m2, r2 = _canonical(pv2)
    assert np.array_equal(m1, m2) and np.array_equal(r1, r2)
    E.assert_bit_equal(gf2.cpu().numpy(), gf.cpu().numpy())


@pytest.mark.parametrize("S", [33, 64])
def test_scenes_sit_on_the_rules_edges(S):
    """what the scenes claim, read from the records: in-pixels of another face (no outward walk) with inward ranges on both
    sides of the look-through threshold, ranges clipped at both ends of a line, in-pixels on the border"""
    B = 3
    faces, maps, g_rgb, g_alpha, _ = _scene(S, B, False)
    _, plan, vis, ws = E.run_k4(faces, maps, g_rgb, g_alpha, S)
    pv = E.PlanView(plan, vis, ws, B, faces.shape[1], S)
    c, _ = pv.crossings(faces)
    rec = pv.xrec[pv.xpos[c][pv.xpos[c] >= 0]]
    bits = rec[:, 3] & 0x3F
    alive, dirpos, owner = (bits & 1) != 0, (bits & 2) != 0, (bits & 16) != 0
    assert alive.all()
    in_from, in_to = (rec[:, 2] & 0xFFFF).astype(np.int64), (rec[:, 2] >> 16).astype(np.int64)
    span = in_to - in_from                   # looked through iff span < XG_DEAD_SCAN, i.e. at most XG_DEAD_SCAN pixels
    d1_cross = rec[:, 0].copy().view(np.float32)
    d1_in = np.where(dirpos, np.floor(d1_cross), np.ceil(d1_cross)).astype(np.int64)
    hidden = ~owner
    for s in (XG_DEAD_SCAN - 2, XG_DEAD_SCAN - 1, XG_DEAD_SCAN, XG_DEAD_SCAN + 1):
        assert (hidden & (span == s)).any(), ("no occluded in-pixel with an inward range of %d pixels" % (s + 1))
    assert (in_from == 0).any() and (in_to == S - 1).any()
    assert (d1_in == 0).any() and (d1_in == S - 1).any()
