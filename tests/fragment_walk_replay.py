"""A float32 numpy replay of stage 1 of the coverage-record adjoints (csrc/d3m_fragments.h states THE ORDER): the per-visible-
face sums over owned pixels of k_vertex_attribute_face_sums / _large_face_sums and k_fragment_geometry_face_sums /
_large_face_sums, every addition in the kernels' order, so that G and Gv can be compared word for word.  Sequential sums and the
64-lane butterfly are tests/row_gather_replay.py's.  The library is built with -ffp-contract=off, so every operation below
rounds once, as numpy's float32 operators do."""
import numpy as np

from row_gather_replay import BLOCK, WAVE, butterfly, seq_sum

FM_LANES = 8                # csrc/d3m_face_major.h
SCAN_CHUNK = 32             # box pixels per chunk of scan_owned_pixels with 8 lanes
FM_MAX_BBOX_AREA = 4096
F32 = np.float32


def pixel_bbox(face, S):
    """csrc/d3m_forward.h pixel_bbox() restated for face [3,3] float32: (x0, x1, y0, y1), or None when the face has no box."""
    x, y = np.asarray(face, F32)[:, 0], np.asarray(face, F32)[:, 1]
    if x[0] == x[1] == x[2] and y[0] == y[1] == y[2]:
        return None
    if not (np.isfinite(x).all() and np.isfinite(y).all()):
        return 0, S - 1, 0, S - 1
    x, y = x.astype(np.float64), y.astype(np.float64)
    m = 4e-6 * (max(np.abs(x).max(), np.abs(y).max()) + 1.0)
    lx, hx = np.ceil(((x.min() - m) * S + S - 1) * 0.5), np.floor(((x.max() + m) * S + S - 1) * 0.5)
    ly, hy = np.ceil(((y.min() - m) * S + S - 1) * 0.5), np.floor(((y.max() + m) * S + S - 1) * 0.5)
    if lx > S - 1 or hx < 0 or ly > S - 1 or hy < 0 or lx > hx or ly > hy:
        return None
    return int(max(lx, 0)), int(min(hx, S - 1)), int(max(ly, 0)), int(min(hy, S - 1))


# ---- the two routes: terms [n, N] float32 of the face's owned pixels, box [n] their ascending box pixel numbers ----------------
def small_route_lanes(box):
    """lane -> the positions (into box / terms) it adds, in its order: the box is cut into chunks of 32 consecutive box pixels;
    WITHIN each chunk the owned pixels are ranked in ascending box order and lane `sub` takes ranks sub, sub + 8, ...; a lane
    goes through chunk 0's, then chunk 1's, ..."""
    lanes = [[] for _ in range(FM_LANES)]
    chunk = np.asarray(box) // SCAN_CHUNK
    for c in np.unique(chunk):
        for rank, pos in enumerate(np.nonzero(chunk == c)[0]):
            lanes[rank % FM_LANES].append(int(pos))
    return lanes


def quad_sum_lane0(v):
    """v [8, N]: the three steps of quad_sum (lane ^ 1, lane ^ 2, the mirror 7 - lane), as lane 0 ends up"""
    lane = np.arange(FM_LANES)
    v = v + v[lane ^ 1]
    v = v + v[lane ^ 2]
    v = v + v[FM_LANES - 1 - lane]
    return v[0]


def small_route_sum(terms, box, lanes_of=small_route_lanes):
    acc = np.stack([seq_sum(terms[l]) for l in lanes_of(box)])
    return quad_sum_lane0(acc)


def large_route_sum(terms, box):
    """lane t adds the owned pixels among box pixels t, t + 256, ... in that order from 0; a 64-lane butterfly per wave; the four
    wave sums added from 0 in wave order"""
    acc = np.zeros((BLOCK, terms.shape[1]), F32)
    for pos, i in enumerate(np.asarray(box)):                         # (ascending box order is every lane's own order)
        acc[i % BLOCK] = acc[i % BLOCK] + terms[pos]
    waves = np.stack([butterfly(acc[w * WAVE:(w + 1) * WAVE])[0] for w in range(BLOCK // WAVE)])
    return seq_sum(waves)


def replay_face_sums(face_index_map, faces, term, n_sums):
    """(sums [B, Fp, n_sums] float32, visible [B, Fp] bool, large [B, Fp] bool): stage 1 of every face that owns a pixel; rows of
    the others are left NaN.  term(b, fn, face [3,3], xs, ys) -> [n, n_sums] float32: the per-pixel terms of the face's owned
    pixels (xs, ys in ascending box order).  Asserts that every owned pixel lies in the restated box."""
    fim, faces = np.asarray(face_index_map), np.asarray(faces, F32)
    B, S = fim.shape[:2]
    Fp = faces.shape[1]
    sums = np.full((B, Fp, n_sums), np.nan, F32)
    visible, large = np.zeros((B, Fp), bool), np.zeros((B, Fp), bool)
    for b in range(B):
        for fn in np.unique(fim[b][fim[b] >= 0]):
            ys, xs = np.nonzero(fim[b] == fn)
            bbox = pixel_bbox(faces[b, fn], S)
            assert bbox is not None, (b, fn)
            x0, x1, y0, y1 = bbox
            assert xs.min() >= x0 and xs.max() <= x1 and ys.min() >= y0 and ys.max() <= y1, (b, fn, bbox)
            bw = x1 - x0 + 1
            box = (ys - y0) * bw + (xs - x0)                           # (np.nonzero is row-major: ascending)
            terms = np.ascontiguousarray(term(b, int(fn), faces[b, fn], xs, ys), F32)
            visible[b, fn] = True
            large[b, fn] = bw * (y1 - y0 + 1) > FM_MAX_BBOX_AREA
            sums[b, fn] = large_route_sum(terms, box) if large[b, fn] else small_route_sum(terms, box)
    return sums, visible, large


# ---- the nodes' per-pixel terms ------------------------------------------------------------------------------------------------
def _out_pixel(xs, ys, S, aa):
    return (xs >> 1, (S - 1 - ys) >> 1) if aa else (xs, S - 1 - ys)


def attribute_term(weight_map, depth_map, grad_images, anti_aliasing):
    """u_c * (scale * g[b, k, out(p)]), u_c = w_c * (d / z_c): [n, 3 C], corner-major (G's layout [3, C])"""
    w, d, g = np.asarray(weight_map, F32), np.asarray(depth_map, F32), np.asarray(grad_images, F32)
    S, scale = d.shape[1], F32(0.25 if anti_aliasing else 1.0)

    def term(b, fn, face, xs, ys):
        xo, yo = _out_pixel(xs, ys, S, anti_aliasing)
        u = w[b, ys, xs] * (d[b, ys, xs][:, None] / face[None, :, 2])  # [n,3]
        sg = scale * g[b][:, yo, xo].T                                # [n,C]
        return (u[:, :, None] * sg[:, None, :]).reshape(len(xs), -1)
    return term


def geometry_term(pixel_grads):
    """fg_face and fg_add_pixel (csrc/d3m_fragment_geometry.h) operation by operation: [n, 9], corner-major (Gv's [3, 3])"""
    h = np.asarray(pixel_grads, F32)
    S, one = h.shape[1], F32(1.0)

    def term(b, fn, face, xs, ys):
        (x0, y0, z0), (x1, y1, z1), (x2, y2, z2) = face
        z = (z0, z1, z2)
        den = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
        nx = ((y1 - y2) / den, (y2 - y0) / den, (y0 - y1) / den)
        ny = ((x2 - x1) / den, (x0 - x2) / den, (x1 - x0) / den)
        dx = (2 * xs + 1 - S).astype(F32) / F32(S) - x2
        dy = (2 * ys + 1 - S).astype(F32) / F32(S) - y2
        b0 = nx[0] * dx + ny[0] * dy
        b1 = nx[1] * dx + ny[1] * dy
        bc = (b0, b1, (one - b0) - b1)
        t = [bc[c] / z[c] for c in range(3)]
        d = one / ((t[0] + t[1]) + t[2])
        u = [t[c] * d for c in range(3)]
        hp = h[b, ys, xs]
        hbar = (u[0] * hp[:, 0] + u[1] * hp[:, 1]) + u[2] * hp[:, 2]
        e = [hp[:, c] - hbar for c in range(3)]
        A = [(d / z[c]) * e[c] for c in range(3)]
        px = (nx[0] * A[0] + nx[1] * A[1]) + nx[2] * A[2]
        py = (ny[0] * A[0] + ny[1] * A[1]) + ny[2] * A[2]
        out = np.empty((len(xs), 9), F32)
        for k in range(3):
            out[:, 3 * k + 0] = -bc[k] * px
            out[:, 3 * k + 1] = -bc[k] * py
            out[:, 3 * k + 2] = -(u[k] / z[k]) * e[k]
        return out
    return term
