"""tests/fragment_walk_replay.py on the CPU: the order it replays (csrc/d3m_fragments.h, THE ORDER of stage 1) is not any of the
orders one might take it for -- on a constructed face the replay's words differ from ranks counted over the whole box (the
literal reading of the comment this replaced), from np.sum and from a plain sequential sum -- and the pixel_bbox restatement
against boxes computed by hand."""
import numpy as np

import fragment_walk_replay as R
from row_gather_replay import seq_sum


def _constructed_face():
    """A 12 x 10 box (120 box pixels: four chunks of 32) whose face owns every pixel but each seventh: 27 or 28 owned pixels in
    each of the three full chunks, so ranks beyond 8 occur in more than two chunks and the per-chunk ranks part from the ranks
    over the box after the first chunk.  27 terms a pixel with magnitudes spread over 2^20."""
    box = np.array([i for i in range(120) if i % 7 != 3])
    rng = np.random.default_rng(7)
    terms = (rng.standard_normal((len(box), 27)) * 2.0 ** rng.integers(-10, 11, (len(box), 27))).astype(np.float32)
    return box, terms


def test_the_constructed_face_has_ranks_beyond_eight_in_two_chunks():
    box, _ = _constructed_face()
    counts = np.bincount(box // R.SCAN_CHUNK)
    assert box.max() >= R.SCAN_CHUNK and int((counts > R.FM_LANES).sum()) >= 2, counts


def test_the_replayed_order_is_none_of_the_plausible_others():
    box, terms = _constructed_face()
    got = R.small_route_sum(terms, box)
    n = len(box)
    others = {
        "ranks over the whole box": R.small_route_sum(terms, box, lambda b: [list(range(sub, n, R.FM_LANES))
                                                                             for sub in range(R.FM_LANES)]),
        "np.sum": np.sum(terms, axis=0, dtype=np.float32),
        "a sequential sum": seq_sum(terms),
    }
    exact = terms.astype(np.float64).sum(0)
    for name, other in others.items():
        assert other.dtype == np.float32 and other.shape == got.shape
        differing = int((other.view(np.int32) != got.view(np.int32)).sum())
        print(name, "differing words:", differing, "of", got.size)
        assert differing > 0, name
        # (another order of the same terms, not another sum)
        assert np.allclose(other, exact, rtol=0, atol=2.0 ** -24 * n * np.abs(terms).astype(np.float64).sum(0).max())
    assert np.allclose(got, exact, rtol=0, atol=2.0 ** -24 * n * np.abs(terms).astype(np.float64).sum(0).max())


def test_a_lane_goes_through_the_chunks_in_order_with_ranks_from_zero_in_each():
    box = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 31, 32, 40, 63, 64, 65, 66, 67, 68, 69, 70, 71, 72])
    lanes = R.small_route_lanes(box)
    assert [[int(box[p]) for p in l] for l in lanes] == [[0, 8, 32, 64, 72], [1, 9, 40, 65], [2, 31, 63, 66], [3, 67], [4, 68],
                                                         [5, 69], [6, 70], [7, 71]]


def test_quad_sum_is_the_stated_tree():
    a = (np.random.default_rng(3).standard_normal((8, 5)) * 1e3).astype(np.float32)
    want = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[7] + a[6]) + (a[5] + a[4]))
    assert np.array_equal(R.quad_sum_lane0(a).view(np.int32), want.view(np.int32))


def test_large_route_is_lane_strided_then_butterfly_then_the_four_waves():
    rng = np.random.default_rng(5)
    box = np.sort(rng.choice(5000, 3000, replace=False))
    terms = (rng.standard_normal((3000, 2)) * 2.0 ** rng.integers(-10, 11, (3000, 2))).astype(np.float32)
    got = R.large_route_sum(terms, box)
    lanes = np.stack([seq_sum(terms[box % 256 == t]) for t in range(256)])
    waves = []
    for w in range(4):
        v = lanes[64 * w:64 * w + 64]
        for off in (32, 16, 8, 4, 2, 1):
            v = v + v[np.arange(64) ^ off]
        waves.append(v[0])
    want = (((np.float32(0) + waves[0]) + waves[1]) + waves[2]) + waves[3]
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert (got.view(np.int32) != seq_sum(terms).view(np.int32)).any()


def _face(xs, ys):
    return np.array([[xs[0], ys[0], 1.0], [xs[1], ys[1], 1.0], [xs[2], ys[2], 1.0]], np.float32)


def test_pixel_bbox_against_hand_computed_boxes():
    S = 16                                                            # NDC v -> pixel (16 v + 15) / 2
    # x in [-0.5, 0.5] -> 3.5 .. 11.5 -> 4 .. 11; y in [-0.25, 0.75] -> 5.5 .. 13.5 -> 6 .. 13
    assert R.pixel_bbox(_face((-0.5, 0.5, 0.0), (-0.25, -0.25, 0.75)), S) == (4, 11, 6, 13)
    # a corner exactly on the centre of pixel 3 (v = -9/16) keeps that pixel; 0.4375 = the centre of pixel 11
    assert R.pixel_bbox(_face((-0.5625, 0.4375, 0.0), (-0.5625, -0.5625, 0.4375)), S) == (3, 11, 3, 11)
    # partly off screen: x in [-1.5, -0.8] -> -4.5 .. 1.1 -> 0 .. 1; y in [0.5, 2] -> 11.5 .. 23.5 -> 12 .. 15
    assert R.pixel_bbox(_face((-1.5, -0.8, -1.0), (0.5, 2.0, 1.0)), S) == (0, 1, 12, 15)
    # wholly off screen, between two pixel centres, three coincident corners: no box
    assert R.pixel_bbox(_face((1.2, 1.5, 1.3), (0.0, 0.5, 0.2)), S) is None
    assert R.pixel_bbox(_face((0.01, 0.02, 0.03), (0.01, 0.03, 0.02)), S) is None
    assert R.pixel_bbox(_face((0.25, 0.25, 0.25), (0.5, 0.5, 0.5)), S) is None
    # a corner that is not finite: the whole screen
    assert R.pixel_bbox(_face((np.nan, 0.5, 0.0), (0.0, 0.5, 0.2)), S) == (0, 15, 0, 15)
    # the box of a whole-screen face at 128 is beyond the small route's limit
    x0, x1, y0, y1 = R.pixel_bbox(_face((-1.5, 1.5, -1.5), (-1.5, -1.5, 1.5)), 128)
    assert (x1 - x0 + 1) * (y1 - y0 + 1) == 128 * 128 > R.FM_MAX_BBOX_AREA
