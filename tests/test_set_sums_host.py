"""The per-set parameter sums (csrc/d3m_set_sums.h), host side: the cases and inputs of tests/test_gpu_set_sums.py, their
float32 terms, and the proof that a bit-exact pass there means something -- at every shape of at least 256 elements the
replay (tests/set_sums_replay.py) with the OTHER wave tree, and the same elements added by np.sum, each differ from the stated
tree in at least one word.  No GPU."""
import collections
import zlib

import numpy as np
import pytest

import set_sums_replay as R

# the nodes' constants (d3m_pose.h, d3m_light_grad.h)
POSE = dict(per_part=256, max_parts=64, sums=12, tree=R.DPP_ROWS)
LIGHT = dict(per_part=1024, max_parts=128, sums=9, tree=R.XOR_BUTTERFLY)

PoseCase = collections.namedtuple("PoseCase", "V B shared")
LightCase = collections.namedtuple("LightCase", "F Bl")

# 257: a second part holding one lane; 16 387 = 64 * 256 + 3: the cap of 64 parts, three lanes take a second element
POSE_CASES = [PoseCase(V, B, shared) for V in (1, 65, 257, 16387) for B, shared in ((1, False), (3, False), (3, True))]
# 1025: a second part; 131 077 = 128 * 1024 + 5: the cap of 128 parts, and the lanes stride
LIGHT_CASES = [LightCase(F, Bl) for F in (1, 65, 1025, 131077) for Bl in (1, 3)]


def case_id(c):
    return "-".join(f"{f}{int(v)}" for f, v in zip(c._fields, c))


def _rng(c):
    return np.random.default_rng(zlib.crc32(case_id(c).encode()))


def pose_inputs(c):
    """vertices [1 or B,V,3], pose [B,7] (scale, three angles, translation) and grad_posed [B,V,3], float32"""
    rng = _rng(c)
    x = rng.standard_normal(((1 if c.shared else c.B), c.V, 3)).astype(np.float32)
    pose = (rng.standard_normal((c.B, 7)) * [0.1, 0.3, 0.3, 0.3, 1, 1, 1] + [1, 0, 0, 0, 0, 0, 0]).astype(np.float32)
    return x, pose, rng.standard_normal((c.B, c.V, 3)).astype(np.float32)


def pose_terms(x, g, b):
    """[V,12] float32, set b: g[j] * x[c] row-major (one float32 product each), then g[j] itself"""
    xb = x[b if x.shape[0] > 1 else 0]
    return np.concatenate([(g[b][:, :, None] * xb[:, None, :]).reshape(-1, 9), g[b]], 1)


def light_inputs(c):
    """grad_light [Bl,F,3] float32 with about one row in sixteen all zeros (those the kernel skips)"""
    rng = _rng(c)
    g = rng.standard_normal((c.Bl, c.F, 3)).astype(np.float32)
    g[rng.random((c.Bl, c.F)) < 1 / 16] = 0
    return g


def pose_partials(c, tree=None):
    x, _pose, g = pose_inputs(c)
    return np.stack([R.set_partials(pose_terms(x, g, b), POSE["per_part"], POSE["max_parts"], tree or POSE["tree"])
                     for b in range(c.B)])


def light_partials(c, tree=None):
    g = light_inputs(c)
    return np.stack([R.set_partials(g[b], LIGHT["per_part"], LIGHT["max_parts"], tree or LIGHT["tree"]) for b in range(c.Bl)])


def _words(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def test_the_cases_reach_every_regime_of_the_tree():
    assert [R.parts_of(c.V, 256, 64) for c in POSE_CASES[::3]] == [1, 1, 2, 64]
    assert [R.parts_of(c.F, 1024, 128) for c in LIGHT_CASES[::2]] == [1, 1, 2, 128]
    assert 16387 > 64 * 256 and 131077 > 128 * 1024                 # beyond the cap: a lane takes a second element
    assert {(c.B, c.shared) for c in POSE_CASES} == {(1, False), (3, False), (3, True)}


def test_both_wave_trees_and_the_part_order_are_exact_on_integers():
    rng = np.random.default_rng(7)
    t = rng.integers(-8, 9, (70000, 5)).astype(np.float32)
    for tree in (R.XOR_BUTTERFLY, R.DPP_ROWS):
        for per_part, max_parts in ((256, 64), (1024, 128)):
            p = R.set_partials(t, per_part, max_parts, tree)
            assert p.shape == (R.parts_of(70000, per_part, max_parts), 5)
            assert np.array_equal(R.add_parts(p), t.sum(0, dtype=np.float64).astype(np.float32))
    one = np.zeros((64, 1), np.float32)
    for lane in range(64):          # every lane reaches the result of either tree exactly once
        one[:] = 0
        one[lane] = 1
        assert R.dpp_rows(one)[0] == 1 and R.butterfly(one)[0, 0] == 1


def test_the_combine_starts_from_wave_zero():
    acc = np.full((R.BLOCK, 1), -0.0, np.float32)
    for tree in (R.XOR_BUTTERFLY, R.DPP_ROWS):
        assert np.signbit(R.part_sum(acc, tree)[0])         # ((-0 + -0) + -0) + -0 = -0; s = 0; s += w gives +0


@pytest.mark.parametrize("c", POSE_CASES, ids=case_id)
def test_pose_replay_tells_the_trees_apart(c):
    right = pose_partials(c)
    assert right.shape == (c.B, R.parts_of(c.V, 256, 64), 12) and np.isfinite(right).all()
    x, _pose, g = pose_inputs(c)
    naive = np.stack([R.naive_partials(pose_terms(x, g, b), 256, 64) for b in range(c.B)])
    assert np.allclose(right, naive, rtol=0, atol=1e-3 * max(1.0, np.abs(naive).max()))
    if c.V >= 256:
        assert (_words(right) != _words(pose_partials(c, R.XOR_BUTTERFLY))).any()
        assert (_words(right) != _words(naive)).any()


@pytest.mark.parametrize("c", LIGHT_CASES, ids=case_id)
def test_light_replay_tells_the_trees_apart(c):
    right = light_partials(c)
    assert right.shape == (c.Bl, R.parts_of(c.F, 1024, 128), 3) and np.isfinite(right).all()
    g = light_inputs(c)
    assert c.F < 1025 or (g == 0).all(-1).any()
    naive = np.stack([R.naive_partials(g[b], 1024, 128) for b in range(c.Bl)])
    assert np.allclose(right, naive, rtol=0, atol=1e-3 * max(1.0, np.abs(naive).max()))
    if c.F >= 256:
        assert (_words(right) != _words(light_partials(c, R.DPP_ROWS))).any()
        assert (_words(right) != _words(naive)).any()
