"""A float32 numpy replay of the per-set parameter sums (csrc/d3m_set_sums.h states the order): every addition the partial
and the finish kernels make, in their order, so the partial arrays can be compared bit for bit.  Lanes are array rows; a
butterfly or DPP step is v + v[the lane it reads]; sequential sums are row_gather_replay's seq_sum."""
import numpy as np

from row_gather_replay import butterfly, seq_sum

BLOCK = 256         # lanes of the workgroup that reduces one part
WAVE = 64
XOR_BUTTERFLY, DPP_ROWS = "xor_butterfly", "dpp_rows"


def parts_of(items, per_part, max_parts):
    """set_parts: per_part elements each, at least 1, at most max_parts"""
    return min(max(-(-int(items) // per_part), 1), max_parts)


def lane_sums(terms, part, parts):
    """[256, N]: lane t of part `part` adds the terms of elements 256 part + t, + 256 parts, ... in that order, from 0."""
    acc = np.zeros((BLOCK, terms.shape[1]), np.float32)
    for first in range(BLOCK * part, terms.shape[0], BLOCK * parts):
        n = min(BLOCK, terms.shape[0] - first)
        acc[:n] = acc[:n] + terms[first:first + n]
    return acc


def dpp_rows(v):
    """v [64, N] -> [N], wave_sum of csrc/d3m_device.h: inside each row of 16 lanes the ^1 and ^2 quad swaps, the mirror
    inside the half of 8, the mirror inside the row; then (r0 + r1) + (r2 + r3) of lanes 0, 16, 32 and 48."""
    lane = np.arange(WAVE)
    v = v + v[lane ^ 1]
    v = v + v[lane ^ 2]
    v = v + v[(lane & ~7) | (7 - (lane & 7))]
    v = v + v[(lane & ~15) | (15 - (lane & 15))]
    return (v[0] + v[16]) + (v[32] + v[48])


def wave_tree(v, tree):
    return butterfly(v)[0] if tree == XOR_BUTTERFLY else dpp_rows(v)


def part_sum(acc, tree):
    """[256, N] lane sums -> [N]: the wave tree in each of the four waves, then ((w0 + w1) + w2) + w3."""
    w = [wave_tree(acc[k * WAVE:(k + 1) * WAVE], tree) for k in range(BLOCK // WAVE)]
    return ((w[0] + w[1]) + w[2]) + w[3]


def set_partials(terms, per_part, max_parts, tree):
    """[parts, N] float32: what the partial kernel stores for one set with terms [elements, N] (float32, element order).  A
    term the kernel skips is a row of zeros here: a lane's sum never holds -0, so adding 0 to it changes no bit."""
    terms = np.ascontiguousarray(terms, np.float32)
    parts = parts_of(terms.shape[0], per_part, max_parts)
    return np.stack([part_sum(lane_sums(terms, p, parts), tree) for p in range(parts)])


def add_parts(partials):
    """[parts, N] -> [N]: the finish kernel's s = 0; s += partial[p] for p ascending."""
    return seq_sum(partials)


def naive_partials(terms, per_part, max_parts):
    """the same elements per part, added by np.sum (pairwise): what an order-blind check would accept"""
    terms = np.ascontiguousarray(terms, np.float32)
    parts = parts_of(terms.shape[0], per_part, max_parts)
    return np.stack([np.concatenate([terms[first:first + BLOCK] for first in range(BLOCK * p, terms.shape[0], BLOCK * parts)])
                     .sum(0, dtype=np.float32) for p in range(parts)])
