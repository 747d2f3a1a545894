"""A float32 numpy replay of the long-row CSR gather (csrc/d3m_row_gather.h states the order): every addition the kernels
make, in their order, so the result can be compared bit for bit.  Sequential sums are np.cumsum from a leading 0 (np.sum and
np.add.reduce add pairwise and give other bits); lanes are array rows, and a butterfly step is v + v[lane ^ off]."""
import numpy as np

BLOCK = 256         # lanes of the workgroup that reduces one chunk
WAVE = 64


def seq_sum(t):
    """s = 0; s += t[i] for i ascending, in float32, per column of t [n, N]."""
    zero = np.zeros((1, t.shape[1]), np.float32)
    return np.cumsum(np.concatenate([zero, t.astype(np.float32, copy=False)]), axis=0, dtype=np.float32)[-1]


def butterfly(v):
    """v [L, N] (L a power of two) -> v after v += shfl_xor(v, off) for off = L/2, ..., 1: every lane holds the sum."""
    lane = np.arange(v.shape[0])
    off = v.shape[0] // 2
    while off >= 1:
        v = v + v[lane ^ off]
        off //= 2
    return v


def chunk_sum(terms, start, end):
    """The workgroup's sum of items [start, end): lane t adds items start + t, start + t + 256, ... in order from 0, a
    64-lane butterfly in each of the four waves, then s = 0; s += wave[w] in wave order."""
    acc = np.zeros((BLOCK, terms.shape[1]), np.float32)
    for first in range(start, end, BLOCK):
        n = min(BLOCK, end - first)
        acc[:n] = acc[:n] + terms[first:first + n]
    waves = np.stack([butterfly(acc[w * WAVE:(w + 1) * WAVE])[0] for w in range(BLOCK // WAVE)])
    return seq_sum(waves)


def replay_gather(terms, offsets, chunks, long_rows, long_chunk_ptr, long_row, lanes_per_row=1):
    """[R, N] float32: row r's sum of terms [n_items, N] (CSR order, float32) over offsets [R + 1].  A row of up to long_row
    items (or any row when there are no long rows): lane `sub` of its lanes_per_row lanes adds items sub, sub + L, ... in
    order from 0, then the butterfly over the L lanes.  A longer row: lane 0 adds the row's chunk sums in chunk order from 0
    (the other lanes hold 0) and the same butterfly follows."""
    terms = np.ascontiguousarray(terms, np.float32)
    offsets, chunks = np.asarray(offsets, np.int64), np.asarray(chunks, np.int64).reshape(-1, 2)
    long_rows, long_chunk_ptr = [int(r) for r in long_rows], np.asarray(long_chunk_ptr, np.int64)
    L, N = int(lanes_per_row), terms.shape[1]
    out = np.zeros((len(offsets) - 1, N), np.float32)
    for r in range(len(offsets) - 1):
        start, end = int(offsets[r]), int(offsets[r + 1])
        lanes = np.zeros((L, N), np.float32)
        if end - start > long_row and long_rows:
            l = long_rows.index(r)
            sums = [chunk_sum(terms, int(chunks[c, 0]), int(chunks[c, 1])) for c in range(long_chunk_ptr[l], long_chunk_ptr[l + 1])]
            assert int(chunks[long_chunk_ptr[l], 0]) == start and int(chunks[long_chunk_ptr[l + 1] - 1, 1]) == end
            lanes[0] = seq_sum(np.stack(sums))
        else:
            for sub in range(min(L, end - start)):
                lanes[sub] = seq_sum(terms[start + sub:end:L])
        out[r] = butterfly(lanes)[0]
    return out
