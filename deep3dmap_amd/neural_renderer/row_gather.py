"""The host side of the long-row CSR gather that the fixed-order adjoints share (csrc/d3m_row_gather.h states the format and
the order of the sums once): uv_textures (the transpose of a layout), vertex_colors (the adjacency of the faces) and
mesh_regularizers (the neighbour and the wing CSR) build their CSRs, their long-row tables and their caches with this.  The
adjacency of the faces itself lives here too: vertex_colors and the deterministic mode's per-vertex gathers (rasterize.py,
mesh_ops.py) walk the same one.

A row of up to LONG_ROW items is summed by its own lane(s) in item order.  A longer row (a hub) must not make one lane walk
thousands of items: it is cut into chunks of CHUNK items, each reduced by a workgroup in a fixed order, and the chunk sums are
added in chunk order -- no float atomics, the same bits on every run."""
from collections import namedtuple

import numpy as np
import torch

from .. import _lib
from .built_cache import CACHE_SIZE, BuiltCache, tensor_key  # noqa: F401 (they stay importable from here)

LONG_ROW = 64           # rows with more items go through the chunked reduction
CHUNK = 1024            # items per chunk (one workgroup of 256 lanes)


def csr_offsets(rows, num_rows):
    """(offsets [num_rows + 1] i64, counts [num_rows]) of a CSR whose items fall in `rows` (an integer tensor of row indices)."""
    counts = torch.bincount(rows, minlength=num_rows)
    offsets = torch.zeros(num_rows + 1, dtype=torch.int64, device=rows.device)
    offsets[1:] = torch.cumsum(counts, 0)
    return offsets, counts


def long_row_chunks(offsets, counts):
    """(chunks [C,2] i32, long_rows [L] i32, long_chunk_ptr [L+1] i32) of a CSR (offsets [R+1] i64, counts [R]): the rows of
    more than LONG_ROW items (few: hubs), ascending, each cut into item ranges [start, end) of CHUNK items in row order.
    Synchronises."""
    dev = offsets.device
    long_rows = torch.nonzero(counts > LONG_ROW).flatten()
    starts = offsets[long_rows].cpu().numpy()
    ends = offsets[long_rows + 1].cpu().numpy()
    n_ch = (ends - starts + CHUNK - 1) // CHUNK
    long_chunk_ptr = np.zeros(len(starts) + 1, np.int64)
    long_chunk_ptr[1:] = np.cumsum(n_ch)
    chunk_start = np.repeat(starts, n_ch) + CHUNK * (np.arange(int(long_chunk_ptr[-1])) - np.repeat(long_chunk_ptr[:-1], n_ch))
    chunks = np.stack([chunk_start, np.minimum(chunk_start + CHUNK, np.repeat(ends, n_ch))], 1).astype(np.int32)
    return (torch.from_numpy(chunks.reshape(-1, 2)).to(dev), long_rows.to(torch.int32).contiguous(),
            torch.from_numpy(long_chunk_ptr.astype(np.int32)).to(dev))


Csr = namedtuple("Csr", "offsets items chunks long_rows long_chunk_ptr num_rows num_chunks num_long_rows c")
Csr.__doc__ = """One gathered CSR as the kernels read it (all i32, on one device): offsets [R+1], items in the node's layout,
chunks [C,2] item ranges of the long rows, long_rows [L] (ascending), long_chunk_ptr [L+1], the counts R, C, L, and `c`: the
d3m_csr (include/d3m_raster.h) that points at them, NULL for an empty tensor; entry points take ctypes.byref(csr.c).  Whoever
holds the Csr keeps the tensors `c` points at."""


def build_csr(rows, num_rows, items):
    """The Csr of `items` (any integer dtype, one or more columns, already in row order) over num_rows rows; `rows` (i64): the
    row index of every item, in any order (they are only counted).  Synchronises (the long rows)."""
    offsets, counts = csr_offsets(rows, num_rows)
    tensors = (offsets.to(torch.int32), items.to(torch.int32).contiguous(), *long_row_chunks(offsets, counts))
    sizes = (int(num_rows), tensors[2].shape[0], tensors[3].shape[0])
    c = _lib.D3MCsr(*[t.data_ptr() if t.numel() else None for t in tensors], *sizes, LONG_ROW)
    return Csr(*tensors, *sizes, c)


def checked_faces(faces):
    if not torch.is_tensor(faces) or faces.dtype not in (torch.int32, torch.int64):
        raise ValueError("faces must be an int32 or int64 tensor")
    if not ((faces.dim() == 2 or (faces.dim() == 3 and faces.shape[0] == 1)) and faces.shape[-1] == 3 and faces.shape[-2] >= 1):
        raise ValueError("faces must be [num_faces, 3] or [1, num_faces, 3]")
    return faces


Adjacency = namedtuple("Adjacency", "csr tri num_vertices num_faces")
Adjacency.__doc__ = """The faces of one mesh as the kernels read them: tri [F,3] i32 and csr, the Csr of V rows whose items [3F]
are 3 f + c, ascending per vertex (offsets and items are what d3m_vertex_gather walks)."""


class AdjacencyCache(BuiltCache):
    """BuiltCache for adjacencies: an entry also holds the caller's faces tensor."""
    what = "the faces' adjacency (textures_from_vertex_colors, the deterministic mode's per-vertex gathers)"


_cache = AdjacencyCache()


def _faces_key(faces, num_vertices):
    return tensor_key(faces) + (int(num_vertices),)


def build_adjacency(faces, num_vertices):
    """The Adjacency of faces [F,3] or [1,F,3] (int32 or int64, any device) over num_vertices vertices.  Raises ValueError
    for an index outside [0, num_vertices).  Synchronises (the range check, the long rows): never inside a capture."""
    V = int(num_vertices)
    flat = faces.reshape(-1).long()
    lo, hi = int(flat.min()), int(flat.max())
    if lo < 0 or hi >= V:
        raise ValueError(f"faces: vertex indices must be in [0, {V}) (found {lo if lo < 0 else hi})")
    # stable: a vertex's items keep ascending order
    csr = build_csr(flat, V, torch.argsort(flat, stable=True))
    return Adjacency(csr, faces.reshape(-1, 3).to(torch.int32).contiguous(), V, int(flat.numel() // 3))


def vertex_adjacency(faces, num_vertices, cache=None):
    """The cached Adjacency of a faces tensor (built on the first call with this tensor at its current version, outside
    any stream capture); `cache`: the AdjacencyCache to keep it in (default: the module's)."""
    cache = _cache if cache is None else cache
    return cache.get(_faces_key(faces, num_vertices), lambda: build_adjacency(faces, num_vertices), holders=(faces,))
