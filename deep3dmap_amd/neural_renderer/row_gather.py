"""The host side of the long-row CSR gather that the fixed-order adjoints share (csrc/d3m_row_gather.h states the format and
the order of the sums once): uv_textures (the transpose of a layout), vertex_colors (the adjacency of the faces) and
mesh_regularizers (the neighbour and the wing CSR) build their CSRs, their long-row tables and their caches with this.

A row of up to LONG_ROW items is summed by its own lane(s) in item order.  A longer row (a hub) must not make one lane walk
thousands of items: it is cut into chunks of CHUNK items, each reduced by a workgroup in a fixed order, and the chunk sums are
added in chunk order -- no float atomics, the same bits on every run."""
from collections import OrderedDict

import numpy as np
import torch

from . import rasterize_ops

LONG_ROW = 64           # rows with more items go through the chunked reduction
CHUNK = 1024            # items per chunk (one workgroup of 256 lanes)
CACHE_SIZE = 8          # built structures kept per cache (least recently used goes)


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


def tensor_key(t):
    """What names a tensor in a cache key: its address, version, shape, dtype and device (None for None).  An entry that
    holds the tensor keeps the address taken."""
    return None if t is None else (t.data_ptr(), t._version, tuple(t.shape), t.dtype, str(t.device))


def checked_faces(faces):
    if not torch.is_tensor(faces) or faces.dtype not in (torch.int32, torch.int64):
        raise ValueError("faces must be an int32 or int64 tensor")
    if not ((faces.dim() == 2 or (faces.dim() == 3 and faces.shape[0] == 1)) and faces.shape[-1] == 3 and faces.shape[-2] >= 1):
        raise ValueError("faces must be [num_faces, 3] or [1, num_faces, 3]")
    return faces


class BuiltCache:
    """Bounded LRU cache of structures built from the caller's tensors.  An entry also holds those tensors (`holders`): the
    key names them by address and version, and holding them keeps those addresses taken.  An entry handed out inside a
    stream capture is registered with rasterize_ops._captured_refs, so the captured step that replays it keeps it alive
    after eviction (graph.CapturedStep.capture claims it).  A build inside a capture raises: the warm-up step builds it."""

    what = "the cached structure"           # (names the payload in the capture error; a subclass says what it keeps)

    def __init__(self, size=CACHE_SIZE):
        self.size = int(size)
        self._items = OrderedDict()

    def get(self, key, build, holders=()):
        hit = self._items.get(key)
        capturing = torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()
        if hit is None:
            if capturing:
                raise RuntimeError(f"{self.what} is not built yet and cannot be built "
                                   "inside a stream capture (it synchronises); run the step once eagerly first "
                                   "(graph.CapturedStep.capture's warm-up steps do)")
            hit = (build(), tuple(holders))
            self._items[key] = hit
            while len(self._items) > self.size:
                self._items.popitem(last=False)
        else:
            self._items.move_to_end(key)
        if capturing:
            rasterize_ops._captured_refs[id(hit[0])] = hit[0]
        return hit[0]

    def clear(self):
        self._items.clear()

    def __len__(self):
        return len(self._items)

    def __contains__(self, key):
        return key in self._items
