"""The one cache of structures built from a caller's tensors (a CSR, a transpose, a checked index vector, a concatenated
basis): keyed by the tensors' address and version, bounded, and safe under a captured step -- what it hands out inside a stream
capture outlives its entry for as long as the step's graphs do."""
from collections import OrderedDict

import torch

from . import rasterize_ops

CACHE_SIZE = 8          # built structures kept per cache (least recently used goes)


def tensor_key(t):
    """What names a tensor in a cache key: its address, version, shape, dtype and device (None for None).  An entry that
    holds the tensor keeps the address taken."""
    return None if t is None else (t.data_ptr(), t._version, tuple(t.shape), t.dtype, str(t.device))


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
