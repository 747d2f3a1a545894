"""ctypes binding of libd3m_raster.so (include/d3m_raster.h).  There is no fallback: if the HIP
library is missing or a call fails, this module raises."""
import ctypes
import os

import torch

from . import _abi
from .build import LOAD_PATH as LIB_PATH, _headers

_I, _F, _SZ, _P = ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.c_void_p

# The header is the binding: the structs (D3MCamera, D3MCsr, D3MG2SBlock, ...: _abi.class_name), every entry point's
# restype / argtypes and the constants are read from include/d3m_raster.h, once per process, here.  Only the host arrays
# whose C type does not tell them from device pointers are named by hand.
_HOST_ARRAYS = {("d3m_timing_collect", "counts"): ctypes.POINTER(_I), ("d3m_timing_collect", "total_ms"): ctypes.POINTER(_F),
                ("d3m_pose_tree_constants", "out4"): ctypes.POINTER(_I)}
HEADER = _headers()[-1]      # include/d3m_raster.h, where the build looks for it
with open(HEADER) as _header:
    _ABI = _abi.read_header(_header.read(), _HOST_ARRAYS)
globals().update({cls.__name__: cls for cls in _ABI.structs.values()})
_SIGNATURES = {name: (res, [t for _, t in params]) for name, (res, params) in _ABI.functions.items()}

CAMERA_NONE, CAMERA_LOOK_AT, CAMERA_LOOK, CAMERA_PROJECTION = (
    _ABI.constants["D3M_CAMERA_" + n] for n in ("NONE", "LOOK_AT", "LOOK", "PROJECTION"))
PRECLEARED, FIT_FINISH_DEFERRED, FIT_POOLED, GRAD_OF_OUTPUT_IMAGE = (     # the flags: what each means is in the header
    _ABI.constants["D3M_" + n] for n in ("PRECLEARED", "FIT_FINISH_DEFERRED", "FIT_POOLED", "GRAD_OF_OUTPUT_IMAGE"))
FRONT_RANGES = 10         # clears d3m_lit_front takes

_lib = None


def exported_symbols():
    """Every entry point include/d3m_raster.h declares."""
    return sorted(_SIGNATURES)


def lib():
    """The loaded library.  Raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: the HIP extension has not been built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (or `python -m deep3dmap_amd.build`). "
                "deep3dmap_amd has no CPU / eager fallback.")
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(handle, name)     # AttributeError if the build is stale
            fn.restype, fn.argtypes = res, args
        _lib = handle
    return _lib


def check(rc, what):
    if rc != 0:
        L = lib()
        raise RuntimeError(f"{what} failed: {L.d3m_error_string(rc).decode()} (code {rc}, hip error "
                           f"{L.d3m_last_hip_error()})")


def stream_ptr():
    """hipStream_t of torch's current stream on the current device.  (Through the raw accessor: torch.cuda.current_stream()
    builds a Stream object per call, ~9 us each and a dozen calls per eager render step.)"""
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(torch.cuda.current_device()))


def ptr(t):
    """Device pointer of a tensor, or NULL for None."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def require_device(*tensors, names=None):
    """The reference's CHECK_INPUT (rasterize_cuda.cpp:66-68): CUDA + contiguous, else RuntimeError.
    Dtypes: the reference's launchers dispatch on faces' type (rasterize_cuda_kernel.cu:614, float and double) and then
    read every map with .data<scalar_t>() / .data<int32_t>(), which raises for a tensor of another type; its Python side
    only ever allocates float32 / int32 maps (rasterize.py:50-69), so scalar_t = double cannot get past the first map.
    This library instantiates scalar_t = float only and raises the same kind of error up front."""
    for i, t in enumerate(tensors):
        if t is None:
            continue
        n = names[i] if names else f"argument {i}"
        if not t.is_cuda:
            raise RuntimeError(f"{n} must be a CUDA tensor")
        if not t.is_contiguous():
            raise RuntimeError(f"{n} must be contiguous")
        if t.is_floating_point() and t.dtype != torch.float32:
            raise RuntimeError(f"{n}: expected scalar type Float but found {t.dtype}; "
                               "libd3m_raster is built for float32 (the reference's float64 dispatch, "
                               "rasterize_cuda_kernel.cu:614, is not reachable from its own Python either)")


COVERAGE_FORMS = {"auto": -1, "binned": 0, "bidding": 1}


class coverage_form:
    """Context manager: run the forward's coverage in one form ("auto" | "binned" | "bidding", d3m_set_coverage_form)."""

    def __init__(self, form):
        self.form = COVERAGE_FORMS[form] if isinstance(form, str) else int(form)

    def __enter__(self):
        self.previous = lib().d3m_get_coverage_form()
        check(lib().d3m_set_coverage_form(self.form), "d3m_set_coverage_form")
        return self

    def __exit__(self, *exc):
        lib().d3m_set_coverage_form(self.previous)
        return False


class deterministic:
    """Context manager: the visibility list in ascending face order (d3m_set_deterministic) inside the block."""

    def __init__(self, on=True):
        self.on = int(bool(on))

    def __enter__(self):
        self.previous = lib().d3m_get_deterministic()
        check(lib().d3m_set_deterministic(self.on), "d3m_set_deterministic")
        return self

    def __exit__(self, *exc):
        lib().d3m_set_deterministic(self.previous)
        return False


ZERO_RANGES_MAX = 6       # FILL_RANGES of csrc/d3m_launch.h


def zero_(*tensors):
    """Zero-fill contiguous device tensors, up to six per launch (d3m_zero_ranges); returns them.  The kernel takes raw
    (pointer, byte count) ranges of whole 4-byte words: a tensor that is not contiguous (its data_ptr + numel would
    cover its neighbours) or whose size is not a multiple of four bytes is cleared by torch instead."""
    raw = []
    for t in tensors:
        if t is None or t.numel() == 0:
            continue
        if t.is_contiguous() and (t.numel() * t.element_size()) % 4 == 0 and t.data_ptr() % 4 == 0:
            raw.append(t)
        else:
            t.zero_()
    for at in range(0, len(raw), ZERO_RANGES_MAX):
        ts = raw[at:at + ZERO_RANGES_MAX]
        ptrs = (_P * len(ts))(*[t.data_ptr() for t in ts])
        sizes = (_SZ * len(ts))(*[t.numel() * t.element_size() for t in ts])
        check(lib().d3m_zero_ranges(ptrs, sizes, len(ts), stream_ptr()), "d3m_zero_ranges")
    return tensors


def zero_raw(ranges):
    """Zero (device pointer, bytes) ranges -- 4-byte multiples -- with as few launches as d3m_zero_ranges allows."""
    ranges = [(int(p), int(n)) for p, n in ranges if p and n]
    for at in range(0, len(ranges), ZERO_RANGES_MAX):
        part = ranges[at:at + ZERO_RANGES_MAX]
        ptrs = (_P * len(part))(*[p for p, _ in part])
        sizes = (_SZ * len(part))(*[n for _, n in part])
        check(lib().d3m_zero_ranges(ptrs, sizes, len(part), stream_ptr()), "d3m_zero_ranges")


def tensor_range(t):
    """(device pointer, bytes) of a contiguous tensor whose size is a multiple of four bytes"""
    assert t.is_contiguous() and (t.numel() * t.element_size()) % 4 == 0
    return t.data_ptr(), t.numel() * t.element_size()


def kernel_timing(enable):
    lib().d3m_timing_enable(int(bool(enable)))


def collect_kernel_times(max_entries=64):
    """{kernel name: (launches, total ms)} since timing was enabled / last collected (synchronises)."""
    names = (ctypes.c_char_p * max_entries)()
    counts = (_I * max_entries)()
    ms = (_F * max_entries)()
    n = lib().d3m_timing_collect(names, counts, ms, max_entries)
    return {names[i].decode(): (counts[i], ms[i]) for i in range(n)}
