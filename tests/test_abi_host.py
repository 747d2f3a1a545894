"""The binding is read from include/d3m_raster.h (deep3dmap_amd/_abi.py): the reader on a header of this file's own, the
derived structs' layout against the compiler's, and that nothing the hand-written table bound was lost (no GPU)."""
import ctypes
import os
import re
import subprocess
from ctypes import POINTER, c_char_p, c_float, c_int, c_long, c_size_t, c_void_p

import pytest

from deep3dmap_amd import _abi, _lib

HEADER = """\
/* One of each construct the reader knows; comments with ( and ; and { in them: int d3m_in_a_comment(int a); */
#ifndef D3M_TEST_H
#define D3M_TEST_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef void* d3m_stream_t; /* a handle ( */
enum {
    D3M_OK = 0,   /* fine; */
    D3M_ERR_X = 1 /* struct { */
};
enum { D3M_MODE_A = 0, D3M_MODE_B = 3 };
#define D3M_FLAG 16
#define D3M_HEX 0x20
#define D3M_NO_EPS (-1.0f)
typedef struct {
    float* grad;        /* [n] (written; NULL = skipped) */
    int a, b, c;
} d3m_plain;
typedef struct d3m_later d3m_later;
int d3m_uses_later(const d3m_later* later, d3m_stream_t stream);
typedef struct d3m_tagged {
    const float* K; int K_batch;
    float *rot, *trans;
    const float *depth, *albedo;
    size_t bytes;
    const unsigned char* marks;
} d3m_tagged;
typedef struct d3m_g2s_outer {
    d3m_plain one, two;
    const d3m_tagged* tagged;
    long count;
} d3m_g2s_outer;
struct d3m_later {
    void* blob;
    uint64_t* z;
};
const char* d3m_name(void);
void d3m_enable(int on);
size_t d3m_bytes(int n, long m, float eps, size_t* each);
int d3m_wrapped(const float* in, const int32_t* index, void* const* ptrs,
                const size_t* sizes, void** out, const char** names, int* counts,
                const d3m_g2s_outer* outer, double* image, d3m_stream_t stream);
#ifdef __cplusplus
}
#endif
#endif /* D3M_TEST_H */
"""
COUNTS = {("d3m_wrapped", "counts"): POINTER(c_int)}


def test_reader_on_a_header_of_its_own():
    abi = _abi.read_header(HEADER, COUNTS)
    assert abi.constants == {"D3M_OK": 0, "D3M_ERR_X": 1, "D3M_MODE_A": 0, "D3M_MODE_B": 3, "D3M_FLAG": 16, "D3M_HEX": 32}
    assert list(abi.structs) == ["d3m_plain", "d3m_later", "d3m_tagged", "d3m_g2s_outer"]
    plain, later, tagged, outer = abi.structs.values()
    assert [c.__name__ for c in abi.structs.values()] == ["D3MPlain", "D3MLater", "D3MTagged", "D3MG2SOuter"]
    assert all(issubclass(c, ctypes.Structure) for c in abi.structs.values())
    assert plain._fields_ == [("grad", c_void_p), ("a", c_int), ("b", c_int), ("c", c_int)]
    assert later._fields_ == [("blob", c_void_p), ("z", c_void_p)]
    assert tagged._fields_ == [("K", c_void_p), ("K_batch", c_int), ("rot", c_void_p), ("trans", c_void_p), ("depth", c_void_p),
                               ("albedo", c_void_p), ("bytes", c_size_t), ("marks", c_void_p)]
    assert outer._fields_ == [("one", plain), ("two", plain), ("tagged", POINTER(tagged)), ("count", c_long)]
    assert abi.functions == {
        "d3m_uses_later": (c_int, [("later", POINTER(later)), ("stream", c_void_p)]),
        "d3m_name": (c_char_p, []),
        "d3m_enable": (None, [("on", c_int)]),
        "d3m_bytes": (c_size_t, [("n", c_int), ("m", c_long), ("eps", c_float), ("each", POINTER(c_size_t))]),
        "d3m_wrapped": (c_int, [("in", c_void_p), ("index", c_void_p), ("ptrs", POINTER(c_void_p)), ("sizes", POINTER(c_size_t)),
                                ("out", POINTER(c_void_p)), ("names", POINTER(c_char_p)), ("counts", POINTER(c_int)),
                                ("outer", POINTER(outer)), ("image", c_void_p), ("stream", c_void_p)])}
    # without the table the host array is what its type says: a pointer to a scalar
    assert dict(_abi.read_header(HEADER).functions["d3m_wrapped"][1])["counts"] is c_void_p

    def refused(text, names, host_arrays=None):
        with pytest.raises(ValueError, match=re.escape(names)):
            _abi.read_header(text, host_arrays)

    end = "#ifdef __cplusplus\n}"
    refused(HEADER.replace(end, "int d3m_bad(short x);\n" + end), "unknown type 'short'")
    refused(HEADER.replace("long count;", "ptrdiff_t count;"), "unknown type 'ptrdiff_t'")
    refused(HEADER.replace("long count;", "float rgb[3];"), "float rgb[3]")
    refused(HEADER.replace(end, "int d3m_bad(int (*callback)(int), int n);\n" + end), "int d3m_bad(int (*callback)(int), int n);")
    refused(HEADER.replace(end, "int d3m_bad(int);\n" + end), "'int' of d3m_bad")
    refused(HEADER.replace("D3M_ERR_X = 1", "D3M_ERR_X"), "D3M_ERR_X")
    refused(HEADER, "('d3m_wrapped', 'count')", {("d3m_wrapped", "count"): POINTER(c_int)})
    refused(HEADER, "('d3m_gone', 'counts')", {("d3m_gone", "counts"): POINTER(c_int)})


def _layout_asserts(scale=1):
    lines = [f'#include "{os.path.abspath(_lib.HEADER)}"', "#include <stddef.h>"]
    for name, cls in _lib._ABI.structs.items():
        lines.append(f'static_assert(sizeof({name}) == {ctypes.sizeof(cls) * scale}, "sizeof({name})");')
        lines += [f'static_assert(offsetof({name}, {f}) == {getattr(cls, f).offset}, "offsetof({name}, {f})");'
                  for f, _ in cls._fields_]
    return "\n".join(lines) + "\n"


def test_derived_struct_layouts_are_the_compilers(tmp_path):
    """sizeof and every offsetof of the derived classes as static_asserts against the real header: a dropped, reordered or
    mistyped field does not compile."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    source = _layout_asserts()
    assert source.count("static_assert") == len(_lib._ABI.structs) + sum(len(c._fields_) for c in _lib._ABI.structs.values())
    (tmp_path / "layout.cpp").write_text(source)
    (tmp_path / "wrong.cpp").write_text(_layout_asserts(scale=2))      # the check has teeth
    run = lambda f: subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-fsyntax-only", str(tmp_path / f)],
                                   capture_output=True, text=True)
    ok = run("layout.cpp")
    assert ok.returncode == 0, ok.stderr
    wrong = run("wrong.cpp")
    assert wrong.returncode != 0 and "sizeof(d3m_camera)" in wrong.stderr


def test_nothing_the_hand_written_table_bound_is_lost():
    assert len(_lib._SIGNATURES) >= 174 and _lib.exported_symbols() == sorted(_lib._ABI.functions)
    # the ten classes under their names, with today's sizes and field counts, and the constants with today's values
    classes = {"D3MCamera": (64, 12), "D3MBasis": (40, 7), "D3MCameraGrad": (48, 6), "D3MVertexTarget": (32, 6),
               "D3MLight": (64, 10), "D3MCsr": (56, 9), "D3MFragments": (80, 12), "D3MMeshTopology": (128, 5),
               "D3MFitTargets": (136, 17), "D3MG2SBlock": (400, 57)}
    assert sorted(c.__name__ for c in _lib._ABI.structs.values()) == sorted(classes)
    for name, (size, fields) in classes.items():
        cls = getattr(_lib, name)
        assert issubclass(cls, ctypes.Structure) and (ctypes.sizeof(cls), len(cls._fields_)) == (size, fields), name
    assert (_lib.CAMERA_NONE, _lib.CAMERA_LOOK_AT, _lib.CAMERA_LOOK, _lib.CAMERA_PROJECTION) == (0, 1, 2, 3)
    assert (_lib.PRECLEARED, _lib.FIT_FINISH_DEFERRED, _lib.FIT_POOLED, _lib.GRAD_OF_OUTPUT_IMAGE) == (1, 2, 4, 32)
    assert (_lib.FRONT_RANGES, _lib.ZERO_RANGES_MAX) == (10, 6)
    # every parameter is bound: an independent count, the commas of the raw declaration
    src = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    declared = {name: 0 if params.strip() == "void" else params.count(",") + 1
                for name, params in re.findall(r"\b(d3m_[a-z0-9_]+)\s*\(([^()]*)\)", src)}
    assert declared == {name: len(args) for name, (_, args) in _lib._SIGNATURES.items()}
    # the host arrays the table names, and the struct pointers typed as the header types them
    assert _lib._SIGNATURES["d3m_timing_collect"][1] == [POINTER(c_char_p), POINTER(c_int), POINTER(c_float), c_int]
    assert _lib._SIGNATURES["d3m_pose_tree_constants"] == (None, [POINTER(c_int)])
    assert _lib._SIGNATURES["d3m_backward_depth_map_mesh"][1][8] == POINTER(_lib.D3MVertexTarget)
    assert _lib._SIGNATURES["d3m_g2s_forward"] == (c_int, [POINTER(_lib.D3MG2SBlock), c_void_p])
