"""Reads the C ABI out of include/d3m_raster.h: the header is the binding, stated once.  Regular expressions over the
comment-stripped text, no C grammar: read_header() knows the constructs that header uses and raises ValueError, naming the
text, on anything else -- it never skips or guesses a declaration."""
import collections
import ctypes
import re

Abi = collections.namedtuple("Abi", "structs functions constants")
#   structs    {C name: ctypes.Structure subclass}, in declaration order
#   functions  {C name: (restype, [(parameter name, ctype), ...])}
#   constants  {C name: int}: the enumerators and every #define with an integer value

_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "long": ctypes.c_long, "size_t": ctypes.c_size_t}
# What a pointer may point to besides a scalar above.  Such a pointer is a DEVICE pointer (the header's first comment) and
# travels as an integer ...
_DEVICE_ONLY = {"void", "double", "int32_t", "uint64_t", "unsigned char"}
# ... except the pointers that are host memory by their type (base, number of stars).
_HOST = {("size_t", 1): ctypes.POINTER(ctypes.c_size_t), ("void", 2): ctypes.POINTER(ctypes.c_void_p),
         ("char", 2): ctypes.POINTER(ctypes.c_char_p), ("char", 1): ctypes.c_char_p}

_STATEMENT = re.compile(r"""\s*(?:
      typedef\s+void\s*\*\s*(?P<handle>\w+)                                  # typedef void* d3m_stream_t
    | typedef\s+struct\s+(?P<forward>\w+)\s+(?P=forward)                     # typedef struct name name
    | enum\s*\{(?P<enum>[^{}]*)\}
    | (?:typedef\s+)?struct\s*(?P<tag>\w*)\s*\{(?P<fields>[^{}]*)\}\s*(?P<alias>\w*)
    | (?P<ret>[\w\s*]+?)\b(?P<function>d3m_\w+)\s*\((?P<parameters>[^()]*)\)
    )\s*;""", re.X)


def class_name(c_name):
    """d3m_camera_grad -> D3MCameraGrad, d3m_g2s_block -> D3MG2SBlock"""
    return "D3M" + c_name[len("d3m_"):].title().replace("_", "")


def read_header(text, host_arrays=None):
    """The Abi of a header's text.  host_arrays {(function, parameter): ctype} types the host arrays that their C type does
    not tell from device pointers; a key the header does not have is an error."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    constants = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(D3M_\w+)[ \t]+(\S.*?)[ \t]*$", text, flags=re.M):
        try:
            constants[name] = int(value, 0)
        except ValueError:      # not an integer (D3M_UV_TEXTURE_REG_NO_EPS): nothing Python binds
            pass
    text = re.sub(r"#ifdef __cplusplus.*?#endif", " ", text, flags=re.S)      # extern "C" { ... }
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M).rstrip()
    scalars, structs, functions = dict(_SCALARS), {}, {}
    host_arrays = dict(host_arrays or {})

    def ctype(c_type):
        stars = c_type.count("*")
        base = " ".join(re.sub(r"\bconst\b|\*", " ", c_type).split())
        if base in structs and stars <= 1:
            return ctypes.POINTER(structs[base]) if stars else structs[base]
        if (base, stars) in _HOST:
            return _HOST[base, stars]
        if stars == 0 and base in scalars:
            return scalars[base]
        if stars == 1 and (base in scalars or base in _DEVICE_ONLY):
            return ctypes.c_void_p
        raise ValueError(f"d3m_raster.h: unknown type {' '.join(c_type.split())!r}")

    def struct(name):
        if name not in structs:
            structs[name] = type(class_name(name), (ctypes.Structure,), {})
        return structs[name]

    at = 0
    while at < len(text):
        m = _STATEMENT.match(text, at)
        if not m:
            raise ValueError(f"d3m_raster.h: cannot parse {' '.join(text[at:].split())[:120]!r}")
        at = m.end()
        if m["handle"]:
            scalars[m["handle"]] = ctypes.c_void_p
        elif m["forward"]:
            struct(m["forward"])
        elif m["enum"] is not None:
            for entry in filter(None, map(str.strip, m["enum"].split(","))):
                d = re.fullmatch(r"(\w+)\s*=\s*(-?\w+)", entry)
                if not d:
                    raise ValueError(f"d3m_raster.h: cannot read the enumerator {entry!r}")
                constants[d[1]] = int(d[2], 0)
        elif m["fields"] is not None:
            fields = []
            for declaration in filter(None, map(str.strip, m["fields"].split(";"))):
                d = re.fullmatch(r"((?:const\s+)?(?:unsigned\s+)?\w+)\b(.*)", declaration, flags=re.S)
                names = [re.fullmatch(r"\s*(\**)\s*(\w+)\s*", n) for n in d[2].split(",")] if d else [None]
                if not all(names):
                    raise ValueError(f"d3m_raster.h: cannot split the field declaration {declaration!r}")
                fields += [(n[2], ctype(d[1] + n[1])) for n in names]
            struct(m["alias"] or m["tag"])._fields_ = fields
        else:
            parameters = []
            if m["parameters"].strip() != "void":
                for p in m["parameters"].split(","):
                    d = re.fullmatch(r"\s*(.*\S)\s*\b(\w+)\s*", p, flags=re.S)
                    if not d:
                        raise ValueError(f"d3m_raster.h: cannot split the parameter {p!r} of {m['function']}")
                    parameters.append((d[2], host_arrays.pop((m["function"], d[2]), None) or ctype(d[1])))
            functions[m["function"]] = (None if m["ret"].strip() == "void" else ctype(m["ret"]), parameters)
    if host_arrays:
        raise ValueError(f"d3m_raster.h has no {sorted(host_arrays)}")
    return Abi(structs, functions, constants)
