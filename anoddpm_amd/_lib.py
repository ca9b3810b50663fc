"""ctypes binding of libanoddpm_hip.so, derived at import from include/anoddpm_hip.h.

The header is the one statement of the C ABI: its argument structs, entry points, op codes and constants -- fields, units and
meaning are documented there, next to the reference code each entry point replaces.  This module reads it and defines
  - one `ctypes.Structure` per `typedef struct`: `anoddpm_igemm_args` is `IgemmArgs`, `anoddpm_op` is `Op`; a field named like a
    Python keyword gets the suffix `p` (`in` is `inp`); every pointer field is a `c_void_p`
  - one integer per enum entry and integer `#define`, without the `ANODDPM_` prefix: `OP_IGEMM`, `ROC_NAN`, `ABI_VERSION`
  - `argtypes` / `restype` of every prototype, set by `lib()`; `SYMBOLS` lists their names, `_STRUCTS` the classes, both in
    declaration order.

The library is mandatory: there is NO CPU or eager-PyTorch fallback anywhere in this package.
`lib()` raises if the shared object is missing, and `require_cuda()` raises for non-HIP tensors.
"""
import ctypes
import keyword
import os
import re
from ctypes import POINTER, Structure, c_char_p, c_double, c_float, c_int, c_int16, c_int32, c_int64, c_uint32, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# ANODDPM_LIB_TAG=<tag>: load lib/libanoddpm_hip_<tag>.so instead -- a second build of the same sources with other compiler flags
# (ANODDPM_BUILD_TAG / ANODDPM_EXTRA_FLAGS of anoddpm_amd.build), for A/B measurements of one gpurun session.  Same ABI, same checks.
SO_PATH = os.path.join(_HERE, "lib", "libanoddpm_hip%s.so" % ("_" + os.environ["ANODDPM_LIB_TAG"] if os.environ.get("ANODDPM_LIB_TAG") else ""))
HEADER = os.path.join(os.path.dirname(_HERE), "include", "anoddpm_hip.h")      # anoddpm_amd.build.HEADER


class AnoddpmError(RuntimeError):
    pass


# ---- a reader of the restricted C the header is written in: whatever it does not recognise is an error, never skipped
_SCALARS = {"int": c_int, "int16_t": c_int16, "int32_t": c_int32, "int64_t": c_int64, "uint32_t": c_uint32, "uint64_t": c_uint64,
            "float": c_float, "double": c_double}
_POINTEES = set(_SCALARS) | {"void", "char", "long long", "uint8_t"}      # what a pointer may point to, besides the header's own structs


def _int(text):
    m = re.fullmatch(r"\(\s*(-?\d+)\s*\)|(-?\d+)", text.strip())
    if not m:
        raise AnoddpmError(f"anoddpm_hip.h: {text.strip()!r} is not an integer constant")
    return int(m[1] or m[2])


def _declarators(decl, structs):
    """'const float *a0, *a1' -> [('a0', 'float', True), ('a1', 'float', True)]: name, base type, is a pointer."""
    out, base = [], None
    for piece in decl.split(","):
        m = re.fullmatch(r"([\w\s*]*?)([A-Za-z_]\w*)", piece.strip())
        if not m:
            raise AnoddpmError(f"anoddpm_hip.h: {decl.strip()!r} is not a plain declaration")
        base = " ".join(w for w in m[1].replace("*", " ").split() if w != "const") or base      # 'a, b': b has a's base type
        pointer = "*" in m[1]
        if base not in _SCALARS and not (pointer and (base in _POINTEES or base in structs)):
            raise AnoddpmError(f"anoddpm_hip.h: {decl.strip()!r}: no ctypes mapping for type {base!r}")
        out.append((m[2], base, pointer))
    return out


def parse_header(text):
    """-> (structs {C name: [(field, base type, is a pointer)]}, constants {name: int}, prototypes {name: (return, [parameter])},
    return and parameter as the field triples), each in declaration order."""
    structs, consts, protos = {}, {}, {}

    def directive(m):
        w = m[1].split(None, 2)
        if w[:1] == ["define"] and len(w) == 3:                # a macro with a body; the include guard has none
            if not w[1].isidentifier():
                raise AnoddpmError(f"anoddpm_hip.h: macro {w[1]!r} takes parameters")
            consts[w[1]] = _int(w[2])
        return ""

    def struct(m):
        structs[m[2]] = [f for decl in m[1].split(";") if decl.strip() for f in _declarators(decl, structs)]
        return ""

    def enum(m):
        for entry in filter(None, (e.strip() for e in m[1].split(","))):
            name, eq, value = entry.partition("=")
            if not eq:
                raise AnoddpmError(f"anoddpm_hip.h: enum entry {entry!r} has no value")
            consts[name.strip()] = _int(value)
        return ""

    def proto(m):
        params = [] if m[2].strip() == "void" else [_declarators(p, structs)[0] for p in m[2].split(",")]
        ret, = _declarators(m[1], structs)
        protos[ret[0]] = (ret, params)
        return ""

    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#(.*)$", directive, text, flags=re.M)
    text = re.sub(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text)
    text = re.sub(r"enum\s*\{([^{}]*)\}\s*;", enum, text)
    text = re.sub(r"([\w\s*]+?)\(([^(){};]*)\)\s*;", proto, text)
    if text.split() not in ([], ["extern", '"C"', "{", "}"]):
        raise AnoddpmError(f"anoddpm_hip.h: not understood: {' '.join(text.split())[:200]!r}")
    return structs, consts, protos


def _ctype(base, pointer, ret=False):
    """Struct fields: every pointer is a c_void_p.  Parameters: a pointer to one of the header's structs is typed.  Return: a string."""
    if not pointer:
        return _SCALARS[base]
    if ret:
        if base != "char":
            raise AnoddpmError(f"anoddpm_hip.h: no ctypes mapping for a returned pointer to {base!r}")
        return c_char_p
    return POINTER(globals()[_PYNAME[base]]) if base in _PYNAME else c_void_p


if not os.path.exists(HEADER):
    raise AnoddpmError(f"{HEADER} is missing: the ctypes binding is derived from it")
with open(HEADER) as _f:
    _C_STRUCTS, _CONSTS, _PROTOS = parse_header(_f.read())
_PYNAME = {}                                                  # filled struct by struct: a struct can only point to an earlier one
for _c, _fields in _C_STRUCTS.items():
    _py = "".join(w.capitalize() for w in _c[len("anoddpm_"):].split("_"))
    globals()[_py] = type(_py, (Structure,), {"_fields_": [(n + "p" * keyword.iskeyword(n), c_void_p if p else _SCALARS[b]) for n, b, p in _fields]})
    _PYNAME[_c] = _py
globals().update({k[len("ANODDPM_"):]: v for k, v in _CONSTS.items()})          # OP_*, ROC_*, ..., ABI_VERSION
_STRUCTS = [globals()[_py] for _py in _PYNAME.values()]
SYMBOLS = list(_PROTOS)

# limits and selectors the header states in prose only
PHILOX_REVERSE, PHILOX_FORWARD, PHILOX_FILL, PHILOX_KNOWN, PHILOX_RENOISE = 0, 1, 2, 3, 4                          # the `domain` word of the philox counter
SSIM_MAX_WIN = 15
MEDIAN_SIZES = (3, 5, 7)                                                                # anoddpm_median_args.k
MEDIAN3D_SIZES = (3, 5)                                                                 # anoddpm_median3d_args.k
ERODE_MAX = 8                                                                           # anoddpm_erode_args.n
KEEP_DILATE_MAX = 8                                                                     # anoddpm_keep_mask_args.r

_lib = None


def _preload_torch_hip_runtime():
    """libanoddpm_hip.so must share ONE HIP runtime with PyTorch (streams, device pointers).  The torch
    wheel bundles its own libamdhip64 (SONAME libamdhip64.so.7, the same as /opt/rocm's); whichever copy is
    mapped first satisfies later DT_NEEDED lookups, so torch's copy is mapped before our library."""
    import glob
    import torch  # noqa: F401  (maps libtorch_hip and its bundled runtime)
    tl = os.path.join(os.path.dirname(torch.__file__), "lib")
    for name in ("libhsa-runtime64.so", "libamdhip64.so"):
        for path in glob.glob(os.path.join(tl, name + "*")):
            try:
                ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
            except OSError:
                pass
            break


def lib():
    """Load the HIP library (once).  Fails loudly: this package has no other compute path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise AnoddpmError(
            f"{SO_PATH} is missing: build it with `python -m anoddpm_amd.build` "
            "(hipcc --offload-arch=gfx950).  anoddpm_amd has no CPU / eager fallback.")
    _preload_torch_hip_runtime()
    L = ctypes.CDLL(SO_PATH)
    if L.anoddpm_abi_version() != ABI_VERSION:  # noqa: F821  (from the header, like every struct and constant)
        raise AnoddpmError("libanoddpm_hip.so ABI version mismatch; rebuild")
    for name, (ret, params) in _PROTOS.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = _ctype(*ret[1:], ret=True), [_ctype(*p[1:]) for p in params]
    for cname, st in zip(_C_STRUCTS, _STRUCTS):
        if L.anoddpm_struct_size(cname.encode()) != ctypes.sizeof(st):
            raise AnoddpmError(f"ABI struct {cname}: C sizeof {L.anoddpm_struct_size(cname.encode())} != ctypes {ctypes.sizeof(st)}")
    # kernel-variant selectors (internal, not in the public header).  A product build accepts only the keys whose values all
    # compute correct results; a key that names a timing ablation raises instead of silently corrupting outputs
    L.anoddpm_internal_variant.argtypes = [ctypes.c_int32, ctypes.c_int32]
    for i in range(16):
        if os.environ.get(f"ANODDPM_DEBUG{i}"):
            if L.anoddpm_internal_variant(i, int(os.environ[f"ANODDPM_DEBUG{i}"], 0)) != 0:
                raise AnoddpmError(f"ANODDPM_DEBUG{i} selects a timing ablation (wrong results by design): rebuild with "
                                   "ANODDPM_ABLATE=1 python -m anoddpm_amd.build --force to use it")
    _lib = L
    return L


def check(rc, what=""):
    if rc != 0:
        msg = lib().anoddpm_last_error()
        raise AnoddpmError(f"{what or 'anoddpm'} failed (code {rc}): {msg.decode(errors='replace') if msg else ''}")


def require_cuda(t, what):
    """The HIP path is the only path: refuse CPU tensors instead of silently computing elsewhere."""
    if not t.is_cuda:
        raise AnoddpmError(
            f"{what}: tensor is on '{t.device}', but anoddpm_amd runs on MI355X (HIP) devices only; "
            "there is no CPU fallback (the CPU restatement lives in oracle/ and is test-only).")
    return t


def current_stream():
    import torch
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return c_void_p(t.data_ptr()) if t is not None else c_void_p(0)
