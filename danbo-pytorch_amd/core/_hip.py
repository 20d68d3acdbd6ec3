"""ctypes binding of libdanbo_hip.so, derived from include/danbo_hip.h when this module is imported.

The header is the only statement of the C ABI.  `parse_header` reads the subset of C it is written in (stated at the top of the
header) and this module builds from it, with nothing typed a second time:
  SIGNATURES / RESTYPES   name -> argtypes / restype of every entry point, set on the library by `lib()`
  the struct classes      one `ctypes.Structure` per `typedef struct`, under the header's name (DanboModel, DanboDwLayer, ...)
  C                       every numeric `#define` and enumerator under the header's name (C.DANBO_J, C.DANBO_T_COUNT, ...)
Every pointer, whatever it points to, is a `c_void_p` (`char*`: `c_char_p`): a parameter takes None, an address, `ptr(tensor)`,
`ctypes.byref(x)` or a ctypes array.  A construct the parser does not know raises HeaderError at import and quotes the text; nothing
is skipped.  A new entry point needs its declaration in the header and its implementation, and is then callable as
`call("danbo_x", ...)`; a wrapper in hip_ops is optional.

The header is $DANBO_HIP_HEADER, else danbo_hip.h beside the library, else include/danbo_hip.h of the source tree.  SIGNATURES,
RESTYPES, STRUCTS and C are the statement of danbo_hip.h alone.  The entry points of a later feature stand in a header of their own
beside it (a satellite), bound the same way and reached as `header("danbo_x.h").signatures / .restypes / .C / .path`: a satellite
declares no struct, and no function or constant that an earlier header declares.  A new header is named in HEADERS, nowhere else.
`lib()` sets the types of every entry of every header of HEADERS and refuses a stale build: a library whose danbo_abi_version() is
not the header's DANBO_ABI_VERSION, or one that lacks an entry a header declares.

The library is the only compute backend of this package: there is NO PyTorch/CPU fallback.  `lib()` raises if the shared object is
missing, and every wrapper in hip_ops raises if a tensor is not a CUDA(HIP) tensor.
"""
import ctypes
import os
import re
from ctypes import c_char_p, c_float, c_int, c_void_p
from types import SimpleNamespace

import torch  # (before the library is opened: torch's bundled libamdhip64 is loaded first, so both share one HIP runtime)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DANBO_HIP_LIB") or os.path.join(os.path.dirname(_HERE), "libdanbo_hip.so")

P = c_void_p  # device pointer
I = c_int
F = c_float


class HeaderError(ValueError):
    """include/danbo_hip.h left the subset of C that parse_header reads"""


_SCALARS = {"int": c_int, "long": ctypes.c_long, "long long": ctypes.c_longlong, "size_t": ctypes.c_size_t, "float": c_float,
            **{f"{u}int{n}_t": getattr(ctypes, f"c_{u}int{n}") for u in ("", "u") for n in (8, 16, 32, 64)}}
_TAIL = r"((?:\*\s*(?:const\b\s*)?)*)(\w+)\s*(?:\[\s*(\w*)\s*\])?$"          # `* const* name[N]` -> stars, name, array length
_DECL = re.compile(r"(?:const\s+)?(long\s+long|\w+)\b\s*" + _TAIL)        # `const T* const* name[N]` -> T, stars, name, array length
_MORE = re.compile(_TAIL)                                                 # the further declarators of `T *a, *b`
_PROTO = re.compile(r"(int|long|size_t)\s+(\w+)\s*\((.*)\)$", re.S)
_STRUCT = re.compile(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)$", re.S)
_ENUM = re.compile(r"enum\s+\w+\s*\{([^{}]*)\}$", re.S)
_TOKEN = re.compile(r"\s*(?:(0[xX][0-9a-fA-F]+|\d+)[uUlL]*(?![\w.])|((?:\d+\.\d*|\.\d+|\d+)(?:[eE][-+]?\d+)?)([fF]?)(?![\w.])"
                    r"|([A-Za-z_]\w*)|(<<|>>|[-+*()|&~]))")


def _expr(expr, sources):
    """a constant expression of C as Python source: integer / float literals, + - * << >> | & ~, parentheses, and the names in
    `sources` replaced by their text as the preprocessor replaces a macro"""
    out, pos = [], 0
    while pos < len(expr.rstrip()):
        m = _TOKEN.match(expr, pos)
        if not m:
            raise HeaderError(f"constant expression not understood: {expr.strip()!r}")
        integer, real, f32, name, op = m.groups()
        if name is not None and name not in sources:
            raise HeaderError(f"{name!r} in {expr.strip()!r} is not a constant defined above it")
        out.append(repr(int(integer, 0)) if integer else repr(c_float(float(real)).value if f32 else float(real)) if real
                   else sources[name] if name else op)
        pos = m.end()
    return " ".join(out)


def _value(source, text):
    try:
        return eval(source, {"__builtins__": {}})     # literals and operators only: _expr matched every token
    except Exception:
        raise HeaderError(f"constant expression not understood: {text.strip()!r}") from None


def _ctype(base, stars, structs, text):
    base = " ".join(base.split())
    if stars:
        if base not in _SCALARS and base not in structs and base not in ("void", "char"):
            raise HeaderError(f"unknown type {base!r} in {text!r}")
        return c_char_p if base == "char" and stars.count("*") == 1 else c_void_p
    if base not in _SCALARS:
        raise HeaderError(f"unknown scalar type {base!r} in {text!r}")
    return _SCALARS[base]


def _fields(body, constants, structs):
    """`const float *a, *b; int n; T* p[8];` -> [(name, ctype)]"""
    fields = []
    for stmt in filter(None, (s.strip() for s in body.split(";"))):
        first, *more = (d.strip() for d in stmt.split(","))
        matches = [_DECL.match(first)] + [_MORE.match(d) for d in more]
        if None in matches:
            raise HeaderError(f"struct field not understood: {stmt!r}")
        for m in matches:
            stars, name, n = m.groups()[-3:]
            t = _ctype(matches[0].group(1), stars, structs, stmt)
            if n is not None:
                if n not in constants and not n.isdigit():
                    raise HeaderError(f"array length {n!r} in {stmt!r} is not a constant defined above it")
                t = t * int(constants.get(n, n))
            fields.append((name, t))
    return fields


def _params(text, structs):
    types = []
    for p in (p.strip() for p in text.split(",") if text.strip() not in ("", "void")):
        m = _DECL.match(p)
        if not m:
            raise HeaderError(f"parameter not understood: {p!r}")
        base, stars, _, n = m.groups()
        t = _ctype(base, stars, structs, p)
        types.append(t if n is None else c_void_p)       # `T x[N]`, `T x[]`: a pointer
    return types


def parse_header(text):
    """-> (functions {name: (restype, [argtypes])}, structs {name: [(field, ctype)]}, constants {name: int | float}) of a header
    written in the subset of C that include/danbo_hip.h states at its top; raises HeaderError on anything else."""
    functions, structs, constants, sources = {}, {}, {}, {}
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    if "/*" in text or "*/" in text or "\\\n" in text:
        raise HeaderError("unterminated comment or continued line")
    code, guard, open_ifs = [], None, []
    for line in text.split("\n"):
        s = line.strip()
        if not s.startswith("#"):
            if "__cplusplus" not in open_ifs:
                code.append(line)
            elif s not in ("", 'extern "C" {', "}"):
                raise HeaderError(f"only the extern \"C\" guard may stand under #ifdef __cplusplus: {s!r}")
            continue
        word, rest = re.match(r"#\s*(\w*)\s*(.*)$", s).groups()
        if word == "include" and re.match(r"<\w+\.h>$", rest):
            pass
        elif word == "ifndef" and guard is None and re.match(r"\w+$", rest):        # the include guard, once
            guard = rest
            open_ifs.append(rest)
        elif word == "ifdef" and rest == "__cplusplus":
            open_ifs.append(rest)
        elif word == "endif" and not rest and open_ifs:
            open_ifs.pop()
        elif word == "define" and rest == guard:
            pass
        elif word == "define" and re.match(r"\w+\s+\S", rest):
            name, expr = rest.split(None, 1)
            if name in constants:
                raise HeaderError(f"{name} is defined twice")
            sources[name] = _expr(expr, sources)
            constants[name] = _value(sources[name], s)
        else:
            raise HeaderError(f"preprocessor line not understood: {s!r}")
    if open_ifs:
        raise HeaderError(f"the #if of {open_ifs[-1]} is never closed")

    decl, depth = [], 0
    for piece in re.split(r"([;{}])", "\n".join(code)):
        depth += (piece == "{") - (piece == "}")
        if piece != ";" or depth:
            decl.append(piece)
            continue
        d = "".join(decl).strip()
        decl = []
        if m := _PROTO.match(d):
            restype, name, params = m.groups()
            if name in functions:
                raise HeaderError(f"{name} is declared twice")
            functions[name] = (_SCALARS[restype], _params(params, structs))
        elif m := _STRUCT.match(d):
            if m.group(1) != m.group(3) or m.group(1) in structs:
                raise HeaderError(f"struct tag and typedef name differ, or the struct is declared twice: {m.group(1)!r} / {m.group(3)!r}")
            structs[m.group(1)] = _fields(m.group(2), constants, structs)
        elif m := _ENUM.match(d):
            nxt = 0
            for item in filter(None, (e.strip() for e in m.group(1).split(","))):
                name, _, expr = (x.strip() for x in item.partition("="))
                if not re.match(r"[A-Za-z_]\w*$", name) or name in constants:
                    raise HeaderError(f"enumerator not understood, or defined twice: {item!r}")
                constants[name] = nxt = _value(_expr(expr, sources), item) if expr else nxt
                sources[name] = repr(nxt)
                nxt += 1
        else:
            raise HeaderError(f"declaration not understood: {d!r}")
    if "".join(decl).strip():
        raise HeaderError(f"text left over after the last declaration: {''.join(decl).strip()!r}")
    return functions, structs, constants


def _header_path():
    env = os.environ.get("DANBO_HIP_HEADER")
    tried = [env] if env else [os.path.join(os.path.dirname(LIB_PATH), "danbo_hip.h"),
                               os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "danbo_hip.h")]
    for p in tried:
        if os.path.exists(p):
            return p
    raise RuntimeError("danbo_hip.h not found (the ctypes binding is derived from it): tried " + ", ".join(tried)
                       + "; set DANBO_HIP_HEADER or put the header beside the library")


HEADERS = ("danbo_hip.h", "danbo_raster.h", "danbo_partmap.h", "danbo_metrics.h", "danbo_cull.h", "danbo_batch.h", "danbo_grid_cc.h",
           "danbo_skel.h", "danbo_depth.h")                                     # the core header, then the satellites


def bind_headers(paths):
    """-> one namespace (path, signatures, restypes, structs, C) per header file of `paths`, the core header first.  Every later one
    is a satellite: HeaderError if it declares a struct, or a function or constant that a header before it declares."""
    bound, owner = [], {}
    for path in paths:
        if not os.path.exists(path):
            raise RuntimeError(f"{path} not found (the binding of its entry points is derived from it, it lies beside {HEADERS[0]})")
        with open(path) as f:
            functions, structs, constants = parse_header(f.read())
        if bound:
            if structs:
                raise HeaderError(f"{path} declares struct {next(iter(structs))}: only {bound[0].path} declares structs")
            for name in (*functions, *constants):
                if name in owner:
                    raise HeaderError(f"{path} declares {name}, which {owner[name]} declares")
        owner.update(dict.fromkeys((*functions, *constants), path))
        bound.append(SimpleNamespace(path=path, signatures={name: argtypes for name, (_, argtypes) in functions.items()},
                                     restypes={name: restype for name, (restype, _) in functions.items()},
                                     structs=structs, C=SimpleNamespace(**constants)))
    return bound


HEADER_PATH = _header_path()
_BOUND = dict(zip(HEADERS, bind_headers([HEADER_PATH] + [os.path.join(os.path.dirname(HEADER_PATH), h) for h in HEADERS[1:]])))


def header(name):
    """what one of HEADERS declares: .path, .signatures {name: argtypes}, .restypes {name: restype}, .C (its constants)"""
    return _BOUND[name]


_core = header(HEADERS[0])
SIGNATURES, RESTYPES, C = _core.signatures, _core.restypes, _core.C
STRUCTS = {name: type(name, (ctypes.Structure,), {"_fields_": fields, "__doc__": f"struct {name} of include/danbo_hip.h"})
           for name, fields in _core.structs.items()}
globals().update(STRUCTS)              # _hip.DanboModel, _hip.DanboDwLayer, ...
MAX_ROW_SPANS = C.DANBO_MAX_ROW_SPANS
ANERF_MAX_D = C.DANBO_ANERF_MAX_D

# ---- training step: the state_dict key of every slot of DanboTrainModel.p / .g (enum DanboTrainTensor; the names are Python's)
TRAIN_TENSORS = (
    ["graph_net.layers.0.lin.weight", "graph_net.layers.0.adj_w", "graph_net.layers.0.bias", "graph_net.layers.1.lin.weight",
     "graph_net.layers.1.adj_w", "graph_net.layers.1.bias", "graph_net.layers.2.weight", "graph_net.layers.2.bias",
     "graph_net.layers.3.weight", "graph_net.layers.3.bias", "graph_net.axis_scale",
     "prob_linears.layers.0.lin.weight", "prob_linears.layers.0.adj_w", "prob_linears.layers.0.bias", "prob_linears.layers.1.weight",
     "prob_linears.layers.1.bias", "prob_linears.layers.2.weight", "prob_linears.layers.2.bias"]
    + [f"pts_linears.{i}.weight" for i in range(8)] + [f"pts_linears.{i}.bias" for i in range(8)]
    + ["alpha_linear.weight", "alpha_linear.bias", "feature_linear.weight", "feature_linear.bias", "views_linears.0.weight",
       "views_linears.0.bias", "rgb_linear.weight", "rgb_linear.bias", "framecodes.codes.weight"])
N_TRAIN_TENSORS = C.DANBO_T_COUNT
_anchors = {"graph_net.axis_scale": C.DANBO_T_AXIS_SCALE, "prob_linears.layers.0.lin.weight": C.DANBO_T_A_W0,
            "pts_linears.0.weight": C.DANBO_T_PTS_W0, "pts_linears.0.bias": C.DANBO_T_PTS_B0, "alpha_linear.weight": C.DANBO_T_ALPHA_W,
            "framecodes.codes.weight": C.DANBO_T_CODES}
if len(TRAIN_TENSORS) != N_TRAIN_TENSORS or any(TRAIN_TENSORS.index(k) != i for k, i in _anchors.items()):
    raise HeaderError(f"TRAIN_TENSORS does not line up with enum DanboTrainTensor of {HEADER_PATH}")

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build it with `make -C danbo-pytorch_amd/csrc` "
                "(or __graft_entry__.build()).  There is no CPU / PyTorch fallback.")
        l = ctypes.CDLL(LIB_PATH)
        # the version first: a library of an older ABI lacks entries too, and the version says more (`int f(void)` needs no types set)
        if l.danbo_abi_version() != C.DANBO_ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH} has ABI version {l.danbo_abi_version()}, {HEADER_PATH} declares {C.DANBO_ABI_VERSION}: "
                               "the library is stale, rebuild it with `make -C danbo-pytorch_amd/csrc`")
        for h in _BOUND.values():
            for name, argtypes in h.signatures.items():
                fn = getattr(l, name, None)
                if fn is None:
                    raise RuntimeError(f"{LIB_PATH} has no {name}, which {h.path} declares: "
                                       "the library is stale, rebuild it with `make -C danbo-pytorch_amd/csrc`")
                fn.argtypes = argtypes
                fn.restype = h.restypes[name]
        _lib = l
    return _lib


def ptr(t):
    """device pointer argument of a tensor (None -> NULL)"""
    return None if t is None else c_void_p(t.data_ptr())


def stream():
    """the current HIP stream as the `void* stream` argument every entry point ends in"""
    return c_void_p(torch.cuda.current_stream().cuda_stream)


class HipError(RuntimeError):
    pass


def check(code, name):
    if code != 0:
        raise HipError(f"{name} failed with code {code}" + (" (invalid argument)" if code == C.DANBO_EINVAL else ""))


def call(name, *args):
    """one entry point that returns a status: raises HipError unless it is 0"""
    check(getattr(lib(), name)(*args), name)
