"""The ctypes binding that core/_hip.py derives from include/danbo_hip.h, checked against the host compiler's reading of the same
header: struct layouts, constants and the type class of every parameter and result.  The compiler is the referee -- the lists of
functions and structs come from this file's own regexes, never from the parser, so a declaration the parser dropped fails here.
The same referee reads every satellite header of _hip.HEADERS (one row of SATELLITES each).  No GPU: the library is loaded (by the
satellites' test and the stale-library case), nothing is launched."""
import ctypes
import os
import re
import subprocess

import pytest

import raster_ref as rr
from core import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
with open(os.path.join(INCLUDE, "danbo_hip.h")) as _f:
    HEADER = _f.read()
BARE = re.sub(r"/\*.*?\*/", " ", HEADER, flags=re.S)


def declared_functions(text):
    """the entry points a header declares, by this file's own reading of its text"""
    return sorted(set(re.findall(r"^(?:int|size_t|long)\s+(danbo_\w+)\s*\(", text, flags=re.M)))


FUNCTIONS = declared_functions(HEADER)
STRUCT_BODIES = dict(re.findall(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}", BARE, flags=re.S))


def compile_and_run(tmp_path_factory, compiler, name, source):
    d = tmp_path_factory.mktemp("abi")
    src, exe = d / name, d / "probe"
    src.write_text(source)
    subprocess.check_call(compiler + ["-I", INCLUDE, "-o", str(exe), str(src)])
    return subprocess.check_output([str(exe)], text=True).splitlines()


# ------------------------------------------------------------------ layouts and constants
# CONST(NAME) prints `const NAME kind value` as the C compiler reads the constant (kind: i integer, f float, d double)
C_CONST = ['#include <stdio.h>', '#include <stddef.h>',
           '#define KIND(x) _Generic((x), float: "f", double: "d", int: "i", long: "i", long long: "i", unsigned: "i", '
           'unsigned long: "i", unsigned long long: "i")',
           '#define CONST(x) printf("const %s %s ", #x, KIND(x)); if (KIND(x)[0] == \'i\') printf("%lld\\n", (long long)(x)); '
           'else printf("%.17g\\n", (double)(x));']


@pytest.fixture(scope="module")
def c_view(tmp_path_factory):
    """what the host C compiler makes of the header: {("sizeof", S): n, ("field", S, f): (offset, size), ("const", NAME): (kind, text)}"""
    lines = ['#include "danbo_hip.h"'] + C_CONST + ['int main(void) {']
    for s, cls in _hip.STRUCTS.items():
        lines.append(f'printf("sizeof {s} %zu\\n", sizeof({s}));')
        lines += [f'printf("field {s} {f} %zu %zu\\n", offsetof({s}, {f}), sizeof((({s}*)0)->{f}));' for f, _ in cls._fields_]
    lines += [f"CONST({name})" for name in vars(_hip.C)]
    out = {}
    for line in compile_and_run(tmp_path_factory, ["cc", "-std=c11"], "layout.c", "\n".join(lines + ["return 0; }"])):
        w = line.split()
        if w[0] == "sizeof":
            out["sizeof", w[1]] = int(w[2])
        elif w[0] == "field":
            out["field", w[1], w[2]] = (int(w[3]), int(w[4]))
        else:
            out["const", w[1]] = (w[2], w[3])
    return out


def test_every_struct_of_the_header_is_bound_with_every_field():
    assert set(STRUCT_BODIES) == set(_hip.STRUCTS) and len(STRUCT_BODIES) == 13
    for s, body in STRUCT_BODIES.items():
        # every field statement ends in `;`, further declarators of a statement follow a `,`
        assert body.count(";") + body.count(",") == len(_hip.STRUCTS[s]._fields_), s
        assert getattr(_hip, s) is _hip.STRUCTS[s] and issubclass(_hip.STRUCTS[s], ctypes.Structure)


def test_struct_layouts_equal_the_host_compilers(c_view):
    n = 0
    for s, cls in _hip.STRUCTS.items():
        assert c_view[("sizeof", s)] == ctypes.sizeof(cls), s
        for f, _ in cls._fields_:
            d = getattr(cls, f)
            assert c_view[("field", s, f)] == (d.offset, d.size), (s, f)
            n += 1
    assert len([k for k in c_view if k[0] == "sizeof"]) == 13 and len([k for k in c_view if k[0] == "field"]) == n


def test_constants_equal_the_host_compilers(c_view):
    names = set(re.findall(r"^#define[ \t]+(DANBO_\w+)[ \t]+\S", BARE, flags=re.M))
    enum = re.search(r"enum\s+DanboTrainTensor\s*\{(.*?)\}", BARE, flags=re.S).group(1)
    names |= {item.split("=")[0].strip() for item in enum.split(",") if item.strip()}
    assert names == set(vars(_hip.C)) and len(names) == 52
    for name in names:
        kind, text = c_view[("const", name)]
        value = getattr(_hip.C, name)
        assert type(value) is (int if kind == "i" else float), (name, kind, value)
        assert value == (int(text) if kind == "i" else float(text)), (name, text, value)
    assert _hip.C.DANBO_T_COUNT == _hip.N_TRAIN_TENSORS == len(_hip.TRAIN_TENSORS) == 43
    assert _hip.C.DANBO_ABI_VERSION == 9 and _hip.C.DANBO_EINVAL == -22 and _hip.C.DANBO_RAY_FLAT_VMAX == 1e4
    assert _hip.MAX_ROW_SPANS == _hip.C.DANBO_MAX_ROW_SPANS and _hip.ANERF_MAX_D == _hip.C.DANBO_ANERF_MAX_D


# ------------------------------------------------------------------ signatures
# type classes: P pointer, i int, l long, q long long, z size_t, f float.  ctypes has one class for two C types of equal size
# (c_longlong is c_long where long has 64 bits), so a letter stands for every C type that shares its ctypes class.
_C_TYPES = dict(P=ctypes.c_void_p, i=ctypes.c_int, l=ctypes.c_long, q=ctypes.c_longlong, z=ctypes.c_size_t, f=ctypes.c_float)
_LETTER = {ctypes.c_char_p: "P"}
for _l, _t in _C_TYPES.items():
    _LETTER.setdefault(_t, _l)


def bound_letters(h, name):
    return _LETTER[h.restypes[name]] + ":" + "".join(_LETTER[t] for t in h.signatures[name])


def same_class(seen):
    """the compiler's letters with every C type replaced by the letter of its ctypes class"""
    return "".join(_LETTER[_C_TYPES[ch]] if ch in _C_TYPES else ch for ch in seen)


def compiled_signatures(tmp_path_factory, includes, names):
    """{name: "r:args"}: the type class of the result and of every parameter of each function, as a C++ compiler reads `includes`"""
    src = ['#include <cstdio>', '#include <cstddef>', '#include <type_traits>'] + [f'#include "{h}"' for h in includes] + [
           'template <class T> constexpr char letter() {',
           '    if constexpr (std::is_pointer_v<T>) return \'P\';',
           '    else if constexpr (std::is_same_v<T, int>) return \'i\';',
           '    else if constexpr (std::is_same_v<T, long>) return \'l\';',
           '    else if constexpr (std::is_same_v<T, long long>) return \'q\';',
           '    else if constexpr (std::is_same_v<T, size_t>) return \'z\';',
           '    else if constexpr (std::is_same_v<T, float>) return \'f\';',
           '    else return \'?\';',
           '}',
           'template <class F> struct Sig;',
           'template <class R, class... A> struct Sig<R(A...)> {',
           '    static void print(const char* name) {',
           '        const char args[] = {letter<A>()..., 0};',
           '        std::printf("%s %c:%s\\n", name, letter<R>(), args);',
           '    }',
           '};',
           'int main() {'] + [f'    Sig<decltype({n})>::print("{n}");' for n in names] + ['}']
    return dict(line.split() for line in compile_and_run(tmp_path_factory, ["g++", "-std=c++17"], "sig.cpp", "\n".join(src)))


def test_signatures_equal_the_host_compilers(tmp_path_factory):
    assert len(FUNCTIONS) == 104
    seen = compiled_signatures(tmp_path_factory, ["danbo_hip.h"], FUNCTIONS)
    assert set(seen) == set(FUNCTIONS) == set(_hip.SIGNATURES) == set(_hip.RESTYPES)
    for name in FUNCTIONS:
        assert "?" not in seen[name], (name, seen[name])
        bound = bound_letters(_hip.header("danbo_hip.h"), name)
        assert same_class(seen[name]) == bound, (name, seen[name], bound)


# ------------------------------------------------------------------ the satellite headers
# one row per header of _hip.HEADERS[1:]: its entry points as "result:parameters" letters (above), its constants, and the words by
# which the ABI history of danbo_hip.h names its entries
SATELLITES = {
    "danbo_raster.h": dict(functions={"danbo_raster_workspace_bytes": "z:iii", "danbo_raster_mesh": "i:PiPiPiPifiiPPPPPP"},
                           constants={"DANBO_RASTER_COLOR": rr.COLOR, "DANBO_RASTER_NORMAL": rr.NORMAL, "DANBO_RASTER_FLAT": rr.FLAT},
                           history="the rasteriser's entries are in danbo_raster.h"),
    "danbo_partmap.h": dict(functions={"danbo_part_colors_fwd": "i:PPPPiiiPPP", "danbo_composite_colors_fwd": "i:PPPPPPiiiPPPP"},
                            constants={}, history="danbo_part_colors_fwd, danbo_composite_colors_fwd"),
    "danbo_metrics.h": dict(functions={"danbo_image_metrics_workspace_bytes": "z:iii", "danbo_image_metrics": "i:PPPPPiiiPiPPPP"},
                            constants={}, history="danbo_image_metrics_workspace_bytes, danbo_image_metrics"),
    "danbo_cull.h": dict(functions={"danbo_bone_cull_rays": "i:PPPPPPPiiiPPPPPPiPPPP"},      # 21 parameters, the stream last
                         constants={}, history="danbo_bone_cull_rays"),
    "danbo_batch.h": dict(functions={"danbo_batch_gather": "i:PPPPPPPPPPPPiiiiPPPiiiPPPPPPPPPPPP"},      # 12 tables, 4 sizes, the draw
                          constants={}, history="danbo_batch_gather"),                 # (3 pointers, 3 ints), 11 outputs, the stream
    "danbo_grid_cc.h": dict(functions={"danbo_grid_cc_workspace_bytes": "z:iii", "danbo_grid_cc_label": "i:PiiillffPPPPP",
                                       "danbo_grid_cc_keep": "i:PiiillffPPPiifPllPP"},
                            constants={}, history="danbo_grid_cc_workspace_bytes, danbo_grid_cc_label, danbo_grid_cc_keep"),
    "danbo_skel.h": dict(functions={"danbo_skel_project": "i:PPPiPiiiPP", "danbo_skel_draw": "i:PiPPiiiiPP"},
                         constants={}, history="danbo_skel_project, danbo_skel_draw"),
    "danbo_depth.h": dict(functions={"danbo_depth_composite_fwd": "i:PPiifPPPPP", "danbo_depth_normals": "i:PPPPPiiiffifPPP"},
                          constants={}, history="danbo_depth_composite_fwd, danbo_depth_normals"),
}


def test_every_satellite_has_its_row():
    core = _hip.header("danbo_hip.h")
    assert _hip.HEADERS[0] == "danbo_hip.h" and core.path == _hip.HEADER_PATH
    assert core.signatures is _hip.SIGNATURES and core.restypes is _hip.RESTYPES and core.C is _hip.C
    assert set(_hip.HEADERS[1:]) == set(SATELLITES) and len(set(_hip.HEADERS)) == len(_hip.HEADERS)


@pytest.mark.parametrize("name", _hip.HEADERS[1:])
def test_satellite_header_as_the_host_compilers_read_it(name, tmp_path_factory):
    """a header beside danbo_hip.h: what it declares (by this file's regex, never the parser's tables) is what is bound, what the
    row pins and what the C and the C++ compiler read; the library exports every entry and lib() has set its types"""
    h, row = _hip.header(name), SATELLITES[name]
    assert os.path.basename(h.path) == name and os.path.dirname(h.path) == os.path.dirname(_hip.HEADER_PATH)
    with open(h.path) as f:
        text = f.read()
    functions = declared_functions(text)
    assert set(functions) == set(row["functions"]) == set(h.signatures) == set(h.restypes)
    parsed, structs, constants = _hip.parse_header(text)
    assert not structs and constants == row["constants"] == vars(h.C) and set(parsed) == set(functions)
    for other in _hip.HEADERS:                               # its names are its own
        o = _hip.header(other)
        if other != name:
            assert not set(h.signatures) & set(o.signatures) and not set(vars(h.C)) & set(vars(o.C)), other
    assert row["history"] in HEADER
    # the C compiler: the header alone, then beside danbo_hip.h, then a second time; every constant read back
    src = [f'#include "{name}"', '#include "danbo_hip.h"', f'#include "{name}"'] + C_CONST + ['int main(void) {']
    src += [f"CONST({c})" for c in row["constants"]] + ["return 0; }"]
    lines = compile_and_run(tmp_path_factory, ["cc", "-std=c11", "-Wall", "-Werror"], "const.c", "\n".join(src))
    assert {w[1]: (w[2], int(w[3])) for w in map(str.split, lines)} == {c: ("i", v) for c, v in row["constants"].items()}
    assert all(type(v) is int for v in vars(h.C).values())
    # the C++ compiler: the type class of every parameter and result
    seen = compiled_signatures(tmp_path_factory, [name, "danbo_hip.h", name], functions)
    assert set(seen) == set(functions)
    lib = _hip.lib()
    raw = ctypes.CDLL(lib._name)
    for fn, pinned in row["functions"].items():
        assert "?" not in seen[fn], (fn, seen[fn])
        assert seen[fn] == same_class(seen[fn]) == bound_letters(h, fn) == pinned, (fn, seen[fn], bound_letters(h, fn), pinned)
        restype, _, args = pinned.partition(":")
        assert h.restypes[fn] is _C_TYPES[restype] and h.signatures[fn] == [_C_TYPES[ch] for ch in args], fn
        assert hasattr(raw, fn), fn
        assert getattr(lib, fn).restype is h.restypes[fn] and getattr(lib, fn).argtypes == h.signatures[fn], fn
    assert lib.danbo_abi_version() == _hip.C.DANBO_ABI_VERSION == 9


CORE = "#define DANBO_N 8\nint danbo_f(int n);\ntypedef struct DanboS { int n; } DanboS;\n"
FIRST = "#define DANBO_FIRST 1\nsize_t danbo_first(const float* s);\n"


def bind(tmp_path, **texts):
    for name, text in texts.items():
        if text is not None:
            (tmp_path / f"{name}.h").write_text(text)
    return _hip.bind_headers([str(tmp_path / f"{name}.h") for name in texts])


def test_bind_headers_binds_each_header_into_tables_of_its_own(tmp_path):
    core, first, probe = bind(tmp_path, core=CORE, first=FIRST, danbo_probe="int danbo_probe(float x, void* stream);\n")
    assert core.signatures == {"danbo_f": [ctypes.c_int]} and vars(core.C) == {"DANBO_N": 8} and list(core.structs) == ["DanboS"]
    assert first.signatures == {"danbo_first": [ctypes.c_void_p]} and first.restypes == {"danbo_first": ctypes.c_size_t}
    assert vars(first.C) == {"DANBO_FIRST": 1} and not first.structs
    assert probe.signatures == {"danbo_probe": [ctypes.c_float, ctypes.c_void_p]} and probe.restypes == {"danbo_probe": ctypes.c_int}
    assert vars(probe.C) == {} and probe.path == str(tmp_path / "danbo_probe.h")
    # a tenth header beside the real nine, through the call that binds the table: no clash, and only its own names
    tenth = _hip.bind_headers([_hip.header(name).path for name in _hip.HEADERS] + [probe.path])[-1]
    assert tenth.signatures == probe.signatures and tenth.restypes == probe.restypes and vars(tenth.C) == {}


@pytest.mark.parametrize("text, error, quoted", [
    ("typedef struct DanboT { int a; } DanboT;", _hip.HeaderError, "struct DanboT"),      # a satellite with a struct
    ("int danbo_f(float x);", _hip.HeaderError, "danbo_f"),                               # a function of the core header
    ("#define DANBO_N 9", _hip.HeaderError, "DANBO_N"),                                   # a constant of the core header
    ("enum E { DANBO_FIRST };", _hip.HeaderError, "DANBO_FIRST"),                         # a constant of an earlier satellite
    ("int danbo_first(void);", _hip.HeaderError, "danbo_first"),                          # a function of an earlier satellite
    (None, RuntimeError, "not found"),                                                    # a missing file
], ids=["struct", "core_function", "core_constant", "satellite_constant", "satellite_function", "missing_file"])
def test_bind_headers_refuses_a_satellite_that_breaks_the_rule(tmp_path, text, error, quoted):
    with pytest.raises(error) as e:
        bind(tmp_path, core=CORE, first=FIRST, danbo_probe=text)
    assert "danbo_probe.h" in str(e.value) and quoted in str(e.value), str(e.value)


# ------------------------------------------------------------------ the parser on small headers
def test_parser_reads_the_constructs_the_header_uses():
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    fns, structs, consts = _hip.parse_header("""
        /* a header */
        #ifndef H
        #define H
        #include <stddef.h>
        #ifdef __cplusplus
        extern "C" {
        #endif
        #define N 8
        #define BYTES ((N + 2) * 4)   /* over an earlier one */
        #define NEG (-22)
        #define BIG 1e4f // a float
        enum E { A = 0, B, C = B + N, D, COUNT };
        typedef struct S {
            const float *a, *b /* second */;
            float* x[8];
            const void* y[COUNT];
            long long n, m;
            int k; float s;
            const uint8_t* const* pp;
        } S;
        int f(const float* a /* [n] */, int n, /* between */ long m, float s, size_t bytes, void* stream);
        size_t g(const S* s, char* name, const float* const* rows, long long big, uint32_t word);
        long h(void);
        int v(float v[3], int idx[]);
        #ifdef __cplusplus
        }
        #endif
        #endif
        """)
    assert consts == dict(N=8, BYTES=40, NEG=-22, BIG=1e4, A=0, B=1, C=9, D=10, COUNT=11)
    assert type(consts["BIG"]) is float and type(consts["BYTES"]) is int
    assert fns == dict(f=(I, [P, I, ctypes.c_long, F, ctypes.c_size_t, P]),
                       g=(ctypes.c_size_t, [P, ctypes.c_char_p, P, ctypes.c_longlong, ctypes.c_uint32]),
                       h=(ctypes.c_long, []), v=(I, [P, P]))
    assert structs == dict(S=[("a", P), ("b", P), ("x", P * 8), ("y", P * 11), ("n", ctypes.c_longlong), ("m", ctypes.c_longlong),
                              ("k", I), ("s", F), ("pp", P)])
    # a macro is replaced as text, as the preprocessor does it
    assert _hip.parse_header("#define A 1 + 2\n#define B A * 3\n")[2] == dict(A=3, B=7)
    assert _hip.parse_header("#define A 0.1f\n#define B 0.1\n")[2] == dict(A=ctypes.c_float(0.1).value, B=0.1)


@pytest.mark.parametrize("text, quoted", [
    ("int f(double x);", "double"),                                       # an unknown scalar type
    ("int f(unsigned int x);", "unsigned int x"),
    ("int f(const Unknown* p);", "Unknown"),
    ("int f(void (*cb)(int), int n);", "(*cb)"),                          # a function pointer
    ("typedef union U { int a; float b; } U;", "union"),
    ("typedef struct S { union { int a; float b; } u; } S;", "union"),
    ("typedef struct S { int a : 3; } S;", "a : 3"),                      # a bit-field
    ("typedef struct S { double d; } S;", "double"),
    ("typedef struct S { int a[M]; } S;", "M"),
    ("typedef struct S { int a; } T;", "'S' / 'T'"),
    ("float f(int x);", "float f"),                                       # a prototype returning something else
    ("void f(int x);", "void f"),
    ("const char* f(void);", "const char"),
    ("int f(int x); stray", "stray"),                                     # text left over
    ("int f(int x) stray;", "stray"),
    ("int f(int x); int f(int y);", "twice"),
    ("static inline int f(int x) { return x; }", "inline"),
    ("#define SQR(x) ((x) * (x))", "SQR"),
    ("#define A B", "'B'"),                                               # not defined above it
    ("#define A 1 / 2", "1 / 2"),
    ("#define A 1\n#define A 2", "twice"),
    ("#if 0\nint f(int x);\n#endif", "#if 0"),
    ("#ifdef X\nint f(int x);\n#endif", "#ifdef X"),
    ("#ifndef H\n#define H\nint f(int x);", "never closed"),
    ("#ifdef __cplusplus\nint f(int x);\n#endif", "int f(int x);"),
    ("enum E { A = 1, A };", "'A'"),
    ("int f(int x); /* open", "comment"),
])
def test_parser_refuses_what_it_does_not_understand(text, quoted):
    with pytest.raises(_hip.HeaderError) as e:
        _hip.parse_header(text)
    assert quoted in str(e.value), str(e.value)


def test_a_library_of_another_abi_version_is_refused(monkeypatch):
    monkeypatch.setattr(_hip, "_lib", None)
    monkeypatch.setattr(_hip.C, "DANBO_ABI_VERSION", 10)
    with pytest.raises(RuntimeError, match="ABI version 9.*declares 10.*stale"):
        _hip.lib()
    assert _hip._lib is None


def test_a_library_that_lacks_a_declared_entry_is_refused(monkeypatch):
    """a library built before a header of the table gained an entry has the same ABI version: lib() names what is missing"""
    h = _hip.header("danbo_depth.h")
    monkeypatch.setattr(_hip, "_lib", None)
    monkeypatch.setitem(h.signatures, "danbo_not_there", [ctypes.c_float, ctypes.c_void_p])
    monkeypatch.setitem(h.restypes, "danbo_not_there", ctypes.c_int)
    with pytest.raises(RuntimeError, match=r"has no danbo_not_there, which \S*danbo_depth\.h declares.*stale, rebuild it with `make -C"):
        _hip.lib()
    assert _hip._lib is None
