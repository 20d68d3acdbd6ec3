"""The ctypes binding that core/_hip.py derives from include/danbo_hip.h, checked against the host compiler's reading of the same
header: struct layouts, constants and the type class of every parameter and result.  The compiler is the referee -- the lists of
functions and structs come from this file's own regexes, never from the parser, so a declaration the parser dropped fails here.
No GPU: the library is not even loaded, except by the stale-library case."""
import ctypes
import os
import re
import subprocess

import pytest

from core import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
with open(os.path.join(INCLUDE, "danbo_hip.h")) as _f:
    HEADER = _f.read()
BARE = re.sub(r"/\*.*?\*/", " ", HEADER, flags=re.S)
FUNCTIONS = sorted(set(re.findall(r"^(?:int|size_t|long)\s+(danbo_\w+)\s*\(", HEADER, flags=re.M)))
STRUCT_BODIES = dict(re.findall(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}", BARE, flags=re.S))


def compile_and_run(tmp_path_factory, compiler, name, source):
    d = tmp_path_factory.mktemp("abi")
    src, exe = d / name, d / "probe"
    src.write_text(source)
    subprocess.check_call(compiler + ["-I", INCLUDE, "-o", str(exe), str(src)])
    return subprocess.check_output([str(exe)], text=True).splitlines()


# ------------------------------------------------------------------ layouts and constants
@pytest.fixture(scope="module")
def c_view(tmp_path_factory):
    """what the host C compiler makes of the header: {("sizeof", S): n, ("field", S, f): (offset, size), ("const", NAME): (kind, text)}"""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "danbo_hip.h"',
             '#define KIND(x) _Generic((x), float: "f", double: "d", int: "i", long: "i", long long: "i", unsigned: "i", '
             'unsigned long: "i", unsigned long long: "i")',
             '#define CONST(x) printf("const %s %s ", #x, KIND(x)); if (KIND(x)[0] == \'i\') printf("%lld\\n", (long long)(x)); '
             'else printf("%.17g\\n", (double)(x));',
             'int main(void) {']
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


def test_signatures_equal_the_host_compilers(tmp_path_factory):
    assert len(FUNCTIONS) == 104
    src = ['#include <cstdio>', '#include <cstddef>', '#include <type_traits>', '#include "danbo_hip.h"',
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
           'int main() {'] + [f'    Sig<decltype({n})>::print("{n}");' for n in FUNCTIONS] + ['}']
    seen = dict(line.split() for line in compile_and_run(tmp_path_factory, ["g++", "-std=c++17"], "sig.cpp", "\n".join(src)))
    assert set(seen) == set(FUNCTIONS) == set(_hip.SIGNATURES) == set(_hip.RESTYPES)
    for name in FUNCTIONS:
        assert "?" not in seen[name], (name, seen[name])
        bound = _LETTER[_hip.RESTYPES[name]] + ":" + "".join(_LETTER[t] for t in _hip.SIGNATURES[name])
        assert "".join(_LETTER[_C_TYPES[ch]] if ch in _C_TYPES else ch for ch in seen[name]) == bound, (name, seen[name], bound)


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
