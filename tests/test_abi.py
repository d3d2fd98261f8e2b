"""CPU: the C-ABI library builds, loads, and exports every symbol include/gank.h declares, and the ctypes binding that
_lib derives from that header binds exactly that set, types it by the stated rules, refuses what it cannot read and lays the
descriptor structs out as the compiler does.  No compute calls -- there is no GPU here."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    src = open(os.path.join(ROOT, "include", "gank.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gank_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_header_symbol():
    from gan_lib_tensorflow_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    syms = header_symbols()
    assert len(syms) >= 40
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in gank.h but not exported"
    assert sorted(_lib.PROTOTYPES) == syms, set(_lib.PROTOTYPES) ^ set(syms)
    assert lib.gank_version() == 100


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "gan_lib_tensorflow_amd")
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                text = open(os.path.join(d, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M), os.path.join(d, f)


def test_compute_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from gan_lib_tensorflow_amd import kernels as K
    x = torch.zeros(8, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        K.relu_fwd(x)


def test_entry_points_reject_bad_arguments_with_a_message():
    """Error behaviour of the C ABI: a non-zero return and a gank_last_error() message, decided on the host before
    anything is launched (so this runs without a GPU): null pointers, empty tables, unsupported shapes."""
    from gan_lib_tensorflow_amd import _lib
    lib = _lib.load()
    P = C.c_void_p
    fake = P(0x1000)      # never dereferenced: every call below is refused by argument checks

    def err():
        return lib.gank_last_error().decode()

    assert lib.gank_conv2d_fprop(None, None, None, None, None, None, 1, 8, 8, 64, 64, 3, 0, C.c_float(1.0), None) != 0
    assert "null pointer" in err()
    assert lib.gank_conv2d_fprop(fake, fake, None, None, None, fake, 1, 8, 8, 64, 64, 2, 0, C.c_float(1.0), None) != 0
    assert "even filter sizes" in err()
    assert lib.gank_conv2d_fprop(fake, fake, None, None, None, fake, 1, 7, 7, 64, 64, 3, 1, C.c_float(1.0), None) != 0   # IN_UPSAMPLE2X, odd size
    assert "even output size" in err()
    assert lib.gank_conv2d_fprop(fake, fake, None, None, None, fake, 1, 8, 8, 64, 64, 3, 64, C.c_float(1.0), None) != 0  # RES_UPSAMPLE2X without residual
    assert "needs a residual" in err()
    assert lib.gank_conv2d_wgrad(fake, fake, fake, None, None, 0, 1, 8, 8, 64, 64, 4, 0, C.c_float(1.0), None) != 0
    assert "even filter sizes" in err()
    assert lib.gank_sn_power_iter_fwd(None, 0, None) != 0 and "empty table" in err()
    assert lib.gank_conv2d_prep_weights_batched(None, 0, None) != 0 and "empty table" in err()
    desc = (_lib.PrepDesc * 1)()
    desc[0].w, desc[0].wf, desc[0].wd = 0x1000, 0x1000, 0x1000
    desc[0].ksize, desc[0].Cin, desc[0].Cout, desc[0].kind = 1, 64, 64, 2        # kind 2 needs ksize 3
    assert lib.gank_conv2d_prep_weights_batched(desc, 1, None) != 0 and "kind 2" in err()
    assert lib.gank_cbn_fwd(fake, fake, fake, fake, fake, fake, fake, 4, 16, 12, 1, 10, 0, None) != 0          # C = 12
    assert "unsupported" in err()
    assert lib.gank_convpool3x3_dgrad(fake, fake, None, fake, 1, 8, 8, 128, 32, None) != 0
    assert "multiple of 64" in err()
    assert lib.gank_linear_bwd(fake, None, None, fake, None, None, 4, 8, 8, None) != 0 and "dx needs w" in err()
    assert lib.gank_copy_bytes(fake, fake, 0, None) != 0 and "bad arguments" in err()
    assert lib.gank_copy_bytes_gather(fake, fake, 17, 16, None) != 0 and "1..16 sources" in err()
    assert lib.gank_conv2d_wgrad_batched(None, 0, 1, 8, 8, 128, 128, 3, 0, C.c_float(1.0), None) != 0 and "empty list" in err()


# ---- the reader itself (_lib.parse_header), on header text written here ------------------------------------------------------
@pytest.mark.parametrize("symbol,text", [
    ("gank_a", "int gank_ok(int n);\nint gank_a(void* p, unsigned n);"),                     # an unknown scalar type
    ("gank_a", "int gank_ok(int n);\nint gank_a(void* p, short n, void* stream);"),
    ("gank_a", "int gank_a(long long);"),                                                    # no name: not `long` called long
    ("gank_a", "int gank_a(void* p, int n)\nint gank_b(int n);"),                            # a declaration without `;`
    ("gank_b", "int gank_a(void* p, int n);\nint gank_b(int n)\n"),                          # ... at the end of the file
    ("gank_b", '#ifdef __cplusplus\nextern "C" {\n#endif\nint gank_b(int n)\n#ifdef __cplusplus\n}\n#endif\n'),
    ("gank_t", "typedef struct gank_t { void* p; size_t n; } gank_t;\nint gank_a(const gank_t* t);"),   # an unknown field type
    ("gank_t", "typedef struct gank_t { void* p; float w[4]; } gank_t;"),
    ("gank_a", "float gank_a(int n);"),                                                      # a return type outside the rules
    ("gank_a", "int gank_a(int n);\nint gank_a(int n);"),                                    # declared twice
    ("GANK_FLAG", "#define GANK_FLAG (1 << 3)\nint gank_a(int n);"),                         # a constant that is no integer literal
])
def test_reader_refuses_what_it_cannot_type_and_names_it(symbol, text):
    from gan_lib_tensorflow_amd import _lib
    with pytest.raises(RuntimeError, match=rf"gank\.h: {symbol}:"):
        _lib.parse_header(text)


def test_reader_details():
    from gan_lib_tensorflow_amd import _lib
    defines, structs, protos, rets = _lib.parse_header('''
        /* a comment that declares int gank_not_this(int n); */
        #ifndef GANK_H
        #define GANK_H
        #define GANK_VERSION 7   /* trailing comment */
        #define GANK_FLAG 0x20   // another
        #ifdef __cplusplus
        extern "C" {
        #endif
        typedef struct gank_two_words {
          const float* w;   /* [k,k,Cin,Cout] */
          void *wf, *wd;
          int ksize, Cin, Cout;   // three in one line
          long n; float scale; double eps; int64_t t; long long m;
          const void* const* rows;
        } gank_two_words;
        const char* gank_name(void);
        long gank_elems(int n);
        double gank_ms(void);
        int gank_call(const void* const* rows, const gank_two_words* one, gank_two_words* many, gank_two_words** table, const int32_t* labels,
                      char* out, int* produced, double a, float b, long c, long long d, int64_t e, const int f,
                      void* stream);
        #ifdef __cplusplus
        }
        #endif
        #endif
        ''')
    assert defines == {"GANK_VERSION": 7, "GANK_FLAG": 32}
    assert list(structs) == ["gank_two_words"]
    s = structs["gank_two_words"]
    assert s.__name__ == "TwoWords" and issubclass(s, C.Structure)
    P = C.c_void_p
    assert s._fields_ == [("w", P), ("wf", P), ("wd", P), ("ksize", C.c_int), ("Cin", C.c_int), ("Cout", C.c_int), ("n", C.c_long),
                          ("scale", C.c_float), ("eps", C.c_double), ("t", C.c_int64), ("m", C.c_longlong), ("rows", P)]
    assert list(protos) == ["gank_name", "gank_elems", "gank_ms", "gank_call"]
    assert protos["gank_name"] == [] and rets["gank_name"] is C.c_char_p
    assert protos["gank_elems"] == [C.c_int] and rets["gank_elems"] is C.c_long
    assert protos["gank_ms"] == [] and rets["gank_ms"] is C.c_double
    assert rets["gank_call"] is C.c_int
    assert protos["gank_call"] == [P, C.POINTER(s), C.POINTER(s), P, P, P, P, C.c_double, C.c_float, C.c_long, C.c_longlong, C.c_int64,
                                   C.c_int, P]


def test_binding_reads_every_declaration_of_the_header():
    from gan_lib_tensorflow_amd import _lib
    src = re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(_lib.HEADER).read(), flags=re.S)
    tokens = re.findall(r"\bgank_[a-z0-9_]+\s*\(", src)
    assert len(tokens) == len(_lib.PROTOTYPES) == len(_lib.RESTYPES) >= 200
    assert len(re.findall(r"\btypedef\s+struct\b", src)) == len(_lib.STRUCTS)
    assert {c.__name__ for c in _lib.STRUCTS.values()} >= {"CriticFeedDesc", "LabelDenseDesc", "PrepDesc", "Res8Head", "SlabJob", "SnDesc", "WgradItem"}
    for c in _lib.STRUCTS.values():
        assert getattr(_lib, c.__name__) is c
    flags = {k: getattr(_lib, k) for k in ("IN_UPSAMPLE2X", "IN_RELU", "OUT_TANH", "DY_UPSAMPLE2X", "RES_UPSAMPLE2X", "STATS_PREZEROED",
                                           "OUT_POOLSUM2X", "STAT_SLOTS", "VERSION")}
    assert flags == {"IN_UPSAMPLE2X": 1, "IN_RELU": 2, "OUT_TANH": 4, "DY_UPSAMPLE2X": 8, "RES_UPSAMPLE2X": 64, "STATS_PREZEROED": 256,
                     "OUT_POOLSUM2X": 512, "STAT_SLOTS": 16, "VERSION": 100}, flags
    assert len(re.findall(r"^[ \t]*#[ \t]*define[ \t]+GANK_\w+[ \t]+\S", src, flags=re.M)) == len(_lib.DEFINES)     # (GANK_H has no value)


def test_hard_cases_of_the_header_bind_as_declared():
    from gan_lib_tensorflow_amd import _lib
    A, R, P, I = _lib.PROTOTYPES, _lib.RESTYPES, C.c_void_p, C.c_int
    assert A["gank_kid_block_sums"] == [P, I, P, I, I, P, P, I, I, C.c_double, C.c_double, I, P, P]
    assert A["gank_inception_score_update"] == [P, I, I, C.c_longlong, C.c_longlong, I, P, P, P]
    assert A["gank_counter_add"] == [P, C.c_int64, P]
    assert A["gank_prof_calibrate"] == [I, P] and R["gank_prof_calibrate"] is C.c_double
    assert A["gank_swd_sort_ws_elems"] == [I, I] and R["gank_swd_sort_ws_elems"] is C.c_long
    assert R["gank_last_error"] is C.c_char_p and R["gank_conv2d_fprop"] is I
    assert A["gank_conv2d_fprop"] == [P] * 6 + [I] * 7 + [C.c_float, P]
    # a pointer to a descriptor keeps its kind; every other pointer, pointers to pointers included, is an address
    assert A["gank_sum_slabs"] == [C.POINTER(_lib.SlabJob), I, P]
    assert A["gank_res8_chain_bwd_head"][0] == C.POINTER(_lib.Res8Head) and A["gank_res8_chain_fwd"][1:5] == [P] * 4
    assert A["gank_sn_power_iter_fwd_prep"] == [C.POINTER(_lib.SnDesc), I, C.POINTER(_lib.PrepDesc), P, I, C.POINTER(_lib.LabelDenseDesc), P]
    lib = _lib.load()
    assert lib.gank_conv2d_fprop.argtypes == A["gank_conv2d_fprop"] and lib.gank_swd_sort_ws_elems.restype is C.c_long
    with pytest.raises(C.ArgumentError):
        lib.gank_sum_slabs((_lib.PrepDesc * 1)(), 1, None)       # the wrong descriptor kind never reaches the library


def test_struct_layouts_match_the_compiler(tmp_path):
    """sizeof of every descriptor struct and offsetof of every field, as ctypes lays the DERIVED classes out, asserted by the
    compiler that builds the library on a translation unit that includes gank.h: ties the parse to what C++ sees, padding included."""
    from gan_lib_tensorflow_amd import _lib, build
    lines = ["#include <cstddef>", '#include "gank.h"']
    for cname, cls in _lib.STRUCTS.items():
        lines.append(f'static_assert(sizeof({cname}) == {C.sizeof(cls)}, "sizeof {cname}");')
        for field, _ in cls._fields_:
            lines.append(f'static_assert(offsetof({cname}, {field}) == {getattr(cls, field).offset}, "offsetof {cname}.{field}");')
            lines.append(f'static_assert(sizeof((({cname}*)0)->{field}) == {getattr(cls, field).size}, "sizeof {cname}.{field}");')
    assert len(lines) == 2 + len(_lib.STRUCTS) + 2 * sum(len(c._fields_) for c in _lib.STRUCTS.values()) and len(lines) > 130
    unit = tmp_path / "gank_layout.cpp"
    unit.write_text("\n".join(lines) + "\n")
    r = subprocess.run(["hipcc", "-std=c++17", "-fsyntax-only", "-I", build.INC, str(unit)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    # ... and the check has teeth: one offset moved by a word must not compile
    unit.write_text("\n".join(lines).replace("offsetof(gank_slab_job, nslabs) == 32", "offsetof(gank_slab_job, nslabs) == 36") + "\n")
    assert "== 36" in unit.read_text()
    r = subprocess.run(["hipcc", "-std=c++17", "-fsyntax-only", "-I", build.INC, str(unit)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode != 0 and "offsetof gank_slab_job.nslabs" in r.stdout.decode()
