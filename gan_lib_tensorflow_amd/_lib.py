"""ctypes binding of libgank.so, derived from include/gank.h at import.  There is NO fallback: if the HIP library is
missing or a symbol is absent this module raises, and every compute entry point of the package goes through it.

The header is the only description of the ABI: parse_header() reads its `#define GANK_*` constants, its descriptor structs and
every function declaration, and nothing here names a symbol or a field.  To add an entry point, declare it in gank.h, define it
in csrc/, wrap it in kernels.py.  The typing rules:
  - by value: int, long, long long, float, double, int64_t -- any other spelling is a RuntimeError at import that names the
    declaration (so is anything else the reader cannot read: it never skips);
  - returns: int, long, double, const char* (c_char_p);
  - a pointer to one of the header's structs: POINTER(that Structure) -- callers pass (Struct * n)() arrays and byref(struct), and
    a descriptor of the wrong kind is refused;
  - every other pointer, struct fields included: c_void_p, which takes tensor addresses, None, byref(c_int / c_double),
    (c_float * n)(), (c_void_p * n)() and string buffers alike.  The element type of such a pointer is NOT checked.  That is
    looser than the hand-kept table this replaces in twelve places, which were POINTER(c_int / c_float / c_double / c_void_p)
    or c_char_p there: the double*, int* and char* outputs of gank_prof_collect and gank_prof_kernel_stats, the window of
    gank_msssim_level, prep_weight of gank_sn_power_iter_fwd_prep / _fwd_b_prep / _fwd_b_prep_feed and u_next of
    gank_sn_adam_fwd_a (and tighter in one: the job table of gank_sum_slabs_label_bwd is POINTER(SlabJob) as the header says)."""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# GANK_DTYPE = bf16 (default) | fp16: the element type of activations / MFMA operands for this PROCESS.  The two are separate
# builds of the same kernels (libgank.so, libgank_f16.so: gank_act_dtype()); everything above the C ABI takes the matching
# torch dtype from ACT_DTYPE_NAME (kernels.BF16).
DTYPE = os.environ.get("GANK_DTYPE", "bf16").lower()
if DTYPE not in ("bf16", "fp16"):
    raise RuntimeError(f"GANK_DTYPE={DTYPE!r}: bf16 or fp16")
ACT_DTYPE_NAME = "bfloat16" if DTYPE == "bf16" else "float16"
LIB_PATH = os.path.join(_HERE, os.environ.get("GANK_LIB_NAME", "libgank.so" if DTYPE == "bf16" else "libgank_f16.so"))   # GANK_LIB_NAME: experiment builds

HEADER = os.path.join(os.path.dirname(_HERE), "include", "gank.h")

# every C type the header may spell by value; anything else fails the import with the declaration's name
_SCALARS = {"int": C.c_int, "long": C.c_long, "long long": C.c_longlong, "float": C.c_float, "double": C.c_double, "int64_t": C.c_int64}
_RETURNS = {"int": C.c_int, "long": C.c_long, "double": C.c_double, "const char*": C.c_char_p}


def _ctype(decl, owner, structs):
    """One `type name` declaration (a function argument or a struct field) of `owner` -> (name, ctype)."""
    *kind, name = [w for w in re.findall(r"\w+|\S", decl) if w != "const"] or [""]
    if re.fullmatch(r"[A-Za-z_]\w*", name) and name not in kind:        # (`long long` without a name is not `long` called long)
        if re.fullmatch(r"\w+( \w+)*( \*)+", " ".join(kind)):
            return name, C.POINTER(structs[kind[0]]) if kind[0] in structs and len(kind) == 2 else C.c_void_p
        if " ".join(kind) in _SCALARS:
            return name, _SCALARS[" ".join(kind)]
    raise RuntimeError(f"gank.h: {owner}: cannot type {' '.join(decl.split())!r}")


def parse_header(text):
    """C header text -> (defines, structs, prototypes, returns): the `#define GANK_*` integers by name, one ctypes.Structure per
    `typedef struct ... { ... } gank_x;` by its C name, and the argtypes and the restype of every declared function by symbol."""
    def bad(decl, why):
        symbol = (re.findall(r"\bgank_\w+", decl, flags=re.I) or ["?"])[0]
        return RuntimeError(f"gank.h: {symbol}: {why}: {' '.join(decl.split())[:100]!r}")

    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    expected = len(re.findall(r"\bgank_[a-z0-9_]+\s*\(", text))
    defines = {}
    for line in re.findall(r"^[ \t]*#[ \t]*define[ \t]+GANK_\w+[ \t]+\S.*$", text, flags=re.M):     # (the include guard has no value)
        try:
            defines[line.split()[1]] = int(line.split(None, 2)[2], 0)
        except ValueError:
            raise bad(line, "not an integer constant") from None
    text = re.sub(r'^[ \t]*#.*$|extern\s+"C"\s*\{', " ", text, flags=re.M)
    structs = {}

    def struct(m):
        fields = []
        for decl in filter(None, (d.strip() for d in m.group(1).split(";"))):
            first, *more = decl.split(",")      # `int ksize, Cin, Cout;`: the type is what stands before the first name (or star)
            base = first.split("*")[0] if "*" in first else re.sub(r"\w+\s*$", "", first)
            fields += [_ctype(d, m.group(2), {}) for d in [first] + [base + " " + d for d in more]]
        camel = "".join(w.capitalize() for w in m.group(2).split("_")[1:])
        structs[m.group(2)] = type(camel, (C.Structure,), {"_fields_": fields, "__doc__": m.group(2)})
        return " "
    text = re.sub(r"typedef\s+struct\s+\w*\s*\{([^{}]*)\}\s*(gank_\w+)\s*;", struct, text)
    prototypes, returns = {}, {}
    *decls, tail = text.split(";")
    if tail.strip() not in ("", "}"):           # (`}` closes extern "C")
        raise bad(tail, "declaration without `;`")
    for decl in filter(None, (d.strip() for d in decls)):
        m = re.fullmatch(r"([\w\s*]+?)\s*\b(gank_[a-z0-9_]+)\s*\(([^()]*)\)", decl)
        ret = re.sub(r"\s*\*", "*", " ".join(m.group(1).split())) if m else None
        if ret not in _RETURNS or m.group(2) in prototypes:
            raise bad(decl, "not one new declaration `ret gank_name(args);` with ret one of " + ", ".join(_RETURNS))
        args = [] if m.group(3).strip() in ("", "void") else m.group(3).split(",")
        prototypes[m.group(2)], returns[m.group(2)] = [_ctype(a, m.group(2), structs)[1] for a in args], _RETURNS[ret]
    if len(prototypes) != expected:
        raise RuntimeError(f"gank.h: {expected} `gank_name(` tokens but {len(prototypes)} declarations read")
    return defines, structs, prototypes, returns


with open(HEADER) as _f:
    DEFINES, STRUCTS, PROTOTYPES, RESTYPES = parse_header(_f.read())     # PROTOTYPES: symbol -> argument ctypes
# Published under the names the callers import: the constants without their prefix (GANK_IN_RELU -> IN_RELU, GANK_STAT_SLOTS ->
# STAT_SLOTS, ...) and each descriptor class under the CamelCase of its C name without it (gank_sn_desc -> SnDesc, ...).
globals().update({k[len("GANK_"):]: v for k, v in DEFINES.items()})
globals().update({s.__name__: s for s in STRUCTS.values()})

_lib = None


def load():
    """Load libgank.so and bind every symbol of include/gank.h.  Raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run "
            "`python -m gan_lib_tensorflow_amd.build` (needs hipcc). There is no CPU fallback.")
    # libgank.so must bind to the HIP runtime that torch ships (torch/lib/libamdhip64.so), not to a second copy from
    # /opt/rocm: with two runtimes in one process the second one sees no device ("no ROCm-capable device is detected" on
    # the first launch).  Importing torch first makes its runtime the one the loader reuses for our DT_NEEDED entry.
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, args in PROTOTYPES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise RuntimeError(f"libgank.so does not export {name}; rebuild it") from e
        fn.argtypes = args
        fn.restype = RESTYPES[name]
    if lib.gank_version() != DEFINES["GANK_VERSION"]:
        raise RuntimeError(f"{LIB_PATH} is version {lib.gank_version()}, include/gank.h declares {DEFINES['GANK_VERSION']}; rebuild it")
    if lib.gank_act_dtype() != (1 if DTYPE == "fp16" else 0):
        raise RuntimeError(f"{LIB_PATH} was built for {'fp16' if lib.gank_act_dtype() else 'bf16'} buffers, this process runs GANK_DTYPE={DTYPE}")
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().gank_last_error()
        raise RuntimeError(f"gank: {what}: {msg.decode() if msg else 'error'}")
