"""CPU-side checks of the C-ABI boundary: the library loads, exports every symbol declared in
include/dhcos.h, the ctypes table matches the header, and compute entry points fail loudly
(NativeError, no fallback) when no gfx950 device is present."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "dhcos.h")


def header_functions():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(dh_[a-z_]+)\s*\(", txt)))


def test_header_declares_expected_entry_points():
    fns = header_functions()
    for f in ("dh_surface_price", "dh_surface_loss", "dh_price_pairs", "dh_cf", "dh_trunc_range",
              "dh_cos_coeffs", "dh_surface_loss_dev", "dh_surface_price_dev", "dh_math_probe"):
        assert f in fns


def test_library_exports_every_header_symbol():
    from dhcos import _native
    lib = _native.load()
    for f in header_functions():
        assert hasattr(lib, f), f
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\bT (dh_[a-z_]+)\b", out))
    assert set(header_functions()) <= exported
    assert set(_native.SIGNATURES) == set(header_functions())


def header_code():
    """The header without its comments."""
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def header_prototypes():
    """[(name, return type, [argument declarations])] of every dh_* prototype, in the header's
    order."""
    protos = []
    for ret, name, args in re.findall(r"([A-Za-z_][\w \*]*?)\b(dh_[a-z_]+)\s*\(([^()]*)\)\s*;",
                                      header_code()):
        args = [" ".join(a.split()) for a in args.split(",")]
        protos.append((name, " ".join(ret.split()), [] if args == ["void"] else args))
    return protos


C_ABI_CLASS = {"int": "i32", "int32_t": "i32", "int64_t": "i64", "uint64_t": "u64", "size_t": "u64",
               "unsigned long long": "u64", "double": "double", "void": "void"}


def c_abi_class(decl, named=True):
    """The ABI class of a C argument declaration ('type name') or, named=False, return type; a
    type this table does not know is a KeyError, not a guess."""
    if "*" in decl:
        return "pointer"
    words = [w for w in decl.split() if w != "const"]
    return C_ABI_CLASS[" ".join(words[:-1] if named else words)]


def ctypes_abi_class(ty):
    """The ABI class of a ctypes restype / argtype."""
    import ctypes as C
    if ty is None:
        return "void"
    if ty in (C.c_void_p, C.c_char_p) or isinstance(ty, type(C.POINTER(C.c_int))):
        return "pointer"
    if ty is C.c_double:
        return "double"
    assert issubclass(ty, C._SimpleCData) and ty._type_ in "ilqLQ", ty   # an integer type
    signed = ty._type_ in "ilq"
    return {(4, True): "i32", (8, True): "i64", (8, False): "u64"}[(C.sizeof(ty), signed)]


def test_abi_class_parsers():
    """The two classifiers on the spellings the header and the binding use."""
    import ctypes as C
    for decl, want in [("int N", "i32"), ("int32_t* n_bad", "pointer"), ("void* stream", "pointer"),
                       ("int64_t P", "i64"), ("uint64_t seed", "u64"), ("size_t bytes", "u64"),
                       ("unsigned long long x", "u64"), ("double L", "double"),
                       ("const dh_surface* s", "pointer"), ("dh_ctx** out", "pointer")]:
        assert c_abi_class(decl) == want, decl
    for decl, want in [("int", "i32"), ("const char*", "pointer"), ("void*", "pointer"),
                       ("void", "void")]:
        assert c_abi_class(decl, named=False) == want, decl
    for ty, want in [(C.c_int, "i32"), (C.c_int32, "i32"), (C.c_int64, "i64"),
                     (C.c_uint64, "u64"), (C.c_size_t, "u64"), (C.c_ulonglong, "u64"),
                     (C.c_double, "double"), (C.c_void_p, "pointer"), (C.c_char_p, "pointer"),
                     (C.POINTER(C.c_double), "pointer"), (C.POINTER(C.c_void_p), "pointer"),
                     (None, "void")]:
        assert ctypes_abi_class(ty) == want, ty


def test_signatures_match_the_header_prototypes():
    """Every dh_* prototype of the header against SIGNATURES: the return type, the argument count
    and each argument in order, by ABI class (pointer, 32-bit int, 64-bit signed, 64-bit unsigned,
    double, void) -- a c_int where the header says int64_t, or a missing or moved argument,
    would truncate or shift what reaches the device code."""
    from dhcos import _native
    protos = header_prototypes()
    assert sorted(p[0] for p in protos) == header_functions()      # the parser misses none
    for name, ret, args in protos:
        res, argtypes = _native.SIGNATURES[name]
        assert ctypes_abi_class(res) == c_abi_class(ret, named=False), name
        assert len(argtypes) == len(args), name
        for i, (ty, decl) in enumerate(zip(argtypes, args)):
            assert ctypes_abi_class(ty) == c_abi_class(decl), (name, i, decl)


def test_signatures_are_in_the_header_order():
    from dhcos import _native
    assert list(_native.SIGNATURES) == [p[0] for p in header_prototypes()]


def header_struct(name):
    """[(field, C element type, array length or None)] of `typedef struct { ... } name;`."""
    body = re.search(r"typedef struct \{([^{}]*)\} " + name + ";", header_code()).group(1)
    fields = []
    for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
        ty, field, length = re.fullmatch(r"(\w+) (\w+)(?:\[(\d+)\])?", decl).groups()
        fields.append((field, ty, int(length) if length else None))
    return fields


@pytest.mark.parametrize("cname, pyname, size", [("dh_lb_options", "LbOptions", 32),
                                                 ("dh_lb_result", "LbResult", 152),
                                                 ("dh_mc_option", "McOption", 32)])
def test_structs_match_the_header(cname, pyname, size):
    """The mirrored structs: field names, order, element type and array length, and the size the
    header's fields add up to (no padding: every 8-byte field sits at a multiple of 8)."""
    import ctypes as C
    from dhcos import _native
    ctype = {"int32_t": C.c_int32, "double": C.c_double}
    want = header_struct(cname)
    got = getattr(_native, pyname)._fields_
    assert [f for f, _ in got] == [f for f, _, _ in want]
    total = 0
    for (field, ty), (_, cty, length) in zip(got, want):
        if length is None:
            assert ty is ctype[cty], field
        else:
            assert ty._type_ is ctype[cty] and ty._length_ == length, field
        total += C.sizeof(ctype[cty]) * (length or 1)
    assert C.sizeof(getattr(_native, pyname)) == total == size


def test_header_constants_match_the_binding():
    """The Python binding's copies of the header's sizes and enums: every #define DH_* integer and
    every one-line enum it mirrors (the request slots of dh_surface_fg_begin, the sharded draw's
    state words, the record stride, the series lengths, the comm id, the Monte Carlo limits and
    kinds, the request paths) and the two strike modes."""
    from dhcos import _native
    txt = open(HEADER).read()
    consts = dict((k, int(v)) for k, v in re.findall(r"#define (DH_[A-Z_]+) (\d+)", txt))
    assert consts["DH_FG_SLOTS"] == _native.FG_SLOTS
    assert consts["DH_GEN_LOC_WORDS"] == _native.GEN_LOC_WORDS
    # every integer #define is mirrored under its name without the DH_ prefix
    assert sorted(consts) == ["DH_COMM_ID_BYTES", "DH_FG_SLOTS", "DH_GEN_LOC_WORDS", "DH_MAX_N",
                              "DH_MAX_N_PER_TERM", "DH_MC_MAX_OPTIONS", "DH_MC_POISSON_CAP",
                              "DH_PARAM_STRIDE"]
    for name, v in consts.items():
        assert getattr(_native, name[3:]) == v, name
    enums = {}
    for body in re.findall(r"enum \{([^{}]*)\}", header_code()):
        enums.update((k, int(v)) for k, v in re.findall(r"(DH_[A-Z_]+) = (-?\d+)", body))
    for name in ("PATH_AUTO", "PATH_SPLIT", "PATH_FUSED", "PATH_GEN", "STRIKE_ABSOLUTE",
                 "STRIKE_PCT_SPOT"):
        assert getattr(_native, name) == enums["DH_" + name], name
    kinds = {k[6:].lower(): v for k, v in enums.items() if k.startswith("DH_MC_")}
    assert kinds == _native.MC_KINDS and len(kinds) == 4


def test_all_lists_the_public_names():
    """__all__ names only what exists, each once, and misses no public function, class or
    upper-case constant that _native.py defines at its top level."""
    import inspect
    from dhcos import _native
    assert len(set(_native.__all__)) == len(_native.__all__)
    for name in _native.__all__:
        assert hasattr(_native, name), name
    public = set()
    for name, v in vars(_native).items():
        if name.startswith("_") or inspect.ismodule(v):
            continue
        if inspect.isfunction(v) or inspect.isclass(v):
            if v.__module__ == _native.__name__:
                public.add(name)
        elif name.isupper():
            public.add(name)
    assert public == set(_native.__all__)
    for name in ("GenDraw", "iv_rows", "FG_SLOTS", "STAMPS_PER_BLOCK"):
        assert name in public


def test_library_is_gfx950_code_object():
    """The fat binary carries a gfx950 (MI355X) code object and nothing else."""
    from dhcos import _native
    data = open(_native.LIB_PATH, "rb").read()
    ids = set(re.findall(rb"amdgcn-amd-amdhsa--(gfx[0-9a-z]+)", data))
    assert ids == {b"gfx950"}, ids


def test_version_and_errors_without_device():
    from dhcos import _native
    lib = _native.load()
    assert lib.dh_version() >= 1
    if _native.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(_native.NativeError):
        _native.Context(0)


def test_product_path_fails_loudly_without_device():
    from dhcos import DoubleHeston, NativeError, _native
    if _native.device_count() > 0:
        pytest.skip("a GPU is present")
    dh = DoubleHeston(100, 100, 1.0, 0.05, 0.04, 2.0, 0.04, 0.3, -0.5, 0.04, 1.5, 0.04, 0.2, -0.3,
                      0.5, -0.05, 0.1)
    with pytest.raises(NativeError):
        dh.pricing()


def test_null_and_range_arguments_are_rejected():
    """Argument validation happens before any device work."""
    import ctypes as C
    from dhcos import _native
    lib = _native.load()
    assert lib.dh_ctx_create(0, None) == -1
    assert lib.dh_surface_price(None, None, None, 1, 128, 10.0, None) == -1
    assert b"null" in lib.dh_last_error()
    n = C.c_int32(-5)
    lib.dh_device_count(C.byref(n))
    assert n.value >= 0
    assert np.int8(1) == 1
    for setter in (lib.dh_ctx_set_tail_cut, lib.dh_ctx_set_exact, lib.dh_ctx_set_path):
        assert setter(None, 1) == -1                  # a null context, not a crash


def test_math_probe_arguments_are_rejected():
    """dh_math_probe (test support) validates its context before any device work, and the binding's
    name table is the header's list of function ids, in order."""
    from dhcos import _native
    lib = _native.load()
    assert lib.dh_math_probe(None, 0, None, None, 0, None, None) == -1
    assert b"null" in lib.dh_last_error()
    txt = open(HEADER).read()
    doc = txt[txt.index("fn: 0 dsincos"):txt.index("any other value gives DH_E_ARG")]
    ids = {name: int(i) for i, name in re.findall(r"(\d+) ([a-z_0-9]+)", doc)}
    assert ids == _native.MATH_PROBE_FNS and len(ids) == 16
    assert "math_probe" in _native.__all__


def test_gen_assemble_arguments_are_rejected():
    """dh_gen_assemble (host code) validates its sizes and pointers."""
    from dhcos import _native
    lib = _native.load()
    assert lib.dh_gen_assemble(None, None, None, None, -1, 3, None, None, None) == -1
    assert lib.dh_gen_assemble(None, None, None, None, 4, 3, None, None, None) == -1
    assert lib.dh_gen_assemble(None, None, None, None, 0, 3, None, None, None) == 0


def test_comm_and_async_fg_arguments_are_rejected():
    """The communicator and the two-slot FD request validate their arguments before any device or
    RCCL work."""
    import ctypes as C
    from dhcos import _native
    lib = _native.load()
    out = C.c_void_p()
    uid = C.create_string_buffer(_native.COMM_ID_BYTES)
    assert lib.dh_comm_create(None, C.cast(uid, C.c_void_p), 1, 0, C.byref(out)) == -1
    assert lib.dh_comm_destroy(None) == 0
    assert lib.dh_comm_broadcast(None, None, 4, 0) == -1
    assert lib.dh_comm_allgather(None, None, 4, None) == -1
    best = C.c_int32(7)
    assert lib.dh_allgather_best(None, None, 1, 3, 0, 1, None, C.byref(best)) == -1
    assert lib.dh_surface_fg_begin(None, None, None, None, 1, 100.0, 0.05, 128, 10.0, 0) == -1
    assert lib.dh_surface_fg_end(None, None, 0, 0, None, None, None) == -1
    assert lib.dh_surface_fg_cancel(None, 0) == -1
    assert b"null" in lib.dh_last_error()


def test_price_cols_and_host_register_arguments_are_rejected():
    """dh_surface_price_cols and the page-locking pair validate their arguments before any device
    work; _native.pinned leaves an array it cannot register pageable (no device here) and never
    raises for it."""
    from dhcos import _native
    lib = _native.load()
    assert lib.dh_surface_price_cols(None, None, None, None, 0.03, 1, 128, 10.0, None) == -1
    assert b"null" in lib.dh_last_error()
    assert lib.dh_host_register(None, 64) == -1
    assert lib.dh_host_unregister(None) == -1
    a = np.ones(1000)
    with _native.pinned(a, None, np.empty(0)) as pin:
        if _native.device_count() == 0:
            assert pin._done == []                    # registration failed: left pageable
        a *= 2.0
    assert pin._done == [] and a[0] == 2.0            # whatever was registered is released
