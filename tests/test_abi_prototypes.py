"""The ctypes prototypes of merge_spmv_amd against the C headers.  A wrong argtypes entry does not raise: it reinterprets memory on the
GPU.  So every function include/mspmv.h and include/mspmv_dev.h declare is parsed here, and its return class, its argument count and
every argument's class are compared with what the LOADED libraries carry (the restype / argtypes objects on the CDLL, not the text
of the table that set them).  CPU only: nothing is called.

Also the life of a library-owned handle (merge_spmv_amd._args._Handle) with a counting stand-in for the C destructor."""
import ctypes
import os
import re

import pytest

from conftest import ROOT
import merge_spmv_amd as M
from merge_spmv_amd._args import _Handle

SETTERS = ["mspmv_set_band_passes", "mspmv_set_compact_tiles", "mspmv_set_record_polls", "mspmv_set_tdm", "mspmv_set_tuning"]


def c_class(decl: str) -> str:
    """the class of one C parameter or return type: pointer | i32 | i64 | size | float | double | void"""
    decl = decl.strip()
    if "*" in decl or re.search(r"\bmspmv_stream_t\b", decl) or "[" in decl:
        return "pointer"
    words = [w for w in re.findall(r"\w+", decl) if w not in ("const", "unsigned", "signed")]
    for ctype, cls in (("int32_t", "i32"), ("int", "i32"), ("int64_t", "i64"), ("size_t", "size"), ("float", "float"), ("double", "double"),
                       ("void", "void")):
        if words and words[0] == ctype:
            return cls
    raise AssertionError(f"a parameter type this test does not know: {decl!r}")


def declared(header: str) -> dict:
    """{function: (return class, [argument classes])} of one header, comments and the MSPMV_DEV experiment block stripped (as
    test_abi_exports.declared_symbols strips them)"""
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"#ifdef MSPMV_DEV\n.*?#endif\n", "", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)                              # the other preprocessor lines
    text = re.sub(r"typedef\s+struct[^{;]*\{.*?\}[^;]*;", "", text, flags=re.S)     # struct bodies: their fields are no parameters
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(mspmv_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        params = params.strip()
        args = [] if params in ("", "void") else [c_class(p) for p in params.split(",")]
        assert name not in out, f"{name} is declared twice in {header}"
        out[name] = (c_class(ret), args)
    return out


def ctypes_class(t) -> str:
    """the class of a ctypes type as a C compiler sees it"""
    if t is None:
        return "void"
    if t in (ctypes.c_void_p, ctypes.c_char_p) or isinstance(t, type(ctypes.POINTER(ctypes.c_int))):
        return "pointer"
    if t is ctypes.c_float:
        return "float"
    if t is ctypes.c_double:
        return "double"
    if t is ctypes.c_size_t:                  # (before the sized integers: on this ABI size_t is c_ulong, no signed type's alias)
        return "size"
    if t in (ctypes.c_int, ctypes.c_int32):
        return "i32"
    if t is ctypes.c_int64:
        return "i64"
    raise AssertionError(f"a ctypes type this test does not know: {t!r}")


def prototyped(lib) -> dict:
    """every mspmv_* function object the CDLL holds (ctypes caches one per name it was asked for), with what it carries"""
    return {name: fn for name, fn in vars(lib).items() if name.startswith("mspmv_") and hasattr(fn, "argtypes")}


def mismatches(lib, functions: dict) -> list:
    bad = []
    for name, (ret, args) in sorted(functions.items()):
        fn = getattr(lib, name)
        if fn.argtypes is None:
            bad.append(f"{name}: no argtypes")
            continue
        have = [ctypes_class(t) for t in fn.argtypes]
        if ctypes_class(fn.restype) != ret:
            bad.append(f"{name}: returns {ret}, restype is {fn.restype!r}")
        if len(have) != len(args):
            bad.append(f"{name}: {len(args)} arguments declared, {len(have)} in argtypes")
        else:
            bad += [f"{name}: argument {i} is {a}, argtypes has {h}" for i, (a, h) in enumerate(zip(args, have)) if a != h]
    return bad


def _libraries():
    prev = M.active_library()
    try:
        M.use_library("product")
        product = M.load_library()
        M.use_library("dev")
        dev = M.load_library()
    finally:
        M.use_library(prev)
    return product, dev


def test_the_parser_reads_the_headers():
    h = declared("mspmv.h")
    assert len(h) == 117 and not [n for n in h if n.startswith("mspmv_set_")]
    assert h["mspmv_version"] == ("i32", [])
    assert h["mspmv_error_string"] == ("pointer", ["i32"])
    assert h["mspmv_mg_plan_stream"] == ("pointer", ["pointer", "i32"])
    assert h["mspmv_csrmv_f64"] == ("i32", ["pointer"] * 7 + ["i32"] * 3 + ["pointer", "i32"])
    assert h["mspmv_vec_dot_f32"][1][4] == "i64" and h["mspmv_probe_read_stream"][1] == ["pointer", "size", "i32", "pointer"]
    assert h["mspmv_pcg_solve_f32"][1][7:9] == ["double", "double"] and h["mspmv_csrmm_f32"][1][13:15] == ["float", "float"]
    d = declared("mspmv_dev.h")
    assert sorted(d) == SETTERS and all(ret == "i32" and set(args) == {"i32"} for ret, args in d.values())


def test_every_declared_function_is_prototyped_as_the_header_declares_it():
    product, dev = _libraries()
    functions, setters = declared("mspmv.h"), declared("mspmv_dev.h")
    assert len(functions) + len(setters) == 122
    assert mismatches(product, functions) == []
    assert mismatches(dev, {**functions, **setters}) == []
    assert product.mspmv_version.argtypes == []


def test_nothing_is_prototyped_that_the_headers_do_not_declare():
    product, dev = _libraries()
    functions, setters = declared("mspmv.h"), declared("mspmv_dev.h")
    for name in functions:                     # (touch every name, so that a function left without a prototype would show up as one)
        getattr(product, name), getattr(dev, name)
    assert sorted(prototyped(product)) == sorted(functions)
    assert sorted(prototyped(dev)) == sorted({**functions, **setters})


class _FakeLib:
    def __init__(self):
        self.destroyed = []

    def fake_destroy(self, handle):
        self.destroyed.append(handle)
        return 0


class _Thing(_Handle):
    _destroy = "fake_destroy"

    def __init__(self, lib, fail_before_the_handle=False):
        self._lib = lib
        if fail_before_the_handle:
            raise M.MspmvError("the create call failed")
        self._handle = ctypes.c_void_p(0x1000)

    def use(self):
        return self._live()


def test_a_handle_is_destroyed_exactly_once():
    lib = _FakeLib()
    t = _Thing(lib)
    handle = t.use()
    t.close()
    t.close()
    t.__del__()
    del t
    assert lib.destroyed == [handle]


def test_a_closed_handle_refuses_use():
    t = _Thing(_FakeLib())
    t.close()
    with pytest.raises(M.MspmvError, match="_Thing: closed"):
        t.use()


def test_del_after_a_failed_constructor_does_nothing():
    lib = _FakeLib()
    t = _Thing.__new__(_Thing)
    with pytest.raises(M.MspmvError):
        t.__init__(lib, fail_before_the_handle=True)
    t.__del__()
    t.close()
    assert lib.destroyed == []
    bare = _Thing.__new__(_Thing)              # (not even the library was captured)
    bare.__del__()


def test_del_never_raises():
    class Broken(_Thing):
        _destroy = "no_such_function"
    t = Broken(_FakeLib())
    with pytest.raises(AttributeError):
        t.close()
    t2 = Broken(_FakeLib())
    t2.__del__()
