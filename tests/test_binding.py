"""CPU: the Python binding layer itself.  The declaration table of
syncfast_amd/_lib.py against every prototype of include/*.h (ctypes checks a
call against argtypes, never against the C prototype, so a wrong arity or a
32/64-bit slip in the table is silent without this), and the small helpers
every wrapper goes through: the SF_ENOSPC grow-and-retry, the explicit-list
normaliser and the taking of library-allocated rows."""
import ctypes
import os
import re

import numpy as np
import pytest

from syncfast_amd import _lib, host
from syncfast_amd._lib import SF_EINVAL, SF_ENOSPC, SF_OK, SfError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = {"syncfast_amd.h": _lib._PUBLIC, "syncfast_amd_test.h": _lib._TEST}
SCALARS = {"int": 4, "uint32_t": 4, "uint64_t": 8, "int64_t": 8}
RETURNS = {"int": ctypes.c_int, "const char *": ctypes.c_char_p, "void": None}


def prototypes(header):
    """{name: (return type, [parameter text, ...])} of every function a header
    declares, and the names of its function-pointer typedefs."""
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    fn_types = set(re.findall(r"typedef\s+[\w\s\*]+?\(\s*\*\s*(\w+)\s*\)\s*\([^)]*\)\s*;", src))
    src = re.sub(r"typedef\s+struct\s+\w+\s*\{.*?\}\s*\w+\s*;", " ", src, flags=re.S)  # members are not prototypes
    src = re.sub(r"typedef[^;{]*;", " ", src)
    out = {}
    for ret, name, params in re.findall(r"\b(int|void|const\s+char\s*\*)\s*(sf_\w+)\s*\(([^()]*)\)\s*;", src):
        params = " ".join(params.split())
        out[name] = (" ".join(ret.split()).replace("char*", "char *"),
                     [] if params == "void" else [p.strip() for p in params.split(",")])
    return out, fn_types


def is_pointer_like(t):
    return t in (ctypes.c_void_p, ctypes.c_char_p) or (
        isinstance(t, type) and issubclass(t, (ctypes._Pointer, ctypes._CFuncPtr)))


def test_the_header_parser_sees_every_function():
    """The prototype parser finds what test_capi's looser name search finds:
    nothing is skipped by the stricter pattern."""
    total = 0
    for header in HEADERS:
        src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        assert sorted(prototypes(header)[0]) == sorted(set(re.findall(r"\b(sf_[a-z0-9_]+)\s*\(", src)))
        total += len(prototypes(header)[0])
    assert total >= 60


@pytest.mark.parametrize("header", sorted(HEADERS))
def test_table_matches_the_header(header):
    table = HEADERS[header]
    protos, fn_types = prototypes(header)
    assert sorted(table) == sorted(protos)  # every entry is a header function and vice versa
    for name, (ret, params) in protos.items():
        restype, argtypes = table[name]
        assert restype is RETURNS[ret], name
        assert len(argtypes) == len(params), (name, params)
        for k, (p, t) in enumerate(zip(params, argtypes)):
            words = p.replace("*", " * ").replace("[", " [ ").split()
            if "*" in words or "[" in words or fn_types & set(words):
                assert is_pointer_like(t), (name, k, p, t)
            else:
                base = [w for w in words[:-1] if w != "const"]  # the last word is the parameter's name
                assert len(base) == 1 and base[0] in SCALARS, (name, k, p)
                assert not is_pointer_like(t) and ctypes.sizeof(t) == SCALARS[base[0]], (name, k, p, t)


def test_exported_names_are_the_tables_keys():
    assert _lib.EXPORTED == tuple(_lib._PUBLIC) and _lib.EXPORTED_TEST == tuple(_lib._TEST)
    assert not set(_lib._PUBLIC) & set(_lib._TEST)


def test_declare_sets_what_the_table_says():
    L = _lib.lib()
    for table in HEADERS.values():
        for name, (restype, argtypes) in table.items():
            fn = getattr(L, name)
            assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    assert L.sf_free_cuts.restype is None and L.sf_free_rows.restype is None


def _script(*results):
    """A fake entry point: returns the scripted (rc, need) in turn and records
    the capacities it was called with."""
    calls, left = [], list(results)

    def call(cap):
        calls.append(cap)
        rc, need = left.pop(0)
        return rc, need, f"value{len(calls)}"
    return call, calls


def test_retry_succeeds_first_time():
    call, calls = _script((SF_OK, 3))
    assert _lib.retry_enospc(call, 10, 4, "x") == (3, "value1") and calls == [10]


def test_retry_grows_once_to_the_reported_need():
    call, calls = _script((SF_ENOSPC, 25), (SF_OK, 25))
    assert _lib.retry_enospc(call, 10, 4, "x") == (25, "value2") and calls == [10, 25]


@pytest.mark.parametrize("need", [10, 9, 0])
def test_retry_does_not_repeat_a_need_that_fits(need):
    call, calls = _script((SF_ENOSPC, need), (SF_OK, need))
    with pytest.raises(SfError) as e:
        _lib.retry_enospc(call, 10, 4, "x")
    assert e.value.code == SF_ENOSPC and calls == [10]


@pytest.mark.parametrize("tries", [1, 2, 4])
def test_retry_stops_at_its_bound(tries):
    call, calls = _script(*[(SF_ENOSPC, 10 * (k + 2)) for k in range(10)])
    with pytest.raises(SfError) as e:
        _lib.retry_enospc(call, 10, tries, "x")
    assert e.value.code == SF_ENOSPC and calls == [10 * (k + 1) for k in range(tries)]


def test_retry_raises_any_other_code_at_once():
    call, calls = _script((SF_EINVAL, 99), (SF_OK, 99))
    with pytest.raises(SfError) as e:
        _lib.retry_enospc(call, 10, 4, lambda rc: f"named {rc}")
    assert e.value.code == SF_EINVAL and calls == [10] and f"named {SF_EINVAL}" in str(e.value)
    call, calls = _script((SF_ENOSPC, 20), (SF_EINVAL, 0), (SF_OK, 0))
    with pytest.raises(SfError) as e:
        _lib.retry_enospc(call, 10, 4, "x")
    assert e.value.code == SF_EINVAL and calls == [10, 20]


@pytest.mark.parametrize("offsets, sizes", [
    ([0, 5, 9], [5, 4, 1]),
    (np.array([0, 5, 9], np.int64), np.array([5, 4, 1], np.int64)),
    (np.array([[0, 5], [9, 12]], np.int64), np.array([[5, 4], [3, 1]], np.int32)),
    (np.arange(12, dtype=np.uint64)[::2], np.ones(12, np.uint32)[::2]),  # strided views
])
def test_list_normaliser(offsets, sizes):
    offs, szs, n = host._list(offsets, sizes)
    assert offs.dtype == np.uint64 and szs.dtype == np.uint32
    assert offs.ndim == szs.ndim == 1 and offs.flags.c_contiguous and szs.flags.c_contiguous
    assert n == offs.size == szs.size == np.asarray(offsets).size
    assert offs.tolist() == np.asarray(offsets).reshape(-1).tolist()
    assert szs.tolist() == np.asarray(sizes).reshape(-1).tolist()


def test_list_normaliser_empty_and_unequal():
    for empty in ([], np.zeros(0, np.uint64), np.zeros((0, 2), np.int64)):
        offs, szs, n = host._list(empty, empty)
        assert n == 0 and offs.shape == szs.shape == (0,)
        assert offs.dtype == np.uint64 and szs.dtype == np.uint32
    for offsets, sizes in (([0, 1], [1]), ([], [1]), (np.zeros((2, 2)), np.zeros(3))):
        with pytest.raises(ValueError, match="differ in length"):
            host._list(offsets, sizes)


def _library_rows(n):
    """n rows in a buffer of the test's own, as a library would hand them out."""
    src = np.zeros(max(n, 1), host.SIG_DTYPE)
    src["offset"][:n] = np.arange(n) * 7
    src["size"][:n] = 7
    src["sha1"][:n] = np.arange(n * 20, dtype=np.uint8).reshape(n, 20)
    return src, src.ctypes.data_as(ctypes.POINTER(_lib.BlockSig))


@pytest.mark.parametrize("n", [0, 1, 5])
def test_take_rows_copies_and_frees_once(n):
    src, p = _library_rows(n)
    freed = []
    got = host._take_rows(p, n, freed.append)
    assert freed == [p]
    assert got.dtype == host.SIG_DTYPE and got.shape == (n,) and np.array_equal(got, src[:n])
    src["size"][:] = 0  # an array of its own, not a view of the library's buffer
    assert n == 0 or got["size"].tolist() == [7] * n


def test_take_rows_frees_when_the_copy_raises(monkeypatch):
    src, p = _library_rows(3)
    freed = []

    def failing(*_a):
        raise MemoryError("copy")
    monkeypatch.setattr(host.ctypes, "memmove", failing)
    with pytest.raises(MemoryError):
        host._take_rows(p, 3, freed.append)
    assert freed == [p]


def test_take_rows_uses_the_librarys_free_by_default(monkeypatch):
    """Without an explicit free function the rows go back through
    sf_free_rows, with the pointer it was given."""
    src, p = _library_rows(2)
    freed = []

    class Lib:
        sf_free_rows = staticmethod(freed.append)
    monkeypatch.setattr(host, "lib", lambda: Lib)
    assert np.array_equal(host._take_rows(p, 2), src[:2]) and freed == [p]
