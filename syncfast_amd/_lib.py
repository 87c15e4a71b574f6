"""ctypes binding of libsyncfast_amd.so (the C-ABI in include/syncfast_amd.h).

The library is built in-tree (``syncfast_amd/lib/libsyncfast_amd.so``) by
``__graft_entry__.build()`` / ``make -C syncfast_amd/csrc``.  There is no
Python or CPU fallback: if the library is missing, importing the compute
entry points raises.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SF_LIB overrides the library path (tuning builds, scripts/tune*.py only).
LIB_PATH = os.environ.get("SF_LIB") or os.path.join(_HERE, "lib", "libsyncfast_amd.so")

SF_OK = 0
SF_EIO = -5
SF_EAGAIN = -11
SF_ENOMEM = -12
SF_ENODEV = -19
SF_EINVAL = -22
SF_ENOSPC = -28
SF_ERANGE = -34
SF_ETIMEDOUT = -110

# Why a FILE_BLOCK parse stopped (sf_wire_parse_blocks_device)
SF_WIRE_END, SF_WIRE_INCOMPLETE, SF_WIRE_OTHER, SF_WIRE_MALFORMED = 0, 1, 2, 3
# sf_receive_files_device only: a whole message the sink's state does not take
SF_WIRE_UNEXPECTED = 4
# sf_receive_file_entries_device only: END_FILES stood after the last entry
SF_WIRE_END_FILES = 5
# Why sf_serve_get_files_device stopped answering
SF_SERVE_ALL, SF_SERVE_BAD_NAME, SF_SERVE_UNKNOWN, SF_SERVE_FULL = 0, 1, 2, 3

HASH_DIGEST_LEN = 20
MAX_BLOCK_SIZE = 32 << 20


class SfError(OSError):
    """A negative SF_E* return code (maps to the reference's Error::Io)."""

    def __init__(self, code: int, what: str = ""):
        msg = _strerror(code)
        super().__init__(-code, f"{what}: {msg}" if what else msg)
        self.code = code


class BlockSig(ctypes.Structure):
    """sf_block_sig: (offset, size, sha1[20]) -- 32 bytes."""
    _fields_ = [("offset", ctypes.c_uint64), ("size", ctypes.c_uint32),
                ("sha1", ctypes.c_uint8 * 20)]


class ChainJob(ctypes.Structure):
    """sf_chain_job: one blocks_hash chain job of an earlier batch."""
    _fields_ = [("d_digests", ctypes.c_void_p), ("n_files", ctypes.c_uint32), ("part", ctypes.c_uint32),
                ("blocks", ctypes.c_uint64), ("d_state", ctypes.c_void_p), ("d_hashes", ctypes.c_void_p)]


class FileStamp(ctypes.Structure):
    """sf_file_stamp: fstat's identity of an open file's contents."""
    _fields_ = [("dev", ctypes.c_uint64), ("ino", ctypes.c_uint64), ("size", ctypes.c_uint64),
                ("nlink", ctypes.c_uint64), ("mtime_sec", ctypes.c_int64), ("mtime_nsec", ctypes.c_int64),
                ("ctime_sec", ctypes.c_int64), ("ctime_nsec", ctypes.c_int64)]


def same_stamp(a: FileStamp, b: FileStamp) -> bool:
    """The library's stamp comparison (include/syncfast_amd.h): dev, ino, size
    and mtime equal, and ctime too unless the link count changed."""
    return (a.dev, a.ino, a.size, a.mtime_sec, a.mtime_nsec) == (b.dev, b.ino, b.size, b.mtime_sec, b.mtime_nsec) \
        and (a.nlink != b.nlink or (a.ctime_sec, a.ctime_nsec) == (b.ctime_sec, b.ctime_nsec))


# sf_test_read_hook_fn: void (*)(void* arg, uint64_t window)
READ_HOOK = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_uint64)


class FileDesc(ctypes.Structure):
    _fields_ = [("offset", ctypes.c_uint64), ("len", ctypes.c_uint64)]


class ChunkerOps(ctypes.Structure):
    """sf_chunker_ops (include/syncfast_amd.h): a caller's native chunker."""
    _fields_ = [("create", ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p)),
                ("next", ctypes.CFUNCTYPE(ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)),
                ("destroy", ctypes.CFUNCTYPE(None, ctypes.c_void_p)),
                ("ctx", ctypes.c_void_p)]


def num_blocks(length: int, block_size: int) -> int:
    """ceil(len / B); 0 for an empty input (no empty blocks)."""
    return (length + block_size - 1) // block_size if length else 0


def _table():
    """name -> (restype, argtypes) of every function the two headers declare;
    tests/test_binding.py holds it against their prototypes."""
    vp, u64, u32, i32, i64, cp = (ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_int64,
                                  ctypes.c_char_p)
    P = ctypes.POINTER
    pu64, pu32, pint, pi64, sig, stamp = P(u64), P(u32), P(i32), P(i64), P(BlockSig), P(FileStamp)
    public = {  # include/syncfast_amd.h
        "sf_version": (cp, []),
        "sf_strerror": (cp, [i32]),
        "sf_device_count": (i32, [pint]),
        "sf_set_device": (i32, [i32]),
        "sf_release_host_cache": (i32, []),
        "sf_index_device_fixed": (i32, [vp, u64, u32, vp, u64, pu64, vp]),
        "sf_index_device_blocks": (i32, [vp, u64, vp, vp, u64, vp, vp, vp]),
        "sf_index_device_fixed_weak": (i32, [vp, u64, u32, vp, vp, u64, pu64, vp]),
        "sf_index_device_blocks_weak": (i32, [vp, u64, vp, vp, u64, vp, vp, vp, vp]),
        "sf_index_device_batch": (i32, [vp, u64, P(FileDesc), u32, u32, vp, u64, vp, vp, pu64, vp, vp]),
        "sf_index_device_batch_chained": (i32, [vp, u32, u64, u32, vp, P(ChainJob), u32, vp]),
        "sf_index_device_batch_chained_cols": (i32, [vp, u32, u64, u32, u64, u64, vp, P(ChainJob), u32, vp]),
        "sf_block_set_build": (i32, [vp, vp, u64, P(vp), vp]),
        "sf_block_set_lookup": (i32, [vp, vp, u64, vp, vp]),
        "sf_block_set_free": (i32, [vp, vp]),
        "sf_wire_file_blocks_device": (i32, [vp, u64, u32, u64, vp, u64, pu64, vp]),
        "sf_wire_blocks_device": (i32, [vp, vp, u64, vp, u64, pu64, vp]),
        "sf_wire_file_blocks_fd": (i32, [vp, u64, u32, u64, i32, pu64, vp]),
        "sf_wire_blocks_fd": (i32, [vp, vp, u64, i32, pu64, vp]),
        "sf_wire_parse_blocks_device": (i32, [vp, u64, vp, vp, u64, pu64, pu64, pint, vp]),
        "sf_receive_blocks_device": (i32, [vp, vp, u64, u64, vp, vp, vp, vp, u64, pu64, pu64, pint, pu64, vp]),
        "sf_receive_blocks_buffer": (i32, [vp, vp, u64, u64, sig, vp, u64, pu64, pu64, pint, pu64]),
        "sf_receive_files_device": (i32, [vp, vp, u64, i32, u64, vp, vp, vp, vp, vp, u64, vp, vp, vp, vp, u64, pu64, pu64,
                                          pu64, pint, pint, pu64, vp]),
        "sf_receive_block_data_device": (i32, [vp, u64, vp, vp, vp, vp, u64, pu64, pu64, pint, pu64, pu64, vp]),
        "sf_receive_block_data_buffer": (i32, [vp, u64, sig, vp, u64, pu64, pu64, pint, pu64, pu64]),
        "sf_wire_block_data_device": (i32, [vp, u64, vp, vp, vp, u64, P(vp), vp]),
        "sf_serve_get_blocks_device": (i32, [vp, vp, vp, vp, u64, vp, u64, P(vp), pu64, pu64, pu64, pint, vp]),
        "sf_wire_run_info": (i32, [vp, P(vp), pu64, pu64]),
        "sf_wire_run_read": (i32, [vp, u64, vp, u64]),
        "sf_wire_run_to_fd": (i32, [vp, i32, pu64]),
        "sf_wire_run_free": (i32, [vp, vp]),
        "sf_wire_files_device": (i32, [vp, vp, u64, vp, vp, vp, u64, P(vp), pu64, vp]),
        "sf_name_set_build": (i32, [vp, vp, vp, u64, P(vp), pu64, vp]),
        "sf_name_set_lookup": (i32, [vp, vp, u64, vp, vp, u64, vp, vp]),
        "sf_name_set_free": (i32, [vp, vp]),
        "sf_wire_file_entries_device": (i32, [vp, vp, vp, vp, u64, i32, P(vp), pu64, vp]),
        "sf_receive_file_entries_device": (i32, [vp, vp, u64, vp, vp, vp, vp, vp, vp, vp, vp, vp, u64, pu64, pu64, pu64,
                                                 pu64, pint, vp]),
        "sf_wire_get_files_device": (i32, [vp, u64, vp, vp, u64, vp, u64, P(vp), pu64, vp]),
        "sf_wire_parse_get_files_device": (i32, [vp, u64, vp, vp, u64, pu64, pu64, pu64, pint, vp]),
        "sf_serve_get_files_device": (i32, [vp, vp, vp, vp, u64, vp, u64, u64, P(vp), pu64, pu64, pu64, pint, pu64, pu64,
                                            pint, vp]),
        "sf_wire_get_blocks_device": (i32, [vp, vp, vp, u64, i32, P(vp), pu64, vp]),
        "sf_place_block_data_device": (i32, [vp, vp, vp, vp, u64, vp, vp, vp, vp, u64, vp, vp, vp, vp, vp, u64, vp,
                                            pu64, pu64, pu64, vp]),
        "sf_copy_blocks_device": (i32, [vp, u64, vp, u64, vp, vp, vp, vp, u64, vp, vp]),
        "sf_write_device_fd": (i32, [vp, u64, i32, u64, pu64, vp]),
        "sf_plan_copies_device": (i32, [vp, vp, vp, vp, vp, u64, vp, u64, vp, vp, vp, u64, vp, vp, u64, vp, u64, vp, vp, vp,
                                       vp, vp, vp, vp, u64, vp, pu64, vp]),
        "sf_fill_splitmix_device": (i32, [vp, u64, u64, u64, vp]),
        "sf_index_buffer": (i32, [vp, u64, u32, sig, u64, pu64]),
        "sf_index_buffer_blocks": (i32, [vp, u64, vp, vp, u64, sig, vp]),
        "sf_index_file_blocks": (i32, [cp, vp, vp, u64, sig, vp]),
        "sf_file_stamp_fd": (i32, [i32, stamp]),
        "sf_read_fd_device": (i32, [i32, stamp, u64, u64, vp, pu64, vp]),
        "sf_index_fd_blocks": (i32, [i32, stamp, vp, vp, u64, sig, vp]),
        "sf_index_fd_fixed": (i32, [i32, stamp, u32, sig, u64, pu64, vp]),
        "sf_index_file": (i32, [cp, u32, sig, u64, pu64, vp]),
        "sf_index_file_range": (i32, [cp, u64, u64, u32, sig, u64, pu64]),
        "sf_index_fd": (i32, [i32, u32, P(sig), pu64, vp]),
        "sf_free_rows": (None, [sig]),
        "sf_index_files": (i32, [P(cp), u32, u32, u64, sig, u64, pu64, vp, pu64, pu32]),
        "sf_index_fds_blocks": (i32, [vp, vp, u32, vp, vp, vp, u64, sig, u64, pu64, vp, vp, pu32]),
        "sf_cut_fd": (i32, [i32, vp, vp, u32, P(vp), P(vp), pu64]),
        "sf_free_cuts": (None, [vp]),
        "sf_index_fd_cut": (i32, [i32, vp, vp, u32, P(sig), pu64, vp]),
        "sf_zpaq_cut_buffer": (i32, [vp, u64, u32, u32, vp, vp, u64, pu64]),
        "sf_zpaq_chunker_ops": (i32, [u32, u32, vp]),
        "sf_cut_device_zpaq": (i32, [vp, u64, u32, u32, vp, vp, u64, pu64, vp]),
        "sf_index_device_zpaq": (i32, [vp, u64, u32, u32, vp, vp, vp, u64, pu64, vp, vp]),
        "sf_index_fd_zpaq": (i32, [i32, vp, u32, u32, P(sig), pu64, vp]),
        "sf_cut_device_zpaq_files": (i32, [vp, u64, vp, vp, u32, u32, u32, u32, vp, vp, u64, vp, pu64, vp, pu32, pu32,
                                           vp]),
        "sf_index_device_zpaq_files": (i32, [vp, u64, vp, vp, u32, u32, u32, u32, vp, vp, vp, u64, vp, pu64, vp, vp, pu32,
                                             pu32, vp]),
        "sf_index_fds_zpaq": (i32, [vp, vp, u32, u32, u32, u32, u64, P(sig), pu64, pu64, vp, vp, pu32]),
        "sf_shard_range": (i32, [u64, u32, u32, u32, pu64, pu64]),
        "sf_index_file_multi": (i32, [cp, u32, u32, sig, u64, pu64, vp]),
        "sf_index_device_multi": (i32, [u32, vp, u64, u32, vp, u32, vp, vp]),
        "sf_index_device_multi_ex": (i32, [u32, vp, u64, u32, vp, u32, vp, vp, vp]),
        "sf_blocks_hash": (i32, [vp, u64, vp]),
        "sf_blocks_hash_sigs": (i32, [sig, u64, vp]),
        "sf_sha1_host": (i32, [vp, u64, vp]),
    }
    # include/syncfast_amd_test.h: knobs latched at load, route counters, the
    # explicit-list processing order, the read hook, the last call's statistics
    test = {
        "sf_test_set_knob": (i32, [cp, i64, pi64]),
        "sf_test_get_knob": (i32, [cp, pi64]),
        "sf_test_get_stat": (i32, [cp, pi64]),
        "sf_test_table_order": (i32, [vp, u64, vp, vp]),
        "sf_test_table_order_bits": (i32, [vp, u64, u32, vp, vp]),
        "sf_test_set_read_hook": (i32, [READ_HOOK, vp]),
        "sf_test_multi_plan": (i32, [u64, u32, u32, u32, i32, vp, vp, vp]),
        "sf_test_xcd_litmus": (i32, [i32, pu32]),
        "sf_test_zpaq_device_stats": (i32, [vp]),
        "sf_test_zpaq_files_stats": (i32, [vp]),
        "sf_test_wire_parse_stats": (i32, [vp]),
        "sf_test_recv_files_stats": (i32, [vp]),
        "sf_test_file_entries_stats": (i32, [vp]),
        "sf_test_serve_files_stats": (i32, [vp]),
        "sf_test_block_data_stats": (i32, [vp]),
        "sf_test_copy_stats": (i32, [vp]),
        "sf_test_plan_copies_stats": (i32, [vp]),
    }
    return public, test


_PUBLIC, _TEST = _table()
EXPORTED, EXPORTED_TEST = tuple(_PUBLIC), tuple(_TEST)

_lib = None


def _declare(L: ctypes.CDLL) -> None:
    for table in (_PUBLIC, _TEST):
        for name, (restype, argtypes) in table.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes


def lib() -> ctypes.CDLL:
    """Load the HIP library; raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(syncfast_amd has no CPU fallback)")
        L = ctypes.CDLL(LIB_PATH)
        _declare(L)
        _lib = L
    return _lib


def _strerror(code: int) -> str:
    try:
        return lib().sf_strerror(code).decode()
    except ImportError:
        return f"error {code}"


def check(rc: int, what: str = "") -> None:
    if rc != SF_OK:
        raise SfError(rc, what)


def retry_enospc(call, cap: int, tries: int, what=""):
    """An entry point whose output is sized by a guess: ``call(cap)`` runs it
    with room for ``cap`` and returns (rc, need, value).  On SF_ENOSPC with a
    need above ``cap`` it is called again with that need, ``tries`` calls at
    the most (a file may grow between two calls; one that grows every time
    ends as SF_ENOSPC).  Returns the last (need, value); any other code, or
    the last SF_ENOSPC, raises SfError (``what``: a string, or a function
    of the failed call's code that gives one)."""
    for attempt in range(tries):
        rc, need, value = call(cap)
        if rc != SF_ENOSPC or need <= cap or attempt == tries - 1:
            break
        cap = need
    if rc != SF_OK:
        raise SfError(rc, what(rc) if callable(what) else what)
    return need, value


def get_knob(name: str) -> int:
    """Current value of a library knob (latched from the environment when the
    library was loaded; include/syncfast_amd_test.h)."""
    v = ctypes.c_int64()
    check(lib().sf_test_get_knob(name.encode(), ctypes.byref(v)), name)
    return v.value


def set_knob(name: str, value: int) -> int:
    """Set a library knob (test hook); returns the previous value."""
    old = ctypes.c_int64()
    check(lib().sf_test_set_knob(name.encode(), int(value), ctypes.byref(old)), name)
    return old.value


def get_stat(name: str) -> int:
    """A route counter of the host entry points ("pages_locked",
    "not_anon_refused")."""
    v = ctypes.c_int64()
    check(lib().sf_test_get_stat(name.encode(), ctypes.byref(v)), name)
    return v.value


_read_hook_ref = None  # keeps the ctypes thunk alive while the library holds it


def set_read_hook(fn) -> None:
    """Test hook (sf_test_set_read_hook): fn(window) runs after each window a
    pread route of the library has read, on the calling thread; None removes
    it."""
    global _read_hook_ref
    if fn is None:
        check(lib().sf_test_set_read_hook(READ_HOOK(), None), "sf_test_set_read_hook")
        _read_hook_ref = None
        return
    thunk = READ_HOOK(lambda _arg, window: fn(int(window)))
    check(lib().sf_test_set_read_hook(thunk, None), "sf_test_set_read_hook")
    _read_hook_ref = thunk


def _elf_sections(b: bytes):
    """(section header tuples, section names) of an ELF64 image; a header is
    (name, type, flags, addr, offset, size, link, info, addralign, entsize)."""
    import struct
    if b[:4] != b"\x7fELF" or b[4] != 2:
        raise ValueError("not an ELF64 image")
    shoff, = struct.unpack_from("<Q", b, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", b, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", b, shoff + i * shentsize) for i in range(shnum)]
    stro = secs[shstrndx][4]
    return secs, [b[stro + s[0]: b.index(b"\0", stro + s[0])] for s in secs]


def _code_objects(path: str):
    """(triple, bytes) of every gfx950 code object in the library's
    .hip_fatbin section (one clang offload bundle per GPU translation unit)."""
    import struct
    with open(path or LIB_PATH, "rb") as f:
        b = f.read()
    secs, names = _elf_sections(b)
    if b".hip_fatbin" not in names:
        raise ValueError("no .hip_fatbin section")
    sec = secs[names.index(b".hip_fatbin")]
    fat = b[sec[4]: sec[4] + sec[5]]
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    pos = fat.find(magic)
    while pos >= 0:  # bundle: magic, u64 entries, then (u64 offset, u64 size, u64 triple length, triple)
        n, = struct.unpack_from("<Q", fat, pos + len(magic))
        p = pos + len(magic) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", fat, p)
            triple = fat[p + 24: p + 24 + tlen]
            p += 24 + tlen
            if triple.startswith(b"hipv4-amdgcn"):
                yield triple, fat[pos + off: pos + off + size]
        pos = fat.find(magic, pos + 1)


def _kernel_symbols(co: bytes):
    """(symbol name, st_info, code bytes) of every sized symbol in a code
    object's .symtab; nothing for a code object without one."""
    import struct
    if co[:4] != b"\x7fELF":
        return
    secs, names = _elf_sections(co)
    if b".symtab" not in names:
        return
    symtab = secs[names.index(b".symtab")]
    strtab = secs[symtab[6]]  # sh_link
    for i in range(symtab[5] // 24):
        st_name, st_info, _other, st_shndx, st_value, st_size = struct.unpack_from("<IBBHQQ", co, symtab[4] + 24 * i)
        if st_size and st_shndx < len(secs):  # defined in a section (not SHN_ABS / SHN_COMMON)
            sec = secs[st_shndx]
            start = sec[4] + (st_value - sec[3])
            yield (co[strtab[4] + st_name: co.index(b"\0", strtab[4] + st_name)].decode(), st_info,
                   co[start: start + st_size])


FIXED_KERNEL = "_ZN2sf17sha1_fixed_kernelILi128ELi1ELb0EEEvPKhmjmPhNS_11PadScheduleEPj"
CHAINED_KERNEL = "_ZN2sf25sha1_fixed_chained_kernelILi128EEEvPKhmjmPhNS_11PadScheduleENS_8ChainJobES5_jjj"
TABLE_KERNEL = "_ZN2sf17sha1_table_kernelILi128ELb0EEEvPKhmPKmPKjmPhPiPjS6_"


def kernel_code_sha256(path: str = None, symbol: str = FIXED_KERNEL) -> str:
    """SHA-256 of one kernel's machine code (its bytes in the gfx950 code
    object's .text, located through .symtab): what the GPU runs for that
    kernel.  Other kernels of the same translation unit can change without
    changing it.  bench.py keys the PMC traffic of profiles/traffic.json on it
    for the headline kernel (sha1_fixed_kernel<128, 1, false>); config 3's
    line names sha1_fixed_chained_kernel<128>'s (CHAINED_KERNEL), whose
    block rate depends on how its block part was compiled (DESIGN.md
    section 3.3b)."""
    import hashlib
    for _, co in _code_objects(path):
        for name, _info, code in _kernel_symbols(co):
            if name == symbol:
                return hashlib.sha256(code).hexdigest()
    raise ValueError(f"no code object defines {symbol}")


def code_object_sha256(path: str = None, kernel: bytes = b"sha1_fixed_kernel") -> str:
    """SHA-256 of the gfx950 code object that holds `kernel` (the library's
    ``.hip_fatbin`` section holds one clang offload bundle per GPU translation
    unit; sha1_fixed_kernel is in sf_capi.hip's, with the stand-alone chain
    kernel and the splitmix fill).  Host-only changes, and changes to other
    translation units' kernels, leave it unchanged; any change to a kernel of
    that unit alters it.  bench.py reports it; nothing is matched on it (the
    PMC traffic of profiles/traffic.json is keyed on kernel_code_sha256)."""
    import hashlib
    for _, co in _code_objects(path):
        if kernel in co:
            return hashlib.sha256(co).hexdigest()
    raise ValueError(f"no code object holds {kernel!r}")


def device_count() -> int:
    n = ctypes.c_int(0)
    check(lib().sf_device_count(ctypes.byref(n)), "sf_device_count")
    return n.value
