"""The stand-in chunker of examples/zpaq_standin_ops.c as a loaded library
(shared by test_cut.py, test_index_api.py, test_gpu_fds_blocks.py and
test_gpu_robustness.py; no code under test)."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "examples", "build", "libzpaq_standin.so")


def load() -> ctypes.CDLL:
    """examples/build/libzpaq_standin.so, built if it is not there:
    sf_zpaq_standin_ops(bits, max_size) gives the address of an
    sf_chunker_ops, sf_zpaq_standin_ops_free(address) releases it."""
    if not os.path.exists(SO):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples"), "build/libzpaq_standin.so"])
    lib = ctypes.CDLL(SO)
    lib.sf_zpaq_standin_ops.restype = ctypes.c_void_p
    lib.sf_zpaq_standin_ops.argtypes = [ctypes.c_uint, ctypes.c_uint32]
    lib.sf_zpaq_standin_ops_free.argtypes = [ctypes.c_void_p]
    return lib
