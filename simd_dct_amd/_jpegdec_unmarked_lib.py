"""ctypes binding of libmdct_jpegdec_unmarked.so -- the C-ABI declared in include/mdct_jpegdec_unmarked.h (the GPU decoder of scans
without restart markers).

Its own signature table: a separate library, linked against libmdct_jpegdec.so (whose table handle and scan descriptor it takes) and
libmdct_hip.so.  No fallback: if the shared object is missing or fails to load, every entry point raises.
"""
import ctypes
import os

from . import _jpegdec_lib, _lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmdct_jpegdec_unmarked.so")

c_size_t = ctypes.c_size_t
c_void_p = ctypes.c_void_p
c_int = ctypes.c_int

NOT_SYNCHRONISED = 6
STATUS_NAMES = {**_jpegdec_lib.STATUS_NAMES, NOT_SYNCHRONISED: "chunks not synchronised"}
CHUNK_BYTES = 8192  # stuffed scan bytes per workgroup: sync_rounds >= ceil(scan_len / CHUNK_BYTES) always converges

# name -> (restype, argtypes); every function include/mdct_jpegdec_unmarked.h declares
SIGNATURES = {
    "mdct_jpegdec_unmarked_workspace": (c_size_t, [ctypes.POINTER(_jpegdec_lib.Scan), c_size_t]),
    "mdct_jpegdec_decode_unmarked": (c_int, [ctypes.POINTER(_jpegdec_lib.Scan), c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p,
                                             c_int, c_void_p]),
    "mdct_jpegdec_unmarked_last_error": (ctypes.c_char_p, []),
}

_lib_handle = None


def load():
    """Load libmdct_jpegdec_unmarked.so (once), after libmdct_jpegdec.so and libmdct_hip.so."""
    global _lib_handle
    if _lib_handle is None:
        _jpegdec_lib.load()
        _lib_handle = _lib.bind(LIB_PATH, SIGNATURES)
    return _lib_handle
