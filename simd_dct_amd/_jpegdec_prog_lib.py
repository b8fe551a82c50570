"""ctypes binding of libmdct_jpegdec_prog.so -- the C-ABI declared in include/mdct_jpegdec_prog.h (the GPU decoder of a progressive
file's scans: spectral selection only, with restart markers).

Its own signature table: a separate library, linked against libmdct_jpegdec.so (whose table handle, scan descriptor and interval index
it takes) and libmdct_hip.so.  No fallback: if the shared object is missing or fails to load, every entry point raises.
"""
import ctypes
import os

from . import _jpegdec_lib, _lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmdct_jpegdec_prog.so")

c_size_t = ctypes.c_size_t
c_void_p = ctypes.c_void_p
c_int = ctypes.c_int

EOBRUN_OVERFLOW = 7
STATUS_NAMES = {**_jpegdec_lib.STATUS_NAMES, EOBRUN_OVERFLOW: "end-of-band run past the interval's last block"}

# name -> (restype, argtypes); every function include/mdct_jpegdec_prog.h declares
SIGNATURES = {
    "mdct_jpegdec_prog_intervals": (c_size_t, [ctypes.POINTER(_jpegdec_lib.Scan), c_int, c_int]),
    "mdct_jpegdec_prog_decode": (c_int, [ctypes.POINTER(_jpegdec_lib.Scan), c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p,
                                         c_void_p]),
    "mdct_jpegdec_prog_last_error": (ctypes.c_char_p, []),
}

_lib_handle = None


def load():
    """Load libmdct_jpegdec_prog.so (once), after libmdct_jpegdec.so and libmdct_hip.so."""
    global _lib_handle
    if _lib_handle is None:
        _jpegdec_lib.load()
        _lib_handle = _lib.bind(LIB_PATH, SIGNATURES)
    return _lib_handle
