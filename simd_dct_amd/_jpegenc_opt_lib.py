"""ctypes binding of libmdct_jpegenc_opt.so -- the C-ABI declared in include/mdct_jpegenc_opt.h (symbol statistics of the planes of a
JPEG encode, optimal Huffman tables for them, and coders that take the caller's tables, on the GPU).

Its own signature table: a separate library, linked against libmdct_hip.so.  No fallback: if the shared object is missing or fails to
load, every entry point raises.
"""
import ctypes
import os

from . import _lib
from ._jpegenc_scan_lib import Plane  # mdct_jpegenc_scan_plane  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmdct_jpegenc_opt.so")
HIST_CLASS = 272  # MDCT_JPEGENC_OPT_HIST_CLASS

c_size_t = ctypes.c_size_t
c_void_p = ctypes.c_void_p
c_int = ctypes.c_int


class Spec(ctypes.Structure):
    """mdct_jpegenc_opt_spec"""

    _fields_ = [("bits16", c_void_p), ("vals", c_void_p), ("nvals", c_int)]


# name -> (restype, argtypes); every function include/mdct_jpegenc_opt.h declares
SIGNATURES = {
    "mdct_jpegenc_opt_stats": (c_int, [ctypes.POINTER(Plane), c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "mdct_jpegenc_opt_table": (c_int, [c_void_p, c_int, c_void_p, c_void_p, ctypes.POINTER(c_int)]),
    "mdct_jpegenc_opt_rows": (c_int, [c_void_p, c_size_t, c_void_p, c_size_t, c_size_t, c_size_t, c_size_t, ctypes.POINTER(Spec), ctypes.POINTER(Spec), c_void_p,
                                      c_size_t, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mdct_jpegenc_opt_scan_rows": (c_int, [ctypes.POINTER(Plane), c_int, c_void_p, c_void_p, ctypes.POINTER(Spec), c_size_t, c_size_t, c_void_p, c_size_t, c_void_p,
                                           c_void_p, c_void_p, c_void_p]),
    "mdct_jpegenc_opt_seg_stride": (c_size_t, [c_size_t]),
    "mdct_jpegenc_opt_last_error": (ctypes.c_char_p, []),
}

_lib_handle = None


def load():
    """Load libmdct_jpegenc_opt.so (once), after libmdct_hip.so (whose launch tally and HIP runtime it shares)."""
    global _lib_handle
    if _lib_handle is None:
        _lib.load()
        _lib_handle = _lib.bind(LIB_PATH, SIGNATURES)
    return _lib_handle
