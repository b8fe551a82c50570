"""ctypes binding of libmdct_jpegenc_opt.so -- the C-ABI declared in include/mdct_jpegenc_opt.h (symbol statistics of the planes of a
JPEG encode, optimal Huffman tables for them, and coders that take the caller's tables, on the GPU).

Its own signature table: a separate library, linked against libmdct_hip.so.  No fallback: if the shared object is missing or fails to
load, every entry point raises.
"""
import ctypes

from . import _lib
from ._jpegenc_scan_lib import Plane  # mdct_jpegenc_scan_plane  # noqa: F401

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

LIB = _lib.Library("mdct_jpegenc_opt", ("mdct_jpegenc_opt.h",), SIGNATURES)
load, LIB_PATH = LIB.load, LIB.path
