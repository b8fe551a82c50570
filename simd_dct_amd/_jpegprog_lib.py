"""ctypes binding of libmdct_jpegprog.so -- the C-ABI declared in include/mdct_jpegprog.h (quantised JPEG coefficient planes -> the
Huffman segments of a progressive file's scans, spectral selection and successive approximation: DC scans and the scans of one AC band
with end-of-band runs, first and refinement, and their symbol statistics, on the GPU).

Its own signature table: a separate library, linked against libmdct_hip.so and libmdct_jpegenc_opt.so.  No fallback: if the shared
object is missing or fails to load, every entry point raises.
"""
import ctypes

from . import _jpegenc_opt_lib, _lib
from ._jpegcoef_lib import Plane  # mdct_jpegcoef_plane  # noqa: F401
from ._jpegenc_opt_lib import HIST_CLASS, Spec  # mdct_jpegenc_opt_spec  # noqa: F401

c_size_t = ctypes.c_size_t
c_void_p = ctypes.c_void_p
c_int = ctypes.c_int

AC_HIST = 256  # counts of mdct_jpegprog_ac_stats, by RRRRSSSS

# name -> (restype, argtypes); every function include/mdct_jpegprog.h declares
SIGNATURES = {
    "mdct_jpegprog_dc_stats": (c_int, [ctypes.POINTER(Plane), c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "mdct_jpegprog_dc_rows": (c_int, [ctypes.POINTER(Plane), c_int, c_int, ctypes.POINTER(Spec), c_size_t, c_size_t, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_void_p]),
    "mdct_jpegprog_ac_stats": (c_int, [ctypes.POINTER(Plane), c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "mdct_jpegprog_ac_rows": (c_int, [ctypes.POINTER(Plane), c_int, c_int, c_size_t, c_size_t, ctypes.POINTER(Spec), c_void_p, c_size_t, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_void_p]),
    "mdct_jpegprog_dc_stats_approx": (c_int, [ctypes.POINTER(Plane), c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "mdct_jpegprog_dc_rows_approx": (c_int, [ctypes.POINTER(Plane), c_int, c_int, ctypes.POINTER(Spec), c_int, c_int, c_size_t, c_size_t, c_void_p, c_size_t, c_void_p,
                                             c_void_p, c_void_p, c_void_p, c_void_p]),
    "mdct_jpegprog_ac_stats_approx": (c_int, [ctypes.POINTER(Plane), c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "mdct_jpegprog_ac_rows_approx": (c_int, [ctypes.POINTER(Plane), c_int, c_int, c_int, c_int, c_size_t, c_size_t, ctypes.POINTER(Spec), c_void_p, c_size_t, c_void_p,
                                             c_void_p, c_void_p, c_void_p, c_void_p]),
    "mdct_jpegprog_last_error": (ctypes.c_char_p, []),
}

LIB = _lib.Library("mdct_jpegprog", ("mdct_jpegprog.h",), SIGNATURES, after=(_jpegenc_opt_lib.LIB,))
load, LIB_PATH = LIB.load, LIB.path
