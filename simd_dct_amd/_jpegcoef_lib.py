"""ctypes binding of libmdct_jpegcoef.so -- the C-ABI declared in include/mdct_jpegcoef.h (quantised JPEG coefficient planes -> Huffman
segments with the caller's tables, their symbol statistics, and the lossless flips, transposes and rotations, on the GPU).

Its own signature table: a separate library, linked against libmdct_hip.so and libmdct_jpegenc_opt.so.  No fallback: if the shared
object is missing or fails to load, every entry point raises.
"""
import ctypes

from . import _jpegenc_opt_lib, _lib
from ._jpegenc_opt_lib import HIST_CLASS, Spec  # mdct_jpegenc_opt_spec  # noqa: F401

c_size_t = ctypes.c_size_t
c_void_p = ctypes.c_void_p
c_int = ctypes.c_int

# MDCT_JPEGCOEF_* operations
OPS = {"flip_h": 0, "flip_v": 1, "transpose": 2, "transverse": 3, "rot90": 4, "rot180": 5, "rot270": 6}


class Plane(ctypes.Structure):
    """mdct_jpegcoef_plane"""

    _fields_ = [("coef", c_void_p), ("pitch", c_size_t), ("blocks_x", ctypes.c_uint32), ("blocks_y", ctypes.c_uint32), ("h", c_int), ("v", c_int)]


# name -> (restype, argtypes); every function include/mdct_jpegcoef.h declares
SIGNATURES = {
    "mdct_jpegcoef_stats": (c_int, [ctypes.POINTER(Plane), c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "mdct_jpegcoef_rows": (c_int, [ctypes.POINTER(Plane), c_size_t, c_size_t, ctypes.POINTER(Spec), ctypes.POINTER(Spec), c_void_p, c_size_t, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p]),
    "mdct_jpegcoef_scan_rows": (c_int, [ctypes.POINTER(Plane), c_int, ctypes.POINTER(Spec), c_size_t, c_size_t, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_void_p]),
    "mdct_jpegcoef_transform": (c_int, [ctypes.POINTER(Plane), ctypes.POINTER(Plane), c_int, c_void_p]),
    "mdct_jpegcoef_last_error": (ctypes.c_char_p, []),
}

LIB = _lib.Library("mdct_jpegcoef", ("mdct_jpegcoef.h",), SIGNATURES, after=(_jpegenc_opt_lib.LIB,))
load, LIB_PATH = LIB.load, LIB.path
