"""ctypes binding of libmdct_jpegscale.so -- the C-ABI declared in include/mdct_jpegscale.h (the reduced-size inverse of a JPEG decode:
coefficient planes -> 8-bit planes at 1/2, 1/4 or 1/8 size on the GPU).

Its own signature table: a separate library, linked against libmdct_hip.so.  No fallback: if the shared object is missing or fails to
load, every entry point raises.
"""
import ctypes

from . import _lib

c_size_t = ctypes.c_size_t
c_void_p = ctypes.c_void_p
c_int = ctypes.c_int


class Plane(ctypes.Structure):
    """mdct_jpegscale_plane"""

    _fields_ = [("coef", c_void_p), ("pitch_coef", c_size_t), ("px", c_void_p), ("pitch_px", c_size_t), ("blocks_x", c_size_t),
                ("blocks_y", c_size_t), ("lut", c_void_p), ("n", c_int), ("rep_x", c_int), ("rep_y", c_int)]


# name -> (restype, argtypes); every function include/mdct_jpegscale.h declares
SIGNATURES = {
    "mdct_jpegscale_inv_i16_u8": (c_int, [ctypes.POINTER(Plane), c_int, c_int, c_void_p]),
    "mdct_jpegscale_last_error": (ctypes.c_char_p, []),
}

LIB = _lib.Library("mdct_jpegscale", ("mdct_jpegscale.h",), SIGNATURES)
load, LIB_PATH = LIB.load, LIB.path
