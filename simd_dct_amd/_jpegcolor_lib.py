"""ctypes binding of libmdct_jpegcolor.so -- the C-ABI declared in include/mdct_jpegcolor.h (chroma upsampling and YCbCr -> RGB of
decoded JPEG planes on the GPU).

Its own signature table: a separate library, linked against libmdct_hip.so.  No fallback: if the shared object is missing or fails to
load, every entry point raises.
"""
import ctypes

from . import _lib

c_size_t = ctypes.c_size_t
c_void_p = ctypes.c_void_p
c_int = ctypes.c_int

YCBCR, RGB, GREY = 0, 1, 2
HWC, CHW = 0, 1


class Plane(ctypes.Structure):
    """mdct_jpegcolor_plane"""

    _fields_ = [("px", c_void_p), ("pitch", c_size_t), ("width", c_size_t), ("height", c_size_t), ("h", c_int), ("v", c_int)]


# name -> (restype, argtypes); every function include/mdct_jpegcolor.h declares
SIGNATURES = {
    "mdct_jpegcolor_to_rgb": (c_int, [ctypes.POINTER(Plane), c_int, c_size_t, c_size_t, c_int, c_int, c_void_p, c_size_t, c_size_t, c_void_p]),
    "mdct_jpegcolor_last_error": (ctypes.c_char_p, []),
}

LIB = _lib.Library("mdct_jpegcolor", ("mdct_jpegcolor.h",), SIGNATURES)
load, LIB_PATH = LIB.load, LIB.path
