"""ctypes binding of libmdct_jpegenc.so -- the C-ABI declared in include/mdct_jpegenc.h (RGB -> YCbCr, chroma downsampling and block
padding of an image before a JPEG encode, on the GPU).

Its own signature table: a separate library, linked against libmdct_hip.so.  No fallback: if the shared object is missing or fails to
load, every entry point raises.
"""
import ctypes

from . import _lib

c_size_t = ctypes.c_size_t
c_void_p = ctypes.c_void_p
c_int = ctypes.c_int

RGB, GREY = 0, 1
HWC, CHW = 0, 1


class Plane(ctypes.Structure):
    """mdct_jpegenc_plane"""

    _fields_ = [("px", c_void_p), ("pitch", c_size_t), ("width", c_size_t), ("height", c_size_t), ("h", c_int), ("v", c_int)]


# name -> (restype, argtypes); every function include/mdct_jpegenc.h declares
SIGNATURES = {
    "mdct_jpegenc_from_rgb": (c_int, [c_void_p, c_size_t, c_size_t, c_size_t, c_size_t, c_int, c_int, ctypes.POINTER(Plane), c_int, c_void_p]),
    "mdct_jpegenc_last_error": (ctypes.c_char_p, []),
}

LIB = _lib.Library("mdct_jpegenc", ("mdct_jpegenc.h",), SIGNATURES)
load, LIB_PATH = LIB.load, LIB.path
