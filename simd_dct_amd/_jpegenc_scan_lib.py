"""ctypes binding of libmdct_jpegenc_scan.so -- the C-ABI declared in include/mdct_jpegenc_scan.h (the three planes of a colour JPEG
encode -> the Huffman segments of one interleaved scan, on the GPU).

Its own signature table: a separate library, linked against libmdct_hip.so.  No fallback: if the shared object is missing or fails to
load, every entry point raises.
"""
import ctypes

from . import _lib

c_size_t = ctypes.c_size_t
c_void_p = ctypes.c_void_p
c_int = ctypes.c_int


class Plane(ctypes.Structure):
    """mdct_jpegenc_scan_plane"""

    _fields_ = [("px", c_void_p), ("pitch", c_size_t), ("width", c_size_t), ("height", c_size_t), ("h", c_int), ("v", c_int)]


# name -> (restype, argtypes); every function include/mdct_jpegenc_scan.h declares
SIGNATURES = {
    "mdct_jpegenc_scan_rows": (c_int, [ctypes.POINTER(Plane), c_int, c_void_p, c_void_p, c_size_t, c_size_t, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]),
    "mdct_jpegenc_scan_seg_stride": (c_size_t, [c_size_t, c_int]),
    "mdct_jpegenc_scan_last_error": (ctypes.c_char_p, []),
}

LIB = _lib.Library("mdct_jpegenc_scan", ("mdct_jpegenc_scan.h",), SIGNATURES)
load, LIB_PATH = LIB.load, LIB.path
