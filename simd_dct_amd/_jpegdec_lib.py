"""ctypes binding of libmdct_jpegdec.so -- the C-ABI declared in include/mdct_jpegdec.h (the GPU JPEG decoder).

Its own signature table: the decoder is a separate library, linked against libmdct_hip.so.  No fallback: if the shared
object is missing or fails to load, every entry point raises.
"""
import ctypes

from . import _lib

c_size_t = ctypes.c_size_t
c_void_p = ctypes.c_void_p
c_int = ctypes.c_int
u8pp = ctypes.POINTER(ctypes.c_void_p)

MAX_COMPONENTS = 3
OK, OUT_OF_DATA, BAD_CODE, COEF_OVERFLOW, UNEXPECTED_MARKER, LEFTOVER = range(6)
STATUS_NAMES = {OK: "ok", OUT_OF_DATA: "out of data", BAD_CODE: "invalid code", COEF_OVERFLOW: "coefficient index beyond 63",
                UNEXPECTED_MARKER: "unexpected marker", LEFTOVER: "bits left over"}


class Component(ctypes.Structure):
    """mdct_jpegdec_component"""

    _fields_ = [("coef", c_void_p), ("pitch", c_size_t), ("blocks_x", c_size_t), ("blocks_y", c_size_t),
                ("h", c_int), ("v", c_int), ("dc_slot", c_int), ("ac_slot", c_int)]


class Scan(ctypes.Structure):
    """mdct_jpegdec_scan"""

    _fields_ = [("n_components", c_int), ("comp", Component * MAX_COMPONENTS), ("mcus_x", c_size_t), ("mcus_y", c_size_t),
                ("restart_interval", c_size_t)]


# name -> (restype, argtypes); every function include/mdct_jpegdec.h declares
SIGNATURES = {
    "mdct_jpegdec_tables_create": (c_int, [ctypes.POINTER(c_void_p), u8pp, u8pp, ctypes.POINTER(c_int)]),
    "mdct_jpegdec_tables_destroy": (c_int, [c_void_p]),
    "mdct_jpegdec_tables_check": (c_int, [u8pp, u8pp, ctypes.POINTER(c_int)]),
    "mdct_jpegdec_index": (c_int, [c_void_p, c_size_t, c_size_t, c_void_p, c_void_p, c_void_p]),
    "mdct_jpegdec_intervals": (c_size_t, [ctypes.POINTER(Scan)]),
    "mdct_jpegdec_decode": (c_int, [ctypes.POINTER(Scan), c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]),
    "mdct_jpegdec_last_error": (ctypes.c_char_p, []),
}

LIB = _lib.Library("mdct_jpegdec", ("mdct_jpegdec.h",), SIGNATURES)
load, LIB_PATH = LIB.load, LIB.path
