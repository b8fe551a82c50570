"""ctypes binding of libmdct_jpegdec.so -- the C-ABI declared in include/mdct_jpegdec.h (the GPU JPEG decoder).

Its own signature table: the decoder is a separate library, linked against libmdct_hip.so.  No fallback: if the shared
object is missing or fails to load, every entry point raises.
"""
import ctypes
import os

from . import _lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmdct_jpegdec.so")

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

_lib_handle = None


def load():
    """Load libmdct_jpegdec.so (once), after libmdct_hip.so (whose launch tally and HIP runtime it shares)."""
    global _lib_handle
    if _lib_handle is None:
        _lib.load()
        _lib_handle = _lib.bind(LIB_PATH, SIGNATURES)
    return _lib_handle
