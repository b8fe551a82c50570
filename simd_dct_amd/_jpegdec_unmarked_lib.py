"""ctypes binding of libmdct_jpegdec_unmarked.so -- the C-ABI declared in include/mdct_jpegdec_unmarked.h (the GPU decoder of scans
without restart markers).

Its own signature table: a separate library, linked against libmdct_jpegdec.so (whose table handle and scan descriptor it takes) and
libmdct_hip.so.  No fallback: if the shared object is missing or fails to load, every entry point raises.
"""
import ctypes

from . import _jpegdec_lib, _lib

c_size_t = ctypes.c_size_t
c_void_p = ctypes.c_void_p
c_int = ctypes.c_int

NOT_SYNCHRONISED = 6
STATUS_NAMES = {**_jpegdec_lib.STATUS_NAMES, NOT_SYNCHRONISED: "chunks not synchronised"}
CHUNK_BYTES = 8192  # stuffed scan bytes per workgroup: sync_rounds >= ceil(scan_len / CHUNK_BYTES) always converges

# name -> (restype, argtypes); every function include/mdct_jpegdec_unmarked.h declares
SIGNATURES = {
    "mdct_jpegdec_unmarked_workspace": (c_size_t, [ctypes.POINTER(_jpegdec_lib.Scan), c_size_t]),
    "mdct_jpegdec_decode_unmarked": (c_int, [ctypes.POINTER(_jpegdec_lib.Scan), c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p,
                                             c_int, c_void_p]),
    "mdct_jpegdec_unmarked_last_error": (ctypes.c_char_p, []),
}

LIB = _lib.Library("mdct_jpegdec_unmarked", ("mdct_jpegdec_unmarked.h",), SIGNATURES, after=(_jpegdec_lib.LIB,), label="mdct_jpegdec")
load, LIB_PATH = LIB.load, LIB.path
