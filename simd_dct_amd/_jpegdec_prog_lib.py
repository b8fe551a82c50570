"""ctypes binding of libmdct_jpegdec_prog.so -- the C-ABI declared in include/mdct_jpegdec_prog.h (the GPU decoder of a progressive
file's scans: spectral selection and successive approximation).

Its own signature table: a separate library, linked against libmdct_jpegdec.so (whose table handle, scan descriptor and interval index
it takes) and libmdct_hip.so.  No fallback: if the shared object is missing or fails to load, every entry point raises.
"""
import ctypes

from . import _jpegdec_lib, _lib

c_size_t = ctypes.c_size_t
c_void_p = ctypes.c_void_p
c_int = ctypes.c_int

EOBRUN_OVERFLOW = 7
STATUS_NAMES = {**_jpegdec_lib.STATUS_NAMES, EOBRUN_OVERFLOW: "end-of-band run past the interval's last block"}

# name -> (restype, argtypes); every function include/mdct_jpegdec_prog.h declares
SIGNATURES = {
    "mdct_jpegdec_prog_intervals": (c_size_t, [ctypes.POINTER(_jpegdec_lib.Scan), c_int, c_int]),
    "mdct_jpegdec_prog_decode": (c_int, [ctypes.POINTER(_jpegdec_lib.Scan), c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p,
                                         c_void_p]),
    "mdct_jpegdec_prog_decode_approx": (c_int, [ctypes.POINTER(_jpegdec_lib.Scan), c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t,
                                                c_void_p, c_void_p, c_void_p]),
    "mdct_jpegdec_prog_last_error": (ctypes.c_char_p, []),
}

LIB = _lib.Library("mdct_jpegdec_prog", ("mdct_jpegdec_prog.h",), SIGNATURES, after=(_jpegdec_lib.LIB,))
load, LIB_PATH = LIB.load, LIB.path
