"""ctypes binding of libmdct_jpegdec_batch.so -- the C-ABI declared in include/mdct_jpegdec_batch.h (the restart-marked scans of many
JPEG files decoded in four launches).

Its own signature table: a separate library, linked against libmdct_hip.so.  No fallback: if the shared object is missing or fails
to load, every entry point raises.
"""
import ctypes

from . import _jpegdec_lib, _lib

c_size_t = ctypes.c_size_t
c_void_p = ctypes.c_void_p
c_int = ctypes.c_int

OUT_OF_RANGE = c_size_t(-1).value  # what the per-scan / per-chunk getters answer for an index out of range


class BatchScan(ctypes.Structure):
    """mdct_jpegdec_batch_scan"""

    _fields_ = [("desc", _jpegdec_lib.Scan), ("byte_offset", c_size_t), ("byte_len", c_size_t),
                ("bits16", c_void_p * 4), ("vals", c_void_p * 4), ("nvals", c_int * 4)]


_plan_getter = (c_size_t, [c_void_p])
_indexed_getter = (c_size_t, [c_void_p, c_size_t])

# name -> (restype, argtypes); every function include/mdct_jpegdec_batch.h declares
SIGNATURES = {
    "mdct_jpegdec_batch_plan_create": (c_int, [ctypes.POINTER(c_void_p), ctypes.POINTER(BatchScan), c_size_t, c_size_t, ctypes.POINTER(c_size_t)]),
    "mdct_jpegdec_batch_plan_destroy": (c_int, [c_void_p]),
    "mdct_jpegdec_batch_scans": _plan_getter,
    "mdct_jpegdec_batch_intervals": _plan_getter,
    "mdct_jpegdec_batch_offsets": _plan_getter,
    "mdct_jpegdec_batch_chunks": _plan_getter,
    "mdct_jpegdec_batch_table_sets": _plan_getter,
    "mdct_jpegdec_batch_first_interval": _indexed_getter,
    "mdct_jpegdec_batch_first_chunk": _indexed_getter,
    "mdct_jpegdec_batch_chunk_bytes": _indexed_getter,
    "mdct_jpegdec_batch_chunk_scan": _indexed_getter,
    "mdct_jpegdec_batch_table_set": _indexed_getter,
    "mdct_jpegdec_batch_image_bytes": _plan_getter,
    "mdct_jpegdec_batch_bind": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mdct_jpegdec_batch_index": (c_int, [c_void_p, c_void_p]),
    "mdct_jpegdec_batch_decode": (c_int, [c_void_p, c_void_p]),
    "mdct_jpegdec_batch_last_error": (ctypes.c_char_p, []),
}

LIB = _lib.Library("mdct_jpegdec_batch", ("mdct_jpegdec_batch.h",), SIGNATURES)
load, LIB_PATH = LIB.load, LIB.path
