"""ctypes binding of libmdct_jpegenc_batch.so -- the C-ABI declared in include/mdct_jpegenc_batch.h (a batch of RGB images -> the
interleaved scans of their JPEG files in three launches).

Its own signature table: a separate library, linked against libmdct_hip.so.  No fallback: if the shared object is missing or fails
to load, every entry point raises.
"""
import ctypes

from . import _jpegenc_lib, _lib

c_size_t = ctypes.c_size_t
c_void_p = ctypes.c_void_p
c_int = ctypes.c_int

OUT_OF_RANGE = c_size_t(-1).value  # what the per-image / per-row getters answer for an index out of range
MAX_ROWS = 16384  # MDCT_JPEGENC_BATCH_MAX_ROWS


class BatchImage(ctypes.Structure):
    """mdct_jpegenc_batch_image"""

    _fields_ = [("in_", c_void_p), ("in_pitch", c_size_t), ("in_plane_stride", c_size_t), ("width", c_size_t), ("height", c_size_t),
                ("planes", _jpegenc_lib.Plane * 3), ("seg", c_void_p), ("seg_stride", c_size_t)]


_plan_getter = (c_size_t, [c_void_p])
_indexed_getter = (c_size_t, [c_void_p, c_size_t])

# name -> (restype, argtypes); every function include/mdct_jpegenc_batch.h declares
SIGNATURES = {
    "mdct_jpegenc_batch_plan_create": (c_int, [ctypes.POINTER(c_void_p), ctypes.POINTER(BatchImage), c_size_t, c_int, c_void_p, c_void_p, ctypes.POINTER(c_size_t)]),
    "mdct_jpegenc_batch_plan_destroy": (c_int, [c_void_p]),
    "mdct_jpegenc_batch_images": _plan_getter,
    "mdct_jpegenc_batch_rows": _plan_getter,
    "mdct_jpegenc_batch_tiles": _plan_getter,
    "mdct_jpegenc_batch_first_row": _indexed_getter,
    "mdct_jpegenc_batch_first_tile": _indexed_getter,
    "mdct_jpegenc_batch_row_image": _indexed_getter,
    "mdct_jpegenc_batch_row_last": _indexed_getter,
    "mdct_jpegenc_batch_row_marker": _indexed_getter,
    "mdct_jpegenc_batch_image_bytes": _plan_getter,
    "mdct_jpegenc_batch_bind": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mdct_jpegenc_batch_planes": (c_int, [c_void_p, c_void_p]),
    "mdct_jpegenc_batch_scan": (c_int, [c_void_p, c_void_p]),
    "mdct_jpegenc_batch_pack": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    "mdct_jpegenc_batch_last_error": (ctypes.c_char_p, []),
}

LIB = _lib.Library("mdct_jpegenc_batch", ("mdct_jpegenc_batch.h",), SIGNATURES)
load, LIB_PATH = LIB.load, LIB.path
