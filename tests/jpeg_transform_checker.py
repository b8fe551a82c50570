"""The numpy statement of the seven lossless JPEG transforms on quantised coefficient planes (include/mdct_jpegcoef.h), written from
the DCT's symmetries and shared by the CPU and GPU tests of test_jpeg_transcode.py.  Shares no code with simd_dct_amd.

Planes are int16 [blocks_y * 8, blocks_x * 8], level (v, u) of block (by, bx) at row by * 8 + v, column bx * 8 + u.
  flip_h     block (by, bx) -> (by, BX - 1 - bx), c'[v][u] = (-1)^u c[v][u]
  flip_v     block (by, bx) -> (BY - 1 - by, bx), c'[v][u] = (-1)^v c[v][u]
  transpose  block (by, bx) -> (bx, by),          c'[v][u] = c[u][v]
  rot180 = flip_h o flip_v; rot90 (clockwise) = transpose, then flip_h; rot270 = flip_h, then transpose; transverse = transpose, then rot180
"""
import numpy as np

OPS = ("flip_h", "flip_v", "transpose", "transverse", "rot90", "rot180", "rot270")
TRANSPOSING = ("transpose", "transverse", "rot90", "rot270")
# the pixel-domain operation each one equals
PIXELS = {
    "flip_h": lambda x: x[:, ::-1],
    "flip_v": lambda x: x[::-1, :],
    "transpose": lambda x: x.T,
    "transverse": lambda x: x[::-1, ::-1].T,
    "rot90": lambda x: np.rot90(x, -1),
    "rot180": lambda x: np.rot90(x, 2),
    "rot270": lambda x: np.rot90(x, 1),
}
# the source axes an operation mirrors
MIRRORED = {"flip_h": "x", "flip_v": "y", "rot180": "xy", "transverse": "xy", "rot90": "y", "rot270": "x", "transpose": ""}

_SIGN = np.array([1, -1] * 4, dtype=np.int64)


def _blocks(p):
    p = np.asarray(p)
    by, bx = p.shape[0] // 8, p.shape[1] // 8
    return p.reshape(by, 8, bx, 8).transpose(0, 2, 1, 3)  # [by, bx, v, u]


def _plane(b):
    by, bx = b.shape[:2]
    return np.ascontiguousarray(b.transpose(0, 2, 1, 3)).reshape(by * 8, bx * 8)


def _flip_h(b):
    return b[:, ::-1] * _SIGN[None, None, None, :]


def _flip_v(b):
    return b[::-1] * _SIGN[None, None, :, None]


def _transpose(b):
    return b.transpose(1, 0, 3, 2)


def transform(plane, op):
    """the plane after `op`; dtype kept (int16 wraps as the device's negation does)"""
    b = _blocks(plane).astype(np.int64) if np.issubdtype(np.asarray(plane).dtype, np.integer) else _blocks(plane)
    if op == "flip_h":
        b = _flip_h(b)
    elif op == "flip_v":
        b = _flip_v(b)
    elif op == "transpose":
        b = _transpose(b)
    elif op == "rot180":
        b = _flip_h(_flip_v(b))
    elif op == "rot90":
        b = _flip_h(_transpose(b))
    elif op == "rot270":
        b = _transpose(_flip_h(b))
    elif op == "transverse":
        b = _flip_h(_flip_v(_transpose(b)))
    else:
        raise ValueError(op)
    return _plane(b).astype(np.asarray(plane).dtype)


def trimmed(width, height, sampling, op):
    """(width, height) of the source after jpegtran -trim for `op`: a mirrored axis cropped to whole iMCUs"""
    hmax, vmax = max(h for h, _ in sampling), max(v for _, v in sampling)
    if op is not None and "x" in MIRRORED[op]:
        width -= width % (8 * hmax)
    if op is not None and "y" in MIRRORED[op]:
        height -= height % (8 * vmax)
    return width, height
