"""Reduced-size JPEG decoding (scale_denom 2, 4, 8) restated in numpy float64 from its rule: test
infrastructure, on top of tests/idct_reference.py.  Shares no code with simd_dct_amd.

  The block rule   a block decoded to N x N samples (N = 4, 2, 1) holds the mean over each (8/N) x (8/N) group of the mathematical
                   8x8 IDCT of its dequantised coefficients: clamp(rne(boxmean(IDCT(c * Q)) + 128), 0, 255).  This is libjpeg-turbo's
                   jidctred.c, not the low-frequency truncation of libjpeg 7 and later.
  The size rule    with m = 8 / scale_denom a component of sampling (h, v) starts at s = m and doubles s while s < 8 and
                   (hmax * m) % (h * s * 2) == 0 and (vmax * m) % (v * s * 2) == 0.
  Geometry         the image is ceil(W * m / 8) x ceil(H * m / 8); component i is ceil(W * h * s / (hmax * 8)) x
                   ceil(H * v * s / (vmax * 8)), cut from a plane of blocks_x * s x blocks_y * s; for the colour stage its sampling
                   factors are (h * s / m, v * s / m).
  kernel_f32       the kernel's own float32 arithmetic (simd_dct_amd/csrc/jpeg_idct_scaled.hip), operation for operation, to measure
                   how far it lands from the rule.
"""
import numpy as np

import idct_reference as R


def _ceil(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------ the block rule
def matrix(N):
    """A_N [N, 8]: A_N[n, k] = mean over the group x in [n * 8/N, (n + 1) * 8/N) of s_k cos((2x + 1) k pi / 16)"""
    return R.C.T.reshape(N, 8 // N, 8).mean(axis=1)


def boxmean(x, N):
    """[..., 8, 8] -> [..., N, N]: the mean over each (8/N) x (8/N) group"""
    g = 8 // N
    return np.asarray(x, dtype=np.float64).reshape(x.shape[:-2] + (N, g, N, g)).mean(axis=(-3, -1))


def scaled_pixels(c, q=None, N=4, level_shift=True):
    """-> (clamp(rne(boxmean(IDCT(c * Q)) + 128), 0, 255), the exact value, the tie window) of coefficient blocks [..., 8, 8];
    outputs [..., N, N].  The window is the full transform's (idct_reference.tie_window): a mean of values cannot be further off than
    they are."""
    z = R.dequantise(c, q)
    shift = 128.0 if level_shift else 0.0
    if N == 1:
        # every basis function but the DC's sums to zero over the block: the mean is z00 / 8, with no rounding at all in float64
        exact = z[..., :1, :1] / 8.0 + shift
    else:
        exact = boxmean(R.idct2(z), N) + shift
    return np.clip(R.rne(exact), 0, 255), exact, R.tie_window(z, shift)


# ------------------------------------------------------------------------------------------ planes <-> blocks
def plane_of(blks, bx, by, N):
    """[by * bx, N, N] block-row major -> [by * N, bx * N]"""
    if N == 1:
        return np.asarray(blks).reshape(by, bx)
    return np.asarray(blks).reshape(by, bx, N, N).transpose(0, 2, 1, 3).reshape(by * N, bx * N)


def blocks_of(plane, N):
    """inverse of plane_of: [by * N, bx * N] -> [by * bx, N, N]"""
    H, W = plane.shape
    return np.asarray(plane).reshape(H // N, N, W // N, N).transpose(0, 2, 1, 3).reshape(-1, N, N)


# ------------------------------------------------------------------------------------------ the size rule and the geometry
def block_size(h, v, hmax, vmax, d):
    m = 8 // d
    s = m
    while s < 8 and (hmax * m) % (h * s * 2) == 0 and (vmax * m) % (v * s * 2) == 0:
        s *= 2
    return s


def geometry(W, H, sampling, d):
    """-> ([(s, true width, true height, effective h, effective v)] per component, (image width, image height))"""
    assert d in (1, 2, 4, 8)
    m = 8 // d
    hmax, vmax = max(h for h, _ in sampling), max(v for _, v in sampling)
    out = []
    for h, v in sampling:
        s = block_size(h, v, hmax, vmax, d)
        out.append((s, _ceil(W * h * s, hmax * 8), _ceil(H * v * s, vmax * 8), h * s // m, v * s // m))
    return out, (_ceil(W * m, 8), _ceil(H * m, 8))


def component(coef_plane, q, s, width, height):
    """one component's coefficient plane [blocks_y * 8, blocks_x * 8] decoded at s x s per block and cropped to width x height
    -> (want, exact, window), each [height, width]"""
    by, bx = coef_plane.shape[0] // 8, coef_plane.shape[1] // 8
    c = R.blocks(coef_plane)
    if s == 8:
        want, exact, tol = R.u8_pixels(c, q)
    else:
        want, exact, tol = scaled_pixels(c, q, s)
    tol = np.broadcast_to(tol, exact.shape)
    return tuple(plane_of(a, bx, by, s)[:height, :width] for a in (want, exact, tol))


# ------------------------------------------------------------------------------------------ the kernel's float32 arithmetic
# jpeg_idct_scaled.hip: the table enters divided by 8 (exact), so the DC basis function is 1 and the others sqrt(8) * A_N[n, k];
# the level shift is 128 added to the dequantised DC term.  Rows n >= N/2 follow from the symmetry of the even and odd columns.
def _consts(N):
    return (np.sqrt(8.0) * matrix(N)).astype(np.float32)


def _pass4(z):
    """z: eight float32 arrays (index 4 unused) -> four"""
    a = _consts(4)
    g = a[0, 2] * z[2] + a[0, 6] * z[6]
    e0, e1 = z[0] + g, z[0] - g
    o0 = ((a[0, 1] * z[1] + a[0, 3] * z[3]) + a[0, 5] * z[5]) + a[0, 7] * z[7]
    o1 = ((a[1, 1] * z[1] + a[1, 3] * z[3]) + a[1, 5] * z[5]) + a[1, 7] * z[7]
    return [e0 + o0, e1 + o1, e1 - o1, e0 - o0]


def _pass2(z):
    a = _consts(2)
    o = ((a[0, 1] * z[1] + a[0, 3] * z[3]) + a[0, 5] * z[5]) + a[0, 7] * z[7]
    return [z[0] + o, z[0] - o]


def kernel_f32(c, q=None, N=4, level_shift=True):
    """-> the kernel's float32 value before its saturating convert, [..., N, N]"""
    c = np.asarray(c)
    q8 = (np.ones(64) if q is None else np.asarray(q, dtype=np.float64)).reshape(8, 8).astype(np.float32) * np.float32(0.125)
    z = c.astype(np.float32) * q8
    z[..., 0, 0] += np.float32(128.0 if level_shift else 0.0)
    assert z.dtype == np.float32
    if N == 1:
        return z[..., :1, :1]
    one = _pass4 if N == 4 else _pass2
    used = (0, 1, 2, 3, 5, 6, 7) if N == 4 else (0, 1, 3, 5, 7)  # the other columns of A_N are zero
    cols = {u: one([z[..., v, u] for v in range(8)]) for u in used}  # column pass: cols[u][n]
    zero = np.zeros(c.shape[:-2], dtype=np.float32)
    rows = [one([cols[u][n] if u in cols else zero for u in range(8)]) for n in range(N)]  # row pass: rows[n][m]
    out = np.stack([np.stack(r, axis=-1) for r in rows], axis=-2)
    assert out.dtype == np.float32
    return out


def kernel_u8(c, q=None, N=4, level_shift=True):
    """kernel_f32 through the kernel's convert: round to nearest even, saturate to 0..255"""
    return np.clip(np.rint(kernel_f32(c, q, N, level_shift)), 0, 255).astype(np.uint8)


def kernel_error_units(c, q=None, N=4, level_shift=True):
    """the largest distance of kernel_f32 from the rule over the blocks, in units of 2^-24 * sum|z| / 8 (idct_reference.TIE_K is in
    these units)"""
    _, exact, tol = scaled_pixels(c, q, N, level_shift)
    err = np.abs(kernel_f32(c, q, N, level_shift).astype(np.float64) - exact)
    return float((err / np.maximum(tol / R.TIE_K, 1e-300)).max())
