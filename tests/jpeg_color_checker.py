"""Test-side restatement of libjpeg-turbo's default decompression back end in numpy: "fancy" chroma upsampling and the integer
YCbCr -> RGB tables (jdsample.c, jdcolor.c), as DESIGN.md section 4.8 lists the rules.  Shares no code with simd_dct_amd.

A component enters at its true size (ceil(W * h / hmax) x ceil(H * v / vmax)); the padding of a decoder's MCU-aligned plane is not
part of it.  Every neighbour outside the component is its own edge sample; every shift is arithmetic."""
import numpy as np

FIX_CR_R, FIX_CB_B, FIX_CB_G, FIX_CR_G = 91881, 116130, 22554, 46802  # FIX(1.40200), FIX(1.77200), FIX(0.34414), FIX(0.71414)


def true_size(width, height, h, v, hmax, vmax):
    return -(-width * h // hmax), -(-height * v // vmax)


def factors(sampling):
    """[(h, v)] -> [(fh, fv)]; a fractional ratio raises ValueError (libjpeg refuses it too)"""
    hmax, vmax = max(h for h, _ in sampling), max(v for _, v in sampling)
    if any(hmax % h or vmax % v for h, v in sampling):
        raise ValueError("fractional sampling ratio")
    return [(hmax // h, vmax // v) for h, v in sampling]


def _shift(a, axis, d):
    """a shifted by d along axis with the edge sample repeated: out[i] = a[clamp(i + d)]"""
    n = a.shape[axis]
    idx = np.clip(np.arange(n) + d, 0, n - 1)
    return np.take(a, idx, axis=axis)


def _interleave(even, odd, axis):
    out = np.stack([even, odd], axis=axis + 1)
    shape = list(even.shape)
    shape[axis] *= 2
    return out.reshape(shape)


def upsample(plane, fh, fv, width, height):
    """one component at its true size -> [height, width] uint8 as libjpeg-turbo's default (fancy) upsampler produces it"""
    p = np.asarray(plane, dtype=np.int32)
    ch, cw = p.shape
    if (fh, fv) == (1, 1):
        out = p
    elif (fh, fv) == (1, 2):
        out = _interleave((3 * p + _shift(p, 0, -1) + 1) >> 2, (3 * p + _shift(p, 0, 1) + 2) >> 2, 0)
    elif fh == 2 and fv in (1, 2) and cw > 2:
        if fv == 2:
            s = _interleave(3 * p + _shift(p, 0, -1), 3 * p + _shift(p, 0, 1), 0)
            bias, shift = (8, 7), 4
        else:
            s = p
            bias, shift = (1, 2), 2
        out = _interleave((3 * s + _shift(s, 1, -1) + bias[0]) >> shift, (3 * s + _shift(s, 1, 1) + bias[1]) >> shift, 1)
    else:
        out = np.repeat(np.repeat(p, fv, axis=0), fh, axis=1)
    assert out.shape[0] >= height and out.shape[1] >= width
    return out[:height, :width].astype(np.uint8)


def ycc_to_rgb(y, cb, cr):
    """three [H, W] uint8 planes -> [H, W, 3] uint8 (jdcolor.c ycc_rgb_convert with its integer tables)"""
    y = np.asarray(y, dtype=np.int32)
    cb = np.asarray(cb, dtype=np.int32) - 128
    cr = np.asarray(cr, dtype=np.int32) - 128
    r = y + ((FIX_CR_R * cr + 32768) >> 16)
    g = y + ((-FIX_CB_G * cb - FIX_CR_G * cr + 32768) >> 16)
    b = y + ((FIX_CB_B * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def to_rgb(planes, sampling, width, height, colour="YCbCr"):
    """planes: one (grey) or three components at their true sizes; sampling: [(h, v)] of the frame; colour: 'YCbCr', 'RGB' (no
    transform) or 'grey' -> [H, W, 3] uint8"""
    if len(planes) == 1:
        y = np.asarray(planes[0], dtype=np.uint8)[:height, :width]
        return np.repeat(y[:, :, None], 3, axis=2)
    up = [upsample(p, fh, fv, width, height) for p, (fh, fv) in zip(planes, factors(sampling))]
    if colour == "RGB":
        return np.stack(up, axis=-1)
    return ycc_to_rgb(*up)
