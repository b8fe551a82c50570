"""Independent numpy restatement of the encoder's front stage (include/mdct_jpegenc.h): libjpeg-turbo's RGB -> YCbCr (jccolor.c),
its h2v1 / h2v2 downsampling (jcsample.c), the edge rules inside a component's true size and the padding beyond it.  Shares no code
with simd_dct_amd; the tests hold it against libjpeg (through Pillow) and the GPU kernel against it."""
import numpy as np

SAMPLING = {"4:4:4": [(1, 1), (1, 1), (1, 1)], "4:2:2": [(2, 1), (1, 1), (1, 1)], "4:2:0": [(2, 2), (1, 1), (1, 1)]}


def rgb_to_ycc(rgb):
    """uint8 [..., 3] -> (Y, Cb, Cr) int32 arrays, jccolor.c's integer rule"""
    r, g, b = (rgb[..., i].astype(np.int32) for i in range(3))  # every sum below stays under 2^24
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def true_sizes(width, height, sampling):
    hmax, vmax = max(h for h, _ in sampling), max(v for _, v in sampling)
    return [(-(-width * h // hmax), -(-height * v // vmax)) for h, v in sampling]


def downsample(full, fh, fv, cw, ch):
    """full-resolution component [H, W] -> [ch, cw]: the input is first extended to [fv * ch, fh * cw] by repeating its last column
    and row (expand_right_edge, the bottom row-group fill); h2v1 bias 0, 1, 0, 1 ..., h2v2 bias 1, 2, 1, 2 ... by output column"""
    H, W = full.shape
    ext = np.pad(full, ((0, fv * ch - H), (0, fh * cw - W)), mode="edge").astype(np.int32)
    if fh == 1 and fv == 1:
        return ext
    s = ext.reshape(ch, fv, cw, fh).sum(axis=(1, 3))
    col = np.arange(cw) & 1
    if fh == 2 and fv == 1:
        return (s + col) >> 1
    if fh == 2 and fv == 2:
        return (s + 1 + col) >> 2
    raise ValueError(f"no rule for {fh}x{fv}")


def planes(image, subsampling="4:2:0", layout="HWC", padded=None):
    """uint8 image [H, W, 3] (HWC), [3, H, W] (CHW) or [H, W] (grey) -> uint8 planes, each padded to `padded` [(width, height)] (default:
    its true size rounded up to multiples of 8) by repeating the component's own last true column and row"""
    image = np.asarray(image)
    if image.ndim == 2:
        comps, sampling = [image.astype(np.int32)], [(1, 1)]
    else:
        rgb = image if layout == "HWC" else np.moveaxis(image, 0, -1)
        comps, sampling = list(rgb_to_ycc(rgb)), SAMPLING[subsampling]
    H, W = comps[0].shape
    hmax, vmax = max(h for h, _ in sampling), max(v for _, v in sampling)
    out = []
    for k, ((h, v), (cw, ch)) in enumerate(zip(sampling, true_sizes(W, H, sampling))):
        p = downsample(comps[k], hmax // h, vmax // v, cw, ch)
        pw, ph = padded[k] if padded is not None else (-(-cw // 8) * 8, -(-ch // 8) * 8)
        out.append(np.pad(p, ((0, ph - ch), (0, pw - cw)), mode="edge").astype(np.uint8))
    return out
