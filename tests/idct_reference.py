"""The mathematical 8x8 DCT in float64, both directions, and what a transform with float32 arithmetic may differ from it by.

Test infrastructure.  numpy only: shares nothing with oracle/dct_oracle.c or the AAN factorisation the kernels use, so a slip that
the kernels and the checker carry together still shows here.

Blocks are float64 / integer arrays [..., 8, 8] indexed (v, u) for coefficients and (row, column) for samples.
  idct2 / dct2     the orthonormal 2-D transforms, from the defining cosine sums (T.81 A.3.3)
  u8_pixels        T.81's decoder output rule: clamp(rne(IDCT(c * Q) + 128), 0, 255)
  i16_samples      its int16 form: sat_i16(rne(IDCT(c * Q)))
  tie_window       per block, how far a float32 inverse may land from the exact value: TIE_K * 2^-24 * sum|z| / 8 with z = c * Q the
                   dequantised coefficients.  Outside the window of a .5 tie the rounded output must equal the exact rule's.
  fwd_coefficients the forward rule sat_i16(rne(DCT(x - shift) / Q)) with its window TIE_K_FWD * 2^-24 * sum|x - shift| / 8 / Q plus
                   4 * 2^-24 * |exact| for the quantiser's factor fl(fl(1/Q) * scale) and its one product; fwd_f32: no quantiser
  ieee1180_*       the IEEE 1180-1990 accuracy procedure: its generator, its coefficient blocks and its five statistical limits.
"""
import functools

import numpy as np

# the measured constant ("Inverse accuracy"): the checker's float32 inverse reached 15.5 units of 2^-24 * sum|z| / 8,
# twice that is the window
TIE_K = 32.0
# the same for the forward transform ("Forward accuracy"): the checker's float32 forward reached 16.24 units of
# 2^-24 * sum|x| / 8 on blocks of 2-3 nonzero samples (single impulses 14.2, both at row / column 7, where the AAN butterflies cancel
# most; dense blocks stay under 4.4, the 3.8 an earlier window of 8 was taken from).  Twice the measured maximum.
TIE_K_FWD = 32.5
# the round trips leave out blocks on a forward tie; on their own block lists (dense blocks: IEEE 1180 pixels, full-scale sign patterns,
# random) the forward error reached 3.96 of the same units, so their window keeps the 8 it had
TIE_K_FWD_RT = 8.0
ULP = 2.0 ** -24

_n = np.arange(8)
# C[k, n] = s_k cos((2n + 1) k pi / 16): row k is basis function k; C @ C.T == I
K = np.cos((2 * _n[None, :] + 1) * _n[:, None] * np.pi / 16.0)  # row 0 is exactly 1
_s = np.where(_n == 0, np.sqrt(1.0 / 8.0), 0.5)
C = _s[:, None] * K
# the 2-D scale s_v s_u, with s_0 s_0 = 1/8 exactly: a DC-only block's samples are exactly z00 / 8, .5 ties stay ties
S2 = np.outer(_s, _s)
S2[0, 0] = 0.125


def idct2(z):
    """orthonormal coefficients [..., 8 (v), 8 (u)] -> samples [..., 8 (row), 8 (column)]"""
    return np.einsum("vy,...vu,ux->...yx", K, np.asarray(z, dtype=np.float64) * S2, K)


def dct2(x):
    """samples -> orthonormal DCT-II coefficients"""
    return np.einsum("vy,...yx,ux->...vu", K, np.asarray(x, dtype=np.float64), K) * S2


def rne(x):
    return np.rint(x)  # numpy rounds halves to even


def sat_i16(x):
    return np.clip(x, -32768, 32767)


def dequantise(c, q=None):
    """c [..., 8, 8] integers, q: 64 entries in natural order (v * 8 + u) or None (all ones)"""
    c = np.asarray(c, dtype=np.float64)
    return c if q is None else c * np.asarray(q, dtype=np.float64).reshape(8, 8)


def tie_window(z, dc_shift=0.0):
    """[..., 1, 1]: TIE_K * 2^-24 * sum|z| / 8 per block.  dc_shift: an output level shift the arithmetic adds to the DC term before
    the transform (the 8-bit outputs add 128 that way: z00 + 8 * 128); it is part of what the float operations see."""
    z = np.array(z, dtype=np.float64)
    z[..., 0, 0] += 8.0 * dc_shift
    return TIE_K * ULP * np.abs(z).sum(axis=(-2, -1), keepdims=True) / 8.0


def tie_distance(exact):
    """distance of each exact value from the nearest .5 tie (where rounding changes)"""
    return np.abs(exact - np.floor(exact) - 0.5)


def i16_samples(c, q=None):
    """-> (sat_i16(rne(IDCT(c * Q))), the exact value, the tie window) of int16 coefficient blocks"""
    z = dequantise(c, q)
    exact = idct2(z)
    return sat_i16(rne(exact)), exact, tie_window(z)


def u8_pixels(c, q=None, level_shift=True):
    """-> (clamp(rne(IDCT(c * Q) + 128), 0, 255), exact, window); level_shift=False leaves the + 128 out"""
    z = dequantise(c, q)
    shift = 128.0 if level_shift else 0.0
    exact = idct2(z) + shift
    return np.clip(rne(exact), 0, 255), exact, tie_window(z, shift)


def f32_samples(z):
    """-> (exact IDCT, window) of float orthonormal coefficient blocks"""
    z = np.asarray(z, dtype=np.float64)
    return idct2(z), tie_window(z)


def decided(exact, tol, lo, hi):
    """where every value within tol of the exact one gives the same output clamp(rne(.), lo, hi): outside the window of a .5 tie, or
    saturated by more than the window"""
    tol = np.broadcast_to(tol, np.shape(exact))
    return np.clip(rne(exact - tol), lo, hi) == np.clip(rne(exact + tol), lo, hi)


def mismatches(got, want, exact, tol, lo, hi):
    """boolean mask of outputs that differ from the exact rule where the window leaves no doubt about it"""
    return (np.asarray(got, dtype=np.float64) != want) & decided(exact, tol, lo, hi)


I16_RANGE = (-32768, 32767)
U8_RANGE = (0, 255)


def fwd_coefficients(x, q=None, shift=0.0, k=None):
    """-> (sat_i16(rne(exact)), exact = DCT(x - shift) / Q, the window) of sample blocks x.  q: 64 entries in natural order, need not
    be integers, or None (no quantiser).  The window is the forward transform's (sum|x - shift| / 8 bounds every coefficient) carried
    through the division, plus two roundings of the quantiser's factor and one of its product: 4 units of 2^-24 |exact| cover them.
    k: the constant, TIE_K_FWD unless given."""
    xs = np.asarray(x, dtype=np.float64) - shift
    qq = 1.0 if q is None else np.asarray(q, dtype=np.float64).reshape(8, 8)
    exact = dct2(xs) / qq
    tol = ULP * ((TIE_K_FWD if k is None else k) * np.abs(xs).sum(axis=(-2, -1), keepdims=True) / 8.0 / np.abs(qq) + 4.0 * np.abs(exact))
    return sat_i16(rne(exact)), exact, tol


def fwd_f32(x):
    """-> (exact DCT, window [..., 1, 1]) of float sample blocks: |got - DCT(x)| <= TIE_K_FWD * 2^-24 * sum|x| / 8"""
    x = np.asarray(x, dtype=np.float64)
    return dct2(x), TIE_K_FWD * ULP * np.abs(x).sum(axis=(-2, -1), keepdims=True) / 8.0


def roundtrip(x, q=None, out="i16", level_shift=True):
    """the float64 composition rne(IDCT(sat_i16(rne(DCT(x) / Q)) * Q)) of sample blocks x (8-bit: x - 128 in, + 128 out, clamped).
    q None: no quantiser, IDCT(DCT(x)) rounded.  -> (want, exact, inverse window, skip [...]: blocks with a forward value inside the
    window of a .5 tie, whose quantised coefficient float32 arithmetic may round either way)"""
    shift = 128.0 if out == "u8" and level_shift else 0.0
    c, yq, tol_f = fwd_coefficients(x, q, shift, k=TIE_K_FWD_RT)
    if q is None:
        z = yq
        skip = np.zeros(yq.shape[:-2], dtype=bool)
    else:
        skip = ((tie_distance(yq) <= tol_f) & (np.abs(yq) < 32767.5)).any(axis=(-2, -1))
        z = c * np.asarray(q, dtype=np.float64).reshape(8, 8)
    exact = idct2(z) + shift
    want = np.clip(rne(exact), 0, 255) if out == "u8" else sat_i16(rne(exact))
    return want, exact, tie_window(z, shift), skip


# ------------------------------------------------------------------------------------------ planes <-> blocks
def blocks(plane):
    """[H, W] -> [H/8 * W/8, 8, 8], block-row major"""
    H, W = plane.shape
    return np.asarray(plane).reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8)


def plane(blks, W, H):
    """inverse of blocks()"""
    return np.asarray(blks).reshape(H // 8, W // 8, 8, 8).transpose(0, 2, 1, 3).reshape(H, W)


def tile_blocks(blks, n):
    """the first n blocks of blks repeated"""
    blks = np.asarray(blks)
    return np.concatenate([blks] * (-(-n // len(blks))))[:n]


# ------------------------------------------------------------------------------------------ IEEE 1180-1990
IEEE1180_CASES = [(256, 255, 1), (256, 255, -1), (5, 5, 1), (5, 5, -1), (300, 300, 1), (300, 300, -1)]
IEEE1180_LIMITS = dict(peak=1, pmse=0.06, omse=0.02, pme=0.015, ome=0.0015)


@functools.lru_cache(maxsize=None)
def _lcg(count):
    """the standard's generator from randx = 1: i = randx & 0x7ffffffe after each step randx = randx * 1103515245 + 12345 (32-bit)"""
    out = np.empty(count, dtype=np.int64)
    randx = 1
    for k in range(count):
        randx = (randx * 1103515245 + 12345) & 0xFFFFFFFF
        out[k] = randx & 0x7FFFFFFE
    out.flags.writeable = False
    return out


def ieee1180_pixels(L, H, sign=1, n=10000):
    """n blocks of integers in [-L, H] from the standard's generator (x = i / 0x7fffffff * (L + H + 1), value = floor(x) - L),
    times sign"""
    x = _lcg(n * 64) / float(0x7FFFFFFF) * float(L + H + 1)
    return (sign * (np.floor(x).astype(np.int64) - L)).reshape(n, 8, 8)


def ieee1180_coefficients(pixels):
    """the standard's test input: the double-precision DCT of the pixel blocks, rounded to the nearest integer, clipped to
    [-2048, 2047]"""
    return np.clip(np.floor(dct2(pixels) + 0.5), -2048, 2047).astype(np.int64)


def ieee1180_reference(coef):
    """the standard's reference output: double-precision IDCT rounded to the nearest integer, clipped to [-256, 255]"""
    return np.clip(np.floor(idct2(coef) + 0.5), -256, 255).astype(np.int64)


def ieee1180_stats(test, ref):
    """the five measures of the procedure over n blocks [n, 8, 8] of integer outputs"""
    e = np.asarray(test, dtype=np.float64) - np.asarray(ref, dtype=np.float64)
    return dict(peak=float(np.abs(e).max()), pmse=float((e * e).mean(0).max()), omse=float((e * e).mean()),
                pme=float(np.abs(e.mean(0)).max()), ome=float(abs(e.mean())))


def ieee1180_failures(test, ref):
    """the limits a result breaks, {measure: value}; empty when it passes"""
    s = ieee1180_stats(test, ref)
    return {k: v for k, v in s.items() if v > IEEE1180_LIMITS[k]}


# ------------------------------------------------------------------------------------------ adversarial coefficient blocks
def uniform_blocks(amps):
    """every coefficient = a"""
    return np.asarray(amps, dtype=np.float64)[:, None, None] * np.ones((1, 8, 8))


def worst_pixel_blocks(amps):
    """for each of the 64 pixels, the sign pattern of its basis row: every coefficient pushes that pixel the same way (the largest
    output |z|_1 coefficients can make)"""
    basis = np.einsum("vy,ux->yxvu", C, C).reshape(64, 8, 8)  # pixel (y, x) -> its weights over (v, u)
    sgn = np.where(basis >= 0, 1.0, -1.0)
    return (np.asarray(amps, dtype=np.float64)[:, None, None, None] * sgn[None]).reshape(-1, 8, 8)


def impulse_blocks(amps):
    """one nonzero coefficient at each of the 64 positions"""
    eye = np.eye(64).reshape(64, 8, 8)
    return (np.asarray(amps, dtype=np.float64)[:, None, None, None] * eye[None]).reshape(-1, 8, 8)


def sparse_blocks(rng, n, amp, k=3):
    """n blocks of k nonzero coefficients of random signs and magnitudes up to amp"""
    out = np.zeros((n, 64))
    for b in range(n):
        pos = rng.choice(64, size=k, replace=False)
        out[b, pos] = rng.integers(1, int(amp) + 1, size=k) * rng.choice([-1.0, 1.0], size=k)
    return out.reshape(n, 8, 8)


AMPS = np.array([1, 2, 3, 7, 100, 255, 1023, 2047, 4096, 16383, 32767], dtype=np.float64)


def adversarial_i16(rng, amps=AMPS, n_sparse=64):
    """integer coefficient blocks: uniform, worst-pixel sign patterns, the 64 impulses and sparse blocks at each amplitude, both
    signs (int16 range)"""
    b = [uniform_blocks(amps), worst_pixel_blocks(amps), impulse_blocks(amps)]
    b += [sparse_blocks(rng, n_sparse, a) for a in amps]
    b = np.concatenate(b)
    b = np.concatenate([b, -b])
    return np.clip(b, -32768, 32767).astype(np.int16)


# ------------------------------------------------------------------------------------------ assertions
def assert_exact_rule(got, want, exact, tol, rng_, what, min_decided=0.5):
    """got == want wherever the window decides the output; and enough of them decided that the check has teeth"""
    bad = mismatches(got, want, exact, tol, *rng_)
    dec = decided(exact, tol, *rng_)
    if bad.any():
        i = np.argwhere(bad)[0]
        b = tuple(i[:-2])
        raise AssertionError(f"{what}: {int(bad.sum())} outputs differ from the exact rule outside the tie window; first at block {b} "
                             f"pixel {tuple(i[-2:])}: got {np.asarray(got)[tuple(i)]}, want {want[tuple(i)]}, exact {exact[tuple(i)]!r}, "
                             f"window {float(np.broadcast_to(tol, exact.shape)[tuple(i)]):.3g}")
    assert dec.size == 0 or dec.mean() >= min_decided, (what, float(dec.mean()))


def check_planes(kind, srcs, gots, luts, level_shift=True, max_skip=0.1, min_decided=0.5):
    """each output plane against the float64 rule of its input plane.  kind: 'inv_i16' / 'inv_u8' (coefficients in), 'rt_i16' / 'rt_u8'
    (samples in, round trip; at most max_skip of the blocks may sit on a forward tie), 'f32' (inverse, within the window); 'fwd_i16' /
    'fwd_u8' (samples in, int16 coefficients out; 8-bit samples minus 128; at least min_decided of a plane's coefficients decided) and
    'fwd_f32' (forward, within the window)"""
    for j, (src, got, lut) in enumerate(zip(srcs, gots, luts)):
        W = src.shape[1]
        x, g = blocks(src), blocks(got)
        what = f"{kind} plane {j} {W}x{src.shape[0]}"
        if kind in ("f32", "fwd_f32"):
            exact, tol = f32_samples(x) if kind == "f32" else fwd_f32(x)
            err = np.abs(g.astype(np.float64) - exact)
            assert (err <= tol).all(), (what, float((err / np.maximum(tol, 1e-300)).max()) * (TIE_K if kind == "f32" else TIE_K_FWD))
            continue
        if kind in ("fwd_i16", "fwd_u8"):
            want, exact, tol = fwd_coefficients(x, lut, 128.0 if kind == "fwd_u8" else 0.0)
            assert_exact_rule(g, want, exact, tol, I16_RANGE, what, min_decided)
            continue
        if kind in ("inv_i16", "inv_u8"):
            want, exact, tol = i16_samples(x, lut) if kind == "inv_i16" else u8_pixels(x, lut, level_shift)
            skip = np.zeros(len(x), dtype=bool)
        else:
            want, exact, tol, skip = roundtrip(x, lut, "i16" if kind == "rt_i16" else "u8", level_shift)
            assert skip.mean() < max_skip, (what, float(skip.mean()))
        rng_ = I16_RANGE if kind.endswith("i16") else U8_RANGE
        assert_exact_rule(g[~skip], want[~skip], exact[~skip], tol[~skip], rng_, what)
