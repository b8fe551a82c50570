"""JPEG decoding at 1/2, 1/4 and 1/8 size (libmdct_jpegscale.so, include/mdct_jpegscale.h, jpeg_decode.scaled_inverse,
jpeg_decode.scaled_geometry, jpeg_decode.decode_jpeg(scale_denom=...)); DESIGN.md section 4.10.

CPU: the checker (tests/jpeg_scaled_checker.py: the block rule, the size rule and the geometry in float64) against Pillow's draft
decode; scaled_geometry against the formulas; the checker's RGB of files whose planes are known exactly against Pillow's; the kernel's
float32 arithmetic, restated in numpy, against the rule and its error constant; the C-ABI's refusals; the code object's kernels;
scale_denom = 1 leaves the new library alone.
GPU: the kernel through the C-ABI against the rule on adversarial and IEEE 1180 coefficient blocks; every lane, tile and tail case
with padded and odd pitches, offset outputs, canaries and the launch tally; one captured launch replayed; decode_jpeg's scaled
planes against the rule applied to its own coefficients and against Pillow; its RGB bit for bit Pillow's on IDCT-exact files and
the colour checker's on natural ones.

4:1:1 (sampling factor 4) is outside what jfif.read_jpeg reads, so no entropy decode of such a file exists to scale: its IDCT-exact
files enter after that stage, as their known coefficient planes through jpeg_decode.scaled_planes and jpeg_decode.to_rgb, and must
give Pillow's RGB bit for bit like the others."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import idct_reference as R
import jpeg_color_checker as C
import jpeg_decode_checker as K
import jpeg_scaled_checker as S
import jpeg_scan_encoder as E
from simd_dct_amd import _jpegscale_lib, api, synth
from simd_dct_amd import jpeg_decode as D

Image = pytest.importorskip("PIL.Image")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE_LIB = os.path.join(ROOT, "simd_dct_amd", "libmdct_jpegscale.so")

# every instantiation of k_idct_scaled<Mix>: 4, 2, 1 when all planes of a call share that n, 0 when they differ
KERNELS = {f"k_idct_scaled<{m}>" for m in (0, 1, 2, 4)}
DENOMS = (2, 4, 8)

SAMPLINGS = {
    "grey": [(1, 1)],
    "444": [(1, 1), (1, 1), (1, 1)],
    "422": [(2, 1), (1, 1), (1, 1)],
    "420": [(2, 2), (1, 1), (1, 1)],
    "440": [(1, 2), (1, 1), (1, 1)],
    "411": [(4, 1), (1, 1), (1, 1)],
    "mixed": [(2, 2), (2, 1), (1, 2)],
    "4x2": [(4, 2), (1, 1), (1, 1)],
    "3x1": [(3, 1), (1, 1), (1, 1)],
    "chroma-above-luma": [(1, 1), (2, 2), (2, 2)],
}
PILLOW_SUBSAMPLING = {"444": 0, "422": 1, "420": 2}


def _ceil(a, b):
    return -(-a // b)


def picture(W, H, seed, colour=True):
    if colour:
        return np.stack([synth.plane_u8_np(W, H, "photo", seed=seed + k) for k in range(3)], axis=-1)
    return synth.plane_u8_np(W, H, "photo", seed=seed)


def pillow_jpeg(img, **kw):
    buf = io.BytesIO()
    Image.fromarray(img, "L" if img.ndim == 2 else "YCbCr").save(buf, "JPEG", **kw)
    return buf.getvalue()


def natural_file(kind, W, H, seed, **kw):
    if kind == "grey":
        return pillow_jpeg(picture(W, H, seed, colour=False), **kw)
    return pillow_jpeg(picture(W, H, seed), subsampling=PILLOW_SUBSAMPLING[kind], **kw)


def pillow_draft(data, mode, d):
    """Pillow's decode at 1 / d in `mode` ('L', 'YCbCr' or 'RGB'); asserts that it ran at that scale and no other.  draft() takes
    the scale from min(W // requested width, H // requested height), which cannot reach d for an image with a side shorter than d
    (5x3 at 1/4 and 1/8): there libjpeg's scale_denom is set through the same three fields draft() sets."""
    im = Image.open(io.BytesIO(data))
    W, H = im.size
    if min(W, H) >= d:
        im.draft(mode, (max(1, W // d), max(1, H // d)))
    else:
        from PIL import ImageFile
        dec, e, o, a = im.tile[0]
        if a[0] == "RGB" and mode in ("L", "YCbCr"):
            im._mode = mode
            a = (mode, "")
        im.tile = [ImageFile._Tile(dec, (e[0], e[1], _ceil(e[2] - e[0], d) + e[0], _ceil(e[3] - e[1], d) + e[1]), o, a)]
        im._size = (_ceil(W, d), _ceil(H, d))
        im.decoderconfig = (d, 0)
    assert im.size == (_ceil(W, d), _ceil(H, d)) and im.decoderconfig == (d, 0), (im.size, im.decoderconfig, W, H, d)
    if mode == "RGB":
        im = im.convert("RGB")
    a = np.asarray(im)
    assert a.shape[:2] == (_ceil(H, d), _ceil(W, d))
    return a


def dc_file(W, H, sampling, seed=0):
    """a baseline file of DC-only blocks, every quantiser 8, random DCs: every IDCT, scaled or not, gives exactly dc + 128 throughout
    the block.  -> (file, its coefficient planes padded to the MCU grid, the quantiser tables per component)"""
    frame = dict(width=W, height=H, comps=list(sampling))
    rng = np.random.default_rng(seed)
    planes = []
    for rows, cols in E.plane_shapes(frame):
        p = np.zeros((rows, cols), dtype=np.int16)
        p[::8, ::8] = rng.integers(-128, 128, (rows // 8, cols // 8))
        planes.append(p)
    n = len(sampling)
    scans = [dict(comps=[(ci, min(ci, 1), min(ci, 1)) for ci in range(n)])]
    qt = [np.full(64, 8, dtype=np.uint16)] * n
    data, _ = E.encode_file(frame, scans, planes, E.ANNEX_K, qtables=qt)
    return data, planes, qt


def checker_planes(coef_planes, qtables, sampling, W, H, d):
    """the rule applied to coefficient planes -> ([(want, exact, window)] per component at its scaled true size, the geometry)"""
    geo, size = S.geometry(W, H, sampling, d)
    return [S.component(np.asarray(cp), q, g[0], g[1], g[2]) for cp, q, g in zip(coef_planes, qtables, geo)], geo, size


def colour_stage_inputs(planes, geo, size, d):
    """the planes and sampling factors libjpeg-turbo's colour stage sees: the effective factors; at 1/8 its triangle filters are off
    (jdsample.c: fancy upsampling only while the smallest block is larger than one sample), so a component that still needs
    upsampling there is replicated, which the colour checker is handed as a full-size component"""
    eff = [(g[3], g[4]) for g in geo]
    if d != 8 or len(planes) == 1:
        return planes, eff
    hmax, vmax = max(h for h, _ in eff), max(v for _, v in eff)
    out = [np.repeat(np.repeat(p, vmax // v, axis=0), hmax // h, axis=1)[:size[1], :size[0]] for p, (h, v) in zip(planes, eff)]
    return out, [(hmax, vmax)] * len(planes)


def checker_rgb(planes, geo, size, d, colour="YCbCr"):
    planes, eff = colour_stage_inputs(planes, geo, size, d)
    return C.to_rgb(planes, eff, size[0], size[1], colour)


# ------------------------------------------------------------------------------------------ CPU: the checker itself
@pytest.mark.parametrize("N", [4, 2])
def test_checker_box_mean_is_the_separable_matrix_form(N):
    A = S.matrix(N)
    zero = [4] if N == 4 else [2, 4, 6]
    assert np.abs(A[:, zero]).max() < 1e-15 and np.abs(np.delete(A, zero, axis=1)).min(axis=0).min() > 0.01
    z = np.random.default_rng(N).normal(size=(50, 8, 8)) * 300
    assert np.abs(S.boxmean(R.idct2(z), N) - np.einsum("nv,...vu,mu->...nm", A, z, A)).max() < 1e-10
    # N = 1: the mean of the whole IDCT is the DC term over 8
    assert np.abs(S.boxmean(R.idct2(z), 1)[..., 0, 0] - z[..., 0, 0] / 8).max() < 1e-10


_decoded = {}


def decoded_natural(kind, W, H, quality):
    """(file, frame, quantiser tables, coefficient planes) of a Pillow file with one restart interval per MCU row, decoded once"""
    key = (kind, W, H, quality)
    if key not in _decoded:
        data = natural_file(kind, W, H, seed=W + quality, quality=quality, restart_marker_rows=1)
        frame, qt, _ = K.parse(data)
        planes, status, _ = K.decode(data)
        assert all(s == 0 for st in status for s in st)
        _decoded[key] = (data, frame, qt, planes)
    return _decoded[key]


@pytest.mark.parametrize("size", [(17, 9), (67, 45), (128, 96)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", ["grey", "444", "420"])
def test_checker_against_pillow(kind, size):
    W, H = size
    for quality in (50, 75, 95):
        data, frame, qt, planes = decoded_natural(kind, W, H, quality)
        sampling = [(h, v) for _, h, v, _ in frame["components"]]
        assert sampling == SAMPLINGS[kind]
        tables = [qt[tq] for _, _, _, tq in frame["components"]]
        for d in DENOMS:
            ref = pillow_draft(data, "L" if kind == "grey" else "YCbCr", d)
            comps, geo, (sw, sh) = checker_planes(planes, tables, sampling, W, H, d)
            assert ref.shape[:2] == (sh, sw)
            for ci, ((want, _, _), g) in enumerate(zip(comps, geo)):
                # none of these components is upsampled: its effective factors are the largest
                assert (g[3], g[4]) == (max(x[3] for x in geo), max(x[4] for x in geo)) and want.shape == (sh, sw)
                got = ref if ref.ndim == 2 else ref[:, :, ci]
                worst = int(np.abs(got.astype(int) - want).max())
                assert worst <= 1, (kind, size, quality, d, ci, worst)
            if kind == "420" and d == 2:
                # the size rule: chroma stays at the full 8x8 IDCT, which is what Pillow's planes are
                assert [g[0] for g in geo] == [4, 8, 8]
                for ci in (1, 2):
                    full = S.plane_of(R.u8_pixels(R.blocks(planes[ci]), tables[ci])[0], planes[ci].shape[1] // 8, planes[ci].shape[0] // 8, 8)
                    assert np.array_equal(full[:sh, :sw], comps[ci][0])


@pytest.mark.parametrize("name", ["grey", "444", "422", "420", "440", "411"])
def test_checker_rgb_equals_pillow_on_idct_exact_files(name):
    sampling = SAMPLINGS[name]
    for W, H in ((17, 9), (37, 29), (5, 3)):
        data, planes, qt = dc_file(W, H, sampling, seed=100 * W + H)
        for d in DENOMS:
            comps, geo, size = checker_planes(planes, qt, sampling, W, H, d)
            got = checker_rgb([c[0].astype(np.uint8) for c in comps], geo, size, d)
            want = pillow_draft(data, "RGB", d)
            assert np.array_equal(got, want), (name, W, H, d, np.argwhere(got != want)[:4].tolist())


# ------------------------------------------------------------------------------------------ CPU: scaled_geometry
@pytest.mark.parametrize("name", ["444", "422", "420", "440", "411", "mixed", "4x2", "3x1", "chroma-above-luma"])
def test_scaled_geometry_against_the_formulas(name):
    sampling = SAMPLINGS[name]
    hmax, vmax = max(h for h, _ in sampling), max(v for _, v in sampling)
    sizes = [(w, h) for w in range(1, 18) for h in range(1, 18)] + [(37, 29), (65535, 65535), (65535, 1), (1, 65535)]
    for W, H in sizes:
        info = dict(width=W, height=H, components=[dict(id=i + 1, h=h, v=v, tq=min(i, 1)) for i, (h, v) in enumerate(sampling)])
        for d in (1, 2, 4, 8):
            m = 8 // d
            got, size = D.scaled_geometry(info, d)
            want, wsize = S.geometry(W, H, sampling, d)
            assert [tuple(g) for g in got] == want and tuple(size) == wsize == (_ceil(W * m, 8), _ceil(H * m, 8))
            for (s, tw, th, eh, ev), (h, v) in zip(got, sampling):
                assert s in (1, 2, 4, 8) and s >= m and (d > 1 or s == 8)
                assert (h * s) % m == 0 and (v * s) % m == 0 and (eh, ev) == (h * s // m, v * s // m)
                assert (tw, th) == (_ceil(W * h * s, hmax * 8), _ceil(H * v * s, vmax * 8))
                # the colour stage derives the same component size from the scaled image and the effective factors
                assert (tw, th) == C.true_size(size[0], size[1], eh, ev, hmax, vmax)
            assert max(g[3] for g in got) == hmax and max(g[4] for g in got) == vmax
    with pytest.raises(ValueError):
        D.scaled_geometry(info, 3)


def test_size_rule_examples():
    geo = lambda name, d: [g[0] for g in S.geometry(64, 64, SAMPLINGS[name], d)[0]]  # noqa: E731
    assert geo("420", 2) == [4, 8, 8] and geo("420", 4) == [2, 4, 4] and geo("420", 8) == [1, 2, 2]
    assert geo("422", 2) == [4, 4, 4]  # the vertical test fails
    assert geo("411", 2) == [4, 4, 4] and geo("444", 8) == [1, 1, 1] and geo("chroma-above-luma", 4) == [4, 2, 2]


# ------------------------------------------------------------------------------------------ CPU: the kernel's arithmetic
_inputs = {}


def rule_inputs():
    """{name: (coefficient blocks int16 [n, 8, 8], table or None)}: the adversarial blocks and the IEEE 1180 blocks with no table, the
    IEEE blocks quantised by the Annex K luma table with that table"""
    if not _inputs:
        ieee = np.concatenate([R.ieee1180_coefficients(R.ieee1180_pixels(L, H, sg)) for L, H, sg in R.IEEE1180_CASES])
        lut = synth.JPEG_LUMA.astype(np.float64)
        _inputs["adversarial"] = (R.adversarial_i16(np.random.default_rng(1180)), None)
        _inputs["ieee1180"] = (ieee.astype(np.int16), None)
        _inputs["ieee1180-annex-k"] = (R.rne(ieee / lut.reshape(8, 8)).astype(np.int16), lut)
        for c, _ in _inputs.values():
            c.flags.writeable = False
    return _inputs


@pytest.mark.parametrize("N", [4, 2, 1])
def test_kernel_arithmetic_restated_in_float32(N):
    """the kernel's float32 operations in numpy: inside the window everywhere, and the figure DESIGN.md section 4.10 quotes"""
    worst = 0.0
    for name, (c, lut) in rule_inputs().items():
        for shift in (True, False):
            want, exact, tol = S.scaled_pixels(c, lut, N, shift)
            got = S.kernel_u8(c, lut, N, shift)
            units = S.kernel_error_units(c, lut, N, shift)
            worst = max(worst, units)
            print(f"n={N} {name} level_shift={shift}: {units:.2f} units of 2^-24 sum|z| / 8, decided {R.decided(exact, tol, 0, 255).mean():.3f}")
            if N == 1:
                assert np.array_equal(got, want), name
            else:
                R.assert_exact_rule(got, want, exact, tol, R.U8_RANGE, f"float32 restatement n={N} {name}", min_decided=0.5)
    assert worst <= 16.0, worst  # half the window TIE_K


# ------------------------------------------------------------------------------------------ CPU: the C-ABI refuses without a device
def _plane(coef, pitch_coef, px, pitch_px, bx, by, lut=None, n=4, rep=(0, 0)):
    return _jpegscale_lib.Plane(coef, pitch_coef, px, pitch_px, bx, by, None if lut is None else lut.ctypes.data, n, rep[0], rep[1])


def _call(planes, n_planes, level_shift=1):
    lib = _jpegscale_lib.load()
    arr = None if planes is None else (_jpegscale_lib.Plane * max(1, len(planes)))(*planes)
    return lib.mdct_jpegscale_inv_i16_u8(arr, n_planes, level_shift, None), lib.mdct_jpegscale_last_error().decode()


def test_cabi_refusals_without_device():
    A, B = 1 << 40, 1 << 44  # addresses far apart; nothing on the device is dereferenced
    good = np.full(64, 3.0, dtype=np.float32)

    def lut_with(i, v):
        t = good.copy()
        t[i] = v
        return t

    tables = [lut_with(0, 0.0), lut_with(63, np.inf), lut_with(17, np.nan), lut_with(5, -np.inf)]
    ok = _plane(A, 512, B, 256, 64, 32, good, 4)
    in_bytes = 2 * ((32 * 8 - 1) * 512 + 512)
    cases = {
        "null planes": (None, 1),
        "no planes": ([ok], 0),
        "five planes": ([ok] * 5, 5),
        "level shift 2": ([ok], 1, 2),
        "level shift -1": ([ok], 1, -1),
        "null coef": ([_plane(0, 512, B, 256, 64, 32)], 1),
        "null px": ([_plane(A, 512, 0, 256, 64, 32)], 1),
        "n 8": ([_plane(A, 512, B, 512, 64, 32, n=8)], 1),
        "n 3": ([_plane(A, 512, B, 256, 64, 32, n=3)], 1),
        "n 0": ([_plane(A, 512, B, 256, 64, 32, n=0)], 1),
        "second plane n 8": ([ok, _plane(A + (1 << 30), 512, B + (1 << 30), 512, 64, 32, n=8)], 2),
        "no blocks across": ([_plane(A, 512, B, 256, 0, 32)], 1),
        "no blocks down": ([_plane(A, 512, B, 256, 64, 0)], 1),
        "8193 blocks across": ([_plane(A, 8193 * 8, B, 8193 * 4, 8193, 1)], 1),
        "8193 blocks down": ([_plane(A, 512, B, 256, 64, 8193)], 1),
        "coefficient pitch short": ([_plane(A, 504, B, 256, 64, 32)], 1),
        "coefficient pitch not a multiple of 8": ([_plane(A, 516, B, 256, 64, 32)], 1),
        "coefficient pointer unaligned": ([_plane(A + 8, 512, B, 256, 64, 32)], 1),
        "output pitch short n 4": ([_plane(A, 512, B, 255, 64, 32)], 1),
        "output pitch short n 2": ([_plane(A, 512, B, 127, 64, 32, n=2)], 1),
        "output pitch short n 1": ([_plane(A, 512, B, 63, 64, 32, n=1)], 1),
        "replication 5": ([_plane(A, 512, B, 512, 64, 32, n=1, rep=(5, 1))], 1),
        "replication -1": ([_plane(A, 512, B, 512, 64, 32, n=1, rep=(1, -1))], 1),
        "replication with n 4": ([_plane(A, 512, B, 512, 64, 32, n=4, rep=(2, 1))], 1),
        "replication with n 2": ([_plane(A, 512, B, 512, 64, 32, n=2, rep=(1, 2))], 1),
        "output pitch short of the replicated row": ([_plane(A, 512, B, 127, 64, 32, n=1, rep=(2, 1))], 1),
        "replicated rows reach the coefficients": ([_plane(A, 512, A - 64 * 64 + 1, 64, 64, 32, n=1, rep=(1, 2))], 1),
        "output over its coefficients": ([_plane(A, 512, A + 4096, 256, 64, 32)], 1),
        "output ends in its coefficients": ([_plane(A, 512, A - (127 * 256 + 256) + 1, 256, 64, 32)], 1),
        "output starts in the coefficients' last byte": ([_plane(A, 512, A + in_bytes - 1, 256, 64, 32)], 1),
        "output over another plane's coefficients": ([ok, _plane(A + (1 << 30), 512, A + 100, 256, 64, 32)], 2),
        "another plane's output over these coefficients": ([_plane(A, 512, B, 256, 64, 32), _plane(A + (1 << 30), 512, A + 100, 256, 64, 32)], 2),
    }
    for i, t in enumerate(tables):
        cases[f"table {i}"] = ([_plane(A, 512, B, 256, 64, 32, t)], 1)
        cases[f"table {i} of the second plane"] = ([ok, _plane(A + (1 << 30), 512, B + (1 << 30), 256, 64, 32, t, 2)], 2)
    for name, args in cases.items():
        rc, msg = _call(*args)
        assert rc == 1, (name, rc, msg)  # MDCT_INVALID_PARAMETER
        assert msg, name
    # the neighbours of the overlap cases that do not overlap are not refused for it (they would launch: not called here)


def test_code_object_holds_the_planned_instantiations():
    from test_kernel_coverage import code_object_kernels
    names, n_objects = code_object_kernels(lib=SCALE_LIB)
    assert n_objects == 1 and names == KERNELS, sorted(names ^ KERNELS)


def test_other_libraries_keep_their_kernels():
    """the scaled inverse lives in its own library: libmdct_hip.so and the colour library hold no kernel of it"""
    from test_kernel_coverage import code_object_kernels
    for lib in ("libmdct_hip.so", "libmdct_jpegcolor.so"):
        names, _ = code_object_kernels(lib=os.path.join(ROOT, "simd_dct_amd", lib))
        assert not any("idct_scaled" in n for n in names), lib


# ------------------------------------------------------------------------------------------ CPU: the unchanged path
_UNTOUCHED = """
import sys
from simd_dct_amd import jpeg_decode as D
info = dict(width=17, height=9, components=[dict(id=1, h=2, v=2, tq=0), dict(id=2, h=1, v=1, tq=1), dict(id=3, h=1, v=1, tq=1)])
assert D.scaled_geometry(info, 2)[1] == (9, 5)
{body}
assert 'simd_dct_amd._jpegscale_lib' not in sys.modules, 'scale_denom = 1 loaded the scaled library'
print('untouched')
"""


def _run_untouched(body, timeout):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-c", _UNTOUCHED.format(body=body)], capture_output=True, text=True, env=env, cwd=ROOT, timeout=timeout)
    assert p.returncode == 0 and p.stdout.strip().endswith("untouched"), (p.returncode, p.stdout[-500:], p.stderr[-2000:])


def test_bad_scale_denom_is_refused_and_the_module_imports_without_the_library():
    data, _, _ = dc_file(16, 16, SAMPLINGS["420"])
    for bad in (3, 0, 16, -2, 2.5, None):
        with pytest.raises(ValueError):
            D.decode_jpeg(data, scale_denom=bad)
    _run_untouched("", 120)


# ------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    torch.cuda.set_device(0)
    api.init(0)
    return torch


def ran_exactly(torch, want):
    torch.cuda.synchronize()
    ran = {k: v for k, v in api.kernel_counts().items() if k.startswith("k_idct_scaled")}
    assert ran == want, (want, ran)


def coef_plane_of(blks, bx):
    """int16 blocks [n, 8, 8] -> (a plane bx blocks wide holding them in block-row order, the last row filled up by repeating them;
    the blocks of the plane)"""
    by = _ceil(len(blks), bx)
    b = R.tile_blocks(blks, bx * by)
    return np.ascontiguousarray(R.plane(b, bx * 8, by * 8)), b, by


@pytest.mark.gpu
@pytest.mark.parametrize("N", [4, 2, 1])
def test_kernel_against_the_rule(gpu, N):
    torch = gpu
    for name, (c, lut) in rule_inputs().items():
        bx = 250
        plane, blks, by = coef_plane_of(c, bx)
        coef = torch.from_numpy(plane).cuda()
        for shift in (True, False):
            px = torch.empty((by * N, bx * N), dtype=torch.uint8, device="cuda")
            api.kernel_counts_reset()
            D.scaled_inverse([(px, coef, bx, by, lut, N)], level_shift=shift)
            ran_exactly(torch, {f"k_idct_scaled<{N}>": 1})
            got = S.blocks_of(px.cpu().numpy(), N)
            want, exact, tol = S.scaled_pixels(blks, lut, N, shift)
            what = f"n={N} {name} level_shift={shift}"
            if N == 1:
                assert np.array_equal(got, want), what
            else:
                R.assert_exact_rule(got, want, exact, tol, R.U8_RANGE, what, min_decided=0.5)
            # and the float32 restatement the error constant was measured on is the kernel's arithmetic
            mine = S.kernel_u8(blks, lut, N, shift)
            assert np.array_equal(got, mine), (what, int((got != mine).sum()))


def _random_coefficients(rng, bx, by):
    """natural-looking quantised blocks: a large DC, ACs that fall off"""
    scale = 400.0 / (1.0 + np.add.outer(np.arange(8), np.arange(8))) ** 2
    c = rng.normal(size=(by * bx, 8, 8)) * scale
    c[:, 0, 0] = rng.integers(-60, 60, by * bx)
    return np.rint(c).astype(np.int16)


def _checked_call(torch, specs, level_shift, seed):
    """one scaled_inverse call over planes specs = [(bx, by, n, extra coefficient pitch, output pitch or None, output offset, table)]
    into canary-filled buffers with a guard after each; the rule decides every output, nothing else is written"""
    rng = np.random.default_rng(seed)
    planes, checks = [], []
    for bx, by, n, cpad, opitch, ooff, lut in specs:
        blks = _random_coefficients(rng, bx, by)
        host = R.plane(blks, bx * 8, by * 8)
        cbuf = torch.zeros((by * 8, bx * 8 + cpad), dtype=torch.int16, device="cuda")
        coef = cbuf[:, :bx * 8]
        coef.copy_(torch.from_numpy(np.ascontiguousarray(host)).cuda())
        opitch = bx * n if opitch is None else opitch
        buf = torch.full((ooff + by * n * opitch + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
        px = torch.as_strided(buf, (by * n, bx * n), (opitch, 1), ooff)
        planes.append((px, coef, bx, by, lut, n))
        checks.append((blks, buf, px, bx, by, n, lut))
    api.kernel_counts_reset()
    D.scaled_inverse(planes, level_shift=level_shift)
    ns = {s[2] for s in specs}
    ran_exactly(torch, {f"k_idct_scaled<{ns.pop() if len(ns) == 1 else 0}>": 1})
    for blks, buf, px, bx, by, n, lut in checks:
        want, exact, tol = S.scaled_pixels(blks, lut, n, level_shift)
        got = S.blocks_of(px.cpu().numpy(), n)
        what = f"{bx}x{by} blocks n={n} of {specs}"
        if n == 1:
            assert np.array_equal(got, want), what
        else:
            R.assert_exact_rule(got, want, exact, tol, R.U8_RANGE, what, min_decided=0.5)
        assert np.array_equal(got, S.kernel_u8(blks, lut, n, level_shift)), what
        assert int((buf != 0xA5).sum()) == int((px != 0xA5).sum()), "bytes written outside the plane: " + what


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, 2, 1])
def test_cabi_shapes_pitches_offsets_and_canaries(gpu, n):
    lut = synth.JPEG_LUMA
    for bx in (1, 2, 3, 63, 64, 65, 129):
        for by in (1, 2, 5):
            w = bx * n
            seed = 1000 * bx + 10 * by + n
            _checked_call(gpu, [(bx, by, n, 0, None, 0, lut)], True, seed)  # both pitches equal to the width
            _checked_call(gpu, [(bx, by, n, 64, w + 16, 0, None)], False, seed + 1)  # both padded; no table, no level shift
            _checked_call(gpu, [(bx, by, n, 8, (w + 3) | 1, 1, None)], True, seed + 2)  # odd output pitch, output 1 byte in
            _checked_call(gpu, [(bx, by, n, 0, w, 3, lut)], False, seed + 3)  # output 3 bytes in
    # wider than one wave's 64 * (4 / n) blocks, with a tail
    _checked_call(gpu, [(64 * (4 // n) * 2 + 5, 3, n, 0, None, 0, lut)], True, 77)


@pytest.mark.gpu
def test_cabi_planes_of_different_sizes_and_n_in_one_call(gpu):
    lut, chroma = synth.JPEG_LUMA, synth.JPEG_CHROMA
    _checked_call(gpu, [(129, 5, 4, 0, None, 0, lut), (65, 3, 2, 8, 65 * 2 + 5, 1, chroma), (33, 2, 1, 0, None, 3, None)], True, 5)
    _checked_call(gpu, [(3, 1, 1, 0, None, 0, lut), (130, 2, 4, 0, None, 0, None), (257, 1, 2, 0, None, 0, chroma), (1, 1, 2, 0, 7, 1, lut)], False, 6)
    _checked_call(gpu, [(70, 2, 2, 0, None, 0, lut), (35, 1, 2, 0, None, 0, chroma), (35, 1, 2, 0, None, 0, chroma)], True, 7)  # one n: <2>


@pytest.mark.gpu
def test_cabi_replicated_output(gpu):
    """n = 1 with every sample written rep_x x rep_y times (libjpeg's plain upsampling at 1/8), next to planes without"""
    torch = gpu
    for (bx, by), (rx, ry), ooff, pad in (((1, 1), (2, 1), 0, 0), ((3, 2), (1, 2), 1, 3), ((65, 5), (2, 2), 3, 0), ((257, 2), (4, 1), 0, 5), ((70, 3), (4, 4), 0, 0)):
        rng = np.random.default_rng(bx + rx)
        blks = _random_coefficients(rng, bx, by)
        coef = torch.from_numpy(np.ascontiguousarray(R.plane(blks, bx * 8, by * 8))).cuda()
        pitch = bx * rx + pad
        buf = torch.full((ooff + by * ry * pitch + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
        px = torch.as_strided(buf, (by * ry, bx * rx), (pitch, 1), ooff)
        other = torch.empty((by * 4, bx * 4), dtype=torch.uint8, device="cuda")
        api.kernel_counts_reset()
        D.scaled_inverse([(px, coef, bx, by, synth.JPEG_LUMA, 1, (rx, ry)), (other, coef, bx, by, synth.JPEG_LUMA, 4)])
        ran_exactly(torch, {"k_idct_scaled<0>": 1})
        want = S.plane_of(S.scaled_pixels(blks, synth.JPEG_LUMA, 1)[0], bx, by, 1).astype(np.uint8)
        assert np.array_equal(px.cpu().numpy(), np.repeat(np.repeat(want, ry, axis=0), rx, axis=1)), (bx, by, rx, ry)
        assert int((buf != 0xA5).sum()) == int((px != 0xA5).sum()), (bx, by, rx, ry)
        assert np.array_equal(S.blocks_of(other.cpu().numpy(), 4), S.kernel_u8(blks, synth.JPEG_LUMA, 4))


@pytest.mark.gpu
def test_cabi_captured_and_replayed_on_new_coefficients(gpu):
    torch = gpu
    specs = [(240, 34, 4, synth.JPEG_LUMA), (120, 17, 2, synth.JPEG_CHROMA), (120, 17, 1, None)]
    coefs = [torch.zeros((by * 8, bx * 8), dtype=torch.int16, device="cuda") for bx, by, _, _ in specs]
    outs = [torch.empty((by * n, bx * n), dtype=torch.uint8, device="cuda") for bx, by, n, _ in specs]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        D.scaled_inverse([(o, c, bx, by, lut, n) for o, c, (bx, by, n, lut) in zip(outs, coefs, specs)], stream=s)
    for seed in (2, 3):
        rng = np.random.default_rng(seed)
        blks = [_random_coefficients(rng, bx, by) for bx, by, _, _ in specs]
        for c, b, (bx, by, _, _) in zip(coefs, blks, specs):
            c.copy_(torch.from_numpy(np.ascontiguousarray(R.plane(b, bx * 8, by * 8))).cuda())
        for o in outs:
            o.fill_(0)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for o, b, (bx, by, n, lut) in zip(outs, blks, specs):
            assert np.array_equal(S.blocks_of(o.cpu().numpy(), n), S.kernel_u8(b, lut, n, True)), (seed, n)
            want, exact, tol = S.scaled_pixels(b, lut, n, True)
            R.assert_exact_rule(S.blocks_of(o.cpu().numpy(), n), want, exact, tol, R.U8_RANGE, f"replay {seed} n={n}", min_decided=0.5)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["grey", "444", "422", "420"])
def test_decode_scaled_planes(gpu, kind):
    for W, H in ((67, 45), (128, 96)):
        for kw in (dict(restart_marker_rows=1), dict()):
            data = natural_file(kind, W, H, seed=W + len(kw), quality=85, **kw)
            frame, qt, _ = K.parse(data)
            sampling = [(h, v) for _, h, v, _ in frame["components"]]
            tables = [qt[tq] for _, _, _, tq in frame["components"]]
            for d in DENOMS:
                planes, coefs = D.decode_jpeg(data, scale_denom=d, coefficients=True)
                comps, geo, (sw, sh) = checker_planes([c.cpu().numpy() for c in coefs], tables, sampling, W, H, d)
                assert len(planes) == len(comps)
                for ci, (p, (want, exact, tol), g) in enumerate(zip(planes, comps, geo)):
                    got = p.cpu().numpy()
                    assert got.shape == (g[2], g[1]) == want.shape, (kind, W, H, d, ci)
                    R.assert_exact_rule(got, want, exact, tol, R.U8_RANGE, f"{kind} {W}x{H} {kw} 1/{d} component {ci}", min_decided=0.5)
                ref = pillow_draft(data, "L" if kind == "grey" else "YCbCr", d)
                luma = planes[0].cpu().numpy()
                assert luma.shape == (sh, sw)
                assert int(np.abs(luma.astype(int) - (ref if ref.ndim == 2 else ref[:, :, 0])).max()) <= 1, (kind, W, H, kw, d)
            # the coefficient planes are the full ones, whatever the scale
            full = D.decode_jpeg(data, coefficients=True)[1]
            assert all(bool((a == b).all()) for a, b in zip(coefs, full))


def _hwc(img, layout):
    return img if layout == "HWC" else np.transpose(img, (1, 2, 0))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["HWC", "CHW"])
def test_decode_scaled_rgb_equals_pillow_on_idct_exact_files(gpu, layout):
    torch = gpu
    for name in ("444", "422", "420", "440", "411", "grey"):
        sampling = SAMPLINGS[name]
        for W, H in ((17, 9), (37, 29), (5, 3)):
            data, coef_planes, qt = dc_file(W, H, sampling, seed=7 * W + H)
            for d in DENOMS:
                want = pillow_draft(data, "RGB", d)
                if name == "411":
                    # read_jpeg takes sampling factors 1 and 2: the stages after the entropy decode, from the file's known coefficients
                    info = dict(width=W, height=H, qtables={0: qt[0], 1: qt[1]}, colorspace="YCbCr",
                                components=[dict(id=i + 1, h=h, v=v, tq=min(i, 1)) for i, (h, v) in enumerate(sampling)])
                    planes = D.scaled_planes(info, [torch.from_numpy(p).cuda() for p in coef_planes], d, replicate=True)
                    sw, sh = D.scaled_geometry(info, d)[1]
                    got = D.to_rgb(planes, D.colour_sampling(info, d)[0], sw, sh, layout=layout)
                else:
                    got = D.decode_jpeg(data, mode="RGB", layout=layout, scale_denom=d)
                sh, sw = want.shape[:2]
                assert tuple(got.shape) == ((sh, sw, 3) if layout == "HWC" else (3, sh, sw)), (name, W, H, d)
                g = _hwc(got.cpu().numpy(), layout)
                assert np.array_equal(g, want), (name, W, H, d, layout, np.argwhere(g != want)[:4].tolist())


NATURAL = [  # (kind, size, save options)
    ("420", (61, 37), dict(quality=75, restart_marker_rows=1)),
    ("444", (100, 52), dict(quality=75)),
    ("422", (100, 52), dict(quality=75, restart_marker_blocks=5)),
    ("420", (333, 101), dict(quality=90)),
    ("422", (37, 29), dict(quality=5)),
    ("grey", (61, 37), dict(quality=75)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,size,kw", NATURAL, ids=[f"{k}-{s[0]}x{s[1]}" for k, s, _ in NATURAL])
def test_decode_scaled_rgb_on_natural_files(gpu, kind, size, kw):
    W, H = size
    data = natural_file(kind, W, H, seed=41 + W, **kw)
    sampling = SAMPLINGS[kind]
    for d in DENOMS:
        geo, (sw, sh) = S.geometry(W, H, sampling, d)
        planes = [p.cpu().numpy() for p in D.decode_jpeg(data, scale_denom=d)]
        assert [p.shape for p in planes] == [(g[2], g[1]) for g in geo]
        planes, eff = colour_stage_inputs(planes, geo, (sw, sh), d)
        for layout in ("HWC", "CHW"):
            got = _hwc(D.decode_jpeg(data, mode="RGB", layout=layout, scale_denom=d).cpu().numpy(), layout)
            assert np.array_equal(got, C.to_rgb(planes, eff, sw, sh, "grey" if kind == "grey" else "YCbCr")), (d, layout)
        assert int(np.abs(got.astype(int) - pillow_draft(data, "RGB", d)).max()) <= 3, d
        if kind != "grey":
            up = np.stack([C.upsample(p, fh, fv, sw, sh) for p, (fh, fv) in zip(planes, C.factors(eff))], axis=-1)
            assert int(np.abs(up.astype(int) - pillow_draft(data, "YCbCr", d)).max()) <= 1, d


@pytest.mark.gpu
def test_scale_denom_1_is_todays_decode_and_loads_nothing_new(gpu):
    _run_untouched("""
import io
import numpy as np
from PIL import Image
from simd_dct_amd import api, synth
api.init(0)
buf = io.BytesIO()
Image.fromarray(np.stack([synth.plane_u8_np(48, 32, 'photo', seed=k) for k in range(3)], axis=-1), 'YCbCr').save(buf, 'JPEG')
a = D.decode_jpeg(buf.getvalue(), mode='RGB', scale_denom=1)
b = D.decode_jpeg(buf.getvalue(), mode='RGB')
assert tuple(a.shape) == (32, 48, 3) and bool((a == b).all())
""", 300)
