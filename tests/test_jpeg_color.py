"""Chroma upsampling and YCbCr -> RGB on the GPU (libmdct_jpegcolor.so, include/mdct_jpegcolor.h, jpeg_decode.decode_jpeg(mode="RGB"),
jpeg_decode.to_rgb) and the colour space jfif.read_jpeg reports.

CPU: the checker (tests/jpeg_color_checker.py) against libjpeg -- Pillow's upsampled YCbCr and RGB of files whose planes are known
exactly (DC-only blocks, quantiser 8: every IDCT gives dc + 128), over every sampling layout libjpeg takes and tiny and odd sizes --
and its colour conversion on Pillow's own natural files; the colour space rules; the C-ABI's refusals; the code object's kernels.
GPU: decode_jpeg(mode="RGB") equals Pillow on the IDCT-exact files and the checker on natural ones; the C-ABI exact against the
checker at full frame sizes and odd ones, with padded pitches, plane strides, rows beyond 4 GiB and a captured graph; each case
names the instantiation that ran, and together they run every one."""
import io
import os
import struct

import numpy as np
import pytest

import jpeg_color_checker as C
import jpeg_scan_encoder as E
from simd_dct_amd import _jpegcolor_lib, api, jfif

Image = pytest.importorskip("PIL.Image")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLOR_LIB = os.path.join(ROOT, "simd_dct_amd", "libmdct_jpegcolor.so")

# every instantiation of k_ycc_rgb<Kind, Planar>: Kind 0 grey, 1 4:4:4, 2 4:2:2, 3 4:2:0 (luma at full size), 4 any other mix
KINDS = {"grey": 0, "444": 1, "422": 2, "420": 3, "any": 4}
KERNELS = {f"k_ycc_rgb<{k}, {p}>" for k in KINDS.values() for p in ("false", "true")}

LAYOUTS = {  # name -> sampling factors (h, v) of the components
    "444": [(1, 1), (1, 1), (1, 1)],
    "422": [(2, 1), (1, 1), (1, 1)],
    "420": [(2, 2), (1, 1), (1, 1)],
    "440": [(1, 2), (1, 1), (1, 1)],
    "mixed": [(2, 2), (2, 1), (1, 2)],
    "411": [(4, 1), (1, 1), (1, 1)],
    "4x2": [(4, 2), (1, 1), (1, 1)],
    "3x1": [(3, 1), (1, 1), (1, 1)],
    "3x2": [(3, 2), (1, 1), (1, 1)],
    "chroma-above-luma": [(1, 1), (2, 2), (2, 2)],
}
SIZES = [(w, h) for w in (1, 2, 3, 4, 5, 17) for h in (1, 2, 3, 9)] + [(37, 29), (45, 21), (5, 3), (6, 7)]
# the layouts jfif.read_jpeg (and so decode_jpeg) takes: sampling factors 1 and 2
READER_LAYOUTS = ["444", "422", "420", "440", "mixed", "chroma-above-luma"]


def dc_file(W, H, sampling, seed=0):
    """a baseline file of DC-only blocks, every quantiser 8, random DCs: libjpeg's and the engine's IDCT both give exactly dc + 128.
    -> (file, the components at their true sizes)"""
    frame = dict(width=W, height=H, comps=list(sampling))
    rng = np.random.default_rng(seed)
    hmax, vmax = max(h for h, _ in sampling), max(v for _, v in sampling)
    planes, known = [], []
    for (rows, cols), (h, v) in zip(E.plane_shapes(frame), sampling):
        dc = rng.integers(-128, 128, (rows // 8, cols // 8))
        p = np.zeros((rows, cols), dtype=np.int16)
        p[::8, ::8] = dc
        planes.append(p)
        cw, ch = C.true_size(W, H, h, v, hmax, vmax)
        known.append(np.kron(dc + 128, np.ones((8, 8), dtype=np.int64))[:ch, :cw].astype(np.uint8))
    n = len(sampling)
    scans = [dict(comps=[(ci, min(ci, 1), min(ci, 1)) for ci in range(n)])]
    data, _ = E.encode_file(frame, scans, planes, E.ANNEX_K, qtables=[np.full(64, 8, dtype=np.uint16)] * n)
    return data, known


def _segments(data):
    """[(marker, offset, length of the whole segment)] of the marker segments before the first SOS"""
    out, i = [], 2
    while data[i + 1] != 0xDA:
        L = struct.unpack_from(">H", data, i + 2)[0]
        out.append((data[i + 1], i, L + 2))
        i += L + 2
    return out


def edit_markers(data, drop_jfif=False, adobe=None, ids=None):
    """the encoder's file with its APP0 JFIF removed, an APP14 Adobe (transform byte `adobe`) added, and / or the component ids of the
    frame and scan headers replaced (ids: new id of component 1, 2, 3)"""
    b = bytearray(data)
    if ids is not None:
        for m, off, L in _segments(bytes(b)):
            if m == 0xC0:
                nf = b[off + 9]
                for c in range(nf):
                    b[off + 10 + 3 * c] = ids[b[off + 10 + 3 * c] - 1]
        i = bytes(b).index(b"\xff\xda")
        ns = b[i + 4]
        for k in range(ns):
            b[i + 5 + 2 * k] = ids[b[i + 5 + 2 * k] - 1]
    if drop_jfif:
        m, off, L = _segments(bytes(b))[0]
        assert m == 0xE0 and bytes(b[off + 4:off + 9]) == b"JFIF\x00"
        del b[off:off + L]
    if adobe is not None:
        app14 = b"Adobe" + struct.pack(">HHHB", 100, 0, 0, adobe)
        b[2:2] = b"\xff\xee" + struct.pack(">H", len(app14) + 2) + app14
    return bytes(b)


def pillow_ycc(data):
    """libjpeg's upsampled planes before colour conversion, [H, W, 3]"""
    im = Image.open(io.BytesIO(data))
    im.draft("YCbCr", im.size)
    return np.asarray(im)


def pillow_rgb(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def pillow_jpeg(img, **kw):
    buf = io.BytesIO()
    Image.fromarray(img, "L" if img.ndim == 2 else "YCbCr").save(buf, "JPEG", **kw)
    return buf.getvalue()


def picture(W, H, seed, colour=True):
    from simd_dct_amd import synth
    if colour:
        return np.stack([synth.plane_u8_np(W, H, "photo", seed=seed + k) for k in range(3)], axis=-1)
    return synth.plane_u8_np(W, H, "photo", seed=seed)


def expected_kind(sampling, widths, colour="YCbCr"):
    """the instantiation include/mdct_jpegcolor.h's dispatcher should pick (widths: the components' true widths)"""
    if len(sampling) == 1:
        return "grey"
    f = C.factors(sampling)
    if colour != "YCbCr" or f[0] != (1, 1) or f[1] != f[2]:
        return "any"
    if f[1] == (1, 1):
        return "444"
    if f[1] in ((2, 1), (2, 2)) and widths[1] > 2:
        return "422" if f[1] == (2, 1) else "420"
    return "any"


def kernel_name(kind, layout):
    return f"k_ycc_rgb<{KINDS[kind]}, {'true' if layout == 'CHW' else 'false'}>"


# ------------------------------------------------------------------------------------------ CPU: the checker against libjpeg
@pytest.mark.parametrize("name", list(LAYOUTS) + ["grey"])
def test_checker_equals_libjpeg_on_idct_exact_files(name):
    sampling = [(1, 1)] if name == "grey" else LAYOUTS[name]
    for W, H in SIZES:
        data, known = dc_file(W, H, sampling, seed=1000 * W + H)
        if name == "grey":
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert("L")), known[0]), (W, H)
            assert np.array_equal(C.to_rgb(known, sampling, W, H), pillow_rgb(data)), (W, H)
            continue
        ycc = pillow_ycc(data)
        f = C.factors(sampling)
        if f[0] == (1, 1):
            assert np.array_equal(ycc[:, :, 0], known[0]), (name, W, H)  # the file is IDCT-exact
        up = np.stack([C.upsample(k, fh, fv, W, H) for k, (fh, fv) in zip(known, f)], axis=-1)
        assert np.array_equal(up, ycc), (name, W, H, np.argwhere(up != ycc)[:4].tolist())
        assert np.array_equal(C.to_rgb(known, sampling, W, H), pillow_rgb(data)), (name, W, H)


def test_checker_refuses_fractional_ratios():
    with pytest.raises(ValueError):
        C.factors([(2, 1), (3, 1), (1, 1)])


@pytest.mark.parametrize("quality", [5, 75, 100])
@pytest.mark.parametrize("sub", [0, 1, 2])
def test_checker_colour_stage_on_pillows_natural_files(quality, sub):
    data = pillow_jpeg(picture(203, 77, 31 + sub), quality=quality, subsampling=sub)
    ycc = pillow_ycc(data)
    assert np.array_equal(C.ycc_to_rgb(ycc[:, :, 0], ycc[:, :, 1], ycc[:, :, 2]), pillow_rgb(data))


# ------------------------------------------------------------------------------------------ CPU: the colour space
FIELDS = {"width", "height", "sof", "components", "qtables", "huffman", "scans", "colorspace"}


def _same_but_colour(a, b):
    """every field read_jpeg returned before colorspace existed is equal (scans compared without their byte offsets)"""
    assert set(a) == set(b) == FIELDS
    for k in ("width", "height", "sof", "components"):
        assert a[k] == b[k], k
    assert all(np.array_equal(a["qtables"][t], b["qtables"][t]) for t in a["qtables"]) and set(a["qtables"]) == set(b["qtables"])
    assert a["huffman"] == b["huffman"]
    strip = lambda s: {k: v for k, v in s.items() if k not in ("start", "end", "qtables")}  # noqa: E731
    assert [strip(s) for s in a["scans"]] == [strip(s) for s in b["scans"]]


def test_colorspace_of_pillows_jfif_files():
    grey = jfif.read_jpeg(pillow_jpeg(picture(40, 24, 3, colour=False)), require_restart=False)
    colour = jfif.read_jpeg(pillow_jpeg(picture(40, 24, 3)), require_restart=False)
    assert grey["colorspace"] == "grey" and colour["colorspace"] == "YCbCr"
    assert set(grey) == set(colour) == FIELDS
    assert all(set(c) == {"id", "h", "v", "tq"} for c in grey["components"] + colour["components"])


def test_colorspace_of_keep_rgb():
    buf = io.BytesIO()
    Image.fromarray(picture(40, 24, 5), "RGB").save(buf, "JPEG", keep_rgb=True, quality=90)
    info = jfif.read_jpeg(buf.getvalue(), require_restart=False)
    assert info["colorspace"] == "RGB"
    assert [c["id"] for c in info["components"]] == [ord("R"), ord("G"), ord("B")]


def test_colorspace_rules_on_edited_markers():
    base, known = dc_file(24, 16, LAYOUTS["420"], seed=3)
    ref = jfif.read_jpeg(base, require_restart=False)
    assert ref["colorspace"] == "YCbCr"
    rgb_ids = [ord("R"), ord("G"), ord("B")]
    cases = [
        (dict(drop_jfif=True, adobe=1), "YCbCr"),
        (dict(drop_jfif=True, adobe=0), "RGB"),
        (dict(drop_jfif=True, adobe=0, ids=rgb_ids), "RGB"),
        (dict(drop_jfif=True, adobe=2), "YCbCr"),
        (dict(drop_jfif=True), "YCbCr"),  # ids 1, 2, 3
        (dict(drop_jfif=True, ids=rgb_ids), "RGB"),
        (dict(ids=rgb_ids), "YCbCr"),  # JFIF decides before the ids
        (dict(adobe=0), "YCbCr"),  # and before Adobe
        (dict(drop_jfif=True, ids=[7, 8, 9]), "YCbCr"),
    ]
    for kw, want in cases:
        data = edit_markers(base, **kw)
        info = jfif.read_jpeg(data, require_restart=False)
        assert info["colorspace"] == want, kw
        if "ids" in kw:
            assert [c["id"] for c in info["components"]] == kw["ids"]
            info = dict(info, components=[dict(c, id=i + 1) for i, c in enumerate(info["components"])])
        _same_but_colour(info, ref)
        # libjpeg agrees: its RGB of an RGB file is the upsampled planes themselves, of a YCbCr file their conversion
        assert np.array_equal(pillow_rgb(data), C.to_rgb(known, LAYOUTS["420"], 24, 16, want)), kw


# ------------------------------------------------------------------------------------------ CPU: the C-ABI refuses without a device
def _plane(px, pitch, w, h, hs=1, vs=1):
    return _jpegcolor_lib.Plane(px, pitch, w, h, hs, vs)


def _call(planes, n, W, H, colour=0, layout=0, out=1 << 44, pitch=None, stride=0):
    lib = _jpegcolor_lib.load()
    arr = None
    if planes is not None:
        arr = (_jpegcolor_lib.Plane * max(1, len(planes)))(*planes)
    pitch = 3 * W if pitch is None else pitch
    return lib.mdct_jpegcolor_to_rgb(arr, n, W, H, colour, layout, out, pitch, stride, None), lib.mdct_jpegcolor_last_error().decode()


def test_cabi_refusals_without_device():
    A = 1 << 40  # addresses far apart; nothing is dereferenced
    ok420 = [_plane(A, 64, 64, 32, 2, 2), _plane(A + (1 << 30), 32, 32, 16), _plane(A + (2 << 30), 32, 32, 16)]
    cases = {
        "null planes": (None, 3, 64, 32),
        "null out": (ok420, 3, 64, 32, 0, 0, 0),
        "two planes": (ok420, 2, 64, 32),
        "four planes": (ok420 + ok420[:1], 4, 64, 32),
        "grey with three planes": (ok420, 3, 64, 32, 2),
        "YCbCr with one plane": (ok420[:1], 1, 64, 32, 0),
        "colour 3": (ok420, 3, 64, 32, 3),
        "layout 2": (ok420, 3, 64, 32, 0, 2),
        "null plane": ([ok420[0], _plane(0, 32, 32, 16), ok420[2]], 3, 64, 32),
        "fractional ratio": ([_plane(A, 64, 64, 32, 3, 2), _plane(A + (1 << 30), 32, 43, 16, 2, 1), ok420[2]], 3, 64, 32),
        "factor 5": ([_plane(A, 80, 80, 32, 5, 1), ok420[1], ok420[2]], 3, 80, 32),
        "factor 0": ([_plane(A, 64, 64, 32, 0, 1), ok420[1], ok420[2]], 3, 64, 32),
        "chroma width": ([ok420[0], _plane(A + (1 << 30), 32, 31, 16), ok420[2]], 3, 64, 32),
        "chroma height": ([ok420[0], ok420[1], _plane(A + (2 << 30), 32, 32, 17)], 3, 64, 32),
        "padded luma given": ([_plane(A, 64, 64, 32, 2, 2), _plane(A + (1 << 30), 32, 32, 16), _plane(A + (2 << 30), 32, 32, 16)], 3, 63, 32),
        "plane pitch": ([_plane(A, 63, 64, 32, 2, 2), ok420[1], ok420[2]], 3, 64, 32),
        "out pitch": (ok420, 3, 64, 32, 0, 0, 1 << 44, 191),
        "CHW pitch": (ok420, 3, 64, 32, 0, 1, 1 << 44, 63, 64 * 32),
        "CHW stride": (ok420, 3, 64, 32, 0, 1, 1 << 44, 64, 64 * 32 - 1),
        "width 0": ([_plane(A, 64, 0, 32)], 1, 0, 32, 2),
        "height 0": ([_plane(A, 64, 64, 0)], 1, 64, 0, 2),
        "width 65536": ([_plane(A, 65536, 65536, 1)], 1, 65536, 1, 2),
        "output over a plane": (ok420, 3, 64, 32, 0, 0, A + (1 << 30) - 100),
        "output ends in a plane": (ok420, 3, 64, 32, 0, 1, A - 2 * 4096 - 64 * 31 - 1, 64, 4096),
        "plane over the output": ([_plane(A, 64, 64, 32, 2, 2), _plane((1 << 44) + 5000, 32, 32, 16), ok420[2]], 3, 64, 32),
    }
    for name, args in cases.items():
        rc, msg = _call(*args)
        assert rc == 1, (name, rc, msg)  # MDCT_INVALID_PARAMETER
        assert msg, name


def test_code_object_holds_the_planned_instantiations():
    from test_kernel_coverage import code_object_kernels
    names, n_objects = code_object_kernels(lib=COLOR_LIB)
    assert n_objects == 1 and names == KERNELS, sorted(names ^ KERNELS)


def test_decode_jpeg_refuses_unknown_modes_before_the_device():
    from simd_dct_amd import jpeg_decode as D
    data, _ = dc_file(16, 16, LAYOUTS["420"])
    with pytest.raises(ValueError):
        D.decode_jpeg(data, mode="YCbCr")
    with pytest.raises(ValueError):
        D.decode_jpeg(data, mode="RGB", layout="HCW")
    with pytest.raises(jfif.JpegFormatError):
        D._colour_params(dict(jfif.read_jpeg(data, require_restart=False), colorspace=None))
    info = jfif.read_jpeg(data, require_restart=False)
    info["components"] = [dict(c, h=h) for c, h in zip(info["components"], (4, 3, 1))]  # 4 / 3 is fractional
    with pytest.raises(jfif.JpegFormatError):
        D._colour_params(info)


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
    ran = {k: v for k, v in api.kernel_counts().items() if k.startswith("k_ycc_rgb")}
    assert set(ran) == {want}, (want, ran)
    return want


def _hwc(img, layout):
    return img if layout == "HWC" else np.transpose(img, (1, 2, 0))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["HWC", "CHW"])
def test_decode_rgb_equals_libjpeg_on_idct_exact_files(gpu, layout):
    from simd_dct_amd import jpeg_decode as D
    cases = [(name, LAYOUTS[name], {}) for name in READER_LAYOUTS] + [("grey", [(1, 1)], {})]
    cases += [("rgb-adobe0", LAYOUTS["444"], dict(drop_jfif=True, adobe=0, ids=[ord("R"), ord("G"), ord("B")])),
              ("rgb-ids-420", LAYOUTS["420"], dict(drop_jfif=True, ids=[ord("R"), ord("G"), ord("B")]))]
    seen = set()
    for name, sampling, edit in cases:
        for W, H in SIZES + [(130, 66), (1031, 17)]:
            data, _ = dc_file(W, H, sampling, seed=7 * W + H)
            if edit:
                data = edit_markers(data, **edit)
            api.kernel_counts_reset()
            got = D.decode_jpeg(data, mode="RGB", layout=layout)
            info = jfif.read_jpeg(data, require_restart=False)
            geo, _ = D.geometry(info)
            seen.add(ran_exactly(gpu, kernel_name(expected_kind(sampling, [g[0] for g in geo], info["colorspace"]), layout)))
            want = pillow_rgb(data)
            g = _hwc(got.cpu().numpy(), layout)
            assert got.shape == ((H, W, 3) if layout == "HWC" else (3, H, W)), (name, W, H)
            assert np.array_equal(g, want), (name, W, H, layout, np.argwhere(g != want)[:4].tolist())
    assert {kernel_name(k, layout) for k in KINDS} <= seen


NATURAL = [  # (size, colour, save options)
    ((61, 37), True, dict(quality=75, subsampling=2, restart_marker_rows=1)),
    ((100, 52), True, dict(quality=75, subsampling=0)),
    ((100, 52), True, dict(quality=75, subsampling=1, restart_marker_blocks=5)),
    ((333, 101), True, dict(quality=90, subsampling=2)),
    ((37, 29), True, dict(quality=5, subsampling=1)),
    ((203, 77), True, dict(quality=100, subsampling=0, restart_marker_rows=1)),
    ((1001, 3), True, dict(quality=75, subsampling=2)),
    ((61, 37), False, dict(quality=75)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("size,colour,kw", NATURAL, ids=[f"{s[0]}x{s[1]}-{'c' if c else 'g'}-{k}" for s, c, k in NATURAL])
def test_decode_rgb_on_natural_files(gpu, size, colour, kw):
    from simd_dct_amd import jpeg_decode as D
    W, H = size
    data = pillow_jpeg(picture(W, H, 41 + W, colour), **kw)
    info = jfif.read_jpeg(data, require_restart=False)
    sampling = [(c["h"], c["v"]) for c in info["components"]]
    for layout in ("HWC", "CHW"):
        got, coefs = D.decode_jpeg(data, mode="RGB", layout=layout, coefficients=True)
        planes = [p.cpu().numpy() for p in D.decode_jpeg(data)]
        g = _hwc(got.cpu().numpy(), layout)
        assert np.array_equal(g, C.to_rgb(planes, sampling, W, H)), layout
        assert len(coefs) == len(planes)
    want = pillow_rgb(data)
    assert int(np.abs(g.astype(int) - want).max()) <= 3
    if colour:
        up = np.stack([C.upsample(p, fh, fv, W, H) for p, (fh, fv) in zip(planes, C.factors(sampling))], axis=-1)
        assert int(np.abs(up.astype(int) - pillow_ycc(data)).max()) <= 1


@pytest.mark.gpu
@pytest.mark.parametrize("sub", [0, 2])
def test_colour_stage_on_pillows_own_planes(gpu, sub):
    """libjpeg's upsampled planes converted on the GPU as full-size 4:4:4 give libjpeg's RGB exactly"""
    torch = gpu
    from simd_dct_amd import jpeg_decode as D
    W, H = 517, 203
    data = pillow_jpeg(picture(W, H, 51), quality=80, subsampling=sub)
    ycc = pillow_ycc(data)
    planes = [torch.from_numpy(np.ascontiguousarray(ycc[:, :, k])).cuda() for k in range(3)]
    api.kernel_counts_reset()
    got = D.to_rgb(planes, [(1, 1)] * 3, W, H)
    ran_exactly(torch, kernel_name("444", "HWC"))
    assert np.array_equal(got.cpu().numpy(), pillow_rgb(data))


def _random_planes(torch, W, H, sampling, seed, pad=0, offset=0, align=1):
    """random components at their true sizes, each in a buffer of pitch (true width rounded up to align) + pad, starting offset bytes
    in -> (device views, host arrays)"""
    rng = np.random.default_rng(seed)
    hmax, vmax = max(h for h, _ in sampling), max(v for _, v in sampling)
    dev, host = [], []
    for h, v in sampling:
        cw, ch = C.true_size(W, H, h, v, hmax, vmax)
        a = rng.integers(0, 256, (ch, cw), dtype=np.uint8)
        pitch = -(-cw // align) * align + pad
        buf = torch.empty(offset + ch * pitch, dtype=torch.uint8, device="cuda")
        view = torch.as_strided(buf, (ch, cw), (pitch, 1), offset)
        view.copy_(torch.from_numpy(a).cuda())
        dev.append(view)
        host.append(a)
    return dev, host


def _checked_run(torch, W, H, sampling, colour, layout, seed, pad=0, offset=0, out_pad=0, out_offset=0, align=1):
    """one to_rgb call into a canary-filled buffer with out_pad bytes after every row (CHW: also after every plane) and a guard after
    the buffer; -> the instantiation that ran.  Exact against the checker; nothing outside the image's bytes written."""
    from simd_dct_amd import jpeg_decode as D
    dev, host = _random_planes(torch, W, H, sampling, seed, pad, offset, align)
    row = 3 * W if layout == "HWC" else W
    pitch = row + out_pad
    guard = 4096
    if layout == "HWC":
        size, shape, strides = out_offset + H * pitch, (H, W, 3), (pitch, 3, 1)
    else:
        plane = H * pitch + out_pad
        size, shape, strides = out_offset + 3 * plane, (3, H, W), (plane, pitch, 1)
    buf = torch.full((size + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.as_strided(buf, shape, strides, out_offset)
    api.kernel_counts_reset()
    D.to_rgb(dev, sampling, W, H, colour=colour, layout=layout, out=out)
    kind = expected_kind(sampling, [h.shape[1] for h in host], colour)
    ran_exactly(torch, kernel_name(kind, layout))
    want = C.to_rgb(host, sampling, W, H, colour)
    g = _hwc(out.cpu().numpy(), layout)
    assert np.array_equal(g, want), (W, H, sampling, layout, np.argwhere(g != want)[:4].tolist())
    inside = int((out != 0xA5).sum())
    assert int((buf != 0xA5).sum()) == inside, "bytes written outside the image"
    return kind


ODD = [  # (W, H, sampling, colour)
    (1, 1, [(1, 1)], "grey"), (37, 29, [(1, 1)], "grey"), (1031, 5, [(2, 2)], "grey"),
    (37, 29, LAYOUTS["444"], "YCbCr"), (1030, 5, LAYOUTS["444"], "YCbCr"),
    (37, 29, [(2, 1), (1, 1), (1, 1)], "YCbCr"), (1031, 7, [(2, 1), (1, 1), (1, 1)], "YCbCr"),
    (37, 29, LAYOUTS["420"], "YCbCr"), (1031, 7, LAYOUTS["420"], "YCbCr"), (6, 1, LAYOUTS["420"], "YCbCr"),
    (3, 5, LAYOUTS["420"], "YCbCr"), (4, 9, LAYOUTS["422"], "YCbCr"),  # chroma 2 wide: replication, kAny
    (37, 29, LAYOUTS["440"], "YCbCr"), (45, 21, LAYOUTS["mixed"], "YCbCr"), (45, 21, LAYOUTS["411"], "YCbCr"),
    (45, 21, LAYOUTS["3x2"], "YCbCr"), (45, 21, LAYOUTS["chroma-above-luma"], "YCbCr"), (37, 29, LAYOUTS["420"], "RGB"),
    (1031, 9, [(2, 2), (1, 1), (2, 1)], "YCbCr"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["HWC", "CHW"])
def test_cabi_odd_sizes_every_instantiation(gpu, layout):
    seen = set()
    for i, (W, H, sampling, colour) in enumerate(ODD):
        seen.add(_checked_run(gpu, W, H, sampling, colour, layout, seed=100 + i))
        # unaligned input and output row starts: the one-pixel path, same instantiation, same bytes
        seen.add(_checked_run(gpu, W, H, sampling, colour, layout, seed=200 + i, pad=3, offset=5, out_pad=7, out_offset=1))
        # aligned but padded
        seen.add(_checked_run(gpu, W, H, sampling, colour, layout, seed=300 + i, pad=64, align=64,
                              out_pad=16 - (3 * W if layout == "HWC" else W) % 16 + 32))
    assert seen == set(KINDS)


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,layout", [(8192, 8192, "HWC"), (8192, 8192, "CHW"), (7680, 4320, "HWC"), (7680, 4320, "CHW")])
def test_cabi_full_frames_420(gpu, W, H, layout):
    assert _checked_run(gpu, W, H, LAYOUTS["420"], "YCbCr", layout, seed=W + H) == "420"


@pytest.mark.gpu
@pytest.mark.parametrize("sampling,kind", [([(1, 1)], "grey"), (LAYOUTS["444"], "444"), (LAYOUTS["422"], "422")])
def test_cabi_full_frame_other_kinds(gpu, sampling, kind):
    assert _checked_run(gpu, 7680, 4320, sampling, "grey" if kind == "grey" else "YCbCr", "HWC", seed=9, out_pad=64) == kind


@pytest.mark.gpu
def test_cabi_output_row_beyond_4gib(gpu):
    """three rows 2 GiB + 4 KiB apart: the last one starts past 2^32 bytes"""
    torch = gpu
    from simd_dct_amd import jpeg_decode as D
    W, H = 1000, 3
    pitch = (1 << 31) + 4096
    dev, host = _random_planes(torch, W, H, LAYOUTS["420"], seed=77)
    buf = torch.full(((H - 1) * pitch + 3 * W + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.as_strided(buf, (H, W, 3), (pitch, 3, 1))
    api.kernel_counts_reset()
    D.to_rgb(dev, LAYOUTS["420"], W, H, out=out)
    ran_exactly(torch, kernel_name("420", "HWC"))
    want = C.to_rgb(host, LAYOUTS["420"], W, H)
    for y in range(H):
        assert np.array_equal(out[y].cpu().numpy(), want[y]), y
    assert int((buf != 0xA5).sum()) == int((out != 0xA5).sum())
    del buf, out
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_cabi_captured_and_replayed_on_new_inputs(gpu):
    torch = gpu
    from simd_dct_amd import jpeg_decode as D
    W, H = 1920, 1080
    dev, _ = _random_planes(torch, W, H, LAYOUTS["420"], seed=1)
    out = torch.empty((3, H, W), dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        D.to_rgb(dev, LAYOUTS["420"], W, H, layout="CHW", out=out, stream=s)
    for seed in (2, 3):
        new, host = _random_planes(torch, W, H, LAYOUTS["420"], seed=seed)
        for d, n in zip(dev, new):
            d.copy_(n)
        out.fill_(0)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_hwc(out.cpu().numpy(), "CHW"), C.to_rgb(host, LAYOUTS["420"], W, H)), seed


@pytest.mark.gpu
def test_engine_three_scan_420_file(gpu):
    """the engine's own file (jfif.write_jpeg: JFIF, one non-interleaved scan per component, Y 2x2) decodes to the checker's RGB of its
    planes and to libjpeg's within the IDCT bounds"""
    from simd_dct_amd import jpeg_decode as D
    from simd_dct_amd import synth
    from test_jpeg_decode import engine_file_cpu
    W, H = 256, 64
    y = synth.plane_u8_np(W, H, "photo", seed=61)
    cb, cr = (synth.plane_u8_np(W // 2, H // 2, "photo", seed=s) for s in (62, 63))
    data, _ = engine_file_cpu([(y, synth.JPEG_LUMA, False), (cb, synth.JPEG_CHROMA, True), (cr, synth.JPEG_CHROMA, True)])
    info = jfif.read_jpeg(data, require_restart=False)
    assert len(info["scans"]) == 3 and info["colorspace"] == "YCbCr"
    api.kernel_counts_reset()
    got = D.decode_jpeg(data, mode="RGB").cpu().numpy()
    ran_exactly(gpu, kernel_name("420", "HWC"))
    planes = [p.cpu().numpy() for p in D.decode_jpeg(data)]
    assert np.array_equal(got, C.to_rgb(planes, LAYOUTS["420"], W, H))
    assert int(np.abs(got.astype(int) - pillow_rgb(data)).max()) <= 3
