"""Baseline JPEG encoding on the GPU: the front stage (libmdct_jpegenc.so, include/mdct_jpegenc.h, jpeg_encode.to_planes) and
jpeg_encode.encode_jpeg / quality_tables, with jfif.write_jpeg's sampling argument.

CPU: the checker (tests/jpeg_encode_checker.py) against libjpeg -- Pillow's files at quality 100 of content whose chroma blocks are
constant under libjpeg's rules only, read back with tests/jpeg_decode_checker.py; quality_tables against Pillow's DQT; write_jpeg
with per-component sampling and odd true sizes; the refusals; the code object's kernels.
GPU: the C-ABI byte for byte against the checker in every instantiation, with odd and full-frame sizes, padded and unaligned pitches,
canaries and a captured graph; encode_jpeg's scans against tests/jpeg_scan_encoder.py on the oracle's coefficients; the round trip
through decode_jpeg; Pillow against its own encode of the same images."""
import io
import os

import numpy as np
import pytest

import jpeg_decode_checker as DC
import jpeg_encode_checker as C
import jpeg_scan_encoder as E
from simd_dct_amd import _jpegenc_lib, api, jfif

Image = pytest.importorskip("PIL.Image")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENC_LIB = os.path.join(ROOT, "simd_dct_amd", "libmdct_jpegenc.so")

# k_rgb_ycc<Kind, Planar>: Kind 0 grey (one instantiation, the layout plays no part), 1 4:4:4, 2 4:2:2, 3 4:2:0
KIND = {"grey": 0, "4:4:4": 1, "4:2:2": 2, "4:2:0": 3}
KERNELS = {"k_rgb_ycc<0, false>"} | {f"k_rgb_ycc<{k}, {p}>" for k in (1, 2, 3) for p in ("false", "true")}
PIL_SUB = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}
SPECS = {0: E.ANNEX_K[(0, 0)], 1: E.ANNEX_K[(1, 0)], 2: E.ANNEX_K[(0, 1)], 3: E.ANNEX_K[(1, 1)]}


def kernel_name(kind, layout):
    return f"k_rgb_ycc<{KIND[kind]}, {'true' if layout == 'CHW' and kind != 'grey' else 'false'}>"


def pillow_q100(rgb, sub):
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, "JPEG", quality=100, subsampling=PIL_SUB[sub], restart_marker_rows=1)
    return b.getvalue()


def assert_dc_only(coef, want, rows, cols):
    """every block of coef inside the component's block grid (rows x cols blocks) has DC 8 * (v - 128) and no AC; want [rows*8, cols*8]"""
    c = coef[:rows * 8, :cols * 8].astype(np.int64).reshape(rows, 8, cols, 8).transpose(0, 2, 1, 3).reshape(rows, cols, 64)
    assert np.array_equal(c[:, :, 0], 8 * (want[::8, ::8].astype(np.int64) - 128)), np.argwhere(c[:, :, 0] != 8 * (want[::8, ::8].astype(np.int64) - 128))[:4]
    assert not c[:, :, 1:].any(), "non-zero AC coefficients"


# ------------------------------------------------------------------------------------------ the checker against libjpeg
def test_checker_444_constant_blocks_equal_libjpeg():
    rng = np.random.default_rng(1)
    nb = 32
    colours = rng.integers(0, 256, (nb * nb, 3), dtype=np.uint8)
    colours[:8] = [[255 * ((i >> k) & 1) for k in range(3)] for i in range(8)]  # the corners of the cube
    img = np.kron(colours.reshape(nb, nb, 3), np.ones((8, 8, 1), dtype=np.uint8))
    planes = C.planes(img, "4:4:4")
    coef, st, _ = DC.decode(pillow_q100(img, "4:4:4"))
    assert all(s == DC.OK for sc in st for s in sc)
    for k in range(3):
        assert_dc_only(coef[k], planes[k], nb, nb)
        assert np.array_equal(planes[k][::8, ::8].reshape(-1), np.array(C.rgb_to_ycc(colours)[k]))


_LOOKUP = None


def chroma_lookup():
    """(cb, cr) -> some 24-bit RGB colour with exactly that chroma, or -1"""
    global _LOOKUP
    if _LOOKUP is None:
        c = np.arange(1 << 24, dtype=np.int32)
        rgb = np.stack([(c >> 16) & 255, (c >> 8) & 255, c & 255], axis=-1).astype(np.uint8)
        _, cb, cr = C.rgb_to_ycc(rgb)
        _LOOKUP = np.full(1 << 16, -1, dtype=np.int64)
        _LOOKUP[cb * 256 + cr] = c
    return _LOOKUP


def _rgb_of(code):
    return np.stack([(code >> 16) & 255, (code >> 8) & 255, code & 255], axis=-1).astype(np.uint8)


def bias_image(sub, cols, rows, seed):
    """an image whose chroma blocks (cols x rows blocks) are constant under libjpeg's bias order and no other: each group's Cb and Cr
    sums are 4c + 2 / 4c - 2 (4:2:0) or 2c + 1 / 2c - 1 (4:2:2) in even / odd output columns.  -> (image, chroma targets [2, rows*8, cols*8])"""
    lut = chroma_lookup()
    rng = np.random.default_rng(seed)
    n = 4 if sub == "4:2:0" else 2
    cw, ch = cols * 8, rows * 8
    target = np.kron(rng.integers(70, 187, (2, rows, cols)), np.ones((1, 8, 8), dtype=np.int64))  # Cb, Cr per block
    odd = np.arange(cw) & 1
    need = n * target + np.where(odd, -(n // 2), n // 2)  # the group sums
    groups = np.zeros((ch, cw, n), dtype=np.int64)
    todo = np.ones((ch, cw), dtype=bool)
    while todo.any():
        idx = np.argwhere(todo)
        t = target[:, idx[:, 0], idx[:, 1]]
        m = len(idx)
        got = np.zeros((m, n), dtype=np.int64)
        ok = np.ones(m, dtype=bool)
        s = np.zeros((2, m), dtype=np.int64)
        for j in range(n - 1):
            cc = t + rng.integers(-20, 21, (2, m))
            code = lut[np.clip(cc[0], 0, 255) * 256 + np.clip(cc[1], 0, 255)]
            ok &= code >= 0
            got[:, j] = code
            s += cc
        last = need[:, idx[:, 0], idx[:, 1]] - s
        inr = (last >= 0).all(axis=0) & (last <= 255).all(axis=0)
        code = np.where(inr, lut[np.clip(last[0], 0, 255) * 256 + np.clip(last[1], 0, 255)], -1)
        ok &= code >= 0
        got[:, n - 1] = code
        groups[idx[ok, 0], idx[ok, 1]] = got[ok]
        todo[idx[ok, 0], idx[ok, 1]] = False
    px = _rgb_of(groups)  # [ch, cw, n, 3]
    if sub == "4:2:0":
        img = px.reshape(ch, cw, 2, 2, 3).transpose(0, 2, 1, 3, 4).reshape(2 * ch, 2 * cw, 3)
    else:
        img = px.reshape(ch, 2 * cw, 3)
    return np.ascontiguousarray(img), target


@pytest.mark.parametrize("sub", ["4:2:2", "4:2:0"])
def test_checker_bias_order_equals_libjpeg(sub):
    img, target = bias_image(sub, 16, 8, seed=7 if sub == "4:2:0" else 8)
    planes = C.planes(img, sub)
    for k in (1, 2):
        assert np.array_equal(planes[k], target[k - 1])
    # any other bias order moves some samples: a constant bias, the swapped order
    _, cb, _ = C.rgb_to_ycc(img)
    n = 4 if sub == "4:2:0" else 2
    s = cb.reshape(cb.shape[0] // (n // 2), n // 2, -1, 2).sum(axis=(1, 3))
    for bias in ([n // 2 - 1] * 2, [n // 2] * 2, [n // 2, n // 2 - 1]):
        assert not np.array_equal((s + np.where(np.arange(s.shape[1]) & 1, bias[1], bias[0])) >> (n // 2), target[0])
    coef, st, _ = DC.decode(pillow_q100(img, sub))
    assert all(x == DC.OK for sc in st for x in sc)
    for k in (1, 2):
        assert_dc_only(coef[k], target[k - 1], 8, 16)


@pytest.mark.parametrize("sub", ["4:4:4", "4:2:2", "4:2:0"])
@pytest.mark.parametrize("W,H", [(1, 1), (17, 9), (33, 31)])
def test_checker_odd_sizes_equal_libjpeg(sub, W, H):
    """one colour per 16 x 16 region, cropped to an odd size: the checker's true-size edge samples against libjpeg's"""
    rng = np.random.default_rng(W * 100 + H)
    colours = rng.integers(0, 256, (-(-H // 16), -(-W // 16), 3), dtype=np.uint8)
    img = np.ascontiguousarray(np.kron(colours, np.ones((16, 16, 1), dtype=np.uint8))[:H, :W])
    planes = C.planes(img, sub)
    coef, st, _ = DC.decode(pillow_q100(img, sub))
    assert all(x == DC.OK for sc in st for x in sc)
    for k, (cw, ch) in enumerate(C.true_sizes(W, H, C.SAMPLING[sub])):
        assert_dc_only(coef[k], planes[k], -(-ch // 8), -(-cw // 8))


def test_quality_tables_equal_pillows():
    from simd_dct_amd import jpeg_encode as J
    img = np.zeros((8, 8, 3), dtype=np.uint8)
    for q in range(1, 101):
        b = io.BytesIO()
        Image.fromarray(img).save(b, "JPEG", quality=q)
        qt = jfif.read_jpeg(b.getvalue(), require_restart=False)["qtables"]
        luma, chroma = J.quality_tables(q)
        assert qt[0].tolist() == luma and qt[1].tolist() == chroma, q


# ------------------------------------------------------------------------------------------ write_jpeg with sampling factors
@pytest.mark.parametrize("sub", ["4:4:4", "4:2:2", "4:2:0", "grey"])
@pytest.mark.parametrize("W,H", [(37, 29), (9, 17), (1, 1)])
def test_write_jpeg_sampling_and_true_size(sub, W, H):
    """non-interleaved DC-only scans (quantiser 8: every IDCT gives exactly dc + 128) over each component's own block grid, written by
    write_jpeg: jfif.read_jpeg parses them, Pillow opens them and its pixels are the checker's"""
    import jpeg_color_checker as CC
    sampling = [(1, 1)] if sub == "grey" else C.SAMPLING[sub]
    rng = np.random.default_rng(W + 7 * H)
    comps, known = [], []
    for k, (cw, ch) in enumerate(C.true_sizes(W, H, sampling)):
        bx, by = -(-cw // 8), -(-ch // 8)
        dc = rng.integers(-128, 128, (by, bx))
        p = np.zeros((by * 8, bx * 8), dtype=np.int16)
        p[::8, ::8] = dc
        frame = dict(width=bx * 8, height=by * 8, comps=[(1, 1)])
        t = min(k, 1)
        data, _ = E.encode_scan(frame, dict(comps=[(0, t, t)], dri=bx), [p], E.ANNEX_K)
        comps.append(dict(scan=data, blocks_per_row=bx, qtable=[8] * 64))
        known.append(np.kron(dc + 128, np.ones((8, 8), dtype=np.int64))[:ch, :cw].astype(np.uint8))
    f = jfif.write_jpeg(comps, W, H, specs=SPECS, sampling=sampling)
    info = jfif.read_jpeg(f)
    assert (info["width"], info["height"]) == (W, H)
    assert [(c["h"], c["v"]) for c in info["components"]] == sampling
    assert [s["restart_interval"] for s in info["scans"]] == [c["blocks_per_row"] for c in comps]
    im = Image.open(io.BytesIO(f))
    im.load()
    if sub == "grey":
        assert np.array_equal(np.asarray(im), known[0])
    else:
        assert np.array_equal(np.asarray(im.convert("RGB")), CC.to_rgb(known, sampling, W, H))


def test_write_jpeg_default_is_unchanged():
    comps = [dict(scan=b"\x00", blocks_per_row=2, qtable=[1] * 64), dict(scan=b"\x01", blocks_per_row=1, qtable=[2] * 64),
             dict(scan=b"\x02", blocks_per_row=1, qtable=[2] * 64)]
    assert jfif.write_jpeg(comps, 16, 16, specs=SPECS) == jfif.write_jpeg(comps, 16, 16, specs=SPECS, sampling=[(2, 2), (1, 1), (1, 1)])
    assert jfif.write_jpeg(comps[:1], 16, 8, specs=SPECS) == jfif.write_jpeg(comps[:1], 16, 8, specs=SPECS, sampling=[(1, 1)])


# ------------------------------------------------------------------------------------------ refusals, code object
def _plane(px, pitch, w, h, hh=1, vv=1):
    return _jpegenc_lib.Plane(px, pitch, w, h, hh, vv)


def _call(in_, planes, n, W, H, colour=0, layout=0, pitch=None, stride=0):
    lib = _jpegenc_lib.load()
    arr = None
    if planes is not None:
        arr = (_jpegenc_lib.Plane * max(1, len(planes)))(*planes)
    pitch = (3 * W if layout == 0 and colour == 0 else W) if pitch is None else pitch
    return lib.mdct_jpegenc_from_rgb(in_, pitch, stride, W, H, colour, layout, arr, n, None), lib.mdct_jpegenc_last_error().decode()


def test_cabi_refusals_without_device():
    A, I = 1 << 40, 1 << 44  # addresses far apart; nothing is dereferenced
    ok = [_plane(A, 64, 64, 32, 2, 2), _plane(A + (1 << 30), 32, 32, 16), _plane(A + (2 << 30), 32, 32, 16)]
    cases = {
        "null input": (None, ok, 3, 64, 32),
        "null planes": (I, None, 3, 64, 32),
        "null plane": (I, [ok[0], _plane(0, 32, 32, 16), ok[2]], 3, 64, 32),
        "two planes": (I, ok, 2, 64, 32),
        "grey with three planes": (I, ok, 3, 64, 32, 1),
        "RGB with one plane": (I, ok[:1], 1, 64, 32, 0),
        "colour 2": (I, ok, 3, 64, 32, 2),
        "layout 2": (I, ok, 3, 64, 32, 0, 2),
        "width 0": (I, ok, 3, 0, 32),
        "height 65536": (I, ok, 3, 64, 65536),
        "grey 2x2": (I, [_plane(A, 64, 64, 32, 2, 2)], 1, 64, 32, 1),
        "4:1:1": (I, [_plane(A, 64, 64, 32, 4, 1)] + ok[1:], 3, 64, 32),
        "4:4:0": (I, [_plane(A, 64, 64, 32, 1, 2), _plane(A + (1 << 30), 64, 64, 16), _plane(A + (2 << 30), 64, 64, 16)], 3, 64, 32),
        "chroma 2x1": (I, [_plane(A, 64, 64, 32, 2, 2), _plane(A + (1 << 30), 64, 32, 16, 2, 1), ok[2]], 3, 64, 32),
        "luma too narrow": (I, [_plane(A, 64, 56, 32, 2, 2)] + ok[1:], 3, 64, 32),
        "luma width not a multiple of 8": (I, [_plane(A, 68, 68, 32, 2, 2)] + ok[1:], 3, 64, 32),
        "chroma too short": (I, [ok[0], ok[1], _plane(A + (2 << 30), 32, 32, 8)], 3, 64, 32),
        "padded beyond 65536": (I, [_plane(A, 65544, 65544, 32, 2, 2)] + ok[1:], 3, 64, 32),
        "plane pitch": (I, [_plane(A, 63, 64, 32, 2, 2)] + ok[1:], 3, 64, 32),
        "input pitch": (I, ok, 3, 64, 32, 0, 0, 191),
        "CHW pitch": (I, ok, 3, 64, 32, 0, 1, 63, 64 * 32),
        "CHW stride": (I, ok, 3, 64, 32, 0, 1, 64, 64 * 31),
        "plane over the input": (A + (1 << 30) - 100, ok, 3, 64, 32),
        "CHW input ends in a plane": (A - 2 * 4096 - 64 * 31 - 1, ok, 3, 64, 32, 0, 1, 64, 4096),
        "planes overlap": (I, [ok[0], ok[1], _plane(A + (1 << 30) + 100, 32, 32, 16)], 3, 64, 32),
        "chroma over luma": (I, [ok[0], _plane(A + 64 * 31, 32, 32, 16), ok[2]], 3, 64, 32),
    }
    for name, args in cases.items():
        rc, msg = _call(*args)
        assert rc == 1, (name, rc, msg)  # MDCT_INVALID_PARAMETER
        assert msg, name


def test_encode_jpeg_refuses_bad_arguments_before_the_device(monkeypatch):
    from simd_dct_amd import jpeg_encode as J

    def no_device(*a, **k):
        raise AssertionError("device work before the arguments were checked")

    monkeypatch.setattr(J, "to_planes", no_device)
    monkeypatch.setattr(J, "_run_scan", no_device)
    img = np.zeros((16, 16, 3), dtype=np.uint8)
    for kw in (dict(quality=0), dict(quality=101), dict(quality=7.5), dict(quality=True), dict(quality="75"), dict(subsampling="4:1:1"),
               dict(subsampling=None), dict(layout="HCW"), dict(layout="CHW")):
        with pytest.raises(ValueError):
            J.encode_jpeg(img, **kw)
    for bad in (img.astype(np.int16), np.zeros((16, 16, 4), np.uint8), np.zeros((2, 16, 16, 3), np.uint8), np.zeros((16,), np.uint8),
                np.zeros((0, 16), np.uint8), np.zeros((16, 65536), np.uint8), [[1, 2], [3, 4]]):
        with pytest.raises(ValueError):
            J.encode_jpeg(bad)
    for q in (0, 101, 2.0):
        with pytest.raises(ValueError):
            J.quality_tables(q)


def test_code_object_holds_the_planned_instantiations():
    from test_kernel_coverage import code_object_kernels
    names, n_objects = code_object_kernels(lib=ENC_LIB)
    assert n_objects == 1 and names == KERNELS, sorted(names ^ KERNELS)


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
    ran = {k: v for k, v in api.kernel_counts().items() if k.startswith("k_rgb_ycc")}
    assert set(ran) == {want}, (want, ran)


def _image(torch, W, H, kind, layout, seed, pad=0, offset=0):
    """a random image in a device buffer: rows pad bytes longer than needed (CHW: also pad bytes between planes), offset bytes in"""
    rng = np.random.default_rng(seed)
    if kind == "grey":
        host = rng.integers(0, 256, (H, W), dtype=np.uint8)
        pitch = W + pad
        shape, strides, size = (H, W), (pitch, 1), H * pitch
    elif layout == "HWC":
        host = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        pitch = 3 * W + pad
        shape, strides, size = (H, W, 3), (pitch, 3, 1), H * pitch
    else:
        host = rng.integers(0, 256, (3, H, W), dtype=np.uint8)
        pitch = W + pad
        stride = H * pitch + pad
        shape, strides, size = (3, H, W), (stride, pitch, 1), 3 * stride
    buf = torch.empty(offset + size, dtype=torch.uint8, device="cuda")
    view = torch.as_strided(buf, shape, strides, offset)
    view.copy_(torch.from_numpy(host).cuda())
    return view, host


def _front(torch, W, H, kind, layout, seed, pad=0, offset=0, out_pad=0, out_offset=0, grow=0):
    """one to_planes call into canary-filled planes (out_pad bytes after every row, grow extra rows and columns of padding, a guard
    after each buffer); exact against the checker, nothing outside the planes written, the expected instantiation and only it ran"""
    from simd_dct_amd import jpeg_encode as J
    view, host = _image(torch, W, H, kind, layout, seed, pad, offset)
    sampling = [(1, 1)] if kind == "grey" else C.SAMPLING[kind]
    sizes = [(pw + grow, ph + grow) for _, _, pw, ph in J.component_sizes(W, H, sampling)]
    bufs, planes = [], []
    for pw, ph in sizes:
        pitch = pw + out_pad
        b = torch.full((out_offset + ph * pitch + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
        bufs.append((b, pitch))
        planes.append(torch.as_strided(b, (ph, pw), (pitch, 1), out_offset))
    api.kernel_counts_reset()
    J.to_planes(view, "4:2:0" if kind == "grey" else kind, layout, planes=planes)
    ran_exactly(torch, kernel_name(kind, layout))
    want = C.planes(host, kind, layout, padded=sizes)
    for k, ((b, pitch), (pw, ph)) in enumerate(zip(bufs, sizes)):
        a = b.cpu().numpy()
        got = a[out_offset:out_offset + ph * pitch].reshape(ph, pitch)
        assert np.array_equal(got[:, :pw], want[k]), (W, H, kind, layout, k, np.argwhere(got[:, :pw] != want[k])[:4].tolist())
        assert (got[:, pw:] == 0xA5).all() and (a[:out_offset] == 0xA5).all() and (a[out_offset + ph * pitch:] == 0xA5).all(), \
            f"plane {k}: bytes written outside the plane"


KINDS = ["grey", "4:4:4", "4:2:2", "4:2:0"]
ODD = [(1, 1), (1, 17), (17, 1), (15, 15), (33, 31), (1041, 19)]


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["HWC", "CHW"])
@pytest.mark.parametrize("kind", KINDS)
def test_front_odd_sizes(gpu, kind, layout):
    for i, (W, H) in enumerate(ODD):
        _front(gpu, W, H, kind, layout, seed=i)
        # unaligned input and output rows: the one-sample path, same instantiation, same bytes
        _front(gpu, W, H, kind, layout, seed=10 + i, pad=5, offset=3, out_pad=3, out_offset=1)
        # aligned but padded, planes larger than their block grid (padding replication)
        _front(gpu, W, H, kind, layout, seed=20 + i, pad=32 - (3 * W if layout == "HWC" and kind != "grey" else W) % 16, out_pad=48 - W % 16, grow=16)


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,kind,layout", [(8192, 8192, "4:2:0", "HWC"), (8192, 8192, "4:2:0", "CHW"), (7680, 4320, "4:2:0", "HWC"),
                                             (7680, 4320, "4:4:4", "HWC"), (7680, 4320, "4:4:4", "CHW"), (7680, 4320, "4:2:2", "HWC"),
                                             (7680, 4320, "4:2:2", "CHW"), (7680, 4320, "grey", "HWC")])
def test_front_full_frames(gpu, W, H, kind, layout):
    _front(gpu, W, H, kind, layout, seed=W + H)


@pytest.mark.gpu
def test_front_captured_and_replayed_on_new_inputs(gpu):
    torch = gpu
    from simd_dct_amd import jpeg_encode as J
    W, H = 1920, 1080
    view, _ = _image(torch, W, H, "4:2:0", "HWC", seed=1)
    planes = [torch.empty((ph, pw), dtype=torch.uint8, device="cuda") for _, _, pw, ph in J.component_sizes(W, H, C.SAMPLING["4:2:0"])]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        J.to_planes(view, "4:2:0", "HWC", planes=planes, stream=s)
    for seed in (2, 3):
        new, host = _image(torch, W, H, "4:2:0", "HWC", seed=seed)
        view.copy_(new)
        for p in planes:
            p.fill_(0)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for p, w in zip(planes, C.planes(host, "4:2:0")):
            assert np.array_equal(p.cpu().numpy(), w), seed


def _expected_scans(host, kind, q):
    """per component: (the scan jpeg_scan_encoder makes from the oracle's coefficients of the checker's planes, blocks per row)"""
    import oracle as O
    from simd_dct_amd import jpeg_encode as J
    luma, chroma = J.quality_tables(q)
    out = []
    for k, p in enumerate(C.planes(host, kind)):
        ph, pw = p.shape
        coef = O.u8_i16("fwd", p, pw, ph, lut=np.asarray(luma if k == 0 else chroma, dtype=np.float32), level_shift=True)
        t = min(k, 1)
        data, _ = E.encode_scan(dict(width=pw, height=ph, comps=[(1, 1)]), dict(comps=[(0, t, t)], dri=pw // 8), [coef], E.ANNEX_K)
        out.append((data, pw // 8, coef))
    return out


def _check_file(f, host, kind, q, W, H):
    from simd_dct_amd import jpeg_encode as J
    info = jfif.read_jpeg(f)
    sampling = [(1, 1)] if kind == "grey" else C.SAMPLING[kind]
    assert (info["width"], info["height"]) == (W, H)
    assert [(c["h"], c["v"]) for c in info["components"]] == sampling
    luma, chroma = J.quality_tables(q)
    assert info["qtables"][0].tolist() == luma and (kind == "grey" or info["qtables"][1].tolist() == chroma)
    assert all(info["huffman"][key] == (list(v[0]), list(v[1])) for key, v in E.ANNEX_K.items() if kind != "grey" or key[1] == 0)
    want = _expected_scans(host, kind, q)
    assert len(info["scans"]) == len(want)
    for k, (sc, (data, bpr, _)) in enumerate(zip(info["scans"], want)):
        assert sc["restart_interval"] == bpr and [c["index"] for c in sc["components"]] == [k]
        assert f[sc["start"]:sc["end"]] == data, (kind, q, W, H, k)
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_encode_jpeg_bit_exact(gpu, kind):
    from simd_dct_amd import jpeg_encode as J
    rng = np.random.default_rng(5)
    for W, H in ((33, 31), (1, 1), (17, 9)):
        for q in (1, 10, 50, 75, 95, 100):
            host = rng.integers(0, 256, (H, W) if kind == "grey" else (H, W, 3), dtype=np.uint8)
            _check_file(J.encode_jpeg(host, quality=q, subsampling="4:2:0" if kind == "grey" else kind), host, kind, q, W, H)
    from simd_dct_amd import synth
    W, H = 392, 264  # the Python scan encoder sets the size
    host = np.stack([synth.plane_u8_np(W, H, "photo", seed=s) for s in (3, 4, 5)], axis=-1)
    if kind == "grey":
        host = host[..., 0].copy()
    for q in (50, 100):
        _check_file(J.encode_jpeg(gpu.from_numpy(host).cuda(), quality=q, subsampling="4:2:0" if kind == "grey" else kind), host, kind, q, W, H)
    # the one-launch form writes the same file; CHW input the same file as HWC
    f = J.encode_jpeg(host, quality=75, subsampling="4:2:0" if kind == "grey" else kind)
    assert J.encode_jpeg(host, quality=75, subsampling="4:2:0" if kind == "grey" else kind, two_launch=False) == f
    if kind != "grey":
        assert J.encode_jpeg(np.ascontiguousarray(np.moveaxis(host, -1, 0)), quality=75, subsampling=kind, layout="CHW") == f


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_round_trip_through_decode_jpeg(gpu, kind):
    from simd_dct_amd import jpeg_decode as D
    from simd_dct_amd import jpeg_encode as J
    W, H = 37, 29
    rng = np.random.default_rng(11)
    host = rng.integers(0, 256, (H, W) if kind == "grey" else (H, W, 3), dtype=np.uint8)
    f = J.encode_jpeg(host, quality=90, subsampling="4:2:0" if kind == "grey" else kind)
    _, coefs = D.decode_jpeg(f, coefficients=True)
    for c, (_, bpr, want) in zip(coefs, _expected_scans(host, kind, 90)):
        ph, pw = want.shape
        assert np.array_equal(c.cpu().numpy()[:ph, :pw], want)
    rgb = D.decode_jpeg(f, mode="RGB")
    assert tuple(rgb.shape) == (H, W, 3)


def _psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 10 * np.log10(255.0 ** 2 / mse)


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(1024, 768), (1920, 1080)])
def test_against_pillows_encode(gpu, W, H):
    from simd_dct_amd import jpeg_encode as J
    from simd_dct_amd import synth
    host = np.stack([synth.plane_u8_np(W, H, "photo", seed=s) for s in (21, 22, 23)], axis=-1)
    for sub in ("4:4:4", "4:2:2", "4:2:0"):
        for q in (50, 75, 90):
            ours = J.encode_jpeg(host, quality=q, subsampling=sub)
            b = io.BytesIO()
            Image.fromarray(host).save(b, "JPEG", quality=q, subsampling=PIL_SUB[sub])
            theirs = b.getvalue()
            mine = np.asarray(Image.open(io.BytesIO(ours)).convert("RGB"))
            ref = np.asarray(Image.open(io.BytesIO(theirs)).convert("RGB"))
            p_ours, p_ref = _psnr(mine, host), _psnr(ref, host)
            assert p_ours >= p_ref - 0.25, (sub, q, p_ours, p_ref)
            assert abs(len(ours) - len(theirs)) <= 0.05 * len(theirs), (sub, q, len(ours), len(theirs))
