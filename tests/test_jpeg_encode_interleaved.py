"""Colour images as ONE interleaved baseline scan: libmdct_jpegenc_scan.so (include/mdct_jpegenc_scan.h, jpeg_encode.scan_rows),
jfif.write_jpeg's interleaved form and jpeg_encode.encode_jpeg(interleaved=True).

The expected bytes everywhere: the checker's planes (tests/jpeg_encode_checker.py) padded to the MCU grid, the oracle's coefficients of
each plane (tests/oracle.py u8_i16, level shift on) and tests/jpeg_scan_encoder.py coding them as one scan of three components with a
restart interval of one MCU row.

CPU: the container (our reader, the decode checker, Pillow), the C-ABI's refusals, encode_jpeg's argument checks, the code object, the
scan-order arithmetic of the kernels (scan_order.h) under sanitizers.
GPU: scan_rows segment by segment in every instantiation; encode_jpeg's files; agreement with the three-scan path through decode_jpeg;
full frames; Pillow; a captured graph; the retry when the first buffer is too small."""
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_color_checker as CC
import jpeg_decode_checker as DC
import jpeg_encode_checker as C
import jpeg_scan_encoder as E
import oracle as O
from simd_dct_amd import _jpegenc_scan_lib, api, jfif

Image = pytest.importorskip("PIL.Image")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCAN_LIB = os.path.join(ROOT, "simd_dct_amd", "libmdct_jpegenc_scan.so")
# k_scan_rows<H, V>: the luma sampling factors
KERNEL = {"4:4:4": "k_scan_rows<1, 1>", "4:2:2": "k_scan_rows<2, 1>", "4:2:0": "k_scan_rows<2, 2>"}
SUBS = ["4:4:4", "4:2:2", "4:2:0"]
PIL_SUB = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}
SPECS = {0: E.ANNEX_K[(0, 0)], 1: E.ANNEX_K[(1, 0)], 2: E.ANNEX_K[(0, 1)], 3: E.ANNEX_K[(1, 1)]}
SCAN = [(0, 0, 0), (1, 1, 1), (2, 1, 1)]


def mcu_grid(W, H, sampling):
    hmax, vmax = max(h for h, _ in sampling), max(v for _, v in sampling)
    mx, my = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    return mx, my, [(mx * 8 * h, my * 8 * v) for h, v in sampling]


def unstuff(data):
    """the inverse of jfif.stuff"""
    return bytes(data).replace(b"\xff\x00", b"\xff")


def expected(host, sub, q, layout="HWC"):
    """(scan bytes, [un-stuffed data of each MCU row], coefficient planes on the MCU grid, mcus_x, mcus_y)"""
    from simd_dct_amd import jpeg_encode as J
    H, W = (host.shape[0], host.shape[1]) if layout == "HWC" else (host.shape[1], host.shape[2])
    sampling = C.SAMPLING[sub]
    mx, my, sizes = mcu_grid(W, H, sampling)
    luma, chroma = J.quality_tables(q)
    planes = C.planes(host, sub, layout, padded=sizes)
    coefs = [O.u8_i16("fwd", p, p.shape[1], p.shape[0], lut=np.asarray(luma if k == 0 else chroma, dtype=np.float32), level_shift=True) for k, p in enumerate(planes)]
    data, st = E.encode_scan(dict(width=W, height=H, comps=sampling), dict(comps=SCAN, dri=mx), coefs, E.ANNEX_K)
    assert len(st["intervals"]) == my
    return data, [unstuff(data[a:b]) for a, b in st["intervals"]], coefs, mx, my


# ------------------------------------------------------------------------------------------ CPU: the container
@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("W,H", [(37, 29), (9, 17), (1, 1)])
def test_write_jpeg_interleaved(sub, W, H):
    """DC-only planes with quantiser 8 (every IDCT gives exactly dc + 128) on the MCU grid, coded as one scan"""
    sampling = C.SAMPLING[sub]
    mx, my, sizes = mcu_grid(W, H, sampling)
    rng = np.random.default_rng(W + 7 * H)
    coefs, known = [], []
    for (pw, ph), (cw, ch) in zip(sizes, C.true_sizes(W, H, sampling)):
        dc = rng.integers(-128, 128, (ph // 8, pw // 8))
        p = np.zeros((ph, pw), dtype=np.int16)
        p[::8, ::8] = dc
        coefs.append(p)
        known.append(np.kron(dc + 128, np.ones((8, 8), dtype=np.int64))[:ch, :cw].astype(np.uint8))
    data, _ = E.encode_scan(dict(width=W, height=H, comps=sampling), dict(comps=SCAN, dri=mx), coefs, E.ANNEX_K)
    f = jfif.write_jpeg([dict(qtable=[8] * 64)] * 3, W, H, specs=SPECS, sampling=sampling, interleaved=dict(scan=data, mcus_per_row=mx))
    info = jfif.read_jpeg(f)
    assert (info["width"], info["height"]) == (W, H)
    assert [(c["h"], c["v"]) for c in info["components"]] == sampling
    assert len(info["scans"]) == 1
    sc = info["scans"][0]
    assert sc["restart_interval"] == mx
    assert [(c["index"], c["td"], c["ta"]) for c in sc["components"]] == SCAN
    assert f[sc["start"]:sc["end"]] == data
    got, st, _ = DC.decode(f)
    assert len(st) == 1 and len(st[0]) == my and all(s == DC.OK for s in st[0])
    for g, w in zip(got, coefs):
        assert np.array_equal(g, w)
    im = Image.open(io.BytesIO(f))
    im.load()
    assert np.array_equal(np.asarray(im.convert("RGB")), CC.to_rgb(known, sampling, W, H))


# ------------------------------------------------------------------------------------------ CPU: refusals, code object
def _plane(px, pitch, w, h, hh=1, vv=1):
    return _jpegenc_scan_lib.Plane(px, pitch, w, h, hh, vv)


def test_cabi_refusals_without_device():
    lib = _jpegenc_scan_lib.load()
    A, OUT, SB, FF = 1 << 40, 1 << 44, 1 << 45, 1 << 46  # addresses far apart; nothing is dereferenced
    good = (np.full(64, 16, dtype=np.float32), np.full(64, 17, dtype=np.float32))
    ok = [_plane(A, 64, 64, 32, 2, 2), _plane(A + (1 << 30), 32, 32, 16), _plane(A + (2 << 30), 32, 32, 16)]  # 4 x 2 MCUs of 4:2:0
    stride = int(lib.mdct_jpegenc_scan_seg_stride(4, 6))
    assert stride == 208 * 24 + 8

    def call(planes=ok, n=3, luma=good[0], chroma=good[1], my0=0, my1=2, out=OUT, seg_stride=stride, sb=SB, ff=FF):
        arr = None if planes is None else (_jpegenc_scan_lib.Plane * max(1, len(planes)))(*planes)
        rc = lib.mdct_jpegenc_scan_rows(arr, n, None if luma is None else luma.ctypes.data, None if chroma is None else chroma.ctypes.data, my0, my1,
                                        out, seg_stride, sb, ff, None)
        return rc, lib.mdct_jpegenc_scan_last_error().decode()

    def table(i, v):
        t = good[0].copy()
        t[i] = v
        return t

    p422 = [_plane(A, 64, 64, 16, 2, 1), ok[1], ok[2]]
    cases = {
        "null planes": dict(planes=None),
        "null plane": dict(planes=[ok[0], _plane(0, 32, 32, 16), ok[2]]),
        "null luma table": dict(luma=None),
        "null chroma table": dict(chroma=None),
        "null out": dict(out=None),
        "null seg_bytes": dict(sb=None),
        "null ff_counts": dict(ff=None),
        "one plane": dict(planes=ok[:1], n=1),
        "two planes": dict(n=2),
        "four planes": dict(planes=ok + ok[:1], n=4),
        "4:1:1": dict(planes=[_plane(A, 128, 128, 16, 4, 1), ok[1], ok[2]]),
        "4:4:0": dict(planes=[_plane(A, 32, 32, 32, 1, 2), ok[1], ok[2]]),
        "chroma 2x1": dict(planes=[ok[0], _plane(A + (1 << 30), 64, 64, 16, 2, 1), ok[2]]),
        "luma narrower than the MCU grid": dict(planes=[_plane(A, 64, 56, 32, 2, 2), ok[1], ok[2]]),
        "luma on the block grid only": dict(planes=[_plane(A, 64, 64, 24, 2, 2), ok[1], ok[2]]),
        "chroma planes differ": dict(planes=[ok[0], ok[1], _plane(A + (2 << 30), 32, 32, 8)]),
        "width not a multiple of 8": dict(planes=[_plane(A, 68, 68, 32, 2, 2), _plane(A + (1 << 30), 34, 34, 16), _plane(A + (2 << 30), 34, 34, 16)]),
        "empty planes": dict(planes=[_plane(A, 64, 0, 32, 2, 2), _plane(A + (1 << 30), 32, 0, 16), _plane(A + (2 << 30), 32, 0, 16)]),
        "luma wider than 65536": dict(planes=[_plane(A, 65552, 65552, 32, 2, 2), _plane(A + (1 << 30), 32776, 32776, 16), _plane(A + (2 << 30), 32776, 32776, 16)]),
        "4:4:4 taller than 65536": dict(planes=[_plane(A + (k << 36), 8, 8, 65544) for k in range(3)], my1=1),
        "luma pitch": dict(planes=[_plane(A, 63, 64, 32, 2, 2), ok[1], ok[2]]),
        "chroma pitch": dict(planes=[ok[0], ok[1], _plane(A + (2 << 30), 31, 32, 16)]),
        "my0 == my1": dict(my0=1, my1=1),
        "my0 > my1": dict(my0=2, my1=1),
        "my1 > mcus_y": dict(my1=3),
        "4:2:2 my1 > mcus_y": dict(planes=p422, my1=3, seg_stride=int(lib.mdct_jpegenc_scan_seg_stride(4, 4))),
        "stride too small": dict(seg_stride=stride - 4),
        "4:2:0 with the 4:2:2 stride": dict(seg_stride=int(lib.mdct_jpegenc_scan_seg_stride(4, 4))),
        "stride not a multiple of 4": dict(seg_stride=stride + 2),
        "out not 4-byte aligned": dict(out=OUT + 2),
        "zero luma entry": dict(luma=table(5, 0.0)),
        "NaN luma entry": dict(luma=table(63, np.nan)),
        "infinite chroma entry": dict(chroma=table(0, np.inf)),
        "zero chroma entry": dict(chroma=table(17, -0.0)),
    }
    for name, kw in cases.items():
        rc, msg = call(**kw)
        assert rc == 1, (name, rc, msg)  # MDCT_INVALID_PARAMETER
        assert msg, name


def test_encode_jpeg_refuses_bad_arguments_before_the_device(monkeypatch):
    from simd_dct_amd import jpeg_encode as J

    def no_device(*a, **k):
        raise AssertionError("device work before the arguments were checked")

    monkeypatch.setattr(J, "to_planes", no_device)
    monkeypatch.setattr(J, "scan_rows", no_device)
    monkeypatch.setattr(J, "_run_scan", no_device)
    img = np.zeros((16, 16, 3), dtype=np.uint8)
    for bad in (1, 0, None, "yes", 1.0, [True]):
        with pytest.raises(ValueError):
            J.encode_jpeg(img, interleaved=bad)
        with pytest.raises(ValueError):
            J.encode_jpeg(img[..., 0], interleaved=bad)
    for kw in (dict(quality=0), dict(quality=101), dict(quality=7.5), dict(quality=True), dict(quality="75"), dict(subsampling="4:1:1"),
               dict(subsampling=None), dict(layout="HCW"), dict(layout="CHW")):
        with pytest.raises(ValueError):
            J.encode_jpeg(img, interleaved=True, **kw)
    for bad in (img.astype(np.int16), np.zeros((16, 16, 4), np.uint8), np.zeros((2, 16, 16, 3), np.uint8), np.zeros((16,), np.uint8),
                np.zeros((0, 16), np.uint8), np.zeros((16, 65536), np.uint8), [[1, 2], [3, 4]]):
        with pytest.raises(ValueError):
            J.encode_jpeg(bad, interleaved=True)


def test_code_object_holds_the_planned_instantiations():
    from test_kernel_coverage import code_object_kernels
    names, n_objects = code_object_kernels(lib=SCAN_LIB)
    assert n_objects == 1 and names == set(KERNEL.values()), sorted(names ^ set(KERNEL.values()))


def test_scan_order_under_sanitizers(tmp_path):
    """scan_order.h's seq_block<H, V> -- which LDS row a thread of k_scan_rows / k_opt codes and where its DC predictor lives -- for every
    thread of the four layouts against T.81 A.2.3 as tests/scan_order_driver.cpp states it: a stand-alone program, sanitizers linked in"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "scan_order"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "simd_dct_amd", "csrc"), os.path.join(ROOT, "tests", "scan_order_driver.cpp"),
                        "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0 and "san" in (r.stderr + r.stdout).lower() and "cannot find" in (r.stderr + r.stdout).lower():
        pytest.skip("sanitizer runtime not installed: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "scan order ok" in r.stdout, r.stdout + r.stderr


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
    ran = {k: v for k, v in api.kernel_counts().items() if k.startswith("k_scan_rows")}
    assert ran == {want: 1}, (want, ran)


def _content(W, H, content, seed):
    if content == "photo":
        from simd_dct_amd import synth
        return np.stack([synth.plane_u8_np(W, H, "photo", seed=seed + s) for s in range(3)], axis=-1)
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def _scan_rows(torch, W, H, sub, q, content="random", seed=0, pad=0, offset=0, rows=None, extra_stride=0):
    """one scan_rows call on the checker's planes (pad bytes after every plane row, planes offset bytes into their buffers) into
    canary-filled buffers: every coded MCU row's segment, byte count and 0xFF count against the expected interval; nothing written
    after a segment's bytes up to a word, in the untouched rows or after the buffers; the expected instantiation ran, once"""
    from simd_dct_amd import jpeg_encode as J
    host = _content(W, H, content, seed)
    sampling = C.SAMPLING[sub]
    _, want, _, mx, my = expected(host, sub, q)
    _, _, sizes = mcu_grid(W, H, sampling)
    planes = []
    for p, (pw, ph) in zip(C.planes(host, sub, padded=sizes), sizes):
        pitch = pw + pad
        b = torch.zeros((offset + ph * pitch,), dtype=torch.uint8, device="cuda")
        v = torch.as_strided(b, (ph, pw), (pitch, 1), offset)
        v.copy_(torch.from_numpy(p).cuda())
        planes.append(v)
    stride = J.scan_seg_stride(mx, sampling) + extra_stride
    assert stride == 208 * mx * sum(h * v for h, v in sampling) + 8 + extra_stride
    guard = 4096
    seg = torch.full((my * stride + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    counts = torch.full((2, my + 8), -7, dtype=torch.int32, device="cuda")
    my0, my1 = rows if rows is not None else (0, my)
    api.kernel_counts_reset()
    J.scan_rows(planes, sampling, J.quality_tables(q), seg, counts[0], counts[1], seg_stride=stride, my0=my0, my1=my1)
    ran_exactly(torch, KERNEL[sub])
    s, c = seg.cpu().numpy(), counts.cpu().numpy()
    assert (s[my * stride:] == 0xA5).all(), "bytes written after the segment buffer"
    for r in range(my):
        row = s[r * stride:(r + 1) * stride]
        if not my0 <= r < my1:
            assert (row == 0xA5).all() and c[0, r] == -7 and c[1, r] == -7, f"MCU row {r} outside [{my0}, {my1}) was touched"
            continue
        w = want[r]
        assert c[0, r] == len(w), (sub, W, H, q, r, int(c[0, r]), len(w))
        assert row[:len(w)].tobytes() == w, (sub, W, H, q, r, int(np.flatnonzero(row[:len(w)] != np.frombuffer(w, dtype=np.uint8))[0]))
        assert c[1, r] == w.count(b"\xff"), (sub, W, H, q, r)
        assert (row[-(-len(w) // 4) * 4:] == 0xA5).all(), f"MCU row {r}: bytes written beyond the segment's last word"
    assert (c[:, my:] == -7).all(), "counts written after the arrays"
    return host


# widths giving mcus_x of 1, 2, 31, 32, 33, 65 in every subsampling (MCU 16 or 8 wide), through odd true sizes
def _width(sub, mcus_x, trim):
    return mcus_x * (8 if sub == "4:4:4" else 16) - trim


@pytest.mark.gpu
@pytest.mark.parametrize("sub", SUBS)
def test_scan_rows_chunk_boundaries(gpu, sub):
    for i, (mx, trim, H) in enumerate([(1, 7, 1), (2, 0, 16), (31, 3, 40), (32, 0, 16), (33, 5, 33), (65, 1, 24)]):
        _scan_rows(gpu, _width(sub, mx, trim), H, sub, 50, seed=i)
    # unaligned plane rows and bases; a longer stride
    _scan_rows(gpu, _width(sub, 33, 2), 35, sub, 50, seed=10, pad=5, offset=3)
    _scan_rows(gpu, _width(sub, 65, 0), 16, sub, 75, seed=11, pad=1, offset=1, extra_stride=64)


@pytest.mark.gpu
@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("q", [1, 50, 100])
def test_scan_rows_random_pixels(gpu, sub, q):
    """quality 100 noise: the longest blocks, several ring windows per chunk; quality 1: all-zero blocks"""
    _scan_rows(gpu, _width(sub, 70, 4), 50, sub, q, seed=q)


@pytest.mark.gpu
@pytest.mark.parametrize("sub", SUBS)
def test_scan_rows_photo_hundreds_of_mcus(gpu, sub):
    _scan_rows(gpu, _width(sub, 260, 0), 40, sub, 75, content="photo", seed=3)


@pytest.mark.gpu
@pytest.mark.parametrize("sub", SUBS)
def test_scan_rows_sub_range(gpu, sub):
    _scan_rows(gpu, _width(sub, 40, 1), 100, sub, 90, seed=4, rows=(2, 5), pad=3)
    _scan_rows(gpu, _width(sub, 40, 1), 100, sub, 90, seed=4, rows=(0, 1))


def _check_file(f, host, sub, q, layout="HWC"):
    from simd_dct_amd import jpeg_encode as J
    data, _, coefs, mx, my = expected(host, sub, q, layout)
    H, W = (host.shape[0], host.shape[1]) if layout == "HWC" else (host.shape[1], host.shape[2])
    info = jfif.read_jpeg(f)
    assert (info["width"], info["height"]) == (W, H)
    assert [(c["h"], c["v"]) for c in info["components"]] == C.SAMPLING[sub]
    luma, chroma = J.quality_tables(q)
    assert info["qtables"][0].tolist() == luma and info["qtables"][1].tolist() == chroma
    assert all(info["huffman"][key] == (list(v[0]), list(v[1])) for key, v in E.ANNEX_K.items())
    assert len(info["scans"]) == 1
    sc = info["scans"][0]
    assert sc["restart_interval"] == mx and [(c["index"], c["td"], c["ta"]) for c in sc["components"]] == SCAN
    assert f[sc["start"]:sc["end"]] == data, (sub, q, W, H)
    return coefs


@pytest.mark.gpu
@pytest.mark.parametrize("sub", SUBS)
def test_encode_jpeg_interleaved_bit_exact(gpu, sub):
    from simd_dct_amd import jpeg_encode as J
    from simd_dct_amd import synth
    rng = np.random.default_rng(5)
    for W, H in ((33, 31), (1, 1), (17, 9)):
        for q in (1, 10, 50, 75, 95, 100):
            host = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            _check_file(J.encode_jpeg(host, quality=q, subsampling=sub, interleaved=True), host, sub, q)
    W, H = 392, 264
    host = np.stack([synth.plane_u8_np(W, H, "photo", seed=s) for s in (3, 4, 5)], axis=-1)
    for q in (50, 100):
        _check_file(J.encode_jpeg(gpu.from_numpy(host).cuda(), quality=q, subsampling=sub, interleaved=True), host, sub, q)
    f = J.encode_jpeg(host, quality=75, subsampling=sub, interleaved=True)
    _check_file(f, host, sub, 75)
    assert J.encode_jpeg(np.ascontiguousarray(np.moveaxis(host, -1, 0)), quality=75, subsampling=sub, layout="CHW", interleaved=True) == f
    assert J.encode_jpeg(host, quality=75, subsampling=sub, interleaved=True, two_launch=False) == f


@pytest.mark.gpu
def test_grey_is_the_same_file(gpu):
    from simd_dct_amd import jpeg_encode as J
    rng = np.random.default_rng(6)
    for W, H in ((33, 31), (64, 40)):
        host = rng.integers(0, 256, (H, W), dtype=np.uint8)
        assert J.encode_jpeg(host, quality=80, interleaved=True) == J.encode_jpeg(host, quality=80)


@pytest.mark.gpu
@pytest.mark.parametrize("sub", SUBS)
def test_agrees_with_the_three_scan_path(gpu, sub):
    from simd_dct_amd import jpeg_decode as D
    from simd_dct_amd import jpeg_encode as J
    for W, H, seed in ((37, 29, 11), (200, 120, 12)):
        host = _content(W, H, "photo" if W > 100 else "random", seed)
        one = J.encode_jpeg(host, quality=90, subsampling=sub, interleaved=True)
        three = J.encode_jpeg(host, quality=90, subsampling=sub)
        assert len(jfif.read_jpeg(one)["scans"]) == 1 and len(jfif.read_jpeg(three)["scans"]) == 3
        _, c1 = D.decode_jpeg(one, coefficients=True)
        _, c3 = D.decode_jpeg(three, coefficients=True)
        for a, b, (_, _, pw, ph) in zip(c1, c3, J.component_sizes(W, H, C.SAMPLING[sub])):
            assert np.array_equal(a.cpu().numpy()[:ph, :pw], b.cpu().numpy()[:ph, :pw])
        assert gpu.equal(D.decode_jpeg(one, mode="RGB"), D.decode_jpeg(three, mode="RGB"))


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,sub", [(8192, 8192, "4:2:0"), (7680, 4320, "4:2:0"), (7680, 4320, "4:2:2"), (7680, 4320, "4:4:4"), (1041, 19, "4:2:0")])
def test_full_frames_through_decode_jpeg(gpu, W, H, sub):
    """where the Python scan encoder is too slow: our own decoder returns the oracle's coefficients on the MCU grid"""
    from simd_dct_amd import jpeg_decode as D
    from simd_dct_amd import jpeg_encode as J
    host = _content(W, H, "photo", W + H)
    f = J.encode_jpeg(host, quality=75, subsampling=sub, interleaved=True)
    info = jfif.read_jpeg(f)
    mx, my, sizes = mcu_grid(W, H, C.SAMPLING[sub])
    assert len(info["scans"]) == 1 and info["scans"][0]["restart_interval"] == mx
    _, coefs = D.decode_jpeg(f, coefficients=True)
    luma, chroma = J.quality_tables(75)
    for k, (c, p) in enumerate(zip(coefs, C.planes(host, sub, padded=sizes))):
        want = O.u8_i16("fwd", p, p.shape[1], p.shape[0], lut=np.asarray(luma if k == 0 else chroma, dtype=np.float32), level_shift=True)
        assert np.array_equal(c.cpu().numpy()[:p.shape[0], :p.shape[1]], want), (k, W, H, sub)


def _psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 10 * np.log10(255.0 ** 2 / mse)


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(1024, 768), (1920, 1080)])
def test_against_pillows_encode(gpu, W, H):
    """the images, settings and bounds of test_jpeg_encode.py::test_against_pillows_encode"""
    from simd_dct_amd import jpeg_encode as J
    from simd_dct_amd import synth
    host = np.stack([synth.plane_u8_np(W, H, "photo", seed=s) for s in (21, 22, 23)], axis=-1)
    for sub in SUBS:
        for q in (50, 75, 90):
            ours = J.encode_jpeg(host, quality=q, subsampling=sub, interleaved=True)
            b = io.BytesIO()
            Image.fromarray(host).save(b, "JPEG", quality=q, subsampling=PIL_SUB[sub])
            theirs = b.getvalue()
            mine = np.asarray(Image.open(io.BytesIO(ours)).convert("RGB"))
            ref = np.asarray(Image.open(io.BytesIO(theirs)).convert("RGB"))
            p_ours, p_ref = _psnr(mine, host), _psnr(ref, host)
            assert p_ours >= p_ref - 0.25, (sub, q, p_ours, p_ref)
            assert abs(len(ours) - len(theirs)) <= 0.05 * len(theirs), (sub, q, len(ours), len(theirs))


@pytest.mark.gpu
def test_captured_and_replayed_on_new_images(gpu):
    torch = gpu
    from simd_dct_amd import jpeg_encode as J
    W, H, sub, q = 328, 200, "4:2:0", 75
    sampling = C.SAMPLING[sub]
    mx, my, sizes = mcu_grid(W, H, sampling)
    image = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    planes = [torch.empty((ph, pw), dtype=torch.uint8, device="cuda") for pw, ph in sizes]
    stride = J.scan_seg_stride(mx, sampling)
    seg = torch.empty((my * stride,), dtype=torch.uint8, device="cuda")
    counts = torch.empty((2, my), dtype=torch.int32, device="cuda")
    out = torch.empty((2 * my * stride,), dtype=torch.uint8, device="cuda")
    off = torch.empty((my + 1,), dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        J.to_planes(image, sub, "HWC", planes=planes, stream=s)
        J.scan_rows(planes, sampling, J.quality_tables(q), seg, counts[0], counts[1], seg_stride=stride, stream=s)
        api.jpeg_pack_rows(seg, counts[0], stride, my, out, off, ff_counts=counts[1], stream=s)
    for seed in (2, 3):
        host = _content(W, H, "random" if seed == 2 else "photo", seed)
        image.copy_(torch.from_numpy(host).cuda())
        for t in (seg, out):
            t.fill_(0)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want = expected(host, sub, q)[0]
        n = int(off[-1].item())
        assert n == len(want) and out[:n].cpu().numpy().tobytes() == want, seed


@pytest.mark.gpu
@pytest.mark.parametrize("sub", SUBS)
def test_scan_that_does_not_fit_is_packed_again(gpu, sub, monkeypatch):
    from simd_dct_amd import jpeg_encode as J
    W, H = 150, 90
    host = _content(W, H, "random", 9)
    want = J.encode_jpeg(host, quality=100, subsampling=sub, interleaved=True)
    _check_file(want, host, sub, 100)
    calls = []
    packer = api.jpeg_pack_rows

    def counted(*a, **k):
        calls.append(a[4].numel())
        return packer(*a, **k)

    monkeypatch.setattr(J, "_first_capacity", lambda pixels: 64)
    monkeypatch.setattr(J.api, "jpeg_pack_rows", counted)
    assert J.encode_jpeg(host, quality=100, subsampling=sub, interleaved=True) == want
    assert len(calls) == 2 and calls[0] == 64 and calls[1] > len(want)
