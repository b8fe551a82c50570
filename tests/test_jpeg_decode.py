"""The GPU JPEG decoder (libmdct_jpegdec.so, include/mdct_jpegdec.h, simd_dct_amd/jpeg_decode.py) and the file reader
jfif.read_jpeg.

CPU: the reader on the engine's own files and on Pillow's, its refusals, the table validation (and the decoders' host-compilable
headers in a stand-alone program under sanitizers: tests/jpegdec_host_driver.cpp), and the independent CPU checker
(tests/jpeg_decode_checker.py) anchored twice -- against the encoder's CPU checker (the levels the scans were made from) and against
libjpeg (Pillow's decode of the same files, within the +-1 of two IDCTs).
GPU: the engine's own scans decode to exactly the coefficients and pixels the encoder side computes; Pillow's files decode to exactly
the checker's coefficients; producer offsets; malformed scans (status per interval as the checker classifies it, other intervals
intact, nothing written outside the planes); a captured decode replayed; every kernel of the library's code object launched."""
import io
import os

import numpy as np
import pytest

import jpeg_decode_checker as C
import oracle as O
from simd_dct_amd import api, jfif, synth

Image = pytest.importorskip("PIL.Image")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JPEGDEC_LIB = os.path.join(ROOT, "simd_dct_amd", "libmdct_jpegdec.so")
K1, K2 = synth.JPEG_LUMA, synth.JPEG_CHROMA


def _picture(W, H, seed, colour=False):
    if colour:
        return np.stack([synth.plane_u8_np(W, H, "photo", seed=seed + k) for k in range(3)], axis=-1)
    return synth.plane_u8_np(W, H, "photo", seed=seed)


def pillow_jpeg(img, **kw):
    buf = io.BytesIO()
    Image.fromarray(img, "L" if img.ndim == 2 else "YCbCr").save(buf, "JPEG", **kw)
    return buf.getvalue()


def _engine_cpu_scan(img, qtable, chroma=False):
    """the encoder's CPU checker: pixels -> coefficients -> records -> Huffman rows -> packed, stuffed scan"""
    H, W = img.shape
    coef = O.u8_i16("fwd", img, W, H, lut=qtable)
    lv, rn, ct = O.zigzag_rle("i16", coef, W, H)
    seg, nb, stride = O.huffman_rows(lv, rn, ct, W, H, chroma=chroma)
    out, off = O.jpeg_pack_rows(seg, nb, stride)
    return coef, out[:int(off[-1])].tobytes(), off


def engine_file_cpu(planes):
    """planes: [(img, qtable, chroma)] (1 grey or Y Cb Cr at 4:2:0) -> (file, coefficient planes)"""
    comps, coefs = [], []
    for img, q, chroma in planes:
        coef, scan, _ = _engine_cpu_scan(img, q, chroma)
        comps.append(dict(blocks_per_row=img.shape[1] // 8, qtable=q, scan=np.frombuffer(scan, dtype=np.uint8)))
        coefs.append(coef)
    H, W = planes[0][0].shape
    return jfif.write_jpeg(comps, W, H), coefs


# ------------------------------------------------------------------------------------------ CPU: the reader
def test_read_jpeg_on_the_engines_grey_file():
    img = _picture(264, 40, 1)
    data, _ = engine_file_cpu([(img, K1, False)])
    info = jfif.read_jpeg(data)
    assert (info["width"], info["height"], info["sof"]) == (264, 40, 0xC0)
    assert info["components"] == [dict(id=1, h=1, v=1, tq=0)]
    assert np.array_equal(info["qtables"][0], K1.astype(np.uint16))
    assert info["huffman"][(0, 0)] == tuple(api.huffman_spec(0)) and info["huffman"][(1, 0)] == tuple(api.huffman_spec(1))
    (sc,) = info["scans"]
    assert sc["restart_interval"] == 33 and sc["components"] == [dict(index=0, td=0, ta=0)]
    _, scan, _ = _engine_cpu_scan(img, K1)
    assert data[sc["start"]:sc["end"]] == scan


def test_read_jpeg_on_the_engines_420_file_three_scans():
    W, H = 96, 48
    ycc = _picture(W, H, 2, colour=True)
    y, cb, cr = (p.astype(np.int32) + 128 for p in O.split420(ycc, W, H))
    planes = [(y.astype(np.uint8), K1, False), (cb.astype(np.uint8), K2, True), (cr.astype(np.uint8), K2, True)]
    data, _ = engine_file_cpu(planes)
    info = jfif.read_jpeg(data)
    assert (info["width"], info["height"]) == (W, H)
    assert [(c["h"], c["v"], c["tq"]) for c in info["components"]] == [(2, 2, 0), (1, 1, 1), (1, 1, 1)]
    assert np.array_equal(info["qtables"][1], K2.astype(np.uint16))
    assert [s["restart_interval"] for s in info["scans"]] == [W // 8, W // 16, W // 16]
    assert [s["components"] for s in info["scans"]] == [[dict(index=i, td=t, ta=t)] for i, t in ((0, 0), (1, 1), (2, 1))]
    for s, (img, q, chroma) in zip(info["scans"], planes):
        assert data[s["start"]:s["end"]] == _engine_cpu_scan(img, q, chroma)[1]


PILLOW_CASES = [  # (size, colour, save options)
    ((72, 40), False, dict(quality=75, restart_marker_rows=1)),
    ((100, 52), True, dict(quality=75, subsampling=0, restart_marker_rows=1)),
    ((100, 52), True, dict(quality=75, subsampling=1, restart_marker_blocks=5)),
    ((100, 52), True, dict(quality=75, subsampling=2, restart_marker_blocks=3, optimize=True)),
    ((61, 37), True, dict(quality=5, subsampling=2, restart_marker_rows=1)),
    ((61, 37), False, dict(quality=100, restart_marker_blocks=7, optimize=True)),
    ((64, 33), True, dict(quality=100, subsampling=2, restart_marker_rows=1, optimize=True)),
]


@pytest.mark.parametrize("size,colour,kw", PILLOW_CASES, ids=[f"{s[0]}x{s[1]}-{'c' if c else 'g'}-{k}" for s, c, k in PILLOW_CASES])
def test_read_jpeg_on_pillow_files(size, colour, kw):
    data = pillow_jpeg(_picture(*size, 3, colour), **kw)
    info = jfif.read_jpeg(data)
    assert (info["width"], info["height"]) == size
    sub = {0: (1, 1), 1: (2, 1), 2: (2, 2)}[kw.get("subsampling", 2)]
    if colour:
        assert [(c["h"], c["v"]) for c in info["components"]] == [sub, (1, 1), (1, 1)]
        assert len(info["scans"]) == 1 and len(info["scans"][0]["components"]) == 3  # one interleaved scan
    else:
        assert [(c["h"], c["v"]) for c in info["components"]] == [(1, 1)]
    hmax, vmax = info["components"][0]["h"], info["components"][0]["v"]
    mcus_x = -(-size[0] // (8 * hmax)) if colour else -(-size[0] // 8)
    ri = info["scans"][0]["restart_interval"]
    assert ri == (mcus_x if "restart_marker_rows" in kw else kw["restart_marker_blocks"])
    for key, (bits, vals) in info["huffman"].items():
        assert sum(bits) == len(vals) and key[0] in (0, 1)
    assert all(q.min() >= 1 for q in info["qtables"].values())


def _edit_marker(data, old, new):
    i = data.index(bytes([0xFF, old]))
    return data[:i] + bytes([0xFF, new]) + data[i + 2:]


def test_read_jpeg_refusals():
    img = _picture(64, 32, 4)
    with pytest.raises(jfif.JpegFormatError, match="progressive"):
        jfif.read_jpeg(pillow_jpeg(img, progressive=True, restart_marker_rows=1))
    with pytest.raises(jfif.JpegFormatError, match="restart"):
        jfif.read_jpeg(pillow_jpeg(img, quality=75))  # Pillow's default: no DRI
    good = pillow_jpeg(img, quality=75, restart_marker_rows=1)
    with pytest.raises(jfif.JpegFormatError, match="progressive"):
        jfif.read_jpeg(_edit_marker(good, 0xC0, 0xC2))
    with pytest.raises(jfif.JpegFormatError, match="arithmetic"):
        jfif.read_jpeg(_edit_marker(good, 0xC0, 0xC9))
    i = good.index(b"\xff\xdb")
    sixteen = good[:i + 4] + bytes([0x10]) + good[i + 5:]
    with pytest.raises(jfif.JpegFormatError, match="16-bit DQT"):
        jfif.read_jpeg(sixteen)
    i = good.index(b"\xff\xc0")
    twelve = good[:i + 4] + bytes([12]) + good[i + 5:]
    with pytest.raises(jfif.JpegFormatError, match="12-bit"):
        jfif.read_jpeg(twelve)


# ------------------------------------------------------------------------------------------ CPU: the tables
def _specs(which=(0, 1, 2, 3)):
    s = [api.huffman_spec(w) for w in which]
    return [s[0], s[2], s[1], s[3]]  # slots: DC luma, DC chroma, AC luma, AC chroma


def test_table_validation_without_device():
    from simd_dct_amd import jpeg_decode as D
    assert D.tables_check(_specs()) == 0
    assert D.tables_check([_specs()[0], None, _specs()[2], None]) == 0
    over = [0] * 16
    over[1] = 5  # five 2-bit codes: over-subscribed
    assert D.tables_check([(over, [0, 1, 2, 3, 4]), None, None, None]) == 1
    assert "over-subscribed" in D.last_error()
    full = [0] * 16
    full[0] = 2  # both 1-bit codes: the all-ones code, refused as libjpeg does
    assert D.tables_check([(full, [0, 1]), None, None, None]) == 1
    many = [0] * 16
    many[15] = 255
    many[14] = 2
    assert D.tables_check([(many, list(range(12)) * 21 + [0] * 5), None, None, None]) == 1  # 257 values
    assert D.tables_check([(_specs()[0][0], _specs()[0][1][:-1]), None, None, None]) == 1  # counts and values disagree
    assert D.tables_check([(_specs()[2][0], [12] + _specs()[0][1][1:]), None, None, None]) == 1  # DC category 12


def _counts(length, n):
    bits = [0] * 16
    bits[length - 1] = n
    return bits


# slot, (bits16, vals): what build_tables (csrc/huff_tables.h) refuses, the over-subscribed ones before it writes anything for the length
REFUSED_SPECS = {
    "three 1-bit codes": (0, (_counts(1, 3), [0, 0, 0])),
    "255 1-bit codes": (2, (_counts(1, 255), [1] * 255)),
    "five 2-bit codes": (1, (_counts(2, 5), [0] * 5)),
    "an all-ones code": (3, ([1, 2] + [0] * 14, [0, 1, 2])),
    "257 values": (2, (_counts(8, 255), [0] * 257)),
    "counts that disagree with the values": (0, (_counts(2, 2), [0, 1, 2])),
    "DC category 12": (0, (_counts(4, 1), [12])),
    "AC size 11": (2, (_counts(4, 1), [0x0B])),
}


@pytest.mark.parametrize("case", sorted(REFUSED_SPECS))
def test_tables_create_refuses_what_tables_check_refuses(case):
    """mdct_jpegdec_tables_create builds into a real table struct where mdct_jpegdec_tables_check only validates: the same code and
    message, no handle, and all of it before the first HIP call (so without a device)"""
    import ctypes

    from simd_dct_amd import _jpegdec_lib
    from simd_dct_amd import jpeg_decode as D
    slot, spec = REFUSED_SPECS[case]
    specs = [spec if t == slot else None for t in range(4)]
    rc = D.tables_check(specs)
    message = D.last_error()
    assert rc == 1 and f"slot {slot}: " in message, (rc, message)
    b, v, n, keep = D._spec_arrays(specs)
    handle = ctypes.c_void_p(0xDEAD)
    assert _jpegdec_lib.load().mdct_jpegdec_tables_create(ctypes.byref(handle), b, v, n) == rc
    assert D.last_error() == message
    assert handle.value is None


def test_host_pieces_under_sanitizers(tmp_path):
    """csrc/huff_tables.h (build_tables writing a real DevTables: every code of the tables it accepts, the specifications it refuses,
    nothing written outside the struct) and csrc/block_place.h (the place of every block of five MCU layouts against T.81 A.2.3, the
    loop that zeroes a range of blocks) as tests/jpegdec_host_driver.cpp checks them: a stand-alone program, sanitizers linked in"""
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "jpegdec_host"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "simd_dct_amd", "csrc"), os.path.join(ROOT, "tests", "jpegdec_host_driver.cpp"),
                        "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0 and "san" in (r.stderr + r.stdout).lower() and "cannot find" in (r.stderr + r.stdout).lower():
        pytest.skip("sanitizer runtime not installed: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "jpegdec host ok" in r.stdout, r.stdout + r.stderr


# ------------------------------------------------------------------------------------------ CPU: the checker, anchored twice
@pytest.mark.parametrize("W,H", [(264, 24), (64, 8), (8, 16)])
def test_checker_decodes_the_encoder_checkers_scans(W, H):
    img = _picture(W, H, 5)
    data, (coef,) = engine_file_cpu([(img, K1, False)])
    planes, st, _ = C.decode(data)
    assert st == [[C.OK] * (H // 8)]
    assert np.array_equal(planes[0], coef)


def test_checker_decodes_the_encoder_checkers_420_scans():
    W, H = 96, 32
    ycc = _picture(W, H, 6, colour=True)
    y, cb, cr = (p.astype(np.int32) + 128 for p in O.split420(ycc, W, H))
    data, coefs = engine_file_cpu([(y.astype(np.uint8), K1, False), (cb.astype(np.uint8), K2, True), (cr.astype(np.uint8), K2, True)])
    planes, st, _ = C.decode(data)
    assert all(s == [C.OK] * len(s) for s in st)
    for p, c in zip(planes, coefs):
        assert np.array_equal(p[:c.shape[0], :c.shape[1]], c)


def _libjpeg_luma(data):
    im = Image.open(io.BytesIO(data))
    if im.mode != "L":
        im.draft("YCbCr", im.size)
        assert im.mode == "YCbCr"
        return np.asarray(im)[:, :, 0]
    return np.asarray(im)


def checker_pixels(data):
    planes, st, meta = C.decode(data)
    assert all(s == C.OK for ss in st for s in ss), st
    return planes, [O.u8_i16("inv", p, p.shape[1], p.shape[0], lut=q) for p, q in zip(planes, meta["qtables"])]


@pytest.mark.parametrize("size,colour,kw", PILLOW_CASES, ids=[f"{s[0]}x{s[1]}-{'c' if c else 'g'}-{k}" for s, c, k in PILLOW_CASES])
def test_checker_against_libjpeg(size, colour, kw):
    data = pillow_jpeg(_picture(*size, 7, colour), **kw)
    _, px = checker_pixels(data)
    W, H = size
    d = np.abs(px[0][:H, :W].astype(int) - _libjpeg_luma(data).astype(int))
    assert d.max() <= 1, int(d.max())


# ------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    torch.cuda.set_device(0)
    api.init(0)
    return torch


def gpu_scan(px, W, H, lut, chroma=False):
    """mdct_fwd_u8_jpeg_scan on a device plane -> (scan bytes on the device, row offsets on the device, length)"""
    import torch
    stride = api.huffman_seg_stride(W)
    n = H // 8
    seg = torch.empty((n * stride,), dtype=torch.uint8, device="cuda")
    work = torch.zeros((n + 2,), dtype=torch.int64, device="cuda")
    cap = n * stride * 2
    out = torch.empty((cap,), dtype=torch.uint8, device="cuda")
    off = torch.empty((n + 1,), dtype=torch.int64, device="cuda")
    api.fwd_u8_jpeg_scan(px, W, H, seg, work, out, off, lut=lut, chroma=chroma, out_capacity=cap)
    total = int(off[-1].item())
    assert 0 < total <= cap
    return out, off, total


def _engine_round_trip(torch, planes, W, H):
    """planes: [(device uint8 plane, w, h, lut, chroma)] -> decode_jpeg of the engine's file == fwd_u8_i16 / roundtrip_u8, exactly"""
    from simd_dct_amd import jpeg_decode as D
    comps = []
    for px, w, h, lut, chroma in planes:
        out, _, total = gpu_scan(px, w, h, lut, chroma)
        comps.append(dict(blocks_per_row=w // 8, qtable=lut, scan=out[:total].cpu().numpy()))
    data = jfif.write_jpeg(comps, W, H)
    got, coefs = D.decode_jpeg(data, coefficients=True)
    for (px, w, h, lut, _), g, c in zip(planes, got, coefs):
        want_c = torch.empty((h, w), dtype=torch.int16, device="cuda")
        api.fwd_u8_i16(px, want_c, w, h, lut=lut)
        assert torch.equal(c[:h, :w], want_c), (w, h, int((c[:h, :w] != want_c).sum()))
        # no level saturated in the Huffman coder: DC differences within +-2047, AC within +-1023
        assert int(want_c.abs().max()) <= 1023
        want_p = torch.empty((h, w), dtype=torch.uint8, device="cuda")
        api.roundtrip_u8(px, want_p, w, h, lut=lut)
        assert g.shape == (h, w) and torch.equal(g, want_p), (w, h)


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(8192, 8192), (264, 40), (1928, 64), (512, 8)])
def test_engine_grey_scans_round_trip_bit_for_bit(gpu, W, H):
    _engine_round_trip(gpu, [(synth.plane_u8_torch(W, H, "photo", seed=11), W, H, K1, False)], W, H)


@pytest.mark.gpu
def test_engine_420_frame_round_trips_bit_for_bit(gpu):
    torch = gpu
    W, H = 7680, 4320
    ycc = torch.stack([synth.plane_u8_torch(W, H, "photo", seed=s) for s in (21, 22, 23)], dim=-1).contiguous()
    y = torch.empty((H, W), dtype=torch.uint8, device="cuda")
    cb = torch.empty((H // 2, W // 2), dtype=torch.uint8, device="cuda")
    cr = torch.empty_like(cb)
    api.split420_u8_planes(ycc, W, H, y, cb, cr)
    _engine_round_trip(torch, [(y, W, H, K1, False), (cb, W // 2, H // 2, K2, True), (cr, W // 2, H // 2, K2, True)], W, H)


GPU_PILLOW_CASES = PILLOW_CASES + [
    ((130, 70), True, dict(quality=75, subsampling=1, restart_marker_blocks=7)),
    ((200, 120), True, dict(quality=100, subsampling=0, restart_marker_rows=1)),
    ((1000, 37), False, dict(quality=5, restart_marker_blocks=9)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("size,colour,kw", GPU_PILLOW_CASES, ids=[f"{s[0]}x{s[1]}-{'c' if c else 'g'}-{k}" for s, c, k in GPU_PILLOW_CASES])
def test_pillow_files_decode_to_the_checkers_coefficients(gpu, size, colour, kw):
    from simd_dct_amd import jpeg_decode as D
    data = pillow_jpeg(_picture(*size, 8, colour), **kw)
    planes, px = checker_pixels(data)
    got, coefs = D.decode_jpeg(data, coefficients=True)
    info = jfif.read_jpeg(data)
    geo, _ = D.geometry(info)
    for c, p, g, want_px, (w, h, _, _) in zip(coefs, planes, got, px, geo):
        assert np.array_equal(c.cpu().numpy(), p)
        assert np.array_equal(g.cpu().numpy(), want_px[:h, :w])
    W, H = size
    assert np.abs(got[0].cpu().numpy().astype(int) - _libjpeg_luma(data).astype(int)).max() <= 1


@pytest.mark.gpu
def test_pillow_7680x4320_interleaved_420(gpu):
    """the checker is serial Python: it decodes a sample of the intervals; libjpeg anchors the whole luma plane"""
    from simd_dct_amd import jpeg_decode as D
    W, H = 7680, 4320
    data = pillow_jpeg(_picture(W, H, 9, colour=True), quality=75, subsampling=2, restart_marker_rows=1)
    got, coefs = D.decode_jpeg(data, coefficients=True)
    n = H // 16
    sample = [0, 1, n // 2, n - 1]
    planes, st, _ = C.decode(data, intervals={0: sample})
    assert [st[0][k] for k in sample] == [C.OK] * 4
    for c, p, sub in zip(coefs, planes, (2, 1, 1)):
        c = c.cpu().numpy()
        for k in sample:
            rows = slice(k * 8 * sub, (k + 1) * 8 * sub)
            assert np.array_equal(c[rows], p[rows]), k
    assert np.abs(got[0].cpu().numpy().astype(int) - _libjpeg_luma(data).astype(int)).max() <= 1


def _low_level(torch, data, scan_bytes=None, offsets=None, guard=16):
    """index + decode of the file's first scan into planes with guard rows above and below, the scan followed by a guard region.
    Returns (coefficient planes, status, guards intact)."""
    from simd_dct_amd import jpeg_decode as D
    info = jfif.read_jpeg(data)
    sc = info["scans"][0]
    geo, grid = D.geometry(info)
    mcus_x, mcus_y, members = D.scan_geometry(info, sc, geo, grid)
    raw = data[sc["start"]:sc["end"]] if scan_bytes is None else scan_bytes
    buf = torch.full((len(raw) + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    buf[:len(raw)] = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    full = []
    planes = []
    specs = [None] * 4
    for c, (ci, h, v) in zip(sc["components"], members):
        _, _, bx, by = geo[ci]
        f = torch.full((by * 8 + 2 * guard, bx * 8), 0x3C3C, dtype=torch.int16, device="cuda")
        full.append(f)
        planes.append((f[guard:guard + by * 8], bx, by, h, v, c["td"], 2 + c["ta"]))
        specs[c["td"]] = sc["huffman"][(0, c["td"])]
        specs[2 + c["ta"]] = sc["huffman"][(1, c["ta"])]
    tables = D.Tables(specs)
    desc = D.scan_desc(planes, mcus_x, mcus_y, sc["restart_interval"])
    n = D.n_intervals(desc)
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    if offsets is None:
        offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        D.index(buf, n, offsets, status, scan_len=len(raw))
    D.decode(desc, tables, buf, offsets, status, scan_len=len(raw))
    torch.cuda.synchronize()
    intact = bool((buf[len(raw):] == 0xA5).all()) and all(bool((f[:guard] == 0x3C3C).all()) and bool((f[-guard:] == 0x3C3C).all()) for f in full)
    tables.close()
    return [p[0] for p in planes], status.cpu().numpy(), intact


@pytest.mark.gpu
def test_producer_offsets_skip_the_index(gpu):
    torch = gpu
    W, H = 1928, 64
    px = synth.plane_u8_torch(W, H, "photo", seed=31)
    out, off, total = gpu_scan(px, W, H, K1)
    data = jfif.write_jpeg([dict(blocks_per_row=W // 8, qtable=K1, scan=out[:total].cpu().numpy())], W, H)
    a, sa, ia = _low_level(torch, data)
    b, sb, ib = _low_level(torch, data, offsets=off)
    want = torch.empty((H, W), dtype=torch.int16, device="cuda")
    api.fwd_u8_i16(px, want, W, H, lut=K1)
    assert ia and ib and (sa == 0).all() and (sb == 0).all()
    assert torch.equal(a[0], want) and torch.equal(b[0], want)


def _flipped(scan, o, head):
    """interval 1 with one byte changed so that the checker rejects it (a changed byte can still decode: try until one does not)"""
    for pos in range((o[1] + o[2] - 2) // 2, o[2] - 2):
        if scan[pos] in (0xFF, 0x00) or scan[pos - 1] == 0xFF:
            continue
        for mask in (0x5A, 0x81, 0x3C, 0xF0, 0x0F):
            b = bytearray(scan)
            b[pos] ^= mask
            if 0xFF in (b[pos],):
                continue
            _, st, _ = C.decode(head + bytes(b) + b"\xff\xd9")
            if st[0][1] != C.OK:
                return bytes(b)
    raise AssertionError("no single-byte change the checker rejects")


def _malformed_cases(scan, offs, head):
    """(name, bytes) of the malformed variants of a 5-interval scan"""
    o = [int(x) for x in offs]
    flip = _flipped(scan, o, head)
    rst = bytearray(scan)
    assert rst[o[2] - 2] == 0xFF and rst[o[2] - 1] == 0xD1
    rst[o[2] - 1] = 0xD5
    return [("truncated", scan[:(o[3] + o[4]) // 2]), ("flipped", bytes(flip)), ("rst out of sequence", bytes(rst)),
            ("surplus in the middle", scan[:o[2] - 2] + b"\x12\x34\x56" + scan[o[2] - 2:]), ("surplus at the end", scan + b"\x00\x00")]


@pytest.mark.gpu
def test_malformed_scans_report_per_interval_and_stay_in_bounds(gpu):
    torch = gpu
    W, H = 264, 40
    img = _picture(W, H, 41)
    data, (coef,) = engine_file_cpu([(img, K1, False)])
    sc = jfif.read_jpeg(data)["scans"][0]
    scan = data[sc["start"]:sc["end"]]
    _, _, offs = _engine_cpu_scan(img, K1)
    for name, bad in _malformed_cases(scan, offs, data[:sc["start"]]):
        i = data.index(scan)
        file_bad = data[:i] + bad + data[i + len(scan):]
        want_planes, want_st, _ = C.decode(file_bad)
        assert any(s != C.OK for s in want_st[0]), name
        planes, st, intact = _low_level(torch, file_bad, scan_bytes=bad)
        assert intact, name
        assert list(st) == want_st[0], (name, list(st), want_st[0])
        g = planes[0].cpu().numpy()
        for k, s in enumerate(want_st[0]):
            if s == C.OK:  # the intervals the damage did not reach decode exactly
                assert np.array_equal(g[k * 8:k * 8 + 8], want_planes[0][k * 8:k * 8 + 8]), (name, k)
                assert k not in (0, 2) or np.array_equal(g[k * 8:k * 8 + 8], coef[k * 8:k * 8 + 8]) or name.startswith("surplus in"), (name, k)


@pytest.mark.gpu
def test_captured_decode_replays_on_a_second_scan(gpu):
    """encoder scan + decode with the producer's offsets captured once; replayed on another picture of the same geometry"""
    torch = gpu
    from simd_dct_amd import jpeg_decode as D
    W, H = 512, 64
    n = H // 8
    stride = api.huffman_seg_stride(W)
    px = synth.plane_u8_torch(W, H, "photo", seed=51)
    seg = torch.empty((n * stride,), dtype=torch.uint8, device="cuda")
    work = torch.zeros((n + 2,), dtype=torch.int64, device="cuda")
    cap = n * stride * 2
    out = torch.empty((cap,), dtype=torch.uint8, device="cuda")
    off = torch.empty((n + 1,), dtype=torch.int64, device="cuda")
    coef = torch.empty((H, W), dtype=torch.int16, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    tables = D.Tables(_specs())
    desc = D.scan_desc([(coef, W // 8, H // 8, 1, 1, 0, 2)], W // 8, H // 8, W // 8)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        api.fwd_u8_jpeg_scan(px, W, H, seg, work, out, off, lut=K1, out_capacity=cap, stream=s)
        D.decode(desc, tables, out, off, status, scan_len=cap, stream=s)
    for seed in (52, 53):
        px.copy_(synth.plane_u8_torch(W, H, "photo", seed=seed))
        g.replay()
        torch.cuda.synchronize()
        want = torch.empty((H, W), dtype=torch.int16, device="cuda")
        api.fwd_u8_i16(px, want, W, H, lut=K1)
        assert (status.cpu().numpy() == 0).all() and torch.equal(coef, want), seed
    tables.close()


@pytest.mark.gpu
def test_every_kernel_of_the_decoder_runs(gpu):
    from test_kernel_coverage import code_object_kernels
    names, n_objects = code_object_kernels(lib=JPEGDEC_LIB)
    assert n_objects >= 1
    assert names == {"k_decode", "k_rst_scan", "k_rst_walk<false>", "k_rst_walk<true>"}, names
    api.kernel_counts_reset()
    data, _ = engine_file_cpu([(_picture(264, 40, 61), K1, False)])
    from simd_dct_amd import jpeg_decode as D
    D.decode_jpeg(data)
    gpu.cuda.synchronize()
    ran = set(api.kernel_counts())
    assert names <= ran, (sorted(names - ran), sorted(ran))


def test_decoder_code_object_holds_the_four_kernels():
    """CPU half of the coverage check: the kernels in libmdct_jpegdec.so's gfx950 code object (the GPU test launches each of them)"""
    from test_kernel_coverage import code_object_kernels
    assert code_object_kernels(lib=JPEGDEC_LIB)[0] == {"k_decode", "k_rst_scan", "k_rst_walk<false>", "k_rst_walk<true>"}
