"""The GPU decoder of baseline scans without restart markers (libmdct_jpegdec_unmarked.so, include/mdct_jpegdec_unmarked.h,
simd_dct_amd/jpeg_decode.py::decode_unmarked / decode_jpeg) and jfif.read_jpeg(require_restart=False).

CPU: the reader accepts Pillow's default files only when asked to; the independent checker (tests/jpeg_decode_checker.py) decodes a
whole unmarked scan as one interval and agrees with libjpeg; the workspace query refuses marked descriptors; the library's code object
holds exactly its kernel set.
GPU: Pillow files without markers decode to exactly the checker's coefficients (and pixels, and luma within +-1 of libjpeg); the same
picture with and without markers gives identical planes; full-size files against the marked path; malformed scans get the checker's
status and block count, with nothing written outside the planes and the workspace; sync_rounds=0 never gives a wrong OK; a captured
decode replays; every kernel of the library is launched; files mixing marked and unmarked scans."""
import ctypes
import os
import struct

import numpy as np
import pytest

import jpeg_decode_checker as C
import oracle as O
from simd_dct_amd import api, jfif

Image = pytest.importorskip("PIL.Image")
from test_jpeg_decode import _libjpeg_luma, _picture, pillow_jpeg  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNMARKED_LIB = os.path.join(ROOT, "simd_dct_amd", "libmdct_jpegdec_unmarked.so")
KERNELS = {"k_um_zero", "k_um_sync", "k_um_round", "k_um_prefix", "k_um_write", "k_um_final"}
NOT_SYNCHRONISED = 6


# ------------------------------------------------------------------------------------------ the checker on a whole scan
def checker_scan(data, si=0):
    """decode_interval over scan si as ONE interval (no restart markers) -> (status, blocks decoded, planes, qtables).  The unit list is
    built the way the checker's decode() builds it for one interval."""
    data = bytes(data)
    frame, qt, scans = C.parse(data)
    fc = frame["components"]
    hmax, vmax = max(c[1] for c in fc), max(c[2] for c in fc)
    mx, my = -(-frame["width"] // (8 * hmax)), -(-frame["height"] // (8 * vmax))
    planes = [np.zeros((my * c[2] * 8, mx * c[1] * 8), dtype=np.int16) for c in fc]
    comps, _, start, end, huff = scans[si]
    if len(comps) == 1:
        ci = comps[0][0]
        gx = -(-(-(-frame["width"] * fc[ci][1] // hmax)) // 8)
        gy = -(-(-(-frame["height"] * fc[ci][2] // vmax)) // 8)
        layout = [(ci, 0, 0, 1, 1)]
    else:
        gx, gy = mx, my
        layout = [(ci, hh, vv, fc[ci][1], fc[ci][2]) for ci, _, _ in comps for vv in range(fc[ci][2]) for hh in range(fc[ci][1])]
    tabs = {("dc", ci): huff[(0, td)] for ci, td, _ in comps}
    tabs.update({("ac", ci): huff[(1, ta)] for ci, _, ta in comps})
    units = [(ci, ("dc", ci), ("ac", ci), (ci, (m // gx) * V + vv, (m % gx) * H + hh)) for m in range(gx * gy) for ci, hh, vv, H, V in layout]
    status, blocks = C.decode_interval(data[start:end], units, tabs, None)
    for (ci, by, bx), blk in blocks:
        planes[ci][by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = blk.reshape(8, 8).astype(np.int16)
    return status, len(blocks), planes, [np.array(qt[c[3]], dtype=np.float32) for c in fc], blocks


def checker_pixels(planes, qtables):
    return [O.u8_i16("inv", p, p.shape[1], p.shape[0], lut=q) for p, q in zip(planes, qtables)]


# ------------------------------------------------------------------------------------------ CPU
SUBSAMPLINGS = [(False, None), (True, 0), (True, 1), (True, 2)]  # grey, 4:4:4, 4:2:2, 4:2:0


@pytest.mark.parametrize("colour,sub", SUBSAMPLINGS, ids=["grey", "444", "422", "420"])
def test_read_jpeg_accepts_pillows_default_files_on_request(colour, sub):
    kw = dict(quality=75) if sub is None else dict(quality=75, subsampling=sub)
    data = pillow_jpeg(_picture(100, 52, 3, colour), **kw)
    with pytest.raises(jfif.JpegFormatError, match="restart"):
        jfif.read_jpeg(data)  # the default is unchanged
    info = jfif.read_jpeg(data, require_restart=False)
    assert (info["width"], info["height"]) == (100, 52)
    assert len(info["scans"]) == 1 and info["scans"][0]["restart_interval"] == 0
    want = {None: (1, 1), 0: (1, 1), 1: (2, 1), 2: (2, 2)}[sub]
    assert (info["components"][0]["h"], info["components"][0]["v"]) == want
    assert len(info["scans"][0]["components"]) == (3 if colour else 1)
    # the marked file still reads the same way with either setting
    marked = pillow_jpeg(_picture(100, 52, 3, colour), restart_marker_rows=1, **kw)
    a, b = jfif.read_jpeg(marked), jfif.read_jpeg(marked, require_restart=False)
    assert [(s["restart_interval"], s["start"], s["end"]) for s in a["scans"]] == [(s["restart_interval"], s["start"], s["end"]) for s in b["scans"]]
    assert a["scans"][0]["restart_interval"] > 0


CHECKER_CASES = [((61, 37), False, dict(quality=75)), ((100, 52), True, dict(quality=75, subsampling=0)),
                 ((100, 52), True, dict(quality=5, subsampling=1)), ((64, 33), True, dict(quality=100, subsampling=2, optimize=True))]


@pytest.mark.parametrize("size,colour,kw", CHECKER_CASES, ids=[f"{s[0]}x{s[1]}-{'c' if c else 'g'}-{k}" for s, c, k in CHECKER_CASES])
def test_checker_whole_scan_against_libjpeg(size, colour, kw):
    data = pillow_jpeg(_picture(*size, 7, colour), **kw)
    st, n, planes, qts, _ = checker_scan(data)
    assert st == C.OK
    px = checker_pixels(planes, qts)
    W, H = size
    assert np.abs(px[0][:H, :W].astype(int) - _libjpeg_luma(data).astype(int)).max() <= 1


def test_workspace_query_without_device():
    import torch
    from simd_dct_amd import jpeg_decode as D
    t = torch.zeros((56, 104), dtype=torch.int16)
    desc = D.scan_desc([(t, 13, 7, 1, 1, 0, 2)], 13, 7, 0)
    small, big = D.unmarked_workspace(desc, 5000), D.unmarked_workspace(desc, 100_000)
    assert 0 < small < big
    assert big >= 13 * 256 * 24  # 13 chunks of 256 lanes, 24 bytes of state per lane
    assert D.unmarked_workspace(desc, 0) == small  # an empty scan is one chunk
    marked = D.scan_desc([(t, 13, 7, 1, 1, 0, 2)], 13, 7, 13)
    assert D.unmarked_workspace(marked, 5000) == 0 and "restart" in D.unmarked_last_error()
    assert D.unmarked_workspace(D.scan_desc([(t, 13, 7, 1, 1, 0, 2)], 14, 7, 0), 5000) == 0  # the plane is too narrow
    assert D.unmarked_workspace(desc, 1 << 28) == 0
    # the marked path still refuses restart interval 0
    assert D._jpegdec_lib.load().mdct_jpegdec_intervals(ctypes.byref(desc)) == 0


def test_unmarked_code_object_holds_its_kernels():
    from test_kernel_coverage import code_object_kernels
    names, n_objects = code_object_kernels(lib=UNMARKED_LIB)
    assert n_objects >= 1 and names == KERNELS, names


# ------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    torch.cuda.set_device(0)
    api.init(0)
    return torch


GPU_CASES = [  # (size, colour, save options): no restart markers anywhere
    ((72, 40), False, dict(quality=75)),
    ((100, 52), True, dict(quality=75, subsampling=0)),
    ((100, 52), True, dict(quality=75, subsampling=1)),
    ((100, 52), True, dict(quality=75, subsampling=2, optimize=True)),
    ((61, 37), True, dict(quality=5, subsampling=2)),
    ((61, 37), False, dict(quality=100, optimize=True)),
    ((1000, 37), False, dict(quality=100)),       # several chunks
    ((400, 300), True, dict(quality=100, subsampling=1)),  # several chunks, interleaved
    ((8, 8), False, dict(quality=75)),            # a single block
    ((8, 8), True, dict(quality=75, subsampling=2)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("size,colour,kw", GPU_CASES, ids=[f"{s[0]}x{s[1]}-{'c' if c else 'g'}-{k}" for s, c, k in GPU_CASES])
def test_pillow_files_without_markers_decode_to_the_checkers_coefficients(gpu, size, colour, kw):
    from simd_dct_amd import jpeg_decode as D
    data = pillow_jpeg(_picture(*size, 8, colour), **kw)
    st, _, planes, qts, _ = checker_scan(data)
    assert st == C.OK
    px = checker_pixels(planes, qts)
    got, coefs = D.decode_jpeg(data, coefficients=True)
    geo, _ = D.geometry(jfif.read_jpeg(data, require_restart=False))
    for c, p, g, want_px, (w, h, _, _) in zip(coefs, planes, got, px, geo):
        assert np.array_equal(c.cpu().numpy(), p)
        assert np.array_equal(g.cpu().numpy(), want_px[:h, :w])
    assert np.abs(got[0].cpu().numpy().astype(int) - _libjpeg_luma(data).astype(int)).max() <= 1


@pytest.mark.gpu
@pytest.mark.parametrize("colour,sub", SUBSAMPLINGS, ids=["grey", "444", "422", "420"])
def test_same_picture_with_and_without_markers(gpu, colour, sub):
    from simd_dct_amd import jpeg_decode as D
    img = _picture(1000, 200, 12, colour)
    kw = dict(quality=90) if sub is None else dict(quality=90, subsampling=sub)
    _, a = D.decode_jpeg(pillow_jpeg(img, **kw), coefficients=True)
    _, b = D.decode_jpeg(pillow_jpeg(img, restart_marker_rows=1, **kw), coefficients=True)
    for x, y in zip(a, b):
        assert gpu.equal(x, y)


def _full_size(torch, W, H, colour, sub, seed, rows_per_interval):
    from simd_dct_amd import jpeg_decode as D
    img = _picture(W, H, seed, colour)
    kw = dict(quality=75) if sub is None else dict(quality=75, subsampling=sub)
    plain, marked = pillow_jpeg(img, **kw), pillow_jpeg(img, restart_marker_rows=1, **kw)
    _, a = D.decode_jpeg(plain, coefficients=True)
    _, b = D.decode_jpeg(marked, coefficients=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # the checker is serial Python: sampled MCU rows (restart intervals of the marked file) against the unmarked decode
    n = -(-H // (8 * rows_per_interval))  # restart intervals of the marked file: one MCU row each
    sample = [0, 1, n // 2, n - 1]
    planes, st, _ = C.decode(marked, intervals={0: sample})
    assert [st[0][k] for k in sample] == [C.OK] * 4
    for c, p, v in zip(a, planes, (rows_per_interval,) + (1, 1)):
        c = c.cpu().numpy()
        for k in sample:
            rows = slice(k * 8 * v, (k + 1) * 8 * v)
            assert np.array_equal(c[rows], p[rows]), k


@pytest.mark.gpu
def test_full_size_grey_8192(gpu):
    _full_size(gpu, 8192, 8192, False, None, 13, 1)


@pytest.mark.gpu
def test_full_size_pillow_7680x4320_interleaved_420(gpu):
    _full_size(gpu, 7680, 4320, True, 2, 9, 2)


def _low_level(torch, data, scan_bytes=None, sync_rounds=4, guard=16):
    """decode_unmarked of the file's first scan into planes with guard rows, the scan and the workspace followed by guard regions.
    Returns (coefficient planes, status [code, blocks], guards intact, workspace)."""
    from simd_dct_amd import jpeg_decode as D
    info = jfif.read_jpeg(data, require_restart=False)
    sc = info["scans"][0]
    geo, grid = D.geometry(info)
    mcus_x, mcus_y, members = D.scan_geometry(info, sc, geo, grid)
    raw = data[sc["start"]:sc["end"]] if scan_bytes is None else scan_bytes
    buf = torch.full((len(raw) + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    if raw:
        buf[:len(raw)] = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    full, planes, specs = [], [], [None] * 4
    for c, (ci, h, v) in zip(sc["components"], members):
        _, _, bx, by = geo[ci]
        f = torch.full((by * 8 + 2 * guard, bx * 8), 0x3C3C, dtype=torch.int16, device="cuda")
        full.append(f)
        planes.append((f[guard:guard + by * 8], bx, by, h, v, c["td"], 2 + c["ta"]))
        specs[c["td"]] = sc["huffman"][(0, c["td"])]
        specs[2 + c["ta"]] = sc["huffman"][(1, c["ta"])]
    tables = D.Tables(specs)
    desc = D.scan_desc(planes, mcus_x, mcus_y, 0)
    nbytes = D.unmarked_workspace(desc, len(raw))
    assert nbytes > 0, D.unmarked_last_error()
    wfull = torch.full((nbytes + 4096,), 0x5A, dtype=torch.uint8, device="cuda")
    status = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    D.decode_unmarked(desc, tables, buf, wfull[:nbytes], status, scan_len=len(raw), sync_rounds=sync_rounds)
    torch.cuda.synchronize()
    intact = (bool((buf[len(raw):] == 0xA5).all()) and bool((wfull[nbytes:] == 0x5A).all())
              and all(bool((f[:guard] == 0x3C3C).all()) and bool((f[-guard:] == 0x3C3C).all()) for f in full))
    tables.close()
    return [p[0] for p in planes], [int(x) for x in status.cpu().numpy()], intact, wfull[:nbytes]


def _blocks_match(planes, blocks):
    g = [p.cpu().numpy() for p in planes]
    return all(np.array_equal(g[ci][by * 8:by * 8 + 8, bx * 8:bx * 8 + 8], blk.reshape(8, 8)) for (ci, by, bx), blk in blocks)


def _changed_byte(data, scan):
    """one byte of the scan changed so that the checker rejects the file"""
    i = data.index(scan)
    for pos in range(len(scan) // 2, len(scan) - 2):
        if scan[pos] in (0xFF, 0x00) or scan[pos - 1] == 0xFF:
            continue
        for mask in (0x5A, 0x81, 0x3C):
            b = bytearray(scan)
            b[pos] ^= mask
            if b[pos] == 0xFF:
                continue
            if checker_scan(data[:i] + bytes(b) + data[i + len(scan):])[0] != C.OK:
                return bytes(b)
    raise AssertionError("no single-byte change the checker rejects")


def _with_rst(scan, at):
    while scan[at - 1] == 0xFF or scan[at] == 0x00:
        at += 1
    return scan[:at] + b"\xff\xd3" + scan[at:]


@pytest.mark.gpu
@pytest.mark.parametrize("size,colour", [((264, 40), False), ((1000, 120), True)], ids=["one-chunk", "multi-chunk"])
def test_malformed_scans(gpu, size, colour):
    torch = gpu
    data = pillow_jpeg(_picture(*size, 41, colour), quality=95)
    sc = jfif.read_jpeg(data, require_restart=False)["scans"][0]
    scan = data[sc["start"]:sc["end"]]
    cases = [("truncated", scan[:len(scan) // 2]), ("ends mid-block", scan[:-3]), ("one byte changed", _changed_byte(data, scan)),
             ("rst inserted", _with_rst(scan, len(scan) // 3)), ("surplus after the last MCU", scan + b"\x12\x34\x56"),
             ("empty", b"")]
    i = data.index(scan)
    for name, bad in cases:
        file_bad = data[:i] + bad + data[i + len(scan):]
        want_st, want_n, _, _, blocks = checker_scan(file_bad)
        assert want_st != C.OK, name
        planes, st, intact, _ = _low_level(torch, file_bad, scan_bytes=bad, sync_rounds=len(bad) // 8192 + 1)
        assert intact, name
        assert st == [want_st, want_n], (name, st, want_st, want_n)
        assert _blocks_match(planes, blocks), name


@pytest.mark.gpu
def test_zero_sync_rounds_never_gives_a_wrong_ok(gpu):
    torch = gpu
    from simd_dct_amd import jpeg_decode as D
    for seed, q in ((61, 100), (62, 75), (63, 40)):
        data = pillow_jpeg(_picture(1200, 160, seed, True), quality=q, subsampling=2)
        sc = jfif.read_jpeg(data, require_restart=False)["scans"][0]
        assert sc["end"] - sc["start"] > 2 * 8192  # several chunks
        want_st, want_n, want_planes, _, _ = checker_scan(data)
        assert want_st == C.OK
        planes, st, intact, work = _low_level(torch, data, sync_rounds=0)
        assert intact and st[0] in (C.OK, NOT_SYNCHRONISED), st
        if st[0] == C.OK:
            assert st[1] == want_n and all(np.array_equal(p.cpu().numpy(), w) for p, w in zip(planes, want_planes))
        planes, st, intact, work = _low_level(torch, data, sync_rounds=4)
        assert intact and st == [C.OK, want_n]
        assert int(work[:4].view(torch.int32)[0]) <= 4  # the last round that changed a chunk's exit
        assert all(np.array_equal(p.cpu().numpy(), w) for p, w in zip(planes, want_planes))
        # decode_jpeg retries a NOT_SYNCHRONISED result; its planes are right whatever the first call returned
        _, coefs = D.decode_jpeg(data, coefficients=True)
        assert all(np.array_equal(c.cpu().numpy(), w) for c, w in zip(coefs, want_planes))


@pytest.mark.gpu
def test_captured_decode_replays(gpu):
    """one decode captured; replayed on garbage planes, on a corrupted copy in the same buffer, and on the original again"""
    torch = gpu
    from simd_dct_amd import jpeg_decode as D
    data = pillow_jpeg(_picture(1000, 120, 71, True), quality=95, subsampling=2)
    sc = jfif.read_jpeg(data, require_restart=False)["scans"][0]
    scan = data[sc["start"]:sc["end"]]
    want_st, want_n, want_planes, _, _ = checker_scan(data)
    bad = _changed_byte(data, scan)
    i = data.index(scan)
    bad_st, bad_n, _, _, bad_blocks = checker_scan(data[:i] + bad + data[i + len(scan):])
    info = jfif.read_jpeg(data, require_restart=False)
    geo, grid = D.geometry(info)
    mcus_x, mcus_y, members = D.scan_geometry(info, sc, geo, grid)
    coefs = [torch.empty((by * 8, bx * 8), dtype=torch.int16, device="cuda") for _, _, bx, by in geo]
    specs = [None] * 4
    planes = []
    for c, (ci, h, v) in zip(sc["components"], members):
        specs[c["td"]] = sc["huffman"][(0, c["td"])]
        specs[2 + c["ta"]] = sc["huffman"][(1, c["ta"])]
        planes.append((coefs[ci], geo[ci][2], geo[ci][3], h, v, c["td"], 2 + c["ta"]))
    tables = D.Tables(specs)
    desc = D.scan_desc(planes, mcus_x, mcus_y, 0)
    buf = torch.frombuffer(bytearray(scan), dtype=torch.uint8).cuda()
    work = torch.empty(D.unmarked_workspace(desc, len(scan)), dtype=torch.uint8, device="cuda")
    status = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        D.decode_unmarked(desc, tables, buf, work, status, stream=s)
    for name, src in (("garbage planes", scan), ("corrupted", bad), ("original", scan)):
        for cf in coefs:
            cf.fill_(0x7777)
        work.fill_(0x99)
        status.fill_(-1)
        buf.copy_(torch.frombuffer(bytearray(src), dtype=torch.uint8).cuda())
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        st = [int(x) for x in status.cpu().numpy()]
        if src is bad:
            assert st == [bad_st, bad_n], (name, st)
            assert _blocks_match(coefs, bad_blocks), name
        else:
            assert st == [want_st, want_n], (name, st)
            assert all(np.array_equal(c.cpu().numpy(), w) for c, w in zip(coefs, want_planes)), name
    tables.close()


@pytest.mark.gpu
def test_every_kernel_of_the_unmarked_decoder_runs(gpu):
    from simd_dct_amd import jpeg_decode as D
    from test_kernel_coverage import code_object_kernels
    names, _ = code_object_kernels(lib=UNMARKED_LIB)
    api.kernel_counts_reset()
    D.decode_jpeg(pillow_jpeg(_picture(1000, 120, 81, True), quality=95))  # several chunks: the fix rounds are launched
    gpu.cuda.synchronize()
    ran = set(api.kernel_counts())
    assert names <= ran, (sorted(names - ran), sorted(ran))


def _sos_scan(data):
    """(SOS segment, entropy-coded bytes) of a single-scan file"""
    info = jfif.read_jpeg(data, require_restart=False)
    sc = info["scans"][0]
    j = data.rindex(b"\xff\xda", 0, sc["start"])
    return data[j:sc["start"]], data[sc["start"]:sc["end"]]


def _segments(data, marker):
    """every marker segment of that kind before the first SOS, joined"""
    out, j = [], 2
    while data[j + 1] != 0xDA:
        n = 2 + struct.unpack_from(">H", data, j + 2)[0]
        if data[j + 1] == marker:
            out.append(data[j:j + n])
        j += n
    return b"".join(out)


@pytest.mark.gpu
def test_file_mixing_marked_and_unmarked_scans(gpu):
    """a 4:2:0 frame of three non-interleaved scans, built from Pillow grey files: Y without markers, Cb with, Cr without"""
    from simd_dct_amd import jpeg_decode as D
    W, H = 333, 150
    y, cb, cr = (_picture(w, h, 90 + k) for k, (w, h) in enumerate(((W, H), (-(-W // 2), -(-H // 2)), (-(-W // 2), -(-H // 2)))))
    fy, fcb, fcr = pillow_jpeg(y, quality=80), pillow_jpeg(cb, quality=80, restart_marker_rows=1), pillow_jpeg(cr, quality=80)
    parts = [b"\xff\xd8", _segments(fy, 0xDB), jfif._seg(0xC0, struct.pack(">BHHB", 8, H, W, 3) + bytes([1, 0x22, 0, 2, 0x11, 0, 3, 0x11, 0])),
             _segments(fy, 0xC4)]
    for cid, f, dri in ((1, fy, 0), (2, fcb, -(-cb.shape[1] // 8)), (3, fcr, 0)):
        sos, scan = _sos_scan(f)
        parts += [jfif._seg(0xDD, struct.pack(">H", dri)), sos[:5] + bytes([cid]) + sos[6:], scan]
    data = b"".join(parts) + b"\xff\xd9"
    info = jfif.read_jpeg(data, require_restart=False)
    assert [s["restart_interval"] for s in info["scans"]] == [0, -(-cb.shape[1] // 8), 0]
    got, coefs = D.decode_jpeg(data, coefficients=True)
    want = [checker_scan(fy)[2][0], C.decode(fcb)[0][0], checker_scan(fcr)[2][0]]
    for c, w in zip(coefs, want):
        c = c.cpu().numpy()
        assert np.array_equal(c[:w.shape[0], :w.shape[1]], w)
    for g, img, f in zip(got, (y, cb, cr), (fy, fcb, fcr)):
        assert g.shape == img.shape
        assert np.abs(g.cpu().numpy().astype(int) - _libjpeg_luma(f).astype(int)).max() <= 1
