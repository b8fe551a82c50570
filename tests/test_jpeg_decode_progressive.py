"""Progressive JPEG input with spectral selection: jfif.sof_marker / read_progressive_jpeg, libmdct_jpegdec_prog.so
(include/mdct_jpegdec_prog.h), and decode_coefficients / decode_jpeg / transcode_jpeg on SOF2 files.

Truth comes from the test side.  Good scans are coded from known coefficients by jpeg_progressive_encoder (or, symbol by symbol, by
hand) and must come back as those coefficients; jpeg_progressive_status states plane contents and per-interval statuses for good and
bad scans alike; jpeg_progressive_checker and Pillow read whole files.  Every comparison is exact.

CPU: the reader against the checker's parser; sof_marker; one row per refusal site of the reader; the C-ABI's refusals; the status
helper against the checker; the code object.
GPU: scans of every shape into sentinel-filled planes inside canaries (seams of 256 lanes, restart intervals, interval sizes, end-of-band
runs, levels and zero runs, stuffing); failing intervals of every class; whole files through decode_coefficients, decode_jpeg and
transcode_jpeg; a captured graph; launch counts."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

import jpeg_decode_checker as DC
import jpeg_progressive_approx_checker as XC
import jpeg_progressive_checker as PC
import jpeg_progressive_encoder as PE
import jpeg_progressive_status as PS
import jpeg_scan_encoder as E
from simd_dct_amd import _jpegdec_lib, _jpegdec_prog_lib, api, jfif
from test_jpeg_progressive import CUSTOM, FRAMES, LONG_AC, S420, S422, S444, SCAN3, as_written, make_planes, sparse, zz_block

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG_DEC_LIB = os.path.join(ROOT, "simd_dct_amd", "libmdct_jpegdec_prog.so")
KERNELS = {"k_decode_prog_dc", "k_decode_prog_ac"}
DC0, DC1 = E.ANNEX_K[(0, 0)], E.ANNEX_K[(0, 1)]
ZRL = (0xF0, 0, 0)


def encoder_files():
    for name, frame in FRAMES.items():
        nc = len(frame["comps"])
        for inter in (True, False):
            for bands in (None, CUSTOM[nc]):
                planes = make_planes(frame, 7, inter)
                data, info = PE.encode_file(frame, planes, bands=bands, interleaved_dc=inter)
                yield (name, inter, bands is not None), data, info, planes


# ------------------------------------------------------------------------------------------ CPU: the reader
def _same_as_the_checker(data):
    got = jfif.read_progressive_jpeg(data)
    frame, qt, scans, _ = PC.parse(data)
    assert got["sof"] == 0xC2 and (got["width"], got["height"]) == (frame["width"], frame["height"])
    assert [(c["id"], c["h"], c["v"], c["tq"]) for c in got["components"]] == frame["components"]
    assert len(got["scans"]) == len(scans)
    for g, s in zip(got["scans"], scans):
        assert (g["ss"], g["se"], g["ah"], g["al"], g["restart_interval"]) == (s["ss"], s["se"], 0, 0, s["dri"])
        assert [(c["index"], c["td"], c["ta"]) for c in g["components"]] == s["comps"]
        assert (g["start"], g["end"]) == (s["start"], s["end"])
        assert {k: DC.code_table(*v) for k, v in g["huffman"].items()} == s["huffman"], "the tables in force at the scan"
    for tq, q in qt.items():
        assert got["qtables"][tq].tolist() == q
    return got


def test_reader_round_trip_on_the_encoders_files():
    for key, data, info, _ in encoder_files():
        got = _same_as_the_checker(data)
        assert [(s["ss"], s["se"], [c["index"] for c in s["components"]]) for s in got["scans"]] == [(s["ss"], s["se"], s["comps"]) for s in info], key


def _engine_style_file():
    body = lambda k, n: bytes((i * k + 7) % 251 for i in range(n))  # noqa: E731
    qa, qb = [1 + (i * 3) % 200 for i in range(64)], [255 - i for i in range(64)]
    scans = [dict(components=SCAN3, ss=0, se=0, restart_interval=3, tables={(0, 0): DC0, (0, 1): DC1}, scan=body(3, 40)),
             dict(components=[(0, 0, 0)], ss=1, se=5, restart_interval=6, tables={(1, 0): LONG_AC}, scan=body(5, 50)),
             dict(components=[(0, 0, 0)], ss=6, se=63, restart_interval=6, tables={(1, 0): LONG_AC}, scan=body(7, 60)),
             dict(components=[(1, 1, 1)], ss=1, se=63, restart_interval=3, tables={(1, 1): E.ANNEX_K[(1, 1)]}, scan=body(11, 30)),
             dict(components=[(2, 1, 1)], ss=1, se=63, restart_interval=3, tables={(1, 1): LONG_AC}, scan=body(13, 31))]
    return jfif.write_progressive_jpeg([qa, qb, qb], 40, 24, S420, scans), scans


def test_reader_round_trip_on_write_progressive_jpeg():
    data, scans = _engine_style_file()
    got = _same_as_the_checker(data)
    for g, s in zip(got["scans"], scans):
        assert data[g["start"]:g["end"]] == s["scan"]
    # a table id redefined between two scans: each scan sees its own
    assert got["scans"][3]["huffman"][(1, 1)][1] == list(E.ANNEX_K[(1, 1)][1])
    assert got["scans"][4]["huffman"][(1, 1)][1] == list(LONG_AC[1])
    assert got["colorspace"] == "YCbCr"


def _baseline_file():
    frame = FRAMES["4:2:0"]
    return E.encode_file(frame, [dict(comps=SCAN3, dri=4)], make_planes(frame, 3, True), E.ANNEX_K)[0]


def test_sof_marker():
    prog = next(encoder_files())[1]
    base = _baseline_file()
    assert jfif.sof_marker(base) == 0xC0 and jfif.sof_marker(prog) == 0xC2
    assert jfif.sof_marker(bytearray(prog)) == 0xC2 and jfif.sof_marker(memoryview(prog)) == 0xC2 and jfif.sof_marker(np.frombuffer(prog, dtype=np.uint8)) == 0xC2
    for empty in (b"", b"\xff", b"\xff\xd8", b"\xff\xd8\xff\xd9", b"not a jpeg at all", b"\x00" * 64):
        assert jfif.sof_marker(empty) is None
    sof_end = prog.index(b"\xff\xc2") + 2 + prog[prog.index(b"\xff\xc2") + 3]  # marker, then a length below 256
    for n in range(len(prog)):  # truncated anywhere: never an exception; the marker once its segment is whole
        assert jfif.sof_marker(prog[:n]) == (0xC2 if n >= sof_end else None), n
    assert jfif.sof_marker(prog.replace(b"\xff\xc2", b"\xff\xc9", 1)) == 0xC9
    # a segment length that points past the end of the file
    cut = bytearray(prog)
    cut[4:6] = b"\xff\xff"
    assert jfif.sof_marker(bytes(cut)) is None


def _sos(data, k, ss=None, se=None, a=None, **_):
    """the file with the band bytes of its k-th SOS replaced"""
    st = PC.parse(data)[2][k]["start"]
    old = data[st - 3:st]
    new = bytes([old[0] if ss is None else ss, old[1] if se is None else se, old[2] if a is None else a])
    return data[:st - 3] + new + data[st:]


def _group(data, k):
    """byte range of scan k with the DHT, DRI and SOS in front of it"""
    scans = PC.parse(data)[2]
    return (scans[k - 1]["end"] if k else data.index(b"\xff\xc4")), scans[k]["end"]


def _grey():
    frame = FRAMES["grey"]
    return PE.encode_file(frame, make_planes(frame, 5, False))[0]


def _colour():
    frame = FRAMES["4:4:4"]
    return PE.encode_file(frame, make_planes(frame, 5, True), interleaved_dc=True)[0]


def _pillow_progressive():
    Image = pytest.importorskip("PIL.Image")
    y, x = np.mgrid[0:32, 0:48]
    img = np.clip(128 + 90 * np.sin(x / 5.0) * np.cos(y / 3.0), 0, 255).astype(np.uint8)
    f = io.BytesIO()
    Image.fromarray(img).save(f, "JPEG", progressive=True, restart_marker_rows=1)
    return f.getvalue()


def _twice(data, k):
    a, b = _group(data, k)
    return data[:b] + data[a:b] + data[b:]


def _without(data, k):
    a, b = _group(data, k)
    return data[:a] + data[b:]


def _p12(data):
    i = data.index(b"\xff\xc2")
    return data[:i + 4] + b"\x0c" + data[i + 5:]


# (what, the file, text of the message): one row per `raise JpegFormatError` of the reader of progressive files, and rows for what it
# leaves to read_jpeg's rules
PROG_REFUSALS = [
    ("a baseline file", _baseline_file, "not a progressive file"),
    ("Pillow's progressive file", _pillow_progressive, "successive approximation"),
    ("Al = 1 in the DC scan", lambda: _sos(_grey(), 0, a=0x01), "successive approximation"),
    ("Ah = 1 in an AC scan", lambda: _sos(_grey(), 1, a=0x10), "successive approximation"),
    ("the DRI segments removed", lambda: re.sub(rb"\xff\xdd\x00\x04..", b"", _grey(), flags=re.S), "without restart markers"),
    ("the last DRI set to 0", lambda: (lambda d, i: d[:i + 4] + b"\x00\x00" + d[i + 6:])(_grey(), _grey().rindex(b"\xff\xdd\x00\x04")), "without restart markers"),
    ("an interleaved AC scan", lambda: _sos(_colour(), 0, ss=1, se=5), "interleaved AC scan"),
    ("a band 0..5", lambda: _sos(_grey(), 0, se=5), "malformed SOS: band 0..5"),
    ("a band 7..3", lambda: _sos(_grey(), 1, ss=7, se=3), "malformed SOS: band 7..3"),
    ("a band 10..64", lambda: _sos(_grey(), 3, se=64), "malformed SOS: band 10..64"),
    ("a band coded twice", lambda: _twice(_grey(), 2), "coded a second time"),
    ("the DC scan coded twice", lambda: _twice(_grey(), 0), "coded a second time"),
    ("overlapping bands", lambda: _sos(_grey(), 2, ss=2), "coded a second time"),
    ("AC before DC", lambda: _without(_grey(), 0), "before its DC scan"),
    ("AC of Cb before its DC scan", lambda: _without(PE.encode_file(FRAMES["4:4:4"], make_planes(FRAMES["4:4:4"], 5, False), interleaved_dc=False)[0], 1), "before its DC scan"),
    ("12-bit samples", lambda: _p12(_grey()), "12-bit samples"),
    ("no frame", lambda: b"\xff\xd8\xff\xd9", "no frame or no scan"),
    ("no SOI", lambda: b"JFIF", "no SOI"),
    ("a truncated file", lambda: _grey()[:-40], "no EOI"),
    ("a second frame header", lambda: (lambda d, i: d[:i] + d[i:i + 2 + d[i + 3]] + d[i:])(_grey(), _grey().index(b"\xff\xc2")), "second frame header"),
    ("a malformed SOS", lambda: (lambda d, st: d[:st - 6] + b"\x02" + d[st - 5:])(_grey(), PC.parse(_grey())[2][0]["start"]), "malformed SOS"),
]


@pytest.mark.parametrize("what,make,text", PROG_REFUSALS, ids=[r[0] for r in PROG_REFUSALS])
def test_reader_refusals(what, make, text):
    data = make()
    with pytest.raises(jfif.JpegFormatError) as e:
        jfif.read_progressive_jpeg(data)
    assert text in str(e.value), str(e.value)
    if what != "a baseline file":
        with pytest.raises(jfif.JpegFormatError):  # read_jpeg refuses them as ever
            jfif.read_jpeg(data, require_restart=False)


def test_every_refusal_site_of_the_progressive_reader_has_a_row():
    """the completeness check of test_jpeg_decode_hostile on the new region of jfif.py (everything after _colorspace)"""
    src = open(jfif.__file__).read()
    src = src[src.index("def _colorspace"):]
    sites = re.findall(r'raise JpegFormatError\(f?"([^"]*)"', src)
    assert len(sites) >= 7 and len(re.findall(r"raise JpegFormatError", src)) == len(sites), sites
    raised = []
    for what, make, _ in PROG_REFUSALS:
        if what == "Pillow's progressive file":
            continue
        with pytest.raises(jfif.JpegFormatError) as e:
            jfif.read_progressive_jpeg(make())
        raised.append(str(e.value))
    for site in sites:
        texts = [t.strip() for t in re.split(r"\{[^}]*\}", site) if len(t.strip()) > 3]
        assert texts and any(all(t in msg for t in texts) for msg in raised), site


def test_a_band_no_scan_codes_is_legal():
    data = _grey()
    info = jfif.read_progressive_jpeg(_without(data, 2))
    assert [(s["ss"], s["se"]) for s in info["scans"]] == [(0, 0), (1, 2), (10, 63)]


# ------------------------------------------------------------------------------------------ CPU: the C-ABI
def _desc(comps, mx, my, ri):
    """comps: [(address, pitch, blocks_x, blocks_y, h, v, dc_slot, ac_slot)]"""
    d = _jpegdec_lib.Scan()
    d.n_components = len(comps)
    for c, row in enumerate(comps):
        d.comp[c] = _jpegdec_lib.Component(*row)
    d.mcus_x, d.mcus_y, d.restart_interval = mx, my, ri
    return d


def test_cabi_refusals_without_device():
    lib = _jpegdec_prog_lib.load()
    A = 0x10000  # never dereferenced: every call below is refused on the host, or is a host function
    one = lambda **k: (A, k.get("pitch", 64), 8, 4, k.get("h", 1), k.get("v", 1), k.get("dc", 0), k.get("ac", 2))  # noqa: E731
    y420 = (A, 128, 16, 8, 2, 2, 0, 2)

    def n(d, ss, se):
        return int(lib.mdct_jpegdec_prog_intervals(ctypes.byref(d) if d is not None else None, ss, se))

    def refused(d, ss, se, text, rc=1):
        assert n(d, ss, se) == 0
        assert text in lib.mdct_jpegdec_prog_last_error().decode(), lib.mdct_jpegdec_prog_last_error().decode()
        assert lib.mdct_jpegdec_prog_decode(ctypes.byref(d) if d is not None else None, ss, se, None, None, 0, None, None, None) == rc

    good = _desc([one()], 8, 4, 8)
    assert n(good, 0, 0) == 4 and n(good, 1, 63) == 4 and n(good, 5, 5) == 4 and n(good, 63, 63) == 4
    assert n(_desc([one()], 5, 3, 4), 1, 5) == 4 and n(_desc([one()], 8, 4, 1), 0, 0) == 32 and n(_desc([one()], 8, 4, 1000), 6, 63) == 1
    colour = _desc([y420, one(dc=1), one(dc=1)], 8, 4, 8)
    assert n(colour, 0, 0) == 4
    # the slot class the band does not use is ignored
    assert n(_desc([one(ac=-5)], 8, 4, 8), 0, 0) == 4 and n(_desc([one(dc=77)], 8, 4, 8), 1, 63) == 4
    # a legal descriptor, no tables
    assert lib.mdct_jpegdec_prog_decode(ctypes.byref(good), 0, 0, None, None, 0, None, None, None) == 1
    assert "null tables" in lib.mdct_jpegdec_prog_last_error().decode()
    refused(None, 0, 0, "null scan descriptor")
    for ss, se in ((0, 5), (7, 3), (1, 64), (63, 64), (-1, 0), (0, -1), (64, 64)):
        refused(good, ss, se, "band")
    refused(colour, 1, 63, "one component")
    refused(_desc([one(), one()], 8, 4, 8), 1, 5, "one component")
    refused(_desc([one(h=2)], 4, 4, 8), 1, 5, "h = v = 1")
    refused(_desc([one(h=2)], 4, 4, 8), 0, 0, "non-interleaved")
    refused(_desc([one()], 8, 4, 0), 0, 0, "restart interval 0")
    refused(_desc([one()], 8, 4, 0), 1, 63, "restart interval 0")
    refused(_desc([one()], 0, 4, 8), 0, 0, "empty MCU grid")
    refused(_desc([(A + 2,) + one()[1:]], 8, 4, 8), 0, 0, "unaligned")
    refused(_desc([(0,) + one()[1:]], 8, 4, 8), 1, 63, "null or unaligned")
    refused(_desc([one(pitch=68)], 8, 4, 8), 1, 63, "unaligned")
    refused(_desc([one(pitch=56)], 8, 4, 8), 0, 0, "needs")
    refused(_desc([one()], 9, 4, 8), 0, 0, "needs")
    # a slot that cannot hold a table of the band's class (whether a legal slot is empty shows with a table handle: GPU test below)
    refused(_desc([one(dc=-1)], 8, 4, 8), 0, 0, "table slots")
    refused(_desc([one(dc=2)], 8, 4, 8), 0, 0, "table slots")
    refused(_desc([one(ac=1)], 8, 4, 8), 1, 63, "table slots")
    refused(_desc([one(ac=4)], 8, 4, 8), 1, 63, "table slots")
    refused(_desc([], 8, 4, 8), 0, 0, "components")
    # 2^31 blocks
    big = _desc([(A, 1 << 20, 1 << 17, 1 << 14, 1, 1, 0, 2)], 1 << 17, 1 << 14, 8)
    refused(big, 0, 0, "2^31", rc=2)  # MDCT_NOT_SUPPORTED, as mdct_jpegdec_decode answers it


# ------------------------------------------------------------------------------------------ CPU: the status helper
def test_status_helper_equals_the_checker_on_the_encoders_files():
    for key, data, info, planes in encoder_files():
        got, statuses = PS.decode(data)
        want, _ = PC.decode(data)
        assert len(statuses) == len(info) and all(s == [0] * len(s) for s in statuses), key
        for g, w, p in zip(got, want, planes):
            assert np.array_equal(g, w) and np.array_equal(g, p), key


def tokens(items, spec):
    """(symbol, extra, n extra bits) tuples and strings of raw bits -> one interval's unstuffed bytes, padded with 1-bits"""
    codes, w = E.canonical_codes(*spec), E._Writer()
    for t in items:
        if isinstance(t, str):
            for ch in t:
                w.put(int(ch), 1)
        else:
            w.put(*codes[t[0]])
            w.put(t[1], t[2])
    return w.finish()[0]


def level(r, v):
    s = abs(v).bit_length()
    return ((r << 4) | s, v if v > 0 else v + (1 << s) - 1, s)


def eob(run=1):
    n = run.bit_length() - 1
    return (n << 4, run - (1 << n), n)


def test_status_helper_the_documented_exception_and_the_error_classes():
    """a ZRL that ends exactly at se + 1 ends its block here (and in the GPU decoder), where the checker refuses the stream"""
    tab = DC.code_table(*LONG_AC)

    def run(items, ss, se, n_blocks, raw=None):
        p = [np.zeros((8, 8 * n_blocks), dtype=np.int16)]
        data = PE.scan_data([tokens(items, LONG_AC)]) if raw is None else raw
        st = PS.decode_scan(data, ss, se, tab, PS.block_order(n_blocks, 1, [(0, 0, 0, 1, 1)]), n_blocks, p)
        return st, p[0]

    st, p = run([level(0, 3), ZRL, level(0, -2), eob()], 1, 17, 2)  # 3 at 1, ZRL to 18 = se + 1: block ends; -2 at 1, EOB
    assert st == [0] and p[0, 1] == 3 and p[0, 9] == -2 and np.count_nonzero(p) == 2
    frame = dict(width=16, height=8, comps=[(1, 1)])
    dcs = PE.dc_scan(frame, [(0, 0)], [np.zeros((8, 16), dtype=np.int16)], {0: DC0})[0]
    f = jfif.write_progressive_jpeg([[1] * 64], 16, 8, [(1, 1)], [
        dict(components=[(0, 0, 0)], ss=0, se=0, restart_interval=2, tables={(0, 0): DC0}, scan=PE.scan_data(dcs)),
        dict(components=[(0, 0, 0)], ss=1, se=17, restart_interval=2, tables={(1, 0): LONG_AC}, scan=PE.scan_data([tokens([level(0, 3), ZRL, level(0, -2), eob()], LONG_AC)])),
        dict(components=[(0, 0, 0)], ss=18, se=63, restart_interval=2, tables={(1, 0): LONG_AC}, scan=PE.scan_data([tokens([eob(2)], LONG_AC)]))])
    with pytest.raises(ValueError, match="ZRL"):
        PC.decode(f)
    got, statuses = PS.decode(f)
    assert statuses == [[0], [0], [0]] and got[0][0, 1] == 3 and got[0][0, 9] == -2
    # the classes
    assert run([ZRL, ZRL], 1, 17, 1)[0] == [PS.COEF_OVERFLOW]
    assert run([level(5, 1)], 1, 5, 1)[0] == [PS.COEF_OVERFLOW]
    assert run([level(4, 1), eob()], 1, 5, 2)[0] == [0]
    assert run([eob(3)], 1, 5, 2)[0] == [PS.EOBRUN_OVERFLOW]
    assert run([eob(2)], 1, 5, 2)[0] == [0]
    assert run([eob(2), eob(1)], 1, 5, 2)[0] == [PS.LEFTOVER]
    assert run([eob(1)], 1, 5, 2)[0] == [PS.OUT_OF_DATA]
    assert run(["1" * 16, eob(2)], 1, 5, 2)[0] == [PS.BAD_CODE]
    assert run(None, 1, 5, 2, raw=tokens([eob(1)], LONG_AC) + b"\xff\xc4" + tokens([eob(1)], LONG_AC))[0] == [PS.UNEXPECTED_MARKER]
    st, p = run([level(0, 7), level(0, 5), level(9, 1), eob(1)], 1, 5, 3)  # block 0 fails after two levels
    assert st == [PS.COEF_OVERFLOW] and p[0, 1] == 7 and p[1, 0] == 5 and np.count_nonzero(p) == 2


def test_code_object_holds_the_two_kernels():
    from test_kernel_coverage import code_object_kernels
    names, n_objects = code_object_kernels(lib=PROG_DEC_LIB)
    assert n_objects == 1 and names == KERNELS, sorted(names ^ KERNELS)


# ------------------------------------------------------------------------------------------ GPU
SENT, CANARY = 0x5A5A, -0x5556


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    torch.cuda.set_device(0)
    api.init(0)
    return torch


class DevPlane:
    """a host plane on the device inside a margin of canaries (8 rows, 8 columns each way: rows stay 16-byte aligned)"""

    def __init__(self, torch, host):
        rows, cols = host.shape
        self.t = torch.full((rows + 16, cols + 16), CANARY, dtype=torch.int16, device="cuda")
        self.v = self.t[8:8 + rows, 8:8 + cols]
        self.v.copy_(torch.from_numpy(np.ascontiguousarray(host)).cuda())

    def result(self):
        a = self.t.cpu().numpy()
        inner = a[8:-8, 8:-8].copy()
        a[8:-8, 8:-8] = CANARY
        assert (a == CANARY).all(), "written outside the plane"
        return inner


def band_mask(ss, se, gx, gy, shape):
    """True at the band's positions of the gx x gy blocks at the top left of a plane of `shape`"""
    blk = np.zeros(64, dtype=bool)
    blk[[E.ZZ[k] for k in range(ss, se + 1)]] = True
    m = np.zeros(shape, dtype=bool)
    m[:gy * 8, :gx * 8] = np.tile(blk.reshape(8, 8), (gy, gx))
    return m


def launch(torch, scan, ss, se, specs, comps, mx, my, ri, tables=None, ah=0, al=0):
    """index + decode of one scan.  comps: [(host plane, h, v, dc_slot, ac_slot)].  -> (planes after, statuses), canaries checked.
    ah, al: successive approximation; a DC refinement scan (ss == 0, ah > 0) reads no table and is given none"""
    from simd_dct_amd import jpeg_decode as D
    planes = [DevPlane(torch, c[0]) for c in comps]
    d = _desc([(p.v.data_ptr(), p.v.stride(0), c[0].shape[1] // 8, c[0].shape[0] // 8, c[1], c[2], c[3], c[4]) for p, c in zip(planes, comps)], mx, my, ri)
    n = D.prog_intervals(d, ss, se)
    L = len(scan)
    buf = torch.full((L + 128,), 0xC3, dtype=torch.uint8, device="cuda")
    if L:
        buf[64:64 + L] = torch.frombuffer(bytearray(scan), dtype=torch.uint8).cuda()
    seg = buf[64:64 + max(L, 1)]
    off = torch.full((n + 3,), -1, dtype=torch.int64, device="cuda")
    status = torch.full((n + 2,), -9, dtype=torch.int32, device="cuda")
    own = tables is None and not (ss == 0 and ah)
    tables = D.Tables(specs) if own else tables
    D.index(seg, n, off[1:n + 2], status[1:n + 1], scan_len=L)
    D.decode_prog(d, ss, se, tables, seg, off[1:n + 2], status[1:n + 1], scan_len=L, ah=ah, al=al)
    torch.cuda.synchronize()
    if own:
        tables.close()
    b = buf.cpu().numpy()
    assert (b[:64] == 0xC3).all() and (b[64 + L:] == 0xC3).all() and b[64:64 + L].tobytes() == bytes(scan), "the scan buffer"
    o, s = off.cpu().numpy(), status.cpu().numpy()
    assert o[0] == -1 and o[-1] == -1 and s[0] == -9 and s[-1] == -9, "offsets / status canaries"
    return [p.result() for p in planes], s[1:-1].tolist()


def check(torch, scan, ss, se, specs, truths, sampling, mx, my, ri, good=True, slots=None, tables=None, ah=0, al=0, pre=None):
    """Decode `scan` on the GPU into planes that hold a sentinel everywhere but in the band's positions of the blocks the scan covers
    (zero there), one block larger each way than the grid, and compare planes and statuses with jpeg_progressive_status.  good: all
    statuses 0 and the band equals truths (the encoder's input).  sampling: [(h, v)] per component, None for one component over its
    own grid of mx x my blocks.  -> (planes, statuses)
    ah, al: successive approximation.  With either set the truth is jpeg_progressive_approx_checker.decode_scan, run on a copy of
    what is uploaded.  A refinement scan (ah = al + 1) finds `pre` (a plane per component) in the band's positions in place of the
    zeros; of a refinement interval that fails only the status is compared: what it leaves in its own blocks' band is unspecified
    (include/mdct_jpegdec_prog.h), every other block, position and sentinel is compared as ever."""
    one = sampling is None
    samp = [(1, 1)] if one else sampling
    slots = slots or [(min(c, 1), 2 + min(c, 1)) for c in range(len(samp))]
    hosts, masks = [], []
    for c, (h, v) in enumerate(samp):
        gx, gy = mx * h, my * v
        host = np.full(((gy + 1) * 8, (gx + 1) * 8), SENT, dtype=np.int16)
        m = band_mask(ss, se, gx, gy, host.shape)
        host[m] = 0
        if pre is not None:
            t = np.zeros(host.shape, dtype=np.int16)
            t[:gy * 8, :gx * 8] = pre[c][:gy * 8, :gx * 8]
            host[m] = t[m]
        hosts.append(host)
        masks.append(m)
    layout = [(ci, hh, vv, h, v) for ci, (h, v) in enumerate(samp) for vv in range(v) for hh in range(h)]
    if ss == 0:
        tabs = None if ah else {ci: DC.code_table(*specs[slots[ci][0]]) for ci in range(len(samp))}
    else:
        tabs = DC.code_table(*specs[slots[0][1]])
    want = [h.copy() for h in hosts]
    order, per = PS.block_order(mx, my, layout), ri * len(layout)
    if ah or al:
        want_st = XC.decode_scan(scan, ss, se, ah, al, tabs, order, per, want)
    else:
        want_st = PS.decode_scan(scan, ss, se, tabs, order, per, want)
    got, st = launch(torch, scan, ss, se, specs, [(hosts[c], samp[c][0], samp[c][1], slots[c][0], slots[c][1]) for c in range(len(samp))], mx, my, ri,
                     tables=tables, ah=ah, al=al)
    assert st == want_st, (st, want_st)
    loose = [np.zeros(h.shape, dtype=bool) for h in hosts]  # the band of the blocks of a failed refinement interval
    if ah:
        for k, s in enumerate(want_st):
            for ci, by, bx in order[k * per:(k + 1) * per] if s else ():
                loose[ci][by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = True
    for c, (g, w, m) in enumerate(zip(got, want, masks)):
        same = (g == w) | (loose[c] & m)
        assert same.all(), (c, np.argwhere(~same)[:8].tolist())
        assert (g[~m] == SENT).all(), "outside the band or the grid"
        if good:
            t = np.zeros(g.shape, dtype=np.int16)
            t[:truths[c].shape[0], :truths[c].shape[1]] = truths[c]
            assert np.array_equal(g[m], t[m]), c
    if good:
        assert st == [0] * len(st), st
    return got, st


def blocks_of(p, gx, gy):
    return [p[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] for by in range(gy) for bx in range(gx)]


def ac_segments(p, gx, gy, ss, se, spec, R=None):
    """the band coded with restart intervals of R blocks (default: a block row)"""
    if R is None or R == gx:
        segs, _, lost, uncoded = PE.ac_scan(p, gx, gy, ss, se, spec)
        assert lost == 0 and uncoded == 0
        return segs
    bl, segs = blocks_of(p, gx, gy), []
    for i in range(0, len(bl), R):
        row = np.concatenate(bl[i:i + R], axis=1)
        s, _, lost, uncoded = PE.ac_scan(row, row.shape[1] // 8, 1, ss, se, spec)
        assert lost == 0 and uncoded == 0
        segs += s
    return segs


def dc_segments(p, gx, gy, spec, R=None):
    bl, segs = blocks_of(p, gx, gy), []
    R = R or gx
    for i in range(0, len(bl), R):
        row = np.concatenate(bl[i:i + R], axis=1)
        s, _, lost = PE.dc_scan(dict(width=row.shape[1], height=8, comps=[(1, 1)]), [(0, 0)], [row], {0: spec})
        assert lost == 0
        segs += s
    return segs


AC_SPECS = [None, None, LONG_AC, None]
DC_SPECS = [DC0, DC1, None, None]


def ac_check(torch, p, gx, gy, ss, se, R=None, spec=LONG_AC):
    scan = PE.scan_data(ac_segments(p, gx, gy, ss, se, spec, R))
    return check(torch, scan, ss, se, [None, None, spec, None], [p], None, gx, gy, R or gx), scan


def dc_check(torch, p, gx, gy, R=None):
    scan = PE.scan_data(dc_segments(p, gx, gy, DC0, R))
    return check(torch, scan, 0, 0, DC_SPECS, [p], None, gx, gy, R or gx), scan


@pytest.mark.gpu
@pytest.mark.parametrize("width", (255, 256, 257))
def test_one_plane_scans_at_the_seams_of_256_lanes(gpu, width):
    rng = np.random.default_rng(width)
    p = sparse(rng, (16, width * 8), density=0.08)
    for ss, se in ((1, 63), (6, 63), (1, 5), (7, 7), (63, 63)):  # (63, 63): se + 1 == 64, where a baseline block ends
        ac_check(gpu, p, width, 2, ss, se)
    dc_check(gpu, p, width, 2)


LAYOUTS = [("4:2:0", S420, (31, 32, 33)), ("4:2:2", S422, (31, 32, 33)), ("4:4:4", S444, (63, 64, 65))]


@pytest.mark.gpu
@pytest.mark.parametrize("name,sampling,widths", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_the_interleaved_dc_scan(gpu, name, sampling, widths):
    for mx in widths:
        hmax, vmax = sampling[0]
        frame = dict(width=mx * 8 * hmax, height=2 * 8 * vmax, comps=sampling)
        rng = np.random.default_rng(mx)
        planes = [sparse(rng, s) for s in E.plane_shapes(frame)]
        segs, _, lost = PE.dc_scan(frame, [(0, 0), (1, 1), (2, 1)], planes, {0: DC0, 1: DC1})
        assert lost == 0 and len(segs) == 2
        check(gpu, PE.scan_data(segs), 0, 0, DC_SPECS, planes, sampling, mx, 2, mx)


@pytest.mark.gpu
@pytest.mark.parametrize("R", (1, 7, 10, 25, 40), ids=lambda r: f"DRI {r}")
def test_restart_intervals_of_every_kind(gpu, R):
    """one block, 7, a row, two and a half rows, the whole plane (4 rows of 10 blocks)"""
    rng = np.random.default_rng(R)
    p = sparse(rng, (32, 80), density=0.2)
    p[8:16, 16:64] = 0
    p[::8, ::8] = rng.integers(-200, 200, (4, 10))
    ac_check(gpu, p, 10, 4, 1, 63, R)
    ac_check(gpu, p, 10, 4, 3, 9, R)
    dc_check(gpu, p, 10, 4, R)
    # more intervals than RST numbers, several rounds of RST0..7
    if R == 1:
        q = sparse(rng, (8, 30 * 8), density=0.1)
        ac_check(gpu, q, 30, 1, 1, 63, 1)
        dc_check(gpu, q, 30, 1, 1)


@pytest.mark.gpu
def test_interval_data_of_every_size(gpu):
    """band 1..2 with +-1 at both positions is two 4-bit tokens per block under LONG_AC (a 3-bit code and the sign): a byte a block, so
    n blocks are n bytes.  Fewer than 8 bytes, exactly 8, and 2047 / 2048 / 2049, where every one of the 256 lanes has data; then a
    dense row under 16-bit codes, whose sub-sequences are far longer than 8 bytes"""
    rng = np.random.default_rng(8)
    assert E.canonical_codes(*LONG_AC)[0x01][1] == 3
    for n in (1, 7, 8, 9, 2047, 2048, 2049):
        p = np.zeros((8, n * 8), dtype=np.int16)
        p[0, 1::8] = rng.choice([-1, 1], n)
        p[1, 0::8] = rng.choice([-1, 1], n)
        (_, _), scan = ac_check(gpu, p, n, 1, 1, 2)
        assert len(scan) == n and b"\xff" not in scan
    # three intervals of 2048 bytes
    p = np.zeros((24, 2048 * 8), dtype=np.int16)
    p[0::8, 1::8] = rng.choice([-1, 1], (3, 2048))
    p[1::8, 0::8] = rng.choice([-1, 1], (3, 2048))
    ac_check(gpu, p, 2048, 3, 1, 2)
    dense = rng.integers(100, 1023, (16, 70 * 8)).astype(np.int16) * rng.choice([-1, 1], (16, 70 * 8)).astype(np.int16)
    (_, _), scan = ac_check(gpu, dense, 70, 2, 1, 63)
    assert len(scan) > 2 * 256 * 24
    dc = np.zeros((8, 600 * 8), dtype=np.int16)
    dc[0, ::8] = rng.integers(-1023, 1024, 600)
    (_, _), scan = dc_check(gpu, dc, 600, 1)
    assert len(scan) > 256 * 3


def busy(rng, ss, se):
    k = int(rng.integers(ss, se + 1))
    return zz_block({k: int(rng.choice([-3, -1, 1, 2, 5]))})


EMPTY = np.zeros((8, 8), dtype=np.int16)


@pytest.mark.gpu
def test_end_of_band_runs(gpu):
    torch = gpu
    rng = np.random.default_rng(18)
    for ss, se in ((1, 63), (6, 63)):
        # every length 1 .. 18 between busy blocks, ending in a run
        row = []
        for n in range(1, 19):
            row += [busy(rng, ss, se)] + [EMPTY] * n
        p = np.concatenate(row, axis=1)
        ac_check(torch, p, len(row), 1, ss, se)
        # ... and ending in a busy block; a block that ends at se between two runs; a tail block followed by empties
        tail = [EMPTY] * 5 + [zz_block({se: 1})] + [EMPTY] * 3 + [zz_block({ss: -2, se: 4})] + [EMPTY] * 9 + [busy(rng, ss, se)]
        ac_check(torch, np.concatenate(row + tail, axis=1), len(row) + len(tail), 1, ss, se)
        ac_check(torch, np.concatenate([busy(rng, ss, se)] + [EMPTY] * 40, axis=1), 41, 1, ss, se)
        # a run that starts in one sub-sequence and ends many lanes' blocks later: 300 busy blocks, 500 empty ones, 300 busy ones
        dense = [zz_block({k: int(rng.integers(1, 900)) for k in range(ss, se + 1, 2)}) for _ in range(40)]
        long = dense[:20] + [EMPTY] * 500 + dense[20:] + [EMPTY] * 77
        ac_check(torch, np.concatenate(long, axis=1), len(long), 1, ss, se)
    # rows with nothing in the band, 1 .. 257 blocks: one token each, two rows per scan
    from simd_dct_amd import jpeg_decode as D
    tables = D.Tables(AC_SPECS)
    for n in range(1, 258):
        p = np.zeros((16, n * 8), dtype=np.int16)
        p[0, 0] = 3  # a DC level is not the band's matter
        scan = PE.scan_data(ac_segments(p, n, 2, 1, 63, LONG_AC))
        check(torch, scan, 1, 63, AC_SPECS, [p], None, n, 2, n, tables=tables)
    tables.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n,at", ((32766, None), (32767, None), (32768, None), (65535, None), (65535, 40000)))
def test_the_longest_runs(gpu, n, at):
    """rows of 32766 .. 65535 empty blocks: EOB14 holds 32767 blocks, the encoder splits there; with one block at 40000"""
    p = np.zeros((8, n * 8), dtype=np.int16)
    if at is not None:
        p[1, at * 8] = -7
    (_, _), scan = ac_check(gpu, p, n, 1, 1, 63)
    assert len(scan) < 16


@pytest.mark.gpu
def test_levels_and_zero_runs(gpu):
    torch = gpu
    for ss, se in ((1, 63), (5, 60)):
        blocks = [zz_block({ss: 1}), zz_block({se: -1}), zz_block({ss: 1023, se: -1023}), zz_block({ss: -1023, ss + 1: 1023})]
        for z in (15, 16, 31, 32, 47):
            blocks += [zz_block({ss: 2, ss + z + 1: -3}), zz_block({ss + z: 5})]  # z zeros after a level; z zeros from the band's start
        blocks += [zz_block({k: (-1) ** k * (1 << (k % 10)) for k in range(ss, se + 1)})]  # every size
        ac_check(torch, np.concatenate(blocks, axis=1), len(blocks), 1, ss, se)
    # by hand: a ZRL that ends exactly at se (k = se + 1 ends the block), in three bands
    for ss, se, items in ((1, 16, [ZRL, level(0, 9), eob()]), (1, 17, [level(0, 3), ZRL, level(2, -2), eob()]), (32, 63, [ZRL, ZRL, eob(1)]),
                          (1, 63, [level(14, 1), ZRL, ZRL, ZRL, eob(1)])):
        scan = PE.scan_data([tokens(items, LONG_AC)])
        got, st = check(torch, scan, ss, se, AC_SPECS, None, None, 2, 1, 2, good=False)
        assert st == [0]
    # DC: +-2047 differences, steps of 2047, 0
    dc = np.zeros((8, 40 * 8), dtype=np.int16)
    dc[0, ::8] = [0, 2047, 0, -2047, 0, 1023, -1024, 1023, 1, -1] * 4
    dc_check(torch, dc, 40, 1)
    dc_check(torch, dc, 40, 1, 3)


@pytest.mark.gpu
def test_stuffing(gpu):
    """band 1..1 with the level 255 under a table whose only long code is 8 bits: code byte, 0xFF, stuffed zero -- three bytes a block,
    so that the 8-byte sub-sequences of a short interval start at every phase of the triple, the stuffed zero included; then longer
    intervals, whose sub-sequences are 10 to 14 bytes; fill bytes before RSTm; every interval ends in 0xFF 0x00"""
    torch = gpu
    spec = E.spec_from_lengths({0x08: 8, 0x00: 8, 0x01: 8, 0x10: 8, 0x20: 8})
    specs = [None, None, spec, None]
    for n in (3, 8, 9, 85, 256 * 3 + 1, 256 * 10 // 3 + 5, 256 * 11 // 3 + 2, 256 * 13 // 3 + 7):
        p = np.zeros((16, n * 8), dtype=np.int16)
        p[0::8, 1::8] = 255
        (got, st), scan = ac_check(torch, p, n, 2, 1, 1, spec=spec)
        assert scan.count(b"\xff\x00") == 2 * n and len(scan) == 6 * n + 2
        # fill bytes in front of the RSTm
        filled = scan.replace(b"\xff\xd0", b"\xff\xff\xff\xff\xd0")
        assert len(filled) == len(scan) + 3
        check(torch, filled, 1, 1, specs, [p], None, n, 2, n)
    # a DC scan whose amplitude bits are all ones: category 8 in Annex K's table is 6 bits, so the 0xFF bytes fall anywhere
    dc = np.zeros((8, 700 * 8), dtype=np.int16)
    dc[0, ::8] = np.cumsum(np.tile([255, -255, 255, 255, -255, -255], 117)[:700])
    (_, _), scan = dc_check(torch, dc, 700, 1, 350)
    assert scan.count(b"\xff\x00") > 50


# ---- failing intervals
def _five_intervals(rng, ss, se, n=24):
    p = sparse(rng, (40, n * 8), density=0.12)
    p[16:24, 10 * 8:] = 0  # the middle interval ends in a run
    p[17, 3 * 8 + 2] = 9
    return p, ac_segments(p, n, 5, ss, se, LONG_AC)


def _bad(torch, segs, ss, se, n, want, k=2, scan=None, specs=AC_SPECS, rows=None):
    """segs: unstuffed intervals (or scan: the bytes); interval k must fail with `want`, the others are good"""
    scan = PE.scan_data(segs) if scan is None else scan
    got, st = check(torch, scan, ss, se, specs, None, None, n, rows or len(segs), n, good=False)
    assert st[k] == want and all(s == 0 for i, s in enumerate(st) if i != k), st
    return got, st


@pytest.mark.gpu
def test_failing_intervals_of_an_ac_band(gpu):
    """every error class in the middle interval of five, then in the first, the last and the only one.  A run "32767 too long" cannot
    be one token: a run that fits ends the interval, and what follows is LEFTOVER.  The longest run there is, 32767, is met instead
    where 21 blocks are left and where one block is left."""
    torch = gpu
    rng = np.random.default_rng(77)
    n = 24
    for ss, se in ((1, 63), (4, 40)):
        p, segs = _five_intervals(rng, ss, se, n)
        check(torch, PE.scan_data(segs), ss, se, AC_SPECS, [p], None, n, 5, n)
        mid = segs[2]

        def with_mid(b):
            return segs[:2] + [b] + segs[3:]

        _bad(torch, with_mid(mid[:len(mid) // 2]), ss, se, n, PS.OUT_OF_DATA)
        _bad(torch, with_mid(b""), ss, se, n, PS.OUT_OF_DATA)
        # by hand: three good blocks, then what fails, then tokens that a re-synchronised decode would take for more blocks
        good3 = [level(0, 5), level(1, -2), eob(1), level(2, 1), eob(2)]
        more = [level(0, 3), eob(1)] * 30
        fin = [eob(n - 3)]
        assert PS.decode_scan(PE.scan_data([tokens(good3 + fin, LONG_AC)]), ss, se, DC.code_table(*LONG_AC), PS.block_order(n, 1, [(0, 0, 0, 1, 1)]), n,
                              [np.zeros((8, n * 8), dtype=np.int16)]) == [0]
        _bad(torch, with_mid(tokens(good3 + ["1" * 16] + more, LONG_AC)), ss, se, n, PS.BAD_CODE)
        _bad(torch, with_mid(tokens(good3 + [level(0, 7), level(15, 1), level(15, 1), level(15, 1), level(15, 1)] + more, LONG_AC)), ss, se, n, PS.COEF_OVERFLOW)
        _bad(torch, with_mid(tokens(good3 + [level(0, 7), ZRL, ZRL, ZRL, ZRL] + more, LONG_AC)), ss, se, n, PS.COEF_OVERFLOW)
        _bad(torch, with_mid(tokens(good3 + [level(0, -4), eob(n - 3 + 1)] + more, LONG_AC)), ss, se, n, PS.EOBRUN_OVERFLOW)
        _bad(torch, with_mid(tokens(good3 + [eob(n - 3 + 1)], LONG_AC)), ss, se, n, PS.EOBRUN_OVERFLOW)
        # the longest run there is (32767) where fewer blocks are left: 32767 - (n - 3) too long; and with one block left
        _bad(torch, with_mid(tokens(good3 + [eob(32767)] + more, LONG_AC)), ss, se, n, PS.EOBRUN_OVERFLOW)
        _bad(torch, with_mid(tokens(good3 + [eob(n - 4), eob(32767)], LONG_AC)), ss, se, n, PS.EOBRUN_OVERFLOW)
        _bad(torch, with_mid(tokens(good3 + fin + [level(0, 3), eob(1)], LONG_AC)), ss, se, n, PS.LEFTOVER)
        _bad(torch, with_mid(mid + b"\x00"), ss, se, n, PS.LEFTOVER)
        # markers: a wrong RSTm after the interval, a marker inside its data, a missing marker
        scan = PE.scan_data(segs)
        assert scan.count(b"\xff\xd2") == 1
        _bad(torch, None, ss, se, n, PS.UNEXPECTED_MARKER, scan=scan.replace(b"\xff\xd2", b"\xff\xd5"), rows=5)
        cut = len(PE.scan_data(segs[:2])) + 2 + 5
        _bad(torch, None, ss, se, n, PS.UNEXPECTED_MARKER, scan=scan[:cut] + b"\xff\xc4" + scan[cut:], rows=5)
        got, st = check(torch, scan.replace(b"\xff\xd2", b""), ss, se, AC_SPECS, None, None, n, 5, n, good=False)
        assert st[:2] == [0, 0] and st[2] != 0 and st[4] == PS.OUT_OF_DATA, st
    # the failing interval as the first, the last, the only one
    p, segs = _five_intervals(rng, 1, 63, n)
    _bad(torch, [tokens(["1" * 16] * 3, LONG_AC)] + segs[1:], 1, 63, n, PS.BAD_CODE, k=0)
    _bad(torch, segs[:4] + [segs[4][:3]], 1, 63, n, PS.OUT_OF_DATA, k=4)
    _bad(torch, [tokens([level(0, 1), eob(n + 1)], LONG_AC)], 1, 63, n, PS.EOBRUN_OVERFLOW, k=0)


@pytest.mark.gpu
def test_failing_intervals_across_many_lanes(gpu):
    """an interval long enough that the lanes behind the error hold blocks of their own: what they wrote goes back to zero"""
    torch = gpu
    rng = np.random.default_rng(78)
    n = 400
    p = sparse(rng, (24, n * 8), density=0.3, amp=300)
    segs = ac_segments(p, n, 3, 1, 63, LONG_AC)
    assert len(segs[1]) > 256 * 16
    half = len(segs[1]) // 2
    for bad, want in ((segs[1][:half], PS.OUT_OF_DATA), (segs[1][:half] + b"\xff\xff" + segs[1][half:], None)):
        scan = PE.scan_data([segs[0], bad, segs[2]])
        got, st = check(torch, scan, 1, 63, AC_SPECS, None, None, n, 3, n, good=False)
        assert st[0] == 0 and st[2] == 0 and st[1] != 0 and (want is None or st[1] == want), st
    # a run too long in the middle of the data, and an invalid code: the data behind them decodes to blocks under speculation
    items = [level(0, int(v)) if i % 10 else eob(1) for i, v in enumerate(rng.integers(1, 500, 3000))]  # 150 blocks before the break
    for broken, want in ((items[:1500] + [eob(32767)] + items[1500:], PS.EOBRUN_OVERFLOW), (items[:1500] + ["1" * 16] + items[1500:], PS.BAD_CODE),
                         (items[:1500] + [ZRL] * 5 + items[1500:], PS.COEF_OVERFLOW)):
        scan = PE.scan_data([segs[0], tokens(broken, LONG_AC), segs[2]])
        got, st = check(torch, scan, 1, 63, AC_SPECS, None, None, n, 3, n, good=False)
        assert st == [0, want, 0], st


@pytest.mark.gpu
def test_failing_intervals_of_a_dc_scan(gpu):
    torch = gpu
    rng = np.random.default_rng(79)
    # one plane
    n = 300
    p = np.zeros((24, n * 8), dtype=np.int16)
    p[::8, ::8] = rng.integers(-1000, 1000, (3, n))
    segs = dc_segments(p, n, 3, DC0)
    assert len(segs[1]) > 256
    stuffed = lambda b: b.replace(b"\xff", b"\xff\x00")  # noqa: E731
    for bad, want in ((stuffed(segs[1][:100]), PS.OUT_OF_DATA), (stuffed(segs[1] + b"\x12"), PS.LEFTOVER), (stuffed(segs[1][:100] + b"\xff\xfe" + segs[1][100:]), None),
                      (stuffed(segs[1][:150]) + b"\xff\xc4" + stuffed(segs[1][150:]), PS.UNEXPECTED_MARKER)):
        scan = stuffed(segs[0]) + b"\xff\xd0" + bad + b"\xff\xd1" + stuffed(segs[2])
        got, st = check(torch, scan, 0, 0, DC_SPECS, None, None, n, 3, n, good=False)
        assert st[0] == 0 and st[2] == 0 and st[1] != 0 and (want is None or st[1] == want), st
    # Annex K's DC table is complete but for the all-ones code: nine 1-bits are no code
    lone = [DC0, DC1, None, None]
    bits = tokens([(4, 9, 4), (0, 0, 0), "1" * 16, (3, 2, 3), (0, 0, 0)] + [(2, 1, 2)] * 40, DC0)
    got, st = check(torch, PE.scan_data([segs[0], bits, segs[2]]), 0, 0, lone, None, None, n, 3, n, good=False)
    assert st == [0, PS.BAD_CODE, 0]
    # interleaved 4:2:0, the middle MCU row truncated
    frame = dict(width=40 * 16, height=3 * 16, comps=S420)
    planes = [sparse(rng, s) for s in E.plane_shapes(frame)]
    segs, _, _ = PE.dc_scan(frame, [(0, 0), (1, 1), (2, 1)], planes, {0: DC0, 1: DC1})
    for bad in (segs[1][:len(segs[1]) // 3], segs[1][:-1]):
        got, st = check(torch, PE.scan_data([segs[0], bad, segs[2]]), 0, 0, DC_SPECS, None, S420, 40, 3, 40, good=False)
        assert st == [0, PS.OUT_OF_DATA, 0], st


@pytest.mark.gpu
def test_an_empty_table_slot_is_refused(gpu):
    torch = gpu
    from simd_dct_amd import jpeg_decode as D
    p = np.zeros((8, 64), dtype=np.int16)
    scan = PE.scan_data(ac_segments(p, 8, 1, 1, 63, LONG_AC))
    comp = [(p, 1, 1, 0, 2)]
    with pytest.raises(api.MdctError, match="empty table slot"):
        launch(torch, scan, 1, 63, [DC0, None, None, LONG_AC], comp, 8, 1, 8)  # the AC slot 2 is empty
    with pytest.raises(api.MdctError, match="empty table slot"):
        launch(torch, scan, 0, 0, [None, DC1, LONG_AC, None], comp, 8, 1, 8)  # the DC slot 0 is empty
    # ... and the other class may be empty
    launch(torch, scan, 1, 63, [None, None, LONG_AC, None], comp, 8, 1, 8)
    launch(torch, PE.scan_data(dc_segments(p, 8, 1, DC0)), 0, 0, [DC0, None, None, None], comp, 8, 1, 8)
    assert D.STATUS_NAMES[7] and D.STATUS_NAMES[3]


# ---- whole files
def _cpu(ts):
    return [t.cpu().numpy() for t in ts]


WHOLE = ["grey 8x8", "grey 2056x16 unmarked", "4:4:4 24x40 interleaved DRI 2", "4:2:0 40x24 three scans unmarked", "4:2:0 528x32 interleaved", "4:2:2 48x16",
         "Adobe RGB, three tables"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", WHOLE)
def test_whole_files(gpu, name):
    Image = pytest.importorskip("PIL.Image")
    from simd_dct_amd import jpeg_decode as D
    from simd_dct_amd import jpeg_transcode as TC
    from test_jpeg_transcode import _input, _legal_interleaved
    data, frame, planes = _input(name)
    src = jfif.read_jpeg(data, require_restart=False)
    sampling = frame["comps"]
    nc = len(sampling)
    qtables = [src["qtables"][c["tq"]].astype(np.int64) for c in src["components"]]
    _, coefs = D.decode_coefficients(data)
    source = _cpu(coefs)
    base_planes = _cpu(D.decode_jpeg(data))
    base_rgb = {(lay, sd): D.decode_jpeg(data, mode="RGB", layout=lay, scale_denom=sd).cpu().numpy() for lay in ("HWC", "CHW") for sd in (1, 2, 4, 8)}
    base_scaled = {sd: _cpu(D.decode_jpeg(data, scale_denom=sd)) for sd in (2, 4, 8)}
    plain = TC.transcode_jpeg(data)
    transposed = TC.transcode_jpeg(data, transform="transpose")
    for inter in (False, True):
        if inter and not _legal_interleaved(sampling):
            continue
        for bands in (None, CUSTOM[nc]):
            if bands is None:
                prog = TC.transcode_jpeg(data, progressive=True, interleaved=inter)
            else:
                prog = TC.encode_coefficients(coefs, qtables, frame["width"], frame["height"], sampling, colorspace=src["colorspace"], progressive=True,
                                              interleaved=inter, bands=bands)
            assert jfif.sof_marker(prog) == 0xC2
            info, got = D.decode_coefficients(prog)
            assert info["sof"] == 0xC2 and info["colorspace"] == src["colorspace"]
            for g, w in zip(_cpu(got), as_written(frame, source, inter)):
                assert np.array_equal(g, w), (name, inter, bands)
            px, cf = D.decode_jpeg(prog, coefficients=True)
            for g, w in zip(_cpu(px), base_planes):
                assert np.array_equal(g, w)
            for g, w in zip(_cpu(cf), _cpu(got)):
                assert np.array_equal(g, w)
            for (lay, sd), want in base_rgb.items():
                assert np.array_equal(D.decode_jpeg(prog, mode="RGB", layout=lay, scale_denom=sd).cpu().numpy(), want), (name, inter, lay, sd)
            for sd, want in base_scaled.items():
                for g, w in zip(_cpu(D.decode_jpeg(prog, scale_denom=sd)), want):
                    assert np.array_equal(g, w), (name, inter, sd)
            # back to baseline, byte for byte what the baseline source gives; with a transform too
            assert TC.transcode_jpeg(prog) == plain
            assert TC.transcode_jpeg(prog, transform="transpose") == transposed
            if bands is None:
                assert TC.transcode_jpeg(prog, progressive=True, interleaved=inter) == prog, "progressive -> progressive"
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(prog)).convert("RGB")), np.asarray(Image.open(io.BytesIO(data)).convert("RGB")))


@pytest.mark.gpu
def test_rgb_equals_pillow_on_idct_exact_progressive_files(gpu):
    """DC-only blocks under a quantiser of 8 decode to dc + 128 in libjpeg and here: on such files test_jpeg_color holds the baseline
    path to Pillow exactly, and the progressive path must be held the same way.  A file with a luma band missing is such a file when
    only that band held AC levels: Pillow and the engine both take the missing band for zeros."""
    torch = gpu
    Image = pytest.importorskip("PIL.Image")
    from simd_dct_amd import jpeg_decode as D
    from simd_dct_amd import jpeg_transcode as TC
    rng = np.random.default_rng(5)
    q = [np.full(64, 8)] * 3
    for sampling, (W, H) in ((S444, (37, 21)), (S420, (83, 45)), (S422, (50, 17)), ([(1, 1)], (19, 30))):
        frame = dict(width=W, height=H, comps=sampling)
        planes = []
        for rows, cols in E.plane_shapes(frame):
            p = np.zeros((rows, cols), dtype=np.int16)
            p[::8, ::8] = rng.integers(-15, 16, (rows // 8, cols // 8))
            planes.append(p)
        zr, zc = divmod(int(E.ZZ[12]), 8)  # zig-zag 12: in luma's band 10..63
        planes[0][zr::8, zc::8] = rng.integers(-3, 4, planes[0][zr::8, zc::8].shape)
        dev = [torch.from_numpy(p).cuda() for p in planes]
        nc = len(sampling)
        for inter in (False, True):
            if inter and nc == 1:
                continue
            prog = TC.encode_coefficients(dev, q[:nc], W, H, sampling, progressive=True, interleaved=inter)
            a, b = _group(prog, [(s["ss"], s["se"]) for s in PC.parse(prog)[2]].index((10, 63)))
            cut = prog[:a] + prog[b:]
            info, got = D.decode_coefficients(cut)
            want = [p.copy() for p in as_written(frame, planes, inter)]
            want[0][zr::8, zc::8] = 0
            for g, w in zip(_cpu(got), want):
                assert np.array_equal(g, w)
            pil = np.asarray(Image.open(io.BytesIO(cut)).convert("RGB"))
            assert np.array_equal(D.decode_jpeg(cut, mode="RGB").cpu().numpy(), pil), (sampling, inter)
            assert np.array_equal(D.decode_jpeg(cut, mode="RGB", layout="CHW").cpu().numpy(), pil.transpose(2, 0, 1))
            # and the whole file against the baseline file of the same coefficients, through Pillow and through the engine
            base = TC.encode_coefficients(dev, q[:nc], W, H, sampling)
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(prog)).convert("RGB")), np.asarray(Image.open(io.BytesIO(base)).convert("RGB")))
            assert np.array_equal(D.decode_jpeg(prog, mode="RGB").cpu().numpy(), D.decode_jpeg(base, mode="RGB").cpu().numpy())


@pytest.mark.gpu
def test_encode_jpeg_progressive_round_trip(gpu):
    from simd_dct_amd import jpeg_decode as D
    from simd_dct_amd import jpeg_encode as J
    rng = np.random.default_rng(31)
    y, x = np.mgrid[0:45, 0:83]
    colour = np.clip(np.stack([128 + 100 * np.sin(x / 5.0 + c) * np.cos(y / 4.0 - c) for c in range(3)], axis=-1) + rng.normal(0, 20, (45, 83, 3)), 0, 255).astype(np.uint8)
    grey = rng.integers(0, 256, (9, 17)).astype(np.uint8)
    for img, q, sub in [(colour, q, s) for q in (5, 75, 100) for s in ("4:2:0", "4:4:4", "4:2:2")] + [(grey, 75, "4:2:0")]:
        base = J.encode_jpeg(img, quality=q, subsampling=sub, optimize=True)
        want_px, want_cf = D.decode_jpeg(base, coefficients=True)
        want_rgb = D.decode_jpeg(base, mode="RGB")
        for kw in (dict(), dict(interleaved=True)):
            prog = J.encode_jpeg(img, quality=q, subsampling=sub, progressive=True, **kw)
            px, cf = D.decode_jpeg(prog, coefficients=True)
            for g, w in zip(px, want_px):
                assert gpu.equal(g, w), (q, sub, kw)
            assert gpu.equal(D.decode_jpeg(prog, mode="RGB"), want_rgb)
            if not kw:
                for g, w in zip(cf, want_cf):
                    assert gpu.equal(g, w), (q, sub)


@pytest.mark.gpu
def test_a_corrupted_interval_raises_with_the_statuses(gpu):
    from simd_dct_amd import jpeg_decode as D
    frame = FRAMES["4:2:0"]
    planes = make_planes(frame, 9, True)
    data, info = PE.encode_file(frame, planes, interleaved_dc=True)
    scans = PC.parse(data)[2]
    k = 2  # the DC scan, luma 1..2, then luma's band 3..9: four intervals of 8 blocks
    assert (scans[k]["ss"], scans[k]["se"], scans[k]["dri"]) == (3, 9, 8)
    s = scans[k]
    body = data[s["start"]:s["end"]]
    cut = body.index(b"\xff\xd1") - 3
    bad = data[:s["start"]] + body[:cut] + body[cut + 3:] + data[s["end"]:]
    with pytest.raises(D.JpegDecodeError, match=r"scan 2 \(band 3\.\.9\): 1 of 4 restart intervals failed; interval 1") as e:
        D.decode_jpeg(bad)
    assert e.value.scan == 2 and [int(x != 0) for x in e.value.status] == [0, 1, 0, 0]
    with pytest.raises(D.JpegDecodeError):
        from simd_dct_amd import jpeg_transcode as TC
        TC.transcode_jpeg(bad)
    # a run too long has its own name
    s = scans[1]
    long = data[:s["start"]] + PE.scan_data([tokens([eob(9)], LONG_AC)] * 4) + data[s["end"]:]
    i = long.rindex(b"\xff\xc4", 0, s["start"])
    long = long[:i] + E._seg(0xC4, bytes([0x10]) + bytes(LONG_AC[0]) + bytes(LONG_AC[1])) + long[i + 4 + long[i + 3] + (long[i + 2] << 8) - 2:]
    with pytest.raises(D.JpegDecodeError, match="end-of-band run") as e:
        D.decode_coefficients(long)
    assert list(e.value.status) == [7, 7, 7, 7]


@pytest.mark.gpu
def test_index_and_decode_in_a_captured_graph(gpu):
    """both scans of a plane captured on one stream; every replay gives the planes and statuses of the plain calls"""
    torch = gpu
    from simd_dct_amd import jpeg_decode as D
    rng = np.random.default_rng(61)
    n = 300
    p = sparse(rng, (24, n * 8), density=0.1)
    ac = PE.scan_data(ac_segments(p, n, 3, 6, 63, LONG_AC)[:2] + [b"\x12\x34"])  # the last interval fails
    dc = PE.scan_data(dc_segments(p, n, 3, DC0))
    comp = [(np.zeros((24, n * 8), dtype=np.int16), 1, 1, 0, 2)]
    (want_dc,), st_dc = launch(torch, dc, 0, 0, DC_SPECS, comp, n, 3, n)
    (want_ac,), st_ac = launch(torch, ac, 6, 63, AC_SPECS, comp, n, 3, n)
    assert st_dc == [0, 0, 0] and st_ac[:2] == [0, 0] and st_ac[2] != 0
    plane = torch.zeros((24, n * 8), dtype=torch.int16, device="cuda")
    d = _desc([(plane.data_ptr(), plane.stride(0), n, 3, 1, 1, 0, 2)], n, 3, n)
    bufs = [torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda() for b in (dc, ac)]
    off = [torch.zeros((4,), dtype=torch.int64, device="cuda") for _ in range(2)]
    status = [torch.full((3,), -1, dtype=torch.int32, device="cuda") for _ in range(2)]
    tables = D.Tables([DC0, None, LONG_AC, None])
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        D.index(bufs[0], 3, off[0], status[0], stream=s)
        D.decode_prog(d, 0, 0, tables, bufs[0], off[0], status[0], stream=s)
        D.index(bufs[1], 3, off[1], status[1], stream=s)
        D.decode_prog(d, 6, 63, tables, bufs[1], off[1], status[1], stream=s)
    for _ in range(2):
        plane.zero_()
        for t in off + status:
            t.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert status[0].cpu().tolist() == st_dc and status[1].cpu().tolist() == st_ac
        assert np.array_equal(plane.cpu().numpy(), want_dc + want_ac)
    tables.close()


@pytest.mark.gpu
def test_one_decode_launch_per_scan(gpu):
    from simd_dct_amd import jpeg_decode as D
    frame = FRAMES["4:2:0 odd"]
    for inter, n_dc in ((True, 1), (False, 3)):
        data, info = PE.encode_file(frame, make_planes(frame, 7, inter), interleaved_dc=inter)
        gpu.cuda.synchronize()
        api.kernel_counts_reset()
        D.decode_coefficients(data)
        gpu.cuda.synchronize()
        ran = api.kernel_counts()
        assert ran.get("k_decode_prog_dc") == n_dc and ran.get("k_decode_prog_ac") == 5, ran
        assert ran.get("k_rst_scan") == n_dc + 5 and "k_decode" not in ran and not any(k.startswith("k_um_") for k in ran), ran
