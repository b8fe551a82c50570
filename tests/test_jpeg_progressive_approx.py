"""Progressive JPEG output with successive approximation: the ..._approx calls of libmdct_jpegprog.so (include/mdct_jpegprog.h),
jpeg_progressive.standard_script / check_script / encode, jfif.write_progressive_jpeg with Ah / Al, and script= of
encode_coefficients, transcode_jpeg and encode_jpeg.

Truth: tests/golden/progressive_pillow/*.prog*.jpg are libjpeg's own files (Pillow's progressive=True, optimize=True) of eight pictures;
jpeg_progressive_approx_encoder codes planes serially by the rules of jcphuff.c and reproduces every one of their scans;
jpeg_progressive_approx_checker decodes serially.  The two flush rules of a refinement scan that no golden file reaches (a run of
0x7FFF blocks, more than 937 buffered bits) are held to that encoder on synthetic planes, on which both are asserted to fire.

CPU: the encoder against the 17 golden files, scan bytes and tables; the scripts; the refusals of check_script and of the C-ABI;
write_progressive_jpeg unchanged for callers without Ah / Al.
GPU: all exact.  Every scan of the golden files from the checker's planes; transcode_jpeg(script="standard") against the golden twin;
read-back through decode_coefficients and the checker; encode_jpeg through decode_jpeg and Pillow; synthetic planes at the chunk
seams and at both flush rules, sub-ranges, canaries; a call on a stream that is not the current one."""
import glob
import io
import os
import struct

import numpy as np
import pytest

import jpeg_optimal_tables as T
import jpeg_progressive_approx_checker as AC
import jpeg_progressive_approx_encoder as AE
import jpeg_progressive_checker as PC
import jpeg_progressive_encoder as PE
import jpeg_scan_encoder as E
from simd_dct_amd import _jpegcoef_lib, _jpegenc_opt_lib, _jpegprog_lib, api, jfif
from simd_dct_amd import jpeg_progressive as P
from simd_dct_amd import jpeg_transcode as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "progressive_pillow")
ALL_FILES = sorted(os.path.basename(f) for f in glob.glob(os.path.join(GOLDEN, "*.prog*.jpg")))
PICTURES = sorted(f[:-len(".prog.jpg")] for f in ALL_FILES if f.endswith(".prog.jpg"))


def golden(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def raw_tables(data):
    """[{(class, id): (bits16, vals)} in force at each scan], from the file's DHT segments"""
    out, tabs, i = [], {}, 2
    while data[i + 1] != 0xD9:
        m, n = data[i + 1], struct.unpack_from(">H", data, i + 2)[0]
        seg = data[i + 4:i + 2 + n]
        i += 2 + n
        if m == 0xC4:
            p = 0
            while p < len(seg):
                bits = list(seg[p + 1:p + 17])
                tabs[(seg[p] >> 4, seg[p] & 15)] = (bits, list(seg[p + 17:p + 17 + sum(bits)]))
                p += 17 + sum(bits)
        elif m == 0xDA:
            out.append(dict(tabs))
            while not (data[i] == 0xFF and data[i + 1] not in (0x00, 0xFF) and not 0xD0 <= data[i + 1] <= 0xD7):
                i += 1
    return out


def spec_lists(spec):
    return [int(x) for x in spec[0]], [int(x) for x in spec[1]]


def parsed(data):
    """-> (jpeg_scan_encoder's frame, scans of jpeg_progressive_checker.parse each with 'raw': the tables in force as specifications)"""
    frame, _, scans, _ = PC.parse(data)
    for sc, raw in zip(scans, raw_tables(data)):
        sc["raw"] = raw
    return dict(width=frame["width"], height=frame["height"], comps=[(h, v) for _, h, v, _ in frame["components"]]), scans


def scan_specs(sc):
    """the specifications the scan codes with, as jpeg_progressive_approx_encoder.encode_scan takes them"""
    if sc["ss"] == 0:
        return None if sc["ah"] else {min(ci, 1): sc["raw"][(0, td)] for ci, td, _ in sc["comps"]}
    return sc["raw"][(1, sc["comps"][0][2])]


_checked = {}


def checker_scans(name):
    """a golden file through the serial encoder: (frame, planes, [(scan, per_interval, result)]), once"""
    if name not in _checked:
        data = golden(name)
        planes, statuses = AC.decode(data)
        assert all(s == AC.OK for st in statuses for s in st)
        frame, scans = parsed(data)
        out = []
        for sc in scans:
            units, upm, _ = AE.scan_units(frame, [ci for ci, _, _ in sc["comps"]], planes)
            per = sc["dri"] * upm if sc["dri"] else len(units)
            out.append((sc, per, AE.encode_scan(units, per, sc["ss"], sc["se"], sc["ah"], sc["al"], scan_specs(sc))))
        _checked[name] = (data, frame, planes, out)
    return _checked[name]


# ------------------------------------------------------------------------------------------ CPU
def test_the_golden_set():
    assert len(ALL_FILES) == 17 and len(PICTURES) == 8


@pytest.mark.parametrize("name", ALL_FILES)
def test_the_encoder_reproduces_every_scan_and_table_of_libjpegs_files(name):
    data, frame, planes, scans = checker_scans(name)
    dc_counts = sum(r["counts"] for sc, _, r in scans if sc["ss"] == 0 and sc["ah"] == 0)
    for k, (sc, per, r) in enumerate(scans):
        assert AE.scan_data(r["segs"]) == data[sc["start"]:sc["end"]], (name, k, sc["ss"], sc["se"], sc["ah"], sc["al"])
        assert r.get("lost", 0) == 0 and r.get("uncoded", 0) == 0
        if sc["ss"] == 0 and sc["ah"] == 0:
            for ci, td, _ in sc["comps"]:
                assert spec_lists(T.optimal_table(dc_counts[min(ci, 1), :16])) == spec_lists(sc["raw"][(0, td)]), (name, k, "DC table", ci)
        elif sc["ss"] != 0:
            assert spec_lists(T.optimal_table(r["counts"])) == spec_lists(sc["raw"][(1, sc["comps"][0][2])]), (name, k, "AC table")
            assert r["full_run_flushes"] == 0 and r.get("bit_flushes", 0) == 0, "no golden file reaches either flush rule"


def test_standard_script_is_the_script_of_the_golden_files():
    seen = set()
    for name in ALL_FILES:
        frame, scans = parsed(golden(name))
        nc = len(frame["comps"])
        seen.add(nc)
        assert [(tuple(ci for ci, _, _ in s["comps"]), s["ss"], s["se"], s["ah"], s["al"]) for s in scans] == P.standard_script(nc), name
    assert seen == {1, 3}
    assert len(P.standard_script(1)) == 6 and len(P.standard_script(3)) == 10
    for nc in (1, 3):
        assert P.check_script(P.standard_script(nc), nc) == P.standard_script(nc)
    with pytest.raises(ValueError):
        P.standard_script(2)


Y, ALL = (0,), (0, 1, 2)
BAD_SCRIPTS = {
    "an AC scan before the DC scan": ([(Y, 1, 63, 0, 0), (Y, 0, 0, 0, 0)], 1, "scan 0"),
    "a position coded a second time": ([(Y, 0, 0, 0, 0), (Y, 1, 63, 0, 0), (Y, 5, 9, 0, 0)], 1, "scan 2"),
    "a refinement of a position no scan has coded": ([(Y, 0, 0, 0, 0), (Y, 1, 5, 0, 1), (Y, 1, 63, 1, 0)], 1, "scan 2"),
    "Ah is not the last Al": ([(Y, 0, 0, 0, 0), (Y, 1, 63, 0, 2), (Y, 1, 63, 1, 0)], 1, "scan 2"),
    "Al is not Ah - 1": ([(Y, 0, 0, 0, 0), (Y, 1, 63, 0, 2), (Y, 1, 63, 2, 0)], 1, "scan 2"),
    "a refinement as the first scan": ([(Y, 0, 0, 1, 0)], 1, "scan 0"),
    "a position left at Al 1": ([(Y, 0, 0, 0, 0), (Y, 1, 63, 0, 1)], 1, "position 1"),
    "the DC left at Al 1": ([(Y, 0, 0, 0, 1), (Y, 1, 63, 0, 0)], 1, "position 0"),
    "a position no scan codes": ([(Y, 0, 0, 0, 0), (Y, 1, 62, 0, 0)], 1, "position 63"),
    "a component no scan codes": ([(Y, 0, 0, 0, 0), (Y, 1, 63, 0, 0)], 3, "component 1"),
    "an interleaved AC scan": ([(ALL, 0, 0, 0, 0), (ALL, 1, 63, 0, 0)], 3, "scan 1"),
    "two of three components": ([((0, 1), 0, 0, 0, 0)], 3, "scan 0"),
    "components out of order": ([((0, 2, 1), 0, 0, 0, 0)], 3, "scan 0"),
    "a component that is not there": ([((1,), 0, 0, 0, 0)], 1, "scan 0"),
    "no component": ([((), 0, 0, 0, 0)], 1, "scan 0"),
    "a band that mixes DC and AC": ([(Y, 0, 5, 0, 0)], 1, "scan 0"),
    "Ss > Se": ([(Y, 0, 0, 0, 0), (Y, 9, 5, 0, 0)], 1, "scan 1"),
    "Se 64": ([(Y, 0, 0, 0, 0), (Y, 1, 64, 0, 0)], 1, "scan 1"),
    "Al 14": ([(Y, 0, 0, 0, 14)], 1, "scan 0"),
    "Al negative": ([(Y, 0, 0, 0, -1)], 1, "scan 0"),
    "Ah negative": ([(Y, 0, 0, -1, 0)], 1, "scan 0"),
    "a fraction": ([(Y, 0, 0, 0, 0), (Y, 1, 62.5, 0, 0)], 1, "script"),
    "four fields": ([(Y, 0, 0, 0)], 1, "script"),
    "no list": (7, 1, "script"),
    "an empty script": ([], 1, "script"),
}


@pytest.mark.parametrize("name", list(BAD_SCRIPTS))
def test_check_script_refuses(name):
    script, nc, where = BAD_SCRIPTS[name]
    with pytest.raises(ValueError, match=where):
        P.check_script(script, nc)


def test_check_script_accepts_what_it_should():
    ok = [(Y, 0, 0, 0, 2), (Y, 1, 63, 0, 3), (Y, 0, 0, 2, 1), (Y, 1, 10, 3, 2), (Y, 11, 63, 3, 2), (Y, 1, 63, 2, 1), (Y, 0, 0, 1, 0), (Y, 1, 63, 1, 0)]
    assert P.check_script(ok, 1) == ok
    assert P.check_script([[[0], 0, 0, 0, 0], [[0], 1, 63, 0, 0]], 1) == [(Y, 0, 0, 0, 0), (Y, 1, 63, 0, 0)]
    assert P.bands_script(P.check_bands(None, 3), 3, True) == P.check_script(P.bands_script(P.check_bands(None, 3), 3, True), 3)
    assert P.bands_script(P.check_bands(None, 1), 1, False)[0] == (Y, 0, 0, 0, 0)


def test_the_entry_points_refuse_a_script_before_any_device_work(monkeypatch):
    from simd_dct_amd import jpeg_decode as D
    from simd_dct_amd import jpeg_encode as J

    def no_device(*a, **k):
        raise AssertionError("device work before the arguments were checked")

    monkeypatch.setattr(D, "decode_coefficients", no_device)
    monkeypatch.setattr(P, "encode", no_device)
    monkeypatch.setattr(J, "to_planes", no_device)
    q = [16] * 64
    args = dict(coefs=[None] * 3, qtables=[q] * 3, width=16, height=16, sampling=[(2, 2), (1, 1), (1, 1)])
    img = np.zeros((8, 8), dtype=np.uint8)
    base = golden("c420_17x9.base.jpg")
    with pytest.raises(ValueError, match="script: only with progressive=True"):
        TC.encode_coefficients(**args, script="standard")
    with pytest.raises(ValueError, match="script: only with progressive=True"):
        TC.transcode_jpeg(base, script="standard")
    with pytest.raises(ValueError, match="script: only with progressive=True"):
        J.encode_jpeg(img, script="standard")
    with pytest.raises(ValueError, match="script and bands"):
        TC.encode_coefficients(**args, progressive=True, script="standard", bands=[[(1, 63)]] * 3)
    for bad in ("libjpeg", 5, [(Y, 1, 63, 0, 0)]):
        with pytest.raises(ValueError, match="script|scan 0"):
            TC.encode_coefficients(**args, progressive=True, script=bad)
        with pytest.raises(ValueError, match="script|scan 0"):
            J.encode_jpeg(img, progressive=True, script=bad)
    with pytest.raises(ValueError, match="all three components"):
        TC.encode_coefficients(**dict(args, sampling=[(4, 1), (1, 1), (1, 1)], width=32), progressive=True, script="standard")


def test_cabi_refuses_ah_and_al_on_the_host():
    lib = _jpegprog_lib.load()
    A, OUT, SB, FF, UN, LO, HI = 1 << 40, 1 << 44, 1 << 45, 1 << 46, 1 << 47, 1 << 48, 1 << 49  # nothing is dereferenced
    err = lambda: lib.mdct_jpegprog_last_error().decode()  # noqa: E731
    stride = int(_jpegenc_opt_lib.load().mdct_jpegenc_opt_seg_stride(8))
    one = _jpegcoef_lib.Plane(A, 64, 8, 4, 1, 1)
    arr = (_jpegcoef_lib.Plane * 1)(one)
    for ah, al, said in ((0, 14, "Al 14"), (0, -1, "Al -1"), (1, 1, "Ah 1 with Al 1"), (3, 1, "Ah 3 with Al 1"), (-1, 0, "Ah -1"), (2, 0, "Ah 2 with Al 0"), (14, 13, None),
                         (15, 14, "Al 14")):
        rcs = [lib.mdct_jpegprog_dc_stats_approx(arr, 1, 0, 0, ah, al, HI, LO, None),
               lib.mdct_jpegprog_dc_rows_approx(arr, 1, 0, None, ah, al, 0, 4, OUT, stride, SB, FF, UN, LO, None) if said else 1,
               lib.mdct_jpegprog_ac_stats_approx(one, 1, 63, ah, al, HI, LO, None) if said else 1,
               lib.mdct_jpegprog_ac_rows_approx(one, 1, 63, ah, al, 0, 4, None, OUT, stride, SB, FF, UN, LO, None) if said else 1]
        assert rcs == [1, 1, 1, 1], (ah, al, rcs)
    # (14, 13) is legal; the statistics of a DC refinement scan are not: it has no symbols
    assert lib.mdct_jpegprog_dc_stats_approx(arr, 1, 0, 0, 1, 0, HI, LO, None) == 1 and "no symbols" in err()
    assert lib.mdct_jpegprog_ac_rows_approx(one, 1, 63, 0, 14, 0, 4, None, OUT, stride, SB, FF, UN, LO, None) == 1 and "Al 14" in err()
    assert lib.mdct_jpegprog_ac_stats_approx(one, 1, 63, 3, 1, HI, LO, None) == 1 and "Ah 3 with Al 1" in err()
    # a first scan still needs its tables, whatever Al
    assert lib.mdct_jpegprog_dc_rows_approx(arr, 1, 0, None, 0, 1, 0, 4, OUT, stride, SB, FF, UN, LO, None) == 1 and "null" in err()
    assert lib.mdct_jpegprog_ac_rows_approx(one, 1, 63, 2, 1, 0, 4, None, OUT, stride, SB, FF, UN, LO, None) == 1 and "AC specification" in err()


def test_write_progressive_jpeg_is_unchanged_without_ah_al_and_writes_them_when_given():
    body = lambda k, n: bytes((i * k + 7) % 251 for i in range(n))  # noqa: E731
    q = [1 + (i * 3) % 200 for i in range(64)]
    dc, ac = E.ANNEX_K[(0, 0)], E.ANNEX_K[(1, 0)]
    scans = [dict(components=[(0, 0, 0)], ss=0, se=0, restart_interval=3, tables={(0, 0): dc}, scan=body(3, 40)),
             dict(components=[(0, 0, 0)], ss=1, se=63, restart_interval=3, tables={(1, 0): ac}, scan=body(5, 50))]
    plain = jfif.write_progressive_jpeg([q], 20, 12, [(1, 1)], scans)
    # the file of a caller that knows nothing of Ah / Al, byte for byte as it always was: rebuilt here from the layout
    seg = lambda m, p: bytes([0xFF, m]) + struct.pack(">H", len(p) + 2) + p  # noqa: E731
    dht = lambda tc, sp: seg(0xC4, bytes([tc << 4]) + bytes(sp[0]) + bytes(sp[1]))  # noqa: E731
    zz = api.zigzag_table()
    want = (b"\xff\xd8" + seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00") + seg(0xDB, bytes([0]) + bytes(q[zz[k]] for k in range(64)))
            + seg(0xC2, struct.pack(">BHHB", 8, 12, 20, 1) + bytes([1, 0x11, 0]))
            + dht(0, dc) + seg(0xDD, struct.pack(">H", 3)) + seg(0xDA, bytes([1, 1, 0x00, 0, 0, 0])) + body(3, 40)
            + dht(1, ac) + seg(0xDD, struct.pack(">H", 3)) + seg(0xDA, bytes([1, 1, 0x00, 1, 63, 0])) + body(5, 50) + b"\xff\xd9")
    assert plain == want
    assert jfif.write_progressive_jpeg([q], 20, 12, [(1, 1)], [dict(s, ah=0, al=0) for s in scans]) == plain
    full = [dict(scans[0], al=1), dict(scans[1], al=1), dict(scans[0], ah=1, al=0, tables={}), dict(scans[1], ah=1, al=0)]
    _, _, got, _ = PC.parse(jfif.write_progressive_jpeg([q], 20, 12, [(1, 1)], full))
    assert [(g["ss"], g["se"], g["ah"], g["al"]) for g in got] == [(0, 0, 0, 1), (1, 63, 0, 1), (0, 0, 1, 0), (1, 63, 1, 0)]
    assert [g["order"] for g in got] == [[0xC4, 0xDD, 0xDA], [0xC4, 0xDD, 0xDA], [0xDD, 0xDA], [0xC4, 0xDD, 0xDA]], "no DHT in front of the DC refinement scan"
    for bad in (dict(al=14), dict(ah=14), dict(al=-1)):
        with pytest.raises(ValueError, match="scan 0"):
            jfif.write_progressive_jpeg([q], 20, 12, [(1, 1)], [dict(scans[0], **bad)])


# ---- synthetic rows for the refinement coder: one block row each, as (blocks in zig-zag order int16 [n, 64], band, Al)
def _row(n, fill=None):
    z = np.zeros((n, 64), dtype=np.int16)
    if fill is not None:
        z[:, 1:] = fill
    return z


def synthetic_rows():
    rows = {}
    # every band coefficient 6 under Al = 1: a = 3, every block 63 correction bits and no symbol; the 937-bit rule fires every 15 blocks
    rows["all correction bits, 300"] = (_row(300, 6), (1, 63), 1)
    z = _row(300, 6)
    z[256, 17], z[257, 40] = 2, -3  # a = 1: one new coefficient each, just behind the chunk seam
    rows["all correction bits, new coefficients at 256 and 257"] = (z, (1, 63), 1)
    # a run that stays open over two whole chunks: 600 empty blocks with few bits, a new coefficient in block 599
    z = _row(600)
    z[::7, 9], z[599, 3] = 5, 2
    rows["a run open over two chunks"] = (z, (1, 63), 1)
    # ZRL with buffered correction bits, r > 15 in front of EOB and behind it
    z = _row(5)
    z[1, 2], z[1, 20], z[1, 24], z[1, 60] = 7, 4, -2, 2    # 17 zeros, a bit, 3 zeros ... : ZRLs in front of 24 and of 60
    z[2, 1], z[2, 40], z[2, 41] = 2, 6, 1                   # 38 zeros between 1 and 40: two ZRLs in front of the bit at 40
    z[3, 5], z[3, 30], z[3, 63] = 3, 2, 5                   # r > 15 behind EOB: no ZRL, the bit at 63 is tail
    rows["ZRL with buffered bits"] = (z, (1, 63), 1)
    for n in (1, 3, 255, 256, 257, 300):
        rng = np.random.default_rng(n)
        z = (rng.integers(-9, 10, (n, 64)) * (rng.random((n, 64)) < 0.2)).astype(np.int16)
        rows[f"random, {n} blocks"] = (z, (1, 63), 1)
    rng = np.random.default_rng(5)
    z = (rng.integers(-40, 41, (257, 64)) * (rng.random((257, 64)) < 0.4)).astype(np.int16)
    rows["band (1, 1)"] = (z, (1, 1), 1)
    rows["band (63, 63)"] = (z, (63, 63), 2)
    rows["Al 0"] = (z, (1, 63), 0)
    rows["band (6, 63), Al 2"] = (z, (6, 63), 2)
    z = (rng.integers(-1, 2, (70, 64)).astype(np.int32) << 13).astype(np.int16)  # bit 13 is the one Al = 13 refines
    z[:, 5] = 16383
    rows["Al 13"] = (z, (1, 63), 13)
    z = _row(40)
    z[3, 1], z[4, 1], z[5, 2], z[6, 2], z[7, 3], z[8, 3] = 1023, -1023, 1024, -1024, 2047, -32768  # clamped to +-1023 first: bit 0 is 1
    rows["the clamp"] = (z, (1, 63), 0)
    return rows


def full_run_row():
    """32 800 blocks whose band (1, 1) is empty but for a new coefficient in the last one: the run reaches 0x7FFF on the way"""
    z = _row(32800)
    z[32799, 1] = 2
    return z, (1, 1), 1


def row_plane(z):
    """blocks in zig-zag order [n, 64] -> one block row as a plane int16 [8, 8 n]"""
    nat = np.zeros_like(z)
    nat[:, E.ZZ] = z
    return np.ascontiguousarray(nat.reshape(-1, 8, 8).transpose(1, 0, 2).reshape(8, -1))


def row_units(z):
    return [(0, b.astype(np.int64)) for b in z]


def test_the_synthetic_rows_reach_both_flush_rules_and_the_clamp():
    rows = synthetic_rows()
    z, (ss, se), al = rows["all correction bits, 300"]
    r = AE.ac_refine(row_units(z), len(z), ss, se, al)
    assert r["bit_flushes"] == 300 // 15 and r["max_buffered"] == 15 * 63 and r["full_run_flushes"] == 0
    assert {s: int(c) for s, c in enumerate(r["counts"]) if c} == {0x30: 20}, "20 runs of 15 blocks: EOB3 each"
    z, (ss, se), al = rows["all correction bits, new coefficients at 256 and 257"]
    r = AE.ac_refine(row_units(z), len(z), ss, se, al)
    assert r["bit_flushes"] > 0 and int(sum(r["counts"][s] for s in range(256) if s & 15 == 1)) == 2
    z, (ss, se), al = full_run_row()
    r = AE.ac_refine(row_units(z), len(z), ss, se, al)
    assert r["full_run_flushes"] == 1 and int(r["counts"][0xE0]) == 1 and r["bit_flushes"] == 0
    z, (ss, se), al = rows["a run open over two chunks"]
    r = AE.ac_refine(row_units(z), len(z), ss, se, al)
    assert int(r["counts"][0x90]) == 1 and r["bit_flushes"] == 0, "one run of 599 blocks, flushed by block 599"
    z, (ss, se), al = rows["ZRL with buffered bits"]
    assert int(AE.ac_refine(row_units(z), len(z), ss, se, al)["counts"][0xF0]) == 4
    z, (ss, se), al = rows["the clamp"]
    assert AE.ac_first(row_units(z), len(z), ss, se, al)["lost"] == 4 and AE.ac_refine(row_units(z), len(z), ss, se, al)["lost"] == 0


# ------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    torch.cuda.set_device(0)
    api.init(0)
    return torch


def _hist_with_canaries(torch, shape):
    n = int(np.prod(shape))
    h = torch.full((n + 16,), -5, dtype=torch.int32, device="cuda")
    return h, h[8:8 + n].view(*shape)


def _guards_hold(h, n):
    g = h.cpu().numpy()
    return bool(np.all(g[:8] == -5) and np.all(g[8 + n:] == -5))


def approx_check(torch, planes, frame, comps, ss, se, ah, al, specs=None, rows=None, pad=0, extra=0, want_lost=None):
    """one scan over `comps` of `frame`, an interval per row of its grid: histogram, segments, byte and 0xFF counts, loss and uncoded
    counts against the serial encoder, with canaries.  specs: as encode_scan takes them; None: made from the counts -> the encoder's result"""
    from test_jpeg_progressive import _coded, _compare, dev
    units, upm, gx = AE.scan_units(frame, comps, planes)
    per = gx * upm
    n_rows = len(units) // per
    count = AE.encode_scan(units, per, ss, se, ah, al)
    if specs is None and not (ss == 0 and ah):
        specs = {cls: T.optimal_table(count["counts"][cls, :16]) for cls in range(2 if len(comps) == 3 else 1)} if ss == 0 else T.optimal_table(count["counts"])
    want = AE.encode_scan(units, per, ss, se, ah, al, specs)
    samp = [frame["comps"][ci] for ci in comps]
    grids = None if len(comps) == 3 else [PE.own_grid(frame, comps[0])]
    d = [dev(torch, planes[ci], pad) for ci in comps]
    if ss == 0 and not ah:
        raw, hist = _hist_with_canaries(torch, (2, P.HIST_CLASS))
        cls = min(comps[0], 1)
        _, lo = P.prog_dc_histogram(d, samp, interleaved=len(comps) == 3, cls=cls, grids=grids, hist=hist, al=al)
        got = hist.cpu().numpy().astype(np.int64)
        ref = want["counts"] if len(comps) == 3 or cls == 0 else want["counts"][::-1]
        assert np.array_equal(got, ref) and _guards_hold(raw, 2 * P.HIST_CLASS) and int(lo.item()) == want["lost"]
    elif ss != 0:
        raw, hist = _hist_with_canaries(torch, (P.AC_HIST,))
        _, lo = P.prog_ac_histogram(d[0], ss, se, grid=grids[0], hist=hist, ah=ah, al=al)
        got = hist.cpu().numpy().astype(np.int64)
        assert np.array_equal(got, want["counts"]), ("histogram", {hex(s): (int(a), int(b)) for s, (a, b) in enumerate(zip(got, want["counts"])) if a != b})
        assert _guards_hold(raw, P.AC_HIST) and int(lo.item()) == want["lost"]
    if want_lost is not None:
        assert want.get("lost", 0) == want_lost
    if ss == 0:
        sp = None if ah else [specs[cls] for cls in sorted(specs)] if len(comps) == 3 else [specs[0] if 0 in specs else specs[1]]
        launch = lambda seg, sb, ff, un, lo, stride, r0, r1: P.prog_dc_rows(d, samp, sp, seg, sb, ff, un, lo, interleaved=len(comps) == 3, grids=grids, seg_stride=stride,  # noqa: E731
                                                                              r0=r0, r1=r1, ah=ah, al=al)
    else:
        launch = lambda seg, sb, ff, un, lo, stride, r0, r1: P.prog_ac_rows(d[0], ss, se, specs, seg, sb, ff, un, lo, grid=grids[0], seg_stride=stride, by0=r0, by1=r1,  # noqa: E731
                                                                              ah=ah, al=al)
    got = _coded(torch, n_rows, per, rows, extra, launch)
    _compare(got, want["segs"])
    if rows is None:
        assert got[3] == want.get("uncoded", 0) and got[4] == want.get("lost", 0), (got[3], got[4], want.get("uncoded"), want.get("lost"))
    return want


def grey_frame(plane):
    return dict(width=plane.shape[1], height=plane.shape[0], comps=[(1, 1)])


@pytest.mark.gpu
@pytest.mark.parametrize("picture", PICTURES)
def test_every_scan_of_a_golden_file_from_the_checkers_planes(gpu, picture):
    """the file's own tables; the packed scan equals the file's entropy-coded bytes, the histogram the encoder's counts"""
    from test_jpeg_progressive import dev
    torch = gpu
    data, frame, planes, scans = checker_scans(picture + ".prog.jpg")
    for k, (sc, per, r) in enumerate(scans):
        comps = [ci for ci, _, _ in sc["comps"]]
        want = approx_check(torch, planes, frame, comps, sc["ss"], sc["se"], sc["ah"], sc["al"], specs=scan_specs(sc))
        assert AE.scan_data(want["segs"]) == data[sc["start"]:sc["end"]], (picture, k)
        if "counts" in r:
            assert np.array_equal(want["counts"], r["counts"])
        # and through the packing launch, as encode runs it
        units, upm, gx = AE.scan_units(frame, comps, planes)
        n_rows, blocks = len(units) // (gx * upm), gx * upm
        stride = TC.opt_seg_stride(blocks)
        seg = torch.empty((n_rows * stride,), dtype=torch.uint8, device="cuda")
        counts = torch.empty((2, n_rows), dtype=torch.int32, device="cuda")
        words = torch.zeros((2,), dtype=torch.int32, device="cuda")
        d = [dev(torch, planes[ci]) for ci in comps]
        samp = [frame["comps"][ci] for ci in comps]
        grids = None if len(comps) == 3 else [PE.own_grid(frame, comps[0])]
        specs = scan_specs(sc)
        if sc["ss"] == 0:
            sp = None if sc["ah"] else [specs[cls] for cls in sorted(specs)]
            P.prog_dc_rows(d, samp, sp, seg, counts[0], counts[1], words[0:1], words[1:2], interleaved=len(comps) == 3, grids=grids, seg_stride=stride, ah=sc["ah"], al=sc["al"])
        else:
            P.prog_ac_rows(d[0], sc["ss"], sc["se"], specs, seg, counts[0], counts[1], words[0:1], words[1:2], grid=grids[0], seg_stride=stride, ah=sc["ah"], al=sc["al"])
        out, off = TC._pack(torch, seg, counts, stride, n_rows, n_rows * blocks * 64, torch.device("cuda"), None)
        assert out[:int(off[-1].item())].cpu().numpy().tobytes() == data[sc["start"]:sc["end"]], (picture, k, "packed")
        assert words.cpu().tolist() == [0, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("picture", PICTURES)
def test_transcode_with_the_standard_script_reproduces_the_golden_twin(gpu, picture):
    """scan by scan the header fields, DRI, DHT contents and entropy-coded bytes of libjpeg's file; and the file reads back"""
    from simd_dct_amd import jpeg_decode as D
    base, gold = golden(picture + ".base.jpg"), golden(picture + ".prog.jpg")
    api.kernel_counts_reset()
    out = TC.transcode_jpeg(base, progressive=True, script="standard")
    ran = api.kernel_counts()
    wf, want = parsed(gold)
    gf, got = parsed(out)
    assert gf == wf and len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert ([c[0] for c in g["comps"]], g["ss"], g["se"], g["ah"], g["al"], g["dri"]) == ([c[0] for c in w["comps"]], w["ss"], w["se"], w["ah"], w["al"], w["dri"]), k
        if w["ss"] == 0 and not w["ah"]:
            assert [spec_lists(g["raw"][(0, td)]) for _, td, _ in g["comps"]] == [spec_lists(w["raw"][(0, td)]) for _, td, _ in w["comps"]], (k, "DC tables")
        elif w["ss"] != 0:
            assert spec_lists(g["raw"][(1, g["comps"][0][2])]) == spec_lists(w["raw"][(1, w["comps"][0][2])]), (k, "AC table")
        assert g["order"] == ([0xDD, 0xDA] if w["ss"] == 0 and w["ah"] else [0xC4, 0xDD, 0xDA]), (k, "no DHT in front of a DC refinement scan")
        assert out[g["start"]:g["end"]] == gold[w["start"]:w["end"]], (picture, k, "entropy-coded bytes")
    # the launch tally: a statistics and a coding launch per Huffman scan, one launch per DC refinement scan
    nc = len(wf["comps"])
    n_ac = sum(1 for w in want if w["ss"] != 0)
    hv = "0, 0" if nc == 1 else {(1, 1): "1, 1", (2, 1): "2, 1", (2, 2): "2, 2"}[wf["comps"][0]]
    assert ran.get("k_prog_ac<true>", 0) == n_ac and ran.get("k_prog_ac<false>", 0) == n_ac
    assert ran.get(f"k_prog_dc<{hv}, true>", 0) == 1 and ran.get(f"k_prog_dc<{hv}, false>", 0) == 2
    assert sum(v for k, v in ran.items() if k.startswith("k_prog_")) == 2 * n_ac + 3
    # read back: the engine's decoder and the serial checker return the input's planes
    _, src = D.decode_coefficients(base)
    _, back = D.decode_coefficients(out)
    planes, statuses = AC.decode(out)
    assert all(s == AC.OK for st in statuses for s in st)
    for ci, (a, b, c) in enumerate(zip(src, back, planes)):
        gx, gy = PE.own_grid(wf, ci)
        a, b = a.cpu().numpy(), b.cpu().numpy()
        assert np.array_equal(a[:gy * 8, :gx * 8], b[:gy * 8, :gx * 8]) and np.array_equal(a[::8, ::8], b[::8, ::8]), (picture, ci, "decode_coefficients")
        assert np.array_equal(b, c), (picture, ci, "the serial checker")


@pytest.mark.gpu
@pytest.mark.parametrize("shape,subsampling", [((45, 83, 3), "4:2:0"), ((24, 40, 3), "4:4:4"), ((35, 50, 3), "4:2:2"), ((20, 27), None)])
def test_encode_jpeg_with_the_standard_script_decodes_to_its_baseline_twin(gpu, shape, subsampling):
    from simd_dct_amd import jpeg_decode as D
    from simd_dct_amd import jpeg_encode as J
    rng = np.random.default_rng(shape[0])
    yy, xx = np.mgrid[:shape[0], :shape[1]]
    img = (128 + 90 * np.sin(xx / 7.0) * np.cos(yy / 5.0))[..., None] + rng.integers(-30, 31, shape[:2] + (3,))
    img = np.clip(img, 0, 255).astype(np.uint8)
    img = img if len(shape) == 3 else np.ascontiguousarray(img[..., 0])
    kw = dict(quality=90) if subsampling is None else dict(quality=90, subsampling=subsampling)
    prog = J.encode_jpeg(img, progressive=True, script="standard", **kw)
    base = J.encode_jpeg(img, optimize=True, **kw)
    frame, scans = parsed(prog)
    nc = len(frame["comps"])
    assert [(tuple(c[0] for c in s["comps"]), s["ss"], s["se"], s["ah"], s["al"]) for s in scans] == P.standard_script(nc)
    a, b = D.decode_jpeg(base), D.decode_jpeg(prog)
    for x, y in zip(a if isinstance(a, (list, tuple)) else [a], b if isinstance(b, (list, tuple)) else [b]):
        assert gpu.equal(x, y)
    planes, statuses = AC.decode(prog)
    assert all(s == AC.OK for st in statuses for s in st)
    # script=None is the file it always was, and a script given as a list is the same file as its name
    assert J.encode_jpeg(img, progressive=True, **kw) == J.encode_jpeg(img, progressive=True, script=None, **kw)
    assert J.encode_jpeg(img, progressive=True, script=P.standard_script(nc), **kw) == prog
    try:
        from PIL import Image
    except ImportError:
        return
    pa, pb = Image.open(io.BytesIO(base)), Image.open(io.BytesIO(prog))
    assert pb.info.get("progressive") and np.array_equal(np.asarray(pa), np.asarray(pb))


@pytest.mark.gpu
def test_encode_coefficients_with_a_script_of_its_own(gpu):
    """a script that is not libjpeg's: DC refined twice, chroma without successive approximation, interleaved and single DC scans"""
    from simd_dct_amd import jpeg_decode as D
    torch = gpu
    frame = dict(width=83, height=45, comps=[(2, 2), (1, 1), (1, 1)])
    rng = np.random.default_rng(11)
    planes = []
    for (r, c), (gx, gy) in zip(E.plane_shapes(frame), (PE.own_grid(frame, ci) for ci in range(3))):
        p = (rng.integers(-60, 61, (r, c)) * (rng.random((r, c)) < 0.2)).astype(np.int16)
        p[::8, ::8] = rng.integers(-300, 301, (r // 8, c // 8))
        dc = p[::8, ::8].copy()
        # a single-component DC refinement covers the component's own grid only: beyond it, bit 1 is one no scan of this script codes
        dc[gy:] &= ~2
        dc[:, gx:] &= ~2
        p[gy * 8:], p[:, gx * 8:] = 0, 0
        p[::8, ::8] = dc
        planes.append(p)
    script = [(ALL, 0, 0, 0, 2), ((0,), 1, 63, 0, 1), ((1,), 1, 63, 0, 0), ((2,), 1, 9, 0, 0), ((2,), 10, 63, 0, 0), ((0,), 0, 0, 2, 1), ((1,), 0, 0, 2, 1), ((2,), 0, 0, 2, 1),
              (ALL, 0, 0, 1, 0), ((0,), 1, 63, 1, 0)]
    q = [[3] * 64, [5] * 64, [5] * 64]
    out = TC.encode_coefficients([torch.from_numpy(p).cuda() for p in planes], q, 83, 45, frame["comps"], progressive=True, script=script)
    _, scans = parsed(out)
    assert [(tuple(c[0] for c in s["comps"]), s["ss"], s["se"], s["ah"], s["al"]) for s in scans] == script
    got, statuses = AC.decode(out)
    assert all(s == AC.OK for st in statuses for s in st)
    for g, p in zip(got, planes):
        assert np.array_equal(g, p)
    _, back = D.decode_coefficients(out)
    for g, b in zip(got, back):
        assert np.array_equal(b.cpu().numpy(), g)


ROWS = synthetic_rows()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ROWS))
def test_refinement_rows_against_the_serial_encoder(gpu, name):
    z, (ss, se), al = ROWS[name]
    plane = row_plane(z)
    approx_check(gpu, [plane], grey_frame(plane), [0], ss, se, al + 1, al)
    # the same row as a first scan with the point transform (Al 0: the parent's path through the new call)
    approx_check(gpu, [plane], grey_frame(plane), [0], ss, se, 0, al, want_lost=4 if name == "the clamp" else None)
    if name == "the clamp":
        approx_check(gpu, [plane], grey_frame(plane), [0], ss, se, 0, 1, want_lost=4)
        approx_check(gpu, [plane], grey_frame(plane), [0], ss, se, 2, 1, want_lost=0)


@pytest.mark.gpu
def test_a_plane_three_blocks_wide_of_four(gpu):
    """blocks_x 3 in a 4-wide plane: the grid leaves the last block column out"""
    rng = np.random.default_rng(2)
    p = (rng.integers(-9, 10, (16, 32)) * (rng.random((16, 32)) < 0.3)).astype(np.int16)
    q = p.copy()
    q[:, 24:] = 0
    from test_jpeg_progressive import _coded, _compare, dev
    units = [(0, b) for b in PE.zz_blocks(q, 3, 2).reshape(-1, 64)]
    for ah, al in ((2, 1), (0, 1), (1, 0)):
        count = AE.encode_scan(units, 3, 1, 63, ah, al)
        spec = T.optimal_table(count["counts"])
        want = AE.encode_scan(units, 3, 1, 63, ah, al, spec)
        d = dev(gpu, p)
        hist, _ = P.prog_ac_histogram(d, 1, 63, grid=(3, 2), ah=ah, al=al)
        assert np.array_equal(hist.cpu().numpy().astype(np.int64), want["counts"])
        got = _coded(gpu, 2, 3, None, 0, lambda seg, sb, ff, un, lo, stride, r0, r1: P.prog_ac_rows(d, 1, 63, spec, seg, sb, ff, un, lo, grid=(3, 2), seg_stride=stride, by0=r0,
                                                                                                      by1=r1, ah=ah, al=al))
        _compare(got, want["segs"])


@pytest.mark.gpu
def test_the_full_run_of_a_refinement_scan(gpu):
    z, (ss, se), al = full_run_row()
    plane = row_plane(z)
    want = approx_check(gpu, [plane], grey_frame(plane), [0], ss, se, al + 1, al)
    assert want["full_run_flushes"] == 1


def dense_blocks(rng, n):
    """n blocks whose refinement scan under Al = 1 is long: every even zig-zag position a new coefficient (+-2, a zero in front of each:
    mostly symbol 0x11, 16 bits in LONG_AC), a quarter of the odd positions a correction bit (+-6)"""
    z = np.zeros((n, 64), dtype=np.int16)
    z[:, 2::2] = 2 * rng.choice(np.array([-1, 1]), (n, 31))
    z[:, 1::2] = 6 * rng.choice(np.array([-1, 1]), (n, 32)) * (rng.random((n, 32)) < 0.25)
    return z


def window_rows():
    """rows whose chunks need several windows of the coder's 1024-word ring (with LONG_AC, band (1, 63), Al = 1)"""
    rng = np.random.default_rng(11)
    dense = dense_blocks(rng, 257)
    # 246 empty blocks and ten of 63 correction bits each leave a run of 256 open across the chunk seam with 630 buffered bits:
    # lane 0 of the second chunk emits EOB8 and the buffer in front of a chunk of several windows
    open_run = _row(256)
    open_run[246:, 1:] = 6
    return {"dense": dense, "open run": np.concatenate([open_run, dense_blocks(rng, 257)])}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["dense", "open run"])
def test_refinement_chunks_of_several_ring_windows(gpu, name):
    """the refinement coder's window loop, which the rows above (optimal tables) never enter: the chunk of the row's first (dense) or
    second (open run) 256 blocks holds more than three windows' bytes, as a refinement scan and as a first scan with the point
    transform.  The serial encoder gives 13,978 / 18,168 bytes (dense: refinement / first) and 14,134 / 19,469 (open run)."""
    from test_jpeg_progressive import LONG_AC
    z = window_rows()[name]
    plane = row_plane(z)
    dense = z[-257:]
    for ah in (2, 0):
        first256 = AE.encode_scan(row_units(dense[:256]), 256, 1, 63, ah, 1, LONG_AC)
        assert len(first256["segs"][0]) > 3 * 4096, "at least four windows of 1024 words"
        want = approx_check(gpu, [plane], grey_frame(plane), [0], 1, 63, ah, 1, specs=LONG_AC)
        assert want["uncoded"] == 0 and want["lost"] == 0
        if name == "open run" and ah:
            assert want["max_buffered"] == 630 and want["bit_flushes"] == 0 and want["full_run_flushes"] == 0
            assert int(want["counts"][0x80]) == 1 and int(want["counts"][0x00]) == 257, "EOB8 for the open run, then a run of one per dense block"
            assert len(want["segs"][0]) == 14134


@pytest.mark.gpu
def test_sub_ranges_and_pitch_of_refinement_scans(gpu):
    """rows by0..by1 of a call equal the same rows of a full call (both are held to the encoder's), with a pitch wider than the
    plane and a stride wider than needed; the DC refinement scan in both forms"""
    rng = np.random.default_rng(9)
    p = (rng.integers(-20, 21, (40, 300 * 8)) * (rng.random((40, 300 * 8)) < 0.15)).astype(np.int16)
    p[16:24] = row_plane(ROWS["all correction bits, new coefficients at 256 and 257"][0])
    f = grey_frame(p)
    for rows in (None, (1, 4), (2, 3), (4, 5)):
        approx_check(gpu, [p], f, [0], 1, 63, 2, 1, rows=rows, pad=0 if rows is None else 2, extra=0 if rows is None else 8)
        approx_check(gpu, [p], f, [0], 0, 0, 1, 0, rows=rows, pad=0 if rows is None else 1, extra=0 if rows is None else 4)
        approx_check(gpu, [p], f, [0], 0, 0, 0, 1, rows=rows)
    for name, samp in (("4:2:0", [(2, 2), (1, 1), (1, 1)]), ("4:2:2", [(2, 1), (1, 1), (1, 1)]), ("4:4:4", [(1, 1)] * 3)):
        frame = dict(width=33 * 8 * samp[0][0] - 3, height=3 * 8 * samp[0][1], comps=samp)
        planes = [rng.integers(-1024, 1024, s).astype(np.int16) for s in E.plane_shapes(frame)]
        for rows in (None, (1, 3)):
            approx_check(gpu, planes, frame, [0, 1, 2], 0, 0, 1, 0, rows=rows, pad=1)
            approx_check(gpu, planes, frame, [0, 1, 2], 0, 0, 2, 1, rows=rows)
            approx_check(gpu, planes, frame, [0, 1, 2], 0, 0, 0, 1, rows=rows)
        approx_check(gpu, planes, frame, [1], 0, 0, 1, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("arrangement,fill", [("A", 0x7F7F7F7F), ("B", None)], ids=["A-stale-7f", "B"])
def test_the_standard_script_on_a_stream_that_is_not_the_current_one(gpu, arrangement, fill):
    """arrangements A and B of tests/test_jpeg_streams.py on transcode_jpeg(script='standard')"""
    import test_jpeg_streams as S
    name = "transcode-standard-script"
    if name not in S.CASES:
        base = golden("noisy_203x117_q90.base.jpg")
        gold = golden("noisy_203x117_q90.prog.jpg")

        def check(truth):
            assert truth[0] == "ok" and [truth[1][s["start"]:s["end"]] for s in parsed(truth[1])[1]] == [gold[s["start"]:s["end"]] for s in parsed(gold)[1]]

        S.CASES[name] = S.Case(name, lambda torch: lambda st: TC.transcode_jpeg(base, progressive=True, script="standard", stream=st), tally=("k_prog_ac<false>", 8), check=check)
    S.run(gpu, name, arrangement, fill=fill)
