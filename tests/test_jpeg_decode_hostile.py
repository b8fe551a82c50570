"""Both GPU JPEG decoders, and the file reader in front of them, on input that is wrong: every error class at every hand-off.

The cases are tests/jpeg_hostile_cases.py: scans written by the test-side encoder from known planes with one wrong thing at a chosen
place, each with a legal twin.  CPU: the checker gives every case the class it is named for and the expected number of complete
blocks, every twin is OK and equals its planes, libjpeg (Pillow) opens the twins, three mutants of the checker each fail a named case;
jfif.read_jpeg reaches every one of its refusals and never raises anything else on prefixes and mutated headers.  GPU: status, complete
blocks, the failing block, zeros after it, guards, twins, on the path each case belongs to; decode_jpeg's exceptions; a captured decode.

The rule after an error (include/mdct_jpegdec.h, include/mdct_jpegdec_unmarked.h): the blocks before the failing one are exact, the
failing block holds the levels decoded before the error and zeros, every block after it in the interval / scan is zero."""
import importlib.util
import io
import os
import struct

import numpy as np
import pytest

import jpeg_decode_checker as C
import jpeg_hostile_cases as HC
import jpeg_scan_encoder as E
import oracle as O
from simd_dct_amd import api, jfif

Image = pytest.importorskip("PIL.Image")
from test_jpeg_decode import _libjpeg_luma  # noqa: E402

NOT_SYNCHRONISED = 6
IDS = HC.case_ids()
NAMES = [HC.case_name(*i) for i in IDS]
DECODER_KERNELS = {"k_decode", "k_rst_scan", "k_rst_walk<false>", "k_rst_walk<true>", "k_um_zero", "k_um_sync", "k_um_round", "k_um_prefix",
                   "k_um_write", "k_um_final"}


def _file(c, scan, planes=None):
    b = HC.base_of(c)
    head, tail = HC.header(b, planes)
    return head + scan + tail


def _expect(c, checker=C):
    """the checker on the hostile scan -> per interval (status, complete blocks, failing block, n)"""
    return HC.check_scan(HC.base_of(c), c.scan) if checker is C else _check_with(checker, c, c.scan)


def _check_with(mod, c, scan):
    b = HC.base_of(c)
    n = b["n_intervals"]
    parts = mod.split_intervals(scan, n) if b["marked"] else [(scan, None)]
    tabs = {key: mod.code_table(*b["specs"][(0 if key[0] == "dc" else 1, [x for x in b["scan"]["comps"] if x[0] == key[1]][0][1 if key[0] == "dc" else 2])])
            for key in HC.tables(b)}
    return [mod.decode_interval(chunk, HC.units(b, k), tabs, None if k == n - 1 else ((mk is not None and mk == k % 8),), partial=True)
            for k, (chunk, mk) in enumerate(parts)]


def _twin_ok(c, scan, planes, checker=C):
    b = HC.base_of(c)
    res = HC.check_scan(b, scan) if checker is C else _check_with(checker, c, scan)
    for k, (st, blocks, failing, n) in enumerate(res):
        if st != C.OK or failing is not None:
            return False
        for (place, blk), (tplace, want) in zip(blocks, HC.truth_blocks(b, planes, k)):
            if place != tplace or not np.array_equal(blk.astype(np.int16), want):
                return False
    return True


# ------------------------------------------------------------------------------------------ CPU: the case list against the checker
@pytest.mark.parametrize("maker,args", IDS, ids=NAMES)
def test_checker_names_the_class_of_every_hostile_case(maker, args):
    c = HC.build(maker, args)
    assert c.check_place()
    res = _expect(c)
    st, blocks, failing, n = res[c.interval]
    assert st == c.klass and n == c.n_before, (st, n, c.klass, c.n_before)
    assert {k: r[0] for k, r in enumerate(res) if r[0] != C.OK and k != c.interval} == c.others
    b = HC.base_of(c)
    for (place, blk), (tplace, want) in zip(blocks, HC.truth_blocks(b, c.twin_planes, c.interval)):
        assert place == tplace and np.array_equal(blk.astype(np.int16), want)
    assert (failing is None) == (c.klass == C.LEFTOVER or c.kind in ("marker-lone-ff-at-end", "marker-wrong-rst-after"))
    assert _twin_ok(c, c.twin, c.twin_planes)
    if hasattr(c, "twin2"):
        assert _twin_ok(c, c.twin2[1], c.twin2[0])


@pytest.mark.parametrize("path", list(HC.PATHS))
def test_injecting_encoder_writes_the_plain_encoders_scan(path):
    """the loop that can replace a symbol and the plain loop (held to Pillow byte for byte) write the same bytes when nothing is
    injected; the intact twins come from the former"""
    for sparse in (False, True) if path.endswith("grey") else (False,):
        b = HC.base(path, sparse)
        plain, st = HC.encode(b)
        traced, st2 = HC.trace(path, sparse)
        assert plain == traced and st["intervals"] == st2["intervals"] and st["stuffed"] == st2["stuffed"] and st["pad_bits"] == st2["pad_bits"]
        assert st["blocks"] == st2["blocks"] == b["n_blocks"]


@pytest.mark.parametrize("path", ["marked-420", "unmarked-420"])
@pytest.mark.parametrize("sign", [1, -1], ids=["up", "down"])
def test_checker_wraps_the_dc_predictor_as_int16(path, sign):
    b, scan, st, truth = HC.make_dc_wrap(path, sign)
    (status, blocks, failing, n), = HC.check_scan(b, scan)
    assert status == C.OK and n == b["n_blocks"]
    assert max(int(abs(blk[0])) for _, blk in blocks) > 32768  # the predictor itself is not confined to 16 bits ...
    for (place, blk), (_, want) in zip(blocks, HC.truth_blocks(b, truth, 0)):
        assert np.array_equal(blk.astype(np.int16), want)  # ... what is stored is its low 16 bits
    assert any(int(blk[0]) != int(np.int16(blk[0])) for _, blk in blocks)


TWIN_KINDS = ["ovf-1s-at-63", "ovf-run15-from-49", "ovf-zrl-at-49", "ovf-four-zrl-from-1"]


def _pillow_agrees(data, planes, W, H):
    got = _libjpeg_luma(data).astype(int)
    want = O.u8_i16("inv", planes[0].astype(np.int16), planes[0].shape[1], planes[0].shape[0], lut=np.ones(64, dtype=np.float32))
    return int(np.abs(want[:H, :W].astype(int) - got).max())


@pytest.mark.parametrize("path", list(HC.PATHS))
def test_libjpeg_opens_the_legal_twins(path):
    """where libjpeg's behaviour is defined: a ZRL that ends the block at 64, a run of 15 onto 63, seven 1-bits of padding, none"""
    W, H = HC.PATHS[path][:2]
    b = HC.base(path)
    place = "y3" if b["upm"] > 1 else "lane-after"
    for kind in TWIN_KINDS:
        c = HC.make(path, kind, place)
        assert _pillow_agrees(_file(c, c.twin, c.twin_planes), c.twin_planes, W, H) <= 1, kind
    c = HC.make_special(path, "left-7-ones-then-ff", "last")
    assert _pillow_agrees(_file(c, c.twin, c.twin_planes), c.twin_planes, W, H) <= 1
    assert _pillow_agrees(_file(c, c.twin2[1], c.twin2[0]), c.twin2[0], W, H) <= 1


MUTANTS = {  # name: (old text, new text, cases one of which the mutant must fail)
    "index-64-allowed": ("        if k > 63:\n", "        if k > 64:\n", [("make", ("marked-grey", "ovf-1s-at-63", "lane-after"))]),
    "zrl-to-64-refused": ("if k + 16 > 64:", "if k + 16 >= 64:", [("make", ("marked-grey", "ovf-zrl-at-49", "lane-after"))]),
    "zero-bit-padding-accepted": ("if len(rem) >= 8 or not all(rem):", "if len(rem) >= 8:",
                                  [("make_special", ("marked-grey", "left-one-0-bit", w)) for w in ("first", "mid", "last")]),
}


def _checker_copy(tmp_path, name, old=None, new=None):
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "jpeg_decode_checker.py")).read()
    if old is not None:
        assert src.count(old) == 1, old
        src = src.replace(old, new)
    f = tmp_path / f"checker_{name.replace('-', '_')}.py"
    f.write_text(src)
    spec = importlib.util.spec_from_file_location(f.stem, str(f))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _passes(mod, c):
    try:
        st, blocks, failing, n = _expect(c, mod)[c.interval]
        return st == c.klass and n == c.n_before and _twin_ok(c, c.twin, c.twin_planes, mod)
    except IndexError:  # a level stored at zig-zag index 64
        return False


def test_unmodified_copy_of_the_checker_passes_the_named_cases(tmp_path):
    mod = _checker_copy(tmp_path, "copy")
    for _, _, cases in MUTANTS.values():
        assert all(_passes(mod, HC.build(*i)) for i in cases)


@pytest.mark.parametrize("name", list(MUTANTS))
def test_mutant_of_the_checker_fails_a_named_case(tmp_path, name):
    old, new, cases = MUTANTS[name]
    mod = _checker_copy(tmp_path, name, old, new)
    assert not all(_passes(mod, HC.build(*i)) for i in cases)


# ------------------------------------------------------------------------------------------ CPU: jfif.read_jpeg
def _small(kind):
    """a small valid file: grey / three-scan / interleaved 4:2:0, with and without DRI"""
    rng = np.random.default_rng(5)
    comps = [(1, 1)] if kind.startswith("grey") else [(2, 2), (1, 1), (1, 1)]
    frame = dict(width=16, height=16, comps=comps)
    dri = 1 if kind.endswith("dri") else 0
    if kind.startswith("grey"):
        scans = [dict(comps=[(0, 0, 0)], dri=dri)]
    elif kind.startswith("three"):
        scans = [dict(comps=[(ci, min(ci, 1), min(ci, 1))], dri=dri) for ci in range(3)]
    else:
        scans = [dict(comps=[(0, 0, 0), (1, 1, 1), (2, 1, 1)], dri=dri)]
    planes = [rng.integers(-3, 4, size=s).astype(np.int16) for s in E.plane_shapes(frame)]
    data, st = E.encode_file(frame, scans, planes, dict(E.ANNEX_K))
    return data, st[0]["start"]


SMALL = ["grey", "grey-dri", "three-scan", "three-scan-dri", "420", "420-dri"]


def _seg_at(data, marker, nth=0):
    """(offset of the marker's 0xFF, offset after the segment) of the nth segment of that kind"""
    i = 2
    while True:
        L = struct.unpack_from(">H", data, i + 2)[0]
        if data[i + 1] == marker:
            if nth == 0:
                return i, i + 2 + L
            nth -= 1
        i += 2 + L


def _edit(data, marker, at, new, nth=0):
    """the byte(s) at payload offset `at` of that segment replaced"""
    i, _ = _seg_at(data, marker, nth)
    return data[:i + 4 + at] + bytes(new) + data[i + 4 + at + len(new):]


def _without(data, marker):
    i, j = _seg_at(data, marker)
    return data[:i] + data[j:]


def _refusals():
    g, _ = _small("grey-dri")
    c, _ = _small("420-dri")
    sof = g[slice(*_seg_at(g, 0xC0))]
    i_sof, j_sof = _seg_at(g, 0xC0)
    i_dht, j_dht = _seg_at(g, 0xC4)
    i_sos, j_sos = _seg_at(g, 0xDA)
    i_dqt, j_dqt = _seg_at(g, 0xDB)
    i_dri, j_dri = _seg_at(g, 0xDD)
    seg = lambda m, p: bytes([0xFF, m]) + struct.pack(">H", len(p) + 2) + p  # noqa: E731
    return [  # (row, file, message, keyword arguments)
        ("no SOI", b"\x00\x00" + g[2:], "no SOI", {}),
        ("an empty file", b"", "no SOI", {}),
        ("no EOI", g[:-2], "runs to the end of the file", {}),
        ("a byte that is no marker after SOI", g[:2] + b"\x00" + g[3:], "expected a marker at offset 2", {}),
        ("the file ends after SOI", g[:2], "expected a marker", {}),
        ("RST outside a scan", g[:2] + b"\xff\xd0" + g[2:], "marker 0xd0 outside", {}),
        ("TEM outside a scan", g[:2] + b"\xff\x01" + g[2:], "marker 0x01 outside", {}),
        ("a marker with no length", g[:2] + b"\xff\xe0\x00", "truncated marker segment", {}),
        ("a segment length past the end of the file", g[:4] + b"\xff\xf0" + g[6:], "truncated segment 0xe0", {}),
        ("a segment length below 2", g[:4] + b"\x00\x01" + g[6:], "truncated segment 0xe0", {}),
        ("SOF2", _edit(g, 0xC0, -3, [0xC2]), "progressive", {}),
        ("DNL", g[:i_sos] + seg(0xDC, b"\x00\x10") + g[i_sos:], "DNL", {}),
        ("a second SOF", g[:j_sof] + sof + g[j_sof:], "a second frame header", {}),
        ("a frame header of 5 bytes", g[:i_sof] + seg(0xC0, b"\x08\x00\x10\x00\x10") + g[j_sof:], "malformed frame header", {}),
        ("12-bit samples", _edit(g, 0xC0, 0, [12]), "12-bit samples", {}),
        ("two components", _edit(g, 0xC0, 5, [2]), "2 components", {}),
        ("zero height", _edit(g, 0xC0, 1, [0, 0]), "height defined by DNL", {}),
        ("zero width", _edit(g, 0xC0, 3, [0, 0]), "malformed frame header", {}),
        ("three components in a one-component header", _edit(g, 0xC0, 5, [3]), "malformed frame header", {}),
        ("sampling factor 3", _edit(g, 0xC0, 7, [0x31]), "sampling 3x1", {}),
        ("quantiser table 4 in SOF", _edit(g, 0xC0, 8, [4]), "table 4", {}),
        ("16-bit DQT", _edit(g, 0xDB, 0, [0x10]), "16-bit DQT", {}),
        ("DQT id out of range", _edit(g, 0xDB, 0, [0x04]), "malformed DQT", {}),
        ("DQT shorter than a table", g[:i_dqt] + seg(0xDB, g[i_dqt + 4:j_dqt - 1]) + g[j_dqt:], "malformed DQT", {}),
        ("DHT class out of range", _edit(g, 0xC4, 0, [0x20]), "Huffman table class 2", {}),
        ("DHT id out of range", _edit(g, 0xC4, 0, [0x02]), "class 0 id 2", {}),
        ("DHT shorter than its counts", g[:i_dht] + seg(0xC4, g[i_dht + 4:i_dht + 14]) + g[j_dht:], "malformed DHT", {}),
        ("DHT counts sum past its payload", _edit(g, 0xC4, 253, [0xFF]), "malformed DHT", {}),
        ("DRI of three bytes", g[:i_dri] + seg(0xDD, b"\x00\x00\x01") + g[j_dri:], "malformed DRI", {}),
        ("SOS before SOF", _without(g, 0xC0), "SOS before the frame header", {}),
        ("SOS with no component", _edit(g, 0xDA, 0, [0]), "malformed SOS", {}),
        ("an empty SOS", g[:i_sos] + seg(0xDA, b"") + g[j_sos:], "malformed SOS", {}),
        ("SOS of the wrong length", g[:i_sos] + seg(0xDA, g[i_sos + 4:j_sos] + b"\x00") + g[j_sos:], "malformed SOS", {}),
        ("SOS names a missing component", _edit(g, 0xDA, 1, [9]), "names component 9", {}),
        ("spectral selection", _edit(g, 0xDA, 3, [1]), "spectral selection", {}),
        ("12 blocks per MCU", _edit(_edit(c, 0xC0, 10, [0x22]), 0xC0, 13, [0x22]), "more than 10 blocks per MCU", {}),
        ("no DRI", _small("grey")[0], "without restart markers", {}),
        ("an unknown marker", g[:2] + seg(0xC8, b"") + g[2:], "marker 0xc8", {}),
        ("no frame", b"\xff\xd8\xff\xd9", "no frame or no scan", {}),
        ("a frame and no scan", g[:i_sos] + b"\xff\xd9", "no frame or no scan", {}),
    ]


REFUSALS = _refusals()


@pytest.mark.parametrize("row,data,message,kw", REFUSALS, ids=[r[0].replace(" ", "-") for r in REFUSALS])
def test_read_jpeg_refusal(row, data, message, kw):
    with pytest.raises(jfif.JpegFormatError, match=message):
        jfif.read_jpeg(data, **kw)


def test_every_refusal_site_of_read_jpeg_has_a_row():
    """every `raise JpegFormatError` of jfif.py is reached by a row above: the text of its message (up to the first substituted
    value; after it where the message begins with one) occurs in what some row raised"""
    import re
    src = open(jfif.__file__).read()
    src = src[src.index("class JpegFormatError"):src.index("def _colorspace")]
    sites = re.findall(r'raise JpegFormatError\(f?"([^"]*)"', src)
    assert len(sites) >= 27
    raised = []
    for _, data, _, kw in REFUSALS:
        with pytest.raises(jfif.JpegFormatError) as e:
            jfif.read_jpeg(data, **kw)
        raised.append(str(e.value))
    for site in sites:
        texts = [t.strip() for t in re.split(r"\{[^}]*\}", site) if len(t.strip()) > 3]
        assert texts and any(all(t in msg for t in texts) for msg in raised), site


def _host_checks(info, data):
    """what decode_jpeg settles on the host before its first launch, by decode_jpeg's own functions (scan_plan, component_luts) over
    planes that are not allocated: one row of zeros seen at every row"""
    import torch
    from simd_dct_amd import jpeg_decode as D
    geo, grid = D.geometry(info)
    one = torch.zeros(8, dtype=torch.int16)
    coefs = [one.as_strided((1, bx * 8), (0, 0)) for _, _, bx, by in geo]
    for si, sc in enumerate(info["scans"]):
        assert 0 <= sc["start"] <= sc["end"] <= len(data)
        specs, desc = D.scan_plan(info, si, sc, geo, grid, coefs)
        assert D.tables_check(specs) == 0
        assert (D.n_intervals(desc) if sc["restart_interval"] else D.unmarked_workspace(desc, sc["end"] - sc["start"])) > 0
    assert len(D.component_luts(info)) == len(info["components"])


@pytest.mark.parametrize("kind", SMALL)
def test_read_jpeg_parses_or_refuses_every_prefix_and_mutated_header(kind):
    data, start = _small(kind)
    assert start < 1024
    _host_checks(jfif.read_jpeg(data, require_restart=False), data)  # the file itself passes
    variants = [data[:n] for n in range(len(data))]
    variants += [data[:i] + bytes([data[i] ^ m]) + data[i + 1:] for i in range(start) for m in (0x01, 0x80, 0xFF)]
    parsed = 0
    for v in variants:
        try:
            info = jfif.read_jpeg(v, require_restart=False)
            _host_checks(info, v)
            parsed += 1
        except (jfif.JpegFormatError, api.MdctError):
            pass
    assert parsed > 0


# ------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    torch.cuda.set_device(0)
    api.init(0)
    return torch


_twins_done = {}


def _run(torch, c, scan, planes, rounds=None):
    """the scan through the path's low-level helper (guard rows, guard bytes) -> (planes as numpy, per-interval status list or
    [class, blocks], guards intact)"""
    b = HC.base_of(c)
    data = _file(c, HC.trace(c.path, b["sparse"])[0], None)  # a valid file of the same geometry and tables: read for its header only
    if b["marked"]:
        from test_jpeg_decode import _low_level
        got, st, intact = _low_level(torch, data, scan_bytes=scan)
        return [g.cpu().numpy() for g in got], [int(x) for x in st], intact
    from test_jpeg_decode_unmarked import _low_level
    got, st, intact, _ = _low_level(torch, data, scan_bytes=scan, sync_rounds=-(-len(scan) // HC.CHUNK) if rounds is None else rounds)
    return [g.cpu().numpy() for g in got], st, intact


def _block(planes, place):
    ci, by, bx = place
    return planes[ci][by * 8:by * 8 + 8, bx * 8:bx * 8 + 8].reshape(64)


def _assert_after_error(b, got, c, res):
    """complete blocks exact, the failing block 0 or the checker's partial block coefficient by coefficient, zeros after it"""
    k = c.interval
    st, blocks, failing, n = res[k]
    truth = HC.truth_blocks(b, c.twin_planes, k)
    for j, (place, want) in enumerate(truth):
        g = _block(got, place)
        if j < n:
            assert np.array_equal(g, want), (c.name, "block before the error", j)
        elif j == n and failing is not None:
            assert failing[0] == place
            part = failing[1].astype(np.int16)
            assert np.all((g == 0) | (g == part)), (c.name, "the failing block", j)
        else:
            assert not g.any(), (c.name, "block after the error", j)


@pytest.mark.gpu
@pytest.mark.parametrize("maker,args", IDS, ids=NAMES)
def test_gpu_hostile_case(gpu, maker, args):
    torch = gpu
    c = HC.build(maker, args)
    b = HC.base_of(c)
    assert c.check_place()
    res = _expect(c)  # classified on the CPU first
    assert res[c.interval][0] == c.klass and res[c.interval][3] == c.n_before
    got, st, intact = _run(torch, c, c.scan, None)
    assert intact, "a guard was written"
    if b["marked"]:
        assert st == [r[0] for r in res], (st, [r[0] for r in res])
        assert st[c.interval] == c.klass and all(s == c.others.get(k, C.OK) for k, s in enumerate(st) if k != c.interval)
        for k, s in enumerate(st):
            if s == C.OK:
                for place, want in HC.truth_blocks(b, c.twin_planes, k):
                    assert np.array_equal(_block(got, place), want), (c.name, "intact interval", k)
        for k in c.others:  # complete, only the marker after it is missing
            for place, want in HC.truth_blocks(b, c.twin_planes, k):
                assert np.array_equal(_block(got, place), want), (c.name, k)
    else:
        assert st == [c.klass, c.n_before], st
        _, st4, intact4 = _run(torch, c, c.scan, None, rounds=4)
        assert intact4 and (st4 == st or st4 == [NOT_SYNCHRONISED, 0]), st4
    _assert_after_error(b, got, c, res)
    for scan, planes in [(c.twin, c.twin_planes)] + ([(c.twin2[1], c.twin2[0])] if hasattr(c, "twin2") else []):
        key = (c.path, b["sparse"], scan)
        if key not in _twins_done:
            tg, ts, ti = _run(torch, c, scan, planes)
            ok = ti and (ts == [C.OK] * b["n_intervals"] if b["marked"] else ts == [C.OK, b["n_blocks"]])
            _twins_done[key] = ok and all(np.array_equal(g, np.asarray(p).astype(np.int16)) for g, p in zip(tg, planes))
        assert _twins_done[key], (c.name, "twin")


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["marked-420", "unmarked-420"])
@pytest.mark.parametrize("sign", [1, -1], ids=["up", "down"])
def test_gpu_stores_the_dc_predictor_as_int16(gpu, path, sign):
    """not an error: a predictor past +-32767 is stored as (int16_t)pred (include/mdct_jpegdec.h), as the checker's planes wrap it"""
    torch = gpu
    b, scan, st, truth = HC.make_dc_wrap(path, sign)
    data, _ = E.encode_file(b["frame"], [b["scan"]], b["planes"], b["specs"])
    if b["marked"]:
        from test_jpeg_decode import _low_level
        got, status, intact = _low_level(torch, data, scan_bytes=scan)
        assert [int(x) for x in status] == [C.OK]
    else:
        from test_jpeg_decode_unmarked import _low_level
        got, status, intact, _ = _low_level(torch, data, scan_bytes=scan)
        assert status == [C.OK, b["n_blocks"]]
    assert intact
    for g, t in zip(got, truth):
        assert np.array_equal(g.cpu().numpy(), t)


FRONT_DOOR = [("marked-grey", "ovf-zrl-at-49", "interval-mid"), ("marked-grey", "bad-ac-16-ones", "interval-last"),
              ("marked-grey", "ood-in-code", "interval0"), ("marked-420", "bad-dc-16-ones", "cb"),
              ("unmarked-grey", "ovf-1s-at-63", "lane-straddle"), ("unmarked-grey", "bad-ac-16-ones", "chunk1-straddle"),
              ("unmarked-grey", "ood-in-code", "lastchunk-after"), ("unmarked-grey", "marker-rst-in-code", "lane-after"),
              ("unmarked-420", "ovf-run15-from-49", "cr")]
FRONT_DOOR_SPECIAL = [("marked-grey", "marker-wrong-rst-after", "mid"), ("marked-grey", "left-extra-block", "last"),
                      ("unmarked-grey", "left-one-0-bit", "last"), ("unmarked-420", "left-7-ones-then-ff", "last")]


@pytest.mark.gpu
def test_decode_jpeg_raises_with_scan_and_status(gpu):
    from simd_dct_amd import jpeg_decode as D
    cases = [HC.make(*a) for a in FRONT_DOOR] + [HC.make_special(*a) for a in FRONT_DOOR_SPECIAL]
    assert {c.klass for c in cases} == {C.OUT_OF_DATA, C.BAD_CODE, C.COEF_OVERFLOW, C.UNEXPECTED_MARKER, C.LEFTOVER}
    for c in cases:
        b = HC.base_of(c)
        with pytest.raises(D.JpegDecodeError) as e:
            D.decode_jpeg(_file(c, c.scan, c.twin_planes))
        assert e.value.scan == 0
        st = [int(x) for x in e.value.status]
        if b["marked"]:
            assert st[c.interval] == c.klass and all(s == C.OK for k, s in enumerate(st) if k != c.interval), (c.name, st)
        else:
            assert st == [c.klass, c.n_before], (c.name, st)
        # a good file decoded next in the same process is exact
        _, coefs = D.decode_jpeg(_file(c, c.twin, c.twin_planes), coefficients=True)
        for g, p in zip(coefs, c.twin_planes):
            assert np.array_equal(g.cpu().numpy(), np.asarray(p).astype(np.int16)), c.name


@pytest.mark.gpu
@pytest.mark.parametrize("dri", [0, 4], ids=["unmarked", "marked"])
def test_decode_jpeg_error_in_the_cb_scan_of_three(gpu, dri):
    """.scan == 1, with mode="RGB" and scale_denom=2 as well, and no inverse, colour or scaled-inverse kernel was launched"""
    from simd_dct_amd import jpeg_decode as D
    frame = dict(width=64, height=32, comps=[(2, 2), (1, 1), (1, 1)])
    scans = [dict(comps=[(ci, min(ci, 1), min(ci, 1))], dri=dri) for ci in range(3)]
    planes = HC.base("marked-420")["planes"]
    good, _ = E.encode_file(frame, scans, planes, dict(E.ANNEX_K))
    bad, st = E.encode_file(frame, scans, planes, dict(E.ANNEX_K), inject={1: dict(block=5, at=7, put=["1" * 16])})
    assert "inject_bit" in st[1] and "inject_bit" not in st[0] and "inject_bit" not in st[2]
    for kw in (dict(), dict(mode="RGB"), dict(scale_denom=2), dict(mode="RGB", scale_denom=2)):
        api.kernel_counts_reset()
        with pytest.raises(D.JpegDecodeError) as e:
            D.decode_jpeg(bad, **kw)
        gpu.cuda.synchronize()
        assert e.value.scan == 1, kw
        st1 = [int(x) for x in e.value.status]
        assert (st1[1] == C.BAD_CODE and st1[0] == C.OK) if dri else st1 == [C.BAD_CODE, 5], (kw, st1)
        ran = {k for k, v in api.kernel_counts().items() if v}
        assert ran and ran <= DECODER_KERNELS, (kw, sorted(ran - DECODER_KERNELS))
        _, coefs = D.decode_jpeg(good, coefficients=True, **kw)
        for g, p in zip(coefs, planes):
            assert np.array_equal(g.cpu().numpy(), p.astype(np.int16)), kw


@pytest.mark.gpu
def test_captured_unmarked_decode_replays_on_a_hostile_scan_then_a_good_one(gpu):
    torch = gpu
    from simd_dct_amd import jpeg_decode as D
    c = HC.make("unmarked-420", "ovf-zrl-at-49", "y3")
    b = HC.base_of(c)
    good = HC.trace(c.path)[0]
    n = len(good)
    # one captured scan_len: the hostile scan is brought to the good one's length; what follows its error decides nothing
    hostile = (c.scan + good[len(c.scan):])[:n]
    res = HC.check_scan(b, hostile)
    assert (res[0][0], res[0][3]) == (c.klass, c.n_before)
    info = jfif.read_jpeg(_file(c, good), require_restart=False)
    sc = info["scans"][0]
    geo, grid = D.geometry(info)
    mcus_x, mcus_y, members = D.scan_geometry(info, sc, geo, grid)
    coefs = [torch.empty((by * 8, bx * 8), dtype=torch.int16, device="cuda") for _, _, bx, by in geo]
    specs, planes = [None] * 4, []
    for cc, (ci, h, v) in zip(sc["components"], members):
        specs[cc["td"]], specs[2 + cc["ta"]] = sc["huffman"][(0, cc["td"])], sc["huffman"][(1, cc["ta"])]
        planes.append((coefs[ci], geo[ci][2], geo[ci][3], h, v, cc["td"], 2 + cc["ta"]))
    tables = D.Tables(specs)
    desc = D.scan_desc(planes, mcus_x, mcus_y, 0)
    buf = torch.zeros(n, dtype=torch.uint8, device="cuda")
    work = torch.empty(D.unmarked_workspace(desc, n), dtype=torch.uint8, device="cuda")
    status = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        D.decode_unmarked(desc, tables, buf, work, status, scan_len=n, sync_rounds=-(-n // HC.CHUNK), stream=s)
    for name, src in (("hostile", hostile), ("good", good)):
        for cf in coefs:
            cf.fill_(0x7777)
        work.fill_(0x99)
        status.fill_(-1)
        buf.copy_(torch.frombuffer(bytearray(src), dtype=torch.uint8).cuda())
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        st = [int(x) for x in status.cpu().numpy()]
        got = [cf.cpu().numpy() for cf in coefs]
        if src is hostile:
            assert st == [c.klass, c.n_before], st
            _assert_after_error(b, got, c, res)
        else:
            assert st == [C.OK, b["n_blocks"]], st
            assert all(np.array_equal(x, np.asarray(p).astype(np.int16)) for x, p in zip(got, b["planes"]))
    tables.close()
