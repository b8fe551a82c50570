"""Progressive JPEG input with successive approximation, with and without restart markers: jfif_sof2.read_sof2_jpeg,
mdct_jpegdec_prog_decode_approx (include/mdct_jpegdec_prog.h) and the decode_jpeg family on the files libjpeg's standard scan script
writes.

Files: tests/golden/progressive_pillow/ (make_progressive_pillow.py): Pillow's progressive=True files of eight small pictures, with
and without restart markers, and the BASELINE TWIN of each, which holds identical coefficients.
Truth: tests/jpeg_progressive_approx_checker.py (T.81 Annex G in serial Python, a status per interval), itself held to
jpeg_decode_checker's planes of the twin; and the twin through the decoder routes the other tests hold to Pillow.
CPU: the checker, the reader and its refusals (one row per raise), the C-ABI's host refusals.  GPU: coefficients, pixels, launches,
canaries, transcoding, the batch fall-back, a non-current stream, damaged scans of every kind."""
import ctypes
import functools
import glob
import os
import re
import time

import numpy as np
import pytest

import jpeg_decode_checker as DC
import jpeg_progressive_approx_checker as AC
import jpeg_progressive_checker as PC
from simd_dct_amd import _jpegdec_prog_lib, api, jfif, jfif_sof2
from test_jpeg_decode_progressive import PROG_REFUSALS, _colour, _desc, _engine_style_file, _grey, _sos, encoder_files

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "progressive_pillow")
FIXTURES = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN, "*.prog*.jpg")))
# libjpeg's standard script (jcparam.c, jpeg_simple_progression) as (components, ss, se, ah, al)
GREY_SCRIPT = [(1, 0, 0, 0, 1), (1, 1, 5, 0, 2), (1, 6, 63, 0, 2), (1, 1, 63, 2, 1), (1, 0, 0, 1, 0), (1, 1, 63, 1, 0)]
COLOUR_SCRIPT = [(3, 0, 0, 0, 1), (1, 1, 5, 0, 2), (1, 1, 63, 0, 1), (1, 1, 63, 0, 1), (1, 6, 63, 0, 2), (1, 1, 63, 2, 1), (3, 0, 0, 1, 0),
                 (1, 1, 63, 1, 0), (1, 1, 63, 1, 0), (1, 1, 63, 1, 0)]


def fixture(name):
    with open(os.path.join(GOLDEN, name + ".jpg"), "rb") as f:
        return f.read()


def twin_of(name):
    return fixture(name.split(".")[0] + ".base")


@functools.lru_cache(None)
def truth(name):
    """the checker's planes and statuses of a fixture, computed once and never changed"""
    planes, statuses = AC.decode(fixture(name))
    for p in planes:
        p.setflags(write=False)
    return planes, statuses


def test_the_fixtures_are_all_there():
    pictures = {n.split(".")[0] for n in FIXTURES}
    assert len(pictures) == 8 and len(FIXTURES) == 17, FIXTURES
    for p in pictures:
        assert {p + ".prog", p + ".prog_nomark"} <= set(FIXTURES) and os.path.exists(os.path.join(GOLDEN, p + ".base.jpg")), p
    assert all(os.path.getsize(f) < 16384 for f in glob.glob(os.path.join(GOLDEN, "*.jpg")))


# ------------------------------------------------------------------------------------------ CPU: the checker
@pytest.mark.parametrize("name", FIXTURES)
def test_checker_equals_the_baseline_checker_on_the_twin(name):
    planes, statuses = truth(name)
    want, twin_statuses, _ = DC.decode(twin_of(name))
    assert all(s == [0] * len(s) for s in statuses) and all(s == [0] * len(s) for s in twin_statuses)
    assert len(planes) == len(want)
    for g, w in zip(planes, want):
        assert np.array_equal(g, w)
    assert any(np.abs(p).max() > 8 for p in planes)  # (not a file of zeros)


# ------------------------------------------------------------------------------------------ CPU: the reader
@pytest.mark.parametrize("name", FIXTURES)
def test_reader_on_the_fixtures(name):
    data = fixture(name)
    info = jfif_sof2.read_sof2_jpeg(data)
    frame, _, scans, _ = PC.parse(data)
    assert info["sof"] == 0xC2 and (info["width"], info["height"]) == (frame["width"], frame["height"])
    got = [(len(s["components"]), s["ss"], s["se"], s["ah"], s["al"]) for s in info["scans"]]
    assert got == (GREY_SCRIPT if len(info["components"]) == 1 else COLOUR_SCRIPT)
    for s, c in zip(info["scans"], scans):
        assert (s["start"], s["end"], s["restart_interval"]) == (c["start"], c["end"], c["dri"])
        assert [(m["index"], m["td"], m["ta"]) for m in s["components"]] == c["comps"]
        assert (s["restart_interval"] == 0) == name.endswith("nomark")
    twin = jfif.read_jpeg(twin_of(name), require_restart=False)
    assert [(c["h"], c["v"]) for c in twin["components"]] == [(c["h"], c["v"]) for c in info["components"]]
    assert all(np.array_equal(twin["qtables"][k], info["qtables"][k]) for k in twin["qtables"]) and twin["colorspace"] == info["colorspace"]
    # the readers that refused these files go on refusing them
    for old in (jfif.read_progressive_jpeg, lambda d: jfif.read_jpeg(d, require_restart=False)):
        with pytest.raises(jfif.JpegFormatError):
            old(data)


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)
    return type(a) is type(b) and a == b


def test_reader_equals_read_progressive_jpeg_on_the_engines_own_files():
    files = [data for _, data, _, _ in encoder_files()] + [_engine_style_file()[0], _grey(), _colour()]
    assert len(files) >= 4
    for data in files:
        assert _same(jfif_sof2.read_sof2_jpeg(data), jfif.read_progressive_jpeg(data))


def _pillow(name="c444_50x35.prog"):
    return fixture(name)


def _scan_header(data, k, ss=None, se=None, a=None):
    return _sos(data, k, ss=ss, se=se, a=a)


def _sof(data, marker):
    i = data.index(b"\xff\xc2")
    return data[:i + 1] + bytes([marker]) + data[i + 2:]


# (what, the file, text of the message): one row per `raise JpegFormatError` of jfif_sof2.py and rows for what it leaves to read_jpeg's
# rules.  Of the old reader's rows, only successive approximation and the missing restart markers are accepted now.
ACCEPTED_NOW = ("successive approximation", "without restart markers")
SOF2_REFUSALS = [r for r in PROG_REFUSALS if r[2] not in ACCEPTED_NOW] + [
    ("Al = 14", lambda: _scan_header(_pillow(), 0, a=0x0E), "Al 14"),
    ("a first scan of coded positions (Ah = 0 again)", lambda: _scan_header(_pillow(), 5, a=0x01), "coded a second time"),
    ("a refinement of positions no scan has coded", lambda: _scan_header(_pillow(), 2, a=0x10), "no scan has coded"),
    ("a refinement whose Ah is not the last Al", lambda: _scan_header(_pillow(), 5, a=0x10), "last coded with Al 2"),
    ("a refinement whose Al is not Ah - 1", lambda: _scan_header(_pillow(), 5, a=0x20), "Ah 2, Al 0"),
    ("a refinement of a band wider than the first scans", lambda: _scan_header(_grey(), 1, ss=1, se=63, a=0x10), "no scan has coded"),
    ("a DC refinement before the DC first scan", lambda: _scan_header(_grey(), 0, a=0x10), "no scan has coded"),
    ("an interleaved AC refinement", lambda: _scan_header(_pillow(), 6, ss=1, se=63), "interleaved AC scan"),
    ("arithmetic coding (SOF10)", lambda: _sof(_pillow(), 0xCA), "not a progressive file"),
    ("a baseline twin", lambda: twin_of("c444_50x35.prog"), "not a progressive file"),
]


@pytest.mark.parametrize("what,make,text", SOF2_REFUSALS, ids=[r[0] for r in SOF2_REFUSALS])
def test_reader_refusals(what, make, text):
    with pytest.raises(jfif.JpegFormatError) as e:
        jfif_sof2.read_sof2_jpeg(make())
    assert text in str(e.value), str(e.value)


def test_what_the_old_reader_refused_and_the_new_one_takes():
    rows = [r for r in PROG_REFUSALS if r[2] in ACCEPTED_NOW and r[0] != "Pillow's progressive file"]
    assert len(rows) == 4
    for what, make, _ in rows:
        if what == "Ah = 1 in an AC scan":  # successive approximation, but not a legal script: nothing to refine there
            with pytest.raises(jfif.JpegFormatError, match="no scan has coded"):
                jfif_sof2.read_sof2_jpeg(make())
            continue
        info = jfif_sof2.read_sof2_jpeg(make())
        assert info["sof"] == 0xC2, what


def test_every_refusal_site_of_the_sof2_reader_has_a_row():
    """the completeness check of test_jpeg_decode_progressive on jfif_sof2.py"""
    src = open(jfif_sof2.__file__).read()
    sites = re.findall(r'raise JpegFormatError\(f?"([^"]*)"', src)
    assert len(sites) >= 8 and len(re.findall(r"raise JpegFormatError", src)) == len(sites), sites
    raised = []
    for _, make, _ in SOF2_REFUSALS:
        with pytest.raises(jfif.JpegFormatError) as e:
            jfif_sof2.read_sof2_jpeg(make())
        raised.append(str(e.value))
    for site in sites:
        texts = [t.strip() for t in re.split(r"\{[^}]*\}", site) if len(t.strip()) > 3]
        assert texts and any(all(t in msg for t in texts) for msg in raised), site


# ------------------------------------------------------------------------------------------ CPU: the C-ABI
def test_cabi_refusals_of_ah_and_al_without_device():
    lib = _jpegdec_prog_lib.load()
    A = 0x10000  # never dereferenced: every call below is refused on the host
    good = _desc([(A, 64, 8, 4, 1, 1, 0, 2)], 8, 4, 8)

    def approx(d, ss, se, ah, al, tables=None):
        rc = lib.mdct_jpegdec_prog_decode_approx(ctypes.byref(d) if d is not None else None, ss, se, ah, al, tables, None, 0, None, None, None)
        return rc, lib.mdct_jpegdec_prog_last_error().decode()

    for ss, se in ((0, 0), (1, 63)):
        for ah, al in ((0, 14), (0, -1), (15, 14), (0, 100)):
            rc, msg = approx(good, ss, se, ah, al)
            assert rc == 1 and f"Al {al}" in msg, msg
        for ah, al in ((1, 1), (2, 0), (3, 1), (-1, 0), (1, 2), (14, 12)):
            rc, msg = approx(good, ss, se, ah, al)
            assert rc == 1 and f"Ah {ah} with Al {al}" in msg, msg
        for ah, al in ((0, 0), (0, 1), (0, 13), (1, 0), (2, 1), (14, 13)):  # legal: refused only for the null pointers behind them
            rc, msg = approx(good, ss, se, ah, al)
            assert rc == 1 and "null tables / scan / offsets / status" in msg, msg
    # what the band and the descriptor are refused for comes first, with the messages of mdct_jpegdec_prog_decode
    rc, msg = approx(good, 0, 5, 9, 9)
    assert rc == 1 and "band 0..5" in msg
    rc, msg = approx(_desc([(A, 64, 8, 4, 1, 1, 0, 2)], 8, 4, 0), 1, 63, 1, 0)
    assert rc == 1 and "restart interval 0" in msg


def test_cabi_approx_at_0_0_refuses_what_decode_refuses_with_the_same_messages():
    lib = _jpegdec_prog_lib.load()
    A = 0x10000
    one = lambda **k: (A, k.get("pitch", 64), 8, 4, k.get("h", 1), k.get("v", 1), k.get("dc", 0), k.get("ac", 2))  # noqa: E731
    y420 = (A, 128, 16, 8, 2, 2, 0, 2)
    colour = _desc([y420, one(dc=1), one(dc=1)], 8, 4, 8)
    good = _desc([one()], 8, 4, 8)
    cases = [(None, 0, 0), (good, 0, 0), (good, 1, 63)] + [(good, ss, se) for ss, se in ((0, 5), (7, 3), (1, 64), (63, 64), (-1, 0), (0, -1), (64, 64))]
    cases += [(colour, 1, 63), (_desc([one(), one()], 8, 4, 8), 1, 5), (_desc([one(h=2)], 4, 4, 8), 1, 5), (_desc([one(h=2)], 4, 4, 8), 0, 0),
              (_desc([one()], 8, 4, 0), 0, 0), (_desc([one()], 8, 4, 0), 1, 63), (_desc([one()], 0, 4, 8), 0, 0), (_desc([(A + 2,) + one()[1:]], 8, 4, 8), 0, 0),
              (_desc([(0,) + one()[1:]], 8, 4, 8), 1, 63), (_desc([one(pitch=68)], 8, 4, 8), 1, 63), (_desc([one(pitch=56)], 8, 4, 8), 0, 0),
              (_desc([one()], 9, 4, 8), 0, 0), (_desc([one(dc=-1)], 8, 4, 8), 0, 0), (_desc([one(dc=2)], 8, 4, 8), 0, 0), (_desc([one(ac=1)], 8, 4, 8), 1, 63),
              (_desc([one(ac=4)], 8, 4, 8), 1, 63), (_desc([], 8, 4, 8), 0, 0), (_desc([(A, 1 << 20, 1 << 17, 1 << 14, 1, 1, 0, 2)], 1 << 17, 1 << 14, 8), 0, 0)]
    seen = set()
    for d, ss, se in cases:
        p = ctypes.byref(d) if d is not None else None
        rc_old = lib.mdct_jpegdec_prog_decode(p, ss, se, None, None, 0, None, None, None)
        msg_old = lib.mdct_jpegdec_prog_last_error().decode()
        rc_new = lib.mdct_jpegdec_prog_decode_approx(p, ss, se, 0, 0, None, None, 0, None, None, None)
        msg_new = lib.mdct_jpegdec_prog_last_error().decode()
        assert rc_old == rc_new and rc_old in (1, 2) and msg_old == msg_new and msg_old, (ss, se, msg_old, msg_new)
        seen.add(msg_old)
    assert len(seen) >= 10, seen


# ------------------------------------------------------------------------------------------ GPU
CANARY = -0x5556


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    torch.cuda.set_device(0)
    api.init(0)
    return torch


@pytest.mark.gpu
def test_decode_jpeg_returns_the_twins_pixels(gpu):
    """on the tree before this feature: JpegFormatError, "not supported: successive approximation" """
    from simd_dct_amd import jpeg_decode as D
    got = D.decode_jpeg(fixture("c420_17x9.prog"), mode="RGB")
    want = D.decode_jpeg(twin_of("c420_17x9.prog"), mode="RGB")
    assert tuple(got.shape) == (9, 17, 3) and gpu.equal(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_coefficients_equal_the_checker_and_the_twin(gpu, name):
    from simd_dct_amd import jpeg_decode as D
    want, _ = truth(name)
    _, got = D.decode_coefficients(fixture(name))
    _, twin = D.decode_coefficients(twin_of(name))
    assert len(got) == len(want) == len(twin)
    for g, w, t in zip(got, want, twin):
        assert np.array_equal(g.cpu().numpy(), w) and gpu.equal(g, t)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_pixels_equal_the_twins(gpu, name):
    from simd_dct_amd import jpeg_decode as D
    data, twin = fixture(name), twin_of(name)
    for kw in (dict(mode="RGB"), dict(mode="RGB", scale_denom=2), dict(mode="RGB", layout="CHW"), dict()):
        got, want = D.decode_jpeg(data, **kw), D.decode_jpeg(twin, **kw)
        if isinstance(got, list):
            assert len(got) == len(want) and all(gpu.equal(g, w) for g, w in zip(got, want)), kw
        else:
            assert got.dtype == gpu.uint8 and gpu.equal(got, want), kw


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["noisy_64x48_q95.prog", "noisy_64x48_q95.prog_nomark", "grey_8x8.prog_nomark"])
def test_only_the_two_kernels_run_the_entropy_stage(gpu, name):
    from simd_dct_amd import jpeg_decode as D
    data = fixture(name)
    info = jfif_sof2.read_sof2_jpeg(data)
    n_dc = sum(1 for s in info["scans"] if s["ss"] == 0)
    n_ac = len(info["scans"]) - n_dc
    gpu.cuda.synchronize()
    api.kernel_counts_reset()
    D.decode_coefficients(data)
    gpu.cuda.synchronize()
    ran = api.kernel_counts()
    assert ran.get("k_decode_prog_dc") == n_dc and ran.get("k_decode_prog_ac") == n_ac, ran
    index = {k: v for k, v in ran.items() if k.startswith("k_rst_")}
    if name.endswith("nomark"):
        assert set(ran) == {"k_decode_prog_dc", "k_decode_prog_ac"}, ran  # no index kernel, nothing else
    else:
        assert set(ran) == {"k_decode_prog_dc", "k_decode_prog_ac"} | set(index) and ran.get("k_rst_scan") == len(info["scans"]), ran


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c420_17x9.prog", "c420_17x9.prog_nomark", "noisy_203x117_q90.prog", "noisy_203x117_q90.prog_nomark"])
def test_a_non_interleaved_scan_leaves_the_planes_padding_alone(gpu, name):
    """17 x 9 at 4:2:0: the luma's own grid is 3 x 2 blocks in a plane of 4 x 2; 203 x 117: 26 x 15 in 26 x 16.  Before every scan of
    one component the blocks outside its grid are filled with canaries: the scan must leave every one of them."""
    torch = gpu
    from simd_dct_amd import jpeg_decode as D
    data = fixture(name)
    info = D.read_file(data)
    geo, grid = D.geometry(info)
    coefs = [torch.zeros((by * 8, bx * 8), dtype=torch.int16, device="cuda") for _, _, bx, by in geo]
    own = [(-(-w // 8), -(-h // 8)) for w, h, _, _ in geo]
    assert (own[0][0] * 8, own[0][1] * 8) != (coefs[0].shape[1], coefs[0].shape[0])
    checked = 0
    for si, sc in enumerate(info["scans"]):
        specs, desc = D.scan_plan(info, si, sc, geo, grid, coefs)
        tables = D.Tables(specs) if any(s is not None for s in specs) else None
        seg = torch.frombuffer(bytearray(data[sc["start"]:sc["end"]]), dtype=torch.uint8).cuda()
        single = len(sc["components"]) == 1
        ci = sc["components"][0]["index"]
        gx, gy = own[ci]
        outside = torch.ones(coefs[ci].shape, dtype=torch.bool, device="cuda")
        outside[:gy * 8, :gx * 8] = False
        keep = coefs[ci].clone()
        if single:
            coefs[ci][outside] = CANARY
        D.decode_scan(torch, si, sc, desc, tables, seg, torch.device("cuda", 0))
        if tables is not None:
            tables.close()
        if single:
            assert bool((coefs[ci][outside] == CANARY).all()), (si, sc["ss"], sc["se"], sc["ah"], sc["al"])
            coefs[ci][outside] = keep[outside]
            checked += int(outside.any())
    assert checked >= 4  # the luma's AC scans
    want, _ = truth(name)
    for g, w in zip(coefs, want):
        assert np.array_equal(g.cpu().numpy(), w)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c422_50x35.prog", "noisy_64x48_q100.prog_nomark"])
def test_transcode_keeps_the_coefficients(gpu, name):
    from simd_dct_amd import jpeg_decode as D
    from simd_dct_amd import jpeg_transcode as TC
    want, _ = truth(name)
    geo, _ = D.geometry(D.read_file(fixture(name)))
    for kw in (dict(), dict(progressive=True)) + ((dict(interleaved=True),) if len(want) == 3 else ()):
        out = TC.transcode_jpeg(fixture(name), **kw)
        assert jfif.sof_marker(out) == (0xC2 if "progressive" in kw else 0xC0)
        _, got = D.decode_coefficients(out)
        for g, w, (width, height, _, _) in zip(got, want, geo):
            # a scan of one component codes the component's own block grid (T.81 A.2.2): the MCU padding beyond it is not in the new file
            gy, gx = (g.shape if "interleaved" in kw else (-(-height // 8) * 8, -(-width // 8) * 8))
            assert np.array_equal(g.cpu().numpy()[:gy, :gx], w[:gy, :gx]), kw


@pytest.mark.gpu
def test_a_progressive_file_between_two_baseline_files_of_a_batch(gpu):
    from simd_dct_amd import jpeg_decode as D
    files = [twin_of("c420_17x9.prog"), fixture("c444_50x35.prog_nomark"), twin_of("noisy_64x48_q95.prog"), fixture("c444_50x35.prog_b3")]
    for kw in (dict(mode="RGB"), dict(coefficients=True)):
        got = D.decode_jpeg_batch(files, **kw)
        for f, g in zip(files, got):
            w = D.decode_jpeg(f, **kw)
            if kw.get("coefficients"):
                assert all(gpu.equal(a, b) for a, b in zip(g[0] + g[1], w[0] + w[1]))
            else:
                assert gpu.equal(g, w)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["noisy_203x117_q90.prog", "noisy_203x117_q90.prog_nomark"])
def test_on_a_stream_that_is_not_current_behind_a_stall(gpu, name):
    """tests/test_jpeg_streams.py's arrangement A: the call's stream is stalled, the default stream is current.  The picture and
    the coefficients come from the host's wait for every scan's status: they must not be back before the stall is over."""
    torch = gpu
    import stream_stall
    from simd_dct_amd import jpeg_decode as D
    data = fixture(name)
    want_px, want_co = D.decode_jpeg(data, mode="RGB", coefficients=True)  # warm, stream=None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    D.decode_jpeg(data, mode="RGB", coefficients=True)
    torch.cuda.synchronize()
    seconds = max(0.2, 5 * (time.perf_counter() - t0))
    assert seconds < 2.0, seconds
    for raw in (False, True):
        s = torch.cuda.Stream()
        done = stream_stall.stall(s, seconds)
        got_px, got_co = D.decode_jpeg(data, mode="RGB", coefficients=True, stream=s.cuda_stream if raw else s)
        assert done.query(), "the call returned while the work before it on its own stream was pending"
        s.synchronize()
        torch.cuda.synchronize()
        assert stream_stall.measured_seconds(done) >= 0.9 * seconds
        assert torch.equal(got_px, want_px) and all(torch.equal(g, w) for g, w in zip(got_co, want_co))


# damaged scans ----------------------------------------------------------------------------------------------------------------
DAMAGED_FILES = ("noisy_64x48_q95.prog", "noisy_64x48_q95.prog_nomark")
# one scan of every kind of the colour script: DC first (Al 1), AC first (Al 2), AC refinement (Ah 2), DC refinement, AC refinement (Ah 1)
DAMAGED_SCANS = {0: "DC first", 1: "AC first", 5: "AC refinement Ah 2", 6: "DC refinement", 9: "AC refinement Ah 1"}
# (numerator, denominator) of the place in the scan, the bits flipped
CHANGES = ((1, 5, 0x10), (2, 5, 0x01), (3, 5, 0x80), (4, 5, 0x04), (1, 7, 0xF0), (3, 7, 0x0F), (5, 7, 0x3C), (6, 7, 0xC3))


def damaged(data, sc):
    """[(what, file)]: the scan truncated by 3 bytes, and single-byte changes at fixed places, moved on to the next byte that is not
    part of a marker or of a stuffed pair and does not become one (the scans keep their places in the file)"""
    s, e = sc["start"], sc["end"]
    assert e - s > 8 and data[e - 4] != 0xFF
    out = [("truncated by 3 bytes", data[:e - 3] + data[e:])]
    for num, den, flip in CHANGES:
        p = s + (e - s) * num // den
        while data[p] == 0xFF or data[p - 1] == 0xFF or data[p] ^ flip == 0xFF:
            p += 1
        assert p < e - 1
        out.append((f"byte {p - s} ^ 0x{flip:02x}", data[:p] + bytes([data[p] ^ flip]) + data[p + 1:]))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("si", sorted(DAMAGED_SCANS), ids=[DAMAGED_SCANS[k] for k in sorted(DAMAGED_SCANS)])
@pytest.mark.parametrize("name", DAMAGED_FILES)
def test_damaged_scans_end_in_a_status(gpu, name, si):
    from simd_dct_amd import jpeg_decode as D
    data = fixture(name)
    info = jfif_sof2.read_sof2_jpeg(data)
    sc = info["scans"][si]
    kind = "first" if sc["ah"] == 0 else "refinement"
    assert DAMAGED_SCANS[si].startswith(("DC " if sc["ss"] == 0 else "AC ") + kind)
    failed = 0
    for what, bad in damaged(data, sc):
        shrunk = len(data) - len(bad)  # (the damage moves no scan, but for the bytes the truncation takes)
        assert [(s["start"] + (shrunk if k > si else 0), s["end"] + (shrunk if k >= si else 0)) for k, s in enumerate(jfif_sof2.read_sof2_jpeg(bad)["scans"])] == \
            [(s["start"], s["end"]) for s in info["scans"]], what
        want, statuses = AC.decode(bad)
        clean = not any(any(st) for st in statuses)
        if clean:
            _, got = D.decode_coefficients(bad)
            for g, w in zip(got, want):
                assert np.array_equal(g.cpu().numpy(), w), what
            continue
        failed += 1
        k = len(statuses) - 1  # the checker stops at the first scan with a failed interval
        with pytest.raises(D.JpegDecodeError, match=rf"scan {k} \(band {info['scans'][k]['ss']}\.\.{info['scans'][k]['se']}, Ah \d+ Al \d+\)") as e:
            D.decode_coefficients(bad)
        assert e.value.scan == k and [int(x) for x in e.value.status] == statuses[k], (what, list(e.value.status), statuses[k])
        with pytest.raises(D.JpegDecodeError):
            D.decode_jpeg(bad, mode="RGB")
    assert failed >= 1  # (the truncation at least)
