"""Progressive JPEG output with spectral selection: libmdct_jpegprog.so (include/mdct_jpegprog.h), jpeg_progressive.prog_dc_histogram,
prog_dc_rows, prog_ac_histogram, prog_ac_rows, jfif.write_progressive_jpeg, encode_coefficients / transcode_jpeg / encode_jpeg with
progressive=True.

Truth comes from the test side: jpeg_progressive_encoder codes known planes serially by the rules of libjpeg's jcphuff.c,
jpeg_progressive_checker decodes SOF2 files serially with EOBRUN, Pillow is the independent decoder.

CPU: encoder -> checker round trips; Pillow reads the encoder's files as progressive and to the pixels of the baseline file of the same
planes; write_progressive_jpeg's layout; the C-ABI's refusals; the Python layer's refusals before any device work; the code object.
GPU: segments, byte counts, 0xFF counts and histograms against the encoder, byte for byte, with canaries: chunk seams, end-of-band runs
of every shape, the 0x7FFF split, band edges, amplitudes and loss, tables that lack a symbol, whole files, encode_jpeg, a captured graph."""
import io
import os

import numpy as np
import pytest

import jpeg_optimal_tables as T
import jpeg_progressive_checker as PC
import jpeg_progressive_encoder as PE
import jpeg_scan_encoder as E
import jpeg_transform_checker as X
from simd_dct_amd import _jpegcoef_lib, _jpegenc_opt_lib, _jpegprog_lib, api, jfif
from simd_dct_amd import jpeg_progressive as P
from simd_dct_amd import jpeg_transcode as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG_LIB = os.path.join(ROOT, "simd_dct_amd", "libmdct_jpegprog.so")
KERNELS = {f"k_prog_dc<{hv}, {st}>" for hv in ("0, 0", "1, 1", "2, 1", "2, 2") for st in ("true", "false")} | {"k_prog_ac<true>", "k_prog_ac<false>"}
S444, S422, S420 = [(1, 1)] * 3, [(2, 1), (1, 1), (1, 1)], [(2, 2), (1, 1), (1, 1)]
SCAN3 = [(0, 0, 0), (1, 1, 1), (2, 1, 1)]
ANNEX_DC = [E.ANNEX_K[(0, 0)], E.ANNEX_K[(0, 1)]]
CUSTOM = {1: [[(1, 1), (2, 9), (10, 62), (63, 63)]], 3: [[(1, 5), (6, 63)], [(1, 63)], [(1, 20), (21, 63)]]}
# every symbol a band scan can emit, 16-bit codes but for three
LONG_AC = E.spec_from_lengths({s: (3 if i < 3 else 15 if i % 2 else 16) for i, s in enumerate([0x00, 0xF0] + [r << 4 | s for r in range(16) for s in range(1, 11)] + [n << 4 for n in range(1, 15)])})


def sparse(rng, shape, amp=40, density=0.15, dc=200):
    p = (rng.integers(-amp, amp + 1, shape) * (rng.random(shape) < density)).astype(np.int16)
    p[::8, ::8] = rng.integers(-dc, dc + 1, (shape[0] // 8, shape[1] // 8))
    return p


def own_shapes(frame):
    return [(gy * 8, gx * 8) for gx, gy in (PE.own_grid(frame, ci) for ci in range(len(frame["comps"])))]


def as_written(frame, planes, interleaved_dc):
    """what a progressive file of these planes holds: AC over each component's own grid only; DC there too, or over the MCU grid
    when the DC scan is interleaved"""
    out = []
    for p, (r, c) in zip(planes, own_shapes(frame)):
        q = np.array(p, dtype=np.int16)
        dc = q[::8, ::8].copy()
        q[r:], q[:, c:] = 0, 0
        if interleaved_dc and len(planes) == 3:
            q[::8, ::8] = dc
        out.append(q)
    return out


def make_planes(frame, seed, interleaved_dc):
    rng = np.random.default_rng(seed)
    return as_written(frame, [sparse(rng, s) for s in E.plane_shapes(frame)], interleaved_dc)


FRAMES = {"grey": dict(width=20, height=12, comps=[(1, 1)]), "4:4:4": dict(width=24, height=40, comps=S444), "4:2:2": dict(width=48, height=16, comps=S422),
          "4:2:0": dict(width=64, height=32, comps=S420), "4:2:0 odd": dict(width=83, height=45, comps=S420)}


# ------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name", list(FRAMES))
def test_encoder_and_checker_round_trip(name):
    frame = FRAMES[name]
    nc = len(frame["comps"])
    for inter in (True, False):
        for bands in (None, CUSTOM[nc]):
            planes = make_planes(frame, 7, inter)
            data, info = PE.encode_file(frame, planes, bands=bands, interleaved_dc=inter)
            got, meta = PC.decode(data)
            assert meta["frame"]["sof"] == 0xC2 and len(meta["scans"]) == len(info)
            for g, p in zip(got, planes):
                assert np.array_equal(g, p), (name, inter, bands)
            assert [(s["ss"], s["se"], s["dri"]) for s in meta["scans"]] == [(s["ss"], s["se"], s["dri"]) for s in info]


def test_the_rules_on_one_block_row_by_hand():
    """band 6..63 over six blocks: a level below the band alone leaves its block empty (run 1); position 30 after 24 zeros inside the band
    flushes EOB0, then ZRL and 8/2, and starts a run that grows to 3; position 63 flushes EOB1, then three ZRLs and 9/1, and starts no
    run; the last block's run of 1 ends with the interval"""
    row = row_of([zz_block({5: 3}), zz_block({30: -2}), zz_block({}), zz_block({}), zz_block({63: 1}), zz_block({})])
    _, counts, lost, _ = PE.ac_scan(row, 6, 1, 6, 63)
    assert {s: int(c) for s, c in enumerate(counts) if c} == {0x00: 2, 0xF0: 4, 0x82: 1, 0x10: 1, 0x91: 1} and lost == 0
    segs = PE.ac_scan(row, 6, 1, 6, 63, LONG_AC)[0]
    codes = E.canonical_codes(*LONG_AC)
    bits = ""
    for sym, extra, n in ((0x00, 0, 0), (0xF0, 0, 0), (0x82, 1, 2), (0x10, 1, 1), (0xF0, 0, 0), (0xF0, 0, 0), (0xF0, 0, 0), (0x91, 1, 1), (0x00, 0, 0)):
        bits += format(codes[sym][0], f"0{codes[sym][1]}b") + (format(extra, f"0{n}b") if n else "")
    bits += "1" * (-len(bits) % 8)
    assert segs[0] == int(bits, 2).to_bytes(len(bits) // 8, "big")


@pytest.mark.parametrize("name", list(FRAMES))
def test_pillow_reads_the_encoders_files_as_progressive(name):
    Image = pytest.importorskip("PIL.Image")
    frame = FRAMES[name]
    nc = len(frame["comps"])
    for inter in (True, False):
        planes = make_planes(frame, 3, inter)
        q = [np.full(64, 3), np.full(64, 5)]
        scans = [dict(comps=SCAN3[:nc] if nc == 3 else [(0, 0, 0)], dri=0)]
        base, _ = E.encode_file(frame, scans, planes, E.ANNEX_K, qtables=q)
        prog, _ = PE.encode_file(frame, planes, qtables=q, bands=CUSTOM[nc] if inter else None, interleaved_dc=inter)
        a, b = Image.open(io.BytesIO(base)), Image.open(io.BytesIO(prog))
        assert b.info.get("progressive") and not a.info.get("progressive")
        assert np.array_equal(np.asarray(a), np.asarray(b)), (name, inter)
        a, b = Image.open(io.BytesIO(base)), Image.open(io.BytesIO(prog))
        mode = "L" if nc == 1 else "RGB"
        a.draft(mode, (frame["width"] // 2, frame["height"] // 2))
        b.draft(mode, (frame["width"] // 2, frame["height"] // 2))
        assert a.size == b.size and a.size[0] < frame["width"] and np.array_equal(np.asarray(a), np.asarray(b)), (name, inter, "draft 1/2")


def test_write_progressive_jpeg_layout():
    body = lambda k, n: bytes((i * k + 7) % 251 for i in range(n))  # noqa: E731
    qa, qb = [1 + (i * 3) % 200 for i in range(64)], [255 - i for i in range(64)]
    dc0, dc1, ac = E.ANNEX_K[(0, 0)], E.ANNEX_K[(0, 1)], LONG_AC
    scans = [dict(components=SCAN3, ss=0, se=0, restart_interval=3, tables={(0, 0): dc0, (0, 1): dc1}, scan=body(3, 40)),
             dict(components=[(0, 0, 0)], ss=1, se=5, restart_interval=6, tables={(1, 0): ac}, scan=body(5, 50)),
             dict(components=[(0, 0, 0)], ss=6, se=63, restart_interval=6, tables={(1, 0): ac}, scan=body(7, 60)),
             dict(components=[(1, 1, 1)], ss=1, se=63, restart_interval=3, tables={(1, 1): ac}, scan=body(11, 30)),
             dict(components=[(2, 1, 1)], ss=1, se=63, restart_interval=3, tables={(1, 1): ac}, scan=body(13, 31))]
    data = jfif.write_progressive_jpeg([qa, qb, qb], 40, 24, S420, scans)
    frame, qt, got, head = PC.parse(data)
    assert head == [0xE0, 0xDB, 0xDB, 0xC2] and frame["sof"] == 0xC2
    assert (frame["width"], frame["height"]) == (40, 24) and frame["components"] == [(1, 2, 2, 0), (2, 1, 1, 1), (3, 1, 1, 1)]
    assert qt[0] == qa and qt[1] == qb and data[-2:] == b"\xff\xd9"
    assert len(got) == len(scans)
    for g, s in zip(got, scans):
        assert g["order"] == [0xC4, 0xDD, 0xDA], "DHT, DRI, SOS before every scan"
        assert (g["comps"], g["ss"], g["se"], g["ah"], g["al"], g["dri"]) == (list(s["components"]), s["ss"], s["se"], 0, 0, s["restart_interval"])
        assert data[g["start"]:g["end"]] == s["scan"]
    # the engine's own reader refuses the file, as it refuses every SOF2 file
    with pytest.raises(jfif.JpegFormatError, match="progressive"):
        jfif.read_jpeg(data)
    # grey; the colour-space markers as write_jpeg writes them
    g1 = jfif.write_progressive_jpeg([qa], 20, 12, [(1, 1)], [dict(scans[0], components=[(0, 0, 0)], tables={(0, 0): dc0}), scans[1], scans[2]], colorspace="grey")
    assert PC.parse(g1)[0]["components"] == [(1, 1, 1, 0)]
    rgb = jfif.write_progressive_jpeg([qa, qa, qa], 40, 24, S444, scans, colorspace="RGB")
    assert b"Adobe" in rgb[:20] and b"JFIF" not in rgb[:20] and PC.parse(rgb)[3].count(0xDB) == 1
    for bad in (dict(scans=[dict(scans[1], ss=0, se=5)]), dict(scans=[dict(scans[1], ss=6, se=5)]), dict(scans=[dict(scans[1], se=64)]),
                dict(scans=[dict(scans[1], components=SCAN3)]), dict(scans=[dict(scans[0], components=SCAN3[:2])]), dict(scans=[dict(scans[1], restart_interval=0)]),
                dict(scans=[dict(scans[1], components=[(3, 0, 0)])]), dict(colorspace="grey"), dict(qtables=[qa, qb]), dict(qtables=[qa, qb, [0] * 64])):
        kw = dict(qtables=[qa, qb, qb], scans=scans, colorspace=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            jfif.write_progressive_jpeg(kw["qtables"], 40, 24, S420, kw["scans"], colorspace=kw["colorspace"])


class _S:
    def __init__(self, bits, vals, nvals=None):
        self.b = np.asarray(bits, dtype=np.uint8)
        self.v = np.asarray(list(vals) + [0], dtype=np.uint8)
        self.spec = _jpegenc_opt_lib.Spec(self.b.ctypes.data, self.v.ctypes.data, len(vals) if nvals is None else nvals)


def _P(coef, pitch, bx, by, h=1, v=1):
    return _jpegcoef_lib.Plane(coef, pitch, bx, by, h, v)


def test_cabi_refusals_without_device():
    lib = _jpegprog_lib.load()
    A, B, C, OUT, SB, FF, UN, LO, HI = 1 << 40, 1 << 41, 1 << 42, 1 << 44, 1 << 45, 1 << 46, 1 << 47, 1 << 48, 1 << 49  # nothing is dereferenced
    err = lambda: lib.mdct_jpegprog_last_error().decode()  # noqa: E731
    stride = lambda n: int(_jpegenc_opt_lib.load().mdct_jpegenc_opt_seg_stride(n))  # noqa: E731
    p420 = [_P(A, 64, 8, 4, 2, 2), _P(B, 32, 4, 2), _P(C, 32, 4, 2)]
    one = _P(A, 64, 8, 4)
    bad_planes = {"null coef": _P(0, 64, 8, 4), "coef misaligned": _P(A + 8, 64, 8, 4), "pitch misaligned": _P(A, 68, 8, 4), "pitch too short": _P(A, 56, 8, 4),
                  "0 blocks wide": _P(A, 64, 0, 4), "0 blocks high": _P(A, 64, 8, 0), "65536 blocks wide": _P(A, 1 << 20, 65536, 4),
                  "65536 blocks high": _P(A, 64, 8, 65536)}
    bad_sampling = {"4:1:1": [_P(A, 128, 16, 2, 4, 1), p420[1], p420[2]], "4:4:0": [_P(A, 32, 4, 4, 1, 2), p420[1], p420[2]],
                    "chroma 2x1": [p420[0], _P(B, 32, 4, 2, 2, 1), p420[2]], "luma off the MCU grid": [_P(A, 64, 8, 3, 2, 2), p420[1], p420[2]],
                    "chroma planes disagree": [p420[0], p420[1], _P(C, 32, 3, 2)]}
    arr = lambda planes: None if planes is None else (_jpegcoef_lib.Plane * max(1, len(planes)))(*planes)  # noqa: E731
    over = [0] * 16
    over[1] = 5
    ones = [0] * 16
    ones[0] = 2
    kdc, kac = _S(*E.ANNEX_K[(0, 0)]), _S(*E.ANNEX_K[(1, 0)])
    bad_dc = {"over-subscribed": _S(over, range(5)), "all-ones code": _S(ones, [0, 1]), "counts and values disagree": _S(E.ANNEX_K[(0, 0)][0], range(12), nvals=11),
              "no values": _S([0] * 16, []), "DC category 12": _S(E.ANNEX_K[(0, 0)][0], list(range(11)) + [12]),
              "a symbol twice": _S(E.ANNEX_K[(0, 0)][0], [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 10]), "AC table as DC": kac,
              "null counts": type("N", (), {"spec": _jpegenc_opt_lib.Spec(None, kdc.v.ctypes.data, 12)})()}
    bad_ac = {"257 values": _S([0] * 15 + [255], range(255), nvals=257), "AC size 11": _S(E.ANNEX_K[(1, 0)][0], [0x0B] + list(E.ANNEX_K[(1, 0)][1][1:])),
              "over-subscribed": _S(over, range(5)), "all-ones code": _S(ones, [0, 1]), "a symbol twice": _S([0, 2] + [0] * 14, [0x10, 0x10]),
              "null values": type("N", (), {"spec": _jpegenc_opt_lib.Spec(kac.b.ctypes.data, None, 162)})()}

    # ---- DC statistics
    def dc_stats(planes=p420, n=3, inter=1, cls=0, hist=HI, lost=LO):
        return lib.mdct_jpegprog_dc_stats(arr(planes), n, inter, cls, hist, lost, None)

    cases = {"null planes": dict(planes=None), "null hist": dict(hist=None), "null unrepresentable": dict(lost=None), "hist unaligned": dict(hist=HI + 2),
             "unrepresentable unaligned": dict(lost=LO + 1), "three planes, not interleaved": dict(inter=0), "one plane, interleaved": dict(planes=[one], n=1),
             "two planes": dict(n=2), "interleaved 2": dict(inter=2), "class 2": dict(cls=2), "class -1": dict(cls=-1)}
    cases.update({name: dict(planes=p) for name, p in bad_sampling.items()})
    for name, p in bad_planes.items():
        cases["one plane, " + name] = dict(planes=[p], n=1, inter=0)
        cases["plane 1, " + name] = dict(planes=[p420[0], p, p420[2]])
    for name, kw in cases.items():
        assert dc_stats(**kw) == 1 and err(), name

    # ---- the DC coder
    def dc_rows(planes=p420, n=3, inter=1, specs=(kdc, kdc), r0=0, r1=2, out=OUT, seg_stride=stride(24), sb=SB, ff=FF, un=UN, lost=LO):
        sp = None if specs is None else (_jpegenc_opt_lib.Spec * len(specs))(*[s.spec for s in specs])
        return lib.mdct_jpegprog_dc_rows(arr(planes), n, inter, sp, r0, r1, out, seg_stride, sb, ff, un, lost, None)

    cases = {"null planes": dict(planes=None), "null specs": dict(specs=None), "null out": dict(out=None), "null seg_bytes": dict(sb=None), "null ff_counts": dict(ff=None),
             "null uncoded": dict(un=None), "null unrepresentable": dict(lost=None), "uncoded unaligned": dict(un=UN + 1), "unrepresentable unaligned": dict(lost=LO + 2),
             "r0 == r1": dict(r0=1, r1=1), "r1 beyond": dict(r1=3), "short stride": dict(seg_stride=stride(24) - 4), "the 4:2:2 stride": dict(seg_stride=stride(16)),
             "stride not a multiple of 4": dict(seg_stride=stride(24) + 2), "out unaligned": dict(out=OUT + 2), "three planes, not interleaved": dict(inter=0),
             "one plane, short stride": dict(planes=[one], n=1, inter=0, r1=4, seg_stride=stride(7))}
    cases.update({name: dict(planes=p) for name, p in bad_sampling.items()})
    cases.update({"plane 2, " + name: dict(planes=[p420[0], p420[1], p]) for name, p in bad_planes.items()})
    cases.update({"luminance " + name: dict(specs=(s, kdc)) for name, s in bad_dc.items()})
    cases.update({"chrominance " + name: dict(specs=(kdc, s)) for name, s in bad_dc.items()})
    for name, kw in cases.items():
        assert dc_rows(**kw) == 1 and err(), name

    # ---- AC statistics
    def ac_stats(plane=one, ss=1, se=63, hist=HI, lost=LO):
        return lib.mdct_jpegprog_ac_stats(plane, ss, se, hist, lost, None)

    bad_bands = {"Ss = 0": dict(ss=0), "Se > 63": dict(se=64), "Ss > Se": dict(ss=6, se=5), "Ss negative": dict(ss=-1)}
    cases = {"null plane": dict(plane=None), "null hist": dict(hist=None), "null unrepresentable": dict(lost=None), "hist unaligned": dict(hist=HI + 1),
             "unrepresentable unaligned": dict(lost=LO + 2)}
    cases.update(bad_bands)
    cases.update({name: dict(plane=p) for name, p in bad_planes.items()})
    for name, kw in cases.items():
        assert ac_stats(**kw) == 1 and err(), name

    # ---- the AC coder
    def ac_rows(plane=one, ss=1, se=63, by0=0, by1=4, ac=kac, out=OUT, seg_stride=stride(8), sb=SB, ff=FF, un=UN, lost=LO):
        return lib.mdct_jpegprog_ac_rows(plane, ss, se, by0, by1, None if ac is None else ac.spec, out, seg_stride, sb, ff, un, lost, None)

    cases = {"null plane": dict(plane=None), "null AC": dict(ac=None), "null out": dict(out=None), "null seg_bytes": dict(sb=None), "null ff_counts": dict(ff=None),
             "null uncoded": dict(un=None), "null unrepresentable": dict(lost=None), "uncoded unaligned": dict(un=UN + 1), "unrepresentable unaligned": dict(lost=LO + 2),
             "by0 == by1": dict(by0=2, by1=2), "by1 beyond": dict(by1=5), "short stride": dict(seg_stride=stride(8) - 4), "the Annex K stride": dict(seg_stride=208 * 8 + 8),
             "stride not a multiple of 4": dict(seg_stride=stride(8) + 2), "out unaligned": dict(out=OUT + 1), "DC table as AC": dict(ac=_S(E.ANNEX_K[(0, 0)][0], [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]))}
    cases.update(bad_bands)
    cases.update({name: dict(plane=p) for name, p in bad_planes.items()})
    cases.update({name: dict(ac=s) for name, s in bad_ac.items()})
    for name, kw in cases.items():
        assert ac_rows(**kw) == 1 and err(), name
    # the EOBn symbols 0x10 .. 0xE0 are legal here: a specification that names 0x10 twice is refused for the repetition, not for the symbol
    # (nothing that would be accepted is called: it would reach the device; the GPU tests code with LONG_AC, which holds every EOBn)
    assert ac_rows(ac=bad_ac["a symbol twice"]) == 1 and "0x10 is named twice" in err()
    assert ac_rows(ac=_S([0, 3] + [0] * 14, [0x10, 0xE0, 0xE0])) == 1 and "0xe0 is named twice" in err()
    assert ac_rows(ac=bad_ac["AC size 11"]) == 1 and "not a baseline AC symbol" in err()


def test_python_refusals_before_any_device_work(monkeypatch):
    from simd_dct_amd import jpeg_decode as D
    from simd_dct_amd import jpeg_encode as J
    from test_jpeg_transcode import _file

    def no_device(*a, **k):
        raise AssertionError("device work before the arguments were checked")

    monkeypatch.setattr(D, "decode_coefficients", no_device)
    for name in ("prog_dc_histogram", "prog_dc_rows", "prog_ac_histogram", "prog_ac_rows", "encode"):
        monkeypatch.setattr(P, name, no_device)
    monkeypatch.setattr(J, "to_planes", no_device)
    f420, _, _ = _file(40, 24, S420)
    grey, _, _ = _file(20, 12, [(1, 1)])
    with pytest.raises(ValueError, match="optimize=True"):
        TC.transcode_jpeg(f420, progressive=True, optimize=False)
    with pytest.raises(ValueError, match="interleaved=True"):
        TC.transcode_jpeg(grey, progressive=True, interleaved=True)
    for bad in (1, 0, None, "yes", 1.0, [True]):
        with pytest.raises(ValueError, match="progressive"):
            TC.transcode_jpeg(f420, progressive=bad)
        with pytest.raises(ValueError, match="progressive"):
            TC.encode_coefficients([None] * 3, [[16] * 64] * 3, 16, 16, S420, progressive=bad)
        with pytest.raises(ValueError, match="progressive"):
            J.encode_jpeg(np.zeros((8, 8), dtype=np.uint8), progressive=bad)
    q = [16] * 64
    args = dict(coefs=[None] * 3, qtables=[q] * 3, width=16, height=16, sampling=S420, progressive=True)
    with pytest.raises(ValueError, match="optimize=True"):
        TC.encode_coefficients(**args, optimize=False)
    with pytest.raises(ValueError, match="bands"):
        TC.encode_coefficients(**dict(args, progressive=False), bands=CUSTOM[3])
    chroma = [(1, 63)]
    for luma in ([(1, 5), (5, 63)], [(1, 5), (7, 63)], [(6, 63), (1, 5)], [(1, 62)], [(2, 63)], [(1, 64)], [(0, 63)], [(5, 1), (6, 63)], [], [(1, 5.5), (6, 63)], [(1, 63, 0)], [1, 63],
                 "ab"):
        with pytest.raises(ValueError, match="bands"):
            TC.encode_coefficients(**args, bands=[luma, chroma, chroma])
    for bands in ([[(1, 63)]], [[(1, 63)]] * 4, 5, [[(1, 63)], chroma, None]):
        with pytest.raises(ValueError, match="bands"):
            TC.encode_coefficients(**args, bands=bands)
    with pytest.raises(ValueError, match="interleaved=True"):
        TC.encode_coefficients([None], [q], 16, 16, [(1, 1)], progressive=True, interleaved=True)
    assert P.check_bands(None, 3) == [[(1, 2), (3, 9), (10, 63)], [(1, 63)], [(1, 63)]] and P.check_bands(None, 1) == [[(1, 2), (3, 9), (10, 63)]]
    assert P.check_bands(CUSTOM[3], 3) == CUSTOM[3]


def test_code_object_holds_the_planned_instantiations():
    from test_kernel_coverage import code_object_kernels
    names, n_objects = code_object_kernels(lib=PROG_LIB)
    assert n_objects == 1 and names == KERNELS, sorted(names ^ KERNELS)


# ------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    torch.cuda.set_device(0)
    api.init(0)
    return torch


def dev(torch, p, pad=0):
    """the plane on the device, its rows `pad` blocks further apart than they are wide"""
    p = np.ascontiguousarray(p)
    t = torch.zeros((p.shape[0], p.shape[1] + 8 * pad), dtype=torch.int16, device="cuda")
    t[:, :p.shape[1]] = torch.from_numpy(p).cuda()
    return t[:, :p.shape[1]]


def _coded(torch, n_rows, blocks, rows, extra, launch):
    """run a coder into canary-filled buffers -> (segments per interval or None, seg_bytes, ff_counts, uncoded, unrepresentable)"""
    stride = TC.opt_seg_stride(blocks) + extra
    seg = torch.full((n_rows * stride + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    counts = torch.full((2, n_rows + 2), -7, dtype=torch.int32, device="cuda")
    words = torch.zeros((4,), dtype=torch.int32, device="cuda")
    words[1], words[3] = -9, -9
    r0, r1 = rows or (0, n_rows)
    launch(seg, counts[0], counts[1], words[0:1], words[2:3], stride, r0, r1)
    s, c, w = seg.cpu().numpy(), counts.cpu().numpy(), words.cpu().numpy()
    assert w[1] == -9 and w[3] == -9 and np.all(c[:, n_rows:] == -7) and np.all(s[n_rows * stride:] == 0xA5)
    out = []
    for r in range(n_rows):
        if r0 <= r < r1:
            n = int(c[0, r])
            assert 0 < n <= stride and np.all(s[r * stride + -(-n // 4) * 4:(r + 1) * stride] == 0xA5), ("past the segment's last word", r, n)
            out.append(s[r * stride:r * stride + n].tobytes())
        else:
            assert c[0, r] == -7 and c[1, r] == -7 and np.all(s[r * stride:(r + 1) * stride] == 0xA5), ("a row not asked for was written", r)
            out.append(None)
    return out, c[0, :n_rows], c[1, :n_rows], int(w[0]), int(w[2])


def _compare(got, want):
    segs, nbytes, ff, _, _ = got
    for r, g in enumerate(segs):
        if g is not None:
            assert g == want[r], ("segment", r, len(g), len(want[r]), g[:24].hex(), want[r][:24].hex())
            assert nbytes[r] == len(want[r]) and ff[r] == want[r].count(b"\xff"), ("counts", r)


def ac_check(torch, plane, ss, se, spec=None, rows=None, pad=0, extra=0, grid=None, lost_want=0):
    """the band's histogram and segments against the encoder; the table made for the band unless one is given -> the counts"""
    bx, by = grid or (plane.shape[1] // 8, plane.shape[0] // 8)
    _, counts, lost, _ = PE.ac_scan(plane, bx, by, ss, se)
    assert lost == lost_want
    spec = spec or T.optimal_table(counts)
    want, _, _, unc = PE.ac_scan(plane, bx, by, ss, se, spec)
    d = dev(torch, plane, pad)
    hist, hl = P.prog_ac_histogram(d, ss, se, grid=(bx, by))
    hist = hist.cpu().numpy().astype(np.int64)
    assert np.array_equal(hist, counts), ("histogram", ss, se, {s: (int(a), int(b)) for s, (a, b) in enumerate(zip(hist, counts)) if a != b})
    assert int(hl.item()) == lost
    got = _coded(torch, by, bx, rows, extra, lambda seg, sb, ff, un, lo, stride, r0, r1: P.prog_ac_rows(d, ss, se, spec, seg, sb, ff, un, lo, grid=(bx, by), seg_stride=stride,
                                                                                                        by0=r0, by1=r1))
    _compare(got, want)
    if rows is None:
        assert got[3] == unc and got[4] == lost
    return counts


def dc_check(torch, planes, sampling=None, specs=None, rows=None, pad=0, extra=0, lost_want=0):
    inter = sampling is not None
    samp = sampling or [(1, 1)]
    frame = dict(width=planes[0].shape[1], height=planes[0].shape[0], comps=samp)
    comps = [(ci, min(ci, 1)) for ci in range(len(planes))]
    _, counts, lost = PE.dc_scan(frame, comps, planes)
    assert lost == lost_want
    specs = specs or [T.optimal_table(counts[cls, :16]) for cls in range(2 if inter else 1)]
    want, _, _ = PE.dc_scan(frame, comps, planes, dict(enumerate(specs)))
    d = [dev(torch, p, pad) for p in planes]
    hist, hl = P.prog_dc_histogram(d, samp, interleaved=inter)
    assert np.array_equal(hist.cpu().numpy().astype(np.int64), counts) and int(hl.item()) == lost
    n_rows, per = planes[-1].shape[0] // 8, planes[-1].shape[1] // 8
    blocks = per * (sum(h * v for h, v in samp) if inter else 1)
    got = _coded(torch, n_rows, blocks, rows, extra, lambda seg, sb, ff, un, lo, stride, r0, r1: P.prog_dc_rows(d, samp, specs, seg, sb, ff, un, lo, interleaved=inter,
                                                                                                                seg_stride=stride, r0=r0, r1=r1))
    _compare(got, want)
    if rows is None:
        assert got[3] == 0 and got[4] == lost
    return counts


def zz_block(levels, dc=0):
    """{zig-zag index: level} -> an 8 x 8 block"""
    b = np.zeros(64, dtype=np.int16)
    b[0] = dc
    for k, v in levels.items():
        b[E.ZZ[k]] = v
    return b.reshape(8, 8)


def row_of(blocks):
    return np.concatenate(blocks, axis=1)


def put(plane, row, bx, block):
    plane[row * 8:row * 8 + 8, bx * 8:bx * 8 + 8] = block


@pytest.mark.gpu
@pytest.mark.parametrize("width", (255, 256, 257))
def test_chunk_seams_of_the_one_plane_forms(gpu, width):
    rng = np.random.default_rng(width)
    p = sparse(rng, (24, width * 8), density=0.1)
    p[:, (width - 40) * 8:(width - 3) * 8][rng.random((24, 37 * 8)) < 0.9] = 0  # a sparse stretch across the end of the first chunk
    for i, (ss, se) in enumerate(((1, 63), (6, 63), (1, 5))):
        ac_check(gpu, p, ss, se, pad=i)
        ac_check(gpu, p, ss, se, rows=(1, 2), extra=8)
    ac_check(gpu, p, 1, 63, spec=LONG_AC)
    dc_check(gpu, [p], pad=1)
    dc_check(gpu, [p], rows=(1, 2), extra=8)
    dc_check(gpu, [p], specs=ANNEX_DC[:1])
    ran = set(api.kernel_counts())
    assert {"k_prog_ac<true>", "k_prog_ac<false>", "k_prog_dc<0, 0, true>", "k_prog_dc<0, 0, false>"} <= ran, ran


LAYOUTS = [("4:2:0", S420, (31, 32, 33)), ("4:2:2", S422, (31, 32, 33)), ("4:4:4", S444, (63, 64, 65))]


@pytest.mark.gpu
@pytest.mark.parametrize("name,sampling,widths", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_chunk_seams_of_the_interleaved_dc_scan(gpu, name, sampling, widths):
    for i, w in enumerate(widths):
        rng = np.random.default_rng(200 + i)
        planes = [sparse(rng, (3 * v * 8, w * h * 8), dc=1000) for h, v in sampling]
        dc_check(gpu, planes, sampling, pad=i)
        dc_check(gpu, planes, sampling, rows=(1, 2), extra=8)
        dc_check(gpu, planes, sampling, specs=ANNEX_DC)
    hv = {"4:2:0": "2, 2", "4:2:2": "2, 1", "4:4:4": "1, 1"}[name]
    assert {f"k_prog_dc<{hv}, true>", f"k_prog_dc<{hv}, false>"} <= set(api.kernel_counts())


@pytest.mark.gpu
@pytest.mark.parametrize("band", ((6, 63), (1, 63)))
def test_end_of_band_runs(gpu, band):
    ss, se = band
    busy = zz_block({ss: 3, 20: -1})  # non-empty, position se zero: a run starts here
    full = zz_block({ss + 1: 2, se: -5})  # position se coded: no run starts here
    empty = zz_block({2: 7} if ss > 2 else {})  # nothing in the band
    # entirely empty rows: one token per row
    for n in (1, 2, 3, 4, 63, 64, 65, 256, 257):
        counts = ac_check(gpu, row_of([empty] * n), ss, se)
        k = n.bit_length() - 1
        assert counts.sum() == 1 and counts[k << 4] == 1, n
    # runs of every length 1..17 between non-empty blocks, after a block that ends at se and after one that does not
    blocks = []
    for n in range(1, 18):
        blocks += [full] + [empty] * n + [busy] + [empty] * n
    blocks += [full]
    counts = ac_check(gpu, row_of(blocks), ss, se)
    assert counts[0x00] >= 1 and counts[0x10] >= 4 and counts[0x40] >= 3  # runs of 1, 2..3 and 16..18 (the busy block counts)
    # wave and chunk crossings; a block with se coded between two runs; a non-empty tail block followed by empties to the row's end
    p = np.zeros((5 * 8, 300 * 8), dtype=np.int16)
    for bx in range(300):
        put(p, 0, bx, empty if 60 <= bx <= 70 else busy if bx % 3 else full)
        put(p, 1, bx, empty if 250 <= bx <= 262 else full if bx % 2 else busy)
        put(p, 2, bx, full if bx == 130 else empty)
        put(p, 3, bx, busy if bx == 200 else empty)
        put(p, 4, bx, busy if bx in (0, 63, 64, 255, 256, 299) else empty)
    ac_check(gpu, p, ss, se, pad=1)
    ac_check(gpu, p, ss, se, spec=LONG_AC, rows=(1, 3))


@pytest.mark.gpu
def test_the_full_run_split(gpu):
    """a run of 0x7FFF is emitted at once: rows of 32766, 32767, 32768 and 65535 blocks without a level in the band, and 65535 blocks
    with one non-empty block at 40000 (a run of 32767, then 7233 before the block, then 25535 from it to the row's end)"""
    torch = gpu
    big = torch.zeros((8, 65535 * 8), dtype=torch.int16, device="cuda")
    zeros = np.zeros((8, 65535 * 8), dtype=np.int16)
    cases = [(n, None) for n in (32766, 32767, 32768, 65535)] + [(65535, 40000)]
    for n, at in cases:
        host = zeros[:, :n * 8].copy()
        if at is not None:
            put(host, 0, at, zz_block({6: 1, 9: -4}))
        big.zero_()
        big[:, :n * 8] = torch.from_numpy(host).cuda()
        _, counts, _, _ = PE.ac_scan(host, n, 1, 6, 63)
        full = {32766: 0, 32767: 1, 32768: 1}.get(n, 2 if at is None else 1)
        assert counts[0xE0] >= full and (at is None or (counts[0xC0] == 1 and counts[0xE0] == 2))  # 7233 -> EOB12, 25534 -> EOB14
        spec = T.optimal_table(counts)
        want = PE.ac_scan(host, n, 1, 6, 63, spec)[0]
        hist, _ = P.prog_ac_histogram(big, 6, 63, grid=(n, 1))
        assert np.array_equal(hist.cpu().numpy().astype(np.int64), counts), (n, at)
        got = _coded(torch, 1, n, None, 0, lambda seg, sb, ff, un, lo, stride, r0, r1: P.prog_ac_rows(big, 6, 63, spec, seg, sb, ff, un, lo, grid=(n, 1), seg_stride=stride))
        _compare(got, want)
        assert got[3] == 0 and got[4] == 0


@pytest.mark.gpu
def test_band_edges(gpu):
    rng = np.random.default_rng(17)
    p = sparse(rng, (16, 70 * 8), density=0.3)
    for ss, se in ((1, 1), (63, 63), (1, 5), (6, 63), (2, 9), (10, 62)):
        ac_check(gpu, p, ss, se)
    # levels only at 6..63: the band (1, 5) is all empty
    q = p.copy()
    zz = PE.zz_blocks(q, 70, 2)
    zz[:, :, 1:6] = 0
    nat = np.zeros_like(zz)
    nat[:, :, E.ZZ] = zz
    q = nat.reshape(2, 70, 8, 8).transpose(0, 2, 1, 3).reshape(16, 70 * 8).astype(np.int16)
    counts = ac_check(gpu, q, 1, 5)
    assert counts.sum() == 2 and counts[0x60] == 2  # one run of 70 per row
    ac_check(gpu, q, 6, 63)
    # levels at ss and se; zero runs of 15 / 16 / 31 / 32 / 47 inside the band; levels just below ss before a long run; ZRL-worthy zeros
    # before the band's end that become an end of band
    for ss, se in ((1, 63), (6, 63)):
        blocks = [zz_block({ss: 1, se: -1}), zz_block({ss: -1023}), zz_block({se: 1023})]
        for run in (15, 16, 31, 32, 47):
            blocks += [zz_block({ss: 2, ss + run + 1: 3}), zz_block({ss + run: 5}), zz_block({ss - 1: 9, ss + run: -5} if ss > 1 else {ss + run: -5})]
        blocks += [zz_block({ss - 1: 4, ss - 2: 4, 60: 1} if ss > 2 else {60: 1}), zz_block({ss + 3: 7}), zz_block({se - 40: 1}), zz_block({}), zz_block({ss: 1, se - 17: 2})]
        row = row_of(blocks * 15)  # 345 blocks: the cases at both sides of the chunk seam
        counts = ac_check(gpu, row, ss, se)
        assert counts[0xF0] > 0 and counts[0x0A] > 0 and counts[0xF1] + counts[0xF2] + counts[0xF3] > 0
        ac_check(gpu, row, ss, se, spec=LONG_AC)


@pytest.mark.gpu
def test_amplitudes_and_loss(gpu):
    torch = gpu
    rng = np.random.default_rng(23)
    # AC +-1023 are coded; +-1024 are clamped and counted by the statistics and by the coder, inside the band only
    p = sparse(rng, (16, 260 * 8))
    p[3, 5], p[9, 258 * 8 + 1], p[1, 0], p[0, 257 * 8 + 1] = 1023, -1023, 1024, -1024  # positions: (3,5) ..; p[1,0] is zig-zag 2, p[0,1] zig-zag 1
    ac_check(torch, p, 1, 63, lost_want=2)
    ac_check(torch, p, 1, 5, lost_want=2)
    ac_check(torch, p, 6, 63, lost_want=0)
    clamped = np.clip(p, -1023, 1023).astype(np.int16)
    assert np.array_equal(PE.ac_scan(p, 260, 2, 1, 63)[1], PE.ac_scan(clamped, 260, 2, 1, 63)[1])
    # DC differences of +-2047 first, last and at the seam; a step of 2048 is counted
    q = np.zeros((8, 258 * 8), dtype=np.int16)
    q[0, ::8] = np.where(np.arange(258) % 2 == 0, -1024, 1023)
    q[0, 0] = 2047
    q[0, 8] = 0
    counts = dc_check(torch, [q])
    assert counts[0, 11] >= 250
    dc_check(torch, [q], specs=ANNEX_DC[:1])
    q[0, 24] = 1024  # between two blocks at -1024: steps of 2048 and -2048
    dc_check(torch, [q], specs=ANNEX_DC[:1], lost_want=2)
    planes = [sparse(rng, (2 * v * 8, 34 * h * 8), dc=900) for h, v in S420]
    planes[0][0, 8], planes[0][8, 0], planes[0][8, 8], planes[0][0, 16] = 0, 1500, -1500, 0  # Y01, Y10, Y11 of the first MCU, Y00 of the second: one step of -3000
    planes[2][0, 33 * 8], planes[2][0, 32 * 8] = -1024, 1024  # the last two MCUs of Cr's first row, past the seam: -2048
    dc_check(torch, planes, S420, specs=ANNEX_DC, lost_want=2)
    # one dense row of 257 blocks with 16-bit codes: several windows of the ring per chunk
    d = rng.integers(1, 1024, (8, 257 * 8)).astype(np.int16) * rng.choice(np.array([-1, 1], dtype=np.int16), (8, 257 * 8))
    want = PE.ac_scan(d, 257, 1, 1, 63, LONG_AC)[0]
    assert len(want[0]) * 8 > 8 * 32768
    ac_check(torch, d, 1, 63, spec=LONG_AC)
    ac_check(torch, d, 6, 63, spec=LONG_AC)


@pytest.mark.gpu
def test_a_table_that_lacks_a_used_symbol(gpu, monkeypatch):
    torch = gpu
    rng = np.random.default_rng(29)
    p = sparse(rng, (16, 300 * 8), density=0.05)
    p[:, 100 * 8:180 * 8] = 0
    _, counts, _, _ = PE.ac_scan(p, 300, 2, 1, 63)
    eobn = max(s for s in range(0x10, 0xF0, 0x10) if counts[s])
    level = int(np.argmax(counts * (np.arange(256) % 16 != 0)))
    for sym in (eobn, level):
        lacking = counts.copy()
        lacking[sym] = 0
        spec = T.optimal_table(lacking)
        want, _, _, unc = PE.ac_scan(p, 300, 2, 1, 63, spec)
        assert unc == counts[sym] > 0
        d = dev(torch, p)
        got = _coded(torch, 2, 300, None, 0, lambda seg, sb, ff, un, lo, stride, r0, r1: P.prog_ac_rows(d, 1, 63, spec, seg, sb, ff, un, lo, seg_stride=stride))
        assert got[3] == unc and got[4] == 0
        _compare(got, want)  # the symbol is written as its extra bits alone
    # a DC table without a category in use
    _, dcc, _ = PE.dc_scan(dict(width=2400, height=16, comps=[(1, 1)]), [(0, 0)], [p])
    cat = int(np.argmax(dcc[0, :16]))
    lacking = dcc[0, :16].copy()
    lacking[cat] = 0
    d = dev(torch, p)
    got = _coded(torch, 2, 300, None, 0, lambda seg, sb, ff, un, lo, stride, r0, r1: P.prog_dc_rows([d], [(1, 1)], [T.optimal_table(lacking)], seg, sb, ff, un, lo, seg_stride=stride))
    assert got[3] == dcc[0, cat] and got[4] == 0
    # the public layer raises when the tables it is given lack a symbol
    real = P.optimal_table

    def without_eob0(c):
        c = np.array(c, dtype=np.int64)
        if c.size == 256:
            c[0x00] = 0
        return real(c)

    monkeypatch.setattr(P, "optimal_table", without_eob0)
    frame = dict(width=64, height=32, comps=S420)
    planes = make_planes(frame, 5, False)
    with pytest.raises(api.MdctError, match="no code"):
        TC.encode_coefficients([dev(torch, q).contiguous() for q in planes], [[16] * 64] * 3, 64, 32, S420, progressive=True)


def _check_file(out, frame, want_planes, inter, src_colorspace="YCbCr"):
    got, meta = PC.decode(out)
    assert meta["frame"]["sof"] == 0xC2 and (meta["frame"]["width"], meta["frame"]["height"]) == (frame["width"], frame["height"])
    assert [(c[1], c[2]) for c in meta["frame"]["components"]] == [tuple(s) for s in frame["comps"]]
    want = as_written(frame, want_planes, inter)
    for g, w in zip(got, want):
        assert g.shape == w.shape and np.array_equal(g, w)
    dc_scans = [s for s in meta["scans"] if s["se"] == 0]
    assert len(dc_scans) == (1 if inter and len(want) == 3 else len(want))
    for s in meta["scans"]:
        assert s["dri"] == (-(-frame["width"] // (8 * max(h for h, _ in frame["comps"]))) if len(s["comps"]) == 3 else PE.own_grid(frame, s["comps"][0][0])[0])
    return meta


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["grey 8x8", "grey 2056x16 unmarked", "4:4:4 24x40 interleaved DRI 2", "4:2:0 40x24 three scans unmarked", "4:2:0 528x32 interleaved", "4:2:2 48x16",
                                  "Adobe RGB, three tables"])
def test_whole_files(gpu, name):
    Image = pytest.importorskip("PIL.Image")
    from simd_dct_amd import jpeg_decode as D
    from test_jpeg_transcode import _input, _legal_interleaved
    data, frame, planes = _input(name)
    src = jfif.read_jpeg(data, require_restart=False)
    sampling = frame["comps"]
    nc = len(sampling)
    px = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    qtables = [src["qtables"][c["tq"]].astype(np.int64) for c in src["components"]]
    _, coefs = D.decode_coefficients(data)
    for inter in (False, True):
        if inter and not _legal_interleaved(sampling):
            with pytest.raises(ValueError, match="interleaved=True"):
                TC.transcode_jpeg(data, progressive=True, interleaved=True)
            continue
        for bands in (None, CUSTOM[nc]):
            out = TC.encode_coefficients(coefs, qtables, frame["width"], frame["height"], sampling, colorspace=src["colorspace"], progressive=True, interleaved=inter, bands=bands)
            meta = _check_file(out, frame, planes, inter)
            ac = [(s["comps"][0][0], s["ss"], s["se"]) for s in meta["scans"] if s["se"]]
            assert ac == [(ci, ss, se) for ci, b in enumerate(bands or PE.default_bands(nc)) for ss, se in b]
            for k, q in enumerate(qtables):
                assert np.array_equal(np.asarray(meta["qtables"][k], dtype=np.int64), q.reshape(64))
            im = Image.open(io.BytesIO(out))
            assert im.info.get("progressive") and np.array_equal(np.asarray(im.convert("RGB")), px), (name, inter, bands)
            assert (b"Adobe" in out[:40]) == (src["colorspace"] == "RGB")
        out = TC.transcode_jpeg(data, progressive=True, interleaved=inter)
        assert out == TC.encode_coefficients(coefs, qtables, frame["width"], frame["height"], sampling, colorspace=src["colorspace"], progressive=True, interleaved=inter)
    # with a transform: the transposed planes, the swapped frame
    tsamp = [(v, h) for h, v in sampling]
    tframe = dict(width=frame["height"], height=frame["width"], comps=tsamp)
    twant = [np.ascontiguousarray(X.transform(p, "transpose")) for p in planes]
    for inter in (False, True):
        if inter and not _legal_interleaved(tsamp):
            continue
        out = TC.transcode_jpeg(data, transform="transpose", progressive=True, interleaved=inter)
        _check_file(out, tframe, twant, inter)
        base = TC.transcode_jpeg(data, transform="transpose", interleaved=inter)
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(out)).convert("RGB")), np.asarray(Image.open(io.BytesIO(base)).convert("RGB")))
    # without the flag nothing changes
    assert TC.transcode_jpeg(data, progressive=False) == TC.transcode_jpeg(data)


@pytest.mark.gpu
def test_encode_jpeg_progressive(gpu):
    Image = pytest.importorskip("PIL.Image")
    from simd_dct_amd import jpeg_decode as D
    from simd_dct_amd import jpeg_encode as J
    rng = np.random.default_rng(31)
    y, x = np.mgrid[0:40, 0:48]
    colour = np.clip(np.stack([128 + 100 * np.sin(x / 5.0 + c) * np.cos(y / 4.0 - c) for c in range(3)], axis=-1) + rng.normal(0, 20, (40, 48, 3)), 0, 255).astype(np.uint8)
    grey = rng.integers(0, 256, (9, 17)).astype(np.uint8)
    board = (((np.mgrid[0:24, 0:32].sum(axis=0)) % 2) * 255).astype(np.uint8)
    cases = [(colour, q, s) for q in (5, 75, 100) for s in ("4:2:0", "4:4:4")] + [(grey, q, "4:2:0") for q in (5, 75, 100)] + [(board, 100, "4:2:0"), (np.stack([board] * 3, axis=-1), 100, "4:2:2")]
    largest = 0
    for img, q, sub in cases:
        base = J.encode_jpeg(img, quality=q, subsampling=sub, optimize=True)
        _, want = D.decode_jpeg(base, coefficients=True)
        want = [w.cpu().numpy() for w in want]
        largest = max([largest] + [int(np.abs(np.where(np.add.outer(np.arange(w.shape[0]) % 8, np.arange(w.shape[1]) % 8) == 0, 0, w)).max()) for w in want])
        H, W = img.shape[:2]
        frame = dict(width=W, height=H, comps=J.sampling_of(sub, img.ndim == 2))
        for kw in (dict(), dict(optimize=True), dict(interleaved=True)):
            out = J.encode_jpeg(img, quality=q, subsampling=sub, progressive=True, **kw)
            got, meta = PC.decode(out)
            inter = bool(kw.get("interleaved")) and img.ndim == 3
            for g, w, (r, c) in zip(got, want, own_shapes(frame)):
                assert np.array_equal(g[:r, :c], w[:r, :c]), (q, sub, kw)
                if not inter:
                    assert np.array_equal(g, w)
            assert Image.open(io.BytesIO(out)).info.get("progressive")
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(out))), np.asarray(Image.open(io.BytesIO(base))))
        assert J.encode_jpeg(img, quality=q, subsampling=sub, progressive=False, optimize=True) == base
    # the checkerboard is the sign pattern of the basis function (7, 7): its level at a table entry of 1 is 127.5 / 4 * (sum |cos((2x + 1) 7 pi / 16)|)^2 =
    # 837, the largest AC level of these cases -- 8-bit pixels and integer tables stay inside +-1023, the coders' clamp is a guard
    assert 830 <= largest <= 1023, largest


@pytest.mark.gpu
def test_the_four_calls_in_a_captured_graph(gpu):
    torch = gpu
    rng = np.random.default_rng(41)
    p = sparse(rng, (24, 300 * 8), density=0.05)
    p[:, 90 * 8:140 * 8] = 0
    frame = dict(width=2400, height=24, comps=[(1, 1)])
    _, dcc, _ = PE.dc_scan(frame, [(0, 0)], [p])
    _, acc, _, _ = PE.ac_scan(p, 300, 3, 6, 63)
    dspec, aspec = T.optimal_table(dcc[0, :16]), T.optimal_table(acc)
    want_dc = PE.dc_scan(frame, [(0, 0)], [p], {0: dspec})[0]
    want_ac = PE.ac_scan(p, 300, 3, 6, 63, aspec)[0]
    d = torch.zeros((24, 2400), dtype=torch.int16, device="cuda")
    stride = TC.opt_seg_stride(300)
    dch = torch.full((2, 272), -1, dtype=torch.int32, device="cuda")
    ach = torch.full((256,), -1, dtype=torch.int32, device="cuda")
    words = torch.zeros((2,), dtype=torch.int32, device="cuda")
    segs = torch.zeros((2, 3 * stride), dtype=torch.uint8, device="cuda")
    counts = torch.zeros((2, 2, 3), dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        P.prog_dc_histogram([d], [(1, 1)], hist=dch, unrepresentable=words[1:2], stream=s)
        P.prog_ac_histogram(d, 6, 63, hist=ach, unrepresentable=words[1:2], stream=s)
        P.prog_dc_rows([d], [(1, 1)], [dspec], segs[0], counts[0][0], counts[0][1], words[0:1], words[1:2], seg_stride=stride, stream=s)
        P.prog_ac_rows(d, 6, 63, aspec, segs[1], counts[1][0], counts[1][1], words[0:1], words[1:2], seg_stride=stride, stream=s)
    d.copy_(torch.from_numpy(p).cuda())
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(dch.cpu().numpy().astype(np.int64), dcc) and np.array_equal(ach.cpu().numpy().astype(np.int64), acc) and words.cpu().tolist() == [0, 0]
    sg, c = segs.cpu().numpy(), counts.cpu().numpy()
    for k, want in enumerate((want_dc, want_ac)):
        for r in range(3):
            assert sg[k, r * stride:r * stride + c[k, 0, r]].tobytes() == want[r] and c[k, 1, r] == want[r].count(b"\xff"), (k, r)
