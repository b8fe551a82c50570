"""JPEG encoding with Huffman tables made for the image: libmdct_jpegenc_opt.so (include/mdct_jpegenc_opt.h), jpeg_encode.symbol_histogram,
optimal_tables, opt_rows, opt_scan_rows and encode_jpeg(optimize=True).

The expected values everywhere come from the CPU side: the checker's planes (tests/jpeg_encode_checker.py), the oracle's coefficients of
each plane (tests/oracle.py u8_i16, level shift on), tests/jpeg_optimal_tables.py (the symbol walk and the table procedure, written from
T.81 K.2 and libjpeg's description) and tests/jpeg_scan_encoder.py coding the coefficients with the tables.

CPU: the table function against Pillow's optimize=True DHT segments and against the Python statement on constructed histograms; the
C-ABI's refusals; encode_jpeg's argument check; the code objects; the segment stride.
GPU: the histogram in every instantiation; the coders' segments with optimal, Annex K and long-code tables; encode_jpeg(optimize=True)
in the three scan forms through decode_jpeg, the decode checker and Pillow; sizes; the uncoded-symbol status; the packing retry."""
import io
import os

import numpy as np
import pytest

import jpeg_decode_checker as DC
import jpeg_encode_checker as C
import jpeg_optimal_tables as T
import jpeg_scan_encoder as E
import oracle as O
from simd_dct_amd import _jpegenc_opt_lib, _jpegenc_scan_lib, api, jfif

Image = pytest.importorskip("PIL.Image")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT_LIB = os.path.join(ROOT, "simd_dct_amd", "libmdct_jpegenc_opt.so")
SUBS = ["4:4:4", "4:2:2", "4:2:0"]
PIL_SUB = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}
FORMS = ["grey", "three", "interleaved"]
LAYOUT = {"grey": "0, 0", "4:4:4": "1, 1", "4:2:2": "2, 1", "4:2:0": "2, 2"}
KERNELS = {f"k_opt<{hv}, {st}>" for hv in LAYOUT.values() for st in ("true", "false")}
ANNEX = {0: E.ANNEX_K[(0, 0)], 1: E.ANNEX_K[(1, 0)], 2: E.ANNEX_K[(0, 1)], 3: E.ANNEX_K[(1, 1)]}
SCAN3 = [(0, 0, 0), (1, 1, 1), (2, 1, 1)]


def especs(specs):
    """{which: spec} -> jpeg_scan_encoder's {(class, id): spec}"""
    return {(w & 1, w >> 1): (list(b), list(v)) for w, (b, v) in specs.items()}


def unstuff(data):
    return bytes(data).replace(b"\xff\x00", b"\xff")


def pillow_picture(W=168, H=120, seed=1, noise=12):
    """smooth plus noise, RGB"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([128 + 100 * np.sin(x / 23.0 + c) * np.cos(y / 17.0 - c) for c in range(3)], axis=-1)
    return np.clip(base + rng.normal(0, noise, (H, W, 3)), 0, 255).astype(np.uint8)


def pillow_file(img, q, sub=None, **kw):
    b = io.BytesIO()
    args = dict(quality=q, optimize=True, restart_marker_rows=1)
    if sub is not None:
        args["subsampling"] = PIL_SUB[sub]
    args.update(kw)
    Image.fromarray(img).save(b, "JPEG", **args)
    return b.getvalue()


# ------------------------------------------------------------------------------------------ CPU: the table function
def check_table(counts, bits, vals):
    """what every optimal table must satisfy"""
    counts = list(counts)
    assert sum(bits) == len(vals) and sorted(vals) == [s for s, c in enumerate(counts) if c], "exactly the symbols with non-zero counts"
    kraft = sum(n << (16 - l) for l, n in enumerate(bits, 1))
    assert kraft < 1 << 16, "Kraft's sum below 1"
    codes = E.canonical_codes(bits, vals)
    longest = max(n for _, n in codes.values())
    assert all(not (n == longest and code == (1 << n) - 1) for code, n in codes.values()), "the all-ones code of the longest length is unused"


def tables_check(spec, ac):
    from simd_dct_amd import jpeg_decode as D
    s = (list(spec[0]), list(spec[1]))
    return D.tables_check([None, None, s, None] if ac else [s, None, None, None])


def test_table_against_pillows_optimized_files():
    from simd_dct_amd import jpeg_encode as J
    pic = pillow_picture()
    noise = np.random.default_rng(3).integers(0, 256, (64, 64, 3), dtype=np.uint8)
    files = [pillow_file(pic, 75, "4:2:0"), pillow_file(pic, 95, "4:4:4"), pillow_file(pic, 20, "4:2:2"), pillow_file(pic, 100, "4:2:0"),
             pillow_file(noise, 100, "4:4:4"), pillow_file(pic[..., 0], 75)]
    n = 0
    for f in files:
        hist, dht = T.histogram_of_file(f)
        grey = len(dht) == 2
        assert len(dht) == (2 if grey else 4)
        ours = J.optimal_tables(hist, grey=grey)
        for which, (bits, vals) in dht.items():
            cls, ac = which >> 1, which & 1
            assert ours[which] == (bits, vals), (len(f), which)
            assert T.optimal_table(hist[cls][16:] if ac else hist[cls][:16]) == (bits, vals), (len(f), which)
            n += 1
    assert n == 22
    # the figures of the size claim: the same picture with the Annex K tables is a tenth larger
    b = io.BytesIO()
    Image.fromarray(pic).save(b, "JPEG", quality=75, subsampling=2, restart_marker_rows=1)
    assert len(files[0]) < 0.92 * len(b.getvalue())


def _constructed():
    fib = [1, 1]
    while len(fib) < 256:
        fib.append(min(fib[-1] + fib[-2], 0xFFFFFFFF))
    rng = np.random.default_rng(8)
    yield "one symbol", [0] * 5 + [7] + [0] * 250
    yield "one symbol of count 1", [0] * 255 + [1]
    yield "two symbols", [0, 3] + [0] * 100 + [3] + [0] * 153
    yield "fibonacci, 256 symbols", fib
    yield "fibonacci, 40 symbols spread", [fib[i // 6] if i % 6 == 0 and i < 240 else 0 for i in range(256)]
    yield "fibonacci descending", fib[::-1]
    yield "near 2^32", [0xFFFFFFFF - i for i in range(256)]
    yield "near 2^32 and ones", [0xFFFFFFFF if i % 2 else 1 for i in range(256)]
    yield "all equal", [5] * 256
    yield "random", rng.integers(0, 1000, 256).tolist()
    yield "random sparse", (rng.integers(0, 1000, 256) * (rng.random(256) < 0.2)).tolist()
    yield "DC class of 12", [10, 200, 300, 150, 80, 40, 20, 10, 5, 2, 1, 1]
    yield "DC class of 12, ties", [4] * 12
    yield "DC class of 16", [9, 0, 3, 0, 0, 1, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0]


def test_table_against_the_python_statement():
    from simd_dct_amd import jpeg_encode as J
    limited = False
    for name, counts in _constructed():
        bits, vals = J.optimal_table(counts)
        assert (bits, vals) == T.optimal_table(counts), name
        check_table(counts, bits, vals)
        ac = len(counts) == 256
        if all(((s & 15) <= 10 if ac else s <= 11) for s in vals):  # baseline symbols only: the decoder's check takes it
            assert tables_check((bits, vals), ac) == 0, name
        if name.startswith("one symbol"):
            assert bits == [1] + [0] * 15 and len(vals) == 1
        if name == "two symbols":
            assert sum(bits) == 2 and bits[0] == 1 and bits[1] == 1  # 0, 10; 11 stays with the reserved symbol
        limited = limited or (name.startswith("fibonacci") and bits[15] > 0)
    assert limited, "no case reached 16 bits: Figure K.3 was not exercised"
    # Annex K statistics do not exist, but a table for counts made from the Annex K lengths must not be longer than Annex K
    counts = [0] * 256
    for s, (_, n) in E.canonical_codes(*E.ANNEX_K[(1, 0)]).items():
        counts[s] = 1 << (17 - n)
    bits, vals = J.optimal_table(counts)
    got = E.canonical_codes(bits, vals)
    want = E.canonical_codes(*E.ANNEX_K[(1, 0)])
    assert sum(counts[s] * got[s][1] for s in got) <= sum(counts[s] * want[s][1] for s in want)
    assert tables_check((bits, vals), True) == 0


def test_histogram_helper_agrees_with_the_scan_encoder():
    """tests/jpeg_optimal_tables.histogram against the statistics jpeg_scan_encoder.encode_scan keeps of its own walk"""
    rng = np.random.default_rng(2)
    frame = dict(width=48, height=32, comps=C.SAMPLING["4:2:0"])  # on the MCU grid: both forms code the same blocks
    planes = [(rng.integers(-40, 41, s) * (rng.random(s) < 0.15)).astype(np.int16) for s in E.plane_shapes(frame)]
    scan = dict(comps=SCAN3, dri=3)
    _, st = E.encode_scan(frame, scan, planes, E.ANNEX_K)
    h = T.histogram(frame, [scan], planes)
    assert {s: int(h[:, 16 + s].sum()) for s in range(256) if h[:, 16 + s].sum()} == dict(st["ac_symbols"])
    assert {s for s in range(16) if h[:, s].sum()} == st["dc_categories"]
    assert h[:, :16].sum() == st["blocks"]
    # the DC categories depend on the scan form, the AC symbols do not
    per = [dict(comps=[c], dri=0) for c in SCAN3]
    h3 = T.histogram(frame, per, planes)
    assert np.array_equal(h3[:, 16:], h[:, 16:]) and not np.array_equal(h3[:, :16], h[:, :16])


# ------------------------------------------------------------------------------------------ CPU: refusals, code objects
def _plane(px, pitch, w, h, hh=1, vv=1):
    return _jpegenc_scan_lib.Plane(px, pitch, w, h, hh, vv)


class _S:
    def __init__(self, bits, vals, nvals=None):
        self.b = np.asarray(bits, dtype=np.uint8)
        self.v = np.asarray(list(vals) + [0], dtype=np.uint8)
        self.spec = _jpegenc_opt_lib.Spec(self.b.ctypes.data, self.v.ctypes.data, len(vals) if nvals is None else nvals)


def test_seg_stride_covers_the_worst_block():
    lib = _jpegenc_opt_lib.load()
    worst_bits = (16 + 11) + 63 * (16 + 10)
    assert worst_bits == 1665 and worst_bits > 208 * 8
    for blocks in (1, 2, 3, 4, 5, 64, 1023, 1024, 6 * 512, 65536):
        s = int(lib.mdct_jpegenc_opt_seg_stride(blocks))
        assert s == -(-(209 * blocks + 8) // 4) * 4
        # the coder writes whole 32-bit words: the bytes of the longest segment rounded up to one, and the padded last word
        assert s >= -(-(blocks * worst_bits) // 32) * 4 + 4


def test_cabi_refusals_without_device():
    lib = _jpegenc_opt_lib.load()
    A, OUT, SB, FF, UN, HI = 1 << 40, 1 << 44, 1 << 45, 1 << 46, 1 << 47, 1 << 48  # nothing is dereferenced
    lut = np.full(64, 16, dtype=np.float32)

    def bad_lut(i, v):
        t = lut.copy()
        t[i] = v
        return t

    err = lambda: lib.mdct_jpegenc_opt_last_error().decode()
    # ---- the table function
    bits, vals, n = np.zeros(16, np.uint8), np.zeros(256, np.uint8), _jpegenc_opt_lib.c_int()
    ok, zeros = np.arange(1, 257, dtype=np.uint32), np.zeros(256, dtype=np.uint32)
    assert lib.mdct_jpegenc_opt_table(ok.ctypes.data, 256, bits.ctypes.data, vals.ctypes.data, n) == 0
    for name, args in {"null counts": (None, 256, bits.ctypes.data, vals.ctypes.data, n), "null bits": (ok.ctypes.data, 256, None, vals.ctypes.data, n),
                       "null vals": (ok.ctypes.data, 256, bits.ctypes.data, None, n), "null nvals": (ok.ctypes.data, 256, bits.ctypes.data, vals.ctypes.data, None),
                       "11 symbols": (ok.ctypes.data, 11, bits.ctypes.data, vals.ctypes.data, n), "17 symbols": (ok.ctypes.data, 17, bits.ctypes.data, vals.ctypes.data, n),
                       "255 symbols": (ok.ctypes.data, 255, bits.ctypes.data, vals.ctypes.data, n), "0 symbols": (ok.ctypes.data, 0, bits.ctypes.data, vals.ctypes.data, n),
                       "all zero": (zeros.ctypes.data, 256, bits.ctypes.data, vals.ctypes.data, n),
                       "all zero DC": (zeros.ctypes.data, 12, bits.ctypes.data, vals.ctypes.data, n)}.items():
        assert lib.mdct_jpegenc_opt_table(*args) == 1 and err(), name
    # ---- statistics
    p420 = [_plane(A, 64, 64, 32, 2, 2), _plane(A + (1 << 30), 32, 32, 16), _plane(A + (2 << 30), 32, 32, 16)]

    def stats(planes=p420, n=3, luma=lut, chroma=lut, inter=1, hist=HI):
        arr = None if planes is None else (_jpegenc_scan_lib.Plane * max(1, len(planes)))(*planes)
        return lib.mdct_jpegenc_opt_stats(arr, n, None if luma is None else luma.ctypes.data, None if chroma is None else chroma.ctypes.data, inter, hist, None)

    for name, kw in {"null planes": dict(planes=None), "null plane": dict(planes=[p420[0], _plane(0, 32, 32, 16), p420[2]]), "null luma": dict(luma=None),
                     "null chroma": dict(chroma=None), "null hist": dict(hist=None), "hist unaligned": dict(hist=HI + 2), "two planes": dict(n=2), "no planes": dict(n=0),
                     "interleaved 2": dict(inter=2), "interleaved -1": dict(inter=-1), "4:1:1": dict(planes=[_plane(A, 128, 128, 16, 4, 1), p420[1], p420[2]]),
                     "luma off the MCU grid": dict(planes=[_plane(A, 64, 64, 24, 2, 2), p420[1], p420[2]]),
                     "three scans, width 20": dict(inter=0, planes=[_plane(A, 64, 20, 32), p420[1], p420[2]]),
                     "three scans, empty": dict(inter=0, planes=[_plane(A, 64, 64, 0), p420[1], p420[2]]),
                     "three scans, pitch": dict(inter=0, planes=[p420[0], _plane(A, 31, 32, 16), p420[2]]),
                     "three scans, too wide": dict(inter=0, planes=[_plane(A, 1 << 17, 65544, 8), p420[1], p420[2]]),
                     "grey null": dict(n=1, planes=[_plane(0, 64, 64, 32)]), "grey height 12": dict(n=1, planes=[_plane(A, 64, 64, 12)]),
                     "zero luma entry": dict(luma=bad_lut(3, 0.0)), "NaN chroma entry": dict(chroma=bad_lut(9, np.nan))}.items():
        assert stats(**kw) == 1 and err(), name
    # ---- the coders
    k = {w: _S(*ANNEX[w]) for w in range(4)}
    stride = int(lib.mdct_jpegenc_opt_seg_stride(8))

    def rows(px=A, pitch=64, t=lut, W=64, H=32, by0=0, by1=4, dc=k[0], ac=k[1], out=OUT, seg_stride=stride, sb=SB, ff=FF, un=UN):
        return lib.mdct_jpegenc_opt_rows(px, pitch, None if t is None else t.ctypes.data, W, H, by0, by1, None if dc is None else dc.spec, None if ac is None else ac.spec,
                                         out, seg_stride, sb, ff, un, None)

    over = [0] * 16
    over[1] = 5  # five codes of two bits
    twice = (list(ANNEX[0][0]), [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 10])
    ones = [0] * 16
    ones[0] = 2  # both one-bit codes: the second is all ones
    for name, kw in {"null plane": dict(px=None), "null table": dict(t=None), "null out": dict(out=None), "null seg_bytes": dict(sb=None), "null ff_counts": dict(ff=None),
                     "null uncoded": dict(un=None), "uncoded unaligned": dict(un=UN + 1), "null DC": dict(dc=None), "null AC": dict(ac=None), "width 60": dict(W=60),
                     "height 0": dict(H=0), "pitch": dict(pitch=63), "by0 == by1": dict(by0=2, by1=2), "by1 beyond": dict(by1=5),
                     "the Annex K stride": dict(seg_stride=208 * 8 + 8), "stride not a multiple of 4": dict(seg_stride=stride + 2), "out unaligned": dict(out=OUT + 1),
                     "zero table entry": dict(t=bad_lut(0, 0.0)), "over-subscribed": dict(dc=_S(over, range(5))), "all-ones code": dict(dc=_S(ones, [0, 1])),
                     "counts and values disagree": dict(dc=_S(ANNEX[0][0], ANNEX[0][1], nvals=11)), "no values": dict(dc=_S([0] * 16, [])),
                     "257 values": dict(ac=_S([0] * 15 + [255], range(255), nvals=257)), "DC category 12": dict(dc=_S(ANNEX[0][0], list(range(11)) + [12])),
                     "AC size 11": dict(ac=_S(ANNEX[1][0], [0x0B] + list(ANNEX[1][1][1:]))), "a symbol twice": dict(dc=_S(*twice)),
                     "AC table as DC": dict(dc=k[1])}.items():
        assert rows(**kw) == 1 and err(), name

    def scan(planes=p420, n=3, luma=lut, chroma=lut, specs=(k[0], k[1], k[2], k[3]), my0=0, my1=2, out=OUT, seg_stride=int(lib.mdct_jpegenc_opt_seg_stride(24)), sb=SB, ff=FF,
             un=UN):
        arr = None if planes is None else (_jpegenc_scan_lib.Plane * max(1, len(planes)))(*planes)
        sp = None if specs is None else (_jpegenc_opt_lib.Spec * 4)(*[s.spec for s in specs])
        return lib.mdct_jpegenc_opt_scan_rows(arr, n, None if luma is None else luma.ctypes.data, None if chroma is None else chroma.ctypes.data, sp, my0, my1, out,
                                              seg_stride, sb, ff, un, None)

    for name, kw in {"null planes": dict(planes=None), "null specs": dict(specs=None), "one plane": dict(n=1), "null uncoded": dict(un=None), "null chroma": dict(chroma=None),
                     "4:4:0": dict(planes=[_plane(A, 32, 32, 32, 1, 2), p420[1], p420[2]]), "my1 beyond": dict(my1=3), "my0 == my1": dict(my0=1, my1=1),
                     "the Annex K stride": dict(seg_stride=208 * 24 + 8), "the 4:2:2 stride": dict(seg_stride=int(lib.mdct_jpegenc_opt_seg_stride(16))),
                     "out unaligned": dict(out=OUT + 2), "DC and AC swapped": dict(specs=(k[1], k[0], k[2], k[3])), "chroma AC over-subscribed": dict(specs=(k[0], k[1], k[2], _S(over, range(5)))),
                     "NaN luma entry": dict(luma=bad_lut(63, np.nan))}.items():
        assert scan(**kw) == 1 and err(), name


def test_encode_jpeg_refuses_optimize_that_is_not_a_bool(monkeypatch):
    from simd_dct_amd import jpeg_encode as J

    def no_device(*a, **k):
        raise AssertionError("device work before the arguments were checked")

    for name in ("to_planes", "scan_rows", "_run_scan", "symbol_histogram", "opt_rows", "opt_scan_rows"):
        monkeypatch.setattr(J, name, no_device)
    img = np.zeros((16, 16, 3), dtype=np.uint8)
    for bad in (1, 0, None, "yes", 1.0, [True]):
        for kw in (dict(), dict(interleaved=True)):
            with pytest.raises(ValueError):
                J.encode_jpeg(img, optimize=bad, **kw)
        with pytest.raises(ValueError):
            J.encode_jpeg(img[..., 0], optimize=bad)
    for kw in (dict(quality=0), dict(subsampling="4:1:1"), dict(layout="HCW"), dict(interleaved=1)):
        with pytest.raises(ValueError):
            J.encode_jpeg(img, optimize=True, **kw)
    monkeypatch.undo()
    with pytest.raises(ValueError):
        J.symbol_histogram([], [], (None, None), interleaved=1)


def test_code_objects_hold_the_planned_instantiations():
    from test_kernel_coverage import code_object_kernels
    names, n_objects = code_object_kernels(lib=OPT_LIB)
    assert n_objects == 1 and names == KERNELS, sorted(names ^ KERNELS)
    # the libraries beside it list what they listed before
    scan, _ = code_object_kernels(lib=os.path.join(ROOT, "simd_dct_amd", "libmdct_jpegenc_scan.so"))
    assert scan == {"k_scan_rows<1, 1>", "k_scan_rows<2, 1>", "k_scan_rows<2, 2>"}
    enc, _ = code_object_kernels(lib=os.path.join(ROOT, "simd_dct_amd", "libmdct_jpegenc.so"))
    assert len(enc) == 7 and all(n.startswith("k_") for n in enc), sorted(enc)
    hip, _ = code_object_kernels(lib=os.path.join(ROOT, "simd_dct_amd", "libmdct_hip.so"))
    assert not any("k_opt" in n for n in hip) and any(n.startswith("k_px_huffman_rows") for n in hip)


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
    ran = {k: v for k, v in api.kernel_counts().items() if k.startswith("k_opt")}
    assert ran == want, (want, ran)


def _content(W, H, content, seed, grey=False):
    from simd_dct_amd import synth
    if content == "photo":
        img = np.stack([synth.plane_u8_np(W, H, "photo", seed=seed + s) for s in range(3)], axis=-1)
    elif content == "flat":
        img = np.full((H, W, 3), 77, dtype=np.uint8)
        img[..., 1] = 200
    else:
        img = np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
    return img[..., 0].copy() if grey else img


def _grid(W, H, sampling, interleaved):
    """[(padded width, padded height)] per component of the form: the MCU grid, or each component's own block grid"""
    hmax, vmax = max(h for h, _ in sampling), max(v for _, v in sampling)
    if interleaved:
        mx, my = -(-W // (8 * hmax)), -(-H // (8 * vmax))
        return [(mx * 8 * h, my * 8 * v) for h, v in sampling]
    return [(-(-cw // 8) * 8, -(-ch // 8) * 8) for cw, ch in C.true_sizes(W, H, sampling)]


class Case:
    """an image in one of the three forms, with everything the CPU side says about it"""

    def __init__(self, W, H, form, sub, q, content="random", seed=0):
        from simd_dct_amd import jpeg_encode as J
        self.W, self.H, self.form, self.sub, self.q = W, H, form, sub, q
        self.grey, self.inter = form == "grey", form == "interleaved"
        self.host = _content(W, H, content, seed, self.grey)
        self.sampling = [(1, 1)] if self.grey else C.SAMPLING[sub]
        self.sizes = _grid(W, H, self.sampling, self.inter)
        self.luts = J.quality_tables(q)
        self.planes = C.planes(self.host, sub, padded=self.sizes)
        self.coefs = [O.u8_i16("fwd", p, p.shape[1], p.shape[0], lut=np.asarray(self.luts[min(k, 1)], dtype=np.float32), level_shift=True) for k, p in enumerate(self.planes)]
        self.frame = dict(width=W, height=H, comps=self.sampling)
        if self.inter:
            self.scans = [dict(comps=SCAN3, dri=self.sizes[1][0] // 8)]
        else:
            self.scans = [dict(comps=[(ci, min(ci, 1), min(ci, 1))], dri=pw // 8) for ci, (pw, _) in enumerate(self.sizes)]
        self.hist = T.histogram(self.frame, self.scans, self.coefs)

    def device_planes(self, torch, pad=0, offset=0):
        out = []
        for p, (pw, ph) in zip(self.planes, self.sizes):
            pitch = pw + pad
            b = torch.zeros((offset + ph * pitch,), dtype=torch.uint8, device="cuda")
            v = torch.as_strided(b, (ph, pw), (pitch, 1), offset)
            v.copy_(torch.from_numpy(p).cuda())
            out.append(v)
        return out

    def expected_scans(self, specs):
        """[(scan bytes, [un-stuffed data of each interval])] per scan, coded with {which: spec}"""
        sp = especs(specs)
        if self.grey:
            sp = {(0, 0): sp[(0, 0)], (1, 0): sp[(1, 0)]}
        out = []
        for sc in self.scans:
            data, st = E.encode_scan(self.frame, sc, self.coefs, sp)
            out.append((data, [unstuff(data[a:b]) for a, b in st["intervals"]]))
        return out

    def stats_kernels(self):
        if self.inter:
            return {f"k_opt<{LAYOUT[self.sub]}, true>": 1}
        return {"k_opt<0, 0, true>": len(self.sampling)}


def _histogram(torch, case, pad=0, offset=0, calls=1):
    from simd_dct_amd import jpeg_encode as J
    planes = case.device_planes(torch, pad, offset)
    buf = torch.full((8 + 2 * 272 + 8,), -7, dtype=torch.int32, device="cuda")
    hist = buf[8:8 + 544].view(2, 272)
    for _ in range(calls):
        api.kernel_counts_reset()
        got = J.symbol_histogram(planes, case.sampling, case.luts, interleaved=case.inter, hist=hist)
        ran_exactly(torch, case.stats_kernels())
        assert got is hist
        h = buf.cpu().numpy()
        assert (h[:8] == -7).all() and (h[-8:] == -7).all(), "counts written beside the histogram"
        got = h[8:-8].reshape(2, 272).astype(np.int64)
        assert np.array_equal(got, case.hist), (case.form, case.sub, case.W, case.H, case.q, np.argwhere(got != case.hist)[:5].tolist())
    return planes, hist


def _width(form, sub, mcus_x, trim):
    return mcus_x * (16 if form != "grey" and sub != "4:4:4" else 8) - trim


FORM_SUBS = [("grey", "4:4:4")] + [(f, s) for f in ("three", "interleaved") for s in SUBS]


@pytest.mark.gpu
@pytest.mark.parametrize("form,sub", FORM_SUBS)
def test_histogram_chunk_boundaries(gpu, form, sub):
    """1, 2, 31, 32, 33, 65 and 260 MCUs per row through odd image sizes; padded pitches and offset bases; a second call on the same
    buffer counts afresh"""
    for i, (mx, trim, H) in enumerate([(1, 7, 1), (2, 0, 16), (31, 3, 40), (32, 0, 16), (33, 5, 33), (65, 1, 24)]):
        _histogram(gpu, Case(_width(form, sub, mx, trim), H, form, sub, 50, seed=i))
    _histogram(gpu, Case(_width(form, sub, 33, 2), 35, form, sub, 50, seed=10), pad=5, offset=3, calls=2)
    _histogram(gpu, Case(_width(form, sub, 260, 0), 24, form, sub, 75, content="photo", seed=3), pad=1, offset=1)
    if form == "grey":  # a plane wider than one chunk of 256 blocks, and exactly two chunks
        _histogram(gpu, Case(8 * 257 - 3, 17, form, sub, 75, content="photo", seed=4))
        _histogram(gpu, Case(8 * 512, 8, form, sub, 90, seed=5))


@pytest.mark.gpu
@pytest.mark.parametrize("form,sub", FORM_SUBS)
@pytest.mark.parametrize("q", [1, 50, 100])
def test_histogram_contents(gpu, form, sub, q):
    """quality 100 noise: 63 entries per block, saturated levels and every size; quality 1: empty blocks; one colour: EOB alone"""
    _histogram(gpu, Case(_width(form, sub, 70, 4), 50, form, sub, q, seed=q))
    _histogram(gpu, Case(_width(form, sub, 35, 1), 30, form, sub, q, content="flat"))
    c = Case(_width(form, sub, 40, 0), 32, form, sub, q, content="photo", seed=q + 1)
    _histogram(gpu, c)
    if q == 100 and form != "grey":
        assert c.hist[0, 16:].sum() > 0 and c.hist[1, 16 + 0xF0] >= 0


@pytest.mark.gpu
def test_histogram_form_changes_the_dc_categories_only(gpu):
    a, b = Case(320, 64, "three", "4:2:0", 75, content="photo", seed=6), Case(320, 64, "interleaved", "4:2:0", 75, content="photo", seed=6)
    assert np.array_equal(a.hist[:, 16:], b.hist[:, 16:]) and not np.array_equal(a.hist[0, :16], b.hist[0, :16])
    _histogram(gpu, a)
    _histogram(gpu, b)


@pytest.mark.gpu
def test_histogram_in_a_captured_graph(gpu):
    torch = gpu
    from simd_dct_amd import jpeg_encode as J
    for form in ("three", "interleaved"):
        cases = [Case(328, 200, form, "4:2:0", 75, content=c, seed=s) for c, s in (("random", 2), ("photo", 3))]
        planes = cases[0].device_planes(torch)
        hist = torch.full((2, 272), -1, dtype=torch.int32, device="cuda")
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            J.symbol_histogram(planes, cases[0].sampling, cases[0].luts, interleaved=cases[0].inter, hist=hist, stream=s)
        for case in (cases[1], cases[0], cases[0]):
            for d, p in zip(planes, case.planes):
                d.copy_(torch.from_numpy(p).cuda())
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(hist.cpu().numpy().astype(np.int64), case.hist), form


def long_code_specs():
    """every baseline symbol, almost all with codes of 15 and 16 bits"""
    def spec(symbols, short):
        lengths = {s: (3 if i < short else 15 if i % 2 else 16) for i, s in enumerate(symbols)}
        return E.spec_from_lengths(lengths)
    dcs = list(range(12))
    acs = [0x00, 0xF0] + [r << 4 | s for r in range(16) for s in range(1, 11)]
    return {0: spec(dcs, 2), 1: spec(acs, 3), 2: spec(dcs[::-1], 1), 3: spec(acs[::-1], 2)}


def _coders(torch, case, specs, uncoded_want=0, rows=None, extra_stride=0, pad=0, offset=0, planes=None):
    """the coder of the case's form with {which: spec} into canary-filled buffers: every segment, byte count and 0xFF count against
    jpeg_scan_encoder's interval; nothing written past a segment's last word, in rows not asked for, or beside the arrays.
    Returns [(segments, counts, stride, intervals)] per scan."""
    from simd_dct_amd import jpeg_encode as J
    planes = planes or case.device_planes(torch, pad, offset)
    want = case.expected_scans(specs) if uncoded_want == 0 else None
    uncoded = torch.zeros((3,), dtype=torch.int32, device="cuda")
    out = []
    for si, sc in enumerate(case.scans):
        n = case.sizes[1 if case.inter else si][1] // 8
        blocks = sc["dri"] * (sum(h * v for h, v in case.sampling) if case.inter else 1)
        stride = J.opt_seg_stride(blocks) + extra_stride
        seg = torch.full((n * stride + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
        counts = torch.full((2, n + 8), -7, dtype=torch.int32, device="cuda")
        r0, r1 = rows if rows is not None else (0, n)
        r1 = min(r1, n)
        api.kernel_counts_reset()
        if case.inter:
            J.opt_scan_rows(planes, case.sampling, case.luts, specs, seg, counts[0], counts[1], uncoded[1:2], seg_stride=stride, my0=r0, my1=r1)
            ran_exactly(torch, {f"k_opt<{LAYOUT[case.sub]}, false>": 1})
        else:
            cls = min(si, 1)
            J.opt_rows(planes[si], case.luts[cls], (specs[2 * cls], specs[2 * cls + 1]), seg, counts[0], counts[1], uncoded[1:2], seg_stride=stride, by0=r0, by1=r1)
            ran_exactly(torch, {"k_opt<0, 0, false>": 1})
        s, c = seg.cpu().numpy(), counts.cpu().numpy()
        assert (s[n * stride:] == 0xA5).all() and (c[:, n:] == -7).all(), "bytes written after the buffers"
        for r in range(n):
            row = s[r * stride:(r + 1) * stride]
            if not r0 <= r < r1:
                assert (row == 0xA5).all() and c[0, r] == -7 and c[1, r] == -7, f"row {r} outside [{r0}, {r1}) was touched"
                continue
            if want is None:
                continue
            w = want[si][1][r]
            assert c[0, r] == len(w), (case.form, case.sub, si, r, int(c[0, r]), len(w))
            assert row[:len(w)].tobytes() == w, (case.form, case.sub, si, r)
            assert c[1, r] == w.count(b"\xff"), (case.form, case.sub, si, r)
            assert (row[-(-len(w) // 4) * 4:] == 0xA5).all(), f"row {r}: bytes written beyond the segment's last word"
        out.append((seg, counts, stride, n))
    u = uncoded.cpu().numpy()
    assert u[0] == 0 and u[2] == 0, "words beside `uncoded` were written"
    assert (u[1] == 0) if uncoded_want == 0 else (u[1] > 0 if uncoded_want is True else u[1] == uncoded_want), (int(u[1]), uncoded_want)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("form,sub", FORM_SUBS)
def test_coders_with_optimal_annex_k_and_long_tables(gpu, form, sub):
    torch = gpu
    from simd_dct_amd import jpeg_encode as J
    for i, (mx, trim, H, q, content) in enumerate([(33, 5, 33, 50, "random"), (65, 1, 24, 100, "random"), (260, 0, 16, 75, "photo"), (1, 7, 1, 1, "random")]):
        case = Case(_width(form, sub, mx, trim), H, form, sub, q, content=content, seed=20 + i)
        optimal = T.specs_of(case.hist, grey=case.grey)
        if case.grey:
            optimal.update({2: optimal[0], 3: optimal[1]})
        for name, specs in (("optimal", optimal), ("Annex K", ANNEX), ("long", long_code_specs())):
            res = _coders(torch, case, specs, pad=3 * (i & 1), offset=i & 1, extra_stride=64 * (i == 2))
            if name != "Annex K":
                continue
            # the existing coders write the same segments
            planes = case.device_planes(torch)
            for si, (seg, counts, stride, n) in enumerate(res):
                if case.inter:
                    st0 = J.scan_seg_stride(case.scans[0]["dri"], case.sampling)
                    seg0 = torch.zeros((n * st0,), dtype=torch.uint8, device="cuda")
                    c0 = torch.zeros((2, n), dtype=torch.int32, device="cuda")
                    J.scan_rows(planes, case.sampling, case.luts, seg0, c0[0], c0[1], seg_stride=st0)
                else:
                    pw, ph = case.sizes[si]
                    st0 = api.huffman_seg_stride(pw)
                    seg0 = torch.zeros((n * st0,), dtype=torch.uint8, device="cuda")
                    c0 = torch.zeros((2, n), dtype=torch.int32, device="cuda")
                    api.fwd_u8_huffman_rows(planes[si], pw, ph, seg0, c0[0], lut=case.luts[min(si, 1)], chroma=si > 0, seg_stride=st0, pitch=planes[si].stride(0), ff_counts=c0[1])
                assert torch.equal(c0, counts[:, :n])
                a, b, nb = seg.cpu().numpy(), seg0.cpu().numpy(), c0[0].cpu().numpy()
                assert all(a[r * stride:r * stride + nb[r]].tobytes() == b[r * st0:r * st0 + nb[r]].tobytes() for r in range(n))


@pytest.mark.gpu
@pytest.mark.parametrize("form,sub", [("grey", "4:4:4"), ("interleaved", "4:2:0"), ("three", "4:2:2")])
def test_coders_sub_range_and_worst_case(gpu, form, sub):
    case = Case(_width(form, sub, 40, 1), 100, form, sub, 90, seed=4)
    _coders(gpu, case, ANNEX, rows=(2, 5), pad=3)
    _coders(gpu, case, long_code_specs(), rows=(0, 1))
    # quality 100 noise with the long table: beyond the Annex K coders' 208 bytes per block, several ring windows per chunk
    case = Case(_width(form, sub, 70, 0), 16, form, sub, 100, seed=5)
    res = _coders(gpu, case, long_code_specs())
    per_block = max(int(c[0, :n].max()) / (case.scans[si]["dri"] * (sum(h * v for h, v in case.sampling) if case.inter else 1)) for si, (_, c, _, n) in enumerate(res))
    assert per_block > 150, per_block


@pytest.mark.gpu
@pytest.mark.parametrize("form,sub", [("grey", "4:4:4"), ("interleaved", "4:2:0"), ("three", "4:4:4")])
def test_symbols_without_a_code_are_counted(gpu, form, sub):
    """an ordinary status: the word counts the symbols, the segments stay inside their buffers"""
    case = Case(_width(form, sub, 20, 0), 32, form, sub, 75, content="photo", seed=7)
    full = T.specs_of(case.hist, grey=case.grey)
    if case.grey:
        full.update({2: full[0], 3: full[1]})
    _coders(gpu, case, full)  # complete for this image: 0
    # without EOB in the luminance AC table: exactly the luminance EOBs are uncoded
    bits, vals = full[1]
    lengths = {s: n for s, (_, n) in E.canonical_codes(bits, vals).items() if s != 0x00}
    cut = dict(full)
    cut[1] = E.spec_from_lengths(lengths)
    _coders(gpu, case, cut, uncoded_want=int(case.hist[0, 16]))
    # a DC table of category 0 alone
    cut = dict(full)
    cut[0] = ([1] + [0] * 15, [0])
    _coders(gpu, case, cut, uncoded_want=int(case.hist[0, 1:16].sum()))
    # encode_jpeg raises when the word is not zero
    from simd_dct_amd import jpeg_encode as J
    import unittest.mock
    with unittest.mock.patch.object(J, "optimal_tables", lambda hist, grey=False: cut):
        with pytest.raises(api.MdctError, match="no code"):
            J.encode_jpeg(case.host, quality=75, subsampling=sub, interleaved=case.inter, optimize=True)


def _file_checks(torch, case, f, plain):
    """f = encode_jpeg(optimize=True) of the case, plain = the optimize=False file"""
    from simd_dct_amd import jpeg_decode as D
    specs = T.specs_of(case.hist, grey=case.grey)
    scans = case.expected_scans(specs if not case.grey else {**specs, 2: specs[0], 3: specs[1]})
    comps = [dict(qtable=case.luts[min(k, 1)]) for k in range(len(case.sampling))]
    if case.inter:
        want = jfif.write_jpeg(comps, case.W, case.H, specs=specs, sampling=case.sampling, interleaved=dict(scan=scans[0][0], mcus_per_row=case.scans[0]["dri"]))
    else:
        for c, (data, _), sc in zip(comps, scans, case.scans):
            c.update(scan=data, blocks_per_row=sc["dri"])
        want = jfif.write_jpeg(comps, case.W, case.H, specs=specs, sampling=case.sampling)
    assert f == want, (case.form, case.sub, case.q, len(f), len(want))
    assert len(f) <= len(plain), (len(f), len(plain))
    # its DHT segments are the optimal tables of its own scan
    hist, dht = T.histogram_of_file(f)
    assert np.array_equal(hist, case.hist)
    assert dht == T.specs_of(hist, grey=case.grey)
    # the same coefficients and pixels as the optimize=False file: our decoder, the decode checker, Pillow
    _, c1 = D.decode_jpeg(f, coefficients=True)
    _, c0 = D.decode_jpeg(plain, coefficients=True)
    assert all(torch.equal(a, b) for a, b in zip(c1, c0))
    assert torch.equal(D.decode_jpeg(f, mode="RGB"), D.decode_jpeg(plain, mode="RGB"))
    p1, p0 = DC.decode(f)[0], DC.decode(plain)[0]
    assert all(np.array_equal(a, b) for a, b in zip(p1, p0))
    for a, (pw, ph), w in zip(p1, case.sizes, case.coefs):
        assert np.array_equal(a[:ph, :pw], w[:ph, :pw]) if not case.inter else np.array_equal(a, w)
    im1, im0 = Image.open(io.BytesIO(f)), Image.open(io.BytesIO(plain))
    assert np.array_equal(np.asarray(im1), np.asarray(im0)) and im1.size == (case.W, case.H)


@pytest.mark.gpu
@pytest.mark.parametrize("form,sub", FORM_SUBS)
def test_encode_jpeg_optimize_bit_exact(gpu, form, sub):
    from simd_dct_amd import jpeg_encode as J
    for W, H, q, content, seed in ((33, 31, 50, "random", 1), (1, 1, 75, "random", 2), (17, 9, 100, "random", 3), (168, 120, 75, "photo", 4), (392, 264, 95, "photo", 5),
                                   (200, 50, 20, "photo", 6)):
        case = Case(W, H, form, sub, q, content=content, seed=seed)
        kw = dict(quality=q, subsampling=sub, interleaved=case.inter)
        api.kernel_counts_reset()
        f = J.encode_jpeg(case.host, optimize=True, **kw)
        gpu.cuda.synchronize()
        ran = {k: v for k, v in api.kernel_counts().items() if k.startswith("k_opt")}
        n = 1 if case.inter else len(case.sampling)
        hv = LAYOUT[sub] if case.inter else "0, 0"
        assert ran == {f"k_opt<{hv}, true>": n, f"k_opt<{hv}, false>": n}, ran
        _file_checks(gpu, case, f, J.encode_jpeg(case.host, **kw))
        assert J.encode_jpeg(gpu.from_numpy(case.host).cuda(), optimize=True, **kw) == f
    if form != "grey":
        assert J.encode_jpeg(np.ascontiguousarray(np.moveaxis(case.host, -1, 0)), layout="CHW", optimize=True, **kw) == f


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(1024, 768)])
def test_size_against_pillows_optimized_encode(gpu, W, H):
    """the images, settings and the 5 % of test_jpeg_encode.py::test_against_pillows_encode, both encoders with optimised tables"""
    from simd_dct_amd import jpeg_encode as J
    from simd_dct_amd import synth
    host = np.stack([synth.plane_u8_np(W, H, "photo", seed=s) for s in (21, 22, 23)], axis=-1)
    for sub in SUBS:
        for q in (50, 75, 90):
            for inter in (False, True):
                ours = J.encode_jpeg(host, quality=q, subsampling=sub, interleaved=inter, optimize=True)
                plain = J.encode_jpeg(host, quality=q, subsampling=sub, interleaved=inter)
                theirs = pillow_file(host, q, sub)  # optimize=True, a restart interval per MCU row
                print(f"{sub} q{q} interleaved={inter}: optimize {len(ours)}, plain {len(plain)}, Pillow optimize {len(theirs)}")
                assert len(ours) <= len(plain)
                assert abs(len(ours) - len(theirs)) <= 0.05 * len(theirs), (sub, q, inter, len(ours), len(theirs))
                assert np.array_equal(np.asarray(Image.open(io.BytesIO(ours))), np.asarray(Image.open(io.BytesIO(plain))))


@pytest.mark.gpu
def test_full_frame_through_decode_jpeg(gpu):
    """where the Python scan encoder is too slow: the optimised file decodes to the oracle's coefficients, its tables are legal and it is
    smaller"""
    from simd_dct_amd import jpeg_decode as D
    from simd_dct_amd import jpeg_encode as J
    W, H, sub = 4096, 2176, "4:2:0"
    host = _content(W, H, "photo", 11)
    for inter in (False, True):
        f = J.encode_jpeg(host, quality=75, subsampling=sub, interleaved=inter, optimize=True)
        plain = J.encode_jpeg(host, quality=75, subsampling=sub, interleaved=inter)
        assert len(f) < len(plain)
        info = jfif.read_jpeg(f)
        assert D.tables_check([info["huffman"][(0, 0)], info["huffman"][(0, 1)], info["huffman"][(1, 0)], info["huffman"][(1, 1)]]) == 0
        _, c1 = D.decode_jpeg(f, coefficients=True)
        _, c0 = D.decode_jpeg(plain, coefficients=True)
        assert all(gpu.equal(a, b) for a, b in zip(c1, c0))
        sizes = _grid(W, H, C.SAMPLING[sub], True)
        luma, chroma = J.quality_tables(75)
        for k, (c, p) in enumerate(zip(c1, C.planes(host, sub, padded=sizes))):
            want = O.u8_i16("fwd", p, p.shape[1], p.shape[0], lut=np.asarray(luma if k == 0 else chroma, dtype=np.float32), level_shift=True)
            assert np.array_equal(c.cpu().numpy()[:p.shape[0], :p.shape[1]], want), (k, inter)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_scan_that_does_not_fit_is_packed_again(gpu, form, monkeypatch):
    from simd_dct_amd import jpeg_encode as J
    case = Case(150, 90, form, "4:2:0", 100, seed=9)
    kw = dict(quality=100, subsampling="4:2:0", interleaved=case.inter, optimize=True)
    want = J.encode_jpeg(case.host, **kw)
    _file_checks(gpu, case, want, J.encode_jpeg(case.host, quality=100, subsampling="4:2:0", interleaved=case.inter))
    calls = []
    packer = api.jpeg_pack_rows

    def counted(*a, **k):
        calls.append(a[4].numel())
        return packer(*a, **k)

    monkeypatch.setattr(J, "_first_capacity", lambda pixels: 64)
    monkeypatch.setattr(J.api, "jpeg_pack_rows", counted)
    assert J.encode_jpeg(case.host, **kw) == want
    n = 1 if form != "three" else 3
    assert len(calls) == 2 * n and calls[:n] == [64] * n and all(c > 64 for c in calls[n:])
