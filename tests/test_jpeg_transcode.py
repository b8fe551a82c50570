"""JPEG in the coefficient domain: libmdct_jpegcoef.so (include/mdct_jpegcoef.h), jpeg_transcode.coef_histogram, coef_rows,
coef_scan_rows, transform_planes, encode_coefficients and transcode_jpeg, jpeg_decode.decode_coefficients, jfif.write_jpeg's keywords.

Truth comes from the test side: jpeg_scan_encoder codes known planes with any tables, jpeg_decode_checker decodes files serially,
jpeg_optimal_tables counts symbols and makes tables, jpeg_transform_checker states the seven operations in numpy and idct_reference
holds that statement against a float64 IDCT.

CPU: the statement against pixels; the C-ABI's refusals; the Python layer's refusals before any device work; write_jpeg's old bytes
(pinned) and new keywords; the code object.
GPU: the coders and the histogram at the chunk boundaries of every layout, the ring's window loop with the DC carry, the symbol edge
cases, the loss count, tables of every kind; the seven operations; transcode_jpeg end to end through the checker, decode_jpeg and
Pillow; a captured graph; hostile input."""
import hashlib
import io
import json
import os

import numpy as np
import pytest

import idct_reference as R
import jpeg_decode_checker as DC
import jpeg_optimal_tables as T
import jpeg_scan_encoder as E
import jpeg_transform_checker as X
from simd_dct_amd import _jpegcoef_lib, _jpegenc_opt_lib, api, jfif
from simd_dct_amd import jpeg_transcode as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COEF_LIB = os.path.join(ROOT, "simd_dct_amd", "libmdct_jpegcoef.so")
ANNEX = {0: E.ANNEX_K[(0, 0)], 1: E.ANNEX_K[(1, 0)], 2: E.ANNEX_K[(0, 1)], 3: E.ANNEX_K[(1, 1)]}
SCAN3 = [(0, 0, 0), (1, 1, 1), (2, 1, 1)]
S444, S422, S420 = [(1, 1)] * 3, [(2, 1), (1, 1), (1, 1)], [(2, 2), (1, 1), (1, 1)]
KERNELS = {f"k_coef<{hv}, {st}>" for hv in ("0, 0", "1, 1", "2, 1", "2, 2") for st in ("true", "false")} | {"k_coef_transform"}


def especs(specs):
    """{which: spec} -> jpeg_scan_encoder's {(class, id): spec}"""
    return {(w & 1, w >> 1): (list(b), list(v)) for w, (b, v) in specs.items()}


def unstuff(data):
    return bytes(data).replace(b"\xff\x00", b"\xff")


def sparse(rng, shape, amp=40, density=0.15, dc=200):
    p = (rng.integers(-amp, amp + 1, shape) * (rng.random(shape) < density)).astype(np.int16)
    p[::8, ::8] = rng.integers(-dc, dc + 1, (shape[0] // 8, shape[1] // 8))
    return p


# ------------------------------------------------------------------------------------------ CPU: the statement of the operations
def test_the_numpy_statement_against_pixels():
    """transformed coefficients, dequantised with the (transposed) table and put through the float64 IDCT, are the flipped, transposed
    or rotated pixels of the original: a bound on double rounding, values reach ~1e5"""
    rng = np.random.default_rng(11)
    W, H = 24, 40
    c = rng.integers(-1023, 1024, (H, W)).astype(np.int16)
    q = rng.integers(1, 256, 64)
    px = R.plane(R.idct2(R.dequantise(R.blocks(c), q)), W, H)
    assert np.abs(px).max() > 1e4
    for op in X.OPS:
        t = X.transform(c, op)
        qt = q.reshape(8, 8).T.reshape(64) if op in X.TRANSPOSING else q
        want = X.PIXELS[op](px)
        assert t.shape == want.shape and t.dtype == np.int16, op
        got = R.plane(R.idct2(R.dequantise(R.blocks(t), qt)), t.shape[1], t.shape[0])
        err = np.abs(got - want).max()
        assert err <= 1e-6, (op, err)
    # the compositions the header states
    assert np.array_equal(X.transform(c, "rot180"), X.transform(X.transform(c, "flip_v"), "flip_h"))
    assert np.array_equal(X.transform(c, "rot90"), X.transform(X.transform(c, "transpose"), "flip_h"))
    assert np.array_equal(X.transform(c, "rot270"), X.transform(X.transform(c, "flip_h"), "transpose"))
    assert np.array_equal(X.transform(c, "transverse"), X.transform(X.transform(c, "transpose"), "rot180"))
    assert np.array_equal(X.transform(X.transform(c, "rot90"), "rot270"), c)


# ------------------------------------------------------------------------------------------ CPU: refusals, code object
class _S:
    def __init__(self, bits, vals, nvals=None):
        self.b = np.asarray(bits, dtype=np.uint8)
        self.v = np.asarray(list(vals) + [0], dtype=np.uint8)
        self.spec = _jpegenc_opt_lib.Spec(self.b.ctypes.data, self.v.ctypes.data, len(vals) if nvals is None else nvals)


def _P(coef, pitch, bx, by, h=1, v=1):
    return _jpegcoef_lib.Plane(coef, pitch, bx, by, h, v)


def test_cabi_refusals_without_device():
    lib = _jpegcoef_lib.load()
    A, B, C, OUT, SB, FF, UN, LO, HI = 1 << 40, 1 << 41, 1 << 42, 1 << 44, 1 << 45, 1 << 46, 1 << 47, 1 << 48, 1 << 49  # nothing is dereferenced
    err = lambda: lib.mdct_jpegcoef_last_error().decode()  # noqa: E731
    stride8 = int(_jpegenc_opt_lib.load().mdct_jpegenc_opt_seg_stride(8))
    p420 = [_P(A, 64, 8, 4, 2, 2), _P(B, 32, 4, 2), _P(C, 32, 4, 2)]
    bad_planes = {"null coef": _P(0, 64, 8, 4), "coef misaligned": _P(A + 8, 64, 8, 4), "pitch misaligned": _P(A, 68, 8, 4), "pitch too short": _P(A, 56, 8, 4),
                  "0 blocks wide": _P(A, 64, 0, 4), "0 blocks high": _P(A, 64, 8, 0), "65536 blocks wide": _P(A, 1 << 20, 65536, 4),
                  "65536 blocks high": _P(A, 64, 8, 65536)}

    # ---- statistics
    def stats(planes=p420, n=3, inter=1, hist=HI, lost=LO):
        arr = None if planes is None else (_jpegcoef_lib.Plane * max(1, len(planes)))(*planes)
        return lib.mdct_jpegcoef_stats(arr, n, inter, hist, lost, None)

    cases = {"null planes": dict(planes=None), "null hist": dict(hist=None), "null unrepresentable": dict(lost=None), "hist unaligned": dict(hist=HI + 2),
             "unrepresentable unaligned": dict(lost=LO + 1), "two planes": dict(n=2), "no planes": dict(n=0), "interleaved 2": dict(inter=2), "interleaved -1": dict(inter=-1),
             "4:1:1": dict(planes=[_P(A, 128, 16, 2, 4, 1), p420[1], p420[2]]), "4:4:0": dict(planes=[_P(A, 32, 4, 4, 1, 2), p420[1], p420[2]]),
             "chroma 2x1": dict(planes=[p420[0], _P(B, 32, 4, 2, 2, 1), p420[2]]), "luma off the MCU grid": dict(planes=[_P(A, 64, 8, 3, 2, 2), p420[1], p420[2]]),
             "chroma planes disagree": dict(planes=[p420[0], p420[1], _P(C, 32, 3, 2)])}
    for name, p in bad_planes.items():
        cases["grey " + name] = dict(n=1, inter=0, planes=[p])
        cases["three scans, " + name] = dict(inter=0, planes=[p420[0], p, p420[2]])
    for name, kw in cases.items():
        assert stats(**kw) == 1 and err(), name

    # ---- the coders
    k = {w: _S(*ANNEX[w]) for w in range(4)}
    over = [0] * 16
    over[1] = 5  # five codes of two bits
    ones = [0] * 16
    ones[0] = 2  # both one-bit codes: the second is all ones
    twice = (list(ANNEX[0][0]), [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 10])
    bad_dc = {"null DC": None, "over-subscribed": _S(over, range(5)), "all-ones code": _S(ones, [0, 1]), "counts and values disagree": _S(ANNEX[0][0], ANNEX[0][1], nvals=11),
              "no values": _S([0] * 16, []), "DC category 12": _S(ANNEX[0][0], list(range(11)) + [12]), "a symbol twice": _S(*twice), "AC table as DC": k[1],
              "null counts": type("N", (), {"spec": _jpegenc_opt_lib.Spec(None, k[0].v.ctypes.data, 12)})()}
    bad_ac = {"null AC": None, "257 values": _S([0] * 15 + [255], range(255), nvals=257), "AC size 11": _S(ANNEX[1][0], [0x0B] + list(ANNEX[1][1][1:]))}

    def rows(plane=_P(A, 64, 8, 4), by0=0, by1=4, dc=k[0], ac=k[1], out=OUT, seg_stride=stride8, sb=SB, ff=FF, un=UN, lost=LO):
        return lib.mdct_jpegcoef_rows(plane, by0, by1, None if dc is None else dc.spec, None if ac is None else ac.spec, out, seg_stride, sb, ff, un, lost, None)

    cases = {"null plane": dict(plane=None), "null out": dict(out=None), "null seg_bytes": dict(sb=None), "null ff_counts": dict(ff=None), "null uncoded": dict(un=None),
             "null unrepresentable": dict(lost=None), "uncoded unaligned": dict(un=UN + 1), "unrepresentable unaligned": dict(lost=LO + 2), "by0 == by1": dict(by0=2, by1=2),
             "by1 beyond": dict(by1=5), "the Annex K stride": dict(seg_stride=208 * 8 + 8), "stride not a multiple of 4": dict(seg_stride=stride8 + 2),
             "out unaligned": dict(out=OUT + 1)}
    cases.update({name: dict(plane=p) for name, p in bad_planes.items()})
    cases.update({name: dict(dc=s) for name, s in bad_dc.items()})
    cases.update({name: dict(ac=s) for name, s in bad_ac.items()})
    for name, kw in cases.items():
        assert rows(**kw) == 1 and err(), name

    def scan(planes=p420, n=3, specs=(k[0], k[1], k[2], k[3]), my0=0, my1=2, out=OUT, seg_stride=int(_jpegenc_opt_lib.load().mdct_jpegenc_opt_seg_stride(24)), sb=SB, ff=FF,
             un=UN, lost=LO):
        arr = None if planes is None else (_jpegcoef_lib.Plane * max(1, len(planes)))(*planes)
        sp = None if specs is None else (_jpegenc_opt_lib.Spec * 4)(*[s.spec for s in specs])
        return lib.mdct_jpegcoef_scan_rows(arr, n, sp, my0, my1, out, seg_stride, sb, ff, un, lost, None)

    cases = {"null planes": dict(planes=None), "null specs": dict(specs=None), "null out": dict(out=None), "null seg_bytes": dict(sb=None), "null ff_counts": dict(ff=None),
             "null uncoded": dict(un=None), "null unrepresentable": dict(lost=None), "one plane": dict(n=1), "4:1:1": dict(planes=[_P(A, 128, 16, 2, 4, 1), p420[1], p420[2]]),
             "4:4:0": dict(planes=[_P(A, 32, 4, 4, 1, 2), p420[1], p420[2]]), "chroma 1x2": dict(planes=[p420[0], p420[1], _P(C, 32, 4, 2, 1, 2)]),
             "luma off the MCU grid": dict(planes=[_P(A, 64, 7, 4, 2, 2), p420[1], p420[2]]), "chroma planes disagree": dict(planes=[p420[0], _P(B, 32, 4, 1), p420[2]]),
             "my1 beyond": dict(my1=3), "my0 == my1": dict(my0=1, my1=1), "the Annex K stride": dict(seg_stride=208 * 24 + 8),
             "the 4:2:2 stride": dict(seg_stride=int(_jpegenc_opt_lib.load().mdct_jpegenc_opt_seg_stride(16))), "out unaligned": dict(out=OUT + 2),
             "DC and AC swapped": dict(specs=(k[1], k[0], k[2], k[3])), "chroma AC over-subscribed": dict(specs=(k[0], k[1], k[2], _S(over, range(5))))}
    cases.update({"plane 1 " + name: dict(planes=[p420[0], p, p420[2]]) for name, p in bad_planes.items()})
    cases.update({"chroma " + name: dict(specs=(k[0], k[1], s if s is not None else k[2], k[3])) for name, s in bad_dc.items() if s is not None})
    for name, kw in cases.items():
        assert scan(**kw) == 1 and err(), name

    # ---- the transform
    def xf(src=_P(A, 64, 8, 4), dst=_P(B, 64, 8, 4), op=0):
        return lib.mdct_jpegcoef_transform(src, dst, op, None)

    cases = {"null src": dict(src=None), "null dst": dict(dst=None), "op -1": dict(op=-1), "op 7": dict(op=7), "flip into the swapped grid": dict(dst=_P(B, 64, 4, 8)),
             "transpose into the same grid": dict(op=2, dst=_P(B, 64, 8, 4)), "rot90 into a wider grid": dict(op=4, dst=_P(B, 64, 5, 8)),
             "the same plane": dict(dst=_P(A, 64, 8, 4)), "dst inside src's pitch": dict(src=_P(A, 128, 8, 4), dst=_P(A + 128, 128, 8, 4)),
             "dst begins in src's last row": dict(dst=_P(A + 2 * (31 * 64 + 56), 64, 8, 4)), "a square plane transposed in place": dict(op=2, src=_P(A, 64, 8, 8), dst=_P(A, 64, 8, 8))}
    cases.update({"src " + name: dict(src=p) for name, p in bad_planes.items()})
    cases.update({"dst " + name: dict(dst=p) for name, p in bad_planes.items()})
    for name, kw in cases.items():
        assert xf(**kw) == 1 and err(), name


def _file(W, H, sampling, seed=1, dri=0, interleaved=True, **kw):
    """-> (file, frame, planes): encode_file of sparse planes; a non-interleaved file's planes are zero beyond each component's own grid"""
    rng = np.random.default_rng(seed)
    frame = dict(width=W, height=H, comps=sampling)
    planes = [sparse(rng, s) for s in E.plane_shapes(frame)]
    nc = len(sampling)
    if nc == 1 or not interleaved:
        hmax, vmax = max(h for h, _ in sampling), max(v for _, v in sampling)
        for p, (h, v) in zip(planes, sampling):
            p[-(-(-(-H * v // vmax)) // 8) * 8:, :] = 0
            p[:, -(-(-(-W * h // hmax)) // 8) * 8:] = 0
        scans = [dict(comps=[SCAN3[c]], dri=dri) for c in range(nc)]
    else:
        scans = [dict(comps=SCAN3, dri=dri)]
    data, _ = E.encode_file(frame, scans, planes, E.ANNEX_K, **kw)
    return data, frame, planes


def test_python_refusals_before_any_device_work(monkeypatch):
    from simd_dct_amd import jpeg_decode as D

    def no_device(*a, **k):
        raise AssertionError("device work before the arguments were checked")

    monkeypatch.setattr(D, "decode_coefficients", no_device)
    for name in ("coef_histogram", "coef_rows", "coef_scan_rows", "transform_planes", "encode_coefficients"):
        monkeypatch.setattr(TC, name, no_device)
    f420, _, _ = _file(40, 24, S420)
    f422, _, _ = _file(48, 16, S422)
    grey, _, _ = _file(20, 12, [(1, 1)])
    f440, _, _ = _file(16, 32, [(1, 2), (1, 1), (1, 1)])
    # an imperfect transform without trim names the axis and the remainder
    for op, axis, rem in (("flip_h", "x", 8), ("flip_v", "y", 8), ("rot180", "x", 8), ("transverse", "x", 8), ("rot90", "y", 8), ("rot270", "x", 8)):
        with pytest.raises(ValueError, match=rf"the {axis} axis.*remainder of {rem}\b"):
            TC.transcode_jpeg(f420, transform=op)
    with pytest.raises(ValueError, match="the y axis.*remainder of 4"):
        TC.transcode_jpeg(grey, transform="flip_v")
    # trim that leaves nothing
    small, _, _ = _file(12, 40, S420)
    with pytest.raises(ValueError, match="no whole iMCU"):
        TC.transcode_jpeg(small, transform="flip_h", trim=True)
    # interleaved=True: grey, transposed 4:2:2, sampling outside the three
    for data, kw in ((grey, {}), (f422, dict(transform="transpose")), (f422, dict(transform="rot90", trim=True)), (f440, {})):
        with pytest.raises(ValueError, match="interleaved=True"):
            TC.transcode_jpeg(data, interleaved=True, **kw)
    for bad in (1, 0, None, "yes", 1.0, [True]):
        with pytest.raises(ValueError, match="optimize"):
            TC.transcode_jpeg(f420, optimize=bad)
        with pytest.raises(ValueError, match="interleaved"):
            TC.transcode_jpeg(f420, interleaved=bad)
    for bad in ("rot45", "FLIP_H", 90, "rotate90"):
        with pytest.raises(ValueError, match="transform"):
            TC.transcode_jpeg(f420, transform=bad)
    with pytest.raises(ValueError, match="trim"):
        TC.transcode_jpeg(f420, transform="flip_h", trim=1)
    # a file the reader refuses is refused as decode_jpeg refuses it
    with pytest.raises(jfif.JpegFormatError):
        TC.transcode_jpeg(b"\xff\xd8\xff\xd9")
    monkeypatch.undo()
    # encode_coefficients checks its own arguments before it looks at a plane
    monkeypatch.setattr(TC, "coef_histogram", no_device)
    monkeypatch.setattr(TC, "coef_rows", no_device)
    monkeypatch.setattr(TC, "coef_scan_rows", no_device)
    q = [16] * 64
    for kw in (dict(optimize=1), dict(interleaved="no"), dict(sampling=[(1, 1)], interleaved=True), dict(sampling=[(1, 2), (1, 1), (1, 1)], interleaved=True),
               dict(sampling=[(2, 2), (2, 1), (1, 1)], interleaved=True), dict(sampling=[(4, 1), (1, 1), (1, 1)], interleaved=True), dict(qtables=[[0] * 64] * 3),
               dict(qtables=[[256] * 64] * 3), dict(qtables=[q, q]), dict(width=0), dict(height=65536), dict(sampling=[(5, 1), (1, 1), (1, 1)])):
        args = dict(coefs=[None] * len(kw.get("sampling", S420)), qtables=[q] * len(kw.get("sampling", S420)), width=16, height=16, sampling=S420)
        args.update(kw)
        with pytest.raises(ValueError):
            TC.encode_coefficients(**args)
    # plan_transform: what the docstring's table says
    assert TC.plan_transform(40, 24, S420, "flip_h", True) == ((32, 24), (32, 24), S420)
    assert TC.plan_transform(40, 24, S420, "flip_v", True) == ((40, 16), (40, 16), S420)
    assert TC.plan_transform(40, 24, S420, "rot180", True) == ((32, 16), (32, 16), S420)
    assert TC.plan_transform(40, 24, S420, "transpose", False) == ((40, 24), (24, 40), S420)
    assert TC.plan_transform(48, 16, S422, "rot90", False) == ((48, 16), (16, 48), [(1, 2), (1, 1), (1, 1)])
    assert TC.plan_transform(40, 24, S420, "rot90", True) == ((40, 16), (16, 40), S420)
    assert TC.plan_transform(40, 24, S420, "rot270", True) == ((32, 24), (24, 32), S420)
    assert TC.plan_transform(40, 24, S420, None, False) == ((40, 24), (40, 24), S420)


def _write_cases():
    scan = lambda k, n: bytes((i * k + 7) % 251 for i in range(n))  # noqa: E731
    qa, qb = [1 + (i * 3) % 200 for i in range(64)], [255 - i for i in range(64)]
    grey = ([dict(scan=scan(3, 90), blocks_per_row=3, qtable=qa)], 20, 12)
    c420 = ([dict(scan=scan(5, 200), blocks_per_row=6, qtable=qa), dict(scan=scan(7, 60), blocks_per_row=3, qtable=qb), dict(scan=scan(11, 61), blocks_per_row=3, qtable=qb)], 40, 24)
    return dict(grey=grey, c420=c420), qa, qb


def test_write_jpeg_keeps_its_bytes_and_takes_the_new_keywords():
    pins = json.load(open(os.path.join(ROOT, "tests", "golden", "jpeg_write_pins.json")))
    cases, qa, qb = _write_cases()
    for name, args in cases.items():
        assert hashlib.sha256(jfif.write_jpeg(*args)).hexdigest() == pins[name], name
    # the defaults spelled out, and keywords that ask for what the defaults do, change nothing
    assert jfif.write_jpeg(*cases["c420"], table_per_component=False, colorspace=None) == jfif.write_jpeg(*cases["c420"])
    assert jfif.write_jpeg(*cases["c420"], table_per_component=True, colorspace="YCbCr") == jfif.write_jpeg(*cases["c420"])
    assert jfif.write_jpeg(*cases["grey"], table_per_component=True, colorspace="grey") == jfif.write_jpeg(*cases["grey"])
    # a table per component; equal tables share an id
    comps, W, H = cases["c420"]
    qc = [(i * 7) % 255 + 1 for i in range(64)]
    for tabs, ids in (([qa, qb, qc], [0, 1, 2]), ([qa, qb, qa], [0, 1, 0]), ([qa, qa, qa], [0, 0, 0]), ([qa, qa, qb], [0, 0, 1])):
        info = jfif.read_jpeg(jfif.write_jpeg([dict(c, qtable=t) for c, t in zip(comps, tabs)], W, H, table_per_component=True, sampling=S444))
        assert [c["tq"] for c in info["components"]] == ids and sorted(info["qtables"]) == sorted(set(ids))
        for c, t in zip(info["components"], tabs):
            assert info["qtables"][c["tq"]].tolist() == t
    # without the keyword the third component takes the second's table, as ever
    info = jfif.read_jpeg(jfif.write_jpeg([dict(c, qtable=t) for c, t in zip(comps, [qa, qb, qc])], W, H))
    assert [c["tq"] for c in info["components"]] == [0, 1, 1] and info["qtables"][1].tolist() == qb
    # the colour space survives
    for cs in ("YCbCr", "RGB"):
        data = jfif.write_jpeg(comps, W, H, colorspace=cs)
        assert jfif.read_jpeg(data)["colorspace"] == cs and (b"JFIF\x00" in data) == (cs == "YCbCr") and (b"Adobe" in data) == (cs == "RGB")
    assert jfif.read_jpeg(jfif.write_jpeg(*cases["grey"], colorspace="grey"))["colorspace"] == "grey"
    for args, cs in ((cases["grey"], "RGB"), (cases["grey"], "YCbCr"), (cases["c420"], "grey"), (cases["c420"], "CMYK")):
        with pytest.raises(ValueError):
            jfif.write_jpeg(*args, colorspace=cs)


def test_code_object_holds_the_planned_instantiations():
    from test_kernel_coverage import code_object_kernels
    names, n_objects = code_object_kernels(lib=COEF_LIB)
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


class Layout:
    """one scan form over known planes: 'plane' (one component, an interval per block row) or an interleaved sampling"""

    def __init__(self, planes, sampling=None):
        self.planes = planes
        self.inter = sampling is not None
        self.sampling = sampling or [(1, 1)]
        h, v = self.sampling[0]
        self.frame = dict(width=planes[0].shape[1], height=planes[0].shape[0], comps=self.sampling)
        self.per_row = planes[-1].shape[1] // 8
        self.rows = planes[-1].shape[0] // 8
        self.scan = dict(comps=SCAN3 if self.inter else [(0, 0, 0)], dri=self.per_row)
        self.blocks = self.per_row * (h * v + 2 if self.inter else 1)
        self.hist = T.histogram(self.frame, [self.scan], planes)

    def expected(self, specs):
        """the unstuffed bytes of every interval"""
        data, st = E.encode_scan(self.frame, self.scan, self.planes, especs(specs))
        return [unstuff(data[a:b]) for a, b in st["intervals"]], st

    def histogram(self, torch, pad=0):
        hist, lost = TC.coef_histogram([dev(torch, p, pad) for p in self.planes], self.sampling, interleaved=self.inter)
        return hist.cpu().numpy().astype(np.int64), int(lost.item())

    def code(self, torch, specs, rows=None, pad=0, extra=0, planes=None):
        """-> (segments per interval or None where not coded, seg_bytes, ff_counts, uncoded, unrepresentable); checks the canaries"""
        stride = TC.opt_seg_stride(self.blocks) + extra
        seg = torch.full((self.rows * stride + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        counts = torch.full((2, self.rows + 2), -7, dtype=torch.int32, device="cuda")
        words = torch.zeros((4,), dtype=torch.int32, device="cuda")
        words[1], words[3] = -9, -9
        r0, r1 = rows or (0, self.rows)
        d = planes or [dev(torch, p, pad) for p in self.planes]
        if self.inter:
            TC.coef_scan_rows(d, self.sampling, specs, seg, counts[0], counts[1], words[0:1], words[2:3], seg_stride=stride, my0=r0, my1=r1)
        else:
            TC.coef_rows(d[0], (specs[0], specs[1]), seg, counts[0], counts[1], words[0:1], words[2:3], seg_stride=stride, by0=r0, by1=r1)
        s, c, w = seg.cpu().numpy(), counts.cpu().numpy(), words.cpu().numpy()
        assert w[1] == -9 and w[3] == -9 and np.all(c[:, self.rows:] == -7) and np.all(s[self.rows * stride:] == 0xA5)
        out = []
        for r in range(self.rows):
            if r0 <= r < r1:
                n = int(c[0, r])
                assert 0 < n <= stride and np.all(s[r * stride + -(-n // 4) * 4:(r + 1) * stride] == 0xA5), ("past the segment's last word", r, n)
                out.append(s[r * stride:r * stride + n].tobytes())
            else:
                assert c[0, r] == -7 and c[1, r] == -7 and np.all(s[r * stride:(r + 1) * stride] == 0xA5), ("a row not asked for was written", r)
                out.append(None)
        return out, c[0, :self.rows], c[1, :self.rows], int(w[0]), int(w[2])

    def check(self, torch, specs, **kw):
        want, st = self.expected(specs)
        got, nbytes, ff, uncoded, lost = self.code(torch, specs, **kw)
        for r, g in enumerate(got):
            if g is not None:
                assert g == want[r], ("segment", r, len(g), len(want[r]))
                assert nbytes[r] == len(want[r]) and ff[r] == want[r].count(b"\xff"), ("counts", r)
        assert uncoded == 0 and lost == 0
        return st


def mcu_planes(rng, sampling, mx, my, **kw):
    return [sparse(rng, (my * v * 8, mx * h * 8), **kw) for h, v in sampling]


LAYOUTS = [("plane", None, (255, 256, 257)), ("4:2:0", S420, (31, 32, 33)), ("4:2:2", S422, (31, 32, 33)), ("4:4:4", S444, (63, 64, 65))]


@pytest.mark.gpu
@pytest.mark.parametrize("name,sampling,widths", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_chunk_boundaries_of_every_layout(gpu, name, sampling, widths):
    torch = gpu
    for i, w in enumerate(widths):
        rng = np.random.default_rng(100 + i)
        planes = [sparse(rng, (16, w * 8), density=0.3)] if sampling is None else mcu_planes(rng, sampling, w, 2, density=0.3)
        lay = Layout(planes, sampling)
        lay.check(torch, ANNEX, pad=i)
        hist, lost = lay.histogram(torch, pad=i)
        assert np.array_equal(hist, lay.hist) and lost == 0, (name, w)
        # a sub-range leaves the other row's segment, counts and everything beside them untouched
        lay.check(torch, ANNEX, rows=(1, 2), extra=8)
        lay.check(torch, ANNEX, rows=(0, 1))
    ran = {k for k in api.kernel_counts() if k.startswith("k_coef<")}
    hv = {"plane": "0, 0", "4:2:0": "2, 2", "4:2:2": "2, 1", "4:4:4": "1, 1"}[name]
    assert {f"k_coef<{hv}, true>", f"k_coef<{hv}, false>"} <= ran, ran


def long_code_specs():
    from test_jpeg_encode_optimized import long_code_specs as f
    return f()


@pytest.mark.gpu
def test_ring_window_loop_and_dc_carry(gpu):
    """one interval of 257 blocks, every coefficient non-zero up to +-1023, 16-bit codes: a chunk is far beyond the ring's 32768 bits, and
    the DC alternates between -1024 and 1023 so that every difference, the one across the chunk seam included, is +-2047"""
    rng = np.random.default_rng(5)
    p = rng.integers(1, 1024, (8, 257 * 8)).astype(np.int16) * rng.choice(np.array([-1, 1], dtype=np.int16), (8, 257 * 8))
    p[0, ::8] = np.where(np.arange(257) % 2 == 0, -1024, 1023)
    p[2, 3::8] = 1023
    p[5, 6::8] = -1023
    lay = Layout([p])
    st = lay.check(gpu, long_code_specs())
    assert st["max_block_bits"] > 1500 and st["length"] * 8 > 8 * 32768 and {2047, -2047} <= st["dc_diffs"]
    hist, lost = lay.histogram(gpu)
    assert np.array_equal(hist, lay.hist) and lost == 0
    # the same in MCU order: every component's DC alternates along the scan, so each carry across the seam of 32 MCUs is +-2047 too
    planes = [rng.integers(1, 1024, (8 * v, 33 * 8 * h)).astype(np.int16) * rng.choice(np.array([-1, 1], dtype=np.int16), (8 * v, 33 * 8 * h)) for h, v in S420]
    seen = {}
    for ci, by, bx in E.block_order(dict(width=33 * 16, height=16, comps=S420), dict(comps=SCAN3))[0]:
        planes[ci][by * 8, bx * 8] = 1023 if seen.get(ci, 0) % 2 else -1024
        seen[ci] = seen.get(ci, 0) + 1
    lay = Layout(planes, S420)
    st = lay.check(gpu, long_code_specs())
    assert st["length"] * 8 > 8 * 32768 and st["dc_diffs"] == {-1024, 2047, -2047}
    hist, lost = lay.histogram(gpu)
    assert np.array_equal(hist, lay.hist) and lost == 0


def _zz_block(levels, dc=0):
    """{zig-zag index: level} -> an 8 x 8 block"""
    b = np.zeros(64, dtype=np.int16)
    b[0] = dc
    for k, v in levels.items():
        b[E.ZZ[k]] = v
    return b.reshape(8, 8)


def _loss(lay):
    """the values a baseline scan cannot hold, counted from the planes: AC levels outside +-1023, DC differences outside +-2047"""
    n = 0
    for p in lay.planes:
        ac = np.asarray(p, dtype=np.int64).copy()
        ac[::8, ::8] = 0
        n += int((np.abs(ac) > 1023).sum())
    order, n_mcus, upm = E.block_order(lay.frame, lay.scan)
    dri = lay.scan["dri"]
    for k in range(-(-n_mcus // dri)):
        pred = {}
        for ci, by, bx in order[k * dri * upm:min((k + 1) * dri, n_mcus) * upm]:
            d = int(lay.planes[ci][by * 8, bx * 8])
            n += abs(d - pred.get(ci, 0)) > 2047
            pred[ci] = d
    return n


@pytest.mark.gpu
def test_symbol_edge_cases_first_last_and_at_a_chunk_seam(gpu):
    special = [_zz_block({}), _zz_block({63: 5}), _zz_block({16: -3}), _zz_block({17: 7, 33: 1}), _zz_block({32: 2}), _zz_block({33: -1}), _zz_block({63: -1023}),
               _zz_block({1: 1023, 2: -1023, 63: 1}), _zz_block({}, dc=-1024), _zz_block({5: 1}, dc=1023), _zz_block({}, dc=-1024), _zz_block({1: 1, 17: 1, 34: 1, 50: 1})]
    n = len(special)
    rng = np.random.default_rng(9)
    p = sparse(rng, (16, 300 * 8))
    for row in range(2):
        for at in (0, 256 - n // 2, 300 - n):
            for i, b in enumerate(special):
                p[row * 8:row * 8 + 8, (at + i) * 8:(at + i + 1) * 8] = b
    lay = Layout([p])
    for specs in (ANNEX, long_code_specs()):
        st = lay.check(gpu, specs)
    assert st["zero_blocks"] >= 12 and st["ends_at_63"] >= 18 and st["zrl_chains"][3] >= 12 and {1023, -1023} <= st["ac_values"] and {2047, -2047} <= st["dc_diffs"]
    assert {0xF0, 0xF2, 0x03, 0xF1, 0x01, 0xE3} <= set(st["ac_symbols"])  # runs of 15, 16, 31, 32 and 62
    hist, lost = lay.histogram(gpu)
    assert np.array_equal(hist, lay.hist) and lost == 0
    # the same blocks as the three components of a 4:2:2 scan, seam at 32 MCUs
    planes = [np.ascontiguousarray(p[:8, :66 * 8]), np.ascontiguousarray(p[:8, 240 * 8:273 * 8]), np.ascontiguousarray(p[8:, 267 * 8:])]
    lay = Layout(planes, S422)
    lay.check(gpu, ANNEX)
    hist, lost = lay.histogram(gpu)
    assert np.array_equal(hist, lay.hist) and lost == 0


@pytest.mark.gpu
def test_loss_is_reported(gpu):
    torch = gpu
    rng = np.random.default_rng(3)
    cases = {}
    p = sparse(rng, (16, 260 * 8))
    p[3, 5], p[9, 258 * 8 + 1] = 1024, -1024
    cases["AC 1024 and -1024"] = ([p], None, 2)
    p = sparse(rng, (8, 24), dc=0)
    p[0, 8], p[0, 16] = 2048, 2048
    cases["a DC step of 2048"] = ([p], None, 1)
    p = sparse(rng, (8, 258 * 8), dc=0)
    p[0, 255 * 8], p[0, 256 * 8] = 32767, -32768
    cases["DC 32767 next to -32768 across the seam"] = ([p], None, 3)
    planes = mcu_planes(rng, S420, 34, 2)
    planes[0][8 + 2, 3], planes[1][1, 33 * 8 + 7], planes[2][8, 0] = -32768, 32767, 2048
    cases["4:2:0"] = (planes, S420, None)
    for name, (planes, sampling, want) in cases.items():
        lay = Layout(planes, sampling)
        lost = _loss(lay)
        assert lost > 0 and (want is None or lost == want), (name, lost)
        assert lay.histogram(torch)[1] == lost, name
        _, nbytes, _, uncoded, got = lay.code(torch, long_code_specs())  # the canaries after every segment are checked there
        assert got == lost and uncoded == 0, name
        # the statistics are those of the clamped values: the coder's bytes are encode_scan's of the clamped planes
        if name == "AC 1024 and -1024":
            clamped = Layout([np.clip(planes[0], -1023, 1023).astype(np.int16)])
            assert np.array_equal(lay.histogram(torch)[0], clamped.hist)
            assert lay.code(torch, ANNEX)[0] == clamped.expected(ANNEX)[0]
        # the public layer refuses, with either kind of table
        samp = sampling or [(1, 1)]
        d = [dev(torch, q).contiguous() for q in planes]
        for kw in (dict(optimize=True), dict(optimize=False), dict(optimize=True, interleaved=True), dict(optimize=False, interleaved=True)):
            if kw.get("interleaved") and sampling is None:
                continue
            with pytest.raises(api.MdctError, match="cannot be written"):
                TC.encode_coefficients(d, [[16] * 64] * len(d), planes[0].shape[1], planes[0].shape[0], samp, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name,sampling,widths", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_tables_of_every_kind(gpu, name, sampling, widths):
    rng = np.random.default_rng(40)
    w = widths[2]
    planes = [sparse(rng, (24, w * 8), amp=300, density=0.4)] if sampling is None else mcu_planes(rng, sampling, w, 1, amp=300, density=0.4)
    lay = Layout(planes, sampling)
    optimal = T.specs_of(lay.hist, grey=sampling is None)
    for specs in (optimal, ANNEX, long_code_specs()):
        lay.check(gpu, specs, pad=1)
    # a table that lacks a used symbol: that symbol is counted, every time it occurs
    sym = int(np.argmax(lay.hist[0, 17:])) + 1  # the luminance AC symbol that occurs most, EOB aside
    bits, vals = list(ANNEX[1][0]), list(ANNEX[1][1])
    bits[E.canonical_codes(bits, vals)[sym][1] - 1] -= 1
    vals.remove(sym)
    lacking = dict(ANNEX)
    lacking[1] = (bits, vals)
    occurs = int(lay.hist[0, 16 + sym])
    assert occurs > 0
    _, _, _, uncoded, lost = lay.code(gpu, lacking)
    assert uncoded == occurs and lost == 0


GRIDS = [(1, 1), (1, 9), (9, 1), (8, 8), (17, 23)]


@pytest.mark.gpu
@pytest.mark.parametrize("grid", GRIDS, ids=[f"{a}x{b}" for a, b in GRIDS])
def test_transform_planes_is_the_numpy_statement(gpu, grid):
    torch = gpu
    by, bx = grid
    rng = np.random.default_rng(by * 100 + bx)
    p = rng.integers(-32768, 32768, (by * 8, bx * 8)).astype(np.int16)
    src = dev(torch, p, pad=2)
    for op in X.OPS:
        want = X.transform(p, op)
        big = torch.full((want.shape[0] + 16, want.shape[1] + 16 + 8 * (by & 1)), 0x5A5A, dtype=torch.int16, device="cuda")
        dst = big[8:8 + want.shape[0], 8:8 + want.shape[1]]
        TC.transform_planes(src, dst, op)
        got = big.cpu().numpy()
        assert np.array_equal(got[8:8 + want.shape[0], 8:8 + want.shape[1]], want), op
        got[8:8 + want.shape[0], 8:8 + want.shape[1]] = 0x5A5A
        assert np.all(got == 0x5A5A), (op, "the border around dst")
        assert torch.equal(src, torch.from_numpy(p).cuda()), (op, "src")
    assert api.kernel_counts().get("k_coef_transform", 0) >= 7
    if by == bx:
        for op in X.TRANSPOSING + ("flip_h",):
            with pytest.raises(api.MdctError, match="overlap"):
                TC.transform_planes(src, src, op)
    else:
        with pytest.raises(api.MdctError, match="dst states"):
            TC.transform_planes(src, torch.empty_like(src), "transpose")
        with pytest.raises(api.MdctError, match="dst states"):
            TC.transform_planes(src, torch.empty((bx * 8, by * 8), dtype=torch.int16, device="cuda"), "rot180")
    with pytest.raises(ValueError):
        TC.transform_planes(src, src, "rot45")


# ------------------------------------------------------------------------------------------ GPU: transcode_jpeg end to end
def _adobe_rgb(data):
    """the file with its JFIF APP0 replaced by an Adobe APP14 of transform 0: libjpeg then takes the three components for R, G, B"""
    assert data[2:4] == b"\xff\xe0" and data[4:6] == b"\x00\x10"
    return data[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00" + data[20:]


def _inputs():
    q3 = [np.arange(1, 65), np.arange(64, 0, -1) * 2, np.full(64, 7)]
    q3[0][1], q3[1][8] = 200, 250  # not symmetric: a transposed table differs
    return {
        "grey 8x8": lambda: _file(8, 8, [(1, 1)], seed=1),
        "grey 2056x16 unmarked": lambda: _file(2056, 16, [(1, 1)], seed=2),
        "4:4:4 24x40 interleaved DRI 2": lambda: _file(24, 40, S444, seed=3, dri=2),
        "4:2:0 40x24 three scans unmarked": lambda: _file(40, 24, S420, seed=4, interleaved=False),
        "4:2:0 528x32 interleaved": lambda: _file(528, 32, S420, seed=5, dri=33),
        "4:2:2 48x16": lambda: _file(48, 16, S422, seed=6, dri=3),
        "Adobe RGB, three tables": lambda: (lambda d, f, p: (_adobe_rgb(d), f, p))(*_file(24, 16, S444, seed=7, qtables=q3, table_per_component=True)),
    }


INPUTS = _inputs()
_made = {}


def _input(name):
    if name not in _made:
        _made[name] = INPUTS[name]()
    return _made[name]


def _legal_interleaved(sampling):
    return len(sampling) == 3 and tuple(sampling[0]) in ((1, 1), (2, 1), (2, 2)) and all(tuple(s) == (1, 1) for s in sampling[1:])


@pytest.mark.gpu
@pytest.mark.parametrize("op", (None,) + X.OPS, ids=lambda o: str(o))
@pytest.mark.parametrize("name", list(INPUTS))
def test_transcode_jpeg_end_to_end(gpu, name, op):
    from simd_dct_amd import jpeg_decode as D
    data, frame, planes = _input(name)
    src = jfif.read_jpeg(data, require_restart=False)
    W, H, sampling = frame["width"], frame["height"], frame["comps"]
    hmax, vmax = max(h for h, _ in sampling), max(v for _, v in sampling)
    tw, th = X.trimmed(W, H, sampling, op)
    needs_trim = (tw, th) != (W, H)
    if name.startswith("4:2:0 40x24"):
        assert needs_trim == (op in ("flip_h", "flip_v", "rot180", "transverse", "rot90", "rot270"))
        assert (tw, th) == {"flip_h": (32, 24), "flip_v": (40, 16), "rot180": (32, 16), "transpose": (40, 24)}.get(op, (tw, th))
    if needs_trim:
        with pytest.raises(ValueError, match="remainder"):
            TC.transcode_jpeg(data, transform=op)
    # the expected planes on the output's MCU grid: the source cropped to the trimmed size's MCUs, then the numpy statement
    mx, my = -(-tw // (8 * hmax)), -(-th // (8 * vmax))
    want = [p[:my * v * 8, :mx * h * 8] for p, (h, v) in zip(planes, sampling)]
    want = [np.ascontiguousarray(X.transform(p, op) if op else p) for p in want]
    transposing = op in X.TRANSPOSING
    ow, oh = (th, tw) if transposing else (tw, th)
    osamp = [(v, h) for h, v in sampling] if transposing else list(sampling)
    oframe = dict(width=ow, height=oh, comps=osamp)
    ohmax, ovmax = max(h for h, _ in osamp), max(v for _, v in osamp)
    own = [(-(-(-(-oh * v // ovmax)) // 8) * 8, -(-(-(-ow * h // ohmax)) // 8) * 8) for h, v in osamp]
    qsrc = [src["qtables"][c["tq"]].reshape(8, 8) for c in src["components"]]
    for inter in (False, True):
        if inter and not _legal_interleaved(osamp):
            with pytest.raises(ValueError, match="interleaved=True"):
                TC.transcode_jpeg(data, transform=op, trim=True, interleaved=True)
            continue
        for optimize in (False, True):
            out = TC.transcode_jpeg(data, transform=op, trim=needs_trim, interleaved=inter, optimize=optimize)
            info = jfif.read_jpeg(out)  # every scan has a restart interval
            assert (info["width"], info["height"]) == (ow, oh) and [(c["h"], c["v"]) for c in info["components"]] == osamp
            assert info["colorspace"] == src["colorspace"] and (b"Adobe" in out[:40]) == (src["colorspace"] == "RGB")
            for c, q in zip(info["components"], qsrc):
                assert np.array_equal(info["qtables"][c["tq"]].reshape(8, 8), q.T if transposing else q)
            assert len(info["qtables"]) == len({q.tobytes() for q in qsrc})
            # the scans: form, restart interval, bytes
            scans = [dict(comps=[(c["index"], c["td"], c["ta"]) for c in sc["components"]], dri=sc["restart_interval"]) for sc in info["scans"]]
            if inter:
                assert len(scans) == 1 and scans[0]["comps"] == SCAN3 and scans[0]["dri"] == -(-ow // (8 * ohmax))
            else:
                assert [s["comps"] for s in scans] == [[SCAN3[c]] for c in range(len(osamp))]
                assert [s["dri"] for s in scans] == [o[1] // 8 for o in own]
            specs = {k: (list(b), list(v)) for k, (b, v) in info["huffman"].items()}
            for sc, s in zip(info["scans"], scans):
                assert out[sc["start"]:sc["end"]] == E.encode_scan(oframe, s, want, {k: (list(b), list(v)) for k, (b, v) in sc["huffman"].items()})[0]
            by_which = {2 * th_ + tc: v for (tc, th_), v in specs.items()}
            if optimize:
                assert by_which == T.specs_of(T.histogram(oframe, scans, want), grey=len(osamp) == 1)
            else:
                assert by_which == {k: (list(b), list(v)) for k, (b, v) in ANNEX.items() if k in by_which}
            # the serial decoder reads exactly the transformed planes, on every component's own grid (an interleaved scan: the MCU grid)
            got, statuses, _ = DC.decode(out)
            assert all(s == DC.OK for st in statuses for s in st)
            for g, w, (r, c) in zip(got, want, own):
                assert g.shape == w.shape
                if inter:
                    assert np.array_equal(g, w)
                else:
                    assert np.array_equal(g[:r, :c], w[:r, :c]) and not g[r:].any() and not g[:, c:].any()
            # and so does the GPU decoder, by its fast path
            _, coefs = D.decode_jpeg(out, coefficients=True)
            for g, w, (r, c) in zip(coefs, want, own):
                g = g.cpu().numpy()
                assert np.array_equal(g, w) if inter else np.array_equal(g[:r, :c], w[:r, :c])


@pytest.mark.gpu
def test_decode_coefficients_is_the_front_of_decode_jpeg(gpu, monkeypatch):
    from simd_dct_amd import jpeg_decode as D

    def no_inverse(*a, **k):
        raise AssertionError("an inverse DCT ran")

    for name in ("4:2:0 40x24 three scans unmarked", "4:2:0 528x32 interleaved"):
        data, frame, planes = _input(name)
        with monkeypatch.context() as m:
            m.setattr(api, "u8_i16_batch", no_inverse)
            info, coefs = D.decode_coefficients(data)
        assert info["width"] == frame["width"] and len(coefs) == 3
        for g, p in zip(coefs, planes):
            assert g.dtype == gpu.int16 and np.array_equal(g.cpu().numpy(), p)
        _, again = D.decode_jpeg(data, coefficients=True)
        assert all(gpu.equal(a, b) for a, b in zip(coefs, again))


@pytest.mark.gpu
def test_against_pillow(gpu):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(1)
    y, x = np.mgrid[0:48, 0:64]
    img = np.clip(np.stack([128 + 90 * np.sin(x / 9.0 + c) * np.cos(y / 7.0 - c) for c in range(3)], axis=-1) + rng.normal(0, 10, (48, 64, 3)), 0, 255).astype(np.uint8)
    files = {}
    for opt in (False, True):
        b = io.BytesIO()
        Image.fromarray(img).save(b, "JPEG", quality=75, subsampling=2, optimize=opt)
        files[opt] = b.getvalue()
        info = jfif.read_jpeg(files[opt], require_restart=False)
        assert len(info["scans"]) == 1 and info["scans"][0]["restart_interval"] == 0 and (info["components"][0]["h"], info["components"][0]["v"]) == (2, 2)
    for opt, data in files.items():
        px = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        for kw in (dict(), dict(interleaved=True), dict(optimize=False), dict(optimize=False, interleaved=True)):
            out = TC.transcode_jpeg(data, **kw)
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(out)).convert("RGB")), px), (opt, kw)
    # made for the file, the tables pay for the restart markers and more: no longer than Pillow's file with the default tables
    for kw in (dict(), dict(interleaved=True)):
        out = TC.transcode_jpeg(files[False], optimize=True, **kw)
        assert len(out) <= len(files[False]), (kw, len(out), len(files[False]))


@pytest.mark.gpu
def test_coders_in_a_captured_graph(gpu):
    torch = gpu
    rng = np.random.default_rng(8)
    sets = [mcu_planes(rng, S420, 33, 3, density=0.3) for _ in range(2)]
    lays = [Layout(s, S420) for s in sets]
    d = [dev(torch, p) for p in sets[0]]
    stride = TC.opt_seg_stride(lays[0].blocks)
    hist = torch.full((2, 272), -1, dtype=torch.int32, device="cuda")
    words = torch.zeros((2,), dtype=torch.int32, device="cuda")
    seg = torch.zeros((3 * stride,), dtype=torch.uint8, device="cuda")
    counts = torch.zeros((2, 3), dtype=torch.int32, device="cuda")
    out = torch.zeros((3 * stride * 2,), dtype=torch.uint8, device="cuda")
    off = torch.zeros((4,), dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        TC.coef_histogram(d, S420, interleaved=True, hist=hist, unrepresentable=words[1:2], stream=s)
        TC.coef_scan_rows(d, S420, ANNEX, seg, counts[0], counts[1], words[0:1], words[1:2], seg_stride=stride, stream=s)
        api.jpeg_pack_rows(seg, counts[0], stride, 3, out, off, ff_counts=counts[1], stream=s)
    for which in (1, 0, 0):
        for t, p in zip(d, sets[which]):
            t.copy_(torch.from_numpy(p).cuda())
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        lay = lays[which]
        assert np.array_equal(hist.cpu().numpy().astype(np.int64), lay.hist)
        want = E.encode_scan(lay.frame, lay.scan, lay.planes, E.ANNEX_K)[0]
        assert out[:int(off[-1].item())].cpu().numpy().tobytes() == want and words.cpu().tolist() == [0, 0]


@pytest.mark.gpu
def test_hostile_input_raises_as_decode_jpeg_does(gpu):
    import jpeg_hostile_cases as HC
    from simd_dct_amd import jpeg_decode as D
    for args in (("marked-grey", "ood-in-code", "interval0"), ("unmarked-grey", "ovf-1s-at-63", "lane-straddle")):
        c = HC.make(*args)
        head, tail = HC.header(HC.base_of(c), c.twin_planes)
        with pytest.raises(D.JpegDecodeError) as e1:
            D.decode_jpeg(head + c.scan + tail)
        with pytest.raises(D.JpegDecodeError) as e2:
            TC.transcode_jpeg(head + c.scan + tail)
        assert e2.value.scan == e1.value.scan and [int(x) for x in e2.value.status] == [int(x) for x in e1.value.status]
        # a good file transcoded next in the same process is exact
        got, statuses, _ = DC.decode(TC.transcode_jpeg(head + c.twin + tail))
        assert all(s == DC.OK for st in statuses for s in st)
        for g, p in zip(got, c.twin_planes):
            assert np.array_equal(g, np.asarray(p).astype(np.int16)), c.name
    with pytest.raises(jfif.JpegFormatError):
        TC.transcode_jpeg(b"\xff\xd8\xff\xc2\x00\x0b\x08\x00\x08\x00\x08\x01\x01\x11\x00\xff\xd9")
