"""Both GPU JPEG decoders (restart-marked: libmdct_jpegdec.so; unmarked: libmdct_jpegdec_unmarked.so) against scans made by the
test-side encoder (tests/jpeg_scan_encoder.py) from known coefficient planes.  The truth is the planes the encoder was given.

CPU: the encoder reproduces Pillow's (libjpeg's) scans byte for byte from the checker's coefficients; the checker
(tests/jpeg_decode_checker.py) decodes every synthetic case to exactly the encoder's planes; fill bytes before RSTm / EOI (T.81 B.1.1.2).
GPU: every case through decode_jpeg(coefficients=True), without restart markers and with at least one DRI, coefficients and pixels;
flat full-size pictures (periodic scans) on both paths; a periodic synthetic scan with few and with enough sync rounds.

Every case asserts its own coverage from the encoder's statistics (code lengths, categories, symbols, blocks per MCU, the byte offsets of
stuffed pairs, padding bits), so a case that stops covering what it names fails instead of passing."""
import numpy as np
import pytest

import jpeg_decode_checker as C
import jpeg_scan_encoder as E
import oracle as O
from simd_dct_amd import jfif

Image = pytest.importorskip("PIL.Image")
from test_jpeg_decode import _picture, pillow_jpeg  # noqa: E402
from test_jpeg_decode_unmarked import checker_scan  # noqa: E402

K = E.ANNEX_K
CHUNK, LANE = 8192, 32  # the unmarked decoder's chunk and lane in stuffed bytes (csrc/jpeg_decode_unmarked.hip)


# ------------------------------------------------------------------------------------------ content
def dc_targets():
    """DC differences of every category 0..11 at both ends of each: +-(2^s - 1), +-2^(s-1)"""
    t = [0]
    for s in range(1, 12):
        for m in sorted({(1 << s) - 1, 1 << (s - 1)}):
            t += [m, -m]
    return t


def dc_values(n, rng, zeros=0):
    """n DC values within +-2047 whose differences hit every dc_targets() entry (through 0 before each, so no difference exceeds
    category 11), then random ones; zeros > 0 makes that fraction of the differences 0"""
    seq = []
    for d in dc_targets():
        a = -(d // 2)
        seq += [0, a, a + d]
    while len(seq) < n:
        seq.append(seq[-1] if rng.random() < zeros else int(np.clip(seq[-1] + rng.integers(-300, 301), -2047, 2047)))
    return seq[:n]


def level(rng, s):
    """an AC level of size s: often one of the extend() boundaries +-(2^s - 1), +-2^(s-1)"""
    m = [(1 << s) - 1, 1 << (s - 1), int(rng.integers(1 << (s - 1), 1 << s))][int(rng.integers(0, 3))]
    return m if rng.random() < 0.5 else -m


def symbol_block(rng, alphabet, weights=None):
    """zig-zag levels 1..63 drawn as a sequence of RS symbols from alphabet (EOB 0x00 ends the block, ZRL 0xF0 skips 16)"""
    z = np.zeros(64, dtype=np.int64)
    k = 1
    p = None if weights is None else np.asarray(weights, dtype=float) / np.sum(weights)
    for _ in range(200):
        rs = int(alphabet[rng.choice(len(alphabet), p=p)])
        r, s = rs >> 4, rs & 15
        if rs == 0x00:
            break
        if rs == 0xF0:
            if k + 16 <= 63:
                k += 16
            continue
        if k + r > 63:
            break
        z[k + r] = level(rng, s)
        k += r + 1
        if k == 64:
            break
    return z


def special_blocks():
    """zig-zag level vectors at the places kernels go wrong: every AC size at both extend() ends, a level at 63 with no EOB, a run of
    15, one to three ZRLs before a level (three ZRLs + run 14 and a level at 15 + two ZRLs + run 15 both land on 63), dense size-10"""
    out = []
    ext = [m * sg for s in range(1, 11) for m in ((1 << s) - 1, 1 << (s - 1)) for sg in (1, -1)]
    z = np.zeros(64, dtype=np.int64)
    z[1:41] = ext
    out.append(z)
    for pos in ([63], [1, 17], [18], [34], [50], [63, 1], [15, 63], [1, 2, 3, 63]):
        z = np.zeros(64, dtype=np.int64)
        z[pos] = 5
        out.append(z)
    z = np.zeros(64, dtype=np.int64)
    z[1:] = [(-1) ** i * (512 + 8 * i) for i in range(63)]
    out.append(z)
    return out


def fill_planes(frame, scans, dc, ac):
    """planes whose blocks, in the decoding order of the scan that covers each component, get DC values dc(component, n) and AC
    vectors ac(component, n, index)"""
    planes = [np.zeros(s, dtype=np.int16) for s in E.plane_shapes(frame)]
    for sc in scans:
        order, _, _ = E.block_order(frame, sc)
        per = {}
        for ci, by, bx in order:
            per.setdefault(ci, []).append((by, bx))
        for ci, blocks in per.items():
            d = dc(ci, len(blocks))
            for i, (by, bx) in enumerate(blocks):
                z = ac(ci, i)
                z[0] = d[i]
                nat = np.zeros(64, dtype=np.int64)
                nat[E.ZZ] = z
                planes[ci][by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = nat.reshape(8, 8)
    return planes


ALL_AC = [0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)]


def mixture(seed, alphabet=ALL_AC, weights=None, specials=True, zeros=0.0):
    """content: the special blocks first, then zero blocks and random symbol blocks"""
    rng = np.random.default_rng(seed)
    sp = special_blocks() if specials else []

    def ac(ci, i):
        if i < len(sp):
            return sp[i].copy()
        if rng.random() < 0.1:
            return np.zeros(64, dtype=np.int64)
        return symbol_block(rng, alphabet, weights)

    return (lambda ci, n: dc_values(n, rng, zeros)), ac


# ------------------------------------------------------------------------------------------ tables
def deep_tables():
    """luma: every length 1..16, the most frequent AC symbol (0x01) and DC category (0) on 16 bits; 16 AC symbols (the all-ones code of
    16 bits stays free), 12 DC categories"""
    ac = [0x02, 0x00, 0x03, 0x11, 0x04, 0x21, 0x05, 0x31, 0xF0, 0x06, 0x41, 0x07, 0x12, 0x08, 0xF1, 0x01]
    dc = {s: s for s in range(1, 12)}
    dc[0] = 16
    return E.spec_from_lengths(dc), E.spec_from_lengths({s: i + 1 for i, s in enumerate(ac)}), ac


def fastslow_tables():
    """the most frequent AC symbols on 9 and 10 bits, just past the fast lookup's 9 (kFastBits)"""
    ac = [0x01, 0x02, 0x11, 0x03, 0x00, 0x21, 0x04, 0x12, 0x31, 0x05, 0xF0, 0x41, 0x22, 0x06, 0x13, 0x51]
    lengths = {s: (9 if i < 4 else 10 if i < 8 else 4 + (i - 8) // 2) for i, s in enumerate(ac)}
    dc = {s: (9 if s < 2 else 10 if s < 4 else 5) for s in range(12)}
    return E.spec_from_lengths(dc), E.spec_from_lengths(lengths), ac


def stuffing_tables():
    """the most frequent AC symbol 0x08 gets the code 11111110 and is used with level 255 (eight 1-bits); DC category 0 is 12 bits of
    which 11 are ones"""
    ac = [0x00, 0x01, 0x02, 0x03, 0x11, 0x21, 0x04, 0x08]
    dc = {s: s for s in range(1, 12)}
    dc[0] = 12
    return E.spec_from_lengths(dc), E.spec_from_lengths({s: i + 1 for i, s in enumerate(ac)}), ac


# ------------------------------------------------------------------------------------------ the case matrix
GEOMETRIES = {  # name: (width, height, [(h, v)])
    "grey": (61, 37, [(1, 1)]), "444": (61, 37, [(1, 1)] * 3), "422": (61, 37, [(2, 1), (1, 1), (1, 1)]),
    "420": (61, 37, [(2, 2), (1, 1), (1, 1)]), "440": (61, 37, [(1, 2), (1, 1), (1, 1)]),
    "8blk": (61, 37, [(2, 2), (2, 1), (1, 2)]), "10blk": (150, 70, [(2, 2), (2, 2), (2, 1)]),
    "chroma-above": (61, 37, [(1, 1), (2, 2), (2, 2)]),
    "1x1-grey": (1, 1, [(1, 1)]), "1x1-420": (1, 1, [(2, 2), (1, 1), (1, 1)]), "8x8-420": (8, 8, [(2, 2), (1, 1), (1, 1)]),
    "mcu-row-420": (203, 16, [(2, 2), (1, 1), (1, 1)]), "mcu-column-420": (16, 203, [(2, 2), (1, 1), (1, 1)]),
}


def interleaved(nc, luma=(0, 0), chroma=(1, 1)):
    return [dict(comps=[(0, *luma)] + [(ci, *chroma) for ci in range(1, nc)])]


def _annexk_case(geo, scans=None, seed=1, dris=None):
    W, H, comps = GEOMETRIES[geo]
    frame = dict(width=W, height=H, comps=comps)
    scans = scans or interleaved(len(comps))
    dc, ac = mixture(seed)
    planes = fill_planes(frame, scans, dc, ac)
    return dict(frame=frame, scans=scans, planes=planes, specs=dict(K), dris=dris or [3])


def _case(name):
    """-> dict(frame, scans (without dri), planes, specs, dris (> 0, run besides the unmarked form), cover(stats list))"""
    if name in GEOMETRIES:
        c = _annexk_case(name)
        if name == "10blk":
            mx = -(-150 // 16)
            c["dris"] = [1, 2, 7, mx, mx + 1, 65535]  # 10 x 5 MCUs: DRI 2 gives 25 intervals (1 mod 8)

        def cover(stats, upm=sum(h * v for h, v in GEOMETRIES[name][2])):
            assert stats[0]["blocks"] % upm == 0 and stats[0]["blocks"] >= upm
        c["cover"] = cover
        return c
    if name == "categories-grey":  # every DC category and AC size at both ends, index 63 without EOB, runs of 15, ZRL chains
        frame = dict(width=128, height=72, comps=[(1, 1)])
        scans = interleaved(1)
        dc, ac = mixture(2)
        c = dict(frame=frame, scans=scans, planes=fill_planes(frame, scans, dc, ac), specs=dict(K), dris=[7])

        def cover(stats):
            s = stats[0]
            assert s["dc_categories"] == set(range(12))
            assert {2047, -2047, 1024, -1024, 1, -1} <= s["dc_diffs"]
            assert {m * sg for t in range(1, 11) for m in ((1 << t) - 1, 1 << (t - 1)) for sg in (1, -1)} <= s["ac_values"]
            assert s["ends_at_63"] > 0 and {1, 2, 3} <= set(s["zrl_chains"]) and any(rs >> 4 == 15 and rs & 15 for rs in s["ac_symbols"])
            assert s["zero_blocks"] > 0 and s["max_block_bits"] > 63 * 10
        c["cover"] = cover
        return c
    if name == "full-444-luma-slot1":  # all 12 DC categories and all 162 AC symbols of Annex K; luma on slots 1/3, chroma on 0/2
        frame = dict(width=160, height=96, comps=[(1, 1)] * 3)
        scans = interleaved(3, luma=(1, 1), chroma=(0, 0))
        dc, ac = mixture(3)
        specs = {(0, 1): K[(0, 0)], (1, 1): K[(1, 0)], (0, 0): K[(0, 1)], (1, 0): K[(1, 1)]}
        c = dict(frame=frame, scans=scans, planes=fill_planes(frame, scans, dc, ac), specs=specs, dris=[11])

        def cover(stats):
            assert set(stats[0]["ac_symbols"]) == set(ALL_AC) and stats[0]["dc_categories"] == set(range(12))
        c["cover"] = cover
        return c
    if name == "deep-420-luma-slot1":
        dcs, acs, alpha = deep_tables()
        frame = dict(width=99, height=70, comps=[(2, 2), (1, 1), (1, 1)])
        scans = interleaved(3, luma=(1, 1), chroma=(0, 0))
        w = [1] * 15 + [40]  # 0x01, on 16 bits, most frequent
        dc, ac = mixture(4, alphabet=alpha, weights=w, specials=False, zeros=0.9)
        specs = {(0, 1): dcs, (1, 1): acs, (0, 0): K[(0, 1)], (1, 0): K[(1, 1)]}
        c = dict(frame=frame, scans=scans, planes=fill_planes(frame, scans, dc, ac), specs=specs, dris=[5])

        def cover(stats):
            lac, ldc = stats[0]["lengths"][(1, 1)], stats[0]["lengths"][(0, 1)]
            assert set(lac) == set(range(1, 17)), sorted(lac)
            assert max(lac, key=lac.get) == 16 and max(ldc, key=ldc.get) == 16
        c["cover"] = cover
        return c
    if name == "fastslow-422":
        dcs, acs, alpha = fastslow_tables()
        frame = dict(width=120, height=64, comps=[(2, 1), (1, 1), (1, 1)])
        scans = interleaved(3)
        dc, ac = mixture(5, alphabet=alpha, weights=[30] * 8 + [1] * 8, specials=False, zeros=0.5)
        specs = {(0, 0): dcs, (1, 0): acs, (0, 1): dcs, (1, 1): acs}
        c = dict(frame=frame, scans=scans, planes=fill_planes(frame, scans, dc, ac), specs=specs, dris=[4])

        def cover(stats):
            lac = stats[0]["lengths"][(1, 0)]
            assert lac[9] > 0 and lac[10] > 0 and lac[9] + lac[10] > sum(lac.values()) / 2, lac
            assert {9, 10} <= set(stats[0]["lengths"][(0, 0)])
        c["cover"] = cover
        return c
    if name in ("stuffing-440", "stuffing-grey-dri1"):
        dcs, acs, alpha = stuffing_tables()
        W, H, comps = (88, 64, [(1, 2), (1, 1), (1, 1)]) if name == "stuffing-440" else (64, 40, [(1, 1)])
        frame = dict(width=W, height=H, comps=comps)
        scans = interleaved(len(comps))
        rng = np.random.default_rng(6)

        def ac(ci, i):
            z = symbol_block(rng, alpha, [1, 1, 1, 1, 1, 1, 1, 40])
            z[np.abs(z) >= 128] = 255
            return z
        planes = fill_planes(frame, scans, lambda ci, n: dc_values(n, rng, 0.8), ac)
        specs = {(0, 0): dcs, (1, 0): acs, (0, 1): dcs, (1, 1): acs}
        c = dict(frame=frame, scans=scans, planes=planes, specs=specs, dris=[1] if "dri1" in name else [2, 9])

        def cover(stats):
            s = stats[0]
            assert len(s["stuffed"]) * 8 >= s["length"], (len(s["stuffed"]), s["length"])
        c["cover"] = cover
        return c
    if name == "minimal-grey":  # a DC table with one code, an AC table with EOB and one symbol
        dcs, acs = E.spec_from_lengths({0: 1}), E.spec_from_lengths({0x00: 1, 0x01: 2})
        frame = dict(width=72, height=40, comps=[(1, 1)])
        scans = interleaved(1)
        rng = np.random.default_rng(7)

        def ac(ci, i):
            z = np.zeros(64, dtype=np.int64)
            n = [0, 63, 1, 62][i] if i < 4 else int(rng.integers(0, 64))
            z[1:1 + n] = rng.choice([-1, 1], n)
            return z
        c = dict(frame=frame, scans=scans, planes=fill_planes(frame, scans, lambda ci, n: [0] * n, ac),
                 specs={(0, 0): dcs, (1, 0): acs}, dris=[2])

        def cover(stats):
            s = stats[0]
            assert set(s["lengths"][(0, 0)]) == {1} and set(s["lengths"][(1, 0)]) == {1, 2}
            assert s["ends_at_63"] > 0 and s["zero_blocks"] > 0
        c["cover"] = cover
        return c
    if name in ("noninterleaved-420-odd", "noninterleaved-422-odd", "y-then-cbcr-420"):
        W, H = 37, 45
        comps = [(2, 1), (1, 1), (1, 1)] if "422" in name else [(2, 2), (1, 1), (1, 1)]
        scans = ([dict(comps=[(0, 0, 0)]), dict(comps=[(1, 1, 1), (2, 1, 1)])] if name.startswith("y-then")
                 else [dict(comps=[(ci, min(ci, 1), min(ci, 1))]) for ci in range(3)])
        frame = dict(width=W, height=H, comps=comps)
        dc, ac = mixture(8)
        c = dict(frame=frame, scans=scans, planes=fill_planes(frame, scans, dc, ac), specs=dict(K), dris=[2])

        def cover(stats):  # A.2.2: a non-interleaved scan covers the component's own block grid, not the padded one
            own = [-(-(-(-W * h // 2)) // 8) * -(-(-(-H * v // (2 if "420" in name else 1))) // 8) for h, v in comps]
            assert stats[0]["blocks"] == own[0]
            if not name.startswith("y-then"):
                assert [s["blocks"] for s in stats] == own and own[0] < np.prod(E.plane_shapes(frame)[0]) // 64
        c["cover"] = cover
        return c
    raise KeyError(name)


CASES = list(GEOMETRIES) + ["categories-grey", "full-444-luma-slot1", "deep-420-luma-slot1", "fastslow-422", "stuffing-440",
                            "stuffing-grey-dri1", "minimal-grey", "noninterleaved-420-odd", "noninterleaved-422-odd", "y-then-cbcr-420"]


def encode(c, dri, **fills):
    scans = [dict(sc, dri=dri, **fills) for sc in c["scans"]]
    return E.encode_file(c["frame"], scans, c["planes"], c["specs"])


def _checker_planes(data):
    """the checker's planes and whether every scan / interval decoded OK"""
    _, _, scans = C.parse(data)
    if scans[0][1]:
        planes, st, _ = C.decode(data)
        return planes, all(s == C.OK for x in st for s in x)
    planes, ok = None, True
    for si in range(len(scans)):
        st, _, p, _, _ = checker_scan(data, si)
        ok &= st == C.OK
        planes = p if planes is None else [a + b for a, b in zip(planes, p)]
    return planes, ok


# ------------------------------------------------------------------------------------------ CPU: the encoder anchored on Pillow
ANCHORS = [((61, 37), False, dict(quality=q)) for q in (5, 75, 100)] + [
    ((100, 52), True, dict(quality=75, subsampling=0)), ((100, 52), True, dict(quality=5, subsampling=1)),
    ((100, 52), True, dict(quality=100, subsampling=2)), ((99, 70), True, dict(quality=75, subsampling=2, optimize=True)),
    ((61, 37), False, dict(quality=90, optimize=True))]
ANCHORS += [(s, c, dict(kw, restart_marker_rows=1)) for s, c, kw in ANCHORS[:6]] + [
    ((100, 52), True, dict(quality=75, subsampling=2, restart_marker_blocks=5)), ((61, 37), False, dict(quality=75, restart_marker_blocks=5))]


@pytest.mark.parametrize("size,colour,kw", ANCHORS, ids=[f"{s[0]}x{s[1]}-{'c' if c else 'g'}-{k}" for s, c, k in ANCHORS])
def test_encoder_reproduces_pillows_scan_byte_for_byte(size, colour, kw):
    data = pillow_jpeg(_picture(*size, 12, colour), **kw)
    info = jfif.read_jpeg(data, require_restart=False)
    sc = info["scans"][0]
    planes, ok = _checker_planes(data)
    assert ok
    frame = dict(width=info["width"], height=info["height"], comps=[(c["h"], c["v"]) for c in info["components"]])
    scan = dict(comps=[(c["index"], c["td"], c["ta"]) for c in sc["components"]], dri=sc["restart_interval"])
    specs = {k: (list(b), list(v)) for k, (b, v) in sc["huffman"].items()}
    body, st = E.encode_scan(frame, scan, planes, specs)
    assert body == data[sc["start"]:sc["end"]]
    assert (st["markers"] != []) == ("restart_marker_rows" in kw or "restart_marker_blocks" in kw)


def test_encoder_tables_and_spec_helper():
    from simd_dct_amd import api
    for w, key in enumerate([(0, 0), (1, 0), (0, 1), (1, 1)]):
        assert tuple(map(list, api.huffman_spec(w))) == K[key]
    with pytest.raises(ValueError, match="Kraft"):
        E.spec_from_lengths({0: 1, 1: 1})  # uses the all-ones code "1"
    with pytest.raises(ValueError, match="Kraft"):
        E.spec_from_lengths({s: 8 for s in range(256)})  # the code space filled exactly
    bits, vals = E.spec_from_lengths({5: 3, 7: 1, 9: 3})
    assert bits[:3] == [1, 0, 2] and vals == [7, 5, 9]
    assert E.canonical_codes(bits, vals) == {7: (0, 1), 5: (4, 3), 9: (5, 3)}


def _specs4(c, sc):
    specs = [None] * 4
    for ci, td, ta in sc["comps"]:
        specs[td], specs[2 + ta] = c["specs"][(0, td)], c["specs"][(1, ta)]
    return specs


# ------------------------------------------------------------------------------------------ CPU: the checker on every synthetic case
@pytest.mark.parametrize("name", CASES)
def test_checker_decodes_synthetic_case_to_the_truth(name):
    from simd_dct_amd import jpeg_decode as D
    c = _case(name)
    for sc in c["scans"]:
        assert D.tables_check(_specs4(c, sc)) == 0
    for dri in [0] + c["dris"]:
        data, stats = encode(c, dri)
        c["cover"](stats)
        planes, ok = _checker_planes(data)
        assert ok, dri
        for p, t in zip(planes, c["planes"]):
            assert np.array_equal(p, t), dri


# ------------------------------------------------------------------------------------------ boundary placement
def ones_content(T, pad, block_bits=150):
    """a grey scan (Annex K) of exactly T stuffed bytes whose last block leaves `pad` padding bits: every block DC 0 (2 bits) and n
    levels of +-1 (3 bits each) then EOB (4 bits); no byte of it is 0xFF.  The last block's DC (0 / 1 / 4: +0 / +2 / +4 bits) settles
    the remainder mod 3."""
    bits = 8 * T - pad
    B = max(1, -(-bits // block_bits))
    extra = {0: 0, 2: 2, 1: 4}[(bits - 6 * B) % 3]
    n = (bits - 6 * B - extra) // 3
    assert 0 <= n <= 62 * B
    rng = np.random.default_rng(T)
    frame = dict(width=8 * B, height=8, comps=[(1, 1)])
    plane = np.zeros((8, 8 * B), dtype=np.int16)
    per = np.full(B, n // B)
    per[:n % B] += 1
    for b in range(B):
        z = np.zeros(64, dtype=np.int64)
        z[1:1 + per[b]] = rng.choice([-1, 1], per[b])
        z[0] = {0: 0, 2: 1, 4: 4}[extra] if b == B - 1 else 0
        nat = np.zeros(64, dtype=np.int64)
        nat[E.ZZ] = z
        plane[:, 8 * b:8 * b + 8] = nat.reshape(8, 8)
    return dict(frame=frame, scans=interleaved(1), planes=[plane], specs=dict(K), dris=[max(1, B // 3)])


LENGTHS = [(CHUNK * n + d, 0 if d == 0 else 7) for n in (1, 2, 3) for d in (-1, 0, 1)] + [(32, 0), (31, 7), (20, 3)]


def ff_at(target, B):
    """a grey scan of B blocks (the ones_content kind) with one block of DC 2047 whose stuffed 0xFF lands exactly at byte `target`:
    the levels before it are varied, three bits at a time, until the encoder's statistics show the pair there"""
    frame = dict(width=8 * B, height=8, comps=[(1, 1)])
    j = min(B - 2, (8 * target) // 150 + 1)
    base = max(0, (8 * target - 6 * j - 24) // 3)
    for n in range(max(0, base - 16), base + 24):
        if n > 62 * j:
            break
        plane = np.zeros((8, 8 * B), dtype=np.int16)
        per = np.full(j, n // j) if j else np.zeros(0, int)
        per[:n % j] += 1
        zs = []
        for b in range(B):
            z = np.zeros(64, dtype=np.int64)
            if b < j:
                z[1:1 + per[b]] = 1
            if b == j:
                z[0] = 2047
            zs.append(z)
        for b, z in enumerate(zs):
            nat = np.zeros(64, dtype=np.int64)
            nat[E.ZZ] = z
            plane[:, 8 * b:8 * b + 8] = nat.reshape(8, 8)
        c = dict(frame=frame, scans=interleaved(1), planes=[plane], specs=dict(K), dris=[])
        _, (st,) = encode(c, 0)
        if target in st["stuffed"]:
            return c
    raise AssertionError(f"no placement puts a stuffed 0xFF at {target}")


PLACEMENTS = {"chunk-end": (CHUNK - 1, 1500), "second-chunk-end": (2 * CHUNK - 1, 2800), "lane-end": (7 * LANE - 1, 60),
              "marked-lane-end": (5 * 8 - 1, 40)}


def _boundary_case(name):
    if name.startswith("len"):
        T, pad = map(int, name[3:].split("-pad"))
        c = ones_content(T, pad)

        def cover(stats, T=T, pad=pad):
            assert stats[0]["length"] == T and stats[0]["pad_bits"][-1] == pad and not stats[0]["stuffed"]
        c["cover"] = cover
        return c
    target, B = PLACEMENTS[name]
    c = ff_at(target, B)
    if name == "marked-lane-end":
        c["dris"] = [B]  # one interval of < 2048 bytes: 8-byte lanes, most idle

    def cover(stats, target=target):
        if stats[0]["markers"]:
            s, e = stats[0]["intervals"][0]
            assert e - s < 8 * 256 and target in stats[0]["stuffed"]
        else:
            assert target in stats[0]["stuffed"]
    c["cover"] = cover
    return c


BOUNDARY = [f"len{T}-pad{p}" for T, p in LENGTHS] + list(PLACEMENTS)


@pytest.mark.parametrize("name", BOUNDARY)
def test_checker_decodes_boundary_case_to_the_truth(name):
    c = _boundary_case(name)
    for dri in [0] + c["dris"]:
        data, stats = encode(c, dri)
        if dri == 0 or name == "marked-lane-end":
            c["cover"](stats)
        planes, ok = _checker_planes(data)
        assert ok and np.array_equal(planes[0], c["planes"][0]), dri


def test_short_marked_intervals_are_there():
    """DRI 1 on the ones content: every interval is one block, about 5 bytes"""
    c = ones_content(600, 3, block_bits=40)
    _, (st,) = encode(c, 1)
    lens = [e - s for s, e in st["intervals"]]
    assert max(lens) < 2048 and min(lens) < 8 and len(lens) == c["frame"]["width"] // 8


# ------------------------------------------------------------------------------------------ fill bytes (T.81 B.1.1.2)
def _fill_case():
    """stuffing-heavy content with DRI 1: many intervals end with a stuffed pair, so fill bytes sit right after a data 0xFF 0x00"""
    c = _case("stuffing-grey-dri1")
    _, (st,) = encode(c, 1)
    ends_stuffed = [k for k, (s, e) in enumerate(st["intervals"][:-1]) if e - 2 in st["stuffed"]]
    plain = [k for k, (s, e) in enumerate(st["intervals"][:-1]) if e - 2 not in st["stuffed"]]
    assert len(ends_stuffed) >= 3 and len(plain) >= 3
    fill = {ends_stuffed[0]: 1, ends_stuffed[1]: 2, ends_stuffed[2]: 7, plain[0]: 1, plain[1]: 2, plain[2]: 7, 0: 3}
    return c, fill


def test_checker_reads_fill_bytes_before_rst_and_eoi():
    c, fill = _fill_case()
    for dri, kw in ((1, dict(fill=fill)), (1, dict(fill=fill, fill_end=2)), (0, dict(fill_end=1)), (0, dict(fill_end=7))):
        data, st = encode(c, dri, **kw)
        planes, ok = _checker_planes(data)
        assert ok and np.array_equal(planes[0], c["planes"][0]), (dri, kw)
        info = jfif.read_jpeg(data, require_restart=False)
        assert info["scans"][0]["end"] - info["scans"][0]["start"] == st[0]["length"]  # fill before EOI is no data


def _pillow_with_fill(n):
    data = pillow_jpeg(_picture(64, 48, 13), quality=75, restart_marker_rows=1)
    out = bytearray(data)
    sc = jfif.read_jpeg(data)["scans"][0]
    at = [p for p in range(sc["start"], sc["end"] - 1) if data[p] == 0xFF and 0xD0 <= data[p + 1] <= 0xD7]
    for p, k in sorted(zip(at[:3], (n, 1, n)), reverse=True):
        out[p:p] = b"\xff" * k
    return data, bytes(out)


@pytest.mark.parametrize("n", [1, 2, 7])
def test_pillow_file_with_fill_bytes_before_rst(n):
    """libjpeg decodes the file to the same pixels; the checker gives OK and the original's coefficients"""
    import io
    data, filled = _pillow_with_fill(n)
    a = np.asarray(Image.open(io.BytesIO(data)))
    b = np.asarray(Image.open(io.BytesIO(filled)))
    assert np.array_equal(a, b)
    p0, ok0 = _checker_planes(data)
    p1, ok1 = _checker_planes(filled)
    assert ok0 and ok1 and all(np.array_equal(x, y) for x, y in zip(p0, p1))


# ------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    torch.cuda.set_device(0)
    from simd_dct_amd import api
    api.init(0)
    return torch


def _gpu_matches(data, truth, qtables=None):
    """decode_jpeg(coefficients=True) == the truth planes, and its pixels == the oracle's inverse of them"""
    from simd_dct_amd import jpeg_decode as D
    got, coefs = D.decode_jpeg(data, coefficients=True)
    info = jfif.read_jpeg(data, require_restart=False)
    geo, _ = D.geometry(info)
    for ci, (c, g, t, (w, h, _, _)) in enumerate(zip(coefs, got, truth, geo)):
        c = c.cpu().numpy()
        assert np.array_equal(c, t), (ci, int((c != t).sum()))
        q = info["qtables"][info["components"][ci]["tq"]].astype(np.float32)
        want = O.u8_i16("inv", t, t.shape[1], t.shape[0], lut=q)
        assert np.array_equal(g.cpu().numpy(), want[:h, :w]), ci


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_gpu_decodes_synthetic_case(gpu, name):
    c = _case(name)
    for dri in [0] + c["dris"]:
        data, stats = encode(c, dri)
        c["cover"](stats)
        _gpu_matches(data, c["planes"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", BOUNDARY)
def test_gpu_decodes_boundary_case(gpu, name):
    c = _boundary_case(name)
    for dri in [0] + c["dris"]:
        data, stats = encode(c, dri)
        if dri == 0 or name == "marked-lane-end":
            c["cover"](stats)
        _gpu_matches(data, c["planes"])


@pytest.mark.gpu
def test_gpu_short_marked_intervals(gpu):
    c = ones_content(600, 3, block_bits=40)
    _gpu_matches(encode(c, 1)[0], c["planes"])


@pytest.mark.gpu
def test_gpu_fill_bytes_before_rst_and_eoi(gpu):
    c, fill = _fill_case()
    for dri, kw in ((1, dict(fill=fill)), (1, dict(fill=fill, fill_end=2)), (0, dict(fill_end=1)), (0, dict(fill_end=7))):
        _gpu_matches(encode(c, dri, **kw)[0], c["planes"])
    for n in (1, 2, 7):
        data, filled = _pillow_with_fill(n)
        _gpu_matches(filled, _checker_planes(data)[0])


@pytest.mark.gpu
def test_gpu_fill_bytes_with_producer_offsets(gpu):
    """the marked decoder trims fill bytes from any offsets it is given, not only the index's"""
    torch = gpu
    from test_jpeg_decode import _low_level
    c, fill = _fill_case()
    data, st = encode(c, 1, fill=fill)
    sc = jfif.read_jpeg(data)["scans"][0]
    offs = torch.tensor([0] + [m + 2 for m in st[0]["markers"]] + [st[0]["length"]], dtype=torch.int64, device="cuda")
    planes, status, intact = _low_level(torch, data, offsets=offs)
    assert intact and (status == 0).all()
    assert np.array_equal(planes[0].cpu().numpy(), c["planes"][0])
    assert sc["end"] - sc["start"] == st[0]["length"]


def _flat_checks(torch, name, data, marked_data):
    """every block equals the first, the first equals the checker's, marked == unmarked.  Prints (pytest -s) the unmarked path's
    first-call status at the default 4 sync rounds and decode_jpeg's time for both files: measured, not asserted."""
    import time
    from simd_dct_amd import jpeg_decode as D
    from test_jpeg_decode_unmarked import _low_level
    _, first_st, _, _ = _low_level(torch, data, sync_rounds=4)
    ms = []
    for d in (data, marked_data):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = D.decode_jpeg(d, coefficients=True)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
        if d is data:
            a = out[1]
    _, b = D.decode_jpeg(marked_data, coefficients=True)
    first, st, _ = C.decode(marked_data, intervals={0: [0]})
    assert st[0][0] == C.OK
    for x, y, f in zip(a, b, first):
        assert torch.equal(x, y)
        blk = x[:8, :8]
        assert torch.equal(x, blk.repeat(x.shape[0] // 8, x.shape[1] // 8))
        assert np.array_equal(blk.cpu().numpy(), f[:8, :8])
    sc = jfif.read_jpeg(data, require_restart=False)["scans"][0]
    print(f"\n{name}: unmarked scan {sc['end'] - sc['start']} bytes, first call at sync_rounds=4: {first_st}; decode_jpeg {ms[0]:.1f} ms unmarked, {ms[1]:.1f} ms marked (host parsing included)")


@pytest.mark.gpu
@pytest.mark.parametrize("value", [0, 128])
def test_gpu_flat_8192_grey(gpu, value):
    img = np.full((8192, 8192), value, dtype=np.uint8)
    _flat_checks(gpu, f"flat 8192^2 grey {value}", pillow_jpeg(img, quality=75), pillow_jpeg(img, quality=75, restart_marker_rows=1))


@pytest.mark.gpu
def test_gpu_flat_7680x4320_420(gpu):
    img = np.full((4320, 7680, 3), (90, 120, 140), dtype=np.uint8)
    _flat_checks(gpu, "flat 7680x4320 4:2:0", pillow_jpeg(img, quality=75, subsampling=2), pillow_jpeg(img, quality=75, subsampling=2, restart_marker_rows=1))


@pytest.mark.gpu
def test_gpu_periodic_scan_sync_rounds(gpu):
    """a periodic scan (every block the same, a period that is no divisor of the lane width) over several chunks: too few rounds may
    say NOT_SYNCHRONISED but never give a wrong OK; one round per chunk converges"""
    torch = gpu
    from test_jpeg_decode_unmarked import NOT_SYNCHRONISED, _low_level
    frame = dict(width=8 * 8000, height=16, comps=[(1, 1)])
    z = np.zeros(64, dtype=np.int64)
    z[[1, 2, 5, 9]] = [3, -1, 1, 2]
    nat = np.zeros(64, dtype=np.int64)
    nat[E.ZZ] = z
    plane = np.tile(nat.reshape(8, 8), (2, 8000)).astype(np.int16)
    c = dict(frame=frame, scans=interleaved(1), planes=[plane], specs=dict(K))
    data, st = encode(c, 0)
    nchunks = -(-st[0]["length"] // CHUNK)
    assert nchunks >= 3
    for rounds in (0, 4, nchunks):
        planes, s, intact, _ = _low_level(torch, data, sync_rounds=rounds)
        assert intact and s[0] in (C.OK, NOT_SYNCHRONISED), (rounds, s)
        if s[0] == C.OK:
            assert np.array_equal(planes[0].cpu().numpy(), plane), rounds
        if rounds == nchunks:
            assert s[0] == C.OK
