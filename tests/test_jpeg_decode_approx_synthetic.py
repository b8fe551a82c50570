"""The successive-approximation half of the progressive decoder (mdct_jpegdec_prog_decode_approx: refine_dc, refine_ac / refine_block
and the al shift of first scans) on scans made from KNOWN planes, where the 17 golden files of test_jpeg_decode_approx.py only hold
libjpeg's standard script on eight small pictures.

Truth: jpeg_progressive_approx_checker.decode_scan (T.81 Annex G, serial, a status per interval) on a host copy of exactly what is
uploaded (check() of test_jpeg_decode_progressive.py).  Good scans are coded from planes by jpeg_progressive_approx_encoder, which is
held byte for byte to libjpeg on the golden files, or written token by token by hand; the plane a refinement scan finds holds the
PRE-STATE in the band, sign(c) * ((min(|c|, 1023) >> ah) << ah) for AC and (c >> ah) << ah for DC, and must hold the POST-STATE (the
same with al) after it.  Both formulas are checked on the CPU, checker o encoder, for every case before a GPU case uses them.
Wrong scans each have a legal twin; of a failed refinement interval only the status is compared (the header leaves its blocks
unspecified), everything else exactly.

CPU: the coverage condition of every case, from the encoder's statistics and the scan's bytes; the formulas; five mutants of the
checker, each failing the cases named with it; one of them passes all 17 golden files, one is caught by nine of them.
GPU: the same cases through the device harness, each naming its kernel from the launch tally; whole files of a four-deep script that
is not libjpeg's through decode_coefficients, decode_jpeg and decode_jpeg_batch."""
import functools
import inspect
import re
import types

import numpy as np
import pytest

import jpeg_decode_checker as DC
import jpeg_optimal_tables as T
import jpeg_progressive_approx_checker as XC
import jpeg_progressive_approx_encoder as AE
import jpeg_progressive_encoder as PE
import jpeg_progressive_status as PS
import jpeg_scan_encoder as E
from simd_dct_amd import api, jfif, jfif_sof2
from test_jpeg_decode_progressive import DC0, DC_SPECS, KERNELS, ZRL, check, eob, level, tokens
from test_jpeg_progressive import LONG_AC, S420, S422, S444, as_written, sparse
from test_jpeg_progressive_approx import full_run_row, row_plane, row_units, synthetic_rows

ONE = [(0, 0, 0, 1, 1)]  # the layout of a scan of one component over its own grid


# ------------------------------------------------------------------------------------------ states and cases
def ac_state(v, a):
    """what the scans down to the point transform `a` leave of the AC coefficients v"""
    v = np.asarray(v, dtype=np.int64)
    return (np.sign(v) * ((np.minimum(np.abs(v), 1023) >> a) << a)).astype(np.int16)


def dc_state(v, a):
    return ((np.asarray(v, dtype=np.int64) >> a) << a).astype(np.int16)


def state(plane, a):
    """a coefficient plane after the scans down to `a`: the AC rule everywhere, the DC rule at every block's (0, 0)"""
    out = ac_state(plane, a)
    out[::8, ::8] = dc_state(plane[::8, ::8], a)
    return out


class Case(types.SimpleNamespace):
    """one scan: its bytes, band, ah / al, the AC specification (None: a DC scan), the planes before (None: a first scan) and after,
    sampling (None: one component over its own grid), mcus mx x my, restart interval ri, stats (the encoder's, where it coded it)"""


def case(name, scan, ss, se, ah, al, spec, planes, mx, my, ri, sampling=None, stats=None, pre=None, post=None):
    return Case(name=name, scan=scan, ss=ss, se=se, ah=ah, al=al, spec=spec, sampling=sampling, mx=mx, my=my, ri=ri, stats=stats,
                pre=(pre if pre is not None else [state(p, ah) for p in planes]) if ah else None,
                post=post if post is not None else [state(p, al) for p in planes])


def layout_of(c):
    return ONE if c.sampling is None else [(ci, hh, vv, h, v) for ci, (h, v) in enumerate(c.sampling) for vv in range(v) for hh in range(h)]


def checker_on(c, scan=None, module=XC):
    """the (possibly mutated) checker on the case's planes as the harness uploads them in the band -> (planes, statuses)"""
    lay = layout_of(c)
    planes = [p.copy() for p in c.pre] if c.ah else [np.zeros_like(p) for p in c.post]
    tabs = None if c.ss == 0 and c.ah else {ci: DC.code_table(*DC_SPECS[min(ci, 1)]) for ci in range(len(planes))} if c.ss == 0 else DC.code_table(*c.spec)
    st = module.decode_scan(c.scan if scan is None else scan, c.ss, c.se, c.ah, c.al, tabs, PS.block_order(c.mx, c.my, lay), c.ri * len(lay), planes)
    return planes, st


def in_band(c, planes):
    ks = [E.ZZ[k] for k in range(c.ss, c.se + 1)]
    return [p.reshape(p.shape[0] // 8, 8, p.shape[1] // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 64)[:, ks] for p in planes]


def holds_on_the_cpu(c, module=XC):
    """checker o encoder: from the pre-state the scan gives the post-state, every status 0"""
    got, st = checker_on(c, module=module)
    return st == [0] * len(st) and all(np.array_equal(g, w) for g, w in zip(in_band(c, got), in_band(c, c.post)))


def spec_of(counts):
    return T.optimal_table(counts) if np.any(counts) else LONG_AC  # a scan of correction bits alone has no symbol to count


def refine_row(name, z, band, al, R=None, buffer=None):
    """an AC refinement scan of one block row z [n, 64] (zig-zag) under the optimal table of its own counts; buffer: the encoder's
    limit of buffered correction bits (libjpeg's 937; T.81 has none, and a decoder must not need one)"""
    z = np.clip(z, -1023, 1023).astype(np.int16)  # the decoder's truth is the clamped plane
    (ss, se), n = band, len(z)
    keep = AE.MAX_BUFFERED
    AE.MAX_BUFFERED = keep if buffer is None else buffer
    try:
        spec = spec_of(AE.ac_refine(row_units(z), R or n, ss, se, al)["counts"])
        r = AE.ac_refine(row_units(z), R or n, ss, se, al, spec)
    finally:
        AE.MAX_BUFFERED = keep
    assert r["uncoded"] == 0
    return case(name, AE.scan_data(r["segs"]), ss, se, al + 1, al, spec, [row_plane(z)], n, 1, R or n, stats=r)


def data_bytes(scan):
    """the scan's data bytes: stuffed zeros and RSTm removed"""
    return re.sub(rb"\xff[\xd0-\xd7]", b"", bytes(scan)).replace(b"\xff\x00", b"\xff")


# ---- 1: the encoder's rows
@functools.lru_cache(None)
def rows_cases():
    out = []
    rows = dict(synthetic_rows())
    rows["the full run"] = full_run_row()
    for name, (z, band, al) in rows.items():
        for R in (None,) + ((1, 7, 256) if len(z) >= 300 else ()):
            out.append(refine_row(f"{name}, R {R}", z, band, al, R))
    return out


def test_rows_conditions():
    cs = {c.name: c for c in rows_cases()}
    assert all(holds_on_the_cpu(c) for c in cs.values())
    assert cs["all correction bits, 300, R None"].stats["bit_flushes"] == 20
    assert cs["the full run, R None"].stats["full_run_flushes"] == 1 and cs["the full run, R None"].stats["counts"][0xE0] == 1
    assert cs["a run open over two chunks, R None"].stats["counts"][0x90] == 1
    assert cs["ZRL with buffered bits, R None"].stats["counts"][0xF0] == 4
    assert {(c.ss, c.se) for c in cs.values()} >= {(1, 1), (63, 63), (6, 63), (1, 63)} and {c.al for c in cs.values()} == {0, 1, 2, 13}
    assert sum(1 for c in cs.values() if c.name.endswith((", R 1", ", R 7", ", R 256"))) == 3 * 5, "the five rows of 300 blocks and more"
    c = cs["the clamp, R None"]
    assert int(np.abs(c.post[0]).max()) == 1023 and c.post[0].min() == -1023, "the clamped plane is the truth"


# ---- 2: every position with history
@functools.lru_cache(None)
def history_cases():
    def row(v, signs=False):
        z = np.zeros((300, 64), dtype=np.int16)
        z[:, 1:] = v
        if signs:
            z[:, 1::2] *= -1
            z[1::2] *= -1
        return z
    # at Al 1 the values 7 and 6 are one scan (pre-state 4, every correction bit set: bytes of 0xFF) with two post-states; 5 has every
    # correction bit clear, and is the one row the 0xFF condition does not apply to
    out = []
    for name, z, ones in (("value 7", row(7), True), ("value 6", row(6), True), ("value 7, alternating signs", row(7, True), True), ("value 5", row(5), False)):
        for R in (None, 7):
            out.append(refine_row(name, z, (1, 63), 1, R))
            out[-1].all_bits_set = ones
    return out


def test_history_conditions():
    for c in history_cases():
        assert holds_on_the_cpu(c), c.name
        assert {s for s in range(256) if c.stats["counts"][s]} <= {n << 4 for n in range(15)}, "no symbol but EOBn"
        assert all(np.count_nonzero(b) == 63 for b in in_band(c, c.pre)[0]), "all 63 positions carry history"
        if c.all_bits_set:
            d = data_bytes(c.scan)
            assert b"\xff\x00" in c.scan and d.count(b"\xff") * 2 > len(d), c.name


# ---- 3: end-of-band runs that carry correction bits
def _busy(k=4, v=2, last=0):
    """a block with a new coefficient at k (and one at 63: the block then ends at se and is part of no end-of-band run)"""
    b = np.zeros(64, dtype=np.int16)
    b[k], b[63] = v, last
    return b


@functools.lru_cache(None)
def run_cases():
    # runs of 1 .. 18 blocks between blocks with a new coefficient; every seventh block of the row has history at three positions
    blocks = []
    for n in range(1, 19):
        blocks += [_busy(3 + n, -2 if n % 2 else 3, last=2)] + [np.zeros(64, dtype=np.int16) for _ in range(n)]
    z = np.array(blocks)
    runs = np.flatnonzero(~z.any(axis=1))
    z[runs[::7], 3], z[runs[::7], 17], z[runs[::7], 40] = 5, -6, 4
    two = np.concatenate([z, z])  # two intervals: the first ends with its run of 18, the second starts with a new coefficient
    short = refine_row("runs of 1 .. 18", two, (1, 63), 1, len(z))
    # runs of 2^j + 3 blocks, j = 5 .. 13, and of 32767, at band (1, 1); every seventh block carries a bit.  4681 bits in one run: far
    # beyond what libjpeg buffers, so the encoder's limit is lifted; T.81 has none
    blocks = []
    for n in [(1 << j) + 3 for j in range(5, 14)] + [32767]:
        r = np.zeros((n + 1, 64), dtype=np.int16)
        r[0, 1] = 2
        r[1::7, 1] = np.resize([5, -7, 6, -4], len(r[1::7]))
        blocks.append(r)
    z = np.concatenate(blocks + [_busy(1, -3)[None]])
    long = refine_row("runs of 35 .. 8195 and 32767", z, (1, 1), 1, buffer=1 << 30)
    return [short, long]


def test_run_conditions():
    short, long = run_cases()
    assert holds_on_the_cpu(short) and holds_on_the_cpu(long)
    hist = short.stats["counts"] + long.stats["counts"]
    assert all(hist[n << 4] > 0 for n in range(15)), "every EOBn"
    assert long.stats["full_run_flushes"] == 1 and long.stats["bit_flushes"] == 0 and long.stats["max_buffered"] == -(-32767 // 7)
    assert short.stats["bit_flushes"] == 0 and short.stats["max_buffered"] >= 3
    n = short.mx // 2
    pre, post = in_band(short, short.pre)[0], in_band(short, short.post)[0]
    assert short.ri == n and len(AE.scan_data([b""] * 2)) == 2 and short.scan.count(b"\xff\xd0") == 1
    assert not ((pre[n - 18:n] == 0) & (post[n - 18:n] != 0)).any() and pre[n - 18:n].any(), "the first interval ends in its run of 18, which carries bits"
    assert ((pre[n] == 0) & (post[n] != 0)).sum() == 2, "the next interval starts with new coefficients"


# ---- 4: ZRL over history, by hand
def new(r, positive):
    """the symbol of a new coefficient behind r positions without history, and its sign bit"""
    return ((r << 4) | 1, 1 if positive else 0, 1)


def cbits(values, al):
    """the correction bits of coefficients that have history"""
    return "".join(str((min(abs(int(v)), 1023) >> al) & 1) for v in values)


def hand_case(name, blocks, items, band, al, per=None, pre=None, post=None):
    """blocks: the true coefficients [n, 64] zig-zag; items: per interval, the tokens written by hand under LONG_AC"""
    z = np.array(blocks, dtype=np.int16)
    scan = PE.scan_data([tokens(it, LONG_AC) for it in items])
    return case(name, scan, band[0], band[1], al + 1, al, LONG_AC, [row_plane(z)], len(z), 1, per or len(z),
                pre=None if pre is None else [row_plane(np.array(pre, dtype=np.int16))], post=None if post is None else [row_plane(np.array(post, dtype=np.int16))])


def _hist(k):
    return (4 + k % 4) * (-1 if k % 3 == 0 else 1)  # 4 .. 7: history at every Al below 2


@functools.lru_cache(None)
def zrl_cases():
    out = []
    zero = np.zeros(64, dtype=np.int16)
    # 16 free positions (k = 1 mod 4) between 47 with history: one ZRL walks to 61 over 45 bits, the EOB takes the bits of 62 and 63
    a = np.array([0 if k == 0 or k % 4 == 1 else _hist(k) for k in range(64)], dtype=np.int16)
    free = [k for k in range(1, 64) if a[k] == 0]
    assert len(free) == 16 and np.count_nonzero(a) == 47 and free[-1] == 61
    out.append(hand_case("16 free among 47", [a, zero], [[ZRL, cbits(a[2:61][a[2:61] != 0], 1), eob(1), cbits(a[62:64], 1), eob(1)]], (1, 63), 1))
    # the sixteenth free position is se: the ZRL ends the block
    out.append(hand_case("ZRL to se, band (1, 16)", [zero, _busy(1, 2)], [[ZRL, new(0, True), eob(1)]], (1, 16), 1))
    b = np.array([_hist(k) if 32 <= k < 48 else 0 for k in range(64)], dtype=np.int16)
    out.append(hand_case("ZRL to se, band (32, 63)", [b, zero, b], [[ZRL, cbits(b[32:48], 1), eob(1), ZRL, cbits(b[32:48], 1)]], (32, 63), 1))
    c = np.array([_hist(k) if 1 <= k < 48 else 0 for k in range(64)], dtype=np.int16)
    out.append(hand_case("ZRL to se, band (1, 63)", [c, c, zero], [[ZRL, cbits(c[1:48], 1), ZRL, cbits(c[1:48], 1), eob(1)]], (1, 63), 1))
    # two ZRLs over 32 free positions and 30 with history, then a new coefficient at 63
    d = np.array([_hist(k) if k and k % 2 == 0 and k < 62 else 0 for k in range(64)], dtype=np.int16)
    d[63] = -2
    f1 = [k for k in range(1, 63) if d[k] == 0]
    assert len(f1) == 32 and np.count_nonzero(d[1:63]) == 30
    m1, m2 = f1[15], f1[31]  # where the two ZRLs end
    out.append(hand_case("two ZRLs, a new coefficient at 63", [d, zero],
                         [[ZRL, cbits(d[1:m1][d[1:m1] != 0], 1), ZRL, cbits(d[m1:m2][d[m1:m2] != 0], 1), new(0, False), eob(1)]], (1, 63), 1))
    return out


def test_zrl_conditions():
    for c in zrl_cases():
        assert holds_on_the_cpu(c), c.name
    assert len(zrl_cases()) == 5


# ---- 5: the bit that is already set
@functools.lru_cache(None)
def set_bit_cases():
    """Not encoder output: the pre-state holds coefficients whose bit al is set already (+-1, +-3 times p1) and clear (+-2, +-6 times
    p1), each met by a set and by a clear correction bit.  A set bit adds +-p1 away from zero only where the bit is clear."""
    out = []
    for al in (0, 1, 5):
        p1 = 1 << al
        kinds = [p1, -p1, 2 * p1, -2 * p1, 3 * p1, -3 * p1, 6 * p1, -6 * p1]
        pre = np.zeros((4, 64), dtype=np.int16)
        bits = np.zeros((4, 64), dtype=np.int64)
        for b in range(4):
            for k in range(1, 17):
                pre[b, k], bits[b, k] = kinds[(k - 1) % 8], ((k - 1) // 8 + b) % 2
        post = pre.copy()
        add = (bits == 1) & (pre != 0) & ((pre.astype(np.int64) & p1) == 0)
        post[add] += (np.sign(pre[add]) * p1).astype(np.int16)
        post[1, 17] = p1  # a new coefficient behind the sixteen: its symbol walks over all of them
        row = lambda b: "".join(str(int(x)) for x in bits[b, 1:17])  # noqa: E731
        items = [[eob(1), row(0), new(0, True), row(1), eob(1), eob(2), row(2), row(3)]]
        out.append(hand_case(f"the bit already set, Al {al}", post, items, (1, 63), al, pre=pre, post=post))
        out[-1].bits = bits
    return out


def test_set_bit_conditions():
    for c in set_bit_cases():
        assert holds_on_the_cpu(c), c.name
        p1 = 1 << c.al
        pre, post = in_band(c, c.pre)[0].astype(np.int64), in_band(c, c.post)[0].astype(np.int64)
        bit = c.bits[:, 1:]
        for sign in (1, -1):
            for is_set in (True, False):
                kind = (np.sign(pre) == sign) & (((pre & p1) != 0) == is_set)
                assert (kind & (bit == 1)).any() and (kind & (bit == 0)).any(), (c.name, sign, is_set)
                if is_set:
                    assert np.array_equal(pre[kind], post[kind]), "a set correction bit on a set bit changes nothing"
        assert (pre == -p1).any() and ((pre == -p1) & (bit == 1)).any()
        assert (post[(pre == 2 * p1) & (bit == 1)] == 3 * p1).all() and (post[(pre == -6 * p1) & (bit == 1)] == -7 * p1).all()


# ---- 6: DC refinement at every byte phase
def dc_levels(rng, bits, al):
    """int16 DC levels whose bit al is `bits`, everything else random, negative values included"""
    bits = np.asarray(bits, dtype=np.int64)
    hi = rng.integers(-(1 << (14 - al)), 1 << (14 - al), len(bits))
    return ((hi << (al + 1)) | (bits << al) | rng.integers(0, 1 << al, len(bits))).astype(np.int16)


def dc_row_case(name, bits, al, rng, rows=1, R=None):
    """rows block rows of len(bits) / rows blocks, one component over its own grid"""
    n = len(bits) // rows
    p = np.zeros((8 * rows, 8 * n), dtype=np.int16)
    p[::8, ::8] = dc_levels(rng, bits, al).reshape(rows, n)
    units = [(0, np.array([v])) for v in p[::8, ::8].reshape(-1)]
    return case(name, AE.scan_data(AE.dc_refine(units, R or n, al)["segs"]), 0, 0, al + 1, al, None, [p], n, rows, R or n)


def bits_of(data):
    return np.unpackbits(np.frombuffer(bytes(data), dtype=np.uint8))


def lanes_sb(c):
    """(sub-sequence bytes, lanes with data) of a one-interval scan in refine_dc"""
    sb = max(8, -(-len(c.scan) // 256))
    return sb, -(-len(c.scan) // sb)


def bytes_with_cuts(n, sb, rng):
    """n data bytes, 0xFF after every one or two others (by turns from one sub-sequence to the next, so that the pairs meet the cuts at
    every phase), and placed besides so that in the stuffed stream cut into sub-sequences of sb bytes a 0xFF is the last byte of a
    sub-sequence (its stuffed zero the first of the next) and the first byte of another wherever the position allows"""
    out, p, plain = bytearray(), 0, 0
    while len(out) < n:
        t, r = divmod(p, sb)
        ff = (r == sb - 1 and t % 4 == 0) or (r == 0 and t % 4 == 2) or plain > t % 2
        ff = ff and not (r == sb - 2 and t % 4 == 0) and not (r == sb - 1 and t % 4 == 1)  # (a pair here would step over the place)
        out.append(0xFF if ff else int(rng.integers(0, 0xFF)))
        plain = 0 if ff else plain + 1
        p += 2 if ff else 1
    return bytes(out)


@functools.lru_cache(None)
def dc_cases():
    rng = np.random.default_rng(66)
    out = {}
    for n in range(1, 81):  # (a) every length: every units % 8, lengths 8 and 16 without a padding bit
        out[f"a {n}"] = dc_row_case(f"{n} blocks", rng.integers(0, 2, n), (0, 3, 13)[n % 3], rng)
    third = bytes(0xFF if j % 3 == 0 else int(rng.integers(0, 0xFF)) for j in range(64))
    out["b"] = dc_row_case("512 blocks, a third 0xFF", bits_of(third), 3, rng)
    out["c"] = dc_row_case("20000 blocks, a third 0xFF", bits_of(bytes_with_cuts(2500, 14, rng)), 13, rng)
    out["d"] = dc_row_case("33000 blocks, no 0xFF", bits_of(bytes(int(x) for x in rng.integers(0, 0xFF, 4125))), 0, rng)
    for si, (name, sampling) in enumerate((("4:2:0", S420), ("4:2:2", S422), ("4:4:4", S444))):  # (e) interleaved
        for mx in (31, 32, 33):
            for R in (mx, 5):
                al = (0, 3, 13)[(si + mx + (R == 5)) % 3]
                frame = dict(width=mx * 8 * sampling[0][0], height=2 * 8 * sampling[0][1], comps=sampling)
                planes = []
                for rows, cols in E.plane_shapes(frame):
                    p = np.zeros((rows, cols), dtype=np.int16)
                    p[::8, ::8] = rng.integers(-32768, 32768, (rows // 8, cols // 8))
                    planes.append(p)
                units, upm, gx = AE.scan_units(frame, [0, 1, 2], planes)
                assert gx == mx
                scan = AE.scan_data(AE.dc_refine(units, R * upm, al)["segs"])
                out[f"e {name} {mx} {R}"] = case(f"{name}, {mx} MCUs, R {R}", scan, 0, 0, al + 1, al, None, planes, mx, 2, R, sampling=sampling)
    return out


def test_dc_conditions():
    cs = dc_cases()
    for c in cs.values():
        assert holds_on_the_cpu(c), c.name
    assert {c.mx % 8 for k, c in cs.items() if k.startswith("a")} == set(range(8)) and {c.al for k, c in cs.items() if k.startswith("a")} == {0, 3, 13}
    assert all(any(p.min() < 0 for p in c.post) for k, c in cs.items() if not k.startswith("a"))
    d = data_bytes(cs["b"].scan)
    assert len(d) == 64 and d.count(b"\xff") == 22
    c = cs["c"]
    sb, lanes = lanes_sb(c)
    d = data_bytes(c.scan)
    assert len(d) == 2500 and d.count(b"\xff") * 3 >= len(d) and sb == 14 and lanes > 200, (sb, lanes)
    cuts = range(sb, len(c.scan), sb)
    assert sum(1 for p in cuts if c.scan[p - 1] == 0xFF and c.scan[p] == 0) >= 10, "a stuffed pair across a lane cut"
    assert sum(1 for p in cuts if c.scan[p] == 0xFF and c.scan[p - 1] != 0xFF) >= 10, "0xFF as a lane's first byte"
    c = cs["d"]
    assert b"\xff" not in c.scan and len(c.scan) == 4125 and lanes_sb(c)[0] == 17
    e = [c for k, c in cs.items() if k.startswith("e")]
    assert len(e) == 18 and {c.al for c in e} == {0, 3, 13}
    assert any((c.ri * len(layout_of(c))) % 8 for c in e), "intervals whose blocks are no whole number of bytes"


# ---- 7: first scans with a point transform
def plane_units(p):
    gy, gx = p.shape[0] // 8, p.shape[1] // 8
    return [(0, b) for b in PE.zz_blocks(p, gx, gy).reshape(-1, 64)]


def dc_tokens(levels):
    """the DC symbols of levels before the point transform (the differences are coded, the predictor starts at 0)"""
    out, pred = [], 0
    for v in levels:
        d, pred = int(v) - pred, int(v)
        s = abs(d).bit_length()
        out.append((s, d if d > 0 else d + (1 << s) - 1, s))
    return out


@functools.lru_cache(None)
def first_cases():
    out = []
    for width in (255, 256, 257):  # the seams of 256 lanes
        rng = np.random.default_rng(width)
        p = sparse(rng, (16, width * 8), amp=1023, density=0.08)
        for al in (1, 9):
            for ss, se in ((1, 63), (6, 63), (63, 63)):
                spec = spec_of(AE.ac_first(plane_units(p), width, ss, se, al)["counts"])
                r = AE.ac_first(plane_units(p), width, ss, se, al, spec)
                assert r["uncoded"] == 0 and r["lost"] == 0
                out.append(case(f"AC {ss}..{se}, Al {al}, width {width}", AE.scan_data(r["segs"]), ss, se, 0, al, spec, [p], width, 2, width, stats=r))
        for al, amp in ((1, 2000), (13, 32767)):  # differences of the shifted levels within +-2047
            q = p.copy()
            q[::8, ::8] = rng.integers(-amp, amp + 1, (2, width))
            r = AE.dc_first(plane_units(q), width, al, {0: DC0})
            assert r["uncoded"] == 0 and r["lost"] == 0
            out.append(case(f"DC, Al {al}, width {width}", AE.scan_data(r["segs"]), 0, 0, 0, al, None, [q], width, 2, width, stats=r))
    # test_levels_and_zero_runs' DC row, as levels BEFORE the shift: +-2047 differences; shifted by 13 the predictor leaves int16
    row = [0, 2047, 0, -2047, 0, 1023, -1024, 1023, 1, -1] * 4
    for al in (1, 13):
        for R in (40, 3):
            scan = PE.scan_data([tokens(dc_tokens(row[i:i + R]), DC0) for i in range(0, 40, R)])
            p = np.zeros((8, 320), dtype=np.int16)
            p[0, ::8] = (np.array(row, dtype=np.int64) << al).astype(np.int16)  # (int16)(pred << al)
            out.append(case(f"DC levels of 2047, Al {al}, R {R}", scan, 0, 0, 0, al, None, [p], 40, 1, R, post=[p]))
    return out


def test_first_scan_conditions():
    cs = first_cases()
    for c in cs:
        assert holds_on_the_cpu(c), c.name
    wrapped = [c for c in cs if c.name.startswith("DC levels") and c.al == 13][0]
    assert wrapped.post[0][0, 8] == np.int64(2047 << 13).astype(np.int16) != 2047 << 13, "the predictor left int16 after the shift"
    assert any(c.post[0][::8, ::8].min() < -8192 for c in cs if c.name.startswith("DC, Al 13")), "negative levels under Al 13"
    for c in cs:
        if c.ss and c.al == 9:
            assert np.count_nonzero(in_band(c, c.post)[0]) > 0, c.name


# ---- 8: whole files of a deep script that is not libjpeg's
def deep_script(nc):
    """(components, ss, se, ah, al): DC from Al 3, refined three times; luma AC 1..63 from Al 3, refined in the bands 1..5 and 6..63
    apart at each of three levels; chroma AC in the bands 1..1, 2..62 and 63..63 from Al 1, then refined"""
    every, bands = list(range(nc)), ((1, 1), (2, 62), (63, 63))
    s = [(every, 0, 0, 0, 3), ([0], 1, 63, 0, 3)] + [([ci], a, b, 0, 1) for ci in range(1, nc) for a, b in bands]
    for ah in (3, 2, 1):
        s += [([0], 1, 5, ah, ah - 1), (every, 0, 0, ah, ah - 1), ([0], 6, 63, ah, ah - 1)]
    return s + [([ci], a, b, 1, 0) for ci in range(1, nc) for a, b in bands]


def deep_file(frame, planes, markers, damage=None):
    """the file of the serial encoder's scans of `planes` under deep_script, with DRI = one MCU row of each scan or without markers;
    damage: {scan index: unstuffed intervals -> unstuffed intervals}"""
    nc, scans = len(frame["comps"]), []
    for k, (comps, ss, se, ah, al) in enumerate(deep_script(nc)):
        units, upm, gx = AE.scan_units(frame, comps, planes)
        per = gx * upm if markers else len(units)
        tables = {}
        if ss == 0 and ah == 0:
            counts = AE.dc_first(units, per, al)["counts"]
            specs = {cls: T.optimal_table(counts[cls][:16]) for cls in range(2) if counts[cls].any()}
            tables = {(0, cls): sp for cls, sp in specs.items()}
        elif ss:
            specs = spec_of(AE.encode_scan(units, per, ss, se, ah, al)["counts"])
            tables = {(1, min(comps[0], 1)): specs}
        else:
            specs = None
        r = AE.encode_scan(units, per, ss, se, ah, al, specs)
        assert r.get("uncoded", 0) == 0 and r.get("lost", 0) == 0
        segs = (damage or {}).get(k, lambda s: s)(r["segs"])
        scans.append(dict(components=[(ci, min(ci, 1), min(ci, 1)) for ci in comps], ss=ss, se=se, ah=ah, al=al, restart_interval=per // upm, tables=tables,
                          scan=AE.scan_data(segs)))
    q = [np.ones(64, dtype=np.int64)] + [np.full(64, 2, dtype=np.int64)] * (nc - 1)  # jpeg_scan_encoder.encode_file's tables
    data = jfif.write_progressive_jpeg(q, frame["width"], frame["height"], frame["comps"], scans)
    if not markers:
        bare = re.sub(rb"\xff\xdd\x00\x04..", b"", data, flags=re.S)
        assert len(bare) == len(data) - 6 * len(scans)
        data = bare
    return data


DEEP = {"grey 40x24": dict(width=40, height=24, comps=[(1, 1)]), "4:2:0 203x117": dict(width=203, height=117, comps=S420)}


@functools.lru_cache(None)
def deep_planes(name):
    frame = DEEP[name]
    rng = np.random.default_rng(len(name))
    planes = as_written(frame, [sparse(rng, s, amp=300, density=0.3, dc=1000) for s in E.plane_shapes(frame)], True)
    for p in planes:
        p.setflags(write=False)
    return planes


@functools.lru_cache(None)
def deep(name, markers):
    return deep_file(DEEP[name], deep_planes(name), markers)


def baseline_twin(name):
    frame = DEEP[name]
    comps = [(ci, min(ci, 1), min(ci, 1)) for ci in range(len(frame["comps"]))]
    return E.encode_file(frame, [dict(comps=comps, dri=4)], deep_planes(name), E.ANNEX_K)[0]


@pytest.mark.parametrize("name", list(DEEP))
def test_deep_files_on_the_cpu(name):
    """the reader takes the script (T.81 G.1.1.1.1 allows a refinement band narrower than the first scan's), and the checker reads
    the planes back from both files"""
    nc = len(DEEP[name]["comps"])
    for markers in (True, False):
        data = deep(name, markers)
        info = jfif_sof2.read_sof2_jpeg(data)
        assert [([c["index"] for c in s["components"]], s["ss"], s["se"], s["ah"], s["al"]) for s in info["scans"]] == deep_script(nc)
        assert all((s["restart_interval"] > 0) == markers for s in info["scans"])
        got, statuses = XC.decode(data)
        assert all(s == [0] * len(s) for s in statuses)
        for g, w in zip(got, deep_planes(name)):
            assert np.array_equal(g, w)
    script = deep_script(nc)
    assert max(al for *_, ah, al in script if ah == 0) == 3 and sum(1 for _, ss, _, ah, _ in script if ss == 0 and ah) == 3
    assert {(ss, se) for _, ss, se, ah, _ in script if ah and ss} >= {(1, 5), (6, 63)} and ([0], 1, 63, 0, 3) in script


# ------------------------------------------------------------------------------------------ wrong refinement scans
def stuffed(seg):
    return bytes(seg).replace(b"\xff", b"\xff\x00")


def joined(intervals):
    """stuffed intervals -> the scan"""
    return b"".join(iv + (bytes([0xFF, 0xD0 + k % 8]) if k + 1 < len(intervals) else b"") for k, iv in enumerate(intervals))


def nbits(items):
    codes = E.canonical_codes(*LONG_AC)
    return sum(len(t) if isinstance(t, str) else codes[t[0]][1] + t[2] for t in items)


def code_of(sym):
    code, n = E.canonical_codes(*LONG_AC)[sym]
    return format(code, f"0{n}b")


# AC: band 1..20 at Al 1, twelve blocks an interval, nine intervals; every block has history at 2, 5 and 9 (true values 5, -6, 7:
# the plane holds 4, -4, 4 and the correction bits are 0, 1, 1), which leaves 17 positions free
BAND, N, NI, HB = (1, 20), 12, 9, "011"
CODED = [new(2, True), HB[0], eob(1), HB[1:]]  # a new coefficient at 4, behind the free 1 and 3 and over the history at 2


def run_of(m):
    return [eob(m)] + [HB] * m


LEGAL = CODED + run_of(6) + CODED * 5


def wrong_ac_plane():
    z = np.zeros((N, 64), dtype=np.int16)
    z[:, 2], z[:, 5], z[:, 9] = 4, -4, 4
    return np.concatenate([row_plane(z)] * NI, axis=0)


def at_places(block, twin=None):
    """the intervals with `block` (tokens of one block) as the first block, as the last one, and where the legal interval's run of six
    is cut after three blocks; with `twin` in those places: legal"""
    def three(b):
        return {"first block": b + run_of(6) + CODED * 5, "last block": CODED + run_of(6) + CODED * 4 + b, "inside the run": CODED + run_of(3) + b + run_of(2) + CODED * 5}
    return three(block), three(twin if twin is not None else CODED)


def aligned(head):
    """whole blocks (a run of m, then 0 .. 3 coded ones) and `head` behind them, which then ends on a byte -> (tokens, whole blocks)"""
    for m in range(1, 9):
        for c in range(4):
            items = run_of(m) + CODED * c + head
            if nbits(items) % 8 == 0 and m + c < N - 3:
                return items, m + c
    raise AssertionError("no prefix aligns the cut")


def cut(items):
    """the interval's bytes up to the end of `items` (a byte boundary by construction)"""
    n = nbits(items)
    assert n % 8 == 0
    return stuffed(tokens(items + ["1" * 64], LONG_AC)[:n // 8])


@functools.lru_cache(None)
def wrong_ac_cases():
    """[(what, {place: the interval's stuffed bytes}, wanted status or None (the checker alone says), {place: the twin's})]"""
    st = lambda d: {k: stuffed(tokens(v, LONG_AC)) for k, v in d.items()}  # noqa: E731
    out = []
    for what, block, twin, want in (("a (run, 2) symbol", [level(0, 2)], None, XC.BAD_CODE),
                                    ("a run that ends past se", [ZRL, HB, new(1, True)], [ZRL, HB, new(0, True)], XC.COEF_OVERFLOW),
                                    ("a ZRL with 15 free positions left", [new(1, True), HB[0], ZRL, HB[1:]], [new(0, True), ZRL, HB], XC.COEF_OVERFLOW),
                                    ("sixteen 1-bits", ["1" * 16], None, XC.BAD_CODE)):
        bad, good = at_places(block, twin)
        out.append((what, st(bad), want, st(good)))
    # EOBn with n == left + 1; the twin has n == left
    bad = {"first block": [eob(N + 1)], "last block": CODED + run_of(6) + CODED * 4 + [eob(2)], "inside the run": CODED + run_of(3) + [eob(N - 4 + 1)]}
    good = {"first block": run_of(N), "last block": CODED + run_of(6) + CODED * 4 + run_of(1), "inside the run": CODED + run_of(3) + run_of(N - 4)}
    out.append(("EOBn with n == left + 1", st(bad), XC.EOBRUN_OVERFLOW, st(good)))
    # data that ends: the cut is on a byte boundary by construction, so that no padding bit stands in for the missing one
    ends = {"inside a code": cut(aligned([code_of(0x21)[:7]])[0]), "in the sign bit": cut(aligned([code_of(0x21)])[0]),
            "in a correction bit of a coded block": cut(aligned([new(2, True)])[0]),
            "in a correction bit of a run's block": cut(aligned(CODED + [eob(3), HB, HB[0]])[0]), "after k whole blocks": cut(aligned(CODED * 2)[0]),
            "an empty interval": b""}
    out.append(("data that ends", ends, XC.OUT_OF_DATA, {k: stuffed(tokens(LEGAL, LONG_AC)) for k in ends}))
    # an EOBn that is the data's last symbol, its extra bits cut off: the smallest run its code can mean fits / does not fit
    fits, k = aligned(CODED + [code_of(0x10)])
    assert 2 <= N - k - 1
    out.append(("an EOBn without its extra bits", {"EOB1 code, 2 or 3 blocks fit": cut(fits), "EOB14 code, 16384 blocks do not fit": cut(aligned(CODED + [code_of(0xE0)])[0])},
                XC.OUT_OF_DATA, {}))
    # markers inside the correction bits of the run
    legal = tokens(LEGAL, LONG_AC)
    q = nbits(CODED + [eob(6)]) // 8 + 1
    assert nbits(CODED + [eob(6)]) < 8 * q < nbits(CODED + run_of(6)) and legal[q - 1] != 0xFF
    out.append(("FF D9 inside correction bits", {"": stuffed(legal[:q]) + b"\xff\xd9" + stuffed(legal[q:])}, XC.UNEXPECTED_MARKER, {}))
    out.append(("a wrong RSTm inside correction bits", {"": stuffed(legal[:q]) + b"\xff\xd5" + stuffed(legal[q:])}, None, {}))
    # behind the last block
    full = next(x for x in (run_of(m) + CODED * c + run_of(N - m - c) for m in range(1, N) for c in range(N - m)) if nbits(x) % 8 == 0)  # twelve blocks that end on a byte
    assert nbits(LEGAL) % 8 != 0
    out.append(("a zero padding bit", {"": stuffed(legal[:-1] + bytes([legal[-1] & 0xFE]))}, XC.LEFTOVER, {"no padding bit at all": stuffed(tokens(full, LONG_AC))}))
    out.append(("a whole extra byte", {"behind a full last byte": stuffed(tokens(full, LONG_AC) + b"\x5a"), "behind a padded last byte": stuffed(legal + b"\xff")}, XC.LEFTOVER, {}))
    return out


def nine(interval, i):
    legal = stuffed(tokens(LEGAL, LONG_AC))
    return joined([interval if k == i else legal for k in range(NI)])


def wrong_ac_case(scan):
    return case("wrong", scan, BAND[0], BAND[1], 2, 1, LONG_AC, [wrong_ac_plane()], N, NI, N, pre=[wrong_ac_plane()])


def test_wrong_ac_scans_on_the_cpu():
    """the checker gives every wrong interval the wanted status and every twin 0, in the intervals 0, 4 and 8 of nine"""
    n = 0
    for what, bad, want, good in wrong_ac_cases():
        for i in (0, NI // 2, NI - 1):
            for place, iv in bad.items():
                st = checker_on(wrong_ac_case(nine(iv, i)))[1]
                if want is not None:
                    assert st == [want if k == i else 0 for k in range(NI)], (what, place, i, st)
                else:
                    assert len(st) == NI and st[i] != 0, (what, place, i, st)
                n += 1
            for place, iv in good.items():
                assert checker_on(wrong_ac_case(nine(iv, i)))[1] == [0] * NI, (what, place, i)
    assert n >= 3 * (5 * 3 + 6 + 2 + 2 + 1 + 2)
    # a lone trailing 0xFF: a fill byte in front of an RSTm (legal), a marker at the end of the last interval
    legal = stuffed(tokens(LEGAL, LONG_AC))
    assert checker_on(wrong_ac_case(nine(legal + b"\xff", 4)))[1] == [0] * NI
    assert checker_on(wrong_ac_case(nine(legal + b"\xff", NI - 1)))[1] == [0] * (NI - 1) + [XC.UNEXPECTED_MARKER]


def wrong_dc(units_mod):
    """three intervals of 24 + units_mod blocks at Al 3 -> (case of the legal scan, its unstuffed intervals)"""
    n = 24 + units_mod
    rng = np.random.default_rng(n)
    c = dc_row_case(f"{n} blocks", rng.integers(0, 2, 3 * n), 3, rng, rows=3)
    units = [(0, np.array([v])) for v in c.post[0][::8, ::8].reshape(-1)]
    return c, AE.dc_refine(units, n, 3)["segs"]


@functools.lru_cache(None)
def wrong_dc_cases():
    """[(what, the legal case, the scan, wanted statuses or None)]"""
    out = []
    for mod in (0, 3):
        c, segs = wrong_dc(mod)
        s = [stuffed(x) for x in segs]
        assert joined(s) == c.scan and len(segs[1]) == 3 + (mod > 0)
        mid = lambda b: joined([s[0], b, s[2]])  # noqa: E731
        out += [(f"one byte short, {mod}", c, mid(stuffed(segs[1][:-1])), [0, XC.OUT_OF_DATA, 0]),
                (f"one byte long, {mod}", c, mid(stuffed(segs[1] + b"\xa5")), [0, XC.LEFTOVER, 0]),
                (f"a marker in the middle, {mod}", c, mid(stuffed(segs[1][:1]) + b"\xff\xc4" + stuffed(segs[1][1:])), [0, XC.UNEXPECTED_MARKER, 0]),
                (f"a lone 0xFF as the last byte, {mod}", c, joined(s) + b"\xff", [0, 0, XC.UNEXPECTED_MARKER]),
                (f"a fill byte before RSTm, {mod}", c, mid(s[1] + b"\xff"), [0, 0, 0]),
                (f"an empty interval, {mod}", c, mid(b""), [0, XC.OUT_OF_DATA, 0]),
                (f"a missing interval, {mod}", c, joined([s[0], s[2]]), None)]
        if mod:
            out.append((f"zero padding bits, {mod}", c, mid(stuffed(segs[1][:-1] + bytes([segs[1][-1] & 0xE0]))), [0, XC.LEFTOVER, 0]))
            out.append((f"one zero padding bit, {mod}", c, mid(stuffed(segs[1][:-1] + bytes([segs[1][-1] & 0xFE]))), [0, XC.LEFTOVER, 0]))
    # a marker exactly at a lane cut of the 20 000-block interval, and one that straddles a cut (the scan keeps its length)
    c = dc_cases()["c"]
    sb, lanes = lanes_sb(c)
    t = next(t for t in range(lanes // 2, lanes) if 0xFF not in c.scan[t * sb - 2:t * sb])
    for what, p in (("at a lane cut", t * sb), ("across a lane cut", t * sb - 1)):
        scan = c.scan[:p] + b"\xff\xc4" + c.scan[p + 2:]
        assert lanes_sb(case("", scan, 0, 0, 14, 13, None, c.post, c.mx, 1, c.ri)) == (sb, lanes)
        out.append((f"a marker {what} of 20000 blocks", c, scan, [XC.UNEXPECTED_MARKER]))
    return out


def test_wrong_dc_scans_on_the_cpu():
    for what, c, scan, want in wrong_dc_cases():
        st = checker_on(c, scan=scan)[1]
        assert (st == want) if want is not None else (len(st) == 3 and st[0] == 0 and any(st[1:])), (what, st)
    assert len(wrong_dc_cases()) == 2 * 7 + 2 + 2


# ------------------------------------------------------------------------------------------ the cases must be able to fail
def mutant(change):
    """a private copy of the checker (its source run again as a module of its own) with `change` applied: a function that replaces
    one of the copy's functions, or, where the mutation sits inside a loop, [(piece of the source, its replacement)]; a piece that is
    not there exactly once fails loudly"""
    src = inspect.getsource(XC)
    for old, new_ in () if callable(change) else change:
        assert src.count(old) == 1, old
        src = src.replace(old, new_)
    m = types.ModuleType("mutant_checker")
    exec(compile(src, "mutant_checker", "exec"), m.__dict__)
    if callable(change):
        change(m)
    return m


def _correct_as(step):
    """_correct of the copy replaced: a set correction bit changes c to step(c, p1)"""
    def change(m):
        def _correct(rd, planes, unit, k, p1):
            p, y, x = m._at(planes, unit, k)
            if rd.bit():
                p[y, x] = m._i16(step(int(p[y, x]), p1))
        m._correct = _correct
    return change


# name: (the mutation, the cases it must fail)
MUTANTS = {
    "the correction added without the (c & p1) == 0 test": (_correct_as(lambda c, p1: c + (p1 if c >= 0 else -p1)), lambda: set_bit_cases()),
    "the correction added towards zero for negatives": (_correct_as(lambda c, p1: c + p1 if (c & p1) == 0 else c),
                                                        lambda: set_bit_cases() + [c for c in history_cases() if "alternating" in c.name]),
    "a ZRL that counts history positions as part of its sixteen": (
        [("                        _correct(rd, planes, unit, k, p1)\n                    elif r == 0:",
          "                        _correct(rd, planes, unit, k, p1)\n                        r -= 1 if rs == 0xF0 and r > 0 else 0\n                    elif r == 0:")],
        lambda: [c for c in zrl_cases() if c.name != "ZRL to se, band (1, 16)"]),  # (that block has no history to count)
    "the blocks of an EOB run not consuming their correction bits": (
        [("                if p[y, x] != 0:\n                    _correct(rd, planes, unit, k, p1)\n                k += 1\n            eobrun -= 1",
          "                k += 1\n            eobrun -= 1")],
        lambda: run_cases() + [c for c in history_cases() if c.ri == 7]),
    "pred << al replaced by a shift of the difference": (
        [("pred[unit[0]] = pred.get(unit[0], 0) + DC.extend(rd.receive(s), s)", "d = DC.extend(rd.receive(s), s)\n                pred[unit[0]] = pred.get(unit[0], 0) + d"),
         ("_i16(pred[unit[0]] << al)", "_i16(pred[unit[0]] - d + (d << al))")],
        lambda: [c for c in first_cases() if c.ss == 0]),
}
ZRL_MUTANT = "a ZRL that counts history positions as part of its sixteen"


def test_the_unchanged_copy_is_the_checker():
    """the copy the mutants are made from decodes as the checker does, so a mutant's failure is its mutation's"""
    m = mutant([])
    assert all(holds_on_the_cpu(c, module=m) for c in set_bit_cases() + zrl_cases() + run_cases()[:1] + first_cases()[-4:])


@pytest.mark.parametrize("name", list(MUTANTS))
def test_a_mutant_of_the_checker_fails_its_named_cases(name):
    change, named = MUTANTS[name]
    m, cases = mutant(change), named()
    assert len(cases) >= 2
    for c in cases:
        assert holds_on_the_cpu(c), c.name
        assert not holds_on_the_cpu(c, module=m), c.name


def golden_files_that_catch(m):
    from test_jpeg_decode_approx import FIXTURES, fixture, truth
    assert len(FIXTURES) == 17
    caught = []
    for f in FIXTURES:
        want, statuses = truth(f)
        try:
            got, st = m.decode(fixture(f))
        except Exception:  # a mutant may lose its place in the data altogether
            got, st = [], None
        if st != statuses or not all(np.array_equal(g, w) for g, w in zip(got, want)):
            caught.append(f)
    return caught


def test_the_golden_files_cannot_catch_the_missing_bit_test():
    """no conforming encoder sends a set correction bit for a coefficient whose bit is set already"""
    assert golden_files_that_catch(mutant(MUTANTS["the correction added without the (c & p1) == 0 test"][0])) == []


def test_the_golden_files_and_the_zrl_mutant():
    """Recorded as found: libjpeg's files DO hold ZRLs that walk over history positions, so a ZRL that counts them loses its place
    there, and these 9 of the 17 golden files catch it.  What none of them shows
    is the ZRL at the edges the cases above build (sixteen free positions among 47 with history, a sixteenth free position that is
    se), which the mutant fails in test_a_mutant_of_the_checker_fails_its_named_cases."""
    caught = golden_files_that_catch(mutant(MUTANTS[ZRL_MUTANT][0]))
    assert caught == ["c420_17x9.prog", "c420_17x9.prog_nomark", "c422_50x35.prog", "c422_50x35.prog_nomark", "c444_50x35.prog", "c444_50x35.prog_b3",
                      "c444_50x35.prog_nomark", "noisy_203x117_q90.prog", "noisy_203x117_q90.prog_nomark"]


# ------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    torch.cuda.set_device(0)
    api.init(0)
    return torch


def tallied(torch, call):
    """-> (what call() returns or the JpegDecodeError it raises, the launch tally of the call)"""
    from simd_dct_amd import jpeg_decode as D
    torch.cuda.synchronize()
    api.kernel_counts_reset()
    try:
        out = call()
    except D.JpegDecodeError as e:
        out = e
    torch.cuda.synchronize()
    return out, api.kernel_counts()


def scans_of(script):
    """the tally a script's scans must leave: one launch of its kernel per scan"""
    return {"k_decode_prog_dc": sum(1 for _, ss, *_ in script if ss == 0), "k_decode_prog_ac": sum(1 for _, ss, *_ in script if ss)}


def on_gpu(torch, c, scan=None, good=True):
    """the case through check(), its kernel named from the launch tally: once, and the other one not at all -> statuses"""
    specs = DC_SPECS if c.ss == 0 else [None, None, c.spec, None]
    torch.cuda.synchronize()
    api.kernel_counts_reset()
    _, st = check(torch, c.scan if scan is None else scan, c.ss, c.se, specs, c.post if good else None, c.sampling, c.mx, c.my, c.ri, good=good, ah=c.ah, al=c.al,
                  pre=c.pre)
    ran = api.kernel_counts()
    kernel = "k_decode_prog_dc" if c.ss == 0 else "k_decode_prog_ac"
    assert ran.get(kernel) == 1 and not (KERNELS - {kernel}) & set(ran), ran
    return st


ROW_NAMES = sorted({c.name.rsplit(", R ", 1)[0] for c in rows_cases()})


@pytest.mark.gpu
@pytest.mark.parametrize("name", ROW_NAMES)
def test_the_encoders_rows_decoded(gpu, name):
    cs = [c for c in rows_cases() if c.name.rsplit(", R ", 1)[0] == name]
    assert len(cs) in (1, 4)
    for c in cs:
        on_gpu(gpu, c)


@pytest.mark.gpu
def test_every_position_with_history(gpu):
    for c in history_cases():
        on_gpu(gpu, c)


@pytest.mark.gpu
@pytest.mark.parametrize("k", (0, 1), ids=("runs of 1 .. 18", "runs up to 32767"))
def test_end_of_band_runs_that_carry_bits(gpu, k):
    on_gpu(gpu, run_cases()[k])


@pytest.mark.gpu
def test_zrl_over_history(gpu):
    for c in zrl_cases():
        assert on_gpu(gpu, c) == [0]


@pytest.mark.gpu
def test_the_bit_that_is_already_set(gpu):
    for c in set_bit_cases():
        on_gpu(gpu, c)


@pytest.mark.gpu
@pytest.mark.parametrize("group", "abcde")
def test_dc_refinement_at_every_byte_phase(gpu, group):
    cs = [c for k, c in dc_cases().items() if k.startswith(group)]
    assert len(cs) == {"a": 80, "e": 18}.get(group, 1)
    for c in cs:
        on_gpu(gpu, c)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ("width 255", "width 256", "width 257", "DC levels of 2047"))
def test_first_scans_with_a_point_transform(gpu, which):
    cs = [c for c in first_cases() if which in c.name]
    assert len(cs) == (4 if which.startswith("DC") else 8)
    for c in cs:
        on_gpu(gpu, c)


@pytest.mark.gpu
def test_deep_scripts_whole_files(gpu):
    from simd_dct_amd import jpeg_decode as D
    from test_jpeg_progressive import own_shapes
    files = {(name, markers): deep(name, markers) for name in DEEP for markers in (True, False)}
    for (name, markers), data in files.items():
        frame, want = DEEP[name], deep_planes(name)
        twin = baseline_twin(name)
        want_tally = scans_of(deep_script(len(frame["comps"])))
        (_, got), ran = tallied(gpu, lambda: D.decode_coefficients(data))
        assert {k: ran.get(k) for k in KERNELS} == want_tally, ran
        (px, cf), ran = tallied(gpu, lambda: D.decode_jpeg(data, coefficients=True))
        assert {k: ran.get(k) for k in KERNELS} == want_tally, ran
        for coefs in (got, cf):
            assert len(coefs) == len(want)
            for g, w, (r, c) in zip(coefs, want, own_shapes(frame)):
                assert np.array_equal(g.cpu().numpy()[:r, :c], w[:r, :c]), (name, markers)
        for g, w in zip(px, D.decode_jpeg(twin)):
            assert gpu.equal(g, w), (name, markers)
        assert gpu.equal(D.decode_jpeg(data, mode="RGB"), D.decode_jpeg(twin, mode="RGB"))
    for markers in (True, False):
        pair = [files[(name, markers)] for name in DEEP]
        batch, ran = tallied(gpu, lambda: D.decode_jpeg_batch(pair, coefficients=True))
        assert {k: ran.get(k) for k in KERNELS} == {k: sum(scans_of(deep_script(len(DEEP[name]["comps"])))[k] for name in DEEP) for k in KERNELS}, ran
        for (px, cf), name in zip(batch, DEEP):
            for g, w, (r, c) in zip(cf, deep_planes(name), own_shapes(DEEP[name])):
                assert np.array_equal(g.cpu().numpy()[:r, :c], w[:r, :c]), (name, markers)
            for g, w in zip(px, D.decode_jpeg(baseline_twin(name))):
                assert gpu.equal(g, w)


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(wrong_ac_cases())), ids=[w[0] for w in wrong_ac_cases()])
def test_wrong_ac_refinement_scans(gpu, k):
    what, bad, want, good = wrong_ac_cases()[k]
    legal = wrong_ac_case(nine(stuffed(tokens(LEGAL, LONG_AC)), 0))
    for i in (0, NI // 2, NI - 1):
        for place, iv in bad.items():
            st = on_gpu(gpu, legal, scan=nine(iv, i), good=False)
            assert st[i] != 0 and (want is None or st == [want if j == i else 0 for j in range(NI)]), (what, place, i, st)
        for place, iv in good.items():
            assert on_gpu(gpu, legal, scan=nine(iv, i), good=False) == [0] * NI, (what, place, i)


@pytest.mark.gpu
def test_a_lone_trailing_ff_of_an_ac_refinement(gpu):
    legal = stuffed(tokens(LEGAL, LONG_AC))
    c = wrong_ac_case(nine(legal, 0))
    assert on_gpu(gpu, c, good=False) == [0] * NI
    assert on_gpu(gpu, c, scan=nine(legal + b"\xff", 4), good=False) == [0] * NI, "a fill byte in front of RSTm"
    assert on_gpu(gpu, c, scan=nine(legal + b"\xff", NI - 1), good=False) == [0] * (NI - 1) + [XC.UNEXPECTED_MARKER]


@pytest.mark.gpu
def test_wrong_dc_refinement_scans(gpu):
    for mod in (0, 3):
        on_gpu(gpu, wrong_dc(mod)[0])  # the legal twin
    for what, c, scan, want in wrong_dc_cases():
        st = on_gpu(gpu, c, scan=scan, good=False)
        assert want is None or st == want, (what, st)


def _shorter(k):
    return lambda segs: segs[:k] + [segs[k][:-1]] + segs[k + 1:]


@pytest.mark.gpu
def test_a_damaged_refinement_scan_of_a_file_raises_with_scan_and_status(gpu):
    from simd_dct_amd import jpeg_decode as D
    script = deep_script(1)
    for markers in (True, False):
        for kind in (([0], 1, 5, 2, 1), ([0], 0, 0, 2, 1), ([0], 6, 63, 1, 0)):
            k = script.index(kind)
            bad = deep_file(DEEP["grey 40x24"], deep_planes("grey 40x24"), markers, damage={k: _shorter(1 if markers else 0)})
            _, statuses = XC.decode(bad)
            assert len(statuses) == k + 1 and any(statuses[k]) and not any(any(s) for s in statuses[:k]), (kind, statuses)
            e, ran = tallied(gpu, lambda: D.decode_coefficients(bad))
            assert isinstance(e, D.JpegDecodeError) and e.scan == k and [int(x) for x in e.status] == statuses[k], (kind, e, statuses[k])
            assert {n: ran.get(n, 0) for n in KERNELS} == scans_of(script[:k + 1]), "every scan up to the damaged one ran its kernel once, none behind it"
            with pytest.raises(D.JpegDecodeError):
                D.decode_jpeg(bad, mode="RGB")
