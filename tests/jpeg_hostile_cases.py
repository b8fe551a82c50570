"""The hostile scans of tests/test_jpeg_decode_hostile.py: one list, used on the CPU (against the checker) and on the GPU (against both
decoders).  Every case is written by tests/jpeg_scan_encoder.py from known planes -- dense noise, so that blocks are long, the n-th AC
symbol of a block stands at zig-zag index n + 1 and symbols land on every boundary -- with ONE wrong thing at a chosen place (the
encoder's `inject`), and comes with its legal twin on the other side of the boundary, which must decode OK to known planes.

A case names: the path (PATHS), the kind (KINDS: what is wrong, and the class it must get), the place (where: first symbol, a symbol
that straddles a sub-sequence / chunk boundary, the first symbol after one, the last block, a block of an interleaved MCU, a restart
interval).  The place is found by searching the encoder's trace of the intact scan and is asserted again from the statistics of the
hostile one (Case.check_place)."""
import functools

import numpy as np

import jpeg_decode_checker as C
import jpeg_scan_encoder as E

K = E.ANNEX_K
CHUNK, LANE = 8192, 32  # the unmarked decoder's chunk and sub-sequence in stuffed bytes (csrc/jpeg_decode_unmarked.hip)
MARKED_LANE = 8         # the marked decoder's sub-sequence for an interval of up to 2048 bytes (csrc/jpeg_decode.hip: max(8, n / 256))

# name: (width, height, sampling, restart interval, seed).  marked-grey has four intervals of four blocks so that one can be "a middle
# interval"; marked-420 has DRI = MCUs per row.  The unmarked scans are a little over two chunks: chunk 1 is a middle chunk, chunk 2 the last.
PATHS = {
    "marked-grey": (64, 16, [(1, 1)], 4, 1),
    "marked-420": (64, 32, [(2, 2), (1, 1), (1, 1)], 4, 2),
    "unmarked-grey": (256, 88, [(1, 1)], 0, 3),
    "unmarked-420": (256, 64, [(2, 2), (1, 1), (1, 1)], 0, 4),
}
SPARSE = (E.spec_from_lengths({0: 1}), E.spec_from_lengths({0x00: 1, 0x01: 2}))  # one DC code "0"; AC codes "0" (EOB) and "10"


def _noise(shape, rng, amp):
    v = rng.integers(1, amp + 1, size=shape) * rng.choice([-1, 1], size=shape)
    return v.astype(np.int64)


@functools.lru_cache(maxsize=None)
def base(path, sparse=False):
    """-> dict(frame, scan, planes (int64, every AC level nonzero), specs, marked, upm)"""
    W, H, comps, dri, seed = PATHS[path]
    frame = dict(width=W, height=H, comps=comps)
    scan = dict(comps=[(ci, min(ci, 1), min(ci, 1)) for ci in range(len(comps))], dri=dri)
    rng = np.random.default_rng(seed)
    planes = []
    for rows, cols in E.plane_shapes(frame):
        p = _noise((rows, cols), rng, 1 if sparse else 15)
        if sparse:
            p[p < 0] = 1  # the sparse AC table has one symbol, 0x01; its extra bit still takes both values
            p *= rng.choice([-1, 1], size=p.shape)
        dc = np.zeros((rows // 8, cols // 8), dtype=np.int64) if sparse else rng.integers(-200, 201, size=(rows // 8, cols // 8))
        p[::8, ::8] = dc
        planes.append(p)
    specs = {(0, 0): SPARSE[0], (1, 0): SPARSE[1]} if sparse else dict(K)
    order, n_mcus, upm = E.block_order(frame, scan)
    return dict(frame=frame, scan=scan, planes=planes, specs=specs, marked=dri > 0, upm=upm, order=order, n_blocks=len(order),
                per_interval=(dri or n_mcus) * upm, n_intervals=-(-n_mcus // (dri or n_mcus)), sparse=sparse, path=path)


def encode(b, planes=None, inject=None):
    return E.encode_scan(b["frame"], b["scan"], b["planes"] if planes is None else planes, b["specs"], inject=inject)


@functools.lru_cache(maxsize=None)
def trace(path, sparse=False):
    """the intact scan of a path: (bytes, stats with the symbol trace)"""
    return encode(base(path, sparse), inject=dict(trace=True))


@functools.lru_cache(maxsize=None)
def _header(path, sparse):
    b = base(path, sparse)
    data, st = E.encode_file(b["frame"], [b["scan"]], b["planes"], b["specs"])
    return data[:st[0]["start"]]


def header(b, planes=None):
    """the file's bytes before the scan (SOI .. SOS) of this path -- they do not depend on the planes -- and the file's tail"""
    return _header(b["path"], b["sparse"]), b"\xff\xd9"


def units(b, k):
    """the checker's unit list of interval k"""
    lo = k * b["per_interval"]
    return [(ci, ("dc", ci), ("ac", ci), (ci, by, bx)) for ci, by, bx in b["order"][lo:lo + b["per_interval"]]]


def tables(b):
    t = {}
    for ci, td, ta in b["scan"]["comps"]:
        t[("dc", ci)] = C.code_table(*b["specs"][(0, td)])
        t[("ac", ci)] = C.code_table(*b["specs"][(1, ta)])
    return t


def check_scan(b, scan):
    """the checker on a whole scan -> [(status, complete blocks [(place, levels)], failing block or None, n complete)] per interval"""
    n = b["n_intervals"]
    parts = C.split_intervals(scan, n) if b["marked"] else [(scan, None)]
    out = []
    for k, (chunk, mk) in enumerate(parts):
        after = None if k == n - 1 else ((mk is not None and mk == k % 8),)
        out.append(C.decode_interval(chunk, units(b, k), tables(b), after, partial=True))
    return out


def truth_blocks(b, planes, k):
    """[(place, 64 levels natural as int16 wraps them)] of interval k from the planes"""
    lo = k * b["per_interval"]
    return [((ci, by, bx), np.asarray(planes[ci][by * 8:by * 8 + 8, bx * 8:bx * 8 + 8]).astype(np.int16).reshape(64))
            for ci, by, bx in b["order"][lo:lo + b["per_interval"]]]


# ------------------------------------------------------------------------------------------ kinds
ONES16 = "1" * 16
# kind: (class, how).  how: ("put", at filter, hostile items, twin (at shift, items, drop_rest) or None for the intact scan)
#                           ("cut" | "marker", which part of a symbol the byte boundary lies in: "code" / "dcx" / "acx"[, marker bytes])
#                           or a special form handled in make()
KINDS = {
    "ovf-1s-at-63": (C.COEF_OVERFLOW, ("put", 62, [(1, 0x11, 1, 1)], (0, [(1, 0x01, 1, 1)], True))),
    "ovf-run15-from-49": (C.COEF_OVERFLOW, ("put", 48, [(1, 0xF1, 1, 1)], (-1, [(1, 0xF1, 1, 1)], True))),
    "ovf-zrl-at-49": (C.COEF_OVERFLOW, ("put", 48, [(1, 0xF0, 0, 0)], (-1, [(1, 0xF0, 0, 0)], True))),
    "ovf-four-zrl-from-1": (C.COEF_OVERFLOW, ("put", 0, [(1, 0xF0, 0, 0)] * 4, (0, [(1, 0xF0, 0, 0)] * 3 + [(1, 0xE1, 1, 1)], True))),
    "bad-dc-16-ones": (C.BAD_CODE, ("put", "dc", [ONES16], None)),
    "bad-ac-16-ones": (C.BAD_CODE, ("put", "ac", [ONES16], None)),
    "ood-in-code": (C.OUT_OF_DATA, ("cut", "code")),
    "ood-in-dc-extra": (C.OUT_OF_DATA, ("cut", "dcx")),
    "ood-in-ac-extra": (C.OUT_OF_DATA, ("cut", "acx")),
    "marker-eoi-in-code": (C.UNEXPECTED_MARKER, ("marker", "code", b"\xff\xd9")),
    "marker-eoi-in-extra": (C.UNEXPECTED_MARKER, ("marker", "acx", b"\xff\xd9")),
    "marker-01-in-code": (C.UNEXPECTED_MARKER, ("marker", "code", b"\xff\x01")),
    "marker-01-in-extra": (C.UNEXPECTED_MARKER, ("marker", "acx", b"\xff\x01")),
    "marker-rst-in-code": (C.UNEXPECTED_MARKER, ("marker", "code", b"\xff\xd5")),
    "marker-rst-in-extra": (C.UNEXPECTED_MARKER, ("marker", "acx", b"\xff\xd5")),
}
# kinds that sit at one place by their nature (the end of an interval's data, a whole interval, a whole scan): make_special()
SPECIAL = {
    "bad-16-bits-left": C.BAD_CODE, "bad-17-bits-left": C.BAD_CODE, "ood-15-bits-left": C.OUT_OF_DATA,
    "ood-after-block": C.OUT_OF_DATA, "ood-empty": C.OUT_OF_DATA, "ood-missing-interval": C.OUT_OF_DATA,
    "marker-lone-ff-at-end": C.UNEXPECTED_MARKER, "marker-wrong-rst-after": C.UNEXPECTED_MARKER,
    "left-one-0-bit": C.LEFTOVER, "left-7-ones-then-ff": C.LEFTOVER, "left-extra-block": C.LEFTOVER,
    "bad-sparse-table": C.BAD_CODE, "dc-wrap-up": C.OK, "dc-wrap-down": C.OK,
}


class Case:
    """name, path, klass, scan (hostile bytes), interval (the failing one), n_before (complete blocks of that interval before the
    error), others {interval: class} (other intervals that are not OK), twin (bytes or None), twin_planes, stats, place"""

    def __init__(self, **kw):
        self.others = {}
        self.twin = None
        self.__dict__.update(kw)

    def __repr__(self):
        return self.name


def _rel(st, k, bit, marked):
    """offset of the stuffed byte holding that bit: from the interval's start (marked) or the scan's (unmarked)"""
    return E.stuffed_offset(st, k, bit) - (st["intervals"][k][0] if marked else 0)


def _boundary_in(start, n):
    """a bit offset p, a multiple of 8, with start < p < start + n (strictly inside n bits from start), or None"""
    p = (start // 8 + 1) * 8
    return p if p < start + n else None


def _candidates(b, st, kind, k):
    """symbols of interval k of the intact trace that this kind can replace / cut: (block, at, first bit, bits of the symbol, previous
    symbol's first bit, cut point or None)"""
    how = KINDS[kind][1]
    syms = st["symbols"][k]
    ends = {}
    for bi, at, s, cl, el in syms:
        ends[bi] = s + cl + el
    out = []
    for j, (bi, at, s, cl, el) in enumerate(syms):
        prev = syms[j - 1][2] if j else -1
        if how[0] == "put":
            want = how[1]
            if (want == "ac" and at != "dc" and at not in (0, 62)) or (want != "ac" and at == want):
                out.append((bi, at, s, cl + el, prev, None))
        else:
            part = how[1]
            if part == "code":
                p = _boundary_in(s, cl)
            elif part == "dcx":
                p = _boundary_in(s + cl - 1, el + 1) if at == "dc" and el else None
            elif part == "acx":
                p = _boundary_in(s + cl - 1, el + 1) if at != "dc" and el else None
            else:
                raise KeyError(part)
            if p is not None:
                out.append((bi, at, s, cl + el, prev, p))
    return out


def _place_filter(b, st, place, k):
    """-> predicate(block, first bit, last bit, previous symbol's first bit, cut point) on offsets of the intact scan"""
    marked = b["marked"]
    rel = lambda bit: _rel(st, k, bit, marked)  # noqa: E731
    lo = k * b["per_interval"]
    hi = lo + min(b["per_interval"], b["n_blocks"] - lo) - 1
    nchunks = -(-st["length"] // CHUNK)

    def straddle(unit, index=None):
        def f(bi, s, e, prev, p):
            a, z = rel(s) // unit, rel(e) // unit
            ok = z == a + 1 and (index is None or z == index)
            return ok and (p is None or rel(p) % unit == 0 and rel(p) // unit == z and rel(p - 1) // unit == a)
        return f

    def after(unit, index=None):
        def f(bi, s, e, prev, p):
            a = rel(s) // unit
            return prev >= 0 and rel(prev) // unit == a - 1 and (index is None or a == index) and (p is None or rel(p) // unit == a)
        return f

    lane = MARKED_LANE if marked else LANE
    if place == "first":
        return lambda bi, s, e, prev, p: bi == lo
    if place == "last-block":
        return lambda bi, s, e, prev, p: bi == hi
    if place == "lane-straddle":
        return straddle(lane)
    if place == "lane-after":
        return after(lane)
    if place in ("chunk1-straddle", "lastchunk-straddle"):
        return straddle(CHUNK, 1 if place.startswith("chunk1") else nchunks - 1)
    if place in ("chunk1-after", "lastchunk-after"):
        return after(CHUNK, 1 if place.startswith("chunk1") else nchunks - 1)
    if place in ("y0", "y3", "cb", "cr"):
        slot = {"y0": 0, "y3": 3, "cb": 4, "cr": 5}[place]
        return lambda bi, s, e, prev, p: bi % b["upm"] == slot and bi >= lo + b["upm"]  # not in the interval's first MCU
    if place.startswith("interval"):
        return lambda bi, s, e, prev, p: bi == lo + 1  # the interval's second block
    raise KeyError(place)


def interval_of(b, place):
    if not b["marked"]:
        return 0
    n = b["n_intervals"]
    return {"interval0": 0, "interval-mid": n // 2, "interval-last": n - 1}.get(place, n - 1 if n < 3 else 1)


def places_of(path, kind):
    """the places a kind goes to on a path"""
    b = base(path)
    p = ["first", "lane-straddle", "lane-after", "last-block"]
    if not b["marked"]:
        p += ["chunk1-straddle", "chunk1-after", "lastchunk-straddle", "lastchunk-after"]
    if b["upm"] > 1:
        p = ["y0", "y3", "cb", "cr"]
    elif b["marked"]:
        p += ["interval0", "interval-mid", "interval-last"]
    how = KINDS[kind][1]
    if b["upm"] > 1 and not b["marked"] and kind in INTERLEAVED_HANDOFF:
        p += ["lane-straddle", "chunk1-straddle"]  # the block-in-MCU state across a lane and a chunk hand-off, one kind per class
    if how[0] == "marker" and how[2][1] == 0xD5 and b["marked"]:
        # the index cuts at every RSTm: a surplus one is defined in the last interval only, where it stays in the data
        p = ["interval-last"] if b["upm"] == 1 else p
    return p


INTERLEAVED_HANDOFF = ("ovf-zrl-at-49", "bad-ac-16-ones", "ood-in-code", "marker-eoi-in-code")


def _twin_planes(b, bi, at_shift, how):
    """the planes the legal twin of a "put" kind decodes to: the block's levels from the replaced symbol on are what the twin's items say"""
    planes = [p.copy() for p in b["planes"]]
    ci, by, bx = b["order"][bi]
    blk = planes[ci][by * 8:by * 8 + 8, bx * 8:bx * 8 + 8].reshape(64).copy()
    z = blk[E.ZZ]
    k = how[1] + at_shift + 1  # zig-zag index where the replaced symbol stands
    z[k:] = 0
    z[63] = 1 if how[3][1][-1][1] != 0xF0 else 0
    nat = np.zeros(64, dtype=np.int64)
    nat[E.ZZ] = z
    planes[ci][by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = nat.reshape(8, 8)
    return planes


def _make_in(b, scan0, st0, path, kind, place, k, only_block=None):
    klass, how = KINDS[kind]
    keep = _place_filter(b, st0, place, k)
    lo = k * b["per_interval"]
    for bi, at, s, nbits, prev, p in _candidates(b, st0, kind, k):
        if only_block is not None and bi != only_block:
            continue
        hostile_bits = nbits
        if how[0] == "put":
            ta = b["scan"]["comps"][[c[0] for c in b["scan"]["comps"]].index(b["order"][bi][0])][2]
            act = E.canonical_codes(*b["specs"][(1, ta)])
            hostile_bits = sum(len(it) if isinstance(it, str) else act[it[1]][1] + it[3] for it in how[2])  # the place is asserted afterwards
        if not keep(bi, s, s + (nbits if how[0] != "put" else hostile_bits) - 1, prev, p):
            continue
        c = Case(name=f"{path}/{kind}/{place}", path=path, kind=kind, place=place, klass=klass, interval=k, n_before=bi - lo, block=bi,
                 at=at, prev_bit=prev, twin_planes=b["planes"], b=b, st0=st0)
        if how[0] == "put":
            c.scan, c.stats = encode(b, inject=dict(block=bi, at=at, put=how[2]))
            if how[3] is not None:
                shift, items, drop = how[3]
                c.twin, _ = encode(b, inject=dict(block=bi, at=at + shift, put=items, drop_rest=drop))
                c.twin_planes = _twin_planes(b, bi, shift, how)
            else:
                c.twin = scan0
            c.span = (c.stats["inject_bit"], c.stats["inject_end_bit"] - 1)
        elif how[0] == "cut":
            c.scan, c.stats = encode(b, inject=dict(stop=(k, p, False)))
            c.twin = scan0
            c.span, c.cut = (s, s + nbits - 1), p
        else:
            c.scan, c.stats = encode(b, inject=dict(splice=(k, p, how[2])))
            c.twin = scan0
            c.span, c.cut = (s, s + nbits - 1), p
        try:
            c.check_place = lambda c=c: check_place(c)
            check_place(c)
        except AssertionError:
            continue
        return c
    return None


@functools.lru_cache(maxsize=None)
def make(path, kind, place):
    """one case of the regular matrix; raises LookupError when the scan holds no such place (the tests fail on that)"""
    b = base(path)
    scan0, st0 = trace(path)
    klass, how = KINDS[kind]
    k0 = interval_of(b, place)
    fixed = place.startswith("interval") or (b["marked"] and how[0] == "marker" and how[2][1] == 0xD5)
    # a place that is no interval of its own is looked for in every interval, the usual one first
    for k in [k0] + ([] if fixed else [j for j in range(b["n_intervals"]) if j != k0]):
        c = _make_in(b, scan0, st0, path, kind, place, k)
        if c is not None:
            return c
    if "chunk" in place:
        c = _make_shifted(b, st0, path, kind, place)
        if c is not None:
            return c
    raise LookupError(f"{path}: no symbol for {kind} at {place}")


def _stuffed_bits(st):
    """-> f(bit of the unstuffed data) = the same bit's position in the stuffed scan, in bits (scans of one interval)"""
    ff = np.asarray(st["stuffed"], dtype=np.int64)
    u = ff - np.arange(ff.size)  # unstuffed index of every data 0xFF
    return lambda bit: (bit // 8 + int(np.searchsorted(u, bit // 8, side="left"))) * 8 + bit % 8


def _make_shifted(b, st0, path, kind, place):
    """A scan has one byte 8192 * n, and the symbol a kind needs (a fixed index of a block, or a part of a symbol) seldom lies on it.
    So the bit stream is shifted: the tails of the two blocks in front of a nearby candidate are zeroed from some index on, which
    removes a known number of bits and leaves everything before them as it was.  The shift is chosen from the trace of the intact scan
    so that the candidate lands on the place; the shifted planes are then encoded and the case is made and asserted on them as any
    other (the prediction ignores stuffed bytes that come or go in the re-aligned stretch: a miss is simply not taken)."""
    how = KINDS[kind][1]
    syms = st0["symbols"][0]
    sb = _stuffed_bits(st0)
    nchunks = -(-st0["length"] // CHUNK)
    B8 = (1 if place.startswith("chunk1") else nchunks - 1) * CHUNK * 8
    per_block = {}
    for j, (bi, at, s0, cl, el) in enumerate(syms):
        per_block.setdefault(bi, []).append((at, s0, cl, el, syms[j - 1][2] if j else -1))

    def wanted(at, cl, el):
        if how[0] == "put":
            return at == how[1] if how[1] != "ac" else at not in ("dc", 0, 62)
        return {"code": cl >= 2, "dcx": at == "dc" and el > 0, "acx": at != "dc" and el > 0}[how[1]]

    def lands(S, Pv, cl, el, bits):
        if how[0] == "put":
            return S < B8 <= S + bits - 1 if place.endswith("straddle") else Pv < B8 <= S
        lo, hi = (S + 1, S + cl - 1) if how[1] == "code" else (S + cl, S + cl + el - 1)  # where the cut point may lie
        if place.endswith("straddle"):
            return lo <= B8 <= hi
        return Pv < B8 <= S and (hi // 8) * 8 >= lo

    def eob_bits(bi):
        ci = b["order"][bi][0]
        ta = [c for c in b["scan"]["comps"] if c[0] == ci][0][2]
        return E.canonical_codes(*b["specs"][(1, ta)])[0x00][1]

    def removals(bi):
        """{zig-zag index j the block is zeroed from (None: untouched): bits that removes}"""
        out, tail = {None: 0}, 0
        for at, s0, cl, el, _ in reversed(per_block[bi]):
            if at == "dc" or at < 1:
                break
            tail += cl + el
            out[at + 1] = tail - eob_bits(bi)
        return out

    tries = 0
    for bi in sorted(per_block):
        if bi < 2 or not B8 - 64 <= sb(per_block[bi][0][1]) <= B8 + 2048:
            continue
        r1s, r2s = removals(bi - 1), removals(bi - 2)
        for at, s0, cl, el, prev in per_block[bi]:
            if not wanted(at, cl, el):
                continue
            bits = cl + el
            if how[0] == "put":
                ta = [c for c in b["scan"]["comps"] if c[0] == b["order"][bi][0]][0][2]
                act = E.canonical_codes(*b["specs"][(1, ta)])
                bits = sum(len(it) if isinstance(it, str) else act[it[1]][1] + it[3] for it in how[2])
            hits = [(r1 + r2, j1, j2) for j1, r1 in r1s.items() for j2, r2 in r2s.items()
                    if lands(sb(s0) - r1 - r2, sb(prev) - (r1 + r2 if at != "dc" else r2 + (r1 if j1 is None else 0)), cl, el, bits)]
            for _, j1, j2 in sorted(hits, key=lambda h: h[0])[:3]:
                planes = [p.copy() for p in b["planes"]]
                for blk, j in ((bi - 1, j1), (bi - 2, j2)):
                    if j is not None:
                        ci, by, bx = b["order"][blk]
                        z = planes[ci][by * 8:by * 8 + 8, bx * 8:bx * 8 + 8].reshape(64)[E.ZZ]
                        z[j:] = 0
                        nat = np.zeros(64, dtype=np.int64)
                        nat[E.ZZ] = z
                        planes[ci][by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = nat.reshape(8, 8)
                b2 = dict(b, planes=planes)
                scan2, st2 = encode(b2, inject=dict(trace=True))
                c = _make_in(b2, scan2, st2, path, kind, place, 0, only_block=bi)
                tries += 1
                if c is not None:
                    return c
                if tries >= 40:
                    return None
    return None


def check_place(c):
    """assert the case's place from the hostile scan's own statistics"""
    b = base_of(c)
    st0 = getattr(c, "st0", None) or trace(c.path, getattr(c, "sparse", False))[1]
    st, k, marked = c.stats, c.interval, b["marked"]
    lane = MARKED_LANE if marked else LANE
    if marked:
        s_, e_ = st["intervals"][k]
        assert e_ - s_ <= 2048, "the marked decoder's sub-sequences are 8 bytes up to 2048 bytes of interval"
    cut = getattr(c, "cut", None)
    if cut is None:
        a, z = _rel(st, k, c.span[0], marked), _rel(st, k, c.span[1], marked)
    else:  # the symbol that is cut: its first bit in the hostile scan, its last bit in the intact one
        a, z = _rel(st0, k, c.span[0], marked), _rel(st0, k, c.span[1], marked)
        where = st.get("stop_offset", st.get("splice_offset")) - (st["intervals"][k][0] if marked else 0)
        assert a < where <= z, (a, where, z)
    prev = _rel(st0, k, c.prev_bit, marked) if c.prev_bit >= 0 else -1
    nchunks = -(-st0["length"] // CHUNK)
    lo = k * b["per_interval"]
    hi = lo + min(b["per_interval"], b["n_blocks"] - lo) - 1
    p = c.place
    if p == "first":
        assert c.block == lo
    elif p == "last-block":
        assert c.block == hi
    elif p.endswith("straddle"):
        unit = lane if p.startswith("lane") else CHUNK
        assert z // unit == a // unit + 1, (a, z)
        if unit == CHUNK:
            assert z // unit == (1 if p.startswith("chunk1") else nchunks - 1)
        if cut is not None:
            assert where % unit == 0 and where // unit == z // unit
    elif p.endswith("after"):
        unit = lane if p.startswith("lane") else CHUNK
        assert prev >= 0 and prev // unit == a // unit - 1, (prev, a)
        if unit == CHUNK:
            assert a // unit == (1 if p.startswith("chunk1") else nchunks - 1)
    elif p in ("y0", "y3", "cb", "cr"):
        assert c.block % b["upm"] == {"y0": 0, "y3": 3, "cb": 4, "cr": 5}[p] and b["order"][c.block][0] == {"y0": 0, "y3": 0, "cb": 1, "cr": 2}[p]
    elif p.startswith("interval"):
        assert k == {"interval0": 0, "interval-mid": b["n_intervals"] // 2, "interval-last": b["n_intervals"] - 1}[p]
    return True


# ------------------------------------------------------------------------------------------ special kinds
def _trim_for_pad(b, k, want):
    """planes whose interval k ends with `want` padding bits: the tail of its last block is zeroed from some index on"""
    lo = k * b["per_interval"]
    hi = lo + min(b["per_interval"], b["n_blocks"] - lo) - 1
    ci, by, bx = b["order"][hi]
    for j, first in ((j, first) for first in (None, 1, 2) for j in range(63, 1, -1)):  # (a level of size 1 costs an odd number of bits)
        planes = [p.copy() for p in b["planes"]]
        blk = planes[ci][by * 8:by * 8 + 8, bx * 8:bx * 8 + 8].reshape(64).copy()
        z = blk[E.ZZ]
        z[j:] = 0
        z[1] = z[1] if first is None else first
        nat = np.zeros(64, dtype=np.int64)
        nat[E.ZZ] = z
        planes[ci][by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = nat.reshape(8, 8)
        scan, st = encode(b, planes)
        if st["pad_bits"][k] == want:
            return planes, scan, st
    raise LookupError(f"no tail gives {want} padding bits")


@functools.lru_cache(maxsize=None)
def make_special(path, kind, where="last"):
    """the kinds that sit at the end of an interval's data, or are a whole interval or scan.  where: "first" / "mid" / "last" interval
    (marked paths; the unmarked scan is its own only interval)"""
    b = base(path)
    scan0, st0 = trace(path)
    n = b["n_intervals"]
    k = {"first": 0, "mid": n // 2, "last": n - 1}[where] if b["marked"] else 0
    lo = k * b["per_interval"]
    per = min(b["per_interval"], b["n_blocks"] - lo)
    c = Case(name=f"{path}/{kind}/interval-{where}" if b["marked"] else f"{path}/{kind}", path=path, kind=kind, place="end", klass=SPECIAL[kind],
             interval=k, n_before=per, twin=scan0, twin_planes=b["planes"], check_place=lambda: True)
    if kind in ("bad-16-bits-left", "bad-17-bits-left", "ood-15-bits-left"):
        # sixteen 1-bits in place of a symbol of the interval's last block, the data cut so that 17 / 16 / 15 bits of it are left
        left = int(kind.split("-")[1])
        for bi, at, s, cl, el in reversed(st0["symbols"][k]):  # the nearest to the interval's end: what follows it is cut off anyway
            if (s + left) % 8 == 0 and at != "dc":
                c.scan, c.stats = encode(b, inject=dict(block=bi, at=at, put=["1" * 17], drop_rest=True, stop=(k, s + left, False)))
                c.n_before, c.block = bi - lo, bi

                def place(c=c, s=s, left=left, k=k):
                    st = c.stats
                    assert st["inject_bit"] == s and (st["stop_offset"] - st["intervals"][k][0]) == len(_unstuffed(c.scan[st["intervals"][k][0]:st["stop_offset"]])) + c.scan[st["intervals"][k][0]:st["stop_offset"]].count(b"\xff\x00")
                    assert 8 * len(_unstuffed(c.scan[st["intervals"][k][0]:st["stop_offset"]])) - st["inject_bit"] == left
                    return True
                c.check_place = place
                return c
        raise LookupError(f"{path}: no symbol begins {left} bits before a byte boundary")
    if kind == "ood-after-block":  # the data ends on a byte boundary exactly after the interval's second block
        bi = lo + 1
        ci, by, bx = b["order"][bi]
        for j, first in ((j, first) for first in (None, 1, 2) for j in range(63, 1, -1)):
            planes = [p.copy() for p in b["planes"]]
            z = planes[ci][by * 8:by * 8 + 8, bx * 8:bx * 8 + 8].reshape(64)[E.ZZ]
            z[j:] = 0
            z[1] = z[1] if first is None else first
            nat = np.zeros(64, dtype=np.int64)
            nat[E.ZZ] = z
            planes[ci][by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = nat.reshape(8, 8)
            twin, st = encode(b, planes, inject=dict(trace=True))
            end = max(s + cl + el for x, at, s, cl, el in st["symbols"][k] if x == bi)
            if end % 8 == 0:
                c.scan, c.stats = encode(b, planes, inject=dict(stop=(k, end, False)))
                c.twin, c.twin_planes, c.n_before, c.block = twin, planes, 2, bi
                c.check_place = lambda c=c, k=k, end=end: c.stats["stop_offset"] == E.stuffed_offset(st, k, end)
                return c
        raise LookupError("no tail ends the block on a byte boundary")
    if kind == "ood-empty":
        c.scan, c.stats = encode(b, inject=dict(stop=(k, 0, False)))
        c.n_before = 0
        return c
    if kind == "ood-missing-interval":  # the scan ends before the last RSTm: the last interval has no marker and no data
        assert b["marked"] and n >= 2
        c.scan, c.stats = scan0[:st0["markers"][-1]], st0
        c.interval, c.n_before, c.name = n - 1, 0, f"{path}/{kind}"
        c.others = {n - 2: C.UNEXPECTED_MARKER}  # complete, but no marker follows it
        return c
    if kind == "marker-lone-ff-at-end":
        assert k == n - 1, "0xFF bytes before an RSTm are fill bytes (T.81 B.1.1.2): legal"
        c.scan, c.stats = encode(b, inject=dict(splice=(k, 1 << 40, b"\xff")))
        return c
    if kind == "marker-wrong-rst-after":
        assert b["marked"] and k < n - 1
        m = st0["markers"][k]
        c.scan, c.stats = scan0[:m + 1] + bytes([0xD0 + ((k + 3) & 7)]) + scan0[m + 2:], st0
        return c
    if kind == "left-one-0-bit":
        c.scan, c.stats = encode(b, inject=dict(append={k: "0"}))
        return c
    if kind == "left-extra-block":
        c.scan, c.stats = encode(b, inject=dict(append={k: [(0, 0, 0, 0), (1, 0x00, 0, 0)]}))
        return c
    if kind == "left-7-ones-then-ff":
        planes, twin, st = _trim_for_pad(b, k, 7)
        c.twin, c.twin_planes = twin, planes
        c.scan, c.stats = encode(b, planes, inject=dict(append={k: "1" * 15}))
        c.twin2 = _trim_for_pad(b, k, 0)  # (planes, scan, stats): no padding at all is legal too

        def place(c=c, k=k):
            s, e = c.stats["intervals"][k]
            assert c.scan[e - 2:e] == b"\xff\x00" and c.scan[e - 3] & 0x7F == 0x7F and st["pad_bits"][k] == 7 and c.twin2[2]["pad_bits"][k] == 0
            return True
        c.check_place = place
        return c
    raise KeyError(kind)


def _unstuffed(data):
    return bytes(data).replace(b"\xff\x00", b"\xff")


@functools.lru_cache(maxsize=None)
def make_sparse(path):
    """a table with one DC code and two AC codes: "11" is no code, and almost every pattern holds it"""
    b = base(path, True)
    scan0, st0 = trace(path, True)
    k = interval_of(b, "interval-mid")
    lo = k * b["per_interval"]
    for bi, at, s, cl, el in st0["symbols"][k]:
        if bi == lo + 1 and at == 5:
            scan, st = encode(b, inject=dict(block=bi, at=at, put=["11" + "0" * 16]))
            return Case(name=f"{path}/bad-sparse-table", path=path, kind="bad-sparse-table", place="mid", klass=C.BAD_CODE, interval=k,
                        n_before=bi - lo, block=bi, scan=scan, stats=st, twin=scan0, twin_planes=b["planes"], sparse=True, check_place=lambda: True)
    raise LookupError("no such symbol")


@functools.lru_cache(maxsize=None)
def make_dc_wrap(path, sign):
    """DC differences of +-2047 until the predictor passes the int16 range: not an error.  What is stored is (int16_t)pred."""
    marked = path.startswith("marked")
    W, H, comps, dri, seed = PATHS["marked-420" if marked else "unmarked-420"]
    frame = dict(width=64, height=32, comps=comps)
    scan = dict(comps=[(ci, min(ci, 1), min(ci, 1)) for ci in range(3)], dri=8 if marked else 0)  # one interval: 32 luma blocks
    order, n_mcus, upm = E.block_order(frame, scan)
    planes = [np.zeros(s, dtype=np.int64) for s in E.plane_shapes(frame)]
    pred = {0: 0, 1: 0, 2: 0}
    for i, (ci, by, bx) in enumerate(order):
        if ci == 0:
            pred[ci] += sign * 2047 if pred[ci] * sign <= 32767 + 2047 else -sign * 2047
        else:
            pred[ci] += (-sign if ci == 1 else sign) * 1000
        planes[ci][by * 8, bx * 8] = pred[ci]
        planes[ci][by * 8, bx * 8 + 1] = 1 + i % 7
    b = dict(frame=frame, scan=scan, planes=planes, specs=dict(K), marked=marked, upm=upm, order=order, n_blocks=len(order),
             per_interval=len(order), n_intervals=1, sparse=False, path=path)
    body, st = encode(b)
    assert max(int(np.abs(p).max()) for p in planes) > 32768 + 2047
    return b, body, st, [p.astype(np.int16) for p in planes]


def base_of(c):
    """the case's planes, frame and tables: the path's, or the shifted copy the case was found on (_make_shifted)"""
    return getattr(c, "b", None) or base(c.path, getattr(c, "sparse", False))


# ------------------------------------------------------------------------------------------ the list
def case_ids():
    """[(maker, args)] of every case, in a fixed order; nothing is encoded here"""
    ids = []
    for path in PATHS:
        b = base(path)
        for kind in KINDS:
            for place in places_of(path, kind):
                ids.append(("make", (path, kind, place)))
        wheres = ["first", "mid", "last"] if b["marked"] and b["upm"] == 1 else ["last"]
        for kind in ("bad-16-bits-left", "bad-17-bits-left", "ood-15-bits-left", "ood-after-block", "ood-empty", "left-one-0-bit", "left-7-ones-then-ff", "left-extra-block"):
            for w in wheres:
                ids.append(("make_special", (path, kind, w)))
        ids.append(("make_special", (path, "marker-lone-ff-at-end", "last")))
        if b["marked"]:
            ids.append(("make_special", (path, "ood-missing-interval", "last")))
            for w in (["first", "mid"] if b["upm"] == 1 else ["first"]):
                ids.append(("make_special", (path, "marker-wrong-rst-after", w)))
    for path in ("marked-grey", "unmarked-grey"):
        ids.append(("make_sparse", (path,)))
    return ids


def build(maker, args):
    return globals()[maker](*args)


def case_name(maker, args):
    return "/".join(args) if maker != "make_sparse" else f"{args[0]}/bad-sparse-table"
