"""Independent CPU checker of the GPU JPEG decoder: a plain, serial baseline Huffman decoder written from ITU-T T.81 (B.2 marker
segments, Annex C code construction, F.2.2 decoding, E.1.4 restart intervals).  Shares no code with simd_dct_amd: its own marker
parser, its own code tables, its own bit reader.  Slow (Python); the tests feed it small pictures or single intervals.

Interval statuses follow include/mdct_jpegdec.h: 0 ok, 1 out of data, 2 invalid code, 3 coefficient index beyond 63,
4 unexpected marker (inside the data, or the marker after interval k is not RST(k mod 8)), 5 bits left over."""
import struct

import numpy as np

OK, OUT_OF_DATA, BAD_CODE, COEF_OVERFLOW, UNEXPECTED_MARKER, LEFTOVER = range(6)

# T.81 Figure A.6 built by walking the anti-diagonals: ZZ[k] = natural index row*8 + col
ZIGZAG = []
for s in range(15):
    cells = [(r, s - r) for r in range(8) if 0 <= s - r < 8]
    ZIGZAG += [r * 8 + c for r, c in (cells if s % 2 else cells[::-1])]


def parse(data):
    """-> (frame dict: width, height, components [(id, h, v, tq)], qt {tq: [64] natural}, scans [(components [(ci, td, ta)], dri, start,
    end, huffman {(tc, th): code dict})])"""
    i = 2
    qt, huff, dri, frame, scans = {}, {}, 0, None, []
    while True:
        m = data[i + 1]
        if m == 0xD9:
            break
        L = struct.unpack_from(">H", data, i + 2)[0]
        seg = data[i + 4:i + 2 + L]
        i += 2 + L
        if m in (0xC0, 0xC1):
            _, Y, X, nf = struct.unpack_from(">BHHB", seg)
            frame = dict(width=X, height=Y, components=[(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(nf)])
        elif m == 0xDB:
            p = 0
            while p < len(seg):
                q = [0] * 64
                for k in range(64):
                    q[ZIGZAG[k]] = seg[p + 1 + k]
                qt[seg[p] & 15] = q
                p += 65
        elif m == 0xC4:
            p = 0
            while p < len(seg):
                bits = seg[p + 1:p + 17]
                n = sum(bits)
                huff[(seg[p] >> 4, seg[p] & 15)] = code_table(bits, seg[p + 17:p + 17 + n])
                p += 17 + n
        elif m == 0xDD:
            dri = struct.unpack(">H", seg)[0]
        elif m == 0xDA:
            ns = seg[0]
            ids = [c[0] for c in frame["components"]]
            comps = [(ids.index(seg[1 + 2 * k]), seg[2 + 2 * k] >> 4, seg[2 + 2 * k] & 15) for k in range(ns)]
            j = i
            while not (data[j] == 0xFF and data[j + 1] not in (0x00, 0xFF) and not 0xD0 <= data[j + 1] <= 0xD7):
                j += 1
            end = j
            while end > i and data[end - 1] == 0xFF:  # B.1.1.2: fill bytes before the marker are not data
                end -= 1
            scans.append((comps, dri, i, end, dict(huff)))
            i = j
    return frame, qt, scans


def code_table(bits, vals):
    """Annex C: {(length, code): value}"""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[(length, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return table


def split_intervals(scan, n):
    """the scan's bytes -> n (data bytes, marker number after it or None) in the order of the RSTm markers; surplus markers stay in the
    last interval's data, missing intervals are (b'', None).  0xFF bytes directly before an RSTm are fill bytes (B.1.1.2), not data: a
    data 0xFF is always followed by its stuffed zero."""
    cuts = [p for p in range(len(scan) - 1) if scan[p] == 0xFF and 0xD0 <= scan[p + 1] <= 0xD7]
    out, s = [], 0
    for j in range(n - 1):
        if j < len(cuts):
            e = cuts[j]
            while e > s and scan[e - 1] == 0xFF:
                e -= 1
            out.append((scan[s:e], scan[cuts[j] + 1] - 0xD0))
            s = cuts[j] + 2
        else:
            out.append((b"", None) if s > len(scan) else (scan[s:], None))
            s = len(scan) + 2
    out.append((scan[s:] if s <= len(scan) else b"", None))
    return out


class _Bits:
    """F.2.2.5 NEXTBIT over one interval's stuffed bytes: 0xFF 0x00 -> 0xFF; any other 0xFF ends the data (a marker)"""

    def __init__(self, data):
        self.bits, self.marker = [], False
        i = 0
        while i < len(data):
            b = data[i]
            if b == 0xFF:
                if i + 1 < len(data) and data[i + 1] == 0:
                    i += 1
                else:
                    self.marker = True
                    break
            self.bits += [(b >> (7 - j)) & 1 for j in range(8)]
            i += 1
        self.pos = 0

    def end_error(self):
        return UNEXPECTED_MARKER if self.marker else OUT_OF_DATA

    def bit(self):
        if self.pos >= len(self.bits):
            raise _Fail(self.end_error())
        self.pos += 1
        return self.bits[self.pos - 1]

    def receive(self, s):
        v = 0
        for _ in range(s):
            v = (v << 1) | self.bit()
        return v

    def decode(self, table):
        """F.2.2.3 DECODE, one bit at a time"""
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.bit()
            if (length, code) in table:
                return table[(length, code)]
        raise _Fail(BAD_CODE)


class _Fail(Exception):
    def __init__(self, status):
        self.status = status


def extend(v, s):
    """F.2.2.1 EXTEND"""
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def decode_block(rd, dc_table, ac_table, seen=None):
    """F.2.2.1 / F.2.2.2 -> (DC difference, {zig-zag index: level}).  seen: a dict that receives what has been decoded of the block as
    it goes ("dc": the difference, zig-zag index: level), so that a caller still has it when the block fails."""
    s = rd.decode(dc_table)
    diff = extend(rd.receive(s), s)
    ac, k = ({} if seen is None else seen), 1
    if seen is not None:
        seen["dc"] = diff
    while k < 64:
        rs = rd.decode(ac_table)
        r, s = rs >> 4, rs & 15
        if s == 0:
            if r == 15:
                if k + 16 > 64:
                    raise _Fail(COEF_OVERFLOW)
                k += 16
                continue
            break
        k += r
        if k > 63:
            raise _Fail(COEF_OVERFLOW)
        ac[k] = extend(rd.receive(s), s)
        k += 1
    return diff, {k: v for k, v in ac.items() if k != "dc"}


def decode_interval(data, units, tables, marker_after, partial=False):
    """one restart interval: units = [(component, dc table, ac table, place)] in decoding order -> (status, [(place, 64 levels natural)]).
    partial=True -> (status, blocks, failing, n): failing = (place, 64 levels natural) of the block the decoder was in when it failed,
    holding what had been decoded of it (the DC only once its difference was complete; None when no block failed), n = the number of
    complete blocks before it."""
    rd = _Bits(data)
    pred, out = {}, []
    failing = None
    status = None
    try:
        for comp, dct, act, place in units:
            seen = {}
            failing = (comp, place, seen)
            diff, ac = decode_block(rd, tables[dct], tables[act], seen)
            pred[comp] = pred.get(comp, 0) + diff
            blk = np.zeros(64, dtype=np.int64)
            blk[0] = pred[comp]
            for k, v in ac.items():
                blk[ZIGZAG[k]] = v
            out.append((place, blk))
            failing = None
    except _Fail as f:
        status = f.status
    if status is None:
        rem = rd.bits[rd.pos:]
        if len(rem) >= 8 or not all(rem):
            status = LEFTOVER
        elif rd.marker:
            status = UNEXPECTED_MARKER
        else:
            status = OK if marker_after is None or marker_after[0] else UNEXPECTED_MARKER
    if not partial:
        return status, out
    if failing is not None:
        comp, place, seen = failing
        blk = np.zeros(64, dtype=np.int64)
        if "dc" in seen:
            blk[0] = pred.get(comp, 0) + seen["dc"]
        for k, v in seen.items():
            if k != "dc":
                blk[ZIGZAG[k]] = v
        failing = (place, blk)
    return status, out, failing, len(out)


def decode(data, intervals=None):
    """Whole file -> (coefficient planes int16 per component [blocks_y*8, blocks_x*8] padded to the MCU grid, per-scan status lists).
    intervals: {scan index: iterable of interval indices} decodes only those (others stay zero, status None)."""
    data = bytes(data)
    frame, qt, scans = parse(data)
    fc = frame["components"]
    hmax, vmax = max(c[1] for c in fc), max(c[2] for c in fc)
    mx, my = -(-frame["width"] // (8 * hmax)), -(-frame["height"] // (8 * vmax))
    planes = [np.zeros((my * c[2] * 8, mx * c[1] * 8), dtype=np.int16) for c in fc]
    statuses = []
    for si, (comps, dri, start, end, huff) in enumerate(scans):
        if len(comps) == 1:
            ci = comps[0][0]
            w = -(-frame["width"] * fc[ci][1] // hmax)
            h = -(-frame["height"] * fc[ci][2] // vmax)
            gx, gy = -(-w // 8), -(-h // 8)
            layout = [(ci, 0, 0, 1, 1)]
        else:
            gx, gy = mx, my
            layout = [(ci, hh, vv, fc[ci][1], fc[ci][2]) for ci, _, _ in comps for vv in range(fc[ci][2]) for hh in range(fc[ci][1])]
        tabs = {("dc", ci): huff[(0, td)] for ci, td, _ in comps}
        tabs.update({("ac", ci): huff[(1, ta)] for ci, _, ta in comps})
        total = gx * gy
        n = -(-total // dri)
        parts = split_intervals(data[start:end], n)
        want = None if intervals is None else set(intervals.get(si, ()))
        st = []
        for k, (chunk, mk) in enumerate(parts):
            if want is not None and k not in want:
                st.append(None)
                continue
            units = []
            for m in range(k * dri, min((k + 1) * dri, total)):
                ux, uy = m % gx, m // gx
                for ci, hh, vv, H, V in layout:
                    units.append((ci, ("dc", ci), ("ac", ci), (ci, uy * V + vv, ux * H + hh)))
            marker_after = None if k == n - 1 else ((mk is not None and mk == k % 8),)
            status, blocks = decode_interval(chunk, units, tabs, marker_after)
            if status == OK:
                for (ci, by, bx), blk in blocks:
                    planes[ci][by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = blk.reshape(8, 8).astype(np.int16)
            st.append(status)
        statuses.append(st)
    return planes, statuses, dict(frame=frame, qtables=[np.array(qt[c[3]], dtype=np.float32) for c in fc])
