"""Test-side baseline JPEG encoder from known coefficients, written from ITU-T T.81: C.2 (canonical codes from BITS / HUFFVAL),
F.1.2 (DC difference and AC run/size coding, ZRL, EOB), B.1.1.5 (byte stuffing), E.1.4 (restart intervals), B.2 (marker segments).
Shares no code with simd_dct_amd or the decoding checker: the tests use it to make scans whose truth is the coefficient planes they
were made from, with any Huffman tables, sampling factors and restart interval, and to assert what a scan really contains.

Planes are int16 [blocks_y * 8, blocks_x * 8] in the decoder's layout: natural order (row v, column u of each block), not
dequantised, padded to the MCU grid.  The frame is dict(width, height, comps=[(h, v), ...]); a scan is dict(comps=[(component index,
td, ta), ...], dri=0, fill={interval: n}, fill_end=n), where fill puts n 0xFF fill bytes before the RSTm after that interval and
fill_end n before the marker that ends the scan (B.1.1.2); specs = {(table class, id): (bits16, vals)}."""
import collections
import struct

import numpy as np

# T.81 Figure A.6: zig-zag index k -> natural index row * 8 + column, walking the anti-diagonals
ZZ = []
for _d in range(15):
    _cells = [(_r, _d - _r) for _r in range(8) if 0 <= _d - _r < 8]
    ZZ += [r * 8 + c for r, c in (_cells if _d % 2 else _cells[::-1])]
ZZ = np.array(ZZ)


def spec_from_lengths(lengths):
    """{symbol: code length 1..16} -> (bits16, vals): symbols ordered by length, then as given.  Kraft's sum must stay below 1, so
    the all-ones code of the longest length is never assigned (T.81 C.2 / libjpeg)."""
    if not lengths:
        raise ValueError("no symbols")
    if any(not 1 <= n <= 16 for n in lengths.values()) or len(set(lengths)) != len(lengths) or any(not 0 <= s <= 255 for s in lengths):
        raise ValueError("code lengths 1..16, distinct 8-bit symbols")
    if sum(1 << (16 - n) for n in lengths.values()) >= 1 << 16:
        raise ValueError("Kraft's sum must be below 1 (the all-ones code stays unused)")
    order = sorted(lengths, key=lambda s: (lengths[s], list(lengths).index(s)))
    bits = [0] * 16
    for s in order:
        bits[lengths[s] - 1] += 1
    return bits, order


def canonical_codes(bits, vals):
    """T.81 C.2 (Figures C.1-C.3): {symbol: (code, length)}"""
    codes, code, k = {}, 0, 0
    for n in range(1, 17):
        for _ in range(bits[n - 1]):
            codes[vals[k]] = (code, n)
            code += 1
            k += 1
        if code > (1 << n):
            raise ValueError("over-subscribed table")
        code <<= 1
    return codes


def category(v):
    """the SSSS of a DC difference or AC level (F.1.2.1.1)"""
    return int(abs(int(v))).bit_length()


def grid(frame, scan):
    """(MCUs per interval row, MCU rows, [(component, h, v)] per block of the MCU) of one scan (A.2.2 / A.2.3)"""
    comps = frame["comps"]
    hmax, vmax = max(h for h, _ in comps), max(v for _, v in comps)
    W, H = frame["width"], frame["height"]
    if len(scan["comps"]) == 1:
        ci = scan["comps"][0][0]
        h, v = comps[ci]
        return -(-(-(-W * h // hmax)) // 8), -(-(-(-H * v // vmax)) // 8), [(ci, 0, 0, 1, 1)]
    layout = [(ci, hh, vv, comps[ci][0], comps[ci][1]) for ci, _, _ in scan["comps"] for vv in range(comps[ci][1]) for hh in range(comps[ci][0])]
    return -(-W // (8 * hmax)), -(-H // (8 * vmax)), layout


def plane_shapes(frame):
    """[(rows, columns)] of each component's coefficient plane, padded to the MCU grid"""
    comps = frame["comps"]
    hmax, vmax = max(h for h, _ in comps), max(v for _, v in comps)
    mx, my = -(-frame["width"] // (8 * hmax)), -(-frame["height"] // (8 * vmax))
    return [(my * v * 8, mx * h * 8) for h, v in comps]


def block_order(frame, scan):
    """[(component, block row, block column)] in decoding order"""
    gx, gy, layout = grid(frame, scan)
    return [(ci, my * V + vv, mx * H + hh) for my in range(gy) for mx in range(gx) for ci, hh, vv, H, V in layout], gx * gy, len(layout)


class _Writer:
    """bits -> bytes, a symbol at a time; the final byte padded with 1-bits (F.1.2.3)"""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        if self.n >= 32:
            m, r = self.n >> 3, self.n & 7
            self.out += (self.acc >> r).to_bytes(m, "big")
            self.acc &= (1 << r) - 1
            self.n = r

    def finish(self):
        pad = (8 - self.n % 8) % 8
        self.put((1 << pad) - 1, pad)
        self.out += self.acc.to_bytes(self.n >> 3, "big")
        self.acc, self.n = 0, 0
        return bytes(self.out), pad


def _new_stats():
    return dict(lengths=collections.defaultdict(collections.Counter), dc_categories=set(), dc_diffs=set(), ac_symbols=collections.Counter(),
                ac_values=set(), zrl_chains=collections.Counter(), blocks=0, zero_blocks=0, ends_at_63=0, max_block_bits=0,
                stuffed=[], markers=[], intervals=[], pad_bits=[], length=0)


def _put_items(w, items, dct, act):
    """write injected items: a str of '0' / '1' is raw bits; (table class 0 DC / 1 AC, symbol, extra, n_extra) is that symbol's code in
    the block's table followed by n_extra bits of extra"""
    for it in items:
        if isinstance(it, str):
            for ch in it:
                w.put(int(ch), 1)
        else:
            cls, sym, extra, n_extra = it
            code, n = (act if cls else dct)[sym]
            w.put(code, n)
            w.put(extra & ((1 << n_extra) - 1), n_extra)


def stuffed_offset(st, k, bit):
    """scan offset of the stuffed byte that holds bit `bit` (counted after unstuffing) of interval k's data, from encode_scan's stats
    (of a scan without spliced bytes before that bit)"""
    base = st["intervals"][k][0]
    o = base + bit // 8
    for f in st["stuffed"]:
        if base <= f < o:
            o += 1
    return o


def encode_scan(frame, scan, planes, specs, inject=None):
    """-> (entropy-coded bytes, stuffed and with RSTm markers; stats).  stats: lengths {(class, id): Counter(code length)} over every
    coded symbol, dc_categories / dc_diffs, ac_symbols (Counter of RS), ac_values, zrl_chains (Counter: ZRLs before a level), blocks,
    zero_blocks, ends_at_63 (blocks whose last level is at index 63: no EOB), max_block_bits, stuffed (offsets of the 0xFF of every
    stuffed pair), markers (offsets of every RSTm's 0xFF), intervals ([start, end) of each interval's data), pad_bits (per interval),
    length.

    inject (optional; without it the scan is what the planes say): a dict that writes something wrong at a chosen place.  Its keys:
      block, at, put[, drop_rest]: in block `block` (decoding order over the scan) the symbol at `at` -- "dc", or n for the n-th AC
        symbol the block would have (ZRLs, levels with their extra bits and the EOB each count as one) -- is replaced by the items of
        `put` (see _put_items; [] drops the symbol).  With drop_rest the block's remaining symbols are not written either.
      append: {interval: items} written after the interval's last block, before its padding.
      stop: (interval, bits, pad): the interval's bit stream is cut after `bits` bits; pad=True fills the last byte with 1-bits,
        pad=False drops a partial last byte.
      splice: (interval, bits, raw bytes): the bytes go into the interval's stuffed data, not stuffed themselves, in front of the byte
        that holds bit `bits` (a multiple of 8; the interval's length in bits or more: after its last byte).
      trace: True -> stats["symbols"] = per interval [(block, at, first bit, code bits, extra bits)] of every true symbol written.
    stats then also hold inject_interval, inject_bit / inject_end_bit (the first bit of the items of `put` and the bit after the
    last, counted in the interval's data after unstuffing), inject_offset / inject_end_offset (scan offsets of the stuffed bytes that
    hold the first and the last of those bits), stop_offset / splice_offset (scan offset where the data was cut / the bytes begin)."""
    inj = inject or {}
    order, n_mcus, upm = block_order(frame, scan)
    dri = scan.get("dri", 0) or n_mcus
    fill = scan.get("fill", {})
    tabs = {}
    for ci, td, ta in scan["comps"]:
        tabs[ci] = ((0, td), canonical_codes(*specs[(0, td)]), (1, ta), canonical_codes(*specs[(1, ta)]))
    st = _new_stats()
    out = bytearray()
    zz_planes = {}
    for ci, _, _ in scan["comps"]:
        p = np.asarray(planes[ci], dtype=np.int64)
        rows, cols = p.shape[0] // 8, p.shape[1] // 8
        zz_planes[ci] = p.reshape(rows, 8, cols, 8).transpose(0, 2, 1, 3).reshape(rows, cols, 64)[:, :, ZZ]
    n_int = -(-n_mcus // dri)
    if inj.get("trace"):
        st["symbols"] = [[] for _ in range(n_int)]
    for k in range(n_int):
        if inj:
            body, pad = _encode_interval_injected(k, order[k * dri * upm:min((k + 1) * dri, n_mcus) * upm], k * dri * upm, tabs, zz_planes, st, inj)
            _emit_interval(out, st, body, pad, k, inj)
            if k + 1 < n_int:
                out += b"\xff" * fill.get(k, 0)
                st["markers"].append(len(out))
                out += bytes([0xFF, 0xD0 + (k & 7)])
            continue
        w = _Writer()
        pred = {}
        for ci, by, bx in order[k * dri * upm:min((k + 1) * dri, n_mcus) * upm]:
            dck, dct, ack, act = tabs[ci]
            z = zz_planes[ci][by, bx]
            bits0 = len(w.out) * 8 + w.n
            diff = int(z[0]) - pred.get(ci, 0)
            pred[ci] = int(z[0])
            s = category(diff)
            if s > 11:
                raise ValueError(f"DC difference {diff} beyond category 11")
            code, n = dct[s]
            w.put(code, n)
            st["lengths"][dck][n] += 1
            w.put(diff if diff >= 0 else diff + (1 << s) - 1, s)
            st["dc_categories"].add(s)
            st["dc_diffs"].add(diff)
            nz = np.flatnonzero(z[1:]) + 1
            k0 = 1
            for pos in nz.tolist():
                v = int(z[pos])
                r = pos - k0
                chain = 0
                while r > 15:
                    code, n = act[0xF0]
                    w.put(code, n)
                    st["lengths"][ack][n] += 1
                    st["ac_symbols"][0xF0] += 1
                    r -= 16
                    chain += 1
                if chain:
                    st["zrl_chains"][chain] += 1
                s = category(v)
                if s > 10:
                    raise ValueError(f"AC level {v} beyond size 10")
                code, n = act[(r << 4) | s]
                w.put(code, n)
                st["lengths"][ack][n] += 1
                st["ac_symbols"][(r << 4) | s] += 1
                st["ac_values"].add(v)
                w.put(v if v >= 0 else v + (1 << s) - 1, s)
                k0 = pos + 1
            if k0 < 64:
                code, n = act[0x00]
                w.put(code, n)
                st["lengths"][ack][n] += 1
                st["ac_symbols"][0x00] += 1
            else:
                st["ends_at_63"] += 1
            st["blocks"] += 1
            st["zero_blocks"] += nz.size == 0
            st["max_block_bits"] = max(st["max_block_bits"], len(w.out) * 8 + w.n - bits0)
        data, pad = w.finish()
        a = np.frombuffer(data, dtype=np.uint8)
        ff = np.flatnonzero(a == 0xFF)
        base = len(out)
        st["stuffed"] += (base + ff + np.arange(ff.size)).tolist()
        out += np.insert(a, ff + 1, 0).tobytes() if ff.size else data
        st["intervals"].append((base, len(out)))
        st["pad_bits"].append(pad)
        if k + 1 < n_int:
            out += b"\xff" * fill.get(k, 0)
            st["markers"].append(len(out))
            out += bytes([0xFF, 0xD0 + (k & 7)])
    st["length"] = len(out)
    return bytes(out), st


def _encode_interval_injected(k, blocks, first_block, tabs, zz_planes, st, inj):
    """one interval's unstuffed bytes with the injection applied: the same symbols as encode_scan's own loop, listed first, then
    written one at a time so that one of them can be replaced.  Of the statistics only blocks, the trace and the injection's are kept."""
    w = _Writer()
    pred = {}
    now = lambda: len(w.out) * 8 + w.n  # noqa: E731
    for bi, (ci, by, bx) in enumerate(blocks, first_block):
        dck, dct, ack, act = tabs[ci]
        z = zz_planes[ci][by, bx]
        diff = int(z[0]) - pred.get(ci, 0)
        pred[ci] = int(z[0])
        s = category(diff)
        if s > 11:
            raise ValueError(f"DC difference {diff} beyond category 11")
        syms = [("dc", 0, s, diff if diff >= 0 else diff + (1 << s) - 1, s)]
        k0, n = 1, 0
        for pos in (np.flatnonzero(z[1:]) + 1).tolist():
            v, r = int(z[pos]), pos - k0
            while r > 15:
                syms.append((n, 1, 0xF0, 0, 0))
                n += 1
                r -= 16
            s = category(v)
            if s > 10:
                raise ValueError(f"AC level {v} beyond size 10")
            syms.append((n, 1, (r << 4) | s, v if v >= 0 else v + (1 << s) - 1, s))
            n += 1
            k0 = pos + 1
        if k0 < 64:
            syms.append((n, 1, 0x00, 0, 0))
        for at, cls, sym, extra, n_extra in syms:
            if inj.get("block") == bi and inj.get("at") == at:
                st["inject_interval"], st["inject_bit"] = k, now()
                _put_items(w, inj["put"], dct, act)
                st["inject_end_bit"] = now()
                if inj.get("drop_rest"):
                    break
                continue
            if "symbols" in st:
                st["symbols"][k].append((bi, at, now(), (act if cls else dct)[sym][1], n_extra))
            _put_items(w, [(cls, sym, extra, n_extra)], dct, act)
        st["blocks"] += 1
    if k in inj.get("append", {}):
        ci = blocks[-1][0]
        _put_items(w, inj["append"][k], tabs[ci][1], tabs[ci][3])
    st["interval_bits"] = st.get("interval_bits", []) + [now()]
    return w.finish()


def _emit_interval(out, st, data, pad, k, inj):
    """stuff one interval's bytes and append them to out, cut (stop) or with raw bytes spliced in (splice) as the injection says"""
    if inj.get("stop") and inj["stop"][0] == k:
        _, bits, padded = inj["stop"]
        nbytes, rem = bits // 8, bits % 8
        if rem and padded:
            data = data[:nbytes] + bytes([data[nbytes] | (0xFF >> rem)])
        else:
            data = data[:nbytes]
        pad = (8 - rem) % 8 if padded else 0
    a = np.frombuffer(data, dtype=np.uint8)
    ff = np.flatnonzero(a == 0xFF)
    base = len(out)
    stuffed = (base + ff + np.arange(ff.size)).tolist()
    body = np.insert(a, ff + 1, 0).tobytes() if ff.size else bytes(data)
    if inj.get("stop") and inj["stop"][0] == k:
        st["stop_offset"] = base + len(body)
    if inj.get("splice") and inj["splice"][0] == k:
        _, bits, raw = inj["splice"]
        if bits % 8:
            raise ValueError("bytes are spliced in at a byte boundary")
        j = min(bits // 8, len(a))
        at = j + int((ff < j).sum())
        body = body[:at] + bytes(raw) + body[at:]
        stuffed = [f if f < base + at else f + len(raw) for f in stuffed]
        st["splice_offset"] = base + at
    st["stuffed"] += stuffed
    out += body
    st["intervals"].append((base, len(out)))
    st["pad_bits"].append(pad)
    if st.get("inject_interval") == k and "inject_offset" not in st:
        st["inject_offset"] = stuffed_offset(st, k, st["inject_bit"])
        st["inject_end_offset"] = stuffed_offset(st, k, max(st["inject_bit"], st["inject_end_bit"] - 1))


def _seg(marker, payload):
    return bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + payload


# Annex K tables K.3-K.6: (bits16, vals)
ANNEX_K = {
    (0, 0): ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12))),
    (0, 1): ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12))),
    (1, 0): ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D], list(bytes.fromhex(
        "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748494a"
        "535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7"
        "c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"))),
    (1, 1): ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], list(bytes.fromhex(
        "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445464748"
        "494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4"
        "c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"))),
}


def encode_file(frame, scans, planes, specs, qtables=None, table_per_component=False, inject=None):
    """-> (a complete JFIF file, [stats of each scan, with 'start': the scan's first byte in the file]).  qtables: [64] natural order per
    component (default: 1 for the first component, 2 for the others); components take quantisation table 0 (first) / 1 (others), or
    with table_per_component table ci each (up to 4 components, T.81 B.2.4.1).  inject: {scan index: encode_scan's inject}."""
    nc = len(frame["comps"])
    if qtables is None:
        qtables = [np.ones(64, dtype=np.uint16)] + [np.full(64, 2, dtype=np.uint16)] * (nc - 1)
    tq_of = list(range(nc)) if table_per_component else [min(ci, 1) for ci in range(nc)]
    f = [b"\xff\xd8", _seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")]
    for tq in range(max(tq_of) + 1):
        q = np.asarray(qtables[tq]).reshape(64)
        f.append(_seg(0xDB, bytes([tq]) + bytes(int(q[ZZ[k]]) for k in range(64))))
    sof = struct.pack(">BHHB", 8, frame["height"], frame["width"], nc)
    for ci, (h, v) in enumerate(frame["comps"]):
        sof += bytes([ci + 1, (h << 4) | v, tq_of[ci]])
    f.append(_seg(0xC0, sof))
    f.append(_seg(0xC4, b"".join(bytes([(tc << 4) | th]) + bytes(b) + bytes(v) for (tc, th), (b, v) in sorted(specs.items()))))
    stats, dri = [], None
    for si, sc in enumerate(scans):
        if sc.get("dri", 0) != dri:
            dri = sc.get("dri", 0)
            f.append(_seg(0xDD, struct.pack(">H", dri)))
        f.append(_seg(0xDA, bytes([len(sc["comps"])]) + b"".join(bytes([ci + 1, (td << 4) | ta]) for ci, td, ta in sc["comps"]) + b"\x00\x3f\x00"))
        body, st = encode_scan(frame, sc, planes, specs, inject=(inject or {}).get(si))
        st["start"] = sum(map(len, f))
        f.append(body + b"\xff" * sc.get("fill_end", 0))
        stats.append(st)
    f.append(b"\xff\xd9")
    return b"".join(f), stats
