"""JFIF container around the entropy-coded row segments of mdct_huffman_rows (host side, numpy only).

The device produces, per component plane, one unstuffed byte-aligned Huffman segment per block row
(restart interval = one block row, ITU-T T.81 E.1.4).  This module does what remains to obtain a
baseline JPEG any decoder opens: byte stuffing (B.1.1.5), RSTm markers between the rows, and the
marker segments (B.2: SOI, APP0/JFIF, DQT, SOF0, DHT, DRI, SOS, EOI).  One non-interleaved scan per
component, so a 4:2:0 picture is three scans (Y at full resolution, Cb / Cr at half) -- or, given the
scan of libmdct_jpegenc_scan.so, one interleaved scan (write_jpeg's `interleaved`).
No reference counterpart (the reference stops at the coefficient reorder, simd_dct.cpp:2221-2230).
"""
import struct

import numpy as np

from . import api


def _seg(marker, payload):
    return b"\xff" + bytes([marker]) + struct.pack(">H", len(payload) + 2) + payload


def _dht(table_class, table_id, bits, vals):
    return bytes([(table_class << 4) | table_id]) + bytes(bits) + bytes(vals)


def stuff(segment):
    """B.1.1.5: a zero byte after every 0xFF of entropy-coded data"""
    a = np.frombuffer(segment, dtype=np.uint8) if not isinstance(segment, np.ndarray) else segment
    ff = np.flatnonzero(a == 0xFF)
    if ff.size == 0:
        return a.tobytes()
    return np.insert(a, ff + 1, 0).tobytes()


def scan_bytes(segments, seg_bytes, seg_stride):
    """rows of one component -> stuffed entropy-coded data with RST0..RST7 between the rows"""
    out = []
    n = len(seg_bytes)
    for r in range(n):
        out.append(stuff(segments[r * seg_stride:r * seg_stride + int(seg_bytes[r])]))
        if r + 1 < n:
            out.append(b"\xff" + bytes([0xD0 + (r & 7)]))
    return b"".join(out)


def write_jpeg(components, width, height, specs=None, sampling=None, interleaved=None, *, table_per_component=False, colorspace=None):
    """components: list of 1 (grey) or 3 (Y, Cb, Cr with Cb/Cr at half resolution) dicts with keys
         'blocks_per_row', 'qtable' (64 integers 1..255, natural order v*8+u) and either
         'scan' (bytes / uint8 array: the stuffed, RST-delimited scan as mdct_jpeg_pack_rows leaves it) or
         'segments' (uint8 array / bytes), 'seg_bytes' (per block row), 'seg_stride' (stuffed and joined here)
       width, height: the image size the frame header states; each component's scan covers its own block grid, ceil(true size / 8)
         blocks per side of the component's true size ceil(width * h / hmax) x ceil(height * v / vmax) (T.81 A.2.2)
       specs: {which: (bits16, vals)} Huffman specifications (default: the library's, api.huffman_spec)
       sampling: [(h, v)] per component (default: (2, 2), (1, 1), (1, 1) for three components, (1, 1) for one)
       interleaved: None, or dict(scan=..., mcus_per_row=...) for three components: ONE scan whose MCUs interleave the components
         (T.81 A.2.3) replaces the per-component scans -- one DRI (= MCUs per row, the scan's restart interval), one SOS naming all
         three components (Y: tables 0/0, Cb and Cr: 1/1), the stuffed, RST-delimited scan as mdct_jpeg_pack_rows leaves it.  The
         components then need 'qtable' only.
       table_per_component: False: two quantisation tables are written, the first component's as table 0 and the second's as table 1,
         which the third shares.  True: every component's own 'qtable' is written; equal tables share an id, in order of appearance.
       colorspace: None, 'grey' or 'YCbCr': a JFIF APP0; 'RGB' (three components that are R, G, B, not converted): an Adobe APP14 with
         transform 0 and no APP0 -- read_jpeg reports it as 'RGB'.
       Returns the file as bytes."""
    specs = specs or {w: api.huffman_spec(w) for w in range(4)}
    zz = api.zigzag_table()
    nc = len(components)
    assert nc in (1, 3)
    if colorspace not in (None, "grey", "YCbCr", "RGB") or (colorspace == "grey") != (nc == 1 and colorspace is not None):
        raise ValueError(f"colorspace {colorspace!r} for {nc} components (None; 'grey' for one; 'YCbCr' or 'RGB' for three)")
    if colorspace == "RGB":
        f = [b"\xff\xd8", _seg(0xEE, b"Adobe" + struct.pack(">HHHB", 100, 0, 0, 0))]
    else:
        f = [b"\xff\xd8", _seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")]
    if table_per_component:
        qts, tq_of = [], []
        for c in components:
            key = [int(x) for x in np.asarray(c["qtable"]).reshape(64)]
            if key not in qts:
                qts.append(key)
            tq_of.append(qts.index(key))
    else:
        qts = [components[0]["qtable"]] + ([components[1]["qtable"]] if nc == 3 else [])
        tq_of = [min(ci, 1) for ci in range(nc)]
    for tq, q in enumerate(qts):
        q = np.asarray(q).reshape(64)
        assert np.all(q == np.rint(q)) and q.min() >= 1 and q.max() <= 255, "baseline DQT holds 8-bit integers"
        f.append(_seg(0xDB, bytes([tq]) + bytes(int(q[zz[k]]) for k in range(64))))
    sof = struct.pack(">BHHB", 8, height, width, nc)
    if sampling is None:
        sampling = [(1, 1)] if nc == 1 else [(2, 2), (1, 1), (1, 1)]
    assert len(sampling) == nc and all(1 <= h <= 4 and 1 <= v <= 4 for h, v in sampling), "sampling factors 1..4 per component"
    for ci, (h, v) in enumerate(sampling):
        sof += bytes([ci + 1, (h << 4) | v, tq_of[ci]])
    f.append(_seg(0xC0, sof))
    f.append(_seg(0xC4, _dht(0, 0, *specs[0]) + _dht(1, 0, *specs[1]) + (_dht(0, 1, *specs[2]) + _dht(1, 1, *specs[3]) if nc == 3 else b"")))
    if interleaved is not None:
        assert nc == 3, "an interleaved scan takes three components"
        f.append(_seg(0xDD, struct.pack(">H", interleaved["mcus_per_row"])))
        f.append(_seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])))
        f.append(bytes(memoryview(np.ascontiguousarray(interleaved["scan"]))))
        components = []
    for ci, c in enumerate(components):
        f.append(_seg(0xDD, struct.pack(">H", c["blocks_per_row"])))
        th = 0 if ci == 0 else 1
        f.append(_seg(0xDA, bytes([1, ci + 1, (th << 4) | th, 0, 63, 0])))
        f.append(bytes(memoryview(np.ascontiguousarray(c["scan"]))) if "scan" in c else scan_bytes(c["segments"], c["seg_bytes"], c["seg_stride"]))
    f.append(b"\xff\xd9")
    return b"".join(f)


def write_progressive_jpeg(qtables, width, height, sampling, scans, *, colorspace=None):
    """A progressive file (SOF2; T.81 Annex G: spectral selection, and successive approximation where a scan names it) around the scans
       of libmdct_jpegprog.so.
       qtables: one table per component (64 integers 1..255, natural order); equal tables share an id, in order of appearance
       sampling: [(h, v)] per component (1 or 3)
       scans: in file order, dicts with
         'components': [(component index, td, ta)] -- one component, or all three for an interleaved DC scan
         'ss', 'se': the band; 0, 0 is the DC scan, an AC band (1 <= ss <= se <= 63) takes one component (G.1.1.1.1)
         'ah', 'al': the scan's successive approximation (optional, 0 each; 0..13)
         'restart_interval': the scan's DRI, in MCUs (blocks of the component's own grid for one component)
         'tables': {(table class, id): (bits16, vals)} defined in a DHT in front of the scan (a later scan may redefine an id); empty
                   for a DC refinement scan, which uses none: no DHT is written
         'scan': bytes / uint8 array, the stuffed, RST-delimited scan as mdct_jpeg_pack_rows leaves it
       colorspace: as write_jpeg.
       Written are SOI, APP0 (or the Adobe APP14), DQT per table, SOF2, and per scan DHT, DRI, SOS and the data; then EOI.
       read_progressive_jpeg reads such a file back where every Ah and Al is 0, jfif_sof2.read_sof2_jpeg every one (read_jpeg refuses
       it, as it refuses every SOF2 file).  Returns the file as bytes."""
    zz = api.zigzag_table()
    nc = len(sampling)
    if nc not in (1, 3) or len(qtables) != nc:
        raise ValueError(f"{len(qtables)} tables for {nc} components (1 or 3 of each)")
    if colorspace not in (None, "grey", "YCbCr", "RGB") or (colorspace == "grey") != (nc == 1 and colorspace is not None):
        raise ValueError(f"colorspace {colorspace!r} for {nc} components (None; 'grey' for one; 'YCbCr' or 'RGB' for three)")
    if any(not (1 <= h <= 4 and 1 <= v <= 4) for h, v in sampling):
        raise ValueError(f"sampling factors {list(sampling)} (1..4)")
    if colorspace == "RGB":
        f = [b"\xff\xd8", _seg(0xEE, b"Adobe" + struct.pack(">HHHB", 100, 0, 0, 0))]
    else:
        f = [b"\xff\xd8", _seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")]
    qts, tq_of = [], []
    for q in qtables:
        q = np.asarray(q).reshape(-1)
        if q.size != 64 or np.any(q != np.rint(q)) or q.min() < 1 or q.max() > 255:
            raise ValueError("a DQT of 8-bit precision holds 64 integers 1..255")
        key = [int(x) for x in q]
        if key not in qts:
            qts.append(key)
        tq_of.append(qts.index(key))
    for tq, q in enumerate(qts):
        f.append(_seg(0xDB, bytes([tq]) + bytes(q[zz[k]] for k in range(64))))
    sof = struct.pack(">BHHB", 8, height, width, nc)
    for ci, (h, v) in enumerate(sampling):
        sof += bytes([ci + 1, (h << 4) | v, tq_of[ci]])
    f.append(_seg(0xC2, sof))
    for k, sc in enumerate(scans):
        comps, ss, se = list(sc["components"]), int(sc["ss"]), int(sc["se"])
        if not ((ss == 0 and se == 0 and len(comps) in (1, nc)) or (1 <= ss <= se <= 63 and len(comps) == 1)):
            raise ValueError(f"scan {k}: band {ss}..{se} of {len(comps)} components (the DC scan is 0..0; an AC band takes one component)")
        if any(not 0 <= ci < nc or td not in (0, 1) or ta not in (0, 1) for ci, td, ta in comps):
            raise ValueError(f"scan {k}: components {comps} (index, DC table 0 / 1, AC table 0 / 1)")
        if not 1 <= int(sc["restart_interval"]) <= 65535:
            raise ValueError(f"scan {k}: restart interval {sc['restart_interval']} (1..65535)")
        ah, al = int(sc.get("ah", 0)), int(sc.get("al", 0))
        if not (0 <= ah <= 13 and 0 <= al <= 13):
            raise ValueError(f"scan {k}: successive approximation Ah {ah}, Al {al} (0..13)")
        if sc["tables"]:
            f.append(_seg(0xC4, b"".join(_dht(tc, th, *spec) for (tc, th), spec in sorted(sc["tables"].items()))))
        f.append(_seg(0xDD, struct.pack(">H", int(sc["restart_interval"]))))
        f.append(_seg(0xDA, bytes([len(comps)]) + b"".join(bytes([ci + 1, (td << 4) | ta]) for ci, td, ta in comps) + bytes([ss, se, (ah << 4) | al])))
        f.append(bytes(memoryview(np.ascontiguousarray(sc["scan"]))))
    f.append(b"\xff\xd9")
    return b"".join(f)


class JpegFormatError(ValueError):
    """a file this reader refuses: malformed, or outside 8-bit baseline / extended-sequential Huffman JPEG with restart markers"""


_SOF_REFUSED = {0xC2: "progressive (SOF2)", 0xC3: "lossless (SOF3)", 0xC5: "hierarchical (SOF5)", 0xC6: "hierarchical progressive (SOF6)",
                0xC7: "hierarchical lossless (SOF7)", 0xC9: "arithmetic coding (SOF9)", 0xCA: "arithmetic progressive (SOF10)",
                0xCB: "arithmetic lossless (SOF11)", 0xCD: "arithmetic hierarchical (SOF13)", 0xCE: "arithmetic hierarchical progressive (SOF14)",
                0xCF: "arithmetic hierarchical lossless (SOF15)", 0xCC: "arithmetic conditioning (DAC)", 0xDC: "DNL"}


def _entropy_end(data, i):
    """offset of the first marker after entropy-coded data starting at i that is neither a stuffed 0xFF nor RSTm"""
    n, i0 = len(data), i
    while True:
        j = data.find(b"\xff", i)
        if j < 0 or j + 1 >= n:
            raise JpegFormatError("entropy-coded data runs to the end of the file (no EOI)")
        m = data[j + 1]
        if m == 0x00 or 0xD0 <= m <= 0xD7:
            i = j + 2
        elif m == 0xFF:
            i = j + 1  # fill byte before a marker
        else:
            k = j
            while k > i0 and data[k - 1] == 0xFF:  # fill bytes belong to the marker (a data 0xFF is followed by its stuffed zero)
                k -= 1
            return k


def read_jpeg(data, require_restart=True):
    """Parse a baseline (SOF0) or 8-bit extended-sequential Huffman (SOF1) JPEG with restart markers (ITU-T T.81 B.2); with
    require_restart=False also a scan without them (no DRI, or DRI 0), whose restart_interval is then 0.
    Returns a dict:
      width, height, sof (0xC0 / 0xC1),
      components: [{'id', 'h', 'v', 'tq'}] in frame order,
      qtables: {tq: uint16 [64] natural order (v*8+u)} as last defined,
      huffman: {(table_class, th): (bits16 list, vals list)} as last defined (class 0 DC, 1 AC),
      scans: [{'components': [{'index' (into components), 'td', 'ta'}], 'restart_interval', 'start', 'end' (byte range of the
               entropy-coded data in `data`, stuffed, RSTm included), 'huffman' / 'qtables' (the tables in force at the scan)}]
      colorspace: 'grey' (one component), 'YCbCr' or 'RGB' (three) as libjpeg decides it: a JFIF APP0 means YCbCr, else an Adobe
               APP14 decides (transform 0: RGB, any other: YCbCr), else component ids 'R', 'G', 'B' mean RGB and any others YCbCr;
               None for other component counts
    Refuses (JpegFormatError) progressive, lossless, hierarchical and arithmetic-coded files, 12-bit samples, 16-bit DQT, DNL,
    other than 1 or 3 components, and (require_restart=True) a scan without a restart interval (no DRI, or DRI 0)."""
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise JpegFormatError("no SOI")
    zz = api.zigzag_table()
    i, n = 2, len(data)
    frame, qt, ht, dri, scans = None, {}, {}, 0, []
    jfif, adobe = False, None  # APP0 'JFIF\0' seen; transform byte of the last APP14 'Adobe'
    while True:
        while i < n and data[i] == 0xFF and i + 1 < n and data[i + 1] == 0xFF:
            i += 1  # fill bytes
        if i + 2 > n or data[i] != 0xFF:
            raise JpegFormatError(f"expected a marker at offset {i}")
        m = data[i + 1]
        if m == 0xD9:
            break
        if m in (0x01,) or 0xD0 <= m <= 0xD7:
            raise JpegFormatError(f"marker 0x{m:02x} outside entropy-coded data")
        if i + 4 > n:
            raise JpegFormatError("truncated marker segment")
        L = struct.unpack_from(">H", data, i + 2)[0]
        seg = data[i + 4:i + 2 + L]
        if L < 2 or len(seg) != L - 2:
            raise JpegFormatError(f"truncated segment 0x{m:02x}")
        i += 2 + L
        if m in _SOF_REFUSED:
            raise JpegFormatError(f"not supported: {_SOF_REFUSED[m]}")
        if m in (0xC0, 0xC1):
            if frame is not None:
                raise JpegFormatError("a second frame header")
            if len(seg) < 6:
                raise JpegFormatError("malformed frame header")
            P, Y, X, nf = struct.unpack_from(">BHHB", seg)
            if P != 8:
                raise JpegFormatError(f"not supported: {P}-bit samples (8-bit only)")
            if nf not in (1, 3):
                raise JpegFormatError(f"not supported: {nf} components (1 or 3)")
            if Y == 0:
                raise JpegFormatError("not supported: height defined by DNL")
            if X == 0 or len(seg) < 6 + 3 * nf:
                raise JpegFormatError("malformed frame header")
            comps = []
            for c in range(nf):
                cid, hv, tq = seg[6 + 3 * c:9 + 3 * c]
                h, v = hv >> 4, hv & 15
                if h not in (1, 2) or v not in (1, 2) or tq > 3:
                    raise JpegFormatError(f"not supported: component {cid} sampling {h}x{v} / table {tq}")
                comps.append(dict(id=cid, h=h, v=v, tq=tq))
            frame = dict(width=X, height=Y, sof=m, components=comps)
        elif m == 0xDB:
            p = 0
            while p < len(seg):
                pq, tq = seg[p] >> 4, seg[p] & 15
                if pq != 0:
                    raise JpegFormatError("not supported: 16-bit DQT")
                if tq > 3 or p + 65 > len(seg):
                    raise JpegFormatError("malformed DQT")
                q = np.zeros(64, dtype=np.uint16)
                q[zz] = np.frombuffer(seg[p + 1:p + 65], dtype=np.uint8)
                qt[tq] = q
                p += 65
        elif m == 0xC4:
            p = 0
            while p < len(seg):
                tc, th = seg[p] >> 4, seg[p] & 15
                if tc > 1 or th > 1:
                    raise JpegFormatError(f"not supported: Huffman table class {tc} id {th} (two DC and two AC tables)")
                if p + 17 > len(seg):
                    raise JpegFormatError("malformed DHT")
                bits = list(seg[p + 1:p + 17])
                k = sum(bits)
                if p + 17 + k > len(seg):
                    raise JpegFormatError("malformed DHT")
                ht[(tc, th)] = (bits, list(seg[p + 17:p + 17 + k]))
                p += 17 + k
        elif m == 0xDD:
            if len(seg) != 2:
                raise JpegFormatError("malformed DRI")
            dri = struct.unpack(">H", seg)[0]
        elif m == 0xDA:
            if frame is None:
                raise JpegFormatError("SOS before the frame header")
            ns = seg[0] if seg else 0
            if ns < 1 or ns > 3 or len(seg) != 4 + 2 * ns:
                raise JpegFormatError("malformed SOS")
            ids = [c["id"] for c in frame["components"]]
            sc = []
            for k in range(ns):
                cid, t = seg[1 + 2 * k:3 + 2 * k]
                if cid not in ids:
                    raise JpegFormatError(f"SOS names component {cid} the frame lacks")
                sc.append(dict(index=ids.index(cid), td=t >> 4, ta=t & 15))
            ss, se, a = seg[1 + 2 * ns:4 + 2 * ns]
            if (ss, se, a) != (0, 63, 0):
                raise JpegFormatError("not supported: spectral selection / successive approximation")
            if ns > 1 and sum(frame["components"][c["index"]]["h"] * frame["components"][c["index"]]["v"] for c in sc) > 10:
                raise JpegFormatError("more than 10 blocks per MCU")
            if dri == 0 and require_restart:
                raise JpegFormatError("not supported: a scan without restart markers (no DRI or restart interval 0)")
            end = _entropy_end(data, i)
            scans.append(dict(components=sc, restart_interval=dri, start=i, end=end, huffman=dict(ht), qtables=dict(qt)))
            i = end
        elif 0xE0 <= m <= 0xEF or m == 0xFE:
            # APPn, COM: only the two that decide the colour space are read, at the lengths libjpeg requires of them
            if m == 0xE0 and len(seg) >= 14 and seg[:5] == b"JFIF\x00":
                jfif = True
            elif m == 0xEE and len(seg) >= 12 and seg[:5] == b"Adobe":
                adobe = seg[11]
        else:
            raise JpegFormatError(f"not supported: marker 0x{m:02x}")
    if frame is None or not scans:
        raise JpegFormatError("no frame or no scan")
    return dict(frame, qtables=qt, huffman=ht, scans=scans, colorspace=_colorspace(frame["components"], jfif, adobe))


def _colorspace(comps, jfif, adobe):
    """libjpeg's default_decompress_parms (jdapimin.c) for one and three components"""
    if len(comps) == 1:
        return "grey"
    if len(comps) != 3:
        return None
    if jfif:
        return "YCbCr"
    if adobe is not None:
        return "RGB" if adobe == 0 else "YCbCr"
    return "RGB" if [c["id"] for c in comps] == [ord("R"), ord("G"), ord("B")] else "YCbCr"


# ------------------------------------------------------------------------------------------ progressive files (SOF2)
def _segments(data):
    """(marker, offset of the payload, its length) of the marker segments from SOI to EOI, entropy-coded data skipped, by read_jpeg's
    walk; where read_jpeg would refuse the next segment the walk just ends"""
    i, n = 2, len(data)
    while i + 4 <= n and data[i] == 0xFF:
        m = data[i + 1]
        if m == 0xFF:
            i += 1  # fill byte
            continue
        L = struct.unpack_from(">H", data, i + 2)[0]
        if m in (0xD9, 0x01) or 0xD0 <= m <= 0xD7 or L < 2 or i + 2 + L > n:
            return
        yield m, i + 4, L - 2
        i += 2 + L
        if m == 0xDA:
            try:
                i = _entropy_end(data, i)
            except JpegFormatError:
                return


def sof_marker(data):
    """the marker code of the file's first frame header (SOFn: 0xC0 baseline, 0xC2 progressive, ...), found by walking the marker
    segments; None if there is none or the file is malformed before it.  Never raises."""
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        return None
    for m, _, _ in _segments(data):
        if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            return m
    return None


def read_progressive_jpeg(data):
    """Parse a progressive Huffman JPEG (SOF2) that uses spectral selection only (T.81 Annex G, Ah = Al = 0) and carries restart
    markers in every scan: what write_progressive_jpeg writes.  Returns read_jpeg's dict with sof = 0xC2; every scan also carries
    'ss', 'se', 'ah', 'al' (its band, zig-zag; ah = al = 0), and its 'huffman' and 'restart_interval' are those in force at it (such a
    file redefines DHT and DRI from scan to scan).  A DC scan's components carry a 'ta' and an AC scan's a 'td' the scan does not use.

    The rules for segments, frame header, DQT, DHT and the SOS header are read_jpeg's own: they are applied to a copy of the file whose
    frame marker is rewritten to SOF1 and whose bands to 0..63, which changes no length and no offset.  On top of them this refuses
    (JpegFormatError) a file that is not SOF2, successive approximation, a scan without restart markers, an interleaved AC scan, a band
    that mixes DC and AC or is out of order, a position of a component coded a second time, and an AC scan of a component whose DC scan
    has not come.  A band that no scan codes is legal: those coefficients are zero, as libjpeg decodes a truncated script."""
    data = bytes(data)
    sof = sof_marker(data)
    if sof != 0xC2:
        if sof is None:
            read_jpeg(data, require_restart=False)  # malformed before any frame header: its message
        raise JpegFormatError(f"not a progressive file: the frame header is SOF{(sof or 0xC0) - 0xC0}, not SOF2")
    twin, bands = bytearray(data), []
    for m, p, n in _segments(data):
        if m == 0xC2:
            twin[p - 3] = 0xC1
        elif m == 0xDA and n and n == 4 + 2 * data[p]:  # (any other SOS is malformed: read_jpeg says so)
            bands.append(tuple(data[p + n - 3:p + n]))
            twin[p + n - 3:p + n] = bytes([0, 63, 0])
    info = read_jpeg(bytes(twin), require_restart=False)
    info["sof"] = 0xC2
    coded = [set() for _ in info["components"]]
    for k, (sc, (ss, se, a)) in enumerate(zip(info["scans"], bands)):
        sc.update(ss=ss, se=se, ah=a >> 4, al=a & 15)
        if a:
            raise JpegFormatError(f"not supported: successive approximation (scan {k}: Ah {a >> 4}, Al {a & 15})")
        if sc["restart_interval"] == 0:
            raise JpegFormatError(f"not supported: a progressive scan without restart markers (scan {k}: no DRI or restart interval 0)")
        if ss > se or se > 63 or (ss == 0 and se != 0):
            raise JpegFormatError(f"malformed SOS: band {ss}..{se} (scan {k}; 0..0, or an AC band inside 1..63)")
        if ss > 0 and len(sc["components"]) > 1:
            raise JpegFormatError(f"malformed SOS: an interleaved AC scan (scan {k}: T.81 G.1.1.1.1)")
        for c in sc["components"]:
            if ss > 0 and 0 not in coded[c["index"]]:
                raise JpegFormatError(f"malformed file: an AC scan of component {c['index']} before its DC scan (scan {k})")
            if not coded[c["index"]].isdisjoint(range(ss, se + 1)):
                raise JpegFormatError(f"malformed file: a position of component {c['index']} is coded a second time (scan {k}: band {ss}..{se})")
            coded[c["index"]].update(range(ss, se + 1))
    return info
