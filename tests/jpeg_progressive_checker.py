"""Test-side decoder of progressive JPEG files (SOF2) with spectral selection only (Ah = Al = 0), written from ITU-T T.81 Annex G.2
(decoding with EOBRUN), B.2 (marker segments, a DRI and a DHT before any scan) and E.1.4 (restart intervals).  Serial Python on the bit
reader and code tables of jpeg_decode_checker; shares no code with simd_dct_amd or the progressive encoder.

decode(data) -> (coefficient planes int16 per component [blocks_y * 8, blocks_x * 8] padded to the MCU grid, info).  Anything the
format forbids or this checker does not read raises ValueError: successive approximation, an interleaved AC scan, a band that is coded
twice or never, a ZRL or a run past its band, an end-of-band run that crosses a restart interval, bits left over, a wrong RSTm."""
import struct

import numpy as np

import jpeg_decode_checker as DC


def parse(data):
    """-> (frame: sof, width, height, components [(id, h, v, tq)]; qt {tq: [64] natural}; scans [dict(comps [(ci, td, ta)], ss, se, ah,
    al, dri, start, end, huffman {(tc, th): code dict}, order: the marker codes of the segments since the previous scan)];
    head: the marker codes before the frame header)"""
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise ValueError("no SOI")
    i = 2
    qt, huff, dri, frame, scans, order, head = {}, {}, 0, None, [], [], []
    while True:
        if data[i] != 0xFF:
            raise ValueError(f"expected a marker at {i}")
        m = data[i + 1]
        if m == 0xD9:
            if i + 2 != len(data):
                raise ValueError("bytes after EOI")
            break
        L = struct.unpack_from(">H", data, i + 2)[0]
        seg = data[i + 4:i + 2 + L]
        i += 2 + L
        (order if frame is not None else head).append(m)
        if m in (0xC0, 0xC1, 0xC2):
            if frame is not None:
                raise ValueError("a second frame header")
            _, Y, X, nf = struct.unpack_from(">BHHB", seg)
            frame = dict(sof=m, width=X, height=Y, components=[(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(nf)])
        elif m == 0xDB:
            p = 0
            while p < len(seg):
                q = [0] * 64
                for k in range(64):
                    q[DC.ZIGZAG[k]] = seg[p + 1 + k]
                qt[seg[p] & 15] = q
                p += 65
        elif m == 0xC4:
            p = 0
            while p < len(seg):
                bits = seg[p + 1:p + 17]
                n = sum(bits)
                huff[(seg[p] >> 4, seg[p] & 15)] = DC.code_table(bits, seg[p + 17:p + 17 + n])
                p += 17 + n
        elif m == 0xDD:
            dri = struct.unpack(">H", seg)[0]
        elif m == 0xDA:
            ns = seg[0]
            ids = [c[0] for c in frame["components"]]
            comps = [(ids.index(seg[1 + 2 * k]), seg[2 + 2 * k] >> 4, seg[2 + 2 * k] & 15) for k in range(ns)]
            ss, se, a = seg[1 + 2 * ns:4 + 2 * ns]
            j = i
            while not (data[j] == 0xFF and data[j + 1] not in (0x00, 0xFF) and not 0xD0 <= data[j + 1] <= 0xD7):
                j += 1
            scans.append(dict(comps=comps, ss=ss, se=se, ah=a >> 4, al=a & 15, dri=dri, start=i, end=j, huffman=dict(huff), order=order))
            order = []
            i = j
        elif not (0xE0 <= m <= 0xEF or m == 0xFE):
            raise ValueError(f"marker 0x{m:02x}")
    if frame is None or not scans:
        raise ValueError("no frame or no scan")
    return frame, qt, scans, head


def _finish_interval(rd, eobrun, mk, k, last):
    rem = rd.bits[rd.pos:]
    if eobrun:
        raise ValueError(f"interval {k}: an end-of-band run of {eobrun} more blocks crosses the restart")
    if len(rem) >= 8 or not all(rem) or rd.marker:
        raise ValueError(f"interval {k}: bits left over, or a marker inside the data")
    if not last and mk != k % 8:
        raise ValueError(f"interval {k}: followed by RST{mk}")


def decode(data):
    frame, qt, scans, head = parse(data)
    if frame["sof"] != 0xC2:
        raise ValueError("not a progressive file (SOF2)")
    fc = frame["components"]
    hmax, vmax = max(c[1] for c in fc), max(c[2] for c in fc)
    mx, my = -(-frame["width"] // (8 * hmax)), -(-frame["height"] // (8 * vmax))
    planes = [np.zeros((my * c[2] * 8, mx * c[1] * 8), dtype=np.int16) for c in fc]
    coded = [np.zeros(64, dtype=np.int64) for _ in fc]  # how often each zig-zag position of a component was coded
    for si, sc in enumerate(scans):
        comps, ss, se, dri = sc["comps"], sc["ss"], sc["se"], sc["dri"]
        if sc["ah"] or sc["al"]:
            raise ValueError(f"scan {si}: successive approximation (Ah {sc['ah']}, Al {sc['al']})")
        if not (ss == se == 0 or (1 <= ss <= se <= 63 and len(comps) == 1)):
            raise ValueError(f"scan {si}: band {ss}..{se} of {len(comps)} components (G.1.1.1.1)")
        if dri == 0:
            raise ValueError(f"scan {si}: no restart interval")
        for ci, _, _ in comps:
            coded[ci][ss:se + 1] += 1
        if len(comps) == 1:
            ci = comps[0][0]
            gx = -(-(-(-frame["width"] * fc[ci][1] // hmax)) // 8)
            gy = -(-(-(-frame["height"] * fc[ci][2] // vmax)) // 8)
            layout = [(ci, 0, 0, 1, 1)]
        else:
            gx, gy = mx, my
            layout = [(ci, hh, vv, fc[ci][1], fc[ci][2]) for ci, _, _ in comps for vv in range(fc[ci][2]) for hh in range(fc[ci][1])]
        total = gx * gy
        n = -(-total // dri)
        parts = DC.split_intervals(data[sc["start"]:sc["end"]], n)
        if len(parts) != n:
            raise ValueError(f"scan {si}: {len(parts)} intervals for {n}")
        try:
            for k, (chunk, mk) in enumerate(parts):
                rd = DC._Bits(chunk)
                units = [(ci, (m // gx) * V + vv, (m % gx) * H + hh) for m in range(k * dri, min((k + 1) * dri, total)) for ci, hh, vv, H, V in layout]
                eobrun = 0
                if ss == 0:
                    tabs = {ci: sc["huffman"][(0, td)] for ci, td, _ in comps}
                    pred = {}
                    for ci, by, bx in units:
                        s = rd.decode(tabs[ci])
                        if s > 11:
                            raise ValueError(f"scan {si}: DC category {s}")
                        pred[ci] = pred.get(ci, 0) + DC.extend(rd.receive(s), s)
                        planes[ci][by * 8, bx * 8] = pred[ci]
                else:
                    tab = sc["huffman"][(1, comps[0][2])]
                    for ci, by, bx in units:
                        if eobrun:
                            eobrun -= 1
                            continue
                        kk = ss
                        while kk <= se:
                            rs = rd.decode(tab)
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r == 15:
                                    kk += 16
                                    if kk > se:
                                        raise ValueError(f"scan {si}: a ZRL runs past the band")
                                    continue
                                eobrun = (1 << r) + rd.receive(r) - 1
                                break
                            if s > 10:
                                raise ValueError(f"scan {si}: AC size {s}")
                            kk += r
                            if kk > se:
                                raise ValueError(f"scan {si}: a level past the band")
                            z = DC.ZIGZAG[kk]
                            planes[ci][by * 8 + z // 8, bx * 8 + z % 8] = DC.extend(rd.receive(s), s)
                            kk += 1
                _finish_interval(rd, eobrun, mk, k, k == n - 1)
        except DC._Fail as e:
            raise ValueError(f"scan {si}: decoding status {e.status}") from None
    for ci, c in enumerate(coded):
        if not np.all(c == 1):
            raise ValueError(f"component {ci}: zig-zag positions coded {c.tolist()} times")
    return planes, dict(frame=frame, scans=scans, head=head, qtables=[np.array(qt[c[3]], dtype=np.float32) for c in fc])
