"""Test-side decoder of progressive JPEG files (SOF2) with spectral selection AND successive approximation, with or without restart
markers: ITU-T T.81 Annex G (G.1.2.1 DC, G.1.2.2 AC first scans with EOBRUN, G.1.2.3 and Figure G.7 AC refinement) in plain serial
Python, from the file to the coefficient planes, with one MDCT_JPEGDEC_* status per restart interval as include/mdct_jpegdec_prog.h
states them.  Built on the marker parser of jpeg_progressive_checker and on the bit reader and code tables of jpeg_decode_checker;
shares no code with simd_dct_amd.

  decode(data) -> (planes, statuses): int16 planes per component padded to the MCU grid; statuses[scan] = [status per interval].  A scan
  without restart markers (no DRI, or DRI 0) is one interval.  Decoding stops after the first scan with a failed interval (what later
  scans would make of its planes means nothing); statuses then ends with that scan.

An interval is OK when it holds exactly its blocks, then 1-bit padding to the byte, then RST(k mod 8) (nothing after the last one).
First scans (Ah = 0) follow jpeg_progressive_status, levels shifted left by Al.  In an AC refinement scan a symbol of size > 1 is
BAD_CODE, a run of positions without history (a ZRL's sixteen included) that ends past se is COEF_OVERFLOW, an EOBn that names more
blocks than the interval has left is EOBRUN_OVERFLOW.  What a failed refinement interval leaves in its blocks is not specified."""
import numpy as np

import jpeg_decode_checker as DC
import jpeg_progressive_checker as PC

OK, OUT_OF_DATA, BAD_CODE, COEF_OVERFLOW, UNEXPECTED_MARKER, LEFTOVER = range(6)
EOBRUN_OVERFLOW = 7


def _at(planes, unit, k):
    ci, by, bx = unit
    z = DC.ZIGZAG[k]
    return planes[ci], by * 8 + z // 8, bx * 8 + z % 8


def _i16(v):
    return np.int64(v).astype(np.int16)


def _first(rd, ss, se, al, tables, units, planes):
    """a first scan's interval; -> None, or raises DC._Fail with .block = the failing block"""
    n, u = len(units), 0
    try:
        if ss == 0:
            pred = {}
            for u, unit in enumerate(units):
                s = rd.decode(tables[unit[0]])
                pred[unit[0]] = pred.get(unit[0], 0) + DC.extend(rd.receive(s), s)
                p, y, x = _at(planes, unit, 0)
                p[y, x] = _i16(pred[unit[0]] << al)
            return
        while u < n:
            k = ss
            while True:
                rs = rd.decode(tables)
                r, s = rs >> 4, rs & 15
                if s == 0 and r == 15:
                    k += 16
                    if k > se + 1:
                        raise DC._Fail(COEF_OVERFLOW)
                    if k == se + 1:
                        u += 1
                        break
                elif s == 0:
                    run = (1 << r) + rd.receive(r)
                    if run > n - u:
                        raise DC._Fail(EOBRUN_OVERFLOW)
                    u += run
                    break
                else:
                    k += r
                    if k > se:
                        raise DC._Fail(COEF_OVERFLOW)
                    p, y, x = _at(planes, units[u], k)
                    p[y, x] = _i16(DC.extend(rd.receive(s), s) << al)
                    k += 1
                    if k == se + 1:
                        u += 1
                        break
    except DC._Fail as f:
        f.block = u
        raise


def _refine_dc(rd, al, units, planes):
    """G.1.2.1: one bit per block"""
    for unit in units:
        if rd.bit():
            p, y, x = _at(planes, unit, 0)
            p[y, x] = _i16(int(p[y, x]) | (1 << al))


def _correct(rd, planes, unit, k, p1):
    """the correction bit of a position with history: away from zero, where that bit is still clear"""
    p, y, x = _at(planes, unit, k)
    c = int(p[y, x])
    if rd.bit() and (c & p1) == 0:
        p[y, x] = _i16(c + (p1 if c >= 0 else -p1))


def _refine_ac(rd, ss, se, al, table, units, planes):
    """G.1.2.3, Figure G.7"""
    p1, n, eobrun = 1 << al, len(units), 0
    for u, unit in enumerate(units):
        k = ss
        if eobrun == 0:
            while k <= se:
                rs = rd.decode(table)
                r, s = rs >> 4, rs & 15
                if s > 1:
                    raise DC._Fail(BAD_CODE)
                if s == 1:
                    new = p1 if rd.bit() else -p1
                elif r != 15:
                    eobrun = (1 << r) + rd.receive(r)
                    if eobrun > n - u:
                        raise DC._Fail(EOBRUN_OVERFLOW)
                    break
                placed = False
                while k <= se:
                    p, y, x = _at(planes, unit, k)
                    if p[y, x] != 0:
                        _correct(rd, planes, unit, k, p1)
                    elif r == 0:
                        placed = True
                        break
                    else:
                        r -= 1
                    k += 1
                if not placed:
                    raise DC._Fail(COEF_OVERFLOW)
                if s:
                    p[y, x] = new
                k += 1
        if eobrun > 0:
            while k <= se:
                p, y, x = _at(planes, unit, k)
                if p[y, x] != 0:
                    _correct(rd, planes, unit, k, p1)
                k += 1
            eobrun -= 1


def decode_scan(scan, ss, se, ah, al, tables, blocks, per_interval, planes):
    """One scan.  scan: its stuffed bytes, RSTm included; tables: {component: DC code table} (a DC first scan), the AC code table (an AC
    scan) or None (a DC refinement scan); blocks: the scan's blocks in decoding order as (component, block row, block column);
    per_interval: blocks per restart interval (all of them for a scan without markers).  -> [status per interval]"""
    n = -(-len(blocks) // per_interval)
    statuses = []
    for k, (chunk, mk) in enumerate(DC.split_intervals(bytes(scan), n)):
        units = blocks[k * per_interval:(k + 1) * per_interval]
        rd = DC._Bits(chunk)
        try:
            if ah == 0:
                _first(rd, ss, se, al, tables, units, planes)
            elif ss == 0:
                _refine_dc(rd, al, units, planes)
            else:
                _refine_ac(rd, ss, se, al, tables, units, planes)
        except DC._Fail as f:
            statuses.append(f.status)
            if ah == 0:  # a first scan zeroes its band behind the failing block (include/mdct_jpegdec_prog.h)
                for unit in units[f.block + 1:]:
                    for kk in range(ss, se + 1):
                        p, y, x = _at(planes, unit, kk)
                        p[y, x] = 0
            continue
        rem = rd.bits[rd.pos:]
        if len(rem) >= 8 or not all(rem):
            statuses.append(LEFTOVER)
        elif rd.marker or (k != n - 1 and mk != k % 8):
            statuses.append(UNEXPECTED_MARKER)
        else:
            statuses.append(OK)
    return statuses


def scan_blocks(frame, comps):
    """(blocks in decoding order, blocks per MCU, MCUs per row) of a scan over `comps` [(component, td, ta)]: T.81 A.2.2 / A.2.3"""
    fc = frame["components"]
    hmax, vmax = max(c[1] for c in fc), max(c[2] for c in fc)
    if len(comps) == 1:
        ci = comps[0][0]
        gx = -(-(-(-frame["width"] * fc[ci][1] // hmax)) // 8)
        gy = -(-(-(-frame["height"] * fc[ci][2] // vmax)) // 8)
        layout = [(ci, 0, 0, 1, 1)]
    else:
        gx, gy = -(-frame["width"] // (8 * hmax)), -(-frame["height"] // (8 * vmax))
        layout = [(ci, hh, vv, fc[ci][1], fc[ci][2]) for ci, _, _ in comps for vv in range(fc[ci][2]) for hh in range(fc[ci][1])]
    blocks = [(ci, (m // gx) * V + vv, (m % gx) * H + hh) for m in range(gx * gy) for ci, hh, vv, H, V in layout]
    return blocks, len(layout), gx


def decode(data, stop_at_failure=True):
    data = bytes(data)
    frame, _, scans, _ = PC.parse(data)
    if frame["sof"] != 0xC2:
        raise ValueError("not a progressive file (SOF2)")
    fc = frame["components"]
    hmax, vmax = max(c[1] for c in fc), max(c[2] for c in fc)
    mx, my = -(-frame["width"] // (8 * hmax)), -(-frame["height"] // (8 * vmax))
    planes = [np.zeros((my * c[2] * 8, mx * c[1] * 8), dtype=np.int16) for c in fc]
    out = []
    for sc in scans:
        comps, ss, ah = sc["comps"], sc["ss"], sc["ah"]
        blocks, upm, _ = scan_blocks(frame, comps)
        tables = None if ss == 0 and ah else {ci: sc["huffman"][(0, td)] for ci, td, _ in comps} if ss == 0 else sc["huffman"][(1, comps[0][2])]
        per = sc["dri"] * upm if sc["dri"] else len(blocks)
        out.append(decode_scan(data[sc["start"]:sc["end"]], ss, sc["se"], ah, sc["al"], tables, blocks, per, planes))
        if stop_at_failure and any(out[-1]):
            break
    return planes, out
