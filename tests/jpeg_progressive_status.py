"""Test-side statement of what the GPU decoder of progressive scans (include/mdct_jpegdec_prog.h) leaves behind, good or bad: serial
Python written from ITU-T T.81 G.2 (decoding with EOBRUN, Ah = Al = 0) and E.1.4 on the bit reader and code tables of
jpeg_decode_checker.  Shares no code with simd_dct_amd.  Where jpeg_progressive_checker raises for anything wrong, this returns the
planes AND one MDCT_JPEGDEC_* status per restart interval, for any restart interval:

  an interval is OK when it holds exactly its blocks, then 1-bit padding to the byte, then RST(k mod 8) (nothing after the last one);
  otherwise its status is the first error in decoding order: OUT_OF_DATA, BAD_CODE, COEF_OVERFLOW (a level run past se, a ZRL past
  se + 1), UNEXPECTED_MARKER, LEFTOVER, or EOBRUN_OVERFLOW (an end-of-band run that names more blocks than the interval has left);
  a ZRL that ends exactly at se + 1 ends its block (jpeg_progressive_checker refuses that stream; a baseline decoder takes the same
  at 64);
  a DC scan writes position 0 of its blocks, an AC band the non-zero levels inside ss..se, and nothing else is touched;
  in a failing interval the blocks before the failing one keep their levels, the failing one what was decoded before the error (the
  block in which an overflowing EOBn was met is the failing one), and the band's positions of every later block are set to 0."""
import numpy as np

import jpeg_decode_checker as DC

OK, OUT_OF_DATA, BAD_CODE, COEF_OVERFLOW, UNEXPECTED_MARKER, LEFTOVER = range(6)
EOBRUN_OVERFLOW = 7


def block_order(gx, gy, layout):
    """the scan's blocks in decoding order as (component, block row, block column); layout = [(component, hh, vv, H, V)] per block of an
    MCU (one component over its own grid: [(ci, 0, 0, 1, 1)]); gx x gy MCUs"""
    return [(ci, (m // gx) * V + vv, (m % gx) * H + hh) for m in range(gx * gy) for ci, hh, vv, H, V in layout]


def _interval(rd, ss, se, tables, units, planes):
    """decode one interval's blocks into the planes; -> index of the block that failed (raises DC._Fail carrying it) or None"""
    n = len(units)
    u = 0
    try:
        if ss == 0:
            pred = {}
            for u, (ci, by, bx) in enumerate(units):
                s = rd.decode(tables[ci])
                pred[ci] = pred.get(ci, 0) + DC.extend(rd.receive(s), s)
                planes[ci][by * 8, bx * 8] = np.int64(pred[ci]).astype(np.int16)
            return
        while u < n:
            ci, by, bx = units[u]
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
                    z = DC.ZIGZAG[k]
                    planes[ci][by * 8 + z // 8, bx * 8 + z % 8] = DC.extend(rd.receive(s), s)
                    k += 1
                    if k == se + 1:
                        u += 1
                        break
    except DC._Fail as f:
        f.block = u
        raise


def decode_scan(scan, ss, se, tables, blocks, per_interval, planes):
    """One scan.  scan: its stuffed bytes, RSTm included; tables: {component: DC code table} (ss = 0) or the AC code table; blocks:
    block_order's list; per_interval: blocks per restart interval (DRI x blocks per MCU); planes: int16 arrays per component, written
    in place under the rules above.  -> [status per interval]"""
    n = -(-len(blocks) // per_interval)
    parts = DC.split_intervals(bytes(scan), n)
    statuses = []
    for k, (chunk, mk) in enumerate(parts):
        units = blocks[k * per_interval:(k + 1) * per_interval]
        rd = DC._Bits(chunk)
        try:
            _interval(rd, ss, se, tables, units, planes)
        except DC._Fail as f:
            statuses.append(f.status)
            for ci, by, bx in units[f.block + 1:]:
                for z in DC.ZIGZAG[ss:se + 1]:
                    planes[ci][by * 8 + z // 8, bx * 8 + z % 8] = 0
            continue
        rem = rd.bits[rd.pos:]
        if len(rem) >= 8 or not all(rem):
            statuses.append(LEFTOVER)
        elif rd.marker or (k != n - 1 and mk != k % 8):
            statuses.append(UNEXPECTED_MARKER)
        else:
            statuses.append(OK)
    return statuses


def decode(data):
    """A whole SOF2 file as jpeg_progressive_checker.parse reads it -> (planes int16 per component padded to the MCU grid, [statuses
    per scan]).  The scans' headers are taken as they are: what the format forbids about them is the checker's and the reader's matter."""
    import jpeg_progressive_checker as PC

    frame, _, scans, _ = PC.parse(data)
    fc = frame["components"]
    hmax, vmax = max(c[1] for c in fc), max(c[2] for c in fc)
    mx, my = -(-frame["width"] // (8 * hmax)), -(-frame["height"] // (8 * vmax))
    planes = [np.zeros((my * c[2] * 8, mx * c[1] * 8), dtype=np.int16) for c in fc]
    out = []
    for sc in scans:
        comps = sc["comps"]
        if len(comps) == 1:
            ci = comps[0][0]
            gx = -(-(-(-frame["width"] * fc[ci][1] // hmax)) // 8)
            gy = -(-(-(-frame["height"] * fc[ci][2] // vmax)) // 8)
            layout = [(ci, 0, 0, 1, 1)]
        else:
            gx, gy = mx, my
            layout = [(ci, hh, vv, fc[ci][1], fc[ci][2]) for ci, _, _ in comps for vv in range(fc[ci][2]) for hh in range(fc[ci][1])]
        tables = {ci: sc["huffman"][(0, td)] for ci, td, _ in comps} if sc["ss"] == 0 else sc["huffman"][(1, comps[0][2])]
        out.append(decode_scan(data[sc["start"]:sc["end"]], sc["ss"], sc["se"], tables, block_order(gx, gy, layout), sc["dri"] * len(layout), planes))
    return planes, out
