"""Test-side encoder of progressive JPEG scans with spectral selection (Ah = Al = 0), written from ITU-T T.81 Annex G.1.2 and the
rules of libjpeg's jcphuff.c (encode_mcu_DC_first, encode_mcu_AC_first with Al = 0).  Serial Python; shares no code with simd_dct_amd
or the progressive checker.  The truth of the GPU coders of libmdct_jpegprog.so: segments, symbol counts, whole files.

Planes, frames and specifications are jpeg_scan_encoder's.  Every scan carries a restart interval per row: a block row of the
component's own grid (one component), or an MCU row (the interleaved DC scan).

The AC rules, per block of a band ss..se: a non-zero level first flushes the pending end-of-band run, then one ZRL (0xF0) per 16 zeros
since the last coded position inside the band, then RRRRSSSS and the amplitude bits; a block whose position se is zero adds 1 to the
run; a run of 0x7FFF is emitted at once; a run is the symbol n << 4, n = floor(log2(run)), then the low n bits of the run; the run is
flushed at the end of every interval.  Levels are clamped to +-1023 and DC differences to +-2047, and the clamped ones counted, as the
device does."""
import struct

import numpy as np

import jpeg_optimal_tables as T
import jpeg_scan_encoder as E

LUMA_BANDS, CHROMA_BANDS = [(1, 2), (3, 9), (10, 63)], [(1, 63)]
FULL_RUN = 0x7FFF


def _amp(v, s):
    return v if v >= 0 else v + (1 << s) - 1


def zz_blocks(plane, blocks_x, blocks_y):
    """-> int64 [blocks_y, blocks_x, 64] in zig-zag order"""
    p = np.asarray(plane, dtype=np.int64)[:blocks_y * 8, :blocks_x * 8]
    return p.reshape(blocks_y, 8, blocks_x, 8).transpose(0, 2, 1, 3).reshape(blocks_y, blocks_x, 64)[:, :, E.ZZ]


def dc_scan(frame, comps, planes, specs=None):
    """The DC-first scan of comps = [(component, td)]: one component over its own block grid, an interval per block row, or all three in
    MCU order, an interval per MCU row.  specs: {td: (bits16, vals)} or None (count only).
    -> (unstuffed bytes per interval or None, counts int64 [2, 272]: class 0 for component 0 and 1 for the others, entries 0..15,
    DC differences outside +-2047)"""
    scan = dict(comps=[(ci, td, 0) for ci, td in comps])
    order, n_mcus, upm = E.block_order(frame, scan)
    per_row = E.grid(frame, scan)[0]
    codes = None if specs is None else {ci: E.canonical_codes(*specs[td]) for ci, td in comps}
    counts, lost, segs = np.zeros((2, T.CLASS), dtype=np.int64), 0, []
    for k in range(n_mcus // per_row):
        w, pred = E._Writer(), {}
        for ci, by, bx in order[k * per_row * upm:(k + 1) * per_row * upm]:
            d = int(planes[ci][by * 8, bx * 8])
            diff = d - pred.get(ci, 0)
            pred[ci] = d
            if abs(diff) > 2047:
                lost += 1
                diff = max(-2047, min(2047, diff))
            s = E.category(diff)
            counts[1 if ci else 0, s] += 1
            if codes is not None:
                if s in codes[ci]:
                    w.put(*codes[ci][s])
                w.put(_amp(diff, s), s)
        segs.append(w.finish()[0])
    return (segs if codes is not None else None), counts, lost


def ac_scan(plane, blocks_x, blocks_y, ss, se, spec=None):
    """One band of one plane over blocks_x x blocks_y blocks, an interval per block row.  spec: (bits16, vals) or None (count only); a
    symbol the table lacks is written as its extra bits alone, as the device writes it, and counted in `uncoded`.
    -> (unstuffed bytes per interval or None, counts int64 [256] by RRRRSSSS, levels outside +-1023, uncoded)"""
    assert 1 <= ss <= se <= 63
    codes = None if spec is None else E.canonical_codes(*spec)
    z = zz_blocks(plane, blocks_x, blocks_y)[:, :, ss:se + 1]
    lost = int((np.abs(z) > 1023).sum())
    z = np.clip(z, -1023, 1023)
    busy = z.any(axis=2)
    counts, segs, uncoded = np.zeros(256, dtype=np.int64), [], 0
    for by in range(blocks_y):
        w = E._Writer()
        run = 0

        def symbol(sym, extra, n_extra):
            nonlocal uncoded
            counts[sym] += 1
            if codes is not None:
                if sym in codes:
                    w.put(*codes[sym])
                else:
                    uncoded += 1
                w.put(extra, n_extra)

        def flush():
            nonlocal run
            if run:
                n = run.bit_length() - 1
                symbol(n << 4, run - (1 << n), n)
                run = 0

        row_busy = busy[by]
        for bx in range(blocks_x):
            if not row_busy[bx]:
                run += 1
                if run == FULL_RUN:
                    flush()
                continue
            r = 0
            for v in z[by, bx].tolist():
                if v == 0:
                    r += 1
                    continue
                flush()
                while r > 15:
                    symbol(0xF0, 0, 0)
                    r -= 16
                s = E.category(v)
                symbol((r << 4) | s, _amp(v, s), s)
                r = 0
            if r > 0:
                run += 1
                if run == FULL_RUN:
                    flush()
        flush()
        segs.append(w.finish()[0])
    return (segs if codes is not None else None), counts, lost, uncoded


def scan_data(segs):
    """unstuffed intervals -> the scan's entropy-coded bytes: stuffed, RSTm between the intervals"""
    out = bytearray()
    for k, s in enumerate(segs):
        out += s.replace(b"\xff", b"\xff\x00")
        if k + 1 < len(segs):
            out += bytes([0xFF, 0xD0 + (k & 7)])
    return bytes(out)


def own_grid(frame, ci):
    """(blocks_x, blocks_y) of a component's own grid (T.81 A.2.2)"""
    gx, gy, _ = E.grid(frame, dict(comps=[(ci, 0, 0)]))
    return gx, gy


def default_bands(nc):
    return [list(LUMA_BANDS)] + [list(CHROMA_BANDS)] * (nc - 1)


def _dht(tc, th, spec):
    return bytes([(tc << 4) | th]) + bytes(spec[0]) + bytes(spec[1])


def encode_file(frame, planes, qtables=None, bands=None, interleaved_dc=True):
    """-> (a complete SOF2 file, [dict(comps, ss, se, dri, spec(s), counts) per scan]).  Tables are jpeg_optimal_tables.optimal_table's:
    one DC table per class over all DC scans, one AC table per AC scan.  Before every scan: DHT with the scan's tables (id 0 for the
    first component, 1 for the others), DRI, SOS."""
    nc = len(frame["comps"])
    bands = bands or default_bands(nc)
    if qtables is None:
        qtables = [np.ones(64, dtype=np.uint16)] + [np.full(64, 2, dtype=np.uint16)] * (nc - 1)
    f = [b"\xff\xd8", E._seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")]
    for tq in range(min(nc, 2)):
        q = np.asarray(qtables[tq]).reshape(64)
        f.append(E._seg(0xDB, bytes([tq]) + bytes(int(q[E.ZZ[k]]) for k in range(64))))
    sof = struct.pack(">BHHB", 8, frame["height"], frame["width"], nc)
    for ci, (h, v) in enumerate(frame["comps"]):
        sof += bytes([ci + 1, (h << 4) | v, min(ci, 1)])
    f.append(E._seg(0xC2, sof))
    dc_scans = [[(ci, min(ci, 1)) for ci in range(nc)]] if interleaved_dc and nc == 3 else [[(ci, min(ci, 1))] for ci in range(nc)]
    hist = sum(dc_scan(frame, comps, planes)[1] for comps in dc_scans)
    dc_specs = {cls: T.optimal_table(hist[cls, :16]) for cls in range(min(nc, 2))}
    info = []
    for comps in dc_scans:
        segs, counts, lost = dc_scan(frame, comps, planes, dc_specs)
        assert lost == 0
        dri = E.grid(frame, dict(comps=[(ci, td, 0) for ci, td in comps]))[0]
        f.append(E._seg(0xC4, b"".join(_dht(0, td, dc_specs[td]) for td in sorted({td for _, td in comps}))))
        f.append(E._seg(0xDD, struct.pack(">H", dri)))
        f.append(E._seg(0xDA, bytes([len(comps)]) + b"".join(bytes([ci + 1, td << 4]) for ci, td in comps) + bytes([0, 0, 0])))
        f.append(scan_data(segs))
        info.append(dict(comps=[ci for ci, _ in comps], ss=0, se=0, dri=dri, counts=counts))
    for ci in range(nc):
        gx, gy = own_grid(frame, ci)
        for ss, se in bands[ci]:
            _, counts, lost, _ = ac_scan(planes[ci], gx, gy, ss, se)
            assert lost == 0
            spec = T.optimal_table(counts)
            segs = ac_scan(planes[ci], gx, gy, ss, se, spec)[0]
            ta = min(ci, 1)
            f.append(E._seg(0xC4, _dht(1, ta, spec)))
            f.append(E._seg(0xDD, struct.pack(">H", gx)))
            f.append(E._seg(0xDA, bytes([1, ci + 1, ta, ss, se, 0])))
            f.append(scan_data(segs))
            info.append(dict(comps=[ci], ss=ss, se=se, dri=gx, counts=counts, spec=spec))
    f.append(b"\xff\xd9")
    return b"".join(f), info
