"""Test-side encoder of progressive JPEG scans with successive approximation, written from ITU-T T.81 Annex G.1.2 and the rules of
libjpeg's jcphuff.c: encode_mcu_DC_first, encode_mcu_AC_first, encode_mcu_DC_refine and encode_mcu_AC_refine.  Serial Python; shares no
code with simd_dct_amd.  Writer, code tables and block order are jpeg_scan_encoder's, the plane-to-block view and the stuffing
jpeg_progressive_encoder's.  The truth of the ..._approx coders of libmdct_jpegprog.so: segments, symbol counts, losses.

A scan is coded over `units`, its blocks in scan order as (component, int64 [64] in zig-zag order), cut into restart intervals of
`per_interval` blocks (all of them: a scan without markers).

The rules.  DC first: the differences of dc >> al (arithmetic), the predictor 0 at every interval's start.  AC first: the level is
|v| >> al with v's sign, a level that becomes 0 is a zero; otherwise jpeg_progressive_encoder.ac_scan.  DC refinement: the raw bit
(dc >> al) & 1 per block.  AC refinement, with a[k] = |v[k]| >> al and EOB the last k of the band with a[k] == 1, walking k = ss..se:
a == 0: r++.  At a non-zero position, first: while r > 15 and k <= EOB, flush the pending run with its bits, emit ZRL, then the block's
buffered correction bits, r -= 16.  a > 1: buffer the bit a & 1.  a == 1: flush the pending run, emit (r << 4) | 1, a sign bit (1:
positive), the block's buffered bits; r = 0.  After the block: if r > 0 or bits are buffered the run grows by one and takes the
block's bits; it is flushed at once at 0x7FFF blocks or more than 937 bits, and at every interval's end.  A flush emits EOBn (none
for a run of 0), its n extra bits, then the buffered bits in order.  AC levels are clamped to +-1023 before the point transform in
every scan kind; the clamped ones are counted by first scans only.  DC differences beyond +-2047 are clamped and counted."""
import numpy as np

import jpeg_optimal_tables as T
import jpeg_progressive_encoder as PE
import jpeg_scan_encoder as E

FULL_RUN = 0x7FFF
MAX_BUFFERED = 937  # MAX_CORR_BITS - DCTSIZE2 + 1


def scan_units(frame, comps, planes):
    """-> ([(component, int64 [64] zig-zag)] in scan order, blocks per MCU, MCUs per row) for the scan over `comps` (component
    indices: one, over its own grid, or all, in MCU order); frame: jpeg_scan_encoder's (width, height, comps [(h, v)])"""
    scan = dict(comps=[(ci, 0, 0) for ci in comps])
    order, _, upm = E.block_order(frame, scan)
    gx = E.grid(frame, scan)[0]
    shapes = E.plane_shapes(frame)
    zz = {ci: PE.zz_blocks(planes[ci], shapes[ci][1] // 8, shapes[ci][0] // 8) for ci in comps}
    return [(ci, zz[ci][by, bx]) for ci, by, bx in order], upm, gx


class _Out:
    """the symbols of one scan: counted, and written if there are codes"""

    def __init__(self, codes):
        self.codes, self.w, self.uncoded = codes, None, 0

    def symbol(self, counts, sym, extra=0, n_extra=0):
        counts[sym] += 1
        if self.codes is not None:
            if sym in self.codes:
                self.w.put(*self.codes[sym])
            else:
                self.uncoded += 1
            self.w.put(extra, n_extra)

    def bits(self, bits):
        if self.codes is not None:
            for b in bits:
                self.w.put(b, 1)


def _intervals(units, per_interval):
    return [units[k:k + per_interval] for k in range(0, len(units), per_interval)]


def dc_first(units, per_interval, al, specs=None):
    """specs: {class: (bits16, vals)} with class 0 for component 0 and 1 for the others, or None (count only)
    -> dict(segs, counts int64 [2, 272], lost, uncoded)"""
    codes = None if specs is None else {cls: E.canonical_codes(*sp) for cls, sp in specs.items()}
    counts, lost, uncoded, segs = np.zeros((2, T.CLASS), dtype=np.int64), 0, 0, []
    for chunk in _intervals(units, per_interval):
        w, pred = E._Writer(), {}
        for ci, z in chunk:
            d = int(z[0]) >> al
            diff = d - pred.get(ci, 0)
            pred[ci] = d
            if abs(diff) > 2047:
                lost += 1
                diff = max(-2047, min(2047, diff))
            s = E.category(diff)
            cls = 1 if ci else 0
            counts[cls, s] += 1
            if codes is not None:
                if s in codes[cls]:
                    w.put(*codes[cls][s])
                else:
                    uncoded += 1
                w.put(PE._amp(diff, s), s)
        segs.append(w.finish()[0])
    return dict(segs=segs if codes is not None else None, counts=counts, lost=lost, uncoded=uncoded)


def dc_refine(units, per_interval, al):
    """-> dict(segs)"""
    segs = []
    for chunk in _intervals(units, per_interval):
        w = E._Writer()
        for _, z in chunk:
            w.put((int(z[0]) >> al) & 1, 1)
        segs.append(w.finish()[0])
    return dict(segs=segs)


def _eob_symbol(run):
    n = run.bit_length() - 1
    return n << 4, run - (1 << n), n


def ac_first(units, per_interval, ss, se, al, spec=None):
    """-> dict(segs, counts int64 [256], lost, uncoded, full_run_flushes)"""
    assert 1 <= ss <= se <= 63
    out = _Out(None if spec is None else E.canonical_codes(*spec))
    counts, lost, segs, full = np.zeros(256, dtype=np.int64), 0, [], 0
    for chunk in _intervals(units, per_interval):
        out.w = E._Writer()
        run = 0

        def flush():
            nonlocal run
            if run:
                out.symbol(counts, *_eob_symbol(run))
                run = 0

        for _, z in chunk:
            r = 0
            for k in range(ss, se + 1):
                v = int(z[k])
                if abs(v) > 1023:
                    lost += 1
                    v = max(-1023, min(1023, v))
                a = abs(v) >> al
                if a == 0:
                    r += 1
                    continue
                flush()
                while r > 15:
                    out.symbol(counts, 0xF0)
                    r -= 16
                s = a.bit_length()
                out.symbol(counts, (r << 4) | s, a if v > 0 else a ^ ((1 << s) - 1), s)
                r = 0
            if r > 0:
                run += 1
                if run == FULL_RUN:
                    full += 1
                    flush()
        flush()
        segs.append(out.w.finish()[0])
    return dict(segs=segs if spec is not None else None, counts=counts, lost=lost, uncoded=out.uncoded, full_run_flushes=full)


def ac_refine(units, per_interval, ss, se, al, spec=None):
    """-> dict(segs, counts int64 [256], lost = 0, uncoded, full_run_flushes, bit_flushes, max_buffered)"""
    assert 1 <= ss <= se <= 63
    out = _Out(None if spec is None else E.canonical_codes(*spec))
    counts, segs, full, over, most = np.zeros(256, dtype=np.int64), [], 0, 0, 0
    for chunk in _intervals(units, per_interval):
        out.w = E._Writer()
        run, buffered = 0, []

        def flush():
            nonlocal run, buffered
            if run:
                out.symbol(counts, *_eob_symbol(run))
                run = 0
            out.bits(buffered)
            buffered = []

        for _, z in chunk:
            a = [min(abs(int(v)), 1023) >> al for v in z]
            eob = max([k for k in range(ss, se + 1) if a[k] == 1], default=0)
            r, block_bits = 0, []
            for k in range(ss, se + 1):
                if a[k] == 0:
                    r += 1
                    continue
                while r > 15 and k <= eob:
                    flush()
                    out.symbol(counts, 0xF0)
                    r -= 16
                    out.bits(block_bits)
                    block_bits = []
                if a[k] > 1:
                    block_bits.append(a[k] & 1)
                    continue
                flush()
                out.symbol(counts, (r << 4) | 1)
                out.bits([1 if int(z[k]) > 0 else 0])
                out.bits(block_bits)
                block_bits = []
                r = 0
            if r > 0 or block_bits:
                run += 1
                buffered += block_bits
                most = max(most, len(buffered))
                if run == FULL_RUN or len(buffered) > MAX_BUFFERED:
                    full += run == FULL_RUN
                    over += run != FULL_RUN
                    flush()
        flush()
        segs.append(out.w.finish()[0])
    return dict(segs=segs if spec is not None else None, counts=counts, lost=0, uncoded=out.uncoded, full_run_flushes=full, bit_flushes=over, max_buffered=most)


def encode_scan(units, per_interval, ss, se, ah, al, specs=None):
    """one scan of any of the four kinds; specs: {class: spec} for a DC first scan, a spec for an AC scan, unused for DC refinement"""
    if ss == 0:
        return dc_refine(units, per_interval, al) if ah else dc_first(units, per_interval, al, specs)
    return (ac_refine if ah else ac_first)(units, per_interval, ss, se, al, specs)


def scan_data(segs):
    """unstuffed intervals -> the scan's entropy-coded bytes: stuffed, RSTm between the intervals"""
    return PE.scan_data(segs)
