"""Progressive JPEG output on the GPU (libmdct_jpegprog.so, include/mdct_jpegprog.h; DESIGN.md sections 4.12 and 4.12.1): quantised
coefficient planes -> a SOF2 file (T.81 Annex G), every scan with a restart interval per row and a Huffman table made for it.  By
default spectral selection alone (Ah = Al = 0): one DC scan, then the scans of AC bands per component with end-of-band runs.  With a
script, any legal sequence of the four scan kinds of G.1.2 -- DC and AC, first and refinement --, libjpeg's standard script
(standard_script: what Pillow's progressive=True, cjpeg -progressive and jpegtran -progressive write) among them.

prog_dc_histogram, prog_dc_rows, prog_ac_histogram and prog_ac_rows are thin wrappers of the C-ABI on device tensors (ah, al: the
..._approx calls); encode is what jpeg_transcode.encode_coefficients(progressive=True) runs.  jpeg_decode reads these files back
(jfif_sof2.read_sof2_jpeg, libmdct_jpegdec_prog.so).  torch is used for device memory and streams only.
"""
import numpy as np

from . import _jpegprog_lib, api, jfif
from .api import _stream
from .jpeg_encode import _Specs, _first_capacity, component_sizes, opt_seg_stride, optimal_table
from .jpeg_transcode import _pack, _plane, _plane_array

HIST_CLASS, AC_HIST = _jpegprog_lib.HIST_CLASS, _jpegprog_lib.AC_HIST
# the default script: the smallest file of the three scripts measured on the 8192 x 8192 4:2:0 q75 picture
LUMA_BANDS, CHROMA_BANDS = ((1, 2), (3, 9), (10, 63)), ((1, 63),)


last_error, _error = _jpegprog_lib.LIB.last_error, _jpegprog_lib.LIB.error


def check_bands(bands, nc):
    """bands of encode_coefficients -> [[(ss, se)]] per component: None is the default script (luma (1, 2), (3, 9), (10, 63); chroma (1, 63);
    grey as luma); otherwise per component a list of (ss, se) that tiles 1..63 in order, or ValueError"""
    if bands is None:
        return [list(LUMA_BANDS)] + [list(CHROMA_BANDS)] * (nc - 1)
    try:
        out = [[(int(ss), int(se)) for ss, se in b] for b in bands]
        exact = all(ss == a and se == b for o, g in zip(out, bands) for (ss, se), (a, b) in zip(o, g))
    except (TypeError, ValueError):
        raise ValueError(f"bands {bands!r}: per component a list of (ss, se)") from None
    if len(out) != nc or not exact:
        raise ValueError(f"bands {bands!r}: per component ({nc}) a list of integer (ss, se)")
    for ci, b in enumerate(out):
        nxt = 1
        for ss, se in b:
            if ss != nxt or se < ss or se > 63:
                raise ValueError(f"bands of component {ci}: {b} must tile 1..63 in order (band ({ss}, {se}) where {nxt} is next)")
            nxt = se + 1
        if nxt != 64:
            raise ValueError(f"bands of component {ci}: {b} must tile 1..63 (they end at {nxt - 1})")
    return out


def standard_script(nc):
    """libjpeg's jpeg_simple_progression for nc = 1 or 3 components as [(components, ss, se, ah, al)]: 6 scans for grey, 10 for colour
    (the chroma AC scans come Cr first)"""
    if nc == 1:
        return [((0,), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1), ((0,), 0, 0, 1, 0), ((0,), 1, 63, 1, 0)]
    if nc != 3:
        raise ValueError(f"{nc} components (1 or 3)")
    return [((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1), ((0, 1, 2), 0, 0, 1, 0),
            ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0)]


def bands_script(bands, nc, interleaved):
    """the script of the default output: the DC scan (interleaved, or one per component), then per component its bands, Ah = Al = 0"""
    dc = [(tuple(range(nc)), 0, 0, 0, 0)] if interleaved else [((c,), 0, 0, 0, 0) for c in range(nc)]
    return dc + [((c,), ss, se, 0, 0) for c in range(nc) for ss, se in bands[c]]


def check_script(script, nc):
    """A scan script -> [(components, ss, se, ah, al)] with tuples of ints, or ValueError naming the scan.  A scan is the DC scan (0, 0) of
    one component or of all nc in order, or an AC band 1 <= ss <= se <= 63 of one component (T.81 G.1.1.1.1); Al is 0..13.  Per
    component and position (G.1.1.1.2, as jfif_sof2.read_sof2_jpeg reads): a first scan (Ah = 0) codes a position no scan has coded, a
    refinement scan one whose last scan left Al = Ah, with Al = Ah - 1; a component's AC scans follow its DC first scan.  And the
    script is complete: every position 0..63 of every component ends at Al = 0."""
    try:
        out = [(tuple(int(c) for c in comps), int(ss), int(se), int(ah), int(al)) for comps, ss, se, ah, al in script]
        exact = all(tuple(o[0]) == tuple(g[0]) and tuple(o[1:]) == tuple(g[1:]) for o, g in zip(out, script))
    except (TypeError, ValueError):
        raise ValueError(f"script {script!r}: a list of (components, ss, se, ah, al)") from None
    if not exact or not out:
        raise ValueError(f"script {script!r}: a non-empty list of (components, ss, se, ah, al) of integers")
    last_al = [{} for _ in range(nc)]
    for k, (comps, ss, se, ah, al) in enumerate(out):
        if not comps or any(not 0 <= c < nc for c in comps) or (len(comps) > 1 and comps != tuple(range(nc))):
            raise ValueError(f"scan {k}: components {list(comps)} (one of 0..{nc - 1}, or all of them in order)")
        if not ((ss == 0 and se == 0) or 1 <= ss <= se <= 63):
            raise ValueError(f"scan {k}: band {ss}..{se} (the DC scan is 0..0, an AC band lies inside 1..63)")
        if ss > 0 and len(comps) > 1:
            raise ValueError(f"scan {k}: an AC band takes one component, not {list(comps)}")
        if not 0 <= al <= 13 or ah < 0:
            raise ValueError(f"scan {k}: successive approximation Ah {ah}, Al {al} (Al 0..13)")
        for c in comps:
            coded = last_al[c]
            if ss > 0 and 0 not in coded:
                raise ValueError(f"scan {k}: an AC scan of component {c} before its DC scan")
            for pos in range(ss, se + 1):
                if ah == 0 and pos in coded:
                    raise ValueError(f"scan {k}: position {pos} of component {c} is coded a second time")
                if ah != 0 and pos not in coded:
                    raise ValueError(f"scan {k}: a refinement of position {pos} of component {c}, which no scan has coded")
                if ah != 0 and (coded[pos] != ah or al != ah - 1):
                    raise ValueError(f"scan {k}: a refinement with Ah {ah}, Al {al} of position {pos} of component {c}, last coded with Al {coded[pos]}")
                coded[pos] = al
    for c in range(nc):
        for pos in range(64):
            if last_al[c].get(pos) != 0:
                raise ValueError(f"script: position {pos} of component {c} " + ("is coded by no scan" if pos not in last_al[c] else f"ends at Al {last_al[c][pos]}, not 0"))
    return out


def _hist(torch, hist, shape, like):
    if hist is None:
        hist = torch.empty(shape, dtype=torch.int32, device=like.device)
    if hist.dtype != torch.int32 or tuple(hist.shape) != shape or not hist.is_contiguous():
        raise ValueError(f"hist: a contiguous int32 tensor {list(shape)}")
    return hist


def prog_dc_histogram(planes, sampling, interleaved=False, cls=0, grids=None, hist=None, unrepresentable=None, stream=None, check=True, al=0):
    """mdct_jpegprog_dc_stats on device tensors: the counts of the DC categories prog_dc_rows emits.  planes: ONE int16 plane
    (interleaved=False, an interval per block row; cls: its class in the histogram) or three on one MCU grid (interleaved=True).
    hist: int32 [2, 272], zeroed by the call; unrepresentable: int32 [1] the caller zeroed (both allocated if None).  al: the point
    transform of a DC first scan (mdct_jpegprog_dc_stats_approx; a refinement scan has no symbols).  Otherwise as
    jpeg_transcode.coef_histogram."""
    import torch

    if not isinstance(interleaved, (bool, np.bool_)):
        raise ValueError(f"interleaved {interleaved!r}: a bool")
    arr = _plane_array(planes, sampling, grids)
    with api._on_stream(stream, planes[0].device):  # the fill of a word made here is ordered in front of the launch that adds to it
        hist = _hist(torch, hist, (2, HIST_CLASS), planes[0])
        if unrepresentable is None:
            unrepresentable = torch.zeros((1,), dtype=torch.int32, device=planes[0].device)
    rc = _jpegprog_lib.load().mdct_jpegprog_dc_stats_approx(arr, len(planes), int(interleaved), cls, 0, al, hist.data_ptr(), unrepresentable.data_ptr(), _stream(stream))
    if check and rc != 0:
        raise _error(rc)
    return (hist, unrepresentable) if check else (rc, hist, unrepresentable)


def prog_dc_rows(planes, sampling, specs, out, seg_bytes, ff_counts, uncoded, unrepresentable, interleaved=False, grids=None, seg_stride=None, r0=0, r1=None, stream=None,
                 check=True, ah=0, al=0):
    """mdct_jpegprog_dc_rows on device tensors: the segments of the DC scan, one per block row (one plane) or MCU row (three planes,
    interleaved=True).  specs: [(bits16, vals)], one DC specification, or luminance and chrominance for the interleaved form.
    ah, al: the scan's successive approximation (mdct_jpegprog_dc_rows_approx); ah = al + 1 is the refinement scan, one raw bit per
    block, which takes no table (specs None).  Otherwise as jpeg_transcode.coef_rows / coef_scan_rows."""
    if not isinstance(interleaved, (bool, np.bool_)):
        raise ValueError(f"interleaved {interleaved!r}: a bool")
    arr = _plane_array(planes, sampling, grids)
    sp = None if specs is None else _Specs(dict(enumerate(specs)), tuple(range(len(specs))))
    per_row, rows = arr[len(planes) - 1].blocks_x, arr[len(planes) - 1].blocks_y
    if seg_stride is None:
        seg_stride = opt_seg_stride(per_row * (sum(h * v for h, v in sampling) if interleaved else 1))
    rc = _jpegprog_lib.load().mdct_jpegprog_dc_rows_approx(arr, len(planes), int(interleaved), None if sp is None else sp.arr, ah, al, r0, rows if r1 is None else r1,
                                                           out.data_ptr(), seg_stride, seg_bytes.data_ptr(), ff_counts.data_ptr(), uncoded.data_ptr(),
                                                           unrepresentable.data_ptr(), _stream(stream))
    if check and rc != 0:
        raise _error(rc)
    return rc


def prog_ac_histogram(plane, ss, se, grid=None, hist=None, unrepresentable=None, stream=None, check=True, ah=0, al=0):
    """mdct_jpegprog_ac_stats on device tensors: the counts, by RRRRSSSS, of the symbols prog_ac_rows emits for the band ss..se of one
    int16 plane, the EOBn included.  hist: int32 [256], zeroed by the call; unrepresentable as above.  ah, al: the scan's successive
    approximation (mdct_jpegprog_ac_stats_approx): a first scan with a point transform, or with ah = al + 1 a refinement scan."""
    import torch

    p = _plane(plane, *(grid or (None, None)))
    with api._on_stream(stream, plane.device):
        hist = _hist(torch, hist, (AC_HIST,), plane)
        if unrepresentable is None:
            unrepresentable = torch.zeros((1,), dtype=torch.int32, device=plane.device)
    rc = _jpegprog_lib.load().mdct_jpegprog_ac_stats_approx(p, ss, se, ah, al, hist.data_ptr(), unrepresentable.data_ptr(), _stream(stream))
    if check and rc != 0:
        raise _error(rc)
    return (hist, unrepresentable) if check else (rc, hist, unrepresentable)


def prog_ac_rows(plane, ss, se, spec, out, seg_bytes, ff_counts, uncoded, unrepresentable, grid=None, seg_stride=None, by0=0, by1=None, stream=None, check=True, ah=0, al=0):
    """mdct_jpegprog_ac_rows on device tensors: the band ss..se of one int16 plane -> one segment per block row, coded with
    spec = (bits16, vals).  ah, al as prog_ac_histogram (mdct_jpegprog_ac_rows_approx).  Otherwise as jpeg_transcode.coef_rows."""
    p = _plane(plane, *(grid or (None, None)))
    sp = _Specs({0: spec}, (0,))
    if seg_stride is None:
        seg_stride = opt_seg_stride(p.blocks_x)
    rc = _jpegprog_lib.load().mdct_jpegprog_ac_rows_approx(p, ss, se, ah, al, by0, p.blocks_y if by1 is None else by1, sp.arr[0], out.data_ptr(), seg_stride,
                                                           seg_bytes.data_ptr(), ff_counts.data_ptr(), uncoded.data_ptr(), unrepresentable.data_ptr(), _stream(stream))
    if check and rc != 0:
        raise _error(rc)
    return rc


def encode(torch, coefs, tabs, width, height, sampling, mcus_x, mcus_y, colorspace, script, stream, saturate=False):
    """encode_coefficients(progressive=True) after its checks, for a checked script [(components, ss, se, ah, al)]: one statistics launch
    per Huffman scan (a DC refinement scan has none), one copy of all histograms and the loss count, the tables (a DC table per class
    over the DC first scans, an AC table per AC scan), one coding and one packing launch per scan, one copy of the lengths, the
    file.  saturate: levels the coders had to clamp are no error (encode_jpeg: the pixel coders saturate AC levels to +-1023 by
    definition)."""
    nc = len(sampling)
    dev = coefs[0].device
    grids = [(pw // 8, ph // 8) for _, _, pw, ph in component_sizes(width, height, sampling)]
    # the scans in file order: (planes, samplings, grids or None, components, ss, se, intervals, blocks per interval, ah, al)
    scans = []
    for comps, ss, se, ah, al in script:
        if len(comps) == 3:
            scans.append((list(coefs), sampling, None, list(comps), ss, se, mcus_y, mcus_x * sum(h * v for h, v in sampling), ah, al))
        else:
            c = comps[0]
            scans.append(([coefs[c]], [sampling[c]], [grids[c]], [c], ss, se, grids[c][1], grids[c][0], ah, al))
    dc_first = [k for k, sc in enumerate(scans) if sc[5] == 0 and sc[8] == 0]
    ac = [k for k, sc in enumerate(scans) if sc[5] != 0]
    n_dc, n_ac = len(dc_first), len(ac)
    with torch.cuda.device(dev), api._on_stream(stream, dev):
        # one int32 block: the DC histograms, the AC histograms, then the words the kernels add to
        words = torch.zeros((n_dc * 2 * HIST_CLASS + n_ac * AC_HIST + 2,), dtype=torch.int32, device=dev)
        unrep, uncoded = words[-2:-1], words[-1:]
        dc_h = words[:n_dc * 2 * HIST_CLASS].view(n_dc, 2, HIST_CLASS)
        ac_h = words[n_dc * 2 * HIST_CLASS:-2].view(n_ac, AC_HIST)
        for k, (planes, samp, g, comps, ss, se, _, _, ah, al) in enumerate(scans):
            if k in dc_first:
                prog_dc_histogram(planes, samp, interleaved=len(planes) == 3, cls=min(comps[0], 1), grids=g, hist=dc_h[dc_first.index(k)], unrepresentable=unrep, stream=stream,
                                  al=al)
            elif se != 0:
                prog_ac_histogram(planes[0], ss, se, grid=g[0], hist=ac_h[ac.index(k)], unrepresentable=unrep, stream=stream, ah=ah, al=al)
        w = words.cpu().numpy().astype(np.int64) & 0xFFFFFFFF  # the copy, on the call's stream, that waits for the histograms brings the loss count with it
        if w[-2] != 0 and not saturate:
            raise api.MdctError(f"{int(w[-2])} coefficients cannot be written in a progressive scan (AC outside +-1023 or DC difference outside +-2047)")
        dc_counts = w[:n_dc * 2 * HIST_CLASS].reshape(n_dc, 2, HIST_CLASS).sum(axis=0)
        dc_specs = [optimal_table(dc_counts[cls, :16]) for cls in range(min(nc, 2))]
        ac_specs = [optimal_table(c) for c in w[n_dc * 2 * HIST_CLASS:-2].reshape(n_ac, AC_HIST)]
        strides = [opt_seg_stride(sc[7]) for sc in scans]
        segs = [torch.empty((sc[6] * st,), dtype=torch.uint8, device=dev) for sc, st in zip(scans, strides)]
        counts = [torch.empty((2, sc[6]), dtype=torch.int32, device=dev) for sc in scans]
        packed, tables = [], []
        for k, (planes, samp, g, comps, ss, se, rows, per, ah, al) in enumerate(scans):
            if se == 0:
                inter = len(planes) == 3
                specs = None if ah else dc_specs if inter else [dc_specs[min(comps[0], 1)]]
                prog_dc_rows(planes, samp, specs, segs[k], counts[k][0], counts[k][1], uncoded, unrep, interleaved=inter, grids=g, seg_stride=strides[k], stream=stream, ah=ah,
                             al=al)
                tables.append({} if ah else {(0, min(c, 1)): dc_specs[min(c, 1)] for c in comps})
            else:
                spec = ac_specs[ac.index(k)]
                prog_ac_rows(planes[0], ss, se, spec, segs[k], counts[k][0], counts[k][1], uncoded, unrep, grid=g[0], seg_stride=strides[k], stream=stream, ah=ah, al=al)
                tables.append({(1, min(comps[0], 1)): spec})
            packed.append(_pack(torch, segs[k], counts[k], strides[k], rows, rows * per * (4 if se == 0 else 64), dev, stream))
        tail = torch.cat([off[-1:] for _, off in packed] + [words[-2:].to(torch.int64)]).cpu().tolist()  # the one copy that waits for the scans: it is ordered on the call's stream
        ends, lost, nocode = tail[:-2], tail[-2], tail[-1]
        if lost and not saturate:
            raise api.MdctError(f"{lost} coefficients cannot be written in a progressive scan (AC outside +-1023 or DC difference outside +-2047)")
        if nocode:
            raise api.MdctError(f"{nocode} symbols of the scans have no code in the tables made for them")
        out_scans = []
        for k, ((out, off), sc) in enumerate(zip(packed, scans)):
            if ends[k] > out.numel():  # the segments are there: only the packing runs again, into the worst case
                out = torch.empty((2 * sc[6] * strides[k],), dtype=torch.uint8, device=dev)
                api.jpeg_pack_rows(segs[k], counts[k][0], strides[k], sc[6], out, off, ff_counts=counts[k][1], stream=stream)
                ends[k] = int(off[-1].item())
            mcus = mcus_x if len(sc[0]) == 3 else sc[7]
            out_scans.append(dict(components=[(c, min(c, 1), min(c, 1)) for c in sc[3]], ss=sc[4], se=sc[5], ah=sc[8], al=sc[9], restart_interval=mcus, tables=tables[k],
                                  scan=out[:ends[k]].cpu().numpy()))
    return jfif.write_progressive_jpeg(tabs, width, height, sampling, out_scans, colorspace=colorspace)


def resolve_script(script, bands, nc, interleaved, sampling):
    """script / bands of the public entry points -> the checked script encode takes.  script None: bands (check_bands) with the DC scan
    `interleaved` selects; 'standard': standard_script; a list: check_script.  A scan of all three components needs the samplings the
    interleaved coders take (ValueError)."""
    if script is None:
        return bands_script(check_bands(bands, nc), nc, interleaved)
    if bands is not None:
        raise ValueError("script and bands: give one of them")
    out = standard_script(nc) if isinstance(script, str) and script == "standard" else None
    if out is None:
        if isinstance(script, str):
            raise ValueError(f"script {script!r} (None, 'standard' or a list of (components, ss, se, ah, al))")
        out = check_script(script, nc)
    if any(len(comps) == 3 for comps, *_ in out):
        from .jpeg_transcode import _check_interleaved

        try:
            _check_interleaved(sampling)
        except ValueError:
            raise ValueError(f"the script holds a scan of all three components, which takes sampling 4:4:4, 4:2:2 or 4:2:0, not {list(sampling)}") from None
    return out
