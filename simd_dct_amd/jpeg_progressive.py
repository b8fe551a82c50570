"""Progressive JPEG output on the GPU (libmdct_jpegprog.so, include/mdct_jpegprog.h): quantised coefficient
planes -> a SOF2 file with spectral selection (T.81 Annex G, Ah = Al = 0): one DC scan, then the scans of AC bands per component with
end-of-band runs, every scan with a restart interval per row and a Huffman table made for it.

prog_dc_histogram, prog_dc_rows, prog_ac_histogram and prog_ac_rows are thin wrappers of the C-ABI on device tensors; encode is what
jpeg_transcode.encode_coefficients(progressive=True) runs.  Successive approximation is out of scope.  jpeg_decode reads these files back
(jfif.read_progressive_jpeg, libmdct_jpegdec_prog.so).  torch is used for device memory and streams only.
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


def _hist(torch, hist, shape, like):
    if hist is None:
        hist = torch.empty(shape, dtype=torch.int32, device=like.device)
    if hist.dtype != torch.int32 or tuple(hist.shape) != shape or not hist.is_contiguous():
        raise ValueError(f"hist: a contiguous int32 tensor {list(shape)}")
    return hist


def prog_dc_histogram(planes, sampling, interleaved=False, cls=0, grids=None, hist=None, unrepresentable=None, stream=None, check=True):
    """mdct_jpegprog_dc_stats on device tensors: the counts of the DC categories prog_dc_rows emits.  planes: ONE int16 plane
    (interleaved=False, an interval per block row; cls: its class in the histogram) or three on one MCU grid (interleaved=True).
    hist: int32 [2, 272], zeroed by the call; unrepresentable: int32 [1] the caller zeroed (both allocated if None).  Otherwise as
    jpeg_transcode.coef_histogram."""
    import torch

    if not isinstance(interleaved, (bool, np.bool_)):
        raise ValueError(f"interleaved {interleaved!r}: a bool")
    arr = _plane_array(planes, sampling, grids)
    with api._on_stream(stream, planes[0].device):  # the fill of a word made here is ordered in front of the launch that adds to it
        hist = _hist(torch, hist, (2, HIST_CLASS), planes[0])
        if unrepresentable is None:
            unrepresentable = torch.zeros((1,), dtype=torch.int32, device=planes[0].device)
    rc = _jpegprog_lib.load().mdct_jpegprog_dc_stats(arr, len(planes), int(interleaved), cls, hist.data_ptr(), unrepresentable.data_ptr(), _stream(stream))
    if check and rc != 0:
        raise _error(rc)
    return (hist, unrepresentable) if check else (rc, hist, unrepresentable)


def prog_dc_rows(planes, sampling, specs, out, seg_bytes, ff_counts, uncoded, unrepresentable, interleaved=False, grids=None, seg_stride=None, r0=0, r1=None, stream=None,
                 check=True):
    """mdct_jpegprog_dc_rows on device tensors: the segments of the DC scan, one per block row (one plane) or MCU row (three planes,
    interleaved=True).  specs: [(bits16, vals)], one DC specification, or luminance and chrominance for the interleaved form.
    Otherwise as jpeg_transcode.coef_rows / coef_scan_rows."""
    if not isinstance(interleaved, (bool, np.bool_)):
        raise ValueError(f"interleaved {interleaved!r}: a bool")
    arr = _plane_array(planes, sampling, grids)
    sp = _Specs(dict(enumerate(specs)), tuple(range(len(specs))))
    per_row, rows = arr[len(planes) - 1].blocks_x, arr[len(planes) - 1].blocks_y
    if seg_stride is None:
        seg_stride = opt_seg_stride(per_row * (sum(h * v for h, v in sampling) if interleaved else 1))
    rc = _jpegprog_lib.load().mdct_jpegprog_dc_rows(arr, len(planes), int(interleaved), sp.arr, r0, rows if r1 is None else r1, out.data_ptr(), seg_stride,
                                                    seg_bytes.data_ptr(), ff_counts.data_ptr(), uncoded.data_ptr(), unrepresentable.data_ptr(), _stream(stream))
    if check and rc != 0:
        raise _error(rc)
    return rc


def prog_ac_histogram(plane, ss, se, grid=None, hist=None, unrepresentable=None, stream=None, check=True):
    """mdct_jpegprog_ac_stats on device tensors: the counts, by RRRRSSSS, of the symbols prog_ac_rows emits for the band ss..se of one
    int16 plane, the EOBn included.  hist: int32 [256], zeroed by the call; unrepresentable as above."""
    import torch

    p = _plane(plane, *(grid or (None, None)))
    with api._on_stream(stream, plane.device):
        hist = _hist(torch, hist, (AC_HIST,), plane)
        if unrepresentable is None:
            unrepresentable = torch.zeros((1,), dtype=torch.int32, device=plane.device)
    rc = _jpegprog_lib.load().mdct_jpegprog_ac_stats(p, ss, se, hist.data_ptr(), unrepresentable.data_ptr(), _stream(stream))
    if check and rc != 0:
        raise _error(rc)
    return (hist, unrepresentable) if check else (rc, hist, unrepresentable)


def prog_ac_rows(plane, ss, se, spec, out, seg_bytes, ff_counts, uncoded, unrepresentable, grid=None, seg_stride=None, by0=0, by1=None, stream=None, check=True):
    """mdct_jpegprog_ac_rows on device tensors: the band ss..se of one int16 plane -> one segment per block row, coded with
    spec = (bits16, vals).  Otherwise as jpeg_transcode.coef_rows."""
    p = _plane(plane, *(grid or (None, None)))
    sp = _Specs({0: spec}, (0,))
    if seg_stride is None:
        seg_stride = opt_seg_stride(p.blocks_x)
    rc = _jpegprog_lib.load().mdct_jpegprog_ac_rows(p, ss, se, by0, p.blocks_y if by1 is None else by1, sp.arr[0], out.data_ptr(), seg_stride, seg_bytes.data_ptr(),
                                                    ff_counts.data_ptr(), uncoded.data_ptr(), unrepresentable.data_ptr(), _stream(stream))
    if check and rc != 0:
        raise _error(rc)
    return rc


def encode(torch, coefs, tabs, width, height, sampling, mcus_x, mcus_y, colorspace, interleaved, bands, stream, saturate=False):
    """encode_coefficients(progressive=True) after its checks: every statistics launch, one copy of all histograms and the loss count,
    the tables, every coding and packing launch, one copy of the lengths, the file.  saturate: levels the coders had to clamp are no
    error (encode_jpeg: the pixel coders saturate AC levels to +-1023 by definition)."""
    nc = len(sampling)
    dev = coefs[0].device
    grids = [(pw // 8, ph // 8) for _, _, pw, ph in component_sizes(width, height, sampling)]
    # the scans in file order: (planes, samplings, grids or None, components, ss, se, intervals, blocks per interval)
    if interleaved:
        scans = [(list(coefs), sampling, None, list(range(nc)), 0, 0, mcus_y, mcus_x * sum(h * v for h, v in sampling))]
    else:
        scans = [([coefs[c]], [sampling[c]], [grids[c]], [c], 0, 0, grids[c][1], grids[c][0]) for c in range(nc)]
    n_dc = len(scans)
    scans += [([coefs[c]], [sampling[c]], [grids[c]], [c], ss, se, grids[c][1], grids[c][0]) for c in range(nc) for ss, se in bands[c]]
    n_ac = len(scans) - n_dc
    with torch.cuda.device(dev), api._on_stream(stream, dev):
        # one int32 block: the DC histograms, the AC histograms, then the words the kernels add to
        words = torch.zeros((n_dc * 2 * HIST_CLASS + n_ac * AC_HIST + 2,), dtype=torch.int32, device=dev)
        unrep, uncoded = words[-2:-1], words[-1:]
        dc_h = words[:n_dc * 2 * HIST_CLASS].view(n_dc, 2, HIST_CLASS)
        ac_h = words[n_dc * 2 * HIST_CLASS:-2].view(n_ac, AC_HIST)
        for k, (planes, samp, g, comps, ss, se, _, _) in enumerate(scans):
            if se == 0:
                prog_dc_histogram(planes, samp, interleaved=len(planes) == 3, cls=min(comps[0], 1), grids=g, hist=dc_h[k], unrepresentable=unrep, stream=stream)
            else:
                prog_ac_histogram(planes[0], ss, se, grid=g[0], hist=ac_h[k - n_dc], unrepresentable=unrep, stream=stream)
        w = words.cpu().numpy().astype(np.int64) & 0xFFFFFFFF  # the copy, on the call's stream, that waits for the histograms brings the loss count with it
        if w[-2] != 0 and not saturate:
            raise api.MdctError(f"{int(w[-2])} coefficients cannot be written in a progressive scan (AC outside +-1023 or DC difference outside +-2047)")
        dc_counts = w[:n_dc * 2 * HIST_CLASS].reshape(n_dc, 2, HIST_CLASS).sum(axis=0)
        dc_specs = [optimal_table(dc_counts[cls, :16]) for cls in range(min(nc, 2))]
        ac_specs = [optimal_table(c) for c in w[n_dc * 2 * HIST_CLASS:-2].reshape(n_ac, AC_HIST)]
        strides = [opt_seg_stride(per) for *_, per in scans]
        segs = [torch.empty((sc[6] * st,), dtype=torch.uint8, device=dev) for sc, st in zip(scans, strides)]
        counts = [torch.empty((2, sc[6]), dtype=torch.int32, device=dev) for sc in scans]
        packed, tables = [], []
        for k, (planes, samp, g, comps, ss, se, rows, per) in enumerate(scans):
            if se == 0:
                inter = len(planes) == 3
                specs = dc_specs if inter else [dc_specs[min(comps[0], 1)]]
                prog_dc_rows(planes, samp, specs, segs[k], counts[k][0], counts[k][1], uncoded, unrep, interleaved=inter, grids=g, seg_stride=strides[k], stream=stream)
                tables.append({(0, min(c, 1)): dc_specs[min(c, 1)] for c in comps})
            else:
                prog_ac_rows(planes[0], ss, se, ac_specs[k - n_dc], segs[k], counts[k][0], counts[k][1], uncoded, unrep, grid=g[0], seg_stride=strides[k], stream=stream)
                tables.append({(1, min(comps[0], 1)): ac_specs[k - n_dc]})
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
            out_scans.append(dict(components=[(c, min(c, 1), min(c, 1)) for c in sc[3]], ss=sc[4], se=sc[5], restart_interval=mcus, tables=tables[k],
                                  scan=out[:ends[k]].cpu().numpy()))
    return jfif.write_progressive_jpeg(tabs, width, height, sampling, out_scans, colorspace=colorspace)
