"""JPEG -> JPEG in the coefficient domain on the GPU (libmdct_jpegcoef.so, include/mdct_jpegcoef.h): what
jpegtran does.  The quantised coefficients a decode leaves are coded again -- with Huffman tables made for them, with a restart interval
per row, as three scans or one interleaved scan -- or flipped, transposed and rotated by quarter turns first.  No inverse or forward
DCT runs and nothing is quantised a second time, so the pixels a decoder gets from the output are those of the input (moved).

transcode_jpeg = jpeg_decode.decode_coefficients, transform_planes, encode_coefficients.  coef_histogram, coef_rows, coef_scan_rows and
transform_planes are thin wrappers of the C-ABI on device tensors.  torch is used for device memory and streams only.
"""
import numpy as np

from . import _jpegcoef_lib, api, jfif, jpeg_decode
from .api import _stream
from .jpeg_encode import _Specs, _ceil, _first_capacity, component_sizes, mcu_grid, opt_seg_stride, optimal_tables

TRANSFORMS = tuple(_jpegcoef_lib.OPS)
TRANSPOSING = ("transpose", "transverse", "rot90", "rot270")
# the SOURCE axes an operation mirrors: such an axis must be a whole number of iMCUs (the partial iMCU would land at the near edge)
MIRRORED = {"flip_h": "x", "flip_v": "y", "rot180": "xy", "transverse": "xy", "rot90": "y", "rot270": "x", "transpose": ""}
INTERLEAVED_LUMA = ((2, 2), (2, 1), (1, 1))


last_error, _error = _jpegcoef_lib.LIB.last_error, _jpegcoef_lib.LIB.error


def _plane(t, blocks_x=None, blocks_y=None, h=1, v=1, name="plane"):
    """an int16 tensor [rows, columns] with contiguous columns -> mdct_jpegcoef_plane over blocks_x x blocks_y blocks (default: all)"""
    if t.dim() != 2 or t.stride(1) != 1 or t.element_size() != 2:
        raise ValueError(f"{name}: int16 tensor [rows, columns] with contiguous columns")
    bx = t.shape[1] // 8 if blocks_x is None else blocks_x
    by = t.shape[0] // 8 if blocks_y is None else blocks_y
    if bx * 8 > t.shape[1] or by * 8 > t.shape[0]:
        raise ValueError(f"{name}: {bx} x {by} blocks in a tensor of {list(t.shape)}")
    return _jpegcoef_lib.Plane(t.data_ptr(), t.stride(0), bx, by, h, v)


def _plane_array(planes, sampling, grids=None):
    arr = (_jpegcoef_lib.Plane * max(1, len(planes)))()
    for k, (p, (h, v)) in enumerate(zip(planes, sampling)):
        bx, by = grids[k] if grids is not None else (None, None)
        arr[k] = _plane(p, bx, by, h, v, f"plane {k}")
    return arr


def coef_histogram(planes, sampling, interleaved=False, grids=None, hist=None, unrepresentable=None, stream=None, check=True):
    """mdct_jpegcoef_stats on device tensors: the counts of the Huffman symbols that coef_rows / coef_scan_rows emit for these planes.
    planes: 1 or 3 int16 [rows, columns] coefficient planes with contiguous columns; sampling: [(h, v)] per component; grids:
    [(blocks_x, blocks_y)] per plane, the blocks to count (default: the whole tensor).  interleaved=False: every plane a scan of its
    own, an interval per block row; True: three planes on one MCU grid, an interval per MCU row.  hist: int32 device tensor [2, 272]
    (allocated if None), zeroed by the call itself.  unrepresentable: int32 device tensor of one element that the CALLER has zeroed
    (allocated and zeroed if None); the call adds the AC levels outside +-1023 and DC differences outside +-2047.
    Returns (hist, unrepresentable) (with check=False: (status, hist, unrepresentable))."""
    import torch

    if not isinstance(interleaved, (bool, np.bool_)):
        raise ValueError(f"interleaved {interleaved!r}: a bool")
    arr = _plane_array(planes, sampling, grids)
    with api._on_stream(stream, planes[0].device):  # the fill of a word made here is ordered in front of the launch that adds to it
        if hist is None:
            hist = torch.empty((2, _jpegcoef_lib.HIST_CLASS), dtype=torch.int32, device=planes[0].device)
        if unrepresentable is None:
            unrepresentable = torch.zeros((1,), dtype=torch.int32, device=planes[0].device)
    if hist.dtype != torch.int32 or tuple(hist.shape) != (2, _jpegcoef_lib.HIST_CLASS) or not hist.is_contiguous():
        raise ValueError("hist: a contiguous int32 tensor [2, 272]")
    rc = _jpegcoef_lib.load().mdct_jpegcoef_stats(arr, len(planes), int(interleaved), hist.data_ptr(), unrepresentable.data_ptr(), _stream(stream))
    if check and rc != 0:
        raise _error(rc)
    return (hist, unrepresentable) if check else (rc, hist, unrepresentable)


def coef_rows(plane, specs, out, seg_bytes, ff_counts, uncoded, unrepresentable, grid=None, seg_stride=None, by0=0, by1=None, stream=None, check=True):
    """mdct_jpegcoef_rows on device tensors: one int16 coefficient plane -> one segment per block row, coded with specs = (DC (bits16,
    vals), AC (bits16, vals)).  grid: (blocks_x, blocks_y) to code (default: the whole tensor).  uncoded / unrepresentable: int32
    device tensors of one element that the caller has zeroed.  Otherwise as jpeg_encode.opt_rows."""
    p = _plane(plane, *(grid or (None, None)))
    sp = _Specs({0: specs[0], 1: specs[1]}, (0, 1))
    if seg_stride is None:
        seg_stride = opt_seg_stride(p.blocks_x)
    rc = _jpegcoef_lib.load().mdct_jpegcoef_rows(p, by0, p.blocks_y if by1 is None else by1, sp.arr[0], sp.arr[1], out.data_ptr(), seg_stride, seg_bytes.data_ptr(),
                                                 ff_counts.data_ptr(), uncoded.data_ptr(), unrepresentable.data_ptr(), _stream(stream))
    if check and rc != 0:
        raise _error(rc)
    return rc


def coef_scan_rows(planes, sampling, specs, out, seg_bytes, ff_counts, uncoded, unrepresentable, seg_stride=None, my0=0, my1=None, stream=None, check=True):
    """mdct_jpegcoef_scan_rows on device tensors: three int16 coefficient planes on one MCU grid -> one segment per MCU row of the
    interleaved scan, coded with specs = {which: (bits16, vals)} keyed like api.huffman_spec.  Otherwise as jpeg_encode.opt_scan_rows."""
    arr = _plane_array(planes, sampling)
    sp = _Specs(specs, (0, 1, 2, 3))
    mcus_x, mcus_y = planes[-1].shape[1] // 8, planes[-1].shape[0] // 8
    if seg_stride is None:
        seg_stride = opt_seg_stride(mcus_x * sum(h * v for h, v in sampling))
    rc = _jpegcoef_lib.load().mdct_jpegcoef_scan_rows(arr, len(planes), sp.arr, my0, mcus_y if my1 is None else my1, out.data_ptr(), seg_stride, seg_bytes.data_ptr(),
                                                      ff_counts.data_ptr(), uncoded.data_ptr(), unrepresentable.data_ptr(), _stream(stream))
    if check and rc != 0:
        raise _error(rc)
    return rc


def transform_planes(src, dst, op, stream=None, check=True):
    """mdct_jpegcoef_transform on device tensors: the blocks of src (int16 [blocks_y * 8, blocks_x * 8], any row pitch that is a
    multiple of 8) flipped, transposed or rotated into dst, which has the same shape or, for a transposing operation, the swapped one.
    op: one of TRANSFORMS."""
    if op not in _jpegcoef_lib.OPS:
        raise ValueError(f"transform {op!r} (one of {', '.join(TRANSFORMS)})")
    s, d = _plane(src, name="src"), _plane(dst, name="dst")
    rc = _jpegcoef_lib.load().mdct_jpegcoef_transform(s, d, _jpegcoef_lib.OPS[op], _stream(stream))
    if check and rc != 0:
        raise _error(rc)
    return rc


def _bools(optimize, interleaved):
    if not isinstance(optimize, (bool, np.bool_)):
        raise ValueError(f"optimize {optimize!r}: a bool")
    if not isinstance(interleaved, (bool, np.bool_)):
        raise ValueError(f"interleaved {interleaved!r}: a bool")


def _check_interleaved(sampling):
    if len(sampling) != 3 or tuple(sampling[0]) not in INTERLEAVED_LUMA or tuple(sampling[1]) != (1, 1) or tuple(sampling[2]) != (1, 1):
        raise ValueError(f"interleaved=True takes three components with sampling 4:4:4, 4:2:2 or 4:2:0 (luma (1, 1), (2, 1) or (2, 2), chroma (1, 1)), not {list(sampling)}")


def _pack(torch, seg, counts, stride, rows, pixels, dev, stream):
    """the packing launch into the small first buffer -> (out, off); the caller reads off[-1] and packs again if it did not fit"""
    with api._on_stream(stream, dev):
        out = torch.empty((_first_capacity(pixels),), dtype=torch.uint8, device=dev)
        off = torch.empty((rows + 1,), dtype=torch.int64, device=dev)
    api.jpeg_pack_rows(seg, counts[0], stride, rows, out, off, ff_counts=counts[1], stream=stream)
    return out, off


def encode_coefficients(coefs, qtables, width, height, sampling, *, colorspace=None, optimize=True, interleaved=False, progressive=False, bands=None, script=None, stream=None):
    """Quantised coefficient planes -> a baseline JPEG file (bytes), or with progressive=True a progressive one, without a DCT.

    coefs: 1 or 3 int16 device tensors [rows, columns], each padded to the MCU grid of the frame (jpeg_encode.mcu_grid), in the layout
    decode_jpeg(..., coefficients=True) returns; rows 16-byte aligned.  qtables: one table per component, 64 integers 1..255 in natural
    order (they are written, not applied).  width, height: the image size; sampling: [(h, v)] per component.  colorspace: None, 'grey',
    'YCbCr' or 'RGB' (jfif.write_jpeg).  Arguments are checked before any device work.

    One scan is written per component over its own block grid ceil(true size / 8) (T.81 A.2.2) with DRI = blocks per row; with
    interleaved=True (three components, 4:4:4, 4:2:2 or 4:2:0) one scan in MCU order with DRI = MCUs per row, which codes the padding
    blocks of the MCU grid as they are.  optimize=True: one statistics launch, the tables made for these coefficients
    (jpeg_encode.optimal_tables); False: the Annex K specifications.  Both go through the same coder (coef_rows / coef_scan_rows), then
    the packing launch, a small first buffer and a second packing into the worst case where that did not fit, as encode_jpeg.
    A coefficient that a baseline scan cannot hold (AC outside +-1023, DC difference outside +-2047) raises api.MdctError: no file is
    returned.  With optimize=True that is known from the statistics launch, before anything is coded.

    progressive=True (a bool): a SOF2 file with spectral selection (T.81 Annex G, Ah = Al = 0; jpeg_progressive, DESIGN.md section
    4.12): the DC scan, then per component the scans of its AC bands with end-of-band runs, every scan with a restart interval per row
    and its own table.  optimize must be True (the Annex K tables have no codes for the end-of-band runs: ValueError).  interleaved
    selects the form of the DC scan only: True one interleaved DC scan (the samplings above), False one per component.  bands: per
    component a list of (ss, se) that tiles 1..63 in order (default: luma (1, 2), (3, 9), (10, 63), chroma (1, 63); grey as luma; anything
    else is a ValueError); without progressive it must be None.  All statistics launches run first and one copy brings every histogram
    and the loss count back; then all coding and packing launches, and one copy of the lengths.  jpeg_decode reads these files back
    (jfif.read_progressive_jpeg, libmdct_jpegdec_prog.so).
    script (with progressive=True, instead of bands): None is the output above, byte for byte.  'standard' is libjpeg's standard script
    with successive approximation (jpeg_progressive.standard_script: what Pillow's progressive=True and jpegtran -progressive write;
    DESIGN.md section 4.12.1); a list of (components, ss, se, ah, al) is any script jpeg_progressive.check_script accepts (ValueError
    naming the scan otherwise).  The scans' component lists decide which DC scans are interleaved (`interleaved` is not consulted); a
    scan of all three components takes the samplings above.  Every scan keeps a restart interval per row of its own grid, a DC
    refinement scan has no table and no statistics launch.  script without progressive=True, or together with bands: ValueError."""
    import torch

    _bools(optimize, interleaved)
    if not isinstance(progressive, (bool, np.bool_)):
        raise ValueError(f"progressive {progressive!r}: a bool")
    if progressive and not optimize:
        raise ValueError("progressive=True needs optimize=True: the Annex K tables have no codes for end-of-band runs")
    if bands is not None and not progressive:
        raise ValueError("bands: only with progressive=True")
    if script is not None and not progressive:
        raise ValueError("script: only with progressive=True")
    sampling = [(int(h), int(v)) for h, v in sampling]
    nc = len(sampling)
    if nc not in (1, 3) or len(coefs) != nc or len(qtables) != nc:
        raise ValueError(f"{len(coefs)} planes, {len(qtables)} tables, {nc} sampling factors (1 or 3 of each)")
    if any(not (1 <= h <= 4 and 1 <= v <= 4) for h, v in sampling):
        raise ValueError(f"sampling factors {sampling} (1..4)")
    if not (1 <= width <= 65535 and 1 <= height <= 65535):
        raise ValueError(f"image {width}x{height}: 1..65535 each way")
    if interleaved:
        _check_interleaved(sampling)
    if progressive:
        from . import jpeg_progressive

        script = jpeg_progressive.resolve_script(script, bands, nc, bool(interleaved), sampling)
    tabs = []
    for k, q in enumerate(qtables):
        q = np.asarray(q).reshape(-1)
        if q.size != 64 or np.any(q != np.rint(q)) or q.min() < 1 or q.max() > 255:
            raise ValueError(f"quantisation table {k}: 64 integers 1..255")
        tabs.append([int(x) for x in q])
    mcus_x, mcus_y, padded = mcu_grid(width, height, sampling)
    for k, (p, (pw, ph)) in enumerate(zip(coefs, padded)):
        if not isinstance(p, torch.Tensor) or p.dtype != torch.int16 or not p.is_cuda or p.dim() != 2 or p.stride(1) != 1:
            raise ValueError(f"plane {k}: an int16 device tensor [rows, columns] with contiguous columns")
        if tuple(p.shape) != (ph, pw):
            raise ValueError(f"plane {k}: shape {list(p.shape)}, the MCU grid makes it [{ph}, {pw}]")
        if p.stride(0) % 8 or p.data_ptr() % 16:
            raise ValueError(f"plane {k}: rows must be 16-byte aligned")
    if progressive:
        from . import jpeg_progressive

        return jpeg_progressive.encode(torch, coefs, tabs, width, height, sampling, mcus_x, mcus_y, colorspace, script, stream)
    grey = nc == 1
    dev = coefs[0].device
    with torch.cuda.device(dev), api._on_stream(stream, dev):
        if interleaved:
            grids = None
            rows = [mcus_y]
            strides = [opt_seg_stride(mcus_x * sum(h * v for h, v in sampling))]
        else:
            grids = [(pw // 8, ph // 8) for _, _, pw, ph in component_sizes(width, height, sampling)]
            rows = [by for _, by in grids]
            strides = [opt_seg_stride(bx) for bx, _ in grids]
        # one int32 block: the histogram, then the words the kernels add to
        words = torch.zeros((2 * _jpegcoef_lib.HIST_CLASS + 2,), dtype=torch.int32, device=dev)
        hist, unrep, uncoded = words[:-2].view(2, _jpegcoef_lib.HIST_CLASS), words[-2:-1], words[-1:]
        if optimize:
            coef_histogram(coefs, sampling, interleaved=bool(interleaved), grids=grids, hist=hist, unrepresentable=unrep, stream=stream)
            w = words.cpu()  # the copy, on the call's stream, that waits for the histogram brings the loss count with it
            if int(w[-2]) != 0:
                raise api.MdctError(f"{int(w[-2])} coefficients cannot be written in a baseline scan (AC outside +-1023 or DC difference outside +-2047)")
            specs = optimal_tables(w[:-2].view(2, _jpegcoef_lib.HIST_CLASS), grey=grey)
        else:
            specs = {k: api.huffman_spec(k) for k in range(2 if grey else 4)}
        segs = [torch.empty((r * s,), dtype=torch.uint8, device=dev) for r, s in zip(rows, strides)]
        counts = [torch.empty((2, r), dtype=torch.int32, device=dev) for r in rows]
        if interleaved:
            coef_scan_rows(coefs, sampling, specs, segs[0], counts[0][0], counts[0][1], uncoded, unrep, seg_stride=strides[0], stream=stream)
            pixels = [sum(pw * ph for pw, ph in padded)]
        else:
            for k, p in enumerate(coefs):
                sp = (specs[2 if k else 0], specs[3 if k else 1])
                coef_rows(p, sp, segs[k], counts[k][0], counts[k][1], uncoded, unrep, grid=grids[k], seg_stride=strides[k], stream=stream)
            pixels = [bx * by * 64 for bx, by in grids]
        packed = [_pack(torch, s, c, st, r, px, dev, stream) for s, c, st, r, px in zip(segs, counts, strides, rows, pixels)]
        tail = torch.cat([off[-1:] for _, off in packed] + [words[-2:].to(torch.int64)]).cpu().tolist()  # the one copy that waits for the scans: it is ordered on the call's stream
        ends, lost, nocode = tail[:-2], tail[-2], tail[-1]
        if lost:
            raise api.MdctError(f"{lost} coefficients cannot be written in a baseline scan (AC outside +-1023 or DC difference outside +-2047)")
        if nocode:
            raise api.MdctError(f"{nocode} symbols of the scans have no code in the tables in use")
        scans = []
        for k, (out, off) in enumerate(packed):
            if ends[k] > out.numel():  # the segments are there: only the packing runs again, into the worst case
                out = torch.empty((2 * rows[k] * strides[k],), dtype=torch.uint8, device=dev)
                api.jpeg_pack_rows(segs[k], counts[k][0], strides[k], rows[k], out, off, ff_counts=counts[k][1], stream=stream)
                ends[k] = int(off[-1].item())
            scans.append(out[:ends[k]].cpu().numpy())
    kw = dict(specs=specs, sampling=sampling, table_per_component=True, colorspace=colorspace)
    if interleaved:
        return jfif.write_jpeg([dict(qtable=t) for t in tabs], width, height, interleaved=dict(scan=scans[0], mcus_per_row=mcus_x), **kw)
    return jfif.write_jpeg([dict(scan=s, blocks_per_row=bx, qtable=t) for s, (bx, _), t in zip(scans, grids, tabs)], width, height, **kw)


def plan_transform(width, height, sampling, transform, trim):
    """What a transform does to a frame, settled on the host: -> (source width and height after trimming, output width and height,
    output sampling).  A mirrored source axis (MIRRORED) must be a whole number of iMCUs, 8 * hmax samples for x and 8 * vmax for y:
    otherwise ValueError, or with trim=True the axis is cropped to whole iMCUs first (ValueError if none is left).  An axis that is
    not mirrored keeps its partial iMCU and its true size."""
    if transform is not None and transform not in MIRRORED:
        raise ValueError(f"transform {transform!r} (None or one of {', '.join(TRANSFORMS)})")
    if not isinstance(trim, (bool, np.bool_)):
        raise ValueError(f"trim {trim!r}: a bool")
    hmax, vmax = max(h for h, _ in sampling), max(v for _, v in sampling)
    size = {"x": width, "y": height}
    for axis, unit in (("x", 8 * hmax), ("y", 8 * vmax)):
        rem = size[axis] % unit
        if transform is None or axis not in MIRRORED[transform] or rem == 0:
            continue
        if not trim:
            raise ValueError(f"{transform} mirrors the {axis} axis, whose {size[axis]} samples leave a remainder of {rem} beyond whole iMCUs of {unit}: "
                             f"the transform is not perfect (trim=True crops the axis to {size[axis] - rem})")
        if size[axis] < unit:
            raise ValueError(f"{transform} with trim=True: the {axis} axis of {size[axis]} samples holds no whole iMCU of {unit}")
        size[axis] -= rem
    if transform in TRANSPOSING:
        return (size["x"], size["y"]), (size["y"], size["x"]), [(v, h) for h, v in sampling]
    return (size["x"], size["y"]), (size["x"], size["y"]), [(h, v) for h, v in sampling]


def transcode_jpeg(data, *, transform=None, trim=False, optimize=True, interleaved=False, progressive=False, script=None, device=None, stream=None):
    """Rewrite a baseline JPEG, or a progressive one decode_jpeg reads, without touching its coefficients (jpegtran):
    decode_coefficients, the optional transform, encode_coefficients.  Returns the new file as bytes.

    transform: None or 'flip_h', 'flip_v', 'transpose', 'transverse', 'rot90' (clockwise), 'rot180', 'rot270'.  A transposing operation
    swaps width and height and each component's (h, v), and transposes every quantisation table.  A source axis the operation mirrors
    (plan_transform) must be a whole number of iMCUs; trim=True crops it to whole iMCUs first (jpegtran -trim), trim=False raises
    ValueError naming the axis and the remainder.
    optimize=True: Huffman tables made for the file (9-14 % smaller than the Annex K tables); False: the Annex K tables.
    interleaved=False: one scan per component, a restart interval per block row; True: one interleaved scan, a restart interval per
    MCU row (three components with 4:4:4, 4:2:2 or 4:2:0 AFTER the transform: ValueError otherwise, before any device work).  Either way
    the output goes through the per-interval decoder ever after, whatever the input's scan form and restart interval were.
    progressive=True: the output is a progressive file with spectral selection (encode_coefficients: optimize must be True; interleaved
    selects the form of its DC scan).  script (with progressive=True only: ValueError otherwise): None, 'standard' -- libjpeg's standard
    script with successive approximation, the file jpegtran -progressive writes -- or a list, as encode_coefficients takes it.
    The quantisation tables (one per component, equal ones shared) and the colour space (grey, YCbCr, Adobe RGB) survive.
    Blocks of the padded planes beyond a component's own grid are zero after a non-interleaved input; an interleaved output codes them
    as they are -- they are invisible, which is not a loss.

    stream: None (torch's current stream), a torch.cuda.Stream or a raw hipStream_t.  All device work of the call -- the kernels of the
    decode, the transform and the coders, its own allocations, fills and uploads, and the copies of statuses, histograms, lengths and
    bytes that the host waits for -- is ordered on that stream (api._on_stream), whatever torch's current stream is.  The bytes returned
    are complete.  (encode_coefficients on its own: the planes it is given must be ready for `stream`.)

    Raises jfif.JpegFormatError / jpeg_decode.JpegDecodeError for the input exactly as decode_jpeg does, ValueError for the arguments,
    api.MdctError if a coefficient cannot be written in a baseline scan (a DC difference beyond +-2047 can arise where blocks become
    neighbours that were not).

    Out of scope: copying EXIF, ICC or comment segments (APPn and COM are dropped but for the colour-space markers); arithmetic-coded
    INPUT; jpegtran's default of leaving an unmirrored edge strip in place (here: perfect,
    trim, or an error); re-quantising (changing quality)."""
    import torch

    _bools(optimize, interleaved)
    if not isinstance(progressive, (bool, np.bool_)):
        raise ValueError(f"progressive {progressive!r}: a bool")
    if progressive and not optimize:
        raise ValueError("progressive=True needs optimize=True: the Annex K tables have no codes for end-of-band runs")
    if script is not None and not progressive:
        raise ValueError("script: only with progressive=True")
    if transform is not None and transform not in MIRRORED:
        raise ValueError(f"transform {transform!r} (None or one of {', '.join(TRANSFORMS)})")
    info = jpeg_decode.read_file(data)
    comps = info["components"]
    sampling = [(c["h"], c["v"]) for c in comps]
    (sw, sh), (ow, oh), osampling = plan_transform(info["width"], info["height"], sampling, transform, trim)
    if interleaved:
        _check_interleaved(osampling)
    qtables = [t.reshape(8, 8) for t in jpeg_decode.component_luts(info)]
    _, coefs = jpeg_decode.decode_coefficients(data, device, stream, info=info)
    # the source cropped to the trimmed size: fewer MCUs of the same planes
    hmax, vmax = max(h for h, _ in sampling), max(v for _, v in sampling)
    mx, my = _ceil(sw, 8 * hmax), _ceil(sh, 8 * vmax)
    coefs = [p[:my * v * 8, :mx * h * 8] for p, (h, v) in zip(coefs, sampling)]
    if transform is not None:
        with torch.cuda.device(coefs[0].device), api._on_stream(stream, coefs[0].device):
            moved = []
            for p in coefs:
                shape = (p.shape[1], p.shape[0]) if transform in TRANSPOSING else tuple(p.shape)
                d = torch.empty(shape, dtype=torch.int16, device=p.device)
                transform_planes(p, d, transform, stream=stream)
                moved.append(d)
        coefs = moved
        if transform in TRANSPOSING:
            qtables = [t.T for t in qtables]
    return encode_coefficients(coefs, [np.rint(t).astype(np.int64).reshape(64) for t in qtables], ow, oh, osampling, colorspace=info["colorspace"],
                               optimize=bool(optimize), interleaved=bool(interleaved), progressive=bool(progressive), script=script, stream=stream)
