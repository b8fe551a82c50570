"""Baseline and progressive (spectral selection, successive approximation) JPEG -> 8-bit planes on the GPU (libmdct_jpegdec.so,
include/mdct_jpegdec.h; libmdct_jpegdec_unmarked.so, include/mdct_jpegdec_unmarked.h; libmdct_jpegdec_prog.so,
include/mdct_jpegdec_prog.h).

decode_jpeg parses the file on the host (read_file: jfif.read_jpeg, or jfif_sof2.read_sof2_jpeg for a SOF2 file), uploads each scan
and decodes it into quantised int16 coefficient planes: a baseline scan with restart markers by finding its restart intervals
(mdct_jpegdec_index) and decoding them (mdct_jpegdec_decode), one without by mdct_jpegdec_decode_unmarked, a scan of a progressive
file by mdct_jpegdec_index (unless it has no restart markers: then it is one interval) and mdct_jpegdec_prog_decode_approx into its
band, and its bit, of the planes.  It checks every scan's status, and runs
mdct_inv_i16_u8_batch over the planes with each component's DQT as the table.  One uint8 plane per component, cropped to the
component's size (T.81 A.1.1).  With mode="RGB" the planes go through one more launch, mdct_jpegcolor_to_rgb
(libmdct_jpegcolor.so, include/mdct_jpegcolor.h): chroma upsampling and YCbCr -> RGB as libjpeg-turbo's default decode gives them.
With scale_denom = 2, 4 or 8 the picture comes out at 1/2, 1/4 or 1/8 size as libjpeg-turbo scales it (scaled_geometry): the scans are
decoded as ever, components whose blocks shrink go through mdct_jpegscale_inv_i16_u8 (libmdct_jpegscale.so,
include/mdct_jpegscale.h, loaded at the first such call) in place of the full inverse.
decode_jpeg_batch decodes many files in one call: the restart-marked baseline scans of all of them in four launches
(libmdct_jpegdec_batch.so, include/mdct_jpegdec_batch.h; BatchPlan), one inverse-DCT call over every plane, errors per file.
torch is used for device memory and streams only.
"""
import ctypes

import numpy as np

from . import _jpegcolor_lib, _jpegdec_batch_lib, _jpegdec_lib, _jpegdec_prog_lib, _jpegdec_unmarked_lib, api, jfif, jfif_sof2
from .api import _ptr, _stream


class JpegDecodeError(RuntimeError):
    """a scan that did not decode cleanly; .status holds that scan's per-interval MDCT_JPEGDEC_* codes (restart-marked scan) or
    [code, blocks decoded before the first error] (scan without restart markers)"""

    def __init__(self, msg, scan=None, status=None):
        super().__init__(msg)
        self.scan = scan
        self.status = status


STATUS_NAMES = _jpegdec_prog_lib.STATUS_NAMES  # every interval status a restart-marked or progressive scan can end in


last_error, _check = _jpegdec_lib.LIB.last_error, _jpegdec_lib.LIB.check


def _spec_arrays(specs):
    """specs: 4 x (bits16, vals) or None -> the three C arrays of mdct_jpegdec_tables_create (and the buffers they point into)"""
    keep = []
    bits_p = (ctypes.c_void_p * 4)()
    vals_p = (ctypes.c_void_p * 4)()
    nv = (ctypes.c_int * 4)()
    for i, sp in enumerate(specs):
        if sp is None:
            continue
        b = np.ascontiguousarray(np.asarray(sp[0], dtype=np.uint8).reshape(16))
        v = np.ascontiguousarray(np.asarray(sp[1], dtype=np.uint8).reshape(-1)) if len(sp[1]) else np.zeros(1, dtype=np.uint8)
        keep += [b, v]
        bits_p[i] = b.ctypes.data
        vals_p[i] = v.ctypes.data
        nv[i] = len(sp[1])
    return bits_p, vals_p, nv, keep


def tables_check(specs):
    """mdct_jpegdec_tables_check (host only): 0 or MDCT_INVALID_PARAMETER"""
    b, v, n, keep = _spec_arrays(specs)
    return _jpegdec_lib.load().mdct_jpegdec_tables_check(b, v, n)


class Tables:
    """device-resident Huffman tables (mdct_jpegdec_tables_*): specs = 4 x (bits16, vals) or None -- slots 0, 1 DC; 2, 3 AC"""

    def __init__(self, specs):
        lib = _jpegdec_lib.load()
        b, v, n, keep = _spec_arrays(specs)
        h = ctypes.c_void_p()
        _check(lib.mdct_jpegdec_tables_create(ctypes.byref(h), b, v, n))
        self.handle = h

    def close(self):
        if self.handle:
            _jpegdec_lib.load().mdct_jpegdec_tables_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def scan_desc(planes, mcus_x, mcus_y, restart_interval):
    """planes: list of (coef int16 tensor [rows, pitch], blocks_x, blocks_y, h, v, dc_slot, ac_slot) -> mdct_jpegdec_scan"""
    d = _jpegdec_lib.Scan()
    d.n_components = len(planes)
    for c, (t, bx, by, h, v, dc, ac) in enumerate(planes):
        d.comp[c] = _jpegdec_lib.Component(_ptr(t), t.shape[-1], bx, by, h, v, dc, ac)
    d.mcus_x, d.mcus_y, d.restart_interval = mcus_x, mcus_y, restart_interval
    return d


def n_intervals(desc):
    n = int(_jpegdec_lib.load().mdct_jpegdec_intervals(ctypes.byref(desc)))
    if n == 0:
        raise api.MdctError(f"invalid scan descriptor: {last_error()}")
    return n


def index(scan, n, offsets, status, scan_len=None, stream=None):
    """mdct_jpegdec_index: offsets = n + 1 int64 device tensor, status = n int32 device tensor (scratch)"""
    L = scan.numel() if scan_len is None else scan_len
    _check(_jpegdec_lib.load().mdct_jpegdec_index(_ptr(scan), L, n, _ptr(offsets), _ptr(status), _stream(stream)))


def decode(desc, tables, scan, offsets, status, scan_len=None, stream=None):
    """mdct_jpegdec_decode"""
    L = scan.numel() if scan_len is None else scan_len
    _check(_jpegdec_lib.load().mdct_jpegdec_decode(ctypes.byref(desc), tables.handle, _ptr(scan), L, _ptr(offsets), _ptr(status), _stream(stream)))


unmarked_last_error = _jpegdec_unmarked_lib.LIB.last_error


def unmarked_workspace(desc, scan_len):
    """mdct_jpegdec_unmarked_workspace (host only): bytes of device workspace, 0 for a descriptor the unmarked path refuses"""
    return int(_jpegdec_unmarked_lib.load().mdct_jpegdec_unmarked_workspace(ctypes.byref(desc), scan_len))


def decode_unmarked(desc, tables, scan, workspace, status, scan_len=None, sync_rounds=4, stream=None):
    """mdct_jpegdec_decode_unmarked: workspace = device tensor of at least unmarked_workspace() bytes, status = 2 int32 device tensor"""
    L = scan.numel() if scan_len is None else scan_len
    rc = _jpegdec_unmarked_lib.load().mdct_jpegdec_decode_unmarked(ctypes.byref(desc), tables.handle, _ptr(scan), L, _ptr(workspace),
                                                                   workspace.numel() * workspace.element_size(), _ptr(status),
                                                                   sync_rounds, _stream(stream))
    _jpegdec_unmarked_lib.LIB.check(rc)  # (reported under the label mdct_jpegdec)


prog_last_error = _jpegdec_prog_lib.LIB.last_error


def prog_intervals(desc, ss, se):
    """mdct_jpegdec_prog_intervals (host only): the scan's restart intervals; MdctError for a descriptor or band the library refuses"""
    n = int(_jpegdec_prog_lib.load().mdct_jpegdec_prog_intervals(ctypes.byref(desc), ss, se))
    if n == 0:
        raise api.MdctError(f"invalid scan descriptor: {prog_last_error()}")
    return n


def decode_prog(desc, ss, se, tables, scan, offsets, status, scan_len=None, stream=None, *, ah=0, al=0):
    """mdct_jpegdec_prog_decode_approx: one scan of a progressive file, band ss..se, successive approximation ah / al; offsets as
    index() leaves them, or [0, scan_len] for a scan without restart markers handed over as one interval (markerless_desc).
    tables: None for a DC refinement scan, which reads no table"""
    L = scan.numel() if scan_len is None else scan_len
    lib = _jpegdec_prog_lib.load()
    _jpegdec_prog_lib.LIB.check(lib.mdct_jpegdec_prog_decode_approx(ctypes.byref(desc), ss, se, ah, al, None if tables is None else tables.handle,
                                                                    _ptr(scan), L, _ptr(offsets), _ptr(status), _stream(stream)))


def read_file(data):
    """the parser the file's frame header asks for: jfif_sof2.read_sof2_jpeg for SOF2, jfif.read_jpeg(require_restart=False) for
    everything else (which refuses what it always refused)"""
    if jfif.sof_marker(data) == 0xC2:
        return jfif_sof2.read_sof2_jpeg(data)
    return jfif.read_jpeg(data, require_restart=False)


def _ceil(a, b):
    return -(-a // b)


def geometry(info):
    """per component of read_jpeg's frame: (true width, true height, plane blocks_x, plane blocks_y), planes padded to the MCU grid"""
    comps = info["components"]
    hmax, vmax = max(c["h"] for c in comps), max(c["v"] for c in comps)
    mx, my = _ceil(info["width"], 8 * hmax), _ceil(info["height"], 8 * vmax)
    return [(_ceil(info["width"] * c["h"], hmax), _ceil(info["height"] * c["v"], vmax), mx * c["h"], my * c["v"]) for c in comps], (mx, my)


def scan_geometry(info, scan, geo, grid):
    """(mcus_x, mcus_y, [(component index, h, v)]) of one scan: T.81 A.2.2 (one component: its own block grid) / A.2.3"""
    if len(scan["components"]) == 1:
        ci = scan["components"][0]["index"]
        w, h = geo[ci][0], geo[ci][1]
        return _ceil(w, 8), _ceil(h, 8), [(ci, 1, 1)]
    comps = info["components"]
    return grid[0], grid[1], [(c["index"], comps[c["index"]]["h"], comps[c["index"]]["v"]) for c in scan["components"]]


def scan_plan(info, si, sc, geo, grid, coefs):
    """Everything decode_jpeg settles about scan si on the host before its first launch: the Huffman specifications the scan names
    (JpegFormatError for one that is not defined), their validation (tables_check) and the descriptor over the coefficient planes,
    which the library it goes to must accept (MdctError).  coefs: one int16 tensor per component, [rows, blocks_x * 8].
    A scan of a progressive file (one with 'ss' / 'se') names only the tables of its band's class: DC for 0..0, AC for an AC band,
    none for a DC refinement scan (Ah > 0), which is raw bits.  One without restart markers is described as ONE restart interval
    (restart_interval = mcus_x * mcus_y: the library has no other way to take it, and decode_scan writes its two offsets itself).
    -> (specs, desc)"""
    mcus_x, mcus_y, members = scan_geometry(info, sc, geo, grid)
    specs = [None] * 4
    planes = []
    band = (sc["ss"], sc["se"]) if "ss" in sc else None
    for c, (ci, h, v) in zip(sc["components"], members):
        dc, ac = (c["td"], (0, c["td"])), (2 + c["ta"], (1, c["ta"]))
        for slot, key in (dc, ac) if band is None else (ac,) if band != (0, 0) else (dc,) if sc.get("ah", 0) == 0 else ():
            if key not in sc["huffman"]:
                raise jfif.JpegFormatError(f"scan {si} uses Huffman table {key} that is not defined")
            specs[slot] = sc["huffman"][key]
        planes.append((coefs[ci], geo[ci][2], geo[ci][3], h, v, c["td"], 2 + c["ta"]))
    if tables_check(specs) != 0:
        raise api.MdctError(f"scan {si}: {last_error()}")
    desc = scan_desc(planes, mcus_x, mcus_y, sc["restart_interval"] or mcus_x * mcus_y if band is not None else sc["restart_interval"])
    if band is not None:
        if band == (0, 0) and sc.get("ah", 0):  # the slot no table stands behind is still checked for its range
            for c in range(desc.n_components):
                desc.comp[c].dc_slot = 0
        prog_intervals(desc, *band)
    elif sc["restart_interval"]:
        n_intervals(desc)
    elif unmarked_workspace(desc, sc["end"] - sc["start"]) == 0:
        raise api.MdctError(f"invalid scan descriptor: {unmarked_last_error()}")
    return specs, desc


def component_luts(info):
    """the quantisation table of every component as float32 [64]; JpegFormatError for one that is not defined"""
    luts = []
    for c in info["components"]:
        if c["tq"] not in info["qtables"]:
            raise jfif.JpegFormatError(f"quantisation table {c['tq']} is not defined")
        luts.append(info["qtables"][c["tq"]].astype(np.float32))
    return luts


SCALE_DENOMS = (1, 2, 4, 8)


def scaled_geometry(info, scale_denom):
    """libjpeg-turbo's geometry of a decode at 1 / scale_denom (1, 2, 4, 8), from read_jpeg's frame; pure Python.  With m = 8 / scale_denom
    a component of sampling (h, v) decodes its blocks to s x s samples: s starts at m and doubles while s < 8 and
    (hmax * m) % (h * s * 2) == 0 and (vmax * m) % (v * s * 2) == 0 (a subsampled component keeps more of its own resolution rather than
    being upsampled afterwards).  -> ([(s, true width, true height, effective h, effective v)] per component, (image width, image
    height)): the component is ceil(W * h * s / (hmax * 8)) x ceil(H * v * s / (vmax * 8)), the image ceil(W * m / 8) x
    ceil(H * m / 8), and (h * s / m, v * s / m) are the sampling factors the colour stage sees."""
    if scale_denom not in SCALE_DENOMS:
        raise ValueError(f"scale_denom {scale_denom!r} (1, 2, 4 or 8)")
    m = 8 // scale_denom
    comps = info["components"]
    W, H = info["width"], info["height"]
    hmax, vmax = max(c["h"] for c in comps), max(c["v"] for c in comps)
    out = []
    for c in comps:
        h, v, s = c["h"], c["v"], m
        while s < 8 and (hmax * m) % (h * s * 2) == 0 and (vmax * m) % (v * s * 2) == 0:
            s *= 2
        out.append((s, _ceil(W * h * s, hmax * 8), _ceil(H * v * s, vmax * 8), h * s // m, v * s // m))
    return out, (_ceil(W * m, 8), _ceil(H * m, 8))


def scaled_last_error():
    from . import _jpegscale_lib

    return _jpegscale_lib.LIB.last_error()


def scaled_inverse(planes, level_shift=True, stream=None):
    """mdct_jpegscale_inv_i16_u8, one launch: planes = 1..4 of (px uint8 [blocks_y * n, blocks_x * n] device tensor, coef int16
    [blocks_y * 8, blocks_x * 8] device tensor, blocks_x, blocks_y, lut (64 floats, natural order) or None, n = 4, 2 or 1[, (rep_x,
    rep_y): n = 1 only, every sample written rep_x x rep_y times into px [blocks_y * rep_y, blocks_x * rep_x]]); rows of either tensor
    may lie any pitch apart, columns must be contiguous"""
    from . import _jpegscale_lib

    lib = _jpegscale_lib.load()
    arr = (_jpegscale_lib.Plane * max(1, len(planes)))()
    keep = []
    for k, (px, coef, bx, by, lut, n, *more) in enumerate(planes):
        rx, ry = more[0] if more else (1, 1)
        if px.dim() != 2 or coef.dim() != 2 or px.stride(1) != 1 or coef.stride(1) != 1:
            raise ValueError(f"plane {k}: [rows, columns] tensors with contiguous columns")
        if lut is not None:
            lut = api._lut64(lut)
            keep.append(lut)
        arr[k] = _jpegscale_lib.Plane(_ptr(coef), coef.stride(0), _ptr(px), px.stride(0), bx, by, None if lut is None else lut.ctypes.data, n, rx, ry)
    _jpegscale_lib.LIB.check(lib.mdct_jpegscale_inv_i16_u8(arr, len(planes), int(bool(level_shift)), _stream(stream)))


def colour_sampling(info, scale_denom):
    """the sampling factors the colour stage is given after a decode at 1 / scale_denom, and the replication (rep_x, rep_y) each
    component gets before it.  Up to 1/4 these are scaled_geometry's effective factors and no replication.  At 1/8 libjpeg-turbo
    switches its triangle ("fancy") filters off (jdsample.c: only while the smallest block is larger than one sample) and upsamples
    by plain replication: a component that still needs upsampling there is written replicated to the image's size by the scaled
    inverse and then enters the colour stage at the largest factors.  -> ([(h, v)], [(rep_x, rep_y)])"""
    sgeo, _ = scaled_geometry(info, scale_denom)
    eff = [(g[3], g[4]) for g in sgeo]
    hmax, vmax = max(h for h, _ in eff), max(v for _, v in eff)
    if scale_denom != 8 or any(hmax % h or vmax % v for h, v in eff):
        return eff, [(1, 1)] * len(eff)
    reps = [(hmax // h, vmax // v) for h, v in eff]
    for g, r in zip(sgeo, reps):
        if r != (1, 1) and g[0] != 1:
            raise jfif.JpegFormatError(f"no RGB at 1/8 for sampling factors {[(c['h'], c['v']) for c in info['components']]}")
    return [(hmax, vmax) if r != (1, 1) else e for e, r in zip(eff, reps)], reps


def scaled_planes(info, coefs, scale_denom, stream=None, replicate=False):
    """the inverse stage of a decode at 1 / scale_denom (2, 4, 8): read_jpeg's frame and its quantised coefficient planes (device int16,
    padded to the MCU grid, as geometry() sizes them) -> one uint8 plane per component, cropped to its scaled true size.  Components
    that keep 8 x 8 blocks take mdct_inv_i16_u8_batch, the others one mdct_jpegscale_inv_i16_u8 call.  replicate=True: the planes
    as the colour stage takes them (colour_sampling): at 1/8 a component that needs upsampling comes replicated, cropped to the image."""
    import torch

    geo, _ = geometry(info)
    sgeo, (sw, sh) = scaled_geometry(info, scale_denom)
    reps = colour_sampling(info, scale_denom)[1] if replicate else [(1, 1)] * len(sgeo)
    luts = component_luts(info)
    with api._on_stream(stream, coefs[0].device):
        px = [torch.empty((g[3] * sg[0] * r[1], g[2] * sg[0] * r[0]), dtype=torch.uint8, device=q.device) for g, sg, q, r in zip(geo, sgeo, coefs, reps)]
        full = [(p, q, g[2] * 8, g[3] * 8, lut) for p, q, g, sg, lut in zip(px, coefs, geo, sgeo, luts) if sg[0] == 8]
        small = [(p, q, g[2], g[3], lut, sg[0], r) for p, q, g, sg, lut, r in zip(px, coefs, geo, sgeo, luts, reps) if sg[0] != 8]
        if full:
            api.u8_i16_batch("inv", full, level_shift=True, stream=stream)
        if small:
            scaled_inverse(small, level_shift=True, stream=stream)
    return [p[:sg[2], :sg[1]] if r == (1, 1) else p[:sh, :sw] for p, sg, r in zip(px, sgeo, reps)]


def decode_coefficients(data, device=None, stream=None, *, info=None):
    """The front of decode_jpeg on its own: parse the file (read_file), plan and entropy-decode every scan on the GPU.  No inverse
    DCT runs.  -> (info, coefs): the reader's dict and one quantised int16 coefficient plane per component on the device,
    [blocks_y * 8, blocks_x * 8], padded to the MCU grid (geometry), not dequantised.  info: read_file(data) if the caller has parsed
    the file already.  The scans of a progressive file each fill their band of the same planes; a band no scan codes stays zero.
    Raises as decode_jpeg does: jfif.JpegFormatError for a file outside the supported subset, JpegDecodeError when a scan does not
    decode cleanly."""
    import torch

    if info is None:
        info = read_file(data)
    dev = api._device(device)
    raw = bytes(data)
    geo, grid = geometry(info)
    # zeroed: a non-interleaved scan of a subsampled component covers its own block grid (T.81 A.2.2), which may be smaller than the
    # plane padded to the MCU grid; and a progressive scan stores non-zero levels only, into a band that must be zero
    with torch.cuda.device(dev), api._on_stream(stream, dev):
        coefs = [torch.zeros((by * 8, bx * 8), dtype=torch.int16, device=dev) for _, _, bx, by in geo]
        for si, sc in enumerate(info["scans"]):
            specs, desc = scan_plan(info, si, sc, geo, grid, coefs)
            tables = Tables(specs) if any(sp is not None for sp in specs) else None  # (a DC refinement scan reads no table)
            seg = torch.frombuffer(bytearray(raw[sc["start"]:sc["end"]]) or bytearray(1), dtype=torch.uint8).to(dev, non_blocking=False)
            try:
                decode_scan(torch, si, sc, desc, tables, seg, dev, stream)
            finally:
                if tables is not None:
                    tables.close()
    return info, coefs


def decode_jpeg(data, device=None, coefficients=False, stream=None, *, mode=None, layout="HWC", scale_denom=1):
    """Decode a baseline JPEG on the GPU, with or without restart markers (scans of both kinds may share a file), or a progressive
    Huffman one (jfif_sof2.read_sof2_jpeg: spectral selection and successive approximation, with or without restart markers -- what
    encode_jpeg(progressive=True) writes and what libjpeg's standard scan script, Pillow's progressive=True, writes; AC refinement scans
    are decoded sequentially inside a restart interval and a scan without markers is one interval: correct, not fast).  Returns one uint8
    tensor [height, width] per component (cropped to its true size); with coefficients=True also the quantised int16 coefficient planes
    ([blocks_y * 8, blocks_x * 8], padded to the MCU grid): (planes, coefficient planes).
    mode="RGB" returns one uint8 image instead of the planes, [height, width, 3] (layout="HWC") or [3, height, width] (layout="CHW"),
    upsampled and converted as libjpeg-turbo's default decode does it (to_rgb); with coefficients=True: (image, coefficient planes).
    scale_denom = 2, 4 or 8 returns the planes or the image at 1/2, 1/4 or 1/8 size, ceil(width / scale_denom) x
    ceil(height / scale_denom), as libjpeg-turbo scales them (scaled_geometry; Pillow's draft): every block becomes the box mean of its
    IDCT, and a subsampled component keeps more of its own samples before any upsampling (at 1/8 what upsampling is left is plain
    replication, as libjpeg-turbo does it: colour_sampling).  The coefficient planes stay the full ones.
    The entropy decode, which is most of a decode's time, is the same at every scale: the scaled picture saves memory, not much time.
    stream: None (torch's current stream), a torch.cuda.Stream or a raw hipStream_t.  All device work of the call -- its kernels, its own
    allocations, fills and uploads, and the copies of the scans' statuses that the host waits for -- is ordered on that stream
    (api._on_stream), whatever torch's current stream is.  The returned device tensors are ready on `stream`, not necessarily on the
    caller's current stream: a consumer on another stream waits for `stream` first (wait_stream / an event).
    Raises jfif.JpegFormatError for a file outside the supported subset and JpegDecodeError when a scan does not decode cleanly."""
    import torch

    if scale_denom not in SCALE_DENOMS:
        raise ValueError(f"scale_denom {scale_denom!r} (1, 2, 4 or 8)")
    if mode not in (None, "RGB"):
        raise ValueError(f"mode {mode!r} (None or 'RGB')")
    if layout not in _LAYOUTS:
        raise ValueError(f"layout {layout!r} ('HWC' or 'CHW')")
    info = read_file(data)
    if mode == "RGB":
        _colour_params(info)
    dev = api._device(device)
    geo, _ = geometry(info)
    _, coefs = decode_coefficients(data, dev, stream, info=info)
    with torch.cuda.device(dev), api._on_stream(stream, dev):
        if scale_denom != 1:
            out = scaled_planes(info, coefs, scale_denom, stream=stream, replicate=mode == "RGB")
            if mode == "RGB":
                sw, sh = scaled_geometry(info, scale_denom)[1]
                out = to_rgb(out, colour_sampling(info, scale_denom)[0], sw, sh, colour=info["colorspace"], layout=layout, stream=stream)
            return (out, coefs) if coefficients else out
        px = [torch.empty((by * 8, bx * 8), dtype=torch.uint8, device=dev) for _, _, bx, by in geo]
        luts = component_luts(info)
        api.u8_i16_batch("inv", [(p, q, g[2] * 8, g[3] * 8, lut) for p, q, g, lut in zip(px, coefs, geo, luts)], level_shift=True, stream=stream)
        out = [p[:g[1], :g[0]] for p, g in zip(px, geo)]
        if mode == "RGB":
            out = to_rgb(out, [(c["h"], c["v"]) for c in info["components"]], info["width"], info["height"], colour=info["colorspace"],
                         layout=layout, stream=stream)
    return (out, coefs) if coefficients else out


batch_last_error = _jpegdec_batch_lib.LIB.last_error


class BatchPlan:
    """mdct_jpegdec_batch_plan: the host's plan of a batch of restart-marked baseline scans (include/mdct_jpegdec_batch.h); no device
    is needed to make one.  scans: list of (desc, byte_offset, byte_len, specs) -- desc as scan_desc() builds it, the scan's bytes at
    [byte_offset, byte_offset + byte_len) of the batch's byte buffer of total_bytes, specs = 4 x (bits16, vals) or None.
    MdctError (.scan: the scan refused, None for the batch as a whole) with the single-scan library's message for what it refuses."""

    def __init__(self, scans, total_bytes):
        lib = _jpegdec_batch_lib.load()
        arr = (_jpegdec_batch_lib.BatchScan * max(1, len(scans)))()
        keep = []
        for i, (desc, off, length, specs) in enumerate(scans):
            b, v, n, k = _spec_arrays(specs)
            keep.append(k)
            arr[i].desc, arr[i].byte_offset, arr[i].byte_len = desc, off, length
            for t in range(4):
                arr[i].bits16[t], arr[i].vals[t], arr[i].nvals[t] = b[t], v[t], n[t]
        h, bad = ctypes.c_void_p(), ctypes.c_size_t()
        rc = lib.mdct_jpegdec_batch_plan_create(ctypes.byref(h), arr, len(scans), total_bytes, ctypes.byref(bad))
        if rc != 0:
            e = _jpegdec_batch_lib.LIB.error(rc)
            e.scan = bad.value if bad.value < len(scans) else None
            raise e
        self.handle, self._lib = h, lib
        self.n_scans = int(lib.mdct_jpegdec_batch_scans(h))
        self.n_intervals = int(lib.mdct_jpegdec_batch_intervals(h))
        self.n_offsets = int(lib.mdct_jpegdec_batch_offsets(h))
        self.n_chunks = int(lib.mdct_jpegdec_batch_chunks(h))
        self.n_table_sets = int(lib.mdct_jpegdec_batch_table_sets(h))
        self.image_bytes = int(lib.mdct_jpegdec_batch_image_bytes(h))
        self.first_interval = [int(lib.mdct_jpegdec_batch_first_interval(h, i)) for i in range(self.n_scans + 1)]

    @property
    def first_chunk(self):
        """the prefix of the scans' index chunk counts"""
        return [int(self._lib.mdct_jpegdec_batch_first_chunk(self.handle, i)) for i in range(self.n_scans + 1)]

    @property
    def chunk_bytes(self):
        """the chunk size mdct_jpegdec_index cuts each scan by"""
        return [int(self._lib.mdct_jpegdec_batch_chunk_bytes(self.handle, i)) for i in range(self.n_scans)]

    @property
    def table_set(self):
        """the table set of each scan"""
        return [int(self._lib.mdct_jpegdec_batch_table_set(self.handle, i)) for i in range(self.n_scans)]

    def chunk_scan(self):
        """the chunk table: the scan every index chunk of the batch belongs to"""
        return [int(self._lib.mdct_jpegdec_batch_chunk_scan(self.handle, c)) for c in range(self.n_chunks)]

    _rc = staticmethod(_jpegdec_batch_lib.LIB.check)

    def bind(self, device_image, scan_bytes, offsets, status):
        """mdct_jpegdec_batch_bind: -> the image as a numpy uint8 array, to be copied to device_image (a device tensor of image_bytes
        bytes) before the first launch.  offsets: n_offsets int64, status: n_intervals int32 device tensors."""
        host = np.zeros(self.image_bytes, dtype=np.uint8)
        self._rc(self._lib.mdct_jpegdec_batch_bind(self.handle, host.ctypes.data, _ptr(device_image), _ptr(scan_bytes), _ptr(offsets), _ptr(status)))
        return host

    def index(self, stream=None):
        """mdct_jpegdec_batch_index: three launches"""
        self._rc(self._lib.mdct_jpegdec_batch_index(self.handle, _stream(stream)))

    def decode(self, stream=None):
        """mdct_jpegdec_batch_decode: one launch"""
        self._rc(self._lib.mdct_jpegdec_batch_decode(self.handle, _stream(stream)))

    def close(self):
        if self.handle:
            self._lib.mdct_jpegdec_batch_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _PlaneShape:
    """stands for a coefficient plane that is not allocated yet where scan_plan only looks at a plane's address and pitch"""

    def __init__(self, rows, cols, address=256):
        self.shape, self._address = (rows, cols), address

    def data_ptr(self):
        return self._address


_ON_ERROR = ("raise", "return")
_ARENA_ALIGN = 256  # bytes between the starts of two planes of an arena, at least


def decode_jpeg_batch(files, device=None, stream=None, *, mode=None, layout="HWC", coefficients=False, on_error="raise"):
    """Decode a sequence of JPEG files (bytes) on the GPU: a list with one entry per file, each exactly what decode_jpeg(file, device,
    coefficients, stream, mode=mode, layout=layout) returns.  Accepts whatever decode_jpeg accepts (scale_denom excepted).
    Files whose every scan is baseline with restart markers take the batch path (libmdct_jpegdec_batch.so,
    include/mdct_jpegdec_batch.h): every file is parsed and every scan planned on the host first; then one upload of all scans' bytes,
    one of the scan records and Huffman table sets (equal tables stored once), one zeroed int16 arena for all coefficient planes and one
    uint8 arena for all pixel planes, four launches for the entropy stage of the whole batch (three index passes, one decode with a
    workgroup per restart interval), ONE copy of all interval statuses to the host, and one api.u8_i16_batch("inv", ...) over the
    planes of all files that decoded cleanly.  mode="RGB" then converts file by file (to_rgb): a batched colour kernel is out of scope.
    The tensors one call returns for batch-path files are views of those arenas: they share storage, and keeping one keeps the
    arena of the whole batch alive.  A file with a scan without restart markers, or a progressive file, goes through decode_jpeg on
    its own inside the call, on the same stream.
    Errors are per file and never change another file's output.  on_error="raise": the exception of the lowest-numbered failing file
    is raised, of the type and with the message decode_jpeg gives for that file alone (jfif.JpegFormatError; JpegDecodeError with .scan
    and .status; api.MdctError), with the added attribute .file, the file's index.  on_error="return": that exception object stands in
    the file's slot, every other file is decoded.  An empty sequence returns [] without touching the device.
    stream: as for decode_jpeg -- every launch, allocation, fill, upload and the status copy of the call is ordered on it."""
    if mode not in (None, "RGB"):
        raise ValueError(f"mode {mode!r} (None or 'RGB')")
    if layout not in _LAYOUTS:
        raise ValueError(f"layout {layout!r} ('HWC' or 'CHW')")
    if on_error not in _ON_ERROR:
        raise ValueError(f"on_error {on_error!r} ('raise' or 'return')")
    files = list(files)
    if not files:
        return []
    results = [None] * len(files)

    def failed(i, e):
        e.file = i
        results[i] = e

    # ---- host: parse every file, plan every scan (against planes that stand for the arena's)
    # batch path: (file index, info, geo, [(int16 arena element, uint8 arena byte) every plane starts at], [(specs, desc) per scan])
    jobs, singles = [], []
    n_coef = n_px = 0
    for i, data in enumerate(files):
        try:
            info = read_file(data)
            if mode == "RGB":
                _colour_params(info)
            if info["sof"] == 0xC2 or any(sc["restart_interval"] == 0 for sc in info["scans"]):
                singles.append(i)
                continue
            geo, grid = geometry(info)
            stand_in = [_PlaneShape(by * 8, bx * 8) for _, _, bx, by in geo]
            plans = [scan_plan(info, si, sc, geo, grid, stand_in) for si, sc in enumerate(info["scans"])]
        except (jfif.JpegFormatError, api.MdctError) as e:
            failed(i, e)
            continue
        at = []
        for _, _, bx, by in geo:
            at.append((n_coef, n_px))
            n_coef += _ceil(by * bx * 64 * 2, _ARENA_ALIGN) * _ARENA_ALIGN // 2
            n_px += _ceil(by * bx * 64, _ARENA_ALIGN) * _ARENA_ALIGN
        jobs.append((i, info, geo, at, plans))
    if jobs or singles:
        import torch

        dev = api._device(device)
    # ---- files outside the batch path, one at a time
    for i in singles:
        try:
            results[i] = decode_jpeg(files[i], dev, coefficients, stream, mode=mode, layout=layout)
        except (jfif.JpegFormatError, JpegDecodeError, api.MdctError) as e:
            failed(i, e)
    if jobs:
        _decode_batch_path(torch, files, jobs, (n_coef, n_px), results, failed, dev, stream, mode, layout, coefficients)
    if on_error == "raise":
        for r in results:
            if isinstance(r, Exception):
                raise r  # the lowest-numbered failing file's, whichever stage found it
    return results


def _decode_batch_path(torch, files, jobs, arena, results, failed, dev, stream, mode, layout, coefficients):
    """the batch path of decode_jpeg_batch for the files `jobs` names (planned and found acceptable already; arena: the sizes of the two
    arenas their planes were placed in)"""
    with torch.cuda.device(dev), api._on_stream(stream, dev):
        n_coef, n_px = arena  # elements of the int16 arena, bytes of the uint8 one
        coef_arena = torch.zeros(n_coef, dtype=torch.int16, device=dev)
        px_arena = torch.empty(n_px, dtype=torch.uint8, device=dev)
        blob, coefs, pxs, scans, owner = bytearray(), {}, {}, [], []
        for i, info, geo, at, plans in jobs:
            coefs[i] = [coef_arena[c0:c0 + by * bx * 64].view(by * 8, bx * 8) for (c0, _), (_, _, bx, by) in zip(at, geo)]
            pxs[i] = [px_arena[p0:p0 + by * bx * 64].view(by * 8, bx * 8) for (_, p0), (_, _, bx, by) in zip(at, geo)]
            raw = bytes(files[i])
            for si, (sc, (specs, desc)) in enumerate(zip(info["scans"], plans)):
                for c, member in enumerate(sc["components"]):  # the planes the descriptor was checked against, now where they are
                    desc.comp[c].coef = _ptr(coefs[i][member["index"]])
                scans.append((desc, len(blob), sc["end"] - sc["start"], specs))
                owner.append((i, si))
                blob += raw[sc["start"]:sc["end"]]
        seg = torch.frombuffer(blob or bytearray(1), dtype=torch.uint8).to(dev, non_blocking=False)
        plan = BatchPlan(scans, len(blob))
        try:
            off = torch.empty(plan.n_offsets, dtype=torch.int64, device=dev)
            status = torch.empty(plan.n_intervals, dtype=torch.int32, device=dev)
            image = torch.empty(plan.image_bytes, dtype=torch.uint8, device=dev)  # the caching allocator's blocks are 512-byte aligned
            image.copy_(torch.from_numpy(plan.bind(image, seg, off, status)))
            plan.index(stream)
            plan.decode(stream)
            st = status.cpu().numpy()  # the call's one wait for the device
            first = plan.first_interval
        finally:
            plan.close()
        for k, (i, si) in enumerate(owner):
            if isinstance(results[i], Exception):
                continue  # an earlier scan of the file failed: decode_jpeg stops there
            s = st[first[k]:first[k + 1]].copy()
            bad = np.flatnonzero(s)
            if bad.size:
                j = int(bad[0])
                failed(i, JpegDecodeError(f"scan {si}: {bad.size} of {s.size} restart intervals failed; "
                                          f"interval {j}: {STATUS_NAMES.get(int(s[j]), int(s[j]))}", scan=si, status=s))
        planes = []
        for i, info, geo, _, _ in jobs:
            if isinstance(results[i], Exception):
                continue
            try:
                luts = component_luts(info)
            except jfif.JpegFormatError as e:
                failed(i, e)
                continue
            planes += [(p, q, g[2] * 8, g[3] * 8, lut) for p, q, g, lut in zip(pxs[i], coefs[i], geo, luts)]
        if planes:
            api.u8_i16_batch("inv", planes, level_shift=True, stream=stream)
        for i, info, geo, _, _ in jobs:
            if isinstance(results[i], Exception):
                continue
            out = [p[:g[1], :g[0]] for p, g in zip(pxs[i], geo)]
            if mode == "RGB":
                out = to_rgb(out, [(c["h"], c["v"]) for c in info["components"]], info["width"], info["height"], colour=info["colorspace"],
                             layout=layout, stream=stream)
            results[i] = (out, coefs[i]) if coefficients else out


_COLOURS = {"YCbCr": _jpegcolor_lib.YCBCR, "RGB": _jpegcolor_lib.RGB, "grey": _jpegcolor_lib.GREY}
_LAYOUTS = {"HWC": _jpegcolor_lib.HWC, "CHW": _jpegcolor_lib.CHW}


def _colour_params(info):
    """refuse (JpegFormatError) a file the colour stage does not take: other than 1 or 3 components, a fractional sampling ratio"""
    comps = info["components"]
    if info.get("colorspace") not in _COLOURS:
        raise jfif.JpegFormatError(f"no RGB conversion for {len(comps)} components")
    hmax, vmax = max(c["h"] for c in comps), max(c["v"] for c in comps)
    if any(hmax % c["h"] or vmax % c["v"] for c in comps):
        raise jfif.JpegFormatError("fractional sampling ratio: " + ", ".join(f"{c['h']}x{c['v']}" for c in comps))


colour_last_error = _jpegcolor_lib.LIB.last_error


def to_rgb(planes, sampling, width, height, colour="YCbCr", layout="HWC", out=None, stream=None):
    """mdct_jpegcolor_to_rgb on device tensors.  planes: one (grey) or three uint8 [rows, columns] components at their true sizes
    (ceil(width * h / hmax) x ceil(height * v / vmax)); rows may lie any pitch apart, columns must be contiguous.  sampling: [(h, v)]
    of the frame.  colour: 'YCbCr', 'RGB' (planes R, G, B, not converted) or 'grey'.  out: uint8 [height, width, 3] (HWC) or
    [3, height, width] (CHW), allocated if None; its rows and planes may lie any pitch apart, its innermost dimension must be contiguous.
    Returns out."""
    import torch

    if colour not in _COLOURS or layout not in _LAYOUTS:
        raise ValueError(f"colour {colour!r} / layout {layout!r}")
    if len(planes) != len(sampling):
        raise ValueError(f"{len(planes)} planes, {len(sampling)} sampling factors")
    arr = (_jpegcolor_lib.Plane * max(1, len(planes)))()
    for k, (p, (h, v)) in enumerate(zip(planes, sampling)):
        if p.dtype != torch.uint8 or p.dim() != 2 or p.stride(1) != 1:
            raise ValueError(f"plane {k}: uint8 [rows, columns] with contiguous columns")
        arr[k] = _jpegcolor_lib.Plane(p.data_ptr(), p.stride(0), p.shape[1], p.shape[0], h, v)
    shape = (height, width, 3) if layout == "HWC" else (3, height, width)
    if out is None:
        with api._on_stream(stream, planes[0].device):
            out = torch.empty(shape, dtype=torch.uint8, device=planes[0].device)
    if out.dtype != torch.uint8 or tuple(out.shape) != shape or out.stride(-1) != 1 or (layout == "HWC" and out.stride(1) != 3):
        raise ValueError(f"out: uint8 {list(shape)} with contiguous {'pixels' if layout == 'HWC' else 'rows'}")
    pitch, stride = (out.stride(0), 0) if layout == "HWC" else (out.stride(1), out.stride(0))
    _jpegcolor_lib.LIB.check(_jpegcolor_lib.load().mdct_jpegcolor_to_rgb(arr, len(planes), width, height, _COLOURS[colour], _LAYOUTS[layout], out.data_ptr(),
                                                                         pitch, stride, _stream(stream)))
    return out


def decode_scan(torch, si, sc, desc, tables, seg, dev, stream=None):
    """decode scan si of the reader's list as scan_plan planned it (seg: its bytes on the device) into the planes its descriptor names,
    by the route its kind and restart interval ask for, and wait for its status (the copy is ordered on the scan's stream, api._on_stream): per interval (restart-marked, progressive), or [code, blocks decoded]
    (no markers; a NOT_SYNCHRONISED result, an ordinary status and not a fault, is decoded once more with one fix round per chunk,
    which always converges).  Returns the status; JpegDecodeError for a scan that did not decode cleanly."""
    with api._on_stream(stream, dev):
        L = sc["end"] - sc["start"]
        band = (sc["ss"], sc["se"]) if "ss" in sc else None
        if band is not None:
            return _decode_prog_scan(torch, si, sc, band, desc, tables, seg, L, dev, stream)
        if sc["restart_interval"] == 0:
            nbytes = unmarked_workspace(desc, L)
            if nbytes == 0:
                raise api.MdctError(f"invalid scan descriptor: {unmarked_last_error()}")
            work = torch.empty(nbytes, dtype=torch.uint8, device=dev)  # the caching allocator's blocks are 512-byte aligned
            status = torch.empty(2, dtype=torch.int32, device=dev)
            decode_unmarked(desc, tables, seg, work, status, scan_len=L, stream=stream)
            st = status.cpu().numpy()
            if st[0] == _jpegdec_unmarked_lib.NOT_SYNCHRONISED:
                rounds = max(1, _ceil(L, _jpegdec_unmarked_lib.CHUNK_BYTES))
                decode_unmarked(desc, tables, seg, work, status, scan_len=L, sync_rounds=rounds, stream=stream)
                st = status.cpu().numpy()
            if st[0] != 0:
                raise JpegDecodeError(f"scan {si} (no restart markers): {_jpegdec_unmarked_lib.STATUS_NAMES.get(int(st[0]), int(st[0]))} "
                                      f"after {int(st[1])} blocks", scan=si, status=st)
            return st
        n = n_intervals(desc)
        off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        index(seg, n, off, status, scan_len=L, stream=stream)
        decode(desc, tables, seg, off, status, scan_len=L, stream=stream)
        st = status.cpu().numpy()
        bad = np.flatnonzero(st)
        if bad.size:
            k = int(bad[0])
            raise JpegDecodeError(f"scan {si}: {bad.size} of {n} restart intervals failed; "
                                  f"interval {k}: {STATUS_NAMES.get(int(st[k]), int(st[k]))}", scan=si, status=st)
        return st


def _decode_prog_scan(torch, si, sc, band, desc, tables, seg, L, dev, stream):
    """decode_scan for a scan of a progressive file: the interval index, unless the scan has no restart markers -- then it is one
    interval, whose two offsets the host writes -- and one decode launch"""
    ah, al = sc.get("ah", 0), sc.get("al", 0)
    n = prog_intervals(desc, *band)
    with api._on_stream(stream, dev):
        status = torch.empty(n, dtype=torch.int32, device=dev)
        if sc["restart_interval"] == 0:
            off = torch.tensor([0, L], dtype=torch.int64).to(dev, non_blocking=False)
        else:
            off = torch.empty(n + 1, dtype=torch.int64, device=dev)
            index(seg, n, off, status, scan_len=L, stream=stream)
        decode_prog(desc, band[0], band[1], tables, seg, off, status, scan_len=L, stream=stream, ah=ah, al=al)
        st = status.cpu().numpy()
    bad = np.flatnonzero(st)
    if bad.size:
        k = int(bad[0])
        approx = f", Ah {ah} Al {al}" if ah or al else ""
        raise JpegDecodeError(f"scan {si} (band {band[0]}..{band[1]}{approx}): {bad.size} of {n} restart intervals failed; "
                              f"interval {k}: {STATUS_NAMES.get(int(st[k]), int(st[k]))}", scan=si, status=st)
    return st
