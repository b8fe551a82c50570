"""8-bit RGB or grey image -> baseline JPEG file on the GPU (libmdct_jpegenc.so, include/mdct_jpegenc.h; the scan kernels of
include/mdct.h).  The mirror of jpeg_decode.decode_jpeg.

encode_jpeg runs one launch of mdct_jpegenc_from_rgb (RGB -> YCbCr, chroma downsampling and padding to the block grid, as
libjpeg-turbo's compressor does them), then one restart-marked scan per component (mdct_fwd_u8_huffman_rows and
mdct_jpeg_pack_rows_counted: pixels -> stuffed scan with RSTm between the block rows, Annex K tables), copies back the scans' lengths and bytes and writes the marker segments (jfif.write_jpeg).
With interleaved=True a colour image becomes ONE scan whose MCUs interleave the components, the form every other encoder writes
(libmdct_jpegenc_scan.so, include/mdct_jpegenc_scan.h: mdct_jpegenc_scan_rows codes the three planes, padded to the MCU grid, in
MCU order; one packing launch and one read-back instead of three).
With optimize=True the Huffman tables are made for the image (T.81 K.2, libjpeg's optimize_coding; libmdct_jpegenc_opt.so,
include/mdct_jpegenc_opt.h): symbol_histogram counts the symbols the coder will emit, optimal_tables builds the tables on the host and
the coders of that library take them in place of the Annex K ones.
encode_jpeg_batch writes many colour images as interleaved files in three launches (libmdct_jpegenc_batch.so,
include/mdct_jpegenc_batch.h): the mirror of jpeg_decode.decode_jpeg_batch.
torch is used for device memory and streams only.
"""
import ctypes

import numpy as np

from . import _jpegenc_batch_lib, _jpegenc_lib, _jpegenc_opt_lib, _jpegenc_scan_lib, api, jfif
from .api import _stream

# ITU-T T.81 Annex K.1 / K.2 (natural order v*8+u)
K1_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
           18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
K2_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32

# subsampling -> (h, v) of Y; Cb and Cr are (1, 1)
SUBSAMPLING = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}
_LAYOUTS = {"HWC": _jpegenc_lib.HWC, "CHW": _jpegenc_lib.CHW}


def quality_tables(quality):
    """IJG quality scaling of the Annex K tables (libjpeg's jpeg_set_quality with force_baseline): scale = 5000 // q below 50, else
    200 - 2q; entry = clamp((base * scale + 50) // 100, 1, 255).  Returns (luma, chroma), 64 integers each in natural order."""
    q = _quality(quality)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple([min(max((b * scale + 50) // 100, 1), 255) for b in base] for base in (K1_LUMA, K2_CHROMA))


def _quality(quality):
    if isinstance(quality, (bool, np.bool_)) or not isinstance(quality, (int, np.integer)) or not 1 <= quality <= 100:
        raise ValueError(f"quality {quality!r}: an integer 1..100")
    return int(quality)


def _ceil(a, b):
    return -(-a // b)


def sampling_of(subsampling, grey=False):
    """[(h, v)] per component of a frame"""
    if grey:
        return [(1, 1)]
    if subsampling not in SUBSAMPLING:
        raise ValueError(f"subsampling {subsampling!r} ('4:4:4', '4:2:2' or '4:2:0')")
    return [SUBSAMPLING[subsampling], (1, 1), (1, 1)]


def component_sizes(width, height, sampling):
    """[(true width, true height, padded width, padded height)] per component: ceil(W * h / hmax) x ceil(H * v / vmax), padded to
    multiples of 8 (each component's own block grid, T.81 A.2.2)"""
    hmax, vmax = max(h for h, _ in sampling), max(v for _, v in sampling)
    out = []
    for h, v in sampling:
        cw, ch = _ceil(width * h, hmax), _ceil(height * v, vmax)
        out.append((cw, ch, _ceil(cw, 8) * 8, _ceil(ch, 8) * 8))
    return out


def mcu_grid(width, height, sampling):
    """(mcus_x, mcus_y, [(padded width, padded height)] per component on the MCU grid: mcus_x * 8 * h x mcus_y * 8 * v)"""
    hmax, vmax = max(h for h, _ in sampling), max(v for _, v in sampling)
    mx, my = _ceil(width, 8 * hmax), _ceil(height, 8 * vmax)
    return mx, my, [(mx * 8 * h, my * 8 * v) for h, v in sampling]


last_error = _jpegenc_lib.LIB.last_error


def _image_shape(image, layout):
    """(height, width, grey) of a uint8 image [H, W, 3] (HWC), [3, H, W] (CHW) or [H, W] (grey)"""
    if layout not in _LAYOUTS:
        raise ValueError(f"layout {layout!r} ('HWC' or 'CHW')")
    shape = tuple(image.shape)
    if len(shape) == 2:
        H, W, grey = shape[0], shape[1], True
    elif len(shape) == 3 and layout == "HWC" and shape[2] == 3:
        H, W, grey = shape[0], shape[1], False
    elif len(shape) == 3 and layout == "CHW" and shape[0] == 3:
        H, W, grey = shape[1], shape[2], False
    else:
        raise ValueError(f"image of shape {list(shape)}: [H, W, 3] (HWC), [3, H, W] (CHW) or [H, W] (grey)")
    if not (1 <= W <= 65535 and 1 <= H <= 65535):
        raise ValueError(f"image {W}x{H}: 1..65535 each way")
    return H, W, grey


def _input_of(image, layout, grey=False):
    """(pitch, plane stride) of a tensor the front kernels read in place: contiguous innermost dimension, HWC pixels of 3 contiguous bytes.
    The stride of a dimension of one element addresses nothing and may be anything (a 1 x 1 image seen through permute or numpy's
    moveaxis, which both call contiguous): it is taken as the contiguous one."""
    def step(dim, natural):
        return natural if image.shape[dim] == 1 else image.stride(dim)

    if grey:
        ok, pitch, stride = step(1, 1) == 1, step(0, image.shape[1]), 0
    elif layout == "HWC":
        ok, pitch, stride = image.stride(2) == 1 and step(1, 3) == 3, step(0, 3 * image.shape[1]), 0
    else:
        ok, pitch, stride = step(2, 1) == 1, step(1, image.shape[2]), image.stride(0)
    if not ok:
        raise ValueError("image: contiguous innermost dimension (HWC: 3 contiguous bytes per pixel)")
    return pitch, stride


def to_planes(image, subsampling="4:2:0", layout="HWC", planes=None, stream=None):
    """mdct_jpegenc_from_rgb on a device tensor.  image: uint8 [H, W, 3] (HWC), [3, H, W] (CHW) or [H, W] (grey); its rows (and CHW
    planes) may lie any pitch apart, the innermost dimension must be contiguous (HWC: pixels of 3 contiguous bytes).  planes: uint8
    [rows, columns] per component, each at least its padded size (component_sizes) with contiguous columns; allocated at exactly that
    size if None.  The whole of each given plane is written.  Returns the planes."""
    import torch

    H, W, grey = _image_shape(image, layout)
    if image.dtype != torch.uint8 or not image.is_cuda:
        raise ValueError("image: a uint8 device tensor")
    sampling = sampling_of(subsampling, grey)
    sizes = component_sizes(W, H, sampling)
    pitch, stride = _input_of(image, layout, grey)
    if planes is None:
        with api._on_stream(stream, image.device):
            planes = [torch.empty((ph, pw), dtype=torch.uint8, device=image.device) for _, _, pw, ph in sizes]
    if len(planes) != len(sampling):
        raise ValueError(f"{len(planes)} planes for {len(sampling)} components")
    arr = (_jpegenc_lib.Plane * len(planes))()
    for k, (p, (h, v)) in enumerate(zip(planes, sampling)):
        if p.dtype != torch.uint8 or p.dim() != 2 or p.stride(1) != 1 or not p.is_cuda:
            raise ValueError(f"plane {k}: uint8 device tensor [rows, columns] with contiguous columns")
        arr[k] = _jpegenc_lib.Plane(p.data_ptr(), p.stride(0), p.shape[1], p.shape[0], h, v)
    colour = _jpegenc_lib.GREY if grey else _jpegenc_lib.RGB
    _jpegenc_lib.LIB.check(_jpegenc_lib.load().mdct_jpegenc_from_rgb(image.data_ptr(), pitch, stride, W, H, colour, _LAYOUTS[layout], arr, len(planes),
                                                                     _stream(stream)))
    return planes


def scan_seg_stride(mcus_x, sampling):
    """smallest legal seg_stride of scan_rows (mdct_jpegenc_scan_seg_stride)"""
    return int(_jpegenc_scan_lib.load().mdct_jpegenc_scan_seg_stride(mcus_x, sum(h * v for h, v in sampling)))


def _plane_array(planes, sampling):
    arr = (_jpegenc_scan_lib.Plane * max(1, len(planes)))()
    for k, (p, (h, v)) in enumerate(zip(planes, sampling)):
        if p.dim() != 2 or p.stride(1) != 1 or p.element_size() != 1:
            raise ValueError(f"plane {k}: uint8 tensor [rows, columns] with contiguous columns")
        arr[k] = _jpegenc_scan_lib.Plane(p.data_ptr(), p.stride(0), p.shape[1], p.shape[0], h, v)
    return arr


def scan_rows(planes, sampling, luts, out, seg_bytes, ff_counts, seg_stride=None, my0=0, my1=None, stream=None, check=True):
    """mdct_jpegenc_scan_rows on device tensors.  planes: Y, Cb, Cr, uint8 [rows, columns] with contiguous columns, each exactly its size
    on the MCU grid (mcu_grid); sampling: [(h, v)] per component; luts: (luma, chroma), 64 numbers each in natural order.  out: uint8,
    one segment per MCU row seg_stride apart (default: scan_seg_stride); seg_bytes / ff_counts: int32 per MCU row.  MCU rows my0 .. my1
    (default: all) are coded.  Returns the status (raises unless check=False)."""
    arr = _plane_array(planes, sampling)
    tabs = [api._lut64(t) for t in luts]
    mcus_x, mcus_y = planes[-1].shape[1] // 8, planes[-1].shape[0] // 8
    if seg_stride is None:
        seg_stride = scan_seg_stride(mcus_x, sampling)
    lib = _jpegenc_scan_lib.load()
    rc = lib.mdct_jpegenc_scan_rows(arr, len(planes), tabs[0].ctypes.data, tabs[1].ctypes.data, my0, mcus_y if my1 is None else my1, out.data_ptr(), seg_stride,
                                    seg_bytes.data_ptr(), ff_counts.data_ptr(), _stream(stream))
    if check:
        _jpegenc_scan_lib.LIB.check(rc)
    return rc


_opt_error = _jpegenc_opt_lib.LIB.error


def symbol_histogram(planes, sampling, luts, interleaved=False, hist=None, stream=None, check=True):
    """mdct_jpegenc_opt_stats on device tensors: the counts of the Huffman symbols that the coder of these planes and tables emits.
    planes: 1 (grey) or 3 (Y, Cb, Cr) uint8 [rows, columns] with contiguous columns -- interleaved=False: each on its own block grid
    (component_sizes), every plane a scan of its own with a restart interval per block row; interleaved=True: on the MCU grid (mcu_grid),
    one scan in MCU order with a restart interval per MCU row.  sampling: [(h, v)] per component; luts: (luma, chroma), 64 numbers each.
    hist: int32 device tensor [2, 272] (allocated if None), zeroed by the call itself: class 0 luminance, 1 chrominance; entries 0..15 the
    DC categories, 16 + RRRRSSSS the AC symbols.  Returns hist (with check=False: (status, hist))."""
    import torch

    if not isinstance(interleaved, (bool, np.bool_)):
        raise ValueError(f"interleaved {interleaved!r}: a bool")
    arr = _plane_array(planes, sampling)
    tabs = [api._lut64(t) for t in luts]
    if hist is None:
        with api._on_stream(stream, planes[0].device):
            hist = torch.empty((2, _jpegenc_opt_lib.HIST_CLASS), dtype=torch.int32, device=planes[0].device)
    if hist.dtype != torch.int32 or tuple(hist.shape) != (2, _jpegenc_opt_lib.HIST_CLASS) or not hist.is_contiguous():
        raise ValueError("hist: a contiguous int32 tensor [2, 272]")
    rc = _jpegenc_opt_lib.load().mdct_jpegenc_opt_stats(arr, len(planes), tabs[0].ctypes.data, tabs[-1].ctypes.data, int(interleaved), hist.data_ptr(), _stream(stream))
    if check and rc != 0:
        raise _opt_error(rc)
    return hist if check else (rc, hist)


def optimal_table(counts):
    """mdct_jpegenc_opt_table (host): libjpeg's optimal Huffman table for the counts of one class (12..16 DC categories or 256 AC
    symbols) -> (bits16, vals)"""
    c = np.ascontiguousarray(np.asarray(counts).astype(np.uint32))
    bits = np.zeros(16, dtype=np.uint8)
    vals = np.zeros(256, dtype=np.uint8)
    n = _jpegenc_opt_lib.c_int()
    rc = _jpegenc_opt_lib.load().mdct_jpegenc_opt_table(c.ctypes.data, c.size, bits.ctypes.data, vals.ctypes.data, n)
    if rc != 0:
        raise _opt_error(rc)
    return bits.tolist(), vals[:n.value].tolist()


def optimal_tables(hist, grey=False):
    """hist of symbol_histogram (a device tensor is copied to the host on torch's current stream: that waits for the histogram only when
    it was made on that stream, as it is inside encode_jpeg, which runs under api._on_stream) -> {which: (bits16, vals)} keyed like
    api.huffman_spec: 0 DC luminance, 1 AC luminance, 2 DC chrominance, 3 AC chrominance (grey: 0 and 1 only)"""
    h = np.asarray(hist.cpu() if hasattr(hist, "cpu") else hist).astype(np.int64).reshape(2, _jpegenc_opt_lib.HIST_CLASS) & 0xFFFFFFFF
    out = {}
    for cls in range(1 if grey else 2):
        out[2 * cls] = optimal_table(h[cls, :16])
        out[2 * cls + 1] = optimal_table(h[cls, 16:])
    return out


class _Specs:
    """{which: (bits16, vals)} as the mdct_jpegenc_opt_spec array of the coders (keeps the host arrays alive)"""

    def __init__(self, specs, which):
        self.keep = []
        self.arr = (_jpegenc_opt_lib.Spec * len(which))()
        for k, w in enumerate(which):
            bits, vals = specs[w]
            b, v = np.ascontiguousarray(np.asarray(bits, dtype=np.uint8)), np.ascontiguousarray(np.asarray(vals, dtype=np.uint8))
            if b.shape != (16,) or v.ndim != 1:
                raise ValueError(f"specification {w}: (16 counts, values)")
            self.keep += [b, v]
            self.arr[k] = _jpegenc_opt_lib.Spec(b.ctypes.data, v.ctypes.data, v.size)


def opt_seg_stride(blocks):
    """smallest legal seg_stride of opt_rows / opt_scan_rows for segments of `blocks` blocks (mdct_jpegenc_opt_seg_stride)"""
    return int(_jpegenc_opt_lib.load().mdct_jpegenc_opt_seg_stride(blocks))


def opt_rows(plane, lut, specs, out, seg_bytes, ff_counts, uncoded, seg_stride=None, by0=0, by1=None, stream=None, check=True):
    """mdct_jpegenc_opt_rows on device tensors: one plane (uint8 [rows, columns], multiples of 8, contiguous columns) -> one segment per
    block row, coded with specs = (DC (bits16, vals), AC (bits16, vals)).  uncoded: an int32 device tensor of one element that the
    caller has zeroed; the call adds the number of symbols the tables have no code for.  Otherwise as api.fwd_u8_huffman_rows."""
    if plane.dim() != 2 or plane.stride(1) != 1 or plane.element_size() != 1:
        raise ValueError("plane: uint8 tensor [rows, columns] with contiguous columns")
    sp = _Specs({0: specs[0], 1: specs[1]}, (0, 1))
    tab = api._lut64(lut)
    ph, pw = plane.shape
    if seg_stride is None:
        seg_stride = opt_seg_stride(pw // 8)
    rc = _jpegenc_opt_lib.load().mdct_jpegenc_opt_rows(plane.data_ptr(), plane.stride(0), tab.ctypes.data, pw, ph, by0, ph // 8 if by1 is None else by1, sp.arr[0], sp.arr[1],
                                                       out.data_ptr(), seg_stride, seg_bytes.data_ptr(), ff_counts.data_ptr(), uncoded.data_ptr(), _stream(stream))
    if check and rc != 0:
        raise _opt_error(rc)
    return rc


def opt_scan_rows(planes, sampling, luts, specs, out, seg_bytes, ff_counts, uncoded, seg_stride=None, my0=0, my1=None, stream=None, check=True):
    """mdct_jpegenc_opt_scan_rows on device tensors: scan_rows with specs = {which: (bits16, vals)} keyed like api.huffman_spec in place of
    the Annex K tables, seg_stride at least opt_seg_stride(blocks per MCU row), and uncoded as for opt_rows."""
    arr = _plane_array(planes, sampling)
    sp = _Specs(specs, (0, 1, 2, 3))
    tabs = [api._lut64(t) for t in luts]
    mcus_x, mcus_y = planes[-1].shape[1] // 8, planes[-1].shape[0] // 8
    if seg_stride is None:
        seg_stride = opt_seg_stride(mcus_x * sum(h * v for h, v in sampling))
    rc = _jpegenc_opt_lib.load().mdct_jpegenc_opt_scan_rows(arr, len(planes), tabs[0].ctypes.data, tabs[1].ctypes.data, sp.arr, my0, mcus_y if my1 is None else my1,
                                                            out.data_ptr(), seg_stride, seg_bytes.data_ptr(), ff_counts.data_ptr(), uncoded.data_ptr(), _stream(stream))
    if check and rc != 0:
        raise _opt_error(rc)
    return rc


def _first_capacity(pixels):
    """bytes of the first scan buffer: ~0.2 bytes per pixel in practice; a scan that does not fit is coded again into its worst case"""
    return pixels + 4096


def _encode_interleaved(torch, image, W, H, sampling, subsampling, layout, tabs, stream, optimize=False):
    """the colour image as one interleaved scan: front launch into planes on the MCU grid, scan_rows, the packing launch, one read-back.
    optimize: the statistics launch and the wait for its histogram first, then opt_scan_rows with the tables made from it"""
    dev = image.device
    with api._on_stream(stream, dev):  # the allocations, the fill of `uncoded` and the copies the host reads: all on the stream of the launches
        mcus_x, mcus_y, sizes = mcu_grid(W, H, sampling)
        planes = to_planes(image, subsampling, layout, planes=[torch.empty((ph, pw), dtype=torch.uint8, device=dev) for pw, ph in sizes], stream=stream)
        stride = opt_seg_stride(mcus_x * sum(h * v for h, v in sampling)) if optimize else scan_seg_stride(mcus_x, sampling)
        seg = torch.empty((mcus_y * stride,), dtype=torch.uint8, device=dev)
        counts = torch.empty((2, mcus_y), dtype=torch.int32, device=dev)
        off = torch.empty((mcus_y + 1,), dtype=torch.int64, device=dev)
        specs = None
        if optimize:
            specs = optimal_tables(symbol_histogram(planes, sampling, tabs, interleaved=True, stream=stream))  # the copy, on the call's stream, that waits for the histogram
            uncoded = torch.zeros((1,), dtype=torch.int32, device=dev)
            opt_scan_rows(planes, sampling, tabs, specs, seg, counts[0], counts[1], uncoded, seg_stride=stride, stream=stream)
        else:
            scan_rows(planes, sampling, (tabs[0], tabs[1]), seg, counts[0], counts[1], seg_stride=stride, stream=stream)
        out = torch.empty((_first_capacity(sum(pw * ph for pw, ph in sizes)),), dtype=torch.uint8, device=dev)
        api.jpeg_pack_rows(seg, counts[0], stride, mcus_y, out, off, ff_counts=counts[1], stream=stream)
        end = int(off[-1].item())  # the one copy that waits for the scan: it is ordered on the call's stream
        if end > out.numel():  # the segments are there: only the packing runs again, into the worst case
            out = torch.empty((2 * mcus_y * stride,), dtype=torch.uint8, device=dev)
            api.jpeg_pack_rows(seg, counts[0], stride, mcus_y, out, off, ff_counts=counts[1], stream=stream)
            end = int(off[-1].item())
        if optimize and int(uncoded.item()) != 0:
            raise api.MdctError(f"{int(uncoded.item())} symbols of the scan have no code in the tables made for it")
        return dict(scan=out[:end].cpu().numpy(), mcus_per_row=mcus_x), specs


class _Scan:
    """device buffers of one component's scan"""

    def __init__(self, torch, dev, pw, ph, capacity, optimize=False):
        rows = ph // 8
        self.stride = opt_seg_stride(pw // 8) if optimize else api.huffman_seg_stride(pw)
        self.seg = torch.empty((rows * self.stride,), dtype=torch.uint8, device=dev)
        self.out = torch.empty((capacity,), dtype=torch.uint8, device=dev)
        self.off = torch.empty((rows + 1,), dtype=torch.int64, device=dev)
        self.work = torch.zeros((rows + 2,), dtype=torch.int64, device=dev)  # the one-launch form's chain between the rows
        self.counts = torch.empty((2, rows), dtype=torch.int32, device=dev)  # the two-launch form's byte and 0xFF counts


def _run_scan(plane, pw, ph, lut, chroma, sc, two_launch, stream, specs=None, uncoded=None):
    if specs is not None:  # optimize: the caller's tables, always the two-launch form
        opt_rows(plane, lut, (specs[2 if chroma else 0], specs[3 if chroma else 1]), sc.seg, sc.counts[0], sc.counts[1], uncoded, seg_stride=sc.stride, stream=stream)
        api.jpeg_pack_rows(sc.seg, sc.counts[0], sc.stride, ph // 8, sc.out, sc.off, ff_counts=sc.counts[1], stream=stream)
    elif two_launch:
        api.fwd_u8_huffman_rows(plane, pw, ph, sc.seg, sc.counts[0], lut=lut, chroma=chroma, seg_stride=sc.stride, pitch=plane.stride(0),
                                ff_counts=sc.counts[1], stream=stream)
        api.jpeg_pack_rows(sc.seg, sc.counts[0], sc.stride, ph // 8, sc.out, sc.off, ff_counts=sc.counts[1], stream=stream)
    else:
        api.fwd_u8_jpeg_scan(plane, pw, ph, sc.seg, sc.work, sc.out, sc.off, lut=lut, chroma=chroma, seg_stride=sc.stride, pitch=plane.stride(0),
                             stream=stream)


def encode_jpeg(image, quality=75, subsampling="4:2:0", layout="HWC", device=None, stream=None, *, two_launch=True, interleaved=False, optimize=False, progressive=False, script=None):
    """Encode an 8-bit image as a baseline JPEG (JFIF) on the GPU and return the file as bytes.

    image: uint8 [H, W, 3] (layout="HWC"), [3, H, W] (layout="CHW") or [H, W] (grey, any layout); a numpy array or CPU tensor is
    uploaded to `device` first (default: the current device).  quality: an integer 1..100 (IJG scaling of the Annex K tables,
    quality_tables).  subsampling: '4:4:4', '4:2:2' or '4:2:0' (ignored for grey).  Arguments are checked before any device work.

    Colour images go through one launch of mdct_jpegenc_from_rgb (libjpeg-turbo's RGB -> YCbCr and downsampling, planes padded to each
    component's block grid by edge replication).  A grey image whose sides are multiples of 8 needs no padding and goes straight to
    its scan, with no front launch.  Each component is then one non-interleaved scan over its own block grid, with the Annex K Huffman
    tables and a restart marker after every block row (DRI = blocks per row, first marker RST0), made by mdct_fwd_u8_huffman_rows and
    mdct_jpeg_pack_rows_counted (two_launch=False: one launch of mdct_fwd_u8_jpeg_scan per component, the same bytes; 9 % slower at
    8192x8192 4:2:0).  Only the scans' lengths and bytes are copied back.

    interleaved=True (a bool): a colour image is written as ONE scan whose MCUs interleave the components (T.81 A.2.3; DRI = MCUs per
    row), the form cameras, libjpeg-turbo and hardware coders write: the planes are padded to the MCU grid, mdct_jpegenc_scan_rows
    codes them in MCU order and one packing launch finishes the scan (two_launch plays no part).  A grey
    image has one component, whose scan is non-interleaved by definition: the argument changes nothing there.

    optimize=True (a bool): the Huffman tables are made for this image (T.81 K.2, what libjpeg's optimize_coding and Pillow's
    optimize=True do; typically a tenth fewer bytes, the same coefficients): after the front launch one statistics launch counts the
    symbols the coder will emit (symbol_histogram), its 2176 bytes are copied back -- a second wait besides the one for the scan --, the
    tables (one luminance and one chrominance pair, whatever the scan form) are built on the host (optimal_tables), and the coders of
    libmdct_jpegenc_opt.so write the segments with them (two_launch plays no part); the file carries the tables in its DHT segment.
    DESIGN.md section 4.9.2.

    progressive=True (a bool): a progressive file (SOF2) with spectral selection, the scans jpeg_transcode.encode_coefficients(
    progressive=True) writes with its default bands.  The planes are padded to the MCU grid, mdct_fwd_u8_i16
    with the level shift and the quality tables makes the quantised coefficients the pixel coders are defined on, and the band coders
    saturate AC levels to +-1023 as the pixel coders do.  The tables are always made for the image: optimize=False is accepted and
    plays no part, nor does two_launch; interleaved selects the form of the DC scan.  decode_jpeg reads the file back.
    script (with progressive=True only: ValueError otherwise): None is the file above; 'standard' is libjpeg's standard script with
    successive approximation, what Pillow's progressive=True writes; a list of (components, ss, se, ah, al)
    is checked by jpeg_progressive.check_script.  With a script its scans' component lists decide which DC scans are interleaved.

    stream: None (torch's current stream), a torch.cuda.Stream or a raw hipStream_t.  All device work of the call -- its kernels, its own
    allocations, fills and the upload of a host image, and the copies of the histogram, the scans' lengths and their bytes that the host
    waits for -- is ordered on that stream (api._on_stream), whatever torch's current stream is.  A device image must be ready for
    `stream`: work that produces it on another stream has to be waited for first (wait_stream / an event).  The bytes returned are
    complete."""
    import torch

    q = _quality(quality)
    if not isinstance(interleaved, (bool, np.bool_)):
        raise ValueError(f"interleaved {interleaved!r}: a bool")
    if not isinstance(optimize, (bool, np.bool_)):
        raise ValueError(f"optimize {optimize!r}: a bool")
    if not isinstance(progressive, (bool, np.bool_)):
        raise ValueError(f"progressive {progressive!r}: a bool")
    if script is not None and not progressive:
        raise ValueError("script: only with progressive=True")
    if isinstance(image, np.ndarray):
        if image.dtype != np.uint8:
            raise ValueError(f"image dtype {image.dtype}: uint8")
    elif not isinstance(image, torch.Tensor) or image.dtype != torch.uint8:
        raise ValueError("image: a uint8 numpy array or torch tensor")
    H, W, grey = _image_shape(image, layout)
    sampling = sampling_of(subsampling, grey)
    sizes = component_sizes(W, H, sampling)
    luma, chroma = quality_tables(q)
    if progressive:
        from . import jpeg_progressive

        script = jpeg_progressive.resolve_script(script, None, len(sampling), bool(interleaved) and not grey, sampling)
    dev = api._device(device)
    if isinstance(image, np.ndarray):
        image = torch.from_numpy(np.ascontiguousarray(image))
    if not image.is_cuda:
        with api._on_stream(stream, dev):
            image = image.to(dev)
    dev = image.device
    with torch.cuda.device(dev), api._on_stream(stream, dev):
        if progressive:
            mcus_x, mcus_y, padded = mcu_grid(W, H, sampling)
            planes = to_planes(image, subsampling, layout, planes=[torch.empty((ph, pw), dtype=torch.uint8, device=dev) for pw, ph in padded], stream=stream)
            tabs = [luma] + [chroma] * (len(planes) - 1)
            coefs = [torch.empty(p.shape, dtype=torch.int16, device=dev) for p in planes]
            api.u8_i16_batch("fwd", [(p, c, pw, ph, np.asarray(t, dtype=np.float32)) for p, c, (pw, ph), t in zip(planes, coefs, padded, tabs)], level_shift=True, stream=stream)
            return jpeg_progressive.encode(torch, coefs, tabs, W, H, sampling, mcus_x, mcus_y, None, script, stream, saturate=True)
        if interleaved and not grey:
            scan, specs = _encode_interleaved(torch, image, W, H, sampling, subsampling, layout, (luma, chroma), stream, optimize)
            return jfif.write_jpeg([dict(qtable=luma), dict(qtable=chroma), dict(qtable=chroma)], W, H, specs=specs, sampling=sampling, interleaved=scan)
        if grey and W % 8 == 0 and H % 8 == 0 and image.stride(1) == 1:
            planes = [image]
        else:
            planes = to_planes(image, subsampling, layout, stream=stream)
        tabs = [luma] + [chroma] * (len(planes) - 1)
        specs = uncoded = None
        if optimize:
            specs = optimal_tables(symbol_histogram(planes, sampling, (luma, chroma), stream=stream), grey=grey)  # the copy, on the call's stream, that waits for the histogram
            uncoded = torch.zeros((1,), dtype=torch.int32, device=dev)
        # ~0.2 bytes per pixel in practice; a scan that does not fit is coded again into its worst case
        scans = [_Scan(torch, dev, pw, ph, _first_capacity(pw * ph), optimize) for _, _, pw, ph in sizes]
        for k, (p, (_, _, pw, ph), sc) in enumerate(zip(planes, sizes, scans)):
            _run_scan(p, pw, ph, tabs[k], k > 0, sc, two_launch, stream, specs, uncoded)
        ends = torch.stack([sc.off[-1] for sc in scans]).cpu().tolist()  # the one copy that waits for the scans: it is ordered on the call's stream
        for k, (p, (_, _, pw, ph), sc) in enumerate(zip(planes, sizes, scans)):
            if ends[k] < 0:  # UINT64_MAX read as int64
                raise api.MdctError(f"scan {k}: the one-launch coder reported a failure (row_offsets = UINT64_MAX)")
            if ends[k] > sc.out.numel():
                sc.out = torch.empty((2 * (ph // 8) * sc.stride,), dtype=torch.uint8, device=dev)
                if optimize:  # the segments are there: only the packing runs again
                    api.jpeg_pack_rows(sc.seg, sc.counts[0], sc.stride, ph // 8, sc.out, sc.off, ff_counts=sc.counts[1], stream=stream)
                else:
                    _run_scan(p, pw, ph, tabs[k], k > 0, sc, two_launch, stream)
                ends[k] = int(sc.off[-1].item())
        if optimize and int(uncoded.item()) != 0:
            raise api.MdctError(f"{int(uncoded.item())} symbols of the scans have no code in the tables made for them")
        comps = [dict(scan=sc.out[:n].cpu().numpy(), blocks_per_row=pw // 8, qtable=t) for sc, n, (_, _, pw, _), t in zip(scans, ends, sizes, tabs)]
    return jfif.write_jpeg(comps, W, H, specs=specs, sampling=sampling)


batch_last_error = _jpegenc_batch_lib.LIB.last_error


class BatchPlan:
    """mdct_jpegenc_batch_plan: the host's plan of a batch of colour images (include/mdct_jpegenc_batch.h); no device is needed to make
    one, the addresses are only compared.  images: list of (address, pitch, plane stride, width, height, planes, segment address,
    seg_stride) with planes = 3 x (address, pitch, padded width, padded height, h, v) on the MCU grid; layout 'HWC' or 'CHW'; luts:
    (luma, chroma), 64 numbers each in natural order.  MdctError (.image: the image refused, None for the batch as a whole) with the
    single-image libraries' messages for what they refuse."""

    def __init__(self, images, layout, luts):
        lib = _jpegenc_batch_lib.load()
        arr = (_jpegenc_batch_lib.BatchImage * max(1, len(images)))()
        for i, (address, pitch, stride, width, height, planes, seg, seg_stride) in enumerate(images):
            arr[i].in_, arr[i].in_pitch, arr[i].in_plane_stride, arr[i].width, arr[i].height = address, pitch, stride, width, height
            for k, p in enumerate(planes):
                arr[i].planes[k] = _jpegenc_lib.Plane(*p)
            arr[i].seg, arr[i].seg_stride = seg, seg_stride
        tabs = [api._lut64(t) for t in luts]
        h, bad = ctypes.c_void_p(), ctypes.c_size_t()
        rc = lib.mdct_jpegenc_batch_plan_create(ctypes.byref(h), arr, len(images), _LAYOUTS[layout], tabs[0].ctypes.data, tabs[1].ctypes.data, ctypes.byref(bad))
        if rc != 0:
            e = _jpegenc_batch_lib.LIB.error(rc)
            e.image = bad.value if bad.value < len(images) else None
            raise e
        self.handle, self._lib = h, lib
        self.n_images = int(lib.mdct_jpegenc_batch_images(h))
        self.n_rows = int(lib.mdct_jpegenc_batch_rows(h))
        self.n_tiles = int(lib.mdct_jpegenc_batch_tiles(h))
        self.image_bytes = int(lib.mdct_jpegenc_batch_image_bytes(h))
        self.first_row = [int(lib.mdct_jpegenc_batch_first_row(h, i)) for i in range(self.n_images + 1)]
        self.first_tile = [int(lib.mdct_jpegenc_batch_first_tile(h, i)) for i in range(self.n_images + 1)]

    def row_table(self):
        """the packer's row table: (image, 1 if the row is its image's last, m of the RSTm after it) per MCU row of the batch"""
        lib, h = self._lib, self.handle
        return [(int(lib.mdct_jpegenc_batch_row_image(h, r)), int(lib.mdct_jpegenc_batch_row_last(h, r)), int(lib.mdct_jpegenc_batch_row_marker(h, r)))
                for r in range(self.n_rows)]

    _rc = staticmethod(_jpegenc_batch_lib.LIB.check)

    def bind(self, device_image, seg_bytes, ff_counts):
        """mdct_jpegenc_batch_bind: -> the image as a numpy uint8 array, to be copied to device_image (a device tensor of image_bytes
        bytes) before the first launch.  seg_bytes, ff_counts: n_rows int32 device tensors each."""
        host = np.zeros(self.image_bytes, dtype=np.uint8)
        self._rc(self._lib.mdct_jpegenc_batch_bind(self.handle, host.ctypes.data, api._ptr(device_image), api._ptr(seg_bytes), api._ptr(ff_counts)))
        return host

    def planes(self, stream=None):
        """mdct_jpegenc_batch_planes: one launch"""
        self._rc(self._lib.mdct_jpegenc_batch_planes(self.handle, _stream(stream)))

    def scan(self, stream=None):
        """mdct_jpegenc_batch_scan: one launch"""
        self._rc(self._lib.mdct_jpegenc_batch_scan(self.handle, _stream(stream)))

    def pack(self, out, row_offsets, stream=None):
        """mdct_jpegenc_batch_pack: one launch.  out: uint8 device tensor (its size is the capacity); row_offsets: n_rows + 1 int64"""
        self._rc(self._lib.mdct_jpegenc_batch_pack(self.handle, api._ptr(out), out.numel(), api._ptr(row_offsets), _stream(stream)))

    def close(self):
        if self.handle:
            self._lib.mdct_jpegenc_batch_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_ARENA_ALIGN = 256  # bytes between the starts of two images, planes or segment ranges of an arena, at least


def _align(n):
    return _ceil(n, _ARENA_ALIGN) * _ARENA_ALIGN


def encode_jpeg_batch(images, quality=75, subsampling="4:2:0", layout="HWC", device=None, stream=None):
    """Encode a sequence of 8-bit images as baseline JPEG files on the GPU: a list of bytes, file i byte for byte what
    encode_jpeg(images[i], quality, subsampling, layout, interleaved=True) returns.  The mirror of jpeg_decode.decode_jpeg_batch.

    images: uint8 images of any sizes, each [H, W, 3] (layout="HWC"), [3, H, W] (layout="CHW") or [H, W] (grey) -- numpy arrays, CPU
    tensors and device tensors in any mix (device tensors on one device; views with a pitch are used in place) -- or one 4-D array or
    tensor, taken as the sequence of its slices.  One quality, subsampling and layout per call.  Every image's arguments are checked
    before any device work: the checks are encode_jpeg's and raise ValueError with its messages and the added attribute .file, the
    image's index.  An empty sequence returns [] without touching the device.

    All colour images go through THREE launches whatever their number (libmdct_jpegenc_batch.so, include/mdct_jpegenc_batch.h; DESIGN.md
    section 4.15): the front kernel over the tiles of all images, the scan coder with one workgroup per MCU row of the batch, the
    packer likewise.  The host images go up in one copy (device images are not copied); planes, segments, counts, row offsets and
    output are one allocation each; the row offsets come back in one copy, the scans' bytes in one more.  The output's first capacity
    is the sum of the images' first capacities; if the scans do not fit, only the packing launch runs again, into the worst case.  A
    batch of more than 16384 MCU rows is cut into consecutive groups below that bound, three launches each.  A grey image has no
    interleaved form: it is coded by encode_jpeg inside the call, on the same stream, at its place in the list.

    stream: as for encode_jpeg -- every launch, allocation, upload and copy back of the call is ordered on it."""
    import torch

    if isinstance(images, (np.ndarray, torch.Tensor)):
        if len(images.shape) != 4:
            raise ValueError(f"images of shape {list(images.shape)}: a sequence of images, or one 4-D array or tensor of them")
        images = [images[i] for i in range(images.shape[0])]
    images = list(images)
    try:  # what encode_jpeg checks first, for the first image
        q = _quality(quality)
        if layout not in _LAYOUTS:
            raise ValueError(f"layout {layout!r} ('HWC' or 'CHW')")
        sampling = sampling_of(subsampling)
    except ValueError as e:
        if images:
            e.file = 0
        raise
    if not images:
        return []
    # ---- host: every image's arguments
    shapes, dev = [], None
    for i, image in enumerate(images):
        try:
            if isinstance(image, np.ndarray):
                if image.dtype != np.uint8:
                    raise ValueError(f"image dtype {image.dtype}: uint8")
            elif not isinstance(image, torch.Tensor) or image.dtype != torch.uint8:
                raise ValueError("image: a uint8 numpy array or torch tensor")
            H, W, grey = _image_shape(image, layout)
            place = None
            if not grey and isinstance(image, torch.Tensor) and image.is_cuda:
                place = _input_of(image, layout)
                if dev is not None and image.device != dev:
                    raise ValueError(f"image on {image.device}: the device images of one batch lie on one device ({dev})")
                dev = image.device
            shapes.append((H, W, grey, place))
        except ValueError as e:
            e.file = i
            raise
    if device is not None:
        dev = torch.device(f"cuda:{device}" if isinstance(device, int) else device) if dev is None else dev
    elif dev is None:
        dev = torch.device("cuda")
    luma, chroma = quality_tables(q)
    results = [None] * len(images)
    colour = [i for i, (_, _, grey, _) in enumerate(shapes) if not grey]
    with torch.cuda.device(dev), api._on_stream(stream, dev):
        # ---- the host images of the colour path: one buffer, one copy
        at, n_up = {}, 0
        for i in colour:
            H, W, _, place = shapes[i]
            if place is None:
                at[i] = n_up
                n_up += _align(3 * W * H)
        if n_up:
            staging = np.empty(n_up, dtype=np.uint8)
            for i, a0 in at.items():
                H, W = shapes[i][:2]
                src = images[i] if isinstance(images[i], np.ndarray) else images[i].numpy()
                staging[a0:a0 + 3 * W * H] = np.ascontiguousarray(src).reshape(-1)
            uploaded = torch.from_numpy(staging).to(dev)
        # ---- consecutive groups of colour images within the packer's row bound
        groups, rows = [[]], 0
        for i in colour:
            my = mcu_grid(shapes[i][1], shapes[i][0], sampling)[1]
            if groups[-1] and rows + my > _jpegenc_batch_lib.MAX_ROWS:
                groups.append([])
                rows = 0
            groups[-1].append(i)
            rows += my
        for group in groups:
            if group:
                inputs = []
                for i in group:
                    H, W, _, place = shapes[i]
                    if place is None:
                        inputs.append((uploaded.data_ptr() + at[i], 3 * W if layout == "HWC" else W, W * H))
                    else:
                        inputs.append((images[i].data_ptr(),) + place)
                _encode_group(torch, group, inputs, shapes, sampling, layout, (luma, chroma), dev, stream, results)
        for i, (_, _, grey, _) in enumerate(shapes):
            if grey:
                results[i] = encode_jpeg(images[i], q, subsampling, layout, device=dev, stream=stream)
    return results


def _encode_group(torch, group, inputs, shapes, sampling, layout, tabs, dev, stream, results):
    """the three launches of encode_jpeg_batch for the colour images `group` names (inputs: (address, pitch, plane stride) of each on
    the device); their files go to results"""
    with api._on_stream(stream, dev):  # (the caller's, again: every allocation and copy below is on the stream of the launches)
        grids, n_planes, n_seg, capacity, worst = [], 0, 0, 0, 0
        for i in group:
            H, W = shapes[i][:2]
            mcus_x, mcus_y, sizes = mcu_grid(W, H, sampling)
            stride = scan_seg_stride(mcus_x, sampling)
            p_at = []
            for pw, ph in sizes:
                p_at.append(n_planes)
                n_planes += _align(pw * ph)
            grids.append((mcus_x, mcus_y, sizes, stride, p_at, n_seg))
            n_seg += _align(mcus_y * stride)
            capacity += _first_capacity(sum(pw * ph for pw, ph in sizes))
            worst += 2 * mcus_y * stride
        planes = torch.empty((n_planes,), dtype=torch.uint8, device=dev)
        seg = torch.empty((n_seg,), dtype=torch.uint8, device=dev)
        described = []
        for i, (address, pitch, pstride), (mcus_x, mcus_y, sizes, stride, p_at, s_at) in zip(group, inputs, grids):
            H, W = shapes[i][:2]
            described.append((address, pitch, pstride, W, H, [(planes.data_ptr() + a0, pw, pw, ph, h, v) for a0, (pw, ph), (h, v) in zip(p_at, sizes, sampling)],
                              seg.data_ptr() + s_at, stride))
        plan = BatchPlan(described, layout, tabs)
        try:
            counts = torch.empty((2, plan.n_rows), dtype=torch.int32, device=dev)
            off = torch.empty((plan.n_rows + 1,), dtype=torch.int64, device=dev)
            out = torch.empty((capacity,), dtype=torch.uint8, device=dev)
            image = torch.empty((plan.image_bytes,), dtype=torch.uint8, device=dev)  # the caching allocator's blocks are 512-byte aligned
            image.copy_(torch.from_numpy(plan.bind(image, counts[0], counts[1])))
            plan.planes(stream)
            plan.scan(stream)
            plan.pack(out, off, stream)
            offsets = off.cpu().numpy()  # the one copy that waits for the scans: it is ordered on the call's stream
            if int(offsets[-1]) > out.numel():  # the segments are there: only the packing runs again, into the worst case
                out = torch.empty((worst,), dtype=torch.uint8, device=dev)
                plan.pack(out, off, stream)
                offsets = off.cpu().numpy()
            first = plan.first_row
        finally:
            plan.close()
        scans = out[:int(offsets[-1])].cpu().numpy()
        luma, chroma = tabs
        for k, (i, (mcus_x, _, _, _, _, _)) in enumerate(zip(group, grids)):
            H, W = shapes[i][:2]
            scan = scans[int(offsets[first[k]]):int(offsets[first[k + 1]])]
            results[i] = jfif.write_jpeg([dict(qtable=luma), dict(qtable=chroma), dict(qtable=chroma)], W, H, specs=None, sampling=sampling,
                                         interleaved=dict(scan=scan, mcus_per_row=mcus_x))
