"""8-bit RGB or grey image -> baseline JPEG file on the GPU (libmdct_jpegenc.so, include/mdct_jpegenc.h; the scan kernels of
include/mdct.h).  The mirror of jpeg_decode.decode_jpeg.

encode_jpeg runs one launch of mdct_jpegenc_from_rgb (RGB -> YCbCr, chroma downsampling and padding to the block grid, as
libjpeg-turbo's compressor does them), then one restart-marked scan per component (mdct_fwd_u8_huffman_rows and
mdct_jpeg_pack_rows_counted: pixels -> stuffed scan with RSTm between the block rows, Annex K tables), copies back the scans' lengths and bytes and writes the marker segments (jfif.write_jpeg).
With interleaved=True a colour image becomes ONE scan whose MCUs interleave the components, the form every other encoder writes
(libmdct_jpegenc_scan.so, include/mdct_jpegenc_scan.h: mdct_jpegenc_scan_rows codes the three planes, padded to the MCU grid, in
MCU order; one packing launch and one read-back instead of three).
torch is used for device memory and streams only.
"""
import numpy as np

from . import _jpegenc_lib, _jpegenc_scan_lib, api, jfif
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


def last_error():
    return _jpegenc_lib.load().mdct_jpegenc_last_error().decode()


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
    if grey:
        ok = image.stride(1) == 1
        pitch, stride = image.stride(0), 0
    elif layout == "HWC":
        ok = image.stride(2) == 1 and image.stride(1) == 3
        pitch, stride = image.stride(0), 0
    else:
        ok = image.stride(2) == 1
        pitch, stride = image.stride(1), image.stride(0)
    if not ok:
        raise ValueError("image: contiguous innermost dimension (HWC: 3 contiguous bytes per pixel)")
    if planes is None:
        planes = [torch.empty((ph, pw), dtype=torch.uint8, device=image.device) for _, _, pw, ph in sizes]
    if len(planes) != len(sampling):
        raise ValueError(f"{len(planes)} planes for {len(sampling)} components")
    arr = (_jpegenc_lib.Plane * len(planes))()
    for k, (p, (h, v)) in enumerate(zip(planes, sampling)):
        if p.dtype != torch.uint8 or p.dim() != 2 or p.stride(1) != 1 or not p.is_cuda:
            raise ValueError(f"plane {k}: uint8 device tensor [rows, columns] with contiguous columns")
        arr[k] = _jpegenc_lib.Plane(p.data_ptr(), p.stride(0), p.shape[1], p.shape[0], h, v)
    colour = _jpegenc_lib.GREY if grey else _jpegenc_lib.RGB
    rc = _jpegenc_lib.load().mdct_jpegenc_from_rgb(image.data_ptr(), pitch, stride, W, H, colour, _LAYOUTS[layout], arr, len(planes),
                                                   _stream(stream))
    if rc != 0:
        raise api.MdctError(f"mdct_jpegenc status {rc}: {last_error()}")
    return planes


def scan_seg_stride(mcus_x, sampling):
    """smallest legal seg_stride of scan_rows (mdct_jpegenc_scan_seg_stride)"""
    return int(_jpegenc_scan_lib.load().mdct_jpegenc_scan_seg_stride(mcus_x, sum(h * v for h, v in sampling)))


def scan_rows(planes, sampling, luts, out, seg_bytes, ff_counts, seg_stride=None, my0=0, my1=None, stream=None, check=True):
    """mdct_jpegenc_scan_rows on device tensors.  planes: Y, Cb, Cr, uint8 [rows, columns] with contiguous columns, each exactly its size
    on the MCU grid (mcu_grid); sampling: [(h, v)] per component; luts: (luma, chroma), 64 numbers each in natural order.  out: uint8,
    one segment per MCU row seg_stride apart (default: scan_seg_stride); seg_bytes / ff_counts: int32 per MCU row.  MCU rows my0 .. my1
    (default: all) are coded.  Returns the status (raises unless check=False)."""
    arr = (_jpegenc_scan_lib.Plane * max(1, len(planes)))()
    for k, (p, (h, v)) in enumerate(zip(planes, sampling)):
        if p.dim() != 2 or p.stride(1) != 1 or p.element_size() != 1:
            raise ValueError(f"plane {k}: uint8 tensor [rows, columns] with contiguous columns")
        arr[k] = _jpegenc_scan_lib.Plane(p.data_ptr(), p.stride(0), p.shape[1], p.shape[0], h, v)
    tabs = [np.ascontiguousarray(np.asarray(t, dtype=np.float32).reshape(64)) for t in luts]
    mcus_x, mcus_y = planes[-1].shape[1] // 8, planes[-1].shape[0] // 8
    if seg_stride is None:
        seg_stride = scan_seg_stride(mcus_x, sampling)
    lib = _jpegenc_scan_lib.load()
    rc = lib.mdct_jpegenc_scan_rows(arr, len(planes), tabs[0].ctypes.data, tabs[1].ctypes.data, my0, mcus_y if my1 is None else my1, out.data_ptr(), seg_stride,
                                    seg_bytes.data_ptr(), ff_counts.data_ptr(), _stream(stream))
    if check and rc != 0:
        raise api.MdctError(f"mdct_jpegenc_scan status {rc}: {lib.mdct_jpegenc_scan_last_error().decode()}")
    return rc


def _first_capacity(pixels):
    """bytes of the first scan buffer: ~0.2 bytes per pixel in practice; a scan that does not fit is coded again into its worst case"""
    return pixels + 4096


def _encode_interleaved(torch, image, W, H, sampling, subsampling, layout, tabs, stream):
    """the colour image as one interleaved scan: front launch into planes on the MCU grid, scan_rows, the packing launch, one read-back"""
    dev = image.device
    mcus_x, mcus_y, sizes = mcu_grid(W, H, sampling)
    planes = to_planes(image, subsampling, layout, planes=[torch.empty((ph, pw), dtype=torch.uint8, device=dev) for pw, ph in sizes], stream=stream)
    stride = scan_seg_stride(mcus_x, sampling)
    seg = torch.empty((mcus_y * stride,), dtype=torch.uint8, device=dev)
    counts = torch.empty((2, mcus_y), dtype=torch.int32, device=dev)
    off = torch.empty((mcus_y + 1,), dtype=torch.int64, device=dev)
    scan_rows(planes, sampling, (tabs[0], tabs[1]), seg, counts[0], counts[1], seg_stride=stride, stream=stream)
    out = torch.empty((_first_capacity(sum(pw * ph for pw, ph in sizes)),), dtype=torch.uint8, device=dev)
    api.jpeg_pack_rows(seg, counts[0], stride, mcus_y, out, off, ff_counts=counts[1], stream=stream)
    end = int(off[-1].item())  # the one copy that waits for the scan
    if end > out.numel():  # the segments are there: only the packing runs again, into the worst case
        out = torch.empty((2 * mcus_y * stride,), dtype=torch.uint8, device=dev)
        api.jpeg_pack_rows(seg, counts[0], stride, mcus_y, out, off, ff_counts=counts[1], stream=stream)
        end = int(off[-1].item())
    return dict(scan=out[:end].cpu().numpy(), mcus_per_row=mcus_x)


class _Scan:
    """device buffers of one component's scan"""

    def __init__(self, torch, dev, pw, ph, capacity):
        rows = ph // 8
        self.stride = api.huffman_seg_stride(pw)
        self.seg = torch.empty((rows * self.stride,), dtype=torch.uint8, device=dev)
        self.out = torch.empty((capacity,), dtype=torch.uint8, device=dev)
        self.off = torch.empty((rows + 1,), dtype=torch.int64, device=dev)
        self.work = torch.zeros((rows + 2,), dtype=torch.int64, device=dev)  # the one-launch form's chain between the rows
        self.counts = torch.empty((2, rows), dtype=torch.int32, device=dev)  # the two-launch form's byte and 0xFF counts


def _run_scan(plane, pw, ph, lut, chroma, sc, two_launch, stream):
    if two_launch:
        api.fwd_u8_huffman_rows(plane, pw, ph, sc.seg, sc.counts[0], lut=lut, chroma=chroma, seg_stride=sc.stride, pitch=plane.stride(0),
                                ff_counts=sc.counts[1], stream=stream)
        api.jpeg_pack_rows(sc.seg, sc.counts[0], sc.stride, ph // 8, sc.out, sc.off, ff_counts=sc.counts[1], stream=stream)
    else:
        api.fwd_u8_jpeg_scan(plane, pw, ph, sc.seg, sc.work, sc.out, sc.off, lut=lut, chroma=chroma, seg_stride=sc.stride, pitch=plane.stride(0),
                             stream=stream)


def encode_jpeg(image, quality=75, subsampling="4:2:0", layout="HWC", device=None, stream=None, *, two_launch=True, interleaved=False):
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
    image has one component, whose scan is non-interleaved by definition: the argument changes nothing there."""
    import torch

    q = _quality(quality)
    if not isinstance(interleaved, (bool, np.bool_)):
        raise ValueError(f"interleaved {interleaved!r}: a bool")
    if isinstance(image, np.ndarray):
        if image.dtype != np.uint8:
            raise ValueError(f"image dtype {image.dtype}: uint8")
    elif not isinstance(image, torch.Tensor) or image.dtype != torch.uint8:
        raise ValueError("image: a uint8 numpy array or torch tensor")
    H, W, grey = _image_shape(image, layout)
    sampling = sampling_of(subsampling, grey)
    sizes = component_sizes(W, H, sampling)
    luma, chroma = quality_tables(q)
    dev = torch.device("cuda" if device is None else (f"cuda:{device}" if isinstance(device, int) else device))
    if isinstance(image, np.ndarray):
        image = torch.from_numpy(np.ascontiguousarray(image))
    if not image.is_cuda:
        image = image.to(dev)
    dev = image.device
    with torch.cuda.device(dev):
        if interleaved and not grey:
            scan = _encode_interleaved(torch, image, W, H, sampling, subsampling, layout, (luma, chroma), stream)
            return jfif.write_jpeg([dict(qtable=luma), dict(qtable=chroma), dict(qtable=chroma)], W, H, sampling=sampling, interleaved=scan)
        if grey and W % 8 == 0 and H % 8 == 0 and image.stride(1) == 1:
            planes = [image]
        else:
            planes = to_planes(image, subsampling, layout, stream=stream)
        tabs = [luma] + [chroma] * (len(planes) - 1)
        # ~0.2 bytes per pixel in practice; a scan that does not fit is coded again into its worst case
        scans = [_Scan(torch, dev, pw, ph, pw * ph + 4096) for _, _, pw, ph in sizes]
        for k, (p, (_, _, pw, ph), sc) in enumerate(zip(planes, sizes, scans)):
            _run_scan(p, pw, ph, tabs[k], k > 0, sc, two_launch, stream)
        ends = torch.stack([sc.off[-1] for sc in scans]).cpu().tolist()  # the one copy that waits for the scans
        for k, (p, (_, _, pw, ph), sc) in enumerate(zip(planes, sizes, scans)):
            if ends[k] < 0:  # UINT64_MAX read as int64
                raise api.MdctError(f"scan {k}: the one-launch coder reported a failure (row_offsets = UINT64_MAX)")
            if ends[k] > sc.out.numel():
                sc.out = torch.empty((2 * (ph // 8) * sc.stride,), dtype=torch.uint8, device=dev)
                _run_scan(p, pw, ph, tabs[k], k > 0, sc, two_launch, stream)
                ends[k] = int(sc.off[-1].item())
        comps = [dict(scan=sc.out[:n].cpu().numpy(), blocks_per_row=pw // 8, qtable=t) for sc, n, (_, _, pw, _), t in zip(scans, ends, sizes, tabs)]
    return jfif.write_jpeg(comps, W, H, sampling=sampling)
