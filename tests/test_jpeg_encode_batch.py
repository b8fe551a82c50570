"""A batch of images encoded to JPEG files in three launches: libmdct_jpegenc_batch.so (include/mdct_jpegenc_batch.h,
simd_dct_amd/_jpegenc_batch_lib.py) and jpeg_encode.encode_jpeg_batch.

The contract is exact: file i is, byte for byte, what encode_jpeg(images[i], quality, subsampling, layout, interleaved=True) returns,
the path tests/test_jpeg_encode_interleaved.py holds to the CPU checker, the oracle and tests/jpeg_scan_encoder.py.  Every comparison
here is bytes ==; the small files are also held to that CPU expectation directly (expected / _check_file of that module).

CPU: the planning entry point (prefixes, the packer's row table, the out-of-range queries; the single-image libraries' refusals in
their words, with the image's index), header and binding name for name, the code object's ten kernels, encode_jpeg_batch's argument
checks and the empty batch.
GPU: the mixed batch (the shapes are listed at images()) at every subsampling and two qualities, as listed and reversed; CHW; a 4-D
tensor; the launch count, which does not depend on the number of images; grey images at their place; the second packing pass; the
three entry points driven directly over buffers with canaries, against scan_rows + jpeg_pack_rows on each image alone; a call on a
stream that is not the current one, behind a stall."""
import functools
import io
import os

import numpy as np
import pytest

from simd_dct_amd import _jpegenc_batch_lib, _jpegenc_lib, _jpegenc_scan_lib, api, synth
from simd_dct_amd import jpeg_encode as J
from test_jpeg_encode_interleaved import _check_file, expected

Image = pytest.importorskip("PIL.Image")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUBS = ["4:4:4", "4:2:2", "4:2:0"]
KIND = {"4:4:4": 1, "4:2:2": 2, "4:2:0": 3}
HV = {"4:4:4": "1, 1", "4:2:2": "2, 1", "4:2:0": "2, 2"}
PACK = "k_batch_pack"
BATCH_KERNELS = {PACK} | {f"k_batch_rgb_ycc<{k}, {p}>" for k in (1, 2, 3) for p in ("false", "true")} | {f"k_batch_scan_rows<{hv}>" for hv in HV.values()}
PACK_WINDOW = 16384  # kPackWindow of csrc/pack_rows.h


def kernels_of(sub, layout="HWC"):
    """the three instantiations a batch of this subsampling and layout launches"""
    return {f"k_batch_rgb_ycc<{KIND[sub]}, {'true' if layout == 'CHW' else 'false'}>", f"k_batch_scan_rows<{HV[sub]}>", PACK}


def test_pack_window_is_the_sources():
    src = open(os.path.join(ROOT, "simd_dct_amd", "csrc", "pack_rows.h")).read()
    assert "kPackBytesPerThread = 64;" in src and "kPackWindow = 256 * kPackBytesPerThread;" in src and PACK_WINDOW == 256 * 64


# ------------------------------------------------------------------------------------------ CPU: the plan
A = 1 << 40  # addresses far apart; nothing is dereferenced


def described(k, W, H, sub="4:2:0", **change):
    """image k of a plan at made-up addresses: (address, pitch, plane stride, W, H, planes, segment address, seg_stride)"""
    sampling = J.sampling_of(sub)
    mx, my, sizes = J.mcu_grid(max(W, 1), H, sampling)
    base = A + (k << 34)
    d = dict(address=base, pitch=3 * W, stride=0, W=W, H=H,
             planes=[(base + ((c + 1) << 30), pw, pw, ph, h, v) for c, ((pw, ph), (h, v)) in enumerate(zip(sizes, sampling))],
             seg=base + (8 << 30), seg_stride=J.scan_seg_stride(mx, sampling))
    d.update(change)
    return tuple(d[n] for n in ("address", "pitch", "stride", "W", "H", "planes", "seg", "seg_stride"))


def test_plan_of_three_images_prefixes_and_row_table():
    # 1, 9 and 3 MCU rows at 4:2:0; the third is two front tiles wide
    p = J.BatchPlan([described(0, 16, 16), described(1, 40, 136), described(2, 1040, 48)], "HWC", J.quality_tables(75))
    assert p.n_images == 3 and p.n_rows == 13
    assert p.first_row == [0, 1, 10, 13]
    # tiles of 1024 luma columns x 4 row groups (4:2:0: a row group is two luma rows): 1 x 2, 1 x 18, 2 x 6
    assert p.first_tile == [0, 2, 20, 32] and p.n_tiles == 32
    table = p.row_table()
    assert [t[0] for t in table] == [0] + [1] * 9 + [2] * 3
    assert [t[1] for t in table] == [1] + [0] * 8 + [1] + [0, 0, 1]  # the last row of each image: no marker follows
    assert [t[2] for t in table] == [0] + [0, 1, 2, 3, 4, 5, 6, 7, 0] + [0, 1, 2]  # RSTm restarts with every image and wraps mod 8
    lib = _jpegenc_batch_lib.load()
    out = _jpegenc_batch_lib.OUT_OF_RANGE
    assert lib.mdct_jpegenc_batch_first_row(p.handle, 4) == out and lib.mdct_jpegenc_batch_first_tile(p.handle, 4) == out
    assert lib.mdct_jpegenc_batch_row_image(p.handle, 13) == out and lib.mdct_jpegenc_batch_row_last(p.handle, 13) == out
    assert lib.mdct_jpegenc_batch_row_marker(p.handle, 13) == out
    assert lib.mdct_jpegenc_batch_rows(None) == 0 and lib.mdct_jpegenc_batch_image_bytes(None) == 0
    assert p.image_bytes >= 13 * 8 + 2 * 4 * 4
    p.close()


def _single_image_message(d, layout="HWC"):
    """what mdct_jpegenc_from_rgb, then mdct_jpegenc_scan_rows, say to the same image (both refuse on the host, before any launch)"""
    address, pitch, stride, W, H, planes, seg, seg_stride = d
    arr = (_jpegenc_lib.Plane * 3)(*[_jpegenc_lib.Plane(*p) for p in planes])
    lib = _jpegenc_lib.load()
    if lib.mdct_jpegenc_from_rgb(address, pitch, stride, W, H, _jpegenc_lib.RGB, J._LAYOUTS[layout], arr, 3, None) != 0:
        return lib.mdct_jpegenc_last_error().decode()
    raise AssertionError("mdct_jpegenc_from_rgb took it: only refusals are asked here")


def _scan_rows_message(d):
    address, pitch, stride, W, H, planes, seg, seg_stride = d
    arr = (_jpegenc_scan_lib.Plane * 3)(*[_jpegenc_scan_lib.Plane(*p) for p in planes])
    tabs = [np.asarray(t, dtype=np.float32) for t in J.quality_tables(75)]
    lib = _jpegenc_scan_lib.load()
    rc = lib.mdct_jpegenc_scan_rows(arr, 3, tabs[0].ctypes.data, tabs[1].ctypes.data, 0, 1, seg, seg_stride, 1 << 50, 1 << 51, None)
    assert rc == 1
    return lib.mdct_jpegenc_scan_last_error().decode()


@pytest.mark.parametrize("what", ["pitch below the row bytes", "a 0 x N image", "a plane overlapping the input", "seg_stride below the minimum",
                                  "seg_stride not a multiple of 4"])
def test_plan_refuses_what_the_single_image_libraries_refuse_in_their_words(what):
    good = described(1, 40, 24)
    if what == "pitch below the row bytes":
        bad = described(1, 40, 24, pitch=119)
        said = _single_image_message(bad)
        assert "pitch" in said
    elif what == "a 0 x N image":
        bad = described(1, 0, 24)
        said = _single_image_message(bad)
        assert "0x24" in said
    elif what == "a plane overlapping the input":
        planes = list(good[5])
        planes[1] = (good[0] + 16,) + planes[1][1:]
        bad = described(1, 40, 24, planes=planes)
        said = _single_image_message(bad)
        assert "overlaps the input" in said
    elif what == "seg_stride below the minimum":
        bad = described(1, 40, 24, seg_stride=good[7] - 4)
        said = _scan_rows_message(bad)
    else:
        bad = described(1, 40, 24, seg_stride=good[7] + 2)
        said = _scan_rows_message(bad)
    assert said
    with pytest.raises(api.MdctError) as e:
        J.BatchPlan([described(0, 16, 16), bad, described(2, 16, 16)], "HWC", J.quality_tables(75))
    assert e.value.image == 1 and str(e.value).endswith(said), (str(e.value), said)


def test_plan_refuses_more_than_16384_rows():
    tall = [described(k, 8, 65535, "4:4:4") for k in range(2)]  # 8192 MCU rows each
    p = J.BatchPlan(tall, "HWC", J.quality_tables(75))
    assert p.n_rows == 16384 == _jpegenc_batch_lib.MAX_ROWS
    p.close()
    with pytest.raises(api.MdctError, match="more than 16384 MCU rows") as e:
        J.BatchPlan(tall + [described(2, 8, 8, "4:4:4")], "HWC", J.quality_tables(75))
    assert e.value.image is None


def test_plan_refuses_two_subsamplings_in_one_batch():
    with pytest.raises(api.MdctError, match="one subsampling per batch") as e:
        J.BatchPlan([described(0, 16, 16), described(1, 16, 16, "4:2:2")], "HWC", J.quality_tables(75))
    assert e.value.image == 1


def test_code_object_holds_the_ten_kernels():
    from test_kernel_coverage import code_object_kernels
    names, n_objects = code_object_kernels(lib=_jpegenc_batch_lib.LIB_PATH)
    assert n_objects == 1 and names == BATCH_KERNELS and len(BATCH_KERNELS) == 10, sorted(names ^ BATCH_KERNELS)


def test_an_empty_batch_is_an_empty_list():
    assert J.encode_jpeg_batch([]) == []
    assert J.encode_jpeg_batch((), quality=90, subsampling="4:4:4", layout="CHW") == []


def test_bad_arguments_are_value_errors_before_any_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("device work before the arguments were checked")

    encode_jpeg = J.encode_jpeg  # (refuses these before any device work itself: test_jpeg_encode_interleaved.py)
    monkeypatch.setattr(J, "_encode_group", no_device)
    monkeypatch.setattr(J, "BatchPlan", no_device)
    monkeypatch.setattr(J, "encode_jpeg", no_device)
    good = np.zeros((16, 16, 3), dtype=np.uint8)
    for kw in (dict(quality=0), dict(quality=101), dict(quality=7.5), dict(quality=True), dict(subsampling="4:1:1"), dict(subsampling=None), dict(layout="HCW")):
        with pytest.raises(ValueError) as e:
            J.encode_jpeg_batch([good, good], **kw)
        assert e.value.file == 0, kw
        with pytest.raises(ValueError):
            J.encode_jpeg_batch([], **kw)
        want = None
        try:
            encode_jpeg(good, interleaved=True, **kw)
        except ValueError as single:
            want = str(single)
        assert str(e.value) == want, kw
    for bad in (good.astype(np.int16), np.zeros((16, 16, 4), np.uint8), np.zeros((2, 16, 16, 3), np.uint8), np.zeros((16,), np.uint8), np.zeros((0, 16), np.uint8),
                np.zeros((16, 65536), np.uint8), [[1, 2], [3, 4]]):
        with pytest.raises(ValueError) as e:
            J.encode_jpeg_batch([good, good[:, :, 0], bad, good])
        assert e.value.file == 2
        with pytest.raises(ValueError) as single:
            encode_jpeg(bad, interleaved=True)
        assert str(e.value) == str(single.value)
    with pytest.raises(ValueError) as e:
        J.encode_jpeg_batch([good], layout="CHW")  # [16, 16, 3] is no CHW image
    assert e.value.file == 0
    with pytest.raises(ValueError):
        J.encode_jpeg_batch(np.zeros((16, 16, 3), np.uint8))  # one image where a sequence is asked: not a 4-D array
    with pytest.raises(ValueError) as e:
        J.encode_jpeg_batch(np.zeros((2, 16, 16, 3), np.int8))
    assert e.value.file == 0


# ------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    torch.cuda.set_device(0)
    api.init(0)
    return torch


CHECKED = (0, 1, 2, 3, 5)  # the images held to the CPU expectation as well: up to 40 x 24, and 528 x 8
NOISE = 6


@functools.lru_cache(None)
def host_images():
    """the mixed batch, as numpy [H, W, 3]:
      0  1 x 1: the smallest image                      1  16 x 16: one 4:2:0 MCU, on the front kernel's vector path
      2  17 x 9: partial MCUs both ways, scalar path    3  40 x 24
      4  24 x 136: 17 / 17 / 9 MCU rows at 4:4:4 / 4:2:2 / 4:2:0, not first in the batch: RSTm wraps mod 8 inside it
      5  528 x 8: 66 / 33 / 33 MCUs, one past a chunk boundary of the scan coder (64 / 32 / 32 MCUs per chunk)
      6  1040 x 16 noise: two front workgroups across, three scan chunks, and at quality 100 segments beyond one packing window
      7  97 x 33, handed over as the device view big[1:, 3:] of a 34 x 100 image: odd pitch and base, no aligned row
      8  33 x 20, handed over as a host numpy array among device tensors"""
    rng = np.random.default_rng(20261019)
    sizes = [(1, 1), (16, 16), (17, 9), (40, 24), (24, 136), (528, 8), (1040, 16), (100, 34), (33, 20)]
    out = []
    for k, (W, H) in enumerate(sizes):
        if k == NOISE:
            out.append(rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
        else:
            out.append(np.stack([synth.plane_u8_np(W, H, "photo", seed=60 + 3 * k + c) for c in range(3)], axis=-1))
    return tuple(out)


_device = {}


def images(torch, layout="HWC"):
    """-> (what is handed to encode_jpeg_batch, the same images as contiguous numpy arrays in that layout)"""
    if layout not in _device:
        given, plain = [], []
        for k, h in enumerate(host_images()):
            if layout == "CHW":
                h = np.moveaxis(h, -1, 0).copy()  # (a copy has the strides of its shape; a 1 x 1 image moved is "contiguous" with any)
            if k == 7:
                big = torch.from_numpy(h).cuda()
                view = big[1:, 3:] if layout == "HWC" else big[:, 1:, 3:]
                assert view.data_ptr() % 2 == 1 and not view.is_contiguous()
                given.append(view)
                plain.append(np.ascontiguousarray(h[1:, 3:] if layout == "HWC" else h[:, 1:, 3:]))
            elif k == 8:
                given.append(h)
                plain.append(h)
            else:
                given.append(torch.from_numpy(h).cuda())
                plain.append(h)
        torch.cuda.synchronize()
        _device[layout] = (given, plain)
    return _device[layout]


_alone = {}


def alone(torch, key, image, **kw):
    """encode_jpeg(image, interleaved=True) on the image alone, computed once per image and form"""
    key = (key, tuple(sorted(kw.items())))
    if key not in _alone:
        _alone[key] = J.encode_jpeg(image, interleaved=True, **kw)
        torch.cuda.synchronize()
    return _alone[key]


@functools.lru_cache(None)
def cpu_expectation(k, sub, q, layout="HWC"):
    h = host_images()[k]
    return expected(np.ascontiguousarray(np.moveaxis(h, -1, 0)) if layout == "CHW" else h, sub, q, layout)


def check_batch(torch, order, sub, q, layout="HWC", cpu=True):
    given, plain = images(torch, layout)
    got = J.encode_jpeg_batch([given[k] for k in order], quality=q, subsampling=sub, layout=layout)
    torch.cuda.synchronize()
    assert len(got) == len(order) and all(isinstance(f, bytes) for f in got)
    for k, f in zip(order, got):
        assert f == alone(torch, (k, layout), given[k], quality=q, subsampling=sub, layout=layout), (k, sub, q)
        if cpu and k in CHECKED:
            _check_file(f, plain[k], sub, q, layout)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["as listed", "reversed"])
@pytest.mark.parametrize("q", [50, 100])
@pytest.mark.parametrize("sub", SUBS)
def test_the_mixed_batch(gpu, sub, q, order):
    from simd_dct_amd import jpeg_decode as D
    torch = gpu
    ks = list(range(len(host_images())))
    if q == 100:  # the noise image's rows are longer than one packing window: from the CPU expectation, not from the code under test
        rows = cpu_expectation(NOISE, sub, 100)[1]
        assert max(len(r) for r in rows) > PACK_WINDOW, (sub, [len(r) for r in rows])
    got = check_batch(torch, ks if order == "as listed" else ks[::-1], sub, q, cpu=order == "as listed")
    if order == "as listed":
        plain = images(torch)[1]
        for k, f in enumerate(got):
            H, W = plain[k].shape[:2]
            rgb = D.decode_jpeg(f, mode="RGB")
            assert tuple(rgb.shape) == (H, W, 3), k
            im = Image.open(io.BytesIO(f))
            im.load()
            assert im.size == (W, H) and im.mode == "RGB", k
        torch.cuda.synchronize()


@pytest.mark.gpu
def test_chw_layout(gpu):
    check_batch(gpu, list(range(len(host_images()))), "4:2:0", 50, layout="CHW")


@pytest.mark.gpu
def test_a_4d_tensor_is_the_sequence_of_its_slices(gpu):
    torch = gpu
    host = np.stack([np.stack([synth.plane_u8_np(40, 24, "photo", seed=90 + 3 * k + c) for c in range(3)], axis=-1) for k in range(5)])
    assert host.shape == (5, 24, 40, 3)
    dev = torch.from_numpy(host).cuda()
    want = [J.encode_jpeg(dev[k], interleaved=True) for k in range(5)]
    assert J.encode_jpeg_batch(dev) == want
    assert J.encode_jpeg_batch(host) == want
    assert J.encode_jpeg_batch([dev[k] for k in range(5)]) == want
    assert len(set(want)) == 5


def _ran(torch):
    torch.cuda.synchronize()
    return api.kernel_counts()


SINGLE = ("k_rgb_ycc", "k_scan_rows", "k_pack_")


@pytest.mark.gpu
@pytest.mark.parametrize("sub", SUBS)
def test_three_launches_whatever_the_number_of_images(gpu, sub):
    torch = gpu
    given, _ = images(torch)
    for n in (2, 9):
        api.kernel_counts_reset()
        got = J.encode_jpeg_batch(given[:n], quality=50, subsampling=sub)
        ran = _ran(torch)
        assert {k: v for k, v in ran.items() if k.startswith("k_batch")} == {k: 1 for k in kernels_of(sub)}, (n, ran)
        assert not any(k.startswith(SINGLE) for k in ran), (n, ran)
        for k, f in enumerate(got):
            assert f == alone(torch, (k, "HWC"), given[k], quality=50, subsampling=sub, layout="HWC")


@pytest.mark.gpu
def test_grey_images_at_their_place(gpu):
    torch = gpu
    given, _ = images(torch)
    grey_dev = synth.plane_u8_torch(33, 31, "photo", seed=7)
    grey_host = synth.plane_u8_np(64, 40, "photo", seed=8)
    batch = [given[3], grey_dev, given[2], grey_host, given[8]]
    api.kernel_counts_reset()
    got = J.encode_jpeg_batch(batch, quality=50)
    ran = _ran(torch)
    assert {k: v for k, v in ran.items() if k.startswith("k_batch")} == {k: 1 for k in kernels_of("4:2:0")}, ran
    assert got[1] == J.encode_jpeg(grey_dev, quality=50) and got[3] == J.encode_jpeg(grey_host, quality=50)
    for at, k in ((0, 3), (2, 2), (4, 8)):
        assert got[at] == alone(torch, (k, "HWC"), given[k], quality=50, subsampling="4:2:0", layout="HWC")
    api.kernel_counts_reset()
    only = J.encode_jpeg_batch([grey_dev, grey_host], quality=50)
    ran = _ran(torch)
    assert not any(k.startswith("k_batch") for k in ran), ran
    assert only == [got[1], got[3]]


@pytest.mark.gpu
def test_scans_that_do_not_fit_are_packed_again(gpu, monkeypatch):
    torch = gpu
    given, _ = images(torch)
    batch = [given[k] for k in (3, 6, 2)]
    want = [alone(torch, (k, "HWC"), given[k], quality=100, subsampling="4:2:0", layout="HWC") for k in (3, 6, 2)]
    monkeypatch.setattr(J, "_first_capacity", lambda pixels: 16)
    api.kernel_counts_reset()
    got = J.encode_jpeg_batch(batch, quality=100)
    ran = _ran(torch)
    front, scan, pack = sorted(kernels_of("4:2:0"), key=lambda k: ("rgb" not in k, "scan" not in k))
    assert {k: v for k, v in ran.items() if k.startswith("k_batch")} == {front: 1, scan: 1, pack: 2}, ran
    assert got == want


CANARY = 0xA5


@pytest.mark.gpu
@pytest.mark.parametrize("sub", SUBS)
def test_c_level_canaries_and_every_image_as_alone(gpu, sub):
    """the three entry points over buffers of the test's own: gaps of canary bytes between and around the planes, between the images'
    segment ranges, an entry either side of seg_bytes, ff_counts and row_offsets, bytes before and after out; every image's planes,
    segments, counts and row offsets equal what to_planes + scan_rows + jpeg_pack_rows give on that image alone"""
    torch = gpu
    given, _ = images(torch)
    sampling = J.sampling_of(sub)
    tabs = J.quality_tables(90)
    batch = [given[k] for k in (3, 4, 7)]
    gap = 80
    grids, n_planes, n_seg = [], gap, gap
    for im in batch:
        H, W = im.shape[:2]
        mx, my, sizes = J.mcu_grid(W, H, sampling)
        stride = J.scan_seg_stride(mx, sampling)
        p_at = []
        for pw, ph in sizes:
            p_at.append(n_planes)
            n_planes += pw * ph + gap
        grids.append((mx, my, sizes, stride, p_at, n_seg))
        n_seg += my * stride + gap
    planes = torch.full((n_planes,), CANARY, dtype=torch.uint8, device="cuda")
    seg = torch.full((n_seg,), CANARY, dtype=torch.uint8, device="cuda")
    desc = [(im.data_ptr(), im.stride(0), 0, im.shape[1], im.shape[0],
             [(planes.data_ptr() + a0, pw, pw, ph, h, v) for a0, (pw, ph), (h, v) in zip(p_at, sizes, sampling)], seg.data_ptr() + s_at, stride)
            for im, (mx, my, sizes, stride, p_at, s_at) in zip(batch, grids)]
    assert all(d[6] % 4 == 0 for d in desc)
    plan = J.BatchPlan(desc, "HWC", tabs)
    rows, first = plan.n_rows, plan.first_row
    assert first == [0] + list(np.cumsum([g[1] for g in grids]))
    counts = torch.full((2, rows + 2), -7, dtype=torch.int32, device="cuda")
    off = torch.full((rows + 3,), -7, dtype=torch.int64, device="cuda")
    capacity = 2 * sum(g[1] * g[3] for g in grids)
    out = torch.full((64 + capacity + 64,), CANARY, dtype=torch.uint8, device="cuda")
    image = torch.empty(plan.image_bytes, dtype=torch.uint8, device="cuda")
    image.copy_(torch.from_numpy(plan.bind(image, counts[0, 1:-1], counts[1, 1:-1])))
    api.kernel_counts_reset()
    plan.planes()
    plan.scan()
    plan.pack(out[64:64 + capacity], off[1:-1])
    ran = _ran(torch)
    assert {k: v for k, v in ran.items() if k.startswith("k_batch")} == {k: 1 for k in kernels_of(sub)}, ran
    plan.close()
    P, S, C, O, OUT = planes.cpu().numpy(), seg.cpu().numpy(), counts.cpu().numpy(), off.cpu().numpy(), out.cpu().numpy()
    assert (C[:, 0] == -7).all() and (C[:, -1] == -7).all() and O[0] == -7 and O[-1] == -7
    total = int(O[1 + rows])
    assert 0 < total <= capacity and (OUT[:64] == CANARY).all() and (OUT[64 + total:] == CANARY).all()
    covered = np.zeros(n_planes, dtype=bool)
    seg_covered = np.zeros(n_seg, dtype=bool)
    for k, (im, (mx, my, sizes, stride, p_at, s_at)) in enumerate(zip(batch, grids)):
        lone = J.to_planes(im, sub, "HWC", planes=[torch.empty((ph, pw), dtype=torch.uint8, device="cuda") for pw, ph in sizes])
        lseg = torch.full((my * stride,), CANARY, dtype=torch.uint8, device="cuda")
        lcounts = torch.empty((2, my), dtype=torch.int32, device="cuda")
        J.scan_rows(lone, sampling, tabs, lseg, lcounts[0], lcounts[1], seg_stride=stride)
        lout = torch.empty((2 * my * stride,), dtype=torch.uint8, device="cuda")
        loff = torch.empty((my + 1,), dtype=torch.int64, device="cuda")
        api.jpeg_pack_rows(lseg, lcounts[0], stride, my, lout, loff, ff_counts=lcounts[1])
        torch.cuda.synchronize()
        for a0, (pw, ph), lp in zip(p_at, sizes, lone):
            assert np.array_equal(P[a0:a0 + pw * ph].reshape(ph, pw), lp.cpu().numpy()), k
            covered[a0:a0 + pw * ph] = True
        assert np.array_equal(S[s_at:s_at + my * stride], lseg.cpu().numpy()), k  # the segments, and the canaries after each of them
        seg_covered[s_at:s_at + my * stride] = True
        assert np.array_equal(C[:, 1 + first[k]:1 + first[k + 1]], lcounts.cpu().numpy()), k
        mine = O[1 + first[k]:1 + first[k + 1] + 1]
        lo = loff.cpu().numpy()
        assert np.array_equal(mine - mine[0], lo), k
        n = int(lo[-1])
        assert OUT[64 + int(mine[0]):64 + int(mine[-1])].tobytes() == lout[:n].cpu().numpy().tobytes(), k
    assert (P[~covered] == CANARY).all() and (S[~seg_covered] == CANARY).all()


@pytest.mark.gpu
@pytest.mark.parametrize("arrangement,fill", [("A", 0), ("A", 0x7F7F7F7F), ("B", None), ("D", None)], ids=["A-stale-0", "A-stale-7f", "B", "D"])
@pytest.mark.parametrize("name", ["encode-batch-mixed", "encode-batch-device"])
def test_a_stalled_stream_that_is_not_the_current_one(gpu, name, arrangement, fill):
    """the arrangements A (with both stale fills), B and D of tests/test_jpeg_streams.py on encode_jpeg_batch: a mixed batch of device
    tensors, a host image and a grey image, and a batch of device tensors only"""
    import test_jpeg_streams as S
    torch = gpu
    if name not in S.CASES:
        given, _ = images(torch)
        if name == "encode-batch-mixed":
            batch = [given[3], given[8], synth.plane_u8_torch(33, 31, "photo", seed=7), given[7], given[4]]
        else:
            batch = [given[k] for k in (1, 3, 4, 5, 7)]
        S.CASES[name] = S.Case(name, lambda torch: lambda st: J.encode_jpeg_batch(batch, stream=st), tally=(PACK, 1))
    S.run(torch, name, arrangement, fill=fill)
