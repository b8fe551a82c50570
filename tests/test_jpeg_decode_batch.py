"""A batch of JPEG files decoded in a fixed number of launches: libmdct_jpegdec_batch.so (include/mdct_jpegdec_batch.h,
simd_dct_amd/_jpegdec_batch_lib.py) and jpeg_decode.decode_jpeg_batch.

CPU: the planning entry point (prefixes, chunk table, totals; the single-scan library's refusals with its messages; equal Huffman
specifications stored once), header and binding name for name, decode_jpeg_batch's argument checks and the empty batch.
GPU: every comparison is exact -- torch.equal against decode_jpeg on the same file, np.array_equal of the coefficient planes against
the CPU checker (tests/jpeg_decode_checker.py).  One file; a mixed batch and the same batch reversed (the shapes are listed at
FILES); table sets; modes; files that fall back to decode_jpeg; a broken file between two intact ones; the two launching entry points
driven directly over planes and bytes with canaries around them, their offsets against mdct_jpegdec_index on each scan alone; the
launch count, which does not depend on the number of files; a decode on a stream that is not the current one, behind a stall."""
import functools
import io
import os
import re

import numpy as np
import pytest

import jpeg_decode_checker as C
import jpeg_hostile_cases as HC
import jpeg_scan_encoder as E
from simd_dct_amd import _jpegdec_batch_lib, api, jfif, synth
from simd_dct_amd import jpeg_decode as D

Image = pytest.importorskip("PIL.Image")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_KERNELS = {"k_batch_walk<false>", "k_batch_scan", "k_batch_walk<true>", "k_decode_batch"}
G, C420, C422, C444 = [(1, 1)], [(2, 2), (1, 1), (1, 1)], [(2, 1), (1, 1), (1, 1)], [(1, 1), (1, 1), (1, 1)]
INTERLEAVED = [(0, 0, 0), (1, 1, 1), (2, 1, 1)]


# ------------------------------------------------------------------------------------------ the files
def _planes(frame, seed, amp=15):
    """dense noise levels (every AC level non-zero, |level| <= amp) with DC steps of up to 200"""
    rng = np.random.default_rng(seed)
    out = []
    for rows, cols in E.plane_shapes(frame):
        p = rng.integers(1, amp + 1, size=(rows, cols)) * rng.choice([-1, 1], size=(rows, cols))
        p[::8, ::8] = rng.integers(-200, 201, size=(rows // 8, cols // 8))
        out.append(p.astype(np.int64))
    return out


def _written(width, height, comps, dri, seed, separate=False):
    """a file from the test-side encoder: one interleaved scan, or one scan per component"""
    frame = dict(width=width, height=height, comps=comps)
    if len(comps) == 1:
        scans = [dict(comps=[(0, 0, 0)], dri=dri)]
    elif separate:
        scans = [dict(comps=[(ci, min(ci, 1), min(ci, 1))], dri=dri) for ci in range(len(comps))]
    else:
        scans = [dict(comps=INTERLEAVED, dri=dri)]
    return E.encode_file(frame, scans, _planes(frame, seed), dict(E.ANNEX_K))[0]


def _pillow(img, **kw):
    buf = io.BytesIO()
    Image.fromarray(img, "L" if img.ndim == 2 else "RGB").save(buf, "JPEG", **kw)
    return buf.getvalue()


def index_chunk_floor():
    """the smallest chunk mdct_jpegdec_index cuts a scan by, read from its source"""
    src = open(os.path.join(ROOT, "simd_dct_amd", "csrc", "jpegdec_common.h")).read()
    return int(re.search(r"chunk = chunk < (\d+) \? \1 : chunk;", src).group(1))


@functools.lru_cache(None)
def FILES():
    """the mixed batch, every file on the batch path:
      0  grey 8 x 8, one interval                      1  17 x 9 4:2:0, one interleaved scan (padding blocks)
      2  17 x 17 4:2:0 interleaved: two MCU rows        3  40 x 24 4:4:4, three non-interleaved scans
      4  24 x 40 4:2:2                                  5  a restart interval of 1 MCU
      6  intervals of one and a half MCU rows, the last one short (16 MCUs: 6, 6, 4)
      7  96 x 8 with 12 one-MCU intervals, not first in the batch: RSTm wraps mod 8 inside it
      8  512 x 16 noise at quality 95, an interval per row: far more than 256 x 8 bytes each
      9  a scan of several intervals that is longer than one index chunk"""
    noise = synth.plane_u8_np(512, 16, "noise", seed=21)
    noise2 = synth.plane_u8_np(96, 64, "noise", seed=22)
    files = [
        _written(8, 8, G, 1, 1), _written(17, 9, C420, 1, 2), _written(17, 17, C420, 2, 3), _written(40, 24, C444, 5, 4, separate=True),
        _written(24, 40, C422, 2, 5), _written(32, 16, G, 1, 6), _written(32, 32, G, 6, 7), _written(96, 8, G, 1, 8),
        _pillow(noise, quality=95, restart_marker_rows=1), _pillow(noise2, quality=95, restart_marker_rows=1),
    ]
    info = [D.read_file(f) for f in files]
    assert all(i["sof"] == 0xC0 and all(s["restart_interval"] > 0 for s in i["scans"]) for i in info)
    assert [len(i["scans"]) for i in info] == [1, 1, 1, 3, 1, 1, 1, 1, 1, 1]
    sc8, sc9 = info[8]["scans"][0], info[9]["scans"][0]
    assert (sc8["end"] - sc8["start"]) / 2 > 256 * 8 * 1.5  # two intervals
    n9, len9 = 8, sc9["end"] - sc9["start"]
    assert len9 > max(index_chunk_floor(), -(-len9 // n9)) + 256  # more than one chunk: a chunk boundary inside the scan
    return tuple(files)


@functools.lru_cache(None)
def checker(data):
    """the CPU checker's coefficient planes of a file, computed once"""
    planes, statuses, _ = C.decode(data)
    assert all(s == C.OK for st in statuses for s in st)
    return planes


_alone = {}


def alone(torch, data, **kw):
    """decode_jpeg on the file alone, computed once per file and form: (outcome kind, value)"""
    key = (data, tuple(sorted(kw.items())))
    if key not in _alone:
        try:
            _alone[key] = ("ok", D.decode_jpeg(data, **kw))
        except (jfif.JpegFormatError, D.JpegDecodeError, api.MdctError) as e:
            _alone[key] = ("error", e)
        torch.cuda.synchronize()
    return _alone[key]


def same(torch, got, want):
    if isinstance(want, (tuple, list)):
        return isinstance(got, (tuple, list)) and len(got) == len(want) and all(same(torch, g, w) for g, w in zip(got, want))
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want)


def same_error(got, want):
    if type(got) is not type(want) or str(got) != str(want):
        return False
    if isinstance(want, D.JpegDecodeError):
        return got.scan == want.scan and np.array_equal(np.asarray(got.status), np.asarray(want.status))
    return True


def check_batch(torch, files, check_coefficients=True, **kw):
    got = D.decode_jpeg_batch(files, coefficients=True, **kw)
    torch.cuda.synchronize()
    assert len(got) == len(files)
    for i, (f, g) in enumerate(zip(files, got)):
        kind, want = alone(torch, f, coefficients=True, **kw)
        assert kind == "ok" and same(torch, g, want), i
        if check_coefficients:
            for q, w in zip(g[1], checker(f)):
                assert np.array_equal(q.cpu().numpy(), w), i
    return got


# ------------------------------------------------------------------------------------------ CPU
def _specs(chroma=False):
    return [E.ANNEX_K[(0, 1 if chroma else 0)], None, E.ANNEX_K[(1, 1 if chroma else 0)], None]


def _grey_desc(mx, my, ri, h=1, address=256, slots=(0, 2)):
    return D.scan_desc([(D._PlaneShape(my * 8, mx * 8, address), mx, my, h, 1, slots[0], slots[1])], mx, my, ri)


def test_plan_of_three_scans_prefixes_chunk_table_and_totals():
    floor = index_chunk_floor()
    # 1, 9 and 3 intervals; the second scan is nine chunks, the last of them short, the third is shorter than one chunk, the first is empty
    lens = [0, 9 * 4 * floor + 5, 10]
    scans, at = [], 0
    for (mx, my), n in zip(((4, 1), (4, 9), (4, 3)), lens):
        scans.append((_grey_desc(mx, my, 4), at, n, _specs()))
        at += n
    p = D.BatchPlan(scans, at)
    assert p.n_scans == 3 and p.n_intervals == 13 and p.n_offsets == 16
    assert p.first_interval == [0, 1, 10, 13]
    chunk1 = -(-(-(-lens[1] // 9)) // 256) * 256  # ceil(len / intervals), up to a multiple of the workgroup
    assert p.chunk_bytes == [floor, chunk1, floor]
    n1 = -(-lens[1] // chunk1)
    assert n1 == 9 and p.first_chunk == [0, 0, n1, n1 + 1] and p.n_chunks == n1 + 1
    assert p.chunk_scan() == [1] * n1 + [2]
    assert p.table_set == [0, 0, 0] and p.n_table_sets == 1
    lib = _jpegdec_batch_lib.load()
    assert lib.mdct_jpegdec_batch_first_interval(p.handle, 4) == _jpegdec_batch_lib.OUT_OF_RANGE
    assert lib.mdct_jpegdec_batch_chunk_scan(p.handle, p.n_chunks) == _jpegdec_batch_lib.OUT_OF_RANGE
    p.close()


def _single_scan_message(desc, specs):
    """what the single-scan library says to the same descriptor and tables (host functions only)"""
    if D.tables_check(specs) != 0:
        return D.last_error()
    try:
        D.n_intervals(desc)
    except api.MdctError:
        return D.last_error()
    return None


@pytest.mark.parametrize("what", ["restart interval 0", "h = 3", "unaligned plane", "over-subscribed table"])
def test_plan_refuses_what_the_single_scan_library_refuses_in_its_words(what):
    desc, specs = _grey_desc(4, 2, 4), _specs()
    if what == "restart interval 0":
        desc = _grey_desc(4, 2, 0)
    elif what == "h = 3":
        desc = _grey_desc(4, 2, 4, h=3)
    elif what == "unaligned plane":
        desc = _grey_desc(4, 2, 4, address=258)
    else:
        specs[0] = ([3] + [0] * 15, [0, 1, 2])  # three codes of one bit
    said = _single_scan_message(desc, specs)
    assert said
    good = (_grey_desc(4, 2, 4), 0, 10, _specs())
    with pytest.raises(api.MdctError) as e:
        D.BatchPlan([good, (desc, 10, 10, specs), good], 30)
    assert e.value.scan == 1 and str(e.value).endswith(said), (str(e.value), said)


def test_plan_refuses_an_empty_table_slot_in_the_single_scan_librarys_words():
    """mdct_jpegdec_decode's message (it needs a table handle, and so a device, to say it itself)"""
    src = open(os.path.join(ROOT, "simd_dct_amd", "csrc", "jpegdec_common.h")).read()
    assert 'fail(MDCT_INVALID_PARAMETER, "component %d uses an empty table slot (%d / %d)", c, q.dc_slot, q.ac_slot)' in src
    with pytest.raises(api.MdctError) as e:
        D.BatchPlan([(_grey_desc(4, 2, 4, slots=(1, 2)), 0, 10, _specs())], 10)
    assert e.value.scan == 0 and str(e.value).endswith("component 0 uses an empty table slot (1 / 2)")


def test_plan_refuses_bytes_outside_the_buffer():
    with pytest.raises(api.MdctError, match="outside the buffer"):
        D.BatchPlan([(_grey_desc(4, 2, 4), 5, 10, _specs())], 14)


def test_equal_table_specifications_share_one_set():
    a, b = _specs(), _specs(chroma=True)
    same_as_a = [([int(x) for x in s[0]], list(s[1])) if s else None for s in a]  # equal content, other objects
    scans = [(_grey_desc(4, 2, 4), 0, 10, sp) for sp in (a, b, same_as_a, b, a)]
    p = D.BatchPlan(scans, 10)
    assert p.table_set == [0, 1, 0, 1, 0] and p.n_table_sets == 2
    one_value_less = list(a)
    one_value_less[2] = (a[2][0][:15] + [a[2][0][15] - 1], a[2][1][:-1])
    q = D.BatchPlan([scans[0], (_grey_desc(4, 2, 4), 0, 10, one_value_less)], 10)
    assert q.table_set == [0, 1]


def test_code_object_holds_the_four_kernels():
    from test_kernel_coverage import code_object_kernels
    assert code_object_kernels(lib=_jpegdec_batch_lib.LIB_PATH)[0] == BATCH_KERNELS


def test_an_empty_batch_is_an_empty_list():
    assert D.decode_jpeg_batch([]) == []
    assert D.decode_jpeg_batch((), mode="RGB", layout="CHW", on_error="return") == []


@pytest.mark.parametrize("kw", [dict(mode="YCbCr"), dict(layout="NHWC"), dict(on_error="ignore")])
def test_bad_arguments_are_value_errors_before_any_device(kw):
    with pytest.raises(ValueError, match=list(kw)[0]):
        D.decode_jpeg_batch([FILES()[0]], **kw)
    with pytest.raises(ValueError, match=list(kw)[0]):
        D.decode_jpeg_batch([], **kw)


# ------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    torch.cuda.set_device(0)
    api.init(0)
    return torch


@pytest.mark.gpu
def test_a_batch_of_one_grey_block(gpu):
    check_batch(gpu, [FILES()[0]])


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["as listed", "reversed"])
def test_the_mixed_batch(gpu, order):
    files = list(FILES())
    check_batch(gpu, files if order == "as listed" else files[::-1])


@pytest.mark.gpu
def test_table_sets_side_by_side(gpu):
    img = synth.plane_u8_np(72, 40, "photo", seed=31)
    std = _pillow(img, quality=75, restart_marker_rows=1)
    opt = _pillow(img, quality=75, restart_marker_rows=1, optimize=True)
    assert D.read_file(std)["scans"][0]["huffman"] != D.read_file(opt)["scans"][0]["huffman"]
    check_batch(gpu, [std, opt, std, opt])
    got = check_batch(gpu, [opt] * 4)
    assert len({g[1][0].data_ptr() for g in got}) == 4  # four decodes, not one result four times


@pytest.mark.gpu
def test_modes_and_layouts(gpu):
    torch = gpu
    files = [FILES()[i] for i in (0, 1, 3, 4, 7)]  # grey files under mode="RGB" among them
    for kw in (dict(), dict(mode="RGB"), dict(mode="RGB", layout="CHW")):
        check_batch(torch, files, check_coefficients=False, **kw)
        got = D.decode_jpeg_batch(files, **kw)
        for f, g in zip(files, got):
            assert same(torch, g, alone(torch, f, **kw)[1])
    rgb = D.decode_jpeg_batch(files, mode="RGB", layout="CHW")
    assert [tuple(t.shape) for t in rgb] == [(3, 8, 8), (3, 9, 17), (3, 24, 40), (3, 40, 24), (3, 8, 96)]


@functools.lru_cache(None)
def _fallback_files():
    from simd_dct_amd import jpeg_encode as J
    img = np.stack([synth.plane_u8_np(40, 24, "photo", seed=41 + k) for k in range(3)], axis=-1)
    unmarked = _pillow(img, quality=75)
    import torch
    prog = J.encode_jpeg(torch.from_numpy(img).cuda(), progressive=True)
    assert D.read_file(unmarked)["scans"][0]["restart_interval"] == 0 and D.read_file(prog)["sof"] == 0xC2
    return unmarked, prog


@pytest.mark.gpu
def test_files_outside_the_batch_path_fall_back_to_decode_jpeg(gpu):
    unmarked, prog = _fallback_files()
    files = [FILES()[1], unmarked, FILES()[3], prog, FILES()[0]]
    for kw in (dict(), dict(mode="RGB")):
        check_batch(gpu, files, check_coefficients=False, **kw)
    api.kernel_counts_reset()
    check_batch(gpu, [unmarked, prog], check_coefficients=False)  # no batch-path file: none of the batch library's launches
    assert not BATCH_KERNELS & set(api.kernel_counts())


def _scan_of(data):
    (sc,) = D.read_file(data)["scans"]
    return sc["start"], sc["end"]


@functools.lru_cache(None)
def _broken():
    """name -> a file that does not decode, each from an intact one"""
    good = FILES()[6]  # 16 MCUs in intervals of 6, 6, 4
    s, e = _scan_of(good)
    body = good[s:e]
    m0, m1 = body.index(b"\xff\xd0"), body.index(b"\xff\xd1")
    c = HC.make("marked-grey", "bad-ac-16-ones", "interval-mid")
    head, tail = HC.header(HC.base_of(c))
    out = {
        "truncated": good[:e - 9] + good[e:],
        "marker removed": good[:s + m0] + good[s + m0 + 2:],
        "marker surplus": good[:s + m1] + b"\xff\xd1" + good[s + m1:],
        "corrupted code": head + c.scan + tail,
    }
    sof = good.index(b"\xff\xc0")
    out["12-bit"] = good[:sof + 4] + bytes([12]) + good[sof + 5:]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["truncated", "marker removed", "marker surplus", "corrupted code", "12-bit"])
def test_a_broken_file_between_two_intact_ones(gpu, name):
    torch = gpu
    bad = _broken()[name]
    kind, want = alone(torch, bad)
    assert kind == "error"
    assert isinstance(want, jfif.JpegFormatError if name == "12-bit" else D.JpegDecodeError), want
    files = [FILES()[2], bad, FILES()[7]]
    api.kernel_counts_reset()
    got = D.decode_jpeg_batch(files, coefficients=True, on_error="return")
    torch.cuda.synchronize()
    for i in (0, 2):
        assert same(torch, got[i], alone(torch, files[i], coefficients=True)[1]), i
        for q, w in zip(got[i][1], checker(files[i])):
            assert np.array_equal(q.cpu().numpy(), w)
    assert same_error(got[1], want) and got[1].file == 1, (got[1], want)
    assert {k: v for k, v in api.kernel_counts().items() if k in BATCH_KERNELS} == {k: 1 for k in BATCH_KERNELS}
    with pytest.raises(type(want)) as e:
        D.decode_jpeg_batch(files, on_error="raise")
    assert same_error(e.value, want) and e.value.file == 1
    # the lowest-numbered failing file is the one raised, whichever stage finds it
    with pytest.raises(D.JpegDecodeError) as e:
        D.decode_jpeg_batch([FILES()[0], _broken()["truncated"], _broken()["12-bit"]])
    assert e.value.file == 1
    with pytest.raises(jfif.JpegFormatError) as e:
        D.decode_jpeg_batch([_broken()["12-bit"], _broken()["truncated"]])
    assert e.value.file == 0


@pytest.mark.gpu
def test_only_broken_files(gpu):
    got = D.decode_jpeg_batch([_broken()["12-bit"], b"no jpeg"], on_error="return")
    assert [type(g) for g in got] == [jfif.JpegFormatError] * 2 and [g.file for g in got] == [0, 1]


CANARY = 0x5A5A


def _c_level_scans():
    """the scans driven at the C level: (frame, scan dict, bytes, planes) -- a 4:2:0 interleaved scan, two grey scans with 12 and 3
    intervals, and the second of them again with its first marker removed"""
    out = []
    for (w, h, comps, dri, seed) in ((48, 32, C420, 3, 51), (96, 8, G, 1, 52), (32, 24, G, 4, 53)):
        frame = dict(width=w, height=h, comps=comps)
        scan = dict(comps=INTERLEAVED if len(comps) == 3 else [(0, 0, 0)], dri=dri)
        planes = _planes(frame, seed)
        body, st = E.encode_scan(frame, scan, planes, dict(E.ANNEX_K))
        out.append((frame, scan, body, planes, st))
    frame, scan, body, planes, st = out[2]
    m = st["markers"][0]
    out.append((frame, scan, body[:m] + body[m + 2:], planes, st))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("after", [0x00, 0xFF, 0xD1])
def test_c_level_canaries_and_offsets(gpu, after):
    """the byte buffer holds `after` before, between and after the scans (0xFF before a scan would make its first byte a stuffed zero
    or a marker's second byte, 0xFF / 0xD1 after it an RSTm across the scan's end, if a neighbour's byte were ever looked at)"""
    torch = gpu
    cases = _c_level_scans()
    blob, at = bytearray([after] * 3), []
    for _, _, body, _, _ in cases:
        at.append(len(blob))
        blob += body + bytes([after] * 3)
    seg = torch.frombuffer(blob, dtype=torch.uint8).cuda()
    scans, guards = [], []
    for (frame, scan, body, planes, _), a in zip(cases, at):
        gx, gy, _ = E.grid(frame, scan)
        comp = []
        for ci, (rows, cols) in enumerate(E.plane_shapes(frame)):
            big = torch.full((rows + 2, cols + 16), CANARY, dtype=torch.int16, device="cuda")
            inner = big[1:-1, 8:-8]
            h, v = frame["comps"][ci]
            comp.append((D._PlaneShape(rows, cols + 16, inner.data_ptr()), cols // 8, rows // 8, h, v, min(ci, 1), 2 + min(ci, 1)))
            guards.append((big, inner, planes[ci]))
        specs = [E.ANNEX_K[(0, 0)], E.ANNEX_K[(0, 1)], E.ANNEX_K[(1, 0)], E.ANNEX_K[(1, 1)]]
        scans.append((D.scan_desc(comp, gx, gy, scan["dri"]), a, len(body), specs))
    plan = D.BatchPlan(scans, len(blob))
    off = torch.full((plan.n_offsets + 2,), -7, dtype=torch.int64, device="cuda")
    status = torch.full((plan.n_intervals + 2,), -7, dtype=torch.int32, device="cuda")
    image = torch.empty(plan.image_bytes, dtype=torch.uint8, device="cuda")
    image.copy_(torch.from_numpy(plan.bind(image, seg, off[1:-1], status[1:-1])))
    api.kernel_counts_reset()
    plan.index()
    plan.decode()
    torch.cuda.synchronize()
    assert {k: v for k, v in api.kernel_counts().items() if k in BATCH_KERNELS} == {k: 1 for k in BATCH_KERNELS}
    off_h, st_h = off.cpu().numpy(), status.cpu().numpy()
    assert off_h[0] == off_h[-1] == -7 and st_h[0] == st_h[-1] == -7
    first = plan.first_interval
    for k, (_, _, body, _, _) in enumerate(cases):
        n = first[k + 1] - first[k]
        alone_seg = torch.frombuffer(bytearray(body), dtype=torch.uint8).cuda()
        o1, s1 = torch.empty(n + 1, dtype=torch.int64, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
        D.index(alone_seg, n, o1, s1)
        assert np.array_equal(off_h[1 + first[k] + k:1 + first[k + 1] + k + 1], o1.cpu().numpy()), k
    assert (st_h[1:1 + first[3]] == 0).all()
    # the scan without its first marker: its first interval runs into the second's data, its last has neither marker nor data;
    # the status of every interval is what the single-scan decoder gives on that scan alone (compared below), and no other scan moved
    broken = st_h[1 + first[3]:1 + first[4]]
    assert broken[0] != 0 and broken[-1] == D._jpegdec_lib.OUT_OF_DATA and int(off_h[1 + first[4] + 3 - 1]) == len(cases[3][2]) + 2
    frame, scan, body, _, _ = cases[3]
    rows, cols = E.plane_shapes(frame)[0]
    lone = torch.zeros((rows, cols), dtype=torch.int16, device="cuda")
    tables = D.Tables([E.ANNEX_K[(0, 0)], None, E.ANNEX_K[(1, 0)], None])
    n = first[4] - first[3]
    o1, s1 = torch.empty(n + 1, dtype=torch.int64, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    alone_seg = torch.frombuffer(bytearray(body), dtype=torch.uint8).cuda()
    D.index(alone_seg, n, o1, s1)
    D.decode(D.scan_desc([(lone, cols // 8, rows // 8, 1, 1, 0, 2)], cols // 8, rows // 8, scan["dri"]), tables, alone_seg, o1, s1)
    torch.cuda.synchronize()
    tables.close()
    assert np.array_equal(broken, s1.cpu().numpy())
    assert torch.equal(guards[-1][1], lone)
    # planes: the levels inside, the canaries around them
    for big, inner, want in guards[:-1]:
        assert np.array_equal(inner.cpu().numpy(), want.astype(np.int16))
    for big, inner, _ in guards:
        b = big.cpu().numpy()
        assert (b[0] == CANARY).all() and (b[-1] == CANARY).all() and (b[:, :8] == CANARY).all() and (b[:, -8:] == CANARY).all()
    plan.close()


@pytest.mark.gpu
def test_four_launches_whatever_the_number_of_files(gpu):
    torch = gpu
    for n in (2, 9):
        files = list(FILES()[:n])
        api.kernel_counts_reset()
        got = D.decode_jpeg_batch(files, coefficients=True)
        torch.cuda.synchronize()
        ran = api.kernel_counts()
        assert {k: v for k, v in ran.items() if k in BATCH_KERNELS} == {k: 1 for k in BATCH_KERNELS}, (n, ran)
        assert not any(k == "k_decode" or k.startswith(("k_rst_", "k_um_", "k_decode_prog")) for k in ran), (n, ran)
        for f, g in zip(files, got):
            assert same(torch, g, alone(torch, f, coefficients=True)[1])


@pytest.mark.gpu
@pytest.mark.parametrize("arrangement,fill", [("A", 0), ("A", 0x7F7F7F7F), ("B", None), ("D", None)], ids=["A-stale-0", "A-stale-7f", "B", "D"])
@pytest.mark.parametrize("name", ["decode-batch", "decode-batch-hostile"])
def test_a_stalled_stream_that_is_not_the_current_one(gpu, name, arrangement, fill):
    """the arrangements A (with both stale fills), B and D of tests/test_jpeg_streams.py on decode_jpeg_batch: a mixed batch with a
    fallback file in RGB, and a batch with a broken file whose statuses come back in the exception"""
    import test_jpeg_streams as S
    torch = gpu
    if name not in S.CASES:
        if name == "decode-batch":
            files = [FILES()[i] for i in (1, 3, 7)] + [_fallback_files()[0]]
            S.CASES[name] = S.Case(name, lambda torch: lambda st: D.decode_jpeg_batch(files, stream=st, mode="RGB", coefficients=True),
                                   tally=("k_decode_batch", 1))
        else:
            files = [FILES()[2], _broken()["corrupted code"], FILES()[7]]
            want = alone(torch, files[1])[1]

            def check(truth):
                assert truth == ("JpegDecodeError", (want.scan, [int(x) for x in want.status])), truth

            S.CASES[name] = S.Case(name, lambda torch: lambda st: D.decode_jpeg_batch(files, stream=st), tally=("k_decode_batch", 1), check=check)
    S.run(torch, name, arrangement, fill=fill)
