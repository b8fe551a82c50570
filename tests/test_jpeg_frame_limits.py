"""The JPEG file entry points -- encode_jpeg, decode_jpeg, transcode_jpeg and both batches -- on thin strips at the 65535-pixel frame
limits (tests/jpeg_frame_limits.py has the cases): geometry the host checks allow and the seeded sweep, whose
widths end at 2100, never reaches.  The per-case checks are jpeg_sweep's, the engine adapter test_jpeg_sweep's.

CPU half: the geometry the cases were made for, asserted from the cases; every file is transcoded with the whole list of operations;
Pillow reads its own files at 65500, its limit; three faults planted in a case's true results each fail the case's checks; the
stand-in engine passes the two one-pixel strips, stage by stage (a full pass of the stand-in costs 13 to 67 s per larger file, so the
other pictures' tie-window caps are checked from the float64 rules alone).
GPU half: simd_dct_amd through FILES, one test per file and stage (the file with its decodes, and each transcode); the Pillow leg at
65500; the largest restart interval and its twin; the batches at and past 16384 MCU rows."""
import functools

import numpy as np
import pytest

import idct_reference as R
import jpeg_decode_checker as DC
import jpeg_encode_checker as EC
import jpeg_frame_limits as FL
import jpeg_progressive_checker as PC
import jpeg_scaled_checker as S
import jpeg_sweep as JS
import test_jpeg_sweep as SW

pytest.importorskip("PIL.Image")

LIMIT, PILLOW_MAX = FL.LIMIT, FL.PILLOW_MAX
NAMES = [c["name"] for c in FL.FILES]


def file_index(name):
    return NAMES.index(name)


# ------------------------------------------------------------------------------------------ CPU: the cases
def test_the_cases_are_the_matrix():
    assert len(set(NAMES)) == len(NAMES) == 35
    wide, tall = [c for c in FL.FILES if c["W"] >= 65521], [c for c in FL.FILES if c["H"] == LIMIT]
    assert len(wide) == 18 and len(tall) == 17 and all(max(c["W"], c["H"]) == LIMIT for c in FL.FILES if c["W"] != 65521)
    for strip in (wide, tall):
        short = {min(c["W"], c["H"]) for c in strip}
        assert short >= {1, 8, 9, 17}, short
        assert {(c["form"], c["layout"]) for c in strip if c["enc_sampling"] == "4:2:0"} >= {
            ("default", "HWC"), ("interleaved", "HWC"), ("optimize", "HWC"), ("interleaved optimize", "HWC"), ("progressive", "HWC"), ("progressive standard", "HWC"),
            ("default", "CHW")}
        for sampling in JS.ENCODER_SAMPLINGS:
            forms = {c["form"] for c in strip if c["enc_sampling"] == sampling and min(c["W"], c["H"]) == 9}
            assert forms >= ({"default"} if sampling == "grey" else {"default", "interleaved"}), (sampling, forms)
        assert {c["enc_sampling"] for c in strip if min(c["W"], c["H"]) == 1} == {"grey", "4:2:0"}
    assert any(c["W"] % 16 == 1 and c["H"] == 17 for c in wide)
    assert all(c["quality"] == 90 and c["picture"] == "noisy photo" for c in FL.FILES)


def test_the_geometry_the_cases_were_made_for():
    for c in FL.FILES:
        g = FL.geometry(c)
        if c["W"] == LIMIT:
            assert g["chunks"] >= 32 and g["row_blocks"] >= 8192 and g["front_tiles"] >= 64, (c["name"], g)  # 32 chunks of the 256-block seam, 64 front tiles
            if c["enc_sampling"] in ("4:2:0", "4:2:2"):
                assert LIMIT % 16 == 15 and g["padded_luma"] == 65536, (c["name"], g)  # the MCU-padded luma width: the last legal value
        if c["H"] == LIMIT and c["enc_sampling"] in ("grey", "4:4:4"):
            assert g["intervals"] == 8192, (c["name"], g)
    g = FL.geometry(FL.FILES[file_index("65535 x 17 4:2:0 interleaved")])
    assert g["row_blocks"] == 24576 and g["seg_stride"] == 208 * 24576 + 8 and g["intervals"] == 2  # about 5.1 MB of segment space per MCU row
    from simd_dct_amd import jpeg_encode as J
    assert J.scan_seg_stride(4096, J.sampling_of("4:2:0")) == g["seg_stride"]
    cw, ch = EC.true_sizes(LIMIT, 17, JS.SAMPLINGS["4:2:0"])[1]
    assert cw == 32768 and (2 * cw - 1) == LIMIT  # fancy upsampling ends on an odd column: the last chroma sample makes one pixel, not two
    for d, side in ((2, 32768), (4, 16384), (8, 8192)):
        assert S.geometry(LIMIT, 9, JS.SAMPLINGS["grey"], d)[1][0] == side and S.geometry(9, LIMIT, JS.SAMPLINGS["grey"], d)[1][1] == side


def test_every_file_is_transcoded_with_every_operation():
    """every file: transpose, rot90, flip_h and flip_v, with trim and without, and progressive=True, each a stage of its own, refused
    or accepted as jpeg_sweep.refusal says; the accepted ones cover every sampling x operation x orientation the geometry allows, the
    four output forms and both progressive scripts"""
    assert len(FL.STAGES) == 10 and len(set(FL.STAGES)) == 10
    seen, forms = set(), set()
    for i, c in enumerate(FL.FILES):
        ts = FL.transcodes(i)
        assert list(ts) == list(FL.STAGES[1:]), c["name"]
        assert [(t.get("transform"), t.get("trim", False), bool(t.get("progressive"))) for t in ts.values()] == \
            [(op, trim, False) for op in ("transpose", "rot90", "flip_h", "flip_v") for trim in (True, False)] + [(None, False, True)], c["name"]
        assert not FL._refused(c, ts["transpose"]) and not FL._refused(c, ts["transpose trim"]) and not FL._refused(c, ts["progressive"])
        assert ts["transpose"] == dict(ts["transpose trim"], trim=False)
        for stage, t in ts.items():
            if not FL._refused(c, t):
                seen.add((c["enc_sampling"], stage, "wide" if c["W"] > c["H"] else "tall"))
                forms.add("progressive " + str(t.get("script")) if t.get("progressive") else (t["optimize"], t["interleaved"]))
    for sampling in JS.ENCODER_SAMPLINGS:
        for strip in ("wide", "tall"):
            for stage in ("transpose", "transpose trim", "rot90 trim", "flip_h trim", "flip_v trim", "progressive"):
                # (4:2:2 runs on 9 x 65535 only, whose 9 columns hold no whole 16-column iMCU for a mirrored x axis to keep)
                assert ((sampling, stage, strip) in seen) == ((sampling, stage, strip) != ("4:2:2", "flip_h trim", "tall")), (sampling, stage, strip)
    # without trim a mirrored axis must be whole iMCUs: only the 8-pixel side of the 4:4:4 strips is
    assert {(s, st, strip) for s, st, strip in seen if st in ("rot90", "flip_h", "flip_v")} == {("4:4:4", "rot90", "wide"), ("4:4:4", "flip_v", "wide"), ("4:4:4", "flip_h", "tall")}
    assert forms == {(True, False), (False, False), (True, True), (False, True), "progressive None", "progressive standard"}, forms
    # what a strip that is no multiple of the iMCU refuses: a mirrored axis without trim, and with trim an axis without a whole iMCU
    c, ts = FL.FILES[file_index("65535 x 9 4:2:0 default")], FL.transcodes(file_index("65535 x 9 4:2:0 default"))
    assert [st for st, t in ts.items() if FL._refused(c, t)] == ["rot90 trim", "rot90", "flip_h", "flip_v trim", "flip_v"]


def reference_caps(case):
    """{rule: smallest decided share over the planes} from the float64 rules alone: the forward rule on the picture's planes, the
    inverse and the scaled rules on rne(DCT / Q) of them (what the stand-in encodes)"""
    W, H, grey = case["W"], case["H"], case["enc_sampling"] == "grey"
    sampling = JS.SAMPLINGS[case["enc_sampling"]]
    sub = "4:2:0" if grey else case["enc_sampling"]
    out = {}
    planes = EC.planes(JS.picture(case), sub, padded=JS.plane_sizes(W, H, sampling, True))
    for k, (p, (cw, ch)) in enumerate(zip(planes, EC.true_sizes(W, H, sampling))):
        q = JS.quality_tables(case["quality"])[min(k, 1)].astype(np.float64)
        _, exact, tol = R.fwd_coefficients(R.blocks(p), q.astype(np.float32), 128.0)
        out["forward"] = min(out.get("forward", 1.0), float(R.decided(exact, tol, *R.I16_RANGE).mean()))
        c = R.plane(R.sat_i16(R.rne(R.dct2(R.blocks(p).astype(np.float64) - 128.0) / q.reshape(8, 8))), p.shape[1], p.shape[0]).astype(np.int16)
        _, exact, tol = S.component(c, q, 8, cw, ch)
        out["inverse"] = min(out.get("inverse", 1.0), float(R.decided(exact, tol, *R.U8_RANGE).mean()))
        for d in JS.SCALES:
            g = S.geometry(W, H, sampling, d)[0][k]
            _, exact, tol = S.component(c, q, g[0], g[1], g[2])
            out[f"1/{d}"] = min(out.get(f"1/{d}", 1.0), float(R.decided(exact, tol, *R.U8_RANGE).mean()))
    return out


PICTURES = sorted({(c["W"], c["H"], c["enc_sampling"]) for c in FL.FILES})


@pytest.mark.parametrize("W,H,sampling", PICTURES)
def test_the_pictures_stay_inside_the_tie_window_caps(W, H, sampling):
    """the cap min_decided = 0.5 applies to every plane on its own here (the smallest has 8192 blocks): the reference alone decides
    more than half of every plane of every picture of FILES under every rule, whatever an engine gives (the least: 0.86, at 1/8,
    where a sample is DC / 8 and every eighth DC level lies on a tie; above 0.99 under the other rules)"""
    caps = reference_caps(next(c for c in FL.FILES if (c["W"], c["H"], c["enc_sampling"]) == (W, H, sampling)))
    print(caps)
    assert min(caps.values()) > JS.MIN_DECIDED, caps


# ------------------------------------------------------------------------------------------ CPU: the stand-in, and the checks bite
WIDE_ONE, TALL_ONE = "65535 x 1 grey default", "1 x 65535 grey default"


@functools.lru_cache(None)
def stand_in_truth(name):
    """(case, the stand-in's file, its planes by the checker, the stand-in's three decodes of it)"""
    case = FL.FILES[file_index(name)]
    engine = JS.StandIn()
    data = bytes(engine.encode(JS.laid_out(JS.picture(case), case["layout"]), case["quality"], "4:2:0", case["layout"], **JS.encode_form(case)))
    C = JS.checker_decode(data)[0]
    got = {}
    got["planes"], got["coefs"] = engine.decode(data, None, "HWC", 1)
    got["rgb"], got["rgb_coefs"] = engine.decode(data, "RGB", case["layout"], 1)
    got["scaled"], got["scaled_coefs"] = engine.decode(data, None, "HWC", case["scale"])
    JS.check_decode(case, data, C, got)
    return case, data, C, got


STAND_IN = JS.StandIn()


@pytest.mark.parametrize("name,stage", [(name, stage) for name in (WIDE_ONE, "1 x 65535 4:2:0 default") for stage in FL.STAGES])
def test_the_stand_in_passes_a_wide_and_a_tall_case(name, stage):
    FL.run_stage(STAND_IN, file_index(name), stage)


def _with_coefficients(got, planes, data):
    """a copy of the true decodes in which the coefficient planes, and the pixels made of them, are `planes`"""
    W, H, sampling, qtables, _ = JS.decoded_frame(data)
    out = dict(got)
    for key in ("coefs", "rgb_coefs", "scaled_coefs"):
        out[key] = [np.array(p) for p in planes]
    out["planes"] = [S.component(c, q, 8, cw, ch)[0].astype(np.uint8) for c, q, (cw, ch) in zip(planes, qtables, EC.true_sizes(W, H, sampling))]
    return out


@pytest.mark.parametrize("name,fault", [(WIDE_ONE, "last block column"), (TALL_ONE, "block rows shifted")])
def test_a_fault_planted_in_the_true_coefficients_fails_the_checks(name, fault):
    """the last block column of the wide strip zeroed; block rows 4096 and above shifted by one on the tall strip: in the coefficient
    planes the comparison with the file's coefficients fails, in the pixels alone the inverse rule does"""
    case, data, C, got = stand_in_truth(name)
    bad = FL.last_block_column_zeroed(C) if fault == "last block column" else FL.block_rows_shifted(C)
    assert any(not np.array_equal(b, c) for b, c in zip(bad, C))
    faulty = _with_coefficients(got, bad, data)
    with pytest.raises(AssertionError, match="differ from the file's coefficients"):
        JS.check_decode(case, data, C, faulty)
    pixels_only = dict(got, planes=faulty["planes"])
    with pytest.raises(AssertionError, match="decode plane 0"):
        JS.check_decode(case, data, C, pixels_only)
    # the same planes as a transcode's output: the transformed source differs
    out = JS.StandIn()._write(case["W"], case["H"], [(1, 1)], bad, [q.astype(np.int64) for q in JS.quality_tables(90)], True, False, False, None, False)
    with pytest.raises(AssertionError, match="differs from the transformed source"):
        JS.check_transcode(FL.with_transcode(case, dict()), data, C, out, pillow=False)


def test_a_wrong_restart_number_after_the_first_wrap_fails_the_checks():
    """the tall grey strip has 8192 restart intervals; RSTm wraps 1023 times and the last is (n - 2) & 7.  One numbered (k + 1) & 7 from
    k = 8 on fails the case's encode checks"""
    case, data, C, _ = stand_in_truth(TALL_ONE)
    marks = FL.rst_markers(data)
    n = FL.geometry(case)["intervals"]
    assert n == 8192 and len(marks) == n - 1 and [m for _, m in marks] == [k & 7 for k in range(n - 1)] and marks[-1][1] == (n - 2) & 7 == 6
    pic = JS.picture(case)
    JS.check_encode(case, data, pic, pillow=False)
    bad = FL.with_wrong_rst(data)
    assert sum(a != b for a, b in zip(bad, data)) == n - 1 - 8
    with pytest.raises(AssertionError):
        JS.check_encode(case, bad, pic, pillow=False)
    statuses = JS.checker_decode(bad)[1]
    assert all(s == 0 for s in statuses[0][:8]) and any(s != 0 for s in statuses[0][8:]), statuses[0][:12]


def test_two_tall_pictures_are_exactly_the_batch_cap():
    from simd_dct_amd import _jpegenc_batch_lib
    from simd_dct_amd import jpeg_encode as J
    from test_jpeg_encode_batch import described
    assert J.mcu_grid(8, LIMIT, J.sampling_of("4:4:4"))[1] == 8192
    p = J.BatchPlan([described(k, 8, LIMIT, "4:4:4") for k in range(2)], "HWC", J.quality_tables(90))
    assert p.n_rows == 16384 == _jpegenc_batch_lib.MAX_ROWS and p.first_row == [0, 8192, 16384]
    p.close()


# ------------------------------------------------------------------------------------------ CPU: Pillow at its limit
PILLOW_STRIPS = [(PILLOW_MAX, 17, False), (PILLOW_MAX, 17, True), (17, PILLOW_MAX, False), (17, PILLOW_MAX, True)]
PILLOW_KINDS = {"marked": dict(restart_marker_rows=1), "unmarked": dict(), "progressive": dict(progressive=True)}
INTERVAL = (PILLOW_MAX, 72)  # grey: 8188 x 9 = 73692 MCUs


def largest_interval_file():
    return FL.pillow_strip(*INTERVAL, True, restart_marker_blocks=65535)


@pytest.mark.parametrize("W,H,grey", PILLOW_STRIPS)
def test_pillow_reads_its_own_files_at_its_limit(W, H, grey):
    assert PILLOW_MAX == 65500
    for kind, kw in PILLOW_KINDS.items():
        data = FL.pillow_strip(W, H, grey, **kw)
        JS.check_pillow(data, W, H, grey, kind)
        frame, _, scans, _ = PC.parse(data)
        assert (frame["sof"] == 0xC2) == (kind == "progressive") and (frame["width"], frame["height"]) == (W, H)
        assert all((sc["dri"] > 0) == (kind == "marked") for sc in scans), (kind, [sc["dri"] for sc in scans])


def test_the_largest_restart_interval_file():
    data = largest_interval_file()
    JS.check_pillow(data, *INTERVAL, True, "DRI 65535")
    frame, _, scans, _ = PC.parse(data)
    mcus = JS.mcus(*INTERVAL, [(1, 1)])
    assert mcus == (8188, 9) and frame["sof"] == 0xC0 and len(scans) == 1 and scans[0]["dri"] == 65535
    # two intervals: the first of 65535 MCUs, one RST0 between them
    assert JS._ceil(mcus[0] * mcus[1], 65535) == 2 and [m for _, m in FL.rst_markers(data)] == [0]


# ------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    from simd_dct_amd import api
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    torch.cuda.set_device(0)
    api.init(0)
    return SW.Engine(torch)


@pytest.mark.gpu
@pytest.mark.parametrize("name,stage", [(name, stage) for name in NAMES for stage in FL.STAGES])
def test_gpu_a_file_at_the_frame_limit(gpu, name, stage):
    """'file': encode_jpeg's file by the serial checker, the forward rule, DQT, scans recoded byte for byte, tables; decode_jpeg to
    planes, RGB (HWC and CHW), coefficients, 1/2, 1/4 and 1/8.  Any other stage: that transcode_jpeg call on the file -- plan_transform's
    ValueError where the host refuses, else the output by the serial checker against the transformed planes"""
    FL.run_stage(gpu, file_index(name), stage)


def _decodes(engine, data):
    """(coefficient planes, pixel planes) of decode_jpeg as device tensors"""
    planes, coefs = engine.D.decode_jpeg(data, coefficients=True)
    engine.torch.cuda.synchronize()
    return coefs, planes


@functools.lru_cache(maxsize=2)
def marked_truth(W, H, grey):
    """(Pillow's restart-marked file of the strip, its coefficient planes by the serial checker): once for the three tests of a strip"""
    marked = FL.pillow_strip(W, H, grey, **PILLOW_KINDS["marked"])
    C, statuses, _ = DC.decode(marked)
    assert all(s == 0 for st in statuses for s in st)
    for p in C:
        p.setflags(write=False)
    return marked, C


def _pillow_case(W, H, grey):
    sampling = "grey" if grey else "4:2:0"
    return JS.explicit_case(f"{W} x {H} {sampling} at Pillow's limit", W, H, sampling, "interleaved", picture_seed=50)


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,grey", PILLOW_STRIPS)
def test_gpu_pillow_opens_the_engines_files_at_65500(gpu, W, H, grey):
    case = _pillow_case(W, H, grey)
    pic = JS.picture(case)
    for form in ({}, dict(interleaved=True), dict(optimize=True), dict(progressive=True), dict(progressive=True, script="standard")):
        JS.check_pillow(bytes(gpu.encode(pic, 90, "4:2:0", "HWC", **form)), W, H, grey, f"{case['name']} {form}")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(PILLOW_KINDS))
@pytest.mark.parametrize("W,H,grey", PILLOW_STRIPS)
def test_gpu_the_engine_decodes_pillows_files_at_65500(gpu, W, H, grey, kind):
    """Pillow's restart-marked file decodes to the serial checker's coefficients; Pillow's file without markers (the 8 KiB-chunk
    decoder) and its progressive file -- the same picture, quality and quantiser -- to the marked twin's tensors, coefficients and
    pixels (a progressive file holds of the MCU grid beyond a component's own grid the DC only; so does every file of libjpeg's, whose
    dummy blocks at the right and bottom edges are a copied DC and no AC); the pixels of all three meet the inverse rule on those
    planes, RGB is the colour checker's, 1/2 meets the scaled rule"""
    case = dict(_pillow_case(W, H, grey))
    case["name"] += " " + kind
    marked, C = marked_truth(W, H, grey)
    data = FL.pillow_strip(W, H, grey, **PILLOW_KINDS[kind])
    got = {}
    got["planes"], got["coefs"] = gpu.decode(data, None, "HWC", 1)
    if kind != "marked":
        twin_planes, twin_coefs = gpu.decode(marked, None, "HWC", 1)
        assert all(np.array_equal(g, w) for g, w in zip(got["coefs"], twin_coefs)) and all(np.array_equal(g, w) for g, w in zip(got["planes"], twin_planes)), kind
    got["rgb"], got["rgb_coefs"] = gpu.decode(data, "RGB", "HWC", 1)
    got["scaled"], got["scaled_coefs"] = gpu.decode(data, None, "HWC", 2)
    JS.check_decode(case, data, C, got)


@pytest.mark.gpu
def test_gpu_the_largest_restart_interval(gpu):
    """DRI = 65535, T.81's largest: the first interval is 65535 MCUs in one k_decode workgroup.  The coefficients are the same
    picture's restart_marker_rows=1 file's, which the test below holds to the checker; also through decode_jpeg_batch beside a
    small file"""
    torch = gpu.torch
    data, twin = largest_interval_file(), FL.pillow_strip(*INTERVAL, True, restart_marker_rows=1)
    assert gpu.D.read_file(data)["scans"][0]["restart_interval"] == 65535 and gpu.D.read_file(twin)["scans"][0]["restart_interval"] == 8188
    torch.cuda.synchronize()
    gpu.api.kernel_counts_reset()
    coefs, planes = _decodes(gpu, data)
    assert gpu.api.kernel_counts().get("k_decode", 0) == 1, gpu.api.kernel_counts()
    twin_coefs, twin_planes = _decodes(gpu, twin)
    assert all(torch.equal(g, w) for g, w in zip(coefs, twin_coefs)) and all(torch.equal(g, w) for g, w in zip(planes, twin_planes))
    small = FL.pillow_strip(72, 40, True, restart_marker_rows=1)
    batch = gpu.decode_batch([small, data, small], None, "HWC")  # (each against decode_jpeg alone, k_decode_batch once)
    assert all(np.array_equal(g, w.cpu().numpy()) for g, w in zip(batch[1][1], twin_coefs))


@pytest.mark.gpu
def test_gpu_the_twin_of_the_largest_interval_file_is_the_checkers(gpu):
    """the 65500 x 72 restart_marker_rows=1 file, the truth of the test above: jpeg_decode_checker reads it (73692 blocks), and the
    engine's coefficients, pixels, RGB and half-size planes are held to that"""
    twin = FL.pillow_strip(*INTERVAL, True, restart_marker_rows=1)
    C, statuses, _ = DC.decode(twin)
    assert all(s == 0 for st in statuses for s in st)
    JS.stage_decode(gpu, JS.explicit_case("65500 x 72 grey, a restart interval per row", *INTERVAL, "grey", picture_seed=50), twin, C)


def _tall_444(torch, k):
    case = JS.explicit_case(f"8 x 65535 4:4:4 picture {k}", 8, LIMIT, "4:4:4", picture_seed=60 + 3 * k)
    return torch.from_numpy(JS.picture(case)).cuda()


@pytest.mark.gpu
def test_gpu_encode_batch_at_exactly_16384_rows(gpu):
    """two 8 x 65535 4:4:4 pictures: 2 x 8192 MCU rows, the packer's bound, in one group of three launches"""
    from simd_dct_amd import _jpegenc_batch_lib
    torch, J = gpu.torch, gpu.J
    images = [_tall_444(torch, k) for k in range(2)]
    assert sum(J.mcu_grid(8, LIMIT, J.sampling_of("4:4:4"))[1] for _ in images) == 16384 == _jpegenc_batch_lib.MAX_ROWS
    torch.cuda.synchronize()
    gpu.api.kernel_counts_reset()
    files = J.encode_jpeg_batch(images, 90, "4:4:4")
    torch.cuda.synchronize()
    ran = gpu.api.kernel_counts()
    assert ran.get("k_batch_pack", 0) == 1 and sum(ran.values()) == 3, ran
    for k, (img, data) in enumerate(zip(images, files)):
        assert bytes(data) == bytes(J.encode_jpeg(img, 90, "4:4:4", interleaved=True)), k
    assert files[0] != files[1]


@pytest.mark.gpu
def test_gpu_encode_batch_past_16384_rows_is_cut_into_groups(gpu):
    """encode_jpeg_batch's docstring: "A batch of more than 16384 MCU rows is cut into consecutive groups below that bound, three
    launches each" (the C plan itself refuses more: test_jpeg_encode_batch.test_plan_refuses_more_than_16384_rows).  A third
    picture: two groups, six launches, every file as alone"""
    torch, J = gpu.torch, gpu.J
    images = [_tall_444(torch, k) for k in range(3)]
    torch.cuda.synchronize()
    gpu.api.kernel_counts_reset()
    files = J.encode_jpeg_batch(images, 90, "4:4:4")
    torch.cuda.synchronize()
    ran = gpu.api.kernel_counts()
    assert ran.get("k_batch_pack", 0) == 2 and sum(ran.values()) == 6, ran
    for k, (img, data) in enumerate(zip(images, files)):
        assert bytes(data) == bytes(J.encode_jpeg(img, 90, "4:4:4", interleaved=True)), k
    assert len({bytes(f) for f in files}) == 3


@pytest.mark.gpu
def test_gpu_decode_batch_of_four_tall_files_and_two_wide_ones(gpu):
    """one decode_jpeg_batch call: every tensor torch.equal to decode_jpeg alone, k_decode_batch once (Engine.decode_batch asserts
    both); the search over the batch's interval prefix runs over 4 x 8192 + ... intervals"""
    names = ["9 x 65535 grey default", "9 x 65535 4:4:4 default", "9 x 65535 4:2:0 interleaved", "8 x 65535 4:4:4 interleaved", "65535 x 9 4:2:2 default",
             "65535 x 9 4:2:0 interleaved"]
    files = []
    for name in names:
        case = FL.FILES[file_index(name)]
        sub = "4:2:0" if case["enc_sampling"] == "grey" else case["enc_sampling"]
        files.append(bytes(gpu.encode(JS.picture(case), 90, sub, "HWC", **JS.encode_form(case))))
    intervals = sum(sum(JS._ceil(JS.scan_grid(W, H, s, [ci for ci, _, _ in sc["comps"]])[0] * JS.scan_grid(W, H, s, [ci for ci, _, _ in sc["comps"]])[1], sc["dri"])
                        for sc in PC.parse(f)[2]) for f in files for W, H, s, _, _ in [JS.decoded_frame(f)])
    assert intervals > 40000, intervals
    for mode, layout in ((None, "HWC"), ("RGB", "CHW")):
        batch = gpu.decode_batch(files, mode, layout)
        assert len(batch) == len(files)
