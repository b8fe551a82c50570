"""Thin strips at the frame limits of the JPEG file entry points: the cases of tests/test_jpeg_frame_limits.py, stated on explicit
values through jpeg_sweep.explicit_case, and the pieces its CPU and GPU halves share.  No GPU in here.

T.81 allows 65535 pixels each way and the engine refuses 65536; libjpeg (Pillow) stops at PILLOW_MAX = 65500, so at 65535 the truths
are the project's own test-side pieces (the serial checkers, the float64 rules, the test-side encoders), and Pillow serves at 65500.

  FILES           the strips the encoder writes: every encoder form at 4:2:0 and every sampling in the default and interleaved forms on a
                  wide and a tall strip, the one-pixel strips, 65535 x 8 / 8 x 65535 and 65521 x 17 (1 mod 16).
  transcodes(i)   what file i is transcoded with: (transpose, rot90, flip_h, flip_v) x (trim, no trim) and progressive=True, refused by
                  plan_transform or accepted; the output form rotates.
  run_stage       an engine through one stage of one file: 'file', jpeg_sweep's checks of the encode and of the decodes with both RGB
                  layouts and all three scales; any other, its checks of that one transcode.  Ten tests per file, so that each stays at
                  a few seconds of serial truth (an accepted output costs a serial read); the file is encoded and read once for all.
  rst_markers, with_wrong_rst, ...   what the CPU half plants and counts."""
import functools

import numpy as np

import jpeg_progressive_checker as PC
import jpeg_sweep as JS

LIMIT = 65535  # T.81's largest frame side, and the engine's
PILLOW_MAX = JS.PILLOW_MAX
QUALITY = 90
RING_BYTES = 4 * 1024  # kFusedRing, kRing: the bit stream the coders hold in LDS per window (test_jpeg_hidden_state.RING_BYTES)
CHUNK = 256  # blocks: the coders' seam
FRONT_TILE = 1024  # luma columns of a front tile


def _files():
    out = []

    def add(W, H, sampling, form, layout="HWC"):
        name = f"{W} x {H} {sampling} {form}" + (" CHW" if layout == "CHW" else "")
        out.append(JS.explicit_case(name, W, H, sampling, form, quality=QUALITY, layout=layout, picture_seed=40 + len(sampling),
                                    dc_interleaved=len(out) % 2 == 1))

    # every encoder form at 4:2:0.  The default and interleaved forms at 17 rows (two MCU rows); the others at 9: a 65535 x 17 4:2:0 file is
    # 49152 blocks, six seconds of serial truth before anything is decoded; what gives way is the short side, 17 -> 9, never the long one
    for W, H in ((LIMIT, 17), (17, LIMIT)):
        add(W, H, "4:2:0", "default")
        add(W, H, "4:2:0", "interleaved")
    for W, H in ((LIMIT, 9), (9, LIMIT)):
        for form in ("optimize", "interleaved optimize", "progressive", "progressive standard"):
            add(W, H, "4:2:0", form)
        add(W, H, "4:2:0", "default", "CHW")
    # every sampling in the default and interleaved forms (a grey picture has no interleaved form)
    for W, H in ((LIMIT, 9), (9, LIMIT)):
        for sampling in JS.ENCODER_SAMPLINGS:
            add(W, H, sampling, "default")
            if sampling != "grey":
                add(W, H, sampling, "interleaved")
    for W, H in ((LIMIT, 1), (1, LIMIT)):
        add(W, H, "grey", "default")
        add(W, H, "4:2:0", "default")
    add(LIMIT, 8, "4:4:4", "interleaved")
    add(8, LIMIT, "4:4:4", "interleaved")
    add(65521, 17, "4:2:0", "default")  # 1 mod 16
    return out


FILES = _files()
# what every file is transcoded with: transpose, rot90 and both flips, with trim and without, and progressive=True
ASKED = tuple(dict(transform=op, trim=trim) for op in ("transpose", "rot90", "flip_h", "flip_v") for trim in (True, False)) + (dict(progressive=True),)
OUTPUT_FORMS = (dict(optimize=True), dict(optimize=False), dict(optimize=True, interleaved=True), dict(optimize=False, interleaved=True))


def stage_name(t):
    return "progressive" if t.get("progressive") else t["transform"] + (" trim" if t["trim"] else "")


STAGES = ("file",) + tuple(stage_name(t) for t in ASKED)  # one test each


def _refused(case, t):
    return JS.refusal(case["W"], case["H"], JS.SAMPLINGS[case["enc_sampling"]], t.get("transform"), t.get("trim", False)) is not None


def transcodes(i):
    """{stage: the transcode arguments} of FILES[i], all of ASKED.  Where plan_transform accepts, the output form rotates over
    OUTPUT_FORMS with the file and the operation (interleaved where the transformed sampling allows it); progressive=True takes the
    default script on even files, the standard one on odd ones"""
    case = FILES[i]
    sampling = JS.SAMPLINGS[case["enc_sampling"]]
    out = {}
    for j, t in enumerate(ASKED):
        t = dict(t)
        if t.get("progressive"):
            if i % 2:
                t["script"] = "standard"
        elif not _refused(case, t):
            t.update(OUTPUT_FORMS[(i + j // 2) % len(OUTPUT_FORMS)])  # (an operation's two trims share a form)
            osampling = [(v, h) for h, v in sampling] if t["transform"] in JS.X.TRANSPOSING else sampling
            t["interleaved"] = bool(t.get("interleaved")) and JS.interleavable(osampling)
        out[stage_name(t)] = t
    return out


def with_transcode(case, t):
    c = dict(case)
    c["transcode"] = JS.explicit_case(case["name"], case["W"], case["H"], case["enc_sampling"], **t)["transcode"]
    c["name"] = f"{case['name']}, transcode {t}"
    return c


def geometry(case):
    """what the kernels see of a case: blocks per row of its largest scan, chunks of 256 of them, front tiles, the padded luma width,
    restart intervals of the luma scan, bytes of segment space per MCU row of an interleaved scan"""
    W, H, sampling = case["W"], case["H"], JS.SAMPLINGS[case["enc_sampling"]]
    inter = bool(JS.FORMS[case["form"]].get("interleaved")) and len(sampling) == 3
    mx, my = JS.mcus(W, H, sampling)
    per_mcu = sum(h * v for h, v in sampling)
    row = mx * per_mcu if inter else JS.own_grids(W, H, sampling)[0][0]
    return dict(row_blocks=row, chunks=JS._ceil(row, CHUNK), front_tiles=JS._ceil(W, FRONT_TILE), padded_luma=JS.plane_sizes(W, H, sampling, True)[0][0],
                intervals=my if inter else JS.own_grids(W, H, sampling)[0][1], seg_stride=208 * mx * per_mcu + 8)


# ------------------------------------------------------------------------------------------ an engine through one file
def scan_bytes_per_chunk(data):
    """the first scan's mean bytes per 256 blocks (the default form's first scan is the luma plane's)"""
    frame, _, scans, _ = PC.parse(bytes(data))
    sc = scans[0]
    assert len(sc["comps"]) == 1
    W, H = frame["width"], frame["height"]
    bx, by = JS.own_grids(W, H, [(h, v) for _, h, v, _ in frame["components"]])[0]
    return (sc["end"] - sc["start"]) * CHUNK / (bx * by)


@functools.lru_cache(maxsize=2)
def encoded(engine, i):
    """(the engine's file of FILES[i], its coefficient planes by the serial checker): once for the stages of a file as long as they
    run one after the other, as pytest orders them; under another order the file is written and read again, which costs time and
    changes no result"""
    case = FILES[i]
    sub = "4:2:0" if case["enc_sampling"] == "grey" else case["enc_sampling"]
    data = bytes(engine.encode(JS.laid_out(JS.picture(case), case["layout"]), case["quality"], sub, case["layout"], **JS.encode_form(case)))
    return data, JS.checker_decode(data)[0]


def run_stage(engine, i, stage):
    """FILES[i] through one stage; a failure names the case.
    'file': the checks of the encoded file, then of its decodes -- planes, RGB in both layouts, 1/2, 1/4 and 1/8, the coefficients
    beside each.  Any other stage: that transcode of the same file, refused or accepted.  Pillow reads only what it can (pillow=)"""
    case = FILES[i]
    try:
        data, C = encoded(engine, i)
        pillow = max(case["W"], case["H"]) <= PILLOW_MAX
        if stage == "transpose trim":
            # trim cuts what a mirrored axis leaves over and transpose mirrors none: the same call, byte for byte, as without it,
            # which the stage "transpose" holds to the checkers
            t = dict(transcodes(i)["transpose"])
            assert JS.X.trimmed(case["W"], case["H"], JS.SAMPLINGS[case["enc_sampling"]], "transpose") == (case["W"], case["H"])
            assert bytes(engine.transcode(data, **dict(t, trim=True))) == bytes(engine.transcode(data, **t)), (JS.label(case), "transpose with trim")
            return
        if stage != "file":
            JS.stage_transcode(engine, with_transcode(case, transcodes(i)[stage]), data, C, pillow=pillow)
            return
        checked = JS.check_encode(case, data, JS.picture(case), pillow=pillow)
        assert all(np.array_equal(a, b) for a, b in zip(checked, C))
        W, H, sampling, _, _ = JS.decoded_frame(data)
        if case["form"] == "default" and W == LIMIT and H >= 8:
            per = scan_bytes_per_chunk(data)
            assert per > RING_BYTES, f"{per:.0f} bytes per chunk of 256 luma blocks: one window of the coders' ring holds it"
        got = {}
        got["planes"], got["coefs"] = engine.decode(data, None, "HWC", 1)
        got["rgb"], got["rgb_coefs"] = engine.decode(data, "RGB", case["layout"], 1)
        got["scaled"], got["scaled_coefs"] = engine.decode(data, None, "HWC", case["scale"])
        JS.check_decode(case, data, C, got)  # planes, RGB in the case's layout, 1/2
        what = JS.label(case) + " decode"
        other = "CHW" if case["layout"] == "HWC" else "HWC"
        rgb, coefs = engine.decode(data, "RGB", other, 1)
        JS.check_rgb(what, got["planes"], sampling, W, H, rgb, other)
        assert all(np.array_equal(g, c) for g, c in zip(coefs, C)), (what, "coefficients beside RGB", other)
        for d in (4, 8):
            scaled, coefs = engine.decode(data, None, "HWC", d)
            JS.check_scaled(what, data, C, scaled, d)
            assert all(np.array_equal(g, c) for g, c in zip(coefs, C)), (what, "coefficients at 1 /", d)
    except JS.CaseFailure:
        raise
    except Exception as e:
        raise JS.CaseFailure(f"{JS.label(case)} ({stage}) failed: {type(e).__name__}: {e}\ncase: {case}") from e


# ------------------------------------------------------------------------------------------ restart markers, and what the CPU half plants
def rst_markers(data, scan=0):
    """[(offset in the file, m)] of the RSTm markers of a scan (inside entropy-coded data 0xFF is followed by 0x00 or by a marker)"""
    sc = PC.parse(bytes(data))[2][scan]
    body = np.frombuffer(bytes(data), dtype=np.uint8)[sc["start"]:sc["end"]]
    at = np.flatnonzero((body[:-1] == 0xFF) & (body[1:] >= 0xD0) & (body[1:] <= 0xD7))
    return [(int(a) + sc["start"], int(body[a + 1]) - 0xD0) for a in at]


def with_wrong_rst(data, scan=0):
    """the file with every RSTm of the scan after the first wrap (marker k >= 8) numbered (k + 1) & 7"""
    out = bytearray(data)
    for k, (a, m) in enumerate(rst_markers(data, scan)):
        assert m == k & 7
        if k >= 8:
            out[a + 1] = 0xD0 + ((k + 1) & 7)
    return bytes(out)


def last_block_column_zeroed(planes):
    out = [np.array(p) for p in planes]
    for p in out:
        p[:, -8:] = 0
    return out


def block_rows_shifted(planes, first=4096):
    """block rows `first` and above moved down by one (the last falls off, row `first` stays twice)"""
    out = [np.array(p) for p in planes]
    for p in out:
        if p.shape[0] > (first + 1) * 8:
            p[(first + 1) * 8:] = np.array(p[first * 8:-8])
    return out


@functools.lru_cache(None)
def pillow_strip(W, H, grey, **kw):
    """Pillow's file of the noisy photo of that size (YCbCr in, so libjpeg converts nothing)"""
    import io
    from PIL import Image
    case = JS.explicit_case("pillow", W, H, "grey" if grey else "4:2:0", picture_seed=50)
    pic = JS.picture(case)
    buf = io.BytesIO()
    Image.fromarray(pic, "L" if grey else "YCbCr").save(buf, "JPEG", quality=QUALITY, **({} if grey else dict(subsampling=2)), **kw)
    return buf.getvalue()
