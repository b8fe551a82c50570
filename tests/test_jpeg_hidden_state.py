"""The JPEG entry points against what a caller does not choose: what their scratch memory held, and whether a repeat gives the same
bytes.  All GPU; the harness's own tests are test_poisoned_alloc.py, the barriers' test_barrier_waits.py.

1. The 40 calls of test_jpeg_streams.CASES (its 34 host calls and the six asynchronous wrappers) under tests/poisoned_alloc.py, each
   under each of its four patterns: every torch.empty of the call holds the pattern and lies between canaries.  Truth: the call's un-poisoned null-stream outcome, which _prepare holds to
   its checkers -- a file, tensors, or an exception type with its status list.  A tally the case names must hold, no guard byte may
   have changed.  And one arrangement without the harness, "after another picture": the same entry point first runs on a different
   picture or file of the same geometry (the catalogue's makers under other seeds), its results are freed, and the call proper must
   give its truth -- the stale data a real caller meets.  For hostile-* the first call is the legal file, and the order is reversed too.
2. The committed sweep (test_jpeg_sweep.py: seed 171's 16 blocks, the PINNED cases) under "rnd" seeded by the block number, through
   test_jpeg_sweep.gpu_block / gpu_pinned: the sweep's own checks are the truth.
3. The five broken files of test_jpeg_decode_batch.py between two intact ones through decode_jpeg_batch(on_error="return") under
   "00" and "ff": the same list as un-poisoned, the intact neighbours torch.equal to decode_jpeg alone.
4. Repeats: one 2048 x 2048 picture (synth's photo planes with noise added) at quality 95, where a luma chunk of 256 blocks takes
   about 8 KB, two windows of a 1024-word ring and more (asserted from the luma scan's length); sixteen entry-point forms, and
   grey noise at quality 100 for the second packing pass, which quality 95 never reaches, each REPS[form] times, every result
   compared with the first (files byte for byte, tensors with torch.equal on the device; one synchronize per comparison).  The
   first result is also opened by Pillow (files) or compared with the same decode after torch.cuda.empty_cache() -- the allocator
   hands out fresh memory -- and with what a second route gives (tensors), so that "all equal" cannot mean "all equally wrong".
   MDCT_SOAK_JPEG_REPEAT=<reps>: the same cases with that count in one opt-in test, ended by the first difference.

Every GPU call here ends with a synchronise before anything is freed or compared."""
import contextlib
import functools
import io
import os
import time

import numpy as np
import pytest
from PIL import Image  # the repeats' first results are read by Pillow: without it this file is an error, not a skip

import jpeg_scan_encoder as E
import test_jpeg_streams as S
import test_jpeg_sweep as SW
from poisoned_alloc import PATTERNS, poisoned
from simd_dct_amd import api, synth
from test_jpeg_streams import CASES, _brief, _outcome, _prepare, _same


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    torch.cuda.set_device(0)
    api.init(0)
    return torch


# ------------------------------------------------------------------------------------------ 1. the catalogue under the harness
def run_poisoned(torch, name, pattern):
    c = CASES[name]
    fn, truth, _ = _prepare(torch, name)
    torch.cuda.synchronize()
    if c.tally:
        api.kernel_counts_reset()
    with poisoned(pattern, seed=sorted(CASES).index(name), strict=False) as p:
        got = _outcome(lambda: fn(None))
        torch.cuda.synchronize()
    problems = list(p.damage)
    print(f"\n{name} under {pattern}: {len(p.blocks)} requests, {sum(n for _, n, _ in p.blocks)} bytes, outcome {got[0]}")
    if not p.blocks and got[0] != "MdctError":  # (a loss is refused from the zeroed words, before anything else is asked for)
        problems.append("the call asked torch.empty for nothing: the harness saw none of its memory")
    if not _same(got, truth):
        problems.append(f"{_brief(got)} differs from the un-poisoned call's {_brief(truth)}")
    if c.tally and api.kernel_counts().get(c.tally[0], 0) != c.tally[1]:
        problems.append(f"{c.tally[0]} ran {api.kernel_counts().get(c.tally[0], 0)} times, not {c.tally[1]}")
    assert not problems, f"{name} under {pattern}: " + "; ".join(problems)


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("name", list(CASES))
def test_a_call_on_poisoned_scratch(gpu, name, pattern):
    run_poisoned(gpu, name, pattern)


class _OtherSynth:
    """synth with every seed moved: another picture of the same geometry"""

    def __getattr__(self, name):
        fn = getattr(synth, name)
        if not name.startswith("plane_"):
            return fn
        return lambda W, H, kind="noise", seed=synth.SEED, **kw: fn(W, H, kind, seed + 1000, **kw)


_periodic = S._periodic  # (the name is replaced while other_picture() is active)


@functools.lru_cache(None)
def _other_periodic():
    """_periodic's scan with every level negated: the same code lengths, so the same 64 bits per block and the same chunk geometry"""
    data, planes = _periodic()
    comps = [(2, 2), (2, 1), (1, 1)]
    other = [(-p).astype(np.int16) for p in planes]
    out, st = E.encode_file(dict(width=16 * S.PERIODIC_MCUS, height=16, comps=comps), [dict(comps=[(0, 0, 0), (1, 0, 0), (2, 0, 0)], dri=0)], other,
                            {k: E.ANNEX_K[k] for k in ((0, 0), (1, 0))})
    assert st[0]["max_block_bits"] == 64 and st[0]["length"] == 8 * 7 * S.PERIODIC_MCUS and not st[0]["stuffed"] and len(out) == len(data) and out != data
    return out, other


_OTHER = {"synth": _OtherSynth(), "_periodic": _other_periodic,
          **{n: functools.lru_cache(None)(getattr(S, n).__wrapped__) for n in ("_image", "_files", "_coefs")}}


@contextlib.contextmanager
def other_picture():
    """test_jpeg_streams' makers see another picture (file, coefficient planes, scan) of the same geometry"""
    kept = {n: getattr(S, n) for n in _OTHER}
    for n, v in _OTHER.items():
        setattr(S, n, v)
    try:
        yield
    finally:
        for n, v in kept.items():
            setattr(S, n, v)


_others = {}


def _other(torch, name):
    if name not in _others:
        with other_picture():
            _others[name] = CASES[name].make(torch)
        torch.cuda.synchronize()
    return _others[name]


def after(torch, first_call, name, first_is_another_picture):
    """first_call(), its results freed, then the case's call: its truth, its tally"""
    c = CASES[name]
    fn, truth, _ = _prepare(torch, name)
    torch.cuda.synchronize()
    first = _outcome(first_call)
    torch.cuda.synchronize()
    assert first[0] != "JpegDecodeError" or not first_is_another_picture, first
    if first_is_another_picture and first[0] == "ok":
        assert truth[0] == "ok" and not _same(first, truth), f"{name}: the first call's picture gave the outcome of the call proper"
    shown = _brief(first)
    del first  # back to the caching allocator, with what the first call left in its scratch
    if c.tally:
        api.kernel_counts_reset()
    got = _outcome(lambda: fn(None))
    torch.cuda.synchronize()
    print(f"\n{name}: first {shown}, then {got[0]}")
    assert _same(got, truth), f"{name} after another call: {_brief(got)} differs from {_brief(truth)}"
    if c.tally:
        assert api.kernel_counts().get(c.tally[0], 0) == c.tally[1], (c.tally, api.kernel_counts())


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_a_call_after_another_picture(gpu, name):
    torch = gpu
    if name.startswith("hostile-"):
        legal = _prepare(torch, "decode-" + name[len("hostile-"):] + "-planes")[0]  # the legal file of the route, the same decode_jpeg call
        after(torch, lambda: legal(None), name, False)
    else:
        other = _other(torch, name)
        after(torch, lambda: other(None), name, True)


@pytest.mark.gpu
@pytest.mark.parametrize("route", S.ROUTES)
def test_a_legal_file_after_the_hostile_one(gpu, route):
    hostile = _prepare(gpu, "hostile-" + route)[0]
    after(gpu, lambda: hostile(None), f"decode-{route}-planes", False)


# ------------------------------------------------------------------------------------------ 2. the sweep under "rnd"
@pytest.fixture(scope="module")
def engine(gpu):
    return SW.Engine(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("b", range(SW.N_BLOCKS))
def test_a_block_of_the_sweep_on_poisoned_scratch(engine, b):
    with poisoned("rnd", seed=b) as p:
        SW.gpu_block(engine, b)
        engine.torch.cuda.synchronize()
    assert len(p.blocks) > 12 * 10, len(p.blocks)


@pytest.mark.gpu
def test_the_pinned_cases_on_poisoned_scratch(engine):
    with poisoned("rnd", seed=SW.N_BLOCKS) as p:
        SW.gpu_pinned(engine)
        engine.torch.cuda.synchronize()
    assert p.blocks


# ------------------------------------------------------------------------------------------ 3. a broken file between two intact ones
@pytest.mark.gpu
@pytest.mark.parametrize("pattern", ["00", "ff"])
@pytest.mark.parametrize("kind", ["truncated", "marker removed", "marker surplus", "corrupted code", "12-bit"])
def test_a_broken_file_between_two_intact_ones_on_poisoned_scratch(gpu, kind, pattern):
    import test_jpeg_decode_batch as B
    from simd_dct_amd import jpeg_decode as D
    torch = gpu
    files = [B.FILES()[2], B._broken()[kind], B.FILES()[7]]
    want = D.decode_jpeg_batch(files, coefficients=True, on_error="return")
    torch.cuda.synchronize()
    assert isinstance(want[1], Exception) and want[1].file == 1
    with poisoned(pattern, seed=1, strict=False) as p:
        got = D.decode_jpeg_batch(files, coefficients=True, on_error="return")
        torch.cuda.synchronize()
    assert not p.damage, p.damage
    assert p.blocks and len(got) == 3
    assert B.same_error(got[1], want[1]) and got[1].file == 1, (got[1], want[1])
    for i in (0, 2):
        assert B.same(torch, got[i], want[i]), i
        kind_alone, alone = B.alone(torch, files[i], coefficients=True)
        assert kind_alone == "ok" and B.same(torch, got[i], alone), i


# ------------------------------------------------------------------------------------------ 4. repeats
SIDE = 2048
QUALITY = 95
CROPS = [(0, 0, 1024, 768), (40, 8, 801, 601), (512, 1024, 640, 480), (1500, 1000, 513, 1023), (7, 1200, 333, 777), (1024, 0, 256, 256), (1000, 2000, 1000, 40),
         (1900, 16, 97, 1200)]  # x, y, width, height
# calls per test: the largest round count that keeps the test at about 4 s (under 5 on a slow clock) at the time per call and comparison
# measured on the MI355X, never fewer than 20 (tests/README.md has the times)
REPS = {"encode-default": 3000, "encode-one-launch": 4000, "encode-interleaved": 5000, "encode-optimize": 3500, "encode-optimize-interleaved": 4000,
        "encode-progressive": 2500, "encode-standard-script": 2000, "encode-444-chw": 2000, "decode-marked": 1000, "decode-unmarked": 550,
        "decode-approximation": 130, "decode-half": 1000, "transcode-rot90": 900, "transcode-standard-script": 800, "decode-batch": 750, "encode-batch": 3500,
        "encode-second-pack": 1000}


@functools.lru_cache(None)
def picture():
    """[2048, 2048, 3] on the device: synth's photo planes, noise of +-16 added"""
    import torch
    planes = [synth.plane_u8_torch(SIDE, SIDE, "photo", seed=60 + k).to(torch.int16) + (synth.plane_u8_torch(SIDE, SIDE, "noise", seed=70 + k) >> 3).to(torch.int16) - 16
              for k in range(3)]
    img = torch.stack(planes, dim=-1).clamp_(0, 255).to(torch.uint8).contiguous()
    torch.cuda.synchronize()
    return img


@functools.lru_cache(None)
def source(kind):
    """the files the decoders and transcoders repeat on"""
    from simd_dct_amd import jpeg_decode as D
    from simd_dct_amd import jpeg_encode as J
    import torch
    if kind == "marked":
        data = J.encode_jpeg(picture(), QUALITY)
    elif kind == "approximation":
        data = J.encode_jpeg(picture(), QUALITY, progressive=True, script="standard")
    elif kind == "unmarked":
        buf = io.BytesIO()
        Image.fromarray(picture().cpu().numpy(), "RGB").save(buf, "JPEG", quality=QUALITY)
        data = buf.getvalue()
    torch.cuda.synchronize()
    info = D.read_file(data)
    assert (info["sof"] == 0xC2) == (kind == "approximation") and all((s["restart_interval"] > 0) == (kind != "unmarked") for s in info["scans"])
    return data


@functools.lru_cache(None)
def crops():
    import torch
    out = [picture()[y:y + h, x:x + w] for x, y, w, h in CROPS]
    assert len({c.shape for c in out}) == len(CROPS) and all(c.shape == (h, w, 3) for c, (_, _, w, h) in zip(out, CROPS))
    torch.cuda.synchronize()
    return out


@functools.lru_cache(None)
def crop_files():
    from simd_dct_amd import jpeg_encode as J
    import torch
    files = [J.encode_jpeg(c.contiguous(), QUALITY) for c in crops()]
    torch.cuda.synchronize()
    return files


def opened_by_pillow(data, width, height, grey=False):
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.size == (width, height) and im.mode == ("L" if grey else "RGB"), (im.size, im.mode)
    return np.asarray(im)


def close_to_the_picture(rgb, want, what):
    """a decode of the quality-95 file is the picture again.  Per pixel only in luma (0.299 R + 0.587 G + 0.114 B, on which the chroma
    cancels): 4:2:0 averages the chroma of this noisy picture away, about 11 grey levels of R, G, B by libjpeg's own round trip.  The luma
    quantiser's largest step at quality 95 is 12, so a coefficient is off by at most 6 and, a uniform error taken for every step, by
    12 / sqrt(12) = 3.5 RMS, which Parseval carries to the pixels; with the roundings of the IDCT and the colour conversion: mean
    absolute error < 5.  The chroma in the means of 16 x 16 tiles, which the 2 x 2 averaging keeps: the DC steps are 2, so a tile's mean
    is off by at most 1 / 8 per component, (1 + 1.772) / 8 = 0.35 in B, plus what the upsampling filter carries across a tile's
    border: mean absolute error < 1.  (libjpeg's round trip of this picture: 1.6 and 0.07.  A wrong plane, a shifted row or a lost
    interval is far above both.)"""
    e = rgb.astype(np.float64) - want.astype(np.float64)
    luma = np.abs(e @ np.array([0.299, 0.587, 0.114])).mean()
    h, w = e.shape[0] // 16 * 16, e.shape[1] // 16 * 16
    tiles = np.abs(e[:h, :w].reshape(h // 16, 16, w // 16, 16, 3).mean(axis=(1, 3))).mean()
    print(f"{what}: mean absolute error {luma:.2f} in luma, {tiles:.3f} in the means of 16 x 16 tiles")
    assert luma < 5.0 and tiles < 1.0, f"{what}: mean absolute error {luma:.2f} in luma, {tiles:.3f} in the tile means, against the picture"


RING_BYTES = 4 * 1024  # kFusedRing, kRing: the words of bit stream the pixel, coefficient and batch coders hold in LDS per window


def several_ring_windows(data):
    """the default form's first scan is the luma plane's, a restart interval and a chunk of 256 blocks per block row: its mean bytes
    per chunk against the ring.  (libjpeg codes this luma plane into about 8.3 KB per 256 blocks.)"""
    from simd_dct_amd import jpeg_decode as D
    sc = D.read_file(data)["scans"][0]
    assert sc["restart_interval"] == SIDE // 8 == 256
    per_chunk = (sc["end"] - sc["start"]) / (SIDE // 8)
    print(f"luma scan: {per_chunk:.0f} bytes per chunk of 256 blocks, {per_chunk / RING_BYTES:.2f} windows of {RING_BYTES} bytes")
    assert per_chunk > 1.5 * RING_BYTES, f"{per_chunk:.0f} bytes per chunk: the repeats' chunks fit one or two ring windows"


def _encode_form(**kw):
    def make(torch):
        from simd_dct_amd import jpeg_encode as J
        img = picture().permute(2, 0, 1).contiguous() if kw.get("layout") == "CHW" else picture()
        want = picture().cpu().numpy()

        def check(first):
            close_to_the_picture(opened_by_pillow(first, SIDE, SIDE), want, "Pillow's decode")
            if not kw:
                several_ring_windows(first)
        return (lambda: J.encode_jpeg(img, QUALITY, **kw)), check
    return make


def _decode_form(kind, **kw):
    def make(torch):
        from simd_dct_amd import jpeg_decode as D
        data = source(kind)

        def check(first):
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            again = D.decode_jpeg(data, **kw)
            torch.cuda.synchronize()
            assert _same(first, again), "the first result differs from the same decode on fresh memory"
            rgb = first[0] if kw.get("coefficients") else first
            if kw.get("scale_denom", 1) == 1:
                close_to_the_picture(rgb.cpu().numpy(), picture().cpu().numpy(), f"decode_jpeg of the {kind} file")
            if kind == "approximation":  # the same picture, quality and quantiser as the restart-marked file: another decoder, the same tensors
                other = D.decode_jpeg(source("marked"), **kw)
                torch.cuda.synchronize()
                assert _same(first, other), "the successive-approximation file and the restart-marked file of one picture decode differently"
        return (lambda: D.decode_jpeg(data, **kw)), check
    return make


def _transcode_form(kw, width, height):
    def make(torch):
        from simd_dct_amd import jpeg_decode as D
        from simd_dct_amd import jpeg_transcode as T
        data = source("marked")

        def check(first):
            opened_by_pillow(first, width, height)
            if not kw.get("transform"):  # the coefficients went through untouched
                got, want = D.decode_coefficients(first)[1], D.decode_coefficients(data)[1]
                torch.cuda.synchronize()
                assert _same(got, want)
        return (lambda: T.transcode_jpeg(data, **kw)), check
    return make


def _decode_batch(torch):
    from simd_dct_amd import jpeg_decode as D
    files = crop_files()

    def check(first):
        for f, got in zip(files, first):
            want = D.decode_jpeg(f, coefficients=True, mode="RGB")
            torch.cuda.synchronize()
            assert _same(got, want)
    return (lambda: D.decode_jpeg_batch(files, coefficients=True, mode="RGB")), check


def _encode_batch(torch):
    from simd_dct_amd import jpeg_encode as J
    images = crops()

    def check(first):
        for img, data, (_, _, w, h) in zip(images, first, CROPS):
            close_to_the_picture(opened_by_pillow(data, w, h), img.cpu().numpy(), "Pillow's decode of a batch file")
            assert data == J.encode_jpeg(img.contiguous(), QUALITY, interleaved=True)
        torch.cuda.synchronize()
    return (lambda: J.encode_jpeg_batch(images, QUALITY)), check


def _second_pack(torch):
    """Quality 95 never fills a scan's first buffer of pixels + 4096 bytes (this picture: 0.58 bytes per pixel; noise over the whole
    range: 0.99), so none of the sixteen forms above runs the second packing pass.  This one does: grey noise at quality 100, about
    1.6 bytes per pixel, no front launch; k_pack_write<true> runs twice per call."""
    from simd_dct_amd import jpeg_encode as J
    img = synth.plane_u8_torch(SIDE, SIDE, "noise", seed=77)
    want = img.cpu().numpy()

    def check(first):
        assert len(first) > SIDE * SIDE + 4096
        got = opened_by_pillow(first, SIDE, SIDE, grey=True)
        err = np.abs(got.astype(np.int16) - want).mean()  # quality 100: every quantiser step is 1, a coefficient is off by at most 1 / 2
        assert err < 1.0, f"Pillow's decode of the quality-100 file: mean absolute error {err:.2f}"
        api.kernel_counts_reset()
        J.encode_jpeg(img, quality=100)
        torch.cuda.synchronize()
        assert api.kernel_counts().get("k_pack_write<true>", 0) == 2, api.kernel_counts()
    return (lambda: J.encode_jpeg(img, quality=100)), check


COEFS_RGB = dict(coefficients=True, mode="RGB")
REPEATS = {
    "encode-default": _encode_form(), "encode-one-launch": _encode_form(two_launch=False), "encode-interleaved": _encode_form(interleaved=True),
    "encode-optimize": _encode_form(optimize=True), "encode-optimize-interleaved": _encode_form(optimize=True, interleaved=True),
    "encode-progressive": _encode_form(progressive=True), "encode-standard-script": _encode_form(progressive=True, script="standard"),
    "encode-444-chw": _encode_form(subsampling="4:4:4", layout="CHW"),
    "decode-marked": _decode_form("marked", **COEFS_RGB), "decode-unmarked": _decode_form("unmarked", **COEFS_RGB),
    "decode-approximation": _decode_form("approximation", **COEFS_RGB), "decode-half": _decode_form("marked", scale_denom=2),
    "transcode-rot90": _transcode_form(dict(transform="rot90", trim=True), SIDE, SIDE),
    "transcode-standard-script": _transcode_form(dict(progressive=True, script="standard"), SIDE, SIDE),
    "decode-batch": _decode_batch, "encode-batch": _encode_batch, "encode-second-pack": _second_pack,
}
assert set(REPEATS) == set(REPS) and min(REPS.values()) >= 20


def _equal(a, b):
    return a == b if isinstance(a, (bytes, bytearray)) else _same(a, b)


def repeat(torch, name, reps):
    """the call `reps` times, every result against the first -> (seconds of one warm call, seconds in all)"""
    call, check = REPEATS[name](torch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    first = call()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    warm = t1 - t0  # (reps = 1: the only call there is)
    for r in range(1, reps):
        t = time.perf_counter()
        got = call()
        torch.cuda.synchronize()
        if r == 1:
            warm = time.perf_counter() - t
        assert _equal(got, first), f"{name}: call {r} of {reps} differs from call 0: {_brief(got)} against {_brief(first)}" + _where(got, first)
        del got
    t2 = time.perf_counter()
    check(first)
    torch.cuda.synchronize()
    print(f"\nrepeat {name}: first call {1e3 * (t1 - t0):.1f} ms, warm call {1e3 * warm:.1f} ms, {reps} calls and comparisons {t2 - t0:.2f} s, "
          f"the first result's check {time.perf_counter() - t2:.2f} s")
    return warm, t2 - t0


def _where(got, first):
    """for two files: where they first differ (the scan boundaries are in the file)"""
    if not isinstance(got, (bytes, bytearray)):
        return ""
    n = next((i for i, (x, y) in enumerate(zip(got, first)) if x != y), min(len(got), len(first)))
    return f"; first different byte {n} of {len(got)} / {len(first)}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(REPEATS))
def test_a_repeated_call_gives_the_same_bytes(gpu, name):
    repeat(gpu, name, REPS[name])


@pytest.mark.gpu
@pytest.mark.skipif(not os.environ.get("MDCT_SOAK_JPEG_REPEAT"), reason="opt-in soak: MDCT_SOAK_JPEG_REPEAT=<reps> python -m pytest tests -m gpu -k soak_of_the_repeats")
def test_gpu_soak_of_the_repeats(gpu):
    """opt-in long run: the seventeen repeat cases with MDCT_SOAK_JPEG_REPEAT calls each, in this one process; the first difference ends it.
    MDCT_SOAK_JPEG_REPEAT_PROGRESS: a file that gets one line per case (a watched box)."""
    reps, progress = int(os.environ["MDCT_SOAK_JPEG_REPEAT"]), os.environ.get("MDCT_SOAK_JPEG_REPEAT_PROGRESS")
    t0 = time.time()
    for name in REPEATS:
        warm, total = repeat(gpu, name, reps)
        if progress:
            with open(progress, "a") as f:
                f.write(f"{name}: {reps} calls identical in {total:.1f} s (one warm call {1e3 * warm:.1f} ms); {time.time() - t0:.0f} s so far\n")
    print(f"soak: {len(REPEATS)} cases x {reps} calls, every result equal to its first, in {time.time() - t0:.0f} s")
