"""The JPEG file entry points -- encode_jpeg, decode_jpeg, transcode_jpeg and both batches -- over the seeded random geometry of
tests/jpeg_sweep.py: 192 drawn cases in 16 blocks of 12, every stage of every case held to the truths the suite already trusts.

CPU half: the stand-in engine of test-side pieces passes every check of every case of the committed draw (which proves the draw, the
checks and the tie-window caps from the reference alone); the draw holds the combinations it was made for (coverage_failures); six
faults planted in the stand-in each fail at least three cases; the draw is reproducible.
GPU half: simd_dct_amd through the same code; PINNED cases; the opt-in soak MDCT_SOAK_JPEG_FILES=<cases> over fresh draws."""
import functools
import hashlib
import os

import numpy as np
import pytest

import jpeg_decode_checker as DC
import jpeg_progressive_checker as PC
import jpeg_sweep as JS

pytest.importorskip("PIL.Image")

SEED, CASES = 171, 192  # the committed draw: the first seed from 1 up whose 192 cases meet every condition of coverage_failures
# cases the soak found failing, as (seed, k): the default run executes them too
PINNED = [
    (1, 190),  # a 1 x 1 CHW picture whose one-element dimensions carry HWC's strides: encode_jpeg refused it
    (1, 1420),  # a flat 2061 x 12 picture whose chroma dequantises onto n + 1/2 throughout: no engine's fault, the cap's (the same section)
]
# sha256 of the committed cases' printed forms: the draw may not drift under a case that once failed
DIGEST = "d060300a5c3fc4106557ddbb1f40b703f7eeb4c02a0e1cf5d3be12e3c7422e03"


@functools.lru_cache(None)
def committed():
    return [JS.draw(SEED, k) for k in range(CASES)]


def block(b):
    return committed()[b * JS.BLOCK:(b + 1) * JS.BLOCK]


N_BLOCKS = CASES // JS.BLOCK


# ------------------------------------------------------------------------------------------ CPU: the draw
def test_the_draw_is_reproducible_and_has_not_drifted():
    again = [JS.draw(SEED, k) for k in range(CASES)]
    assert again == committed() and [repr(c) for c in again] == [repr(c) for c in committed()]
    assert all((c["seed"], c["k"]) == (SEED, k) for k, c in enumerate(again))
    assert JS.draw(SEED + 1, 0) != JS.draw(SEED, 0)
    digest = hashlib.sha256("\n".join(repr(c) for c in again).encode()).hexdigest()
    assert digest == DIGEST, digest


def test_every_drawn_script_is_one_the_engine_accepts():
    from simd_dct_amd import jpeg_progressive as P
    n = 0
    for c in committed():
        nc_enc, nc_src = len(JS.SAMPLINGS[c["enc_sampling"]]), len(JS.SAMPLINGS[JS.source_frame(c)[2]])
        for script, nc in ((c["script"], nc_enc), (c.get("written", {}).get("script"), nc_src), (c["transcode"]["script"], nc_src)):
            if isinstance(script, list):
                assert P.check_script(script, nc) == script, JS.label(c)
                first = [al for _, _, _, ah, al in script if ah == 0]
                assert 0 <= min(first) and max(first) <= 3 and 1 <= sum(1 for comps, ss, _, ah, _ in script if ss and comps == (0,) and ah == 0) <= 4, JS.label(c)
                n += 1
    assert n >= 40, n
    for nc in (1, 3):
        assert P.standard_script(nc) == JS.STANDARD[nc]
        for inter in (False, True):
            assert P.bands_script(P.check_bands(None, nc), nc, inter and nc == 3) == JS.resolve_script(None, nc, inter)


def test_the_committed_draw_holds_the_combinations_it_was_made_for():
    assert JS.coverage_failures(committed()) == []
    # and the same statement notices what is missing
    assert any("1 x 1" in f for f in JS.coverage_failures([c for c in committed() if (c["W"], c["H"]) != (1, 1)]))
    accepted = [c for c in committed() if JS.refusal(c["W"], c["H"], JS.SAMPLINGS[JS.source_frame(c)[2]], c["transcode"]["transform"], c["transcode"]["trim"]) is None]
    assert 0 < len(committed()) - len(accepted) <= CASES // 4 and any("refused" in f for f in JS.coverage_failures(accepted))
    assert any("DRI class 0" in f for f in JS.coverage_failures([c for c in committed() if c.get("written", {}).get("dri") != 0]))


def test_the_quality_tables_are_libjpegs():
    """the IJG scaling restated in jpeg_sweep against libjpeg itself (Pillow)"""
    import io
    from PIL import Image
    for quality in JS.QUALITIES:
        buf = io.BytesIO()
        Image.fromarray(np.zeros((8, 8, 3), dtype=np.uint8), "RGB").save(buf, "JPEG", quality=quality)
        _, qt, _, _ = PC.parse(buf.getvalue())
        for k, want in enumerate(JS.quality_tables(quality)):
            assert np.array_equal(np.array(qt[k]), want), (quality, k)


def test_the_restated_serial_decoder_is_the_checker():
    """jpeg_sweep.serial_baseline exists for scans without restart markers; on files with them it is jpeg_decode_checker.decode"""
    seen = 0
    for c in committed()[:60]:
        if c["source"] == "written" and c["written"]["sof"] == 0 and not c["wide"]:
            data, planes = JS.written_file(c)
            got, statuses = JS.serial_baseline(data)
            assert all(s == 0 for st in statuses for s in st) and all(np.array_equal(g, w) for g, w in zip(got, planes)), JS.label(c)
            if c["written"]["dri"] != 0:
                want, st, _ = DC.decode(data)
                assert st == statuses and all(np.array_equal(g, w) for g, w in zip(got, want)), JS.label(c)
                seen += 1
    assert seen >= 5


# ------------------------------------------------------------------------------------------ CPU: the stand-in through every check
@pytest.mark.parametrize("b", range(N_BLOCKS))
def test_the_stand_in_passes_every_check(b):
    """... and the planes of the draw stay inside the tie-window caps: from the reference alone"""
    pool = JS.run_block(JS.StandIn(), block(b))
    assert set(pool.sums) <= {"forward", "inverse", "scaled 1", "scaled 2", "scaled 4", "scaled 8"}, pool.sums


@functools.lru_cache(None)
def clean_source(k):
    """(own file, its planes, source file, its planes) of committed case k by the correct stand-in"""
    case = committed()[k]
    sub = "4:2:0" if case["enc_sampling"] == "grey" else case["enc_sampling"]
    own = JS.StandIn().encode(JS.laid_out(JS.picture(case), case["layout"]), case["quality"], sub, case["layout"], **JS.encode_form(case))
    C_own = JS.checker_decode(own)[0]
    return (own, C_own) + tuple(JS.source_of(case, own, C_own))


def fires(fault, case):
    """where the planted fault can change what the stand-in does; everywhere else the faulty stand-in is the correct one, line for line"""
    W, H, name = JS.source_frame(case)
    sampling = JS.SAMPLINGS[name]
    t = case["transcode"]
    refused = JS.refusal(W, H, sampling, t["transform"], t["trim"]) is not None
    if fault in JS.FAULTS[:2]:
        return JS.source_kind(case) != "progressive" and any(not inter for *_, inter in JS.source_scans(case))
    if fault == JS.FAULTS[2]:
        return not refused and t["transform"] is not None and "y" in JS.X.MIRRORED[t["transform"]]
    if fault == JS.FAULTS[3]:
        return not refused and t["transform"] in JS.X.TRANSPOSING
    if fault == JS.FAULTS[4]:
        return case["layout"] == "CHW" and case["enc_sampling"] != "grey"
    return True


@pytest.mark.parametrize("fault", JS.FAULTS)
def test_a_planted_fault_fails_cases_of_the_draw(fault):
    """each of the six faults, planted in the stand-in, is caught by at least three cases of the committed draw"""
    engine = JS.StandIn(faults=(fault,))
    failing = []
    for k, case in enumerate(committed()):
        if not fires(fault, case):
            continue
        try:
            if fault == JS.FAULTS[4]:
                JS.stage_encode(engine, case)
            else:
                _, _, data, C = clean_source(k)
                (JS.stage_transcode if fault in JS.FAULTS[2:4] else JS.stage_decode)(engine, case, data, C)
        except AssertionError:
            failing.append(k)
    print(f"{fault}: {len(failing)} cases fail: k = {failing}")
    assert len(failing) >= 3, (fault, failing)


def test_a_plane_under_the_cap_is_the_references_own_statement():
    """PINNED (1, 1420), which ended a soak: the flat picture's Cb is 142, its DC level 12 under quality 75's 9 and 12 * 9 / 8 + 128 = 141.5 in
    every sample of the plane.  The stand-in, which is the reference, misses the cap in the same plane; where the soak goes on"""
    case = JS.draw(1, 1420)
    with pytest.raises(JS.CaseFailure, match="decode plane 1") as e:
        JS.run_case(JS.StandIn(), case, JS.Pool())
    assert isinstance(e.value.__cause__, JS.CapMiss)
    pool = JS.Pool(strict=False)
    JS.run_case(JS.StandIn(), case, pool)
    # (at 1/2 the chroma of a 4:2:0 file keeps its 8 x 8 blocks: the same plane again)
    assert pool.missed == [("(seed, k) = (1, 1420) decode plane 1", 0.0), ("(seed, k) = (1, 1420) decode plane 1 at 1/2", 0.0)]


def test_a_failure_shows_seed_k_and_the_case():
    case = next(c for c in committed() if fires(JS.FAULTS[4], c))
    with pytest.raises(JS.CaseFailure) as e:
        JS.run_case(JS.StandIn(faults=(JS.FAULTS[4],)), case)
    assert f"(seed, k) = ({SEED}, {case['k']})" in str(e.value) and repr(case) in str(e.value)


def test_the_stride_of_a_one_element_dimension_is_not_the_images_layout():
    """what PINNED (1, 190) found: a 1 x 1 picture moved from HWC to CHW keeps HWC's strides on its two
    one-element dimensions, numpy and torch call it contiguous, and encode_jpeg took stride(2) = 3 for a layout it refuses"""
    torch = pytest.importorskip("torch")
    from simd_dct_amd import jpeg_encode as J
    case = JS.draw(*PINNED[0])
    image = JS.laid_out(JS.picture(case), case["layout"])
    assert image.shape == (3, 1, 1) and image.flags["C_CONTIGUOUS"] and image.strides == (1, 3, 3)
    t = torch.from_numpy(image)
    assert t.is_contiguous() and t.stride() == (1, 3, 3)
    assert J._input_of(t, "CHW") == (1, 1)
    assert J._input_of(torch.zeros((1, 1, 3), dtype=torch.uint8), "HWC") == (3, 0)
    assert J._input_of(torch.zeros((5, 1, 3), dtype=torch.uint8).permute(2, 0, 1), "CHW") == (3, 1)  # (the library refuses these overlapping planes)
    assert J._input_of(torch.zeros((1, 7), dtype=torch.uint8).t(), "HWC", grey=True) == (1, 0)  # [7, 1] with strides (1, 7)
    for bad, layout in ((torch.zeros((4, 6, 3), dtype=torch.uint8).permute(2, 0, 1), "CHW"), (torch.zeros((3, 4, 6), dtype=torch.uint8).permute(1, 2, 0), "HWC"),
                        (torch.zeros((4, 12), dtype=torch.uint8)[:, ::2], "HWC")):
        with pytest.raises(ValueError, match="contiguous innermost"):
            J._input_of(bad, layout, grey=bad.dim() == 2)


# ------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    from simd_dct_amd import api
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    torch.cuda.set_device(0)
    api.init(0)
    return Engine(torch)


class Engine:
    """simd_dct_amd behind the engine interface of jpeg_sweep: results come back as numpy"""

    def __init__(self, torch):
        from simd_dct_amd import api, jpeg_decode, jpeg_encode, jpeg_transcode
        self.torch, self.api, self.D, self.J, self.TC = torch, api, jpeg_decode, jpeg_encode, jpeg_transcode

    @staticmethod
    def _np(out):
        return out.cpu().numpy() if hasattr(out, "cpu") else [p.cpu().numpy() for p in out]

    def encode(self, image, quality, subsampling, layout, **form):
        return self.J.encode_jpeg(image, quality, subsampling, layout, **form)

    def decode(self, data, mode=None, layout="HWC", scale_denom=1):
        out, coefs = self.D.decode_jpeg(data, coefficients=True, mode=mode, layout=layout, scale_denom=scale_denom)
        return self._np(out), self._np(coefs)

    def transcode(self, data, transform=None, trim=False, optimize=True, interleaved=False, progressive=False, script=None):
        W, H, sampling, _, _ = JS.decoded_frame(data)
        try:
            return self.TC.transcode_jpeg(data, transform=transform, trim=trim, optimize=optimize, interleaved=interleaved, progressive=progressive, script=script)
        except ValueError as e:
            # where plan_transform raises on the host, the call raises the same ValueError
            with pytest.raises(ValueError) as host:
                self.TC.plan_transform(W, H, sampling, transform, trim)
            assert type(e) is ValueError and str(e) == str(host.value), (str(e), str(host.value))
            raise

    def decode_batch(self, files, mode, layout):
        """the restart-marked baseline files take the batch path: k_decode_batch is in the launch tally once; and every tensor is
        torch.equal to decode_jpeg's on the file alone"""
        torch = self.torch
        on_path = [PC.parse(bytes(f))[0]["sof"] != 0xC2 and all(sc["dri"] for sc in PC.parse(bytes(f))[2]) for f in files]
        torch.cuda.synchronize()
        self.api.kernel_counts_reset()
        batch = self.D.decode_jpeg_batch(files, mode=mode, layout=layout, coefficients=True)
        torch.cuda.synchronize()
        ran = self.api.kernel_counts()
        assert ran.get("k_decode_batch", 0) == (1 if any(on_path) else 0), (ran, on_path)
        for data, (out, coefs) in zip(files, batch):
            one, one_coefs = self.D.decode_jpeg(data, coefficients=True, mode=mode, layout=layout)
            pairs = [(out, one)] if mode == "RGB" else list(zip(out, one))
            assert all(torch.equal(g, w) for g, w in pairs + list(zip(coefs, one_coefs)))
        return [(self._np(out), self._np(coefs)) for out, coefs in batch]

    def encode_batch(self, images, quality, subsampling, layout):
        return self.J.encode_jpeg_batch(images, quality, subsampling, layout)


def gpu_block(engine, b):
    """block b of the committed draw through every check (test_jpeg_hidden_state.py runs the same on poisoned scratch memory)"""
    JS.run_block(engine, block(b))


def gpu_pinned(engine):
    for seed, k in PINNED:
        JS.run_case(engine, JS.draw(seed, k), JS.Pool(strict=False))


@pytest.mark.gpu
@pytest.mark.parametrize("b", range(N_BLOCKS))
def test_gpu_block_of_the_sweep(gpu, b):
    gpu_block(gpu, b)


@pytest.mark.gpu
def test_gpu_pinned_cases(gpu):
    """the cases the soak found failing, kept; each runs alone, under the soak's rule for the cap"""
    gpu_pinned(gpu)


@pytest.mark.gpu
@pytest.mark.skipif(not os.environ.get("MDCT_SOAK_JPEG_FILES"), reason="opt-in soak: MDCT_SOAK_JPEG_FILES=<cases> python -m pytest tests -m gpu -k soak_of_the_jpeg_files")
def test_gpu_soak_of_the_jpeg_files(gpu):
    """opt-in long run: MDCT_SOAK_JPEG_FILES fresh cases from MDCT_SOAK_JPEG_FILES_SEED (default 1) through the same code, block by
    block with the batches, in this one process; the first failing case or exception ends it.  MDCT_SOAK_JPEG_FILES_PROGRESS: a file
    that gets one line per block (a watched box).  A case that fails goes into PINNED."""
    import time
    n, seed = int(os.environ["MDCT_SOAK_JPEG_FILES"]), int(os.environ.get("MDCT_SOAK_JPEG_FILES_SEED", "1"))
    progress = os.environ.get("MDCT_SOAK_JPEG_FILES_PROGRESS")
    assert seed != SEED, "the soak is for fresh draws"
    t0, missed = time.time(), []
    for k0 in range(0, n, JS.BLOCK):
        missed += JS.run_block(gpu, [JS.draw(seed, k) for k in range(k0, min(k0 + JS.BLOCK, n))], strict=False).missed
        if progress:
            with open(progress, "a") as f:
                f.write(f"seed {seed}: cases 0 .. {min(k0 + JS.BLOCK, n) - 1} passed after {time.time() - t0:.0f} s; {len(missed)} planes under the cap\n")
    print(f"soak: {n} cases of seed {seed} passed in {time.time() - t0:.0f} s; planes under the tie-window cap (the reference's own numbers): {missed}")
    if progress:
        with open(progress, "a") as f:
            f.write(f"done: {n} cases; under the cap: {missed}\n")
