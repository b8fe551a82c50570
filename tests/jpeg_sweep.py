"""The JPEG file entry points swept over seeded random geometry: the draw, a correct stand-in engine and the checks.  No GPU in here;
tests/test_jpeg_sweep.py runs these over the stand-in on the CPU and over simd_dct_amd on the MI355X.

  draw(seed, k)     one case, a plain dict, from np.random.default_rng((seed, k)) alone: a picture (size, content, quality, layout,
                    sampling, encoder form), the source of the file that is decoded and transcoded (the case's own encoded file, or a
                    file written from known planes by the test-side encoders), the decode form and the transcode.
  explicit_case     a case of the same form from stated values, the picture "noisy photo" with it (tests/jpeg_frame_limits.py).
  StandIn           an engine made of test-side pieces only: jpeg_encode_checker.planes, the float64 DCT, rne(. / Q), the test-side
                    entropy encoders; the serial checkers, the float64 IDCT, the colour and scaled checkers; the transform checker.
                    faults=...: one of FAULTS planted in it, which the checks must catch.
  check_encode / check_decode (check_rgb, check_scaled) / check_transcode / check_batches
                    pure functions of bytes and arrays, the truths the suite already trusts.
  run_case / run_block   an engine (StandIn, or the adapter of test_jpeg_sweep.py) through a case / a block of cases with its batches.
  coverage_failures      what the committed draw must contain, stated on the cases.

An engine has encode(image, quality, subsampling, layout, **form) -> bytes; decode(data, mode, layout, scale_denom) -> (planes or
image as numpy, coefficient planes as numpy); transcode(data, transform, trim, optimize, interleaved, progressive, script) -> bytes;
decode_batch(files, mode, layout) and encode_batch(images, quality, subsampling, layout).

Tie windows: wherever a window leaves a value undecided idct_reference's cap min_decided = 0.5 applies to a plane of 64 blocks or
more on its own, and to the smaller planes of a block of cases pooled per rule (Pool).  (Its other cap, max_skip = 0.1, belongs to
the round-trip rules, which nothing here uses.)"""
import functools
import io
import re

import numpy as np

import idct_reference as R
import jpeg_color_checker as CC
import jpeg_decode_checker as DC
import jpeg_encode_checker as EC
import jpeg_optimal_tables as T
import jpeg_progressive_approx_checker as XC
import jpeg_progressive_approx_encoder as AE
import jpeg_progressive_checker as PC
import jpeg_progressive_encoder as PE
import jpeg_scaled_checker as S
import jpeg_scan_encoder as E
import jpeg_transform_checker as X
from simd_dct_amd import jfif, synth

# ------------------------------------------------------------------------------------------ what is drawn from
SIDES = (1, 2, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 47, 48, 49, 63, 64, 65)
QUALITIES = (1, 10, 25, 50, 75, 90, 95, 100)
SAMPLINGS = {"grey": [(1, 1)], "4:4:4": [(1, 1), (1, 1), (1, 1)], "4:2:2": [(2, 1), (1, 1), (1, 1)], "4:2:0": [(2, 2), (1, 1), (1, 1)],
             "4:4:0": [(1, 2), (1, 1), (1, 1)], "2x2 2x1 1x2": [(2, 2), (2, 1), (1, 2)], "chroma above luma": [(1, 1), (2, 2), (2, 2)]}
ENCODER_SAMPLINGS = ("grey", "4:4:4", "4:2:2", "4:2:0")  # what encode_jpeg takes
FORMS = {"default": {}, "one launch": dict(two_launch=False), "interleaved": dict(interleaved=True), "optimize": dict(optimize=True),
         "interleaved optimize": dict(interleaved=True, optimize=True), "progressive": dict(progressive=True),
         "progressive standard": dict(progressive=True, script="standard"), "progressive drawn": dict(progressive=True, script="drawn")}
STRUCTURES = ("interleaved", "per component", "y then cbcr")
DRI_CLASSES = (0, 1, 2, 7, "mx", "mx+1", "mx*my", 65535)
SCALES = (2, 4, 8)
TRANSFORMS = (None,) + X.OPS
BLOCK = 12  # cases per block: one parametrized test, one decode batch, one encode batch
SCAN3 = [(0, 0, 0), (1, 1, 1), (2, 1, 1)]
FAULTS = ("a non-interleaved component's grid is taken from the padded plane", "its restart interval is counted on the MCU grid",
          "the trim skips the y axis", "a transposing operation leaves the DQT as it was", "CHW is read as HWC",
          "the scaled size uses floor in place of ceil")
# libjpeg's jpeg_simple_progression (jcparam.c) as (components, ss, se, ah, al); the chroma AC scans come Cr first
STANDARD = {1: [((0,), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1), ((0,), 0, 0, 1, 0), ((0,), 1, 63, 1, 0)],
            3: [((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1),
                ((0, 1, 2), 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0)]}
# T.81 Annex K.1 / K.2 in natural order
K1 = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
K2 = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32


def _ceil(a, b):
    return -(-a // b)


def quality_tables(quality):
    """libjpeg's jpeg_set_quality with force_baseline on the Annex K tables -> (luma, chroma) int64 [64], natural order"""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((np.array(base, dtype=np.int64) * scale + 50) // 100, 1, 255) for base in (K1, K2))


def interleavable(sampling):
    """the samplings the engine's interleaved coders take"""
    return len(sampling) == 3 and tuple(sampling[0]) in ((1, 1), (2, 1), (2, 2)) and all(tuple(s) == (1, 1) for s in sampling[1:])


# ------------------------------------------------------------------------------------------ geometry, from T.81 A.1.1 and A.2
def mcus(W, H, sampling):
    hmax, vmax = max(h for h, _ in sampling), max(v for _, v in sampling)
    return _ceil(W, 8 * hmax), _ceil(H, 8 * vmax)


def own_grids(W, H, sampling):
    """[(blocks_x, blocks_y)] of every component's own grid: ceil(true size / 8)"""
    return [(_ceil(cw, 8), _ceil(ch, 8)) for cw, ch in EC.true_sizes(W, H, sampling)]


def plane_sizes(W, H, sampling, on_mcu_grid):
    """[(padded width, padded height)]: the MCU grid, or every component's own grid"""
    if on_mcu_grid:
        mx, my = mcus(W, H, sampling)
        return [(mx * 8 * h, my * 8 * v) for h, v in sampling]
    return [(bx * 8, by * 8) for bx, by in own_grids(W, H, sampling)]


def scan_grid(W, H, sampling, comps):
    """(intervals' row length in MCUs, rows) of a scan over the components `comps`: A.2.2 for one, A.2.3 for several"""
    return own_grids(W, H, sampling)[comps[0]] if len(comps) == 1 else mcus(W, H, sampling)


def dri_of(cls, gx, gy):
    return {"mx": gx, "mx+1": gx + 1, "mx*my": gx * gy}.get(cls, cls)


def resolve_script(script, nc, interleaved):
    """the scans a progressive form writes: None the default bands behind the DC scan `interleaved` selects, 'standard' libjpeg's"""
    if script is None:
        dc = [(tuple(range(nc)), 0, 0, 0, 0)] if interleaved and nc == 3 else [((c,), 0, 0, 0, 0) for c in range(nc)]
        return dc + [((c,), ss, se, 0, 0) for c in range(nc) for ss, se in (PE.LUMA_BANDS if c == 0 else PE.CHROMA_BANDS)]
    if isinstance(script, str):
        assert script == "standard"
        return list(STANDARD[nc])
    return [(tuple(comps), ss, se, ah, al) for comps, ss, se, ah, al in script]


# ------------------------------------------------------------------------------------------ the draw
def _side(rng):
    return int(rng.choice(SIDES)) if rng.random() < 0.5 else int(rng.integers(1, 97))


def _pick(rng, options):
    return options[int(rng.integers(len(options)))]


def draw_script(rng, nc, may_interleave):
    """a script jpeg_progressive.check_script accepts: the DC first scan(s) with Al 0..3, interleaved or per component; per component
    one to four AC bands that tile 1..63, each with its own first Al 0..3, in any order; then every refinement scan down to Al 0, the
    chains of the bands and of the DC merged in a drawn order"""
    together = bool(rng.integers(2)) and may_interleave and nc == 3
    groups = [tuple(range(nc))] if together else [(c,) for c in range(nc)]
    al = int(rng.integers(4))
    script = [(g, 0, 0, 0, al) for g in groups]
    chains = [[(g, 0, 0, a, a - 1) for a in range(al, 0, -1)] for g in groups]
    first = []
    for c in range(nc):
        n = int(rng.integers(1, 5))
        edges = [1] + sorted(int(x) for x in rng.choice(np.arange(2, 64), size=n - 1, replace=False)) + [64]
        for a, b in zip(edges, edges[1:]):
            al = int(rng.integers(4))
            first.append(((c,), a, b - 1, 0, al))
            chains.append([((c,), a, b - 1, x, x - 1) for x in range(al, 0, -1)])
    script += [first[int(i)] for i in rng.permutation(len(first))]
    chains = [ch for ch in chains if ch]
    while chains:
        i = int(rng.integers(len(chains)))
        script.append(chains[i].pop(0))
        if not chains[i]:
            chains.pop(i)
    return script


def draw(seed, k):
    rng = np.random.default_rng((seed, k))
    c = dict(seed=int(seed), k=int(k))
    c["wide"] = bool(rng.integers(8) == 0)
    if c["wide"]:
        c["W"], c["H"] = int(rng.integers(2040, 2101)), int(rng.integers(1, 18))
    else:
        c["W"], c["H"] = _side(rng), _side(rng)
    c["picture"] = _pick(rng, ("photo", "noise", "flat"))
    c["picture_seed"] = int(rng.integers(1 << 16))  # a flat picture: its value is the low byte
    c["quality"] = _pick(rng, QUALITIES)
    c["layout"] = _pick(rng, ("HWC", "CHW"))
    c["enc_sampling"] = _pick(rng, ENCODER_SAMPLINGS)
    c["form"] = _pick(rng, tuple(FORMS))
    nc = len(SAMPLINGS[c["enc_sampling"]])
    c["dc_interleaved"] = bool(rng.integers(2))  # the form "progressive": which DC scan its default script gets
    c["script"] = draw_script(rng, nc, True) if c["form"] == "progressive drawn" else None
    c["source"] = _pick(rng, ("own", "written"))
    if c["source"] == "written":
        w = c["written"] = dict(sampling=_pick(rng, tuple(SAMPLINGS)), sof=_pick(rng, (0, 2)), levels=_pick(rng, ("sparse", "dense")),
                                tables=_pick(rng, ("annex k", "optimal")), structure=_pick(rng, STRUCTURES), dri=_pick(rng, DRI_CLASSES))
        w["script"] = draw_script(rng, len(SAMPLINGS[w["sampling"]]), True) if w["sof"] == 2 else None
        sampling = SAMPLINGS[w["sampling"]]
    else:
        sampling = SAMPLINGS[c["enc_sampling"]]
    c["scale"] = _pick(rng, SCALES)
    t = c["transcode"] = dict(transform=_pick(rng, TRANSFORMS), trim=bool(rng.random() < 0.75))
    osampling = [(v, h) for h, v in sampling] if t["transform"] in X.TRANSPOSING else sampling
    t["progressive"] = bool(rng.integers(3) == 0)
    t["optimize"] = bool(rng.integers(2)) or t["progressive"]
    t["interleaved"] = bool(rng.integers(2)) and interleavable(osampling)  # (where the transformed sampling allows it)
    kind = _pick(rng, (None, "standard", "drawn")) if t["progressive"] else None
    if kind == "standard" and len(sampling) == 3 and not interleavable(osampling):
        kind = "drawn"  # the standard script holds scans of all three components
    t["script"] = draw_script(rng, len(sampling), interleavable(osampling)) if kind == "drawn" else kind
    return c


def label(case):
    return case.get("name") or f"(seed, k) = ({case['seed']}, {case['k']})"


def explicit_case(name, W, H, sampling, form="default", *, picture="noisy photo", picture_seed=0, quality=90, layout="HWC", dc_interleaved=False, scale=2,
                  transform=None, trim=False, optimize=True, interleaved=False, progressive=False, script=None):
    """a case of draw()'s form from stated values (tests/jpeg_frame_limits.py): its own file is the source; script: None or 'standard' for the
    transcode; the encoder's comes with `form`"""
    assert sampling in ENCODER_SAMPLINGS and form in FORMS and form != "progressive drawn" and script in (None, "standard")
    return dict(seed=None, k=None, name=name, wide=W > 2000, W=int(W), H=int(H), picture=picture, picture_seed=int(picture_seed), quality=quality, layout=layout,
                enc_sampling=sampling, form=form, dc_interleaved=bool(dc_interleaved), script=None, source="own", scale=scale,
                transcode=dict(transform=transform, trim=bool(trim), progressive=bool(progressive), optimize=bool(optimize) or bool(progressive), interleaved=bool(interleaved),
                               script=script))


def source_frame(case):
    """(W, H, sampling name) of the file that is decoded and transcoded"""
    return case["W"], case["H"], case["written"]["sampling"] if case["source"] == "written" else case["enc_sampling"]


def encode_form(case):
    """the keywords of encode_jpeg for the case's form"""
    kw = dict(FORMS[case["form"]])
    if kw.get("script") == "drawn":
        kw["script"] = case["script"]
    if case["form"] == "progressive":
        kw["interleaved"] = case["dc_interleaved"]
    return kw


def encoded_scans(case):
    """[(components, ss, se, ah, al)] of the case's own file if it is progressive, else None"""
    kw = encode_form(case)
    if not kw.get("progressive"):
        return None
    return resolve_script(kw.get("script"), len(SAMPLINGS[case["enc_sampling"]]), kw.get("interleaved", False))


def source_scans(case):
    """the scans of the source file as [(components, ss, se, ah, al, DRI, interleaved)]; a baseline scan has ss = None"""
    W, H, name = source_frame(case)
    sampling = SAMPLINGS[name]
    nc = len(sampling)
    out = []
    if case["source"] == "written":
        w = case["written"]
        if w["sof"] == 2:
            script = w["script"]
        else:
            groups = [(0,)] if nc == 1 else {"interleaved": [(0, 1, 2)], "per component": [(0,), (1,), (2,)], "y then cbcr": [(0,), (1, 2)]}[w["structure"]]
            script = [(g, None, None, 0, 0) for g in groups]
        for comps, ss, se, ah, al in script:
            out.append((tuple(comps), ss, se, ah, al, dri_of(w["dri"], *scan_grid(W, H, sampling, comps)), len(comps) > 1))
        return out
    script = encoded_scans(case)
    if script is None:
        inter = FORMS[case["form"]].get("interleaved", False) and nc == 3
        script = [((0, 1, 2), None, None, 0, 0)] if inter else [((c,), None, None, 0, 0) for c in range(nc)]
    return [(tuple(comps), ss, se, ah, al, scan_grid(W, H, sampling, comps)[0], len(comps) > 1) for comps, ss, se, ah, al in script]


def source_kind(case):
    """how decode_jpeg_batch takes the source file: 'batch', or the fallback 'progressive' or 'unmarked'"""
    scans = source_scans(case)
    if scans[0][1] is not None:
        return "progressive"
    return "unmarked" if any(s[5] == 0 for s in scans) else "batch"


def row_blocks(case):
    """the most blocks a row of one of the source file's scans holds"""
    W, H, name = source_frame(case)
    sampling = SAMPLINGS[name]
    return max(scan_grid(W, H, sampling, comps)[0] * (1 if len(comps) == 1 else sum(sampling[ci][0] * sampling[ci][1] for ci in comps)) for comps, *_ in source_scans(case))


def refusal(W, H, sampling, transform, trim):
    """None, or (axis, 'remainder' | 'no whole iMCU'): what transcode_jpeg refuses, the x axis first"""
    hmax, vmax = max(h for h, _ in sampling), max(v for _, v in sampling)
    for axis, size, unit in (("x", W, 8 * hmax), ("y", H, 8 * vmax)):
        if transform is not None and axis in X.MIRRORED[transform] and size % unit:
            if not trim:
                return axis, "remainder"
            if size < unit:
                return axis, "no whole iMCU"
    return None


# ------------------------------------------------------------------------------------------ pictures and written files
def picture(case):
    """uint8 [H, W, 3], or [H, W] for grey"""
    W, H, n = case["W"], case["H"], len(SAMPLINGS[case["enc_sampling"]])
    if case["picture"] == "flat":
        chans = [np.full((H, W), (case["picture_seed"] + 85 * k) & 255, dtype=np.uint8) for k in range(n)]
    elif case["picture"] == "noisy photo":  # (no draw takes it: explicit_case's) synth's photo planes, noise of +-16 added
        chans = [np.clip(synth.plane_u8_np(W, H, "photo", seed=case["picture_seed"] + k).astype(np.int16)
                         + (synth.plane_u8_np(W, H, "noise", seed=case["picture_seed"] + 10 + k) >> 3) - 16, 0, 255).astype(np.uint8) for k in range(n)]
    else:
        chans = [synth.plane_u8_np(W, H, case["picture"], seed=case["picture_seed"] + k) for k in range(n)]
    return chans[0] if n == 1 else np.stack(chans, axis=-1)


def laid_out(pic, layout):
    return pic if pic.ndim == 2 or layout == "HWC" else np.ascontiguousarray(np.moveaxis(pic, -1, 0))


def as_scanned(planes, W, H, sampling, whole, dc_whole):
    """what a file's scans hold of planes on the MCU grid: every block (whole: one interleaved scan), or each component's own grid
    only, with the DC of the other blocks kept where the DC scan is interleaved (dc_whole)"""
    out = []
    for p, (bx, by) in zip(planes, own_grids(W, H, sampling)):
        q = np.array(p, dtype=np.int16)
        if not whole:
            dc = q[::8, ::8].copy()
            q[by * 8:], q[:, bx * 8:] = 0, 0
            if dc_whole:
                q[::8, ::8] = dc
        out.append(q)
    return out


def _spec_map(by_which):
    """{2 * id + class: spec} (api.huffman_spec's keys) -> {(class, id): spec}"""
    return {(w & 1, w >> 1): (list(b), list(v)) for w, (b, v) in by_which.items()}


def sof2_file(frame, planes, script, qtables, dri_class="mx", shared_dc=False):
    """a progressive file of the serial encoder's scans (the writer of test_jpeg_decode_approx_synthetic.deep_file, for any script and
    restart interval): every AC scan with the table made for it; the DC first scans each with its own tables, or (shared_dc, what
    jpeg_progressive.encode writes) with one table per class over all of them"""
    W, H, sampling = frame["width"], frame["height"], frame["comps"]
    coded = []
    for comps, ss, se, ah, al in script:
        units, upm, gx = AE.scan_units(frame, list(comps), planes)
        dri = dri_of(dri_class, gx, len(units) // (gx * upm))
        per = dri * upm if dri else len(units)
        coded.append((comps, ss, se, ah, al, units, per, dri))
    dc_counts = sum(AE.dc_first(u, per, al)["counts"] for comps, ss, se, ah, al, u, per, _ in coded if ss == 0 and ah == 0)
    scans = []
    for comps, ss, se, ah, al, units, per, dri in coded:
        tables, specs = {}, None
        if ss == 0 and ah == 0:
            counts = dc_counts if shared_dc else AE.dc_first(units, per, al)["counts"]
            specs = {cls: T.optimal_table(counts[cls][:16]) for cls in {min(ci, 1) for ci in comps}}
            tables = {(0, cls): sp for cls, sp in specs.items()}
        elif ss:
            specs = T.optimal_table(AE.encode_scan(units, per, ss, se, ah, al)["counts"])
            tables = {(1, min(comps[0], 1)): specs}
        r = AE.encode_scan(units, per, ss, se, ah, al, specs)
        assert r.get("uncoded", 0) == 0
        scans.append(dict(components=[(ci, min(ci, 1), min(ci, 1)) for ci in comps], ss=ss, se=se, ah=ah, al=al, restart_interval=dri or 1, tables=tables,
                          scan=AE.scan_data(r["segs"])))
    data = jfif.write_progressive_jpeg(qtables, W, H, sampling, scans)
    if dri_class == 0:  # no DRI at all: every scan is one interval
        bare = re.sub(rb"\xff\xdd\x00\x04\x00\x01", b"", data)
        assert len(bare) == len(data) - 6 * len(scans)
        data = bare
    return data


def baseline_file(frame, planes, scans, qtables, optimize, table_per_component=False):
    """jpeg_scan_encoder.encode_file with the Annex K tables or the ones made for the planes"""
    if optimize:
        specs = _spec_map(T.specs_of(T.histogram(frame, scans, planes), grey=len(frame["comps"]) == 1))
    else:
        specs = {k: v for k, v in E.ANNEX_K.items() if k[1] == 0 or len(frame["comps"]) == 3}
    return E.encode_file(frame, scans, planes, specs, qtables=qtables, table_per_component=table_per_component)[0]


@functools.lru_cache(maxsize=2 * BLOCK)
def _written(seed, k):
    case = draw(seed, k)
    w = case["written"]
    W, H, sampling = case["W"], case["H"], SAMPLINGS[w["sampling"]]
    frame = dict(width=W, height=H, comps=sampling)
    rng = np.random.default_rng((seed, k, 1))
    planes = []
    for shape in E.plane_shapes(frame):
        if w["levels"] == "dense":
            p = rng.integers(-120, 121, shape)
        else:
            p = rng.integers(-40, 41, shape) * (rng.random(shape) < 0.15)
        p[::8, ::8] = rng.integers(-500, 501, (shape[0] // 8, shape[1] // 8))  # no transform can make an unrepresentable DC difference
        planes.append(p.astype(np.int16))
    # neither table is symmetric: a transposed one differs
    qtables = [rng.integers(1, 13, 64), rng.integers(1, 25, 64)]
    per_comp = [qtables[min(ci, 1)] for ci in range(len(sampling))]
    scans = source_scans(case)
    if w["sof"] == 2:
        planes = as_scanned(planes, W, H, sampling, False, len(w["script"][0][0]) == 3)
        data = sof2_file(frame, planes, w["script"], per_comp, dri_class=w["dri"])
    else:
        if len(sampling) == 3 and w["structure"] != "interleaved":
            own = as_scanned(planes, W, H, sampling, False, False)
            planes = own if w["structure"] == "per component" else [own[0], planes[1], planes[2]]
        described = [dict(comps=[(ci, min(ci, 1), min(ci, 1)) for ci in comps], dri=dri) for comps, _, _, _, _, dri, _ in scans]
        data = baseline_file(frame, planes, described, qtables, w["tables"] == "optimal")
    for p in planes:
        p.setflags(write=False)
    return data, planes


def written_file(case):
    """(the file, the known planes it was written from: what a decoder must read out of it)"""
    return _written(case["seed"], case["k"])


# ------------------------------------------------------------------------------------------ the serial checkers, on any file
def serial_baseline(data, faults=()):
    """jpeg_decode_checker.decode, which divides by the restart interval, restated for files that may have none (a scan without
    markers is one interval); the stand-in's planted geometry faults live here -> (planes, statuses)"""
    data = bytes(data)
    frame, _, scans = DC.parse(data)
    fc = frame["components"]
    hmax, vmax = max(c[1] for c in fc), max(c[2] for c in fc)
    mx, my = _ceil(frame["width"], 8 * hmax), _ceil(frame["height"], 8 * vmax)
    planes = [np.zeros((my * c[2] * 8, mx * c[1] * 8), dtype=np.int16) for c in fc]
    statuses = []
    for comps, dri, start, end, huff in scans:
        if len(comps) == 1:
            ci = comps[0][0]
            gx, gy = _ceil(_ceil(frame["width"] * fc[ci][1], hmax), 8), _ceil(_ceil(frame["height"] * fc[ci][2], vmax), 8)
            if FAULTS[0] in faults:
                gx, gy = mx * fc[ci][1], my * fc[ci][2]
            layout = [(ci, 0, 0, 1, 1)]
        else:
            gx, gy = mx, my
            layout = [(ci, hh, vv, fc[ci][1], fc[ci][2]) for ci, _, _ in comps for vv in range(fc[ci][2]) for hh in range(fc[ci][1])]
        tabs = {("dc", ci): huff[(0, td)] for ci, td, _ in comps}
        tabs.update({("ac", ci): huff[(1, ta)] for ci, _, ta in comps})
        total = gx * gy
        per = dri or total
        n = _ceil(mx * my if FAULTS[1] in faults and len(comps) == 1 else total, per)
        st = []
        for k, (chunk, mk) in enumerate(DC.split_intervals(data[start:end], n)):
            units = []
            for m in range(k * per, min((k + 1) * per, total)):
                ux, uy = m % gx, m // gx
                for ci, hh, vv, Hc, Vc in layout:
                    units.append((ci, ("dc", ci), ("ac", ci), (ci, uy * Vc + vv, ux * Hc + hh)))
            marker_after = None if k == n - 1 else ((mk is not None and mk == k % 8),)
            status, blocks = DC.decode_interval(chunk, units, tabs, marker_after)
            if status == DC.OK:
                for (ci, by, bx), blk in blocks:
                    if by * 8 < planes[ci].shape[0] and bx * 8 < planes[ci].shape[1]:
                        planes[ci][by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = blk.reshape(8, 8).astype(np.int16)
            st.append(status)
        statuses.append(st)
    return planes, statuses


@functools.lru_cache(maxsize=16)
def checker_decode(data):
    """the serial checker for the file's SOF -> (planes, read-only; statuses; dict(frame, qtables per component, scans, qt))"""
    frame, qt, scans, _ = PC.parse(data)
    if frame["sof"] == 0xC2:
        planes, statuses = XC.decode(data)
    elif all(sc["dri"] for sc in scans):
        planes, statuses, _ = DC.decode(data)
    else:
        planes, statuses = serial_baseline(data)
    for p in planes:
        p.setflags(write=False)
    return planes, statuses, dict(frame=frame, qtables=[np.array(qt[c[3]], dtype=np.float32) for c in frame["components"]], scans=scans)


def spec_of_codes(table):
    """jpeg_decode_checker.code_table's {(length, code): value} -> (bits16, vals)"""
    keys = sorted(table)
    bits = [0] * 16
    for length, _ in keys:
        bits[length - 1] += 1
    return bits, [table[k] for k in keys]


# ------------------------------------------------------------------------------------------ the tie-window caps
MIN_DECIDED = 0.5  # idct_reference's cap


class CapMiss(AssertionError):
    """fewer than MIN_DECIDED of a plane's values lie outside the tie windows: a statement about the reference's numbers alone (the
    exact values and the windows), whatever the engine gave; the check of those values has no teeth"""


class Pool:
    """the decided and all values of the planes of fewer than 64 blocks of a block of cases, per rule; the cap applies to the sums.
    strict=False (the soak, whose draws nobody has looked at): a plane under the cap is noted in `missed`, not raised -- every value the
    windows do decide has been compared by then"""

    def __init__(self, strict=True):
        self.sums, self.strict, self.missed = {}, strict, []

    def add(self, rule, dec):
        s = self.sums.setdefault(rule, [0, 0])
        s[0] += int(dec.sum())
        s[1] += int(dec.size)

    def cap(self, what, dec):
        if dec.size and dec.mean() < MIN_DECIDED:
            if self.strict:
                raise CapMiss((what, "decided", float(dec.mean())))
            self.missed.append((what, float(dec.mean())))

    def check(self):
        for rule, (n, of) in self.sums.items():
            self.cap(f"pooled small planes, rule {rule}", np.arange(of) < n)


def capped(dec, what, rule, n_blocks, pool):
    """the cap for a plane of 64 blocks or more, the pool's for a smaller one"""
    if n_blocks < 64 and pool is not None:
        pool.add(rule, dec)
    else:
        (pool or Pool()).cap(what, dec)


def exact_rule(got, want, exact, tol, rng_, what, rule, n_blocks, pool):
    """idct_reference.assert_exact_rule, then its cap"""
    R.assert_exact_rule(got, want, exact, tol, rng_, what, min_decided=0.0)
    capped(R.decided(exact, tol, *rng_), what, rule, n_blocks, pool)


# ------------------------------------------------------------------------------------------ the checks
def _frame_of(info):
    f = info["frame"]
    return dict(width=f["width"], height=f["height"], comps=[(h, v) for _, h, v, _ in f["components"]])


def check_scans(data, info, C, expected, what):
    """the file's scans are `expected` [(components, ss, se, ah, al, DRI)] (ss None: a baseline scan), and the entropy layer is exact:
    the test-side encoders code C with the file's own tables, script and restart intervals into every scan byte for byte"""
    frame = _frame_of(info)
    sof2 = info["frame"]["sof"] == 0xC2
    got = [(tuple(ci for ci, _, _ in sc["comps"]), sc["ss"] if sof2 else None, sc["se"] if sof2 else None, sc["ah"], sc["al"], sc["dri"]) for sc in info["scans"]]
    assert got == [tuple(e) for e in expected], (what, "scans", got, expected)
    for si, sc in enumerate(info["scans"]):
        body = data[sc["start"]:sc["end"]]
        if not sof2:
            specs = {key: spec_of_codes(t) for key, t in sc["huffman"].items()}
            want = E.encode_scan(frame, dict(comps=sc["comps"], dri=sc["dri"]), C, specs)[0]
        else:
            units, upm, _ = AE.scan_units(frame, [ci for ci, _, _ in sc["comps"]], C)
            per = sc["dri"] * upm if sc["dri"] else len(units)
            if sc["ss"] == 0:
                specs = None if sc["ah"] else {min(ci, 1): spec_of_codes(sc["huffman"][(0, td)]) for ci, td, _ in sc["comps"]}
            else:
                specs = spec_of_codes(sc["huffman"][(1, sc["comps"][0][2])])
            r = AE.encode_scan(units, per, sc["ss"], sc["se"], sc["ah"], sc["al"], specs)
            assert r.get("uncoded", 0) == 0, (what, "scan", si)
            want = AE.scan_data(r["segs"])
        assert body == want, (what, f"scan {si}: the entropy-coded bytes differ from the test-side encoder's", len(body), len(want))


def check_tables(info, C, optimize, what):
    """the DHT of a file the engine wrote: Annex K, or the tables jpeg_optimal_tables makes from C's histogram -- for a progressive
    file one DC table per class over the DC first scans and one AC table per AC scan"""
    frame = _frame_of(info)
    nc = len(frame["comps"])
    if info["frame"]["sof"] != 0xC2:
        have = {2 * th + tc: spec_of_codes(t) for (tc, th), t in info["scans"][-1]["huffman"].items()}
        if optimize:
            scans = [dict(comps=sc["comps"], dri=sc["dri"]) for sc in info["scans"]]
            want = T.specs_of(T.histogram(frame, scans, C), grey=nc == 1)
        else:
            want = {2 * th + tc: v for (tc, th), v in E.ANNEX_K.items() if th == 0 or nc == 3}
        assert have == {k: (list(b), list(v)) for k, (b, v) in want.items()}, (what, "DHT")
        return
    coded = []
    for sc in info["scans"]:
        units, upm, _ = AE.scan_units(frame, [ci for ci, _, _ in sc["comps"]], C)
        coded.append((sc, units, sc["dri"] * upm if sc["dri"] else len(units)))
    dc = sum(AE.dc_first(u, per, sc["al"])["counts"] for sc, u, per in coded if sc["ss"] == 0 and sc["ah"] == 0)
    for si, (sc, units, per) in enumerate(coded):
        if sc["ss"] == 0 and sc["ah"] == 0:
            for ci, td, _ in sc["comps"]:
                b, v = T.optimal_table(dc[min(ci, 1)][:16])
                assert spec_of_codes(sc["huffman"][(0, td)]) == (list(b), list(v)), (what, "DC table of scan", si)
        elif sc["ss"]:
            b, v = T.optimal_table(AE.encode_scan(units, per, sc["ss"], sc["se"], sc["ah"], sc["al"])["counts"])
            assert spec_of_codes(sc["huffman"][(1, sc["comps"][0][2])]) == (list(b), list(v)), (what, "AC table of scan", si)


PILLOW_MAX = 65500  # libjpeg's JPEG_MAX_DIMENSION: Pillow neither writes nor reads a larger side (T.81 allows 65535); a caller with such a
# picture says pillow=False to check_encode / check_transcode


def check_pillow(data, W, H, grey, what):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    assert im.size == (W, H) and im.mode == ("L" if grey else "RGB"), (what, im.size, im.mode)
    im.load()  # libjpeg reads every scan


def expected_scans(W, H, sampling, progressive, script, interleaved):
    """[(components, ss, se, ah, al, DRI)] of a file the engine writes: a restart interval per row of every scan's own grid"""
    nc = len(sampling)
    if progressive:
        scans = resolve_script(script, nc, interleaved)
    elif interleaved and nc == 3:
        scans = [((0, 1, 2), None, None, 0, 0)]
    else:
        scans = [((c,), None, None, 0, 0) for c in range(nc)]
    return [(tuple(comps), ss, se, ah, al, scan_grid(W, H, sampling, comps)[0]) for comps, ss, se, ah, al in scans]


def check_encode(case, data, pic, pool=None, pillow=True):
    """-> C, the coefficient planes the serial checker reads out of the case's own file.  pillow=False: a side lies above PILLOW_MAX"""
    from test_fdct_accuracy import check_file_against_rule
    what = label(case) + " encode"
    data = bytes(data)
    W, H, grey = case["W"], case["H"], case["enc_sampling"] == "grey"
    sampling = SAMPLINGS[case["enc_sampling"]]
    kw = encode_form(case)
    progressive, inter = bool(kw.get("progressive")), bool(kw.get("interleaved")) and not grey
    C, statuses, info = checker_decode(data)
    assert info["frame"]["sof"] == (0xC2 if progressive else 0xC0), (what, hex(info["frame"]["sof"]))
    assert (info["frame"]["width"], info["frame"]["height"]) == (W, H), what
    assert all(s == 0 for st in statuses for s in st) and len(statuses) == len(info["scans"]), (what, statuses)
    for k, q in enumerate(info["qtables"]):
        assert np.array_equal(q, quality_tables(case["quality"])[min(k, 1)]), (what, "DQT of component", k)
    # the forward rule on the encoding checker's planes, padding included, the file's own DQT as the table
    # (a progressive file's AC scans, and its DC scans unless interleaved, cover each component's own grid: the rest of the MCU grid
    # is not in the file; the own grid's pixels are the same under either padding)
    expected = expected_scans(W, H, sampling, progressive, kw.get("script"), inter)
    on_mcu = inter and not progressive
    sizes = plane_sizes(W, H, sampling, on_mcu)
    blocks = [pw * ph // 64 for pw, ph in sizes]
    sub = "4:2:0" if grey else case["enc_sampling"]
    check_file_against_rule(data, pic, sub, grey, on_mcu, what, decoded=(C, statuses, info), min_decided=0.0)  # (the cap: below)
    for k, (p, q, n) in enumerate(zip(EC.planes(pic, sub, padded=sizes), info["qtables"], blocks)):
        _, exact, tol = R.fwd_coefficients(R.blocks(p), q, 128.0)
        capped(R.decided(exact, tol, *R.I16_RANGE), f"{what} component {k}", "forward", n, pool)
    if progressive and len(expected[0][0]) == 3:  # an interleaved DC scan: the DC of every block of the MCU grid
        full = plane_sizes(W, H, sampling, True)
        for k, (p, c, q) in enumerate(zip(EC.planes(pic, sub, padded=full), C, info["qtables"])):
            want, exact, tol = R.fwd_coefficients(R.blocks(p), q, 128.0)
            bad = R.mismatches(R.blocks(c), want, exact, tol, *R.I16_RANGE)[:, 0, 0]
            assert not bad.any(), (what, f"component {k}: the DC of {int(bad.sum())} blocks of the MCU grid differs from the exact rule")
    check_scans(data, info, C, expected, what)
    if progressive or kw.get("optimize"):
        check_tables(info, C, True, what)
    if pillow:
        check_pillow(data, W, H, grey, what)
    return C


@functools.lru_cache(maxsize=16)
def _decoded_frame(data):
    frame, qt, _, _ = PC.parse(data)
    return frame["width"], frame["height"], [(h, v) for _, h, v, _ in frame["components"]], [np.array(qt[c[3]], dtype=np.float64) for c in frame["components"]], frame["sof"]


def decoded_frame(data):
    """(W, H, sampling, quantisation table per component, sof) of a file, by the test-side parser"""
    return _decoded_frame(bytes(data))


def check_decode(case, data, C, got, pool=None):
    """got: dict(planes, coefs, rgb, rgb_coefs, scaled, scaled_coefs) as numpy, of the three decodes of `data`; C: its true planes"""
    what = label(case) + " decode"
    W, H, sampling, qtables, _ = decoded_frame(data)
    for key in ("coefs", "rgb_coefs", "scaled_coefs"):
        assert len(got[key]) == len(C), (what, key)
        for ci, (g, c) in enumerate(zip(got[key], C)):
            assert g.shape == c.shape and g.dtype == np.int16, (what, key, ci, g.shape, c.shape)
            if not np.array_equal(g, c):
                at = np.argwhere(g != c)[0]
                raise AssertionError(f"{what}: {key} of component {ci} differ from the file's coefficients at {int((g != c).sum())} places, first at "
                                     f"row {at[0]} column {at[1]} (block {at[0] // 8}, {at[1] // 8}): got {g[tuple(at)]}, want {c[tuple(at)]}")
    sizes = EC.true_sizes(W, H, sampling)
    assert len(got["planes"]) == len(C), what
    for ci, (p, c, q, (cw, ch)) in enumerate(zip(got["planes"], C, qtables, sizes)):
        assert p.shape == (ch, cw) and p.dtype == np.uint8, (what, "plane", ci, p.shape, (ch, cw))
        want, exact, tol = S.component(c, q, 8, cw, ch)
        exact_rule(p, want, exact, tol, R.U8_RANGE, f"{what} plane {ci}", "inverse", c.size // 64, pool)
    check_rgb(what, got["planes"], sampling, W, H, got["rgb"], case["layout"])
    check_scaled(what, data, C, got["scaled"], case["scale"], pool)


def check_rgb(what, planes, sampling, W, H, got, layout):
    """mode="RGB" is jpeg_color_checker.to_rgb of the engine's own planes, in the layout asked for"""
    rgb = CC.to_rgb(planes, sampling, W, H, "grey" if len(planes) == 1 else "YCbCr")
    want = rgb if layout == "HWC" else np.moveaxis(rgb, -1, 0)
    assert got.shape == want.shape and np.array_equal(got, want), (what, "RGB", layout, got.shape, want.shape)


def check_scaled(what, data, C, scaled, d, pool=None):
    """the planes at 1/d against the scaled rule on the file's true coefficients C"""
    W, H, sampling, qtables, _ = decoded_frame(data)
    geo, _ = S.geometry(W, H, sampling, d)
    assert len(scaled) == len(C), what
    for ci, (p, c, q, g) in enumerate(zip(scaled, C, qtables, geo)):
        assert p.shape == (g[2], g[1]) and p.dtype == np.uint8, (what, f"plane {ci} at 1/{d}", p.shape, (g[2], g[1]))
        want, exact, tol = S.component(c, q, g[0], g[1], g[2])
        exact_rule(p, want, exact, tol, R.U8_RANGE, f"{what} plane {ci} at 1/{d}", f"scaled {g[0]}", c.size // 64, pool)


def transcode_args(case):
    return dict(case["transcode"])


def check_transcode(case, data, C, outcome, pillow=True):
    """outcome: the file transcode_jpeg returned, or the exception it raised; data, C: the source file and its true planes"""
    what = label(case) + " transcode"
    t = case["transcode"]
    op = t["transform"]
    W, H, sampling, qtables, _ = decoded_frame(data)
    refused = refusal(W, H, sampling, op, t["trim"])
    if refused is not None:
        axis, why = refused
        assert isinstance(outcome, ValueError), (what, "no ValueError for", refused, type(outcome))
        text = {"remainder": "remainder", "no whole iMCU": "holds no whole iMCU"}[why]
        assert f"the {axis} axis" in str(outcome) and text in str(outcome), (what, str(outcome), refused)
        return
    if isinstance(outcome, Exception):
        raise AssertionError(f"{what}: raised {type(outcome).__name__}: {outcome}")
    out = bytes(outcome)
    tw, th = X.trimmed(W, H, sampling, op)
    mx, my = mcus(tw, th, sampling)
    want = [np.ascontiguousarray(p[:my * v * 8, :mx * h * 8]) for p, (h, v) in zip(C, sampling)]
    want = [X.transform(p, op) if op else p for p in want]
    transposing = op in X.TRANSPOSING
    ow, oh = (th, tw) if transposing else (tw, th)
    osampling = [(v, h) for h, v in sampling] if transposing else list(sampling)
    got, statuses, info = checker_decode(out)
    assert all(s == 0 for st in statuses for s in st) and len(statuses) == len(info["scans"]), (what, statuses)
    f = info["frame"]
    assert (f["width"], f["height"]) == (ow, oh), (what, "size", (f["width"], f["height"]), (ow, oh))
    assert [(h, v) for _, h, v, _ in f["components"]] == osampling, (what, "sampling", f["components"], osampling)
    assert f["sof"] == (0xC2 if t["progressive"] else 0xC0), (what, hex(f["sof"]))
    for ci, (q, src) in enumerate(zip(info["qtables"], qtables)):
        src = src.reshape(8, 8)
        assert np.array_equal(q.reshape(8, 8), src.T if transposing else src), (what, "DQT of component", ci)
    assert out[2:4] == b"\xff\xe0" and out[6:11] == b"JFIF\x00", (what, "the colour space marker")
    if pillow:
        check_pillow(out, ow, oh, len(osampling) == 1, what)
    inter = t["interleaved"] and len(osampling) == 3
    expected = expected_scans(ow, oh, osampling, t["progressive"], t["script"], inter)
    whole = not t["progressive"] and inter
    dc_whole = t["progressive"] and len(expected[0][0]) == 3
    held = as_scanned(want, ow, oh, osampling, whole, dc_whole)
    for ci, (g, w) in enumerate(zip(got, held)):
        assert g.shape == w.shape, (what, "planes of component", ci, g.shape, w.shape)
        if not np.array_equal(g, w):
            at = np.argwhere(g != w)[0]
            raise AssertionError(f"{what}: component {ci} of the output differs from the transformed source at {int((g != w).sum())} places, first at row "
                                 f"{at[0]} column {at[1]}: got {g[tuple(at)]}, want {w[tuple(at)]}")
    check_scans(out, info, got, expected, what)
    check_tables(info, got, t["optimize"], what)


def check_batches(engine, cases, sources, pool=None):
    """the block's two batches: decode_jpeg_batch over its source files against decode on each alone, encode_jpeg_batch over its colour
    pictures against encode(..., interleaved=True) on each"""
    what = f"block of {label(cases[0])}"
    rng = np.random.default_rng((cases[0]["seed"], cases[0]["k"], 2))
    mode, layout = _pick(rng, (None, "RGB")), _pick(rng, ("HWC", "CHW"))
    sub, quality, enc_layout = _pick(rng, ENCODER_SAMPLINGS[1:]), _pick(rng, QUALITIES), _pick(rng, ("HWC", "CHW"))
    batch = engine.decode_batch(sources, mode, layout)
    assert len(batch) == len(sources), what
    for case, data, (out, coefs) in zip(cases, sources, batch):
        one, one_coefs = engine.decode(data, mode, layout, 1)
        outs, ones = ([out], [one]) if mode == "RGB" else (list(out), list(one))
        assert len(outs) == len(ones) and all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(outs, ones)), (what, "decode batch", label(case), mode, layout)
        assert len(coefs) == len(one_coefs) and all(np.array_equal(g, w) for g, w in zip(coefs, one_coefs)), (what, "decode batch coefficients", label(case))
    colour = [c for c in cases if c["enc_sampling"] != "grey"]
    images = [laid_out(picture(c), enc_layout) for c in colour]
    files = engine.encode_batch(images, quality, sub, enc_layout)
    assert len(files) == len(images), what
    for case, image, data in zip(colour, images, files):
        assert bytes(data) == bytes(engine.encode(image, quality, sub, enc_layout, interleaved=True)), (what, "encode batch", label(case), quality, sub, enc_layout)


# ------------------------------------------------------------------------------------------ the stand-in engine
class StandIn:
    """a correct engine of test-side pieces; faults: members of FAULTS planted in it"""

    def __init__(self, faults=()):
        assert all(f in FAULTS for f in faults)
        self.faults = tuple(faults)

    # -- writing: coefficient planes -> a file of the form asked for
    def _write(self, W, H, sampling, C, qtables, optimize, interleaved, progressive, script, per_component):
        frame = dict(width=W, height=H, comps=list(sampling))
        nc = len(sampling)
        inter = bool(interleaved) and nc == 3
        if progressive:
            resolved = resolve_script(script, nc, inter)
            full = [np.pad(c, ((0, ph - c.shape[0]), (0, pw - c.shape[1]))) for c, (pw, ph) in zip(C, plane_sizes(W, H, sampling, True))]
            return sof2_file(frame, full, resolved, [qtables[min(ci, 1)] for ci in range(nc)] if not per_component else qtables, shared_dc=True)
        if inter:
            scans = [dict(comps=SCAN3, dri=mcus(W, H, sampling)[0])]
        else:
            scans = [dict(comps=[SCAN3[ci]], dri=bx) for ci, (bx, _) in enumerate(own_grids(W, H, sampling))]
        return baseline_file(frame, C, scans, qtables, optimize, table_per_component=per_component)

    def encode(self, image, quality, subsampling, layout, two_launch=True, interleaved=False, optimize=False, progressive=False, script=None):
        pic = np.asarray(image)
        grey = pic.ndim == 2
        if not grey and layout == "CHW":
            pic = pic.reshape(pic.shape[1], pic.shape[2], 3) if FAULTS[4] in self.faults else np.moveaxis(pic, 0, -1)
        H, W = pic.shape[:2]
        sampling = [(1, 1)] if grey else EC.SAMPLING[subsampling]
        luma, chroma = quality_tables(quality)
        on_mcu = progressive or (interleaved and not grey)
        planes = EC.planes(pic, subsampling, padded=plane_sizes(W, H, sampling, on_mcu))
        C = []
        for k, p in enumerate(planes):
            q = (luma if k == 0 else chroma).reshape(8, 8).astype(np.float64)
            c = R.sat_i16(R.rne(R.dct2(R.blocks(p).astype(np.float64) - 128.0) / q))
            C.append(R.plane(c, p.shape[1], p.shape[0]).astype(np.int16))
        return self._write(W, H, sampling, C, [luma, chroma], optimize, interleaved, progressive, script, False)

    # -- reading
    def _coefficients(self, data):
        data = bytes(data)
        if decoded_frame(data)[4] == 0xC2:
            return XC.decode(data)[0]
        if self.faults:
            return serial_baseline(data, self.faults)[0]
        return [np.array(p) for p in checker_decode(data)[0]]

    def decode(self, data, mode=None, layout="HWC", scale_denom=1):
        W, H, sampling, qtables, _ = decoded_frame(data)
        C = self._coefficients(data)
        if scale_denom == 1:
            geo = [(8, cw, ch, h, v) for (cw, ch), (h, v) in zip(EC.true_sizes(W, H, sampling), sampling)]
            size = (W, H)
        else:
            geo, size = S.geometry(W, H, sampling, scale_denom)
            if FAULTS[5] in self.faults:
                hmax, vmax = max(h for h, _ in sampling), max(v for _, v in sampling)
                geo = [(g[0], W * h * g[0] // (hmax * 8), H * v * g[0] // (vmax * 8), g[3], g[4]) for g, (h, v) in zip(geo, sampling)]
        planes = [S.component(c, q, g[0], g[1], g[2])[0].astype(np.uint8) for c, q, g in zip(C, qtables, geo)]
        if mode != "RGB":
            return planes, C
        assert scale_denom == 1
        rgb = CC.to_rgb(planes, sampling, size[0], size[1], "grey" if len(C) == 1 else "YCbCr")
        return (rgb if layout == "HWC" else np.ascontiguousarray(np.moveaxis(rgb, -1, 0))), C

    def transcode(self, data, transform=None, trim=False, optimize=True, interleaved=False, progressive=False, script=None):
        W, H, sampling, qtables, _ = decoded_frame(data)
        refused = refusal(W, H, sampling, transform, trim)
        if refused is not None:
            axis, why = refused
            raise ValueError(f"{transform}: the {axis} axis " + ("leaves a remainder beyond whole iMCUs" if why == "remainder" else "holds no whole iMCU"))
        C = self._coefficients(data)
        tw, th = X.trimmed(W, H, sampling, transform)
        if FAULTS[2] in self.faults:
            th = H
        mx, my = mcus(tw, th, sampling)
        C = [np.ascontiguousarray(p[:my * v * 8, :mx * h * 8]) for p, (h, v) in zip(C, sampling)]
        if transform is not None:
            C = [X.transform(p, transform) for p in C]
        if transform in X.TRANSPOSING:
            tw, th, sampling = th, tw, [(v, h) for h, v in sampling]
            if FAULTS[3] not in self.faults:
                qtables = [q.reshape(8, 8).T.reshape(64) for q in qtables]
        if interleaved and not interleavable(sampling):
            raise ValueError(f"interleaved=True takes 4:4:4, 4:2:2 or 4:2:0, not {sampling}")
        qtables = [np.rint(q).astype(np.int64) for q in qtables]
        return self._write(tw, th, sampling, C, qtables, optimize, interleaved, progressive, script, True)

    # -- batches
    def decode_batch(self, files, mode, layout):
        return [self.decode(f, mode, layout, 1) for f in files]

    def encode_batch(self, images, quality, subsampling, layout):
        return [self.encode(im, quality, subsampling, layout, interleaved=True) for im in images]


# ------------------------------------------------------------------------------------------ an engine through a case, a block
def stage_encode(engine, case, pool=None):
    """-> (the case's own file, its coefficients by the checker)"""
    pic = picture(case)
    sub = "4:2:0" if case["enc_sampling"] == "grey" else case["enc_sampling"]
    data = bytes(engine.encode(laid_out(pic, case["layout"]), case["quality"], sub, case["layout"], **encode_form(case)))
    return data, check_encode(case, data, pic, pool)


def source_of(case, own, C_own):
    """(the file that is decoded and transcoded, its true planes)"""
    return (own, C_own) if case["source"] == "own" else written_file(case)


def stage_decode(engine, case, data, C, pool=None):
    got = {}
    got["planes"], got["coefs"] = engine.decode(data, None, "HWC", 1)
    got["rgb"], got["rgb_coefs"] = engine.decode(data, "RGB", case["layout"], 1)
    got["scaled"], got["scaled_coefs"] = engine.decode(data, None, "HWC", case["scale"])
    check_decode(case, data, C, got, pool)


def stage_transcode(engine, case, data, C, pillow=True):
    try:
        outcome = engine.transcode(data, **transcode_args(case))
    except ValueError as e:  # (what a refusal raises; anything else is the engine's failure and goes up)
        outcome = e
    check_transcode(case, data, C, outcome, pillow)


class CaseFailure(AssertionError):
    pass


def run_case(engine, case, pool=None):
    """every stage of one case; a failure names (seed, k) and shows the case -> the source file"""
    try:
        own, C_own = stage_encode(engine, case, pool)
        data, C = source_of(case, own, C_own)
        stage_decode(engine, case, data, C, pool)
        stage_transcode(engine, case, data, C)
    except CaseFailure:
        raise
    except Exception as e:
        raise CaseFailure(f"{label(case)} failed: {type(e).__name__}: {e}\ncase: {case}") from e
    return data


def run_block(engine, cases, strict=True):
    """a block of cases, ended by the first failing one; then the block's batches and the pooled caps (strict: Pool)"""
    pool = Pool(strict)
    sources = [run_case(engine, c, pool) for c in cases]
    try:
        check_batches(engine, cases, sources, pool)
    except Exception as e:
        raise CaseFailure(f"the batches of the block of {label(cases[0])} .. {label(cases[-1])} failed: {type(e).__name__}: {e}") from e
    pool.check()
    return pool


# ------------------------------------------------------------------------------------------ what the committed draw must contain
def coverage_failures(cases):
    """the conditions the committed draw does not meet (none: []).  A transform can trim, or be refused for, only an axis it mirrors
    (transpose mirrors none: it needs only its untrimmed case)."""
    bad = []

    def need(ok, text):
        if not ok:
            bad.append(text)

    pairs = {}
    for c in cases:
        pairs[(c["enc_sampling"], c["form"])] = pairs.get((c["enc_sampling"], c["form"]), 0) + 1
    for s in ENCODER_SAMPLINGS:
        for f in FORMS:
            need(pairs.get((s, f), 0) >= 2, f"sampling {s} with form {f}: {pairs.get((s, f), 0)} cases")
    seen, refusals = set(), 0
    for c in cases:
        W, H, name = source_frame(c)
        sampling = SAMPLINGS[name]
        t = c["transcode"]
        op = t["transform"]
        if refusal(W, H, sampling, op, t["trim"]) is not None:
            refusals += 1
            seen.add((op, "refused"))
            continue
        tw, th = X.trimmed(W, H, sampling, op)
        seen |= {(op, "x")} if tw != W else set()
        seen |= {(op, "y")} if th != H else set()
        seen |= {(op, "neither")} if (tw, th) == (W, H) else set()
    for op in X.OPS:
        for axis in X.MIRRORED[op]:
            need((op, axis) in seen, f"{op} with a trimmed {axis} axis")
        need((op, "neither") in seen, f"{op} with neither axis trimmed")
        need(not X.MIRRORED[op] or (op, "refused") in seen, f"{op} refused")
    need(refusals * 4 <= len(cases), f"{refusals} refusals among {len(cases)} cases")
    for side in "WH":
        for mod in (8, 16):
            for r in (0, 1, 7):
                need(any(c[side] % mod == r for c in cases), f"{side} = {r} mod {mod}")
    need(any((c["W"], c["H"]) == (1, 1) for c in cases), "a 1 x 1 picture")
    need(any(c["W"] == 1 and c["H"] > 1 for c in cases), "a one-pixel-wide picture")
    need(any(c["H"] == 1 and c["W"] > 1 for c in cases), "a one-pixel-tall picture")
    scaled = {(source_frame(c)[2], c["scale"]) for c in cases}
    for s in SAMPLINGS:
        for d in SCALES:
            need((s, d) in scaled, f"scale 1/{d} with sampling {s}")
    dri = {(c["written"]["dri"], inter) for c in cases if c["source"] == "written" for *_, inter in source_scans(c)}
    for cls in DRI_CLASSES:
        for inter in (True, False):
            need((cls, inter) in dri, f"DRI class {cls} on {'an interleaved' if inter else 'a non-interleaved'} scan")
    scripts = [s for c in cases for s in (c["script"], c.get("written", {}).get("script"), c["transcode"]["script"]) if isinstance(s, list)]
    # (every script ends at Al 0: a first scan with Al 3 is refined three times)
    need(any(ah == 0 and al >= 3 for s in scripts for _, _, _, ah, al in s), "a script that refines a position three times")
    need(any(ss == 0 and ah and len(comps) == 3 for s in scripts for comps, ss, se, ah, al in s), "an interleaved DC refinement scan")
    need(any(ss == 0 and ah and tuple(comps) in ((1,), (2,)) for s in scripts for comps, ss, se, ah, al in s), "a DC refinement scan per component of a colour file")
    wide = sum(1 for c in cases if c["wide"] and row_blocks(c) > 256)
    need(wide >= 8, f"{wide} wide cases whose rows hold more than 256 blocks")
    for kind in ("unmarked", "progressive"):
        ok = False
        for b in range(0, len(cases), BLOCK):
            kinds = [source_kind(c) for c in cases[b:b + BLOCK]]
            ok |= any(k == kind and "batch" in kinds[:i] and "batch" in kinds[i + 1:] for i, k in enumerate(kinds))
        need(ok, f"a fallback file ({kind}) inside a batch with batch-path files on both sides")
    for b in range(0, len(cases), BLOCK):
        need(any(source_kind(c) == "batch" for c in cases[b:b + BLOCK]), f"a batch-path file in block {b // BLOCK}")
        need(any(c["enc_sampling"] != "grey" for c in cases[b:b + BLOCK]), f"a colour picture in block {b // BLOCK}")
    return bad
