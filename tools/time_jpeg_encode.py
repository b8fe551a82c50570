"""Times the encoder's front stage (libmdct_jpegenc.so, mdct_jpegenc_from_rgb) on full frames, next to mdct_split420_u8_planes on the
same frame in the same process (it moves the same 4.5 B per pixel at 4:2:0), and encode_jpeg of an 8192x8192 RGB image at q75 4:2:0
in both scan forms (the fused coder + counted packing, the default, or one launch per component), with the wall clock to the returned bytes split
into device work, the length readback and the copy of the scans, next to Pillow's encode of the same image on one host core; and the
one-interleaved-scan form (encode_jpeg(interleaved=True), libmdct_jpegenc_scan.so) against the three-scan form on the same images,
taken alternately in one process: device time of the whole path, the scan coder alone against the three launches it replaces, wall time;
and encode_jpeg(optimize=True) (libmdct_jpegenc_opt.so) against optimize=False in both scan forms: device time, the statistics launch
alone, the wait for the histogram, wall time and file sizes.

Each case runs in a child process of its own under `timeout`; the parent prints one JSON line per case.  Front-stage times are
HIP-event medians of 5 repetitions of 20 back-to-back launches, per launch; encode times are medians of 5 calls.  Kernel times come
from a separate `rocprofv3 --kernel-trace --stats` run of the same command.

    python tools/time_jpeg_encode.py [--out FILE]      all cases
    python tools/time_jpeg_encode.py --case NAME        one case, in this process
"""
import argparse
import io
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name -> (W, H, subsampling, layout)
FRONT_CASES = {
    "front-8192-420-hwc": (8192, 8192, "4:2:0", "HWC"),
    "front-8192-420-chw": (8192, 8192, "4:2:0", "CHW"),
    "front-7680x4320-420-hwc": (7680, 4320, "4:2:0", "HWC"),
    "front-7680x4320-444-hwc": (7680, 4320, "4:4:4", "HWC"),
}
# one interleaved scan (libmdct_jpegenc_scan.so) against the three-scan path on the same image, alternating: name -> (W, H, subsampling)
INTERLEAVED_CASES = {
    "interleaved-8192-420-q75": (8192, 8192, "4:2:0"),
    "interleaved-8192-444-q75": (8192, 8192, "4:4:4"),
    "interleaved-7680x4320-420-q75": (7680, 4320, "4:2:0"),
    "interleaved-7680x4320-444-q75": (7680, 4320, "4:4:4"),
}
# encode_jpeg(optimize=True) (libmdct_jpegenc_opt.so) against optimize=False on the same image, alternating: name -> (W, H, subsampling, interleaved)
OPTIMIZED_CASES = {
    "optimized-8192-420-q75-three": (8192, 8192, "4:2:0", False),
    "optimized-8192-420-q75-interleaved": (8192, 8192, "4:2:0", True),
    "optimized-7680x4320-444-q75-three": (7680, 4320, "4:4:4", False),
    "optimized-7680x4320-444-q75-interleaved": (7680, 4320, "4:4:4", True),
}
CASES = list(FRONT_CASES) + ["encode-8192-420-q75"] + list(INTERLEAVED_CASES) + list(OPTIMIZED_CASES)
REPS, LAUNCHES = 5, 20


def _median_us(torch, fn, launches):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(REPS):
        start.record()
        for _ in range(launches):
            fn()
        end.record()
        end.synchronize()
        t.append(start.elapsed_time(end) * 1000.0 / launches)
    return sorted(t)[len(t) // 2], t


def front_case(name):
    import torch

    from simd_dct_amd import api
    from simd_dct_amd import jpeg_encode as J

    W, H, sub, layout = FRONT_CASES[name]
    api.init(0)
    g = torch.Generator(device="cuda").manual_seed(1)
    img = torch.randint(0, 256, (H, W, 3) if layout == "HWC" else (3, H, W), dtype=torch.uint8, device="cuda", generator=g)
    sizes = J.component_sizes(W, H, J.sampling_of(sub))
    planes = [torch.empty((ph, pw), dtype=torch.uint8, device="cuda") for _, _, pw, ph in sizes]
    api.kernel_counts_reset()
    us, reps = _median_us(torch, lambda: J.to_planes(img, sub, layout, planes=planes), LAUNCHES)
    ran = sorted(k for k in api.kernel_counts() if k.startswith("k_rgb_ycc"))
    moved = 3 * W * H + sum(pw * ph for _, _, pw, ph in sizes)
    res = dict(case=name, width=W, height=H, subsampling=sub, layout=layout, kernels=ran, us=round(us, 2), reps_us=[round(x, 2) for x in reps],
               bytes=moved, tb_s=round(moved / us / 1e6, 3))
    if sub == "4:2:0":
        ycc = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
        y, cb, cr = planes
        sus, sreps = _median_us(torch, lambda: api.split420_u8_planes(ycc, W, H, y, cb, cr), LAUNCHES)
        res.update(split420_us=round(sus, 2), split420_reps_us=[round(x, 2) for x in sreps], ratio_to_split420=round(us / sus, 3))
    return res


def encode_case(name):
    import numpy as np
    import torch
    from PIL import Image

    from simd_dct_amd import api, synth
    from simd_dct_amd import jpeg_encode as J

    api.init(0)
    W, H = 8192, 8192
    host = np.stack([synth.plane_u8_np(W, H, "photo", seed=31 + k) for k in range(3)], axis=-1)
    img = torch.from_numpy(host).cuda()
    res = dict(case=name, width=W, height=H)
    for form, two in (("one_launch", False), ("two_launch", True)):
        data = J.encode_jpeg(img, quality=75, two_launch=two)  # warm: allocations, tables
        wall = []
        for _ in range(REPS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            data = J.encode_jpeg(img, quality=75, two_launch=two)
            wall.append((time.perf_counter() - t0) * 1e6)
        # the device part alone: the same launches into buffers kept across calls, timed by events
        sizes = J.component_sizes(W, H, J.sampling_of("4:2:0"))
        planes = J.to_planes(img, "4:2:0", "HWC")
        scans = [J._Scan(torch, img.device, pw, ph, pw * ph + 4096) for _, _, pw, ph in sizes]
        luma, chroma = J.quality_tables(75)

        def device():
            J.to_planes(img, "4:2:0", "HWC", planes=planes)
            for k, (p, (_, _, pw, ph), sc) in enumerate(zip(planes, sizes, scans)):
                J._run_scan(p, pw, ph, luma if k == 0 else chroma, k > 0, sc, two, None)

        dev_us, dev_reps = _median_us(torch, device, 1)
        device()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ends = torch.stack([sc.off[-1] for sc in scans]).cpu().tolist()
        t1 = time.perf_counter()
        parts = [sc.out[:n].cpu().numpy() for sc, n in zip(scans, ends)]
        t2 = time.perf_counter()
        res[form] = dict(wall_us=round(sorted(wall)[len(wall) // 2], 1), wall_reps_us=[round(x, 1) for x in wall], device_us=round(dev_us, 1),
                         device_reps_us=[round(x, 1) for x in dev_reps], length_readback_us=round((t1 - t0) * 1e6, 1),
                         scan_copy_us=round((t2 - t1) * 1e6, 1), scan_bytes=int(sum(ends)), file_bytes=len(data))
        del scans, planes, parts
    t = []
    for _ in range(3):
        b = io.BytesIO()
        t0 = time.process_time()
        Image.fromarray(host).save(b, "JPEG", quality=75, subsampling=2)
        t.append((time.process_time() - t0) * 1e6)
    res.update(pillow_cpu_us=round(sorted(t)[1], 1), pillow_file_bytes=len(b.getvalue()))
    return res


def interleaved_case(name):
    """device time (events, per repetition: front launch + scans + packing) of the interleaved path and of the three-scan path
    (interleaved=False, two_launch=True), taken alternately on the same planes' image; the scan coder alone against the three
    mdct_fwd_u8_huffman_rows launches it replaces; wall time of encode_jpeg both ways.  HWC, quality 75, synth "photo" content."""
    import numpy as np
    import torch

    from simd_dct_amd import api, synth
    from simd_dct_amd import jpeg_encode as J

    api.init(0)
    W, H, sub = INTERLEAVED_CASES[name]
    host = np.stack([synth.plane_u8_np(W, H, "photo", seed=31 + k) for k in range(3)], axis=-1)
    img = torch.from_numpy(host).cuda()
    sampling = J.sampling_of(sub)
    luma, chroma = J.quality_tables(75)
    # the three-scan path's buffers
    sizes = J.component_sizes(W, H, sampling)
    planes3 = J.to_planes(img, sub, "HWC")
    scans = [J._Scan(torch, img.device, pw, ph, pw * ph + 4096) for _, _, pw, ph in sizes]
    # the interleaved path's
    mx, my, msizes = J.mcu_grid(W, H, sampling)
    planes1 = [torch.empty((ph, pw), dtype=torch.uint8, device="cuda") for pw, ph in msizes]
    stride = J.scan_seg_stride(mx, sampling)
    seg = torch.empty((my * stride,), dtype=torch.uint8, device="cuda")
    counts = torch.empty((2, my), dtype=torch.int32, device="cuda")
    off = torch.empty((my + 1,), dtype=torch.int64, device="cuda")
    out = torch.empty((sum(pw * ph for pw, ph in msizes) + 4096,), dtype=torch.uint8, device="cuda")

    def three_rows():
        for k, (p, (_, _, pw, ph), sc) in enumerate(zip(planes3, sizes, scans)):
            api.fwd_u8_huffman_rows(p, pw, ph, sc.seg, sc.counts[0], lut=luma if k == 0 else chroma, chroma=k > 0, seg_stride=sc.stride, pitch=p.stride(0),
                                    ff_counts=sc.counts[1])

    def three():
        J.to_planes(img, sub, "HWC", planes=planes3)
        for k, (p, (_, _, pw, ph), sc) in enumerate(zip(planes3, sizes, scans)):
            J._run_scan(p, pw, ph, luma if k == 0 else chroma, k > 0, sc, True, None)

    def one_rows():
        J.scan_rows(planes1, sampling, (luma, chroma), seg, counts[0], counts[1], seg_stride=stride)

    def one():
        J.to_planes(img, sub, "HWC", planes=planes1)
        one_rows()
        api.jpeg_pack_rows(seg, counts[0], stride, my, out, off, ff_counts=counts[1])

    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        start.record()
        fn()
        end.record()
        end.synchronize()
        return start.elapsed_time(end) * 1000.0

    for fn in (three, one, three, one):  # warm: code objects, tables
        fn()
    torch.cuda.synchronize()
    t = dict(three=[], one=[], three_rows=[], one_rows=[])
    for _ in range(2 * REPS + 1):  # alternating
        t["three"].append(timed(three))
        t["one"].append(timed(one))
        t["three_rows"].append(timed(three_rows))
        t["one_rows"].append(timed(one_rows))
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    assert int(off[-1].item()) <= out.numel()
    wall = dict(three=[], one=[])
    for form, flag in (("three", False), ("one", True), ("three", False), ("one", True)):
        J.encode_jpeg(img, quality=75, subsampling=sub, interleaved=flag)
    files = {}
    for _ in range(REPS):
        for form, flag in (("three", False), ("one", True)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            files[form] = J.encode_jpeg(img, quality=75, subsampling=sub, interleaved=flag)
            wall[form].append((time.perf_counter() - t0) * 1e6)
    res = dict(case=name, width=W, height=H, subsampling=sub, mcus=[mx, my], kernels=sorted(k for k in api.kernel_counts() if k.startswith("k_scan_rows")))
    for k, label in (("three", "three_scan"), ("one", "interleaved")):
        res[label] = dict(device_us=round(med[k], 1), device_min_max_us=[round(min(t[k]), 1), round(max(t[k]), 1)], device_reps_us=[round(x, 1) for x in t[k]],
                          rows_us=round(med[k + "_rows"], 1), rows_min_max_us=[round(min(t[k + "_rows"]), 1), round(max(t[k + "_rows"]), 1)],
                          wall_us=round(sorted(wall[k])[len(wall[k]) // 2], 1), wall_reps_us=[round(x, 1) for x in wall[k]], file_bytes=len(files[k]))
    res["interleaved_over_three_scan_device"] = round(med["one"] / med["three"], 4)
    res["inside_three_scan_spread"] = bool(med["one"] <= max(t["three"]))
    return res


def optimized_case(name):
    """device time (events, buffers kept: front launch + coder(s) + packing, with optimize also the statistics launch and the coders
    of libmdct_jpegenc_opt.so with the image's tables) with and without optimize, taken alternately on the same image, 11 repetitions;
    the statistics launch(es) alone and the Annex K coder launch(es) alone on the same planes; the wait for the histogram (the copy of
    its 2176 bytes after the statistics launch, wall clock); wall time of encode_jpeg to bytes and the file sizes both ways."""
    import numpy as np
    import torch

    from simd_dct_amd import api, synth
    from simd_dct_amd import jpeg_encode as J

    api.init(0)
    W, H, sub, inter = OPTIMIZED_CASES[name]
    host = np.stack([synth.plane_u8_np(W, H, "photo", seed=31 + k) for k in range(3)], axis=-1)
    img = torch.from_numpy(host).cuda()
    sampling = J.sampling_of(sub)
    luts = J.quality_tables(75)
    bpm = sum(h * v for h, v in sampling)
    if inter:
        mx, my, msizes = J.mcu_grid(W, H, sampling)
        sizes = [(pw, ph) for pw, ph in msizes]
        rows = [(my, mx * bpm)]
    else:
        sizes = [(pw, ph) for _, _, pw, ph in J.component_sizes(W, H, sampling)]
        rows = [(ph // 8, pw // 8) for pw, ph in sizes]
    planes = [torch.empty((ph, pw), dtype=torch.uint8, device="cuda") for pw, ph in sizes]
    J.to_planes(img, sub, "HWC", planes=planes)
    hist = torch.empty((2, 272), dtype=torch.int32, device="cuda")
    specs = J.optimal_tables(J.symbol_histogram(planes, sampling, luts, interleaved=inter, hist=hist))
    uncoded = torch.zeros((1,), dtype=torch.int32, device="cuda")
    # per scan: segments at the Annex K stride and at the stride of the coders that take tables, counts, the packed scan, offsets
    bufs = []
    for n, blocks in rows:
        st0, st1 = 208 * blocks + 8, J.opt_seg_stride(blocks)
        bufs.append(dict(n=n, st0=st0, st1=st1, seg=torch.empty((n * st1,), dtype=torch.uint8, device="cuda"), counts=torch.empty((2, n), dtype=torch.int32, device="cuda"),
                         out=torch.empty((n * blocks * 64 + 4096,), dtype=torch.uint8, device="cuda"), off=torch.empty((n + 1,), dtype=torch.int64, device="cuda")))

    def stats():
        J.symbol_histogram(planes, sampling, luts, interleaved=inter, hist=hist)

    def coders(opt):
        for k, b in enumerate(bufs):
            if inter:
                if opt:
                    J.opt_scan_rows(planes, sampling, luts, specs, b["seg"], b["counts"][0], b["counts"][1], uncoded, seg_stride=b["st1"])
                else:
                    J.scan_rows(planes, sampling, luts, b["seg"], b["counts"][0], b["counts"][1], seg_stride=b["st0"])
            elif opt:
                J.opt_rows(planes[k], luts[min(k, 1)], (specs[2 * min(k, 1)], specs[2 * min(k, 1) + 1]), b["seg"], b["counts"][0], b["counts"][1], uncoded, seg_stride=b["st1"])
            else:
                pw, ph = sizes[k]
                api.fwd_u8_huffman_rows(planes[k], pw, ph, b["seg"], b["counts"][0], lut=luts[min(k, 1)], chroma=k > 0, seg_stride=b["st0"], pitch=planes[k].stride(0),
                                        ff_counts=b["counts"][1])

    def whole(opt):
        J.to_planes(img, sub, "HWC", planes=planes)
        if opt:
            stats()
        coders(opt)
        for b in bufs:
            api.jpeg_pack_rows(b["seg"], b["counts"][0], b["st1"] if opt else b["st0"], b["n"], b["out"], b["off"], ff_counts=b["counts"][1])

    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        start.record()
        fn()
        end.record()
        end.synchronize()
        return start.elapsed_time(end) * 1000.0

    for _ in range(2):  # warm: code objects, tables
        whole(False)
        whole(True)
    torch.cuda.synchronize()
    t = dict(plain=[], optimize=[], stats=[], plain_coders=[], optimize_coders=[], hist_wait=[])
    for _ in range(2 * REPS + 1):  # alternating
        t["plain"].append(timed(lambda: whole(False)))
        t["optimize"].append(timed(lambda: whole(True)))
        t["stats"].append(timed(stats))
        t["plain_coders"].append(timed(lambda: coders(False)))
        t["optimize_coders"].append(timed(lambda: coders(True)))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stats()
        hist.cpu()
        t["hist_wait"].append((time.perf_counter() - t0) * 1e6)
    assert int(uncoded.item()) == 0 and all(int(b["off"][-1].item()) <= b["out"].numel() for b in bufs)
    wall, files = dict(plain=[], optimize=[]), {}
    for flag in (False, True, False, True):
        J.encode_jpeg(img, quality=75, subsampling=sub, interleaved=inter, optimize=flag)
    for _ in range(2 * REPS + 1):
        for form, flag in (("plain", False), ("optimize", True)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            files[form] = J.encode_jpeg(img, quality=75, subsampling=sub, interleaved=inter, optimize=flag)
            wall[form].append((time.perf_counter() - t0) * 1e6)
    t.update(plain_wall=wall["plain"], optimize_wall=wall["optimize"])
    res = dict(case=name, width=W, height=H, subsampling=sub, interleaved=inter, kernels=sorted(k for k in api.kernel_counts() if k.startswith("k_opt")))
    for k, v in t.items():
        res[k + "_us"] = dict(median=round(sorted(v)[len(v) // 2], 1), min_max=[round(min(v), 1), round(max(v), 1)], reps=[round(x, 1) for x in v])
    res.update(plain_file_bytes=len(files["plain"]), optimize_file_bytes=len(files["optimize"]), size_ratio=round(len(files["optimize"]) / len(files["plain"]), 4),
               stats_no_longer_than_the_coders=bool(res["stats_us"]["median"] <= res["plain_coders_us"]["median"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=CASES)
    ap.add_argument("--out")
    ap.add_argument("--timeout", type=int, default=300)
    a = ap.parse_args()
    if a.case:
        res = (encode_case(a.case) if a.case.startswith("encode") else interleaved_case(a.case) if a.case in INTERLEAVED_CASES
               else optimized_case(a.case) if a.case in OPTIMIZED_CASES else front_case(a.case))
        print(json.dumps(res), flush=True)
        return 0
    lines, rc = [], 0
    for name in CASES:
        p = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--case", name],
                           capture_output=True, text=True)
        if p.returncode != 0:
            print(json.dumps(dict(case=name, returncode=p.returncode, stderr=p.stderr[-2000:])), flush=True)
            rc = p.returncode
            break  # a failed or faulted child ends the run: nothing more is started on the device
        line = p.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
