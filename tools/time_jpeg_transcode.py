"""Times the coefficient-domain path (libmdct_jpegcoef.so, simd_dct_amd/jpeg_transcode.py) on the 8192x8192
4:2:0 q75 picture tools/time_jpeg_encode.py uses:
  coder      coef_rows (three scans) and coef_scan_rows (interleaved) with the picture's optimal tables against the pixel coders
             opt_rows / opt_scan_rows of the same picture's planes and tables, and the statistics launches of both, taken alternately;
  transform  transform_planes of the luma plane, every operation, against mdct_stream_copy of the same bytes;
  whole      transcode_jpeg of the engine's file and of Pillow's (q75, no optimize, no restart markers) to bytes, wall clock, next to
             decode_jpeg + encode_jpeg(optimize=True) of the same file; file sizes in and out.
HIP-event medians of 11 repetitions per figure; each case runs in a child process of its own under `timeout`, one JSON line per case.

    python tools/time_jpeg_transcode.py [--out FILE]      all cases
    python tools/time_jpeg_transcode.py --case NAME        one case, in this process
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

CASES = ["coder", "transform", "whole"]
W = H = 8192
REPS = 11


def _picture():
    import numpy as np

    from simd_dct_amd import synth

    return np.stack([synth.plane_u8_np(W, H, "photo", seed=31 + k) for k in range(3)], axis=-1)


def _timer(torch):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        start.record()
        fn()
        end.record()
        end.synchronize()
        return start.elapsed_time(end) * 1000.0

    return timed


def _stat(v):
    return dict(median=round(sorted(v)[len(v) // 2], 1), min_max=[round(min(v), 1), round(max(v), 1)])


def coder_case():
    import torch

    from simd_dct_amd import api
    from simd_dct_amd import jpeg_decode as D
    from simd_dct_amd import jpeg_encode as J
    from simd_dct_amd import jpeg_transcode as TC

    api.init(0)
    img = torch.from_numpy(_picture()).cuda()
    sampling = J.sampling_of("4:2:0")
    luts = J.quality_tables(75)
    mx, my, msizes = J.mcu_grid(W, H, sampling)
    px = J.to_planes(img, "4:2:0", "HWC", planes=[torch.empty((ph, pw), dtype=torch.uint8, device="cuda") for pw, ph in msizes])
    _, coefs = D.decode_coefficients(J.encode_jpeg(img, quality=75, interleaved=True))
    del img
    timed = _timer(torch)
    res = dict(case="coder", width=W, height=H, subsampling="4:2:0")
    words = torch.zeros((2,), dtype=torch.int32, device="cuda")
    hist = torch.empty((2, 272), dtype=torch.int32, device="cuda")
    for inter in (False, True):
        specs = J.optimal_tables(J.symbol_histogram(px, sampling, luts, interleaved=inter))
        hc, _ = TC.coef_histogram(coefs, sampling, interleaved=inter)
        assert torch.equal(hc, J.symbol_histogram(px, sampling, luts, interleaved=inter)), "the two sources count different symbols"
        rows = [(my, mx * 6)] if inter else [(p.shape[0] // 8, p.shape[1] // 8) for p in px]
        bufs = [(torch.empty((n * J.opt_seg_stride(b),), dtype=torch.uint8, device="cuda"), torch.empty((2, n), dtype=torch.int32, device="cuda")) for n, b in rows]

        def pixels():
            if inter:
                J.opt_scan_rows(px, sampling, luts, specs, bufs[0][0], bufs[0][1][0], bufs[0][1][1], words[0:1])
            else:
                for k, (seg, c) in enumerate(bufs):
                    J.opt_rows(px[k], luts[min(k, 1)], (specs[2 * min(k, 1)], specs[2 * min(k, 1) + 1]), seg, c[0], c[1], words[0:1])

        def coefficients():
            if inter:
                TC.coef_scan_rows(coefs, sampling, specs, bufs[0][0], bufs[0][1][0], bufs[0][1][1], words[0:1], words[1:2])
            else:
                for k, (seg, c) in enumerate(bufs):
                    TC.coef_rows(coefs[k], (specs[2 * min(k, 1)], specs[2 * min(k, 1) + 1]), seg, c[0], c[1], words[0:1], words[1:2])

        fns = dict(pixel_coder=pixels, coef_coder=coefficients, pixel_stats=lambda: J.symbol_histogram(px, sampling, luts, interleaved=inter, hist=hist),
                   coef_stats=lambda: TC.coef_histogram(coefs, sampling, interleaved=inter, hist=hist, unrepresentable=words[1:2]))
        pixels()
        ref = [b[0].clone() for b in bufs], [b[1].clone() for b in bufs]
        coefficients()
        same = all(torch.equal(a[1], b) for a, b in zip(bufs, ref[1]))
        t = {k: [] for k in fns}
        for _ in range(REPS):  # alternating
            for k, fn in fns.items():
                t[k].append(timed(fn))
        form = "interleaved" if inter else "three_scans"
        res[form] = {k + "_us": _stat(v) for k, v in t.items()}
        res[form].update(same_segment_lengths=bool(same), coef_over_pixel_coder=round(_stat(t["coef_coder"])["median"] / _stat(t["pixel_coder"])["median"], 4))
    assert words.cpu().tolist() == [0, 0]
    res["kernels"] = sorted(k for k in api.kernel_counts() if k.startswith(("k_coef", "k_opt")))
    return res


def transform_case():
    import torch

    from simd_dct_amd import api
    from simd_dct_amd import jpeg_transcode as TC

    api.init(0)
    g = torch.Generator(device="cuda").manual_seed(1)
    src = torch.randint(-1023, 1024, (H, W), dtype=torch.int16, device="cuda", generator=g)
    dst = torch.empty_like(src)
    timed = _timer(torch)
    fns = {op: (lambda op=op: TC.transform_planes(src, dst, op)) for op in TC.TRANSFORMS}
    fns["stream_copy"] = lambda: api.stream_copy(src, dst, src.numel() * 2)
    for fn in fns.values():
        fn()
    t = {k: [] for k in fns}
    for _ in range(REPS):
        for k, fn in fns.items():
            t[k].append(timed(fn))
    res = dict(case="transform", width=W, height=H, bytes_moved=4 * W * H)
    for k, v in t.items():
        s = _stat(v)
        res[k] = dict(s, tb_s=round(4 * W * H / s["median"] / 1e6, 3))
    return res


def whole_case():
    import torch
    from PIL import Image

    from simd_dct_amd import api
    from simd_dct_amd import jpeg_decode as D
    from simd_dct_amd import jpeg_encode as J
    from simd_dct_amd import jpeg_transcode as TC

    api.init(0)
    host = _picture()
    b = io.BytesIO()
    Image.fromarray(host).save(b, "JPEG", quality=75, subsampling=2)
    files = dict(pillow=b.getvalue(), engine=J.encode_jpeg(torch.from_numpy(host).cuda(), quality=75, interleaved=True))
    res = dict(case="whole", width=W, height=H)

    def wall(fn):
        fn()
        t = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            t.append((time.perf_counter() - t0) * 1e6)
        return _stat(t), out

    for name, data in files.items():
        r = dict(file_bytes=len(data))
        for label, kw in (("transcode", dict()), ("transcode_interleaved", dict(interleaved=True)), ("transcode_rot90", dict(transform="rot90")),
                          ("transcode_annex_k", dict(optimize=False))):
            s, out = wall(lambda: TC.transcode_jpeg(data, **kw))
            r[label] = dict(wall_us=s, file_bytes=len(out), size_ratio=round(len(out) / len(data), 4))
        s, out = wall(lambda: J.encode_jpeg(D.decode_jpeg(data, mode="RGB"), quality=75, optimize=True))
        r["decode_then_encode"] = dict(wall_us=s, file_bytes=len(out))
        res[name] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=CASES)
    ap.add_argument("--out")
    ap.add_argument("--timeout", type=int, default=300)
    a = ap.parse_args()
    if a.case:
        print(json.dumps(dict(coder=coder_case, transform=transform_case, whole=whole_case)[a.case]()), flush=True)
        return 0
    lines, rc = [], 0
    for name in CASES:
        p = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--case", name], capture_output=True, text=True)
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
