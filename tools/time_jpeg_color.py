"""Times the colour stage (libmdct_jpegcolor.so, mdct_jpegcolor_to_rgb) on full frames, next to mdct_split420_u8_planes on the same
frames in the same process, and decode_jpeg(mode="RGB") against decode_jpeg() on a Pillow 7680x4320 4:2:0 file.

Each case runs in a child process of its own under `timeout`; the parent prints one JSON line per case.  Times are HIP-event medians of
5 repetitions of 20 back-to-back launches (decode: of 5 single calls), per launch.  Kernel times come from a separate
`rocprofv3 --kernel-trace --stats` run of the same command.

    python tools/time_jpeg_color.py [--out FILE]      all cases
    python tools/time_jpeg_color.py --case NAME        one case, in this process
"""
import argparse
import io
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name -> (W, H, kind, layout)
COLOUR_CASES = {
    "color-8192-420-hwc": (8192, 8192, "420", "HWC"),
    "color-8192-420-chw": (8192, 8192, "420", "CHW"),
    "color-7680x4320-420-hwc": (7680, 4320, "420", "HWC"),
    "color-7680x4320-444-hwc": (7680, 4320, "444", "HWC"),
    "color-7680x4320-grey-hwc": (7680, 4320, "grey", "HWC"),
}
CASES = list(COLOUR_CASES) + ["decode-7680x4320-420"]
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


def colour_case(name):
    import torch

    from simd_dct_amd import api
    from simd_dct_amd import jpeg_decode as D

    W, H, kind, layout = COLOUR_CASES[name]
    api.init(0)
    g = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda h, w: torch.randint(0, 256, (h, w), dtype=torch.uint8, device="cuda", generator=g)  # noqa: E731
    if kind == "grey":
        planes, sampling, colour, in_bytes = [rnd(H, W)], [(1, 1)], "grey", W * H
    elif kind == "444":
        planes, sampling, colour, in_bytes = [rnd(H, W) for _ in range(3)], [(1, 1)] * 3, "YCbCr", 3 * W * H
    else:
        planes, sampling, colour = [rnd(H, W), rnd(H // 2, W // 2), rnd(H // 2, W // 2)], [(2, 2), (1, 1), (1, 1)], "YCbCr"
        in_bytes = W * H + 2 * (W // 2) * (H // 2)
    out = torch.empty((H, W, 3) if layout == "HWC" else (3, H, W), dtype=torch.uint8, device="cuda")
    api.kernel_counts_reset()
    us, reps = _median_us(torch, lambda: D.to_rgb(planes, sampling, W, H, colour=colour, layout=layout, out=out), LAUNCHES)
    ran = sorted(k for k in api.kernel_counts() if k.startswith("k_ycc_rgb"))
    moved = in_bytes + 3 * W * H
    res = dict(case=name, width=W, height=H, kind=kind, layout=layout, kernels=ran, us=round(us, 2), reps_us=[round(x, 2) for x in reps],
               bytes=moved, tb_s=round(moved / us / 1e6, 3), share_of_8tb_s=round(moved / us / 1e6 / 8.0, 3))
    if kind == "420":
        # the encoder's front stage on the same frame: interleaved 8-bit YCbCr -> Y, Cb, Cr planes (the same 4.5 B per pixel)
        ycc = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
        y, cb, cr = rnd(H, W), rnd(H // 2, W // 2), rnd(H // 2, W // 2)
        sus, sreps = _median_us(torch, lambda: api.split420_u8_planes(ycc, W, H, y, cb, cr), LAUNCHES)
        res.update(split420_us=round(sus, 2), split420_reps_us=[round(x, 2) for x in sreps], ratio_to_split420=round(us / sus, 3))
    return res


def decode_case(name):
    import numpy as np
    import torch
    from PIL import Image

    from simd_dct_amd import api, synth
    from simd_dct_amd import jpeg_decode as D

    api.init(0)
    W, H = 7680, 4320
    img = np.stack([synth.plane_u8_np(W, H, "photo", seed=21 + k) for k in range(3)], axis=-1)
    buf = io.BytesIO()
    Image.fromarray(img, "YCbCr").save(buf, "JPEG", quality=90, subsampling=2)
    data = buf.getvalue()
    planes_us, planes_reps = _median_us(torch, lambda: D.decode_jpeg(data), 1)
    rgb_us, rgb_reps = _median_us(torch, lambda: D.decode_jpeg(data, mode="RGB"), 1)
    return dict(case=name, width=W, height=H, file_bytes=len(data), decode_planes_us=round(planes_us, 1), decode_rgb_us=round(rgb_us, 1),
                planes_reps_us=[round(x, 1) for x in planes_reps], rgb_reps_us=[round(x, 1) for x in rgb_reps],
                colour_share=round((rgb_us - planes_us) / rgb_us, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=CASES)
    ap.add_argument("--out")
    ap.add_argument("--timeout", type=int, default=300)
    a = ap.parse_args()
    if a.case:
        res = decode_case(a.case) if a.case.startswith("decode") else colour_case(a.case)
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
