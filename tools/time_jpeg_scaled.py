"""Times the reduced-size inverse (libmdct_jpegscale.so, mdct_jpegscale_inv_i16_u8) next to the full inverse (mdct_inv_i16_u8_batch) on
the same coefficient planes in the same process, and decode_jpeg(mode="RGB") at scale_denom 1, 2, 4, 8 on a Pillow 7680x4320 4:2:0 file.

Each case runs in a child process of its own under `timeout`; the parent prints one JSON line per case.  Times are HIP-event medians of
5 repetitions of 20 back-to-back launches (decode: of 5 single calls), per launch.  Kernel times come from a separate
`rocprofv3 --kernel-trace --stats` run of the same command.

    python tools/time_jpeg_scaled.py [--out FILE]      all cases
    python tools/time_jpeg_scaled.py --case NAME        one case, in this process
"""
import argparse
import io
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GREY = [(8192, 8192, "luma")]
FRAME = [(7680, 4320, "luma"), (3840, 2160, "chroma"), (3840, 2160, "chroma")]
# name -> [(plane width, plane height, table, n)]: the planes of the call (a component that keeps 8x8 blocks is not part of it)
INVERSE_CASES = {
    "grey-8192-n4": [p + (4,) for p in GREY],
    "grey-8192-n2": [p + (2,) for p in GREY],
    "grey-8192-n1": [p + (1,) for p in GREY],
    "frame-420-d2": [FRAME[0] + (4,)],  # chroma stays at 8x8: the existing call
    "frame-420-d4": [FRAME[0] + (2,), FRAME[1] + (4,), FRAME[2] + (4,)],
    "frame-420-d8": [FRAME[0] + (1,), FRAME[1] + (2,), FRAME[2] + (2,)],
}
CASES = list(INVERSE_CASES) + ["decode-7680x4320-420"]
REPS, LAUNCHES = 5, 20
READ_ROWS = {4: 7, 2: 5, 1: 1}  # coefficient rows of 8 a block's lane loads


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


def inverse_case(name):
    import torch

    from simd_dct_amd import api, synth
    from simd_dct_amd import jpeg_decode as D

    api.init(0)
    tables = dict(luma=synth.JPEG_LUMA, chroma=synth.JPEG_CHROMA)
    g = torch.Generator(device="cuda").manual_seed(1)
    scaled, full, moved, moved_full = [], [], 0, 0
    for W, H, table, n in INVERSE_CASES[name]:
        coef = torch.randint(-40, 40, (H, W), dtype=torch.int16, device="cuda", generator=g)
        px = torch.empty((H // 8 * n, W // 8 * n), dtype=torch.uint8, device="cuda")
        px8 = torch.empty((H, W), dtype=torch.uint8, device="cuda")
        scaled.append((px, coef, W // 8, H // 8, tables[table], n))
        full.append((px8, coef, W, H, tables[table]))
        moved += 2 * W * H * READ_ROWS[n] // 8 + px.numel()
        moved_full += 3 * W * H
    api.kernel_counts_reset()
    us, reps = _median_us(torch, lambda: D.scaled_inverse(scaled), LAUNCHES)
    ran = sorted(k for k in api.kernel_counts() if k.startswith("k_idct_scaled"))
    fus, freps = _median_us(torch, lambda: api.u8_i16_batch("inv", full), LAUNCHES)
    # the copy rate of the same process: as many bytes read and written as the scaled call moves, halved each way
    nbytes = max(1 << 20, moved // 2 // 4096 * 4096)
    a, b = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    cus, _ = _median_us(torch, lambda: api.stream_copy(a, b, nbytes), LAUNCHES)
    copy_tb_s = 2 * nbytes / cus / 1e6
    return dict(case=name, planes=[[W, H, n] for W, H, _, n in INVERSE_CASES[name]], kernels=ran, us=round(us, 2), reps_us=[round(x, 2) for x in reps],
                full_inverse_us=round(fus, 2), full_reps_us=[round(x, 2) for x in freps], ratio_to_full=round(us / fus, 3),
                bytes=moved, full_bytes=moved_full, tb_s=round(moved / us / 1e6, 3), copy_us=round(cus, 2), copy_tb_s=round(copy_tb_s, 3),
                share_of_copy_rate=round(moved / us / 1e6 / copy_tb_s, 3))


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
    res = dict(case=name, width=W, height=H, file_bytes=len(data))
    for d in (1, 2, 4, 8):
        us, reps = _median_us(torch, lambda: D.decode_jpeg(data, mode="RGB", scale_denom=d), 1)
        res[f"rgb_d{d}_us"] = round(us, 1)
        res[f"rgb_d{d}_reps_us"] = [round(x, 1) for x in reps]
    # everything up to the coefficient planes (parsing, upload, entropy decode, status read-back) is the same at every scale:
    # timed as the decode with the smallest inverse and no colour stage
    us, _ = _median_us(torch, lambda: D.decode_jpeg(data, scale_denom=8), 1)
    res["planes_d8_us"] = round(us, 1)
    res["share_before_the_inverse_d1"] = round(us / res["rgb_d1_us"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=CASES)
    ap.add_argument("--out")
    ap.add_argument("--timeout", type=int, default=300)
    a = ap.parse_args()
    if a.case:
        res = decode_case(a.case) if a.case.startswith("decode") else inverse_case(a.case)
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
