"""Times encode_jpeg_batch (libmdct_jpegenc_batch.so) against a plain loop of encode_jpeg over the same images.

Two cases: 64 device-resident images of 224 x 224 and 64 of 512 x 512, each a different synthetic photo, written 4:2:0 at quality 75.
Per case, in one process and alternating (batch, loop, batch, loop, ...), after WARM untimed rounds of both:

  batch_ms   encode_jpeg_batch(images), wall clock from the call to the returned list of bytes: planning, allocations, the upload of
             the plan, three launches, the copies of the row offsets and the scans, the marker segments of every file
  loop_ms    [encode_jpeg(x, interleaved=True) for x in images], the same way.  encode_jpeg is what it was before the batch library
             existed, so this column stands for the parent commit.
  launches_us
             the three launches of the batch alone (mdct_jpegenc_batch_planes, _scan, _pack on a plan bound once), between two HIP
             events: device time, no host work.

Medians of REPS repetitions with their minimum and maximum.  The files of both ways are compared (bytes ==) before anything is timed.
One JSON line per case.

    python tools/time_jpeg_encode_batch.py [--images N] [--label TEXT] [--out FILE]     (--out appends)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM, REPS = 3, 11
SIZES = (224, 512)
SUB, QUALITY = "4:2:0", 75


def _stat(v, digits=3):
    return dict(median=round(sorted(v)[len(v) // 2], digits), min_max=[round(min(v), digits), round(max(v), digits)])


def _images(torch, size, n):
    import numpy as np

    from simd_dct_amd import synth

    out = []
    for k in range(n):
        img = np.stack([synth.plane_u8_np(size, size, "photo", seed=1000 * size + 3 * k + c) for c in range(3)], axis=-1)
        out.append(torch.from_numpy(img).cuda())
    return out


def _launches_only(torch, J, images):
    """a plan of the batch bound once over buffers of its own -> (launch, plan, row offsets, capacity, what to keep alive)"""
    sampling = J.sampling_of(SUB)
    described, keep, capacity = [], [], 0
    for im in images:
        H, W = im.shape[:2]
        mcus_x, mcus_y, sizes = J.mcu_grid(W, H, sampling)
        stride = J.scan_seg_stride(mcus_x, sampling)
        planes = [torch.empty((ph, pw), dtype=torch.uint8, device="cuda") for pw, ph in sizes]
        seg = torch.empty((mcus_y * stride,), dtype=torch.uint8, device="cuda")
        keep += planes + [seg]
        described.append((im.data_ptr(), im.stride(0), 0, W, H, [(p.data_ptr(), pw, pw, ph, h, v) for p, (pw, ph), (h, v) in zip(planes, sizes, sampling)],
                          seg.data_ptr(), stride))
        capacity += 2 * mcus_y * stride
    plan = J.BatchPlan(described, "HWC", J.quality_tables(QUALITY))
    counts = torch.empty((2, plan.n_rows), dtype=torch.int32, device="cuda")
    off = torch.empty((plan.n_rows + 1,), dtype=torch.int64, device="cuda")
    out = torch.empty((capacity,), dtype=torch.uint8, device="cuda")
    image = torch.empty(plan.image_bytes, dtype=torch.uint8, device="cuda")
    image.copy_(torch.from_numpy(plan.bind(image, counts[0], counts[1])))
    keep += [counts, out, image]

    def launch():
        plan.planes()
        plan.scan()
        plan.pack(out, off)

    return launch, plan, off, capacity, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--label", default="")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch

    from simd_dct_amd import api
    from simd_dct_amd import jpeg_encode as J

    assert torch.cuda.is_available(), "this tool measures on the GPU"
    api.init(0)
    for size in SIZES:
        images = _images(torch, size, a.images)
        torch.cuda.synchronize()

        def batch():
            return J.encode_jpeg_batch(images, quality=QUALITY, subsampling=SUB)

        def loop():
            return [J.encode_jpeg(x, quality=QUALITY, subsampling=SUB, interleaved=True) for x in images]

        def wall(fn):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            return (time.perf_counter() - t) * 1e3

        got, want = batch(), loop()
        assert len(got) == len(want) == a.images and all(g == w for g, w in zip(got, want))
        file_bytes = sum(map(len, got))
        del got, want
        for _ in range(WARM):
            wall(batch)
            wall(loop)
        tb, tl = [], []
        for _ in range(REPS):
            tb.append(wall(batch))
            tl.append(wall(loop))
        launch, plan, off, capacity, keep = _launches_only(torch, J, images)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        td = []
        for r in range(WARM + REPS):
            start.record()
            launch()
            end.record()
            end.synchronize()
            if r >= WARM:
                td.append(start.elapsed_time(end) * 1e3)
        scan_bytes = int(off[-1].item())
        assert 0 < scan_bytes <= capacity
        counts = dict(rows=plan.n_rows, tiles=plan.n_tiles, scan_bytes=scan_bytes)
        plan.close()
        del keep
        api.kernel_counts_reset()
        batch()
        torch.cuda.synchronize()
        ran_batch = sum(api.kernel_counts().values())
        api.kernel_counts_reset()
        loop()
        torch.cuda.synchronize()
        ran_loop = sum(api.kernel_counts().values())
        res = dict(case="encode_batch", label=a.label, images=a.images, width=size, height=size, subsampling=SUB, quality=QUALITY,
                   file_bytes=file_bytes, device=torch.cuda.get_device_name(0), warm=WARM, reps=REPS,
                   batch_ms=_stat(tb), loop_ms=_stat(tl), launches_us=_stat(td, 1), launches=dict(batch=ran_batch, loop=ran_loop), **counts)
        res["loop_over_batch"] = round(res["loop_ms"]["median"] / res["batch_ms"]["median"], 2)
        res["batch_median_below_loop_min"] = res["batch_ms"]["median"] < res["loop_ms"]["min_max"][0]
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
