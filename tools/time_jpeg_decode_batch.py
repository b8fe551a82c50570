"""Times decode_jpeg_batch (libmdct_jpegdec_batch.so) against a plain loop of decode_jpeg over the same files.

Two cases: 64 files of 224 x 224 and 64 files of 512 x 512, each a different synthetic photo, 4:2:0 at quality 75, written by
encode_jpeg(interleaved=True): one interleaved scan with a restart marker after every MCU row.  Per case, in one process and
alternating (batch, loop, batch, loop, ...), after WARM untimed rounds of both:

  batch_ms   decode_jpeg_batch(files, mode="RGB"), wall clock from the call to the end of torch.cuda.synchronize(): parsing, planning,
             uploads, launches, the status copy, the inverse DCT and the colour conversion of every file
  loop_ms    [decode_jpeg(f, mode="RGB") for f in files], the same way.  decode_jpeg is what it was before the batch library
             existed, so this column stands for the parent commit.
  entropy_us the four launches of the batch's entropy stage alone (mdct_jpegdec_batch_index + mdct_jpegdec_batch_decode on a plan
             bound once), between two HIP events: device time, no host work.
  entropy_single_scan_us
             beside it, the same scans through the single-scan library with everything made beforehand (table handles, uploaded
             scans, planes): mdct_jpegdec_index + mdct_jpegdec_decode per scan, four launches each, between two HIP events.

Medians of REPS repetitions with their minimum and maximum.  The results of both ways are compared (torch.equal) before anything is
timed.  One JSON line per case.

    python tools/time_jpeg_decode_batch.py [--files N] [--label TEXT] [--out FILE]     (--out appends)
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


def _stat(v, digits=3):
    return dict(median=round(sorted(v)[len(v) // 2], digits), min_max=[round(min(v), digits), round(max(v), digits)])


def _files(torch, J, size, n):
    import numpy as np

    from simd_dct_amd import synth

    out = []
    for k in range(n):
        img = np.stack([synth.plane_u8_np(size, size, "photo", seed=1000 * size + 3 * k + c) for c in range(3)], axis=-1)
        out.append(J.encode_jpeg(torch.from_numpy(img).cuda(), quality=75, subsampling="4:2:0", interleaved=True))
    return out


def _entropy_only(torch, D, files):
    """the batch's entropy stage on its own, and the same scans one by one through the single-scan library:
    -> (launch, launch_single, status, plan, what to keep alive and close, counts)"""
    scans, blob, keep, single, handles = [], bytearray(), [], [], []
    for data in files:
        info = D.read_file(data)
        geo, grid = D.geometry(info)
        coefs = [torch.zeros((by * 8, bx * 8), dtype=torch.int16, device="cuda") for _, _, bx, by in geo]
        keep.append(coefs)
        for si, sc in enumerate(info["scans"]):
            specs, desc = D.scan_plan(info, si, sc, geo, grid, coefs)
            scans.append((desc, len(blob), sc["end"] - sc["start"], specs))
            n = D.n_intervals(desc)
            handles.append(D.Tables(specs))
            single.append((desc, handles[-1], torch.frombuffer(bytearray(data[sc["start"]:sc["end"]]), dtype=torch.uint8).cuda(), n,
                           torch.empty(n + 1, dtype=torch.int64, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")))
            blob += data[sc["start"]:sc["end"]]
    seg = torch.frombuffer(blob, dtype=torch.uint8).cuda()
    plan = D.BatchPlan(scans, len(blob))
    off = torch.empty(plan.n_offsets, dtype=torch.int64, device="cuda")
    status = torch.empty(plan.n_intervals, dtype=torch.int32, device="cuda")
    image = torch.empty(plan.image_bytes, dtype=torch.uint8, device="cuda")
    image.copy_(torch.from_numpy(plan.bind(image, seg, off, status)))
    keep += [seg, off, image]

    def launch():
        plan.index()
        plan.decode()

    def launch_single():
        for desc, tables, s, n, o, st in single:
            D.index(s, n, o, st)
            D.decode(desc, tables, s, o, st)

    counts = dict(scans=plan.n_scans, intervals=plan.n_intervals, chunks=plan.n_chunks, table_sets=plan.n_table_sets, scan_bytes=len(blob))
    return launch, launch_single, status, plan, (keep, handles), counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--label", default="")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch

    from simd_dct_amd import api
    from simd_dct_amd import jpeg_decode as D
    from simd_dct_amd import jpeg_encode as J

    assert torch.cuda.is_available(), "this tool measures on the GPU"
    api.init(0)
    for size in SIZES:
        files = _files(torch, J, size, a.files)

        def batch():
            return D.decode_jpeg_batch(files, mode="RGB")

        def loop():
            return [D.decode_jpeg(f, mode="RGB") for f in files]

        def wall(fn):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t) * 1e3

        got, want = batch(), loop()
        torch.cuda.synchronize()
        assert len(got) == len(want) and all(torch.equal(g, w) for g, w in zip(got, want))
        del got, want
        for _ in range(WARM):
            wall(batch)
            wall(loop)
        tb, tl = [], []
        for _ in range(REPS):
            tb.append(wall(batch))
            tl.append(wall(loop))
        launch, launch_single, status, plan, keep, counts = _entropy_only(torch, D, files)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        te, ts = [], []
        for r in range(WARM + REPS):
            for fn, t in ((launch, te), (launch_single, ts)):
                start.record()
                fn()
                end.record()
                end.synchronize()
                if r >= WARM:
                    t.append(start.elapsed_time(end) * 1e3)
        assert int(status.count_nonzero()) == 0
        plan.close()
        for h in keep[1]:
            h.close()
        api.kernel_counts_reset()
        batch()
        torch.cuda.synchronize()
        ran_batch = sum(api.kernel_counts().values())
        api.kernel_counts_reset()
        loop()
        torch.cuda.synchronize()
        ran_loop = sum(api.kernel_counts().values())
        res = dict(case="decode_batch", label=a.label, files=a.files, width=size, height=size, subsampling="4:2:0", quality=75,
                   file_bytes=sum(map(len, files)), device=torch.cuda.get_device_name(0), warm=WARM, reps=REPS,
                   batch_ms=_stat(tb), loop_ms=_stat(tl), entropy_us=_stat(te, 1), entropy_single_scan_us=_stat(ts, 1),
                   launches=dict(batch=ran_batch, loop=ran_loop), **counts)
        res["loop_over_batch"] = round(res["loop_ms"]["median"] / res["batch_ms"]["median"], 2)
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
