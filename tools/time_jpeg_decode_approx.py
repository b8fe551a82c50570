"""Times the decode of progressive files with successive approximation (libjpeg's standard scan script, as Pillow writes it;
libmdct_jpegdec_prog.so) next to the baseline twin of the same picture.

  --make DIR    (needs Pillow, no GPU) writes the files: for 512 x 512 and 2048 x 2048 "photo" pictures (simd_dct_amd.synth) at 4:2:0,
                quality 75: <size>.prog.jpg (restart markers every MCU row), <size>.prog_nomark.jpg (none), <size>.base.jpg (the
                baseline twin, restart markers every MCU row).
  --dir DIR     times them: per scan, the HIP-event median of REPS repetitions of the scan's launches (mdct_jpegdec_index, unless the
                scan has no markers, + mdct_jpegdec_prog_decode_approx) -- the planes are set back to what the earlier scans left
                before every repetition, outside the timed region, because a refinement scan reads them -- summed per scan kind; and
                the wall clock of whole calls: decode_jpeg(mode="RGB") of each progressive file and of the twin (median, min, max).

One JSON line per file.    python tools/time_jpeg_decode_approx.py --dir DIR [--label TEXT] [--out FILE]     (--out appends)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from time_jpeg_transcode import REPS, _stat, _timer  # noqa: E402

SIZES = (512, 2048)
KINDS = ("prog", "prog_nomark", "base")


def make(out):
    import io

    import numpy as np
    from PIL import Image

    from simd_dct_amd import synth

    os.makedirs(out, exist_ok=True)
    for n in SIZES:
        img = Image.fromarray(np.stack([synth.plane_u8_np(n, n, "photo", seed=31 + k) for k in range(3)], axis=-1))
        for kind in KINDS:
            kw = dict(progressive=kind != "base")
            if kind != "prog_nomark":
                kw["restart_marker_rows"] = 1
            f = io.BytesIO()
            img.save(f, "JPEG", quality=75, subsampling="4:2:0", **kw)
            with open(os.path.join(out, f"{n}.{kind}.jpg"), "wb") as fo:
                fo.write(f.getvalue())
            print(f"{n}.{kind}.jpg: {len(f.getvalue())} bytes")


def scan_kind(sc):
    return ("DC" if sc["ss"] == 0 else "AC") + ("_first" if sc["ah"] == 0 else "_refinement")


def per_scan(torch, D, data, info):
    """{scan kind: summed median us}, [per scan], the planes at the end"""
    geo, grid = D.geometry(info)
    coefs = [torch.zeros((by * 8, bx * 8), dtype=torch.int16, device="cuda") for _, _, bx, by in geo]
    timed = _timer(torch)
    kinds, scans = {}, []
    for si, sc in enumerate(info["scans"]):
        specs, desc = D.scan_plan(info, si, sc, geo, grid, coefs)
        tables = D.Tables(specs) if any(s is not None for s in specs) else None
        L = sc["end"] - sc["start"]
        seg = torch.frombuffer(bytearray(data[sc["start"]:sc["end"]]), dtype=torch.uint8).cuda()
        n = D.prog_intervals(desc, sc["ss"], sc["se"])
        marked = sc["restart_interval"] != 0
        off = torch.empty(n + 1, dtype=torch.int64, device="cuda") if marked else torch.tensor([0, L], dtype=torch.int64).cuda()
        status = torch.empty(n, dtype=torch.int32, device="cuda")
        before = [c.clone() for c in coefs]

        def launch():
            if marked:
                D.index(seg, n, off, status, scan_len=L)
            D.decode_prog(desc, sc["ss"], sc["se"], tables, seg, off, status, scan_len=L, ah=sc["ah"], al=sc["al"])

        t = []
        for _ in range(REPS + 1):  # the first warms
            for c, b in zip(coefs, before):
                c.copy_(b)
            torch.cuda.synchronize()
            t.append(timed(launch))
        assert int(status.count_nonzero()) == 0, si
        if tables is not None:
            tables.close()
        st = _stat(t[1:])
        comps = "".join("Y Cb Cr".split()[c["index"]] for c in sc["components"])
        scans.append(dict(scan=f"{comps}_{sc['ss']}_{sc['se']}_ah{sc['ah']}_al{sc['al']}", kind=scan_kind(sc), intervals=n, scan_bytes=L, us=st))
        kinds[scan_kind(sc)] = round(kinds.get(scan_kind(sc), 0.0) + st["median"], 1)
    return kinds, scans, coefs


def wall(torch, D, data):
    t = []
    for _ in range(REPS + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        D.decode_jpeg(data, mode="RGB")
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e6)
    return _stat(t[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--make")
    ap.add_argument("--dir")
    ap.add_argument("--label", default="")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.make:
        make(a.make)
        return 0
    import torch

    from simd_dct_amd import api
    from simd_dct_amd import jpeg_decode as D

    api.init(0)
    for n in SIZES:
        files = {k: open(os.path.join(a.dir, f"{n}.{k}.jpg"), "rb").read() for k in KINDS}
        _, twin = D.decode_coefficients(files["base"])
        base_wall = wall(torch, D, files["base"])
        for kind in KINDS[:2]:
            data = files[kind]
            info = D.read_file(data)
            kinds, scans, coefs = per_scan(torch, D, data, info)
            assert all(torch.equal(g, w) for g, w in zip(coefs, twin)), (n, kind)
            res = dict(case="decode_approx", label=a.label, width=n, height=n, subsampling="4:2:0", quality=75, file=kind, file_bytes=len(data),
                       device=torch.cuda.get_device_name(0), device_us_per_scan_kind=kinds, device_sum_us=round(sum(kinds.values()), 1), scans=scans,
                       decode_jpeg_rgb_wall_us=wall(torch, D, data), baseline_twin_bytes=len(files["base"]), baseline_twin_decode_jpeg_rgb_wall_us=base_wall)
            line = json.dumps(res)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
