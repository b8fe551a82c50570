"""Times the GPU decoder of scans without restart markers against the marked path on the same picture, in the same process, with HIP
events (median of 5 rounds of 20 back-to-back decodes, coefficients only; uploads and host parsing excluded).  Cases:
  grey8192   Pillow 8192^2 grey, quality 75: no markers / restart_marker_rows=1
  pillow420  Pillow 7680x4320 interleaved 4:2:0, quality 75: no markers / restart_marker_rows=1
Per case it also reports the last fix round in which a chunk's state changed (the fix rounds after it return at once).
    python3 tools/time_jpeg_decode_unmarked.py              every case, each in its own child process under `timeout`
    python3 tools/time_jpeg_decode_unmarked.py --case NAME  one case in this process
For each kernel's share, run one case under `rocprofv3 --kernel-trace --stats -- python3 ... --case NAME` in a run of its own."""
import io
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
CASES = ("grey8192", "pillow420")

from time_jpeg_decode import median_us  # noqa: E402


def prepare(torch, D, jfif, data):
    """device buffers of every scan of the file -> (coefficient planes, one call that decodes them all)"""
    info = jfif.read_jpeg(data, require_restart=False)
    geo, grid = D.geometry(info)
    coefs = [torch.empty((by * 8, bx * 8), dtype=torch.int16, device="cuda") for _, _, bx, by in geo]
    calls, works = [], []
    for si, sc in enumerate(info["scans"]):
        specs, desc = D.scan_plan(info, si, sc, geo, grid, coefs)
        tab = D.Tables(specs)
        seg = torch.frombuffer(bytearray(data[sc["start"]:sc["end"]]), dtype=torch.uint8).cuda()
        if sc["restart_interval"] == 0:
            work = torch.empty(D.unmarked_workspace(desc, seg.numel()), dtype=torch.uint8, device="cuda")
            st = torch.empty(2, dtype=torch.int32, device="cuda")
            calls.append(lambda desc=desc, tab=tab, seg=seg, work=work, st=st: D.decode_unmarked(desc, tab, seg, work, st))
            works.append((work, st, seg.numel()))
        else:
            n = D.n_intervals(desc)
            off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
            st = torch.empty(n, dtype=torch.int32, device="cuda")

            def f(desc=desc, tab=tab, seg=seg, n=n, off=off, st=st):
                D.index(seg, n, off, st)
                D.decode(desc, tab, seg, off, st)
            calls.append(f)
            works.append((None, st, seg.numel()))

    def run():
        for f in calls:
            f()
    return coefs, run, works


def run_case(name):
    import numpy as np
    import torch
    from PIL import Image

    import simd_dct_amd as M
    from simd_dct_amd import jfif, synth
    from simd_dct_amd import jpeg_decode as D

    M.init(0)
    t = M.Timer()
    res = dict(case=name, device=M.device_info()["name"])
    probe = torch.zeros(16, dtype=torch.int64, device="cuda")
    M.clock_probe(probe, 2_000_000, waves=8)
    torch.cuda.synchronize()
    p = probe.cpu().numpy().reshape(8, 2)
    res["shader_clock_ghz"] = round(float((p[:, 0] / (p[:, 1] * 10.0)).mean()), 3)
    if name == "grey8192":
        img, mode, kw = synth.plane_u8_np(8192, 8192, "photo"), "L", dict(quality=75)
    else:
        img = np.stack([synth.plane_u8_np(7680, 4320, "photo", seed=s) for s in (5, 6, 7)], axis=-1)
        mode, kw = "YCbCr", dict(quality=75, subsampling=2)
    files = {}
    for key, extra in (("unmarked", {}), ("marked", dict(restart_marker_rows=1))):
        buf = io.BytesIO()
        Image.fromarray(img, mode).save(buf, "JPEG", **kw, **extra)
        files[key] = buf.getvalue()
    out = {}
    for key, data in files.items():
        coefs, run, works = prepare(torch, D, jfif, data)
        run()
        torch.cuda.synchronize()
        for work, st, _ in works:  # unmarked: [status, blocks]; marked: one status per interval
            assert int((st[:1] if work is not None else st).abs().sum()) == 0, (key, st.cpu().numpy()[:4])
        res[f"{key}_scan_bytes"] = [n for _, _, n in works]
        res[f"{key}_coefficients_us"] = round(median_us(t, run), 1)
        if key == "unmarked":
            res["unmarked_chunks"] = [-(-n // 8192) for _, _, n in works]
            res["unmarked_last_changing_round"] = [int(w[:4].view(torch.int32)[0]) for w, _, _ in works]
        out[key] = coefs
    res["identical_planes"] = all(bool(torch.equal(a, b)) for a, b in zip(out["unmarked"], out["marked"]))
    res["unmarked_over_marked"] = round(res["unmarked_coefficients_us"] / res["marked_coefficients_us"], 3)
    print(json.dumps(res), flush=True)


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--case":
        return run_case(sys.argv[2])
    for c in CASES:
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--case", c])
        if r.returncode != 0:
            print(f"case {c}: exit status {r.returncode}; stopping", flush=True)
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
