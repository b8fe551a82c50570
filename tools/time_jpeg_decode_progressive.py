"""Times the entropy decode of a progressive file (libmdct_jpegdec_prog.so) on the 8192x8192 4:2:0 q75 picture
tools/time_jpeg_transcode.py uses, by the method of tools/time_jpeg_progressive.py: HIP-event medians of 11 alternating repetitions.

  progressive   the picture's coefficients written by encode_coefficients(progressive=True) with the default bands: every scan's
                mdct_jpegdec_index + mdct_jpegdec_prog_decode, per scan and in sum -- coefficients only, no inverse DCT;
  baseline      beside it, in the same process and the same alternation, the three scans of encode_coefficients(optimize=True)'s
                file of the same coefficients: mdct_jpegdec_index + mdct_jpegdec_decode.

One JSON line.  --baseline-only times the baseline file alone and uses nothing newer than decode_coefficients, so the same script
measures an older checkout: the existing decoder's figures before and after a change, in the order old / new / old.

    python tools/time_jpeg_decode_progressive.py [--baseline-only] [--label TEXT] [--out FILE]     (--out appends)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from time_jpeg_transcode import H, REPS, W, _picture, _stat, _timer  # noqa: E402


def _scans(torch, D, data, info):
    """every scan of the file ready to decode: [(name, launch)], the planes they fill, what to close afterwards"""
    geo, grid = D.geometry(info)
    coefs = [torch.zeros((by * 8, bx * 8), dtype=torch.int16, device="cuda") for _, _, bx, by in geo]
    out, keep = [], []
    for si, sc in enumerate(info["scans"]):
        specs, desc = D.scan_plan(info, si, sc, geo, grid, coefs)
        tables = D.Tables(specs)
        L = sc["end"] - sc["start"]
        seg = torch.frombuffer(bytearray(data[sc["start"]:sc["end"]]), dtype=torch.uint8).cuda()
        band = (sc["ss"], sc["se"]) if "ss" in sc else None
        n = D.n_intervals(desc) if band is None else D.prog_intervals(desc, *band)
        off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        status = torch.empty(n, dtype=torch.int32, device="cuda")

        def launch(desc=desc, tables=tables, seg=seg, off=off, status=status, n=n, L=L, band=band):
            D.index(seg, n, off, status, scan_len=L)
            if band is None:
                D.decode(desc, tables, seg, off, status, scan_len=L)
            else:
                D.decode_prog(desc, band[0], band[1], tables, seg, off, status, scan_len=L)

        comps = "".join("Y Cb Cr".split()[c["index"]] for c in sc["components"])
        out.append((f"{comps}_{band[0]}_{band[1]}" if band else comps, launch, status, L, n))
        keep.append(tables)
    return out, coefs, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch

    from simd_dct_amd import api, jfif
    from simd_dct_amd import jpeg_decode as D
    from simd_dct_amd import jpeg_encode as J
    from simd_dct_amd import jpeg_transcode as TC

    api.init(0)
    img = torch.from_numpy(_picture()).cuda()
    info, coefs = D.decode_coefficients(J.encode_jpeg(img, quality=75, interleaved=True))
    del img
    q = [t.reshape(64).astype("int64") for t in D.component_luts(info)]
    sampling = [(c["h"], c["v"]) for c in info["components"]]
    files = {"baseline": TC.encode_coefficients(coefs, q, W, H, sampling, optimize=True)}
    if not a.baseline_only:
        files["progressive"] = TC.encode_coefficients(coefs, q, W, H, sampling, progressive=True)
    want = [c.clone() for c in coefs]
    del coefs
    res = dict(case="decode", label=a.label, width=W, height=H, subsampling="4:2:0", device=torch.cuda.get_device_name(0))
    fns, planes, keep = {}, {}, []
    for kind, data in files.items():
        parsed = jfif.read_jpeg(data, require_restart=False) if kind == "baseline" else jfif.read_progressive_jpeg(data)
        scans, planes[kind], k = _scans(torch, D, data, parsed)
        keep += k
        res[kind + "_file_bytes"] = len(data)
        for name, launch, status, L, n in scans:
            fns[f"{kind}_{name}"] = (launch, status, L, n)
    for launch, status, _, _ in fns.values():  # warm, and right
        launch()
        assert int(status.count_nonzero()) == 0
    for kind, got in planes.items():
        for g, w in zip(got, want):
            assert torch.equal(g, w), kind
    timed = _timer(torch)
    t = {k: [] for k in fns}
    for _ in range(REPS):  # alternating
        for k, (launch, _, _, _) in fns.items():
            t[k].append(timed(launch))
    for k, v in t.items():
        res[k + "_us"] = dict(_stat(v), scan_bytes=fns[k][2], intervals=fns[k][3])
    for kind in files:
        res[kind + "_sum_us"] = round(sum(_stat(v)["median"] for k, v in t.items() if k.startswith(kind + "_")), 1)
    if not a.baseline_only:
        res["progressive_over_baseline"] = round(res["progressive_sum_us"] / res["baseline_sum_us"], 3)
    res["kernels"] = sorted(k for k in api.kernel_counts() if k.startswith(("k_decode", "k_rst")))
    for tb in keep:
        tb.close()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
