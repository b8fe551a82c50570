"""Times progressive output (libmdct_jpegprog.so, simd_dct_amd/jpeg_progressive.py) on the 8192x8192 4:2:0 q75
picture tools/time_jpeg_transcode.py uses, by its method:
  sizes   encode_coefficients(progressive=True) under three band scripts against encode_coefficients(optimize=True), the smallest
          baseline file of the same coefficients; bytes per scan;
  coder   the statistics and the coding launch of every scan of the default script (interleaved DC scan, the luminance bands, Cb, Cr) against
          coef_histogram + coef_rows of the same planes, taken alternately; HIP-event medians of 11 repetitions;
  whole   transcode_jpeg(progressive=True) of the engine's file to bytes, wall clock, next to transcode_jpeg();
  ac      the band coder of the luminance plane's band 6-63 and coef_rows of the same plane, three launches each and little else:
          the process to run under a counter collection.
Each case runs in a child process of its own under `timeout`, one JSON line per case.

    python tools/time_jpeg_progressive.py [--out FILE]      sizes, coder, whole
    python tools/time_jpeg_progressive.py --case NAME        one case, in this process
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from time_jpeg_transcode import H, REPS, W, _picture, _stat, _timer  # noqa: E402

CASES = ["sizes", "coder", "whole"]
SCRIPTS = {"luma_1_5__6_63": [[(1, 5), (6, 63)], [(1, 63)], [(1, 63)]], "luma_1_63": [[(1, 63)], [(1, 63)], [(1, 63)]], "luma_1_2__3_9__10_63": [[(1, 2), (3, 9), (10, 63)], [(1, 63)], [(1, 63)]]}


def _coefficients():
    import torch

    from simd_dct_amd import api
    from simd_dct_amd import jpeg_decode as D
    from simd_dct_amd import jpeg_encode as J

    api.init(0)
    img = torch.from_numpy(_picture()).cuda()
    data = J.encode_jpeg(img, quality=75, interleaved=True)
    info, coefs = D.decode_coefficients(data)
    return torch, data, info, coefs


def _scan_bytes(data):
    """[(components, ss, se, bytes of entropy-coded data)] of a file this engine wrote"""
    out, i = [], 2
    while data[i + 1] != 0xD9:
        m, n = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        seg = data[i + 4:i + 2 + n]
        i += 2 + n
        if m == 0xDA:
            j = i
            while True:
                j = data.index(b"\xff", j)
                if data[j + 1] != 0 and not 0xD0 <= data[j + 1] <= 0xD7:
                    break
                j += 2
            out.append((seg[0], seg[1 + 2 * seg[0]], seg[2 + 2 * seg[0]], j - i))
            i = j
    return out


def sizes_case():
    from simd_dct_amd import jpeg_decode as D
    from simd_dct_amd import jpeg_transcode as TC

    torch, data, info, coefs = _coefficients()
    q = [t.reshape(64).astype("int64") for t in D.component_luts(info)]
    sampling = [(c["h"], c["v"]) for c in info["components"]]
    res = dict(case="sizes", width=W, height=H, input_bytes=len(data))
    for inter in (False, True):
        base = TC.encode_coefficients(coefs, q, W, H, sampling, optimize=True, interleaved=inter)
        r = dict(baseline_optimized=len(base))
        for name, bands in SCRIPTS.items():
            out = TC.encode_coefficients(coefs, q, W, H, sampling, progressive=True, interleaved=inter, bands=bands)
            r[name] = dict(file_bytes=len(out), ratio=round(len(out) / len(base), 4), scans=_scan_bytes(out))
        res["interleaved_dc" if inter else "dc_per_component"] = r
    return res


def coder_case():
    from simd_dct_amd import jpeg_encode as J
    from simd_dct_amd import jpeg_progressive as P
    from simd_dct_amd import jpeg_transcode as TC

    torch, _, info, coefs = _coefficients()
    from simd_dct_amd import api

    sampling = [(c["h"], c["v"]) for c in info["components"]]
    timed = _timer(torch)
    words = torch.zeros((2,), dtype=torch.int32, device="cuda")
    grids = [(p.shape[1] // 8, p.shape[0] // 8) for p in coefs]
    mcus_x, mcus_y = grids[1]
    # one segment buffer for every scan: the largest of the DC scan's MCU rows and each plane's block rows
    seg = torch.empty((max([mcus_y * J.opt_seg_stride(mcus_x * 6)] + [by * J.opt_seg_stride(bx) for bx, by in grids]),), dtype=torch.uint8, device="cuda")
    counts = torch.empty((2, grids[0][1]), dtype=torch.int32, device="cuda")
    dch = torch.empty((2, 272), dtype=torch.int32, device="cuda")
    ach = torch.empty((256,), dtype=torch.int32, device="cuda")
    fns = {}
    # the parent's coder on the same planes: three scans
    specs = J.optimal_tables(TC.coef_histogram(coefs, sampling)[0])

    def base_stats():
        TC.coef_histogram(coefs, sampling, hist=dch, unrepresentable=words[1:2])

    def base_rows():
        for k, p in enumerate(coefs):
            TC.coef_rows(p, (specs[2 * min(k, 1)], specs[2 * min(k, 1) + 1]), seg, counts[0], counts[1], words[0:1], words[1:2])

    fns["baseline_stats"], fns["baseline_rows"] = base_stats, base_rows
    h, _ = P.prog_dc_histogram(coefs, sampling, interleaved=True)
    hc = h.cpu().numpy()
    dspecs = [J.optimal_table(hc[c, :16]) for c in range(2)]
    fns["dc_stats"] = lambda: P.prog_dc_histogram(coefs, sampling, interleaved=True, hist=dch, unrepresentable=words[1:2])
    fns["dc_rows"] = lambda: P.prog_dc_rows(coefs, sampling, dspecs, seg, counts[0], counts[1], words[0:1], words[1:2], interleaved=True)
    for ci, bands in enumerate(P.check_bands(None, 3)):
        for ss, se in bands:
            spec = J.optimal_table(P.prog_ac_histogram(coefs[ci], ss, se)[0].cpu().numpy())
            name = f"{'Y Cb Cr'.split()[ci]}_{ss}_{se}"
            fns[name + "_stats"] = lambda ci=ci, ss=ss, se=se: P.prog_ac_histogram(coefs[ci], ss, se, hist=ach, unrepresentable=words[1:2])
            fns[name + "_rows"] = lambda ci=ci, ss=ss, se=se, spec=spec: P.prog_ac_rows(coefs[ci], ss, se, spec, seg, counts[0], counts[1], words[0:1], words[1:2])
    for fn in fns.values():
        fn()
    t = {k: [] for k in fns}
    for _ in range(REPS):  # alternating
        for k, fn in fns.items():
            t[k].append(timed(fn))
    assert words.cpu().tolist() == [0, 0]
    res = dict(case="coder", width=W, height=H, subsampling="4:2:0")
    res.update({k + "_us": _stat(v) for k, v in t.items()})
    med = {k: _stat(v)["median"] for k, v in t.items()}
    prog = sum(v for k, v in med.items() if not k.startswith("baseline"))
    base = med["baseline_stats"] + med["baseline_rows"]
    res.update(progressive_sum_us=round(prog, 1), baseline_sum_us=round(base, 1), progressive_over_baseline=round(prog / base, 3))
    res["kernels"] = sorted(k for k in api.kernel_counts() if k.startswith(("k_coef", "k_prog")))
    return res


def whole_case():
    from simd_dct_amd import jpeg_transcode as TC

    torch, data, _, _ = _coefficients()
    res = dict(case="whole", width=W, height=H, file_bytes=len(data))
    for label, kw in (("transcode", dict()), ("transcode_progressive", dict(progressive=True)), ("transcode_progressive_interleaved_dc", dict(progressive=True, interleaved=True))):
        TC.transcode_jpeg(data, **kw)
        t = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = TC.transcode_jpeg(data, **kw)
            t.append((time.perf_counter() - t0) * 1e6)
        res[label] = dict(wall_us=_stat(t), file_bytes=len(out))
    return res


def ac_case():
    from simd_dct_amd import jpeg_encode as J
    from simd_dct_amd import jpeg_progressive as P
    from simd_dct_amd import jpeg_transcode as TC

    torch, _, _, coefs = _coefficients()
    y = coefs[0]
    bx, by = y.shape[1] // 8, y.shape[0] // 8
    seg = torch.empty((by * J.opt_seg_stride(bx),), dtype=torch.uint8, device="cuda")
    counts = torch.empty((2, by), dtype=torch.int32, device="cuda")
    words = torch.zeros((2,), dtype=torch.int32, device="cuda")
    spec = J.optimal_table(P.prog_ac_histogram(y, 6, 63)[0].cpu().numpy())
    base = J.optimal_tables(TC.coef_histogram([y], [(1, 1)])[0], grey=True)
    for _ in range(3):  # the luminance plane: its band 6..63, and the baseline coder of the whole block beside it
        P.prog_ac_rows(y, 6, 63, spec, seg, counts[0], counts[1], words[0:1], words[1:2])
        TC.coef_rows(y, (base[0], base[1]), seg, counts[0], counts[1], words[0:1], words[1:2])
    torch.cuda.synchronize()
    return dict(case="ac", launches=6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=CASES + ["ac"])
    ap.add_argument("--out")
    ap.add_argument("--timeout", type=int, default=300)
    a = ap.parse_args()
    if a.case:
        print(json.dumps(dict(sizes=sizes_case, coder=coder_case, whole=whole_case, ac=ac_case)[a.case]()), flush=True)
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
