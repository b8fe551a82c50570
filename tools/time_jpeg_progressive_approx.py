"""Times progressive output with successive approximation (libmdct_jpegprog.so, simd_dct_amd/jpeg_progressive.py; DESIGN.md section
4.12.1) on the 8192x8192 4:2:0 q75 picture of tools/time_jpeg_progressive.py, by its method: the statistics and the coding launch of
every scan, HIP-event medians of 11 repetitions taken alternately, and the size of the file encode_coefficients writes.

  default    script=None, the file progressive=True has always written (DC per component, the default bands), next to the baseline
             coder (coef_histogram + coef_rows, the optimize=True file) of the same planes.  Uses nothing this script's commit added,
             so --tree DIR times another checkout of the engine (the parent commit, built) with the same code: before and after.
  standard   script="standard", libjpeg's ten scans, per scan kind.
Each case runs in a child process of its own under `timeout`, one JSON line per case.

    python tools/time_jpeg_progressive_approx.py [--out FILE] [--label TEXT] [--tree DIR] [--cases default,standard]
    python tools/time_jpeg_progressive_approx.py --case NAME [--tree DIR]      one case, in this process
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["default", "standard"]
W = H = 8192
REPS = 11


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


def _setup():
    import numpy as np
    import torch

    from simd_dct_amd import api, synth
    from simd_dct_amd import jpeg_decode as D
    from simd_dct_amd import jpeg_encode as J

    api.init(0)
    img = torch.from_numpy(np.stack([synth.plane_u8_np(W, H, "photo", seed=31 + k) for k in range(3)], axis=-1)).cuda()
    data = J.encode_jpeg(img, quality=75, interleaved=True)
    info, coefs = D.decode_coefficients(data)
    q = [t.reshape(64).astype("int64") for t in D.component_luts(info)]
    sampling = [(c["h"], c["v"]) for c in info["components"]]
    return torch, coefs, q, sampling


def _buffers(torch, J, coefs):
    grids = [(p.shape[1] // 8, p.shape[0] // 8) for p in coefs]
    mcus_x, mcus_y = grids[1]
    seg = torch.empty((max([mcus_y * J.opt_seg_stride(mcus_x * 6)] + [by * J.opt_seg_stride(bx) for bx, by in grids]),), dtype=torch.uint8, device="cuda")
    counts = torch.empty((2, grids[0][1]), dtype=torch.int32, device="cuda")
    return seg, counts, torch.zeros((2,), dtype=torch.int32, device="cuda")


def _run(torch, fns):
    """{name: us statistics} of the launches, each taken REPS times in turn after one warming round"""
    timed = _timer(torch)
    for fn in fns.values():
        fn()
    t = {k: [] for k in fns}
    for _ in range(REPS):
        for k, fn in fns.items():
            t[k].append(timed(fn))
    return {k: _stat(v) for k, v in t.items()}


def default_case():
    from simd_dct_amd import jpeg_encode as J
    from simd_dct_amd import jpeg_progressive as P
    from simd_dct_amd import jpeg_transcode as TC

    torch, coefs, q, sampling = _setup()
    seg, counts, words = _buffers(torch, J, coefs)
    dch = torch.empty((2, 272), dtype=torch.int32, device="cuda")
    ach = torch.empty((256,), dtype=torch.int32, device="cuda")
    specs = J.optimal_tables(TC.coef_histogram(coefs, sampling)[0])
    fns = {"baseline_stats": lambda: TC.coef_histogram(coefs, sampling, hist=dch, unrepresentable=words[1:2])}

    def base_rows():
        for k, p in enumerate(coefs):
            TC.coef_rows(p, (specs[2 * min(k, 1)], specs[2 * min(k, 1) + 1]), seg, counts[0], counts[1], words[0:1], words[1:2])

    fns["baseline_rows"] = base_rows
    names = "Y Cb Cr".split()
    for ci, p in enumerate(coefs):
        hc = P.prog_dc_histogram([p], [sampling[ci]], cls=min(ci, 1))[0].cpu().numpy()
        dspec = [J.optimal_table(hc[min(ci, 1), :16])]
        fns[f"{names[ci]}_dc_stats"] = lambda p=p, ci=ci: P.prog_dc_histogram([p], [sampling[ci]], cls=min(ci, 1), hist=dch, unrepresentable=words[1:2])
        fns[f"{names[ci]}_dc_rows"] = lambda p=p, ci=ci, dspec=dspec: P.prog_dc_rows([p], [sampling[ci]], dspec, seg, counts[0], counts[1], words[0:1], words[1:2])
    for ci, bands in enumerate(P.check_bands(None, 3)):
        for ss, se in bands:
            spec = J.optimal_table(P.prog_ac_histogram(coefs[ci], ss, se)[0].cpu().numpy())
            fns[f"{names[ci]}_{ss}_{se}_stats"] = lambda ci=ci, ss=ss, se=se: P.prog_ac_histogram(coefs[ci], ss, se, hist=ach, unrepresentable=words[1:2])
            fns[f"{names[ci]}_{ss}_{se}_rows"] = lambda ci=ci, ss=ss, se=se, spec=spec: P.prog_ac_rows(coefs[ci], ss, se, spec, seg, counts[0], counts[1], words[0:1], words[1:2])
    us = _run(torch, fns)
    assert words.cpu().tolist() == [0, 0]
    prog = sum(v["median"] for k, v in us.items() if not k.startswith("baseline"))
    base = us["baseline_stats"]["median"] + us["baseline_rows"]["median"]
    return dict(case="default", width=W, height=H, subsampling="4:2:0", quality=75, device=torch.cuda.get_device_name(0), us=us, progressive_sum_us=round(prog, 1),
                baseline_sum_us=round(base, 1), progressive_file_bytes=len(TC.encode_coefficients(coefs, q, W, H, sampling, progressive=True)),
                baseline_optimized_file_bytes=len(TC.encode_coefficients(coefs, q, W, H, sampling, optimize=True)))


def standard_case():
    from simd_dct_amd import jpeg_encode as J
    from simd_dct_amd import jpeg_progressive as P
    from simd_dct_amd import jpeg_transcode as TC

    torch, coefs, q, sampling = _setup()
    seg, counts, words = _buffers(torch, J, coefs)
    dch = torch.empty((2, 272), dtype=torch.int32, device="cuda")
    ach = torch.empty((256,), dtype=torch.int32, device="cuda")
    names = "Y Cb Cr".split()
    fns, kind_of = {}, {}
    for comps, ss, se, ah, al in P.standard_script(3):
        name = f"{''.join(names[c] for c in comps)}_{ss}_{se}_ah{ah}_al{al}"
        kind = ("DC" if ss == 0 else "AC") + ("_refinement" if ah else "_first")
        if ss == 0 and ah == 0:
            hc = P.prog_dc_histogram(coefs, sampling, interleaved=True, al=al)[0].cpu().numpy()
            dspecs = [J.optimal_table(hc[c, :16]) for c in range(2)]
            fns[name + "_stats"] = lambda al=al: P.prog_dc_histogram(coefs, sampling, interleaved=True, hist=dch, unrepresentable=words[1:2], al=al)
            fns[name + "_rows"] = lambda al=al, dspecs=dspecs: P.prog_dc_rows(coefs, sampling, dspecs, seg, counts[0], counts[1], words[0:1], words[1:2], interleaved=True, al=al)
            kind_of[name + "_stats"] = kind_of[name + "_rows"] = kind
        elif ss == 0:
            fns[name + "_rows"] = lambda ah=ah, al=al: P.prog_dc_rows(coefs, sampling, None, seg, counts[0], counts[1], words[0:1], words[1:2], interleaved=True, ah=ah, al=al)
            kind_of[name + "_rows"] = kind
        else:
            p = coefs[comps[0]]
            spec = J.optimal_table(P.prog_ac_histogram(p, ss, se, ah=ah, al=al)[0].cpu().numpy())
            fns[name + "_stats"] = lambda p=p, ss=ss, se=se, ah=ah, al=al: P.prog_ac_histogram(p, ss, se, hist=ach, unrepresentable=words[1:2], ah=ah, al=al)
            fns[name + "_rows"] = lambda p=p, ss=ss, se=se, ah=ah, al=al, spec=spec: P.prog_ac_rows(p, ss, se, spec, seg, counts[0], counts[1], words[0:1], words[1:2], ah=ah,
                                                                                                      al=al)
            kind_of[name + "_stats"] = kind_of[name + "_rows"] = kind
    us = _run(torch, fns)
    assert words.cpu().tolist() == [0, 0]
    kinds = {}
    for k, v in us.items():
        kinds[kind_of[k]] = round(kinds.get(kind_of[k], 0.0) + v["median"], 1)
    return dict(case="standard", width=W, height=H, subsampling="4:2:0", quality=75, device=torch.cuda.get_device_name(0), us=us, us_per_scan_kind=kinds,
                standard_sum_us=round(sum(v["median"] for v in us.values()), 1),
                standard_file_bytes=len(TC.encode_coefficients(coefs, q, W, H, sampling, progressive=True, script="standard")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=CASES)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--tree", default=ROOT, help="the checkout whose simd_dct_amd is timed (default: this one)")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", help="append the JSON lines to this file")
    ap.add_argument("--timeout", type=int, default=300)
    a = ap.parse_args()
    if a.case:
        sys.path.insert(0, os.path.abspath(a.tree))
        print(json.dumps(dict(default=default_case, standard=standard_case)[a.case]()), flush=True)
        return 0
    rc = 0
    for name in a.cases.split(","):
        p = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--case", name, "--tree", a.tree], capture_output=True, text=True)
        if p.returncode != 0:
            print(json.dumps(dict(case=name, label=a.label, returncode=p.returncode, stderr=p.stderr[-2000:])), flush=True)
            rc = p.returncode
            break  # a failed or faulted child ends the run: nothing more is started on the device
        res = json.loads(p.stdout.strip().splitlines()[-1])
        res["label"] = a.label
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
