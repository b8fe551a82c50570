"""Times the GPU JPEG decoder with HIP events (median of 5 rounds of 20 back-to-back decodes), beside the encoder's one-launch scan of
the same 8192^2 grey plane measured in the same process.  Cases:
  grey8192   the engine's 8192^2 grey scan, Annex K.1 (1024 intervals of 1024 blocks)
  frame420   the engine's 7680x4320 4:2:0 frame (BASELINE configs[2]): three non-interleaved scans, K.1 / K.2
  pillow420  Pillow's interleaved 4:2:0 file of the same size, restart_marker_rows=1
Per case: coefficients with the index launches, coefficients with the producer's offsets where the producer knows them (engine scans),
and to pixels (index + decode + mdct_inv_i16_u8_batch).
    python3 tools/time_jpeg_decode.py              every case, each in its own child process under `timeout`
    python3 tools/time_jpeg_decode.py --case NAME  one case in this process"""
import io
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = ("grey8192", "frame420", "pillow420")


def median_us(t, f, reps=20, rounds=5):
    for _ in range(5):
        f()
    r = []
    for _ in range(rounds):
        t.start()
        for _ in range(reps):
            f()
        t.stop()
        r.append(t.elapsed_ms() / reps * 1e3)
    return sorted(r)[rounds // 2]


def run_case(name):
    import numpy as np
    import torch

    import simd_dct_amd as M
    from simd_dct_amd import api, jfif, synth
    from simd_dct_amd import jpeg_decode as D

    M.init(0)
    K1, K2 = synth.JPEG_LUMA, synth.JPEG_CHROMA
    t = M.Timer()
    res = dict(case=name, device=M.device_info()["name"])
    # the shader clock over ~20 ms
    probe = torch.zeros(16, dtype=torch.int64, device="cuda")
    M.clock_probe(probe, 2_000_000, waves=8)
    torch.cuda.synchronize()
    p = probe.cpu().numpy().reshape(8, 2)
    res["shader_clock_ghz"] = round(float((p[:, 0] / (p[:, 1] * 10.0)).mean()), 3)

    def engine_scan(px, W, H, lut, chroma):
        n = H // 8
        stride = api.huffman_seg_stride(W)
        seg = torch.empty((n * stride,), dtype=torch.uint8, device="cuda")
        work = torch.zeros((n + 2,), dtype=torch.int64, device="cuda")
        cap = n * stride * 2
        out = torch.empty((cap,), dtype=torch.uint8, device="cuda")
        off = torch.empty((n + 1,), dtype=torch.int64, device="cuda")
        f = lambda: api.fwd_u8_jpeg_scan(px, W, H, seg, work, out, off, lut=lut, chroma=chroma, out_capacity=cap)
        f()
        total = int(off[-1].item())
        return f, dict(blocks_per_row=W // 8, qtable=lut, scan=out[:total].cpu().numpy()), off

    offs = None
    if name == "grey8192":
        W = H = 8192
        px = synth.plane_u8_torch(W, H, "photo")
        f, comp, off = engine_scan(px, W, H, K1, False)
        res["encoder_scan_us"] = round(median_us(t, f), 1)
        data, offs = jfif.write_jpeg([comp], W, H), [off]
    else:
        W, H = 7680, 4320
        ycc = torch.stack([synth.plane_u8_torch(W, H, "photo", seed=s) for s in (5, 6, 7)], dim=-1).contiguous()
        if name == "frame420":
            y = torch.empty((H, W), dtype=torch.uint8, device="cuda")
            cb = torch.empty((H // 2, W // 2), dtype=torch.uint8, device="cuda")
            cr = torch.empty_like(cb)
            api.split420_u8_planes(ycc, W, H, y, cb, cr)
            comps, offs = [], []
            for px, w, h, lut, chroma in ((y, W, H, K1, False), (cb, W // 2, H // 2, K2, True), (cr, W // 2, H // 2, K2, True)):
                _, comp, off = engine_scan(px, w, h, lut, chroma)
                comps.append(comp)
                offs.append(off)
            data = jfif.write_jpeg(comps, W, H)
        else:
            from PIL import Image
            buf = io.BytesIO()
            Image.fromarray(ycc.cpu().numpy(), "YCbCr").save(buf, "JPEG", quality=75, subsampling=2, restart_marker_rows=1)
            data = buf.getvalue()
    res["file_bytes"] = len(data)
    # everything decode_jpeg does on the device, prepared once
    info = jfif.read_jpeg(data)
    geo, grid = D.geometry(info)
    coefs = [torch.empty((by * 8, bx * 8), dtype=torch.int16, device="cuda") for _, _, bx, by in geo]
    pxs = [torch.empty((by * 8, bx * 8), dtype=torch.uint8, device="cuda") for _, _, bx, by in geo]
    luts = [info["qtables"][c["tq"]].astype(np.float32) for c in info["components"]]
    scans = []
    for sc in info["scans"]:
        mcus_x, mcus_y, members = D.scan_geometry(info, sc, geo, grid)
        specs = [None] * 4
        planes = []
        for c, (ci, h, v) in zip(sc["components"], members):
            specs[c["td"]] = sc["huffman"][(0, c["td"])]
            specs[2 + c["ta"]] = sc["huffman"][(1, c["ta"])]
            planes.append((coefs[ci], geo[ci][2], geo[ci][3], h, v, c["td"], 2 + c["ta"]))
        desc = D.scan_desc(planes, mcus_x, mcus_y, sc["restart_interval"])
        n = D.n_intervals(desc)
        seg = torch.frombuffer(bytearray(data[sc["start"]:sc["end"]]), dtype=torch.uint8).cuda()
        scans.append((desc, D.Tables(specs), seg, n, torch.empty(n + 1, dtype=torch.int64, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")))
    res["intervals"] = [s[3] for s in scans]
    res["scan_bytes"] = [int(s[2].numel()) for s in scans]

    def coefficients():
        for desc, tab, seg, n, off, st in scans:
            D.index(seg, n, off, st)
            D.decode(desc, tab, seg, off, st)

    def to_pixels():
        coefficients()
        api.u8_i16_batch("inv", [(p, q, g[2] * 8, g[3] * 8, lut) for p, q, g, lut in zip(pxs, coefs, geo, luts)])

    coefficients()
    torch.cuda.synchronize()
    assert all(int(s[5].abs().sum()) == 0 for s in scans), "an interval failed"
    res["coefficients_us"] = round(median_us(t, coefficients), 1)
    if offs is not None:
        def decode_only():
            for (desc, tab, seg, n, _, st), off in zip(scans, offs):
                D.decode(desc, tab, seg, off, st)
        res["coefficients_producer_offsets_us"] = round(median_us(t, decode_only), 1)
    res["to_pixels_us"] = round(median_us(t, to_pixels), 1)
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
