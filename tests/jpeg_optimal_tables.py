"""Test-side statement of optimal Huffman tables for a JPEG scan, written from ITU-T T.81 K.2 and the published description of
libjpeg's jpeg_gen_optimal_table; shares no code with simd_dct_amd.

optimal_table(counts) -> (bits16, vals): Figure K.1 with a 257th symbol of frequency 1 (so that no real symbol gets the all-ones code),
ties resolved towards the larger symbol index (`<=` in both searches for the minimum), Figure K.3's adjustment down to 16 bits, the
reserved symbol removed from the longest length in use, the values sorted by code length (before the adjustment), then symbol value.

histogram(frame, scans, planes) -> int64 [2, 272]: the symbols a baseline coder emits for these coefficient planes (the walk of
jpeg_scan_encoder.encode_scan, counting instead of writing): class 0 the first component, class 1 the others; entries 0..15 the DC
categories, 16 + RRRRSSSS the AC symbols; the DC predictor restarts with every restart interval of every scan."""
import numpy as np

import jpeg_scan_encoder as E

CLASS = 272


def optimal_table(counts):
    freq = [int(c) for c in counts] + [0] * (256 - len(counts)) + [1]
    if len(freq) != 257 or not any(freq[:256]):
        raise ValueError("1..256 counts, not all zero")
    codesize, others = [0] * 257, [-1] * 257
    while True:
        c1, v = -1, None
        for i in range(257):
            if freq[i] and (v is None or freq[i] <= v):
                c1, v = i, freq[i]
        c2, v = -1, None
        for i in range(257):
            if freq[i] and i != c1 and (v is None or freq[i] <= v):
                c2, v = i, freq[i]
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    longest = max(codesize)
    bits = [0] * (max(longest, 16) + 2)
    for n in codesize:
        if n:
            bits[n] += 1
    i = longest
    while i > 16:
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
        i -= 1
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1
    vals = [s for n in range(1, longest + 1) for s in range(256) if codesize[s] == n]
    return bits[1:17], vals


def histogram(frame, scans, planes):
    hist = np.zeros((2, CLASS), dtype=np.int64)
    zz = {}
    for ci, p in enumerate(planes):
        p = np.asarray(p, dtype=np.int64)
        rows, cols = p.shape[0] // 8, p.shape[1] // 8
        zz[ci] = p.reshape(rows, 8, cols, 8).transpose(0, 2, 1, 3).reshape(rows, cols, 64)[:, :, E.ZZ]
    for scan in scans:
        order, n_mcus, upm = E.block_order(frame, scan)
        dri = scan.get("dri", 0) or n_mcus
        for k in range(-(-n_mcus // dri)):
            pred = {}
            for ci, by, bx in order[k * dri * upm:min((k + 1) * dri, n_mcus) * upm]:
                h = hist[0 if ci == 0 else 1]
                z = zz[ci][by, bx]
                diff = int(z[0]) - pred.get(ci, 0)
                pred[ci] = int(z[0])
                h[E.category(diff)] += 1
                k0 = 1
                for pos in (np.flatnonzero(z[1:]) + 1).tolist():
                    r = pos - k0
                    h[16 + 0xF0] += r >> 4
                    h[16 + (((r & 15) << 4) | E.category(int(z[pos])))] += 1
                    k0 = pos + 1
                if k0 < 64:
                    h[16] += 1
    return hist


def specs_of(hist, grey=False):
    """{which: (bits16, vals)} keyed like api.huffman_spec"""
    out = {}
    for cls in range(1 if grey else 2):
        out[2 * cls] = optimal_table(hist[cls][:16])
        out[2 * cls + 1] = optimal_table(hist[cls][16:])
    return out


def histogram_of_file(data):
    """the histogram of a file's own scans, from the coefficients the decoding checker reads out of it; and its DHT specifications keyed
    like api.huffman_spec"""
    import jpeg_decode_checker as DC
    from simd_dct_amd import jfif
    planes, statuses, _ = DC.decode(data)
    assert all(s == DC.OK for st in statuses for s in st)
    info = jfif.read_jpeg(data)
    frame = dict(width=info["width"], height=info["height"], comps=[(c["h"], c["v"]) for c in info["components"]])
    scans = [dict(comps=[(c["index"], c["td"], c["ta"]) for c in sc["components"]], dri=sc["restart_interval"]) for sc in info["scans"]]
    ht = info["huffman"]
    return histogram(frame, scans, planes), {2 * th + tc: (list(b), list(v)) for (tc, th), (b, v) in ht.items()}
