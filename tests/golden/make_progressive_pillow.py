"""Generates tests/golden/progressive_pillow/: small progressive JPEG files as libjpeg's standard scan script writes them (Pillow's
progressive=True: successive approximation, 6 scans for a grey picture, 10 for a colour one with the luma AC refined twice), each with
and without restart markers, and the BASELINE TWIN of every picture: the same image, quality and subsampling with progressive=False.
libjpeg quantises once and differs only in the entropy coding, so a progressive file and its twin hold identical coefficients; the
script checks that they decode to equal pixels.  The tests read the files only: the machine that runs them needs no Pillow.

    python tests/golden/make_progressive_pillow.py

Files: <picture>.prog.jpg (restart markers every MCU row of each scan), <picture>.prog_nomark.jpg (none), <picture>.base.jpg (the twin,
restart markers every MCU row), and for one picture <picture>.prog_b3.jpg (a restart interval of 3 MCUs: intervals that end mid-row).
"""
import io
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "progressive_pillow")


def smooth(w, h, ch):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    planes = [128 + 100 * np.sin(x / (9.0 + 3 * c) + c) * np.cos(y / (7.0 + 2 * c)) for c in range(ch)]
    return np.clip(np.stack(planes, axis=-1), 0, 255).astype(np.uint8)


def noisy(w, h, ch, seed, amp):
    rng = np.random.default_rng(seed)
    base = smooth(w, h, ch).astype(np.float64)
    return np.clip(base + rng.normal(0, amp, base.shape), 0, 255).astype(np.uint8)


# name: (pixels [h, w, channels], quality, Pillow's subsampling or None for grey)
PICTURES = {
    "grey_8x8": (noisy(8, 8, 1, 1, 40), 90, None),
    "c420_17x9": (noisy(17, 9, 3, 2, 30), 90, "4:2:0"),
    "c422_50x35": (noisy(50, 35, 3, 3, 25), 90, "4:2:2"),
    "c444_50x35": (noisy(50, 35, 3, 4, 25), 90, "4:4:4"),
    "smooth_64x48_q30": (smooth(64, 48, 3), 30, "4:2:0"),
    "noisy_64x48_q95": (noisy(64, 48, 3, 5, 60), 95, "4:2:0"),
    "noisy_64x48_q100": (noisy(64, 48, 1, 6, 70), 100, None),
    "noisy_203x117_q90": (noisy(203, 117, 3, 7, 14), 90, "4:2:0"),
}
BLOCKS3 = "c444_50x35"


def save(img, quality, subsampling, **kw):
    f = io.BytesIO()
    if subsampling is not None:
        kw["subsampling"] = subsampling
    img.save(f, "JPEG", quality=quality, **kw)
    return f.getvalue()


def main():
    os.makedirs(OUT, exist_ok=True)
    for name, (px, quality, subsampling) in PICTURES.items():
        img = Image.fromarray(px[..., 0] if px.shape[-1] == 1 else px)
        files = {
            "base": save(img, quality, subsampling, progressive=False, restart_marker_rows=1),
            "prog": save(img, quality, subsampling, progressive=True, restart_marker_rows=1),
            "prog_nomark": save(img, quality, subsampling, progressive=True),
        }
        if name == BLOCKS3:
            files["prog_b3"] = save(img, quality, subsampling, progressive=True, restart_marker_blocks=3)
        want = np.asarray(Image.open(io.BytesIO(files["base"])))
        for kind, data in files.items():
            assert len(data) < 16384, (name, kind, len(data))
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), want), (name, kind)
            n_scans = data.count(b"\xff\xda")
            assert n_scans == (1 if kind == "base" else 6 if subsampling is None else 10), (name, kind, n_scans)
            with open(os.path.join(OUT, f"{name}.{kind}.jpg"), "wb") as fo:
                fo.write(data)
            print(f"{name}.{kind}.jpg: {len(data)} bytes, {n_scans} scans")


if __name__ == "__main__":
    main()
