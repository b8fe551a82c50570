"""Every kernel instantiation in the library's gfx950 code objects has a case here, and every case proves which instantiation ran.

CPU: the code objects are unbundled from libmdct_hip.so and their kernel symbols listed; that set must equal the matrix's kernels
plus ALLOWLIST, so a new instantiation without a case, or a case for a kernel that is gone, fails.

GPU: for each matrix row the launch tally (mdct_kernel_counts) is reset, the public call runs, and the tally must name exactly the
expected instantiation(s) -- a dispatch change that moves the shape to another form fails with both names.  The output (canaries
included) is compared with the CPU checker byte for byte, and the engine's own forward transforms also with the double-precision
definition, which does not depend on the checker."""
import os
import struct
import subprocess

import numpy as np
import pytest

import idct_reference as R
import oracle as O
import simd_dct_amd as M
from simd_dct_amd import api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "simd_dct_amd", "libmdct_hip.so")
LLVM = "/opt/rocm/llvm/bin"

# kernels in the code object that no case launches, each with its reason
ALLOWLIST = {
    "k_clock_probe": "diagnostics only (mdct_clock_probe spins for a wall-clock time); computes nothing to compare",
}

BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _kernel_name(demangled):
    """'void mdct::k_f32<0, true>(mdct::F32Args)' -> 'k_f32<0, true>' (what mdct_kernel_counts reports)"""
    s = demangled[5:] if demangled.startswith("void ") else demangled
    s = s.split("(", 1)[0]
    t = s.find("<")
    ns = s.rfind("::", 0, t if t >= 0 else len(s))
    return s[ns + 2:] if ns >= 0 else s


def code_object_kernels(lib=LIB, workdir=None):
    """kernel names of every gfx950 code object in lib's .hip_fatbin (one offload bundle per translation unit)"""
    import tempfile
    with tempfile.TemporaryDirectory(dir=workdir) as tmp:
        fat = os.path.join(tmp, "fatbin")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, os.path.join(tmp, "lib.copy")], check=True)
        data = open(fat, "rb").read()
        names, n_objects, pos = set(), 0, 0
        while (pos := data.find(BUNDLE_MAGIC, pos)) >= 0:
            (n_entries,) = struct.unpack_from("<Q", data, pos + 24)
            p = pos + 32
            for _ in range(n_entries):
                off, size, tlen = struct.unpack_from("<QQQ", data, p)
                triple = data[p + 24:p + 24 + tlen].decode()
                p += 24 + tlen
                if "gfx950" in triple and size:
                    obj = os.path.join(tmp, f"dev{n_objects}.o")
                    with open(obj, "wb") as f:
                        f.write(data[pos + off:pos + off + size])
                    n_objects += 1
                    out = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-s", "--demangle", obj], check=True, capture_output=True, text=True).stdout
                    for line in out.splitlines():
                        parts = line.split(None, 7)
                        if len(parts) == 8 and parts[3] == "FUNC" and not parts[7].endswith(".kd"):
                            names.add(_kernel_name(parts[7]))
            pos += len(BUNDLE_MAGIC)
    return names, n_objects


# ------------------------------------------------------------------------------------------ inputs
RNG_SEED = 20261015


def rng(k=0):
    return np.random.default_rng(RNG_SEED + k)


def u8_full(W, H, k=0):
    return rng(k).integers(0, 256, (H, W), dtype=np.uint8)


def i16_full(W, H, k=0):
    return rng(k).integers(-32768, 32768, (H, W), dtype=np.int16)


def i16_worst(W, H):
    """block (u, v) = the sign pattern of basis function (u, v) at -32768 / 32767 (the largest coefficients int16 samples make),
    the complement below; tiled over the plane"""
    xs = np.arange(8)
    cosm = np.cos((2 * xs[None, :] + 1) * xs[:, None] * np.pi / 16)
    tile = np.zeros((16, 512), dtype=np.int16)
    for u in range(8):
        for v in range(8):
            blk = np.where(np.outer(cosm[v], cosm[u]) > 0, 32767, -32768).astype(np.int16)
            tile[0:8, (u * 8 + v) * 8:(u * 8 + v) * 8 + 8] = blk
            tile[8:16, (u * 8 + v) * 8:(u * 8 + v) * 8 + 8] = -1 - blk
    return np.ascontiguousarray(np.tile(tile, (H // 16 + 1, W // 512 + 1))[:H, :W])


def lut_random(k=0, lo=0.5, hi=40.0):
    return rng(100 + k).uniform(lo, hi, 64).astype(np.float32)


EXTREME_ENTRIES = (0.0, 1e-30, -1e-30, -0.3, np.inf, -np.inf, np.nan, 3e38)


def lut_extreme():
    """the reference's quantiser tables can hold anything: every integer-indefinite corner of cvtps_epi32 in one table"""
    lut = M.QUANTIZE_BASE.copy()
    for i, v in enumerate(EXTREME_ENTRIES):
        lut[i * 7 + 1] = v
    return lut


# ------------------------------------------------------------------------------------------ cases
MATRIX = []  # (kernels, call, description, run)


def case(kernels, call, desc):
    def reg(fn):
        MATRIX.append((tuple([kernels] if isinstance(kernels, str) else kernels), call, desc, fn))
        return fn
    return reg


def _blocks(a, W, H):
    return a.reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 64)


def check_i16_fwd_vs_double(src, got, W, H, lut, by0=0, by1=None, u8_shift=None):
    """|got - sat(rint(f64 DCT / lut))| <= 1 on the block rows computed"""
    by1 = H // 8 if by1 is None else by1
    x = src.astype(np.float32) - (np.float32(u8_shift) if u8_shift else np.float32(0))
    ref = O.f32("f64ref", x, W, H)
    q = 1.0 if lut is None else np.tile(lut.reshape(8, 8).astype(np.float64), (H // 8, W // 8))
    want = np.clip(np.rint(ref / q), -32768, 32767)
    d = np.abs(got.astype(np.float64) - want)[by0 * 8:by1 * 8]
    assert d.max() <= 1, ("int16 forward vs double", float(d.max()))
    # and the exact rule wherever the window decides (tests/test_fdct_accuracy.py chooses inputs that it mostly does; these full-scale
    # planes are taken as they are, so no floor on the decided share here)
    rows = slice(by0 * 8, by1 * 8)
    R.check_planes("fwd_u8" if u8_shift else "fwd_i16", [np.asarray(src)[rows]], [np.asarray(got)[rows]], [lut], min_decided=0.0)


def check_f32_vs_double(src, got, W, H):
    want = O.f32("f64ref", src, W, H)
    rel = np.abs(_blocks(got.astype(np.float64), W, H) - _blocks(want, W, H)).max(1) / np.maximum(np.abs(_blocks(want, W, H)).max(1), 1e-30)
    assert rel.max() < 1e-5, float(rel.max())
    R.check_planes("fwd_f32", [src], [got], [None])


def check_inv_vs_double(kind, src, got, W, H, lut, by0=0, by1=None, level_shift=True):
    """an inverse or round trip against the float64 IDCT (tests/idct_reference.py) on the block rows computed: kind 'inv_i16' / 'inv_u8' /
    'rt_i16' / 'rt_u8' equal to the exact rule wherever the tie window decides the output, 'f32' within the window.  A round trip's
    block whose forward value sits within the forward window of a .5 tie is left out (full-scale int16 samples under a table of 8 leave
    out most blocks: tests/test_idct_accuracy.py holds the round trips to the rule on inputs where few are)"""
    by1 = H // 8 if by1 is None else by1
    rows = slice(by0 * 8, by1 * 8)
    R.check_planes(kind, [np.asarray(src)[rows]], [np.asarray(got)[rows]], [lut], level_shift=level_shift, max_skip=1.0)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def full(shape, value, dtype):
    import torch
    return torch.full(shape, value, dtype=dtype, device="cuda")


# ---- the reference's uint8 products through the drop-in API (device pointers; processed block rows = ceil(endY/16)...)
CANARY = 0xA5
BEH = {  # behaviour -> (drop-in function, --max-simd level)
    "q32_avx": ("simdDCT_EncodeQuantize32ReorderBuffer", M.SIMD_AVX2),
    "stereo_sse": ("simdDCT_EncodeQuantizeReorderStereoBuffer", M.SIMD_AVX2),
    "encq_sse": ("simdDCT_EncodeQuantizeBuffer", M.SIMD_AVX2),
    "stereo_scalar": ("simdDCT_EncodeQuantizeReorderStereoBuffer", 0),
    "encq_scalar": ("simdDCT_EncodeQuantizeBuffer", 0),
}


def _dropin(beh, W, H, y0, y1, lut, k=0):
    def run():
        import torch
        img = u8_full(W, H, k)
        img[:8] = 0  # a block row of zeros: 0 * inf = NaN through the extreme tables
        fn, level = BEH[beh]
        M.set_max_simd(level)
        try:
            out = full((W * H,), CANARY, torch.uint8)
            rc = getattr(M, fn)(dev(img.reshape(-1)), out, lut, W, H, y0, y1)
        finally:
            M.set_max_simd(M.SIMD_AVX2)

        def check():
            want = np.full(W * H, CANARY, dtype=np.uint8)
            rc2, want = O.run_behaviour(beh, img, lut, W, H, y0, y1, out=want)
            assert rc == rc2 == 0, M.last_error()
            got = out.cpu().numpy()
            assert np.array_equal(got, want), int((got != want).sum())
        return check
    return run


NORMAL = {"q32_avx": 100.0, "stereo_sse": 1.0, "encq_sse": 1.0, "stereo_scalar": 1.0, "encq_scalar": 1.0}
for beh, (prof, lay) in {"stereo_sse": (1, 1), "encq_sse": (1, 3), "stereo_scalar": (2, 1), "encq_scalar": (2, 2)}.items():
    # linear form: 64 wide (16 blocks per launch row, partial last wave); TILED: a block row of whole 256-block workgroups, 2048 wide
    case(f"k_fwd_quant_u8<{prof}, {lay}, false, false>", "drop-in", f"{beh} 64x32")(_dropin(beh, 64, 32, 0, 32, (M.QUANTIZE_BASE * np.float32(NORMAL[beh])).astype(np.float32)))
    case(f"k_fwd_quant_u8<{prof}, {lay}, false, true>", "drop-in", f"{beh} 2048x64 rows 16..32")(_dropin(beh, 2048, 64, 16, 32, (M.QUANTIZE_BASE * np.float32(NORMAL[beh])).astype(np.float32)))
    if prof == 1:  # the SSE tiers' SAFE form: cvtps_epi32's integer-indefinite result, exactly
        case(f"k_fwd_quant_u8<{prof}, {lay}, true, false>", "drop-in", f"{beh} 64x32 extreme table")(_dropin(beh, 64, 32, 0, 32, lut_extreme()))
        case(f"k_fwd_quant_u8<{prof}, {lay}, true, true>", "drop-in", f"{beh} 2048x64 extreme table")(_dropin(beh, 2048, 64, 0, 64, lut_extreme()))
Q = (M.QUANTIZE_BASE * np.float32(100.0)).astype(np.float32)
case("k_q32_tile", "drop-in", "q32 512x64 rows 16..32")(_dropin("q32_avx", 512, 64, 16, 32, Q))
case("k_q32_avx<false, false>", "drop-in", "q32 256x64 (128 blocks, 32 per row)")(_dropin("q32_avx", 256, 64, 0, 64, Q))
case("k_q32_avx<false, true>", "drop-in", "q32 64x32 (16 blocks)")(_dropin("q32_avx", 64, 32, 0, 32, Q))
case("k_q32_avx<true, true>", "drop-in", "q32 64x32 extreme table")(_dropin("q32_avx", 64, 32, 0, 32, lut_extreme()))
case("k_q32_avx<true, false>", "drop-in", "q32 512x32 extreme table (128 blocks)")(_dropin("q32_avx", 512, 32, 0, 32, lut_extreme()))


# ---- engine-own int16 planes, native C-ABI: tile form (width % 512), SMALL tile form (2049..6144 tiles), linear form
I16_FN = {0: M.fwd_i16, 1: M.inv_i16, 2: M.roundtrip_i16}
I16_MODE = {0: "fwd", 1: "inv", 2: "roundtrip"}


def _i16_native(mode, W, H, lut, by0, by1, src_kind):
    def run():
        import torch
        src = i16_worst(W, H) if src_kind == "worst" else i16_full(W, H, mode)
        out = full((H, W), 77, torch.int16)
        I16_FN[mode](dev(src), out, W, H, lut=lut, by0=by0, by1=by1)

        def check():
            want = np.full((H, W), 77, dtype=np.int16)
            O.i16(I16_MODE[mode], src, W, H, lut=lut, by0=by0, by1=by1, out=want)
            got = out.cpu().numpy()
            assert np.array_equal(got, want), int((got != want).sum())
            if mode == 0:
                check_i16_fwd_vs_double(src, got, W, H, lut, by0, by1)
            else:
                check_inv_vs_double("inv_i16" if mode == 1 else "rt_i16", src, got, W, H, lut, by0, by1)
        return check
    return run


B8 = np.full(64, 8.0, dtype=np.float32)        # keeps the saturations (|coef| / 8 can leave int16)
B801 = np.full(64, 8.01, dtype=np.float32)     # bounded: the round trip drops them
for mode in (0, 1, 2):
    for has_lut in (False, True):
        lut = B8 if has_lut else None
        kind = "worst" if mode != 1 else "full"
        case(f"k_i16_tile<{mode}, {str(has_lut).lower()}, true, 2>", "native", f"{I16_MODE[mode]} 512x40 rows 1..4")(_i16_native(mode, 512, 40, lut, 1, 4, kind))
        case(f"k_i16_tile<{mode}, {str(has_lut).lower()}, true, 4>", "native", f"{I16_MODE[mode]} 4096x2400 (2400 tiles)")(_i16_native(mode, 4096, 2400, lut, 0, 300, kind))
        case(f"k_i16<{mode}, {str(has_lut).lower()}, true>", "native", f"{I16_MODE[mode]} 200x40 rows 1..4")(_i16_native(mode, 200, 40, lut, 1, 4, kind))
case("k_i16_tile<2, true, false, 2>", "native", "roundtrip 512x40 table 8.01 rows 1..4")(_i16_native(2, 512, 40, B801, 1, 4, "worst"))
case("k_i16_tile<2, true, false, 4>", "native", "roundtrip 4096x2400 table 8.01")(_i16_native(2, 4096, 2400, B801, 0, 300, "worst"))
case("k_i16<2, true, false>", "native", "roundtrip 200x40 table 8.01 rows 1..4")(_i16_native(2, 200, 40, B801, 1, 4, "worst"))


def _park():
    run0 = _i16_native(0, 200, 24, None, 0, 3, "full")

    def run():
        lut = lut_random(k=int(rng(7).integers(1 << 30)))  # content the table cache has not seen: an upload, then a launch that reads it
        inner = _i16_native(0, 200, 24, lut, 0, 3, "full")
        return inner()
    del run0
    return run


case(("k_park_table", "k_i16<0, true, true>"), "native", "fwd 200x24, a table the cache has not seen")(_park())


# ---- int16 plane batches (mdct_*_i16_batch): total tiles in (2048, 6144] take the SMALL build
def _i16_batch(mode, planes_spec):
    """planes_spec: list of (W, H, lut, kind)"""
    def run():
        import torch
        planes, keep = [], []
        for j, (W, H, lut, kind) in enumerate(planes_spec):
            src = i16_worst(W, H) if kind == "worst" else i16_full(W, H, 10 + j)
            out = full((H, W), 77, torch.int16)
            planes.append((dev(src), out, W, H, lut))
            keep.append((src, out, W, H, lut))
        M.i16_batch(I16_MODE[mode], planes)

        def check():
            for src, out, W, H, lut in keep:
                got = out.cpu().numpy()
                assert np.array_equal(got, O.i16(I16_MODE[mode], src, W, H, lut=lut)), (W, H)
                if mode == 0:
                    check_i16_fwd_vs_double(src, got, W, H, lut)
                else:
                    check_inv_vs_double("inv_i16" if mode == 1 else "rt_i16", src, got, W, H, lut)
        return check
    return run


MIXED = [(512, 8, None, "worst"), (200, 24, None, "full"), (1024, 32, None, "full")]
BIG = [(4096, 2400, None, "worst")]


def _with(spec, lut):
    return [(W, H, lut if l is None else l, k) for (W, H, l, k) in spec]


for small in (False, True):
    sp = BIG if small else MIXED
    sm = str(small).lower()
    tag = "4096x2400" if small else "512x8 + 200x24 + 1024x32"
    case(f"k_i16_batch<0, 1, true, {sm}>", "batch", f"fwd {tag}, tables")(_i16_batch(0, _with(sp, B8)))
    case(f"k_i16_batch<1, 1, true, {sm}>", "batch", f"inv {tag}, tables")(_i16_batch(1, _with(sp, B8)))
    case(f"k_i16_batch<2, 0, true, {sm}>", "batch", f"roundtrip {tag}, no tables")(_i16_batch(2, sp))
    case(f"k_i16_batch<2, 1, false, {sm}>", "batch", f"roundtrip {tag}, bounded tables 8.01")(_i16_batch(2, _with(sp, B801)))
    case(f"k_i16_batch<2, 1, true, {sm}>", "batch", f"roundtrip {tag}, tables 8.0")(_i16_batch(2, _with(sp, B8)))
    mixed = [(W, H, (B8 if j % 2 == 0 else None), k) for j, (W, H, _, k) in enumerate(sp + ([(200, 24, None, "full")] if small else []))]
    case(f"k_i16_batch<2, 2, true, {sm}>", "batch", f"roundtrip {tag}, some planes with a table")(_i16_batch(2, mixed))


# ---- 8-bit plane batches: round trip (mode 0), pixels -> coefficients (1), coefficients -> pixels (2)
TAME = (M.QUANTIZE_BASE * np.float32(16.0)).astype(np.float32)
WILD = TAME.copy()
WILD[5] = 0.01  # below 1/16: the GENERAL build (saturations kept)
U8_MIXED = [(512, 8), (200, 24), (1024, 32)]
U8_BIG = [(4096, 2400)]


def _u8_batch(mode, shapes, lut):
    def run():
        import torch
        keep, planes = [], []
        for j, (W, H) in enumerate(shapes):
            if mode == 2:
                coef = O.u8_i16("fwd", u8_full(W, H, 20 + j), W, H, lut=lut)
                coef[:8, :8] = 32767  # a block that leaves the pixel range: the saturating output
                src, out = coef, full((H, W), 0x5A, torch.uint8)
                planes.append((out, dev(src), W, H, lut))
            else:
                src = u8_full(W, H, 20 + j)
                out = full((H, W), 0x5A, torch.uint8) if mode == 0 else full((H, W), 77, torch.int16)
                planes.append((dev(src), out, W, H, lut))
            keep.append((src, out, W, H))
        if mode == 0:
            M.roundtrip_u8_batch(planes)
        else:
            M.u8_i16_batch("fwd" if mode == 1 else "inv", planes)

        def check():
            for src, out, W, H in keep:
                got = out.cpu().numpy()
                want = O.roundtrip_u8(src, W, H, lut=lut) if mode == 0 else O.u8_i16("fwd" if mode == 1 else "inv", src, W, H, lut=lut)
                assert np.array_equal(got, want), (W, H, int((got != want).sum()))
                if mode == 1:
                    check_i16_fwd_vs_double(src, got, W, H, lut, u8_shift=128)
                else:
                    check_inv_vs_double("inv_u8" if mode == 2 else "rt_u8", src, got, W, H, lut)
        return check
    return run


for small in (False, True):
    shapes, sm = (U8_BIG, "true") if small else (U8_MIXED, "false")
    tag = "4096x2400" if small else "512x8 + 200x24 + 1024x32"
    case(f"k_u8_batch<0, false, {sm}>", "u8 batch", f"roundtrip {tag}")(_u8_batch(0, shapes, TAME))
    case(f"k_u8_batch<0, true, {sm}>", "u8 batch", f"roundtrip {tag}, an entry below 1/16")(_u8_batch(0, shapes, WILD))
    case(f"k_u8_batch<1, false, {sm}>", "u8 batch", f"fwd {tag}")(_u8_batch(1, shapes, TAME))
    case(f"k_u8_batch<1, true, {sm}>", "u8 batch", f"fwd {tag}, an entry below 1/16")(_u8_batch(1, shapes, WILD))
    case(f"k_u8_batch<2, true, {sm}>", "u8 batch", f"inv {tag}")(_u8_batch(2, shapes, TAME))


def _q32_batch(lut):
    def run():
        import torch
        shapes = [(512, 8), (64, 24), (1024, 32)]
        keep, planes = [], []
        for j, (W, H) in enumerate(shapes):
            img = u8_full(W, H, 30 + j)
            out = full((W * H,), CANARY, torch.uint8)
            planes.append((dev(img), out, W, H, lut))
            keep.append((img, out, W, H))
        M.fwd_quant32_u8_batch(planes)

        def check():
            for img, out, W, H in keep:
                want = np.full(W * H, CANARY, dtype=np.uint8)
                O.q32_native(img, lut, W, H, 0, H // 8, out=want)
                assert np.array_equal(out.cpu().numpy(), want), (W, H)
        return check
    return run


case("k_q32_batch<false>", "q32 batch", "512x8 + 64x24 + 1024x32")(_q32_batch(Q))
case("k_q32_batch<true>", "q32 batch", "512x8 + 64x24 + 1024x32, extreme table")(_q32_batch(lut_extreme()))


# ---- float32
def _f32(mode, W, H, by0, by1):
    def run():
        import torch
        src = (rng(40).standard_normal((H, W)) * 300).astype(np.float32)
        out = full((H, W), 3.25, torch.float32)
        (M.fwd_f32 if mode == 0 else M.inv_f32)(dev(src), out, W, H, by0=by0, by1=by1)

        def check():
            got = out.cpu().numpy()
            want = np.full((H, W), 3.25, dtype=np.float32)
            want[by0 * 8:by1 * 8] = O.f32("fwd" if mode == 0 else "inv", src, W, H)[by0 * 8:by1 * 8]
            assert np.array_equal(got, want)
            if mode == 0:
                check_f32_vs_double(src[by0 * 8:by1 * 8], got[by0 * 8:by1 * 8], W, (by1 - by0) * 8)
            else:
                check_inv_vs_double("f32", src, got, W, H, None, by0, by1)
        return check
    return run


def _f32_wide(mode):
    """512 x 524288 (65536 block rows > the 2-D grid's 65535): the wide linear form.  The input repeats every 64 block rows, so the
    output must too: one period against the checker and the double definition, every other period against the first on the device."""
    W, period, H = 512, 512, 524288

    def run():
        import torch
        src = (rng(41 + mode).standard_normal((period, W)) * 300).astype(np.float32)
        d = dev(src).repeat(H // period, 1)
        out = torch.empty_like(d)
        (M.fwd_f32 if mode == 0 else M.inv_f32)(d, out, W, H)
        del d

        def check():
            first = out[:period]
            same = bool((out.view(H // period, period, W) == first.unsqueeze(0)).all().item())
            got = first.cpu().numpy()
            assert np.array_equal(got, O.f32("fwd" if mode == 0 else "inv", src, W, period))
            assert same, "a period of the output differs from the first"
            if mode == 0:
                check_f32_vs_double(src, got, W, period)
            else:
                check_inv_vs_double("f32", src, got, W, period, None)
        return check
    return run


for mode in (0, 1):
    case(f"k_f32_tile<{mode}>", "f32", f"{('fwd', 'inv')[mode]} 1024x40 rows 1..4")(_f32(mode, 1024, 40, 1, 4))
    case(f"k_f32<{mode}, false>", "f32", f"{('fwd', 'inv')[mode]} 200x40 rows 1..4")(_f32(mode, 200, 40, 1, 4))
    case(f"k_f32<{mode}, true>", "f32", f"{('fwd', 'inv')[mode]} 512x524288")(_f32_wide(mode))


# ---- pixels -> coefficients, single plane
def _u8_i16(W, H, lut):
    def run():
        import torch
        img = u8_full(W, H, 50)
        out = full((H, W), 77, torch.int16)
        M.fwd_u8_i16(dev(img), out, W, H, lut=lut)

        def check():
            got = out.cpu().numpy()
            assert np.array_equal(got, O.u8_i16("fwd", img, W, H, lut=lut))
            check_i16_fwd_vs_double(img, got, W, H, lut, u8_shift=128)
        return check
    return run


case("k_u8_i16_fwd", "native", "fwd 200x40, a table with an entry below 1/16")(_u8_i16(200, 40, WILD))


def _copy():
    nbytes = 16 * (256 * 8 * 3 + 5)  # three whole workgroups and a guarded tail of 5 lanes

    def run():
        import torch
        src = torch.from_numpy(u8_full(nbytes + 64, 1, 60).reshape(-1)).cuda()
        dst = full((nbytes + 64,), 0x5A, torch.uint8)
        M.stream_copy(src, dst, nbytes)

        def check():
            s, g = src.cpu().numpy(), dst.cpu().numpy()
            assert np.array_equal(g[:nbytes], s[:nbytes]) and (g[nbytes:] == 0x5A).all()
        return check
    return run


case("k_stream_copy", "native", "16 * 6149 bytes")(_copy())


# ---- stages: zig-zag scan + run/level records, Huffman rows, packing, 4:2:0 split, fused pixels -> Huffman rows / scan
SCAN_SRC = {0: "i16", 1: "q32", 2: "stereo", 3: "block"}


def _scan(src_id, rle, W=128, H=48):
    def run():
        import torch
        nblk = (W // 8) * (H // 8)
        if src_id == 0:
            coef = (rng(70).integers(-300, 300, (H, W)) * (rng(71).random((H, W)) < 0.2)).astype(np.int16)
        else:
            coef = u8_full(W, H, 72).reshape(-1)
        lv = full((nblk, 64), 0x3C3C, torch.int16)
        rn = full((nblk, 64), 0x3C, torch.uint8) if rle else None
        ct = full((nblk,), 0x3C, torch.uint8) if rle else None
        if src_id == 0:
            api.zigzag_rle_i16(dev(coef), W, H, lv, rn, ct)
        elif src_id == 1:
            api.zigzag_rle_q32(dev(coef), W, H, lv, rn, ct)
        else:
            api.zigzag_rle_u8(dev(coef), api.LAYOUT_STEREO if src_id == 2 else api.LAYOUT_BLOCK, W, H, lv, rn, ct)

        def check():
            wl, wr, wc = O.zigzag_rle(SCAN_SRC[src_id], coef, W, H, rle=rle, fill=0x3C3C)
            assert np.array_equal(lv.cpu().numpy(), wl)
            if rle:
                assert np.array_equal(rn.cpu().numpy(), wr) and np.array_equal(ct.cpu().numpy(), wc)
        return check
    return run


for src_id in range(4):
    for rle in (True, False):
        case(f"k_scan<{src_id}, {str(rle).lower()}>", "stage", f"{SCAN_SRC[src_id]} 128x48{'' if rle else ', levels only'}")(_scan(src_id, rle))

K1 = synth.JPEG_LUMA
K2 = synth.JPEG_CHROMA


def _records(i16_in, lut, W=264, H=24):
    def run():
        import torch
        nblk = (W // 8) * (H // 8)
        src = i16_full(W, H, 80) // 16 if i16_in else u8_full(W, H, 80)
        lv, rn, ct = full((nblk, 64), 0x3C3C, torch.int16), full((nblk, 64), 0x3C, torch.uint8), full((nblk,), 0x3C, torch.uint8)
        (api.fwd_i16_records if i16_in else api.fwd_u8_records)(dev(src), W, H, lv, rn, ct, lut=lut)

        def check():
            coef = O.i16("fwd", src, W, H, lut=lut) if i16_in else O.u8_i16("fwd", src, W, H, lut=lut)
            wl, wr, wc = O.zigzag_rle("i16", coef, W, H)
            c = ct.cpu().numpy()
            assert np.array_equal(c, wc)
            gl, gr = lv.cpu().numpy(), rn.cpu().numpy()
            for b in range(nblk):  # the pairs a block holds; the rest of its row is scratch
                assert np.array_equal(gl[b, :c[b]], wl[b, :c[b]]) and np.array_equal(gr[b, :c[b]], wr[b, :c[b]]), b
        return check
    return run


case("k_u8_records<false, true>", "stage", "u8 264x24, a table entry below 1/16")(_records(False, WILD))
case("k_u8_records<false, false>", "stage", "u8 264x24, Annex K luma")(_records(False, K1))
case("k_u8_records<true, true>", "stage", "int16 264x24, Annex K chroma")(_records(True, K2))


def _huff_rows(W=264, H=24):
    def run():
        import torch
        img = u8_full(W, H, 90)
        lvh, rnh, cth = O.u8_records(img, W, H, lut=K1)
        stride = api.huffman_seg_stride(W)
        seg = full(((H // 8) * stride,), 0x5A, torch.uint8)
        nb = full((H // 8,), -1, torch.int32)
        api.huffman_rows(dev(lvh), dev(rnh), dev(cth), W, H, seg, nb, by0=1, by1=3)

        def check():
            ws, wn, _ = O.huffman_rows(lvh, rnh, cth, W, H, by0=1, by1=3, fill=0x5A)
            gn = nb.cpu().numpy()
            assert np.array_equal(gn[1:3].astype(np.uint32), wn[1:3]) and gn[0] == -1
            gs = seg.cpu().numpy()
            assert (gs[:stride] == 0x5A).all()
            for r in (1, 2):
                assert np.array_equal(gs[r * stride:r * stride + wn[r]], ws[r * stride:r * stride + wn[r]]), r
        return check
    return run


case("k_huffman_rows", "stage", "264x24 rows 1..3")(_huff_rows())


def _segments(W, H, k):
    img = u8_full(W, H, k)
    lvh, rnh, cth = O.u8_records(img, W, H, lut=np.ones(64, dtype=np.float32))
    seg, nb, stride = O.huffman_rows(lvh, rnh, cth, W, H)
    return seg, nb, stride


def _pack(counted):
    def run():
        import torch
        W, H = 264, 40
        seg, nb, stride = _segments(W, H, 95)
        n = H // 8
        ff = np.array([int((seg[r * stride:r * stride + nb[r]] == 0xFF).sum()) for r in range(n)], dtype=np.int32)
        want, woff = O.jpeg_pack_rows(seg, nb, stride, first_rst=5)
        total = int(woff[-1])
        out = full((total + 32,), 0x33, torch.uint8)
        off = full((n + 1,), -7, torch.int64)
        api.jpeg_pack_rows(dev(seg), dev(nb.astype(np.int32)), stride, n, out, off, first_rst=5, out_capacity=total, ff_counts=dev(ff) if counted else None)

        def check():
            assert np.array_equal(off.cpu().numpy(), woff.astype(np.int64))
            g = out.cpu().numpy()
            assert np.array_equal(g[:total], want[:total]) and (g[total:] == 0x33).all()
        return check
    return run


case("k_pack_write<true>", "stage", "264x40, counted rows")(_pack(True))
case(("k_pack_count", "k_pack_scan", "k_pack_write<false>"), "stage", "264x40, uncounted rows")(_pack(False))


def _split(planes8):
    def run():
        import torch
        W, H = 48, 32
        ycc = u8_full(3 * W, H, 99)
        dt = torch.uint8 if planes8 else torch.int16
        y, cb, cr = full((H, W), 77, dt), full((H // 2, W // 2), 77, dt), full((H // 2, W // 2), 77, dt)
        (api.split420_u8_planes if planes8 else api.split420_u8)(dev(ycc), W, H, y, cb, cr)

        def check():
            for g, w in zip((y, cb, cr), O.split420(ycc, W, H)):
                w = (w.astype(np.int32) + 128).astype(np.uint8) if planes8 else w
                assert np.array_equal(g.cpu().numpy(), w)
        return check
    return run


case("k_split420<false>", "stage", "48x32 -> int16 planes")(_split(False))
case("k_split420<true>", "stage", "48x32 -> 8-bit planes")(_split(True))


def _px_huff(i16_in, pack, lut, W=264, H=24):
    def run():
        import torch
        src = i16_full(W, H, 110) // 16 if i16_in else u8_full(W, H, 110)
        n = H // 8
        stride = api.huffman_seg_stride(W)
        coef = O.i16("fwd", src, W, H, lut=lut) if i16_in else O.u8_i16("fwd", src, W, H, lut=lut)
        lvh, rnh, cth = O.zigzag_rle("i16", coef, W, H)
        ws, wn, _ = O.huffman_rows(lvh, rnh, cth, W, H)
        if not pack:
            seg = full((n * stride + 64,), 0x5A, torch.uint8)
            nb = full((n,), -1, torch.int32)
            (api.fwd_i16_huffman_rows if i16_in else api.fwd_u8_huffman_rows)(dev(src), W, H, seg, nb, lut=lut)

            def check():
                assert np.array_equal(nb.cpu().numpy().astype(np.uint32), wn)
                g = seg.cpu().numpy()
                for r in range(n):
                    assert np.array_equal(g[r * stride:r * stride + wn[r]], ws[r * stride:r * stride + wn[r]]), r
                assert (g[n * stride:] == 0x5A).all()
            return check
        want, woff = O.jpeg_pack_rows(ws, wn, stride, first_rst=2)
        total = int(woff[-1])
        seg_w = torch.empty((n * stride,), dtype=torch.uint8, device="cuda")
        work = torch.zeros((n + 2,), dtype=torch.int64, device="cuda")
        out = full((total + 32,), 0x33, torch.uint8)
        off = full((n + 1,), -7, torch.int64)
        (api.fwd_i16_jpeg_scan if i16_in else api.fwd_u8_jpeg_scan)(dev(src), W, H, seg_w, work, out, off, lut=lut, first_rst=2, out_capacity=total)

        def check():
            assert np.array_equal(off.cpu().numpy(), woff.astype(np.int64))
            g = out.cpu().numpy()
            assert np.array_equal(g[:total], want[:total]) and (g[total:] == 0x33).all()
        return check
    return run


for pack in (False, True):
    p = str(pack).lower()
    what = "scan" if pack else "rows"
    case(f"k_px_huffman_rows<false, 4, {p}, true>", "stage", f"u8 264x24 -> {what}, a table entry below 1.01")(_px_huff(False, pack, np.where(np.arange(64) == 9, 1.0, K1).astype(np.float32)))
    case(f"k_px_huffman_rows<false, 4, {p}, false>", "stage", f"u8 264x24 -> {what}, Annex K luma")(_px_huff(False, pack, K1))
    case(f"k_px_huffman_rows<true, 4, {p}, true>", "stage", f"int16 264x24 -> {what}, Annex K chroma")(_px_huff(True, pack, K2))


MATRIX_KERNELS = {k for ks, _, _, _ in MATRIX for k in ks}


# ------------------------------------------------------------------------------------------ CPU
def test_matrix_rows_are_unique():
    ids = [(ks, desc) for ks, _, desc, _ in MATRIX]
    assert len(ids) == len(set(ids))
    assert not set(ALLOWLIST) & MATRIX_KERNELS


def test_code_object_kernels_equal_the_matrix():
    """every kernel in the gfx950 code objects has a case (or an allowlist reason), and every case names a kernel that exists"""
    if not os.path.exists(LIB):
        pytest.fail("libmdct_hip.so is not built (python -c 'import __graft_entry__ as g; g.build()')")
    names, n_objects = code_object_kernels()
    assert n_objects >= 2, "expected the code objects of mdct_kernels.hip and stages.hip"
    missing = sorted(names - MATRIX_KERNELS - set(ALLOWLIST))
    stale = sorted((MATRIX_KERNELS | set(ALLOWLIST)) - names)
    assert not missing, f"instantiations in the code object without a coverage case: {missing}"
    assert not stale, f"coverage cases / allowlist entries for kernels the code object does not hold: {stale}"


def test_kernel_name_form():
    assert _kernel_name("void mdct::k_fwd_quant_u8<1, 3, true, true>(mdct::U8Args)") == "k_fwd_quant_u8<1, 3, true, true>"
    assert _kernel_name("mdct::k_stream_copy(unsigned int vector[4] const*, unsigned int vector[4]*, unsigned long)") == "k_stream_copy"


# ------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    torch.cuda.set_device(0)
    M.init(0)
    yield torch
    M.set_max_simd(M.SIMD_AVX2)


@pytest.mark.gpu
@pytest.mark.parametrize("kernels,call,desc,run", MATRIX, ids=[f"{'+'.join(ks)}|{desc}" for ks, _, desc, _ in MATRIX])
def test_instantiation_runs_and_matches(gpu, kernels, call, desc, run):
    torch = gpu
    torch.cuda.synchronize()
    M.kernel_counts_reset()
    check = run()
    torch.cuda.synchronize()
    counts = M.kernel_counts()
    ran = set(counts)
    if "k_park_table" not in kernels:
        ran.discard("k_park_table")  # a table's first sight uploads it; whether this process saw it before is not the case's business
    assert ran == set(kernels), f"{call} {desc}: expected {sorted(kernels)}, the tally shows {sorted(counts.items())}"
    check()
