"""Every inverse DCT path held to the mathematical IDCT (tests/idct_reference.py: float64, from the cosine definition), not to the
checker it is kept in lock-step with.

The rule: an int16 or 8-bit output must equal the exact rule (sat_i16(rne(IDCT(c * Q))) / clamp(rne(IDCT(c * Q) + 128), 0, 255))
wherever every value within the tie window of the exact one rounds and saturates alike; a float32 output must lie within the window.
The window is TIE_K * 2^-24 * sum|c * Q| / 8 per block ("Inverse accuracy").

CPU: the checker's orc_inv_f32, orc_inv_i16 (with and without a table), orc_inv_i16_u8 (level shift x table), orc_idct8_own and the
round trips with a table, each through the IEEE 1180-1990 procedure (six ranges x signs, 10,000 blocks, five limits, zero in -> zero
out) and against the exact rule on adversarial blocks.
GPU: every inverse instantiation (k_i16_tile / k_i16 / k_i16_batch modes 1 and 2, k_u8_batch modes 0 and 2, k_f32_tile<1>, k_f32<1, ..>)
fed the IEEE 1180 blocks and the adversarial blocks at its tile, linear, SMALL and batch shapes, the launch tally naming the
instantiation; and decode_jpeg's pixels of files encoded from known coefficients, against T.81's rule."""
import ctypes

import numpy as np
import pytest

import idct_reference as R
import oracle as O

RNG_SEED = 1180


def rng(k=0):
    return np.random.default_rng(RNG_SEED + k)


def _ieee_blocks():
    """{case: (pixels, coefficients, reference output)} for the six IEEE 1180 cases"""
    out = {}
    for L, H, sign in R.IEEE1180_CASES:
        px = R.ieee1180_pixels(L, H, sign)
        coef = R.ieee1180_coefficients(px)
        out[(L, H, sign)] = (px, coef, R.ieee1180_reference(coef))
    return out


_IEEE = None


def ieee():
    global _IEEE
    if _IEEE is None:
        _IEEE = _ieee_blocks()
    return _IEEE


def table_random(k, lo=1, hi=255):
    return rng(200 + k).integers(lo, hi + 1, 64).astype(np.float32)


TABLES = {  # name -> 64 entries or None (no table)
    "none": None,
    "ones": np.ones(64, dtype=np.float32),
    "random": table_random(0, 1, 40),
    "random-255": table_random(1, 1, 255),
    "all-255": np.full(64, 255.0, dtype=np.float32),
}


# ------------------------------------------------------------------------------------------ the checker, block lists in and out
def _side(n):
    """a plane of at least n blocks: (W, H) with 100 blocks per row"""
    return 800, 8 * -(-n // 100)


def _to_plane(blks, dtype):
    W, H = _side(len(blks))
    return R.plane(R.tile_blocks(blks, (W // 8) * (H // 8)), W, H).astype(dtype), W, H


def orc_inv_i16(c, q=None):
    src, W, H = _to_plane(c, np.int16)
    return R.blocks(O.i16("inv", src, W, H, lut=q))[:len(c)]


def orc_inv_u8(c, q=None, level_shift=True):
    src, W, H = _to_plane(c, np.int16)
    lp = None
    if q is not None:
        keep, lp = O._lut(q)
    out = np.zeros((H, W), dtype=np.uint8)
    assert O.oracle().orc_inv_i16_u8(src.ctypes.data, out.ctypes.data, W, W, lp, int(level_shift), W, H, 0, H // 8) == 0
    return R.blocks(out)[:len(c)]


def orc_inv_f32(z):
    src, W, H = _to_plane(z, np.float32)
    return R.blocks(O.f32("inv", src, W, H))[:len(z)]


def orc_idct_own(z):
    """the checker's 1-D inverse, down the columns then along the rows of each block"""
    b = np.array(z, dtype=np.float32).reshape(-1, 64)  # a copy: transformed in place
    fn, base = O.oracle().orc_idct8_own, b.ctypes.data
    for k in range(len(b)):
        for c in range(8):
            fn(ctypes.c_void_p(base + (k * 64 + c) * 4), 8)
        for r in range(8):
            fn(ctypes.c_void_p(base + (k * 64 + r * 8) * 4), 1)
    return b.reshape(-1, 8, 8)


def orc_roundtrip(x, q, out="i16", level_shift=True):
    if out == "i16":
        src, W, H = _to_plane(x, np.int16)
        return R.blocks(O.i16("roundtrip", src, W, H, lut=q))[:len(x)]
    src, W, H = _to_plane(x, np.uint8)
    return R.blocks(O.roundtrip_u8(src, W, H, lut=q, level_shift=level_shift))[:len(x)]


# ------------------------------------------------------------------------------------------ CPU: the reference itself
def test_reference_transform_is_orthonormal_and_matches_checker_double_dct():
    assert np.abs(R.C @ R.C.T - np.eye(8)).max() < 1e-15
    x = rng(1).integers(-300, 300, (50, 8, 8))
    assert np.abs(R.idct2(R.dct2(x)) - x).max() < 1e-10
    # the checker's own double-precision DCT-II (an independent restatement of the definition)
    W, H = 80, 40
    px = rng(2).integers(-256, 256, (H, W)).astype(np.float32)
    assert np.abs(R.blocks(O.f32("f64ref", px, W, H)) - R.dct2(R.blocks(px.astype(np.float64)))).max() < 1e-9
    # a DC-only block is flat at z / 8
    assert np.abs(R.idct2(R.impulse_blocks([8.0])[0]) - 1.0).max() < 1e-15


def test_reference_window_and_rules():
    z = np.zeros((1, 8, 8))
    z[0, 0, 0] = 8 * 2.5
    want, exact, tol = R.i16_samples(z)
    assert (want == 2).all() and np.abs(exact - 2.5).max() < 1e-12  # a tie rounds to even
    assert not R.decided(exact, tol, *R.I16_RANGE).any()           # ... and is never decided
    assert R.decided(exact + 0.25, tol, *R.I16_RANGE).all()
    big = np.full((1, 8, 8), 40000.0 * 8)
    assert R.decided(R.idct2(big), R.tie_window(big), *R.I16_RANGE).any()  # saturated beyond the window
    px, exact8, _ = R.u8_pixels(np.full((1, 8, 8), -4000, dtype=np.int16))
    assert px.min() == 0
    assert float(R.tie_window(np.ones((1, 8, 8)))[0, 0, 0]) == R.TIE_K * R.ULP * 8


def test_ieee1180_generator_and_reference():
    px = R.ieee1180_pixels(256, 255, 1)
    assert px.shape == (10000, 8, 8) and px.min() == -256 and px.max() == 255
    assert np.array_equal(R.ieee1180_pixels(5, 5, -1), -R.ieee1180_pixels(5, 5, 1))
    # the first three outputs of the standard's generator from randx = 1
    r, first = 1, []
    for _ in range(3):
        r = (r * 1103515245 + 12345) % (1 << 32)
        first.append(int((r & 0x7FFFFFFE) / 0x7FFFFFFF * 512) - 256)
    assert px.reshape(-1)[:3].tolist() == first
    coef = R.ieee1180_coefficients(px)
    assert coef.min() >= -2048 and coef.max() <= 2047
    # the reference passes its own procedure, and a float32 rendering of it does too
    ref = R.ieee1180_reference(coef)
    assert not R.ieee1180_failures(ref, ref)
    f32 = np.clip(np.floor(R.idct2(coef.astype(np.float32)).astype(np.float32) + 0.5), -256, 255)
    assert not R.ieee1180_failures(f32, ref)
    assert R.ieee1180_failures(ref + (rng(3).random(ref.shape) < 0.03), ref)  # a 3 % bias breaks the mean-error limits


# ------------------------------------------------------------------------------------------ CPU: IEEE 1180 on the checker
PATHS_1180 = ["inv_f32", "inv_i16", "inv_i16_table", "inv_u8_shift", "inv_u8_shift_table", "inv_u8", "inv_u8_table", "idct8_own"]


def _run_1180_path(path, coef):
    """-> the path's output on the coefficient blocks, as the standard's integer result clipped to [-256, 255] (8-bit outputs: minus
    their level shift), and the range the reference must be clipped to for the comparison"""
    ones = np.ones(64, dtype=np.float32)
    if path in ("inv_f32", "idct8_own"):
        y = orc_inv_f32(coef) if path == "inv_f32" else orc_idct_own(coef)
        return np.clip(np.floor(y.astype(np.float64) + 0.5), -256, 255), (-256, 255)
    if path.startswith("inv_i16"):
        return np.clip(orc_inv_i16(coef, ones if path.endswith("table") else None).astype(np.int64), -256, 255), (-256, 255)
    shift = 128 if "shift" in path else 0
    y = orc_inv_u8(coef, ones if path.endswith("table") else None, level_shift=bool(shift)).astype(np.int64) - shift
    return y, (-shift, 255 - shift)


@pytest.mark.parametrize("path", PATHS_1180)
@pytest.mark.parametrize("case", R.IEEE1180_CASES, ids=[f"{L}_{H}_{'+' if s > 0 else '-'}" for L, H, s in R.IEEE1180_CASES])
def test_ieee1180_checker(path, case):
    _, coef, ref = ieee()[case]
    got, (lo, hi) = _run_1180_path(path, coef)
    fails = R.ieee1180_failures(got, np.clip(ref, lo, hi))
    assert not fails, (path, case, fails, R.ieee1180_stats(got, np.clip(ref, lo, hi)))


@pytest.mark.parametrize("path", PATHS_1180)
def test_ieee1180_zero_in_zero_out(path):
    got, (lo, hi) = _run_1180_path(path, np.zeros((4, 8, 8), dtype=np.int64))
    assert (got == 0).all()


# ------------------------------------------------------------------------------------------ CPU: float32 within the window
def f32_blocks():
    r = rng(10)
    amps = np.concatenate([R.AMPS, [0.37, 12345.678]])
    b = [R.uniform_blocks(amps), R.worst_pixel_blocks(amps), R.impulse_blocks(amps)]
    b += [R.sparse_blocks(r, 200, a, k) for a in R.AMPS for k in (2, 3)]
    b += [r.standard_normal((2000, 8, 8)) * 300]
    b = np.concatenate(b)
    return np.concatenate([b, -b]).astype(np.float32)


@pytest.mark.parametrize("path", ["inv_f32", "idct8_own"])
def test_f32_inverse_within_window(path):
    z = f32_blocks()
    got = (orc_inv_f32(z) if path == "inv_f32" else orc_idct_own(z)).astype(np.float64)
    exact, tol = R.f32_samples(z)
    err = np.abs(got - exact)
    worst = float((err / tol).max())
    assert (err <= tol).all(), (path, worst * R.TIE_K, int((err > tol).sum()))


# ------------------------------------------------------------------------------------------ CPU: int16 and 8-bit outputs
def coef_blocks():
    """IEEE 1180 coefficient blocks (5000 of each case), the adversarial blocks, full-range random and saturating blocks"""
    r = rng(20)
    b = [coef[:5000] for _, coef, _ in ieee().values()]
    b += [R.adversarial_i16(r)]
    b += [r.integers(-32768, 32768, (500, 8, 8)), r.integers(-64, 64, (2000, 8, 8))]
    return np.concatenate([np.asarray(x, dtype=np.int64) for x in b]).astype(np.int16)


@pytest.mark.parametrize("table", list(TABLES))
def test_inv_i16_exact_outside_window(table):
    q = TABLES[table]
    c = coef_blocks()
    want, exact, tol = R.i16_samples(c, q)
    assert want.min() == -32768 and want.max() == 32767  # saturates at both ends
    R.assert_exact_rule(orc_inv_i16(c, q), want, exact, tol, R.I16_RANGE, f"orc_inv_i16 table {table}")


@pytest.mark.parametrize("level_shift", [True, False], ids=["shift", "noshift"])
@pytest.mark.parametrize("table", list(TABLES))
def test_inv_u8_exact_outside_window(table, level_shift):
    q = TABLES[table]
    c = coef_blocks()
    want, exact, tol = R.u8_pixels(c, q, level_shift)
    assert want.min() == 0 and want.max() == 255
    R.assert_exact_rule(orc_inv_u8(c, q, level_shift), want, exact, tol, R.U8_RANGE, f"orc_inv_i16_u8 table {table} shift {level_shift}")


def dc_only_blocks():
    """DC-only blocks: every value of c = 4 (mod 8) in [-32764, 32764] and a spread of others"""
    dc = np.concatenate([np.arange(-32764, 32765, 8), np.arange(-2000, 2001), [-32768, 32767]])
    b = np.zeros((dc.size, 8, 8), dtype=np.int16)
    b[:, 0, 0] = dc
    return b


@pytest.mark.parametrize("table", ["none", "ones", "random-255", "all-255"])
def test_dc_only_blocks_exact_without_window(table):
    """z / 8 (+ 128) is exact in float32 through every operation, so the output is the exact rule's everywhere, ties to even"""
    q = TABLES[table]
    c = dc_only_blocks()
    z00 = c[:, 0, 0].astype(np.float64) * (1.0 if q is None else float(q[0]))
    flat = np.broadcast_to((z00 / 8.0)[:, None, None], c.shape)
    want16 = np.clip(np.rint(flat), -32768, 32767)
    assert np.array_equal(R.i16_samples(c, q)[0], want16)
    assert np.array_equal(orc_inv_i16(c, q), want16), table
    for shift in (True, False):
        want8 = np.clip(np.rint(flat + (128.0 if shift else 0.0)), 0, 255)
        assert np.array_equal(orc_inv_u8(c, q, shift), want8), (table, shift)
    if q is None or q[0] == 1:  # c = 4 (mod 8): exactly half way, to even
        tie = c[:, 0, 0] % 8 == 4
        assert np.array_equal(want16[tie, 0, 0] % 2, np.zeros(int(tie.sum())))


# ------------------------------------------------------------------------------------------ CPU: round trips with a table
RT_TABLES = {"random-float": rng(30).uniform(1.0, 64.0, 64).astype(np.float32),
             "random-float-wide": rng(31).uniform(0.7, 255.0, 64).astype(np.float32)}


def rt_i16_blocks():
    r = rng(40)
    b = [px[:3000] for px, _, _ in ieee().values()]
    worst = np.where(R.worst_pixel_blocks([1.0]) > 0, 32767, -32768)  # coefficients that saturate the quantiser
    b += [r.integers(-500, 500, (3000, 8, 8)), worst, -1 - worst]
    return np.concatenate(b).astype(np.int16)


def rt_u8_blocks():
    r = rng(41)
    b = [np.clip(px[:3000] + 128, 0, 255) for px, _, _ in ieee().values()]
    b += [r.integers(0, 256, (6000, 8, 8)), np.where(R.worst_pixel_blocks([1.0]) > 0, 255, 0)]
    return np.concatenate(b).astype(np.uint8)


@pytest.mark.parametrize("table", list(RT_TABLES))
def test_roundtrip_i16_with_table_is_the_composition(table):
    q = RT_TABLES[table]
    x = rt_i16_blocks()
    want, exact, tol, skip = R.roundtrip(x, q, "i16")
    assert skip.mean() < 0.01, float(skip.mean())
    got = orc_roundtrip(x, q, "i16")
    R.assert_exact_rule(got[~skip], want[~skip], exact[~skip], tol[~skip], R.I16_RANGE, f"orc_roundtrip_i16 {table}")


@pytest.mark.parametrize("level_shift", [True, False], ids=["shift", "noshift"])
@pytest.mark.parametrize("table", list(RT_TABLES))
def test_roundtrip_u8_with_table_is_the_composition(table, level_shift):
    q = RT_TABLES[table]
    x = rt_u8_blocks()
    want, exact, tol, skip = R.roundtrip(x, q, "u8", level_shift)
    assert skip.mean() < 0.01, float(skip.mean())
    got = orc_roundtrip(x, q, "u8", level_shift)
    R.assert_exact_rule(got[~skip], want[~skip], exact[~skip], tol[~skip], R.U8_RANGE, f"orc_roundtrip_u8 {table} shift {level_shift}")


# ------------------------------------------------------------------------------------------ GPU: every inverse instantiation
@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    torch.cuda.set_device(0)
    import simd_dct_amd as M
    M.init(0)
    return torch, M


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def inv_blocks():
    """all 60,000 IEEE 1180 coefficient blocks, then the adversarial blocks"""
    return np.concatenate([coef for _, coef, _ in ieee().values()] + [R.adversarial_i16(rng(50)).astype(np.int64)]).astype(np.int16)


def rt_i16_gpu_blocks():
    r = rng(51)
    worst = np.where(R.worst_pixel_blocks([1.0]) > 0, 32767, -32768)
    return np.concatenate([px for px, _, _ in ieee().values()] + [worst, -1 - worst, r.integers(-500, 500, (2000, 8, 8))]).astype(np.int16)


def rt_u8_gpu_blocks():
    r = rng(52)
    ext = np.where(R.worst_pixel_blocks([1.0]) > 0, 255, 0)
    return np.concatenate([np.clip(px + 128, 0, 255) for px, _, _ in ieee().values()] + [ext, 255 - ext, r.integers(0, 256, (2000, 8, 8))]).astype(np.uint8)


def f32_gpu_blocks():
    return np.concatenate([coef.astype(np.float32) for _, coef, _ in ieee().values()] + [f32_blocks()])


def _planes_of(blks, shapes):
    """the block list cut into planes of the given (W, H), cycling when the planes hold more blocks"""
    n = sum((W // 8) * (H // 8) for W, H in shapes)
    allb = R.tile_blocks(blks, n)
    out, k = [], 0
    for W, H in shapes:
        m = (W // 8) * (H // 8)
        out.append(R.plane(allb[k:k + m], W, H))
        k += m
    return out


def _rows_for(n, W):
    return 8 * -(-n // (W // 8))


B8 = np.full(64, 8.0, dtype=np.float32)      # the round trip keeps its saturations
B801 = np.full(64, 8.01, dtype=np.float32)   # bounded: the round trip leaves them out
Q_RAND = TABLES["random-255"]
TAME = np.array(__import__("simd_dct_amd.jpeg_encode", fromlist=["quality_tables"]).quality_tables(50)[0], dtype=np.float32)
WILD = TAME.copy()
WILD[5] = 0.01  # below 1/16: the general 8-bit build
NONSMALL = [(512, 2000), (200, 2000), (1024, 3200)]  # about 1,300 tiles: the 2-waves-per-SIMD build
SMALL = [(4096, 2400)]                              # 2,400 tiles: the SMALL (4 waves per SIMD) build


GPU_CASES = []  # (kernels, description, run() -> check())


def gcase(kernels, desc):
    def reg(fn):
        GPU_CASES.append(((kernels,) if isinstance(kernels, str) else tuple(kernels), desc, fn))
        return fn
    return reg


def _i16_single(mode, shape, lut, blks_fn):
    def run(torch, M):
        (src,) = _planes_of(blks_fn(), [shape])
        out = torch.full(src.shape, 77, dtype=torch.int16, device="cuda")
        (M.inv_i16 if mode == "inv" else M.roundtrip_i16)(dev(src), out, shape[0], shape[1], lut=lut)
        return lambda: R.check_planes("inv_i16" if mode == "inv" else "rt_i16", [src], [out.cpu().numpy()], [lut])
    return run


def _tile_shape(n, small):
    return (4096, 2400) if small else (512, _rows_for(n, 512))


N_INV = 60000 + 2 * (11 + 2 * 704 + 11 * 64)
for small, w in ((False, 2), (True, 4)):
    for tname, lut in (("false", None), ("true", Q_RAND)):
        shp = _tile_shape(N_INV, small)
        gcase(f"k_i16_tile<1, {tname}, true, {w}>", f"inv {shp[0]}x{shp[1]}")(_i16_single("inv", shp, lut, inv_blocks))
    for tname, lut in (("false, true", None), ("true, true", B8), ("true, false", B801)):
        shp = _tile_shape(64000, small)
        gcase(f"k_i16_tile<2, {tname}, {w}>", f"roundtrip {shp[0]}x{shp[1]} table {None if lut is None else lut[0]}")(
            _i16_single("rt", shp, lut, rt_i16_gpu_blocks))
for tname, lut in (("false", None), ("true", Q_RAND)):
    gcase(f"k_i16<1, {tname}, true>", "inv 200 wide")(_i16_single("inv", (200, _rows_for(N_INV, 200)), lut, inv_blocks))
for tname, lut in (("false, true", None), ("true, true", B8), ("true, false", B801)):
    gcase(f"k_i16<2, {tname}>", f"roundtrip 200 wide table {None if lut is None else lut[0]}")(
        _i16_single("rt", (200, _rows_for(64000, 200)), lut, rt_i16_gpu_blocks))


def _i16_batch(mode, shapes, luts, blks_fn):
    def run(torch, M):
        srcs = _planes_of(blks_fn(), shapes)
        outs = [torch.full(s.shape, 77, dtype=torch.int16, device="cuda") for s in srcs]
        M.i16_batch(mode, [(dev(s), o, s.shape[1], s.shape[0], l) for s, o, l in zip(srcs, outs, luts)])
        return lambda: R.check_planes("inv_i16" if mode == "inv" else "rt_i16", srcs, [o.cpu().numpy() for o in outs], luts)
    return run


for sm, shapes in (("false", NONSMALL), ("true", SMALL)):
    n = len(shapes)
    gcase(f"k_i16_batch<1, 1, true, {sm}>", f"inv batch {shapes}")(_i16_batch("inv", shapes, [Q_RAND] * n, inv_blocks))
    gcase(f"k_i16_batch<2, 0, true, {sm}>", f"roundtrip batch {shapes}, no tables")(_i16_batch("roundtrip", shapes, [None] * n, rt_i16_gpu_blocks))
    gcase(f"k_i16_batch<2, 1, false, {sm}>", f"roundtrip batch {shapes}, tables 8.01")(_i16_batch("roundtrip", shapes, [B801] * n, rt_i16_gpu_blocks))
    gcase(f"k_i16_batch<2, 1, true, {sm}>", f"roundtrip batch {shapes}, tables 8")(_i16_batch("roundtrip", shapes, [B8] * n, rt_i16_gpu_blocks))
    mixed = shapes if n > 1 else shapes + [(200, 24)]
    gcase(f"k_i16_batch<2, 2, true, {sm}>", f"roundtrip batch {mixed}, some tables")(
        _i16_batch("roundtrip", mixed, [B8 if j % 2 == 0 else None for j in range(len(mixed))], rt_i16_gpu_blocks))


def _u8_inv(shapes, lut, level_shift, single):
    def run(torch, M):
        srcs = _planes_of(inv_blocks(), shapes)
        outs = [torch.full(s.shape, 0x5A, dtype=torch.uint8, device="cuda") for s in srcs]
        if single:
            M.inv_i16_u8(dev(srcs[0]), outs[0], shapes[0][0], shapes[0][1], lut=lut, level_shift=level_shift)
        else:
            M.u8_i16_batch("inv", [(o, dev(s), s.shape[1], s.shape[0], lut) for s, o in zip(srcs, outs)], level_shift=level_shift)
        return lambda: R.check_planes("inv_u8", srcs, [o.cpu().numpy() for o in outs], [lut] * len(srcs), level_shift)
    return run


def _u8_rt(shapes, lut, level_shift, single):
    def run(torch, M):
        srcs = _planes_of(rt_u8_gpu_blocks(), shapes)
        outs = [torch.full(s.shape, 0x5A, dtype=torch.uint8, device="cuda") for s in srcs]
        if single:
            M.roundtrip_u8(dev(srcs[0]), outs[0], shapes[0][0], shapes[0][1], lut=lut, level_shift=level_shift)
        else:
            M.roundtrip_u8_batch([(dev(s), o, s.shape[1], s.shape[0], lut) for s, o in zip(srcs, outs)], level_shift=level_shift)
        return lambda: R.check_planes("rt_u8", srcs, [o.cpu().numpy() for o in outs], [lut] * len(srcs), level_shift)
    return run


gcase("k_u8_batch<2, true, false>", f"inv batch {NONSMALL}, random table")(_u8_inv(NONSMALL, Q_RAND, True, False))
gcase("k_u8_batch<2, true, false>", "inv_i16_u8 512 wide, no table, no level shift")(_u8_inv([(512, _rows_for(N_INV, 512))], None, False, True))
gcase("k_u8_batch<2, true, true>", "inv batch 4096x2400, all-ones table")(_u8_inv(SMALL, np.ones(64, dtype=np.float32), True, False))
gcase("k_u8_batch<2, true, true>", "inv_i16_u8 4096x2400, random table")(_u8_inv(SMALL, Q_RAND, True, True))
gcase("k_u8_batch<0, false, false>", f"roundtrip batch {NONSMALL}, quality 50")(_u8_rt(NONSMALL, TAME, True, False))
gcase("k_u8_batch<0, true, false>", f"roundtrip batch {NONSMALL}, an entry below 1/16")(_u8_rt(NONSMALL, WILD, True, False))
gcase("k_u8_batch<0, false, true>", "roundtrip_u8 4096x2400, quality 50, no level shift")(_u8_rt(SMALL, TAME, False, True))
gcase("k_u8_batch<0, true, true>", "roundtrip_u8 4096x2400, an entry below 1/16")(_u8_rt(SMALL, WILD, True, True))


def _f32(shape):
    def run(torch, M):
        (src,) = _planes_of(f32_gpu_blocks(), [shape])
        out = torch.full(src.shape, 3.25, dtype=torch.float32, device="cuda")
        M.inv_f32(dev(src), out, shape[0], shape[1])
        return lambda: R.check_planes("f32", [src], [out.cpu().numpy()], [None])
    return run


def _f32_wide():
    """512 x 524288 (65536 block rows): the wide linear form; the input repeats every 512 rows, so must the output"""
    W, period, H = 512, 512, 524288

    def run(torch, M):
        blks = f32_gpu_blocks()
        (src,) = _planes_of(blks[rng(53).permutation(len(blks))], [(W, period)])
        d = dev(src).repeat(H // period, 1)
        out = torch.empty_like(d)
        M.inv_f32(d, out, W, H)
        del d

        def check():
            same = bool((out.view(H // period, period, W) == out[:period].unsqueeze(0)).all().item())
            assert same, "a period of the output differs from the first"
            R.check_planes("f32", [src], [out[:period].cpu().numpy()], [None])
        return check
    return run


N_F32 = 60000 + 2 * (13 + 2 * 13 * 64 + 2 * 11 * 200 + 2000)
gcase("k_f32_tile<1>", "inv 1024 wide")(_f32((1024, _rows_for(N_F32, 1024))))
gcase("k_f32<1, false>", "inv 200 wide")(_f32((200, _rows_for(N_F32, 200))))
gcase("k_f32<1, true>", "inv 512x524288")(_f32_wide())


@pytest.mark.gpu
@pytest.mark.parametrize("kernels,desc,run", GPU_CASES, ids=[f"{'+'.join(k)}|{d}" for k, d, _ in GPU_CASES])
def test_gpu_inverse_instantiation_vs_double(gpu, kernels, desc, run):
    torch, M = gpu
    torch.cuda.synchronize()
    M.kernel_counts_reset()
    check = run(torch, M)
    torch.cuda.synchronize()
    counts = M.kernel_counts()
    ran = set(counts) - {"k_park_table"}  # a table's first sight uploads it
    assert ran == set(kernels), f"{desc}: expected {sorted(kernels)}, the tally shows {sorted(counts.items())}"
    check()


def test_gpu_cases_cover_every_inverse_instantiation():
    """the cases above name every inverse / round-trip instantiation of the coverage matrix"""
    import test_kernel_coverage as K
    inverse = {k for k in K.MATRIX_KERNELS if k.startswith(("k_i16_tile<1", "k_i16_tile<2", "k_i16<1", "k_i16<2", "k_i16_batch<1",
                                                               "k_i16_batch<2", "k_u8_batch<0", "k_u8_batch<2", "k_f32_tile<1", "k_f32<1"))}
    covered = {k for ks, _, _ in GPU_CASES for k in ks}
    assert len(inverse) == 34 and inverse <= covered, sorted(inverse - covered)


# ------------------------------------------------------------------------------------------ GPU: decoded JPEG pixels
def dqt_sets():
    """name -> one DQT per component (integers 1..255, natural order)"""
    from simd_dct_amd.jpeg_encode import quality_tables
    sets = {"ones": [np.ones(64)], "all-255": [np.full(64, 255)]}
    for q in (1, 25, 50, 75, 95, 100):
        sets[f"quality-{q}"] = [np.array(quality_tables(q)[0])]
    luma, chroma = quality_tables(75)
    sets["per-component"] = [np.array(luma), np.array(chroma), rng(60).integers(1, 256, 64)]
    return {k: [np.asarray(t, dtype=np.uint16) for t in v] for k, v in sets.items()}


def decoder_planes(q, W, H, k):
    """int16 [H, W] quantised coefficients: IEEE 1180 pixel blocks of every case through rne(DCT / Q), and baseline-range extremes
    (|coefficient| <= 1023) that push pixels past 0 and 255: worst-pixel sign patterns at 1023 with DC at +-1023, flat blocks"""
    n = (W // 8) * (H // 8)
    r = rng(70 + k)
    px = np.concatenate([p[r.choice(10000, -(-n // 6), replace=False)] for p, _, _ in ieee().values()])
    qq = np.asarray(q, dtype=np.float64).reshape(8, 8)
    c = np.clip(R.rne(R.dct2(px) / qq), -1023, 1023)
    ext = np.where(R.worst_pixel_blocks([1.0]) > 0, 1023, -1023)
    ext[:32, 0, 0], ext[32:, 0, 0] = 1023, -1023
    flat = np.zeros((8, 8, 8))
    flat[:, 0, 0] = [-1023, -1022, -1020, -1012, 1012, 1020, 1022, 1023]
    allb = np.concatenate([ext, flat, c])[:n]
    return R.plane(r.permutation(allb), W, H).astype(np.int16)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(dqt_sets()))
def test_gpu_decoded_pixels_follow_t81_rule(gpu, name):
    """files encoded from known coefficient planes (tests/jpeg_scan_encoder.py), decoded by decode_jpeg without restart markers and
    with a DRI: every pixel equals clamp(rne(IDCT(c * Q) + 128), 0, 255) wherever the tie window decides it"""
    import jpeg_scan_encoder as E
    from simd_dct_amd import jpeg_decode as D
    tables = dqt_sets()[name]
    W, H = 400, 240
    nc = len(tables)
    frame = dict(width=W, height=H, comps=[(1, 1)] * nc)
    planes = [decoder_planes(tables[ci], W, H, ci) for ci in range(nc)]
    assert all(np.abs(p).max() <= 1023 for p in planes)
    for dri in (0, 7):
        scan = dict(comps=[(0, 0, 0)] + [(ci, 1, 1) for ci in range(1, nc)], dri=dri)
        data, _ = E.encode_file(frame, [scan], planes, E.ANNEX_K, qtables=tables, table_per_component=True)
        got = D.decode_jpeg(data)
        for ci in range(nc):
            c = R.blocks(planes[ci])
            want, exact, tol = R.u8_pixels(c, tables[ci])
            assert (want == 0).any() and (want == 255).any()
            R.assert_exact_rule(R.blocks(got[ci].cpu().numpy()), want, exact, tol, R.U8_RANGE, f"{name} component {ci} dri {dri}")
