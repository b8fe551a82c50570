"""Every engine-own forward DCT and quantiser path held to the mathematical DCT (tests/idct_reference.py: float64, from the cosine
definition), not to the checker it is kept in lock-step with.

The rule: an int16 coefficient must equal sat_i16(rne(DCT(x - shift) / Q)) wherever every value within the window of the exact one
rounds and saturates alike; a float32 coefficient must lie within the window.  The window is 2^-24 * (TIE_K_FWD * sum|x - shift| / 8 / Q
+ 4 * |exact|) per coefficient.  Flat blocks are exact in float32 through every operation when Q(0,0) is a power of
two, so they are compared with no window, .5 ties (to even) included.

CPU: the checker's orc_fwd_i16, orc_fwd_u8_i16, orc_fwd_f32 and the composition behind the records and the Huffman rows, on every
input-and-table pair below; three mutants of oracle/dct_oracle.c that the old |got - want| <= 1 bound passes and the rule refuses.
GPU: every forward-only instantiation of k_i16_tile / k_i16 / k_i16_batch / k_u8_batch / k_f32_tile / k_f32 at its tile, linear,
SMALL and batch shapes, the launch tally naming it; the fused records, Huffman-row and one-launch scan kernels; and encode_jpeg's four
forms from the coefficients decoded out of their files, the file's DQT as the table."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import idct_reference as R
import oracle as O
import test_idct_accuracy as A
from test_idct_accuracy import _planes_of, _rows_for, dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RNG_SEED = 8118


def rng(k=0):
    return np.random.default_rng(RNG_SEED + k)


# ------------------------------------------------------------------------------------------ inputs
def basis_signs():
    """[64, 8, 8] bool: block v * 8 + u holds the sign pattern of basis function (v, u) over the pixels, the input that makes the
    largest coefficient at (v, u)"""
    return np.einsum("vy,ux->vuyx", R.C, R.C).reshape(64, 8, 8) >= 0


def _mixed(parts, k):
    """one list in a fixed random order, so that every plane cut from it holds blocks of every family"""
    b = np.concatenate(parts)
    return b[rng(k).permutation(len(b))]


def _u8_special():
    sgn, eye = basis_signs(), np.eye(64, dtype=np.int64).reshape(64, 8, 8) * 255
    ext = np.where(sgn, 255, 0)
    flat = np.arange(256)[:, None, None] * np.ones((1, 8, 8), dtype=np.int64)
    return [ext, 255 - ext, flat, eye, 255 - eye, rng(1).integers(0, 256, (2000, 8, 8))]


@functools.lru_cache(maxsize=None)
def u8_blocks():
    """the six IEEE 1180 pixel sets + 128 clipped, each basis function's sign pattern at 0 / 255 and its negation, flat blocks at every
    level, single-pixel impulses, 2000 uniform random blocks"""
    b = _mixed([np.clip(px + 128, 0, 255) for px, _, _ in A.ieee().values()] + _u8_special(), 2).astype(np.uint8)
    b.flags.writeable = False
    return b


@functools.lru_cache(maxsize=None)
def u8_few_blocks():
    """the same families with 600 of the IEEE 1180 blocks: what the small fused and coded planes are cut from"""
    b = _mixed([np.clip(px[:100] + 128, 0, 255) for px, _, _ in A.ieee().values()] + _u8_special(), 3).astype(np.uint8)
    b.flags.writeable = False
    return b


I16_AMPS = (1, 255, 1023, 4095, 32767)


def _i16_families(a):
    """sign patterns, flat blocks, impulses and 400 random blocks at amplitude a, both signs (32767: -32768 on the other side)"""
    lo = -32768 if a == 32767 else -a
    sgn, eye = basis_signs(), np.eye(64, dtype=np.int64).reshape(64, 8, 8)
    ext = np.where(sgn, a, lo)
    flat = np.array([a, lo])[:, None, None] * np.ones((1, 8, 8), dtype=np.int64)
    return [ext, (a + lo) - ext, flat, eye * a, eye * lo, rng(10 + a).integers(lo, a + 1, (400, 8, 8))]


@functools.lru_cache(maxsize=None)
def i16_blocks():
    """the families at amplitudes 1, 255, 1023, 4095 and 32767 / -32768, and the round trips' blocks (the IEEE 1180 pixel sets among
    them)"""
    b = _mixed([x for a in I16_AMPS for x in _i16_families(a)] + [A.rt_i16_gpu_blocks().astype(np.int64)], 4).astype(np.int16)
    b.flags.writeable = False
    return b


@functools.lru_cache(maxsize=None)
def f32_blocks():
    b = _mixed([A.f32_blocks(), i16_blocks().astype(np.float32)], 5)
    b.flags.writeable = False
    return b


def _quality(q):
    from simd_dct_amd.jpeg_encode import quality_tables
    return np.array(quality_tables(q)[0], dtype=np.float32)


FRAC = np.where(np.arange(64) % 2 == 0, 0.5, 1.0 / 3.0).astype(np.float32)  # fl(1 / Q) is inexact at every odd entry
TABLES = {  # name -> 64 entries in natural order, or None (no quantiser)
    "none": None,
    "ones": np.ones(64, dtype=np.float32),
    "quality-1": _quality(1),
    "quality-50": _quality(50),
    "quality-100": _quality(100),
    "random-255": A.Q_RAND,
    "8.01": A.B801,
    "half-third": FRAC,
    "wild": A.WILD,  # an entry below 1/16: the general 8-bit build
}
Q50, ONES = TABLES["quality-50"], TABLES["ones"]
assert Q50[0] == 16 and A.WILD[5] < 1.0 / 16


# ------------------------------------------------------------------------------------------ the checker, block lists in and out
sz, vp, f32p = ctypes.c_size_t, ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)


def _declare(lib):
    lib.orc_fwd_i16.argtypes = [vp, vp, sz, sz, f32p, sz, sz, sz, sz]
    lib.orc_fwd_u8_i16.argtypes = [vp, vp, sz, sz, f32p, ctypes.c_int, sz, sz, sz, sz]
    lib.orc_fwd_f32.argtypes = [vp, vp, sz, sz, sz, sz, sz, sz]
    lib.orc_zigzag_rle_i16.argtypes = [vp, sz, sz, sz, sz, sz, vp, vp, vp]
    return lib


def orc_fwd(lib, kind, blks, q=None):
    """the checker `lib` on a block list: kind 'fwd_i16' / 'fwd_u8' (level shift on) -> int16 blocks, 'fwd_f32' -> float32 blocks"""
    dt = {"fwd_i16": np.int16, "fwd_u8": np.uint8, "fwd_f32": np.float32}[kind]
    src, W, H = A._to_plane(blks, dt)
    src = np.ascontiguousarray(src)
    out = np.zeros((H, W), dtype=np.float32 if kind == "fwd_f32" else np.int16)
    lp = None
    if q is not None:
        keep, lp = O._lut(q)
    if kind == "fwd_f32":
        rc = lib.orc_fwd_f32(src.ctypes.data, out.ctypes.data, W, W, W, H, 0, H // 8)
    elif kind == "fwd_i16":
        rc = lib.orc_fwd_i16(src.ctypes.data, out.ctypes.data, W, W, lp, W, H, 0, H // 8)
    else:
        rc = lib.orc_fwd_u8_i16(src.ctypes.data, out.ctypes.data, W, W, lp, 1, W, H, 0, H // 8)
    assert rc == 0, rc
    return R.blocks(out)[:len(blks)]


ZIGZAG = np.array(sorted(range(64), key=lambda i: (i // 8 + i % 8, i // 8 if (i // 8 + i % 8) % 2 else i % 8)))  # scan position -> natural index


def expand_records(levels, runs, counts):
    """run/level records [nblk, 64] + counts [nblk] -> natural-order coefficients [nblk, 8, 8]: pair i of a block sits at scan position
    cumsum(run + 1) - 1, the pairs beyond the block's count are scratch"""
    levels, runs, counts = np.asarray(levels), np.asarray(runs).astype(np.int64), np.asarray(counts).astype(np.int64)
    pos = np.cumsum(runs + 1, axis=1) - 1
    live = np.arange(64)[None, :] < counts[:, None]
    assert (pos[live] < 64).all()
    scan = np.zeros((len(levels), 65), dtype=np.int16)
    b = np.broadcast_to(np.arange(len(levels))[:, None], pos.shape)
    scan[b[live], pos[live]] = levels[live]
    nat = np.zeros((len(levels), 64), dtype=np.int16)
    nat[:, ZIGZAG] = scan[:, :64]
    return nat.reshape(-1, 8, 8)


def orc_records(lib, blks, q):
    """the checker's composition behind mdct_fwd_u8_records: pixels -> coefficients -> records, expanded again"""
    src, W, H = A._to_plane(blks, np.uint8)
    coef = np.ascontiguousarray(R.plane(R.tile_blocks(orc_fwd(lib, "fwd_u8", R.blocks(src), q), (W // 8) * (H // 8)), W, H), dtype=np.int16)
    nblk = (W // 8) * (H // 8)
    lv, rn, ct = np.zeros((nblk, 64), dtype=np.int16), np.zeros((nblk, 64), dtype=np.uint8), np.zeros(nblk, dtype=np.uint8)
    assert lib.orc_zigzag_rle_i16(coef.ctypes.data, W, W, H, 0, H // 8, lv.ctypes.data, rn.ctypes.data, ct.ctypes.data) == 0
    return expand_records(lv, rn, ct)[:len(blks)]


# ------------------------------------------------------------------------------------------ the rule on a checker
SHIFT = {"fwd_i16": 0.0, "fwd_u8": 128.0}
INPUTS = {"fwd_i16": i16_blocks, "fwd_u8": u8_blocks}
PAIRS = [(kind, t) for kind in ("fwd_i16", "fwd_u8") for t in TABLES]


@functools.lru_cache(maxsize=None)
def _rule(kind, table):
    """(want, exact, tol) of the pair, computed once"""
    out = R.fwd_coefficients(INPUTS[kind](), TABLES[table], SHIFT[kind])
    for a in out:
        a.flags.writeable = False
    return out


def flat_inputs(kind):
    if kind == "fwd_u8":
        v = np.arange(256)
    else:
        v = np.concatenate([np.arange(-32768, 32768, 37), np.arange(-2001, 2002), [32767]])
    return (v[:, None, None] * np.ones((1, 8, 8), dtype=np.int64)).astype(np.uint8 if kind == "fwd_u8" else np.int16), v - int(SHIFT[kind])


FLAT_TABLES = [t for t, q in TABLES.items() if q is None or float(np.log2(q[0])).is_integer()]


def check_flat(lib, kind, table):
    """flat blocks: DC = sat_i16(rne(8 (v - shift) / Q00)) exactly, every AC coefficient zero; no window"""
    q = TABLES[table]
    x, v = flat_inputs(kind)
    got = orc_fwd(lib, kind, x, q)
    want = np.zeros(x.shape)
    want[:, 0, 0] = np.clip(np.rint(8.0 * v / (1.0 if q is None else float(q[0]))), -32768, 32767)
    bad = got != want
    assert not bad.any(), (f"{kind} table {table}: flat blocks", int(bad.sum()), v[np.argwhere(bad)[0][0]], got[tuple(np.argwhere(bad)[0])], want[tuple(np.argwhere(bad)[0])])


def check_pair(lib, kind, table):
    want, exact, tol = _rule(kind, table)
    got = orc_fwd(lib, kind, INPUTS[kind](), TABLES[table])
    R.assert_exact_rule(got, want, exact, tol, R.I16_RANGE, f"{kind} table {table}")


def check_f32(lib):
    x = f32_blocks()
    exact, tol = R.fwd_f32(x)
    err = np.abs(orc_fwd(lib, "fwd_f32", x).astype(np.float64) - exact)
    assert (err <= tol).all(), ("fwd_f32", float((err / np.maximum(tol, 1e-300)).max()) * R.TIE_K_FWD, int((err > tol).sum()))


def rule_failures(lib, pairs=PAIRS):
    """every check of the rule on one checker build -> the messages of those it breaks"""
    checks = [lambda: check_f32(lib)]
    checks += [functools.partial(check_pair, lib, kind, t) for kind, t in pairs]
    checks += [functools.partial(check_flat, lib, kind, t) for kind in ("fwd_i16", "fwd_u8") for t in FLAT_TABLES]
    out = []
    for c in checks:
        try:
            c()
        except AssertionError as e:
            out.append(str(e)[:300])
    return out


def old_bound_failures(lib, pairs=PAIRS):
    """what test_kernel_coverage.check_i16_fwd_vs_double asserted alone: |got - sat_i16(rne(exact))| <= 1.  On the 8-bit inputs and
    the int16 blocks up to amplitude 4095: at full scale the butterflies' terms reach 2^21, where a constant cut to five digits already
    moves a coefficient by 2 and the old bound notices"""
    out = []
    for kind, t in pairs:
        x = INPUTS[kind]()
        keep = np.abs(x.astype(np.int64)).reshape(len(x), 64).max(axis=1) <= 4095
        d = np.abs(orc_fwd(lib, kind, x, TABLES[t]).astype(np.float64) - _rule(kind, t)[0])[keep]
        if d.max() > 1:
            out.append((kind, t, float(d.max())))
    return out


# ------------------------------------------------------------------------------------------ CPU: the reference itself
def test_reference_forward_is_orthonormal_and_inverts():
    assert np.abs(R.C @ R.C.T - np.eye(8)).max() < 1e-15
    x = rng(20).integers(-32768, 32768, (200, 8, 8)).astype(np.float64)
    y = R.dct2(x)
    assert np.abs((y * y).sum(axis=(-2, -1)) - (x * x).sum(axis=(-2, -1))).max() < 1e-9 * (x * x).sum(axis=(-2, -1)).max()  # Parseval
    z = rng(21).integers(-2048, 2048, (200, 8, 8)).astype(np.float64)
    assert np.abs(R.dct2(R.idct2(z)) - z).max() < 1e-9
    # each basis function transforms to its own impulse
    basis = np.einsum("vy,ux->vuyx", R.C, R.C).reshape(64, 8, 8)
    assert np.abs(R.dct2(basis).reshape(64, 64) - np.eye(64)).max() < 1e-14
    # flat blocks: exactly 8 (v - 128) in DC and zero AC, no window
    for kind in ("fwd_u8", "fwd_i16"):
        x, v = flat_inputs(kind)
        want, exact, _ = R.fwd_coefficients(x, None, SHIFT[kind])
        assert np.array_equal(exact[:, 0, 0], 8.0 * v) and np.abs(exact.reshape(len(x), 64)[:, 1:]).max() < 1e-9
        assert np.array_equal(want[:, 0, 0], np.clip(8.0 * v, -32768, 32767)) and not want.reshape(len(x), 64)[:, 1:].any()
    # the scan order restated here is T.81 Figure A.6 as the checker walks it
    assert np.array_equal(ZIGZAG, O.zigzag_table())


def test_forward_window_and_rule():
    x = np.full((1, 8, 8), 129 + 1)  # 8 * 2 / 16 = 1: decided; 8 * 1 / 16 = .5: a tie, never decided
    want, exact, tol = R.fwd_coefficients(x, Q50, 128.0)
    assert want[0, 0, 0] == 1 and R.decided(exact, tol, *R.I16_RANGE).all()
    want, exact, tol = R.fwd_coefficients(x - 1, Q50, 128.0)
    assert exact[0, 0, 0] == 0.5 and want[0, 0, 0] == 0 and not R.decided(exact, tol, *R.I16_RANGE)[0, 0, 0]
    assert float(tol[0, 0, 0]) == R.ULP * (R.TIE_K_FWD * 64 / 8 / 16 + 4 * 0.5)
    # saturated by more than the window: decided
    want, exact, tol = R.fwd_coefficients(np.full((1, 8, 8), 32767), None)
    assert want[0, 0, 0] == 32767 and R.decided(exact, tol, *R.I16_RANGE)[0, 0, 0]
    e, t = R.fwd_f32(np.ones((1, 8, 8)))
    assert float(t[0, 0, 0]) == R.TIE_K_FWD * R.ULP * 8 and abs(e[0, 0, 0] - 8) < 1e-12
    # the round trip's forward half is this helper
    xs = i16_blocks()[:500]
    _, _, _, skip = R.roundtrip(xs, A.B801, "i16")
    _, yq, tf = R.fwd_coefficients(xs, A.B801, k=R.TIE_K_FWD_RT)
    assert np.array_equal(skip, ((R.tie_distance(yq) <= tf) & (np.abs(yq) < 32767.5)).any(axis=(-2, -1)))


@pytest.mark.parametrize("kind,table", PAIRS, ids=[f"{k}-{t}" for k, t in PAIRS])
def test_pairs_are_decided_by_the_float64_rule_alone(kind, table):
    """the condition on the inputs: under half of a pair's coefficients sit inside the window of a tie, so the floor in
    assert_exact_rule holds before any transform under test is looked at; planes cut from the lists (mixed order) meet it too"""
    want, exact, tol = _rule(kind, table)
    dec = R.decided(exact, tol, *R.I16_RANGE)
    assert dec.mean() > 0.5, float(dec.mean())
    worst = min(float(dec[k:k + 6250].mean()) for k in range(0, len(dec), 6250))  # the smallest plane of the GPU cases: 200 x 2000
    assert worst > 0.5, worst
    if table == "none" and kind == "fwd_i16":  # the DC and the low AC positions saturate at both ends
        for v, u in ((0, 0), (0, 1), (1, 0), (1, 1)):
            assert want[:, v, u].min() == -32768 and want[:, v, u].max() == 32767, (v, u)
    if kind == "fwd_u8":  # the largest coefficient 8-bit samples make, at both signs
        assert want[:, 0, 0].min() == R.rne(-1024 / TABLES["ones" if table == "none" else table][0]).clip(-32768, 32767)


# ------------------------------------------------------------------------------------------ CPU: the checker
@pytest.mark.parametrize("kind,table", PAIRS, ids=[f"{k}-{t}" for k, t in PAIRS])
def test_checker_forward_follows_the_rule(kind, table):
    check_pair(_declare(O.oracle()), kind, table)


def test_checker_forward_f32_within_window():
    check_f32(_declare(O.oracle()))


@pytest.mark.parametrize("kind", ["fwd_i16", "fwd_u8"])
def test_checker_flat_blocks_exact_without_window(kind):
    assert {"none", "ones", "quality-50", "quality-100", "half-third"} <= set(FLAT_TABLES)
    x, v = flat_inputs(kind)
    assert (np.abs(8.0 * v / 16 % 1 - 0.5) < 1e-12).sum() > 100  # quality 50: every odd level is a .5 tie
    for t in FLAT_TABLES:
        check_flat(_declare(O.oracle()), kind, t)


@pytest.mark.parametrize("table", list(TABLES))
def test_checker_records_follow_the_rule(table):
    """the composition behind mdct_fwd_u8_records / the Huffman rows: the records of the checker's coefficients, expanded"""
    want, exact, tol = _rule("fwd_u8", table)
    got = orc_records(_declare(O.oracle()), u8_blocks(), TABLES[table])
    R.assert_exact_rule(got, want, exact, tol, R.I16_RANGE, f"records table {table}")


def coded_planes():
    """[(W, H, uint8 plane)]: 264 x 64 and 1928 x 24 (a partial last tile) of the 8-bit families"""
    shapes = [(264, 64), (1928, 24)]
    return [(W, H, p.astype(np.uint8)) for (W, H), p in zip(shapes, _planes_of(u8_few_blocks(), shapes))]


def decode_scan(scan, W, H, q):
    """a packed one-component scan with a restart interval per block row -> its coefficient plane, by the decoding checker"""
    import jpeg_decode_checker as DC
    from simd_dct_amd import jfif
    data = jfif.write_jpeg([dict(blocks_per_row=W // 8, qtable=[int(v) for v in q], scan=np.asarray(scan, dtype=np.uint8))], W, H)
    planes, status, info = DC.decode(data)
    assert all(s == 0 for st in status for s in st), status
    assert np.array_equal(info["qtables"][0], np.asarray(q, dtype=np.float32))
    return planes[0][:H, :W]


@pytest.mark.parametrize("table", ["quality-50", "ones"])
def test_checker_huffman_rows_follow_the_rule(table):
    q = TABLES[table]
    for W, H, src in coded_planes():
        lv, rn, ct = O.u8_records(src, W, H, lut=q)
        seg, nb, stride = O.huffman_rows(lv, rn, ct, W, H)
        out, off = O.jpeg_pack_rows(seg, nb, stride)
        R.check_planes("fwd_u8", [src], [decode_scan(out[:int(off[-1])], W, H, q)], [q])


# ------------------------------------------------------------------------------------------ CPU: the rule has teeth
MUTANTS = {  # name -> (text of oracle/dct_oracle.c, its replacement)
    "forward AAN constant to five digits": ("static const float A_1306 = 1.306562964876376528f;", "static const float A_1306 = 1.30656f;"),
    "forward table entry (7, 7) times 1.00002": ("fwd[v * 8 + u] = (float)(1.0 / (8.0 * a));",
                                                 "fwd[v * 8 + u] = (float)(1.0 / (8.0 * a) * (v == 7 && u == 7 ? 1.00002 : 1.0));"),
    "quantiser rounds halves away from zero": ("  float t = fmaf(y, qf, magic);", "  float t = (float)round((double)y * (double)qf) + magic;"),
}


def build_checker(tmp_path, name, old=None, new=None):
    text = open(os.path.join(ROOT, "oracle", "dct_oracle.c")).read()
    if old is not None:
        assert text.count(old) == 1, (name, text.count(old))
        text = text.replace(old, new)
    d = tmp_path / f"m{abs(hash(name)) % 10 ** 8}"
    d.mkdir()
    (d / "dct_oracle.c").write_text(text)
    so = str(d / "liboracle_variant.so")
    subprocess.run(["gcc", "-std=c11", "-O2", "-ffp-contract=off", "-fPIC", "-msse4.1", "-shared", "-pthread", "-I", os.path.join(ROOT, "oracle"), "-o", so,
                    str(d / "dct_oracle.c"), os.path.join(ROOT, "oracle", "time_mt.c"), "-lm"], check=True)
    return _declare(ctypes.CDLL(so))


def test_unmodified_copy_of_the_checker_passes(tmp_path):
    lib = build_checker(tmp_path, "copy")
    assert not rule_failures(lib) and not old_bound_failures(lib)


@pytest.mark.parametrize("name", list(MUTANTS))
def test_mutant_meets_the_old_bound_and_fails_the_rule(tmp_path, name):
    lib = build_checker(tmp_path, name, *MUTANTS[name])
    assert not old_bound_failures(lib), name
    fails = rule_failures(lib)
    print(name, len(fails), fails[:3])
    assert fails, f"{name}: the rule did not notice"


# ------------------------------------------------------------------------------------------ GPU: every forward-only instantiation
@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    torch.cuda.set_device(0)
    import simd_dct_amd as M
    M.init(0)
    return torch, M


GPU_CASES = []  # (kernels, description, run() -> check())


def gcase(kernels, desc):
    def reg(fn):
        GPU_CASES.append(((kernels,) if isinstance(kernels, str) else tuple(kernels), desc, fn))
        return fn
    return reg


NONSMALL, SMALL = A.NONSMALL, A.SMALL
N_I16 = 5 * (128 + 2 + 128 + 400) + 60000 + 128 + 2000
N_U8 = 60000 + 128 + 256 + 128 + 2000
N_F32 = A.N_F32 - 60000 + N_I16


def _i16_single(shape, lut):
    def run(torch, M):
        (src,) = _planes_of(i16_blocks(), [shape])
        out = torch.full(src.shape, 77, dtype=torch.int16, device="cuda")
        M.fwd_i16(dev(src), out, shape[0], shape[1], lut=lut)
        return lambda: R.check_planes("fwd_i16", [src], [out.cpu().numpy()], [lut])
    return run


for tname, lut, what in (("false", None, "no table"), ("true", A.Q_RAND, "random-255"), ("true", FRAC, "entries 0.5 and 1/3")):
    for w, shp in ((2, (512, _rows_for(N_I16, 512))), (4, SMALL[0])):
        gcase(f"k_i16_tile<0, {tname}, true, {w}>", f"fwd_i16 {shp[0]}x{shp[1]}, {what}")(_i16_single(shp, lut))
    gcase(f"k_i16<0, {tname}, true>", f"fwd_i16 200 wide, {what}")(_i16_single((200, _rows_for(N_I16, 200)), lut))
gcase("k_i16_tile<0, true, true, 2>", "fwd_i16 512 wide, table 8.01")(_i16_single((512, _rows_for(N_I16, 512)), A.B801))


def _i16_batch(shapes, luts):
    def run(torch, M):
        srcs = _planes_of(i16_blocks(), shapes)
        outs = [torch.full(s.shape, 77, dtype=torch.int16, device="cuda") for s in srcs]
        M.i16_batch("fwd", [(dev(s), o, s.shape[1], s.shape[0], l) for s, o, l in zip(srcs, outs, luts)])
        return lambda: R.check_planes("fwd_i16", srcs, [o.cpu().numpy() for o in outs], luts)
    return run


for sm, shapes in (("false", NONSMALL), ("true", SMALL)):
    gcase(f"k_i16_batch<0, 1, true, {sm}>", f"fwd batch {shapes}, quality 50")(_i16_batch(shapes, [Q50] * len(shapes)))
    mixed = shapes if len(shapes) > 1 else shapes + [(200, 24)]
    gcase(f"k_i16_batch<0, 1, true, {sm}>", f"fwd batch {mixed}, some planes with a table")(
        _i16_batch(mixed, [A.B801 if j % 2 == 0 else None for j in range(len(mixed))]))


def _u8_batch(shapes, lut):
    def run(torch, M):
        srcs = [p.astype(np.uint8) for p in _planes_of(u8_blocks(), shapes)]
        outs = [torch.full(s.shape, 77, dtype=torch.int16, device="cuda") for s in srcs]
        M.u8_i16_batch("fwd", [(dev(s), o, s.shape[1], s.shape[0], lut) for s, o in zip(srcs, outs)])
        return lambda: R.check_planes("fwd_u8", srcs, [o.cpu().numpy() for o in outs], [lut] * len(srcs))
    return run


for sm, shapes in (("false", NONSMALL), ("true", SMALL)):
    gcase(f"k_u8_batch<1, false, {sm}>", f"fwd_u8 batch {shapes}, quality 50")(_u8_batch(shapes, Q50))
    gcase(f"k_u8_batch<1, true, {sm}>", f"fwd_u8 batch {shapes}, an entry below 1/16")(_u8_batch(shapes, A.WILD))
gcase("k_u8_batch<1, false, false>", f"fwd_u8 batch {NONSMALL}, entries 0.5 and 1/3")(_u8_batch(NONSMALL, FRAC))
gcase("k_u8_batch<1, false, false>", f"fwd_u8 batch {NONSMALL}, random-255")(_u8_batch(NONSMALL, A.Q_RAND))


def _u8_single(shape, lut):
    def run(torch, M):
        src = _planes_of(u8_blocks(), [shape])[0].astype(np.uint8)
        out = torch.full(src.shape, 77, dtype=torch.int16, device="cuda")
        M.fwd_u8_i16(dev(src), out, shape[0], shape[1], lut=lut)
        return lambda: R.check_planes("fwd_u8", [src], [out.cpu().numpy()], [lut])
    return run


gcase("k_u8_i16_fwd", "fwd_u8_i16 200 wide, table 8.01")(_u8_single((200, _rows_for(N_U8, 200)), A.B801))


def _f32(shape):
    def run(torch, M):
        src = _planes_of(f32_blocks(), [shape])[0].astype(np.float32)
        out = torch.full(src.shape, 3.25, dtype=torch.float32, device="cuda")
        M.fwd_f32(dev(src), out, shape[0], shape[1])
        return lambda: R.check_planes("fwd_f32", [src], [out.cpu().numpy()], [None])
    return run


gcase("k_f32_tile<0>", "fwd_f32 1024 wide")(_f32((1024, _rows_for(N_F32, 1024))))
gcase("k_f32<0, false>", "fwd_f32 200 wide")(_f32((200, _rows_for(N_F32, 200))))

WIDE_F32 = "k_f32<0, true>"  # 512 x 524288: test_kernel_coverage.py keeps it, with the rule on one period


@pytest.mark.gpu
@pytest.mark.parametrize("kernels,desc,run", GPU_CASES, ids=[f"{'+'.join(k)}|{d}" for k, d, _ in GPU_CASES])
def test_gpu_forward_instantiation_vs_double(gpu, kernels, desc, run):
    torch, M = gpu
    torch.cuda.synchronize()
    M.kernel_counts_reset()
    check = run(torch, M)
    torch.cuda.synchronize()
    counts = M.kernel_counts()
    ran = set(counts) - {"k_park_table"}  # a table's first sight uploads it
    assert ran == set(kernels), f"{desc}: expected {sorted(kernels)}, the tally shows {sorted(counts.items())}"
    check()


def test_gpu_cases_cover_every_forward_instantiation():
    """the cases above name every forward-only instantiation of the coverage matrix in these families, the wide float32 form excepted"""
    import test_kernel_coverage as K
    families = ("k_i16_tile<", "k_i16<", "k_i16_batch<", "k_u8_batch<", "k_f32_tile<", "k_f32<")
    inverse = ("k_i16_tile<1", "k_i16_tile<2", "k_i16<1", "k_i16<2", "k_i16_batch<1", "k_i16_batch<2", "k_u8_batch<0", "k_u8_batch<2", "k_f32_tile<1", "k_f32<1")
    forward = {k for k in K.MATRIX_KERNELS if k.startswith(families) and not k.startswith(inverse)}
    assert all(k.startswith(("k_i16_tile<0", "k_i16<0", "k_i16_batch<0", "k_u8_batch<1", "k_f32_tile<0", "k_f32<0")) for k in forward)
    covered = {k for ks, _, _ in GPU_CASES for k in ks}
    assert len(forward) == 15 and WIDE_F32 in forward and forward - {WIDE_F32} <= covered, sorted(forward - covered)
    assert len(N_CHECK) == 3 and N_CHECK == (len(i16_blocks()), len(u8_blocks()), len(f32_blocks()))


N_CHECK = (N_I16, N_U8, N_F32)


# ------------------------------------------------------------------------------------------ GPU: the fused and the coded paths
def _only(M, prefixes):
    ran = set(M.kernel_counts()) - {"k_park_table"}
    assert ran and all(k.startswith(prefixes) for k in ran), (prefixes, sorted(ran))


@pytest.mark.gpu
@pytest.mark.parametrize("table", ["quality-50", "ones"])
@pytest.mark.parametrize("path", ["u8_records", "i16_records", "huffman_rows+pack", "jpeg_scan"])
def test_gpu_fused_paths_vs_double(gpu, path, table):
    torch, M = gpu
    from simd_dct_amd import api
    q = TABLES[table]
    for W, H, src in coded_planes():
        n, nblk = H // 8, (W // 8) * (H // 8)
        torch.cuda.synchronize()
        M.kernel_counts_reset()
        if path.endswith("records"):
            lv = torch.zeros((nblk, 64), dtype=torch.int16, device="cuda")
            rn, ct = torch.zeros((nblk, 64), dtype=torch.uint8, device="cuda"), torch.zeros((nblk,), dtype=torch.uint8, device="cuda")
            if path == "u8_records":
                api.fwd_u8_records(dev(src), W, H, lv, rn, ct, lut=q)
            else:  # the same samples, level shift done here
                api.fwd_i16_records(dev(src.astype(np.int16) - 128), W, H, lv, rn, ct, lut=q)
            torch.cuda.synchronize()
            _only(M, ("k_u8_records<true" if path == "i16_records" else "k_u8_records<false",))
            got = R.plane(expand_records(lv.cpu().numpy(), rn.cpu().numpy(), ct.cpu().numpy()), W, H)
        else:
            stride = api.huffman_seg_stride(W)
            seg = torch.zeros((n * stride,), dtype=torch.uint8, device="cuda")
            off = torch.zeros((n + 1,), dtype=torch.int64, device="cuda")
            cap = 2 * n * stride
            out = torch.zeros((cap,), dtype=torch.uint8, device="cuda")
            if path == "jpeg_scan":
                work = torch.zeros((n + 2,), dtype=torch.int64, device="cuda")
                api.fwd_u8_jpeg_scan(dev(src), W, H, seg, work, out, off, lut=q, out_capacity=cap)
                torch.cuda.synchronize()
                _only(M, ("k_px_huffman_rows<false, 4, true",))
            else:
                nb = torch.zeros((n,), dtype=torch.int32, device="cuda")
                api.fwd_u8_huffman_rows(dev(src), W, H, seg, nb, lut=q)
                api.jpeg_pack_rows(seg, nb, stride, n, out, off, out_capacity=cap)
                torch.cuda.synchronize()
                _only(M, ("k_px_huffman_rows<false, 4, false", "k_pack_"))
            total = int(off[-1].item())
            assert 0 < total <= cap
            got = decode_scan(out[:total].cpu().numpy(), W, H, q)
        R.check_planes("fwd_u8", [src], [got], [q])


FORMS = {"grey": dict(), "three": dict(), "interleaved": dict(interleaved=True), "optimize": dict(optimize=True), "interleaved+optimize": dict(interleaved=True, optimize=True)}
SUBS = ["4:4:4", "4:2:2", "4:2:0"]
ENC = [("grey", "4:4:4")] + [(f, s) for f in FORMS if f != "grey" for s in SUBS]


def encoder_image(W=203, H=117):
    """smooth content with noise and hard edges, so that quality 25 keeps levels and quality 100 stays inside the coder's range"""
    r = rng(30)
    y, x = np.mgrid[0:H, 0:W]
    img = np.stack([128 + 90 * np.sin(x / 9.0 + c) * np.cos(y / 7.0 - c) for c in range(3)], axis=-1) + r.normal(0, 10, (H, W, 3))
    img[20:60, 30:90] = r.integers(0, 256, (40, 60, 3))
    img[70:, 120:] = np.where((x[70:, 120:, None] // 4 + y[70:, 120:, None] // 4) % 2 == 0, 0, 255)
    return np.clip(img, 0, 255).astype(np.uint8)


def check_file_against_rule(data, image, sub, grey, interleaved, what, decoded=None, min_decided=0.5):
    """the coefficients the decoding checker reads out of `data` against the rule on the encoding checker's planes, padding included,
    with the file's own DQT as the table -> the coefficient planes.  decoded: (planes, statuses, dict(frame=..., qtables=[one per
    component])) of another serial checker in jpeg_decode_checker.decode's form (a progressive file's: tests/jpeg_sweep.py), in place of
    that checker's own.  min_decided: idct_reference.check_planes' cap (a caller that pools planes of a few blocks hands 0 and applies
    the cap itself)."""
    import jpeg_decode_checker as DC
    import jpeg_encode_checker as C
    from test_jpeg_encode_optimized import _grid
    coefs, status, info = DC.decode(data) if decoded is None else decoded
    frame = info["frame"]
    assert all(s == 0 for st in status for s in st), (what, status)
    H, W = image.shape[:2]
    sampling = [(1, 1)] if grey else C.SAMPLING[sub]
    assert [(h, v) for _, h, v, _ in frame["components"]] == sampling
    sizes = _grid(W, H, sampling, interleaved)
    planes = C.planes(image, sub, padded=sizes)
    for k, (p, (pw, ph), c) in enumerate(zip(planes, sizes, coefs)):
        assert p.shape == (ph, pw) and c.shape[0] >= ph and c.shape[1] >= pw
        q = info["qtables"][k]
        try:
            R.check_planes("fwd_u8", [p], [c[:ph, :pw]], [q], min_decided=min_decided)
        except AssertionError as e:
            raise AssertionError(f"{what} component {k}: {e}") from None
    return info["qtables"], coefs


@pytest.mark.gpu
@pytest.mark.parametrize("q", [25, 100])
@pytest.mark.parametrize("form,sub", ENC)
def test_gpu_encode_jpeg_coefficients_vs_double(gpu, form, sub, q):
    """encode_jpeg's files: grey, three scans, one interleaved scan and optimised tables (k_scan_rows<H, V>, k_opt<H, V, false>); and the
    symbol histogram of the same call (k_opt<H, V, true>) against the symbols of the coefficients decoded out of its file"""
    torch, M = gpu
    import jpeg_optimal_tables as T
    from simd_dct_amd import jpeg_encode as J
    from simd_dct_amd.jpeg_encode import quality_tables
    img = encoder_image()
    grey = form == "grey"
    host = img[..., 1].copy() if grey else img
    kw = dict(FORMS[form])
    seen = []
    for optimize in ([False, True] if grey else [kw.pop("optimize", False)]):
        original = J.optimal_tables

        def spy(hist, grey=False):
            seen.append(np.asarray(hist.cpu() if hasattr(hist, "cpu") else hist).astype(np.int64).copy())
            return original(hist, grey=grey)

        J.optimal_tables = spy
        try:
            torch.cuda.synchronize()
            M.kernel_counts_reset()
            data = J.encode_jpeg(host, quality=q, subsampling=sub, optimize=optimize, **kw)
            torch.cuda.synchronize()
            ran = set(M.kernel_counts())
        finally:
            J.optimal_tables = original
        inter = bool(kw.get("interleaved"))
        qtables, coefs = check_file_against_rule(data, host, sub, grey, inter, f"{form} {sub} q{q} optimize={optimize}")
        luma, chroma = quality_tables(q)
        assert all(np.array_equal(t, np.asarray(luma if k == 0 else chroma, dtype=np.float32)) for k, t in enumerate(qtables))
        if inter:
            assert any(k.startswith("k_opt<" if optimize else "k_scan_rows<") for k in ran), sorted(ran)
        if optimize:
            assert any(k.startswith("k_opt<") and k.endswith("true>") for k in ran) and any(k.startswith("k_opt<") and k.endswith("false>") for k in ran), sorted(ran)
            assert len(seen) == 1
            hist, _ = T.histogram_of_file(data)
            assert np.array_equal(seen[0].reshape(hist.shape), hist), (form, sub, q)
