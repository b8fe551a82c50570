"""Every JPEG entry point that takes stream= on a stream that is NOT torch's current one (simd_dct_amd/jpeg_decode.py, jpeg_encode.py,
jpeg_transcode.py, jpeg_progressive.py; the contract: INTEGRATION.md section 2, api._on_stream).

The other JPEG tests call with stream=None, or with a stream that a graph capture has made current, so torch's own work for a call (its
allocations, zero fills, uploads and the copies the host reads) and the engine's launches always shared one stream.  Here they do not,
unless the call itself sees to it.

Truth: the same call with stream=None and the null stream current, the arrangement the other tests hold to Pillow, the checkers and
the float64 references.  Files compare byte for byte, tensors with torch.equal, exceptions by type and status / message.

Arrangements (tests/stream_stall.py makes the stalls; a stall lasts max(0.2 s, 5 x T_host), T_host the wall time of the truth call made
once, warm: every hazard window lies inside the call's host phase, and a stall above 2 s means the picture is too big):
  A      current stream = default, stream=s (fresh), s stalled before the call.  A call that returns something computed on the host must
         not return, or raise, before the stall's event has completed: bytes, a status or an exception handed back while earlier work on
         the call's own stream is pending cannot have waited for the call's own work.  Then the result is compared.  Before the call
         the caching allocator is seeded with freed blocks of the sizes of the status, offset and histogram words, filled with 0 (a
         stale read of a hostile file's status looks clean) or 0x7F7F7F7F (a stale read of a good file's looks failed).
  A-raw  as A with stream=s.cuda_stream, the integer handle.
  B      the DEFAULT stream is stalled, stream=s is idle: a fill the call left on the current stream lands after the kernels that add
         into the filled words and wipes them.  Compared after s.synchronize() and torch.cuda.synchronize().
  D      with torch.cuda.stream(s): the call with stream=None, s stalled: the form that always worked.
Every case ends with s.synchronize(); torch.cuda.synchronize() before anything is freed or compared.

Cases: decode_jpeg on a restart-marked, an unmarked and a progressive file of one 203 x 117 4:2:0 picture (planes, RGB, RGB at 1/2,
coefficients=True); decode_coefficients; one hostile file per route (statuses from the serial checkers); the unmarked decoder's second
pass; encode_jpeg in eight forms (the second packing pass: 88 x 88 grey noise at quality 100, the smallest square of whole blocks whose
scan, 12243 bytes, exceeds the first buffer of pixels + 4096; at 64 x 64 it is 6440 of 8192); encode_coefficients (a loss count
included); transcode_jpeg; the asynchronous wrappers that allocate or fill an argument left to them; two host threads with a stream
each.  CPU: no function of jpeg_*.py that takes `stream` allocates, fills or reads outside api._on_stream."""
import ast
import functools
import glob
import os
import re
import threading
import time

import numpy as np
import pytest

import jpeg_decode_checker as C
import jpeg_progressive_status as PS
import jpeg_scan_encoder as E
from simd_dct_amd import api, jfif, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 203, 117  # 13 x 8 MCUs at 4:2:0: partial MCUs both ways, 15 / 8 restart intervals per scan, a ragged last row
MX, MY = 13, 8
FRAME = dict(width=W, height=H, comps=[(2, 2), (1, 1), (1, 1)])
SCAN = dict(comps=[(0, 0, 0), (1, 1, 1), (2, 1, 1)])
S420 = [(2, 2), (1, 1), (1, 1)]
FILLS = {"stale-0": 0, "stale-7f": 0x7F7F7F7F}
MIN_STALL, MAX_STALL = 0.2, 2.0


# ------------------------------------------------------------------------------------------ CPU: the rule, held statically
HELPER = "_on_stream"
TORCH_MAKERS = {"zeros", "empty"}  # torch.zeros / torch.empty: a block tied to the current stream, a fill enqueued on it
HOST_TOUCH = {"cpu", "item", "to"}  # copies ordered on the current stream


def stream_lint(source):
    """-> ["function:line call"] for every torch.zeros / torch.empty / .cpu() / .item() / .to( that a function taking `stream` makes
    outside a `with ... _on_stream(...)` block (nested functions are judged on their own)"""
    found = []

    def under_helper(node):
        return any(isinstance(i.context_expr, ast.Call) and getattr(i.context_expr.func, "attr", getattr(i.context_expr.func, "id", None)) == HELPER
                   for i in node.items)

    def visit(node, fn, covered):
        if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)) and node is not fn:
            return
        if isinstance(node, ast.With) and under_helper(node):
            for i in node.items:
                visit(i, fn, covered)
            for child in node.body:
                visit(child, fn, True)
            return
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and not covered:
            a = node.func
            if (a.attr in TORCH_MAKERS and getattr(a.value, "id", None) == "torch") or a.attr in HOST_TOUCH:
                found.append(f"{fn.name}:{node.lineno} {ast.unparse(a)}")
        for child in ast.iter_child_nodes(node):
            visit(child, fn, covered)

    for fn in ast.walk(ast.parse(source)):
        if isinstance(fn, (ast.FunctionDef, ast.AsyncFunctionDef)) and any(a.arg == "stream" for a in fn.args.args + fn.args.kwonlyargs):
            visit(fn, fn, False)
    return found


def test_the_lint_bites():
    bad = ("def f(x, stream=None):\n    w = torch.zeros((1,))\n    with api._on_stream(stream):\n        y = torch.empty(3)\n    return int(w.item()), y.cpu(), x.to(0)\n"
           "def g(x):\n    return x.cpu()\n"
           "def h(stream):\n    def inner(t):\n        return t.item()\n    with _on_stream(stream, None), other():\n        return torch.zeros(2).cpu().item()\n")
    assert [p.split(" ", 1)[1] for p in stream_lint(bad)] == ["torch.zeros", "w.item", "y.cpu", "x.to"]


def test_functions_that_take_a_stream_touch_torch_only_under_the_helper():
    files = sorted(glob.glob(os.path.join(ROOT, "simd_dct_amd", "jpeg_*.py")))
    assert len(files) >= 4
    found = {os.path.basename(f): stream_lint(open(f).read()) for f in files}
    assert not any(found.values()), {k: v for k, v in found.items() if v}
    src = open(os.path.join(ROOT, "simd_dct_amd", "api.py")).read()
    assert f"def {HELPER}(" in src


# ------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    torch.cuda.set_device(0)
    api.init(0)
    return torch


@functools.lru_cache(None)
def _image():
    import torch
    return torch.stack([synth.plane_u8_torch(W, H, "photo", seed=40 + k) for k in range(3)], dim=-1).contiguous()


@functools.lru_cache(None)
def _files():
    """the three decoder routes on one picture -> ({route: file}, its quantised coefficient planes as numpy, padded to the MCU grid)"""
    from simd_dct_amd import jpeg_decode as D
    from simd_dct_amd import jpeg_encode as J
    marked = J.encode_jpeg(_image())  # quality 75, 4:2:0: three scans, RSTm after every block row
    prog = J.encode_jpeg(_image(), progressive=True)
    planes = [c.cpu().numpy() for c in D.decode_coefficients(marked)[1]]
    luma, chroma = J.quality_tables(75)
    unmarked, _ = E.encode_file(FRAME, [dict(SCAN, dri=0)], planes, dict(E.ANNEX_K), qtables=[luma, chroma])
    info = {k: D.read_file(f) for k, f in dict(marked=marked, unmarked=unmarked, progressive=prog).items()}
    assert [s["restart_interval"] for s in info["marked"]["scans"]] == [26, 13, 13] and info["marked"]["sof"] == 0xC0
    assert [s["restart_interval"] for s in info["unmarked"]["scans"]] == [0]
    assert info["progressive"]["sof"] == 0xC2 and len(info["progressive"]["scans"]) == 8
    return dict(marked=marked, unmarked=unmarked, progressive=prog), planes


def hostile_baseline(planes, dri):
    """the interleaved scan of the planes with sixteen 1-bits in place of the DC code of the first block of the middle MCU row
    -> (file, failing scan, the status the serial checker gives)"""
    block = ((MY // 2) * MX) * 6
    bad, st = E.encode_file(FRAME, [dict(SCAN, dri=dri)], planes, dict(E.ANNEX_K), inject={0: dict(block=block, at="dc", put=["1" * 16])})
    assert "inject_bit" in st[0]
    if dri:
        want = C.decode(bad)[1][0]
        assert len(want) == MY and want[MY // 2] == C.BAD_CODE and all(s == C.OK for k, s in enumerate(want) if k != MY // 2), want
        return bad, 0, [int(s) for s in want]
    from test_jpeg_decode_unmarked import checker_scan
    status, n = checker_scan(bad)[:2]
    assert (status, n) == (C.BAD_CODE, block)
    return bad, 0, [int(status), int(n)]


def hostile_progressive(prog, band=(3, 9), mid=7):
    """three bytes cut from the end of interval `mid` of the luma band's scan (the corrupted-interval case of
    test_jpeg_decode_progressive.py) -> (file, failing scan, the statuses jpeg_progressive_status gives that scan)"""
    info = jfif.read_progressive_jpeg(prog)
    k = [i for i, s in enumerate(info["scans"]) if (s["ss"], s["se"]) == band and s["components"][0]["index"] == 0][0]
    sc = info["scans"][k]
    body = prog[sc["start"]:sc["end"]]
    cut = body.index(bytes([0xFF, 0xD0 + mid])) - 3  # the first RST7 closes interval 7
    assert cut > body.index(bytes([0xFF, 0xD0 + mid - 1])) + 2, "the interval holds fewer than three bytes"
    bad = prog[:sc["start"]] + body[:cut] + body[cut + 3:] + prog[sc["end"]:]
    statuses = PS.decode(bad)[1]
    assert [i for i, s in enumerate(statuses) if any(s)] == [k] and [i for i, s in enumerate(statuses[k]) if s] == [mid], statuses
    return bad, k, [int(s) for s in statuses[k]]


@functools.lru_cache(None)
def _hostile():
    files, planes = _files()
    return dict(marked=hostile_baseline(planes, MX), unmarked=hostile_baseline(planes, 0), progressive=hostile_progressive(files["progressive"]))


PERIODIC_MCUS = 1100


@functools.lru_cache(None)
def _periodic():
    """A scan the unmarked decoder cannot synchronise in its default four fix rounds.  (The periodic scan of test_jpeg_decode_synthetic.py
    does: measured on the MI355X, its four rounds leave one decode launch.)  Every block is the same 64 bits -- DC difference 0, six AC
    levels of category 4, one of 3, one of 2, EOB; no stuffed byte -- so every 8 KiB chunk begins at a block, 1024 blocks after the last.
    The MCU holds 7 blocks (sampling 2x2, 2x1, 1x1) that share one pair of tables: a chunk's guess, "the MCU's first block", parses the
    same bits as the truth and keeps its block-in-MCU index 1024 c mod 7 = 2 c mod 7 off, which is zero only for chunk 7.  Chunks 1..6
    become exact one per round, so four rounds leave NOT_SYNCHRONISED and decode_scan decodes a second time."""
    z = np.zeros(64, dtype=np.int64)
    z[1:9] = [9, -10, 12, -9, 11, -13, 5, -2]
    nat = np.zeros(64, dtype=np.int64)
    nat[E.ZZ] = z
    comps = [(2, 2), (2, 1), (1, 1)]
    planes = [np.tile(nat.reshape(8, 8), (v, PERIODIC_MCUS * h)).astype(np.int16) for h, v in comps]
    data, st = E.encode_file(dict(width=16 * PERIODIC_MCUS, height=16, comps=comps), [dict(comps=[(0, 0, 0), (1, 0, 0), (2, 0, 0)], dri=0)], planes,
                             {k: E.ANNEX_K[k] for k in ((0, 0), (1, 0))})
    assert st[0]["max_block_bits"] == 64 and st[0]["length"] == 8 * 7 * PERIODIC_MCUS > 7 * 8192 and not st[0]["stuffed"]
    return data, planes


@functools.lru_cache(None)
def _coefs():
    """the picture's coefficient planes on the device (encode_coefficients' input), and a single plane with two AC levels and one DC step
    that no baseline scan holds, with the counts numpy gives"""
    import torch
    planes = _files()[1]
    dev = [torch.from_numpy(p).cuda() for p in planes]
    loss = planes[0].copy()
    loss[3, 5], loss[9, 8 * 3 + 1] = 1024, -1024
    loss[16, 8] = loss[16, 0] + 2048
    ac = loss.astype(np.int64).copy()
    ac[::8, ::8] = 0
    dc = loss[::8, ::8].astype(np.int64)
    n_ac = int((np.abs(ac) > 1023).sum())
    n_dc = int((np.abs(np.diff(dc, axis=1, prepend=0)) > 2047).sum())  # a restart interval per block row: the predictor starts at 0
    assert n_ac == 2 and n_dc >= 1
    torch.cuda.synchronize()
    return dev, torch.from_numpy(loss).cuda(), n_ac, n_dc


def _qtables():
    from simd_dct_amd import jpeg_encode as J
    luma, chroma = J.quality_tables(75)
    return [luma, chroma, chroma]


class Case:
    """make(torch) -> fn(stream): the call.  host: it returns something computed on the host (it must wait for its stream).
    tally: (kernel, launches) the call must make.  check(truth): what the truth itself must satisfy (checkers, numpy)."""

    def __init__(self, name, make, host=True, tally=None, check=None):
        self.name, self.make, self.host, self.tally, self.check = name, make, host, tally, check


CASES = {}


def case(name, **kw):
    def add(make):
        CASES[name] = Case(name, make, **kw)
        return make
    return add


DECODE_FORMS = {"planes": dict(), "rgb": dict(mode="RGB"), "rgb-half": dict(mode="RGB", scale_denom=2), "coefficients": dict(coefficients=True)}
ROUTES = ("marked", "unmarked", "progressive")

for _route in ROUTES:
    for _form, _kw in DECODE_FORMS.items():
        @case(f"decode-{_route}-{_form}")
        def _(torch, route=_route, kw=_kw):
            from simd_dct_amd import jpeg_decode as D
            data = _files()[0][route]
            return lambda st: D.decode_jpeg(data, stream=st, **kw)

    @case(f"coefficients-{_route}")
    def _(torch, route=_route):
        from simd_dct_amd import jpeg_decode as D
        data = _files()[0][route]
        return lambda st: D.decode_coefficients(data, stream=st)[1]

    def _hostile_check(truth, route=_route):
        _, scan, status = _hostile()[route]
        assert truth == ("JpegDecodeError", (scan, status)), truth

    @case(f"hostile-{_route}", check=_hostile_check)
    def _(torch, route=_route):
        from simd_dct_amd import jpeg_decode as D
        data = _hostile()[route][0]
        return lambda st: D.decode_jpeg(data, stream=st)


def _periodic_check(truth):
    planes, coefs = truth[1]
    assert all(np.array_equal(c.cpu().numpy(), p) for c, p in zip(coefs, _periodic()[1]))


@case("decode-unmarked-second-pass", tally=("k_um_final", 2), check=_periodic_check)
def _(torch):
    from simd_dct_amd import jpeg_decode as D
    data = _periodic()[0]
    return lambda st: D.decode_jpeg(data, coefficients=True, stream=st)


ENCODE_FORMS = {"default": dict(), "one-launch": dict(two_launch=False), "interleaved": dict(interleaved=True), "optimize": dict(optimize=True),
                "optimize-interleaved": dict(optimize=True, interleaved=True), "progressive": dict(progressive=True)}

for _form, _kw in ENCODE_FORMS.items():
    @case(f"encode-{_form}")
    def _(torch, kw=_kw):
        from simd_dct_amd import jpeg_encode as J
        img = _image()
        return lambda st: J.encode_jpeg(img, stream=st, **kw)


@case("encode-grey-64")
def _(torch):
    from simd_dct_amd import jpeg_encode as J
    img = synth.plane_u8_torch(64, 64, "photo", seed=50)  # multiples of 8: no front launch
    return lambda st: J.encode_jpeg(img, stream=st)


@case("encode-second-pack", tally=("k_pack_write<true>", 2))
def _(torch):
    from simd_dct_amd import jpeg_encode as J
    img = synth.plane_u8_torch(88, 88, "noise", seed=77)  # 12243 bytes of scan > 88 * 88 + 4096 (module docstring)
    return lambda st: J.encode_jpeg(img, quality=100, stream=st)


COEF_FORMS = {"optimize": dict(optimize=True), "annex-k": dict(optimize=False), "interleaved": dict(interleaved=True), "progressive": dict(progressive=True)}

for _form, _kw in COEF_FORMS.items():
    @case(f"encode-coefficients-{_form}")
    def _(torch, kw=_kw):
        from simd_dct_amd import jpeg_transcode as T
        coefs, q = _coefs()[0], _qtables()
        return lambda st: T.encode_coefficients(coefs, q, W, H, S420, stream=st, **kw)


def _loss_check(truth):
    _, _, n_ac, n_dc = _coefs()
    assert truth[0] == "MdctError" and int(re.match(r"(\d+) coefficients cannot be written", truth[1]).group(1)) == n_ac + n_dc, truth


@case("encode-coefficients-loss", check=_loss_check)
def _(torch):
    from simd_dct_amd import jpeg_transcode as T
    loss, q = _coefs()[1], _qtables()[:1]
    return lambda st: T.encode_coefficients([loss], q, loss.shape[1], loss.shape[0], [(1, 1)], stream=st)


@case("transcode-rot90")
def _(torch):
    from simd_dct_amd import jpeg_transcode as T
    data = _files()[0]["marked"]
    return lambda st: T.transcode_jpeg(data, transform="rot90", trim=True, stream=st)  # rot90 mirrors y: 117 rows are trimmed to 112


@case("transcode-progressive-in")
def _(torch):
    from simd_dct_amd import jpeg_transcode as T
    data = _files()[0]["progressive"]
    return lambda st: T.transcode_jpeg(data, stream=st)


def _unrep_check(want):
    def check(truth):
        hist, unrep = truth[1]
        assert int(unrep.item()) == want() > 0, (int(unrep.item()), want())
    return check


@case("coef-histogram", host=False, check=_unrep_check(lambda: _coefs()[2] + _coefs()[3]))
def _(torch):
    from simd_dct_amd import jpeg_transcode as T
    loss = _coefs()[1]
    return lambda st: T.coef_histogram([loss], [(1, 1)], stream=st)


@case("prog-dc-histogram", host=False, check=_unrep_check(lambda: _coefs()[3]))
def _(torch):
    from simd_dct_amd import jpeg_progressive as P
    loss = _coefs()[1]
    return lambda st: P.prog_dc_histogram([loss], [(1, 1)], stream=st)


@case("prog-ac-histogram", host=False, check=_unrep_check(lambda: _coefs()[2]))
def _(torch):
    from simd_dct_amd import jpeg_progressive as P
    loss = _coefs()[1]
    return lambda st: P.prog_ac_histogram(loss, 1, 63, stream=st)


@case("symbol-histogram", host=False)
def _(torch):
    from simd_dct_amd import jpeg_encode as J
    planes, q = J.to_planes(_image()), J.quality_tables(75)
    return lambda st: J.symbol_histogram(planes, S420, q, stream=st)


@case("to-planes", host=False)
def _(torch):
    from simd_dct_amd import jpeg_encode as J
    img = _image()
    return lambda st: J.to_planes(img, stream=st)


@case("to-rgb", host=False)
def _(torch):
    from simd_dct_amd import jpeg_decode as D
    planes = D.decode_jpeg(_files()[0]["marked"])
    return lambda st: D.to_rgb(planes, S420, W, H, stream=st)


HOST = [n for n, c in CASES.items() if c.host]
ASYNC = [n for n, c in CASES.items() if not c.host]


# ------------------------------------------------------------------------------------------ running a case
def _outcome(call):
    """("ok", value) or (exception type, what it carries)"""
    from simd_dct_amd import jpeg_decode as D
    try:
        return ("ok", call())
    except D.JpegDecodeError as e:
        return ("JpegDecodeError", (e.scan, [int(x) for x in e.status]))
    except Exception as e:  # whatever a call built on stale words raises is a result to compare, after the streams have drained
        return (type(e).__name__, str(e))


def _same(a, b):
    import torch
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        return isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


def _brief(v):
    import torch
    if isinstance(v, torch.Tensor):
        return f"tensor{list(v.shape)}"
    if isinstance(v, (bytes, bytearray)):
        return f"{len(v)} bytes"
    if isinstance(v, (tuple, list)):
        return "(" + ", ".join(_brief(x) for x in v) + ")"
    return repr(v)[:200]


_prepared = {}


def _prepare(torch, name):
    """-> (fn, truth, T_host): the call, its outcome with stream=None on the null stream, and the wall time of that call made warm"""
    if name not in _prepared:
        c = CASES[name]
        assert torch.cuda.current_stream() == torch.cuda.default_stream()
        fn = c.make(torch)
        torch.cuda.synchronize()
        _outcome(lambda: fn(None))  # warm
        torch.cuda.synchronize()
        if c.tally:
            api.kernel_counts_reset()
        t = time.perf_counter()
        truth = _outcome(lambda: fn(None))
        t_host = time.perf_counter() - t
        torch.cuda.synchronize()
        if c.tally:
            assert api.kernel_counts().get(c.tally[0], 0) == c.tally[1], (c.tally, api.kernel_counts())
        if c.check:
            c.check(truth)
        print(f"\nT_host {name}: {t_host * 1e3:.2f} ms -> {truth[0]}")
        _prepared[name] = (fn, truth, t_host)
    return _prepared[name]


def _seed(torch, fill):
    """freed blocks of the sizes the calls allocate for their status, offset and histogram words (int32 counts: up to 512 bytes for a
    status or offset array, 2184 bytes for encode_coefficients' words, 7.3 KB for jpeg_progressive.encode's), holding `fill`"""
    blocks = [torch.full((n,), fill, dtype=torch.int32, device="cuda") for n in [128] * 32 + [640] * 8 + [2048] * 8]
    torch.cuda.synchronize()
    del blocks


def run(torch, name, arrangement, fill=None, raw=False):
    from stream_stall import measured_seconds, stall
    c = CASES[name]
    fn, truth, t_host = _prepare(torch, name)
    seconds = max(MIN_STALL, 5 * t_host)
    assert seconds <= MAX_STALL, f"T_host {t_host:.3f} s asks for a stall of {seconds:.2f} s: the picture is too big"
    default = torch.cuda.default_stream()
    assert torch.cuda.current_stream() == default
    s = torch.cuda.Stream()
    if fill is not None:
        _seed(torch, fill)
    torch.cuda.synchronize()
    if c.tally:
        api.kernel_counts_reset()
    ev = got = waited = None
    try:
        if arrangement == "B":
            ev = stall(default, seconds)
            got = _outcome(lambda: fn(s))
        elif arrangement == "D":
            ev = stall(s, seconds)
            with torch.cuda.stream(s):
                got = _outcome(lambda: fn(None))
        else:
            ev = stall(s, seconds)
            got = _outcome(lambda: fn(s.cuda_stream if raw else s))
        waited = ev.query()
    finally:  # before anything is freed or allocated: pending kernels never run on memory that something else has taken
        s.synchronize()
        torch.cuda.synchronize()
    problems = []
    took = measured_seconds(ev)
    print(f"\n{name} {arrangement}: stall {took:.3f} s of {seconds:.3f} s, stall over at return: {waited}, outcome {got[0]}")
    # the factor 5 in the stall is margin for host jitter; a stall that came out at half of it (the sleep counts shader cycles, and the
    # clock moves) is still 2.5 x T_host and 0.1 s, twenty times the longest T_host of these cases.  Below that the case showed nothing.
    if took < 0.5 * seconds:
        problems.append(f"the stall took {took:.3f} s of the {seconds:.3f} s asked for")
    if c.host and arrangement != "B" and not waited:
        problems.append("it returned while the stall on its own stream was pending: it cannot have waited for its own work")
    if not _same(got, truth):
        problems.append(f"{_brief(got)} differs from the null-stream call's {_brief(truth)}")
    if c.tally and api.kernel_counts().get(c.tally[0], 0) != c.tally[1]:
        problems.append(f"{c.tally[0]} ran {api.kernel_counts().get(c.tally[0], 0)} times, not {c.tally[1]}")
    assert not problems, f"{name} {arrangement}: " + "; ".join(problems)


@pytest.mark.gpu
@pytest.mark.parametrize("fill", list(FILLS))
@pytest.mark.parametrize("name", HOST)
def test_a_stalled_own_stream(gpu, name, fill):
    run(gpu, name, "A", fill=FILLS[fill])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["decode-marked-rgb", "encode-default"])
def test_a_stalled_own_stream_as_a_raw_handle(gpu, name):
    run(gpu, name, "A", fill=FILLS["stale-7f"], raw=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ASYNC)
def test_a_stalled_own_stream_asynchronous_wrappers(gpu, name):
    run(gpu, name, "A")


@pytest.mark.gpu
@pytest.mark.parametrize("name", HOST + ASYNC)
def test_b_stalled_current_stream(gpu, name):
    run(gpu, name, "B")


@pytest.mark.gpu
@pytest.mark.parametrize("name", HOST)
def test_d_stream_made_current(gpu, name):
    run(gpu, name, "D")


# ------------------------------------------------------------------------------------------ two host threads
THREAD_CASES = ["decode-marked-rgb", "decode-unmarked-rgb", "decode-progressive-rgb", "hostile-marked", "encode-optimize"]
ROUNDS = 8


@pytest.mark.gpu
def test_two_host_threads_with_a_stream_each(gpu):
    torch = gpu
    prepared = {n: _prepare(torch, n) for n in THREAD_CASES}
    torch.cuda.synchronize()
    results, errors = [[], []], [None, None]

    def work(k):
        try:
            torch.cuda.set_device(0)
            s = torch.cuda.Stream()
            order = THREAD_CASES if k == 0 else THREAD_CASES[::-1]
            for r in range(ROUNDS):
                for n in order[r % len(order):] + order[:r % len(order)]:
                    results[k].append((n, _outcome(lambda: prepared[n][0](s))))
            s.synchronize()
        except BaseException as e:  # noqa: B036 -- reported by the main thread
            errors[k] = e

    threads = [threading.Thread(target=work, args=(k,), daemon=True) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    alive = [t.is_alive() for t in threads]
    assert not any(alive), f"threads still running after the timeout: {alive}"
    torch.cuda.synchronize()
    assert errors == [None, None], errors
    for k in range(2):
        assert len(results[k]) == ROUNDS * len(THREAD_CASES)
        for i, (n, got) in enumerate(results[k]):
            assert _same(got, prepared[n][1]), f"thread {k}, call {i} ({n}): {_brief(got)} differs from the single-thread {_brief(prepared[n][1])}"
