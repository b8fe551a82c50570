"""CPU tests of the thirteen shared libraries as a set: what the Makefile builds, what the headers declare, what the binding modules
(simd_dct_amd/_lib.py and _*_lib.py) bind and load, and the label each library's errors are reported under.

Every library is a simd_dct_amd._lib.Library; _lib.LIBRARIES holds them all.  For each: the mdct_* functions its headers declare are
its SIGNATURES and the built library exports them; the libmdct_* libraries it was linked against (the Makefile's row) are
libmdct_hip.so and those its binding loads first (`after`); and the built libraries are the registered ones, no more and no fewer.
The error texts are checked through the public wrappers alone, with arguments the C libraries refuse on the host: nothing is
launched, no device is needed."""
import ctypes
import glob
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import __graft_entry__ as G
from simd_dct_amd import (_jpegcoef_lib, _jpegcolor_lib, _jpegdec_batch_lib, _jpegdec_lib, _jpegdec_prog_lib, _jpegdec_unmarked_lib, _jpegenc_batch_lib,
                          _jpegenc_opt_lib, _jpegenc_scan_lib, _jpegprog_lib, _jpegscale_lib, _lib, api)
from simd_dct_amd import jpeg_decode as D
from simd_dct_amd import jpeg_encode as J
from simd_dct_amd import jpeg_progressive as P
from simd_dct_amd import jpeg_transcode as T
from test_kernel_coverage import LLVM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# library -> the label its errors carry: "<label> status <rc>: <the C library's message>".  The decoder of scans without markers
# reports as the decoder it extends.
LABELS = {
    "mdct_hip": "mdct",
    "mdct_jpegdec": "mdct_jpegdec",
    "mdct_jpegdec_unmarked": "mdct_jpegdec",
    "mdct_jpegdec_prog": "mdct_jpegdec_prog",
    "mdct_jpegdec_batch": "mdct_jpegdec_batch",
    "mdct_jpegcolor": "mdct_jpegcolor",
    "mdct_jpegscale": "mdct_jpegscale",
    "mdct_jpegenc": "mdct_jpegenc",
    "mdct_jpegenc_scan": "mdct_jpegenc_scan",
    "mdct_jpegenc_batch": "mdct_jpegenc_batch",
    "mdct_jpegenc_opt": "mdct_jpegenc_opt",
    "mdct_jpegcoef": "mdct_jpegcoef",
    "mdct_jpegprog": "mdct_jpegprog",
}


# ------------------------------------------------------------------------------------------ (d) the labels, through the wrappers
def _u8(*shape):
    return torch.zeros(shape, dtype=torch.uint8)


def _i16(*shape):
    return torch.zeros(shape, dtype=torch.int16)


def _i32(n=1):
    return torch.zeros(n, dtype=torch.int32)


NO_TABLES = types.SimpleNamespace(handle=None)
OVERSUBSCRIBED = ([0, 5] + [0] * 14, [0, 1, 2, 3, 4])  # five codes of two bits


def _grey_desc(restart_interval):
    """a legal one-component scan descriptor over a CPU tensor: 2 x 1 blocks"""
    coef = _i16(8, 16)
    return D.scan_desc([(coef, 2, 1, 1, 1, 0, 2)], 2, 1, restart_interval), coef


def _mdct_hip():
    a = np.zeros(64 * 16, dtype=np.uint8)
    api.fwd_quant_u8(None, a, api.QUANTIZE_BASE, 64, 16, 0, 2)  # null source


def _jpegdec():
    D.Tables([OVERSUBSCRIBED, None, None, None])


def _jpegdec_unmarked():
    desc, keep = _grey_desc(0)
    D.decode_unmarked(desc, NO_TABLES, _u8(64), _u8(4096), _i32(2), scan_len=64)


def _jpegdec_prog():
    desc, keep = _grey_desc(2)
    D.decode_prog(desc, 0, 0, NO_TABLES, _u8(64), None, _i32(1), scan_len=64)


def _jpegdec_batch():
    D.BatchPlan([], 0)  # a batch of no scans


def _jpegcolor():
    planes = [_u8(32, 64), _u8(16, 43), _u8(16, 32)]
    D.to_rgb(planes, [(3, 2), (2, 1), (1, 1)], 64, 32, out=_u8(32, 64, 3))  # a fractional sampling ratio


def _jpegscale():
    D.scaled_inverse([(_u8(8, 8), _i16(8, 8), 1, 1, None, 3)])  # blocks of 3 x 3 samples


def _jpegenc_scan():
    planes = [_u8(16, 16), _u8(8, 8), _u8(8, 8)]
    J.scan_rows(planes, [(2, 2), (1, 1), (1, 1)], J.quality_tables(75), _u8(4096), _i32(1), _i32(1), seg_stride=2)  # a stride no segment fits in


def _jpegenc_batch():
    J.BatchPlan([], "HWC", J.quality_tables(75))  # a batch of no images


def _jpegenc_opt():
    J.optimal_table([1] * 5)  # neither 12..16 DC categories nor 256 AC symbols


def _jpegcoef():
    T.transform_planes(_i16(8, 16), _i16(8, 8), "flip_h")  # destination of another shape


def _jpegprog():
    P.prog_ac_histogram(_i16(8, 16), 0, 5)  # an AC band that begins at the DC coefficient


# library -> (its binding module, a wrapper call the C library refuses on the host, the status it answers: MDCT_INVALID_PARAMETER).
# libmdct_jpegenc.so has none: its one wrapper, to_planes, takes device tensors only.
REFUSALS = {
    "mdct_hip": (_lib, _mdct_hip, 1),
    "mdct_jpegdec": (_jpegdec_lib, _jpegdec, 1),
    "mdct_jpegdec_unmarked": (_jpegdec_unmarked_lib, _jpegdec_unmarked, 1),
    "mdct_jpegdec_prog": (_jpegdec_prog_lib, _jpegdec_prog, 1),
    "mdct_jpegdec_batch": (_jpegdec_batch_lib, _jpegdec_batch, 1),
    "mdct_jpegcolor": (_jpegcolor_lib, _jpegcolor, 1),
    "mdct_jpegscale": (_jpegscale_lib, _jpegscale, 1),
    "mdct_jpegenc_scan": (_jpegenc_scan_lib, _jpegenc_scan, 1),
    "mdct_jpegenc_batch": (_jpegenc_batch_lib, _jpegenc_batch, 1),
    "mdct_jpegenc_opt": (_jpegenc_opt_lib, _jpegenc_opt, 1),
    "mdct_jpegcoef": (_jpegcoef_lib, _jpegcoef, 1),
    "mdct_jpegprog": (_jpegprog_lib, _jpegprog, 1),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_a_refusal_is_reported_under_the_librarys_label_with_its_message(name):
    binding, call, rc = REFUSALS[name]
    with pytest.raises(api.MdctError) as e:
        call()
    (last_error,) = [n for n in binding.SIGNATURES if n.endswith("_last_error")]
    said = getattr(binding.load(), last_error)().decode()  # the C library's own words, read past the wrapper
    assert said and str(e.value) == f"{LABELS[name]} status {rc}: {said}"


def test_the_refusals_cover_every_library_with_a_device_free_wrapper():
    assert set(LABELS) - set(REFUSALS) == {"mdct_jpegenc"} and len(LABELS) == 13


# ------------------------------------------------------------------------------------------ the registry
@pytest.fixture(scope="module")
def built():
    G.build_hip()


def _library(name):
    (lib,) = [lib for lib in _lib.LIBRARIES if lib.name == name]
    return lib


def test_the_registry_holds_the_thirteen_libraries_in_dependency_order():
    LIBRARIES = _lib.LIBRARIES
    assert sorted(lib.name for lib in LIBRARIES) == sorted(LABELS) and len(LIBRARIES) == 13
    assert LIBRARIES[0] is _lib.LIB and _lib.LIB.path == _lib.LIB_PATH and _lib.LIB.signatures is _lib.SIGNATURES
    for k, lib in enumerate(LIBRARIES):
        assert all(a in LIBRARIES[:k] for a in lib.after), lib.name
    assert _jpegdec_unmarked_lib.LIB is _library("mdct_jpegdec_unmarked") and _jpegdec_unmarked_lib.load == _jpegdec_unmarked_lib.LIB.load
    assert api.MdctError is _lib.MdctError


@pytest.mark.parametrize("name", sorted(LABELS))
def test_every_library_reports_under_its_label(name, built):
    """every library, the one without a device-free wrapper included: the text error(rc) gives is the label of the table, the status
    and the C library's last message"""
    lib = _library(name)
    assert lib.label == LABELS[name]
    e = lib.error(7)
    assert isinstance(e, api.MdctError) and str(e) == f"{LABELS[name]} status 7: {lib.last_error()}"
    lib.check(0)
    with pytest.raises(api.MdctError, match=f"^{LABELS[name]} status 3: "):
        lib.check(3)


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(mdct_[a-z0-9_]+)\s*\(", txt)))


# what the tests of single libraries asked of their headers: (at least this many functions, every one with this prefix)
DECLARED_AT_LEAST = {"mdct_hip": (20, "mdct_"), "mdct_jpegdec_batch": (10, "mdct_jpegdec_batch_"), "mdct_jpegenc_batch": (10, "mdct_jpegenc_batch_")}


@pytest.mark.parametrize("name", sorted(LABELS))
def test_every_declared_symbol_is_exported_and_bound(name, built):
    """(a) the mdct_* functions the library's headers declare are its SIGNATURES, and the built library exports every one"""
    lib = _library(name)
    names = [n for h in lib.headers for n in _declared(h)]
    at_least, prefix = DECLARED_AT_LEAST.get(name, (2, "mdct_"))
    assert len(names) >= at_least and all(n.startswith(prefix) for n in names)
    handle = lib.load()
    for n in names:
        assert hasattr(handle, n), f"{n} declared in include/ but not exported"
        assert n in lib.signatures, f"{n} has no ctypes signature"
    for n in lib.signatures:
        assert n in names, f"{n} bound but not declared in include/"
    exported = ctypes.CDLL(lib.path)
    for n in names:
        assert getattr(exported, n)


def test_the_batch_encoders_row_limit_is_the_headers():
    src = open(os.path.join(ROOT, "include", "mdct_jpegenc_batch.h")).read()
    assert f"#define MDCT_JPEGENC_BATCH_MAX_ROWS {_jpegenc_batch_lib.MAX_ROWS}\n" in src


@pytest.mark.parametrize("name", sorted(LABELS))
def test_linked_against_what_the_binding_loads_first(name, built):
    """(b) the Makefile's link list of the library and the loader's order say the same: its NEEDED libmdct_* entries are libmdct_hip.so
    (but for libmdct_hip.so itself) and the libraries of `after`"""
    lib = _library(name)
    out = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-d", lib.path], check=True, capture_output=True, text=True).stdout
    needed = set(re.findall(r"\(NEEDED\)\s+Shared library: \[(libmdct_[^\]]+)\]", out))
    want = {"lib" + a.name + ".so" for a in lib.after} | ({"libmdct_hip.so"} if lib is not _lib.LIB else set())
    assert needed == want


def test_the_built_libraries_are_the_registered_ones(built):
    """(c) after build(): every libmdct_*.so in the package has a binding, every binding a library"""
    assert sorted(glob.glob(os.path.join(ROOT, "simd_dct_amd", "libmdct_*.so"))) == sorted(lib.path for lib in _lib.LIBRARIES)
