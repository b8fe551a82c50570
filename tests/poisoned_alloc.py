"""poisoned(pattern): while it is active, what torch.empty hands out on the device holds a chosen pattern, and lies between canaries.

simd_dct_amd/jpeg_decode.py, jpeg_encode.py, jpeg_transcode.py and jpeg_progressive.py request all their uninitialised device memory
as `torch.empty(` -- the attribute of the torch module (test_poisoned_alloc.py holds them to that spelling).  The context manager
replaces that attribute.  A call that asks for a tensor on one of `devices` is served from a larger uint8 block: the request rounded
up to 512 bytes (the code's comments rely on the caching allocator's 512-byte blocks) plus a 512-byte guard.  The whole block is
filled with the pattern on the current stream, so under api._on_stream the fill is ordered before the call's kernels, and the tensor
returned is the view of the block's first bytes with the requested dtype and shape.  Everything else goes to the real torch.empty:
other devices, out=, pin_memory=.  Every block stays alive until the context ends, so no request is served from memory a poisoned
request of the same context gave back.  On exit the device is synchronised and every block's tail -- the rounding slack and the
guard -- must still hold the pattern: a changed byte names the allocation's site (file and line of the caller), its size and the
first changed offset.

Patterns: "00" (a stale OK or empty), "ff" (marker prefixes in byte buffers, -1 in counts), "7f" (large positive counts and offsets),
"rnd": byte i of the k-th allocation's block is (i * 197 + 31 * k + seed) & 255, which the tail check regenerates."""
import contextlib
import math
import os
import sys

PATTERNS = ("00", "ff", "7f", "rnd")
ROUND = GUARD = 512
_HERE = os.path.abspath(__file__)


class GuardChanged(AssertionError):
    pass


def expected_bytes(torch, pattern, k, seed, n, device):
    """bytes 0 .. n - 1 of the k-th block; n is a multiple of 256"""
    if pattern != "rnd":
        return torch.full((n,), int(pattern, 16), dtype=torch.uint8, device=device)
    base = (torch.arange(256, dtype=torch.int64, device=device) * 197 + 31 * k + seed) & 255
    return base.to(torch.uint8).repeat(n // 256)


def _site():
    f = sys._getframe(2)
    while f is not None and os.path.abspath(f.f_code.co_filename) == _HERE:
        f = f.f_back
    return f"{os.path.relpath(f.f_code.co_filename)}:{f.f_lineno}" if f is not None else "?"


class Poison:
    """what poisoned() yields: .blocks (one entry per served request), .damage (filled by check())"""

    def __init__(self, torch, pattern, seed, devices):
        assert pattern in PATTERNS, pattern
        self.torch, self.pattern, self.seed, self.devices = torch, pattern, seed, tuple(devices)
        self.real = torch.empty
        self.blocks = []  # (block, bytes asked for, site)
        self.damage = []

    def empty(self, *size, **kw):
        torch = self.torch
        device = kw.get("device")
        device = torch.device(device) if device is not None else self.real(0).device
        if device.type not in self.devices or kw.get("out") is not None or kw.get("pin_memory") or kw.get("requires_grad") \
                or kw.get("layout", torch.strided) is not torch.strided or kw.get("memory_format", torch.contiguous_format) is not torch.contiguous_format:
            return self.real(*size, **kw)
        if "size" in kw:
            size = (kw["size"],)
        shape = tuple(size[0]) if len(size) == 1 and not isinstance(size[0], int) else tuple(int(s) for s in size)
        dtype = kw.get("dtype") or torch.get_default_dtype()
        nbytes = math.prod(shape) * self.real(0, dtype=dtype).element_size()
        total = -(-nbytes // ROUND) * ROUND + GUARD
        block = self.real(total, dtype=torch.uint8, device=device)
        block.copy_(expected_bytes(torch, self.pattern, len(self.blocks), self.seed, total, device))
        self.blocks.append((block, nbytes, _site()))
        return block[:nbytes].view(dtype).view(shape)

    def check(self):
        """every block's tail against the pattern -> the damage found (also kept in .damage)"""
        torch, self.damage = self.torch, []
        if any(b.is_cuda for b, _, _ in self.blocks):
            torch.cuda.synchronize()
        for k, (block, nbytes, site) in enumerate(self.blocks):
            want = expected_bytes(torch, self.pattern, k, self.seed, block.numel(), block.device)
            if not torch.equal(block[nbytes:], want[nbytes:]):
                first = nbytes + int(torch.nonzero(block[nbytes:] != want[nbytes:])[0])
                self.damage.append(f"allocation {k} at {site}, {nbytes} bytes under pattern {self.pattern}: byte {first} ({first - nbytes} past its end) "
                                   f"changed from 0x{int(want[first]):02x} to 0x{int(block[first]):02x}")
        return self.damage


@contextlib.contextmanager
def poisoned(pattern, seed=0, devices=("cuda",), strict=True):
    """strict: a changed guard byte raises GuardChanged on exit (after a body that did not raise); otherwise read .damage"""
    import torch
    p = Poison(torch, pattern, seed, devices)
    assert not isinstance(getattr(torch.empty, "__self__", None), Poison), "poisoned() does not nest"
    torch.empty = p.empty
    try:
        yield p
    except BaseException:
        if "cuda" in p.devices and torch.cuda.is_available():
            torch.cuda.synchronize()  # before the blocks are freed: pending kernels never run on memory something else has taken
        raise
    finally:
        torch.empty = p.real
    p.check()
    if strict and p.damage:
        raise GuardChanged("; ".join(p.damage))


def under_patterns(call, same, patterns=PATTERNS, seed=0, devices=("cuda",), truth=None, brief=repr):
    """call() under each pattern -> problems: an outcome that differs from `truth` (default: the first pattern's), a changed guard byte"""
    problems, outcomes = [], {}
    for pattern in patterns:
        with poisoned(pattern, seed=seed, devices=devices, strict=False) as p:
            outcomes[pattern] = call()
        problems += p.damage
    first = patterns[0]
    for pattern in patterns:
        want, name = (truth, "the truth") if truth is not None else (outcomes[first], f"pattern {first}'s")
        if not same(outcomes[pattern], want):
            problems.append(f"under pattern {pattern} the outcome {brief(outcomes[pattern])} differs from {name} {brief(want)}")
    return problems
