"""tests/poisoned_alloc.py on CPU tensors (devices=("cpu",)): a result that depends on what torch.empty held is reported, a write past a
tensor's end is reported with its site, a function that writes all it reads passes; and simd_dct_amd/*.py request uninitialised device
memory in the one spelling the harness replaces."""
import ast
import ctypes
import glob
import os

import pytest

from poisoned_alloc import GUARD, PATTERNS, ROUND, GuardChanged, expected_bytes, poisoned, under_patterns

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = ("cpu",)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


# ------------------------------------------------------------------------------------------ toys
def sums_what_it_did_not_write(n=100):
    """writes the first half of its buffer and sums all of it"""
    buf = torch.empty((n,), dtype=torch.int32, device="cpu")
    buf[:n // 2] = 1
    return buf.to(torch.int64).sum()


def writes_one_byte_past_its_tensor(n=1000):
    buf = torch.empty(n, dtype=torch.uint8, device=torch.device("cpu"))
    ctypes.memset(buf.data_ptr(), 3, n + 1)
    return buf.sum()


def writes_all_it_reads(shape=(7, 33)):
    out = torch.empty(shape, dtype=torch.int16)
    counts = torch.empty(*shape, dtype=torch.int64, device="cpu")
    counts.zero_()
    out.copy_(counts + 5)
    return out * 2


def test_a_sum_over_unwritten_words_differs_between_patterns():
    a, b = [], []
    for pattern, got in (("00", a), ("7f", b)):
        with poisoned(pattern, devices=CPU):
            got.append(sums_what_it_did_not_write())
    assert int(a[0]) == 50 and int(b[0]) == 50 + 50 * 0x7F7F7F7F
    problems = under_patterns(sums_what_it_did_not_write, same, devices=CPU)
    assert len(problems) == 3 and all("differs from pattern 00's" in p for p in problems), problems
    assert [p.split()[2] for p in problems] == ["ff", "7f", "rnd"]
    problems = under_patterns(sums_what_it_did_not_write, same, devices=CPU, truth=torch.tensor(50))
    assert len(problems) == 3 and all("differs from the truth" in p for p in problems), problems


def test_a_write_past_the_tensor_is_reported_with_its_site():
    line = writes_one_byte_past_its_tensor.__code__.co_firstlineno + 1
    for pattern in PATTERNS:
        with pytest.raises(GuardChanged) as e:
            with poisoned(pattern, seed=5, devices=CPU):
                writes_one_byte_past_its_tensor()
        text = str(e.value)
        assert f"test_poisoned_alloc.py:{line}" in text and "1000 bytes" in text and "byte 1000 (0 past its end)" in text and "to 0x03" in text, text
    # not strict: the damage is there to read, the outcome too
    with poisoned("ff", devices=CPU, strict=False) as p:
        got = writes_one_byte_past_its_tensor()
    assert int(got) == 3000 and len(p.damage) == 1 and "changed from 0xff to 0x03" in p.damage[0]
    assert len(under_patterns(writes_one_byte_past_its_tensor, same, devices=CPU)) == 4
    # a write into the last byte of the guard, and one just past the rounding slack
    for at in (1024 + GUARD - 1, 1024):
        with pytest.raises(GuardChanged, match=f"byte {at} "):
            with poisoned("rnd", devices=CPU) as p:
                torch.empty(1000, dtype=torch.uint8)
                p.blocks[0][0][at] ^= 0x80


def test_a_function_that_writes_all_it_reads_passes():
    truth = writes_all_it_reads()
    assert under_patterns(writes_all_it_reads, same, devices=CPU, truth=truth) == []
    assert under_patterns(writes_all_it_reads, same, devices=CPU) == []


def test_what_the_harness_hands_out():
    real = torch.empty
    with poisoned("rnd", seed=9, devices=CPU) as p:
        assert torch.empty is not real
        a = torch.empty((3, 5), dtype=torch.int16, device="cpu")
        b = torch.empty(0, dtype=torch.int64)
        c = torch.empty(513, dtype=torch.uint8)
        out = torch.zeros(4)
        assert torch.empty(4, out=out) is out and len(p.blocks) == 3  # out= goes to the real torch.empty
        assert torch.empty(4, device="meta").device.type == "meta" and len(p.blocks) == 3  # as does another device
        assert (a.shape, a.dtype, a.is_contiguous()) == ((3, 5), torch.int16, True) and b.numel() == 0
        assert [blk.numel() for blk, _, _ in p.blocks] == [ROUND + GUARD, GUARD, 2 * ROUND + GUARD] and [n for _, n, _ in p.blocks] == [30, 0, 513]
        assert all(blk.data_ptr() == t.data_ptr() for (blk, _, _), t in zip(p.blocks, (a, b, c)) if t.numel())
        for k, (blk, _, _) in enumerate(p.blocks):
            want = bytes((i * 197 + 31 * k + 9) & 255 for i in range(blk.numel()))
            assert bytes(blk.numpy()) == want == bytes(expected_bytes(torch, "rnd", k, 9, blk.numel(), "cpu").numpy())
        assert bytes(a.view(torch.uint8).reshape(-1).numpy()) == bytes((i * 197 + 9) & 255 for i in range(30))
    assert torch.empty is real
    for pattern, byte in (("00", 0), ("ff", 255), ("7f", 127)):
        with poisoned(pattern, devices=CPU):
            assert set(torch.empty(700, dtype=torch.uint8).tolist()) == {byte}
    with poisoned("00"):  # devices = cuda: a CPU request is the real one's
        assert torch.empty(3, device="cpu").untyped_storage().nbytes() == 12
    with pytest.raises(ZeroDivisionError):  # an exception leaves through the context, and torch.empty is restored
        with poisoned("00", devices=CPU):
            1 / 0
    assert torch.empty is real


# ------------------------------------------------------------------------------------------ the spelling the harness relies on
BANNED_ATTRS = {"empty_like", "new_empty", "empty_strided", "new_empty_strided", "empty_permuted", "empty_quantized", "new"}
LEGACY = {"Tensor", "ByteTensor", "CharTensor", "ShortTensor", "IntTensor", "LongTensor", "HalfTensor", "FloatTensor", "DoubleTensor", "BoolTensor", "BFloat16Tensor"}


def empty_lint(source):
    """-> ["line: what"] for every way of asking for uninitialised memory other than a call spelt torch.empty( ... ); numpy's empty is host memory"""
    found, tree = [], ast.parse(source)
    called = {id(n.func) for n in ast.walk(tree) if isinstance(n, ast.Call)}
    for node in ast.walk(tree):
        if isinstance(node, ast.Attribute):
            if node.attr in BANNED_ATTRS:
                found.append(f"{node.lineno}: {ast.unparse(node)}")
            elif node.attr in LEGACY and id(node) in called:
                found.append(f"{node.lineno}: {ast.unparse(node)}(")
            elif node.attr == "empty" and getattr(node.value, "id", None) not in ("np", "numpy") and not (id(node) in called and isinstance(node.value, ast.Name) and node.value.id == "torch"):
                found.append(f"{node.lineno}: {ast.unparse(node)} is not a call of torch.empty")
        elif isinstance(node, ast.ImportFrom) and node.module and node.module.split(".")[0] == "torch" and any(a.name in BANNED_ATTRS | LEGACY | {"empty"} for a in node.names):
            found.append(f"{node.lineno}: from {node.module} import {', '.join(a.name for a in node.names)}")
        elif isinstance(node, ast.Import) and any(a.name == "torch" and a.asname not in (None, "torch") for a in node.names):
            found.append(f"{node.lineno}: torch imported under another name")
    return found


def test_the_lint_bites():
    bad = ("import torch\nimport torch as th\nfrom torch import empty\n"
           "def f(x):\n    a = torch.empty(3, device=x.device)\n    b = torch.empty_like(x)\n    c = x.new_empty((2,))\n    d = torch.empty_strided((2,), (1,))\n"
           "    e = torch.Tensor(4)\n    g = torch.cuda.ByteTensor(5)\n    make = torch.empty\n    h = th.empty(3)\n    i = x.new(3)\n    return torch.zeros(2), isinstance(x, torch.Tensor)\n")
    assert [p.split(": ", 1)[1] for p in sorted(empty_lint(bad), key=lambda p: int(p.split(":")[0]))] == [
        "torch imported under another name", "from torch import empty", "torch.empty_like", "x.new_empty", "torch.empty_strided", "torch.Tensor(", "torch.cuda.ByteTensor(",
        "torch.empty is not a call of torch.empty", "th.empty is not a call of torch.empty", "x.new"]
    assert empty_lint("import torch\ndef f(n, dev):\n    return [torch.empty((n,), dtype=torch.uint8, device=dev) for _ in range(3)]\n") == []


def test_uninitialised_device_memory_is_requested_only_as_torch_empty():
    files = sorted(glob.glob(os.path.join(ROOT, "simd_dct_amd", "*.py")))
    assert len(files) >= 20
    found = {os.path.basename(f): empty_lint(open(f).read()) for f in files}
    assert not any(found.values()), {k: v for k, v in found.items() if v}
    # and the four files the harness is for do use it
    for name in ("jpeg_decode.py", "jpeg_encode.py", "jpeg_transcode.py", "jpeg_progressive.py"):
        assert "torch.empty(" in open(os.path.join(ROOT, "simd_dct_amd", name)).read(), name
