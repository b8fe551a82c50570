"""Every s_barrier of every library waits for the wave's own LDS operations first (csrc/wg_sync.h says why: __syncthreads() may compile
to s_barrier without s_waitcnt lgkmcnt(0), and a ds_write still queued when its wave passes the barrier can be overtaken by what a
wave of another SIMD issues after it).  CPU only: nothing here runs a kernel.

Which assembly: each library's gfx950 code objects are unbundled as test_kernel_coverage.code_object_kernels does and disassembled
(llvm-objdump -d --symbolize-operands, which gives every branch target inside a function a label <Ln> and prints the label as the
branching instruction's operand).  That is what the GPU runs, it needs no second compile, and the labels are enough for the walk.

The rule, per s_barrier: walk backwards along every path.  A path is settled by an s_waitcnt whose lgkmcnt is 0; it fails at an LDS
memory instruction (ds_read*, ds_write*, ds_load*, ds_store*, the ds_ atomics; ds_bpermute / ds_permute / ds_swizzle touch no memory
and are passed over).  The predecessors of an instruction are the one before it and, where a label stands in front of it, every
instruction that names the label as an operand.  The walk takes no instruction for an unconditional jump, so it follows some paths the
hardware never takes: it can refuse a good barrier, never pass a bad one -- as long as every LDS instruction stands in a kernel's own
text: the walk steps over a call, so it would not see what a callee that was not inlined issues.  The test therefore asserts that no
function other than a kernel holds an s_barrier or a ds_ instruction (today every function of every code object is a kernel).  A path that reaches a kernel's entry is settled: a wave
starts with no LDS operation in flight.  A path that reaches the entry of a function that is no kernel is undecided and needs a line
in ALLOW (kernel, the barrier's ordinal in it, a reason); a line no barrier uses fails the test.  Today every barrier is decided by
following the predecessors (one of libmdct_jpegdec_unmarked.so's stands at the head of a block and is undecided inside it), so ALLOW
is empty, and it may never hold more than that one."""
import functools
import os
import re
import struct
import subprocess
import tempfile

import pytest

from test_kernel_coverage import BUNDLE_MAGIC, LLVM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (library, kernel as llvm-objdump names it, ordinal of the barrier in the kernel) -> reason
ALLOW = {}
ALLOW_MAX = 1  # what today's build leaves undecided inside a basic block: one barrier, in libmdct_jpegdec_unmarked.so

NO_MEMORY = ("ds_bpermute", "ds_permute", "ds_swizzle")
LDS_MEMORY = re.compile(r"ds_(read|write|load|store|add|sub|rsub|inc|dec|min|max|and|or|xor|mskor|cmpst|cmpswap|wrxchg|wrap|pk_add|append|consume|condxchg|ordered|gws)")

SYMBOL = re.compile(r"^[0-9a-f]+ <(.+)>:$")
LABEL = re.compile(r"^L\d+$")
LABEL_USE = re.compile(r"\bL\d+\b")


def parse(text):
    """disassembly -> {function: [(mnemonic, operands, labels in front of it)]}"""
    functions, current, pending = {}, None, []
    for line in text.splitlines():
        m = SYMBOL.match(line.strip())
        if m:
            if LABEL.match(m.group(1)):
                pending.append(m.group(1))
            else:
                current, pending = functions.setdefault(m.group(1), []), []
            continue
        code = line.split("//", 1)[0].strip()
        if not code or current is None or not line[:1].isspace():
            continue
        mnemonic, _, operands = code.partition(" ")
        current.append((mnemonic, operands.strip(), tuple(pending)))
        pending = []
    return functions


def waits_for_lds(mnemonic, operands):
    """an s_waitcnt that leaves no LDS (or scalar-memory) operation of the wave in flight"""
    if mnemonic != "s_waitcnt":
        return False
    m = re.search(r"lgkmcnt\((\d+)\)", operands)
    if m:
        return int(m.group(1)) == 0
    if re.fullmatch(r"(0x[0-9a-fA-F]+|\d+)", operands):  # the raw immediate: lgkmcnt is bits 11:8 on gfx9
        return (int(operands, 0) >> 8) & 15 == 0
    return False


def touches_lds(mnemonic):
    return mnemonic.startswith("ds_") and not mnemonic.startswith(NO_MEMORY) and bool(LDS_MEMORY.match(mnemonic))


def walk(instructions, is_kernel=True):
    """-> (barriers, {ordinal: "fails: ..." | "undecided: ..."}) for one function"""
    at = {}
    for i, (_, _, labels) in enumerate(instructions):
        for name in labels:
            at[name] = i
    preds = [set([i - 1]) if i else set() for i in range(len(instructions))]
    for i, (mnemonic, operands, _) in enumerate(instructions):
        for name in LABEL_USE.findall(operands):
            if name in at:
                preds[at[name]].add(i)
    for mnemonic, _, _ in instructions:
        assert not mnemonic.startswith("ds_") or mnemonic.startswith(NO_MEMORY) or touches_lds(mnemonic), f"{mnemonic}: an LDS instruction this test has not classified"
    found, ordinal = {}, 0
    for b, (mnemonic, _, _) in enumerate(instructions):
        if mnemonic != "s_barrier":
            continue
        todo, seen, verdict = list(preds[b]), set(), None
        if not preds[b] and not is_kernel:
            verdict = "undecided: the barrier is the function's first instruction"
        while todo and verdict is None:
            i = todo.pop()
            if i in seen:
                continue
            seen.add(i)
            m, ops, _ = instructions[i]
            if waits_for_lds(m, ops):
                continue
            if touches_lds(m):
                verdict = f"fails: {m} {ops} (instruction {i}) reaches the barrier (instruction {b}) with no s_waitcnt lgkmcnt(0) between them"
            elif not preds[i] and not is_kernel:
                verdict = "undecided: a path reaches the entry of a function that is no kernel"
            todo.extend(preds[i])
        if verdict:
            found[ordinal] = verdict
        ordinal += 1
    return ordinal, found


# ------------------------------------------------------------------------------------------ the walker on hand-written fragments
def fragment(*lines, name="k"):
    return "\n".join([f"0000000000001000 <{name}>:"] + ["\t" + ln if not ln.endswith(":") else ln for ln in lines]) + "\n"


def verdicts(text, is_kernel=True):
    (instructions,) = parse(text).values()
    return walk(instructions, is_kernel)


def test_wait_then_barrier_passes():
    text = fragment("ds_write_b32 v4, v1 offset:6976                // 0000000034C4: D81A1B40 00000104",
                    "s_waitcnt lgkmcnt(0)                           // 0000000034F8: BF8CC07F",
                    "other v1, 0", "s_barrier", "ds_read_b32 v18, v9 offset:6720", "s_waitcnt vmcnt(0) lgkmcnt(0)", "s_barrier")
    assert verdicts(text) == (2, {})
    assert verdicts(fragment("other v1, 0", "s_barrier")) == (1, {})  # nothing before it touches LDS
    assert verdicts(fragment("ds_write_b32 v4, v1", "s_waitcnt 0xc07f", "s_barrier")) == (1, {})  # the immediate, lgkmcnt = 0


def test_a_write_then_barrier_fails():
    n, found = verdicts(fragment("s_waitcnt lgkmcnt(0)", "ds_write_b32 v4, v1 offset:64", "other v1, 0", "s_barrier"))
    assert n == 1 and found[0].startswith("fails: ds_write_b32"), found
    for wait in ("s_waitcnt vmcnt(0)", "s_waitcnt lgkmcnt(1)", "s_waitcnt 0xc17f"):  # waits that leave an LDS operation in flight
        assert verdicts(fragment("ds_write_b32 v4, v1", wait, "s_barrier"))[1], wait
    for op in ("ds_read_b64 v[0:1], v2", "ds_or_b32 v9, v18 offset:6720", "ds_add_rtn_u32 v0, v1, v2", "ds_read2_b32 v[0:1], v2 offset1:1", "ds_write_b8 v0, v1"):
        assert verdicts(fragment(op, "s_barrier"))[1], op


def test_a_write_then_a_permute_then_barrier_fails():
    """ds_bpermute_b32 touches no memory: it neither counts as an access nor hides the write before it"""
    n, found = verdicts(fragment("ds_write_b32 v4, v1 offset:64", "ds_bpermute_b32 v2, v3, v4", "s_barrier"))
    assert n == 1 and found[0].startswith("fails: ds_write_b32"), found
    assert verdicts(fragment("s_waitcnt lgkmcnt(0)", "ds_bpermute_b32 v2, v3, v4", "ds_swizzle_b32 v2, v3 offset:swizzle(SWAP,1)", "s_barrier")) == (1, {})


def test_the_walk_follows_every_predecessor():
    # the barrier heads a block that two paths reach: one waited, the other wrote
    text = fragment("s_waitcnt lgkmcnt(0)", "other vcc, 0, v1", "jump_if L1", "ds_write_b32 v4, v1", "0000000000001010 <L1>:", "s_barrier")
    n, found = verdicts(text)
    assert n == 1 and found[0].startswith("fails: ds_write_b32"), found
    good = fragment("s_waitcnt lgkmcnt(0)", "other vcc, 0, v1", "jump_if L1", "ds_write_b32 v4, v1", "s_waitcnt lgkmcnt(0)", "0000000000001014 <L1>:", "s_barrier")
    assert verdicts(good) == (1, {})
    # a loop: the write after the barrier comes round to it again
    loop = fragment("s_waitcnt lgkmcnt(0)", "0000000000001004 <L0>:", "s_barrier", "ds_write_b32 v4, v1", "jump_if L0")
    assert verdicts(loop)[1][0].startswith("fails: ds_write_b32")
    assert verdicts(fragment("s_waitcnt lgkmcnt(0)", "0000000000001004 <L0>:", "s_barrier", "ds_write_b32 v4, v1", "s_waitcnt lgkmcnt(0)", "jump_if L0")) == (1, {})
    # a function that is no kernel may be entered with LDS operations in flight
    assert verdicts(fragment("other v1, 0", "s_barrier"), is_kernel=False)[1][0].startswith("undecided")


def test_an_allowlist_line_must_be_used():
    text = fragment("other v1, 0", "s_barrier", name="helper")
    instructions = parse(text)
    assert judge("lib", instructions, set(), {("lib", "helper", 0): "entered after wg_sync() only"}) == ({"helper": 1}, [])
    _, problems = judge("lib", instructions, set(), {("lib", "helpr", 0): "misspelt"})
    assert len(problems) == 2 and any("no barrier uses" in p for p in problems) and any("undecided" in p for p in problems), problems
    _, problems = judge("lib", parse(fragment("ds_write_b32 v4, v1", "s_barrier", name="helper")), set(), {("lib", "helper", 0): "a failing barrier is not excused"})
    assert any("fails" in p for p in problems), problems


# ------------------------------------------------------------------------------------------ the libraries
def judge(library, functions, kernels, allow):
    """-> ({function: barriers}, problems)"""
    counts, problems, used = {}, [], set()
    for name, instructions in functions.items():
        n, found = walk(instructions, name in kernels)
        if n:
            counts[name] = n
        for ordinal, verdict in found.items():
            key = (library, name, ordinal)
            if verdict.startswith("undecided") and key in allow:
                used.add(key)
            else:
                problems.append(f"{library} {name} barrier {ordinal} {verdict}")
    problems += [f"ALLOW line {key}: no barrier uses it" for key in allow if key[0] == library and key not in used]
    return counts, problems


def disassembled(lib):
    """-> ({function: instructions}, the kernels' names) over every gfx950 code object in lib's .hip_fatbin"""
    functions, kernels = {}, set()
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fatbin")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, os.path.join(tmp, "lib.copy")], check=True)
        data = open(fat, "rb").read()
        n_objects, pos = 0, 0
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
                    out = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-s", obj], check=True, capture_output=True, text=True).stdout
                    kd = {ln.split()[-1][:-3] for ln in out.splitlines() if ln.strip().endswith(".kd")}
                    text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--symbolize-operands", "--no-show-raw-insn", obj], check=True, capture_output=True, text=True).stdout
                    for name, instructions in parse(text).items():
                        key = name if name not in functions else f"{name} (object {n_objects})"
                        functions[key] = instructions
                        if name in kd:
                            kernels.add(key)
                    n_objects += 1
            pos += len(BUNDLE_MAGIC)
    assert n_objects, f"{lib}: no gfx950 code object"
    return functions, kernels


@functools.lru_cache(None)
def libraries():
    from simd_dct_amd import _lib
    return {lib.name: lib.path for lib in _lib.LIBRARIES}


LIBRARY_NAMES = ("mdct_hip", "mdct_jpegenc_scan", "mdct_jpegenc_opt", "mdct_jpegcoef", "mdct_jpegcolor", "mdct_jpegdec", "mdct_jpegdec_batch", "mdct_jpegdec_prog",
                 "mdct_jpegdec_unmarked", "mdct_jpegenc", "mdct_jpegenc_batch", "mdct_jpegprog", "mdct_jpegscale")


def test_the_libraries_are_the_registry():
    assert tuple(libraries()) == LIBRARY_NAMES and len(ALLOW) <= ALLOW_MAX
    assert all(key[0] == "mdct_jpegdec_unmarked" for key in ALLOW), "only that library has a barrier a walk inside its block leaves undecided"


@pytest.mark.parametrize("name", LIBRARY_NAMES)
def test_every_barrier_waits_for_lds(name):
    path = libraries()[name]
    assert os.path.exists(path), f"{path}: build() makes it"
    functions, kernels = disassembled(path)
    assert kernels, name
    outside = sorted(f for f, instructions in functions.items() if f not in kernels and any(m == "s_barrier" or m.startswith("ds_") for m, _, _ in instructions))
    assert not outside, f"{name}: functions that are no kernels hold barriers or LDS instructions, which a walk inside the calling kernel cannot see: {outside}"
    counts, problems = judge(name, functions, kernels, ALLOW)
    print(f"\nlib{name}.so: {sum(counts.values())} s_barrier in {len(counts)} of {len(functions)} functions ({len(kernels)} kernels)")
    assert not problems, "\n".join(problems)
