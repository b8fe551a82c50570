"""bench.py's JSON line must stay short enough for the driver to parse (round 5 printed 27 KB and lost its
roofline / cpu_baseline).  The line is built by a pure function from measured figures; this builds it from canned
figures of the largest shape a run produces and checks size, syntax and the contract's keys.  The reference's own
harness prints one short row per mode (main.cpp:72-78)."""
import json
import os
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import bench_cpu  # noqa: E402

CONTRACT_KEYS = ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline"]
ROOFLINE_KEYS = ["bound", "achieved", "peak", "unit", "frac", "traffic"]
CPU_KEYS = ["value", "unit", "cores", "kind", "sample"]


def canned(world=1):
    k = {"ms": 0.0296, "GBps": 4534.4, "frac": 0.5668, "fvf": 0.823, "clock_GHz": 1.792, "ok": True}
    stat = {"median": 3772.9, "iqr": 640.7, "min_time": 4212.3, "runs": 40, "threads": 16, "pinned": 16}
    m = {"wall_s": 0.000880, "kernel_ms": 0.04321, "steps": 20, "warmup": 5, "world": world, "verified": True, "device": "gfx950:sramecc+:xnack-",
         "cold_first_launch_ms": 1.234, "from_idle_20_launch_ms": 0.0631, "traffic": 268583339, "traffic_round": 6, "copy_GBps": 6301.2,
         "kernels": {n: dict(k) for n in ("q32", "stereo_sse", "stereo_scalar", "encq_sse", "encq_scalar", "cfg3_u8_frame", "cfg3_i16_frame", "cfg3_q32_frame",
                                          "cfg4_256_planes", "cfg5_f32", "copy", "fwd_i16", "inv_i16")},
         "cpu_baseline": {"value": 5462.8, "unit": "Mpixels/s", "cores": 16, "kind": "port",
                          "sample": "orc_roundtrip_i16 (scalar C, -O2 -ffp-contract=off), 16 threads, 65562 Mpx of 8192x64 int16 stripes in 12.0 s",
                          "reference_q32": {"kind": "reference", "unit": "Mpixels/s", "cpu": "AMD EPYC 9575F 64-Core Processor", "affinity_cpus": 128, "cgroup_cpu_quota": 16.0,
                                            "one_pinned_core": dict(stat, threads=1, pinned=1), "all_host_threads": dict(stat)}},
         "extras_file": "bench_extras.json"}
    if world > 1:
        m.update(ranks_seen=world, backend="rccl", per_rank_Mpx_s=[1512345.6] * world,
                 allgather={"seconds_per_batch": {"compute_only": 0.00123, "gather_only": 0.0456, "pipelined": 0.0461}, "busbw_GBps_gather_only": 312.4,
                            "busbw_frac_of_xgmi_ceiling": 0.292, "gathered_checksums_match_owners": True})
    return m


@pytest.mark.parametrize("world", [1, 2, 8])
def test_line_is_short_and_complete(world):
    line, text = bench.build_line(canned(world))
    assert "\n" not in text and len(text) <= bench.LINE_LIMIT < 6000
    back = json.loads(text)
    assert back == json.loads(json.dumps(line))
    for k in CONTRACT_KEYS:
        assert k in back, k
    for k in ROOFLINE_KEYS:
        assert k in back["roofline"], k
    assert back["roofline"]["bound"] == "hbm" and back["roofline"]["peak"] == 8000.0
    assert abs(back["roofline"]["frac"] - back["roofline"]["achieved"] / 8000.0) < 1e-3
    assert "workload" in back["config"] and "model" not in back["config"]
    for k in CPU_KEYS:
        assert k in back["cpu_baseline"], k
    assert back["n_gpus"] == world and back["steps"] == 20 and back["warmup"] == 5
    assert back["vs_baseline"] is None and back["higher_is_better"] is True and back["scaling"] == "weak"
    for k in ("cold_first_launch_ms", "from_idle_20_launch_ms", "steady_ms"):
        assert isinstance(back["cold"][k], float)
    # value = whole-job pixels / wall time
    assert back["value"] == pytest.approx(world * 8192 * 8192 * 20 / 0.000880 / 1e6, rel=1e-6)
    if world > 1:
        assert back["ranks_seen"] == world and "rccl_ranks_seen" not in back and back["backend"] == "rccl"
    # every per-kernel entry is numbers (and one flag) only
    for name, e in back["kernels"].items():
        assert all(isinstance(v, (int, float, bool)) or v is None for v in e.values()), name


def test_oversized_optional_blocks_are_dropped_not_the_line():
    m = canned(8)
    m["kernels"] = {f"kernel_{i}": {"ms": 0.1, "note": "x" * 200} for i in range(40)}
    line, text = bench.build_line(m)
    assert len(text) <= bench.LINE_LIMIT
    back = json.loads(text)
    assert back["kernels"] == {"see": "bench_extras.json"} and "roofline" in back and "cpu_baseline" in back


def test_gpus_n_without_world_size_starts_a_child_and_relays_its_line(monkeypatch, capsys):
    """`python bench.py --gpus N` (the driver's form) must launch torch.distributed.run itself -- as a child process, never exec"""
    seen = {}
    child_line = json.dumps({"metric": bench.METRIC, "value": 1.0, "n_gpus": 2})

    def fake_run(cmd, **kw):
        seen["cmd"], seen["kw"] = cmd, kw
        return types.SimpleNamespace(returncode=0, stdout="NCCL version banner\n" + child_line + "\n")

    monkeypatch.setattr(bench.subprocess, "run", fake_run)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2", "--steps", "20", "--warmup", "5", "--backend", "gloo"])
    monkeypatch.setattr(bench.os, "execv", lambda *a: pytest.fail("exec from the launcher"), raising=False)
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 0
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node=2" in cmd and "127.0.0.1" in cmd
    assert cmd[-7:] == ["--gpus", "2", "--steps", "20", "--warmup", "5", "--backend", "gloo"][-7:] and os.path.basename(cmd[cmd.index("--gpus") - 1]) == "bench.py"
    out = capsys.readouterr().out.strip().splitlines()
    assert out[-1] == child_line and len(out) == 1


def test_child_failure_is_the_launchers_exit_code(monkeypatch, capsys):
    monkeypatch.setattr(bench.subprocess, "run", lambda cmd, **kw: types.SimpleNamespace(returncode=17, stdout=""))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 17 and capsys.readouterr().out == ""


def test_cpu_statistics_are_median_and_iqr():
    s = bench_cpu.summarise([1.0 / r for r in (10, 20, 30, 40, 50, 60, 70, 80)], 1e6)  # rates 10..80 Mpx/s
    assert s["runs"] == 8 and s["min_time"] == 80.0 and s["median"] == 45.0 and s["iqr"] > 0


def test_mt_timing_harness_transforms_the_whole_plane():
    """oracle/time_mt.c (the cpu_baseline's clock): N pinned threads over disjoint startY/endY ranges == one whole-plane call"""
    import ctypes

    import numpy as np

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle as O
    from simd_dct_amd import synth
    from simd_dct_amd.api import QUANTIZE_BASE

    Wd, Hd = 512, 256
    lib = O.oracle()
    img = np.ascontiguousarray(synth.plane_u8_np(Wd, Hd, "photo").reshape(-1))
    lut = np.ascontiguousarray((QUANTIZE_BASE * np.float32(2000)).astype(np.float32))
    want = np.full(Wd * Hd, 7, dtype=np.uint8)
    O.run_behaviour("q32_avx", img, lut, Wd, 2 * Hd, 0, 2 * Hd, out=want)
    cpus = sorted(os.sched_getaffinity(0))
    pin = (ctypes.c_int * len(cpus))(*cpus)
    for nthreads in (1, 3, 40):  # 40 > 32 block rows: some threads own nothing
        got = np.full(Wd * Hd, 7, dtype=np.uint8)
        sec = (ctypes.c_double * 4)()
        rc = lib.orc_time_q32_mt(ctypes.cast(lib.orc_q32_avx, ctypes.c_void_p), -1, img.ctypes.data, got.ctypes.data, lut.ctypes.data_as(O.f32p), Wd, Hd, nthreads, pin, len(cpus), 1, 4, sec)
        assert rc == nthreads and np.array_equal(got, want) and all(s > 0 for s in sec)
    assert lib.orc_time_q32_mt(None, -1, img.ctypes.data, want.ctypes.data, lut.ctypes.data_as(O.f32p), Wd, Hd, 1, pin, len(cpus), 1, 4, sec) == -1


def test_dump_sample_is_fixed_in_bounds_and_small(tmp_path):
    """--dump-outputs: the same positions in every run, all inside the plane, one per stride, and at most 64 MB as float32"""
    import numpy as np

    n = bench.W * bench.H
    idx = bench.dump_sample_index(n)
    assert np.array_equal(idx, bench.dump_sample_index(n))
    assert idx.size == bench.DUMP_SAMPLES and idx.min() >= 0 and idx.max() < n
    assert np.array_equal(idx // (n // bench.DUMP_SAMPLES), np.arange(idx.size))
    assert idx.size * 4 <= 64 * 2**20
    plane = np.arange(n, dtype=np.int16)
    bench.dump_outputs(str(tmp_path / "out"), {"roundtrip_i16": plane[idx].astype(np.float32)})
    back = np.load(tmp_path / "out" / "roundtrip_i16.npy")
    assert back.dtype == np.float32 and np.array_equal(back, plane[idx].astype(np.float32))
