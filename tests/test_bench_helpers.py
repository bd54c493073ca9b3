"""The pieces of bench.py and distributed.py that need no GPU -- counter files tied to a build, the
interior / boundary split of a rank's blocks -- and one plain bench.py run on the GPU."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_counter_files_of_another_build_are_refused(tmp_path):
    import bench
    f = tmp_path / "pmc.json"
    f.write_text(json.dumps({"kernel": "panel_kernel<double", "alg_bytes_per_launch": 100, "build": "abc",
                             "traffic_bytes_per_launch": 105}))
    d, why = bench.counter_file(str(f), "abc", kernel="bsm::panel_kernel<double,8,true,false,true>", alg_bytes=100)
    assert d is not None and why is None and d["traffic_bytes_per_launch"] == 105
    d, why = bench.counter_file(str(f), "xyz", kernel="bsm::panel_kernel<double,8,true,false,true>", alg_bytes=100)
    assert d is None and "build" in why
    d, why = bench.counter_file(str(f), "abc", kernel="bsm::panel_kernel<float,8,true,false,true>", alg_bytes=100)
    assert d is None and "kernel" in why
    d, why = bench.counter_file(str(f), "abc", kernel="bsm::panel_kernel<double,8,true,false,true>", alg_bytes=101)
    assert d is None and "bytes" in why
    d, why = bench.counter_file(str(tmp_path / "missing.json"), "abc")
    assert d is None and "no counter file" in why
    # the committed files belong to the committed kernels: same build id as the library reports
    from bsm_amd import _lib
    build = _lib.lib().bsm_version().decode().split("build ")[-1]
    for name in (bench.PMC_FILE, bench.MFMA_FILE):
        if os.path.exists(name):
            assert json.load(open(name))["build"] == build, name + " was taken with another build of the kernels: re-run tools/profile_round.sh"


def test_interior_boundary_split():
    import bsm_amd as bsm
    from bsm_amd import distributed as D
    # symmetric, banded: the boundary blocks of a rank are the off-diagonal blocks that reach into the previous rank
    prob = bsm.synthetic.config5(n=6000, lo=16, hi=96, halfband=3)
    seen_d = seen_o = 0
    for r in range(3):
        local, own, touched = D.split_symmetric(prob, r, 3)
        inner, outer, bt, bx = D.split_interior(local, own)
        seen_d += len(inner["diagonals"]) + len(outer["diagonals"])
        seen_o += len(inner["offdiagonals"]) + len(outer["offdiagonals"])
        for idx in inner["diagonalindices"] + inner["rowindices"] + inner["colindices"]:
            assert own[0] <= idx.min() and idx.max() <= own[1]
        for ri, ci in zip(outer["rowindices"], outer["colindices"]):
            assert not (own[0] <= min(ri.min(), ci.min()) and max(ri.max(), ci.max()) <= own[1])
        if r == 0:
            assert D.is_empty(outer) and bt[1] < bt[0] and bx[1] < bx[0]
        else:
            assert not D.is_empty(outer) and bt[0] < own[0] <= bt[1] and bx == bt  # symmetric: reads what it writes
            assert (bt[0], bt[1]) == (touched[0], max(idx.max() for idx in outer["rowindices"]))
    assert seen_d == len(prob["diagonals"]) and seen_o == len(prob["offdiagonals"])
    # VBCRS with scattered columns: interior = the blocks whose columns the rank owns
    vp = bsm.synthetic.config2(n=8000, nblocks=400)
    total = 0
    for r in range(4):
        local, own = D.split_vbcrs(vp, r, 4)
        inner, outer, bt, bx = D.split_interior(local, own)
        total += len(inner["blocks"]) + len(outer["blocks"])
        for c0, b in zip(inner["colstart"], inner["blocks"]):
            assert own[0] <= c0 and c0 + b.shape[1] - 1 <= own[1]
        for c0, b in zip(outer["colstart"], outer["blocks"]):
            assert c0 < own[0] or c0 + b.shape[1] - 1 > own[1]
        if len(outer["blocks"]):
            assert own[0] <= bt[0] and bt[1] <= own[1]  # they write own rows only, but read beyond
    assert total == len(vp["blocks"])


def test_live_traffic_falls_back_when_the_profiler_is_absent(monkeypatch):
    """bench.live_traffic: no rocprofv3 on the box -> (None, reason); the caller then reads the stamped file"""
    import shutil
    import bench
    monkeypatch.setattr(shutil, "which", lambda name: None)
    d, why = bench.live_traffic("panel_kernel<double, 8, true, false", 54553920)
    assert d is None and "rocprofv3" in why


def test_live_traffic_is_skipped_under_a_profiler(monkeypatch):
    """bench.py started under rocprofv3 (its preload / control variables in the environment) must not start profiler
    children of its own: they would inherit the preload and nest profilers"""
    import shutil
    import bench
    monkeypatch.setattr(shutil, "which", lambda name: "/opt/rocm/bin/rocprofv3")
    for k, v in (("ROCPROFILER_LIBRARY_CTOR", "1"), ("ROCP_TOOL_LIBRARIES", "x"), ("LD_PRELOAD", "/opt/rocm/lib/librocprofiler-sdk-tool.so")):
        monkeypatch.setenv(k, v)
        d, why = bench.live_traffic("panel_kernel<double, 8, true, false", 54553920)
        assert d is None and "profiler" in why and k in why
        monkeypatch.delenv(k)
    assert bench.profiler_in_environment({"LD_PRELOAD": "/usr/lib/libjemalloc.so", "PATH": "/opt/rocm/bin"}) is None


def test_fixture_coo_of_the_bench_is_the_reference_operator():
    """bench.fixture_coo (the parity reference of the BEM legs) against the test suite's own COO product, per element type"""
    import numpy as np
    import bench
    from _common import fixture_problem, scipy_mul, relerr, N
    for tname, dtn, part, tol in bench.BEM_TYPES:
        fx = fixture_problem("cuboid", np.dtype(dtn), part)
        n0 = fx["size"][0]
        rng = np.random.default_rng(3)
        x = rng.standard_normal(n0).astype(np.complex128 if np.dtype(dtn).kind == "c" else np.float64)
        got = bench.fixture_coo(np, fx, n0) @ x
        ref = scipy_mul({k: ([b.astype(x.dtype) for b in v] if k in ("diagonals", "offdiagonals") else v) for k, v in fx.items()},
                        N, x, np.zeros(n0, x.dtype))
        assert relerr(got, ref) < 1e-13, tname


def test_dump_outputs_writes_float_arrays_and_a_seeded_sample_under_the_cap(tmp_path, monkeypatch):
    """bench.dump_outputs (--dump-outputs DIR): float64 / float32 as they are, complex as n x 2 (real, imaginary), and an
    array over its share of DUMP_BYTES as the same seeded sample in every run, with its row indices beside it"""
    import bench
    rng = np.random.default_rng(5)
    y = rng.standard_normal(1000)
    z = (rng.standard_normal(300) + 1j * rng.standard_normal(300)).astype(np.complex64)
    bench.dump_outputs(str(tmp_path / "a"), {"y": y, "z": z})
    got = np.load(tmp_path / "a" / "y.npy")
    assert got.dtype == np.float64 and np.array_equal(got, y)
    gz = np.load(tmp_path / "a" / "z.npy")
    assert gz.dtype == np.float32 and gz.shape == (300, 2)
    assert np.array_equal(gz[:, 0], z.real) and np.array_equal(gz[:, 1], z.imag)
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == ["y.npy", "z.npy"]
    monkeypatch.setattr(bench, "DUMP_BYTES", 4000)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), {"y": y}, share=2)  # 2000 bytes for this rank's one array
    s, idx = np.load(tmp_path / "b" / "y.npy"), np.load(tmp_path / "b" / "y_index.npy")
    assert s.nbytes + idx.nbytes <= 2000 and len(s) == len(idx) > 100 and idx.dtype == np.float64
    assert np.all(np.diff(idx) > 0) and np.array_equal(s, y[idx.astype(np.int64)])
    assert np.array_equal(s, np.load(tmp_path / "c" / "y.npy")) and np.array_equal(idx, np.load(tmp_path / "c" / "y_index.npy"))


def test_bench_refuses_a_step_count_below_one():
    """--steps K is the number of timed steps that ms_per_step divides by: K = 0 is refused before anything runs"""
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--steps" in r.stderr


def test_bench_offers_the_full_run_as_an_option():
    """everything beside the headline sits behind --full: the option exists and is off unless given"""
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--full" in r.stdout


@pytest.mark.gpu
def test_a_plain_bench_run_prints_the_headline_and_nothing_else(tmp_path):
    """bench.py without --full: set-up, warm-up, the K timed steps, --dump-outputs and the result line -- no `extra`
    legs, no CPU baseline, no stream floor or counter passes"""
    import subprocess
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 20 and d["warmup"] == 5 and d["unit"] == "GB/s" and d["dtype"] == "f64" and d["higher_is_better"]
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["config"]["full"] is False
    assert "extra" not in d and "cpu_baseline" not in d and "stream_floor_us" not in d["roofline"]
    y = np.load(out / "y.npy")
    assert y.shape == (100_000,) and np.all(np.isfinite(y))


def test_native_oracle_of_the_cpu_baseline_is_built_outside_the_tree(oracle):
    """bench.native_oracle (the -O3 -march=native oracle the CPU baseline times) compiles in a temporary directory -- the
    tree the benchmark runs from may be read-only -- and computes what the test oracle computes"""
    import bench
    import bsm_amd as bsm
    from _common import N, oracle_mul, relerr
    here = os.path.join(ROOT, "oracle")
    before = sorted(os.listdir(here))
    fast = bench.native_oracle()
    assert sorted(os.listdir(here)) == before
    prob = bsm.synthetic.config2(n=3000, nblocks=150)
    y0 = np.zeros(prob["size"][0])
    assert relerr(oracle_mul(fast, prob, N, prob["x"], y0), oracle_mul(oracle, prob, N, prob["x"], y0)) < 1e-13


def test_the_timed_region_is_exactly_the_k_steps(monkeypatch):
    """--steps K: the timed region of the N = 1 line (bench.time_k_steps) holds exactly the K steps, once, and
    ms_per_step = its time / K -- a stub plan counts its calls between the two clock reads"""
    import types
    import pytest
    import bench
    clock, calls = {"t": 0.0, "reads": []}, []

    def perf_counter():
        clock["reads"].append(len(calls))
        return clock["t"]

    def plan():  # one step: 1 ms
        calls.append(1)
        clock["t"] += 1e-3

    class Event:
        def __init__(self, enable_timing):
            self.at = None

        def record(self):
            self.at = clock["t"]

        def elapsed_time(self, end):
            return (end.at - self.at) * 1e3

    monkeypatch.setattr(bench, "time", types.SimpleNamespace(perf_counter=perf_counter))
    torch = types.SimpleNamespace(cuda=types.SimpleNamespace(Event=Event))
    K = 37
    wall, dev = bench.time_k_steps(lambda: [plan() for _ in range(K)], lambda: None, torch)
    assert clock["reads"] == [0, K] and len(calls) == K
    assert wall * 1e3 / K == pytest.approx(1.0) and dev == pytest.approx(wall)
