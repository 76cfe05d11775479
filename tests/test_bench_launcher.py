"""CPU suite: `python bench.py --gpus N` starts its own N ranks (bench.py launch_ranks) -- against a stub rank
(tests/helpers/stub_rank.py) that checks the environment it is given and meets the other ranks over the host transport."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = "%s %s" % (sys.executable, os.path.join(ROOT, "tests", "helpers", "stub_rank.py"))


def _bench(args, **env):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "RAFTX_COMM_TOKEN")}
    e.update(env)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=e, capture_output=True, text=True, timeout=120)


def test_gpus_n_starts_n_ranks_without_a_launcher():
    r = _bench(["--gpus", "3", "--steps", "2"], RAFTX_BENCH_RANK_CMD=STUB)
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout                       # rank 0 alone owns stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 3 and out["sum"] == 6.0 and out["argv"] == ["--gpus", "3", "--steps", "2"]


def test_a_failing_rank_stops_the_job_with_its_exit_code():
    t0 = time.time()
    r = _bench(["--gpus", "2"], RAFTX_BENCH_RANK_CMD=STUB, STUB_MODE="fail")
    assert r.returncode == 3 and "rank 1 exited with code 3" in r.stderr
    assert time.time() - t0 < 30                           # rank 0 (sleeping) was terminated, not waited for


def test_gpus_must_match_the_world_an_external_launcher_made():
    r = _bench(["--gpus", "8"], WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    assert r.returncode == 2 and "--gpus 8 but WORLD_SIZE=2" in r.stderr
    r = _bench(["--gpus", "1"], WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    assert r.returncode == 2


def test_more_gpus_than_the_host_has_fails_loudly():
    r = _bench(["--gpus", "2"])                            # this container has no GPU at all
    assert r.returncode == 2 and "GPU(s) visible" in r.stderr


import pytest  # noqa: E402


@pytest.mark.gpu
def test_two_ranks_on_one_gpu_through_bench_itself():
    """`python bench.py --gpus 2` with no launcher around it, both ranks on device 0 (RAFTX_BENCH_DEVICE=0: RCCL refuses two
    ranks on one device, the exchange steps take the host transport and the line says so): two ranks are started, the
    statistics of both are gathered inside the timed steps, rank 0 prints ONE line that says n_gpus = 2 and carries the
    per-rank / gather / single-rank keys."""
    r = _bench(["--gpus", "2", "--steps", "3", "--warmup", "1", "--designs", "512", "--no-cpu-baseline", "--full"], RAFTX_BENCH_DEVICE="0")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and r.stdout.strip().splitlines()[-1] == lines[0], r.stdout[-500:]     # the JSON line is the LAST line
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["designs_per_gpu"] == 512
    assert "host-tcp" in out["config"]["gather"]
    assert len(out["per_rank_ms"]["all"]) == 2 and out["gather_ms"]["rank0"] >= 0.0
    assert 0.2 < out["scaling_efficiency"] < 1.2 and out["single_rank_same_invocation"]["value"] > 0
    assert out["parity"]["niter_mismatches_vs_reference"] == 0
    # N > 1 weak line ALSO carries configs[2]'s literal shape: ONE sweep of --designs cut into N shards, same invocation
    st = out["strong_same_invocation"]
    assert st["scaling"] == "strong" and st["shard_designs"] == [256, 256] and st["total_designs"] == 512
    assert abs(st["value"] - 512 * out["config"]["nw"] / (st["ms_per_step"] * 1e-3)) < 1e-6 * st["value"]


@pytest.mark.gpu
def test_single_gpu_line_carries_the_numbers_a_reader_needs():
    """beside `value` the line has the step-level roofline fraction, SURVEY 8d's literal step (responses
    downloaded) as a top-level key, and the 1/8 shard of the sweep (what one rank of an 8-GPU strong-scaling run does)."""
    r = _bench(["--steps", "4", "--warmup", "1", "--designs", "2048", "--no-cpu-baseline", "--legs", "xi,shard", "--full"],
               RAFTX_BENCH_XI_STEPS="6")
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    rf = out["roofline"]
    assert 0 < rf["step_frac"] <= rf["frac"] < 1 and rf["kernel_ms_per_step"] <= out["ms_per_step"]
    assert abs(rf["step_frac"] - rf["algorithmic_flops_per_step"] / (out["ms_per_step"] * 1e-3) / 1e12 / rf["peak"]) < 1e-9
    assert out["value_xi_out"] == out["xi_out"]["streamed_dcf_per_s"] > 0
    sh = out["shard_1250"]
    assert sh["designs_per_step"] == 256 and sh["ms_per_step"] > 0
    assert abs(sh["projected_8_gpu_strong_speedup"] - out["ms_per_step"] / sh["ms_per_step"]) < 1e-9


@pytest.mark.gpu
def test_sharded_qtf_workload_through_bench_itself():
    """--workload c5 with two ranks on one GPU: rows of every QTF interleaved over the ranks, one SUM-reduce onto rank 0; the
    reduced matrices are Hermitian and finite (asserted inside), the line carries both ranks' kernel times."""
    r = _bench(["--gpus", "2", "--workload", "c5", "--steps", "2", "--sets", "2"], RAFTX_BENCH_DEVICE="0")
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["n_gpus"] == 2 and out["scaling"] == "strong" and out["hermitian"] is True
    assert len(out["per_rank_ms"]["qtf_kernels"]) == 2


@pytest.mark.gpu
def test_strong_scaling_mode_cuts_one_sweep_into_ragged_shards():
    """--scaling strong: ONE sweep of --designs cut into N contiguous shards (1001 over 3 ranks = 334 + 334 + 333),
    gathered with ragged counts inside the timed steps; the line says "strong", names the shards and carries every rank's
    descriptor-expansion time."""
    r = _bench(["--gpus", "3", "--scaling", "strong", "--designs", "1001", "--steps", "3", "--warmup", "1", "--no-cpu-baseline",
                "--full"], RAFTX_BENCH_DEVICE="0")
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["n_gpus"] == 3 and out["scaling"] == "strong"
    assert out["config"]["shard_designs"] == [334, 334, 333] and out["config"]["total_designs"] == 1001
    assert abs(out["value"] - 1001 * out["config"]["nw"] / (out["ms_per_step"] * 1e-3)) < 1e-6 * out["value"]
    assert len(out["host_descriptor_ms_per_rank"]["all"]) == 3
    assert out["parity"]["niter_mismatches_vs_reference"] == 0


def test_dump_outputs_writes_float64_within_its_budget(tmp_path, monkeypatch):
    """--dump-outputs: float64 files, complex arrays split in two, and where the whole would pass the budget the same
    seeded sample of designs in every file (named by design_index.npy), identical from call to call."""
    import numpy as np
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    std = np.arange(40 * 6, dtype=np.float64).reshape(40, 1, 6)
    niter = np.arange(40, dtype=np.int32).reshape(40, 1)
    Xi = (np.arange(40 * 12) * (1 + 2j)).reshape(40, 1, 1, 6, 2)
    assert bench.dump_outputs(str(tmp_path / "a"), {"std": std, "niter": niter, "Xi": Xi}) == ["Xi_im", "Xi_re", "niter", "std"]
    got = {n: np.load(str(tmp_path / "a" / (n + ".npy"))) for n in ("std", "niter", "Xi_re", "Xi_im")}
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["std"], std) and np.array_equal(got["niter"], niter) and np.array_equal(got["Xi_im"], Xi.imag)
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 10 * 7 * 8)             # room for about a quarter of the designs
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), {"std": std, "niter": niter})
    idx = np.load(str(tmp_path / "b" / "design_index.npy")).astype(int)
    assert 0 < len(idx) < 40 and np.all(np.diff(idx) > 0)
    for n in ("std", "niter", "design_index"):
        b, c = np.load(str(tmp_path / "b" / (n + ".npy"))), np.load(str(tmp_path / "c" / (n + ".npy")))
        assert np.array_equal(b, c)
    assert np.array_equal(np.load(str(tmp_path / "b" / "std.npy")), std[idx])
    assert sum(os.path.getsize(str(p)) for p in (tmp_path / "b").iterdir()) < 10 * 7 * 8 + 3 * 256        # + .npy headers


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone_and_its_outputs_repeat(tmp_path):
    """A plain run times exactly --steps steps and carries none of the --full legs; --dump-outputs writes the last timed
    step's statistics, and a second run with the same arguments writes the same bits."""
    import numpy as np
    outs = []
    for d in ("one", "two"):
        r = _bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--designs", "512", "--dump-outputs", str(tmp_path / d)])
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1 and r.stdout.strip().splitlines()[-1] == lines[0], r.stdout[-500:]
        outs.append(json.loads(lines[0]))
    for out in outs:
        assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["unit"] == "dcf solves/s" and out["dtype"] == "f64"
        assert abs(out["value"] - 512 * out["config"]["nw"] / (out["ms_per_step"] * 1e-3)) < 1e-6 * out["value"]
        assert not {"cpu_baseline", "xi_out", "isolated_call", "featured_sweeps", "shard_1250", "c2_dropin"} & set(out)
    std = np.load(str(tmp_path / "one" / "std.npy"))
    assert std.shape == (512, 1, 6) and std.dtype == np.float64 and np.all(np.isfinite(std)) and np.all(std > 0)
    for n in ("std", "niter", "flags", "strips_per_design"):
        a, b = np.load(str(tmp_path / "one" / (n + ".npy"))), np.load(str(tmp_path / "two" / (n + ".npy")))
        assert a.dtype == np.float64 and np.array_equal(a, b), n
