"""bench.py's contract, run as the driver runs it (one JSON line on stdout), on small batches."""
import json
import os
import socket
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

BENCH = os.path.join(ROOT, "bench.py")
SMALL = ["--steps", "2", "--warmup", "1", "--reads", "12"]


def _line(cmd, env=None, timeout=600):
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run(cmd, capture_output=True, text=True, env=e, cwd=ROOT, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.split("\n") if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _check_common(d, n_gpus):
    assert d["metric"] == "cytosine sites/sec (CpG+CHG+CHH)" and d["unit"] == "sites/s"
    assert d["n_gpus"] == n_gpus and d["steps"] == 2 and d["warmup"] == 1
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["data"] == "synthetic" and d["dtype"] == "f16x3+f32acc"
    assert "workload" in d["config"] and "model" not in d["config"]
    assert d["value"] > 0 and abs(d["value"] - n_gpus * d["config"]["sites_per_gpu_step"] * 2 / (d["ms_per_step"] * 2e-3)) < 0.35 * d["value"]
    rf = d["roofline"]
    assert rf["bound"] == "mfma" and rf["unit"] == "TFLOP/s" and rf["peak"] == 2500.0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12 and 0 < rf["frac"] < 1 and "traffic" in rf
    # every MFMA kernel's executed rate, and the device's over the wall time (VERDICT r04 #6a)
    bk = rf["by_kernel"]
    assert abs(sum(bk[k]["share_of_device_ms"] for k in ("trunk", "edge", "tail")) - 1) < 1e-9
    for k in ("trunk", "edge", "tail"):
        assert 0 < bk[k]["frac"] < 1 and abs(bk[k]["frac"] - bk[k]["executed"] / rf["peak"]) < 1e-12
    assert abs(bk["trunk"]["frac"] - rf["frac"]) < 1e-12 and 0 < bk["whole_device"]["frac_over_timed_region"] < bk["trunk"]["frac"]
    assert bk["tail"]["strip_tail_passes"] > 0 and 1 <= bk["tail"]["strip_tail_sites_per_pass"] <= 16
    rk = d["ranks"]
    assert rk["world"] == n_gpus and len(rk["sites_per_s"]) == n_gpus and abs(sum(rk["sites_per_s"]) - d["value"]) < 0.1 * d["value"]


def test_bench_line_single_gpu_with_cpu_baseline():
    d = _line([sys.executable, BENCH, "--full"] + SMALL)
    _check_common(d, 1)
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["unit"] == "sites/s" and cb["cores"] >= 1 and cb["value"] > 0 and cb["sample"]
    assert d["parity"]["max_abs_dp_vs_oracle"] <= d["parity"]["tolerance"] == 1e-4
    assert d["parity"]["sites_checked"] > 10000 and "STREAMED" in d["parity"]["sample"]
    rf = d["roofline"]
    assert 0 < rf["utilisation"] < 1 and abs(rf["utilisation"] - rf["frac_executed"]) < 1e-12 and rf["algorithmic_bytes"] > 0
    assert abs(rf["frac"] - rf["frac_executed"]) < 1e-12 and rf["algorithmic"] > rf["achieved"]   # frac is the EXECUTED figure
    # HBM bytes cannot be measured inside the run: `traffic` stays null, the kept PMC pass is quoted under a key of its own
    assert rf["traffic"] is None
    if "traffic_quoted" in rf:
        q = rf["traffic_quoted"]
        assert q["bytes_per_launch"] > rf["algorithmic_bytes"] and q["source"].startswith("profiles/") and q["command"]
    assert d["config"]["group_bases"] >= (1 << 20) and d["config"]["group_bytes"] > 0
    e2e = d["end_to_end"]
    assert "error" not in e2e, e2e
    assert e2e["value"] > 0 and e2e["unit"] == "sites/s" and e2e["reads"] == 72 and e2e["host_threads"] >= 1   # the pool of 3 x 12 reads, twice
    assert e2e["with_flag"]["-Z"]["exit"] == 0
    assert e2e["sites"] > 100000 and "defaults" in e2e["flags"]


def test_bench_plain_run_is_lean_and_dumps_repeatable_outputs(tmp_path):
    """without --full the line carries no leg that takes runs of its own; --dump-outputs writes the last timed step's records
    (float32 / float64 .npy), and two runs with the same arguments write the same arrays"""
    import numpy as np
    dumps = []
    for i in range(2):
        out = tmp_path / f"run{i}"
        d = _line([sys.executable, BENCH, "--dump-outputs", str(out)] + SMALL)
        _check_common(d, 1)
        for k in ("cpu_baseline", "parity", "end_to_end", "resident_slab", "feature_extraction", "fp32_mode"):
            assert k not in d, k
        files = sorted(out.glob("*.npy"))
        assert sum(f.stat().st_size for f in files) <= 64 << 20
        arrays = {f.stem: np.load(f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        n = int(arrays["sites_by_context"].sum())
        assert 0 < n < 2 * d["config"]["sites_per_gpu_step"]   # one step's sites (12-read slabs differ from step to step)
        for k in ("index", "read_id", "qoff", "strand", "ctx", "scaled_prob", "p"):
            assert len(arrays[k]) == n, k   # small slabs: every record of the step
        assert np.array_equal(arrays["index"], np.arange(n)) and ((arrays["p"] >= 0) & (arrays["p"] <= 1)).all()
        assert set(np.unique(arrays["ctx"])) <= {0, 1, 2} and np.all(np.diff(arrays["read_id"]) >= 0)
        dumps.append(arrays)
    assert dumps[0].keys() == dumps[1].keys()
    for k in dumps[0]:
        assert np.array_equal(dumps[0][k], dumps[1][k]), k


def test_bench_rccl_world_of_one():
    """the barrier and the two reductions of the multi-GPU path on RCCL, with one rank"""
    port = _free_port()
    d = _line([sys.executable, BENCH, "--no-cpu-baseline"] + SMALL,
              env={"HM_BENCH_FORCE_DIST": "1", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "RANK": "0",
                   "LOCAL_RANK": "0", "WORLD_SIZE": "1"})
    _check_common(d, 1)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_bench_two_ranks_launched_like_the_driver():
    """`torch.distributed.run --nproc-per-node 2 bench.py --gpus 2`: both ranks share the one card of this box (gloo for
    the reductions, since RCCL refuses two ranks on one device); rank 0 prints the whole-job line"""
    one = _line([sys.executable, BENCH, "--no-cpu-baseline"] + SMALL)
    d = _line([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
               "--master-port", str(_free_port()), BENCH, "--gpus", "2"] + SMALL, env={"HM_DIST_BACKEND": "gloo"})
    _check_common(d, 2)
    assert "cpu_baseline" not in d
    # two different read sets (seed + rank): about twice the sites of one rank
    job_sites = d["value"] * d["ms_per_step"] * 1e-3
    assert 1.5 < job_sites / one["config"]["sites_per_gpu_step"] < 2.5 and job_sites != 2 * one["config"]["sites_per_gpu_step"]


def _plain_env():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["HM_DIST_BACKEND"] = "gloo"
    return env


def test_bench_starts_its_own_ranks():
    """plain `python bench.py --gpus 2` (no torchrun, no WORLD_SIZE): the process launches two ranks itself and rank 0 prints the
    whole-job line with n_gpus = 2 (gloo here: the two ranks share this box's one card)"""
    d = _line([sys.executable, BENCH, "--gpus", "2", "--no-cpu-baseline"] + SMALL, env=_plain_env(), timeout=900)
    _check_common(d, 2)
    rk = d["ranks"]
    assert rk["world"] == 2 and rk["backend"] == "gloo" and rk["rccl_ranks"] == 0 and len(rk["sites_per_s"]) == 2 and min(rk["sites_per_s"]) > 0
    assert abs(max(rk["seconds"]) - d["ms_per_step"] * 2e-3) < 1e-6
    assert "torch.distributed.run" in d["config"]["launch"]


def test_bench_e2e_dist_leg_calls_one_bam_with_queue_ranks():
    """`--e2e-dist`: after the timed region ONE BAM file is called by queue-mode ranks (python -m hifimeth_amd.call_dist), here two
    ranks sharing the one card behind a single bench process (the box allows six processes on its GPU)"""
    d = _line([sys.executable, BENCH, "--no-cpu-baseline", "--no-extras", "--e2e-dist", "--e2e-dist-ranks", "2", "--e2e-reads", "48"] + SMALL,
              env=_plain_env(), timeout=900)
    _check_common(d, 1)
    e = d["end_to_end_dist"]
    assert "error" not in e, e
    assert e["ranks"] == 2 and e["reads_in_file"] == 48 and e["sites"] > 50000 and sum(e["parts_taken_by_rank"]) == 8 and e["value"] > 0


def test_bench_refuses_a_world_that_contradicts_gpus():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1"] + SMALL, capture_output=True, text=True, cwd=ROOT, timeout=300,
                       env=dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port())))
    assert r.returncode != 0 and "WORLD_SIZE" in r.stderr
