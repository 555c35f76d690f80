"""bench.py's command line on a small fleet (GPU): a plain run times `--steps` steps and prints
the headline only; `--full` adds the figures that take runs of their own; `--dump-outputs`
writes the last timed step's outputs, the same from run to run and with or without `--full`.

The fleet: 96 config-3 nodes (192k processes, Z = 4), so the process tables (768k elements)
take the sampled path of bench.dump_ranges and every other table is written whole; the totals
mode is the flagship's (tables)."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--steps", "5", "--warmup", "2", "--nodes", "96", "--totals", "tables"]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY = ("roofline", "cpu_baseline", "scrape_powers", "slot_layouts", "pipeline", "host_path", "host_path_ticks",
             "value_with_scrape")


def _bench(extra, out_dir):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *ARGS, "--dump-outputs", str(out_dir), *extra],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    # one JSON result line, the last (RCCL prints a version banner of its own when it initialises)
    lines = [x for x in p.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1 and p.stdout.rstrip().endswith(lines[0]), p.stdout
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    d = tmp_path_factory.mktemp("plain")
    return _bench([], d), d


@pytest.fixture(scope="module")
def full(tmp_path_factory):
    d = tmp_path_factory.mktemp("full")
    # the CPU baseline and the config-3-sized secondary lines are switched off: seconds each
    return _bench(["--full", "--no-cpu-baseline", "--no-pipeline-line", "--no-host-line"], d), d


def _arrays(d):
    return {n[:-4]: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d)) if n.endswith(".npy")}


def test_plain_run_prints_the_headline_only(plain):
    res, _ = plain
    for k in HEADLINE:
        assert k in res, k
    assert res["steps"] == 5 and res["warmup"] == 2
    assert res["unit"] == "proc-attr/s" and res["higher_is_better"] is True and res["dtype"] == "f64+u64"
    assert res["ms_per_step"] > 0
    # value is the processes of the timed steps over their time: 96 x 2000 per step
    assert res["config"]["procs_per_gpu"] == 96 * 2000
    assert res["value"] == pytest.approx(96 * 2000 / (res["ms_per_step"] * 1e-3), rel=1e-9)
    for k in FULL_ONLY + ("kernel_ms", "kernel_timing"):
        assert k not in res, k


def test_full_run_adds_the_secondary_figures(full):
    res, _ = full
    for k in HEADLINE + ("kernel_ms", "totals_compute_ms", "kernel_timing", "roofline", "scrape_powers",
                         "slot_layouts"):
        assert k in res, k
    assert len(res["kernel_ms_steps"]) == 5
    assert res["kernel_timing"]["step_events"] == "separate"
    assert res["roofline"]["achieved"] > 0
    assert "error" not in res["scrape_powers"] and "error" not in res["slot_layouts"]


def test_dump_outputs_float_arrays_within_budget(plain):
    from kepler_amd import accel

    import bench

    _, d = plain
    arrays = _arrays(d)
    names = [n for n, _ in accel.TABLES] + ["cluster_ns_energy", "cluster_ns_power", "cluster_node_energy",
                                            "cluster_node_power"]
    assert sorted(arrays) == sorted(names)
    assert all(a.dtype == np.float64 and a.ndim == 1 for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 * 1000 * 1000
    Z, N, P = 4, 96, 96 * 2000
    assert arrays["node_power"].size == N * Z and arrays["cluster_node_energy"].size == 2 * Z
    assert arrays["proc_energy"].size == bench.DUMP_TABLE_ELEMS < P * Z  # sampled
    # the timed steps ran: every node has a previous reading and a power, processes were attributed
    assert np.all(arrays["node_has_prev"] == 1) and np.all(arrays["node_power"] > 0)
    assert np.count_nonzero(arrays["proc_energy"]) > 0 and np.count_nonzero(arrays["cluster_ns_energy"]) > 0
    # the cluster node totals of the last step are the sums of the node tables it left:
    # [2Z] = Σ ActiveEnergyTotal, Σ IdleEnergyTotal (integers far below 2^53: exact in float64)
    want = np.r_[arrays["node_active_total"].reshape(N, Z).sum(axis=0),
                 arrays["node_idle_total"].reshape(N, Z).sum(axis=0)]
    assert np.array_equal(arrays["cluster_node_energy"], want)


def test_dump_outputs_same_with_full(plain, full):
    a, b = _arrays(plain[1]), _arrays(full[1])
    assert sorted(a) == sorted(b)
    for n in a:
        assert np.array_equal(a[n], b[n], equal_nan=True), n
