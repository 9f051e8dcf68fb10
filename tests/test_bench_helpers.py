"""CPU checks of bench.py's host-side helpers: the benchmark lattice, the stratified parity sample, the per-launch statistics the bench line
carries since round 6, the command-line defaults the driver relies on, and the sample --dump-outputs writes; one GPU run of a plain bench.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def test_lattice_is_a_permutation_of_the_32_x_32_x_1024_grid():
    b = _bench()
    EAS, h, psi, cell = b.lattice(0)
    assert EAS.size == 1 << 20 and EAS.min() == 35.0 and EAS.max() == 55.0 and h.min() == 200.0 and h.max() == 3000.0
    assert np.unique(cell).size == 1024 and np.bincount(cell).min() == 1024 and np.bincount(cell).max() == 1024     # every (EAS, h) cell 1024 times
    key = (cell.astype(np.int64) << 10) | np.round((psi + np.pi) / (2 * np.pi) * 1024).astype(np.int64)
    assert np.unique(key).size == 1 << 20                                                                        # every lattice point exactly once
    assert (np.diff(cell[:64]) != 0).any(), "neighbouring lanes sit in different table cells"
    EAS1 = b.lattice(1)[0]
    assert not np.array_equal(EAS, EAS1) and np.array_equal(np.sort(EAS), np.sort(EAS1))                          # another rank: the same points, another order


def test_stratified_sample_covers_every_cell():
    b = _bench()
    cell = b.lattice(0)[3]
    sel = b.stratified_sample(cell)
    assert sel.size == 4096 and np.unique(sel).size == 4096 and np.all(np.diff(sel) > 0)
    assert np.unique(cell[sel]).size == 1024 and np.bincount(cell[sel]).min() == 4
    assert sel.max() > (1 << 20) * 0.99 and sel.min() < (1 << 20) * 0.01                                          # drawn over the whole permuted order


def test_launch_stats_reports_the_median_and_keeps_every_launch():
    b = _bench()
    ms = [10.9, 10.1, 9.85, 9.84, 9.86, 40.0, 9.83]          # a ramp behind the trim and one stalled launch
    s = b.launch_stats(ms)
    assert s["kernel_ms"] == 9.86 and s["kernel_ms_min"] == 9.83 and s["kernel_ms_max"] == 40.0 and s["launches_timed"] == 7
    assert s["kernel_ms_per_launch"] == ms
    assert abs(np.mean(ms) - s["kernel_ms"]) > 4.0, "what the median is for: one stall moves the mean by 4 ms and the median not at all"


def test_command_line_defaults():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True).stdout
    assert "--gpus" in out and "--steps" in out and "--warmup" in out and "strong (default)" in out
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert 'scaling = args.scaling or "strong"' in src and 'PROFILE_COUNTERS = "r06_counters.json"' in src


def test_full_and_dump_outputs_options():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True).stdout
    assert "--full" in out and "--dump-outputs DIR" in out


def test_output_sample_is_fixed_and_within_64_mb(fb):
    b = _bench()
    sel = b.output_sample(b.N_TOTAL)
    assert np.array_equal(sel, b.output_sample(b.N_TOTAL)), "the same aircraft on every run"
    assert sel.size == b.OUTPUT_SAMPLE and np.unique(sel).size == sel.size and np.all(np.diff(sel) > 0)
    assert sel.min() < b.N_TOTAL * 0.01 and sel.max() > b.N_TOTAL * 0.99
    assert np.array_equal(b.output_sample(1000), np.arange(1000))
    rows = fb.K["FB_NX"] + fb.K["FB_NS"] + 2                          # x, s, status, index
    assert rows * 8 * sel.size <= 64 << 20


def test_sample_outputs_and_write_outputs(tmp_path):
    b = _bench()
    n, sel = 50, np.array([3, 7, 41])
    x = np.random.default_rng(0).normal(size=(27, n))
    s = np.arange(2 * n, dtype=np.int32).reshape(2, n)
    st = (np.arange(n) % 3).astype(np.int32)
    o = b.sample_outputs(x, s, st, sel)
    b.write_outputs(str(tmp_path / "out"), o)
    got = {f[:-4]: np.load(tmp_path / "out" / f) for f in os.listdir(tmp_path / "out")}
    assert sorted(got) == ["index", "s", "status", "x"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["x"], x[:, sel]) and np.array_equal(got["s"], s[:, sel])
    assert np.array_equal(got["status"], st[sel]) and np.array_equal(got["index"], sel)


@pytest.mark.gpu
def test_plain_run_times_the_steps_asked_for_and_dumps_its_outputs(tmp_path, fb):
    """the headline only: --steps timed launches, ms_per_step on the line, no --full legs; the outputs of the last step on disk — the
    sampled aircraft flown again here through the same 1 warm-up + 3 timed launches land where the dump says, one launch beyond 3"""
    d = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(d)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["roofline"]["launches_timed"] == 3 and line["roofline"]["kernel_ms"] > 0 and line["ms_per_step"] >= line["roofline"]["kernel_ms_min"]
    assert line["value"] > 0 and line["unit"] == "aircraft-steps/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert "cpu_baseline" not in line and "rel_err_vs_cpu" not in line and "extra" not in line
    b = _bench()
    x, s, st, idx = (np.load(d / f"{k}.npy") for k in ("x", "s", "status", "index"))
    assert x.shape == (27, b.OUTPUT_SAMPLE) and s.shape == (2, b.OUTPUT_SAMPLE) and sorted(os.listdir(d)) == ["index.npy", "s.npy", "status.npy", "x.npy"]
    assert np.array_equal(idx, b.output_sample(b.N_TOTAL)) and (st == 0).all() and np.isfinite(x).all()
    assert sum(f.stat().st_size for f in d.iterdir()) <= 64 << 20
    sel = idx.astype(np.int64)
    EAS, h, psi, _ = b.lattice(0)
    w = fb.BatchedWorld(sel.size)
    fb.f_init(w, fb.TrimParameters(EAS=EAS[sel], h_e=h[sel], ψ_nb=psi[sel]))
    sim = fb.Simulation(w, dt=b.DT, save_on=False, steps_per_launch=50)
    for _ in range(3):
        fb.step(sim, 50 * b.DT)
    w.sync()
    x3 = w.x
    fb.step(sim, 50 * b.DT)
    w.sync()
    x4 = w.x
    w.close()
    assert (x[8] < x3[8]).all(), "fuel after the last timed launch is below what it is one launch earlier"
    assert b.scaled_error(x, x4).max() < 1e-9, "the dump is the state after warm-up + timed launches"
