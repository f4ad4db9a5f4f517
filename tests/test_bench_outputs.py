"""bench.py's plain run and its --dump-outputs files: what a plain run leaves out (--full), the layout and
size bound of the dumped arrays, and on the GPU one small C4 run end to end."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _parse(argv):
    old = sys.argv
    try:
        sys.argv = ["bench.py"] + argv
        return bench.parse()
    finally:
        sys.argv = old


def test_full_and_dump_outputs_are_off_by_default():
    a = _parse(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 3
    a = _parse(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_writes_float64_arrays(tmp_path):
    rng = np.random.default_rng(1)
    st, cnt = rng.standard_normal((37, 90)), np.arange(37, dtype=np.int32)
    bench.dump_outputs(str(tmp_path / "o"), {"state": st, "hl_counter": cnt})
    assert sorted(os.listdir(tmp_path / "o")) == ["hl_counter.npy", "state.npy"]
    s, c = np.load(tmp_path / "o" / "state.npy"), np.load(tmp_path / "o" / "hl_counter.npy")
    assert s.dtype == np.float64 and c.dtype == np.float64
    assert np.array_equal(s, st) and np.array_equal(c, cnt)
    bench.dump_outputs(str(tmp_path / "o"), {"state": st}, rank=1, world=2)
    assert os.path.exists(tmp_path / "o" / "state_rank1.npy")


def test_dump_outputs_samples_beyond_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 10_000)
    st = np.arange(500 * 6, dtype=np.float64).reshape(500, 6)
    it = np.arange(500, dtype=np.int32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"state": st, "iters": it})
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["iters.npy", "sample_index.npy", "state.npy"]
    arrays = {f: np.load(tmp_path / "a" / f) for f in files}
    assert sum(a.nbytes for a in arrays.values()) <= 10_000
    idx = arrays["sample_index.npy"].astype(int)
    assert len(idx) == 10_000 // (6 * 8 + 8 + 8) and np.all(np.diff(idx) > 0)  # the same rows of every array
    assert np.array_equal(arrays["state.npy"], st[idx]) and np.array_equal(arrays["iters.npy"], it[idx])
    for f in files:  # a fixed sample: the same rows in every run
        assert np.array_equal(arrays[f], np.load(tmp_path / "b" / f))


@pytest.mark.gpu
def test_gpu_plain_bench_dumps_the_last_steps_states(tmp_path):
    """A plain C4 run (96 scenarios in 4 forests on 4 sub-batch streams, 2 + 3 steps): one result line with
    ms_per_step and no --full legs; the dumped states are bit for bit those of an engine driven over the same
    seeded inputs for warmup + steps HL periods (a scenario's arithmetic does not depend on the others')."""
    from distributed_aerial_transportation_amd import BatchedController, scenarios

    B, n, warm, steps, nf = 96, 6, 2, 3, 4
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                        str(warm), "--batch", str(B), "--forests", str(nf), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["ms_per_step"] > 0 and d["dtype"] == "f64" and d["higher_is_better"] is True
    assert d["stats"]["agent_qp_solves"] >= steps * B * n  # at least one ADMM pass of every scenario and step
    assert "cpu_baseline" not in d and d["stats"]["sustained"] is None and d["stats"]["mean_admm_iters"] is None
    st, cnt = np.load(out / "state.npy"), np.load(out / "hl_counter.npy")
    assert st.dtype == np.float64 and st.shape == (B, 12 * n + 18) and cnt.shape == (B,)
    scen_forest, states, forests = bench.bench_states(n, B, 0, 1, nf, "path", None)
    eng = BatchedController("cadmm", n, B, scenarios.params_block(n))
    eng.set_forests(forests, scen_forest)
    eng.set_state(states, np.zeros(B, dtype=np.int32))
    eng.set_sub_batches(bench.auto_sub_batches(B))
    eng.closed_loop(warm)
    eng.closed_loop(steps)
    st_ref, cnt_ref = eng.get_state()
    eng.close()
    assert np.all(np.isfinite(st))
    assert np.array_equal(st, st_ref) and np.array_equal(cnt, cnt_ref)
