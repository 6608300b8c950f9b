"""bench.py --dump-outputs: what the last timed step computed, as float32 .npy files of at most 64 MB in all, from inputs that are
the same on every run (so two builds can be compared output for output); and --steps is the number of timed steps."""
import gc
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(REPO, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _run(args, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    return subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + args, env=env, capture_output=True, text=True,
                          timeout=timeout)


def test_small_arrays_are_written_whole_as_float32(tmp_path):
    b = _bench_module()
    rng = np.random.Generator(np.random.PCG64(3))
    arrays = {"rows": rng.random((8, 16), dtype=np.float32), "ids": np.arange(12, dtype=np.int64).reshape(3, 4)}
    info = b.dump_outputs(arrays, str(tmp_path / "d"))
    for name, v in arrays.items():
        got = np.load(tmp_path / "d" / f"{name}.npy")
        assert got.dtype == np.float32 and got.shape == v.shape
        assert np.array_equal(got, v.astype(np.float32))
        assert info[name] == {"shape": list(v.shape), "saved_elements": v.size, "sampled": False}


def test_large_arrays_are_sampled_within_the_budget_the_same_way_every_time(tmp_path):
    b = _bench_module()
    budget = 64 << 10
    big = np.arange(40000, dtype=np.float32).reshape(200, 200)
    arrays = {"big": big, "small": np.ones((4, 4), np.float32)}
    info = b.dump_outputs(arrays, str(tmp_path / "a"), budget=budget)
    b.dump_outputs(arrays, str(tmp_path / "b"), budget=budget)
    sizes = [os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")]
    assert sum(sizes) <= budget
    assert info["big"]["sampled"] and info["big"]["shape"] == [200, 200]
    a1, a2 = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a1.size == info["big"]["saved_elements"] and np.array_equal(a1, a2)
    # the sample is of the flattened elements, in index order (here value == index)
    assert np.all(np.diff(a1) > 0) and np.array_equal(a1, np.unique(a1))


def test_steps_below_one_are_refused():
    r = _run(["--gpus", "1", "--steps", "0", "--warmup", "1"])
    assert r.returncode != 0 and "--steps" in r.stderr


@pytest.mark.gpu
def test_dump_is_the_last_timed_step(tmp_path):
    B = 8
    outs = {}
    for steps in (2, 3):
        d = tmp_path / f"s{steps}"
        r = _run(["--gpus", "1", "--steps", str(steps), "--warmup", "1", "--batch", str(B), "--quick", "--dump-outputs", str(d)])
        assert r.returncode == 0, r.stderr[-3000:]
        res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert res["steps"] == steps and res["dump_outputs"]["dir"] == str(d)
        outs[steps] = {n: np.load(d / f"{n}.npy") for n in ("rows", "mask_pred", "objectness", "features")}
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64 << 20
    o = outs[3]
    assert o["rows"].shape == (B, 16) and o["mask_pred"].shape == (B, 6, 20, 28, 28) and o["objectness"].shape == (B, 6, 20, 1)
    for v in o.values():
        assert v.dtype == np.float32 and np.isfinite(v).all()
    for n in o:  # the same inputs every step and every run
        assert np.array_equal(outs[2][n], o[n]), n
    # the same step in this process: forward + evaluator post-processing on the same seeded inputs
    import torch
    b = _bench_module()
    wl = b.Workload(torch.device("cuda", 0), 16, 224, B, graph=False)
    try:
        wl.keep_last = True
        rows = wl.step().cpu().numpy()
        torch.cuda.synchronize()
        got = {n: wl.last_out[n].cpu().numpy() for n in ("mask_pred", "objectness", "features")}
    finally:
        del wl
        gc.collect()  # the workload's graph cache holds a reference cycle: free its HIP objects here, not in a later test
    np.testing.assert_allclose(o["rows"], rows, rtol=1e-6, atol=1e-6)
    for n, v in got.items():
        np.testing.assert_allclose(o[n], v, rtol=1e-6, atol=1e-6, err_msg=n)
