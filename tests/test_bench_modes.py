"""bench.py's two modes: a plain run prints the headline alone (set up, warm up, time the steps, print), --full adds the legs beyond
it (per-kernel roofline taps, sustained, end to end, serving, other shapes, CPU baseline); --full --quick keeps the roofline only."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup")
FULL_ONLY = ("roofline", "roofline_other_kernels", "sustained", "end_to_end", "serving", "throughput_mode", "other_shapes",
             "refine_384", "pseudo_masks", "cpu_baseline")


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(REPO, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _run(args, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + args, env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


def _kern(name, avg_us, total_ms, overhead_us=3.0):
    return name, {"launches_per_forward": 1.0, "avg_launch_us": avg_us, "total_ms_per_forward": total_ms,
                  "event_overhead_us": overhead_us, "flops_per_launch": 1e9, "bytes_per_launch": 1e6,
                  "achieved_tflops": 200.0, "achieved_gbs": 1000.0}


def test_full_roofline_fields_from_the_taps():
    b = _bench_module()
    kern = dict([_kern("gemm_w16m16_kernel<256, 256>", 80.0, 1.0), _kern("layernorm_kernel", 5.0, 0.1)])
    r = b.headline_roofline(kern, "w16", 300.0)
    assert list(r) == ["roofline", "roofline_other_kernels"]
    roof = r["roofline"]
    assert roof["kernel"] == "gemm_w16m16_kernel<256, 256>" and roof["bound"] == "mfma" and roof["achieved"] == 200.0
    assert "traffic" in roof and roof["traffic_source"]
    assert roof["whole_step"]["achieved"] == 300.0 and roof["whole_step"]["peak"] == b.F16_MFMA_PEAK_TFLOPS
    assert roof["whole_step"]["frac"] == round(300.0 / b.F16_MFMA_PEAK_TFLOPS, 4)
    assert roof["whole_step"]["mfma_issued_tflops"] == 900.0  # w16: three MFMAs per product
    assert list(r["roofline_other_kernels"]) == ["layernorm_kernel"]
    # a launch under three event-pair overheads gets no rate
    assert r["roofline_other_kernels"]["layernorm_kernel"]["achieved"] is None
    assert b.headline_roofline(kern, "fp32", 10.0)["roofline"]["whole_step"]["mfma_issued_tflops"] == 10.0


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_full_quick_adds_the_roofline():
    args = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "8"]
    plain = _run(args)
    full = _run(args + ["--full", "--quick"])
    for res in (plain, full):
        for k in CONTRACT:
            assert k in res, k
        assert res["value"] > 0 and res["ms_per_step"] > 0 and res["unit"] == "images/sec" and res["higher_is_better"] is True
        assert res["steps"] == 2 and res["warmup"] == 1 and res["n_gpus"] == 1
    assert not set(plain) & set(FULL_ONLY), sorted(set(plain) & set(FULL_ONLY))
    assert full["roofline"]["kernel"] and full["roofline"]["launches_per_forward"] > 0 and full["roofline_other_kernels"]
    assert full["sustained"] is None and full["end_to_end"] is None  # --quick: the roofline only
    assert not set(full) & {"serving", "throughput_mode", "other_shapes", "refine_384", "pseudo_masks", "cpu_baseline"}
