#!/usr/bin/env python3
"""ResNet-50 backbone (selfmask_amd.ResNet50, csrc/conv.hip) at 224 x 224 -> profiles/resnet_bench.log.

    python scripts/resnet_bench.py [--log profiles/resnet_bench.log] [--dilated 1]

Steps, each a child process under its own time limit (a step that fails or runs out of time ends the run):
  hip     images/s of ``ResNet50.forward`` at batch 1 and 32: device events around each forward, the median of REPS after WARMUP with
          the min - max range; then ONE forward per batch size under the library's own taps (sm_forward_timing: an event pair per
          launch), summed by launch name, with the gathers' share of the tapped time.  The taps serialise nothing (one stream) but
          their sum excludes the gaps between launches, so it is below the forward's time.
  torch   the same network as tests/_resnet_ref.py's layer table through torch.nn.functional on the device - PyTorch-ROCm's own
          convolutions in fp32 - timed the same way in the same job, and its distance from the HIP maps (same weights and input).
Weights and inputs are synthetic (tests/_resnet_cases.py).  Nothing here gates anything: the figures size the implicit-GEMM follow-up.
"""
import argparse
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "salient-object-detection_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

WARMUP, REPS = 5, 30
BATCHES = (1, 32)
SIZE = 224
STEP_LIMIT_S = {"hip": 240, "torch": 360}


def _timed(fn, torch):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def _setup(dilated):
    import torch
    import _resnet_cases as RC
    from selfmask_amd import ResNet50
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    sd = RC.synthetic_resnet_state_dict(11, dilated)
    m = ResNet50(use_dilated_resnet=dilated)
    m.load_state_dict(sd, strict=True)
    return torch, RC, sd, m.to("cuda:0")


def step_hip(dilated):
    torch, RC, _sd, m = _setup(dilated)
    from selfmask_amd import _native as N
    lib = N.load()
    for B in BATCHES:
        x = RC.synthetic_input(200 + B, (B, 3, SIZE, SIZE)).to("cuda:0")
        med, lo, hi = _timed(lambda: m(x), torch)
        print(f"hip   B={B:<3d} forward {med:8.3f} ms (min {lo:.3f} - max {hi:.3f}, median of {REPS}) = {B / med * 1e3:9.1f} images/s", flush=True)
        N.check(lib.sm_forward_timing(1), "sm_forward_timing")
        try:
            m(x)
            buf = (N.KernelTime * 64)()
            n = lib.sm_forward_timing_read(buf, 64)
        finally:
            lib.sm_forward_timing(0)
        assert n > 0, lib.sm_last_error()
        rows = sorted(((buf[k].name.decode(), buf[k].launches, buf[k].total_us, buf[k].flops) for k in range(n)), key=lambda r: -r[2])
        total = sum(r[2] for r in rows)
        for name, launches, us, flops in rows:
            rate = f"{flops / us / 1e6:7.1f} TFLOP/s" if flops > 0 and us > 0 else ""
            print(f"      B={B:<3d} {name:<28s} {launches:3d} launches {us:9.1f} us {100 * us / total:5.1f} % {rate}")
        g = sum(r[2] for r in rows if "gather" in r[0])
        print(f"      B={B:<3d} tapped total {total:.1f} us; gathers {g:.1f} us = {100 * g / total:.1f} % of it", flush=True)


def step_torch(dilated):
    torch, RC, sd, m = _setup(dilated)
    import _resnet_ref as RR
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    prepared = RR.prepare(sd, torch.device("cuda:0"), torch.float32)
    for B in BATCHES:
        x = RC.synthetic_input(200 + B, (B, 3, SIZE, SIZE)).to("cuda:0")
        t0 = time.time()
        ref = RR.forward(prepared, x, dilated, torch.float32, prefix=None)
        torch.cuda.synchronize()
        first = time.time() - t0
        med, lo, hi = _timed(lambda: RR.forward(prepared, x, dilated, torch.float32, prefix=None), torch)
        print(f"torch B={B:<3d} forward {med:8.3f} ms (min {lo:.3f} - max {hi:.3f}, median of {REPS}) = {B / med * 1e3:9.1f} images/s "
              f"(first call {first:.1f} s)", flush=True)
        hmed, hlo, hhi = _timed(lambda: m(x), torch)
        print(f"hip   B={B:<3d} forward {hmed:8.3f} ms (min {hlo:.3f} - max {hhi:.3f}) in the same process: hip / torch time = {hmed / med:.2f}")
        d = [(a - b).abs().max().item() for a, b in zip(m(x), ref)]
        print(f"      B={B:<3d} max |hip - torch fp32| per map: " + ", ".join(f"{v:.2e}" for v in d), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=("hip", "torch"))
    ap.add_argument("--dilated", type=int, default=1)
    ap.add_argument("--log")
    a = ap.parse_args()
    if a.step:
        return {"hip": step_hip, "torch": step_torch}[a.step](bool(a.dilated))
    out = [f"# scripts/resnet_bench.py: ResNet50(use_dilated_resnet={bool(a.dilated)}) at {SIZE} x {SIZE}, batches {BATCHES}, warm-up {WARMUP}, "
           f"median of {REPS}"]
    rc, shown = 0, 0
    for step in ("hip", "torch"):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--dilated", str(a.dilated)], capture_output=True,
                               text=True, timeout=STEP_LIMIT_S[step])
            out.append(r.stdout.rstrip())
            rc = r.returncode
            if rc:
                out.append(f"step {step} failed (exit {rc}): {r.stderr.strip()[-600:]}")
        except subprocess.TimeoutExpired as e:
            out.append(((e.stdout or b"").decode() if isinstance(e.stdout, bytes) else (e.stdout or "")).rstrip())
            out.append(f"step {step}: not measured (ran out of its {STEP_LIMIT_S[step]} s)")
            rc = 124
        print("\n".join(out[shown:]), flush=True)
        shown = len(out)
        if rc:
            break
    text = "\n".join(out) + "\n"
    if a.log:
        with open(a.log, "w") as f:
            f.write(text)
    return rc


if __name__ == "__main__":
    sys.exit(main())
