"""Cost of the encoder taps -> profiles/encoder_taps_bench.log.

Steps, each a child process of its own under its own time limit (a step that fails or runs out of time ends the run):
  model    ViT-S/16 at 224^2, w16, attention_path "auto", batch 1 and batch 64; device events around one call, 3 warm-up and 30 timed
           repetitions, the sides alternating in one process: forward(x) against forward(x, return_layers=range(12)) (the cost of all
           twelve taps), forward(encoder_only=True) against encoder_layers(x, [5]) (the early stop), and twelve
           get_last_selfattention(x) calls' worth against one forward_selfattention(x, return_interm_attn=True).
  kernel   the token tap kernel inside a batch-64 encoder_layers(x) call, by the library's own timing taps (an event pair around each
           launch, the empty pair's time subtracted): bytes read + written over time, against the 6.3 TB/s a streaming kernel
           achieves on this device's HBM (8 TB/s peak).

    python scripts/encoder_taps_bench.py            # all steps, tee'd into profiles/encoder_taps_bench.log
    python scripts/encoder_taps_bench.py --step kernel
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "salient-object-detection_amd"))
STEPS = {"model": 400, "kernel": 180}  # seconds
WARMUP, REPS = 3, 30
HBM_ACHIEVABLE = 6.3e12  # bytes/s


def _stats(ms):
    import numpy as np
    ms = np.asarray(ms)
    return f"min {ms.min():8.3f}  median {np.median(ms):8.3f}  max {ms.max():8.3f} ms ({len(ms)} reps)"


def _time_sides(sides):
    """Alternate the sides, one device-event pair around each call; returns name -> list of ms."""
    import torch
    ms = {k: [] for k in sides}
    for rep in range(WARMUP + REPS):
        for k, fn in sides.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= WARMUP:
                ms[k].append(e0.elapsed_time(e1))
    return ms


def _model():
    from selfmask_amd import MaskFormer, synthetic_state_dict
    m = MaskFormer(n_queries=20, patch_size=16, n_decoder_layers=6, return_intermediate=True, use_binary_classifier=True, gemm_mode="w16")
    m.load_state_dict(synthetic_state_dict(4, "calib", patch_size=16), strict=True)
    return m.to("cuda:0")


def step_model():
    import torch
    from selfmask_amd import synthetic_images
    m = _model()
    for B in (1, 64):
        x = torch.from_numpy(synthetic_images(11, (B, 3, 224, 224))).to("cuda:0")
        mb = B * 12 * 197 * 384 * 4 / 1e6

        def twelve_last():
            for _ in range(12):
                m.get_last_selfattention(x)

        sides = {
            "forward(x)": lambda: m(x),
            f"forward(x, return_layers=range(12))  [{mb:.1f} MB]": lambda: m(x, return_layers=range(12)),
            "forward(x, encoder_only=True)": lambda: m(x, encoder_only=True),
            "encoder_layers(x, [5])": lambda: m.encoder_layers(x, [5]),
            "encoder_layers(x)": lambda: m.encoder_layers(x),
            "12 x get_last_selfattention(x)": twelve_last,
            "forward_selfattention(x, return_interm_attn=True)": lambda: m.encoder.forward_selfattention(x, return_interm_attn=True),
        }
        print(f"ViT-S/16 224^2, batch {B}, w16, attention_path = 'auto', device events around one call:")
        for k, v in _time_sides(sides).items():
            print(f"  {k:52s} {_stats(v)}", flush=True)


def step_kernel():
    import torch
    from selfmask_amd import _native as N, synthetic_images
    m, lib = _model(), N.load()
    B = 64
    x = torch.from_numpy(synthetic_images(11, (B, 3, 224, 224))).to("cuda:0")
    for _ in range(WARMUP):
        m.encoder_layers(x)
    torch.cuda.synchronize()
    lib.sm_forward_timing(1)
    for _ in range(REPS):
        m.encoder_layers(x)
    torch.cuda.synchronize()
    rows = (N.KernelTime * 64)()
    n = lib.sm_forward_timing_read(rows, 64)
    lib.sm_forward_timing(0)
    assert n > 0, "no timing taps read"
    print(f"token tap kernel inside encoder_layers(x), batch {B} (12 launches per call, {REPS} calls, timing taps):")
    for r in list(rows)[:n]:
        name = r.name.decode()
        if name.startswith("encoder_tap"):
            us, byts = r.total_us / r.launches, r.bytes / r.launches
            print(f"  {name}: {r.launches} launches, mean {us:.2f} us each (empty event pair {r.overhead_us:.2f} us subtracted), "
                  f"{byts / 1e6:.1f} MB read + written each -> {byts / (us * 1e-6) / 1e12:.2f} TB/s, "
                  f"{100 * byts / (us * 1e-6) / HBM_ACHIEVABLE:.0f} % of the {HBM_ACHIEVABLE / 1e12:.1f} TB/s achievable on HBM", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS), default=None)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "encoder_taps_bench.log"))
    args = ap.parse_args()
    if args.step:
        {"model": step_model, "kernel": step_kernel}[args.step]()
        return 0
    with open(args.log, "w") as log:
        for step, limit in STEPS.items():
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step], timeout=limit, capture_output=True, text=True)
            except subprocess.TimeoutExpired:
                log.write(f"[{step}] ran out of its {limit} s\n")
                print(f"[{step}] ran out of its {limit} s")
                return 124
            log.write(p.stdout)
            print(p.stdout, end="")
            if p.returncode != 0:
                log.write(f"[{step}] failed with status {p.returncode}\n{p.stderr[-2000:]}\n")
                print(p.stderr[-2000:])
                return p.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
