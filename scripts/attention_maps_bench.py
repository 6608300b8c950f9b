"""Cost of the last block's attention maps -> profiles/attention_maps_bench.log.

Steps, each a child process of its own under its own time limit (a step that fails or runs out of time ends the run):
  model    ViT-S/16 at 224^2, batch 64, w16, attn_path pinned ("fused"), device events around one call, 3 warm-up and 30 timed
           repetitions, the sides alternating in one process: forward(encoder_only=True) - which runs exactly what it ran before the
           attention outputs existed -, get_last_selfattention(cls_only=True), get_last_selfattention() (59.6 MB written), and a full
           forward with and without return_attention="cls".
  kernel   sm_attention_probs_f16x2 alone on random F16X2 operands at 197 tokens: batch 64 and batch 1, all rows and the CLS row
           alone; for the full matrix the achieved write bandwidth (bytes of P / time).

    python scripts/attention_maps_bench.py            # all steps, tee'd into profiles/attention_maps_bench.log
    python scripts/attention_maps_bench.py --step kernel
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "salient-object-detection_amd"))
STEPS = {"model": 300, "kernel": 180}  # seconds
WARMUP, REPS = 3, 30


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


def step_model():
    import torch
    from selfmask_amd import MaskFormer, synthetic_images, synthetic_state_dict
    dev = "cuda:0"
    m = MaskFormer(n_queries=20, patch_size=16, n_decoder_layers=6, return_intermediate=True, use_binary_classifier=True, gemm_mode="w16")
    m.load_state_dict(synthetic_state_dict(4, "calib", patch_size=16), strict=True)
    m = m.to(dev)
    m.attention_path = "fused"
    x = torch.from_numpy(synthetic_images(11, (64, 3, 224, 224))).to(dev)
    sides = {
        "forward(encoder_only=True)": lambda: m(x, encoder_only=True),
        "get_last_selfattention(cls_only=True)": lambda: m.get_last_selfattention(x, cls_only=True),
        "get_last_selfattention()  [59.6 MB]": lambda: m.get_last_selfattention(x),
        "forward(x)": lambda: m(x),
        "forward(x, return_attention='cls')": lambda: m(x, return_attention="cls"),
    }
    print("ViT-S/16 224^2, batch 64, w16, attention_path = 'fused', device events around one call:")
    for k, v in _time_sides(sides).items():
        print(f"  {k:40s} {_stats(v)}", flush=True)


def step_kernel():
    import torch
    from selfmask_amd import _native as N, ops
    dev = "cuda:0"
    lib = N.load()
    n = 197
    print("sm_attention_probs_f16x2 alone, 197 tokens, 6 heads, random unit-variance F16X2 operands (Q|K rows of 768):")
    for B in (64, 1):
        qk = ops.split_f16x2(torch.randn(B * n, 768, device=dev))
        full = torch.empty((B, 6, n, n), device=dev)
        cls = torch.empty((B, 6, n), device=dev)

        def launch(out, nq):
            a = N.AttnProbsArgs()
            a.Q, a.K, a.P = qk.data_ptr(), qk.data_ptr() + 384 * 4, out.data_ptr()
            a.sQb = a.sKb = n * 768
            a.sQr = a.sKr = 768
            a.batch, a.heads, a.n_q, a.n_k, a.q0, a.nq, a.scale = B, 6, n, n, 0, nq, 0.125
            N.check(lib.sm_attention_probs_f16x2(a, torch.cuda.current_stream().cuda_stream), "sm_attention_probs_f16x2")

        ms = _time_sides({"all rows": lambda: launch(full, n), "CLS row": lambda: launch(cls, 1)})
        import numpy as np
        med = float(np.median(ms["all rows"]))
        print(f"  batch {B:2d}  all rows  {_stats(ms['all rows'])}   {full.numel() * 4 / 1e6:6.2f} MB of P -> "
              f"{full.numel() * 4 / (med * 1e-3) / 1e9:7.1f} GB/s written (median)")
        print(f"  batch {B:2d}  CLS row   {_stats(ms['CLS row'])}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS), default=None)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "attention_maps_bench.log"))
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
